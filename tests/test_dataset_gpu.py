"""-m gpu: the frame-preparation kernels of muvo_amd/csrc/dataset.hip, `input_pipeline.prepare_frames` and the batch iterator
of muvo_amd/data/dataset.py.  Every kernel against the numpy restatement (tests/dataset_reference.py) element by element and
against the digests the REAL reference wrote (tests/golden/dataset.json): the bar is zero differing elements.  The raw frames
come from muvo_amd/data/recording_inputs.py directly; only the end-to-end test reads files (pandas, PIL).

Every test runs under a watchdog of its own (`bounded`): when it expires the process is ended with a traceback, so nothing
more is started on the GPU.  The component kernel does not lean on it: each of its loops has a stated bound."""
import faulthandler
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dataset_reference as DR  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def bounded(seconds):
    def deco(fn):
        @functools.wraps(fn)
        def run(*a, **k):
            faulthandler.dump_traceback_later(seconds, exit=True)
            try:
                return fn(*a, **k)
            finally:
                faulthandler.cancel_dump_traceback_later()
        return run
    return deco


def _np(t):
    return t.cpu().numpy()


def _differing(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == 'f':                       # bit patterns, so that -0.0 / NaN cannot hide a difference
        bits = np.dtype(f'u{got.dtype.itemsize}')
        got, want = np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)
    return int((got != want).sum())


# ---- raw sequences without files ------------------------------------------------------------------------------------------------
def generated_frame(split, run_id, t, cfg):
    """What CarlaDataset.read_frame returns for frame t, from the generator's arrays instead of the files."""
    from muvo_amd.data import recording_inputs as RI
    town, run = run_id.split('/')
    a, row = RI.frame_arrays(split, town, run, t), RI.frame_row(split, town, run, t)
    throttle, steering, brake = row['action']
    out = {'n_classes': row['n_classes'], 'image': a['image'], 'route_map': a['route_map'], 'birdview_int': a['birdview'],
           'points_xyz': a['points_xyz'], 'obj_tag': a['ObjTag'], 'voxel_rows': a['voxel'].astype(np.int64),
           'steering': np.array([steering], dtype=np.float32),
           'throttle_brake': np.array([throttle if throttle > 0 else -brake], dtype=np.float32), 'speed': row['speed'],
           'reward': np.array([row['reward']], dtype=np.float32).clip(-1.0, 1.0),
           'value_function': np.array([row['value']], dtype=np.float32)}
    if cfg.LOSSES.RGB_INSTANCE or cfg.SEMANTIC_IMAGE.ENABLED or cfg.DEPTH.ENABLED:
        out['depth_semantic'] = a['depth_semantic']
    return out


class GeneratedDataset:
    """The part of CarlaDataset a BatchLoader uses, over the fixture's data pointers."""

    def __init__(self, cfg, split, variant):
        from muvo_amd.data.dataset import calculate_geometry_from_config
        meta = json.load(open(os.path.join(GOLD, 'dataset.json')))
        self.cfg, self.split = cfg, split
        self.ref = meta['datasets'][f'{variant}/{split}']
        self.data_pointers = [(r, idx) for r, idx in self.ref['data_pointers']]
        self.intrinsics, self.extrinsics = calculate_geometry_from_config(cfg)
        self.reads = []

    def __len__(self):
        return len(self.data_pointers)

    def read_frame(self, run_id, t):
        self.reads.append((run_id, t))
        return generated_frame(self.split, run_id, t, self.cfg)

    def read_raw(self, i):
        from muvo_amd.data.dataset import stack_frames
        run_id, idx = self.data_pointers[i]
        return stack_frames([self.read_frame(run_id, t) for t in idx], self.intrinsics, self.extrinsics)


def _to_dev(raw, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in raw.items()}


# ---- kernels ---------------------------------------------------------------------------------------------------------------------
@bounded(300)
def test_birdview_decode_frames(dev):
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data import recording_inputs as RI
    bev = np.stack([RI.birdview_frame(RI._frame_key('train', 'Town01', '0000', t), t) for t in range(6)])
    rnd = np.random.RandomState(1).randint(0, 1 << 12, size=(3, 50, 70)).astype(np.int32)
    rnd[0, :5] = 0
    for frames, n in ((bev, RI.N_CLASSES), (rnd, 12), (rnd, 5)):
        planes, label, mask = IP.birdview_decode_frames(torch.from_numpy(frames).to(dev), n)
        assert planes.dtype == torch.float32 and label.dtype == torch.int64 and mask.dtype == torch.uint8
        for f in range(len(frames)):
            p, l, m = DR.birdview_decode(frames[f], n)
            assert _differing(_np(planes[f]), p) == 0 and _differing(_np(label[f]), l[0]) == 0
            assert _differing(_np(mask[f]).astype(bool), m) == 0


def _spiral(H, W):
    """A one-pixel-wide arm winding inwards with one-pixel gaps: a single component whose pixels are far apart along it."""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax])
        if free:
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def _hand_made(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    comb = (xx % 2 == 0) | (yy == H - 1)                      # teeth that only join in the last row: every early label is merged late
    u = np.zeros((H, W), bool)                                # one-pixel-wide U across every tile border it can reach
    u[: H - 1, 1 % W] = u[: H - 1, W - 2] = True
    u[H - 2, 1 % W:W - 1] = True
    snake = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == W - 1)) | ((yy % 4 == 3) & (xx == 0))      # one component, HW/2 long
    return {'empty': np.zeros((H, W), bool), 'full': np.ones((H, W), bool), 'checkerboard': (yy + xx) % 2 == 0, 'comb': comb,
            'u': u, 'snake': snake, 'spiral': _spiral(H, W), 'noise': np.random.RandomState(H * 1000 + W).rand(H, W) < 0.55}


@bounded(600)
@pytest.mark.parametrize('hw', [(192, 192), (45, 77), (64, 96), (33, 31), (1, 100), (100, 1), (1, 1)])
def test_label_components_hand_made(dev, hw):
    from muvo_amd import input_pipeline as IP
    masks = _hand_made(*hw)
    names = sorted(masks)
    got = IP.label_components_frames(torch.from_numpy(np.stack([masks[n] for n in names]).astype(np.uint8)).to(dev))
    assert got.dtype == torch.int32
    got = _np(got)
    for f, name in enumerate(names):
        want = DR.label_components(masks[name])[0]
        assert _differing(got[f], want) == 0, (hw, name, int(got[f].max()), int(want.max()))
    if hw == (192, 192):
        assert int(got[names.index('checkerboard')].max()) == 192 * 192 // 2
        assert int(got[names.index('snake')].max()) == 1 and int(got[names.index('spiral')].max()) >= 1


@bounded(300)
def test_label_components_recording(dev):
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data import recording_inputs as RI
    bev = np.stack([RI.birdview_frame(RI._frame_key('val0', 'Town02', '0000', t), t) for t in range(12)])
    _, _, mask = IP.birdview_decode_frames(torch.from_numpy(bev).to(dev), RI.N_CLASSES)
    got = _np(IP.label_components_frames(mask))
    n = []
    for f in range(len(bev)):
        want = DR.label_components(DR.birdview_decode(bev[f], RI.N_CLASSES)[2])[0]
        assert _differing(got[f], want) == 0, f
        n.append(int(want.max()))
    assert n[4] == 0 and n[9] == 0 and max(n) >= 8
    again = _np(IP.label_components_frames(mask))              # independent of the order of the atomics
    assert _differing(again, got) == 0


@bounded(300)
def test_depth_semantic_decode_frames(dev):
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data.voxelize_inputs import camera_frame
    full = np.stack([camera_frame(key='dataset_gpu_depth0'), camera_frame(key='dataset_gpu_depth1')])
    # every (R, G) pair with hashed B, every tag the remap knows, and the codes around the 0.999 threshold
    yy, xx = np.mgrid[0:256, 0:256]
    grid = np.stack([yy, xx, (yy * 7 + xx * 13) % 256, (yy + xx) % 23], axis=-1).astype(np.uint8)[None]
    edge = 0.999 * (256 ** 3 - 1)
    codes = np.arange(int(edge) - 128, int(edge) + 128)
    grid[0, 0, :, 0], grid[0, 0, :, 1], grid[0, 0, :, 2] = codes >> 16, (codes >> 8) & 255, codes & 255
    for img in (full, grid):
        out = IP.depth_semantic_decode_frames(torch.from_numpy(img).to(dev))
        assert {k: v.dtype for k, v in out.items()} == {'semantic_image': torch.int64, 'image_instance_mask': torch.bool,
                                                        'depth_color': torch.float64, 'depth': torch.float64}
        for f in range(len(img)):
            sem, inst, col, dep = DR.depth_semantic_decode(img[f])
            assert _differing(_np(out['semantic_image'][f]), sem[0]) == 0 and _differing(_np(out['image_instance_mask'][f]), inst[0]) == 0
            assert _differing(_np(out['depth_color'][f]), col) == 0 and _differing(_np(out['depth'][f]), dep[0]) == 0
    d = _np(out['depth'][0, 0])
    assert (d == -1).any() and (d > 0.99).any()                 # both sides of the threshold are hit
    only = IP.depth_semantic_decode_frames(torch.from_numpy(grid).to(dev), semantic=False, instance_mask=True, depth=False)
    assert sorted(only) == ['image_instance_mask'] and torch.equal(only['image_instance_mask'], out['image_instance_mask'])


@bounded(300)
def test_batched_range_and_voxel_equal_per_frame(dev):
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data.lidar_inputs import lidar_case, voxel_case
    from oracle import muvo_ref as R
    sweeps = [lidar_case(P=p, key=f'dataset_gpu_lidar{i}') for i, p in enumerate((60000, 200, 20000, 33300))] + \
             [(np.zeros((0, 3), np.float32), np.zeros(0, np.uint8))]
    sweeps[1] = (sweeps[1][0][-1:], sweeps[1][1][-1:])          # a sweep of one point
    rows = [voxel_case(Q=q, key=f'dataset_gpu_voxel{i}') for i, q in enumerate((400000, 30000, 7))] + [np.zeros((0, 4), np.int64)]
    from muvo_amd.data.dataset import _pad_stack
    pts, npt = _pad_stack([s[0] for s in sweeps], np.float32)
    tag, _ = _pad_stack([s[1] for s in sweeps], np.uint8)
    pts[1, 1:] = 7.0                                            # padding is never read, whatever it holds
    xyzd, seg = IP.range_projection_frames(torch.from_numpy(pts).to(dev), torch.from_numpy(tag).to(dev), torch.from_numpy(npt).to(dev))
    assert seg.dtype == torch.int64
    for f, (p, t) in enumerate(sweeps):
        rx, rs = R.range_projection(p, t)
        if len(p):                                              # (the per-frame entry point refuses an empty sweep)
            one_x, one_s = IP.range_projection(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev))
            assert _differing(_np(xyzd[f]), _np(one_x)) == 0 and _differing(_np(seg[f]), _np(one_s).astype(np.int64)) == 0
        assert _differing(_np(xyzd[f]), rx) == 0 and _differing(_np(seg[f]), rs.astype(np.int64)) == 0
    x2, none = IP.range_projection_frames(torch.from_numpy(pts).to(dev), torch.from_numpy(tag).to(dev), torch.from_numpy(npt).to(dev),
                                          with_seg=False)
    assert none is None and torch.equal(x2, xyzd)
    vr, nq = _pad_stack(rows, np.int64)
    vr[2, 7:] = 5
    vox = IP.voxel_grid_frames(torch.from_numpy(vr).to(dev), torch.from_numpy(nq).to(dev))
    for f, r in enumerate(rows):
        if len(r):
            assert _differing(_np(vox[f]), _np(IP.voxel_grid(torch.from_numpy(r).to(dev)))) == 0
        assert _differing(_np(vox[f]), R.voxel_grid(r)) == 0


# ---- prepare_frames and the iterator -------------------------------------------------------------------------------------------
@bounded(600)
@pytest.mark.parametrize('variant', ['default', 'heads_on'])
def test_prepare_frames_equals_restatement_and_reference_digests(dev, variant):
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import collate_raw
    cfg = RI.recording_cfg(variant)
    for split in ('train', 'val0'):
        ds = GeneratedDataset(cfg, split, variant)
        items = sorted(int(i) for i in ds.ref['items'])
        raws = [ds.read_raw(i) for i in items]
        batch = IP.prepare_frames(_to_dev(collate_raw(raws), dev), cfg)
        want = DR.prepare_batch(raws, cfg)
        assert sorted(batch) == sorted(want)
        for j, i in enumerate(items):
            ref = ds.ref['items'][str(i)]
            assert sorted(ref) == sorted(batch)
            for k in ref:
                got = _np(batch[k][j])
                assert _differing(got, want[k][j]) == 0, (variant, split, i, k)
                assert DR.digest(got) == ref[k], (variant, split, i, k)


@bounded(600)
@pytest.mark.parametrize('input_stream', [True, False])
def test_iterator_batches_equal_prepare_frames(dev, input_stream):
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import BatchLoader, collate_raw
    cfg = RI.recording_cfg('heads_on')
    ds = GeneratedDataset(cfg, 'train', 'heads_on')
    loader = BatchLoader(ds, 2, dev, seed=11, n_workers=4, input_stream=input_stream)
    loader.set_epoch(1)
    order = loader.batch_indices()
    assert len(order) == 6 and len(loader) == 6
    seen = 0
    for k, batch in enumerate(loader):
        if k in (0, 3, 5):                                      # first, a reused staging slot, last
            want = IP.prepare_frames(_to_dev(collate_raw([ds.read_raw(i) for i in order[k]]), dev), cfg)
            assert sorted(batch) == sorted(want)
            for key in want:
                assert batch[key].device == dev and batch[key].shape[:2] == (2, 2)
                assert torch.equal(batch[key], want[key]), (k, key)
        seen += 1
    assert seen == 6 and len(ds.reads) >= 6 * 2 * 2
    assert (loader._stream is not None) == input_stream
    # a resumed run: the epoch's batches from number 4 on are the last two
    tail = list(loader.iterate(4))
    assert len(tail) == 2 and torch.equal(tail[1]['voxel'], batch['voxel']) and torch.equal(tail[1]['image'], batch['image'])


@bounded(900)
def test_forward_with_aux_and_bev_heads_takes_the_loaders_batch(dev):
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import BatchLoader
    from muvo_amd.trainer import WorldModelTrainer
    cfg = RI.recording_cfg('heads_on', RECEPTIVE_FIELD=2, FUTURE_HORIZON=0, STEPS=100000, BATCHSIZE=1)
    batch = next(iter(BatchLoader(GeneratedDataset(cfg, 'train', 'heads_on'), 1, dev, seed=0, n_workers=2)))
    tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    tr.train()
    losses, _, _, _ = tr.shared_step(batch, mode='train')
    total = tr.loss_reducing(losses)
    names = ' '.join(losses)
    for head in ('bev_segmentation', 'bev_center', 'lidar_seg', 'semantic_image', 'depth'):
        assert head in names, (head, sorted(losses))
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()) and bool(torch.isfinite(total))


@bounded(1200)
def test_fit_from_recording_equals_fit_from_restated_batches(dev, tmp_path, monkeypatch):
    """Two optimizer steps at b1 x s2 in deterministic mode: batches from the iterator (files -> host threads -> kernels) against
    batches the numpy restatement builds from the same files - identical losses in both steps."""
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import ops, train
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    root = str(tmp_path / 'rec')
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 8, True), ('train', 'Town01', '0002', 4, False)))
    monkeypatch.chdir(tmp_path)
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=0, STEPS=2, BATCHSIZE=1, VAL_CHECK_INTERVAL=0, LOGGING_INTERVAL=1)
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        _, hist_loader = train.fit(cfg, dev, log=lambda s: None, dataset_root=root)
        dm = DataModule(cfg, root, device=dev, seed=1234)
        dm.setup()
        loader = dm.train_dataloader()
        per_epoch = len(loader)
        assert len(dm.train_dataset) == 2 and per_epoch == 2 and sorted(sum(loader.batch_indices(0), [])) == [0, 1]
        cache = {}

        def restated(micro):
            # the loop draws ACCUMULATE_GRAD_BATCHES micro-batches per step and runs through the epochs like train_batches()
            idx = tuple(loader.batch_indices(micro // per_epoch)[micro % per_epoch])
            if idx not in cache:
                cache[idx] = DR.prepare_batch([dm.train_dataset.read_raw(i) for i in idx], cfg)
            return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cache[idx].items()}

        _, hist_restated = train.fit(cfg, dev, log=lambda s: None, batch_fn=restated)
    finally:
        ops.set_deterministic(was)
    assert [h['step'] for h in hist_loader] == [h['step'] for h in hist_restated] == [1, 2]
    for a, b in zip(hist_loader, hist_restated):
        assert sorted(a) == sorted(b) and sum(k.startswith('train_') for k in a) >= 10
        for k in a:
            assert a[k] == b[k] and np.isfinite(a[k]), (a['step'], k, a[k], b[k])
    assert hist_loader[0] != hist_loader[1]
