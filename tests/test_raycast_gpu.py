"""-m gpu: the ray-casting kernels (csrc/raycast.hip) against the numpy float32 restatement (tests/raycast_reference.py) bit for
bit - bricks, first hits from class grids and from logits, the shaded tile, the `_voxel` panel through
`WorldModelTrainer.visualise`, the RayIoU counts and metric - and one `predict --mode test --ray-iou --voxel` run."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import raycast_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 171
C9 = 9


def _all_rays(g):
    return np.concatenate([R.scene_rays(), np.array([r for _, r, _ in R.hand_rays(g)], np.float32), np.array([R.CORNER_RAY], np.float32)])


@pytest.fixture(scope='module')
def scenes():
    """{name: (grids (3, X, Y, Z) of different content, rays, [(hit, t, face)] of the restatement per grid)}, computed once"""
    g = R.scene()
    q = R.cube_scene()
    out = {'scene': (np.stack([g, R.corner_scene(), R.shifted(g)]), _all_rays(g)),
           'cube': (np.stack([q, R.shifted(q, 4), np.zeros_like(q)]),
                    np.concatenate([R.camera_rays(8, 8, 8, 12), R.fan_rays((2.5, 4.5, 3.5), 4, 16, 10.0, -30.0)]))}
    return {k: (grids, rays, [R.cast(x, rays) for x in grids]) for k, (grids, rays) in out.items()}


@pytest.mark.parametrize('name', ['scene', 'cube'])
@pytest.mark.parametrize('source', ['grid', 'logits'])
def test_raycast_equals_the_restatement_bit_for_bit(dev, scenes, name, source):
    from muvo_amd import ops
    grids, rays, want = scenes[name]
    if source == 'grid':
        src = torch.from_numpy(grids).to(dev)
    else:
        src = torch.from_numpy(np.stack([R.logits_for(x, C9, seed=3 + i) for i, x in enumerate(grids)])).to(dev)
    cls, bricks = ops.raycast_bricks(src)
    assert cls.dtype == torch.uint8 and np.array_equal(cls.cpu().numpy(), grids)
    words = bricks.cpu().numpy().view(np.uint64)
    assert words.shape == (3, len(R.pack_bricks(grids[0])))
    for f in range(3):
        assert np.array_equal(words[f], R.pack_bricks(grids[f])), f
    hit, t, face = (x.cpu().numpy() for x in ops.raycast(cls, bricks, torch.from_numpy(rays).to(dev)))
    assert hit.shape == t.shape == face.shape == (3, len(rays)) and hit.dtype == np.int32 and t.dtype == np.float32 and face.dtype == np.uint8
    for f in range(3):
        wh, wt, wf = want[f]
        bad = np.flatnonzero((hit[f] != wh) | (face[f] != wf) | (t[f].view(np.int32) != wt.view(np.int32)))
        assert not len(bad), (f, bad[:5], hit[f][bad[:5]], wh[bad[:5]], t[f][bad[:5]], wt[bad[:5]])
    assert (want[0][0] >= 0).sum() > 50 and set(np.unique(np.concatenate([w[2][w[0] >= 0] for w in want])).tolist()) >= {0, 1, 2}


def _palette(dev):
    from muvo_amd.visualise import VOXEL_COLOURS
    pal = R.palette256(VOXEL_COLOURS)
    return pal, torch.from_numpy(pal).to(dev)


def test_panel_voxel_view_tile(dev):
    from muvo_amd import ops
    g = R.scene()
    grids = np.stack([g, R.shifted(g)])
    rays = R.camera_rays(R.X, R.Y, R.Z, R.R)
    pal, dpal = _palette(dev)
    T = R.R + 4
    panel = torch.full((1, 3, T + 5, 2 * T + 9), SENTINEL, dtype=torch.uint8, device=dev)
    cls, bricks = ops.raycast_bricks(torch.from_numpy(grids).to(dev))
    ops.panel_voxel_view(cls, bricks, torch.from_numpy(rays).to(dev), dpal, panel, ops.tile_place(panel, 2, x0=3, y0=5, xstep=T + 1), 2, 204)
    host = panel.cpu().numpy()[0]
    want = np.full_like(host, SENTINEL)
    for k in range(2):
        want[:, 5:, 3 + k * (T + 1):3 + k * (T + 1) + T] = R.view_tile(grids[k], rays, R.R, pal)
    assert np.array_equal(host, want), np.argwhere(host != want)[:5]
    tile = host[:, 5:, 3:3 + T]
    assert (tile[:, :2] == 204).all() and (tile[:, :, -2:] == 204).all() and len(np.unique(tile[:, 2:-2, 2:-2])) > 8
    # a tile that would leave the panel is refused before anything is written
    with pytest.raises(RuntimeError, match='leaves the'):
        ops.panel_voxel_view(cls, bricks, torch.from_numpy(rays).to(dev), dpal, panel, ops.tile_place(panel, 2, x0=3, y0=6, xstep=T + 1), 2, 204)
    assert np.array_equal(panel.cpu().numpy()[0], want)


# ---- the panel through the trainer ------------------------------------------------------------------------------------------------
B, S, RF = 1, 3, 2


class _Writer:
    def __init__(self):
        self.images = {}

    def add_images(self, name, tensor, global_step=0):
        self.images[name] = tensor.cpu().numpy()

    def add_video(self, name, tensor, global_step=0, fps=2):
        self.images[name] = tensor.cpu().numpy()


def _visualise(cfg, batch, output, imagines, **attrs):
    from muvo_amd.trainer import WorldModelTrainer
    stub = types.SimpleNamespace(cfg=cfg, panel_writer=None, traj_panels=False, traj_options={}, flow_panels=False, _step_now=lambda: 0, **attrs)
    writer = _Writer()
    WorldModelTrainer.visualise(stub, batch, output, imagines, 0, prefix='val', writer=writer)
    return writer.images


def _logits(dev, grids, seed):
    """(b, T, X, Y, Z) class grids -> (b, T, 9, X, Y, Z) logits on the device"""
    return torch.from_numpy(np.stack([np.stack([R.logits_for(x, C9, seed=seed + 10 * n + t) for t, x in enumerate(row)]) for n, row in enumerate(grids)])).to(dev)


@pytest.fixture(scope='module')
def sequence():
    g = R.scene()
    label = np.stack([g, R.shifted(g, 11), R.shifted(R.shifted(g, 11), 12)])[None]                 # (1, 3, X, Y, Z)
    recon = np.stack([R.shifted(g, 13), R.corner_scene()])[None]                                  # (1, 2, ...)
    imagines = [np.stack([R.shifted(label[0, 2], 14 + i)])[None] for i in range(2)]               # 2 x (1, 1, ...)
    return label, recon, imagines


def test_voxel_panel_through_visualise(dev, sequence):
    import visualise_reference as VR
    from muvo_amd.visualise import render_panels
    label, recon, imagines = sequence
    cfg = VR.panel_cfg(voxel=True)
    batch = {'voxel_label_1': torch.from_numpy(label[:, :, None]).to(dev)}
    output = {'voxel_1': _logits(dev, recon, 20)}
    ims = [{'voxel_1': _logits(dev, im, 30 + i)} for i, im in enumerate(imagines)]
    plain = render_panels(cfg, batch, output, ims)
    off = _visualise(cfg, batch, output, ims)                               # the stub of earlier tests: no voxel attributes at all
    off2 = _visualise(cfg, batch, output, ims, voxel_panels=False, voxel_options={})
    for images in (off, off2):
        assert list(images) == [f'val_outputs_0{k}' for k in plain] == ['val_outputs_0_voxel_top']
        assert np.array_equal(images['val_outputs_0_voxel_top'], plain['_voxel_top'].cpu().numpy())
    on = _visualise(cfg, batch, output, ims, voxel_panels=True, voxel_options=dict(size=R.R))
    assert list(on) == ['val_outputs_0_voxel_top', 'val_outputs_0_voxel'] and np.array_equal(on['val_outputs_0_voxel_top'], off['val_outputs_0_voxel_top'])
    got = on['val_outputs_0_voxel']
    T = R.R + 4
    assert got.shape == (B, 3, 3 * T, S * T + int(T / 4)) and got.dtype == np.uint8
    pal, _ = _palette(dev)
    want = R.panel(label, recon, imagines, R.camera_rays(R.X, R.Y, R.Z, R.R), R.R, pal)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (got[:, :, :, RF * T:RF * T + 7] == 255).all() and (got[0, :, 2 * T + 2:3 * T - 2, 2:T - 2] == 255).all()     # separator; blank tile of class 0
    # the head switched off: no panel whatever the switch says; without imagined samples one prediction row, no separator
    assert _visualise(VR.panel_cfg(), batch, output, ims, voxel_panels=True, voxel_options={}) == {}
    from muvo_amd.voxel_view import voxel_panel
    short = voxel_panel(cfg, {'voxel_label_1': batch['voxel_label_1'][:, :RF]}, output, [], size=R.R).cpu().numpy()
    assert short.shape == (B, 3, 2 * T, RF * T) and np.array_equal(short, R.panel(label[:, :RF], recon, [], R.camera_rays(R.X, R.Y, R.Z, R.R), R.R, pal))


# ---- RayIoU ----------------------------------------------------------------------------------------------------------------------
def test_ray_iou_counts(dev):
    from muvo_amd import ops
    g = R.scene()
    label = np.stack([g, R.shifted(g, 5)])
    pred = np.stack([R.shifted(g), R.shifted(label[1], 6)])
    rays = _all_rays(g)
    res = 0.5                                                   # 1 / 2 / 4 m are 2 / 4 / 8 cells of this 13-cell grid
    want, terms = np.zeros((3, C9, 3), np.int64), []
    for f in range(2):
        c, t = R.iou_counts(R.class_hits(label[f], rays), R.class_hits(pred[f], rays), C9, res)
        want += c
        terms.append(t)
    terms = np.concatenate(terms)
    assert want[:, :, 0].sum() > 50 and want[0, :, 0].sum() < want[2, :, 0].sum() and want[:, :, 1].sum() > 50 and want[:, :, 2].sum() > 50
    drays = torch.from_numpy(rays).to(dev)
    lg, lb = ops.raycast_bricks(torch.from_numpy(label).to(dev))
    pg, pb = ops.raycast_bricks(torch.from_numpy(pred).to(dev))
    counts = torch.zeros((3, C9, 3), dtype=torch.int64, device=dev)
    depth = torch.zeros(2, dtype=torch.float64, device=dev)
    ops.ray_iou_counts(lg, lb, pg, pb, drays, C9, res, counts, depth)
    assert np.array_equal(counts.cpu().numpy(), want), counts.cpu().numpy() - want
    total = float(terms.astype(np.float64).sum())
    d = depth.cpu().tolist()
    print(f'depth sum {d[0]!r} against {total!r} over {len(terms)} rays')
    assert d[1] == len(terms) and abs(d[0] - total) <= 1e-6 * total
    ops.ray_iou_counts(lg, lb, pg, pb, drays, C9, res, counts, depth)                       # a second call accumulates
    assert np.array_equal(counts.cpu().numpy(), 2 * want) and depth.cpu().tolist()[1] == 2 * len(terms)
    assert abs(depth.cpu().tolist()[0] - 2 * total) <= 1e-6 * 2 * total


def test_ray_iou_metric_over_two_batches(dev, sequence):
    from muvo_amd.config import get_cfg
    from muvo_amd.voxel_view import RayIoUMetric, lidar_rays
    label, recon, imagines = sequence
    cfg = get_cfg(cfg_dict={'POINTS': {'CHANNELS': 8, 'HORIZON_RESOLUTION': 128, 'LIDAR_POSITION': [0.75, 0.0, 1.25]},
                            'VOXEL': {'SIZE': [R.X, R.Y, R.Z], 'RESOLUTION': 0.5, 'EV_POSITION': [3, 5, 1]}})
    rays = lidar_rays(cfg, 4)
    assert rays.shape == (8 * 32, 7) and np.array_equal(rays, R.fan_rays((4.5, 5.0, 3.5), 8, 128, 10.0, -30.0).reshape(8, 128, 7)[:, ::4].reshape(-1, 7))
    batches = [(label, recon, imagines), (label[:, ::-1].copy(), recon[:, ::-1].copy(), imagines[::-1])]
    m = RayIoUMetric(cfg, stride=4)
    m.start_loader(0)
    counts, terms = np.zeros((2, 3, C9, 3), np.int64), [[], []]
    for i, (lab, rec, ims) in enumerate(batches):
        batch = {'voxel_label_1': torch.from_numpy(lab[:, :, None]).to(dev)}
        m.update(i, batch, {'voxel_1': _logits(dev, rec, 40 + i)}, [{'voxel_1': _logits(dev, im, 50 + i + k)} for k, im in enumerate(ims)])
        for which, (ls, ps) in enumerate(((lab[0, :RF], rec[0]), (lab[0, RF:], ims[0][0]))):
            for lg, pg in zip(ls, ps):
                c, t = R.iou_counts(R.class_hits(lg, rays), R.class_hits(pg, rays), C9, 0.5)
                counts[which] += c
                terms[which].append(t)
    res = m.result()
    for which, tail in ((0, ''), (1, '_imagine')):
        means = R.ray_iou(counts[which])
        t = np.concatenate(terms[which]).astype(np.float64)
        for k, thr in enumerate((1, 2, 4)):
            assert res[f'test0_ray_iou_{thr}m{tail}'] == pytest.approx(means[k], abs=1e-12)
        assert res[f'test0_ray_iou{tail}'] == pytest.approx(sum(means) / 3, abs=1e-12)
        assert res[f'test0_ray_pairs{tail}'] == len(t) > 20
        assert res[f'test0_ray_depth_l1{tail}'] == pytest.approx(t.sum() / len(t), rel=1e-6)
    assert 0 < res['test0_ray_iou_1m'] <= res['test0_ray_iou_4m'] < 1


def test_predict_ray_iou_and_voxel_panel_leave_the_metrics_alone(dev, tmp_path):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import ops
    from muvo_amd import predict as P
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    from muvo_amd.visualise import png_read
    root = str(tmp_path / 'rec')
    os.makedirs(root)
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(79)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    assert module.voxel_panels is False and module.voxel_options == {} and cfg.VOXEL_SEG.ENABLED

    def data():
        dm = DataModule(cfg, root, device=dev, seed=79)
        dm.setup()
        dm.test_sampler_0 = range(0, 4, 2)
        return dm
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'rays')
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        P.run(cfg, dev, a, 'test', loaders=[0], limit_batches=2, seed=79, data=data(), module=module, log=lambda s: None)
        out = P.run(cfg, dev, b, 'test', loaders=[0], limit_batches=2, seed=79, data=data(), module=module, log=lambda s: None, panels=1,
                    voxel=True, voxel_size=32, ray_iou=dict(stride=4))
    finally:
        ops.set_deterministic(was)
    assert open(os.path.join(a, 'metrics.json'), 'rb').read() == open(os.path.join(b, 'metrics.json'), 'rb').read()
    assert module.voxel_panels is False and module.voxel_options == {} and module.panel_writer is None
    res = json.load(open(os.path.join(b, 'ray_iou.json')))
    keys = [f'ray_iou_{k}m' for k in (1, 2, 4)] + ['ray_iou', 'ray_iou_per_class', 'ray_depth_l1', 'ray_pairs']
    assert res == json.loads(json.dumps(out['ray_iou'])) and set(res) == {f'test0_{k}{tail}' for k in keys for tail in ('', '_imagine')}
    for k in keys[:4]:
        for tail in ('', '_imagine'):
            v = res[f'test0_{k}{tail}']
            assert np.isfinite(v) and 0.0 <= v <= 1.0, (k, tail, v)
    assert all(np.isfinite(res[f'test0_ray_depth_l1{t}']) and res[f'test0_ray_depth_l1{t}'] >= 0 for t in ('', '_imagine'))
    assert not os.path.exists(os.path.join(a, 'ray_iou.json')) and not os.path.exists(os.path.join(a, 'panels'))
    views = [f for f in out['files'] if os.path.basename(os.path.dirname(f)).endswith('_voxel')]
    assert [os.path.relpath(f, b) for f in views] == ['panels/pred0_outputs_0_voxel/step00000000_b0.png']
    image = png_read(open(views[0], 'rb').read())
    n_rows = max(cfg.PREDICTION.N_SAMPLES, 1)                                 # s = 6 tiles of 32 + 4 pixels and the separator
    assert image.shape == ((1 + n_rows) * 36, 6 * 36 + 9, 3) and tuple(image[0, 0]) == (204, 204, 204)
    with pytest.raises(ValueError, match='mode test'):
        P.run(cfg, dev, str(tmp_path / 'sim'), 'sim', loaders=[2], data=data(), module=module, log=lambda s: None, ray_iou=dict(stride=4))
