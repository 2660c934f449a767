"""-m gpu: `muvo_amd.predict.run(..., 'test', bev_pq={}, panels=1, inst=True)` over the tiny `heads_on` recording of
tests/test_predict_iou_gpu.py (one module, one recording, 2 batches per loader): `bev_pq.json` against what the numpy restatement
(tests/bev_instance_reference.py) computes from the centre maps, offsets, logits and `instance_label_1` a hook copies out of every
output and of the first imagined sample; `metrics.json` byte for byte against a run without the switches; the `_inst` panel
against the reference's ids through the palette.  The model is untrained: its centre map is noise with thousands of peaks and
few matches - the comparison is against the reference, not against a quality bar, and the test asserts that the run has capped
frames and foreground pixels so that it is not vacuous."""
import json
import os

import numpy as np
import pytest
import torch

import bev_instance_reference as R

pytestmark = pytest.mark.gpu
SEED = 78                # the seed of tests/test_predict_iou_gpu.py; it gives capped frames and foreground pixels (asserted below)
KEYS = ('bev_instance_center_1', 'bev_instance_offset_1', 'bev_segmentation_1')
INT_FIELDS = ('tp', 'fp', 'fn', 'label_segments', 'pred_segments', 'pq_frames', 'pq_capped')


@pytest.fixture(scope='module')
def world(dev, tmp_path_factory):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path_factory.mktemp('rec'))
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('heads_on', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1)
    torch.manual_seed(SEED)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    dm = DataModule(cfg, root, device=dev, seed=SEED)
    dm.setup()
    assert len(dm.test_dataset) == 4 and len(dm.test_sampler_1) == 0
    dm.test_sampler_0, dm.test_sampler_2 = range(0, 4, 2), range(1, 4, 2)      # two batches each from a recording this small
    return cfg, module, dm


@pytest.fixture(scope='module')
def runs(dev, world, tmp_path_factory):
    """one run without the switches, one with them and a hook; deterministic mode, so the two repeat each other bit for bit"""
    from muvo_amd import ops
    from muvo_amd import predict as P
    cfg, module, dm = world
    assert module.inst_panels is False and module.inst_options == {} and cfg.SEMANTIC_SEG.ENABLED
    seen = []

    def hook(i, batch, output, output_imagines):
        assert len(output_imagines) == cfg.PREDICTION.N_SAMPLES >= 1
        host = lambda out: [out[k].detach().float().cpu().numpy() for k in KEYS]      # noqa: E731
        seen.append((i, host(output), host(output_imagines[0]), batch['instance_label_1'].cpu().numpy()))
    base = tmp_path_factory.mktemp('out')
    a, b = str(base / 'plain'), str(base / 'pq')
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        plain = P.run(cfg, dev, a, 'test', limit_batches=2, seed=SEED, data=dm, module=module, log=lambda s: None)
        lines = []
        out = P.run(cfg, dev, b, 'test', limit_batches=2, seed=SEED, data=dm, module=module, log=lines.append, hook=hook, bev_pq={}, panels=1, inst=True)
    finally:
        ops.set_deterministic(was)
    return a, b, plain, out, seen, lines


def _frames(x):
    return x.reshape(x.shape[0] * x.shape[1], *x.shape[2:])


def _reference(entries, rf):
    """the hook's copies of one loader -> ([counts (7,), IoU sum] for the reconstruction and for the imagination, capped frames, foreground pixels)"""
    acc, capped_frames, fg_pixels = [[np.zeros(7, np.int64), 0.0], [np.zeros(7, np.int64), 0.0]], 0, 0
    for _, recon, imagine, label in entries:
        for which, (c, o, seg), lab in ((0, recon, label[:, :rf]), (1, imagine, label[:, rf:])):
            c, o, seg, lab = _frames(c)[:, 0], _frames(o), _frames(seg), _frames(lab)[:, 0]
            assert c.shape[0] == lab.shape[0] and lab.dtype == np.uint8
            ids, _, _, capped = R.decode(c, o, seg, threshold=0.1, radius=1, K=100, thing_classes=(3, 4))
            counts, total = R.pq_counts(lab, ids, capped)
            acc[which][0] += counts
            acc[which][1] += total
            capped_frames += int(capped.sum())
            fg_pixels += int(sum(R.foreground_of(s).sum() for s in seg))
    return acc, capped_frames, fg_pixels


def test_bev_pq_json_equals_the_reference(world, runs):
    cfg, module, _ = world
    a, b, plain, out, seen, lines = runs
    rf = cfg.RECEPTIVE_FIELD
    assert out['batches'] == {0: 2, 1: 0, 2: 2} and [i for i, *_ in seen] == [0, 1, 0, 1]          # loader 0, then loader 2
    got = json.load(open(os.path.join(b, 'bev_pq.json')))
    assert got == json.loads(json.dumps(out['bev_pq'])) and os.path.join(b, 'bev_pq.json') in out['files']
    assert any(line.startswith('bev_pq ') for line in lines)
    names = ['bev_pq', 'bev_sq', 'bev_rq'] + [f'bev_{k}' for k in INT_FIELDS]
    assert set(got) == {f'test{idx}_{n}{tail}' for idx in (0, 1, 2) for n in names for tail in ('', '_imagine')}
    assert all(got[f'test1_{n}{tail}'] == 0 for n in names for tail in ('', '_imagine'))            # the empty loader
    capped_frames = fg_pixels = 0
    for k, idx in enumerate((0, 2)):
        acc, cf, fp = _reference(seen[2 * k:2 * k + 2], rf)
        capped_frames, fg_pixels = capped_frames + cf, fg_pixels + fp
        for which, tail in ((0, ''), (1, '_imagine')):
            counts, total = acc[which]
            want = dict(zip(R.COUNT_NAMES, counts.tolist()))
            ints = {'tp': want['tp'], 'fp': want['fp'], 'fn': want['fn'], 'label_segments': want['label_segments'], 'pred_segments': want['pred_segments'],
                    'pq_frames': want['frames'], 'pq_capped': want['capped']}
            print(f'test{idx}{tail}', ints, total, {n: got[f'test{idx}_bev_{n}{tail}'] for n in ('pq', 'sq', 'rq')})
            for n, v in ints.items():
                g = got[f'test{idx}_bev_{n}{tail}']
                assert isinstance(g, int) and g == v, (idx, tail, n, g, v)
            assert ints['pq_frames'] == 2 * (rf if which == 0 else cfg.FUTURE_HORIZON)
            for n, v in R.pq_summary(counts, total).items():
                g = got[f'test{idx}_bev_{n}{tail}']
                assert isinstance(g, float) and abs(g - v) <= 1e-12 * abs(v), (idx, tail, n, g, v)
    print('capped frames', capped_frames, 'foreground pixels', fg_pixels)
    assert capped_frames >= 1 and fg_pixels >= 1                 # else the comparison is vacuous: pick another SEED


def test_metrics_json_is_untouched_and_the_module_restored(world, runs):
    cfg, module, _ = world
    a, b, plain, out, _, _ = runs
    assert open(os.path.join(a, 'metrics.json'), 'rb').read() == open(os.path.join(b, 'metrics.json'), 'rb').read()
    assert os.listdir(a) == ['metrics.json'] and sorted(os.listdir(b)) == ['bev_pq.json', 'metrics.json', 'panels']
    assert 'bev_pq' not in plain and plain['metrics'] == out['metrics']
    assert module.inst_panels is False and module.inst_options == {} and module.panel_writer is None


def test_inst_panel_shows_the_reference_ids(world, runs):
    from muvo_amd.bev_instances import INSTANCE_COLOURS
    from muvo_amd.visualise import png_read
    cfg, _, _ = world
    _, b, _, out, seen, _ = runs

    def panel(loader, suffix):
        files = [f for f in out['files'] if os.path.basename(os.path.dirname(f)).endswith(suffix) and f'{loader}_outputs_0' in f]
        assert len(files) == 1 and files[0].endswith('_b0.png'), files
        return png_read(open(files[0], 'rb').read())
    pal = np.asarray(INSTANCE_COLOURS, np.uint8)
    for k, loader in enumerate((0, 2)):
        image, bev = panel(loader, '_inst'), panel(loader, '_bev')
        assert image.shape == bev.shape and image.dtype == np.uint8
        _, (c, o, seg), _, label = seen[2 * k]                   # batch 0 of the loader: the one with panels
        ids = R.decode(c[0, :1, 0], o[0, :1], seg[0, :1], threshold=0.1, radius=1, K=100)[0][0]
        h, w = ids.shape
        for row, tile in ((1, ids), (0, label[0, 0, 0])):        # the reconstruction row and the label row, first frame
            want = np.rot90(np.pad(pal[tile], ((2, 2), (2, 2), (0, 0)), constant_values=204), 1, axes=(0, 1))
            assert want.shape == (w + 4, h + 4, 3)
            got = image[row * (w + 4):(row + 1) * (w + 4), :h + 4]
            assert np.array_equal(got, want), (loader, row, np.argwhere(got != want)[:5])
