"""-m gpu: `muvo_amd.predict.run(..., 'test', voxel_calibration={}, panels=1, uncert=True)` over the tiny recording of
tests/test_predict_bev_pq_gpu.py (one module, one recording; voxel head on, PREDICTION.N_SAMPLES = 2, one batch of loader 0):
`voxel_calibration.json` against `summarise` of what the numpy restatement (tests/calibration_reference.py) accumulates from the
`voxel_1` logits of the output and of every imagined sample and the labels a hook copies out; `metrics.json` byte for byte against a
run without the switches; the `_uncert` panel against the restatement's byte maps through the colour ramp.  A third run has
VOXEL_SEG.VISIBILITY on, so that labels of 255 occur.  Integers match exactly; a real figure lies within the bar of
tests/test_voxel_calibration_gpu.py (four times what the float32 twin loses against float64, voxel by voxel, plus the fixed-point
step) carried through the figure's formula.  The model is untrained: the comparison is against the restatement, not a quality bar."""
import json
import os

import numpy as np
import pytest
import torch

import calibration_reference as R

pytestmark = pytest.mark.gpu
SEED = 78
BINS = 15
REAL = ('brier', 'nll', 'entropy_correct', 'entropy_wrong', 'mi_correct', 'mi_wrong')
INTS = ('voxels', 'ignored', 'skipped_nonfinite')


@pytest.fixture(scope='module')
def world(dev, tmp_path_factory):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path_factory.mktemp('rec'))
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, **{'PREDICTION.N_SAMPLES': 2})
    torch.manual_seed(SEED)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    dm = DataModule(cfg, root, device=dev, seed=SEED)
    dm.setup()
    assert len(dm.test_dataset) == 4
    dm.test_sampler_0 = range(0, 4, 2)
    return cfg, module, dm


def _set_visibility(cfgs, on):
    for cfg in cfgs:
        if on:
            cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True, 'LIDAR_STRIDE': 4, 'CAMERA_STRIDE': 8})
        else:
            cfg.VOXEL_SEG.pop('VISIBILITY', None)


@pytest.fixture(scope='module')
def runs(dev, world, tmp_path_factory):
    """a run without the switches, one with them and a hook, one with them under the visibility mask; deterministic mode, so the
    first two repeat each other bit for bit"""
    from muvo_amd import ops
    from muvo_amd import predict as P
    from muvo_amd.trainer import voxel_target
    cfg, module, dm = world
    assert module.uncert_panels is False and cfg.VOXEL_SEG.ENABLED and cfg.PREDICTION.N_SAMPLES == 2
    seen = {'plain': [], 'masked': []}

    def hook_into(bucket):
        def hook(i, batch, output, output_imagines):
            assert len(output_imagines) == 2
            host = lambda out: out['voxel_1'].detach().float().cpu().numpy()      # noqa: E731
            label = voxel_target(cfg, batch, 1)
            label = label[:, :, 0] if label.dim() == 6 else label
            bucket.append((host(output), [host(im) for im in output_imagines], label.cpu().numpy().astype(np.uint8)))
        return hook
    base = tmp_path_factory.mktemp('out')
    a, b, c = str(base / 'plain'), str(base / 'cal'), str(base / 'masked')
    quiet = lambda s: None      # noqa: E731
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        plain = P.run(cfg, dev, a, 'test', loaders=[0], limit_batches=1, seed=SEED, data=dm, module=module, log=quiet)
        lines = []
        out = P.run(cfg, dev, b, 'test', loaders=[0], limit_batches=1, seed=SEED, data=dm, module=module, log=lines.append, hook=hook_into(seen['plain']),
                    voxel_calibration={}, panels=1, uncert=True)
        _set_visibility((cfg, module.cfg), True)
        try:
            masked = P.run(cfg, dev, c, 'test', loaders=[0], limit_batches=1, seed=SEED, data=dm, module=module, log=quiet, hook=hook_into(seen['masked']),
                           voxel_calibration={'bins': 10})
        finally:
            _set_visibility((cfg, module.cfg), False)
    finally:
        ops.set_deterministic(was)
    return a, b, plain, out, masked, seen, lines


def _reference(entries, rf, B):
    """the hook's copies -> per group (0 reconstruction, 1 imagined ensemble): the restatement's accumulators summed over the frames, the
    bars of the real sums and of the bins' conf sums, and the byte maps per frame"""
    groups = []
    for which in (0, 1):
        acc, bar_sums, bar_conf, maps = None, np.zeros(6), np.zeros(B), []
        for recon, imagines, label in entries:
            fh = imagines[0].shape[1]
            samples, lab = ([recon], label[:, :rf]) if which == 0 else (imagines, label[:, rf:rf + fh])
            for b in range(lab.shape[0]):
                for t in range(lab.shape[1]):                                # frame by frame: the sums and the bars add up
                    lg = [np.ascontiguousarray(s[b, t][None]) for s in samples]
                    ref, twin = R.accumulate(lg, lab[b, t][None], B), R.accumulate(lg, lab[b, t][None], B, np.float32)
                    s, c = R.bars(ref, twin)
                    bar_sums, bar_conf = bar_sums + s, bar_conf + c
                    maps.append((ref['top_entropy'][0], ref['top_mi'][0]))
                    if acc is None:
                        acc = {k: ref[k].copy() for k in ('table', 'counts', 'ssc', 'sums')}
                    else:
                        for k in acc:
                            acc[k] += ref[k]
        groups.append((acc, bar_sums, bar_conf, maps))
    return groups


@pytest.fixture(scope='module')
def plain_groups(world, runs):
    return _reference(runs[5]['plain'], world[0].RECEPTIVE_FIELD, BINS)


def _check_json(got, groups, B, prefix='test0_voxel_'):
    from muvo_amd.calibration import VoxelCalibrationMetric
    fixed = [R.to_fixed(g[0]) for g in groups]
    want = VoxelCalibrationMetric.summarise(**{k: [fixed[0][k], fixed[1][k]] for k in fixed[0]}, samples=2)
    assert {k[len(prefix):] for k in got if k.startswith(prefix)} == {k[len('voxel_'):] for k in want}
    for which, tail in ((0, ''), (1, '_imagine')):
        acc, bar_sums, bar_conf, _ = groups[which]
        g = lambda name: got[f'{prefix}{name}{tail}']      # noqa: E731
        w = lambda name: want[f'voxel_{name}{tail}']       # noqa: E731
        n, correct = int(acc['counts'][0]), int(acc['counts'][3])
        for name in INTS:
            assert isinstance(g(name), int) and g(name) == w(name) == int(acc['counts'][INTS.index(name)]), (tail, name, g(name), w(name))
        assert g('accuracy') == w('accuracy') == correct / n and g('ens_iou') == w('ens_iou') and g('ens_miou') == w('ens_miou')
        den = dict(brier=n, nll=n, entropy_correct=correct, entropy_wrong=n - correct, mi_correct=correct, mi_wrong=n - correct)
        for k, name in enumerate(REAL):
            bar = bar_sums[k] / max(den[name], 1) + 1e-12
            print(f'{prefix}{name}{tail}: json {g(name):.9g} restatement {w(name):.9g} deviation {abs(g(name) - w(name)):.3g} bar {bar:.3g}')
            assert abs(g(name) - w(name)) <= bar, (tail, name, g(name), w(name), bar)
        rows = acc['table']
        assert [r[0] for r in g('reliability')] == rows[:, 0].astype(np.int64).tolist()
        assert [r[1] for r in g('reliability')] == [r[1] for r in w('reliability')]
        for b in range(B):
            assert abs(g('reliability')[b][2] - w('reliability')[b][2]) <= bar_conf[b] / max(rows[b, 0], 1) + 1e-12, (tail, b)
        # ece = sum_b |ok_b - conf_b| / N and mce = max_b |ok_b - conf_b| / n_b move by at most the conf sums' errors
        assert abs(g('ece') - w('ece')) <= bar_conf.sum() / n + 1e-12, (tail, g('ece'), w('ece'))
        assert abs(g('mce') - w('mce')) <= max(bar_conf[b] / max(rows[b, 0], 1) for b in range(B)) + 1e-12, (tail, g('mce'), w('mce'))
    assert got[f'{prefix}samples_imagine'] == 2
    return want


def test_voxel_calibration_json_equals_the_restatement(world, runs, plain_groups):
    cfg, module, _ = world
    a, b, plain, out, masked, seen, lines = runs
    assert out['batches'] == {0: 1} and len(seen['plain']) == 1
    got = json.load(open(os.path.join(b, 'voxel_calibration.json')))
    assert got == json.loads(json.dumps(out['voxel_calibration'])) and os.path.join(b, 'voxel_calibration.json') in out['files']
    assert any(line.startswith('voxel_calibration ') for line in lines)
    _check_json(got, plain_groups, BINS)
    frame = int(np.prod(seen['plain'][0][2].shape[2:]))
    assert got['test0_voxel_voxels'] == 2 * frame and got['test0_voxel_voxels_imagine'] == 4 * frame and got['test0_voxel_ignored'] == 0
    assert got['test0_voxel_mi_correct'] == 0.0 and got['test0_voxel_mi_wrong'] == 0.0             # K = 1
    assert got['test0_voxel_mi_correct_imagine'] + got['test0_voxel_mi_wrong_imagine'] > 0         # the two samples differ


def test_the_visibility_mask_reaches_the_metric(world, runs):
    cfg, _, _ = world
    masked, seen = runs[4], runs[5]
    got = masked['voxel_calibration']
    assert len(got['test0_voxel_reliability']) == 10
    _check_json(got, _reference(seen['masked'], cfg.RECEPTIVE_FIELD, 10), 10)
    assert got['test0_voxel_ignored'] > 0 and got['test0_voxel_ignored_imagine'] > 0 and got['test0_voxel_voxels'] > 0
    assert (seen['masked'][0][2] == 255).any() and not (seen['plain'][0][2] == 255).any()


def test_metrics_json_is_untouched_and_the_module_restored(world, runs):
    cfg, module, _ = world
    a, b, plain, out = runs[:4]
    assert open(os.path.join(a, 'metrics.json'), 'rb').read() == open(os.path.join(b, 'metrics.json'), 'rb').read()
    assert os.listdir(a) == ['metrics.json'] and sorted(os.listdir(b)) == ['metrics.json', 'panels', 'voxel_calibration.json']
    assert 'voxel_calibration' not in plain and plain['metrics'] == out['metrics']
    assert module.uncert_panels is False and module.panel_writer is None and 'VISIBILITY' not in module.cfg.VOXEL_SEG


def test_uncert_panel_shows_the_restatement_maps(world, runs, plain_groups):
    from muvo_amd.calibration import UNCERT_COLOURS
    from muvo_amd.visualise import PAD_BYTE, png_read, strip_size
    cfg, _, _ = world
    b, out, seen = runs[1], runs[3], runs[5]
    files = [f for f in out['files'] if os.path.basename(os.path.dirname(f)).endswith('_uncert')]
    assert len(files) == 1 and files[0].endswith('_b0.png') and '0_outputs_0' in files[0], files
    image = png_read(open(files[0], 'rb').read())
    rf, fh = cfg.RECEPTIVE_FIELD, cfg.FUTURE_HORIZON
    X, Y = seen['plain'][0][2].shape[2:4]
    th, tw, sep = X + 4, Y + 4, int((Y + 4) / 4)
    assert image.shape == (*strip_size([th] * 3, tw, rf + fh, rf, sep), 3) and image.dtype == np.uint8
    groups = plain_groups
    ramp = np.asarray(UNCERT_COLOURS, np.int64)
    assert np.array_equal(ramp.sum(1), 3 * np.arange(256))                  # a pixel's level is (r + g + b) / 3

    def tile(row, t):
        x0 = t * tw + (sep if t >= rf else 0)
        return image[row * th:(row + 1) * th, x0:x0 + tw].astype(np.int64)

    def shows(row, t, want):
        got = tile(row, t)
        assert (got[:2] == PAD_BYTE).all() and (got[:, :2] == PAD_BYTE).all() and (got[-2:] == PAD_BYTE).all() and (got[:, -2:] == PAD_BYTE).all()
        inner = got[2:-2, 2:-2]
        level = inner.sum(2) // 3
        assert np.array_equal(ramp[level], inner)                            # every pixel is a colour of the ramp
        assert np.abs(level - want.astype(np.int64)).max() <= 1, (row, t, np.abs(level - want.astype(np.int64)).max())
    for t in range(rf):
        shows(0, t, groups[0][3][t][0])
        for row in (1, 2):
            assert (tile(row, t)[2:-2, 2:-2] == 255).all()                   # the receptive steps of the ensemble rows are blank
    for t in range(fh):
        shows(1, rf + t, groups[1][3][t][0])
        shows(2, rf + t, groups[1][3][t][1])
        assert (tile(0, rf + t)[2:-2, 2:-2] == 255).all()
    assert max(m[0].max() for m in groups[1][3]) > 0                         # not a black picture
