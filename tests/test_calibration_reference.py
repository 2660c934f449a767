"""CPU: the numpy restatement of muvo_voxel_calibration (tests/calibration_reference.py) against independent computations and
hand-made cases; `VoxelCalibrationMetric.summarise`; the argument checks of ops.voxel_calibration and of the C entry, which run
before the device is touched; the switches.  The generator of the GPU test's inputs is checked here too."""
import math
import types

import numpy as np
import pytest
import torch

import calibration_reference as R

LN2 = math.log(2.0)


@pytest.fixture(scope='module')
def random_case():
    logits, label, dropped = R.make_case(5, 3, 5, 4, 5, 6, 3, 15)
    assert dropped == 0
    return logits, label, R.accumulate(logits, label, 15)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_per_voxel_against_torch(random_case):
    logits, label, ref = random_case
    x = torch.from_numpy(np.stack(logits)).double()                          # (K, F, C, X, Y, Z)
    p = torch.softmax(x, dim=2)
    pbar = p.mean(0)
    H = torch.special.entr(pbar).sum(1).reshape(-1).numpy()
    ebar = torch.special.entr(p).sum(2).mean(0).reshape(-1).numpy()
    v = ref['voxel']
    got = np.moveaxis(v['pbar'].reshape(5, *label.shape), 0, 1)
    assert np.abs(got - pbar.numpy()).max() < 1e-14
    assert np.abs(v['H'] - H).max() < 1e-13 and np.abs(v['MI'] - np.maximum(0, H - ebar)).max() < 1e-13
    scored = label.reshape(-1) != 255
    assert np.array_equal(ref['ens'].reshape(-1)[scored], pbar.argmax(1).reshape(-1).numpy()[scored])
    onehot = torch.nn.functional.one_hot(torch.from_numpy(np.where(label == 255, 0, label).astype(np.int64)), 5).movedim(-1, 1).double()
    brier = ((pbar - onehot) ** 2).sum(1).reshape(-1).numpy()
    nll = torch.nn.functional.nll_loss(pbar.log(), torch.from_numpy(label.astype(np.int64)), ignore_index=255, reduction='sum')
    assert abs(ref['sums'][0] - brier[scored].sum()) < 1e-9 and abs(ref['sums'][1] - float(nll)) < 1e-9


def test_ece_by_explicit_loops(random_case):
    from muvo_amd.calibration import VoxelCalibrationMetric
    logits, label, ref = random_case
    B = 15
    v = ref['voxel']
    conf, ok = v['conf'][v['scored']], v['correct'][v['scored']]
    ece, mce, n = 0.0, 0.0, len(conf)
    for b in range(B):
        members = [i for i in range(n) if (b / B <= conf[i] < (b + 1) / B) or (b == B - 1 and conf[i] >= 1.0)]
        if members:
            gap = abs(sum(ok[i] for i in members) / len(members) - sum(conf[i] for i in members) / len(members))
            ece, mce = ece + len(members) / n * gap, max(mce, gap)
    fixed = R.to_fixed(ref)
    zero = R.to_fixed(R.accumulate(logits, np.full_like(label, 255), B))
    out = VoxelCalibrationMetric.summarise(**{k: [fixed[k], zero[k]] for k in fixed}, samples=3)
    assert abs(out['voxel_ece'] - ece) < 1e-6 and abs(out['voxel_mce'] - mce) < 1e-6          # fixed point: 2^-25 a voxel
    assert out['voxel_accuracy'] == ok.sum() / n and out['voxel_voxels'] == n
    assert out['voxel_voxels_imagine'] == 0 and out['voxel_ece_imagine'] == 0.0 and out['voxel_samples_imagine'] == 3


def test_ssc_counts_at_k1_against_the_ssc_restatement(random_case):
    from oracle import muvo_ref
    logits, label, _ = random_case
    for C_label in (5, 7):                                                   # 7: labels 5 and 6 lie outside the head's 5 classes
        lab = label.copy()
        if C_label == 7:
            lab[0, 0] = 5
            lab[0, 1] = 6
        ref = R.accumulate(logits[:1], lab, 15)
        pred = torch.from_numpy(logits[0]).argmax(1)
        comp, tps, fps, fns = muvo_ref.ssc_counts(pred, torch.from_numpy(lab), 5)
        want = comp.tolist() + [v for j in range(5) for v in (int(tps[j]), int(fps[j]), int(fns[j]))]
        assert ref['ssc'].tolist() == want
        assert np.all(ref['voxel']['MI'] == 0)                               # K = 1: H and Ebar are the same number
    assert ref['counts'][3] < R.accumulate(logits[:1], label, 15)['counts'][3]             # an out-of-range label is never correct


def test_the_input_generator_keeps_its_margins():
    """the condition the GPU test puts on its inputs, for its shapes: no voxel dropped, both margins >= 1e-4"""
    for grid in ((5, 6, 7), (8, 8, 64), (3, 5, 70)):
        for C, K, B in ((2, 1, 1), (9, 3, 15), (16, 8, 32), (2, 8, 32), (16, 1, 15)):
            logits, label, dropped = R.make_case(1000 * C + 10 * K + B, 3, C, *grid, K, B)
            assert dropped == 0
            top, edge = R.margins(R.accumulate(logits, label, B), B)
            assert top.min() >= 1e-4 and edge.min() >= 1e-4 and (label[2] == 255).all() and (label[:2] != 255).any()


# ------------------------------------------------------------------------------------------------ hand-made cases
def test_hand_made_cases():
    cases = R.hand_cases()
    for C in (2, 4):
        logits, label, B = cases[f'equal_c{C}']
        ref = R.accumulate(logits, label, B)
        v = ref['voxel']
        assert (ref['ens'] == 0).all() and (v['conf'] == 1.0 / C).all() and np.abs(v['H'] - math.log(C)).max() < 1e-15 and (v['MI'] == 0).all()
        assert (ref['top_entropy'] == 255).all() and (ref['top_mi'] == 0).all()
        assert ref['table'][min(B - 1, int(B / C))][0] == label.size and ref['counts'].tolist() == [label.size, 0, 0, int((label == 0).sum())]
    logits, label, B = cases['onehot_pair']
    ref = R.accumulate(logits, label, B)
    v = ref['voxel']
    assert np.abs(v['H'] - LN2).max() < 1e-15 and np.abs(v['MI'] - LN2).max() < 1e-15 and (ref['top_mi'] == 255).all() and (ref['ens'] == 0).all()
    assert abs(ref['sums'][0] - 0.5 * label.size) < 1e-12 and abs(ref['sums'][1] - LN2 * label.size) < 1e-9
    logits, label, B = cases['conf_one']
    ref = R.accumulate(logits, label, B)
    assert (ref['voxel']['conf'] == 1.0).all() and ref['table'][B - 1][0] == label.size and ref['table'][:B - 1, 0].sum() == 0
    assert (ref['ens'] == 1).all() and (ref['top_entropy'] == 0).all()
    wrong = int((label != 1).sum())
    assert abs(ref['sums'][1] - wrong * 160.0) > 1 and abs(ref['sums'][1] - wrong * -math.log(1e-12)) < 1e-9     # e^-160 is below the floor
    logits, label, B = cases['neg_inf']
    ref = R.accumulate(logits, label, B)
    v = ref['voxel']
    assert ref['counts'].tolist()[:3] == [30 - 2, 30 + 2, 0] and (v['pbar'][1] == 0).all() and np.abs(v['H'][v['scored']] - LN2).max() < 1e-15
    assert (ref['ens'][1] == 255).all() and (ref['ens'][0, 0, 0, :2] == 255).all() and (ref['top_entropy'][1] == quantised_ln2_of_3()).all()
    logits, label, B = cases['nonfinite']
    ref = R.accumulate(logits, label, B)
    # frame 0: 30 scored; frame 1: +inf everywhere, one voxel ignored; frame 2: a column of -inf (one of its 5 ignored) and a NaN column
    assert ref['counts'].tolist()[:3] == [30 + 20, 2, 29 + 4 + 5]
    assert (ref['ens'][1] == 255).all() and (ref['top_entropy'][1] == 0).all() and (ref['top_mi'][1] == 0).all()
    assert ref['ens'][2, 1, 1, 2] == 255 and ref['top_entropy'][2, 0, 0] == 0 and ref['top_entropy'][2, 1, 1] == 0 and (ref['top_entropy'][0] > 0).all()
    assert int(ref['table'][:, 0].sum()) == ref['counts'][0]


def quantised_ln2_of_3():
    return int(np.rint(255 * LN2 / math.log(3)))


# ------------------------------------------------------------------------------------------------ summarise
def test_summarise_on_hand_written_accumulators():
    from muvo_amd.calibration import VoxelCalibrationMetric
    F = 1 << 24
    B, C = 4, 3
    table = [[0, 0, 0], [4, 1, int(1.5 * F)], [0, 0, 0], [6, 6, int(5.4 * F)]]               # bins 0 and 2 empty
    counts = [10, 5, 1, 7]
    ssc = [6, 1, 1, 2, 1, 0, 3, 0, 1, 2, 2, 2]
    sums = [int(2.5 * F), int(7.0 * F), int(0.7 * F), int(1.2 * F), int(0.07 * F), int(0.6 * F)]
    zeros = dict(table=[[0] * 3] * B, counts=[0] * 4, ssc=[0] * (3 + 3 * C), sums=[0] * 6)
    out = VoxelCalibrationMetric.summarise([table, zeros['table']], [counts, zeros['counts']], [ssc, zeros['ssc']], [sums, zeros['sums']], samples=2)
    gap1, gap3 = abs(1 / 4 - 1.5 / 4), abs(1.0 - 5.4 / 6)
    assert abs(out['voxel_ece'] - (0.4 * gap1 + 0.6 * gap3)) < 1e-7 and abs(out['voxel_mce'] - max(gap1, gap3)) < 1e-7
    assert out['voxel_reliability'][0] == [0, 0.0, 0.0] and out['voxel_reliability'][1][:2] == [4, 0.25]
    assert abs(out['voxel_brier'] - 0.25) < 1e-7 and abs(out['voxel_nll'] - 0.7) < 1e-7 and out['voxel_accuracy'] == 0.7
    assert abs(out['voxel_entropy_correct'] - 0.1) < 1e-7 and abs(out['voxel_entropy_wrong'] - 0.4) < 1e-7
    assert abs(out['voxel_mi_correct'] - 0.01) < 1e-7 and abs(out['voxel_mi_wrong'] - 0.2) < 1e-7
    iou = [np.float32(tp) / (np.float32(tp + fp + fn) + np.float32(1e-5)) for tp, fp, fn in ((2, 1, 0), (3, 0, 1), (2, 2, 2))]
    assert out['voxel_ens_iou'] == [float(v) for v in iou] and out['voxel_ens_miou'] == float((iou[1] + iou[2]) / np.float32(2))
    assert (out['voxel_voxels'], out['voxel_ignored'], out['voxel_skipped_nonfinite']) == (10, 5, 1)
    # all-zero input: every figure 0, no division by zero
    names = ('ece', 'mce', 'brier', 'nll', 'accuracy', 'ens_miou', 'entropy_correct', 'entropy_wrong', 'mi_correct', 'mi_wrong', 'voxels', 'ignored',
             'skipped_nonfinite')
    assert all(out[f'voxel_{n}_imagine'] == 0 for n in names)
    assert out['voxel_ens_iou_imagine'] == [0.0] * C and out['voxel_reliability_imagine'] == [[0, 0.0, 0.0]] * B
    assert out['voxel_samples_imagine'] == 2 and 'voxel_samples' not in out
    assert set(out) == {f'voxel_{n}{t}' for n in names + ('ens_iou', 'reliability') for t in ('', '_imagine')} | {'voxel_samples_imagine'}


def test_result_of_an_empty_metric():
    from muvo_amd import config
    from muvo_amd.calibration import VoxelCalibrationMetric
    m = VoxelCalibrationMetric(config.get_cfg(cfg_dict={}), bins=3)
    m.start_loader(1)
    out = m.result()
    assert out['test1_voxel_ece'] == 0.0 and out['test1_voxel_reliability_imagine'] == [[0, 0.0, 0.0]] * 3 and out['test1_voxel_samples_imagine'] == 0
    with pytest.raises(ValueError, match='bins'):
        VoxelCalibrationMetric(config.get_cfg(cfg_dict={}), bins=33)


def test_the_colour_ramp_is_its_closed_form():
    from muvo_amd.calibration import UNCERT_COLOURS
    assert len(UNCERT_COLOURS) == 256 and UNCERT_COLOURS[0] == (0, 0, 0) and UNCERT_COLOURS[255] == (255, 255, 255)
    assert all(sum(c) == 3 * k and max(c) <= 255 and min(c) >= 0 for k, c in enumerate(UNCERT_COLOURS))


# ------------------------------------------------------------------------------------------------ argument checks, no GPU
def test_ops_checks_limits_before_the_library():
    from muvo_amd import ops
    z = lambda *s: torch.zeros(s, dtype=torch.int64)      # noqa: E731
    lg = torch.zeros(1, 3, 2, 2, 2)
    lab = torch.zeros(1, 2, 2, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match='samples'):
        ops.voxel_calibration([], lab, z(15, 3), z(4), z(12), z(6))
    with pytest.raises(ValueError, match='samples'):
        ops.voxel_calibration([lg] * 9, lab, z(15, 3), z(4), z(12), z(6))
    with pytest.raises(ValueError, match='classes'):
        ops.voxel_calibration([torch.zeros(1, 17, 2, 2, 2)], lab, z(15, 3), z(4), z(54), z(6))
    with pytest.raises(ValueError, match='classes'):
        ops.voxel_calibration([torch.zeros(1, 1, 2, 2, 2)], lab, z(15, 3), z(4), z(6), z(6))
    for B in (0, 33):
        with pytest.raises(ValueError, match='bins'):
            ops.voxel_calibration([lg], lab, z(B, 3), z(4), z(12), z(6))
    with pytest.raises(ValueError, match='frames'):
        ops.voxel_calibration([torch.zeros(0, 3, 2, 2, 2)], lab[:0], z(15, 3), z(4), z(12), z(6))
    with pytest.raises(AssertionError, match='one shape'):
        ops.voxel_calibration([lg, lg[:, :, :1]], lab, z(15, 3), z(4), z(12), z(6))
    with pytest.raises(AssertionError, match='float32'):
        ops.voxel_calibration([lg.double()], lab, z(15, 3), z(4), z(12), z(6))
    with pytest.raises(AssertionError, match='label'):
        ops.voxel_calibration([lg], lab.long(), z(15, 3), z(4), z(12), z(6))
    with pytest.raises(AssertionError, match='ssc'):
        ops.voxel_calibration([lg], lab, z(15, 3), z(4), z(11), z(6))
    with pytest.raises(AssertionError, match='sums'):
        ops.voxel_calibration([lg], lab, z(15, 3), z(4), z(12), z(6).double())
    with pytest.raises(AssertionError, match='top_mi'):
        ops.voxel_calibration([lg], lab, z(15, 3), z(4), z(12), z(6), top_mi=torch.zeros(1, 2, 2, 2, dtype=torch.uint8))


def test_the_entry_validates_before_touching_the_device():
    """bad arguments come back as MUVO_ERR_INVALID_ARG with a message naming the argument; nothing is launched"""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    i64, p, null = C.c_int64, C.c_void_p(4096), C.c_void_p(0)
    ptrs = (C.c_void_p * 8)(*[4096] * 8)
    holes = (C.c_void_p * 8)(4096, 4096, 0, 4096, 4096, 4096, 4096, 4096)

    def call(lg=ptrs, K=2, label=p, F=3, Cn=9, X=5, Y=6, Z=7, B=15, table=p, counts=p, ssc=p, sums=p):
        return L.muvo_voxel_calibration(lg, K, label, i64(F), Cn, X, Y, Z, B, table, counts, ssc, sums, null, null, null, null)
    for kw, msg in (({'K': 0}, b'K=0'), ({'K': 9}, b'K=9'), ({'Cn': 1}, b'C=1'), ({'Cn': 17}, b'C=17'), ({'B': 0}, b'B=0'), ({'B': 33}, b'B=33'),
                    ({'F': 0}, b'F=0'), ({'X': 0}, b'X=0'), ({'Z': 0}, b'Z=0'), ({'F': 1 << 30, 'X': 1 << 10, 'Y': 1 << 10, 'Z': 2}, b'2^40'),
                    ({'lg': null}, b'logits is null'), ({'lg': holes, 'K': 3}, b'logits[2] is null'), ({'label': null}, b'label is null'),
                    ({'table': null}, b'table is null'), ({'counts': null}, b'counts is null'), ({'ssc': null}, b'ssc is null'),
                    ({'sums': null}, b'sums is null')):
        assert call(**kw) == -1 and msg in L.muvo_last_error(), (kw, L.muvo_last_error())
    assert call(lg=holes, K=2, label=null) == -1 and b'label is null' in L.muvo_last_error()        # the hole lies past K


# ------------------------------------------------------------------------------------------------ the switches
def test_predict_refuses_the_switches_outside_mode_test_and_without_the_head(tmp_path):
    from muvo_amd import config
    from muvo_amd import predict as P
    base = ['--config-file', 'x.yml', '--out', 'o']
    for flag in (['--voxel-calibration'], ['--panels', '0', '--uncert']):
        with pytest.raises(SystemExit, match='--voxel-calibration and --uncert go with --mode test'):
            P.parse_args(base + ['--mode', 'sim'] + flag)
    with pytest.raises(SystemExit, match='--uncert goes with --panels N'):
        P.parse_args(base + ['--mode', 'test', '--uncert'])
    for bins in ('0', '33'):
        with pytest.raises(SystemExit, match='--calibration-bins'):
            P.parse_args(base + ['--mode', 'test', '--voxel-calibration', '--calibration-bins', bins])
    args = P.parse_args(base + ['--mode', 'test', '--voxel-calibration', '--calibration-bins', '10', '--panels', '1', '--uncert'])
    assert args.voxel_calibration is True and args.calibration_bins == 10 and args.uncert is True
    assert P.parse_args(base + ['--mode', 'test']).calibration_bins == 15
    module = types.SimpleNamespace(panel_writer=None, traj_panels=False, traj_options={}, flow_panels=False, voxel_panels=False, voxel_options={})
    off = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}})
    for kw in ({'voxel_calibration': {}}, {'uncert': True}):
        with pytest.raises(ValueError, match='need the voxel head'):
            P._run_test(off, module, {}, 'unused', None, 500, 0, None, print, **kw)
    assert not hasattr(module, 'uncert_panels')
    data = types.SimpleNamespace(test_dataloader=lambda: [[], [], []])
    on = config.get_cfg(cfg_dict={'EVAL': {'RGB_SUPERVISION': True}})              # mode sim wants the RGB, lidar and voxel heads on
    assert on.VOXEL_SEG.ENABLED and on.LIDAR_RE.ENABLED and on.EVAL.RGB_SUPERVISION
    for kw in ({'voxel_calibration': {}}, {'uncert': True}):
        with pytest.raises(ValueError, match='belong to mode test'):
            P.run(on, 'cpu', str(tmp_path), 'sim', loaders=[2], data=data, module=module, **kw)


def test_train_forwards_the_switch_and_needs_the_head():
    from muvo_amd import config
    from muvo_amd import train as T
    assert T.build_parser().parse_args(['--panel-dir', 'd', '--uncert']).uncert is True
    assert T.build_parser().parse_args([]).uncert is False
    with pytest.raises(ValueError, match='needs the voxel head'):
        T.fit(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}}), 'cpu', steps=0, uncert=True)
