"""CPU: the numpy restatement of the BEV instance decode and of the panoptic-quality counts (tests/bev_instance_reference.py)
against independent computations - scipy's maximum filter for the peaks, a set-based brute force for PQ, hand-made frames for the
selection and the grouping - and the argument checks of the host entries, which fire before the device is touched."""
import types

import numpy as np
import pytest

import bev_instance_reference as R


# ------------------------------------------------------------------------------------------------ peaks
@pytest.mark.parametrize('radius', [1, 2, 3])
def test_peaks_equal_scipys_maximum_filter(radius):
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(5 + radius)
    for shape, quant in (((37, 53), 0), ((64, 64), 16), ((5, 3), 4)):
        c = rng.random(shape).astype(np.float32)
        if quant:
            c = (np.floor(c * quant) / quant).astype(np.float32)         # ties and plateaus
        # in-bounds maximum: the border is padded with -inf, which never wins
        mx = ndi.maximum_filter(c, size=2 * radius + 1, mode='constant', cval=-np.inf)
        want = (c > np.float32(0.25)) & (c >= mx)
        got = R.peaks(c, 0.25, radius)
        assert np.array_equal(got, want) and want.any()


def test_peaks_plateau_threshold_and_nan():
    c = np.zeros((6, 7), np.float32)
    c[1:3, 2:4] = 0.5                                  # a 2 x 2 plateau: 4 peaks
    c[5, 6] = 0.1                                      # exactly the threshold: no peak
    c[4, 0] = 0.3
    c[4, 1] = np.nan                                   # never a peak, never suppresses (4, 0)
    p = R.peaks(c, 0.1, 1)
    assert sorted(zip(*np.nonzero(p))) == [(1, 2), (1, 3), (2, 2), (2, 3), (4, 0)]
    assert not R.peaks(np.full((4, 4), np.nan, np.float32), 0.1, 1).any()


def test_selection_orders_by_score_then_index_and_caps():
    c = np.zeros((4, 5), np.float32)
    peak = np.zeros((4, 5), bool)
    for (y, x), v in {(3, 4): 0.5, (0, 1): 0.5, (2, 2): 0.75, (1, 0): 0.25}.items():
        c[y, x], peak[y, x] = v, True
    centres, n, capped = R.select(c, peak, 3)
    assert centres.tolist() == [[2, 2], [0, 1], [3, 4]] and n == 3 and capped == 1
    centres, n, capped = R.select(c, peak, 6)
    assert centres.tolist() == [[2, 2], [0, 1], [3, 4], [1, 0], [-1, -1], [-1, -1]] and n == 4 and capped == 0
    centres, n, capped = R.select(c, np.zeros((4, 5), bool), 2)
    assert centres.tolist() == [[-1, -1]] * 2 and n == 0 and capped == 0


def test_grouping_by_hand():
    H, W = 5, 9
    centres = np.asarray([[2, 2], [2, 6], [-1, -1]], np.int32)
    off = np.zeros((2, H, W), np.float32)
    fg = np.ones((H, W), bool)
    fg[0, 0] = False
    off[:, 1, 1] = np.inf                              # no finite distance: id 0
    off[1, 4, 0] = 7.0                                 # (4, 0) points at x = 7: centre 2
    off[1, 3, 8] = 100.0                               # a target outside the image: still nearest to centre 2
    ids = R.group(off, fg, centres, 2)
    assert ids.dtype == np.uint8 and ids[0, 0] == 0 and ids[1, 1] == 0 and ids[4, 0] == 2 and ids[3, 8] == 2
    assert ids[2, 4] == 1 and ids[0, 4] == 1           # equidistant from both centres: the lower id
    assert ids[2, 3] == 1 and ids[2, 5] == 2
    assert not R.group(off, fg, centres, 0).any()      # no centre: nothing


def test_foreground_first_maximum_and_nan():
    logits = np.zeros((5, 1, 4), np.float32)
    logits[3, 0, 0] = logits[4, 0, 0] = 2.0            # a tie between two thing classes: class 3
    logits[1, 0, 1] = logits[3, 0, 1] = 2.0            # a tie of road and vehicle: road, the first maximum
    logits[4, 0, 2], logits[2, 0, 2] = np.nan, 1.0     # the NaN never replaces the maximum: class 2
    logits[4, 0, 3] = 1.0
    assert R.argmax_first(logits).tolist() == [[3, 1, 2, 4]]
    assert R.foreground_of(logits, (3, 4)).tolist() == [[True, False, False, True]]
    assert R.foreground_of(logits, (1,)).tolist() == [[False, True, False, False]]


# ------------------------------------------------------------------------------------------------ panoptic quality
def _brute_pq(label, pred):
    """sets of pixel indices per segment; IoU as a fraction of set sizes"""
    g, q = label.reshape(-1), pred.reshape(-1)
    gs = {i: set(np.flatnonzero(g == i)) for i in np.unique(g) if i}
    qs = {j: set(np.flatnonzero(q == j)) for j in np.unique(q) if j}
    tp, iou, used_g, used_q = 0, 0.0, set(), set()
    for i, a in gs.items():
        for j, b in qs.items():
            inter, union = len(a & b), len(a | b)
            if 2 * inter > union:
                assert i not in used_g and j not in used_q             # IoU > 1/2: unique
                used_g.add(i), used_q.add(j)
                tp += 1
                iou += inter / union
    return len(gs), len(qs), tp, len(qs) - tp, len(gs) - tp, iou


def test_pq_equals_a_set_based_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(6):
        H, W = (9, 14) if trial % 2 else (16, 16)
        label = np.zeros((H, W), np.uint8)
        for k, i in enumerate(rng.choice(np.arange(1, 256), 5, replace=False)):
            y, x = rng.integers(0, H - 3), rng.integers(0, W - 3)
            label[y:y + rng.integers(1, 5), x:x + rng.integers(1, 5)] = i
        pred = np.where(rng.random((H, W)) < 0.8, label, 0).astype(np.uint8)
        pred = (np.where(pred > 0, pred % 7 + 1, 0) if trial < 4 else rng.integers(0, 4, (H, W))).astype(np.uint8)
        got, want = R.pq_frame(label, pred), _brute_pq(label, pred)
        assert got[:5] == want[:5] and abs(got[5] - want[5]) <= 1e-12 * max(want[5], 1.0), (trial, got, want)
    label = np.zeros((3, 4), np.uint8)
    assert R.pq_frame(label, label) == (0, 0, 0, 0, 0, 0.0)


def test_pq_half_is_no_match_and_three_fifths_is():
    label, pred = np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8)
    label[0, 0:4], pred[0, 0:2] = 4, 9                 # 2 / 4: IoU exactly 1/2
    label[2, 0:5], pred[2, 0:3] = 255, 2               # 3 / 5
    assert R.pq_frame(label, pred) == (2, 2, 1, 1, 1, 0.6)
    counts, total = R.pq_counts(np.stack([label, label * 0]), np.stack([pred, pred]), capped=[0, 1])
    assert counts.tolist() == [2, 1, 2, 4, 1, 3, 1] and total == 0.6
    s = R.pq_summary(counts, total)
    assert s['pq'] == pytest.approx(0.6 / 3.0, abs=1e-15) and s['sq'] == 0.6 and s['rq'] == pytest.approx(1 / 3.0, abs=1e-15)
    assert R.pq_summary(np.zeros(7, np.int64), 0.0) == {'pq': 0.0, 'sq': 0.0, 'rq': 0.0}


def test_summarise_names_and_zero_denominators():
    from muvo_amd.bev_instances import INSTANCE_COLOURS, PanopticQualityMetric
    out = PanopticQualityMetric.summarise([[5, 2, 4, 6, 1, 5, 3], [0] * 7], [[0.75], [0.0]])
    assert out['bev_pq'] == pytest.approx(0.75 / 5.0, abs=1e-15) and out['bev_sq'] == 0.75 and out['bev_rq'] == pytest.approx(0.2, abs=1e-15)
    assert (out['bev_pq_frames'], out['bev_pq_capped'], out['bev_label_segments'], out['bev_pred_segments']) == (5, 2, 4, 6)
    assert (out['bev_tp'], out['bev_fp'], out['bev_fn']) == (1, 5, 3)
    names = ['bev_pq', 'bev_sq', 'bev_rq', 'bev_tp', 'bev_fp', 'bev_fn', 'bev_label_segments', 'bev_pred_segments', 'bev_pq_frames', 'bev_pq_capped']
    assert set(out) == {n + tail for n in names for tail in ('', '_imagine')}
    assert all(out[n + '_imagine'] == 0 for n in names)
    m = PanopticQualityMetric(types.SimpleNamespace(), max_centres=7)
    m.start_loader(2)
    assert m.result()['test2_bev_pq'] == 0.0 and m.result()['test2_bev_pq_frames_imagine'] == 0 and m.options == {'max_centres': 7}
    assert len(INSTANCE_COLOURS) == 256 and INSTANCE_COLOURS[0] == (255, 255, 255) and len(set(INSTANCE_COLOURS)) == 256
    assert all(0 <= v <= 255 for c in INSTANCE_COLOURS for v in c)


# ------------------------------------------------------------------------------------------------ argument checks, no GPU
def test_ops_validate_before_touching_the_device():
    import torch
    from muvo_amd import ops
    F, H, W = 2, 6, 5
    c, o = torch.zeros((F, H, W)), torch.zeros((F, 2, H, W))
    seg, fg = torch.zeros((F, 8, H, W)), torch.zeros((F, H, W), dtype=torch.uint8)
    with pytest.raises(AssertionError, match='centre maps'):
        ops.bev_instance_decode(c.double(), o, seg)
    with pytest.raises(AssertionError, match='centre maps'):
        ops.bev_instance_decode(c[0], o, seg)
    with pytest.raises(AssertionError, match='offsets'):
        ops.bev_instance_decode(c, o[:, :1], seg)
    with pytest.raises(AssertionError, match='either logits or a foreground mask'):
        ops.bev_instance_decode(c, o)
    with pytest.raises(AssertionError, match='either logits or a foreground mask'):
        ops.bev_instance_decode(c, o, seg, fg)
    with pytest.raises(AssertionError, match='logits'):
        ops.bev_instance_decode(c, o, seg.half())
    with pytest.raises(AssertionError, match='foreground mask'):
        ops.bev_instance_decode(c, o, foreground=fg.float())
    for K in (0, 255, -3):
        with pytest.raises(ValueError, match='centres outside 1..254'):
            ops.bev_instance_decode(c, o, seg, max_centres=K)
    for r in (0, 4):
        with pytest.raises(ValueError, match='radius . outside 1..3'):
            ops.bev_instance_decode(c, o, seg, radius=r)
    for C in (1, 33):
        with pytest.raises(ValueError, match='classes outside 2..32'):
            ops.bev_instance_decode(c, o, torch.zeros((F, C, H, W)))
    with pytest.raises(ValueError, match='thing class 32'):
        ops.bev_instance_decode(c, o, seg, thing_classes=(3, 32))
    with pytest.raises(ValueError, match='NaN'):
        ops.bev_instance_decode(c, o, seg, threshold=float('nan'))
    counts, total = torch.zeros(7, dtype=torch.int64), torch.zeros(1, dtype=torch.float64)
    with pytest.raises(AssertionError, match='id maps'):
        ops.bev_pq_counts(fg.long(), fg, counts, total)
    with pytest.raises(AssertionError, match='id maps'):
        ops.bev_pq_counts(fg[0], fg[0], counts, total)
    with pytest.raises(AssertionError, match='one shape'):
        ops.bev_pq_counts(fg, fg[:, :3], counts, total)
    with pytest.raises(AssertionError, match='counts'):
        ops.bev_pq_counts(fg, fg, counts[:6], total)
    with pytest.raises(AssertionError, match='iou_sum'):
        ops.bev_pq_counts(fg, fg, counts, total.float())
    with pytest.raises(AssertionError, match='capped'):
        ops.bev_pq_counts(fg, fg, counts, total, capped=torch.zeros(F, dtype=torch.int64))


def test_entry_points_validate_before_touching_the_device():
    """bad arguments come back as MUVO_ERR_INVALID_ARG with a message; nothing is launched (this runs without a GPU)"""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    i64, p, null, st = C.c_int64, C.c_void_p(4096), C.c_void_p(0), C.c_void_p(0)
    need = L.muvo_bev_instance_ws_bytes(i64(3), 37, 53)
    assert need == 16 + 3 * 37 * 53 * 8
    assert L.muvo_bev_instance_ws_bytes(i64(0), 4, 4) == -1 and L.muvo_bev_instance_ws_bytes(i64(65536), 4, 4) == -1
    assert L.muvo_bev_instance_ws_bytes(i64(1), 4097, 4) == -1 and L.muvo_bev_instance_ws_bytes(i64(1), 4096, 4097) == -1

    def dec(F=3, H=37, W=53, c=p, o=p, lg=p, Cn=8, fg=null, T=0.1, r=1, K=100, ws=p, wsb=need, ids=p, cen=p, n=p, cap=p):
        return L.muvo_bev_instance_decode(c, o, lg, Cn, C.c_uint32(24), fg, i64(F), H, W, C.c_float(T), r, K, ws, i64(wsb), ids, cen, n, cap, st)
    for kw, msg in (({'F': 0}, b'65535'), ({'F': 65536}, b'65535'), ({'H': 0}, b'4096'), ({'W': 4097}, b'4096'), ({'K': 0}, b'1..254'), ({'K': 255}, b'1..254'),
                    ({'r': 0}, b'1..3'), ({'r': 4}, b'1..3'), ({'Cn': 1}, b'2..32'), ({'Cn': 33}, b'2..32'), ({'T': float('nan')}, b'NaN'),
                    ({'lg': null}, b'either logits'), ({'fg': p}, b'either logits'), ({'c': null}, b'null pointer'), ({'o': null}, b'null pointer'),
                    ({'ids': null}, b'null pointer'), ({'cen': null}, b'null pointer'), ({'n': null}, b'null pointer'), ({'cap': null}, b'null pointer'),
                    ({'ws': null}, b'workspace'), ({'wsb': need - 1}, b'workspace'), ({'ws': C.c_void_p(4100)}, b'workspace'),
                    ({'c': C.c_void_p(4098)}, b'4-byte')):
        assert dec(**kw) == -1 and msg in L.muvo_last_error(), (kw, L.muvo_last_error())
    pqn = L.muvo_bev_pq_ws_bytes(i64(3))
    assert pqn == 3 * (65536 * 4 + 8) and L.muvo_bev_pq_ws_bytes(i64(0)) == -1 and L.muvo_bev_pq_ws_bytes(i64(65536)) == -1

    def pq(F=3, H=37, W=53, g=p, q=p, cap=null, counts=p, total=p, ws=p, wsb=pqn):
        return L.muvo_bev_pq_counts(g, q, cap, i64(F), H, W, counts, total, ws, i64(wsb), st)
    for kw, msg in (({'F': 0}, b'65535'), ({'H': 4097}, b'4096'), ({'g': null}, b'null pointer'), ({'q': null}, b'null pointer'),
                    ({'counts': null}, b'null pointer'), ({'total': null}, b'null pointer'), ({'ws': null}, b'workspace'), ({'wsb': pqn - 1}, b'workspace'),
                    ({'counts': C.c_void_p(4100)}, b'8-byte'), ({'cap': C.c_void_p(4098)}, b'4-byte')):
        assert pq(**kw) == -1 and msg in L.muvo_last_error(), (kw, L.muvo_last_error())


# ------------------------------------------------------------------------------------------------ the switches
def test_predict_refuses_the_switches_outside_mode_test():
    from muvo_amd import config
    from muvo_amd import predict as P
    for flag in ('--bev-pq', '--inst'):
        with pytest.raises(SystemExit, match='--bev-pq and --inst go with --mode test'):
            P.parse_args(['--config-file', 'x.yml', '--out', 'o', '--mode', 'sim', flag])
    with pytest.raises(SystemExit, match='--inst goes with --panels N'):
        P.parse_args(['--config-file', 'x.yml', '--out', 'o', '--mode', 'test', '--inst'])
    with pytest.raises(SystemExit, match='--inst-max-centres'):
        P.parse_args(['--config-file', 'x.yml', '--out', 'o', '--mode', 'test', '--bev-pq', '--inst-max-centres', '255'])
    args = P.parse_args(['--config-file', 'x.yml', '--out', 'o', '--mode', 'test', '--bev-pq', '--panels', '1', '--inst', '--inst-threshold', '0.3'])
    assert args.bev_pq is True and args.inst is True and args.inst_threshold == 0.3 and args.inst_max_centres == 100
    # the bird's-eye-view head off: refused before a batch is touched
    module = types.SimpleNamespace(panel_writer=None, traj_panels=False, traj_options={}, flow_panels=False, voxel_panels=False, voxel_options={})
    cfg = config.get_cfg(cfg_dict={'SEMANTIC_SEG': {'ENABLED': False}})
    for kw in ({'bev_pq': {}}, {'inst': True}, {'inst': {}}):
        with pytest.raises(ValueError, match='need the bird\'s-eye-view head'):
            P._run_test(cfg, module, {}, 'unused', None, 500, 0, None, print, **kw)
    assert not hasattr(module, 'inst_panels')


def test_train_forwards_the_switch():
    from muvo_amd import train as T
    assert T.build_parser().parse_args(['--panel-dir', 'd', '--inst']).inst is True
    assert T.build_parser().parse_args([]).inst is False
