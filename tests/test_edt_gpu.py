"""-m gpu: the distance-transform unit (muvo_amd/csrc/edt.hip through ops.voxel_edt, ops.voxel_boundary_loss / _parts,
ops.voxel_cd_counts, losses.BoundaryLoss, WorldModelTrainer.compute_loss and predict.run) against the restatement of
tests/edt_reference.py.  The transform, the prediction's class grid, n_G and every integer count must EQUAL the restatement.  The
loss and dlogits are judged as absolute errors against the float64 evaluation; each bar is 4 x the error of the float32 evaluation
of the same restatement on the same input, computed here; where that error is 0 the bar of the general case of the same shape and
C stands in.  The fp64 sums of the metric agree to 1.2e-10 relative: n 2^-53 for n < 2^20 addends in arbitrary order, each addend a
correctly rounded sqrt of an exact integer.  Inputs sit inside guard buffers at odd element offsets.  Each loss case prints
`EDTSTAT <id> <name>: error (bar)` lines.

Measured on one MI355X (error, bar), worst over the cases of a kind: see DESIGN.md section 15."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import edt_reference as E
import lovasz_reference as LV

pytestmark = pytest.mark.gpu
GUARD = {torch.float32: 12345.0, torch.uint8: 77}
GOUT = -1.5
GROUPS = (('empty', 'full', 'first'), ('last', 'plane', 'random'), ('unknown', 'only_unknown', 'random'))
EDT_SHAPES = [(5, 7, 3), (33, 17, 9), (70, 6, 4), (6, 70, 4), (4, 6, 70), (1, 1, 1)]
LOSS_SHAPES = {'13x10x7': (13, 10, 7), '8x8x8': (8, 8, 8)}
LOSS_CASES = [(s, C, T) for s in LOSS_SHAPES for C in (2, 9) for T in (1, 3, 20)]


def _place(t, dev, off, grad=False):
    """`t` on the device inside a fresh buffer of guard values, `off` elements after four guard elements; returns (buffer,
    contiguous view of t's shape)"""
    n = t.numel()
    buf = torch.full((n + 12,), GUARD[t.dtype], dtype=t.dtype, device=dev)
    buf[4 + off:4 + off + n] = t.reshape(-1).to(dev)
    if grad:
        buf.requires_grad_(True)
    return buf, buf[4 + off:4 + off + n].view(t.shape)


def _guards_intact(buf, off, n):
    b = buf.detach()
    return bool((b[:4 + off] == GUARD[b.dtype]).all()) and bool((b[4 + off + n:] == GUARD[b.dtype]).all())


def _caps(shape):
    return (1, 9, 25, E.full_cap(shape), E.full_cap(shape) + 5)


# ------------------------------------------------------------------------------------------------ the transform
@functools.lru_cache(maxsize=None)
def _edt_frames(shape, group):
    return np.stack([E.scene(kind, shape, seed=17 + 3 * i + len(group[0])) for i, kind in enumerate(group)])


@pytest.mark.parametrize('shape', EDT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_transform_equals_the_restatement_on_every_cell(dev, shape):
    """three frames of different content per call; caps on both sides of the window / whole-column boundary of every axis"""
    from muvo_amd import ops
    for group in GROUPS:
        frames = _edt_frames(shape, group)
        buf, grid = _place(torch.from_numpy(frames), dev, 1 + len(group[0]) % 2 * 2)
        for cap in _caps(shape):
            got = ops.voxel_edt(grid, cap)
            assert got.dtype == torch.int32 and tuple(got.shape) == frames.shape
            want = E.edt2(frames, cap)
            assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (group, cap)
            for f, kind in enumerate(group):
                if kind in ('empty', 'only_unknown'):
                    assert (want[f] == cap).all()
        assert _guards_intact(buf, 1 + len(group[0]) % 2 * 2, frames.size), 'an input guard element changed'
        assert np.array_equal(grid.cpu().numpy(), frames), 'the grid changed'


def test_transform_at_the_coarsest_real_level(dev):
    from muvo_amd import ops
    shape = (48, 48, 16)
    frames = np.stack([E.scene('random', shape, seed=5), E.scene('unknown', shape, seed=6)])
    buf, grid = _place(torch.from_numpy(frames), dev, 3)
    for cap in _caps(shape):
        assert np.array_equal(ops.voxel_edt(grid, cap).cpu().numpy().astype(np.int64), E.edt2(frames, cap)), cap
    assert _guards_intact(buf, 3, frames.size)
    # frames are independent: each frame alone gives its part of the stack
    both = ops.voxel_edt(grid, 25)
    for f in range(2):
        assert torch.equal(ops.voxel_edt(grid[f:f + 1], 25)[0], both[f])


def test_transform_refuses_bad_arguments_without_a_launch(dev):
    import ctypes as C
    from muvo_amd import ops
    g = torch.zeros(1, 2, 2, 2, dtype=torch.uint8, device=dev)
    for cap in (0, -3, 2 ** 31):
        with pytest.raises(ValueError, match='voxel_edt'):
            ops.voxel_edt(g, cap)
    with pytest.raises(ValueError, match='voxel_edt'):
        ops.voxel_edt(torch.zeros(1, 0, 2, 2, dtype=torch.uint8, device=dev), 4)
    with pytest.raises(ValueError, match='voxel_edt'):
        ops.voxel_edt(torch.zeros(2, 2, 2, dtype=torch.uint8, device=dev), 4)
    L = ops.lib()
    out = torch.full((8,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(32, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    null = C.c_void_p(0)
    for args in ((null, p(ws), p(out)), (p(g), null, p(out)), (p(g), p(ws), null)):
        assert L.muvo_voxel_edt(args[0], C.c_int64(1), 2, 2, 2, C.c_int32(4), args[1], C.c_int64(32), args[2], C.c_void_p(0)) == -1
        assert b'null pointer' in L.muvo_last_error()
    assert L.muvo_voxel_edt(p(g), C.c_int64(1), 2, 2, 2, C.c_int32(0), p(ws), C.c_int64(32), p(out), C.c_void_p(0)) == -1
    assert L.muvo_voxel_edt(p(g), C.c_int64(1), 2, 0, 2, C.c_int32(4), p(ws), C.c_int64(32), p(out), C.c_void_p(0)) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all()), 'a refused call wrote its output'


# ------------------------------------------------------------------------------------------------ the loss
@functools.lru_cache(maxsize=None)
def _loss_inputs(shape_id, C, kind='general'):
    """four frames: a shell of several classes, a label with 255s, an empty label, a plane"""
    shape = LOSS_SHAPES[shape_id]
    rng = np.random.default_rng(len(shape_id) + C)
    labels = np.stack([E.scene('random', shape, seed=21), E.scene('unknown', shape, seed=22), np.zeros(shape, np.uint8), E.scene('plane', shape)])
    labels[0][labels[0] > 0] = rng.integers(1, C, int((labels[0] > 0).sum()))
    logits = (2 * rng.standard_normal((4, C, *shape))).astype(np.float32)
    if kind == 'x40':
        logits = E.saturated(logits)
    return logits, labels


@functools.lru_cache(maxsize=None)
def _reference(shape_id, C, T, kind='general'):
    """(float64 reference, the float32 errors every bar is 4 x of)"""
    logits, labels = _loss_inputs(shape_id, C, kind)
    ref = E.loss_and_grad(logits, labels, T, E.WEIGHT)
    low = E.loss_and_grad(logits, labels, T, E.WEIGHT, dtype=np.float32)
    err = {'loss': abs(float(low['loss']) - float(ref['loss'])), 'dlogits': float(np.abs(low['dlogits'].astype(np.float64) - ref['dlogits']).max())}
    return ref, low, err


def _bars(shape_id, C, T, kind):
    err = _reference(shape_id, C, T, kind)[2]
    general = _reference(shape_id, C, T, 'general')[2]
    return {k: 4 * (e if e > 0 else general[k]) for k, e in err.items()}


def _run(dev, logits, labels, T, offsets=(1, 3), weight=E.WEIGHT, gout=GOUT, parts=True):
    """ops.voxel_boundary_loss forward + backward (and ops.voxel_boundary_parts) on numpy inputs placed at element offsets inside
    guard buffers; checks that nothing outside the views was written"""
    from muvo_amd import ops
    F, C = logits.shape[:2]
    shape = logits.shape[2:]
    l6 = torch.from_numpy(logits).view(1, F, C, *shape)
    t6 = torch.from_numpy(labels).view(1, F, 1, *shape)
    lo, to = offsets
    lbuf, lg = _place(l6, dev, lo, grad=True)
    tbuf, tg = _place(t6, dev, to)
    out = ops.voxel_boundary_loss(lg, tg, T, weight)
    assert out.shape == (1,) and out.dtype == torch.float32
    (gout * out[0]).backward()
    grad = lbuf.grad
    assert not grad[:4 + lo].any() and not grad[4 + lo + logits.size:].any(), 'gradient written outside the view'
    got = {'loss': float(out[0].detach().cpu().double()), 'loss_bits': out.detach().cpu(),
           'dlogits': grad[4 + lo:4 + lo + logits.size].view(F, C, *shape).cpu().numpy()}
    if parts:
        eg, ep, pred, n_g = ops.voxel_boundary_parts(lg, tg, T)
        got.update(edt_label=eg.cpu().numpy(), edt_pred=ep.cpu().numpy(), pred=pred.cpu().numpy(), n_g=n_g.cpu().numpy())
    assert _guards_intact(lbuf, lo, logits.size) and _guards_intact(tbuf, to, labels.size), 'an input guard element changed'
    return got


def _judge(tag, got, ref, bars, labels, gout=GOUT):
    assert np.array_equal(got['edt_label'].astype(np.int64), ref['edt_label']), f'{tag}: edt2 of the label'
    assert np.array_equal(got['pred'], ref['pred']), f'{tag}: the predicted class grid'
    assert np.array_equal(got['edt_pred'].astype(np.int64), ref['edt_pred']), f'{tag}: edt2 of the prediction'
    assert np.array_equal(got['n_g'].astype(np.int64), ref['n_g']), f'{tag}: n_G'
    errs = {'loss': abs(got['loss'] - float(ref['loss'])), 'dlogits': float(np.abs(got['dlogits'] - gout * ref['dlogits']).max())}
    all_bars = dict(bars, dlogits=abs(gout) * bars['dlogits'])
    for k, e in errs.items():
        print(f'EDTSTAT {tag} {k}: {e:.3e} ({all_bars[k]:.3e})')
    assert np.isfinite(got['loss']) and np.isfinite(got['dlogits']).all()
    assert not np.moveaxis(got['dlogits'], 1, 0)[:, labels == 255].any(), f'{tag}: gradient on a 255 cell'
    assert not got['dlogits'][ref['n_g'] == 0].any(), f'{tag}: gradient on a frame without a label cell'
    bad = {k: e for k, e in errs.items() if not e <= all_bars[k]}
    assert not bad, f'{tag}: ' + '; '.join(f'{k} {e:.3e} over its bar {all_bars[k]:.3e}' for k, e in bad.items())


@pytest.mark.parametrize('shape_id,C,T', LOSS_CASES, ids=[f'{s}-C{C}-T{T}' for s, C, T in LOSS_CASES])
def test_boundary_loss_cases(dev, shape_id, C, T):
    """four different frames per call; 13 x 10 x 7 takes the guarded scalar path of the dense passes (V = 910 is no multiple of 4,
    and the bases are odd), 8 x 8 x 8 at offsets (0, 0) the 16-byte path; T = 20 exceeds both grids"""
    logits, labels = _loss_inputs(shape_id, C)
    ref, _, _ = _reference(shape_id, C, T)
    assert ref['n_g'][2] == 0 and (labels[1] == 255).sum() >= 50 and ref['n_g'][[0, 1, 3]].min() > 0
    got = _run(dev, logits, labels, T, offsets=(0, 0) if shape_id == '8x8x8' else (1, 3))
    _judge(f'{shape_id}-C{C}-T{T}', got, ref, _bars(shape_id, C, T, 'general'), labels)


def test_unaligned_bases_equal_the_aligned_call(dev):
    logits, labels = _loss_inputs('8x8x8', 9)
    ref, _, _ = _reference('8x8x8', 9, 3)
    got = _run(dev, logits, labels, 3, offsets=(1, 1))
    _judge('8x8x8-C9-T3-unaligned', got, ref, _bars('8x8x8', 9, 3, 'general'), labels)
    aligned = _run(dev, logits, labels, 3, offsets=(0, 0), parts=False)
    assert torch.equal(aligned['loss_bits'], got['loss_bits']) and aligned['dlogits'].tobytes() == got['dlogits'].tobytes()


@pytest.mark.parametrize('T', [1, 3, 20])
def test_saturated_logits_give_the_hard_set_expression(dev, T):
    """logits x 40 (edt_reference.saturated): p is 0 or 1 in float32 and the loss is sum_f (sum_{P \\ G} dG + sum_{G \\ P} dP) / n_G
    formed from ops.voxel_edt outputs alone"""
    from muvo_amd import ops
    logits, labels = _loss_inputs('13x10x7', 9, 'x40')
    ref, low, err = _reference('13x10x7', 9, T, 'x40')
    assert set(np.unique(low['p']).tolist()) == {0.0, 1.0}
    bars = _bars('13x10x7', 9, T, 'x40')
    got = _run(dev, logits, labels, T)
    print(f'EDTSTAT x40-T{T} float32 errors of the restatement: {err}')
    _judge(f'13x10x7-C9-T{T}-x40', got, ref, bars, labels)
    pred = ops.raycast_bricks(torch.from_numpy(logits).to(dev))[0]
    eg = ops.voxel_edt(torch.from_numpy(labels).to(dev), T * T).cpu().numpy()
    ep = ops.voxel_edt(pred, T * T).cpu().numpy()
    hard = E.hard_loss(eg, ep, labels, pred.cpu().numpy(), T, E.WEIGHT)
    e = abs(got['loss'] - hard)
    print(f'EDTSTAT x40-T{T} loss against the hard-set expression: {e:.3e} ({bars["loss"]:.3e})')
    assert hard > 0 and e <= bars['loss']


def test_second_call_is_bit_identical_in_both_modes(dev):
    from muvo_amd import ops
    logits, labels = _loss_inputs('13x10x7', 9)
    first = _run(dev, logits, labels, 3, parts=False)
    second = _run(dev, logits, labels, 3, parts=False)
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        det = _run(dev, logits, labels, 3, parts=False)
    finally:
        ops.set_deterministic(was)
    for other in (second, det):
        assert torch.equal(first['loss_bits'], other['loss_bits']) and first['dlogits'].tobytes() == other['dlogits'].tobytes()


def test_no_label_cell_gives_zero_loss_and_zero_gradient(dev):
    logits, _ = _loss_inputs('13x10x7', 2)
    labels = np.zeros((4, 13, 10, 7), np.uint8)
    labels[1] = 255
    got = _run(dev, logits, labels, 3)
    assert got['loss'] == 0.0 and not got['dlogits'].any() and np.isfinite(got['dlogits']).all() and not got['n_g'].any()
    assert (got['edt_label'] == 9).all()


def test_no_grad_terms_and_module(dev):
    from muvo_amd import ops
    from muvo_amd.losses import BoundaryLoss
    logits, labels = _loss_inputs('8x8x8', 9)
    F, C = logits.shape[:2]
    l6 = torch.from_numpy(logits).view(1, F, C, 8, 8, 8).to(dev).requires_grad_(True)
    t6 = torch.from_numpy(labels).view(1, F, 1, 8, 8, 8).to(dev)
    with_grad = ops.voxel_boundary_loss(l6, t6, 3, 1.0)
    with torch.no_grad():
        without = ops.voxel_boundary_loss(l6, t6, 3, 1.0)
    term = ops.voxel_boundary_loss(l6, t6, 3, 1.0, terms=True)
    assert isinstance(term, tuple) and len(term) == 1 and term[0].dim() == 0
    assert with_grad.requires_grad and not without.requires_grad and without.grad_fn is None
    assert torch.equal(with_grad.detach(), without) and torch.equal(term[0].detach(), without[0])
    a = BoundaryLoss(3)(l6, t6)
    ga, = torch.autograd.grad(a, l6)
    gb, = torch.autograd.grad(with_grad[0], l6, retain_graph=True)
    assert a.dim() == 0 and torch.equal(a.detach(), without[0]) and torch.equal(ga, gb)
    with pytest.raises(ValueError, match='2..16 classes'):
        ops.voxel_boundary_loss(torch.zeros(1, 1, 17, 2, 2, 2, device=dev), torch.zeros(1, 1, 1, 2, 2, 2, dtype=torch.uint8, device=dev), 3, 1.0)
    with pytest.raises(ValueError, match='truncation'):
        ops.voxel_boundary_loss(torch.zeros(1, 1, 2, 2, 2, 2, device=dev), torch.zeros(1, 1, 1, 2, 2, 2, dtype=torch.uint8, device=dev), 0, 1.0)


# ------------------------------------------------------------------------------------------------ the metric
def _metric_grids():
    shape = (13, 10, 7)
    plane = E.scene('plane', shape)
    label = np.stack([E.scene('random', shape, seed=31), plane, E.scene('random', shape, seed=33), np.zeros(shape, np.uint8),
                      E.scene('unknown', shape, seed=35), E.scene('first', shape)])
    pred = np.stack([E.scene('random', shape, seed=32), np.roll(plane, 3, axis=1), np.full(shape, 255, np.uint8), E.scene('random', shape, seed=34),
                     E.scene('random', shape, seed=36), E.scene('last', shape)])
    return label, pred


def test_cd_counts_equal_the_restatement(dev):
    from muvo_amd import ops
    label, pred = _metric_grids()
    thr = [4, 25, 100]
    want, sums, n = E.cd_counts(label, pred, thr)
    assert want[1] == 2 and want[0] == 4 and 0 < want[4] < want[5] <= want[6] <= want[2] and 0 < want[7] < want[9] <= want[3] and n < 2 ** 20
    lbuf, lg = _place(torch.from_numpy(label), dev, 1)
    pbuf, pg = _place(torch.from_numpy(pred), dev, 3)
    counts = torch.zeros(10, dtype=torch.int64, device=dev)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    ops.voxel_cd_counts(lg, pg, thr, counts, acc)
    assert counts.cpu().tolist() == want.tolist()
    got = acc.cpu().numpy()
    assert (np.abs(got - sums) <= 1.2e-10 * sums).all() and (sums > 0).all(), (got, sums)
    # two calls add up to one call on the concatenation, and to twice the counts when repeated
    two_c = torch.zeros(10, dtype=torch.int64, device=dev)
    two_s = torch.zeros(2, dtype=torch.float64, device=dev)
    ops.voxel_cd_counts(lg[:2], pg[:2], thr, two_c, two_s)
    ops.voxel_cd_counts(lg[2:], pg[2:], thr, two_c, two_s)
    assert torch.equal(two_c, counts) and bool(((two_s - acc).abs() <= 1.2e-10 * acc).all())
    ops.voxel_cd_counts(lg, pg, thr, counts, acc)
    assert counts.cpu().tolist() == (2 * want).tolist() and (np.abs(acc.cpu().numpy() - 2 * sums) <= 1.2e-10 * 2 * sums).all()
    assert _guards_intact(lbuf, 1, label.size) and _guards_intact(pbuf, 3, pred.size)
    # an aligned grid with V % 4 == 0 takes the vector path
    shape = (8, 8, 8)
    l8 = np.stack([E.scene('random', shape, seed=41), E.scene('plane', shape)])
    p8 = np.stack([E.scene('random', shape, seed=42), E.scene('unknown', shape, seed=43)])
    w8, s8, _ = E.cd_counts(l8, p8, thr)
    c8 = torch.zeros(10, dtype=torch.int64, device=dev)
    a8 = torch.zeros(2, dtype=torch.float64, device=dev)
    ops.voxel_cd_counts(torch.from_numpy(l8).to(dev), torch.from_numpy(p8).to(dev), thr, c8, a8)
    assert c8.cpu().tolist() == w8.tolist() and w8[0] == 2 and (np.abs(a8.cpu().numpy() - s8) <= 1.2e-10 * s8).all()


def test_voxel_distance_metric_over_two_batches(dev):
    from muvo_amd.voxel_view import VoxelDistanceMetric
    label, pred = _metric_grids()
    cfg = types.SimpleNamespace(VOXEL=types.SimpleNamespace(RESOLUTION=0.5))
    m = VoxelDistanceMetric(cfg)
    m.start_loader(2)
    rf = 4                                                                         # frames 0..3 reconstructed, 4..5 imagined

    def logits_of(grid):
        z = torch.zeros((1, grid.shape[0], 9, *grid.shape[1:]), device=dev)
        z.scatter_(2, torch.from_numpy(np.where(grid == 255, 0, np.minimum(grid, 8))).to(dev).long()[None, :, None], 5.0)
        return z
    hard = np.where(pred == 255, 0, np.minimum(pred, 8)).astype(np.uint8)        # the class grid those logits give
    for i in range(2):
        batch = {'voxel_label_1': torch.from_numpy(label[None, :, None]).to(dev)}
        m.update(i, batch, {'voxel_1': logits_of(pred[:rf])}, [{'voxel_1': logits_of(pred[rf:])}])
    res = m.result()
    thr = E.thresholds2(0.5)
    assert thr == [4, 16, 64]
    for tail, sl in (('', slice(0, rf)), ('_imagine', slice(rf, 6))):
        c, s, _ = E.cd_counts(label[sl], hard[sl], thr)
        assert res[f'test2_voxel_cd_frames{tail}'] == 2 * c[0] and res[f'test2_voxel_cd_skipped{tail}'] == 2 * c[1]
        assert res[f'test2_voxel_cd{tail}'] == pytest.approx(0.5 * (s[0] / c[2] + s[1] / c[3]), rel=1e-9)
        for k, t in enumerate((1, 2, 4)):
            assert res[f'test2_voxel_precision_{t}m{tail}'] == c[4 + k] / c[2] and res[f'test2_voxel_recall_{t}m{tail}'] == c[7 + k] / c[3]
    assert res['test2_voxel_cd_skipped'] == 4 and 0 < res['test2_voxel_fscore_1m'] <= res['test2_voxel_fscore_4m'] <= 1


# ------------------------------------------------------------------------------------------------ end to end
def test_compute_loss_with_the_key_on(dev):
    from muvo_amd.trainer import WorldModelTrainer
    batch, output = LV.voxel_dicts(device=dev, sizes=((8, 8, 4), (4, 4, 2), (2, 2, 1)), b=1, s=2, C=2)
    for v in output.values():
        v.requires_grad_(True)
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_BOUNDARY.WEIGHT': 0.5, 'LOSSES.VOXEL_BOUNDARY.FACTORS': [1, 4]})
    off = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=LV.voxel_only_cfg()), batch, output)
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
    assert list(losses) == list(off) + ['voxel_boundary_1', 'voxel_boundary_4']
    for k in ('voxel_boundary_1', 'voxel_boundary_4'):
        assert losses[k].dim() == 0 and bool(torch.isfinite(losses[k])) and float(losses[k].detach()) >= 0
        print(f'EDTSTAT compute-loss {k}: {float(losses[k].detach()):.6g}')
    assert float(losses['voxel_boundary_1'].detach()) > 0
    (losses['voxel_boundary_1'] + losses['voxel_boundary_4']).backward()
    assert output['voxel_1'].grad is not None and bool(output['voxel_1'].grad.abs().sum() > 0) and bool(torch.isfinite(output['voxel_1'].grad).all())
    assert output['voxel_4'].grad is not None and output['voxel_2'].grad is None


def test_predict_voxel_cd_leaves_the_metrics_alone(dev, tmp_path):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import ops
    from muvo_amd import predict as P
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path / 'rec')
    os.makedirs(root)
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(79)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    assert cfg.VOXEL_SEG.ENABLED

    def data():
        dm = DataModule(cfg, root, device=dev, seed=79)
        dm.setup()
        dm.test_sampler_0 = range(0, 4, 2)
        return dm
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'cd')
    lines = []
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        P.run(cfg, dev, a, 'test', loaders=[0], limit_batches=2, seed=79, data=data(), module=module, log=lambda s: None)
        out = P.run(cfg, dev, b, 'test', loaders=[0], limit_batches=2, seed=79, data=data(), module=module, log=lines.append, voxel_cd={})
    finally:
        ops.set_deterministic(was)
    assert open(os.path.join(a, 'metrics.json'), 'rb').read() == open(os.path.join(b, 'metrics.json'), 'rb').read()
    res = json.load(open(os.path.join(b, 'voxel_cd.json')))
    names = ['voxel_cd', 'voxel_cd_frames', 'voxel_cd_skipped'] + [f'voxel_{k}_{t}m' for k in ('precision', 'recall', 'fscore') for t in (1, 2, 4)]
    assert res == json.loads(json.dumps(out['voxel_cd'])) and set(res) == {f'test0_{k}{tail}' for k in names for tail in ('', '_imagine')}
    assert os.path.join(b, 'voxel_cd.json') in out['files'] and not os.path.exists(os.path.join(a, 'voxel_cd.json'))
    assert [s for s in lines if s.startswith('voxel_cd ')] == ['voxel_cd ' + json.dumps(res, sort_keys=True)]
    for tail, n in (('', 2 * 2), ('_imagine', 2 * 4 if cfg.PREDICTION.N_SAMPLES > 0 else 0)):
        assert res[f'test0_voxel_cd_frames{tail}'] + res[f'test0_voxel_cd_skipped{tail}'] == n
        assert np.isfinite(res[f'test0_voxel_cd{tail}']) and res[f'test0_voxel_cd{tail}'] >= 0
        for k in ('precision', 'recall'):
            assert 0.0 <= res[f'test0_voxel_{k}_1m{tail}'] <= res[f'test0_voxel_{k}_2m{tail}'] <= res[f'test0_voxel_{k}_4m{tail}'] <= 1.0
        assert all(0.0 <= res[f'test0_voxel_fscore_{t}m{tail}'] <= 1.0 for t in (1, 2, 4))
    with pytest.raises(ValueError, match='mode test'):
        P.run(cfg, dev, str(tmp_path / 'sim'), 'sim', loaders=[2], data=data(), module=module, log=lambda s: None, voxel_cd={})
