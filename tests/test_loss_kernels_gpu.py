"""-m gpu: the loss and AdamW kernels of muvo_amd/csrc/losses.hip, through muvo_amd.ops, against the float64 references of
tests/loss_reference.py with its normalised error and its bars (4 x the error of the float32 CPU evaluation of the same
reference; tests/test_loss_reference.py shows on the CPU that these bars reject planted errors).  The case lists live in
loss_reference.py; every id is built from path(), the restatement of the launch arithmetic, and every case asserts the path
properties it exists for.  Each case prints `LOSSSTAT <id> <name>: max_e rms (bar)` lines.

Cross entropy and label 255: the reference project's F.cross_entropy raises on a label >= C, so it defines nothing there.  In
the cases that contain 255, CE and its gradient are held to the kernel's own documented rule (a term only for label < C, divisor
always F * V, gradient 0 for such voxels) evaluated in float64; SemScal and GeoScal are held to the reference."""
import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu


def _judge(tag, cmp):
    for line in R.statlines(tag, cmp):
        print(line)
    bad = R.failures(cmp)
    assert not bad, f'{tag}: ' + '; '.join(f'{n} max_e {s["max_e"]:.3e} at {s["index"]} (bar {cmp[n][1]:.2e})' for n, s in bad.items())


def _place(t, dev, off, grad=False):
    """`t` on the device in a fresh buffer, starting `off` elements after the buffer's (at least 256-byte aligned) start and
    four guard elements; returns (buffer, contiguous view of t's shape)"""
    n = t.numel()
    buf = torch.zeros(n + 12, dtype=t.dtype, device=dev)
    buf[4 + off:4 + off + n] = t.reshape(-1).to(dev)
    if grad:
        buf.requires_grad_(True)
    return buf, buf[4 + off:4 + off + n].view(t.shape)


def _inner(buf, off, shape):
    n = 1
    for s in shape:
        n *= s
    return buf[4 + off:4 + off + n].view(shape)


# ------------------------------------------------------------------------------------------------ voxel CE + SemScal + GeoScal
def _assert_content(case, lab, ref):
    """the float64 reference took the branches the case is there for"""
    C, content = case['C'], case['content']
    f = R.voxel_label_facts(lab, C)
    nan = {k: bool(torch.isnan(ref[k])) for k in ('ce', 'sem', 'geo')}
    if content == 'mix':
        assert f['M'] == lab.numel()
        if case['V'] >= 8191:          # (a frame of 1, 3 or 5 voxels takes whatever branches its few labels give)
            assert f['count'] == C and not any(nan.values())
    elif content == 'absent':
        assert f['T'][C - 1] == 0 and f['count'] == C - 1 and not any(nan.values())
    elif content == 'one':
        assert f['T'][1] == f['M'] > 0 and f['R'][1] == 0 and f['count'] == 1
        assert nan['geo'] and not nan['sem'] and not nan['ce']          # GeoScal: specificity 0 / 0, as in the reference
    elif content == 'all255':
        assert f['M'] == 0 and f['count'] == 0 and nan['sem'] and nan['geo']
        assert float(ref['ce']) == 0.0 and not ref['dlogits'].any()
    elif content == 'half255':
        assert 0.4 < 1 - f['M'] / lab.numel() < 0.6 and f['count'] == C and not any(nan.values())
    elif content == 'tail255':
        V = case['V']
        assert bool((lab[:, V - (V % 4 or 4):] == 255).all()) and f['M'] == lab.numel() - lab.shape[0] * (V % 4 or 4)
    elif content == 'oneframe':
        assert bool((lab[0] == 255).all()) and bool((lab[2:] == 255).all()) and f['M'] == case['V']


@pytest.mark.parametrize('case', R.VOXEL_CASES, ids=R.voxel_id)
def test_voxel_losses(dev, case):
    from muvo_amd import ops
    from muvo_amd.losses import VOXEL_SEG_WEIGHTS
    assert tuple(VOXEL_SEG_WEIGHTS) == R.PROD_W9
    fwd, bwd = R.voxel_paths(case)
    R.check_expect(case['expect'], {'fwd': fwd, 'bwd': bwd})
    nf, C, V = case['F'], case['C'], case['V']
    logits, lab, cw = R.voxel_inputs(case)
    ref = R.voxel_reference(logits, lab, cw)
    _assert_content(case, lab, ref)
    lo = 1 if case['offset'] in ('logits', 'both') else 0
    bo = 1 if case['offset'] in ('labels', 'both') else 0
    lbuf, lg = _place(logits.view(1, nf, C, V), dev, lo, grad=True)
    _, lb = _place(lab.view(1, nf, 1, V), dev, bo)
    assert (lg.data_ptr() % 16 == 0) == (lo == 0) and (lb.data_ptr() % 4 == 0) == (bo == 0)
    out = ops.voxel_losses(lg, lb, R.VOXEL_WEIGHT, None if cw is None else cw.to(dev))
    (R.VOXEL_GOUT[0] * out[0] + R.VOXEL_GOUT[1] * out[1] + R.VOXEL_GOUT[2] * out[2]).backward()
    grad = lbuf.grad
    got = {'ce': out[0], 'sem': out[1], 'geo': out[2], 'dlogits': _inner(grad, lo, (nf, C, V))}
    assert not grad[:4 + lo].any() and not grad[4 + lo + nf * C * V:].any(), 'gradient written outside the view'
    _judge(R.voxel_id(case), R.compare('voxel', got, ref))


@pytest.mark.parametrize('nf,C,V', [(2, 1, 8), (2, 17, 8), (65536, 2, 1)], ids=['C1', 'C17', 'F65536'])
def test_voxel_losses_argument_errors(dev, nf, C, V):
    """rejected by the argument checks of the launcher (an error code, an exception in Python): nothing is launched"""
    from muvo_amd import ops
    logits = torch.zeros(1, nf, C, V, device=dev)
    lab = torch.zeros(1, nf, 1, V, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='voxel_loss_fwd'):
        ops.voxel_losses(logits, lab, 1.0)


# ------------------------------------------------------------------------------------------------ spatial regression
@pytest.mark.parametrize('case', R.SPATIAL_CASES, ids=R.spatial_id)
def test_spatial_losses(dev, case):
    from muvo_amd import ops
    R.check_expect(case['expect'], {'': R.path('spatial_fwd', case['F'], 0, case['HW'], not case['offset'])})
    nf, Ct, HW = case['F'], case['Ct'], case['HW']
    pred, target, mask = R.spatial_inputs(case)
    ref = R.spatial_reference(case, pred, target, mask)
    off = 1 if case['offset'] else 0
    pbuf, pg = _place(pred.view(1, nf, Ct, 1, HW), dev, off, grad=True)
    _, tg = _place(target.view(1, nf, Ct, 1, HW), dev, off)
    assert (pg.data_ptr() % 16 == 0) == (off == 0) and (tg.data_ptr() % 16 == 0) == (off == 0)
    out = ops.spatial_losses(pg, tg, case['parts'], 255.0, None if mask is None else mask.view(1, nf, 1, 1, HW).to(dev))
    sum(g * out[i] for i, g in zip(range(len(case['parts'])), R.SPATIAL_GOUT)).backward()
    dpred = _inner(pbuf.grad, off, (nf, Ct, HW))
    got = {**{f'loss.{i}': out[i] for i in range(len(case['parts']))}, 'dpred': dpred}
    if case['ignore'] == 'all' or case['mask'] == 'zero':
        assert not out.detach().any() and not dpred.any()                                            # empty mask: exactly 0
        assert all(float(ref[f'loss.{i}']) == 0.0 for i in range(len(case['parts']))) and not ref['dpred'].any()
    covered = set(c for c0, c1, _, _ in case['parts'] for c in range(c0, c1))
    for c in set(range(Ct)) - covered:
        assert not dpred[:, c].any(), f'channel {c} is in no part: its gradient must be exactly 0'
    _judge(R.spatial_id(case), R.compare('spatial', got, ref))


# ------------------------------------------------------------------------------------------------ KL, L1, per-pixel CE
@pytest.mark.parametrize('case', R.KL_CASES, ids=lambda c: 'kl-B%dT%dS%d-alpha%g' % c)
def test_kl_loss(dev, case):
    from muvo_amd import ops
    inputs = R.kl_inputs(case)
    ref = R.kl_reference(case, inputs)
    leaves = [v.to(dev).requires_grad_(True) for v in inputs]
    out = ops.kl_loss(*leaves, R.KL_WEIGHT, case[3])
    (R.KL_GOUT * out[0]).backward()
    got = {'loss': out[0], 'dpm': leaves[0].grad, 'dps': leaves[1].grad, 'dqm': leaves[2].grad, 'dqs': leaves[3].grad}
    if case[3] == 1.0:
        assert not got['dqm'].any() and not got['dqs'].any()
    if case[3] == 0.0:
        assert not got['dpm'].any() and not got['dps'].any()
    _judge('kl-B%dT%dS%d-alpha%g' % case, R.compare('kl', got, ref))


def test_kl_loss_needs_two_steps(dev):
    from muvo_amd import ops
    t = [torch.ones(2, 1, 8, device=dev) for _ in range(4)]
    with pytest.raises(RuntimeError, match='T >= 2'):
        ops.kl_loss(*t, 1.0, 0.75)
    with pytest.raises(ValueError):
        R.kl64(*[v.cpu() for v in t], 1.0, 0.75)


@pytest.mark.parametrize('case', R.L1_CASES, ids=lambda c: 'l1-%dx%d' % c)
def test_l1_rows_loss(dev, case):
    from muvo_amd import ops
    p, t = R.l1_inputs(case)
    ref = R.l1_reference(case, p, t)
    assert int((ref['dp'] == 0).sum()) >= case[0] // 3 * case[1]         # the p == t elements: sign 0
    pg = p.to(dev).requires_grad_(True)
    out = ops.l1_rows_loss(pg, t.to(dev), 1.0)
    (R.L1_GOUT * out[0]).backward()
    assert bool((pg.grad.cpu()[::3] == 0).all())
    _judge('l1-%dx%d' % case, R.compare('l1', {'loss': out[0], 'dp': pg.grad}, ref))


@pytest.mark.parametrize('case', R.SEGCE_CASES, ids=lambda c: 'segce-N%dC%dHW%d-w%s' % c)
def test_seg_ce_pixel_loss(dev, case):
    from muvo_amd import ops
    logits, t, cw, gloss = R.segce_inputs(case)
    ref = R.segce_reference(case, logits, t, cw, gloss)
    lg = logits.to(dev).requires_grad_(True)
    out = ops.seg_ce_pixel_loss(lg, t.to(dev), None if cw is None else cw.to(dev))
    (out * gloss.to(dev)).sum().backward()
    invalid = t >= case[1]
    assert invalid.any() and not out.cpu()[invalid].any()                # label >= C: loss and gradient exactly 0
    assert not lg.grad.cpu().permute(0, 2, 1)[invalid].any()
    _judge('segce-N%dC%dHW%d-w%s' % case, R.compare('segce', {'map': out, 'dlogits': lg.grad}, ref))


# ------------------------------------------------------------------------------------------------ AdamW
GUARD = 12345.0


def _adamw_run(ops, dev, case, inputs, off):
    p0, m0, v0, grads = inputs
    n = case['n']
    bufs, views = [], []
    for t in (p0, m0, v0):
        buf = torch.full((n + 12,), GUARD, device=dev)
        buf[4 + off:4 + off + n] = t.to(dev)
        bufs.append(buf)
        views.append(buf[4 + off:4 + off + n])
    for step, g in zip(case['steps'], grads):
        _, gv = _place(g, dev, off)
        assert all((v.data_ptr() % 16 == 0) == (off == 0) for v in views + [gv])
        ops.adamw_step(views[0], gv, views[1], views[2], R.ADAMW_HP['lr'], R.ADAMW_HP['beta1'], R.ADAMW_HP['beta2'],
                       R.ADAMW_HP['eps'], case['wd'], step, case['grad_scale'])
    for buf in bufs:           # elements just outside the updated range are untouched
        assert bool((buf[:4 + off] == GUARD).all()) and bool((buf[4 + off + n:] == GUARD).all()), 'AdamW wrote outside its range'
    return {'p': views[0].clone(), 'm': views[1].clone(), 'v': views[2].clone()}


@pytest.mark.parametrize('case', R.ADAMW_CASES, ids=R.adamw_id)
def test_adamw_step(dev, case):
    from muvo_amd import ops
    off = 1 if case['offset'] else 0
    R.check_expect(case['expect'], {'': R.path('adamw', 0, 0, case['n'], not case['offset'])})
    inputs = R.adamw_inputs(case)
    ref = R.adamw_reference(case, *inputs)
    if case['zeros']:
        assert bool((ref['v'][::3] == 0).all()) and case['steps'][0] == 1       # v == 0: the denominator is eps alone
    got = _adamw_run(ops, dev, case, inputs, off)
    _judge(R.adamw_id(case), R.compare('adamw', got, ref, lr=R.ADAMW_HP['lr']))
    if case['offset']:
        # the same data through the vector kernel (aligned) and the scalar kernel (this view): the vector kernel promises the scalar
        # kernel's order of operations, so the results are bit-identical
        assert R.path('adamw', 0, 0, case['n'], True)['vec']
        aligned = _adamw_run(ops, dev, case, inputs, 0)
        for k in ('p', 'm', 'v'):
            assert torch.equal(aligned[k], got[k]), f'{k}: vector and scalar AdamW kernels differ'
