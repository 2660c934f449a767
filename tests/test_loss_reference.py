"""CPU: the float64 references, the metric, the bars and path() of tests/loss_reference.py, which tests/test_loss_kernels_gpu.py
applies to the loss and AdamW kernels.  Three things are shown here, without a GPU:
  * the new references agree with the oracle's loss functions (which the golden fixtures pin to the reference project) and with
    F.cross_entropy / torch.optim.AdamW;
  * the bars bite: results built from the float64 reference rounded to float32 with ONE planted error each (what a subtly wrong
    kernel would produce) are all rejected by the very comparison the GPU test uses, and the float32 CPU evaluation of the
    reference is accepted;
  * path() reproduces launches computed by hand from losses.hip, and the case lists reach every path the suite is there for."""
import pytest
import torch
import torch.nn.functional as F

import loss_reference as R


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize('dtype,tol', [(torch.float32, 16 * 2.0 ** -24), (torch.float64, 1e-11)], ids=['f32', 'f64'])
def test_references_agree_with_the_oracle(dtype, tol):
    from oracle import muvo_ref as O
    g = torch.Generator().manual_seed(3)
    nf, C, V = 3, 4, 6 * 5 * 4
    logits = torch.randn(nf, C, V, generator=g).to(dtype)
    lab = torch.randint(0, 3, (nf, V), generator=g).to(torch.uint8)           # class 3 absent
    cw = torch.tensor([1.0, 2.0, 0.5, 3.0])
    ce, _, _ = R.voxel_losses64(logits, lab, 1.0, cw, dtype=dtype)
    assert _rel(ce, F.cross_entropy(logits, lab.long(), weight=cw.to(dtype), reduction='none').mean()) <= tol
    lab[0, :7] = 255                                                          # SemScal / GeoScal mask 255
    _, sem, geo = R.voxel_losses64(logits, lab, 1.0, None, dtype=dtype)
    l5, t4 = logits.view(nf, C, 6, 5, 4), lab.view(nf, 6, 5, 4)
    assert _rel(sem, O._sem_scal(l5, t4)) <= tol and _rel(geo, O._geo_scal(l5, t4)) <= tol
    pred, target = torch.randn(nf, 4, 60, generator=g).to(dtype), torch.rand(nf, 4, 60, generator=g).to(dtype)
    target[0, 0, 5] = target[2, 3, 7] = 255.0
    got = R.spatial_loss64(pred, target, [(0, 3, 2, 1.0), (3, 4, 1, 1.0)], dtype=dtype)
    p5, t5 = pred.view(1, nf, 4, 6, 10), target.view(1, nf, 4, 6, 10)
    assert _rel(got[0], O._spatial_regression(p5[:, :, :3], t5[:, :, :3], 2)) <= tol
    assert _rel(got[1], O._spatial_regression(p5[:, :, -1:], t5[:, :, -1:], 1)) <= tol
    mask = torch.rand(nf, 60, generator=g) < 0.3
    got = R.spatial_loss64(pred, target, [(0, 4, 1, 1.0)], mask=mask, dtype=dtype)
    assert _rel(got[0], O._spatial_regression(p5, t5, 1, mask.view(1, nf, 1, 6, 10))) <= tol
    assert float(R.spatial_loss64(pred, target, [(0, 4, 1, 1.0)], mask=torch.zeros_like(mask), dtype=dtype)[0]) == 0.0
    pm, qm = (torch.randn(2, 4, 16, generator=g).to(dtype) for _ in range(2))
    ps, qs = (0.2 + torch.rand(2, 4, 16, generator=g).to(dtype) for _ in range(2))
    want = 0.75 * O._kl(pm, ps, qm, qs) + 0.25 * O._kl(pm, ps, qm, qs)
    assert _rel(R.kl64(pm, ps, qm, qs, 1.0, 0.75, dtype=dtype), want) <= tol


def test_kl_gradients_split_by_alpha():
    """the value is the same for every alpha; the prior side receives alpha, the posterior side 1 - alpha of the gradient"""
    inputs = R.kl_inputs((2, 3, 5, 0.75))
    full = [R.kl_reference((2, 3, 5, a), inputs) for a in (0.0, 0.75, 1.0)]
    assert _rel(full[0]['loss'], full[2]['loss']) < 1e-14
    assert not full[0]['dpm'].any() and not full[2]['dqs'].any()
    assert torch.allclose(full[1]['dpm'], 0.75 * full[2]['dpm'], rtol=1e-13, atol=0)
    assert torch.allclose(full[1]['dqs'], 0.25 * full[0]['dqs'], rtol=1e-13, atol=0)


def test_adamw64_is_torch_adamw():
    torch.manual_seed(5)
    n = 1000
    p0, grads = torch.randn(n, dtype=torch.float64), [torch.randn(n, dtype=torch.float64) * (k + 1) for k in range(3)]
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pr], lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p, m, v = p0, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step, g in enumerate(grads, 1):
        pr.grad = 0.125 * g
        opt.step()
        p, m, v = R.adamw64(p, g, m, v, 3e-4, 0.9, 0.999, 1e-8, 0.01, step, grad_scale=0.125)
    assert float((p - pr.data).abs().max()) <= 1e-14
    st = opt.state[pr]
    assert float((m - st['exp_avg']).abs().max()) <= 1e-15 and float((v - st['exp_avg_sq']).abs().max()) <= 1e-15


def test_seg_ce64_and_l1():
    g = torch.Generator().manual_seed(6)
    x, t = torch.randn(2, 5, 30, generator=g, dtype=torch.float64), torch.randint(0, 5, (2, 30), generator=g)
    cw = torch.tensor([1.0, 2.0, 3.0, 0.5, 1.5])
    want = F.cross_entropy(x, t, weight=cw.double(), reduction='none')
    t8 = t.to(torch.uint8)
    assert torch.equal(R.seg_ce64(x, t8, cw), want)
    t8[0, 3], t8[1, 4] = 5, 255
    got = R.seg_ce64(x, t8, cw)
    assert got[0, 3] == 0 and got[1, 4] == 0 and torch.equal(got[1, 5:], want[1, 5:])
    p, q = torch.randn(7, 3, generator=g), torch.randn(7, 3, generator=g)
    assert _rel(R.l1_rows64(p, q, 2.0), 2.0 * (p.double() - q.double()).abs().sum(-1, keepdim=True).mean()) < 1e-15


def test_error_stats_zero_and_nan_rules():
    ref = torch.tensor([0.0, 1.0, float('nan')], dtype=torch.float64)
    assert R.error_stats(torch.tensor([0.0, 1.0, float('nan')]), ref, 1.0)['max_e'] == 0.0
    assert R.error_stats(torch.tensor([0.0, 1.0, 0.5]), ref, 1.0)['max_e'] == float('inf')            # NaN expected
    assert R.error_stats(torch.tensor([float('nan'), 1.0, float('nan')]), ref, 1.0)['max_e'] == float('inf')
    s = R.error_stats(torch.tensor([1e-30, 1.0, float('nan')]), ref, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
    assert s['max_e'] > 1e200 and s['index'] == (0,)                                                   # den 0: exactly 0 demanded
    assert R.scale_of(ref) == 1.0 and R.scale_of(torch.tensor([float('nan')])) == 0.0


# ------------------------------------------------------------------------------------------------ the bars
def test_bars_come_from_the_float32_evaluation():
    for fam, bar in R.BARS.items():
        floor = R.SCALAR_FLOOR if fam.endswith('_loss') else 0.0
        assert bar == max(4 * R.MEASURED[fam], floor), fam
        assert bar <= 5e-6, fam                                       # three orders below the 2e-5 + rtol of the early tests


@pytest.mark.parametrize('kind', ['voxel', 'spatial', 'kl', 'l1', 'segce', 'adamw'])
def test_float32_evaluation_is_accepted(kind):
    """the float32 CPU evaluation of every case (up to 8 M input elements here; `python tests/loss_reference.py` runs them all)
    stays inside the bar: at most a quarter of it where the table was measured, more under another thread count's summation order"""
    worst = R.float32_errors(kind, max_elements=8 << 20)
    assert worst
    for fam, e in worst.items():
        print(f'LOSSSTAT float32-evaluation {kind}_{fam}: {e:.3e} ({R.BARS[f"{kind}_{fam}"]:.2e})')
        assert e <= R.BARS[f'{kind}_{fam}'], (kind, fam, e)


def _f32(ref):
    """what a perfect float32 kernel returns: the float64 reference rounded to float32"""
    return {k: v.float() for k, v in ref.items()}


def _rejected(kind, got, ref, names, **kw):
    bad = R.failures(R.compare(kind, got, ref, **kw))
    assert set(names) <= set(bad), f'planted error in {names} not rejected: only {sorted(bad)} failed'


def _accepted(kind, got, ref, **kw):
    bad = R.failures(R.compare(kind, got, ref, **kw))
    assert not bad, {n: s['max_e'] for n, s in bad.items()}


def test_planted_voxel_errors_are_rejected():
    # a scalar-path case with a two-voxel tail, production weights
    case = R.vcase(3, 9, 8194, 'prod')
    logits, lab, cw = R.voxel_inputs(case)
    ref = R.voxel_reference(logits, lab, cw)
    _accepted('voxel', _f32(ref), ref)
    _accepted('voxel', R.voxel_reference(logits, lab, cw, dtype=torch.float32), ref)
    got = _f32(ref)
    assert ref['dlogits'][1, :, 8192:].abs().max() > 0.01 * R.scale_of(ref['dlogits'])
    got['dlogits'][1, :, 8192:] = 0                                   # the last partial quad of a frame left zero
    _rejected('voxel', got, ref, ['dlogits'])
    got = _f32(ref)
    got['dlogits'][1] *= 1 + 1e-3                                     # one frame's gradient scaled by 1 + 1e-3
    _rejected('voxel', got, ref, ['dlogits'])
    cw1 = cw.clone()
    cw1[5] = 1.0                                                      # the weight of one class replaced by 1
    _rejected('voxel', _f32(R.voxel_reference(logits, lab, cw1)), ref, ['ce', 'dlogits'])
    # the same grid with 255 on half the voxels: CE divided by the number of valid voxels and not by F * V
    case = R.vcase(3, 9, 8194, 'prod', 'half255')
    logits, lab, cw = R.voxel_inputs(case)
    ref = R.voxel_reference(logits, lab, cw)
    _accepted('voxel', R.voxel_reference(logits, lab, cw, dtype=torch.float32), ref)
    factor = lab.numel() / float((lab != 255).sum())

    def ce_over_valid(*a, **k):
        ce, sem, geo = R.voxel_losses64(*a, **k)
        return ce * factor, sem, geo
    _rejected('voxel', _f32(R.voxel_reference(logits, lab, cw, fn=ce_over_valid)), ref, ['ce', 'dlogits'])
    # a class that never occurs: the SemScal coefficient b_i = 1 / P_i (the derivative of -log(N_i / P_i)) applied although T_i == 0
    case = R.vcase(3, 9, 20000, 'prod', 'absent')
    logits, lab, cw = R.voxel_inputs(case)
    ref = R.voxel_reference(logits, lab, cw)
    facts = R.voxel_label_facts(lab, 9)
    assert facts['T'][8] == 0 and facts['count'] == 8

    def b_on_absent_class(x, labels, weight, class_w, dtype):
        ce, sem, geo = R.voxel_losses64(x, labels, weight, class_w, dtype=dtype)
        P = torch.softmax(x, dim=1)[:, 8].sum()
        return ce, sem + (weight * (torch.log(P) - torch.log(P).detach()) / facts['count']), geo
    got = _f32(R.voxel_reference(logits, lab, cw, fn=b_on_absent_class))
    assert _rel(got['sem'], ref['sem']) < 1e-7                        # the value is untouched: only the gradient can tell
    _rejected('voxel', got, ref, ['dlogits'])
    # the <2> head on a vector-path grid
    case = R.vcase(2, 2, 96 * 96 * 32)
    logits, lab, cw = R.voxel_inputs(case)
    ref = R.voxel_reference(logits, lab, cw)
    _accepted('voxel', R.voxel_reference(logits, lab, cw, dtype=torch.float32), ref)
    got = _f32(ref)
    got['dlogits'][1] *= 1 + 1e-3
    _rejected('voxel', got, ref, ['dlogits'])
    got = _f32(ref)
    got['dlogits'][0, :, -4:] = 0
    _rejected('voxel', got, ref, ['dlogits'])


def test_planted_spatial_kl_l1_segce_errors_are_rejected():
    case = R.scase(3, 4, 40003, R.LIDAR)
    inp = R.spatial_inputs(case)
    ref = R.spatial_reference(case, *inp)
    _accepted('spatial', R.spatial_reference(case, *inp, dtype=torch.float32), ref)
    got = _f32(ref)
    assert ref['dpred'][2, :, 40000:].abs().max() > 0.01 * R.scale_of(ref['dpred'])
    got['dpred'][2, :, 40000:] = 0
    _rejected('spatial', got, ref, ['dpred'])
    got = _f32(ref)
    got['dpred'][1] *= 1 + 1e-3
    _rejected('spatial', got, ref, ['dpred'])
    got = _f32(ref)
    got['loss.0'] = got['loss.0'] * (1 + 2e-6)        # e.g. a count off by one in 500 000 masked pixels
    _rejected('spatial', got, ref, ['loss.0'])
    case = (8, 12, 512, 0.75)
    inp = R.kl_inputs(case)
    ref = R.kl_reference(case, inp)
    _accepted('kl', R.kl_reference(case, inp, dtype=torch.float32), ref)
    got = _f32(ref)
    got['dqs'][:, 1] = (ref['dqs'][:, 1] - R.KL_GOUT * R.KL_WEIGHT * 0.25 * (-1 / inp[3][:, 1].double() + inp[3][:, 1].double()) / (8 * 12)).float()
    _rejected('kl', got, ref, ['dqs'])                # the first-step term's gradient on sigma_q[t = 1] forgotten
    got = _f32(ref)
    got['loss'] = got['loss'] * (12 / 11)             # mean over T - 1 steps
    _rejected('kl', got, ref, ['loss'])
    case = (300, 3)
    inp = R.l1_inputs(case)
    ref = R.l1_reference(case, *inp)
    _accepted('l1', R.l1_reference(case, *inp, dtype=torch.float32), ref)
    got = _f32(ref)
    got['dp'][299] = 0
    _rejected('l1', got, ref, ['dp'])
    got = _f32(ref)
    got['loss'] = got['loss'] / 3                     # mean over elements and not over rows
    _rejected('l1', got, ref, ['loss'])
    case = R.SEGCE_CASES[1]
    logits, t, _, gloss = R.segce_inputs(case)
    cw = torch.tensor(R.PROD_W9)
    ref = R.segce_reference(case, logits, t, cw, gloss)
    _accepted('segce', R.segce_reference(case, logits, t, cw, gloss, dtype=torch.float32), ref)
    cw1 = cw.clone()
    cw1[3] = 1.0
    _rejected('segce', _f32(R.segce_reference(case, logits, t, cw1, gloss)), ref, ['map', 'dlogits'])


def test_planted_adamw_errors_are_rejected():
    lr = R.ADAMW_HP['lr']
    for case in (R.acase(4100), R.acase(4096, steps=(10000, 10001, 10002)), R.acase(4100, 0.125, 0.0)):
        inp = R.adamw_inputs(case)
        ref = R.adamw_reference(case, *inp)
        _accepted('adamw', _f32(ref), ref, lr=lr)
        _accepted('adamw', R.adamw_reference(case, *inp, dtype=torch.float32), ref, lr=lr)

        if case['steps'][0] == 1:            # (at step 10000 bc2 is 0.99995: rooted or not differs by 2e-5 of the update, far below p's scale)
            _rejected('adamw', _f32(R.adamw_reference(case, *inp, fn=_adamw_bc2)), ref, ['p'], lr=lr)
        # the last float4 missed the last step
        short = dict(case, steps=case['steps'][:2])
        prev = R.adamw_reference(short, inp[0], inp[1], inp[2], inp[3][:2])
        got = _f32(ref)
        for k in ('p', 'm', 'v'):
            got[k][-4:] = prev[k][-4:].float()
        _rejected('adamw', got, ref, ['p', 'm', 'v'], lr=lr)
        # grad_scale forgotten
        if case['grad_scale'] != 1.0:
            _rejected('adamw', _f32(R.adamw_reference(dict(case, grad_scale=1.0), *inp)), ref, ['m', 'v'], lr=lr)


def _adamw_bc2(p, g, m, v, lr, b1, b2, eps, wd, step, gs, dtype=torch.float64):
    """adamw64 with the second bias correction not square-rooted"""
    p, g, m, v = (a.to(dtype) for a in (p, g, m, v))
    g = g * gs
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - (lr / (1 - b1 ** step)) * (m / (v.sqrt() / (1 - b2 ** step) + eps)), m, v


# ------------------------------------------------------------------------------------------------ path()
def test_path_against_hand_computed_launches():
    # one 192 x 192 x 64 frame pair, C = 2: 2359296 / 8192 = 288 workgroups per frame, 576 <= 1280; 589824 quads / (288 * 256) = 8
    assert R.path('voxel_fwd', 2, 2, 192 * 192 * 64) == {'inst': 2, 'vec': True, 'wg': 288, 'capped': False, 'trips': 8}
    assert R.path('voxel_bwd', 2, 2, 192 * 192 * 64) == {'inst': 2, 'vec': True, 'wg': 576, 'capped': False, 'trips': 4}
    # 640 frames of 32768: 4 workgroups per frame would be 2560 > 1280 -> 1280 / 640 = 2; 8192 quads / 512 threads = 16 trips
    assert R.path('voxel_fwd', 640, 2, 32768) == {'inst': 2, 'vec': True, 'wg': 2, 'capped': True, 'trips': 16}
    assert R.path('voxel_bwd', 640, 2, 32768) == {'inst': 2, 'vec': True, 'wg': 8, 'capped': False, 'trips': 4}
    assert R.path('voxel_bwd', 1040, 2, 32768) == {'inst': 2, 'vec': True, 'wg': 7, 'capped': True, 'trips': 5}
    assert R.path('voxel_fwd', 3, 9, 8193) == {'inst': 0, 'vec': False, 'wg': 2, 'capped': False, 'trips': 5}
    assert R.path('voxel_fwd', 3, 9, 20000, aligned=False)['vec'] is False and R.path('voxel_fwd', 3, 9, 20000)['vec'] is True
    assert R.path('voxel_fwd', 3, 16, 1) == {'inst': 0, 'vec': False, 'wg': 1, 'capped': False, 'trips': 1}
    # rgb_1 at 600 x 960, 16 frames: 144000 quads -> 141 workgroups, 2256 > 1024 -> 64; 144000 / 16384 = 8.8 -> 9 trips: the flush
    assert R.path('spatial_fwd', 16, 0, 600 * 960) == {'vec': True, 'wg': 64, 'capped': True, 'trips': 9, 'flush': True}
    assert R.path('spatial_fwd', 20, 0, 64 * 1024) == {'vec': True, 'wg': 16, 'capped': False, 'trips': 4, 'flush': False}
    assert R.path('spatial_fwd', 3, 0, 5) == {'vec': False, 'wg': 1, 'capped': False, 'trips': 1, 'flush': False}
    assert R.path('adamw', 0, 0, 4096) == {'vec': True, 'wg': 2, 'partial': False, 'tail4': 512}
    assert R.path('adamw', 0, 0, 4092)['vec'] is False and R.path('adamw', 0, 0, 10007)['vec'] is False
    assert R.path('adamw', 0, 0, 4096 + 4 * 511) == {'vec': True, 'wg': 3, 'partial': True, 'tail4': 511}
    assert R.path('adamw', 0, 0, 512 * 4 * 3 + 4) == {'vec': True, 'wg': 4, 'partial': True, 'tail4': 1}
    assert R.path('adamw', 0, 0, 4100, aligned=False)['vec'] is False


def test_case_lists_reach_every_path():
    vp = [R.voxel_paths(c) for c in R.VOXEL_CASES]
    for inst in (2, 0):
        for vec in (True, False):
            assert any(f['inst'] == inst and f['vec'] == vec for f, _ in vp), (inst, vec)
    assert any(f['trips'] >= 8 and not f['capped'] for f, _ in vp) and any(f['capped'] and f['trips'] >= 16 for f, _ in vp)
    assert any(b['capped'] for _, b in vp) and any(b['trips'] > 1 for _, b in vp)
    assert any(c['offset'] != 'none' and c['V'] % 4 == 0 and not f['vec'] for c, (f, _) in zip(R.VOXEL_CASES, vp))
    sp = [R.path('spatial_fwd', c['F'], 0, c['HW'], not c['offset']) for c in R.SPATIAL_CASES]
    assert any(p['flush'] for p in sp) and any(not p['vec'] for p in sp) and any(p['vec'] and p['trips'] > 1 for p in sp)
    assert any(c['mask'] == 'some' for c in R.SPATIAL_CASES) and any(c['mask'] == 'some' and c['HW'] % 4 for c in R.SPATIAL_CASES)
    ap = [R.path('adamw', 0, 0, c['n'], not c['offset']) for c in R.ADAMW_CASES]
    assert any(p['vec'] and p['partial'] for p in ap) and any(p['vec'] and not p['partial'] for p in ap)
    assert any(not p['vec'] for p in ap) and any(p['vec'] and p['tail4'] == 1 for p in ap)
    for c in R.VOXEL_CASES:
        R.check_expect(c['expect'], dict(zip(('fwd', 'bwd'), R.voxel_paths(c))))
    for c, p in zip(R.SPATIAL_CASES, sp):
        R.check_expect(c['expect'], {'': p})
    for c, p in zip(R.ADAMW_CASES, ap):
        R.check_expect(c['expect'], {'': p})
    ids = [R.voxel_id(c) for c in R.VOXEL_CASES] + [R.spatial_id(c) for c in R.SPATIAL_CASES] + [R.adamw_id(c) for c in R.ADAMW_CASES]
    assert len(set(ids)) == len(ids), 'case ids must be unique'
