"""CPU: the float64 references, the bars, the case lists and path() of tests/norm_reference.py, which tests/test_norm_kernels_gpu.py
applies to the normalisation kernels.  Shown here, without a GPU:
  * the references agree with torch's batch_norm / instance_norm / layer_norm and their autograd;
  * the MEASURED table is the float32 CPU evaluation (every case is evaluated again: within a factor of 4 either way, which is what
    another thread count's summation order can move it by, and never above the bar), and the offset cases stay inside their
    derived bar;
  * under that evaluation the ReLU masks differ from the float64 ones on at most 1e-4 of the elements, all of them at the origin;
  * the bars bite: the float64 reference rounded to float32 with ONE planted error each is rejected by the very comparison the GPU
    test uses;
  * path() reproduces launches computed by hand from norm.hip, every `expect` holds, and the ids show every path the suite is for."""
import pytest
import torch
import torch.nn.functional as F

import norm_reference as R

FAMILIES = ['bn_y', 'bn_stat', 'bn_run', 'bn_dx', 'bn_dparam', 'bn_dres', 'adain_y', 'adain_stat', 'adain_dx', 'adain_dstyle',
            'head_logits', 'head_dx', 'head_dparam', 'ln_y', 'ln_dx', 'ln_da', 'ln_dparam']


# ------------------------------------------------------------------------------------------------ the references
def test_references_agree_with_torch():
    c = R.bcase(3, 5, 40, 1, True)
    inp = R.bn_inputs(c)
    ref = R.bn_reference(c, inp)
    x, r, g, b = (inp[k].double().requires_grad_(True) for k in ('x', 'res', 'gamma', 'beta'))
    rm, rv = inp['rm0'].double().clone(), inp['rv0'].double().clone()
    y = F.relu(F.batch_norm(x, rm, rv, g, b, True, R.BN_MOMENTUM, R.BN_EPS) + r)
    gs = torch.autograd.grad(y, [x, r, g, b], inp['dy'].double())
    for got, want in ((ref['y'], y), (ref['running_mean'], rm), (ref['running_var'], rv), (ref['dx'], gs[0]), (ref['dres'], gs[1]),
                      (ref['dgamma'] - inp['dgamma0'].double(), gs[2]), (ref['dbeta'] - inp['dbeta0'].double(), gs[3])):
        assert torch.allclose(got, want.detach(), rtol=1e-11, atol=1e-12)
    c2 = R.bcase(3, 5, 40, 2, True)
    y2 = R.bn_reference(c2, inp)['y']
    assert torch.allclose(y2, (F.relu(F.batch_norm(x, None, None, g, b, True, 0.1, R.BN_EPS)) + r).detach(), rtol=1e-11, atol=1e-12)
    one = R.bcase(1, 7, 1, 0, False)                    # one element per channel: variance 0, unbiased = biased
    i1 = R.bn_inputs(one)
    r1 = R.bn_reference(one, i1)
    assert torch.equal(r1['y'][0, :, 0], i1['beta'].double()) and not r1['dx'].any()
    assert torch.allclose(r1['running_var'], (1 - R.BN_MOMENTUM) * i1['rv0'].double(), rtol=1e-15)
    for bcast in (False, True):
        a = dict(R.acase(3, 4, 50, bcast=bcast), pre=False)
        ai = R.adain_inputs(a)
        ar = R.adain_reference(a, ai)
        h = ai['x'].double().requires_grad_(True)
        hh = h.expand(3, 4, 50) if bcast else h
        s = ai['style'].double().requires_grad_(True)
        yy = s[:, :4, None] * F.instance_norm(hh, eps=R.ADAIN_EPS) + s[:, 4:, None]
        gh, gs_ = torch.autograd.grad(yy, [h, s], ai['dy'].double())
        assert torch.allclose(ar['y'], yy.detach(), rtol=1e-10, atol=1e-11) and torch.allclose(ar['dx'], gh, rtol=1e-9, atol=1e-10)
        assert torch.allclose(ar['dstyle'], gs_, rtol=1e-10, atol=1e-11)
        assert torch.allclose(ar['aff_a'][:, :, None] * hh.detach() + ar['aff_b'][:, :, None], ar['y'], rtol=1e-9, atol=1e-9)
    p = dict(R.acase(2, 3, 64), pre=True)               # the LeakyReLU derivative, slope at an output of exactly 0
    pi = R.adain_inputs(p)
    pi['x'][0, 0, :3] = torch.tensor([0.0, -1.0, 2.0])
    plain = R.adain_reference(dict(p, pre=False), pi)['dx']
    ratio = R.adain_reference(p, pi)['dx'][0, 0, :3] / plain[0, 0, :3]
    assert torch.allclose(ratio, torch.tensor([R.SLOPE, R.SLOPE, 1.0], dtype=torch.float64), rtol=1e-12)
    hc = R.hcase(2, 1024, True, False)
    hi = R.head_inputs(hc)
    hr = R.head_reference(hc, hi)
    ya = R.adain_reference(dict(R.acase(2, 8, 1024), pre=False), {'x': hi['x'], 'style': hi['style'], 'dy': torch.zeros(2, 8, 1024)})['y']
    want = F.conv1d(ya, hi['w'].double()[:, :, None], hi['b'].double())
    assert torch.allclose(hr['logits'], want, rtol=1e-11, atol=1e-12)
    lc = R.lcase(9, 33, 0.5)
    li = R.ln_inputs(lc)
    lr = R.ln_reference(lc, li, li['cpu_scale'])
    x, a, g, b = (li[k].double().requires_grad_(True) for k in ('x', 'a', 'gamma', 'beta'))
    y = F.layer_norm(x + a * li['cpu_scale'].double(), (33,), g, b, R.LN_EPS)
    gs = torch.autograd.grad(y, [x, a, g, b], li['dy'].double())
    assert torch.allclose(lr['y'], y.detach(), rtol=1e-11, atol=1e-12) and torch.allclose(lr['dx'], gs[0], rtol=1e-10, atol=1e-12)
    assert torch.allclose(lr['da'], gs[1], rtol=1e-10, atol=1e-12) and not lr['da'][li['cpu_scale'] == 0].any()
    assert torch.allclose(lr['dgamma'] - li['dgamma0'].double(), gs[2], rtol=1e-10, atol=1e-12)


def test_inputs_carry_sentinels_and_offsets():
    c = R.bcase(3, 5, 2731, 0, False)
    x = R.bn_inputs(c)['x']
    per = R.path('bn_fwd', 3, 5, 2731)['per']
    assert R.boundaries(3 * 2731, per) == [2732, 5464]
    flat = x.transpose(0, 1).reshape(5, -1)
    for b in (2732, 5464):
        assert bool((flat[:, b - 4:b + 4] >= 40).all())
    assert bool((x[:, :, :4] >= 40).all()) and bool((x[:, :, -4:] >= 40).all()) and float((x >= 40).float().mean()) < 0.01
    xo = R.bn_inputs(R.bcase(4, 6, 2080, 0, False, offset=True))['x'].double().transpose(0, 1).reshape(6, -1)
    assert torch.allclose(xo.mean(1) / xo.var(1, unbiased=False).sqrt(), torch.full((6,), R.OFFSET, dtype=torch.float64), rtol=1e-5)
    ao = R.adain_inputs(dict(R.acase(2, 4, 4160, offset=True), pre=False))['x'].double()
    assert torch.allclose(ao.mean(-1) / ao.var(-1, unbiased=False).sqrt(), torch.full((2, 4), R.OFFSET, dtype=torch.float64), rtol=1e-5)
    z = R.adain_inputs(dict(R.acase(3, 10, 2048), pre=True))['x']
    assert 0.005 < float((z == 0).float().mean()) < 0.02 and float(z.min()) < 0


# ------------------------------------------------------------------------------------------------ the bars
def test_bars_come_from_the_float32_evaluation():
    assert sorted(R.BARS) == sorted(FAMILIES)
    for fam, bar in R.BARS.items():
        assert bar == 4 * R.MEASURED[fam] and bar <= 2e-5, fam          # the early tests: rtol 5e-4
    assert R.OFFSET_FACTOR == 257.0 and R.SPLIT_RESIDUE == 2.0 ** -16


@pytest.mark.parametrize('kind', ['bn', 'adain', 'head', 'ln'])
def test_measured_table_is_the_float32_evaluation(kind):
    worst = R.float32_errors(kind)
    assert set(worst) == {f for f in FAMILIES if f.startswith(kind + '_')}
    for fam, e in worst.items():
        print(f'NORMSTAT float32-evaluation {fam}: {e:.3e} (table {R.MEASURED[fam]:.2e}, bar {R.BARS[fam]:.2e})')
        assert e <= R.BARS[fam] and e >= R.MEASURED[fam] / 4, (fam, e)
    for fam, e in R.float32_errors(kind, offset=True).items():
        print(f'NORMSTAT float32-evaluation offset {fam}: {e:.3e} (bar {R.BARS[fam] * R.OFFSET_FACTOR:.2e})')
        assert e <= R.BARS[fam] * R.OFFSET_FACTOR, (fam, e)


def test_relu_masks_of_the_float32_evaluation_stay_within_the_cap():
    seen = 0
    for c in R.BN_CASES:
        if c['relu'] and not c['mis'] and not c['det']:         # (the twins share their data with a case that is looked at)
            frac, worst = R.evaluate32('bn', c)[1]['_mask']
            assert frac <= R.MASK_CAP and worst <= R.MASK_BAND, (R.bn_id(c), frac, worst)
            seen += 1
    assert seen >= 20


def _f32(ref):
    """what a perfect float32 kernel returns: the float64 reference rounded to float32"""
    return {k: v.float() for k, v in ref.items() if not k.startswith('_')}


def _rejected(fam, got, ref, names):
    bad = R.failures(R.compare(fam, got, ref))
    assert set(names) <= set(bad), f'planted error in {names} not rejected: only {sorted(bad)} failed'


def _accepted(fam, got, ref):
    bad = R.failures(R.compare(fam, got, ref))
    assert not bad, {n: s['max_e'] for n, s in bad.items()}


def test_planted_batchnorm_errors_are_rejected():
    c = R.bcase(4, 6, 2080, 1, True)
    assert R.path('bn_fwd', 4, 6, 2080)['per'] == 2776 and c['N'] * c['S'] == 8320
    inp = R.bn_inputs(c)
    ref = R.bn_reference(c, inp)
    _accepted(R.BN_FAM, _f32(ref), ref)
    sub = R.bn_reference(c, inp, torch.float32)
    _accepted(R.BN_FAM, sub, R.bn_reference(c, inp, y_out=sub['y']))
    # a statistics pass that drops one float4: the last of a row, the first behind a chunk boundary (element 2776 of a channel is
    # element 696 of image 1)
    for n, s in ((2, 2076), (1, 696)):
        x = inp['x'].clone()
        assert float(x[n, 3, s:s + 4].min()) >= 40
        x[n, 3, s:s + 4] = 0
        _rejected(R.BN_FAM, _f32(R.bn_reference(c, dict(inp, x=x))), ref, ['mean', 'rstd', 'running_mean', 'y', 'dx'])
    _rejected(R.BN_FAM, _f32(R.bn_reference(c, inp, unbiased_y=True)), ref, ['y', 'rstd', 'dx'])        # 1 / (2 x 8320) of rstd
    _rejected(R.BN_FAM, _f32(R.bn_reference(c, inp, biased_running=True)), ref, ['running_var'])
    _rejected(R.BN_FAM, _f32(R.bn_reference(c, inp, swap_res=True)), ref, ['y'])
    got = _f32(ref)
    got['dgamma'] = (ref['dgamma'] - inp['dgamma0'].double()).float()                                    # overwritten, not accumulated
    _rejected(R.BN_FAM, got, ref, ['dgamma'])
    got = _f32(ref)
    flip = (ref['_pre'].abs() < 1e-3) & (inp['dy'].abs() > 0.1)      # the backward takes the other sign on elements next to the origin
    assert 0 < int(flip.sum()) < 100
    got['dx'][flip] = (ref['dx'][flip] + 1.0).float()
    _rejected(R.BN_FAM, got, ref, ['dx'])


def test_planted_adain_and_head_errors_are_rejected():
    c = dict(R.acase(2, 4, 4160), pre=False)
    assert R.path('adain_fwd', 2, 4, 4160)['per'] == 2080
    inp = R.adain_inputs(c)
    ref = R.adain_reference(c, inp)
    _accepted(R.ADAIN_FAM, _f32(ref), ref)
    _accepted(R.ADAIN_FAM, R.adain_reference(c, inp, torch.float32), ref)
    for s in (4156, 2080):                   # the last float4 of a row, the first of the second statistics chunk
        x = inp['x'].clone()
        assert float(x[1, 2, s:s + 4].min()) >= 40
        x[1, 2, s:s + 4] = 0
        _rejected(R.ADAIN_FAM, _f32(R.adain_reference(c, dict(inp, x=x))), ref, ['mean', 'rstd', 'y', 'dx'])
    got = _f32(ref)
    got['dx'][1, 3, -4:] = 0                 # a tail quad of dx left unwritten
    _rejected(R.ADAIN_FAM, got, ref, ['dx'])
    p = dict(c, pre=True)
    pi = R.adain_inputs(p)
    pr = R.adain_reference(p, pi)
    got = _f32(pr)
    zero = pi['x'] == 0
    assert int(zero.sum()) > 100
    got['dx'][zero] = (pr['dx'][zero] / R.SLOPE).float()       # derivative 1 at an output of exactly 0
    _rejected(R.ADAIN_FAM, got, pr, ['dx'])
    hc = R.hcase(2, 1028, True, True)
    hi = R.head_inputs(hc)
    hr = R.head_reference(hc, hi)
    _accepted(R.HEAD_FAM, _f32(hr), hr)
    _accepted(R.HEAD_FAM, R.head_reference(hc, hi, torch.float32), hr)
    got = _f32(hr)
    got['db'] = (hi['db0'].double() + (hr['db'] - hi['db0'].double()) * (1 + 1e-3)).float()              # the bias gradient scaled by 1 + 1e-3
    _rejected(R.HEAD_FAM, got, hr, ['db'])
    got = _f32(hr)
    got['dw'] = (hr['dw'] - hi['dw0'].double()).float()
    _rejected(R.HEAD_FAM, got, hr, ['dw'])
    got = _f32(hr)
    got['logits'][1, :, 1024:] = 0           # S4 = 257: the quad behind the first workgroup's 256
    _rejected(R.HEAD_FAM, got, hr, ['logits'])


def test_planted_layernorm_errors_are_rejected():
    c = R.lcase(37, 96, 0.5)
    inp = R.ln_inputs(c)
    ref = R.ln_reference(c, inp, inp['cpu_scale'])
    _accepted(R.LN_FAM, _f32(ref), ref)
    _accepted(R.LN_FAM, R.ln_reference(c, inp, inp['cpu_scale'], torch.float32), ref)
    _rejected(R.LN_FAM, _f32(R.ln_reference(c, inp, inp['cpu_scale'], unmasked_da=True)), ref, ['da'])   # da without the mask
    other = (torch.rand(37, 96, generator=torch.Generator().manual_seed(1)) >= 0.5).float() * 2
    _rejected(R.LN_FAM, _f32(R.ln_reference(c, inp, other)), ref, ['y', 'da'])                            # another mask in forward
    got = _f32(ref)
    got['y'][32:], got['dx'][32:] = 0, 0     # the row tail (rows % 16) left unwritten
    _rejected(R.LN_FAM, got, ref, ['y', 'dx'])
    got = _f32(ref)
    got['dbeta'] = (ref['dbeta'] - inp['dbeta0'].double()).float()
    _rejected(R.LN_FAM, got, ref, ['dbeta'])


# ------------------------------------------------------------------------------------------------ path()
def test_path_against_hand_computed_launches():
    # 4 x 2080 = 8320 per channel: 3 chunks of cdiv(8320, 3) = 2774 -> 2776; S / 4 = 520 quads: one workgroup column, 3 passes
    assert R.path('bn_fwd', 4, 6, 2080) == {'chunks': 3, 'capped': False, 'per': 2776, 'stat': 'vec4', 'stat_passes': 1, 'flush': False,
                                            'apply': 'vec', 'apply_passes': 3}
    assert R.path('bn_fwd', 4, 6, 2080, det=True)['chunks'] == 1 and R.path('bn_fwd', 4, 6, 2080, det=True)['per'] == 8320
    # 3 x 2731 = 8193: 3 chunks of 2731 -> 2732: boundaries at 2732 and 5464, inside images 1 and 2; scalar: 11 passes of 256
    assert R.path('bn_bwd', 3, 5, 2731) == {'chunks': 3, 'capped': False, 'per': 2732, 'stat': 'scalar', 'stat_passes': 11, 'flush': False,
                                            'apply': 'scalar', 'apply_passes': 1}
    # 1 080 000 per channel want 264 chunks: 256 of cdiv = 4219 -> 4220, two passes; 135 000 quads on 64 workgroups: 9 passes
    p = R.path('bn_fwd', 2, 3, 540000)
    assert (p['chunks'], p['capped'], p['per'], p['stat_passes'], p['flush'], p['apply'], p['apply_passes']) == (256, True, 4220, 2, False, 'vec', 9)
    assert R.path('bn_fwd', 2, 1, 1600000)['per'] == 12500 and R.path('bn_fwd', 2, 1, 1600000)['flush']
    assert R.path('bn_fwd', 3, 10, 260)['apply'] == 'quad' and R.path('bn_bwd', 3, 10, 260)['apply'] == 'scalar'
    assert R.path('bn_fwd', 5, 24, 126)['stat'] == 'scalar' and R.path('bn_fwd', 5, 24, 126)['apply'] == 'scalar'
    assert R.path('bn_fwd', 1, 7, 1)['per'] == 4 and R.path('bn_fwd', 1, 7, 1)['stat_passes'] == 1
    # the alignment guards: x in every float4 path, the residual in the forward apply, dy in both backward kernels
    assert R.path('bn_fwd', 3, 10, 1280, mis=('x',))['stat'] == 'scalar' and R.path('bn_fwd', 3, 10, 1280, mis=('x',))['apply'] == 'scalar'
    assert R.path('bn_fwd', 3, 10, 1280, mis=('res',))['stat'] == 'vec4' and R.path('bn_fwd', 3, 10, 1280, mis=('res',))['apply'] == 'scalar'
    assert R.path('bn_fwd', 3, 10, 260, mis=('res',))['apply'] == 'scalar'
    assert R.path('bn_bwd', 3, 10, 1280, mis=('dy',))['stat'] == 'scalar' and R.path('bn_bwd', 3, 10, 1280, mis=('dy',))['apply'] == 'scalar'
    assert R.path('bn_bwd', 3, 10, 1280, mis=('res',))['apply'] == 'vec'
    # AdaIN: per instance; 540672 = 132 x 4096 wants 132 chunks: 128 of 4224
    p = R.path('adain_fwd', 2, 2, 540672)
    assert (p['chunks'], p['capped'], p['per'], p['stat_passes'], p['apply'], p['grow']) == (128, True, 4224, 2, 'vec', False)
    assert R.path('adain_fwd', 2, 3, 4099)['per'] == 2052 and R.path('adain_fwd', 2, 3, 4099)['stat'] == 'scalar'
    assert R.path('adain_fwd', 40000, 1, 4)['grow'] and not R.path('adain_fwd', 32768, 1, 4)['grow']
    assert R.path('adain_fwd', 3, 10, 9, bcast=True)['launches'] == 3
    assert R.path('adain_bwd', 3, 10, 2048, mis=('dy',))['apply'] == 'scalar' and R.path('adain_fwd', 3, 10, 2048, mis=('dy',))['apply'] == 'vec'
    # the head: 257 quads -> 1 workgroup of 1024 in forward and apply ... cdiv(257, 1024) = 1; 132096 quads want 129 -> 128, 5 passes
    assert R.path('head_fwd', 2, 8, 1028) == {'gx': 1, 'capped': False, 'passes': 2}
    assert R.path('head_bwd', 2, 8, 528384) == {'gx': 128, 'capped': True, 'passes': 5}
    assert R.path('head_fwd', 1, 8, 524288) == {'gx': 128, 'capped': False, 'passes': 4}
    assert R.path('ln', 37, 0, 511) == {'blocks': 3, 'rows_per_block': 16, 'tail': 5, 'slots': 8, 'trips': 1}
    assert R.path('ln', 70, 0, 96, det=True) == {'blocks': 1, 'rows_per_block': 70, 'tail': 0, 'slots': 2, 'trips': 5}


def test_case_lists_reach_every_path():
    for c in R.BN_CASES:
        R.check_expect(c['expect'], R.bn_paths(c))
    for c in R.ADAIN_CASES + R.MOMENT_CASES:
        R.check_expect(c['expect'], R.adain_paths(c))
    for c in R.HEAD_CASES:
        R.check_expect(c['expect'], R.head_paths(c))
    for c in R.LN_CASES:
        R.check_expect(c['expect'], {'': R.ln_path(c)})
    ids = [R.bn_id(c) for c in R.BN_CASES] + [R.adain_id(c) for c in R.ADAIN_CASES] + [R.head_id(c) for c in R.HEAD_CASES] + \
          [R.ln_id(c) for c in R.LN_CASES]
    assert len(set(ids)) == len(ids), 'case ids must be unique'
    bn = [i for i in ids if i.startswith('bn-')]
    for piece in ('st1x', 'st3x2776vec4', 'st3x2732scalar', 'st256capx4220vec4x2', 'flush', '-quadx', '-vecx', '-scalarx', 'bwdscalar-scalarx',
                  'bwdvec4-vecx', '-offset', '-misx', '-misres', '-misdy', '-det', 'N1C7S1', '-r0lin', '-r0relu', '-r1relu', '-r2relu'):
        assert any(piece in i for i in bn), piece
    ad = [i for i in ids if i.startswith('adain-')]
    for piece in ('st1x', 'st2x2080vec4', 'st2x2052scalar', 'st128capx4224', 'flush', '-bcast', '-grow', '-offset', '-misx', '-misdy', '-lrelu',
                  '-vecx1', '-scalarx'):
        assert any(piece in i for i in ad), piece
    grow = [i for i, c in enumerate(R.ADAIN_CASES) if R.adain_paths(c)['fwd']['grow']]
    assert grow and 0 < grow[0] and grow[-1] < len(R.ADAIN_CASES) - 1, 'the accumulator grows in the middle of the list'
    assert any('gx128capx5' in i for i in ids) and any('-nobias' in i for i in ids) and any('S1028-gx1x2' in i for i in ids)
    ln = [c for c in R.LN_CASES]
    assert {c['E'] for c in ln} >= {1, 63, 64, 65, 96, 384, 511, 512} and {c['rows'] for c in ln} >= {1, 3, 4, 15, 16, 17, 70}
    assert {(c['E'], c['p']) for c in ln} >= {(e, p) for e in (96, 384) for p in (0.0, 0.1, 0.5)} and sum(c['det'] for c in ln) == 2
