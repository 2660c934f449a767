"""-m gpu: the normalisation kernels of muvo_amd/csrc/norm.hip, reached as the model reaches them (muvo_amd.nn.BatchNorm2d /
ops.bn_act, ops.adain, ops.adain_lazy, ops.adain_head, ops.add_dropout_layernorm; the _planes BatchNorm entry points directly),
against the float64 references of tests/norm_reference.py with its normalised error and its bars (4 x the error of the float32 CPU
evaluation of the same reference; tests/test_norm_reference.py shows on the CPU that these bars reject planted errors).  The case
lists live in norm_reference.py; every id is built from path(), the restatement of the launch arithmetic, and every case asserts
the path properties it exists for.  Each case prints `NORMSTAT <id> <name>: max_e rms (bar)` lines.

No case loops, retries or sets a MUVO_NORM_* variable; deterministic mode is switched through ops.set_deterministic alone and
restored in `finally`."""
import ctypes as C
import math

import pytest
import torch

import norm_reference as R

pytestmark = pytest.mark.gpu


def _judge(tag, cmp):
    for line in R.statlines(tag, cmp):
        print(line)
    bad = R.failures(cmp)
    assert not bad, f'{tag}: ' + '; '.join(f'{n} max_e {s["max_e"]:.3e} at {s["index"]} (bar {cmp[n][1]:.2e})' for n, s in bad.items())


def _place(t, dev, off=0):
    """`t` on the device as a contiguous tensor of its own that starts `off` elements after a 16-byte boundary"""
    n = t.numel()
    buf = torch.zeros(n + 12, dtype=t.dtype, device=dev)
    buf[4 + off:4 + off + n] = t.reshape(-1).to(dev)
    v = buf[4 + off:4 + off + n].view(t.shape).detach()
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off == 0)
    return v


class _Deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from muvo_amd import ops
        self.was = ops.get_deterministic()
        if self.on:
            ops.set_deterministic(True)

    def __exit__(self, *exc):
        from muvo_amd import ops
        if self.on:
            ops.set_deterministic(self.was)


def _assert_mask(tag, ref):
    if ref['_mask'] is not None:
        frac, worst = ref['_mask']
        print(f'NORMSTAT {tag} relu-mask: disagrees with float64 on {frac:.3e} of the elements, |pre| there <= {worst:.3e} of max')
        assert frac <= R.MASK_CAP and worst <= R.MASK_BAND, (frac, worst)


# ------------------------------------------------------------------------------------------------ BatchNorm
def _run_bn(dev, c, inp):
    from muvo_amd import nn as hnn
    N, Cn, S, mis = c['N'], c['C'], c['S'], c['mis']
    with torch.device(dev):
        bn = hnn.BatchNorm2d(Cn)
    assert R.f32r(bn.eps) == R.BN_EPS and R.f32r(bn.momentum) == R.BN_MOMENTUM
    with torch.no_grad():
        for dst, k in ((bn.weight, 'gamma'), (bn.bias, 'beta'), (bn.running_mean, 'rm0'), (bn.running_var, 'rv0')):
            dst.copy_(inp[k])
    bn.weight.grad, bn.bias.grad = inp['dgamma0'].to(dev), inp['dbeta0'].to(dev)          # the kernels ACCUMULATE into these
    x = _place(inp['x'].view(N, Cn, 1, S), dev, mis == 'x').requires_grad_(True)
    res = _place(inp['res'].view(N, Cn, 1, S), dev, mis == 'res').requires_grad_(True) if c['res_mode'] else None
    dy = _place(inp['dy'].view(N, Cn, 1, S), dev, mis == 'dy')
    y = bn(x, residual=res, res_mode=c['res_mode'] or 1, relu=c['relu'])
    mean, rstd = y.grad_fn.saved_tensors[2:4]
    got = {'y': y.detach().view(N, Cn, S), 'mean': mean.clone(), 'rstd': rstd.clone(), 'running_mean': bn.running_mean.clone(),
           'running_var': bn.running_var.clone()}
    seen = []
    y.register_hook(lambda g: seen.append(g.data_ptr() % 16))
    y.backward(dy)
    assert seen == [4 if mis == 'dy' else 0], 'the upstream gradient did not reach the backward at the offset the case is for'
    got.update(dx=x.grad.view(N, Cn, S), dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if res is not None:
        got['dres'] = res.grad.view(N, Cn, S)
    assert int(bn.state_dict()['num_batches_tracked']) == 1          # applied lazily, before the buffer is read
    return got


def _check_bn(dev, c, tag=None, names=None):
    """names: the results to judge (all of them when None)"""
    tag = tag or R.bn_id(c)
    R.check_expect(c['expect'], R.bn_paths(c))
    inp = R.bn_inputs(c)
    with _Deterministic(c['det']):
        got = _run_bn(dev, c, inp)
        got = {k: v.cpu() for k, v in got.items()}
    ref = R.bn_reference(c, inp, y_out=got['y'])
    _assert_mask(tag, ref)
    if c['N'] * c['S'] == 1:
        assert not ref['mean'].ne(inp['x'].double()[0, :, 0]).any() and float((ref['rstd'] - R.BN_EPS ** -0.5).abs().max()) < 1e-9
    fam = {k: v for k, v in R.BN_FAM.items() if names is None or k in names}
    _judge(tag, R.compare(fam, got, ref, R.factor_of(c)))


ONE_ELEMENT = ('y', 'rstd')          # judged apart for the one-element cases: see test_batchnorm_one_element_per_channel


@pytest.mark.parametrize('case', R.BN_CASES, ids=R.bn_id)
def test_batchnorm(dev, case):
    one = case['N'] * case['S'] == 1
    _check_bn(dev, case, names=[k for k in R.BN_FAM if k not in ONE_ELEMENT] if one else None)


@pytest.mark.xfail(strict=True, reason='one element per channel: the one-pass variance E[x^2] - m^2 and the x * sc + sh form of the apply '
                                       'kernels leave rounding residue of x^2 and of x * rstd, amplified by 1 / eps: by design, not widened')
@pytest.mark.parametrize('case', [c for c in R.BN_CASES if c['N'] * c['S'] == 1], ids=R.bn_id)
def test_batchnorm_one_element_per_channel(dev, case):
    """(1, 7, 1): the documented rule evaluated in float64 is variance 0, rstd = 1 / sqrt(eps), y = beta.  The kernels miss it by
    design and nothing that trains has one element per channel, so the case stays as a strict expected failure instead of a
    wider bar.  rstd: the statistics pass adds float32 x and x * x into its float64 sums, so E[x^2] - m^2 is the rounding
    residue of x * x (up to 2^-24 x^2) where it should be 0; against eps = 1e-5 that is percents of rstd.  y: the apply kernels
    compute x * sc + (beta - mean * sc) with sc = gamma * rstd of about 316 gamma, so beta comes back with the rounding error of a
    product of several hundred.  Measured on an MI355X, res_mode / ReLU (0, no), (0, yes), (1, yes), (2, yes):
        y     1.22e-04  2.74e-04  1.68e-05  7.25e-06   (bar 7.24e-07)
        rstd  2.00e-02  2.91e-02  3.15e-03  4.84e-03   (bar 5.56e-07)
    Everything else of these cases (mean, running statistics, dx = 0, dres, parameter gradients) is held to the usual bars by
    test_batchnorm."""
    _check_bn(dev, case, names=ONE_ELEMENT)


def _decode_planes(ws, N, S, Cn):
    """(values hi + lo as (N, Cn, S), the padding channels, the 16 bytes behind the planes) of a split-planes workspace"""
    cp = (Cn + 7) // 8 * 8
    n = N * S * cp
    b = ws.view(torch.bfloat16)
    v = (b[:n].double() + b[n:2 * n].double()).view(N, S, cp)
    return v[:, :, :Cn].permute(0, 2, 1).contiguous(), torch.cat([b[:n].view(N, S, cp)[:, :, Cn:], b[n:2 * n].view(N, S, cp)[:, :, Cn:]]), b[2 * n:2 * n + 8]


@pytest.mark.parametrize('mode', R.MODES, ids=lambda m: f'r{m[0]}{"relu" if m[1] else "lin"}')
@pytest.mark.parametrize('shape', [(4, 70, 2080), (3, 12, 260)], ids=lambda s: 'N%dC%dS%d' % s)
def test_batchnorm_planes(dev, shape, mode):
    """muvo_bn_train_fwd_planes / _bwd_planes with deterministic mode off (three statistics workgroups per channel at 2080; the
    float4 tile kernel at 2080, the pixel-per-lane kernel at 260; 70 and 12 channels: padding to 72 and 16): the fp32 results and
    statistics at the usual bars, the planes decoded as hi + lo at the bar + 2^-16, padding channels and the trailing quad 0."""
    from muvo_amd import ops
    L = ops.lib()
    N, Cn, S = shape
    c = R.bcase(N, Cn, S, *mode)
    f = R.bn_paths(c)['fwd']
    assert f['chunks'] == (3 if S == 2080 else 1) and not ops.get_deterministic()
    tag = f'bnplanes-N{N}C{Cn}S{S}-r{mode[0]}{"relu" if mode[1] else "lin"}-{R._stat_tag(f)}-{"tile4" if S >= 1024 else "pixel"}'
    inp = R.bn_inputs(c)
    d = {k: v.to(dev) for k, v in inp.items()}
    nws = (L.muvo_split_planes_bytes(N, Cn, C.c_int64(S)) + 3) // 4
    y, mean, rstd = torch.empty_like(d['x']), torch.empty(Cn, device=dev), torch.empty(Cn, device=dev)
    rm, rv = d['rm0'].clone(), d['rv0'].clone()
    ws = torch.full((nws,), 7.0, device=dev)
    ops._ck(L.muvo_bn_train_fwd_planes(ops._f(d['x']), ops._f(d['gamma']), ops._f(d['beta']), ops._f(d['res']) if mode[0] else None, ops._f(y),
                                       ops._f(mean), ops._f(rstd), ops._f(rm), ops._f(rv), N, Cn, C.c_int64(S), C.c_float(1e-5),
                                       C.c_float(0.1), mode[0], int(mode[1]), ops._p(ws), ops._st()))
    yp, pad, tail = _decode_planes(ws, N, S, Cn)
    assert not pad.float().any() and not tail.float().any(), 'forward planes: padding channels / trailing quad not zero'
    mask_mode = 0 if not mode[1] else (1 if mode[0] == 1 else 2)
    dx, dres = torch.empty_like(d['x']), torch.empty_like(d['x']) if mode[0] == 1 else None
    dg, db = d['dgamma0'].clone(), d['dbeta0'].clone()
    ws2 = torch.full((nws,), 7.0, device=dev)
    ops._ck(L.muvo_bn_train_bwd_planes(ops._f(d['x']), ops._f(y), ops._f(d['dy']), ops._f(d['gamma']), ops._f(d['beta']), ops._f(mean),
                                       ops._f(rstd), ops._f(dx), ops._f(dres), ops._f(dg), ops._f(db), N, Cn, C.c_int64(S), mask_mode,
                                       ops._p(ws2), ops._st()))
    dxp, pad, tail = _decode_planes(ws2, N, S, Cn)
    assert not pad.float().any() and not tail.float().any(), 'backward planes: padding channels / trailing quad not zero'
    got = {'y': y, 'mean': mean, 'rstd': rstd, 'running_mean': rm, 'running_var': rv, 'dx': dx, 'dgamma': dg, 'dbeta': db}
    if mode[0] == 1:
        got['dres'] = dres
    got = {k: v.cpu() for k, v in got.items()}
    ref = R.bn_reference(c, inp, y_out=got['y'])
    _assert_mask(tag, ref)
    cmp = R.compare(R.BN_FAM, got, ref)
    cmp['y.planes'] = R.compare({'y': 'bn_y'}, {'y': yp.cpu()}, ref, extra=R.SPLIT_RESIDUE)['y']
    cmp['dx.planes'] = R.compare({'dx': 'bn_dx'}, {'dx': dxp.cpu()}, ref, extra=R.SPLIT_RESIDUE)['dx']
    _judge(tag, cmp)


def test_batchnorm_ring_wrap(dev):
    """520 forward passes of a 2048-channel BatchNorm: each takes 4096 doubles of the 2^20-double statistics ring, so the ring
    wraps (and is cleared behind its readers) at least twice wherever it stood; every output against float64 on the device"""
    from muvo_amd import nn as hnn
    from muvo_amd import ops
    Cn, N, S = 2048, 2, 4
    gen = torch.Generator(device=dev).manual_seed(7)
    with torch.device(dev):
        bn = hnn.BatchNorm2d(Cn)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(Cn, generator=gen, device=dev))
        bn.bias.copy_(torch.rand(Cn, generator=gen, device=dev) - 0.5)
    g, b = bn.weight.detach().double()[None, :, None, None], bn.bias.detach().double()[None, :, None, None]
    worst = torch.zeros(520, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for i in range(520):
            xd = (torch.randn(N, Cn, 1, S, generator=gen, device=dev) * 2 + 0.5).double()
            m = xd.mean(dim=(0, 2, 3), keepdim=True)
            xd = xd - m + 0.5 * (xd - m).pow(2).mean(dim=(0, 2, 3), keepdim=True).sqrt()        # groups of 8: mean / std = 0.5
            x = xd.float()
            y = bn(x)
            xd = x.double()
            m = xd.mean(dim=(0, 2, 3), keepdim=True)
            yr = (xd - m) / torch.sqrt((xd - m).pow(2).mean(dim=(0, 2, 3), keepdim=True) + R.BN_EPS) * g + b
            worst[i] = (y.double() - yr).abs().max() / yr.abs().max()
    w = worst.cpu()
    print(f'NORMSTAT bn-ringwrap-C{Cn}N{N}S{S}-520passes y: {float(w.max()):.3e} {float(w.pow(2).mean().sqrt()):.3e} ({R.BARS["bn_y"]:.2e})')
    assert int(bn.state_dict()['num_batches_tracked']) == 520
    assert float(w.max()) <= R.BARS['bn_y'], f'pass {int(w.argmax())}: {float(w.max()):.3e}'


# ------------------------------------------------------------------------------------------------ AdaIN
def _run_adain(dev, c, inp, how='plain'):
    """how: 'plain' (statistics pass), 'moments' (sums handed in), 'lazy' (statistics -> affine table, nothing applied)"""
    from muvo_amd import ops
    N, Cn, S, mis = c['N'], c['C'], c['S'], c['mis']
    x = _place(inp['x'].view(Cn, 1, 1, S) if c['bcast'] else inp['x'].view(N, Cn, 1, 1, S), dev, mis == 'x').requires_grad_(True)
    style = inp['style'].to(dev).requires_grad_(True)
    dy = _place(inp['dy'].view(N, Cn, 1, 1, S), dev, mis == 'dy')
    act = ops.ACT_LEAKY if c['pre'] else ops.ACT_NONE
    moments, got = None, {}
    if how != 'plain':
        xd = x.detach().double().view(N, Cn, S)
        moments = torch.stack([xd.sum(-1), (xd * xd).sum(-1)], dim=-1).contiguous()
    if how == 'lazy':
        y, _, aff = ops.adain_lazy(x, style, 1e-8, act, 0.2, moments)
        got.update(aff_a=aff[..., 0].clone(), aff_b=aff[..., 1].clone())
    else:
        y = ops.adain(x, style, 1e-8, N, act, 0.2, moments)
        got['y'] = y.detach().view(N, Cn, S)
    if moments is not None:
        assert float(moments.abs().max()) == 0.0, 'the moments must come back cleared'
    mean, rstd = y.grad_fn.saved_tensors[2:4]
    got.update(mean=mean.clone(), rstd=rstd.clone())
    seen = []
    y.register_hook(lambda g: seen.append(g.data_ptr() % 16))
    y.backward(dy)
    assert seen == [4 if mis == 'dy' else 0]
    got.update(dx=x.grad.view(inp['x'].shape), dstyle=style.grad)
    return {k: v.cpu() for k, v in got.items()}


def _check_adain(dev, c, how='plain', tag=None):
    tag = tag or R.adain_id(c)
    R.check_expect(c['expect'], R.adain_paths(c))
    inp = R.adain_inputs(c)
    if c['pre']:
        z = float((inp['x'] == 0).float().mean())
        assert 0.002 < z < 0.03 or inp['x'].numel() < 2000, 'about 1 % of a pre-activated input is exactly 0'
    got = _run_adain(dev, c, inp, how)
    _judge(tag, R.compare(R.ADAIN_FAM, got, R.adain_reference(c, inp), R.factor_of(c)))


@pytest.mark.parametrize('case', R.ADAIN_CASES, ids=R.adain_id)
def test_adain(dev, case):
    _check_adain(dev, case)


@pytest.mark.parametrize('how', ['moments', 'lazy'])
@pytest.mark.parametrize('case', R.MOMENT_CASES, ids=R.adain_id)
def test_adain_from_moments(dev, case, how):
    """muvo_adain_fwd_moments / muvo_adain_affine with float64 moments computed here: y or the affine table, mean / rstd, the
    moments cleared, and the backward (muvo_adain_bwd in both forms)"""
    _check_adain(dev, case, how, R.adain_id(case) + '-' + how)


# ------------------------------------------------------------------------------------------------ AdaIN + head
@pytest.mark.parametrize('case', R.HEAD_CASES, ids=R.head_id)
def test_adain_head(dev, case):
    from muvo_amd import ops
    N, S, c = case['N'], case['S'], case
    R.check_expect(c['expect'], R.head_paths(c))
    inp = R.head_inputs(c)
    x = inp['x'].view(N, R.HEAD_C, 1, 1, S).to(dev).requires_grad_(True)
    style = inp['style'].to(dev).requires_grad_(True)
    hw = torch.nn.Parameter(inp['w'].view(R.HEAD_CO, R.HEAD_C, 1, 1, 1).to(dev))
    hb = torch.nn.Parameter(inp['b'].to(dev)) if c['bias'] else None
    hw.grad = inp['dw0'].view_as(hw).to(dev)                                  # the kernels ACCUMULATE into these
    if hb is not None:
        hb.grad = inp['db0'].to(dev)
    xd = x.detach().double().view(N, R.HEAD_C, S)
    moments = torch.stack([xd.sum(-1), (xd * xd).sum(-1)], dim=-1).contiguous()
    assert ops.adain_head_supported(x, hw, moments)
    logits = ops.adain_head(x, style, hw, hb, 1e-8, moments, ops.ACT_LEAKY if c['pre'] else ops.ACT_NONE, 0.2)
    assert float(moments.abs().max()) == 0.0
    logits.backward(inp['dl'].view(N, R.HEAD_CO, 1, 1, S).to(dev))
    got = {'logits': logits.detach().view(N, R.HEAD_CO, S), 'dx': x.grad.view(N, R.HEAD_C, S), 'dstyle': style.grad,
           'dw': hw.grad.view(R.HEAD_CO, R.HEAD_C)}
    if hb is not None:
        got['db'] = hb.grad
    _judge(R.head_id(c), R.compare(R.HEAD_FAM, {k: v.cpu() for k, v in got.items()}, R.head_reference(c, inp)))


# ------------------------------------------------------------------------------------------------ add + dropout + LayerNorm
@pytest.mark.parametrize('case', R.LN_CASES, ids=R.ln_id)
def test_add_dropout_layernorm(dev, case):
    from muvo_amd import nn as hnn
    from muvo_amd import ops
    c, rows, E, p = case, case['rows'], case['E'], case['p']
    R.check_expect(c['expect'], {'': R.ln_path(c)})
    inp = R.ln_inputs(c)
    with torch.device(dev):
        ln = hnn.LayerNorm(E)
    assert R.f32r(ln.eps) == R.LN_EPS
    with torch.no_grad():
        ln.weight.copy_(inp['gamma'])
        ln.bias.copy_(inp['beta'])
    ln.weight.grad, ln.bias.grad = inp['dgamma0'].to(dev), inp['dbeta0'].to(dev)
    # the dropout's scale, from the same hash over the same flat index: forward and backward must both agree with it
    scale = ops.dropout(torch.ones(rows, E, device=dev), p, R.LN_SEED).cpu()
    if p > 0:
        inv = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)))
        assert bool(((scale == 0) | (scale == inv)).all()), 'a dropout scale is 0 or 1 / (1 - p)'
        keep, n = float((scale > 0).double().mean()), rows * E
        assert abs(keep - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), f'keep rate {keep} of {n} at p = {p}'
    else:
        assert bool((scale == 1).all())
    x, a = inp['x'].to(dev).requires_grad_(True), inp['a'].to(dev).requires_grad_(True)
    with _Deterministic(c['det']):
        y = ops.add_dropout_layernorm(x, a, ln, p, R.LN_SEED)
        y.backward(inp['dy'].to(dev))
        got = {'y': y.detach().cpu(), 'dx': x.grad.cpu(), 'da': a.grad.cpu(), 'dgamma': ln.weight.grad.cpu(), 'dbeta': ln.bias.grad.cpu()}
    _judge(R.ln_id(c), R.compare(R.LN_FAM, got, R.ln_reference(c, inp, scale)))


# ------------------------------------------------------------------------------------------------ housekeeping paths
def test_first_use_on_a_fresh_side_stream(dev):
    """a new stream gets its own statistics ring and accumulator, allocated and cleared on that stream at first use"""
    bc, ac = R.bcase(4, 6, 2080, 1, True), dict(R.acase(2, 4, 4160), pre=True)
    binp, ainp = R.bn_inputs(bc), R.adain_inputs(ac)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        gb = {k: v.cpu() for k, v in _run_bn(dev, bc, binp).items()}
        ga = _run_adain(dev, ac, ainp)
    torch.cuda.current_stream(dev).wait_stream(side)
    side.synchronize()
    ref = R.bn_reference(bc, binp, y_out=gb['y'])
    _assert_mask('sidestream-' + R.bn_id(bc), ref)
    _judge('sidestream-' + R.bn_id(bc), R.compare(R.BN_FAM, gb, ref))
    _judge('sidestream-' + R.adain_id(ac), R.compare(R.ADAIN_FAM, ga, R.adain_reference(ac, ainp)))


def test_reset_accumulators_then_ordinary_cases(dev):
    """ops.reset_accumulators() clears every stream's ring and accumulator and rewinds the ring
    (test_reset_accumulators_after_interrupted_step of test_kernels_gpu.py looks at the per-layer moments buffers only): the
    cases that follow see all-zero slots"""
    from muvo_amd import ops
    _check_bn(dev, R.bcase(3, 10, 1280, 2, True), 'before-reset-' + R.bn_id(R.bcase(3, 10, 1280, 2, True)))
    ops.reset_accumulators()
    c = R.bcase(4, 6, 2080, 1, True)
    _check_bn(dev, c, 'after-reset-' + R.bn_id(c))
    a = dict(R.acase(2, 4, 4160), pre=False)
    _check_adain(dev, a, tag='after-reset-' + R.adain_id(a))
