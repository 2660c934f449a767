"""-m gpu: the dense GEMM unit (muvo_amd/csrc/gemm.hip: the tiled fp32 MFMA kernel, the k-vector / k-contiguous / n-contiguous
skinny kernels, the grouped Linear) and the two elementwise kernels every Linear backward runs next to it (muvo_colsum_acc,
muvo_act_bwd) against float64 CPU references, with the normalised error metric of tests/vox_reference.py and the bars of
tests/gemm_reference.py (f32_bar, or 2 x the kernel's own CPU emulation where that module says so; none from a GPU).  Every case
is tied to the kernel it exists for: the route the library reports (muvo_gemm_route / muvo_grouped_linear_route) must be the
one the case is listed for and the one the dispatch mirror gives, whose thresholds tests/test_gemm_reference.py sweeps.  C is
pre-filled with a marker wherever the kernel must not write (the padding between N and scm, one row past M in every batch slot,
the offset in front and the tail behind) and compared bit for bit afterwards.  On failure the worst element is printed with
its batch, row, column, workgroup and K ranges.

GPU-measured GEMMSTAT maxima are recorded next to the bars in gemm_reference.py.  No case is left out."""
import contextlib
import ctypes as C
import types

import pytest
import torch

import gemm_reference as R

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def det_mode(on):
    from muvo_amd import ops
    was = ops.get_deterministic()
    try:
        if on != was:
            ops.set_deterministic(on)
        yield
    finally:
        if ops.get_deterministic() != was:
            ops.set_deterministic(was)


def _check(label, kind, K, got, ref, bar=None):
    """one result tensor against (reference, denominator) under the bar of kernel `kind` over K terms"""
    bar = bar or R.kernel_bar(kind, K)
    st = R.error_stats(got, *ref)
    print(f'GEMMSTAT {label} {kind}: max e {st["max_e"]:.3e} rms {st["rms"]:.3e} share {R.excess(st, bar):.2f}')
    assert R.within(st, bar), (label, kind, st, bar)
    return st


# ================================================================================================ muvo_gemm
def _call(c, d, t):
    from muvo_amd import ops
    Cs = d.C0.to(t['A'].device)
    ops.gemm(t['A'], t['B'], Cs, c['M'], c['N'], c['K'], d.sam, d.sak, d.sbk, d.sbn, d.scm, bias=t['bias'], alpha=c['alpha'],
             act=c['act'], slope=c['slope'], mode=c['mode'], B1=c['B1'], B2=c['B2'], a_b=d.a_b, b_b=d.b_b, c_b=d.c_b,
             bias_div=c['bias_div'], a_off=c['a_off'], b_off=c['b_off'], c_off=c['c_off'])
    return Cs.cpu()


@pytest.mark.parametrize('c', R.GEMM_CASES, ids=[c['name'] for c in R.GEMM_CASES])
def test_gemm(dev, c):
    from muvo_amd import ops
    d = R.make(c)
    t = {'A': d.A.to(dev), 'B': d.B.to(dev), 'bias': None if d.bias is None else d.bias.to(dev)}
    assert t['A'].data_ptr() % 16 == 0 and t['B'].data_ptr() % 16 == 0
    with det_mode(c['det']):
        route = ops.gemm_route(c['M'], c['N'], c['K'], d.sam, d.sak, d.sbk, d.sbn, d.scm, c['bias'], c['act'], c['mode'], c['B1'], c['B2'],
                               t['A'].data_ptr() + 4 * c['a_off'], t['B'].data_ptr() + 4 * c['b_off'])
        assert route == R.case_plan(c), (route, R.case_plan(c))
        for k, v in c['expect'].items():
            assert route[k] == v, (k, route[k], v)
        Cs = _call(c, d, t)
        if c['twice']:
            assert torch.equal(Cs.view(torch.int32), _call(c, d, t).view(torch.int32)), 'deterministic mode: two runs differ'
    j = R.judge(c, d, Cs)
    print(R.statline(c, j, route['kernel']))
    assert j['canary_ok'], f'{j["n_canary_bad"]} elements outside the result were written'
    assert R.within(j['stats'], j['bar']), (j['stats'], j['bar'], 'worst element: ' + j['where'])


# ================================================================================================ grouped Linear
def _layers(c, inp, dev):
    lins = []
    for l in range(len(c['ns'])):
        wt, bt = R.grouped_trains(c, l)
        w = torch.nn.Parameter(inp.ws[l].to(dev), requires_grad=wt)
        b = None if inp.bs[l] is None else torch.nn.Parameter(inp.bs[l].to(dev), requires_grad=bt)
        if wt:
            w.grad = inp.gw[l].to(dev)
        if b is not None and bt:
            b.grad = inp.gb[l].to(dev)
        lins.append(types.SimpleNamespace(weight=w, bias=b))
    return lins


@pytest.mark.parametrize('c', R.GROUPED_CASES, ids=[c['name'] for c in R.GROUPED_CASES])
def test_grouped_linear(dev, c):
    from muvo_amd import ops
    inp = R.grouped_inputs(c)
    L, M, K = len(c['ns']), c['M'], c['K']
    assert ops.grouped_linear_route(M, K, c['ns']) == R.grouped_plan(M, K, c['ns'])
    lins = _layers(c, inp, dev)
    x = inp.x.to(dev).requires_grad_(c['x_grad'])
    assert ops.grouped_linear_supported(x, lins)
    ys = ops.grouped_linear(x, lins)
    for l in range(L):
        assert ys[l].shape == (M, c['ns'][l])
        _check(f'{c["name"]} y{l}', 'grouped_fwd', K, ys[l], R.ref_grouped_fwd(inp.x, inp.ws[l], inp.bs[l]))
    used = [l for l in range(L) if l not in c['unused']]
    torch.autograd.backward([ys[l] for l in used], [inp.dys[l].to(dev) for l in used])
    torch.cuda.synchronize()
    if c['x_grad']:
        _check(f'{c["name"]} dx', 'grouped_dx', sum(c['ns'][l] for l in used), x.grad,
               R.ref_grouped_dx([inp.dys[l] for l in used], [inp.ws[l] for l in used]))
    else:
        assert x.grad is None
    for l in range(L):
        wt, bt = R.grouped_trains(c, l)
        dy = inp.dys[l] if l in used else torch.zeros(M, c['ns'][l])          # an unused output: its gradient counts as zero
        if wt:
            _check(f'{c["name"]} dW{l}', 'grouped_dw', M, lins[l].weight.grad, R.ref_dw(dy, inp.x, inp.gw[l]))
        else:
            assert lins[l].weight.grad is None
        if lins[l].bias is not None:
            if bt:      # (also the layer whose weight is frozen: its bias gradient must not be lost)
                _check(f'{c["name"]} db{l}', 'grouped_db', M, lins[l].bias.grad, R.ref_colsum(dy, inp.gb[l]))
            else:
                assert lins[l].bias.grad is None


def test_grouped_linear_raw_entry_points(dev):
    """muvo_grouped_linear_fwd / _bwd called directly: a NULL dx, a NULL weight-gradient entry next to a bias gradient, a NULL
    bias-gradient entry next to a weight gradient; the marker behind every buffer survives"""
    from muvo_amd import ops
    lib = ops.lib()
    c = R.grcase('gr-raw-9x68', 9, 68, [5, 16, 130])
    inp = R.grouped_inputs(c)
    M, K, ns = c['M'], c['K'], c['ns']
    pad = lambda t: torch.cat([t.reshape(-1), torch.full((4,), R.MARKER)]).to(dev)        # noqa: E731
    x, ws, bs = inp.x.to(dev), [w.to(dev) for w in inp.ws], [b.to(dev) for b in inp.bs]
    ys = [pad(torch.full((M, n), R.MARKER)) for n in ns]
    narr = (C.c_int * 3)(*ns)
    ops._ck(lib.muvo_grouped_linear_fwd(ops._f(x), M, K, 3, ops._ptr_array(ws), ops._ptr_array(bs), ops._ptr_array(ys), narr, ops._st()))
    for l, n in enumerate(ns):
        assert bool((ys[l][M * n:].cpu() == R.MARKER).all())
        _check(f'raw y{l}', 'grouped_fwd', K, ys[l][:M * n].view(M, n), R.ref_grouped_fwd(inp.x, inp.ws[l], inp.bs[l]))
    dys = [d.to(dev) for d in inp.dys]
    gw = [pad(inp.gw[0]), None, pad(inp.gw[2])]
    gb = [pad(inp.gb[0]), pad(inp.gb[1]), None]
    ops._ck(lib.muvo_grouped_linear_bwd(ops._f(x), M, K, 3, ops._ptr_array(ws), ops._ptr_array(dys), None, ops._ptr_array(gw),
                                        ops._ptr_array(gb), narr, ops._st()))
    for l, n in enumerate(ns):
        if gw[l] is not None:
            assert bool((gw[l][n * K:].cpu() == R.MARKER).all())
            _check(f'raw dW{l}', 'grouped_dw', M, gw[l][:n * K].view(n, K), R.ref_dw(inp.dys[l], inp.x, inp.gw[l]))
        if gb[l] is not None:
            assert bool((gb[l][n:].cpu() == R.MARKER).all())
            _check(f'raw db{l}', 'grouped_db', M, gb[l][:n], R.ref_colsum(inp.dys[l], inp.gb[l]))


# ================================================================================================ column sums, activation backward
@pytest.mark.parametrize('det', (False, True), ids=('atomic', 'deterministic'))
@pytest.mark.parametrize('rows,cols,pad', R.COLSUM_CASES)
def test_colsum_acc(dev, rows, cols, pad, det):
    from muvo_amd import ops
    x, prior = R.colsum_inputs(rows, cols, pad)
    xs = x._base.to(dev)                                     # the (rows, cols + pad) storage: ld = cols + pad
    out = torch.cat([prior, torch.full((3,), R.MARKER)]).to(dev)
    with det_mode(det):
        runs = []
        for _ in range(2 if det else 1):
            o = out.clone()
            ops._ck(ops.lib().muvo_colsum_acc(ops._f(xs), ops._f(o), ops._i64(rows), ops._i64(cols), ops._i64(cols + pad), ops._st()))
            runs.append(o.cpu())
    assert len(runs) == 1 or torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    assert bool((runs[0][cols:] == R.MARKER).all())
    _check(f'colsum {rows}x{cols}+{pad} det={int(det)}', 'colsum', rows, runs[0][:cols], R.ref_colsum(x, prior))


@pytest.mark.parametrize('act', R.ALL_ACTS, ids=R.ACT_NAMES)
def test_act_bwd(dev, act):
    from muvo_amd import ops
    g = R._gen('act_bwd', act)
    y = R.act32(torch.randn(4099, generator=g), act)
    dy = torch.randn(4099, generator=g)
    yd, dyd, dz = y.to(dev), dy.to(dev), torch.full((4099 + 5,), R.MARKER).to(dev)
    ops._ck(ops.lib().muvo_act_bwd(ops._f(yd), ops._f(dyd), ops._f(dz), ops._i64(4099), act, ops._fl(R.SLOPE), ops._st()))
    dz = dz.cpu()
    assert bool((dz[4099:] == R.MARKER).all())
    _check(f'act_bwd {R.ACT_NAMES[act]}', 'act_bwd', 1, dz[:4099], R.ref_act_bwd(y, dy, act), bar=R.ACT_BWD_BAR)


# ================================================================================================ composites
def _act_bwd_on_device(y, dy, act, slope):
    from muvo_amd import ops
    dz = torch.empty_like(dy)
    ops._ck(ops.lib().muvo_act_bwd(ops._f(y), ops._f(dy), ops._f(dz), ops._i64(dy.numel()), act, ops._fl(slope), ops._st()))
    return dz


def _product_bar(M, N, K, sam, sak, sbk, sbn, mode=0, has_bias=False, act=R.ACT_NONE):
    """(kernel, bar) of one muvo_gemm product of a composite: the dispatch mirror on 16-byte aligned, dense operands"""
    k = R.gemm_plan(M, N, K, sam, sak, sbk, sbn, N, has_bias, act, mode)['kernel']
    return k, R.kernel_bar(k, K)


@pytest.mark.parametrize('act', R.ALL_ACTS, ids=R.ACT_NAMES)
@pytest.mark.parametrize('shape', R.LINEAR_FN_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_linear_fn(dev, shape, act):
    """ops.LinearFn stage by stage: y against float64 of (x, W, b); dz = act_bwd(own y, dy) is recomputed by the same kernel on the
    device and checked on its own; dx, dW (added to a non-zero .grad) and db against float64 of that dz"""
    from muvo_amd import ops
    rows, out_f, in_f = shape
    g = R._gen('linear_fn', shape, act)
    x, w, b = torch.randn(rows, in_f, generator=g), torch.randn(out_f, in_f, generator=g) / in_f ** 0.5, torch.randn(out_f, generator=g)
    dy, gw, gb = torch.randn(rows, out_f, generator=g), torch.randn(out_f, in_f, generator=g) * rows ** 0.5, torch.randn(out_f, generator=g) * rows ** 0.5
    W, B = torch.nn.Parameter(w.to(dev)), torch.nn.Parameter(b.to(dev))
    W.grad, B.grad = gw.to(dev), gb.to(dev)
    xg = x.to(dev).requires_grad_(True)
    y = ops.LinearFn.apply(xg, W, B, act, R.SLOPE)
    k, bar = _product_bar(rows, out_f, in_f, in_f, 1, 1, in_f, has_bias=True, act=act)
    assert k == (R.T if rows > 32 else R.KV)
    pre = x.double() @ w.double().t() + b.double()
    _check(f'linear {shape} {R.ACT_NAMES[act]} y', k, in_f, y, (R.act64(pre, act), ((x.double() ** 2) @ (w.double() ** 2).t() + b.double() ** 2).sqrt()), bar)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    dz = _act_bwd_on_device(y.detach(), dy.to(dev), act, R.SLOPE).cpu() if act != R.ACT_NONE else dy
    if act != R.ACT_NONE:
        _check(f'linear {shape} {R.ACT_NAMES[act]} dz', 'act_bwd', 1, dz, R.ref_act_bwd(y.detach().cpu(), dy, act), R.ACT_BWD_BAR)
    k, bar = _product_bar(rows, in_f, out_f, out_f, 1, in_f, 1)
    _check(f'linear {shape} {R.ACT_NAMES[act]} dx', k, out_f, xg.grad, R.CR.ref_matmul(dz, w), bar)
    k, bar = _product_bar(out_f, in_f, rows, 1, out_f, in_f, 1, mode=1)
    assert k == R.T
    _check(f'linear {shape} {R.ACT_NAMES[act]} dW', k, rows, W.grad, R.ref_dw(dz, x, gw), bar)
    _check(f'linear {shape} {R.ACT_NAMES[act]} db', 'colsum', rows, B.grad, R.ref_colsum(dz, gb))


def test_seed_convt_fn(dev):
    """_Seed1x1ConvTFn (ConvTranspose2d on a 1x1 input as one GEMM, bias per output channel through bias_div, fused ELU) at
    (n 4, ci 48, co 20, 5 x 13), stage by stage in float64"""
    from muvo_amd import ops
    from muvo_amd.models.common import _Seed1x1ConvTFn
    s = R.SEED_CASE
    n, ci, co, kh, kw = s['n'], s['ci'], s['co'], s['kh'], s['kw']
    ncol = co * kh * kw
    g = R._gen('seed')
    x, w, b = torch.randn(n, ci, 1, 1, generator=g), torch.randn(ci, co, kh, kw, generator=g) / ci ** 0.5, torch.randn(co, generator=g)
    dy, gw, gb = torch.randn(n, co, kh, kw, generator=g), torch.randn(ci, co, kh, kw, generator=g) * 2, torch.randn(co, generator=g) * 16
    W, B = torch.nn.Parameter(w.to(dev)), torch.nn.Parameter(b.to(dev))
    W.grad, B.grad = gw.to(dev), gb.to(dev)
    xg = x.to(dev).requires_grad_(True)
    y = _Seed1x1ConvTFn.apply(xg, W, B, ops.ACT_ELU)
    k, bar = _product_bar(n, ncol, ci, ci, 1, ncol, 1, has_bias=True, act=R.ACT_ELU)
    assert k == R.NC
    x2, w2 = x.view(n, ci).double(), w.view(ci, ncol).double()
    bcol = b.double().repeat_interleave(kh * kw)
    _check('seed y', k, ci, y.view(n, ncol), (R.act64(x2 @ w2 + bcol, R.ACT_ELU), ((x2 ** 2) @ (w2 ** 2) + bcol ** 2).sqrt()), bar)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    dz = _act_bwd_on_device(y.detach(), dy.to(dev), ops.ACT_ELU, 0.0).cpu()
    _check('seed dz', 'act_bwd', 1, dz, R.ref_act_bwd(y.detach().cpu(), dy, R.ACT_ELU), R.ACT_BWD_BAR)
    dz2 = dz.view(n, ncol)
    k, bar = _product_bar(n, ci, ncol, ncol, 1, 1, ncol)
    assert k == R.KV
    _check('seed dx', k, ncol, xg.grad.view(n, ci), R.CR.ref_matmul(dz2, w.view(ci, ncol).t()), bar)
    k, bar = _product_bar(ci, ncol, n, 1, ci, ncol, 1, mode=1)
    _check('seed dW', k, n, W.grad.view(ci, ncol), R.ref_dw(x.view(n, ci), dz2, gw.view(ci, ncol)), bar)
    # (the bias gradient is muvo_bias_grad_nchw of conv_gemm.hip: n * kh * kw terms per channel, fp32 sums)
    _check('seed db', 'bias_grad_nchw', n * kh * kw, B.grad, R.ref_colsum(dz.permute(0, 2, 3, 1).reshape(-1, co), gb), R.f32_bar(n * kh * kw))


@pytest.mark.parametrize('case', R.ATTN_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_attention_fn(dev, case):
    """the unfused attention core (five batched products on the tiled kernel straight on the packed qkv layout, two-level batches
    with offsets) at p = 0 against attention_reference.reference64, bar = 4 x the float32 CPU evaluation"""
    from muvo_amd import ops
    l, n, heads, dh = case
    qkv, dout = R.attention_inputs(case)
    q = qkv.to(dev).requires_grad_(True)
    o = ops.AttentionFn.apply(q, heads, 0.0, 0)
    o.backward(dout.to(dev))
    torch.cuda.synchronize()
    e = R.attention_errors(case, {'o': o.detach().cpu(), 'dqkv': q.grad.cpu()})
    for name, v in e.items():
        print(f'GEMMSTAT attention {case} {name}: max e {v:.3e} share {v / R.ATTN_BARS[case][name]:.2f}')
    for name, v in e.items():
        assert v <= R.ATTN_BARS[case][name], (name, v, R.ATTN_BARS[case][name])
