"""-m gpu: the implicit-GEMM convolution kernels (muvo_amd/csrc/conv_gemm.hip, conv_bf3.hip, conv_pw.hip) against float64 CPU
references, with the normalised error metric of tests/vox_reference.py and bars at the scale of the arithmetic each direction
runs on (tests/conv_reference.py: BF3_BAR for the bf16x3 split products, f32_bar(reduction length) for exact fp32).  Every
case is tied to the kernels it exists for: the library's family and variant must agree with the dispatch mirror
(conv_reference.conv_plan), whose tiles and splits tests/test_conv_bars.py pins.  On failure the worst element is printed with
its phase, row group, m-tile and pixel tile.

GPU-measured CONVSTAT maxima are recorded next to the bars in conv_reference.py."""
import collections
import contextlib
import ctypes
import math

import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu

NONE, RELU, LEAKY, ELU = R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY, R.ACT_ELU
ACT_NAMES = {NONE: 'none', RELU: 'relu', LEAKY: 'leaky', ELU: 'elu'}
OPS = ('fwd', 'dgrad', 'wgrad')
BF3, F32 = R.BF3, R.F32


class Case(collections.namedtuple('Case', 'layer n in_sz act mode marks')):
    """marks: 'b' also runs with x.requires_grad = False (weight gradient alone), 'c' with the parameters frozen (data gradient
    alone); split-K cases also run in deterministic mode (test_conv_deterministic)."""
    __slots__ = ()

    @property
    def id(self):
        return f'{self.layer.name()}-n{self.n}-{"x".join(map(str, self.in_sz))}-{ACT_NAMES[self.act]}-{self.mode}'


def _c(kind, cin, cout, k, s, p, n, in_sz, act=NONE, mode=BF3, marks='', out_pad=0):
    return Case(R.Layer(kind, cin, cout, k, s, p, out_pad), n, tuple(in_sz), act, mode, marks)


# bf16x3 mode.  What each case is for: see the table in test_conv_bars.py::PINNED (tile, split-K, merge, K order per direction).
CASES = [
    _c('conv2d', 32, 32, 3, 1, 1, 2, (9, 7), LEAKY),            # 126 pixels: one partial pixel tile over both samples; M = 32
    _c('conv2d', 40, 48, 3, 1, 1, 3, (5, 13), ELU, marks='bc'),  # Cp = 40: taps outermost, K steps straddle taps; ragged M = 48
    _c('conv2d', 8, 64, 5, 1, 2, 2, (12, 11), RELU),            # Cp = 8; forward bf16x3, dgrad (M = 8) and wgrad (C < 32) fp32 split-K
    _c('conv2d', 64, 128, 3, 2, 1, 2, (21, 27), LEAKY, marks='bc'),   # odd input: dgrad = four separate phases, 4/2/2/1 taps
    _c('conv2d', 64, 128, 3, 2, 1, 2, (20, 26), NONE),          # even input: dgrad phases union-merged (M = 256, T = 4)
    _c('conv2d', 64, 64, 5, 2, 2, 2, (12, 12), ELU),            # union merge 9/6/6/4 of 9
    _c('conv2d', 64, 48, 5, 2, 2, 2, (11, 9), RELU),            # the same kernel unmerged (odd grid)
    _c('convT2d', 64, 32, 6, 2, 2, 2, (5, 13), ELU, marks='bc'),      # identical-tap merge with Msub = 32; dgrad bf16x3 split-K, 2 ranges
    _c('convT2d', 48, 64, 4, 2, 1, 2, (6, 7), LEAKY),           # transposed forward that does not merge: four launches, Cp = 48
    _c('convT2d', 160, 96, 5, 2, 2, 1, (4, 6), ELU, out_pad=1),  # output padding: unequal sub-grids, split-K + forced two ranges
    _c('conv2d', 136, 64, 3, 1, 1, 1, (6, 7), LEAKY, marks='bc'),     # split-K 39 steps as 20 + 19; dgrad M = 136: three m-tiles
    _c('conv2d', 520, 64, 3, 1, 1, 1, (5, 13), ELU),            # 147 K steps as 9 ranges, finishing bias + ELU pass
    _c('conv2d', 48, 256, 3, 2, 1, 1, (9, 11), NONE),           # dgrad: unmerged, the 4-tap phase splits and forces its siblings
    _c('conv2d', 256, 48, 3, 2, 1, 1, (9, 11), RELU),           # the transpose of the above
    _c('conv2d', 32, 160, 3, 1, 1, 1, (128, 128), NONE),        # exactly 128 workgroups of 256x128
    _c('conv2d', 32, 160, 3, 1, 1, 1, (127, 128), NONE),        # one below: 64x128, three m-tiles
    _c('conv2d', 32, 96, 3, 1, 1, 2, (128, 128), NONE),         # the same threshold for the 128x256 tile
    _c('conv2d', 32, 96, 3, 1, 1, 2, (127, 128), LEAKY),        # (LeakyReLU + bias through the v4 fused preamble)
    _c('convT2d', 96, 160, 6, 2, 2, 2, (64, 64), ELU),          # merged M = 640 on 256x128 tiles; merged ping-pong wgrad; v4 preamble
    _c('conv2d', 72, 96, 3, 1, 1, 2, (7, 9), LEAKY),            # wgrad 128x256 ping-pong
    _c('conv2d', 96, 48, 3, 1, 1, 2, (7, 9), ELU),              # wgrad 64x128 (M <= 64, 64 < C <= 128)
    _c('conv2d', 96, 32, 3, 1, 1, 2, (23, 21), NONE),           # wgrad 64x128 at M = 32; 966 pixels = 31 steps: quantised split 16 + 15
    _c('conv2d', 32, 64, 1, 2, 0, 2, (12, 14), NONE, marks='bc'),     # dgrad phases without a tap: whole operation on fp32
    _c('conv2d', 32, 64, 1, 1, 0, 2, (12, 14), LEAKY),          # 1x1 on all three bf16x3 directions
    _c('conv3d', 40, 32, 3, 1, 1, 2, (3, 5, 7), ELU),           # 27 taps through the general kernels
    _c('conv2d', 32, 32, 3, 1, 1, 1, (33, 35), LEAKY),          # output size >= 1024 but no multiple of 4: scalar preamble
    _c('conv2d', 160, 32, 3, 1, 1, 1, (6, 7), NONE),            # wgrad 64x256 (C > 128 at M <= 64)
    # exact fp32 mode
    _c('conv2d', 3, 64, 7, 2, 3, 2, (38, 50), NONE, F32),       # Cp = 4
    _c('conv2d', 3, 96, 3, 1, 1, 1, (9, 7), LEAKY, F32),        # Cp = 4 on the 128-row tile
    _c('conv2d', 4, 16, 3, 1, 1, 2, (5, 6), NONE, F32),         # Cp = 4 on the 32-row tile
    _c('conv2d', 8, 16, 3, 1, 1, 3, (9, 7), RELU, F32),         # Cp = 8, 32x128 tile
    _c('conv2d', 20, 40, 3, 1, 1, 2, (10, 13), LEAKY, F32),     # 64x128
    _c('conv2d', 70, 130, 3, 1, 1, 2, (6, 11), ELU, F32),       # 128x128, ragged second m-tile, Cp = 80
    # split-K with the finishing pass.  (256 -> 64 k3 and ConvT 160 -> 96 k6, the shapes of test_kernels_gpu.py::test_conv_family,
    # reduce over 2304 / 3456 products: there a bar with margin 2 over the serial fp32 chain no longer fails bf16x3 arithmetic
    # 4x - test_conv_bars.py - so the same paths run at 1152 / 1024 products)
    _c('conv2d', 128, 64, 3, 1, 1, 1, (6, 7), ELU, F32),
    _c('convT2d', 128, 32, 6, 2, 2, 1, (3, 4), LEAKY, F32),     # merged phases (M = 128, Msub = 32)
    _c('convT2d', 40, 24, 5, 2, 2, 3, (5, 13), ELU, F32, out_pad=1),
    _c('conv2d', 64, 128, 3, 2, 1, 2, (20, 26), NONE, F32),     # merged data-gradient phases on the fp32 kernel
    # one per weight-gradient column tile (bn 32 / 64 / 128): a pixel count that is no multiple of 32, several workgroups each
    _c('conv2d', 24, 32, 3, 1, 1, 3, (21, 19), NONE, F32),
    _c('conv2d', 24, 64, 3, 1, 1, 3, (21, 19), RELU, F32),
    _c('conv2d', 24, 128, 3, 1, 1, 3, (21, 19), NONE, F32),
]

# bf16x3 products inside the fp32-staged weight gradient (conv_wgrad_kernel<..., true>: above 2 GFLOP per launch): weight and
# bias gradient only
# One per column tile (bn 64 / 128 / 32), each 2.03 GFLOP against the threshold of 2.  The arithmetic can identify the variant
# only while the fp32 bar of the pixel count lies below the bf16x3 error (rms 4.4e-6), i.e. below ~25 000 pixels: at 340 x 340
# (8 -> 64 N = 2, 8 -> 128 N = 1, 16 -> 32 N = 2: 115 600 / 231 200 pixels) the kernel measured rms 4.43e-6 / 4.40e-6 / 4.50e-6
# against fp32 bars of 1.3e-5 / 9.3e-6 / 1.3e-5, which tells nothing.  So the work comes from taps and channels instead.
WGRAD_BF3_IN_F32 = [
    _c('conv2d', 24, 64, 7, 1, 3, 1, (116, 116)),
    _c('conv2d', 24, 128, 5, 1, 2, 1, (115, 115)),
    _c('conv2d', 31, 32, 7, 1, 3, 1, (144, 144)),     # (fp32 bar 3.9e-6 at 20 736 pixels: the smallest count that reaches 2 GFLOP on 32 columns)
]

# 1x1 heads (conv_pw.hip, family 3, exact fp32 VALU)
PW_CASES = [_c('conv2d', cin, co, 1, 1, 0, 2, (32, 32), mode=mode) for cin, co, mode in
            ((16, 1, BF3), (130, 2, BF3), (16, 3, F32), (130, 4, BF3))]
PW_CASES += [_c('conv3d', cin, co, 1, 1, 0, 1, (16, 16, 8)) for cin, co in ((130, 1), (16, 2), (130, 3), (16, 4))]

# fused head in the epilogue: (stage, N, input size, head channels, trunk gradient present)
HEAD_CASES = [(R.Layer('convT2d', 64, 64, 6, 2, 2, 0), 2, (64, 128), co, t) for co, t in ((1, True), (2, False), (4, True))]
HEAD_CASES += [(R.Layer('convT2d', 64, 128, 6, 2, 2, 0), 2, (64, 64), co, t) for co, t in ((1, False), (2, True), (4, False))]

# rows, in features, out features.  (36 produced features, a float4 row tail, cannot run: LinearBf16x3Fn sizes both packed
# copies up front and the data-gradient copy needs features % 8 == 0; ops.linear only routes out features % 16 == 0 here.)
LINEAR_CASES = [(130, 40, 48), (257, 64, 160)]


def split_k_cases():
    out = []
    for c in CASES:
        plans = [R.conv_plan(c.layer, c.n, c.in_sz, op, c.mode) for op in ('fwd', 'dgrad')]
        if any(p['finish'] for p in plans):
            out.append(c)
    return out


@contextlib.contextmanager
def conv_mode(mode, det=False):
    from muvo_amd import ops
    old, was_det = ops.get_conv_mode(), ops.get_deterministic()
    try:
        if det:
            ops.set_deterministic(True)
        ops.set_conv_mode(ops.CONV_BF16X3 if mode == BF3 else ops.CONV_F32, min_gflop=0.0)
        yield
    finally:
        ops.set_conv_mode(old, min_gflop=-1.0)
        if det:
            ops.set_deterministic(was_det)


def library_answers(geom, n, in_sz):
    """families and eight-wave variants of the three directions as the library reports them in the current mode"""
    from muvo_amd import ops
    d = geom.plan(n, (1,) + tuple(in_sz) if geom.nd == 2 else tuple(in_sz))[0]
    L = ops.lib()
    return (tuple(L.muvo_conv_kernel_family(ctypes.byref(d), op) for op in (0, 1, 2)),
            tuple(L.muvo_conv_kernel_variant(ctypes.byref(d), op) for op in (0, 1, 2)))


def check(name, got, ref, den, bar, where=None):
    s = R.error_stats(got, ref, den)
    print(f'CONVSTAT {name}: max_e {s["max_e"]:.3e} rms {s["rms"]:.3e} (bars {bar[1]:.1e} / {bar[0]:.1e})')
    assert R.within(s, bar), (f'{name}: max(e) {s["max_e"]:.3e} (bar {bar[1]:.1e}), rms {s["rms"]:.3e} (bar {bar[0]:.1e}); '
                              f'worst {where(s["index"]) if where else s["index"]}')
    return s


def _weight_where(idx):
    return f'weight element {idx}'


def _bias_where(idx):
    return f'channel {idx[0]}'


def plan_bar(plan, reduction=None):
    """the bar of the arithmetic a direction runs on; fp32: at the longest reduction of its launches"""
    if plan['family'] == 1:
        return R.BF3_BAR
    if reduction is None:
        reduction = max(p['T'] * p['C'] for p in plan['phases'])
    return R.f32_bar(reduction)


def _dz(case, g, y):
    """Gradient at the pre-activation, formed in float64 from the kernel's OWN activated output as the kernels form it
    (common.h: act_grad_from_out - ReLU / LeakyReLU by the sign of y, ELU y + 1 below 0).  A derivative taken from the float64
    pre-activation instead would carry the forward's rounding error (bf16x3, or an fp32 chain over taps x channels) into the
    checks of the weight and bias gradient, whose own reductions are short: measured on 128 -> 64 k3 in fp32 mode, the weight
    gradient over 42 pixels then shows rms 1.8e-7 = 0.47 u sqrt(42), twice its serial chain, all of it from y."""
    return g.double() * R.act_derivative(y, case.act).double()


def run_case(dev, case, seed, need_dx=True, need_dw=True, det=False):
    from muvo_amd import ops
    layer, n, in_sz, act, mode, _ = case
    tag = case.id + ('' if need_dx else '-wgrad-only') + ('' if need_dw else '-dgrad-only') + ('-det' if det else '')
    plans = [R.conv_plan(layer, n, in_sz, op, mode, det) for op in OPS]
    assert all(p is not None for p in plans), f'{tag}: not an implicit-GEMM shape'
    with conv_mode(mode, det):
        torch.manual_seed(seed)
        m = layer.module(dev, bias=True)
        fam, var = library_answers(m.geom, n, in_sz)
        assert fam == tuple(p['family'] for p in plans), f'{tag}: families {fam}, the mirror expects {[p["family"] for p in plans]}'
        assert var == tuple(p['variant'] for p in plans), f'{tag}: variants {var}, the mirror expects {[p["variant"] for p in plans]}'
        if not need_dw:
            m.weight.requires_grad_(False)
            m.bias.requires_grad_(False)
        x = torch.randn(n, layer.cin, *in_sz)
        xg = x.to(dev).requires_grad_(need_dx)
        w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
        y = m(xg, act=act, slope=R.SLOPE)
        pre, den = R.ref_forward(layer, x, w, b)
        check(f'{tag} fwd', y, R.act64(pre, act), den, plan_bar(plans[0]), lambda i: R.locate(i, plans[0]))
        for p in m.parameters():
            p.grad = torch.zeros_like(p) if p.requires_grad else None
        g = torch.randn(y.shape)
        y.backward(g.to(dev))
        dz = _dz(case, g, y)
        out = {'y': y.detach().cpu()}
        if need_dx:
            ref, dden = R.ref_dgrad(layer, dz, w, x.shape)
            check(f'{tag} dgrad', xg.grad, ref, dden, plan_bar(plans[1]), lambda i: R.locate(i, plans[1]))
            untouched = dden == 0                       # input positions no output reads (1x1 stride 2): exactly zero
            if bool(untouched.any()):
                assert float(xg.grad.detach().cpu()[untouched].abs().max()) == 0.0, f'{tag}: dx is not 0 where no tap reaches'
            out['dx'] = xg.grad.detach().cpu().clone()
        if need_dw:
            pixels = max(p['npix'] for p in plans[2]['phases'])
            wbar = plan_bar(plans[2], pixels)
            bbar = R.BF3_BAR if plans[2]['family'] == 1 else R.f32_bar(n * math.prod(layer.out_size(in_sz)))
            gw1, gb1 = m.weight.grad.clone(), m.bias.grad.clone()
            rw, dw = R.ref_wgrad(layer, x, dz)
            rb, db = R.ref_bgrad(dz)
            check(f'{tag} wgrad', gw1, rw, dw, wbar, _weight_where)
            check(f'{tag} dbias', gb1, rb, db, bbar, _bias_where)
            # the kernels accumulate into .grad: a second backward gives twice the first
            y2 = m(xg, act=act, slope=R.SLOPE)
            y2.backward(g.to(dev))
            dz2 = _dz(case, g, y2)
            if torch.equal(dz2, dz):
                rw, dw, rb, db = 2 * rw, 2 * dw, 2 * rb, 2 * db
            else:                                        # (split-K atomics: an output next to 0 may change its sign between runs)
                rw, dw = R.ref_wgrad(layer, x, dz + dz2)
                rb, db = R.ref_bgrad(dz + dz2)
            check(f'{tag} wgrad accumulated', m.weight.grad, rw, dw, wbar, _weight_where)
            check(f'{tag} dbias accumulated', m.bias.grad, rb, db, bbar, _bias_where)
            out['gw'], out['gb'] = gw1.cpu(), gb1.cpu()
        return out


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_conv_kernel_case(dev, case):
    """run mode (a): x and the parameters need gradients (the fused dy * act'(y) preamble where both directions are bf16x3)"""
    run_case(dev, case, 5000 + CASES.index(case))


MARKED_B = [c for c in CASES if 'b' in c.marks]
MARKED_C = [c for c in CASES if 'c' in c.marks]


@pytest.mark.parametrize('case', MARKED_B, ids=[c.id for c in MARKED_B])
def test_conv_weight_gradient_alone(dev, case):
    """run mode (b): the input needs no gradient - muvo_act_bwd, the weight gradient's own split passes, bias_grad_kernel"""
    run_case(dev, case, 6000 + CASES.index(case), need_dx=False)


@pytest.mark.parametrize('case', MARKED_C, ids=[c.id for c in MARKED_C])
def test_conv_data_gradient_alone(dev, case):
    """run mode (c): frozen parameters - the data gradient splits dy itself"""
    run_case(dev, case, 7000 + CASES.index(case), need_dw=False)


SPLIT_K = split_k_cases()


@pytest.mark.parametrize('case', SPLIT_K, ids=[c.id for c in SPLIT_K])
def test_conv_deterministic(dev, case):
    """run mode (d): deterministic mode runs the split-K shapes unsplit; two runs are bit-identical"""
    for op in OPS:
        assert all(p['ksplit'] == 1 for p in R.conv_plan(case.layer, case.n, case.in_sz, op, case.mode, det=True)['phases'])
    seed = 8000 + CASES.index(case)
    a = run_case(dev, case, seed, det=True)
    b = run_case(dev, case, seed, det=True)
    for k in a:
        assert torch.equal(a[k], b[k]), f'{case.id}: {k} differs between two deterministic runs'


@pytest.mark.parametrize('case', WGRAD_BF3_IN_F32, ids=[c.id for c in WGRAD_BF3_IN_F32])
def test_wgrad_bf16x3_products_in_fp32_kernel(dev, case):
    """conv_wgrad_kernel<..., true>: no query names this variant, so the arithmetic identifies it - the bf16x3 bar holds AND the
    rms error is above the fp32 bar of the case (else the launch ran on fp32 products: the mirror's 2-GFLOP rule or the case is
    wrong)."""
    layer, n, in_sz = case.layer, case.n, case.in_sz
    plan = R.conv_plan(layer, n, in_sz, 'wgrad', BF3)
    assert plan['family'] == 0 and all(p['kernel'].endswith('true>') for p in plan['phases']), plan['phases']
    with conv_mode(BF3):
        torch.manual_seed(9000 + WGRAD_BF3_IN_F32.index(case))
        m = layer.module(dev, bias=True)         # (with a bias the stem kernels do not take the shape)
        fam, _ = library_answers(m.geom, n, in_sz)
        assert fam[2] == 0, fam
        x = torch.randn(n, layer.cin, *in_sz)
        y = m(x.to(dev))
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        g = torch.randn(y.shape)
        y.backward(g.to(dev))
        rw, dw = R.ref_wgrad(layer, x, g)
        rb, db = R.ref_bgrad(g)
        pixels = n * math.prod(layer.out_size(in_sz))
        s = check(f'{case.id} wgrad (bf16x3 products, fp32 staging)', m.weight.grad, rw, dw, R.BF3_BAR, _weight_where)
        check(f'{case.id} dbias', m.bias.grad, rb, db, R.f32_bar(pixels), _bias_where)
        assert s['rms'] > R.f32_bar(pixels)[0], (f'{case.id}: rms {s["rms"]:.3e} is within the fp32 bar {R.f32_bar(pixels)[0]:.3e}: '
                                                 'the launch ran on fp32 products')


@pytest.mark.parametrize('case', PW_CASES, ids=[c.id for c in PW_CASES])
def test_pw_head_kernels(dev, case):
    """conv_pw.hip for 1 ... 4 produced channels: forward with bias, data gradient, weight and bias gradient, and the data
    gradient accumulated into a non-zero trunk gradient (muvo_conv_dgrad_accumulate through ops.head_branch)."""
    from muvo_amd import ops
    layer, n, in_sz = case.layer, case.n, case.in_sz
    assert R.conv_plan(layer, n, in_sz, 'fwd', case.mode) is None and R.pw_applicable(layer, in_sz)
    s_out = n * math.prod(in_sz)
    with conv_mode(case.mode):
        torch.manual_seed(9100 + PW_CASES.index(case))
        m = layer.module(dev, bias=True)
        fam, _ = library_answers(m.geom, n, in_sz)
        assert fam == (3, 3, 3), fam
        x = torch.randn(n, layer.cin, *in_sz)
        xg = x.to(dev).requires_grad_(True)
        w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        y = m(xg)
        ref, den = R.ref_forward(layer, x, w, b)
        check(f'{case.id} pw fwd', y, ref, den, R.f32_bar(layer.cin))
        g = torch.randn(y.shape)
        y.backward(g.to(dev))
        ref, den = R.ref_dgrad(layer, g, w, x.shape)
        check(f'{case.id} pw dgrad', xg.grad, ref, den, R.f32_bar(layer.cout))
        rw, dw = R.ref_wgrad(layer, x, g)
        rb, db = R.ref_bgrad(g)
        check(f'{case.id} pw wgrad', m.weight.grad, rw, dw, R.f32_bar(s_out), _weight_where)
        check(f'{case.id} pw dbias', m.bias.grad, rb, db, R.f32_bar(s_out), _bias_where)
        # head hanging off a trunk: the head's data gradient is added into the trunk's non-zero gradient in place
        t = x.to(dev).requires_grad_(True)
        a, logits = ops.head_branch(t * 1.0, m.weight, m.bias, m.geom, m._packed)
        assert type(logits.grad_fn).__name__.startswith('HeadBranchFn')
        up = torch.randn(x.shape)
        torch.autograd.backward([a * 1.0, logits], [up.to(dev), g.to(dev)])
        hd, hden = R.ref_dgrad(layer, g, w, x.shape)
        check(f'{case.id} pw dgrad accumulated', t.grad, up.double() + hd, (up.double() ** 2 + hden ** 2).sqrt(),
              R.f32_bar(layer.cout + 1))
        check(f'{case.id} pw wgrad accumulated', m.weight.grad, 2 * rw, 2 * dw, R.f32_bar(s_out), _weight_where)


@pytest.mark.parametrize('case', HEAD_CASES, ids=[f'{c[0].name()}-n{c[1]}-{c[2][0]}x{c[2][1]}-co{c[3]}-{"trunk" if c[4] else "head-only"}'
                                                  for c in HEAD_CASES])
def test_fused_head_epilogue(dev, case):
    """ops.conv_head: ELU(ConvTranspose2d) with the 1x1 head formed in the epilogue of the eight-wave tiles (64 channels per
    group: one wave, direct store; 128: spread over waves, atomic adds, bias once).  The logits against the float64 head applied
    to the kernel's OWN y with the fp32 bar (the epilogue alone) and against the full float64 composition with the bf16x3 bar; the
    head's gradients and the stage's dx, dW, db with normalised bars."""
    from muvo_amd import nn as hnn
    from muvo_amd import ops
    layer, n, in_sz, co, trunk = case
    tag = f'{layer.name()}-co{co}-{"trunk" if trunk else "head-only"}'
    plans = [R.conv_plan(layer, n, in_sz, op, BF3) for op in OPS]
    assert all(p['family'] == 1 for p in plans) and plans[0]['variant'] == 1
    with conv_mode(BF3):
        torch.manual_seed(9200 + HEAD_CASES.index(case))
        conv = layer.module(dev, bias=True)
        with torch.device(dev):
            head = hnn.Conv2d(layer.cout, co, 1, 1, 0)
        x = torch.randn(n, layer.cin, *in_sz)
        xg = x.to(dev).requires_grad_(True)
        assert ops.conv_head_supported(xg, conv.geom, head.geom)
        d = conv.geom.plan(n, (1,) + tuple(in_sz))[0]
        assert ops.lib().muvo_conv_forward_head_supported(ctypes.byref(d), co) == 1
        params = (conv.weight, conv.bias, head.weight, head.bias)
        for p in params:
            p.grad = torch.zeros_like(p)
        y, logits = ops.conv_head(xg, conv.weight, conv.bias, conv.geom, conv._packed, ELU, 0.0, head.weight, head.bias,
                                  head.geom, head._packed)
        w, b, hw, hb = (p.detach().cpu() for p in params)
        hl = R.Layer('conv2d', layer.cout, co, 1, 1, 0, 0)
        pre, den = R.ref_forward(layer, x, w, b)
        yref = R.act64(pre, ELU)
        check(f'{tag} stage fwd', y, yref, den, R.BF3_BAR, lambda i: R.locate(i, plans[0]))
        own, oden = R.ref_forward(hl, y, hw, hb)
        check(f'{tag} logits vs head(own y)', logits, own, oden, R.f32_bar(layer.cout))
        # full composition: the error of y (scale den) propagates through |head weight|
        full, _ = R.ref_forward(hl, yref, hw, hb)
        fden = torch.nn.functional.conv2d(den ** 2, hw.double() ** 2).sqrt()
        check(f'{tag} logits vs float64 composition', logits, full, fden, R.BF3_BAR)
        gl, gy = torch.randn(logits.shape), torch.randn(y.shape)
        if trunk:
            torch.autograd.backward([y, logits], [gy.to(dev), gl.to(dev)])
        else:
            logits.backward(gl.to(dev))
            gy = torch.zeros(y.shape)
        # head gradients (the fused pass forms them from the kernel's own y)
        yo = y.detach().cpu()
        rhw, dhw = R.ref_wgrad(hl, yo, gl)
        rhb, dhb = R.ref_bgrad(gl)
        pixels = n * math.prod(layer.out_size(in_sz))
        check(f'{tag} head dW', head.weight.grad, rhw, dhw, R.f32_bar(pixels), _weight_where)
        check(f'{tag} head db', head.bias.grad, rhb, dhb, R.f32_bar(pixels), _bias_where)
        hd, _ = R.ref_dgrad(hl, gl, hw, y.shape)
        dz = (gy.double() + hd) * R.act_derivative(y, ELU).double()
        ref, dden = R.ref_dgrad(layer, dz, w, x.shape)
        check(f'{tag} dx', xg.grad, ref, dden, R.BF3_BAR, lambda i: R.locate(i, plans[1]))
        rw, dw = R.ref_wgrad(layer, x, dz)
        rb, db = R.ref_bgrad(dz)
        check(f'{tag} dW', conv.weight.grad, rw, dw, R.BF3_BAR, _weight_where)
        check(f'{tag} db', conv.bias.grad, rb, db, R.BF3_BAR, _bias_where)


@pytest.mark.parametrize('shape', LINEAR_CASES, ids=['x'.join(map(str, s)) for s in LINEAR_CASES])
def test_linear_token_major(dev, shape):
    """ops.LinearBf16x3Fn (token-major output, float4 row epilogue, out_sC == 1) at row counts that are no multiple of a pixel
    tile: forward with ELU, data gradient, weight and bias gradient."""
    from muvo_amd import nn as hnn
    from muvo_amd import ops
    rows, in_f, out_f = shape
    with_w = out_f % 16 == 0
    with conv_mode(BF3):
        torch.manual_seed(9300 + rows + out_f)
        with torch.device(dev):
            lin = hnn.Linear(in_f, out_f)
        lin.weight.requires_grad_(with_w)
        lin.bias.requires_grad_(with_w)
        x = torch.randn(rows, in_f)
        xg = x.to(dev).requires_grad_(with_w)
        w, b = lin.weight.detach().cpu(), lin.bias.detach().cpu()
        for p in lin.parameters():
            p.grad = torch.zeros_like(p) if with_w else None
        y = ops.LinearBf16x3Fn.apply(xg, lin.weight, lin.bias, ELU, 0.0)
        pre, den = R.ref_linear(x, w, b)
        tag = f'linear {rows}x{in_f}->{out_f}'
        check(f'{tag} fwd', y, R.act64(pre, ELU), den, R.BF3_BAR)
        g = torch.randn(y.shape)
        y.backward(g.to(dev))
        dz = g.double() * R.act_derivative(y, ELU).double()
        ref, dden = R.ref_matmul(dz, w)
        check(f'{tag} dgrad', xg.grad, ref, dden, R.BF3_BAR)
        rw, dw = R.ref_matmul(dz.t(), x)
        check(f'{tag} wgrad', lin.weight.grad, rw, dw, R.BF3_BAR, _weight_where)
        check(f'{tag} dbias', lin.bias.grad, dz.sum(0), (dz * dz).sum(0).sqrt(), R.f32_bar(rows), _bias_where)
