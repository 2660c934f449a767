"""-m gpu: the 3x3x3 voxel convolution kernels (muvo_amd/csrc/conv_vox.hip) against float64 CPU references, with the normalised
error metric of tests/vox_reference.py and bars at the scale of the arithmetic (bf16x3 or exact fp32) rather than an
elementwise rtol.  Every case names the kernel instantiations each direction must reach (vox_reference.vox_plan, a restatement
of the dispatch) and checks that muvo_conv_kernel_family agrees, so a policy change cannot silently move a case off the kernel
it exists for.  On failure the worst element is printed with its x segment and y tile."""
import contextlib
import ctypes

import pytest
import torch

import vox_reference as V

pytestmark = pytest.mark.gpu

NONE, RELU, LEAKY, ELU = V.ACT_NONE, V.ACT_RELU, V.ACT_LEAKY, V.ACT_ELU
ACT_NAMES = {NONE: 'none', RELU: 'relu', LEAKY: 'leaky', ELU: 'elu'}
OPS = ('fwd', 'dgrad', 'wgrad')

# (Cin, Cout, N, (X, Y, Z), forward activation, mode).  Output rows per tile: plane-streaming 8, two-row 16, vox_bf3 8; weight
# gradient 4 / 8 / 16 at Z = 64 / 32 / 16; fp32 vox_conv 6 (8 produced channels) / 4 (16).  With N = 1 and one y tile, X = 50
# splits into x segments of 7: seven of them and a last one of a single plane.
CASES = [
    (16, 8, 3, (5, 9, 32), RELU, 'bf3'),        # Y one above the tile; 8 -> 16 data gradient on vox_bf3<8, 32>
    (16, 8, 1, (50, 8, 32), ELU, 'bf3'),        # segments 7 x 7 + 1, GENERIC forward
    (16, 16, 3, (2, 7, 64), LEAKY, 'bf3'),      # X = 2, Y one below the tile
    (16, 16, 1, (50, 4, 64), ELU, 'bf3'),       # segments 7 x 7 + 1 at Z = 64
    (8, 8, 3, (3, 17, 32), ELU, 'bf3'),         # two-row kernel, Y one above its 16-row tile
    (8, 8, 2, (1, 15, 64), ELU, 'bf3'),         # X = 1, Y one below the 16-row tile
    (8, 16, 3, (4, 1, 64), ELU, 'bf3'),         # Y = 1; 8 -> 16 weight gradient on vox_bf3_wgrad<64, 8>
    (8, 16, 1, (50, 8, 32), ELU, 'bf3'),        # segmented vox_bf3<8, 32> and vox_bf3_wgrad<32, 8>
    (32, 16, 3, (3, 9, 32), LEAKY, 'bf3'),      # two accumulating passes (cin_total stride, N = 3)
    (32, 8, 3, (2, 5, 64), NONE, 'bf3'),        # two passes into 8 channels; 8 -> 32 data gradient on vox_bf3<8, 64>
    (64, 8, 1, (50, 8, 32), RELU, 'bf3'),       # four passes, segmented
    (16, 32, 3, (3, 9, 64), ELU, 'bf3'),        # 32 produced channels (two row blocks); 32 -> 16 data gradient in two passes
    (32, 32, 3, (2, 17, 16), LEAKY, 'bf3'),     # z lines of 16; weight-gradient tile of 16 rows, Y one above it
    (32, 8, 3, (3, 15, 16), ELU, 'bf3'),        # Z = 16 into 8 channels, Y one below the 16-row weight-gradient tile
    (16, 8, 1, (1, 1, 16), NONE, 'bf3'),        # X = Y = 1 at Z = 16
    (64, 16, 2, (2, 5, 32), ELU, 'bf3'),        # four passes into 16 channels
    (64, 32, 1, (50, 4, 16), NONE, 'bf3'),      # four passes at Z = 16, segments 7 x 7 + 1
    # exact fp32 kernels (CONV_F32): vox_conv_kernel <2, 6> / <4, 4> and vox_wgrad_kernel <4, 2> / <2, 1> at Z = 64 and 32
    (16, 8, 3, (3, 13, 64), LEAKY, 'f32'),
    (8, 16, 3, (5, 7, 32), ELU, 'f32'),
    (8, 8, 1, (2, 5, 64), RELU, 'f32'),
    (16, 16, 2, (7, 9, 32), NONE, 'f32'),
]

# One case per level of the voxel decoder at its real Y x Z, N = 2, X cropped (41 planes at 192 x 192 x 64 segment as 11, 11,
# 11, 8), LeakyReLU as in DecoderBlock3d.
PRODUCTION_CASES = [
    (64, 32, 2, (48, 48, 16), LEAKY, 'bf3'),
    (32, 32, 2, (48, 48, 16), LEAKY, 'bf3'),
    (32, 16, 2, (40, 96, 32), LEAKY, 'bf3'),
    (16, 16, 2, (40, 96, 32), LEAKY, 'bf3'),
    (16, 8, 2, (41, 192, 64), LEAKY, 'bf3'),
    (8, 8, 2, (41, 192, 64), LEAKY, 'bf3'),
]

# affine staging (muvo_conv_forward_affine / muvo_conv_wgrad_affine): (Cin, Cout, N, (X, Y, Z)), one pass and segmented
AFFINE_CASES = [
    (16, 8, 2, (3, 9, 32)),
    (16, 16, 1, (50, 4, 64)),
    (8, 8, 2, (4, 17, 32)),
    (8, 16, 1, (50, 8, 64)),
]

# deterministic mode: the weight gradient moves to the exact-fp32 ticketed kernel
DET_CASES = [
    (16, 8, 2, (5, 9, 64)),
    (8, 16, 2, (6, 11, 32)),
]


def case_id(case, det=False):
    cin, cout, n, shape, act, mode = case
    names = []
    for op in OPS:
        p = V.vox_plan(cin, cout, n, shape, op, act, mode, det)
        names.append(op + '-' + (V.short_name(p['kernels'][-1]) + (f'x{len(p["kernels"])}' if len(p['kernels']) > 1 else '')
                                 if p else 'gemm'))
    return f'{cin}to{cout}-n{n}-{"x".join(map(str, shape))}-{ACT_NAMES[act]}-{mode}-' + '-'.join(names)


@contextlib.contextmanager
def conv_mode(mode, det=False):
    from muvo_amd import ops
    old, was_det = ops.get_conv_mode(), ops.get_deterministic()
    try:
        if det:
            ops.set_deterministic(True)
        ops.set_conv_mode(ops.CONV_BF16X3 if mode == 'bf3' else ops.CONV_F32, min_gflop=0.0)
        yield
    finally:
        ops.set_conv_mode(old, min_gflop=-1.0)
        if det:
            ops.set_deterministic(was_det)


def families(m, n, shape):
    from muvo_amd import ops
    d = m.geom.plan(n, tuple(shape))[0]
    return tuple(ops.lib().muvo_conv_kernel_family(ctypes.byref(d), op) for op in (0, 1, 2))


def check_families(fam, plans, tag):
    for op, f, p in zip(OPS, fam, plans):
        if p is None:
            assert f not in (2, 4), f'{tag}: {op} runs on voxel family {f}, the dispatch mirror expects the implicit-GEMM kernels'
        else:
            assert f == p['family'], f'{tag}: {op} family {f}, expected {p["family"]} ({", ".join(p["kernels"])})'


def check(name, got, ref, den, bar, where):
    s = V.error_stats(got, ref, den)
    print(f'VOXSTAT {name}: max_e {s["max_e"]:.3e} rms {s["rms"]:.3e} (bars {bar[1]:.1e} / {bar[0]:.1e})')
    assert V.within(s, bar), (f'{name}: max(e) {s["max_e"]:.3e} (bar {bar[1]:.1e}), rms {s["rms"]:.3e} (bar {bar[0]:.1e}); '
                              f'worst {where(s["index"])}')
    return s


def _weight_where(idx):
    return f'(co, ci, kx, ky, kz) = {idx}'


def _bias_where(idx):
    return f'channel {idx[0]}'


def check_moments(name, buf, y):
    ref, scale = V.moments64(y)
    got = buf.detach().cpu()
    diff = (got - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())
    print(f'VOXSTAT {name} moments: max rel {worst:.3e} (bar {V.MOMENTS_BAR:.1e})')
    i = int((diff / scale.clamp_min(1e-300)).argmax())
    assert worst <= V.MOMENTS_BAR, f'{name}: moments off by {worst:.3e} of sum|y| at (n, c, stat) = {tuple(int(v) for v in torch.unravel_index(torch.tensor(i), diff.shape))}'


def _act_mask(y, act):
    """d act / d pre-activation from the kernel's own output (exact for LeakyReLU with slope > 0)."""
    yc = y.detach().cpu()
    if act == LEAKY:
        return torch.where(yc > 0, torch.ones_like(yc), torch.full_like(yc, V.SLOPE))
    return torch.ones_like(yc)


def run_case(dev, case, seed, det=False):
    from muvo_amd import nn as hnn
    from muvo_amd import ops
    cin, cout, n, shape, act, mode = case
    tag = case_id(case, det)
    plans = [V.vox_plan(cin, cout, n, shape, op, act, mode, det) for op in OPS]
    bars = [(V.BARS['bf3'] if p['family'] == 4 else V.BARS['f32']) if p else None for p in plans]
    assert plans[2] is not None, f'{tag}: every case exercises a voxel weight-gradient kernel'
    with conv_mode(mode, det):
        torch.manual_seed(seed)
        with torch.device(dev):
            m = hnn.Conv3d(cin, cout, 3, 1, 1, bias=True)
        check_families(families(m, n, shape), plans, tag)
        x = torch.randn(n, cin, *shape)
        xg = x.to(dev).requires_grad_(True)
        w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
        # forward with the case's activation, and the instance-norm moments where the epilogue produces them
        buf = ops.conv_moments_buffer(xg, m.geom)
        assert (buf is not None) == (plans[0] is not None and plans[0]['family'] == 4 and not det), f'{tag}: moments availability'
        y = m(xg, act=act, slope=V.SLOPE, moments=buf)
        fwd_where = lambda i: V.locate(i, plans[0])
        if plans[0] is not None:
            ref, den = V.ref_forward(x, w, b, act)
            check(f'{tag} fwd', y, ref, den, bars[0], fwd_where)
        if buf is not None:
            check_moments(tag, buf, y)
        # gradients: no activation, except LeakyReLU whose derivative comes from the sign of the kernel's own y
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        yb = y if act == LEAKY else m(xg)
        g = torch.randn(yb.shape)
        yb.backward(g.to(dev))
        dz = g * _act_mask(yb, act)
        if plans[1] is not None:
            ref, den = V.ref_dgrad(dz, w, x.shape)
            check(f'{tag} dgrad', xg.grad, ref, den, bars[1], lambda i: V.locate(i, plans[1]))
        gw1, gb1 = m.weight.grad.clone(), m.bias.grad.clone()
        rw, dw = V.ref_wgrad(x, dz, w.shape)
        rb, db = V.ref_bgrad(dz)
        check(f'{tag} wgrad', gw1, rw, dw, bars[2], _weight_where)
        check(f'{tag} dbias', gb1, rb, db, bars[2], _bias_where)
        # the kernels accumulate into .grad: a second backward gives twice the first
        y2 = m(xg, act=act, slope=V.SLOPE) if act == LEAKY else m(xg)
        y2.backward(g.to(dev))
        dz2 = g * _act_mask(y2, act)
        if not torch.equal(dz2, dz):
            rw, dw = V.ref_wgrad(x, dz2 + dz, w.shape)
            rb, db = V.ref_bgrad(dz2 + dz)
        else:
            rw, dw, rb, db = 2 * rw, 2 * dw, 2 * rb, 2 * db
        check(f'{tag} wgrad accumulated', m.weight.grad, rw, dw, bars[2], _weight_where)
        check(f'{tag} dbias accumulated', m.bias.grad, rb, db, bars[2], _bias_where)
        return gw1, gb1


@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_vox_kernel_case(dev, case):
    run_case(dev, case, 1000 + CASES.index(case))


@pytest.mark.parametrize('case', PRODUCTION_CASES, ids=[case_id(c) for c in PRODUCTION_CASES])
def test_vox_production_level(dev, case):
    run_case(dev, case, 2000 + PRODUCTION_CASES.index(case))


@pytest.mark.parametrize('case', DET_CASES, ids=[case_id(c + (NONE, 'bf3'), det=True) for c in DET_CASES])
def test_vox_deterministic_wgrad(dev, case):
    """Deterministic mode: the weight gradient runs on the exact-fp32 kernel (family 2, ordered adds): two runs are
    bit-identical and match float64 within the fp32 bar; forward and data gradient stay on bf16x3."""
    full = case + (NONE, 'bf3')
    seed = 3000 + DET_CASES.index(case)
    assert V.vox_plan(*case, 'wgrad', NONE, 'bf3', det=True)['family'] == 2
    gw1, gb1 = run_case(dev, full, seed, det=True)
    gw2, gb2 = run_case(dev, full, seed, det=True)
    assert torch.equal(gw1, gw2) and torch.equal(gb1, gb2), 'deterministic weight gradient differs between two runs'


@pytest.mark.parametrize('case', AFFINE_CASES, ids=[case_id(c + (LEAKY, 'bf3')) for c in AFFINE_CASES])
def test_vox_affine_staging(dev, case):
    """Convolution of scale * x + shift per (n, input channel) with the zero padding applied AFTER the map (the lazy AdaIN of
    DecoderBlock3d), forward (with moments) and weight gradient.  |shift| ~ 3: padding before the map would put an O(1) error
    on every border voxel, while interior x-segment borders must see the real neighbours."""
    from muvo_amd import nn as hnn
    from muvo_amd import ops
    cin, cout, n, shape = case
    tag = case_id(case + (LEAKY, 'bf3'))
    plans = [V.vox_plan(cin, cout, n, shape, op, LEAKY, 'bf3') for op in OPS]
    bar = V.BARS['bf3']
    with conv_mode('bf3'):
        torch.manual_seed(4000 + AFFINE_CASES.index(case))
        with torch.device(dev):
            m = hnn.Conv3d(cin, cout, 3, 1, 1, bias=True)
        check_families(families(m, n, shape), plans, tag)
        raw = torch.randn(n, cin, *shape)
        aff = torch.empty(n, cin, 2)
        aff[..., 0].uniform_(0.3, 2.0)
        aff[..., 1] = (2.5 + torch.rand(n, cin)) * torch.where(torch.rand(n, cin) < 0.5, -1.0, 1.0)
        rawg, affg = raw.to(dev), aff.to(dev).contiguous()
        ph = torch.empty(n, cin, *shape, device=dev).requires_grad_(True)      # the lazy AdaIN's placeholder output
        assert ops.conv_affine_supported(ph, m.geom, torch.zeros(1)), f'{tag}: no affine staging for this shape'
        buf = ops.conv_moments_buffer(ph, m.geom)
        assert buf is not None
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        y = m(ph, act=LEAKY, slope=V.SLOPE, moments=buf, lazy=(rawg, affg))
        a = V.affine_input(raw, aff)
        w, b = m.weight.detach().cpu(), m.bias.detach().cpu()
        ref, den = V.ref_forward(a, w, b, LEAKY)
        check(f'{tag} affine fwd', y, ref, den, bar, lambda i: V.locate(i, plans[0]))
        check_moments(f'{tag} affine', buf, y)
        g = torch.randn(y.shape)
        y.backward(g.to(dev))
        dz = g * _act_mask(y, LEAKY)
        ref, den = V.ref_dgrad(dz, w, raw.shape)
        check(f'{tag} affine dgrad', ph.grad, ref, den, bar, lambda i: V.locate(i, plans[1]))
        rw, dw = V.ref_wgrad(a, dz, w.shape)
        check(f'{tag} affine wgrad', m.weight.grad, rw, dw, bar, _weight_where)
        rb, db = V.ref_bgrad(dz)
        check(f'{tag} affine dbias', m.bias.grad, rb, db, bar, _bias_where)


@pytest.mark.parametrize('shape,voxel', [((1023, 1025, 32), True), ((1024, 1024, 32), False)])
def test_vox_descriptor_limit_family(dev, shape, voxel):
    """One sample addressed through a 32-bit buffer descriptor (vox_geometry_ok): just below 2 GiB the voxel kernels serve
    16 -> 8, at 2 GiB every direction falls back off families 2 / 4.  Family query only, nothing is launched."""
    from muvo_amd import ops
    with conv_mode('bf3'):
        d = ops.ConvDesc(3, 0, 1, 16, 8, (ctypes.c_int32 * 3)(*shape), (ctypes.c_int32 * 3)(*shape), (ctypes.c_int32 * 3)(3, 3, 3),
                         (ctypes.c_int32 * 3)(1, 1, 1), (ctypes.c_int32 * 3)(1, 1, 1), (ctypes.c_int32 * 3)(1, 1, 1))
        fam = tuple(ops.lib().muvo_conv_kernel_family(ctypes.byref(d), op) for op in (0, 1, 2))
        plans = [V.vox_plan(16, 8, 1, shape, op) for op in OPS]
        if voxel:
            assert fam == (4, 4, 4) and all(p['family'] == 4 for p in plans), fam
        else:
            assert all(f not in (2, 4) for f in fam) and all(p is None for p in plans), fam
