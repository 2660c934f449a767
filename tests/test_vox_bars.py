"""CPU self-test of the voxel-kernel bars (tests/test_vox_kernels_gpu.py): on the shapes of that matrix (x cropped), the CPU
emulation of the kernels' bf16x3 arithmetic passes the bars with a margin of 2, while the two subtle faults an elementwise
rtol misses - one cross product lost everywhere, both cross products of one tap lost - fail them by 4x or more.  Also checks
that the matrix reaches every kernel instantiation the dispatch can take (all that conv_vox.hip compiles)."""
import pytest
import torch

import vox_reference as V
from test_vox_kernels_gpu import AFFINE_CASES, CASES, DET_CASES, OPS, PRODUCTION_CASES

MARGIN, SEPARATION = 2.0, 4.0
CENTRE = (1, 1, 1)          # the tap whose lo terms the faulty form drops: never in the padding, so every element sees it


def _reduced(case):
    cin, cout, n, (x, y, z), act, mode = case
    return cin, cout, min(n, 2), (min(x, 6), min(y, 24), z), act, mode


BF3_SHAPES = sorted({_reduced(c) for c in CASES + PRODUCTION_CASES if c[5] == 'bf3'}, key=str)


def _operands(cin, cout, n, shape, seed):
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / (cin * 27) ** 0.5
    x = torch.randn(n, cin, *shape, generator=g)
    w = (torch.rand(cout, cin, 3, 3, 3, generator=g) * 2 - 1) * bound
    dy = torch.randn(n, cout, *shape, generator=g)
    return x, w, dy


@pytest.mark.parametrize('case', BF3_SHAPES, ids=[f'{c[0]}to{c[1]}-n{c[2]}-{"x".join(map(str, c[3]))}' for c in BF3_SHAPES])
def test_bf16x3_bars_separate_faults(case):
    cin, cout, n, shape, _, _ = case
    x, w, dy = _operands(cin, cout, n, shape, 7)
    bar = V.BARS['bf3']
    legs = {
        'fwd': (V.ref_forward(x, w), lambda f: V.emulate_forward(x, w, f, CENTRE)),
        'dgrad': (V.ref_dgrad(dy, w, x.shape), lambda f: V.emulate_dgrad(dy, w, x.shape, f, CENTRE)),
        'wgrad': (V.ref_wgrad(x, dy, w.shape), lambda f: V.emulate_wgrad(x, dy, w.shape, f, CENTRE)),
    }
    for op, ((ref, den), emu) in legs.items():
        good = V.excess(V.error_stats(emu('bf16x3'), ref, den), bar)
        assert good <= 1.0 / MARGIN, f'{op}: the bf16x3 emulation uses {good:.2f} of the bar (at most {1 / MARGIN})'
        for form in ('two_products', 'tap_lo_dropped'):
            bad = V.excess(V.error_stats(emu(form), ref, den), bar)
            assert bad >= SEPARATION, f'{op}: the faulty form {form} exceeds the bar only {bad:.2f}x'


@pytest.mark.parametrize('case', AFFINE_CASES, ids=[f'{c[0]}to{c[1]}-{"x".join(map(str, c[3]))}' for c in AFFINE_CASES])
def test_affine_padding_after_map_is_separated(case):
    """With the shifts of the GPU test (|shift| ~ 3), zero padding applied before the affine map instead of after it fails
    the bars by far, forward and weight gradient, while the bf16x3 emulation of the right order passes them."""
    cin, cout, n, (xx, yy, zz) = case
    x, w, dy = _operands(cin, cout, n, (min(xx, 6), yy, zz), 11)
    aff = torch.empty(n, cin, 2)
    aff[..., 0].uniform_(0.3, 2.0)
    aff[..., 1] = 3.0 * torch.where(torch.rand(n, cin) < 0.5, -1.0, 1.0)
    a = V.affine_input(x, aff)
    bar = V.BARS['bf3']
    ref, den = V.ref_forward(a, w)
    assert V.excess(V.error_stats(V.emulate_forward(a, w), ref, den), bar) <= 1.0 / MARGIN
    padded = torch.nn.functional.pad(x.double(), (1, 1, 1, 1, 1, 1))
    wrong = padded * aff[:, :, 0, None, None, None].double() + aff[:, :, 1, None, None, None].double()
    assert V.excess(V.error_stats(torch.nn.functional.conv3d(wrong, w.double()), ref, den), bar) >= SEPARATION
    rw, dw = V.ref_wgrad(a, dy, w.shape)
    assert V.excess(V.error_stats(V.emulate_wgrad(a, dy, w.shape), rw, dw), bar) <= 1.0 / MARGIN
    wrong_w = torch.nn.grad.conv3d_weight(wrong, w.shape, dy.double(), padding=0)
    assert V.excess(V.error_stats(wrong_w, rw, dw), bar) >= SEPARATION


# Every instantiation vox_conv_dispatch / vox_wgrad can launch, i.e. every templated kernel of conv_vox.hip (template arguments
# as rocprofv3 prints them; GENERIC = true for an activation beyond LeakyReLU or an accumulating pass).
REACHABLE = (
    [f'vox_bf3_ps_kernel<{z}, 8, {co8}, {g}>' for z in (16, 32, 64) for co8 in ('true', 'false') for g in ('true', 'false')]
    + [f'vox_bf3_2row_kernel<{z}, 8, {g}>' for z in (32, 64) for g in ('true', 'false')]
    + [f'vox_bf3_kernel<8, {z}, 8, {g}>' for z in (32, 64) for g in ('true', 'false')]
    + ['vox_bf3_wgrad_ps_kernel<16, 16, true, 4>', 'vox_bf3_wgrad_ps_kernel<16, 16, false, 0>']
    + [f'vox_bf3_wgrad_ps_kernel<{z}, 8, true, 0>' for z in (32, 64)]
    + [f'vox_bf3_wgrad_ps_kernel<{z}, 16, true, 4>' for z in (32, 64)]
    + [f'vox_bf3_wgrad_ps_kernel<{z}, 16, false, 0>' for z in (32, 64)]
    + [f'vox_bf3_wgrad_kernel<{z}, 8, false>' for z in (32, 64)]
    + [f'vox_conv_kernel<{cq}, {ty}, {z}>' for cq, ty in ((2, 6), (4, 4)) for z in (32, 64)]
    + [f'vox_wgrad_kernel<{r}, {c}, {z}, {4 if z == 64 else 8}>' for r, c in ((4, 2), (2, 1)) for z in (32, 64)]
)


def test_matrix_reaches_every_instantiation():
    reached = set()
    for cin, cout, n, shape, act, mode in CASES + PRODUCTION_CASES:
        for op in OPS:
            p = V.vox_plan(cin, cout, n, shape, op, act, mode)
            if p:
                reached.update(p['kernels'])
    for cin, cout, n, shape in DET_CASES:
        reached.update(V.vox_plan(cin, cout, n, shape, 'wgrad', det=True)['kernels'])
    missing = sorted(set(REACHABLE) - reached)
    assert not missing, f'no case reaches {missing}'
    assert reached <= set(REACHABLE), sorted(reached - set(REACHABLE))


def test_segmentation_edges():
    """The geometry the matrix exists for: a last x segment of one plane at N = 1, and 11, 11, 11, 8 at the top level."""
    p = V.vox_plan(16, 8, 1, (50, 8, 32), 'fwd')
    assert p['xseg'] == 7 and 50 % 7 == 1
    p = V.vox_plan(16, 8, 2, (41, 192, 64), 'fwd')
    assert p['xseg'] == 11 and 41 - 3 * 11 == 8
