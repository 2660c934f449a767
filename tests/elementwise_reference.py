"""Plain float64 references, float32 CPU emulations of each kernel's operation order, planted faults, the case lists and a
restatement of the host dispatch for the pooling / upsample / glue unit (muvo_amd/csrc/elementwise.hip, plus
muvo_resize_bilinear_bwd of bev.hip).  Helpers only: no fixtures, no tests.  tests/test_elementwise_reference.py (CPU) and
tests/test_elementwise_kernels_gpu.py (GPU) share everything here, so the bars the GPU test applies are the ones the CPU test
proves to pass the emulated arithmetic and to reject the planted faults.

Metric.  vox_reference.error_stats: e = |got - ref64| / den per element next to rms(got - ref) / rms(ref); den is the scale of
the terms summed for that element, sqrt(sum (w x)^2) (the convention of gemm_reference.py).

References (float64, straight from the definition).  The trilinear x2 upsample (align_corners=False) is a per-axis matrix
(up2_matrix); forward = the three matrices applied, backward = their transposes, so forward, adjoint and the identity
<U x, g> = <x, U^T g> come from one object.  Max pooling: first maximum wins, winner byte a * K + b.  Softmax with dropout: P,
Pd = P * mask, dS = P (g - sum P g) with g = dPd * mask; the mask comes from the caller (on the GPU: the library's own
muvo_dropout over ones with the same seed, whose element index is row * cols + c, the convention of test_attention_stream_gpu).

Emulations (float32 on the CPU, every product and every sum rounded once: the library is built with -ffp-contract=off).
  upsample forward  'scalar' the nested form a (b (c v + fw v) + fh (..)) + fd (..);  'vec' the same form over the four clamped
                    column slots of a lane;  'row' the four rows blended first ((w00 r00 + w01 r01) + w10 r10) + w11 r11 with the
                    weights wd * wh of the 2 x 2 block form (0.75 / 0.25 on both clamped planes, also at the borders), then
                    0.25 / 0.75 across columns
  upsample backward 'scalar' the gather (row sums over c, then acc += (wa wb) row);  'vec' acc += (wa wb) (column form) over the
                    16 (a, b);  'row' plane contributions sum_b wb (column form) first, then (wa0 P + wa1 P) + (wa2 P + wa3 P)
                    (clamped, zero-weighted loads add an exact 0)
  average pool      64 strided lanes, then the xor butterfly of wave_sum, then / S
  softmax, GRU, RSSM sample, activations: the kernel's own sequence with the host's expf / tanhf / expm1f
  bilinear resize   the kernel's float32 coordinates and weights; forward the nested two-row form, adjoint the gather order

Bars.  A summing kernel's bar is 2 x the worst rms and 2 x the worst max e of its own emulation over its case list (OWN_WORST;
the margin of 2 is gemm_reference.OWN_WORST's: another rounding order of the same arithmetic).  Kernels with transcendentals get
4 x the plain float32 CPU evaluation (TRANS_WORST; attention_reference's rule: the device's functions are not the host's).  The
CPU test recomputes both tables and fails when they are stale.  No bar comes from a GPU run.

Dispatch mirror.  upsample_plan / maxpool_plan / softmax_plan restate muvo_upsample3d_route / muvo_maxpool2d_route /
muvo_softmax_dropout_route (MUVO_EW_GRID_CAP at its default of 4096)."""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from vox_reference import error_stats, excess, within  # noqa: F401

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_ELU, ACT_TANH, ACT_SIGMOID = range(6)
ACT_NAMES = ('none', 'relu', 'leaky', 'elu', 'tanh', 'sigmoid')
SLOPE = 0.2
MARKER = -12345.678          # canary value of the guard bands around every output (compared bit for bit)
GUARD = 8                    # guard elements in front of and behind an output
U32 = 2.0 ** -24
TINY = 1e-30                 # floor of the relative-error denominators: results that underflow float32 do not count

# ------------------------------------------------------------------------------------------------------------------- bars
# OWN_WORST: worst (rms, max e) of each summing kernel's own float32 emulation over its case list; the bar is 2 x that.
# TRANS_WORST: worst (rms, max e) of the plain float32 CPU evaluation of each kernel with expf / tanhf; the bar is 4 x that.
# tests/test_elementwise_reference.py::test_bar_tables_are_not_stale recomputes every entry (within 2 % / never above).
OWN_WORST = {
    'up_fwd_row': (6.384e-08, 3.257e-07), 'up_fwd_vec': (5.342e-08, 2.954e-07),
    'up_fwd_scalar': (5.611e-08, 2.486e-07),
    'up_bwd_row': (7.776e-08, 4.139e-07), 'up_bwd_vec': (8.972e-08, 6.221e-07),
    'up_bwd_scalar': (1.022e-07, 4.409e-07),
    'avgpool_fwd': (6.046e-07, 1.565e-07),           # (rms against the rms of the MEANS, which cancel: larger than max e)
    # the kernels form their source coordinates in float32: 96 / 42 * 40.5 = 92.6 is rounded at ulp(92.6) / 2 = 3.8e-6, which is
    # the error of the two weights of that output ((60, 96) -> (16, 42) sets both figures; the other cases stay below 1e-6)
    'resize_bilinear': (5.087e-06, 5.367e-05), 'resize_bilinear_bwd': (5.093e-06, 7.638e-05),
}
TRANS_WORST = {          # rms here: rms of the normalised error (norm_stats)
    'softmax_P': (2.291e-07, 2.054e-06), 'softmax_Pd': (2.145e-07, 2.135e-06), 'softmax_dS': (2.559e-07, 1.737e-06),
    # (the spiked rows: scores of size 3 minus a maximum of 80 or 100 are rounded at ulp(80) / 2 = 3.8e-6 before the exponential)
    'gru_fwd': (8.063e-08, 3.940e-07), 'gru_bwd': (1.252e-08, 5.648e-08),
    'sample_fwd': (5.898e-08, 1.482e-07), 'sample_bwd': (3.080e-08, 8.082e-08),
    'act_fwd': (3.574e-08, 9.790e-08),
}
# Measured on an MI355X by tests/test_elementwise_kernels_gpu.py (ELEMSTAT lines: largest max e / rms over all cases of a kernel
# and the largest share of its bar).  Not the source of any bar.
#   upsample forward   row 3.26e-7 / 6.38e-8   vec 2.95e-7 / 5.34e-8   scalar 2.49e-7 / 5.61e-8   (0.50 each)
#   upsample backward  row 4.14e-7 / 7.78e-8   vec 6.22e-7 / 8.97e-8   scalar 4.41e-7 / 1.02e-7   (0.50 each)
#   (vec: with the shapes that the retired eight-outputs forward and block-per-plane backward kernels used to take)
#   avgpool_fwd 1.57e-7 / 6.04e-7 (0.50)   resize_bilinear 5.37e-5 / 5.09e-6 (0.50)   resize_bilinear_bwd 7.64e-5 / 5.09e-6 (0.50)
#   (a share of 0.50 is the emulation's own worst case: the kernel rounds exactly as emulated)
#   softmax P 2.05e-6 / 2.29e-7 (0.25)   Pd 2.13e-6 / 2.06e-7 (0.25)   dS 1.74e-6 / 2.61e-7 (0.26)
#   gru_fwd 3.94e-7 / 8.11e-8 (0.25)   gru_bwd 5.65e-8 / 1.25e-8 (0.25)   sample_fwd 1.48e-7 / 5.70e-8 (0.25)
#   sample_bwd 8.08e-8 / 3.08e-8 (0.25)   act_fwd (ELU, tanh, sigmoid) 1.06e-7 / 3.62e-8 (0.27)
#   (a share of 0.25 is the host's float32 evaluation: the worst elements are set by the float32 rounding of the arguments)
#   bit for bit equal: max pool forward (3/2/1 and 2/2/0, 16-byte and scalar loads) and backward (eight-column, generic 3/2/1,
#   generic 2/2/0) over the four input families, avgpool backward, the dropout mask against host_dropout_mask, both token
#   transposes, mu of the sample, copy2d, axpby, batchsum, act_fwd (none, ReLU, LeakyReLU), resize_nearest (float32, uint8)


def kernel_bar(kind):
    if kind in OWN_WORST:
        return (2 * OWN_WORST[kind][0], 2 * OWN_WORST[kind][1])
    return (4 * TRANS_WORST[kind][0], 4 * TRANS_WORST[kind][1])


def norm_stats(got, ref, den):
    """error_stats with rms = rms((got - ref) / den): for the kernels with transcendentals, whose reference itself vanishes where
    the gates saturate or the softmax gradient cancels, so that rms(got - ref) / rms(ref) measures nothing"""
    st = error_stats(got, ref, den)
    st['rms'] = float(((_d(got) - ref) / den.clamp_min(1e-300)).pow(2).mean().sqrt())
    return st


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _cdiv(a, b):
    return -(-a // b)


def _d(t):
    return t.detach().cpu().double()


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ================================================================================================== dispatch mirror
def ew_grid(n, cap=4096):
    return max(1, min(_cdiv(n, 256), cap))


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def upsample_plan(backward, NC, D, H, W, in16=True, out16=True):
    """muvo_upsample3d_route: dict(kernel, grid, block, segs, dseg)"""
    oq = W // 2
    oq_ok = W % 4 == 0 and oq <= 64 and _pow2(oq)
    r = {'segs': 1, 'dseg': D, 'block': (256, 1, 1)}
    if not backward:
        if oq_ok and D + 1 <= 65535 and NC <= 65535 and in16 and out16:
            r.update(kernel='row', grid=(_cdiv((H + 1) * oq, 256), D + 1, NC))
        elif W % 2 == 0 and 2 * D <= 65535 and NC <= 65535 and out16:
            r.update(kernel='vec', grid=(_cdiv(2 * H * (2 * W // 4), 256), 2 * D, NC))
        else:
            r.update(kernel='scalar', grid=(ew_grid(NC * D * H * W * 8), 1, 1))
        return r
    if oq_ok and NC <= 65535 and in16 and out16:
        rg, segs = _cdiv(H, 256 // oq), 1
        while NC * rg * segs < 4096 and segs * 16 <= D:
            segs *= 2
        dseg = _cdiv(D, segs)
        r.update(kernel='row', dseg=dseg, segs=_cdiv(D, dseg), grid=(rg, _cdiv(D, dseg), NC))
    elif W % 4 == 0 and D <= 65535 and NC <= 65535 and in16 and out16:
        r.update(kernel='vec', grid=(_cdiv(H * (W // 4), 256), D, NC))
    else:
        r.update(kernel='scalar', grid=(ew_grid(NC * D * H * W), 1, 1))
    return r


# pointers each upsample kernel accesses with 16-byte instructions: (in, out)
UPSAMPLE_NEEDS16 = {(0, 'row'): (True, True), (0, 'vec'): (False, True), (0, 'scalar'): (False, False),
                    (1, 'row'): (True, True), (1, 'vec'): (True, True), (1, 'scalar'): (False, False)}
# (the backward row kernel stores dx as float2; the route asks for 16 bytes all the same)


def pool_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def maxpool_plan(backward, NC, H, W, k, s, p, in16=True, idx4=True, out16=True):
    """muvo_maxpool2d_route: dict(k, load16, v8, grid, block)"""
    OH, OW = pool_out(H, k, s, p), pool_out(W, k, s, p)
    r = {'k': k, 'load16': False, 'v8': False, 'block': (64, 4, 1)}
    if not backward:
        r['load16'] = s == 2 and W % 8 == 0 and OW * 2 == W and in16
        r['grid'] = (_cdiv(OW, 256), _cdiv(OH, 4), NC)
    elif k == 3 and W % 8 == 0 and OW % 4 == 0 and 2 * OW == W and 2 * OH == H and in16 and out16 and idx4:
        r['v8'] = True
        r['grid'] = (_cdiv(W // 8, 64), _cdiv(H // 2, 4), NC)
    else:
        r['grid'] = (_cdiv(W, 256), _cdiv(H, 4), NC)
    return r


SOFTMAX_MAX_COLS = 1088


def softmax_plan(cols):
    assert 0 < cols <= SOFTMAX_MAX_COLS
    return {'maxv': 8 if cols <= 512 else 17}


# ================================================================================================== case lists
def ucase(kernel, NC, D, H, W, in16=True, out16=True):
    mis = ('' if in16 else '-in+4B') + ('' if out16 else '-out+4B')
    return {'name': f'{kernel}-{NC}x{D}x{H}x{W}{mis}', 'kernel': kernel, 'NC': NC, 'D': D, 'H': H, 'W': W, 'in16': in16, 'out16': out16}


# Every case names the kernel it exists for (the mirror test checks that the dispatch agrees).  A misaligned x goes to the vec
# forward kernel (dword loads of x, float4 stores of y), a misaligned y to the scalar one; the backward kernels below the scalar
# one all take 16-byte loads of dy, so any misaligned pointer goes to the scalar gather.
UP_FWD_CASES = [
    ucase('row', 2, 1, 1, 4),            # OQ = 2, every axis clamps on both sides
    ucase('row', 3, 2, 3, 8),
    ucase('row', 1, 3, 5, 128),          # OQ = 64: 384 live lanes, a partial second workgroup
    ucase('row', 2, 2, 7, 32),
    ucase('vec', 2, 2, 3, 256),          # W / 2 = 128 is past the row kernel: 768 live lanes, three workgroups
    ucase('vec', 1, 1, 1, 256),
    ucase('vec', 2, 2, 3, 2), ucase('vec', 1, 3, 2, 6), ucase('vec', 2, 1, 4, 12), ucase('vec', 1, 2, 3, 20),
    ucase('vec', 3, 2, 3, 8, in16=False),          # a row shape with a misaligned x
    ucase('vec', 1, 1, 1, 256, in16=False),        # the widest shape with a misaligned x
    ucase('scalar', 2, 2, 3, 5), ucase('scalar', 1, 3, 3, 1),
    ucase('scalar', 65536, 1, 1, 4),     # NC beyond the z extent of a grid
    ucase('scalar', 3, 2, 3, 8, out16=False), ucase('scalar', 1, 1, 1, 256, out16=False), ucase('scalar', 2, 2, 3, 2, out16=False),
    ucase('scalar', 2, 2, 7, 32, in16=False, out16=False),
]
UP_BWD_CASES = [
    ucase('row', 2, 1, 1, 4),
    ucase('row', 1, 2, 5, 128),          # four coarse rows per workgroup: the last workgroup recomputes row H - 1
    ucase('row', 2, 17, 6, 32),          # two segments of 9 and 8
    ucase('row', 1, 33, 3, 8),           # four segments, the last of 6
    ucase('row', 1, 16, 2, 16),          # two segments of 8
    # W / 2 no power of two <= 64: the float4 gather, one lane per four coarse columns, H (W / 4) lanes per (d, nc)
    ucase('vec', 1, 1, 43, 12),          # 129 lanes
    ucase('vec', 2, 9, 43, 12),
    ucase('vec', 1, 8, 22, 24),
    ucase('vec', 1, 2, 341, 12),         # 1023 lanes: four workgroups, the last with 255 live lanes
    ucase('vec', 1, 1, 2, 256),          # W / 2 = 128 is past the row kernel: 128 lanes
    ucase('vec', 1, 2, 16, 256),         # 1024 lanes: exactly four workgroups
    ucase('vec', 1, 2, 3, 12), ucase('vec', 1, 1, 42, 12), ucase('vec', 1, 1, 342, 12),      # 9 / 126 / 1026 lanes
    ucase('scalar', 2, 2, 3, 5), ucase('scalar', 1, 2, 2, 6), ucase('scalar', 1, 3, 3, 2),
    ucase('scalar', 65536, 1, 1, 4),
    ucase('scalar', 1, 16, 2, 16, in16=False), ucase('scalar', 1, 2, 3, 12, in16=False),
    ucase('scalar', 1, 8, 22, 24, out16=False), ucase('scalar', 1, 2, 3, 12, out16=False),
]


def up_inputs(c, backward):
    """the float32 input of a case: x (NC, D, H, W) forward, dy (NC, 2D, 2H, 2W) backward"""
    g = _gen('up', backward, c['NC'], c['D'], c['H'], c['W'])
    m = 2 if backward else 1
    return torch.randn(c['NC'], m * c['D'], m * c['H'], m * c['W'], generator=g)


def mcase(kind, NC, H, W, k, in16=True, out16=True):
    s, p = 2, (1 if k == 3 else 0)
    mis = ('' if in16 else '-in+4B') + ('' if out16 else '-out+4B')
    return {'name': f'{kind}-{NC}x{H}x{W}{mis}', 'kind': kind, 'NC': NC, 'H': H, 'W': W, 'k': k, 's': s, 'p': p, 'in16': in16,
            'out16': out16}


# kind: forward '<k>-load16' / '<k>-scalar', backward 'v8' / '<k>-generic'
MAXPOOL_FWD_CASES = [
    mcase('3-load16', 2, 2, 8, 3), mcase('3-load16', 3, 5, 16, 3), mcase('3-load16', 1, 4, 520, 3),      # OW = 260: two column groups
    mcase('3-scalar', 2, 7, 7, 3), mcase('3-scalar', 1, 5, 18, 3), mcase('3-scalar', 1, 1, 1, 3), mcase('3-scalar', 2, 4, 8, 3, in16=False),
    mcase('2-load16', 2, 4, 8, 2), mcase('2-scalar', 3, 6, 6, 2), mcase('2-scalar', 1, 5, 7, 2),          # odd: last row / column unused
    mcase('2-scalar', 2, 4, 8, 2, in16=False),
]
MAXPOOL_BWD_CASES = [
    mcase('v8', 2, 2, 8, 3), mcase('v8', 1, 4, 8, 3), mcase('v8', 1, 10, 520, 3),      # 65 lanes in two groups, five row pairs
    mcase('v8', 3, 6, 24, 3),
    mcase('3-generic', 2, 7, 18, 3), mcase('3-generic', 1, 5, 8, 3),                    # 2 OH != H
    mcase('3-generic', 1, 4, 8, 3, in16=False), mcase('3-generic', 1, 4, 8, 3, out16=False),
    mcase('2-generic', 2, 4, 8, 2), mcase('2-generic', 1, 5, 7, 2),
]
MAXPOOL_FAMILIES = ('random', 'ties', 'constant', 'negative')


def maxpool_kind(plan, backward):
    if backward:
        return 'v8' if plan['v8'] else f"{plan['k']}-generic"
    return f"{plan['k']}-{'load16' if plan['load16'] else 'scalar'}"


def maxpool_inputs(c, family):
    """(x, dy): x of the family, dy dyadic (multiples of 2^-10 below 4: the up-to-four-term sums are exact in any order)"""
    g = _gen('maxpool', c['NC'], c['H'], c['W'], c['k'], family)
    x = torch.randn(c['NC'], c['H'], c['W'], generator=g)
    if family == 'ties':
        x = (x * 2).round() / 2
    elif family == 'constant':
        x = torch.full_like(x, 0.75)
    elif family == 'negative':
        x = -x.abs() - 0.125
    OH, OW = pool_out(c['H'], c['k'], c['s'], c['p']), pool_out(c['W'], c['k'], c['s'], c['p'])
    dy = torch.randint(-4095, 4096, (c['NC'], OH, OW), generator=g).float() / 1024
    return x, dy


AVGPOOL_CASES = [(G, S) for S in (1, 4, 63, 64, 65, 200) for G in (1, 5)]
SOFTMAX_CASES = [(rows, cols, p) for cols in (1, 63, 64, 65, 512, 513, 1088) for rows in (1, 5) for p in (0.0, 0.1, 0.5)]
SOFTMAX_SEED = 0x5EED1234
TOKEN_CASES = [(C_, L, emb) for C_ in (1, 31, 33, 40) for L in (1, 32, 33, 35) for emb in (True, False)]       # N = 3
GRU_CASES = [(B, H, fam) for B in (1, 3) for H in (4, 96) for fam in ('randn', 'saturated')]
SAMPLE_CASES = [(B, S, fam) for B in (1, 3) for S in (4, 40) for fam in ('randn', 'saturated')]
SAMPLE_ABSENT = (None, 'eps', 'dmu', 'dsigma', 'dsample')
BILINEAR_CASES = [((60, 96), (16, 42)), ((8, 8), (8, 8)), ((5, 7), (1, 3)), ((3, 4), (12, 16)), ((1, 1), (4, 4))]      # NC = 3
NEAREST_CASES = [((12,), (5,)), ((7, 12), (3, 5)), ((200,), (192,)), ((3, 7, 12), (2, 3, 5)), ((4, 5), (8, 10))]      # NC = 2


# ================================================================================================== upsample: float64
def up2_matrix(n, dtype=torch.float64):
    """(2n, n): row o holds the weights with which output o reads the inputs (align_corners=False, scale 2)"""
    U = torch.zeros(2 * n, n, dtype=dtype)
    for o in range(2 * n):
        src = max(0.5 * (o + 0.5) - 0.5, 0.0)
        i0 = int(src)
        i1 = i0 + (1 if i0 < n - 1 else 0)
        U[o, i0] += 1.0 - (src - i0)
        U[o, i1] += src - i0
    return U


def up_apply(x, D, H, W, transpose=False, square=False):
    mats = [up2_matrix(n) for n in (D, H, W)]
    if square:
        mats = [m * m for m in mats]
    if transpose:
        return torch.einsum('ad,bh,cw,nabc->ndhw', *mats, x)
    return torch.einsum('ad,bh,cw,ndhw->nabc', *mats, x)


def ref_up_fwd(x):
    """(reference, denominator) of the trilinear x2 upsample of x (NC, D, H, W)"""
    x = _d(x)
    D, H, W = x.shape[1:]
    return up_apply(x, D, H, W), up_apply(x * x, D, H, W, square=True).sqrt()


def ref_up_bwd(g):
    """(reference, denominator) of the adjoint applied to g (NC, 2D, 2H, 2W)"""
    g = _d(g)
    D, H, W = (v // 2 for v in g.shape[1:])
    return up_apply(g, D, H, W, transpose=True), up_apply(g * g, D, H, W, transpose=True, square=True).sqrt()


# ================================================================================================== upsample: emulations
def _lin_src(n):
    """lin_src of the kernels for all outputs of an axis: (i0, i1, w1) as (long, long, float32) tensors"""
    o = torch.arange(2 * n, dtype=torch.float32)
    src = (0.5 * (o + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.long()
    i1 = i0 + (i0 < n - 1).long()
    return i0, i1, src - i0.float()


def _block_src(n):
    """the 2 x 2 block form of the row kernel: output o = 2 p - 1 + a reads the clamped inputs (p - 1, p) with (0.75, 0.25) / (0.25, 0.75)"""
    o = torch.arange(2 * n)
    p = (o + 1) // 2
    a = o - (2 * p - 1)
    i0, i1 = (p - 1).clamp_min(0), p.clamp_max(n - 1)
    w0 = torch.where(a == 1, f32(0.25), f32(0.75))
    return i0, i1, w0, 1.0 - w0


def _col_blend(c, fault=None):
    """output columns from the (d, h)-blended input columns c (..., W): 2 i = 0.25 left + 0.75 own, 2 i + 1 = 0.75 own + 0.25 right,
    both neighbours clamped.  fault 'same_lane': at the float4 boundary i = 4 the left neighbour is the lane's own last column."""
    W = c.shape[-1]
    left = torch.cat([c[..., :1], c[..., :-1]], -1)
    right = torch.cat([c[..., 1:], c[..., -1:]], -1)
    if fault == 'same_lane':
        assert W >= 8
        left = left.clone()
        left[..., 4] = c[..., 7]
    q, t = f32(0.25), f32(0.75)
    out = torch.empty(*c.shape[:-1], 2 * W)
    out[..., 0::2] = q * left + t * c
    out[..., 1::2] = t * c + q * right
    return out


def emu_up_fwd(kind, x, fault=None):
    """float32 emulation of the forward kernel `kind` ('scalar', 'vec', 'row') on x (NC, D, H, W)"""
    assert x.dtype == torch.float32
    NC, D, H, W = x.shape

    def rows(di, hi):
        return x[:, di][:, :, hi]                            # (NC, 2D, 2H, W)
    if kind in ('scalar', 'vec'):
        d0, d1, fd = _lin_src(D)
        h0, h1, fh = _lin_src(H)
        w0, w1, fw = _lin_src(W)
        if kind == 'vec':                                    # the slots of a lane: clamp(2 j - 1 + s); output 4 j + e reads slots (e + 1) / 2, + 1
            assert W % 2 == 0
            ow = torch.arange(2 * W)
            j, e = ow // 4, ow % 4
            s0 = (e + 1) // 2
            w0 = (2 * j - 1 + s0).clamp(0, W - 1)
            w1 = (2 * j - 1 + s0 + 1).clamp(0, W - 1)
        a, b, c = (1 - fd).view(1, -1, 1, 1), (1 - fh).view(1, 1, -1, 1), (1 - fw).view(1, 1, 1, -1)
        fd, fh, fw = fd.view(1, -1, 1, 1), fh.view(1, 1, -1, 1), fw.view(1, 1, 1, -1)
        r00, r01, r10, r11 = rows(d0, h0), rows(d0, h1), rows(d1, h0), rows(d1, h1)

        def lerp_w(r):
            return c * r[..., w0] + fw * r[..., w1]
        return a * (b * lerp_w(r00) + fh * lerp_w(r01)) + fd * (b * lerp_w(r10) + fh * lerp_w(r11))
    assert kind == 'row'
    d0, d1, wd0, wd1 = _block_src(D)
    h0, h1, wh0, wh1 = _block_src(H)
    wd0, wd1 = wd0.view(1, -1, 1, 1), wd1.view(1, -1, 1, 1)
    wh0, wh1 = wh0.view(1, 1, -1, 1), wh1.view(1, 1, -1, 1)
    w00, w01, w10, w11 = wd0 * wh0, wd0 * wh1, wd1 * wh0, wd1 * wh1
    c = ((w00 * rows(d0, h0) + w01 * rows(d0, h1)) + w10 * rows(d1, h0)) + w11 * rows(d1, h1)
    return _col_blend(c, fault)


def _bwd_w(n, fault_last=False):
    """up2_bwd_weights for all inputs i of an axis: (4, n) float32, weight of output 2 i - 1 + k for input i (0: no such output)"""
    i = torch.arange(n)
    lo, hi = i > 0, i < n - 1
    last = f32(0.75) if fault_last else f32(1.0)
    return torch.stack([torch.where(lo, f32(0.25), f32(0.0)), torch.where(lo, f32(0.75), f32(1.0)),
                        torch.where(hi, f32(0.75), last), torch.where(hi, f32(0.25), f32(0.0))])


def _col_reduce(G, W, fault=None):
    """the column form of the vectorised adjoints: coarse column w = (0.25 g[2w-1] + w1 g[2w]) + (w2 g[2w+1] + 0.25 g[2w+2]) with
    g = 0 outside the row.  faults: 'last_col' (w2 = 0.75 at w = W - 1); 'same_lane' (row kernel: the left neighbour of coarse
    column 4, fine column 7, taken from the lane's own last element, fine column 11)"""
    g0, g1 = G[..., 0::2], G[..., 1::2]
    z = torch.zeros_like(g0[..., :1])
    gm1 = torch.cat([z, g1[..., :-1]], -1)
    g2 = torch.cat([g0[..., 1:], z], -1)
    if fault == 'same_lane':
        assert W >= 8
        gm1 = gm1.clone()
        gm1[..., 4] = G[..., 11]
    w1 = torch.where(torch.arange(W) > 0, f32(0.75), f32(1.0))
    w2 = torch.where(torch.arange(W) < W - 1, f32(0.75), f32(0.75) if fault == 'last_col' else f32(1.0))
    return (f32(0.25) * gm1 + w1 * g0) + (w2 * g1 + f32(0.25) * g2)


def _take(G, dim, k, n):
    """G indexed along `dim` at 2 i - 1 + k for i in range(n), clamped (the weight of a clamped index is 0)"""
    idx = (2 * torch.arange(n) - 1 + k).clamp(0, 2 * n - 1)
    return G.index_select(dim, idx)


def emu_up_bwd(kind, g, dseg=None, fault=None):
    """float32 emulation of the backward kernel `kind` ('scalar', 'vec', 'row') on g (NC, 2D, 2H, 2W).
    faults: 'last_col' / 'last_row' / 'last_plane' (weight 0.75 instead of 1 at the last index), 'same_lane', and for the walking
    row kernel 'no_lead_in' (every d segment but the first starts with its two lead-in planes at zero)"""
    assert g.dtype == torch.float32
    NC, D, H, W = g.shape[0], g.shape[1] // 2, g.shape[2] // 2, g.shape[3] // 2
    wa, wb = _bwd_w(D, fault == 'last_plane'), _bwd_w(H, fault == 'last_row')
    if kind == 'scalar':
        wc = _bwd_w(W, fault == 'last_col')
        acc = torch.zeros(NC, D, H, W)
        for ia in range(4):
            Ga = _take(g, 1, ia, D)
            for ib in range(4):
                Gab = _take(Ga, 2, ib, H)
                row = torch.zeros(NC, D, H, W)
                for ic in range(4):
                    row = row + wc[ic] * _take(Gab, 3, ic, W)
                acc = acc + (wa[ia].view(1, -1, 1, 1) * wb[ib].view(1, 1, -1, 1)) * row
        return acc
    cf = fault if fault in ('last_col', 'same_lane') else None
    if kind == 'vec':
        acc = torch.zeros(NC, D, H, W)
        for ia in range(4):
            Ga = _take(g, 1, ia, D)
            for ib in range(4):
                col = _col_reduce(_take(Ga, 2, ib, H), W, cf)
                acc = acc + (wa[ia].view(1, -1, 1, 1) * wb[ib].view(1, 1, -1, 1)) * col
        return acc
    assert kind == 'row'
    P = torch.zeros(NC, 2 * D, H, W)                          # plane contributions: sum over the four fine rows, in row order
    for ib in range(4):
        P = P + wb[ib].view(1, 1, -1, 1) * _col_reduce(_take(g, 2, ib, H), W, cf)
    Pk = [_take(P, 1, k, D) for k in range(4)]
    if fault == 'no_lead_in':
        assert dseg and dseg < D
        starts = torch.arange(D) % dseg == 0
        starts[0] = False
        m = (~starts).float().view(1, -1, 1, 1)
        Pk[0], Pk[1] = Pk[0] * m, Pk[1] * m
    w = [wa[k].view(1, -1, 1, 1) for k in range(4)]
    return (w[0] * Pk[0] + w[1] * Pk[1]) + (w[2] * Pk[2] + w[3] * Pk[3])


def up_owner(kind, backward, c, index, plan):
    """who computes element `index` = (nc, d, h, w) of the result of an upsample case: text for a failure message"""
    nc, d, h, w = index
    D, H, W = c['D'], c['H'], c['W']
    n = (D, H, W) if backward else (2 * D, 2 * H, 2 * W)
    border = [ax for ax, v, m in zip('dhw', (d, h, w), n) if v in (0, m - 1)]
    s = f'element (nc {nc}, d {d}, h {h}, w {w}) kernel {kind}'
    if not backward and kind == 'row':
        idx = ((h + 1) // 2) * (W // 2) + w // 4
        s += f': workgroup ({idx // 256}, {(d + 1) // 2}, {nc}) lane {idx % 256}'
    elif kind == 'vec':
        idx = h * (W // 4 if backward else W // 2) + w // 4
        s += f': workgroup ({idx // 256}, {d}, {nc}) lane {idx % 256}'
    elif backward and kind == 'row':
        per = 256 // (W // 2)
        s += f': workgroup ({h // per}, {d // plan["dseg"]}, {nc}) lane {(h % per) * (W // 2) + w // 2}'
    else:
        flat = ((nc * n[0] + d) * n[1] + h) * n[2] + w
        s += f': grid-stride element {flat}, first pass workgroup {(flat // 256) % plan["grid"][0]} lane {flat % 256}'
    if backward and kind == 'row' and plan['segs'] > 1:
        s += f'; d segment {d // plan["dseg"]} of {plan["segs"]}' + (' (first plane of its segment)' if d % plan['dseg'] == 0 and d else '')
    return s + ('; border in ' + ''.join(border) if border else '; interior')


# ================================================================================================== max pooling
def ref_maxpool(x, k, s, p, last_wins=False, pad_value=-math.inf):
    """(y, winner byte a * k + b) of max pooling x (NC, H, W): the first maximum of a window wins (row-major scan), padding never
    wins.  Planted faults: last_wins (>= instead of >), pad_value 0 (the padding takes part as a zero)"""
    NC, H, W = x.shape
    OH, OW = pool_out(H, k, s, p), pool_out(W, k, s, p)
    xp = torch.full((NC, H + 2 * p + s, W + 2 * p + s), -math.inf, dtype=x.dtype)
    live = torch.zeros(H + 2 * p + s, W + 2 * p + s, dtype=torch.bool)
    xp[:, p:p + H, p:p + W] = x
    live[p:p + H, p:p + W] = True
    best = torch.full((NC, OH, OW), -math.inf, dtype=x.dtype)
    code = torch.full((NC, OH, OW), -1, dtype=torch.long)
    for a in range(k):
        for b in range(k):
            v = xp[:, a:a + s * OH:s, b:b + s * OW:s]
            ok = live[a:a + s * OH:s, b:b + s * OW:s].unsqueeze(0)
            if pad_value != -math.inf:
                v = torch.where(ok, v, torch.full_like(v, pad_value))
                ok = torch.ones_like(ok)
            better = ok & ((v >= best if last_wins else v > best) | (code < 0))
            best = torch.where(better, v, best)
            code = torch.where(better, torch.full_like(code, a * k + b), code)
    return best, code.to(torch.uint8)


def ref_maxpool_bwd(dy, code, H, W, k, s, p, drop_fifth=False):
    """dx (NC, H, W): every window's gradient goes to its winner (float64 sums; exact for the dyadic gradients of the cases).
    Planted fault drop_fifth: the eight-column kernel without the fifth window of a lane (window 4 l + 4 into column 8 l + 7)"""
    NC, OH, OW = dy.shape
    dx = torch.zeros(NC, H + 2 * p + s, W + 2 * p + s, dtype=torch.float64)
    oh, ow = torch.meshgrid(torch.arange(OH), torch.arange(OW), indexing='ij')
    a, b = (code.long() // k), (code.long() % k)
    hh, ww = oh * s + a, ow * s + b                      # padded coordinates
    val = dy.double()
    if drop_fifth:
        fifth = (ow % 4 == 0) & (ow >= 4) & (b == 0)
        val = torch.where(fifth, torch.zeros_like(val), val)
    nc = torch.arange(NC).view(-1, 1, 1).expand_as(hh)
    dx.index_put_((nc, hh, ww), val, accumulate=True)
    return dx[:, p:p + H, p:p + W].contiguous()


# ================================================================================================== average pooling
def ref_avgpool(x):
    """x (G, S) -> (mean, denominator)"""
    x = _d(x)
    S = x.shape[1]
    return x.mean(1), (x * x).sum(1).sqrt() / S


def wave_sum32(v):
    """the xor butterfly of wave_sum over the last axis (64 lanes), lane 0's value"""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def lane_sums32(x, cols):
    """per lane the serial sum over c = lane, lane + 64, ... of x (rows, cols): (rows, 64) float32"""
    pad = _cdiv(cols, 64) * 64 - cols
    xp = torch.cat([x, torch.zeros(x.shape[0], pad)], 1).view(x.shape[0], -1, 64)
    s = torch.zeros(x.shape[0], 64)
    for kk in range(xp.shape[1]):
        s = s + xp[:, kk]
    return s


def emu_avgpool(x):
    assert x.dtype == torch.float32
    return wave_sum32(lane_sums32(x, x.shape[1])) / f32(float(x.shape[1]))


def emu_avgpool_bwd(dy, S):
    """bit-exact float32 form: dy * (1 / S)"""
    return (dy * (f32(1.0) / f32(float(S)))).view(-1, 1).expand(-1, S).contiguous()


# ================================================================================================== softmax + dropout
def softmax_inputs(rows, cols, p):
    """(S, dPd): randn * 3 scores; the last row is the spiked one: +80 next to -80.  e^80 = 5.5e34 is still a finite float32, so
    a kernel without the max subtraction would pass that row: with five rows the one before it carries +100 next to -100, where
    e^100 is not."""
    g = _gen('softmax', rows, cols, p)
    S = torch.randn(rows, cols, generator=g) * 3
    if cols >= 2:
        S[-1, cols // 2], S[-1, cols // 2 - 1] = 80.0, -80.0
        if rows >= 5:
            S[-2, cols // 2], S[-2, cols // 2 - 1] = 100.0, -100.0
    return S, torch.randn(rows, cols, generator=g)


def ref_softmax(S, dPd, mask):
    """float64 {P, Pd, dS} with their denominators.  mask: the dropout factor per element (0 or 1 / (1 - p); ones for p = 0)"""
    S, dPd, mask = _d(S), _d(dPd), _d(mask)
    P = torch.softmax(S, dim=1)
    g = dPd * mask
    dot = (P * g).sum(1, keepdim=True)
    dS = P * (g - dot)
    den_dS = P * (g * g + (P * g).pow(2).sum(1, keepdim=True)).sqrt() + TINY
    return {'P': (P, P + TINY), 'Pd': (P * mask, P * mask + TINY), 'dS': (dS, den_dS)}


def emu_softmax(S, dPd, mask, no_max=False):
    """the kernels' sequence in float32 with the host's expf: {P, Pd, dS}.  Planted fault no_max: no max subtraction"""
    assert S.dtype == torch.float32
    cols = S.shape[1]
    mx = torch.zeros(S.shape[0], 1) if no_max else S.max(1, keepdim=True).values
    v = torch.exp(S - mx)
    inv = f32(1.0) / wave_sum32(lane_sums32(v, cols))
    P = v * inv.view(-1, 1)
    g = dPd * mask
    dot = wave_sum32(lane_sums32(P * g, cols)).view(-1, 1)
    return {'P': P, 'Pd': P * mask, 'dS': P * (g - dot)}


def host_dropout_mask(rows, cols, p, seed, index_cols=None):
    """dropout_scale of common.h for element row * index_cols + c (index_cols = cols; another value: the planted fault of a mask
    indexed with another row length).  Pure Python integers; used by the CPU test only - the GPU test takes the library's mask."""
    index_cols = index_cols or cols
    if p <= 0:
        return torch.ones(rows, cols)
    M = (1 << 64) - 1
    out = torch.empty(rows, cols)
    keep = f32(1.0) / (f32(1.0) - f32(p))
    for r in range(rows):
        for c in range(cols):
            z = (seed + (r * index_cols + c) * 0x9E3779B97F4A7C15) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            u = f32(float((z >> 32) >> 8)) * f32(1.0 / 16777216.0)
            out[r, c] = 0.0 if float(u) < float(f32(p)) else keep
    return out


# ================================================================================================== tokens
def ref_tokens(x, pos, temb, tok, l0):
    """tokens[(l0 + l)][n][c] = (x[n][c][l] + pos[c][l]) + temb[c] written into a copy of `tok` (float32, bit-exact order)"""
    N, C_, L = x.shape
    v = x
    if pos is not None:
        v = v + pos.view(1, C_, L)
    if temb is not None:
        v = v + temb.view(1, C_, 1)
    out = tok.clone()
    out[l0:l0 + L] = v.permute(2, 0, 1)
    return out


def ref_untoken(tok, N, C_, L, l0):
    return tok[l0:l0 + L].permute(1, 2, 0).contiguous()


# ================================================================================================== GRU / RSSM sample
def _sig32(x):
    return f32(1.0) / (f32(1.0) + torch.exp(-x))


def gru_inputs(B, H, fam):
    g = _gen('gru', B, H, fam)
    gi, gh = torch.randn(B, 3 * H, generator=g), torch.randn(B, 3 * H, generator=g)
    if fam == 'saturated':                                   # pre-activations of +-30: gates at 0 / 1, tanh at +-1
        sign = torch.where(torch.rand(B, 3 * H, generator=g) < 0.5, -1.0, 1.0)
        gi = gi * 0.01 + 30.0 * sign
        gh = gh * 0.01
    return gi, gh, torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)


def gru_eval(gi, gh, h, dhn, dtype, drop_r=False):
    """the cell in PyTorch's gate order (r, z, n) and its backward, in `dtype` with the kernel's sequence of operations.
    Planted fault drop_r: dgh_n = dpre_n instead of dpre_n * r"""
    gi, gh, h, dhn = (t.to(dtype) for t in (gi, gh, h, dhn))
    H = h.shape[1]
    sig = _sig32 if dtype == torch.float32 else torch.sigmoid
    r = sig(gi[:, :H] + gh[:, :H])
    z = sig(gi[:, H:2 * H] + gh[:, H:2 * H])
    ghn = gh[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * ghn)
    hn = (1 - z) * n + z * h
    dn, dz = dhn * (1 - z), dhn * (h - n)
    dpre_n = dn * (1 - n * n)
    dpre_r = dpre_n * ghn * r * (1 - r)
    dpre_z = dz * z * (1 - z)
    dgi = torch.cat([dpre_r, dpre_z, dpre_n], 1)
    dgh = torch.cat([dpre_r, dpre_z, dpre_n if drop_r else dpre_n * r], 1)
    return {'hn': hn, 'dgi': dgi, 'dgh': dgh, 'dh': dhn * z,
            'den_hn': (((1 - z) * n).pow(2) + (z * h).pow(2)).sqrt() + TINY, 'ghn': ghn}


def gru_dens(gi, gh, h, dhn):
    """denominators: hn by its two terms; every gradient by |dhn| (1 + |h| + |gh_n|), which bounds the cell's partial derivatives"""
    e = gru_eval(gi, gh, h, dhn, torch.float64)
    dg = _d(dhn).abs() * (1 + _d(h).abs() + e['ghn'].abs()) + TINY
    return {'hn': e['den_hn'], 'dgi': dg.repeat(1, 3), 'dgh': dg.repeat(1, 3), 'dh': dg}


def sample_inputs(B, S, fam, eps_pad=3):
    g = _gen('sample', B, S, fam)
    mls = torch.randn(B, 2 * S, generator=g)
    if fam == 'saturated':
        mls[:, S:] = mls[:, S:] * 0.01 + 60.0 * torch.where(torch.rand(B, S, generator=g) < 0.5, -1.0, 1.0)     # ls / 2 = +-30
    eps_store = torch.randn(B, S + eps_pad, generator=g)     # leading dimension S + eps_pad
    return mls, eps_store, [torch.randn(B, S, generator=g) for _ in range(3)]


def sample_eval(mls, eps, dmu, dsigma, dsample, min_std, dtype):
    """sigma = 2 sigmoid(ls / 2) + min_std, sample = mu + sigma eps, and the backward with absent (None) operands as zeros"""
    S = mls.shape[1] // 2
    c = lambda t: None if t is None else t.to(dtype)      # noqa: E731
    mls, eps, dmu, dsigma, dsample = c(mls), c(eps), c(dmu), c(dsigma), c(dsample)
    zero = torch.zeros(mls.shape[0], S, dtype=dtype)
    sig = _sig32 if dtype == torch.float32 else torch.sigmoid
    ms = torch.tensor(min_std, dtype=torch.float32).to(dtype)
    s = sig(mls[:, S:] * 0.5)
    mu, sigma = mls[:, :S], 2 * s + ms
    e = zero if eps is None else eps
    dsm = zero if dsample is None else dsample
    dm = (zero if dmu is None else dmu) + dsm
    dl = ((zero if dsigma is None else dsigma) + dsm * e) * s * (1 - s)
    ds_ = zero if dsigma is None else dsigma
    return {'mu': mu, 'sigma': sigma, 'sample': mu + sigma * e, 'dmls': torch.cat([dm, dl], 1),
            'den_sample': (mu.pow(2) + (sigma * e).pow(2)).sqrt() + TINY,
            'den_dmls': torch.cat([((zero if dmu is None else dmu).pow(2) + dsm.pow(2)).sqrt() + TINY,
                                   (ds_.pow(2) + (dsm * e).pow(2)).sqrt() + TINY], 1)}


# ================================================================================================== small glue operations
def ref_copy2d(src, dst, rows, cols, lds, ldd, accumulate):
    """flat float32 storages; returns the expected dst storage (bit-exact: one add at most)"""
    out = dst.clone()
    s = torch.as_strided(src, (rows, cols), (lds, 1))
    o = torch.as_strided(out, (rows, cols), (ldd, 1))
    o.copy_(o + s if accumulate else s)
    return out


def ref_axpby(a, b, alpha, beta):
    """alpha * a + (beta * b | 0) in float32, the kernel's order (bit-exact)"""
    return f32(alpha) * a + (f32(beta) * b if b is not None else torch.zeros_like(a))


def ref_batchsum(x, prior, accumulate):
    """x (N, inner): serial float32 sum over n from 0, then prior + s when accumulating (bit-exact)"""
    s = torch.zeros(x.shape[1])
    for n in range(x.shape[0]):
        s = s + x[n]
    return prior + s if accumulate else s


def act32(v, act, slope=SLOPE):
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * f32(slope))
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return _sig32(v)
    return v


def act64(v, act, slope=SLOPE):
    v = _d(v)
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * float(f32(slope)))
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


ACT_EXACT = (ACT_NONE, ACT_RELU, ACT_LEAKY)          # no transcendental: compared bit for bit with act32


def act_inputs():
    g = _gen('act_fwd')
    return torch.cat([torch.randn(500, generator=g) * 3, torch.tensor([0.0, -0.0, 1e-8, -1e-8, 30.0, -30.0])])


def ref_act(v, act):
    """(reference, denominator): relative to the result, floored for ELU / tanh near zero by the argument's own rounding"""
    r = act64(v, act)
    return r, r.abs() + _d(v).abs() * U32 + TINY


# ================================================================================================== resizes
def _bilinear_axis(n_in, n_out, dtype):
    """(n_out, n_in) weights of bilinear, align_corners=False; float32: with the kernel's float32 coordinates"""
    M = torch.zeros(n_out, n_in, dtype=dtype)
    if dtype == torch.float32:
        sc = f32(float(n_in)) / f32(float(n_out))
        o = torch.arange(n_out, dtype=torch.float32)
        f = (sc * (o + 0.5) - 0.5).clamp_min(0.0)
        i0 = f.long()
        i1 = i0 + (i0 < n_in - 1).long()
        l1 = f - i0.float()
        return i0, i1, 1.0 - l1, l1
    for o in range(n_out):
        f = max(n_in / n_out * (o + 0.5) - 0.5, 0.0)
        i0 = int(f)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        M[o, i0] += 1.0 - (f - i0)
        M[o, i1] += f - i0
    return M


def ref_bilinear(x, oh, ow):
    """(reference, denominator) of the bilinear resize of x (NC, H, W) to (oh, ow)"""
    x = _d(x)
    My, Mx = _bilinear_axis(x.shape[1], oh, torch.float64), _bilinear_axis(x.shape[2], ow, torch.float64)
    return torch.einsum('ah,bw,nhw->nab', My, Mx, x), torch.einsum('ah,bw,nhw->nab', My * My, Mx * Mx, x * x).sqrt() + TINY


def ref_bilinear_bwd(g, h, w):
    """(reference, denominator) of the adjoint: g (NC, oh, ow) -> (NC, h, w)"""
    g = _d(g)
    My, Mx = _bilinear_axis(h, g.shape[1], torch.float64), _bilinear_axis(w, g.shape[2], torch.float64)
    return torch.einsum('ah,bw,nab->nhw', My, Mx, g), torch.einsum('ah,bw,nab->nhw', My * My, Mx * Mx, g * g).sqrt() + TINY


def emu_bilinear(x, oh, ow):
    assert x.dtype == torch.float32
    y0, y1, hy, ly = _bilinear_axis(x.shape[1], oh, torch.float32)
    x0, x1, hx, lx = _bilinear_axis(x.shape[2], ow, torch.float32)
    r0, r1 = x[:, y0], x[:, y1]
    hy, ly = hy.view(1, -1, 1), ly.view(1, -1, 1)
    return hy * (hx * r0[..., x0] + lx * r0[..., x1]) + ly * (hx * r1[..., x0] + lx * r1[..., x1])


def emu_bilinear_bwd(g, h, w):
    """the gather of bev.hip: per input pixel, rows of outputs in ascending order, row = sum_ox wx g, acc += wy row (outputs that
    do not read the pixel have weight 0 or lie outside the kernel's index window: an exact 0 either way)"""
    assert g.dtype == torch.float32
    NC, oh, ow = g.shape

    def wmat(n_in, n_out):
        i0, i1, w0, w1 = _bilinear_axis(n_in, n_out, torch.float32)
        i = torch.arange(n_in).view(1, -1)
        z = torch.zeros(n_out, n_in)
        return torch.where(i0.view(-1, 1) == i, w0.view(-1, 1), z) + torch.where(i1.view(-1, 1) == i, w1.view(-1, 1), z)
    Wy, Wx = wmat(h, oh), wmat(w, ow)
    row = torch.zeros(NC, oh, w)
    for ox in range(ow):
        row = row + Wx[ox].view(1, 1, -1) * g[:, :, ox:ox + 1]
    acc = torch.zeros(NC, h, w)
    for oy in range(oh):
        acc = acc + Wy[oy].view(1, -1, 1) * row[:, oy:oy + 1]
    return acc


def ref_nearest(x, out_sz):
    """F.interpolate(mode='nearest') on the CPU over the trailing len(out_sz) axes of x (NC, ...); float32 or uint8, exact"""
    xf = x.float().unsqueeze(0)
    return F.interpolate(xf, size=tuple(out_sz), mode='nearest')[0].to(x.dtype)


# ================================================================================================== bar tables: recomputation
def _worst(stats_list):
    return (max(s['rms'] for s in stats_list), max(s['max_e'] for s in stats_list))


@functools.lru_cache(maxsize=None)
def compute_own_worst():
    """worst (rms, max e) of every summing kernel's emulation over its case list: the source of OWN_WORST"""
    out = {}
    for backward, cases in ((0, UP_FWD_CASES), (1, UP_BWD_CASES)):
        per = {}
        for c in cases:
            v = up_inputs(c, backward)
            if backward:
                st = error_stats(emu_up_bwd(c['kernel'], v), *ref_up_bwd(v))
            else:
                st = error_stats(emu_up_fwd(c['kernel'], v), *ref_up_fwd(v))
            per.setdefault(c['kernel'], []).append(st)
        for k, sts in per.items():
            out[f'up_{"bwd" if backward else "fwd"}_{k}'] = _worst(sts)
    sts = []
    for G, S in AVGPOOL_CASES:
        x = torch.randn(G, S, generator=_gen('avgpool', G, S))
        sts.append(error_stats(emu_avgpool(x), *ref_avgpool(x)))
    out['avgpool_fwd'] = _worst(sts)
    f, b = [], []
    for (h, w), (oh, ow) in BILINEAR_CASES:
        x, g = bilinear_inputs(h, w, oh, ow)
        f.append(error_stats(emu_bilinear(x, oh, ow), *ref_bilinear(x, oh, ow)))
        b.append(error_stats(emu_bilinear_bwd(g, h, w), *ref_bilinear_bwd(g, h, w)))
    out['resize_bilinear'], out['resize_bilinear_bwd'] = _worst(f), _worst(b)
    return out


def bilinear_inputs(h, w, oh, ow, NC=3):
    g = _gen('bilinear', h, w, oh, ow)
    return torch.randn(NC, h, w, generator=g), torch.randn(NC, oh, ow, generator=g)


@functools.lru_cache(maxsize=None)
def compute_trans_worst():
    """worst (rms, max e) of the plain float32 CPU evaluation of every kernel with transcendentals: the source of TRANS_WORST"""
    out = {}
    per = {'P': [], 'Pd': [], 'dS': []}
    for rows, cols, p in SOFTMAX_CASES:
        S, dPd = softmax_inputs(rows, cols, p)
        mask = host_dropout_mask(rows, cols, p, SOFTMAX_SEED)
        ref, emu = ref_softmax(S, dPd, mask), emu_softmax(S, dPd, mask)
        for k in per:
            per[k].append(norm_stats(emu[k], *ref[k]))
    for k, sts in per.items():
        out[f'softmax_{k}'] = _worst(sts)
    fw, bw = [], []
    for B, H, fam in GRU_CASES:
        args = gru_inputs(B, H, fam)
        e32, e64, den = gru_eval(*args, torch.float32), gru_eval(*args, torch.float64), gru_dens(*args)
        fw.append(norm_stats(e32['hn'], e64['hn'], den['hn']))
        bw += [norm_stats(e32[k], e64[k], den[k]) for k in ('dgi', 'dgh', 'dh')]
    out['gru_fwd'], out['gru_bwd'] = _worst(fw), _worst(bw)
    fw, bw = [], []
    for B, S, fam in SAMPLE_CASES:
        mls, eps_store, (dmu, dsigma, dsample) = sample_inputs(B, S, fam)
        for absent in SAMPLE_ABSENT:
            kw = sample_args(eps_store[:, :S], dmu, dsigma, dsample, absent)
            e32, e64 = sample_eval(mls, min_std=0.1, dtype=torch.float32, **kw), sample_eval(mls, min_std=0.1, dtype=torch.float64, **kw)
            fw += [norm_stats(e32['sigma'], e64['sigma'], e64['sigma']), norm_stats(e32['sample'], e64['sample'], e64['den_sample'])]
            bw.append(norm_stats(e32['dmls'], e64['dmls'], e64['den_dmls']))
    out['sample_fwd'], out['sample_bwd'] = _worst(fw), _worst(bw)
    v = act_inputs()
    out['act_fwd'] = _worst([norm_stats(act32(v, a), *ref_act(v, a)) for a in (ACT_ELU, ACT_TANH, ACT_SIGMOID)])
    return out


def sample_args(eps, dmu, dsigma, dsample, absent):
    kw = {'eps': eps, 'dmu': dmu, 'dsigma': dsigma, 'dsample': dsample}
    if absent:
        kw[absent] = None
    return kw
