"""Plain float64 references, CPU emulations of each kernel's summation order, planted faults, the case lists and a restatement
of the host dispatch for the dense GEMM unit (muvo_amd/csrc/gemm.hip: the tiled fp32 MFMA kernel, the three skinny kernels and
the grouped Linear; muvo_colsum_acc / muvo_act_bwd of elementwise.hip, which every Linear backward runs next to them).
Helpers only: no fixtures, no tests.  tests/test_gemm_reference.py (CPU) and tests/test_gemm_kernels_gpu.py (GPU) share
everything here, so the bars the GPU test applies are the ones the CPU test proves to pass the emulated arithmetic and to reject
the planted faults.  The metric is that of tests/vox_reference.py (error_stats: e = |got - ref64| / den per element, next to
rms(got - ref) / rms(ref)), the fp32 bar that of tests/conv_reference.py (f32_bar).

References.  ref_gemm evaluates the formula at the top of gemm.hip in float64 straight from storage, strides, batch strides
and offsets:  C[b1][b2][m][n] = act(alpha * sum_k A(m,k) B(k,n) + bias[n / bias_div]);  mode 1: prior C + alpha * sum.
The denominator is sqrt(alpha^2 sum a^2 b^2 + bias^2 [+ prior C^2]): the scale of the rounding error of that one element
before the activation.  ReLU / LeakyReLU / ELU / tanh have |derivative| <= 1 and act(0) = 0, so that scale bounds the error
after them; the sigmoid's output is rounded at the scale of 0.5 whatever its argument (0.25 u), so sigmoid cases keep their
pre-activation scale at >= 0.2 and K >= 16 (checked by the CPU test): 1.25 u against bars of >= 8 u.  tanh / sigmoid cases
scale B by 1 / sqrt(K), which keeps the pre-activations of size 1: a saturated output would hide any error.

Emulations (float32 on the CPU, every product and every sum rounded once: the library is built with -ffp-contract=off).
  'tiled'           the serial chain of v_mfma_f32_32x32x2_f32 steps, two products per step, one chain per K range of a split-K
                    launch (conv_reference.emulate_gemm 'f32_chain'); ranges are added to C in index order
  'skinny_kcontig'  64 lanes stride over k, then the xor butterfly of wave_sum (a balanced tree)
  'skinny_kvec'     per lane a float4 dot over k and k + 2048 per pass of 4096, eight waves split k; the LDS transpose sums
                    (four interleaved serial sums over 64 lanes, then a pair tree), then the eight waves in order
  'skinny_ncontig'  per wave 32 k of every 128-chunk in groups of four ((p0 + p1) + (p2 + p3)), the four waves in order, the KS
                    ranges added in index order
and the same for the grouped Linear's forward (the k-vector scheme), data gradient (the n-contiguous scheme over 128-row slabs),
weight / bias gradient (serial over the rows) and the column sums.  Where float atomics decide the order on the GPU the
emulation takes index order; any other order is another sample of the same error distribution.

Dispatch mirror.  gemm_plan / grouped_plan restate muvo_gemm_route / muvo_grouped_linear_route for default tuning variables
(MUVO_GEMM_KSPLIT_BLOCKS 768, MUVO_GEMM_KSPLIT_MINTILES 8, MUVO_SKINNY_KS_BLOCKS 512), both deterministic modes."""
import collections
import functools
import math
import types

import torch

import conv_reference as CR
from conv_reference import f32_bar
from vox_reference import error_stats, excess, within  # noqa: F401

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_ELU, ACT_TANH, ACT_SIGMOID = range(6)
ACT_NAMES = ('none', 'relu', 'leaky', 'elu', 'tanh', 'sigmoid')
ALL_ACTS = tuple(range(6))
SLOPE = 0.2
MARKER = -12345.678          # canary value of every C element a kernel must not write (compared bit for bit)

# Bars, all in the form (rms, max e) = (c_rms, c_e) * u * sqrt(K), u = 2^-24, K = the reduction length (at least 1).
#   Tiled kernel, k-vector and n-contiguous skinny kernels: conv_reference.f32_bar(K) = (0.46, 4.8), 2 x the f32_chain
#     emulation of the MFMA chain (derived there).  tests/test_gemm_reference.py asserts that the emulations of the two VALU
#     kernels stay within HALF of it at every case below (0.41 of it at most), so they need no bar of their own.
#   Every other VALU kernel's emulation does NOT stay within half of f32_bar's rms somewhere on the case lists: bias, alpha, the
#     activation and the prior gradient add roundings to a short sum, every product is rounded, and a reduction of 1 ... 24
#     rows has none of the averaging a long chain has.  Each of them gets its own bar, derived the same way: 2 x the worst rms
#     and 2 x the worst max e of ITS OWN emulation over its case list, in units of u sqrt(K) (OWN_WORST; margin 2).  The CPU
#     test recomputes OWN_WORST from the emulations and fails when the table is stale.
#   muvo_act_bwd: no sum at all, so no sqrt(K) law: (rms, max e) = 2 x the worst of its float32 emulation over the six
#     activations on 4099 randn elements (ACT_BWD_WORST: tanh, 1 - y * y next to y = +-1), e in units of |dy|.
# None of these numbers comes from a GPU.
OWN_WORST = {          # emulation: worst (rms, max e) / (u sqrt(K)) over the case list
    'skinny_kcontig': (0.253, 1.104),
    'grouped_fwd': (0.259, 0.709), 'grouped_dx': (0.411, 1.406), 'grouped_dw': (0.654, 2.801), 'grouped_db': (0.905, 1.352),
    'colsum': (0.776, 1.266),
}
ACT_BWD_WORST = (4.1e-8, 8.2e-8)
ACT_BWD_BAR = (2 * ACT_BWD_WORST[0], 2 * ACT_BWD_WORST[1])


def kernel_bar(kind, K):
    """(rms, max e) bar of a result of kernel `kind` ('tiled', 'skinny_*', 'grouped_*', 'colsum') over K terms"""
    if kind in OWN_WORST:
        r = math.sqrt(max(K, 1)) * CR.U32
        return (2 * OWN_WORST[kind][0] * r, 2 * OWN_WORST[kind][1] * r)          # margin 2 over the kernel's own emulation
    return f32_bar(K)


# Measured on an MI355X by tests/test_gemm_kernels_gpu.py (GEMMSTAT lines; largest max e / rms over all cases of a kernel and the
# largest share of its bar).  Not the source of any bar: the bars above come from the float64 reference and the CPU emulations.
#   tiled            3.8e-6 / 5.0e-7 (0.93 of its bar: K = 1, one rounded product; the CPU emulation gives the same 0.93)
#   skinny_kvec      5.2e-7 / 1.5e-7 (0.51)        skinny_kcontig   4.3e-7 / 1.3e-7 (0.50)        skinny_ncontig   4.4e-7 / 9.7e-8 (0.41)
#   grouped forward  6.0e-7 / 1.5e-7 (0.54)        dx  4.6e-7 / 8.9e-8 (0.50)       dW  8.2e-7 / 8.8e-8 (0.50)       db  3.9e-7 / 1.6e-7 (0.50)
#   colsum           3.9e-7 / 3.2e-7 (0.50)        act_bwd  8.6e-8 / 4.0e-8 (0.52)  bias_grad_nchw of the seed ConvTranspose  1.0e-7 / 5.3e-8 (0.12)
#   AttentionFn      o 1.5e-7 ... 5.1e-7, dqkv 1.2e-7 ... 4.3e-7: 0.23 ... 0.31 of the bars below
#   (a share of 0.50 is the emulation's own worst case: the kernel rounds exactly as emulated)

# AttentionFn (the unfused path: QK^T, softmax, PV and the five backward products on the tiled kernel) against
# attention_reference.reference64 at p = 0, e = max |got - ref| / max |ref| per tensor.  The bar is built as
# attention_reference builds its own: 4 x the e of the plain float32 CPU evaluation (attention_float32 below) on the same
# inputs; tests/test_gemm_reference.py recomputes these numbers and asserts they still hold.
ATTN_CASES = [(70, 2, 3, 12), (33, 1, 2, 20), (17, 2, 2, 12)]           # (l, n, heads, dh)
ATTN_MEASURED = {
    (70, 2, 3, 12): {'o': 1.55e-07, 'dqkv': 3.79e-07},
    (33, 1, 2, 20): {'o': 5.10e-07, 'dqkv': 4.26e-07},
    (17, 2, 2, 12): {'o': 1.41e-07, 'dqkv': 1.33e-07},
}
ATTN_BARS = {k: {n: 4 * e for n, e in v.items()} for k, v in ATTN_MEASURED.items()}


def _gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _cdiv(a, b):
    return -(-a // b)


# ================================================================================================ activations
def act64(y, act, slope=SLOPE):
    """all six activations of common.h in float64 (vox_reference.act64 stops at ELU)"""
    if act == ACT_RELU:
        return y.clamp_min(0)
    if act == ACT_LEAKY:
        return torch.where(y > 0, y, y * slope)
    if act == ACT_ELU:
        return torch.where(y > 0, y, torch.expm1(y))
    if act == ACT_TANH:
        return torch.tanh(y)
    if act == ACT_SIGMOID:
        return torch.sigmoid(y)
    return y


def act32(v, act, slope=SLOPE):
    """act_apply of common.h in float32, operation by operation"""
    assert v.dtype == torch.float32
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    return v


def act_grad_from_out(y, act, slope=SLOPE):
    """d act / d pre-activation through the OUTPUT y (common.h: act_grad_from_out), in y's dtype"""
    one = torch.ones_like(y)
    if act == ACT_RELU:
        return torch.where(y > 0, one, torch.zeros_like(y))
    if act == ACT_LEAKY:
        return torch.where(y > 0, one, torch.full_like(y, slope))
    if act == ACT_ELU:
        return torch.where(y > 0, one, y + 1)
    if act == ACT_TANH:
        return 1 - y * y
    if act == ACT_SIGMOID:
        return y * (1 - y)
    return one


# ================================================================================================ dispatch mirror
def gemm_plan(M, N, K, sam, sak, sbk, sbn, scm, has_bias=False, act=ACT_NONE, mode=0, nb=1, a_aligned=True, b_aligned=True,
              det=False):
    """What muvo_gemm launches (muvo_gemm_route): dict(kernel, rm, tile, lay, ksplit, grid, block), default tuning variables.
    a_aligned / b_aligned: the operand's first element sits on a 16-byte boundary."""
    vec_ok = (sbk == 1 and sak == 1 and K % 4 == 0 and sam % 4 == 0 and sbn % 4 == 0 and a_aligned and b_aligned)
    skinny = M <= 32 and mode == 0 and nb == 1
    if skinny and ((N >= 64 and K >= 16) or (K >= 64 and vec_ok)):
        if M <= 24 and vec_ok:
            rm = 4 if M <= 4 else 8 if M <= 8 else 16 if M <= 16 else 24
            return dict(kernel='skinny_kvec', rm=rm, tile=(0, 0), lay=(-1, -1), ksplit=1, grid=(_cdiv(N, 4), 1, 1), block=512)
        if sbk == 1:
            return dict(kernel='skinny_kcontig', rm=4 if M <= 4 else 8, tile=(0, 0), lay=(-1, -1), ksplit=1,
                        grid=(_cdiv(N, 8), 1, 1), block=256)
        blocks, ks = _cdiv(N, 64), 1
        if not has_bias and act == ACT_NONE and scm == N:
            ks = min(_cdiv(512, blocks), K // 64)
            if ks < 1 or det:
                ks = 1
        return dict(kernel='skinny_ncontig', rm=4 if M <= 4 else 8 if M <= 8 else 24, tile=(0, 0), lay=(-1, -1), ksplit=ks,
                    grid=(blocks, ks, 1), block=256)
    bm, bn = (32, 128) if M <= 32 else (128, 64) if N <= 64 else (128, 128)
    gx, gy, ksplit = _cdiv(N, bn), _cdiv(M, bm), 1
    if mode == 1:
        ksplit = min(_cdiv(768, gx * gy * nb), _cdiv(_cdiv(K, 16), 8))
        if ksplit < 1 or det:
            ksplit = 1
    al = 0 if (sam == 1 and sak != 1) else (1 if sak == 1 else 0)
    bl = 0 if sbn == 1 else (1 if sbk == 1 else 0)
    return dict(kernel='tiled', rm=0, tile=(bm, bn), lay=(al, bl), ksplit=ksplit, grid=(gx, gy, nb * ksplit), block=256)


def grouped_plan(M, K, ns):
    """muvo_grouped_linear_route: the forward row template and the three grids"""
    return dict(fwd_rm=8 if M <= 8 else 24, fwd_grid=sum(_cdiv(n, 4) for n in ns),
                dgrad_grid=(_cdiv(K, 64), sum(_cdiv(n, 128) for n in ns)), wgrad_grid=(_cdiv(K, 256), sum(_cdiv(n, 16) for n in ns)))


# ================================================================================================ cases
CASE_DEFAULTS = dict(a='k', b='k', sam_pad=0, scm_pad=0, a_off=0, b_off=0, c_off=0, B1=1, B2=1, bias=False, bias_div=1,
                     act=ACT_NONE, slope=SLOPE, alpha=1.0, mode=0, det=False, ident=None, twice=False)


def gcase(name, M, N, K, expect, **kw):
    """One muvo_gemm call.  a: 'k' A stored (M, K) row-major (k-contiguous) | 'm' stored (K, M) (m-contiguous) | 's' no unit stride
    (sak = 2); b: 'k' B stored (N, K) (nn.Linear weight) | 'n' stored (K, N) | 's' (sbk = 2).  sam_pad / scm_pad widen the row
    stride, *_off shift the first element (floats), batches are stored one after the other.  expect: the route fields the case
    exists for.  ident: arithmetic-identifying (bf16x3 arithmetic must fail the bar 4x); default: store mode, no activation, no
    bias, 16 <= K <= 1350.  twice: run two times and compare the bits (deterministic cases)."""
    bad = set(kw) - set(CASE_DEFAULTS)
    assert not bad, bad
    c = dict(CASE_DEFAULTS, name=name, M=M, N=N, K=K, expect=expect, **kw)
    if c['ident'] is None:
        c['ident'] = c['mode'] == 0 and c['act'] == ACT_NONE and not c['bias'] and 16 <= K <= 1350
    return c


def strides(c):
    """storage geometry of a case: dict(sam, sak, sbk, sbn, scm, a_b, b_b, c_b, a_size, b_size, c_size, c_rows)"""
    M, N, K = c['M'], c['N'], c['K']
    if c['a'] == 'k':
        sam, sak = K + c['sam_pad'], 1
        a_slot = M * sam
    elif c['a'] == 'm':
        sam, sak = 1, M + c['sam_pad']
        a_slot = max(K, 1) * sak
    else:
        sam, sak = 2 * K + 1, 2
        a_slot = M * sam
    if c['b'] == 'k':
        sbn, sbk = K, 1
        b_slot = N * max(K, 1)
    elif c['b'] == 'n':
        sbk, sbn = N, 1
        b_slot = max(K, 1) * N
    else:
        sbn, sbk = 2 * K + 1, 2
        b_slot = N * sbn
    scm = N + c['scm_pad']
    c_rows = M + 1                                   # one canary row past M in every batch slot
    c_slot = c_rows * scm
    return dict(sam=sam, sak=sak, sbk=sbk, sbn=sbn, scm=scm, a_b=(c['B2'] * a_slot, a_slot), b_b=(c['B2'] * b_slot, b_slot),
                c_b=(c['B2'] * c_slot, c_slot), a_size=c['a_off'] + c['B1'] * c['B2'] * a_slot + 4,
                b_size=c['b_off'] + c['B1'] * c['B2'] * b_slot + 4, c_size=c['c_off'] + c['B1'] * c['B2'] * c_slot + 8, c_rows=c_rows)


def case_plan(c, det=None):
    s = strides(c)
    return gemm_plan(c['M'], c['N'], c['K'], s['sam'], s['sak'], s['sbk'], s['sbn'], s['scm'], c['bias'], c['act'], c['mode'],
                     c['B1'] * c['B2'], c['a_off'] % 4 == 0, c['b_off'] % 4 == 0, c['det'] if det is None else det)


def make(c):
    """Seeded float32 storage of a case: A, B, bias (N entries: the planted bias[n] fault reads them all), C0 (the marker
    everywhere; mode 1: non-zero prior values where the result goes), and the geometry."""
    s = strides(c)
    g = _gen('gemm', c['name'])
    A = torch.randn(s['a_size'], generator=g)
    B = torch.randn(s['b_size'], generator=g)
    if c['act'] in (ACT_TANH, ACT_SIGMOID):          # pre-activations of size 1: a saturated tanh would hide any error
        B = B / math.sqrt(max(c['K'], 1))
    bias = torch.randn(c['N'], generator=g) if c['bias'] else None
    C0 = torch.full((s['c_size'],), MARKER)
    if c['mode'] == 1:
        prior = torch.randn(c['B1'], c['B2'], c['M'], c['N'], generator=g) * (0.5 * math.sqrt(max(c['K'], 1)))
        c_view(c, C0)[:, :, :c['M']] = prior
    return types.SimpleNamespace(A=A, B=B, bias=bias, C0=C0, **s)


def c_view(c, Cs):
    """(B1, B2, M + 1, N) view of the result (and its canary row) inside the C storage"""
    s = strides(c)
    return torch.as_strided(Cs, (c['B1'], c['B2'], s['c_rows'], c['N']), (s['c_b'][0], s['c_b'][1], s['scm'], 1), c['c_off'])


def valid_mask(c, Cs):
    m = torch.zeros(Cs.shape, dtype=torch.bool)
    c_view(c, m)[:, :, :c['M']] = True
    return m


def operands(c, d, dtype=torch.float64):
    """logical A (B1, B2, M, K) and B (B1, B2, K, N) read from storage through strides, batch strides and offsets"""
    nb = (c['B1'], c['B2'])
    A = torch.as_strided(d.A.to(dtype), nb + (c['M'], c['K']), (d.a_b[0], d.a_b[1], d.sam, d.sak), c['a_off'])
    B = torch.as_strided(d.B.to(dtype), nb + (c['K'], c['N']), (d.b_b[0], d.b_b[1], d.sbk, d.sbn), c['b_off'])
    return A, B


def _bias_cols(c, bias, dtype, fault=None):
    n = torch.arange(c['N'])
    return bias.to(dtype)[n if fault == 'bias_n' else n // c['bias_div']]


# ================================================================================================ float64 references
def ref_gemm(c, d):
    """(reference, denominator), both (B1, B2, M, N) float64, of the case's call on the storage `d` (make)"""
    A, B = operands(c, d)
    acc = A @ B
    den2 = (c['alpha'] ** 2) * ((A * A) @ (B * B))
    if c['mode'] == 1:
        prior = c_view(c, d.C0)[:, :, :c['M']].double()
        return prior + c['alpha'] * acc, (den2 + prior * prior).sqrt()
    y = c['alpha'] * acc
    if d.bias is not None:
        b = _bias_cols(c, d.bias, torch.float64)
        y, den2 = y + b, den2 + b * b
    return act64(y, c['act'], c['slope']), den2.sqrt()


def _d(t):
    return t.detach().cpu().double()


def ref_grouped_fwd(x, w, b=None):
    x, w = _d(x), _d(w)
    y, den2 = x @ w.t(), (x * x) @ (w * w).t()
    if b is not None:
        y, den2 = y + _d(b), den2 + _d(b) ** 2
    return y, den2.sqrt()


def ref_grouped_dx(dys, ws):
    """dx = sum_l dy_l W_l over the layers with an upstream gradient"""
    y = sum(_d(dy) @ _d(w) for dy, w in zip(dys, ws))
    den2 = sum((_d(dy) ** 2) @ (_d(w) ** 2) for dy, w in zip(dys, ws))
    return y, den2.sqrt()


def ref_dw(dy, x, prior=None):
    """prior + dy^T x"""
    dy, x = _d(dy), _d(x)
    y, den2 = dy.t() @ x, (dy * dy).t() @ (x * x)
    if prior is not None:
        y, den2 = y + _d(prior), den2 + _d(prior) ** 2
    return y, den2.sqrt()


def ref_colsum(x, prior=None):
    """prior + column sums of x (rows, cols): the bias gradient, muvo_colsum_acc"""
    x = _d(x)
    y, den2 = x.sum(0), (x * x).sum(0)
    if prior is not None:
        y, den2 = y + _d(prior), den2 + _d(prior) ** 2
    return y, den2.sqrt()


def ref_act_bwd(y, dy, act, slope=SLOPE):
    """dy * act'(through y).  The derivative is formed from terms of size <= 1 (1 - y * y, y * (1 - y), y + 1), so its rounding
    error is absolute, not relative to the derivative: the denominator is |dy|, the scale of one product with a factor <= 1."""
    dy = _d(dy)
    return dy * act_grad_from_out(_d(y), act, slope), dy.abs()


# ================================================================================================ emulations (float32)
F32 = torch.float32


def _chain(a, b):
    """serial MFMA chain over the whole K of a (M, K) x (K, N) float32 product, as float32"""
    if a.shape[1] == 0:
        return torch.zeros(a.shape[0], b.shape[1])
    g = types.SimpleNamespace(a=a, b=b, unpack=lambda r: r)
    return CR.emulate_gemm(g, 'f32_chain').float()


def emu_tiled_sum(a, b, ksplit=1):
    """list of per-range chain sums (float32 (M, N)) of the tiled kernel: 16-wide k-tiles dealt to ksplit ranges"""
    K = a.shape[1]
    nkt = _cdiv(K, 16)
    per = _cdiv(nkt, ksplit) if ksplit else 0
    parts = []
    for s in range(ksplit):
        k0, k1 = min(s * per * 16, K), min((s + 1) * per * 16, K)
        parts.append(None if (k0 >= k1 and ksplit > 1) else _chain(a[:, k0:k1], b[k0:k1]))
    return parts


def emu_kcontig_sum(a, b):
    M, K = a.shape
    N = b.shape[1]
    Kp = _cdiv(max(K, 1), 64) * 64
    ap, bp = torch.zeros(M, Kp), torch.zeros(Kp, N)
    ap[:, :K], bp[:K] = a, b
    acc = torch.zeros(M, N, 64)
    for k0 in range(0, Kp, 64):
        acc = acc + ap[:, None, k0:k0 + 64] * bp[k0:k0 + 64].t()[None]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):                   # wave_sum: v += shfl_xor(v, o)
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def emu_kvec_sum(a, b):
    M, K = a.shape
    N = b.shape[1]
    it = _cdiv(K, 4096)
    ap, bp = torch.zeros(M, it * 4096), torch.zeros(N, it * 4096)
    ap[:, :K], bp[:, :K] = a, b.t()
    ap, bp = ap.view(M, 1, it, 2, 512, 4), bp.view(1, N, it, 2, 512, 4)
    acc = torch.zeros(M, N, 512)
    for i in range(it):
        p, q = ap[:, :, i, 0] * bp[:, :, i, 0], ap[:, :, i, 1] * bp[:, :, i, 1]
        e = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
        e = (((e + q[..., 0]) + q[..., 1]) + q[..., 2]) + q[..., 3]
        acc = acc + e
    acc = acc.view(M, N, 8, 16, 4)                   # (wave, lane / 4, lane % 4): four interleaved serial sums over the lanes
    s = torch.zeros(M, N, 8, 4)
    for l in range(16):
        s = s + acc[:, :, :, l]
    red = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
    out = torch.zeros(M, N)
    for w in range(8):
        out = out + red[:, :, w]
    return out


def emu_ncontig_sum(a, b, ks=1):
    """list of the KS range sums (float32 (M, N)) of the n-contiguous kernel"""
    M, K = a.shape
    N = b.shape[1]
    kper = _cdiv(_cdiv(K, ks), 128) * 128
    ap, bp = torch.zeros(M, ks * kper), torch.zeros(ks * kper, N)
    ap[:, :K], bp[:K] = a[:, :ks * kper], b[:ks * kper]
    assert K <= ks * kper
    ap, bp = ap.view(M, 1, ks, kper // 128, 4, 8, 4), bp.t().reshape(1, N, ks, kper // 128, 4, 8, 4)
    acc = torch.zeros(M, N, ks, 4)
    for ch in range(kper // 128):
        for g in range(8):
            p = ap[:, :, :, ch, :, g] * bp[:, :, :, ch, :, g]
            acc = acc + ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))
    s = ((acc[..., 0] + acc[..., 1]) + acc[..., 2]) + acc[..., 3]
    return [s[:, :, y] for y in range(ks)]


FAULTS = ('ktile_dropped', 'half_dropped', 'bias_n', 'bias_alpha', 'row_clamp', 'bf16x3')


def fault_applies(c, fault):
    if fault in ('ktile_dropped', 'bf16x3'):
        return c['K'] >= 1
    if fault == 'half_dropped':
        return c['K'] > 2048
    if fault == 'bias_n':
        return c['bias'] and c['bias_div'] > 1 and c['N'] > 1
    if fault == 'bias_alpha':
        return c['bias'] and c['alpha'] != 1.0
    return fault == 'row_clamp'


def emulate(c, d, fault=None):
    """The C storage after the case's call in the emulated arithmetic of the kernel gemm_plan routes it to.
    Faults: 'ktile_dropped' the middle 16-wide k-tile contributes nothing; 'half_dropped' k in [2048, 4096) contributes
    nothing; 'bias_n' bias[n] in place of bias[n / bias_div]; 'bias_alpha' the bias is multiplied by alpha; 'row_clamp' the row
    past M is computed from row M - 1 and stored; 'bf16x3' the products are formed from bf16 hi / lo planes."""
    plan = case_plan(c)
    A, B = operands(c, d, F32)
    A, B = A.clone(), B.clone()
    K = c['K']
    if fault == 'ktile_dropped':
        t = (_cdiv(K, 16) // 2) * 16
        A[..., t:t + 16] = 0
    if fault == 'half_dropped':
        A[..., 2048:4096] = 0
    alpha = torch.tensor(c['alpha'], dtype=F32)
    Cs = d.C0.clone()
    out = c_view(c, Cs)
    for b1 in range(c['B1']):
        for b2 in range(c['B2']):
            a, b = A[b1, b2], B[b1, b2]
            if fault == 'bf16x3':
                g = types.SimpleNamespace(a=a, b=b, unpack=lambda r: r)
                parts = [CR.emulate_gemm(g, 'bf16x3').float()]
            elif plan['kernel'] == 'tiled':
                parts = emu_tiled_sum(a, b, plan['ksplit'])
            elif plan['kernel'] == 'skinny_kcontig':
                parts = [emu_kcontig_sum(a, b)]
            elif plan['kernel'] == 'skinny_kvec':
                parts = [emu_kvec_sum(a, b)]
            else:
                parts = emu_ncontig_sum(a, b, plan['ksplit'])
            if c['mode'] == 1 or (plan['kernel'] == 'skinny_ncontig' and plan['ksplit'] > 1):
                y = out[b1, b2, :c['M']].clone() if c['mode'] == 1 else torch.zeros(c['M'], c['N'])
                for p in parts:
                    if p is not None:
                        y = y + alpha * p
            else:
                y = alpha * parts[0]
                if d.bias is not None:
                    bv = _bias_cols(c, d.bias, F32, fault)
                    y = y + (alpha * bv if fault == 'bias_alpha' else bv)
                y = act32(y, c['act'], c['slope'])
            out[b1, b2, :c['M']] = y
            if fault == 'row_clamp':
                out[b1, b2, c['M']] = y[c['M'] - 1]
    return Cs


# ================================================================================================ judging a result
def bar_of(c):
    """the bar of a muvo_gemm case: that of the kernel the dispatch mirror routes it to"""
    return kernel_bar(case_plan(c)['kernel'], c['K'])


def judge(c, d, Cs, ref=None):
    """Compares the C storage after a call with the float64 reference and the canaries.
    Returns dict(stats, bar, share, canary_ok, n_canary_bad, where)."""
    ref, den = ref if ref is not None else ref_gemm(c, d)
    Cs = Cs.detach().cpu()
    got = c_view(c, Cs)[:, :, :c['M']]
    st = error_stats(got, ref, den)
    bar = bar_of(c)
    keep = ~valid_mask(c, Cs)
    bad = (Cs.view(torch.int32)[keep] != d.C0.view(torch.int32)[keep])
    return dict(stats=st, bar=bar, share=excess(st, bar), canary_ok=not bool(bad.any()), n_canary_bad=int(bad.sum()),
                where=locate(c, st['index']))


def passes(j):
    return j['canary_ok'] and within(j['stats'], j['bar'])


def locate(c, index):
    """the worst element by batch, row, column, workgroup and the K ranges that add into it"""
    b1, b2, m, n = index
    p = case_plan(c)
    if p['kernel'] == 'tiled':
        wg = f'tile ({n // p["tile"][1]}, {m // p["tile"][0]}) of {p["tile"][0]}x{p["tile"][1]}'
        own = f'k ranges 0..{p["ksplit"] - 1} of {_cdiv(_cdiv(c["K"], 16), p["ksplit"])} k-tiles each' if p['ksplit'] > 1 else 'one k range'
    elif p['kernel'] == 'skinny_ncontig':
        wg, own = f'column block {n // 64} lane {n % 64}', f'k ranges 0..{p["ksplit"] - 1}' if p['ksplit'] > 1 else 'one k range'
    elif p['kernel'] == 'skinny_kvec':
        wg, own = f'workgroup {n // 4} column {n % 4}, row template {p["rm"]}', 'eight waves split k'
    else:
        wg, own = f'workgroup {n // 8} wave {(n // 2) % 4} column {n % 2}, row chunk {m // p["rm"]}', 'one wave strides k'
    return f'batch ({b1}, {b2}) row {m} column {n}: {p["kernel"]} {wg}; {own}'


def statline(c, j, kernel):
    s = j['stats']
    return f'GEMMSTAT {c["name"]} {kernel}: max e {s["max_e"]:.3e} rms {s["rms"]:.3e} share {j["share"]:.2f}'


# ================================================================================================ the case lists
T, KV, KC, NC = 'tiled', 'skinny_kvec', 'skinny_kcontig', 'skinny_ncontig'


def _tiled_cases():
    out = [
        gcase('t32-7x33x5', 7, 33, 5, dict(kernel=T, tile=(32, 128)), bias=True),
        gcase('t32-20x200x10', 20, 200, 10, dict(kernel=T, tile=(32, 128))),                       # K < 16 keeps M <= 32 off the skinny kernels
        gcase('t32-16x40x12-batched', 16, 40, 12, dict(kernel=T, tile=(32, 128), grid=(1, 1, 6)), B1=2, B2=3, bias=True, act=ACT_RELU),
        gcase('t64-130x48x70', 130, 48, 70, dict(kernel=T, tile=(128, 64), grid=(1, 2, 1))),
        gcase('t64-300x1x16', 300, 1, 16, dict(kernel=T, tile=(128, 64), grid=(1, 3, 1)), bias=True),
        gcase('t64-64x64x1', 64, 64, 1, dict(kernel=T, tile=(128, 64))),
        gcase('t128-130x257x70', 130, 257, 70, dict(kernel=T, tile=(128, 128), grid=(3, 2, 1)), bias=True, act=ACT_ELU),
    ]
    # loader pairs on the 128x128 and the 32x128 tile (M <= 32 stays tiled through mode / K < 16 / batches: here K = 13 ... )
    for a, b, lay in (('k', 'k', (1, 1)), ('k', 'n', (1, 0)), ('m', 'k', (0, 1)), ('m', 'n', (0, 0)), ('s', 's', (0, 0))):
        out.append(gcase(f't128-lay-{a}{b}', 130, 131, 37, dict(kernel=T, tile=(128, 128), lay=lay), a=a, b=b, ident=a != 's'))
        out.append(gcase(f't32-lay-{a}{b}', 9, 131, 37, dict(kernel=T, tile=(32, 128), lay=lay), a=a, b=b, B2=2))
    out.append(gcase('t128-K0-bias', 130, 70, 0, dict(kernel=T, tile=(128, 128)), bias=True))
    for K in (1, 15, 17, 129):
        out.append(gcase(f't128-K{K}', 130, 70, K, dict(kernel=T, tile=(128, 128))))
    for act in ALL_ACTS:
        out.append(gcase(f't128-act-{ACT_NAMES[act]}', 130, 131, 70, dict(kernel=T, tile=(128, 128)), bias=True, act=act, alpha=0.37))
    out += [
        gcase('t128-biasdiv65', 40, 20 * 65, 24, dict(kernel=T, tile=(128, 128)), bias=True, bias_div=65, alpha=0.37, act=ACT_ELU),
        gcase('t128-scm', 130, 70, 37, dict(kernel=T, tile=(128, 128)), scm_pad=3, bias=True),
        gcase('t128-offsets', 130, 70, 37, dict(kernel=T, tile=(128, 128)), a_off=1, b_off=1, c_off=1),
        # accumulate mode
        gcase('t128-acc-40x70x130', 40, 70, 130, dict(kernel=T, tile=(128, 128), ksplit=2), mode=1, a='m', b='n'),
        gcase('t128-acc-48x96x1000', 48, 96, 1000, dict(kernel=T, tile=(128, 128), ksplit=8), mode=1, a='m', b='n', alpha=0.37),
        gcase('t32-acc-8x70x300', 8, 70, 300, dict(kernel=T, tile=(32, 128), ksplit=3), mode=1),   # M <= 32, N >= 64, K >= 16: tiled only because mode = 1
        gcase('t32-acc-batched', 16, 40, 130, dict(kernel=T, tile=(32, 128), ksplit=2, grid=(1, 1, 12)), mode=1, B1=2, B2=3),
        gcase('t128-acc-det', 48, 96, 1000, dict(kernel=T, tile=(128, 128), ksplit=1), mode=1, a='m', b='n', det=True, twice=True),
    ]
    return out


def _kvec_cases():
    out = []
    ms, ns, ks = (1, 4, 5, 8, 9, 16, 17, 24), (2, 66, 67), (64, 68, 2048, 2052, 4096, 4104)
    rm = {1: 4, 4: 4, 5: 8, 8: 8, 9: 16, 16: 16, 17: 24, 24: 24}
    # every M at every K once (N cycles), every N at every K; the other axes ride along: bias_div 1 / 3, the six activations
    # and scm > N cycle through the list so that each appears on every row template
    i = 0
    for mi, M in enumerate(ms):
        for ki, K in enumerate(ks):
            N = ns[(mi + ki) % 3]
            act = ALL_ACTS[i % 6]
            bias = i % 12 not in (0, 7)
            out.append(gcase(f'kv-{M}x{N}x{K}', M, N, K, dict(kernel=KV, rm=rm[M], grid=(_cdiv(N, 4), 1, 1)), bias=bias,
                             bias_div=3 if (bias and i % 2) else 1, act=act, scm_pad=5 if i % 3 == 0 else 0,
                             alpha=0.37 if i % 5 == 0 else 1.0))
            i += 1
    return out


def _kcontig_cases():
    e4, e8 = dict(kernel=KC, rm=4), dict(kernel=KC, rm=8)
    return [
        gcase('kc-K70-3x66', 3, 66, 70, e4, bias=True, act=ACT_TANH),                   # K % 4 != 0
        gcase('kc-K70-4x65', 4, 65, 70, dict(e4, grid=(9, 1, 1))),                      # last wave: one column
        gcase('kc-aoff-5x66x64', 5, 66, 64, e8, a_off=1, bias=True, bias_div=3),        # A off 16-byte alignment
        gcase('kc-boff-8x66x68', 8, 66, 68, e8, b_off=1),
        gcase('kc-sam-24x67x64', 24, 67, 64, e8, sam_pad=1, act=ACT_SIGMOID, bias=True),       # sam = K + 1; three row chunks
        gcase('kc-25x65x68', 25, 65, 68, e8, bias=True, act=ACT_LEAKY, scm_pad=2),      # 25 rows: vector-eligible but past its 24 rows
        gcase('kc-32x66x64', 32, 66, 64, e8),
        gcase('kc-32x2x64', 32, 2, 64, e8, alpha=0.37, bias=True),                      # N < 64 reaches the skinny branch through the vector test alone
        gcase('kc-K17-5x65', 5, 65, 17, e8, bias=True, act=ACT_ELU),                    # idle lanes
        gcase('kc-K2052-9x66', 9, 66, 2052, e8, a_off=2),
    ]


def _ncontig_cases():
    rm = {3: 4, 4: 4, 5: 8, 8: 8, 9: 24, 24: 24, 25: 24, 32: 24}
    out = []
    for i, M in enumerate((3, 4, 5, 8, 9, 24, 25, 32)):
        N = (64, 100)[i % 2]
        out.append(gcase(f'nc-{M}x{N}x130', M, N, 130, dict(kernel=NC, rm=rm[M], ksplit=2, grid=(_cdiv(N, 64), 2, 1)), b='n'))
    out += [
        gcase('nc-seed-4x1300x48', 4, 1300, 48, dict(kernel=NC, rm=4, ksplit=1), b='n', bias=True, bias_div=65, act=ACT_ELU),
        gcase('nc-5x100x640', 5, 100, 640, dict(kernel=NC, rm=8, ksplit=10), b='n'),    # kper 128: ranges 5 ... 9 are empty
        gcase('nc-9x100x130-scm', 9, 100, 130, dict(kernel=NC, rm=24, ksplit=1), b='n', scm_pad=4),
        gcase('nc-25x64x130-det', 25, 64, 130, dict(kernel=NC, rm=24, ksplit=1), b='n', det=True, twice=True),
        gcase('nc-8x100x16-act', 8, 100, 16, dict(kernel=NC, rm=8, ksplit=1), b='n', act=ACT_TANH, bias=True, alpha=0.37, a='m'),
    ]
    return out


GEMM_CASES = _tiled_cases() + _kvec_cases() + _kcontig_cases() + _ncontig_cases()
assert len({c['name'] for c in GEMM_CASES}) == len(GEMM_CASES)


# grouped Linear: (name, M, K, layer widths, per layer: has bias, weight trains, bias trains, upstream gradient present), x trains
def grcase(name, M, K, ns, nobias=(), frozen=(), frozen_w=(), unused=(), x_grad=True):
    return dict(name=name, M=M, K=K, ns=list(ns), nobias=set(nobias), frozen=set(frozen), frozen_w=set(frozen_w),
                unused=set(unused), x_grad=x_grad)


WIDTHS = [1, 2, 5, 16, 130]
GROUPED_CASES = [
    grcase('gr-1x64', 1, 64, WIDTHS),
    grcase('gr-8x68', 8, 68, WIDTHS, nobias={1}),
    grcase('gr-9x260', 9, 260, WIDTHS, frozen={2}),                              # a frozen layer in the middle
    grcase('gr-24x2052', 24, 2052, WIDTHS, frozen_w={3}),                        # frozen weight, trainable bias
    grcase('gr-8x4100', 8, 4100, WIDTHS, unused={0, 4}),                         # second pass of the k loop; unused outputs
    grcase('gr-24x4100', 24, 4100, [5, 130], x_grad=False),
    grcase('gr-9x68-L16', 9, 68, [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3], nobias={15}, frozen_w={0}),
    grcase('gr-24x64-L1', 24, 64, [130]),
    grcase('gr-1x260-L1', 1, 260, [1], x_grad=False),
]

COLSUM_CASES = [(rows, cols, pad) for rows in (1, 63, 64, 65, 130) for cols, pad in ((1, 2), (64, 0), (65, 3))]
LINEAR_FN_CASES = [(130, 40, 70), (9, 64, 16)]                                  # rows, out features, in features
SEED_CASE = dict(n=4, ci=48, co=20, kh=5, kw=13)


def grouped_inputs(c):
    g = _gen('grouped', c['name'])
    x = torch.randn(c['M'], c['K'], generator=g)
    ws = [torch.randn(n, c['K'], generator=g) for n in c['ns']]
    bs = [None if l in c['nobias'] else torch.randn(n, generator=g) for l, n in enumerate(c['ns'])]
    dys = [None if l in c['unused'] else torch.randn(c['M'], n, generator=g) for l, n in enumerate(c['ns'])]
    gw = [torch.randn(n, c['K'], generator=g) * math.sqrt(c['M']) for n in c['ns']]          # non-zero .grad to accumulate into
    gb = [torch.randn(n, generator=g) * math.sqrt(c['M']) for n in c['ns']]
    return types.SimpleNamespace(x=x, ws=ws, bs=bs, dys=dys, gw=gw, gb=gb)


def grouped_trains(c, l):
    """(weight trains, bias trains) of layer l"""
    w = l not in c['frozen'] and l not in c['frozen_w']
    b = l not in c['frozen'] and l not in c['nobias']
    return w, b


def emu_grouped_fwd(x, w, b=None):
    y = emu_kvec_sum(x, w.t())
    return y if b is None else y + b


def emu_grouped_dx(dys, ws):
    """slabs of 128 weight rows in layer order, each in the n-contiguous kernel's wave scheme, added to the zeroed dx"""
    dx = None
    for dy, w in zip(dys, ws):
        for n0 in range(0, w.shape[0], 128):
            part = emu_ncontig_sum(dy[:, n0:n0 + 128], w[n0:n0 + 128], 1)[0]
            dx = part if dx is None else dx + part
    return dx


def emu_grouped_dw(dy, x, prior):
    g = torch.zeros(dy.shape[1], x.shape[1])
    for m in range(x.shape[0]):
        g = g + dy[m][:, None] * x[m][None]
    return prior + g


def emu_grouped_db(dy, prior):
    s = torch.zeros(dy.shape[1])
    for m in range(dy.shape[0]):
        s = s + dy[m]
    return prior + s


def emu_colsum(x, prior, det=False):
    """colsum_kernel: row chunks, four row lanes per column (eight rows per pass as a pair tree, then one by one), the chunks
    added to `out` in index order"""
    rows = x.shape[0]
    chunks = 1 if det else min(_cdiv(rows, 64), 1024)
    per = _cdiv(rows, chunks)
    out = prior.clone()
    for ch in range(chunks):
        r0, r1 = ch * per, min((ch + 1) * per, rows)
        lanes = []
        for rl in range(4):
            s, r = torch.zeros(x.shape[1]), r0 + rl
            while r + 28 < r1:
                v = [x[r + 4 * u] for u in range(8)]
                s = s + (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
                r += 32
            while r < r1:
                s = s + x[r]
                r += 4
            lanes.append(s)
        out = out + (((lanes[0] + lanes[1]) + lanes[2]) + lanes[3])
    return out


def grouped_emulated(c, inp):
    """[(kind, label, K, emulated result, (reference, denominator))] of every output of a grouped case"""
    used = [l for l in range(len(c['ns'])) if l not in c['unused']]
    out = [('grouped_fwd', f'y{l}', c['K'], emu_grouped_fwd(inp.x, inp.ws[l], inp.bs[l]), ref_grouped_fwd(inp.x, inp.ws[l], inp.bs[l]))
           for l in range(len(c['ns']))]
    dys, ws = [inp.dys[l] for l in used], [inp.ws[l] for l in used]
    out.append(('grouped_dx', 'dx', sum(c['ns'][l] for l in used), emu_grouped_dx(dys, ws), ref_grouped_dx(dys, ws)))
    for l in used:
        out.append(('grouped_dw', f'dW{l}', c['M'], emu_grouped_dw(inp.dys[l], inp.x, inp.gw[l]), ref_dw(inp.dys[l], inp.x, inp.gw[l])))
        out.append(('grouped_db', f'db{l}', c['M'], emu_grouped_db(inp.dys[l], inp.gb[l]), ref_colsum(inp.dys[l], inp.gb[l])))
    return out


def colsum_inputs(rows, cols, pad):
    """x as a (rows, cols) view of a (rows, cols + pad) matrix, and a non-zero prior"""
    g = _gen('colsum', rows, cols)
    return torch.randn(rows, cols + pad, generator=g)[:, :cols], torch.randn(cols, generator=g) * math.sqrt(rows)


def own_worst():
    """OWN_WORST recomputed from the emulations: {kind: [rms, max e] in units of u sqrt(K)} (all kernels, not only the listed)"""
    w = collections.defaultdict(lambda: [0.0, 0.0])

    def upd(kind, st, K):
        r = math.sqrt(max(K, 1)) * CR.U32
        w[kind] = [max(w[kind][0], st['rms'] / r), max(w[kind][1], st['max_e'] / r)]
    for c in GEMM_CASES:
        d = make(c)
        upd(case_plan(c)['kernel'], judge(c, d, emulate(c, d))['stats'], c['K'])
    for c in GROUPED_CASES:
        for kind, _, K, got, ref in grouped_emulated(c, grouped_inputs(c)):
            upd(kind, error_stats(got, *ref), K)
    for rows, cols, pad in COLSUM_CASES:
        x, prior = colsum_inputs(rows, cols, pad)
        for det in (False, True):
            upd('colsum', error_stats(emu_colsum(x, prior, det), *ref_colsum(x, prior)), rows)
    return dict(w)


def grouped_fault_frozen_bias(c, inp):
    """the suspected fault of grouped_linear_wgrad_kernel: a layer whose weight is frozen loses its bias gradient.  Returns
    {layer: db} as that kernel would leave them (the prior .grad untouched) for the layers it applies to."""
    return {l: inp.gb[l].clone() for l in c['frozen_w'] if l not in c['nobias'] and l not in c['unused']}


# ================================================================================================ attention in float32
def attention_float32(qkv, heads, dout):
    """the unfused attention core (scores, softmax, PV and the backward products) in plain float32 torch on the CPU, p = 0"""
    import attention_reference as AR
    E = qkv.shape[-1] // 3
    scale = (E // heads) ** -0.5
    q, k, v = (AR._heads(qkv[:, :, i * E:(i + 1) * E].float(), heads) for i in range(3))
    do = AR._heads(dout.float(), heads)
    P = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1)
    o = P @ v
    dv = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    dS = (dP - (dP * P).sum(-1, keepdim=True)) * P
    dq, dk = (dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale
    return {'o': AR._packed(o), 'dqkv': torch.cat([AR._packed(dq), AR._packed(dk), AR._packed(dv)], -1)}


def attention_inputs(case):
    l, n, h, dh = case
    g = _gen('gemm-attention', case)
    return torch.randn(l, n, 3 * h * dh, generator=g), torch.randn(l, n, h * dh, generator=g)


@functools.lru_cache(maxsize=None)
def attention_reference64(case):
    import attention_reference as AR
    qkv, dout = attention_inputs(case)
    return AR.reference64(qkv, case[2], dout)


def attention_errors(case, got):
    """{name: e} of o / dqkv against the float64 reference, e = max |got - ref| / max |ref|"""
    from loss_reference import error_stats as es, scale_of
    ref = attention_reference64(case)
    return {n: es(got[n], ref[n], scale_of(ref[n]))['max_e'] for n in ('o', 'dqkv')}


if __name__ == '__main__':
    for k, (rms, e) in sorted(own_worst().items()):
        print(f"    '{k}': ({rms:.3f}, {e:.3f}),   share of f32_bar: rms {rms / 0.46:.2f} max e {e / 4.8:.2f}")
    for case in ATTN_CASES:
        qkv, dout = attention_inputs(case)
        e = attention_errors(case, attention_float32(qkv, case[2], dout))
        print(f'    {case}: {{' + ', '.join(f"'{n}': {v:.2e}" for n, v in e.items()) + '},')
