"""Plain float64 references, CPU emulations of the two arithmetics and a restatement of the dispatch for the implicit-GEMM
convolutions (muvo_amd/csrc/conv_gemm.hip: exact fp32 MFMA; conv_bf3.hip: bf16x3 split products; conv_pw.hip: 1x1 heads).
Helpers only: no fixtures, no tests.  The metric, the activations and the bf16x3 bar are those of tests/vox_reference.py.

References.  `Layer` describes one Conv2d / ConvTranspose2d / Conv3d (any kernel size, stride, padding, output padding; no
dilation: muvo_amd.nn has none).  ref_forward / ref_dgrad / ref_wgrad / ref_bgrad return (reference, denominator) in
float64; the denominator is the same operation on the squared operands, square-rooted, i.e. the scale of the rounding error
of that one element (vox_reference: e = |got - ref64| / den).

Emulations.  Every operation here is a GEMM over an im2col matrix of a stride-s "conv form" (a transposed convolution is the
conv form of its zero-inserted input with the flipped kernel): gemm_form() returns the two fp32 factors with K ordered
(tap, channel) as the fp32 kernels pack it.  emulate_gemm() evaluates them
  'bf16x3'          hi = bf16(v), lo = bf16(v - hi), round to nearest even; lo*hi + hi*lo + hi*hi
  'two_products'    the data operand's lo times the weight's hi is lost everywhere
  'tap_lo_dropped'  both cross products of one tap are lost
  'krange_lo_dropped'  both cross products of one contiguous K range (one workgroup of a split-K launch) are lost
  'f32_chain'       serial fp32 accumulation over the whole K in K order, two products per step as mfma_f32_32x32x2f32
                    consumes them: the pessimistic model of the fp32 kernels (split-K only shortens the chain).

Dispatch mirror.  conv_plan() restates, for muvo_conv_set_bf16x3_min_gflop(0) and no MUVO_* tuning variable, what
conv_gemm.hip / conv_bf3.hip decide on the host: phases, one arithmetic per operation, merging, layouts, family, tile,
split-K and the weight-gradient launch.  tests/test_conv_bars.py holds it against the library's own answers."""
import collections
import itertools
import math

import torch
import torch.nn.functional as F

import vox_reference as V
from vox_reference import ACT_ELU, ACT_LEAKY, ACT_NONE, ACT_RELU, SLOPE, act64, error_stats, excess, within  # noqa: F401

U32 = 2.0 ** -24            # unit roundoff of fp32

BF3_BAR = V.BARS['bf3']     # (rms 1.5e-5, max e 6e-5): 3x the arithmetic (emulated: rms 4.0-5.0e-6, max e 1.3-2.5e-5 at K = 12 ... 5760)

# Measured on an MI355X by tests/test_conv_kernels_gpu.py (CONVSTAT lines; largest over all cases and run modes).  Not the source
# of any bar: the bars above / below come from the float64 reference and the CPU emulations alone.
#   bf16x3 (family 1)      forward   max e 2.4e-5  rms 4.7e-6      data gradient  2.3e-5 / 4.9e-6     weight gradient 2.5e-5 / 4.7e-6
#                          bias gradient (fp32 sums of the split pass / bias_grad_kernel) 9.3e-7 / 2.3e-7
#   bf16x3 products in conv_wgrad_kernel<..., true>                    weight gradient 2.1e-5 / 4.4e-6 (fp32 bars of the cases: rms 3.2-3.9e-6)
#   fused head             stage y 2.4e-5 / 4.6e-6   logits vs head(own y) 5.9e-7 / 8.6e-8   logits vs composition 2.0e-5 / 4.2e-6
#                          dx 2.6e-5 / 4.6e-6   dW 2.2e-5 / 4.5e-6   db 1.2e-6 / 2.7e-7   head dW 7.8e-7 / 2.0e-7   head db 2.7e-7 / 3.1e-7
#   token-major Linear     forward 1.9e-5 / 4.5e-6   data gradient 1.9e-5 / 4.4e-6   weight gradient 1.7e-5 / 4.5e-6   bias 2.8e-7 / 9.0e-8
#   fp32 (family 0)        forward 6.3e-6 / 5.4e-7 (at most 0.76 of its bar)   data gradient 5.0e-6 / 5.9e-7 (0.66)
#                          weight gradient 4.9e-6 / 6.0e-7 (0.65)   bias gradient 4.5e-7 / 2.0e-7 (0.38)
#   1x1 heads (family 3)   forward 1.6e-6 / 2.1e-7 (0.74)   data gradient 2.6e-7 / 4.8e-8 (0.95: with 1 ... 4 terms the VALU kernel rounds
#                          every product and every sum, which the MFMA chain does not)   accumulated 2.6e-7 / 5.1e-8 (0.83)
#                          weight gradient 3.7e-7 / 1.1e-7 (0.09)   bias gradient 2.0e-7 / 3.6e-7 (0.30)


def f32_bar(k):
    """(rms, max e) bar of an exact-fp32 result whose reduction has k terms (forward / data gradient: taps x channels of the
    longest launch; weight / bias gradient: pixels): 2x the f32_chain emulation.  A serial chain of k / 2 MFMA steps rounds
    partial sums of growing size, which leaves c u sqrt(k) in units of the element's scale sqrt(sum a^2 b^2); the emulation
    measures c = 0.165 ... 0.228 for the rms and up to 2.4 for the largest of <= 5 * 10^5 elements on the layers of the test
    matrix at k = 12 ... 5760.  tests/test_conv_bars.py checks the margin of 2 on every case, and that the bf16x3 arithmetic
    (rms 4.0-5.0e-6) fails this bar 4x: that holds up to k ~ 1350 products, so the fp32 cases stay below that."""
    r = math.sqrt(max(k, 1))
    return (0.46 * U32 * r, 4.8 * U32 * r)


# ------------------------------------------------------------------------------------------------ layers
class Layer(collections.namedtuple('Layer', 'kind cin cout k stride pad out_pad')):
    """kind: 'conv2d', 'convT2d' or 'conv3d'; k / stride / pad / out_pad: one int for every axis."""
    __slots__ = ()

    @property
    def nd(self):
        return 3 if self.kind == 'conv3d' else 2

    @property
    def transposed(self):
        return self.kind == 'convT2d'

    def out_size(self, in_sz):
        if self.transposed:
            return tuple((i - 1) * self.stride - 2 * self.pad + self.k + self.out_pad for i in in_sz)
        return tuple((i + 2 * self.pad - self.k) // self.stride + 1 for i in in_sz)

    def weight_shape(self):
        k = (self.k,) * self.nd
        return ((self.cin, self.cout) if self.transposed else (self.cout, self.cin)) + k

    def module(self, dev, bias=True):
        from muvo_amd import nn as hnn
        with torch.device(dev):
            if self.kind == 'conv3d':
                return hnn.Conv3d(self.cin, self.cout, self.k, self.stride, self.pad, bias=bias)
            if self.transposed:
                return hnn.ConvTranspose2d(self.cin, self.cout, self.k, self.stride, self.pad, self.out_pad, bias=bias)
            return hnn.Conv2d(self.cin, self.cout, self.k, self.stride, self.pad, bias=bias)

    def name(self):
        t = {'conv2d': '', 'convT2d': 'T', 'conv3d': '3d'}[self.kind]
        return f'{t}{self.cin}to{self.cout}k{self.k}s{self.stride}p{self.pad}' + (f'o{self.out_pad}' if self.out_pad else '')


def _d(t):
    return t.detach().cpu().double()


def fwd_op(layer, x, w):
    if layer.kind == 'conv3d':
        return F.conv3d(x, w, None, layer.stride, layer.pad)
    if layer.transposed:
        return F.conv_transpose2d(x, w, None, layer.stride, layer.pad, layer.out_pad)
    return F.conv2d(x, w, None, layer.stride, layer.pad)


def _grad(layer, x, w, dy, wrt):
    """d <fwd_op(x, w), dy> / d (x or w): the operation is bilinear, so the point of evaluation does not matter."""
    x = x.clone().requires_grad_(wrt == 'x')
    w = w.clone().requires_grad_(wrt == 'w')
    with torch.enable_grad():
        y = fwd_op(layer, x, w)
    return torch.autograd.grad(y, x if wrt == 'x' else w, dy)[0]


def ref_forward(layer, x, w, b=None, act=ACT_NONE, slope=SLOPE):
    """(reference, denominator) of act(conv(x, w) + b).  |act'| <= 1, so the pre-activation scale bounds the error after it."""
    x, w = _d(x), _d(w)
    y = fwd_op(layer, x, w)
    if b is not None:
        y = y + _d(b).view(1, -1, *([1] * layer.nd))
    return act64(y, act, slope), fwd_op(layer, x * x, w * w).sqrt()


def ref_dgrad(layer, dy, w, x_shape):
    dy, w = _d(dy), _d(w)
    z = torch.zeros(x_shape, dtype=torch.float64)
    return _grad(layer, z, w, dy, 'x'), _grad(layer, z, w * w, dy * dy, 'x').sqrt()


def ref_wgrad(layer, x, dy):
    x, dy = _d(x), _d(dy)
    z = torch.zeros(layer.weight_shape(), dtype=torch.float64)
    return _grad(layer, x, z, dy, 'w'), _grad(layer, x * x, z, dy * dy, 'w').sqrt()


def ref_bgrad(dy):
    dy = _d(dy)
    dims = (0,) + tuple(range(2, dy.dim()))
    return dy.sum(dim=dims), (dy * dy).sum(dim=dims).sqrt()


def ref_linear(x, w, b=None, act=ACT_NONE):
    x, w = _d(x), _d(w)
    y = x @ w.t()
    if b is not None:
        y = y + _d(b)
    return act64(y, act), ((x * x) @ (w * w).t()).sqrt()


def ref_matmul(a, b):
    """(a @ b, denominator) in float64 (Linear data / weight gradients, 1x1 heads)."""
    a, b = _d(a), _d(b)
    return a @ b, ((a * a) @ (b * b)).sqrt()


def act_derivative(y, act, slope=SLOPE):
    """d act / d pre-activation from the activated output y (exact for ReLU / LeakyReLU away from 0; ELU: y + 1 below 0)."""
    yc = y.detach().cpu()
    if act == ACT_RELU:
        return (yc > 0).to(yc.dtype)
    if act == ACT_LEAKY:
        return torch.where(yc > 0, torch.ones_like(yc), torch.full_like(yc, slope))
    if act == ACT_ELU:
        return torch.where(yc > 0, torch.ones_like(yc), yc + 1)
    return torch.ones_like(yc)


# ------------------------------------------------------------------------------------------------ GEMM form
def _im2col(inp, k, stride, pad_lo, out_sz):
    """inp [N][C][D][H][W] -> [N][T][C][P] with taps in (kz, ky, kx) order, P = prod(out_sz); element = inp at
    o * stride - pad_lo + tap (zero outside)."""
    n, c = inp.shape[:2]
    pads = []
    for a in (2, 1, 0):
        hi = max(0, (out_sz[a] - 1) * stride[a] + k[a] - pad_lo[a] - inp.shape[2 + a])
        pads += [pad_lo[a], hi]
    xp = F.pad(inp, pads)
    cols = []
    for kz, ky, kx in itertools.product(range(k[0]), range(k[1]), range(k[2])):
        cols.append(xp[:, :, kz:kz + (out_sz[0] - 1) * stride[0] + 1:stride[0], ky:ky + (out_sz[1] - 1) * stride[1] + 1:stride[1],
                       kx:kx + (out_sz[2] - 1) * stride[2] + 1:stride[2]].reshape(n, c, -1))
    return torch.stack(cols, dim=1)


def _zero_insert(t, stride):
    n, c, d, h, w = t.shape
    out = t.new_zeros(n, c, (d - 1) * stride[0] + 1, (h - 1) * stride[1] + 1, (w - 1) * stride[2] + 1)
    out[:, :, ::stride[0], ::stride[1], ::stride[2]] = t
    return out


def _as3d(layer, t):
    return t if layer.nd == 3 else t.unsqueeze(2)


def _geom3(layer):
    if layer.nd == 3:
        return (layer.k,) * 3, (layer.stride,) * 3, (layer.pad,) * 3
    return (1, layer.k, layer.k), (1, layer.stride, layer.stride), (0, layer.pad, layer.pad)


class GemmForm(collections.namedtuple('GemmForm', 'a b taps chans data_is_b unpack')):
    """result = unpack(a @ b) with a [R][K] and b [K][Q], both fp32.  taps / chans: tap and channel of each K index (weight
    gradient: of each result column; its K runs over pixels).  data_is_b: the activation operand (x or dy) is b, the weight a
    (forward / data gradient); weight gradient: a = dy, b = x columns."""
    __slots__ = ()


def gemm_form(layer, op, x=None, w=None, dy=None, in_sz=None):
    """The operation `op` ('fwd', 'dgrad', 'wgrad') of `layer` as one GEMM over all samples."""
    k3, s3, p3 = _geom3(layer)
    nd = layer.nd
    T = k3[0] * k3[1] * k3[2]
    one = (1, 1, 1)
    flip = op != 'wgrad' and (layer.transposed == (op == 'fwd'))        # convT forward / conv data gradient: zero-inserted form
    if op == 'wgrad':
        # conv: dw[m][c][t] = sum_p dy[m][p] col(x)[t][c][p]; convT: the same with the roles of x and dy exchanged
        big, small = (dy, x) if layer.transposed else (x, dy)           # big: the tensor the taps slide over
        big3, small3 = _as3d(layer, big.float()), _as3d(layer, small.float())
        col = _im2col(big3, k3, s3, p3, small3.shape[2:])               # [N][T][C][P]
        n, _, c, p = col.shape
        b = col.permute(0, 3, 1, 2).reshape(n * p, T * c)
        a = small3.reshape(n, small3.shape[1], p).permute(1, 0, 2).reshape(small3.shape[1], n * p)
        taps = torch.arange(T).repeat_interleave(c)
        chans = torch.arange(c).repeat(T)
        ksz = k3[3 - nd:]

        def unpack(r):               # [small][T][big] -> [small][big][k...]: conv [Cout][Cin][k], convT [Cin][Cout][k]
            return r.reshape(a.shape[0], T, c).permute(0, 2, 1).reshape(a.shape[0], c, *ksz)
        return GemmForm(a, b, taps, chans, False, unpack)
    src = x if op == 'fwd' else dy
    src3, w3 = _as3d(layer, src.float()), _as3d(layer, w.float())
    out_sz = _dims3(layer, in_sz if op == 'dgrad' else layer.out_size(src.shape[2:]))
    if not flip:
        # conv forward: weight [M][C][k]; convT data gradient: conv of dy (Cout) with the convT weight [Cin][Cout][k] as [M = Cin][C = Cout]
        col = _im2col(src3, k3, s3, p3, out_sz)
        wm = w3
    else:
        # zero-inserted form: out[o] = sum_r w[r] z[o + pad - r]  ->  tap r' = k - 1 - r, pad_lo = k - 1 - pad, stride 1
        z = _zero_insert(src3, s3)
        col = _im2col(z, k3, one, tuple(k - 1 - p for k, p in zip(k3, p3)), out_sz)
        wm = w3.flip(2, 3, 4).transpose(0, 1)
    n, _, c, p = col.shape
    b = col.permute(1, 2, 0, 3).reshape(T * c, n * p)
    m = wm.shape[0]
    a = wm.reshape(m, c, T).permute(0, 2, 1).reshape(m, T * c)
    taps = torch.arange(T).repeat_interleave(c)
    chans = torch.arange(c).repeat(T)

    def unpack(r):
        return r.reshape(m, n, p).permute(1, 0, 2).reshape(n, m, *out_sz[3 - nd:])
    return GemmForm(a.contiguous(), b.contiguous(), taps, chans, True, unpack)


def split_bf16(v):
    return V.split_bf16(v)


FORMS = ('bf16x3', 'two_products', 'tap_lo_dropped', 'krange_lo_dropped', 'f32_chain')


def emulate_gemm(g, form='bf16x3', tap=0, krange=None):
    """The GEMM `g` in one of the arithmetics (module docstring), as float64 holding the fp32 result.  krange: (k0, k1) of the K
    indices (forward / data gradient) or pixels (weight gradient) whose cross products 'krange_lo_dropped' loses."""
    if form == 'f32_chain':
        # one step = one MFMA: acc <- fp32(acc + a0 b0 + a1 b1), a single rounding per two products
        a, b = g.a.double(), g.b.double()
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
        K = a.shape[1]
        for k in range(0, K - 1, 2):
            acc = (acc + a[:, k, None] * b[None, k, :] + a[:, k + 1, None] * b[None, k + 1, :]).float().double()
        if K % 2:
            acc = (acc + a[:, K - 1, None] * b[None, K - 1, :]).float().double()
        return g.unpack(acc.double())
    ah, al = split_bf16(g.a)
    bh, bl = split_bf16(g.b)
    hh = ah @ bh
    if form == 'bf16x3':
        out = hh + ah @ bl + al @ bh
    elif form == 'two_products':                     # lo of b (the activation columns) x hi of a lost
        out = hh + al @ bh
    elif form in ('tap_lo_dropped', 'krange_lo_dropped'):
        if g.data_is_b or form == 'krange_lo_dropped':
            K = g.a.shape[1]
            keep = torch.ones(K, dtype=torch.float64)
            if form == 'tap_lo_dropped':
                keep[g.taps == tap] = 0
            else:
                keep[krange[0]:krange[1]] = 0
            out = hh + (ah * keep) @ bl + (al * keep) @ bh
        else:                                        # weight gradient: the result columns of that tap keep hi * hi only
            out = hh + ah @ bl + al @ bh
            sel = g.taps == tap
            out[:, sel] = hh[:, sel]
    else:
        raise ValueError(form)
    return g.unpack(out.float().double())


# ------------------------------------------------------------------------------------------------ dispatch mirror
F32, BF3 = 'f32', 'bf3'
MERGE_MAX_ROWS = 2048
BIAS_REPLICAS = 64
PW_MAXCO = 4


def _cdiv(a, b):
    return -(-a // b)


def _roundup(a, b):
    return _cdiv(a, b) * b


class Phase:
    """One gather-conv launch (ConvPhase in conv_plan.h)."""

    def __init__(self, n, c, m, taps, sub, in_dims, residue, stride):
        self.N, self.C, self.M, self.Msub, self.nmerge = n, c, m, m, 1
        self.taps = list(taps)                       # input offsets (dz, dy, dx), in K order
        self.sub, self.in_dims = tuple(sub), tuple(in_dims)
        self.residues = [tuple(residue)]             # output residue of each row group
        self.group_taps = [list(taps)]               # taps each row group really has
        self.os = tuple(stride)                      # out coord = i * os + residue
        self.bf3 = False

    @property
    def T(self):
        return len(self.taps)

    def finish(self, mode, force=0):
        structural = self.M >= 32 and self.T * self.C >= 32
        self.bf3 = mode == BF3 and structural and force >= 0        # (min_gflop = 0: every structurally eligible phase)
        if self.bf3:
            self.Cp = _roundup(self.C, 8)
            self.Mp = _roundup(self.M, 256) if self.M > 128 else (128 if self.M > 64 else 64)
            self.Kp = _roundup(self.T * self.Cp, 32)
        else:
            self.Cp = 4 if self.C <= 4 else (8 if self.C <= 8 else _roundup(self.C, 16))
            self.Mp = _roundup(self.M, 32)
            self.Kp = _roundup(self.T * self.Cp, 16)
        self.npix = self.N * self.sub[0] * self.sub[1] * self.sub[2]
        return self

    @property
    def tap_inner(self):
        return self.bf3 and self.Cp % 32 == 0 and self.T > 1


def _conv_form(n, c, m, k3, s3, in_dims, out_dims, mode):
    taps = list(itertools.product(range(k3[0]), range(k3[1]), range(k3[2])))
    return [Phase(n, c, m, taps, out_dims, in_dims, (0, 0, 0), (1, 1, 1)).finish(mode)]


def _transposed_form(n, c, m, k3, s3, p3, in_dims, out_dims, mode, allow_merge):
    phases = []
    for res in itertools.product(range(s3[0]), range(s3[1]), range(s3[2])):
        sub = [_cdiv(out_dims[a] - res[a], s3[a]) for a in range(3)]
        per_axis = []
        for a in range(3):
            offs = []
            for r in range(k3[a]):
                num = res[a] + p3[a] - r
                if num % s3[a] == 0:
                    offs.append(num // s3[a] if num >= 0 else -((-num) // s3[a]))
            per_axis.append(offs)
        if min(sub) <= 0:
            continue
        phases.append(Phase(n, c, m, itertools.product(*per_axis), sub, in_dims, res, s3).finish(mode))
    # one arithmetic per operation
    if any(p.bf3 for p in phases):
        all_struct = all(p.M >= 32 and p.T * p.C >= 32 for p in phases)
        for p in phases:
            if p.bf3 != all_struct:
                p.finish(mode, 1 if all_struct else -1)
    count = len(phases)
    if allow_merge and 1 < count <= 8 and m % 32 == 0 and count * m <= MERGE_MAX_ROWS:
        same_grid = all(p.sub == phases[0].sub and p.T > 0 for p in phases)
        same_taps = all(p.taps == phases[0].taps for p in phases)
        union = []
        for p in phases:
            for t in p.taps:
                if t not in union:
                    union.append(t)
        real = sum(p.T for p in phases)
        if same_grid and (same_taps or (len(union) <= 64 and len(union) > 1 and 100 * real >= 50 * count * len(union))):
            g = Phase(n, c, count * m, union, phases[0].sub, in_dims, phases[0].residues[0], s3)
            g.Msub, g.nmerge = m, count
            g.residues = [p.residues[0] for p in phases]
            g.group_taps = [p.taps for p in phases]
            phases = [g.finish(mode)]
    return phases


def _dims3(layer, sz):
    return tuple(sz) if layer.nd == 3 else (1,) + tuple(sz)


def _phases(layer, n, in_sz, op, mode, allow_merge=True):
    """forward-form ('fwd') or data-gradient ('dgrad') phases of build_plan in `mode`"""
    k3, s3, p3 = _geom3(layer)
    i3, o3 = _dims3(layer, in_sz), _dims3(layer, layer.out_size(in_sz))
    if not layer.transposed:
        if op == 'fwd':
            return _conv_form(n, layer.cin, layer.cout, k3, s3, i3, o3, mode)
        return _transposed_form(n, layer.cout, layer.cin, k3, s3, p3, o3, i3, mode, allow_merge)
    if op == 'fwd':
        return _transposed_form(n, layer.cin, layer.cout, k3, s3, p3, i3, o3, mode, allow_merge)
    return _conv_form(n, layer.cout, layer.cin, k3, s3, o3, i3, mode)


def _bf3_uses_pp(p):
    if p.M <= 64:
        return False
    big = _cdiv(p.npix, 128) * _cdiv(p.M, 256) if p.M > 128 else _cdiv(p.npix, 256) * _cdiv(p.M, 128)
    return big >= 128


def _phase_ksplit(p, det):
    if p.npix <= 0 or det:
        return 1
    if p.bf3:
        if _bf3_uses_pp(p):
            return 1
        tiles, nk, tgt, min_steps = _cdiv(p.npix, 128) * _cdiv(p.M, 64), p.Kp // 32, 512, 16
        if tiles >= 192 or nk < 2 * min_steps:
            return 1
    else:
        bm = 128 if p.M > 64 else (64 if p.M > 32 else 32)
        tiles, nk, tgt, min_steps = _cdiv(p.npix, 128) * _cdiv(p.M, bm), p.Kp // 16, 384, 8
        if tiles >= 192 or nk < 4 * min_steps:
            return 1
    return max(1, min(_cdiv(tgt, tiles), nk // min_steps))


def _bf3_wgrad_ksplit(tiles, nsteps, tgt, minst, slots, det):
    if det:
        return 1
    ks = max(1, min(_cdiv(tgt, tiles), _cdiv(nsteps, minst)))
    if tiles * ks < 4 * slots:
        best = 1e30
        for k in range(1, max(nsteps // 12, 1) + 1):
            if tiles * k > 8 * slots:
                break
            sps = _cdiv(nsteps, k)
            if _cdiv(nsteps, sps) != k:
                continue
            cost = _cdiv(tiles * k, slots) * (sps * 1.2 + 12.0)
            if cost < best - 1e-9:
                best, ks = cost, k
    return ks


def _wgrad_uses_bf3(phases, mode):
    if mode != BF3 or not phases:
        return False
    return all(p.Msub >= 32 and p.C >= 32 and not (p.Msub % 16 != 0 and p.nmerge > 1) for p in phases)


def pw_applicable(layer, in_sz):
    s = math.prod(in_sz)
    return (not layer.transposed and layer.cout <= PW_MAXCO and layer.cin <= 1024 and layer.k == 1 and layer.stride == 1
            and layer.pad == 0 and s % 4 == 0 and s >= 1024)


def _vox_takes(layer, n, in_sz, op, mode, det):
    if layer.kind != 'conv3d' or (layer.k, layer.stride, layer.pad) != (3, 1, 1):
        return False
    return V.vox_plan(layer.cin, layer.cout, n, tuple(in_sz), op, ACT_NONE, 'bf3' if mode == BF3 else 'f32', det) is not None


def _bf3_ws_bytes(n, c, s):
    return n * s * _roundup(c, 8) * 4 + 16 + BIAS_REPLICAS * _roundup(c, 8) * 4


def conv_plan(layer, n, in_sz, op, mode, det=False):
    """What the library launches for `op` ('fwd', 'dgrad', 'wgrad') of `layer` at batch n and input size in_sz in `mode` (F32 /
    BF3) with the work threshold at 0; None where conv_pw.hip or the voxel kernels take the shape.  dict:
      family, variant         muvo_conv_kernel_family / muvo_conv_kernel_variant
      phases                  list of dict(M, Msub, nmerge, C, Cp, Mp, Kp, T, npix, sub, residues, os, bf3, tap_inner, tile (BM, BN),
                              kernel, ksplit, steps (K steps per range))
      finish                  forward / data gradient: a bias / activation finishing pass follows split-K when there is any
      unpack                  weight gradient: 'fp32', 'tiled' or 'elementwise' per phase
      reach                   names of the instantiations and code paths this operation runs (tests/test_conv_bars.py)"""
    if pw_applicable(layer, in_sz) or _vox_takes(layer, n, in_sz, op, mode, det):
        return None
    if op == 'wgrad':
        return _wgrad_plan(layer, n, in_sz, mode, det)
    phases = _phases(layer, n, in_sz, op, mode)
    fam = 1 if any(p.bf3 for p in phases) else 0
    ks = [_phase_ksplit(p, det) for p in phases]
    use = any(k > 1 for k in ks)
    out, reach = [], set()
    for p, k in zip(phases, ks):
        k = (k if k > 1 else 2) if use else 1
        if p.bf3:
            nk = p.Kp // 32
            if k > 1 or not _bf3_uses_pp(p):
                tile, kern = (64, 128), 'conv_bf3_kernel<64,128,1,4,4,2>'
            elif p.M > 128:
                tile, kern = (256, 128), 'conv_bf3_kernel<256,128,4,2,4,3>'
            else:
                tile, kern = (128, 256), 'conv_bf3_kernel<128,256,2,4,4,3>'
            reach.add('bf3 K order: ' + ('tap inner' if p.tap_inner else 'taps outermost'))
            reach.add('bf3 ' + ('merged' if p.nmerge > 1 else 'plain') + ' phase')
        else:
            nk = p.Kp // 16
            bm = 128 if p.M > 64 else (64 if p.M > 32 else 32)
            tile, kern = (bm, 128), f'conv_fwd_kernel<{bm},128,run{4 if p.Cp == 4 else 8}>'
        if p.npix > 0:
            reach.add(kern + (' split-K' if k > 1 else ''))
        out.append(dict(M=p.M, Msub=p.Msub, nmerge=p.nmerge, C=p.C, Cp=p.Cp, Mp=p.Mp, Kp=p.Kp, T=p.T, npix=p.npix, sub=p.sub,
                        residues=p.residues, os=p.os, bf3=p.bf3, tap_inner=p.tap_inner, tile=tile, kernel=kern, ksplit=k,
                        steps=_cdiv(nk, k), N=p.N))
    if use:
        reach.add('bias_act_kernel')
    if fam == 1:
        reach.add('nchw_split_nhwc')
    return dict(family=fam, variant=1 if fam == 1 and _bf3_uses_pp(phases[0]) else 0, phases=out, finish=use, reach=reach,
                pack=sum(p.Kp * p.Mp for p in phases),
                ws=_bf3_ws_bytes(n, phases[0].C, math.prod(phases[0].in_dims)) if fam == 1 else 0)


def _wgrad_plan(layer, n, in_sz, mode, det):
    pf = _phases(layer, n, in_sz, 'fwd', F32, allow_merge=False)
    bf3 = _wgrad_uses_bf3(pf, mode)
    phases = pf
    if bf3:
        pm = _phases(layer, n, in_sz, 'fwd', F32, allow_merge=True)
        if _wgrad_uses_bf3(pm, mode):
            phases = pm
    out, reach, unpack = [], set(), []
    for p in phases:
        if p.npix <= 0 or p.T == 0:
            continue
        nsteps = _cdiv(p.npix, 32)
        if bf3:
            pp = p.M > 128 or (p.M > 64 and p.C > 64)
            if p.M > 128:
                tile, kern = (256, 128), 'conv_bf3_wgrad_pp_kernel<256,128>'
            elif p.M > 64:
                tile, kern = ((128, 256), 'conv_bf3_wgrad_pp_kernel<128,256>') if p.C > 64 else ((128, 128), 'conv_bf3_wgrad_kernel<128,128,2,2,2>')
            elif p.M <= 32 and p.C <= 64:
                tile, kern = (32, 64), 'conv_bf3_wgrad_kernel<32,64,1,2,2>'
            elif p.C > 128:
                tile, kern = (64, 256), 'conv_bf3_wgrad_kernel<64,256,1,4,2>'
            elif p.C > 64:
                tile, kern = (64, 128), 'conv_bf3_wgrad_kernel<64,128,1,2,2>'
            else:
                tile, kern = (64, 64), 'conv_bf3_wgrad_kernel<64,64,1,2,2>'
            lds = 3 * 2 * 32 * (tile[0] // 8 + tile[1] // 8) * 16
            slots = 256 if pp else 256 * (160 * 1024 // lds)
            tiles = _cdiv(p.C, tile[1]) * p.T * _cdiv(p.M, tile[0])
            ks = _bf3_wgrad_ksplit(tiles, nsteps, 2048, 32, slots, det)
            sps = _cdiv(nsteps, ks)
            ks = _cdiv(nsteps, sps)
            up = 'tiled' if p.M * p.C * p.T >= 4096 else 'elementwise'
            reach.add('bf3_unpack_wgrad_tiled_kernel' if up == 'tiled' else 'bf3_unpack_wgrad_kernel')
        else:
            bn = 128 if p.M > 64 else (64 if p.M > 32 else 32)
            gx, gy = _cdiv(p.Kp, 128), _cdiv(p.M, bn)
            ks = min(_cdiv(2048, gx * gy), _cdiv(nsteps, 4))
            if ks < 1 or det:
                ks = 1
            sps = _cdiv(nsteps, ks)
            ks = _cdiv(nsteps, sps)
            b3 = mode == BF3 and 2e-9 * p.M * p.npix * p.T * p.C >= 2.0
            tile, kern = (128, bn), f'conv_wgrad_kernel<128,{bn},{"true" if b3 else "false"}>'
            up = 'fp32'
            reach.add('unpack_wgrad_kernel')
        reach.add(kern)
        unpack.append(up)
        out.append(dict(M=p.M, Msub=p.Msub, nmerge=p.nmerge, C=p.C, T=p.T, npix=p.npix, tile=tile, kernel=kern, ksplit=ks, steps=sps,
                        bf3=bf3))
    i3, o3 = _dims3(layer, in_sz), _dims3(layer, layer.out_size(in_sz))
    return dict(family=1 if bf3 else 0, variant=1 if bf3 and (phases[0].M > 128 or (phases[0].M > 64 and phases[0].C > 64)) else 0,
                phases=out, unpack=unpack, reach=reach, finish=False,
                pack=sum(p.Kp * p.Mp for p in pf),
                ws=(_bf3_ws_bytes(n, layer.cin, math.prod(i3)), _bf3_ws_bytes(n, layer.cout, math.prod(o3))) if bf3 else (0, 0))


def layer_answers(layer, n, in_sz, mode, det=False):
    """The mirror's version of what ops.ConvPlan asks the library: families, variants, pack sizes, the four workspace sizes."""
    f, d, w = (conv_plan(layer, n, in_sz, op, mode, det) for op in ('fwd', 'dgrad', 'wgrad'))
    if f is None:
        return None
    return dict(family=(f['family'], d['family'], w['family']), variant=(f['variant'], d['variant'], w['variant']),
                pack_fwd=max(f['pack'], w['pack']), pack_dgrad=d['pack'], ws=(f['ws'], d['ws']) + tuple(w['ws']))


def fused_dy_kernel(layer, n, in_sz, mode, need_dx=True, need_dw=True):
    """Which backward preamble ops.ConvFn runs: 'v4' / 'scalar' (muvo_conv_prepare_dy on nchw_split_nhwc_v4_kernel / the 4-byte
    kernel) when both gradient directions are family 1 and both are wanted, else None (un-fused: muvo_act_bwd, the kernels' own
    split passes, bias_grad_kernel)."""
    d, w = conv_plan(layer, n, in_sz, 'dgrad', mode), conv_plan(layer, n, in_sz, 'wgrad', mode)
    if d is None or not (d['family'] == 1 and w['family'] == 1 and need_dx and need_dw):
        return None
    s = math.prod(layer.out_size(in_sz))
    return 'v4' if s % 4 == 0 and s >= 1024 else 'scalar'


def locate(index, plan):
    """Where the launch computes output element `index` = (n, channel, [z,] y, x) of a forward / data-gradient plan: phase, row
    group, m-tile, pixel tile, sample and the number of K ranges that add into it."""
    if plan is None or not plan['phases'] or 'os' not in plan['phases'][0]:
        return f'element {tuple(index)}'
    n, c = index[0], index[1]
    pos = tuple(index[2:]) if len(index) == 5 else (0,) + tuple(index[2:])
    for i, p in enumerate(plan['phases']):
        res = tuple(pos[a] % p['os'][a] for a in range(3))
        if res not in p['residues']:
            continue
        grp = p['residues'].index(res)
        sub = p['sub']
        q = [pos[a] // p['os'][a] for a in range(3)]
        pix = ((n * sub[0] + q[0]) * sub[1] + q[1]) * sub[2] + q[2]
        m = grp * p['Msub'] + c
        bm, bn = p['tile']
        ks = f', {p["ksplit"]} K ranges of {p["steps"]} steps' if p['ksplit'] > 1 else ''
        return (f'element {tuple(index)}: phase {i} of {len(plan["phases"])} ({p["kernel"]}), row group {grp} (row {m}), m-tile {m // bm} '
                f'(row {m % bm} of {bm}), pixel {pix} = tile {pix // bn} column {pix % bn}, sample {n}{ks}')
    return f'element {tuple(index)}: in no phase (an output position without a tap)'
