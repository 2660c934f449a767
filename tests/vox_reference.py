"""Plain float64 references, a normalised error metric and CPU emulations of the bf16x3 arithmetic for the 3x3x3 voxel
convolutions (muvo_amd/csrc/conv_vox.hip).  Helpers only: no fixtures, no tests.

The metric.  For every result element, e = |got - ref64| / sqrt((a^2) * (b^2)), where the denominator is the same operation
run on the squared operands (forward: x^2 conv w^2; data gradient: dy^2 with w^2 through the adjoint; weight gradient: x^2
against dy^2).  It is the scale of the rounding error of that one element, whatever its cancellation, so an error confined
to one face, one segment border or one tail tile shows up at full size in max(e) instead of being diluted by the rest of
the tensor as in an elementwise rtol against the tensor's largest value.  Next to it: rms(got - ref) / rms(ref).

The emulations.  conv_vox.hip splits each fp32 operand v into hi = bf16(v) and lo = bf16(v - hi), both rounded to nearest
even (vox_split2: v_cvt_pk_bf16_f32; vox_bf3_ps_pack_kernel: the same rounding in integer form), and sums
hi*hi + hi*lo + lo*hi on the matrix cores.  `emulate` forms these products in float64 on the CPU; its degraded forms drop
one cross product everywhere ('two_products': data lo * weight hi) or both cross products of one tap ('tap_lo_dropped'),
which is what a kernel that loses a product on one halo plane or one tap looks like.
"""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_ELU = 0, 1, 2, 3
SLOPE = 0.2

# Bars of the normalised metric: (rms(got - ref) / rms(ref), max(e)).  The bf16x3 arithmetic measures a relative rms error of
# 4.5-4.9e-6 on these layers.  The fp32 4x4x1 kernels add the 27 * Cin products of an output one after the other in fp32:
# with 16 reduction channels that chain alone gives rms 3.5e-7 and max(e) 3.5e-6 (emulated on the CPU, the same as measured),
# so the fp32 bar has no margin of 2 there and must not be tightened.
BARS = {'bf3': (1.5e-5, 6e-5), 'f32': (5e-7, 5e-6)}
MOMENTS_BAR = 1e-6          # |sum(y) - sum64(y)| <= MOMENTS_BAR * sum|y|, sum of squares likewise


# ------------------------------------------------------------------------------------------------ operations (float64)
def fwd_op(x, w):
    return F.conv3d(x, w, padding=1)


def dgrad_op(dy, w, x_shape):
    return torch.nn.grad.conv3d_input(x_shape, w, dy, padding=1)


def wgrad_op(x, dy, w_shape):
    return torch.nn.grad.conv3d_weight(x, w_shape, dy, padding=1)


def _d(t):
    return t.detach().cpu().double()


def act64(y, act, slope=SLOPE):
    if act == ACT_RELU:
        return F.relu(y)
    if act == ACT_LEAKY:
        return F.leaky_relu(y, slope)
    if act == ACT_ELU:
        return F.elu(y)
    return y


def ref_forward(x, w, b=None, act=ACT_NONE, slope=SLOPE):
    """(reference, denominator) of act(conv3d(x, w) + b).  The activations used here have |derivative| <= 1, so the
    pre-activation scale bounds the error after them."""
    x, w = _d(x), _d(w)
    y = fwd_op(x, w)
    if b is not None:
        y = y + _d(b).view(1, -1, 1, 1, 1)
    return act64(y, act, slope), fwd_op(x * x, w * w).sqrt()


def ref_dgrad(dy, w, x_shape):
    dy, w = _d(dy), _d(w)
    return dgrad_op(dy, w, x_shape), dgrad_op(dy * dy, w * w, x_shape).sqrt()


def ref_wgrad(x, dy, w_shape):
    x, dy = _d(x), _d(dy)
    return wgrad_op(x, dy, w_shape), wgrad_op(x * x, dy * dy, w_shape).sqrt()


def ref_bgrad(dy):
    dy = _d(dy)
    return dy.sum(dim=(0, 2, 3, 4)), (dy * dy).sum(dim=(0, 2, 3, 4)).sqrt()


def affine_input(raw, aff):
    """The operand the affine-staging kernels convolve: scale * raw + shift per (n, input channel), in fp32 as the kernels
    form it (a product, then a sum: the build contracts no multiply-add).  Zero padding is applied to this tensor, i.e.
    AFTER the map."""
    raw, aff = raw.detach().cpu().float(), aff.detach().cpu().float()
    return raw * aff[:, :, 0, None, None, None] + aff[:, :, 1, None, None, None]


def moments64(y):
    """Per-(n, c) (sum y, sum y^2) in float64 of the kernel's own fp32 output, and the scale sum |y| (sum y^2) of each."""
    y = _d(y)
    ref = torch.stack([y.sum(dim=(2, 3, 4)), (y * y).sum(dim=(2, 3, 4))], dim=-1)
    scale = torch.stack([y.abs().sum(dim=(2, 3, 4)), (y * y).sum(dim=(2, 3, 4))], dim=-1)
    return ref, scale


# ------------------------------------------------------------------------------------------------ metric
def error_stats(got, ref, den):
    """Normalised error of `got` against the float64 reference: dict(max_e, rms, index of the worst element)."""
    g = _d(got)
    assert g.shape == ref.shape, f'shape {tuple(g.shape)} vs {tuple(ref.shape)}'
    diff = (g - ref).abs()
    e = diff / den.clamp_min(1e-300)
    i = int(e.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e.shape))
    rms_ref = float(ref.pow(2).mean().sqrt())
    rms = float(diff.pow(2).mean().sqrt()) / rms_ref if rms_ref > 0 else float(diff.pow(2).mean().sqrt())
    return {'max_e': float(e.reshape(-1)[i]), 'rms': rms, 'index': idx}


def within(stats, bar):
    rms_bar, e_bar = bar
    return stats['rms'] <= rms_bar and stats['max_e'] <= e_bar


def excess(stats, bar):
    """How far past the bar: max(rms / rms bar, max(e) / max(e) bar) (<= 1 passes)."""
    return max(stats['rms'] / bar[0], stats['max_e'] / bar[1])


# ------------------------------------------------------------------------------------------------ bf16x3 emulation
def split_bf16(v):
    """hi = bf16(v), lo = bf16(v - hi), round to nearest even, as float64 (v - hi is exact in fp32)."""
    v = v.detach().cpu().float()
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


FORMS = ('bf16x3', 'two_products', 'tap_lo_dropped')


def emulate(op, a, b, form='bf16x3', tap=(1, 1, 1), per_tap=False):
    """op(a, b) of two fp32 operands in the kernels' split arithmetic, evaluated in float64 and rounded to the fp32 result.

    op: bilinear in (a, b); a is the data operand (x or dy), b the weight (forward / data gradient: a [Cout][Cin][3][3][3]
    tensor) or dy (weight gradient, per_tap: the result is per tap).  form:
      'bf16x3'          hi*hi + hi*lo + lo*hi (the kernels' arithmetic)
      'two_products'    hi*hi + hi*lo: the data operand's lo times the other's hi is lost everywhere
      'tap_lo_dropped'  bf16x3 except that tap `tap` (kz index order of the weight: (kx, ky, kz)) keeps hi*hi only."""
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    hh, hl = op(ah, bh), op(ah, bl)
    if form == 'bf16x3':
        out = hh + hl + op(al, bh)
    elif form == 'two_products':
        out = hh + hl
    elif form == 'tap_lo_dropped':
        kx, ky, kz = tap
        if per_tap:                                          # weight gradient: the result is per tap
            out = hh + hl + op(al, bh)
            out[:, :, kx, ky, kz] = hh[:, :, kx, ky, kz]
        else:                                                # weight operand: zero its tap in the cross products
            m = torch.ones(3, 3, 3, dtype=torch.float64)
            m[kx, ky, kz] = 0
            out = hh + op(ah, bl * m) + op(al, bh * m)
    else:
        raise ValueError(form)
    return out.float().double()


def emulate_forward(x, w, form='bf16x3', tap=(1, 1, 1)):
    return emulate(fwd_op, x, w, form, tap)


def emulate_dgrad(dy, w, x_shape, form='bf16x3', tap=(1, 1, 1)):
    return emulate(lambda a, b: dgrad_op(a, b, x_shape), dy, w, form, tap)


def emulate_wgrad(x, dy, w_shape, form='bf16x3', tap=(1, 1, 1)):
    return emulate(lambda a, b: wgrad_op(a, b, w_shape), x, dy, form, tap, per_tap=True)


# ------------------------------------------------------------------------------------------------ dispatch mirror
PS_TY = 8          # output rows per plane-streaming workgroup (VOX_PS_TY in conv_vox.hip)
WGPS_SW = 4        # (VOX_WGPS_SW in conv_vox.hip) staging waves of vox_bf3_wgrad_ps_kernel with 16 input / <= 8 produced channels
BLOCKS_TARGET = 128


def _cdiv(a, b):
    return -(-a // b)


def _xseg(n, x, ytiles, factor=1):
    """x-segment length of a bf16x3 voxel launch (vox_xseg in conv_vox.hip): x is halved until the grid has
    BLOCKS_TARGET workgroups or a segment would drop to 12 planes or fewer."""
    xseg = x
    while n * ytiles * _cdiv(x, xseg) * factor < BLOCKS_TARGET and xseg > 12:
        xseg = _cdiv(xseg, 2)
    return xseg


def _b(v):
    return 'true' if v else 'false'


def vox_plan(cin, cout, n, shape, op, act=ACT_NONE, mode='bf3', det=False):
    """The conv_vox.hip kernels a 3x3x3 / stride 1 / pad 1 convolution runs for `op` ('fwd', 'dgrad', 'wgrad') with
    muvo_conv_set_bf16x3_min_gflop(0) in bf16x3 mode (and MUVO_VOX_BLOCKS / MUVO_VOX_WGRAD_BLOCKS unset), restated from
    vox_conv_dispatch / vox_wgrad and the applicability rules in conv_vox.hip / conv_gemm.hip.

    Returns None when the voxel kernels do not serve the shape, else dict(family (muvo_conv_kernel_family: 4 bf16x3, 2 fp32),
    kernels (instantiations in launch order, written as rocprofv3 prints them), ty (output rows per y tile), xseg (x planes per
    segment / per x group))."""
    x, y, z = shape
    geom = z in (32, 64) and cin % 4 == 0 and cout % 4 == 0 and x * y * z * max(cin, cout) * 4 < 0x7fffff00
    geom16 = (z == 16 or geom) and cin % 4 == 0 and cout % 4 == 0 and x * y * z * max(cin, cout) * 4 < 0x7fffff00
    if op in ('fwd', 'dgrad'):
        red, cp = (cin, cout) if op == 'fwd' else (cout, cin)
        a = act if op == 'fwd' else ACT_NONE
        ps = red in (16, 32, 64) and cp in (8, 16, 32)
        if geom16 and (z == 16 or red == 64):
            bf3_ok = ps
        else:
            bf3_ok = geom and red in (8, 16, 32) and cp in (8, 16, 32)
        fp32_ok = geom and cp in (8, 16) and 27 * cin * cout * 4 <= 64 * 1024
        if mode == 'bf3' and bf3_ok:
            if ps:
                npass = red // 16
                gen = [p > 0 or (npass == 1 and a > ACT_LEAKY) for p in range(npass)]
                names = [f'vox_bf3_ps_kernel<{z}, {PS_TY}, {_b(cp <= 8)}, {_b(g)}>' for g in gen]
                ty = PS_TY
            elif red == 8 and cp == 8:
                ty = 16
                names = [f'vox_bf3_2row_kernel<{z}, 8, {_b(a > ACT_LEAKY)}>']
            else:                                    # red 8, 16 or 32 produced channels
                ty = 8
                names = [f'vox_bf3_kernel<8, {z}, 8, {_b(a > ACT_LEAKY)}>']
            return {'family': 4, 'kernels': names, 'ty': ty, 'xseg': _xseg(n, x, _cdiv(y, ty))}
        if fp32_ok:
            cq, ty = (2, 6) if cp == 8 else (4, 4)
            return {'family': 2, 'kernels': [f'vox_conv_kernel<{cq}, {ty}, {z}>'], 'ty': ty, 'xseg': 64 // z}
        return None
    # weight gradient
    applicable = geom and cout % 8 == 0 and cin % 8 == 0 and cout <= 32 and cin <= 64
    ps_only = geom16 and (z == 16 or cout == 32) and cin % 16 == 0 and cin <= 64 and cout in (8, 16, 32)
    bf3_ok = ps_only or (applicable and (cin == 8 or cin % 16 == 0) and cout in (8, 16))
    if mode == 'bf3' and bf3_ok and not det:
        co8 = cout <= 8
        zh = z // 32 if z >= 32 else 1
        if z == 16 or cin != 8 or co8:               # plane-streaming
            ci = 8 if cin == 8 else 16
            sw = WGPS_SW if (ci == 16 and co8) else 0
            wrows = 8 // zh * (1 if z >= 32 else 32 // z)
            name = f'vox_bf3_wgrad_ps_kernel<{z}, {ci}, {_b(co8)}, {sw}>'
            factor = (cin // ci) * _cdiv(cout, 16)
        else:                                        # 8 input -> 16 produced channels
            wrows = 8 // zh
            name = f'vox_bf3_wgrad_kernel<{z}, 8, false>'
            factor = cin // 8
        return {'family': 4, 'kernels': [name], 'ty': wrows, 'xseg': _xseg(n, x, _cdiv(y, wrows), factor)}
    if applicable:
        r4 = cin % 16 == 0
        tyb = 4 if z == 64 else 8
        name = f'vox_wgrad_kernel<4, 2, {z}, {tyb}>' if r4 else f'vox_wgrad_kernel<2, 1, {z}, {tyb}>'
        return {'family': 2, 'kernels': [name], 'ty': tyb, 'xseg': x}
    return None


def short_name(kernel):
    """'vox_bf3_ps_kernel<32, 8, true, false>' -> 'ps32co8', for test ids."""
    base, args = kernel.split('<')
    args = [s.strip() for s in args.rstrip('>').split(',')]
    if base == 'vox_bf3_ps_kernel':
        return f'ps{args[0]}' + ('co8' if args[2] == 'true' else '')
    if base == 'vox_bf3_2row_kernel':
        return f'2row{args[0]}'
    if base == 'vox_bf3_kernel':
        return f'bf3k8z{args[1]}'
    if base == 'vox_bf3_wgrad_ps_kernel':
        return f'wps{args[0]}ci{args[1]}' + ('co8' if args[2] == 'true' else '')
    if base == 'vox_bf3_wgrad_kernel':
        return f'wbf3z{args[0]}ci{args[1]}'
    if base == 'vox_conv_kernel':
        return f'f32cq{args[0]}z{args[2]}'
    if base == 'vox_wgrad_kernel':
        return f'f32w{args[0]}z{args[2]}'
    return base


def locate(index, plan):
    """'(n, c, x, y, z) segment s y-tile t' of a result element of the forward / data gradient (plan: vox_plan of that op)."""
    n, c, x, y, z = index
    if plan is None:
        return f'(n, c, x, y, z) = {index}'
    return f'(n, c, x, y, z) = {index}, x segment {x // plan["xseg"]} (of {plan["xseg"]} planes), y tile {y // plan["ty"]} (of {plan["ty"]} rows)'
