"""Plain float64 references, the normalised error metric, the case lists and a restatement of the launch arithmetic for the
normalisation kernels (muvo_amd/csrc/norm.hip): train-mode BatchNorm, AdaIN3d (plain, from moments, lazy affine, fused with the
1x1x1 head) and the fused add + dropout + LayerNorm.  Helpers only: no fixtures, no tests.  tests/test_norm_reference.py (CPU) and
tests/test_norm_kernels_gpu.py (GPU) share everything here, so the bars the GPU test applies are the ones the CPU test proves to
reject planted errors.  The metric (error_stats), check_expect and the seeded generator are those of tests/loss_reference.py.

The references.  Every function takes `dtype` (default float64); evaluated with dtype=float32 it is "the float32 CPU evaluation"
the bars come from.  Statistics are two-pass.  Gradients come from autograd.

ReLU masks are the subject's.  The gradient of a BatchNorm case with ReLU is evaluated with the mask read off the SUBJECT's own
forward output (y > 0; res_mode 2: y - res > 0), so an element whose sign differs between the subject's forward and backward is
an error of order one.  mask_facts() says how far that mask is from the float64 one: the tests cap the disagreeing fraction at
MASK_CAP = 1e-4 and allow disagreement only where |pre-activation| <= MASK_BAND = 1e-5 x max |pre-activation|.

The metric.  e = |got - ref64| / den, den = max |ref| of the tensor; for save_mean / running_mean den = max(|mean|, std) of the
group.  A reference of exactly 0 demands exactly 0.  Parameter gradients are compared as the accumulated total (pre-filled value
+ gradient): a kernel that overwrites shows at once.

The bars.  Per family, 4 x the largest e of the float32 CPU evaluation over the family's cases (`python tests/norm_reference.py`
prints the table; the offset cases are left out of it, see below).  The factor 4 is for what legitimately differs between that
evaluation and a kernel: summation order, and coefficients handed between kernels as float32.

    family        float32 evaluation, max(e)    bar
    bn_y          1.81e-07                      7.24e-07
    bn_stat       1.39e-07                      5.56e-07
    bn_run        3.63e-07                      1.45e-06
    bn_dx         8.02e-07                      3.21e-06
    bn_dparam     2.08e-07                      8.32e-07
    bn_dres       0.00e+00                      0.00e+00   (dz is dy or 0: exact)
    adain_y       1.77e-07                      7.08e-07
    adain_stat    1.38e-07                      5.52e-07
    adain_dx      8.49e-07                      3.40e-06
    adain_dstyle  2.90e-07                      1.16e-06
    head_logits   3.31e-07                      1.32e-06
    head_dx       9.83e-07                      3.93e-06
    head_dparam   2.86e-06                      1.14e-05
    ln_y          1.49e-07                      5.96e-07
    ln_dx         1.75e-07                      7.00e-07
    ln_da         1.87e-07                      7.48e-07
    ln_dparam     2.22e-07                      8.88e-07

Offset cases (group mean / std = OFFSET = 16) are held to the family bar x (1 + 16^2): the kernels form the variance in one pass
as E[x^2] - m^2 (the unit's header comment), whose condition number is 1 + (mean / std)^2.  Derived, not measured.

Inputs.  randn * 2 + 0.5 with sentinels of magnitude 50 (50 x uniform(0.8, 1.2), all positive, so a dropped float4 moves the sum
by about 200) on the first and last four elements of every row and on the four elements either side of every statistics-chunk
boundary path() computes.  Rows shorter than 16 carry no sentinels, and groups of 2..15 elements are shifted to mean / std = 0.5:
a handful of samples cannot average an unlucky draw out, and those cases are about buffers, not conditioning.

path() restates the launchers of norm.hip; every case id is built from it and every case's `expect` is checked against it."""
import torch

from loss_reference import _gen, check_expect, error_stats, f32r, failures, scale_of, within      # noqa: F401 (re-exported)

MEASURED = {'bn_y': 1.81e-7, 'bn_stat': 1.39e-7, 'bn_run': 3.63e-7, 'bn_dx': 8.02e-7, 'bn_dparam': 2.08e-7, 'bn_dres': 0.0,
            'adain_y': 1.77e-7, 'adain_stat': 1.38e-7, 'adain_dx': 8.49e-7, 'adain_dstyle': 2.90e-7, 'head_logits': 3.31e-7,
            'head_dx': 9.83e-7, 'head_dparam': 2.86e-6, 'ln_y': 1.49e-7, 'ln_dx': 1.75e-7, 'ln_da': 1.87e-7, 'ln_dparam': 2.22e-7}
BARS = {k: 4 * v for k, v in MEASURED.items()}
OFFSET = 16.0
OFFSET_FACTOR = 1 + OFFSET ** 2
SPLIT_RESIDUE = 2.0 ** -16           # what a two-term bf16 split (8 + 8 significand bits) leaves of a value
MASK_CAP, MASK_BAND = 1e-4, 1e-5
BN_EPS, BN_MOMENTUM, ADAIN_EPS, LN_EPS, SLOPE = f32r(1e-5), f32r(0.1), f32r(1e-8), f32r(1e-5), f32r(0.2)
F64 = torch.float64


# ================================================================================================ launch arithmetic
def _cdiv(a, b):
    return -(-a // b)


def _ew(total):
    """ew_grid: blocks of a grid-stride kernel and the most passes a thread makes"""
    blocks = max(min(_cdiv(total, 256), 4096), 1)
    return blocks, _cdiv(total, blocks * 256)


def _stats(cnt, cap, det, vec):
    """a statistics launch over groups of cnt elements: workgroups per group (one per 4096 elements, capped; one in
    deterministic mode), elements per workgroup rounded up to a multiple of four, passes of a thread, and whether a thread reaches
    the periodic flush of its float32 partial sums into the float64 ones (every 4 vec4 / 64 scalar passes)"""
    want = _cdiv(cnt, 4096)
    chunks = 1 if det else min(want, cap)
    per = (_cdiv(cnt, chunks) + 3) & ~3
    passes = _cdiv(min(per, cnt), 4096 if vec else 256)
    return {'chunks': chunks, 'capped': not det and want > cap, 'per': per, 'stat': 'vec4' if vec else 'scalar',
            'stat_passes': passes, 'flush': passes >= (4 if vec else 64)}


def path(kind, N, C, S, det=False, mis=(), bcast=False):
    """What norm.hip launches.  mis: the tensors that do NOT start on a 16-byte boundary ('x', 'res', 'dy').  kind:
      'bn_fwd' / 'bn_bwd' (N, C, S): the statistics launch (chunks, capped, per, stat, stat_passes, flush), apply ('vec': one
                  (n, c) row per workgroup row, float4; 'quad': grid-stride float4, forward only; 'scalar'), apply_passes
      'adain_fwd' / 'adain_bwd' (N, C, S; bcast: the input is one (C, S) tensor for all N): the same keys, launches (statistics
                  launches: N for a broadcast input), grow (the per-stream accumulator of 65536 doubles is re-allocated)
      'head_fwd' / 'head_bwd' (N, C = 8, S): gx, capped (the cap of 128 workgroups per frame binds), passes; backward: of the
                  statistics and the apply kernel alike (gx is 1 for the statistics in deterministic mode)
      'ln' (N rows, S = E): blocks, rows_per_block (16; rows in deterministic mode), tail (rows % rows_per_block), slots (64-lane
                  slots per row), trips (most four-row trips of a wave)"""
    al = lambda *names: not any(n in mis for n in names)      # noqa: E731
    v4 = S % 4 == 0
    if kind == 'bn_fwd':
        p = _stats(N * S, 256, det, v4 and al('x'))
        if v4 and S >= 1024 and N * C <= 65535 and al('x', 'res'):
            gx = min(_cdiv(S // 4, 1024), 64)
            p.update(apply='vec', apply_passes=_cdiv(S // 4, gx * 256))
        elif v4 and al('x', 'res'):
            p.update(apply='quad', apply_passes=_ew(N * C * S // 4)[1])
        else:
            p.update(apply='scalar', apply_passes=_ew(N * C * S)[1])
        return p
    if kind == 'bn_bwd':
        p = _stats(N * S, 256, det, v4 and al('x', 'dy'))
        if v4 and S >= 1024 and N * C <= 65535 and al('x', 'dy'):
            gx = min(_cdiv(S // 4, 1024), 64)
            p.update(apply='vec', apply_passes=_cdiv(S // 4, gx * 256))
        else:
            p.update(apply='scalar', apply_passes=_ew(N * C * S)[1])
        return p
    if kind in ('adain_fwd', 'adain_bwd'):
        names = ('x',) if kind == 'adain_fwd' else ('x', 'dy')
        p = _stats(S, 128, det, v4 and al(*names))
        if v4 and S >= 1024 and N * C <= 65535 and al(*names):
            p.update(apply='vec', apply_passes=1)            # the grid is sized for one pass of four float4 per lane
        else:
            p.update(apply='scalar', apply_passes=_ew(N * C * S)[1])
        p.update(launches=N if bcast else 1, grow=2 * N * C > 65536)
        return p
    if kind in ('head_fwd', 'head_bwd'):
        assert C == 8 and v4 and S >= 1024, 'muvo_adain_head_supported'
        want = _cdiv(S // 4, 1024)
        gx = min(want, 128)
        p = {'gx': gx, 'capped': want > 128, 'passes': _cdiv(S // 4, gx * 256)}
        if kind == 'head_bwd' and det:
            p.update(stat_gx=1)
        return p
    if kind == 'ln':
        rpb = N if det else 16
        return {'blocks': _cdiv(N, rpb), 'rows_per_block': rpb, 'tail': N % rpb, 'slots': _cdiv(S, 64), 'trips': _cdiv(rpb, 16)}
    raise ValueError(kind)


def boundaries(cnt, per):
    """the statistics-chunk boundaries inside a group of cnt elements"""
    return list(range(per, cnt, per))


# ================================================================================================ inputs
def _sentinel_index(cnt, S, per):
    idx = []
    if S >= 16:
        rows = torch.arange(cnt // S) * S
        for d in range(4):
            idx += [rows + d, rows + S - 1 - d]
    for b in boundaries(cnt, per):
        idx.append(torch.arange(max(b - 4, 0), min(b + 4, cnt)))
    return torch.unique(torch.cat(idx)) if idx else torch.zeros(0, dtype=torch.long)


def stat_input(g, groups, cnt, S, per, offset=False, base=None):
    """(groups, cnt) float32: randn * 2 + 0.5 (or `base`) with the sentinels of a group made of rows of S elements whose statistics
    workgroups take `per` elements each; offset: every group shifted to mean / std = OFFSET"""
    x = torch.randn(groups, cnt, generator=g) * 2 + 0.5 if base is None else base
    idx = _sentinel_index(cnt, S, per)
    if idx.numel():
        x[:, idx] = 50.0 * (0.8 + 0.4 * torch.rand(groups, idx.numel(), generator=g))
    if offset or 1 < cnt < 16:
        xd = x.double()
        m, sd = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True).sqrt()
        x = (xd - m + (OFFSET if offset else 0.5) * sd).float()
    return x


def _rows(t, N, C, S):
    """(C, N * S) in a BatchNorm channel's order -> (N, C, S)"""
    return t.view(C, N, S).transpose(0, 1).contiguous()


# ------------------------------------------------------------------------------------------------ BatchNorm
MODES = [(0, False), (0, True), (1, True), (2, True)]          # (res_mode, relu)


def bcase(N, C, S, res_mode, relu, offset=False, mis=None, det=False, **expect):
    return dict(N=N, C=C, S=S, res_mode=res_mode, relu=relu, offset=offset, mis=mis, det=det, expect=expect)


def _bn_cases():
    out = []
    for rm, relu in MODES:
        out += [bcase(5, 24, 126, rm, relu, chunks=1, stat='scalar', apply='scalar'),
                bcase(3, 10, 260, rm, relu, chunks=1, stat='vec4', fwd_apply='quad', bwd_apply='scalar'),
                bcase(3, 10, 1280, rm, relu, chunks=1, stat='vec4', apply='vec'),
                bcase(4, 6, 2080, rm, relu, chunks=3, stat='vec4', apply='vec', per=2776),
                bcase(3, 5, 2731, rm, relu, chunks=3, stat='scalar', apply='scalar', per=2732),
                bcase(1, 7, 1, rm, relu, chunks=1, per=4),
                bcase(4, 6, 2080, rm, relu, offset=True, chunks=3),
                bcase(4, 6, 2080, rm, relu, det=True, chunks=1, stat_passes=3), bcase(3, 5, 2731, rm, relu, det=True, chunks=1)]
    for rm, relu in MODES[2:]:
        # more than 256 x 4096 elements per channel: the cap binds, every statistics workgroup makes a second pass
        out.append(bcase(2, 3, 540000, rm, relu, chunks=256, capped=True, per=4220, stat_passes=2, stat='vec4', apply='vec'))
    # more than 256 x 3 x 4096: a thread makes the four passes after which it flushes its float32 sums into the float64 ones
    out.append(bcase(2, 1, 1600000, 1, True, capped=True, flush=True, stat_passes=4))
    for N, C, S in ((3, 10, 1280), (4, 6, 2080)):
        out += [bcase(N, C, S, 1, True, mis='x', stat='scalar', apply='scalar'),
                bcase(N, C, S, 1, True, mis='res', fwd_stat='vec4', fwd_apply='scalar', bwd_apply='vec'),
                bcase(N, C, S, 2, True, mis='res', fwd_stat='vec4', fwd_apply='scalar'),
                bcase(N, C, S, 1, True, mis='dy', fwd_apply='vec', bwd_stat='scalar', bwd_apply='scalar'),
                bcase(N, C, S, 0, False, mis='x', stat='scalar', apply='scalar')]
    return out


def bn_paths(c):
    mis = (c['mis'],) if c['mis'] else ()
    return {k: path('bn_' + k, c['N'], c['C'], c['S'], c['det'], mis) for k in ('fwd', 'bwd')}


def _stat_tag(p):
    return f'st{p["chunks"]}{"cap" if p["capped"] else ""}x{p["per"]}{p["stat"]}x{p["stat_passes"]}{"flush" if p["flush"] else ""}'


def bn_id(c):
    p = bn_paths(c)
    f, b = p['fwd'], p['bwd']
    tag = f'bn-N{c["N"]}C{c["C"]}S{c["S"]}-r{c["res_mode"]}{"relu" if c["relu"] else "lin"}-{_stat_tag(f)}-{f["apply"]}x{f["apply_passes"]}' \
          f'-bwd{b["stat"]}-{b["apply"]}x{b["apply_passes"]}'
    return tag + ('-offset' if c['offset'] else '') + (f'-mis{c["mis"]}' if c['mis'] else '') + ('-det' if c['det'] else '')


def bn_inputs(c):
    """x, res, dy (N, C, S); gamma, beta; running statistics and parameter gradients to start from (none trivial)"""
    N, C, S = c['N'], c['C'], c['S']
    g = _gen('bn', N, C, S, c['res_mode'], c['relu'], c['offset'])
    per = path('bn_fwd', N, C, S)['per']                      # the twins (misaligned, deterministic) share the data
    x = _rows(stat_input(g, C, N * S, S, per, c['offset']), N, C, S)
    dy = _rows(stat_input(g, C, N * S, S, per, base=torch.randn(C, N * S, generator=g)), N, C, S)
    return {'x': x, 'res': torch.randn(N, C, S, generator=g), 'dy': dy, 'gamma': 0.5 + torch.rand(C, generator=g),
            'beta': torch.rand(C, generator=g) - 0.5, 'rm0': 0.3 * torch.randn(C, generator=g), 'rv0': 0.5 + 1.5 * torch.rand(C, generator=g),
            'dgamma0': torch.randn(C, generator=g), 'dbeta0': torch.randn(C, generator=g)}


def mask_from_output(res_mode, y_out, res, pre64):
    """the ReLU mask a subject applied, read off its forward output.  res_mode 0 / 1: y > 0.  res_mode 2 (y = relu(bn) + res):
    y - res > 0, exact in float64; where y == res and the float64 pre-activation is positive but below half an ulp of res the
    output cannot tell (the sum absorbed it): the float64 mask stands there."""
    if res_mode != 2:
        return torch.as_tensor(y_out).detach().cpu() > 0
    r = res.double()
    m = torch.as_tensor(y_out).detach().cpu().double() - r > 0
    return m | (~m & (pre64 > 0) & (pre64 <= 2.0 ** -22 * r.abs()))


def mask_facts(mask, pre64):
    """(fraction of elements on which `mask` differs from the float64 mask, largest |pre-activation| at such an element over
    max |pre-activation|)"""
    dis = mask != (pre64 > 0)
    n = int(dis.sum())
    return n / max(mask.numel(), 1), (float(pre64[dis].abs().max()) / float(pre64.abs().max()) if n else 0.0)


def bn_reference(c, inp, dtype=F64, y_out=None, swap_res=False, biased_running=False, unbiased_y=False):
    """train-mode BatchNorm2d over (N, C, S) + residual / ReLU epilogue: y = act(bn(x) [+ res, res_mode 1]) [+ res, res_mode 2];
    biased variance in y, unbiased in running_var (biased when a channel has one element: the kernel's documented rule, PyTorch
    refuses that call), momentum update; gradients under the upstream dy, parameter gradients added to the pre-filled ones.
    y_out: a subject's forward output, whose ReLU mask the gradient is evaluated with (None: the evaluation's own).
    swap_res / biased_running / unbiased_y: planted errors for the CPU test."""
    N, C, S, rm, relu = c['N'], c['C'], c['S'], c['res_mode'], c['relu']
    if swap_res and rm:
        rm = 3 - rm
    cnt = N * S
    x, gamma, beta, res = (inp[k].to(dtype).clone().requires_grad_(True) for k in ('x', 'gamma', 'beta', 'res'))
    col = lambda t: t[None, :, None]      # noqa: E731
    m = x.mean(dim=(0, 2))
    d = x - col(m)
    var = (d * d).mean(dim=(0, 2))
    unb = var * (cnt / (cnt - 1.0)) if cnt > 1 else var
    rstd = 1.0 / torch.sqrt((unb if unbiased_y else var) + BN_EPS)
    pre = d * col(rstd) * col(gamma) + col(beta)
    if rm == 1:
        pre = pre + res
    out, y, facts = pre, pre.detach(), None
    if relu:
        pre64 = pre.detach().double()
        mask = pre.detach() > 0 if y_out is None else mask_from_output(rm, y_out, inp['res'], pre64)
        facts = mask_facts(mask, pre64)
        out, y = torch.where(mask, pre, torch.zeros_like(pre)), pre.detach().clamp_min(0)
    if rm == 2:
        out, y = out + res, y + res.detach()
    gx, gg, gb, gr = torch.autograd.grad(out, [x, gamma, beta, res], inp['dy'].to(dtype), allow_unused=True)
    md, vd = m.detach(), var.detach()
    ref = {'y': y, 'mean': md, 'rstd': rstd.detach(),
           'running_mean': (1 - BN_MOMENTUM) * inp['rm0'].to(dtype) + BN_MOMENTUM * md,
           'running_var': (1 - BN_MOMENTUM) * inp['rv0'].to(dtype) + BN_MOMENTUM * (vd if biased_running else unb.detach()),
           'dx': gx, 'dgamma': inp['dgamma0'].to(dtype) + gg, 'dbeta': inp['dbeta0'].to(dtype) + gb,
           '_mean_den': torch.maximum(md.abs(), vd.sqrt()).double(), '_mask': facts, '_pre': pre.detach()}
    if rm:
        ref['dres'] = gr
    return ref


BN_FAM = {'y': 'bn_y', 'mean': 'bn_stat', 'rstd': 'bn_stat', 'running_mean': 'bn_run', 'running_var': 'bn_run', 'dx': 'bn_dx',
          'dres': 'bn_dres', 'dgamma': 'bn_dparam', 'dbeta': 'bn_dparam'}


# ------------------------------------------------------------------------------------------------ AdaIN
def acase(N, C, S, bcast=False, offset=False, mis=None, **expect):
    return dict(N=N, C=C, S=S, bcast=bcast, offset=offset, mis=mis, expect=expect)


ADAIN_SHAPES = [
    acase(3, 10, 144, chunks=1, stat='vec4', apply='scalar'),
    acase(3, 10, 2048, chunks=1, stat='vec4', apply='vec'),
    acase(2, 4, 4160, chunks=2, per=2080, stat='vec4', apply='vec'),
    acase(2, 3, 4099, chunks=2, per=2052, stat='scalar', apply='scalar'),
    acase(2, 2, 540672, chunks=128, capped=True, per=4224, stat_passes=2, apply='vec'),
    acase(40000, 1, 4, grow=True, stat='vec4', apply='scalar'),      # 80000 doubles: the accumulator is freed and re-allocated ...
    acase(3, 10, 9, bcast=True, launches=3, stat='scalar'),          # ... and an ordinary case follows
    acase(3, 4, 2048, bcast=True, launches=3, stat='vec4', apply='vec'),
    acase(3, 10, 2048, mis='x', stat='scalar', apply='scalar'),
    acase(3, 10, 2048, mis='dy', fwd_stat='vec4', fwd_apply='vec', bwd_stat='scalar', bwd_apply='scalar'),
    acase(2, 4, 4160, offset=True, chunks=2),
    acase(1, 2, 1600000, capped=True, flush=True, stat_passes=4),    # 128 x 3 x 4096 < S: the periodic flush to float64
]
ADAIN_CASES = [dict(c, pre=pre) for c in ADAIN_SHAPES for pre in (False, True)]
MOMENT_CASES = [dict(acase(2, 8, 1028), pre=False), dict(acase(2, 8, 4160), pre=True)]      # moments handed in: no statistics pass


def adain_paths(c):
    mis = (c['mis'],) if c['mis'] else ()
    return {k: path('adain_' + k, c['N'], c['C'], c['S'], False, mis, c['bcast']) for k in ('fwd', 'bwd')}


def adain_id(c):
    p = adain_paths(c)
    f, b = p['fwd'], p['bwd']
    tag = f'adain-N{c["N"]}C{c["C"]}S{c["S"]}-{_stat_tag(f)}-{f["apply"]}x{f["apply_passes"]}-bwd{b["stat"]}-{b["apply"]}x{b["apply_passes"]}'
    return tag + ('-bcast' if c['bcast'] else '') + ('-grow' if f['grow'] else '') + ('-offset' if c['offset'] else '') + \
        (f'-mis{c["mis"]}' if c['mis'] else '') + ('-lrelu' if c['pre'] else '')


def _pre_activate(g, z):
    """the output of a LeakyReLU with about 1 % exact zeros"""
    z = torch.where(torch.rand(z.shape, generator=g) < 0.01, torch.zeros_like(z), z)
    return torch.nn.functional.leaky_relu(z, SLOPE)


def adain_inputs(c):
    """x (N, C, S), or (C, S) for a broadcast input; style (N, 2C); dy (N, C, S).  pre: x is the output of LeakyReLU(0.2)"""
    N, C, S = c['N'], c['C'], c['S']
    g = _gen('adain', N, C, S, c['bcast'], c['offset'], c['pre'])
    per = path('adain_fwd', N, C, S)['per']
    G = C if c['bcast'] else N * C
    x = stat_input(g, G, S, S, per, c['offset'])
    if c['pre']:
        x = _pre_activate(g, x)
    dy = stat_input(g, N * C, S, S, per, base=torch.randn(N * C, S, generator=g))
    return {'x': x.view(C, S) if c['bcast'] else x.view(N, C, S), 'style': torch.randn(N, 2 * C, generator=g), 'dy': dy.view(N, C, S)}


def _adain(h, style, C):
    """(y, mean, rstd, std) of style[:, :C] * (h - mean) * rstd + style[:, C:], statistics per (n, c) over the last axis"""
    m = h.mean(-1, keepdim=True)
    d = h - m
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + ADAIN_EPS)
    return style[:, :C, None] * (d * rstd) + style[:, C:, None], m[..., 0], rstd[..., 0], var[..., 0].sqrt()


def _act_grad(x, dtype):
    """act_grad_from_out of a LeakyReLU: 1 where the output is positive, `slope` elsewhere - at exactly 0 too"""
    return torch.where(x > 0, torch.ones((), dtype=dtype), torch.full((), SLOPE, dtype=dtype))


def adain_reference(c, inp, dtype=F64):
    N, C = c['N'], c['C']
    h, style = inp['x'].to(dtype).clone().requires_grad_(True), inp['style'].to(dtype).clone().requires_grad_(True)
    y, m, rstd, sd = _adain(h.expand(N, *h.shape) if c['bcast'] else h, style, C)
    gx, gs = torch.autograd.grad(y, [h, style], inp['dy'].to(dtype))
    if c['pre']:
        gx = gx * _act_grad(inp['x'], dtype)
    a = style.detach()[:, :C] * rstd.detach()
    return {'y': y.detach(), 'mean': m.detach().reshape(-1), 'rstd': rstd.detach().reshape(-1), 'dx': gx, 'dstyle': gs,
            'aff_a': a, 'aff_b': style.detach()[:, C:] - a * m.detach(),
            '_mean_den': torch.maximum(m.detach().abs(), sd.detach()).double().reshape(-1)}


ADAIN_FAM = {'y': 'adain_y', 'mean': 'adain_stat', 'rstd': 'adain_stat', 'aff_a': 'adain_stat', 'aff_b': 'adain_stat',
             'dx': 'adain_dx', 'dstyle': 'adain_dstyle'}


# ------------------------------------------------------------------------------------------------ AdaIN + 1x1x1 head
HEAD_C, HEAD_CO = 8, 2


def hcase(N, S, bias, pre, **expect):
    return dict(N=N, S=S, bias=bias, pre=pre, expect=expect)


HEAD_CASES = [hcase(N, S, bias, pre, **ex) for (N, S, ex) in ((3, 1024, dict(gx=1, passes=1)), (2, 1028, dict(gx=1, passes=2)), (1, 4100, dict(gx=2, passes=3)))
              for bias in (True, False) for pre in (False, True)] + \
             [hcase(2, 528384, bias, pre, gx=128, capped=True, passes=5) for bias, pre in ((True, True), (False, False))]
# S = 528384: 132096 quads want 129 workgroups of 1024, the cap of 128 binds in forward and in both backward kernels: 5 passes


def head_paths(c):
    return {k: path('head_' + k, c['N'], HEAD_C, c['S']) for k in ('fwd', 'bwd')}


def head_id(c):
    f = head_paths(c)['fwd']
    return f'head-N{c["N"]}S{c["S"]}-gx{f["gx"]}{"cap" if f["capped"] else ""}x{f["passes"]}-{"bias" if c["bias"] else "nobias"}' + ('-lrelu' if c['pre'] else '')


def head_inputs(c):
    N, S = c['N'], c['S']
    g = _gen('head', N, S, c['bias'], c['pre'])
    x = stat_input(g, N * HEAD_C, S, S, S)
    if c['pre']:
        x = _pre_activate(g, x)
    dl = stat_input(g, N * HEAD_CO, S, S, S, base=torch.randn(N * HEAD_CO, S, generator=g))
    return {'x': x.view(N, HEAD_C, S), 'style': torch.randn(N, 2 * HEAD_C, generator=g), 'dl': dl.view(N, HEAD_CO, S),
            'w': 0.3 * torch.randn(HEAD_CO, HEAD_C, generator=g), 'b': torch.randn(HEAD_CO, generator=g) if c['bias'] else None,
            'dw0': torch.randn(HEAD_CO, HEAD_C, generator=g), 'db0': torch.randn(HEAD_CO, generator=g)}


def head_reference(c, inp, dtype=F64):
    """logits[n, o, s] = b[o] + sum_c w[o, c] adain(x)[n, c, s]; dx, dstyle, and the head gradients added to the pre-filled ones"""
    h, style, w = (inp[k].to(dtype).clone().requires_grad_(True) for k in ('x', 'style', 'w'))
    b = inp['b'].to(dtype).clone().requires_grad_(True) if c['bias'] else None
    y = _adain(h, style, HEAD_C)[0]
    logits = torch.einsum('oc,ncs->nos', w, y)
    if b is not None:
        logits = logits + b[None, :, None]
    gs = torch.autograd.grad(logits, [h, style, w] + ([b] if c['bias'] else []), inp['dl'].to(dtype))
    gx = gs[0] * _act_grad(inp['x'], dtype) if c['pre'] else gs[0]
    ref = {'logits': logits.detach(), 'dx': gx, 'dstyle': gs[1], 'dw': inp['dw0'].to(dtype) + gs[2]}
    if c['bias']:
        ref['db'] = inp['db0'].to(dtype) + gs[3]
    return ref


HEAD_FAM = {'logits': 'head_logits', 'dx': 'head_dx', 'dstyle': 'head_dparam', 'dw': 'head_dparam', 'db': 'head_dparam'}


# ------------------------------------------------------------------------------------------------ add + dropout + LayerNorm
def lcase(rows, E, p=0.1, det=False, **expect):
    return dict(rows=rows, E=E, p=p, det=det, expect=expect)


LN_CASES = [lcase(37, E, slots=_cdiv(E, 64), tail=5, blocks=3) for E in (1, 63, 64, 65, 96, 384, 511, 512)] + \
           [lcase(r, 96, blocks=_cdiv(r, 16), tail=r % 16) for r in (1, 3, 4, 15, 16, 17, 70)] + \
           [lcase(37, E, p) for E in (96, 384) for p in (0.0, 0.5)] + \
           [lcase(70, 96, det=True, blocks=1, rows_per_block=70, trips=5), lcase(37, 512, det=True, blocks=1, rows_per_block=37, trips=3)]
LN_SEED = 20240613


def ln_path(c):
    return path('ln', c['rows'], 0, c['E'], c['det'])


def ln_id(c):
    p = ln_path(c)
    return f'ln-rows{c["rows"]}E{c["E"]}-p{c["p"]}-blk{p["blocks"]}x{p["rows_per_block"]}tail{p["tail"]}-slots{p["slots"]}-trips{p["trips"]}' + \
        ('-det' if c['det'] else '')


def ln_inputs(c):
    rows, E = c['rows'], c['E']
    g = _gen('ln', rows, E, c['p'])
    keep = (torch.rand(rows, E, generator=g) >= c['p']).float()
    return {'x': torch.randn(rows, E, generator=g), 'a': torch.randn(rows, E, generator=g), 'dy': torch.randn(rows, E, generator=g),
            'gamma': 0.5 + torch.rand(E, generator=g), 'beta': torch.rand(E, generator=g) - 0.5, 'dgamma0': torch.randn(E, generator=g),
            'dbeta0': torch.randn(E, generator=g),
            'cpu_scale': keep / (1 - c['p'])}       # stands in for ops.dropout(ones, p, seed) where there is no GPU


def ln_reference(c, inp, scale, dtype=F64, unmasked_da=False):
    """y = LayerNorm(x + a * scale), scale the dropout's (0 or 1 / (1 - p)) as a tensor; dx, da, parameter gradient totals"""
    x, a, gamma, beta = (inp[k].to(dtype).clone().requires_grad_(True) for k in ('x', 'a', 'gamma', 'beta'))
    z = x + a * scale.to(dtype)
    m = z.mean(-1, keepdim=True)
    d = z - m
    y = d / torch.sqrt((d * d).mean(-1, keepdim=True) + LN_EPS) * gamma + beta
    gx, ga, gg, gb = torch.autograd.grad(y, [x, a, gamma, beta], inp['dy'].to(dtype))
    return {'y': y.detach(), 'dx': gx, 'da': gx.clone() if unmasked_da else ga, 'dgamma': inp['dgamma0'].to(dtype) + gg,
            'dbeta': inp['dbeta0'].to(dtype) + gb}


LN_FAM = {'y': 'ln_y', 'dx': 'ln_dx', 'da': 'ln_da', 'dgamma': 'ln_dparam', 'dbeta': 'ln_dparam'}


# ================================================================================================ comparison
def compare(fam, got, ref, factor=1.0, extra=0.0):
    """{name: (stats, bar)} of the results named in `fam` (a *_FAM table) that the reference has; mean-like statistics are
    normalised by ref['_mean_den'], everything else by max |ref|; the bar is the family's x factor + extra"""
    out = {}
    for name, family in fam.items():
        if name not in ref or name not in got:
            continue
        den = ref['_mean_den'].reshape(ref[name].shape) if name in ('mean', 'running_mean') else scale_of(ref[name])
        out[name] = (error_stats(got[name], ref[name], den), BARS[family] * factor + extra)
    return out


def statlines(tag, cmp):
    return [f'NORMSTAT {tag} {n}: {s["max_e"]:.3e} {s["rms"]:.3e} ({bar:.2e})' for n, (s, bar) in cmp.items()]


def factor_of(c):
    return OFFSET_FACTOR if c.get('offset') else 1.0


# ================================================================================================ the table in the docstring
def evaluate32(kind, c):
    """(comparison of the float32 CPU evaluation of one case with the float64 reference, the float64 reference)"""
    if kind == 'bn':
        inp = bn_inputs(c)
        sub = bn_reference(c, inp, torch.float32)
        ref = bn_reference(c, inp, y_out=sub['y'])
        return compare(BN_FAM, sub, ref, factor_of(c)), ref
    if kind == 'adain':
        inp = adain_inputs(c)
        ref = adain_reference(c, inp)
        return compare(ADAIN_FAM, adain_reference(c, inp, torch.float32), ref, factor_of(c)), ref
    if kind == 'head':
        inp = head_inputs(c)
        ref = head_reference(c, inp)
        return compare(HEAD_FAM, head_reference(c, inp, torch.float32), ref), ref
    inp = ln_inputs(c)
    ref = ln_reference(c, inp, inp['cpu_scale'])
    return compare(LN_FAM, ln_reference(c, inp, inp['cpu_scale'], torch.float32), ref), ref


CASES = {'bn': None, 'adain': ADAIN_CASES + MOMENT_CASES, 'head': HEAD_CASES, 'ln': LN_CASES}
FAMS = {'bn': BN_FAM, 'adain': ADAIN_FAM, 'head': HEAD_FAM, 'ln': LN_FAM}
BN_CASES = CASES['bn'] = _bn_cases()


def float32_errors(kind, offset=False):
    """{family: largest e of the float32 CPU evaluation} over the cases of `kind`; offset: over the offset cases alone (normally
    left out: their bar is derived from the others')"""
    worst = {}
    for c in CASES[kind]:
        if bool(c.get('offset')) != offset:
            continue
        for n, (s, _) in evaluate32(kind, c)[0].items():
            f = FAMS[kind][n]
            worst[f] = max(worst.get(f, 0.0), s['max_e'])
    return worst


if __name__ == '__main__':
    import time
    for kind in ('ln', 'bn', 'adain', 'head'):
        t0 = time.time()
        for fam, e in sorted(float32_errors(kind).items()):
            print(f'{fam:13s} float32 evaluation max(e) {e:.2e}   4x = {4 * e:.2e}   bar in use {BARS[fam]:.2e}   ({time.time() - t0:.0f} s)', flush=True)
        for fam, e in sorted(float32_errors(kind, offset=True).items()):
            print(f'{fam:13s} OFFSET cases: float32 evaluation max(e) {e:.2e}   bar {BARS[fam] * OFFSET_FACTOR:.2e}', flush=True)
