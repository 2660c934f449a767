"""Plain float64 references, float32 CPU emulations, planted faults, the case lists and a restatement of the host-side size
functions for the two persistent RSSM kernels (muvo_amd/csrc/rssm.hip: rssm_fwd_kernel / rssm_bwd_kernel, 4 grid barriers per time
step each).  Helpers only: no fixtures, no tests.  tests/test_rssm_reference.py (CPU) and tests/test_rssm_kernels_gpu.py (GPU)
share everything here, so the bars the GPU test applies are the ones the CPU test proves to pass the emulated arithmetic and to
reject the planted faults.  The metric is that of tests/vox_reference.py (error_stats: e = |got - ref64| / den per element, next
to rms(got - ref) / rms(ref)), the fp32 bar that of tests/conv_reference.py (f32_bar).

One evaluator for everything.  `evaluate` walks the T steps forward and back from the formulas at the top of rssm.hip and
oracle/muvo_ref.py:RSSM, with the backward written out by hand (every kept gradient gets a value, an absent upstream is
expressible).  In float64 with plain products it is the reference; in float32 with `emu_wave_dots` (the summation order of
wave_dots) and the float32 pointwise parts of tests/elementwise_reference.py (gru_eval, sample_eval) it is the emulation of the
kernels; the planted faults are switches on it.  It returns the 7 outputs, the 12 kept tensors, the 10 kept gradients and the two
carries of every step.

One-stage ("teacher-forced") references.  `stages` takes a result (the emulation's or the GPU's) and evaluates every stage of every
step in float64 FROM THAT RESULT'S OWN STORED INPUTS of the stage: u from zprev, gh from hprev, the two action latents from aprev,
gi from u, h from (gi, gh, hprev), y1* from x*, mls* from y1*, sigma and z from mls* and the noise; backward: dmls* from the
upstreams, mls* and the dz carry, dy1* from dmls*, d_emb / dla* from dy1*, dgi / dgh from the stored forward tensors and g, du from
dgi.  The carries are not kept per step: dz_{t-1} = W_pre^T du_t and dh_{t-1} = W_hh^T dgh_t + g_t z_t (g the gradient that reaches
h_t) are rebuilt in float64 from the kept tensors.  Every stage comes with its denominator: sqrt(sum w^2 x^2 + b^2) for a mat-vec,
the scales of elementwise_reference (den_hn, den_sample, den_dmls, |g| (1 + |h| + |gh_n|)) for the pointwise parts, with the
mat-vec denominators of a rebuilt input in place of its absolute value, and for h the scale of its three rounded pre-activation
sums next to den_hn (_gru_pre_scale: den_hn alone vanishes where gi_n and r gh_n cancel).  That puts a u sqrt(K) bar on every stage
of every step instead of one loose bar on the end of the recurrence.  What the kernels copy (hprev, zprev, aprev, the h / embedding slices of x*,
mu = mls[:S]) is compared bit for bit (`copies`).

Bars: see STAGE_OWN_WORST / E2E_MEASURED below.  None comes from a GPU."""
import collections
import functools
import math
import types
import zlib

import torch

import elementwise_reference as EW
from conv_reference import U32, f32_bar
from elementwise_reference import wave_sum32
from vox_reference import error_stats, excess, within  # noqa: F401

F32, F64 = torch.float32, torch.float64
MIN_STD = 0.1
BM = 4                           # RSSM_BM: sequences per launch (slab)
WPB = 8                          # waves per workgroup
MAX_DYN_LDS = 160 * 1024 - 256   # RSSM_MAX_DYN_LDS
DEFAULT_CUS = 256                # MI355X: the default grid is one workgroup per CU (the coverage restatement uses it)

WNAMES = ('w_pre', 'b_pre', 'w_ih', 'w_hh', 'b_ih', 'b_hh', 'w_pa', 'b_pa', 'w_qa', 'b_qa', 'w_p0', 'b_p0', 'w_p2', 'b_p2', 'w_q0',
          'b_q0', 'w_q2', 'b_q2')
# the same 18 tensors under their names in oracle.muvo_ref.RSSM / muvo_amd.models.transition.RSSM (ops.rssm_weights order)
MODULE_NAMES = ('pre_gru_net.0.weight', 'pre_gru_net.0.bias', 'recurrent_model.weight_ih', 'recurrent_model.weight_hh',
                'recurrent_model.bias_ih', 'recurrent_model.bias_hh', 'prior_action_module.0.weight', 'prior_action_module.0.bias',
                'posterior_action_module.0.weight', 'posterior_action_module.0.bias', 'prior.module.0.weight', 'prior.module.0.bias',
                'prior.module.2.weight', 'prior.module.2.bias', 'posterior.module.0.weight', 'posterior.module.0.bias',
                'posterior.module.2.weight', 'posterior.module.2.bias')
OUT7 = ('h', 'mu_p', 'sg_p', 'z_p', 'mu_q', 'sg_q', 'z_q')
KEEP12 = ('hprev', 'zprev', 'aprev', 'u', 'gi', 'gh', 'xp', 'xq', 'y1p', 'y1q', 'mls_p', 'mls_q')
KEPT5 = ('hprev', 'gi', 'gh', 'mls_p', 'mls_q')              # what muvo_rssm_backward reads of them
GRAD10 = ('d_emb', 'dmls_p', 'dmls_q', 'dy1p', 'dy1q', 'dgi', 'dgh', 'du', 'dla_p', 'dla_q')
UP7 = ('g_h', 'g_mu_p', 'g_sg_p', 'g_z_p', 'g_mu_q', 'g_sg_q', 'g_z_q')
# weight gradient = dY^T X, bias gradient = column sums of dY (ops.RSSMFusedFn.backward): (dY, X, weight, bias)
PARAM_PAIRS = (('du', 'zprev', 'w_pre', 'b_pre'), ('dgi', 'u', 'w_ih', 'b_ih'), ('dgh', 'hprev', 'w_hh', 'b_hh'),
               ('dla_p', 'aprev', 'w_pa', 'b_pa'), ('dla_q', 'aprev', 'w_qa', 'b_qa'), ('dy1p', 'xp', 'w_p0', 'b_p0'),
               ('dmls_p', 'y1p', 'w_p2', 'b_p2'), ('dy1q', 'xq', 'w_q0', 'b_q0'), ('dmls_q', 'y1q', 'w_q2', 'b_q2'))


def _cdiv(a, b):
    return -(-a // b)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def widths(c):
    """last-axis width of every (B, T, .) tensor of the C ABI"""
    H, S, E, A = c['dims']
    HP, HQ, AD = H + A, H + E + A, c['AD']
    w = dict(h=H, hprev=H, zprev=S, aprev=AD, u=H, gi=3 * H, gh=3 * H, xp=HP, xq=HQ, y1p=HP, y1q=HQ, mls_p=2 * S, mls_q=2 * S,
             d_emb=E, dmls_p=2 * S, dmls_q=2 * S, dy1p=HP, dy1q=HQ, dgi=3 * H, dgh=3 * H, du=H, dla_p=A, dla_q=A, g_h=H,
             emb=E, act=AD, noise=2 * S)
    for n in OUT7[1:] + UP7[1:]:
        w[n] = S
    return w


def wshapes(c):
    H, S, E, A = c['dims']
    HP, HQ, AD = H + A, H + E + A, c['AD']
    return dict(w_pre=(H, S), b_pre=(H,), w_ih=(3 * H, H), w_hh=(3 * H, H), b_ih=(3 * H,), b_hh=(3 * H,), w_pa=(A, AD), b_pa=(A,),
                w_qa=(A, AD), b_qa=(A,), w_p0=(HP, HP), b_p0=(HP,), w_p2=(2 * S, HP), b_p2=(2 * S,), w_q0=(HQ, HQ), b_q0=(HQ,),
                w_q2=(2 * S, HQ), b_q2=(2 * S,))


# ================================================================================================ host-side mirror
def dims_ok(B, T, H, S, E, A, AD):
    return (1 <= B <= 64 and 1 <= T <= 64 and H % 4 == 0 and S % 4 == 0 and E % 4 == 0 and A % 4 == 0 and AD >= 1 and H > 0 and S > 0
            and E > 0 and A > 0)


def fwd_lds(B, H, S, E, A, AD):
    """rssm_fwd_lds: bytes of dynamic LDS of a forward launch over B <= 4 sequences (xa holds z_{t-1} in stage 0, xq afterwards)"""
    return 4 * (B * (max(H + E + A, S) + (H + A) + H + AD) + 16)


def bwd_lds(B, H, S, E, A):
    """rssm_bwd_lds (xa / xb hold dmls in B0: 2S each, dy1 in B1, dgi / dgh in B2: 3H each)"""
    HP, HQ = H + A, H + E + A
    return 4 * (B * (max(HQ, 3 * H, 2 * S) + max(HP, 3 * H, 2 * S) + H) + 16)


def supported(B, T, H, S, E, A, AD):
    """muvo_rssm_supported on a machine with a GPU"""
    if not dims_ok(B, T, H, S, E, A, AD):
        return 0
    Bc = min(B, BM)
    return int(fwd_lds(Bc, H, S, E, A, AD) <= MAX_DYN_LDS and bwd_lds(Bc, H, S, E, A) <= MAX_DYN_LDS)


def transposed_floats(H, S, E, A):
    HP, HQ = H + A, H + E + A
    return H * S + 2 * 3 * H * H + HP * HP + 2 * S * HP + HQ * HQ + 2 * S * HQ


def scratch_floats(B, H, S, E, A):
    return B * ((H + A) + (H + E + A) + 2 * H + S)


# Points at which muvo_rssm_supported is 0, as changes to a point at which it is just 1.
#   LIMIT_BWD (the 'lds-limit-b4-t1' case): the BACKWARD kernel's LDS is exactly MAX_DYN_LDS.  One step past it (H = 1464) the forward
#     still fits (its xa / xb hold HQ and HP, not 3H), so it is muvo_rssm_backward that returns the argument error there.
#   LIMIT_FWD: the FORWARD kernel's LDS is exactly MAX_DYN_LDS (7H + E = 10220 floats per sequence with A = 2H - 4, AD = 8; the
#     backward needs 4 floats less).  One step of 4 past it in H, E or A, and at each violated range or % 4 condition,
#     muvo_rssm_forward returns the argument error without a launch.  Its weights are 208 MB: the point is queried, not run.
LIMIT_BWD = dict(B=4, T=1, H=1460, S=4, E=4, A=4, AD=2)
LIMIT_FWD = dict(B=4, T=1, H=1456, S=4, E=28, A=2908, AD=8)
PAST_BWD = [dict(H=1464), dict(E=4400), dict(B=1, H=4 * 1460 + 4), dict(S=2192)]          # 2S = 4384 > 3H = 4380
PAST_FWD = [dict(E=32), dict(A=2912), dict(H=1460), dict(AD=9), dict(S=4396), dict(B=0), dict(B=65), dict(T=0), dict(T=65), dict(H=1458), dict(S=6),
            dict(E=30), dict(A=2910), dict(AD=0), dict(H=0), dict(S=0), dict(E=0), dict(A=0), dict(H=-4), dict(S=-4)]


def matvecs(c):
    """Restatement of the kernels' loops: {stage: (output rows dealt to the waves, [K of each wave_dots call])}"""
    H, S, E, A = c['dims']
    HP, HQ = H + A, H + E + A
    return {'f0': (4 * H + 2 * A, [S, H]), 'f1': (H, [H]), 'f2': (HP + HQ, [HP, HQ]), 'f3': (2 * S, [HP, HQ]),
            'b0': (HP + HQ, [2 * S]), 'b1': (HP + HQ, [HP, HQ]), 'b2': (2 * H, [3 * H]), 'b3': (S, [H])}


def all_K(c):
    return sorted({k for _, ks in matvecs(c).values() for k in ks})


# ================================================================================================ cases
def rcase(name, B, T, dims, AD, masks, ups=('all',)):
    return dict(name=name, B=B, T=T, dims=dims, AD=AD, masks=tuple(masks), ups=tuple(ups))


TINY, SUB256, PASS2 = (4, 4, 4, 4), (260, 132, 4, 4), (344, 516, 8, 4)
UPS_PATTERNS = ('all', 'zq_only', 'h_only', 'sgp_only', 'none')
CASES = [
    # fewer than 64 active lanes (every K <= 12); every mask and every upstream pattern; one short slab
    rcase('tiny-b3-t5', 3, 5, TINY, 2, ('alt', 'none', 'ones', 'bit0', 'last'), UPS_PATTERNS),
    rcase('tiny-b64-t1', 64, 1, TINY, 1, ('none',)),                         # sixteen slabs
    rcase('tiny-b1-t64', 1, 64, TINY, 3, ('alt', 'hi', 'last', 'ones')),     # mask bits 62 and 63
    rcase('sub256-b5-t2', 5, 2, SUB256, 2, ('bit0', 'none')),                # K = 260, 264, 268, 780; slab + 1
    rcase('pass2-b8-t2', 8, 2, PASS2, 3, ('bit0', 'none')),                  # 3H = 2S = 1032: second pass, 2-lane tail; two slabs
    rcase('k256-b4-t2', 4, 2, (256, 128, 4, 4), 2, ('ones',)),               # K = H = 2S = 256, 3H = 768; a full slab
    rcase('k1024-b1-t2', 1, 2, (4, 1024, 4, 4), 1, ('bit0',)),               # K = S = 1024, 2S = 2048
    # 7H * 16 + 64 = MAX_DYN_LDS exactly (backward); 4H + 2A = 5848 rows over 2048 waves: several rows per wave
    rcase('lds-limit-b4-t1', 4, 1, (1460, 4, 4, 4), 2, ('none',)),
]
CASE = {c['name']: c for c in CASES}
assert len(CASE) == len(CASES)
GRID_CASES = ('sub256-b5-t2', 'pass2-b8-t2')         # the small-grid check
FAMILY_CASES = ('tiny-b3-t5', 'sub256-b5-t2', 'pass2-b8-t2')      # frozen-parameter runs through ops.RSSMFusedFn


def mask_value(name, T):
    """64-bit use_prior mask: bit t set = step t + 1 continues from the prior sample of step t"""
    full = (1 << 64) - 1
    return {'none': 0, 'ones': full, 'alt': 0xAAAAAAAAAAAAAAAA if T > 2 else 0x5555555555555555, 'bit0': 1,
            'last': 1 << max(T - 2, 0), 'hi': (1 << 62) | (1 << 63)}[name]


def irrelevant_bits(T):
    """the bits no step reads: the forward reads bit t - 1 for t < T, the backward bit t only where a carry exists (t < T - 1)"""
    return ((1 << 64) - 1) & ~((1 << (T - 1)) - 1)


def runs():
    """every (case, mask name, upstream pattern) the per-stage checks visit: every mask with all upstreams, every other
    upstream pattern with the case's first mask"""
    out = []
    for c in CASES:
        out += [(c['name'], m, 'all') for m in c['masks']]
        out += [(c['name'], c['masks'][0], u) for u in c['ups'] if u != 'all']
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """seeded CPU inputs of a case: weights of size 1 / sqrt(fan_in) (gate and log sigma pre-activations of size 1), biases of
    size 0.3, embedding and noise N(0, 1), actions in [-1, 1], the seven upstream gradients N(0, 1)"""
    c = CASE[name]
    g = _gen('rssm', name)
    W = {}
    for n, shp in wshapes(c).items():
        W[n] = torch.randn(*shp, generator=g) * (1 / math.sqrt(shp[1]) if len(shp) == 2 else 0.3)
    wd = widths(c)
    B, T = c['B'], c['T']
    emb = torch.randn(B, T, wd['emb'], generator=g)
    act = torch.rand(B, T, wd['act'], generator=g) * 2 - 1
    noise = torch.randn(B, T, 2, c['dims'][1], generator=g)
    ups = {n: torch.randn(B, T, wd[n], generator=g) for n in UP7}
    return types.SimpleNamespace(W=W, emb=emb, act=act, noise=noise, ups=ups)


def upstreams(inp, pattern):
    """{name: tensor or None (a NULL pointer)}"""
    keep = {'all': UP7, 'zq_only': ('g_z_q',), 'h_only': ('g_h',), 'sgp_only': ('g_sg_p',), 'none': ()}[pattern]
    return {n: (inp.ups[n] if n in keep else None) for n in UP7}


# ================================================================================================ emulation of wave_dots
def emu_wave_dots(x, w, drop_tail=False):
    """x (B, K) float32 dotted with the rows of w (O, K) in the order of wave_dots: per lane, passes of 1024 columns; within a pass
    four 256-column sub-blocks; within a sub-block (w0 x0 + w1 x1) + (w2 x2 + w3 x3), every product and sum rounded once (the
    library is built without contraction); then the xor butterfly of wave_sum.  The bias is the caller's.
    drop_tail (planted fault): the last 4 columns contribute nothing."""
    assert x.dtype == F32 and w.dtype == F32
    B, K = x.shape
    O = w.shape[0]
    P = _cdiv(K, 1024)
    xp = torch.zeros(B, P * 1024)
    xp[:, :K - 4 if drop_tail else K] = x[:, :K - 4 if drop_tail else K]
    xp = xp.view(B, 1, P, 4, 64, 4)
    out = torch.empty(B, O)
    step = max(1, (1 << 22) // (B * P * 1024))
    for o0 in range(0, O, step):
        wc = w[o0:o0 + step]
        wp = torch.zeros(wc.shape[0], P * 1024)
        wp[:, :K] = wc
        wp = wp.view(1, -1, P, 4, 64, 4)
        acc = torch.zeros(B, wc.shape[0], 64)
        for p in range(P):
            for u in range(4):
                if 1024 * p + 256 * u >= K:
                    break
                pr = wp[:, :, p, u] * xp[:, :, p, u]
                acc = acc + ((pr[..., 0] + pr[..., 1]) + (pr[..., 2] + pr[..., 3]))
        out[:, o0:o0 + step] = wave_sum32(acc)
    return out


# ================================================================================================ the evaluator
FAULTS = {          # planted fault -> (case, mask) at which test_bars_bite proves it rejected
    'mask_t': ('tiny-b3-t5', 'alt'),            # forward reads mask bit t in place of t - 1
    'noise_slab': ('sub256-b5-t2', 'bit0'),     # the second slab reads the first slab's noise
    'ktail': ('sub256-b5-t2', 'bit0'),          # the last 4 columns of a K past a 256 boundary are dropped
    'ktail_1024': ('pass2-b8-t2', 'bit0'),      # ... past a 1024 boundary
    'action_t': ('tiny-b3-t5', 'alt'),          # action t in place of t - 1
    'dz_branch': ('tiny-b3-t5', 'alt'),         # the dz carry is added to the other branch
    'no_gz': ('tiny-b3-t5', 'alt'),             # the direct g z term of the dh carry is dropped
    'drop_r': ('tiny-b3-t5', 'alt'),            # dgh's n gate lacks the factor r
    'half_dls': ('tiny-b3-t5', 'alt'),          # s (1 - s) / 2 in dls
    'dh_parity': ('tiny-b3-t5', 'alt'),         # the dh carry is read from the other buffer (the one step t + 2 wrote)
    'no_min_std': ('tiny-b3-t5', 'alt'),        # sigma without min_std
}


def evaluate(c, inp, mask, ups, emu=False, fault=None):
    """The whole model, forward and backward.  emu = False: float64, plain products (the reference).  emu = True: float32 in the
    kernels' order of operations.  Returns {name: (B, T, .) tensor} for OUT7 + KEEP12 + GRAD10 and the carries 'dz_c' / 'dh_c'
    (entry t: what step t hands to step t - 1)."""
    dt = F32 if emu else F64
    B, T, AD = c['B'], c['T'], c['AD']
    H, S, E, A = c['dims']
    W = {k: v.to(dt) for k, v in inp.W.items()}
    emb, act, noise = inp.emb.to(dt), inp.act.to(dt), inp.noise.to(dt)
    if fault == 'noise_slab':
        idx = torch.arange(B)
        idx[BM:2 * BM] -= BM
        noise = noise[idx]
    ms = 0.0 if fault == 'no_min_std' else MIN_STD
    up = {n: (None if t is None else t.to(dt)) for n, t in ups.items()}

    def mv(x, w, b=None):
        K = w.shape[1]
        drop = (fault == 'ktail' and K > 256 and K % 256 != 0) or (fault == 'ktail_1024' and K > 1024 and K % 1024 != 0)
        if emu:
            y = emu_wave_dots(x, w.contiguous(), drop)
        else:
            y = (x[:, :K - 4] @ w[:, :K - 4].t()) if drop else x @ w.t()
        return y if b is None else y + b

    def small(a, w, b):              # the action latents: one lane per (row, sequence), a serial sum that starts at the bias
        if not emu:
            return a @ w.t() + b
        v = b.expand(B, -1).clone()
        for k in range(AD):
            v = v + w[:, k] * a[:, k:k + 1]
        return v

    wd = widths(c)
    r = {n: torch.zeros(B, T, wd[n], dtype=dt) for n in OUT7 + KEEP12 + GRAD10}
    r['dz_c'], r['dh_c'] = torch.zeros(B, T, S, dtype=dt), torch.zeros(B, T, H, dtype=dt)
    zero_h = torch.zeros(B, H, dtype=dt)
    for t in range(T):
        if t == 0:
            zp, hp, ap = torch.zeros(B, S, dtype=dt), zero_h, torch.zeros(B, AD, dtype=dt)
        else:
            bit = (mask >> (t if fault == 'mask_t' else t - 1)) & 1
            zp, hp = (r['z_p'] if bit else r['z_q'])[:, t - 1], r['h'][:, t - 1]
            ap = act[:, t if fault == 'action_t' else t - 1]
        u, gh = mv(zp, W['w_pre'], W['b_pre']), mv(hp, W['w_hh'], W['b_hh'])
        gi = mv(u, W['w_ih'], W['b_ih'])
        hn = EW.gru_eval(gi, gh, hp, zero_h, dt)['hn']
        xp = torch.cat([hn, small(ap, W['w_pa'], W['b_pa'])], 1)
        xq = torch.cat([hn, emb[:, t], small(ap, W['w_qa'], W['b_qa'])], 1)
        y1p, y1q = mv(xp, W['w_p0'], W['b_p0']), mv(xq, W['w_q0'], W['b_q0'])
        mp, mq = mv(y1p, W['w_p2'], W['b_p2']), mv(y1q, W['w_q2'], W['b_q2'])
        sp = EW.sample_eval(mp, noise[:, t, 0], None, None, None, ms, dt)
        sq = EW.sample_eval(mq, noise[:, t, 1], None, None, None, ms, dt)
        for n, v in (('hprev', hp), ('zprev', zp), ('aprev', ap), ('u', u), ('gi', gi), ('gh', gh), ('xp', xp), ('xq', xq),
                     ('y1p', y1p), ('y1q', y1q), ('mls_p', mp), ('mls_q', mq), ('h', hn), ('mu_p', sp['mu']), ('sg_p', sp['sigma']),
                     ('z_p', sp['sample']), ('mu_q', sq['mu']), ('sg_q', sq['sigma']), ('z_q', sq['sample'])):
            r[n][:, t] = v
    # ---------------------------------------------------------------------------------------------- backward
    wt = {n: W[n].t().contiguous() for n in ('w_pre', 'w_ih', 'w_hh', 'w_p0', 'w_p2', 'w_q0', 'w_q2')}
    at = lambda n, t: None if up[n] is None else up[n][:, t]          # noqa: E731
    for t in range(T - 1, -1, -1):
        prior_next = bool((mask >> t) & 1)
        has_carry = t < T - 1
        dm = {}
        for post, tag in ((0, 'p'), (1, 'q')):
            dz = at('g_z_' + tag, t)
            takes = (prior_next == bool(post)) if fault == 'dz_branch' else (prior_next != bool(post))
            if has_carry and takes:
                dz = r['dz_c'][:, t + 1] if dz is None else dz + r['dz_c'][:, t + 1]
            d = EW.sample_eval(r['mls_' + tag][:, t], noise[:, t, post], at('g_mu_' + tag, t), at('g_sg_' + tag, t), dz, ms, dt)['dmls']
            if fault == 'half_dls':
                d = torch.cat([d[:, :S], d[:, S:] * 0.5], 1)
            dm[tag] = d
        dy1p, dy1q = mv(dm['p'], wt['w_p2']), mv(dm['q'], wt['w_q2'])
        dxp, dxq = mv(dy1p, wt['w_p0']), mv(dy1q, wt['w_q0'])
        gh_up = at('g_h', t)
        g = ((zero_h if gh_up is None else gh_up) + dxp[:, :H]) + dxq[:, :H]
        if has_carry:
            if fault != 'dh_parity':
                g = g + r['dh_c'][:, t + 1]
            elif t + 2 < T:
                g = g + r['dh_c'][:, t + 2]
        ge = EW.gru_eval(r['gi'][:, t], r['gh'][:, t], r['hprev'][:, t], g, dt, drop_r=fault == 'drop_r')
        du = mv(ge['dgi'], wt['w_ih'])
        dh = mv(ge['dgh'], wt['w_hh'])
        if fault != 'no_gz':
            dh = dh + ge['dh']
        for n, v in (('dmls_p', dm['p']), ('dmls_q', dm['q']), ('dy1p', dy1p), ('dy1q', dy1q), ('dla_p', dxp[:, H:]),
                     ('d_emb', dxq[:, H:H + E]), ('dla_q', dxq[:, H + E:]), ('dgi', ge['dgi']), ('dgh', ge['dgh']), ('du', du),
                     ('dh_c', dh), ('dz_c', mv(du, wt['w_pre']))):
            r[n][:, t] = v
    return r


@functools.lru_cache(maxsize=None)
def reference64(name, mask_name, pattern):
    c, inp = CASE[name], inputs(name)
    return evaluate(c, inp, mask_value(mask_name, c['T']), upstreams(inp, pattern))


@functools.lru_cache(maxsize=64)
def emulated(name, mask_name, pattern):
    c, inp = CASE[name], inputs(name)
    return evaluate(c, inp, mask_value(mask_name, c['T']), upstreams(inp, pattern), emu=True)


def param_grads(res, dtype):
    """the 18 parameter gradients formed from a result's kept tensors as ops.RSSMFusedFn.backward forms them: dW = dY^T X over the
    B T rows, db = column sums of dY (plain products in `dtype`)"""
    out = {}
    for dy, x, wn, bn in PARAM_PAIRS:
        d, xx = res[dy].to(dtype).flatten(0, 1), res[x].to(dtype).flatten(0, 1)
        out[wn], out[bn] = d.t() @ xx, d.sum(0)
    return out


# ================================================================================================ one-stage references
def _mv64(x, w, b=None):
    """(reference, denominator) of x w^T + b in float64 over the flattened rows"""
    x, w = x.double(), w.double()
    y, den2 = x @ w.t(), (x * x) @ (w * w).t()
    if b is not None:
        y, den2 = y + b.double(), den2 + b.double() ** 2
    return y, den2.sqrt()


def _shift(x):
    """x[:, t + 1] at position t, zeros at T - 1 (what step t + 1 hands back to step t)"""
    return torch.cat([x[:, 1:], torch.zeros_like(x[:, :1])], 1)


def _bits(mask, T, shift=0):
    """(1, T, 1) bool: bit t + shift of the mask at position t (False where t + shift < 0)"""
    return torch.tensor([bool((mask >> (t + shift)) & 1) if t + shift >= 0 else False for t in range(T)]).view(1, T, 1)


def _gru_pre_scale(gi, gh, h):
    """What the rounding of the three pre-activation sums leaves in h_t, per unit roundoff: each sum is rounded at the scale of its
    two terms and reaches h through the cell's partial derivative.  elementwise_reference's den_hn = |((1 - z) n, z h)| alone
    vanishes where gi_n and r gh_n cancel (n ~ 0 at h ~ 0, as in every first step), and there this term is all the error there is."""
    H = h.shape[1]
    ir, iz, in_ = gi[:, :H], gi[:, H:2 * H], gi[:, 2 * H:]
    hr, hz, hn = gh[:, :H], gh[:, H:2 * H], gh[:, 2 * H:]
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(in_ + r * hn)
    dn = (1 - z) * (1 - n * n)
    return (dn * (in_.abs() + (r * hn).abs()) + dn * hn.abs() * r * (1 - r) * (ir.abs() + hr.abs())
            + (h - n).abs() * z * (1 - z) * (iz.abs() + hz.abs()))


POINTWISE = ('h', 'sigma', 'z', 'dmls', 'dgate')         # stages without a sum of their own: rms of the normalised error


def stages(c, inp, mask, ups, res):
    """[dict(name, kind, K, got, ref, den)] of every stage over all steps at once, each reference formed in float64 from the
    stored inputs of that stage in `res` itself."""
    B, T = c['B'], c['T']
    H, S, E, A = c['dims']
    HP, HQ = H + A, H + E + A
    W = {k: v.double() for k, v in inp.W.items()}
    d = {k: v.detach().cpu().double() for k, v in res.items()}
    noise = inp.noise.double()
    out = []

    def add(name, kind, K, got, ref, den):
        out.append(dict(name=name, kind=kind, K=K, got=got, ref=ref.reshape(got.shape), den=den.reshape(got.shape)))

    def mvs(name, kind, got, x, w, b=None):
        add(name, kind, w.shape[1], got, *_mv64(x.flatten(0, 1), w, b))
    mvs('u', 'u', d['u'], d['zprev'], W['w_pre'], W['b_pre'])
    mvs('gh', 'gh', d['gh'], d['hprev'], W['w_hh'], W['b_hh'])
    mvs('la_p', 'la', d['xp'][..., H:], d['aprev'], W['w_pa'], W['b_pa'])
    mvs('la_q', 'la', d['xq'][..., H + E:], d['aprev'], W['w_qa'], W['b_qa'])
    mvs('gi', 'gi', d['gi'], d['u'], W['w_ih'], W['b_ih'])
    flat = lambda x: x.flatten(0, 1)          # noqa: E731
    ge = EW.gru_eval(flat(d['gi']), flat(d['gh']), flat(d['hprev']), torch.zeros(B * T, H), F64)
    add('h', 'h', 1, d['h'], ge['hn'], ge['den_hn'] + _gru_pre_scale(flat(d['gi']), flat(d['gh']), flat(d['hprev'])))
    mvs('y1p', 'y1', d['y1p'], d['xp'], W['w_p0'], W['b_p0'])
    mvs('y1q', 'y1', d['y1q'], d['xq'], W['w_q0'], W['b_q0'])
    mvs('mls_p', 'mls', d['mls_p'], d['y1p'], W['w_p2'], W['b_p2'])
    mvs('mls_q', 'mls', d['mls_q'], d['y1q'], W['w_q2'], W['b_q2'])
    # ---- backward.  The dz carry of step t + 1 and its mat-vec denominator, from the kept du
    dzc, dzc_den = (_shift(v.reshape(B, T, S)) for v in _mv64(flat(d['du']), W['w_pre'].t()))
    prior_next = _bits(mask, T)
    u64 = {n: (None if t is None else t.double()) for n, t in ups.items()}
    zS = torch.zeros(B, T, S, dtype=F64)
    for post, tag in ((0, 'p'), (1, 'q')):
        se = EW.sample_eval(flat(d['mls_' + tag]), flat(noise[:, :, post]), None, None, None, MIN_STD, F64)
        add('sg_' + tag, 'sigma', 1, d['sg_' + tag], se['sigma'], se['sigma'])
        add('z_' + tag, 'z', 1, d['z_' + tag], se['sample'], se['den_sample'])
        takes = prior_next != bool(post)
        carry, cden = torch.where(takes, dzc, zS), torch.where(takes, dzc_den, zS)
        gz, gmu, gsg = (zS if u64[k + tag] is None else u64[k + tag] for k in ('g_z_', 'g_mu_', 'g_sg_'))
        sb = EW.sample_eval(flat(d['mls_' + tag]), flat(noise[:, :, post]), flat(gmu), flat(gsg), flat(gz + carry), MIN_STD, F64)
        e = noise[:, :, post]
        den = torch.cat([(gmu ** 2 + gz ** 2 + cden ** 2).sqrt(), (gsg ** 2 + (gz * e) ** 2 + (cden * e) ** 2).sqrt()], 2) + EW.TINY
        add('dmls_' + tag, 'dmls', H, d['dmls_' + tag], sb['dmls'], den)
    mvs('dy1p', 'dy1', d['dy1p'], d['dmls_p'], W['w_p2'].t())
    mvs('dy1q', 'dy1', d['dy1q'], d['dmls_q'], W['w_q2'].t())
    dxp, dxp_den = (v.reshape(B, T, HP) for v in _mv64(flat(d['dy1p']), W['w_p0'].t()))
    dxq, dxq_den = (v.reshape(B, T, HQ) for v in _mv64(flat(d['dy1q']), W['w_q0'].t()))
    add('dla_p', 'dx', HP, d['dla_p'], dxp[..., H:], dxp_den[..., H:])
    add('d_emb', 'dx', HQ, d['d_emb'], dxq[..., H:H + E], dxq_den[..., H:H + E])
    add('dla_q', 'dx', HQ, d['dla_q'], dxq[..., H + E:], dxq_den[..., H + E:])
    # g_t, the gradient that reaches h_t: upstream + the two MLP inputs' h slices + the dh carry of step t + 1, rebuilt backwards
    gup = torch.zeros(B, T, H, dtype=F64) if u64['g_h'] is None else u64['g_h']
    g, gden = torch.zeros(B, T, H, dtype=F64), torch.zeros(B, T, H, dtype=F64)
    gate_z = torch.sigmoid(d['gi'][..., H:2 * H] + d['gh'][..., H:2 * H])
    for t in range(T - 1, -1, -1):
        g[:, t] = gup[:, t] + dxp[:, t, :H] + dxq[:, t, :H]
        den2 = gup[:, t] ** 2 + dxp_den[:, t, :H] ** 2 + dxq_den[:, t, :H] ** 2
        if t < T - 1:
            cw, cw_den = _mv64(d['dgh'][:, t + 1], W['w_hh'].t())
            gz1 = g[:, t + 1] * gate_z[:, t + 1]
            g[:, t] += cw + gz1
            den2 = den2 + cw_den ** 2 + gz1 ** 2
        gden[:, t] = den2.sqrt()
    gb = EW.gru_eval(flat(d['gi']), flat(d['gh']), flat(d['hprev']), flat(g), F64)
    dg = (flat(gden) * (1 + flat(d['hprev']).abs() + gb['ghn'].abs()) + EW.TINY).repeat(1, 3)
    add('dgi', 'dgate', HP + HQ + 3 * H, d['dgi'], gb['dgi'], dg)
    add('dgh', 'dgate', HP + HQ + 3 * H, d['dgh'], gb['dgh'], dg)
    mvs('du', 'du', d['du'], d['dgi'], W['w_ih'].t())
    return out


def copies(c, inp, mask, res):
    """[(name, got, expected)]: what the kernels copy, to be compared bit for bit"""
    H, S, E, A = c['dims']
    T = c['T']
    r = {k: v.detach().cpu() for k, v in res.items()}
    prev = lambda x: torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)          # noqa: E731
    sel = torch.where(_bits(mask, T, -1), prev(r['z_p']), prev(r['z_q']))
    return [('hprev', r['hprev'], prev(r['h'])), ('zprev', r['zprev'], sel), ('aprev', r['aprev'], prev(inp.act.to(r['aprev'].dtype))),
            ('xp[:H]', r['xp'][..., :H], r['h']), ('xq[:H]', r['xq'][..., :H], r['h']),
            ('xq[emb]', r['xq'][..., H:H + E], inp.emb.to(r['xq'].dtype)), ('mu_p', r['mu_p'], r['mls_p'][..., :S]),
            ('mu_q', r['mu_q'], r['mls_q'][..., :S])]


# ================================================================================================ bars
# Per stage, (rms, max e) = (c_rms, c_e) u sqrt(K), u = 2^-24, K the stage's reduction length (1 for the pointwise stages h, sigma,
# z; H for dmls, whose dz carry is a K = H mat-vec; HP + HQ + 3H for dgi / dgh, whose g sums three mat-vecs).
#   A stage whose float32 emulation stays within HALF of conv_reference.f32_bar(K) = (0.46, 4.8) over every run of the case list
#     (runs(): every case x mask, every upstream pattern) is held to f32_bar(K).
#   Every other stage gets its own bar: 2 x the worst (rms, max e) of the emulation, in units of u sqrt(K) (STAGE_OWN_WORST).
#     These are the short sums (K = 1 ... 12 at the smallest dims, where every product and the bias are rounded and nothing
#     averages) and the pointwise stages.  tests/test_rssm_reference.py recomputes the table and fails when it is stale.
#   End to end over the T steps (the 7 outputs, d_emb, the 18 parameter gradients formed as dY^T X and column sums):
#     e = max |got - ref64| / max |ref64| per tensor, bar = 4 x the e of the float32 emulation on the same inputs (E2E_MEASURED,
#     per case at its first mask with all upstreams: the largest e among the 7 outputs, that of d_emb, the largest among the 18
#     parameter gradients; the margin attention_reference uses).  A tensor of 4 elements has no worst case of its own worth 4 x,
#     so every tensor is held to its group's figure.  Recomputed by the CPU test.
# None of these numbers comes from a GPU.
STAGE_OWN_WORST = {          # emulation: worst (rms, max e) / (u sqrt(K)) over runs(); 'dgate' (0.066, 0.603) stays under f32_bar
    'u': (0.566, 1.390), 'gh': (0.503, 1.886), 'la': (0.566, 1.702), 'gi': (0.504, 1.723), 'h': (0.772, 10.764),
    'y1': (0.421, 1.337), 'mls': (0.427, 1.616), 'sigma': (0.961, 2.357), 'z': (0.985, 3.647),
    'dmls': (0.278, 1.542), 'dy1': (0.341, 1.518), 'dx': (0.440, 1.502), 'du': (0.397, 1.242),
}
E2E_MEASURED = {             # emulation: largest max |got - ref64| / max |ref64| per group of tensors
    'tiny-b3-t5': {'out': 1.56e-07, 'd_emb': 1.61e-07, 'dparam': 1.93e-07},
    'tiny-b64-t1': {'out': 1.82e-07, 'd_emb': 1.11e-07, 'dparam': 3.35e-07},
    'tiny-b1-t64': {'out': 2.15e-07, 'd_emb': 1.55e-07, 'dparam': 3.78e-07},
    'sub256-b5-t2': {'out': 3.71e-07, 'd_emb': 1.31e-07, 'dparam': 2.19e-07},
    'pass2-b8-t2': {'out': 5.54e-07, 'd_emb': 1.47e-07, 'dparam': 3.69e-07},
    'k256-b4-t2': {'out': 3.40e-07, 'd_emb': 1.05e-07, 'dparam': 2.68e-07},
    'k1024-b1-t2': {'out': 9.74e-08, 'd_emb': 2.13e-07, 'dparam': 2.28e-07},
    'lds-limit-b4-t1': {'out': 1.31e-07, 'd_emb': 2.03e-07, 'dparam': 1.88e-07},
}


# Measured on an MI355X by tests/test_rssm_kernels_gpu.py (RSSMSTAT lines: largest max e / rms over every case, mask and upstream
# pattern of a stage kind, and the largest share of its bar).  Records, not the source of any bar.
#   u      4.05e-7 / 8.68e-8 (0.59)   gh   3.77e-7 / 6.26e-8 (0.52)   la    1.58e-7 / 4.63e-8 (0.50)   gi  4.91e-7 / 8.43e-8 (0.50)
#   h      6.19e-7 / 4.39e-8 (0.48)   y1   4.13e-7 / 7.94e-8 (0.56)   mls   4.79e-7 / 8.17e-8 (0.50)   sigma 1.40e-7 / 5.67e-8 (0.50)
#   z      2.09e-7 / 5.45e-8 (0.48)   dmls 3.66e-7 / 3.70e-8 (0.55)   dy1   4.66e-7 / 1.58e-7 (0.49)   dx  3.10e-7 / 1.93e-7 (0.56)
#   dgi / dgh (f32_bar) 2.91e-7 / 2.33e-8 (0.15)                      du    4.98e-7 / 9.50e-8 (0.50)
#   (a share of 0.50 of an own bar is the emulation's own worst case: the kernel rounds as emulated.  Where the stage's inputs come
#   through expf / tanhf - z_prev, y1 of h, the carries - the device's last bit differs from the host's, the stage sees slightly
#   other inputs than the emulation did and draws another sample of the same roundings: 0.48 ... 0.59)
#   end to end: outputs 5.2e-7 (0.50 of 4 x the emulation's e), d_emb 2.1e-7 (0.34), parameter gradients 4.6e-7 (0.35)
#   bit for bit: every copy (hprev, zprev, aprev, the h / embedding slices of x*, mu), two runs, masks that differ in bits >= T - 1,
#   MUVO_RSSM_GRID = 1 and 3 against the default grid of 256, frozen against unfrozen parameter gradients, the model against the C ABI


def stage_bar(kind, K):
    r = math.sqrt(max(K, 1)) * U32
    if kind in STAGE_OWN_WORST:
        return (2 * STAGE_OWN_WORST[kind][0] * r, 2 * STAGE_OWN_WORST[kind][1] * r)
    return f32_bar(K)


def stage_stats(s):
    return (EW.norm_stats if s['kind'] in POINTWISE else error_stats)(s['got'], s['ref'], s['den'])


def locate(c, s, index):
    b, t = index[0], index[1]
    return f'stage {s["name"]} step {t} sequence {b} (slab {b // BM}) row {index[2]}, K = {s["K"]}'


def judge(c, inp, mask, ups, res, label='', emit=None):
    """Every per-stage and bit-for-bit check of one result.  Returns (failures, [(stage name, kind, K, stats, share)])."""
    fails, rows = [], []
    for name, got, want in copies(c, inp, mask, res):
        if not torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)):
            bad = (got != want).nonzero()
            fails.append(f'{label} copy {name}: {len(bad)} elements differ, first at (sequence, step, row) {tuple(bad[0].tolist())}')
    for s in stages(c, inp, mask, ups, res):
        st, bar = stage_stats(s), stage_bar(s['kind'], s['K'])
        share = excess(st, bar)
        rows.append((s['name'], s['kind'], s['K'], st, share))
        if emit:
            emit(f'RSSMSTAT {label} {s["name"]}: max e {st["max_e"]:.3e} rms {st["rms"]:.3e} share {share:.2f}')
        if not within(st, bar):
            fails.append(f'{label} {locate(c, s, st["index"])}: max e {st["max_e"]:.3e} rms {st["rms"]:.3e} bar {bar}')
    return fails, rows


def stage_worst():
    """{kind: [rms, max e] in units of u sqrt(K)}: the emulation's worst over runs()"""
    w = collections.defaultdict(lambda: [0.0, 0.0])
    for name, m, p in runs():
        c, inp = CASE[name], inputs(name)
        for s in stages(c, inp, mask_value(m, c['T']), upstreams(inp, p), emulated(name, m, p)):
            st, r = stage_stats(s), math.sqrt(max(s['K'], 1)) * U32
            w[s['kind']] = [max(w[s['kind']][0], st['rms'] / r), max(w[s['kind']][1], st['max_e'] / r)]
    return dict(w)


E2E_GROUPS = {'out': OUT7, 'd_emb': ('d_emb',), 'dparam': WNAMES}
E2E_GROUP_OF = {n: g for g, names in E2E_GROUPS.items() for n in names}


def e2e_errors(ref, got):
    """{name: max |got - ref| / max |ref|} over the names present in `got` (a reference that is zero throughout, such as dW_pre
    at T = 1 where z_prev = 0, leaves max |got|: it has to be met exactly)"""
    out = {}
    for n, g in E2E_GROUP_OF.items():
        if n in got:
            rf = ref[n].double()
            scale = float(rf.abs().max())
            out[n] = float((got[n].detach().cpu().double() - rf).abs().max()) / (scale if scale > 0 else 1.0)
    return out


@functools.lru_cache(maxsize=None)
def e2e_reference(name):
    """float64 outputs, d_emb and parameter gradients of a case at its first mask with all upstreams"""
    r = reference64(name, CASE[name]['masks'][0], 'all')
    return dict({n: r[n] for n in OUT7 + ('d_emb',)}, **param_grads(r, F64))


def e2e_measure(name):
    """{group: the emulation's largest e over the group's tensors}"""
    r = emulated(name, CASE[name]['masks'][0], 'all')
    e = e2e_errors(e2e_reference(name), dict({n: r[n] for n in OUT7 + ('d_emb',)}, **param_grads(r, F32)))
    return {g: max(e[n] for n in names) for g, names in E2E_GROUPS.items()}


def e2e_bar(name, tensor):
    return 4 * E2E_MEASURED[name][E2E_GROUP_OF[tensor]]


def saturation(name):
    """share of GRU gate (r, z) and sigma (log sigma / 2) pre-activations with |x| > 8 in the float64 reference"""
    c = CASE[name]
    H, S = c['dims'][:2]
    r = reference64(name, c['masks'][0], 'all')
    gates = (r['gi'] + r['gh'])[..., :2 * H]
    ls = torch.cat([r['mls_p'][..., S:], r['mls_q'][..., S:]], -1) * 0.5
    return float((gates.abs() > 8).double().mean()), float((ls.abs() > 8).double().mean())


# ================================================================================================ the C ABI on a GPU
MARKER = -12345.678          # canary value of the guard words and of the row past B T of every buffer (compared bit for bit)
GUARD = 8                    # guard floats in front of and behind a buffer (a multiple of 4: the data stays 16-byte aligned)


class Guarded:
    """a device buffer of `rows` x `width` floats with GUARD marker floats in front, one marker row past the last row and GUARD marker
    floats behind; the payload starts as NaN (a result the kernels must overwrite) or as `data`"""

    def __init__(self, dev, rows, width, data=None):
        self.n = rows * width
        self.store = torch.full((GUARD + self.n + width + GUARD,), MARKER, device=dev)
        self.t = self.store[GUARD:GUARD + self.n]
        if data is None:
            self.t.fill_(float('nan'))
        else:
            self.t.copy_(data.reshape(-1))
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        s = self.store.cpu()
        want = torch.full_like(s, MARKER)
        outside = torch.cat([s[:GUARD], s[GUARD + self.n:]]).view(torch.int32)
        return torch.equal(outside, torch.cat([want[:GUARD], want[GUARD + self.n:]]).view(torch.int32))


def gpu_run(dev, c, inp, mask, ups, backward=True):
    """muvo_rssm_forward (and muvo_rssm_backward) through ctypes on guarded, NaN-poisoned buffers.  Returns
    (results {name: (B, T, .) CPU tensor}, info dict(G_fwd, G_bwd, err, broken: names of buffers whose canaries changed))."""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    B, T, AD = c['B'], c['T'], c['AD']
    H, S, E, A = c['dims']
    wd = widths(c)
    rows = B * T
    W = [inp.W[n].to(dev).contiguous() for n in WNAMES]
    emb, act, noise = inp.emb.to(dev).contiguous(), inp.act.to(dev).contiguous(), inp.noise.to(dev).contiguous()
    buf = {n: Guarded(dev, rows, wd[n]) for n in OUT7 + KEEP12}
    bar = torch.zeros(4, device=dev, dtype=torch.int32)
    tab = lambda names: ops._ptr_table([buf[n].t for n in names])          # noqa: E731
    ops._ck(L.muvo_rssm_forward(B, T, H, S, E, A, AD, ops._ptr_table(W), ops._f(emb), ops._f(act), ops._f(noise), C.c_uint64(mask),
                                tab(OUT7), tab(KEEP12), ops._p(bar), ops._fl(MIN_STD), ops._st()))
    torch.cuda.synchronize()
    words = bar.cpu().tolist()
    info = dict(err=words[1], G_fwd=words[0] / (4 * T), G_bwd=None)
    if backward:
        for n in GRAD10:
            buf[n] = Guarded(dev, rows, wd[n])
        buf['wt_scratch'] = Guarded(dev, 1, int(L.muvo_rssm_transposed_floats(H, S, E, A)))
        buf['scratch'] = Guarded(dev, 1, int(L.muvo_rssm_scratch_floats(B, H, S, E, A)))
        up = [None if ups[n] is None else ups[n].to(dev).contiguous() for n in UP7]
        ops._ck(L.muvo_rssm_backward(B, T, H, S, E, A, AD, ops._ptr_table(W), ops._f(buf['wt_scratch'].t), ops._f(noise),
                                     C.c_uint64(mask), tab(KEPT5), ops._ptr_table(up), tab(GRAD10), ops._f(buf['scratch'].t),
                                     ops._p(bar), ops._st()))
        torch.cuda.synchronize()
        words = bar.cpu().tolist()
        info['err'] |= words[1]
        info['G_bwd'] = words[0] / (4 * T)
    info['broken'] = [n for n, b in buf.items() if not b.intact()]
    res = {n: b.t.cpu().view(B, T, wd[n]) for n, b in buf.items() if n in wd}
    return res, info


def crcs(res):
    return {n: zlib.crc32(res[n].contiguous().numpy().tobytes()) for n in sorted(res)}


if __name__ == '__main__':
    print('STAGE_OWN_WORST = {')
    for k, (rms, e) in sorted(stage_worst().items()):
        own = rms > 0.23 or e > 2.4
        print(f"    {'' if own else '# '}'{k}': ({rms:.3f}, {e:.3f}),")
    print('}\nE2E_MEASURED = {')
    for c in CASES:
        m = e2e_measure(c['name'])
        print(f"    '{c['name']}': {{" + ', '.join(f"'{n}': {v:.2e}" for n, v in m.items()) + '},')
    print('}')
