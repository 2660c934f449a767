"""Float64 reference, float32 restatement of the softmax recurrence, case lists, spiked inputs and the comparison for the fused
attention kernels (muvo_amd/csrc/attention.hip), one unit with two paths: streamed (K / V blocks of BK rows under an online
softmax, any L) and resident (K / V of a head whole in LDS, L <= 384: the same recurrence with ONE block, which is the two-pass
softmax and the unblocked dQ sum).  Helpers only: no fixtures, no tests.
tests/test_attention_reference.py (CPU) and tests/test_attention_stream_gpu.py (GPU) share everything here, so the bars the GPU
test applies are the ones the CPU test proves to reject planted errors.  The metric (error_stats) and the seeded generator are
those of tests/loss_reference.py.

Layout.  qkv (L, N, 3E) packed q | k | v, heads contiguous inside each; o (L, N, E); lse (N * H, L); dqkv like qkv.

The metric.  e = max |got - ref64| / max |ref64|, per tensor: o, lse, dqkv.

The bar.  One for every float64 comparison: 4 x the e of blocked_float32() - the recurrence the forward kernel runs (running
maximum m, running sum l, O rescaled by exp(m_old - m_new) per block of BK keys, divided by l at the end; backward from the row
log-sum-exp, key block by key block), evaluated in float32 torch on the CPU with the block of the case's path (float32_block:
BK for a streamed case, the whole row for a resident one, id suffix -res) - on the same inputs, tabulated per case in MEASURED
(`python tests/attention_reference.py` prints the table).  The factor 4 is what tests/norm_reference.py allows for another
summation order.  Never the kernels' own error.  The dropout cases are tabulated with a CPU Bernoulli keep-mask of the same p
(the GPU test takes the mask the library generates: same statistics, other bits).

Spiked inputs (a data-dependent rescale needs an input that forces it).  For every 7th query i the key
j = min((i mod nblocks) * BK + (13 i mod BK), L - 1) is set to 10 q_i (per frame and head): that row's largest score, 10 |q_i|^2
/ sqrt(DH), lies beyond float32 exp's overflow point (88.7) and first appears in block 0 for some rows, in a middle block for
others, in the last block for others.  spiked_facts() asserts all of that.  A kernel that loses track of the running maximum
returns inf / NaN instead of a small error."""
import functools

import torch

from loss_reference import _gen, error_stats, scale_of

F64 = torch.float64
BQ, BK = 128, 128          # what muvo_attention_stream_blocks reports (asserted by both tests): MEASURED is for this BK
NAMES = ('o', 'lse', 'dqkv')


# ================================================================================================ cases
def case(L, N, H, DH, spiked=False, p=0.0, res=False):
    return dict(L=L, N=N, H=H, DH=DH, spiked=spiked, p=p, res=res)


def case_id(c):
    return f'L{c["L"]}-N{c["N"]}H{c["H"]}D{c["DH"]}' + ('-spiked' if c['spiked'] else '') + (f'-p{c["p"]}' if c['p'] else '') + \
        ('-res' if c['res'] else '')


PARITY_CASES = [case(L, 2, 2, 48) for L in (1, 15, BK - 1, BK, BK + 1, 385, 2 * BK + 23, 1037)] + \
               [case(2 * BK + 23, 1, 3, DH) for DH in (16, 32, 64)]       # odd head count: a swapped n / h split shows
BIG_CASE = case(5184, 1, 1, 48)                                           # 41 key blocks: the token count of the next size class
SPIKED_CASES = [case(2 * BK + 23, 2, 2, 48, spiked=True), case(1037, 2, 2, 48, spiked=True)] + \
               [case(1037, 1, 2, DH, spiked=True) for DH in (16, 64)]
DROPOUT_CASES = [case(517, 2, 4, 48, p=p) for p in (0.1, 0.5)]
STREAM_CASES = PARITY_CASES + [BIG_CASE] + SPIKED_CASES + DROPOUT_CASES
# The resident path (res=True: its own ids, the same (L, N, H, DH) has another float32 evaluation there).  DH = 48: one key, one
# key tile and its edges, 128 queries per workgroup (the last wave's rows; a second workgroup with seven idle waves), the model's
# L, all RES_MAXT register tiles; the other head sizes on an odd head count; the largest L whose dK / dV LDS fits at DH = 64.
RES_WG, RES_MAXL, RES_MAXL_D64 = 128, 384, 288
RESIDENT_CASES = [case(L, 2, 2, 48, res=True) for L in (1, 15, 16, 17, RES_WG - 1, RES_WG, RES_WG + 1, 324, RES_MAXL - 1, RES_MAXL)] + \
                 [case(279, 1, 3, DH, res=True) for DH in (16, 32, 64)] + [case(RES_MAXL_D64, 2, 2, 64, res=True)]
RESIDENT_DROPOUT_CASES = [case(324, 2, 4, 48, p=p, res=True) for p in (0.1, 0.5)]
ALL_CASES = STREAM_CASES + RESIDENT_CASES + RESIDENT_DROPOUT_CASES
DROPOUT_SEEDS = {0.1: 77, 0.5: 123456789}

# e of blocked_float32(bk = float32_block(case)) against reference64 (this file run as a script; 16 CPU threads)
MEASURED = {
    'L1-N2H2D48': {'o': 0.00e+00, 'lse': 3.96e-08, 'dqkv': 4.76e-07},       # one key: p = 1, o = v exactly
    'L15-N2H2D48': {'o': 2.47e-07, 'lse': 8.84e-08, 'dqkv': 2.81e-07},
    'L127-N2H2D48': {'o': 6.01e-07, 'lse': 8.08e-08, 'dqkv': 7.74e-07},
    'L128-N2H2D48': {'o': 6.14e-07, 'lse': 8.41e-08, 'dqkv': 6.77e-07},
    'L129-N2H2D48': {'o': 6.35e-07, 'lse': 8.09e-08, 'dqkv': 3.62e-07},
    'L385-N2H2D48': {'o': 6.58e-07, 'lse': 7.10e-08, 'dqkv': 9.78e-07},
    'L279-N2H2D48': {'o': 3.91e-07, 'lse': 7.00e-08, 'dqkv': 7.86e-07},
    'L1037-N2H2D48': {'o': 1.19e-06, 'lse': 7.76e-08, 'dqkv': 6.73e-07},
    'L279-N1H3D16': {'o': 4.09e-07, 'lse': 6.43e-08, 'dqkv': 5.47e-07},
    'L279-N1H3D32': {'o': 7.47e-07, 'lse': 6.95e-08, 'dqkv': 5.19e-07},
    'L279-N1H3D64': {'o': 4.72e-07, 'lse': 7.63e-08, 'dqkv': 1.07e-06},
    'L5184-N1H1D48': {'o': 7.84e-07, 'lse': 9.85e-08, 'dqkv': 1.08e-06},
    'L279-N2H2D48-spiked': {'o': 1.86e-06, 'lse': 2.72e-07, 'dqkv': 1.50e-06},
    'L1037-N2H2D48-spiked': {'o': 3.02e-06, 'lse': 2.33e-07, 'dqkv': 2.13e-06},
    'L1037-N1H2D16-spiked': {'o': 1.26e-06, 'lse': 1.46e-07, 'dqkv': 2.03e-06},
    'L1037-N1H2D64-spiked': {'o': 2.89e-06, 'lse': 2.53e-07, 'dqkv': 2.62e-06},
    'L517-N2H4D48-p0.1': {'o': 1.34e-06, 'lse': 9.66e-08, 'dqkv': 8.45e-07},
    'L517-N2H4D48-p0.5': {'o': 1.59e-06, 'lse': 9.66e-08, 'dqkv': 1.00e-06},
    # resident path: blocked_float32 with one block (bk = L), the two-pass softmax and the unblocked dQ sum
    'L1-N2H2D48-res': {'o': 0.00e+00, 'lse': 3.96e-08, 'dqkv': 4.76e-07},
    'L15-N2H2D48-res': {'o': 2.47e-07, 'lse': 8.84e-08, 'dqkv': 2.81e-07},
    'L16-N2H2D48-res': {'o': 2.95e-07, 'lse': 8.08e-08, 'dqkv': 2.95e-07},
    'L17-N2H2D48-res': {'o': 3.77e-07, 'lse': 9.07e-08, 'dqkv': 3.76e-07},
    'L127-N2H2D48-res': {'o': 6.01e-07, 'lse': 8.08e-08, 'dqkv': 7.74e-07},
    'L128-N2H2D48-res': {'o': 6.14e-07, 'lse': 8.41e-08, 'dqkv': 6.77e-07},
    'L129-N2H2D48-res': {'o': 5.62e-07, 'lse': 8.09e-08, 'dqkv': 3.62e-07},
    'L324-N2H2D48-res': {'o': 5.18e-07, 'lse': 6.97e-08, 'dqkv': 6.37e-07},
    'L383-N2H2D48-res': {'o': 7.19e-07, 'lse': 7.03e-08, 'dqkv': 9.93e-07},
    'L384-N2H2D48-res': {'o': 8.41e-07, 'lse': 7.93e-08, 'dqkv': 9.16e-07},
    'L279-N1H3D16-res': {'o': 5.61e-07, 'lse': 6.85e-08, 'dqkv': 5.65e-07},
    'L279-N1H3D32-res': {'o': 7.63e-07, 'lse': 7.08e-08, 'dqkv': 5.88e-07},
    'L279-N1H3D64-res': {'o': 6.55e-07, 'lse': 7.72e-08, 'dqkv': 1.07e-06},
    'L288-N2H2D64-res': {'o': 6.91e-07, 'lse': 8.17e-08, 'dqkv': 1.02e-06},
    'L324-N2H4D48-p0.1-res': {'o': 7.26e-07, 'lse': 7.28e-08, 'dqkv': 1.12e-06},
    'L324-N2H4D48-p0.5-res': {'o': 8.61e-07, 'lse': 7.28e-08, 'dqkv': 7.19e-07},
}
BARS = {k: {n: 4 * e for n, e in v.items()} for k, v in MEASURED.items()}


# ================================================================================================ inputs
def _heads(t, H):
    """(L, N, H * DH) -> (N, H, L, DH)"""
    L, N, E = t.shape
    return t.reshape(L, N, H, E // H).permute(1, 2, 0, 3)


def _packed(t):
    """(N, H, L, DH) -> (L, N, H * DH)"""
    N, H, L, DH = t.shape
    return t.permute(2, 0, 1, 3).reshape(L, N, H * DH)


def spike_key(i, L, bk=BK):
    nblocks = -(-L // bk)
    return min((i % nblocks) * bk + (13 * i) % bk, L - 1)


def inputs(c):
    """qkv (L, N, 3E) and dout (L, N, E), float32, seeded by the case; p > 0: also `cpu_keep` (N, H, L, L), 0 or 1 / (1 - p),
    which stands in for the library's mask where there is no GPU"""
    L, N, E = c['L'], c['N'], c['H'] * c['DH']
    g = _gen('attention', L, N, c['H'], c['DH'], c['spiked'])
    qkv = torch.randn(L, N, 3 * E, generator=g)
    dout = torch.randn(L, N, E, generator=g)
    if c['spiked']:
        for i in range(0, L, 7):                     # ascending: a later query overwrites an earlier one's key
            qkv[spike_key(i, L), :, E:2 * E] = 10.0 * qkv[i, :, :E]
    out = {'qkv': qkv, 'dout': dout}
    if c['p']:
        out['cpu_keep'] = (torch.rand(N, c['H'], L, L, generator=g) >= c['p']).float() / (1 - c['p'])
    return out


def spiked_facts(c, qkv):
    """asserts what the spiked inputs are for; returns (largest |score|, {where: rows whose maximum first appears there})"""
    L, E, H = c['L'], c['H'] * c['DH'], c['H']
    q, k = _heads(qkv[:, :, :E].double(), H), _heads(qkv[:, :, E:2 * E].double(), H)
    s = q @ k.transpose(-1, -2) / c['DH'] ** 0.5
    smax = float(s.abs().max())
    assert 89 < smax < 200, smax
    nblocks = -(-L // BK)
    rows = list(range(0, L, 7))
    blk = s[:, :, rows].argmax(-1) // BK            # (N, H, spiked rows)
    where = {'first': int((blk == 0).sum()), 'middle': int(((blk > 0) & (blk < nblocks - 1)).sum()), 'last': int((blk == nblocks - 1).sum())}
    assert all(v > 0 for v in where.values()), where
    return smax, where


# ================================================================================================ float64 reference
def reference64(qkv, heads, dout, keep=None):
    """The attention core with every L x L matrix written out, in float64: o = (softmax(q k^T / sqrt(DH)) * keep) v, lse the row
    log-sum-exp of the scaled scores, dqkv under the upstream dout (formulas, not autograd; the CPU test checks them against it)"""
    E = qkv.shape[-1] // 3
    scale = (E // heads) ** -0.5
    q, k, v = (_heads(qkv[:, :, i * E:(i + 1) * E].double(), heads) for i in range(3))
    do = _heads(dout.double(), heads)
    s = q @ k.transpose(-1, -2)
    s *= scale
    lse = torch.logsumexp(s, -1)
    P = s.sub_(lse[..., None]).exp_()
    Pd = P if keep is None else P * keep.double()
    o = Pd @ v
    dv = Pd.transpose(-1, -2) @ do
    del Pd
    dP = do @ v.transpose(-1, -2)
    if keep is not None:
        dP *= keep.double()
    D = (do * o).sum(-1, keepdim=True)              # = sum_j dP_j P_j
    dS = dP.sub_(D).mul_(P)
    dq = (dS @ k) * scale
    dk = (dS.transpose(-1, -2) @ q) * scale
    return {'o': _packed(o), 'lse': lse.reshape(-1, lse.shape[-1]), 'dqkv': torch.cat([_packed(dq), _packed(dk), _packed(dv)], -1)}


# ================================================================================================ the recurrence, blocked
def blocked(qkv, heads, bk, dout=None, keep=None, dtype=torch.float32, fault=None):
    """Online softmax over key blocks of bk rows, in `dtype` on the CPU.  Forward: per block m' = max(m, block max),
    a = exp(m - m'), l = l a + sum exp(s - m'), O = O a + (exp(s - m') * keep) V; at the end o = O / l, lse = m + log l.  Backward
    (dout given): p = exp(s - lse) per key block, D = dout . o, dS = p (dP keep - D); dq summed over the blocks.
    fault: one planted error for the CPU test, (kind, block, (n, h, query)):
      'o_rescale'  O of that query is not multiplied by a at that block
      'l_rescale'  l of that query is not multiplied by a at that block
      'tail_key'   one key >= L of the last block is counted with score 0 (and V = 0) for every query"""
    E = qkv.shape[-1] // 3
    dh = E // heads
    scale = torch.tensor(dh ** -0.5, dtype=dtype)
    q, k, v = (_heads(qkv[:, :, i * E:(i + 1) * E].to(dtype), heads) for i in range(3))
    N, H, L, _ = q.shape
    kp = None if keep is None else keep.to(dtype)
    m = torch.full((N, H, L), float('-inf'), dtype=dtype)
    l = torch.zeros(N, H, L, dtype=dtype)
    O = torch.zeros(N, H, L, dh, dtype=dtype)
    kind, fblock, fidx = fault if fault else (None, None, None)
    for b, k0 in enumerate(range(0, L, bk)):
        k1 = min(k0 + bk, L)
        s = (q @ k[:, :, k0:k1].transpose(-1, -2)) * scale
        mn = torch.maximum(m, s.max(-1).values)
        a = torch.exp(m - mn)
        p = torch.exp(s - mn[..., None])
        ps = p.sum(-1)
        if kind == 'tail_key' and k1 == L:
            ps = ps + torch.exp(-mn)
        al, ao = a, a
        if kind == 'l_rescale' and b == fblock:
            al = a.clone()
            al[fidx] = 1.0
        if kind == 'o_rescale' and b == fblock:
            ao = a.clone()
            ao[fidx] = 1.0
        l = l * al + ps
        if kp is not None:
            p = p * kp[:, :, :, k0:k1]
        O = O * ao[..., None] + p @ v[:, :, k0:k1]
        m = mn
    o = O / l[..., None]
    lse = m + torch.log(l)
    out = {'o': _packed(o), 'lse': lse.reshape(N * H, L), 'alpha_last': a}
    if dout is None:
        return out
    do = _heads(dout.to(dtype), heads)
    D = (do * o).sum(-1, keepdim=True)
    dq = torch.zeros_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    for k0 in range(0, L, bk):
        k1 = min(k0 + bk, L)
        kb, vb = k[:, :, k0:k1], v[:, :, k0:k1]
        p = torch.exp((q @ kb.transpose(-1, -2)) * scale - lse[..., None])
        dP = do @ vb.transpose(-1, -2)
        pd = p
        if kp is not None:
            dP = dP * kp[:, :, :, k0:k1]
            pd = p * kp[:, :, :, k0:k1]
        dS = p * (dP - D)
        dq += dS @ kb
        dk[:, :, k0:k1] = (dS.transpose(-1, -2) @ q) * scale
        dv[:, :, k0:k1] = pd.transpose(-1, -2) @ do
    out['dqkv'] = torch.cat([_packed(dq * scale), _packed(dk), _packed(dv)], -1)
    return out


def blocked_float32(qkv, heads, bk, dout=None, keep=None):
    return blocked(qkv, heads, bk, dout, keep, torch.float32)


# ================================================================================================ comparison
def compare(cid, got, ref):
    """{name: (stats, bar)} of o, lse, dqkv (those `got` has) against the float64 reference, each normalised by its max |ref|;
    the bar is 4 x MEASURED[cid][name]"""
    return {n: (error_stats(got[n], ref[n], scale_of(ref[n])), BARS[cid][n]) for n in NAMES if n in got}


def failures(cmp):
    return {n: (s, bar) for n, (s, bar) in cmp.items() if not s['max_e'] <= bar}


def statlines(tag, cmp):
    return [f'ATTNSTAT {tag} {n}: {s["max_e"]:.3e} {s["rms"]:.3e} ({bar:.2e})' for n, (s, bar) in cmp.items()]


@functools.lru_cache(maxsize=None)
def _reference_cached(cid):
    c = next(c for c in ALL_CASES if case_id(c) == cid)
    inp = inputs(c)
    return inp, reference64(inp['qkv'], c['H'], inp['dout'], inp.get('cpu_keep'))


def reference(c):
    """(inputs, float64 reference with the CPU keep-mask if p > 0) of a listed case, computed once per process; read-only"""
    return _reference_cached(case_id(c))


def float32_block(c):
    """key rows per block of the float32 evaluation: BK on the streamed path, the whole head (one block) on the resident one"""
    return c['L'] if c['res'] else BK


def float32_errors(c):
    """{name: e} of blocked_float32 on the case's inputs, with the block of the case's path"""
    inp, ref = reference(c)
    sub = blocked_float32(inp['qkv'], c['H'], float32_block(c), inp['dout'], inp.get('cpu_keep'))
    return {n: error_stats(sub[n], ref[n], scale_of(ref[n]))['max_e'] for n in NAMES}


if __name__ == '__main__':
    for c in ALL_CASES:
        e = float32_errors(c)
        _reference_cached.cache_clear()
        print(f"    '{case_id(c)}': {{" + ', '.join(f"'{n}': {v:.2e}" for n, v in e.items()) + '},', flush=True)
