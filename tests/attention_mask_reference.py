"""Float64 reference, float32 restatement of the recurrence, case list and bars for the key-padding mask of the fused attention
kernels (muvo_amd/csrc/attention.hip: muvo_attention_mask_* resident, muvo_attention_stream_mask_* streamed).  Helpers only: no
fixtures, no tests; everything that is not about the mask (layout, metric, seeded inputs, spiked inputs, comparison) is
tests/attention_reference.py's, imported and unchanged.  tests/test_attention_mask_reference.py (CPU) and
tests/test_attention_mask_gpu.py (GPU) share this file, so the bars the GPU test applies are the ones the CPU test proves to reject
planted errors.

The mask.  key_mask (N, L) bool, True = the key is ignored by every query and head of its frame (torch's src_key_padding_mask).
A masked key has the score -inf BEFORE the row maximum is taken; queries are never masked.  A row with no live key - here always a
whole frame, since the mask is per frame - is DEFINED as o = 0, lse = -inf, dqkv = 0 (torch gives NaN).

The bar.  The rule of tests/attention_reference.py: 4 x the error e = max |got - ref64| / max |ref64| (over the finite elements; a
-inf of the reference must be a -inf of the result) of blocked_masked() - the online-softmax recurrence with the mask and the
guards the kernels need, in float32 torch on the CPU with the block of the case's path (BK streamed, the whole row resident) - on
the same inputs, tabulated per case in MEASURED (`python tests/attention_mask_reference.py` prints the table).  Never the kernels'
own error.  The dropout cases are tabulated with a CPU Bernoulli keep-mask of the same p, as there.

Cases.  DH = 48, H = 2, N = 3 frames with DIFFERENT masks per frame unless noted, so a mask indexed by the wrong frame or by the head
shows.  A mask is written as one list per frame of (start, stop[, step]) key ranges."""
import functools

import torch

import attention_reference as R
from attention_reference import BK, F64, NAMES, _heads, _packed
from loss_reference import error_stats, scale_of

CAMERA, LIDAR = [(0, 260)], [(260, 324)]                 # the model's tokens: 260 image, 64 range-view


# ================================================================================================ cases
def mcase(name, frames, L, N=3, H=2, DH=48, spiked=False, p=0.0, res=False, boost=1.0):
    """boost: the K rows of the masked keys are multiplied by it (inputs()).  Nothing of the reference depends on a masked key,
    so the reference is that of boost = 1; a kernel that lets a masked score into the maximum sees scores `boost` times as large"""
    assert len(frames) == N
    return dict(R.case(L, N, H, DH, spiked, p, res), mask=name, frames=frames, boost=boost)


def case_id(c):
    return R.case_id(c) + '-' + c['mask']


def key_mask(c):
    """(N, L) bool of a case"""
    m = torch.zeros(c['N'], c['L'], dtype=torch.bool)
    for n, ranges in enumerate(c['frames']):
        for r in ranges:
            m[n, slice(*r)] = True
    return m


def inputs(c):
    """R.inputs(c) with 'key_mask' (N, L) bool, the masked keys' K rows times c['boost']"""
    inp = dict(R.inputs(c), key_mask=key_mask(c))
    if c['boost'] != 1.0:
        E = c['H'] * c['DH']
        inp['qkv'] = inp['qkv'].clone()
        inp['qkv'][:, :, E:2 * E][inp['key_mask'].T] *= c['boost']
    return inp


def _spike_keys(L, first):
    """the spike key of every other spiked row (rows first, first + 14, ...; the spiked rows are every 7th)"""
    return [(k, k + 1) for k in sorted({R.spike_key(i, L) for i in range(first, L, 14)})]


RESIDENT_CASES = [
    mcase('none', [[], [], []], 1, res=True),
    mcase('key0', [[], [(0, 1)], []], 1, res=True),                                     # frame 1: the all-masked frame
    mcase('key16', [[(16, 17)], [], [(16, 17), (3, 4)]], 17, res=True),
    mcase('tile0', [[(0, 16)], [], [(1, 17)]], 17, res=True),                           # the whole first tile
    mcase('sensors', [[], CAMERA, LIDAR], 324, res=True),                               # the model's length
    mcase('lasttile', [[(368, 384)], [], [(368, 384), (0, 16)]], 384, res=True),
] + [mcase('third', [[(0, 279, 3)]], 279, N=1, H=3, DH=dh, res=True) for dh in (16, 32, 64)] + [
    mcase('sensors', [[], [(0, 224)], [(224, 288)]], 288, DH=64, res=True),             # the largest resident L of DH = 64
    mcase('spikes2x', [_spike_keys(279, 0), [], _spike_keys(279, 7)], 279, spiked=True, res=True, boost=2.0),
]
STREAM_CASES = [
    mcase('onlytail', [[(0, 128)], [], [(1, 128)]], 129),                               # frame 0: only the tail block's key is live
    mcase('notail', [[(128, 129)], [], [(128, 129), (0, 1)]], 129),                     # the tail block is empty
    mcase('middle', [[(128, 256)], [], [(128, 256), (0, 5)]], 279),                     # the whole middle block
    mcase('alternate', [[(0, 279, 2)], [(1, 279, 2)], []], 279),
    mcase('deadframe', [[(0, 50)], [(0, 279)], []], 279),                               # one frame fully masked next to two live ones
    mcase('spikes', [_spike_keys(1037, 0), [], _spike_keys(1037, 7)], 1037, spiked=True),
    # the same with the masked spike keys doubled: their scores (up to 209) lie more than 104 above the row's largest live score
    # in rows of every block, so exp(live score - masked maximum) is 0 in float32: maximum before mask = 0 / 0
    mcase('spikes2x', [_spike_keys(279, 0), [], _spike_keys(279, 7)], 279, spiked=True, boost=2.0),
]
DROPOUT_CASES = [mcase('sensors', [[], CAMERA, LIDAR], 324, p=0.1, res=True), mcase('sensors', [[], [(0, 415)], [(415, 517)]], 517, p=0.1)]
ALL_CASES = RESIDENT_CASES + STREAM_CASES + DROPOUT_CASES
DROPOUT_SEED = R.DROPOUT_SEEDS[0.1]

# e of blocked_masked(bk = R.float32_block(case)) in float32 against reference64_masked (this file run as a script; 8 CPU threads)
MEASURED = {
    'L1-N3H2D48-res-none': {'o': 0.00e+00, 'lse': 8.17e-08, 'dqkv': 2.89e-07},             # one key: p = 1, o = v exactly
    'L1-N3H2D48-res-key0': {'o': 0.00e+00, 'lse': 2.02e-08, 'dqkv': 3.08e-07},             # and o = 0 exactly in the dead frame
    'L17-N3H2D48-res-key16': {'o': 4.39e-07, 'lse': 9.27e-08, 'dqkv': 2.16e-07},
    'L17-N3H2D48-res-tile0': {'o': 2.24e-07, 'lse': 1.22e-07, 'dqkv': 2.88e-07},
    'L324-N3H2D48-res-sensors': {'o': 4.58e-07, 'lse': 7.24e-08, 'dqkv': 4.96e-07},
    'L384-N3H2D48-res-lasttile': {'o': 1.25e-06, 'lse': 7.54e-08, 'dqkv': 8.57e-07},
    'L279-N1H3D16-res-third': {'o': 3.65e-07, 'lse': 7.19e-08, 'dqkv': 6.10e-07},
    'L279-N1H3D32-res-third': {'o': 8.40e-07, 'lse': 7.42e-08, 'dqkv': 9.53e-07},
    'L279-N1H3D64-res-third': {'o': 5.14e-07, 'lse': 7.17e-08, 'dqkv': 9.15e-07},
    'L288-N3H2D64-res-sensors': {'o': 6.32e-07, 'lse': 8.04e-08, 'dqkv': 5.13e-07},
    'L279-N3H2D48-spiked-res-spikes2x': {'o': 1.67e-06, 'lse': 2.05e-07, 'dqkv': 1.95e-06},
    'L129-N3H2D48-onlytail': {'o': 1.44e-07, 'lse': 1.13e-07, 'dqkv': 1.49e-07},
    'L129-N3H2D48-notail': {'o': 5.73e-07, 'lse': 9.21e-08, 'dqkv': 3.97e-07},
    'L279-N3H2D48-middle': {'o': 7.29e-07, 'lse': 7.97e-08, 'dqkv': 6.74e-07},
    'L279-N3H2D48-alternate': {'o': 8.11e-07, 'lse': 8.34e-08, 'dqkv': 8.88e-07},
    'L279-N3H2D48-deadframe': {'o': 8.19e-07, 'lse': 8.34e-08, 'dqkv': 8.81e-07},
    'L1037-N3H2D48-spiked-spikes': {'o': 2.60e-06, 'lse': 3.02e-07, 'dqkv': 3.65e-06},
    'L279-N3H2D48-spiked-spikes2x': {'o': 1.62e-06, 'lse': 2.05e-07, 'dqkv': 1.92e-06},
    'L324-N3H2D48-p0.1-res-sensors': {'o': 5.06e-07, 'lse': 7.24e-08, 'dqkv': 6.44e-07},
    'L517-N3H2D48-p0.1-sensors': {'o': 6.84e-07, 'lse': 8.36e-08, 'dqkv': 8.55e-07},
}
BARS = {k: {n: 4 * e for n, e in v.items()} for k, v in MEASURED.items()}


# ================================================================================================ float64 reference
def reference64_masked(qkv, heads, dout, key_mask, keep=None):
    """R.reference64 under a key mask (N, L) bool: every L x L matrix written out in float64.  Masked scores are -inf before the
    softmax; a row without a live key has P = 0 by definition, hence o = 0, lse = -inf and no gradient through it."""
    E = qkv.shape[-1] // 3
    scale = (E // heads) ** -0.5
    q, k, v = (_heads(qkv[:, :, i * E:(i + 1) * E].double(), heads) for i in range(3))
    do = _heads(dout.double(), heads)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(key_mask[:, None, None, :], float('-inf'))
    lse = torch.logsumexp(s, -1)                                             # -inf where no key is live
    P = (s - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse)[..., None]).exp()   # exp(-inf - 0) = 0 there, never -inf + inf
    Pd = P if keep is None else P * keep.double()
    o = Pd @ v
    dv = Pd.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    if keep is not None:
        dP = dP * keep.double()
    D = (do * o).sum(-1, keepdim=True)
    dS = (dP - D) * P
    dq = (dS @ k) * scale
    dk = (dS.transpose(-1, -2) @ q) * scale
    return {'o': _packed(o), 'lse': lse.reshape(-1, lse.shape[-1]), 'dqkv': torch.cat([_packed(dq), _packed(dk), _packed(dv)], -1)}


# ================================================================================================ the recurrence, blocked
def blocked_masked(qkv, heads, bk, key_mask, dout=None, keep=None, dtype=torch.float32, fault=None):
    """R.blocked with the mask, as the kernels run it.  Per block: s = -inf on masked keys, m' = max(m, block max) - which stays
    -inf while no key has been live -, the exponentials subtract m* = (m' if finite else 0): a = exp(m - m*), p = exp(s - m*),
    l = l a + sum p, O = O a + (p keep) V.  At the end o = O / l and lse = m + log l where l > 0, else o = 0 and lse = -inf.
    Backward: p = exp(s - lse) on live pairs, 0 SELECTED on the others (exp(s - lse) is +inf for a dead row).
    fault: one planted error for the CPU test:
      'mask_after_max'  the maximum is taken over all keys < L, the mask only zeroes p afterwards
      'frame_shift'     frame n reads the mask row of frame n + 1
      'unguarded'       the exponentials subtract m' itself: exp(-inf - (-inf)) when a row's first block has no live key"""
    E = qkv.shape[-1] // 3
    dh = E // heads
    scale = torch.tensor(dh ** -0.5, dtype=dtype)
    q, k, v = (_heads(qkv[:, :, i * E:(i + 1) * E].to(dtype), heads) for i in range(3))
    N, H, L, _ = q.shape
    if fault == 'frame_shift':
        key_mask = key_mask.roll(-1, 0)
    dead = key_mask[:, None, None, :]                                        # (N, 1, 1, L)
    ninf = torch.tensor(float('-inf'), dtype=dtype)
    kp = None if keep is None else keep.to(dtype)
    m = torch.full((N, H, L), float('-inf'), dtype=dtype)
    l = torch.zeros(N, H, L, dtype=dtype)
    O = torch.zeros(N, H, L, dh, dtype=dtype)
    for k0 in range(0, L, bk):
        k1 = min(k0 + bk, L)
        raw = (q @ k[:, :, k0:k1].transpose(-1, -2)) * scale
        s = torch.where(dead[..., k0:k1], ninf, raw)
        mn = torch.maximum(m, (raw if fault == 'mask_after_max' else s).max(-1).values)
        ms = mn if fault == 'unguarded' else torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
        a = torch.exp(m - ms)
        p = torch.exp(s - ms[..., None])
        l = l * a + p.sum(-1)
        if kp is not None:
            p = p * kp[:, :, :, k0:k1]
        O = O * a[..., None] + p @ v[:, :, k0:k1]
        m = mn
    live_row = l > 0
    o = torch.where(live_row[..., None], O / l[..., None], torch.zeros_like(O))
    lse = torch.where(live_row, m + torch.log(l), ninf)
    out = {'o': _packed(o), 'lse': lse.reshape(N * H, L)}
    if dout is None:
        return out
    do = _heads(dout.to(dtype), heads)
    D = (do * o).sum(-1, keepdim=True)
    dq = torch.zeros_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    for k0 in range(0, L, bk):
        k1 = min(k0 + bk, L)
        kb, vb = k[:, :, k0:k1], v[:, :, k0:k1]
        p = torch.where(dead[..., k0:k1], torch.zeros((), dtype=dtype), torch.exp((q @ kb.transpose(-1, -2)) * scale - lse[..., None]))
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


# ================================================================================================ comparison
def compare(cid, got, ref):
    """R.compare under this file's bars"""
    return {n: (error_stats(got[n], ref[n], scale_of(ref[n])), BARS[cid][n]) for n in NAMES if n in got}


failures, statlines = R.failures, R.statlines


@functools.lru_cache(maxsize=None)
def _reference_cached(cid):
    c = next(c for c in ALL_CASES if case_id(c) == cid)
    inp = inputs(c)
    return inp, reference64_masked(inp['qkv'], c['H'], inp['dout'], inp['key_mask'], inp.get('cpu_keep'))


def reference(c):
    """(inputs with 'key_mask', float64 reference with the CPU keep-mask if p > 0) of a listed case, once per process; read-only"""
    return _reference_cached(case_id(c))


def float32_errors(c, fault=None):
    """{name: e} of blocked_masked in float32 on the case's inputs, with the block of the case's path"""
    inp, ref = reference(c)
    sub = blocked_masked(inp['qkv'], c['H'], R.float32_block(c), inp['key_mask'], inp['dout'], inp.get('cpu_keep'), fault=fault)
    return {n: error_stats(sub[n], ref[n], scale_of(ref[n]))['max_e'] for n in NAMES}


if __name__ == '__main__':
    for c in ALL_CASES:
        e = float32_errors(c)
        print(f"    '{case_id(c)}': {{" + ', '.join(f"'{n}': {v:.2e}" for n, v in e.items()) + '},', flush=True)
