"""Numpy restatement of muvo_voxel_calibration (include/muvo_hip.h): calibration, ensemble forecast and
uncertainty of K logit samples against a label grid.  `accumulate(..., dtype=np.float64)` is the reference; the same statements
with dtype=np.float32 are the float32 twin of the per-voxel formulae (every operation rounds to fp32, in the kernel's order) - it
is used only to measure what fp32 arithmetic itself costs on a case, which sets the tolerance of the real sums (`bars`)."""
import numpy as np

FIX = float(1 << 24)
NLL_FLOOR = 1e-12


def entropy(p):
    """-sum_c p ln p over axis 0 with 0 ln 0 = 0, classes added in ascending order"""
    h = np.zeros(p.shape[1:], p.dtype)
    for c in range(p.shape[0]):
        pc = p[c]
        safe = np.where(pc > 0, pc, 1).astype(p.dtype)
        h = h - np.where(pc > 0, pc * np.log(safe), 0).astype(p.dtype)
    return h


def per_voxel(logits, dtype=np.float64):
    """logits (K, C, N) float32 -> dict of per-voxel arrays in `dtype`: finite (N,) bool, pbar (C, N), yhat (N,), conf, H, Ebar, MI.
    Non-finite voxels hold zeros."""
    K, C, N = logits.shape
    x = logits.astype(dtype)
    with np.errstate(all='ignore'):
        m = x.max(axis=1)                                                    # NaN where any logit is NaN
        finite = ~(np.isnan(x).any(axis=1) | np.isposinf(m) | np.isneginf(m)).any(axis=0)
    x = x[:, :, finite]
    pbar = np.zeros((C, x.shape[2]), dtype)
    ebar = np.zeros(x.shape[2], dtype)
    for k in range(K):
        with np.errstate(all='ignore'):
            e = np.exp(x[k] - x[k].max(axis=0)).astype(dtype)              # exp(-inf) = 0
        s = np.zeros(e.shape[1], dtype)
        for c in range(C):
            s = s + e[c]
        p = (e * (dtype(1) / s)).astype(dtype)
        pbar = pbar + p
        ebar = ebar + entropy(p)
    pbar = (pbar / dtype(K)).astype(dtype)
    ebar = (ebar / dtype(K)).astype(dtype)
    H = entropy(pbar)
    out = {'finite': finite, 'pbar': np.zeros((C, N), dtype), 'yhat': np.zeros(N, np.int64)}
    out['pbar'][:, finite] = pbar
    out['yhat'][finite] = pbar.argmax(axis=0)                                # the first maximum
    for name, v in (('conf', pbar.max(axis=0)), ('H', H), ('Ebar', ebar), ('MI', np.maximum(dtype(0), H - ebar))):
        out[name] = np.zeros(N, dtype)
        out[name][finite] = v
    return out


def quantise(v, C):
    return np.rint(255.0 * np.minimum(1.0, v.astype(np.float64) / np.log(float(C)))).astype(np.int64)


def ssc_counts(pred, label, C):
    """the counting rule of muvo_ssc_counts over (prediction, label) pairs with label != 255 -> (3 + 3 C,) int64"""
    out = np.zeros(3 + 3 * C, np.int64)
    out[0] = ((label > 0) & (pred > 0)).sum()                               # completion: occupied is class != 0
    out[1] = ((label == 0) & (pred > 0)).sum()
    out[2] = ((label > 0) & (pred == 0)).sum()
    for j in range(C):
        out[3 + 3 * j] = ((pred == j) & (label == j)).sum()                  # tp
        out[3 + 3 * j + 1] = ((pred == j) & (label != j)).sum()              # fp: also under a label >= C
        out[3 + 3 * j + 2] = ((pred != j) & (label == j)).sum()              # fn: a label >= C is nobody's
    return out


def accumulate(logits_list, label, B, dtype=np.float64):
    """logits_list: K arrays (F, C, X, Y, Z) float32; label (F, X, Y, Z) uint8 -> dict: table (B, 3) float64 [n, n_correct, sum conf],
    counts (4,) int64 [voxels, ignored, skipped_nonfinite, correct], ssc (3 + 3 C,) int64, sums (6,) float64 [brier, nll, H correct,
    H wrong, MI correct, MI wrong], ens (F, X, Y, Z) uint8, top_entropy / top_mi (F, X, Y) uint8, and under `voxel` the per-voxel arrays
    (flat, in label order): scored, correct, bin, conf, brier, nll, H, MI, pbar."""
    F, C, X, Y, Z = logits_list[0].shape
    N = F * X * Y * Z
    lg = np.stack([np.moveaxis(t, 1, 0).reshape(C, N) for t in logits_list])         # (K, C, N)
    lab = label.reshape(N).astype(np.int64)
    v = per_voxel(lg, dtype)
    ignored = lab == 255
    scored = ~ignored & v['finite']
    pbar, yhat, conf = v['pbar'], v['yhat'], v['conf']
    onehot = (np.arange(C)[:, None] == lab[None, :]).astype(dtype)                   # all zero where the label is >= C
    brier = np.zeros(N, dtype)
    for c in range(C):
        d = pbar[c] - onehot[c]
        brier = brier + d * d
    py = np.where(lab < C, np.take_along_axis(pbar, np.minimum(lab, C - 1)[None, :], 0)[0], 0).astype(dtype)
    nll = (-np.log(np.maximum(py, dtype(NLL_FLOOR)))).astype(dtype)
    correct = scored & (yhat == lab)
    bins = np.minimum(B - 1, np.floor(conf * dtype(B)).astype(np.int64))
    table = np.zeros((B, 3), np.float64)
    for b in range(B):
        inside = scored & (bins == b)
        table[b] = inside.sum(), (inside & correct).sum(), conf[inside].astype(np.float64).sum()
    counts = np.array([scored.sum(), ignored.sum(), (~ignored & ~v['finite']).sum(), correct.sum()], np.int64)
    wrong = scored & ~correct
    f64 = lambda a, mask: float(a[mask].astype(np.float64).sum())                    # noqa: E731
    sums = np.array([f64(brier, scored), f64(nll, scored), f64(v['H'], correct), f64(v['H'], wrong), f64(v['MI'], correct), f64(v['MI'], wrong)])
    ens = np.where(scored, yhat, 255).astype(np.uint8).reshape(F, X, Y, Z)
    qh = np.where(v['finite'], quantise(v['H'], C), 0).reshape(F, X, Y, Z).max(axis=3).astype(np.uint8)
    qm = np.where(v['finite'], quantise(v['MI'], C), 0).reshape(F, X, Y, Z).max(axis=3).astype(np.uint8)
    voxel = dict(scored=scored, correct=correct, bin=bins, conf=conf, brier=brier, nll=nll, H=v['H'], MI=v['MI'], pbar=pbar)
    return dict(table=table, counts=counts, ssc=ssc_counts(yhat[scored], lab[scored], C), sums=sums, ens=ens, top_entropy=qh, top_mi=qm, voxel=voxel)


def margins(ref, B):
    """per scored voxel of a float64 `accumulate`: (gap between the two largest pbar, distance of conf * B to the nearest integer)"""
    v = ref['voxel']
    top = np.sort(v['pbar'], axis=0)
    scaled = v['conf'] * B
    return (top[-1] - top[-2])[v['scored']], np.abs(scaled - np.rint(scaled))[v['scored']]


def bars(ref, twin):
    """What fp32 arithmetic costs on this case, times 4, for every real sum the kernel keeps: (bar of sums (6,), bar of the table's
    conf sums (B,)).  A sum's distance between twin and reference is taken voxel by voxel, sum_i |twin_i - ref_i| - a bound on any
    signed sum of such errors, whatever the order, whereas the difference of the two totals is a random walk that can come out near
    zero by luck and then bounds nothing.  The factor 4 covers a device exp / log that differs from numpy's by a few ulp and another
    summation order.  On top, the number format: the kernel rounds every voxel's value to a multiple of 2^-24, at most 2^-25 a voxel.
    Which voxels are correct and which bin holds them is taken from the reference - the kernel takes the decisions fp32 rounding
    could turn in fp64 - so the twin only supplies values; its conf is the mean probability of the reference's class."""
    a, b = ref['voxel'], dict(twin['voxel'])
    assert np.array_equal(a['scored'], b['scored'])
    yhat = ref['ens'].reshape(-1).astype(np.int64) % b['pbar'].shape[0]             # 255 (unscored) -> some class, masked out below
    b['conf'] = np.take_along_axis(b['pbar'], yhat[None, :], 0)[0]
    scored, correct = a['scored'], a['correct']
    wrong = scored & ~correct
    dist = lambda name, mask: float(np.abs(b[name][mask].astype(np.float64) - a[name][mask]).sum()) * 4 + int(mask.sum()) * 2.0 ** -25     # noqa: E731
    sums = np.array([dist('brier', scored), dist('nll', scored), dist('H', correct), dist('H', wrong), dist('MI', correct), dist('MI', wrong)])
    B = ref['table'].shape[0]
    conf = np.array([dist('conf', scored & (a['bin'] == k)) for k in range(B)])
    return sums, conf


def to_fixed(acc):
    """the accumulators of a float64 `accumulate` as the nested integer lists the kernel would leave (real sums rounded to 2^-24)"""
    table = [[int(r[0]), int(r[1]), int(round(r[2] * FIX))] for r in acc['table']]
    return dict(table=table, counts=[int(v) for v in acc['counts']], ssc=[int(v) for v in acc['ssc']], sums=[int(round(v * FIX)) for v in acc['sums']])


def make_case(seed, F, C, X, Y, Z, K, B, margin=1e-4, ignore_share=0.15, rounds=60):
    """Random fp32 logits (K of (F, C, X, Y, Z)) and labels whose scored voxels keep, in the float64 restatement, a gap of `margin`
    between the two largest pbar and between conf * B and the nearest integer, so that an fp32 implementation must agree with float64
    on every integer output.  Offending voxels are drawn again; the last frame is all 255.  Returns (logits_list, label, dropped):
    dropped = voxels still offending after `rounds` (the tests assert 0)."""
    rng = np.random.default_rng(seed)
    N = F * X * Y * Z
    lg = (rng.standard_normal((K, C, N)) * 3.0).astype(np.float32)
    lab = rng.integers(0, C, N).astype(np.uint8)
    lab[rng.random(N) < ignore_share] = 255
    lab = lab.reshape(F, X * Y * Z)
    lab[F - 1] = 255
    lab = lab.reshape(N)
    bad = np.arange(N)
    for r in range(rounds + 1):
        v = per_voxel(lg[:, :, bad])
        top = np.sort(v['pbar'], axis=0)
        scaled = v['conf'] * B
        off = (lab[bad] != 255) & ((top[-1] - top[-2] < margin) | (np.abs(scaled - np.rint(scaled)) < margin))
        bad = bad[off]
        if not bad.size or r == rounds:
            break
        lg[:, :, bad] = (rng.standard_normal((K, C, bad.size)) * 3.0).astype(np.float32)
    logits_list = [np.ascontiguousarray(np.moveaxis(lg[k].reshape(C, F, X, Y, Z), 0, 1)) for k in range(K)]
    return logits_list, lab.reshape(F, X, Y, Z), int(bad.size)


def hand_cases():
    """Hand-made cases whose answers are known in closed form: {name: (logits_list, label, B)}; every grid is (F, C, 2, 3, 5)."""
    X, Y, Z = 2, 3, 5
    inf, nan = np.float32(np.inf), np.float32(np.nan)

    def const(F, values):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(values, np.float32)[None, :, None, None, None], (F, len(values), X, Y, Z)))

    def labels(F, C):
        return (np.arange(F * X * Y * Z) % C).astype(np.uint8).reshape(F, X, Y, Z)
    cases = {}
    for C in (2, 4):                                                        # all logits equal: yhat 0, conf 1/C, H = ln C, MI = 0
        cases[f'equal_c{C}'] = ([const(2, [1.5] * C)], labels(2, C), 15)
    # two samples, one-hot on different classes (logits of +-80): pbar = (1/2, 1/2), H = ln 2, Ebar = 0, MI = ln 2
    cases['onehot_pair'] = ([const(2, [80, -80]), const(2, [-80, 80])], labels(2, 2), 15)
    cases['conf_one'] = ([const(1, [-80, 80, -80])], labels(1, 3), 32)     # conf = 1.0 lands in bin B - 1
    lab = labels(2, 3)
    lab[1] = 255                                                            # a whole frame ignored
    lab[0, 0, 0, :2] = 255
    cases['neg_inf'] = ([const(2, [0, -inf, 0])], lab, 15)                  # p = (1/2, 0, 1/2): H = ln 2
    lg = const(3, [0.25, -0.5, 1.0]).copy()
    lg2 = const(3, [0.0, 2.0, -1.0]).copy()
    lg[1, 0] = inf                                                          # frame 1: the maximum is +inf in sample 0
    lg2[1, 1, 0] = nan                                                      # ... and NaNs in sample 1 on top
    lg[2, :, 0, 0] = -inf                                                   # frame 2: some columns all -inf, one NaN column, the rest finite
    lg[2, 2, 1, 1] = nan
    lab = labels(3, 3)
    lab[1, 0, 0, 0] = lab[2, 0, 0, 1] = 255                                 # ignored wins over non-finite
    cases['nonfinite'] = ([lg, lg2], lab, 15)
    return cases
