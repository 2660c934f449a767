"""The distance transform, the boundary loss and the voxel Chamfer counts of include/muvo_hip.h (muvo_voxel_edt,
muvo_voxel_boundary_forward / _backward, muvo_voxel_cd_counts) restated in numpy.  Helpers only: no fixtures, no tests.
    occupied     1 <= v <= 254; 0 is free, 255 "unknown" and never occupied
    edt2         edt2(grid, cap)[f, v] = min(cap, min over the occupied u of frame f of |v - u|^2), distances in cells, by three
                 separable min-plus passes d(i) = min_j (i - j)^2 + d(j) in int64, capped after each; `cap` where a frame is empty
    class grid   of a prediction: the first maximum over C (a tie with class 0 is free)
    loss         per frame, in a dtype (float64 is the reference, float32 measures the error every bar is 4 x of):
                 e_c = exp(z_c - max z), s = e_0 + e_1 + ... in ascending c, q = e_0 / s, p = 1 - q, s_c = e_c / s
                 dG = sqrt(edt2(label, T^2)) / T, dP = sqrt(edt2(P, T^2)) / T, n_G = the occupied label cells
                 L_f = (sum_{!g, !k} p dG + sum_{g} q dP) / n_G;  loss = weight x mean of L_f over the frames with n_G > 0, else 0
    gradient     dP and P are constants: dL/dz_c = w dp/dz_c, dp/dz_0 = -q p, dp/dz_c = q s_c,
                 w = weight / (frames n_G) x (dG where !g and !k, -dP where g, 0 where k)
    counts       per frame pair with both sets non-empty, from the untruncated transforms: n_P, n_G, hits_P[i] = #{v in P :
                 edt2_G(v) <= k_i}, hits_G[i] likewise, sum_PG = sum_{v in P} sqrt(edt2_G(v)), sum_GP likewise; frames, skipped"""
import math

import numpy as np

WEIGHT = 0.75
BIG = 1 << 40


def occupied(grid):
    g = np.asarray(grid)
    return (g >= 1) & (g <= 254)


def full_cap(shape):
    X, Y, Z = shape[-3:]
    return X * X + Y * Y + Z * Z


def edt2(grid, cap):
    """grid (..., X, Y, Z) uint8 -> int64 of the same shape"""
    g = np.asarray(grid)
    cap = int(cap)
    assert cap >= 1
    d = np.minimum(np.where(occupied(g), 0, BIG).astype(np.int64), cap)
    for axis in (-1, -2, -3):
        n = g.shape[axis]
        src = np.moveaxis(d, axis, 0)
        out = np.full_like(src, cap)
        i = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        for j in range(n):
            out = np.minimum(out, (i - j) ** 2 + src[j][None])
        d = np.ascontiguousarray(np.moveaxis(np.minimum(out, cap), 0, axis))
    return d


def edt2_brute(grid, cap):
    """(X, Y, Z) uint8 -> int64 by the definition itself, O(V^2)"""
    g = np.asarray(grid)
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in g.shape], indexing='ij'), -1).reshape(-1, 3).astype(np.int64)
    occ = cells[occupied(g).reshape(-1)]
    if not len(occ):
        return np.full(g.shape, int(cap), np.int64)
    d = ((cells[:, None, :] - occ[None, :, :]) ** 2).sum(-1).min(1)
    return np.minimum(d, int(cap)).reshape(g.shape)


def class_grid(logits):
    """(F, C, X, Y, Z) float32 -> (F, X, Y, Z) uint8: the first maximum over C"""
    return np.asarray(logits).argmax(1).astype(np.uint8)


def loss_and_grad(logits, labels, T, weight, dtype=np.float64, pred=None):
    """logits (F, C, X, Y, Z) float32, labels (F, X, Y, Z) uint8 -> dict: loss, dlogits (F, C, X, Y, Z), frame_loss (F,) = L_f,
    n_g (F,), edt_label, edt_pred (F, X, Y, Z) int64, pred (F, X, Y, Z) uint8, p (F, X, Y, Z).  pred: the class grid to hold
    constant (finite differences); None: that of the logits."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    F, C = logits.shape[:2]
    T = int(T)
    pred = class_grid(logits) if pred is None else np.asarray(pred)
    edt_label, edt_pred = edt2(labels, T * T), edt2(pred, T * T)
    z = logits.astype(dtype)
    e = np.exp(z - z.max(1, keepdims=True)).astype(dtype)
    s = e[:, 0].copy()
    for c in range(1, C):
        s = s + e[:, c]
    q = (e[:, 0] / s).astype(dtype)
    p = (dtype(1) - q).astype(dtype)
    g, k = occupied(labels), labels == 255
    dG = (np.sqrt(edt_label.astype(dtype)) / dtype(T)).astype(dtype)
    dP = (np.sqrt(edt_pred.astype(dtype)) / dtype(T)).astype(dtype)
    terms = np.where(g, q * dP, np.where(k, dtype(0), p * dG)).astype(dtype)
    w = np.where(g, -dP, np.where(k, dtype(0), dG)).astype(dtype)
    n_g = g.reshape(F, -1).sum(1).astype(np.int64)
    frames = int((n_g > 0).sum())
    frame_loss = np.zeros(F, dtype)
    dl = np.zeros(logits.shape, dtype)
    total = dtype(0)
    for f in range(F):
        if n_g[f] == 0:
            continue
        frame_loss[f] = terms[f].sum(dtype=dtype) / dtype(n_g[f])
        total = total + frame_loss[f]
        a = (w[f] * (dtype(weight) / dtype(frames * n_g[f]))).astype(dtype)
        dl[f, 0] = a * (-(q[f] * p[f]))
        for c in range(1, C):
            dl[f, c] = a * (q[f] * (e[f, c] / s[f]))
    loss = dtype(weight) * total / dtype(frames) if frames else dtype(0)
    return {'loss': dtype(loss), 'dlogits': dl, 'frame_loss': frame_loss, 'n_g': n_g, 'edt_label': edt_label, 'edt_pred': edt_pred,
            'pred': pred, 'p': p}


def saturated(logits):
    """logits x 40 with 30 more on each cell's first maximum: the winner leads by at least 30, so q is below e^-30 or within
    (C - 1) e^-30 of 1 and p = 1 - q is exactly 1 or 0 in float32"""
    z = (np.asarray(logits, np.float32) * np.float32(40)).astype(np.float32)
    w = z.argmax(1)[:, None]
    np.put_along_axis(z, w, np.take_along_axis(z, w, 1) + np.float32(30), 1)
    return z


def hard_loss(edt_label, edt_pred, labels, pred, T, weight):
    """the hard-set expression mean_f (sum_{P \\ G} dG + sum_{G \\ P} dP) / n_G over the frames with n_G > 0, float64, from the
    transforms alone (255 cells of the label take no part)"""
    g, k, P = occupied(labels), np.asarray(labels) == 255, occupied(pred)
    dG, dP = np.sqrt(np.asarray(edt_label, np.float64)) / T, np.sqrt(np.asarray(edt_pred, np.float64)) / T
    total, frames = 0.0, 0
    for f in range(len(g)):
        n = int(g[f].sum())
        if n:
            total += (dG[f][P[f] & ~g[f] & ~k[f]].sum() + dP[f][g[f] & ~P[f]].sum()) / n
            frames += 1
    return weight * total / frames if frames else 0.0


def thresholds2(resolution, thresholds=(1.0, 2.0, 4.0)):
    return [int(math.floor((t / resolution) ** 2 + 1e-9)) for t in thresholds]


def cd_counts(label, pred, thr2):
    """label, pred (F, X, Y, Z) uint8 -> (counts (10,) int64: frames, skipped, n_P, n_G, hits_P[3], hits_G[3]; sums (2,) float64:
    sum_PG, sum_GP; the addends of both sums, for the order-free bound of the tests)"""
    label, pred = np.asarray(label), np.asarray(pred)
    cap = full_cap(label.shape)
    counts, sums, addends = np.zeros(10, np.int64), np.zeros(2), 0
    for f in range(len(label)):
        G, P = occupied(label[f]), occupied(pred[f])
        if not G.any() or not P.any():
            counts[1] += 1
            continue
        eg, ep = edt2(label[f], cap), edt2(pred[f], cap)
        counts[0] += 1
        counts[2] += P.sum()
        counts[3] += G.sum()
        for i, k in enumerate(thr2):
            counts[4 + i] += (eg[P] <= k).sum()
            counts[7 + i] += (ep[G] <= k).sum()
        sums[0] += np.sqrt(eg[P].astype(np.float64)).sum()
        sums[1] += np.sqrt(ep[G].astype(np.float64)).sum()
        addends += int(P.sum() + G.sum())
    return counts, sums, addends


# ---- scenes of the transform tests: (X, Y, Z) uint8 -----------------------------------------------------------------------------
def scene(kind, shape, seed=0):
    g = np.zeros(shape, np.uint8)
    rng = np.random.default_rng(seed)
    if kind == 'empty':
        pass
    elif kind == 'full':
        g[:] = 1
    elif kind == 'first':
        g[0, 0, 0] = 3
    elif kind == 'last':
        g[-1, -1, -1] = 254
    elif kind == 'plane':
        g[:, shape[1] // 2, :] = 2
    elif kind == 'random':
        g[rng.random(shape) < 0.02] = 1
        if not g.any():
            g[tuple(int(rng.integers(n)) for n in shape)] = 1
    elif kind == 'unknown':                       # 255s among a few occupied cells: they must not count as occupied
        g[rng.random(shape) < 0.3] = 255
        g[rng.random(shape) < 0.03] = 7
    elif kind == 'only_unknown':
        g[:] = 255
    else:
        raise ValueError(kind)
    return g
