"""The rendered first-hit class loss of include/muvo_hip.h (muvo_render_class_fwd / muvo_render_class_bwd) restated in numpy.
Helpers only: no fixtures, no tests.  The cell sequence, the validity rule and the per-cell probabilities are those of
tests/render_reference.py, by import (cell_table, occupancy: e_c = exp(z_c - max z), s = e_0 + (e_1 + ... + e_{C-1}), p_c = e_c / s).
Here, per ray and in a dtype (float64 is the reference, float32 measures the error every bar is 4 x of):
    T_0 = 1, T_{k+1} = T_k q_k with q = p_0
    y   = the label's class at the first cell of the sequence whose class is not 0, 0 without one; -1 (the ray is ignored, like
          an invalid ray) where that class is >= C
    S_y = sum_k T_k p_{k,y} for y >= 1, S_0 = T_n, products and sum in the order of k;  sum_c S_c = 1 (asserted in float64)
    l   = -log((S_y + EPS) / (1 + EPS)), EPS = 2^-10;  loss = weight / F sum_f 1 / N sum_{valid rays} l, N = the valid rays
    A_j = T_j p_{j,y}, B_j = S_y - sum_{k<=j} A_k (y >= 1);  A_j = 0, B_j = T_n (y = 0)
    dS_y/dz_{j,c} = A_j [c = y] + B_j [c = 0] - p_{j,c} (A_j + B_j),  dl/dS_y = -1 / (S_y + EPS)
    accumulator: slot y += -A_j / (S_y + EPS), slot 0 += -B_j / (S_y + EPS);  dz_{j,c} = (acc_c - p_c sum_c' acc_c') weight / (F N)"""
import numpy as np

import render_reference as R

f32 = np.float32
FIX_BITS = 37                                  # fraction bits of the device's gradient accumulator
EPS = 2.0 ** -10
WEIGHT = R.WEIGHT


def target_class(label, table, C):
    """y (R,) int64 of one label grid (X, Y, Z): the class of the first cell of the sequence whose class is not 0, 0 without one,
    -1 at invalid rays and where that class is >= C"""
    flat = np.asarray(label).reshape(-1).astype(np.int64)
    cls = np.where(table['cells'] >= 0, flat[np.maximum(table['cells'], 0)], 0)
    first = (cls != 0).argmax(1)
    y = cls[np.arange(len(first)), first]                              # 0 where no cell is occupied
    return np.where(table['valid'] & (y < C), y, -1)


def transmittance(q, table, dtype=np.float64):
    """q flat (V,) -> (T (R, nmax) = T_k with pads continuing unchanged, T_n (R,)) in dtype, the products in the order of k"""
    idx, pad = np.maximum(table['cells'], 0), table['cells'] < 0
    qk = np.where(pad, 1, np.asarray(q, dtype)[idx]).astype(dtype)
    T = np.ones_like(qk)
    for k in range(1, qk.shape[1]):
        T[:, k] = T[:, k - 1] * qk[:, k - 1]
    return T, (T[:, -1] * qk[:, -1]).astype(dtype)


def masses(p, table, dtype=np.float64):
    """p (C, V) -> S (C, R): S_c = sum_k T_k p_{k,c} for c >= 1 and S_0 = T_n, for every class (0 at invalid rays)"""
    p = np.asarray(p, dtype)
    idx, pad = np.maximum(table['cells'], 0), table['cells'] < 0
    T, Tn = transmittance(p[0], table, dtype)
    S = np.zeros((len(p), len(idx)), dtype)
    S[0] = Tn
    for c in range(1, len(p)):
        A = T * np.where(pad, 0, p[c][idx]).astype(dtype)
        for k in range(A.shape[1]):
            S[c] = S[c] + A[:, k]
    return np.where(table['valid'], S, 0).astype(dtype)


def loss_and_grad(logits, labels, rays, weight, dtype=np.float64, table=None):
    """logits (F, C, X, Y, Z), labels (F, X, Y, Z) uint8 -> dict: loss, dlogits (F, C, X, Y, Z) through the accumulator form, S (F, R)
    = S_y (0 at invalid and ignored rays), y (F, R), Tn (F, R), cost (F, R) = l per ray, visits (F, V) = the rays through each cell
    that add to its gradient (valid, not ignored, T_k != 0), and the table."""
    logits = np.asarray(logits)
    F, C = logits.shape[:2]
    shape = logits.shape[2:]
    V = int(np.prod(shape))
    table = R.cell_table(shape, rays) if table is None else table
    valid, N = table['valid'], int(table['valid'].sum())
    idx, pad = np.maximum(table['cells'], 0), table['cells'] < 0
    out = {'S': [], 'y': [], 'Tn': [], 'cost': [], 'visits': np.zeros((F, V), np.int64), 'table': table, 'n_valid': N}
    dl = np.zeros((F, C, V), dtype)
    total = dtype(0)
    eps = dtype(EPS)
    for f in range(F):
        _, _, p = R.occupancy(logits[f].reshape(C, V), dtype)
        if dtype == np.float64:
            err = np.abs(masses(p, table).sum(0) - 1)[valid]
            assert not len(err) or err.max() <= 1e-12, 'the masses of a ray do not add up to 1'
        T, Tn = transmittance(p[0], table, dtype)
        y = target_class(labels[f], table, C)
        live = valid & (y >= 0)
        py = np.where(pad | (y < 1)[:, None], 0, p[np.maximum(y, 0)[:, None], idx]).astype(dtype)
        A = T * py
        S = np.zeros(len(idx), dtype)
        for k in range(A.shape[1]):
            S = S + A[:, k]
        S = np.where(live, np.where(y == 0, Tn, S), 0).astype(dtype)
        cost = np.where(live, -np.log((S + eps) / (dtype(1) + eps)), 0).astype(dtype)
        out['S'].append(S), out['y'].append(y), out['Tn'].append(np.where(valid, Tn, 0).astype(dtype)), out['cost'].append(cost)
        if N:
            total = total + cost.sum(dtype=dtype) / dtype(N)
            B = np.where((y == 0)[:, None], Tn[:, None], S[:, None] - np.cumsum(A, 1, dtype=dtype))
            r = dtype(1) / (S + eps)
            at = ~pad & live[:, None]
            acc = np.zeros((C, V), dtype)
            np.add.at(acc[0], table['cells'][at], (-B * r[:, None])[at])
            np.add.at(acc, (np.broadcast_to(np.maximum(y, 0)[:, None], at.shape)[at], table['cells'][at]), (-A * r[:, None])[at])
            np.add.at(out['visits'][f], table['cells'][at & (T != 0)], 1)
            dl[f] = (acc - p * acc.sum(0)) * (dtype(weight) / dtype(F * N))
    out['loss'] = dtype(weight) * total / dtype(F)
    out['dlogits'] = dl.reshape(logits.shape)
    for k in ('S', 'y', 'Tn', 'cost'):
        out[k] = np.stack(out[k])
    return out


def direct_gradient(logits, labels, rays, weight, table=None):
    """dlogits (F, C, X, Y, Z) float64 from the formula for dS_y/dz_{j,c} itself, ray by ray and cell by cell - slow; what the
    accumulator form of loss_and_grad is held against on small inputs"""
    logits = np.asarray(logits)
    F, C = logits.shape[:2]
    V = int(np.prod(logits.shape[2:]))
    table = R.cell_table(logits.shape[2:], rays) if table is None else table
    N = int(table['valid'].sum())
    dl = np.zeros((F, C, V))
    for f in range(F):
        _, _, p = R.occupancy(logits[f].reshape(C, V))
        T, Tn = transmittance(p[0], table)
        y = target_class(labels[f], table, C)
        for r in np.flatnonzero(table['valid'] & (y >= 0)):
            cells = table['cells'][r, :table['n'][r]]
            A = T[r, :len(cells)] * p[y[r], cells] if y[r] >= 1 else np.zeros(len(cells))
            S = A.sum() if y[r] >= 1 else Tn[r]
            B = S - np.cumsum(A) if y[r] >= 1 else np.full(len(cells), Tn[r])
            g = -p[:, cells] * (A + B)
            g[y[r]] += A
            g[0] += B
            dl[f][:, cells] += -g / (S + EPS) * weight / (F * N)                   # the cells of one ray are distinct
    return dl.reshape(logits.shape)
