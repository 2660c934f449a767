"""The rendered first-hit depth loss of include/muvo_hip.h (muvo_render_fwd / muvo_render_bwd) restated in numpy.  Helpers only:
no fixtures, no tests.  The cell sequence of a ray is the float32 march of raycast_reference.march - the same statements in the
same order, here for all rays of a table at once and without the occupancy test (tests/test_render_reference.py holds the two
against each other cell by cell) - so the sequence is the device's by construction.  The compositing takes a dtype: float64 is
the reference, float32 measures the error every bar is 4 x of."""
import numpy as np

f32 = np.float32
FIX_BITS = 26                                  # fraction bits of the device's gradient accumulator


# ---- the cell sequence ------------------------------------------------------------------------------------------------------------
def cell_table(shape, rays):
    """rays (R, 7) through an empty grid `shape` = (X, Y, Z) -> dict: valid (R,) bool, n (R,) cells per ray (-1: invalid), cells
    (R, nmax) linear indices (-1 behind the end), t (R, nmax) float32 entry depths, t_exit (R,) float32 (0 at invalid rays)"""
    rays = np.asarray(rays, f32)
    R = len(rays)
    N = tuple(int(v) for v in shape)
    with np.errstate(all='ignore'):
        o, d = [rays[:, a].copy() for a in range(3)], [rays[:, 3 + a].copy() for a in range(3)]
        t0, t1 = np.zeros(R, f32), rays[:, 6].copy()
        ok, moving, inv = np.ones(R, bool), np.zeros(R, bool), [np.zeros(R, f32) for _ in range(3)]
        for a in range(3):
            move = d[a] != 0
            inv[a] = np.where(move, f32(1) / np.where(move, d[a], f32(1)), f32(0)).astype(f32)
            ta, tb = (f32(0) - o[a]) * inv[a], (f32(N[a]) - o[a]) * inv[a]
            asc = ta <= tb
            lo, hi = np.where(asc, ta, tb), np.where(asc, tb, ta)
            ok &= np.where(move, lo <= hi, (f32(0) <= o[a]) & (o[a] < f32(N[a])))
            t0 = np.where(move & (lo > t0), lo, t0)
            t1 = np.where(move & (hi < t1), hi, t1)
            moving |= move
        valid = ok & moving & (t0 < t1)
        c = []
        for a in range(3):
            fl = np.floor(o[a] + d[a] * t0)
            c.append(np.where(~(fl >= 0), 0, np.where(fl > f32(N[a] - 1), N[a] - 1, np.nan_to_num(fl, nan=0.0, posinf=0.0, neginf=0.0))).astype(np.int64))
        t = t0.copy()
        alive = valid.copy()
        cells, ts = [], []
        for _ in range(N[0] + N[1] + N[2] + 3):
            if not alive.any():
                break
            cells.append(np.where(alive, (c[0] * N[1] + c[1]) * N[2] + c[2], -1))
            ts.append(np.where(alive, t, f32(0)).astype(f32))
            best, axis = np.full(R, np.inf, f32), np.full(R, -1)
            for a in range(3):
                tn = ((c[a] + (d[a] > 0)).astype(f32) - o[a]) * inv[a]
                take = (d[a] != 0) & (tn < best)
                best, axis = np.where(take, tn, best).astype(f32), np.where(take, a, axis)
            alive &= ~((axis < 0) | (best > t1))
            for a in range(3):
                c[a] = c[a] + np.where(alive & (axis == a), np.where(d[a] > 0, 1, -1), 0)
                alive &= ~((c[a] < 0) | (c[a] >= N[a]))
            t = np.where(alive, best, t).astype(f32)
    cells = np.stack(cells, 1) if cells else np.full((R, 1), -1)
    ts = np.stack(ts, 1) if ts else np.zeros((R, 1), f32)
    n = np.where(valid, (cells >= 0).sum(1), -1)
    return {'valid': valid, 'n': n, 'cells': cells, 't': ts, 't_exit': np.where(valid, t1, f32(0)).astype(f32)}


def target_depth(label, table):
    """t* (R,) float32 of one label grid (X, Y, Z): the entry depth of the first cell of the sequence whose class is not 0, t_exit
    without one (0 at invalid rays)"""
    flat = np.asarray(label).reshape(-1)
    occ = (table['cells'] >= 0) & (flat[np.maximum(table['cells'], 0)] != 0)
    first = occ.argmax(1)
    return np.where(occ.any(1), table['t'][np.arange(len(first)), first], table['t_exit']).astype(f32)


# ---- per cell ----------------------------------------------------------------------------------------------------------------------
def occupancy(logits, dtype=np.float64):
    """logits (C, ...) -> (q, a, p (C, ...)) in dtype: e_c = exp(z_c - max z), occ = e_1 + ... + e_{C-1}, s = e_0 + occ"""
    z = np.asarray(logits, dtype)
    e = np.exp(z - z.max(0))
    occ = np.zeros_like(e[0])
    for c in range(1, len(e)):
        occ = occ + e[c]
    s = e[0] + occ
    return e[0] / s, occ / s, e / s


# ---- compositing -------------------------------------------------------------------------------------------------------------------
def render(q, a, table, dtype=np.float64):
    """q, a flat (V,) -> dict of per-ray arrays in dtype: D (0 at invalid rays), T_n, and the padded (R, nmax) T (= T_k), w"""
    idx, pad = np.maximum(table['cells'], 0), table['cells'] < 0
    qk = np.where(pad, 1, np.asarray(q, dtype)[idx]).astype(dtype)
    ak = np.where(pad, 0, np.asarray(a, dtype)[idx]).astype(dtype)
    T = np.ones_like(qk)
    for k in range(1, qk.shape[1]):            # the products in the order of k (np.cumprod is free to reassociate)
        T[:, k] = T[:, k - 1] * qk[:, k - 1]
    Tn = T[:, -1] * qk[:, -1]
    w = T * ak
    D = np.zeros(len(qk), dtype)
    tk = table['t'].astype(dtype)
    for k in range(qk.shape[1]):
        D = D + w[:, k] * tk[:, k]
    D = np.where(table['valid'], D + Tn * table['t_exit'].astype(dtype), 0).astype(dtype)
    return {'D': D, 'Tn': np.where(table['valid'], Tn, 0).astype(dtype), 'T': T, 'w': w, 'q': qk}


def loss_and_grad(logits, labels, rays, weight, dtype=np.float64, table=None):
    """logits (F, C, X, Y, Z), labels (F, X, Y, Z) uint8 -> dict: loss, dlogits (F, C, X, Y, Z) by the closed form, D (F, R), tstar
    (F, R) float32, Tn (F, R), visits (F, V) = the rays through each cell that add to its gradient (valid, sign != 0, T_k != 0),
    and the table."""
    logits = np.asarray(logits)
    F, C = logits.shape[:2]
    shape = logits.shape[2:]
    V = int(np.prod(shape))
    table = cell_table(shape, rays) if table is None else table
    valid, N = table['valid'], int(table['valid'].sum())
    out = {'D': [], 'tstar': [], 'Tn': [], 'visits': np.zeros((F, V), np.int64), 'table': table, 'n_valid': N}
    dl = np.zeros((F, C, V), dtype)
    total = dtype(0)
    tk, pad = table['t'].astype(dtype), table['cells'] < 0
    for f in range(F):
        q, a, p = occupancy(logits[f].reshape(C, V), dtype)
        r = render(q, a, table, dtype)
        ts = target_depth(labels[f], table)
        diff = np.where(valid, r['D'] - ts.astype(dtype), 0)
        out['D'].append(r['D']), out['tstar'].append(ts), out['Tn'].append(r['Tn'])
        if N:
            total = total + np.abs(diff).sum(dtype=dtype) / dtype(N)
            wt = r['w'] * tk
            Pk = np.cumsum(wt, 1) - wt                                   # P_k = sum_{j<k} w_j t_j
            Qk = r['D'][:, None] - Pk - wt
            g = np.sign(diff)[:, None] * (r['T'] * r['q'] * tk - Qk)      # sign (T_{k+1} t_k - Q_k)
            live = ~pad & valid[:, None] & (diff != 0)[:, None]
            acc = np.zeros(V, dtype)
            np.add.at(acc, table['cells'][live], g[live])
            np.add.at(out['visits'][f], table['cells'][live & (r['T'] != 0)], 1)
            delta = np.zeros((C, 1), dtype)
            delta[0] = 1
            dl[f] = acc[None] * dtype(weight) / dtype(F * N) * (p - delta)
            dl[f, 0] = acc * dtype(weight) / dtype(F * N) * -a            # p_0 - 1 = -a without the cancellation
    out['loss'] = dtype(weight) * total / dtype(F)
    out['dlogits'] = dl.reshape(logits.shape)
    for k in ('D', 'tstar', 'Tn'):
        out[k] = np.stack(out[k])
    return out


# ---- inputs of the tests ------------------------------------------------------------------------------------------------------------
WEIGHT = 0.5


def frames(label_scenes, C, seed=0, margin=3.0):
    """logits (F, C, X, Y, Z) float32 for F label grids: random, pushed towards the label's class by `margin` on most cells - a
    prediction that is roughly right, with surfaces that are not sharp"""
    rng = np.random.default_rng(seed)
    out = []
    for g in label_scenes:
        x = rng.standard_normal((C, *g.shape)).astype(f32)
        cls = np.minimum(g.astype(np.int64), C - 1)
        keep = rng.random(g.shape) < 0.85
        idx = np.indices(g.shape)
        x[(cls, *idx)] += np.where(keep, f32(margin), f32(0))
        out.append(x)
    return np.stack(out)


def clip_classes(g, C):
    """labels for a C-class head: occupied classes folded into 1 .. C - 1"""
    return np.where(g == 0, 0, (g.astype(np.int64) - 1) % (C - 1) + 1).astype(np.uint8)
