"""The fill of unobserved voxel-label cells from neighbouring frames - include/muvo_hip.h: muvo_voxel_pose_chain and
muvo_voxel_aggregate, DESIGN.md section 18 - restated in numpy / Python float64.  Helpers only: no fixtures, no tests.

States.  Frame f = i s + t is time t of sequence i.  S(f, c) = the class v >= 1 of an occupied cell, 0 for a free cell that is SEEN,
UNK for a free cell that is not (the masked label of tests/visibility_reference.py with UNK in place of 255).
Poses.  T_t, 4 x 4 float64, p_{t-1} ~ T_t p_t in range-view coordinates (metres of the ego frame); a link is valid iff its status is
no failure code, its fitness >= min_fitness and its top three rows are finite.  M(t' <- t) is the product of the links between t
and t' (towards the past) or of their rigid inverses [R^T, -R^T tau] (towards the future), conjugated into cells by the affine map
g = a r + o.  Every sum is written in the order the header states; Python floats and numpy float64 do not contract.
Fill.  A(f, c) = S(f, c) unless UNK; else d = 1 .. window, t - d before t + d, skipping pairs that are not usable: q = M (c + 1/2),
j = floor(q); inside the grid and S(f', j) != UNK: A = S(f', j), stop.  Nothing found: 255."""
import math

import numpy as np

UNK = -1
ICP_FAILURES = (3, 4, 5)                    # MUVO_ICP_FEW_INLIERS, MUVO_ICP_EMPTY, MUVO_ICP_BAD_FRAME


def states(label, seen):
    """(…, X, Y, Z) int16: S of every cell from the label (uint8) and the SEEN plane (bool)"""
    label = np.asarray(label)
    return np.where(label != 0, label.astype(np.int16), np.where(np.asarray(seen, bool), 0, UNK)).astype(np.int16)


def link_valid(T, fitness=None, status=None, min_fitness=0.0):
    """one link: T (4, 4); fitness / status None: only finiteness decides"""
    ok = all(math.isfinite(float(v)) for v in np.asarray(T)[:3].reshape(-1))
    if fitness is not None:
        ok = ok and float(fitness) >= min_fitness                      # NaN: invalid
    if status is not None:
        ok = ok and int(status) not in ICP_FAILURES
    return bool(ok)


def rigid_inverse(L):
    """L: 12 floats, row-major 3 x 4 -> [R^T, -R^T tau]"""
    return [L[0], L[4], L[8], -((L[0] * L[3] + L[4] * L[7]) + L[8] * L[11]),
            L[1], L[5], L[9], -((L[1] * L[3] + L[5] * L[7]) + L[9] * L[11]),
            L[2], L[6], L[10], -((L[2] * L[3] + L[6] * L[7]) + L[10] * L[11])]


def compose(L, M):
    """L M for two 3 x 4 rigid matrices (12 floats each)"""
    out = []
    for a in range(3):
        l0, l1, l2, l3 = L[4 * a:4 * a + 4]
        out += [(l0 * M[0] + l1 * M[4]) + l2 * M[8], (l0 * M[1] + l1 * M[5]) + l2 * M[9], (l0 * M[2] + l1 * M[6]) + l2 * M[10],
                ((l0 * M[3] + l1 * M[7]) + l2 * M[11]) + l3]
    return out


def to_cells(M, cell_map):
    """A M A^-1 for the map g_a = cell_map[a] r_a + cell_map[3 + a]"""
    a, o = cell_map[:3], cell_map[3:]
    out = []
    for r in range(3):
        c = [(a[r] * M[4 * r + k]) / a[k] for k in range(3)]
        out += c + [(a[r] * M[4 * r + 3] + o[r]) - ((c[0] * o[0] + c[1] * o[1]) + c[2] * o[2])]
    return out


def chain(T, b, s, window, cell_map, fitness=None, status=None, min_fitness=0.0):
    """T (b (s - 1), 4, 4) -> (mats (b s, 2 window, 12) float64, usable (b s, 2 window) uint8): slot 2 (d - 1) is t' = t - d, slot
    2 (d - 1) + 1 is t' = t + d; a slot that is not usable holds zeros"""
    T = np.asarray(T, np.float64).reshape(b * (s - 1), 4, 4)
    cell_map = [float(v) for v in cell_map]
    mats = np.zeros((b * s, 2 * window, 12), np.float64)
    usable = np.zeros((b * s, 2 * window), np.uint8)
    for i in range(b):
        for t in range(s):
            for direction in (0, 1):
                M = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
                ok = True
                for d in range(1, window + 1):
                    tp = t + d if direction else t - d
                    ok = ok and 0 <= tp < s
                    if ok:
                        link = i * (s - 1) + (t + d - 1 if direction else t - d)
                        ok = link_valid(T[link], None if fitness is None else fitness[link], None if status is None else status[link], min_fitness)
                        if ok:
                            L = [float(v) for v in T[link, :3].reshape(-1)]
                            M = compose(rigid_inverse(L) if direction else L, M)
                    if ok:
                        mats[i * s + t, 2 * (d - 1) + direction] = to_cells(M, cell_map)
                        usable[i * s + t, 2 * (d - 1) + direction] = 1
    return mats, usable


def aggregate(label, seen, s, mats, usable, near=1e-9):
    """label (F, X, Y, Z) uint8, seen (F, X, Y, Z) bool -> (A (F, X, Y, Z) uint8, counts [filled occupied, filled free, still unknown]
    int64, close (F, X, Y, Z) bool: cells for which a component of some q that was looked at lies within `near` of an integer)"""
    label = np.asarray(label)
    F, X, Y, Z = label.shape
    assert F % s == 0 and mats.shape[:2] == usable.shape and mats.shape[0] == F
    S = states(label, seen)
    out = np.where(S == UNK, 255, S).astype(np.uint8)
    close = np.zeros(label.shape, bool)
    counts = np.zeros(3, np.int64)
    size = np.array([X, Y, Z], np.float64)
    for f in range(F):
        t = f % s
        pend = np.argwhere(S[f] == UNK)                                # (n, 3) cells still without a value
        for slot in range(usable.shape[1]):
            if not len(pend):
                break
            if not usable[f, slot]:
                continue
            d = slot // 2 + 1
            tp = t + d if slot % 2 else t - d
            assert 0 <= tp < s, 'a usable slot outside the sequence'
            fs = f - t + tp
            m = mats[f, slot]
            cx, cy, cz = pend[:, 0] + 0.5, pend[:, 1] + 0.5, pend[:, 2] + 0.5
            with np.errstate(all='ignore'):
                q = np.stack([((m[4 * r] * cx + m[4 * r + 1] * cy) + m[4 * r + 2] * cz) + m[4 * r + 3] for r in range(3)], 1)
                j = np.floor(q)
                inside = ((j >= 0) & (j < size)).all(1)                # NaN: outside
                hot = (np.abs(q - np.rint(q)) < near).any(1)
            close[f][tuple(pend[hot].T)] = True
            ji = np.where(inside[:, None], j, 0).astype(np.int64)
            src = np.where(inside, S[fs][ji[:, 0], ji[:, 1], ji[:, 2]], UNK)
            got = src != UNK
            out[f][tuple(pend[got].T)] = src[got].astype(np.uint8)
            counts[0] += int((src[got] != 0).sum())
            counts[1] += int((src[got] == 0).sum())
            pend = pend[~got]
        counts[2] += len(pend)
    return out, counts, close


# ---- poses ------------------------------------------------------------------------------------------------------------------------
def pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """4 x 4 float64: R = Rz(yaw) Ry(pitch) Rx(roll), angles in degrees, translation t"""
    y, p, r = (math.radians(v) for v in (yaw, pitch, roll))
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------
CELL_MAP = (5.0, 5.0, 5.0, 2.0, 3.0, 1.0)           # 0.2 m cells, the ego point in cell (2, 3, 1): the shape of ops.voxel_cell_map
MIN_FITNESS = 0.3
# link kinds, in metres of the ego frame: whole cells are multiples of 0.2
LINKS = {
    'identity': dict(T=pose()),
    'shift': dict(T=pose(t=(0.2, -0.4, 0.0))),
    'shift_z': dict(T=pose(t=(-0.2, 0.0, 0.2))),
    'yaw': dict(T=pose(yaw=3.7, t=(0.13, -0.071, 0.023))),
    'tilt': dict(T=pose(pitch=2.3, roll=-1.9, t=(-0.057, 0.091, 0.037))),
    'far': dict(T=pose(yaw=1.3, t=(1.47, 0.33, -0.21))),                          # throws most of a small grid outside
    'nan': dict(T=np.full((4, 4), np.nan)),
    'low_fitness': dict(T=pose(yaw=1.1, t=(0.031, 0.017, 0.0)), fitness=0.29),
    'few_inliers': dict(T=pose(t=(0.2, 0.0, 0.0)), status=3),
}
MIXES = {'a': ('identity', 'shift', 'yaw', 'tilt', 'shift_z', 'far', 'yaw', 'identity'),
         'b': ('yaw', 'low_fitness', 'shift', 'far', 'tilt', 'nan', 'few_inliers', 'yaw')}


def make_case(shape, b, s, window, classes, mix, seed):
    """One input of the aggregate tests: label (b s, X, Y, Z) uint8 with ~15 % occupied cells of `classes`, a hand-made SEEN plane -
    45 % of the cells at random plus one fully seen and one fully unseen x slab per frame -, links drawn in turn from MIXES[mix]
    (sequence i starts at offset 3 i), their fitness and status."""
    rng = np.random.default_rng(seed)
    F = b * s
    label = ((rng.random((F, *shape)) < 0.15) * rng.integers(1, classes, (F, *shape))).astype(np.uint8)
    seen = rng.random((F, *shape)) < 0.45
    for f in range(F):
        seen[f, f % shape[0]] = True
        seen[f, (f + 2) % shape[0]] = False
    kinds = [MIXES[mix][(3 * i + t) % len(MIXES[mix])] for i in range(b) for t in range(s - 1)]
    T = np.stack([LINKS[k]['T'] for k in kinds]).reshape(-1, 4, 4) if kinds else np.zeros((0, 4, 4))
    fitness = np.array([LINKS[k].get('fitness', 0.8) for k in kinds], np.float64)
    status = np.array([LINKS[k].get('status', 1) for k in kinds], np.int64)
    return dict(label=label, seen=seen, T=T, fitness=fitness, status=status, kinds=kinds, b=b, s=s, window=window, shape=tuple(shape))


def solve(case):
    """the restatement's answer to make_case: mats, usable, out, counts, close"""
    mats, usable = chain(case['T'], case['b'], case['s'], case['window'], CELL_MAP, case['fitness'], case['status'], MIN_FITNESS)
    out, counts, close = aggregate(case['label'], case['seen'], case['s'], mats, usable)
    return dict(mats=mats, usable=usable, out=out, counts=counts, close=close)
