"""Float64 restatement, inputs, case list, conditions and bars for the on-device ICP (muvo_amd/csrc/icp.hip through
ops.icp_step / ops.icp_register, muvo_amd/odometry.py).  Helpers only: no fixtures, no tests.  tests/test_icp_reference.py (CPU)
and tests/test_icp_gpu.py (GPU) share everything here, so the bars the GPU test applies are the ones the CPU test proves to
reject planted errors.

The restatement (`icp`).  open3d is not available, so this is the published algorithm of `registration_icp` with
TransformationEstimationPointToPoint (the call of compute_pcd_transformation, muvo/utils/geometry_utils.py:248-267), in numpy:
    evaluate:  every valid source point, moved by T, takes its nearest valid target point (squared distance from coordinate
               differences, LOWEST index on a tie); it is an inlier iff d^2 <= thr^2; fitness = inliers / valid source points,
               inlier_rmse = sqrt(sum d^2 / inliers)
    loop:      evaluate; if this is not the first evaluation and |d fitness| < 1e-6 and |d rmse| < 1e-6: stop, T unchanged;
               if `max_iteration` fits were applied: stop; else U = Kabsch / Umeyama without scale over the inlier pairs
               (numpy.linalg.svd of the centred cross-covariance, the reflection guarded by the determinant), T <- U T.
Own definitions (open3d leaves them open or does them differently): the moved points are always T applied to the ORIGINAL
points (open3d moves its copy step by step); fewer than 3 inliers stop the pair with T unchanged; no valid source or no valid
target point gives the identity at iteration 0 (the reference's `len(...) > 0`); `source_stride` k uses source points 0, k, 2k ...
It takes `dtype` (default float64): the same code with dtype=float32 is "the float32 CPU evaluation" of the bars.

Conditions (`reference(id)` asserts them before anything is judged; no case and no point is excluded):
    gap        per query and evaluation of the float64 run, (s2 - s1) / s2 >= GAP_MIN = 1e-4 for the smallest and second-smallest
               squared distance (1 with a single candidate): a float32 evaluation selects the same neighbour
    threshold  no nearest squared distance within THR_MARGIN = 1e-3 (relative) of thr^2: the same inliers
    stop       float32 and float64 restatement stop at the same iteration; at the stop both deltas are <= 1e-6 / 5, at every
               earlier evaluation the larger delta is >= 5e-6 (the first evaluation has no delta)

Bars.  icp_step sums: 4 x the error of the float32 evaluation of the same evaluation, normalised by the largest |sum| of its
group (count, d^2, s, q, s q^T), floored at 8 * 2^-24 as the loss scalars of loss_reference.py.  icp_register T: per entry
max(4 x |T_float32 - T_float64|, floor), the floor from the ulp of a 50 m coordinate in float32 (2^-18 m = 3.8e-6 m): every
stored coordinate and every moved source point carries up to half of it, and a rigid fit cannot be trusted below the unit of
its inputs, so translation entries get FLOOR_T = 4 ulp = 1.53e-5 m and rotation entries FLOOR_R = FLOOR_T / 50 = 3.05e-7 (the
rotation that moves a point at 50 m by FLOOR_T).  The floor matters where the float32 evaluation happens to be nearly exact
(n = 3, the empty cases: identity in both)."""
import functools
import zlib

import numpy as np

GAP_MIN = 1e-4
THR_MARGIN = 1e-3
STOP_TOL = 1e-6
STOP_FACTOR = 5.0
ULP_50M = 2.0 ** -18
FLOOR_T = 4 * ULP_50M
FLOOR_R = FLOOR_T / 50.0
SUM_FLOOR = 8 * 2.0 ** -24
SUM_GROUPS = ((0, 1), (1, 2), (2, 5), (5, 8), (8, 17))        # count, sum d^2, sum s, sum q, sum s q^T
RUNNING, CONVERGED, MAX_ITERATION, FEW_INLIERS, EMPTY = 0, 1, 2, 3, 4
THRESHOLD = 5.0


# ================================================================================================ restatement
def valid_mask(frame):
    """frame (C, n): range (plane 3) > 0; NaN is invalid"""
    with np.errstate(invalid='ignore'):
        return frame[3] > 0


def points_of(frame, scale, dtype, stride=1):
    """valid points of a (C, n) frame as (m, 3) in `dtype`, scaled in float32 as the kernels do, and their indices"""
    idx = np.nonzero(valid_mask(frame))[0]
    if stride > 1:
        idx = idx[idx % stride == 0]
    pts = (frame[:3, idx].astype(np.float32) * np.float32(scale)).T
    return pts.astype(dtype), idx


def nearest(q, s, chunk=256):
    """q (m, 3), s (k, 3): per q the smallest squared distance, its (lowest) index and the second-smallest squared distance"""
    m = q.shape[0]
    first, idx, second = np.empty(m, q.dtype), np.empty(m, np.int64), np.full(m, np.inf, q.dtype)
    for a in range(0, m, chunk):
        diff = q[a:a + chunk, None, :] - s[None, :, :]
        d2 = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
        i = np.argmin(d2, axis=1)                             # first minimal index
        rows = np.arange(d2.shape[0])
        first[a:a + chunk], idx[a:a + chunk] = d2[rows, i], i
        if s.shape[0] > 1:
            d2[rows, i] = np.inf
            second[a:a + chunk] = d2.min(axis=1)
    return first, idx, second


def evaluate(S, Q, T, thr, swap=None, drop=None):
    """S (m, 3) source points, Q (k, 3) target points, T (4, 4), all of one dtype -> dict: moved (m, 3), d2, idx (into Q), inlier
    mask, sums (17), fitness, rmse, gap, margin.  swap = (i, j): query i takes target j instead (planted error); drop = i: query
    i is left out of the inliers (planted error)."""
    dt = S.dtype
    moved = (S @ T[:3, :3].T + T[:3, 3]).astype(dt)
    d2, idx, second = nearest(moved, Q)
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = np.where(np.isinf(second), 1.0, np.where(second > 0, (second - d2) / second, 0.0))
    if swap is not None:
        i, j = swap
        idx = idx.copy()
        idx[i] = j
        d2 = d2.copy()
        d2[i] = ((moved[i] - Q[j]) ** 2).sum()
    thr2 = dt.type(thr) * dt.type(thr)
    inl = d2 <= thr2
    if drop is not None:
        inl = inl.copy()
        inl[drop] = False
    s, q = moved[inl], Q[idx[inl]]
    sums = np.zeros(17, dt)
    sums[0] = inl.sum()
    sums[1] = d2[inl].sum()
    sums[2:5], sums[5:8] = s.sum(0), q.sum(0)
    sums[8:17] = (s[:, :, None] * q[:, None, :]).sum(0).reshape(9)
    n_in = int(inl.sum())
    return dict(moved=moved, d2=d2, idx=idx, inlier=inl, sums=sums, fitness=n_in / max(len(S), 1),
                rmse=float(np.sqrt(sums[1] / n_in)) if n_in else 0.0, gap=gap,
                margin=np.abs(d2.astype(np.float64) - float(thr) ** 2) / float(thr) ** 2)


def kabsch(sums, guard=True):
    """the rigid motion (4, 4) that maps s onto q in the least-squares sense, from the 17 sums (dtype of `sums`)"""
    dt = sums.dtype
    n = sums[0]
    ms, mq = sums[2:5] / n, sums[5:8] / n
    H = sums[8:17].reshape(3, 3) / n - np.outer(ms, mq)       # sum (s - ms)(q - mq)^T / n
    U, _, Vt = np.linalg.svd(H)
    D = np.eye(3, dtype=dt)
    if guard and np.linalg.det(Vt.T @ U.T) < 0:
        D[2, 2] = -1
    R = (Vt.T @ D @ U.T).astype(dt)
    out = np.eye(4, dtype=dt)
    out[:3, :3], out[:3, 3] = R, mq - R @ ms
    return out


def icp(src, tgt, scale=1.0, thr=THRESHOLD, max_iteration=2000, init=None, stride=1, dtype=np.float64, order='UT', guard=True,
        keep=False):
    """src, tgt (C, n) frames -> dict(T (4, 4), fitness, rmse, iterations, status, history).  history: per evaluation (fitness,
    rmse, d fitness, d rmse, min gap, min margin); keep: also the evaluations themselves.  order = 'TU' and guard = False are
    planted errors."""
    dt = np.dtype(dtype)
    S, _ = points_of(src, scale, dt, stride)
    Q, _ = points_of(tgt, scale, dt)
    T = np.eye(4, dtype=dt) if init is None else np.asarray(init, dt).copy()
    out = dict(T=T, fitness=0.0, rmse=0.0, iterations=0, status=EMPTY, history=[], evals=[])
    if len(S) == 0 or len(Q) == 0:
        out['T'] = np.eye(4, dtype=dt)
        return out
    prev, it = None, 0
    while True:
        ev = evaluate(S, Q, T, thr)
        dfit = abs(ev['fitness'] - prev['fitness']) if prev is not None else None
        drmse = abs(ev['rmse'] - prev['rmse']) if prev is not None else None
        out['history'].append((ev['fitness'], ev['rmse'], dfit, drmse, float(ev['gap'].min()), float(ev['margin'].min())))
        if keep:
            out['evals'].append(ev)
        out['fitness'], out['rmse'] = ev['fitness'], ev['rmse']
        if ev['sums'][0] < 3:
            status = FEW_INLIERS
        elif prev is not None and dfit < STOP_TOL and drmse < STOP_TOL:
            status = CONVERGED
        elif it >= max_iteration:
            status = MAX_ITERATION
        else:
            U = kabsch(ev['sums'], guard)
            T = (U @ T if order == 'UT' else T @ U).astype(dt)
            it += 1
            prev = ev
            continue
        out.update(T=T, iterations=it, status=status)
        return out


def assert_conditions(r64, r32, tag=''):
    """the conditions of the module docstring on a float64 run and its float32 twin"""
    for k, (_, _, dfit, drmse, gap, margin) in enumerate(r64['history']):
        assert gap >= GAP_MIN, f'{tag}: evaluation {k}: a query with a nearest / second-nearest gap of {gap:.2e} (< {GAP_MIN:g})'
        assert margin >= THR_MARGIN, f'{tag}: evaluation {k}: a nearest distance within {margin:.2e} of the threshold'
    assert r64['iterations'] == r32['iterations'] and r64['status'] == r32['status'], \
        f"{tag}: float64 stops at {r64['iterations']} ({r64['status']}), float32 at {r32['iterations']} ({r32['status']})"
    for name, r in (('float64', r64), ('float32', r32)):
        last = len(r['history']) - 1
        for k, (_, _, dfit, drmse, _, _) in enumerate(r['history']):
            if dfit is None:
                continue
            big = max(dfit, drmse)
            if k == last and r['status'] == FEW_INLIERS:
                continue                                     # stopped by the inlier count, whatever the deltas
            if k == last and r['status'] == CONVERGED:
                assert big <= STOP_TOL / STOP_FACTOR, f'{tag}: {name}: the stopping deltas ({dfit:.2e}, {drmse:.2e}) are not 5 x below 1e-6'
            else:
                assert big >= STOP_TOL * STOP_FACTOR, \
                    f'{tag}: {name}: evaluation {k} continues with deltas ({dfit:.2e}, {drmse:.2e}) less than 5 x above 1e-6'


# ================================================================================================ bars
def t_bar(T64, T32):
    """(4, 4) per-entry bound on |T_gpu - T64|"""
    floor = np.full((4, 4), FLOOR_R)
    floor[:3, 3] = FLOOR_T
    return np.maximum(4 * np.abs(T32.astype(np.float64) - T64), floor)


def t_failures(T, T64, T32):
    err = np.abs(np.asarray(T, np.float64)[:3] - T64[:3])
    return err, t_bar(T64, T32)[:3], bool((err > t_bar(T64, T32)[:3]).any())


def sums_error(got, ref):
    """per group the largest |got - ref| over the group's largest |ref| (1 where the group is all zero)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    out = []
    for a, b in SUM_GROUPS:
        scale = np.abs(ref[a:b]).max()
        out.append(float(np.abs(got[a:b] - ref[a:b]).max() / (scale if scale > 0 else 1.0)))
    return np.array(out)


def sums_bar(ref32, ref64):
    return np.maximum(4 * sums_error(ref32, ref64), SUM_FLOOR)


# ================================================================================================ scene
SPHERES = ((9.0, 4.0, -0.5, 2.5), (-7.0, 9.0, 0.0, 3.0), (-12.0, -6.0, -1.0, 2.0), (6.0, -10.0, 0.5, 3.0))
WALLS = (24.0, 17.0)          # |x| = 24, |y| = 17
GROUND = -2.0


def pose(dx, dy, yaw_deg):
    c, s = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    T = np.eye(4)
    T[:3, :3] = ((c, -s, 0), (s, c, 0), (0, 0, 1))
    T[:3, 3] = (dx, dy, 0)
    return T


def ray_cast(T, h, w, jitter=None):
    """the scene seen from the sensor pose T (world <- sensor): h x w rays over +-180 deg x [-30, 10] deg -> (4, h w) float64
    x, y, z, range in the SENSOR frame; range = 0 where nothing is hit within 50 m"""
    az = -np.pi + (np.arange(w) + 0.5) * (2 * np.pi / w)
    el = np.radians(-30 + (np.arange(h) + 0.5) * (40.0 / h))
    az, el = np.meshgrid(az, el)
    if jitter is not None:
        az, el = az + jitter[0], el + jitter[1]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    dw = d @ T[:3, :3].T
    o = T[:3, 3]
    best = np.full(len(d), np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = (GROUND - o[2]) / dw[:, 2]
        best = np.where((t > 0) & (t < best), t, best)
        for axis, lim in ((0, WALLS[0]), (1, WALLS[1])):
            for sign in (-1, 1):
                t = (sign * lim - o[axis]) / dw[:, axis]
                best = np.where((t > 0) & (t < best), t, best)
        for cx, cy, cz, r in SPHERES:
            oc = o - np.array((cx, cy, cz))
            b = dw @ oc
            disc = b * b - (oc @ oc - r * r)
            t = -b - np.sqrt(disc)
            best = np.where((disc > 0) & (t > 0) & (t < best), t, best)
    rng = np.where(best < 50.0, best, 0.0)
    return np.concatenate([(d * rng[:, None]).T, rng[None]], 0)


def frame_of(cloud, C, scale, invalid=None, nan=True):
    """(4, n) metric cloud -> (C, n) float32 planes / scale; `invalid` (bool mask): range 0 there; invalid points get NaN
    coordinates (nan) - planes >= 4 are NaN throughout"""
    n = cloud.shape[1]
    out = np.full((C, n), np.nan, np.float32)
    out[:4] = (cloud / scale).astype(np.float32)
    if invalid is not None:
        out[3, invalid] = 0.0
    bad = ~(out[3] > 0)
    out[:3, bad] = np.nan if nan else 0.0
    return out


def case(id, h, w, motion=(1.0, 0.1, 2.0), C=4, scale=1.0, stride=1, invalid=0.0, content='scene', seed=0, thr=THRESHOLD):
    return dict(id=id, h=h, w=w, n=h * w, motion=motion, C=C, scale=scale, stride=stride, invalid=invalid, content=content, seed=seed,
                thr=thr)


# seeds: the first for which assert_conditions holds (python tests/icp_reference.py --seeds)
CASES = [
    case('n1-single-point', 1, 1, content='rigid'),
    case('n3-three-points', 1, 3, content='rigid'),
    case('n1024-one-tile', 32, 32, motion=(0.5, 0.1, 1.5), content='noisy'),
    case('n1025-tile-plus-one', 25, 41, motion=(0.5, 0.1, 1.5), content='noisy'),
    case('n2500-ragged-tile', 50, 50, motion=(0.5, 0.1, 1.5), content='noisy', seed=18),
    case('n2500-rigid-copy-known-answer', 50, 50, motion=(0.3, 0.0, 1.0), content='rigid'),
    case('n1025-invalid-10pct-nan', 25, 41, motion=(0.5, 0.1, 1.5), invalid=0.1, content='noisy'),
    case('n300-source-all-invalid', 10, 30, content='src-empty'),
    case('n300-target-all-invalid', 10, 30, content='tgt-empty'),
    case('n1025-large-motion-fitness-below-1', 25, 41, motion=(2.0, 0.5, 4.0), thr=1.0, seed=6),
    case('n1025-scale-100', 25, 41, scale=100.0, seed=23),
    case('n1025-C5', 25, 41, C=5, seed=4),
    case('n1025-stride-3', 25, 41, stride=3),
]
CASE = {c['id']: c for c in CASES}
MULTI = ('n1025-C5', 'n3-three-points', 'n2500-ragged-tile', 'n300-source-all-invalid')      # 9, 2, 5 and 0 iterations


def _seed(id, seed):
    return zlib.crc32(id.encode()) % (1 << 30) + 7919 * seed


@functools.lru_cache(maxsize=None)
def inputs(id):
    """(src (C, n), tgt (C, n), truth (4, 4) or None) float32 frames of a case: tgt = the scene from the first pose, src = from
    the pose `motion` away; truth maps src onto tgt"""
    c = CASE[id]
    g = np.random.default_rng(_seed(id, c['seed']))
    h, w, n = c['h'], c['w'], c['n']
    truth = pose(*c['motion'])
    jit = (g.uniform(-0.2, 0.2, (h, w)) * (2 * np.pi / w), g.uniform(-0.2, 0.2, (h, w)) * np.radians(40.0 / h))
    tgt_cloud = ray_cast(np.eye(4), h, w, jit)
    if c['content'] in ('rigid', 'noisy'):
        # the target is an exact rigid copy of the source, permuted: the answer is known without the oracle
        if n <= 3:
            src_cloud = np.zeros((4, n))
            src_cloud[:3] = g.uniform(-10, 10, (3, n))
            src_cloud[3] = np.linalg.norm(src_cloud[:3], axis=0)
        else:
            src_cloud = ray_cast(truth, h, w, jit)
        perm = g.permutation(n)
        moved = truth[:3, :3] @ src_cloud[:3] + truth[:3, 3:4]
        if c['content'] == 'noisy':                          # every target point 2 cm (sigma) off its rigid copy: rmse > 0
            moved = moved + g.normal(0.0, 0.02, moved.shape)
        tgt_cloud = np.concatenate([moved, src_cloud[3:4]], 0)[:, perm]
    else:
        jit2 = (g.uniform(-0.2, 0.2, (h, w)) * (2 * np.pi / w), g.uniform(-0.2, 0.2, (h, w)) * np.radians(40.0 / h))
        src_cloud = ray_cast(truth, h, w, jit2)
    inv_s = g.random(n) < c['invalid'] if c['invalid'] else None
    inv_t = g.random(n) < c['invalid'] if c['invalid'] else None
    if c['content'] == 'src-empty':
        inv_s = np.ones(n, bool)
    if c['content'] == 'tgt-empty':
        inv_t = np.ones(n, bool)
    return frame_of(src_cloud, c['C'], c['scale'], inv_s), frame_of(tgt_cloud, c['C'], c['scale'], inv_t), truth


@functools.lru_cache(maxsize=None)
def reference(id):
    """(float64 run, float32 run) of a case, computed once and shared (treat as read-only); the conditions are asserted"""
    c = CASE[id]
    src, tgt, _ = inputs(id)
    r64 = icp(src, tgt, c['scale'], c['thr'], stride=c['stride'], keep=True)
    r32 = icp(src, tgt, c['scale'], c['thr'], stride=c['stride'], dtype=np.float32, keep=True)
    assert_conditions(r64, r32, id)
    return r64, r32


def corr_full(id, ev):
    """the (n,) int32 correspondence array the kernel writes for evaluation `ev` of a case: target index per source point, -1
    where the point is invalid, gated out, or (stride) no query; target indices count ALL target points"""
    c = CASE[id]
    src, tgt, _ = inputs(id)
    _, si = points_of(src, c['scale'], np.float64, c['stride'])
    _, ti = points_of(tgt, c['scale'], np.float64)
    out = np.full(c['n'], -1, np.int32)
    out[si[ev['inlier']]] = ti[ev['idx'][ev['inlier']]]
    return out


TRAJ_SEED = 0                 # the first seed for which assert_conditions holds for all four pairs (--traj-seed)
TRAJ_MOTIONS = (((0.5, 0.1, 1.5), (0.4, -0.1, -1.0)), ((0.6, 0.0, 2.0), (0.3, 0.1, 1.0)))


@functools.lru_cache(maxsize=None)
def trajectory_batch(seed=TRAJ_SEED, h=25, w=41):
    """a (2, 3, 4, h, w) float32 batch whose frame t moves onto frame t - 1 by TRAJ_MOTIONS[b][t - 1] up to 2 cm of noise per
    point (every frame a permuted copy of the middle one), and the (2, 2, 4, 4) float64 / float32 restatement poses"""
    g = np.random.default_rng(1000 + seed)
    n = h * w
    rv = np.zeros((2, 3, 4, n), np.float32)
    for b in range(2):
        jit = (g.uniform(-0.2, 0.2, (h, w)) * (2 * np.pi / w), g.uniform(-0.2, 0.2, (h, w)) * np.radians(40.0 / h))
        mid = ray_cast(pose(0.3 * b, 0.2, 5.0 * b), h, w, jit)
        T1, T2 = pose(*TRAJ_MOTIONS[b][0]), pose(*TRAJ_MOTIONS[b][1])
        first = np.concatenate([T1[:3, :3] @ mid[:3] + T1[:3, 3:4] + g.normal(0, 0.02, (3, n)), mid[3:4]], 0)[:, g.permutation(n)]
        inv = np.linalg.inv(T2)
        last = np.concatenate([inv[:3, :3] @ (mid[:3] + g.normal(0, 0.02, (3, n))) + inv[:3, 3:4], mid[3:4]], 0)[:, g.permutation(n)]
        for t, cloud in enumerate((first, mid, last)):
            rv[b, t] = frame_of(cloud, 4, 1.0)
    T64, T32 = np.zeros((2, 2, 4, 4)), np.zeros((2, 2, 4, 4), np.float32)
    for b in range(2):
        for t in (1, 2):
            r64, r32 = (icp(rv[b, t], rv[b, t - 1], dtype=dt) for dt in (np.float64, np.float32))
            assert_conditions(r64, r32, f'trajectory batch: sample {b} step {t}')
            T64[b, t - 1], T32[b, t - 1] = r64['T'], r32['T']
    return rv.reshape(2, 3, 4, h, w), T64, T32


# ================================================================================================ trajectory
def chain(Ts):
    """Ts (s - 1, 4, 4) -> Rot (s, 3, 3), pos (s, 3): compute_pcd_transformation's lines 262-265, step by step"""
    path = [{'Rot': np.eye(3), 'pos': np.zeros((3, 1))}]
    for transformation in Ts:
        Rt = path[-1]
        R = transformation[:3, :3]
        t = transformation[:3, -1:]
        Rot = R @ Rt['Rot']
        pos = Rt['pos'] + Rt['Rot'] @ t
        path.append({'Rot': Rot, 'pos': pos})
    return np.stack([p['Rot'] for p in path]), np.stack([p['pos'][:, 0] for p in path])


def _line(img, p0, p1, colour):
    """Bresenham, all octants, both end points, pixels off the canvas dropped; p = (x, y)"""
    x0, y0 = p0
    x1, y1 = p1
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx + dy
    while True:
        if 0 <= x0 < img.shape[1] and 0 <= y0 < img.shape[0]:
            img[y0, x0] = colour
        if x0 == x1 and y0 == y1:
            return
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def _disc(img, centre, colour):
    cx, cy = centre
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx * dx + dy * dy <= 4 and 0 <= cx + dx < img.shape[1] and 0 <= cy + dy < img.shape[0]:
                img[cy + dy, cx + dx] = colour


def plot_traj(traj, img):
    """trainer.py:969-978 with cv2.line / cv2.circle replaced by the own definitions (1-pixel Bresenham, disc dx^2 + dy^2 <= 4)"""
    x, y, z = traj[-1]['pos']
    plot_x = int(96 - 5 * y)
    plot_y = int(96 - 5 * x)
    x_, y_, _ = traj[-2]['pos'] if len(traj) > 1 else traj[-1]['pos']
    plot_x_ = int(96 - 5 * y_)
    plot_y_ = int(96 - 5 * x_)
    _line(img, (plot_x, plot_y), (plot_x_, plot_y_), (20, 150, 20))
    _disc(img, (plot_x, plot_y), (150, 20, 20))
    return img


def render_traj_ref(pos_label, pos_rows):
    """trainer.py:809-840 for positions that are given: pos_label (b, s, 3), pos_rows list of (b, s, 3) -> (b, 3, 196, 196 (1 + rows)) uint8"""
    out = []
    for bs in range(pos_label.shape[0]):
        path_target = [{'pos': np.zeros(3)}]
        traj_target = np.pad(np.zeros((192, 192)), pad_width=2, mode='constant', constant_values=50)
        traj_target = np.tile(traj_target[..., None], (1, 1, 3))
        traj_target = plot_traj(path_target, traj_target)
        path_preds = [[{'pos': np.zeros(3)}] for _ in pos_rows]
        traj_preds = [traj_target.copy() for _ in pos_rows]
        for step in range(1, pos_label.shape[1]):
            path_target.append({'pos': pos_label[bs, step]})
            traj_target = plot_traj(path_target, traj_target)
            for j, rows in enumerate(pos_rows):
                if step < rows.shape[1]:                    # a row without imagined steps ends after the reconstruction
                    path_preds[j].append({'pos': rows[bs, step]})
                    traj_preds[j] = plot_traj(path_preds[j], traj_preds[j])
        traj = np.concatenate([traj_target, *traj_preds], axis=1).transpose((2, 0, 1))[None]
        out.append(traj.astype(np.uint8))
    return np.concatenate(out, 0)


if __name__ == '__main__':
    import sys
    import time
    if '--traj-seed' in sys.argv:
        for seed in range(40):
            try:
                trajectory_batch(seed)
                print('trajectory batch: seed', seed)
                break
            except AssertionError as e:
                print('   ', str(e)[:150])
        sys.exit(0)
    if '--seeds' in sys.argv:
        for c in [c for c in CASES if not sys.argv[2:] or c['id'] in sys.argv[2:]]:
            for seed in range(40):
                c['seed'] = seed
                inputs.cache_clear()
                reference.cache_clear()
                try:
                    reference(c['id'])
                    break
                except AssertionError as e:
                    print('   ', str(e)[:150])
            print(f"{c['id']}: seed {seed}")
    for c in [c for c in CASES if not sys.argv[2:] or c['id'] in sys.argv[2:]]:
        t0 = time.time()
        r64, r32 = reference(c['id'])
        truth = inputs(c['id'])[2]
        print(f"{c['id']:45s} it {r64['iterations']:3d} status {r64['status']} fit {r64['fitness']:.4f} rmse {r64['rmse']:.3e} "
              f"|T32-T64| {np.abs(r32['T'] - r64['T']).max():.2e} |T64-truth| {np.abs(r64['T'] - truth).max():.2e} {time.time() - t0:.1f}s")
