"""Numpy restatement of the grid search of the on-device ICP (muvo_amd/csrc/icp.hip: icp_grid_* and icp_correspond_grid_kernel,
search='grid' of ops.icp_step / ops.icp_register) and the hand-made inputs of its tests.  Helpers only: no fixtures, no tests.
tests/test_icp_grid_reference.py (CPU) and tests/test_icp_grid_gpu.py (GPU) share everything here.

The restatement works in float32 and follows the kernel step by step: the same grid points (valid, three finite scaled
coordinates), the same cell edge (threshold / 8, doubled until the box has at most 2^17 cells, in float64), the same cell function
clamp(floor((v - lo) * (1 / h)), 0, dim - 1), the same visited range cell(q - r) .. cell(q + r) with r = max(thr (1 + 2^-12), 2^-60),
the same walk over Chebyshev rings and the same termination: after ring k the six border gaps (tested with the cell function
itself, see `side_gap`), L = m^2 of the smallest, stop iff best < L or thr^2 < L.  Within the cells the winner is the
lexicographic minimum of (d^2, target index).  Two planted errors can be switched on: `shrink` (the visited range loses its
outermost cell on every side) and `strict` (the walk stops on best <= L, so an equal distance in a farther ring is lost).

numpy has no fused multiply-add; the kernel computes d = fmaf(dz, dz, fmaf(dy, dy, dx dx)).  On the lattice inputs below every
coordinate is a multiple of 2^-3 of magnitude <= 64, so every difference, square and sum is exact in float32 and numpy, the
exhaustive kernel and the grid kernel must agree to the bit; elsewhere only indices and inlier sets are compared."""
import numpy as np

F = np.float32
CELLS = 1 << 17
EDGE = 0.125                     # cell edge / threshold before the cap
BIG = 1 << 24


def scaled_points(frame, scale):
    """(n, 3) float32 scaled coordinates of a (C, n) frame as the kernels load them, and the (n,) valid mask (range > 0)"""
    with np.errstate(invalid='ignore', over='ignore'):
        pts = (frame[:3].astype(F) * F(scale)).T
        return pts, frame[3] > 0


def cell(v, lo, inv, dim):
    """the kernel's icp_cell on float32 scalars or arrays"""
    with np.errstate(invalid='ignore', over='ignore'):
        t = np.floor((F(v) - F(lo)) * F(inv))
    t = np.asarray(t, F)
    c = np.where(t >= BIG, BIG, np.where(t > -BIG, np.where(np.isfinite(t), t, 0), -BIG)).astype(np.int64)
    return np.clip(c, 0, dim - 1)


def build(tgt, scale, thr):
    """the grid of one target frame (C, n): dict(lo (3,), h, inv, dims (3,), cend (cells + 1,), rec (m, 3), idx (m,))"""
    pts, valid = scaled_points(tgt, scale)
    keep = valid & np.isfinite(pts).all(1)
    idx = np.nonzero(keep)[0]
    P = pts[idx]
    if len(idx):
        lo, hi = P.min(0), P.max(0)
    else:
        lo = hi = np.zeros(3, F)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    h = min(max(float(F(thr) * F(EDGE)), 2.0 ** -100), 2.0 ** 126)
    while True:
        dims = np.floor(ext / h) + 2.0
        if dims.prod() <= CELLS or h >= 2.0 ** 126:
            break
        h = min(h * 2.0, 2.0 ** 126)
    h = F(h)
    inv = F(1.0) / h
    dims = dims.astype(np.int64)
    cx, cy, cz = (cell(P[:, a], lo[a], inv, dims[a]) for a in range(3))
    c = (cz * dims[1] + cy) * dims[0] + cx
    order = np.argsort(c, kind='stable')
    cend = np.zeros(int(dims.prod()) + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=int(dims.prod())), out=cend[1:])
    return dict(lo=lo.astype(F), h=h, inv=inv, dims=dims, cend=cend, rec=P[order], idx=idx[order])


def side_gap(q, lo, inv, h, dim, e, above):
    """the kernel's icp_side_gap: a lower bound of |q - p| for the grid points beyond cell e on one side, 0 where none is shown"""
    border = F(lo + F(F(e + 1 if above else e) * h))
    for s in (F(0), F(h * F(0.015625))):
        G = F(border - s) if above else F(border + s)
        c = int(cell(np.nextafter(G, F(-np.inf) if above else F(np.inf)), lo, inv, dim))
        if (c <= e) if above else (c >= e):
            return max(F(G - q) if above else F(q - G), F(0))
    return F(0)


def nearest(G, q, thr, shrink=0, strict=False, stats=None):
    """(float32 d^2, target index) of one moved query q (3,) float32; (inf, -1) without a candidate"""
    q = np.asarray(q, F)
    best, bj = F(np.inf), -1
    if not np.isfinite(q).all():
        return best, bj
    thr = F(thr)
    thr2 = F(thr * thr)
    r = max(F(thr * F(1.0 + 2.0 ** -12)), F(2.0 ** -60))
    lo, inv, h, dims = G['lo'], G['inv'], G['h'], G['dims']
    with np.errstate(over='ignore'):
        c = [int(cell(q[a], lo[a], inv, dims[a])) for a in range(3)]
        r0 = [int(cell(F(q[a] - r), lo[a], inv, dims[a])) for a in range(3)]
        r1 = [int(cell(F(q[a] + r), lo[a], inv, dims[a])) for a in range(3)]
    if shrink:                                                 # planted error: the outermost cell of the range is not visited
        r0 = [min(r0[a] + shrink, c[a]) for a in range(3)]
        r1 = [max(r1[a] - shrink, c[a]) for a in range(3)]
    kmax = max(max(c[a] - r0[a], r1[a] - c[a]) for a in range(3))
    rec, idx, cend = G['rec'], G['idx'], G['cend']
    for k in range(kmax + 1):
        for z in range(max(r0[2], c[2] - k), min(r1[2], c[2] + k) + 1):
            for y in range(max(r0[1], c[1] - k), min(r1[1], c[1] + k) + 1):
                row = (z * int(dims[1]) + y) * int(dims[0])
                if abs(z - c[2]) == k or abs(y - c[1]) == k:
                    runs = [(max(r0[0], c[0] - k), min(r1[0], c[0] + k))]
                else:
                    runs = [(x, x) for x in (c[0] - k, c[0] + k) if r0[0] <= x <= r1[0]]
                for a, b in runs:
                    first, last = int(cend[row + a]), int(cend[row + b + 1])
                    if last <= first:
                        continue
                    with np.errstate(over='ignore'):
                        diff = q[None, :] - rec[first:last]
                        d = diff[:, 2] * diff[:, 2] + (diff[:, 1] * diff[:, 1] + diff[:, 0] * diff[:, 0])
                    dmin = d.min()
                    jmin = int(idx[first:last][d == dmin].min())
                    if dmin < best or (dmin == best and jmin < bj):
                        best, bj = F(dmin), jmin
                    if stats is not None:
                        stats['candidates'] = stats.get('candidates', 0) + (last - first)
        if k == kmax:
            break
        m = F(np.inf)
        for a in range(3):
            if c[a] + k < r1[a]:
                m = min(m, side_gap(q[a], lo[a], inv, h, dims[a], c[a] + k, True))
            if c[a] - k > r0[a]:
                m = min(m, side_gap(q[a], lo[a], inv, h, dims[a], c[a] - k, False))
        with np.errstate(over='ignore'):
            L = F(m * m)
        if (best <= L if strict else best < L) or thr2 < L:
            if stats is not None:
                stats.setdefault('exit_ring', []).append(k)
            break
    return best, bj


def moved_queries(src, scale, T=None, stride=1):
    """(indices of the valid queries, their moved float32 coordinates (m, 3)): float32 scaling, float64 motion, rounded"""
    pts, valid = scaled_points(src, scale)
    i = np.nonzero(valid)[0]
    i = i[i % stride == 0]
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        x = pts[i].astype(np.float64)
        moved = np.stack([T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1] + T[r, 2] * x[:, 2] + T[r, 3] for r in range(3)], 1).astype(F)
    return i, moved


def grid_search(src, tgt, scale, thr, T=None, stride=1, **planted):
    """per source point (n,): float32 d^2 of the winner (inf: none) and its target index (-1: none / no query)"""
    n = src.shape[1]
    d2, idx = np.full(n, np.inf, F), np.full(n, -1, np.int64)
    G = build(tgt, scale, thr)
    qi, moved = moved_queries(src, scale, T, stride)
    for i, q in zip(qi, moved):
        d2[i], idx[i] = nearest(G, q, thr, **planted)
    return d2, idx


def brute_search(src, tgt, scale, thr, T=None, stride=1):
    """the exhaustive search in float32 numpy, non-finite coordinates as the kernel treats them: a NaN or inf distance never wins"""
    n = src.shape[1]
    d2, idx = np.full(n, np.inf, F), np.full(n, -1, np.int64)
    pts, valid = scaled_points(tgt, scale)
    ti = np.nonzero(valid)[0]
    qi, moved = moved_queries(src, scale, T, stride)
    if not len(ti):
        return d2, idx
    for i, q in zip(qi, moved):
        with np.errstate(invalid='ignore', over='ignore'):
            diff = q[None, :] - pts[ti]
            d = diff[:, 2] * diff[:, 2] + (diff[:, 1] * diff[:, 1] + diff[:, 0] * diff[:, 0])
        d = np.where(np.isnan(d), np.inf, d)
        j = int(np.argmin(d))                                  # the first minimum: the lowest index
        if d[j] < np.inf:
            d2[i], idx[i] = d[j], ti[j]
    return d2, idx


def corr_of(d2, idx, thr):
    """the correspondence array the kernels write: the index where d^2 <= thr^2 in float32, else -1"""
    thr2 = F(F(thr) * F(thr))
    return np.where((idx >= 0) & (d2 <= thr2), idx, -1).astype(np.int32)


# ================================================================================================ hand-made inputs
def frame(points, valid=None):
    """(m, 3) points -> (4, m) float32 frame, range 1 (0 where not valid)"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.ones((4, len(points)), F)
    out[:3] = points.T.astype(F)
    if valid is not None:
        out[3, ~np.asarray(valid, bool)] = 0
    return out


def thrice(points, seed):
    """every point three times at scattered indices"""
    points = np.asarray(points, np.float64)
    return np.concatenate([points] * 3)[np.random.default_rng(seed).permutation(3 * len(points))]


def _on_lattice(f):
    pts = f[:3][:, f[3] > 0]
    pts = pts[np.isfinite(pts)]
    return bool((np.abs(pts) <= 64).all() and (pts * 8 == np.round(pts * 8)).all())


CORNERS = [(sx * 64.0, sy * 64.0, sz * 8.0) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
Q0 = np.array((1.375, -2.75, 0.25))         # 3/4, 1/2, 1/2 into its cell of edge 1/2 (threshold 4) when the box starts at -64, -64, -8
TIES = (((5, 0, 0), (3, 4, 0)), ((0, 0, 5), (4, 0, 3)))


def _tie_input(k, kind, axis_first, corners=CORNERS):
    """two targets at exactly the same distance 5 * 2^k from Q0, the lower index on the axis-aligned one iff axis_first; the box
    corners fix the grid's extent.  No duplicates here: the order of the two IS the case."""
    A, B = (np.array(o, np.float64) * 2.0 ** k for o in TIES[kind])
    pair = [Q0 + A, Q0 + B] if axis_first else [Q0 + B, Q0 + A]
    tgt = pair + list(corners)
    src = [Q0, (-63.0, 63.0, 7.0), (40.5, -17.25, -3.125)]
    return frame(src), frame(tgt)


def lattice_inputs():
    """name -> dict(src (4, n), tgt (4, m), thr, init) with every valid coordinate a multiple of 2^-3 of magnitude <= 64"""
    out = {}
    for k in range(-3, 4):
        for kind in (0, 1):
            axis_first = (k + 3 + kind) % 2 == 0
            if abs(Q0 + np.array(TIES[kind][0]) * 2.0 ** k).max() > 64 or abs(Q0 + np.array(TIES[kind][1]) * 2.0 ** k).max() > 64:
                continue
            s, t = _tie_input(k, kind, axis_first)
            for thr in (64.0, 4.0):
                out[f'tie-k{k}-kind{kind}-thr{thr:g}'] = dict(src=s, tgt=t, thr=thr)
    # the tie the early exit must not lose: thr 4 -> cells of 1/2; Q0 + (5/8, 0, 0) lies exactly on a cell border, so in ring 2,
    # and has the lower index; Q0 + (3/8, 1/2, 0) at the same distance is in ring 1.  The box starts at x = 0: the border test
    # cell(prev(2.0)) is then exact (2.0 - ulp - 0), the x gap is the border itself, 5/8, and L = best to the bit.
    s, t = _tie_input(-3, 0, True, [(x, y, z) for x in (0.0, 16.0) for y in (-8.0, 8.0) for z in (-2.0, 2.0)])     # 34 x 34 x 10 cells of 1/2
    out['tie-on-the-border-of-ring-1'] = dict(src=s, tgt=t, thr=4.0)
    # a random lattice cloud, every target three times; the queries are other lattice points
    g = np.random.default_rng(5)
    cloud = np.round(g.uniform(-20, 20, (60, 3)) * 8) / 8
    cloud[:, 2] = np.round(g.uniform(-4, 4, 60) * 8) / 8
    qs = np.round((cloud[g.permutation(60)[:40]] + g.uniform(-3, 3, (40, 3))) * 8) / 8
    for thr in (4.0, 1.0, 32.0):
        out[f'cloud-thrice-thr{thr:g}'] = dict(src=frame(qs), tgt=frame(thrice(cloud, 9)), thr=thr)
    # exactly on the threshold, and the threshold one float32 step lower
    tgt = [Q0 + (4, 0, 0), Q0 + (0, -4, 0), Q0 + (0, 0, 4)] + CORNERS
    src = [Q0, Q0 + (8, 0, 0), Q0 + (0, -8, 0), Q0 + (0, 0, 8)]
    out['threshold-exact'] = dict(src=frame(src), tgt=frame(thrice(tgt, 2)), thr=4.0)
    out['threshold-one-step-lower'] = dict(src=frame(src), tgt=frame(thrice(tgt, 2)), thr=float(np.nextafter(F(4), F(0))))
    # queries outside the box of the targets: within the threshold of a face, just beyond it
    box = [(x, y, z) for x in (-4.0, 0.0, 4.0) for y in (-4.0, 0.0, 4.0) for z in (-1.0, 0.0, 1.0)]
    src = [(7.875, 0, 0), (8.0, 0, 0), (8.125, 0, 0), (0, -8.0, 1), (0, -8.125, 1), (0, 0, 5.0), (0, 0, 5.125), (-7.5, -7.5, 0), (60, 60, 8)]
    out['queries-outside-the-box'] = dict(src=frame(src), tgt=frame(thrice(box, 3)), thr=4.0)
    far = np.eye(4)
    far[0, 3] = 1e30
    out['queries-1e30-away-through-init'] = dict(src=frame(src), tgt=frame(thrice(box, 3)), thr=4.0, init=far)
    out['all-targets-identical'] = dict(src=frame([(1, 1, 1), (1.125, 1, 1), (5, 1, 1), (5.125, 1, 1)]), tgt=frame([(1, 1, 1)] * 7), thr=4.0)
    plane = [(x * 0.625, y * 1.125, 2.5) for x in range(-6, 7) for y in range(-4, 5)]
    src = [(x * 1.25 + 0.125, y * 0.75, z) for x in range(-3, 4) for y in range(-3, 4) for z in (2.5, 0.0, 6.0, 6.625)]
    out['all-targets-in-one-plane'] = dict(src=frame(src), tgt=frame(thrice(plane, 4)), thr=4.0)
    out['n1'] = dict(src=frame([(1.5, -2, 0.25)]), tgt=frame([(2.5, -2, 0.25)]), thr=4.0)
    many = [(x * 1.5, 0.5, -0.25) for x in range(-5, 6)]
    valid = np.zeros(11, bool)
    valid[7] = True
    out['one-valid-target-among-invalid'] = dict(src=frame([(4.5, 0.5, 0), (0, 0, 0), (9.0, 0.5, -0.25)]), tgt=frame(many, valid), thr=4.0)
    for name, inp in out.items():
        inp.setdefault('init', None)
        assert _on_lattice(inp['src']) and _on_lattice(inp['tgt']), name
    return out


def nonfinite_inputs():
    """name -> input with non-finite or huge coordinates at points whose range is > 0"""
    g = np.random.default_rng(11)
    cloud = np.round(g.uniform(-10, 10, (48, 3)) * 8) / 8
    qs = np.round((cloud[:24] + g.uniform(-2, 2, (24, 3))) * 8) / 8
    out = {}
    for name, bad in (('nan', np.nan), ('inf', np.inf), ('1e30', 1e30), ('1e18', 1e18)):
        t = frame(cloud)
        t[0, 5], t[1, 17], t[2, 30] = bad, bad, -bad
        t[:3, 40] = bad
        out[f'target-{name}'] = dict(src=frame(qs), tgt=t, thr=4.0, init=None)
    s = frame(qs)
    s[:3, 3] = np.nan
    s[1, 9] = np.nan
    s[0, 12] = np.inf
    out['source-nan'] = dict(src=s, tgt=frame(cloud), thr=4.0, init=None)
    return out
