"""The ray march of include/muvo_hip.h (muvo_raycast) restated in numpy float32, statement by statement - the kernels of
csrc/raycast.hip are compared with it bit for bit - plus a float64 brute-force ray / box search it is itself checked against, the
brick packing, the shading and the assembly of the `_voxel` panel, the RayIoU counts, the ray generators and the test scenes."""
import math

import numpy as np

f32 = np.float32
MISS = (-1, f32(0), 0)
SHADE = (176, 208, 255, 255)
THRESHOLDS = (1.0, 2.0, 4.0)


# ---- the march -----------------------------------------------------------------------------------------------------------------
def _cell(p, N):
    f = np.floor(p)
    return 0 if not (f >= 0) else (N - 1 if f > f32(N - 1) else int(f))


def march(grid, ray):
    """(linear index or -1, t float32, face) of one ray (7 float32) through grid (X, Y, Z) uint8"""
    with np.errstate(all='ignore'):
        N = grid.shape
        o, d, tmax = [f32(v) for v in ray[:3]], [f32(v) for v in ray[3:6]], f32(ray[6])
        t0, t1, entry, inv, moving = f32(0), tmax, 3, [f32(0)] * 3, False
        for a in range(3):
            if d[a] != 0:
                inv[a] = f32(1) / d[a]
                ta, tb = (f32(0) - o[a]) * inv[a], (f32(N[a]) - o[a]) * inv[a]
                lo, hi = (ta, tb) if ta <= tb else (tb, ta)
                if not (lo <= hi):
                    return MISS
                if lo > t0:
                    t0, entry = lo, a
                if hi < t1:
                    t1 = hi
                moving = True
            elif not (f32(0) <= o[a] and o[a] < f32(N[a])):
                return MISS
        if not moving or not (t0 < t1):
            return MISS
        c = [_cell(o[a] + d[a] * t0, N[a]) for a in range(3)]
        t, face = t0, entry
        for _ in range(N[0] + N[1] + N[2] + 3):
            if grid[c[0], c[1], c[2]] != 0:
                return (c[0] * N[1] + c[1]) * N[2] + c[2], t, face
            best, axis = f32(np.inf), -1
            for a in range(3):
                if d[a] != 0:
                    tn = (f32(c[a] + (1 if d[a] > 0 else 0)) - o[a]) * inv[a]
                    if tn < best:
                        best, axis = tn, a
            if axis < 0 or best > t1:
                return MISS
            c[axis] += 1 if d[axis] > 0 else -1
            if c[axis] < 0 or c[axis] >= N[axis]:
                return MISS
            t, face = best, axis
        return MISS


def cast(grid, rays):
    """(hit int32, t float32, face uint8) of rays (R, 7) through one grid"""
    out = [march(grid, r) for r in np.asarray(rays, f32)]
    return (np.array([h for h, _, _ in out], np.int32), np.array([t for _, t, _ in out], f32), np.array([f for _, _, f in out], np.uint8))


def brute_force(grid, ray):
    """float64, no traversal: the occupied cell whose box the ray enters first inside [0, tmax] -> (linear index or -1, t, the gap
    to the second nearest entry or inf).  Boxes the ray only touches (entry == exit) do not count."""
    N = grid.shape
    o, d, tmax = np.asarray(ray[:3], np.float64), np.asarray(ray[3:6], np.float64), float(ray[6])
    cells = np.argwhere(grid != 0).astype(np.float64)
    if not len(cells) or not np.isfinite(d).all() or not np.isfinite(o).all() or not d.any():
        return -1, 0.0, math.inf
    tin, tout = np.zeros(len(cells)), np.full(len(cells), tmax)
    inside = np.ones(len(cells), bool)
    for a in range(3):
        if d[a] != 0:
            ta, tb = (cells[:, a] - o[a]) / d[a], (cells[:, a] + 1 - o[a]) / d[a]
            tin, tout = np.maximum(tin, np.minimum(ta, tb)), np.minimum(tout, np.maximum(ta, tb))
        else:
            inside &= (cells[:, a] <= o[a]) & (o[a] < cells[:, a] + 1)
    ok = inside & (tin < tout)
    if not ok.any():
        return -1, 0.0, math.inf
    order = np.argsort(np.where(ok, tin, np.inf), kind='stable')
    x, y, z = (int(v) for v in cells[order[0]])
    gap = tin[order[1]] - tin[order[0]] if ok.sum() > 1 else math.inf
    return (x * N[1] + y) * N[2] + z, float(tin[order[0]]), float(gap)


# ---- bricks, shading, panel ------------------------------------------------------------------------------------------------------
def pack_bricks(grid):
    """uint64 (ceil(X/4) ceil(Y/4) ceil(Z/4),): bit (x&3) 16 + (y&3) 4 + (z&3) of word ((x>>2) BY + (y>>2)) BZ + (z>>2)"""
    X, Y, Z = grid.shape
    BX, BY, BZ = (X + 3) // 4, (Y + 3) // 4, (Z + 3) // 4
    words = np.zeros(BX * BY * BZ, np.uint64)
    for x, y, z in np.argwhere(grid != 0):
        words[((x >> 2) * BY + (y >> 2)) * BZ + (z >> 2)] |= np.uint64(1) << np.uint64((x & 3) * 16 + (y & 3) * 4 + (z & 3))
    return words


def palette256(table):
    pal = np.zeros((256, 3), np.uint8)
    for c in range(256):
        pal[c] = table[c] if c < len(table) else ((37 * c) % 256, (91 * c + 60) % 256, (151 * c + 120) % 256)
    return pal


def view_tile(grid, rays, R, palette, pad=2, padbyte=204):
    """(3, R + 2 pad, R + 2 pad) uint8: ray i R + j is pixel (i, j)"""
    Z = grid.shape[2]
    hit, _, face = cast(grid, rays)
    tile = np.full((3, R + 2 * pad, R + 2 * pad), padbyte, np.uint8)
    flat = grid.reshape(-1)
    for k in range(R * R):
        if hit[k] < 0:
            rgb = [int(v) for v in palette[0]]
        else:
            s = SHADE[face[k]] * (96 + (159 * int(hit[k] % Z)) // max(Z - 1, 1))
            rgb = [(int(p) * s) // 65025 for p in palette[flat[hit[k]]]]
        tile[:, pad + k // R, pad + k % R] = rgb
    return tile


def panel(label, recon, imagines, rays, R, palette, pad=2, padbyte=204):
    """label (b, s, X, Y, Z), recon (b, rf, X, Y, Z), imagines [(b, s - rf, X, Y, Z)] uint8 class grids -> the `_voxel` panel
    (b, 3, (1 + rows) T, s T [+ sep]), T = R + 2 pad: row 0 the label; row 1 + i the reconstruction (i = 0) or blank tiles of class
    0, then imagination i; sep = int(T / 4) columns of 255 before step rf when rf < s."""
    b, s = label.shape[:2]
    rf = recon.shape[1]
    T = R + 2 * pad
    sep = int(T / 4) if rf < s else 0
    rows = max(len(imagines), 1)
    out = np.zeros((b, 3, (1 + rows) * T, s * T + sep), np.uint8)
    blank = np.full((3, T, T), padbyte, np.uint8)
    blank[:, pad:-pad, pad:-pad] = palette[0][:, None, None]
    cache = {}

    def tile(g):
        key = g.tobytes()
        if key not in cache:
            cache[key] = view_tile(g, rays, R, palette, pad, padbyte)
        return cache[key]
    for n in range(b):
        for t in range(s):
            x = t * T + (sep if t >= rf else 0)
            out[n, :, :T, x:x + T] = tile(label[n, t])
            for i in range(rows):
                if t < rf:
                    img = tile(recon[n, t]) if i == 0 else blank
                elif imagines:
                    img = tile(imagines[i][n, t - rf])
                else:
                    continue
                out[n, :, (1 + i) * T:(2 + i) * T, x:x + T] = img
        if sep:
            out[n, :, :, rf * T:rf * T + sep] = 255
    return out


# ---- RayIoU ----------------------------------------------------------------------------------------------------------------------
def iou_counts(label_hits, pred_hits, C, res, thresholds=THRESHOLDS):
    """hits: [(class or -1 for a miss, t float32)] per ray -> (counts (3, C, 3) int64 [threshold][class][tp, fp, fn], the fp32 terms
    fabsf(tp - tl) res of the rays that hit in both)"""
    counts, terms = np.zeros((3, C, 3), np.int64), []
    for (cl, tl), (cp, tp) in zip(label_hits, pred_hits):
        both = cl >= 0 and cp >= 0
        err = np.abs(f32(tp) - f32(tl)) * f32(res) if both else f32(0)
        if both:
            terms.append(err)
        for k, thr in enumerate(thresholds):
            if both and cl == cp and err <= f32(thr):
                counts[k, cl, 0] += 1
            else:
                if cl >= 0:
                    counts[k, cl, 2] += 1
                if cp >= 0:
                    counts[k, cp, 1] += 1
    return counts, np.array(terms, f32)


def class_hits(grid, rays):
    hit, t, _ = cast(grid, rays)
    flat = grid.reshape(-1)
    return [(int(flat[h]) if h >= 0 else -1, tt) for h, tt in zip(hit, t)]


def ray_iou(counts):
    """counts (3, C, 3) -> the three means over the classes 1 .. C - 1 that occur (0.0 without one)"""
    out = []
    for k in range(3):
        ious = [counts[k, c, 0] / counts[k, c].sum() for c in range(1, counts.shape[1]) if counts[k, c].sum() > 0]
        out.append(float(np.mean(ious)) if ious else 0.0)
    return out


# ---- ray generators ----------------------------------------------------------------------------------------------------------------
def camera_rays(X, Y, Z, R, elev=60.0, azim=165.0):
    e, a = math.radians(elev), math.radians(azim)
    back = np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)])
    right = np.array([-math.sin(a), math.cos(a), 0.0])
    up = np.array([back[1] * right[2] - back[2] * right[1], back[2] * right[0] - back[0] * right[2], back[0] * right[1] - back[1] * right[0]])
    half = 0.5 * math.sqrt(X * X + Y * Y + Z * Z)
    centre = np.array([X, Y, Z]) / 2
    rays = np.zeros((R * R, 7))
    for i in range(R):
        for j in range(R):
            u, v = ((j + 0.5) / R * 2 - 1) * half, (1 - (i + 0.5) / R * 2) * half
            rays[i * R + j] = [*(centre + 2 * half * back + u * right + v * up), *(-back), 4 * half]
    return rays.astype(f32)


def fan_rays(origin, H, W, fov_up, fov_down):
    """H x W unit directions about one origin: yaw = pi (1 - 2 (c + 1/2) / W), pitch from fov_up to fov_down (degrees) at (r + 1/2) / H"""
    rays = np.zeros((H * W, 7))
    for r in range(H):
        p = math.radians(fov_up + (fov_down - fov_up) * (r + 0.5) / H)
        for c in range(W):
            y = math.pi * (1 - 2 * (c + 0.5) / W)
            rays[r * W + c] = [*origin, math.cos(p) * math.cos(y), math.cos(p) * math.sin(y), math.sin(p), math.inf]
    return rays.astype(f32)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
X, Y, Z = 13, 10, 7
R = 24


def scene():
    rng = np.random.default_rng(0)
    g = (rng.random((X, Y, Z)) < 0.06) * rng.integers(1, 9, (X, Y, Z))
    g[:, :, 0] = np.where(rng.random((X, Y)) < 0.7, 1, 0)
    return g.astype(np.uint8)


def corner_scene():
    g = np.zeros((X, Y, Z), np.uint8)
    g[X - 1, Y - 1, Z - 1] = 5
    return g


def cube_scene():
    """8 x 8 x 8: the unpadded brick path"""
    rng = np.random.default_rng(1)
    g = (rng.random((8, 8, 8)) < 0.08) * rng.integers(1, 9, (8, 8, 8))
    g[:, :, 0] = np.where(rng.random((8, 8)) < 0.6, 2, 0)
    return g.astype(np.uint8)


def shifted(g, seed=2):
    """a prediction for label g: moved one cell in x, 10 % of the occupied cells with another class"""
    rng = np.random.default_rng(seed)
    p = np.zeros_like(g)
    p[1:] = g[:-1]
    change = (rng.random(g.shape) < 0.1) & (p != 0)
    return np.where(change, p % 8 + 1, p).astype(np.uint8)


def scene_rays():
    """the 24 x 24 camera table, then 8 x 32 lidar-like rays: the 832 rays of the brute-force check"""
    return np.concatenate([camera_rays(X, Y, Z, R), fan_rays((3.5, 5.0, 3.5), 8, 32, 10.0, -30.0)])


def occupied_cell(g):
    """an occupied cell above the ground layer and its free neighbour cells, for the hand-made rays"""
    for x, y, z in np.argwhere(g[:, :, 1:] != 0):
        return int(x), int(y), int(z) + 1
    raise AssertionError('no occupied cell above the ground')


def hand_rays(g):
    """[(name, ray, expected (index, t, face) or None when only the restatement speaks)] on scene g"""
    inf = math.inf
    cx, cy, cz = occupied_cell(g)
    lin = (cx * Y + cy) * Z + cz
    col = np.flatnonzero(g[2, 3, ::-1] != 0)                   # highest occupied z of column (2, 3) seen from above
    top = Z - 1 - int(col[0]) if len(col) else None
    down = ((2 * Y + 3) * Z + top, f32(9.0 - (top + 1)), 2) if top is not None else MISS
    return [
        ('down the column (2, 3), d_x = d_y = 0, from above the grid', [2.5, 3.5, 9.0, 0, 0, -1, inf], down),
        ('axis-parallel outside the grid', [2.5, 10.5, 9.0, 0, 0, -1, inf], MISS),
        ('axis-parallel inside, along +x through the air layer', [0.25, 0.5, 6.5, 1, 0, 0, inf], None),
        ('origin inside an occupied cell', [cx + 0.5, cy + 0.25, cz + 0.75, 0.3, -0.2, 0.1, inf], (lin, f32(0), 3)),
        ('tmax ends before the hit', [2.5, 3.5, 9.0, 0, 0, -1, 9.0 - (top + 1) - 0.5 if top is not None else 1.0], MISS),
        ('all-negative direction', [12.5, 9.5, 6.9, -1.0, -0.7, -0.45, inf], None),
        ('a clean miss', [-3.0, -3.0, 20.0, -1, 0, 0.5, inf], MISS),
        ('NaN direction', [2.5, 3.5, 9.0, math.nan, 0, -1, inf], MISS),
        ('NaN origin', [math.nan, 3.5, 3.5, 1, 0, 0, inf], MISS),
        ('NaN tmax', [2.5, 3.5, 9.0, 0, 0, -1, math.nan], MISS),
        ('zero direction inside an occupied cell', [cx + 0.5, cy + 0.5, cz + 0.5, 0, 0, 0, inf], MISS),
        ('infinite direction component', [2.5, 3.5, 9.0, 0, 0, -inf, inf], MISS),
    ]


CORNER_RAY = [0, 0, 0, 13, 10, 7, math.inf]                     # onto the single cell of corner_scene: t = 12 / 13 through face x


def logits_for(grid, C=9, seed=3):
    """(C, X, Y, Z) float32 whose first maximum over C (strict >) is grid, with exact ties behind the winner on about a third of
    the cells"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, *grid.shape)).astype(f32)
    top = x.max(axis=0) + f32(0.5)
    tie = rng.random(grid.shape) < 0.33
    later = np.minimum(grid.astype(np.int64) + 1 + rng.integers(0, C, grid.shape), C - 1)       # a class after the winner (or itself)
    idx = np.indices(grid.shape)
    x[(later, *idx)] = np.where(tie, top, x[(later, *idx)])
    x[(grid.astype(np.int64), *idx)] = top
    assert np.array_equal(x.argmax(axis=0), grid) and (x == top).sum() > grid.size
    return x
