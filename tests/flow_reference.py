"""A numpy restatement of the dense optical flow behind the `_flow` panel (include/muvo_hip.h: muvo_flow_*), written from the
definition there and not from the kernels: Farneback's two-frame method (polynomial expansion, SCIA 2003) with the parameters
the reference passes to cv2 (pyramid scale 0.5, 3 levels, window 15, 3 iterations, neighbourhood 5, sigma 1.2, box window),
and the colour coding of trainer.py:1014-1020.  Everything takes a dtype: float64 is the yardstick, float32 (the kernels'
arithmetic, in the definition's summation order) measures how far rounding alone moves a result.

Besides the flow it returns the BRANCH-FRAGILE mask (a displaced sample position came within 1e-3 px of the inside/outside
boundary with a non-zero displacement, spread once by the 15-pixel window and carried to the finer levels)
and, for the colour coding, the QUANTISATION-FRAGILE mask (hue or saturation within 1e-3 of a step; the sextant formula is
integer arithmetic and has no fragile values of its own).

The tables below were measured with this file on a CPU (tests/test_flow_reference.py re-measures and prints them with -s).
Aliasing: textures with frequencies up to 0.25 cycles/px were expected to alias in the coarse levels and lock onto wrong
shifts of about 5 px; with this restatement the example kept in the tests (131 x 150, shift (-4.5, 1.5), fmax 0.25) measured
0.082 px - no lock-on was seen.  Such inputs stay out of the bars all the same."""
import numpy as np

BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
POLY_N, POLY_SIGMA, WINDOW, ITERATIONS, LEVELS, MIN_SIZE = 5, 1.2, 15, 3, 3, 32
PAD, PAD_BYTE = 5, 204
RECOVERY_SIZES = ((70, 93), (131, 150), (150, 131))
RECOVERY_SHIFTS = ((1.3, -0.7), (2.75, 2.2), (-4.5, 1.5), (0.25, 0.0))
GPU_SIZES = ((45, 61), (70, 93), (131, 150), (150, 131))
GPU_SHIFTS = ((1.3, -0.7), (2.75, 2.2), (-4.5, 1.5))
ZOOM = 1.03
# {(h, w): measured worst error (px) of the float64 flow against the true shift, more than 12 px from the border, over
# RECOVERY_SHIFTS on the texture family}; the recovery bar of a size is twice its entry.
RECOVERY_MEASURED = {(45, 61): 0.0832, (70, 93): 0.0674, (131, 150): 0.0753, (150, 131): 0.1513}
# {(h, w): measured worst |float32 restatement - float64 restatement| in px over the cases of gpu_cases(h, w), outside the
# branch-fragile mask}; the kernels' bar is 8 x this (another summation order, fused multiply-adds, libm), floored at 1e-4 px.
F32_DEVIATION = {(45, 61): 6.41e-6, (70, 93): 7.53e-6, (131, 150): 1.33e-5, (150, 131): 1.19e-5}
FRAGILE_BAR = 0.05


def recovery_bar(h, w):
    return 2.0 * RECOVERY_MEASURED[(h, w)]


def kernel_bar(h, w):
    return max(8.0 * F32_DEVIATION[(h, w)], 1e-4)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def texture_fn(seed=0, n=24, fmax=0.08):
    """f(x, y) in [0, 1): 24 sinusoids, frequencies 0.01 .. fmax cycles/px per axis with random sign, amplitudes 0.3 .. 1."""
    rng = np.random.default_rng(seed)
    fx = rng.uniform(0.01, fmax, n) * rng.choice([-1.0, 1.0], n)
    fy = rng.uniform(0.01, fmax, n) * rng.choice([-1.0, 1.0], n)
    amp = rng.uniform(0.3, 1.0, n)
    ph = rng.uniform(0.0, 2 * np.pi, n)

    def f(x, y):
        v = np.zeros(np.broadcast(x, y).shape)
        for i in range(n):
            v = v + amp[i] * np.sin(2 * np.pi * (fx[i] * x + fy[i] * y) + ph[i])
        return 0.5 + 0.5 * v / amp.sum()
    return f


def frame_bytes(f, h, w, warp=None):
    """(h, w) uint8: floor(256 f) at the pixel centres, or at warp(x, y) -> (x', y')"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if warp is not None:
        x, y = warp(x, y)
    return np.clip(np.floor(f(x, y) * 256.0), 0, 255).astype(np.uint8)


def frames_rgb(grey):
    """uint8 (h, w) -> float32 (3, h, w) whose bytes by the rule of image_u8 are `grey` on all channels (so the grey value is
    `grey` again: 4899 + 9617 + 1868 = 16384)"""
    return np.repeat(((grey.astype(np.float32) + 0.5) / 255.0)[None], 3, axis=0).astype(np.float32)


def shift_pair(h, w, shift, seed=0, fmax=0.08):
    """two byte frames; the content of the second is the first moved by `shift` = (dx, dy): frame2(x) = frame1(x - d)"""
    f = texture_fn(seed, fmax=fmax)
    dx, dy = shift
    return frame_bytes(f, h, w), frame_bytes(f, h, w, lambda x, y: (x - dx, y - dy))


def zoom_pair(h, w, zoom=ZOOM, seed=0):
    """frame2(x) = frame1(c + (x - c) / zoom): the true flow at x of frame 1 is (zoom - 1)(x - c)"""
    f = texture_fn(seed)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return frame_bytes(f, h, w), frame_bytes(f, h, w, lambda x, y: (cx + (x - cx) / zoom, cy + (y - cy) / zoom))


def image_u8(x):
    t = x.astype(np.float32) * np.float32(255.0)
    with np.errstate(invalid='ignore'):
        return np.where(~(t > 0), 0, np.where(t >= 255, 255, np.trunc(np.where(np.isfinite(t), t, 0)))).astype(np.uint8)


def grey_of(rgb):
    """float (3, h, w) -> (h, w) int: (4899 R + 9617 G + 1868 B + 8192) >> 14 on the bytes; None: an all-white frame"""
    b = image_u8(rgb).astype(np.int64)
    return (4899 * b[0] + 9617 * b[1] + 1868 * b[2] + 8192) >> 14


# ---- the method ---------------------------------------------------------------------------------------------------------------
def levels(h, w):
    n = LEVELS
    while n > 1 and min(h, w) * 0.5 ** (n - 1) < MIN_SIZE:
        n -= 1
    return n


def level_size(n, k):
    return (n + ((1 << k) >> 1)) >> k            # round(n 0.5^k), halves up


def gauss_taps(sigma, n):
    x = np.arange(n, dtype=np.float64) - n // 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


def _stencil(img, taps, axis, dt):
    """sum_i taps[i] img[.. + i - n // 2 ..] along axis, replicated border, ascending i, every product and sum in dt"""
    n = len(taps)
    r = n // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(img, pad, mode='edge')
    size = img.shape[axis]
    acc = None
    for i in range(n):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(i, i + size)
        term = dt(taps[i]) * p[tuple(sl)]
        acc = term if acc is None else acc + term
    return acc.astype(dt)


def resize(img, ho, wo, dt):
    """bilinear, half-pixel centres, clamped"""
    h, w = img.shape

    def axis(n_in, n_out):
        s = dt(n_in) / dt(n_out)
        c = (np.arange(n_out).astype(dt) + dt(0.5)) * s - dt(0.5)
        c = np.minimum(np.maximum(c, dt(0)), dt(n_in - 1))
        i0 = np.floor(c).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), (c - i0.astype(dt)).astype(dt)
    y0, y1, fy = axis(h, ho)
    x0, x1, fx = axis(w, wo)
    one = dt(1)
    top = (one - fx) * img[y0][:, x0] + fx * img[y0][:, x1]
    bot = (one - fx) * img[y1][:, x0] + fx * img[y1][:, x1]
    return ((one - fy)[:, None] * top + fy[:, None] * bot).astype(dt)


def pyramid_level(grey, k, dt):
    g = grey.astype(dt)
    if k == 0:
        return g
    sigma = (2.0 ** k - 1.0) / 2.0
    n = max(int(np.floor(5.0 * sigma + 0.5)) | 1, 3)
    taps = gauss_taps(sigma, n)
    g = _stencil(_stencil(g, taps, 1, dt), taps, 0, dt)           # along x, then along y
    return resize(g, level_size(grey.shape[0], k), level_size(grey.shape[1], k), dt)


def poly_constants():
    """(taps g, x g, x^2 g; kb, ka0, ka1, ka2, kxy) in float64: rows of the inverse of the constant 6 x 6 normal matrix over the
    basis 1, x, y, x^2, y^2, xy, so that b = kb m10, A_xx = ka0 m00 + ka1 m20 + ka2 m02, A_xy = kxy m11 (half the xy coefficient)"""
    n = 2 * POLY_N + 1
    g = gauss_taps(POLY_SIGMA, n)
    x = np.arange(n, dtype=np.float64) - POLY_N
    X, Y = np.meshgrid(x, x)
    W = np.outer(g, g)
    phi = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y])
    G = np.einsum('iyx,jyx,yx->ij', phi, phi, W)
    ig = np.linalg.inv(G)
    return (g, g * x, g * x * x), (ig[1, 1], ig[3, 0], ig[3, 3], ig[3, 4], ig[5, 5] / 2.0)


def poly_expansion(img, dt):
    """(5, h, w): b_x, b_y, A_xx, A_yy, A_xy; vertical moments first, then horizontal"""
    (t0, t1, t2), (kb, ka0, ka1, ka2, kxy) = poly_constants()
    v0, v1, v2 = (_stencil(img, t, 0, dt) for t in (t0, t1, t2))
    m00, m10, m20 = (_stencil(v0, t, 1, dt) for t in (t0, t1, t2))
    m01, m11 = _stencil(v1, t0, 1, dt), _stencil(v1, t1, 1, dt)
    m02 = _stencil(v2, t0, 1, dt)
    kb, ka0, ka1, ka2, kxy = (dt(v) for v in (kb, ka0, ka1, ka2, kxy))
    return np.stack([kb * m10, kb * m01, ka0 * m00 + ka1 * m20 + ka2 * m02, ka0 * m00 + ka2 * m20 + ka1 * m02, kxy * m11]).astype(dt)


def border_scale(n, dt, on=True):
    s = np.ones(n, dtype=dt)
    if on:
        for i in range(n):
            k = min(i, n - 1 - i)
            if k < len(BORDER):
                s[i] = dt(BORDER[k])
    return s


def _dilate(mask, r):
    h, w = mask.shape
    p = np.pad(mask, r, mode='constant')
    out = np.zeros_like(mask)
    rows = np.zeros((h + 2 * r, w), dtype=bool)
    for i in range(2 * r + 1):
        rows |= p[:, i:i + w]
    for i in range(2 * r + 1):
        out |= rows[i:i + h]
    return out


def iteration(R0, R1, d, dt, sign_db=1.0, box=WINDOW, border=True, eps=1e-3):
    """one iteration: (new flow (2, h, w), pixels whose sample position lies within eps of the inside / outside boundary)"""
    _, h, w = R0.shape
    y, x = np.mgrid[0:h, 0:w]
    fx, fy = x.astype(dt) + d[0], y.astype(dt) + d[1]
    inside = (fx >= 0) & (fx < w - 1) & (fy >= 0) & (fy < h - 1)
    near = ((np.abs(fx) < eps) | (np.abs(fx - (w - 1)) < eps) | (np.abs(fy) < eps) | (np.abs(fy - (h - 1)) < eps)) & ((d[0] != 0) | (d[1] != 0))
    x1 = np.where(inside, np.floor(fx), 0).astype(np.int64)
    y1 = np.where(inside, np.floor(fy), 0).astype(np.int64)
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)
    a, b = (fx - x1.astype(dt)).astype(dt), (fy - y1.astype(dt)).astype(dt)
    one = dt(1)
    w00, w01, w10, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    S = (w00 * R1[:, y1, x1] + w01 * R1[:, y1, x2] + w10 * R1[:, y2, x1] + w11 * R1[:, y2, x2]).astype(dt)
    half = dt(0.5)
    axx = np.where(inside, (R0[2] + S[2]) * half, R0[2])
    ayy = np.where(inside, (R0[3] + S[3]) * half, R0[3])
    axy = np.where(inside, (R0[4] + S[4]) * half, R0[4])
    dbx = np.where(inside, dt(sign_db) * (R0[0] - S[0]) * half, dt(0))
    dby = np.where(inside, dt(sign_db) * (R0[1] - S[1]) * half, dt(0))
    bx = dbx + (axx * d[0] + axy * d[1])
    by = dby + (axy * d[0] + ayy * d[1])
    s = (border_scale(h, dt, border)[:, None] * border_scale(w, dt, border)[None, :]).astype(dt)
    axx, ayy, axy, bx, by = axx * s, ayy * s, axy * s, bx * s, by * s
    M = [axx * axx + axy * axy, axy * (axx + ayy), ayy * ayy + axy * axy, axx * bx + axy * by, axy * bx + ayy * by]
    ones = np.ones(box)
    inv = dt(1.0 / (box * box))
    g11, g12, g22, h1, h2 = ((_stencil(_stencil(m.astype(dt), ones, 0, dt), ones, 1, dt) * inv).astype(dt) for m in M)
    idet = one / (g11 * g22 - g12 * g12 + dt(1e-3))
    return np.stack([(g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet]).astype(dt), near


def farneback(grey0, grey1, dtype=np.float64, with_mask=False, with_levels=False, sign_db=1.0, level_mult=2.0, box=WINDOW, border=True):
    """grey0, grey1 (h, w) integer grey images -> flow (2, h, w) [dx, dy] in `dtype`: frame1(x + d) ~ frame0(x)"""
    dt = np.dtype(dtype).type
    h, w = grey0.shape
    assert grey1.shape == (h, w) and h >= 16 and w >= 16
    n = levels(h, w)
    d, mask = None, None
    for k in range(n - 1, -1, -1):
        I0, I1 = pyramid_level(grey0, k, dt), pyramid_level(grey1, k, dt)
        hk, wk = I0.shape
        if d is None:
            d, mask = np.zeros((2, hk, wk), dtype=dt), np.zeros((hk, wk), dtype=bool)
        else:
            d = np.stack([resize(d[0], hk, wk, dt), resize(d[1], hk, wk, dt)]) * dt(level_mult)
            mask = resize(mask.astype(np.float64), hk, wk, np.float64) > 0
        R0, R1 = poly_expansion(I0, dt), poly_expansion(I1, dt)
        for _ in range(ITERATIONS):
            d, near = iteration(R0, R1, d, dt, sign_db, box, border)
            mask = mask | _dilate(near, WINDOW // 2)
    out = (d,)
    if with_mask:
        out += (mask,)
    if with_levels:
        out += (n,)
    return out if len(out) > 1 else d


# ---- colour coding --------------------------------------------------------------------------------------------------------------
def _sextant(hue, sat):
    """8-bit HSV -> RGB with value 255, hue in units of 2 degrees (0 .. 179), in integers, rounded to nearest"""
    hue, sat = hue.astype(np.int64), sat.astype(np.int64)
    i, r = hue // 30, hue % 30
    v = np.full_like(hue, 255)
    p = 255 - sat
    q = 255 - (2 * sat * r + 30) // 60
    t = 255 - (2 * sat * (30 - r) + 30) // 60
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros((3,) + hue.shape, dtype=np.uint8)
    for k, rgb in enumerate(table):
        for c in range(3):
            out[c] = np.where(i == k, rgb[c], out[c])
    return out


def colour(flow, dtype=np.float64, with_mask=False, truncate_hue=True, eps=1e-3, flow_tol=0.0):
    """flow (2, h, w) -> (3, h, w) uint8 (and the quantisation-fragile mask: hue or saturation before truncation within eps of
    a step.  flow_tol: the field itself is only known to that many px per component - a hue then moves by up to
    flow_tol sqrt(2) / mag rad and a saturation, through the magnitude and the pair's min and max, by up to
    3 sqrt(2) flow_tol 255 / (max - min): both are added to eps)"""
    dt = np.dtype(dtype).type
    dx, dy = flow[0].astype(dt), flow[1].astype(dt)
    mag = np.sqrt(dx * dx + dy * dy).astype(dt)
    ang = (np.arctan2(dy, dx) * dt(180.0 / np.pi)).astype(dt)
    ang = np.where(ang < 0, ang + dt(360), ang)
    hq = ang * dt(0.5)
    hue = np.minimum(np.trunc(hq) if truncate_hue else np.floor(hq + dt(0.5)), 179)
    mn, mx = mag.min(), mag.max()
    sq = (mag - mn) * dt(255) / (mx - mn) if mx > mn else np.zeros_like(mag)
    sat = np.minimum(np.trunc(sq), 255)
    rgb = _sextant(hue, sat)
    if not with_mask:
        return rgb
    if not mx > mn:
        return rgb, np.zeros(mag.shape, dtype=bool), hue.astype(np.int64), sat.astype(np.int64)
    tol = np.sqrt(2.0) * flow_tol
    eps_h = eps + tol / np.maximum(mag, 1e-12) * (90.0 / np.pi)
    eps_s = eps + 3.0 * tol * 255.0 / float(mx - mn)
    fragile = (np.abs(hq - np.round(hq)) < eps_h) | (np.abs(sq - np.round(sq)) < eps_s)
    if flow_tol:
        fragile |= hq > 180.0 - eps_h                       # the angle may wrap
    return rgb, fragile, hue.astype(np.int64), sat.astype(np.int64)


def hue_step_effect(hue, sat):
    """per byte, the largest change a step of one in hue or in saturation (either direction) makes: the allowance inside the
    quantisation-fragile mask"""
    base = _sextant(hue, sat).astype(np.int64)
    worst = np.zeros_like(base)
    for dh, ds in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        other = _sextant((hue + dh) % 180, np.clip(sat + ds, 0, 255)).astype(np.int64)
        worst = np.maximum(worst, np.abs(other - base))
    return worst


def tile(flow, dtype=np.float64):
    """the padded tile of the panel: (3, h + 10, w + 10) uint8"""
    rgb = colour(flow, dtype)
    return np.pad(rgb, ((0, 0), (PAD, PAD), (PAD, PAD)), mode='constant', constant_values=PAD_BYTE)


# ---- the panel, after trainer.py:729-750 ----------------------------------------------------------------------------------------
def panel(label, rows, rf, tile_fn):
    """label (b, s, 3, h, w), rows: list of (b, L, 3, h, w) float arrays whose blank frames are all ones (L = s, or rf without
    imagined samples) -> (b, 3, (1 + rows)(h + 10), (s - 1)(w + 10)) uint8; tile_fn(img1, img2) -> (3, h + 10, w + 10).
    Tiles a short row does not reach stay 255."""
    b, s, _, h, w = label.shape
    out = np.full((b, 3, (1 + len(rows)) * (h + 2 * PAD), (s - 1) * (w + 2 * PAD)), 255, np.uint8)
    for bs in range(b):
        for step in range(1, s):
            col = [tile_fn(label[bs, step - 1], label[bs, step])]
            for i, row in enumerate(rows):
                if step >= row.shape[1]:
                    col.append(None)
                    continue
                img1 = row[bs, step - 1]
                if i == rf:
                    img1 = rows[0][bs, step - 1]
                col.append(tile_fn(img1, row[bs, step]))
            for r, t in enumerate(col):
                if t is not None:
                    out[bs, :, r * (h + 2 * PAD):(r + 1) * (h + 2 * PAD), (step - 1) * (w + 2 * PAD):step * (w + 2 * PAD)] = t
    return out


def flow_tile_fn(dtype=np.float64):
    return lambda a, b: tile(farneback(grey_of(a), grey_of(b), dtype), dtype)


# ---- the cases of the kernel tests and what a candidate must meet -------------------------------------------------------------
# (-4.5, 1.5) flags 5.7 % of (45, 61) and 11.3 % of (70, 93) branch-fragile - border pixels whose flow points out of the image
# settle ON the inside / outside boundary, and one such pixel spreads over 225 - so these two sizes take (-4.4, 1.5), for which
# nothing is flagged.  The zoom flags 3 - 7 % when the second frame is the magnified one (all border flow points outward);
# the cases magnify the FIRST frame, flow in every direction pointing inward, nothing flagged.
GPU_SHIFTS_AT = {(45, 61): ((1.3, -0.7), (2.75, 2.2), (-4.4, 1.5)), (70, 93): ((1.3, -0.7), (2.75, 2.2), (-4.4, 1.5)),
                 (131, 150): GPU_SHIFTS, (150, 131): GPU_SHIFTS}
MAX_BRANCH_FRAGILE, MAX_QUANT_FRAGILE = 0.02, 0.05


def gpu_cases(h, w):
    """[(name, grey0, grey1)] of one size: the three shifts and the 1.03 x zoom about the centre"""
    out = [(f'shift{s}', *shift_pair(h, w, s)) for s in GPU_SHIFTS_AT[(h, w)]]
    z0, z1 = zoom_pair(h, w)
    return out + [('zoom', z1, z0)]


_CACHE = {}


def reference_flow(h, w, name):
    """(flow float64, branch-fragile mask, flow of the float32 restatement) of a case, computed once"""
    key = (h, w, name)
    if key not in _CACHE:
        g0, g1 = next((a, b) for n, a, b in gpu_cases(h, w) if n == name)
        d, m = farneback(g0, g1, np.float64, with_mask=True)
        _CACHE[key] = (d, m, farneback(g0, g1, np.float32))
    return _CACHE[key]


def flow_deviation(cand, ref, mask):
    """(worst |cand - ref| outside the mask, worst inside it) in px, per component"""
    e = np.abs(np.asarray(cand, np.float64) - ref).max(axis=0)
    return (float(e[~mask].max()) if (~mask).any() else 0.0), (float(e[mask].max()) if mask.any() else 0.0)


def flow_accepted(cand, ref, mask, h, w):
    free, fragile = flow_deviation(cand, ref, mask)
    return free <= kernel_bar(h, w) and fragile <= FRAGILE_BAR


def zoom_field(h, w, zoom=ZOOM):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([(zoom - 1) * (x - (w - 1) / 2.0), (zoom - 1) * (y - (h - 1) / 2.0)]).astype(np.float32)


def rotation_field(h, w, omega=0.02, centre=(0.31, 0.64)):
    """rotation by omega rad about the off-centre point (centre[0] w, centre[1] h)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = centre[0] * w, centre[1] * h
    return np.stack([-omega * (y - cy), omega * (x - cx)]).astype(np.float32)


def colour_accepted(cand, flow, flow_tol=0.0, skip=None):
    """cand (3, h, w) uint8 against the float64 colour coding of the field `flow`: equal outside the quantisation-fragile mask,
    within one hue / saturation step's effect inside it; pixels of `skip` (the branch-fragile mask of a computed flow) are not
    compared.  Returns (ok, share flagged, bytes that differ)"""
    ref, fragile, hue, sat = colour(flow, np.float64, with_mask=True, flow_tol=flow_tol)
    diff = np.abs(cand.astype(np.int64) - ref.astype(np.int64))
    if skip is not None:
        diff = np.where(skip[None], 0, diff)
    ok = not diff[:, ~fragile].any() and bool((diff <= hue_step_effect(hue, sat))[:, fragile].all())
    return ok, float(fragile.mean()), int((diff > 0).sum())
