"""Ego trajectory from consecutive lidar frames: the `_traj` block of the reference's `WorldModelTrainer.visualise`
(trainer.py:808-842).  The reference registers frame t onto frame t - 1 with open3d's point-to-point ICP at threshold 5 m
(compute_pcd_transformation, utils/geometry_utils.py:248-267), chains the poses and draws the label path next to the path of
every prediction row (plot_traj, trainer.py:969-978).  Here the registrations of a whole batch run as one work list on the device
(ops.icp_register -> csrc/icp.hip); the chaining (a handful of 3 x 3 products) and the drawing (a few dozen pixels) run on the
host from the P poses that come back.

Own definitions where the reference delegates to open3d / cv2: the ICP itself (include/muvo_hip.h), the 1-pixel line is
Bresenham's, the disc is dx^2 + dy^2 <= 4 without anti-aliasing, pixels off the canvas are dropped."""
import json
import os

import numpy as np
import torch

TILE, CANVAS, PAD_VALUE = 196, 192, 50
LINE_COLOUR, DISC_COLOUR = (20, 150, 20), (150, 20, 20)


def register_consecutive(range_view, scale, threshold=5.0, queued=False, **kw):
    """range_view (b, s, C, H, W) -> ops.IcpResult over the b (s - 1) pairs (bs, t), t = 1 .. s - 1, in that order: frame t is
    moved onto frame t - 1 of the same tensor, from the identity.  queued: ops.icp_register_queued - the whole budget
    `max_iteration` is queued and the host never waits for the device (the training loop's way); the same result.  Further
    keywords go to the registration: max_iteration, source_stride, search ('brute' or 'grid', ops.icp_register)."""
    from muvo_amd import ops
    b, s, C, H, W = range_view.shape
    frames = range_view.detach().float().contiguous().view(b * s, C, H * W)
    src = [i * s + t for i in range(b) for t in range(1, s)]
    register = ops.icp_register_queued if queued else ops.icp_register
    return register(frames, frames, src, [f - 1 for f in src], scale, threshold, **kw)


def chain(T):
    """T (b, s - 1, 4, 4) float64 numpy -> Rot (b, s, 3, 3), pos (b, s, 3): Rot_t = R Rot_{t-1}, pos_t = pos_{t-1} + Rot_{t-1} t
    (geometry_utils.py:262-265), Rot_0 = identity, pos_0 = 0."""
    b, sm1 = T.shape[:2]
    Rot = np.zeros((b, sm1 + 1, 3, 3))
    pos = np.zeros((b, sm1 + 1, 3))
    Rot[:, 0] = np.eye(3)
    for i in range(b):
        for t in range(1, sm1 + 1):
            R, tr = T[i, t - 1, :3, :3], T[i, t - 1, :3, 3]
            Rot[i, t] = R @ Rot[i, t - 1]
            pos[i, t] = pos[i, t - 1] + Rot[i, t - 1] @ tr
    return Rot, pos


def trajectory(range_view, scale, threshold=5.0, with_result=False, **kw):
    """range_view (b, s, C, H, W) on the device -> Rot (b, s, 3, 3), pos (b, s, 3) float64 numpy (and the IcpResult)."""
    b, s = range_view.shape[:2]
    if s < 2:
        Rot, pos = chain(np.zeros((b, 0, 4, 4)))
        return (Rot, pos, None) if with_result else (Rot, pos)
    res = register_consecutive(range_view, scale, threshold, **kw)
    Rot, pos = chain(res.T.cpu().numpy().reshape(b, s - 1, 4, 4))
    return (Rot, pos, res) if with_result else (Rot, pos)


def _pixel(p):
    return int(96 - 5 * p[1]), int(96 - 5 * p[0])          # (x_pix, y_pix), truncating like the reference's int()


def _line(img, p0, p1):
    x0, y0 = p0
    x1, y1 = p1
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx + dy
    while True:
        if 0 <= x0 < TILE and 0 <= y0 < TILE:
            img[y0, x0] = LINE_COLOUR
        if x0 == x1 and y0 == y1:
            return
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def _disc(img, c):
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            x, y = c[0] + dx, c[1] + dy
            if dx * dx + dy * dy <= 4 and 0 <= x < TILE and 0 <= y < TILE:
                img[y, x] = DISC_COLOUR


def _draw(img, pos, first=0):
    for t in range(first, len(pos)):
        here = _pixel(pos[t])
        _line(img, here, _pixel(pos[t - 1]) if t > 0 else here)
        _disc(img, here)


def render_traj(pos_label, pos_rows):
    """pos_label (b, s, 3), pos_rows: list of (b, s, 3) -> (b, 3, 196, 196 (1 + rows)) uint8: per tile a zero 192 x 192 canvas
    padded by 2 pixels of 50; the label tile holds the label path, every prediction tile starts as the label tile with the origin
    only and then holds its own path (trainer.py:811-838)."""
    pos_label = np.asarray(pos_label, np.float64)
    b = pos_label.shape[0]
    out = np.zeros((b, TILE, TILE * (1 + len(pos_rows)), 3), np.uint8)
    for i in range(b):
        blank = np.full((TILE, TILE, 3), PAD_VALUE, np.uint8)
        blank[2:2 + CANVAS, 2:2 + CANVAS] = 0
        origin = blank.copy()
        _draw(origin, pos_label[i, :1])
        label = origin.copy()
        _draw(label, pos_label[i], first=1)
        out[i, :, :TILE] = label
        for j, rows in enumerate(pos_rows):
            tile = origin.copy()
            _draw(tile, np.asarray(rows, np.float64)[i], first=1)
            out[i, :, TILE * (j + 1):TILE * (j + 2)] = tile
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def prediction_rows(output, output_imagines, key='lidar_reconstruction_1'):
    """the rows of `_pcd_xy`: row i = the reconstruction, then imagination i (one row, the reconstruction, without imaginations)"""
    recon = output[key].detach()
    imagines = list(output_imagines or [])
    if not imagines:
        return [recon]
    return [torch.cat([recon, im[key].detach()], dim=1) for im in imagines]


def batch_trajectories(cfg, batch, output, output_imagines, threshold=5.0, **kw):
    """((Rot, pos) of the label, [(Rot, pos) of every row], IcpResult over all pairs) of one batch: all rows in ONE work list,
    label pairs first, then row by row, each (sample, step) in order"""
    from muvo_amd import ops
    scale = float(cfg.LIDAR_RE.SCALE)
    rows = [batch['range_view_label_1'].float()] + prediction_rows(output, output_imagines)
    b, s = rows[0].shape[:2]
    for r in rows:
        if r.shape[0] != b or r.shape[1] > s or r.shape[1] < 1 or r.shape[3:] != rows[0].shape[3:]:
            raise ValueError(f'trajectory: a prediction row of shape {tuple(r.shape)} for a label of {tuple(rows[0].shape)}')
    C = min(int(r.shape[2]) for r in rows)
    H, W = rows[0].shape[3:]
    # a row may be shorter than the label (no imagined samples in validation / test: the reconstruction covers the first rf
    # steps): its path ends there
    lens = [int(r.shape[1]) for r in rows]
    base = [b * sum(lens[:k]) for k in range(len(rows))]
    frames = torch.cat([r[:, :, :C].reshape(b * r.shape[1], C, H * W) for r in rows], dim=0).contiguous()
    src = [base[k] + i * lens[k] + t for k in range(len(rows)) for i in range(b) for t in range(1, lens[k])]
    if not src:                                             # one-frame sequences: nothing to register
        return chain(np.zeros((b, 0, 4, 4))), [chain(np.zeros((b, 0, 4, 4))) for _ in rows[1:]], None
    res = ops.icp_register(frames, frames, src, [f - 1 for f in src], scale, threshold, **kw)
    T = res.T.cpu().numpy()
    chained, at = [], 0
    for k in range(len(rows)):
        m = b * (lens[k] - 1)
        chained.append(chain(T[at:at + m].reshape(b, lens[k] - 1, 4, 4)))
        at += m
    return chained[0], chained[1:], res


def traj_panel(cfg, batch, output, output_imagines, **kw):
    """the `_traj` panel of one batch as a (b, 3, 196, 196 (1 + rows)) uint8 tensor (host)"""
    (_, pos_label), rows, _ = batch_trajectories(cfg, batch, output, output_imagines, **kw)
    return torch.from_numpy(render_traj(pos_label, [pos for _, pos in rows]))


def _yaw(Rot):
    return np.arctan2(Rot[..., 1, 0], Rot[..., 0, 0])


class EgoMotionMetric:
    """`predict --mode test --ego-motion`: per loader, how far the ego path implied by the predicted lidar (row 0: the
    reconstruction, then imagination 0) drifts from the path implied by the recorded lidar.  `update` is the per-batch hook of
    predict.run; `result()` the content of ego_motion.json."""
    KEYS = ('pos_error_reconstructed', 'pos_error_imagined', 'pos_error_last', 'yaw_error', 'fitness', 'pairs', 'pairs_at_max_iteration',
            'samples')

    def __init__(self, cfg, threshold=5.0, stride=1, max_iteration=2000, search='brute'):
        self.cfg, self.kw = cfg, dict(threshold=threshold, source_stride=stride, max_iteration=max_iteration, search=search)
        self.loader = None
        self.acc = {}

    def start_loader(self, idx):
        self.loader = str(idx)
        self.acc[self.loader] = dict(rec=[], ima=[], last=[], yaw=[], fit=[], pairs=0, hit=0, samples=0)

    def update(self, i, batch, output, output_imagines):
        from muvo_amd import ops
        if self.loader is None:
            self.start_loader(0)
        rf = output['lidar_reconstruction_1'].shape[1]
        (rot_l, pos_l), rows, res = batch_trajectories(self.cfg, batch, output, output_imagines[:1] if output_imagines else [], **self.kw)
        rot_p, pos_p = rows[0]
        if res is None:
            return
        L = pos_p.shape[1]                                   # without imagined samples the row ends after the rf reconstructed steps
        rot_l, pos_l = rot_l[:, :L], pos_l[:, :L]
        err = np.linalg.norm(pos_p - pos_l, axis=-1)                     # (b, L)
        a = self.acc[self.loader]
        a['rec'] += err[:, 1:rf].reshape(-1).tolist()
        a['ima'] += err[:, rf:].reshape(-1).tolist()
        a['last'] += err[:, -1].tolist()
        dyaw = _yaw(rot_p) - _yaw(rot_l)
        a['yaw'] += np.abs(np.arctan2(np.sin(dyaw), np.cos(dyaw)))[:, 1:].reshape(-1).tolist()
        a['fit'] += res.fitness.cpu().tolist()
        a['pairs'] += int(res.status.numel())
        a['hit'] += int((res.status == ops.ICP_MAX_ITERATION).sum())
        a['samples'] += err.shape[0]

    def result(self):
        def mean(v):
            return float(np.mean(v)) if len(v) else 0.0
        return {idx: {'pos_error_reconstructed': mean(a['rec']), 'pos_error_imagined': mean(a['ima']), 'pos_error_last': mean(a['last']),
                      'yaw_error': mean(a['yaw']), 'fitness': mean(a['fit']), 'pairs': a['pairs'],
                      'pairs_at_max_iteration': a['hit'], 'samples': a['samples']} for idx, a in self.acc.items()}

    def write(self, out_dir):
        path = os.path.join(out_dir, 'ego_motion.json')
        with open(path, 'w') as fh:
            json.dump(self.result(), fh, indent=1, sort_keys=True)
            fh.write('\n')
        return path
