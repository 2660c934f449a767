"""The voxel head in 3-D: the `_voxel` panel and the RayIoU metric, both on one primitive - the first-hit ray march through a class
grid of csrc/raycast.hip (include/muvo_hip.h: muvo_raycast), straight from the model's logits: the logits become a uint8 class
grid plus occupancy bricks on the device and no voxel tensor crosses to the host.

Panel `_voxel` stands where the reference draws matplotlib figures (trainer.py:923-966: `ax.voxels`, `view_init(elev=60,
azim=165)`).  OUR DEFINITION: an orthographic view from that elevation and azimuth, one ray per pixel; voxels stay cubic
(matplotlib stretches the axes to its 4:4:3 box); a face is shaded by the axis it faces and by its height (the reference's
`shade=False` with a two-entry palette is a flat silhouette).  (b, 3, (1 + rows)(R + 4), s (R + 4) [+ sep]) uint8, a strip laid
out exactly like `_voxel_top`: row 0 `voxel_label_1[:, :, 0]`, then one row per imagined sample (row 0: reconstruction then
imagination 0; row i > 0: blank then imagination i), pad 2 of 204, blank = class 0, sep = int((R + 4) / 4) of 255 before step rf,
VOXEL_COLOURS through palette256.

RayIoU after Liu et al., "Fully Sparse 3D Occupancy Prediction" (ECCV 2024): lidar-like rays through label and prediction, a ray
is a true positive of its class when both first hits have that class and their depths differ by at most 1 / 2 / 4 m.  Different
from the paper: ONE origin, the lidar's own (the paper adds origins along the ego path); the rays are the pixel centres of the
dataset's range view (every `stride`-th azimuth), not a fixed 32-beam pattern; depth is the entry into the first occupied cell,
along the unit direction, times VOXEL.RESOLUTION."""
import json
import math
import os

import numpy as np
import torch

ELEV, AZIM = 60.0, 165.0                    # view_init of the reference's figures
PAD, PAD_BYTE = 2, 204
THRESHOLDS = (1.0, 2.0, 4.0)                # metres


def camera_rays(X, Y, Z, R):
    """(R * R, 7) float32 numpy: the orthographic ray table of the panel, computed in float64.  back = (cos e cos a, cos e sin a,
    sin e), right = (-sin a, cos a, 0), up = back x right; half = |(X, Y, Z)| / 2; pixel (i, j) starts at centre + 2 half back +
    u right + v up with u = ((j + 1/2) / R 2 - 1) half, v = (1 - (i + 1/2) / R 2) half, looks along -back, tmax = 4 half."""
    e, a = math.radians(ELEV), math.radians(AZIM)
    back = np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)])
    right = np.array([-math.sin(a), math.cos(a), 0.0])
    up = np.cross(back, right)
    size = np.array([X, Y, Z], np.float64)
    half = 0.5 * float(np.sqrt((size * size).sum()))
    centre = size / 2
    k = (np.arange(R, dtype=np.float64) + 0.5) / R * 2
    u, v = (k - 1) * half, (1 - k) * half
    origin = centre + 2 * half * back + u[None, :, None] * right + v[:, None, None] * up
    rays = np.empty((R, R, 7), np.float64)
    rays[..., :3] = origin
    rays[..., 3:6] = -back
    rays[..., 6] = 4 * half
    return rays.reshape(R * R, 7).astype(np.float32)


def lidar_rays(cfg, stride=4):
    """(H * ceil(W / stride), 7) float32 numpy: one unit direction per pixel centre (r, c) of the dataset's range view, c = 0,
    stride, ...: yaw = pi (1 - 2 (c + 1/2) / W), pitch linear from fov-up to fov-down at (r + 1/2) / H, direction (cos p cos y,
    cos p sin y, sin p) in grid axes; one origin, the lidar: VOXEL.EV_POSITION + (px, -py, pz) / VOXEL.RESOLUTION of
    POINTS.LIDAR_POSITION (the convention of input_pipeline.voxelize_geometry); tmax = +inf."""
    if stride < 1:
        raise ValueError(f'lidar_rays: stride {stride} below 1')
    H, W = int(cfg.POINTS.CHANNELS), int(cfg.POINTS.HORIZON_RESOLUTION)
    down, top = (math.radians(float(v)) for v in cfg.POINTS.FOV)
    px, py, pz = (float(v) for v in cfg.POINTS.LIDAR_POSITION)
    res = float(cfg.VOXEL.RESOLUTION)
    origin = np.array([float(v) for v in cfg.VOXEL.EV_POSITION]) + np.array([px, -py, pz]) / res
    cols = np.arange(0, W, stride, dtype=np.float64)
    yaw = math.pi * (1 - 2 * (cols + 0.5) / W)
    pitch = top + (down - top) * (np.arange(H, dtype=np.float64) + 0.5) / H
    rays = np.empty((H, len(cols), 7), np.float64)
    rays[..., :3] = origin
    rays[..., 3] = np.cos(pitch)[:, None] * np.cos(yaw)[None]
    rays[..., 4] = np.cos(pitch)[:, None] * np.sin(yaw)[None]
    rays[..., 5] = np.sin(pitch)[:, None]
    rays[..., 6] = np.inf
    return rays.reshape(-1, 7).astype(np.float32)


def valid_rays(rays, X, Y, Z):
    """(R,) bool numpy: the rays (R, 7) float32 that the march of include/muvo_hip.h (muvo_raycast) does not call a miss before its
    step 2 on a grid (X, Y, Z) - step 1, the slabs, in float32 and in its order.  The rendered depth loss averages over these."""
    rays = np.asarray(rays, np.float32)
    f32 = np.float32
    with np.errstate(all='ignore'):
        t0, t1 = np.zeros(len(rays), f32), rays[:, 6].copy()
        ok, moving = np.ones(len(rays), bool), np.zeros(len(rays), bool)
        for a, N in enumerate((X, Y, Z)):
            o, d = rays[:, a], rays[:, 3 + a]
            move = d != 0
            inv = f32(1) / np.where(move, d, f32(1))
            ta, tb = (f32(0) - o) * inv, (f32(N) - o) * inv
            asc = ta <= tb
            lo, hi = np.where(asc, ta, tb), np.where(asc, tb, ta)
            ok &= np.where(move, lo <= hi, (f32(0) <= o) & (o < f32(N)))
            t0 = np.where(move & (lo > t0), lo, t0)
            t1 = np.where(move & (hi < t1), hi, t1)
            moving |= move
        return ok & moving & (t0 < t1)


_RENDER_TABLES = {}


def render_table(cfg, factor, stride, shape, device):
    """(rays (R, 7) float32 on the device, the number of valid rays) of the rendered depth loss at output scale `factor`:
    lidar_rays(cfg, stride) with the origin divided by the factor - the grid of scale f has cells f times as large - and the
    directions as they are.  Cached per (geometry, factor, stride, grid size, device); the valid rays are counted once, here."""
    key = (tuple(float(v) for v in cfg.VOXEL.EV_POSITION), tuple(float(v) for v in cfg.POINTS.LIDAR_POSITION), tuple(float(v) for v in cfg.POINTS.FOV),
           int(cfg.POINTS.CHANNELS), int(cfg.POINTS.HORIZON_RESOLUTION), float(cfg.VOXEL.RESOLUTION), int(factor), int(stride),
           tuple(int(n) for n in shape), str(device))
    if key not in _RENDER_TABLES:
        rays = lidar_rays(cfg, stride)
        rays[:, :3] = (rays[:, :3].astype(np.float64) / factor).astype(np.float32)
        _RENDER_TABLES[key] = (torch.from_numpy(rays).to(device), int(valid_rays(rays, *shape).sum()))
    return _RENDER_TABLES[key]


def camera_label_rays(cfg, stride=2):
    """(ceil(H / stride) * ceil(W / stride), 7) float32 numpy, computed in float64: one ray per `stride`-th pixel (r, c), r = 0,
    stride, ..., c = 0, stride, ..., row-major, of the full IMAGE.SIZE = (H, W) frame at IMAGE.FOV - the depth camera the voxel
    labels come from.  Unit direction through the point csrc/voxelize.hip unprojects that pixel to: it takes the pixel's integer
    coordinates (c, r) - the pixel's CORNER, not its centre - against the principal point (W / 2, H / 2), x = (c - W / 2) depth /
    f, y = (r - H / 2) depth / f, f = W / (2 tan(FOV / 2)), and puts the point at (depth, -x, -y) from the camera in grid axes:
    direction (1, -(c - W / 2) / f, -(r - H / 2) / f) normalised.  One origin, the camera: VOXEL.EV_POSITION + (forward, -right,
    up) / VOXEL.RESOLUTION of IMAGE.CAMERA_POSITION (the convention of input_pipeline.voxelize_geometry); tmax = +inf."""
    if isinstance(stride, bool) or int(stride) != stride or stride < 1:
        raise ValueError(f'camera_label_rays: stride {stride} below 1')
    H, W = (int(v) for v in cfg.IMAGE.SIZE)
    f = W / (2.0 * math.tan(float(cfg.IMAGE.FOV) * math.pi / 360.0))
    forward, right, up = (float(v) for v in cfg.IMAGE.CAMERA_POSITION)
    res = float(cfg.VOXEL.RESOLUTION)
    origin = np.array([float(v) for v in cfg.VOXEL.EV_POSITION]) + np.array([forward, -right, up]) / res
    rows, cols = np.arange(0, H, stride, dtype=np.float64), np.arange(0, W, stride, dtype=np.float64)
    d = np.empty((len(rows), len(cols), 3), np.float64)
    d[..., 0] = 1.0
    d[..., 1] = -(cols[None, :] - W / 2.0) / f
    d[..., 2] = -(rows[:, None] - H / 2.0) / f
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    rays = np.empty((len(rows), len(cols), 7), np.float64)
    rays[..., :3] = origin
    rays[..., 3:6] = d
    rays[..., 6] = np.inf
    return rays.reshape(-1, 7).astype(np.float32)


_VISIBILITY_TABLES = {}


def visibility_table(cfg, factor, shape, device):
    """rays (R, 7) float32 on the device of the visibility mask at label scale `factor`: the rows of
    lidar_rays(cfg, LIDAR_STRIDE) followed by those of camera_label_rays(cfg, CAMERA_STRIDE) of VOXEL_SEG.VISIBILITY, origins
    divided by the factor - the grid of scale f has cells f times as large - directions as they are.  Cached per (geometry,
    factor, strides, grid size, device)."""
    from muvo_amd.config import voxel_visibility
    _, lidar_stride, camera_stride = voxel_visibility(cfg)
    key = (tuple(float(v) for v in cfg.VOXEL.EV_POSITION), tuple(float(v) for v in cfg.POINTS.LIDAR_POSITION), tuple(float(v) for v in cfg.POINTS.FOV),
           int(cfg.POINTS.CHANNELS), int(cfg.POINTS.HORIZON_RESOLUTION), float(cfg.VOXEL.RESOLUTION),
           tuple(int(v) for v in cfg.IMAGE.SIZE), float(cfg.IMAGE.FOV), tuple(float(v) for v in cfg.IMAGE.CAMERA_POSITION),
           int(factor), lidar_stride, camera_stride, tuple(int(n) for n in shape), str(device))
    if key not in _VISIBILITY_TABLES:
        rays = np.concatenate([lidar_rays(cfg, lidar_stride), camera_label_rays(cfg, camera_stride)])
        rays[:, :3] = (rays[:, :3].astype(np.float64) / factor).astype(np.float32)
        _VISIBILITY_TABLES[key] = torch.from_numpy(rays).to(device)
    return _VISIBILITY_TABLES[key]


_CAMERAS = {}


def _camera(X, Y, Z, R, device):
    """the ray table of the panel on the device, cached per (X, Y, Z, R)"""
    key = (X, Y, Z, R, str(device))
    if key not in _CAMERAS:
        _CAMERAS[key] = torch.from_numpy(camera_rays(X, Y, Z, R)).to(device)
    return _CAMERAS[key]


def _frames(x):
    return x.reshape(x.shape[0] * x.shape[1], *x.shape[2:])


def _label_grid(batch):
    label = batch['voxel_label_1']
    label = label[:, :, 0] if label.dim() == 6 else label
    return _frames(label.to(torch.uint8))


def voxel_panel(cfg, batch, output, output_imagines, size=256):
    """the `_voxel` panel of one batch as a (b, 3, (1 + rows)(R + 4), s (R + 4) [+ sep]) uint8 device tensor, R = size"""
    from muvo_amd import ops
    from muvo_amd.visualise import VOXEL_COLOURS, _Strip, _lengths, _palette, _prediction_rows, _rows
    R = int(size)
    if R < 1:
        raise ValueError(f'voxel_panel: size {size} below 1')
    imagines = list(output_imagines or [])
    pred = output['voxel_1'].detach().float()
    b, rf, _, X, Y, Z = pred.shape
    s = batch['voxel_label_1'].shape[1]
    fh = _lengths(s, rf, imagines, 'voxel_1', '_voxel')
    pal, blank0 = _palette(VOXEL_COLOURS, pred.device)
    rays = _camera(X, Y, Z, R, pred.device)
    T = R + 2 * PAD
    st = _Strip(b, [T] * (1 + _rows(imagines)), T, s, rf, int(T / 4), pred.device)

    def view(src, place):
        ops.panel_voxel_view(*ops.raycast_bricks(src), rays, pal, st.panel, place, PAD, PAD_BYTE)
    view(_label_grid(batch), st.place(0, s))
    _prediction_rows(
        imagines,
        lambda row: view(_frames(pred), st.place(row, rf)),
        lambda row, im: view(_frames(im['voxel_1'].detach().float()), st.place(row, fh, rf)),
        lambda row: ops.panel_fill(b * rf, R, R, blank0, st.panel, st.place(row, rf), PAD, PAD_BYTE))
    return st.panel


def ray_iou_from_counts(counts):
    """counts (3, C, 3) integers (threshold x class x tp / fp / fn) -> (the three RayIoU: per threshold the mean over the classes
    1 .. C - 1 with tp + fp + fn > 0 of tp / (tp + fp + fn), 0.0 without such a class; per-class IoU (3, C) with None where absent)"""
    means, per_class = [], []
    for row in counts:
        ious = [(int(tp) / (int(tp) + int(fp) + int(fn)) if int(tp) + int(fp) + int(fn) > 0 else None) for tp, fp, fn in row]
        present = [v for v in ious[1:] if v is not None]
        means.append(sum(present) / len(present) if present else 0.0)
        per_class.append(ious)
    return means, per_class


class RayIoUMetric:
    """`predict --mode test --ray-iou`: per loader the RayIoU of the reconstructed frames and, apart from them, of the frames of the
    first imagined sample against `voxel_label_1`.  `update` is the per-batch hook of predict.run and only queues kernels (integer
    counts and fp64 sums stay on the device); `result()` reads them once per loader."""

    def __init__(self, cfg, prefix='test', stride=4):
        self.cfg, self.prefix, self.stride = cfg, prefix, int(stride)
        self.loader = None
        self.acc = {}
        self._rays = {}

    def start_loader(self, idx):
        self.loader = str(idx)
        self.acc[self.loader] = dict(counts=None, depth=None)

    def _add(self, a, which, label, pred):
        from muvo_amd import ops
        if not pred.shape[0]:
            return
        C = pred.shape[1]
        if str(pred.device) not in self._rays:
            self._rays[str(pred.device)] = torch.from_numpy(lidar_rays(self.cfg, self.stride)).to(pred.device)
        rays = self._rays[str(pred.device)]
        if a['counts'] is None:
            a['counts'] = torch.zeros((2, 3, C, 3), dtype=torch.int64, device=pred.device)
            a['depth'] = torch.zeros((2, 2), dtype=torch.float64, device=pred.device)
        ops.ray_iou_counts(*ops.raycast_bricks(label), *ops.raycast_bricks(pred), rays, C, float(self.cfg.VOXEL.RESOLUTION), a['counts'][which],
                           a['depth'][which], THRESHOLDS)

    def update(self, i, batch, output, output_imagines):
        if self.loader is None:
            self.start_loader(0)
        a = self.acc[self.loader]
        pred = output['voxel_1'].detach().float()
        b, rf = pred.shape[:2]
        label = batch['voxel_label_1']
        label = (label[:, :, 0] if label.dim() == 6 else label).to(torch.uint8)
        with torch.no_grad():
            self._add(a, 0, _frames(label[:, :rf].contiguous()), _frames(pred))
            if output_imagines:
                im = output_imagines[0]['voxel_1'].detach().float()
                self._add(a, 1, _frames(label[:, rf:rf + im.shape[1]].contiguous()), _frames(im))

    @staticmethod
    def summarise(counts, depth):
        """counts (2, 3, C, 3), depth (2, 2) as nested lists -> the figures of one loader without its prefix"""
        out = {}
        for which, tail in ((0, ''), (1, '_imagine')):
            means, per_class = ray_iou_from_counts(counts[which])
            for thr, m in zip(THRESHOLDS, means):
                out[f'ray_iou_{int(thr)}m{tail}'] = m
            out[f'ray_iou{tail}'] = sum(means) / len(means)
            out[f'ray_iou_per_class{tail}'] = per_class
            s, n = depth[which]
            out[f'ray_depth_l1{tail}'] = s / n if n else 0.0
            out[f'ray_pairs{tail}'] = int(n)
        return out

    def result(self):
        out = {}
        for idx, a in self.acc.items():
            if a['counts'] is None:
                counts, depth = [[[[0, 0, 0]]] * 3] * 2, [[0.0, 0.0]] * 2
            else:
                counts, depth = a['counts'].cpu().tolist(), a['depth'].cpu().tolist()
            out.update({f'{self.prefix}{idx}_{k}': v for k, v in self.summarise(counts, depth).items()})
        return out

    def write(self, out_dir):
        path = os.path.join(out_dir, 'ray_iou.json')
        with open(path, 'w') as fh:
            json.dump(self.result(), fh, indent=1, sort_keys=True)
            fh.write('\n')
        return path


def cd_thresholds2(resolution, thresholds=THRESHOLDS):
    """RayIoU's thresholds in metres as squared distances in cells: floor((thr / resolution)^2 + 1e-9) - 25, 100, 400 at 0.2 m"""
    return [int(math.floor((t / resolution) ** 2 + 1e-9)) for t in thresholds]


class VoxelDistanceMetric:
    """`predict --mode test --voxel-cd`: per loader the Chamfer distance and the F-scores at 1 / 2 / 4 m between the occupied cells
    of `voxel_label_1` (unmasked) and of the prediction's class grid, from the untruncated distance transforms of both grids
     - the reconstructed frames and, apart from them, the frames of the first imagined sample.  `update` is the
    per-batch hook of predict.run and only queues kernels (integer counts and fp64 sums stay on the device); `result()` reads them
    once per loader."""

    def __init__(self, cfg, prefix='test'):
        self.cfg, self.prefix = cfg, prefix
        self.thresholds2 = cd_thresholds2(float(cfg.VOXEL.RESOLUTION))
        self.loader = None
        self.acc = {}

    def start_loader(self, idx):
        self.loader = str(idx)
        self.acc[self.loader] = dict(counts=None, sums=None)

    def _add(self, a, which, label, pred):
        from muvo_amd import ops
        if not pred.shape[0]:
            return
        if a['counts'] is None:
            a['counts'] = torch.zeros((2, 10), dtype=torch.int64, device=pred.device)
            a['sums'] = torch.zeros((2, 2), dtype=torch.float64, device=pred.device)
        ops.voxel_cd_counts(label, ops.raycast_bricks(pred)[0], self.thresholds2, a['counts'][which], a['sums'][which])

    def update(self, i, batch, output, output_imagines):
        if self.loader is None:
            self.start_loader(0)
        a = self.acc[self.loader]
        pred = output['voxel_1'].detach().float()
        b, rf = pred.shape[:2]
        label = batch['voxel_label_1']
        label = (label[:, :, 0] if label.dim() == 6 else label).to(torch.uint8)
        with torch.no_grad():
            self._add(a, 0, _frames(label[:, :rf].contiguous()), _frames(pred))
            if output_imagines:
                im = output_imagines[0]['voxel_1'].detach().float()
                self._add(a, 1, _frames(label[:, rf:rf + im.shape[1]].contiguous()), _frames(im))

    @staticmethod
    def summarise(counts, sums, resolution):
        """counts (2, 10) - frames, skipped, n_P, n_G, hits_P[3], hits_G[3] - and sums (2, 2) - sum_PG, sum_GP - as nested lists ->
        the figures of one loader without its prefix; a figure whose denominator is 0 is 0.0"""
        def ratio(a, b):
            return a / b if b else 0.0
        out = {}
        for which, tail in ((0, ''), (1, '_imagine')):
            frames, skipped, n_p, n_g = (int(v) for v in counts[which][:4])
            out[f'voxel_cd{tail}'] = float(resolution) * (ratio(sums[which][0], n_p) + ratio(sums[which][1], n_g))
            for k, thr in enumerate(THRESHOLDS):
                p, r = ratio(int(counts[which][4 + k]), n_p), ratio(int(counts[which][7 + k]), n_g)
                out[f'voxel_precision_{int(thr)}m{tail}'] = p
                out[f'voxel_recall_{int(thr)}m{tail}'] = r
                out[f'voxel_fscore_{int(thr)}m{tail}'] = ratio(2 * p * r, p + r)
            out[f'voxel_cd_frames{tail}'] = frames
            out[f'voxel_cd_skipped{tail}'] = skipped
        return out

    def result(self):
        out = {}
        for idx, a in self.acc.items():
            if a['counts'] is None:
                counts, sums = [[0] * 10] * 2, [[0.0, 0.0]] * 2
            else:
                counts, sums = a['counts'].cpu().tolist(), a['sums'].cpu().tolist()
            out.update({f'{self.prefix}{idx}_{k}': v for k, v in self.summarise(counts, sums, self.cfg.VOXEL.RESOLUTION).items()})
        return out

    def write(self, out_dir):
        path = os.path.join(out_dir, 'voxel_cd.json')
        with open(path, 'w') as fh:
            json.dump(self.result(), fh, indent=1, sort_keys=True)
            fh.write('\n')
        return path
