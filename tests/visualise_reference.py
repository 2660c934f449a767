"""Host restatement of the reference's picture grids (trainer.py:569-1007) in plain torch / numpy: float tiles in [0, 1], padded,
concatenated and rotated the way the reference does it, turned into bytes at the very end by TensorBoard's rule
(`(x.astype(float32) * 255).clip(0, 255).astype(uint8)`).  Plus the project's three own definitions: palettes beyond the
reference's tables, the bars without their text, the voxel top view.  tests/golden/visualise_ref.npz (made by
tools/make_golden_visualise.py from the real reference) pins the reference-backed parts; the GPU tests compare
csrc/visualise.hip with this file bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

from muvo_amd.visualise import BIRDVIEW_COLOURS, VOXEL_COLOURS, palette256

SCALE = 50            # LIDAR_RE.SCALE


def to_u8(x):
    """What the TensorBoard writer does to a float image or video; NaN -> 0 (there the cast is undefined)."""
    t = np.asarray(x).astype(np.float32) * np.float32(255)
    return np.nan_to_num(t, nan=0.0).clip(0, 255).astype(np.uint8)


def colours(table):
    return torch.from_numpy(palette256(table)) / 255.0


def strip(rows, s, rf, sep, sep_at=None, reverse_rows=False):
    """rows: list of (b, s, c, h_i, w) float tensors -> (b, c, sum h_i, s * w [+ sep]): per step the rows top to bottom, the
    steps left to right, ones of width sep before step rf.  The keyword arguments plant errors for the tests."""
    rows = rows[::-1] if reverse_rows else rows
    grid = torch.cat(rows, dim=-2)
    b, _, c, h, _ = grid.shape
    parts = []
    for step in range(s):
        if step == (rf if sep_at is None else sep_at):
            parts.append(torch.ones(b, c, h, sep, dtype=grid.dtype))
        parts.append(grid[:, step])
    return torch.cat(parts, dim=-1)


def prediction_rows(pred, imagines, blank):
    """Row i: the reconstruction (i = 0) or `blank`-valued frames of its shape, then imagination i (if there are any)."""
    rows = []
    for i, im in enumerate(imagines if imagines else [None]):
        first = pred if i == 0 else torch.full_like(pred, blank)
        rows.append(first if im is None else torch.cat([first, im], dim=1))
    return rows


def class_tiles(cls, table, pad, value=0.8):
    """(b, T, h, w) integer classes -> (b, T, 3, h + 2 pad, w + 2 pad) float colours with a border of `value`."""
    return F.pad(colours(table)[cls.long() & 255].permute(0, 1, 4, 2, 3), [pad] * 4, 'constant', value)


def argmax(logits):
    """torch.argmax over dim -3 (the first maximum on ties, like the kernels' strict >)."""
    return torch.argmax(logits, dim=-3)


def bev(target, pred, imagines, s, rf, transposed_rotation=False, **planted):
    """trainer.py:604-646.  target (b, s, H, W) classes; pred / imagines logits (b, T, C, H, W)."""
    rows = [class_tiles(target, BIRDVIEW_COLOURS, 2)]
    rows += [class_tiles(p, BIRDVIEW_COLOURS, 2) for p in prediction_rows(argmax(pred), [argmax(i) for i in imagines], 0)]
    wide = torch.cat(rows[::-1], dim=-1)                       # predictions in reverse order, the target last, side by side ...
    if transposed_rotation:
        wide = torch.cat(rows, dim=-1).transpose(3, 4)
    else:
        wide = torch.rot90(wide, k=1, dims=[3, 4])             # ... so that the rotation puts the target on top
    return to_u8(strip([wide], s, rf, int(wide.shape[-1] / 4), **planted))


def sem_image(target, pred, imagines, s, rf, **planted):
    """trainer.py:875-910"""
    rows = [class_tiles(target, VOXEL_COLOURS, 5)]
    rows += [class_tiles(p, VOXEL_COLOURS, 5) for p in prediction_rows(argmax(pred), [argmax(i) for i in imagines], 0)]
    return to_u8(strip(rows, s, rf, int(rows[0].shape[-1] / 4), **planted))


def lidar_seg(target, pred, imagines):
    """trainer.py:845-872: every tile below the other - the targets, one tile of ones, then the rows."""
    t = class_tiles(target, VOXEL_COLOURS, 3)
    rows = [class_tiles(p, VOXEL_COLOURS, 3) for p in prediction_rows(argmax(pred), [argmax(i) for i in imagines], 0)]
    col = torch.cat([t, torch.ones_like(t[:, -1:]), *rows], dim=1)
    return to_u8(col.transpose(1, 2).flatten(2, 3))


def depth(target, pred, imagines):
    """trainer.py:913-921: (b, T, 1, 2h, w), the prediction above the label."""
    if imagines:
        pred = torch.cat([pred, imagines[0]], dim=1)
    return to_u8(torch.cat([pred, target], dim=-2))


def lidar(target, pred, imagines):
    """trainer.py:755-769: (b, T, 1, 2H, W), the last channel; the label above."""
    if imagines:
        pred = torch.cat([pred, imagines[0]], dim=1)
    return to_u8(torch.cat([target[:, :, -1], pred[:, :, -1]], dim=-2).unsqueeze(-3))


def route_map(route, s, rf, **planted):
    """trainer.py:944-957"""
    tiles = F.pad(route, [2, 2, 2, 2], 'constant', 0.8)
    return to_u8(strip([tiles], s, rf, int(tiles.shape[-1] / 4), **planted))


def pcd_xy_image(range_view, strict=True):
    """trainer.py:980-1007 for (b, T, C, H, W) float32: (b, T, 3, 256, 256) float64 of zeros and ones.  float32 arithmetic in the
    reference's order: scale, negate, * 2.56, + 128.  strict=False plants a non-strict bound."""
    pts = range_view.numpy().transpose(0, 1, 3, 4, 2) * SCALE
    xy = -pts[..., :2]
    xy *= 256 / (2 * 50)
    xy += np.array([128.0, 128.0]).reshape(1, 1, 1, 1, 2)
    valid = pts[..., -1] > 0
    b, T = pts.shape[:2]
    image = np.zeros((b, T, 256, 256, 3))
    for i in range(b):
        for j in range(T):
            p = xy[i, j][valid[i, j]]
            if strict:
                p = p[(0 < p[:, 0]) & (p[:, 0] < 256) & (0 < p[:, 1]) & (p[:, 1] < 256)]
            else:
                p = p[(0 <= p[:, 0]) & (p[:, 0] < 256) & (0 <= p[:, 1]) & (p[:, 1] < 256)]
            p = np.fabs(p).astype(np.int32)
            image[i, j][p[:, 0], p[:, 1]] = 1.0
    return torch.from_numpy(image.transpose(0, 1, 4, 2, 3))


def pcd_xy(target, pred, imagines, s, rf, **planted):
    """trainer.py:772-806"""
    rows = [F.pad(pcd_xy_image(target), [2, 2, 2, 2], 'constant', 0.2)]
    rows += [F.pad(p, [2, 2, 2, 2], 'constant', 0.2)
             for p in prediction_rows(pcd_xy_image(pred), [pcd_xy_image(i) for i in imagines], 1.0)]
    return to_u8(strip(rows, s, rf, int(rows[0].shape[-1] / 4), **planted))


def bars(values, kind, h, w):
    """trainer.py:679-706 without the text: values (b, s, 1) float32 -> (b, s, 3, int(h/4), w + 10) float in {0, 200, 255} / 255.
    The column range is clamped to the tile (the reference's negative indices wrap for |v| > 1)."""
    b, s = values.shape[:2]
    out = np.ones((b, s, int(h / 4), w + 10, 3)).astype(np.uint8) * 255
    mid = int(w / 2) + 5
    for i in range(b):
        for t in range(s):
            v = values[i, t].reshape(-1)[:1].float()
            k = int(w / 2 * v)
            lo, hi = (mid, mid + k) if v >= 0 else (mid + k, mid)
            lo, hi = max(lo, 0), min(hi, w + 10)
            colour = (0, 0, 200) if kind == 1 else ((0, 200, 0) if v >= 0 else (200, 0, 0))
            if hi > lo:
                out[i, t, 5:max(int(h / 4) - 5, 5), lo:hi, :] = colour
    return torch.tensor(out.transpose(0, 1, 4, 2, 3), dtype=torch.float) / 255.0


def rgb(target, pred, imagines, throttle, steering, s, rf, **planted):
    """trainer.py:656-721 (the text in the bars left out)"""
    h, w = target.shape[-2:]
    rows = [bars(throttle, 0, h, w), bars(steering, 1, h, w), F.pad(target, [5] * 4, 'constant', 0.8)]
    rows += [F.pad(p, [5] * 4, 'constant', 0.8) for p in prediction_rows(pred, imagines, 1.0)]
    return to_u8(strip(rows, s, rf, int(w / 4), **planted))


def voxel_top_tiles(cls, table):
    """Own definition: (b, T, X, Y, Z) classes -> (b, T, 3, X, Y) uint8.  z* = the highest z with a class != 0; none: palette[0];
    else (p * (96 + (159 z*) // max(Z - 1, 1))) // 255; tile pixel [i][j] = column x = X - 1 - i, y = j."""
    pal = palette256(table).astype(np.int64)
    cls = np.asarray(cls).astype(np.int64) & 255
    Z = cls.shape[-1]
    occupied = cls != 0
    top = Z - 1 - np.argmax(occupied[..., ::-1], axis=-1)
    any_ = occupied.any(-1)
    c = np.take_along_axis(cls, top[..., None], -1)[..., 0]
    shade = 96 + (159 * top) // max(Z - 1, 1)
    tile = np.where(any_[..., None], (pal[c] * shade[..., None]) // 255, pal[0])
    return np.ascontiguousarray(tile[:, :, ::-1].transpose(0, 1, 4, 2, 3)).astype(np.uint8)


def voxel_top(target, pred, imagines, s, rf, **planted):
    """target (b, s, X, Y, Z) classes, pred / imagines logits (b, T, C, X, Y, Z)."""
    def tiles(cls):
        return F.pad(torch.from_numpy(voxel_top_tiles(cls, VOXEL_COLOURS)), [2] * 4, 'constant', 204)
    am = [torch.argmax(i, dim=2) for i in imagines]
    rows = [tiles(target)] + [tiles(p) for p in prediction_rows(torch.argmax(pred, dim=2), am, 0)]
    return strip([r.float() / 255.0 for r in rows], s, rf, int(rows[0].shape[-1] / 4), **planted).mul(255).round().byte().numpy()


def panel_cfg(**on):
    """A config with exactly the heads of `on` switched on (keys: bev, rgb, lidar, lidar_seg, sem_image, depth, voxel, route)."""
    from muvo_amd.config import get_cfg
    f = lambda k: bool(on.get(k, False))
    return get_cfg(cfg_dict={'SEMANTIC_SEG': {'ENABLED': f('bev')}, 'EVAL': {'RGB_SUPERVISION': f('rgb')}, 'LIDAR_RE': {'ENABLED': f('lidar')},
                             'LIDAR_SEG': {'ENABLED': f('lidar_seg')}, 'SEMANTIC_IMAGE': {'ENABLED': f('sem_image')},
                             'DEPTH': {'ENABLED': f('depth')}, 'VOXEL_SEG': {'ENABLED': f('voxel')}, 'MODEL': {'ROUTE': {'ENABLED': f('route')}}})


FIXTURE = dict(b=2, s=5, rf=2, bev=(6, 10), lidar_seg=(4, 16), sem_image=(5, 7), depth=(4, 4), route=(4, 4), rgb=(8, 12), lidar=(4, 64),
               voxel=(5, 7, 3))
FIXTURE_HEADS = ('bev', 'lidar_seg', 'sem_image', 'depth', 'route')         # what the reference can draw without cv2 / open3d / matplotlib
FIXTURE_SUFFIXES = ('_bev', '_lidar_seg', '_sem_image', '_depth', '_input_route_map')


def fixture_inputs(n_samples, seed=2024, seg_classes=2, rf=None):
    """Seeded (batch, output, imagines) host dicts at the fixture's shapes; without imagined samples the output covers all s frames.
    seg_classes: classes of the lidar / camera segmentation heads (the reference's table has 2)."""
    g = torch.Generator().manual_seed(seed + n_samples)
    b, s = FIXTURE['b'], FIXTURE['s']
    rf = (FIXTURE['rf'] if n_samples else s) if rf is None else rf
    fh = s - rf if n_samples else 0
    rand = lambda *shape: torch.rand(*shape, generator=g) * 1.5 - 0.25               # beyond [0, 1] on both sides: the bytes clip
    randn = lambda *shape: torch.randn(*shape, generator=g)
    ints = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)
    X, Y, Z = FIXTURE['voxel']
    range_view = lambda T: torch.cat([randn(b, T, 3, *FIXTURE['lidar']) * 0.5, rand(b, T, 1, *FIXTURE['lidar'])], dim=2)
    batch = {'birdview_label': ints(8, b, s, 1, *FIXTURE['bev']),
             'range_view_seg_label_1': ints(seg_classes, b, s, 1, *FIXTURE['lidar_seg']),
             'semantic_image_label_1': ints(seg_classes, b, s, 1, *FIXTURE['sem_image']),
             'depth_label_1': rand(b, s, 1, *FIXTURE['depth']), 'route_map': rand(b, s, 3, *FIXTURE['route']) * 2,
             'rgb_label_1': rand(b, s, 3, *FIXTURE['rgb']), 'throttle_brake': rand(b, s, 1) * 2 - 1, 'steering': rand(b, s, 1) * 2 - 1,
             'range_view_label_1': range_view(s), 'voxel_label_1': (ints(4, b, s, 1, X, Y, Z) == 1).to(torch.uint8)}

    def heads(T):
        return {'bev_segmentation_1': randn(b, T, 8, *FIXTURE['bev']), 'lidar_segmentation_1': randn(b, T, seg_classes, *FIXTURE['lidar_seg']),
                'semantic_image_1': randn(b, T, seg_classes, *FIXTURE['sem_image']), 'depth_1': rand(b, T, 1, *FIXTURE['depth']),
                'rgb_1': rand(b, T, 3, *FIXTURE['rgb']), 'lidar_reconstruction_1': range_view(T), 'voxel_1': randn(b, T, 2, X, Y, Z)}
    return batch, heads(rf), [heads(fh) for _ in range(n_samples)]


def fixture_range_view(seed=7):
    """(1, 2, 4, 4, 64) float32 scaled range views whose points also sit on and next to the image's borders."""
    g = torch.Generator().manual_seed(seed)
    rv = torch.randn(1, 2, 4, 4, 64, generator=g) * 0.6
    rv[:, :, 3] = torch.rand(1, 2, 4, 64, generator=g) - 0.3                         # ranges of both signs
    edge = torch.tensor([1.0, -1.0, 0.999, -0.999, 0.9999999, 127.5 / 128, -127.5 / 128, 0.0]) # r = 0, 256, just inside, ...
    rv[0, 0, 0, 0, :8], rv[0, 0, 1, 0, :8], rv[0, 0, 3, 0, :8] = edge, edge.flip(0), 0.5
    rv[0, 1, 3, 1, :4] = torch.tensor([0.0, -0.0, -0.5, 1e-30])
    return rv


def render_panels(cfg, batch, output, output_imagines):
    """The counterpart of muvo_amd.visualise.render_panels on host tensors: {suffix: uint8 numpy array}."""
    cpu = lambda d: {k: v.detach().cpu() for k, v in d.items() if torch.is_tensor(v)}
    batch, output, ims = cpu(batch), cpu(output), [cpu(i) for i in (output_imagines or [])]
    s = next(iter(batch.values())).shape[1]
    rf = list(output.values())[-1].shape[1]
    get = lambda key: [i[key].float() for i in ims]
    out = {}
    if cfg.SEMANTIC_SEG.ENABLED:
        out['_bev'] = bev(batch['birdview_label'][:, :, 0], output['bev_segmentation_1'], get('bev_segmentation_1'), s, rf)
    if cfg.EVAL.RGB_SUPERVISION:
        out['_rgb'] = rgb(batch['rgb_label_1'].float(), output['rgb_1'], get('rgb_1'), batch['throttle_brake'], batch['steering'], s, rf)
    if cfg.LIDAR_RE.ENABLED:
        args = batch['range_view_label_1'].float(), output['lidar_reconstruction_1'], get('lidar_reconstruction_1')
        out['_lidar'] = lidar(*args)
        out['_pcd_xy'] = pcd_xy(*args, s, rf)
    if cfg.LIDAR_SEG.ENABLED:
        out['_lidar_seg'] = lidar_seg(batch['range_view_seg_label_1'][:, :, 0], output['lidar_segmentation_1'], get('lidar_segmentation_1'))
    if cfg.SEMANTIC_IMAGE.ENABLED:
        out['_sem_image'] = sem_image(batch['semantic_image_label_1'][:, :, 0], output['semantic_image_1'], get('semantic_image_1'), s, rf)
    if cfg.DEPTH.ENABLED:
        out['_depth'] = depth(batch['depth_label_1'].float(), output['depth_1'], get('depth_1'))
    if cfg.VOXEL_SEG.ENABLED:
        out['_voxel_top'] = voxel_top(batch['voxel_label_1'][:, :, 0], output['voxel_1'], get('voxel_1'), s, rf)
    if cfg.MODEL.ROUTE.ENABLED:
        out['_input_route_map'] = route_map(batch['route_map'].float(), s, rf)
    return out


# ---- helpers of the GPU tests: a panel between guard bytes, and the expected bytes of placed tiles ---------------------------------
SENTINEL = 0x5A


def guarded_panel(shape, device, guard=64):
    """(buffer, panel): a uint8 panel of `shape` inside a buffer of SENTINEL bytes with `guard` bytes on either side (a guard that
    is no multiple of 4 gives a panel whose base does not allow dword stores)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.uint8, device=device)
    return buf, buf[guard:guard + n].view(*shape)


def expected_buffer(expect, guard=64):
    flat = np.full(expect.size + 2 * guard, SENTINEL, np.uint8)
    flat[guard:guard + expect.size] = expect.reshape(-1)
    return flat


def paste(expect, tiles, T, t0=0, x0=0, y0=0, xstep=0, ystep=0, tsep=None, sepw=0):
    """Writes tiles (b, T, c, TH, TW) into expect (b, c, PH, PW) where ops.tile_place(panel, T, t0, x0, ...) puts them."""
    tiles = np.asarray(tiles)
    TH, TW = tiles.shape[-2:]
    for k in range(T):
        t = t0 + k
        r, c = y0 + t * ystep, x0 + t * xstep + (sepw if tsep is not None and t >= tsep else 0)
        assert 0 <= r and r + TH <= expect.shape[-2] and 0 <= c and c + TW <= expect.shape[-1]
        expect[:, :, r:r + TH, c:c + TW] = tiles[:, k]
    return expect
