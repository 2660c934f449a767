"""Prediction panels: the picture grids of the reference's `WorldModelTrainer.visualise` (trainer.py:569-957), rendered on the
device.  The reference copies every output tensor to the host and builds the grids there (argmax, palette indexing, F.pad,
torch.cat, rot90, numpy loops); here csrc/visualise.hip writes every tile of a grid straight from the model's tensors into
the final uint8 mosaic, and only those bytes leave the device (`PanelWriter`: one copy per panel).

`render_panels(cfg, batch, output, output_imagines)` returns {suffix: uint8 device tensor}.  With s the label's time length,
rf that of `output` and one row per imagined sample (row 0: reconstruction then imagination 0; row i > 0: a blank receptive part
then imagination i; without imaginations one row, the reconstruction), a STRIP stacks the rows of step t top to bottom, runs
the steps left to right and puts one all-255 block of width `sep` before step rf when rf < s:

    _bev              SEMANTIC_SEG         birdview_label[:, :, 0] / argmax bev_segmentation_1, BIRDVIEW_COLOURS, pad 2 of 204,
                                           every padded tile rotated (rot90 k = 1), blank = class 0, sep int((H + 4) / 4)
    _rgb              EVAL.RGB_SUPERVISION throttle bar, steering bar (unpadded), rgb_label_1, rgb_1 rows; pad 5 of 204,
                                           blank 255, sep int(w / 4)
    _pcd_xy           LIDAR_RE             bird's-eye scatter (256 x 256) of range_view_label_1 / lidar_reconstruction_1; pad 2 of
                                           51, blank 255, sep 65
    _sem_image        SEMANTIC_IMAGE       semantic_image_label_1[:, :, 0] / argmax semantic_image_1, VOXEL_COLOURS, pad 5 of 204,
                                           blank = class 0, sep int((w + 10) / 4)
    _input_route_map  MODEL.ROUTE          batch['route_map'] (normalised: it clips), one row, pad 2 of 204, sep int((w + 4) / 4)
    _voxel_top        VOXEL_SEG            top view (own definition, include/muvo_hip.h) of voxel_label_1[:, :, 0] / voxel_1,
                                           VOXEL_COLOURS, pad 2 of 204, blank = class 0, sep int((Y + 4) / 4)
    _lidar_seg        LIDAR_SEG            no strip (trainer.py:868-869): one column of tiles, pad 3 of 204 - the s targets, one
                                           all-255 tile, then the tiles of every row
    _lidar            LIDAR_RE             video (b, T, 1, 2H, W): channel -1 of range_view_label_1 above reconstruction + imagination 0
    _depth            DEPTH                video (b, T, 1, 2h, w): prediction above depth_label_1 (trainer.py:919)

Float images become bytes by the rule of `ops.image_u8` - trunc(x * 255) saturated, what TensorBoard's writer does to a float
image.  `_traj` is not one of these panels: it is opt-in (`WorldModelTrainer.traj_panels`) and lives in muvo_amd/odometry.py
(ICP between consecutive lidar frames on the device); `_flow` likewise (`WorldModelTrainer.flow_panels`, muvo_amd/flow.py: dense
optical flow between consecutive camera frames on the device); the reference's matplotlib voxel figures likewise: `_voxel`
(`WorldModelTrainer.voxel_panels`, muvo_amd/voxel_view.py: the grids ray-cast in 3-D on the device, next to `_voxel_top`).  Not built:
the numbers cv2.putText prints into the bars and TensorBoard's tiling of the batch into one grid."""
import os
import struct
import zlib

import numpy as np
import torch

# The reference's two colour tables (constants.py:22-30,94-95), kept as numbers.
BIRDVIEW_COLOURS = ((255, 255, 255), (225, 225, 225), (160, 160, 160), (0, 83, 138), (127, 255, 212), (50, 205, 50), (255, 215, 0),
                    (220, 20, 60))
VOXEL_COLOURS = ((255, 255, 255), (115, 115, 115))
PAD_BYTE, PCD_PAD_BYTE = 204, 51          # trunc(0.8 * 255), trunc(0.2 * 255)
PCD_IMAGE = 256                           # pcd_xy_image's image_size (trainer.py:981)
SUFFIXES = ('_bev', '_rgb', '_lidar', '_pcd_xy', '_lidar_seg', '_sem_image', '_depth', '_voxel_top', '_input_route_map')
VIDEO_SUFFIXES = ('_lidar', '_depth')


def palette256(table):
    """(256, 3) uint8: `table`, then for every class c past its end ((37c) % 256, (91c + 60) % 256, (151c + 120) % 256).  The
    reference indexes its table directly and raises there (VOXEL_COLOURS has 2 entries, LIDAR_SEG.N_CLASSES is 9)."""
    pal = np.zeros((256, 3), np.uint8)
    for c in range(256):
        pal[c] = table[c] if c < len(table) else ((37 * c) % 256, (91 * c + 60) % 256, (151 * c + 120) % 256)
    return pal


_PALETTES = {}


def _palette(table, device):
    """(the 256-entry palette on the device, the byte of a blank tile: class 0)"""
    key = (table, str(device))
    if key not in _PALETTES:
        pal = palette256(table)
        assert pal[0, 0] == pal[0, 1] == pal[0, 2], 'a blank tile is one byte value: class 0 must be grey'
        _PALETTES[key] = (torch.from_numpy(pal).to(device), int(pal[0, 0]))
    return _PALETTES[key]


def panel_enabled(cfg):
    """The suffixes `render_panels` delivers for cfg, in the reference's order."""
    on = {'_bev': cfg.SEMANTIC_SEG.ENABLED, '_rgb': cfg.EVAL.RGB_SUPERVISION, '_lidar': cfg.LIDAR_RE.ENABLED,
          '_pcd_xy': cfg.LIDAR_RE.ENABLED, '_lidar_seg': cfg.LIDAR_SEG.ENABLED, '_sem_image': cfg.SEMANTIC_IMAGE.ENABLED,
          '_depth': cfg.DEPTH.ENABLED, '_voxel_top': cfg.VOXEL_SEG.ENABLED, '_input_route_map': cfg.MODEL.ROUTE.ENABLED}
    return [k for k in SUFFIXES if on[k]]


def strip_size(rows, tile_w, s, rf, sep):
    """(PH, PW) of a strip whose rows have the heights `rows` and whose tiles are tile_w wide."""
    return sum(rows), s * tile_w + (sep if rf < s else 0)


def panel_sizes(cfg, shapes, s, rf, n_rows):
    """{suffix: shape of the panel without the batch axis} from the tile sizes: shapes = {'bev': (H, W), 'rgb': (h, w),
    'lidar': (H, W), 'lidar_seg': (H, W), 'sem_image': (h, w), 'depth': (h, w), 'voxel': (X, Y, Z), 'route': (h, w)};
    n_rows = max(number of imagined samples, 1)."""
    out = {}
    for suffix in panel_enabled(cfg):
        if suffix == '_bev':
            H, W = shapes['bev']
            out[suffix] = (3, *strip_size([W + 4] * (1 + n_rows), H + 4, s, rf, int((H + 4) / 4)))
        elif suffix == '_rgb':
            h, w = shapes['rgb']
            out[suffix] = (3, *strip_size([int(h / 4)] * 2 + [h + 10] * (1 + n_rows), w + 10, s, rf, int(w / 4)))
        elif suffix == '_pcd_xy':
            out[suffix] = (3, *strip_size([PCD_IMAGE + 4] * (1 + n_rows), PCD_IMAGE + 4, s, rf, int((PCD_IMAGE + 4) / 4)))
        elif suffix == '_sem_image':
            h, w = shapes['sem_image']
            out[suffix] = (3, *strip_size([h + 10] * (1 + n_rows), w + 10, s, rf, int((w + 10) / 4)))
        elif suffix == '_input_route_map':
            h, w = shapes['route']
            out[suffix] = (3, *strip_size([h + 4], w + 4, s, rf, int((w + 4) / 4)))
        elif suffix == '_voxel_top':
            X, Y, _ = shapes['voxel']
            out[suffix] = (3, *strip_size([X + 4] * (1 + n_rows), Y + 4, s, rf, int((Y + 4) / 4)))
        elif suffix == '_lidar_seg':
            H, W = shapes['lidar_seg']
            out[suffix] = (3, (s + 1 + n_rows * s) * (H + 6), W + 6)
        elif suffix == '_lidar':
            H, W = shapes['lidar']
            out[suffix] = (s, 1, 2 * H, W)
        elif suffix == '_depth':
            h, w = shapes['depth']
            out[suffix] = (s, 1, 2 * h, w)
    return out


class _Strip:
    """One strip panel and the placement of its tiles."""

    def __init__(self, b, rows, tile_w, s, rf, sep, device):
        from muvo_amd import ops
        self.ops, self.s, self.rf, self.tile_w, self.sep = ops, s, rf, tile_w, sep
        self.y = [sum(rows[:i]) for i in range(len(rows))]
        PH, PW = strip_size(rows, tile_w, s, rf, sep)
        self.panel = torch.empty((b, 3, PH, PW), dtype=torch.uint8, device=device)
        if rf < s and sep > 0:
            ops.panel_fill(b, PH, sep, 255, self.panel, ops.tile_place(self.panel, 1, x0=rf * tile_w))

    def place(self, row, T, t0=0):
        tsep = self.rf if self.rf < self.s else self.ops.PANEL_NO_SEP
        return self.ops.tile_place(self.panel, T, t0, y0=self.y[row], xstep=self.tile_w, tsep=tsep, sepw=self.sep)


def _frames(x):
    """(b, T, ...) -> (b * T, ...) without a copy where the tensor allows it."""
    return x.reshape(x.shape[0] * x.shape[1], *x.shape[2:])


def _labels(x):
    """A label tensor (b, T, 1, ...) or (b, T, ...) as frames of uint8 / int64 classes."""
    if x.dim() >= 5 and x.shape[2] == 1:
        x = x[:, :, 0]
    if x.dtype not in (torch.uint8, torch.int64):
        x = x.long()
    return _frames(x)


def _lengths(s, rf, imagines, key, what):
    fh = imagines[0][key].shape[1] if imagines else 0
    if rf + fh != s:
        raise ValueError(f'{what}: {rf} reconstructed + {fh} imagined frames for a label of {s} (the rows of a panel cover every step)')
    return fh


def _rows(imagines):
    return max(len(imagines), 1)


def _prediction_rows(imagines, recon, imagine, blank, first_row=1):
    """Row first_row + i: the reconstruction (i = 0) or a blank receptive part, then imagination i."""
    for i in range(_rows(imagines)):
        if i == 0:
            recon(first_row)
        else:
            blank(first_row + i)
        if imagines:
            imagine(first_row + i, imagines[i])


def _class_strip(target, pred, imagines, key, table, pad, s, rf, rotate=False):
    from muvo_amd import ops
    b = pred.shape[0]
    h, w = pred.shape[-2:]
    fh = _lengths(s, rf, imagines, key, key)
    pal, blank0 = _palette(table, pred.device)
    th, tw = (w + 2 * pad, h + 2 * pad) if rotate else (h + 2 * pad, w + 2 * pad)
    st = _Strip(b, [th] * (1 + _rows(imagines)), tw, s, rf, int(tw / 4), pred.device)
    ops.panel_classes(_labels(target), pal, st.panel, st.place(0, s), pad, PAD_BYTE, rotate)
    _prediction_rows(
        imagines,
        lambda row: ops.panel_classes(_frames(pred.detach()), pal, st.panel, st.place(row, rf), pad, PAD_BYTE, rotate),
        lambda row, im: ops.panel_classes(_frames(im[key].detach()), pal, st.panel, st.place(row, fh, rf), pad, PAD_BYTE, rotate),
        lambda row: ops.panel_fill(b * rf, th - 2 * pad, tw - 2 * pad, blank0, st.panel, st.place(row, rf), pad, PAD_BYTE))
    return st.panel


def render_panels(cfg, batch, output, output_imagines):
    """trainer.py:569-957 block by block: {suffix: uint8 device tensor} - (b, 3, PH, PW) strips and `_lidar_seg`, (b, T, 1, 2H, W)
    videos.  `batch` is the batch after `preprocess`; nothing is copied to the host and the host never waits."""
    from muvo_amd import ops
    imagines = list(output_imagines or [])
    s = next(iter(batch.values())).shape[1]
    rf = list(output.values())[-1].shape[1]
    panels = {}
    if cfg.SEMANTIC_SEG.ENABLED:
        panels['_bev'] = _class_strip(batch['birdview_label'], output['bev_segmentation_1'], imagines, 'bev_segmentation_1',
                                      BIRDVIEW_COLOURS, 2, s, rf, rotate=True)
    if cfg.EVAL.RGB_SUPERVISION:
        pred = output['rgb_1'].detach()
        b, _, _, h, w = pred.shape
        fh = _lengths(s, rf, imagines, 'rgb_1', '_rgb')
        bh = int(h / 4)
        st = _Strip(b, [bh, bh] + [h + 10] * (1 + _rows(imagines)), w + 10, s, rf, int(w / 4), pred.device)
        ops.panel_bars(batch['throttle_brake'].float().reshape(-1), 0, h, w, st.panel, st.place(0, s))
        ops.panel_bars(batch['steering'].float().reshape(-1), 1, h, w, st.panel, st.place(1, s))
        ops.panel_image(_frames(batch['rgb_label_1'].float()), st.panel, st.place(2, s), 5, PAD_BYTE)
        _prediction_rows(
            imagines,
            lambda row: ops.panel_image(_frames(pred), st.panel, st.place(row, rf), 5, PAD_BYTE),
            lambda row, im: ops.panel_image(_frames(im['rgb_1'].detach()), st.panel, st.place(row, fh, rf), 5, PAD_BYTE),
            lambda row: ops.panel_fill(b * rf, h, w, 255, st.panel, st.place(row, rf), 5, PAD_BYTE), first_row=3)
        panels['_rgb'] = st.panel
    if cfg.LIDAR_RE.ENABLED:
        target = batch['range_view_label_1'].float()
        pred = output['lidar_reconstruction_1'].detach()
        b, _, _, H, W = pred.shape
        fh = _lengths(s, rf, imagines, 'lidar_reconstruction_1', '_lidar')
        video = torch.empty((b, s, 1, 2 * H, W), dtype=torch.uint8, device=pred.device)
        ops.panel_image(_frames(target), video, ops.tile_place(video, s, ystep=2 * H), channel=-1)
        ops.panel_image(_frames(pred), video, ops.tile_place(video, rf, y0=H, ystep=2 * H), channel=-1)
        if imagines:
            ops.panel_image(_frames(imagines[0]['lidar_reconstruction_1'].detach()), video,
                            ops.tile_place(video, fh, rf, y0=H, ystep=2 * H), channel=-1)
        panels['_lidar'] = video
        n = PCD_IMAGE
        scale = float(cfg.LIDAR_RE.SCALE)
        st = _Strip(b, [n + 4] * (1 + _rows(imagines)), n + 4, s, rf, int((n + 4) / 4), pred.device)
        ops.panel_scatter(_frames(target), scale, st.panel, st.place(0, s), 2, PCD_PAD_BYTE)
        _prediction_rows(
            imagines,
            lambda row: ops.panel_scatter(_frames(pred), scale, st.panel, st.place(row, rf), 2, PCD_PAD_BYTE),
            lambda row, im: ops.panel_scatter(_frames(im['lidar_reconstruction_1'].detach()), scale, st.panel, st.place(row, fh, rf),
                                              2, PCD_PAD_BYTE),
            lambda row: ops.panel_fill(b * rf, n, n, 255, st.panel, st.place(row, rf), 2, PCD_PAD_BYTE))
        panels['_pcd_xy'] = st.panel
    if cfg.LIDAR_SEG.ENABLED:
        key = 'lidar_segmentation_1'
        pred = output[key].detach()
        b, _, _, H, W = pred.shape
        fh = _lengths(s, rf, imagines, key, '_lidar_seg')
        pal, blank0 = _palette(VOXEL_COLOURS, pred.device)
        th = H + 6
        panel = torch.empty((b, 3, (s + 1 + _rows(imagines) * s) * th, W + 6), dtype=torch.uint8, device=pred.device)

        def at(T, t0):
            return ops.tile_place(panel, T, t0, ystep=th)
        ops.panel_classes(_labels(batch['range_view_seg_label_1']), pal, panel, at(s, 0), 3, PAD_BYTE)
        ops.panel_fill(b, th, W + 6, 255, panel, at(1, s))
        _prediction_rows(
            imagines,
            lambda row: ops.panel_classes(_frames(pred), pal, panel, at(rf, s + 1 + row * s), 3, PAD_BYTE),
            lambda row, im: ops.panel_classes(_frames(im[key].detach()), pal, panel, at(fh, s + 1 + row * s + rf), 3, PAD_BYTE),
            lambda row: ops.panel_fill(b * rf, H, W, blank0, panel, at(rf, s + 1 + row * s), 3, PAD_BYTE), first_row=0)
        panels['_lidar_seg'] = panel
    if cfg.SEMANTIC_IMAGE.ENABLED:
        panels['_sem_image'] = _class_strip(batch['semantic_image_label_1'], output['semantic_image_1'], imagines, 'semantic_image_1',
                                            VOXEL_COLOURS, 5, s, rf)
    if cfg.DEPTH.ENABLED:
        pred = output['depth_1'].detach()
        b, _, _, h, w = pred.shape
        fh = _lengths(s, rf, imagines, 'depth_1', '_depth')
        video = torch.empty((b, s, 1, 2 * h, w), dtype=torch.uint8, device=pred.device)
        ops.panel_image(_frames(pred), video, ops.tile_place(video, rf, ystep=2 * h))
        if imagines:
            ops.panel_image(_frames(imagines[0]['depth_1'].detach()), video, ops.tile_place(video, fh, rf, ystep=2 * h))
        ops.panel_image(_frames(batch['depth_label_1'].float()), video, ops.tile_place(video, s, y0=h, ystep=2 * h))
        panels['_depth'] = video
    if cfg.VOXEL_SEG.ENABLED:
        pred = output['voxel_1'].detach()
        b, _, _, X, Y, Z = pred.shape
        fh = _lengths(s, rf, imagines, 'voxel_1', '_voxel_top')
        pal, blank0 = _palette(VOXEL_COLOURS, pred.device)
        st = _Strip(b, [X + 4] * (1 + _rows(imagines)), Y + 4, s, rf, int((Y + 4) / 4), pred.device)
        label = batch['voxel_label_1']
        label = label[:, :, 0] if label.dim() == 6 else label
        ops.panel_voxel_top(_frames(label.to(torch.uint8)), pal, st.panel, st.place(0, s), 2, PAD_BYTE)
        _prediction_rows(
            imagines,
            lambda row: ops.panel_voxel_top(_frames(pred), pal, st.panel, st.place(row, rf), 2, PAD_BYTE),
            lambda row, im: ops.panel_voxel_top(_frames(im['voxel_1'].detach()), pal, st.panel, st.place(row, fh, rf), 2, PAD_BYTE),
            lambda row: ops.panel_fill(b * rf, X, Y, blank0, st.panel, st.place(row, rf), 2, PAD_BYTE))
        panels['_voxel_top'] = st.panel
    if cfg.MODEL.ROUTE.ENABLED:
        route = batch['route_map'].float()
        b, _, _, h, w = route.shape
        st = _Strip(b, [h + 4], w + 4, s, rf, int((w + 4) / 4), route.device)
        ops.panel_image(_frames(route), st.panel, st.place(0, s), 2, PAD_BYTE)
        panels['_input_route_map'] = st.panel
    return panels


# ---- writer -----------------------------------------------------------------------------------------------------------------------
def png_bytes(image):
    """An (H, W) or (H, W, 3) uint8 array as a PNG file (8-bit grey / RGB, no filter) with the standard library alone."""
    image = np.ascontiguousarray(image)
    assert image.dtype == np.uint8 and (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3)), (image.dtype, image.shape)
    H, W = image.shape[:2]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), image.reshape(H, -1)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    head = struct.pack('>IIBBBBB', W, H, 8, 0 if image.ndim == 2 else 2, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', head) + chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b'')


def png_read(data):
    """The inverse of png_bytes (its own output only: 8-bit grey or RGB, filter 0, no interlace)."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, head = 8, b'', None
    while pos < len(data):
        n, tag = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b'IHDR':
            head = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    W, H, depth, colour = head[:4]
    assert depth == 8 and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * ch)
    assert not rows[:, 0].any()
    image = rows[:, 1:].reshape(H, W, ch)
    return image[:, :, 0].copy() if ch == 1 else image.copy()


class PanelWriter:
    """`add_images(name, tensor, global_step)` / `add_video(name, tensor, global_step, fps=2)` of the reference's TensorBoard
    writer, writing PNG files: one device-to-host copy per panel, one file per sample,
    `{directory}/{name}/step{global_step:08d}_b{i}.png`; the frames of a video lie side by side."""

    def __init__(self, directory):
        self.directory = str(directory)
        self.files = []

    def _write(self, name, host, global_step):
        folder = os.path.join(self.directory, name)
        os.makedirs(folder, exist_ok=True)
        for i, image in enumerate(host):
            image = image[0] if image.shape[0] == 1 else image.transpose(1, 2, 0)
            path = os.path.join(folder, f'step{int(global_step):08d}_b{i}.png')
            with open(path, 'wb') as fh:
                fh.write(png_bytes(image))
            self.files.append(path)

    def add_images(self, name, tensor, global_step=0):
        assert tensor.dtype == torch.uint8 and tensor.dim() == 4
        self._write(name, tensor.cpu().numpy(), global_step)

    def add_video(self, name, tensor, global_step=0, fps=2):
        assert tensor.dtype == torch.uint8 and tensor.dim() == 5
        host = tensor.cpu().numpy()                                     # (b, T, c, H, W) -> (b, c, H, T * W)
        b, T, c, H, W = host.shape
        self._write(name, host.transpose(0, 2, 3, 1, 4).reshape(b, c, H, T * W), global_step)


def write_panels(writer, name, panels, global_step):
    for suffix, tensor in panels.items():
        if suffix in VIDEO_SUFFIXES:
            writer.add_video(f'{name}{suffix}', tensor, global_step=global_step, fps=2)
        else:
            writer.add_images(f'{name}{suffix}', tensor, global_step=global_step)
