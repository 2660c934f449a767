"""Per-element restatement in numpy of the frame preparation of the reference's dataset (muvo/data/dataset.py:231-369): the
model for tests/test_dataset.py (against the fixture the real reference wrote) and tests/test_dataset_gpu.py (against the HIP
kernels of muvo_amd/csrc/dataset.hip).  Connected components by flood fill, depth in float64; the range projection and the
voxel densification are the restatements of oracle/muvo_ref.py, which tests/golden/input_pipeline.npz pins to the reference."""
import hashlib

import numpy as np

from oracle import muvo_ref as R

VEHICLE_TAG, PEDESTRIAN_TAG = 10, 4             # constants.py:41-65


def birdview_decode(bev, n_classes):
    """(H, W) integers -> (planes (n, H, W) float32, label (1, H, W) int64, instance mask (H, W) bool)."""
    bev = np.asarray(bev).astype(np.int64)
    planes = np.stack([((bev >> c) & 1) for c in range(n_classes)]).astype(np.float32)
    label = np.full(bev.shape, n_classes - 1, dtype=np.int64)          # argmax of all-zero planes is 0 -> n-1
    for c in range(n_classes):                                         # ascending: the highest set bit stays
        label[planes[c] > 0] = c
    mask = (planes[3] > 0) | (planes[4] > 0)
    return planes, label[None], mask


def label_components(mask):
    """scipy.ndimage.label(mask[None]) with the default structure, by flood fill: 4-connectivity in the plane, components
    numbered from 1 in the order a row-major scan meets their first pixel.  (1, H, W) int32."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    out = np.zeros((H, W), dtype=np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(m)):                                 # np.nonzero is row-major
        if out[y0, x0]:
            continue
        n += 1
        out[y0, x0] = n
        stack = [(int(y0), int(x0))]
        while stack:
            y, x = stack.pop()
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and not out[yy, xx]:
                    out[yy, xx] = n
                    stack.append((yy, xx))
    return out[None]


def remap_table():
    return R.label_remap()                                             # 23 entries, as the reference builds it


def depth_semantic_decode(rgba):
    """(H, W, 4) uint8 -> semantic_image (1, H, W) int64, image_instance_mask (1, H, W) bool, depth_color (3, H, W) and depth
    (1, H, W) float64."""
    a = rgba[..., 3]
    semantic = remap_table()[a][None].astype(np.int64)
    inst = ((a == VEHICLE_TAG) | (a == PEDESTRIAN_TAG))[None]
    col = rgba[..., :3].transpose(2, 0, 1).astype(np.float64)
    depth = (256 ** 2 * col[0] + 256 * col[1] + col[2]) / (256 ** 3 - 1)
    depth[depth > 0.999] = -1
    return semantic, inst, col / 255.0, depth[None]


def prepare_sequence(raw, cfg):
    """The reference's __getitem__ result (numpy, (s, ...)) from CarlaDataset.read_raw's arrays."""
    s = raw['image'].shape[0]
    out = {k: raw[k] for k in ('image', 'route_map', 'steering', 'throttle_brake', 'speed', 'reward', 'value_function', 'intrinsics',
                               'extrinsics')}
    per = {}

    def put(k, v):
        per.setdefault(k, []).append(v)

    for f in range(s):
        planes, label, mask = birdview_decode(raw['birdview_int'][f], raw['n_classes'])
        put('birdview', planes), put('birdview_label', label), put('instance_label', label_components(mask))
        n = int(raw['num_points'][f])
        xyzd, seg = R.range_projection(raw['points_xyz'][f, :n], raw['obj_tag'][f, :n], lidar_position=tuple(cfg.POINTS.LIDAR_POSITION),
                                       fov=tuple(cfg.POINTS.FOV), H=cfg.POINTS.CHANNELS, W=cfg.POINTS.HORIZON_RESOLUTION)
        if cfg.MODEL.LIDAR.ENABLED:
            put('range_view_pcd_xyzd', xyzd)
        if cfg.LIDAR_SEG.ENABLED:
            put('range_view_pcd_seg', seg[None].astype(np.int64))
        if cfg.VOXEL_SEG.ENABLED:
            q = int(raw['num_voxels'][f])
            put('voxel', R.voxel_grid(raw['voxel_rows'][f, :q], size=tuple(cfg.VOXEL.SIZE))[None])
        if 'depth_semantic' in raw:
            semantic, inst, col, depth = depth_semantic_decode(raw['depth_semantic'][f])
            if cfg.LOSSES.RGB_INSTANCE:
                put('image_instance_mask', inst)
            if cfg.SEMANTIC_IMAGE.ENABLED:
                put('semantic_image', semantic)
            if cfg.DEPTH.ENABLED:
                put('depth_color', col), put('depth', depth)
    out.update({k: np.stack(v) for k, v in per.items()})
    return out


def prepare_batch(raws, cfg):
    """b sequences -> the collated batch (b, s, ...)."""
    seqs = [prepare_sequence(r, cfg) for r in raws]
    return {k: np.stack([q[k] for q in seqs]) for k in seqs[0]}


# ---- what the fixture records of an array (tools/golden/make_golden_dataset.py) ----------------------------------------------
SAMPLE_STRIDE, FULL_BELOW = 997, 4096


def digest(a):
    a = np.ascontiguousarray(a)
    return {'dtype': str(a.dtype), 'shape': list(a.shape), 'sha256': hashlib.sha256(a.tobytes()).hexdigest()}


def sample(a):
    flat = np.ascontiguousarray(a).reshape(-1)
    return flat if flat.size <= FULL_BELOW else flat[::SAMPLE_STRIDE]
