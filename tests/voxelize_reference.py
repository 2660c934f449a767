"""Numpy restatement of the reference's voxel-label generation (data/generate_voxels.py::voxelize_one ->
data/data_preprocessing.py::read_img, depth2pcd, convert_coor_img, convert_coor_lidar, merge_pcd, voxel_filter) for one frame,
written per element in the reference's order of operations, all float64 unless said otherwise.  tests/golden/voxelize.npz pins
it against the real reference functions; the HIP kernels are compared against it where no fixture exists.

The one thing the reference leaves open is defined here as in the kernels: among the points of a voxel at exactly the same
smallest distance the lowest global index wins (camera pixels row-major, then lidar points in sweep order)."""
import numpy as np

EGO_VEHICLE_DIMENSION = (4.902, 2.128, 1.511)
ROADLINE = 6


def ego_points(depth_semantic, points_xyz, obj_tag, *, camera_position, lidar_position, fov, max_range=100.0):
    """-> (points (n, 3) float64 in the ego frame, tags (n,) uint8, global index (n,) int64) of the valid camera pixels and all
    lidar points, camera first."""
    H, W = depth_semantic.shape[:2]
    c = depth_semantic[..., :3].astype(np.float64).reshape(-1, 3)
    d = 1000 * ((256 ** 2 * c[:, 0] + 256 * c[:, 1] + c[:, 2]) / (256 ** 3 - 1))
    f = W / (2.0 * np.tan(fov * np.pi / 360.0))
    cx, cy = W / 2.0, H / 2.0
    yy, xx = np.mgrid[0:H, 0:W]
    xx, yy = xx.reshape(-1).astype(np.float64), yy.reshape(-1).astype(np.float64)
    x, y = ((xx - cx) * d) / f, ((yy - cy) * d) / f
    keep = (d < 1000) & (np.sqrt((x * x + y * y) + d * d) < max_range)
    forward, right, up = camera_position
    cam = np.float32([forward, -right, up]).astype(np.float64)          # the camera matrix is float32
    e = np.stack([d + cam[0], -x + cam[1], -y + cam[2]], axis=1)[keep]
    lid = (np.asarray(points_xyz, np.float32).reshape(-1, 3).astype(np.float64) + np.asarray(lidar_position, np.float64)).astype(np.float32)
    lid[:, 1] = -lid[:, 1]                                              # in-place float32 update of the sweep
    pts = np.concatenate([e, lid.astype(np.float64)], axis=0)
    tags = np.concatenate([depth_semantic[..., 3].reshape(-1)[keep], np.asarray(obj_tag, np.uint8).reshape(-1)])
    index = np.concatenate([np.nonzero(keep)[0], H * W + np.arange(len(lid))]).astype(np.int64)
    return pts, tags.astype(np.uint8), index


def voxel_rows(depth_semantic, points_xyz, obj_tag, *, camera_position, lidar_position, fov, voxel_resolution, voxel_size, offset,
               mask_ego=True, max_range=100.0):
    """-> int64 (Q, 4): x, y, z, raw tag, ascending in x + y*Dx + z*Dx*Dy."""
    pts, tags, index = ego_points(depth_semantic, points_xyz, obj_tag, camera_position=camera_position, lidar_position=lidar_position,
                                  fov=fov, max_range=max_range)
    if mask_ego:
        x, y, z = EGO_VEHICLE_DIMENSION
        box = np.array([[-x / 2, -y / 2, 0], [x / 2, y / 2, z]])
        with np.errstate(invalid='ignore'):
            ego = ((box[0] < pts) & (pts < box[1])).all(axis=1)
        pts, tags, index = pts[~ego], tags[~ego], index[~ego]
    size, res = np.asarray(voxel_size), np.asarray(voxel_resolution)
    off = np.asarray(offset, dtype=np.float64) + res * size / 2
    b = pts + off
    with np.errstate(invalid='ignore'):
        inside = ((0 <= b) & (b < size * res)).all(axis=1)
    b, tags, index = b[inside], tags[inside], index[inside]
    q, m = np.divmod(b, res)
    q = np.minimum(q.astype(np.int64), size - 1)      # the snap of np.divmod can give `size` within an ulp of the upper face
    h = q[:, 0] + q[:, 1] * size[0] + q[:, 2] * size[0] * size[1]
    dis = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
    order = np.lexsort((index, dis, h))
    first = np.r_[True, h[order][1:] != h[order][:-1]] if len(order) else np.zeros(0, bool)
    win = order[first]
    lab = tags[win].astype(np.int64)
    road = np.zeros(int(size.prod()), bool)
    road[h[tags == ROADLINE]] = True
    lab[road[h[win]]] = ROADLINE
    hv = h[win]
    return np.stack([hv % size[0], (hv // size[0]) % size[1], hv // (size[0] * size[1]), lab], axis=1).astype(np.int64).reshape(-1, 4)


def label_remap():
    """constants.py:180-204 + dataset.py:281-283 as a 256-entry table."""
    t = np.ones(256, np.uint8)
    t[0] = t[13] = 0
    return t


def dense_grid(rows, voxel_size):
    """dataset.py:316-327 on rows (Q, 4)."""
    sem = rows[:, 3].copy()
    sem[sem == 255] = 0
    vox = np.zeros(tuple(voxel_size), np.uint8)
    vox[rows[:, 0], rows[:, 1], rows[:, 2]] = label_remap()[sem]
    return vox
