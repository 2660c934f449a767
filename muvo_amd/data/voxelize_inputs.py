"""Deterministic raw inputs of the voxel-label generator (input_pipeline.depth_lidar_voxels) for fixtures and tests: a
depth+semantic camera image as the recorder's PNG holds it (R, G, B = 24-bit depth code, A = CARLA tag) and the full lidar
sweep of lidar_inputs.lidar_case."""
import numpy as np

from ..utils import detinit
from .lidar_inputs import lidar_case


def camera_frame(H=600, W=960, fov=110, key='voxelize_frame'):
    """uint8 (H, W, 4): a ground plane 2 m below the camera, walls at 12-42 m in 40-pixel columns, sky above (depth code of
    1000 m = invalid, and a band of far wall beyond the range filter), road-line stripes (tag 6), 2 % random tags in [0, 22];
    depth quantised to the 24-bit code, so many neighbouring pixels share a voxel."""
    k = detinit.name_key(key)
    f = W / (2.0 * np.tan(fov * np.pi / 360.0))
    yy, xx = np.mgrid[0:H, 0:W]
    z = np.full((H, W), 1000.0)
    g = yy > H / 2 + 4
    z[g] = 2.0 * f / (yy[g] - H / 2.0)
    wall = 12.0 + 30.0 * detinit.uniform_01(k + 1, W // 40 + 1)[xx // 40]
    sky = (~g) & (yy < H / 2 - 60)
    zz = np.minimum(z, wall)
    zz[sky] = 1000.0
    sem = np.where(z <= wall, 7, 1).astype(np.uint8)
    sem[(z <= wall) & ((xx // 6) % 23 == 0)] = 6
    sem[sky] = 13
    rnd = detinit.hash_u64(k + 2, H * W).reshape(H, W)
    pick = (rnd % np.uint64(50)) == 0
    sem[pick] = (rnd[pick] // np.uint64(50) % np.uint64(23)).astype(np.uint8)
    code = np.clip(np.round(zz / 1000.0 * (256 ** 3 - 1)), 0, 256 ** 3 - 1).astype(np.int64)
    return np.stack([code >> 16, (code >> 8) & 255, code & 255, sem], axis=-1).astype(np.uint8)


def frame_case(H=600, W=960, P=60000, fov=110, key='voxelize_frame', lidar_key='lidar_full'):
    """(depth_semantic uint8 (H, W, 4), points_xyz float32 (P, 3) in the lidar frame, ObjTag uint8 (P,))."""
    pts, tag = lidar_case(P=P, key=lidar_key)
    return camera_frame(H, W, fov, key), pts, tag
