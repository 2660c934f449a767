"""Golden fixture of the voxel-label generator (muvo_amd.input_pipeline.depth_lidar_voxels): the REAL reference functions
depth2pcd, convert_coor_img, convert_coor_lidar and voxel_filter (data/data_preprocessing.py) on the deterministic frame of
muvo_amd/data/voxelize_inputs.py; only the glue of read_img / merge_pcd (decode the depth code, concatenate, ego mask) is
restated here.  Writes tests/golden/voxelize.npz: the uint16 rows the reference would np.save, for the dataset's parameter set
and for the one of the shipped data_preprocess.yaml, plus the constants used.  The inputs are not stored.

Usage: python tools/golden/make_golden_voxelize.py --reference DIR      (a checkout of the reference; development machine only)
The file is written with fixed zip time stamps, so a second run reproduces it byte for byte.
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, REPO)

from muvo_amd.data.voxelize_inputs import frame_case  # noqa: E402

CAMERA_POSITION, LIDAR_POSITION, FOV, SIZE = [1.0, 0.0, 2.0], [1.0, 0.0, 2.0], 110, [192, 192, 64]
SETS = {'dataset': (0.2, [-64 * 0.2, 0, -20 * 0.2]),          # bev_offset_forward * bev_resolution, 0, offset_z * voxel_resolution
        'preprocess_yaml': (0.5, [0.0, 0, -10.0])}


def tie_count(pcd, sem, res, size, offset):
    """Voxels whose two smallest distances are equal while the two points carry different tags: which one the reference
    takes there is an accident of its unstable argsort, so the fixture must contain none."""
    size = np.asarray(size)
    b = pcd + (np.asarray(offset, dtype=np.float64) + res * size / 2)
    idx = ((0 <= b) & (b < size * res)).all(axis=1)
    b, s = b[idx], sem[idx].squeeze()
    hx, hm = np.divmod(b, res)
    h = (hx[:, 0] + hx[:, 1] * size[0] + hx[:, 2] * size[0] * size[1]).astype(np.int64)
    d = (hm ** 2).sum(1)
    o = np.lexsort((d, h))
    h, d, s = h[o], d[o], s[o]
    first = np.r_[True, h[1:] != h[:-1]]
    # all points of a voxel at its smallest distance must agree on the tag: compare every point with the voxel's first
    start = np.maximum.accumulate(np.where(first, np.arange(len(h)), 0))
    tie = (d == d[start]) & (s != s[start])
    return int(idx.sum()), int(first.sum()), int(np.unique(h[tie]).size)


def write_npz(path, arrays):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order='C'), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refimport', 'stubs'))          # cv2 is imported by data_preprocessing
    from data.data_preprocessing import (EGO_VEHICLE_DIMENSION, convert_coor_img, convert_coor_lidar, depth2pcd, voxel_filter)
    rgba, pts, tag = frame_case()
    # read_img (cv2 gives B, G, R, A; PIL R, G, B, A: the depth code is 65536 R + 256 G + B either way)
    dc = rgba[..., :3].astype(float)
    depth = 1000 * ((256 ** 2 * dc[..., 0] + 256 * dc[..., 1] + dc[..., 2]) / (256 ** 3 - 1))
    # merge_pcd
    img_pcd, img_sem = depth2pcd(depth, rgba[..., 3], FOV)
    img_pcd = convert_coor_img(img_pcd, CAMERA_POSITION)
    lidar_pcd = convert_coor_lidar(pts.copy(), LIDAR_POSITION)
    pcd = np.concatenate([img_pcd, lidar_pcd], axis=0)
    sem = np.concatenate([img_sem, tag[:, None]], axis=0)
    x, y, z = EGO_VEHICLE_DIMENSION
    box = np.array([[-x / 2, -y / 2, 0], [x / 2, y / 2, z]])
    ego = ((box[0] < pcd) & (pcd < box[1])).all(axis=1)
    sem, pcd = sem[~ego], pcd[~ego]
    out = {'camera_position': np.asarray(CAMERA_POSITION), 'lidar_position': np.asarray(LIDAR_POSITION), 'fov': np.asarray(FOV),
           'voxel_size': np.asarray(SIZE), 'ego': np.asarray(EGO_VEHICLE_DIMENSION)}
    for name, (res, offset) in SETS.items():
        n_in, n_vox, n_tie = tie_count(pcd, sem, res, SIZE, offset)
        assert n_tie == 0, f'{name}: {n_tie} voxels with an exact distance tie between different tags - change the scene'
        voxels, semantics = voxel_filter(pcd, sem, res, SIZE, list(offset))          # voxelize_one
        rows = np.concatenate([voxels, semantics[:, None]], axis=1)
        assert rows.dtype == np.uint16 and len(rows) == n_vox
        print(f'{name}: res {res} offset {list(offset)}: {len(pcd)} points, {n_in} in the grid, {len(rows)} voxels, '
              f'{int((semantics == 6).sum())} road-line voxels')
        out[f'rows_{name}'] = rows
        out[f'resolution_{name}'] = np.asarray(res)
        out[f'offset_{name}'] = np.asarray(offset, dtype=np.float64)
    path = os.path.join(REPO, 'tests', 'golden', 'voxelize.npz')
    write_npz(path, out)
    print('wrote tests/golden/voxelize.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
