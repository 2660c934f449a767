"""Voxel labels of recorded runs, on the GPU: what the reference's data/generate_voxels.py does offline on a CPU pool.

    python -m muvo_amd.generate_voxels --root DIR [--config-file YML] [--fov 110] [--frames-per-call N] [--overwrite]

Walks DIR/**/Town*/*/ (one directory per recorded run), reads pd_dataframe.pkl, per frame the `depth_semantic_path` PNG
(R, G, B = depth code, A = CARLA tag) and the `points_semantic_path` .npy (pickled dict with `points_xyz`, `ObjTag`), and
writes voxel/voxel_<9 digits>.npy as uint16 (Q, 4) rows x, y, z, tag plus the `voxel_path` column of the data frame
(generate_voxels.py:110-164).  Geometry from the project's config: VOXEL.RESOLUTION, VOXEL.SIZE,
offset = (VOXEL.EV_POSITION - VOXEL.SIZE // 2) * resolution, IMAGE.CAMERA_POSITION, POINTS.LIDAR_POSITION.
Unlike the reference it does not delete an existing voxel/ directory unless --overwrite is given.
The work per frame on the device is well below a millisecond; the run is bound by PNG decoding on the host."""
import argparse
import re
import shutil
import sys
from pathlib import Path

import numpy as np
import torch

from . import input_pipeline as IP
from .config import get_cfg


def geometry_from_cfg(cfg, fov=110):
    """Keyword arguments of input_pipeline.depth_lidar_voxels from the config.  The integers are subtracted first:
    [-64, 0, -20] * 0.2 = [-12.8, 0.0, -4.0] is the recording set-up's bev_offset_forward * bev_resolution and
    offset_z * voxel_resolution exactly (32 * 0.2 - 192 * 0.2 / 2 is -12.800000000000002, and the bins are compared exactly)."""
    size, res = [int(v) for v in cfg.VOXEL.SIZE], float(cfg.VOXEL.RESOLUTION)
    offset = [(int(e) - s // 2) * res for e, s in zip(cfg.VOXEL.EV_POSITION, size)]
    return dict(camera_position=list(cfg.IMAGE.CAMERA_POSITION), lidar_position=list(cfg.POINTS.LIDAR_POSITION), fov=fov,
                voxel_resolution=res, voxel_size=size, offset=offset)


def _load_frame(run, row):
    from PIL import Image
    depth_file, lidar_file = str(run.joinpath(row['depth_semantic_path'])), str(run.joinpath(row['points_semantic_path']))
    name, name_ = re.match(r'.*/.*_(\d{9})\.png', depth_file).group(1), re.match(r'.*/.*_(\d{9})\.npy', lidar_file).group(1)
    if name != name_:
        raise RuntimeError(f'file sequence is false: {depth_file} / {lidar_file}')
    img = np.asarray(Image.open(depth_file))
    if img.ndim != 3 or img.shape[2] != 4 or img.dtype != np.uint8:
        raise RuntimeError(f'{depth_file}: expected an 8-bit RGBA image, got {img.shape} {img.dtype}')
    sweep = np.load(lidar_file, allow_pickle=True).item()
    return name, img, np.asarray(sweep['points_xyz'], np.float32).reshape(-1, 3), np.asarray(sweep['ObjTag']).astype(np.uint8).reshape(-1)


def voxelize_run(run, geom, device, frames_per_call=8, overwrite=False, log=print):
    """One recorded run directory; returns the number of frames written."""
    import pandas as pd
    run = Path(run)
    pd_file = run / 'pd_dataframe.pkl'
    frame_table = pd.read_pickle(pd_file)
    save_path = run / 'voxel'
    if save_path.exists():
        if not overwrite:
            raise FileExistsError(f'{save_path} exists; pass --overwrite to replace it')
        shutil.rmtree(save_path)
    save_path.mkdir()
    voxel_paths = []
    for j0 in range(0, len(frame_table), frames_per_call):
        frames = [_load_frame(run, frame_table.iloc[j]) for j in range(j0, min(len(frame_table), j0 + frames_per_call))]
        if len({f[1].shape for f in frames}) != 1:
            raise RuntimeError(f'{run}: images of different sizes in one run')
        pmax = max(len(f[2]) for f in frames)
        pts, tag = np.zeros((len(frames), pmax, 3), np.float32), np.zeros((len(frames), pmax), np.uint8)
        for i, f in enumerate(frames):
            pts[i, :len(f[2])], tag[i, :len(f[3])] = f[2], f[3]
        rows = IP.depth_lidar_voxels(torch.from_numpy(np.stack([f[1] for f in frames])).to(device), torch.from_numpy(pts).to(device),
                                     torch.from_numpy(tag).to(device), [len(f[2]) for f in frames], frames_per_call=frames_per_call, **geom)
        for f, r in zip(frames, rows):
            file_name = f'{save_path.name}/voxel_{f[0]}.npy'
            np.save(run / file_name, r.cpu().numpy().astype(np.uint16))
            voxel_paths.append(file_name)
    frame_table['voxel_path'] = voxel_paths
    frame_table.to_pickle(pd_file)
    log(f'{run}: {len(voxel_paths)} frames, saved in {save_path}')
    return len(voxel_paths)


def main(argv=None):
    ap = argparse.ArgumentParser(description='voxel labels of recorded runs from depth images and lidar sweeps')
    ap.add_argument('--root', required=True, help='data root; every **/Town*/*/ below it is one run')
    ap.add_argument('--config-file', default='', help='YAML config (VOXEL.*, IMAGE.CAMERA_POSITION, POINTS.LIDAR_POSITION)')
    ap.add_argument('--fov', type=float, default=110, help='horizontal field of view of the depth camera in degrees')
    ap.add_argument('--frames-per-call', type=int, default=8)
    ap.add_argument('--overwrite', action='store_true', help='replace existing voxel/ directories')
    args = ap.parse_args(argv)
    cfg = get_cfg(argparse.Namespace(config_file=args.config_file, opts=[]))
    root = Path(args.root)
    runs = sorted(p for p in root.glob('**/Town*/*/') if p.is_dir())
    if not root.exists() or not runs:
        print('Root path does not exist or holds no Town*/*/ run directories', file=sys.stderr)
        return 1
    if not torch.cuda.is_available():
        print('generate_voxels needs a GPU (there is no CPU path)', file=sys.stderr)
        return 1
    if not args.overwrite:
        taken = [str(r / 'voxel') for r in runs if (r / 'voxel').exists()]
        if taken:
            print('refusing to replace existing voxel directories without --overwrite: ' + ', '.join(taken), file=sys.stderr)
            return 2
    geom = geometry_from_cfg(cfg, args.fov)
    for i, run in enumerate(runs):
        print(f'{i + 1}/{len(runs)} voxelizing {run}')
        voxelize_run(run, geom, torch.device('cuda'), max(1, args.frames_per_call), args.overwrite)
    return 0


if __name__ == '__main__':
    sys.exit(main())
