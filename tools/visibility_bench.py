"""Times the sensor-visibility mask alone (ops.visibility_mark, ops.visibility_apply; csrc/visibility.hip) on one GPU at the shape
of a base_1d step: 20 frames of 192 x 192 x 64 and the pyramid's two coarser grids, with VOXEL_SEG.VISIBILITY's default table
(65,536 lidar rays + 300 x 480 camera rays) and, for the comparison with the rendered depth loss's forward march (DESIGN.md
section 12: the same walk, the lidar's 65,536 rays), the lidar rows alone.  Labels:
    synthetic   the voxel tensor of muvo_amd/data/synthetic.py (10 % of the cells occupied at random: rays end after ~10 cells)
    recording   what generate_voxels makes of the test recording's depth images and lidar sweeps (muvo_amd/data/
                recording_inputs.py through input_pipeline.depth_lidar_voxels): a shell of visible surfaces, rays run long
    free        no occupied cell: every ray walks to its exit - the cells the rendered depth loss marches
Each row is one JSON line: ms per call of the bricks pass, the mark and the apply, each the mean over a window of at least
`--window` seconds between two device events (after `--warmup` untimed calls); the unknown share and the seen-free share from the
device's counts; the SEEN bits set; and the atomics of the mark - 8 bytes each, one per run of consecutive cells of a ray in one
brick - ESTIMATED by walking every `--sample`-th ray of the first frame on the host (numpy, the walk of the tests) and scaling.

    python tools/visibility_bench.py [--frames 20] [--factors 1 2 4] [--labels synthetic recording free] [--window 1.0] [--sample 16]

DESIGN.md section 13 records the figures of one MI355X."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
GRID = (192, 192, 64)


def labels_of(kind, frames, dev):
    """(frames, 192, 192, 64) uint8 on the device"""
    if kind == 'free':
        return torch.zeros((frames, *GRID), dtype=torch.uint8, device=dev)
    if kind == 'synthetic':
        from muvo_amd.data.synthetic import make_batch
        return make_batch(1, frames, seed=1234, image_hw=(8, 8), route_hw=(8, 8), range_hw=(8, 8), voxel=GRID, device=dev)['voxel'].view(frames, *GRID).contiguous()
    from muvo_amd import input_pipeline as IP
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.data import recording_inputs as RI
    cfg = base_1d_cfg()
    res = float(cfg.VOXEL.RESOLUTION)
    offset = [(int(e) - s // 2) * res for e, s in zip(cfg.VOXEL.EV_POSITION, GRID)]
    out = []
    todo = [(split, town, run, t) for split, town, run, n, ok in RI.RUNS if ok for t in range(n)]
    for split, town, run, t in todo[:frames]:
        fr = RI.frame_arrays(split, town, run, t)
        out.append(IP.depth_lidar_voxels(torch.from_numpy(fr['depth_semantic']).to(dev), torch.from_numpy(fr['points_xyz']).to(dev),
                                         torch.from_numpy(fr['ObjTag']).to(dev), camera_position=list(cfg.IMAGE.CAMERA_POSITION),
                                         lidar_position=list(cfg.POINTS.LIDAR_POSITION), fov=float(cfg.IMAGE.FOV), voxel_resolution=res,
                                         voxel_size=list(GRID), offset=offset, dense=True)[0])
    while len(out) < frames:
        out.append(out[len(out) % len(todo)])
    return torch.stack(out).contiguous()


def window_ms(fn, warmup, window):
    """mean ms per call over a window of at least `window` seconds between two device events"""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    n = max(10, int(window * 1e3 / max(a.elapsed_time(b), 1e-3) * 1.1) + 1)
    while True:
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window * 1e3:
            return round(ms / n, 5), n
        n *= 2


def host_atomics(grid, rays, sample):
    """the mark's atomics for one frame, from every `sample`-th ray walked on the host: (atomics, cells marked), scaled by `sample`"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import render_reference as RR
    X, Y, Z = grid.shape
    BY, BZ = (Y + 3) // 4, (Z + 3) // 4
    cells = RR.cell_table(grid.shape, rays[::sample])['cells']
    flat = grid.reshape(-1)
    inside = cells >= 0
    occ = inside & (flat[np.maximum(cells, 0)] != 0)
    marked = inside & (np.cumsum(occ, 1) - occ == 0)
    c = np.maximum(cells, 0)
    x, y, z = c // (Y * Z), (c // Z) % Y, c % Z
    brick = ((x >> 2) * BY + (y >> 2)) * BZ + (z >> 2)
    first = np.ones_like(marked)
    first[:, 1:] = brick[:, 1:] != brick[:, :-1]
    return int((marked & first).sum()) * sample, int(marked.sum()) * sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--factors', type=int, nargs='+', default=[1, 2, 4])
    ap.add_argument('--labels', nargs='+', default=['synthetic', 'recording', 'free'])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--sample', type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('visibility_bench: needs a GPU (a CPU run says nothing about these times)')
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.voxel_view import lidar_rays, visibility_table
    dev = torch.device('cuda:0')
    cfg = base_1d_cfg()
    cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True})
    n_lidar = len(lidar_rays(cfg, 1))
    for kind in args.labels:
        full = labels_of(kind, args.frames, dev)
        for factor in args.factors:
            label = full if factor == 1 else ops.resize_nearest(full, tuple(n // factor for n in GRID))
            shape = tuple(int(n) for n in label.shape[1:])
            table = visibility_table(cfg, factor, shape, dev)
            for name, rays in (('lidar+camera', table), ('lidar', table[:n_lidar].contiguous())):
                grid, bricks = ops.raycast_bricks(label)
                seen = ops.visibility_mark(grid, bricks, rays)
                _, counts = ops.visibility_apply(grid, seen)
                free_seen, unknown = (int(v) for v in counts.tolist())
                bits = int(sum(bin(int(w) & 0xffffffffffffffff).count('1') for w in seen.view(-1).cpu().tolist())) if seen.numel() <= 1 << 22 else -1
                acc = torch.zeros(2, dtype=torch.int64, device=dev)
                t_bricks, _ = window_ms(lambda: ops.raycast_bricks(label), args.warmup, args.window)
                t_mark, n_mark = window_ms(lambda: ops.visibility_mark(grid, bricks, rays), args.warmup, args.window)
                t_apply, _ = window_ms(lambda: ops.visibility_apply(grid, seen, acc), args.warmup, args.window)
                atomics, marked = host_atomics(label[0].cpu().numpy(), rays.cpu().numpy(), args.sample)
                V = shape[0] * shape[1] * shape[2]
                print(json.dumps({'labels': kind, 'factor': factor, 'grid': list(shape), 'frames': args.frames, 'table': name, 'rays': int(rays.shape[0]),
                                  'bricks_ms': t_bricks, 'mark_ms': t_mark, 'apply_ms': t_apply, 'calls_in_mark_window': n_mark,
                                  'unknown_share': round(unknown / (V * args.frames), 4), 'seen_free_share': round(free_seen / (V * args.frames), 4),
                                  'seen_bits': bits, 'est_cells_marked_per_call': marked * args.frames, 'est_atomics_per_call': atomics * args.frames,
                                  'est_atomic_bytes_per_call': 8 * atomics * args.frames,
                                  'apply_bytes': args.frames * (2 * V + V // 8)}), flush=True)


if __name__ == '__main__':
    main()
