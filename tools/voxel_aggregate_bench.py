"""Times the fill of unobserved voxel-label cells from neighbouring frames (ops.voxel_pose_chain, ops.voxel_aggregate;
csrc/voxel_aggregate.hip) on one GPU at the shape of a base_1d step: 2 sequences of 10 frames of
192 x 192 x 64 and the pyramid's two coarser grids, under VOXEL_SEG.VISIBILITY's default ray table.  Three parts, each row one JSON
line:

  calls   ms per call of the chain and of the aggregate pass for WINDOW 1 / 4 / 9, next to muvo_visibility_apply on the same frames
          (the dense pass the aggregate kernel extends), each the mean over a window of at least `--window` seconds between two
          device events after `--warmup` untimed calls; the bytes the pass must move (label in, label out, the SEEN words) and what
          the gather adds at most (two 8-byte words per cell and slot looked at, counted on the host from the device's result).
          Labels: `synthetic` (muvo_amd/data/synthetic.py: 10 % of the cells occupied at random, frames unrelated) with the
          explicit poses of a car at 10 m/s in a slight curve, and `recording` (what generate_voxels makes of the test recording)
          with the same poses.
  shares  Voxel_Unknown_Share (single frame) against Voxel_Unknown_Share_Aggregated and Voxel_Filled_Share for WINDOW 1 / 4 / 9:
          synthetic labels with the explicit poses, the recording's labels with poses from ICP on its own range views
          (ICP_ITERATIONS 30, ICP_STRIDE 4, MIN_FITNESS 0.3), whose per-link fitness and status are printed too.
  step    WorldModelTrainer.training_step + backward + optimizer step as bench.py runs it, one process, the keys switched between
          windows of `--steps` steps after 3 untimed ones, `--rounds` rounds alternating: key absent, visibility alone,
          visibility + aggregation with ICP, visibility + aggregation with explicit poses (the difference is the ICP); and the ICP
          alone, queued as PreProcess queues it.

    python tools/voxel_aggregate_bench.py [--parts calls shares step] [--window 1.0] [--steps 20] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from visibility_bench import GRID, labels_of, window_ms  # noqa: E402

B, S = 2, 10
WINDOWS = (1, 4, 9)


def drive_poses(b, s):
    """(b, s - 1, 4, 4) float64: p_{t-1} = T_t p_t for a car that moves 1 m a frame along x and turns 1.5 degrees a frame"""
    a = np.radians(1.5)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [1.0, 0.02, 0.0]
    return torch.from_numpy(np.broadcast_to(T, (b, s - 1, 4, 4)).copy())


def recording_range_views(dev):
    """(B, S, 4, 64, 1024) float32: the range views of the test recording's first B S frames, metres"""
    from muvo_amd import input_pipeline as IP
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.data import recording_inputs as RI
    cfg = base_1d_cfg()
    todo = [(split, town, run, t) for split, town, run, n, ok in RI.RUNS if ok for t in range(n)]
    out = []
    for split, town, run, t in todo[:B * S]:
        fr = RI.frame_arrays(split, town, run, t)
        out.append(IP.range_projection(torch.from_numpy(fr['points_xyz']).to(dev), torch.from_numpy(fr['ObjTag']).to(dev),
                                       lidar_position=tuple(float(v) for v in cfg.POINTS.LIDAR_POSITION), fov=tuple(float(v) for v in cfg.POINTS.FOV),
                                       H=int(cfg.POINTS.CHANNELS), W=int(cfg.POINTS.HORIZON_RESOLUTION), with_seg=False)[0])
    return torch.stack(out).view(B, S, 4, *out[0].shape[-2:]).contiguous()


def part_calls_and_shares(args, dev, parts):
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.odometry import register_consecutive
    from muvo_amd.voxel_view import visibility_table
    cfg = base_1d_cfg()
    cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True})
    F = B * S
    explicit = drive_poses(B, S).to(dev).view(-1, 4, 4)
    for kind in args.labels:
        full = labels_of(kind, F, dev)
        poses = {'explicit': (explicit, None, None)}
        if kind == 'recording' and 'shares' in parts:
            rv = recording_range_views(dev)
            res = register_consecutive(rv / float(cfg.LIDAR_RE.SCALE), float(cfg.LIDAR_RE.SCALE), queued=True, max_iteration=30, source_stride=4)
            poses['icp'] = (res.T, res.fitness, res.status)
            print(json.dumps({'part': 'icp', 'labels': kind, 'fitness': [round(float(v), 3) for v in res.fitness.tolist()],
                              'status': res.status.tolist(), 'iterations': res.iterations.tolist()}), flush=True)
        for factor in args.factors:
            label = full if factor == 1 else ops.resize_nearest(full, tuple(n // factor for n in GRID))
            shape = tuple(int(n) for n in label.shape[1:])
            V = shape[0] * shape[1] * shape[2]
            grid, bricks = ops.raycast_bricks(label)
            seen = ops.visibility_mark(grid, bricks, visibility_table(cfg, factor, shape, dev))
            _, single = ops.visibility_apply(grid, seen)
            unknown = int(single[1])
            acc2 = torch.zeros(2, dtype=torch.int64, device=dev)
            t_apply = window_ms(lambda: ops.visibility_apply(grid, seen, acc2), args.warmup, args.window)[0] if 'calls' in parts else None
            for source, (T, fitness, status) in poses.items():
                for window in WINDOWS:
                    cell_map = ops.voxel_cell_map(cfg, factor)
                    mats, usable = ops.voxel_pose_chain(T, B, S, window, cell_map, fitness, status, 0.3)
                    _, counts = ops.voxel_aggregate(grid, bricks, seen, S, mats, usable)
                    occ, free, still = (int(v) for v in counts.tolist())
                    row = {'part': 'shares', 'labels': kind, 'poses': source, 'factor': factor, 'grid': list(shape), 'frames': F, 'window': window,
                           'usable_slots': int(usable.sum()), 'slots': int(usable.numel()),
                           'unknown_share': round(unknown / (V * F), 4), 'unknown_share_aggregated': round(still / (V * F), 4),
                           'filled_share': round((occ + free) / (V * F), 4), 'filled_occupied_share': round(occ / (V * F), 5)}
                    if 'calls' in parts and source == 'explicit':
                        acc3 = torch.zeros(3, dtype=torch.int64, device=dev)
                        t_chain = window_ms(lambda: ops.voxel_pose_chain(T, B, S, window, cell_map, fitness, status, 0.3), args.warmup, args.window)[0]
                        t_agg, n_agg = window_ms(lambda: ops.voxel_aggregate(grid, bricks, seen, S, mats, usable, acc3), args.warmup, args.window)
                        dense = F * (2 * V + V // 8)                              # label in, label out, the SEEN words
                        row.update({'part': 'calls', 'chain_ms': t_chain, 'aggregate_ms': t_agg, 'calls_in_window': n_agg, 'apply_ms': t_apply,
                                    'ratio_to_apply': round(t_agg / t_apply, 2), 'dense_bytes': dense,
                                    'dense_floor_ms_at_8TBs': round(dense / 8e12 * 1e3, 4),
                                    'aggregate_GBs_of_dense_bytes': round(dense / (t_agg * 1e-3) / 1e9, 1)})
                    print(json.dumps(row), flush=True)


def part_step(args, dev):
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.data.synthetic import make_batch
    from muvo_amd.odometry import register_consecutive
    from muvo_amd.trainer import WorldModelTrainer
    cfg = base_1d_cfg(RECEPTIVE_FIELD=6, FUTURE_HORIZON=S - 6, BATCHSIZE=B, STEPS=100000)
    torch.manual_seed(1234)
    tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    tr.train()
    opts, scheds = tr.configure_optimizers()
    opt, sched = opts[0], scheds[0]['scheduler']
    batches = [make_batch(B, S, seed=1234 + k, device=dev) for k in range(2)]
    poses = drive_poses(B, S).to(dev)
    node = type(tr.cfg)

    def set_keys(kind):
        tr.cfg.VOXEL_SEG.pop('VISIBILITY', None)
        tr.cfg.VOXEL_SEG.pop('AGGREGATE', None)
        if kind != 'absent':
            tr.cfg.VOXEL_SEG['VISIBILITY'] = node({'ENABLED': True})
        if kind.startswith('aggregate'):
            tr.cfg.VOXEL_SEG['AGGREGATE'] = node({'ENABLED': True})

    def step(i, kind):
        batch = dict(batches[i % 2])
        if kind == 'aggregate_explicit':
            batch['voxel_ego_poses'] = poses
        opt.zero_grad()
        loss = tr.training_step(batch, i)
        loss.backward()
        tr.on_after_backward()
        opt.step()
        sched.step()

    kinds = ('absent', 'visibility', 'aggregate_icp', 'aggregate_explicit')
    rows = {k: [] for k in kinds}
    i = 0
    for _ in range(args.rounds):
        for kind in kinds:
            set_keys(kind)
            for _ in range(3):
                step(i, kind)
                i += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(i, kind)
                i += 1
            torch.cuda.synchronize()
            rows[kind].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 2))
    set_keys('absent')
    rv = tr.preprocess(dict(batches[0]))['range_view_label_1']
    t_icp = window_ms(lambda: register_consecutive(rv, float(cfg.LIDAR_RE.SCALE), queued=True, max_iteration=30, source_stride=4), 2, args.window)[0]
    print(json.dumps({'part': 'step', 'batch': B, 'frames': S, 'steps': args.steps, 'ms_per_step': rows, 'icp_queued_ms': t_icp,
                      'icp_pairs': B * (S - 1), 'host_read_of_done': False}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['calls', 'shares', 'step'])
    ap.add_argument('--labels', nargs='+', default=['synthetic', 'recording'])
    ap.add_argument('--factors', type=int, nargs='+', default=[1, 2, 4])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('voxel_aggregate_bench: needs a GPU (a CPU run says nothing about these times)')
    dev = torch.device('cuda:0')
    if 'calls' in args.parts or 'shares' in args.parts:
        part_calls_and_shares(args, dev, args.parts)
    if 'step' in args.parts:
        part_step(args, dev)


if __name__ == '__main__':
    main()
