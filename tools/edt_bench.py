"""Times the distance-transform unit alone (csrc/edt.hip through ops.voxel_edt, ops.voxel_boundary_loss and ops.voxel_cd_counts) on
one GPU, in the shape of tools/render_class_bench.py and on the synthetic scene of tools/render_bench.py: 20 frames, C = 2 and
C = 9, at the three scales of the voxel head (factors 1, 2, 4 of the 192 x 192 x 64 grid), truncated (the trainer's default
TRUNCATE_M = 4 m: 20 / 10 / 5 cells) and untruncated.  Prints one JSON line per measurement: the median, smallest and largest time
of `--repeats` calls (device events around each call, after `--warmup` untimed calls) and, beside the times, the traffic floor:
what the passes must move at least, divided by `--tbps` (5 TB/s, what the project's streaming kernels reach) -
    transform         z pass: the grid read, int32 written; y and x pass: int32 read and written      21 F V
    loss forward      the class grid of the prediction (logits read, grid and bricks written),       (4 C + 1 + 1/8) F V
                      two transforms, the dense pass: logits, labels, both transforms                 42 F V + (4 C + 9) F V
    loss backward     logits and labels and both transforms read, dlogits written                     (8 C + 9) F V
    metric            two transforms, the dense pass: both grids, both transforms                     42 F V + 10 F V
- and the min-adds of a transform: F V sum over the axes of min(2 r + 1, N), r^2 < cap.
`--step`: compute_loss + backward on synthetic tensors with the shapes of one base_1d step (20 frames, `--step-classes` classes),
voxel head only, with LOSSES.VOXEL_BOUNDARY absent and with WEIGHT 0.5 and FACTORS [1, 2, 4], [2, 4], [4]: the cost per factor
list in a step, and the size of the new terms beside `voxel_f` at these synthetic logits.

    python tools/edt_bench.py [--frames 20] [--classes 2 9] [--factors 1 2 4] [--warmup 3] [--repeats 10] [--step [--step-classes 2]]

DESIGN.md section 15 records the figures of one MI355X."""
import argparse
import json
import math
import os
import sys
import types

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from render_bench import inputs, timed  # noqa: E402


def min_adds(F, shape, cap):
    r = math.isqrt(max(0, min(cap, sum(n * n for n in shape)) - 1))
    return F * shape[0] * shape[1] * shape[2] * sum(min(2 * r + 1, n) for n in shape)


def step_times(args, dev):
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.trainer import WorldModelTrainer
    C = args.step_classes
    batch, output = {}, {}
    for f in (1, 2, 4):
        lg, lb = inputs(args.frames, C, f, dev, seed=f)
        shape = lg.shape[3:]
        output[f'voxel_{f}'] = lg.detach().view(2, args.frames // 2, C, *shape).requires_grad_(True)
        batch[f'voxel_label_{f}'] = lb.view(2, args.frames // 2, 1, *shape)
    base = {'EVAL.RGB_SUPERVISION': False, 'LIDAR_RE.ENABLED': False, 'SEMANTIC_SEG.ENABLED': False}
    for factors in (None, [1, 2, 4], [2, 4], [4]):
        extra = {} if factors is None else {'LOSSES.VOXEL_BOUNDARY.WEIGHT': 0.5, 'LOSSES.VOXEL_BOUNDARY.FACTORS': factors}
        me = types.SimpleNamespace(cfg=base_1d_cfg(**base, **extra))
        last = {}

        def step():
            for v in output.values():
                v.grad = None
            losses = WorldModelTrainer.compute_loss(me, batch, output)
            last.update(losses)
            ops.sum_scalars(list(losses.values())).backward()

        row = {'compute_loss_backward': 'key absent' if factors is None else f'FACTORS {factors}', 'C': C, 'frames': args.frames,
               **timed(step, args.warmup, args.repeats)}
        row['terms'] = {k: round(float(v.detach()), 6) for k, v in last.items() if k.startswith('voxel_')}
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--classes', type=int, nargs='+', default=[2, 9])
    ap.add_argument('--factors', type=int, nargs='+', default=[1, 2, 4])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--tbps', type=float, default=5.0)
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--step-classes', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('edt_bench: needs a GPU (a CPU run says nothing about these times)')
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg, voxel_boundary, voxel_boundary_cells
    dev = torch.device('cuda:0')
    if args.step:
        return step_times(args, dev)
    cfg = base_1d_cfg()
    F = args.frames

    def floor(nbytes):
        return round(nbytes / (args.tbps * 1e12) * 1e3, 4)
    for C in args.classes:
        for factor in args.factors:
            logits, labels = inputs(F, C, factor, dev)
            shape = tuple(int(n) for n in logits.shape[3:])
            V = shape[0] * shape[1] * shape[2]
            grid = labels.view(F, *shape)
            T = voxel_boundary_cells(cfg, voxel_boundary(cfg)[2], factor)
            full = sum(n * n for n in shape)
            if C == args.classes[0]:                     # the transform and the metric do not depend on C
                for name, cap in ((f'T={T}', T * T), ('untruncated', full)):
                    t = timed(lambda: ops.voxel_edt(grid, cap), args.warmup, args.repeats)
                    adds = min_adds(F, shape, cap)
                    print(json.dumps({'transform': name, 'factor': factor, 'V': V, 'frames': F, **t, 'floor_ms': floor(21 * F * V), 'min_adds': adds,
                                      'gadds_per_s': round(adds / (t['median_ms'] * 1e-3) / 1e9, 1)}), flush=True)
                pred = ops.raycast_bricks(logits.detach().view(F, C, *shape))[0]
                counts = torch.zeros(10, dtype=torch.int64, device=dev)
                sums = torch.zeros(2, dtype=torch.float64, device=dev)
                t = timed(lambda: ops.voxel_cd_counts(grid, pred, [25, 100, 400], counts, sums), args.warmup, args.repeats)
                print(json.dumps({'metric': 'voxel_cd_counts', 'factor': factor, 'V': V, 'frames': F, **t, 'floor_ms': floor(52 * F * V),
                                  'min_adds': 2 * min_adds(F, shape, full)}), flush=True)

            def both():
                logits.grad = None
                ops.voxel_boundary_loss(logits, labels, T, 0.5)[0].backward()

            def forward():
                with torch.no_grad():
                    ops.voxel_boundary_loss(logits, labels, T, 0.5)

            fb = timed(both, args.warmup, args.repeats)
            fw = timed(forward, args.warmup, args.repeats)
            f_fwd = int((4 * C + 1.125) * F * V + 42 * F * V + (4 * C + 9) * F * V)
            print(json.dumps({'loss': f'T={T}', 'C': C, 'factor': factor, 'V': V, 'frames': F, 'fwd': fw, 'fwd_bwd': fb, 'floor_fwd_ms': floor(f_fwd),
                              'floor_fwd_bwd_ms': floor(f_fwd + (8 * C + 9) * F * V), 'min_adds': 2 * min_adds(F, shape, T * T)}), flush=True)
            del logits, labels
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
