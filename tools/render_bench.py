"""Times the rendered first-hit depth loss alone (ops.voxel_render_loss) on one GPU: 20 frames, C = 2 and C = 9, at the three scales
of the voxel head (factors 1, 2, 4 of the 192 x 192 x 64 grid), with the lidar's ray table at STRIDE 1 and 4 (65,536 and 16,384
rays).  The scene is synthetic - a ground slab under the sensor and boxes on it, shifted from frame to frame - and the logits
favour the label by a margin of 4 with unit noise: rays run on behind the first surface, as on an early checkpoint.  Prints one
JSON line per (C, factor, stride): the median, smallest and largest time of `--repeats` calls (device events around each call,
after `--warmup` untimed calls) of the forward alone (no_grad) and of forward + backward, the cell visits of the call (cells per
ray summed over rays and frames, from the device's own count) and, beside the times, the traffic floor: what the passes must
move at least, divided by `--tbps` (5 TB/s, what the project's streaming kernels reach) -
    label pass      labels read, brick words written; hit and t written                  F V + F V / 8 + 8 F R
    occupancy pass  logits read once, q and a written                                    F V (4 C + 8)
    march           q and a read once (every cell at most), rays, hit, t; D, t* written   8 F V + 28 R + 8 F R + 12 F R
    finish          -
    backward        the occupancy pass again, the accumulator cleared and read,          F V (4 C + 8) + 16 F V
                    q and a read once, one 8-byte atomic per visit (an upper bound of    8 F V + 8 visits
                    the traffic: a wave sums neighbouring lanes in one cell first),
                    logits read and dlogits written by the dense pass                    8 F C V
`--step`: compute_loss + backward on synthetic tensors with the shapes of one base_1d step (20 frames, 2 classes), voxel head only,
with LOSSES.VOXEL_RENDER absent and with WEIGHT 0.5 and FACTORS [1, 2, 4], [2, 4], [4] at STRIDE 1, and [1, 2, 4] at STRIDE 4: the
cost per factor list in a step.

    python tools/render_bench.py [--frames 20] [--classes 2 9] [--factors 1 2 4] [--strides 1 4] [--warmup 3] [--repeats 10] [--step]

DESIGN.md section 12 records the figures of one MI355X."""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))

GRID = (192, 192, 64)


def scene(seed=0):
    """(192, 192, 64) uint8: a ground slab up to 2 cells under the sensor's height minus 10, 80 boxes on it, free around the sensor"""
    rng = np.random.default_rng(seed)
    g = np.zeros(GRID, np.uint8)
    g[:, :, :10] = 1
    for _ in range(80):
        x, y = rng.integers(0, 180, 2)
        g[x:x + rng.integers(3, 14), y:y + rng.integers(3, 14), 10:rng.integers(14, 44)] = rng.integers(1, 9)
    g[30:44, 90:102, 10:] = 0
    return g


def inputs(frames, C, factor, dev, seed=0):
    """logits (1, frames, C, X, Y, Z) with requires_grad and labels (1, frames, 1, X, Y, Z) uint8 at scale `factor`"""
    base = torch.from_numpy(scene(seed)[::factor, ::factor, ::factor].copy()).to(dev)
    base = torch.where(base == 0, base, (base - 1) % (C - 1) + 1)
    labels = torch.stack([torch.roll(base, shifts=(k, -2 * k), dims=(0, 1)) for k in range(frames)])
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    logits = torch.randn(frames, C, *base.shape, device=dev, generator=g)
    logits.scatter_add_(1, labels[:, None].long(), torch.full((frames, 1, *base.shape), 4.0, device=dev))
    return logits[None].contiguous().requires_grad_(True), labels[None, :, None].contiguous()


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def floor_bytes(F, C, V, R, visits):
    fwd = F * V + F * V // 8 + 8 * F * R + F * V * (4 * C + 8) + 8 * F * V + 28 * R + 20 * F * R
    both = fwd + F * V * (4 * C + 8) + 16 * F * V + 8 * F * V + 8 * visits + 8 * F * C * V
    return fwd, both


def step_times(args, dev):
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.trainer import WorldModelTrainer
    batch, output = {}, {}
    for f in (1, 2, 4):
        lg, lb = inputs(args.frames, 2, f, dev, seed=f)
        shape = lg.shape[3:]
        output[f'voxel_{f}'] = lg.detach().view(2, args.frames // 2, 2, *shape).requires_grad_(True)
        batch[f'voxel_label_{f}'] = lb.view(2, args.frames // 2, 1, *shape)
    base = {'EVAL.RGB_SUPERVISION': False, 'LIDAR_RE.ENABLED': False, 'SEMANTIC_SEG.ENABLED': False}
    for factors, stride in ((None, 1), ([1, 2, 4], 1), ([2, 4], 1), ([4], 1), ([1, 2, 4], 4)):
        extra = {} if factors is None else {'LOSSES.VOXEL_RENDER.WEIGHT': 0.5, 'LOSSES.VOXEL_RENDER.FACTORS': factors,
                                            'LOSSES.VOXEL_RENDER.STRIDE': stride}
        me = types.SimpleNamespace(cfg=base_1d_cfg(**base, **extra))

        def step():
            for v in output.values():
                v.grad = None
            ops.sum_scalars(list(WorldModelTrainer.compute_loss(me, batch, output).values())).backward()

        print(json.dumps({'compute_loss_backward': 'key absent' if factors is None else f'FACTORS {factors} STRIDE {stride}', 'frames': args.frames,
                          **timed(step, args.warmup, args.repeats)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--classes', type=int, nargs='+', default=[2, 9])
    ap.add_argument('--factors', type=int, nargs='+', default=[1, 2, 4])
    ap.add_argument('--strides', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--tbps', type=float, default=5.0)
    ap.add_argument('--step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_bench: needs a GPU (a CPU run says nothing about these times)')
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.voxel_view import render_table
    dev = torch.device('cuda:0')
    if args.step:
        return step_times(args, dev)
    cfg = base_1d_cfg()
    for C in args.classes:
        for factor in args.factors:
            logits, labels = inputs(args.frames, C, factor, dev)
            shape = tuple(int(n) for n in logits.shape[3:])
            V = shape[0] * shape[1] * shape[2]
            for stride in args.strides:
                rays, n_valid = render_table(cfg, factor, stride, shape, dev)
                R = int(rays.shape[0])

                def both():
                    logits.grad = None
                    ops.voxel_render_loss(logits, labels, rays, n_valid, 0.5)[0].backward()

                def forward():
                    with torch.no_grad():
                        ops.voxel_render_loss(logits, labels, rays, n_valid, 0.5)

                fb = timed(both, args.warmup, args.repeats)
                fw = timed(forward, args.warmup, args.repeats)
                cells = ops.voxel_render_parts(logits, labels, rays, n_valid)[4]
                visits = int(cells.clamp(min=0).sum())
                f_fwd, f_both = floor_bytes(args.frames, C, V, R, visits)
                print(json.dumps({'C': C, 'factor': factor, 'stride': stride, 'V': V, 'rays': R, 'valid_rays': n_valid, 'frames': args.frames, 'fwd': fw,
                                  'fwd_bwd': fb, 'visits': visits, 'cells_per_ray': round(visits / max(1, args.frames * n_valid), 1),
                                  'gvisits_per_s_bwd': round(visits / max(1e-9, (fb['median_ms'] - fw['median_ms']) * 1e-3) / 1e9, 2),
                                  'floor_fwd_ms': round(f_fwd / (args.tbps * 1e12) * 1e3, 4),
                                  'floor_fwd_bwd_ms': round(f_both / (args.tbps * 1e12) * 1e3, 4)}), flush=True)
            del logits, labels
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
