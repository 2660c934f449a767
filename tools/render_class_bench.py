"""Times the rendered first-hit class loss alone (ops.voxel_render_class_loss) on one GPU, in the shape of tools/render_bench.py and
on its synthetic scene (imported from it): 20 frames, C = 2 and C = 9, at the three scales of the voxel head (factors 1, 2, 4 of
the 192 x 192 x 64 grid), with the lidar's ray table at STRIDE 1 and 4 (65,536 and 16,384 rays).  Prints one JSON line per
(C, factor, stride): the median, smallest and largest time of `--repeats` calls (device events around each call, after `--warmup`
untimed calls) of the forward alone (no_grad) and of forward + backward, the workspace bytes of the call, the cell visits (cells
per ray summed over rays and frames, from the device's own count) and, beside the times, the traffic floor: what the passes must
move at least, divided by `--tbps` (5 TB/s, what the project's streaming kernels reach) -
    label pass        labels read, brick words written; hit and t written               F V + F V / 8 + 8 F R
    probability pass  logits read once, the C probabilities written                     8 C F V
    march             q and p_y of every cell at most once, rays, hit, the label's      8 F V + 28 R + 5 F R + 12 F R
                      byte; S and y written
    finish            -
    backward          the probability pass again, the accumulator cleared and read,     8 C F V + 16 C F V
                      q and p_y read once, one 8-byte atomic per visit at least (a      8 F V + 8 visits
                      visit issues up to two; a wave sums neighbouring lanes first),
                      logits read and dlogits written by the dense pass                 8 C F V
`--step`: compute_loss + backward on synthetic tensors with the shapes of one base_1d step (20 frames, `--step-classes` classes),
voxel head only, with LOSSES.VOXEL_RENDER_CLASS absent and with WEIGHT 0.5 and FACTORS [1, 2, 4], [2, 4], [4] at STRIDE 1, and
[1, 2, 4] at STRIDE 4: the cost per factor list in a step.

    python tools/render_class_bench.py [--frames 20] [--classes 2 9] [--factors 1 2 4] [--strides 1 4] [--warmup 3] [--repeats 10]
                                       [--step [--step-classes 2]]

DESIGN.md section 14 records the figures of one MI355X."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from render_bench import inputs, timed  # noqa: E402


def floor_bytes(F, C, V, R, visits):
    fwd = F * V + F * V // 8 + 8 * F * R + 8 * C * F * V + 8 * F * V + 28 * R + 17 * F * R
    both = fwd + 8 * C * F * V + 16 * C * F * V + 8 * F * V + 8 * visits + 8 * C * F * V
    return fwd, both


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
    for factors, stride in ((None, 1), ([1, 2, 4], 1), ([2, 4], 1), ([4], 1), ([1, 2, 4], 4)):
        extra = {} if factors is None else {'LOSSES.VOXEL_RENDER_CLASS.WEIGHT': 0.5, 'LOSSES.VOXEL_RENDER_CLASS.FACTORS': factors,
                                            'LOSSES.VOXEL_RENDER_CLASS.STRIDE': stride}
        me = types.SimpleNamespace(cfg=base_1d_cfg(**base, **extra))

        def step():
            for v in output.values():
                v.grad = None
            ops.sum_scalars(list(WorldModelTrainer.compute_loss(me, batch, output).values())).backward()

        print(json.dumps({'compute_loss_backward': 'key absent' if factors is None else f'FACTORS {factors} STRIDE {stride}', 'C': C,
                          'frames': args.frames, **timed(step, args.warmup, args.repeats)}), flush=True)


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
    ap.add_argument('--step-classes', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_class_bench: needs a GPU (a CPU run says nothing about these times)')
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
                    ops.voxel_render_class_loss(logits, labels, rays, n_valid, 0.5)[0].backward()

                def forward():
                    with torch.no_grad():
                        ops.voxel_render_class_loss(logits, labels, rays, n_valid, 0.5)

                fb = timed(both, args.warmup, args.repeats)
                fw = timed(forward, args.warmup, args.repeats)
                cells = ops.voxel_render_class_parts(logits, labels, rays, n_valid)[4]
                visits = int(cells.clamp(min=0).sum())
                f_fwd, f_both = floor_bytes(args.frames, C, V, R, visits)
                print(json.dumps({'C': C, 'factor': factor, 'stride': stride, 'V': V, 'rays': R, 'valid_rays': n_valid, 'frames': args.frames, 'fwd': fw,
                                  'fwd_bwd': fb, 'visits': visits, 'cells_per_ray': round(visits / max(1, args.frames * n_valid), 1),
                                  'ws_bytes': int(ops.lib().muvo_render_class_ws_bytes(ops._i64(args.frames), C, ops._i64(V), ops._i64(R))),
                                  'gvisits_per_s_bwd': round(visits / max(1e-9, (fb['median_ms'] - fw['median_ms']) * 1e-3) / 1e9, 2),
                                  'floor_fwd_ms': round(f_fwd / (args.tbps * 1e12) * 1e3, 4),
                                  'floor_fwd_bwd_ms': round(f_both / (args.tbps * 1e12) * 1e3, 4)}), flush=True)
            del logits, labels
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
