"""Times the Lovasz-softmax training loss alone (ops.voxel_lovasz_loss) on one GPU: 20 frames, C = 2 and C = 9, at the three
scales of the voxel head - V = 36,864 / 294,912 / 2,359,296 voxels (factors 4, 2, 1 of the 192 x 192 x 64 grid) - a tenth of the
voxels occupied and a tenth ignored.  Prints one JSON line per (C, V): the median, smallest and largest time of `--repeats`
calls (device events around each call, after `--warmup` untimed calls) of the forward alone (no_grad: no dlde written) and of
forward + backward, the key rate of the sort (F C V keys / forward time) and, beside them, the traffic floor: what the passes
must move at least, divided by `--tbps` (5 TB/s, what the project's streaming kernels reach) -
    key pass      logits read once, labels, keys + payload written                     F V (4 C + 1 + 8 C)
    4 sort passes keys + payload read once and written once per pass                   4 x 16 F C V
    ranking pass  keys + payload read, dlde written (with a backward)                  F C V (8 + 4)
    gradient pass logits, labels, dlde read, dlogits written                           F V (4 C + 1 + 4 C + 4 C)
(the histogram of each sort pass reads the keys once more and the foreground count the payload: 4 x 4 + 4 bytes per key that a
fused design would not move - they are NOT in the floor).
`--step`: compute_loss + backward on synthetic tensors with the shapes of one base_1d step (20 frames, 2 classes), voxel head only,
with LOSSES.VOXEL_LOVASZ absent and with WEIGHT 0.5 and FACTORS [1, 2, 4], [2, 4], [4]: the cost per factor in a step.

    python tools/lovasz_bench.py [--frames 20] [--classes 2 9] [--sizes 36864 294912 2359296] [--warmup 3] [--repeats 10] [--step]

DESIGN.md section 11 records the figures of one MI355X."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))


def inputs(frames, C, V, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = 2 * torch.randn(1, frames, C, V, 1, 1, generator=g)
    u = torch.rand(1, frames, 1, V, 1, 1, generator=g)
    labels = torch.zeros(1, frames, 1, V, 1, 1, dtype=torch.uint8)
    labels[u < 0.1] = 255
    occ = torch.randint(1, C, labels.shape, generator=g).to(torch.uint8)
    labels = torch.where((u >= 0.1) & (u < 0.2), occ, labels)
    return logits.to(dev).requires_grad_(True), labels.to(dev)


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


def floor_bytes(F, C, V):
    key = F * V * (4 * C + 1 + 8 * C)
    sort = 4 * 16 * F * C * V
    fwd = key + sort + 8 * F * C * V
    both = fwd + 4 * F * C * V + F * V * (12 * C + 1)
    return fwd, both


def step_times(args, dev):
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.trainer import WorldModelTrainer
    batch, output = {}, {}
    for f in (1, 2, 4):
        x, y, z = 192 // f, 192 // f, 64 // f
        lg, lb = inputs(args.frames, 2, x * y * z, dev, seed=f)
        output[f'voxel_{f}'] = lg.detach().view(2, args.frames // 2, 2, x, y, z).requires_grad_(True)
        batch[f'voxel_label_{f}'] = lb.view(2, args.frames // 2, 1, x, y, z)
    base ={'EVAL.RGB_SUPERVISION': False, 'LIDAR_RE.ENABLED': False, 'SEMANTIC_SEG.ENABLED': False}
    for factors in (None, [1, 2, 4], [2, 4], [4]):
        extra = {} if factors is None else {'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5, 'LOSSES.VOXEL_LOVASZ.FACTORS': factors}
        me = types.SimpleNamespace(cfg=base_1d_cfg(**base, **extra))

        def step():
            for v in output.values():
                v.grad = None
            ops.sum_scalars(list(WorldModelTrainer.compute_loss(me, batch, output).values())).backward()

        print(json.dumps({'compute_loss_backward': 'key absent' if factors is None else f'FACTORS {factors}', 'frames': args.frames,
                          **timed(step, args.warmup, args.repeats)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--classes', type=int, nargs='+', default=[2, 9])
    ap.add_argument('--sizes', type=int, nargs='+', default=[36864, 294912, 2359296])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--tbps', type=float, default=5.0)
    ap.add_argument('--step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lovasz_bench: needs a GPU (a CPU run says nothing about these times)')
    from muvo_amd import ops
    dev = torch.device('cuda:0')
    if args.step:
        return step_times(args, dev)
    for C in args.classes:
        for V in args.sizes:
            logits, labels = inputs(args.frames, C, V, dev)

            def both():
                logits.grad = None
                ops.voxel_lovasz_loss(logits, labels, 0.5)[0].backward()

            def forward():
                with torch.no_grad():
                    ops.voxel_lovasz_loss(logits, labels, 0.5)

            fb = timed(both, args.warmup, args.repeats)
            fw = timed(forward, args.warmup, args.repeats)
            keys = args.frames * C * V
            f_fwd, f_both = floor_bytes(args.frames, C, V)
            print(json.dumps({'C': C, 'V': V, 'frames': args.frames, 'fwd': fw, 'fwd_bwd': fb, 'keys': keys,
                              'gkeys_per_s': round(keys / (fw['median_ms'] * 1e-3) / 1e9, 2),
                              'floor_fwd_ms': round(f_fwd / (args.tbps * 1e12) * 1e3, 4),
                              'floor_fwd_bwd_ms': round(f_both / (args.tbps * 1e12) * 1e3, 4)}), flush=True)
            del logits, labels
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
