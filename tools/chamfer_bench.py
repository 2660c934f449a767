"""Times the Chamfer-distance training loss alone (ops.chamfer_loss: forward + backward) on one GPU, at the three scales of the
lidar head - 20 frames of n = 4,096 / 16,384 / 65,536 points (factors 4, 2, 1 of the 64 x 1024 range view) - in the normal
and in the deterministic mode.  Prints one JSON line per (n, mode): the median, smallest and largest time of `--repeats`
forward + backward calls (device events around each call, after `--warmup` untimed calls), the same for the forward alone,
and the achieved pair rate 2 F n^2 / forward time (the search visits every pair once per direction).  A tenth of the target
points is (0, 0, 0), as label pixels without a lidar return are, so the backward scatter collides as it does on real labels.

    python tools/chamfer_bench.py [--frames 20] [--sizes 4096 16384 65536] [--warmup 3] [--repeats 10]

DESIGN.md section 10 records the figures of one MI355X."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))


def inputs(frames, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    pred = 2 * torch.rand(1, frames, 4, 1, n, generator=g) - 1
    target = 2 * torch.rand(1, frames, 4, 1, n, generator=g) - 1
    target[:, :, :, :, ::10] = 0.0
    return pred.to(dev).requires_grad_(True), target.to(dev)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--sizes', type=int, nargs='+', default=[4096, 16384, 65536])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('chamfer_bench: needs a GPU (a CPU run says nothing about these times)')
    from muvo_amd import ops
    dev = torch.device('cuda:0')
    was = ops.get_deterministic()
    try:
        for n in args.sizes:
            pred, target = inputs(args.frames, n, dev)

            def both():
                pred.grad = None
                ops.chamfer_loss(pred, target, 0.5)[0].backward()

            def forward():
                with torch.no_grad():
                    ops.chamfer_loss(pred, target, 0.5)

            for det in (False, True):
                ops.set_deterministic(det)
                fb = timed(both, args.warmup, args.repeats)
                fw = timed(forward, args.warmup, args.repeats)
                pairs = 2.0 * args.frames * n * n
                print(json.dumps({'n': n, 'frames': args.frames, 'mode': 'deterministic' if det else 'normal', 'fwd_bwd': fb, 'fwd': fw,
                                  'pairs': pairs, 'gpairs_per_s': round(pairs / (fw['median_ms'] * 1e-3) / 1e9, 2)}), flush=True)
    finally:
        ops.set_deterministic(was)


if __name__ == '__main__':
    main()
