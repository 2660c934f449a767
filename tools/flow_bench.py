"""Times the optical flow behind the `_flow` panel on the GPU: `ops.optical_flow` over the label pairs of one base_1d test batch
and the whole panel (muvo_amd/flow.py: flow_panel) - b 2, s 10 of which 6 reconstructed, one imagined row, 320 x 832.
HIP events around back-to-back calls after a warm-up, three alternating windows, median (min .. max) per call.  The traffic
floor of a stencil is what it must move once: the poly expansion reads 1 float per pixel and frame and writes 5; an iteration
reads the flow (2), both frames' coefficients (10) and writes the flow (2).  No host figure for cv2 stands next to these:
cv2 is not a dependency and is not installed where this runs.

    python tools/flow_bench.py [--out profiles/flow_bench.txt] [--b 2] [--s 10] [--rf 6] [--size 320 832]
Per-kernel times: run the same command under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/flow_bench.py --calls 3`."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def frames(b, n, h, w, seed, dev):
    """(b, n, 3, h, w): a smooth random texture that drifts by a sub-pixel amount per frame"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(b, 1, 3, h // 8 + 4, w // 8 + 4, generator=g)
    out = []
    for t in range(n):
        theta = torch.tensor([[1.0, 0.0, 0.004 * t], [0.0, 1.0, -0.003 * t]]).repeat(b, 1, 1)
        grid = torch.nn.functional.affine_grid(theta, (b, 3, h, w), align_corners=False)
        up = torch.nn.functional.interpolate(coarse[:, 0], size=(h, w), mode='bicubic', align_corners=False).clamp(0, 1)
        out.append(torch.nn.functional.grid_sample(up, grid, mode='bilinear', padding_mode='border', align_corners=False))
    return torch.stack(out, dim=1).contiguous().to(dev)


def timed(fn, calls, windows=3):
    fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        z.record()
        z.synchronize()
        per.append(a.elapsed_time(z) / calls)
    return statistics.median(per), min(per), max(per)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--b', type=int, default=2)
    ap.add_argument('--s', type=int, default=10)
    ap.add_argument('--rf', type=int, default=6)
    ap.add_argument('--size', type=int, nargs=2, default=(320, 832))
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('flow_bench measures on the GPU: none found')
    from muvo_amd import ops
    from muvo_amd.flow import flow_panel
    dev = torch.device('cuda', 0)
    b, s, rf, (h, w) = args.b, args.s, args.rf, args.size
    label = frames(b, s, h, w, 1, dev)
    recon = frames(b, rf, h, w, 2, dev)
    imagine = frames(b, s - rf, h, w, 3, dev)
    batch, output, imagines = {'rgb_label_1': label}, {'rgb_1': recon}, [{'rgb_1': imagine}]
    stack = label.reshape(b * s, 3, h, w)
    first = [n * s + t - 1 for n in range(b) for t in range(1, s)]
    second = [i + 1 for i in first]
    P, N = len(first), h * w
    out = torch.empty(P, 2, h, w, device=dev)
    lines = [f'# optical flow of one base_1d test batch: b {b}, s {s} ({rf} reconstructed + {s - rf} imagined), 1 imagined row, {h} x {w}; '
             f'3 alternating windows of {args.calls} back-to-back calls, HIP events; median ms per call (min .. max)']
    t = timed(lambda: ops.optical_flow(stack, stack, first, second, out=out), args.calls)
    levels = 3
    sizes = [((h + ((1 << k) >> 1)) >> k) * ((w + ((1 << k) >> 1)) >> k) for k in range(levels)]
    floor = sum(4 * P * n * (2 * (1 + 5) + 3 * (2 + 10 + 2)) for n in sizes) + 4 * P * N * (2 * 3 + 2)
    lines.append(f'ops.optical_flow  {P} pairs   {t[0]:9.3f} ({t[1]:9.3f} .. {t[2]:9.3f})   {t[0] / P:7.3f} ms per pair; traffic floor of the stencils '
                 f'{floor / 1e6:.1f} MB -> {floor / t[0] / 1e6:.0f} GB/s achieved against it')
    t = timed(lambda: flow_panel(batch, output, imagines), args.calls)
    pairs = 2 * b * (s - 1)
    lines.append(f'flow_panel        {pairs} pairs   {t[0]:9.3f} ({t[1]:9.3f} .. {t[2]:9.3f})   panel {tuple(flow_panel(batch, output, imagines).shape)}')
    host = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    panel = flow_panel(batch, output, imagines)
    host[0].record()
    panel.cpu()
    host[1].record()
    host[1].synchronize()
    lines.append(f'panel to host                {host[0].elapsed_time(host[1]):9.3f}')
    lines.append('cv2.calcOpticalFlowFarneback on the host: not measured (cv2 is not installed where this runs)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
