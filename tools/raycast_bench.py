"""Times the voxel ray casting behind the `_voxel` panel and the RayIoU metric on the GPU at the model's grid,
192 x 192 x 64 with 9 classes, over 20 frames: a synthetic street scene (ground, boxes, sparse clutter) as the label and logits
that favour the label's class by `--bias` over unit noise as the prediction, so the prediction is the label plus scattered
wrong cells - the hard case for the march, whose rays then stop at different depths inside one wave.
  (a)  occupancy bricks + class grid from logits, and bricks from a uint8 grid
  (b)  the march + shading of 20 tiles at R = 256, and one whole `_voxel` strip (b 2, s 10, rf 6, one imagined sample)
  (c)  ray_iou_counts over the 64 x 256 rays of stride 4, label against prediction
HIP events around back-to-back calls after a warm-up, five alternating windows, median (min .. max) per call.

    python tools/raycast_bench.py [--out profiles/raycast_bench.txt] [--frames 20] [--bias 4.0]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def street(F, X, Y, Z, seed, dev):
    """(F, X, Y, Z) uint8: class 1 ground of slowly varying height, boxes of the classes 2 .. 8, 0.2 % clutter"""
    g = torch.Generator().manual_seed(seed)
    grid = torch.zeros(F, X, Y, Z, dtype=torch.uint8)
    z = torch.arange(Z)
    for f in range(F):
        h = 4 + torch.nn.functional.interpolate(torch.rand(1, 1, 6, 6, generator=g) * 6, size=(X, Y), mode='bilinear', align_corners=False)[0, 0]
        grid[f][z[None, None, :] < h[:, :, None]] = 1
        for _ in range(40):
            x0, y0 = int(torch.randint(0, X - 24, (1,), generator=g)), int(torch.randint(0, Y - 24, (1,), generator=g))
            w, d, top = (int(torch.randint(4, 24, (1,), generator=g)) for _ in range(3))
            grid[f, x0:x0 + w, y0:y0 + d, 4:min(Z, 8 + 2 * top)] = int(torch.randint(2, 9, (1,), generator=g))
        clutter = torch.rand(X, Y, Z, generator=g) < 0.002
        grid[f][clutter] = 8
    return grid.to(dev)


def timed(fn, calls, windows=5):
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
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--bias', type=float, default=4.0)
    ap.add_argument('--size', type=int, nargs=3, default=(192, 192, 64))
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('raycast_bench measures on the GPU: none found')
    from muvo_amd import ops
    from muvo_amd.config import get_cfg
    from muvo_amd.visualise import VOXEL_COLOURS, _palette
    from muvo_amd.voxel_view import _camera, lidar_rays, voxel_panel
    dev = torch.device('cuda', 0)
    F, (X, Y, Z), C, R = args.frames, args.size, 9, args.tile
    label = street(F, X, Y, Z, 1, dev)
    logits = torch.randn(F, C, X, Y, Z, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    logits.scatter_add_(1, label.long().unsqueeze(1), torch.full((F, 1, X, Y, Z), args.bias, device=dev))
    lg, lb = ops.raycast_bricks(label)
    pg, pb = ops.raycast_bricks(logits)
    agree = float((pg == lg).float().mean())
    lines = [f'# voxel ray casting, {F} frames of {X} x {Y} x {Z}, {C} classes; label occupancy {float((lg != 0).float().mean()):.4f}, prediction occupancy '
             f'{float((pg != 0).float().mean()):.4f}, {agree:.4f} of the cells agree; library {os.path.basename(ops._LIB_PATH)}; 5 windows of {args.calls} '
             f'back-to-back calls, HIP events; median ms per call (min .. max)']

    def row(name, t, note=''):
        lines.append(f'{name:<46}{t[0]:9.3f} ({t[1]:9.3f} .. {t[2]:9.3f})   {note}')
    t = timed(lambda: ops.raycast_bricks(logits), args.calls)
    nbytes = logits.numel() * 4 + lg.numel() + lb.numel() * 8
    row('(a) bricks + class grid from logits', t, f'{nbytes / 1e6:.0f} MB moved once -> {nbytes / t[0] / 1e6:.0f} GB/s')
    t = timed(lambda: ops.raycast_bricks(label), args.calls)
    row('(a) bricks from a uint8 grid', t, f'{(lg.numel() + lb.numel() * 8) / t[0] / 1e6:.0f} GB/s')
    rays = _camera(X, Y, Z, R, dev)
    pal, _ = _palette(VOXEL_COLOURS, dev)
    T = R + 4
    panel = torch.empty((1, 3, T, F * T), dtype=torch.uint8, device=dev)
    place = ops.tile_place(panel, F, xstep=T)
    for name, g, b in (('label', lg, lb), ('prediction', pg, pb)):
        t = timed(lambda: ops.panel_voxel_view(g, b, rays, pal, panel, place, 2, 204), args.calls)
        hit = float((ops.raycast(g, b, rays)[0] >= 0).float().mean())
        row(f'(b) march + shading, {F} tiles of {R} x {R}, {name}', t, f'{F * R * R / t[0] / 1e6:.2f} G rays/s, {hit:.3f} of the rays hit')
    b_, s, rf = 2, F // 2, (F // 2) * 6 // 10
    shape5 = lambda x: x.reshape(b_, s, *x.shape[1:])                       # noqa: E731
    batch = {'voxel_label_1': shape5(label).unsqueeze(2)}
    output = {'voxel_1': shape5(logits)[:, :rf].contiguous()}
    imagines = [{'voxel_1': shape5(logits)[:, rf:].contiguous()}]
    t = timed(lambda: voxel_panel(None, batch, output, imagines, size=R), args.calls)
    row(f'(b) one `_voxel` strip: b {b_}, s {s}, rf {rf}, 1 imagined', t, f'panel {tuple(voxel_panel(None, batch, output, imagines, size=R).shape)}, bricks included')
    lrays = torch.from_numpy(lidar_rays(get_cfg(), 4)).to(dev)
    counts = torch.zeros((3, C, 3), dtype=torch.int64, device=dev)
    depth = torch.zeros(2, dtype=torch.float64, device=dev)
    t = timed(lambda: ops.ray_iou_counts(lg, lb, pg, pb, lrays, C, 0.2, counts, depth), args.calls)
    row(f'(c) ray_iou_counts, {lrays.shape[0]} rays x {F} frames x 2 grids', t, f'{2 * F * lrays.shape[0] / t[0] / 1e6:.2f} G rays/s')
    counts.zero_()
    depth.zero_()
    ops.ray_iou_counts(lg, lb, pg, pb, lrays, C, 0.2, counts, depth)
    from muvo_amd.voxel_view import ray_iou_from_counts
    means, _ = ray_iou_from_counts(counts.cpu().tolist())
    d = depth.cpu().tolist()
    lines.append(f'    RayIoU 1 / 2 / 4 m {means[0]:.4f} {means[1]:.4f} {means[2]:.4f}; depth L1 {d[0] / max(d[1], 1):.3f} m over {int(d[1])} rays; '
                 f'count checksum {int(counts.sum())}, panel checksum {int(panel.long().sum())}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
