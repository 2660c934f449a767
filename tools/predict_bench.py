"""Time of the two voxel-export routes of a prediction run (muvo_amd/predict.py) on the GPU, and of the
confusion counts behind the segmentation heads' IoU.

    python tools/predict_bench.py [--rounds 5] [--iters 50] [--host-iters 1] [--out profiles/predict_export.txt]
    (--host-iters 0: the kernel route only, e.g. under a kernel trace)
    python tools/predict_bench.py --what confusion [--rounds 5] [--iters 50] [--host-iters 3] [--out profiles/predict_confusion.txt]

Routes, on the same logits (F frames of C x 192 x 192 x 64 float32 on the device, about 10 % of the voxels occupied):
  kernels    ops.voxel_rows (csrc/export.hip: classify + count, scan, ordered compaction), the rows copied to the host.
             `device` is the three kernels alone between HIP events (ops.voxel_rows_into, a preallocated buffer, no host
             read), `to host` the whole call including the read of the counts and the copy of the rows, by the host clock
             around a device synchronise.
  host       the reference's route restated (sim_run.py:78-79): logits.cpu(), torch.argmax, torch.where, stack - by the host
             clock; `copy` is the .cpu() alone.  torch's CPU thread count is printed: it bounds argmax and where.
Warm-up first, then `--rounds` windows per route, the routes alternating; median (min .. max) over the windows of the
per-call mean.  The traffic floor of the kernel route is C * 4 B read + 1 B written and 1 B read per voxel + 8 B per row; its
share of the HBM peak is quoted for the `device` time only.  Before timing, the rows of both routes are compared once.

--what confusion: the three segmentation heads at their real sizes, 20 frames each (bird's-eye view 8 x 192 x 192, lidar
9 x 64 x 1024, camera 9 x 320 x 832 = the cropped image of base_1d), labels and predictions constant over 16 x 16 tiles, the
prediction equal to the label in about nine tiles of ten:
  kernel     muvo_seg_confusion alone between HIP events, adding into one buffer; traffic floor C * 4 + 1 bytes per pixel.
  update     JaccardIndex.update by the host clock: `queued` = calls back to back with one synchronise per window (how the
             evaluation loop runs it), `synced` = a synchronise after every call.
  reference  the reference's route restated (trainer.py:428-433 + the metric's update): torch.argmax on the device, prediction
             and label to the host, bincount of label * C + prediction there - by the host clock.
The counts of both routes are compared once before timing.

--what panels: the picture grids (muvo_amd/visualise.py, csrc/visualise.hip) of one base_1d test batch, b = 2 with
RECEPTIVE_FIELD + FUTURE_HORIZON frames and PREDICTION.N_SAMPLES imagined samples, random tensors at the real sizes (camera
3 x 320 x 832, range view 4 x 64 x 1024, voxels 2 x 192 x 192 x 64, route map 3 x 64 x 64), per head and all together:
    python tools/predict_bench.py --what panels [--rounds 5] [--iters 20] [--host-iters 1] [--out profiles/predict_panels.txt]
  device     render_panels between HIP events, calls back to back (allocation of the panels included).
  to host    render_panels and the copy of every panel to the host, by the host clock around a device synchronise.
  host       the reference's route restated: .cpu() of every source tensor, then tests/visualise_reference.render_panels - by
             the host clock; `copy` is the .cpu() calls alone.
`read` is the bytes of every source tensor once, `written` the bytes of the panels once; their sum over the `device` time is
quoted as a share of the HBM peak.  The panels of both routes are compared once before timing."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from muvo_amd import ops  # noqa: E402

HBM_PEAK_GBS = 8000.0           # MI355X, 8 TB/s
GRID = (192, 192, 64)
CASES = [(20, 2), (20, 9)]      # (frames, classes): the two-class head of base_1d, the nine-class head


def make_logits(F, C, dev, occupancy=0.10):
    """Class 0 wins everywhere except in a seeded `occupancy` share of the voxels, where one of the other classes does."""
    g = torch.Generator(device=dev).manual_seed(F * 100 + C)
    lg = torch.randn((F, C, *GRID), generator=g, device=dev)
    occ = torch.rand((F, *GRID), generator=g, device=dev) < occupancy
    lg[:, 0] = torch.where(occ, lg[:, 0] - 8.0, lg[:, 0] + 8.0)
    return lg


def kernels_to_host(lg):
    rows, counts = ops.voxel_rows(lg)
    return rows.cpu().numpy(), counts


def host_route(lg, timing=None):
    t0 = time.perf_counter()
    host = lg.cpu()
    t1 = time.perf_counter()
    am = torch.argmax(host, dim=1)
    f, x, y, z = torch.where(am != 0)
    rows = torch.stack([x, y, z, am[f, x, y, z]], 1).numpy()
    if timing is not None:
        timing.append(t1 - t0)
    return rows, torch.bincount(f, minlength=lg.shape[0]).tolist()


def wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def device_ms(lg, buf, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        ops.voxel_rows_into(lg, buf)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def fmt(t):
    return f'{statistics.median(t):10.3f} ({min(t):9.3f} .. {max(t):9.3f})'


CONFUSION_CASES = [('bev', 8, 192, 192), ('lidar', 9, 64, 1024), ('camera', 9, 320, 832)]
CONFUSION_FRAMES = 20


def make_head(F, C, H, W, dev, tile=16, agree=0.9):
    g = torch.Generator(device=dev).manual_seed(C * 1000 + H)
    th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
    label_t = torch.randint(0, C, (F, th, tw), generator=g, device=dev)
    other_t = torch.randint(0, C, (F, th, tw), generator=g, device=dev)
    pred_t = torch.where(torch.rand((F, th, tw), generator=g, device=dev) < agree, label_t, other_t)

    def up(t):
        return t.repeat_interleave(tile, 1).repeat_interleave(tile, 2)[:, :H, :W].contiguous()
    lg = torch.randn((F, C, H, W), generator=g, device=dev)
    lg.scatter_add_(1, up(pred_t).unsqueeze(1), torch.full((F, 1, H, W), 8.0, device=dev))
    return lg, up(label_t).to(torch.uint8).unsqueeze(1).contiguous()


def reference_confusion(lg, lb, C):
    pred = torch.argmax(lg, dim=1).view(-1).cpu()
    target = lb.view(-1).cpu()
    return torch.bincount(target.long() * C + pred, minlength=C * C)


def confusion_main(a):
    from muvo_amd.metrics import JaccardIndex, seg_confusion
    dev = torch.device('cuda')
    F = CONFUSION_FRAMES
    lines = [f'# confusion counts of the segmentation heads, {F} frames; {a.rounds} alternating windows; kernel / update: {a.iters} calls '
             f'per window, reference: {a.host_iters}; median ms per call (min .. max); torch CPU threads: {torch.get_num_threads()}']
    for name, C, H, W in CONFUSION_CASES:
        lg, lb = make_head(F, C, H, W, dev)
        counts = torch.zeros(C * C + 1, dtype=torch.int64, device=dev)
        seg_confusion(lg, lb, C, out=counts)
        want = reference_confusion(lg, lb, C)
        assert torch.equal(counts[:-1].cpu(), want) and int(counts[-1]) == 0, 'the two routes disagree'
        m = JaccardIndex(task='multiclass', num_classes=C, average='none')

        def kernel_ms(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                seg_confusion(lg, lb, C, out=counts)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        def synced():
            m.update(lg, lb)
            torch.cuda.synchronize()
        kernel_ms(3)
        wall(lambda: m.update(lg, lb), 3)
        wall(lambda: reference_confusion(lg, lb, C), 1)
        k_t, q_t, s_t, r_t = [], [], [], []
        for _ in range(a.rounds):
            k_t.append(kernel_ms(a.iters))
            q_t.append(wall(lambda: m.update(lg, lb), a.iters))
            s_t.append(wall(synced, a.iters))
            if a.host_iters:
                r_t.append(wall(lambda: reference_confusion(lg, lb, C), a.host_iters))
        floor = F * H * W * (4 * C + 1)
        med = statistics.median(k_t)
        first = len(lines)
        lines += [f'{name}  F {F}  C {C}  {H} x {W}  logits {4 * F * C * H * W / 1e6:.1f} MB  diagonal share {float(want.view(C, C).diag().sum()) / (F * H * W):.3f}',
                  f'  kernel              {fmt(k_t)}   traffic floor {floor / 1e6:.1f} MB -> {floor / med / 1e6:.0f} GB/s, '
                  f'{100 * floor / med / 1e6 / HBM_PEAK_GBS:.1f} % of the {HBM_PEAK_GBS / 1e3:.0f} TB/s HBM peak',
                  f'  update   queued     {fmt(q_t)}',
                  f'  update   synced     {fmt(s_t)}']
        if r_t:
            lines += [f'  reference           {fmt(r_t)}',
                      f'  reference / update synced = {statistics.median(r_t) / statistics.median(s_t):.0f}']
        for line in lines[first:]:
            print(line, flush=True)
        del lg, lb
    return lines


PANEL_HEADS = (('rgb', ('_rgb',)), ('lidar', ('_lidar', '_pcd_xy')), ('voxel', ('_voxel_top',)), ('route', ('_input_route_map',)))


def make_panel_batch(cfg, b, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    rf, fh, n = cfg.RECEPTIVE_FIELD, cfg.FUTURE_HORIZON, cfg.PREDICTION.N_SAMPLES
    s = rf + fh
    rand = lambda *shape: torch.rand(shape, generator=g, device=dev)

    def range_view(T):
        return torch.cat([torch.randn((b, T, 3, 64, 1024), generator=g, device=dev) * 0.4, rand(b, T, 1, 64, 1024)], dim=2)

    def heads(T):
        return {'rgb_1': rand(b, T, 3, 320, 832), 'lidar_reconstruction_1': range_view(T),
                'voxel_1': torch.cat([lg.unsqueeze(0) for lg in (make_logits(T, 2, dev) for _ in range(b))])}
    batch = {'rgb_label_1': rand(b, s, 3, 320, 832), 'throttle_brake': rand(b, s, 1) * 2 - 1, 'steering': rand(b, s, 1) * 2 - 1,
             'range_view_label_1': range_view(s), 'voxel_label_1': (rand(b, s, 1, *GRID) < 0.1).to(torch.uint8),
             'route_map': rand(b, s, 3, 64, 64) * 3 - 1}
    return batch, heads(rf), [heads(fh) for _ in range(n)]


def panels_main(a):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    import visualise_reference as VR
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.visualise import render_panels
    dev = torch.device('cuda')
    base = base_1d_cfg()
    b = 2
    batch, output, imagines = make_panel_batch(base, b, dev)
    keys = {'rgb': ('rgb_label_1', 'throttle_brake', 'steering', 'rgb_1'), 'lidar': ('range_view_label_1', 'lidar_reconstruction_1'),
            'voxel': ('voxel_label_1', 'voxel_1'), 'route': ('route_map',)}
    lines = [f'# prediction panels of one base_1d test batch: b {b}, {base.RECEPTIVE_FIELD} + {base.FUTURE_HORIZON} frames, '
             f'{len(imagines)} imagined sample(s); {a.rounds} alternating windows; device / to host: {a.iters} calls per window, host: '
             f'{a.host_iters}; median ms per call (min .. max); torch CPU threads: {torch.get_num_threads()}']
    for name, suffixes in PANEL_HEADS + (('all', tuple(k for _, v in PANEL_HEADS for k in v)),):
        on = [name] if name != 'all' else [h for h, _ in PANEL_HEADS]
        cfg = VR.panel_cfg(**{h: True for h in on})
        used = [k for h in on for k in keys[h]]
        sub = lambda d: {k: v for k, v in d.items() if k in used}
        bt, out, ims = sub(batch), sub(output), [sub(i) for i in imagines]
        # `s` and `rf` are read from the first batch entry and the last output entry: any entry has the right length
        bt.setdefault('route_map', batch['route_map'])
        out.setdefault('rgb_1', output['rgb_1'])
        got = render_panels(cfg, bt, out, ims)
        assert tuple(got) == suffixes, (tuple(got), suffixes)

        def host(timing=None):
            t0 = time.perf_counter()
            cpu = lambda d: {k: v.cpu() for k, v in d.items()}
            hb, ho, hi = cpu(bt), cpu(out), [cpu(i) for i in ims]
            t1 = time.perf_counter()
            if timing is not None:
                timing.append(t1 - t0)
            return VR.render_panels(cfg, hb, ho, hi)
        want = host()
        for k in suffixes:
            assert np.array_equal(got[k].cpu().numpy(), want[k]), f'the two routes disagree on {k}'

        def device_panels(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                render_panels(cfg, bt, out, ims)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        def to_host():
            return {k: v.cpu() for k, v in render_panels(cfg, bt, out, ims).items()}
        device_panels(3)
        wall(to_host, 2)
        d_t, k_t, h_t, c_t = [], [], [], []
        for _ in range(a.rounds):
            d_t.append(device_panels(a.iters))
            k_t.append(wall(to_host, max(1, a.iters // 5)))
            if a.host_iters:
                per = []
                h_t.append(wall(lambda: host(per), a.host_iters))
                c_t.append(statistics.mean(per) * 1e3)
        read = sum(v.numel() * v.element_size() for d in [bt, out] + ims for k, v in d.items() if k in used)
        written = sum(v.numel() for v in got.values())
        med = statistics.median(d_t)
        first = len(lines)
        lines += [f'{name}  panels {" ".join(f"{k} {tuple(got[k].shape)}" for k in suffixes)}',
                  f'  read {read / 1e6:.1f} MB  written {written / 1e6:.2f} MB',
                  f'  device            {fmt(d_t)}   {(read + written) / med / 1e6:.0f} GB/s, '
                  f'{100 * (read + written) / med / 1e6 / HBM_PEAK_GBS:.1f} % of the {HBM_PEAK_GBS / 1e3:.0f} TB/s HBM peak',
                  f'  to host           {fmt(k_t)}']
        if h_t:
            lines += [f'  host     total    {fmt(h_t)}',
                      f'  host     copy     {fmt(c_t)}',
                      f'  host total / to host = {statistics.median(h_t) / statistics.median(k_t):.0f}']
        for line in lines[first:]:
            print(line, flush=True)
    return lines


def write_out(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', choices=('export', 'confusion', 'panels'), default='export')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda')
    if a.what == 'confusion':
        write_out(a.out, confusion_main(a))
        return
    if a.what == 'panels':
        write_out(a.out, panels_main(a))
        return
    lines = [f'# voxel export routes, {GRID[0]} x {GRID[1]} x {GRID[2]} voxels per frame; {a.rounds} alternating windows; kernels: '
             f'{a.iters} calls per window, host: {a.host_iters}; median ms per call (min .. max); torch CPU threads: {torch.get_num_threads()}']
    for F, C in CASES:
        lg = make_logits(F, C, dev)
        rows_k, counts = kernels_to_host(lg)                           # warm-up of the kernel route, and the comparison
        rows_h, counts_h = host_route(lg)
        assert counts == counts_h and np.array_equal(rows_k.astype(np.int64), rows_h), 'the two routes disagree'
        total, V = sum(counts), GRID[0] * GRID[1] * GRID[2]
        buf = torch.empty((total, 4), dtype=torch.uint16, device=dev)
        device_ms(lg, buf, 3)
        wall(lambda: kernels_to_host(lg), 2)
        dev_t, k_t, h_t, copy_t = [], [], [], []
        for _ in range(a.rounds):
            dev_t.append(device_ms(lg, buf, a.iters))
            k_t.append(wall(lambda: kernels_to_host(lg), max(1, a.iters // 5)))
            if a.host_iters:
                per = []
                h_t.append(wall(lambda: host_route(lg, per), a.host_iters))
                copy_t.append(statistics.mean(per) * 1e3)
        floor = F * V * (4 * C + 2) + 8 * total
        med = statistics.median(dev_t)
        lines += [f'F {F}  C {C}  occupied {100 * total / (F * V):.2f} %  rows {total} ({8 * total / 1e6:.1f} MB)  logits {4 * F * C * V / 1e6:.0f} MB',
                  f'  kernels  device   {fmt(dev_t)}   traffic floor {floor / 1e6:.0f} MB -> {floor / med / 1e6:.0f} GB/s, '
                  f'{100 * floor / med / 1e6 / HBM_PEAK_GBS:.1f} % of the {HBM_PEAK_GBS / 1e3:.0f} TB/s HBM peak',
                  f'  kernels  to host  {fmt(k_t)}']
        if h_t:
            lines += [f'  host     total    {fmt(h_t)}',
                      f'  host     copy     {fmt(copy_t)}   ({4 * F * C * V / statistics.median(copy_t) / 1e6:.1f} GB/s device to pageable host memory)',
                      f'  host total / kernels to host = {statistics.median(h_t) / statistics.median(k_t):.0f}']
        for line in lines[(-6 if h_t else -3):]:
            print(line, flush=True)
        del lg, buf
    write_out(a.out, lines)


if __name__ == '__main__':
    main()
