"""Time of the two voxel-export routes of a prediction run (muvo_amd/predict.py) on the GPU.

    python tools/predict_bench.py [--rounds 5] [--iters 50] [--host-iters 1] [--out profiles/predict_export.txt]
    (--host-iters 0: the kernel route only, e.g. under a kernel trace)

Routes, on the same logits (F frames of C x 192 x 192 x 64 float32 on the device, about 10 % of the voxels occupied):
  kernels    ops.voxel_rows (csrc/export.hip: classify + count, scan, ordered compaction), the rows copied to the host.
             `device` is the three kernels alone between HIP events (ops.voxel_rows_into, a preallocated buffer, no host
             read), `to host` the whole call including the read of the counts and the copy of the rows, by the host clock
             around a device synchronise.
  host       the reference's route restated (sim_run.py:78-79): logits.cpu(), torch.argmax, torch.where, stack - by the host
             clock; `copy` is the .cpu() alone.  torch's CPU thread count is printed: it bounds argmax and where.
Warm-up first, then `--rounds` windows per route, the routes alternating; median (min .. max) over the windows of the
per-call mean.  The traffic floor of the kernel route is C * 4 B read + 1 B written and 1 B read per voxel + 8 B per row; its
share of the HBM peak is quoted for the `device` time only.  Before timing, the rows of both routes are compared once."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda')
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
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
