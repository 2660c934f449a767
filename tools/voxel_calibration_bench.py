"""Times muvo_voxel_calibration on the GPU at the voxel head's size, 20 frames of 192 x 192 x 64, for C = 2 and
C = 9 classes and K = 1 and K = 2 samples, without and with the byte maps, and in the same run a plain PyTorch composition of the
same figures (softmax per sample, their mean, two entropies, a one-hot for the Brier score, a bucketised confidence, masked
sums), so that the ratio is on record.  Logits are unit normal noise scaled by 3, 15 % of the labels are 255.  HIP events around
back-to-back calls after a warm-up, five windows, median (min .. max) ms per call; GB/s = the logits' bytes (K F C X Y Z 4) per
call time.

    python tools/voxel_calibration_bench.py [--out profiles/voxel_calibration_bench.txt] [--frames 20] [--grid 192 192 64]"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


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


def torch_composition(logits_list, label, B):
    """The same figures with stock tensor operations: (table (B, 3), counts (4,), per-class tp / fp / fn (C, 3), sums (6,))"""
    C = logits_list[0].shape[1]
    p = [torch.softmax(t, dim=1) for t in logits_list]
    pbar = torch.stack(p).mean(0)
    ebar = torch.stack([torch.special.entr(q).sum(1) for q in p]).mean(0)
    H = torch.special.entr(pbar).sum(1)
    mi = (H - ebar).clamp_min(0)
    conf, yhat = pbar.max(1)
    valid = label != 255
    target = torch.where(valid, label, torch.zeros_like(label)).long()
    ok = (yhat == target) & valid
    onehot = torch.nn.functional.one_hot(target, C).movedim(-1, 1)
    brier = ((pbar - onehot) ** 2).sum(1)
    nll = -pbar.gather(1, target.unsqueeze(1)).squeeze(1).clamp_min(1e-12).log()
    bins = (conf * B).floor().long().clamp_max(B - 1)
    w = valid.double()
    table = torch.stack([torch.bincount(bins.reshape(-1), weights=x.reshape(-1), minlength=B) for x in (w, ok.double(), conf.double() * w)], 1)
    counts = torch.stack([valid.sum(), (~valid).sum(), torch.zeros_like(valid.sum()), ok.sum()])
    per = torch.stack([torch.stack([((yhat == j) & (target == j) & valid).sum(), ((yhat == j) & (target != j) & valid).sum(),
                                    ((yhat != j) & (target == j) & valid).sum()]) for j in range(C)])
    wrong = valid & ~ok
    sums = torch.stack([(brier.double() * w).sum(), (nll.double() * w).sum(), (H.double() * ok).sum(), (H.double() * wrong).sum(),
                        (mi.double() * ok).sum(), (mi.double() * wrong).sum()])
    return table, counts, per, sums


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--grid', type=int, nargs=3, default=(192, 192, 64))
    ap.add_argument('--bins', type=int, default=15)
    ap.add_argument('--calls', type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('voxel_calibration_bench measures on the GPU: none found')
    from muvo_amd import ops
    from muvo_amd.calibration import VoxelCalibrationMetric, ensemble_calibration, new_accumulators
    dev = torch.device('cuda', 0)
    F, (X, Y, Z), B = args.frames, args.grid, args.bins
    lines = [f'# muvo_voxel_calibration, {F} frames of {X} x {Y} x {Z}, {B} bins, 15 % of the labels 255; library {os.path.basename(ops._LIB_PATH)}; '
             f'5 windows of {args.calls} back-to-back calls, HIP events; median ms per call (min .. max); GB/s against the logits\' bytes']
    g = torch.Generator(device=dev).manual_seed(1)
    for C in (2, 9):
        label = torch.randint(0, C, (F, X, Y, Z), generator=g, device=dev).to(torch.uint8)
        label[torch.rand((F, X, Y, Z), generator=g, device=dev) < 0.15] = 255
        samples = [torch.randn((F, C, X, Y, Z), generator=g, device=dev) * 3 for _ in range(2)]
        for K in (1, 2):
            lg = samples[:K]
            gbytes = K * F * C * X * Y * Z * 4 / 1e9
            acc = new_accumulators(C, B, dev)
            maps = ensemble_calibration(lg, label, bins=B, maps=True)
            extra = {k: maps[k] for k in ('ens', 'top_entropy', 'top_mi')}
            t0 = timed(lambda: ops.voxel_calibration(lg, label, acc['table'], acc['counts'], acc['ssc'], acc['sums']), args.calls)
            t1 = timed(lambda: ops.voxel_calibration(lg, label, acc['table'], acc['counts'], acc['ssc'], acc['sums'], **extra), args.calls)
            tt = timed(lambda: torch_composition(lg, label, B), max(1, args.calls // 2))
            s = VoxelCalibrationMetric.summarise(**{k: [v.cpu().tolist()] * 2 for k, v in maps.items() if k in acc})
            table, counts, per, sums = torch_composition(lg, label, B)
            agree = (int(counts[0]) == s['voxel_voxels'] and abs(float(sums[0]) / int(counts[0]) - s['voxel_brier']) < 1e-5
                     and abs(float(sums[1]) / int(counts[0]) - s['voxel_nll']) < 1e-5)
            name = f'C = {C}, K = {K} ({gbytes:.2f} GB of logits)'
            lines.append(f'{name + ": counters only":<52}{t0[0]:9.3f} ({t0[1]:9.3f} .. {t0[2]:9.3f})   {gbytes / t0[0] * 1e3:7.0f} GB/s')
            lines.append(f'{name + ": with ens + maps":<52}{t1[0]:9.3f} ({t1[1]:9.3f} .. {t1[2]:9.3f})   {gbytes / t1[0] * 1e3:7.0f} GB/s')
            lines.append(f'{name + ": PyTorch composition":<52}{tt[0]:9.3f} ({tt[1]:9.3f} .. {tt[2]:9.3f})   {tt[0] / t0[0]:7.1f} x the kernel')
            lines.append(f'    ece {s["voxel_ece"]:.5f} brier {s["voxel_brier"]:.5f} nll {s["voxel_nll"]:.5f} accuracy {s["voxel_accuracy"]:.5f} '
                         f'(ln C = {math.log(C):.4f}); the composition agrees on voxels, brier and nll: {agree}')
            del maps, extra, table, counts, per, sums
        del samples, label
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
