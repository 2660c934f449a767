"""Forward and backward time of the three attention paths of muvo_amd.ops (fused: K / V of a head whole in LDS, L <= 384;
stream: K / V blocks under an online softmax, any L; unfused: batched GEMMs + softmax kernel with L x L tensors in HBM).

    python tools/attention_bench.py [--rounds 5] [--iters 10] [--mask none|camera|lidar|mixed] [--lengths L ...] [--out FILE]

HIP events around each forward and each backward call, random data, the paths of one shape interleaved round by round in one
process; the table gives the median over the rounds of the per-call mean, the spread (min .. max over the rounds) and the rate
in TFLOP/s of the ALGORITHM's operations - forward 4 N H L^2 DH (Q K^T, P V), backward 8 N H L^2 DH (dV, dP, dQ, dK; the
recomputation of S inside the fused and streamed backward kernels is not counted) - against the fp32 matrix peak of 157.3.

--mask other than none: the fused and the streamed path are timed a second time with a key mask (rows `fused+mask`,
`stream+mask`: the muvo_attention_*mask* entry points), interleaved with the unmasked calls; the unfused path has no mask.
camera: the first 260 / 324 of the keys of every frame are masked (the image tokens' share of the model's sequence), lidar: the
rest, mixed: frames without a mask, with the camera mask and with the lidar mask in turn (what sensor dropout launches).  The
rates stay those of the full L x L problem, so a masked row reads as the time of the same call, not of less work."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from muvo_amd import ops  # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = [  # (L, N, H, DH, paths)
    (324, 20, 8, 48, ('fused', 'stream', 'unfused')),
    (388, 20, 8, 48, ('stream', 'unfused')),
    (1037, 4, 8, 48, ('stream', 'unfused')),
    (5184, 20, 8, 48, ('stream',)),          # unfused: three (20, 8, 5184, 5184) float tensors = 52 GB of scores: not run
]
FNS = {'fused': ops.FlashAttentionFn, 'stream': ops.StreamAttentionFn, 'unfused': ops.AttentionFn}


MASKED = {'fused+mask': ops.MaskedFlashAttentionFn, 'stream+mask': ops.MaskedStreamAttentionFn}


def key_mask(kind, L, N, dev):
    """(N, roundup(L, 16)) uint8 rows as the kernels read them"""
    cut = round(L * 260 / 324)
    m = torch.zeros(N, L, dtype=torch.bool)
    for n in range(N):
        which = {'camera': 1, 'lidar': 2, 'mixed': n % 3}[kind]
        if which == 1:
            m[n, :cut] = True
        elif which == 2:
            m[n, cut:] = True
    return ops.key_mask_rows(m.to(dev), N, L)


def time_calls(fn, qkv, dout, heads, p, iters, *mask):
    """(mean forward ms, mean backward ms) over `iters` calls"""
    f = b = 0.0
    for i in range(iters):
        x = qkv.detach().requires_grad_(True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        o = fn.apply(x, heads, p, 1000 + i, *mask)
        e[1].record()
        e[2].record()
        o.backward(dout)
        e[3].record()
        torch.cuda.synchronize()
        f += e[0].elapsed_time(e[1])
        b += e[2].elapsed_time(e[3])
    return f / iters, b / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--mask', choices=('none', 'camera', 'lidar', 'mixed'), default='none')
    ap.add_argument('--lengths', type=int, nargs='*', default=None, help='only these L of the shape list')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda')
    lines = [f'# attention paths, fp32, dropout p = {a.dropout}, key mask {a.mask}; {a.rounds} interleaved rounds x {a.iters} calls; median ms (min .. max), '
             f'TFLOP/s of 4 / 8 N H L^2 DH, share of the {PEAK_TFLOPS} TFLOP/s fp32 matrix peak',
             f'{"L":>5} {"N":>3} {"path":11} {"fwd ms":>26} {"TF/s":>6} {"peak":>6} {"bwd ms":>26} {"TF/s":>6} {"peak":>6}']
    for L, N, H, DH, paths in SHAPES:
        if a.lengths and L not in a.lengths:
            continue
        g = torch.Generator().manual_seed(L)
        qkv = torch.randn(L, N, 3 * H * DH, generator=g).to(dev)
        dout = torch.randn(L, N, H * DH, generator=g).to(dev)
        runs = {path: (FNS[path],) for path in paths}
        if a.mask != 'none':
            rows = key_mask(a.mask, L, N, dev)
            runs = {k: v for path in paths for k, v in ((path, (FNS[path],)),) + (((path + '+mask', (MASKED[path + '+mask'], rows)),)
                                                                                  if path + '+mask' in MASKED else ())}
        paths = list(runs)
        for path in paths:
            time_calls(runs[path][0], qkv, dout, H, a.dropout, 2, *runs[path][1:])           # warm-up: code objects, allocator
        res = {p: [] for p in paths}
        for _ in range(a.rounds):
            for path in paths:
                res[path].append(time_calls(runs[path][0], qkv, dout, H, a.dropout, a.iters, *runs[path][1:]))
        flop = N * H * L * L * DH
        for path in paths:
            cols = []
            for k, mult in ((0, 4), (1, 8)):
                t = [r[k] for r in res[path]]
                med = statistics.median(t)
                tf = mult * flop / (med * 1e-3) / 1e12
                cols.append(f'{med:9.3f} ({min(t):7.3f} .. {max(t):7.3f}) {tf:6.1f} {100 * tf / PEAK_TFLOPS:5.1f}%')
            lines.append(f'{L:5d} {N:3d} {path:11} {cols[0]} {cols[1]}')
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
