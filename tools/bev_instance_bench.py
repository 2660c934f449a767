"""Times the BEV instance decode and the panoptic-quality counts on the GPU at the model's bird's-eye-view
size, 20 frames of 192 x 192 with 8 classes, K = 100:
  (a)  a synthetic scene: a dozen Gaussian blobs per frame as the centre map, offsets that point at the nearest blob plus noise,
       logits whose argmax is a thing class on discs around the blobs; the label ids are those discs
  (b)  the quantised-noise map: uniform noise in steps of 1 / 64 (thousands of peaks, tied scores, every frame capped), random
       offsets of several cells, 40 % foreground - the worst case of the selection and what an untrained head produces
Decode and counting are timed apart.  HIP events around back-to-back calls after a warm-up, five windows, median (min .. max) per
call.

    python tools/bev_instance_bench.py [--out profiles/bev_instance_bench.txt] [--frames 20] [--size 192 192] [--centres 100]"""
import argparse
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


def thing_logits(fg, C, g):
    """(F, C, H, W): class 3 or 4 wins on fg, another class elsewhere"""
    F, H, W = fg.shape
    logits = torch.randn(F, C, H, W, generator=g)
    other = torch.tensor([k for k in range(C) if k not in (3, 4)])[torch.randint(0, C - 2, (F, H, W), generator=g)]
    top = torch.where(fg, torch.randint(3, 5, (F, H, W), generator=g), other)
    return logits.scatter_(1, top.unsqueeze(1), 9.0)


def blobs(F, H, W, C, n, seed):
    """centre (F, H, W), offset (F, 2, H, W), logits (F, C, H, W), label ids (F, H, W) uint8"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    centre, offset, label = torch.zeros(F, H, W), torch.zeros(F, 2, H, W), torch.zeros(F, H, W, dtype=torch.uint8)
    for f in range(F):
        cy, cx = torch.randint(8, H - 8, (n,), generator=g).float(), torch.randint(8, W - 8, (n,), generator=g).float()
        d2 = (yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2
        centre[f] = torch.exp(-d2 / 18.0).amax(0)
        near = d2.argmin(0)
        offset[f, 0], offset[f, 1] = cy[near] - yy, cx[near] - xx
        label[f] = torch.where(d2.amin(0) <= 36.0, near + 1, torch.zeros_like(near)).to(torch.uint8)
    offset += torch.randn(F, 2, H, W, generator=g) * 0.5
    return centre, offset, thing_logits(label != 0, C, g), label


def noise(F, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    centre = torch.floor(torch.rand(F, H, W, generator=g) * 64) / 64
    offset = torch.randn(F, 2, H, W, generator=g) * 6
    fg = torch.rand(F, H, W, generator=g) < 0.4
    blocks = torch.randint(0, 40, (F, H // 8 + 1, W // 8 + 1), generator=g).to(torch.uint8)
    label = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()
    return centre, offset, thing_logits(fg, C, g), label


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(192, 192))
    ap.add_argument('--classes', type=int, default=8)
    ap.add_argument('--centres', type=int, default=100)
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bev_instance_bench measures on the GPU: none found')
    from muvo_amd import ops
    from muvo_amd.bev_instances import PanopticQualityMetric
    dev = torch.device('cuda', 0)
    F, (H, W), C, K = args.frames, args.size, args.classes, args.centres
    lines = [f'# BEV instance decode and panoptic-quality counts, {F} frames of {H} x {W}, {C} classes, K = {K}, threshold 0.1, radius 1; library '
             f'{os.path.basename(ops._LIB_PATH)}; 5 windows of {args.calls} back-to-back calls, HIP events; median ms per call (min .. max)']
    for name, scene in (('(a) a dozen Gaussian blobs', blobs(F, H, W, C, 12, 1)), ('(b) noise quantised to 1/64', noise(F, H, W, C, 2))):
        centre, offset, logits, label = (t.to(dev) for t in scene)
        run = lambda: ops.bev_instance_decode(centre, offset, logits, None, 0.1, 1, K)      # noqa: E731
        ids, _, n, capped = run()
        counts, total = torch.zeros(7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        td = timed(run, args.calls)
        tc = timed(lambda: ops.bev_pq_counts(label, ids, counts, total, capped), args.calls)
        counts.zero_()
        total.zero_()
        ops.bev_pq_counts(label, ids, counts, total, capped)
        s = PanopticQualityMetric.summarise([counts.cpu().tolist(), [0] * 7], [total.cpu().tolist(), [0.0]])
        lines.append(f'{name + ": decode":<44}{td[0]:9.3f} ({td[1]:9.3f} .. {td[2]:9.3f})   {F * H * W / td[0] / 1e6:.2f} G pixels/s')
        lines.append(f'{name + ": counts":<44}{tc[0]:9.3f} ({tc[1]:9.3f} .. {tc[2]:9.3f})   {F * H * W / tc[0] / 1e6:.2f} G pixels/s')
        lines.append(f'    centres per frame {float(n.float().mean()):.1f}, capped frames {int(capped.sum())}, foreground {float((ids != 0).float().mean()):.3f} of the pixels; '
                     f'PQ {s["bev_pq"]:.4f} SQ {s["bev_sq"]:.4f} RQ {s["bev_rq"]:.4f}, tp {s["bev_tp"]} fp {s["bev_fp"]} fn {s["bev_fn"]}; id checksum {int(ids.long().sum())}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
