"""Golden fixture of the Chamfer-distance training loss: the REAL reference class muvo.losses.CDLoss (losses.py:352-367,
reducer = mean), forward and backward on the CPU, on fixed-seed point clouds of (frames, n) = (3, 20), (3, 300), (2, 1031).
Writes tests/golden/chamfer_loss.npz - data only: per case k the inputs pred_k / target_k (frames, n, 3) float32 as the
reference takes them, its loss_k and dpred_k, and ref_f64_loss_k / ref_f64_dpred_k: the reference's OWN distance from the
float64 restatement of tests/chamfer_reference.py (normalised as the tests normalise: |loss - loss64| / |loss64|, max |dpred -
dpred64| / max |dpred64|).  Above 25 rows torch.cdist evaluates |p|^2 - 2 p.t + |t|^2 with a matrix product, which is where that
distance comes from.

The coordinates are multiples of 2^-14 in [-1, 1) (the file then compresses to well under 100 KB).  For every case the seed is
the first for which every query's nearest / second-nearest gap is >= 1e-4 (chamfer_reference.GAP_MIN); the script asserts that
the reference's own argmin indices (of its cdist matrix) equal the float64 ones, so both differentiate the same selections.

Usage: python tools/golden/make_golden_chamfer.py --reference DIR      (a checkout of the reference; development machine only)
The file is written with fixed zip time stamps, so a second run reproduces it byte for byte.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, HERE)

import chamfer_reference as R  # noqa: E402
import loss_reference as LR  # noqa: E402
from make_golden_voxelize import write_npz  # noqa: E402


def draw(frames, n, seed):
    g = torch.Generator().manual_seed(seed)
    q = lambda: (torch.randint(-(1 << 14), 1 << 14, (frames, n, 3), generator=g).float() / (1 << 14))      # noqa: E731
    return q(), q()


def planar(x):
    return x.permute(0, 2, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refimport', 'stubs'))
    sys.path.insert(0, os.path.abspath(args.reference))
    from muvo.losses import CDLoss
    crit = CDLoss()
    out = {'shapes': np.asarray(R.GOLDEN_SHAPES, dtype=np.int64)}
    for k, (frames, n) in enumerate(R.GOLDEN_SHAPES):
        for seed in range(1000):
            pred, target = draw(frames, n, 1000 * k + seed)
            ref = R.chamfer64(planar(pred), planar(target))
            if min(float(ref['gap_pt'].min()), float(ref['gap_tp'].min())) >= R.GAP_MIN:
                break
        else:
            raise SystemExit(f'case {k}: no seed without a near tie')
        p = pred[None].clone().requires_grad_(True)
        loss = crit(p, target[None])
        loss.backward()
        dpred = p.grad[0]
        # the selections the reference differentiated: argmin of ITS distance matrix
        dist = torch.cdist(pred, target, 2)
        assert torch.equal(dist.min(2)[1], ref['idx_pt']) and torch.equal(dist.min(1)[1], ref['idx_tp']), \
            f'case {k}: the reference selects other neighbours than float64 does - change the seed'
        e_loss = abs(float(loss) - float(ref['loss'])) / abs(float(ref['loss']))
        d64 = ref['dpred'].permute(0, 2, 1)
        e_grad = LR.error_stats(dpred, d64, LR.scale_of(d64))['max_e']
        print(f'case {k}: frames {frames} n {n} seed {1000 * k + seed}: loss {float(loss):.9g}, reference vs float64: loss {e_loss:.2e}, '
              f'dpred {e_grad:.2e}')
        out.update({f'pred_{k}': pred.numpy(), f'target_{k}': target.numpy(), f'loss_{k}': np.float32(loss.item()),
                    f'dpred_{k}': dpred.numpy(), f'ref_f64_loss_{k}': np.float64(e_loss), f'ref_f64_dpred_{k}': np.float64(e_grad),
                    f'seed_{k}': np.int64(1000 * k + seed)})
    path = os.path.join(REPO, 'tests', 'golden', 'chamfer_loss.npz')
    write_npz(path, out)
    print('wrote tests/golden/chamfer_loss.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
