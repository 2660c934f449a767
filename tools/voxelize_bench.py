"""Time per frame of input_pipeline.depth_lidar_voxels on the GPU (600 x 960 image + 60 000-point sweep, the dataset's grid):
rows and dense output, F = 1 and F = 16 frames per call, HIP-event timed after warm-up (two windows each: the spread shows in
the two figures), next to the traffic floor of the design.

    python tools/voxelize_bench.py [--seconds 1.0] [--frames 1 16] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from muvo_amd import input_pipeline as IP  # noqa: E402
from muvo_amd.config import get_cfg  # noqa: E402
from muvo_amd.data.voxelize_inputs import frame_case  # noqa: E402
from muvo_amd.generate_voxels import geometry_from_cfg  # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X peak


def traffic_floor_bytes(H, W, P, slots, dense):
    """Bytes the design must move per frame: the inputs are read by the distance pass and again by the winner pass; the scratch
    is cleared (best 8 + winner 4 + road 1 bytes per slot), read by the label pass (winner 4 + road 1) which writes 2 bytes of
    label per slot, read again by the output pass (2), which writes 1 byte per slot (dense) or 32 bytes per occupied voxel."""
    inputs = 2 * (H * W * 4 + P * 13)
    return inputs + slots * (13 + 5 + 2 + 2 + (1 if dense else 0))


def time_call(fn, seconds):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    reps = max(5, int(seconds * 1e3 / max(start.elapsed_time(end), 1e-3)))
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=1.0, help='length of each timed window')
    ap.add_argument('--frames', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('voxelize_bench needs a GPU')
    dev = torch.device('cuda')
    geom = geometry_from_cfg(get_cfg())
    img, pts, tag = frame_case()
    H, W, P = img.shape[0], img.shape[1], len(pts)
    slots = int(np.prod(geom['voxel_size']))
    lines = [f'device {torch.cuda.get_device_name(0)}; frame {H} x {W} + {P} points, grid {geom["voxel_size"]} at {geom["voxel_resolution"]} m']
    results = []
    for F in args.frames:
        # frames of one call differ (rolled images), as in a recorded run
        dimg = torch.from_numpy(np.stack([np.roll(img, 7 * f, axis=1) for f in range(F)])).to(dev)
        dpts, dtag = torch.from_numpy(np.stack([pts] * F)).to(dev), torch.from_numpy(np.stack([tag] * F)).to(dev)
        for dense in (True, False):
            per = [time_call(lambda: IP.depth_lidar_voxels(dimg, dpts, dtag, dense=dense, frames_per_call=F, **geom), args.seconds)[0] / F
                   for _ in range(2)]
            floor = traffic_floor_bytes(H, W, P, slots, dense) / HBM_BYTES_PER_S * 1e3
            results.append(dict(F=F, output='dense' if dense else 'rows', ms_per_frame=per, floor_ms=floor))
            lines.append(f'F={F:3d} {"dense" if dense else "rows ":5s}: ' + ' / '.join(f'{v:.4f}' for v in per) +
                         f' ms per frame; traffic floor {floor:.4f} ms ({100 * floor / min(per):.1f} % reached)')
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(results))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
