"""Where the time of a batch from recorded runs goes, for the base_1d batch of 2 x 10 frames (600 x 960 camera and depth image,
192 x 192 bird's-eye view, ~20 000-point sweeps, ~20 000 voxel rows per frame; the miniature recording of
muvo_amd/data/recording_inputs.py, written to a temporary directory):

  host     file reading + decoding + staging into pinned memory, ms per batch at the pool size used;
  copy     host -> device of the staged batch, ms (HIP events);
  kernels  each preparation entry point of csrc/dataset.hip, ms per batch (HIP events) next to the bytes it must move;
  step     `train.fit` ms per step with batches from the loader (input stream / main stream) against two synthetic batches
           resident in HBM, alternating (what bench.py times).

    python tools/dataset_bench.py [--steps 20] [--warmup 5] [--workers 4] [--heads-on] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from muvo_amd import input_pipeline as IP  # noqa: E402
from muvo_amd.data import recording_inputs as RI  # noqa: E402
from muvo_amd.data.dataset import BatchLoader, DataModule, PinnedBuffers, collate_raw  # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X peak
B, RF, FH, RUN_FRAMES = 2, 6, 4, 40


def event_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_table(raw, cfg):
    """ms per batch and minimum traffic of every preparation entry point on the raw device batch."""
    b, s = raw['image'].shape[:2]
    F = b * s
    fr = {k: v.reshape(F, *v.shape[2:]) for k, v in raw.items() if torch.is_tensor(v)}
    n = int(raw['n_classes'])
    HW_bev = fr['birdview_int'].shape[1] * fr['birdview_int'].shape[2]
    mask = IP.birdview_decode_frames(fr['birdview_int'], n)[2]
    P, Q = int(fr['num_points'].sum()), int(fr['num_voxels'].sum())
    hw_rv = cfg.POINTS.CHANNELS * cfg.POINTS.HORIZON_RESOLUTION
    nvox = int(np.prod(cfg.VOXEL.SIZE))
    img = fr['depth_semantic'].shape[1] * fr['depth_semantic'].shape[2] if 'depth_semantic' in fr else 0
    rows = [
        ('birdview_decode_frames', lambda: IP.birdview_decode_frames(fr['birdview_int'], n), F * HW_bev * (4 + 4 * n + 8 + 1)),
        # mask read, parent written / read / written by the flatten, read by the numbering, ranks, labels written
        ('label_components_frames', lambda: IP.label_components_frames(mask), F * HW_bev * (1 + 4 * 5)),
        # points read by two passes (13 B each) + winner's re-read, 12-byte scratch cleared and read, 16-byte pixel written
        ('range_projection_frames', lambda: IP.range_projection_frames(fr['points_xyz'], fr['obj_tag'], fr['num_points'], with_seg=False),
         2 * P * 12 + F * hw_rv * (12 + 12 + 16)),
        # rows read (32 B), 4-byte key cleared and read, 1 byte written per voxel
        ('voxel_grid_frames', lambda: IP.voxel_grid_frames(fr['voxel_rows'], fr['num_voxels'], size=tuple(cfg.VOXEL.SIZE)), Q * 32 + F * nvox * 9),
    ]
    if img:
        rows.append(('depth_semantic_decode_frames (all four outputs)', lambda: IP.depth_semantic_decode_frames(fr['depth_semantic']),
                     F * img * (4 + 8 + 1 + 24 + 8)))
    rows.append(('prepare_frames (this configuration)', lambda: IP.prepare_frames(raw, cfg), None))
    out = []
    for name, fn, nbytes in rows:
        ms = event_ms(fn)
        out.append({'entry': name, 'ms_per_batch': ms, 'bytes': nbytes,
                    'ms_at_hbm_peak': None if nbytes is None else nbytes / HBM_BYTES_PER_S * 1e3})
    return out


def fit_ms(cfg, dev, steps, warmup, next_batch):
    """ms per optimizer step of train.fit, from HIP events recorded each time the loop asks for a batch."""
    from muvo_amd import train
    marks = []

    def batch_fn(micro):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((e, time.perf_counter()))
        return next_batch(micro)

    module, _ = train.fit(cfg, dev, steps=warmup + steps + 1, log=lambda s: None, batch_fn=batch_fn)
    torch.cuda.synchronize()
    ms = sorted(marks[i][0].elapsed_time(marks[i + 1][0]) for i in range(warmup, warmup + steps))
    wall = (marks[warmup + steps][1] - marks[warmup][1]) / steps * 1e3
    del module
    torch.cuda.empty_cache()
    return {'mean_ms': sum(ms) / len(ms), 'median_ms': ms[len(ms) // 2], 'min_ms': ms[0], 'max_ms': ms[-1], 'host_wall_ms': wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--workers', type=int, default=4, help='N_WORKERS: host threads of the loader (at most 16 are used)')
    ap.add_argument('--heads-on', action='store_true', help='also read and decode the depth / semantic image (config-off heads)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('dataset_bench needs a GPU')
    dev = torch.device('cuda', 0)
    variant = 'heads_on' if args.heads_on else 'default'
    cfg = RI.recording_cfg(variant, RECEPTIVE_FIELD=RF, FUTURE_HORIZON=FH, BATCHSIZE=B, STEPS=100000, N_WORKERS=args.workers,
                           VAL_CHECK_INTERVAL=0, LOGGING_INTERVAL=1000000,
                           **{'OPTIMIZER.ACCUMULATE_GRAD_BATCHES': 1})          # one batch per optimizer step, as bench.py times it
    res = {'device': torch.cuda.get_device_name(0), 'batch': [B, RF + FH], 'variant': variant, 'steps': args.steps}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        RI.write_recording(root, runs=(('train', 'Town01', '0000', RUN_FRAMES, True), ('train', 'Town01', '0001', RUN_FRAMES, True)))
        dm = DataModule(cfg, root, device=dev, seed=1234)
        dm.setup()
        ds = dm.train_dataset
        loader = dm.train_dataloader()
        res['recording'] = {'sequences': len(ds), 'batches_per_epoch': len(loader), 'write_s': time.perf_counter() - t0}
        # host: frames of one batch through the pool, then stacked and staged in pinned memory
        order = loader.batch_indices(0)
        slot = PinnedBuffers()
        from muvo_amd.data.dataset import stack_frames
        with ThreadPoolExecutor(max_workers=loader.n_threads) as pool:
            host = []
            for rep in range(4):
                t0 = time.perf_counter()
                seqs = [[pool.submit(ds.read_frame, ds.data_pointers[i][0], t) for t in ds.data_pointers[i][1]] for i in order[rep % len(order)]]
                raws = [stack_frames([f.result() for f in q], ds.intrinsics, ds.extrinsics) for q in seqs]
                t1 = time.perf_counter()
                staged = collate_raw(raws, slot)
                host.append({'read_decode_ms': (t1 - t0) * 1e3, 'stage_ms': (time.perf_counter() - t1) * 1e3})
        t0 = time.perf_counter()
        ds.read_frame(*[(r, idx[0]) for r, idx in ds.data_pointers][0])
        res['host'] = {'threads': loader.n_threads, 'per_batch': host[1:], 'one_frame_one_thread_ms': (time.perf_counter() - t0) * 1e3,
                       'staged_mbytes': sum(v.numel() * v.element_size() for v in staged.values() if torch.is_tensor(v)) / 1e6}
        res['h2d_ms'] = event_ms(lambda: {k: v.to(dev, non_blocking=True) for k, v in staged.items() if torch.is_tensor(v)}, reps=10)
        raw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in staged.items()}
        res['kernels'] = kernel_table(raw, cfg)
        del raw
        # step time: loader on its input stream, loader on the main stream, two resident synthetic batches
        from muvo_amd.data.synthetic import make_batch
        syn = [make_batch(B, RF + FH, seed=1234 + k, device=dev) for k in range(2)]
        res['fit_synthetic'] = fit_ms(cfg, dev, args.steps, args.warmup, lambda m: dict(syn[m % 2]))
        del syn
        for name, stream in (('fit_loader_input_stream', True), ('fit_loader_main_stream', False)):
            d = DataModule(cfg, root, device=dev, seed=1234, input_stream=stream)
            d.setup()
            it = d.train_batches()
            res[name] = fit_ms(cfg, dev, args.steps, args.warmup, lambda m: next(it))
            it.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
