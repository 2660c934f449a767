"""Times the two neighbour searches of the on-device ICP (csrc/icp.hip; DESIGN.md section 8b, "grid search") against each other
on one GPU, in one process, the two modes interleaved repetition by repetition, device events around the launches after
untimed warm-up calls, at least five repetitions with their spread.  Inputs: the ray-cast scene of tests/icp_reference.py at
64 x 1024 rays, every point valid, three rows of seven frames 1 m / 0.1 m / 2 degrees apart = 18 pairs of 65,536 points (the
work list of section 8b).  Each row one JSON line:

  build      muvo_icp_grid_build of the 18 pairs (bounding box, histogram, scan, scatter), ms per call and per pair
  iteration  one iteration (correspond + update) with all 18 pairs running - iterations 3 .. 2 + reps of a registration from the
             identity, the same poses in both modes since their states are equal bit for bit -, brute and grid, source_stride 1
             and 4; `accepted` = the grid's slowest repetition is below brute's fastest
  register   the whole ops.icp_register call (the grid build and the `done` reads included), host wall clock around the call
  queued     ops.icp_register_queued with the budget of section 18: 30 iterations, stride 4, the 18 links
  step       (--parts step) the training step of section 18 with VOXEL_SEG.AGGREGATE and poses from ICP, ICP_SEARCH brute and grid,
             the keys switched inside one process between windows of --steps steps after 3 untimed ones, --rounds rounds

    python tools/icp_search_bench.py [--parts build iteration register queued step] [--reps 5] [--steps 20] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W, ROWS, FRAMES = 64, 1024, 3, 7
THRESHOLD = 5.0
MODES = ('brute', 'grid')


def scene_frames(dev):
    """(ROWS * FRAMES, 4, H W) float32 and the work list: frame t of a row moves onto frame t - 1"""
    import icp_reference as R
    frames = []
    for r in range(ROWS):
        T = R.pose(0.3 * r, 0.2 * r, 5.0 * r)
        for t in range(FRAMES):
            frames.append(R.frame_of(R.ray_cast(T, H, W), 4, 1.0))
            T = T @ R.pose(1.0, 0.1, 2.0)
    src = [r * FRAMES + t for r in range(ROWS) for t in range(1, FRAMES)]
    return torch.from_numpy(np.stack(frames)).to(dev), src, [f - 1 for f in src]


def spread(ms):
    ms = sorted(ms)
    return {'min': round(ms[0], 4), 'median': round(ms[len(ms) // 2], 4), 'max': round(ms[-1], 4), 'reps': len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_build(args, dev, frames, src, tgt):
    from muvo_amd import ops
    fr, state, done, ws, P, n = ops._icp_setup(frames, frames, src, tgt, 1.0, THRESHOLD, None, 1)
    for _ in range(args.warmup):
        ops._icp_grid(frames, fr, P, n, 1.0, THRESHOLD, done)
    ms = [timed(lambda: ops._icp_grid(frames, fr, P, n, 1.0, THRESHOLD, done)) for _ in range(args.reps)]
    print(json.dumps({'part': 'build', 'pairs': P, 'n': n, 'ms': spread(ms), 'ms_per_pair': spread([m / P for m in ms]),
                      'grid_MiB': round(int(ops.lib().muvo_icp_grid_bytes(ops._i64(P), ops._i64(n))) / 2 ** 20, 1)}), flush=True)


def part_iteration(args, dev, frames, src, tgt):
    from muvo_amd import ops
    for stride in (1, 4):
        st = {}
        for mode in MODES:
            fr, state, done, ws, P, n = ops._icp_setup(frames, frames, src, tgt, 1.0, THRESHOLD, None, stride)
            grid = ops._icp_grid(frames, fr, P, n, 1.0, THRESHOLD, done) if mode == 'grid' else None
            st[mode] = (fr, state, done, ws, P, n, grid)

        def one(mode):
            fr, state, done, ws, P, n, grid = st[mode]
            ops._icp_iterate(frames, frames, fr, P, n, 1.0, THRESHOLD, stride, 2000, 1, ws, state, done, grid=grid)
        for _ in range(args.warmup):
            for mode in MODES:
                one(mode)
        ms = {m: [] for m in MODES}
        for _ in range(args.reps):
            for mode in MODES:
                ms[mode].append(timed(lambda: one(mode)))
        running = all(int(st[m][2].sum()) == 0 for m in MODES)
        equal = torch.equal(st['brute'][1], st['grid'][1])
        P = st['brute'][4]
        print(json.dumps({'part': 'iteration', 'source_stride': stride, 'pairs': P, 'all_pairs_running': running, 'states_equal': equal,
                          'brute_ms': spread(ms['brute']), 'grid_ms': spread(ms['grid']),
                          'brute_ms_per_pair_iteration': round(sorted(ms['brute'])[len(ms['brute']) // 2] / P, 4),
                          'grid_ms_per_pair_iteration': round(sorted(ms['grid'])[len(ms['grid']) // 2] / P, 4),
                          'ratio_of_medians': round(spread(ms['brute'])['median'] / spread(ms['grid'])['median'], 2),
                          'accepted': max(ms['grid']) < min(ms['brute'])}), flush=True)


def part_register(args, dev, frames, src, tgt):
    from muvo_amd import ops
    for stride in (1, 4):
        res, ms = {}, {m: [] for m in MODES}
        for rep in range(args.reps + 1):                    # the first round is the warm-up
            for mode in MODES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[mode] = ops.icp_register(frames, frames, src, tgt, 1.0, THRESHOLD, source_stride=stride, search=mode)
                torch.cuda.synchronize()
                if rep:
                    ms[mode].append((time.perf_counter() - t0) * 1e3)
        equal = all(torch.equal(a, b) for a, b in zip(res['brute'], res['grid']))
        its = res['grid'].iterations.tolist()
        print(json.dumps({'part': 'register', 'source_stride': stride, 'iterations': [min(its), max(its)], 'results_equal': equal,
                          'brute_ms': spread(ms['brute']), 'grid_ms_with_build': spread(ms['grid']),
                          'ratio_of_medians': round(spread(ms['brute'])['median'] / spread(ms['grid'])['median'], 2)}), flush=True)


def part_queued(args, dev, frames, src, tgt):
    from muvo_amd import ops
    res, ms = {}, {m: [] for m in MODES}
    for rep in range(args.reps + 1):
        for mode in MODES:
            def call():
                res[mode] = ops.icp_register_queued(frames, frames, src, tgt, 1.0, THRESHOLD, 30, source_stride=4, search=mode)
            t = timed(call)
            if rep:
                ms[mode].append(t)
    equal = all(torch.equal(a, b) for a, b in zip(res['brute'], res['grid']))
    print(json.dumps({'part': 'queued', 'iterations': 30, 'source_stride': 4, 'links': len(src), 'results_equal': equal,
                      'brute_ms': spread(ms['brute']), 'grid_ms_with_build': spread(ms['grid']),
                      'ratio_of_medians': round(spread(ms['brute'])['median'] / spread(ms['grid'])['median'], 2)}), flush=True)


def part_step(args, dev):
    """section 18's row "+ AGGREGATE, poses from ICP (defaults)" in both searches, its method: one process, the keys switched"""
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.data.synthetic import make_batch
    from muvo_amd.odometry import register_consecutive
    from muvo_amd.trainer import WorldModelTrainer
    B, S = 2, 10
    cfg = base_1d_cfg(RECEPTIVE_FIELD=6, FUTURE_HORIZON=S - 6, BATCHSIZE=B, STEPS=100000)
    torch.manual_seed(1234)
    tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    tr.train()
    opts, scheds = tr.configure_optimizers()
    opt, sched = opts[0], scheds[0]['scheduler']
    batches = [make_batch(B, S, seed=1234 + k, device=dev) for k in range(2)]
    node = type(tr.cfg)

    def set_keys(kind):
        tr.cfg.VOXEL_SEG.pop('VISIBILITY', None)
        tr.cfg.VOXEL_SEG.pop('AGGREGATE', None)
        if kind != 'absent':
            tr.cfg.VOXEL_SEG['VISIBILITY'] = node({'ENABLED': True})
            tr.cfg.VOXEL_SEG['AGGREGATE'] = node({'ENABLED': True, 'ICP_SEARCH': kind})

    def step(i):
        opt.zero_grad()
        loss = tr.training_step(dict(batches[i % 2]), i)
        loss.backward()
        tr.on_after_backward()
        opt.step()
        sched.step()

    kinds = ('absent', 'brute', 'grid')
    rows = {k: [] for k in kinds}
    i = 0
    for _ in range(args.rounds):
        for kind in kinds:
            set_keys(kind)
            for _ in range(3):
                step(i)
                i += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(i)
                i += 1
            torch.cuda.synchronize()
            rows[kind].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 2))
    set_keys('absent')
    rv = tr.preprocess(dict(batches[0]))['range_view_label_1']
    alone = {m: [] for m in MODES}
    for rep in range(args.reps + 1):
        for mode in MODES:
            t = timed(lambda: register_consecutive(rv, float(cfg.LIDAR_RE.SCALE), queued=True, max_iteration=30, source_stride=4, search=mode))
            if rep:
                alone[mode].append(t)
    print(json.dumps({'part': 'step', 'batch': B, 'frames': S, 'steps': args.steps, 'ms_per_step': rows,
                      'icp_queued_alone_ms': {m: spread(alone[m]) for m in MODES}, 'icp_pairs': B * (S - 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['build', 'iteration', 'register', 'queued'])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('icp_search_bench: needs a GPU (a CPU run says nothing about these times)')
    if args.reps < 5:
        raise SystemExit('icp_search_bench: at least five repetitions')
    dev = torch.device('cuda:0')
    if set(args.parts) & {'build', 'iteration', 'register', 'queued'}:
        frames, src, tgt = scene_frames(dev)
        for name, part in (('build', part_build), ('iteration', part_iteration), ('register', part_register), ('queued', part_queued)):
            if name in args.parts:
                part(args, dev, frames, src, tgt)
    if 'step' in args.parts:
        part_step(args, dev)


if __name__ == '__main__':
    main()
