"""bench.py — world-model training samples/sec of the MI355X-native MUVO step (BASELINE.json metric).

`python bench.py --gpus N --steps K --warmup W`; for N > 1 either launch it through torch.distributed.run (one rank per
GPU, RCCL) or run it plainly — it then starts that launcher itself as a child process.  One "step" = preprocess + forward + 21 losses + backward + gradient all-reduce + fused AdamW on one
synthetic base_1d batch (per-GPU batch 2 x seq_len 10, 600x960 RGB -> 320x832 crop, 64x1024 range view,
192x192x64 voxels) that is already resident in HBM.  Prints ONE JSON line on rank 0.

A plain run measures the headline only: set-up, `--warmup` untimed steps, `--steps` timed steps, the result line.  `--full`
adds everything else the bench reports (HIP-event brackets of the dominant kernel class inside the timed region and the per-class
table from extra untimed steps, the exact-fp32 steps, the extension workloads, the CPU baseline).  `--dump-outputs DIR` writes
what the last timed step computed as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import muvo_amd  # noqa: E402,F401  (sets GPU_MAX_HW_QUEUES before the HIP runtime initialises)
import torch  # noqa: E402

GFLOP_PER_FRAME = 794.36       # fwd 265.35 + bwd 529.01 (2*MAC, conv/convT/matmul)


def usable_cores():
    """Host cores this process may actually use: min(affinity mask, cgroup CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


# the dominant kernel class is bracketed with HIP events on every BRACKET_EVERY-th step of the timed region (162 pairs per bracketed
# step; on every step they cost the region 0.3-0.5 ms per step: 77.3 vs 76.9 ms)
BRACKET_EVERY = 4


def cpu_baseline(cores):
    """The oracle restatement (validated against the reference, tests/golden) timed on the host cores on a bounded sample of
    BASELINE.json configs[0] (batch 1 x seq_len 4, the reference's own CPU-runnable case): one warm-up step at batch 1 x
    seq_len 2 (allocator, thread pool), then ONE full training step (fwd + 21 losses + bwd + AdamW) at batch 1 x seq_len 4;
    ~20-30 s of CPU work on 16 cores.  value = frames/s / 10 (one sample = 10 frames)."""
    import resource
    from muvo_amd.data.synthetic import make_batch, make_noise
    from muvo_amd.utils import detinit
    from oracle import muvo_ref as R
    torch.set_num_threads(cores)
    model = R.MileRef()
    detinit.fill_state_dict_(model)
    model.train()
    opt, sched = R.make_optimizer(model, model.cfg)
    times = []
    for b, s in ((1, 2), (1, 4)):
        batch = make_batch(b, s, seed=1234)
        eps, use_prior = make_noise(b, s, seed=1234)
        t0 = time.time()
        total, _, _, _ = R.training_step(model, batch, eps, use_prior)
        opt.zero_grad(set_to_none=True)
        total.backward()
        opt.step()
        times.append(time.time() - t0)
        del total
    dt = times[1]
    frames_per_s = 4.0 / dt
    return dict(value=frames_per_s / 10.0, unit='samples/s', cores=cores, kind='port',
                peak_rss_gb=round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20, 1),
                sample=f'one training step of the oracle port at batch 1 x seq_len 4 (BASELINE configs[0]; 4 frames) after one '
                       f'warm-up step at batch 1 x seq_len 2; {sum(times):.1f} s of CPU work in all; the timed step: {dt:.1f} s = '
                       f'{frames_per_s:.3f} frames/s; value = frames/s / 10 (one sample = 10 frames)')


def run_extension(name, dev, batch, s, steps=5, warmup=2):
    """One extension workload (no reference code for these sizes / this arithmetic: parity unpinned, own oracle only,
    tests/test_extension.py): a fresh trainer, `warmup` untimed steps, `steps` steps between HIP events.
    rv2048 = the 64 x 2048 range view north_star names, vox256 = the 256 x 256 x 64 voxel grid of BASELINE configs[4],
    bf16 = base_1d sizes with ONE bf16 product per fp32 product (the reference's shipped '16-mixed' arithmetic)."""
    import gc
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.data.synthetic import make_batch
    from muvo_amd.trainer import WorldModelTrainer
    ext, sizes = {}, {}
    if name == 'rv2048':
        ext, sizes = {'MODEL.CONSTANT_SIZE.LIDAR': [1, 32]}, dict(range_hw=(64, 2048))
    elif name == 'vox256':
        ext, sizes = {'MODEL.CONSTANT_SIZE.VOXEL': [4, 4, 1]}, dict(voxel=(256, 256, 64))
    old_mode = ops.get_conv_mode()
    if name == 'bf16':
        ops.set_conv_mode(ops.CONV_BF16)
    try:
        cfg = base_1d_cfg(RECEPTIVE_FIELD=min(6, s), FUTURE_HORIZON=s - min(6, s), BATCHSIZE=batch, STEPS=100000, **ext)
        torch.manual_seed(1234)
        tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
        tr.train()
        opts, scheds = tr.configure_optimizers()
        opt, sched = opts[0], scheds[0]['scheduler']
        batches = [make_batch(batch, s, seed=1234 + k, device=dev, **sizes) for k in range(2)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        for i in range(warmup + steps):
            if i == warmup:
                ev[0].record()
            opt.zero_grad()
            loss = tr.training_step(dict(batches[i % 2]), i)
            loss.backward()
            tr.on_after_backward()
            opt.step()
            sched.step()
            if i >= warmup:
                ev[i - warmup + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
        res = dict(ms_per_step=ev[0].elapsed_time(ev[steps]) / steps, median_ms_per_step=ms[len(ms) // 2], steps=steps, warmup=warmup,
                   value=batch / (ev[0].elapsed_time(ev[steps]) / steps * 1e-3), unit='samples/s', parity='unpinned',
                   final_loss=float(loss.item()),
                   what={'rv2048': '64 x 2048 range view (MODEL.CONSTANT_SIZE.LIDAR = [1, 32]), bf16x3',
                         'vox256': '256 x 256 x 64 voxel grid (MODEL.CONSTANT_SIZE.VOXEL = [4, 4, 1]), bf16x3',
                         'bf16': 'base_1d sizes, large contractions with ONE bf16 product (muvo_conv_set_products(1))'}[name])
    finally:
        ops.set_conv_mode(old_mode)
    del tr, opt, sched, opts, scheds, batches, loss
    gc.collect()
    torch.cuda.empty_cache()
    return res


# the parameter store holds 176 M floats: a fixed sample of this many positions is written (48 MB)
DUMP_SAMPLE = 12 * 2 ** 20


def dump_outputs(path, tr, loss):
    """What a caller of the training step holds after the last timed step, as float64 / float32 .npy files: loss.npy (the
    returned total), loss_<term>.npy (the logged loss terms), params.npy (the updated parameters at DUMP_SAMPLE positions of the
    flat parameter store, drawn from a generator seeded with 1234, in ascending order: the same positions in every run of the same
    model).  The gradients are not written: with float atomics in the reductions single gradient entries differ by up to a few
    percent of the largest from run to run, while the updated parameters agree to ~1e-5."""
    import re
    import numpy as np
    os.makedirs(path, exist_ok=True)
    out = {'loss': loss.detach().double().reshape(1)}
    for k, v in sorted(tr.last_losses.items()):
        out['loss_' + re.sub(r'[^A-Za-z0-9_.-]', '_', k)] = v.double().reshape(-1)
    flat = tr.store.flat_param
    if flat.numel() > DUMP_SAMPLE:
        g = torch.Generator().manual_seed(1234)
        flat = flat[torch.randint(flat.numel(), (DUMP_SAMPLE,), generator=g).sort().values.to(flat.device)]
    out['params'] = flat.float()
    for name, t in out.items():
        np.save(os.path.join(path, name + '.npy'), t.cpu().numpy())


def dry_run(args):
    """`python bench.py --gpus N --dry-run`: everything of the N-rank run that does not need a GPU, on CPU over gloo - launched
    exactly like the real run (self-launch through torch.distributed.run or the driver's launcher; RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* from the environment), replicated initial weights (seed 1234) and per-rank data seeds (1234 + 7919 * rank), the REAL
    ParamStore / SegmentedGradReducer with backward hooks on a toy model whose sub-module names are the real segment prefixes,
    barrier + max-over-ranks timing, rank 0 prints one JSON line of the same shape.  NOT a measurement (`dry_run: true`)."""
    import torch.distributed as dist
    from muvo_amd.parallel import SegmentedGradReducer
    from muvo_amd.param_store import ParamStore
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.set_num_threads(1)
    if world > 1:
        dist.init_process_group('gloo')
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'
    assert 0 <= local_rank < max(world, 1)

    class Toy(torch.nn.Module):
        def __init__(self, d=32):
            super().__init__()
            L = torch.nn.Linear
            self.encoder, self.range_view_encoder, self.transformer_encoder = L(d, d), L(d, d), L(2 * d, d)
            self.rssm, self.policy = L(d, d), L(d, 2)
            self.rgb_decoder, self.lidar_re, self.voxel_decoder = L(d, 3 * d), L(d, 2 * d), L(d, d)
            self.encoder_layer = L(d, d)          # registered, never used (reference: mile.py:96)

    torch.manual_seed(1234)                       # replicated initial weights
    m = Toy()
    store = ParamStore(m)
    red = SegmentedGradReducer(store)
    torch.manual_seed(1234 + 7919 * rank)         # data / noise differ per rank from here on
    batches = [torch.randn(args.batch * args.seq_len, 32) for _ in range(2)]

    def step(i):
        x = batches[i % 2]
        red.begin_step()
        store.zero_grad()
        img = torch.tanh(m.encoder(x))
        rv = torch.tanh(m.range_view_encoder(x))
        tok = torch.cat([img, rv], 1)
        tok.register_hook(lambda g: red.segment_done('fusion'))            # d(tokens) arrives: fusion (and everything before) is complete
        emb = torch.tanh(m.transformer_encoder(tok))
        emb.register_hook(lambda g: red.segment_done('rssm'))
        state = torch.tanh(m.rssm(emb))
        state.register_hook(lambda g: red.segment_done('policy'))
        # decoders recorded in the order of muvo_amd/models/mile.py (voxel, range view, RGB): backward completes RGB first
        sv = state + 0
        sv.register_hook(lambda g: red.segment_done('voxel_decoder'))
        lv = m.voxel_decoder(sv).pow(2).mean()
        sl = state + 0
        sl.register_hook(lambda g: red.segment_done('lidar_re'))
        ll = m.lidar_re(sl).pow(2).mean()
        sr = state + 0
        sr.register_hook(lambda g: red.segment_done('rgb_decoder'))
        lr_ = m.rgb_decoder(sr).pow(2).mean()
        loss = lv + ll + lr_ + m.policy(state).abs().mean()
        loss.backward()
        red.finish()
        with torch.no_grad():
            store.flat_param.add_(store.flat_grad, alpha=-1e-2 * red.grad_scale)
        return loss.detach()

    for i in range(args.warmup):
        step(i)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(args.warmup + i)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    log = list(red.launch_log)
    t = torch.tensor([dt, float(loss), float(store.flat_param.double().sum()), float(store.flat_param.double().abs().sum())], dtype=torch.float64)
    if world > 1:
        gathered = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
    else:
        gathered = [t]
    if rank == 0:
        dt = max(float(g[0]) for g in gathered)
        losses = [float(g[1]) for g in gathered]
        sums = {(float(g[2]), float(g[3])) for g in gathered}
        out = {'metric': 'world-model training samples/sec (seq_len=10)', 'value': args.batch * world * args.steps / dt, 'unit': 'samples/s',
               'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': dt / args.steps * 1e3,
               'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
               'dry_run': True,
               'config': {'workload': 'DRY RUN on CPU over gloo: toy model with the real segment names - launch, seeds, timing protocol and '
                                      'gradient exchange only, not a measurement', 'global_batch': args.batch * world,
                          'seq_len': args.seq_len, 'parallelism': f'dp{world}'},
               'n_ranks_seen': dist.get_world_size() if dist.is_initialized() else 1,
               'per_rank_final_loss': losses, 'per_rank_losses_distinct': len({round(v, 9) for v in losses}) == world,
               'params_identical_across_ranks': len(sums) == 1,
               'gradient_exchange': {'segments': {name: dict(mbytes=round((b - a) * 4 / 2 ** 20, 6), from_hook=dict(log).get(name))
                                                  for name, a, b in store.segment_ranges},
                                     'order': [n for n, _ in log], 'grad_scale': red.grad_scale}}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--seq-len', type=int, default=10)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-kernel-timing', action='store_true')
    ap.add_argument('--no-exact-f32', action='store_true', help='skip the extra exact-fp32 steps after the timed region')
    ap.add_argument('--conv-mfma', default=os.environ.get('MUVO_CONV_MFMA', 'bf16x3'), choices=['f32', 'bf16x3', 'bf16'],
                    help='matrix-pipe arithmetic of the large convolutions (DESIGN.md section 5)')
    ap.add_argument('--layer-table', default='', help='write the per-layer conv timing table to this file')
    ap.add_argument('--workload', default='base_1d', choices=['base_1d', 'rv2048', 'vox256'],
                    help='base_1d: BASELINE.json configs[1] (the judged line).  Extensions through MODEL.CONSTANT_SIZE (no reference '
                         'implementation, parity unpinned): rv2048 = the 64 x 2048 range view north_star names; vox256 = the '
                         '256 x 256 x 64 voxel grid of configs[4] (use with --batch 8 --seq-len 12 for that configuration)')
    ap.add_argument('--dry-run', action='store_true',
                    help='CPU rehearsal of the multi-rank control flow (no GPU, no measurement): the same self-launch, environment, seeds, '
                         'barrier / max-over-ranks timing and segmented gradient exchange over gloo on a toy model whose parameter '
                         'names follow the real segments (tests/test_bench_dry_run.py)')
    ap.add_argument('--no-extensions', action='store_true',
                    help='skip the extension workloads (rv2048, vox256, single-product bf16: 5 steps each after the judged region)')
    ap.add_argument('--full', action='store_true',
                    help='everything beyond the headline: dominant-class brackets in the timed region, per-class table, exact-fp32 '
                         'steps, extension workloads, CPU baseline (each still switched off by its --no-* option)')
    ap.add_argument('--dump-outputs', default='', metavar='DIR',
                    help='after the timed steps, write what the last one computed to DIR/<name>.npy (bench.py: dump_outputs)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    if args.layer_table and not args.full:
        ap.error('--layer-table needs --full (the table comes from the per-class instrumentation steps)')
    if not args.full:
        # a plain run: set-up, warm-up, the timed steps and the result line, nothing else
        args.no_kernel_timing = args.no_exact_f32 = args.no_extensions = args.no_cpu_baseline = True

    if os.environ.get('MUVO_BENCH_CORES'):
        # what an 8-rank box leaves each rank: restrict this process (and the threads it starts) to that many host cores
        # BEFORE anything touches the GPU (an env switch, not a wrapper process)
        ncore = max(1, int(os.environ['MUVO_BENCH_CORES']))
        os.sched_setaffinity(0, set(sorted(os.sched_getaffinity(0))[:ncore]))

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N` without a launcher: start one rank per GPU through torch.distributed.run as a CHILD
        # process (before anything in this process touches the GPU) and pass its output and exit code through
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    if args.dry_run:
        return dry_run(args)
    import torch.distributed as dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    force_dist = os.environ.get('MUVO_BENCH_FORCE_DIST') == '1'   # one-rank RCCL group: exercises the collective path on one GPU
    if world > 1 or force_dist:
        if world == 1:
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29511')
            os.environ.setdefault('RANK', '0')
            os.environ.setdefault('WORLD_SIZE', '1')
        dist.init_process_group('nccl', device_id=dev)
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'

    from muvo_amd import ops
    ops.set_conv_mode({'bf16x3': ops.CONV_BF16X3, 'bf16': ops.CONV_BF16, 'f32': ops.CONV_F32}[args.conv_mfma])
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.data.synthetic import make_batch
    from muvo_amd.parallel import SegmentedGradReducer
    from muvo_amd.trainer import WorldModelTrainer

    s = args.seq_len
    ext, sizes = {}, {}
    if args.workload == 'rv2048':
        ext, sizes = {'MODEL.CONSTANT_SIZE.LIDAR': [1, 32]}, dict(range_hw=(64, 2048))
    elif args.workload == 'vox256':
        ext, sizes = {'MODEL.CONSTANT_SIZE.VOXEL': [4, 4, 1]}, dict(voxel=(256, 256, 64))
    cfg = base_1d_cfg(RECEPTIVE_FIELD=min(6, s), FUTURE_HORIZON=s - min(6, s), BATCHSIZE=args.batch, STEPS=100000, **ext)
    torch.manual_seed(1234)  # same initial weights on every rank (replicated data parallel)
    tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    tr.train()
    opts, scheds = tr.configure_optimizers()
    opt, sched = opts[0], scheds[0]['scheduler']
    fake_peers = int(os.environ.get('MUVO_DP_FAKE_PEERS', '0')) if world == 1 else 0
    if tr._reducer is None and (force_dist or fake_peers > 1):
        # one-rank RCCL group / stand-in kernel with a collective's footprint: same wiring as WorldModelTrainer._attach_reducer
        tr._reducer = SegmentedGradReducer(tr.store, force_collectives=force_dist, fake_peers=fake_peers)
        tr.model.segment_done = tr._reducer.segment_done
    assert (tr._reducer is not None) == (world > 1 or force_dist or fake_peers > 1)
    if tr._reducer is not None:
        tr._reducer.timing = True             # per-segment all-reduce time and exposed (not overlapped) time in the JSON line
        if os.environ.get('MUVO_DP_OVERLAP') == '0':
            tr._reducer.overlap = False       # A/B: every segment sent after backward
    torch.manual_seed(1234 + 7919 * rank)    # RSSM noise / use-prior coins differ per rank from here on

    # two distinct synthetic batches per rank, staged in HBM before the timed region
    batches = [make_batch(args.batch, s, seed=1234 + 2 * rank + k, device=dev, **sizes) for k in range(2)]

    def step(i):
        batch = dict(batches[i % 2])
        opt.zero_grad()
        loss = tr.training_step(batch, i)      # begins the reducer's step; backward hooks launch the segment all-reduces
        loss.backward()
        tr.on_after_backward()                 # sends what is left, optimizer stream waits for the side stream
        opt.step()
        sched.step()
        return loss

    # inside the timed region only the dominant kernel class is bracketed with HIP events (roofline object); the per-class
    # table and the layer table come from two extra, untimed steps after it.  The last warm-up step runs with the brackets on:
    # it counts them, and the timed region's events are created (and recorded once) before it starts (ops.KernelTiming)
    dominant = 'bf16x3_implicit_gemm' if args.conv_mfma in ('bf16x3', 'bf16') else 'f32_implicit_gemm'
    probe = None
    pool_reserved = 0
    for i in range(args.warmup):
        if i == args.warmup - 1 and not args.no_kernel_timing:
            probe = ops.KERNEL_TIMING = ops.KernelTiming(only=dominant)
        step(i)
        if i == 0 and os.environ.get('MUVO_POOL_RESERVE', '1') != '0':
            # the caching allocator's per-stream pools sized after the first step (ops.reserve_memory_pools): 14-16 -> 2-3 hipMalloc
            # calls inside the timed region, same step time (75.8-76.1 ms either way); MUVO_POOL_RESERVE=0: off
            torch.cuda.synchronize()
            pool_reserved = ops.reserve_memory_pools(dev)
    ops.KERNEL_TIMING = None
    if not args.no_kernel_timing:
        per_step = 2 * len(probe.rec) if probe is not None else 800
        probe = None
        ops.KERNEL_TIMING = ops.KernelTiming(only=dominant, prealloc=per_step * ((args.steps + BRACKET_EVERY - 1) // BRACKET_EVERY) + 64)
    if world > 1 or force_dist:
        dist.barrier()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    if tr._reducer is not None:
        tr._reducer._steps_timed = []          # exchange timing: the timed steps only
        tr._reducer.host_s = 0.0
    # no cyclic-GC pass inside the timed region: the host is at most ~0.4 steps ahead of the GPU (kernel-argument pool of the
    # queue), so a generation-2 collection over the module / autograd objects (tens of ms) stalls the
    # device; reference counting frees the step's tensors as before
    import gc
    gc.collect()
    gc.disable()
    ms0 = torch.cuda.memory_stats()
    c0 = time.process_time()
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        if ops.KERNEL_TIMING is not None:
            ops.KERNEL_TIMING.enabled = i % BRACKET_EVERY == 0
        loss = step(args.warmup + i)
        marks[i + 1].record()                  # stream-side step boundaries (no host sync): median step time
    host_issue_ms = (time.perf_counter() - t0) / args.steps * 1e3      # until everything is queued (no sync inside the loop)
    host_cpu_ms = (time.process_time() - c0) / args.steps * 1e3        # CPU time of this process (all threads) per step
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()
    ms1 = torch.cuda.memory_stats()
    # hipMalloc / hipFree calls of the caching allocator inside the timed region: without the reservation above its per-stream pools
    # still grow after five warm-up steps (blocks freed on one stream while another still reads them come back late)
    alloc_delta = {k: int(ms1.get(k, 0) - ms0.get(k, 0)) for k in ('num_device_alloc', 'num_device_free', 'num_alloc_retries')}
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tr, loss)   # before any step of --full changes the parameters
    step_ms_seq = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
    step_ms = sorted(step_ms_seq)
    median_ms = step_ms[len(step_ms) // 2] if len(step_ms) % 2 else 0.5 * (step_ms[len(step_ms) // 2 - 1] + step_ms[len(step_ms) // 2])
    timing = ops.KERNEL_TIMING
    ops.KERNEL_TIMING = None
    dp_report = tr._reducer.timing_report() if tr._reducer is not None else None
    if tr._reducer is not None:
        tr._reducer.timing = False
    full_timing, extra_steps = None, 2
    loss_val = float(loss.item())
    del loss       # the last timed step's graph (its AccumulateGrad nodes live on the side streams) must not outlive the switch below:
    #                autograd otherwise warns about a stream mismatch in the first instrumentation step (tools/dev/accgrad_params.py)
    if timing is not None:
        # per-class table from extra steps with the side streams OFF: next to each other on several streams the kernels share
        # the chip and every event bracket also contains its neighbours' work, so the isolated durations are the ones that say
        # how good a kernel is (the timed region above runs with the streams on; its brackets of the dominant class are
        # reported as roofline.achieved / frac, the isolated figures as roofline.achieved_isolated / frac_isolated)
        streams_were = (ops.STREAMS, ops.WGRAD_STREAM)
        ops.STREAMS = ops.WGRAD_STREAM = False
        step(args.warmup + args.steps)            # one untimed step for the per-stream scratch of the main stream
        full_timing = ops.KERNEL_TIMING = ops.KernelTiming()
        for i in range(extra_steps):
            step(args.warmup + args.steps + 1 + i)
        torch.cuda.synchronize()
        ops.KERNEL_TIMING = None
        ops.STREAMS, ops.WGRAD_STREAM = streams_were
    if world > 1:
        t = torch.tensor([dt, median_ms], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt, median_ms = t[0].item(), t[1].item()
    # the same step with every contraction on exact-fp32 MFMA, a few steps after the timed region
    exact_f32 = None
    if args.conv_mfma == 'bf16x3' and not args.no_exact_f32:
        ops.set_conv_mode(ops.CONV_F32)
        step(10_000)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        for i in range(3):
            step(10_001 + i)
            ev[i + 1].record()
        torch.cuda.synchronize()
        f32_ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(3))[1]
        if world > 1:
            t = torch.tensor([f32_ms], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            f32_ms = t.item()
        exact_f32 = dict(ms_per_step=f32_ms, value=args.batch * world / (f32_ms * 1e-3), unit='samples/s', steps=3,
                         note='median of 3 steps after 1 warm-up with MUVO_CONV_MFMA=f32 (v_mfma_f32_32x32x2_f32 everywhere)')
        ops.set_conv_mode(ops.CONV_BF16X3)

    if rank == 0:
        ms = dt / args.steps * 1e3
        samples = args.batch * world * args.steps
        frames_per_gpu_step = args.batch * s
        out = {
            'metric': 'world-model training samples/sec (seq_len=10)', 'value': samples / dt, 'unit': 'samples/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': {'f32': 'f32', 'bf16x3': 'f32 storage/accumulate; large contractions (convolutions, transformer Linear) as bf16x3 split products',
                      'bf16': 'f32 storage/accumulate; large contractions with bf16 operands, ONE product (extension: not the fp32 parity arithmetic)'}[args.conv_mfma],
            'data': 'synthetic',
            'peak_hbm_gb': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
            'config': {'workload': f'base_1d (resnet18 + range-view + transformer fusion + 1D latent), batch={args.batch} '
                                   f'per GPU, seq_len={s}, 600x960 RGB (crop 320x832) + 64x{sizes.get("range_hw", (64, 1024))[1]} range-view + '
                                   f'{"x".join(str(v) for v in sizes.get("voxel", (192, 192, 64)))} voxels, full step incl. 21 losses, backward, AdamW'
                                   + ('' if args.workload == 'base_1d' else f' [EXTENSION {args.workload}: MODEL.CONSTANT_SIZE, no reference code]'),
                       'global_batch': args.batch * world, 'seq_len': s, 'parallelism': f'dp{world}',
                       'conv_mfma': args.conv_mfma},
            'parity': ('pinned by reference fixtures (tests/golden)' if (args.workload == 'base_1d' and args.conv_mfma != 'bf16')
                       else 'unpinned (extension, own oracle only)'),
            'median_ms_per_step': median_ms, 'value_at_median': args.batch * world / (median_ms * 1e-3),
            'step_ms': [round(v, 2) for v in step_ms_seq],     # rank 0's stream-side step times, in order (outliers are host stalls)
            'allocator_calls_in_timed_region': alloc_delta, 'pool_reserved_gb': round(pool_reserved / 2 ** 30, 1),
            'frames_per_s': samples * s / dt,
            'step_tflops_per_gpu': (GFLOP_PER_FRAME * frames_per_gpu_step / (ms * 1e-3) / 1e3) if args.workload == 'base_1d' else None,
            'final_loss': loss_val,
            # host side of a step: wall time until the step is queued / CPU time of the process.  Both include the time the
            # launching threads spin on a full HIP queue: with the GPU work shrunk (batch 1 x 2 frames, same launch count) the
            # same loop issues a step in 23 ms (tools/host_issue_time.py 1 2, profiles/r03a_host_issue.txt)
            'host_issue_ms': host_issue_ms, 'host_cpu_ms': host_cpu_ms,
            'n_ranks_seen': dist.get_world_size() if dist.is_initialized() else 1,
            'rccl_version': '.'.join(str(v) for v in torch.cuda.nccl.version()) if (world > 1 or force_dist) else None,
        }
        # whole-step fractions: all 15.89 TFLOP of the step against (a) the ceiling of ANY three-product bf16 scheme
        # (2500 / 3 TFLOP/s) and (b), for the exact-fp32 run, the fp32 matrix peak
        out['step_frac_of_bf16x3_ceiling'] = (out['step_tflops_per_gpu'] / (2500.0 / 3.0)
                                              if (args.conv_mfma == 'bf16x3' and args.workload == 'base_1d') else None)
        if args.conv_mfma == 'f32' and args.workload == 'base_1d':
            out['step_frac_fp32_exact'] = out['step_tflops_per_gpu'] / 157.3
        if dp_report is not None:
            out['gradient_exchange'] = dp_report     # rank 0's view: per-segment RCCL time, bus bandwidth, exposed time
            if fake_peers > 1:
                dp_report['fake_peers'] = fake_peers
                dp_report['fake_peers_calibration'] = ops.fake_allreduce_calibration()
                dp_report['note'] = ('one GPU: every segment all-reduce replaced by muvo_fake_allreduce (a kernel with a ring '
                                     "collective's local footprint at the xGMI rate, values unchanged) on the communication stream")
        if exact_f32 is not None:
            exact_f32['step_tflops_per_gpu'] = GFLOP_PER_FRAME * frames_per_gpu_step / (exact_f32['ms_per_step'] * 1e-3) / 1e3
            out['exact_f32'] = exact_f32
            out['step_frac_fp32_exact'] = exact_f32['step_tflops_per_gpu'] / 157.3 if args.workload == 'base_1d' else None
        if full_timing is not None and args.layer_table:
            with open(args.layer_table, 'w') as f:
                f.write(full_timing.layer_table() + '\n')
        if timing is not None:
            out['roofline'], _ = timing.summary()                      # dominant class, events inside the timed region
            if out['roofline'] is not None:
                out['roofline']['bracketed_steps'] = (f'every {BRACKET_EVERY}th step of the timed region '
                                                      f'({(args.steps + BRACKET_EVERY - 1) // BRACKET_EVERY} of {args.steps})')
            iso, out['kernel_classes'] = full_timing.summary()         # every class, from the extra untimed steps (streams off)
            if out['roofline'] is not None and iso is not None and iso['kernel'] == out['roofline']['kernel']:
                out['roofline']['achieved_isolated'] = iso['achieved']
                out['roofline']['frac_isolated'] = iso['frac']
                out['roofline']['avg_launch_us_isolated'] = iso['avg_launch_us']
                out['roofline']['isolation_note'] = ('achieved / frac: HIP-event brackets inside the timed region, where the class shares the '
                                                     'chip with kernels of the side streams (muvo_amd/ops.py: branch, wgrad_stream); '
                                                     '*_isolated: the same brackets in extra steps with MUVO_STREAMS off')
            out['side_streams'] = dict(enabled=bool(streams_were[0]), branches=sorted(ops.BRANCHES), wgrad_stream=bool(streams_were[1]),
                                       budget=ops.STREAM_BUDGET[0], hw_queues=os.environ.get('GPU_MAX_HW_QUEUES'),
                                       hw_queues_state=muvo_amd.hw_queue_state(), side_priority=dict(ops.SIDE_PRIORITY))
            out['kernel_class_steps'] = extra_steps
            if out['roofline'] is not None:
                conv_s = sum(c['seconds'] for c in out['kernel_classes'].values())
                dom_s = sum(c['seconds'] for k, c in out['kernel_classes'].items() if k.split(':')[0] == dominant)
                out['roofline']['share_of_conv_time'] = dom_s / max(conv_s, 1e-12)
            if out['roofline'] is not None:
                # clock probe of the dominant kernel (workgroup 0 of the most recent eight-wave launch, include/muvo_hip.h):
                # the class runs power-limited below the 2.4 GHz the peak is quoted at
                import ctypes
                mhz, usk = ctypes.c_double(0.0), ctypes.c_double(0.0)
                if ops.lib().muvo_bf3_loop_clock(ctypes.byref(mhz), ctypes.byref(usk)) == 0 and mhz.value > 0:
                    r = out['roofline']
                    r['shader_clock_mhz_under_load'] = mhz.value
                    r['peak_at_that_clock'] = r['peak'] * mhz.value / 2400.0
                    r['frac_at_that_clock'] = r['achieved'] / r['peak_at_that_clock']
                    # one K step of a workgroup = 24 MFMA 32x32x16 (8 passes = 32 clocks each) per wave, two waves per SIMD
                    r['k_loop_mfma_busy'] = 24 * 32 * 2 / (usk.value * mhz.value)
                    r['clock_note'] = 'shader clock and time per K step measured by workgroup 0 of the last eight-wave launch with >= 2048 workgroups (s_memtime / s_memrealtime)'
            # HBM-side bytes per launch of the dominant class: PMC counters cannot be read from inside this process, so the
            # figure comes from the committed rocprofv3 --pmc passes over this same command (tools/pmc_step.sh)
            import glob
            files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'r*_hbm_traffic.json')))
            if out['roofline'] is not None and files:
                tf = files[-1]                       # the latest round's measurement
                pm = json.load(open(tf))
                psteps = pm.get('steps_profiled', 3)         # tools/pmc_step.sh: bench.py --steps 2 --warmup 1
                for cname, c in pm['classes'].items():
                    if ops.KERNEL_NAMES.get(cname) == out['roofline']['kernel']:
                        r = out['roofline']
                        r['traffic'] = c['hbm_bytes_per_launch']
                        r['traffic_unit'] = ('bytes per kernel DISPATCH (FETCH_SIZE x2 + WRITE_SIZE, includes Infinity-Cache hits); '
                                             '`launches` / `algorithmic_bytes` count sub-pixel phases, of which a merged dispatch '
                                             'carries several: compare the per-step totals below')
                        r['traffic_source'] = (f'profiles/{os.path.basename(tf)} (tools/pmc_step.sh) - a STORED rocprofv3 --pmc profile of '
                                               f'this command, not measured in this run: PMC counters cannot be read in-process')
                        r['traffic_bytes_per_step'] = c['hbm_bytes_per_launch'] * c['dispatches'] / psteps
                        r['algorithmic_bytes_per_step'] = r['algorithmic_bytes'] * r['launches'] / args.steps
                        r['traffic_over_algorithmic'] = r['traffic_bytes_per_step'] / max(r['algorithmic_bytes_per_step'], 1.0)
        if 'kernel_classes' in out:
            # every class against the HBM roof as well (algorithmic bytes: both activation tensors + the weight, fp32, each touched
            # once per operation): the voxel class (8 / 16 channels) is the one where this is the tighter roof
            for c in out['kernel_classes'].values():
                c['hbm_gbs'] = c['algorithmic_gb'] / max(c['seconds'], 1e-12)
                c['hbm_frac'] = c['hbm_gbs'] / 8000.0
            vox = {k: c for k, c in out['kernel_classes'].items() if k.startswith('vox_bf16x3')}
            if vox:
                sec, gb, tf = (sum(c[k] for c in vox.values()) for k in ('seconds', 'algorithmic_gb', 'tflop'))
                out['voxel_class'] = dict(ms_per_step=sec / extra_steps * 1e3, algorithmic_gb_per_step=gb / extra_steps,
                                          hbm_gbs=gb / max(sec, 1e-12), hbm_frac=gb / max(sec, 1e-12) / 8000.0,
                                          ms_at_hbm_roof=gb / extra_steps / 8000.0 * 1e3,
                                          mfma_frac=3.0 * tf / max(sec, 1e-12) / 2500.0)
                # by level of the voxel decoder (input size of the convolution): until round 4 the class held the 192 and 96 levels only
                import re
                lv = {}
                for cls, _fl, _ln, e0, e1, tag, _nb in full_timing.rec:
                    if cls.startswith('vox_bf16x3'):
                        m = re.search(r'in\(([^)]*)\)', tag)
                        key = 'x'.join(v.strip() for v in m.group(1).split(',')) if m else 'other'
                        lv[key] = lv.get(key, 0.0) + e0.elapsed_time(e1) / extra_steps
                out['voxel_class']['ms_per_step_by_level'] = {k: round(v, 3) for k, v in sorted(lv.items())}
        if out.get('roofline') is not None:
            out['roofline']['frac_is'] = ('in situ: HIP-event brackets inside the timed region, side streams on (a bracket also contains the '
                                          "neighbours' share of the chip); frac_isolated = the kernel figure (same brackets, side streams off)")
        if (world == 1 and args.workload == 'base_1d' and args.conv_mfma == 'bf16x3' and not args.no_extensions
                and not args.no_kernel_timing):       # (the reduced command lines of the A/B and profiling scripts skip them)
            # (the judged trainer, its optimizer state and the last step's autograd graph go first: 70 GB peak otherwise doubles)
            del batches, tr, opt, sched, opts, scheds
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            out['extensions'] = {}
            for name in ('rv2048', 'vox256', 'bf16'):
                try:
                    out['extensions'][name] = run_extension(name, dev, args.batch, s)
                except Exception as e:          # an extension must never cost the judged line
                    out['extensions'][name] = dict(error=f'{type(e).__name__}: {e}'[:300], parity='unpinned')
        if world == 1 and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(usable_cores())
        print(json.dumps(out), flush=True)
    if world > 1 or force_dist:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
