"""Skinny and grouped GEMM paths of csrc/gemm.hip at the model's own shapes: median us per call and the error against float64.
    python tools/skinny_bench.py            (MUVO_HIP_LIB=<other build> for an A/B comparison)"""
import ctypes as C, os, sys, types, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from muvo_amd import ops
dev = torch.device('cuda:0')
torch.manual_seed(0)


def timed(fn, reps=7, calls=50):
    """median over `reps` windows of `calls` back-to-back calls, us per call"""
    fn(); torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls): fn()
        e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / calls)
    return sorted(us)[len(us) // 2]


def rel_err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def row(name, rows, out_f, in_f, route, us, err):
    print(f'{name:<16} {rows:3d} {out_f:6d} {in_f:6d}  {route:<26} {us:9.1f} us/call  rel err {err:.1e}')


print(f'# {ops._LIB_PATH}')
# Linear forward: the k-vector kernel (<= 24 rows: the 2 x 10 frames of a step) and, for a batch of 26 / 32 frames, the k-contiguous one
for rows, out_f, in_f in ((20, 512, 33280), (20, 512, 8192), (20, 128, 1536), (2, 3072, 1024), (20, 16, 1536), (20, 1536, 1536),
                          (32, 512, 1536), (26, 1536, 1536)):
    x = torch.randn(rows, in_f, device=dev); w = torch.randn(out_f, in_f, device=dev) * 0.01; b = torch.randn(out_f, device=dev)
    r = ops.gemm_route(rows, out_f, in_f, in_f, 1, 1, in_f, out_f, True, a_addr=x.data_ptr(), b_addr=w.data_ptr())
    err = rel_err(ops.linear(x, w, b), x.double() @ w.double().t() + b.double())
    row('linear fwd', rows, out_f, in_f, f'{r["kernel"]}<{r["rm"]}>', timed(lambda: ops.linear(x, w, b)), err)
# The n-contiguous kernel.  With its k split: Linear data gradients dx = dz W.  Without (bias and ELU fused): the seed
# ConvTranspose of the rgb / lidar decoders as a GEMM over (channel, 5 x 13 pixel) columns, one bias per channel.
for rows, out_f, in_f, bias_div in ((20, 1536, 1536, 0), (20, 512, 1536, 0), (20, 512, 1056, 0), (20, 512, 33280, 65), (20, 512, 8192, 16)):
    dz = torch.randn(rows, out_f, device=dev); w = torch.randn(out_f, in_f, device=dev) * 0.01; dx = torch.empty(rows, in_f, device=dev)
    b = torch.randn(in_f // bias_div, device=dev) if bias_div else None
    act = ops.ACT_ELU if bias_div else ops.ACT_NONE
    r = ops.gemm_route(rows, in_f, out_f, out_f, 1, in_f, 1, in_f, b is not None, act, a_addr=dz.data_ptr(), b_addr=w.data_ptr())
    dgrad = lambda: ops.gemm(dz, w, dx, rows, in_f, out_f, out_f, 1, in_f, 1, in_f, bias=b, act=act, bias_div=max(bias_div, 1))      # noqa: E731
    dgrad()
    ref = dz.double() @ w.double()
    if bias_div:
        ref = torch.nn.functional.elu(ref + b.double().repeat_interleave(bias_div))
    row('dgrad' if not bias_div else 'seed convT', rows, out_f, in_f, f'{r["kernel"]}<{r["rm"]}> ks {r["ksplit"]}', timed(dgrad), rel_err(dx, ref))
# grouped Linear: the style projections of the voxel decoder's 14 AdaIN layers on the (20, 1536) latent, and a short table
for rows, in_f, ns in ((20, 1536, [1024, 512] + [512] * 6 + [256, 256, 128, 128, 64, 64]), (8, 1536, [128, 64, 16])):
    lins = [types.SimpleNamespace(weight=torch.nn.Parameter(torch.randn(n, in_f, device=dev) * 0.01),
                                  bias=torch.nn.Parameter(torch.randn(n, device=dev))) for n in ns]
    x = torch.randn(rows, in_f, device=dev)
    dys = [torch.randn(rows, n, device=dev) for n in ns]
    ys = ops.grouped_linear(x, lins)
    err = max(rel_err(y, x.double() @ l.weight.detach().double().t() + l.bias.detach().double()) for y, l in zip(ys, lins))
    row('grouped fwd', rows, sum(ns), in_f, f'{len(ns)} layers', timed(lambda: ops.grouped_linear(x, lins)), err)
    # backward through the library entry point (dx, dW, db in one call; through autograd the row would time the host)
    dx, dws, dbs = torch.empty_like(x), [torch.zeros_like(l.weight) for l in lins], [torch.zeros_like(l.bias) for l in lins]
    args = (ops._f(x), rows, in_f, len(ns), ops._ptr_array([l.weight for l in lins]), ops._ptr_array(dys), ops._f(dx), ops._ptr_array(dws),
            ops._ptr_array(dbs), (C.c_int * len(ns))(*ns))
    bwd = lambda: ops._ck(ops.lib().muvo_grouped_linear_bwd(*args, ops._st()))      # noqa: E731
    bwd()
    err = rel_err(dx, sum(d.double() @ l.weight.detach().double() for d, l in zip(dys, lins)))
    row('grouped bwd', rows, sum(ns), in_f, f'{len(ns)} layers, dx err', timed(bwd), err)
