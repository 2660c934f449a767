"""CPU self-test of the implicit-GEMM convolution tests (tests/test_conv_kernels_gpu.py); needs no GPU.

  * the dispatch mirror (conv_reference.conv_plan) against the library's host-only queries on every case and direction: family,
    eight-wave variant, pack sizes (sum of Kp * Mp over the phases: pins phases, merging, Cp, Kp, Mp) and the four workspace sizes;
  * launch facts that have no query - tile, split-K ranges, K steps per range, merged groups, K order - pinned as literals, so that
    a policy change fails here and makes its author look at the case again;
  * the matrix reaches every instantiation the launchers can take;
  * the bars separate faults: on the matrix's own layers (spatial size cropped) the CPU emulation of the bf16x3 arithmetic uses at
    most 1 / MARGIN of the bf16x3 bar while a lost cross product (everywhere, on one tap, on one K range of a split-K launch)
    exceeds it SEPARATION times; the serial fp32 chain uses at most 1 / MARGIN of the fp32 bar of its reduction length while the
    bf16x3 arithmetic exceeds that bar SEPARATION times (a kernel that silently runs bf16x3 where fp32 was asked for fails)."""
import ctypes
import math

import pytest
import torch

import conv_reference as R
from test_conv_kernels_gpu import (BF3, CASES, HEAD_CASES, OPS, PW_CASES, SPLIT_K, WGRAD_BF3_IN_F32, Case, conv_mode,
                                   library_answers)

MARGIN, SEPARATION = 2.0, 4.0


# ------------------------------------------------------------------------------------------------ mirror against the library
def _library(case, det=False):
    from muvo_amd import ops
    layer, n, in_sz = case.layer, case.n, case.in_sz
    with conv_mode(case.mode, det):
        geom = ops.ConvGeom(layer.nd, layer.transposed, layer.cin, layer.cout, layer.k, layer.stride, layer.pad, 1, layer.out_pad)
        pl = geom.plan(n, (1,) + in_sz if layer.nd == 2 else in_sz)
        fam, var = library_answers(geom, n, in_sz)
        return dict(family=fam, variant=var, pack_fwd=pl.pack_fwd, pack_dgrad=pl.pack_dgrad,
                    ws=(pl.ws_fwd_x, pl.ws_dgrad_dy, pl.ws_wgrad_x, pl.ws_wgrad_dy))


ALL_GEMM_CASES = CASES + WGRAD_BF3_IN_F32


@pytest.mark.parametrize('case', ALL_GEMM_CASES, ids=[c.id for c in ALL_GEMM_CASES])
def test_mirror_matches_library(case):
    for det in (False, True):
        assert R.layer_answers(case.layer, case.n, case.in_sz, case.mode, det) == _library(case, det), f'deterministic = {det}'


def test_mirror_head_and_pw_shapes():
    from muvo_amd import ops
    for case in PW_CASES:
        assert all(R.conv_plan(case.layer, case.n, case.in_sz, op, case.mode) is None for op in OPS)
        assert _library(case)['family'] == (3, 3, 3)
    for layer, n, in_sz, co, _ in HEAD_CASES:
        c = Case(layer, n, in_sz, R.ACT_ELU, BF3, '')
        assert R.layer_answers(layer, n, in_sz, BF3) == _library(c)
        with conv_mode(BF3):
            geom = ops.ConvGeom(2, 1, layer.cin, layer.cout, layer.k, layer.stride, layer.pad, 1, layer.out_pad)
            d = geom.plan(n, (1,) + in_sz)[0]
            assert ops.lib().muvo_conv_forward_head_supported(ctypes.byref(d), co) == 1
        p = R.conv_plan(layer, n, in_sz, 'fwd', BF3)['phases'][0]
        assert p['tile'] == (256, 128) and p['ksplit'] == 1 and p['Msub'] == layer.cout and p['nmerge'] == 4


def test_voxel_shapes_are_not_mirrored():
    """3x3x3 layers the voxel kernels serve are theirs (tests/test_vox_kernels_gpu.py); the 27-tap case of this matrix is not"""
    assert R.conv_plan(R.Layer('conv3d', 16, 8, 3, 1, 1, 0), 2, (4, 8, 32), 'fwd', BF3) is None
    assert R.conv_plan(R.Layer('conv3d', 40, 32, 3, 1, 1, 0), 2, (3, 5, 7), 'fwd', BF3) is not None


# ------------------------------------------------------------------------------------------------ pinned launch facts
def facts(case, det=False):
    """per direction: 'tile / K ranges x steps / merged groups / K order' of each launch ('!' marks a finishing bias / activation
    pass; weight gradient: tile / pixel ranges x steps / merged groups / unpack)"""
    out = []
    for op in OPS:
        p = R.conv_plan(case.layer, case.n, case.in_sz, op, case.mode, det)
        ph = []
        for i, q in enumerate(p['phases']):
            if op == 'wgrad':
                last = ('b3' if q['kernel'].endswith('true>') else 'f32') if not q['bf3'] else p['unpack'][i][:4]
                name = ('pp' if '_pp_' in q['kernel'] else ('bf3' if q['bf3'] else 'f32'))
            else:
                last = ('in' if q['tap_inner'] else 'out') if q['bf3'] else f'run{4 if q["Cp"] == 4 else 8}'
                name = 'bf3' if q['bf3'] else 'f32'
            ph.append(f'{name} {q["tile"][0]}x{q["tile"][1]} {q["ksplit"]}x{q["steps"]} g{q["nmerge"]} {last}')
        # identical launches are written once with a count
        uniq = []
        for s in ph:
            if uniq and uniq[-1][0] == s:
                uniq[-1][1] += 1
            else:
                uniq.append([s, 1])
        out.append(', '.join(s if k == 1 else f'{k} * ({s})' for s, k in uniq) + (' !' if p['finish'] else ''))
    return tuple(out)


PINNED = {}   # filled below: case id -> (fwd, dgrad, wgrad)


def _pin(cid, fwd, dgrad, wgrad):
    PINNED[cid] = (fwd, dgrad, wgrad)


# (written from facts() on the commit that added these tests)
_pin('32to32k3s1p1-n2-9x7-leaky-bf3',
     'bf3 64x128 1x9 g1 in',
     'bf3 64x128 1x9 g1 in',
     'bf3 32x64 1x4 g1 tile')
_pin('40to48k3s1p1-n3-5x13-elu-bf3',
     'bf3 64x128 1x12 g1 out',
     'bf3 64x128 1x14 g1 out',
     'bf3 64x64 1x7 g1 tile')
_pin('8to64k5s1p2-n2-12x11-relu-bf3',
     'bf3 64x128 1x7 g1 out',
     'f32 32x128 12x9 g1 run8 !',
     'f32 128x64 3x3 g1 f32')
_pin('64to128k3s2p1-n2-21x27-leaky-bf3',
     'bf3 64x128 1x18 g1 in',
     'bf3 64x128 1x4 g1 out, 2 * (bf3 64x128 1x8 g1 in), bf3 64x128 1x16 g1 in',
     'bf3 128x128 1x10 g1 tile')
_pin('64to128k3s2p1-n2-20x26-none-bf3',
     'bf3 64x128 1x18 g1 in',
     'bf3 64x128 1x16 g4 in',
     'bf3 128x128 1x9 g1 tile')
_pin('64to64k5s2p2-n2-12x12-elu-bf3',
     'bf3 64x128 3x17 g1 in !',
     'bf3 64x128 1x18 g4 in',
     'bf3 64x64 1x3 g1 tile')
_pin('64to48k5s2p2-n2-11x9-relu-bf3',
     'bf3 64x128 3x17 g1 in !',
     'bf3 64x128 1x14 g1 out, 2 * (bf3 64x128 1x9 g1 out), bf3 64x128 1x6 g1 out',
     'bf3 64x64 1x2 g1 tile')
_pin('T64to32k6s2p2-n2-5x13-elu-bf3',
     'bf3 64x128 1x18 g4 in',
     'bf3 64x128 2x18 g1 in !',
     'bf3 128x128 1x5 g4 tile')
_pin('T48to64k4s2p1-n2-6x7-leaky-bf3',
     '4 * (bf3 64x128 1x6 g1 out)',
     'bf3 64x128 2x16 g1 in !',
     '4 * (bf3 64x64 1x3 g1 tile)')
_pin('T160to96k5s2p2o1-n1-4x6-elu-bf3',
     'bf3 64x128 2x23 g4 in !',
     'bf3 64x128 4x19 g1 in !',
     'pp 256x128 1x1 g4 tile')
_pin('136to64k3s1p1-n1-6x7-leaky-bf3',
     'bf3 64x128 2x20 g1 out !',
     'bf3 64x128 1x18 g1 in',
     'bf3 64x256 1x2 g1 tile')
_pin('520to64k3s1p1-n1-5x13-elu-bf3',
     'bf3 64x128 9x17 g1 out !',
     'bf3 64x128 1x18 g1 in',
     'bf3 64x256 1x3 g1 tile')
_pin('48to256k3s2p1-n1-9x11-none-bf3',
     'bf3 64x128 1x14 g1 out',
     'bf3 64x128 2x4 g1 out, 2 * (bf3 64x128 2x8 g1 in), bf3 64x128 2x16 g1 in !',
     'pp 256x128 1x1 g1 tile')
_pin('256to48k3s2p1-n1-9x11-relu-bf3',
     'bf3 64x128 4x18 g1 in !',
     'bf3 64x128 1x2 g1 out, 2 * (bf3 64x128 1x3 g1 out), bf3 64x128 1x6 g1 out',
     'bf3 64x256 1x1 g1 tile')
_pin('32to160k3s1p1-n1-128x128-none-bf3',
     'bf3 256x128 1x9 g1 in',
     'bf3 64x128 2x23 g1 in !',
     'pp 256x128 27x19 g1 tile')
_pin('32to160k3s1p1-n1-127x128-none-bf3',
     'bf3 64x128 1x9 g1 in',
     'bf3 64x128 2x23 g1 in !',
     'pp 256x128 27x19 g1 tile')
_pin('32to96k3s1p1-n2-128x128-none-bf3',
     'bf3 128x256 1x9 g1 in',
     'bf3 64x128 1x27 g1 in',
     'bf3 128x128 28x37 g1 tile')
_pin('32to96k3s1p1-n2-127x128-leaky-bf3',
     'bf3 64x128 1x9 g1 in',
     'bf3 64x128 1x27 g1 in',
     'bf3 128x128 28x37 g1 tile')
_pin('T96to160k6s2p2-n2-64x64-elu-bf3',
     'bf3 256x128 1x27 g4 in',
     'bf3 64x128 4x45 g1 in !',
     'pp 256x128 9x29 g4 tile')
_pin('72to96k3s1p1-n2-7x9-leaky-bf3',
     'bf3 64x128 1x21 g1 out',
     'bf3 64x128 1x27 g1 in',
     'pp 128x256 1x4 g1 tile')
_pin('96to48k3s1p1-n2-7x9-elu-bf3',
     'bf3 64x128 1x27 g1 in',
     'bf3 64x128 1x14 g1 out',
     'bf3 64x128 1x4 g1 tile')
_pin('96to32k3s1p1-n2-23x21-none-bf3',
     'bf3 64x128 1x27 g1 in',
     'bf3 64x128 1x9 g1 in',
     'bf3 64x128 2x16 g1 tile')
_pin('32to64k1s2p0-n2-12x14-none-bf3',
     'bf3 64x128 1x1 g1 out',
     'f32 32x128 1x4 g1 run8, 3 * (f32 32x128 1x0 g1 run8)',
     'bf3 64x64 1x3 g1 elem')
_pin('32to64k1s1p0-n2-12x14-leaky-bf3',
     'bf3 64x128 1x1 g1 out',
     'bf3 64x128 1x2 g1 out',
     'bf3 64x64 1x11 g1 elem')
_pin('3d40to32k3s1p1-n2-3x5x7-elu-bf3',
     'bf3 64x128 2x17 g1 out !',
     'bf3 64x128 1x27 g1 in',
     'bf3 32x64 1x7 g1 tile')
_pin('32to32k3s1p1-n1-33x35-leaky-bf3',
     'bf3 64x128 1x9 g1 in',
     'bf3 64x128 1x9 g1 in',
     'bf3 32x64 3x13 g1 tile')
_pin('160to32k3s1p1-n1-6x7-none-bf3',
     'bf3 64x128 2x23 g1 in !',
     'bf3 64x128 1x9 g1 in',
     'bf3 64x256 1x2 g1 tile')
_pin('3to64k7s2p3-n2-38x50-none-f32',
     'f32 64x128 1x13 g1 run4',
     'f32 32x128 4x9 g1 run8, 2 * (f32 32x128 6x8 g1 run8), f32 32x128 8x8 g1 run8 !',
     'f32 128x64 8x4 g1 f32')
_pin('3to96k3s1p1-n1-9x7-leaky-f32',
     'f32 128x128 1x3 g1 run4',
     'f32 32x128 6x9 g1 run8 !',
     'f32 128x128 1x2 g1 f32')
_pin('4to16k3s1p1-n2-5x6-none-f32',
     'f32 32x128 1x3 g1 run4',
     'f32 32x128 1x9 g1 run8',
     'f32 128x32 1x2 g1 f32')
_pin('8to16k3s1p1-n3-9x7-relu-f32',
     'f32 32x128 1x5 g1 run8',
     'f32 32x128 1x9 g1 run8',
     'f32 128x32 2x3 g1 f32')
_pin('20to40k3s1p1-n2-10x13-leaky-f32',
     'f32 64x128 1x18 g1 run8',
     'f32 32x128 1x27 g1 run8',
     'f32 128x64 3x3 g1 f32')
_pin('70to130k3s1p1-n2-6x11-elu-f32',
     'f32 128x128 5x9 g1 run8 !',
     'f32 128x128 10x9 g1 run8 !',
     'f32 128x128 2x3 g1 f32')
_pin('128to64k3s1p1-n1-6x7-elu-f32',
     'f32 64x128 9x8 g1 run8 !',
     'f32 128x128 4x9 g1 run8 !',
     'f32 128x64 1x2 g1 f32')
_pin('T128to32k6s2p2-n1-3x4-leaky-f32',
     'f32 128x128 9x8 g4 run8 !',
     'f32 128x128 9x8 g1 run8 !',
     '4 * (f32 128x32 1x1 g1 f32)')
_pin('T40to24k5s2p2o1-n3-5x13-elu-f32',
     'f32 32x128 1x27 g1 run8, 2 * (f32 32x128 1x18 g1 run8), f32 32x128 1x12 g1 run8',
     'f32 64x128 6x9 g1 run8 !',
     '4 * (f32 128x32 2x4 g1 f32)')
_pin('64to128k3s2p1-n2-20x26-none-f32',
     'f32 128x128 4x9 g1 run8 !',
     'f32 128x128 4x8 g4 run8 !',
     'f32 128x128 3x3 g1 f32')
_pin('24to32k3s1p1-n3-21x19-none-f32',
     'f32 32x128 1x18 g1 run8',
     'f32 32x128 1x18 g1 run8',
     'f32 128x32 10x4 g1 f32')
_pin('24to64k3s1p1-n3-21x19-relu-f32',
     'f32 64x128 1x18 g1 run8',
     'f32 32x128 4x9 g1 run8 !',
     'f32 128x64 10x4 g1 f32')
_pin('24to128k3s1p1-n3-21x19-none-f32',
     'f32 128x128 1x18 g1 run8',
     'f32 32x128 9x8 g1 run8 !',
     'f32 128x128 10x4 g1 f32')
_pin('24to64k7s1p3-n1-116x116-none-bf3',
     'bf3 64x128 2x19 g1 out !',
     'f32 32x128 4x49 g1 run8 !',
     'f32 128x64 106x4 g1 b3')
_pin('24to128k5s1p2-n1-115x115-none-bf3',
     'bf3 64x128 1x19 g1 out',
     'f32 32x128 4x50 g1 run8 !',
     'f32 128x128 104x4 g1 b3')
_pin('31to32k7s1p3-n1-144x144-none-bf3',
     'bf3 64x128 3x17 g1 in !',
     'f32 32x128 3x33 g1 run8 !',
     'f32 128x32 130x5 g1 b3')


def test_pinned_launch_facts():
    ids = [c.id for c in ALL_GEMM_CASES]
    assert sorted(PINNED) == sorted(ids), set(PINNED) ^ set(ids)
    wrong = {c.id: (facts(c), PINNED[c.id]) for c in ALL_GEMM_CASES if facts(c) != PINNED[c.id]}
    assert not wrong, '\n'.join(f'{k}:\n  mirror {a}\n  pinned {b}' for k, (a, b) in wrong.items())


def test_split_k_cases_run_unsplit_in_deterministic_mode():
    assert len(SPLIT_K) >= 8
    for c in SPLIT_K:
        assert any('!' in f for f in facts(c)[:2])
        for f in facts(c, det=True):
            assert '!' not in f and all(' 1x' in s for s in f.split(', ')), (c.id, f)


# ------------------------------------------------------------------------------------------------ reach
# Every instantiation / code path the launchers can take at test sizes.  conv_fwd_kernel: RUN is 4 (Cp == 4) or 8 (Cp == 8, and
# KPT = 16 / (256 / BN) = 8 for all three tiles, whose BN is 128); split-K needs >= 32 K steps of 16, i.e. T * Cp >= 512: with
# Cp == 4 that is more taps than MAX_TAPS, so RUN = 4 has no split-K form.  Out of reach at test sizes: the pointer-store
# epilogue (outputs >= 2 GB), merges refused by the 2048-row cap, and the two-stage eight-wave forward tiles that only
# MUVO_BF3_VARIANT=2 selects (kept for the sake of their neighbours' machine code, conv_bf3.hip: bf3_launch_fwd_phase).  The other
# variants that MUVO_* tuning switches selected have been retired.
REACHABLE = (
    [f'conv_fwd_kernel<{bm},128,run{r}>' for bm in (128, 64, 32) for r in (4, 8)]
    + [f'conv_fwd_kernel<{bm},128,run8> split-K' for bm in (128, 64, 32)]
    + ['bias_act_kernel',
       'conv_bf3_kernel<64,128,1,4,4,2>', 'conv_bf3_kernel<64,128,1,4,4,2> split-K', 'conv_bf3_kernel<128,256,2,4,4,3>',
       'conv_bf3_kernel<256,128,4,2,4,3>', 'bf3 K order: tap inner', 'bf3 K order: taps outermost', 'bf3 merged phase',
       'bf3 plain phase', 'bf3 fused head: one wave per group', 'bf3 fused head: atomic partial logits']
    + [f'conv_wgrad_kernel<128,{bn},{b}>' for bn in (128, 64, 32) for b in ('false', 'true')]
    + ['unpack_wgrad_kernel', 'conv_bf3_wgrad_pp_kernel<256,128>', 'conv_bf3_wgrad_pp_kernel<128,256>',
       'conv_bf3_wgrad_kernel<128,128,2,2,2>', 'conv_bf3_wgrad_kernel<32,64,1,2,2>', 'conv_bf3_wgrad_kernel<64,256,1,4,2>',
       'conv_bf3_wgrad_kernel<64,128,1,2,2>', 'conv_bf3_wgrad_kernel<64,64,1,2,2>', 'bf3_unpack_wgrad_tiled_kernel',
       'bf3_unpack_wgrad_kernel',
       'split: scalar', 'split: v4', 'split: scalar fused dy', 'split: v4 fused dy', 'bias_grad_kernel']
    + [f'pw<{co}>' for co in (1, 2, 3, 4)]
)


def test_matrix_reaches_every_instantiation():
    reached = set()
    for c in ALL_GEMM_CASES:
        ops_run = ('wgrad',) if c in WGRAD_BF3_IN_F32 else OPS
        for op in ops_run:
            reached |= {r for r in R.conv_plan(c.layer, c.n, c.in_sz, op, c.mode)['reach'] if r != 'nchw_split_nhwc'}
        if c in WGRAD_BF3_IN_F32:
            reached.add('bias_grad_kernel')
            continue
        # the split passes: forward splits x itself; backward runs the fused preamble or (run modes b / c, mixed families) plain splits
        s_in, s_out = math.prod(c.in_sz), math.prod(c.layer.out_size(c.in_sz))
        plans = [R.conv_plan(c.layer, c.n, c.in_sz, op, c.mode) for op in OPS]
        if plans[0]['family'] == 1:
            reached.add('split: v4' if s_in % 4 == 0 and s_in >= 1024 else 'split: scalar')
        fused = R.fused_dy_kernel(c.layer, c.n, c.in_sz, c.mode)
        if fused:
            reached.add(f'split: {fused} fused dy')
        if not fused or 'b' in c.marks:
            reached.add('bias_grad_kernel')
            if plans[2]['family'] == 1:
                reached.add('split: v4' if s_out % 4 == 0 and s_out >= 1024 else 'split: scalar')
    for layer, n, in_sz, co, _ in HEAD_CASES:
        reached.add('bf3 fused head: one wave per group' if layer.cout <= 64 else 'bf3 fused head: atomic partial logits')
    reached |= {f'pw<{c.layer.cout}>' for c in PW_CASES}
    missing = sorted(set(REACHABLE) - reached)
    assert not missing, f'no case reaches {missing}'
    assert reached <= set(REACHABLE), sorted(reached - set(REACHABLE))


def test_fused_preamble_kernels():
    """the v4 preamble needs an output size % 4 == 0 and >= 1024: the two cases marked for it take it, the 33 x 35 case falls back"""
    by_id = {c.id: c for c in CASES}
    for cid, want in (('32to96k3s1p1-n2-127x128-leaky-bf3', 'v4'), ('T96to160k6s2p2-n2-64x64-elu-bf3', 'v4'),
                      ('32to32k3s1p1-n1-33x35-leaky-bf3', 'scalar'), ('32to32k3s1p1-n2-9x7-leaky-bf3', 'scalar'),
                      ('8to64k5s1p2-n2-12x11-relu-bf3', None), ('32to64k1s2p0-n2-12x14-none-bf3', None)):
        c = by_id[cid]
        assert R.fused_dy_kernel(c.layer, c.n, c.in_sz, c.mode) == want, cid


# ------------------------------------------------------------------------------------------------ bars separate faults
def _cropped(case):
    """the case's layer at a spatial size cropped to <= 12 per axis (parity kept: odd / even grids plan differently), N <= 2"""
    in_sz = tuple(d if d <= 12 else 12 - (d % 2) for d in case.in_sz)
    return case._replace(n=min(case.n, 2), in_sz=in_sz)


def _operands(case, seed):
    layer = case.layer
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(case.n, layer.cin, *case.in_sz, generator=g)
    fan = layer.weight_shape()[1] * layer.k ** layer.nd
    w = (torch.rand(layer.weight_shape(), generator=g) * 2 - 1) / fan ** 0.5
    dy = torch.randn(case.n, layer.cout, *layer.out_size(case.in_sz), generator=g)
    return x, w, dy


def _legs(case, x, w, dy):
    layer = case.layer
    return {'fwd': (R.ref_forward(layer, x, w), R.gemm_form(layer, 'fwd', x=x, w=w)),
            'dgrad': (R.ref_dgrad(layer, dy, w, x.shape), R.gemm_form(layer, 'dgrad', dy=dy, w=w, in_sz=case.in_sz)),
            'wgrad': (R.ref_wgrad(layer, x, dy), R.gemm_form(layer, 'wgrad', x=x, dy=dy))}


def _reduction(op, plan, g):
    """reduction length of the case's fp32 chain: taps x channels of the longest launch; weight gradient: pixels"""
    return g.a.shape[1] if op == 'wgrad' else max(p['T'] * p['C'] for p in plan['phases'])


WGRAD_ONLY = {c.layer for c in WGRAD_BF3_IN_F32}
BARS_CASES = sorted({_cropped(c) for c in CASES + WGRAD_BF3_IN_F32}, key=lambda c: c.id)


@pytest.mark.parametrize('case', BARS_CASES, ids=[c.id for c in BARS_CASES])
def test_bars_separate_faults(case):
    x, w, dy = _operands(case, 7)
    for op, ((ref, den), g) in _legs(case, x, w, dy).items():
        if case.layer in WGRAD_ONLY and op != 'wgrad':       # those cases check the weight gradient alone
            continue
        plan = R.conv_plan(case.layer, case.n, case.in_sz, op, case.mode)
        stat = lambda form, **kw: R.error_stats(R.emulate_gemm(g, form, **kw), ref, den)      # noqa: E731
        if plan['family'] == 1:
            bar = R.BF3_BAR
            good = R.excess(stat('bf16x3'), bar)
            assert good <= 1 / MARGIN, f'{op}: the bf16x3 emulation uses {good:.2f} of the bar (at most {1 / MARGIN})'
            centre = int(g.taps.max()) // 2
            forms = [('two_products', {}), ('tap_lo_dropped', {'tap': centre})]
            split = [p['ksplit'] for p in plan['phases'] if p['ksplit'] > 1]
            if op != 'wgrad' and split:
                k = g.a.shape[1]
                forms.append(('krange_lo_dropped', {'krange': (0, -(-k // max(split)))}))
            for form, kw in forms:
                bad = R.excess(stat(form, **kw), bar)
                assert bad >= SEPARATION, f'{op}: the faulty form {form} exceeds the bar only {bad:.2f}x'
        else:
            bar = R.f32_bar(_reduction(op, plan, g))
            good = R.excess(stat('f32_chain'), bar)
            assert good <= 1 / MARGIN, f'{op}: the fp32 chain uses {good:.2f} of the fp32 bar {bar} (at most {1 / MARGIN})'
            bad = R.excess(stat('bf16x3'), bar)
            assert bad >= SEPARATION, f'{op}: bf16x3 arithmetic exceeds the fp32 bar only {bad:.2f}x'


def test_krange_fault_is_exercised():
    """the third degraded form runs on the split-K cases of the matrix (forward or data gradient on bf16x3 with K ranges)"""
    n = 0
    for c in BARS_CASES:
        for op in ('fwd', 'dgrad'):
            p = R.conv_plan(c.layer, c.n, c.in_sz, op, c.mode)
            n += p['family'] == 1 and any(q['ksplit'] > 1 for q in p['phases'])
    assert n >= 6, n
