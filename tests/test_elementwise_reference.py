"""CPU: the helpers of tests/elementwise_reference.py are what tests/test_elementwise_kernels_gpu.py takes them for.

  - the Python dispatch mirror equals the library's route queries (host code of the cross-compiled library, no device) over a
    sweep of sizes, batch counts and pointer alignments, and no route with a misaligned pointer names a kernel that accesses
    that pointer with 16-byte instructions;
  - every kernel of the unit is named by a case and every case takes the route it is listed for;
  - the float64 references agree with PyTorch's own CPU operators, the adjoint identity holds;
  - every emulation stays within its bar, the bar tables are not stale;
  - the bars reject the planted faults by a clear factor (printed)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as R

FAULT_FACTOR = 10.0          # a planted fault must exceed its bar by at least this factor


def _ops():
    from muvo_amd import build, ops
    build.build(verbose=False)
    return ops


def _addr(aligned):
    return 0x1000 if aligned else 0x1004


# ================================================================================================ dispatch mirror
def _h_candidates(W):
    hs = {1, 3}
    if W % 4 == 0:
        q = W // 4
        for t in (R._cdiv(128, q), 1024 // q):
            hs |= {t - 1, t, t + 1}
    return sorted(h for h in hs if h > 0)


def test_upsample_mirror_equals_route_and_respects_alignment():
    ops = _ops()
    n = 0
    seen = set()
    for W in range(1, 261):
        for H, D, NC in itertools.product(_h_candidates(W), (1, 8, 15, 16, 17, 33), (1, 2, 4096, 65535, 65536)):
            for backward, in16, out16 in itertools.product((0, 1), (True, False), (True, False)):
                got = ops.upsample3d_route(backward, NC, D, H, W, _addr(in16), _addr(out16))
                want = R.upsample_plan(backward, NC, D, H, W, in16, out16)
                assert got == want, ((backward, NC, D, H, W, in16, out16), got, want)
                need_in, need_out = R.UPSAMPLE_NEEDS16[(backward, got['kernel'])]
                assert (in16 or not need_in) and (out16 or not need_out), ((backward, NC, D, H, W, in16, out16), got)
                assert NC <= 65535 or got['kernel'] == 'scalar'
                seen.add((backward, got['kernel']))
                n += 1
    assert seen == set(R.UPSAMPLE_NEEDS16), seen
    print(f'ELEMSTAT upsample route sweep: {n} queries')


def test_upsample_route_reports_three_kernels_per_direction():
    """the route query never names a kernel outside scalar / vec / row, whatever the width and the alignment of the pointers"""
    ops = _ops()
    assert ops.UPSAMPLE_KERNELS == ('scalar', 'vec', 'row')
    seen = {0: set(), 1: set()}
    for W in range(1, 261):
        for backward, in16, out16 in itertools.product((0, 1), (True, False), (True, False)):
            for NC, D, H in ((1, 2, 3), (2, 16, 43), (65536, 1, 1)):
                seen[backward].add(ops.upsample3d_route(backward, NC, D, H, W, _addr(in16), _addr(out16))['kernel'])
    assert seen == {0: {'scalar', 'vec', 'row'}, 1: {'scalar', 'vec', 'row'}}, seen


def test_maxpool_mirror_equals_route_and_respects_alignment():
    ops = _ops()
    seen = set()
    for (k, s, p), H, W, NC in itertools.product(((3, 2, 1), (2, 2, 0)), range(1, 13), list(range(1, 41)) + [256, 260, 512, 520], (1, 3)):
        if H + 2 * p < k or W + 2 * p < k:
            continue
        for backward, in16, idx4, out16 in itertools.product((0, 1), (True, False), (True, False), (True, False)):
            got = ops.maxpool2d_route(backward, NC, H, W, k, s, p, _addr(in16), 0x1000 if idx4 else 0x1001, _addr(out16))
            want = R.maxpool_plan(backward, NC, H, W, k, s, p, in16, idx4, out16)
            assert got == want, ((backward, NC, H, W, k, in16, idx4, out16), got, want)
            assert in16 or not got['load16']
            assert (in16 and out16 and idx4) or not got['v8']
            seen.add(R.maxpool_kind(got, backward))
    assert seen == {'3-load16', '3-scalar', '2-load16', '2-scalar', 'v8', '3-generic', '2-generic'}, seen


def test_softmax_mirror_equals_route():
    ops = _ops()
    for cols in range(1, R.SOFTMAX_MAX_COLS + 1):
        assert ops.softmax_dropout_route(cols) == R.softmax_plan(cols), cols
    assert ops.softmax_dropout_route(512)['maxv'] == 8 and ops.softmax_dropout_route(513)['maxv'] == 17
    for cols in (0, -1, R.SOFTMAX_MAX_COLS + 1):
        with pytest.raises(RuntimeError):
            ops.softmax_dropout_route(cols)


def test_route_queries_validate_arguments_without_a_device():
    import ctypes as C
    ops = _ops()
    L = ops.lib()
    with pytest.raises(RuntimeError):
        ops.upsample3d_route(0, 1, 0, 2, 4)
    with pytest.raises(RuntimeError):
        ops.maxpool2d_route(0, 1, 4, 4, 3, 1, 1)                   # 3 / 1 / 1 is not on the path
    with pytest.raises(RuntimeError):
        ops.maxpool2d_route(1, 1, 1, 1, 2, 2, 0)                   # window larger than the image
    assert L.muvo_upsample3d_route(0, C.c_int64(1), 1, 1, 4, None, None, None) == -1
    assert L.muvo_maxpool2d_route(0, C.c_int64(1), 4, 4, 3, 2, 1, None, None, None, None) == -1


# ================================================================================================ case lists
def test_every_kernel_is_named_and_every_case_takes_its_route():
    for backward, cases in ((0, R.UP_FWD_CASES), (1, R.UP_BWD_CASES)):
        for c in cases:
            plan = R.upsample_plan(backward, c['NC'], c['D'], c['H'], c['W'], c['in16'], c['out16'])
            assert plan['kernel'] == c['kernel'], (c['name'], plan)
        assert {(backward, c['kernel']) for c in cases} == {k for k in R.UPSAMPLE_NEEDS16 if k[0] == backward}
        assert len({c['name'] for c in cases}) == len(cases)
    by = {c['name']: R.upsample_plan(1, c['NC'], c['D'], c['H'], c['W']) for c in R.UP_BWD_CASES if c['in16'] and c['out16']}
    assert (by['row-2x17x6x32']['segs'], by['row-2x17x6x32']['dseg']) == (2, 9)             # 9 + 8
    assert (by['row-1x33x3x8']['segs'], by['row-1x33x3x8']['dseg']) == (4, 9)               # 9 + 9 + 9 + 6
    assert (by['row-1x16x2x16']['segs'], by['row-1x16x2x16']['dseg']) == (2, 8)             # 8 + 8
    assert (by['vec-2x9x43x12']['segs'], by['vec-2x9x43x12']['dseg']) == (1, 9)             # only the row kernel walks in segments
    assert by['vec-2x9x43x12']['grid'] == (1, 9, 2) and by['vec-1x1x43x12']['grid'] == (1, 1, 1)        # 129 lanes
    assert by['vec-1x2x341x12']['grid'] == (4, 2, 1) and by['vec-1x2x16x256']['grid'] == (4, 2, 1)      # 1023 / 1024 lanes
    assert by['vec-1x1x2x256']['grid'] == (1, 1, 1)
    assert all(p['block'] == (256, 1, 1) for p in by.values())
    assert by['row-1x2x5x128']['grid'] == (2, 1, 1)
    fw = {c['name']: R.upsample_plan(0, c['NC'], c['D'], c['H'], c['W']) for c in R.UP_FWD_CASES if c['in16'] and c['out16']}
    assert fw['row-1x3x5x128']['grid'] == (2, 4, 1) and fw['vec-2x2x3x256']['grid'] == (3, 4, 2)
    for backward, cases in ((0, R.MAXPOOL_FWD_CASES), (1, R.MAXPOOL_BWD_CASES)):
        for c in cases:
            plan = R.maxpool_plan(backward, c['NC'], c['H'], c['W'], c['k'], c['s'], c['p'], c['in16'], True, c['out16'])
            assert R.maxpool_kind(plan, backward) == c['kind'], (c['name'], plan)
    assert {c['kind'] for c in R.MAXPOOL_FWD_CASES} == {'3-load16', '3-scalar', '2-load16', '2-scalar'}
    assert {c['kind'] for c in R.MAXPOOL_BWD_CASES} == {'v8', '3-generic', '2-generic'}
    assert {R.softmax_plan(c)['maxv'] for _, c, _ in R.SOFTMAX_CASES} == {8, 17}
    # the failure message of the GPU test names an owner for every element of every case
    for backward, cases in ((0, R.UP_FWD_CASES), (1, R.UP_BWD_CASES)):
        for c in cases:
            plan = R.upsample_plan(backward, c['NC'], c['D'], c['H'], c['W'], c['in16'], c['out16'])
            m = 1 if backward else 2
            last = (c['NC'] - 1, m * c['D'] - 1, m * c['H'] - 1, m * c['W'] - 1)
            for idx in ((0, 0, 0, 0), last, tuple(v // 2 for v in last)):
                text = R.up_owner(c['kernel'], backward, c, idx, plan)
                assert c['kernel'] in text and ('border' in text or 'interior' in text), text
    c = next(c for c in R.UP_BWD_CASES if c['name'] == 'row-2x17x6x32')
    assert 'first plane of its segment' in R.up_owner('row', 1, c, (1, 9, 2, 5), R.upsample_plan(1, 2, 17, 6, 32))
    assert 'workgroup (1, 0, 0) lane 1' in R.up_owner('row', 1, {'NC': 1, 'D': 2, 'H': 5, 'W': 128}, (0, 1, 4, 2), R.upsample_plan(1, 1, 2, 5, 128))
    # a misaligned case never runs a kernel with 16-byte accesses of that pointer
    for backward, cases in ((0, R.UP_FWD_CASES), (1, R.UP_BWD_CASES)):
        for c in cases:
            need_in, need_out = R.UPSAMPLE_NEEDS16[(backward, c['kernel'])]
            assert (c['in16'] or not need_in) and (c['out16'] or not need_out), c['name']


# ================================================================================================ references
def test_float64_references_agree_with_pytorch():
    g = R._gen('refcheck')
    x = torch.randn(2, 3, 5, 6, generator=g, dtype=torch.float64)
    want = F.interpolate(x[None], scale_factor=2.0, mode='trilinear', align_corners=False)[0]
    assert torch.allclose(R.ref_up_fwd(x)[0], want, rtol=0, atol=1e-14)
    for (k, s, p), shape in itertools.product(((3, 2, 1), (2, 2, 0)), ((2, 7, 7), (1, 5, 18), (1, 4, 8), (1, 1, 1), (1, 5, 7))):
        if shape[1] + 2 * p < k:
            continue
        for fam in R.MAXPOOL_FAMILIES:
            c = {'NC': shape[0], 'H': shape[1], 'W': shape[2], 'k': k, 's': s, 'p': p}
            xm, dy = R.maxpool_inputs(c, fam)
            y, code = R.ref_maxpool(xm, k, s, p)
            xr = xm.clone().requires_grad_(True)
            yr = F.max_pool2d(xr[None], k, s, p)[0]
            assert torch.equal(y, yr), (k, shape, fam)
            if fam != 'constant' and fam != 'ties':       # (PyTorch's own tie rule is not part of its contract)
                yr.backward(dy)
                assert torch.equal(R.ref_maxpool_bwd(dy, code, shape[1], shape[2], k, s, p).float(), xr.grad), (k, shape, fam)
    xm = torch.full((1, 4, 4), 0.75)
    assert R.ref_maxpool(xm, 3, 2, 1)[1].flatten().tolist() == [4, 3, 1, 0]      # first live element of every window
    assert R.ref_maxpool(xm, 2, 2, 0)[1].flatten().tolist() == [0, 0, 0, 0]
    for (h, w), (oh, ow) in R.BILINEAR_CASES:
        xb = torch.randn(2, h, w, generator=g, dtype=torch.float64)
        want = F.interpolate(xb[None], size=(oh, ow), mode='bilinear', align_corners=False)[0]
        assert torch.allclose(R.ref_bilinear(xb, oh, ow)[0], want, rtol=0, atol=1e-13)
    # GRU / sample backward against autograd of the float64 forward
    gi, gh, h, dhn = (t.double().requires_grad_(True) for t in R.gru_inputs(3, 4, 'randn'))
    e = R.gru_eval(gi, gh, h, dhn, torch.float64)
    e['hn'].backward(dhn.detach())
    for got, want in ((e['dgi'], gi.grad), (e['dgh'], gh.grad), (e['dh'], h.grad)):
        assert torch.allclose(got.detach(), want, rtol=0, atol=1e-14)
    cell = torch.nn.GRUCell(4, 4).double()
    xin = torch.randn(3, 4, dtype=torch.float64, generator=g)
    hh = h.detach()
    gi2, gh2 = xin @ cell.weight_ih.T + cell.bias_ih, hh @ cell.weight_hh.T + cell.bias_hh
    assert torch.allclose(R.gru_eval(gi2, gh2, hh, hh, torch.float64)['hn'], cell(xin, hh), rtol=0, atol=1e-14)
    mls, eps_store, (dmu, dsigma, dsample) = R.sample_inputs(3, 4, 'randn')
    m = mls.double().requires_grad_(True)
    ev = R.sample_eval(m, eps_store[:, :4], dmu, dsigma, dsample, 0.1, torch.float64)
    (ev['mu'] * dmu).sum().add((ev['sigma'] * dsigma).sum()).add((ev['sample'] * dsample).sum()).backward()
    assert torch.allclose(ev['dmls'].detach(), m.grad, rtol=0, atol=1e-14)
    assert torch.allclose(ev['sigma'], 2 * torch.sigmoid(m[:, 4:] / 2) + float(R.f32(0.1)), rtol=0, atol=1e-15)
    # softmax backward against autograd
    S, dPd = R.softmax_inputs(5, 65, 0.5)
    mask = R.host_dropout_mask(5, 65, 0.5, R.SOFTMAX_SEED)
    assert 0.3 < float((mask == 0).float().mean()) < 0.7 and set(mask.unique().tolist()) == {0.0, 2.0}
    Sd = S.double().requires_grad_(True)
    (torch.softmax(Sd, 1) * mask.double() * dPd.double()).sum().backward()
    assert torch.allclose(R.ref_softmax(S, dPd, mask)['dS'][0], Sd.grad, rtol=0, atol=1e-14)
    for in_sz, out_sz in R.NEAREST_CASES:                       # the kernel's float32 index rule equals PyTorch's legacy 'nearest'
        for n_in, n_out in zip(in_sz, out_sz):
            sc = R.f32(float(n_in)) / R.f32(float(n_out))
            mine = torch.floor(torch.arange(n_out, dtype=torch.float32) * sc).long().clamp_max(n_in - 1)
            want = R.ref_nearest(torch.arange(n_in, dtype=torch.float32)[None], (n_out,))[0].long()
            assert torch.equal(mine, want), (n_in, n_out)


def test_upsample_adjoint_identity():
    for c in R.UP_FWD_CASES[:14]:
        if c['NC'] > 4:
            continue
        x, g = R.up_inputs(c, 0).double(), R.up_inputs(c, 1).double()
        lhs, rhs = float((R.ref_up_fwd(x)[0] * g).sum()), float((x * R.ref_up_bwd(g)[0]).sum())
        scale = float((R.ref_up_fwd(x)[0] * g).abs().sum())
        assert abs(lhs - rhs) <= 1e-12 * scale, (c['name'], lhs, rhs)
    for (h, w), (oh, ow) in R.BILINEAR_CASES:
        x, g = (t.double() for t in R.bilinear_inputs(h, w, oh, ow))
        lhs, rhs = float((R.ref_bilinear(x, oh, ow)[0] * g).sum()), float((x * R.ref_bilinear_bwd(g, h, w)[0]).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((R.ref_bilinear(x, oh, ow)[0] * g).abs().sum()), ((h, w), (oh, ow))


# ================================================================================================ bars
def test_bar_tables_are_not_stale_and_emulations_stay_within():
    own, trans = R.compute_own_worst(), R.compute_trans_worst()
    assert set(own) == set(R.OWN_WORST) and set(trans) == set(R.TRANS_WORST)
    for k, (rms, e) in sorted(own.items()):
        t = R.OWN_WORST[k]
        print(f'ELEMSTAT worst emulated {k}: rms {rms:.3e} max e {e:.3e} (tabulated {t[0]:.3e} {t[1]:.3e})')
        assert rms <= t[0] <= 1.02 * rms and e <= t[1] <= 1.02 * e, (k, rms, e, t)
        assert R.within({'rms': rms, 'max_e': e}, R.kernel_bar(k))
    for k, (rms, e) in sorted(trans.items()):
        t = R.TRANS_WORST[k]
        print(f'ELEMSTAT worst float32 evaluation {k}: rms {rms:.3e} max e {e:.3e} (tabulated {t[0]:.3e} {t[1]:.3e})')
        # the host's expf / tanhf differ between C libraries and vector widths: a factor of 2 either way, against a bar of 4 x
        assert rms <= 2 * t[0] and t[0] <= 2 * rms and e <= 2 * t[1] and t[1] <= 2 * e, (k, rms, e, t)
    # no bar is so loose that a float32 kernel could lose a term.  The smallest term of an output or gradient element carries
    # the weight 0.25^3 among at most 64 terms of weight <= 1, so losing it moves e by about 0.25^3 / sqrt(64) = 2e-3 = 3e4 u; the
    # bars stay three orders of magnitude below that.  The largest is the float4 gather's: its 16 serial additions per element
    # reach 10.4 u once among the 74304 elements of its largest case, so its bar is 20.8 u (the other kernels' stay below 16 u).
    for k in R.OWN_WORST:
        if k.startswith('up_'):
            assert R.kernel_bar(k)[1] < (32 if k == 'up_bwd_vec' else 16) * R.U32, k


def test_exact_emulations_are_exact():
    """the bit-for-bit references are float32 evaluations in the kernel's order: they sit within one rounding of float64"""
    x = torch.randn(7, 300, generator=R._gen('batchsum'))
    assert torch.allclose(R.ref_batchsum(x, None, False).double(), x.double().sum(0), rtol=0, atol=7 * 2 * R.U32 * float(x.abs().max()))
    a, b = torch.randn(300, generator=R._gen('axpby')), torch.randn(300, generator=R._gen('axpby', 2))
    assert torch.allclose(R.ref_axpby(a, b, 0.3, -1.7).double(), float(R.f32(0.3)) * a.double() + float(R.f32(-1.7)) * b.double(), rtol=0, atol=1e-6)
    assert torch.equal(R.ref_axpby(a, None, 2.0, 5.0), 2 * a)
    dy = torch.randn(5, generator=R._gen('avgb'))
    assert torch.allclose(R.emu_avgpool_bwd(dy, 63).double(), (dy.double() / 63).view(-1, 1).expand(-1, 63), rtol=2 * R.U32, atol=0)
    src, dst = torch.arange(40.0), torch.full((50,), -1.0)
    out = R.ref_copy2d(src, dst, 3, 4, 10, 7, True)
    assert out[:4].tolist() == [-1 + v for v in (0, 1, 2, 3)] and out[7:11].tolist() == [9.0, 10.0, 11.0, 12.0] and out[4:7].tolist() == [-1.0] * 3
    N, C_, L, l0 = 3, 5, 4, 2
    xx, pos, te = torch.randn(N, C_, L), torch.randn(C_, L), torch.randn(C_)
    tok = R.ref_tokens(xx, pos, te, torch.zeros(l0 + L + 1, N, C_), l0)
    assert float(tok[:l0].abs().sum()) == 0 and float(tok[l0 + L:].abs().sum()) == 0
    assert torch.equal(tok[l0 + 1, 2, 3], (xx[2, 3, 1] + pos[3, 1]) + te[3])
    assert torch.equal(R.ref_untoken(tok, N, C_, L, l0), (xx + pos) + te.view(1, -1, 1))


# ================================================================================================ planted faults
def _clear(label, st, bar):
    ex = R.excess(st, bar)
    print(f'ELEMSTAT planted fault {label}: max e {st["max_e"]:.3e} rms {st["rms"]:.3e} = {ex:.0f} x the bar')
    assert ex >= FAULT_FACTOR, (label, st, bar)


def _case(cases, name):
    return next(c for c in cases if c['name'] == name)


def test_planted_upsample_faults_fail():
    for name in ('row-2x17x6x32', 'vec-2x9x43x12', 'vec-1x2x3x12', 'scalar-2x2x3x5', 'row-1x33x3x8', 'vec-1x8x22x24', 'row-1x16x2x16'):
        c = _case(R.UP_BWD_CASES, name)
        g = R.up_inputs(c, 1)
        ref, bar = R.ref_up_bwd(g), R.kernel_bar(f'up_bwd_{c["kernel"]}')
        assert R.within(R.error_stats(R.emu_up_bwd(c['kernel'], g), *ref), bar)
        for fault in ('last_col', 'last_row', 'last_plane'):
            _clear(f'{name} {fault}', R.error_stats(R.emu_up_bwd(c['kernel'], g, fault=fault), *ref), bar)
        if c['kernel'] == 'row':
            plan = R.upsample_plan(1, c['NC'], c['D'], c['H'], c['W'])
            assert plan['segs'] > 1
            _clear(f'{name} no_lead_in', R.error_stats(R.emu_up_bwd(c['kernel'], g, dseg=plan['dseg'], fault='no_lead_in'), *ref), bar)
        if c['kernel'] == 'row':
            _clear(f'{name} same_lane', R.error_stats(R.emu_up_bwd('row', g, fault='same_lane'), *ref), bar)
    for name in ('row-3x2x3x8', 'row-1x3x5x128', 'row-2x2x7x32'):
        c = _case(R.UP_FWD_CASES, name)
        x = R.up_inputs(c, 0)
        _clear(f'fwd {name} same_lane', R.error_stats(R.emu_up_fwd(c['kernel'], x, fault='same_lane'), *R.ref_up_fwd(x)),
               R.kernel_bar(f'up_fwd_{c["kernel"]}'))
    # the forward clamps: 0.75 of the last column alone (its 0.25 neighbour dropped) instead of weight 1
    c = _case(R.UP_FWD_CASES, 'vec-2x1x4x12')
    x = R.up_inputs(c, 0)
    bad = R.emu_up_fwd('vec', x)
    bad[..., -1] = bad[..., -1] * R.f32(0.75)
    _clear('fwd vec last column weight 0.75', R.error_stats(bad, *R.ref_up_fwd(x)), R.kernel_bar('up_fwd_vec'))


def test_planted_maxpool_faults_fail():
    n_fifth = 0
    for c in R.MAXPOOL_BWD_CASES:
        if c['kind'] != 'v8' or c['W'] < 16:
            continue
        x, dy = R.maxpool_inputs(c, 'random')
        _, code = R.ref_maxpool(x, 3, 2, 1)
        good = R.ref_maxpool_bwd(dy, code, c['H'], c['W'], 3, 2, 1)
        bad = R.ref_maxpool_bwd(dy, code, c['H'], c['W'], 3, 2, 1, drop_fifth=True)
        diff = int((good != bad).sum())
        print(f'ELEMSTAT planted fault maxpool {c["name"]} fifth window dropped: {diff} elements differ')
        assert diff > 0 and bool(((good != bad).nonzero()[:, 2] % 8 == 7).all())
        n_fifth += 1
    assert n_fifth >= 2
    for c in R.MAXPOOL_FWD_CASES:
        if c['H'] * c['W'] == 1 or not c['in16']:
            continue
        x, _ = R.maxpool_inputs(c, 'ties')
        first, last = R.ref_maxpool(x, c['k'], c['s'], c['p']), R.ref_maxpool(x, c['k'], c['s'], c['p'], last_wins=True)
        assert torch.equal(first[0], last[0])
        d = int((first[1] != last[1]).sum())
        print(f'ELEMSTAT planted fault maxpool {c["name"]} last maximum wins: {d} winner bytes differ')
        assert d > 0, c['name']
        xc, _ = R.maxpool_inputs(c, 'constant')
        assert not torch.equal(R.ref_maxpool(xc, c['k'], c['s'], c['p'])[1], R.ref_maxpool(xc, c['k'], c['s'], c['p'], last_wins=True)[1])
        if c['p']:
            xn, _ = R.maxpool_inputs(c, 'negative')
            good, bad = R.ref_maxpool(xn, c['k'], c['s'], c['p']), R.ref_maxpool(xn, c['k'], c['s'], c['p'], pad_value=0.0)
            d = int((good[0] != bad[0]).sum())
            print(f'ELEMSTAT planted fault maxpool {c["name"]} padding 0: {d} maxima differ')
            assert d > 0 and bool((bad[0][good[0] != bad[0]] == 0).all())


def test_planted_softmax_and_gru_faults_fail():
    rows, cols, p = 5, 65, 0.5
    S, dPd = R.softmax_inputs(rows, cols, p)
    mask = R.host_dropout_mask(rows, cols, p, R.SOFTMAX_SEED)
    ref = R.ref_softmax(S, dPd, mask)
    for k in ('P', 'Pd', 'dS'):
        assert R.within(R.norm_stats(R.emu_softmax(S, dPd, mask)[k], *ref[k]), R.kernel_bar(f'softmax_{k}'))
    bad = R.emu_softmax(S, dPd, mask, no_max=True)
    assert bool(torch.isfinite(bad['P'][-1]).all()) and not bool(torch.isfinite(bad['P'][-2]).all())     # e^80 is finite, e^100 is not
    st = R.norm_stats(bad['P'], *ref['P'])
    print(f'ELEMSTAT planted fault softmax without the max subtraction: max e {st["max_e"]} rms {st["rms"]}')
    assert not R.within(st, R.kernel_bar('softmax_P'))
    wrong = R.host_dropout_mask(rows, cols, p, R.SOFTMAX_SEED, index_cols=cols - 1)      # the mask of a 64-column matrix
    assert torch.equal(wrong[0, :cols - 1], mask[0, :cols - 1]) and not torch.equal(wrong[1:], mask[1:])
    bad = R.emu_softmax(S, dPd, wrong)
    for k in ('Pd', 'dS'):
        _clear(f'softmax {k} mask of another row length', R.norm_stats(bad[k], *ref[k]), R.kernel_bar(f'softmax_{k}'))
    for B, H, fam in R.GRU_CASES:
        if fam == 'saturated':          # tanh at +-1: dpre_n itself is 0 there
            continue
        args = R.gru_inputs(B, H, fam)
        e64, den = R.gru_eval(*args, torch.float64), R.gru_dens(*args)
        bad = R.gru_eval(*args, torch.float32, drop_r=True)
        st = R.norm_stats(bad['dgh'], e64['dgh'], den['dgh'])
        _clear(f'gru {B}x{H} {fam} dgh without r', st, R.kernel_bar('gru_bwd'))
