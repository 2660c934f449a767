"""CPU: the float64 references, the emulations, the bars, the planted faults and the dispatch mirror of tests/gemm_reference.py,
which tests/test_gemm_kernels_gpu.py applies to the dense GEMM unit (muvo_amd/csrc/gemm.hip).  Shown here, without a device:
  * every emulation passes its bar at every case of the GPU file, the VALU emulations that share f32_bar within half of it, and
    the two kernels with a bar of their own have exactly the bar their emulation gives (margin 2);
  * every planted fault is rejected at every case it applies to, by the very comparison (judge) the GPU test uses;
  * bf16x3 arithmetic fails the bar at least 4x at every arithmetic-identifying case;
  * gemm_plan / grouped_plan equal the library's routing queries on every case and on a sweep around each threshold, in both
    deterministic modes; every case is routed to the kernel it is listed for;
  * the references agree with torch in float64; the attention bars are the float32 evaluation's."""
import collections
import contextlib
import ctypes
import itertools
import math

import pytest
import torch

import gemm_reference as R

IDS = [c['name'] for c in R.GEMM_CASES]


@contextlib.contextmanager
def deterministic(on):
    from muvo_amd import ops
    L = ops.lib()
    was = L.muvo_get_deterministic()
    try:
        assert L.muvo_set_deterministic(1 if on else 0) == 0
        yield
    finally:
        L.muvo_set_deterministic(was)


@pytest.fixture(scope='module')
def emulated():
    """{case name: (data, judge of the emulation)}: computed once, read-only"""
    out = {}
    for c in R.GEMM_CASES:
        d = R.make(c)
        out[c['name']] = (d, R.judge(c, d, R.emulate(c, d)))
    return out


# ================================================================================================ references
def test_ref_gemm_reads_storage_like_torch():
    """strides, batch strides, offsets, bias_div, alpha and the activation against plain torch on materialised operands"""
    for name in ('t32-16x40x12-batched', 't128-offsets', 't128-biasdiv65', 't32-lay-ss', 't128-act-sigmoid', 'kc-sam-24x67x64'):
        c = next(c for c in R.GEMM_CASES if c['name'] == name)
        d = R.make(c)
        ref, den = R.ref_gemm(c, d)
        s = R.strides(c)
        for b1 in range(c['B1']):
            for b2 in range(c['B2']):
                a = torch.empty(c['M'], c['K'], dtype=torch.float64)
                b = torch.empty(c['K'], c['N'], dtype=torch.float64)
                a0 = c['a_off'] + b1 * s['a_b'][0] + b2 * s['a_b'][1]
                b0 = c['b_off'] + b1 * s['b_b'][0] + b2 * s['b_b'][1]
                for k in range(c['K']):
                    a[:, k] = d.A[a0 + k * s['sak']: a0 + k * s['sak'] + (c['M'] - 1) * s['sam'] + 1: s['sam']].double()
                    b[k] = d.B[b0 + k * s['sbk']: b0 + k * s['sbk'] + (c['N'] - 1) * s['sbn'] + 1: s['sbn']].double()
                y = c['alpha'] * (a @ b)
                if c['bias']:
                    y = y + d.bias.double()[torch.arange(c['N']) // c['bias_div']]
                y = {R.ACT_NONE: y, R.ACT_RELU: torch.relu(y), R.ACT_SIGMOID: torch.sigmoid(y), R.ACT_ELU: torch.nn.functional.elu(y)}[c["act"]]
                assert torch.allclose(ref[b1, b2], y, rtol=1e-13, atol=1e-13), name
    assert ref.shape == den.shape and bool((den > 0).all())


def test_ref_mode1_adds_to_prior():
    c = next(c for c in R.GEMM_CASES if c['name'] == 't32-acc-batched')
    d = R.make(c)
    ref, den = R.ref_gemm(c, d)
    A, B = R.operands(c, d)
    prior = R.c_view(c, d.C0)[:, :, :c['M']].double()
    assert bool((prior != 0).all()) and torch.allclose(ref, prior + A @ B, rtol=1e-13, atol=1e-13)
    assert torch.allclose(den, ((A * A) @ (B * B) + prior ** 2).sqrt())


def test_sigmoid_cases_keep_their_scale():
    for c in R.GEMM_CASES:
        if c['act'] == R.ACT_SIGMOID:
            assert c['K'] >= 16 and float(R.ref_gemm(c, R.make(c))[1].min()) >= 0.2, c['name']


def test_case_list_covers_the_issue():
    by = collections.defaultdict(list)
    for c in R.GEMM_CASES:
        by[R.case_plan(c)['kernel']].append(c)
    kv, kc, nc, t = by[R.KV], by[R.KC], by[R.NC], by[R.T]
    assert {c['M'] for c in kv} == {1, 4, 5, 8, 9, 16, 17, 24} and {c['N'] for c in kv} == {2, 66, 67}
    assert {c['K'] for c in kv} == {64, 68, 2048, 2052, 4096, 4104}
    assert {(c['M'], c['K']) for c in kv} == set(itertools.product((1, 4, 5, 8, 9, 16, 17, 24), (64, 68, 2048, 2052, 4096, 4104)))
    assert {(c['N'], c['K']) for c in kv} == set(itertools.product((2, 66, 67), (64, 68, 2048, 2052, 4096, 4104)))
    for rm in (4, 8, 16, 24):
        sub = [c for c in kv if R.case_plan(c)['rm'] == rm]
        assert {c['act'] for c in sub} == set(R.ALL_ACTS), rm
        assert {c['bias_div'] for c in sub if c['bias']} == {1, 3} and any(c['scm_pad'] for c in sub) and any(not c['bias'] for c in sub)
    assert {c['M'] for c in kc} >= {3, 4, 5, 25, 32} and {R.case_plan(c)['rm'] for c in kc} == {4, 8}
    assert any(c['K'] == 70 for c in kc) and any(c['a_off'] == 1 for c in kc) and any(c['sam_pad'] == 1 for c in kc)
    assert any(c['N'] == 65 for c in kc) and any(c['K'] == 17 for c in kc)
    assert {c['M'] for c in nc} == {3, 4, 5, 8, 9, 24, 25, 32} and {c['N'] for c in nc} >= {64, 100}
    assert {R.case_plan(c)['rm'] for c in nc} == {4, 8, 24}
    assert any((c['M'], c['N'], c['K'], c['bias_div']) == (4, 1300, 48, 65) for c in nc)
    assert {R.case_plan(c)['tile'] for c in t} == {(32, 128), (128, 64), (128, 128)}
    for tile in ((32, 128), (128, 128)):
        assert {R.case_plan(c)['lay'] for c in t if R.case_plan(c)['tile'] == tile} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c['K'] for c in t} >= {0, 1, 15, 17, 129}
    assert {c['act'] for c in t if c['alpha'] == 0.37 and c['bias']} == set(R.ALL_ACTS)
    assert any(c['mode'] == 1 and c['B1'] * c['B2'] > 1 for c in t) and any(c['mode'] == 1 and c['det'] for c in t)
    assert len(R.GROUPED_CASES) >= 9 and {c['M'] for c in R.GROUPED_CASES} == {1, 8, 9, 24}
    assert {c['K'] for c in R.GROUPED_CASES} == {64, 68, 260, 2052, 4100}
    assert {len(c['ns']) for c in R.GROUPED_CASES} >= {1, 5, 16}


# ================================================================================================ emulations and bars
@pytest.mark.parametrize('c', R.GEMM_CASES, ids=IDS)
def test_emulation_passes_its_bar(c, emulated):
    d, j = emulated[c['name']]
    kernel = R.case_plan(c)['kernel']
    print(R.statline(c, j, 'emulated ' + kernel))
    assert j['canary_ok'] and R.within(j['stats'], j['bar']), (j['stats'], j['bar'], j['where'])
    # the margin: every bar is (at least) 2 x the emulation of the kernel it is applied to.  (The MFMA chain of the tiled
    # kernel IS the emulation f32_bar was derived from, with margin 2 on the conv layers; a single product, K = 1, rounds at
    # rms 0.43 u where that fit allows 0.46 u, so the tiled kernel is held to the bar itself, not to half.)
    if kernel != R.T:
        assert j['share'] <= 0.5 * 1.005, (c['name'], j['share'])
    if kernel in (R.KV, R.NC):                               # on f32_bar itself
        assert j['bar'] == R.f32_bar(c['K'])


def test_own_bars_are_twice_their_own_emulation():
    worst = R.own_worst()
    for k, (rms, e) in sorted(worst.items()):
        print(f'GEMMSTAT worst emulated {k}: rms {rms:.3f} max e {e:.3f} u sqrt(K)')
    for k, (rms, e) in R.OWN_WORST.items():
        assert worst[k][0] <= rms <= 1.02 * worst[k][0] and worst[k][1] <= e <= 1.02 * worst[k][1], (k, worst[k])
        assert worst[k][0] > 0.5 * 0.46, k                   # listed because it does not stay within half of f32_bar
    for k in set(worst) - set(R.OWN_WORST) - {R.T}:          # the VALU kernels that keep f32_bar do stay within half of it
        assert worst[k][0] <= 0.5 * 0.46 and worst[k][1] <= 0.5 * 4.8, (k, worst[k])
    assert set(worst) == {R.T, R.KV, R.KC, R.NC, 'grouped_fwd', 'grouped_dx', 'grouped_dw', 'grouped_db', 'colsum'}


@pytest.mark.parametrize('c', R.GEMM_CASES, ids=IDS)
def test_planted_faults_fail(c, emulated):
    d = emulated[c['name']][0]
    ref = R.ref_gemm(c, d)
    applied = []
    for fault in R.FAULTS:
        if not R.fault_applies(c, fault) or fault == 'bf16x3':
            continue
        j = R.judge(c, d, R.emulate(c, d, fault), ref)
        applied.append(fault)
        assert not R.passes(j), (fault, j['stats'], j['bar'])
        if fault == 'row_clamp':
            assert not j['canary_ok'] and j['n_canary_bad'] == c['B1'] * c['B2'] * c['N']
        else:
            assert j['canary_ok'] and j['share'] > 4, (fault, j['share'])
    assert 'row_clamp' in applied and (c['K'] == 0 or 'ktile_dropped' in applied)


def test_every_fault_is_planted_somewhere():
    for fault in R.FAULTS:
        assert sum(R.fault_applies(c, fault) for c in R.GEMM_CASES) >= 5, fault
    kernels = {f: {R.case_plan(c)['kernel'] for c in R.GEMM_CASES if R.fault_applies(c, f)} for f in R.FAULTS}
    assert kernels['half_dropped'] == {R.KV, R.KC} and kernels['bias_n'] >= {R.T, R.KV, R.KC, R.NC}
    assert kernels['bias_alpha'] >= {R.T, R.KV, R.KC, R.NC}


IDENT = [c for c in R.GEMM_CASES if c['ident']]


@pytest.mark.parametrize('c', IDENT, ids=[c['name'] for c in IDENT])
def test_bf16x3_arithmetic_fails_4x(c, emulated):
    assert 1 <= c['K'] <= 1350
    d = emulated[c['name']][0]
    j = R.judge(c, d, R.emulate(c, d, 'bf16x3'))
    print(R.statline(c, j, 'bf16x3'))
    assert j['canary_ok'] and j['share'] >= 4, j['share']


def test_ident_cases_cover_every_kernel():
    assert {R.case_plan(c)['kernel'] for c in IDENT} == {R.T, R.KV, R.KC, R.NC}
    assert {R.case_plan(c)['tile'] for c in IDENT if R.case_plan(c)['kernel'] == R.T} == {(32, 128), (128, 64), (128, 128)}


# ================================================================================================ grouped Linear, column sums
@pytest.mark.parametrize('c', R.GROUPED_CASES, ids=[c['name'] for c in R.GROUPED_CASES])
def test_grouped_emulations_and_faults(c):
    inp = R.grouped_inputs(c)
    half = lambda bar: (0.5 * bar[0] * 1.005, 0.5 * bar[1] * 1.005)         # noqa: E731
    refs = {}
    for kind, label, K, got, ref in R.grouped_emulated(c, inp):
        st = R.error_stats(got, *ref)
        assert R.within(st, half(R.kernel_bar(kind, K))), (label, st)
        refs[label] = (ref, R.kernel_bar(kind, K))
    used = [l for l in range(len(c['ns'])) if l not in c['unused']]

    def fails(label, got, factor=4):
        ref, bar = refs[label]
        return R.excess(R.error_stats(got, *ref), bar) > factor
    for l, n in enumerate(c['ns']):
        if c['K'] > 2048:                                    # the k + 2048 half lost
            x = inp.x.clone()
            x[:, 2048:4096] = 0
            assert fails(f'y{l}', R.emu_grouped_fwd(x, inp.ws[l], inp.bs[l]))
        if inp.bs[l] is not None and n > 1:                  # the neighbouring column's bias
            assert fails(f'y{l}', R.emu_grouped_fwd(inp.x, inp.ws[l], inp.bs[l].roll(1)))
    if len(used) > 1:                                        # one layer's contribution lost
        assert fails('dx', R.emu_grouped_dx([inp.dys[l] for l in used[1:]], [inp.ws[l] for l in used[1:]]))
    for l in used:
        if c['M'] > 1:                                       # the last row lost
            assert fails(f'dW{l}', R.emu_grouped_dw(inp.dys[l][:-1], inp.x[:-1], inp.gw[l]))
            assert fails(f'db{l}', R.emu_grouped_db(inp.dys[l][:-1], inp.gb[l]))
    for l, db in R.grouped_fault_frozen_bias(c, inp).items():    # the bias gradient of a frozen-weight layer left out
        assert fails(f'db{l}', db)


def test_frozen_weight_fault_is_planted():
    assert sum(bool(R.grouped_fault_frozen_bias(c, R.grouped_inputs(c))) for c in R.GROUPED_CASES) >= 2


@pytest.mark.parametrize('rows,cols,pad', R.COLSUM_CASES)
def test_colsum_emulation(rows, cols, pad):
    x, prior = R.colsum_inputs(rows, cols, pad)
    ref = R.ref_colsum(x, prior)
    bar = R.kernel_bar('colsum', rows)
    for det in (False, True):
        st = R.error_stats(R.emu_colsum(x, prior, det), *ref)
        assert R.within(st, (0.5 * bar[0] * 1.005, 0.5 * bar[1] * 1.005)), (det, st)
    if rows > 1:
        assert R.excess(R.error_stats(R.emu_colsum(x[:-1], prior), *ref), bar) > 4      # the last row lost
    assert not R.within(R.error_stats(prior, *ref), bar)     # nothing added


@pytest.mark.parametrize('act', R.ALL_ACTS)
def test_act_bwd_emulation(act):
    g = R._gen('act_bwd', act)
    y = R.act32(torch.randn(4099, generator=g), act)
    dy = torch.randn(4099, generator=g)
    ref = R.ref_act_bwd(y, dy, act)
    st = R.error_stats(dy * R.act_grad_from_out(y, act), *ref)
    print(f'GEMMSTAT emulated act_bwd {R.ACT_NAMES[act]}: max e {st["max_e"]:.3e} rms {st["rms"]:.3e}')
    assert R.within(st, (0.5 * R.ACT_BWD_BAR[0], 0.5 * R.ACT_BWD_BAR[1])), st
    wrong = dy * R.act_grad_from_out(y, (act + 1) % 6)       # the neighbouring activation's derivative
    assert not R.within(R.error_stats(wrong, *ref), R.ACT_BWD_BAR)


# ================================================================================================ dispatch mirror
def _route(c, det):
    from muvo_amd import ops
    s = R.strides(c)
    with deterministic(det):
        return ops.gemm_route(c['M'], c['N'], c['K'], s['sam'], s['sak'], s['sbk'], s['sbn'], s['scm'], c['bias'], c['act'],
                              c['mode'], c['B1'], c['B2'], 4096 + 4 * c['a_off'], 8192 + 4 * c['b_off'])


@pytest.mark.parametrize('c', R.GEMM_CASES, ids=IDS)
def test_plan_equals_route_on_cases(c):
    for det in (False, True):
        assert R.case_plan(c, det) == _route(c, det), det
    plan = R.case_plan(c)
    for k, v in c['expect'].items():
        assert plan[k] == v, (c['name'], k, plan[k], v)


def test_plan_equals_route_on_sweep():
    from muvo_amd import ops
    ms = (1, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 130)
    ns = (1, 63, 64, 65, 200)
    ks = (0, 15, 16, 63, 64, 66, 68, 640, 1000)
    # (sam, sak, sbk, sbn) builders and operand alignment: k-contiguous pair with each alignment condition broken in turn,
    # then the other layouts
    lays = [
        ('kk', lambda M, N, K: (K, 1, 1, K), 0, 0),
        ('kk-a-unaligned', lambda M, N, K: (K, 1, 1, K), 4, 0),
        ('kk-b-unaligned', lambda M, N, K: (K, 1, 1, K), 0, 8),
        ('kk-sam', lambda M, N, K: (K + 1, 1, 1, K), 0, 0),
        ('kk-sbn', lambda M, N, K: (K, 1, 1, K + 2), 0, 0),
        ('kn', lambda M, N, K: (K, 1, N, 1), 0, 0),
        ('mk', lambda M, N, K: (1, M, 1, K), 0, 0),
        ('mn', lambda M, N, K: (1, M, N, 1), 0, 0),
        ('ss', lambda M, N, K: (2 * K + 1, 2, 2, 2 * K + 1), 0, 0),
    ]
    count, kernels = 0, collections.Counter()
    for det in (False, True):
        with deterministic(det):
            for (name, lay, ao, bo), M, N, K in itertools.product(lays, ms, ns, ks):
                sam, sak, sbk, sbn = lay(M, N, K)
                for mode, nb, bias, scm in ((0, 1, False, N), (0, 1, True, N), (0, 1, False, N + 1), (0, 2, False, N), (1, 1, False, N),
                                            (1, 6, False, N), (0, 1, False, N)):
                    act = R.ACT_RELU if (mode, nb, bias, scm) == (0, 1, False, N) and count % 2 else R.ACT_NONE
                    want = R.gemm_plan(M, N, K, sam, sak, sbk, sbn, scm, bias, act, mode, nb, ao % 16 == 0, bo % 16 == 0, det)
                    got = ops.gemm_route(M, N, K, sam, sak, sbk, sbn, scm, bias, act, mode, 1 if nb == 1 else 2, 1 if nb == 1 else nb // 2,
                                         4096 + ao, 8192 + bo)
                    assert want == got, (name, M, N, K, mode, nb, bias, scm, act, det, want, got)
                    count += 1
                    kernels[want['kernel'], want['rm'], want['tile']] += 1
    assert len(kernels) == 4 + 2 + 3 + 3, kernels            # every kernel and template was reached
    # the query validates like the launch and touches no device
    L = ops.lib()
    d = ops.GemmDesc(4, 4, 4, 4, 1, 1, 4, 4, 1, 1, 0, 0, 0, 0, 0, 0, 1.0, 1, 0, 0.0, 1)
    r = ops.GemmRouteInfo()
    assert L.muvo_gemm_route(ctypes.byref(d), None, None, 1, ctypes.byref(r)) == -1 and b'accumulate' in L.muvo_last_error()
    assert L.muvo_gemm_route(ctypes.byref(d), None, None, 0, None) == -1 and b'null' in L.muvo_last_error()
    assert L.muvo_gemm_route(ctypes.byref(d), None, None, 0, ctypes.byref(r)) == 0 and r.kernel == 0 and r.ksplit == 1


def test_grouped_plan_equals_route():
    from muvo_amd import ops
    for c in R.GROUPED_CASES:
        assert R.grouped_plan(c['M'], c['K'], c['ns']) == ops.grouped_linear_route(c['M'], c['K'], c['ns']), c['name']
    for M, K, ns in itertools.product((1, 8, 9, 24), (64, 252, 256, 260, 4100), ([1], [3, 4, 5], [15, 16, 17, 127, 128, 129], [7] * 16)):
        assert R.grouped_plan(M, K, ns) == ops.grouped_linear_route(M, K, ns)
    assert {R.grouped_plan(c['M'], c['K'], c['ns'])['fwd_rm'] for c in R.GROUPED_CASES} == {8, 24}
    for M, K, ns in ((25, 64, [4]), (8, 66, [4]), (8, 60, [4]), (8, 64, [0]), (8, 64, [1] * 17)):
        with pytest.raises(RuntimeError):
            ops.grouped_linear_route(M, K, ns)


# ================================================================================================ attention bar
@pytest.mark.parametrize('case', R.ATTN_CASES)
def test_attention_bar_is_the_float32_evaluation(case):
    qkv, dout = R.attention_inputs(case)
    e = R.attention_errors(case, R.attention_float32(qkv, case[2], dout))
    for n, v in e.items():
        m = R.ATTN_MEASURED[case][n]
        print(f'GEMMSTAT float32 attention {case} {n}: {v:.3e} (tabulated {m:.2e})')
        assert v <= 4 * m and m <= 4 * v, (n, v, m)           # another thread count's summation order (attention_reference)
    # the bar bites: one probability-weighted value row lost
    ref = R.attention_reference64(case)
    bad = {k: v.float().clone() for k, v in ref.items() if k in ('o', 'dqkv')}
    bad['o'][0, 0, 0] += 1e-5 * float(ref['o'].abs().max())
    assert R.attention_errors(case, bad)['o'] > R.ATTN_BARS[case]['o']
