"""CPU: tests/rssm_reference.py itself.  The float64 evaluator agrees with torch.autograd on oracle.muvo_ref.RSSM, the bars pass
the emulated arithmetic of the two persistent kernels and reject every planted fault, the bar tables are current, the inputs do
not saturate, every edge of the case table is hit by a named case, and the mirrors of the host-side size functions match their
formulas.  Nothing here needs a GPU; tests/test_rssm_kernels_gpu.py applies the same bars to the kernels."""
import math

import pytest
import torch

import rssm_reference as R

F64 = torch.float64


# ================================================================================================ float64 reference
@pytest.mark.parametrize('name,mask', [('tiny-b3-t5', 'alt'), ('tiny-b3-t5', 'bit0'), ('tiny-b1-t64', 'hi'), ('sub256-b5-t2', 'bit0'),
                                       ('tiny-b64-t1', 'none')])
def test_reference_agrees_with_autograd(name, mask):
    """all 7 outputs, d_emb and the 18 parameter gradients (dY^T X and column sums of the hand-written backward's kept gradients)
    against torch.autograd on the oracle's module in float64"""
    from oracle import muvo_ref
    c, inp = R.CASE[name], R.inputs(name)
    H, S, E, A = c['dims']
    m = muvo_ref.RSSM(E, c['AD'], H, S, A).double()
    m.load_state_dict({mn: inp.W[wn].double() for mn, wn in zip(R.MODULE_NAMES, R.WNAMES)})
    bits = R.mask_value(mask, c['T'])
    emb = inp.emb.double().requires_grad_(True)
    pri, pos = m(emb, inp.act.double(), inp.noise.double(), [bool((bits >> t) & 1) for t in range(c['T'])])
    outs = {'h': pri['hidden_state'], 'mu_p': pri['mu'], 'sg_p': pri['sigma'], 'z_p': pri['sample'], 'mu_q': pos['mu'],
            'sg_q': pos['sigma'], 'z_q': pos['sample']}
    assert torch.equal(pri['hidden_state'], pos['hidden_state'])
    sum((outs[o] * inp.ups[g].double()).sum() for o, g in zip(R.OUT7, R.UP7)).backward()
    ref = R.reference64(name, mask, 'all')
    # the reference adds the kernels' min_std, float32(0.1) = 0.1 + 1.5e-9, the oracle the double 0.1: they agree to 1e-8, not 1e-15
    close = lambda a, b, n: torch.testing.assert_close(a, b, rtol=1e-7, atol=1e-8, msg=lambda s: f'{n}: {s}')      # noqa: E731
    for o in R.OUT7:
        close(ref[o], outs[o].detach(), o)
    close(ref['d_emb'], emb.grad, 'd_emb')
    pg = R.param_grads(ref, F64)
    named = dict(m.named_parameters())
    for mn, wn in zip(R.MODULE_NAMES, R.WNAMES):
        close(pg[wn], named[mn].grad, wn)


def test_reference_absent_upstreams():
    """an absent upstream is a zero upstream; with all seven absent every gradient and carry is exactly 0"""
    name, mask = 'tiny-b3-t5', 'alt'
    c, inp = R.CASE[name], R.inputs(name)
    for pat in ('zq_only', 'h_only', 'sgp_only', 'none'):
        ups = R.upstreams(inp, pat)
        zeros = {n: (torch.zeros_like(inp.ups[n]) if t is None else t) for n, t in ups.items()}
        for emu in (False, True):
            a = R.evaluate(c, inp, R.mask_value(mask, c['T']), ups, emu=emu)
            b = R.evaluate(c, inp, R.mask_value(mask, c['T']), zeros, emu=emu)
            for n in R.GRAD10 + ('dz_c', 'dh_c'):
                assert torch.equal(a[n], b[n]), (pat, n)
                if pat == 'none':
                    assert not a[n].any(), n


# ================================================================================================ emulation and bars
def test_emu_wave_dots_order():
    """the emulated order: within the bar against float64, exact on exactly representable inputs whatever the order, and equal to
    the sum written out by hand for one lane of a K = 1032 row (four sub-blocks of the first pass, then the second pass)"""
    g = R._gen('order')
    x, w = torch.randn(2, 1032, generator=g), torch.randn(3, 1032, generator=g)
    got = R.emu_wave_dots(x, w)
    ref, den = R._mv64(x, w)
    st = R.error_stats(got, ref, den)
    assert R.within(st, R.f32_bar(1032)), st
    xi, wi = torch.randint(-8, 9, (2, 1032), generator=g).float(), torch.randint(-8, 9, (3, 1032), generator=g).float()
    assert torch.equal(R.emu_wave_dots(xi, wi).double(), xi.double() @ wi.double().t())
    # by hand at one lane: lane 1 holds columns 4 ... 7 of every 256-column sub-block and, in the second pass, 1028 ... 1031
    x1, w1 = torch.zeros(1, 1032), torch.zeros(1, 1032)
    cols = [4, 5, 6, 7, 260, 516, 772, 1028, 1031]
    x1[0, cols], w1[0, cols] = x[0, cols], w[0, cols]
    p = lambda k: x1[0, k] * w1[0, k]          # noqa: E731
    acc = (p(4) + p(5)) + (p(6) + p(7))
    for k in (260, 516, 772):
        acc = acc + ((p(k) + 0) + (0 + 0.0))
    acc = acc + ((p(1028) + 0) + (0 + p(1031)))
    assert float(R.emu_wave_dots(x1, w1)[0, 0]) == float(acc)


def test_tables_are_current_and_emulation_passes():
    """STAGE_OWN_WORST and E2E_MEASURED recomputed.  The stage inputs are what the float32 recurrence produced, and the host's expf /
    tanhf differ between C libraries and vector widths, so another machine draws another sample of the same roundings: the tables
    hold within a factor 1.25 either way (against margins of 2 and 4).  Every stage without an entry stays within half of f32_bar."""
    worst = R.stage_worst()
    for kind, (rms, e) in sorted(worst.items()):
        print(f'RSSMSTAT worst emulated {kind}: rms {rms:.3f} max e {e:.3f} u sqrt(K)')
        if kind in R.STAGE_OWN_WORST:
            t = R.STAGE_OWN_WORST[kind]
            assert t[0] / 1.25 <= rms <= 1.25 * t[0] and t[1] / 1.25 <= e <= 1.25 * t[1], (kind, rms, e, t)
            assert rms > 0.23 or e > 2.4, f'{kind} stays within half of f32_bar: it needs no bar of its own'
        else:
            assert rms <= 0.23 and e <= 2.4, (kind, rms, e)
    assert set(R.STAGE_OWN_WORST) <= set(worst)
    assert set(R.E2E_MEASURED) == set(R.CASE)
    for name in R.CASE:
        got = R.e2e_measure(name)
        for g, e in got.items():
            t = R.E2E_MEASURED[name][g]
            assert t / 1.25 <= e <= 1.25 * t, (name, g, e, t)


@pytest.mark.parametrize('name,mask,pattern', R.runs(), ids=['-'.join(r) for r in R.runs()])
def test_emulation_passes_every_check(name, mask, pattern):
    c, inp = R.CASE[name], R.inputs(name)
    fails, rows = R.judge(c, inp, R.mask_value(mask, c['T']), R.upstreams(inp, pattern), R.emulated(name, mask, pattern), name)
    assert not fails, fails
    for stage, kind, K, st, share in rows:
        assert share <= (0.625 if kind in R.STAGE_OWN_WORST else 0.5), (stage, st, share)      # margin 2 (x 1.25, see above)


def test_mask_bits_nobody_reads_change_nothing():
    for name in ('tiny-b3-t5', 'tiny-b1-t64', 'tiny-b64-t1'):
        c, inp = R.CASE[name], R.inputs(name)
        ups = R.upstreams(inp, 'all')
        m = R.mask_value(c['masks'][0], c['T'])
        a = R.evaluate(c, inp, m & ~R.irrelevant_bits(c['T']), ups, emu=True)
        b = R.evaluate(c, inp, m | R.irrelevant_bits(c['T']), ups, emu=True)
        for n in a:
            assert torch.equal(a[n], b[n]), (name, n)


@pytest.mark.parametrize('fault', sorted(R.FAULTS))
def test_bars_bite(fault):
    """every planted fault is rejected by the per-stage and bit-for-bit checks at the case listed for it (and the same run without
    the fault passes: test_emulation_passes_every_check)"""
    name, mask = R.FAULTS[fault]
    c, inp = R.CASE[name], R.inputs(name)
    ups = R.upstreams(inp, 'all')
    res = R.evaluate(c, inp, R.mask_value(mask, c['T']), ups, emu=True, fault=fault)
    fails, _ = R.judge(c, inp, R.mask_value(mask, c['T']), ups, res, fault)
    print('\n'.join(fails))
    assert fails, f'{fault} passes every check at {name} / {mask}'
    # ... and by the end-to-end bars, except where the fault leaves the outputs and d_emb alone by construction
    ref = R.reference64(name, mask, 'all')
    e = R.e2e_errors(dict(ref, **R.param_grads(ref, F64)), dict({n: res[n] for n in R.OUT7 + ('d_emb',)}, **R.param_grads(res, torch.float32)))
    over = {n: v for n, v in e.items() if v > 4 * max(R.E2E_MEASURED[name].values())}
    assert over, f'{fault} passes the end-to-end bars'


# ================================================================================================ inputs and coverage
@pytest.mark.parametrize('name', list(R.CASE))
def test_inputs_do_not_saturate(name):
    gates, sig = R.saturation(name)
    assert gates <= 0.01 and sig <= 0.01, (gates, sig)


def test_every_edge_is_hit_by_a_named_case():
    K = {n: R.all_K(c) for n, c in R.CASE.items()}
    lanes = lambda k: k // 4          # noqa: E731  (active lanes of a pass of k < 1024 columns)
    assert max(K['tiny-b3-t5']) <= 12 and all(lanes(k) < 64 for k in K['tiny-b3-t5'])
    assert set(K['sub256-b5-t2']) == {132, 260, 264, 268, 780} and 260 % 256 == 4 and 780 % 256 == 12
    # the second pass of 1024 with lanes 0 and 1 only; (344, 516, 8, 4) has no other K past 1024 (4H = 1376 is a row count)
    assert [k for k in K['pass2-b8-t2'] if k > 1024] == [1032] and (1032 - 1024) // 4 == 2
    c = R.CASE['pass2-b8-t2']
    assert 3 * c['dims'][0] == 2 * c['dims'][1] == 1032
    assert any(k % 1024 == 0 for k in K['k1024-b1-t2']) and {256, 768} <= set(K['k256-b4-t2'])
    # the dynamic-LDS limit: supported, and one step of 4 in H, E or A past it is not
    c = R.CASE['lds-limit-b4-t1']
    H, S, E, A = c['dims']
    assert R.supported(c['B'], c['T'], H, S, E, A, c['AD']) == 1
    assert R.bwd_lds(4, H, S, E, A) == R.MAX_DYN_LDS
    assert R.supported(c['B'], c['T'], H + 4, S, E, A, c['AD']) == 0
    # several output rows per wave at the default grid, in every stage of either kernel that has more rows than waves
    nw = R.DEFAULT_CUS * R.WPB
    many = [s for s, (rows, _) in R.matvecs(c).items() if rows > nw]
    assert {'f0', 'f2', 'b0', 'b1', 'b2'} <= set(many), many
    for n in R.GRID_CASES:            # ... and at grids 1 and 3 in every stage
        assert all(rows > 3 * R.WPB for rows, _ in R.matvecs(R.CASE[n]).values())
    # slabs, steps, action widths, masks, upstream patterns
    assert {c['B'] for c in R.CASES} >= {1, 3, 4, 5, 8, 64} and {c['T'] for c in R.CASES} >= {1, 2, 5, 64}
    assert {c['AD'] for c in R.CASES} == {1, 2, 3}
    assert R.CASE['tiny-b64-t1']['dims'] == R.CASE['tiny-b1-t64']['dims'] == R.TINY
    assert {m for c in R.CASES for m in c['masks']} == {'none', 'ones', 'alt', 'bit0', 'last', 'hi'}
    assert R.mask_value('last', 5) == 1 << 3 and R.mask_value('hi', 64) == 3 << 62 and R.mask_value('last', 64) == 1 << 62
    assert set(R.CASE['tiny-b3-t5']['ups']) == set(R.UPS_PATTERNS)
    for c in R.CASES:
        H, S, E, A = c['dims']
        assert R.supported(c['B'], c['T'], H, S, E, A, c['AD']) == 1, c['name']
    for f, (name, mask) in R.FAULTS.items():
        assert mask in R.CASE[name]['masks'], f
    # no case is left out: every case x mask and every upstream pattern is a run, the grid and family cases exist
    visited = set(R.runs())
    assert len(visited) == len(R.runs())
    for c in R.CASES:
        assert {(c['name'], m, 'all') for m in c['masks']} <= visited and {(c['name'], c['masks'][0], u) for u in c['ups']} <= visited
    assert set(R.GRID_CASES) | set(R.FAMILY_CASES) <= set(R.CASE) and set(R.E2E_MEASURED) == set(R.CASE)


# ================================================================================================ host-side mirrors
def test_size_mirrors_match_their_formulas():
    for c in R.CASES:
        H, S, E, A = c['dims']
        shp = R.wshapes(c)
        big = ('w_pre', 'w_ih', 'w_hh', 'w_p0', 'w_p2', 'w_q0', 'w_q2')          # the seven transposed matrices
        assert R.transposed_floats(H, S, E, A) == sum(math.prod(shp[n]) for n in big)
        wd = R.widths(c)
        Bc = min(c['B'], R.BM)
        # scratch: dxp, dxq, two dh carries, dz carry, sized for all B rows (a slab uses its first Bc rows of each)
        assert R.scratch_floats(c['B'], H, S, E, A) == c['B'] * (wd['xp'] + wd['xq'] + 2 * H + S)
        assert R.scratch_floats(Bc, H, S, E, A) <= R.scratch_floats(c['B'], H, S, E, A)
            # LDS: forward xa [B][max(HQ, S)], xb [B][HP], h [B][H], a [B][AD]; backward xa / xb hold max(., 3H, 2S), dd [B][H]; 16 spare
        assert R.fwd_lds(Bc, H, S, E, A, c['AD']) == 4 * (Bc * (max(wd['xq'], wd['zprev']) + wd['xp'] + H + c['AD']) + 16)
        assert R.bwd_lds(Bc, H, S, E, A) == 4 * (Bc * (max(wd['xq'], wd['gi'], wd['dmls_q']) + max(wd['xp'], wd['gi'], wd['dmls_p']) + H) + 16)


def test_support_mirror_sweep():
    """supported() over the limit in every direction and at each violated condition"""
    sup = lambda base, **kw: R.supported(**dict(base, **kw))          # noqa: E731
    assert sup(R.LIMIT_BWD) == 1 and sup(R.LIMIT_BWD, B=64, T=64) == 1 and sup(R.LIMIT_BWD, B=1, H=4 * 1460) == 1
    p = R.LIMIT_BWD
    assert R.bwd_lds(4, p['H'], p['S'], p['E'], p['A']) == R.MAX_DYN_LDS > R.fwd_lds(4, p['H'] + 4, p['S'], p['E'], p['A'], p['AD'])
    assert sup(R.LIMIT_BWD, S=2188) == 1
    for kw in R.PAST_BWD:
        assert sup(R.LIMIT_BWD, **kw) == 0, kw
    p = R.LIMIT_FWD
    assert sup(p) == 1 and R.fwd_lds(4, p['H'], p['S'], p['E'], p['A'], p['AD']) == R.MAX_DYN_LDS == R.bwd_lds(4, p['H'], p['S'], p['E'], p['A']) + 64
    for kw in R.PAST_FWD:
        q = dict(p, **kw)
        assert sup(p, **kw) == 0, kw
        fits = R.fwd_lds(min(q['B'], 4), q['H'], q['S'], q['E'], q['A'], q['AD']) <= R.MAX_DYN_LDS
        assert not (R.dims_ok(**q) and fits), kw          # the forward itself refuses
    # forward-bound limit: a wide embedding, both kernels' xa holds HQ = H + E + A
    assert R.supported(4, 1, 4, 4, 10196, 4, 1) == 1 and R.supported(4, 1, 4, 4, 10200, 4, 1) == 0
    for H in range(1400, 1500, 4):
        assert R.supported(4, 1, H, 4, 4, 4, 2) == int(H <= 1460)


def test_ops_tables_are_the_reference_tables():
    """ops.RSSMFusedFn addresses its tensors by the names and in the table orders stated here (plain data: no GPU, no library)"""
    from muvo_amd import ops
    assert ops.RSSM_PARAM_PAIRS == R.PARAM_PAIRS
    assert tuple(ops.RSSM_WEIGHTS) == R.WNAMES and tuple(ops.RSSM_WEIGHTS.values()) == R.MODULE_NAMES
    assert tuple(ops.RSSM_KEEP12) == R.KEEP12 and tuple(ops.RSSM_GRAD10) == R.GRAD10
    for c in R.CASES:
        wd = R.widths(c)
        dims = (1, 1, *c['dims'], c['AD'])
        made = dict(ops._rssm_new(ops.RSSM_KEEP12, dims, 'cpu'), **ops._rssm_new(ops.RSSM_GRAD10, dims, 'cpu'))
        assert {n: t.shape[-1] for n, t in made.items()} == {n: wd[n] for n in R.KEEP12 + R.GRAD10}, c['name']
