"""CPU: the float64 reference, the float32 recurrence, the bars and the case list of tests/attention_mask_reference.py, which
tests/test_attention_mask_gpu.py applies to the masked attention kernels; and what of the feature needs no GPU.  Shown here:
  * reference64_masked agrees with float64 autograd through a masked softmax on the frames that have a live key;
  * the all-masked definition (o = 0, lse = -inf, dqkv = 0, nothing else non-finite) holds in the reference and in the recurrence;
  * the MEASURED table is the float32 evaluation of blocked_masked (within a factor of 4 either way, never above the bar);
  * the bars bite: a mask applied after the maximum, a mask shifted by one frame and an unguarded rescale are each rejected by the
    very comparison the GPU test uses;
  * the masked result equals the unmasked float64 reference on the gathered subsequence of live keys;
  * the new entry points validate their arguments without a device; ops.masked_attention_path."""
import ctypes as C

import pytest
import torch

import attention_mask_reference as M
import attention_reference as R


def test_case_list():
    ids = [M.case_id(c) for c in M.ALL_CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(M.MEASURED)
    assert all(c['res'] for c in M.RESIDENT_CASES) and not any(c['res'] for c in M.STREAM_CASES)
    assert [c['L'] for c in M.RESIDENT_CASES] == [1, 1, 17, 17, 324, 384, 279, 279, 279, 288, 279]
    assert [c['L'] for c in M.STREAM_CASES] == [129, 129, 279, 279, 279, 1037, 279]
    assert [(c['L'], c['p'], c['res']) for c in M.DROPOUT_CASES] == [(324, 0.1, True), (517, 0.1, False)]
    for c in M.ALL_CASES:
        m = M.key_mask(c)
        if c['N'] > 1:                                     # different masks per frame
            assert len({tuple(r.tolist()) for r in m}) == c['N'] or c['L'] == 1, M.case_id(c)
    by = {M.case_id(c): M.key_mask(c) for c in M.ALL_CASES}
    assert by['L1-N3H2D48-res-key0'].tolist() == [[False], [True], [False]]
    assert by['L17-N3H2D48-res-tile0'][0].tolist() == [True] * 16 + [False]
    assert by['L129-N3H2D48-onlytail'][0].tolist() == [True] * 128 + [False]
    assert by['L129-N3H2D48-notail'][0].tolist() == [False] * 128 + [True]
    mid = by['L279-N3H2D48-middle'][0]
    assert mid[R.BK:2 * R.BK].all() and not mid[:R.BK].any() and not mid[2 * R.BK:].any()
    assert by['L279-N3H2D48-deadframe'][1].all() and not by['L279-N3H2D48-deadframe'][2].any()
    assert by['L324-N3H2D48-res-sensors'].sum(1).tolist() == [0, 260, 64]


def test_resident_cases_fit():
    from muvo_amd import ops
    assert all(ops.lib().muvo_attention_supported(c['L'], c['DH']) == 1 for c in M.ALL_CASES if c['res'])


@pytest.mark.parametrize('c,gap,rows', [(M.STREAM_CASES[5], 50.0, 40), (M.STREAM_CASES[6], 104.0, 20), (M.RESIDENT_CASES[10], 104.0, 20)],
                         ids=lambda v: M.case_id(v) if isinstance(v, dict) else None)
def test_spikes_are_masked(c, gap, rows):
    """The masks of the spiked cases hide the row's largest score, in rows whose maximum lies in the first, a middle and the last
    block.  As the generator makes them that score lies up to 93 above the row's largest live score (more than 50 in 40 rows a
    frame): a kernel that takes the maximum before masking keeps a few denormal bits there.  With the masked keys doubled it lies
    more than 104 above in at least 20 rows a frame: exp(live - maximum) is 0 in float32 and such a kernel returns 0 / 0.  The
    reference does not depend on the doubling."""
    inp, ref = M.reference(c)
    R.spiked_facts(c, R.inputs(c)['qkv'])
    E, H = c['H'] * c['DH'], c['H']
    q, k = R._heads(inp['qkv'][:, :, :E].double(), H), R._heads(inp['qkv'][:, :, E:2 * E].double(), H)
    s = q @ k.transpose(-1, -2) / c['DH'] ** 0.5
    top = s.argmax(-1)                                                        # (N, H, L)
    live = s.masked_fill(inp['key_mask'][:, None, None, :], float('-inf')).amax(-1)
    hidden = torch.gather(inp['key_mask'][:, None, :].expand(-1, H, -1), 2, top) & (s.amax(-1) - live > gap)
    assert int(hidden[0].sum()) >= rows and int(hidden[2].sum()) >= rows and not hidden[1].any()
    blocks = set((top[hidden] // R.BK).tolist())
    assert {0, -(-c['L'] // R.BK) - 1} <= blocks and len(blocks) > 2
    if c['boost'] != 1.0:
        plain = M.reference64_masked(R.inputs(c)['qkv'], H, inp['dout'], inp['key_mask'])
        assert all(torch.equal(plain[n], ref[n]) for n in R.NAMES)


def test_reference_agrees_with_autograd():
    for c in (M.mcase('t', [[(0, 37, 3)], [(5, 30)]], 37, N=2, H=3, DH=16), M.mcase('t', [[(20, 21)]], 21, N=1, H=2, DH=48, p=0.5)):
        inp = R.inputs(c)
        keep, mask = inp.get('cpu_keep'), M.key_mask(c)
        ref = M.reference64_masked(inp['qkv'], c['H'], inp['dout'], mask, keep)
        x = inp['qkv'].double().requires_grad_(True)
        E = c['H'] * c['DH']
        q, k, v = (R._heads(t, c['H']) for t in x.split(E, dim=-1))
        s = (q @ k.transpose(-1, -2) / c['DH'] ** 0.5).masked_fill(mask[:, None, None, :], float('-inf'))
        P = torch.softmax(s, -1)
        o = R._packed((P if keep is None else P * keep.double()) @ v)
        g, = torch.autograd.grad(o, x, inp['dout'].double())
        assert torch.allclose(ref['o'], o.detach(), rtol=1e-11, atol=1e-11)
        assert torch.allclose(ref['lse'], torch.logsumexp(s, -1).reshape(-1, c['L']).detach(), rtol=1e-11, atol=1e-11)
        assert torch.allclose(ref['dqkv'], g, rtol=1e-11, atol=1e-11)
        assert (ref['dqkv'][:, :, E:].reshape(c['L'], c['N'], 2, E)[mask.T] == 0).all()      # dk, dv rows of masked keys


@pytest.mark.parametrize('c', [M.RESIDENT_CASES[1], M.STREAM_CASES[4]], ids=M.case_id)
def test_all_masked_definition(c):
    inp, ref = M.reference(c)
    dead = inp['key_mask'].all(1)
    assert dead.tolist() == [False, True, False]
    E, H, L = c['H'] * c['DH'], c['H'], c['L']
    for got in (ref, M.blocked_masked(inp['qkv'], H, R.float32_block(c), inp['key_mask'], inp['dout'])):
        assert (got['o'][:, dead] == 0).all() and (got['dqkv'][:, dead] == 0).all()
        lse = got['lse'].reshape(c['N'], H, L)
        assert (lse[dead] == float('-inf')).all() and torch.isfinite(lse[~dead]).all()
        assert torch.isfinite(got['o']).all() and torch.isfinite(got['dqkv']).all()
    x = inp['qkv'].double()                                                   # what torch makes of it: NaN, hence the definition
    s = torch.zeros(1, L).masked_fill(inp['key_mask'][1:2], float('-inf'))
    assert torch.isnan(torch.softmax(s, -1)).all() and torch.isfinite(x).all()


@pytest.mark.parametrize('c', M.ALL_CASES, ids=M.case_id)
def test_measured_table_is_the_float32_evaluation(c):
    e = M.float32_errors(c)
    for n, v in e.items():
        m = M.MEASURED[M.case_id(c)][n]
        print(f'ATTNSTAT float32 {M.case_id(c)} {n}: {v:.3e} (tabulated {m:.2e})')
        assert v <= 4 * m and m <= 4 * v or (m == 0.0 and v == 0.0), (n, v, m)


@pytest.mark.parametrize('what,idx', [('mask_after_max', 6), ('frame_shift', 5), ('frame_shift', 2), ('unguarded', 0)])
def test_bars_bite(what, idx):
    """blocked_masked with one planted error: without the error it passes, with it the comparison of the GPU test rejects it (NaN
    from exp(-inf + inf); another frame's mask; 0 / 0 where the maximum was a masked key).  In float64
    rounded to float32, but for the mask after the maximum: that error IS float32's - exp(s - max) underflows only there."""
    c = M.STREAM_CASES[idx]
    inp, ref = M.reference(c)
    dtype = torch.float32 if what == 'mask_after_max' else R.F64

    def run(fault):
        got = M.blocked_masked(inp['qkv'], c['H'], R.BK, inp['key_mask'], inp['dout'], dtype=dtype, fault=fault)
        return M.compare(M.case_id(c), {n: got[n].float() for n in R.NAMES}, ref)

    clean = run(None)
    assert not M.failures(clean), clean
    cmp = run(what)
    print('\n'.join(M.statlines(f'planted {what} {M.case_id(c)}', cmp)))
    bad = M.failures(cmp)
    assert 'o' in bad and 'lse' in bad, cmp


@pytest.mark.parametrize('c', [M.RESIDENT_CASES[3], M.STREAM_CASES[3], M.STREAM_CASES[5]], ids=M.case_id)
def test_masked_equals_gathered_subsequence(c):
    """per frame: the masked result on every query, and the dk / dv of the live keys, are the unmasked float64 reference run with
    the live keys alone (all L queries, K and V gathered)"""
    inp, ref = M.reference(c)
    E, H, L = c['H'] * c['DH'], c['H'], c['L']
    scale = c['DH'] ** -0.5
    for n in range(c['N']):
        live = ~inp['key_mask'][n]
        q, k, v = (R._heads(inp['qkv'][:, n:n + 1, i * E:(i + 1) * E].double(), H) for i in range(3))
        do = R._heads(inp['dout'][:, n:n + 1].double(), H)
        kg, vg = k[:, :, live], v[:, :, live]
        s = (q @ kg.transpose(-1, -2)) * scale
        P = torch.softmax(s, -1)
        o = P @ vg
        dP = do @ vg.transpose(-1, -2)
        dS = (dP - (do * o).sum(-1, keepdim=True)) * P
        assert torch.allclose(ref['o'][:, n:n + 1], R._packed(o), rtol=1e-11, atol=1e-12)
        assert torch.allclose(ref['lse'][n * H:(n + 1) * H], torch.logsumexp(s, -1)[0], rtol=1e-11, atol=1e-12)
        assert torch.allclose(ref['dqkv'][:, n:n + 1, :E], R._packed(dS @ kg * scale), rtol=1e-10, atol=1e-11)
        assert torch.allclose(ref['dqkv'][live, n:n + 1, E:2 * E], R._packed(dS.transpose(-1, -2) @ q * scale), rtol=1e-10, atol=1e-11)
        assert torch.allclose(ref['dqkv'][live, n:n + 1, 2 * E:], R._packed(P.transpose(-1, -2) @ do), rtol=1e-10, atol=1e-11)
        assert (ref['dqkv'][~live, n, E:] == 0).all()


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def test_mask_entry_points_without_gpu():
    from muvo_amd import ops
    L = ops.lib()
    buf = (C.c_float * 64)()
    mask = (C.c_uint8 * 64)()
    base = C.addressof(mask)
    assert base % 4 == 0
    z, sd = C.c_float(0.0), C.c_uint64(0)
    for fwd in (L.muvo_attention_mask_fwd, L.muvo_attention_stream_mask_fwd):
        assert fwd(buf, buf, buf, 8, 1, 1, 12, z, sd, None, C.c_void_p(base), C.c_int64(8)) == -1
        assert b'head dim' in L.muvo_last_error()
        assert fwd(buf, None, buf, 8, 1, 1, 16, z, sd, None, C.c_void_p(base), C.c_int64(8)) == -1
        assert fwd(buf, buf, buf, 8, 1, 1, 16, z, sd, None, C.c_void_p(base), C.c_int64(6)) == -1       # stride no multiple of 4
        assert b'key mask' in L.muvo_last_error()
        assert fwd(buf, buf, buf, 9, 1, 1, 16, z, sd, None, C.c_void_p(base), C.c_int64(8)) == -1       # stride < roundup(L, 4)
        assert b'key mask' in L.muvo_last_error()
        assert fwd(buf, buf, buf, 8, 1, 1, 16, z, sd, None, C.c_void_p(base + 1), C.c_int64(8)) == -1   # base not aligned
        assert b'key mask' in L.muvo_last_error()
    assert L.muvo_attention_mask_fwd(buf, buf, buf, 385, 1, 1, 48, z, sd, None, C.c_void_p(base), C.c_int64(400)) == -1
    assert b"fused kernel's range" in L.muvo_last_error()
    assert L.muvo_attention_mask_bwd(buf, buf, buf, buf, None, 8, 1, 1, 16, z, sd, None, C.c_void_p(base), C.c_int64(8)) == -1
    assert L.muvo_attention_stream_mask_bwd(buf, buf, buf, buf, buf, None, 8, 1, 1, 16, z, sd, None, C.c_void_p(base), C.c_int64(8)) == -1
    assert L.muvo_attention_stream_mask_bwd(buf, buf, buf, buf, buf, buf, 8, 1, 1, 16, z, sd, None, C.c_void_p(base), C.c_int64(7)) == -1


def test_masked_attention_path(monkeypatch):
    from muvo_amd import ops
    monkeypatch.setattr(ops, 'FLASH_ATTENTION', True)
    assert ops.masked_attention_path(324, 48) == 'fused' and ops.masked_attention_path(288, 64) == 'fused'
    assert ops.masked_attention_path(385, 48) == 'stream' and ops.masked_attention_path(289, 64) == 'stream'
    assert ops.STREAM_MIN_L == 385 and ops.attention_path(289, 64) == 'unfused'       # without a mask that length is unfused
    with pytest.raises(ValueError):
        ops.masked_attention_path(70, 12)
    monkeypatch.setattr(ops, 'FLASH_ATTENTION', False)
    with pytest.raises(ValueError, match='MUVO_FLASH_ATTN'):
        ops.masked_attention_path(324, 48)
