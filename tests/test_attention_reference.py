"""CPU: the float64 reference, the bars, the spiked inputs and the case list of tests/attention_reference.py, which
tests/test_attention_stream_gpu.py applies to the streamed attention kernels; and what of the feature needs no GPU.  Shown here:
  * the float64 reference agrees with torch autograd in float64, with and without a keep-mask;
  * the MEASURED table is the float32 evaluation of the blocked recurrence (every case is evaluated again: within a factor of 4
    either way, which is what another thread count's summation order can move it by, and never above the bar);
  * the spiked inputs do what they are for (spiked_facts asserts it), and the float32 recurrence stays finite on them;
  * the bars bite: the float64 result rounded to float32 with ONE planted error each is rejected by the very comparison the GPU
    test uses;
  * the library's new entry points answer and validate their arguments without a device, the fused ones keep their range;
  * ops.attention_path."""
import ctypes as C

import pytest
import torch

import attention_reference as R


def test_reference_agrees_with_autograd():
    for c in (R.case(37, 2, 3, 16), R.case(21, 1, 2, 48, p=0.5)):
        inp = R.inputs(c)
        keep = inp.get('cpu_keep')
        ref = R.reference64(inp['qkv'], c['H'], inp['dout'], keep)
        x = inp['qkv'].double().requires_grad_(True)
        E = c['H'] * c['DH']
        q, k, v = (R._heads(t, c['H']) for t in x.split(E, dim=-1))
        s = q @ k.transpose(-1, -2) / c['DH'] ** 0.5
        P = torch.softmax(s, -1)
        o = R._packed((P if keep is None else P * keep.double()) @ v)
        g, = torch.autograd.grad(o, x, inp['dout'].double())
        assert torch.allclose(ref['o'], o.detach(), rtol=1e-11, atol=1e-11)
        assert torch.allclose(ref['lse'], torch.logsumexp(s, -1).reshape(-1, c['L']).detach(), rtol=1e-11, atol=1e-11)
        assert torch.allclose(ref['dqkv'], g, rtol=1e-11, atol=1e-11)


def test_case_list():
    ids = [R.case_id(c) for c in R.ALL_CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(R.MEASURED)
    bk = R.BK
    assert [c['L'] for c in R.PARITY_CASES[:8]] == [1, 15, bk - 1, bk, bk + 1, 385, 2 * bk + 23, 1037]
    assert {(c['H'], c['DH']) for c in R.PARITY_CASES[8:]} == {(3, 16), (3, 32), (3, 64)}
    assert -(-R.BIG_CASE['L'] // bk) == 41


def test_resident_case_list():
    from muvo_amd import ops
    cases = R.RESIDENT_CASES + R.RESIDENT_DROPOUT_CASES
    assert all(R.case_id(c).endswith('-res') and R.float32_block(c) == c['L'] for c in cases)
    assert not any(c['res'] for c in R.STREAM_CASES) and {R.float32_block(c) for c in R.STREAM_CASES} == {R.BK}
    assert all(ops.lib().muvo_attention_supported(c['L'], c['DH']) == 1 for c in cases)
    wg, top = R.RES_WG, R.RES_MAXL
    assert [c['L'] for c in R.RESIDENT_CASES[:10]] == [1, 15, 16, 17, wg - 1, wg, wg + 1, 324, top - 1, top]
    assert [(c['L'], c['H'], c['DH']) for c in R.RESIDENT_CASES[10:]] == [(279, 3, 16), (279, 3, 32), (279, 3, 64), (R.RES_MAXL_D64, 2, 64)]
    assert [(c['L'], c['p']) for c in R.RESIDENT_DROPOUT_CASES] == [(324, 0.1), (324, 0.5)]
    assert ops.lib().muvo_attention_supported(R.RES_MAXL_D64 + 1, 64) == 0 and ops.lib().muvo_attention_supported(top + 1, 48) == 0


@pytest.mark.parametrize('c', R.ALL_CASES, ids=R.case_id)
def test_measured_table_is_the_float32_evaluation(c):
    e = R.float32_errors(c)
    for n, v in e.items():
        m = R.MEASURED[R.case_id(c)][n]
        print(f'ATTNSTAT float32 {R.case_id(c)} {n}: {v:.3e} (tabulated {m:.2e})')
        assert v <= 4 * m and m <= 4 * v or (m == 0.0 and v == 0.0), (n, v, m)
    if c is R.BIG_CASE:
        R._reference_cached.cache_clear()          # 215 MB matrices: not kept for the rest of the session


@pytest.mark.parametrize('c', R.SPIKED_CASES, ids=R.case_id)
def test_spiked_inputs_force_the_rescale(c):
    inp, _ = R.reference(c)
    smax, where = R.spiked_facts(c, inp['qkv'])
    print(f'ATTNSTAT spiked {R.case_id(c)}: max |s| {smax:.1f}, row maxima {where}')
    sub = R.blocked_float32(inp['qkv'], c['H'], R.BK, inp['dout'])
    assert all(torch.isfinite(sub[n]).all() for n in R.NAMES)
    plain = R.inputs(dict(c, spiked=False))['qkv']
    with pytest.raises(AssertionError):
        R.spiked_facts(c, plain)                   # the random inputs have no such scores


def _planted(c, ref, what):
    """the float64 result rounded to float32 with one planted error"""
    inp, _ = R.reference(c)
    got = {n: ref[n].float() for n in R.NAMES}
    if what in ('o_rescale', 'l_rescale', 'tail_key'):
        probe = R.blocked(inp['qkv'], c['H'], R.BK, dtype=R.F64)
        a = probe['alpha_last']                    # the last block's factors: plant where the factor is furthest from 1
        idx = tuple(int(i) for i in torch.unravel_index((a - 1).abs().argmax(), a.shape))
        assert float(a[idx]) < 0.9
        bad = R.blocked(inp['qkv'], c['H'], R.BK, dtype=R.F64, fault=(what, -(-c['L'] // R.BK) - 1, idx))
        assert torch.allclose(probe['o'], ref['o'], rtol=1e-10, atol=1e-12)        # without the fault: the reference
        got['o'], got['lse'] = bad['o'].float(), bad['lse'].float()
    elif what == 'lse':
        got['lse'][1, c['L'] // 2] += torch.log(torch.tensor(1 + 1e-4))
    elif what == 'dk_row':
        E = c['H'] * c['DH']
        row = int(ref['dqkv'][:, :, E:2 * E].abs().amax(dim=(1, 2)).argmax())
        got['dqkv'][row, :, E:2 * E] *= 1 + 1e-4
    return got


@pytest.mark.parametrize('what', ['o_rescale', 'l_rescale', 'tail_key', 'lse', 'dk_row'])
def test_bars_bite(what):
    c = R.PARITY_CASES[6]                          # L = 2 BK + 23: three blocks, a tail
    _, ref = R.reference(c)
    clean = R.compare(R.case_id(c), {n: ref[n].float() for n in R.NAMES}, ref)
    assert not R.failures(clean), clean            # rounding alone passes
    cmp = R.compare(R.case_id(c), _planted(c, ref, what), ref)
    print('\n'.join(R.statlines(f'planted {what}', cmp)))
    assert R.failures(cmp), cmp


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def test_stream_entry_points_without_gpu():
    from muvo_amd import ops
    L = ops.lib()
    assert [L.muvo_attention_stream_supported(l, dh) for l, dh in ((1, 16), (385, 48), (5184, 64))] == [1, 1, 1]
    assert [L.muvo_attention_stream_supported(l, dh) for l, dh in ((385, 12), (0, 48))] == [0, 0]
    bq, bk = C.c_int(0), C.c_int(0)
    assert L.muvo_attention_stream_blocks(C.byref(bq), C.byref(bk)) == 0
    assert bq.value > 0 and bk.value > 0 and bq.value % 16 == 0 and bk.value % 16 == 0
    assert (bq.value, bk.value) == (R.BQ, R.BK), 'tests/attention_reference.py: MEASURED and the case list are for another block size'
    assert L.muvo_attention_stream_blocks(None, None) == -1
    buf = (C.c_float * 16)()
    args = (8, 1, 1)
    assert L.muvo_attention_stream_fwd(buf, buf, buf, *args, 12, C.c_float(0.0), C.c_uint64(0), None) == -1
    assert b'head dim' in L.muvo_last_error()
    assert L.muvo_attention_stream_fwd(None, buf, buf, *args, 16, C.c_float(0.0), C.c_uint64(0), None) == -1
    assert L.muvo_attention_stream_fwd(buf, None, None, *args, 16, C.c_float(0.0), C.c_uint64(0), None) == -1
    assert L.muvo_attention_stream_bwd(buf, buf, buf, buf, buf, None, *args, 16, C.c_float(0.0), C.c_uint64(0), None) == -1
    assert L.muvo_attention_stream_bwd(buf, buf, buf, buf, buf, buf, 0, 1, 1, 16, C.c_float(0.0), C.c_uint64(0), None) == -1
    assert L.muvo_attention_supported(385, 48) == 0 and L.muvo_attention_supported(384, 48) == 1


def test_attention_path(monkeypatch):
    from muvo_amd import ops
    monkeypatch.setattr(ops, 'FLASH_ATTENTION', True)
    assert ops.attention_path(324, 48) == 'fused'
    assert ops.attention_path(1037, 48) == 'stream' and ops.attention_path(5184, 48) == 'stream'
    assert ops.attention_path(70, 12) == 'unfused' and ops.attention_path(1037, 12) == 'unfused'
    monkeypatch.setattr(ops, 'FLASH_ATTENTION', False)
    assert {ops.attention_path(l, dh) for l, dh in ((324, 48), (1037, 48), (5184, 48), (70, 12))} == {'unfused'}
