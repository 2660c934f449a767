"""GPU: the key-padding mask of the fused attention kernels (muvo_amd/csrc/attention.hip), through the C ABI - muvo_attention_mask_*
resident, muvo_attention_stream_mask_* streamed - against the float64 reference of tests/attention_mask_reference.py under its bars
(4 x the float32 CPU evaluation of the same recurrence on the same inputs; tests/test_attention_mask_reference.py shows those bars
reject a mask applied after the maximum, a mask of the wrong frame and an unguarded rescale).  Every listed case: o, lse and dqkv,
exact zeros in the dk / dv rows of masked keys, the all-masked frame as defined and nothing non-finite but its lse.  An all-zero
mask gives the bits of the unmasked entry points; two calls give the same bits; dropout with the library's own keep-mask; and
ops.attention(..., key_mask=) picks the path and never drops the mask."""
import ctypes as C

import pytest
import torch

import attention_mask_reference as M
import attention_reference as R

pytestmark = pytest.mark.gpu


def _entry(path, masked):
    from muvo_amd import ops
    L = ops.lib()
    return {('fused', False): (L.muvo_attention_fwd, L.muvo_attention_bwd), ('fused', True): (L.muvo_attention_mask_fwd, L.muvo_attention_mask_bwd),
            ('stream', False): (L.muvo_attention_stream_fwd, L.muvo_attention_stream_bwd),
            ('stream', True): (L.muvo_attention_stream_mask_fwd, L.muvo_attention_stream_mask_bwd)}[path, masked]


def _kernels(c, inp, dev, mask, p=0.0, seed=0):
    """{o, lse, dqkv} of the case's path through the C ABI; mask: (N, L) bool on the CPU, or None = the unmasked entry points"""
    from muvo_amd import ops
    path = 'fused' if c['res'] else 'stream'
    if c['res']:
        assert ops.lib().muvo_attention_supported(c['L'], c['DH']) == 1
    fwd, bwd = _entry(path, mask is not None)
    L, N, H, DH = c['L'], c['N'], c['H'], c['DH']
    qkv, dout = inp['qkv'].to(dev), inp['dout'].to(dev)
    o, lse, dqkv = torch.empty_like(dout), torch.empty(N * H, L, device=dev), torch.empty_like(qkv)
    tail = ()
    if mask is not None:
        rows = ops.key_mask_rows(mask.to(dev), N, L)
        assert rows.shape[1] % 16 == 0 and rows.data_ptr() % 16 == 0
        tail = (ops._p(rows), ops._i64(rows.shape[1]))
    dims = (L, N, H, DH, ops._fl(p), C.c_uint64(seed), ops._st())
    ops._ck(fwd(ops._f(qkv), ops._f(o), ops._f(lse), *dims, *tail))
    dws = (ops._f(torch.empty_like(lse)),) if path == 'stream' else ()
    ops._ck(bwd(ops._f(qkv), ops._f(o), ops._f(dout), ops._f(lse), ops._f(dqkv), *dws, *dims, *tail))
    torch.cuda.synchronize()
    return {'o': o, 'lse': lse, 'dqkv': dqkv}


def _check(c, got, ref, tag=''):
    cmp = M.compare(M.case_id(c), got, ref)
    print('\n'.join(M.statlines(M.case_id(c) + tag, cmp)))
    bad = M.failures(cmp)
    assert not bad, bad


def _exact_facts(c, got, mask):
    """what holds exactly: zeros in the dk / dv rows of masked keys, the all-masked frame, nothing non-finite but its lse"""
    E, H, L, N = c['H'] * c['DH'], c['H'], c['L'], c['N']
    o, lse, dqkv = got['o'].cpu(), got['lse'].cpu().reshape(N, H, L), got['dqkv'].cpu()
    assert (dqkv[:, :, E:].reshape(L, N, 2, E)[mask.T] == 0).all(), 'dk / dv rows of masked keys'
    dead = mask.all(1)
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all() and torch.isfinite(lse[~dead]).all()
    assert (o[:, dead] == 0).all() and (dqkv[:, dead] == 0).all() and (lse[dead] == float('-inf')).all()


@pytest.mark.parametrize('c', M.RESIDENT_CASES + M.STREAM_CASES, ids=M.case_id)
def test_float64_parity(dev, c):
    inp, ref = M.reference(c)
    got = _kernels(c, inp, dev, inp['key_mask'])
    _exact_facts(c, got, inp['key_mask'])
    _check(c, got, ref)


@pytest.mark.parametrize('c', M.DROPOUT_CASES, ids=M.case_id)
def test_dropout(dev, c):
    """float64 with the library's own keep-mask - its dropout over ones, same seed, index ((n*H + h)*L + query)*L + key with L
    the full length - as tests/test_attention_stream_gpu.py::test_dropout: the live pairs draw the bits of an unmasked run"""
    from muvo_amd import ops
    p, seed = c['p'], M.DROPOUT_SEED
    inp = M.inputs(c)
    got = _kernels(c, inp, dev, inp['key_mask'], p, seed)
    _exact_facts(c, got, inp['key_mask'])
    keep = ops.dropout(torch.ones(c['N'], c['H'], c['L'], c['L'], device=dev), p, seed).cpu()
    assert abs(float((keep > 0).float().mean()) - (1 - p)) < 5e-3
    ref = M.reference64_masked(inp['qkv'], c['H'], inp['dout'], inp['key_mask'], keep)
    _check(c, got, ref, ' library mask')
    plain = _kernels(c, inp, dev, inp['key_mask'])
    assert not torch.allclose(got['o'], plain['o'])         # the dropout does something


@pytest.mark.parametrize('c', [M.RESIDENT_CASES[4], M.RESIDENT_CASES[9], M.STREAM_CASES[2], M.DROPOUT_CASES[1]], ids=M.case_id)
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_zero_mask_gives_the_unmasked_bits(dev, c, p):
    inp = M.inputs(c)
    a = _kernels(c, inp, dev, None, p, M.DROPOUT_SEED)
    b = _kernels(c, inp, dev, torch.zeros(c['N'], c['L'], dtype=torch.bool), p, M.DROPOUT_SEED)
    for n in R.NAMES:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize('c', [M.RESIDENT_CASES[4], M.STREAM_CASES[4], M.STREAM_CASES[5]], ids=M.case_id)
def test_reproducible(dev, c):
    inp = M.inputs(c)
    for p in (0.0, 0.1):
        a, b = (_kernels(c, inp, dev, inp['key_mask'], p, M.DROPOUT_SEED) for _ in range(2))
        for n in R.NAMES:
            assert torch.equal(a[n], b[n]), (n, p)             # -inf == -inf


def test_mask_row_stride(dev):
    """the rows of one frame, not of its neighbour: a mask tensor with a wider row stride gives the same bits"""
    from muvo_amd import ops
    c = M.STREAM_CASES[3]
    inp = M.inputs(c)
    a = _kernels(c, inp, dev, inp['key_mask'])
    L, N, H, DH = c['L'], c['N'], c['H'], c['DH']
    wide = torch.ones(N, 512, dtype=torch.uint8, device=dev)                   # beyond L: masked bytes that must not matter
    wide[:, :L] = inp['key_mask'].to(dev)
    qkv = inp['qkv'].to(dev)
    o, lse = torch.empty(L, N, H * DH, device=dev), torch.empty(N * H, L, device=dev)
    ops._ck(ops.lib().muvo_attention_stream_mask_fwd(ops._f(qkv), ops._f(o), ops._f(lse), L, N, H, DH, ops._fl(0.0), C.c_uint64(0), ops._st(),
                                                     ops._p(wide), ops._i64(512)))
    assert torch.equal(o, a['o']) and torch.equal(lse, a['lse'])


@pytest.mark.parametrize('L,path', [(324, 'fused'), (385, 'stream'), (17, 'fused')])
def test_ops_attention_with_a_mask(dev, monkeypatch, L, path):
    from muvo_amd import ops
    c = M.mcase('ops', [[], [(0, L - L // 5)], [(L - L // 5, L)]], L, res=path == 'fused')
    inp = M.inputs(c)
    want = _kernels(c, inp, dev, inp['key_mask'], 0.1, 5)
    monkeypatch.setattr(ops, 'FLASH_ATTENTION', True)
    assert ops.masked_attention_path(L, c['DH']) == path
    taken = []
    for name, fn in list(ops._MASKED_ATTENTION_FNS.items()):
        monkeypatch.setitem(ops._MASKED_ATTENTION_FNS, name, type('Spy', (), {'apply': staticmethod(
            lambda *a, _n=name, _f=fn: (taken.append(_n), _f.apply(*a))[1])}))
    for mask in (inp['key_mask'].to(dev), inp['key_mask'].to(dev).to(torch.uint8) * 7):       # bool; uint8, any non-zero value
        x = inp['qkv'].to(dev).requires_grad_(True)
        o = ops.attention(x, c['H'], 0.1, 5, key_mask=mask)
        o.backward(inp['dout'].to(dev))
        assert torch.equal(o.detach(), want['o']) and torch.equal(x.grad, want['dqkv'])
    assert taken == [path, path]
    o0 = ops.attention(inp['qkv'].to(dev), c['H'], 0.1, 5)                                     # no mask: the functions as they were
    assert not torch.equal(o0, want['o']) and torch.equal(o0[:, 0], want['o'][:, 0])          # frame 0 has nothing masked
    with pytest.raises(ValueError):
        ops.attention(inp['qkv'].to(dev), c['H'], 0.0, 0, key_mask=inp['key_mask'][:2].to(dev))
    with pytest.raises(ValueError):
        ops.attention(inp['qkv'].to(dev), c['H'], 0.0, 0, key_mask=inp['key_mask'].to(dev).float())
    monkeypatch.setattr(ops, 'FLASH_ATTENTION', False)                                       # MUVO_FLASH_ATTN=0
    with pytest.raises(ValueError, match='MUVO_FLASH_ATTN'):
        ops.attention(inp['qkv'].to(dev), c['H'], 0.0, 0, key_mask=inp['key_mask'].to(dev))
