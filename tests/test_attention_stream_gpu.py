"""GPU: the fused attention kernels (muvo_amd/csrc/attention.hip), streamed through ops.StreamAttentionFn and resident (K / V of a
head whole in LDS, L <= 384) through ops.FlashAttentionFn, against the float64 reference of tests/attention_reference.py under its
bar (4 x the float32 CPU evaluation of the same recurrence on the same inputs; tests/test_attention_reference.py shows that bar
rejects planted errors).  Streamed: lengths at every edge of the block sizes the library reports, spiked inputs that force the
rescale, dropout against the unfused path and against float64 with the library's own mask, reproducibility, memory (nothing
L x L), and inside the transformer encoder.  Resident: one key, the edges of a key tile, of a workgroup's 128 queries and of the
register tiles, the model's L, every head size, the largest L of DH = 64, and dropout the same two ways."""
import ctypes as C

import pytest
import torch

import attention_reference as R

pytestmark = pytest.mark.gpu


def _close(a, b, rtol=2e-4, atol=2e-5, name=''):          # tests/test_kernels_gpu.py::_close
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, f'{name}: shape {tuple(a.shape)} vs {tuple(b.shape)}'
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol + rtol * ref * 0.1), f'{name}: max err {err:.3e} (ref max {ref:.3e})'


def _run(fn, qkv, dout, heads, p=0.0, seed=0):
    x = qkv.clone().requires_grad_(True)
    o = fn(x, heads, p, seed)
    o.backward(dout)
    return o.detach(), x.grad


def _kernels(path, c, inp, dev, p=0.0, seed=0):
    """{o, lse, dqkv} of one path's kernels ('stream' | 'fused') on a case's inputs (lse from the library call itself)"""
    from muvo_amd import ops
    fwd = {'stream': ops.lib().muvo_attention_stream_fwd, 'fused': ops.lib().muvo_attention_fwd}[path]
    qkv, dout = inp['qkv'].to(dev), inp['dout'].to(dev)
    o, dqkv = _run(ops._ATTENTION_FNS[path].apply, qkv, dout, c['H'], p, seed)
    o2, lse = torch.empty_like(o), torch.empty(c['N'] * c['H'], c['L'], device=dev)
    ops._ck(fwd(ops._f(qkv), ops._f(o2), ops._f(lse), c['L'], c['N'], c['H'], c['DH'], ops._fl(p), C.c_uint64(seed), ops._st()))
    assert torch.equal(o, o2)
    return {'o': o, 'lse': lse, 'dqkv': dqkv}


def _stream(c, inp, dev, p=0.0, seed=0):
    return _kernels('stream', c, inp, dev, p, seed)


def _resident(c, inp, dev, p=0.0, seed=0):
    from muvo_amd import ops
    assert c['res'] and ops.lib().muvo_attention_supported(c['L'], c['DH']) == 1
    return _kernels('fused', c, inp, dev, p, seed)


def _check(c, got, ref, tag=''):
    cmp = R.compare(R.case_id(c), got, ref)
    print('\n'.join(R.statlines(R.case_id(c) + tag, cmp)))
    bad = R.failures(cmp)
    assert not bad, bad


def test_block_sizes(dev):
    from muvo_amd import ops
    bq, bk = C.c_int(0), C.c_int(0)
    assert ops.lib().muvo_attention_stream_blocks(C.byref(bq), C.byref(bk)) == 0
    assert (bq.value, bk.value) == (R.BQ, R.BK)


@pytest.mark.parametrize('c', R.PARITY_CASES + [R.BIG_CASE], ids=R.case_id)
def test_float64_parity(dev, c):
    inp, ref = R.reference(c)
    _check(c, _stream(c, inp, dev), ref)
    if c is R.BIG_CASE:
        R._reference_cached.cache_clear()


@pytest.mark.parametrize('c', R.SPIKED_CASES, ids=R.case_id)
def test_forced_rescale(dev, c):
    inp, ref = R.reference(c)
    R.spiked_facts(c, inp['qkv'])
    got = _stream(c, inp, dev)
    for n in R.NAMES:
        assert torch.isfinite(got[n]).all(), n
    _check(c, got, ref)


@pytest.mark.parametrize('c', R.DROPOUT_CASES, ids=R.case_id)
def test_dropout(dev, c):
    from muvo_amd import ops
    p, seed = c['p'], R.DROPOUT_SEEDS[c['p']]
    inp = R.inputs(c)
    qkv, dout = inp['qkv'].to(dev), inp['dout'].to(dev)
    got = _stream(c, inp, dev, p, seed)
    ou, du = _run(ops.AttentionFn.apply, qkv, dout, c['H'], p, seed)
    _close(got['o'], ou, rtol=2e-5, name=f'stream vs unfused fwd p={p}')
    _close(got['dqkv'], du, rtol=1e-4, name=f'stream vs unfused dqkv p={p}')
    # the library's own mask: its dropout over ones, same seed, same index convention ((n*H + h)*L + query)*L + key
    keep = ops.dropout(torch.ones(c['N'], c['H'], c['L'], c['L'], device=dev), p, seed).cpu()
    assert abs(float((keep > 0).float().mean()) - (1 - p)) < 5e-3
    ref = R.reference64(inp['qkv'], c['H'], inp['dout'], keep)
    _check(c, got, ref, ' library mask')
    o0, _ = _run(ops.StreamAttentionFn.apply, qkv, dout, c['H'])
    assert not torch.allclose(got['o'], o0)                 # the mask does something


def test_reproducible(dev):
    from muvo_amd import ops
    c = R.PARITY_CASES[7]
    inp = R.inputs(c)
    qkv, dout = inp['qkv'].to(dev), inp['dout'].to(dev)
    for p, seed in ((0.0, 0), (0.1, 77)):
        a, b = (_run(ops.StreamAttentionFn.apply, qkv, dout, c['H'], p, seed) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_nothing_l_by_l_in_memory(dev):
    """A condition, not a measurement: forward + backward at L = 2048 may allocate 4 x the bytes of qkv (o, dqkv, a contiguous
    dout, lse, D, allocator rounding); one L x L float tensor would be 14 x."""
    from muvo_amd import ops
    l, n, h, dh = 2048, 2, 8, 48
    g = torch.Generator().manual_seed(2048)
    qkv = torch.randn(l, n, 3 * h * dh, generator=g).to(dev).requires_grad_(True)
    dout = torch.randn(l, n, h * dh, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    o = ops.StreamAttentionFn.apply(qkv, h, 0.1, 5)
    o.backward(dout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    budget = 4 * qkv.numel() * 4
    print(f'ATTNSTAT memory: rise {rise / 1e6:.1f} MB, budget {budget / 1e6:.1f} MB, one L x L tensor {n * h * l * l * 4 / 1e6:.0f} MB')
    assert rise <= budget
    assert torch.isfinite(qkv.grad).all()


MASK_CAP, MASK_BAND = 1e-4, 1e-5          # tests/norm_reference.py: the same rule for ReLU masks, the same two constants


def test_encoder_stream_vs_unfused(dev, monkeypatch):
    """hnn.TransformerEncoder(384, 8, 2 layers, dropout 0.1) on (517, 2, 384): output, input gradient and every parameter gradient
    with the streamed attention kernels against the unfused path, at the bars of test_transformer_layer.

    The encoder has a ReLU (2 layers x 1034 tokens x 2048 units) behind the attention, and the two attention paths differ in
    the last bits, so a pre-activation that rounds to either side of zero gets another mask in each run: measured on six seeds,
    three had one or two such units, every one with |pre-activation| <= 1.2e-7, and ONE flipped unit moved dx by 5e-3 .. 1.2e-2
    (8 .. 22 x the bar; its own gradient times a row of linear1.weight), while with the mask shared dx agreed to 1.4e-6 (0.002 x
    the bar) on all six.  That is the comparison's discontinuity, not an error of either path, and the suite has a rule for it
    (tests/norm_reference.py, 'ReLU masks are the subject's'): the stream run is the encoder as it stands; the unfused
    reference run applies the ReLU mask read off the stream run's own FFN activations, and the masks may disagree on at most
    MASK_CAP of the units, only where |pre-activation| <= MASK_BAND x max |pre-activation| - an attention error large enough to
    move a mask anywhere else fails here."""
    from muvo_amd import nn as hnn, ops
    torch.manual_seed(11)
    with torch.device(dev):
        enc = hnn.TransformerEncoder(384, 8, num_layers=2, dropout=0.1)
    x = torch.randn(517, 2, 384, device=dev)
    g = torch.randn(517, 2, 384, device=dev)
    linear = ops.linear
    masks, facts = [], []

    def subject_linear(x, weight, bias=None, act=ops.ACT_NONE, slope=0.0):
        y = linear(x, weight, bias, act, slope)            # unchanged; only looked at
        if act == ops.ACT_RELU:
            masks.append(y.detach() > 0)
        return y

    def reference_linear(x, weight, bias=None, act=ops.ACT_NONE, slope=0.0):
        if act != ops.ACT_RELU:
            return linear(x, weight, bias, act, slope)
        pre = linear(x, weight, bias)
        m = masks[len(facts)]
        dis = m != (pre.detach() > 0)
        n = int(dis.sum())
        facts.append((n / m.numel(), float(pre.detach()[dis].abs().max()) / float(pre.detach().abs().max()) if n else 0.0))
        return pre * m.float()

    def run(flash, fn):
        monkeypatch.setattr(ops, 'FLASH_ATTENTION', flash)
        monkeypatch.setattr(ops, 'linear', fn)
        assert ops.attention_path(517, 48) == ('stream' if flash else 'unfused')
        xg = x.clone().requires_grad_(True)
        for p in enc.parameters():
            p.grad = torch.zeros_like(p)
        y = enc(xg, seed=3)
        y.backward(g)
        torch.cuda.synchronize()
        return y.detach(), xg.grad, {k: p.grad.clone() for k, p in enc.named_parameters()}

    ys, dxs, gs = run(True, subject_linear)
    yu, dxu, gu = run(False, reference_linear)
    print(f'ATTNSTAT encoder ReLU masks (fraction that differs, largest |pre| there / max |pre|) per layer: {facts}')
    assert len(masks) == len(facts) == 2
    for frac, band in facts:
        assert frac <= MASK_CAP and band <= MASK_BAND, facts
    _close(ys, yu, rtol=5e-4, name='encoder fwd')
    _close(dxs, dxu, rtol=1e-3, name='encoder dx')
    for k in gs:
        _close(gs[k], gu[k], rtol=1e-3, atol=1e-4, name=f'encoder grad {k}')


# ------------------------------------------------------------------------------------------------ resident kernels (L <= 384)
def test_resident_range(dev):
    from muvo_amd import ops
    L = ops.lib()
    assert L.muvo_attention_supported(R.RES_MAXL_D64, 64) == 1 and L.muvo_attention_supported(R.RES_MAXL_D64 + 1, 64) == 0
    assert L.muvo_attention_supported(R.RES_MAXL, 48) == 1 and L.muvo_attention_supported(R.RES_MAXL + 1, 48) == 0


@pytest.mark.parametrize('c', R.RESIDENT_CASES, ids=R.case_id)
def test_resident_float64_parity(dev, c):
    inp, ref = R.reference(c)
    _check(c, _resident(c, inp, dev), ref)


@pytest.mark.parametrize('c', R.RESIDENT_DROPOUT_CASES, ids=R.case_id)
def test_resident_dropout(dev, c):
    """test_dropout on the resident path"""
    from muvo_amd import ops
    p, seed = c['p'], R.DROPOUT_SEEDS[c['p']]
    inp = R.inputs(c)
    qkv, dout = inp['qkv'].to(dev), inp['dout'].to(dev)
    got = _resident(c, inp, dev, p, seed)
    ou, du = _run(ops.AttentionFn.apply, qkv, dout, c['H'], p, seed)
    _close(got['o'], ou, rtol=2e-5, name=f'resident vs unfused fwd p={p}')
    _close(got['dqkv'], du, rtol=1e-4, name=f'resident vs unfused dqkv p={p}')
    keep = ops.dropout(torch.ones(c['N'], c['H'], c['L'], c['L'], device=dev), p, seed).cpu()
    assert abs(float((keep > 0).float().mean()) - (1 - p)) < 5e-3
    ref = R.reference64(inp['qkv'], c['H'], inp['dout'], keep)
    _check(c, got, ref, ' library mask')
    o0, _ = _run(ops.FlashAttentionFn.apply, qkv, dout, c['H'])
    assert not torch.allclose(got['o'], o0)                 # the mask does something
