"""GPU: every kernel of the pooling / upsample / glue unit (muvo_amd/csrc/elementwise.hip, muvo_resize_bilinear_bwd of bev.hip)
against the float64 references of tests/elementwise_reference.py under the bars that module derives on the CPU, one case per
dispatch path and edge.  Each upsample / max-pool / softmax case is tied to the kernel it exists for: the route the library
reports (muvo_upsample3d_route / muvo_maxpool2d_route / muvo_softmax_dropout_route) must be the listed kernel and must equal the
Python mirror, and a case with a misaligned pointer is launched only after the reported kernel is known to make no 16-byte access
of that pointer.  Max pooling, the token transposes, the copies, the sums without transcendentals and the nearest resizes are
compared bit for bit.

The kernels are called through the C ABI on pointers into buffers this module owns: every output lies between two guard bands
of a marker value which are compared bit for bit afterwards, inputs and outputs can start 4 bytes off a 16-byte boundary, and an
absent operand (Pd at p = 0, eps, an upstream gradient) is a null pointer.  Every case runs twice and the two results must be
bit-identical (no kernel here uses atomics).  On failure the worst element is printed with the lane and workgroup that own it.

GPU-measured ELEMSTAT maxima are recorded next to the bars in elementwise_reference.py.  No case is left out."""
import ctypes as C

import pytest
import torch

import elementwise_reference as R

pytestmark = pytest.mark.gpu

U8_MARKER = 0xA5


class Buf:
    """n elements on the device between two guard bands; `off` extra elements in front shift the start off a 16-byte boundary"""

    def __init__(self, dev, n, dtype=torch.float32, off=0, init=None):
        self.n, self.start, self.dtype = n, R.GUARD + off, dtype
        self.marker = U8_MARKER if dtype == torch.uint8 else R.MARKER
        self.t = torch.full((self.start + n + R.GUARD,), self.marker, dtype=dtype, device=dev)
        self.ptr = self.t.data_ptr() + self.start * self.t.element_size()
        assert self.t.data_ptr() % 256 == 0
        if init is not None:
            self.set(init)

    def set(self, v):
        self.t[self.start:self.start + self.n] = v.reshape(-1).to(self.t.device)
        return self

    def fill(self):
        self.t.fill_(self.marker)
        return self

    @property
    def p(self):
        return C.c_void_p(self.ptr)

    def get(self, shape=None):
        """the payload on the CPU, after checking both guard bands bit for bit"""
        h = self.t.cpu()
        m = torch.full((1,), self.marker, dtype=self.dtype)
        assert torch.equal(h[:self.start], m.expand(self.start)), 'guard band in front of the output was written'
        assert torch.equal(h[self.start + self.n:], m.expand(R.GUARD)), 'guard band behind the output was written'
        v = h[self.start:self.start + self.n]
        return v.view(shape) if shape is not None else v


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _twice(launch, outs):
    """run `launch` twice into freshly marked outputs; the payloads (guards checked) of the first run, bit-identical to the second"""
    runs = []
    for _ in range(2):
        for o in outs:
            o.fill()
        launch()
        runs.append([o.get().clone() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), 'two runs differ'
    return runs[0]


def _check(label, kind, got, ref, den, where=None, stats=R.error_stats):
    bar = R.kernel_bar(kind)
    st = stats(got, ref, den)
    print(f'ELEMSTAT {kind} {label}: max e {st["max_e"]:.3e} rms {st["rms"]:.3e} share {R.excess(st, bar):.2f}')
    assert R.within(st, bar), (label, kind, st, bar, where(st['index']) if where else st['index'],
                               float(got[st['index']]), float(ref[st['index']]))


def _exact(label, kind, got, want):
    same = torch.equal(_bits(got), _bits(want))
    print(f'ELEMSTAT {kind} {label}: bit for bit {"equal" if same else "DIFFERENT"}')
    if not same:
        bad = (_bits(got) != _bits(want)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError((label, kind, f'{len(bad)} elements differ, first at {i}: got {got[i]}, expected {want[i]}'))


def _lib():
    from muvo_amd import ops
    return ops, ops.lib()


# ================================================================================================ upsample
def _upsample(c, backward, dev):
    ops, L = _lib()
    NC, D, H, W = c['NC'], c['D'], c['H'], c['W']
    v = R.up_inputs(c, backward)
    out_shape = (NC, D, H, W) if backward else (NC, 2 * D, 2 * H, 2 * W)
    n_out = NC * D * H * W * (1 if backward else 8)
    src = Buf(dev, v.numel(), off=0 if c['in16'] else 1, init=v)
    out = Buf(dev, n_out, off=0 if c['out16'] else 1)
    assert (src.ptr % 16 == 0) == c['in16'] and (out.ptr % 16 == 0) == c['out16']
    route = ops.upsample3d_route(backward, NC, D, H, W, src.ptr, out.ptr)
    assert route['kernel'] == c['kernel'], (c['name'], route)
    assert route == R.upsample_plan(backward, NC, D, H, W, c['in16'], c['out16']), (c['name'], route)
    need_in, need_out = R.UPSAMPLE_NEEDS16[(backward, route['kernel'])]
    assert (src.ptr % 16 == 0 or not need_in) and (out.ptr % 16 == 0 or not need_out), 'a 16-byte kernel on a misaligned pointer'
    fn = L.muvo_upsample3d_x2_bwd if backward else L.muvo_upsample3d_x2_fwd
    (got,) = _twice(lambda: ops._ck(fn(src.p, out.p, ops._i64(NC), D, H, W, ops._st())), [out])
    ref, den = R.ref_up_bwd(v) if backward else R.ref_up_fwd(v)
    _check(c['name'], f'up_{"bwd" if backward else "fwd"}_{c["kernel"]}', got.view(out_shape), ref, den,
           where=lambda i: R.up_owner(c['kernel'], backward, c, i, route))


@pytest.mark.parametrize('c', R.UP_FWD_CASES, ids=[c['name'] for c in R.UP_FWD_CASES])
def test_upsample_forward(c, dev):
    _upsample(c, 0, dev)


@pytest.mark.parametrize('c', R.UP_BWD_CASES, ids=[c['name'] for c in R.UP_BWD_CASES])
def test_upsample_backward(c, dev):
    _upsample(c, 1, dev)


# ================================================================================================ max pooling
@pytest.mark.parametrize('c', R.MAXPOOL_FWD_CASES, ids=[c['name'] for c in R.MAXPOOL_FWD_CASES])
def test_maxpool_forward(c, dev):
    ops, L = _lib()
    NC, H, W, k, s, p = (c[n] for n in ('NC', 'H', 'W', 'k', 's', 'p'))
    OH, OW = R.pool_out(H, k, s, p), R.pool_out(W, k, s, p)
    for fam in R.MAXPOOL_FAMILIES:
        x, _ = R.maxpool_inputs(c, fam)
        src = Buf(dev, x.numel(), off=0 if c['in16'] else 1, init=x)
        y, idx = Buf(dev, NC * OH * OW, off=0 if c['out16'] else 1), Buf(dev, NC * OH * OW, torch.uint8)
        route = ops.maxpool2d_route(0, NC, H, W, k, s, p, src.ptr, idx.ptr, y.ptr)
        assert R.maxpool_kind(route, 0) == c['kind'] and route == R.maxpool_plan(0, NC, H, W, k, s, p, c['in16'], True, c['out16'])
        assert src.ptr % 16 == 0 or not route['load16'], 'the 16-byte load path on a misaligned x'
        gy, gi = _twice(lambda: ops._ck(L.muvo_maxpool2d_fwd(src.p, y.p, idx.p, ops._i64(NC), H, W, OH, OW, k, s, p, ops._st())), [y, idx])
        ry, ri = R.ref_maxpool(x, k, s, p)
        _exact(f'{c["name"]} {fam} y', f'maxpool_fwd_{c["kind"]}', gy.view(NC, OH, OW), ry)
        _exact(f'{c["name"]} {fam} winner', f'maxpool_fwd_{c["kind"]}', gi.view(NC, OH, OW), ri)


@pytest.mark.parametrize('c', R.MAXPOOL_BWD_CASES, ids=[c['name'] for c in R.MAXPOOL_BWD_CASES])
def test_maxpool_backward(c, dev):
    ops, L = _lib()
    NC, H, W, k, s, p = (c[n] for n in ('NC', 'H', 'W', 'k', 's', 'p'))
    OH, OW = R.pool_out(H, k, s, p), R.pool_out(W, k, s, p)
    for fam in R.MAXPOOL_FAMILIES:
        x, dy = R.maxpool_inputs(c, fam)
        _, code = R.ref_maxpool(x, k, s, p)
        g = Buf(dev, dy.numel(), off=0 if c['in16'] else 1, init=dy)
        idx = Buf(dev, code.numel(), torch.uint8, init=code)
        dx = Buf(dev, NC * H * W, off=0 if c['out16'] else 1)
        route = ops.maxpool2d_route(1, NC, H, W, k, s, p, g.ptr, idx.ptr, dx.ptr)
        assert R.maxpool_kind(route, 1) == c['kind'] and route == R.maxpool_plan(1, NC, H, W, k, s, p, c['in16'], True, c['out16'])
        assert (g.ptr % 16 == 0 and dx.ptr % 16 == 0 and idx.ptr % 4 == 0) or not route['v8'], 'the eight-column kernel on a misaligned pointer'
        (got,) = _twice(lambda: ops._ck(L.muvo_maxpool2d_bwd(g.p, idx.p, dx.p, ops._i64(NC), H, W, OH, OW, k, s, p, ops._st())), [dx])
        _exact(f'{c["name"]} {fam} dx', f'maxpool_bwd_{c["kind"]}', got.view(NC, H, W), R.ref_maxpool_bwd(dy, code, H, W, k, s, p).float())


# ================================================================================================ average pooling
@pytest.mark.parametrize('G,S', R.AVGPOOL_CASES)
def test_avgpool(G, S, dev):
    ops, L = _lib()
    x = torch.randn(G, S, generator=R._gen('avgpool', G, S))
    src, y = Buf(dev, G * S, init=x), Buf(dev, G)
    (got,) = _twice(lambda: ops._ck(L.muvo_avgpool_fwd(src.p, y.p, ops._i64(G), ops._i64(S), ops._st())), [y])
    _check(f'{G}x{S}', 'avgpool_fwd', got, *R.ref_avgpool(x))
    dy = torch.randn(G, generator=R._gen('avgpool_bwd', G, S))
    g, dx = Buf(dev, G, init=dy), Buf(dev, G * S)
    (got,) = _twice(lambda: ops._ck(L.muvo_avgpool_bwd(g.p, dx.p, ops._i64(G), ops._i64(S), ops._st())), [dx])
    _exact(f'{G}x{S}', 'avgpool_bwd', got.view(G, S), R.emu_avgpool_bwd(dy, S))


# ================================================================================================ softmax + dropout
@pytest.mark.parametrize('rows,cols,p', R.SOFTMAX_CASES)
def test_softmax_dropout(rows, cols, p, dev):
    ops, L = _lib()
    seed, n = C.c_uint64(R.SOFTMAX_SEED), rows * cols
    assert ops.softmax_dropout_route(cols) == R.softmax_plan(cols)
    kind = f'maxv{R.softmax_plan(cols)["maxv"]}'
    S, dPd = R.softmax_inputs(rows, cols, p)
    # the library's own mask: muvo_dropout over ones, element index row * cols + c
    ones, mk = Buf(dev, n, init=torch.ones(n)), Buf(dev, n)
    ops._ck(L.muvo_dropout(ones.p, mk.p, ops._i64(n), ops._fl(p), seed, ops._st()))
    mask = mk.get((rows, cols)).clone()
    _exact(f'{rows}x{cols} p={p} mask', 'dropout', mask, R.host_dropout_mask(rows, cols, p, R.SOFTMAX_SEED))
    ref = R.ref_softmax(S, dPd, mask)
    label = f'{kind} {rows}x{cols} p={p}'
    src, P, Pd = Buf(dev, n, init=S), Buf(dev, n), Buf(dev, n)
    pd_ptr = Pd.p if p > 0 else C.c_void_p(0)                        # Pd absent at p = 0
    gP, gPd = _twice(lambda: ops._ck(L.muvo_softmax_dropout_fwd(src.p, P.p, pd_ptr, ops._i64(rows), cols, ops._fl(p), seed, ops._st())), [P, Pd])
    gP, gPd = gP.view(rows, cols), gPd.view(rows, cols)
    assert bool(torch.isfinite(gP).all())
    _check(label, 'softmax_P', gP, *ref['P'], stats=R.norm_stats)
    if p > 0:
        _check(label, 'softmax_Pd', gPd, *ref['Pd'], stats=R.norm_stats)
    else:
        assert bool((gPd == R.MARKER).all()), 'Pd written although absent'
    # backward on the kernel's own P
    Pin, g, dS = Buf(dev, n, init=gP), Buf(dev, n, init=dPd), Buf(dev, n)
    (gdS,) = _twice(lambda: ops._ck(L.muvo_softmax_dropout_bwd(Pin.p, g.p, dS.p, ops._i64(rows), cols, ops._fl(p), seed, ops._st())), [dS])
    _check(label, 'softmax_dS', gdS.view(rows, cols), *ref['dS'], stats=R.norm_stats)
    ops._ck(L.muvo_softmax_dropout_bwd(Pin.p, g.p, g.p, ops._i64(rows), cols, ops._fl(p), seed, ops._st()))     # in place, as AttentionFn runs it
    assert torch.equal(_bits(g.get()), _bits(gdS)), 'the in-place backward differs'
    # the same mask in both directions: with P = 1 / (2 cols) and dPd = 1 the backward returns a (g - s), s <= max(g) / 2, which is
    # positive exactly where the gradient passes and <= 0 where the mask cuts it
    Pc, one = Buf(dev, n, init=torch.full((n,), 0.5 / cols)), Buf(dev, n, init=torch.ones(n))
    ops._ck(L.muvo_softmax_dropout_bwd(Pc.p, one.p, dS.fill().p, ops._i64(rows), cols, ops._fl(p), seed, ops._st()))
    cut = dS.get((rows, cols)) <= 0
    assert torch.equal(cut, mask == 0), 'the backward cuts other elements than the mask'
    if p > 0:
        assert torch.equal(gPd == 0, cut | (gP == 0)), 'Pd is not zero exactly where the backward cuts the gradient'


# ================================================================================================ tokens
@pytest.mark.parametrize('C_,L,emb', R.TOKEN_CASES)
def test_token_transposes(C_, L, emb, dev):
    ops, Lb = _lib()
    N, L2 = 3, max(1, L - 1)                                       # second sensor block of another length at l0 = L
    g = R._gen('tokens', C_, L, emb)
    x1, x2 = torch.randn(N, C_, L, generator=g), torch.randn(N, C_, L2, generator=g)
    pos1, pos2, te = torch.randn(C_, L, generator=g), torch.randn(C_, L2, generator=g), torch.randn(C_, 2, generator=g)
    b = {k: Buf(dev, v.numel(), init=v) for k, v in (('x1', x1), ('x2', x2), ('pos1', pos1), ('pos2', pos2), ('te', te))}
    tok = Buf(dev, (L + L2) * N * C_)
    null = C.c_void_p(0)

    def fwd():
        ops._ck(Lb.muvo_nchw_to_tokens(b['x1'].p, b['pos1'].p if emb else null, b['te'].p if emb else null, 2, tok.p, N, C_, L, 0, ops._st()))
        ops._ck(Lb.muvo_nchw_to_tokens(b['x2'].p, b['pos2'].p if emb else null, C.c_void_p(b['te'].ptr + 4) if emb else null, 2, tok.p,
                                       N, C_, L2, L, ops._st()))
    (got,) = _twice(fwd, [tok])
    want = R.ref_tokens(x1, pos1 if emb else None, te[:, 0] if emb else None, torch.zeros(L + L2, N, C_), 0)
    want = R.ref_tokens(x2, pos2 if emb else None, te[:, 1] if emb else None, want, L)
    _exact(f'C{C_} L{L}+{L2} emb={int(emb)}', 'nchw_to_tokens', got.view(L + L2, N, C_), want)
    tin = Buf(dev, want.numel(), init=want)
    for l0, ll in ((0, L), (L, L2)):
        xo = Buf(dev, N * C_ * ll)
        (back,) = _twice(lambda: ops._ck(Lb.muvo_tokens_to_nchw(tin.p, xo.p, N, C_, ll, l0, ops._st())), [xo])
        _exact(f'C{C_} L{ll} l0={l0}', 'tokens_to_nchw', back.view(N, C_, ll), R.ref_untoken(want, N, C_, ll, l0))


# ================================================================================================ GRU / RSSM sample
@pytest.mark.parametrize('B,H,fam', R.GRU_CASES)
def test_gru_pointwise(B, H, fam, dev):
    ops, L = _lib()
    gi, gh, h, dhn = R.gru_inputs(B, H, fam)
    e64, den = R.gru_eval(gi, gh, h, dhn, torch.float64), R.gru_dens(gi, gh, h, dhn)
    bi, bh, bhh, bd = (Buf(dev, t.numel(), init=t) for t in (gi, gh, h, dhn))
    hn = Buf(dev, B * H)
    (got,) = _twice(lambda: ops._ck(L.muvo_gru_fwd(bi.p, bh.p, bhh.p, hn.p, B, H, ops._st())), [hn])
    label = f'{B}x{H} {fam}'
    _check(label + ' hn', 'gru_fwd', got.view(B, H), e64['hn'], den['hn'], stats=R.norm_stats)
    dgi, dgh, dh = Buf(dev, 3 * B * H), Buf(dev, 3 * B * H), Buf(dev, B * H)
    outs = _twice(lambda: ops._ck(L.muvo_gru_bwd(bi.p, bh.p, bhh.p, bd.p, dgi.p, dgh.p, dh.p, B, H, ops._st())), [dgi, dgh, dh])
    for name, got in zip(('dgi', 'dgh', 'dh'), outs):
        _check(f'{label} {name}', 'gru_bwd', got.view(B, -1), e64[name], den[name], stats=R.norm_stats)


@pytest.mark.parametrize('B,S,fam', R.SAMPLE_CASES)
def test_rssm_sample(B, S, fam, dev):
    ops, L = _lib()
    mls, eps_store, (dmu, dsigma, dsample) = R.sample_inputs(B, S, fam)
    ld = eps_store.shape[1]
    assert ld > S
    bm, be = Buf(dev, mls.numel(), init=mls), Buf(dev, eps_store.numel(), init=eps_store)
    grads = {k: Buf(dev, B * S, init=v) for k, v in (('dmu', dmu), ('dsigma', dsigma), ('dsample', dsample))}
    null = C.c_void_p(0)
    for absent in R.SAMPLE_ABSENT:
        kw = R.sample_args(eps_store[:, :S], dmu, dsigma, dsample, absent)
        e64 = R.sample_eval(mls, min_std=0.1, dtype=torch.float64, **kw)
        pe = null if absent == 'eps' else be.p
        mu, sigma, sample, dmls = Buf(dev, B * S), Buf(dev, B * S), Buf(dev, B * S), Buf(dev, 2 * B * S)
        gm, gs, gx = _twice(lambda: ops._ck(L.muvo_rssm_sample_fwd(bm.p, pe, ops._i64(ld), mu.p, sigma.p, sample.p, B, S, ops._fl(0.1), ops._st())),
                            [mu, sigma, sample])
        label = f'{B}x{S} {fam} absent={absent}'
        _exact(label + ' mu', 'sample_fwd', gm.view(B, S), mls[:, :S].contiguous())
        _check(label + ' sigma', 'sample_fwd', gs.view(B, S), e64['sigma'], e64['sigma'], stats=R.norm_stats)
        _check(label + ' sample', 'sample_fwd', gx.view(B, S), e64['sample'], e64['den_sample'], stats=R.norm_stats)
        ptrs = [null if absent == k else grads[k].p for k in ('dmu', 'dsigma', 'dsample')]
        (gd,) = _twice(lambda: ops._ck(L.muvo_rssm_sample_bwd(bm.p, pe, ops._i64(ld), *ptrs, dmls.p, B, S, ops._st())), [dmls])
        _check(label + ' dmls', 'sample_bwd', gd.view(B, 2 * S), e64['dmls'], e64['den_dmls'], stats=R.norm_stats)


# ================================================================================================ small glue operations
@pytest.mark.parametrize('accumulate', (0, 1))
def test_copy2d_axpby_batchsum(accumulate, dev):
    ops, L = _lib()
    g = R._gen('glue', accumulate)
    rows, cols, lds, ldd = 17, 23, 29, 31
    src, dst = torch.randn(rows * lds, generator=g), torch.randn(rows * ldd, generator=g)
    bs, bd = Buf(dev, src.numel(), init=src), Buf(dev, (rows - 1) * ldd + cols)       # dst ends with its last row: the guard follows at once
    launch = lambda: (bd.set(dst[:bd.n]), ops._ck(L.muvo_copy2d(bs.p, bd.p, ops._i64(rows), ops._i64(cols), ops._i64(lds), ops._i64(ldd),      # noqa: E731
                                                                accumulate, ops._st())))
    (got,) = _twice(launch, [bd])
    _exact(f'{rows}x{cols} ld {lds}->{ldd} acc={accumulate}', 'copy2d', got, R.ref_copy2d(src, dst[:bd.n], rows, cols, lds, ldd, accumulate))
    n = 777
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ba, bb, out = Buf(dev, n, init=a), Buf(dev, n, init=b), Buf(dev, n)
    pb = bb.p if accumulate else C.c_void_p(0)                    # b absent
    (got,) = _twice(lambda: ops._ck(L.muvo_axpby(ba.p, pb, out.p, ops._i64(n), ops._fl(0.3), ops._fl(-1.7), ops._st())), [out])
    _exact(f'{n} b={"present" if accumulate else "absent"}', 'axpby', got, R.ref_axpby(a, b if accumulate else None, 0.3, -1.7))
    N, inner = 7, 301
    x, prior = torch.randn(N, inner, generator=g), torch.randn(inner, generator=g)
    bx, bo = Buf(dev, x.numel(), init=x), Buf(dev, inner)
    (got,) = _twice(lambda: (bo.set(prior), ops._ck(L.muvo_batchsum(bx.p, bo.p, N, ops._i64(inner), accumulate, ops._st()))), [bo])
    _exact(f'{N}x{inner} acc={accumulate}', 'batchsum', got, R.ref_batchsum(x, prior, accumulate))


@pytest.mark.parametrize('act', range(6), ids=R.ACT_NAMES)
def test_act_fwd(act, dev):
    ops, L = _lib()
    v = R.act_inputs()
    src, out = Buf(dev, v.numel(), init=v), Buf(dev, v.numel())
    (got,) = _twice(lambda: ops._ck(L.muvo_act_fwd(src.p, out.p, ops._i64(v.numel()), act, ops._fl(R.SLOPE), ops._st())), [out])
    if act in R.ACT_EXACT:
        _exact(R.ACT_NAMES[act], 'act_fwd', got, R.act32(v, act))
    else:
        _check(R.ACT_NAMES[act], 'act_fwd', got, *R.ref_act(v, act), stats=R.norm_stats)


# ================================================================================================ resizes
@pytest.mark.parametrize('in_hw,out_hw', R.BILINEAR_CASES)
def test_resize_bilinear_and_adjoint(in_hw, out_hw, dev):
    ops, L = _lib()
    (h, w), (oh, ow), NC = in_hw, out_hw, 3
    x, g = R.bilinear_inputs(h, w, oh, ow, NC)
    bx, by = Buf(dev, x.numel(), init=x), Buf(dev, NC * oh * ow)
    (got,) = _twice(lambda: ops._ck(L.muvo_resize_bilinear(bx.p, by.p, ops._i64(NC), h, w, oh, ow, ops._st())), [by])
    _check(f'{h}x{w}->{oh}x{ow}', 'resize_bilinear', got.view(NC, oh, ow), *R.ref_bilinear(x, oh, ow))
    bg, bdx = Buf(dev, g.numel(), init=g), Buf(dev, NC * h * w)
    (got,) = _twice(lambda: ops._ck(L.muvo_resize_bilinear_bwd(bg.p, bdx.p, ops._i64(NC), h, w, oh, ow, ops._st())), [bdx])
    _check(f'{h}x{w}<-{oh}x{ow}', 'resize_bilinear_bwd', got.view(NC, h, w), *R.ref_bilinear_bwd(g, h, w))


@pytest.mark.parametrize('in_sz,out_sz', R.NEAREST_CASES)
def test_resize_nearest(in_sz, out_sz, dev):
    ops, L = _lib()
    NC = 2
    i3, o3 = (1,) * (3 - len(in_sz)) + tuple(in_sz), (1,) * (3 - len(out_sz)) + tuple(out_sz)
    g = R._gen('nearest', in_sz, out_sz)
    n_out = NC * o3[0] * o3[1] * o3[2]
    for dtype, fn in ((torch.float32, L.muvo_resize_nearest_f32), (torch.uint8, L.muvo_resize_nearest_u8)):
        x = torch.randn(NC, *in_sz, generator=g) if dtype == torch.float32 else torch.randint(0, 256, (NC, *in_sz), generator=g, dtype=torch.uint8)
        bx, by = Buf(dev, x.numel(), dtype, init=x), Buf(dev, n_out, dtype)
        (got,) = _twice(lambda: ops._ck(fn(bx.p, by.p, ops._i64(NC), *i3, *o3, ops._st())), [by])
        _exact(f'{in_sz}->{out_sz} {str(dtype)[6:]}', 'resize_nearest', got.view(NC, *out_sz), R.ref_nearest(x, out_sz))
