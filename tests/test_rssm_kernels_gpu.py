"""-m gpu: the two persistent RSSM kernels (muvo_amd/csrc/rssm.hip) through the C ABI (ctypes) against the float64 references of
tests/rssm_reference.py: every stage of every step under its one-stage bar from the kernel's own stored inputs of that stage, what
the kernels copy bit for bit, the outputs / d_emb / parameter gradients end to end, NaN poison and canaries around every buffer,
bit-reproducibility, the grid-barrier words, small grids (MUVO_RSSM_GRID, in child processes), NULL upstream gradients, mask
bits nobody reads, and muvo_rssm_supported / the argument errors at the dynamic-LDS limit.  The bars are those the CPU test
(tests/test_rssm_reference.py) proves to pass the emulated arithmetic and to reject the planted faults; none comes from a GPU.
On failure the worst element is printed with its stage, step, sequence and row.  Nothing here makes a barrier time out.

GPU-measured RSSMSTAT maxima are recorded next to the bars in rssm_reference.py.  No case is left out."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import rssm_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@functools.lru_cache(maxsize=None)
def _run(dev, name, mask_name, pattern):
    """one forward + backward of a case through the C ABI, shared by the tests below (results are not modified)"""
    c, inp = R.CASE[name], R.inputs(name)
    return R.gpu_run(dev, c, inp, R.mask_value(mask_name, c['T']), R.upstreams(inp, pattern))


def _healthy(dev, c, res, info, label):
    """what holds after every run in this file: no error word, the barrier counter at 4 T G of the last slab with the default G of
    one workgroup per CU, canaries intact, no NaN left in any result"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    want = int(os.environ.get('MUVO_RSSM_GRID', '0') or 0)
    want = want if want > 0 else cus
    assert info['err'] == 0, f'{label}: barrier error word {info["err"]}'
    assert info['G_fwd'] == want and info['G_bwd'] in (None, want), (label, info, want)
    assert not info['broken'], f'{label}: guard words or the row past B T changed in {info["broken"]}'
    for n in R.OUT7 + R.KEEP12 + (R.GRAD10 if info['G_bwd'] is not None else ()):
        assert not torch.isnan(res[n]).any(), f'{label}: NaN poison left in {n}'


# ================================================================================================ 1, 3, 6: per-stage parity
@pytest.mark.parametrize('name,mask,pattern', R.runs(), ids=['-'.join(r) for r in R.runs()])
def test_stages(dev, name, mask, pattern):
    """every kept tensor, output and kept gradient of every step under its one-stage bar; copies bit for bit; poison and canaries;
    the NULL-upstream patterns (with all seven NULL every gradient is exactly 0)"""
    c, inp = R.CASE[name], R.inputs(name)
    label = f'{name} {mask} {pattern}'
    res, info = _run(dev, name, mask, pattern)
    _healthy(dev, c, res, info, label)
    fails, rows = R.judge(c, inp, R.mask_value(mask, c['T']), R.upstreams(inp, pattern), res, label, emit=print)
    assert not fails, '\n'.join(fails)
    if pattern == 'none':
        for n in R.GRAD10:
            assert not res[n].any(), f'{n} is not exactly 0 without upstream gradients'


# ================================================================================================ 2: end to end
def _module(dev, c, inp):
    from muvo_amd.models.transition import RSSM
    H, S, E, A = c['dims']
    with torch.device(dev):
        m = RSSM(embedding_dim=E, action_dim=c['AD'], hidden_state_dim=H, state_dim=S, action_latent_dim=A, receptive_field=c['T'])
    m.load_state_dict({mn: inp.W[wn].to(dev) for mn, wn in zip(R.MODULE_NAMES, R.WNAMES)})
    m.train()
    return m


def _module_run(dev, c, inp, mask, frozen=()):
    """forward + backward through the model (ops.rssm_fused -> ops.RSSMFusedFn) with all seven upstreams.  Returns
    (outputs, d_emb, {weight name: .grad}, out dict)."""
    from muvo_amd import ops
    m = _module(dev, c, inp)
    named = dict(m.named_parameters())
    par = {wn: named[mn] for mn, wn in zip(R.MODULE_NAMES, R.WNAMES)}
    for wn, p in par.items():
        p.requires_grad_(wn not in frozen)
        p.grad = torch.full_like(p, R.MARKER) if wn in frozen else None
    e = inp.emb.to(dev).requires_grad_(True)
    H, S, E, A = c['dims']
    assert ops.rssm_fused_supported(c['B'], c['T'], H, S, E, A, c['AD'])
    out = m(e, inp.act.to(dev), noise=inp.noise.to(dev), use_prior=[bool((mask >> t) & 1) for t in range(c['T'])])
    outs = {'h': out['prior']['hidden_state'], 'mu_p': out['prior']['mu'], 'sg_p': out['prior']['sigma'], 'z_p': out['prior']['sample'],
            'mu_q': out['posterior']['mu'], 'sg_q': out['posterior']['sigma'], 'z_q': out['posterior']['sample']}
    sum((outs[o] * inp.ups[g].to(dev)).sum() for o, g in zip(R.OUT7, R.UP7)).backward()
    torch.cuda.synchronize()
    words = ops.rssm_barrier_words(dev).cpu().tolist()          # the wrapper's own barrier words, after its backward launch
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert words[1] == 0 and words[0] == 4 * c['T'] * cus, words
    return {k: v.detach().cpu() for k, v in outs.items()}, e.grad.cpu(), {wn: p.grad.cpu() for wn, p in par.items()}, out


@pytest.mark.parametrize('name', list(R.CASE))
def test_end_to_end(dev, name):
    """outputs and d_emb of the C ABI run, and the 18 parameter gradients formed by ops.RSSMFusedFn, against the float64 reference
    of the whole recurrence under 4 x the float32 emulation's error; the model's run gives the C ABI run's bits"""
    c, inp = R.CASE[name], R.inputs(name)
    mask_name = c['masks'][0]
    mask = R.mask_value(mask_name, c['T'])
    res, info = _run(dev, name, mask_name, 'all')
    outs, d_emb, grads, out = _module_run(dev, c, inp, mask)
    assert out['prior']['hidden_state'] is out['posterior']['hidden_state'], 'the hidden state is one tensor for both dicts'
    for n in R.OUT7:
        assert torch.equal(outs[n].view(torch.int32), res[n].view(torch.int32)), f'{n}: the model and the C ABI run differ'
    assert torch.equal(d_emb.view(torch.int32), res['d_emb'].view(torch.int32))
    got = dict({n: res[n] for n in R.OUT7 + ('d_emb',)}, **grads)
    errs = R.e2e_errors(R.e2e_reference(name), got)
    bad = []
    for n, e in errs.items():
        bar = R.e2e_bar(name, n)
        print(f'RSSMSTAT {name} end-to-end {n}: e {e:.3e} share {e / bar if bar else 0.0:.2f}')
        if e > bar:
            bad.append((n, e, bar))
    assert not bad, bad


@pytest.mark.parametrize('name', R.FAMILY_CASES)
def test_frozen_parameters(dev, name):
    """some parameters with requires_grad = False: their .grad is untouched, the others' are the unfrozen run's bits"""
    c, inp = R.CASE[name], R.inputs(name)
    mask = R.mask_value(c['masks'][0], c['T'])
    frozen = ('b_pre', 'w_ih', 'b_pa', 'w_qa', 'w_q2', 'b_q0')
    _, d_emb, full, _ = _module_run(dev, c, inp, mask)
    _, d_emb_f, part, _ = _module_run(dev, c, inp, mask, frozen)
    assert torch.equal(d_emb.view(torch.int32), d_emb_f.view(torch.int32))
    for wn in R.WNAMES:
        if wn in frozen:
            assert torch.equal(part[wn].view(torch.int32), torch.full_like(part[wn], R.MARKER).view(torch.int32)), f'{wn}: frozen, but .grad changed'
        else:
            assert torch.equal(part[wn].view(torch.int32), full[wn].view(torch.int32)), f'{wn}: differs from the unfrozen run'


# ================================================================================================ 4: reproducible
@pytest.mark.parametrize('name', ['tiny-b3-t5', 'tiny-b1-t64', 'pass2-b8-t2', 'lds-limit-b4-t1'])
def test_two_runs_are_bit_identical(dev, name):
    c, inp = R.CASE[name], R.inputs(name)
    m = c['masks'][0]
    a, ia = _run(dev, name, m, 'all')
    b, ib = R.gpu_run(dev, c, inp, R.mask_value(m, c['T']), R.upstreams(inp, 'all'))
    _healthy(dev, c, b, ib, name)
    assert (ia['G_fwd'], ia['G_bwd']) == (ib['G_fwd'], ib['G_bwd'])
    for n in R.OUT7 + R.KEEP12 + R.GRAD10:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n


# ================================================================================================ 6: mask bits nobody reads
@pytest.mark.parametrize('name', ['tiny-b3-t5', 'tiny-b1-t64', 'tiny-b64-t1'])
def test_mask_bits_nobody_reads(dev, name):
    """a mask that differs only in bits >= T - 1 gives the same bits"""
    c, inp = R.CASE[name], R.inputs(name)
    m = R.mask_value(c['masks'][0], c['T'])
    ups = R.upstreams(inp, 'all')
    a, ia = R.gpu_run(dev, c, inp, m & ~R.irrelevant_bits(c['T']), ups)
    b, ib = R.gpu_run(dev, c, inp, m | R.irrelevant_bits(c['T']), ups)
    _healthy(dev, c, a, ia, name)
    _healthy(dev, c, b, ib, name)
    for n in R.OUT7 + R.KEEP12 + R.GRAD10:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n


# ================================================================================================ 5: small grids
CHILD = """
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import rssm_reference as R
dev = torch.device('cuda:0')
out = {{}}
for name in R.GRID_CASES:
    c, inp = R.CASE[name], R.inputs(name)
    m = c['masks'][0]
    res, info = R.gpu_run(dev, c, inp, R.mask_value(m, c['T']), R.upstreams(inp, 'all'))
    out[name] = dict(info=info, crc=R.crcs(res))
print('RSSMGRID ' + json.dumps(out))
"""


def test_small_grids(dev):
    """MUVO_RSSM_GRID = 1 and 3 (read once per process: one child each, one after the other): G from the barrier word is the
    requested grid and every result tensor has the bits of the default-grid run.  The dot products do not depend on the grid, so
    a difference is a stride-loop, ownership or visibility bug."""
    base = {}
    for name in R.GRID_CASES:
        res, info = _run(dev, name, R.CASE[name]['masks'][0], 'all')
        _healthy(dev, R.CASE[name], res, info, name)
        base[name] = R.crcs(res)
    code = CHILD.format(root=ROOT, tests=os.path.dirname(os.path.abspath(__file__)))
    for grid in (1, 3):
        env = dict(os.environ, MUVO_RSSM_GRID=str(grid))
        r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, f'grid {grid}: child ended with {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-2000:]}'
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RSSMGRID ')]
        assert line, r.stdout[-1000:]
        got = json.loads(line[-1][len('RSSMGRID '):])
        for name in R.GRID_CASES:
            info = got[name]['info']
            print(f'RSSMSTAT {name} grid {grid}: G forward {info["G_fwd"]} backward {info["G_bwd"]}')
            assert info['err'] == 0 and not info['broken'], (grid, name, info)
            assert info['G_fwd'] == grid and info['G_bwd'] == grid, (grid, name, info)
            diff = [n for n, v in base[name].items() if got[name]['crc'][n] != v]
            assert not diff, f'grid {grid}, {name}: {diff} differ from the default-grid run'


# ================================================================================================ the limit and the argument errors
def test_supported_and_argument_errors(dev):
    """muvo_rssm_supported agrees with the mirror at every case, at the limit and at each point past it or outside a condition;
    there muvo_rssm_forward returns the argument error and launches nothing (the barrier word keeps its sentinel)"""
    from muvo_amd import ops
    L = ops.lib()
    for c in R.CASES:
        H, S, E, A = c['dims']
        assert L.muvo_rssm_supported(c['B'], c['T'], H, S, E, A, c['AD']) == 1 == R.supported(c['B'], c['T'], H, S, E, A, c['AD'])
        assert L.muvo_rssm_transposed_floats(H, S, E, A) == R.transposed_floats(H, S, E, A)
        assert L.muvo_rssm_scratch_floats(c['B'], H, S, E, A) == R.scratch_floats(c['B'], H, S, E, A)
    dummy = torch.zeros(64, device=dev)
    bar = torch.full((4,), 77, device=dev, dtype=torch.int32)
    order = ('B', 'T', 'H', 'S', 'E', 'A', 'AD')
    tab = lambda n: ops._ptr_table([dummy] * n)          # noqa: E731
    assert L.muvo_rssm_supported(*[R.LIMIT_FWD[k] for k in order]) == 1 == R.supported(**R.LIMIT_FWD)
    for kw in R.PAST_FWD:
        p = dict(R.LIMIT_FWD, **kw)
        args = [p[k] for k in order]
        assert L.muvo_rssm_supported(*args) == 0 == R.supported(**p), kw
        rc = L.muvo_rssm_forward(*args, tab(18), ops._f(dummy), ops._f(dummy), ops._f(dummy), C.c_uint64(0), tab(7), tab(12),
                                 ops._p(bar), ops._fl(R.MIN_STD), ops._st())
        assert rc == -1, (kw, rc, L.muvo_last_error().decode())          # MUVO_ERR_INVALID_ARG
    for kw in R.PAST_BWD:
        p = dict(R.LIMIT_BWD, **kw)
        args = [p[k] for k in order]
        assert L.muvo_rssm_supported(*args) == 0 == R.supported(**p), kw
        rc = L.muvo_rssm_backward(*args, tab(18), ops._f(dummy), ops._f(dummy), C.c_uint64(0), tab(5), tab(7), tab(10), ops._f(dummy),
                                  ops._p(bar), ops._st())
        assert rc == -1, (kw, rc, L.muvo_last_error().decode())
    torch.cuda.synchronize()
    assert bar.cpu().tolist() == [77] * 4 and not dummy.any(), 'an argument error launched something'
