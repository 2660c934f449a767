"""-m gpu: the Lovasz-softmax training loss of the voxel head (muvo_amd/csrc/lovasz.hip through ops.voxel_lovasz_loss,
ops.voxel_lovasz_parts, losses.LovaszSoftmaxLoss and WorldModelTrainer.compute_loss) against the float64 restatement of
tests/lovasz_reference.py with its normalised error and bars (4 x the error of the float32 CPU evaluation of the same
restatement; tests/test_lovasz_reference.py shows on the CPU that these bars reject planted errors).  The errors and the loss
are judged against float64 as it stands; dlde, `present` and the gradient against float64 on the ranking of the errors the
device returned (lovasz64(order_from=...)): together with the tie cases that pins the ranking itself - a misplaced key changes
an integer count.  No case and no voxel is excluded.  Each case prints `LOSSSTAT <id> <name>: max_e rms (bar)` lines."""
import pytest
import torch

import lovasz_reference as R
import loss_reference as LR

pytestmark = pytest.mark.gpu
GUARD = {torch.float32: 12345.0, torch.uint8: 77}


def _judge(tag, cmp):
    for line in R.statlines(tag, cmp):
        print(line)
    bad = R.failures(cmp)
    assert not bad, f'{tag}: ' + '; '.join(f'{n} max_e {s["max_e"]:.3e} at {s["index"]} (bar {cmp[n][1]:.2e})' for n, s in bad.items())


def _place(t, dev, off, grad=False):
    """`t` on the device inside a fresh buffer of guard values, `off` elements after four guard elements (as _place of
    tests/test_chamfer_loss_gpu.py, for float32 and uint8); returns (buffer, contiguous view of t's shape)"""
    n = t.numel()
    buf = torch.full((n + 12,), GUARD[t.dtype], dtype=t.dtype, device=dev)
    buf[4 + off:4 + off + n] = t.reshape(-1).to(dev)
    if grad:
        buf.requires_grad_(True)
    return buf, buf[4 + off:4 + off + n].view(t.shape)


def _six(logits, labels):
    F, C, V = logits.shape
    return logits.view(1, F, C, V, 1, 1), labels.view(1, F, 1, V, 1, 1)


def _run(dev, logits, labels, weight=R.WEIGHT, gout=R.GOUT, offsets=(0, 0), parts=True):
    """ops.voxel_lovasz_loss forward + backward (and ops.voxel_lovasz_parts) on (F, C, V) / (F, V) CPU tensors placed at element
    offsets; checks that nothing outside the views was written"""
    from muvo_amd import ops
    F, C, V = logits.shape
    l6, t6 = _six(logits, labels)
    lo, to = offsets
    lbuf, lg = _place(l6, dev, lo, grad=True)
    tbuf, tg = _place(t6, dev, to)
    out = ops.voxel_lovasz_loss(lg, tg, weight)
    assert out.shape == (1,)
    (gout * out[0]).backward()
    grad = lbuf.grad
    assert not grad[:4 + lo].any() and not grad[4 + lo + logits.numel():].any(), 'gradient written outside the view'
    got = {'loss': out[0].detach().cpu(), 'dlogits': grad[4 + lo:4 + lo + logits.numel()].view(F, C, V).cpu()}
    if parts:
        errors, dlde, present, lfc = ops.voxel_lovasz_parts(lg, tg)
        assert errors.shape == (F, C, V) and dlde.shape == (F, C, V) and present.shape == (F, C) and lfc.shape == (F, C)
        got.update(errors=errors.cpu(), dlde=dlde.cpu(), present=present.cpu().bool(), frame_class_loss=lfc.cpu())
    for buf, off, t in ((lbuf, lo, logits), (tbuf, to, labels)):
        b = buf.detach()
        assert bool((b[:4 + off] == GUARD[t.dtype]).all()) and bool((b[4 + off + t.numel():] == GUARD[t.dtype]).all()), 'an input guard element changed'
    return got


@pytest.mark.parametrize('id', [c['id'] for c in R.CASES])
def test_lovasz_cases(dev, id):
    case = R.CASE[id]
    logits, labels = R.inputs(id)
    F, C, V = logits.shape
    ref = R.reference(id)                                    # float64, its own order
    got = _run(dev, logits, labels, offsets=(1, 2) if case['content'] == 'guard' else (0, 0))
    _judge(id, R.compare(got, ref, ('errors',)))
    handed = R.lovasz64(logits, labels, R.WEIGHT, R.GOUT, order_from=got['errors'])      # float64 on the device's ranking
    assert torch.equal(got['present'], handed['present']) and torch.equal(got['present'], ref['present'])
    _judge(id, R.compare(got, handed, ('dlde',)))
    _judge(id, R.compare(got, ref, ('loss',)))
    lfc = LR.error_stats(got['frame_class_loss'], handed['frame_class_loss'], handed['frame_class_loss'].abs().clamp_min(LR.SCALAR_FLOOR))
    print(f'LOSSSTAT {id} frame_class_loss: {lfc["max_e"]:.3e} ({R.BARS["lovasz_loss"]:.2e})')
    assert lfc['max_e'] <= R.BARS['lovasz_loss']
    _judge(id, R.compare(got, handed, ('dlogits',)))
    ign = (labels.long() >= C)[:, None, :].expand(F, C, V)
    assert not got['dlogits'][ign].any() and not got['dlde'][ign].any() and not got['errors'][ign].any()
    assert bool(torch.isfinite(got['loss'])) and all(bool(torch.isfinite(got[k]).all()) for k in ('dlogits', 'errors', 'dlde'))
    if case['content'] == 'frame-ignored':
        assert not got['dlogits'][1].any() and not got['present'][1].any() and bool((labels[1] == 255).all())
    if case['content'] == 'one':
        assert got['present'].tolist() == [[True, False], [False, True], [False, False]]
    if case['content'] == 'all-fg':                          # the known answer, without the oracle: U = G at every rank
        valid = labels[0] == 1
        G = int(valid.sum())
        assert torch.equal(got['dlde'][0, 1][valid], torch.full((G,), 1.0 / G).float()) and not got['dlde'][0, 0].any()
    if case['content'] == 'const':                           # every error of classes 0 and 1 ties: the ranking is the voxel index
        valid = labels[0].long() < C
        for c in (0, 1):
            assert bool((got['errors'][0, c][valid] == 0.5).all())
            st = LR.error_stats(got['dlde'][0, c], R.index_order_dlde(labels, C, 0, c), R.index_order_dlde(labels, C, 0, c).abs())
            assert st['max_e'] <= R.BARS['lovasz_dlde'], st
    if case['content'] == 'sat':                             # errors of exactly 0 and exactly 1, and denormal ones in between
        e = got['errors'][~ign]
        assert bool((e == 0).any()) and bool((e == 1).any()) and bool(((e > 0) & (e < 1e-30)).any())


def test_second_call_is_bit_identical_in_both_modes(dev):
    from muvo_amd import ops
    logits, labels = R.inputs('F1-C3-V70001-many-tiles-ragged-tail')
    first = _run(dev, logits, labels, parts=False)
    second = _run(dev, logits, labels, parts=False)
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        det = _run(dev, logits, labels, parts=False)
        det2 = _run(dev, logits, labels, parts=False)
    finally:
        ops.set_deterministic(was)
    for other in (second, det, det2):
        assert torch.equal(first['loss'], other['loss']) and torch.equal(first['dlogits'], other['dlogits'])


@pytest.mark.parametrize('id', ['F2-C9-V4099-mix', 'F4-C2-V36864-guard-buffers'])
def test_optional_outputs_and_no_grad_leave_the_value_bit_equal(dev, id):
    from muvo_amd import ops
    logits, labels = R.inputs(id)
    l6, t6 = (t.to(dev) for t in _six(logits, labels))
    values = [ops._lovasz_forward(l6, t6, R.WEIGHT, with_dlde, with_errors)[2] for with_dlde in (False, True) for with_errors in (False, True)]
    l6.requires_grad_(True)
    with_grad = ops.voxel_lovasz_loss(l6, t6, R.WEIGHT)
    assert with_grad.requires_grad
    with torch.no_grad():
        without = ops.voxel_lovasz_loss(l6, t6, R.WEIGHT)
    assert not without.requires_grad
    again = ops.voxel_lovasz_loss(l6, t6, R.WEIGHT, terms=True)[0]
    assert again.dim() == 0 and torch.equal(again.detach(), without[0])
    for v in values + [with_grad.detach()]:
        assert torch.equal(v, without)
    print(f'LOSSSTAT {id} no_grad: {float(without):.9g} == {float(with_grad.detach()):.9g}')


def test_terms_and_upstream_gradient_from_the_device(dev):
    from muvo_amd import ops
    id = 'F2-C2-V4099-mix'
    logits, labels = R.inputs(id)
    l6, t6 = (t.to(dev) for t in _six(logits, labels))
    l6.requires_grad_(True)
    w = LR.f32r(0.37)
    errors = ops.voxel_lovasz_parts(l6, t6)[0].cpu()
    grads = []
    for g in (LR.f32r(-2.5), LR.f32r(0.75)):
        term = ops.voxel_lovasz_loss(l6, t6, w, terms=True)[0]
        assert term.dim() == 0
        up = torch.tensor(g, device=dev)                     # the upstream scalar stays on the device
        grad, = torch.autograd.grad(term * up, l6)
        ref = R.lovasz64(logits, labels, w, g, order_from=errors)
        _judge(f'{id} weight 0.37 gout {g}', R.compare({'loss': term.detach().cpu(), 'dlogits': grad[0].flatten(2).cpu()}, ref, ('loss', 'dlogits')))
        grads.append(grad)
    st = LR.error_stats(grads[1], grads[0] * (0.75 / -2.5), LR.scale_of(grads[1]))
    assert st['max_e'] <= R.BARS['lovasz_grad']


def test_module_equals_the_ops_call(dev):
    from muvo_amd import ops
    from muvo_amd.losses import LovaszSoftmaxLoss
    logits, labels = R.inputs('F2-C2-V257-frame-all-ignored')
    l6 = logits.view(1, 2, 2, 257, 1, 1).to(dev).requires_grad_(True)
    t6 = labels.view(1, 2, 1, 257, 1, 1).to(dev)
    a = LovaszSoftmaxLoss()(l6, t6)
    ga, = torch.autograd.grad(a, l6)
    b = ops.voxel_lovasz_loss(l6, t6, 1.0)[0]
    gb, = torch.autograd.grad(b, l6)
    assert a.dim() == 0 and torch.equal(a.detach(), b.detach()) and torch.equal(ga, gb)


def test_argument_errors(dev):
    """rejected by the argument checks of the launcher: nothing is launched"""
    from muvo_amd import ops
    lab = torch.zeros(1, 1, 1, 2, 2, 2, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='classes'):
        ops.voxel_lovasz_loss(torch.zeros(1, 1, 17, 2, 2, 2, device=dev), lab, 1.0)
    with pytest.raises(RuntimeError, match='classes'):
        ops.voxel_lovasz_loss(torch.zeros(1, 1, 1, 2, 2, 2, device=dev), lab, 1.0)


def test_compute_loss_at_two_frames_of_base_1d(dev):
    """compute_loss on synthetic dicts with the shapes of 1 x 2 frames of test_base_1d, FACTORS [1, 2, 4]: each term and its
    gradient against the restatement on the device's ranking (one float64 evaluation per factor: handing the order over moves
    the loss by < 1e-10 relative, lovasz_reference.py), the other terms bit-identical to a run with the key absent."""
    import types
    from muvo_amd import ops
    from muvo_amd.trainer import WorldModelTrainer
    cfg0 = R.voxel_only_cfg()
    X, Y, Z = cfg0.VOXEL.SIZE
    C = cfg0.VOXEL_SEG.N_CLASSES
    batch, output = R.voxel_dicts(device=dev, sizes=tuple((X // f, Y // f, Z // f) for f in (1, 2, 4)), C=C)
    assert tuple(output['voxel_1'].shape) == (1, 2, 2, 192, 192, 64)
    for v in output.values():
        v.requires_grad_(True)

    def run(cfg):
        return WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)

    plain = run(cfg0)
    losses = run(R.voxel_only_cfg(**{'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5, 'LOSSES.VOXEL_LOVASZ.FACTORS': [1, 2, 4]}))
    assert list(losses) == list(plain) + ['voxel_lovasz_1', 'voxel_lovasz_2', 'voxel_lovasz_4']
    for k, v in plain.items():
        assert torch.equal(v.detach(), losses[k].detach()), f'{k} changed with the key on'
    for f in (1, 2, 4):
        pred, label = output[f'voxel_{f}'], batch[f'voxel_label_{f}']
        grad, = torch.autograd.grad(losses[f'voxel_lovasz_{f}'], pred)
        errors = ops.voxel_lovasz_parts(pred, label)[0].cpu()
        ref = R.lovasz64(pred.detach().cpu().flatten(0, 1).flatten(2), label.cpu().flatten(0, 1).flatten(1), 0.5 / f, 1.0, order_from=errors)
        got = {'loss': losses[f'voxel_lovasz_{f}'].detach().cpu(), 'dlogits': grad.flatten(0, 1).flatten(2).cpu(), 'errors': errors}
        _judge(f'compute_loss voxel_lovasz_{f}', R.compare(got, ref, ('errors', 'loss', 'dlogits')))


def test_training_step_with_the_key_on(dev):
    """one training step (1 x 2 frames of test_base_1d) with LOSSES.VOXEL_LOVASZ on and the same seeded step with it off, in the
    deterministic mode (two identical steps are bit-identical there and nowhere else): every other term bit-equal, exactly the
    three new names, the voxel decoder's gradients - and its parameters after the step - different."""
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg, voxel_lovasz
    from muvo_amd.data.synthetic import make_batch, make_noise
    from muvo_amd.trainer import WorldModelTrainer
    from muvo_amd.utils import detinit
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        cfg = base_1d_cfg(RECEPTIVE_FIELD=2, FUTURE_HORIZON=0, STEPS=100000)
        tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
        tr.train()
        tr.preprocess.augment = False
        detinit.fill_state_dict_(tr.model)
        for layer in tr.model.transformer_encoder.layers:
            layer.p = 0.0
        opts, _ = tr.configure_optimizers()
        eps, use_prior = make_noise(1, 2, seed=1234)
        eps = eps.to(dev)
        head = [n for n, _ in tr.model.named_parameters() if n.startswith('voxel_decoder.')]
        rgb = [n for n, _ in tr.model.named_parameters() if n.startswith('rgb_decoder.')]
        assert head and rgb

        def step():
            opts[0].zero_grad()
            tr.model.seed_epoch, tr.model._step_seed = 1, 0
            tr.training_step(make_batch(1, 2, seed=1234, device=dev), 0, noise=eps, use_prior=use_prior).backward()
            ops.join_side_streams()
            params = dict(tr.model.named_parameters())
            return dict(tr.last_losses), {n: params[n].grad.detach().clone() for n in head}

        off, g_off = step()
        assert not [k for k in off if k.startswith('voxel_lovasz')] and voxel_lovasz(tr.cfg)[0] == 0.0
        tr.cfg.LOSSES['VOXEL_LOVASZ'] = type(tr.cfg)({'WEIGHT': 0.5})
        assert voxel_lovasz(tr.cfg) == (0.5, (1, 2, 4))
        on, g_on = step()
        params = dict(tr.model.named_parameters())
        before = {n: params[n].detach().clone() for n in head}
        opts[0].step()
        torch.cuda.synchronize()
        after = {n: params[n].detach().clone() for n in head + rgb}
    finally:
        ops.set_deterministic(was)
    names = ['voxel_lovasz_1', 'voxel_lovasz_2', 'voxel_lovasz_4']
    assert list(on) == list(off) + names
    for k in names:
        assert bool(torch.isfinite(on[k])) and 0 < float(on[k]) <= 0.5
        print(f'LOSSSTAT training-step {k}: {float(on[k]):.6g}')
    for k, v in off.items():
        assert torch.equal(v, on[k]), f'{k} changed with the key on'
    assert all(bool(torch.isfinite(g).all()) for g in g_on.values())
    assert any(not torch.equal(g_on[n], g_off[n]) for n in head)
    assert any(not torch.equal(after[n], before[n]) for n in head)
    assert not any(bool(torch.isnan(after[n]).any()) for n in rgb)
