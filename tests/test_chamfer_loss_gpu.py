"""-m gpu: the Chamfer-distance training loss (muvo_amd/csrc/chamfer.hip through ops.chamfer_loss, losses.CDLoss and
WorldModelTrainer.compute_loss) against the float64 restatement of tests/chamfer_reference.py with its normalised error and
bars (4 x the error of the float32 CPU evaluation of the same restatement; tests/test_chamfer_reference.py shows on the CPU that
these bars reject planted errors).  Every case's inputs have a nearest / second-nearest gap >= 1e-4 for EVERY query - asserted
on the CPU (chamfer_reference.reference / assert_gaps) before anything is judged - so the kernel must select exactly the
float64 neighbours; no case and no point is excluded.  Each case prints `LOSSSTAT <id> <name>: max_e rms (bar)` lines."""
import pytest
import torch

import chamfer_reference as R
import loss_reference as LR

pytestmark = pytest.mark.gpu
GUARD = 12345.0


def _judge(tag, cmp):
    for line in R.statlines(tag, cmp):
        print(line)
    bad = R.failures(cmp)
    assert not bad, f'{tag}: ' + '; '.join(f'{n} max_e {s["max_e"]:.3e} at {s["index"]} (bar {cmp[n][1]:.2e})' for n, s in bad.items())


def _place(t, dev, off, grad=False):
    """`t` on the device inside a fresh buffer of GUARD values, `off` elements after four guard elements (so the view starts
    4 * (4 + off) bytes after an at least 256-byte aligned address); returns (buffer, contiguous view of t's shape)"""
    n = t.numel()
    buf = torch.full((n + 12,), GUARD, dtype=t.dtype, device=dev)
    buf[4 + off:4 + off + n] = t.reshape(-1).to(dev)
    if grad:
        buf.requires_grad_(True)
    return buf, buf[4 + off:4 + off + n].view(t.shape)


def _run(dev, pred, target, weight=R.WEIGHT, gout=R.GOUT, offsets=(1, 2)):
    """ops.chamfer_loss forward + backward on (F, C, n) planar CPU tensors placed at element offsets; returns loss, dpred (F, C, n)
    and the two index arrays, after checking that nothing outside the views was written"""
    from muvo_amd import ops
    F, C, n = pred.shape
    po, to = offsets
    pbuf, pg = _place(pred.view(1, F, C, 1, n), dev, po, grad=True)
    tbuf, tg = _place(target.view(1, F, target.shape[1], 1, n), dev, to)
    out = ops.chamfer_loss(pg, tg, weight)
    assert out.shape == (1,)
    (gout * out[0]).backward()
    idx = ops.chamfer_nearest(pg, tg)
    grad = pbuf.grad
    assert not grad[:4 + po].any() and not grad[4 + po + pred.numel():].any(), 'gradient written outside the view'
    for buf, off, t in ((pbuf, po, pred), (tbuf, to, target)):
        b = buf.detach()
        assert bool((b[:4 + off] == GUARD).all()) and bool((b[4 + off + t.numel():] == GUARD).all()), 'an input guard element changed'
    return {'loss': out[0].detach(), 'dpred': grad[4 + po:4 + po + pred.numel()].view(F, C, n), 'idx_pt': idx[0].cpu().long(),
            'idx_tp': idx[1].cpu().long()}


@pytest.mark.parametrize('id', [c['id'] for c in R.CASES])
def test_chamfer_loss_cases(dev, id):
    case = R.CASE[id]
    pred, target, extra = R.inputs(id)
    ref = R.reference(id)                                   # float64, gaps asserted for every query
    got = _run(dev, pred, target)
    assert bool(torch.isfinite(got['loss'])) and bool(torch.isfinite(got['dpred']).all())
    assert torch.equal(got['idx_pt'], ref['idx_pt']) and torch.equal(got['idx_tp'], ref['idx_tp']), 'another neighbour than float64'
    n = case['n']
    if case['C'] > 3:                                       # the depth plane: never read (NaN there), its gradient exactly 0
        assert bool(torch.isnan(pred[:, 3]).all()) and bool(torch.isnan(target[:, 3]).all())
        assert not got['dpred'][:, 3:].any()
        assert bool((ref['idx_pt'][0] != ref['idx_pt'][1]).any()) and bool((ref['idx_pt'][1] != ref['idx_pt'][2]).any())
    if case['content'] == 'perm':                           # the known answer, without the oracle
        perm = extra['perm']
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n)
        assert torch.equal(got['idx_tp'][0], perm) and torch.equal(got['idx_pt'][0], inv)
        for j, i in R.PERM_FIXED:
            assert int(got['idx_tp'][0, j]) == i
        assert {i for _, i in R.PERM_FIXED} >= {0, n - 1} and any(i >= n - n % 1024 for _, i in R.PERM_FIXED if n % 1024)
    if case['content'] == 'origin':                         # the heavy-collision scatter
        hit = torch.bincount(got['idx_tp'][0], minlength=n)
        assert int(hit.max()) >= n // 2 and bool((target[0, :3, ::2] == 0).all())
    if case['content'] == 'coincident':
        i, j = extra['pair']
        assert torch.equal(pred[0, :3, i], target[0, :3, j]) and int(got['idx_pt'][0, i]) == j and int(got['idx_tp'][0, j]) == i
        if int((got['idx_tp'][0] == i).sum()) == 1:         # nobody else sends to i: both of its terms have d = 0
            assert not got['dpred'][0, :, i].any()
    _judge(id, R.compare(got, ref, origin=case['content'] == 'origin'))


def test_weight_and_upstream_gradient(dev):
    id = 'n257-second-query-slot'
    pred, target, _ = R.inputs(id)
    w, g = LR.f32r(0.37), LR.f32r(-2.5)
    ref = R.chamfer64(pred, target, w, g)
    R.assert_gaps(ref, id)
    got = _run(dev, pred, target, weight=w, gout=g, offsets=(0, 0))
    _judge(id + ' weight 0.37 gout -2.5', R.compare(got, ref))
    plain = R.reference(id)
    assert abs(float(ref['loss']) / float(plain['loss']) - w / R.WEIGHT) < 1e-12


@pytest.mark.parametrize('id', ['n1031-two-workgroups-two-tiles', 'F3-C4-nan-plane3'])
def test_no_grad_value_is_bit_equal(dev, id):
    from muvo_amd import ops
    pred, target, _ = R.inputs(id)
    F, C, n = pred.shape
    pg = pred.view(1, F, C, 1, n).to(dev).requires_grad_(True)
    tg = target.view(1, F, C, 1, n).to(dev)
    with_grad = ops.chamfer_loss(pg, tg, R.WEIGHT)
    assert with_grad.requires_grad
    with torch.no_grad():
        without = ops.chamfer_loss(pg, tg, R.WEIGHT)
    assert not without.requires_grad
    assert torch.equal(with_grad.detach(), without)
    again = ops.chamfer_loss(pg, tg, R.WEIGHT, terms=True)[0]
    assert again.dim() == 0 and torch.equal(again.detach(), without[0])
    print(f'LOSSSTAT {id} no_grad: {float(without):.9g} == {float(with_grad):.9g}')


def test_deterministic_mode_on_the_collision_case(dev):
    from muvo_amd import ops
    id = 'origin-half-targets-collide-n1031'
    pred, target, _ = R.inputs(id)
    ref = R.reference(id)
    normal = _run(dev, pred, target)
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        first = _run(dev, pred, target)
        second = _run(dev, pred, target)
    finally:
        ops.set_deterministic(was)
    assert ops.get_deterministic() == was
    assert torch.equal(first['dpred'], second['dpred']) and torch.equal(first['loss'], second['loss'])
    assert torch.equal(first['loss'], normal['loss'])                   # the forward is the same in both modes
    _judge(id + ' deterministic', R.compare(first, ref, origin=True))
    against_normal = LR.error_stats(first['dpred'], normal['dpred'], LR.scale_of(normal['dpred']))
    print(f'LOSSSTAT {id} deterministic-vs-normal dpred: {against_normal["max_e"]:.3e} {against_normal["rms"]:.3e} '
          f'({R.BARS["chamfer_grad_origin"]:.2e})')
    assert against_normal['max_e'] <= R.BARS['chamfer_grad_origin']


@pytest.mark.parametrize('k', range(len(R.GOLDEN_SHAPES)), ids=['F%d-n%d' % s for s in R.GOLDEN_SHAPES])
def test_fixture_inputs_nearer_to_float64_than_the_reference(dev, k):
    z = R.load_golden()
    pred, target = R.golden_planar(z, k)
    ref = R.chamfer64(pred, target, R.WEIGHT, R.GOUT)
    R.assert_gaps(ref, f'fixture {k}')
    got = _run(dev, pred, target, offsets=(0, 1))
    assert torch.equal(got['idx_pt'], ref['idx_pt']) and torch.equal(got['idx_tp'], ref['idx_tp'])
    cmp = R.compare(got, ref)
    _judge(f'fixture-{k}', cmp)
    for name, recorded in (('loss', float(z[f'ref_f64_loss_{k}'])), ('dpred', float(z[f'ref_f64_dpred_{k}']))):
        stats, bar = cmp[name]
        print(f'LOSSSTAT fixture-{k} {name}: kernel {stats["max_e"]:.3e}, reference project {recorded:.3e}')
        if recorded > bar:
            assert stats['max_e'] < recorded
    # the drop-in module on the reference's own layout (b, s, n, 3): the same value as the reference's, to its own error
    from muvo_amd.losses import CDLoss
    p = torch.from_numpy(z[f'pred_{k}'])[None].to(dev).requires_grad_(True)
    loss = CDLoss()(p, torch.from_numpy(z[f'target_{k}'])[None].to(dev))
    loss.backward()
    plain = R.chamfer64(pred, target)
    _judge(f'fixture-{k} CDLoss', R.compare({'loss': loss.detach(), 'dpred': p.grad[0].permute(0, 2, 1)}, plain))
    assert abs(float(loss) - float(z[f'loss_{k}'])) <= 1e-6 * abs(float(z[f'loss_{k}']))


def test_argument_errors(dev):
    """rejected by the argument checks of the launcher: nothing is launched"""
    from muvo_amd import ops
    with pytest.raises(RuntimeError, match='chamfer_loss_fwd'):
        ops.chamfer_loss(torch.zeros(1, 2, 2, 1, 8, device=dev), torch.zeros(1, 2, 3, 1, 8, device=dev), 1.0)      # no z plane
    with pytest.raises(RuntimeError, match='65535 frames'):
        ops.chamfer_loss(torch.zeros(1, 65536, 3, 1, 1, device=dev), torch.zeros(1, 65536, 3, 1, 1, device=dev), 1.0)


def test_compute_loss_on_synthetic_dicts(dev):
    import types
    from muvo_amd import ops
    from muvo_amd.trainer import WorldModelTrainer
    batch, output = R.lidar_dicts(device=dev)
    assert [tuple(output[f'lidar_reconstruction_{f}'].shape) for f in (1, 2, 4)] == [(1, 2, 4, 8, 32), (1, 2, 4, 4, 16), (1, 2, 4, 2, 8)]
    for v in output.values():
        v.requires_grad_(True)
    keys = [f'lidar_reconstruction_{f}' for f in (1, 2, 4)]

    def run(cfg):
        losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
        total = ops.sum_scalars(list(losses.values()))
        grads = torch.autograd.grad(total, [output[k] for k in keys])
        return losses, dict(zip(keys, grads))

    plain, g_plain = run(R.lidar_only_cfg())
    cfg = R.lidar_only_cfg(**{'LOSSES.LIDAR_CD.WEIGHT': 0.5, 'LOSSES.LIDAR_CD.FACTORS': [1, 2, 4]})
    losses, g_total = run(cfg)
    assert list(losses) == list(plain) + ['lidar_cd_1', 'lidar_cd_2', 'lidar_cd_4']
    for k, v in plain.items():
        assert torch.equal(v.detach(), losses[k].detach()), f'{k} changed with the key on'
    for f in (1, 2, 4):
        pred, label = output[f'lidar_reconstruction_{f}'], batch[f'range_view_label_{f}']
        ref = R.chamfer64(pred.detach().cpu().flatten(0, 1).flatten(2), label.cpu().flatten(0, 1).flatten(2), 0.5 / f, 1.0)
        R.assert_gaps(ref, f'factor {f}')
        assert not ref['dpred'][:, 3].any()
        # the gradient of the total on the head's output = the sum of its two consumers' gradients
        g_cd, = torch.autograd.grad(ops.chamfer_loss(pred, label, 0.5 / f)[0], pred)
        both = g_plain[f'lidar_reconstruction_{f}'] + g_cd
        st = LR.error_stats(g_total[f'lidar_reconstruction_{f}'], both, LR.scale_of(both))
        print(f'LOSSSTAT compute_loss factor {f} total-vs-sum-of-consumers: {st["max_e"]:.3e} {st["rms"]:.3e} ({R.BARS["chamfer_grad"]:.2e})')
        assert st['max_e'] <= R.BARS['chamfer_grad']
        assert bool((g_cd.flatten(0, 1)[:, 3] == 0).all()) and bool((g_plain[f'lidar_reconstruction_{f}'].flatten(0, 1)[:, 3] != 0).any())
        _judge(f'compute_loss lidar_cd_{f}', R.compare({'loss': losses[f'lidar_cd_{f}'].detach(), 'dpred': g_cd.flatten(0, 1).flatten(2)}, ref))


def test_training_step_with_the_key_on(dev):
    """one training step (1 x 2 frames of test_base_1d) with LOSSES.LIDAR_CD on (factors 2, 4) and the same seeded step with it
    off, in the deterministic mode (two identical steps are bit-identical there and nowhere else): every other term bit-equal,
    the lidar head's parameter gradients different."""
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg, lidar_cd
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
        head = [n for n, _ in tr.model.named_parameters() if n.startswith('lidar_re.')]
        assert head

        def step():
            opts[0].zero_grad()
            tr.model.seed_epoch, tr.model._step_seed = 1, 0
            tr.training_step(make_batch(1, 2, seed=1234, device=dev), 0, noise=eps, use_prior=use_prior).backward()
            ops.join_side_streams()
            params = dict(tr.model.named_parameters())
            return dict(tr.last_losses), {n: params[n].grad.detach().clone() for n in head}

        off, g_off = step()
        assert not [k for k in off if k.startswith('lidar_cd')] and lidar_cd(tr.cfg)[0] == 0.0
        tr.cfg.LOSSES['LIDAR_CD'] = type(tr.cfg)({'WEIGHT': 0.5})
        assert lidar_cd(tr.cfg) == (0.5, (2, 4))
        on, g_on = step()
    finally:
        ops.set_deterministic(was)
    assert list(on) == list(off) + ['lidar_cd_2', 'lidar_cd_4']
    for k in ('lidar_cd_2', 'lidar_cd_4'):
        assert bool(torch.isfinite(on[k])) and float(on[k]) > 0
        print(f'LOSSSTAT training-step {k}: {float(on[k]):.6g}')
    for k, v in off.items():
        assert torch.equal(v, on[k]), f'{k} changed with the key on'
    assert all(bool(torch.isfinite(g).all()) for g in g_on.values())
    assert any(not torch.equal(g_on[n], g_off[n]) for n in head)
