"""-m gpu: sensor dropout (MODEL.TRANSFORMER.SENSOR_DROPOUT, batch['sensor_drop']; muvo_amd/models/mile.py) on the masked attention
kernels.  Block level: the fusion encoder's output of a frame does not depend on what its dropped sensor delivered - other values,
inf, NaN - bit for bit, and a frame that drops nothing has the bits of the run without a mask.  Model level (test_base_1d, 1 x 2
frames, deterministic mode): with a sensor dropped nothing but the losses on that sensor's own label depends on its input; without
the key and without `sensor_drop` no new code runs; a training step with SENSOR_DROPOUT.CAMERA = 1 has finite losses and
gradients and none for the camera encoder.  Tool level: `predict --mode test --drop-sensor camera` over a tiny recording."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 77


# ------------------------------------------------------------------------------------------------ the block
def test_encoder_ignores_a_dropped_sensor(dev):
    from muvo_amd import nn as hnn, ops
    from muvo_amd.models.common import position_embedding_sine
    from muvo_amd.models.mile import drop_sensor_features
    E, NI, NL, N = 96, 17, 15, 3
    torch.manual_seed(5)
    with torch.device(dev):
        enc = hnn.TransformerEncoder(E, 2, num_layers=2, dropout=0.1)
    enc.train()                                                # attention dropout on: the live pairs keep their bits
    g = torch.Generator().manual_seed(6)
    xi, xl = torch.randn(N, E, 1, NI, generator=g).to(dev), torch.randn(N, E, 1, NL, generator=g).to(dev)
    type_emb = torch.randn(1, 1, E, 2, generator=g).to(dev)
    pos_i, pos_l = position_embedding_sine(1, NI, E // 2).to(dev), position_embedding_sine(1, NL, E // 2).to(dev)
    drop = torch.tensor([0, 1, 2], dtype=torch.int8, device=dev)

    def run(xi, xl, drop):
        mask = None
        if drop is not None:
            xi, xl, mask = drop_sensor_features(drop, xi, xl)
            assert mask.sum(1).tolist() == [0, NI, NL]
        tokens = ops.make_tokens(xi, xl, pos_i, pos_l, type_emb)
        assert tuple(tokens.shape) == (NI + NL, N, E)
        return enc(tokens, 3) if mask is None else enc(tokens, 3, mask)

    base = run(xi, xl, drop).detach()
    assert torch.isfinite(base).all()
    for fill in (3.25, float('inf'), float('nan')):
        yi, yl = xi.clone(), xl.clone()
        yi[1] = fill                                           # frame 1 has no camera, frame 2 no lidar
        yl[2] = -fill
        got = run(yi, yl, drop)
        assert torch.equal(got, base), fill
    plain = run(xi, xl, None)
    assert torch.equal(plain[:, 0], base[:, 0])                # frame 0 drops nothing: the bits of the run without a mask
    assert not torch.equal(plain[:, 1], base[:, 1]) and not torch.equal(plain[:, 2], base[:, 2])
    # the dropped sensor's tokens are still queries: their output rows differ from token to token
    assert float(base[:NI, 1].std(0).mean()) > 1e-3 and float(base[NI:, 2].std(0).mean()) > 1e-3


def test_encoder_gradients_with_a_mask(dev):
    """backward through two masked layers: finite, and nothing flows to the dropped sensor's features"""
    from muvo_amd import nn as hnn, ops
    from muvo_amd.models.common import position_embedding_sine
    from muvo_amd.models.mile import drop_sensor_features
    E, NI, NL, N = 96, 17, 15, 3
    torch.manual_seed(5)
    with torch.device(dev):
        enc = hnn.TransformerEncoder(E, 2, num_layers=2, dropout=0.0)
    g = torch.Generator().manual_seed(8)
    xi = torch.randn(N, E, 1, NI, generator=g).to(dev).requires_grad_(True)
    xl = torch.randn(N, E, 1, NL, generator=g).to(dev).requires_grad_(True)
    type_emb = torch.randn(1, 1, E, 2, generator=g).to(dev)
    pos_i, pos_l = position_embedding_sine(1, NI, E // 2).to(dev), position_embedding_sine(1, NL, E // 2).to(dev)
    drop = torch.tensor([0, 1, 2], dtype=torch.int8, device=dev)
    yi, yl, mask = drop_sensor_features(drop, xi, xl)
    out = enc(ops.make_tokens(yi, yl, pos_i, pos_l, type_emb), 3, mask)
    out.backward(torch.randn(out.shape, generator=g).to(dev))
    assert torch.isfinite(xi.grad).all() and torch.isfinite(xl.grad).all()
    assert all(torch.isfinite(p.grad).all() for p in enc.parameters())
    assert (xi.grad[1] == 0).all() and (xl.grad[2] == 0).all()
    assert float(xi.grad[0].abs().max()) > 0 and float(xi.grad[2].abs().max()) > 0 and float(xl.grad[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the model
def _tensors(out, prefix=''):
    flat = {}
    for k, v in out.items():
        if isinstance(v, dict):
            flat.update(_tensors(v, f'{prefix}{k}.'))
        elif torch.is_tensor(v):
            flat[prefix + k] = v.detach()
    return flat


# losses that read the sensor's own label (made from its input), by the start of their name
LABEL_LOSSES = {'camera': ('rgb_', 'ssim_'), 'lidar': ('lidar_re_', 'lidar_depth_', 'lidar_cd_', 'voxel_render')}


@pytest.fixture(scope='module')
def trainer(dev):
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg
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
        yield tr
    finally:
        ops.set_deterministic(was)


def _forward(tr, dev, drop=None, image_seed=1234, lidar_seed=1234):
    from muvo_amd import ops
    from muvo_amd.data.synthetic import make_batch, make_noise
    eps, use_prior = make_noise(1, 2, seed=1234)
    batch = make_batch(1, 2, seed=1234, device=dev)
    if image_seed != 1234:
        batch['image'] = make_batch(1, 2, seed=image_seed, device=dev)['image']
    if lidar_seed != 1234:
        batch['range_view_pcd_xyzd'] = make_batch(1, 2, seed=lidar_seed, device=dev)['range_view_pcd_xyzd']
    if drop is not None:
        batch['sensor_drop'] = torch.tensor(drop, dtype=torch.int8)
    tr.model.seed_epoch, tr.model._step_seed = 1, 0
    with torch.no_grad():
        losses, output, _, _ = tr.shared_step(batch, mode='train', noise=eps.to(dev), use_prior=use_prior)
    ops.join_side_streams()
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in losses.items()}, _tensors(output)


@pytest.mark.parametrize('sensor,code', [('camera', 1), ('lidar', 2)])
def test_model_ignores_a_dropped_sensor(dev, trainer, sensor, code):
    other = dict(image_seed=4321) if sensor == 'camera' else dict(lidar_seed=4321)
    la, oa = _forward(trainer, dev, [code])
    lb, ob = _forward(trainer, dev, [code], **other)
    assert sorted(oa) == sorted(ob) and len(oa) > 10 and sorted(la) == sorted(lb)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), f'output {k} depends on the dropped {sensor}'
        assert torch.isfinite(oa[k].float()).all(), k
    own = [k for k in la if k.startswith(LABEL_LOSSES[sensor])]
    assert own, sorted(la)
    for k in la:
        assert bool(torch.isfinite(la[k])), k
        if k not in own:
            assert torch.equal(la[k], lb[k]), f'loss {k} depends on the dropped {sensor}'
    assert any(not torch.equal(la[k], lb[k]) for k in own)       # the label did change
    # and the other input is NOT ignored: with the sensor present the outputs differ
    _, oc = _forward(trainer, dev, None)
    _, od = _forward(trainer, dev, None, **other)
    assert any(not torch.equal(oc[k], od[k]) for k in oc)
    assert any(not torch.equal(oc[k], oa[k]) for k in oc)        # dropping does something


def test_model_without_the_key_runs_no_new_code(dev, trainer, monkeypatch):
    from muvo_amd import ops
    from muvo_amd.models import mile
    assert trainer.model.sensor_dropout == (0.0, 0.0)
    want_l, want_o = _forward(trainer, dev, None)
    called = []
    monkeypatch.setattr(ops, 'key_mask_rows', lambda *a, **k: called.append('key_mask_rows'))
    monkeypatch.setattr(mile, 'drop_sensor_features', lambda *a, **k: called.append('drop_sensor_features'))
    monkeypatch.setattr(mile, 'draw_sensor_drop', lambda *a, **k: called.append('draw_sensor_drop'))
    monkeypatch.setattr(ops, '_MASKED_ATTENTION_FNS', {})
    got_l, got_o = _forward(trainer, dev, None)
    zero_l, zero_o = _forward(trainer, dev, [0])                  # "none" for every sequence: the same path
    assert not called
    for k in want_o:
        assert torch.equal(want_o[k], got_o[k]) and torch.equal(want_o[k], zero_o[k]), k
    for k in want_l:
        assert torch.equal(want_l[k], got_l[k]) and torch.equal(want_l[k], zero_l[k]), k
    with pytest.raises(ValueError, match='sensor_drop'):
        _forward(trainer, dev, [3])
    with pytest.raises(ValueError, match='sensor_drop'):
        _forward(trainer, dev, [1, 2])


def test_training_step_with_the_camera_always_dropped(dev):
    from muvo_amd import ops
    from muvo_amd.config import base_1d_cfg, sensor_dropout
    from muvo_amd.data.synthetic import make_batch, make_noise
    from muvo_amd.trainer import WorldModelTrainer
    from muvo_amd.utils import detinit
    cfg = base_1d_cfg(RECEPTIVE_FIELD=2, FUTURE_HORIZON=0, STEPS=100000, MODEL__TRANSFORMER__SENSOR_DROPOUT__CAMERA=1.0)
    assert sensor_dropout(cfg) == (1.0, 0.0)
    tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    tr.train()
    tr.preprocess.augment = False
    detinit.fill_state_dict_(tr.model)
    assert tr.model.sensor_dropout == (1.0, 0.0)
    opts, _ = tr.configure_optimizers()
    opts[0].zero_grad()
    eps, use_prior = make_noise(1, 2, seed=1234)
    tr.training_step(make_batch(1, 2, seed=1234, device=dev), 0, noise=eps.to(dev), use_prior=use_prior).backward()
    ops.join_side_streams()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in tr.last_losses.values()), tr.last_losses
    camera, seen = ('encoder.', 'feat_decoder.'), 0
    for name, p in tr.model.named_parameters():
        if p.grad is None:
            continue
        assert torch.isfinite(p.grad).all(), name
        if name.startswith(camera):
            assert not p.grad.any(), f'{name}: the dropped camera encoder has a gradient'
        seen += 1
    assert seen > 100
    lidar = [p.grad for n, p in tr.model.named_parameters() if n.startswith('range_view_encoder.') and p.grad is not None]
    assert lidar and any(g.any() for g in lidar)
    tr.eval()                                                      # evaluation mode: nothing is drawn
    assert tr.model._sensor_drop({}, 1, 2, dev) is None


# ------------------------------------------------------------------------------------------------ the tool
def test_predict_drop_sensor(dev, tmp_path_factory):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import ops, predict as P
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path_factory.mktemp('rec'))
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(SEED)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)

    def data():
        dm = DataModule(cfg, root, device=dev, seed=SEED)
        dm.setup()
        dm.test_sampler_0 = range(0, 4, 2)
        return dm

    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        out = {}
        for name, drop in (('plain', None), ('camera', 'camera')):
            d = str(tmp_path_factory.mktemp(name))
            res = P.run(cfg, dev, d, 'test', loaders=[0], limit_batches=1, seed=SEED, data=data(), module=module, log=lambda s: None,
                        drop_sensor=drop)
            assert res['batches'] == {0: 1}
            out[name] = json.load(open(os.path.join(d, 'metrics.json')))
    finally:
        ops.set_deterministic(was)
    names = P.expected_metric_names(cfg, {0: 1})
    assert sorted(out['plain']) == sorted(names + ['batches'])
    assert sorted(out['camera']) == sorted(names + ['batches', 'drop_sensor']) and out['camera']['drop_sensor'] == 'camera'
    assert all(isinstance(out['camera'][n], float) and np.isfinite(out['camera'][n]) for n in names), out['camera']
    assert any(out['camera'][n] != out['plain'][n] for n in names)
    bad = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    bad.MODEL.TRANSFORMER['ENABLED'] = False
    with pytest.raises(ValueError, match='TRANSFORMER.ENABLED'):
        P.run(bad, dev, str(tmp_path_factory.mktemp('bad')), 'test', drop_sensor='camera', data=data(), module=module, log=lambda s: None)
