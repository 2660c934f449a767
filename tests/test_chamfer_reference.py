"""CPU: the float64 restatement of the Chamfer-distance loss (tests/chamfer_reference.py) against the fixture made from the
reference's CDLoss (tests/golden/chamfer_loss.npz, tools/golden/make_golden_chamfer.py), the bars against planted errors, and
the configuration surface of the extension key LOSSES.LIDAR_CD."""
import argparse
import types

import pytest
import torch

import chamfer_reference as R
import loss_reference as LR


# ------------------------------------------------------------------------------------------------ restatement vs the fixture
@pytest.mark.parametrize('k', range(len(R.GOLDEN_SHAPES)), ids=['F%d-n%d' % s for s in R.GOLDEN_SHAPES])
def test_restatement_matches_reference_fixture(k):
    z = R.load_golden()
    frames, n = R.GOLDEN_SHAPES[k]
    assert tuple(z['shapes'][k]) == (frames, n) and z[f'pred_{k}'].shape == (frames, n, 3)
    pred, target = R.golden_planar(z, k)
    ref = R.chamfer64(pred, target)
    R.assert_gaps(ref, f'fixture {k}')
    e_loss = abs(float(ref['loss']) - float(z[f'loss_{k}'])) / abs(float(ref['loss']))
    want = torch.from_numpy(z[f'dpred_{k}']).permute(0, 2, 1)
    st = LR.error_stats(want, ref['dpred'], LR.scale_of(ref['dpred']))
    print(f'LOSSSTAT fixture-{k} reference-vs-float64: loss {e_loss:.3e} dpred {st["max_e"]:.3e} (recorded {float(z[f"ref_f64_dpred_{k}"]):.3e})')
    assert e_loss <= 1e-6
    # the distance is the reference's own matmul-form error; 2 x absorbs the platform's rounding of that form, nothing more
    assert st['max_e'] <= 2 * float(z[f'ref_f64_dpred_{k}'])
    if n > 25:       # above 25 rows the reference is measurably off, as recorded
        assert float(z[f'ref_f64_dpred_{k}']) > R.BARS['chamfer_grad']


def test_tie_goes_to_the_lowest_index():
    pred = torch.tensor([[[0.0, 1.0, 5.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])          # points (0,0,0), (1,0,0), (5,0,0)
    target = torch.tensor([[[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])        # three identical points between the first two
    ref = R.chamfer64(pred, target)
    assert ref['idx_pt'].tolist() == [[0, 0, 0]] and ref['idx_tp'].tolist() == [[0, 0, 0]]
    assert float(ref['gap_pt'].min()) == 0.0
    with pytest.raises(AssertionError, match='another seed'):
        R.assert_gaps(ref)


# ------------------------------------------------------------------------------------------------ bars vs planted errors
def _bad(got, ref, origin=False):
    return set(R.failures(R.compare(got, ref, origin)))


@pytest.mark.parametrize('id', [c['id'] for c in R.CASES])
def test_float32_evaluation_is_within_the_bars(id):
    pred, target, _ = R.inputs(id)
    ref = R.reference(id)
    got = R.chamfer64(pred, target, R.WEIGHT, R.GOUT, dtype=torch.float32)
    cmp = R.compare(got, ref, origin=R.CASE[id]['content'] == 'origin')
    for line in R.statlines(id + ' float32', cmp):
        print(line)
    assert not R.failures(cmp)


@pytest.mark.parametrize('id', ['n257-second-query-slot', 'n1031-two-workgroups-two-tiles', 'origin-half-targets-collide-n1031'])
def test_bars_reject_planted_errors(id):
    pred, target, _ = R.inputs(id)
    ref = R.reference(id)
    origin = R.CASE[id]['content'] == 'origin'
    n = R.CASE[id]['n']
    # one swapped index, in either direction: the second-nearest neighbour instead of the nearest
    for which, q, s in (('idx_pt', pred, target), ('idx_tp', target, pred)):
        i = n // 2 + 1           # (an odd index: a non-origin target in the origin case)
        d2 = ((q[0, :3, i][:, None] - s[0, :3]) ** 2).sum(0).double()
        second = int(d2.topk(2, largest=False)[1][1])
        idx = {k: ref[k].clone() for k in ('idx_pt', 'idx_tp')}
        assert idx[which][0, i] != second
        idx[which][0, i] = second
        got = R.chamfer64(pred, target, R.WEIGHT, R.GOUT, idx=(idx['idx_pt'], idx['idx_tp']))
        assert 'dpred' in _bad(got, ref, origin), which
    # a missing 1/n
    assert _bad({'loss': ref['loss'] * n, 'dpred': ref['dpred'] * n}, ref, origin) == {'loss', 'dpred'}
    # the sign of one direction
    assert 'dpred' in _bad({'loss': ref['loss'], 'dpred': ref['dpred_pt'] - ref['dpred_tp']}, ref, origin)
    assert 'dpred' in _bad({'loss': ref['loss'], 'dpred': ref['dpred_tp'] - ref['dpred_pt']}, ref, origin)
    # one direction only
    assert _bad({'loss': ref['loss'], 'dpred': ref['dpred_pt']}, ref, origin) == {'dpred'}


def test_bars_reject_a_gradient_at_distance_zero():
    id = 'coincident-point-zero-distance'
    pred, target, extra = R.inputs(id)
    ref = R.reference(id)
    i, j = extra['pair']
    assert torch.equal(pred[0, :3, i], target[0, :3, j])
    assert int(ref['idx_pt'][0, i]) == j and int(ref['idx_tp'][0, j]) == i
    assert torch.isfinite(ref['dpred']).all()
    # both terms of point i are the coincident pair: what is left is what other targets send to it
    others = [k for k in range(R.CASE[id]['n']) if int(ref['idx_tp'][0, k]) == i and k != j]
    if not others:
        assert not ref['dpred'][0, :, i].any()
    for plant in (float('nan'), float(ref['dpred'].abs().max())):           # 0/0, or a unit vector's worth
        got = {'loss': ref['loss'], 'dpred': ref['dpred'].clone()}
        got['dpred'][0, 0, i] += plant
        assert _bad(got, ref) == {'dpred'}


# ------------------------------------------------------------------------------------------------ configuration
def test_defaults_do_not_carry_the_key():
    from muvo_amd import config
    cfg = config.get_cfg()
    assert 'LIDAR_CD' not in cfg.LOSSES and 'LIDAR_CD' not in config.base_1d_cfg().LOSSES
    assert config.lidar_cd(cfg) == (0.0, (2, 4))
    text = open(config.os.path.join(config._HERE, 'configs', 'defaults.yml')).read()
    assert 'LIDAR_CD' not in text


def test_key_round_trips_through_yaml_dict_and_override(tmp_path):
    from muvo_amd import config
    y = tmp_path / 'cd.yml'
    y.write_text('LIDAR_RE: {ENABLED: true}\nLOSSES:\n  LIDAR_CD: {WEIGHT: 0.5, FACTORS: [1, 2, 4]}\n')
    cfg = config.get_cfg(argparse.Namespace(config_file=str(y), opts=[]))
    assert config.lidar_cd(cfg) == (0.5, (1, 2, 4))
    assert cfg.convert_to_dict()['LOSSES']['LIDAR_CD'] == {'WEIGHT': 0.5, 'FACTORS': [1, 2, 4]}
    again = config.get_cfg(cfg_dict=cfg.convert_to_dict())                   # the dict a checkpoint carries
    assert config.lidar_cd(again) == (0.5, (1, 2, 4))
    cfg = config.get_cfg(cfg_dict={'LIDAR_RE': {'ENABLED': True}, 'LOSSES': {'LIDAR_CD': {'WEIGHT': 2}}})
    assert config.lidar_cd(cfg) == (2.0, (2, 4))                              # FACTORS absent: [2, 4]
    cfg = config.get_cfg(argparse.Namespace(config_file='', opts=['LIDAR_RE.ENABLED', 'True', 'LOSSES.LIDAR_CD.WEIGHT', '0.25',
                                                                  'LOSSES.LIDAR_CD.FACTORS', '[4]']))
    assert config.lidar_cd(cfg) == (0.25, (4,))
    cfg = config.base_1d_cfg(**{'LOSSES.LIDAR_CD.WEIGHT': 0.5})
    assert config.lidar_cd(cfg) == (0.5, (2, 4))
    with pytest.raises(KeyError):
        config.get_cfg().merge_from_list(['LOSSES.LIDAR_CE.WEIGHT', '1'])


@pytest.mark.parametrize('factors', [[3], [2, 8], [0], [2, 2], 2, [True]], ids=str)
def test_bad_factors_raise(factors):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'LIDAR_RE': {'ENABLED': True}, 'LOSSES': {'LIDAR_CD': {'WEIGHT': 1.0, 'FACTORS': factors}}})
    with pytest.raises(ValueError, match='FACTORS'):
        config.lidar_cd(cfg)


def test_bad_weight_and_disabled_head_raise():
    from muvo_amd import config
    with pytest.raises(ValueError, match='LIDAR_RE.ENABLED'):
        config.lidar_cd(config.get_cfg(cfg_dict={'LIDAR_RE': {'ENABLED': False}, 'LOSSES': {'LIDAR_CD': {'WEIGHT': 1.0}}}))
    assert config.lidar_cd(config.get_cfg(cfg_dict={'LIDAR_RE': {'ENABLED': False}, 'LOSSES': {'LIDAR_CD': {'WEIGHT': 0.0}}}))[0] == 0.0
    for w in (-1.0, 'much', True):
        with pytest.raises(ValueError, match='WEIGHT'):
            config.lidar_cd(config.get_cfg(cfg_dict={'LIDAR_RE': {'ENABLED': True}, 'LOSSES': {'LIDAR_CD': {'WEIGHT': w}}}))


def test_compute_loss_key_set_with_and_without_the_key(monkeypatch):
    """the trainer's wiring with the kernels stubbed out: without the key today's terms and no Chamfer call; with it one call
    per configured factor, on the head's tensors as they are, with weight WEIGHT / f"""
    from muvo_amd import ops
    from muvo_amd.trainer import WorldModelTrainer
    calls = []
    monkeypatch.setattr(ops, 'spatial_losses', lambda pred, target, parts, *a, **k: tuple(torch.zeros(()) for _ in parts))

    def chamfer(pred, target, weight, terms=False):
        calls.append((pred, target, weight, terms))
        return (torch.zeros(()),)
    monkeypatch.setattr(ops, 'chamfer_loss', chamfer)
    batch, output = R.lidar_dicts()
    today = ['lidar_re_1', 'lidar_depth_1', 'lidar_re_2', 'lidar_depth_2', 'lidar_re_4', 'lidar_depth_4']
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=R.lidar_only_cfg()), batch, output)
    assert list(losses) == today and not calls
    cfg = R.lidar_only_cfg(**{'LOSSES.LIDAR_CD.WEIGHT': 0.5})
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
    assert list(losses) == today + ['lidar_cd_2', 'lidar_cd_4']
    assert [(c[2], c[3]) for c in calls] == [(0.25, True), (0.125, True)]
    assert calls[0][0] is output['lidar_reconstruction_2'] and calls[0][1] is batch['range_view_label_2']
    assert calls[1][0] is output['lidar_reconstruction_4'] and calls[1][1] is batch['range_view_label_4']
    del calls[:]
    cfg = R.lidar_only_cfg(**{'LOSSES.LIDAR_CD.WEIGHT': 0.5, 'LOSSES.LIDAR_CD.FACTORS': [1]})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today + ['lidar_cd_1']
    assert calls[0][2] == 0.5 and calls[0][0] is output['lidar_reconstruction_1']


def test_cdloss_module_guards():
    from muvo_amd.losses import CDLoss
    with pytest.raises(NotImplementedError):
        CDLoss(reducer=torch.sum)
    crit = CDLoss()
    with pytest.raises(ValueError):
        crit(torch.zeros(1, 2, 5, 4), torch.zeros(1, 2, 5, 4))


def test_entry_points_validate_before_touching_the_device():
    """bad arguments come back as MUVO_ERR_INVALID_ARG with a message; nothing is launched (this runs without a GPU)"""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    p = C.c_void_p(256)            # never dereferenced: every call below is rejected by its argument checks
    i64, st = C.c_int64, C.c_void_p(0)
    assert L.muvo_chamfer_loss_ws_doubles(i64(20), i64(65536)) == 2 * 20 * 64 and L.muvo_chamfer_loss_ws_doubles(i64(1), i64(1)) == 2
    assert L.muvo_chamfer_loss_fwd(p, p, i64(65536), 3, 3, i64(8), C.c_float(1.0), p, p, p, p, st) == -1
    assert b'65535 frames' in L.muvo_last_error()
    assert L.muvo_chamfer_loss_fwd(p, p, i64(2), 2, 3, i64(8), C.c_float(1.0), p, p, p, p, st) == -1          # no z plane
    assert L.muvo_chamfer_loss_fwd(p, p, i64(2), 3, 3, i64(0), C.c_float(1.0), p, p, p, p, st) == -1
    assert L.muvo_chamfer_loss_fwd(p, p, i64(2), 3, 3, i64(8), C.c_float(1.0), p, p, C.c_void_p(0), p, st) == -1          # one index array
    assert b'both index arrays or none' in L.muvo_last_error()
    assert L.muvo_chamfer_loss_fwd(p, p, i64(2), 3, 3, i64((1 << 30) + 1), C.c_float(1.0), p, C.c_void_p(0), C.c_void_p(0), p, st) == -1
    assert L.muvo_chamfer_loss_bwd(p, p, C.c_void_p(0), p, p, i64(2), 3, 3, i64(8), C.c_float(1.0), p, st) == -1
    assert b'chamfer_loss_bwd: null pointer' in L.muvo_last_error()
    assert L.muvo_chamfer_loss_bwd(p, p, p, p, p, i64(65536), 3, 3, i64(8), C.c_float(1.0), p, st) == -1
