"""CPU: the restatements of tests/edt_reference.py - the separable transform against the O(V^2) definition and, where it imports,
scipy.ndimage; the analytic gradient of the boundary loss against central differences - the configuration surface of the
extension key LOSSES.VOXEL_BOUNDARY, the trainer's wiring with stubs, VoxelDistanceMetric.summarise on hand-written counts and the
argument checks of the entries."""
import argparse
import types

import numpy as np
import pytest
import torch

import edt_reference as E
import lovasz_reference as LV

KINDS = ('empty', 'full', 'first', 'last', 'plane', 'random', 'unknown', 'only_unknown')


# ------------------------------------------------------------------------------------------------ the transform
@pytest.mark.parametrize('shape', [(6, 5, 4), (1, 1, 1), (4, 1, 6), (3, 5, 2)], ids=str)
def test_separable_transform_equals_the_definition(shape):
    for kind in KINDS:
        g = E.scene(kind, shape, seed=3)
        for cap in (1, 2, 9, 25, E.full_cap(shape), E.full_cap(shape) + 7):
            want = E.edt2_brute(g, cap)
            assert np.array_equal(E.edt2(g, cap), want), (kind, cap)
            if not E.occupied(g).any():
                assert (want == cap).all()
    # frames are independent: a stack equals its frames one by one
    stack = np.stack([E.scene(k, shape, seed=5) for k in ('random', 'empty', 'unknown')])
    assert np.array_equal(E.edt2(stack, 9), np.stack([E.edt2_brute(g, 9) for g in stack]))


@pytest.mark.parametrize('shape', [(5, 7, 3), (33, 17, 9), (48, 48, 16)], ids=str)
def test_transform_equals_scipy(shape):
    ndi = pytest.importorskip('scipy.ndimage')
    g = E.scene('random', shape, seed=11)
    g[E.scene('unknown', shape, seed=12) == 255] = 255
    exact = np.rint(ndi.distance_transform_edt(~E.occupied(g)) ** 2).astype(np.int64)
    assert np.array_equal(E.edt2(g, E.full_cap(shape)), exact)
    for T in (1, 3, 5):
        assert np.array_equal(E.edt2(g, T * T), np.minimum(exact, T * T))
    assert (E.edt2(np.zeros(shape, np.uint8), 17) == 17).all()


# ------------------------------------------------------------------------------------------------ loss and gradient
def _small_case(seed=0):
    rng = np.random.default_rng(seed)
    shape = (6, 5, 4)
    labels = np.stack([E.scene('random', shape, seed=1), E.scene('unknown', shape, seed=2), np.zeros(shape, np.uint8)])
    labels[0, 2, 2, 1] = 4
    logits = (2 * rng.standard_normal((3, 3, *shape))).astype(np.float32)
    return logits, labels


def test_gradient_equals_central_differences():
    logits, labels = _small_case()
    T = 3
    ref = E.loss_and_grad(logits, labels, T, E.WEIGHT)
    assert ref['n_g'][2] == 0 and (ref['n_g'][:2] > 0).all() and (labels[1] == 255).any()
    assert E.occupied(ref['pred']).any() and ref['loss'] > 0
    z = logits.astype(np.float64)
    h = 1e-6
    flat = np.arange(0, z.size, 7)
    for i in flat:
        at = np.unravel_index(i, z.shape)
        up, down = z.copy(), z.copy()
        up[at] += h
        down[at] -= h
        fd = (E.loss_and_grad(up, labels, T, E.WEIGHT, pred=ref['pred'])['loss'] - E.loss_and_grad(down, labels, T, E.WEIGHT, pred=ref['pred'])['loss']) / (2 * h)
        assert abs(fd - ref['dlogits'][at]) <= 1e-7, (at, fd, ref['dlogits'][at])
    assert not ref['dlogits'][2].any()                                            # the frame without a label cell
    assert not np.moveaxis(ref['dlogits'], 1, 0)[:, labels == 255].any()         # 255 cells are inert
    assert np.abs(ref['dlogits'][:2]).max() > 1e-4


def test_hard_predictions_give_the_truncated_chamfer_sum():
    """saturated logits: p is 0 or 1 in float32 (within e^-30 of it in float64), the loss is the hard-set expression formed from the
    transforms alone"""
    logits, labels = _small_case(seed=4)
    logits = E.saturated(logits)
    for T in (1, 3, 20):
        ref = E.loss_and_grad(logits, labels, T, E.WEIGHT)
        low = E.loss_and_grad(logits, labels, T, E.WEIGHT, dtype=np.float32)
        assert set(np.unique(low['p']).tolist()) == {0.0, 1.0} and np.array_equal(low['p'] == 1, E.occupied(ref['pred']))
        hard = E.hard_loss(ref['edt_label'], ref['edt_pred'], labels, ref['pred'], T, E.WEIGHT)
        assert hard > 0 and abs(ref['loss'] - hard) <= 1e-9 * hard          # 120 cells x 2 e^-30 = 2e-11 in float64


def test_no_label_cell_gives_zero_loss_and_gradient():
    logits, _ = _small_case()
    labels = np.stack([np.zeros((6, 5, 4), np.uint8), np.full((6, 5, 4), 255, np.uint8), np.zeros((6, 5, 4), np.uint8)])
    ref = E.loss_and_grad(logits, labels, 3, E.WEIGHT)
    assert ref['loss'] == 0 and not ref['dlogits'].any() and not ref['n_g'].any()


# ------------------------------------------------------------------------------------------------ the metric
def test_metric_counts_on_a_hand_made_pair():
    """one label cell at (0,0,0), predictions at (0,0,0) and (3,4,0): edt2_G = 0 and 25, edt2_P = 0"""
    lab, pred = np.zeros((1, 6, 6, 2), np.uint8), np.zeros((1, 6, 6, 2), np.uint8)
    lab[0, 0, 0, 0] = 1
    pred[0, 0, 0, 0] = 1
    pred[0, 3, 4, 0] = 2
    counts, sums, n = E.cd_counts(lab, pred, [24, 25, 400])
    assert counts.tolist() == [1, 0, 2, 1, 1, 2, 2, 1, 1, 1] and sums.tolist() == [5.0, 0.0] and n == 3
    empty = np.zeros_like(lab)
    assert E.cd_counts(np.concatenate([lab, empty, lab]), np.concatenate([empty, pred, np.full_like(pred, 255)]), [1, 2, 3])[0].tolist() == [0, 3] + [0] * 8
    assert E.thresholds2(0.2) == [25, 100, 400]


def test_summarise_on_hand_written_counts():
    from muvo_amd.voxel_view import VoxelDistanceMetric, cd_thresholds2
    assert cd_thresholds2(0.2) == [25, 100, 400] and cd_thresholds2(0.5) == [4, 16, 64]
    counts = [[3, 1, 10, 20, 5, 8, 10, 4, 10, 20], [0, 2, 0, 0, 0, 0, 0, 0, 0, 0]]
    sums = [[30.0, 10.0], [0.0, 0.0]]
    out = VoxelDistanceMetric.summarise(counts, sums, 0.2)
    assert out['voxel_cd'] == pytest.approx(0.2 * (3.0 + 0.5), abs=1e-15)
    assert (out['voxel_precision_1m'], out['voxel_precision_2m'], out['voxel_precision_4m']) == (0.5, 0.8, 1.0)
    assert (out['voxel_recall_1m'], out['voxel_recall_2m'], out['voxel_recall_4m']) == (0.2, 0.5, 1.0)
    assert out['voxel_fscore_1m'] == pytest.approx(2 * 0.5 * 0.2 / 0.7, abs=1e-15) and out['voxel_fscore_4m'] == 1.0
    assert out['voxel_cd_frames'] == 3 and out['voxel_cd_skipped'] == 1
    names = ['voxel_cd', 'voxel_cd_frames', 'voxel_cd_skipped'] + [f'voxel_{k}_{t}m' for k in ('precision', 'recall', 'fscore') for t in (1, 2, 4)]
    assert set(out) == {n + tail for n in names for tail in ('', '_imagine')}
    # zero denominators give 0.0
    assert out['voxel_cd_imagine'] == 0.0 and out['voxel_cd_frames_imagine'] == 0 and out['voxel_cd_skipped_imagine'] == 2
    assert all(out[f'voxel_{k}_{t}m_imagine'] == 0.0 for k in ('precision', 'recall', 'fscore') for t in (1, 2, 4))
    none = VoxelDistanceMetric.summarise([[1, 0, 4, 4, 0, 0, 0, 0, 0, 0]] * 2, [[9.0, 9.0]] * 2, 0.2)
    assert none['voxel_fscore_1m'] == 0.0 and none['voxel_precision_1m'] == 0.0           # P + R = 0
    m = VoxelDistanceMetric(types.SimpleNamespace(VOXEL=types.SimpleNamespace(RESOLUTION=0.2)))
    m.start_loader(1)
    assert m.result()['test1_voxel_cd'] == 0.0 and m.result()['test1_voxel_cd_frames_imagine'] == 0


# ------------------------------------------------------------------------------------------------ configuration
KEYS = ('LOSSES.VOXEL_BOUNDARY', 'LOSSES.VOXEL_BOUNDARY.WEIGHT', 'LOSSES.VOXEL_BOUNDARY.FACTORS', 'LOSSES.VOXEL_BOUNDARY.TRUNCATE_M')


def test_defaults_do_not_carry_the_key():
    from muvo_amd import config
    cfg = config.get_cfg()
    assert 'VOXEL_BOUNDARY' not in cfg.LOSSES and 'VOXEL_BOUNDARY' not in config.base_1d_cfg().LOSSES
    assert config.voxel_boundary(cfg) == (0.0, (1, 2, 4), 4.0)
    assert config.DEFAULT_VOXEL_BOUNDARY_FACTORS == (1, 2, 4) and config.DEFAULT_VOXEL_BOUNDARY_TRUNCATE_M == 4.0
    assert [config.voxel_boundary_cells(cfg, 4.0, f) for f in (1, 2, 4)] == [20, 10, 5]
    assert config.voxel_boundary_cells(cfg, 0.05, 4) == 1
    import glob
    import yaml
    for path in glob.glob(config.os.path.join(config._HERE, 'configs', '*.yml')):
        assert 'VOXEL_BOUNDARY' not in open(path).read(), path
    assert 'VOXEL_BOUNDARY' not in yaml.safe_dump(config.base_1d_cfg().convert_to_dict())
    for key in KEYS:
        assert key in config.EXTENSION_KEYS


def test_key_round_trips_through_yaml_dict_and_override(tmp_path):
    from muvo_amd import config
    y = tmp_path / 'bd.yml'
    y.write_text('VOXEL_SEG: {ENABLED: true}\nLOSSES:\n  VOXEL_BOUNDARY: {WEIGHT: 0.5, FACTORS: [2, 4], TRUNCATE_M: 2.0}\n')
    cfg = config.get_cfg(argparse.Namespace(config_file=str(y), opts=[]))
    assert config.voxel_boundary(cfg) == (0.5, (2, 4), 2.0) and config.voxel_lovasz(cfg)[0] == 0.0
    assert cfg.convert_to_dict()['LOSSES']['VOXEL_BOUNDARY'] == {'WEIGHT': 0.5, 'FACTORS': [2, 4], 'TRUNCATE_M': 2.0}
    again = config.get_cfg(cfg_dict=cfg.convert_to_dict())                   # the dict a checkpoint carries
    assert config.voxel_boundary(again) == (0.5, (2, 4), 2.0)
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_BOUNDARY': {'WEIGHT': 2}}})
    assert config.voxel_boundary(cfg) == (2.0, (1, 2, 4), 4.0)
    cfg = config.get_cfg(argparse.Namespace(config_file='', opts=['VOXEL_SEG.ENABLED', 'True', 'LOSSES.VOXEL_BOUNDARY.WEIGHT', '0.25',
                                                                  'LOSSES.VOXEL_BOUNDARY.FACTORS', '[4]', 'LOSSES.VOXEL_BOUNDARY.TRUNCATE_M', '3']))
    assert config.voxel_boundary(cfg) == (0.25, (4,), 3.0)
    with pytest.raises(KeyError):
        config.get_cfg().merge_from_list(['LOSSES.VOXEL_BOUNDRY.WEIGHT', '1'])
    with pytest.raises(KeyError):
        config.get_cfg().merge_from_list(['LOSSES.VOXEL_BOUNDARY.STRIDE', '1'])


@pytest.mark.parametrize('factors', [[3], [2, 8], [0], [2, 2], 2, [True]], ids=str)
def test_bad_factors_raise(factors):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_BOUNDARY': {'WEIGHT': 1.0, 'FACTORS': factors}}})
    with pytest.raises(ValueError, match='LOSSES.VOXEL_BOUNDARY.FACTORS must be a list of distinct factors drawn from 1, 2, 4'):
        config.voxel_boundary(cfg)


@pytest.mark.parametrize('truncate', [0, -1.0, True, 'far', None], ids=str)
def test_bad_truncation_raises(truncate):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_BOUNDARY': {'WEIGHT': 1.0, 'TRUNCATE_M': truncate}}})
    with pytest.raises(ValueError, match='LOSSES.VOXEL_BOUNDARY.TRUNCATE_M must be a number > 0'):
        config.voxel_boundary(cfg)


def test_bad_weight_and_disabled_head_raise():
    from muvo_amd import config
    with pytest.raises(ValueError, match='LOSSES.VOXEL_BOUNDARY.WEIGHT > 0 needs VOXEL_SEG.ENABLED: the loss is on the voxel head'):
        config.voxel_boundary(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_BOUNDARY': {'WEIGHT': 1.0}}}))
    assert config.voxel_boundary(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_BOUNDARY': {'WEIGHT': 0.0}}}))[0] == 0.0
    for w in (-1.0, 'much', True):
        with pytest.raises(ValueError, match='LOSSES.VOXEL_BOUNDARY.WEIGHT must be a number >= 0'):
            config.voxel_boundary(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_BOUNDARY': {'WEIGHT': w}}}))
    # the texts of voxel_render, word for word, with the key's name in place
    with pytest.raises(ValueError) as a:
        config.voxel_render(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': 1.0, 'FACTORS': [3]}}}))
    with pytest.raises(ValueError) as b:
        config.voxel_boundary(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_BOUNDARY': {'WEIGHT': 1.0, 'FACTORS': [3]}}}))
    assert str(b.value) == str(a.value).replace('VOXEL_RENDER', 'VOXEL_BOUNDARY')


# ------------------------------------------------------------------------------------------------ the trainer's wiring
def test_compute_loss_key_set_with_and_without_the_key(monkeypatch):
    """the kernels stubbed out: without the key today's terms and no call; with it one call per configured factor, after every other
    term, on the head's tensors and the tensor voxel_target names, weight WEIGHT / f, 20 / 10 / 5 cells at the defaults"""
    from muvo_amd import ops
    from muvo_amd.trainer import WorldModelTrainer
    calls = []
    monkeypatch.setattr(ops, 'voxel_losses', lambda logits, target, weight, cw=None, terms=False: tuple(torch.zeros(()) for _ in range(3)))
    monkeypatch.setattr(ops, 'voxel_lovasz_loss', lambda logits, labels, weight, terms=False: (torch.zeros(()),))

    def boundary(logits, labels, truncate_cells, weight, terms=False):
        calls.append((logits, labels, truncate_cells, weight, terms))
        return (torch.zeros(()),)
    monkeypatch.setattr(ops, 'voxel_boundary_loss', boundary)
    batch, output = LV.voxel_dicts(sizes=((8, 8, 4), (4, 4, 2), (2, 2, 1)), b=1, s=1, C=2)
    for f in (1, 2, 4):
        batch[f'voxel_visible_label_{f}'] = torch.full_like(batch[f'voxel_label_{f}'], 255)
    today = [f'{name}_{f}' for f in (1, 2, 4) for name in ('voxel', 'sem_scal', 'geo_scal')]
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=LV.voxel_only_cfg()), batch, output)
    assert list(losses) == today and not calls
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_BOUNDARY.WEIGHT': 0.5, 'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5})
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
    assert list(losses) == today + [f'voxel_lovasz_{f}' for f in (1, 2, 4)] + [f'voxel_boundary_{f}' for f in (1, 2, 4)]
    for k, (f, cells) in enumerate(((1, 20), (2, 10), (4, 5))):
        logits, labels, truncate_cells, weight, terms = calls[k]
        assert logits is output[f'voxel_{f}'] and labels is batch[f'voxel_label_{f}'] and terms is True
        assert weight == 0.5 * (1 / f) and truncate_cells == cells and isinstance(truncate_cells, int)
    del calls[:]
    # with the visibility mask on the term reads the masked labels, as the Lovasz term does
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_BOUNDARY.WEIGHT': 2.0, 'LOSSES.VOXEL_BOUNDARY.FACTORS': [2], 'LOSSES.VOXEL_BOUNDARY.TRUNCATE_M': 1.0,
                               'VOXEL_SEG.VISIBILITY.ENABLED': True})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today + ['voxel_boundary_2']
    assert calls[0][0] is output['voxel_2'] and calls[0][1] is batch['voxel_visible_label_2'] and calls[0][2] == 2 and calls[0][3] == 1.0
    del calls[:]
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_BOUNDARY.WEIGHT': 0.0})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today and not calls


def test_module_guards():
    from muvo_amd.losses import BoundaryLoss
    crit = BoundaryLoss(3)
    with pytest.raises(ValueError, match='Expected 6-D logits and labels'):
        crit(torch.zeros(1, 2, 5, 4), torch.zeros(1, 2, 5, 4))
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match='truncate_cells must be an integer >= 1'):
            BoundaryLoss(bad)


def test_predict_refuses_the_flag_outside_mode_test():
    from muvo_amd import predict as P
    with pytest.raises(SystemExit, match='--voxel-cd'):
        P.parse_args(['--config-file', 'x.yml', '--out', 'o', '--mode', 'sim', '--voxel-cd'])
    assert P.parse_args(['--config-file', 'x.yml', '--out', 'o', '--mode', 'test', '--voxel-cd']).voxel_cd is True
    # the voxel head off: refused before a batch is touched, as the ray IoU is
    module = types.SimpleNamespace(panel_writer=None, traj_panels=False, traj_options={}, flow_panels=False, voxel_panels=False, voxel_options={})
    cfg = LV.voxel_only_cfg(**{'VOXEL_SEG.ENABLED': False})
    with pytest.raises(ValueError, match='the voxel Chamfer distance needs the voxel head'):
        P._run_test(cfg, module, {}, 'unused', None, 500, 0, None, print, voxel_cd={})


# ------------------------------------------------------------------------------------------------ the entries' argument checks
def test_entry_points_validate_before_touching_the_device():
    """bad arguments come back as MUVO_ERR_INVALID_ARG with a message; nothing is launched (this runs without a GPU)"""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    p, null = C.c_void_p(256), C.c_void_p(0)      # never dereferenced: every call below is rejected by its argument checks
    i64, st, w = C.c_int64, C.c_void_p(0), C.c_float(1.0)
    assert L.muvo_voxel_edt_ws_bytes(i64(3), 13, 10, 7) == 3 * 910 * 4
    for bad in ((0, 13, 10, 7), (65536, 13, 10, 7), (3, 0, 10, 7), (3, 13, 10, -1), (1, 46341, 1, 1), (1, 32768, 32768, 1), (4096, 2048, 2048, 4)):
        assert L.muvo_voxel_edt_ws_bytes(i64(bad[0]), *bad[1:]) == -1, bad
    assert L.muvo_voxel_edt_ws_bytes(i64(1), 46340, 1, 1) == 46340 * 4

    def edt(F=3, X=13, Y=10, Z=7, cap=9, grid=p, ws=p, wsb=3 * 910 * 4, out=p):
        return L.muvo_voxel_edt(grid, i64(F), X, Y, Z, C.c_int32(cap), ws, i64(wsb), out, st)
    for kw, msg in (({'cap': 0}, b'cap 0 below 1'), ({'cap': -4}, b'below 1'), ({'X': 0}, b'every axis >= 1'), ({'F': 0}, b'1..65535 frames'),
                    ({'Z': 46341}, b'2^31'), ({'grid': null}, b'null pointer'), ({'out': null}, b'null pointer'), ({'ws': null}, b'null pointer'),
                    ({'wsb': 3 * 910 * 4 - 1}, b'workspace'), ({'out': C.c_void_p(258)}, b'workspace')):
        assert edt(**kw) == -1 and msg in L.muvo_last_error(), (kw, L.muvo_last_error())
    V = 910
    need = L.muvo_voxel_boundary_ws_bytes(i64(3), i64(V))
    assert need >= 3 * 12 and L.muvo_voxel_boundary_ws_bytes(i64(0), i64(V)) == -1 and L.muvo_voxel_boundary_ws_bytes(i64(3), i64(1 << 30)) == -1

    def fwd(F=3, Cn=9, X=13, Y=10, Z=7, T=3, logits=p, labels=p, eg=p, ep=p, ws=p, wsb=need, ng=p, loss=p):
        return L.muvo_voxel_boundary_forward(logits, labels, eg, ep, i64(F), Cn, X, Y, Z, T, w, ws, i64(wsb), ng, loss, st)

    def bwd(F=3, Cn=9, X=13, Y=10, Z=7, T=3, logits=p, labels=p, eg=p, ep=p, ng=p, gout=p, dl=p):
        return L.muvo_voxel_boundary_backward(logits, labels, eg, ep, ng, i64(F), Cn, X, Y, Z, T, w, gout, dl, st)
    for call in (fwd, bwd):
        for kw, msg in (({'Cn': 1}, b'2..16'), ({'Cn': 17}, b'2..16'), ({'F': 0}, b'65535'), ({'X': 2049}, b'2048'), ({'Z': 0}, b'2048'),
                        ({'T': 0}, b'truncation'), ({'T': 46341}, b'truncation'), ({'logits': null}, b'null pointer'), ({'labels': null}, b'null pointer'),
                        ({'eg': null}, b'null pointer'), ({'ep': null}, b'null pointer'), ({'ng': null}, b'null pointer'), ({'eg': C.c_void_p(258)}, b'4-byte')):
            assert call(**kw) == -1 and msg in L.muvo_last_error(), (call.__name__, kw, L.muvo_last_error())
    for kw, msg in (({'ws': null}, b'workspace'), ({'wsb': need - 1}, b'workspace'), ({'ws': C.c_void_p(264)}, b'workspace'), ({'loss': null}, b'null pointer')):
        assert fwd(**kw) == -1 and msg in L.muvo_last_error()
    for kw in ({'gout': null}, {'dl': null}):
        assert bwd(**kw) == -1 and b'voxel_boundary_backward: null pointer' in L.muvo_last_error()
    cdn = L.muvo_voxel_cd_ws_bytes(i64(3), i64(V))
    assert cdn == 3 * 16 and L.muvo_voxel_cd_ws_bytes(i64(3), i64(8193)) == 3 * 32 and L.muvo_voxel_cd_ws_bytes(i64(3), i64(0)) == -1
    thr = (C.c_int32 * 3)(25, 100, 400)

    def cd(F=3, X=13, Y=10, Z=7, label=p, pred=p, eg=p, ep=p, t=thr, counts=p, sums=p, ws=p, wsb=cdn):
        return L.muvo_voxel_cd_counts(label, pred, eg, ep, i64(F), X, Y, Z, t, counts, sums, ws, i64(wsb), st)
    for kw, msg in (({'F': 0}, b'65535'), ({'Y': 2049}, b'2048'), ({'label': null}, b'null pointer'), ({'pred': null}, b'null pointer'),
                    ({'counts': null}, b'null pointer'), ({'sums': null}, b'null pointer'), ({'t': (C.c_int32 * 3)(1, -1, 4)}, b'negative'),
                    ({'ws': null}, b'workspace'), ({'wsb': cdn - 1}, b'workspace'), ({'counts': C.c_void_p(260)}, b'8-byte')):
        assert cd(**kw) == -1 and msg in L.muvo_last_error(), (kw, L.muvo_last_error())
