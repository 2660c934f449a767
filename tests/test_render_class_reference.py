"""CPU: the restatement of the rendered first-hit class loss (tests/render_class_reference.py) - its cell sequence and target class
against the march of raycast_reference, its masses and gradient against torch float64 autograd through cumprod, the formula for
dS_y/dz and central differences, four closed forms - the configuration surface of the extension key LOSSES.VOXEL_RENDER_CLASS,
the trainer's wiring with stubs and the argument checks of the entries."""
import argparse
import math
import types

import numpy as np
import pytest
import torch

import lovasz_reference as LV
import raycast_reference as RC
import render_class_reference as K
import render_reference as R

ORIGIN = (3.5, 5.0, 3.5)


def _rays(g):
    hand = np.array([r for _, r, _ in RC.hand_rays(g)], np.float32)
    return np.concatenate([RC.fan_rays(ORIGIN, 8, 32, 10.0, -30.0), hand, RC.camera_rays(RC.X, RC.Y, RC.Z, RC.R)[::7]])


def _case(C, seed=0):
    scenes = [R.clip_classes(g, C) for g in (RC.scene(), RC.shifted(RC.scene()), np.zeros((RC.X, RC.Y, RC.Z), np.uint8))]
    return R.frames(scenes, C, seed), np.stack(scenes), _rays(RC.scene())


# ------------------------------------------------------------------------------------------------ the cell sequence and the target
def test_cell_sequence_and_target_class_are_the_march_of_raycast_reference():
    """every cell of a sequence, occupied alone with a class of its own, is what raycast_reference.march hits and the class the
    restatement reads there; on a scene the target class is the class at the first hit of the march, 0 at a miss, -1 at an invalid
    ray and at a class the head does not have"""
    g = R.clip_classes(RC.scene(), 9)
    rays = _rays(g)
    tab = R.cell_table(g.shape, rays)
    for r in range(0, len(rays), 5):
        if not tab['valid'][r]:
            assert RC.march(np.ones_like(g), rays[r])[0] < 0 and K.target_class(np.ones_like(g), tab, 9)[r] == -1
            continue
        for k in range(int(tab['n'][r])):
            one = np.zeros(g.size, np.uint8)
            one[tab['cells'][r, k]] = 1 + k % 8
            idx, _, _ = RC.march(one.reshape(g.shape), rays[r])
            assert idx == tab['cells'][r, k] and K.target_class(one.reshape(g.shape), tab, 9)[r] == 1 + k % 8, (r, k)
    hit, _, _ = RC.cast(g, rays)
    y = K.target_class(g, tab, 9)
    want = np.where(tab['valid'], np.where(hit >= 0, g.reshape(-1).astype(np.int64)[np.maximum(hit, 0)], 0), -1)
    assert np.array_equal(y, want) and (y > 0).sum() >= 100 and (y == 0).sum() >= 5 and len(set(y[y > 0].tolist())) >= 4
    few = K.target_class(g, tab, 3)                                               # a head with 3 classes: classes 3..8 are ignored
    assert np.array_equal(few, np.where(want >= 3, -1, want)) and (few != y).any()


# ------------------------------------------------------------------------------------------------ masses and gradient
def _autograd(logits, labels, rays, weight):
    """the definition through torch float64 autograd: softmax, cumprod, gather, log"""
    tab = R.cell_table(logits.shape[2:], rays)
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    F, C = z.shape[:2]
    cells = torch.from_numpy(tab['cells'])
    pad, idx = cells < 0, cells.clamp(min=0)
    valid = torch.from_numpy(tab['valid'])
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    total, Ss = 0.0, []
    for f in range(F):
        p = torch.softmax(z[f].reshape(C, -1), 0)
        qk = torch.where(pad, one, p[0][idx])
        T = torch.cat([torch.ones(len(qk), 1, dtype=torch.float64), torch.cumprod(qk, 1)], 1)
        y = torch.from_numpy(K.target_class(labels[f], tab, C))
        py = torch.where(pad, zero, p[y.clamp(min=0)[:, None], idx])
        S = torch.where(y == 0, T[:, -1], (T[:, :-1] * py).sum(1))
        live = valid & (y >= 0)
        total = total + (-torch.log((S + K.EPS) / (1 + K.EPS)))[live].sum() / int(valid.sum())
        Ss.append(torch.where(live, S, zero))
    loss = weight * total / F
    grad, = torch.autograd.grad(loss, z)
    return loss.item(), grad.numpy(), torch.stack(Ss).detach().numpy()


@pytest.mark.parametrize('C', [2, 9])
def test_gradient_equals_autograd_and_the_masses_add_up_to_one(C):
    logits, labels, rays = _case(C)
    ref = K.loss_and_grad(logits, labels, rays, K.WEIGHT)                       # asserts sum_c S_c = 1 to 1e-12 itself
    loss, grad, S = _autograd(logits, labels, rays, K.WEIGHT)
    assert abs(ref['loss'] - loss) <= 1e-13 * abs(loss)
    assert np.abs(ref['S'] - S).max() <= 1e-13
    scale = np.abs(grad).max()
    assert scale > 0 and np.abs(ref['dlogits'] - grad).max() <= 1e-13 * scale
    _, _, p = R.occupancy(logits[0].reshape(C, -1))
    total = K.masses(p, ref['table']).sum(0)
    assert np.abs(total - 1)[ref['table']['valid']].max() <= 1e-12 and not total[~ref['table']['valid']].any()
    unseen = ref['visits'].reshape(3, *logits.shape[2:]) == 0
    assert unseen.any() and not np.moveaxis(ref['dlogits'], 1, 0)[:, unseen].any()            # no ray, no gradient
    assert (ref['y'][2][ref['table']['valid']] == 0).all() and len(set(ref['y'][0].tolist())) >= min(C, 4)


def test_accumulator_form_equals_the_formula_for_ds_dz():
    logits, labels, rays = _case(9, seed=2)
    ref = K.loss_and_grad(logits, labels, rays, K.WEIGHT)
    direct = K.direct_gradient(logits, labels, rays, K.WEIGHT, table=ref['table'])
    assert np.abs(ref['dlogits'] - direct).max() <= 1e-13 * np.abs(direct).max()


def test_gradient_equals_central_differences():
    logits, labels, rays = _case(9, seed=1)
    tab = R.cell_table(logits.shape[2:], rays)
    ref = K.loss_and_grad(logits, labels, rays, K.WEIGHT, table=tab)
    z = logits.astype(np.float64)
    order = np.argsort(-np.abs(ref['dlogits']).reshape(-1))[:12]                 # the largest entries, where a difference resolves
    h = 1e-6
    for flat in order:
        at = np.unravel_index(flat, z.shape)
        up, down = z.copy(), z.copy()
        up[at] += h
        down[at] -= h
        fd = (K.loss_and_grad(up, labels, rays, K.WEIGHT, table=tab)['loss'] - K.loss_and_grad(down, labels, rays, K.WEIGHT, table=tab)['loss']) / (2 * h)
        assert abs(fd - ref['dlogits'][at]) <= 1e-7 * max(1.0, abs(fd)), (at, fd, ref['dlogits'][at])


# ------------------------------------------------------------------------------------------------ closed forms
def test_constant_logits_render_one_minus_two_to_the_minus_n():
    """C = 2, equal logits, the label full of class 1: p_1 = q = 1/2, so S_1 = sum 2^-(k+1) = 1 - 2^-n"""
    g = RC.scene()
    rays = _rays(g)
    ref = K.loss_and_grad(np.full((1, 2, *g.shape), 0.75, np.float32), np.ones((1, *g.shape), np.uint8), rays, 1.0)
    tab = ref['table']
    v = tab['valid']
    assert (ref['y'][0][v] == 1).all() and np.array_equal(ref['S'][0][v], 1 - 2.0 ** -tab['n'][v]) and not ref['S'][0][~v].any()


def test_confidently_empty_costs_nothing_where_the_label_misses():
    g = RC.scene()
    rays = _rays(g)
    logits = np.zeros((1, 9, *g.shape), np.float32)
    logits[:, 0] = 60.0
    empty = K.loss_and_grad(logits, np.zeros((1, *g.shape), np.uint8), rays, 1.0)
    assert empty['cost'].max() <= 1e-12 and 0 <= empty['loss'] <= 1e-12
    ref = K.loss_and_grad(logits, R.clip_classes(g, 9)[None], rays, 1.0)
    miss = ref['table']['valid'] & (ref['y'][0] == 0)
    assert miss.any() and ref['cost'][0][miss].max() <= 1e-12 and ref['loss'] > 1.0      # the rays that hit the label are charged


def test_confident_correct_prediction_renders_one_minus_the_mass_before_the_hit():
    """the label's class favoured by 40 in every cell: S_y = 1 - (the mass of the cells before the label's hit), both from the
    restatement: the first is the sum over the target class, the second the other classes' masses and the exit"""
    g = R.clip_classes(RC.scene(), 9)
    rays = _rays(g)
    logits = np.zeros((1, 9, *g.shape), np.float32)
    logits[(0, g.astype(np.int64), *np.indices(g.shape))] = 40.0
    ref = K.loss_and_grad(logits, g[None], rays, 1.0)
    _, _, p = R.occupancy(logits[0].reshape(9, -1))
    S = K.masses(p, ref['table'])
    y = ref['y'][0]
    hit = ref['table']['valid'] & (y >= 1)
    assert hit.sum() >= 100
    for r in np.flatnonzero(hit):
        before = S[:, r].sum() - S[y[r], r]
        assert abs(ref['S'][0][r] - (1 - before)) <= 1e-12 and before <= 300 * 9 * math.exp(-40)
    assert ref['loss'] <= 1e-12 + 300 * 9 * math.exp(-40) * 2


def test_all_mass_on_a_wrong_class_costs_log_one_plus_eps_over_eps():
    g = RC.scene()
    rays = _rays(g)
    logits = np.zeros((1, 3, *g.shape), np.float32)
    logits[:, 2] = 2000.0                                                        # p_2 = 1, p_0 = p_1 = 0 exactly: S_1 = 0, T_n = 0
    ones = K.loss_and_grad(logits, np.ones((1, *g.shape), np.uint8), rays, 1.0)
    none = K.loss_and_grad(logits, np.zeros((1, *g.shape), np.uint8), rays, 1.0)
    want = math.log((1 + K.EPS) / K.EPS)
    for ref, y in ((ones, 1), (none, 0)):
        v = ref['table']['valid']
        assert (ref['y'][0][v] == y).all() and not ref['S'][0].any()
        assert np.array_equal(ref['cost'][0][v], np.full(v.sum(), -math.log(K.EPS / (1 + K.EPS)))) and abs(ref['loss'] - want) <= 1e-14
        assert np.isfinite(ref['dlogits']).all()
    assert abs(want - math.log(1025)) <= 1e-15


def test_no_valid_ray_gives_zero_loss_and_gradient():
    logits, labels, _ = _case(2)
    rays = np.array([[-3.0, -3.0, 20.0, -1, 0, 0.5, np.inf], [2.5, 3.5, 9.0, np.nan, 0, -1, np.inf], [1, 1, 1, 0, 0, 0, np.inf]], np.float32)
    ref = K.loss_and_grad(logits, labels, rays, K.WEIGHT)
    assert ref['n_valid'] == 0 and ref['loss'] == 0 and not ref['dlogits'].any() and np.isfinite(ref['dlogits']).all()
    assert (ref['y'] == -1).all()


# ------------------------------------------------------------------------------------------------ configuration
def test_defaults_do_not_carry_the_key():
    from muvo_amd import config
    cfg = config.get_cfg()
    assert 'VOXEL_RENDER_CLASS' not in cfg.LOSSES and 'VOXEL_RENDER_CLASS' not in config.base_1d_cfg().LOSSES
    assert config.voxel_render_class(cfg) == (0.0, config.DEFAULT_VOXEL_RENDER_CLASS_FACTORS, config.DEFAULT_VOXEL_RENDER_CLASS_STRIDE)
    assert config.DEFAULT_VOXEL_RENDER_CLASS_FACTORS == (1, 2, 4) and config.DEFAULT_VOXEL_RENDER_CLASS_STRIDE == 1
    import glob
    import yaml
    for path in glob.glob(config.os.path.join(config._HERE, 'configs', '*.yml')):
        assert 'VOXEL_RENDER_CLASS' not in open(path).read(), path
    assert 'VOXEL_RENDER_CLASS' not in yaml.safe_dump(config.base_1d_cfg().convert_to_dict())
    for key in ('LOSSES.VOXEL_RENDER_CLASS', 'LOSSES.VOXEL_RENDER_CLASS.WEIGHT', 'LOSSES.VOXEL_RENDER_CLASS.FACTORS', 'LOSSES.VOXEL_RENDER_CLASS.STRIDE'):
        assert key in config.EXTENSION_KEYS


def test_key_round_trips_through_yaml_dict_and_override(tmp_path):
    from muvo_amd import config
    y = tmp_path / 'rc.yml'
    y.write_text('VOXEL_SEG: {ENABLED: true}\nLOSSES:\n  VOXEL_RENDER_CLASS: {WEIGHT: 0.5, FACTORS: [2, 4], STRIDE: 4}\n')
    cfg = config.get_cfg(argparse.Namespace(config_file=str(y), opts=[]))
    assert config.voxel_render_class(cfg) == (0.5, (2, 4), 4) and config.voxel_render(cfg)[0] == 0.0
    assert cfg.convert_to_dict()['LOSSES']['VOXEL_RENDER_CLASS'] == {'WEIGHT': 0.5, 'FACTORS': [2, 4], 'STRIDE': 4}
    again = config.get_cfg(cfg_dict=cfg.convert_to_dict())                   # the dict a checkpoint carries
    assert config.voxel_render_class(again) == (0.5, (2, 4), 4)
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER_CLASS': {'WEIGHT': 2}}})
    assert config.voxel_render_class(cfg) == (2.0, (1, 2, 4), 1)
    cfg = config.get_cfg(argparse.Namespace(config_file='', opts=['VOXEL_SEG.ENABLED', 'True', 'LOSSES.VOXEL_RENDER_CLASS.WEIGHT', '0.25',
                                                                  'LOSSES.VOXEL_RENDER_CLASS.FACTORS', '[4]', 'LOSSES.VOXEL_RENDER_CLASS.STRIDE', '2']))
    assert config.voxel_render_class(cfg) == (0.25, (4,), 2)
    with pytest.raises(KeyError):
        config.get_cfg().merge_from_list(['LOSSES.VOXEL_RENDER_CLAS.WEIGHT', '1'])


@pytest.mark.parametrize('factors', [[3], [2, 8], [0], [2, 2], 2, [True]], ids=str)
def test_bad_factors_raise(factors):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER_CLASS': {'WEIGHT': 1.0, 'FACTORS': factors}}})
    with pytest.raises(ValueError, match='LOSSES.VOXEL_RENDER_CLASS.FACTORS must be a list of distinct factors drawn from 1, 2, 4'):
        config.voxel_render_class(cfg)


@pytest.mark.parametrize('stride', [0, -1, 1.5, True, 'four'], ids=str)
def test_bad_stride_raises(stride):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER_CLASS': {'WEIGHT': 1.0, 'STRIDE': stride}}})
    with pytest.raises(ValueError, match='LOSSES.VOXEL_RENDER_CLASS.STRIDE must be an integer >= 1'):
        config.voxel_render_class(cfg)


def test_bad_weight_and_disabled_head_raise():
    from muvo_amd import config
    with pytest.raises(ValueError, match='LOSSES.VOXEL_RENDER_CLASS.WEIGHT > 0 needs VOXEL_SEG.ENABLED: the loss is on the voxel head'):
        config.voxel_render_class(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_RENDER_CLASS': {'WEIGHT': 1.0}}}))
    assert config.voxel_render_class(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_RENDER_CLASS': {'WEIGHT': 0.0}}}))[0] == 0.0
    for w in (-1.0, 'much', True):
        with pytest.raises(ValueError, match='LOSSES.VOXEL_RENDER_CLASS.WEIGHT must be a number >= 0'):
            config.voxel_render_class(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER_CLASS': {'WEIGHT': w}}}))
    # the texts of voxel_render, word for word, with the key's name in place
    with pytest.raises(ValueError) as a:
        config.voxel_render(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': 1.0, 'STRIDE': 0}}}))
    with pytest.raises(ValueError) as b:
        config.voxel_render_class(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER_CLASS': {'WEIGHT': 1.0, 'STRIDE': 0}}}))
    assert str(b.value) == str(a.value).replace('VOXEL_RENDER', 'VOXEL_RENDER_CLASS')


# ------------------------------------------------------------------------------------------------ the trainer's wiring
def test_compute_loss_key_set_with_and_without_the_key(monkeypatch):
    """the kernels stubbed out: without the key today's terms, no call and no table; with it one call per configured factor on the
    head's tensors and the UNMASKED labels, after every other term, weight WEIGHT / f, with the table of the depth term when both
    keys use one stride"""
    from muvo_amd import ops, voxel_view
    from muvo_amd.trainer import WorldModelTrainer
    calls, depth_calls = [], []
    monkeypatch.setattr(ops, 'voxel_losses', lambda logits, target, weight, cw=None, terms=False: tuple(torch.zeros(()) for _ in range(3)))
    monkeypatch.setattr(ops, 'voxel_lovasz_loss', lambda logits, labels, weight, terms=False: (torch.zeros(()),))
    monkeypatch.setattr(voxel_view, '_RENDER_TABLES', {})

    def depth(logits, labels, rays, n_valid, weight, terms=False):
        depth_calls.append((logits, labels, rays, n_valid, weight, terms))
        return (torch.zeros(()),)

    def klass(logits, labels, rays, n_valid, weight, terms=False):
        calls.append((logits, labels, rays, n_valid, weight, terms))
        return (torch.zeros(()),)
    monkeypatch.setattr(ops, 'voxel_render_loss', depth)
    monkeypatch.setattr(ops, 'voxel_render_class_loss', klass)
    batch, output = LV.voxel_dicts(sizes=((192, 192, 64), (96, 96, 32), (48, 48, 16)), b=1, s=1, C=9)
    for f in (1, 2, 4):                                                           # present, and never to be read by this term
        batch[f'voxel_visible_label_{f}'] = torch.full_like(batch[f'voxel_label_{f}'], 255)
    today = [f'{name}_{f}' for f in (1, 2, 4) for name in ('voxel', 'sem_scal', 'geo_scal')]
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=LV.voxel_only_cfg()), batch, output)
    assert list(losses) == today and not calls and not depth_calls and not voxel_view._RENDER_TABLES
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_RENDER_CLASS.WEIGHT': 0.5, 'LOSSES.VOXEL_RENDER_CLASS.STRIDE': 32, 'LOSSES.VOXEL_RENDER.WEIGHT': 0.25,
                               'LOSSES.VOXEL_RENDER.STRIDE': 32, 'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5})
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
    assert list(losses) == today + [f'voxel_lovasz_{f}' for f in (1, 2, 4)] + [f'voxel_render_{f}' for f in (1, 2, 4)] + \
        [f'voxel_render_class_{f}' for f in (1, 2, 4)]
    base = voxel_view.lidar_rays(cfg, 32)
    for k, f in enumerate((1, 2, 4)):
        logits, labels, rays, n_valid, weight, terms = calls[k]
        assert logits is output[f'voxel_{f}'] and labels is batch[f'voxel_label_{f}'] and terms is True
        assert weight == 0.5 * (1 / f)
        assert rays is depth_calls[k][2] and n_valid == depth_calls[k][3]         # one table for both terms
        assert rays.dtype == torch.float32 and tuple(rays.shape) == base.shape
        assert n_valid == int(R.cell_table(tuple(logits.shape[3:]), rays.numpy())['valid'].sum()) == len(base)
    assert len(voxel_view._RENDER_TABLES) == 3
    del calls[:], depth_calls[:]
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_RENDER_CLASS.WEIGHT': 2.0, 'LOSSES.VOXEL_RENDER_CLASS.FACTORS': [2], 'LOSSES.VOXEL_RENDER_CLASS.STRIDE': 64})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today + ['voxel_render_class_2']
    assert calls[0][0] is output['voxel_2'] and calls[0][4] == 1.0 and not depth_calls and len(voxel_view._RENDER_TABLES) == 4
    del calls[:]
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_RENDER_CLASS.WEIGHT': 0.0})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today and not calls


def test_module_guards():
    from muvo_amd.losses import RenderedClassLoss
    crit = RenderedClassLoss(torch.zeros(4, 7), n_valid=0)
    with pytest.raises(ValueError):
        crit(torch.zeros(1, 2, 5, 4), torch.zeros(1, 2, 5, 4))


# ------------------------------------------------------------------------------------------------ the entries' argument checks
def test_entry_points_validate_before_touching_the_device():
    """bad arguments come back as MUVO_ERR_INVALID_ARG with a message; nothing is launched (this runs without a GPU)"""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    p, null = C.c_void_p(256), C.c_void_p(0)      # never dereferenced: every call below is rejected by its argument checks
    i64, st, w = C.c_int64, C.c_void_p(0), C.c_float(1.0)
    V, Rn = 13 * 10 * 7, 300
    need = L.muvo_render_class_ws_bytes(i64(3), 9, i64(V), i64(Rn))
    assert need >= 3 * V * 9 * 4 + 3 * 9 * V * 8 + 3 * 2 * 8                      # the probabilities, the 64-bit accumulator, the partials
    assert need <= 3 * V * 9 * 12 + 3 * 2 * 8 + 16
    for bad in ((0, 9, V, Rn), (65536, 9, V, Rn), (3, 1, V, Rn), (3, 17, V, Rn), (3, 9, 0, Rn), (3, 9, 1 << 30, Rn), (3, 9, V, 0),
                (3, 9, V, (1 << 24) + 1)):
        assert L.muvo_render_class_ws_bytes(i64(bad[0]), bad[1], i64(bad[2]), i64(bad[3])) == -1

    def fwd(F=3, Cn=9, X=13, Y=10, Z=7, R_=Rn, nv=Rn, logits=p, labels=p, rays=p, hit=p, ws=p, wsb=need, mass=p, target=p, loss=p):
        return L.muvo_render_class_fwd(logits, labels, i64(F), Cn, X, Y, Z, rays, i64(R_), i64(nv), hit, w, ws, i64(wsb), mass, target, null, null, loss, st)

    def bwd(F=3, Cn=9, X=13, Y=10, Z=7, R_=Rn, nv=Rn, logits=p, rays=p, mass=p, target=p, gout=p, ws=p, wsb=need, dl=p):
        return L.muvo_render_class_bwd(logits, i64(F), Cn, X, Y, Z, rays, i64(R_), i64(nv), mass, target, w, gout, ws, i64(wsb), dl, st)
    for call in (fwd, bwd):
        for kw, msg in (({'Cn': 1}, b'2..16'), ({'Cn': 17}, b'2..16'), ({'F': 0}, b'65535'), ({'F': 65536}, b'65535'), ({'X': 2049}, b'2048'),
                        ({'Z': 0}, b'2048'), ({'X': 2048, 'Y': 2048, 'Z': 256}, b'2^30'), ({'R_': 0}, b'2^24'), ({'R_': (1 << 24) + 1}, b'2^24'),
                        ({'nv': Rn + 1}, b'valid rays'), ({'nv': -1}, b'valid rays'), ({'ws': null}, b'workspace'), ({'wsb': need - 1}, b'workspace'),
                        ({'ws': C.c_void_p(264)}, b'workspace'), ({'logits': null}, b'null pointer'), ({'rays': null}, b'null pointer'),
                        ({'mass': null}, b'null pointer'), ({'target': null}, b'null pointer'), ({'mass': C.c_void_p(260)}, b'8-byte')):
            assert call(**kw) == -1 and msg in L.muvo_last_error(), (call.__name__, kw, L.muvo_last_error())
    for kw in ({'labels': null}, {'hit': null}, {'loss': null}):
        assert fwd(**kw) == -1 and b'render_class_fwd: null pointer' in L.muvo_last_error()
    for kw in ({'gout': null}, {'dl': null}):
        assert bwd(**kw) == -1 and b'render_class_bwd: null pointer' in L.muvo_last_error()
