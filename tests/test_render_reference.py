"""CPU: the restatement of the rendered first-hit depth loss (tests/render_reference.py) - its cell sequence against the march of
raycast_reference cell by cell, its compositing and closed-form gradient against torch float64 autograd and central differences,
three closed forms - and the configuration surface of the extension key LOSSES.VOXEL_RENDER."""
import argparse
import types

import numpy as np
import pytest
import torch

import lovasz_reference as LV
import raycast_reference as RC
import render_reference as R

ORIGIN = (3.5, 5.0, 3.5)


def _rays(g):
    hand = np.array([r for _, r, _ in RC.hand_rays(g)], np.float32)
    return np.concatenate([RC.fan_rays(ORIGIN, 8, 32, 10.0, -30.0), hand, RC.camera_rays(RC.X, RC.Y, RC.Z, RC.R)[::7]])


# ------------------------------------------------------------------------------------------------ the cell sequence
def test_cell_sequence_is_the_march_of_raycast_reference():
    """every cell of every sequence, occupied alone, is what raycast_reference.march hits, at the same float32 depth; an invalid
    ray misses even a full grid; and on a random scene the first occupied cell of the sequence is the first hit - or the ray
    misses and no cell of its sequence is occupied"""
    g = RC.scene()
    rays = _rays(g)
    tab = R.cell_table(g.shape, rays)
    full = np.ones_like(g)
    for r in range(0, len(rays), 3):
        first = RC.march(full, rays[r])
        assert (first[0] >= 0) == bool(tab['valid'][r])
        if not tab['valid'][r]:
            assert tab['n'][r] == -1 and tab['t_exit'][r] == 0
            continue
        n = int(tab['n'][r])
        assert n >= 1 and len(set(tab['cells'][r, :n].tolist())) == n and (tab['cells'][r, n:] == -1).all()
        for k in range(n):
            one = np.zeros(g.size, np.uint8)
            one[tab['cells'][r, k]] = 1
            idx, t, _ = RC.march(one.reshape(g.shape), rays[r])
            assert idx == tab['cells'][r, k] and np.float32(t).tobytes() == tab['t'][r, k].tobytes(), (r, k)
        assert (np.diff(tab['t'][r, :n]) >= 0).all() and tab['t'][r, n - 1] <= tab['t_exit'][r]
    hit, t, _ = RC.cast(g, rays)
    ts = R.target_depth(g, tab)
    flat = g.reshape(-1)
    for r in range(len(rays)):
        seq = tab['cells'][r][tab['cells'][r] >= 0]
        if hit[r] >= 0:
            assert tab['valid'][r] and ts[r].tobytes() == t[r].tobytes()
        else:
            assert not flat[seq].any() and ts[r] == tab['t_exit'][r]
    assert tab['valid'].sum() >= 256 and (~tab['valid']).sum() >= 6              # NaN, zero direction, clean misses


def test_valid_rays_of_the_package_equal_the_table():
    from muvo_amd.voxel_view import valid_rays
    g = RC.scene()
    rays = _rays(g)
    assert np.array_equal(valid_rays(rays, *g.shape), R.cell_table(g.shape, rays)['valid'])
    cube = RC.fan_rays((20.0, 4.0, 4.0), 4, 8, 10.0, -30.0)                       # from outside an 8 x 8 x 8 grid
    assert np.array_equal(valid_rays(cube, 8, 8, 8), R.cell_table((8, 8, 8), cube)['valid'])


# ------------------------------------------------------------------------------------------------ compositing and gradient
def _case(C, seed=0):
    scenes = [R.clip_classes(g, C) for g in (RC.scene(), RC.shifted(RC.scene()), np.zeros((RC.X, RC.Y, RC.Z), np.uint8))]
    return R.frames(scenes, C, seed), np.stack(scenes), _rays(RC.scene())


def _autograd(logits, labels, rays, weight):
    """the definition through torch float64 autograd: softmax, cumprod, abs"""
    tab = R.cell_table(logits.shape[2:], rays)
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    F, C = z.shape[:2]
    cells = torch.from_numpy(tab['cells'])
    pad, idx = cells < 0, cells.clamp(min=0)
    tk, texit, valid = torch.from_numpy(tab['t']).double(), torch.from_numpy(tab['t_exit']).double(), torch.from_numpy(tab['valid'])
    total, Ds = 0.0, []
    for f in range(F):
        p = torch.softmax(z[f].reshape(C, -1), 0)
        q, a = p[0], p[1:].sum(0)
        qk, ak = torch.where(pad, torch.ones(()).double(), q[idx]), torch.where(pad, torch.zeros(()).double(), a[idx])
        T = torch.cat([torch.ones(len(qk), 1, dtype=torch.float64), torch.cumprod(qk, 1)], 1)
        D = (T[:, :-1] * ak * tk).sum(1) + T[:, -1] * texit
        ts = torch.from_numpy(R.target_depth(labels[f], tab)).double()
        total = total + (D - ts).abs()[valid].sum() / int(valid.sum())
        Ds.append(torch.where(valid, D, torch.zeros(()).double()))
    loss = weight * total / F
    grad, = torch.autograd.grad(loss, z)
    return loss.item(), grad.numpy(), torch.stack(Ds).detach().numpy()


@pytest.mark.parametrize('C', [2, 9])
def test_closed_form_gradient_equals_autograd(C):
    logits, labels, rays = _case(C)
    ref = R.loss_and_grad(logits, labels, rays, R.WEIGHT)
    loss, grad, D = _autograd(logits, labels, rays, R.WEIGHT)
    assert abs(ref['loss'] - loss) <= 1e-13 * abs(loss)
    assert np.abs(ref['D'] - D).max() <= 1e-12
    scale = np.abs(grad).max()
    assert scale > 0 and np.abs(ref['dlogits'] - grad).max() <= 1e-13 * scale
    unseen = ref['visits'].reshape(3, *logits.shape[2:]) == 0
    assert unseen.any() and not np.moveaxis(ref['dlogits'], 1, 0)[:, unseen].any()            # no ray, no gradient


def test_gradient_equals_central_differences():
    logits, labels, rays = _case(2, seed=1)
    tab = R.cell_table(logits.shape[2:], rays)
    ref = R.loss_and_grad(logits, labels, rays, R.WEIGHT, table=tab)
    z = logits.astype(np.float64)
    order = np.argsort(-np.abs(ref['dlogits']).reshape(-1))[:12]                 # the largest entries, where a difference resolves
    h = 1e-6
    for flat in order:
        at = np.unravel_index(flat, z.shape)
        up, down = z.copy(), z.copy()
        up[at] += h
        down[at] -= h
        fd = (R.loss_and_grad(up, labels, rays, R.WEIGHT, table=tab)['loss'] - R.loss_and_grad(down, labels, rays, R.WEIGHT, table=tab)['loss']) / (2 * h)
        assert abs(fd - ref['dlogits'][at]) <= 1e-7 * max(1.0, abs(fd)), (at, fd, ref['dlogits'][at])


def test_constant_logits_render_the_geometric_series():
    """C = 2, equal logits: a = q = 1/2, so D = sum 2^-(k+1) t_k + 2^-n t_exit"""
    g = RC.scene()
    rays = _rays(g)
    tab = R.cell_table(g.shape, rays)
    q, a, _ = R.occupancy(np.full((2, g.size), 0.75, np.float32))
    assert (q == 0.5).all() and (a == 0.5).all()
    D = R.render(q, a, tab)['D']
    for r in np.flatnonzero(tab['valid']):
        n = int(tab['n'][r])
        want = sum(2.0 ** -(k + 1) * float(tab['t'][r, k]) for k in range(n)) + 2.0 ** -n * float(tab['t_exit'][r])
        assert abs(D[r] - want) <= 1e-13 * max(1.0, want)
    assert not D[~tab['valid']].any()


def test_confidently_empty_renders_at_the_exit_and_costs_nothing_where_the_label_misses():
    g = RC.scene()
    rays = _rays(g)
    logits = np.zeros((1, 2, *g.shape), np.float32)
    logits[:, 0] = 60.0
    empty = R.loss_and_grad(logits, np.zeros((1, *g.shape), np.uint8), rays, 1.0)
    tab = empty['table']
    assert np.abs(empty['D'][0] - tab['t_exit'])[tab['valid']].max() <= 1e-12 and empty['loss'] <= 1e-12
    ref = R.loss_and_grad(logits, g[None], rays, 1.0)
    miss = tab['valid'] & (ref['tstar'][0] == tab['t_exit'])
    assert miss.any() and np.abs(ref['D'][0] - ref['tstar'][0])[miss].max() <= 1e-12
    assert ref['loss'] > 0.1                                                     # the rays that hit the label are charged


def test_confident_correct_prediction_renders_the_labels_first_hit():
    g = R.clip_classes(RC.scene(), 9)
    rays = _rays(g)
    logits = np.zeros((1, 9, *g.shape), np.float32)
    idx = np.indices(g.shape)
    logits[(0, g.astype(np.int64), *idx)] = 40.0
    ref = R.loss_and_grad(logits, g[None], rays, 1.0)
    v = ref['table']['valid']
    assert np.abs(ref['D'][0] - ref['tstar'][0])[v].max() <= 1e-12 and ref['loss'] <= 1e-12


def test_no_valid_ray_gives_zero_loss_and_gradient():
    logits, labels, _ = _case(2)
    rays = np.array([[-3.0, -3.0, 20.0, -1, 0, 0.5, np.inf], [2.5, 3.5, 9.0, np.nan, 0, -1, np.inf], [1, 1, 1, 0, 0, 0, np.inf]], np.float32)
    ref = R.loss_and_grad(logits, labels, rays, R.WEIGHT)
    assert ref['n_valid'] == 0 and ref['loss'] == 0 and not ref['dlogits'].any() and np.isfinite(ref['dlogits']).all()


def test_inputs_of_the_gpu_tests_keep_their_signs():
    """|D - t*| >= 1e-4 on every valid ray of the float64 reference: no sign can flip under a float32 evaluation"""
    for C in (2, 9):
        logits, labels, rays = _case(C)
        ref = R.loss_and_grad(logits, labels, rays, R.WEIGHT)
        v = ref['table']['valid']
        assert np.abs(ref['D'] - ref['tstar'])[:, v].min() >= 1e-4


# ------------------------------------------------------------------------------------------------ configuration
def test_defaults_do_not_carry_the_key():
    from muvo_amd import config
    cfg = config.get_cfg()
    assert 'VOXEL_RENDER' not in cfg.LOSSES and 'VOXEL_RENDER' not in config.base_1d_cfg().LOSSES
    assert config.voxel_render(cfg) == (0.0, config.DEFAULT_VOXEL_RENDER_FACTORS, config.DEFAULT_VOXEL_RENDER_STRIDE)
    import glob
    import yaml
    for path in glob.glob(config.os.path.join(config._HERE, 'configs', '*.yml')):
        assert 'VOXEL_RENDER' not in open(path).read(), path
    assert 'VOXEL_RENDER' not in yaml.safe_dump(config.base_1d_cfg().convert_to_dict())


def test_key_round_trips_through_yaml_dict_and_override(tmp_path):
    from muvo_amd import config
    y = tmp_path / 'rd.yml'
    y.write_text('VOXEL_SEG: {ENABLED: true}\nLOSSES:\n  VOXEL_RENDER: {WEIGHT: 0.5, FACTORS: [2, 4], STRIDE: 4}\n')
    cfg = config.get_cfg(argparse.Namespace(config_file=str(y), opts=[]))
    assert config.voxel_render(cfg) == (0.5, (2, 4), 4)
    assert cfg.convert_to_dict()['LOSSES']['VOXEL_RENDER'] == {'WEIGHT': 0.5, 'FACTORS': [2, 4], 'STRIDE': 4}
    again = config.get_cfg(cfg_dict=cfg.convert_to_dict())                   # the dict a checkpoint carries
    assert config.voxel_render(again) == (0.5, (2, 4), 4)
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': 2}}})
    assert config.voxel_render(cfg) == (2.0, config.DEFAULT_VOXEL_RENDER_FACTORS, config.DEFAULT_VOXEL_RENDER_STRIDE)
    cfg = config.get_cfg(argparse.Namespace(config_file='', opts=['VOXEL_SEG.ENABLED', 'True', 'LOSSES.VOXEL_RENDER.WEIGHT', '0.25',
                                                                  'LOSSES.VOXEL_RENDER.FACTORS', '[4]', 'LOSSES.VOXEL_RENDER.STRIDE', '2']))
    assert config.voxel_render(cfg) == (0.25, (4,), 2)
    with pytest.raises(KeyError):
        config.get_cfg().merge_from_list(['LOSSES.VOXEL_RENDR.WEIGHT', '1'])


@pytest.mark.parametrize('factors', [[3], [2, 8], [0], [2, 2], 2, [True]], ids=str)
def test_bad_factors_raise(factors):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': 1.0, 'FACTORS': factors}}})
    with pytest.raises(ValueError, match='FACTORS'):
        config.voxel_render(cfg)


@pytest.mark.parametrize('stride', [0, -1, 1.5, True, 'four'], ids=str)
def test_bad_stride_raises(stride):
    from muvo_amd import config
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': 1.0, 'STRIDE': stride}}})
    with pytest.raises(ValueError, match='STRIDE'):
        config.voxel_render(cfg)


def test_bad_weight_and_disabled_head_raise():
    from muvo_amd import config
    with pytest.raises(ValueError, match='VOXEL_SEG.ENABLED'):
        config.voxel_render(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': 1.0}}}))
    assert config.voxel_render(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': 0.0}}}))[0] == 0.0
    for w in (-1.0, 'much', True):
        with pytest.raises(ValueError, match='WEIGHT'):
            config.voxel_render(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}, 'LOSSES': {'VOXEL_RENDER': {'WEIGHT': w}}}))


def test_compute_loss_key_set_with_and_without_the_key(monkeypatch):
    """the trainer's wiring with the kernels stubbed out: without the key today's terms, no call and no table; with it one call per
    configured factor on the head's tensors as they are, after every other term, with the table of that scale - the lidar's origin
    divided by f, the directions of scale 1 - and the weight in the scaled depth units of lidar_depth_f"""
    from muvo_amd import ops, voxel_view
    from muvo_amd.trainer import WorldModelTrainer
    calls = []
    monkeypatch.setattr(ops, 'voxel_losses', lambda logits, target, weight, cw=None, terms=False: tuple(torch.zeros(()) for _ in range(3)))
    monkeypatch.setattr(ops, 'voxel_lovasz_loss', lambda logits, labels, weight, terms=False: (torch.zeros(()),))
    monkeypatch.setattr(voxel_view, '_RENDER_TABLES', {})

    def render(logits, labels, rays, n_valid, weight, terms=False):
        calls.append((logits, labels, rays, n_valid, weight, terms))
        return (torch.zeros(()),)
    monkeypatch.setattr(ops, 'voxel_render_loss', render)
    batch, output = LV.voxel_dicts(sizes=((192, 192, 64), (96, 96, 32), (48, 48, 16)), b=1, s=1)
    today = [f'{name}_{f}' for f in (1, 2, 4) for name in ('voxel', 'sem_scal', 'geo_scal')]
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=LV.voxel_only_cfg()), batch, output)
    assert list(losses) == today and not calls and not voxel_view._RENDER_TABLES
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_RENDER.WEIGHT': 0.5, 'LOSSES.VOXEL_RENDER.STRIDE': 32, 'LOSSES.VOXEL_LOVASZ.WEIGHT': 0.5})
    losses = WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
    assert list(losses) == today + [f'voxel_lovasz_{f}' for f in (1, 2, 4)] + [f'voxel_render_{f}' for f in (1, 2, 4)]
    base = voxel_view.lidar_rays(cfg, 32)
    for k, f in enumerate((1, 2, 4)):
        logits, labels, rays, n_valid, weight, terms = calls[k]
        assert logits is output[f'voxel_{f}'] and labels is batch[f'voxel_label_{f}'] and terms is True
        assert weight == 0.5 * (1 / f) * (cfg.VOXEL.RESOLUTION * f / cfg.LIDAR_RE.SCALE)
        assert rays.dtype == torch.float32 and tuple(rays.shape) == base.shape
        assert np.array_equal(rays[:, 3:].numpy(), base[:, 3:]) and np.allclose(rays[:, :3].numpy() * f, base[:, :3], rtol=1e-6)
        assert n_valid == int(R.cell_table(tuple(logits.shape[3:]), rays.numpy())['valid'].sum()) == len(base)
    assert len(voxel_view._RENDER_TABLES) == 3
    WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)
    assert len(voxel_view._RENDER_TABLES) == 3 and calls[3][2] is calls[0][2]         # the tables are cached
    del calls[:]
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_RENDER.WEIGHT': 0.5, 'LOSSES.VOXEL_RENDER.FACTORS': [2], 'LOSSES.VOXEL_RENDER.STRIDE': 32})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today + ['voxel_render_2']
    assert calls[0][0] is output['voxel_2']
    del calls[:]
    cfg = LV.voxel_only_cfg(**{'LOSSES.VOXEL_RENDER.WEIGHT': 0.0})
    assert list(WorldModelTrainer.compute_loss(types.SimpleNamespace(cfg=cfg), batch, output)) == today and not calls


def test_validation_curves_pick_the_terms_up_by_name():
    import inspect
    from muvo_amd import validate
    src = inspect.getsource(validate)
    assert "{f'val{idx}_{k}': v for k, v in loss.items()}" in src and 'voxel_render' not in src


def test_module_guards():
    from muvo_amd.losses import RenderedDepthLoss
    crit = RenderedDepthLoss(torch.zeros(4, 7), n_valid=0)
    with pytest.raises(ValueError):
        crit(torch.zeros(1, 2, 5, 4), torch.zeros(1, 2, 5, 4))


def test_entry_points_validate_before_touching_the_device():
    """bad arguments come back as MUVO_ERR_INVALID_ARG with a message; nothing is launched (this runs without a GPU)"""
    import ctypes as C
    from muvo_amd import ops
    L = ops.lib()
    p, null = C.c_void_p(256), C.c_void_p(0)      # never dereferenced: every call below is rejected by its argument checks
    i64, st, w = C.c_int64, C.c_void_p(0), C.c_float(1.0)
    V, Rn = 13 * 10 * 7, 300
    need = L.muvo_render_ws_bytes(i64(3), i64(V), i64(Rn))
    assert need >= 3 * V * 16 + 3 * 2 * 8                                       # q, a, the 64-bit accumulator, the partials
    for bad in ((0, V, Rn), (65536, V, Rn), (3, 0, Rn), (3, 1 << 30, Rn), (3, V, 0), (3, V, (1 << 24) + 1)):
        assert L.muvo_render_ws_bytes(*(i64(v) for v in bad)) == -1

    def fwd(F=3, Cn=2, X=13, Y=10, Z=7, R_=Rn, nv=Rn, logits=p, rays=p, hit=p, lt=p, ws=p, wsb=need, depth=p, target=p, loss=p):
        return L.muvo_render_fwd(logits, i64(F), Cn, X, Y, Z, rays, i64(R_), i64(nv), hit, lt, w, ws, i64(wsb), depth, target, null, null, null, loss, st)

    def bwd(F=3, Cn=2, X=13, Y=10, Z=7, R_=Rn, nv=Rn, logits=p, rays=p, depth=p, target=p, gout=p, ws=p, wsb=need, dl=p):
        return L.muvo_render_bwd(logits, i64(F), Cn, X, Y, Z, rays, i64(R_), i64(nv), depth, target, w, gout, ws, i64(wsb), dl, st)
    for call in (fwd, bwd):
        for kw, msg in (({'Cn': 1}, b'2..16'), ({'Cn': 17}, b'2..16'), ({'F': 0}, b'65535'), ({'F': 65536}, b'65535'), ({'X': 2049}, b'2048'),
                        ({'Z': 0}, b'2048'), ({'X': 2048, 'Y': 2048, 'Z': 256}, b'2^30'), ({'R_': 0}, b'2^24'), ({'R_': (1 << 24) + 1}, b'2^24'),
                        ({'nv': Rn + 1}, b'valid rays'), ({'nv': -1}, b'valid rays'), ({'ws': null}, b'workspace'), ({'wsb': need - 1}, b'workspace'),
                        ({'ws': C.c_void_p(264)}, b'workspace'), ({'logits': null}, b'null pointer'), ({'rays': null}, b'null pointer'),
                        ({'depth': null}, b'null pointer'), ({'target': null}, b'null pointer'), ({'depth': C.c_void_p(260)}, b'8-byte')):
            assert call(**kw) == -1 and msg in L.muvo_last_error(), (call.__name__, kw, L.muvo_last_error())
    for kw in ({'hit': null}, {'lt': null}, {'loss': null}):
        assert fwd(**kw) == -1 and b'render_fwd: null pointer' in L.muvo_last_error()
    for kw in ({'gout': null}, {'dl': null}):
        assert bwd(**kw) == -1 and b'render_bwd: null pointer' in L.muvo_last_error()
