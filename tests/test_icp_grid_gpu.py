"""-m gpu: search='grid' of the on-device ICP (muvo_amd/csrc/icp.hip: icp_grid_* kernels and icp_correspond_grid_kernel through
ops.icp_step / ops.icp_register / ops.icp_register_queued, muvo_amd/odometry.py, PreProcess, predict) against search='brute' with
torch.equal on every output - corr, the 17 sums, T, fitness, rmse, iterations, status - and, where stated, against the float64
restatement of tests/icp_reference.py and the numpy restatement of the grid search (tests/icp_grid_reference.py, shown on the CPU
by tests/test_icp_grid_reference.py to equal the exhaustive search and to see planted errors)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import icp_grid_reference as G
import icp_reference as R

pytestmark = pytest.mark.gpu
GUARD = 12345.0
IDS = [c['id'] for c in R.CASES]
LATTICE = G.lattice_inputs()
NONFINITE = G.nonfinite_inputs()


def _place(t, dev, off):
    """`t` on the device inside a fresh buffer of GUARD values, `off` elements after four guard elements; (buffer, view)"""
    n = t.numel()
    buf = torch.full((n + 12,), GUARD, dtype=t.dtype, device=dev)
    buf[4 + off:4 + off + n] = t.reshape(-1).to(dev)
    return buf, buf[4 + off:4 + off + n].view(t.shape)


def _guards_ok(buf, off, n):
    return bool((buf[:4 + off] == GUARD).all()) and bool((buf[4 + off + n:] == GUARD).all())


def _same(a, b, what=''):
    for name, x, y in zip(a._fields, a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), f'{what}: {name} differs between the searches'


def _step_both(dev, src, tgt, sf, tf, scale, thr, **kw):
    """icp_step in both searches, the grid's outputs between guard values; asserts equal bytes and returns the grid's"""
    from muvo_amd import ops
    P, n = len(sf), src.shape[2]
    cb, sb, rb = ops.icp_step(src, tgt, sf, tf, scale, thr, search='brute', **kw)
    cbuf, corr = _place(torch.zeros(P, n, dtype=torch.int32), dev, 1)
    sbuf, sums = _place(torch.zeros(P, 17, dtype=torch.float64), dev, 1)
    cg, sg, rg = ops.icp_step(src, tgt, sf, tf, scale, thr, search='grid', out=(corr, sums), **kw)
    assert _guards_ok(cbuf, 1, P * n) and _guards_ok(sbuf, 1, P * 17), 'a guard element changed'
    assert torch.equal(cg, cb), 'corr differs between the searches'
    assert torch.equal(sg, sb), 'the sums differ between the searches'
    _same(rg, rb, 'icp_step')
    return cg, sg, rg


def _pair_frames(dev, src, tgt):
    """(2, 4, n) on the device: frame 0 = src, frame 1 = tgt, both padded to one n with invalid points (range 0, NaN coordinates)"""
    n = max(src.shape[1], tgt.shape[1])
    frames = torch.full((2, 4, n), float('nan'))
    frames[:, 3] = 0.0
    frames[0, :, :src.shape[1]] = torch.from_numpy(src)
    frames[1, :, :tgt.shape[1]] = torch.from_numpy(tgt)
    return frames.to(dev)


def _dev_frames(dev, *frames):
    return [torch.from_numpy(np.ascontiguousarray(f))[None].to(dev) for f in frames]


# ---- 1. every case of icp_reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('id', IDS)
def test_cases_step_and_register(dev, id):
    from muvo_amd import ops
    c = R.CASE[id]
    r64, _ = R.reference(id)
    s, t = _dev_frames(dev, *R.inputs(id)[:2])
    corr, sums, res = _step_both(dev, s, t, [0], [0], c['scale'], c['thr'], source_stride=c['stride'])
    brute = ops.icp_register(s, t, [0], [0], c['scale'], c['thr'], source_stride=c['stride'])
    grid = ops.icp_register(s, t, [0], [0], c['scale'], c['thr'], source_stride=c['stride'], search='grid')
    _same(grid, brute, 'icp_register')
    if r64['status'] == R.EMPTY:
        assert int(res.status[0]) == ops.ICP_EMPTY and bool((corr == -1).all()) and not sums.any()
        assert int(grid.status[0]) == ops.ICP_EMPTY and torch.equal(grid.T[0].cpu(), torch.eye(4, dtype=torch.float64))
        return
    assert np.array_equal(corr[0].cpu().numpy(), R.corr_full(id, r64['evals'][0])), 'another correspondence than float64'
    assert int(grid.iterations[0]) == r64['iterations'] and int(grid.status[0]) == r64['status']


# ---- 2. lattice inputs: also against numpy, exactly --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _numpy_search(name):
    inp = (LATTICE if name in LATTICE else NONFINITE)[name]
    return G.grid_search(inp['src'], inp['tgt'], 1.0, inp['thr'], inp['init']), G.brute_search(inp['src'], inp['tgt'], 1.0, inp['thr'], inp['init'])


@pytest.mark.parametrize('name', list(LATTICE))
def test_lattice_inputs(dev, name):
    inp = LATTICE[name]
    (d2, idx), (bd2, bidx) = _numpy_search(name)
    want = G.corr_of(d2, idx, inp['thr'])
    assert np.array_equal(want, G.corr_of(bd2, bidx, inp['thr']))
    frames = _pair_frames(dev, inp['src'], inp['tgt'])
    init = None if inp['init'] is None else torch.from_numpy(inp['init'])[None]
    corr, sums, res = _step_both(dev, frames, frames, [0], [1], 1.0, inp['thr'], init=init)
    got = corr[0].cpu().numpy()
    assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all(), 'another correspondence than numpy'
    inl = want >= 0
    assert float(sums[0, 0]) == inl.sum() and float(sums[0, 1]) == float(d2[inl].astype(np.float64).sum()), 'sum d^2 is not numpy\'s, exactly'


# ---- 3. non-finite coordinates at points with range > 0 ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(NONFINITE))
def test_nonfinite_inputs(dev, name):
    inp = NONFINITE[name]
    (d2, idx), (bd2, bidx) = _numpy_search(name)
    want = G.corr_of(bd2, bidx, inp['thr'])
    assert np.array_equal(G.corr_of(d2, idx, inp['thr']), want)
    frames = _pair_frames(dev, inp['src'], inp['tgt'])
    corr, sums, res = _step_both(dev, frames, frames, [0], [1], 1.0, inp['thr'])
    got = corr[0].cpu().numpy()
    assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all()
    assert (want >= 0).sum() >= 10


# ---- 4. grid shapes ------------------------------------------------------------------------------------------------------------------
def test_extent_far_above_the_threshold_and_threshold_above_the_extent(dev):
    g = np.random.default_rng(17)
    wide = g.uniform(-4000, 4000, (2000, 3))
    grid = G.build(G.frame(wide), 1.0, 0.5)
    assert grid['h'] > 0.0625 and grid['dims'].prod() <= G.CELLS, 'the cell cap must engage'
    src = wide[g.permutation(2000)] + g.normal(0, 0.15, (2000, 3))
    src[:20] += 1e4                                          # far outside the box: the clamp
    s, t = _dev_frames(dev, G.frame(src), G.frame(wide))
    corr, sums, _ = _step_both(dev, s, t, [0], [0], 1.0, 0.5)
    assert 1000 < float(sums[0, 0]) < 1980 and bool((corr[0, :20] == -1).all())
    small = g.uniform(-1, 1, (300, 3))
    s, t = _dev_frames(dev, G.frame(small[g.permutation(300)] + 0.3), G.frame(small))
    assert list(G.build(G.frame(small), 1.0, 40.0)['dims']) == [2, 2, 2]
    corr, sums, _ = _step_both(dev, s, t, [0], [0], 1.0, 40.0)
    assert float(sums[0, 0]) == 300


@pytest.mark.parametrize('thr', [5.0, 0.7])
def test_cluster_and_background_full_registration_is_deterministic(dev, thr):
    from muvo_amd import ops
    g = np.random.default_rng(23)
    tgt = np.concatenate([g.normal(0, 0.3, (2048, 3)) + (20, -30, 1), g.uniform((0, -50, -4), (100, 50, 4), (2048, 3))])[g.permutation(4096)]
    move = np.linalg.inv(R.pose(0.2, -0.1, 1.0))
    src = (tgt @ move[:3, :3].T + move[:3, 3] + g.normal(0, 0.02, tgt.shape))[g.permutation(4096)]
    s, t = _dev_frames(dev, G.frame(src), G.frame(tgt))
    was = ops.get_deterministic()
    runs = []
    try:
        for det in (False, True):
            ops.set_deterministic(det)
            for _ in range(2):
                runs.append(ops.icp_register(s, t, [0], [0], 1.0, thr, max_iteration=12, search='grid'))
        brute = ops.icp_register(s, t, [0], [0], 1.0, thr, max_iteration=12)
    finally:
        ops.set_deterministic(was)
    assert int(runs[0].iterations[0]) >= 3, 'several iterations'
    for r in runs[1:]:
        _same(r, runs[0], 'two grid runs')
    _same(runs[0], brute, 'icp_register')
    _step_both(dev, s, t, [0], [0], 1.0, thr)


# ---- 5. work lists -------------------------------------------------------------------------------------------------------------------
def test_work_list_shared_tensor_empty_pair_init_stride_queued(dev):
    from muvo_amd import ops
    a_src, a_tgt, _ = R.inputs('n1025-C5')
    b_src, b_tgt, _ = R.inputs('n1025-stride-3')
    n = 1025
    frames = torch.full((5, 5, n), float('nan'))
    for k, f in enumerate((a_src, a_tgt, b_src, b_tgt)):
        frames[k, :f.shape[0]] = torch.from_numpy(f)
    frames[4, 3] = 0.0                                      # frame 4: no valid point
    fbuf, view = _place(frames, dev, 3)
    sf, tf = [0, 2, 4, 2, 0], [1, 1, 1, 3, 3]               # two pairs on target frame 1, an EMPTY pair in the middle
    init = torch.stack([torch.from_numpy(R.pose(0.05 * k, -0.02 * k, 0.3 * k)) for k in range(5)])
    kw = dict(init=init, source_stride=3)
    corr, sums, res = _step_both(dev, view, view, sf, tf, 1.0, R.THRESHOLD, **kw)
    assert int(res.status[2]) == ops.ICP_EMPTY and bool((corr[2] == -1).all()) and not sums[2].any()
    assert bool((corr[:, 1::3] == -1).all()) and bool((corr[:, 2::3] == -1).all()), 'points that are no query stay -1'
    assert all(float(sums[p, 0]) > 300 for p in (0, 1, 3, 4))
    brute = ops.icp_register(view, view, sf, tf, 1.0, R.THRESHOLD, max_iteration=6, **kw)
    grid = ops.icp_register(view, view, sf, tf, 1.0, R.THRESHOLD, max_iteration=6, search='grid', **kw)
    queued = ops.icp_register_queued(view, view, sf, tf, 1.0, R.THRESHOLD, 6, search='grid', **kw)
    _same(grid, brute, 'icp_register')
    _same(queued, grid, 'icp_register_queued')
    assert int(grid.status[2]) == ops.ICP_EMPTY and torch.equal(grid.T[2].cpu(), torch.eye(4, dtype=torch.float64))
    assert _guards_ok(fbuf, 3, frames.numel()), 'an input guard element changed'
    for p in (0, 3):                                        # a pair of the list equals its solo run
        solo = ops.icp_register(view, view, [sf[p]], [tf[p]], 1.0, R.THRESHOLD, max_iteration=6, init=init[p:p + 1], source_stride=3, search='grid')
        for x, y in zip(grid, solo):
            assert torch.equal(x[p], y[0])


# ---- 6. the workload's own layout ------------------------------------------------------------------------------------------------
def test_one_step_at_64_x_1024(dev):
    h, w = 64, 1024
    tgt = R.frame_of(R.ray_cast(np.eye(4), h, w), 4, 1.0)
    src = R.frame_of(R.ray_cast(R.pose(1.0, 0.1, 2.0), h, w), 4, 1.0)
    s, t = _dev_frames(dev, src, tgt)
    corr, sums, res = _step_both(dev, s, t, [0], [0], 1.0, R.THRESHOLD)
    assert float(sums[0, 0]) > 0.9 * float((src[3] > 0).sum())
    _step_both(dev, s, t, [0], [0], 1.0, R.THRESHOLD, source_stride=4)


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------
def _agg_cfg(window=4, search=None, **over):
    from muvo_amd.config import base_1d_cfg
    cfg = base_1d_cfg(**over)
    cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True, 'LIDAR_STRIDE': 4, 'CAMERA_STRIDE': 8})
    cfg.VOXEL_SEG['AGGREGATE'] = type(cfg)({'ENABLED': True, 'WINDOW': window})
    if search is not None:
        cfg.VOXEL_SEG['AGGREGATE']['ICP_SEARCH'] = search
    return cfg


def test_preprocess_with_icp_search_grid_writes_the_same_labels(dev):
    from muvo_amd.data.synthetic import make_batch
    from muvo_amd.models.preprocess import PreProcess
    b, s, window = 2, 3, 2
    plain = PreProcess(_agg_cfg(window)).to(dev).eval()(make_batch(b, s, seed=21, device=dev))
    grid = PreProcess(_agg_cfg(window, 'grid')).to(dev).eval()(make_batch(b, s, seed=21, device=dev))
    assert set(plain) == set(grid)
    for key in ('voxel_visible_label_1', 'voxel_visible_label_2', 'voxel_visible_label_4', 'voxel_aggregate_counts'):
        assert torch.equal(plain[key], grid[key]), key
    assert int(plain['voxel_aggregate_counts'].sum()) > 0


def test_predict_ego_search_grid_writes_the_same_ego_motion(dev, tmp_path):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd import ops
    from muvo_amd import predict as P
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    assert P.build_parser().parse_args(['--out', 'o', '--mode', 'test', '--ego-motion', '--ego-search', 'grid']).ego_search == 'grid'
    root = str(tmp_path / 'rec')
    os.makedirs(root)
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(77)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)

    def data():
        dm = DataModule(cfg, root, device=dev, seed=77)
        dm.setup()
        dm.test_sampler_0 = range(0, 4, 2)
        return dm
    was = ops.get_deterministic()
    ops.set_deterministic(True)                             # no order-dependent float atomics in the forward pass: equal means equal
    try:
        for out, search in ((str(tmp_path / 'brute'), None), (str(tmp_path / 'grid'), 'grid')):
            ego = dict(threshold=5.0, stride=16, max_iteration=20)
            if search is not None:
                ego['search'] = search
            P.run(cfg, dev, out, 'test', loaders=[0], limit_batches=1, seed=77, data=data(), module=module, log=lambda s: None, ego_motion=ego)
    finally:
        ops.set_deterministic(was)
    a = open(os.path.join(str(tmp_path / 'brute'), 'ego_motion.json'), 'rb').read()
    assert a == open(os.path.join(str(tmp_path / 'grid'), 'ego_motion.json'), 'rb').read()
    assert json.loads(a)['0']['pairs'] > 0
