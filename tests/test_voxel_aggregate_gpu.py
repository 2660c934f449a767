"""-m gpu: voxel labels filled from neighbouring frames (muvo_amd/csrc/voxel_aggregate.hip through ops.voxel_pose_chain,
ops.voxel_aggregate, PreProcess and WorldModelTrainer) against the restatement of
tests/voxel_aggregate_reference.py.  The aggregate kernel is held to the restatement EXACTLY - bytes and counts - on the same
matrices: both evaluate q = M (c + 1/2) in float64 in one stated order, and the CPU side first shows that no q of the chosen
inputs lies within 1e-9 of a cell face.  The chain kernel is held to 1e-12 of each matrix's largest entry: products of at most
`window` rigid float64 matrices, a few ulp (2.2e-16) each."""
import functools

import numpy as np
import pytest
import torch

import visibility_reference as VR
import voxel_aggregate_reference as AR

pytestmark = pytest.mark.gpu
SHAPES = {'5x6x7-scalar': (5, 6, 7), '8x8x4-vec': (8, 8, 4)}


def _words(planes):
    return np.stack([VR.pack_seen(p) for p in planes]).view(np.int64)


@functools.lru_cache(maxsize=None)
def _case(shape_id, s, window, mix):
    classes = 2 if (s + window) % 2 else 9
    case = AR.make_case(SHAPES[shape_id], 2, s, window, classes, mix, seed=10 * s + window)
    ref = AR.solve(case)
    for a in list(case.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case, ref


def _device_case(dev, case):
    from muvo_amd import ops
    grid, bricks = ops.raycast_bricks(torch.from_numpy(case['label'].copy()).to(dev))
    seen = torch.from_numpy(_words(case['seen'])).to(dev)
    return grid, bricks, seen


@pytest.mark.parametrize('mix', ['a', 'b'])
@pytest.mark.parametrize('window', [1, 2, 6])
@pytest.mark.parametrize('s', [1, 3, 5])
@pytest.mark.parametrize('shape_id', list(SHAPES))
def test_aggregate_bytes_and_counts(dev, shape_id, s, window, mix):
    """b = 2 sequences; links of every kind (identity, whole-cell shifts, yaw with a fractional shift, roll / pitch, one that throws
    most of the grid outside, invalid ones: NaN, low fitness, a failure status); called twice in both deterministic modes into
    counts that already hold something"""
    from muvo_amd import ops
    case, ref = _case(shape_id, s, window, mix)
    assert not ref['close'].any(), 'a q of the restatement within 1e-9 of a cell face: exactness would not be a fair demand'
    masked, n = VR.masked(case['label'], case['seen'])
    assert int(ref['counts'].sum()) == int(n[1])
    if s > 1:
        assert ref['counts'].min() > 0 and ref['usable'].any()
        assert mix == 'a' or not all(AR.link_valid(T, f, st, AR.MIN_FITNESS) for T, f, st in zip(case['T'], case['fitness'], case['status']))
    else:
        assert np.array_equal(ref['out'], masked) and not ref['usable'].any()
    grid, bricks, seen = _device_case(dev, case)
    mats, usable = torch.from_numpy(ref['mats'].copy()).to(dev), torch.from_numpy(ref['usable'].copy()).to(dev)
    was = ops.get_deterministic()
    outs = []
    try:
        for mode in (False, True):
            ops.set_deterministic(mode)
            for _ in range(2):
                acc = torch.tensor([7, 1 << 40, 3], dtype=torch.int64, device=dev)
                out, counts = ops.voxel_aggregate(grid, bricks, seen, s, mats, usable, acc)
                assert counts is acc and out.dtype == torch.uint8 and out.shape == grid.shape
                assert (acc.cpu().numpy() - np.array([7, 1 << 40, 3])).tolist() == ref['counts'].tolist()
                outs.append(out.cpu().numpy())
    finally:
        ops.set_deterministic(was)
    for o in outs:
        assert np.array_equal(o, ref['out'])
    assert np.array_equal(grid.cpu().numpy(), case['label']), 'the label grid was written'
    own = masked != 255                                                 # own observations: what muvo_visibility_apply writes
    assert np.array_equal(outs[0][own], ops.visibility_apply(grid, seen)[0].cpu().numpy()[own])
    fresh = ops.voxel_aggregate(grid, bricks, seen, s, mats, usable)[1]
    assert fresh.cpu().tolist() == ref['counts'].tolist()


@pytest.mark.parametrize('mix', ['a', 'b'])
@pytest.mark.parametrize('window', [1, 2, 6])
@pytest.mark.parametrize('s', [1, 3, 5])
def test_chain_flags_exact_and_matrices(dev, s, window, mix):
    from muvo_amd import ops
    case, ref = _case('5x6x7-scalar', s, window, mix)
    T = torch.from_numpy(case['T'].copy()).to(dev)
    fitness, status = torch.from_numpy(case['fitness'].copy()).to(dev), torch.from_numpy(case['status'].copy()).to(dev)
    mats, usable = ops.voxel_pose_chain(T, 2, s, window, AR.CELL_MAP, fitness, status, AR.MIN_FITNESS)
    assert mats.shape == (2 * s, 2 * window, 12) and mats.dtype == torch.float64 and usable.shape == (2 * s, 2 * window) and usable.dtype == torch.uint8
    assert np.array_equal(usable.cpu().numpy(), ref['usable'])
    got = mats.cpu().numpy()
    scale = np.abs(ref['mats']).max(-1, keepdims=True)
    err = np.abs(got - ref['mats']) / np.where(scale > 0, scale, 1.0)
    print(f'AGGSTAT chain s{s} w{window} {mix}: max relative error {err.max():.3e} (bar 1e-12), usable {int(ref["usable"].sum())} of {ref["usable"].size}')
    assert err.max() <= 1e-12
    assert not got[ref['usable'] == 0].any(), 'a slot that is not usable holds zeros'
    # without fitness and status only finiteness decides
    _, open_flags = ops.voxel_pose_chain(T, 2, s, window, AR.CELL_MAP)
    assert np.array_equal(open_flags.cpu().numpy(), AR.chain(case['T'], 2, s, window, AR.CELL_MAP)[1])


def test_base_shape(dev):
    """192 x 192 x 64, b = 1, s = 3, window 2: the SEEN planes of the cfg's own ray table (marked on the device - held to the
    restatement bit for bit in tests/test_visibility_gpu.py), a yaw and a tilt link.  Cells whose q comes within 1e-9 of a cell
    face may be left out, at most 1e-4 of the cells (the restatement alone decides which)."""
    from muvo_amd import ops, voxel_view
    from muvo_amd.config import base_1d_cfg
    cfg = base_1d_cfg()
    cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True, 'LIDAR_STRIDE': 4, 'CAMERA_STRIDE': 8})
    shape = (192, 192, 64)
    labels = VR.base_grid(3, shape)
    grid, bricks = ops.raycast_bricks(torch.from_numpy(labels).to(dev))
    words = ops.visibility_mark(grid, bricks, voxel_view.visibility_table(cfg, 1, shape, dev))
    seen = np.stack([VR.unpack_seen(w, shape) for w in words.cpu().numpy()])
    T = np.stack([AR.pose(yaw=2.9, t=(1.13, -0.271, 0.013)), AR.pose(pitch=0.7, roll=-0.4, yaw=-1.7, t=(0.83, 0.117, -0.021))])
    cell_map = ops.voxel_cell_map(cfg, 1)
    mats, usable = AR.chain(T, 1, 3, 2, cell_map)
    out, counts, close = AR.aggregate(labels, seen, 3, mats, usable)
    left_out = int(close.sum())
    print(f'AGGSTAT base: counts {counts.tolist()}, unknown before {float((VR.masked(labels, seen)[0] == 255).mean()):.4f} after '
          f'{float((out == 255).mean()):.4f}, {left_out} cells within 1e-9 of a face')
    assert left_out <= 1e-4 * close.size and counts.min() > 0
    got, n = ops.voxel_aggregate(grid, bricks, words, 3, torch.from_numpy(mats).to(dev), torch.from_numpy(usable).to(dev))
    keep = ~close
    assert np.array_equal(got.cpu().numpy()[keep], out[keep])
    assert np.abs(n.cpu().numpy() - counts).max() <= left_out
    # the chain on the device gives the same fill
    dm, du = ops.voxel_pose_chain(torch.from_numpy(T).to(dev), 1, 3, 2, cell_map)
    assert np.array_equal(du.cpu().numpy(), usable)
    again = ops.voxel_aggregate(grid, bricks, words, 3, dm, du)[0]
    assert int((again != got).sum()) <= 1e-4 * close.size


def test_argument_errors(dev):
    from muvo_amd import ops
    case, ref = _case('5x6x7-scalar', 3, 2, 'a')
    grid, bricks, seen = _device_case(dev, case)
    mats, usable = torch.from_numpy(ref['mats'].copy()).to(dev), torch.from_numpy(ref['usable'].copy()).to(dev)
    T = torch.from_numpy(case['T'].copy()).to(dev)
    with pytest.raises(ValueError, match='sequences of 4'):
        ops.voxel_aggregate(grid, bricks, seen, 4, mats, usable)
    with pytest.raises(AssertionError, match='voxel_pose_chain'):
        ops.voxel_aggregate(grid, bricks, seen, 3, mats[:, :3].contiguous(), usable[:, :3].contiguous())
    with pytest.raises(AssertionError, match='visibility_mark'):
        ops.voxel_aggregate(grid, bricks, seen[:, :-1].contiguous(), 3, mats, usable)
    with pytest.raises(ValueError, match='link matrices'):
        ops.voxel_pose_chain(T, 2, 4, 2, AR.CELL_MAP)
    with pytest.raises(ValueError, match='window'):
        ops.voxel_pose_chain(T, 2, 3, 0, AR.CELL_MAP)
    with pytest.raises(ValueError, match='together'):
        ops.voxel_pose_chain(T, 2, 3, 2, AR.CELL_MAP, fitness=torch.ones(4, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match='map entry'):
        ops.voxel_pose_chain(T, 2, 3, 2, (0.0, 1.0, 1.0, 0.0, 0.0, 0.0))


# ---- geometry end to end -------------------------------------------------------------------------------------------------------------
def _agg_cfg(window=4, **over):
    from muvo_amd.config import base_1d_cfg
    cfg = base_1d_cfg(**over)
    cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True, 'LIDAR_STRIDE': 4, 'CAMERA_STRIDE': 8})
    cfg.VOXEL_SEG['AGGREGATE'] = type(cfg)({'ENABLED': True, 'WINDOW': window})
    return cfg


def _render(cfg, dev, ego_points):
    """ego-frame points (N, 3) float64 (x forward, y as the grid has it, z up; metres) -> (range view (4, H, W), voxel grid) by the
    project's own input pipeline: the raw lidar sweep that convert_coor_lidar turns into these points, no camera point"""
    from muvo_amd import input_pipeline as IP
    lx, ly, lz = (float(v) for v in cfg.POINTS.LIDAR_POSITION)
    raw = np.stack([ego_points[:, 0] - lx, -ego_points[:, 1] - ly, ego_points[:, 2] - lz], 1).astype(np.float32)
    pts, tag = torch.from_numpy(raw).to(dev), torch.full((len(raw),), 7, dtype=torch.uint8, device=dev)
    size, res = [int(v) for v in cfg.VOXEL.SIZE], float(cfg.VOXEL.RESOLUTION)
    far = torch.full((2, 2, 4), 255, dtype=torch.uint8, device=dev)          # a depth image of nothing: every pixel at the far plane
    vox = IP.depth_lidar_voxels(far, pts, tag, camera_position=[float(v) for v in cfg.IMAGE.CAMERA_POSITION],
                                lidar_position=[lx, ly, lz], fov=float(cfg.IMAGE.FOV), voxel_resolution=res, voxel_size=size,
                                offset=[(int(e) - n // 2) * res for e, n in zip(cfg.VOXEL.EV_POSITION, size)], dense=True)[0]
    rv, _ = IP.range_projection(pts, tag, lidar_position=(lx, ly, lz), fov=tuple(float(v) for v in cfg.POINTS.FOV),
                                H=int(cfg.POINTS.CHANNELS), W=int(cfg.POINTS.HORIZON_RESOLUTION), with_seg=False)
    return rv, (vox != 0).to(torch.uint8)


def _dilate(occ, r):
    return torch.nn.functional.max_pool3d(occ[None, None].float(), 2 * r + 1, 1, r)[0, 0] > 0


def test_geometry_end_to_end(dev):
    """a static scene - a wall 8 m ahead that shadows a cloud of points behind it - from two ego poses 1 m and 4 degrees apart.
    Frame 0 holds the wall only (the cloud is in its shadow), frame 1 holds both; the true link goes in as `voxel_ego_poses`.
    Every cell of frame 0 that is filled occupied from frame 1 lies within Chebyshev distance 2 of a cell the same points
    voxelise to in frame 0 itself (two half-cell roundings under a rotation are at most sqrt(3) cells apart); a flipped axis or
    an inverted pose fails that.  The range view of frame 1, carried through the link and the cell map, lands on those cells too."""
    from muvo_amd import ops
    from muvo_amd.data.synthetic import make_batch
    from muvo_amd.models.preprocess import PreProcess
    cfg = _agg_cfg()
    rng = np.random.default_rng(3)
    yy, zz = np.meshgrid(np.arange(-12.0, 12.0, 0.1) + 0.05, np.arange(-2.35, 10.2, 0.1))
    wall = np.stack([np.full(yy.size, 8.05), yy.reshape(-1), zz.reshape(-1)], 1)
    cloud = rng.uniform([10.0, -3.0, 0.0], [13.0, 3.0, 2.0], (3000, 3))
    cloud[:, 1] += 1.5                                                      # off the axis: a mirrored y would show
    link = AR.pose(yaw=4.0, t=(1.0, 0.3, 0.0))                              # p_0 = link p_1
    inv = np.linalg.inv(link)
    everything = np.concatenate([wall, cloud])
    in1 = everything @ inv[:3, :3].T + inv[:3, 3]
    rv0, vox0 = _render(cfg, dev, wall)
    rv1, vox1 = _render(cfg, dev, in1)
    _, direct = _render(cfg, dev, everything)                               # what the same points voxelise to in frame 0
    assert int(direct.sum()) > int(vox0.sum()) > 1000
    batch = make_batch(1, 2, seed=5, device=dev)
    batch['voxel'] = torch.stack([vox0, vox1])[None, :, None].contiguous()
    batch['range_view_pcd_xyzd'] = torch.stack([rv0, rv1])[None].contiguous()
    batch['voxel_ego_poses'] = torch.from_numpy(link)[None, None]
    pre = PreProcess(cfg).to(dev).eval()
    out = pre(batch)
    agg = out['voxel_visible_label_1'][0, 0, 0]
    filled = (agg != 0) & (agg != 255) & (vox0 == 0)
    n_filled = int(filled.sum())
    print(f'AGGSTAT geometry: {n_filled} cells filled occupied, {int((filled & ~_dilate(direct, 1)).sum())} of them farther than 1 cell, '
          f'counts {out["voxel_aggregate_counts"].cpu().tolist()}')
    assert n_filled > 100
    assert not bool((filled & ~_dilate(direct, 2)).any())
    # the map itself: range-view points of frame 1 (metres = label x LIDAR_RE.SCALE) through the link into the cells of frame 0
    rv = (out['range_view_label_1'][0, 1].double() * float(cfg.LIDAR_RE.SCALE)).cpu().numpy()
    r = rv[:3, rv[3] > 0].T
    m = np.array(ops.voxel_cell_map(cfg, 1))
    g = np.floor((r @ link[:3, :3].T + link[:3, 3]) * m[:3] + m[3:]).astype(np.int64)
    inside = ((g >= 0) & (g < np.array(agg.shape))).all(1)
    assert inside.sum() > 1000
    near = _dilate(direct, 1).cpu().numpy()
    assert near[tuple(g[inside].T)].all()


# ---- PreProcess ------------------------------------------------------------------------------------------------------------------------
def test_preprocess_icp_path_and_key_absent(dev):
    from muvo_amd import ops, voxel_view
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.data.synthetic import make_batch
    from muvo_amd.models.preprocess import PreProcess
    from muvo_amd.odometry import register_consecutive
    b, s, window = 2, 3, 2
    cfg = _agg_cfg(window)
    out = PreProcess(cfg).to(dev).eval()(make_batch(b, s, seed=21, device=dev))
    res = register_consecutive(out['range_view_label_1'], float(cfg.LIDAR_RE.SCALE), max_iteration=30, source_stride=4)
    assert res.T.shape == (b * (s - 1), 4, 4) and res.fitness.dtype == torch.float64 and res.status.dtype == torch.int64
    for f in (1, 2, 4):
        label = out[f'voxel_label_{f}']
        grid = label.reshape(-1, *label.shape[-3:])
        rays = voxel_view.visibility_table(cfg, f, tuple(grid.shape[1:]), dev)
        g, bricks = ops.raycast_bricks(grid)
        seen = ops.visibility_mark(g, bricks, rays)
        mats, usable = ops.voxel_pose_chain(res.T, b, s, window, ops.voxel_cell_map(cfg, f), res.fitness, res.status, 0.3)
        want, counts = ops.voxel_aggregate(g, bricks, seen, s, mats, usable)
        assert torch.equal(out[f'voxel_visible_label_{f}'], want.view(label.shape))
        if f == 1:
            assert torch.equal(out['voxel_aggregate_counts'], counts)
            assert int(counts.sum()) == int(ops.visibility_apply(g, seen)[1][1])
    # the key absent: the keys and bytes of the visibility mask alone; both absent: no such keys
    vis = _agg_cfg()
    vis.VOXEL_SEG.pop('AGGREGATE')
    only = PreProcess(vis).to(dev).eval()(make_batch(b, s, seed=21, device=dev))
    assert set(out) - set(only) == {'voxel_aggregate_counts'}
    for f in (1, 2, 4):
        label = only[f'voxel_label_{f}']
        grid = label.reshape(-1, *label.shape[-3:])
        want = ops.visible_labels(grid, voxel_view.visibility_table(vis, f, tuple(grid.shape[1:]), dev))[0]
        assert torch.equal(only[f'voxel_visible_label_{f}'], want.view(label.shape))
        assert torch.equal(only[f'voxel_label_{f}'], out[f'voxel_label_{f}'])
    plain = PreProcess(base_1d_cfg()).to(dev).eval()(make_batch(b, s, seed=21, device=dev))
    assert not [k for k in plain if 'visible' in k or 'aggregate' in k]
    assert set(only) - set(plain) == {'voxel_visible_label_1', 'voxel_visible_label_2', 'voxel_visible_label_4'}
    # refusals: a pose tensor of the wrong shape; no poses and no range view
    bad = make_batch(b, s, seed=21, device=dev)
    bad['voxel_ego_poses'] = torch.eye(4, dtype=torch.float64)[None, None].expand(b, s, 4, 4)
    with pytest.raises(ValueError, match='voxel_ego_poses'):
        PreProcess(cfg).to(dev).eval()(bad)
    with pytest.raises(ValueError, match='VOXEL_SEG.AGGREGATE.ENABLED needs VOXEL_SEG.VISIBILITY.ENABLED'):
        no_vis = _agg_cfg()
        no_vis.VOXEL_SEG.pop('VISIBILITY')
        PreProcess(no_vis)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trainer(dev):
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.trainer import WorldModelTrainer
    from muvo_amd.utils import detinit
    cfg = base_1d_cfg(RECEPTIVE_FIELD=2, FUTURE_HORIZON=1, STEPS=100000)
    tr = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    tr.train()
    tr.preprocess.augment = False
    detinit.fill_state_dict_(tr.model)
    for layer in tr.model.transformer_encoder.layers:
        layer.p = 0.0
    return tr


def _set_keys(tr, visibility, aggregate):
    tr.cfg.VOXEL_SEG.pop('VISIBILITY', None)
    tr.cfg.VOXEL_SEG.pop('AGGREGATE', None)
    if visibility:
        tr.cfg.VOXEL_SEG['VISIBILITY'] = type(tr.cfg)({'ENABLED': True, 'LIDAR_STRIDE': 4, 'CAMERA_STRIDE': 8})
    if aggregate:
        tr.cfg.VOXEL_SEG['AGGREGATE'] = type(tr.cfg)({'ENABLED': True, 'WINDOW': 2})


def test_training_step_with_the_key(dev, trainer):
    """one seeded training step (1 x 2 frames) with the visibility mask alone and the same step with aggregation on top, explicit
    poses, in the deterministic mode: the same loss names, only the dense voxel terms differ, the voxel decoder's gradient
    differs; the cross-entropy has exactly no gradient at a cell that is still 255 and some at a cell that was filled"""
    from muvo_amd import ops
    from muvo_amd.data.synthetic import make_batch, make_noise
    tr = trainer
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        opts, _ = tr.configure_optimizers()
        eps, use_prior = make_noise(1, 2, seed=1234)
        eps = eps.to(dev)
        head = [n for n, _ in tr.model.named_parameters() if n.startswith('voxel_decoder.')]

        def step():
            opts[0].zero_grad()
            tr.model.seed_epoch, tr.model._step_seed = 1, 0
            batch = make_batch(1, 2, seed=1234, device=dev)
            batch['voxel_ego_poses'] = torch.from_numpy(AR.pose(yaw=2.0, t=(0.7, 0.1, 0.0)))[None, None].to(dev)
            tr.training_step(batch, 0, noise=eps, use_prior=use_prior).backward()
            ops.join_side_streams()
            params = dict(tr.model.named_parameters())
            return batch, dict(tr.last_losses), {n: params[n].grad.detach().clone() for n in head}

        _set_keys(tr, True, False)
        b_vis, l_vis, g_vis = step()
        _set_keys(tr, True, True)
        b_on, l_on, g_on = step()
    finally:
        _set_keys(tr, False, False)
        ops.set_deterministic(was)
    assert list(l_on) == list(l_vis)
    assert set(b_on) - set(b_vis) == {'voxel_aggregate_counts'}
    assert all(bool(torch.isfinite(v)) for v in l_on.values())
    for k in l_on:
        same = torch.equal(l_on[k], l_vis[k])
        assert same != k.startswith(('voxel_', 'sem_scal_', 'geo_scal_')), k
    assert any(not torch.equal(g_on[n], g_vis[n]) for n in head)
    for f in (1, 2, 4):
        lab, vis, agg = b_on[f'voxel_label_{f}'], b_vis[f'voxel_visible_label_{f}'], b_on[f'voxel_visible_label_{f}']
        assert agg.shape == lab.shape and agg.dtype == torch.uint8 and torch.equal(lab, b_vis[f'voxel_label_{f}'])
        assert torch.equal(agg[vis != 255], vis[vis != 255]) and bool((agg[vis == 255] != 255).any()) and bool((agg == 255).any())
    counts = b_on['voxel_aggregate_counts'].cpu().tolist()
    vis1, agg1 = b_vis['voxel_visible_label_1'], b_on['voxel_visible_label_1']
    assert counts == [int(((vis1 == 255) & (agg1 != 255) & (agg1 != 0)).sum()), int(((vis1 == 255) & (agg1 == 0)).sum()), int((agg1 == 255).sum())]
    # the gradient of the cross-entropy on the aggregated labels of scale 4
    vis4, agg4 = b_vis['voxel_visible_label_4'], b_on['voxel_visible_label_4']
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(1, 2, 2, *agg4.shape[-3:], generator=g).to(dev).requires_grad_(True)
    ops.voxel_losses(logits, agg4, 0.1, None)[0].backward()
    grad = logits.grad.cpu()
    still = (agg4 == 255).cpu().expand(1, 2, 2, *agg4.shape[-3:])
    filled = ((vis4 == 255) & (agg4 != 255)).cpu().expand(1, 2, 2, *agg4.shape[-3:])
    assert still.any() and filled.any()
    assert not grad[still].any() and bool((grad[filled] != 0).all())


def test_evaluation_logs_the_shares(dev, trainer):
    """one validation pass with the key on and poses from ICP: the two new names follow `_Voxel_Unknown_Share` in both metric sets
    and equal the host's count over the whole batch"""
    from muvo_amd import ops, voxel_view
    from muvo_amd.data.synthetic import make_batch, make_noise
    from muvo_amd.trainer import metric_log_names, metric_names
    tr = trainer
    rf, fh, ns = tr.rf, tr.fh, tr.cfg.PREDICTION.N_SAMPLES
    eps, use_prior = make_noise(1, rf + ns * fh, seed=77)
    batch = make_batch(1, rf + fh, seed=77, device=dev)
    sent = []
    _set_keys(tr, True, False)
    before = metric_log_names(tr.cfg, 'val0')
    _set_keys(tr, True, True)
    tr.log_fn = lambda name, value: sent.append((name, value))
    try:
        assert metric_log_names(tr.cfg, 'val0') == before + ['val0_Voxel_Filled_Share', 'val0_Voxel_Unknown_Share_Aggregated']
        assert metric_names(tr.cfg, 'val0')[-2:] == ['val0_Voxel_Filled_Share', 'val0_Voxel_Unknown_Share_Aggregated']
        for m in (tr.metrics_vals[0], tr.metrics_vals_imagine[0]):
            m.clear()
        tr.validation_step(batch, noise=eps.to(dev), use_prior=use_prior, cd_index=np.arange(10000))
        assert 'filled' in tr.metrics_vals[0] and 'filled' in tr.metrics_vals_imagine[0]
        tr.on_validation_epoch_end()
        names = [n for n, _ in sent]
        want = metric_log_names(tr.cfg, 'val0') + metric_log_names(tr.cfg, 'val_imagine0')
        assert [n for n in names if n in want] == want
        cfg_on = tr.cfg.clone()
    finally:
        tr.log_fn = None
        _set_keys(tr, False, False)
        for m in (tr.metrics_vals[0], tr.metrics_vals_imagine[0]):
            m.clear()
    logged = dict(sent)
    agg = batch['voxel_visible_label_1']
    label = batch['voxel_label_1']
    grid = label.reshape(-1, *label.shape[-3:])
    vis = ops.visible_labels(grid, voxel_view.visibility_table(cfg_on, 1, tuple(grid.shape[1:]), dev))[0].view(label.shape)
    unknown = int((agg == 255).sum()) / agg.numel()
    filled = (int((vis == 255).sum()) - int((agg == 255).sum())) / agg.numel()
    assert torch.equal(agg[vis != 255], vis[vis != 255])
    print(f'AGGSTAT evaluation: single-frame unknown {int((vis == 255).sum()) / agg.numel():.4f}, filled {filled:.4f}, unknown after {unknown:.4f}')
    for prefix in ('val0', 'val_imagine0'):
        assert float(logged[f'{prefix}_Voxel_Filled_Share']) == filled
        assert float(logged[f'{prefix}_Voxel_Unknown_Share_Aggregated']) == unknown
    assert float(logged['val0_Voxel_Unknown_Share']) == int((vis[:, :rf] == 255).sum()) / vis[:, :rf].numel()   # keeps its meaning
