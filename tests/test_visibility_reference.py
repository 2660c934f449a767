"""CPU: the sensor-visibility mask of the voxel labels without a GPU - the config accessor, the ray tables of
muvo_amd/voxel_view.py, and the properties of the numpy restatement (tests/visibility_reference.py) the device kernels are
compared with in tests/test_visibility_gpu.py."""
import math

import numpy as np
import pytest

import raycast_reference as RC
import visibility_reference as VR
from muvo_amd import config, voxel_view

inf = math.inf


def _cfg(**vis):
    node = {'VOXEL_SEG': {'ENABLED': True, 'VISIBILITY': vis}} if vis else {'VOXEL_SEG': {'ENABLED': True}}
    return config.get_cfg(cfg_dict=node)


# ---- the config accessor -----------------------------------------------------------------------------------------------------------
def test_absent_is_off_and_the_defaults_do_not_carry_the_key():
    import yaml
    cfg = config.get_cfg()
    assert 'VISIBILITY' not in cfg.VOXEL_SEG and 'VISIBILITY' not in config.base_1d_cfg().VOXEL_SEG
    assert config.voxel_visibility(cfg) == (False, 1, 2)
    assert 'VISIBILITY' not in yaml.safe_dump(config.base_1d_cfg().convert_to_dict())
    from muvo_amd.trainer import metric_log_names, metric_names
    assert not [n for n in metric_names(cfg, 'val0') + metric_log_names(cfg, 'val0') if 'Unknown' in n]


def test_defaults_and_values():
    assert config.voxel_visibility(_cfg(ENABLED=True)) == (True, 1, 2)
    assert config.voxel_visibility(_cfg(ENABLED=True, LIDAR_STRIDE=4, CAMERA_STRIDE=8)) == (True, 4, 8)
    assert config.voxel_visibility(_cfg(ENABLED=False, CAMERA_STRIDE=3)) == (False, 1, 3)
    cfg = config.get_cfg(cfg_dict=_cfg(ENABLED=True, LIDAR_STRIDE=2).convert_to_dict())            # the dict a checkpoint carries
    assert config.voxel_visibility(cfg) == (True, 2, 2)
    for key in ('VOXEL_SEG.VISIBILITY', 'VOXEL_SEG.VISIBILITY.ENABLED', 'VOXEL_SEG.VISIBILITY.LIDAR_STRIDE', 'VOXEL_SEG.VISIBILITY.CAMERA_STRIDE'):
        assert key in config.EXTENSION_KEYS


def test_metric_names_list_the_share_only_with_the_key_on():
    from muvo_amd.trainer import metric_log_names, metric_names
    cfg = _cfg(ENABLED=True)
    assert metric_names(cfg, 'val0')[-1] == 'val0_Voxel_Unknown_Share' and metric_names(cfg, 'val0')[-2] == 'val0_Voxel_Recall'
    assert metric_log_names(cfg, 'test1')[-1] == 'test1_Voxel_Unknown_Share'
    off = _cfg(ENABLED=False)
    assert metric_names(off, 'val0') == metric_names(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True}}), 'val0')


@pytest.mark.parametrize('key', ['LIDAR_STRIDE', 'CAMERA_STRIDE'])
@pytest.mark.parametrize('stride', [0, -1, 1.5, True, '2', None])
def test_bad_strides_raise(key, stride):
    with pytest.raises(ValueError, match=key):
        config.voxel_visibility(_cfg(ENABLED=True, **{key: stride}))


@pytest.mark.parametrize('enabled', [1, 'yes', 0.0])
def test_bad_enabled_raises(enabled):
    with pytest.raises(ValueError, match='ENABLED'):
        config.voxel_visibility(_cfg(ENABLED=enabled))


def test_the_two_refusals():
    with pytest.raises(ValueError, match='VOXEL_SEG.ENABLED'):
        config.voxel_visibility(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False, 'VISIBILITY': {'ENABLED': True}}}))
    with pytest.raises(ValueError, match='USE_TOP_K'):
        config.voxel_visibility(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': True, 'USE_TOP_K': True, 'VISIBILITY': {'ENABLED': True}}}))
    # off: neither refusal
    assert not config.voxel_visibility(config.get_cfg(cfg_dict={'VOXEL_SEG': {'ENABLED': False, 'USE_TOP_K': True, 'VISIBILITY': {'ENABLED': False}}}))[0]


# ---- camera_label_rays ---------------------------------------------------------------------------------------------------------------
def test_camera_label_rays_shape_norm_origin_axis():
    cfg = config.get_cfg()
    H, W = cfg.IMAGE.SIZE
    for stride in (1, 2, 7):
        rays = voxel_view.camera_label_rays(cfg, stride)
        assert rays.dtype == np.float32 and rays.shape == (math.ceil(H / stride) * math.ceil(W / stride), 7)
        assert np.abs(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1) - 1).max() < 1e-6
        assert np.isposinf(rays[:, 6]).all()
        fwd, right, up = cfg.IMAGE.CAMERA_POSITION
        want = np.array(cfg.VOXEL.EV_POSITION, np.float64) + np.array([fwd, -right, up]) / cfg.VOXEL.RESOLUTION
        assert np.array_equal(rays[:, :3], np.broadcast_to(want.astype(np.float32), (len(rays), 3)))
    # the pixel (H / 2, W / 2) is the principal point of csrc/voxelize.hip (pixel corners): its ray is the optical axis, +x of the grid
    rays = voxel_view.camera_label_rays(cfg, 2).reshape(H // 2, W // 2, 7)
    assert np.array_equal(rays[H // 4, W // 4, 3:6], np.float32([1, 0, 0]))
    # column 0 looks to +y (the camera's left), row 0 up; the horizontal field of view is IMAGE.FOV from column 0 to column W
    assert rays[H // 4, 0, 4] > 0 and rays[0, W // 4, 5] > 0
    d = rays[H // 4, 0, 3:6].astype(np.float64)
    assert abs(math.degrees(math.atan2(d[1], d[0])) - cfg.IMAGE.FOV / 2) < 1e-4
    with pytest.raises(ValueError):
        voxel_view.camera_label_rays(cfg, 0)


def test_visibility_table_row_order_and_origin_scaling():
    cfg = _cfg(ENABLED=True, LIDAR_STRIDE=16, CAMERA_STRIDE=40)
    lidar, camera = voxel_view.lidar_rays(cfg, 16), voxel_view.camera_label_rays(cfg, 40)
    for factor in (1, 2, 4):
        shape = tuple(n // factor for n in cfg.VOXEL.SIZE)
        table = voxel_view.visibility_table(cfg, factor, shape, 'cpu')
        assert table is voxel_view.visibility_table(cfg, factor, shape, 'cpu')                 # cached
        t = table.numpy()
        assert t.dtype == np.float32 and t.shape == (len(lidar) + len(camera), 7)
        both = np.concatenate([lidar, camera])
        assert np.array_equal(t[:, 3:], both[:, 3:])
        assert np.array_equal(t[:, :3], (both[:, :3].astype(np.float64) / factor).astype(np.float32))
    assert not np.array_equal(lidar[0, :3], camera[0, :3]) or cfg.POINTS.LIDAR_POSITION == cfg.IMAGE.CAMERA_POSITION


# ---- the restatement on hand-made grids ------------------------------------------------------------------------------------------------
def _cells_on_segment(shape, ray, n=20001):
    """float64, no traversal: the cells whose interior the ray's segment inside the box passes, by dense sampling"""
    o, d = np.asarray(ray[:3], np.float64), np.asarray(ray[3:6], np.float64)
    ts = np.linspace(0, 4 * max(shape), n)
    p = o + ts[:, None] * d
    ok = ((p >= 0) & (p < np.array(shape))).all(1)
    return {tuple(int(v) for v in np.floor(q)) for q in p[ok]}


def test_empty_grid_origin_inside_every_cell_up_to_the_exit_is_seen():
    g = np.zeros((9, 7, 5), np.uint8)
    for ray in ([4.3, 3.6, 2.2, 0.7, 0.5, 0.3, inf], [4.3, 3.6, 2.2, -0.2, 0.9, -0.4, inf], [4.5, 3.5, 2.5, 1, 0, 0, inf]):
        cells = VR.visited(g, ray)
        assert len(set(cells)) == len(cells) and cells[0] == (4, 3, 2)
        assert all(abs(a[0] - b[0]) + abs(a[1] - b[1]) + abs(a[2] - b[2]) == 1 for a, b in zip(cells, cells[1:]))       # face neighbours
        last = cells[-1]
        assert last[0] in (0, 8) or last[1] in (0, 6) or last[2] in (0, 4)                                          # ends at a face of the box
        assert _cells_on_segment(g.shape, ray) <= set(cells)                                                       # nothing on the ray is left out
    assert VR.seen_grid(g, [[4.5, 3.5, 2.5, 1, 0, 0, inf]]).sum() == 5                                                # x = 4..8


def test_a_wall_is_seen_and_nothing_behind_it():
    g = np.zeros((9, 7, 5), np.uint8)
    g[6] = 4
    rays = [[0.5, y + 0.5, z + 0.5, 1, 0, 0, inf] for y in range(7) for z in range(5)]
    seen = VR.seen_grid(g, rays)
    assert seen[:7].all() and not seen[7:].any()
    out, counts = VR.masked(g, seen)
    assert (out[:6] == 0).all() and (out[6] == 4).all() and (out[7:] == 255).all()
    assert counts.tolist() == [6 * 35, 2 * 35]


def test_origin_cell_occupied_marks_only_that_cell():
    g = np.zeros((5, 6, 7), np.uint8)
    g[2, 3, 4] = 1
    assert VR.visited(g, [2.5, 3.25, 4.75, 0.3, -0.2, 0.1, inf]) == [(2, 3, 4)]


@pytest.mark.parametrize('ray', [[-3.0, -3.0, 20.0, -1, 0, 0.5, inf], [2.5, 10.5, 9.0, 0, 0, -1, inf], [math.nan, 3.5, 3.5, 1, 0, 0, inf],
                                 [2.5, 3.5, 2.0, math.nan, 0, -1, inf], [2.5, 3.5, 9.0, 0, 0, -1, math.nan], [2.5, 2.5, 2.5, 0, 0, 0, inf],
                                 [2.5, 3.5, 9.0, 0, 0, -inf, inf], [1.5, 1.5, 1.5, 1, 0, 0, 0.0]])
def test_a_miss_before_step_2_marks_nothing(ray):
    g = VR.edge_grid((5, 6, 7), 0)
    assert VR.visited(g, ray) == [] and not VR.seen_grid(g, [ray]).any()


def test_finite_tmax_ends_the_ray_mid_grid():
    g = np.zeros((9, 7, 5), np.uint8)
    assert VR.visited(g, [0.5, 3.5, 2.5, 1, 0, 0, 2.75]) == [(0, 3, 2), (1, 3, 2), (2, 3, 2), (3, 3, 2)]  # it ends at x = 3.25: best = 3.5 > t1


def test_corner_ties_go_x_before_y_before_z():
    g = np.zeros((3, 3, 3), np.uint8)
    assert VR.visited(g, [0, 0, 0, 1, 1, 1, inf]) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]


@pytest.mark.parametrize('shape', [(5, 6, 7), (8, 8, 4)])
def test_table_form_equals_the_march_and_the_counts_add_up(shape):
    """seen_table (all rays at once) against seen_grid (RC.march ray by ray) on the inputs of the GPU tests; occupied cells are never
    255; counts[0] + counts[1] + occupied = X Y Z F"""
    frames = [VR.edge_grid(shape, 1), VR.edge_grid(shape, 2)]
    total = 0
    for g in frames:
        rays = np.array([r for _, r in VR.edge_rays(g)] + [VR.CROWD_RAY], np.float32)
        seen = VR.seen_grid(g, rays)
        assert np.array_equal(VR.seen_table(g, rays), seen)
        assert seen.any() and not seen.all()
        out, counts = VR.masked(g, seen)
        assert np.array_equal(out[g != 0], g[g != 0]) and not (out[g != 0] == 255).any()
        assert set(np.unique(out[g == 0])) == {0, 255}
        total += counts.sum() + int((g != 0).sum())
        assert np.array_equal(VR.unpack_seen(VR.pack_seen(seen), shape), seen)
        # every ray alone: its hit cell, when it hits, is among the cells it marks - the last one
        for ray in rays:
            hit = RC.march(g, ray)[0]
            cells = VR.visited(g, ray)
            if hit >= 0:
                x, y, z = cells[-1]
                assert (x * shape[1] + y) * shape[2] + z == hit
            assert all(g[c] == 0 for c in cells[:-1])
    assert total == 2 * shape[0] * shape[1] * shape[2]


def test_base_shaped_inputs_have_a_mixed_mask():
    """the base-shaped case of the GPU tests at a quarter of its size per axis (the same construction, the cfg's table at scale 4):
    the restatement's unknown share must lie in [0.05, 0.95] - an all-0 or all-255 mask would let a broken kernel pass"""
    cfg = _cfg(ENABLED=True, LIDAR_STRIDE=4, CAMERA_STRIDE=8)
    g = VR.base_grid(2, (48, 48, 16))
    g[:, 30] = 3
    rays = voxel_view.visibility_table(cfg, 4, (48, 48, 16), 'cpu').numpy()
    for frame in g:
        out, counts = VR.masked(frame, VR.seen_table(frame, rays))
        assert 0.05 <= counts[1] / frame.size <= 0.95 and counts[0] > 0
