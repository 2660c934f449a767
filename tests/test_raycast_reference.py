"""CPU: the float32 restatement of the ray march (tests/raycast_reference.py) against a float64 brute-force ray / box search, the
hand-made rays, the counts rule and the figures of RayIoUMetric, the ray generators, the command-line flags, the exports and the
argument validation of the new entry points (no GPU anywhere)."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import raycast_reference as R  # noqa: E402

NEW_EXPORTS = ('muvo_raycast_brick_words', 'muvo_raycast_bricks_grid', 'muvo_raycast_bricks_logits', 'muvo_raycast', 'muvo_panel_voxel_view',
               'muvo_ray_iou_ws_doubles', 'muvo_ray_iou_counts')


def test_restatement_equals_the_brute_force_search():
    g = R.scene()
    rays = R.scene_rays()
    assert rays.shape == (832, 7) and g.shape == (13, 10, 7) and g.dtype == np.uint8
    hit, t, face = R.cast(g, rays)
    aside, bad = 0, []
    for k, ray in enumerate(rays):
        want, tw, gap = R.brute_force(g, ray)
        if gap < 1e-4:
            aside += 1
            continue
        if want != hit[k] or (want >= 0 and abs(float(t[k]) - tw) > 1e-4 * abs(tw)):
            bad.append((k, want, tw, int(hit[k]), float(t[k])))
    print(f'{len(rays)} rays: {int((hit >= 0).sum())} hit, {aside} set aside as near-ties, {len(bad)} disagree')
    assert aside <= 0.01 * len(rays) and not bad, bad
    assert 100 < (hit >= 0).sum() < 800
    hand = [R.march(g, np.array(r, np.float32)) for _, r, _ in R.hand_rays(g)]
    faces = set(face[hit >= 0].tolist()) | {f for h, _, f in hand if h >= 0}
    assert faces == {0, 1, 2, 3}, faces
    # the second scene too (the unpadded brick path of the kernels)
    q = R.cube_scene()
    qr = np.concatenate([R.camera_rays(8, 8, 8, 12), R.fan_rays((2.5, 4.5, 3.5), 4, 16, 10.0, -30.0)])
    hit, t, _ = R.cast(q, qr)
    for k, ray in enumerate(qr):
        want, tw, gap = R.brute_force(q, ray)
        assert gap < 1e-4 or (want == hit[k] and (want < 0 or abs(float(t[k]) - tw) <= 1e-4 * abs(tw))), (k, want, tw, hit[k], t[k])


def test_hand_made_rays():
    g = R.scene()
    for name, ray, want in R.hand_rays(g):
        got = R.march(g, np.array(ray, np.float32))
        if want is not None:
            assert got[0] == want[0] and got[2] == want[2] and np.float32(got[1]) == np.float32(want[1]), (name, got, want)
        if all(math.isfinite(v) for v in ray[:6]) and any(ray[3:6]):
            bf = R.brute_force(g, np.array(ray, np.float32))
            assert bf[0] == got[0] and abs(bf[1] - float(got[1])) <= 1e-4 * max(bf[1], 1e-9), (name, got, bf)
    names = [n for n, _, _ in R.hand_rays(g)]
    assert len(names) == len(set(names)) >= 10
    inside = R.march(g, np.array(R.hand_rays(g)[2][1], np.float32))
    assert inside[0] >= 0 and inside[2] == 0                                   # the axis-parallel ray inside meets a wall through a face x
    hit, t, face = R.march(R.corner_scene(), np.array(R.CORNER_RAY, np.float32))
    assert hit == (12 * 10 + 9) * 7 + 6 and face == 0 and abs(float(t) - 12 / 13) < 1e-6
    # the loop bound holds for rays that cross the whole empty grid
    empty = np.zeros((13, 10, 7), np.uint8)
    assert R.march(empty, np.array(R.CORNER_RAY, np.float32)) == R.MISS


def test_brick_packing():
    g = np.zeros((5, 6, 9), np.uint8)
    g[4, 5, 8] = 3
    g[0, 0, 0] = 1
    w = R.pack_bricks(g)
    assert w.shape == (2 * 2 * 3,) and w.dtype == np.uint64
    assert int(w[0]) == 1 and int(w[(1 * 2 + 1) * 3 + 2]) == 1 << (0 * 16 + 1 * 4 + 0) and np.count_nonzero(w) == 2


def test_counts_rule():
    hits_l = [(2, 1.0), (2, 1.0), (2, 1.0), (-1, 0.0), (3, 5.0), (-1, 0.0), (1, 2.0)]
    hits_p = [(2, 1.5), (2, 9.0), (4, 1.0), (4, 2.0), (-1, 0.0), (-1, 0.0), (1, 2.0 + 5.0)]
    counts, terms = R.iou_counts(hits_l, hits_p, 6, res=0.5)
    # ray 0: |dt| 0.25 m tp[2] at all thresholds; ray 1: 4 m: tp only at 4 m; ray 2: classes differ: fn[2], fp[4]; ray 3: fp[4];
    # ray 4: fn[3]; ray 5: nothing; ray 6: 2.5 m: tp[1] at 4 m only
    want = np.zeros((3, 6, 3), np.int64)
    want[:, 2, 0] += 1
    want[2, 2, 0] += 1
    want[:2, 2, 2] += 1
    want[:2, 2, 1] += 1
    want[:, 2, 2] += 1
    want[:, 4, 1] += 2
    want[:, 3, 2] += 1
    want[2, 1, 0] += 1
    want[:2, 1, 1] += 1
    want[:2, 1, 2] += 1
    assert np.array_equal(counts, want), counts - want
    assert terms.dtype == np.float32 and terms.tolist() == [0.25, 4.0, 0.0, 2.5]
    means = R.ray_iou(counts)
    # at 1 m: class 1 0/2, class 2 1/4, class 3 0/1, class 4 0/2, class 5 absent; at 4 m: class 1 1/1, class 2 2/3
    assert means[0] == pytest.approx((0 + 1 / 4 + 0 + 0) / 4) and means[2] == pytest.approx((1 + 2 / 3 + 0 + 0) / 4)


def test_ray_iou_metric_from_hand_made_counts(tmp_path):
    torch = pytest.importorskip('torch')
    from muvo_amd.voxel_view import RayIoUMetric, ray_iou_from_counts
    counts = np.zeros((2, 3, 5, 3), np.int64)
    counts[0, :, 0] = (7, 7, 7)                                 # class 0 never enters the mean
    counts[0, 0, 1] = (1, 2, 1)
    counts[0, 1, 1] = (2, 1, 1)
    counts[0, 2, 1] = (4, 0, 0)
    counts[0, :, 3] = (0, 3, 0)                                 # class 2 and 4 absent, class 3 only false positives
    m = RayIoUMetric(types.SimpleNamespace(), prefix='test')
    m.start_loader(2)
    m.acc['2'] = dict(counts=torch.from_numpy(counts), depth=torch.tensor([[6.0, 4.0], [0.0, 0.0]], dtype=torch.float64))
    m.start_loader(1)                                           # a loader without a batch
    res = m.result()
    keys = [f'ray_iou_{k}m' for k in (1, 2, 4)] + ['ray_iou', 'ray_iou_per_class', 'ray_depth_l1', 'ray_pairs']
    assert set(res) == {f'test{i}_{k}{tail}' for i in (1, 2) for k in keys for tail in ('', '_imagine')}
    assert res['test2_ray_iou_1m'] == pytest.approx((1 / 4 + 0) / 2) and res['test2_ray_iou_2m'] == pytest.approx((2 / 4 + 0) / 2)
    assert res['test2_ray_iou_4m'] == pytest.approx((4 / 4 + 0) / 2)
    assert res['test2_ray_iou'] == pytest.approx((res['test2_ray_iou_1m'] + res['test2_ray_iou_2m'] + res['test2_ray_iou_4m']) / 3)
    assert res['test2_ray_iou_per_class'][0] == [pytest.approx(1 / 3), 0.25, None, 0.0, None]
    assert res['test2_ray_depth_l1'] == 1.5 and res['test2_ray_pairs'] == 4
    # all misses / no batch: zeros, nothing divides by zero
    for k in ('test2_ray_iou_imagine', 'test2_ray_iou_1m_imagine', 'test2_ray_depth_l1_imagine', 'test1_ray_iou', 'test1_ray_iou_4m', 'test1_ray_depth_l1'):
        assert res[k] == 0.0
    assert res['test1_ray_pairs'] == 0 and res['test2_ray_pairs_imagine'] == 0
    means, per_class = ray_iou_from_counts(counts[0].tolist())
    assert means == pytest.approx(R.ray_iou(counts[0]))
    import json
    path = m.write(str(tmp_path))
    assert os.path.basename(path) == 'ray_iou.json' and json.load(open(path)) == res


def test_ray_generators():
    from muvo_amd.config import get_cfg
    from muvo_amd.voxel_view import camera_rays, lidar_rays
    cam = camera_rays(13, 10, 7, 24)
    assert cam.shape == (576, 7) and cam.dtype == np.float32 and np.array_equal(cam, R.camera_rays(13, 10, 7, 24))
    half = 0.5 * math.sqrt(13 * 13 + 10 * 10 + 7 * 7)
    e, a = math.radians(60), math.radians(165)
    back = np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)])
    assert np.allclose(cam[:, 3:6], -back, atol=1e-7) and np.allclose(cam[:, 6], 4 * half)
    mid = cam.reshape(24, 24, 7)[11:13, 11:13, :3].mean(axis=(0, 1))           # the four central pixels surround the view axis
    assert np.allclose(mid, np.array([13, 10, 7]) / 2 + 2 * half * back, atol=1e-5)
    assert cam.reshape(24, 24, 7)[0, 0, 2] > cam.reshape(24, 24, 7)[23, 0, 2]  # row 0 is the top of the picture
    cfg = get_cfg()
    rays = lidar_rays(cfg, stride=4)
    H, W = cfg.POINTS.CHANNELS, cfg.POINTS.HORIZON_RESOLUTION
    assert (H, W, list(cfg.POINTS.FOV)) == (64, 1024, [-30, 10]) and rays.shape == (64 * 256, 7) and rays.dtype == np.float32
    assert np.array_equal(rays, R.fan_rays((32 + 1.0 / 0.2, 96.0, 12 + 2.0 / 0.2), 64, 1024, 10.0, -30.0).reshape(64, 1024, 7)[:, ::4].reshape(-1, 7))
    assert np.all(rays[:, :3] == np.float32([37, 96, 22])) and np.isinf(rays[:, 6]).all()
    assert np.allclose(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1), 1.0, atol=1e-6)
    first = rays[0, 3:6]
    p, y = math.radians(10 - 40 * 0.5 / 64), math.pi * (1 - 1 / 1024)
    assert np.allclose(first, [math.cos(p) * math.cos(y), math.cos(p) * math.sin(y), math.sin(p)], atol=1e-7)
    assert lidar_rays(cfg, stride=8).shape == (64 * 128, 7) and lidar_rays(cfg, stride=1000).shape == (64 * 2, 7)
    with pytest.raises(ValueError):
        lidar_rays(cfg, stride=0)


def test_parsers():
    from muvo_amd import predict, train
    base = ['--out', 'o', '--mode', 'test']
    a = predict.parse_args(base + ['--ray-iou', '--ray-stride', '8', '--voxel', '--panels', '1', '--voxel-size', '64'])
    assert a.ray_iou and a.ray_stride == 8 and a.voxel and a.voxel_size == 64 and a.panels == 1
    d = predict.parse_args(base)
    assert not d.ray_iou and not d.voxel and d.ray_stride == 4 and d.voxel_size == 256
    with pytest.raises(SystemExit):
        predict.parse_args(base + ['--voxel'])
    with pytest.raises(SystemExit, match='--mode test'):
        predict.parse_args(['--out', 'o', '--mode', 'sim', '--ray-iou'])
    with pytest.raises(SystemExit):
        predict.parse_args(base + ['--ray-iou', '--ray-stride', '0'])
    t = train.build_parser().parse_args(['--panel-dir', 'p', '--voxel', '--voxel-size', '64'])
    assert t.voxel and t.voxel_size == 64 and not train.build_parser().parse_args([]).voxel


def test_exports():
    from muvo_amd import ops
    assert set(NEW_EXPORTS) <= set(ops.EXPORTS)
    L = ops.lib()
    assert all(hasattr(L, n) for n in NEW_EXPORTS)


def test_argument_validation_without_gpu():
    """every entry refuses bad arguments before it touches the device"""
    from muvo_amd import ops
    L = ops.lib()
    p = C.c_void_p(4096)                                        # never dereferenced: the calls below are refused first
    null, st = C.c_void_p(0), C.c_void_p(0)
    i64 = C.c_int64
    place = ops.TilePlace(3 * 100 * 100, 100 * 100, 100, 100, 1, 0, 0, 0, 0, 0, ops.PANEL_NO_SEP, 0)
    thr = (C.c_float * 3)(1, 2, 4)

    def refused(rc, word):
        assert rc == -1 and word in L.muvo_last_error(), (rc, L.muvo_last_error())
    assert L.muvo_raycast_brick_words(2, 13, 10, 7) == 2 * 4 * 3 * 2 and L.muvo_raycast_brick_words(1, 192, 192, 64) == 48 * 48 * 16
    assert L.muvo_raycast_brick_words(1, 0, 4, 4) == -1 and L.muvo_raycast_brick_words(0, 4, 4, 4) == -1 and L.muvo_raycast_brick_words(1, 4, 4, 4096) == -1
    assert L.muvo_ray_iou_ws_doubles(i64(3), i64(257)) == 3 * 2 * 2 and L.muvo_ray_iou_ws_doubles(i64(3), i64(0)) == -1
    refused(L.muvo_raycast_bricks_grid(null, 1, 8, 8, 8, p, i64(8), st), b'null pointer')
    refused(L.muvo_raycast_bricks_grid(p, 1, 8, 8, 8, p, i64(7), st), b'brick words')
    refused(L.muvo_raycast_bricks_logits(p, 1, 17, 8, 8, 8, p, p, i64(8), st), b'C = 17')
    refused(L.muvo_raycast_bricks_logits(p, 1, 9, 8, 8, 8, null, p, i64(8), st), b'null pointer')
    refused(L.muvo_raycast(p, p, 1, 8, 8, 8, p, i64(0), p, p, p, st), b'0 rays')
    refused(L.muvo_raycast(p, null, 1, 8, 8, 8, p, i64(5), p, p, p, st), b'null pointer')
    refused(L.muvo_raycast(p, p, 1, 8, 0, 8, p, i64(5), p, p, p, st), b'grid 8 x 0 x 8')
    refused(L.muvo_panel_voxel_view(p, p, 1, 8, 8, 8, p, 0, p, 2, 204, p, i64(30000), C.byref(place), st), b'R = 0')
    refused(L.muvo_panel_voxel_view(p, p, 1, 8, 8, 8, p, 24, null, 2, 204, p, i64(30000), C.byref(place), st), b'null pointer')
    refused(L.muvo_panel_voxel_view(p, p, 1, 8, 8, 8, p, 97, p, 2, 204, p, i64(30000), C.byref(place), st), b'leaves the')
    refused(L.muvo_panel_voxel_view(p, p, 1, 8, 8, 8, p, 24, p, 2, 204, p, i64(29999), C.byref(place), st), b'too small')
    refused(L.muvo_ray_iou_counts(p, p, p, p, 1, 17, 8, 8, 8, p, i64(5), C.c_float(0.2), thr, p, p, i64(2), p, st), b'C = 17')
    refused(L.muvo_ray_iou_counts(p, p, p, p, 1, 9, 8, 8, 8, p, i64(0), C.c_float(0.2), thr, p, p, i64(2), p, st), b'0 rays')
    refused(L.muvo_ray_iou_counts(p, p, null, p, 1, 9, 8, 8, 8, p, i64(5), C.c_float(0.2), thr, p, p, i64(2), p, st), b'null pointer')
    refused(L.muvo_ray_iou_counts(p, p, p, p, 1, 9, 8, 8, 8, p, i64(5), C.c_float(0.2), thr, p, p, i64(1), p, st), b'workspace')
    refused(L.muvo_ray_iou_counts(p, p, p, p, 1, 9, 8, 8, 8, p, i64(5), C.c_float(0.0), thr, p, p, i64(2), p, st), b'resolution')
