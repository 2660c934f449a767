"""Voxel labels from depth images and lidar sweeps (input_pipeline.depth_lidar_voxels, muvo_amd/csrc/voxelize.hip, the tool
muvo_amd.generate_voxels): the reference's data/generate_voxels.py::voxelize_one.
CPU: the numpy restatement (tests/voxelize_reference.py) against the rows the REAL reference functions produced
(tests/golden/voxelize.npz, tools/golden/make_golden_voxelize.py) - bit for bit - and on hand-made edge cases; the argument
validation of the C entry.  GPU: the HIP kernels against the same fixture and the same edge cases - bit for bit (the selection is
integer work on exactly reproduced float64 arithmetic)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import voxelize_reference as VR

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'voxelize.npz')
SETS = ('dataset', 'preprocess_yaml')
SKY = (255, 255, 255, 13)          # depth code of 1000 m: not a point


def _params(g, name):
    return dict(camera_position=g['camera_position'].tolist(), lidar_position=g['lidar_position'].tolist(), fov=int(g['fov']),
                voxel_resolution=float(g[f'resolution_{name}']), voxel_size=g['voxel_size'].tolist(), offset=g[f'offset_{name}'].tolist())


def _sky(H=2, W=2):
    return np.tile(np.array(SKY, np.uint8), (H, W, 1))


def _pixel(img, y, x, code, tag):
    img[y, x] = (code >> 16, (code >> 8) & 255, code & 255, tag)
    return img


def _small(**kw):
    """lidar at the ego origin, so a raw point (x, y, z) is the ego point (x, -y, z); grid x, y in [-2, 2), z in [-1, 1)."""
    p = dict(camera_position=[1.0, 0.0, 2.0], lidar_position=[0.0, 0.0, 0.0], fov=110, voxel_resolution=0.5, voxel_size=[8, 8, 4],
             offset=[0.0, 0.0, 0.0], mask_ego=False)
    p.update(kw)
    return p


def edge_cases():
    """[(name, depth_semantic, points_xyz, obj_tag, params, expected rows)]"""
    f32, u8 = np.float32, np.uint8
    none = np.zeros((0, 4), np.int64)
    cases = [('empty sweep, all-sky image', _sky(4, 6), np.zeros((0, 3), f32), np.zeros(0, u8), _small(), none)]
    # b == 0 is inside (first voxel), b == hi is outside
    cases.append(('grid faces', _sky(), f32([[-2.0, 2.0, -1.0], [2.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 1.0]]), u8([3, 4, 5, 7]), _small(),
                  np.array([[0, 0, 0, 3]], np.int64)))
    # ego box, strict on both sides: z == 0 (lower face) stays, the interior goes, the float32 neighbours of x/2 split
    big = _small(voxel_size=[40, 24, 8], mask_ego=True)
    below, above = np.nextafter(f32(4.902 / 2), f32(0)), np.nextafter(f32(4.902 / 2), f32(9))
    assert float(below) < 4.902 / 2 < float(above)
    cases.append(('ego box', _sky(), f32([[0.5, -0.3, 0.0], [0.5, -0.3, 0.25], [below, 0.0, 0.3], [above, 0.0, 0.3], [0.0, 1.0, 1.5]]),
                  u8([1, 2, 3, 4, 5]), big, np.array([[21, 12, 4, 1], [24, 12, 4, 4]], np.int64)))
    # the centre pixel of a 2 x 2 image looks along the axis: x = y = 0, range = depth
    wide = _small(voxel_resolution=10.0, voxel_size=[256, 16, 16], max_range=2000.0)
    cases.append(('depth just below 1000 is a point', _pixel(_sky(), 1, 1, 0xfffffe, 9), np.zeros((0, 3), f32), np.zeros(0, u8), wide,
                  np.array([[228, 8, 8, 9]], np.int64)))
    cases.append(('depth == 1000 is none', _pixel(_sky(), 1, 1, 0xffffff, 9), np.zeros((0, 3), f32), np.zeros(0, u8), wide, none))
    rng = _small(voxel_resolution=1.0, voxel_size=[256, 16, 16])
    cases.append(('range just below max_range', _pixel(_sky(), 1, 1, 1677721, 9), np.zeros((0, 3), f32), np.zeros(0, u8), rng,
                  np.array([[228, 8, 10, 9]], np.int64)))
    cases.append(('range just above max_range', _pixel(_sky(), 1, 1, 1677722, 9), np.zeros((0, 3), f32), np.zeros(0, u8), rng, none))
    # the nearest point of the voxel is tag 7, a farther one a road line
    cases.append(('road line overrides the nearest', _sky(), f32([[0.0625, 0.0, 0.0], [0.25, -0.25, 0.25], [0.625, 0.0, 0.0]]), u8([7, 6, 8]), _small(),
                  np.array([[4, 4, 2, 6], [5, 4, 2, 8]], np.int64)))
    cases.append(('identical points: lowest index', _sky(), f32([[0.75, 0.25, 0.0], [0.125, 0.25, 0.0], [0.125, 0.25, 0.0], [0.125, 0.25, 0.0]]),
                  u8([1, 9, 4, 2]), _small(), np.array([[4, 3, 2, 9], [5, 3, 2, 1]], np.int64)))
    # depth code 0 at the centre pixel is the camera position itself; the lidar point (0, 0, 0) with the lidar at the same place too
    cases.append(('camera before lidar', _pixel(_sky(), 1, 1, 0, 9), f32([[0.0, 0.0, 0.0]]), u8([4]),
                  _small(lidar_position=[1.0, 0.0, 2.0], voxel_size=[8, 8, 12]), np.array([[6, 4, 10, 9]], np.int64)))
    cases.append(('lidar alone at that place', _sky(), f32([[0.0, 0.0, 0.0]]), u8([4]),
                  _small(lidar_position=[1.0, 0.0, 2.0], voxel_size=[8, 8, 12]), np.array([[6, 4, 10, 4]], np.int64)))
    return cases


def odd_geometry():
    """48 x 64 image, grid (40, 24, 8) at 0.5 m, camera / lidar positions float32 cannot represent, another fov."""
    from muvo_amd.data.voxelize_inputs import frame_case
    img, pts, tag = frame_case(H=48, W=64, P=4000, fov=100, key='voxelize_odd', lidar_key='voxelize_odd_lidar')
    pts = (pts * np.float32(0.2)).astype(np.float32)                     # most of the sweep inside the 20 m x 12 m x 4 m grid
    return img, pts, tag, dict(camera_position=[1.3, -0.4, 1.9], lidar_position=[0.7, 0.3, 2.1], fov=100, voxel_resolution=0.5,
                               voxel_size=[40, 24, 8], offset=[2.0, 0.0, -1.0])


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize('name', SETS)
def test_restatement_matches_reference_rows(name):
    from muvo_amd.data.voxelize_inputs import frame_case
    g = np.load(GOLD)
    img, pts, tag = frame_case()
    rows = VR.voxel_rows(img, pts, tag, **_params(g, name))
    gold = g[f'rows_{name}']
    assert gold.dtype == np.uint16 and len(gold) > 30000
    assert rows.shape == gold.shape and np.array_equal(rows.astype(np.uint16), gold) and np.array_equal(rows, gold.astype(np.int64))
    h = rows[:, 0] + rows[:, 1] * 192 + rows[:, 2] * 192 * 192
    assert (np.diff(h) > 0).all()
    # dense form: dataset.py:316-327 applied to the reference's rows
    vox = np.zeros((192, 192, 64), np.uint8)
    sem = gold[:, 3].astype(np.int64)
    sem[sem == 255] = 0
    vox[gold[:, 0], gold[:, 1], gold[:, 2]] = VR.label_remap()[sem]
    assert np.array_equal(VR.dense_grid(rows, (192, 192, 64)), vox) and int((vox > 0).sum()) > 20000


def test_restatement_edge_cases():
    for name, img, pts, tag, p, want in edge_cases():
        got = VR.voxel_rows(img, pts, tag, **p)
        assert got.dtype == np.int64 and np.array_equal(got, want), (name, got.tolist(), want.tolist())
    img, pts, tag, p = odd_geometry()
    rows = VR.voxel_rows(img, pts, tag, **p)
    assert len(rows) > 500 and (rows[:, :3] < np.array(p['voxel_size'])).all()
    n_img = len(VR.voxel_rows(img, pts[:0], tag[:0], **p))
    assert 0 < n_img < len(rows)                                         # camera and lidar both contribute


def test_tool_geometry_is_the_dataset_set():
    """The tool's defaults from the config are the parameter set the fixture pins, to the bit."""
    from muvo_amd.config import get_cfg
    from muvo_amd.generate_voxels import geometry_from_cfg
    g = np.load(GOLD)
    geom, want = geometry_from_cfg(get_cfg()), _params(g, 'dataset')
    assert geom == want and isinstance(geom['offset'][0], float) and geom['offset'] == [-12.8, 0.0, -4.0]


def test_voxelize_exports_and_argument_validation_without_gpu():
    from muvo_amd import input_pipeline as IP
    from muvo_amd import ops
    assert {'muvo_voxelize_frames', 'muvo_voxelize_scratch_bytes'} <= set(ops.EXPORTS)
    L = ops.lib()
    assert L.muvo_abi_version() == 1
    assert L.muvo_voxelize_scratch_bytes(2, 192, 192, 64) == 2 * (15 * 192 * 192 * 64 + 4 * 1152)
    assert L.muvo_voxelize_scratch_bytes(1, 2048, 2048, 512) == -1 and L.muvo_voxelize_scratch_bytes(0, 8, 8, 8) == -1
    buf = C.create_string_buffer(64)
    ok = C.cast(buf, C.c_void_p)                                         # never dereferenced: every call below fails its checks first
    null = C.c_void_p(0)

    def geom(**kw):
        g = IP.voxelize_geometry(4, 4, camera_position=[1.0, 0.0, 2.0], lidar_position=[1.0, 0.0, 2.0], fov=110, voxel_resolution=0.5,
                                 voxel_size=[8, 8, 4], offset=[0.0, 0.0, 0.0])
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def call(img=ok, pts=ok, tag=ok, F=1, Pmax=4, g=None, remap=ok, scratch=ok, rows=ok, cap=20, counts=ok, dense=null, geom_ptr=None):
        g = g or geom()
        return L.muvo_voxelize_frames(img, pts, tag, null, F, C.c_int64(Pmax), geom_ptr if geom_ptr is not None else C.byref(g), remap, scratch,
                                      rows, C.c_int64(cap), counts, dense, null)
    bad = [dict(img=null), dict(geom_ptr=null), dict(scratch=null), dict(rows=null, dense=null), dict(pts=null), dict(tag=null),
           dict(counts=null), dict(rows=null, dense=ok, remap=null), dict(cap=0), dict(F=0), dict(F=-3), dict(Pmax=-1),
           dict(g=geom(H=0)), dict(g=geom(W=-1)), dict(g=geom(Dx=0)), dict(g=geom(Dy=0)), dict(g=geom(Dz=-2)),
           dict(Pmax=2 ** 32 - 16), dict(g=geom(H=65536, W=65536)), dict(g=geom(Dx=2048, Dy=2048, Dz=512)), dict(g=geom(Dx=65536, Dy=1, Dz=1)),
           dict(g=geom(Dz=70000, Dx=1, Dy=1)), dict(g=geom(res=0.0)), dict(g=geom(res=-0.2))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.muvo_last_error().startswith(b'voxelize:'), (kw, L.muvo_last_error())


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _hip_rows(dev, img, pts, tag, **p):
    from muvo_amd import input_pipeline as IP
    out = IP.depth_lidar_voxels(*_dev(dev, img, pts, tag), **p)
    assert isinstance(out, list) and len(out) == 1 and out[0].dtype == torch.int64 and out[0].dim() == 2 and out[0].shape[1] == 4
    return out[0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', SETS)
def test_hip_rows_and_dense_match_reference(dev, name):
    """The 600 x 960 image + 60 000-point sweep against the rows of the real reference; the dense form three ways."""
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data.voxelize_inputs import frame_case
    g = np.load(GOLD)
    p = _params(g, name)
    img, pts, tag = frame_case()
    rows = _hip_rows(dev, img, pts, tag, **p)
    gold = g[f'rows_{name}']
    assert rows.shape == gold.shape and np.array_equal(rows.cpu().numpy().astype(np.uint16), gold)
    assert np.array_equal(rows.cpu().numpy(), gold.astype(np.int64))
    dense = IP.depth_lidar_voxels(*_dev(dev, img, pts, tag), dense=True, **p)
    assert dense.dtype == torch.uint8 and tuple(dense.shape) == (1, 192, 192, 64)
    assert torch.equal(dense[0], IP.voxel_grid(rows))
    assert np.array_equal(dense[0].cpu().numpy(), VR.dense_grid(gold.astype(np.int64), (192, 192, 64)))
    again = _hip_rows(dev, img, pts, tag, **p)                           # run-to-run reproducible
    assert torch.equal(rows, again) and torch.equal(dense, IP.depth_lidar_voxels(*_dev(dev, img, pts, tag), dense=True, **p))


@pytest.mark.gpu
def test_hip_edge_cases(dev):
    from muvo_amd import input_pipeline as IP
    for name, img, pts, tag, p, want in edge_cases():
        got = _hip_rows(dev, img, pts, tag, **p).cpu().numpy()
        assert np.array_equal(got, VR.voxel_rows(img, pts, tag, **p)) and np.array_equal(got, want), (name, got.tolist(), want.tolist())
        dense = IP.depth_lidar_voxels(*_dev(dev, img, pts, tag), dense=True, **p)
        assert np.array_equal(dense[0].cpu().numpy(), VR.dense_grid(want, p['voxel_size'])), name


@pytest.mark.gpu
def test_hip_odd_geometry(dev):
    """Positions that float32 cannot represent (the float32 camera matrix and the float32 in-place lidar update), a grid whose
    sizes are no multiples of the tiles, a small image."""
    from muvo_amd import input_pipeline as IP
    img, pts, tag, p = odd_geometry()
    want = VR.voxel_rows(img, pts, tag, **p)
    got = _hip_rows(dev, img, pts, tag, **p)
    assert len(want) > 500 and np.array_equal(got.cpu().numpy(), want)
    dense = IP.depth_lidar_voxels(*_dev(dev, img, pts, tag), dense=True, **p)
    assert tuple(dense.shape) == (1, 40, 24, 8) and np.array_equal(dense[0].cpu().numpy(), VR.dense_grid(want, p['voxel_size']))
    assert torch.equal(dense[0], IP.voxel_grid(got, size=(40, 24, 8)))
    for kw in (dict(mask_ego=False), dict(max_range=9.0)):
        q = dict(p, **kw)
        assert np.array_equal(_hip_rows(dev, img, pts, tag, **q).cpu().numpy(), VR.voxel_rows(img, pts, tag, **q)), kw


@pytest.mark.gpu
def test_hip_order_independence(dev):
    from muvo_amd.data.voxelize_inputs import frame_case
    g = np.load(GOLD)
    p = _params(g, 'dataset')
    img, pts, tag = frame_case()
    keep = np.ones(len(pts), bool)
    keep[-600:] = False                      # drop the exact duplicates: with them the winner depends on the index by design
    p2, t2 = pts[keep], tag[keep]
    a = _hip_rows(dev, img, p2, t2, **p)
    perm = np.random.RandomState(0).permutation(len(p2))
    b = _hip_rows(dev, img, p2[perm], t2[perm], **p)
    assert len(a) > 30000 and torch.equal(a, b) and torch.equal(a, _hip_rows(dev, img, p2, t2, **p))


@pytest.mark.gpu
def test_hip_batch_and_padding(dev):
    """Three frames with different num_points (one of them 0) equal three single-frame calls; what lies beyond num_points - NaN
    and in-grid coordinates - is never read.  Also in chunks of two frames."""
    from muvo_amd import input_pipeline as IP
    from muvo_amd.data.voxelize_inputs import camera_frame, frame_case
    g = np.load(GOLD)
    p = _params(g, 'dataset')
    img0, pts, tag = frame_case()
    imgs = np.stack([img0, camera_frame(key='voxelize_frame_b'), img0[::-1].copy()])
    nump = [60000, 0, 31234]
    bp, bt = np.zeros((3, 60000, 3), np.float32), np.zeros((3, 60000), np.uint8)
    for f, n in enumerate(nump):
        bp[f, :n], bt[f, :n] = pts[:n], tag[:n]
        bp[f, n:] = np.nan
        bp[f, n::2] = (3.0, 0.5, -1.0)           # would land in the grid
        bt[f, n:] = 6
    single = [_hip_rows(dev, imgs[f], pts[:n], tag[:n], **p) for f, n in enumerate(nump)]
    assert len({len(s) for s in single}) == 3
    dimg, dpts, dtag = _dev(dev, imgs, bp, bt)
    for fpc in (4, 2):
        for num in (nump, torch.tensor(nump, device=dev)):
            batch = IP.depth_lidar_voxels(dimg, dpts, dtag, num, frames_per_call=fpc, **p)
            assert len(batch) == 3 and all(torch.equal(a, b) for a, b in zip(batch, single))
        dense = IP.depth_lidar_voxels(dimg, dpts, dtag, nump, dense=True, frames_per_call=fpc, **p)
        assert tuple(dense.shape) == (3, 192, 192, 64) and all(torch.equal(dense[f], IP.voxel_grid(single[f])) for f in range(3))


@pytest.mark.gpu
def test_generate_voxels_tool(dev, tmp_path):
    Image = pytest.importorskip('PIL.Image')
    pd = pytest.importorskip('pandas')
    from muvo_amd import generate_voxels as GV
    from muvo_amd.data.voxelize_inputs import frame_case
    g = np.load(GOLD)
    img, pts, tag = frame_case()
    run = tmp_path / 'trainval' / 'train' / 'Town01' / '0000'
    (run / 'depth_semantic').mkdir(parents=True)
    (run / 'points_semantic').mkdir()
    names, sweeps = ['000000007', '000000008'], [(pts, tag), (pts[:30000], tag[:30000])]
    for n, (sp, st) in zip(names, sweeps):
        Image.fromarray(img, 'RGBA').save(run / 'depth_semantic' / f'depth_semantic_{n}.png')
        np.save(run / 'points_semantic' / f'points_semantic_{n}.npy', {'points_xyz': sp, 'ObjTag': st.astype(np.uint32)}, allow_pickle=True)
    pd.DataFrame({'depth_semantic_path': [f'depth_semantic/depth_semantic_{n}.png' for n in names],
                  'points_semantic_path': [f'points_semantic/points_semantic_{n}.npy' for n in names]}).to_pickle(run / 'pd_dataframe.pkl')
    assert GV.main(['--root', str(tmp_path)]) == 0
    first, second = np.load(run / 'voxel' / 'voxel_000000007.npy'), np.load(run / 'voxel' / 'voxel_000000008.npy')
    gold = g['rows_dataset']
    assert first.dtype == np.uint16 and first.shape == gold.shape and np.array_equal(first, gold)
    want = VR.voxel_rows(img, pts[:30000], tag[:30000], **_params(g, 'dataset')).astype(np.uint16)
    assert second.dtype == np.uint16 and second.shape == want.shape and np.array_equal(second, want)
    table = pd.read_pickle(run / 'pd_dataframe.pkl')
    assert list(table['voxel_path']) == [f'voxel/voxel_{n}.npy' for n in names]
    stamp = os.path.getmtime(run / 'voxel' / 'voxel_000000007.npy')
    assert GV.main(['--root', str(tmp_path)]) == 2                                   # refuses to replace voxel/ without --overwrite
    with pytest.raises(FileExistsError):
        GV.voxelize_run(run, GV.geometry_from_cfg(GV.get_cfg()), dev)
    assert os.path.getmtime(run / 'voxel' / 'voxel_000000007.npy') == stamp
    assert GV.main(['--root', str(tmp_path), '--overwrite', '--frames-per-call', '1']) == 0
    assert np.array_equal(np.load(run / 'voxel' / 'voxel_000000007.npy'), gold)
