"""CPU: the VOXEL_SEG.AGGREGATE accessor of muvo_amd/config.py and the restatement of tests/voxel_aggregate_reference.py on hand-made
cases.  The GPU tests (tests/test_voxel_aggregate_gpu.py) hold the kernels to this restatement."""
import numpy as np
import pytest

import visibility_reference as VR
import voxel_aggregate_reference as AR

UNIT = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)              # poses in cells


# ---- the accessor -----------------------------------------------------------------------------------------------------------------
def _cfg(aggregate=None, visibility=True, **over):
    from muvo_amd.config import base_1d_cfg
    cfg = base_1d_cfg(**over)
    if visibility:
        cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True})
    if aggregate is not None:
        cfg.VOXEL_SEG['AGGREGATE'] = type(cfg)(aggregate)
    return cfg


def test_accessor_absent_is_off_and_defaults():
    from muvo_amd import config
    from muvo_amd.config import base_1d_cfg, voxel_aggregate
    cfg = base_1d_cfg()
    assert 'AGGREGATE' not in cfg.VOXEL_SEG
    assert voxel_aggregate(cfg) == (False, 4, 0.3, 30, 4)
    assert voxel_aggregate(_cfg({'ENABLED': True})) == (True, 4, 0.3, 30, 4)
    assert voxel_aggregate(_cfg({'ENABLED': True, 'WINDOW': 9, 'MIN_FITNESS': 0, 'ICP_ITERATIONS': 5, 'ICP_STRIDE': 1})) == (True, 9, 0.0, 5, 1)
    assert voxel_aggregate(_cfg({'ENABLED': False, 'WINDOW': 2}, visibility=False)) == (False, 2, 0.3, 30, 4)
    for key in ('', '.ENABLED', '.WINDOW', '.MIN_FITNESS', '.ICP_ITERATIONS', '.ICP_STRIDE'):
        assert 'VOXEL_SEG.AGGREGATE' + key in config.EXTENSION_KEYS
    # from the command line and from a cfg dict, like every extension key
    cfg = base_1d_cfg(**{'VOXEL_SEG__VISIBILITY__ENABLED': True, 'VOXEL_SEG__AGGREGATE__ENABLED': True, 'VOXEL_SEG__AGGREGATE__WINDOW': 2})
    assert voxel_aggregate(cfg) == (True, 2, 0.3, 30, 4)
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'VISIBILITY': {'ENABLED': True}, 'AGGREGATE': {'ENABLED': True, 'MIN_FITNESS': 0.5}}})
    assert voxel_aggregate(cfg) == (True, 4, 0.5, 30, 4)


@pytest.mark.parametrize('node, text', [
    ({'ENABLED': 1}, 'VOXEL_SEG.AGGREGATE.ENABLED'),
    ({'ENABLED': 'yes'}, 'VOXEL_SEG.AGGREGATE.ENABLED'),
    ({'ENABLED': True, 'WINDOW': 0}, 'VOXEL_SEG.AGGREGATE.WINDOW'),
    ({'ENABLED': True, 'WINDOW': 2.0}, 'VOXEL_SEG.AGGREGATE.WINDOW'),
    ({'ENABLED': True, 'WINDOW': True}, 'VOXEL_SEG.AGGREGATE.WINDOW'),
    ({'ENABLED': True, 'WINDOW': 65}, 'VOXEL_SEG.AGGREGATE.WINDOW'),
    ({'ENABLED': True, 'MIN_FITNESS': -0.1}, 'VOXEL_SEG.AGGREGATE.MIN_FITNESS'),
    ({'ENABLED': True, 'MIN_FITNESS': 1.5}, 'VOXEL_SEG.AGGREGATE.MIN_FITNESS'),
    ({'ENABLED': True, 'MIN_FITNESS': 'high'}, 'VOXEL_SEG.AGGREGATE.MIN_FITNESS'),
    ({'ENABLED': True, 'MIN_FITNESS': float('nan')}, 'VOXEL_SEG.AGGREGATE.MIN_FITNESS'),
    ({'ENABLED': True, 'ICP_ITERATIONS': 0}, 'VOXEL_SEG.AGGREGATE.ICP_ITERATIONS'),
    ({'ENABLED': True, 'ICP_ITERATIONS': 3.5}, 'VOXEL_SEG.AGGREGATE.ICP_ITERATIONS'),
    ({'ENABLED': True, 'ICP_STRIDE': 0}, 'VOXEL_SEG.AGGREGATE.ICP_STRIDE'),
    ({'ENABLED': True, 'ICP_STRIDE': False}, 'VOXEL_SEG.AGGREGATE.ICP_STRIDE'),
    ({'ENABLED': False, 'WINDOW': -1}, 'VOXEL_SEG.AGGREGATE.WINDOW'),           # checked even when off
])
def test_accessor_refuses_bad_values(node, text):
    from muvo_amd.config import voxel_aggregate
    with pytest.raises(ValueError, match=text.replace('.', r'\.')):
        voxel_aggregate(_cfg(node))


def test_accessor_needs_the_visibility_mask_and_inherits_its_refusals():
    from muvo_amd.config import voxel_aggregate
    with pytest.raises(ValueError, match=r'VOXEL_SEG\.AGGREGATE\.ENABLED needs VOXEL_SEG\.VISIBILITY\.ENABLED'):
        voxel_aggregate(_cfg({'ENABLED': True}, visibility=False))
    cfg = _cfg({'ENABLED': True})
    cfg.VOXEL_SEG['ENABLED'] = False
    with pytest.raises(ValueError, match=r'VOXEL_SEG\.VISIBILITY\.ENABLED needs VOXEL_SEG\.ENABLED'):
        voxel_aggregate(cfg)
    cfg = _cfg({'ENABLED': True})
    cfg.VOXEL_SEG['USE_TOP_K'] = True
    with pytest.raises(ValueError, match='USE_TOP_K'):
        voxel_aggregate(cfg)


def test_cell_map_of_the_label_scales():
    """g = r / (RESOLUTION k) + EV_POSITION / k: the lidar, at POINTS.LIDAR_POSITION (y mirrored) in the ego frame, lands on the
    origin of voxel_view.lidar_rays at every scale"""
    from muvo_amd import voxel_view
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.ops import voxel_cell_map
    cfg = base_1d_cfg()
    px, py, pz = (float(v) for v in cfg.POINTS.LIDAR_POSITION)
    origin = voxel_view.lidar_rays(cfg, 64)[0, :3].astype(np.float64)
    for k in (1, 2, 4):
        m = voxel_cell_map(cfg, k)
        assert m[:3] == [1.0 / (0.2 * k)] * 3 and m[3:] == [32 / k, 96 / k, 12 / k]
        g = np.array(m[:3]) * np.array([px, -py, pz]) + np.array(m[3:])
        assert np.allclose(g, origin / k, rtol=0, atol=1e-6)


# ---- the restatement on hand-made cases ---------------------------------------------------------------------------------------------
def _shift(dx, dy=0, dz=0):
    return AR.pose(t=(dx, dy, dz))


def _scene(F, shape=(6, 5, 4)):
    """F all-free frames, nothing seen"""
    return np.zeros((F, *shape), np.uint8), np.zeros((F, *shape), bool)


def _run(label, seen, T, b, s, window, faces=False, **kw):
    mats, usable = AR.chain(np.asarray(T, np.float64).reshape(-1, 4, 4), b, s, window, UNIT, **kw)
    out, counts, close = AR.aggregate(label, seen, s, mats, usable)
    assert faces or not close.any()
    masked, n = VR.masked(label, seen)
    assert int(counts.sum()) == int(n[1]), 'filled + still unknown = the unknown count of the mask'
    own = masked != 255
    assert np.array_equal(out[own], masked[own]), 'an own observation was overridden'
    return out, counts, usable, mats


def test_single_frame_equals_the_masked_label():
    rng = np.random.default_rng(0)
    label = ((rng.random((2, 6, 5, 4)) < 0.2) * 3).astype(np.uint8)
    seen = rng.random(label.shape) < 0.5
    out, counts, usable, _ = _run(label, seen, np.zeros((0, 4, 4)), 2, 1, 3)
    assert not usable.any()
    assert np.array_equal(out, VR.masked(label, seen)[0]) and counts.tolist() == [0, 0, int(VR.masked(label, seen)[1][1])]


def test_window_larger_than_the_sequence():
    label, seen = _scene(2)
    label[0, 3] = 2
    seen[0, 1] = True
    out, counts, usable, _ = _run(label, seen, [np.eye(4)], 1, 2, 5)
    assert usable.tolist() == [[0, 1] + [0] * 8, [1, 0] + [0] * 8]
    assert (out[1, 3] == 2).all() and (out[1, 1] == 0).all() and (out[1, 0] == 255).all()
    assert np.array_equal(out[0], VR.masked(label, seen)[0][0])          # frame 1 saw nothing: nothing to give


def test_identity_wall_seen_then_shadowed():
    """frame 0 sees the wall at x = 3 and the free cells in front; frame 1 sees only x = 0: it gets the wall and the free cells"""
    label, seen = _scene(2)
    label[:, 3] = 4
    seen[0, :4] = True
    seen[1, 0] = True
    label[1, 3] = 0                                                       # the labels of frame 1 do not even hold the wall
    out, counts, _, _ = _run(label, seen, [np.eye(4)], 1, 2, 1)
    assert (out[1, 3] == 4).all() and (out[1, :3] == 0).all() and (out[1, 4:] == 255).all()
    assert counts.tolist() == [20, 40, 40 + 40]


def test_whole_cell_translation_shifts_the_fill():
    """p_0 = p_1 + (2, -1, 0) cells: cell c of frame 1 is cell c + (2, -1, 0) of frame 0"""
    label, seen = _scene(2)
    label[0, 4, 1, 2] = 7
    seen[0, 5, 0, :] = True
    out, _, _, mats = _run(label, seen, [_shift(2, -1)], 1, 2, 1)
    assert mats[1, 0].reshape(3, 4)[:, 3].tolist() == [2.0, -1.0, 0.0]
    want = np.full(label.shape[1:], 255, np.uint8)
    want[2, 2, 2] = 7
    want[3, 1, :] = 0
    assert np.array_equal(out[1], want)
    # and back: frame 0 looks into frame 1 through the inverse
    label, seen = _scene(2)
    label[1, 2, 2, 2] = 7
    out, _, _, mats = _run(label, seen, [_shift(2, -1)], 1, 2, 1)
    assert mats[0, 1].reshape(3, 4)[:, 3].tolist() == [-2.0, 1.0, 0.0]
    assert out[0, 4, 1, 2] == 7 and int((out[0] != 255).sum()) == 1


def test_past_before_future_at_equal_distance():
    label, seen = _scene(3)
    label[0, 2, 2, 2] = 1
    label[2, 2, 2, 2] = 2
    label[2, 3, 3, 3] = 5
    out, _, _, _ = _run(label, seen, [np.eye(4), np.eye(4)], 1, 3, 1)
    assert out[1, 2, 2, 2] == 1 and out[1, 3, 3, 3] == 5


def test_nearer_wins_over_farther():
    label, seen = _scene(5)               # the observer is frame 2
    label[0, 1, 1, 1] = 1                 # d = 2 into the past
    label[3, 1, 1, 1] = 2                 # d = 1 into the future: nearer
    label[4, 2, 2, 2] = 6                 # d = 2 into the future
    label[0, 2, 2, 2] = 3                 # d = 2 into the past: before the future at equal d
    out, _, _, _ = _run(label, seen, [np.eye(4)] * 4, 1, 5, 2)
    assert out[2, 1, 1, 1] == 2 and out[2, 2, 2, 2] == 3
    out, _, _, _ = _run(label, seen, [np.eye(4)] * 4, 1, 5, 1)
    assert out[2, 1, 1, 1] == 2 and out[2, 2, 2, 2] == 255


def test_unknown_source_is_skipped_not_copied():
    label, seen = _scene(3)
    seen[2, 1, 1, 1] = True               # frame 0 (past) does not know the cell, frame 2 (future) saw it free
    out, counts, _, _ = _run(label, seen, [np.eye(4)] * 2, 1, 3, 1)
    assert out[1, 1, 1, 1] == 0 and counts.tolist() == [0, 1, 3 * 120 - 2] and out[0, 1, 1, 1] == 255        # frame 0 would need d = 2


def test_source_outside_the_grid():
    label, seen = _scene(2)
    seen[0] = True
    out, _, _, _ = _run(label, seen, [_shift(4)], 1, 2, 1)
    assert (out[1, :2] == 0).all() and (out[1, 2:] == 255).all()           # x + 4 >= 6 is outside
    out, _, _, _ = _run(label, seen, [_shift(0, 0, -100)], 1, 2, 1)
    assert (out[1] == 255).all()
    out, _, _, _ = _run(label, seen, [_shift(1e300)], 1, 2, 1, faces=True)          # 1e300 is an integer
    assert (out[1] == 255).all()


def test_invalid_middle_link_blocks_every_pair_across_it_and_no_other():
    s = 5
    T = np.stack([np.eye(4)] * (s - 1))
    for how in ('nan', 'fitness', 'status'):
        Tc, fitness, status = T.copy(), np.full(s - 1, 0.9), np.ones(s - 1, np.int64)
        if how == 'nan':
            Tc[2, 1, 3] = np.inf
        elif how == 'fitness':
            fitness[2] = 0.1
        else:
            status[2] = 4
        _, usable = AR.chain(Tc, 1, s, 4, UNIT, fitness, status, 0.3)        # link 2 joins frames 2 and 3
        for t in range(s):
            for slot in range(8):
                d = slot // 2 + 1
                tp = t + d if slot % 2 else t - d
                want = 0 <= tp < s and not (min(t, tp) <= 2 < max(t, tp))
                assert bool(usable[t, slot]) == want, (how, t, tp)
    _, usable = AR.chain(T, 1, s, 4, UNIT, np.full(s - 1, 0.3), np.array([0, 1, 2, 1]), 0.3)      # at the bar; running / stopped are no failures
    assert int(usable.sum()) == 2 * (4 + 3 + 2 + 1)
    label, seen = _scene(s)
    label[0, 1, 1, 1] = 1
    Tc = T.copy()
    Tc[2] = np.nan
    out, _, _, _ = _run(label, seen, Tc, 1, s, 4)
    assert [int(out[t, 1, 1, 1]) for t in range(s)] == [1, 1, 1, 255, 255]


def test_no_fill_across_sequences():
    label, seen = _scene(4)
    label[1, 2, 2, 2] = 9                  # last frame of sequence 0
    label[2, 3, 3, 3] = 8                  # first frame of sequence 1
    out, _, usable, _ = _run(label, seen, [np.eye(4), np.eye(4)], 2, 2, 3)
    assert out[0, 2, 2, 2] == 9 and out[3, 3, 3, 3] == 8
    assert out[2, 2, 2, 2] == 255 and out[1, 3, 3, 3] == 255 and out[3, 2, 2, 2] == 255 and out[0, 3, 3, 3] == 255
    assert usable[:, 2:].sum() == 0


def test_own_free_observation_never_becomes_occupied():
    label, seen = _scene(2)
    label[0] = 5                           # a frame full of a moving object
    seen[1, 2] = True                      # frame 1 looked through x = 2 and found it free
    out, counts, _, _ = _run(label, seen, [np.eye(4)], 1, 2, 1)
    assert (out[1, 2] == 0).all() and (out[1, :2] == 5).all() and (out[1, 3:] == 5).all()
    assert counts.tolist() == [100, 0, 0]


def test_rotation_carries_cells_about_the_mapped_origin():
    """a quarter turn about z in metres, through the map of a 0.5 m grid whose ego point is cell corner (3, 3, 0): cell centre
    c + 1/2 goes to Rz (c + 1/2 - o) + o"""
    cell_map = (2.0, 2.0, 2.0, 3.0, 3.0, 0.0)
    mats, usable = AR.chain(AR.pose(yaw=90.0)[None], 1, 2, 1, cell_map)
    M = mats[1, 0].reshape(3, 4)
    q = M[:, :3] @ np.array([4.5, 3.5, 1.5]) + M[:, 3]
    assert np.allclose(q, [2.5, 4.5, 1.5], atol=1e-12) and usable.tolist() == [[0, 1], [1, 0]]
    inv = mats[0, 1].reshape(3, 4)
    assert np.allclose(inv[:, :3] @ q + inv[:, 3], [4.5, 3.5, 1.5], atol=1e-12)


def test_chain_products_against_numpy_matrices():
    """the chain's ordered sums against plain 4 x 4 products and numpy's general inverse, to 1e-12"""
    case = AR.make_case((5, 6, 7), 2, 5, 6, 9, 'a', 3)
    b, s, W = 2, 5, 6
    A = np.diag(list(AR.CELL_MAP[:3]) + [1.0])
    A[:3, 3] = AR.CELL_MAP[3:]
    mats, usable = AR.chain(case['T'], b, s, W, AR.CELL_MAP)
    T = case['T'].reshape(b, s - 1, 4, 4)
    for i in range(b):
        for t in range(s):
            for slot in range(2 * W):
                d = slot // 2 + 1
                tp = t + d if slot % 2 else t - d
                assert bool(usable[i * s + t, slot]) == (0 <= tp < s)
                if not 0 <= tp < s:
                    continue
                M = np.eye(4)
                for k in range(1, d + 1):
                    M = (np.linalg.inv(T[i, t + k - 1]) if slot % 2 else T[i, t - k]) @ M
                want = (A @ M @ np.linalg.inv(A))[:3].reshape(-1)
                assert np.abs(mats[i * s + t, slot] - want).max() <= 1e-12 * np.abs(want).max()


def test_shared_cases_keep_clear_of_cell_faces():
    """the inputs of the GPU tests: no q of the restatement within 1e-9 of an integer, something filled of every kind, something left"""
    for shape in ((5, 6, 7), (8, 8, 4)):
        for mix in ('a', 'b'):
            case = AR.make_case(shape, 2, 5, 2, 9, mix, 1)
            ref = AR.solve(case)
            assert not ref['close'].any()
            assert ref['counts'].min() > 0, ref['counts']
            assert int(ref['counts'].sum()) == int(VR.masked(case['label'], case['seen'])[1][1])
