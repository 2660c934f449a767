"""CPU: the float64 restatement of tests/icp_reference.py against an independent brute force, the known motions, the bars
against planted errors, and the host side of muvo_amd/odometry.py (pose chaining, render_traj) against a literal restatement of
the reference's lines."""
import numpy as np
import pytest

import icp_reference as R


def _brute_icp(src, tgt, thr=R.THRESHOLD):
    """plain loops: nearest neighbour point by point, Kabsch from the centred point sets with numpy.linalg.svd"""
    S = np.array([src[:3, i] for i in range(src.shape[1]) if src[3, i] > 0], np.float64)
    Q = np.array([tgt[:3, j] for j in range(tgt.shape[1]) if tgt[3, j] > 0], np.float64)
    T, prev, it = np.eye(4), None, 0
    while True:
        M = S @ T[:3, :3].T + T[:3, 3]
        pairs = []
        for m in M:
            d2 = ((m - Q) ** 2).sum(1)
            j = int(np.argmin(d2))
            if d2[j] <= thr * thr:
                pairs.append((m, Q[j], d2[j]))
        fit, rmse = len(pairs) / len(S), float(np.sqrt(np.mean([p[2] for p in pairs])))
        if prev is not None and abs(fit - prev[0]) < 1e-6 and abs(rmse - prev[1]) < 1e-6:
            return T, it
        a, b = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        H = (a - a.mean(0)).T @ (b - b.mean(0))
        U, _, Vt = np.linalg.svd(H)
        D = np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))])
        Rm = Vt.T @ D @ U.T
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = Rm, b.mean(0) - Rm @ a.mean(0)
        T, prev, it = step @ T, (fit, rmse), it + 1


@pytest.mark.parametrize('id', ['n3-three-points', 'n1025-invalid-10pct-nan', 'n1025-large-motion-fitness-below-1'])
def test_restatement_equals_brute_force(id):
    c = R.CASE[id]
    src, tgt, _ = R.inputs(id)
    r64, _ = R.reference(id)
    T, it = _brute_icp(src, tgt, c['thr'])
    assert it == r64['iterations'] and np.abs(T - r64['T']).max() < 1e-9


@pytest.mark.parametrize('id', [c['id'] for c in R.CASES])
def test_conditions_hold_and_known_motions(id):
    c = R.CASE[id]
    r64, r32 = R.reference(id)                              # asserts gap, threshold margin and the stopping rule
    truth = R.inputs(id)[2]
    if c['content'] == 'rigid' and c['n'] >= 3:
        assert (np.abs(r64['T'] - truth)[:3] <= R.t_bar(truth, truth.astype(np.float32))[:3]).all()
    if c['content'] == 'noisy' and not c['invalid']:
        assert np.abs(r64['T'] - truth).max() < 0.005       # a quarter of the 2 cm noise of a single point
    if c['content'].endswith('-empty'):
        assert r64['status'] == R.EMPTY and np.array_equal(r64['T'], np.eye(4)) and r64['iterations'] == 0
    if id == 'n1-single-point':
        assert r64['status'] == R.FEW_INLIERS and np.array_equal(r64['T'], np.eye(4))


def test_bars_reject_planted_errors():
    id = 'n1025-tile-plus-one'
    c = R.CASE[id]
    src, tgt, _ = R.inputs(id)
    r64, r32 = R.reference(id)
    ev64, ev32 = r64['evals'][0], r32['evals'][0]
    bar = R.sums_bar(ev32['sums'], ev64['sums'])
    assert (R.sums_error(ev32['sums'], ev64['sums']) <= bar).all()
    S, _ = R.points_of(src, 1.0, np.float64)
    Q, _ = R.points_of(tgt, 1.0, np.float64)
    i = 517
    second = int(np.argsort(((ev64['moved'][i] - Q) ** 2).sum(1))[1])
    swapped = R.evaluate(S, Q, np.eye(4), c['thr'], swap=(i, second))
    assert not np.array_equal(swapped['idx'], ev64['idx'])
    assert (R.sums_error(swapped['sums'], ev64['sums']) > bar).any(), 'one swapped neighbour passes the bars'
    dropped = R.evaluate(S, Q, np.eye(4), c['thr'], drop=i)
    assert (R.sums_error(dropped['sums'], ev64['sums']) > bar).any(), 'a dropped inlier passes the bars'
    wrong = R.icp(src, tgt, order='TU')
    assert R.t_failures(wrong['T'], r64['T'], r32['T'])[2] or wrong['iterations'] != r64['iterations'], 'T U for U T passes the bars'
    assert not R.t_failures(r32['T'], r64['T'], r32['T'])[2]


def test_reflection_guard():
    g = np.random.default_rng(3)
    S = np.concatenate([g.uniform(-5, 5, (40, 2)), np.zeros((40, 1))], 1)          # planar: a mirror image fits as well as a rotation
    Q = S * np.array([1.0, -1.0, 1.0]) + g.normal(0, 0.01, S.shape) * np.array([1.0, 1.0, 0.0])
    sums = np.zeros(17)
    sums[0], sums[2:5], sums[5:8], sums[8:] = len(S), S.sum(0), Q.sum(0), (S[:, :, None] * Q[:, None, :]).sum(0).reshape(9)
    good, bad = R.kabsch(sums), R.kabsch(sums, guard=False)
    assert abs(np.linalg.det(good[:3, :3]) - 1) < 1e-12 and abs(np.linalg.det(bad[:3, :3]) + 1) < 1e-12
    assert R.t_failures(bad, good, good.astype(np.float32))[2], 'a missing reflection guard passes the bars'


def test_chain_and_render_traj_equal_the_literal_restatement():
    from muvo_amd import odometry                            # this import fails without the feature
    g = np.random.default_rng(0)
    Ts = np.stack([[R.pose(g.uniform(0, 3), g.uniform(-1, 1), g.uniform(-20, 20)) for _ in range(5)] for _ in range(2)])
    Ts[1, 2] = np.eye(4)
    rot, pos = odometry.chain(Ts)
    for b in range(2):
        rr, pp = R.chain(Ts[b])
        assert np.array_equal(rot[b], rr) and np.array_equal(pos[b], pp)
    assert np.array_equal(rot[:, 0], np.stack([np.eye(3)] * 2)) and not pos[:, 0].any()
    rows = [pos * np.array([1.0, -1.5, 1.0]), (pos[:, ::-1] - pos[:, -1:]) * 3.0, pos * 40.0]       # every path starts at the origin; the last leaves the canvas
    got = odometry.render_traj(pos, rows)
    assert got.shape == (2, 3, 196, 196 * 4) and got.dtype == np.uint8
    assert np.array_equal(got, R.render_traj_ref(pos, rows))
    assert tuple(got[0, :, 0, 0]) == (50, 50, 50) and tuple(got[0, :, 2, 2]) == (0, 0, 0)
    assert (got[0] == np.array([20, 150, 20])[:, None, None]).all(0).any(), 'no line pixel'
    # every prediction tile shows the origin of the label tile and not the label path
    origin_only = odometry.render_traj(pos[:, :1], [pos[:, :1]])
    assert np.array_equal(origin_only[:, :, :, :196], origin_only[:, :, :, 196:]) and tuple(origin_only[0, :, 96, 96]) == (150, 20, 20)
    assert int((origin_only[0, 0, :, :196] == 150).sum()) == 13          # the disc dx^2 + dy^2 <= 4


def test_line_and_disc_properties():
    """the own-definition line and disc of odometry.py on their own, without the restatement's copy of them: both end points
    drawn, max(|dx|, |dy|) + 1 pixels, one per step along the major axis, never more than half a pixel off the ideal line, the
    same pixels in both directions up to the tie rule; one octant by hand"""
    from muvo_amd import odometry
    green = np.array(odometry.LINE_COLOUR)

    def pixels(p0, p1):
        img = np.zeros((196, 196, 3), np.uint8)
        odometry._line(img, p0, p1)
        ys, xs = np.nonzero((img == green).all(-1))
        return sorted(zip(xs.tolist(), ys.tolist()))
    assert pixels((10, 10), (15, 12)) == [(10, 10), (11, 10), (12, 11), (13, 11), (14, 12), (15, 12)]      # by hand: y = 10 + 0.4 (x - 10), rounded
    assert pixels((7, 7), (7, 7)) == [(7, 7)]
    g = np.random.default_rng(5)
    ends = [((96, 96), (96, 120)), ((96, 96), (60, 96)), ((20, 30), (40, 50)), ((50, 20), (30, 40))]
    ends += [(tuple(g.integers(0, 196, 2).tolist()), tuple(g.integers(0, 196, 2).tolist())) for _ in range(60)]
    for p0, p1 in ends:
        got = pixels(p0, p1)
        dx, dy = p1[0] - p0[0], p1[1] - p0[1]
        assert p0 in got and p1 in got and len(got) == max(abs(dx), abs(dy)) + 1, (p0, p1)
        major = 0 if abs(dx) >= abs(dy) else 1
        assert len({p[major] for p in got}) == len(got), 'two pixels in one step of the major axis'
        for x, y in got:                                    # distance to the ideal line along the minor axis
            t = ((x - p0[0]) / dx) if major == 0 and dx else ((y - p0[1]) / dy if dy else 0.0)
            ideal = p0[1 - major] + t * (dy if major == 0 else dx)
            assert abs((y if major == 0 else x) - ideal) <= 0.5 + 1e-9, (p0, p1, x, y)
    off = np.zeros((196, 196, 3), np.uint8)
    odometry._line(off, (190, 100), (260, 100))             # leaves the canvas: the pixels outside are dropped
    assert int((off == green).all(-1).sum()) == 6
    disc = np.zeros((196, 196, 3), np.uint8)
    odometry._disc(disc, (0, 100))                          # half a disc at the edge
    ys, xs = np.nonzero((disc == np.array(odometry.DISC_COLOUR)).all(-1))
    assert sorted(zip(xs.tolist(), ys.tolist())) == [(0, 98), (0, 99), (0, 100), (0, 101), (0, 102), (1, 99), (1, 100), (1, 101), (2, 100)]
    assert odometry._pixel((1.0, -2.0, 0.0)) == (106, 91) and odometry._pixel((0.19, 0.19, 0.0)) == (95, 95)      # int() truncates


def test_exports_and_flags():
    from muvo_amd import ops, predict
    assert {'muvo_icp_init', 'muvo_icp_iterate', 'muvo_icp_state_doubles', 'muvo_icp_ws_doubles'} <= set(ops.EXPORTS)
    args = predict.parse_args(['--out', 'x', '--mode', 'test', '--ego-motion', '--traj', '--panels', '1', '--ego-threshold', '4',
                               '--ego-stride', '2', '--ego-max-iteration', '50'])
    assert args.ego_motion and args.traj and args.ego_threshold == 4.0 and args.ego_stride == 2 and args.ego_max_iteration == 50
    with pytest.raises(SystemExit):
        predict.parse_args(['--out', 'x', '--mode', 'sim', '--ego-motion'])
    import inspect
    assert list(inspect.signature(ops.icp_register).parameters) == ['src', 'tgt', 'src_frames', 'tgt_frames', 'scale', 'threshold', 'max_iteration',
                                                                    'init', 'source_stride']
    from muvo_amd import train
    t = train.build_parser().parse_args(['--panel-dir', 'p', '--traj', '--traj-stride', '8', '--traj-max-iteration', '50'])
    assert t.traj and t.traj_stride == 8 and t.traj_max_iteration == 50
