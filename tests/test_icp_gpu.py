"""-m gpu: the on-device ICP (muvo_amd/csrc/icp.hip through ops.icp_step / ops.icp_register and muvo_amd/odometry.py) against
the float64 restatement of tests/icp_reference.py and its bars (4 x the error of the float32 CPU evaluation of the same
restatement, floors justified there; tests/test_icp_reference.py shows on the CPU that the bars reject planted errors).  Every
case's conditions - nearest / second-nearest gap, distance to the threshold, equal stopping iteration of both restatements with
both deltas 5 x away from 1e-6 - are asserted on the CPU (icp_reference.reference) before anything is judged; no case and no
point is excluded.  Each case prints `ICPSTAT <case>: ...` lines with the measured errors."""
import numpy as np
import pytest
import torch

import icp_reference as R

pytestmark = pytest.mark.gpu
GUARD = 12345.0
IDS = [c['id'] for c in R.CASES]


def _place(t, dev, off):
    """`t` on the device inside a fresh buffer of GUARD values, `off` elements after four guard elements; (buffer, view)"""
    n = t.numel()
    buf = torch.full((n + 12,), GUARD, dtype=t.dtype, device=dev)
    buf[4 + off:4 + off + n] = t.reshape(-1).to(dev)
    return buf, buf[4 + off:4 + off + n].view(t.shape)


def _guards_ok(buf, off, n):
    return bool((buf[:4 + off] == GUARD).all()) and bool((buf[4 + off + n:] == GUARD).all())


def _frames(dev, id):
    src, tgt, _ = R.inputs(id)
    return torch.from_numpy(src)[None].to(dev), torch.from_numpy(tgt)[None].to(dev)


def _register(dev, id, **kw):
    from muvo_amd import ops
    c = R.CASE[id]
    s, t = _frames(dev, id)
    return ops.icp_register(s, t, [0], [0], c['scale'], c['thr'], source_stride=c['stride'], **kw)


@pytest.mark.parametrize('id', IDS)
def test_icp_step_cases(dev, id):
    from muvo_amd import ops
    c = R.CASE[id]
    r64, r32 = R.reference(id)
    s, t = _frames(dev, id)
    corr, sums, res = ops.icp_step(s, t, [0], [0], c['scale'], c['thr'], source_stride=c['stride'])
    if r64['status'] == R.EMPTY:
        assert int(res.status[0]) == ops.ICP_EMPTY and bool((corr == -1).all()) and not sums.any()
        assert torch.equal(res.T[0].cpu(), torch.eye(4, dtype=torch.float64)) and int(res.iterations[0]) == 0
        return
    ev64, ev32 = r64['evals'][0], r32['evals'][0]
    assert np.array_equal(corr[0].cpu().numpy(), R.corr_full(id, ev64)), 'another correspondence than float64'
    err, bar = R.sums_error(sums[0].cpu().numpy(), ev64['sums']), R.sums_bar(ev32['sums'], ev64['sums'])
    print(f'ICPSTAT {id} step: sums err ' + ' '.join(f'{e:.2e}' for e in err) + ' (bars ' + ' '.join(f'{b:.2e}' for b in bar) + ')')
    assert (err <= bar).all(), (err, bar)
    assert float(sums[0, 0]) == float(ev64['sums'][0])
    assert abs(float(res.fitness[0]) - ev64['fitness']) < 1e-12


@pytest.mark.parametrize('id', IDS)
def test_icp_register_cases(dev, id):
    c = R.CASE[id]
    r64, r32 = R.reference(id)
    res = _register(dev, id)
    T = res.T[0].cpu().numpy()
    assert int(res.iterations[0]) == r64['iterations'], (int(res.iterations[0]), r64['iterations'])
    assert int(res.status[0]) == r64['status'] and bool(res.converged[0]) == (r64['status'] == R.CONVERGED)
    err, bar, bad = R.t_failures(T, r64['T'], r32['T'])
    print(f"ICPSTAT {id} register: it {int(res.iterations[0])} status {int(res.status[0])} fitness {float(res.fitness[0]):.4f} rmse "
          f"{float(res.inlier_rmse[0]):.3e} |R err| {err[:, :3].max():.2e} (f32 {np.abs(r32['T'] - r64['T'])[:3, :3].max():.2e}) |t err| "
          f"{err[:, 3].max():.2e} (f32 {np.abs(r32['T'] - r64['T'])[:3, 3].max():.2e})")
    assert not bad, (err, bar)
    assert np.array_equal(T[3], (0, 0, 0, 1))
    # every distance is made of float32 coordinates (a moved point is off by up to sqrt(3)/2 ulp of 50 m) and its square carries a
    # few 2^-24 relative: |d rmse| <= ulp(50 m) + 1e-6 rmse
    assert abs(float(res.fitness[0]) - r64['fitness']) < 1e-12 and abs(float(res.inlier_rmse[0]) - r64['rmse']) <= R.ULP_50M + 1e-6 * r64['rmse']
    if c['id'] == 'n1025-large-motion-fitness-below-1':
        assert 0 < r64['fitness'] < 1
    if c['content'] == 'rigid' and c['n'] > 3:              # the known answer, without the oracle, at the floor
        truth = R.inputs(id)[2]
        floor = R.t_bar(truth, truth.astype(np.float32))[:3]
        assert (np.abs(T[:3] - truth[:3]) <= floor).all(), np.abs(T[:3] - truth[:3])


def test_pairs_in_one_call_equal_their_solo_runs_and_guards(dev):
    """four pairs that stop at different iterations, frames at odd element offsets between guard values; a done pair's state
    does not change in later chunks; a second run is bit-identical"""
    from muvo_amd import ops
    ids = [id for id in R.MULTI]
    its = [R.reference(id)[0]['iterations'] for id in ids]
    assert len(set(its)) == len(its), its
    n = max(R.CASE[id]['n'] for id in ids)
    frames = torch.full((8, 4, n), float('nan'))
    frames[:, 3] = 0.0                                      # padding points are invalid
    for k, id in enumerate(ids):
        src, tgt, _ = R.inputs(id)
        assert R.CASE[id]['scale'] == 1.0 and R.CASE[id]['stride'] == 1 and R.CASE[id]['thr'] == R.THRESHOLD
        frames[2 * k, :, :src.shape[1]] = torch.from_numpy(tgt[:4])      # consecutive frames of one tensor: t - 1 = target
        frames[2 * k + 1, :, :src.shape[1]] = torch.from_numpy(src[:4])
    buf, view = _place(frames, dev, 3)
    snaps = []
    src_f, tgt_f = [1, 3, 5, 7], [0, 2, 4, 6]
    res = ops._icp_run(view, view, src_f, tgt_f, 1.0, R.THRESHOLD, on_chunk=lambda st, dn: snaps.append((st.clone(), dn.clone())))
    assert _guards_ok(buf, 3, frames.numel()), 'an input guard element changed'
    # the outputs of icp_step between guards as well: the correspondence store has the widest index of the kernels (p n + i)
    cbuf, corr = _place(torch.zeros(4, n, dtype=torch.int32), dev, 1)
    sbuf, sums = _place(torch.zeros(4, 17, dtype=torch.float64), dev, 1)
    ops.icp_step(view, view, src_f, tgt_f, 1.0, R.THRESHOLD, out=(corr, sums))
    assert _guards_ok(cbuf, 1, 4 * n) and _guards_ok(sbuf, 1, 4 * 17) and _guards_ok(buf, 3, frames.numel()), 'a guard element changed'
    for k, id in enumerate(ids):
        r64 = R.reference(id)[0]
        want = np.full(n, -1, np.int32)
        if r64['status'] != R.EMPTY:
            want[:R.CASE[id]['n']] = R.corr_full(id, r64['evals'][0])
            assert float(sums[k, 0]) == float(r64['evals'][0]['sums'][0])
        assert np.array_equal(corr[k].cpu().numpy(), want), f'{id}: another correspondence than float64'
    assert len(snaps) >= 2, 'the cases must span more than one chunk'
    for (st0, dn0), (st1, dn1) in zip(snaps, snaps[1:]):
        was = dn0.bool()
        assert bool(dn1[was].all()) and torch.equal(st0[was], st1[was]), 'the state of a done pair changed in a later chunk'
    again = ops.icp_register(view, view, src_f, tgt_f, 1.0, R.THRESHOLD)
    for a, b in zip(res, again):
        assert torch.equal(a, b), 'two runs differ'
    for k, id in enumerate(ids):
        solo = ops.icp_register(view, view, [src_f[k]], [tgt_f[k]], 1.0, R.THRESHOLD)
        for a, b in zip(res, solo):
            assert torch.equal(a[k], b[0]), f'{id}: differs from its solo run'
        assert int(res.iterations[k]) == its[k]
        r64, r32 = R.reference(id)
        assert not R.t_failures(res.T[k].cpu().numpy(), r64['T'], r32['T'])[2]


def test_max_iteration_and_init(dev):
    from muvo_amd import ops
    id = 'n1025-tile-plus-one'
    r64, _ = R.reference(id)
    assert r64['iterations'] > 2
    res = _register(dev, id, max_iteration=2)
    assert int(res.iterations[0]) == 2 and int(res.status[0]) == ops.ICP_MAX_ITERATION and not bool(res.converged[0])
    src, tgt, _ = R.inputs(id)
    ref, ref32 = (R.icp(src, tgt, max_iteration=2, dtype=dt) for dt in (np.float64, np.float32))
    assert ref['status'] == R.MAX_ITERATION and not R.t_failures(res.T[0].cpu().numpy(), ref['T'], ref32['T'].astype(np.float64))[2]
    start = R.pose(0.45, 0.08, 1.3)                         # near the answer: fewer iterations than from the identity
    w64, w32 = (R.icp(src, tgt, init=start, dtype=dt) for dt in (np.float64, np.float32))
    R.assert_conditions(w64, w32, 'warm start')
    warm = _register(dev, id, init=torch.from_numpy(start)[None])
    assert int(warm.iterations[0]) == w64['iterations'] < r64['iterations'] and bool(warm.converged[0])
    assert not R.t_failures(warm.T[0].cpu().numpy(), w64['T'], w32['T'].astype(np.float64))[2]


def test_trajectory_and_render(dev):
    """a 2 x 3-frame batch: poses against the restatement (its conditions asserted per pair), the panel pixel for pixel"""
    from muvo_amd import odometry
    rv, T64, T32 = R.trajectory_batch()
    rot, pos, res = odometry.trajectory(torch.from_numpy(rv).to(dev), 1.0, with_result=True)
    got = res.T.cpu().numpy().reshape(2, 2, 4, 4)
    for b in range(2):
        for t in (0, 1):
            err, bar, bad = R.t_failures(got[b, t], T64[b, t], T32[b, t].astype(np.float64))
            print(f'ICPSTAT trajectory sample {b} step {t + 1}: |R err| {err[:, :3].max():.2e} |t err| {err[:, 3].max():.2e}')
            assert not bad, (b, t, err, bar)
            truth = R.pose(*R.TRAJ_MOTIONS[b][t])
            assert np.abs(got[b, t] - truth).max() < 0.005  # a quarter of the 2 cm noise of a single point
    assert rot.shape == (2, 3, 3, 3) and pos.shape == (2, 3, 3) and rot.dtype == np.float64 and pos.dtype == np.float64
    rot_ref, pos_ref = zip(*(R.chain(T64[b]) for b in range(2)))
    for b in range(2):                                      # the chaining itself: the literal restatement on the same poses
        rr, pp = R.chain(got[b])
        assert np.array_equal(rr, rot[b]) and np.array_equal(pp, pos[b])
    assert np.array_equal(rot[:, 0], np.stack([np.eye(3)] * 2)) and not pos[:, 0].any()
    rows = [pos * np.array([1.0, -3.0, 1.0]) + np.array([2.0, 1.0, 0.0]) * (np.arange(3)[None, :, None] > 0)]
    assert np.array_equal(odometry.render_traj(pos, rows), R.render_traj_ref(np.stack(pos_ref), rows)), 'a pixel differs from the restatement'


def _kdtree_icp(src, tgt, thr=R.THRESHOLD):
    """the float64 restatement with an exact k-d tree search (scipy) where there is one: 55 iterations at n = 2500 in well under a
    second; the brute force of icp_reference otherwise"""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        r = R.icp(src, tgt, thr=thr)
        return r['T'], r['iterations']
    S, _ = R.points_of(src, 1.0, np.float64)
    Q, _ = R.points_of(tgt, 1.0, np.float64)
    tree, T, prev, its = cKDTree(Q), np.eye(4), None, 0
    while True:
        M = S @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(M, k=1)
        inl = d * d <= thr * thr
        fit, rmse = inl.mean(), np.sqrt((d[inl] ** 2).mean())
        if prev is not None and abs(fit - prev[0]) < R.STOP_TOL and abs(rmse - prev[1]) < R.STOP_TOL:
            return T, its
        s, q = M[inl], Q[j[inl]]
        sums = np.zeros(17)
        sums[0], sums[2:5], sums[5:8], sums[8:] = inl.sum(), s.sum(0), q.sum(0), (s[:, :, None] * q[:, None, :]).sum(0).reshape(9)
        T, prev, its = R.kabsch(sums) @ T, (fit, rmse), its + 1


def test_two_pose_scene_many_chunks(dev):
    """The ray-cast scene at n = 2500 seen from two poses 1.0 m / 0.1 m / 2 deg apart: about 55 iterations, seven chunks, three
    target tiles.  The conditions of icp_reference cannot hold here - among 55 x 2500 queries the smallest nearest / second-nearest
    gap is 2e-6, and the delta creeps through 1e-6 (last deltas 2.8e-6, 9.3e-7) - so this case is judged on the final pose with a
    tolerance that is reasoned, not measured: a near-tie (gap < 1e-4) resolved the other way swaps one of 2500 pairs between two
    targets at most one ray spacing (about 1 m) apart, which moves the fitted translation by up to 1 / 2500 = 4e-4 m; stopping
    one evaluation earlier or later moves the pose by about the last step, whose rmse delta is < 5e-6.  Bound: 1e-3 m on the
    translation, 1e-4 on the rotation entries (1e-3 m at a lever of 10 m), the iteration count within 2; and the pose is as far
    from the truth as the float64 restatement is (0.071 m: different rays hit different points) plus that bound."""
    from muvo_amd import ops
    c = R.case('n2500-two-pose', 50, 50)
    R.CASE.setdefault(c['id'], c)
    src, tgt, truth = R.inputs(c['id'])
    T64, its = _kdtree_icp(src, tgt)
    res = ops.icp_register(torch.from_numpy(src)[None].to(dev), torch.from_numpy(tgt)[None].to(dev), [0], [0], 1.0, R.THRESHOLD)
    T = res.T[0].cpu().numpy()
    err = np.abs(T - T64)
    print(f'ICPSTAT n2500-two-pose register: it {int(res.iterations[0])} (float64 {its}) |R err| {err[:3, :3].max():.2e} |t err| '
          f'{err[:3, 3].max():.2e} |T64 - truth| {np.abs(T64 - truth).max():.2e}')
    assert its > 3 * ops.ICP_CHUNK and bool(res.converged[0]) and abs(int(res.iterations[0]) - its) <= 2
    assert err[:3, :3].max() <= 1e-4 and err[:3, 3].max() <= 1e-3
    assert np.abs(T - truth).max() <= np.abs(T64 - truth).max() + 1e-3


def test_rows_without_imagined_samples(dev):
    """output_imagines = []: in training the row is as long as the label; in validation / test with PREDICTION.N_SAMPLES = 0 the
    reconstruction covers the first rf steps only - the row's path ends there"""
    from types import SimpleNamespace
    from muvo_amd import odometry
    rv, T64, T32 = R.trajectory_batch()
    label = torch.from_numpy(rv).to(dev)
    cfg = SimpleNamespace(LIDAR_RE=SimpleNamespace(SCALE=1.0))
    for rf in (3, 2):
        output = {'lidar_reconstruction_1': label[:, :rf].clone()}
        (rot_l, pos_l), rows, res = odometry.batch_trajectories(cfg, {'range_view_label_1': label}, output, [])
        assert len(rows) == 1 and rows[0][1].shape == (2, rf, 3) and pos_l.shape == (2, 3, 3) and res.T.shape[0] == 2 * 2 + 2 * (rf - 1)
        assert np.array_equal(rows[0][1], pos_l[:, :rf]), 'the same frames give the same path'
        panel = odometry.traj_panel(cfg, {'range_view_label_1': label}, output, [])
        assert panel.shape == (2, 3, 196, 392) and panel.dtype == torch.uint8
        assert np.array_equal(panel.numpy(), R.render_traj_ref(pos_l, [rows[0][1]]))
    metric = odometry.EgoMotionMetric(cfg)
    metric.update(0, {'range_view_label_1': label}, {'lidar_reconstruction_1': label[:, :2].clone()}, [])
    out = metric.result()['0']
    assert out['pos_error_reconstructed'] == 0.0 and out['pos_error_last'] == 0.0 and out['pairs'] == 6 and out['pos_error_imagined'] == 0.0
