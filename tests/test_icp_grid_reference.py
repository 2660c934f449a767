"""CPU: the numpy restatement of the ICP grid search (tests/icp_grid_reference.py) against the exhaustive search - bit for bit on
the lattice inputs, index and inlier set on the cases of tests/icp_reference.py -, the proof that the lattice inputs see the two
planted errors, and the Python surface of search='grid': the refusal in ops, the config accessor, the command-line flags.  The
GPU tests (tests/test_icp_grid_gpu.py) hold the kernels to the exhaustive kernel's bytes and to this restatement."""
import numpy as np
import pytest

import icp_grid_reference as G
import icp_reference as R

LATTICE = G.lattice_inputs()
NONFINITE = G.nonfinite_inputs()


def _both(inp, **planted):
    T = inp.get('init')
    return (G.grid_search(inp['src'], inp['tgt'], 1.0, inp['thr'], T, **planted), G.brute_search(inp['src'], inp['tgt'], 1.0, inp['thr'], T))


@pytest.mark.parametrize('name', list(LATTICE))
def test_lattice_inputs_equal_the_exhaustive_search_to_the_bit(name):
    inp = LATTICE[name]
    (d2, idx), (bd2, bidx) = _both(inp)
    # the exhaustive search of icp_reference in float32 on the same operands
    qi, moved = G.moved_queries(inp['src'], 1.0, inp.get('init'))
    Q, ti = R.points_of(inp['tgt'], 1.0, np.float32)
    with np.errstate(over='ignore'):
        first, j, _ = R.nearest(moved, Q)
    ok = first < np.inf
    assert np.array_equal(bidx[qi][ok], ti[j][ok]) and np.array_equal(bd2[qi][ok], first[ok]) and (bidx[qi][~ok] == -1).all()
    # every winner that can be an inlier is the same point at the same distance; beyond the threshold both gate to -1
    thr2 = np.float32(np.float32(inp['thr']) * np.float32(inp['thr']))
    inl = (bidx >= 0) & (bd2 <= thr2)
    assert np.array_equal(G.corr_of(d2, idx, inp['thr']), G.corr_of(bd2, bidx, inp['thr'])), name
    assert np.array_equal(d2[inl].view(np.uint32), bd2[inl].view(np.uint32)), name


def test_lattice_inputs_hold_what_they_are_named_for():
    c = {k: G.corr_of(*G.brute_search(v['src'], v['tgt'], 1.0, v['thr'], v.get('init')), v['thr']) for k, v in LATTICE.items()}
    assert c['threshold-exact'][0] >= 0 and c['threshold-one-step-lower'][0] == -1 and (c['threshold-one-step-lower'][1:] == -1).all()
    assert (c['threshold-exact'][1:] >= 0).all()
    out = c['queries-outside-the-box']
    assert out[0] >= 0 and out[1] >= 0 and out[2] == -1 and out[3] >= 0 and out[4] == -1 and out[5] >= 0 and out[6] == -1 and out[8] == -1
    assert (c['queries-1e30-away-through-init'] == -1).all()
    assert list(c['all-targets-identical']) == [0, 0, 0, -1]
    assert list(c['one-valid-target-among-invalid']) == [7, 7, -1]
    assert list(c['n1']) == [0]
    ties = [k for k in LATTICE if k.startswith('tie-k')]
    assert len(ties) >= 24
    for k in ties:                                          # the lower index of the two equidistant targets wins where it is an inlier
        assert c[k][0] in (0, -1), k
    assert sum(c[k][0] == 0 for k in ties) >= 16
    low_on_axis = [np.count_nonzero(LATTICE[k]['tgt'][:3, 0] != LATTICE[k]['src'][:3, 0]) == 1 for k in ties]
    assert 0 < sum(low_on_axis) < len(ties)                 # the lower index sits on the axis-aligned one in some, on the other in others


@pytest.mark.parametrize('planted', [dict(shrink=1), dict(strict=True)])
def test_planted_errors_change_a_result_on_the_lattice_inputs(planted):
    changed = []
    for name, inp in LATTICE.items():
        (d2, idx), (bd2, bidx) = _both(inp, **planted)
        if not np.array_equal(G.corr_of(d2, idx, inp['thr']), G.corr_of(bd2, bidx, inp['thr'])):
            changed.append(name)
    print('planted', planted, 'seen by', changed)
    assert changed, f'no lattice input sees the planted error {planted}'
    if 'strict' in planted:
        assert 'tie-on-the-border-of-ring-1' in changed
    else:
        assert 'threshold-exact' in changed


@pytest.mark.parametrize('name', list(NONFINITE))
def test_nonfinite_inputs(name):
    inp = NONFINITE[name]
    (d2, idx), (bd2, bidx) = _both(inp)
    got, want = G.corr_of(d2, idx, inp['thr']), G.corr_of(bd2, bidx, inp['thr'])
    assert np.array_equal(got, want)
    assert (want >= 0).sum() >= 10                           # the other queries still find their neighbours
    if name == 'source-nan':
        assert want[3] == -1 and want[9] == -1 and want[12] == -1
    else:
        assert not np.isin([5, 17, 30, 40], want).any()     # a target with a non-finite or far-away coordinate is nobody's inlier


@pytest.mark.parametrize('id', [c['id'] for c in R.CASES])
def test_cases_of_icp_reference_same_index_and_inliers(id):
    """the first evaluation of every case: the same neighbour and the same inlier set as the float64 restatement (whose gaps
    >= 1e-4 make the float32 choice unambiguous)"""
    c = R.CASE[id]
    r64, _ = R.reference(id)
    src, tgt, _ = R.inputs(id)
    d2, idx = G.grid_search(src, tgt, c['scale'], c['thr'], None, c['stride'])
    got = G.corr_of(d2, idx, c['thr'])
    if r64['status'] == R.EMPTY:
        assert (got == -1).all()
        return
    assert np.array_equal(got, R.corr_full(id, r64['evals'][0]))
    bd2, bidx = G.brute_search(src, tgt, c['scale'], c['thr'], None, c['stride'])
    assert np.array_equal(got, G.corr_of(bd2, bidx, c['thr']))


def test_grid_shapes_of_the_restatement():
    """the cell edge: threshold / 8 while the box fits into 2^17 cells, doubled beyond; cell() clamps whatever comes in"""
    g = np.random.default_rng(3)
    wide = G.frame(g.uniform(-4000, 4000, (2000, 3)))
    grid = G.build(wide, 1.0, 0.5)
    assert grid['h'] > 0.5 / 8 and grid['dims'].prod() <= G.CELLS and float(np.log2(grid['h'] / (0.5 / 8))) % 1 == 0
    small = G.build(G.frame(g.uniform(-1, 1, (50, 3))), 1.0, 40.0)
    assert small['h'] == 5.0 and list(small['dims']) == [2, 2, 2]
    lo, inv = np.float32(-1), np.float32(2)
    vals = np.array([-np.inf, -1e38, -1.0, 0.0, 1e38, np.inf, np.nan], np.float32)
    assert list(G.cell(vals, lo, inv, 7)) == [0, 0, 0, 2, 6, 6, 0]
    empty = G.build(G.frame([(np.nan, 0, 0)]), 1.0, 1.0)
    assert len(empty['idx']) == 0 and G.nearest(empty, (0, 0, 0), 1.0) == (np.inf, -1)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_unknown_search_is_refused_before_the_library_is_loaded(monkeypatch):
    import torch
    from muvo_amd import ops

    def no_lib():
        raise AssertionError('the library must not be loaded')
    monkeypatch.setattr(ops, 'lib', no_lib)
    t = torch.zeros(1, 4, 8)
    for call in (lambda: ops.icp_register(t, t, [0], [0], 1.0, 5.0, search='octree'),
                 lambda: ops.icp_register_queued(t, t, [0], [0], 1.0, 5.0, 3, search='octree'),
                 lambda: ops.icp_step(t, t, [0], [0], 1.0, 5.0, search='Grid'),
                 lambda: ops._icp_run(t, t, [0], [0], 1.0, 5.0, search=None)):
        with pytest.raises(ValueError, match="search must be 'brute' or 'grid'"):
            call()


def _cfg(aggregate=None):
    from muvo_amd.config import base_1d_cfg
    cfg = base_1d_cfg()
    cfg.VOXEL_SEG['VISIBILITY'] = type(cfg)({'ENABLED': True})
    if aggregate is not None:
        cfg.VOXEL_SEG['AGGREGATE'] = type(cfg)(aggregate)
    return cfg


def test_config_accessor():
    from muvo_amd import config
    from muvo_amd.config import base_1d_cfg, voxel_aggregate, voxel_aggregate_icp_search
    assert voxel_aggregate_icp_search(base_1d_cfg()) == 'brute'
    assert voxel_aggregate_icp_search(_cfg({'ENABLED': True})) == 'brute'
    assert voxel_aggregate_icp_search(_cfg({'ENABLED': True, 'ICP_SEARCH': 'grid'})) == 'grid'
    assert voxel_aggregate_icp_search(_cfg({'ENABLED': True, 'ICP_SEARCH': 'brute'})) == 'brute'
    assert voxel_aggregate(_cfg({'ENABLED': True, 'ICP_SEARCH': 'grid'})) == (True, 4, 0.3, 30, 4)      # the 5-tuple stays
    assert 'VOXEL_SEG.AGGREGATE.ICP_SEARCH' in config.EXTENSION_KEYS
    cfg = base_1d_cfg(**{'VOXEL_SEG__VISIBILITY__ENABLED': True, 'VOXEL_SEG__AGGREGATE__ENABLED': True, 'VOXEL_SEG__AGGREGATE__ICP_SEARCH': 'grid'})
    assert voxel_aggregate_icp_search(cfg) == 'grid'
    cfg = config.get_cfg(cfg_dict={'VOXEL_SEG': {'VISIBILITY': {'ENABLED': True}, 'AGGREGATE': {'ENABLED': True, 'ICP_SEARCH': 'grid'}}})
    assert voxel_aggregate_icp_search(cfg) == 'grid'
    for bad in ('octree', 'GRID', '', 1, True, None, ['grid']):
        with pytest.raises(ValueError, match=r'VOXEL_SEG\.AGGREGATE\.ICP_SEARCH'):
            voxel_aggregate_icp_search(_cfg({'ENABLED': True, 'ICP_SEARCH': bad}))


def test_preprocess_refuses_a_bad_search_at_construction():
    from muvo_amd.models.preprocess import PreProcess
    with pytest.raises(ValueError, match=r'VOXEL_SEG\.AGGREGATE\.ICP_SEARCH'):
        PreProcess(_cfg({'ENABLED': True, 'ICP_SEARCH': 'kdtree'}))


def test_command_line_flags():
    from muvo_amd import predict, train
    p, need = predict.build_parser(), ['--out', 'o', '--mode', 'test']
    assert p.parse_args(need).ego_search == 'brute'
    assert p.parse_args(need + ['--ego-search', 'grid']).ego_search == 'grid'
    with pytest.raises(SystemExit):
        p.parse_args(need + ['--ego-search', 'octree'])
    t = train.build_parser()
    assert t.parse_args([]).traj_search == 'brute'
    assert t.parse_args(['--traj-search', 'grid']).traj_search == 'grid'
    with pytest.raises(SystemExit):
        t.parse_args(['--traj-search', 'octree'])


def test_metric_options_carry_the_search():
    from types import SimpleNamespace
    from muvo_amd import odometry
    cfg = SimpleNamespace(LIDAR_RE=SimpleNamespace(SCALE=1.0))
    assert odometry.EgoMotionMetric(cfg).kw['search'] == 'brute'
    assert odometry.EgoMotionMetric(cfg, search='grid').kw['search'] == 'grid'
