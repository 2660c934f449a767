"""-m gpu: muvo_voxel_calibration (csrc/calibration.hip) against the float64 restatement (tests/calibration_reference.py) on the
same fp32 logits.  Integers - counts, the table's n and n_correct, the ensemble SSC counts, `ens` - are compared with ==: the
inputs keep a margin of 1e-4 between the two largest mean probabilities and between conf * B and the nearest integer in float64
(asserted; a condition on the inputs, tests/test_calibration_reference.py checks the generator), so fp32 arithmetic cannot change
a decision; one test drops the margin to 1e-12, where the kernel must take its decisions again in fp64.  The real sums - kept as fixed-point integers - lie within `R.bars`: four times what the float32 twin of the formulae
loses against float64 on that case, voxel by voxel, plus the 2^-25 a voxel of the fixed-point format; never taken from the
kernel's output.  Byte maps: within one level (one fp32 rounding step cannot move a value further), equal on the hand-made cases.
Shapes: F = 3 with 5 x 6 x 7 (eight columns a wave, a partial last wave), 8 x 8 x 64 (one column a wave, several workgroups) and
3 x 5 x 70 (a column in two rounds, the second partial); the last frame of every random case is all 255."""
import numpy as np
import pytest
import torch

import calibration_reference as R

pytestmark = pytest.mark.gpu
GRIDS = ((5, 6, 7), (8, 8, 64), (3, 5, 70))
FIX = R.FIX


def _run(dev, logits, label, B, maps=True, into=None):
    from muvo_amd.calibration import ensemble_calibration
    out = ensemble_calibration([torch.from_numpy(t).to(dev) for t in logits], torch.from_numpy(label).to(dev), bins=B, maps=maps, into=into)
    torch.cuda.synchronize()
    return out


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, twin, what, exact_maps=False):
    """integers with ==, real sums within the bars, byte maps within one level (equal with exact_maps)"""
    assert got['counts'].tolist() == ref['counts'].tolist(), what
    assert got['table'][:, :2].tolist() == ref['table'][:, :2].astype(np.int64).tolist(), what
    assert got['ssc'].tolist() == ref['ssc'].tolist(), what
    assert np.array_equal(got['ens'], ref['ens']), what
    bar_sums, bar_conf = R.bars(ref, twin)
    dev_sums = np.abs(got['sums'] / FIX - ref['sums'])
    dev_conf = np.abs(got['table'][:, 2] / FIX - ref['table'][:, 2])
    print(what, 'sums: deviation', ' '.join(f'{v:.3g}' for v in dev_sums), '| bar', ' '.join(f'{v:.3g}' for v in bar_sums),
          '| conf: worst deviation / bar', f'{(dev_conf / bar_conf.clip(1e-300)).max():.3g}')
    assert (dev_sums <= bar_sums).all(), (what, dev_sums, bar_sums)
    assert (dev_conf <= bar_conf).all(), (what, dev_conf, bar_conf)
    for name in ('top_entropy', 'top_mi'):
        d = np.abs(got[name].astype(np.int64) - ref[name].astype(np.int64)).max()
        assert d <= (0 if exact_maps else 1), (what, name, d)


@pytest.mark.parametrize('B', (1, 15, 32))
@pytest.mark.parametrize('K', (1, 3, 8))
@pytest.mark.parametrize('C', (2, 9, 16))
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(map(str, g)))
def test_against_the_restatement(dev, grid, C, K, B):
    from muvo_amd import metrics as M
    logits, label, dropped = R.make_case(1000 * C + 10 * K + B, 3, C, *grid, K, B)
    ref = R.accumulate(logits, label, B)
    top, edge = R.margins(ref, B)
    assert dropped == 0 and top.min() >= 1e-4 and edge.min() >= 1e-4           # the condition on the inputs
    assert (label[2] == 255).all() and ref['counts'][1] > label[2].size and ref['counts'][0] > 0
    got = _host(_run(dev, logits, label, B))
    _compare(got, ref, R.accumulate(logits, label, B, np.float32), f'{grid} C{C} K{K} B{B}')
    assert got['counts'][:3].sum() == label.size
    if K == 1:                                                                 # the counting kernel of the SSC metric, on the device
        comp, tps, fps, fns = M.ssc_counts(torch.from_numpy(logits[0]).to(dev), torch.from_numpy(label).to(dev), C)
        want = comp.tolist() + [int(v) for row in zip(tps.tolist(), fps.tolist(), fns.tolist()) for v in row]
        assert got['ssc'].tolist() == want
        assert got['sums'][4] == 0 and got['sums'][5] == 0 and (got['top_mi'] == 0).all()          # MI is exactly 0 at K = 1


@pytest.mark.parametrize('name', sorted(R.hand_cases()))
def test_hand_made_cases(dev, name):
    logits, label, B = R.hand_cases()[name]
    ref = R.accumulate(logits, label, B)
    got = _host(_run(dev, logits, label, B))
    # H / ln C and MI / ln C are 0 or 1 in the first four; `neg_inf` (ln 2 / ln 3) and `nonfinite` keep the one-level rule
    _compare(got, ref, R.accumulate(logits, label, B, np.float32), name, exact_maps=name in ('equal_c2', 'equal_c4', 'onehot_pair', 'conf_one'))
    if name == 'conf_one':
        assert got['table'][B - 1, 0] == label.size and got['table'][B - 1, 2] == label.size * (1 << 24)
    if name.startswith('equal'):
        C = logits[0].shape[1]
        assert (got['ens'] == 0).all() and got['table'][:, 2].sum() == label.size * (1 << 24) // C and (got['top_entropy'] == 255).all()
    if name == 'nonfinite':
        assert got['counts'].tolist()[:3] == [50, 2, 38] and (got['top_entropy'][1] == 0).all() and (got['ens'][1] == 255).all()


@pytest.mark.parametrize('K', (1, 2))
def test_near_ties_are_decided_as_float64_decides(dev, K):
    """Voxels whose two largest mean probabilities differ by 1e-8 .. 1e-5, and voxels whose conf * B lies that close to an integer:
    fp32 arithmetic cannot decide them, the kernel takes such decisions again in fp64 (CAL_CLOSE), so the integers still equal the
    float64 restatement.  The condition on the inputs: the restatement's own margins exceed 1e-12 (float64 is good to 1e-15)."""
    rng = np.random.default_rng(40 + K)
    F, X, Y, Z, B = 2, 6, 8, 64, 15
    N = F * X * Y * Z
    eps = rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-8, -5, N)
    edge = rng.integers(8, 15, N) / B                                          # a bin edge in (1/2, 1)
    target = np.where(np.arange(N) % 2 == 0, 0.5 + eps, edge + eps)            # even voxels: a near-tie; odd: conf near an edge
    d = (np.log(target) - np.log1p(-target)).astype(np.float32)                # softmax((d, 0))[0] = target
    lg = np.zeros((K, 2, N), np.float32)
    lg[:, 0] = d
    if K == 2:                                                                 # two samples around the same mean
        shift = rng.uniform(0.0, 0.3, N).astype(np.float32)
        lg[0, 0] += shift
        lg[1, 0] -= shift
        keep = np.arange(N) % 2 == 0                                           # the mean of two softmaxes moves off an edge: keep the ties only
        lg[:, 0, ~keep] = rng.standard_normal((2, (~keep).sum())).astype(np.float32)
    flip = rng.random(N) < 0.5                                                 # either class may lead
    lg[:, :, flip] = lg[:, ::-1, flip]
    logits = [np.ascontiguousarray(np.moveaxis(lg[k].reshape(2, F, X, Y, Z), 0, 1)) for k in range(K)]
    label = rng.integers(0, 2, (F, X, Y, Z)).astype(np.uint8)
    ref = R.accumulate(logits, label, B)
    top, edge_gap = R.margins(ref, B)
    assert top.min() > 1e-12 and edge_gap.min() > 1e-12
    assert (top < 1e-6).sum() > N // 8 and (K == 2 or (edge_gap < 1e-6 * B).sum() > N // 8)       # the case is what it claims to be
    got = _host(_run(dev, logits, label, B))
    _compare(got, ref, R.accumulate(logits, label, B, np.float32), f'near ties K{K}')


def test_label_outside_the_classes_goes_the_way_of_ssc_counts(dev):
    from muvo_amd import metrics as M
    C, B = 4, 15
    logits, label, dropped = R.make_case(77, 3, C, 5, 6, 7, 1, B)
    label[0, 0] = 4
    label[0, 1] = 200
    ref = R.accumulate(logits, label, B)
    assert dropped == 0 and min(m.min() for m in R.margins(ref, B)) >= 1e-4
    got = _host(_run(dev, logits, label, B))
    _compare(got, ref, R.accumulate(logits, label, B, np.float32), 'label >= C')
    comp, tps, fps, fns = M.ssc_counts(torch.from_numpy(logits[0]).to(dev), torch.from_numpy(label).to(dev), C)
    assert got['ssc'].tolist() == comp.tolist() + [int(v) for row in zip(tps.tolist(), fps.tolist(), fns.tolist()) for v in row]


def test_two_calls_add_up_and_a_repeated_call_repeats_its_bits(dev):
    from muvo_amd.calibration import new_accumulators
    C, K, B = 9, 3, 15
    a = R.make_case(1, 3, C, 8, 8, 64, K, B)
    b = R.make_case(2, 3, C, 8, 8, 64, K, B)
    first, second = _run(dev, *a[:2], B), _run(dev, *b[:2], B)
    acc = new_accumulators(C, B, dev)
    _run(dev, *a[:2], B, maps=False, into=acc)
    _run(dev, *b[:2], B, maps=False, into=acc)
    for name in ('table', 'counts', 'ssc', 'sums'):
        assert torch.equal(acc[name], first[name] + second[name]), name
    again = _run(dev, *a[:2], B)                                               # fresh accumulators: the same bits
    for name, t in first.items():
        assert torch.equal(t, again[name]), name
    without = _run(dev, *a[:2], B, maps=False)                                 # the optional outputs change nothing
    assert set(without) == {'table', 'counts', 'ssc', 'sums'} and all(torch.equal(without[n], first[n]) for n in without)


def test_lead_axes_and_frames_give_the_same(dev):
    from muvo_amd.calibration import ensemble_calibration
    logits, label, _ = R.make_case(3, 4, 3, 5, 6, 7, 2, 15)
    lg = [torch.from_numpy(t).to(dev) for t in logits]
    lab = torch.from_numpy(label).to(dev)
    flat = ensemble_calibration(lg, lab, maps=True)
    nested = ensemble_calibration([t.reshape(2, 2, *t.shape[1:]) for t in lg], lab.reshape(2, 2, 1, *lab.shape[1:]), maps=True)
    assert nested['ens'].shape == (2, 2, 5, 6, 7) and nested['top_mi'].shape == (2, 2, 5, 6)
    assert all(torch.equal(flat[n].reshape(-1), nested[n].reshape(-1)) for n in flat)
