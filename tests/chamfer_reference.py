"""Float64 restatement, inputs, case list and bars for the Chamfer-distance training loss (muvo_amd/csrc/chamfer.hip through
ops.chamfer_loss).  Helpers only: no fixtures, no tests.  tests/test_chamfer_reference.py (CPU) and
tests/test_chamfer_loss_gpu.py (GPU) share everything here, so the bars the GPU test applies are the ones the CPU test proves
to reject planted errors.  The error metric, `failures` and the LOSSSTAT lines are those of tests/loss_reference.py.

The restatement (`chamfer64`).  CDLoss of the reference project (muvo/losses.py:352-367, reducer = mean) on channel-planar
points pred (F, Cp, n), target (F, Ct, n), x / y / z = planes 0 / 1 / 2:
    d_ij = |p_i - t_j|,  loss = weight * mean_f ( mean_j min_i d_ij + mean_i min_j d_ij )
from per-pair coordinate differences (never torch.cdist, which changes to |p|^2 - 2 p.t + |t|^2 above 25 rows), with the rules
the kernels document: the nearest neighbour is the argmin of the squared distance and the LOWEST index wins a tie; the gradient
goes to the prediction only, through the selected pair only; d|a - b| = (a - b) / |a - b| and exactly 0 where the two points
coincide.  It takes `dtype` (default float64): the same code with dtype=float32 is "the float32 CPU evaluation" of the bars.

The gap.  Per query point, (s2 - s1) / s2 for the smallest and second-smallest squared distance s1 <= s2 in float64 (1 where
there is one candidate only, 0 where s2 = 0).  A float32 evaluation computes a squared distance from the differences to a few
1e-7 relative, so it selects the same neighbour wherever the gap is >= GAP_MIN = 1e-4; every case's inputs are drawn so that
this holds for EVERY query (seeds chosen for it; `assert_gaps` is called before anything is judged, nothing is excluded).

The bars.  4 x the largest normalised error of the float32 CPU evaluation against float64 over the family's cases
(`python tests/chamfer_reference.py` prints the table from the case list), loss scalars floored at 8 * 2^-24 as in
loss_reference.py.  The gradient is normalised by its largest element.  The `origin` cases have a family of their own: there
one prediction point receives the sum of hundreds of unit vectors, which the float32 evaluation adds one after the other
(index_add_), so its error - and the bar - is larger than where every point has a handful of senders.  The fixture's three
inputs (tests/golden/chamfer_loss.npz) count as cases of chamfer_loss / chamfer_grad.

    family               float32 evaluation, max(e) over the family     bar
    chamfer_loss         1.81e-07                                        7.24e-07
    chamfer_grad         1.46e-07                                        5.84e-07
    chamfer_grad_origin  6.83e-06                                        2.73e-05
"""
import functools
import os

import numpy as np
import torch

import loss_reference as LR

GAP_MIN = 1e-4
MEASURED = {'chamfer_loss': 1.81e-7, 'chamfer_grad': 1.46e-7, 'chamfer_grad_origin': 6.83e-6}
BARS = {k: max(4 * v, LR.SCALAR_FLOOR if k.endswith('_loss') else 0.0) for k, v in MEASURED.items()}
WEIGHT = LR.f32r(0.5)                  # LOSSES.LIDAR_CD.WEIGHT of the cases
GOUT = 1.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chamfer_loss.npz')
GOLDEN_SHAPES = ((3, 20), (3, 300), (2, 1031))            # (frames, n) of the fixture


# ================================================================================================ restatement
def _nearest(q, s):
    """q, s: (n, 3).  For every q point: squared distance to its nearest s point, that point's index (lowest on a tie), and
    the second-smallest squared distance (inf with one candidate)."""
    d2 = ((q[:, None, :] - s[None, :, :]) ** 2).sum(-1)
    k = min(2, s.shape[0])
    val, _ = torch.topk(d2, k, dim=1, largest=False)
    idx = torch.argmin(d2, dim=1)                          # first minimal index
    first = val[:, 0]
    assert torch.equal(first, d2.gather(1, idx[:, None])[:, 0])
    lower = (d2 == first[:, None]).int().argmax(dim=1)     # the lowest index that attains the minimum, spelled out
    assert torch.equal(lower, idx)
    second = val[:, 1] if k == 2 else torch.full_like(first, float('inf'))
    return first, idx, second


def _unit(a, b):
    """(a - b) / |a - b| per row, exactly 0 where a == b"""
    diff = a - b
    d = (diff ** 2).sum(-1).sqrt()
    return torch.where(d[:, None] > 0, diff / d.clamp_min(torch.finfo(d.dtype).tiny)[:, None], torch.zeros_like(diff)), d


def chamfer64(pred, target, weight=1.0, gout=1.0, dtype=torch.float64, idx=None):
    """pred (F, Cp, n), target (F, Ct, n) -> dict(loss, dpred, dpred_pt, dpred_tp (F, Cp, n), idx_pt, idx_tp (F, n) int64, gap_pt, gap_tp (F, n)).
    dpred = gout * d loss / d pred.  idx = (idx_pt, idx_tp): use these selections instead of the argmin (planted errors)."""
    F, Cp, n = pred.shape
    p, t = pred.to(dtype), target.to(dtype)
    total = torch.zeros((), dtype=dtype)
    dpred, dpred_pt, dpred_tp = (torch.zeros(F, Cp, n, dtype=dtype) for _ in range(3))
    out = {k: [] for k in ('idx_pt', 'idx_tp', 'gap_pt', 'gap_tp')}
    scale = torch.tensor(weight, dtype=dtype) * torch.tensor(gout, dtype=dtype) / (F * n)
    for f in range(F):
        P, T = p[f, :3].t(), t[f, :3].t()                  # (n, 3)
        s1a, a, s2a = _nearest(P, T)                       # prediction point i -> target a[i]
        s1b, b, s2b = _nearest(T, P)                       # target j -> prediction point b[j]
        for key, s1, s2 in (('gap_pt', s1a, s2a), ('gap_tp', s1b, s2b)):
            gap = torch.where(s2 > 0, (s2 - s1) / s2, torch.zeros_like(s2))
            out[key].append(torch.where(torch.isinf(s2), torch.ones_like(s2), gap))
        if idx is not None:
            a, b = idx[0][f], idx[1][f]
        ua, da = _unit(P, T[a])                            # gather: point i and its own nearest target
        ub, db = _unit(P[b], T)                            # scatter: target j adds into its nearest prediction point
        total = total + da.mean() + db.mean()
        g = ua * scale
        tp = torch.zeros_like(g).index_add_(0, b, ub * scale)
        dpred_pt[f, :3], dpred_tp[f, :3] = g.t(), tp.t()
        g.index_add_(0, b, ub * scale)
        dpred[f, :3] = g.t()
        out['idx_pt'].append(a)
        out['idx_tp'].append(b)
    res = {k: torch.stack(v) for k, v in out.items()}
    res['loss'] = torch.tensor(weight, dtype=dtype) * total / F
    res['dpred'], res['dpred_pt'], res['dpred_tp'] = dpred, dpred_pt, dpred_tp      # the sum, and its two terms on their own
    return res


def assert_gaps(ref, tag=''):
    lo = min(float(ref['gap_pt'].min()), float(ref['gap_tp'].min()))
    assert lo >= GAP_MIN, f'{tag}: a query whose nearest and second-nearest squared distances differ by {lo:.2e} relative ' \
                          f'(< {GAP_MIN:g}): choose another seed for this case'


# ================================================================================================ metric
def compare(got, ref, origin=False):
    """{name: (stats, bar)} in the form of loss_reference.compare: the loss normalised by |ref|, dpred by max |ref|"""
    r = LR._d(ref['loss'])
    out = {'loss': (LR.error_stats(got['loss'], r, r.abs()), BARS['chamfer_loss'])}
    r = LR._d(ref['dpred'])
    out['dpred'] = (LR.error_stats(got['dpred'], r, LR.scale_of(r)), BARS['chamfer_grad_origin' if origin else 'chamfer_grad'])
    return out


failures, statlines = LR.failures, LR.statlines


# ================================================================================================ cases
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _planes(points, C, fill):
    """(F, n, 3) points -> (F, C, n) channel-planar float32, planes >= 3 = fill"""
    F, n, _ = points.shape
    out = torch.full((F, C, n), fill, dtype=torch.float32)
    out[:, :3] = points.permute(0, 2, 1)
    return out


def _lattice(n, g):
    """n distinct points on a jittered unit lattice (spacing 1, jitter < 0.2 per axis: any two are >= 0.6 apart), shuffled"""
    m = 1
    while m ** 3 < n:
        m += 1
    cells = torch.stack(torch.meshgrid(*[torch.arange(m, dtype=torch.float32)] * 3, indexing='ij'), -1).reshape(-1, 3)
    cells = cells[torch.randperm(m ** 3, generator=g)[:n]]
    return cells + 0.4 * (torch.rand(n, 3, generator=g) - 0.5)


def case(id, n, F=1, C=3, content='random', seed=0):
    return dict(id=id, n=n, F=F, C=C, content=content, seed=seed)


# seeds: the first for which assert_gaps holds for every query of the case (python tests/chamfer_reference.py --seeds)
CASES = [
    case('n1-single-point', 1, seed=0),
    case('n63-partial-wave', 63, seed=0),
    case('n64-one-wave', 64, seed=0),
    case('n65-wave-plus-one', 65, seed=0),
    case('n255-below-workgroup', 255, seed=0),
    case('n256-one-workgroup', 256, seed=0),
    case('n257-second-query-slot', 257, seed=0),
    case('n1031-two-workgroups-two-tiles', 1031, seed=0),
    case('F3-C4-nan-plane3', 300, F=3, C=4, content='nan3', seed=0),
    case('perm-known-answer-n1031', 1031, content='perm', seed=0),
    case('origin-half-targets-collide-n1031', 1031, content='origin', seed=1),
    case('coincident-point-zero-distance', 257, content='coincident', seed=1),
]
CASE = {c['id']: c for c in CASES}
PERM_FIXED = ((0, 1030), (1030, 0), (1027, 5))      # perm case: target j sits next to prediction point i for these (j, i)


@functools.lru_cache(maxsize=None)
def inputs(id):
    """(pred (F, C, n), target (F, C, n), extra) float32 of a case; extra: 'perm' (target j = prediction perm[j] + offset),
    'pair' ((i, j) of the coincident points)"""
    c = CASE[id]
    n, F, C, g = c['n'], c['F'], c['C'], _gen(zlib_seed(id, c['seed']))
    extra = {}
    fill = float('nan') if c['content'] == 'nan3' else 0.0
    if c['content'] in ('random', 'nan3', 'coincident'):
        P = 2 * torch.rand(F, n, 3, generator=g) - 1       # the scaled units of the range view: about [-1, 1]
        T = 2 * torch.rand(F, n, 3, generator=g) - 1
        if c['content'] == 'coincident':
            i, j = n - 2, 3
            T[0, j] = P[0, i]
            extra['pair'] = (i, j)
    elif c['content'] == 'perm':
        P = _lattice(n, g)[None]
        perm = torch.randperm(n, generator=g)
        for j, i in PERM_FIXED:                            # nearest neighbour at index 0, at n - 1 and in the last partial tile
            k = int((perm == i).nonzero()[0, 0])
            perm[k], perm[j] = perm[j].clone(), perm[k].clone()
        T = P[:, perm] + 1e-3 * (torch.rand(1, n, 3, generator=g) - 0.5)       # offset << the spacing of 0.6
        extra['perm'] = perm
    elif c['content'] == 'origin':
        # points in a box far from the origin; every second target is an empty label pixel (0, 0, 0); the others sit next to a
        # prediction point, so no prediction point's nearest target is the origin cluster (whose members tie exactly)
        P = (_lattice(n, g) * 0.1 + 2.0)[None]
        perm = torch.randperm(n, generator=g)
        T = P[:, perm] + 0.02 * (torch.rand(1, n, 3, generator=g) - 0.5)
        T[:, ::2] = 0.0
    else:
        raise ValueError(c['content'])
    return _planes(P, C, fill), _planes(T, C, fill), extra


def zlib_seed(id, seed):
    import zlib
    return zlib.crc32(id.encode()) % (1 << 30) + 7919 * seed


@functools.lru_cache(maxsize=None)
def reference(id):
    """float64 restatement of a case (computed once, shared; treat as read-only), gaps asserted"""
    pred, target, _ = inputs(id)
    ref = chamfer64(pred, target, WEIGHT, GOUT)
    assert_gaps(ref, id)
    return ref


# ================================================================================================ trainer wiring
def lidar_only_cfg(**extra):
    """base_1d with every head but the lidar reconstruction off"""
    from muvo_amd.config import base_1d_cfg
    return base_1d_cfg(**{'EVAL.RGB_SUPERVISION': False, 'VOXEL_SEG.ENABLED': False, 'SEMANTIC_SEG.ENABLED': False,
                          'LIDAR_RE.ENABLED': True, **extra})


LIDAR_DICTS_SEED = 0          # the first seed for which every query of the three scales has a gap >= GAP_MIN


def lidar_dicts(seed=LIDAR_DICTS_SEED, device='cpu', sizes=((8, 32), (4, 16), (2, 8)), b=1, s=2):
    """synthetic `batch` / `output` dicts of the lidar head at three scales ((b, s, 4, h, w), channel 3 = the depth channel)"""
    g = torch.Generator().manual_seed(seed)
    batch, output = {}, {}
    for f, (h, w) in zip((1, 2, 4), sizes):
        batch[f'range_view_label_{f}'] = (2 * torch.rand(b, s, 4, h, w, generator=g) - 1).to(device)
        output[f'lidar_reconstruction_{f}'] = (2 * torch.rand(b, s, 4, h, w, generator=g) - 1).to(device)
    return batch, output


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def golden_planar(z, k):
    """fixture case k: (pred, target) as (F, 3, n) planar float32 tensors (stored as the reference takes them: (F, n, 3))"""
    return tuple(torch.from_numpy(z[f'{name}_{k}']).permute(0, 2, 1).contiguous() for name in ('pred', 'target'))


def float32_errors():
    """{family: max normalised error of the float32 evaluation over the cases} - the MEASURED table"""
    worst = {k: 0.0 for k in MEASURED}
    for c in CASES:
        pred, target, _ = inputs(c['id'])
        ref = reference(c['id'])
        got = chamfer64(pred, target, WEIGHT, GOUT, dtype=torch.float32)
        assert torch.equal(got['idx_pt'], ref['idx_pt']) and torch.equal(got['idx_tp'], ref['idx_tp']), c['id']
        cmp = compare(got, ref, origin=c['content'] == 'origin')
        fam = 'chamfer_grad_origin' if c['content'] == 'origin' else 'chamfer_grad'
        worst['chamfer_loss'] = max(worst['chamfer_loss'], cmp['loss'][0]['max_e'])
        worst[fam] = max(worst[fam], cmp['dpred'][0]['max_e'])
        print(f'{c["id"]:45s} loss {cmp["loss"][0]["max_e"]:.3e}  dpred {cmp["dpred"][0]["max_e"]:.3e}')
    z = load_golden()
    for k in range(len(GOLDEN_SHAPES)):                    # the fixture's inputs belong to the family as well
        pred, target = golden_planar(z, k)
        ref = chamfer64(pred, target, WEIGHT, GOUT)
        assert_gaps(ref, f'fixture {k}')
        cmp = compare(chamfer64(pred, target, WEIGHT, GOUT, dtype=torch.float32), ref)
        worst['chamfer_loss'] = max(worst['chamfer_loss'], cmp['loss'][0]['max_e'])
        worst['chamfer_grad'] = max(worst['chamfer_grad'], cmp['dpred'][0]['max_e'])
        print(f'{"fixture-%d" % k:45s} loss {cmp["loss"][0]["max_e"]:.3e}  dpred {cmp["dpred"][0]["max_e"]:.3e}')
    return worst


if __name__ == '__main__':
    import sys
    if '--seeds' in sys.argv:
        for c in CASES:
            for seed in range(200):
                c['seed'] = seed
                inputs.cache_clear()
                pred, target, _ = inputs(c['id'])
                ref = chamfer64(pred, target)
                if min(float(ref['gap_pt'].min()), float(ref['gap_tp'].min())) >= GAP_MIN:
                    break
            print(f"{c['id']}: seed {seed}")
        inputs.cache_clear()
    for fam, v in float32_errors().items():
        print(f'{fam:20s} {v:.2e}   bar {max(4 * v, LR.SCALAR_FLOOR if fam.endswith("_loss") else 0.0):.2e}')
