"""Float64 restatement, inputs, case list and bars for the Lovasz-softmax training loss of the voxel head
(muvo_amd/csrc/lovasz.hip through ops.voxel_lovasz_loss).  Helpers only: no fixtures, no tests.  tests/test_lovasz_reference.py
(CPU) and tests/test_lovasz_gpu.py (GPU) share everything here, so the bars the GPU test applies are the ones the CPU test
proves to reject planted errors.  The error metric, `failures` and the LOSSSTAT lines are those of tests/loss_reference.py.

The restatement (`lovasz64`), from the definition of DESIGN.md section 11.  logits (F, C, V), labels (F, V) bytes.  A voxel is
valid iff label < C.  Per frame f and class c, over the valid voxels: fg = [label == c], e = |fg - softmax(logits)_c|,
G = sum fg; rank descending by e, ties by ascending voxel index; at rank i = 1..n: I = G - #fg(ranks <= i),
U = G + #bg(ranks <= i), g_i = 1 / U (foreground) or I / (U (U - 1)) (background; evaluated as (I / U) / (U - 1) so that the
same code runs in float32, where U (U - 1) is not exact); L_fc = sum_i e_(i) g_i.
    loss = weight / F * sum_f (sum_{c: G_fc > 0} L_fc) / max(1, #{c: G_fc > 0})
The gradient treats the ranking as fixed: dlde = g at the voxel's rank (0 for ignored voxels and absent classes),
q_c = scale_f * [present] * (-1 if fg else +1) * dlde_c, dlogits_k = p_k (q_k - sum_c q_c p_c), zeros at ignored voxels.
It takes `dtype` (default float64): the same code with dtype=float32 is "the float32 CPU evaluation" of the bars.

The order.  The loss is piecewise linear in the errors: two voxels whose float64 errors differ by less than float32 resolves
may legitimately swap ranks, which moves the loss by nothing measurable and two gradient elements by a lot.  So `order_from=`
hands a ranking over: an (F, C, V) array whose values are ranked (stable, descending) instead of the errors computed here,
everything else evaluated in `dtype`.  The GPU's dlde and gradient are judged against float64 on the order of the errors the
device returned; the errors themselves (lovasz_errors) and the loss (its own order on both sides) pin the rest.  Nothing is
excluded and no gap condition is needed.

The bars.  4 x the largest normalised error of the float32 CPU evaluation against float64 over the family's cases
(`python tests/lovasz_reference.py` prints the table from the case list), loss scalars floored at 8 * 2^-24 as in
loss_reference.py.
    lovasz_loss    |loss - ref| / |ref|, float32 with its own order
    lovasz_errors  absolute (errors live in [0, 1])
    lovasz_dlde    relative per element, against float64 on the same order
    lovasz_grad    normalised by the largest element, the float64 order handed over

    family          float32 evaluation, max(e) over the family     bar
    lovasz_loss     1.42e-07                                        5.68e-07
    lovasz_errors   2.92e-07                                        1.17e-06
    lovasz_dlde     1.16e-07                                        4.63e-07
    lovasz_grad     3.03e-06                                        1.21e-05
(float32 with its OWN order, for the record: the gradient is up to 9.9e-2 of its largest element away at the quantised case,
where float32 and float64 break near-ties differently, and 7.8e-5 at V = 70001 - the reason for handing the order over.)
"""
import functools
import zlib

import torch

import loss_reference as LR

MEASURED = {'lovasz_loss': 1.42e-7, 'lovasz_errors': 2.92e-7, 'lovasz_dlde': 1.16e-7, 'lovasz_grad': 3.03e-6}
BARS = {k: max(4 * v, LR.SCALAR_FLOOR if k.endswith('_loss') else 0.0) for k, v in MEASURED.items()}
WEIGHT = LR.f32r(0.7)                  # LOSSES.VOXEL_LOVASZ.WEIGHT of the cases
GOUT = 1.0
SCALE1 = (192, 192, 64)                # the voxel grid of base_1d at scale 1


# ================================================================================================ restatement
def softmax_errors(logits, labels, dtype=torch.float64):
    """p (F, C, V), errors (F, C, V), fg (F, C, V) bool, valid (F, V) bool"""
    F, C, V = logits.shape
    z = logits.to(dtype)
    ex = torch.exp(z - z.max(dim=1, keepdim=True).values)
    p = ex / ex.sum(dim=1, keepdim=True)
    lab = labels.long()
    valid = lab < C
    fg = lab[:, None, :] == torch.arange(C)[None, :, None]
    errors = torch.where(valid[:, None, :], torch.where(fg, 1 - p, p), torch.zeros_like(p))
    return p, errors, fg, valid


def jaccard_increments(fgs, dtype=torch.float64):
    """fgs: bool (n,), the foreground flags along the ranking -> g (n,) in `dtype` from the closed forms; zeros when G = 0"""
    n = fgs.numel()
    G = int(fgs.sum())
    if G == 0 or n == 0:
        return torch.zeros(n, dtype=dtype)
    cum = torch.cumsum(fgs.long(), 0)
    i = torch.arange(1, n + 1)
    I, U = (G - cum).to(dtype), (G + (i - cum)).to(dtype)
    bg = (I / U) / (U - 1).clamp_min(1)                     # U - 1 >= G >= 1 at every background rank
    return torch.where(fgs, 1 / U, bg)


def lovasz64(logits, labels, weight=1.0, gout=1.0, dtype=torch.float64, order_from=None, descending_ties=False,
             count_ignored=None, mean_over_all_classes=False):
    """logits (F, C, V) float32, labels (F, V) uint8 -> dict(loss, dlogits (F, C, V), errors, dlde (F, C, V), present (F, C) bool,
    frame_class_loss (F, C)), in `dtype`.  dlogits = gout * d loss / d logits with the ranking fixed.
    order_from: (F, C, V) values to rank by instead of the errors.  The last three arguments plant errors for the CPU tests:
    ties by DESCENDING index; (f, v) of one ignored voxel to count as background; 1 / C instead of 1 / #present."""
    F, C, V = logits.shape
    p, errors, fg, valid = softmax_errors(logits, labels, dtype)
    if count_ignored is not None:
        valid = valid.clone()
        valid[count_ignored] = True
        errors = torch.where(valid[:, None, :], torch.where(fg, 1 - p, p), torch.zeros_like(p))
    key = errors if order_from is None else torch.as_tensor(order_from).cpu()
    dlde = torch.zeros(F, C, V, dtype=dtype)
    lfc = torch.zeros(F, C, dtype=dtype)
    present = torch.zeros(F, C, dtype=torch.bool)
    for f in range(F):
        vox = valid[f].nonzero()[:, 0]
        for c in range(C):
            k = key[f, c, vox].double()
            if descending_ties:
                order = (vox.numel() - 1) - torch.sort(-k.flip(0), stable=True).indices
            else:
                order = torch.sort(-k, stable=True).indices      # stable: equal errors stay in ascending voxel order
            ranked = vox[order]
            fgs = fg[f, c, ranked]
            g = jaccard_increments(fgs, dtype)
            present[f, c] = bool(fgs.any())
            dlde[f, c, ranked] = g
            lfc[f, c] = (errors[f, c, ranked] * g).sum()
    npres = present.sum(1)
    den = torch.full_like(npres, C) if mean_over_all_classes else npres.clamp_min(1)
    w = torch.tensor(weight, dtype=dtype)
    frame = (lfc * present.to(dtype)).sum(1) / den.to(dtype)
    loss = w * frame.sum() / F
    scale = (w * torch.tensor(gout, dtype=dtype) / (F * den.to(dtype)))[:, None, None]
    sign = torch.where(fg, -torch.ones((), dtype=dtype), torch.ones((), dtype=dtype))
    q = scale * present.to(dtype)[:, :, None] * sign * dlde
    dz = p * (q - (q * p).sum(1, keepdim=True))
    dz = torch.where(valid[:, None, :], dz, torch.zeros_like(dz))
    return {'loss': loss, 'dlogits': dz, 'errors': errors, 'dlde': dlde, 'present': present, 'frame_class_loss': lfc}


# ================================================================================================ metric
def compare(got, ref, names=('loss', 'dlogits', 'errors', 'dlde')):
    """{name: (stats, bar)} in the form of loss_reference.compare, for those of `names` that `got` holds"""
    out = {}
    for name in names:
        if name not in got:
            continue
        r = LR._d(ref[name])
        if name == 'loss':
            out[name] = (LR.error_stats(got[name], r, r.abs()), BARS['lovasz_loss'])
        elif name == 'errors':
            out[name] = (LR.error_stats(got[name], r, 1.0), BARS['lovasz_errors'])
        elif name == 'dlde':
            out[name] = (LR.error_stats(got[name], r, r.abs()), BARS['lovasz_dlde'])
        else:
            out[name] = (LR.error_stats(got[name], r, LR.scale_of(r)), BARS['lovasz_grad'])
    return out


failures, statlines = LR.failures, LR.statlines


# ================================================================================================ cases
def case(id, F, C, V, content='mix'):
    return dict(id=id, F=F, C=C, V=V, content=content)


CASES = [
    case('F2-C2-V4099-mix', 2, 2, 4099),
    case('F2-C9-V4099-mix', 2, 9, 4099),
    case('F1-C3-V70001-many-tiles-ragged-tail', 1, 3, 70001),
    case('F3-C2-V1-one-voxel', 3, 2, 1, 'one'),
    case('F2-C2-V257-frame-all-ignored', 2, 2, 257, 'frame-ignored'),
    case('F1-C2-V8192-all-foreground', 1, 2, 8192, 'all-fg'),
    case('F1-C4-V8192-constant-logits', 1, 4, 8192, 'const'),
    case('F1-C3-V16384-quantised-tie-runs', 1, 3, 16384, 'quant'),
    case('F1-C2-V16384-saturated-x40', 1, 2, 16384, 'sat'),
    case('F1-C2-scale1-frame', 1, 2, SCALE1[0] * SCALE1[1] * SCALE1[2], 'scale1'),
    case('F4-C2-V36864-guard-buffers', 4, 2, 36864, 'guard'),
]
CASE = {c['id']: c for c in CASES}


def _gen(id):
    return torch.Generator().manual_seed(zlib.crc32(id.encode()) % (1 << 30))


def mix_labels(F, C, V, g, absent_frame=0):
    """a tenth of the voxels occupied (classes 1..C-1), a tenth ignored (255, and labels in [C, 255) among them), the rest class
    0; class C - 1 is absent from frame `absent_frame` only (from the only frame when F = 1)"""
    u = torch.rand(F, V, generator=g)
    lab = torch.zeros(F, V, dtype=torch.uint8)
    occ = torch.randint(1, C, (F, V), generator=g).to(torch.uint8)
    lab = torch.where(u < 0.1, occ, lab)
    other = torch.randint(C, 255, (F, V), generator=g).to(torch.uint8)
    lab = torch.where((u >= 0.1) & (u < 0.15), torch.full_like(lab, 255), lab)
    lab = torch.where((u >= 0.15) & (u < 0.2), other, lab)
    if absent_frame is not None:
        lab[absent_frame][lab[absent_frame] == C - 1] = 0
    return lab


@functools.lru_cache(maxsize=None)
def inputs(id):
    """(logits (F, C, V) float32, labels (F, V) uint8) of a case"""
    c = CASE[id]
    F, C, V, g = c['F'], c['C'], c['V'], _gen(id)
    content = c['content']
    logits = 2 * torch.randn(F, C, V, generator=g)
    if content in ('mix', 'guard'):
        labels = mix_labels(F, C, V, g)
    elif content == 'one':
        labels = torch.tensor([[0], [1], [255]], dtype=torch.uint8)
    elif content == 'frame-ignored':
        labels = mix_labels(F, C, V, g, absent_frame=None)
        labels[1] = 255
    elif content == 'all-fg':                               # U = G at every rank: g = 1 / G everywhere
        labels = torch.where(torch.rand(F, V, generator=g) < 0.1, torch.tensor(255, dtype=torch.uint8), torch.tensor(1, dtype=torch.uint8))
    elif content == 'const':                                # p = (1/2, 1/2, 0, 0) exactly: every error of classes 0 and 1 is 1/2
        labels = mix_labels(F, C, V, g, absent_frame=None)
        logits = torch.tensor([0.0, 0.0, -100.0, -100.0])[None, :, None].expand(F, C, V).contiguous()
    elif content == 'quant':
        labels = mix_labels(F, C, V, g)
        logits = torch.randint(0, 3, (F, C, V), generator=g).float()
    elif content == 'sat':
        labels = mix_labels(F, C, V, g, absent_frame=None)
        logits = 40 * torch.randn(F, C, V, generator=g)
    elif content == 'scale1':                               # a tenth of the 16^3 blocks occupied, 1 % of the voxels ignored
        X, Y, Z = SCALE1
        blocks = (torch.rand(X // 16, Y // 16, Z // 16, generator=g) < 0.1).to(torch.uint8)
        lab = blocks.repeat_interleave(16, 0).repeat_interleave(16, 1).repeat_interleave(16, 2).reshape(1, V)
        labels = torch.where(torch.rand(1, V, generator=g) < 0.01, torch.tensor(255, dtype=torch.uint8), lab)
    else:
        raise ValueError(content)
    return logits.contiguous(), labels.contiguous()


@functools.lru_cache(maxsize=None)
def reference(id):
    """float64 restatement of a case with its own order (computed once, shared; treat as read-only)"""
    logits, labels = inputs(id)
    return lovasz64(logits, labels, WEIGHT, GOUT)


def index_order_dlde(labels, C, f, c):
    """dlde of one (frame, class) when every valid voxel ties: the closed forms evaluated in voxel order"""
    lab = labels[f].long()
    vox = (lab < C).nonzero()[:, 0]
    out = torch.zeros(labels.shape[1], dtype=torch.float64)
    out[vox] = jaccard_increments(lab[vox] == c)
    return out


# ================================================================================================ trainer wiring
def voxel_only_cfg(**extra):
    """base_1d with every head but the voxel head off"""
    from muvo_amd.config import base_1d_cfg
    return base_1d_cfg(**{'EVAL.RGB_SUPERVISION': False, 'LIDAR_RE.ENABLED': False, 'SEMANTIC_SEG.ENABLED': False,
                          'VOXEL_SEG.ENABLED': True, **extra})


def voxel_dicts(seed=0, device='cpu', sizes=((8, 8, 4), (4, 4, 2), (2, 2, 1)), b=1, s=2, C=2):
    """synthetic `batch` / `output` dicts of the voxel head at three scales"""
    g = torch.Generator().manual_seed(seed)
    batch, output = {}, {}
    for f, (x, y, z) in zip((1, 2, 4), sizes):
        lab = mix_labels(b * s, C, x * y * z, g, absent_frame=None)
        batch[f'voxel_label_{f}'] = lab.view(b, s, 1, x, y, z).to(device)
        output[f'voxel_{f}'] = (2 * torch.randn(b, s, C, x, y, z, generator=g)).to(device)
    return batch, output


def float32_errors():
    """{family: max normalised error of the float32 evaluation over the cases} - the MEASURED table"""
    worst = {k: 0.0 for k in MEASURED}
    own = 0.0
    for c in CASES:
        logits, labels = inputs(c['id'])
        ref = reference(c['id'])
        mine = lovasz64(logits, labels, WEIGHT, GOUT, dtype=torch.float32)                        # its own order
        handed = lovasz64(logits, labels, WEIGHT, GOUT, dtype=torch.float32, order_from=ref['errors'])
        a = compare(mine, ref, names=('loss', 'errors'))
        b = compare(handed, ref, names=('dlde', 'dlogits'))
        o = compare(mine, ref, names=('dlogits',))['dlogits'][0]['max_e']
        own = max(own, o)
        row = {'lovasz_loss': a['loss'][0]['max_e'], 'lovasz_errors': a['errors'][0]['max_e'], 'lovasz_dlde': b['dlde'][0]['max_e'],
               'lovasz_grad': b['dlogits'][0]['max_e']}
        for k, v in row.items():
            worst[k] = max(worst[k], v)
        print(f'{c["id"]:42s} ' + '  '.join(f'{k[7:]} {v:.3e}' for k, v in row.items()) + f'  grad(own order) {o:.3e}')
    print(f'gradient of the float32 evaluation with its own order: {own:.3e}')
    return worst


if __name__ == '__main__':
    for fam, v in float32_errors().items():
        print(f'{fam:15s} {v:.2e}   bar {max(4 * v, LR.SCALAR_FLOOR if fam.endswith("_loss") else 0.0):.2e}')
