"""Plain float64 references, a normalised error metric, the case lists and a restatement of the launch arithmetic for the loss and
AdamW kernels (muvo_amd/csrc/losses.hip).  Helpers only: no fixtures, no tests.  tests/test_loss_reference.py (CPU) and
tests/test_loss_kernels_gpu.py (GPU) share everything here, so the bars the GPU test applies are the ones the CPU test proves to
reject planted errors.

The references.  Every function takes `dtype` (default float64): the same code evaluated with dtype=float32 is "the float32 CPU
evaluation" the bars are derived from.  Inputs that already have that dtype are used as they are, so a caller makes its autograd
leaf first and differentiates the result.

The metric.  e = |got - ref64| / den, den a scale of the tensor: max |ref| for a gradient, |ref| for a loss scalar, |p_ref| + lr
for an AdamW parameter.  A reference of exactly 0 (den = 0) demands exactly 0; a NaN in the reference demands a NaN at the same
place.  There is no absolute floor.

The bars.  For each family, 4 x the largest normalised error of the float32 CPU evaluation against float64 over all cases of
the family (`python tests/loss_reference.py` prints the table below from the case lists; it evaluates every case, the largest
ones included), loss scalars floored at 8 * 2^-24.  The factor 4 is for what legitimately differs between the CPU float32
evaluation and a kernel: device expf / logf (~2 ulp against <= 1 ulp), summation order, coefficients handed from the finalize
kernel to the backward kernel as float32.

    family          float32 evaluation, max(e) over the family     bar
    voxel_loss      1.97e-07                                        7.88e-07
    voxel_grad      1.20e-06                                        4.80e-06
    spatial_loss    8.57e-08                                        4.77e-07 (floor)
    spatial_grad    1.44e-07                                        5.76e-07
    kl_loss         1.11e-07                                        4.77e-07 (floor)
    kl_grad         3.23e-07                                        1.29e-06
    l1_loss         8.98e-08                                        4.77e-07 (floor)
    l1_grad         4.75e-08                                        1.90e-07
    segce_map       1.27e-07 (the per-pixel loss map, over its max) 5.08e-07
    segce_grad      2.30e-07                                        9.20e-07
    adamw_p         3.90e-07 (three steps, over |p| + lr)           1.56e-06
    adamw_m         8.31e-08                                        3.32e-07
    adamw_v         8.78e-08                                        3.51e-07

For orientation: one frame's gradient scaled by 1 + 1e-3 shows as max(e) 1e-3, an untouched tail quad as max(e) of order 0.1.
"""
import zlib

import torch
import torch.nn.functional as F

SCALAR_FLOOR = 8 * 2.0 ** -24
# largest normalised error of the float32 CPU evaluation over the family's cases (the table above)
MEASURED = {'voxel_loss': 1.97e-7, 'voxel_grad': 1.20e-6, 'spatial_loss': 8.57e-8, 'spatial_grad': 1.44e-7, 'kl_loss': 1.11e-7,
            'kl_grad': 3.23e-7, 'l1_loss': 8.98e-8, 'l1_grad': 4.75e-8, 'segce_map': 1.27e-7, 'segce_grad': 2.30e-7,
            'adamw_p': 3.90e-7, 'adamw_m': 8.31e-8, 'adamw_v': 8.78e-8}
BARS = {k: max(4 * v, SCALAR_FLOOR if k.endswith('_loss') else 0.0) for k, v in MEASURED.items()}


def f32r(v):
    """The float32 value a C `float` argument receives, as a Python float: the kernels' hyper-parameters ARE these values (with
    beta2 = 0.999, 1 - float32(beta2) differs from 0.001 by 4.7e-5 relative), so the reference is given the same ones."""
    return float(torch.tensor(v, dtype=torch.float32))


# ================================================================================================ references
def _bce1(x):
    """F.binary_cross_entropy(x, 1): -log x with torch's clamp of the log at -100."""
    return -torch.log(x).clamp(min=-100.0)


def voxel_losses64(logits, labels, weight, class_w=None, dtype=torch.float64):
    """(weight * CE, weight * SemScal, weight * GeoScal) of logits (F, C, V), labels uint8 (F, V): VoxelLoss / SemScalLoss /
    GeoScalLoss of the reference project as oracle/muvo_ref.py restates them, every intermediate in `dtype`.

    CE = cross_entropy(reduction='none', weight).mean() over ALL F * V voxels.  The reference defines nothing for a label >= C
    (F.cross_entropy raises); the kernel's documented rule is: a term only for label < C, the divisor stays F * V, no gradient
    for such a voxel.  With ignore_index=255 and reduction='none' that voxel's term is 0 and the mean still divides by F * V,
    which is exactly that rule (and plain cross entropy when no label is 255).
    SemScal / GeoScal select the voxels with label != 255 (torch.where passes no gradient, not even a NaN one, to an unselected
    voxel, like the reference's boolean indexing), keep every `if` of the reference and the clamp of the log at -100.  SemScal
    with no class present is 0 / 0: NaN here and in the kernel (the reference's Python integers would raise)."""
    x = logits.to(dtype)
    nf, C, V = x.shape
    t = labels.long()
    cw = None if class_w is None else torch.as_tensor(class_w).to(dtype)
    ce = F.cross_entropy(x, t, weight=cw, ignore_index=255, reduction='none').mean()
    p = torch.softmax(x, dim=1)
    m = t != 255
    zero = x.new_zeros(())
    sem, count = x.new_zeros(()), 0.0
    for i in range(C):
        ct = (t == i).to(dtype)                       # 255 is no class: ct is 0 on ignored voxels
        if ct.sum() > 0:
            count += 1.0
            pi = torch.where(m, p[:, i], zero)
            nom = (pi * ct).sum()
            if pi.sum() > 0:
                prec = nom / pi.sum()
                if 0 <= prec <= 1:
                    sem = sem + _bce1(prec)
            rec = nom / ct.sum()
            if 0 <= rec <= 1:
                sem = sem + _bce1(rec)
            nct = torch.where(m, 1 - ct, zero)
            if nct.sum() > 0:
                spec = (torch.where(m, 1 - p[:, i], zero) * nct).sum() / nct.sum()
                if 0 <= spec <= 1:
                    sem = sem + _bce1(spec)
    sem = sem / count
    ne_t = torch.where(m, (t != 0).to(dtype), zero)
    e_t = torch.where(m, (t == 0).to(dtype), zero)
    ne_p = torch.where(m, 1 - p[:, 0], zero)
    e_p = torch.where(m, p[:, 0], zero)
    inter = (ne_t * ne_p).sum()
    geo = _bce1(inter / ne_p.sum()) + _bce1(inter / ne_t.sum()) + _bce1((e_t * e_p).sum() / e_t.sum())
    return weight * ce, weight * sem, weight * geo


def voxel_label_facts(labels, C):
    """What the data-dependent branches of SemScal / GeoScal see of the labels: per class T (voxels of the class) and R (unmasked
    voxels of another class), the number of unmasked voxels, and `count` (classes present)."""
    t = labels.long()
    m = t != 255
    T = [int((t == i).sum()) for i in range(C)]
    M = int(m.sum())
    return {'T': T, 'R': [M - v for v in T], 'M': M, 'count': sum(v > 0 for v in T)}


def spatial_loss64(pred, target, parts, ignore=255.0, mask=None, dtype=torch.float64):
    """[weight * SpatialRegressionLoss(norm)(pred[:, c0:c1], target[:, c0:c1]) for (c0, c1, norm, weight) in parts]; pred / target
    (F, Ct, HW); the pixel mask is `mask` (F, HW) when given, else target[:, c0] != ignore; loss = mean over masked pixels of the
    channel sum of |d| (norm 1) or d^2 (norm 2); an empty mask gives 0 (and no gradient)."""
    x, t = pred.to(dtype), target.to(dtype)
    out = []
    for c0, c1, norm, weight in parts:
        d = x[:, c0:c1] - t[:, c0:c1]
        per_pixel = (d.abs() if norm == 1 else d * d).sum(dim=1)
        m = mask.bool() if mask is not None else target[:, c0] != ignore
        out.append(weight * per_pixel[m].mean() if m.any() else (x * 0).sum())
    return out


def _kl_once(pm, ps, qm, qs):
    """KL(q || p) summed over the state, mean over (batch, time); the t = 0 term is the reference's: KL against N(0, 1) with the
    posterior MEAN of t = 0 but the posterior SIGMA of t = 1 (it indexes the already time-shifted tensors)."""
    qv, pv = qs[:, 1:] ** 2, ps[:, 1:] ** 2
    kl = torch.log(ps[:, 1:]) - torch.log(qs[:, 1:]) - 0.5 + (qv + (qm[:, 1:] - pm[:, 1:]) ** 2) / (2 * pv)
    first = -torch.log(qs[:, 1:2]) - 0.5 + (qv[:, :1] + qm[:, :1] ** 2) / 2
    return torch.cat([first, kl], dim=1).sum(-1).mean()


def kl64(pm, ps, qm, qs, weight, alpha, dtype=torch.float64):
    """weight * (alpha * KL(prior | posterior detached) + (1 - alpha) * KL(prior detached | posterior)), inputs (B, T, S), T >= 2"""
    pm, ps, qm, qs = (v.to(dtype) for v in (pm, ps, qm, qs))
    if pm.shape[1] < 2:
        raise ValueError('the first-step term needs T >= 2')
    return weight * (alpha * _kl_once(pm, ps, qm.detach(), qs.detach()) + (1 - alpha) * _kl_once(pm.detach(), ps.detach(), qm, qs))


def l1_rows64(p, t, weight, dtype=torch.float64):
    """weight * mean over rows of sum over the last axis of |p - t|"""
    return weight * (p.to(dtype) - t.to(dtype)).abs().sum(-1).mean()


def seg_ce64(logits, target, class_w=None, dtype=torch.float64):
    """per-pixel -w[t] log softmax(x)[t] of logits (N, C, HW), target (N, HW); a label >= C gives 0 (and no gradient)"""
    x = logits.to(dtype)
    t = target.long()
    t = torch.where(t < x.shape[1], t, torch.full_like(t, -100))
    cw = None if class_w is None else torch.as_tensor(class_w).to(dtype)
    return F.cross_entropy(x, t, weight=cw, ignore_index=-100, reduction='none')


def adamw64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, dtype=torch.float64):
    """One step of torch.optim.AdamW's single-tensor form, in its order of operations: p *= 1 - lr * wd; m = b1 m + (1 - b1) g;
    v = b2 v + (1 - b2) g^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps), g = grad_scale * gradient.  Returns new (p, m, v)."""
    p, g, m, v = (a.to(dtype) for a in (p, g, m, v))
    g = g * grad_scale
    p = p * (1 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - (lr / bc1) * (m / denom), m, v


def grad_of(total, leaves):
    """gradients of a scalar with respect to `leaves`; a total that depends on none of them (all masks empty) gives zeros"""
    if not total.requires_grad:
        return [torch.zeros_like(v) for v in leaves]
    gs = torch.autograd.grad(total, leaves, allow_unused=True)
    return [torch.zeros_like(v) if g is None else g for g, v in zip(gs, leaves)]


# ================================================================================================ metric
def _d(t):
    return torch.as_tensor(t).detach().cpu().double()


def scale_of(ref):
    """max |ref| over the finite elements (0 when there is none)"""
    r = _d(ref)
    r = r[torch.isfinite(r)]
    return float(r.abs().max()) if r.numel() else 0.0


def error_stats(got, ref, den):
    """Normalised error e = |got - ref| / den of `got` against the float64 reference: dict(max_e, rms (of e), index of the worst
    element).  den: a number or a tensor like ref.  Where den is 0 the result must equal the reference exactly; where the
    reference is NaN the result must be NaN and nowhere else (otherwise e = inf there)."""
    g, r = _d(got), _d(ref)
    assert g.shape == r.shape, f'shape {tuple(g.shape)} vs {tuple(r.shape)}'
    den = torch.as_tensor(den, dtype=torch.float64).expand_as(r)
    nan_g, nan_r = torch.isnan(g), torch.isnan(r)
    diff = torch.where(nan_g | nan_r, torch.zeros_like(r), (g - r).abs())
    e = torch.where(diff > 0, diff / den.clamp_min(1e-300), torch.zeros_like(r))
    e = torch.where(nan_g != nan_r, torch.full_like(r, float('inf')), e).reshape(-1)
    if e.numel() == 0:
        return {'max_e': 0.0, 'rms': 0.0, 'index': ()}
    i = int(e.argmax())
    idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), r.shape)) if r.dim() else ()
    return {'max_e': float(e[i]), 'rms': float(e.pow(2).mean().sqrt()), 'index': idx}


def within(stats, bar):
    return stats['max_e'] <= bar


FAMILY_OF = {'ce': 'loss', 'sem': 'loss', 'geo': 'loss', 'loss': 'loss', 'p': 'p', 'm': 'm', 'v': 'v', 'map': 'map'}


def compare(kind, got, ref, lr=None):
    """{name: (stats, bar)} for the named results of one case of family `kind` ('voxel', 'spatial', 'kl', 'l1', 'segce',
    'adamw'): loss scalars are normalised by |ref|, an AdamW parameter by |p_ref| + lr, every other tensor (gradients, the per-pixel
    loss map of the segmentation cross entropy, AdamW moments) by its max |ref|."""
    out = {}
    for name, r in ref.items():
        fam = FAMILY_OF.get(name.split('.')[0], 'grad')
        r = _d(r)
        if fam == 'loss':
            den = r.abs().nan_to_num(0.0)
        elif fam == 'p':
            den = r.abs() + lr
        else:
            den = scale_of(r)
        out[name] = (error_stats(got[name], r, den), BARS[f'{kind}_{fam}'])
    return out


def failures(cmp):
    return {n: s for n, (s, bar) in cmp.items() if not within(s, bar)}


def statlines(tag, cmp):
    return [f'LOSSSTAT {tag} {n}: {s["max_e"]:.3e} {s["rms"]:.3e} ({bar:.2e})' for n, (s, bar) in cmp.items()]


# ================================================================================================ launch arithmetic
def _cdiv(a, b):
    return -(-a // b)


def path(kind, F, C, V, aligned=True):
    """What losses.hip launches, restated from its launchers.  kind:
      'voxel_fwd' / 'voxel_bwd'  (F frames, C classes, V voxels per frame): inst (template argument: 2 for C = 2, else 0 = run-time
                       class count), vec (16-byte logit / 4-byte label loads: V % 4 == 0 and aligned tensors), wg (workgroups per
                       frame: one per 8192 (forward) / 4096 (backward) voxels, capped so that wg * F <= 1280 / 8192), capped,
                       trips (most trips of a thread: each takes four voxels)
      'spatial_fwd'    (F frames, V = HW pixels; C unused): vec, wg (one per 4096 pixels, capped at 1024 / F), capped, trips, flush
                       (a thread reaches the 8-trip flush of its float32 partial sum into the float64 one)
      'adamw'          (V = elements; F, C unused): vec (the two-float4-per-lane kernel: n % 4 == 0, n >= 4096, aligned), wg,
                       partial (the last workgroup of the vector kernel has lanes beyond the end), tail4 (float4 in the last
                       workgroup)."""
    if kind in ('voxel_fwd', 'voxel_bwd'):
        per_wg, cap = (8192, 1280) if kind == 'voxel_fwd' else (4096, 8192)
        wg = _cdiv(V, per_wg)
        capped = wg * F > cap
        if capped:
            wg = max(cap // F, 1)
        return {'inst': 2 if C == 2 else 0, 'vec': V % 4 == 0 and aligned, 'wg': wg, 'capped': capped,
                'trips': _cdiv(_cdiv(V, 4), wg * 256)}
    if kind == 'spatial_fwd':
        wg = (V // 4 + 1023) // 1024
        capped = wg * F > 1024
        if capped:
            wg = max(1024 // F, 1)
        wg = max(wg, 1)
        trips = _cdiv(_cdiv(V, 4), wg * 256)
        return {'vec': V % 4 == 0 and aligned, 'wg': wg, 'capped': capped, 'trips': trips, 'flush': trips >= 8}
    if kind == 'adamw':
        vec = V % 4 == 0 and V >= 4096 and aligned
        if vec:
            n4 = V // 4
            return {'vec': True, 'wg': _cdiv(n4, 512), 'partial': n4 % 512 != 0, 'tail4': n4 % 512 or 512}
        return {'vec': False, 'wg': min(_cdiv(V, 256), 4096), 'partial': V % 256 != 0, 'tail4': 0}     # ew_grid: a grid-stride loop
    raise ValueError(kind)


# ================================================================================================ cases
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


VOXEL_WEIGHT = 0.1                 # LOSSES.WEIGHT_VOXEL
VOXEL_GOUT = (1.0, 2.0, 3.0)       # upstream weights of (CE, SemScal, GeoScal)
PROD_W9 = (1.0, 1.0, 1.0, 1.5, 2.0, 3.0, 1.0, 1.0, 1.0)     # == muvo_amd.losses.VOXEL_SEG_WEIGHTS (asserted by the GPU test)


def vcase(F, C, V, w='none', content='mix', offset='none', **expect):
    """w: 'none' | 'prod' (the 9 production weights) | 'rand'; content: see voxel_inputs; offset: which tensor starts off its
    natural alignment ('logits': one float, 'labels': one byte, 'both'); expect: properties of path('voxel_fwd' / 'voxel_bwd') the
    case exists for, keys 'fwd_<key>' / 'bwd_<key>' / '<key>' (both), a value or ('>=', n)"""
    return dict(F=F, C=C, V=V, w=w, content=content, offset=offset, expect=expect)


VOXEL_CASES = [
    # production grids cropped in frames, the two trained heads
    vcase(2, 2, 192 * 192 * 64, inst=2, vec=True, fwd_trips=('>=', 8)), vcase(2, 9, 192 * 192 * 64, 'prod', inst=0, vec=True),
    vcase(3, 2, 96 * 96 * 32, inst=2, vec=True), vcase(3, 9, 96 * 96 * 32, 'prod', inst=0),
    vcase(4, 2, 48 * 48 * 16, inst=2), vcase(4, 9, 48 * 48 * 16, 'prod', inst=0),
    # class counts with and without weights
    vcase(3, 2, 24576, 'rand'), vcase(3, 3, 24576), vcase(3, 3, 24576, 'rand'), vcase(3, 9, 24576), vcase(3, 16, 24576),
    vcase(3, 16, 24576, 'rand'),
    # scalar loads and tails around one workgroup's span, and tiny frames
    *[vcase(3, c, v, 'prod' if c == 9 else 'none', vec=False) for c in (2, 9) for v in (8191, 8193, 8194, 1, 3, 5)],
    # the workgroup caps binding: 2 / 1 forward workgroups per frame, and the backward cap
    vcase(640, 2, 32768, fwd_capped=True, fwd_wg=2, fwd_trips=('>=', 16)),
    vcase(1040, 2, 32768, fwd_capped=True, fwd_wg=1, fwd_trips=('>=', 16), bwd_capped=True),
    # label content (each takes the matching branches of the finalize kernel)
    *[vcase(3, c, v, 'prod' if c == 9 else 'none', content)
      for c in (3, 9) for content, v in (('absent', 20000), ('one', 20000), ('all255', 20000), ('half255', 20000),
                                         ('tail255', 8194), ('tail255', 20000), ('oneframe', 20000))],
    vcase(3, 2, 20000, content='one'), vcase(3, 2, 20000, content='half255'),
    # views at a storage offset: V % 4 == 0 but the scalar path
    *[vcase(3, c, 20000, 'prod' if c == 9 else 'none', 'half255', off, vec=False) for c in (2, 9) for off in ('logits', 'labels', 'both')],
]


def voxel_paths(case):
    a = case['offset'] == 'none'
    return path('voxel_fwd', case['F'], case['C'], case['V'], a), path('voxel_bwd', case['F'], case['C'], case['V'], a)


def check_expect(expect, paths):
    """assert the path properties a case exists for; paths: {'fwd': ..., 'bwd': ...} or {'': ...}; a key 'fwd_<k>' / 'bwd_<k>' is
    for that side, a plain key for every side"""
    for key, want in expect.items():
        side, k = key.split('_', 1) if key.split('_', 1)[0] in ('fwd', 'bwd') else (None, key)
        for s, p in paths.items():
            if side in (None, s):
                ok = p[k] >= want[1] if isinstance(want, tuple) else p[k] == want
                assert ok, f'{s or "path"}: {k} = {p[k]}, the case needs {want}'


def voxel_id(case):
    f, b = voxel_paths(case)
    tag = f'vox{f["inst"]}-{"vec" if f["vec"] else "scalar"}-F{case["F"]}C{case["C"]}V{case["V"]}-wg{f["wg"]}{"cap" if f["capped"] else ""}' \
          f'x{f["trips"]}trips-bwd{b["wg"]}{"cap" if b["capped"] else ""}-w{case["w"]}-{case["content"]}'
    return tag + ('' if case['offset'] == 'none' else f'-off{case["offset"]}')


def voxel_inputs(case):
    """(logits float32 (F, C, V) with a spread of 2, labels uint8 (F, V), class weights or None).  content: 'mix' 70 % class 0,
    the rest uniform over the other classes; 'absent' the last class never occurs; 'one' every voxel is class 1; 'all255';
    'half255' about half the voxels ignored; 'tail255' the last (partial) quad of every frame ignored; 'oneframe' every frame but
    frame 1 ignored."""
    nf, C, V, content = case['F'], case['C'], case['V'], case['content']
    g = _gen('voxel', nf, C, V, case['w'], content)
    logits = 2.0 * torch.randn(nf, C, V, generator=g)
    hi = C - 1 if content == 'absent' else C
    lab = torch.randint(1, max(hi, 2), (nf, V), generator=g)
    lab = torch.where(torch.rand(nf, V, generator=g) < 0.7, torch.zeros_like(lab), lab).to(torch.uint8)
    if content == 'one':
        lab.fill_(1)
    elif content == 'all255':
        lab.fill_(255)
    elif content == 'half255':
        lab[torch.rand(nf, V, generator=g) < 0.5] = 255
    elif content == 'tail255':
        lab[:, V - (V % 4 or 4):] = 255
    elif content == 'oneframe':
        lab[torch.arange(nf) != 1] = 255
    cw = {'none': None, 'prod': torch.tensor(PROD_W9), 'rand': 0.5 + 2.5 * torch.rand(C, generator=g)}[case['w']]
    return logits, lab, cw


def voxel_reference(logits, lab, cw, dtype=torch.float64, fn=voxel_losses64):
    """{'ce', 'sem', 'geo', 'dlogits'} of one case with the upstream weights VOXEL_GOUT"""
    x = logits.to(dtype).requires_grad_(True)
    ce, sem, geo = fn(x, lab, VOXEL_WEIGHT, cw, dtype=dtype)
    (dl,) = grad_of(VOXEL_GOUT[0] * ce + VOXEL_GOUT[1] * sem + VOXEL_GOUT[2] * geo, [x])
    return {'ce': ce.detach(), 'sem': sem.detach(), 'geo': geo.detach(), 'dlogits': dl}


def scase(F, Ct, HW, parts, ignore='some', mask=None, offset=False, **expect):
    """parts: [(c0, c1, norm, weight)]; ignore: 'some' (~30 % of the pixels carry the ignore value in each part's first channel),
    'none', 'all'; mask: None, 'some' (~20 % set), 'zero'; offset: pred and target start one float off a 16-byte boundary"""
    return dict(F=F, Ct=Ct, HW=HW, parts=parts, ignore=ignore, mask=mask, offset=offset, expect=expect)


RGB = [(0, 3, 1, 0.1)]
LIDAR = [(0, 3, 2, 0.1), (3, 4, 1, 0.05)]           # (0, 3) + (c - 1, c) as the lidar head uses them
SPATIAL_GOUT = (1.5, 0.5)
SPATIAL_CASES = [
    scase(16, 3, 600 * 960, RGB, flush=True, wg=64, capped=True, vec=True), scase(20, 4, 64 * 1024, LIDAR, vec=True),
    scase(6, 3, 192 * 192, [(0, 3, 2, 1.0)], 'none'), scase(6, 3, 192 * 192, [(0, 3, 1, 1.0)], 'none'),
    *[scase(3, 4, hw, LIDAR, vec=False) for hw in (40001, 40002, 40003, 1, 3, 5)],
    scase(3, 4, 36864, LIDAR, 'all'), scase(3, 3, 36864, RGB, 'none', 'some'), scase(3, 3, 36864, RGB, 'some', 'zero'),
    scase(3, 3, 40003, RGB, 'some', 'some', vec=False), scase(3, 3, 600 * 960, RGB, 'none', 'some', trips=('>=', 4)),
    scase(3, 5, 36864, [(0, 2, 2, 0.3), (4, 5, 1, 0.7)]),                       # channels 2, 3 in no part: gradient exactly 0
    scase(3, 4, 36864, LIDAR, offset=True, vec=False),
]


def spatial_id(case):
    p = path('spatial_fwd', case['F'], 0, case['HW'], not case['offset'])
    tag = f'spatial-{"vec" if p["vec"] else "scalar"}-F{case["F"]}c{case["Ct"]}HW{case["HW"]}-wg{p["wg"]}{"cap" if p["capped"] else ""}x{p["trips"]}trips' \
          f'{"-flush" if p["flush"] else ""}-{"+".join(f"{a}:{b}n{n}" for a, b, n, _ in case["parts"])}-ign{case["ignore"]}'
    return tag + (f'-mask{case["mask"]}' if case['mask'] else '') + ('-offset' if case['offset'] else '')


def spatial_inputs(case):
    """(pred, target float32 (F, Ct, HW), mask uint8 (F, HW) or None)"""
    nf, Ct, HW = case['F'], case['Ct'], case['HW']
    g = _gen('spatial', nf, Ct, HW, case['parts'], case['ignore'], case['mask'])
    pred, target = torch.randn(nf, Ct, HW, generator=g), torch.rand(nf, Ct, HW, generator=g)
    for c0, _, _, _ in case['parts']:
        if case['ignore'] == 'some':
            target[:, c0][torch.rand(nf, HW, generator=g) < 0.3] = 255.0
        elif case['ignore'] == 'all':
            target[:, c0] = 255.0
    mask = None
    if case['mask'] == 'some':
        mask = (torch.rand(nf, HW, generator=g) < 0.2).to(torch.uint8)
    elif case['mask'] == 'zero':
        mask = torch.zeros(nf, HW, dtype=torch.uint8)
    return pred, target, mask


def spatial_reference(case, pred, target, mask, dtype=torch.float64):
    x = pred.to(dtype).requires_grad_(True)
    losses = spatial_loss64(x, target, case['parts'], 255.0, mask, dtype=dtype)
    (dp,) = grad_of(sum(g * l for g, l in zip(SPATIAL_GOUT, losses)), [x])
    return {**{f'loss.{i}': l.detach() for i, l in enumerate(losses)}, 'dpred': dp}


KL_WEIGHT, KL_GOUT = 1e-3, 1.7
KL_CASES = [(2, 10, 512, 0.75), (8, 12, 512, 0.75), (8, 12, 512, 0.0), (8, 12, 512, 1.0), (3, 2, 512, 0.75), (3, 5, 1, 0.75),
            (3, 5, 33, 0.75), (2, 2, 1, 0.0), (2, 3, 33, 1.0)]          # (B, T, S, alpha)


def kl_inputs(case):
    B, T, S, _ = case
    g = _gen('kl', case)
    pm, qm = torch.randn(B, T, S, generator=g), torch.randn(B, T, S, generator=g)
    ps, qs = (0.1 + 2 * torch.rand(B, T, S, generator=g) for _ in range(2))     # the range of 2 sigmoid(x / 2) + 0.1
    return pm, ps, qm, qs


def kl_reference(case, inputs, dtype=torch.float64):
    leaves = [v.to(dtype).requires_grad_(True) for v in inputs]
    loss = kl64(*leaves, KL_WEIGHT, case[3], dtype=dtype)
    gs = grad_of(KL_GOUT * loss, leaves)
    return {'loss': loss.detach(), **{n: g for n, g in zip(('dpm', 'dps', 'dqm', 'dqs'), gs)}}


L1_GOUT = 0.6
L1_CASES = [(20, 1), (24, 2), (96, 1), (257, 3), (300, 3)]          # (rows, cols)


def l1_inputs(case):
    rows, cols = case
    g = _gen('l1', case)
    p, t = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    t[::3] = p[::3]                  # p == t exactly: sign 0
    return p, t


def l1_reference(case, p, t, dtype=torch.float64):
    x = p.to(dtype).requires_grad_(True)
    loss = l1_rows64(x, t, 1.0, dtype=dtype)
    (dp,) = grad_of(L1_GOUT * loss, [x])
    return {'loss': loss.detach(), 'dp': dp}


SEGCE_CASES = [(2, 9, 64 * 1024, 'prod'), (2, 9, 4099, 'none')]     # (N, C, HW, weights); labels 9..11 and 255 occur: loss, gradient 0


def segce_inputs(case):
    N, C, HW, w = case
    g = _gen('segce', case)
    logits = 2.0 * torch.randn(N, C, HW, generator=g)
    t = torch.randint(0, C + 3, (N, HW), generator=g).to(torch.uint8)
    t[:, ::17] = 255
    return logits, t, torch.tensor(PROD_W9) if w == 'prod' else None, torch.rand(N, HW, generator=g)


def segce_reference(case, logits, t, cw, gloss, dtype=torch.float64):
    x = logits.to(dtype).requires_grad_(True)
    loss = seg_ce64(x, t, cw, dtype=dtype)
    (dl,) = grad_of((loss * gloss.to(dtype)).sum(), [x])
    return {'map': loss.detach(), 'dlogits': dl}


def acase(n, grad_scale=1.0, wd=0.01, steps=(1, 2, 3), zeros=False, offset=False, **expect):
    """steps: the step numbers of three consecutive calls; zeros: a third of the gradient is exactly 0 in every step (v stays 0
    there: denominator eps); offset: the tensors start one element off a 16-byte boundary"""
    return dict(n=n, grad_scale=grad_scale, wd=wd, steps=steps, zeros=zeros, offset=offset, expect=expect)


ADAMW_HP = dict(lr=f32r(3e-4), beta1=f32r(0.9), beta2=f32r(0.999), eps=f32r(1e-8))
ADAMW_CASES = [
    acase(4096, vec=True, wg=2, partial=False), acase(4092, vec=False), acase(4100, vec=True, wg=3, tail4=1),
    acase(4096 + 4 * 511, vec=True, partial=True, tail4=511), acase(512 * 4 * 3 + 4, vec=True, wg=4, tail4=1),
    acase(1 << 22, vec=True, partial=False), acase(10007, vec=False),
    acase(4096 + 4 * 511, 0.125, 0.0, vec=True), acase(10007, 0.125, 0.0, vec=False), acase(4100, 0.125, vec=True),
    acase(4096, steps=(10000, 10001, 10002), vec=True), acase(4092, steps=(10000, 10001, 10002), vec=False),
    acase(4100, zeros=True, vec=True), acase(4092, zeros=True, vec=False), acase(4100, offset=True, vec=False),
]


def adamw_id(case):
    p = path('adamw', 0, 0, case['n'], not case['offset'])
    tag = f'adamw-{"vec" if p["vec"] else "scalar"}-n{case["n"]}-wg{p["wg"]}{"partial" if p["partial"] else ""}-gs{case["grad_scale"]}-wd{case["wd"]}-step{case["steps"][0]}'
    return tag + ('-zeros' if case['zeros'] else '') + ('-offset' if case['offset'] else '')


def adamw_inputs(case):
    """(p0, m0, v0, [g of each step]): step numbers > 1 at the start mean a state from earlier steps, so m0, v0 are not zero"""
    n = case['n']
    g = _gen('adamw', n, case['grad_scale'], case['wd'], case['steps'], case['zeros'])
    p0 = torch.randn(n, generator=g)
    warm = case['steps'][0] > 1
    m0 = 0.1 * torch.randn(n, generator=g) if warm else torch.zeros(n)
    v0 = 0.01 * torch.rand(n, generator=g) if warm else torch.zeros(n)
    grads = [torch.randn(n, generator=g) * (1 + k) for k in range(len(case['steps']))]
    if case['zeros']:
        for gr in grads:
            gr[::3] = 0.0
    return p0, m0, v0, grads


def adamw_reference(case, p0, m0, v0, grads, dtype=torch.float64, fn=adamw64):
    p, m, v = p0, m0, v0
    for step, g in zip(case['steps'], grads):
        p, m, v = fn(p, g, m, v, ADAMW_HP['lr'], ADAMW_HP['beta1'], ADAMW_HP['beta2'], ADAMW_HP['eps'], f32r(case['wd']), step,
                     f32r(case['grad_scale']), dtype=dtype)
    return {'p': p, 'm': m, 'v': v}


# ================================================================================================ the table in the docstring
def float32_errors(kind, max_elements=None):
    """{name: largest normalised error of the float32 CPU evaluation against float64} over the cases of `kind` (all of them, or
    those with at most max_elements input elements)"""
    worst = {}

    def note(cmp):
        for n, (s, _) in cmp.items():
            fam = FAMILY_OF.get(n.split('.')[0], 'grad')
            worst[fam] = max(worst.get(fam, 0.0), s['max_e'])

    if kind == 'voxel':
        for c in VOXEL_CASES:
            if max_elements and c['F'] * c['C'] * c['V'] > max_elements:
                continue
            inp = voxel_inputs(c)
            note(compare('voxel', voxel_reference(*inp, dtype=torch.float32), voxel_reference(*inp)))
    elif kind == 'spatial':
        for c in SPATIAL_CASES:
            if max_elements and c['F'] * c['Ct'] * c['HW'] > max_elements:
                continue
            inp = spatial_inputs(c)
            note(compare('spatial', spatial_reference(c, *inp, dtype=torch.float32), spatial_reference(c, *inp)))
    elif kind == 'kl':
        for c in KL_CASES:
            inp = kl_inputs(c)
            note(compare('kl', kl_reference(c, inp, dtype=torch.float32), kl_reference(c, inp)))
    elif kind == 'l1':
        for c in L1_CASES:
            inp = l1_inputs(c)
            note(compare('l1', l1_reference(c, *inp, dtype=torch.float32), l1_reference(c, *inp)))
    elif kind == 'segce':
        for c in SEGCE_CASES:
            inp = segce_inputs(c)
            note(compare('segce', segce_reference(c, *inp, dtype=torch.float32), segce_reference(c, *inp)))
    elif kind == 'adamw':
        for c in ADAMW_CASES:
            if max_elements and c['n'] > max_elements:
                continue
            inp = adamw_inputs(c)
            note(compare('adamw', adamw_reference(c, *inp, dtype=torch.float32), adamw_reference(c, *inp), lr=ADAMW_HP['lr']))
    return worst


if __name__ == '__main__':
    import time
    for kind in ('l1', 'kl', 'segce', 'adamw', 'spatial', 'voxel'):
        t0 = time.time()
        for fam, e in float32_errors(kind).items():
            print(f'{kind}_{fam:6s} float32 evaluation max(e) {e:.2e}   4x = {4 * e:.2e}   bar in use {BARS[f"{kind}_{fam}"]:.2e}   '
                  f'({time.time() - t0:.0f} s)', flush=True)
