"""Evaluation metrics of the validation path on the GPU: the reference's SSIMMetric, PSNRMetric,
CDMetric and SSCMetrics (muvo/metrics.py:47-317) as driven by WorldModelTrainer.add_metrics / compute_ssc_metrics
(muvo/trainer.py:426-490), computed by the HIP kernels of csrc/metrics.hip through the C ABI.  Same class names, methods
and running-average semantics (including the reference's `count = 1e-8` start value); no CPU fallback.

JaccardIndex is the multiclass, per-class form of torchmetrics.JaccardIndex the reference's trainer keeps per segmentation
head (trainer.py:74-178): a confusion matrix counted on the device by one kernel per update (argmax fused in), read once per
epoch in compute()."""
import ctypes as C

import numpy as np
import torch

from . import ops


def _gauss_window(window_size=11, sigma=1.5):
    """losses.py:304-314: the 2-D window exactly as the reference builds it (fp32 outer product of the normalised 1-D
    Gaussian)."""
    x = torch.arange(window_size)
    g = torch.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2))
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().contiguous()


def ssim_frames(prediction, target, window_size=11, sigma=1.5, L=1.0):
    """SSIMLoss._ssim (losses.py:316-339): per-frame mean of the SSIM map.  (b, s, c, h, w) -> (b*s,) float32."""
    assert window_size == 11, 'the kernel is built for the reference window (11)'
    b, s, c, h, w = prediction.shape
    p, t = prediction.float().contiguous(), target.float().contiguous()
    win = _gauss_window(window_size, sigma).to(p.device)
    sums = torch.zeros(b * s, dtype=torch.float64, device=p.device)
    ops._ck(ops.lib().muvo_ssim_frames(ops._f(p), ops._f(t), ops._f(win), ops._p(sums), b * s, c, h, w,
                                       ops._fl((0.01 * L) ** 2), ops._fl((0.03 * L) ** 2), ops._st()))
    return (sums / (c * (h - window_size + 1) * (w - window_size + 1))).float()


def psnr_frames(prediction, target, max_pixel_val=1.0):
    """PSNRMetric.psnr (metrics.py:305-309): (b, s, c, h, w) -> (b, s)."""
    b, s = prediction.shape[:2]
    L = prediction[0, 0].numel()
    p, t = prediction.float().contiguous(), target.float().contiguous()
    sums = torch.zeros(b * s, dtype=torch.float64, device=p.device)
    ops._ck(ops.lib().muvo_sqdiff_frames(ops._f(p), ops._f(t), ops._p(sums), b * s, ops._i64(L), ops._st()))
    mse = (sums / L).float().view(b, s)
    return 20 * torch.log10(max_pixel_val / torch.sqrt(mse))


def chamfer_frames(prediction, target):
    """CDMetric.add_batch with reducer = mean (metrics.py:243-249): (n, P, 3), (n, Q, 3) -> (n,)."""
    n, P, _ = prediction.shape
    Q = target.shape[1]
    a, b = prediction.float().contiguous(), target.float().contiguous()
    sums = torch.zeros(n, 2, dtype=torch.float64, device=a.device)
    ops._ck(ops.lib().muvo_chamfer_sums(ops._f(a), ops._f(b), ops._p(sums), n, P, Q, ops._st()))
    # dist.min(1) runs over the prediction points (one value per target point), dist.min(2) over the target points
    return ((sums[:, 1] / Q + sums[:, 0] / P) / 2).float()


def ssc_counts(logits, label, n_classes):
    """argmax + SSCMetrics counts (trainer.py:482-490, metrics.py:77-100,143-214).  logits (n, C, x, y, z) float32, label
    (n, x, y, z) uint8 with 255 = ignore -> (completion[3], tps[C], fps[C], fns[C]) int64 device tensors."""
    n, c = logits.shape[:2]
    assert c == n_classes
    V = logits[0, 0].numel()
    lg, lb = logits.float().contiguous(), label.to(torch.uint8).contiguous()
    counts = torch.zeros(3 + 3 * c, dtype=torch.int64, device=lg.device)
    ops._ck(ops.lib().muvo_ssc_counts(ops._f(lg), ops._p(lb), ops._p(counts), ops._i64(n), c, ops._i64(V), ops._st()))
    per = counts[3:].view(c, 3)
    return counts[:3], per[:, 0], per[:, 1], per[:, 2]


SEG_MAX_CLASSES = 16        # SEG_MAXC of csrc/metrics.hip


def _class_bytes(x, n_classes):
    """Integer class map -> contiguous uint8 with every value outside [0, n_classes) turned into 255, which the kernel counts
    as out of range (a plain .to(torch.uint8) would wrap -1 or 256 into a valid class).  uint8 input passes as it is."""
    if x.dtype == torch.uint8:
        return x.contiguous()
    if x.is_floating_point() or x.dtype == torch.bool or x.is_complex():
        raise TypeError(f'seg_confusion: class indices must be an integer tensor, got {x.dtype}')
    if x.dtype == torch.int8:                        # 255 does not fit
        x = x.to(torch.int16)
    return x.masked_fill((x < 0) | (x >= n_classes), 255).to(torch.uint8).contiguous()


def seg_confusion(preds, target, n_classes, out=None):
    """Confusion counts of a segmentation head, argmax fused in.  preds: float logits (N, C, ...) or integer class indices
    shaped like target; target: integer class map (N, ...) or (N, 1, ...).  -> int64 (C*C + 1,) device tensor: entry t*C + p
    counts the pixels with label t and prediction p, the last entry those whose label (index path: or prediction) is outside
    [0, C).  `out`: such a tensor to ADD into instead of a fresh one.  One kernel launch, no host read."""
    c = int(n_classes)
    if not 2 <= c <= SEG_MAX_CLASSES:
        raise ValueError(f'seg_confusion: n_classes={c} unsupported (2..{SEG_MAX_CLASSES})')
    if out is None:
        out = torch.zeros(c * c + 1, dtype=torch.int64, device=preds.device)
    assert out.dtype == torch.int64 and out.shape == (c * c + 1,)
    if preds.is_floating_point():
        if preds.dim() < 2 or preds.shape[1] != c:
            raise ValueError(f'seg_confusion: logits {tuple(preds.shape)} need {c} classes in dimension 1')
        n = preds.shape[0]
        P = preds[0, 0].numel()
        if target.numel() != n * P:
            raise ValueError(f'seg_confusion: target {tuple(target.shape)} does not match logits {tuple(preds.shape)}')
        if n * P == 0:
            return out
        lg, lb = preds.detach().float().contiguous(), _class_bytes(target, c)
        ops._ck(ops.lib().muvo_seg_confusion(ops._f(lg), ops._p(lb), ops._p(out), ops._i64(n), c, ops._i64(P), ops._st()))
    else:
        if target.numel() != preds.numel():
            raise ValueError(f'seg_confusion: target {tuple(target.shape)} does not match predictions {tuple(preds.shape)}')
        if preds.numel() == 0:
            return out
        pr, lb = _class_bytes(preds, c), _class_bytes(target, c)
        ops._ck(ops.lib().muvo_seg_confusion_index(ops._p(pr), ops._p(lb), ops._p(out), ops._i64(pr.numel()), c, ops._st()))
    return out


def jaccard_from_confmat(confmat):
    """torchmetrics' _jaccard_index_reduce with average='none': (C, C) integer matrix [label, prediction] -> float32 (C,)
    intersection / union per class; a class absent from both prediction and label (union 0) scores 0.  Any device."""
    num = confmat.diag()
    den = confmat.sum(0) + confmat.sum(1) - num
    num, den = num.float(), den.float()
    return torch.where(den != 0, num / den, torch.zeros_like(num))


class JaccardIndex:
    """torchmetrics.JaccardIndex(task='multiclass', num_classes=C, average='none') as the reference's trainer uses it
    (trainer.py:74-178,427-478,525-554).  update() takes the head's LOGITS (N, C, ...) - the argmax of trainer.py:429 happens in
    the counting kernel - or integer predictions, launches that kernel and nothing else; the (C, C) int64 matrix `confmat`
    [label, prediction] and the count `out_of_range` stay on the device until compute() reads them once.  The reference's metric
    raises on the first batch holding a label outside [0, C); here compute() raises with their count (validate_args=True) or
    leaves such pixels out (False)."""

    def __init__(self, task='multiclass', num_classes=None, average='none', validate_args=True, device=None):
        if task != 'multiclass':
            raise NotImplementedError(f"JaccardIndex: task={task!r} is not built (only 'multiclass')")
        if average != 'none':
            raise NotImplementedError(f"JaccardIndex: average={average!r} is not built (only 'none')")
        if num_classes is None or not 2 <= int(num_classes) <= SEG_MAX_CLASSES:
            raise ValueError(f'JaccardIndex: num_classes={num_classes} unsupported (2..{SEG_MAX_CLASSES})')
        self.num_classes, self.validate_args = int(num_classes), validate_args
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        c = self.num_classes
        self._counts = torch.zeros(c * c + 1, dtype=torch.int64, device=self.device)
        self.confmat, self.out_of_range = self._counts[:c * c].view(c, c), self._counts[c * c]

    def update(self, preds, target):
        seg_confusion(preds, target, self.num_classes, out=self._counts)

    __call__ = update

    def compute(self, with_confmat=False):
        """float32 (C,) scores on the host; with_confmat=True: (scores, the host copy of confmat they were computed from)."""
        c = self.num_classes
        counts = self._counts.cpu()                      # the one host read of an epoch
        bad = int(counts[c * c])
        if bad and self.validate_args:
            raise RuntimeError(f'JaccardIndex: {bad} pixels carry a label outside [0, {c}) (validate_args=False leaves them out)')
        confmat = counts[:c * c].view(c, c)
        scores = jaccard_from_confmat(confmat)
        return (scores, confmat) if with_confmat else scores

    def reset(self):
        self._counts.zero_()


class SSIMMetric:
    """metrics.py:219-235."""

    def __init__(self, channel=3, window_size=11, sigma=1.5, L=1, non_negative=False):
        self.window_size, self.sigma, self.L, self.non_negative = window_size, sigma, L, non_negative
        self.reset()

    def add_batch(self, prediction, target):
        self.count += 1
        v = ssim_frames(prediction, target, self.window_size, self.sigma, self.L)
        if self.non_negative:
            v = torch.relu(v)
        self.ssim_score += v.mean()
        self.ssim_avg = self.ssim_score / self.count

    def get_stat(self):
        return self.ssim_avg

    def reset(self):
        self.ssim_score, self.count, self.ssim_avg = 0, 1e-8, 0


class PSNRMetric:
    """metrics.py:295-317."""

    def __init__(self, max_pixel_val=1.0):
        self.max_pixel_value = max_pixel_val
        self.reset()

    def add_batch(self, prediction, target):
        self.count += 1
        self.total_psnr += self.psnr(prediction, target).mean()
        self.avg_psnr = self.total_psnr / self.count

    def psnr(self, prediction, target):
        return psnr_frames(prediction, target, self.max_pixel_value)

    def get_stat(self):
        return self.avg_psnr

    def reset(self):
        self.total_psnr, self.count, self.avg_psnr = 0, 1e-8, 0


class CDMetric:
    """metrics.py:238-258 (reducer fixed to the mean the trainer uses)."""

    def __init__(self, reducer=torch.mean):
        assert reducer is torch.mean, 'only the mean reducer of the reference trainer is implemented'
        self.reset()

    def add_batch(self, prediction, target):
        self.count += 1
        self.total_cost += chamfer_frames(prediction, target).mean()
        self.avg_cost = self.total_cost / self.count

    def get_stat(self):
        return self.avg_cost

    def reset(self):
        self.total_cost, self.count, self.avg_cost = 0, 1e-8, 0


class SSCMetrics:
    """metrics.py:47-141.  add_batch takes the voxel LOGITS (the argmax of trainer.py:487 is fused into the kernel) or an
    already arg-maxed integer prediction."""

    def __init__(self, n_classes):
        self.n_classes = n_classes
        self.reset()

    def add_batch(self, y_pred, y_true, nonempty=None, nonsurface=None):
        assert nonempty is None and nonsurface is None, 'the reference trainer never passes masks'
        self.count += 1
        if not y_pred.is_floating_point():      # class indices -> one-hot "logits"
            y_pred = torch.nn.functional.one_hot(y_pred.long(), self.n_classes).movedim(-1, 1).float()
        comp, tps, fps, fns = ssc_counts(y_pred, y_true, self.n_classes)
        self._comp += comp
        self.tps += tps
        self.fps += fps
        self.fns += fns
        self.compute()

    def compute(self):
        tp, fp, fn = (int(v) for v in self._comp.tolist())
        self.completion_tp, self.completion_fp, self.completion_fn = tp, fp, fn
        if tp != 0:
            self.precision, self.recall, self.iou = tp / (tp + fp), tp / (tp + fn), tp / (tp + fp + fn)
        else:
            self.precision, self.recall, self.iou = 0, 0, 0
        self.iou_ssc = self.tps.float() / (self.tps + self.fps + self.fns + 1e-5).float()

    def get_stats(self):
        return {'precision': self.precision, 'recall': self.recall, 'iou': self.iou, 'iou_ssc': self.iou_ssc,
                'iou_ssc_mean': torch.mean(self.iou_ssc[1:])}

    def reset(self):
        dev = torch.device('cuda', torch.cuda.current_device())
        self._comp = torch.zeros(3, dtype=torch.int64, device=dev)
        self.tps, self.fps, self.fns = (torch.zeros(self.n_classes, dtype=torch.int64, device=dev) for _ in range(3))
        self.completion_tp = self.completion_fp = self.completion_fn = 0
        self.precision = self.recall = self.iou = 0
        self.count = 1e-8
        self.iou_ssc = torch.zeros(self.n_classes, dtype=torch.float32, device=dev)


class VoxelUnknownShare:
    """`{prefix}_Voxel_Unknown_Share` (extension, config.py: VOXEL_SEG.VISIBILITY): the share of the label cells at scale 1 that
    the visibility mask sets to 255, over the frames of one metric set.  add_batch marks and applies the frames' labels again -
    the batch's masked labels carry no count, and a metric set sees a slice of the frames - and only queues kernels: the (2,)
    integer counts of muvo_visibility_apply stay on the device until get_stat."""

    def __init__(self):
        self.reset()

    def add_batch(self, label, rays):
        from muvo_amd import ops
        if not label.shape[0]:
            return
        if self.counts is None:
            self.counts = torch.zeros(2, dtype=torch.int64, device=label.device)
        ops.visible_labels(label, rays, self.counts)
        self.cells += label.numel()

    def get_stat(self):
        return int(self.counts[1]) / self.cells if self.cells else 0.0

    def reset(self):
        self.counts, self.cells = None, 0


class VoxelFilledShare:
    """`{prefix}_Voxel_Filled_Share` and `{prefix}_Voxel_Unknown_Share_Aggregated` (extension, config.py: VOXEL_SEG.AGGREGATE): of
    the label cells at scale 1, the share that was unknown to its own frame and filled from a neighbouring one (occupied or free),
    and the share that stays 255 after that.  add_batch adds the batch's (3,) counts of muvo_voxel_aggregate - whole batches: a
    frame is filled from frames on both sides of any slice - on the device; get_stat reads them."""

    def __init__(self):
        self.reset()

    def add_batch(self, counts, cells):
        self.counts = counts.clone() if self.counts is None else self.counts + counts
        self.cells += int(cells)

    def get_stat(self):
        if not self.cells:
            return 0.0, 0.0
        occupied, free, unknown = (int(v) for v in self.counts.tolist())
        return (occupied + free) / self.cells, unknown / self.cells

    def reset(self):
        self.counts, self.cells = None, 0


class EvalMetrics:
    """The metric set of one validation dataloader on base_1d (trainer.py:426-490): ssim, psnr, cd, ssc."""

    def __init__(self, n_classes=2, scale=50.0):
        self.scale = scale
        self.ssim, self.psnr, self.cd, self.ssc = SSIMMetric(channel=3), PSNRMetric(1.0), CDMetric(), SSCMetrics(n_classes)

    def add_batch(self, rgb_pred, rgb_target, rv_pred, rv_target, cd_index, voxel_logits, voxel_label):
        self.ssim.add_batch(prediction=rgb_pred, target=rgb_target)
        self.psnr.add_batch(prediction=rgb_pred, target=rgb_target)
        pt = rv_target.permute(0, 1, 3, 4, 2).flatten(2, 3).flatten(0, 1) * self.scale      # trainer.py:450-456
        pp = rv_pred.permute(0, 1, 3, 4, 2).flatten(2, 3).flatten(0, 1) * self.scale
        idx = torch.as_tensor(cd_index, device=pp.device).long()
        self.cd.add_batch(pp[:, idx, :-1], pt[:, idx, :-1])
        b, s, c, x, y, z = voxel_logits.shape
        self.ssc.add_batch(voxel_logits.reshape(b * s, c, x, y, z), voxel_label.reshape(b * s, x, y, z))

    def stats(self):
        st = self.ssc.get_stats()
        return dict(ssim=float(self.ssim.get_stat()), psnr=float(self.psnr.get_stat()), cd=float(self.cd.get_stat()),
                    precision=st['precision'], recall=st['recall'], iou=st['iou'], iou_ssc=st['iou_ssc'],
                    iou_ssc_mean=float(st['iou_ssc_mean']),
                    completion=[self.ssc.completion_tp, self.ssc.completion_fp, self.ssc.completion_fn],
                    tps=self.ssc.tps.tolist(), fps=self.ssc.fps.tolist(), fns=self.ssc.fns.tolist())
