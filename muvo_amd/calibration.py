"""Calibration and uncertainty of the voxel head over the imagined samples (the definitions:
include/muvo_hip.h, muvo_voxel_calibration).  An extension: the reference decodes every sample drawn from the RSSM prior, scores its
argmax on its own and drops it.  Here the K samples of a batch are read jointly, once, by one kernel (csrc/calibration.hip) that
leaves integer accumulators on the device; nothing crosses to the host before `VoxelCalibrationMetric.result()`.

    ensemble_calibration     K logit tensors + label -> reliability table, counts, ensemble SSC counts, fixed-point sums [, maps]
    VoxelCalibrationMetric   `predict --mode test --voxel-calibration` -> OUT/voxel_calibration.json
    uncert_panel             the `_uncert` strip (`predict --panels N --uncert`, `train --panel-dir DIR --uncert`)"""
import json
import os

import numpy as np
import torch

DEFAULT_BINS = 15
COUNT_NAMES = ('voxels', 'ignored', 'skipped_nonfinite', 'correct')                 # counts (4,) of ops.voxel_calibration
SUM_NAMES = ('brier', 'nll', 'entropy_correct', 'entropy_wrong', 'mi_correct', 'mi_wrong')      # sums (6,), in units of 2^-24
FIX = float(1 << 24)
# level k of a byte map: black - red - yellow - white, each channel a clipped line; r + g + b = 3 k, so the level can be read back
UNCERT_COLOURS = tuple((min(255, 3 * k), min(255, max(0, 3 * k - 255)), max(0, 3 * k - 510)) for k in range(256))


def _frames(x, tail):
    """(b, s, ...) or (F, ...) with `tail` trailing axes -> (frames, lead shape)"""
    lead = tuple(x.shape[:x.dim() - tail])
    if len(lead) not in (1, 2):
        raise ValueError(f'ensemble_calibration: (b, s, ...) or (F, ...) tensors, got {tuple(x.shape)}')
    return x.reshape(-1, *x.shape[x.dim() - tail:]), lead


def new_accumulators(n_classes, bins, device, groups=None):
    """Zeroed table, counts, ssc, sums on `device`; with groups = G each gets a leading axis of G (slices are contiguous)."""
    lead = () if groups is None else (int(groups),)
    z = lambda *shape: torch.zeros(lead + shape, dtype=torch.int64, device=device)      # noqa: E731
    return dict(table=z(int(bins), 3), counts=z(4), ssc=z(3 + 3 * int(n_classes)), sums=z(6))


def ensemble_calibration(logits_list, label, bins=DEFAULT_BINS, maps=False, into=None):
    """logits_list: K tensors (b, s, C, X, Y, Z) or (F, C, X, Y, Z) fp32, one per sample; label (b, s, X, Y, Z) / (b, s, 1, X, Y, Z) /
    (F, X, Y, Z) uint8 with 255 = ignore -> dict(table (B, 3), counts (4,), ssc (3 + 3 C,), sums (6,)), int64 device tensors as
    ops.voxel_calibration leaves them (`into`: such a dict to add to instead of fresh zeros), and with maps=True also `ens`
    (..., X, Y, Z), `top_entropy` and `top_mi` (..., X, Y) uint8 with the leading axes of the logits."""
    from muvo_amd import ops
    frames = []
    lead = None
    for t in logits_list:
        f, lead_t = _frames(t.detach(), 4)
        if lead is not None and lead_t != lead:
            raise ValueError('ensemble_calibration: samples of one shape')
        lead = lead_t
        frames.append(f.float())
    if not frames:
        raise ValueError('ensemble_calibration: at least one sample')
    F, Cn, X, Y, Z = frames[0].shape
    lab = label.detach().reshape(F, X, Y, Z)
    lab = lab if lab.dtype == torch.uint8 else lab.to(torch.uint8)
    acc = into if into is not None else new_accumulators(Cn, bins, lab.device)
    out = dict(acc)
    extra = {}
    if maps:
        extra = dict(ens=torch.empty((F, X, Y, Z), dtype=torch.uint8, device=lab.device),
                     top_entropy=torch.empty((F, X, Y), dtype=torch.uint8, device=lab.device),
                     top_mi=torch.empty((F, X, Y), dtype=torch.uint8, device=lab.device))
    ops.voxel_calibration(frames, lab, acc['table'], acc['counts'], acc['ssc'], acc['sums'], **extra)
    for name, t in extra.items():
        out[name] = t.reshape(*lead, *t.shape[1:])
    return out


def _voxel_label(cfg, batch):
    from muvo_amd.trainer import voxel_target
    label = voxel_target(cfg, batch, 1)
    return label[:, :, 0] if label.dim() == 6 else label


class VoxelCalibrationMetric:
    """`predict --mode test --voxel-calibration`: per loader the calibration (ECE, MCE, reliability table, Brier score, NLL), the
    ensemble's accuracy and IoU and the mean predictive entropy and mutual information over correct and over wrong voxels - of the
    reconstructed frames (K = 1) against the label's `[:, :rf]` and, apart from them, of ALL imagined samples jointly (K =
    PREDICTION.N_SAMPLES) against `[:, rf:rf + fh]`.  The label is `trainer.voxel_target(cfg, batch, 1)`: with the visibility mask on,
    unobserved cells are 255 and ignored.  `update` is the per-batch hook of predict.run and only queues kernels (int64 accumulators
    stay on the device); `result()` reads them once per loader."""

    def __init__(self, cfg, prefix='test', bins=DEFAULT_BINS):
        from muvo_amd import ops
        if not 1 <= int(bins) <= ops.CALIBRATION_MAX_BINS:
            raise ValueError(f'VoxelCalibrationMetric: {bins} bins (1..{ops.CALIBRATION_MAX_BINS})')
        self.cfg, self.prefix, self.bins = cfg, prefix, int(bins)
        self.loader = None
        self.acc = {}

    def start_loader(self, idx):
        self.loader = str(idx)
        self.acc[self.loader] = dict(buffers=None, samples=0)

    def _add(self, a, which, label, logits_list):
        if not label.shape[0] * label.shape[1]:
            return
        if a['buffers'] is None:
            a['buffers'] = new_accumulators(logits_list[0].shape[2], self.bins, label.device, groups=2)
        ensemble_calibration(logits_list, label, into={k: v[which] for k, v in a['buffers'].items()})

    def update(self, i, batch, output, output_imagines):
        from muvo_amd import ops
        if self.loader is None:
            self.start_loader(0)
        a = self.acc[self.loader]
        label = _voxel_label(self.cfg, batch)
        rf = output['voxel_1'].shape[1]
        with torch.no_grad():
            self._add(a, 0, label[:, :rf], [output['voxel_1']])
            if output_imagines:
                if len(output_imagines) > ops.CALIBRATION_MAX_SAMPLES:
                    raise ValueError(f'VoxelCalibrationMetric: {len(output_imagines)} imagined samples (at most {ops.CALIBRATION_MAX_SAMPLES} per call)')
                fh = output_imagines[0]['voxel_1'].shape[1]
                self._add(a, 1, label[:, rf:rf + fh], [im['voxel_1'] for im in output_imagines])
                a['samples'] = len(output_imagines)

    @staticmethod
    def summarise(table, counts, ssc, sums, samples=0):
        """table (2, B, 3), counts (2, 4), ssc (2, 3 + 3 C), sums (2, 6) as nested lists of the integers the kernel leaves (group 0: the
        reconstruction, group 1: the imagined ensemble) -> the figures of one loader without its prefix; a figure whose denominator is
        0 is 0.0.  The IoU is the trainer's: tp / (tp + fp + fn + 1e-5) in float32, the mean over the classes 1.. (SSCMetrics)."""
        def ratio(a, b):
            return float(a) / float(b) if b else 0.0
        out = {}
        for which, tail in ((0, ''), (1, '_imagine')):
            c = dict(zip(COUNT_NAMES, (int(v) for v in counts[which])))
            s = dict(zip(SUM_NAMES, (int(v) / FIX for v in sums[which])))
            n, wrong = c['voxels'], c['voxels'] - c['correct']
            rows = [(int(r[0]), int(r[1]), int(r[2]) / FIX) for r in table[which]]
            gaps = [(k, abs(ratio(ok, k) - ratio(conf, k))) for k, ok, conf in rows if k]
            per = np.asarray(ssc[which][3:], dtype=np.int64).reshape(-1, 3)
            iou = per[:, 0].astype(np.float32) / (per.sum(1).astype(np.float32) + np.float32(1e-5))
            figures = {
                'ece': sum(ratio(k, n) * g for k, g in gaps), 'mce': max((g for _, g in gaps), default=0.0),
                'brier': ratio(s['brier'], n), 'nll': ratio(s['nll'], n), 'accuracy': ratio(c['correct'], n),
                'ens_miou': float(iou[1:].mean(dtype=np.float32)) if len(iou) > 1 else 0.0, 'ens_iou': [float(v) for v in iou],
                'entropy_correct': ratio(s['entropy_correct'], c['correct']), 'entropy_wrong': ratio(s['entropy_wrong'], wrong),
                'mi_correct': ratio(s['mi_correct'], c['correct']), 'mi_wrong': ratio(s['mi_wrong'], wrong),
                'reliability': [[k, ratio(ok, k), ratio(conf, k)] for k, ok, conf in rows],
                'voxels': n, 'ignored': c['ignored'], 'skipped_nonfinite': c['skipped_nonfinite']}
            out.update({f'voxel_{name}{tail}': v for name, v in figures.items()})
        out['voxel_samples_imagine'] = int(samples)
        return out

    def result(self):
        out = {}
        n_classes = int(self.cfg.VOXEL_SEG.N_CLASSES)
        for idx, a in self.acc.items():
            if a['buffers'] is None:
                lists = dict(table=[[[0] * 3] * self.bins] * 2, counts=[[0] * 4] * 2, ssc=[[0] * (3 + 3 * n_classes)] * 2, sums=[[0] * 6] * 2)
            else:
                lists = {k: v.cpu().tolist() for k, v in a['buffers'].items()}
            out.update({f'{self.prefix}{idx}_{k}': v for k, v in self.summarise(samples=a['samples'], **lists).items()})
        return out

    def write(self, out_dir):
        path = os.path.join(out_dir, 'voxel_calibration.json')
        with open(path, 'w') as fh:
            json.dump(self.result(), fh, indent=1, sort_keys=True)
            fh.write('\n')
        return path


def uncert_strip_rows(n_imagines):
    """Rows of the `_uncert` strip: the reconstruction's entropy; with imagined samples also the ensemble's entropy and, below it,
    its mutual information."""
    return 3 if n_imagines else 1


def uncert_panel(cfg, batch, output, output_imagines):
    """The `_uncert` strip (b, 3, PH, PW) uint8, laid out like `_voxel_top` (tiles of (X + 4) x (Y + 4), pad 2): row 0 the top view of the
    predictive entropy of the reconstructed frames (the imagined steps white); rows 1 and 2 the top views of the predictive entropy
    and of the mutual information of the ensemble of all imagined samples (the receptive steps white).  A pixel is the column's
    maximum, a byte of muvo_voxel_calibration, shown through UNCERT_COLOURS."""
    from muvo_amd import ops
    from muvo_amd import visualise as V
    imagines = list(output_imagines or [])
    if len(imagines) > ops.CALIBRATION_MAX_SAMPLES:
        raise ValueError(f'uncert_panel: {len(imagines)} imagined samples (at most {ops.CALIBRATION_MAX_SAMPLES})')
    label = _voxel_label(cfg, batch)
    pred = output['voxel_1'].detach()
    b, rf = pred.shape[:2]
    X, Y = pred.shape[3:5]
    s = label.shape[1]
    fh = V._lengths(s, rf, imagines, 'voxel_1', '_uncert')
    pal, _ = V._palette(UNCERT_COLOURS, pred.device)
    st = V._Strip(b, [X + 4] * uncert_strip_rows(len(imagines)), Y + 4, s, rf, int((Y + 4) / 4), pred.device)

    def tiles(row, maps, T, t0):
        ops.panel_classes(maps.reshape(-1, X, Y), pal, st.panel, st.place(row, T, t0), 2, V.PAD_BYTE)

    def blank(row, T, t0):
        if T:
            ops.panel_fill(b * T, X, Y, 255, st.panel, st.place(row, T, t0), 2, V.PAD_BYTE)
    if rf:
        tiles(0, ensemble_calibration([pred], label[:, :rf], maps=True)['top_entropy'], rf, 0)
    if imagines:
        got = ensemble_calibration([im['voxel_1'] for im in imagines], label[:, rf:rf + fh], maps=True)
        blank(0, fh, rf)
        for row, name in ((1, 'top_entropy'), (2, 'top_mi')):
            blank(row, rf, 0)
            tiles(row, got[name], fh, rf)
    return st.panel
