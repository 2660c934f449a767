"""Instances from the bird's-eye-view centre / offset heads, their panoptic quality and the `_inst` panel (DESIGN.md section 16;
the definitions: include/muvo_hip.h, muvo_bev_instance_decode and muvo_bev_pq_counts).  An extension: the reference trains the two
heads (`bev_instance_center_{f}`, `bev_instance_offset_{f}`) and never reads them.  Everything runs on the device over whole
batches of frames (csrc/bev_instance.hip); nothing crosses to the host before `PanopticQualityMetric.result()`.

    decode_instances        centre map + offsets + segmentation logits (or a foreground mask) -> ids, centres, counts
    PanopticQualityMetric   `predict --mode test --bev-pq` -> OUT/bev_pq.json
    inst_panel              the `_inst` strip (`predict --panels N --inst`, `train --panel-dir DIR --inst`), laid out like `_bev`"""
import json
import os

import torch

THING_CLASSES = (3, 4)            # Vehicle, Pedestrian: the two planes the label's instance mask is built from
COUNT_NAMES = ('pq_frames', 'pq_capped', 'label_segments', 'pred_segments', 'tp', 'fp', 'fn')      # the order of ops.bev_pq_counts
# id 0 is white; id k in 1..255 is a closed form whose three factors are odd, so the 255 colours are distinct
INSTANCE_COLOURS = ((255, 255, 255),) + tuple(((67 * k + 29) % 256, (149 * k + 101) % 256, (211 * k + 173) % 256) for k in range(1, 256))


def _frames(x, tail):
    """(b, s, ...) or (F, ...) with `tail` trailing axes -> (frames, lead shape)"""
    lead = tuple(x.shape[:x.dim() - tail])
    if len(lead) not in (1, 2):
        raise ValueError(f'decode_instances: (b, s, ...) or (F, ...) tensors, got {tuple(x.shape)}')
    return x.reshape(-1, *x.shape[x.dim() - tail:]), lead


def decode_instances(center, offset, segmentation=None, foreground=None, threshold=0.1, radius=1, max_centres=100, thing_classes=THING_CLASSES):
    """center (b, s, 1, H, W) / (b, s, H, W) / (F, 1, H, W) / (F, H, W) fp32, offset (..., 2, H, W) fp32 and either the segmentation
    logits (..., C, H, W) fp32 or a foreground mask (..., H, W) / (..., 1, H, W) uint8 or bool -> (ids (..., H, W) uint8, centres
    (..., K, 2) int32 (y, x; (-1, -1) past the count), n (...) int32, capped (...) int32), the leading axes those of `offset`."""
    from muvo_amd import ops
    off, lead = _frames(offset.detach(), 3)
    H, W = off.shape[-2:]
    F = off.shape[0]
    c = center.detach().reshape(F, H, W)
    seg = fg = None
    if segmentation is not None:
        seg, _ = _frames(segmentation.detach(), 3)
    if foreground is not None:
        fg = foreground.detach().reshape(F, H, W)
        fg = fg if fg.dtype == torch.uint8 else (fg != 0).to(torch.uint8)
    ids, centres, n, capped = ops.bev_instance_decode(c.float(), off.float(), None if seg is None else seg.float(), fg, threshold, radius, max_centres,
                                                      thing_classes)
    return ids.reshape(*lead, H, W), centres.reshape(*lead, *centres.shape[1:]), n.reshape(lead), capped.reshape(lead)


def _decode_output(output, options):
    return decode_instances(output['bev_instance_center_1'], output['bev_instance_offset_1'], output['bev_segmentation_1'], **options)


class PanopticQualityMetric:
    """`predict --mode test --bev-pq`: per loader the panoptic quality PQ = SQ x RQ of the instances decoded from the reconstructed
    frames against `instance_label_1[:, :rf]` and, apart from them, of the frames of the first imagined sample against
    `instance_label_1[:, rf:]`.  `update` is the per-batch hook of predict.run and only queues kernels (int64 counts and the fp64
    IoU sum stay on the device); `result()` reads them once per loader.  options: threshold, radius, max_centres, thing_classes of
    `decode_instances`."""

    def __init__(self, cfg, prefix='test', **options):
        self.cfg, self.prefix, self.options = cfg, prefix, dict(options)
        self.loader = None
        self.acc = {}

    def start_loader(self, idx):
        self.loader = str(idx)
        self.acc[self.loader] = dict(counts=None, sums=None)

    def _add(self, a, which, label, output):
        from muvo_amd import ops
        if not label.shape[0] * label.shape[1]:
            return
        ids, _, _, capped = _decode_output(output, self.options)
        if a['counts'] is None:
            a['counts'] = torch.zeros((2, 7), dtype=torch.int64, device=ids.device)
            a['sums'] = torch.zeros((2, 1), dtype=torch.float64, device=ids.device)
        H, W = ids.shape[-2:]
        ops.bev_pq_counts(label.to(torch.uint8).reshape(-1, H, W), ids.reshape(-1, H, W), a['counts'][which], a['sums'][which], capped.reshape(-1))

    def update(self, i, batch, output, output_imagines):
        if self.loader is None:
            self.start_loader(0)
        a = self.acc[self.loader]
        label = batch['instance_label_1']
        rf = output['bev_instance_center_1'].shape[1]
        with torch.no_grad():
            self._add(a, 0, label[:, :rf], output)
            if output_imagines:
                fh = output_imagines[0]['bev_instance_center_1'].shape[1]
                self._add(a, 1, label[:, rf:rf + fh], output_imagines[0])

    @staticmethod
    def summarise(counts, sums):
        """counts (2, 7) in the order of COUNT_NAMES and sums (2, 1) as nested lists -> the figures of one loader without its prefix; a
        figure whose denominator is 0 is 0.0"""
        def ratio(a, b):
            return a / b if b else 0.0
        out = {}
        for which, tail in ((0, ''), (1, '_imagine')):
            c = dict(zip(COUNT_NAMES, (int(v) for v in counts[which])))
            den = c['tp'] + 0.5 * c['fp'] + 0.5 * c['fn']
            iou = float(sums[which][0])
            out[f'bev_pq{tail}'], out[f'bev_sq{tail}'], out[f'bev_rq{tail}'] = ratio(iou, den), ratio(iou, c['tp']), ratio(c['tp'], den)
            for name, v in c.items():
                out[f'bev_{name}{tail}'] = v
        return out

    def result(self):
        out = {}
        for idx, a in self.acc.items():
            if a['counts'] is None:
                counts, sums = [[0] * 7] * 2, [[0.0]] * 2
            else:
                counts, sums = a['counts'].cpu().tolist(), a['sums'].cpu().tolist()
            out.update({f'{self.prefix}{idx}_{k}': v for k, v in self.summarise(counts, sums).items()})
        return out

    def write(self, out_dir):
        path = os.path.join(out_dir, 'bev_pq.json')
        with open(path, 'w') as fh:
            json.dump(self.result(), fh, indent=1, sort_keys=True)
            fh.write('\n')
        return path


def inst_panel(cfg, batch, output, output_imagines, **options):
    """The `_inst` strip (b, 3, PH, PW) uint8: `visualise._class_strip` as `_bev` calls it (label row, reconstruction row, one row per
    imagined sample; tiles rotated, pad 2) over `instance_label_1` and the decoded ids, through the 256-entry instance palette."""
    from muvo_amd import visualise as V
    key = 'bev_instance_center_1'
    label = batch['instance_label_1'].to(torch.uint8)
    ids = _decode_output(output, options)[0]
    imagines = [{key: _decode_output(im, options)[0]} for im in (output_imagines or [])]
    return V._class_strip(label, ids, imagines, key, INSTANCE_COLOURS, 2, label.shape[1], output[key].shape[1], rotate=True)
