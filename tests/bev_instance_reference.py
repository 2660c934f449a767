"""numpy restatement of the BEV instance decode and of the panoptic-quality counts (include/muvo_hip.h: muvo_bev_instance_decode,
muvo_bev_pq_counts).  No torch: nothing here can share a bug with the device path.  The grouping is float32
in the stated order, everything else integers or float64.

Per frame: a centre map c (H, W) float32, offsets o (2, H, W) float32 (channel 0 = centre_y - y, channel 1 = centre_x - x) and either
logits (C, H, W) float32 with a set of thing classes or a foreground mask (H, W).

  foreground  the argmax class is a thing; the argmax starts at class 0, scans upward and replaces on strictly greater (first
              maximum; a NaN never replaces the running maximum)
  peaks       c[p] > T and no in-bounds q of the (2r + 1)^2 window has c[q] > c[p]; plateaus are peaks throughout, a NaN is never
              a peak and never suppresses
  selection   the K highest scores, the lower row-major index among equal scores; numbered 1..n in that order; `capped` when the
              frame had more than K peaks
  grouping    ty = float32(y) + o0, tx = float32(x) + o1, d_k = (ty - cy_k) * (ty - cy_k) + (tx - cx_k) * (tx - cx_k) in float32;
              the id is the k of the smallest finite d_k, the lowest k on a tie, 0 without a finite d_k or off the foreground
  PQ          segments i, j > 0 match iff 3 n_ij > a_i + b_j; TP / FP / FN per frame; IoU sum in float64"""
import numpy as np

COUNT_NAMES = ('frames', 'capped', 'label_segments', 'pred_segments', 'tp', 'fp', 'fn')


def argmax_first(logits):
    """(C, H, W) -> (H, W) int64: upward scan, replaced on strictly greater"""
    logits = np.asarray(logits, np.float32)
    best, arg = logits[0].copy(), np.zeros(logits.shape[1:], np.int64)
    for c in range(1, logits.shape[0]):
        with np.errstate(invalid='ignore'):
            take = logits[c] > best
        best = np.where(take, logits[c], best)
        arg = np.where(take, c, arg)
    return arg


def foreground_of(logits, thing_classes=(3, 4)):
    arg = argmax_first(logits)
    return np.isin(arg, np.asarray(list(thing_classes), np.int64))


def peaks(c, threshold=0.1, radius=1):
    """(H, W) bool"""
    c = np.asarray(c, np.float32)
    H, W = c.shape
    r = int(radius)
    pad = np.full((H + 2 * r, W + 2 * r), np.nan, np.float32)          # out of bounds: a NaN, which never suppresses
    pad[r:r + H, r:r + W] = c
    with np.errstate(invalid='ignore'):
        out = c > np.float32(threshold)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                out &= ~(pad[dy:dy + H, dx:dx + W] > c)
    return out


def select(c, peak, K=100):
    """-> (centres (K, 2) int32 with (-1, -1) past n, n, capped)"""
    c = np.asarray(c, np.float32)
    H, W = c.shape
    idx = np.flatnonzero(peak.reshape(-1))
    score = c.reshape(-1)[idx].astype(np.float64)          # -0.0 == 0.0 in a comparison
    order = np.lexsort((idx, -score))                      # score descending, then index ascending
    kept = idx[order][:K]
    centres = np.full((K, 2), -1, np.int32)
    centres[:len(kept), 0] = kept // W
    centres[:len(kept), 1] = kept % W
    return centres, len(kept), int(len(idx) > K)


def group(offset, foreground, centres, n):
    """(H, W) uint8"""
    offset = np.asarray(offset, np.float32)
    _, H, W = offset.shape
    ids = np.zeros((H, W), np.uint8)
    if n == 0:
        return ids
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    with np.errstate(invalid='ignore', over='ignore'):
        ty = (yy + offset[0]).astype(np.float32)
        tx = (xx + offset[1]).astype(np.float32)
        cy = centres[:n, 0].astype(np.float32)[:, None, None]
        cx = centres[:n, 1].astype(np.float32)[:, None, None]
        dy = (ty[None] - cy).astype(np.float32)
        dx = (tx[None] - cx).astype(np.float32)
        d = ((dy * dy).astype(np.float32) + (dx * dx).astype(np.float32)).astype(np.float32)
    assert d.dtype == np.float32
    finite = np.isfinite(d)
    d = np.where(finite, d, np.float32(np.inf))
    arg = np.argmin(d, axis=0)                             # the first minimum: the lowest k
    ids = np.where(finite.any(axis=0) & np.asarray(foreground, bool), arg + 1, 0).astype(np.uint8)
    return ids


def decode_frame(c, offset, logits=None, foreground=None, threshold=0.1, radius=1, K=100, thing_classes=(3, 4)):
    assert (logits is None) != (foreground is None)
    fg = foreground_of(logits, thing_classes) if logits is not None else np.asarray(foreground) != 0
    centres, n, capped = select(c, peaks(c, threshold, radius), K)
    return group(offset, fg, centres, n), centres, n, capped


def decode(center, offset, logits=None, foreground=None, **kw):
    """frames along axis 0 -> ids (F, H, W) uint8, centres (F, K, 2) int32, n (F,) int32, capped (F,) int32"""
    out = [decode_frame(center[f], offset[f], None if logits is None else logits[f], None if foreground is None else foreground[f], **kw)
           for f in range(len(center))]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.asarray([o[2] for o in out], np.int32),
            np.asarray([o[3] for o in out], np.int32))


def pq_frame(label, pred):
    """-> (label segments, predicted segments, tp, fp, fn, IoU sum as float64) of one frame"""
    g, q = np.asarray(label).astype(np.int64).reshape(-1), np.asarray(pred).astype(np.int64).reshape(-1)
    assert g.min() >= 0 and g.max() <= 255 and q.min() >= 0 and q.max() <= 255
    table = np.bincount(g * 256 + q, minlength=65536).reshape(256, 256)
    a, b = table.sum(1), table.sum(0)
    tp, iou = 0, np.float64(0.0)
    for i, j in zip(*np.nonzero(table)):                   # the order of the device sum does not matter within 1e-12
        n = int(table[i, j])
        if i > 0 and j > 0 and 3 * n > int(a[i]) + int(b[j]):
            tp += 1
            iou += np.float64(n) / np.float64(int(a[i]) + int(b[j]) - n)
    nl, npred = int((a[1:] > 0).sum()), int((b[1:] > 0).sum())
    return nl, npred, tp, npred - tp, nl - tp, float(iou)


def pq_counts(label, pred, capped=None):
    """frames along axis 0 -> (counts (7,) int64 in the order of COUNT_NAMES, IoU sum float64)"""
    counts, total = np.zeros(7, np.int64), np.float64(0.0)
    for f in range(len(label)):
        nl, npred, tp, fp, fn, iou = pq_frame(label[f], pred[f])
        counts += np.asarray([1, int(capped[f] != 0) if capped is not None else 0, nl, npred, tp, fp, fn], np.int64)
        total += iou
    return counts, float(total)


def pq_summary(counts, iou_sum):
    """PQ = iou_sum / (tp + fp / 2 + fn / 2), SQ = iou_sum / tp, RQ = tp / (tp + fp / 2 + fn / 2); 0.0 on a zero denominator"""
    tp, fp, fn = int(counts[4]), int(counts[5]), int(counts[6])
    den = tp + 0.5 * fp + 0.5 * fn
    return {'pq': float(iou_sum) / den if den else 0.0, 'sq': float(iou_sum) / tp if tp else 0.0, 'rq': tp / den if den else 0.0}
