"""-m gpu: the BEV instance decode and the panoptic-quality counts (csrc/bev_instance.hip through ops.bev_instance_decode and
ops.bev_pq_counts) against the numpy restatement tests/bev_instance_reference.py.  ids, centres, n, the capped flags and the
integer counts are compared with ==; the fp64 IoU sum within 1e-12 relative (at most a few thousand fp64 terms added in another
order: about 2e-13).  Every call has F = 3 frames, at 192 x 192 and at 37 x 53 (no multiple of a tile or a wave), and its last
frame is all-background."""
import numpy as np
import pytest
import torch

import bev_instance_reference as R

pytestmark = pytest.mark.gpu
SIZES = [(192, 192), (37, 53)]
T = 0.1


def _dev(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(dev, c, o, logits=None, fg=None, **kw):
    """device decode == reference decode; returns the reference's outputs"""
    from muvo_amd import ops
    want = R.decode(c, o, logits, fg, threshold=kw.get('threshold', T), radius=kw.get('radius', 1), K=kw.get('max_centres', 100),
                    thing_classes=kw.get('thing_classes', (3, 4)))
    got = ops.bev_instance_decode(_dev(dev, c), _dev(dev, o), _dev(dev, logits), _dev(dev, fg), **{'threshold': T, **kw})
    got = [g.cpu().numpy() for g in got]
    for name, g, w in zip(('ids', 'centres', 'n', 'capped'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])
    return want


def _blob_offsets(H, W, centres):
    """offsets that point every pixel at its nearest listed centre (the label convention: centre - pixel)"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = [(yy - cy) ** 2 + (xx - cx) ** 2 for cy, cx in centres]
    k = np.argmin(np.stack(d), 0)
    cy, cx = np.asarray(centres)[:, 0][k], np.asarray(centres)[:, 1][k]
    return np.stack([cy - yy, cx - xx]).astype(np.float32)


def _thing_logits(fg, rng, C=8):
    """logits (C, H, W) whose argmax is class 3 or 4 exactly on fg"""
    H, W = fg.shape
    logits = rng.normal(size=(C, H, W)).astype(np.float32)
    top = np.where(fg, rng.integers(3, 5, (H, W)), rng.choice([k for k in range(C) if k not in (3, 4)], (H, W)))
    np.put_along_axis(logits, top[None], 9.0, 0)
    return logits


# ------------------------------------------------------------------------------------------------ peaks
@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('radius', [1, 3])
def test_peaks_plateau_corners_edges_threshold_nan(dev, H, W, radius):
    c = np.zeros((3, H, W), np.float32)
    a = c[0]
    a[10:12, 20:22] = 0.5                                        # a 2 x 2 plateau
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):  # the corners
        a[y, x] = 0.9
    for y, x in ((0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):   # the edges
        a[y, x] = 0.8
    a[20, 10] = np.float32(T)                                    # exactly the threshold
    a[25, 25], a[25, 26] = 0.7, np.nan                           # a NaN next to a peak
    a[30, 30], a[30, 31] = np.nan, np.nan
    a[5, 40], a[5, 41] = 0.3, 0.6                                # the lower neighbour is suppressed at every radius
    c[2] = a                                                     # frame 2: the same peaks, no foreground
    o = np.zeros((3, 2, H, W), np.float32)
    fg = np.ones((3, H, W), np.uint8)
    fg[2] = 0
    ids, centres, n, capped = _check(dev, c, o, fg=fg, radius=radius)
    assert n.tolist() == [14, 0, 14] and capped.tolist() == [0, 0, 0]           # frame 1: no peak at all
    kept = {tuple(v) for v in centres[0, :14].tolist()}
    assert {(10, 20), (10, 21), (11, 20), (11, 21), (0, 0), (H - 1, W - 1), (H // 2, 0), (25, 25), (5, 41)} <= kept
    assert (20, 10) not in kept and (25, 26) not in kept and (5, 40) not in kept
    assert centres[0, 0].tolist() == [0, 0] and centres[0, 3].tolist() == [H - 1, W - 1]      # 0.9 four times: by index
    assert ids[0].min() >= 1 and not ids[1].any() and not ids[2].any()          # foreground without a centre; background with centres


@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('K', [100, 7])
def test_quantised_noise_cut_ties_and_offsets_logits_and_mask(dev, H, W, K):
    """far more than K peaks in steps of 1/64, so scores tie across the cut; random offsets of several cells, some targets outside the
    image; a partial foreground once as logits (with an exact tie of the two thing logits and a NaN logit) and once as a mask"""
    rng = np.random.default_rng(H * 1000 + K)
    c = (np.floor(rng.random((3, H, W)) * 64) / 64).astype(np.float32)
    o = (rng.normal(size=(3, 2, H, W)) * 6).astype(np.float32)
    o[0, :, :3] += 40.0                                          # far outside
    o[1, :, :, :2] -= 40.0
    fg = rng.random((3, H, W)) < 0.4
    fg[2] = False
    logits = np.stack([_thing_logits(fg[f], rng) for f in range(3)])
    y, x = np.argwhere(fg[0])[0]
    logits[0, 3, y, x] = logits[0, 4, y, x] = 9.0                # an exact tie of the thing classes: still foreground
    y, x = np.argwhere(fg[0])[1]
    logits[0, 5, y, x] = np.nan                                  # never replaces the maximum
    y, x = np.argwhere(~fg[1])[0]
    logits[1, 4, y, x] = np.nan                                  # a NaN thing logit: still background
    assert np.array_equal(np.stack([R.foreground_of(l) for l in logits]), fg)
    ids, centres, n, capped = _check(dev, c, o, logits=logits, max_centres=K)
    assert n.tolist() == [K, K, K] and capped.tolist() == [1, 1, 1]
    flat = c[0].reshape(-1)[centres[0, :, 0] * W + centres[0, :, 1]]
    assert (np.diff(flat) <= 0).all() and len(np.unique(flat)) < K            # ties inside the kept set
    assert len(np.unique(ids[0])) > min(K, 5) and not ids[2].any()
    ids2 = _check(dev, c, o, fg=fg.astype(np.uint8) * 255, max_centres=K)[0]
    assert np.array_equal(ids2, ids)


@pytest.mark.parametrize('H,W', SIZES)
def test_grouping_equidistant_infinite_offset_and_other_thing_classes(dev, H, W):
    rng = np.random.default_rng(3)
    c = np.zeros((3, H, W), np.float32)
    c[0, 10, 10], c[0, 10, 16], c[0, 30, 40] = 0.9, 0.8, 0.7
    c[1, 5, 5] = 0.5
    c[2, 7, 7] = 0.5
    o = np.zeros((3, 2, H, W), np.float32)
    o[1] = _blob_offsets(H, W, [(5, 5)])
    o[0, 0, 12, 12] = np.inf                                     # d_k = inf for every k: id 0
    o[0, 1, 13, 13] = -np.inf
    o[0, 0, 14, 14] = np.nan
    fg = np.ones((3, H, W), bool)
    fg[2] = False
    logits = np.stack([_thing_logits(fg[f], rng, C=5) for f in range(3)])
    ids, centres, n, _ = _check(dev, c, o, logits=logits)
    assert n.tolist() == [3, 1, 1] and centres[0, :3].tolist() == [[10, 10], [10, 16], [30, 40]]
    assert ids[0, 10, 13] == 1 and ids[0, 2, 13] == 1            # equidistant from centres 1 and 2 at zero offset: the lower id
    assert ids[0, 10, 12] == 1 and ids[0, 10, 14] == 2
    assert ids[0, 12, 12] == 0 and ids[0, 13, 13] == 0 and ids[0, 14, 14] == 0 and ids[0, 12, 13] == 1
    assert (ids[1] == 1).all() and not ids[2].any()
    # another thing set, two classes at the limits of the mask: class 0 and class 31 of 32
    wide = rng.normal(size=(3, 32, H, W)).astype(np.float32)
    wide[2, 1] = 50.0
    got = _check(dev, c, o, logits=wide, thing_classes=(0, 31))[0]
    assert got[0].any() and (got[0] == 0).any() and not got[2].any()


@pytest.mark.parametrize('H,W', SIZES)
def test_negative_threshold_signed_zeros_tie_by_index(dev, H, W):
    """T = -0.5: scores of +0 and -0 are peaks and are EQUAL scores, so the row-major index alone orders them, whatever their sign bits"""
    c = np.full((3, H, W), -1.0, np.float32)
    spots = [(2, 3), (2, 30), (9, 9), (20, 5), (33, 50), (36, 1)]
    for k, (y, x) in enumerate(spots):
        c[0, y, x] = -0.0 if k % 2 == 0 else 0.0                 # -0 first in index order: bit order would put every +0 before it
    c[0, 15, 15], c[0, 15, 40] = 0.25, -0.25                     # one above the zeros, one below them
    c[1, 4, 4], c[1, 4, 20] = 0.0, -0.0
    c[2] = c[0]
    assert np.signbit(c[0, 2, 3]) and not np.signbit(c[0, 2, 30])
    o = np.zeros((3, 2, H, W), np.float32)
    fg = np.ones((3, H, W), np.uint8)
    fg[2] = 0
    for K in (100, 4):                                           # K = 4 cuts inside the run of zeros
        ids, centres, n, capped = _check(dev, c, o, fg=fg, threshold=-0.5, max_centres=K)
        order = [(15, 15)] + spots + [(15, 40)]
        assert centres[0, :min(K, 8)].tolist() == [list(v) for v in order[:K]] and n.tolist() == [min(K, 8), 2, min(K, 8)]
        assert centres[1, :2].tolist() == [[4, 4], [4, 20]] and capped.tolist() == [int(K < 8), 0, int(K < 8)]
        assert ids[0].min() >= 1 and not ids[2].any()


# ------------------------------------------------------------------------------------------------ panoptic quality
def _pq_maps(H, W, rng):
    """label ids with gaps (255 among them), predicted ids up to 254; frame 1 has no label segment, frame 2 nothing at all (the frame
    with label segments and no predicted segment is in the second call of the test)"""
    label, pred = np.zeros((3, H, W), np.uint8), np.zeros((3, H, W), np.uint8)
    label[0, 0, 0:4], pred[0, 0, 0:2] = 4, 209                   # IoU exactly 1/2: no match
    label[0, 2, 0:5], pred[0, 2, 0:3] = 255, 254                 # 3 / 5: a match
    label[0, 5:15, 5:20], pred[0, 6:15, 5:22] = 17, 100          # a match
    label[0, 20:30, 0:10] = 200                                  # no prediction on it
    pred[0, 20:25, 30:40] = 201                                  # no label under it
    blocks = rng.integers(1, 60, (H // 4 + 1, W // 4 + 1)).astype(np.uint8)
    noise = np.kron(blocks, np.ones((4, 4), np.uint8))[:H, :W]
    label[0, 32:], pred[0, 32:] = noise[32:] * 3, np.where(rng.random((H - 32, W)) < 0.7, noise[32:], 0)
    pred[1] = noise                                              # predictions, no label
    return label, pred                                           # (the noise: label ids 3..177 in threes, predicted ids 1..59)


@pytest.mark.parametrize('H,W', SIZES)
def test_pq_counts_accumulate_over_two_calls(dev, H, W):
    from muvo_amd import ops
    rng = np.random.default_rng(H)
    label, pred = _pq_maps(H, W, rng)
    first = R.pq_frame(label[0], pred[0])
    assert first[2] >= 3 and first[3] >= 2 and first[4] >= 2     # matches, unmatched predictions, unmatched labels
    assert R.pq_frame(label[0, :4], pred[0, :4]) == (2, 2, 1, 1, 1, 0.6)        # the 1/2 pair and the 3/5 pair alone
    assert R.pq_frame(label[1], pred[1])[:3] == (0, len(np.unique(pred[1])), 0) and R.pq_frame(label[2], pred[2])[:2] == (0, 0)
    label2 = label.copy()                                        # second call: frame 0 has one match, every other label segment unmatched;
    label2[1] = label[0]                                         # frame 1 has label segments and no predicted segment: all of them FN,
    pred2 = np.where(label2 == 200, 7, 0).astype(np.uint8)       # FP 0; frame 2 has neither
    pred2[1] = 0
    nl = len(np.unique(label2[1])) - 1
    assert nl > 10 and R.pq_frame(label2[1], pred2[1]) == (nl, 0, 0, 0, nl, 0.0) and R.pq_frame(label2[2], pred2[2]) == (0, 0, 0, 0, 0, 0.0)
    capped = np.asarray([1, 0, 1], np.int32)
    counts, total = torch.zeros(7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    ops.bev_pq_counts(_dev(dev, label), _dev(dev, pred), counts, total, _dev(dev, capped))
    w1, t1 = R.pq_counts(label, pred, capped)
    assert counts.cpu().numpy().tolist() == w1.tolist()
    assert abs(float(total[0]) - t1) <= 1e-12 * t1 and t1 > 0
    ops.bev_pq_counts(_dev(dev, label2), _dev(dev, pred2), counts, total)
    w2, t2 = R.pq_counts(label2, pred2)
    assert w2[4] == 1 and w2[6] > 0 and w2[1] == 0
    print('counts', counts.cpu().numpy().tolist(), (w1 + w2).tolist(), 'iou', float(total[0]), t1 + t2)
    assert counts.cpu().numpy().tolist() == (w1 + w2).tolist()
    assert abs(float(total[0]) - (t1 + t2)) <= 1e-12 * (t1 + t2)
    alone, total2 = torch.zeros(7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    ops.bev_pq_counts(_dev(dev, label2[1:]), _dev(dev, pred2[1:]), alone, total2)       # the label-only frame and the empty frame by themselves
    assert alone.cpu().numpy().tolist() == R.pq_counts(label2[1:], pred2[1:])[0].tolist() == [2, 0, nl, 0, 0, 0, nl] and float(total2[0]) == 0.0


@pytest.mark.parametrize('H,W', SIZES)
def test_decode_then_count_through_the_public_entry(dev, H, W):
    """decode_instances over (b, s, ...) tensors, its ids counted against a label: the whole path against the reference"""
    from muvo_amd import ops
    from muvo_amd.bev_instances import decode_instances
    rng = np.random.default_rng(W)
    b, s = 1, 3
    spots = [(8, 9), (20, 30), (30, 12)]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    heat = np.max([np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8.0) for cy, cx in spots], 0).astype(np.float32)
    c = np.stack([heat, heat, heat])
    o = np.stack([_blob_offsets(H, W, spots)] * 3) + rng.normal(size=(3, 2, H, W)).astype(np.float32) * 0.3
    near = np.min([(yy - cy) ** 2 + (xx - cx) ** 2 for cy, cx in spots], 0) <= 16
    fg = np.stack([near, near, np.zeros_like(near)])
    label = np.zeros((3, H, W), np.uint8)
    for k, (cy, cx) in enumerate(spots):
        label[:2][:, (yy - cy) ** 2 + (xx - cx) ** 2 <= 16] = 50 * (k + 1)
    logits = np.stack([_thing_logits(fg[f], rng) for f in range(3)])
    ids, centres, n, capped = decode_instances(_dev(dev, c).view(b, s, 1, H, W), _dev(dev, o).view(b, s, 2, H, W), _dev(dev, logits).view(b, s, 8, H, W))
    assert ids.shape == (b, s, H, W) and centres.shape == (b, s, 100, 2) and n.shape == (b, s) and capped.shape == (b, s)
    want = R.decode(c, o, logits, threshold=T, radius=1, K=100)
    assert np.array_equal(ids.cpu().numpy()[0], want[0]) and np.array_equal(centres.cpu().numpy()[0], want[1])
    assert n.cpu().numpy().tolist() == [[3, 3, 3]] and centres[0, 0, :3].cpu().numpy().tolist() == [list(v) for v in spots]
    counts, total = torch.zeros(7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    ops.bev_pq_counts(_dev(dev, label), ids.reshape(-1, H, W), counts, total, capped.reshape(-1))
    wc, wt = R.pq_counts(label, want[0], want[3])
    assert counts.cpu().numpy().tolist() == wc.tolist() == [3, 0, 6, 6, 6, 0, 0]
    assert abs(float(total[0]) - wt) <= 1e-12 * wt and wt > 5.0
