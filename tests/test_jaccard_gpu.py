"""-m gpu: the confusion-matrix kernel of the segmentation IoU (csrc/metrics.hip, muvo_seg_confusion) and JaccardIndex on top of
it.  The oracle is built here: torch.argmax on the CPU, np.bincount over the in-range labels, a separate count of the others.
Counts must be equal, not close.  Logits come from a nine-value grid (multiples of 0.25 in [-1, 1]) so ties are common and the
first-maximum rule is exercised everywhere."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# The launch covers at most SEG_MAX_BLOCKS (512) blocks x SEG_THREADS (256) lanes x 4 pixels per lane on the 16-byte path and
# x 1 pixel per lane on the scalar path (csrc/metrics.hip): beyond that the grid-stride loop runs more than once.
STRIDE_CAP_VECTOR = 512 * 256 * 4
STRIDE_CAP_SCALAR = 512 * 256


def _grid_logits(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).float() * 0.25


def _labels(shape, c, seed, extra=()):
    """uint8 labels in [0, c), with the values of `extra` sprinkled in (about 1 in 16 each)."""
    g = torch.Generator().manual_seed(seed + 1000)
    lb = torch.randint(0, c, shape, generator=g, dtype=torch.int64)
    for k, v in enumerate(extra):
        lb[torch.randint(0, 16, shape, generator=g) == k] = v
    return lb


def _oracle(pred_idx, label, c):
    """pred_idx, label: integer CPU tensors with as many elements -> (C*C counts, out-of-range count)."""
    p = pred_idx.reshape(-1).numpy().astype(np.int64)
    t = label.reshape(-1).numpy().astype(np.int64)
    ok = (t >= 0) & (t < c)
    return np.bincount(t[ok] * c + p[ok], minlength=c * c), int((~ok).sum())


def _one_hot_logits(pred, c):
    """Logits whose argmax is `pred` (N, H, W), with a unique maximum."""
    return torch.nn.functional.one_hot(pred, c).permute(0, 3, 1, 2).float().contiguous()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(logits (F, C, H, W) float32, label int64 (F, H, W)) on the CPU, built once per name."""
    if name == 'odd':                   # P = 35: scalar path, frames cross inside a block
        return _grid_logits((3, 8, 5, 7), 1), _labels((3, 5, 7), 8, 1)
    if name == 'one_pixel':
        return _grid_logits((1, 2, 1, 1), 2), _labels((1, 1, 1), 2, 2)
    if name == 'lidar':                 # 16-byte path at the lidar head's own size
        return _grid_logits((2, 9, 64, 1024), 3), _labels((2, 64, 1024), 9, 3)
    if name == 'distinct':
        # pixel i sits in lane i // 4 as its pixel i % 4 (16-byte path); bin = i % 256 gives the 64 lanes of a wave 64 different
        # bins for each of their four pixels: the merge loop runs its 64 rounds
        i = torch.arange(3 * 4 * 36)
        b = i % 256
        return _one_hot_logits((b % 16).view(3, 4, 36), 16), (b // 16).view(3, 4, 36)
    if name == 'constant':              # every lane the same bin
        return _one_hot_logits(torch.full((2, 192, 192), 5), 8), torch.full((2, 192, 192), 3)
    if name == 'stride_vector':
        shape = (1, 512, 1028)
        assert shape[1] * shape[2] > STRIDE_CAP_VECTOR and (shape[1] * shape[2]) % 4 == 0
        return _grid_logits((1, 2, *shape[1:]), 4), _labels(shape, 2, 4, extra=(2, 255))
    if name == 'stride_scalar':
        shape = (1, 363, 365)
        assert shape[1] * shape[2] > STRIDE_CAP_SCALAR and (shape[1] * shape[2]) % 4 != 0
        return _grid_logits((1, 2, *shape[1:]), 5), _labels(shape, 2, 5, extra=(2, 255))
    raise KeyError(name)


@pytest.mark.parametrize('name', ['odd', 'one_pixel', 'lidar', 'distinct', 'constant', 'stride_vector', 'stride_scalar'])
def test_counts_equal_argmax_and_bincount(dev, name):
    from muvo_amd.metrics import seg_confusion
    logits, label = _case(name)
    c = logits.shape[1]
    want, want_out = _oracle(torch.argmax(logits, dim=1), label, c)
    got = seg_confusion(logits.to(dev), label.to(torch.uint8).to(dev), c)
    assert got.dtype == torch.int64 and got.shape == (c * c + 1,) and got.is_cuda
    got = got.cpu().numpy()
    assert int(got.sum()) == label.numel()
    assert np.array_equal(got[:-1], want), np.argwhere(got[:-1] != want)[:8]
    assert int(got[-1]) == want_out
    if name == 'distinct':
        assert (want > 0).sum() == 256 and want.max() == 2        # all 256 bins are hit
    if name == 'constant':
        assert want[3 * 8 + 5] == 2 * 192 * 192
    if name.startswith('stride'):
        assert want_out > 0
    # the integer-prediction path on the same data
    got_idx = seg_confusion(torch.argmax(logits, dim=1).to(dev), label.to(dev), c).cpu().numpy()
    assert np.array_equal(got_idx, got)


def test_unaligned_bases_take_the_scalar_path(dev):
    """P % 4 == 0 but the logits start 4 bytes and the labels 1 byte past an aligned address: no 16-byte loads there."""
    logits, label = _case('lidar')
    c = logits.shape[1]
    from muvo_amd.metrics import seg_confusion
    buf = torch.empty(logits.numel() + 1, device=dev)
    lbuf = torch.empty(label.numel() + 1, dtype=torch.uint8, device=dev)
    lg, lb = buf[1:].view(logits.shape), lbuf[1:].view(label.shape)
    lg.copy_(logits)
    lb.copy_(label)
    assert lg.is_contiguous() and lg.data_ptr() % 16 == 4 and lb.data_ptr() % 4 == 1
    want, want_out = _oracle(torch.argmax(logits, dim=1), label, c)
    got = seg_confusion(lg, lb, c).cpu().numpy()
    assert np.array_equal(got[:-1], want) and int(got[-1]) == want_out == 0


def test_out_of_range_labels(dev):
    from muvo_amd.metrics import seg_confusion
    c = 9
    logits = _grid_logits((2, c, 6, 10), 7)
    pred = torch.argmax(logits, dim=1)
    # bytes holding 255 and C itself
    label = _labels((2, 6, 10), c, 7, extra=(255, c))
    assert (label == 255).any() and (label == c).any()
    want, want_out = _oracle(pred, label, c)
    got = seg_confusion(logits.to(dev), label.to(torch.uint8).to(dev), c).cpu().numpy()
    assert np.array_equal(got[:-1], want) and int(got[-1]) == want_out == int((label >= c).sum())
    # int64 labels holding -1, 256 and 300 (a byte cast would turn 256 into class 0 and 300 into 44): exact count, no other bin
    label = _labels((2, 6, 10), c, 8, extra=(-1, 256, 300))
    n_bad = int(((label < 0) | (label >= c)).sum())
    assert n_bad >= 3 and (label == 256).any()
    want, want_out = _oracle(pred, label, c)
    assert want_out == n_bad
    for lb in (label, label.unsqueeze(1), label.to(torch.int32), label.to(torch.int16)):      # with a singleton channel too
        got = seg_confusion(logits.to(dev), lb.to(dev), c).cpu().numpy()
        assert np.array_equal(got[:-1], want) and int(got[-1]) == n_bad
    # only out-of-range labels: nothing but the last bin moves
    got = seg_confusion(logits.to(dev), torch.full((2, 6, 10), -1).to(dev), c).cpu().numpy()
    assert got[:-1].sum() == 0 and int(got[-1]) == 120


def test_bad_arguments(dev):
    from muvo_amd.metrics import seg_confusion
    lg = torch.zeros(1, 17, 2, 2, device=dev)
    with pytest.raises(ValueError):
        seg_confusion(lg, torch.zeros(1, 2, 2, dtype=torch.uint8, device=dev), 17)
    with pytest.raises(ValueError):
        seg_confusion(lg[:, :8], torch.zeros(1, 2, 3, dtype=torch.uint8, device=dev), 8)
    with pytest.raises(ValueError):
        seg_confusion(lg[:, :8], torch.zeros(1, 2, 2, dtype=torch.uint8, device=dev), 9)


def test_jaccard_index_update_reset_compute(dev):
    from muvo_amd.metrics import JaccardIndex, jaccard_from_confmat
    c = 8
    logits, label = _case('odd')
    lg2, lb2 = _grid_logits((2, c, 4, 12), 11), _labels((2, 4, 12), c, 11)
    w1, _ = _oracle(torch.argmax(logits, dim=1), label, c)
    w2, _ = _oracle(torch.argmax(lg2, dim=1), lb2, c)
    m = JaccardIndex(task='multiclass', num_classes=c, average='none')
    assert m.confmat.shape == (c, c) and m.confmat.dtype == torch.int64 and m.confmat.is_cuda and int(m.out_of_range) == 0
    m.update(logits.to(dev), label.to(dev))
    assert np.array_equal(m.confmat.cpu().numpy().reshape(-1), w1)
    m(lg2.to(dev), lb2.unsqueeze(1).to(torch.uint8).to(dev))                 # two updates add; __call__ is update
    assert np.array_equal(m.confmat.cpu().numpy().reshape(-1), w1 + w2) and int(m.out_of_range) == 0
    scores = m.compute()
    assert scores.dtype == torch.float32 and scores.shape == (c,)
    want = jaccard_from_confmat(torch.from_numpy((w1 + w2).reshape(c, c)))
    w = (w1 + w2).reshape(c, c).astype(np.float64)
    den = w.sum(0) + w.sum(1) - np.diag(w)
    assert (den > 0).all()
    want64 = np.diag(w) / den
    np.testing.assert_allclose(scores.cpu().numpy(), want.numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(scores.cpu().numpy().astype(np.float64), want64, rtol=1e-6, atol=0)
    m.reset()
    assert int(m.confmat.sum()) == 0 and int(m.out_of_range) == 0
    assert m.compute().tolist() == [0.0] * c
    # out-of-range labels: compute() raises with their count, or leaves them out
    bad = label.clone()
    bad[0, 0, :3] = 200
    wb, nb = _oracle(torch.argmax(logits, dim=1), bad, c)
    assert nb == 3
    m.update(logits.to(dev), bad.to(dev))
    assert int(m.out_of_range) == 3
    with pytest.raises(RuntimeError, match='3 pixels'):
        m.compute()
    loose = JaccardIndex(task='multiclass', num_classes=c, average='none', validate_args=False)
    loose.update(logits.to(dev), bad.to(dev))
    got = loose.compute()
    np.testing.assert_allclose(got.numpy(), jaccard_from_confmat(torch.from_numpy(wb.reshape(c, c))).numpy(), rtol=1e-6, atol=0)
    assert np.array_equal(loose.confmat.cpu().numpy().reshape(-1), wb)
