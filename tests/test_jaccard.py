"""CPU: the host side of the segmentation IoU - `jaccard_from_confmat` against a float64 evaluation of the definition, the names
`log_metrics` sends for the bird's-eye-view, lidar and camera heads, and what `JaccardIndex` refuses."""
import numpy as np
import pytest
import torch

# three float32 roundings (numerator, denominator, quotient) of 2^-24 each are about 1.8e-7 relative
RTOL = 1e-6

BEV_NAMES = ['Background', 'Road', 'Lane marking', 'Vehicle', 'Pedestrian', 'Green light', 'Yellow light', 'Red light and stop sign']


def _jaccard64(m):
    """intersection / union per class in float64 from exact integer sums; union 0 -> 0."""
    m = np.asarray(m, dtype=np.int64)
    num = np.diag(m)
    den = m.sum(0) + m.sum(1) - num
    return np.where(den != 0, num.astype(np.float64) / np.where(den != 0, den, 1).astype(np.float64), 0.0)


def _check(m):
    from muvo_amd.metrics import jaccard_from_confmat
    got = jaccard_from_confmat(torch.from_numpy(m))
    assert got.dtype == torch.float32 and got.shape == (m.shape[0],)
    want = _jaccard64(m)
    np.testing.assert_allclose(got.numpy().astype(np.float64), want, rtol=RTOL, atol=0)
    return got, want


@pytest.mark.parametrize('c', [2, 8, 9, 16])
def test_jaccard_from_confmat_random(c):
    rs = np.random.RandomState(c)
    _check(rs.randint(0, 5000, size=(c, c)).astype(np.int64))
    # counts above 2^24: float32 no longer holds them exactly
    big = rs.randint(1 << 24, 1 << 40, size=(c, c), dtype=np.int64)
    assert big.min() > 1 << 24
    _check(big)
    # one class absent from label and prediction: exactly 0, and it still counts in the mean
    m = rs.randint(1, 5000, size=(c, c)).astype(np.int64)
    k = c // 2
    m[k, :] = 0
    m[:, k] = 0
    got, want = _check(m)
    assert float(got[k]) == 0.0 and want[k] == 0.0
    assert abs(float(got.mean()) - want.sum() / c) <= RTOL * want.sum() / c
    assert float(got.mean()) < float(got[torch.arange(c) != k].mean())
    # perfect prediction: all 1
    got, _ = _check(np.diag(rs.randint(1, 1 << 30, size=c)).astype(np.int64))
    assert got.tolist() == [1.0] * c


def test_jaccard_from_confmat_all_empty():
    from muvo_amd.metrics import jaccard_from_confmat
    assert jaccard_from_confmat(torch.zeros(9, 9, dtype=torch.int64)).tolist() == [0.0] * 9


def test_metric_names_with_the_three_heads():
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.predict import expected_metric_names
    from muvo_amd.trainer import metric_log_names, metric_names
    cfg = base_1d_cfg(SEMANTIC_SEG__ENABLED=True, LIDAR_SEG__ENABLED=True, SEMANTIC_IMAGE__ENABLED=True)
    assert (cfg.SEMANTIC_SEG.N_CHANNELS, cfg.LIDAR_SEG.N_CLASSES, cfg.SEMANTIC_IMAGE.N_CLASSES) == (8, 9, 9)
    voxel = ['Voxel_Background_SemIoU', 'Voxel_Occupancy_SemIoU', 'Voxel_mIoU', 'Voxel_IoU', 'Voxel_Precision', 'Voxel_Recall']
    want = ([f'bev_iou_{n}' for n in BEV_NAMES] + ['bev_mean_iou', 'ssim', 'psnr', 'chamfer_distance'] +
            # nine lidar / camera classes, two names in the reference's table: the zip stops there
            ['lidar_iou_Background', 'lidar_iou_Occupancy', 'lidar_mean_iou'] +
            ['camera_iou_Background', 'camera_iou_Occupancy', 'camera_mean_iou'] + voxel)
    assert metric_names(cfg, 'test0') == [f'test0_{n}' for n in want]
    assert metric_names(cfg, 'val_imagine2') == [f'val_imagine2_{n}' for n in want]
    # the names that go through self.log are the same as without the heads
    assert metric_log_names(cfg, 'test0') == metric_log_names(base_1d_cfg(), 'test0')
    assert [n for n in metric_names(cfg, 'test0') if '_iou_' not in n and 'mean_iou' not in n] == metric_log_names(cfg, 'test0')
    lidar = base_1d_cfg(LIDAR_SEG__ENABLED=True)
    assert [n for n in metric_names(lidar, 'val1') if 'lidar' in n] == ['val1_lidar_iou_Background', 'val1_lidar_iou_Occupancy',
                                                                         'val1_lidar_mean_iou']
    three = base_1d_cfg(SEMANTIC_SEG__ENABLED=True, SEMANTIC_SEG__N_CHANNELS=3)
    assert metric_names(three, 't0')[:4] == ['t0_bev_iou_Background', 't0_bev_iou_Road', 't0_bev_iou_Lane marking', 't0_bev_mean_iou']
    names = expected_metric_names(cfg, {0: 1, 1: 0, 2: 3})
    assert names == [f'{k}_{n}' for k in ('test0', 'test2', 'test_imagine0', 'test_imagine2') for n in want]


def test_metric_names_without_the_heads_are_the_log_names():
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.trainer import metric_log_names, metric_names
    for cfg in (base_1d_cfg(), base_1d_cfg(EVAL__RGB_SUPERVISION=False), base_1d_cfg(VOXEL_SEG__N_CLASSES=9),
                base_1d_cfg(EVAL__RGB_SUPERVISION=False, LIDAR_RE__ENABLED=False, VOXEL_SEG__ENABLED=False)):
        assert metric_names(cfg, 'test1') == metric_log_names(cfg, 'test1')


def test_jaccard_index_refuses_what_is_not_built():
    from muvo_amd.metrics import JaccardIndex
    with pytest.raises(NotImplementedError, match='macro'):
        JaccardIndex(task='multiclass', num_classes=8, average='macro')
    with pytest.raises(NotImplementedError, match='binary'):
        JaccardIndex(task='binary', num_classes=2, average='none')
    with pytest.raises(ValueError):
        JaccardIndex(task='multiclass', num_classes=17, average='none')
    with pytest.raises(ValueError):
        JaccardIndex(task='multiclass', num_classes=1, average='none')


def test_class_bytes_send_every_value_outside_the_classes_to_255():
    """The label conversion in front of the kernel, on the host: no value wraps into a valid class."""
    from muvo_amd.metrics import _class_bytes
    t = torch.tensor([-1, 0, 8, 9, 255, 256, 300, -256, 1 << 40], dtype=torch.int64)
    assert _class_bytes(t, 9).tolist() == [255, 0, 8, 255, 255, 255, 255, 255, 255]
    assert _class_bytes(t, 9).dtype == torch.uint8
    assert _class_bytes(torch.tensor([-1, 1, 127], dtype=torch.int8), 2).tolist() == [255, 1, 255]
    u8 = torch.tensor([0, 9, 255], dtype=torch.uint8)
    assert _class_bytes(u8, 9).tolist() == [0, 9, 255]              # bytes pass: the kernel itself sends >= C out of range
    with pytest.raises(TypeError):
        _class_bytes(torch.zeros(3), 9)
