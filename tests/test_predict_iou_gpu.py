"""-m gpu: `muvo_amd.predict.run(..., 'test')` with the bird's-eye-view, lidar and camera segmentation heads on, over a tiny
recording: the confusion matrices and IoU values of `metrics.json` against matrices built on the host (torch.argmax + bincount)
from the logits and labels a hook copies out of every reconstruction and imagined output.  One model, one recording."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 78

BEV_NAMES = ['Background', 'Road', 'Lane marking', 'Vehicle', 'Pedestrian', 'Green light', 'Yellow light', 'Red light and stop sign']
VOXEL_NAMES = ['Background', 'Occupancy']
# tag in the logged names: (output key, label key, class names the scores are zipped with)
HEADS = {'bev': ('bev_segmentation_1', 'birdview_label', BEV_NAMES),
         'lidar': ('lidar_segmentation_1', 'range_view_seg_label_1', VOXEL_NAMES),
         'camera': ('semantic_image_1', 'semantic_image_label_1', VOXEL_NAMES)}


@pytest.fixture(scope='module')
def world(dev, tmp_path_factory):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path_factory.mktemp('rec'))
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('heads_on', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1)
    torch.manual_seed(SEED)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)
    dm = DataModule(cfg, root, device=dev, seed=SEED)
    dm.setup()
    assert len(dm.test_dataset) == 4 and len(dm.test_sampler_1) == 0
    dm.test_sampler_0, dm.test_sampler_2 = range(0, 4, 2), range(1, 4, 2)      # two batches each from a recording this small
    return cfg, module, dm


def _host_confusion(logits, label, c):
    """logits (b, s, C, H, W), label (b, s, 1, H, W) on the host -> (C, C) int64 [label][prediction]."""
    assert logits.shape[2] == c and label.numel() == logits.numel() // c
    p = torch.argmax(logits, dim=2).reshape(-1).numpy().astype(np.int64)
    t = label.reshape(-1).numpy().astype(np.int64)
    assert t.min() >= 0 and t.max() < c
    return np.bincount(t * c + p, minlength=c * c).reshape(c, c)


def test_metrics_json_holds_the_iou_of_the_three_heads(dev, world, tmp_path):
    from muvo_amd import predict as P
    cfg, module, dm = world
    rf = cfg.RECEPTIVE_FIELD
    classes = {'bev': cfg.SEMANTIC_SEG.N_CHANNELS, 'lidar': cfg.LIDAR_SEG.N_CLASSES, 'camera': cfg.SEMANTIC_IMAGE.N_CLASSES}
    assert classes == {'bev': 8, 'lidar': 9, 'camera': 9}
    seen, lines = [], []

    def hook(i, batch, output, output_imagines):
        entry = {}
        for tag, (out_key, label_key, _) in HEADS.items():
            assert output[out_key].is_cuda and output[out_key].shape[1] == rf
            label = batch[label_key].cpu()
            entry[tag] = [_host_confusion(output[out_key].float().cpu(), label[:, :rf], classes[tag]),
                          sum(_host_confusion(o[out_key].float().cpu(), label[:, rf:], classes[tag]) for o in output_imagines)]
        assert len(output_imagines) == cfg.PREDICTION.N_SAMPLES >= 1
        seen.append((i, entry))

    out = P.run(cfg, dev, str(tmp_path), 'test', limit_batches=2, seed=SEED, hook=hook, data=dm, module=module, log=lines.append)
    assert out['batches'] == {0: 2, 1: 0, 2: 2} and os.listdir(tmp_path) == ['metrics.json']
    assert [i for i, _ in seen] == [0, 1, 0, 1]                        # loader 0, then loader 2
    assert not any('no_metric_for' in line for line in lines) and lines
    got = json.load(open(os.path.join(tmp_path, 'metrics.json')))
    names = P.expected_metric_names(cfg, out['batches'])
    confusion_names = [f'{kind}{idx}_{tag}_confusion' for kind in ('test', 'test_imagine') for idx in (0, 2) for tag in HEADS]
    assert sorted(got) == sorted(names + confusion_names + ['batches'])
    assert all(isinstance(got[n], float) and np.isfinite(got[n]) for n in names), got
    checked = 0
    for k, idx in enumerate((0, 2)):
        for which, kind in enumerate(('test', 'test_imagine')):
            for tag, (_, _, class_names) in HEADS.items():
                c = classes[tag]
                want = sum(entry[tag][which] for _, entry in seen[2 * k:2 * k + 2])
                matrix = got[f'{kind}{idx}_{tag}_confusion']
                assert isinstance(matrix, list) and all(isinstance(v, int) for row in matrix for v in row)
                assert np.array_equal(np.asarray(matrix, dtype=np.int64), want), (kind, idx, tag)
                assert want.sum() > 0
                num = np.diag(want).astype(np.float64)
                den = (want.sum(0) + want.sum(1)).astype(np.float64) - num
                iou = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)
                for j, name in enumerate(class_names[:c]):
                    v = got[f'{kind}{idx}_{tag}_iou_{name}']
                    print(f'{kind}{idx}_{tag}_iou_{name}', v, iou[j])
                    assert abs(v - iou[j]) <= 1e-6 * max(iou[j], 1e-30) or v == iou[j], (kind, idx, tag, name, v, iou[j])
                    checked += 1
                v = got[f'{kind}{idx}_{tag}_mean_iou']                   # over ALL classes, named or not
                print(f'{kind}{idx}_{tag}_mean_iou', v, iou.mean())
                assert abs(v - iou.mean()) <= 1e-6 * iou.mean() or v == iou.mean(), (kind, idx, tag, v, iou.mean())
                checked += 1
    assert checked == 4 * (9 + 3 + 3) == sum('iou' in n for n in names)
    # the metric objects are reset
    for sets in (module.metrics_tests, module.metrics_tests_imagine):
        assert sets[1] == {}
        for idx in (0, 2):
            for key in ('iou', 'pcd_iou', 'image_iou'):
                assert int(sets[idx][key].confmat.sum()) == 0 and int(sets[idx][key].out_of_range) == 0
            assert sets[idx]['ssim'].count == 1e-8 and int(sets[idx]['ssc'].tps.sum()) == 0
    assert module.on_confusion is None and module.log_fn is None
