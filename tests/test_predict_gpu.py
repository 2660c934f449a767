"""-m gpu: `muvo_amd.predict.run` end to end over a tiny recording - the shards of `--mode sim` against the host route of the
reference's sim_run.py:75-94 applied to the captured device tensors, `metrics.json` of `--mode test` against `test_step` driven
by hand.  One model and one recording for all cases."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 77


@pytest.fixture(scope='module')
def world(dev, tmp_path_factory):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path_factory.mktemp('rec'))
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    # 2 observed + 4 future frames: the imagination has the steps 0 and 3 of (0, 3, 9)
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(SEED)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)

    def data():
        dm = DataModule(cfg, root, device=dev, seed=SEED)
        dm.setup()
        assert len(dm.test_dataset) == 4 and len(dm.test_sampler_1) == 0
        dm.test_sampler_0, dm.test_sampler_2 = range(0, 4, 2), range(1, 4, 2)      # two batches each from a recording this small
        return dm
    return cfg, module, data


def _host_bytes(x):
    """The product's byte rule on the host: numpy's `(x * 255).astype(np.uint8)` where that is defined, saturated outside."""
    t = x.cpu().numpy() * np.float32(255)
    plain = np.nan_to_num(np.trunc(t), nan=0.0, posinf=255.0, neginf=0.0).clip(0, 255).astype(np.uint8)
    ok = (t >= 0) & (t < 256)
    assert np.array_equal(plain[ok], t[ok].astype(np.uint8))
    return plain


def _host_rows(grid):
    """sim_run.py:75-82: torch.where on the host grid, plus the class at those positions."""
    grid = grid.cpu()
    x, y, z = torch.where(grid != 0)
    return torch.stack([x, y, z, grid[x, y, z].long()], 1).numpy().astype(np.uint16)


def test_sim_shards_equal_the_host_route(dev, world, tmp_path):
    from muvo_amd import predict as P
    cfg, module, data = world
    seen = []

    def hook(i, batch, output, output_imagine):
        steps = [k for k in P.IMAGINE_STEPS if k < output_imagine['voxel_1'].shape[1]]
        assert output['voxel_1'].dtype == torch.float32 and output['voxel_1'].is_cuda
        want = {'rgb_label': _host_bytes(batch['rgb_label_1'][0][0]), 'throttle_brake': batch['throttle_brake'][0][0].cpu().numpy(),
                'steering': batch['steering'][0][0].cpu().numpy(), 'pcd_label': batch['range_view_label_1'][0][0].cpu().numpy(),
                'voxel_label': _host_rows(batch['voxel_label_1'][0][0].reshape(batch['voxel_label_1'].shape[-3:])),
                'rgb_re': _host_bytes(output['rgb_1'][0][0]), 'pcd_re': output['lidar_reconstruction_1'][0][0].cpu().numpy(),
                'voxel_re': _host_rows(torch.argmax(output['voxel_1'][0][0], dim=-4)),
                'rgb_im': _host_bytes(output_imagine['rgb_1'][0][steps]),
                'pcd_im': output_imagine['lidar_reconstruction_1'][0][steps].cpu().numpy(),
                'voxel_im': [_host_rows(torch.argmax(output_imagine['voxel_1'][0][k], dim=-4)) for k in steps]}
        seen.append((i, steps, want))

    out = P.run(cfg, dev, str(tmp_path), 'sim', limit_batches=2, shard_size=1, seed=SEED, hook=hook, data=data(), module=module,
                log=lambda s: None)
    assert out['batches'] == {2: 2} and [os.path.basename(f) for f in out['files']] == ['data_0.npz', 'data_1.npz']
    assert sorted(os.listdir(tmp_path)) == ['data_0.npz', 'data_1.npz'] and len(seen) == 2
    for path, (i, steps, want) in zip(out['files'], seen):
        back = P.read_shard(path)
        assert back['batch_index'].tolist() == [i] and back['imagine_steps'].tolist() == steps == [0, 3]
        for name in P.ENTRIES:
            got = back[name][0]
            if name == 'voxel_im':
                assert len(got) == len(steps)
                pairs = list(zip(got, want[name]))
            else:
                pairs = [(got, want[name])]
            for g, w in pairs:
                assert g.dtype == w.dtype and g.shape == w.shape, (i, name, g.dtype, w.dtype, g.shape, w.shape)
                assert g.tobytes() == w.tobytes(), (i, name)
        assert back['rgb_re'][0].dtype == np.uint8 and back['voxel_re'][0].dtype == np.uint16 and back['pcd_im'][0].dtype == np.float32
        assert len(back['voxel_label'][0]) > 0                     # the recording's voxel files are not empty
    # the two batches are different sequences
    assert seen[0][2]['rgb_label'].tobytes() != seen[1][2]['rgb_label'].tobytes()


def _stats(metrics):
    st = metrics['ssc'].get_stats()
    return {'ssim': float(metrics['ssim'].get_stat()), 'psnr': float(metrics['psnr'].get_stat()),
            'chamfer_distance': float(metrics['cd'].get_stat()), 'Voxel_Background_SemIoU': float(st['iou_ssc'][0]),
            'Voxel_Occupancy_SemIoU': float(st['iou_ssc'][1]), 'Voxel_mIoU': float(st['iou_ssc_mean']), 'Voxel_IoU': float(st['iou']),
            'Voxel_Precision': float(st['precision']), 'Voxel_Recall': float(st['recall'])}


def test_metrics_json_equals_test_step_by_hand(dev, world, tmp_path):
    """In the library's deterministic mode (no order-dependent float atomics in the forward pass): equal means equal."""
    from muvo_amd import ops
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        _metrics_json_equals_test_step_by_hand(dev, world, tmp_path)
    finally:
        ops.set_deterministic(was)


def _metrics_json_equals_test_step_by_hand(dev, world, tmp_path):
    from muvo_amd import predict as P
    cfg, module, data = world
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    out = P.run(cfg, dev, a, 'test', limit_batches=2, seed=SEED, data=data(), module=module, log=lambda s: None)
    assert out['batches'] == {0: 2, 1: 0, 2: 2} and os.listdir(a) == ['metrics.json']
    got = json.load(open(os.path.join(a, 'metrics.json')))
    names = P.expected_metric_names(cfg, out['batches'])
    assert len(names) == 4 * 9 and sorted(got) == sorted(names + ['batches'])
    assert got['batches'] == {'0': 2, '1': 0, '2': 2}
    assert all(isinstance(got[n], float) and np.isfinite(got[n]) for n in names), got
    # the metric objects are reset
    for sets in (module.metrics_tests, module.metrics_tests_imagine):
        assert sets[1] == {}
        for idx in (0, 2):
            m = sets[idx]
            assert m['ssim'].count == 1e-8 and m['psnr'].count == 1e-8 and m['cd'].count == 1e-8 and m['ssc'].count == 1e-8
            assert int(m['ssc'].tps.sum()) == 0 and float(m['ssim'].get_stat()) == 0.0
    # test_step by hand, with the seeds of the tool
    loaders = data().test_dataloader()
    want = {}
    for idx in (0, 2):
        for i, batch in enumerate(loaders[idx]):
            if i >= 2:
                break
            P.seed_batch(module, SEED, idx, i)
            output, output_imagines = module.test_step(batch, i, idx)
            assert len(output_imagines) == cfg.PREDICTION.N_SAMPLES and output['voxel_1'].shape[1] == 2
        for kind, sets in (('test', module.metrics_tests), ('test_imagine', module.metrics_tests_imagine)):
            want.update({f'{kind}{idx}_{k}': v for k, v in _stats(sets[idx]).items()})
    for n in names:
        print(n, got[n], want[n])
    assert sorted(want) == sorted(names)
    assert {n: got[n] for n in names} == want
    module.log_fn = lambda name, value: None
    try:
        module.on_test_epoch_end()
    finally:
        module.log_fn = None
    # a second run with the same seed writes the same file
    P.run(cfg, dev, b, 'test', limit_batches=2, seed=SEED, data=data(), module=module, log=lambda s: None)
    assert open(os.path.join(a, 'metrics.json'), 'rb').read() == open(os.path.join(b, 'metrics.json'), 'rb').read()
