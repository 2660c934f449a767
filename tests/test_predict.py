"""CPU: the host side of `python -m muvo_amd.predict` - shard layout, metric names, command line, the one-process rule."""
import numpy as np
import pytest


def _record(rs, q_label, q_re, q_im, k):
    def rows(q):
        return rs.randint(0, 60000, size=(q, 4)).astype(np.uint16)
    return {'rgb_label': rs.randint(0, 256, size=(3, 5, 7)).astype(np.uint8), 'rgb_re': rs.randint(0, 256, size=(3, 5, 7)).astype(np.uint8),
            'rgb_im': rs.randint(0, 256, size=(k, 3, 5, 7)).astype(np.uint8),
            'throttle_brake': rs.rand(1).astype(np.float32), 'steering': rs.rand(1).astype(np.float32),
            'pcd_label': rs.randn(4, 6, 8).astype(np.float32), 'pcd_re': rs.randn(4, 6, 8).astype(np.float32),
            'pcd_im': rs.randn(k, 4, 6, 8).astype(np.float32),
            'voxel_label': rows(q_label), 'voxel_re': rows(q_re), 'voxel_im': [rows(q) for q in q_im]}


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize('k', [3, 1, 0])
def test_shard_round_trip(tmp_path, k):
    from muvo_amd import predict as P
    rs = np.random.RandomState(5 + k)
    steps = list(P.IMAGINE_STEPS[:k])
    # batch 1 has no occupied voxel anywhere; batch 2 an empty imagined step between two filled ones
    records = [_record(rs, 11, 4, [3, 9, 2][:k], k), _record(rs, 0, 0, [0, 0, 0][:k], k), _record(rs, 1, 70000, [5, 0, 6][:k], k)]
    path = P.write_shard(str(tmp_path / 'data_9.npz'), records, [7, 8, 9], steps)
    back = P.read_shard(path)
    assert sorted(back) == sorted(P.ENTRIES + ('imagine_steps', 'batch_index'))
    assert back['batch_index'].tolist() == [7, 8, 9] and back['imagine_steps'].tolist() == steps
    for name in P.ENTRIES:
        assert len(back[name]) == 3, name
        for got, rec in zip(back[name], records):
            if name == 'voxel_im':
                assert len(got) == k and all(_same(g, w) for g, w in zip(got, rec[name])), name
            else:
                assert _same(got, rec[name]), name
    with np.load(path) as z:
        assert z['voxel_re_rows'].dtype == np.uint16 and z['voxel_re_rows'].shape == (70004, 4)
        assert z['voxel_label_offsets'].tolist() == [0, 11, 11, 12] and z['voxel_label_offsets'].dtype == np.int64
        assert len(z['voxel_im_offsets']) == 3 * k + 1
        assert z['rgb_im'].shape == (3, k, 3, 5, 7) and z['pcd_label'].dtype == np.float32


def test_metric_names_of_base_1d_and_without_rgb():
    from muvo_amd.config import base_1d_cfg
    from muvo_amd.predict import expected_metric_names
    from muvo_amd.trainer import VOXEL_LABEL, metric_heads_left_out, metric_log_names
    assert VOXEL_LABEL == ('Background', 'Occupancy')
    cfg = base_1d_cfg()
    voxel = ['Voxel_Background_SemIoU', 'Voxel_Occupancy_SemIoU', 'Voxel_mIoU', 'Voxel_IoU', 'Voxel_Precision', 'Voxel_Recall']
    full = ['ssim', 'psnr', 'chamfer_distance'] + voxel
    assert metric_log_names(cfg, 'test0') == [f'test0_{n}' for n in full]
    assert metric_log_names(cfg, 'val_imagine2') == [f'val_imagine2_{n}' for n in full]
    no_rgb = base_1d_cfg(EVAL__RGB_SUPERVISION=False)
    assert metric_log_names(no_rgb, 'test1') == [f'test1_{n}' for n in ['chamfer_distance'] + voxel]
    nine = base_1d_cfg(VOXEL_SEG__N_CLASSES=9)                 # the reference's zip stops at the two names of its table
    assert metric_log_names(nine, 'test0') == metric_log_names(cfg, 'test0')
    assert metric_log_names(base_1d_cfg(EVAL__RGB_SUPERVISION=False, LIDAR_RE__ENABLED=False, VOXEL_SEG__ENABLED=False), 'test0') == []
    # an empty loader logs nothing; reconstruction sets come before the imagined ones
    names = expected_metric_names(cfg, {0: 2, 1: 0, 2: 1})
    assert names == ([f'test0_{n}' for n in full] + [f'test2_{n}' for n in full] +
                     [f'test_imagine0_{n}' for n in full] + [f'test_imagine2_{n}' for n in full])
    assert metric_heads_left_out(cfg) == []
    assert metric_heads_left_out(base_1d_cfg(SEMANTIC_SEG__ENABLED=True, SEMANTIC_IMAGE__ENABLED=True)) == ['bev_iou', 'camera_iou']


def test_argument_parsing():
    from muvo_amd import predict as P
    from muvo_amd.config import get_cfg
    a = P.parse_args(['--config-file', 'muvo_amd/configs/test_base_1d.yml', '--dataset-root', '/data/x', '--checkpoint', 'w.ckpt',
                      '--out', 'o', '--mode', 'sim', 'BATCHSIZE', '1'])
    assert (a.dataset_root, a.checkpoint, a.out, a.mode, a.loader, a.limit_batches, a.shard_size, a.seed) == \
        ('/data/x', 'w.ckpt', 'o', 'sim', None, None, 500, 1234)
    assert a.opts == ['BATCHSIZE', '1'] and get_cfg(a).BATCHSIZE == 1
    assert P.chosen_loaders('sim') == [2] and P.chosen_loaders('test') == [0, 1, 2] and P.chosen_loaders('test', 1) == [1]
    b = P.parse_args(['--out', 'o', '--mode', 'test', '--loader', '0', '--limit-batches', '3', '--shard-size', '7', '--seed', '5'])
    assert (b.loader, b.limit_batches, b.shard_size, b.seed) == (0, 3, 7, 5)
    for bad in (['--out', 'o'], ['--mode', 'test'], ['--out', 'o', '--mode', 'train'], ['--out', 'o', '--mode', 'sim', '--loader', '3'],
                ['--out', 'o', '--mode', 'sim', '--limit-batches', '0'], ['--out', 'o', '--mode', 'sim', '--shard-size', '0']):
        with pytest.raises(SystemExit):
            P.parse_args(bad)


def test_refuses_more_than_one_process(monkeypatch, tmp_path):
    from muvo_amd import predict as P
    from muvo_amd.config import base_1d_cfg
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(RuntimeError, match='one process'):
        P.run(base_1d_cfg(), 'cuda:0', str(tmp_path / 'out'), 'test')
    with pytest.raises(RuntimeError, match='WORLD_SIZE=2'):
        P.main(['--out', str(tmp_path / 'out'), '--mode', 'sim'])
    assert not (tmp_path / 'out').exists()
    monkeypatch.setenv('WORLD_SIZE', '1')
    P.refuse_multi_process()
