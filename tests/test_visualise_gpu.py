"""-m gpu: `muvo_amd.visualise.render_panels` against the host restatement (every panel) and against bytes of the real reference
(tests/golden/visualise_ref.npz: the panels it can draw without cv2 / open3d / matplotlib), then the way through
`WorldModelTrainer.test_step` and `python -m muvo_amd.predict --mode test --panels N` on a miniature recording."""
import os

import numpy as np
import pytest
import torch

import visualise_reference as VR

pytestmark = pytest.mark.gpu
SEED = 78
ALL = dict(bev=True, rgb=True, lidar=True, lidar_seg=True, sem_image=True, depth=True, voxel=True, route=True)


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _render(dev, cfg, batch, output, imagines):
    from muvo_amd.visualise import render_panels
    got = render_panels(cfg, _to(batch, dev), _to(output, dev), [_to(i, dev) for i in imagines])
    assert all(v.dtype == torch.uint8 and v.device.type == 'cuda' for v in got.values())
    return {k: v.cpu().numpy() for k, v in got.items()}


def _compare(got, want):
    assert list(got) == list(want)
    for suffix in want:
        assert got[suffix].shape == want[suffix].shape, (suffix, got[suffix].shape, want[suffix].shape)
        bad = np.argwhere(got[suffix] != want[suffix])
        assert len(bad) == 0, (suffix, len(bad), bad[:5].tolist())


@pytest.mark.parametrize('n', [0, 1, 2])
def test_panels_equal_restatement_and_reference(dev, n):
    """n imagined samples at the fixture's shapes; n = 0: rf == s, no separator."""
    from muvo_amd.visualise import SUFFIXES
    cfg = VR.panel_cfg(**ALL)
    batch, output, imagines = VR.fixture_inputs(n)
    got = _render(dev, cfg, batch, output, imagines)
    assert tuple(got) == SUFFIXES
    _compare(got, VR.render_panels(cfg, batch, output, imagines))
    with np.load(os.path.join(os.path.dirname(__file__), 'golden', 'visualise_ref.npz')) as z:
        for suffix in VR.FIXTURE_SUFFIXES:
            assert np.array_equal(got[suffix], z[f'n{n}{suffix}']), suffix


def test_panels_with_classes_past_the_tables(dev):
    """Nine lidar / camera classes (LIDAR_SEG.N_CLASSES) on the two-entry table, labels as uint8, an uneven split rf = 4, fh = 1."""
    cfg = VR.panel_cfg(**ALL)
    batch, output, imagines = VR.fixture_inputs(1, seed=5, seg_classes=9, rf=4)
    for key in ('birdview_label', 'range_view_seg_label_1', 'semantic_image_label_1'):
        batch[key] = batch[key].to(torch.uint8)
    _compare(_render(dev, cfg, batch, output, imagines), VR.render_panels(cfg, batch, output, imagines))


def test_rows_that_do_not_cover_the_label_are_refused(dev):
    cfg = VR.panel_cfg(depth=True)
    batch, output, _ = VR.fixture_inputs(1)
    with pytest.raises(ValueError, match='cover every step'):
        _render(dev, cfg, batch, output, [])


@pytest.fixture(scope='module')
def world(dev, tmp_path_factory):
    pytest.importorskip('pandas')
    pytest.importorskip('PIL')
    from muvo_amd.data import recording_inputs as RI
    from muvo_amd.data.dataset import DataModule
    from muvo_amd.trainer import WorldModelTrainer
    root = str(tmp_path_factory.mktemp('rec'))
    RI.write_recording(root, runs=(('train', 'Town01', '0000', 18, True),))
    cfg = RI.recording_cfg('default', RECEPTIVE_FIELD=2, FUTURE_HORIZON=4, BATCHSIZE=1, STEPS=100000)
    torch.manual_seed(SEED)
    module = WorldModelTrainer(cfg.convert_to_dict(), device=dev)

    def data():
        dm = DataModule(cfg, root, device=dev, seed=SEED)
        dm.setup()
        dm.test_sampler_0, dm.test_sampler_2 = range(0, 4, 2), range(1, 4, 2)
        return dm
    return cfg, module, data


def test_predict_writes_the_panels_of_the_first_batches(dev, world, tmp_path):
    from muvo_amd import predict as P
    from muvo_amd.visualise import VIDEO_SUFFIXES, panel_enabled, png_read, render_panels
    cfg, module, data = world
    want = {}

    def hook(i, batch, output, output_imagines):
        if i == 0:
            want.update({k: v.cpu().numpy() for k, v in render_panels(cfg, batch, output, output_imagines).items()})
    out = P.run(cfg, dev, str(tmp_path), 'test', loaders=[0], limit_batches=2, seed=SEED, hook=hook, data=data(), module=module,
                log=lambda s: None, panels=1)
    assert out['batches'] == {0: 2} and module.panel_writer is None
    suffixes = panel_enabled(cfg)
    assert list(want) == suffixes and {'_rgb', '_lidar', '_pcd_xy', '_voxel_top', '_input_route_map'} <= set(suffixes)
    files = sorted(os.path.relpath(f, str(tmp_path)) for f in out['files'])
    assert files == sorted(['metrics.json'] + [f'panels/pred0_outputs_0{k}/step00000000_b0.png' for k in suffixes])   # batch 1: none
    for k in suffixes:
        image = png_read(open(os.path.join(str(tmp_path), 'panels', f'pred0_outputs_0{k}', 'step00000000_b0.png'), 'rb').read())
        panel = want[k][0]
        if k in VIDEO_SUFFIXES:
            assert np.array_equal(image, np.concatenate(list(panel[:, 0]), axis=1)), k
        else:
            assert np.array_equal(image, panel.transpose(1, 2, 0)), k
            assert len(np.unique(image)) > 2, k


def test_test_step_is_the_same_with_and_without_a_writer(dev, world):
    """Deterministic mode, the seeds of the tool: the tensors test_step returns do not depend on the writer."""
    from muvo_amd import ops
    from muvo_amd import predict as P
    cfg, module, data = world
    seen = []

    class Writer:
        def add_images(self, name, tensor, global_step=0):
            seen.append((name, tuple(tensor.shape)))

        def add_video(self, name, tensor, global_step=0, fps=2):
            seen.append((name, tuple(tensor.shape)))
    batch = next(iter(data().test_dataloader()[2]))
    was = ops.get_deterministic()
    ops.set_deterministic(True)
    try:
        runs = []
        for writer in (None, Writer()):
            module.panel_writer = writer
            P.seed_batch(module, SEED, 2, 0)
            output, imagines = module.test_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 3, 2)
            runs.append([output] + list(imagines))
    finally:
        module.panel_writer = None
        ops.set_deterministic(was)
        for sets in (module.metrics_tests, module.metrics_tests_imagine):
            sets[2].clear()
    assert seen and all(n.startswith('pred2_outputs_3_') for n, _ in seen)
    for a, b in zip(*runs):
        assert a.keys() == b.keys()
        for key in a:
            if torch.is_tensor(a[key]):
                assert torch.equal(a[key], b[key]), key
