"""CPU: the host side of the prediction panels - the restatement (tests/visualise_reference.py) against bytes the real
reference produced (tests/golden/visualise_ref.npz, tools/make_golden_visualise.py), planted errors, panel sizes, the PNG
writer, the command lines and the `vis_step` criterion."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import visualise_reference as VR

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'visualise_ref.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _fixture_cfg():
    return VR.panel_cfg(**{k: True for k in VR.FIXTURE_HEADS})


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize('n', [0, 1, 2])
def test_restatement_equals_the_reference_bytes(golden, n):
    batch, output, imagines = VR.fixture_inputs(n)
    got = VR.render_panels(_fixture_cfg(), batch, output, imagines)
    assert tuple(got) == VR.FIXTURE_SUFFIXES
    for suffix in VR.FIXTURE_SUFFIXES:
        assert _same(got[suffix], golden[f'n{n}{suffix}']), suffix


def test_pcd_xy_image_equals_the_reference_bytes(golden):
    rv = VR.fixture_range_view()
    got = VR.to_u8(VR.pcd_xy_image(rv).numpy())
    assert _same(got, golden['pcd_xy_image'])
    assert 0 < int((got == 255).sum()) < got.size // 10 and set(np.unique(got)) == {0, 255}
    # the fixture has points on a bound: a non-strict comparison draws them
    assert not _same(VR.to_u8(VR.pcd_xy_image(rv, strict=False).numpy()), golden['pcd_xy_image'])


def test_planted_errors_are_rejected(golden):
    batch, output, imagines = VR.fixture_inputs(2)
    s, rf = VR.FIXTURE['s'], VR.FIXTURE['rf']
    get = lambda key: [i[key] for i in imagines]
    sem = batch['semantic_image_label_1'][:, :, 0], output['semantic_image_1'], get('semantic_image_1'), s, rf
    assert _same(VR.sem_image(*sem), golden['n2_sem_image'])
    assert not _same(VR.sem_image(*sem, reverse_rows=True), golden['n2_sem_image'])            # swapped row order
    assert not _same(VR.sem_image(*sem, sep_at=rf + 1), golden['n2_sem_image'])                # separator one step late
    bev = batch['birdview_label'][:, :, 0], output['bev_segmentation_1'], get('bev_segmentation_1'), s, rf
    assert _same(VR.bev(*bev), golden['n2_bev'])
    wrong = VR.bev(*bev, transposed_rotation=True)                                             # transposed, not rotated
    assert wrong.shape == golden['n2_bev'].shape and not np.array_equal(wrong, golden['n2_bev'])
    route = VR.route_map(batch['route_map'], s, rf)
    assert _same(route, golden['n2_input_route_map'])
    assert not _same(VR.route_map(batch['route_map'], s, rf, sep_at=rf - 1), golden['n2_input_route_map'])


def test_palette_bytes_survive_the_float_route():
    from muvo_amd.visualise import BIRDVIEW_COLOURS, VOXEL_COLOURS, palette256
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(VR.to_u8((torch.from_numpy(every) / 255.0).numpy()), every)
    assert VR.to_u8(np.float32(0.8)) == 204 and VR.to_u8(np.array(0.2)) == 51
    for table in (BIRDVIEW_COLOURS, VOXEL_COLOURS):
        pal = palette256(table)
        assert pal.shape == (256, 3) and pal.dtype == np.uint8 and pal[:len(table)].tolist() == [list(c) for c in table]
        c = len(table) + 3
        assert pal[c].tolist() == [(37 * c) % 256, (91 * c + 60) % 256, (151 * c + 120) % 256]


@pytest.mark.parametrize('n', [0, 1, 2])
def test_panel_sizes(golden, n):
    from muvo_amd.visualise import panel_enabled, panel_sizes
    cfg = VR.panel_cfg(bev=True, rgb=True, lidar=True, lidar_seg=True, sem_image=True, depth=True, voxel=True, route=True)
    batch, output, imagines = VR.fixture_inputs(n)
    s, rf = VR.FIXTURE['s'], (VR.FIXTURE['rf'] if n else VR.FIXTURE['s'])
    shapes = {k: VR.FIXTURE[k] for k in ('bev', 'rgb', 'lidar', 'lidar_seg', 'sem_image', 'depth', 'voxel', 'route')}
    sizes = panel_sizes(cfg, shapes, s, rf, max(n, 1))
    assert list(sizes) == panel_enabled(cfg)
    want = VR.render_panels(cfg, batch, output, imagines)
    assert list(want) == list(sizes)
    for suffix, size in sizes.items():
        assert want[suffix].shape == (VR.FIXTURE['b'], *size), suffix
        if f'n{n}{suffix}' in golden:
            assert golden[f'n{n}{suffix}'].shape == (VR.FIXTURE['b'], *size), suffix
    if n == 2:
        assert sizes['_bev'] == (3, 42, 52) and sizes['_pcd_xy'] == (3, 3 * 260, 5 * 260 + 65)
        assert sizes['_rgb'] == (3, 2 + 2 + 3 * 18, 5 * 22 + 3) and sizes['_lidar_seg'] == (3, 16 * 10, 22)


def test_voxel_top_definition():
    """Hand-made columns: empty, occupied only at z = 0, a class beyond the table on top."""
    from muvo_amd.visualise import VOXEL_COLOURS, palette256
    grid = np.zeros((1, 1, 2, 3, 5), np.uint8)
    grid[0, 0, 0, 1, 0] = 1                       # only the bottom voxel
    grid[0, 0, 1, 2, 1], grid[0, 0, 1, 2, 4] = 1, 7
    tile = VR.voxel_top_tiles(grid, VOXEL_COLOURS)
    pal = palette256(VOXEL_COLOURS).astype(int)
    assert tile.shape == (1, 1, 3, 2, 3)
    assert tile[0, 0, :, 1, 0].tolist() == [255, 255, 255]                                     # x = 0, y = 0: empty -> palette[0]
    assert tile[0, 0, :, 1, 1].tolist() == [(115 * 96) // 255] * 3                             # x = 0 is the LAST tile row
    assert tile[0, 0, :, 0, 2].tolist() == [(int(p) * (96 + 159)) // 255 for p in pal[7]]      # z* = Z - 1: full brightness


def test_png_round_trip(tmp_path):
    from muvo_amd.visualise import PanelWriter, png_bytes, png_read
    rs = np.random.RandomState(3)
    for shape in ((5, 7, 3), (1, 1, 3), (4, 9)):
        image = rs.randint(0, 256, size=shape).astype(np.uint8)
        assert np.array_equal(png_read(png_bytes(image)), image)
    PIL = pytest.importorskip('PIL.Image')
    image = rs.randint(0, 256, size=(6, 11, 3)).astype(np.uint8)
    path = tmp_path / 'a.png'
    path.write_bytes(png_bytes(image))
    assert np.array_equal(np.asarray(PIL.open(str(path))), image)
    writer = PanelWriter(str(tmp_path / 'out'))
    panel = torch.from_numpy(rs.randint(0, 256, size=(2, 3, 4, 6)).astype(np.uint8))
    video = torch.from_numpy(rs.randint(0, 256, size=(2, 3, 1, 4, 5)).astype(np.uint8))
    writer.add_images('pred0_outputs_1_bev', panel, global_step=12)
    writer.add_video('pred0_outputs_1_depth', video, global_step=12, fps=2)
    assert [os.path.relpath(f, writer.directory) for f in writer.files] == [
        'pred0_outputs_1_bev/step00000012_b0.png', 'pred0_outputs_1_bev/step00000012_b1.png',
        'pred0_outputs_1_depth/step00000012_b0.png', 'pred0_outputs_1_depth/step00000012_b1.png']
    for i in range(2):
        got = png_read(open(writer.files[i], 'rb').read())
        assert np.array_equal(got, panel[i].numpy().transpose(1, 2, 0))
        got = png_read(open(writer.files[2 + i], 'rb').read())
        assert got.shape == (4, 15) and np.array_equal(got, np.concatenate(list(video[i, :, 0].numpy()), axis=1))


def test_command_lines():
    from muvo_amd import predict as P
    from muvo_amd import train as T
    base = ['--out', 'o', '--mode', 'test']
    assert P.parse_args(base).panels == 0
    assert P.parse_args(base + ['--panels', '3']).panels == 3
    with pytest.raises(SystemExit):
        P.parse_args(base + ['--panels', '-1'])
    with pytest.raises(SystemExit):
        P.parse_args(['--out', 'o', '--mode', 'sim', '--panels', '1'])
    assert T.build_parser().parse_args([]).panel_dir == ''
    assert T.build_parser().parse_args(['--panel-dir', 'p']).panel_dir == 'p'


def test_vis_step_criterion():
    """trainer.py:502-509: training draws on the multiples of LOG_VIDEO_INTERVAL, once per step; evaluation on batch 0; and
    nothing at all without a writer."""
    from muvo_amd.trainer import WorldModelTrainer
    calls = []

    class Writer:
        def add_images(self, *a, **k):
            raise AssertionError('the fake visualise never reaches the writer')
        add_video = add_images
    this = SimpleNamespace(cfg=SimpleNamespace(LOG_VIDEO_INTERVAL=4), vis_step=-1, panel_writer=Writer(), _global_step=0, global_step=0,
                           log=lambda *a, **k: None)
    this._step_now = lambda: this._global_step
    this.visualise = lambda batch, output, imagines, batch_idx, prefix='train': calls.append((prefix, this._global_step, batch_idx))
    hook = WorldModelTrainer.logging_and_visualisation
    for step in range(10):
        this._global_step = this.global_step = step
        for micro in range(2):                                   # two micro-batches of one optimizer step: drawn once
            hook(this, {}, {}, [], {}, None, 2 * step + micro, prefix='train')
    assert calls == [('train', 0, 0), ('train', 4, 8), ('train', 8, 16)] and this.vis_step == 9
    del calls[:]
    for batch_idx in range(3):
        hook(this, {}, {}, [], {}, None, batch_idx, prefix='val1')
    assert calls == [('val1', 9, 0)]
    del calls[:]
    this.panel_writer, this.vis_step = None, -1
    for step in range(5):
        this._global_step = step
        hook(this, {}, {}, [], {}, None, step, prefix='train')
        hook(this, {}, {}, [], {}, None, 0, prefix='val0')
    assert calls == [] and this.vis_step == -1
