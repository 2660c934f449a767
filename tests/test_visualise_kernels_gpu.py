"""-m gpu: every tile kind of csrc/visualise.hip, bit for bit against the host restatement (tests/visualise_reference.py), in
panels that lie between guard bytes: whatever a kernel writes outside its own tiles shows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import visualise_reference as VR

pytestmark = pytest.mark.gpu
S = VR.SENTINEL


def _check(buf, expect, guard, what=''):
    got, want = buf.cpu().numpy(), VR.expected_buffer(expect, guard)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _pal(table, dev):
    from muvo_amd.visualise import palette256
    return torch.from_numpy(palette256(table)).to(dev)


def _special_values():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                           np.array([np.nan, np.inf, -np.inf, -1 / 50, 1 + 1e-6, -0.0], np.float32)])
    return torch.from_numpy(vals)


@pytest.mark.parametrize('guard', [64, 3])
@pytest.mark.parametrize('shape,pad,x0', [((6, 3, 5, 7), 5, 0), ((6, 3, 5, 7), 5, 3), ((4, 1, 6, 16), 0, 0), ((4, 1, 6, 16), 0, 2)])
def test_float_tiles(dev, shape, pad, x0, guard):
    from muvo_amd import ops
    F_, C, h, w = shape
    b, T = 2, F_ // 2
    vals = _special_values()
    g = torch.Generator().manual_seed(1)
    src = torch.rand(shape, generator=g) * 1.5 - 0.25
    n = min(src.numel(), vals.numel())
    off = 0 if C == 3 else 630                   # the two sources together hold every special value
    chunk = vals[off:off + n] if off < vals.numel() else vals[:0]
    src.view(-1)[:chunk.numel()] = chunk
    TH, TW = h + 2 * pad, w + 2 * pad
    kw = dict(x0=x0, y0=1, xstep=TW + 1)
    PH, PW = TH + 3, x0 + T * (TW + 1) + 2
    buf, panel = VR.guarded_panel((b, C, PH, PW), dev, guard)
    ops.panel_image(src.to(dev), panel, ops.tile_place(panel, T, **kw), pad, 204)
    tiles = VR.to_u8(F.pad(src.view(b, T, C, h, w), [pad] * 4, 'constant', 0.8).numpy())
    _check(buf, VR.paste(np.full((b, C, PH, PW), S, np.uint8), tiles, T, **kw), guard)


def test_float_tiles_cover_every_special_value():
    assert _special_values().numel() <= 6 * 3 * 5 * 7 + 4 * 1 * 6 * 16


def test_float_tile_of_one_channel(dev):
    """channel -1 of a four-channel source into a video panel (the `_lidar` layout)."""
    from muvo_amd import ops
    b, T, H, W = 2, 3, 4, 10
    src = torch.rand(b, T, 4, H, W) * 1.2 - 0.1
    buf, video = VR.guarded_panel((b, T, 1, 2 * H, W), dev)
    ops.panel_image(src.flatten(0, 1).to(dev), video, ops.tile_place(video, T, y0=H, ystep=2 * H), channel=-1)
    expect = np.full((b, T, 1, 2 * H, W), S, np.uint8)
    expect[:, :, 0, H:] = VR.to_u8(src[:, :, -1].numpy())
    _check(buf, expect, 64)


def _tied_logits(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.round(torch.randn(shape, generator=g) * 2) / 2            # steps of 0.5: plenty of equal maxima


@pytest.mark.parametrize('rotate', [False, True])
@pytest.mark.parametrize('C', [2, 8, 9, 16])
def test_logit_tiles(dev, C, rotate):
    from muvo_amd import ops
    from muvo_amd.visualise import BIRDVIEW_COLOURS
    b, T, h, w, pad = 2, 2, 6, 10, 2
    logits = _tied_logits((b, T, C, h, w), C)
    cls = torch.argmax(logits, dim=2)
    assert (logits == logits.max(dim=2, keepdim=True).values).sum(2).max() > 1, 'no tie in the input'
    tiles = VR.class_tiles(cls, BIRDVIEW_COLOURS, pad)
    if rotate:
        tiles = torch.rot90(tiles, k=1, dims=[3, 4])
    tiles = VR.to_u8(tiles.numpy())
    TH, TW = tiles.shape[-2:]
    assert (TH, TW) == ((w + 4, h + 4) if rotate else (h + 4, w + 4))
    kw = dict(t0=1, x0=1, y0=2, xstep=TW, tsep=2, sepw=3)
    PH, PW = TH + 4, 1 + 3 * TW + 3 + 1
    buf, panel = VR.guarded_panel((b, 3, PH, PW), dev)
    ops.panel_classes(logits.flatten(0, 1).to(dev), _pal(BIRDVIEW_COLOURS, dev), panel, ops.tile_place(panel, T, **kw), pad, 204, rotate)
    _check(buf, VR.paste(np.full((b, 3, PH, PW), S, np.uint8), tiles, T, **kw), 64)


@pytest.mark.parametrize('rotate', [False, True])
@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64])
def test_label_tiles(dev, dtype, rotate):
    from muvo_amd import ops
    from muvo_amd.visualise import VOXEL_COLOURS
    b, T, h, w, pad = 2, 3, 6, 10, 3
    g = torch.Generator().manual_seed(4)
    cls = torch.randint(0, 256, (b, T, h, w), generator=g)              # far past the two entries of the table
    cls[0, 0, 0, :4] = torch.tensor([0, 1, 2, 255])
    if dtype == torch.int64:
        cls[1, 2, 5, :3] = torch.tensor([256 + 7, -1, 1 << 40])          # the low byte counts
    cls = cls.to(dtype)
    tiles = VR.class_tiles(cls, VOXEL_COLOURS, pad)
    if rotate:
        tiles = torch.rot90(tiles, k=1, dims=[3, 4])
    tiles = VR.to_u8(tiles.numpy())
    TH, TW = tiles.shape[-2:]
    kw = dict(ystep=TH, x0=2)                                            # one column of tiles, like `_lidar_seg`
    PH, PW = T * TH, TW + 5
    buf, panel = VR.guarded_panel((b, 3, PH, PW), dev, 5)
    ops.panel_classes(cls.flatten(0, 1).to(dev), _pal(VOXEL_COLOURS, dev), panel, ops.tile_place(panel, T, **kw), pad, 204, rotate)
    _check(buf, VR.paste(np.full((b, 3, PH, PW), S, np.uint8), tiles, T, **kw), 5)


def test_constant_tiles(dev):
    from muvo_amd import ops
    b, T, h, w, pad = 2, 2, 3, 5, 2
    kw = dict(x0=3, xstep=w + 2 * pad)
    buf, panel = VR.guarded_panel((b, 3, h + 2 * pad + 1, 3 + T * (w + 2 * pad)), dev, 7)
    ops.panel_fill(b * T, h, w, 255, panel, ops.tile_place(panel, T, **kw), pad, 51)
    tiles = np.full((b, T, 3, h + 2 * pad, w + 2 * pad), 51, np.uint8)
    tiles[..., pad:-pad, pad:-pad] = 255
    _check(buf, VR.paste(np.full(tuple(panel.shape), S, np.uint8), tiles, T, **kw), 7)


def _scatter_frames():
    """(2, 2, 4, 4, 64): points on and next to every bound, ranges of zero and below, a crowded pixel, an empty frame."""
    g = torch.Generator().manual_seed(11)
    rv = torch.randn(2, 2, 4, 4, 64, generator=g) * 0.6
    rv[:, :, 3] = torch.rand(2, 2, 4, 64, generator=g) - 0.3
    edge = torch.tensor([1.0, -1.0, 0.999, -0.999, 0.995, -0.995, 0.25, 0.25])
    rv[0, 0, 0, 0, :8], rv[0, 0, 1, 0, :8], rv[0, 0, 3, 0, :8] = edge, 0.3, 0.5         # r on / next to the bounds, c inside
    rv[0, 0, 0, 1, :8], rv[0, 0, 1, 1, :8], rv[0, 0, 3, 1, :8] = -0.3, edge, 0.5        # c on / next to the bounds, r inside
    rv[0, 1, 0, 2, :20], rv[0, 1, 1, 2, :20], rv[0, 1, 3, 2, :20] = 0.1234, -0.4321, 0.7  # twenty points on one pixel
    rv[0, 1, 3, 3, :4] = torch.tensor([0.0, -0.0, -0.5, 1e-30])
    rv[0, 1, 0, 3, :4], rv[0, 1, 1, 3, :4] = 0.5, -0.5
    rv[1, 1, 3] = -rv[1, 1, 3].abs()                                                    # an empty frame
    return rv


def test_scatter_inputs_hit_the_edges():
    rv = _scatter_frames().numpy()
    for ch in (0, 1):
        r = (-(rv[0, 0, ch] * np.float32(50))) * np.float32(2.56) + np.float32(128)
        assert (r == 0).any() and (r == 256).any() and ((r > 0) & (r < 1)).any() and ((r > 255) & (r < 256)).any(), ch
    assert (rv[0, 1, 3] == 0).any() and (rv[0, 1, 3] < 0).any() and not (rv[1, 1, 3] > 0).any()
    image = VR.pcd_xy_image(torch.from_numpy(rv)).numpy()
    assert image[1, 1].sum() == 0 and image[0, 0].sum() > 0 and image[0, 1].sum() > 0


@pytest.mark.parametrize('guard', [64, 2])
def test_scatter(dev, guard):
    from muvo_amd import ops
    rv = _scatter_frames()
    b, T = rv.shape[:2]
    tiles = VR.to_u8(F.pad(VR.pcd_xy_image(rv), [2] * 4, 'constant', 0.2).numpy())
    kw = dict(x0=1, xstep=261)
    buf, panel = VR.guarded_panel((b, 3, 261, 1 + T * 261), dev, guard)
    ops.panel_scatter(rv.flatten(0, 1).to(dev), 50.0, panel, ops.tile_place(panel, T, **kw), 2, 51)
    _check(buf, VR.paste(np.full(tuple(panel.shape), S, np.uint8), tiles, T, **kw), guard)


@pytest.mark.parametrize('w', [7, 832])
@pytest.mark.parametrize('kind', [0, 1])
def test_bars(dev, w, kind):
    from muvo_amd import ops
    h = 48
    values = torch.tensor([0.0, -0.0, 1e-4, 0.5, -0.5, 1.0, -1.0]).view(1, 7, 1)
    tiles = VR.to_u8(VR.bars(values, kind, h, w).numpy())
    assert tiles.shape == (1, 7, 3, 12, w + 10) and (tiles != 255).any()
    kw = dict(xstep=w + 10, y0=1)
    buf, panel = VR.guarded_panel((1, 3, 14, 7 * (w + 10)), dev, 6)
    ops.panel_bars(values.to(dev), kind, h, w, panel, ops.tile_place(panel, 7, **kw))
    _check(buf, VR.paste(np.full(tuple(panel.shape), S, np.uint8), tiles, 7, **kw), 6)


def _voxel_logits(b, T, C, X, Y, Z, seed):
    logits = _tied_logits((b, T, C, X, Y, Z), seed)
    logits[:, :, 0, 0, :, :] += 50.0                  # x = 0: empty columns
    logits[:, :, 0, X - 1, :, 1:] += 50.0             # x = X - 1: nothing above z = 0 ...
    logits[:, :, 1, X - 1, :, 0] += 100.0             # ... and z = 0 occupied
    return logits


@pytest.mark.parametrize('grid', [(5, 7, 3), (6, 10, 50), (4, 4, 64), (3, 5, 1), (2, 3, 300)])
@pytest.mark.parametrize('C', [0, 2, 9])
def test_voxel_top(dev, grid, C):
    """C = 0: a uint8 class grid; otherwise logits of C classes."""
    from muvo_amd import ops
    from muvo_amd.visualise import VOXEL_COLOURS
    X, Y, Z = grid
    b, T = 2, 2
    if C:
        src = _voxel_logits(b, T, C, X, Y, Z, X + C)
        cls = torch.argmax(src, dim=2)
        if Z > 1:
            assert (cls[:, :, 0] == 0).all() and (cls[:, :, X - 1, :, 0] == 1).all() and (cls[:, :, X - 1, :, 1:] == 0).all()
    else:
        g = torch.Generator().manual_seed(Z)
        src = torch.randint(0, 256, (b, T, X, Y, Z), generator=g) * (torch.rand(b, T, X, Y, Z, generator=g) < 0.2)
        src[:, :, 0] = 0
        src[:, :, X - 1, :, 1:] = 0
        src[:, :, X - 1, :, 0] = 3
        src = cls = src.to(torch.uint8)
    tiles = F.pad(torch.from_numpy(VR.voxel_top_tiles(cls.numpy(), VOXEL_COLOURS)), [2] * 4, 'constant', 204).numpy()
    TH, TW = X + 4, Y + 4
    kw = dict(x0=1, xstep=TW, y0=TH, t0=0)
    buf, panel = VR.guarded_panel((b, 3, 2 * TH + 1, 1 + T * TW + 2), dev, 9)
    ops.panel_voxel_top(src.flatten(0, 1).to(dev), _pal(VOXEL_COLOURS, dev), panel, ops.tile_place(panel, T, **kw), 2, 204)
    _check(buf, VR.paste(np.full(tuple(panel.shape), S, np.uint8), tiles, T, **kw), 9)


def test_a_tile_outside_the_panel_is_refused(dev):
    """The entry points check every tile against the panel before they launch anything."""
    from muvo_amd import ops
    buf, panel = VR.guarded_panel((1, 3, 8, 20), dev)
    src = torch.zeros(2, 3, 4, 6, device=dev)
    for kw in (dict(xstep=15), dict(y0=5), dict(x0=-1), dict(xstep=10, tsep=1, sepw=5)):
        with pytest.raises(RuntimeError, match='leaves the'):
            ops.panel_image(src, panel, ops.tile_place(panel, 2, **kw), 0, 0)
    with pytest.raises(RuntimeError, match='too small'):
        place = ops.tile_place(panel, 2, xstep=10)
        place.sample_stride *= 2
        ops.panel_image(src.repeat(2, 1, 1, 1), panel, place, 0, 0)
    torch.cuda.synchronize()
    assert (buf == S).all()
