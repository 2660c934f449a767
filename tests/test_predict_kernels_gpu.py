"""-m gpu: the export kernels of muvo_amd/csrc/export.hip, bit-exact against the host route of the reference's sim_run.py:75-92 -
`torch.where(torch.argmax(logits, 1) != 0)` plus the class at those positions for the occupied-voxel rows,
`(x * np.float32(255)).astype(np.uint8)` for the image bytes (and the stated saturation rule outside numpy's defined range)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 2048                                   # ops.VOXEL_ROWS_CHUNK, asserted below
# (F, C, X, Y, Z): below one chunk with odd sizes | exactly K voxels, 9 classes | across chunks with a ragged tail, V % 4 != 0 (no
# wide loads) | many chunks | V % 4 == 0 with a ragged last chunk (wide loads next to the bound) | axes of extent 1
SHAPES = [(3, 2, 5, 7, 3), (2, 9, 16, 16, 8), (2, 2, 33, 31, 5), (1, 2, 48, 48, 16), (2, 3, 6, 10, 50), (2, 2, 2100, 1, 1)]
VARIANTS = ['random', 'empty_first', 'full_last', 'ties', 'straddle']


def _logits(shape, variant):
    F, C, X, Y, Z = shape
    V = X * Y * Z
    g = torch.Generator().manual_seed(F * 1000003 + C * 1009 + V)
    lg = torch.randn(F, C, V, generator=g)
    lg[:, 0] += 0.4 + 0.9 * torch.arange(F).view(F, 1)              # a different number of occupied voxels in every frame
    if variant == 'empty_first':
        lg[0, 0] = 50.0
    elif variant == 'full_last':
        lg[F - 1, 0] = -50.0
    elif variant == 'ties':
        for lo in (0, max(0, min(V, K) - 20)):                     # the first voxels, and a stretch across the first chunk boundary
            lg[:, :, lo:lo + 40] = 0.25                             # all classes equal -> class 0 -> no row
        if C >= 6:
            lg[:, :, 50:90] = torch.randn(F, C, 40, generator=g).clamp(max=1.0)
            lg[:, 3, 50:90] = 2.5                                   # classes 3 and 5 equal and largest -> 3
            lg[:, 5, 50:90] = 2.5
        lg[:, 0, 95:100] = -9.0
        lg[:, 1:, 95:100] = 1.5                                     # classes 1 .. C-1 equal and largest -> 1
    elif variant == 'straddle':
        lg[:, 0] = 50.0                                             # occupied only in runs across every chunk boundary (and the ends)
        for edge in range(0, V + K, K):
            lo, hi = max(0, edge - 11 - edge // K), min(V, edge + 9)
            if lo < hi:
                lg[:, 0, lo:hi] = -50.0
    return lg.view(F, C, X, Y, Z).contiguous()


_CASES = {}


def case(shape, variant):
    """(logits on the host, expected rows (Q, 4) uint16, expected counts, argmax as uint8), computed once per (shape, variant)."""
    key = (shape, variant)
    if key not in _CASES:
        lg = _logits(shape, variant)
        am = torch.argmax(lg, 1)
        f, x, y, z = torch.where(am != 0)
        rows = torch.stack([x, y, z, am[f, x, y, z]], 1).numpy().astype(np.uint16)
        counts = torch.bincount(f, minlength=shape[0]).tolist()
        _CASES[key] = (lg, rows, counts, am.to(torch.uint8))
    return _CASES[key]


def _host(rows):
    return rows.cpu().numpy()


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES)
def test_rows_of_logits(dev, shape, variant):
    from muvo_amd import ops
    assert ops.VOXEL_ROWS_CHUNK == K
    lg, want, counts, _ = case(shape, variant)
    if variant == 'empty_first':
        assert counts[0] == 0
    if variant == 'full_last':
        assert counts[-1] == lg[0, 0].numel()
    if variant == 'ties' and shape[1] >= 6:
        assert (want[:, 3] == 3).sum() >= 40 * shape[0] and (want[:, 3] == 5).sum() > 0
    rows, got_counts = ops.voxel_rows(lg.to(dev))
    assert rows.dtype == torch.uint16 and rows.device == dev and tuple(rows.shape) == (sum(counts), 4)
    print(shape, variant, 'counts', got_counts, 'expected', counts)
    assert got_counts == counts
    assert np.array_equal(_host(rows), want)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]])
def test_rows_of_uint8_grid(dev, shape):
    from muvo_amd import ops
    for variant in ('random', 'empty_first', 'straddle'):
        _, want, counts, am = case(shape, variant)
        rows, got_counts = ops.voxel_rows(am.to(dev))
        assert got_counts == counts and np.array_equal(_host(rows), want), variant
    # any non-zero byte is a class of its own, 255 included
    g = torch.Generator().manual_seed(3)
    grid = torch.randint(0, 256, (shape[0], *shape[2:]), generator=g, dtype=torch.uint8)
    grid[torch.rand(grid.shape, generator=g) < 0.6] = 0
    f, x, y, z = torch.where(grid != 0)
    want = torch.stack([x, y, z, grid[f, x, y, z].long()], 1).numpy().astype(np.uint16)
    rows, got_counts = ops.voxel_rows(grid.to(dev))
    assert got_counts == torch.bincount(f, minlength=shape[0]).tolist() and np.array_equal(_host(rows), want)
    assert (want[:, 3] == 255).any()


@pytest.mark.parametrize('as_grid', [False, True])
def test_capacity_below_the_count(dev, as_grid):
    from muvo_amd import ops
    lg, want, counts, am = case(SHAPES[2], 'random')
    src = (am if as_grid else lg).to(dev)
    total, guard = sum(counts), 64
    assert counts[0] > 100 and counts[1] > 0
    for cap in (0, 1, counts[0] - 3, counts[0] + 5, total - 1, total):      # inside frame 0, across the frame edge, one short, exact
        buf = torch.full((cap + guard, 4), -21555, dtype=torch.int16, device=dev).view(torch.uint16)       # 0xABCD
        got = ops.voxel_rows_into(src, buf, cap=cap)
        assert got.dtype == torch.int64 and got.tolist() == counts, cap                # the true totals whatever the capacity
        host = _host(buf)
        assert np.array_equal(host[:cap], want[:cap]), cap
        assert (host[cap:] == 0xABCD).all(), cap
    with pytest.raises(RuntimeError, match='C = 17'):
        ops.voxel_rows(torch.zeros(1, 17, 2, 2, 2, device=dev))
    with pytest.raises(ValueError):
        ops.voxel_rows(torch.zeros(1, 2, 2, 2, device=dev))


def test_rows_round_trip_through_the_dense_grid_path(dev):
    """rows -> input_pipeline.voxel_grid (what the dataset makes of a recorded voxel file) -> the argmax grid again."""
    from muvo_amd import input_pipeline as IP
    from muvo_amd import ops
    shape = SHAPES[2]
    _, _, counts, am = case(shape, 'random')
    lg = case(shape, 'random')[0]
    rows, got_counts = ops.voxel_rows(lg.to(dev))
    assert got_counts == counts
    edges = np.concatenate([[0], np.cumsum(counts)])
    for f in range(shape[0]):
        mine = rows[edges[f]:edges[f + 1]].view(torch.int16).to(torch.int64) & 0xFFFF
        grid = IP.voxel_grid(mine, size=tuple(shape[2:]))
        assert grid.dtype == torch.uint8 and torch.equal(grid.cpu(), am[f])


def _want_bytes(x):
    return (x * np.float32(255)).astype(np.uint8)


def test_image_bytes_equal_numpy_cast(dev):
    from muvo_amd import ops
    exact = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    around = np.concatenate([np.nextafter(exact, np.float32(-np.inf)), np.nextafter(exact, np.float32(np.inf))])[1:]   # (not below 0)
    rnd = np.random.RandomState(0).rand(4099).astype(np.float32)
    for name, x in (('k/255', exact), ('ulp', around), ('random', rnd)):
        t = x * np.float32(255)
        assert (t >= 0).all() and (t < 256).all(), name                    # the range in which numpy's cast is defined
        got = ops.image_u8(torch.from_numpy(x).to(dev))
        assert got.dtype == torch.uint8 and got.shape == x.shape
        assert np.array_equal(got.cpu().numpy(), _want_bytes(x)), name
    assert np.array_equal(_want_bytes(exact), np.arange(256, dtype=np.uint8))
    whole = torch.from_numpy(rnd).to(dev)
    for n in (1, 3, 17, 4099):
        assert np.array_equal(ops.image_u8(whole[:n].clone()).cpu().numpy(), _want_bytes(rnd[:n])), n
        if n < 4099:                                                        # a start that is not 16-byte aligned
            assert np.array_equal(ops.image_u8(whole[1:1 + n]).cpu().numpy(), _want_bytes(rnd[1:1 + n])), n
    img = torch.from_numpy(rnd[:4095].reshape(3, 5, 273)).to(dev)          # a shape, kept
    assert np.array_equal(ops.image_u8(img).cpu().numpy(), _want_bytes(rnd[:4095]).reshape(3, 5, 273))


def test_image_bytes_saturate(dev):
    from muvo_amd import ops
    x = np.array([-0.5, 1.0, 1.5, np.inf, -np.inf, np.nan, -0.0, 256 / 255, 1e30, -1e30, 0.999], dtype=np.float32)
    want = np.array([0, 255, 255, 255, 0, 0, 0, 255, 255, 0, 254], dtype=np.uint8)
    for n in (len(x), 4, 3):                                                # the wide and the one-by-one form
        assert np.array_equal(ops.image_u8(torch.from_numpy(x[:n]).to(dev)).cpu().numpy(), want[:n]), n
