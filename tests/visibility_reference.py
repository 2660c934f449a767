"""The sensor-visibility mask of include/muvo_hip.h (muvo_visibility_mark / muvo_visibility_apply) restated in numpy.  Helpers only:
no fixtures, no tests.  The walk is raycast_reference.march itself, not a copy: it is handed a grid that records every cell the
march tests for occupancy - the cells it visits, up to and including the first occupied one.  `seen_table` does the same for all
rays of a table at once on render_reference.cell_table, the vectorised form of that walk (tests/test_render_reference.py holds
the two against each other cell by cell; tests/test_visibility_reference.py holds seen_table against seen_grid)."""
import numpy as np

import raycast_reference as RC
import render_reference as RR

f32 = np.float32


class _Recorder:
    """a grid for RC.march: indexing it returns the class of the cell and remembers that the cell was asked for"""

    def __init__(self, grid):
        self.grid, self.shape, self.cells = grid, grid.shape, []

    def __getitem__(self, c):
        self.cells.append(tuple(int(v) for v in c))
        return self.grid[c]


def visited(grid, ray):
    """[(x, y, z)] in order: the cells one ray (7 float32) marks in grid (X, Y, Z) uint8; [] for a ray that is a miss before step 2"""
    rec = _Recorder(grid)
    RC.march(rec, np.asarray(ray, f32))
    return rec.cells


def seen_grid(grid, rays):
    """(X, Y, Z) bool: the cells the rays (R, 7) mark in one grid, ray by ray through RC.march"""
    seen = np.zeros(grid.shape, bool)
    for ray in np.asarray(rays, f32):
        for c in visited(grid, ray):
            seen[c] = True
    return seen


def seen_table(grid, rays, table=None):
    """seen_grid for a whole table at once; `table` = RR.cell_table(grid.shape, rays) may be shared between the frames of one size"""
    table = RR.cell_table(grid.shape, rays) if table is None else table
    cells = table['cells']                                       # (R, nmax), -1 behind the end
    flat = grid.reshape(-1)
    occupied = (cells >= 0) & (flat[np.maximum(cells, 0)] != 0)
    before = np.cumsum(occupied, axis=1) - occupied               # occupied cells strictly before this one
    marked = (cells >= 0) & (before == 0)
    seen = np.zeros(flat.shape, bool)
    seen[cells[marked]] = True
    return seen.reshape(grid.shape)


def masked(label, seen):
    """(masked label uint8, counts [free and seen, unknown]) of one frame or a stack of frames"""
    free = label == 0
    out = np.where(free, np.where(seen, 0, 255), label).astype(np.uint8)
    return out, np.array([int((free & seen).sum()), int((free & ~seen).sum())], np.int64)


def pack_seen(seen):
    """the SEEN words of one frame: layout and bit order of RC.pack_bricks"""
    return RC.pack_bricks(seen.astype(np.uint8))


def unpack_seen(words, shape):
    """(X, Y, Z) bool from the words of one frame (uint64 or the int64 the device tensors hold)"""
    X, Y, Z = shape
    BY, BZ = (Y + 3) // 4, (Z + 3) // 4
    w = np.asarray(words).astype(np.uint64)
    x, y, z = np.indices(shape)
    return ((w[((x >> 2) * BY + (y >> 2)) * BZ + (z >> 2)] >> ((x & 3) * 16 + (y & 3) * 4 + (z & 3)).astype(np.uint64)) & np.uint64(1)).astype(bool)


# ---- the inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------
def edge_grid(shape, seed):
    """~8 % occupied cells of classes 1..8 and a partial floor"""
    rng = np.random.default_rng(seed)
    g = (rng.random(shape) < 0.08) * rng.integers(1, 9, shape)
    g[:, :, 0] = np.where(rng.random(shape[:2]) < 0.5, 1, g[:, :, 0])
    return g.astype(np.uint8)


def edge_rays(grid):
    """the ray table of the edge cases for one grid: [(name, ray)]"""
    X, Y, Z = grid.shape
    inf, nan = np.inf, np.nan
    occ = [tuple(int(v) for v in c) for c in np.argwhere(grid != 0)]
    ox, oy, oz = occ[len(occ) // 2]
    rays = [
        ('inside, oblique', [1.3, 2.2, 1.6, 0.7, 0.5, 0.3, inf]),
        ('inside, all negative', [X - 0.4, Y - 0.7, Z - 0.2, -1.0, -0.7, -0.45, inf]),
        ('outside, entering through x', [-3.0, Y / 2 + 0.1, Z / 2 + 0.2, 1.0, 0.1, -0.05, inf]),
        ('outside, entering from above', [X / 2 + 0.3, Y / 2 - 0.2, Z + 4.0, 0.05, 0.1, -1.0, inf]),
        ('axis-parallel +x, d_y = d_z = 0', [0.25, 1.5, Z - 0.5, 1, 0, 0, inf]),
        ('axis-parallel -y from outside', [2.5, Y + 2.0, 1.5, 0, -1, 0, inf]),
        ('axis-parallel -z down a column', [X - 0.5, 0.5, Z + 1.0, 0, 0, -1, inf]),
        ('axis-parallel outside the box', [2.5, Y + 0.5, 9.0, 0, 0, -1, inf]),
        ('plane ray, d_z = 0', [0.5, 0.25, 2.5, 1, 1, 0, inf]),
        ('exact corner crossings, ties x before y before z', [0, 0, 0, 1, 1, 1, inf]),
        ('corner crossings in a plane', [1, 1, 1.5, 1, 1, 0, inf]),
        ('corner crossings backwards', [X, Y, Z, -1, -1, -1, inf]),
        ('along a cell face', [0.0, 2.0, 3.0, 1, 0, 0, inf]),
        ('a clean miss', [-3.0, -3.0, Z + 20.0, -1, 0, 0.5, inf]),
        ('NaN direction', [2.5, 3.5, 2.0, nan, 0, -1, inf]),
        ('NaN origin', [nan, 3.5, 3.5, 1, 0, 0, inf]),
        ('NaN tmax', [2.5, 3.5, 2.0, 0, 0, -1, nan]),
        ('infinite direction component', [2.5, 3.5, 2.0, 0, 0, -inf, inf]),
        ('infinite origin', [inf, 3.5, 2.0, -1, 0, 0, inf]),
        ('zero direction', [2.5, 2.5, 2.5, 0, 0, 0, inf]),
        ('start cell occupied', [ox + 0.5, oy + 0.25, oz + 0.75, 0.3, -0.2, 0.1, inf]),
        ('finite tmax ends mid-grid', [0.5, 0.6, Z - 0.3, 1.0, 0.8, -0.1, 2.75]),
        ('tmax 0', [1.5, 1.5, 1.5, 1, 0, 0, 0.0]),
        ('negative tmax', [1.5, 1.5, 1.5, 1, 0, 0, -1.0]),
    ]
    fan = RC.fan_rays((X / 2 + 0.25, Y / 2 - 0.3, Z / 2 + 0.1), 6, 24, 40.0, -60.0)
    return rays + [(f'fan {k}', list(r)) for k, r in enumerate(fan)]


CROWD_RAY = [0.3, 0.4, 0.2, 0.9, 0.8, 0.6, np.inf]               # 4 096 copies: all atomics of a wave land on one word
CROWD = 4096


def edge_table(grid):
    return np.concatenate([np.array([r for _, r in edge_rays(grid)], f32), np.tile(np.array(CROWD_RAY, f32), (CROWD, 1))])


def base_grid(frames=2, shape=(192, 192, 64), seed=5):
    """(F, X, Y, Z) uint8 in the manner of muvo_amd/data/synthetic.py - 10 % of the cells occupied at random - plus one solid wall
    across the grid in front of the sensors (x = 120).  Rays end after ~10 cells in such a grid, so every frame but the first
    has 0.2 % of its cells occupied instead and a floor at z = 0: long walks, a shadow behind the wall."""
    rng = np.random.default_rng(seed)
    share = np.array([0.1] + [0.002] * (frames - 1)).reshape(-1, 1, 1, 1)
    g = ((rng.random((frames, *shape)) < share) * rng.integers(1, 9, (frames, *shape))).astype(np.uint8)
    g[1:, :, :, 0] = 1
    g[:, min(120, shape[0] - 1)] = 3
    return g
