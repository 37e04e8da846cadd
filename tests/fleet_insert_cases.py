"""Cases of the fleet inserter (rgrid_batch_insert_* of include/rgrid.h, ScanMatchFleet.insert), shared by
tests/test_fleet_insert_cpu.py and tests/test_fleet_insert_gpu.py.  Built on tests/grid_cases.py and on the scenes of
tests/test_grid_gpu.py's inserter tests, by their own construction.

A grid here is ``(cells, resolution, max_xy)``; a scan is ``(grid_slot, origin_xy, returns_xy, misses_xy_or_None)`` as
``ScanMatchFleet.submit_insert`` takes it.  The specification of a scan's result is the pair GrowAsNeeded + Insert: ``oracle_pair``
gives it from the CPU oracle, ``handle_pair`` from a GridFrontEnd.  Every comparison is exact.
"""
from __future__ import annotations

import math

import numpy as np

from tests.grid_cases import room_grid, scan_of

OK, INVALID, CAPACITY = 0, -1, -4
WG_WAVES = 16                       # kgb_insert: 1024 threads; its waves stride over the rays, its threads over the end points

# (n_returns, n_misses) of the shape sweep: nothing at all, one ray of either kind, returns on both sides of a wave (64), ray
# counts on both sides of the workgroup's wave count and more end points than the workgroup has threads
SHAPE_COUNTS = ((0, 0), (1, 0), (0, 1), (63, 5), (64, 0), (65, 60), (300, 1), (1500, 60))
SHAPE_RES, SHAPE_N, SHAPE_MAX_XY = 0.1, 120, (6.0, 6.0)


def known_grid(rng, ny, nx):
    """A finished grid with known and unknown cells (test_grow_as_needed_matches_oracle_...'s construction)."""
    g = rng.integers(1, 32767, (ny, nx)).astype(np.uint16)
    g[rng.random((ny, nx)) < 0.3] = 0
    return g


def cell_of(grid, point):
    """(row, column) of a point's cell: MapLimits::GetCellIndex (map_limits.h:47-55)."""
    _, res, max_xy = grid
    return int(np.rint((max_xy[0] - point[0]) / res - 0.5)), int(np.rint((max_xy[1] - point[1]) / res - 0.5))


def limits_of(cells, res, max_xy):
    """What GetLimits returns for a grid."""
    return (cells.shape[1], cells.shape[0], float(res), float(max_xy[0]), float(max_xy[1]))


def option_values(options=None):
    """(hit_probability, miss_probability, insert_free_space) of a RangeDataInserterOptions (None: the defaults)."""
    return (0.55, 0.49, True) if options is None else (options.hit_probability, options.miss_probability, options.insert_free_space)


def oracle_pair(grid, scan, options=None):
    """GrowAsNeeded + Insert in the oracle -> (cells, limits tuple)."""
    from oracle.binding import oracle_grow, oracle_insert
    cells, res, max_xy = grid
    _, origin, ret, mis = scan
    grown, new_max, _ = oracle_grow(cells, res, max_xy, origin, ret, mis)
    out = oracle_insert(grown, res, new_max, origin, ret, mis, *option_values(options))
    return out, limits_of(out, res, new_max)


def handle_pair(gf, grid, scan, options=None):
    """GrowAsNeeded + Insert on a GridFrontEnd holding `grid` -> (status, cells, limits): the first code of the pair that is not OK."""
    from reflector_ekf_slam_amd.grid import RgridError
    cells, res, max_xy = grid
    _, origin, ret, mis = scan
    gf.SetGrid(cells, res, max_xy)
    status = OK
    try:
        gf.Insert(origin, ret, mis, options)
    except RgridError as e:
        status = e.code
    lim = gf.GetLimits()
    gf._grid_shape = (lim[1], lim[0])
    return status, gf.GetGrid(), lim


_shape = None


def shape_case():
    """-> (eight grids, eight scans, scan k into slot k): SHAPE_COUNTS from different origins, everything inside the grid; every
    other slot starts unknown, the others with known cells."""
    global _shape
    if _shape is None:
        rng = np.random.default_rng(301)
        grids, scans = [], []
        for k, (nr, nm) in enumerate(SHAPE_COUNTS):
            cells = np.zeros((SHAPE_N, SHAPE_N), np.uint16) if k % 2 == 0 else known_grid(rng, SHAPE_N, SHAPE_N)
            origin = rng.uniform(-4.0, 4.0, 2).astype(np.float32)
            ret = rng.uniform(-5.9, 5.9, (nr, 2)).astype(np.float32)
            mis = rng.uniform(-5.9, 5.9, (nm, 2)).astype(np.float32)
            grids.append((cells, SHAPE_RES, SHAPE_MAX_XY))
            scans.append((k, origin, ret, mis if nm else None))
        _shape = (grids, scans)
    return _shape


def corner_case():
    """The three origins of test_insert_exact_corner_crossings and its half-cell case -> (four grids, four scans)."""
    res, n, max_xy = 0.1, 120, (6.0, 6.0)
    cells = np.zeros((n, n), np.uint16)
    k = np.arange(-12, 13)
    gx, gy = np.meshgrid(k, k, indexing="ij")
    scans = []
    for slot, origin_cell in enumerate(((60, 60), (30, 75), (90, 20))):
        ox, oy = max_xy[0] - (origin_cell[0] + 0.5) * res, max_xy[1] - (origin_cell[1] + 0.5) * res
        ret = np.stack([ox + gx.ravel() * res, oy + gy.ravel() * res], 1).astype(np.float32)
        scans.append((slot, np.array([ox, oy], np.float32), ret[:300], ret[300:]))
    ox, oy = max_xy[0] - 60 * res, max_xy[1] - 60 * res
    ret = np.stack([ox + (gx.ravel() + 0.5) * res, oy + gy.ravel() * res], 1).astype(np.float32)
    scans.append((3, np.array([ox, oy], np.float32), ret, None))
    return [(cells, res, max_xy)] * 4, scans


GROW_SHAPES = ((40, 40), (33, 57))
GROW_FAR = ((0.9, 0.8), (2.2, 0.4), (-1.9, 0.2), (0.1, -6.5), (0.2, 7.9))
GROW_MAX_CELLS = 64 * 33 * 57       # 8 x growth per side of the larger grid (the smaller one needs 64 * 40 * 40)


def growth_case():
    """The two grids and five scans each of test_grow_as_needed_matches_oracle_and_insert_continues_on_the_grown_grid ->
    [(grid, [scan])], slot = position."""
    out = []
    for slot, (ny, nx) in enumerate(GROW_SHAPES):
        rng = np.random.default_rng(nx)
        ref = known_grid(rng, ny, nx)
        origin = np.array([0.3, 0.5], np.float32)
        scans = []
        for far in GROW_FAR:
            ang = rng.uniform(-math.pi, math.pi, 200)
            rad = rng.uniform(0.05, 0.4, 200)
            ret = np.stack([origin[0] + rad * np.cos(ang), origin[1] + rad * np.sin(ang)], 1).astype(np.float32)
            ret[0] = far
            mis = np.array([[far[0] * 0.5, far[1] * 0.5]], np.float32)
            scans.append((slot, origin, ret, mis))
        out.append(((ref, 0.05, (1.0, 1.4)), scans))
    return out


STATUS_N, STATUS_RES, STATUS_MAX_XY = 64, 0.1, (3.2, 3.2)
STATUS_MAX_POINTS = 256
STATUS_MAX_CELLS = 4 * STATUS_N * STATUS_N          # one doubling fits, a second does not


def status_case():
    """-> (six grids, six scans, the statuses they must get): growth beyond max_cells, a NaN coordinate, more returns than
    max_points inside the grid, more returns than max_points that also leave the grid (the pair grows, then refuses), and two
    ordinary scans, the second of which grows once."""
    rng = np.random.default_rng(404)
    grids = [(known_grid(rng, STATUS_N, STATUS_N), STATUS_RES, STATUS_MAX_XY) for _ in range(6)]
    inside = lambda n: rng.uniform(-3.0, 3.0, (n, 2)).astype(np.float32)
    org = lambda: rng.uniform(-2.0, 2.0, 2).astype(np.float32)
    too_far = inside(50); too_far[7] = (100.0, 0.0)
    nan = inside(50); nan[49, 1] = np.nan
    many = inside(STATUS_MAX_POINTS + 1)
    many_out = inside(STATUS_MAX_POINTS + 1); many_out[3] = (4.5, -1.0)
    grows = inside(120); grows[0] = (-5.0, 2.0)
    scans = [(0, org(), too_far, inside(4)), (1, org(), nan, None), (2, org(), many, None), (3, org(), many_out, inside(3)),
             (4, org(), inside(200), inside(20)), (5, org(), grows, inside(9))]
    return grids, scans, [CAPACITY, INVALID, CAPACITY, CAPACITY, OK, OK]


CROWD, CROWD_N = 300, 64


def crowd_case():
    """More workgroups than an MI355X has compute units: -> (CROWD grids of 64 x 64 cells, CROWD scans of 100 to 200 returns)."""
    rng = np.random.default_rng(707)
    grids, scans = [], []
    for k in range(CROWD):
        cells = np.zeros((CROWD_N, CROWD_N), np.uint16) if k % 3 else known_grid(rng, CROWD_N, CROWD_N)
        grids.append((cells, 0.1, (3.2, 3.2)))
        n = int(rng.integers(100, 201))
        scans.append((k, rng.uniform(-2.5, 2.5, 2).astype(np.float32), rng.uniform(-3.1, 3.1, (n, 2)).astype(np.float32),
                      rng.uniform(-3.1, 3.1, (k % 4, 2)).astype(np.float32) if k % 4 else None))
    return grids, scans


def map_scene():
    """The three insertions of test_insert_matches_oracle_cell_for_cell_and_feeds_the_matcher and its match ->
    (max_xy, [(origin, returns, misses)], (prediction, points))."""
    _, max_xy, occ = room_grid()
    rng = np.random.default_rng(21)
    inserts = []
    for k, pose in enumerate(((0.5, 0.3, 0.2), (1.5, -0.8, 1.1), (-2.0, 1.0, -2.0))):
        loc = scan_of(occ, pose, n_points=1500, seed=40 + k)
        c, s = math.cos(pose[2]), math.sin(pose[2])
        world = np.stack([pose[0] + c * loc[:, 0] - s * loc[:, 1], pose[1] + s * loc[:, 0] + c * loc[:, 1]], 1).astype(np.float32)
        ang = rng.uniform(-math.pi, math.pi, 60)
        misses = np.stack([pose[0] + 5.0 * np.cos(ang), pose[1] + 3.5 * np.sin(ang)], 1).astype(np.float32)
        inserts.append((np.array(pose[:2], np.float32), world, misses))
    true = np.array([0.2, 0.1, 0.4])
    pts = scan_of(occ, true, n_points=600, seed=77)
    return max_xy, inserts, (true + [0.1, 0.05, 0.05], pts)
