"""Cases of the grid's WRITE path -- GrowAsNeeded + ProbabilityGridRangeDataInserter2D::Insert: kg_ends / kg_hits / kg_rays /
kg_finish / kg_grow behind GridFrontEnd, kgb_insert behind ScanMatchFleet.insert -- shared by tests/test_grid_write_cpu.py and
tests/test_grid_write_gpu.py.  The specification is the pair grow_witness + insert_witness of tests/witness/grid_witness.py;
the CPU file holds oracle/grid_oracle.c to it, the GPU file the kernels.  Every comparison is exact.

A grid is ``(cells, resolution, max_xy)``, a scan ``(slot, origin_xy, returns_xy, misses_xy_or_None)`` as in
tests/fleet_insert_cases.py.  A CHAIN is one grid and the scans that go into it one after the other, each starting from the
previous one's result: ``NS(name, slot, grid, steps=[scan], options=[None or (hit, miss, insert_free_space)], grow)``; a chain's
position in its family is its grid slot in the fleet handle.  ``grow``: GrowAsNeeded runs before every Insert (elsewhere every
point is inside and nothing grows).

Families (``FAMILIES``; every builder is seeded and memoised, ``SIZES`` pins the number of chains and of scans):
  geometry  four maps with num_x_cells != num_y_cells and max.x != max.y and one square control, 70 % known cells, 200 returns +
            40 misses uniform inside: tells the convention (x index from world y and max.y, row from world x and max.x, rows
            num_x_cells apart) from its transpose (grid_witness.MUTANTS).
  counts    COUNTS on the 33 x 57 map: ray counts on both sides of kg_rays' 4 waves per workgroup, kgb_insert's 16 waves,
            kg_ends' 256 threads and kgb_insert's 1024 threads.
  thin      rays a few sub-pixels wide that cross a pixel border (X0 != X1 with |dx| <= 3: the closed form's two-column case with
            a_out, fdiv / cdiv at their narrowest), a zero-length ray.
  border    ends in the first and last sub-pixels of the grid and next to pixel borders, in both axes.
  ties      ends and origins exactly on cell borders, cell corners and cell centres at a resolution that is exact in binary:
            lround's ties in the cell index, rays through pixel corners (`sub_y == den`).
  long      corner-to-corner rays in all four directions, exactly axis-parallel rays, full-height rays that cross one
            pixel-column border (one column of more than 64 rows: the flattened pixel list exceeds one pass of 64 lanes), rays of
            more than 128 columns (three passes of 64 columns) on a non-square stride.
  options   three inserts into the same grid, then hits only with other probabilities, then the defaults again: the known-cell
            entries of both tables and the table switch.
  growth    old grids whose cell counts lie at and around kgb_insert's in-place chunk of 8192 cells; a far point beyond each
            side at one and at two doublings, beyond two opposite sides at once; a second growth from the grown grid.
  loop      three world scans of the room of tests/grid_cases.py inserted with growth into an unknown off-centre grid, then a
            correlative match on the map that came out.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from tests.fleet_insert_cases import known_grid, limits_of
from tests.grid_cases import room_grid, scan_of
from tests.witness import grid_witness as W

S = W.S
f32 = np.float32
HITS_ONLY = (0.7, 0.4, False)                   # (hit_probability, miss_probability, insert_free_space)
DEFAULTS = (0.55, 0.49, True)

# (ny, nx, resolution, max_xy)
GEOMETRY_MAPS = ((33, 57, 0.05, (1.0, 1.4)), (57, 33, 0.05, (-0.7, 2.3)), (150, 40, 0.1, (9.0, -3.0)), (40, 150, 0.1, (-2.0, 11.0)))
SQUARE_CONTROL = (120, 120, 0.1, (6.0, 6.0))
COUNTS = ((0, 0), (1, 0), (0, 1), (3, 0), (4, 0), (3, 2), (15, 0), (16, 0), (12, 5), (255, 0), (256, 0), (250, 7), (1023, 0),
          (1024, 0), (1020, 5), (1025, 0))
THIN_MAP = (40, 300, 0.05, (1.3, -2.0))
TIES_MAP = (24, 40, 0.25, (3.0, -1.0))
TIES_ORIGINS = ((1.0, -5.0), (1.125, -5.125))   # a cell corner, a cell centre
TIES_RETURNS = 1500
GROWTH_GRIDS = ((33, 57), (57, 33), (64, 128), (90, 91), (91, 91), (128, 129))          # (ny, nx)
GROWTH_RES = 0.05
GROWTH_MAX_XY = (1.0, 1.4)
GROWTH_MAX_CELLS = 16 * 128 * 129               # the largest old grid doubled twice; 64 * 33 * 57 (factor 8) is smaller
GROW_CHUNK = 8192                               # KGI_THREADS * KGI_GROW_PER of kgb_insert's in-place move
LOOP_GRID = (60, 100, 0.1, (2.0, 7.0))
LOOP_POSES = (((0.5, 0.3, 0.2), 4.0), ((-2.0, 1.0, -2.0), 8.0), ((1.5, -0.8, 1.1), 30.0))   # (pose, max_range): the map grows twice
LOOP_TRUE, LOOP_PREDICTION_OFFSET = (0.2, 0.1, 0.4), (0.1, 0.05, 0.05)
LOOP_MAX_CELLS = 16 * 60 * 100
MATCH_ANGULAR_WINDOW = math.radians(15.0)       # RealTimeCorrelativeScanMatcherOptions' default

# chains, scans per family
SIZES = {"geometry": (5, 5), "counts": (16, 16), "thin": (1, 1), "border": (1, 1), "ties": (2, 2), "long": (8, 8),
         "options": (4, 20), "growth": (58, 84),"loop": (1, 3)}


def chain(name, slot, grid, steps, options=None, grow=False):
    steps = [(slot, np.asarray(o, f32), np.asarray(r, f32).reshape(-1, 2), None if m is None else np.asarray(m, f32).reshape(-1, 2))
             for o, r, m in steps]
    return NS(name=name, slot=slot, grid=grid, steps=steps, options=list(options) if options else [None] * len(steps), grow=grow)


def world_of(grid_or_map, ix, iy):
    """World (x, y) float32 of the CENTRE of the sub-pixel with super-index (ix, iy): ix counts along world y from max.y."""
    res, max_xy = grid_or_map[-2], grid_or_map[-1]
    ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
    return np.stack([max_xy[0] - (iy + 0.5) * res / S, max_xy[1] - (ix + 0.5) * res / S], -1).astype(f32)


def super_of(grid, scan):
    """The witness' super-indices of a scan's points on `grid`: (origin, [(ix, iy)] of the returns then the misses)."""
    _, origin, ret, mis = scan
    idx = W.super_indices(grid[1], grid[2], origin, ret, mis)
    return idx[0], idx[1:]


def _uniform_inside(rng, m, n, margin=1e-3):
    ny, nx, res, (mx, my) = m
    return np.stack([rng.uniform(mx - ny * res + margin, mx - margin, n), rng.uniform(my - nx * res + margin, my - margin, n)], 1).astype(f32)


def _map_scan(rng, m, n_ret, n_miss):
    return (_uniform_inside(rng, m, 1)[0], _uniform_inside(rng, m, n_ret), _uniform_inside(rng, m, n_miss) if n_miss else None)


_memo = {}


def _memoised(fn):
    def get():
        if fn.__name__ not in _memo:
            _memo[fn.__name__] = fn()
        return _memo[fn.__name__]
    get.__name__, get.__doc__ = fn.__name__, fn.__doc__
    return get


@_memoised
def geometry():
    """The four non-square maps, then the square control."""
    out = []
    for slot, m in enumerate(GEOMETRY_MAPS + (SQUARE_CONTROL,)):
        rng = np.random.default_rng(1100 + slot)
        ny, nx, res, max_xy = m
        out.append(chain(f"geometry/{ny}x{nx}", slot, (known_grid(rng, ny, nx), res, max_xy), [_map_scan(rng, m, 200, 40)]))
    return out


@_memoised
def counts():
    m = GEOMETRY_MAPS[0]
    ny, nx, res, max_xy = m
    out = []
    for slot, (nr, nm) in enumerate(COUNTS):
        rng = np.random.default_rng(1200 + slot)
        cells = known_grid(rng, ny, nx) if slot % 2 else np.zeros((ny, nx), np.uint16)
        out.append(chain(f"counts/{nr}+{nm}", slot, (cells, res, max_xy), [_map_scan(rng, m, nr, nm)]))
    return out


THIN_ORIGIN = (150 * S + 999, 20 * S)           # the last sub-pixel of its pixel column, the first of its pixel row


@_memoised
def thin():
    ny, nx, res, max_xy = THIN_MAP
    rng = np.random.default_rng(1300)
    bx, by = THIN_ORIGIN
    ex_a, ey_a = bx + rng.integers(-3, 4, 200), rng.integers(0, ny * S, 200)        # thin in x, anywhere in y
    ex_b, ey_b = rng.integers(0, nx * S, 200), by + rng.integers(-3, 4, 200)        # anywhere in x, thin in y
    ret = world_of(THIN_MAP, np.append(ex_a, bx), np.append(ey_a, by))              # ... and the zero-length ray
    mis = world_of(THIN_MAP, ex_b, ey_b)
    return [chain("thin", 0, (known_grid(rng, ny, nx), res, max_xy), [(world_of(THIN_MAP, bx, by), ret, mis)])]


def border_values(n):
    return (0, 1, S - 1, S, n * S - 2, n * S - 1, (n - 1) * S)


@_memoised
def border():
    ny, nx, res, max_xy = THIN_MAP
    rng = np.random.default_rng(1400)
    ix, iy = np.meshgrid(border_values(nx), border_values(ny), indexing="ij")
    ends = world_of(THIN_MAP, ix.ravel(), iy.ravel())
    origin = world_of(THIN_MAP, 137 * S + 421, 17 * S + 333)
    return [chain("border", 0, (known_grid(rng, ny, nx), res, max_xy), [(origin, ends, ends[::-1])])]


@_memoised
def ties():
    ny, nx, res, (mx, my) = TIES_MAP
    i, j = np.meshgrid(np.arange(1, 2 * ny), np.arange(1, 2 * nx), indexing="ij")   # the half-cell lattice strictly inside
    nodes = np.stack([mx - i.ravel() * (res / 2), my - j.ravel() * (res / 2)], 1)
    assert np.array_equal(nodes.astype(f32).astype(np.float64), nodes)               # exact in float32
    out = []
    for slot, origin in enumerate(TIES_ORIGINS):
        rng = np.random.default_rng(1500 + slot)
        pts = nodes[rng.permutation(nodes.shape[0])]
        cells = known_grid(rng, ny, nx) if slot == 0 else np.zeros((ny, nx), np.uint16)
        out.append(chain(f"ties/origin{slot}", slot, (cells, res, (mx, my)), [(origin, pts[:TIES_RETURNS], pts[TIES_RETURNS:])]))
    return out


@_memoised
def long():
    """Per map and per corner cell: the origin in that cell, in the sub-pixel next to the cell's inner corner."""
    out = []
    for m in GEOMETRY_MAPS[2:]:
        ny, nx, res, max_xy = m
        for cx, cy in ((0, 0), (1, 0), (0, 1), (1, 1)):                             # the origin's corner: low / high x index, y index
            slot = len(out)
            rng = np.random.default_rng(1600 + slot)
            inward_x, inward_y = (1, -1)[cx], (1, -1)[cy]
            bx = (nx - 1) * S if cx else S - 1                                      # next to the border of the neighbouring column
            by = (ny - 1) * S if cy else S - 1
            far_x0, far_y0 = (0 if cx else (nx - 1) * S), (0 if cy else (ny - 1) * S)   # the opposite corner cell
            far_x, far_y = far_x0 + (S - 1 if not cx else 0), far_y0 + (S - 1 if not cy else 0)   # its outermost sub-pixel
            ends = [(far_x0 + a, far_y0 + b) for a, b in ((0, 0), (S - 1, S - 1), (S // 2, S // 2), (0, S - 1), (S - 1, 0))]
            ends += [(bx, far_y), (far_x, by)]                                      # dx == 0 and dy == 0 exactly
            thin_ends = [(bx + inward_x * d, far_y) for d in (1, 2, 3)]             # full height, crosses one pixel-column border
            thin_ends += [(far_x, by + inward_y * d) for d in (1, 2, 3)]            # full width, crosses one pixel-row border
            ret = world_of(m, *np.array(ends).T)
            mis = world_of(m, *np.array(thin_ends).T)
            cells = known_grid(rng, ny, nx) if slot % 2 else np.zeros((ny, nx), np.uint16)
            out.append(chain(f"long/{ny}x{nx}/corner{cx}{cy}", slot, (cells, res, max_xy), [(world_of(m, bx, by), ret, mis)]))
    return out


@_memoised
def options():
    out = []
    for slot, m in enumerate(GEOMETRY_MAPS):
        rng = np.random.default_rng(1700 + slot)
        ny, nx, res, max_xy = m
        steps = [_map_scan(rng, m, 120, 20) for _ in range(5)]
        out.append(chain(f"options/{ny}x{nx}", slot, (np.zeros((ny, nx), np.uint16), res, max_xy), steps,
                         options=[None, None, None, HITS_ONLY, None]))
    return out


def _growth_scan(rng, grid, far_points):
    """60 returns around an origin near the grid's middle, the far points among them, one miss half-way to the first far point."""
    cells, res, (mx, my) = grid
    ny, nx = cells.shape
    origin = np.array([mx - (0.5 * ny + 0.3) * res, my - (0.5 * nx - 0.2) * res])
    ang, rad = rng.uniform(-math.pi, math.pi, 60), rng.uniform(0.05, 0.4 * min(nx, ny) * res, 60)
    ret = np.stack([origin[0] + rad * np.cos(ang), origin[1] + rad * np.sin(ang)], 1)
    ret[:len(far_points)] = far_points
    return origin, ret, (origin + np.asarray(far_points[0])) / 2


def _beyond(grid, side, doublings):
    """A point beyond side 0..3 (x high, x low, y high, y low) of `grid` that needs exactly `doublings` doublings: k doublings
    push every side out by (2^k - 1) / 2 of the extent, so 0.25, 1.0 and 2.5 extents lie strictly between two steps."""
    cells, res, (mx, my) = grid
    ny, nx = cells.shape
    d = (0.25, 1.0, 2.5)[doublings - 1]
    x, y = mx - 0.37 * ny * res, my - 0.61 * nx * res                               # the other coordinate: inside
    return ((mx + d * ny * res, y), (mx - (1 + d) * ny * res, y), (x, my + d * nx * res), (x, my - (1 + d) * nx * res))[side]


def _after(grid, scan):
    """Limits of the grid after the scan's growth, the cells left open: the next scan of the chain is built from these."""
    grown, new_max, _ = W.grow_witness(grid[0], grid[1], grid[2], *scan)
    return (grown, grid[1], new_max)


@_memoised
def growth():
    """Per old grid nine chains: per side one doubling and then one more from the grown grid on the opposite side, per side two
    doublings at once, one scan beyond two opposite sides at once; on the two small grids one chain that reaches factor 8 in
    two scans (4, then 2) and one that reaches it in one."""
    out = []
    for g, (ny, nx) in enumerate(GROWTH_GRIDS):
        rng = np.random.default_rng(1800 + g)
        grid = (known_grid(rng, ny, nx), GROWTH_RES, GROWTH_MAX_XY)
        plans = [[(side, 1), (side ^ 1, 1)] for side in range(4)] + [[(side, 2)] for side in range(4)] + [[((2 * (g % 2), 2 * (g % 2) + 1), 1)]]
        if g < 2:
            plans += [[(g, 2), (3 - g, 1)], [(2 + g, 3)]]
        for plan in plans:
            steps, now = [], grid
            for sides, doublings in plan:
                far = [_beyond(now, s, doublings) for s in (sides if isinstance(sides, tuple) else (sides,))]
                steps.append(_growth_scan(rng, now, far))
                now = _after(now, steps[-1])
            tag = "+".join(f"side{''.join(map(str, s)) if isinstance(s, tuple) else s}x{2 ** d}" for s, d in plan)
            out.append(chain(f"growth/{ny}x{nx}/{tag}", len(out), grid, steps, grow=True))
    return out


@_memoised
def loop():
    ny, nx, res, max_xy = LOOP_GRID
    _, _, occ = room_grid(resolution=res, half=10.0)
    steps = []
    for k, (pose, max_range) in enumerate(LOOP_POSES):
        loc = scan_of(occ, pose, n_points=600, seed=1900 + k, max_range=max_range)
        c, s = math.cos(pose[2]), math.sin(pose[2])
        world = np.stack([pose[0] + c * loc[:, 0] - s * loc[:, 1], pose[1] + s * loc[:, 0] + c * loc[:, 1]], 1)
        steps.append((pose[:2], world, None))
    return [chain("loop", 0, (np.zeros((ny, nx), np.uint16), res, max_xy), steps, grow=True)]


def loop_match_scan():
    """(slot, prediction, points) of the fourth scan: matched on the map the loop built."""
    _, _, occ = room_grid(resolution=LOOP_GRID[2], half=10.0)
    true = np.array(LOOP_TRUE)
    return (0, true + LOOP_PREDICTION_OFFSET, scan_of(occ, true, n_points=600, seed=1977))


FAMILIES = {"geometry": geometry, "counts": counts, "thin": thin, "border": border, "ties": ties, "long": long, "options": options,
            "growth": growth, "loop": loop}


def max_cells_of(family):
    return {"growth": GROWTH_MAX_CELLS, "loop": LOOP_MAX_CELLS}.get(family, 150 * 150)


# ---- the specification: witness, and the oracle beside it -------------------------------------------------------------------
def _run(ch, grow_fn, insert_fn):
    """[(cells, limits, offset of the step's growth)] after every step of a chain."""
    cells, res, max_xy = ch.grid
    out = []
    for (_, origin, ret, mis), opt in zip(ch.steps, ch.options):
        offset = (0, 0)
        if ch.grow:
            cells, max_xy, offset = grow_fn(cells, res, max_xy, origin, ret, mis)
        cells = insert_fn(cells, res, max_xy, origin, ret, mis, *(opt or DEFAULTS))
        assert cells is not None, (ch.name, "a point outside the grid")
        out.append((cells, limits_of(cells, res, max_xy), tuple(offset)))
    return out


_witness = {}


def witness_chain(ch):
    """grow_witness + insert_witness along the chain; computed once and shared (do not write into the arrays)."""
    if ch.name not in _witness:
        _witness[ch.name] = _run(ch, W.grow_witness, W.insert_witness)
        for cells, _, _ in _witness[ch.name]:
            cells.setflags(write=False)
    return _witness[ch.name]


def oracle_chain(ch):
    from oracle.binding import oracle_grow, oracle_insert
    return _run(ch, oracle_grow, oracle_insert)


def grid_before(ch, k):
    """The grid step k of a chain starts from: the chain's own grid, or the witness' result of step k - 1."""
    if k == 0:
        return ch.grid
    cells, lim, _ = witness_chain(ch)[k - 1]
    return (cells, ch.grid[1], (lim[3], lim[4]))


def ray_shapes(grid, scan):
    """Per ray (origin -> every return and miss) from the witness' own pixels: (X0 != X1, |dx| in sub-pixels, number of pixel
    columns, most rows in one column)."""
    (bx, by), ends = super_of(grid, scan)
    out = []
    for ex, ey in ends:
        px = W.ray_pixels(bx, by, ex, ey)
        cols = {}
        for x, y in px:
            cols.setdefault(x, set()).add(y)
        out.append((bx // S != ex // S, abs(ex - bx), len(cols), max(len(v) for v in cols.values())))
    return out


def diff_report(name, got, want):
    """What an assertion says about two grids that differ: the case, how many cells, their bounding box."""
    if got.shape != want.shape:
        return f"{name}: shape {got.shape} != {want.shape}"
    rows, cols = np.nonzero(got != want)
    if rows.size == 0:
        return f"{name}: equal"
    return f"{name}: {rows.size} cells differ, rows {rows.min()}..{rows.max()}, columns {cols.min()}..{cols.max()}"
