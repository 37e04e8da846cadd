"""Cases of the fleet texture (rgrid_batch_texture_* of include/rgrid.h, ScanMatchFleet.draw_textures), shared by
tests/test_fleet_texture_cpu.py and tests/test_fleet_texture_gpu.py: the smallest grids at which kgb_texture can still go wrong.

A grid here is ``(cells, resolution, max_xy)`` as in tests/fleet_insert_cases.py; a texture is ``(cells uint8 (height, width, 2), box
(offset_x, offset_y, width, height), slice_max (x, y))`` as ``GridFrontEnd.DrawTexture`` and ``oracle_draw_texture`` return it.  The
specification is ProbabilityGrid::DrawToSubmapTexture (probability_grid.cc:86-131): ``oracle_texture`` gives it from the CPU oracle,
``model_texture`` restates its GEOMETRY in numpy (the bytes come from the oracle's table), with three defects that can be planted.
Every comparison is exact.

What the kernel's paths depend on: a workgroup of WG_THREADS threads walks a slot as one array of nx * ny cells, VEC cells per
16-byte load where the address allows and PASS_CELLS cells per pass, and writes the box's pairs VEC at a time.  A slot starts
slot * max_cells cells into the pool, so an ODD max_cells gives slot starts of every alignment a uint16 array can have.
"""
from __future__ import annotations

import math

import numpy as np

WG_THREADS = 512                    # kgb_texture's workgroup
VEC = 8                             # cells per 16-byte load, pairs per 16-byte store
PASS_CELLS = WG_THREADS * 4 * VEC   # cells a workgroup takes in per pass of phase 1 (four vectors in flight per thread)

SWEEP_NAMES = ("inserted_61x37", "last_row_513", "last_column_1023", "one_by_one", "empty", "first_cell", "last_cell", "every_value")
SWEEP_MAX_CELLS = 183 * 181         # odd: slot k starts 3 k mod 8 cells behind a 16-byte boundary -- every residue once in 8 slots


def same_texture(a, b):
    """Bytes, box and slice_max of two textures, exactly."""
    (ca, ba, sa), (cb, bb, sb) = a, b
    return tuple(ba) == tuple(bb) and tuple(sa) == tuple(sb) and ca.shape == cb.shape and ca.dtype == cb.dtype and np.array_equal(ca, cb)


def oracle_texture(grid):
    from oracle.binding import oracle_draw_texture
    return oracle_draw_texture(*grid)


_sweep = None


def sweep_case():
    """-> eight grids, slot = position, named by SWEEP_NAMES:
    0  61 x 37 (nx odd, no multiple of 8 or 64, not square), built by three oracle_insert scans as test_draw_texture_matches_oracle's;
    1  57 x 9 = WG_THREADS + 1 cells, known cells only in the last row: a box of odd width (7) at an odd offset_x (3);
    2  33 x 31 = 2 WG_THREADS - 1 cells, known cells only in the last column;
    3  a 1 x 1 grid, its cell known;
    4  an empty slot;
    5  a single known cell at (0, 0);
    6  a single known cell at (nx - 1, ny - 1);
    7  183 x 181 = max_cells cells: every cell value 1 .. 32767 once (the whole table) and 356 unknown cells, scattered, the four
       corners known: a box that touches all four borders."""
    global _sweep
    if _sweep is not None:
        return _sweep
    from oracle.binding import oracle_insert
    rng = np.random.default_rng(1107)
    res = 0.05
    grids = []
    cells, max_xy, origin = np.zeros((37, 61), np.uint16), (1.0, 1.6), np.array([0.1, 0.1], np.float32)
    for _ in range(3):
        ang = rng.uniform(-math.pi, math.pi, 150)
        rad = rng.uniform(0.2, 0.7, 150)
        ret = np.stack([origin[0] + rad * np.cos(ang), origin[1] + rad * np.sin(ang)], 1).astype(np.float32)
        cells = oracle_insert(cells, res, max_xy, origin, ret)
    grids.append((cells, res, max_xy))
    g = np.zeros((9, 57), np.uint16)
    g[8, 3:10] = rng.integers(1, 32768, 7)
    grids.append((g, res, (0.7, -0.2)))
    g = np.zeros((31, 33), np.uint16)
    g[4:29, 32] = rng.integers(1, 32768, 25)
    grids.append((g, res, (2.0, 3.0)))
    grids.append((np.full((1, 1), 12345, np.uint16), 0.1, (0.3, 0.4)))
    grids.append((np.zeros((19, 23), np.uint16), res, (1.5, 2.5)))
    g = np.zeros((27, 45), np.uint16)
    g[0, 0] = 1
    grids.append((g, res, (-1.0, 0.25)))
    g = np.zeros((27, 45), np.uint16)
    g[26, 44] = 32767
    grids.append((g, res, (4.0, -3.0)))
    size, corners = 183 * 181, np.array([0, 182, 180 * 183, 183 * 181 - 1])
    values = rng.permutation(np.arange(1, 32768, dtype=np.uint16))
    flat = np.zeros(size, np.uint16)
    flat[corners] = values[:4]                                                     # the corners hold four of the values ...
    flat[rng.permutation(np.setdiff1d(np.arange(size), corners))[:32767 - 4]] = values[4:]   # ... 32763 other cells the rest
    grids.append((flat.reshape(181, 183), 0.1, (9.0, 9.5)))
    _sweep = grids
    return grids


MULTI_SHAPE, MULTI_BEHIND = (257, 300), (259, 301)      # (ny, nx): 77100 cells in a slot of 301 * 259 = 77959 (odd)
MULTI_MAX_CELLS = MULTI_BEHIND[0] * MULTI_BEHIND[1]
MULTI_SLOT = 1                                          # starts 77959 cells into the pool: 2-byte aligned, no more


def multi_pass_case():
    """-> (garbage, grid): `grid` has 300 x 257 cells -- more than PASS_CELLS, so every thread makes several passes -- with known
    cells strictly inside; `garbage` (301 x 259, no cell 0) is set in the same slot FIRST, so the 859 cells of the slot behind the
    grid are not 0: a read past nx * ny moves the box."""
    rng = np.random.default_rng(2203)
    garbage = (rng.integers(1, 32768, MULTI_BEHIND).astype(np.uint16), 0.05, (7.0, 8.0))
    g = np.zeros(MULTI_SHAPE, np.uint16)
    inside = rng.integers(1, 32768, (191, 244)).astype(np.uint16)
    inside[rng.random(inside.shape) < 0.4] = 0
    inside[0, 17], inside[190, 100], inside[50, 0], inside[77, 243] = 9, 99, 999, 9999      # the box is the whole patch
    g[10:201, 7:251] = inside
    return garbage, (g, 0.05, (6.5, 7.5))


def byte_table():
    """(32768, 2) uint8: the (value, alpha) pair of every cell value, read off oracle_draw_texture of the every-value grid (its box
    is the whole grid); unknown cells give (0, 0)."""
    grid = sweep_case()[7]
    tex, box, _ = oracle_texture(grid)
    assert box == (0, 0, grid[0].shape[1], grid[0].shape[0])
    table = np.zeros((32768, 2), np.uint8)
    table[grid[0].reshape(-1)] = tex.reshape(-1, 2)
    return table


DEFECTS = ("swapped", "exclusive", "slice")


def model_texture(grid, table, defect=None):
    """The geometry of DrawToSubmapTexture in numpy: the box of the cells that are not 0, the window, slice_max.  Defects: "swapped"
    takes x for y in the box, "exclusive" takes the maxima as one past the end (a box one short), "slice" exchanges the offsets
    in slice_max."""
    assert defect is None or defect in DEFECTS
    cells, res, max_xy = grid
    ys, xs = np.nonzero(cells)
    if defect == "swapped":
        xs, ys = ys, xs
    if xs.size == 0:
        x0, y0, w, h = 0, 0, 1, 1
    else:
        x0, y0 = int(xs.min()), int(ys.min())
        w, h = int(xs.max()) - x0 + 1, int(ys.max()) - y0 + 1
        if defect == "exclusive":
            w, h = w - 1, h - 1
    window = cells[y0:y0 + h, x0:x0 + w]
    off = (x0, y0) if defect == "slice" else (y0, x0)
    return table[window & 32767], (x0, y0, w, h), (float(max_xy[0]) - float(res) * off[0], float(max_xy[1]) - float(res) * off[1])


SUBMAP_N, SUBMAP_RES, SUBMAP_MAX_CELLS = 100, 0.05, 400 * 400


def submap_scene():
    """Range data of three scans around one origin, the second and third reaching beyond the initial submap (100 x 100 cells,
    MapBuilder::InsertIntoSubmap, map_builder.cc:110-120) -> [(origin, returns, misses)]."""
    rng = np.random.default_rng(3301)
    origin = np.array([0.3, 0.5], np.float32)
    out = []
    for reach in (2.0, 3.5, 4.5):
        ang = rng.uniform(-math.pi, math.pi, 240)
        rad = rng.uniform(0.4, reach, 240)
        pts = np.stack([origin[0] + rad * np.cos(ang), origin[1] + rad * np.sin(ang)], 1).astype(np.float32)
        out.append((origin, pts[:200], pts[200:]))
    return out
