"""Cases of the occupancy grid and the saved map (rgrid_occupancy_grid / rgrid_batch_occupancy_* of include/rgrid.h,
GridFrontEnd.OccupancyGrid, ScanMatchFleet.occupancy_grids), shared by tests/test_occupancy_cpu.py and tests/test_occupancy_gpu.py:
the smallest grids at which kgb_occupancy can still go wrong.

A case is ``(grid, submap_origin)``: a grid ``(cells, resolution, max_xy)`` as in tests/fleet_texture_cases.py and the translation of
its submap's local pose.  The specification is the reference's painting of the grid's texture: ``expected`` feeds the CPU oracle's
texture to tests/witness/occupancy_witness.py, which tests/test_occupancy_cpu.py pins against libcairo.  Every comparison is exact.

What the kernel's paths depend on: phase 1 is kgb_texture's (tests/fleet_texture_cases.py); phase 2 lays tiles of T x T bytes over
the OUTPUT block -- box width rows of box height bytes, rows STRIDE_ALIGN-aligned -- and a workgroup of WG_THREADS threads takes
them in turn, a wave per grid row of a tile, a lane per VEC bytes of an output row.
"""
from __future__ import annotations

import numpy as np

from tests import fleet_texture_cases as TC
from tests.witness import occupancy_witness as W

T = 64                              # side of kgb_occupancy's LDS tile (OCC_T)
WG_THREADS = 512                    # its workgroup (KGT_THREADS)
VEC = 16                            # bytes a lane stores at once
STRIDE_ALIGN = 16                   # rows of the device's block start on multiples of it
OCCUPANCY, IMAGE = 0, 1
RES = float(np.float32(0.05))       # MapBuilder's `float resolution` as a double

SWEEP_ORIGINS = [(float(np.float32(0.1 * k - 0.3)), float(np.float32(0.25 - 0.07 * k))) for k in range(8)]


def sweep_case():
    """fleet_texture_cases.sweep_case() as it is (odd max_cells: slots start at every 2-byte alignment), each grid with a submap
    origin -> [(grid, submap_origin)] * 8; slot = position.  Grid 7 is the 183 x 181 every-value grid."""
    return list(zip(TC.sweep_case(), SWEEP_ORIGINS))


def _boxed(rng, w, h, off=(2, 1), behind=(1, 1), max_xy=(1.0, 2.0), res=RES):
    """A grid whose known-cells box is w x h at offset `off`, a third of the box unknown, its four border lines touched."""
    nx, ny = off[0] + w + behind[0], off[1] + h + behind[1]
    inside = rng.integers(1, 32768, (h, w)).astype(np.uint16)
    inside[rng.random((h, w)) < 0.33] = 0
    inside[0, rng.integers(0, w)] = inside[h - 1, rng.integers(0, w)] = 77
    inside[rng.integers(0, h), 0] = inside[rng.integers(0, h), w - 1] = 30000
    g = np.zeros((ny, nx), np.uint16)
    g[off[1]:off[1] + h, off[0]:off[0] + w] = inside
    return g, res, max_xy


EDGE_SIDES = (1, T - 1, T, T + 1, 2 * T + 1)
EDGE_BOXES = [(w, h) for w in EDGE_SIDES for h in EDGE_SIDES if {w, h} & {EDGE_SIDES[0], EDGE_SIDES[-1]}]    # every pair with an extreme
STRIDE_BOXES = [(5, 15), (5, 16), (5, 17)]                                      # the row-stride edge
LONG_N = WG_THREADS + 88                                                        # 600: more rows / bytes than threads
LONG_BOXES = [(1, LONG_N), (LONG_N, 1)]
EDGE_MAX_CELLS = (LONG_N + 3) * 3 + 15484                                       # 17293, odd; the largest grid here is 132 x 131 = 17292

_edges = None


def edge_cases():
    """-> [(grid, submap_origin)]: EDGE_BOXES, STRIDE_BOXES, LONG_BOXES in that order, every box strictly inside its grid."""
    global _edges
    if _edges is None:
        rng = np.random.default_rng(4409)
        out = []
        for k, (w, h) in enumerate(EDGE_BOXES + STRIDE_BOXES + LONG_BOXES):
            grid = _boxed(rng, w, h, max_xy=(1.0 + 0.35 * k, 2.0 - 0.2 * k))
            out.append((grid, (float(np.float32(0.31 * k - 2.0)), float(np.float32(1.0 - 0.17 * k)))))
        _edges = out
    return _edges


QUIRK_FORMS = ((1, 0), (0, 1), (1, 1))
_quirks = None


def quirk_cases():
    """-> three (grid, submap_origin), one per QUIRK_FORMS: limits and origin found by a seeded search with the witness such that the
    image is one pixel larger than box side + 10 in x only, in y only, in both."""
    global _quirks
    if _quirks is None:
        rng = np.random.default_rng(7151)
        found = {}
        while len(found) < 3:
            w, h = int(rng.integers(3, 30)), int(rng.integers(3, 30))
            res = float(rng.uniform(0.02, 0.1))
            max_xy = tuple(float(v) for v in rng.uniform(-300.0, 300.0, 2))
            origin = tuple(float(np.float32(v)) for v in rng.uniform(-5.0, 5.0, 2))
            off = (2, 1)
            slice_max = (max_xy[0] - res * off[1], max_xy[1] - res * off[0])
            if not W.in_domain(w, h, slice_max, res, origin):
                continue
            size, _ = W.size_and_origin(w, h, slice_max, res, origin)
            q = (size[0] - h - 10, size[1] - w - 10)
            if q in QUIRK_FORMS and q not in found:
                found[q] = (_boxed(rng, w, h, off=off, max_xy=max_xy, res=res), origin)
        _quirks = [found[q] for q in QUIRK_FORMS]
    return _quirks


_replay = None


def replay_case():
    """-> (grid, submap_origin) whose translation (slice_max - o) + o differs from slice_max by an ulp that moves a float32 corner, so
    that a port taking t = slice_max reports another origin: a directed search with the witness that puts the corner (0, height) next
    to the midpoint of two float32 values."""
    global _replay
    if _replay is None:
        rng = np.random.default_rng(9203)
        off = (2, 1)
        while _replay is None:
            w, h = int(rng.integers(3, 30)), int(rng.integers(3, 30))
            origin = tuple(float(np.float32(v)) for v in rng.uniform(-5.0, 5.0, 2))
            corner = np.float32(rng.uniform(100.0, 12000.0) * rng.choice([-1.0, 1.0]))
            midpoint = 0.5 * (float(corner) + float(np.nextafter(corner, np.float32(np.inf))))
            max_x = (midpoint + h) * RES + RES * off[1]
            for _ in range(9):
                max_x = float(np.nextafter(max_x, np.inf))
                max_xy = (max_x, float(rng.uniform(-20.0, 20.0)))
                slice_max = (max_xy[0] - RES * off[1], max_xy[1] - RES * off[0])
                if (W.translation(slice_max, origin) != slice_max and
                        W.size_and_origin(w, h, slice_max, RES, origin) != W.size_and_origin(w, h, slice_max, RES, origin, "slice_max")):
                    _replay = (_boxed(rng, w, h, off=off, max_xy=max_xy), origin)
                    break
    return _replay


def out_of_domain_case():
    """A grid whose texture lies 18000 pixels from the origin of the map frame: beyond the 16384 the painting's closed form holds for."""
    rng = np.random.default_rng(8803)
    return _boxed(rng, 9, 7, max_xy=(18000 * RES, 1.0)), (float(np.float32(0.5)), float(np.float32(-0.5)))


def expected(case, mode):
    """-> (data (height, width) int8 / uint8, origin (x, y), box) of a case, or None outside the domain: the CPU oracle's texture
    through the witness."""
    grid, submap_origin = case
    tex = TC.oracle_texture(grid)
    try:
        painting = W.paint(tex, grid[1], submap_origin)
    except W.OutOfDomain:
        return None
    data, origin = W.occupancy(painting, grid[1])
    if mode == IMAGE:
        data = W.image_red(painting)
    return np.ascontiguousarray(data), origin, tuple(tex[1])


def same(got, want):
    """An OccupancyGrid record against ``expected``'s answer: bytes, dtype, shape, origin, box, exactly."""
    data, origin, box = want
    return (got.data.dtype == data.dtype and got.data.shape == data.shape and np.array_equal(got.data, data) and
            tuple(got.origin) == tuple(origin) and tuple(got.box) == tuple(box))
