"""Cases that tie the grid matchers to the grid's GEOMETRY, shared by tests/test_grid_geometry_cpu.py and
tests/test_grid_geometry_gpu.py: maps with num_x_cells != num_y_cells and max.x != max.y, and clouds on the map's border.

The reference's convention (map_limits.h:47-57, grid_2d.h:83-106): the x index comes from world y and max.y, the row from world
x and max.x, rows are num_x_cells apart.  On a square map with equal maxima a transposed bounds test, swapped maxima or a row
stride of num_y_cells compute the same thing, and every other matcher fixture of the suite is such a map
(tests/witness/grid_witness.MUTANTS, tests/test_grid_geometry_cpu.py::test_the_square_room_cannot_tell).

Maps (``maps()``; a map's position in the list is its grid slot in the fleet handle):
  * three crops of grid_cases.room_grid() (0.05 m) and one of its 0.1 m variant, the first crop once more with map and scans
    moved as a whole so that both maxima are negative and different;
  * two maps of random values, 57 x 33 and 33 x 57 cells, 20 % unknown, 10 % with the update marker.
Cases (``cases()``, needs the oracle library):
  * room scans: grid_cases.scan_of clouds of the WHOLE room, so that 10 % .. 70 % of a cloud lies outside its cropped map;
    start pose of the refinement = the oracle's correlative match from a prediction a few centimetres off.  Only the
    (scan, option set) pairs are kept on which the oracle alone ends with CONVERGENCE in at most MAX_ORACLE_ITERATIONS
    iterations: a long run through a flat valley amplifies rounding (tests/test_grid_gpu.py::
    test_refine_match_follows_the_oracle_iterate_for_iterate) and says nothing about geometry.
  * edge clouds on the random maps: 64 points in a band from 10 cells outside to 3 cells inside one side or one corner, one
    cloud inside, one 2e6 cells away (inside the interpolator's padding of 2^29 - 1 cells).  The landscape is noise, so they run
    with max_num_iterations = 0: the cost at the start pose is what is compared.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from tests.grid_cases import room_grid, scan_of

RES = 0.05
MAX_ORACLE_ITERATIONS = 40
# CeresScanMatcherOptions2D argument sets of the room scans, and the one of the edge clouds (default weights, no iteration)
OPTION_SETS = {"default": (1.0, 0.1, 0.4, 100, True), "heavy": (2.0, 10.0, 40.0, 100, False)}
ZERO_ITERATIONS = (1.0, 0.1, 0.4, 0, True)
PREDICTION_OFFSET = np.array([0.06, -0.04, math.radians(2.0)])
EDGE_POINTS = 64
OUTSIDE_MIN, OUTSIDE_MAX = 0.10, 0.70

# MEASURED (tests/test_grid_geometry_cpu.py::test_oracle_costs_equal_the_witness prints it): the worst relative difference
# between the oracle's float64 initial_cost / final_cost and refine_cost_witness in longdouble, over every case below.  The
# test's bound is 100 times this; the GPU tests hold the kernels to the project's 1e-12.
WITNESS_VS_ORACLE_ROOM = 4.1e-15
WITNESS_VS_ORACLE_EDGE = 3.6e-16


def crop(cells, max_xy, res, r0, r1, c0, c1):
    """cells[r0:r1, c0:c1] as a map of its own: rows run along world x from max.x down, columns along world y from max.y."""
    return np.ascontiguousarray(cells[r0:r1, c0:c1]), (max_xy[0] - r0 * res, max_xy[1] - c0 * res)


def random_map(ny, nx, seed):
    rng = np.random.default_rng(seed)
    cells = rng.integers(1, 32767, (ny, nx)).astype(np.uint16)                     # 1 .. 32766
    cells[rng.random((ny, nx)) < 0.2] = 0
    cells[rng.random((ny, nx)) < 0.1] |= 0x8000
    return cells


_maps = None


def maps():
    """[NS(name, cells, res, max_xy, occ, shift)]: occ = the room's occupied points in this map's world frame (None: random map)."""
    global _maps
    if _maps is None:
        c05, m05, o05 = room_grid()
        c10, m10, o10 = room_grid(resolution=0.1, half=10.0)
        out = []
        for name, (r0, r1, c0, c1) in (("room_341x390", (40, 381, 90, 480)), ("room_233x457", (100, 333, 0, 457)),
                                       ("room_480x131", (0, 480, 200, 331))):
            cells, mx = crop(c05, m05, RES, r0, r1, c0, c1)
            out.append(NS(name=name, cells=cells, res=RES, max_xy=mx, occ=o05, shift=np.zeros(2)))
        cells, mx = crop(c10, m10, 0.1, 10, 190, 60, 170)
        out.append(NS(name="room01_180x110", cells=cells, res=0.1, max_xy=mx, occ=o10, shift=np.zeros(2)))
        wide = out[0]
        shift = np.array([-3.0 - wide.max_xy[0], -41.5 - wide.max_xy[1]])
        out.append(NS(name="room_341x390_negative_maxima", cells=wide.cells, res=RES, max_xy=(-3.0, -41.5), occ=o05 + shift, shift=shift))
        for k, (ny, nx) in enumerate(((57, 33), (33, 57))):
            out.append(NS(name=f"random_{ny}x{nx}", cells=random_map(ny, nx, 900 + k), res=RES, max_xy=(-3.0, 41.5), occ=None, shift=None))
        assert [m.cells.shape for m in out] == [(341, 390), (233, 457), (480, 131), (180, 110), (341, 390), (57, 33), (33, 57)]
        assert out[0].max_xy == (10.0, 7.5) and out[1].max_xy == (7.0, 12.0) and out[2].max_xy == (12.0, 2.0)
        assert all(m.cells.shape[0] != m.cells.shape[1] and m.max_xy[0] != m.max_xy[1] for m in out)
        _maps = out
    return _maps


def square_room():
    """The old fixture, as a map record: 480 x 480, maxima (12, 12)."""
    cells, max_xy, occ = room_grid()
    return NS(name="room_480x480", cells=cells, res=RES, max_xy=max_xy, occ=occ, shift=np.zeros(2))


def world_of(pose, pts):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    p = np.asarray(pts, np.float64)
    return np.stack([pose[0] + c * p[:, 0] - s * p[:, 1], pose[1] + s * p[:, 0] + c * p[:, 1]], 1)


def outside_fraction(m, pose, pts):
    """Fraction of the cloud that `pose` puts outside the map."""
    w = world_of(pose, pts)
    ix, iy = np.rint((m.max_xy[1] - w[:, 1]) / m.res - 0.5), np.rint((m.max_xy[0] - w[:, 0]) / m.res - 0.5)
    return float(((ix < 0) | (iy < 0) | (ix >= m.cells.shape[1]) | (iy >= m.cells.shape[0])).mean())


# (true pose in the room's own frame, number of points): poses inside the room, counts from one wave to the largest cloud
ROOM_SCANS = (((0.8, -0.6, 0.35), 700), ((-2.0, 1.2, -1.9), 64), ((0.3, 0.2, 3.0), 257), ((3.1, -1.2, 0.9), 500))


def room_match_scans(slot, m):
    """[(name, (slot, prediction, points))] of one room map."""
    out = []
    for k, (true, n) in enumerate(ROOM_SCANS):
        true = np.array(true)
        pts = scan_of(m.occ - m.shift, true, n_points=n, seed=800 + 10 * slot + k)
        assert pts.shape[0] == n
        prediction = true + PREDICTION_OFFSET * (1, 1, 1 if k % 2 else -1) + np.array([m.shift[0], m.shift[1], 0.0])
        frac = outside_fraction(m, prediction, pts)
        assert OUTSIDE_MIN <= frac <= OUTSIDE_MAX, (m.name, k, frac)
        out.append((f"{m.name}/scan{k}_{n}", (slot, prediction, pts)))
    return out


EDGE_KINDS = ("side_x_high", "side_x_low", "side_y_high", "side_y_low", "corner_hh", "corner_hl", "corner_lh", "corner_ll", "inside", "far")


def edge_clouds(slot, m, seed):
    """[(name, pose, points)] of one random map: world positions drawn per EDGE_KINDS, seen from a pose near the map's middle."""
    rng = np.random.default_rng(seed)
    ny, nx = m.cells.shape
    x_hi, y_hi = m.max_xy
    x_lo, y_lo = x_hi - ny * m.res, y_hi - nx * m.res
    out_, in_ = 10 * m.res, 3 * m.res
    band = {"h": lambda hi, lo: (hi - in_, hi + out_), "l": lambda hi, lo: (lo - out_, lo + in_), "all": lambda hi, lo: (lo - out_, hi + out_),
            "in": lambda hi, lo: (lo, hi)}
    spec = {"side_x_high": ("h", "all"), "side_x_low": ("l", "all"), "side_y_high": ("all", "h"), "side_y_low": ("all", "l"),
            "corner_hh": ("h", "h"), "corner_hl": ("h", "l"), "corner_lh": ("l", "h"), "corner_ll": ("l", "l"), "inside": ("in", "in"),
            "far": ("in", "in")}
    out = []
    for k, kind in enumerate(EDGE_KINDS):
        bx, by = spec[kind]
        world = np.stack([rng.uniform(*band[bx](x_hi, x_lo), EDGE_POINTS), rng.uniform(*band[by](y_hi, y_lo), EDGE_POINTS)], 1)
        pose = np.array([(x_hi + x_lo) / 2 + 0.11, (y_hi + y_lo) / 2 - 0.07, 0.7 + 0.3 * k])
        if kind == "far":                                                          # cloud and pose together: the ranges stay small
            far = np.array([2e6 * m.res, -2e6 * m.res])
            world += far
            pose[:2] += far
        c, s = math.cos(pose[2]), math.sin(pose[2])
        d = world - pose[:2]
        pts = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1).astype(np.float32)
        out.append((f"{m.name}/{kind}", pose, pts))
    return out


def oracle_refine(m, scan, values):
    from oracle.binding import oracle_refine_match
    _, target, start, pts = scan
    return oracle_refine_match(target, start, pts, m.cells, m.res, m.max_xy, *values)


def oracle_match(m, scan):
    from oracle.binding import oracle_match as om
    _, pose, pts = scan
    return om(np.asarray(pose, np.float64), pts, m.cells, m.res, m.max_xy)


def _room_case(name, slot, m, match_scan):
    """A room scan's record: the oracle's match, the refine scan that starts from it, the oracle's run per kept option set."""
    om = oracle_match(m, match_scan)
    refine = (slot, np.asarray(match_scan[1], np.float64)[:2].copy(), om[1].copy(), match_scan[2])
    runs = {}
    for key, values in OPTION_SETS.items():
        pose, summ = oracle_refine(m, refine, values)
        if summ["termination"] == 0 and summ["iterations"] <= MAX_ORACLE_ITERATIONS:
            runs[key] = (values, pose, summ)
    return NS(name=name, slot=slot, kind="room", match=match_scan, oracle_match=om, refine=refine, runs=runs)


_cases = None


def cases():
    """Every case, in map order.  NS(name, slot, kind, match = (slot, prediction, points), oracle_match, refine = (slot, target,
    start, points), runs = {option key: (option values, oracle pose, oracle summary)})."""
    global _cases
    if _cases is None:
        out = []
        for slot, m in enumerate(maps()):
            if m.occ is not None:
                mine = [_room_case(name, slot, m, scan) for name, scan in room_match_scans(slot, m)]
                assert sum(bool(c.runs) for c in mine) >= 3, (m.name, [list(c.runs) for c in mine])
                out += mine
                continue
            for k, (name, pose, pts) in enumerate(edge_clouds(slot, m, 950 + slot)):
                match_scan = (slot, pose + PREDICTION_OFFSET * (1, -1, 1), pts)
                refine = (slot, match_scan[1][:2].copy(), pose.copy(), pts)
                opose, summ = oracle_refine(m, refine, ZERO_ITERATIONS)
                assert np.array_equal(opose, pose) and summ["iterations"] == 0 and summ["termination"] == 1, (name, opose, summ)
                out.append(NS(name=name, slot=slot, kind="edge", match=match_scan, oracle_match=oracle_match(m, match_scan), refine=refine,
                              runs={"zero": (ZERO_ITERATIONS, opose, summ)}))
        assert all(c.match[2].shape[0] <= 700 for c in out)
        _cases = out
    return _cases


_square = None


def square_cases():
    """The negative control: scans of the square room, built like the room cases."""
    global _square
    if _square is None:
        m = square_room()
        _square = [_room_case(f"{m.name}/scan{k}", 0, m, (0, np.array(true) + PREDICTION_OFFSET, scan_of(m.occ, np.array(true), n_points=n, seed=690 + k)))
                   for k, (true, n) in enumerate(ROOM_SCANS[:2])]
    return _square


def witness_cost(m, c, pose, values, mutant=None, start=None):
    """refine_cost_witness at `pose` for a run of the case that began at `start` (default: the case's own start pose)."""
    from tests.witness.grid_witness import refine_cost_witness
    _, target, start0, pts = c.refine
    return refine_cost_witness(pose, target, (start0 if start is None else start)[2], pts, m.cells, m.res, m.max_xy, values[0], values[1], values[2], mutant=mutant)


def rel(a, b):
    """|a - b| / |b| in longdouble."""
    a, b = np.longdouble(a), np.longdouble(b)
    return float(abs(a - b) / abs(b))
