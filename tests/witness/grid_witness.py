"""tests/witness/grid_witness.py -- TEST INFRASTRUCTURE: second, independent statements of five grid-mapper pieces whose
only other restatement is oracle/grid_oracle.c (reference: src/mapping/probability_grid_range_data_inserter_2d.cc:40-114
with ray_to_pixel_mask.cc:17-168, probability_values.cc; src/scan_matching/real_time_correlative_scan_matcher_2d.cc:20-136).

  * insert_witness: the ray mask is stated GEOMETRICALLY with exact rational arithmetic -- "column X of the pixel grid is
    crossed between the ordinates y_in and y_out; with half-open pixels [Y, Y+1) an ascending ray covers rows floor(y_in) ..
    ceil(y_out) - 1" -- instead of the oracle's (and the reference's) incremental sub-pixel recurrence; the lookup tables are
    rebuilt with vectorised float32 numpy.
  * grow_witness: GrowAsNeeded + Grid2D::GrowLimits (probability_grid_range_data_inserter_2d.cc:20-38, grid_2d.cc:59-99) as a
    closed form -- the number of doublings from the padded bounding box, the offsets as a sum, the old cells pasted as one block
    -- instead of the oracle's (and the reference's) point-by-point loop that doubles until the point is inside.
  * match_witness: every (rotation, x, y) candidate scored at once with array indexing, the float32 point-order sum as a
    cumulative sum; the oracle loops candidate by candidate.
  * refine_cost_witness: the objective of the Ceres refinement (ceres_scan_matcher_2d.cc:26-62 with
    occupied_space_cost_function_2d.cc:25-81) at one pose, in longdouble, the bicubic interpolation as a tensor product of
    Catmull-Rom weights over all points at once; the oracle and the kernel nest two Horner splines point by point.
  * refine_eval_witness / refine_solve_witness: the refinement's derivatives and its trust-region loop in longdouble -- the
    stacked (n + 3) x 3 Jacobian with g = J'r and H = J'J as matrix products, the derivative weights DERIVED from the value
    weights (numpy.polynomial), the damped 3 x 3 system by Cramer's rule, a trace of every decision and its distance from the
    threshold; the oracle and the kernels keep ten running sums, type the Hermite derivative in and factor by Cholesky.
    SOLVER_MUTANTS: eight deliberately wrong pieces of it, for the test that shows tests/refine_solver_cases.py sees each.
All of them take `mutant`: the grid convention transposed in one place (MUTANTS), for the tests that show which fixtures can
tell the convention from its transpose (tests/grid_geometry_cases.py for the matchers, tests/grid_write_cases.py for
insert_witness and grow_witness).
None of them pins parity with the reference (no tests there, Ceres/Eigen semantics restated): they pin the oracle against a
differently structured implementation.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
S = 1000                       # kSubpixelScale (probability_grid_range_data_inserter_2d.cc:16)
MARK = 32768                   # kUpdateMarker (probability_values.h:34)
_libm = ctypes.CDLL("libm.so.6")
for _n in ("cosf", "sinf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


# ---- probability <-> value (probability_values.{h,cc}) --------------------------------------------------------------
def value_to_cost(v):
    v = np.asarray(v, np.int64) & 32767
    lower, upper = f32(1) - (f32(1) - f32(0.1)), f32(1) - f32(0.1)
    k = f32((upper - lower) / (f32(32768) - f32(2)))
    out = (v.astype(f32) * k + f32(lower - k)).astype(f32)
    return np.where(v == 0, upper, out).astype(f32)


def cost_to_value(c):
    lower, upper = f32(1) - (f32(1) - f32(0.1)), f32(1) - f32(0.1)
    cl = np.minimum(np.maximum(np.asarray(c, f32), lower), upper).astype(f32)
    x = ((cl - lower).astype(f32) * f32(f32(32766) / f32(upper - lower))).astype(f32)
    return (np.floor(x.astype(np.float64) + 0.5).astype(np.int64) + 1)          # lroundf of a non-negative float


def lookup_table(probability):
    """ComputeLookupTableToApplyCorrespondenceCostOdds (probability_values.cc:76-96), marker set."""
    p = f32(probability)
    odds = f32(p / f32(f32(1) - p))
    t = np.zeros(32768, np.int64)
    t[0] = cost_to_value(f32(f32(1) - f32(odds / f32(odds + f32(1))))) + MARK
    cells = np.arange(1, 32768)
    pc = (f32(1) - value_to_cost(cells)).astype(f32)
    o = (odds * (pc / (f32(1) - pc).astype(f32)).astype(f32)).astype(f32)
    pr = (o / (o + f32(1)).astype(f32)).astype(f32)
    t[1:] = cost_to_value((f32(1) - pr).astype(f32)) + MARK
    return t


# ---- ray mask, geometrically ----------------------------------------------------------------------------------------
def ray_pixels(bx, by, ex, ey):
    """Pixels (X, Y) touched by the segment between the CENTRES of sub-pixels (bx, by) and (ex, ey) (super-scaled indices,
    kSubpixelScale sub-pixels per pixel), half-open pixels.  Coordinates are doubled so that centres are integers:
    centre = 2 i + 1, pixel boundaries at multiples of 2 S."""
    if bx > ex:
        bx, by, ex, ey = ex, ey, bx, by
    X0, X1 = bx // S, ex // S
    if X0 == X1:
        y0, y1 = min(by, ey) // S, max(by, ey) // S
        return [(X0, y) for y in range(y0, y1 + 1)]
    x0, y0, x1, y1 = 2 * bx + 1, 2 * by + 1, 2 * ex + 1, 2 * ey + 1
    slope = Fraction(y1 - y0, x1 - x0)
    D = 2 * S
    out = []
    for X in range(X0, X1 + 1):
        xa = max(x0, X * D)
        xb = min(x1, (X + 1) * D)
        ya = Fraction(y0) + slope * (xa - x0)
        yb = Fraction(y0) + slope * (xb - x0)
        if slope > 0:
            lo, hi = math.floor(ya / D), math.ceil(yb / D) - 1
        elif slope < 0:
            lo, hi = math.floor(yb / D), math.ceil(ya / D) - 1
        else:
            lo = hi = math.floor(ya / D)
        # a segment END sits on a sub-pixel centre, never on a pixel boundary: its pixel is always inside [lo, hi]
        out.extend((X, Y) for Y in range(lo, hi + 1))
    return out


def _cell_index(px, py, max_x, max_y, res):
    """MapLimits::GetCellIndex (map_limits.h:48-57): x index from y."""
    rnd = lambda v: int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))       # lround
    return rnd((max_y - float(py)) / res - 0.5), rnd((max_x - float(px)) / res - 0.5)


def super_indices(resolution, max_xy, origin, returns_xy, misses_xy=None):
    """[(x, y)] super-scaled cell indices (kSubpixelScale sub-pixels per pixel) of the origin, the returns and the misses, in
    that order (probability_grid_range_data_inserter_2d.cc:48-68)."""
    rs = resolution / S
    pts = [tuple(origin)] + [tuple(p) for p in np.asarray(returns_xy, f32).reshape(-1, 2)] + \
          [tuple(p) for p in (np.asarray(misses_xy, f32).reshape(-1, 2) if misses_xy is not None else [])]
    return [_cell_index(p[0], p[1], max_xy[0], max_xy[1], rs) for p in pts]


def insert_witness(cells, resolution, max_xy, origin, returns_xy, misses_xy=None, hit_probability=0.55,
                   miss_probability=0.49, insert_free_space=True, mutant=None):
    """ProbabilityGridRangeDataInserter2D::Insert on cells[ny, nx] (uint16).  Returns the new grid, or None when a point
    falls outside (the oracle reports -1 and leaves the grid alone; growing is a separate step).  `mutant`: one of MUTANTS --
    the bounds test, the maxima or the row stride transposed; a write that a mutant sends past the end of the array is dropped."""
    g, nx, ny, max_x, max_y, bound_x, bound_y, stride = _geometry(cells, max_xy, mutant)
    g = g.copy()
    idx = super_indices(resolution, (max_x, max_y), origin, returns_xy, misses_xy)
    if any(ix < 0 or iy < 0 or ix >= bound_x * S or iy >= bound_y * S for ix, iy in idx):
        return None
    n_ret = np.asarray(returns_xy).reshape(-1, 2).shape[0]
    hit, miss = lookup_table(hit_probability), lookup_table(miss_probability)

    def apply(table, x, y):                                     # ApplyLookupTable (probability_grid.cc:38-53)
        k = stride * y + x
        if 0 <= k < g.size and g[k] < MARK:
            g[k] = table[g[k]]

    for ix, iy in idx[1:1 + n_ret]:                             # hits first (:57-62)
        apply(hit, ix // S, iy // S)
    if insert_free_space:
        bx, by = idx[0]
        for ix, iy in idx[1:]:                                  # then the rays to every return and miss (:69-91)
            for x, y in ray_pixels(bx, by, ix, iy):
                apply(miss, x, y)
    g[g >= MARK] -= MARK                                        # FinishUpdate (grid_2d.cc:20-29)
    return g.reshape(ny, nx).astype(np.uint16)


def grow_witness(cells, resolution, max_xy, origin, returns_xy, misses_xy=None, mutant=None):
    """GrowAsNeeded + Grid2D::GrowLimits (probability_grid_range_data_inserter_2d.cc:20-38, grid_2d.cc:59-99) in closed form ->
    (grown cells, new max_xy, offset (x, y) of the old cell (0, 0)).

    The box of origin, returns and misses in float32, padded by float32 1e-6; k = the smallest number of doublings after which
    both padded corners have a cell index inside; after k doublings a side of n cells has 2^k n, the old cell (0, 0) lies at
    sum_{j<k} floor(n 2^j / 2) in each axis, and the maxima have grown by resolution times the OTHER axis' offset of each step
    (max.x belongs to the rows), accumulated in double step by step as the reference rounds them; the old cells are one block
    in a grid of zeros.  `mutant`="maxima" feeds each maximum from its own axis' offset (the other two MUTANTS have no place
    here and change nothing); k is decided by the convention itself, so that a mutant stays defined."""
    assert mutant is None or mutant in MUTANTS, mutant
    old = np.asarray(cells, np.uint16)
    ny, nx = old.shape
    pts = np.concatenate([np.asarray(origin, f32).reshape(1, 2), np.asarray(returns_xy, f32).reshape(-1, 2),
                          np.asarray(misses_xy if misses_xy is not None else [], f32).reshape(-1, 2)])
    pad = f32(1e-6)
    corners = ((pts[:, 0].min() - pad, pts[:, 1].min() - pad), (pts[:, 0].max() + pad, pts[:, 1].max() + pad))
    maxima = [(float(max_xy[0]), float(max_xy[1]))]              # after 0, 1, 2 ... doublings

    def inside(k):
        cols, rows = nx << k, ny << k
        at = [_cell_index(px, py, maxima[k][0], maxima[k][1], resolution) for px, py in corners]
        return all(0 <= ix < cols and 0 <= iy < rows for ix, iy in at)

    k = 0
    while not inside(k):
        maxima.append((maxima[k][0] + resolution * float((ny << k) // 2), maxima[k][1] + resolution * float((nx << k) // 2)))
        k += 1
    off_x, off_y = sum((nx << j) // 2 for j in range(k)), sum((ny << j) // 2 for j in range(k))
    new_max = maxima[k]
    if mutant == "maxima":
        mx, my = maxima[0]
        for j in range(k):
            mx, my = mx + resolution * float((nx << j) // 2), my + resolution * float((ny << j) // 2)
        new_max = (mx, my)
    grown = np.zeros((ny << k, nx << k), np.uint16)
    grown[off_y:off_y + ny, off_x:off_x + nx] = old
    return grown, new_max, (off_x, off_y)


# ---- real-time correlative matcher ----------------------------------------------------------------------------------
def _rotation_cs(angle):
    """Project2D(Rigid3f::Rotation(AngleAxisf(angle, UnitZ))) as a float32 (cos, sin) (transform.h:27-41,93-98)."""
    ha = f32(f32(0.5) * f32(angle))
    w, z = f32(_libm.cosf(float(ha))), f32(_libm.sinf(float(ha)))
    uvy = f32(z + z)
    dx = f32(f32(f32(1) + f32(w * f32(0))) + f32(f32(f32(0) * f32(0)) - f32(z * uvy)))
    dy = f32(f32(f32(0) + f32(w * uvy)) + f32(f32(z * f32(0)) - f32(f32(0) * f32(0))))
    yaw = f32(_libm.atan2f(float(dy), float(dx)))
    return f32(_libm.cosf(float(yaw))), f32(_libm.sinf(float(yaw)))


def _rotate(pts, c, s):
    x, y = pts[:, 0], pts[:, 1]
    return np.stack([((c * x).astype(f32) - (s * y).astype(f32)).astype(f32), ((s * x).astype(f32) + (c * y).astype(f32)).astype(f32)], -1)


# ---- deliberately wrong geometry (tests/test_grid_geometry_cpu.py) ----------------------------------------------------------
# The reference's convention -- x index from world y and max_y, row from world x and max_x, row stride num_x_cells -- transposed
# in one place each.  On a square grid with equal maxima all three are the identity; the geometry cases exist to tell them apart.
MUTANTS = ("bounds", "maxima", "stride")


def _geometry(cells, max_xy, mutant):
    """-> (flat cells, nx, ny, max_x, max_y, bound on x, bound on y, row stride) under `mutant` (None: the convention itself)."""
    assert mutant is None or mutant in MUTANTS, mutant
    g = np.asarray(cells, np.int64)
    ny, nx = g.shape
    mx, my = float(max_xy[0]), float(max_xy[1])
    if mutant == "maxima":
        mx, my = my, mx
    bx, by = (ny, nx) if mutant == "bounds" else (nx, ny)
    return g.reshape(-1), nx, ny, mx, my, bx, by, (ny if mutant == "stride" else nx)


def _load(flat, nx, ny, stride, cx, cy):
    """The cell at (x, y) clamped into the grid, rows `stride` apart (a wrong stride may run past the end: clamped too)."""
    return flat[np.minimum(stride * np.clip(cy, 0, ny - 1) + np.clip(cx, 0, nx - 1), flat.size - 1)]


def match_witness(initial_pose, points_xy, cells, resolution, max_xy, linear_search_window=0.2, angular_search_window=0.26,
                  translation_delta_cost_weight=1e-1, rotation_delta_cost_weight=1e-1, mutant=None):
    """RealTimeCorrelativeScanMatcher2D::Match.  -> (score float32, pose (3,), (scan, x_off, y_off)).  `mutant`: one of MUTANTS."""
    pts = np.ascontiguousarray(points_xy, f32).reshape(-1, 2)
    n = pts.shape[0]
    flat, nx, ny, max_x, max_y, bound_x, bound_y, stride = _geometry(cells, max_xy, mutant)
    rot0 = _rotate(pts, *_rotation_cs(f32(initial_pose[2])))
    rng = np.sqrt(((rot0[:, 0] * rot0[:, 0]).astype(f32) + (rot0[:, 1] * rot0[:, 1]).astype(f32)).astype(f32)).astype(f32)
    max_range = max(f32(f32(3) * f32(resolution)), rng.max() if n else f32(0))
    step = (1. - 1e-3) * math.acos(1. - (resolution * resolution) / (2. * float(f32(max_range * max_range))))
    na = int(math.ceil(angular_search_window / step))
    nl = int(math.ceil(linear_search_window / resolution))
    prob = np.concatenate([(f32(1) - value_to_cost(np.arange(32768))).astype(f32)] * 2)       # value (with or without marker) -> probability
    tx, ty = f32(initial_pose[0]), f32(initial_pose[1])
    offs = np.arange(-nl, nl + 1)
    best = None
    dth = -na * step
    for scan in range(2 * na + 1):
        rot = _rotate(rot0, *_rotation_cs(f32(dth)))
        dth += step
        px, py = (rot[:, 0] + tx).astype(f32), (rot[:, 1] + ty).astype(f32)
        lround = lambda v: np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5)).astype(np.int64)
        ix = lround((max_y - py.astype(np.float64)) / resolution - 0.5)
        iy = lround((max_x - px.astype(np.float64)) / resolution - 0.5)
        cx = ix[None, None, :] + offs[:, None, None]            # [x_off, y_off, point]
        cy = iy[None, None, :] + offs[None, :, None]
        inside = (cx >= 0) & (cy >= 0) & (cx < bound_x) & (cy < bound_y)
        p = np.where(inside, prob[_load(flat, nx, ny, stride, cx, cy)], f32(0.1)).astype(f32)
        score = (np.add.accumulate(p, axis=2, dtype=f32)[:, :, -1] / f32(n)).astype(f32)     # float32 sum in point order
        orientation = (scan - na) * step
        x = -offs[None, :] * resolution + 0.0 * offs[:, None]
        y = -offs[:, None] * resolution + 0.0 * offs[None, :]
        a = np.hypot(x, y) * translation_delta_cost_weight + abs(orientation) * rotation_delta_cost_weight
        score = (score.astype(np.float64) * np.exp(-(a * a))).astype(f32)
        k = int(np.argmax(score))                               # first maximum in (x_off, y_off) order
        xi, yi = divmod(k, offs.size)
        if best is None or score[xi, yi] > best[0]:
            best = (score[xi, yi], (initial_pose[0] + x[xi, yi], initial_pose[1] + y[xi, yi], initial_pose[2] + orientation),
                    (scan, int(offs[xi]), int(offs[yi])))
    return best


# ---- the refinement's objective ---------------------------------------------------------------------------------------------
K_PADDING = 536870911          # kPadding = INT_MAX / 4 (occupied_space_cost_function_2d.cc:57)


def _catmull_rom_terms(t):
    """The four Catmull-Rom basis weights as a tuple; t is anything with + - * and / by a number (an array, a Polynomial)."""
    t2 = t * t
    t3 = t2 * t
    return (-t3 + 2 * t2 - t) / 2, (3 * t3 - 5 * t2 + 2) / 2, (-3 * t3 + 4 * t2 + t) / 2, (t3 - t2) / 2


def _catmull_rom_weights(t):
    """The four Catmull-Rom basis weights of the samples at -1, 0, 1, 2 for the offset t in [0, 1): ceres::CubicHermiteSpline
    written as a weighted sum of its four samples.  t: longdouble (n,) -> (4, n)."""
    return np.stack(_catmull_rom_terms(t))


def _catmull_rom_derivative_weights(t):
    """d/dt of _catmull_rom_weights, DERIVED from it: the value weights evaluated on the polynomial `t` itself
    (numpy.polynomial.Polynomial), differentiated with .deriv(), the coefficients (halves of integers, exact) applied in
    longdouble.  Nothing about the derivative is typed in.  t: longdouble (n,) -> (4, n)."""
    from numpy.polynomial import Polynomial
    out = []
    for w in _catmull_rom_terms(Polynomial([0.0, 1.0])):
        acc = np.zeros_like(t)
        for c in w.deriv().coef[::-1]:
            acc = acc * t + np.longdouble(c)
        out.append(acc)
    return np.stack(out)


def refine_cost_witness(pose, target_translation, initial_angle, points_xy, cells, resolution, max_xy, w_occ, w_t, w_r, mutant=None):
    """The cost CeresScanMatcher2D::Match minimises (ceres_scan_matcher_2d.cc:26-62), at `pose`, as np.longdouble:

      1/2 [ sum_i (w_occ / sqrt(n) bicubic_i)^2 + (w_t (x - tx))^2 + (w_t (y - ty))^2 + (w_r (theta - theta0))^2 ]

    bicubic_i = ceres::BiCubicInterpolator over GridArrayAdapter::GetValue (occupied_space_cost_function_2d.cc:25-81) at the
    point's padded (row, column).  The padded coordinate (max - w) / res - 0.5 + kPadding is formed in float64 as the reference
    forms it: adding kPadding quantises the fractional offset to ~6e-8 cells, which is part of the operation.  Everything after
    it is longdouble.  The interpolation is stated as the tensor product of the Catmull-Rom basis weights over the 4 x 4 taps,
    all points at once -- not as the nested Horner splines of the oracle and of the kernel.  `mutant`: one of MUTANTS."""
    LD = np.longdouble
    pts = np.ascontiguousarray(points_xy, f32).reshape(-1, 2).astype(np.float64)
    n = pts.shape[0]
    flat, nx, ny, max_x, max_y, bound_x, bound_y, stride = _geometry(cells, max_xy, mutant)
    x, y, th = (float(v) for v in pose)
    c, s = math.cos(th), math.sin(th)
    wx = c * pts[:, 0] - s * pts[:, 1] + x
    wy = s * pts[:, 0] + c * pts[:, 1] + y
    r = (max_x - wx) / resolution - 0.5 + float(K_PADDING)              # float64, rounding included
    q = (max_y - wy) / resolution - 0.5 + float(K_PADDING)
    rf, qf = np.floor(r), np.floor(q)
    row, col = rf.astype(np.int64) - K_PADDING, qf.astype(np.int64) - K_PADDING
    tap = np.arange(-1, 3)
    cy = (row[None, :] + tap[:, None])[:, None, :]                      # [4, 1, n]
    cx = (col[None, :] + tap[:, None])[None, :, :]                      # [1, 4, n]
    inside = (cx >= 0) & (cy >= 0) & (cx < bound_x) & (cy < bound_y)
    taps = np.where(inside, value_to_cost(_load(flat, nx, ny, stride, cx, cy)), f32(0.9)).astype(LD)     # [4, 4, n]
    wr = _catmull_rom_weights(r.astype(LD) - rf.astype(LD))
    wc = _catmull_rom_weights(q.astype(LD) - qf.astype(LD))
    bicubic = (wr[:, None, :] * wc[None, :, :] * taps).sum(axis=(0, 1))
    occ = LD(w_occ) / np.sqrt(LD(n)) * bicubic
    d = np.array([LD(w_t) * (LD(x) - LD(float(target_translation[0]))), LD(w_t) * (LD(y) - LD(float(target_translation[1]))),
                  LD(w_r) * (LD(th) - LD(float(initial_angle)))])
    return LD(0.5) * ((occ * occ).sum() + (d * d).sum())


# ---- the refinement's derivatives and its solver ----------------------------------------------------------------------------
# Deliberately wrong solver pieces (tests/test_refine_solver_cpu.py shows that the cases of tests/refine_solver_cases.py see
# each of them; no kernel with a planted defect exists).  The first three act in refine_eval_witness, the others in
# refine_solve_witness:
#   angle_dwx_sign        d(world x)/d(angle) with the wrong sign in the angle column
#   dvdq_value_rows       d(value)/d(column) interpolated from the value rows instead of the derivative rows (it IS the value then)
#   angle_without_ninv    the angle column without its factor -1 / resolution
#   jacobi_rescaled       the Jacobi scaling recomputed at every accepted step instead of fixed at iteration 0
#   lm_no_floor           the LM diagonal without its floor of 1e-6
#   rho_first_ratio       step quality from the first ratio only (no non-monotonic reference)
#   radius_no_cap         the radius update without the cap of 1/3 on its divisor
#   last_iterate          the answer = the last iterate, not the accepted iterate of least cost
SOLVER_MUTANTS = ("angle_dwx_sign", "dvdq_value_rows", "angle_without_ninv", "jacobi_rescaled", "lm_no_floor", "rho_first_ratio",
                  "radius_no_cap", "last_iterate")


def _split_mutant(mutant):
    """-> (geometry mutant, solver mutant): `mutant` is one of MUTANTS, one of SOLVER_MUTANTS or None."""
    assert mutant is None or mutant in MUTANTS or mutant in SOLVER_MUTANTS, mutant
    return (None, mutant) if mutant in SOLVER_MUTANTS else (mutant, None)


def refine_eval_witness(pose, target_translation, initial_angle, points_xy, cells, resolution, max_xy, w_occ, w_t, w_r, mutant=None,
                        padding=True):
    """-> (cost, g[3], H[3, 3]) as np.longdouble: cost = 1/2 |r|^2 of refine_cost_witness, g = J'r, H = J'J with J the stacked
    (n + 3) x 3 Jacobian of the residuals (n occupied-space rows, two translation rows, one rotation row).

    Coordinates as in refine_cost_witness: the padded (row, column) in float64 with kPadding added, everything after it
    longdouble.  Value and both partial derivatives are tensor products over the 4 x 4 taps, all points at once; the derivative
    weights are _catmull_rom_derivative_weights (derived from the value weights, not typed in).  g and H are matrix products of
    the stacked J -- no running sums.  `padding=False` leaves kPadding out and forms the coordinates in longdouble from a
    longdouble pose: the objective is then smooth inside a cell, which is what the finite-difference check of
    tests/test_refine_solver_cpu.py needs.  `mutant`: one of MUTANTS or of SOLVER_MUTANTS."""
    LD = np.longdouble
    geo, sol = _split_mutant(mutant)
    pts = np.ascontiguousarray(points_xy, f32).reshape(-1, 2).astype(np.float64)
    n = pts.shape[0]
    flat, nx, ny, max_x, max_y, bound_x, bound_y, stride = _geometry(cells, max_xy, geo)
    if padding:
        x, y, th = (float(v) for v in pose)
        c, s = math.cos(th), math.sin(th)
        wx = c * pts[:, 0] - s * pts[:, 1] + x
        wy = s * pts[:, 0] + c * pts[:, 1] + y
        r = (max_x - wx) / resolution - 0.5 + float(K_PADDING)          # float64, rounding included
        q = (max_y - wy) / resolution - 0.5 + float(K_PADDING)
        rf, qf = np.floor(r), np.floor(q)
        row, col = rf.astype(np.int64) - K_PADDING, qf.astype(np.int64) - K_PADDING
        tr, tq = r.astype(LD) - rf.astype(LD), q.astype(LD) - qf.astype(LD)
    else:
        x, y, th = (LD(v) for v in pose)
        c, s = np.cos(th), np.sin(th)
        p = pts.astype(LD)
        r = (LD(max_x) - (c * p[:, 0] - s * p[:, 1] + x)) / LD(resolution) - LD(0.5)
        q = (LD(max_y) - (s * p[:, 0] + c * p[:, 1] + y)) / LD(resolution) - LD(0.5)
        rf, qf = np.floor(r), np.floor(q)
        row, col = rf.astype(np.int64), qf.astype(np.int64)
        tr, tq = r - rf, q - qf
    tap = np.arange(-1, 3)
    cy = (row[None, :] + tap[:, None])[:, None, :]                      # [4, 1, n]
    cx = (col[None, :] + tap[:, None])[None, :, :]                      # [1, 4, n]
    inside = (cx >= 0) & (cy >= 0) & (cx < bound_x) & (cy < bound_y)
    taps = np.where(inside, value_to_cost(_load(flat, nx, ny, stride, cx, cy)), f32(0.9)).astype(LD)     # [4, 4, n]
    wr, wc = _catmull_rom_weights(tr), _catmull_rom_weights(tq)
    dwr, dwc = _catmull_rom_derivative_weights(tr), _catmull_rom_derivative_weights(tq)
    bicubic = (wr[:, None, :] * wc[None, :, :] * taps).sum(axis=(0, 1))
    dvdr = (dwr[:, None, :] * wc[None, :, :] * taps).sum(axis=(0, 1))
    dvdq = (wr[:, None, :] * dwc[None, :, :] * taps).sum(axis=(0, 1)) if sol != "dvdq_value_rows" else bicubic
    px, py = pts[:, 0].astype(LD), pts[:, 1].astype(LD)
    cl, sl = LD(c), LD(s)
    dwx, dwy = -sl * px - cl * py, cl * px - sl * py                    # d world / d angle
    if sol == "angle_dwx_sign":
        dwx = -dwx
    ninv = -LD(1) / LD(resolution)                                      # d row / d world x = d column / d world y
    scale = LD(w_occ) / np.sqrt(LD(n))
    J = np.zeros((n + 3, 3), LD)
    J[:n, 0], J[:n, 1] = scale * dvdr * ninv, scale * dvdq * ninv
    J[:n, 2] = scale * (dvdr * dwx + dvdq * dwy) * (ninv if sol != "angle_without_ninv" else LD(1))
    J[n, 0] = J[n + 1, 1] = LD(w_t)
    J[n + 2, 2] = LD(w_r)
    occ = LD(w_occ) / np.sqrt(LD(n)) * bicubic
    d = np.array([LD(w_t) * (LD(x) - LD(float(target_translation[0]))), LD(w_t) * (LD(y) - LD(float(target_translation[1]))),
                  LD(w_r) * (LD(th) - LD(float(initial_angle)))])
    res = np.concatenate([occ, d])
    return LD(0.5) * ((occ * occ).sum() + (d * d).sum()), J.T @ res, J.T @ J


def _double_range(v):
    """`v` (longdouble) with every entry that is not finite AS A FLOAT64 replaced by that float64 (inf, nan)."""
    v = np.asarray(v, np.longdouble)
    f = v.astype(np.float64)
    return np.where(np.isfinite(f), v, f.astype(np.longdouble))[()]


def _det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def _cramer3(A, b):
    d = _det3(A)
    out = []
    for k in range(3):
        M = A.copy()
        M[:, k] = b
        out.append(_det3(M) / d)
    return np.array(out, np.longdouble)


def refine_solve_witness(target_translation, initial_pose, points_xy, cells, resolution, max_xy, w_occ=1.0, w_t=0.1, w_r=0.4,
                         max_num_iterations=100, use_nonmonotonic_steps=True, mutant=None):
    """CeresScanMatcher2D::Match (ceres_scan_matcher_2d.cc:26-62) under the solver options of src/ros_node.cc:364-377, the
    trust-region loop as oracle/grid_oracle.c documents it, in longdouble on top of refine_eval_witness.
    -> (pose float64 (3,), summary, trace).

    Differently built than the oracle and the kernels: g and H come from the stacked Jacobian, the damped 3 x 3 system is solved by
    Cramer's rule (no Cholesky), the model cost change is -(d'g) - d'Hd / 2 in matrix products.  Two places keep the precision of
    the real solver ON PURPOSE: the iterate is rounded to float64 after every step (the solver's parameters are doubles), and a
    total (cost, g, H) that is not finite as a float64 counts as not finite, so that weights which overflow a double take the
    invalid-step branch here as they do in a double solver although longdouble could carry them.

    summary: initial_cost, final_cost (longdouble), iterations, termination (0 convergence, 1 no convergence, 2 failure) and
    margin = the smallest distance of any decision from its threshold: function tolerance, parameter tolerance and rho against
    1e-3 as |value - threshold| / threshold; cost < min_cost, ev_cur < ev_min and ev_cur > ev_cand as |difference of the two
    costs| / (model cost change of the step that produced the newer one) -- the unit in which the solver itself judges a cost
    change (rho is such a quotient), and the quantity a reordered float64 sum moves by about 1e-12.  Relative to the COST these
    three could never keep a margin of 1e-3: a run that ends by function tolerance has just accepted steps that changed the
    cost by little more than 1e-6 of it.
    trace: one letter per decision of the loop -- a accepted with the cost down, n accepted with the cost up, r rejected,
    I invalid step; then how it ended -- M iteration limit, G gradient tolerance, P parameter tolerance, F function tolerance,
    Z radius below its minimum, X failure (five invalid steps in a row)."""
    LD = np.longdouble
    _, sol = _split_mutant(mutant)
    tt = (float(target_translation[0]), float(target_translation[1]))
    a0 = float(initial_pose[2])

    def ev(p):
        c_, g_, H_ = refine_eval_witness(p, tt, a0, points_xy, cells, resolution, max_xy, w_occ, w_t, w_r, mutant=mutant)
        return _double_range(c_), _double_range(g_), _double_range(H_)

    margins = []

    def near(a, b):                                                     # a decision `a against the threshold b`
        if np.isfinite(a) and np.isfinite(b) and b != 0:
            margins.append(float(abs(a - b) / abs(b)))

    def near_cost(a, b, unit):                                          # a decision between two costs, in units of the step's mcc
        if np.isfinite(a) and np.isfinite(b) and np.isfinite(unit) and unit > 0:
            margins.append(float(abs(a - b) / unit))

    jacobi = lambda H_: LD(1) / (LD(1) + np.sqrt(np.diag(H_)))
    norm = lambda v: np.sqrt((np.asarray(v, LD) ** 2).sum())
    with np.errstate(all="ignore"):
        x = np.array([float(v) for v in initial_pose], np.float64)
        cost, g, H = ev(x)
        s = jacobi(H)
        radius, decrease = LD(1e4), LD(2)
        ev_min = ev_cur = ev_ref = ev_cand = initial = cost
        acc_ref = acc_cand = LD(0)
        nonmono = invalid = it = 0
        max_nonmono = 5 if use_nonmonotonic_steps else 0
        successful, best, min_cost, trace, mcc = True, x.copy(), LD(np.inf), [], LD(0)
        while True:
            if successful:
                near_cost(cost, min_cost, mcc)
                if cost < min_cost:
                    min_cost, best = cost, x.copy()
            if it >= int(max_num_iterations):
                end, termination = "M", 1
                break
            if successful and np.abs(g).max() <= LD(1e-10):
                end, termination = "G", 0
                break
            if radius < LD(1e-32):
                end, termination = "Z", 0
                break
            it += 1
            D = np.diag(s)
            Hs, gs = D @ H @ D, D @ g
            A = Hs + np.diag(np.clip(np.diag(Hs), LD(0.0 if sol == "lm_no_floor" else 1e-6), LD(1e32)) / radius)
            step = -_cramer3(A, gs)
            mcc = -(step @ gs) - LD(0.5) * (step @ Hs @ step)
            if not (np.isfinite(step).all() and mcc > 0):
                trace.append("I")
                successful = False
                invalid += 1
                if invalid >= 5:
                    end, termination = "X", 2
                    break
                radius, decrease = radius / decrease, decrease * 2
                continue
            invalid = 0
            xc = (x.astype(LD) + D @ step).astype(np.float64)               # the solver's parameters are doubles
            c_cost, cg, cH = ev(xc)
            moved, enough = norm(x.astype(LD) - xc.astype(LD)), LD(1e-8) * (norm(x) + LD(1e-8))
            near(moved, enough)
            if moved <= enough:
                end, termination = "P", 0
                break
            change, enough = abs(cost - c_cost), LD(1e-6) * cost
            near(change, enough)
            if change <= enough:
                end, termination = "F", 0
                break
            rho = (ev_cur - c_cost) / mcc
            if sol != "rho_first_ratio":
                rho = max(rho, (ev_ref - c_cost) / (acc_ref + mcc))
            near(rho, LD(1e-3))
            if rho > LD(1e-3):
                trace.append("a" if c_cost < cost else "n")
                x, cost, g, H = xc, c_cost, cg, cH
                if sol == "jacobi_rescaled":
                    s = jacobi(H)
                successful = True
                t = 2 * rho - 1
                shrink = 1 - t * t * t
                radius = min(LD(1e16), radius / (shrink if sol == "radius_no_cap" else max(LD(1) / 3, shrink)))
                decrease = LD(2)
                ev_cur, acc_cand, acc_ref = c_cost, acc_cand + mcc, acc_ref + mcc
                near_cost(ev_cur, ev_min, mcc)
                if ev_cur < ev_min:
                    ev_min, nonmono, ev_cand, acc_cand = ev_cur, 0, ev_cur, LD(0)
                else:
                    nonmono += 1
                    near_cost(ev_cur, ev_cand, mcc)
                    if ev_cur > ev_cand:
                        ev_cand, acc_cand = ev_cur, LD(0)
                if nonmono == max_nonmono:
                    ev_ref, acc_ref = ev_cand, acc_cand
            else:
                trace.append("r")
                successful = False
                radius, decrease = radius / decrease, decrease * 2
    last = sol == "last_iterate"
    summary = {"initial_cost": initial, "final_cost": cost if last else min_cost, "iterations": it, "termination": termination,
               "margin": min(margins) if margins else math.inf}
    return (x if last else best).copy(), summary, "".join(trace) + end
