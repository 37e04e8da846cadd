"""Cases that tie the Ceres-style refinement -- oracle/grid_oracle.c ogrid_refine_match on the CPU, kg_refine / kgb_refine of
csrc/rgrid_refine_dev.h on the GPU -- to grid_witness.refine_solve_witness: the solver's steps, its Jacobians and every branch of
its trust-region loop that can be reached.  Shared by tests/test_refine_solver_cpu.py and tests/test_refine_solver_gpu.py.

Maps (``maps()``, a map's position is its grid slot in the fleet handle): of grid_geometry_cases.maps() the first room crop
(0.05 m), the 0.1 m room, the crop with negative maxima and both maps of random values.

Families (``cases()``, needs the oracle library):
  counts     COUNTS points -- both sides of every edge of kg_refine's thread rule T = min(1024, roundup64(n)), T / 64 wave
             partials added in wave order, several points per thread above 1024 -- as room scans over the three room maps, and three
             counts once more as uniform clouds over a random map.  Default options.
  landscape  room scans started 1-2 cells and 1-2 degrees off (the correlative matcher's quantisation) under the default and the
             heavy option set; grid_geometry_cases.edge_clouds on both random maps, `far` included, with iterations allowed; uniform
             clouds over the random maps with 10 .. 60 % of their points outside; the room scans once more from the pose the
             oracle's correlative matcher finds for them (`.../matched`: what ScanMatchFleet.scan_match refines from).
  steps      every counts and landscape scan (from its first start) again with max_num_iterations = 1, 2, 3, non-monotonic steps on and off, the weights
             going round WEIGHTS.  With a cap of 1 the answer is the first Levenberg-Marquardt step at radius 1e4 -- almost the
             Gauss-Newton step: three numbers straight from the g and H of IterationZero.
  branches   the inputs on which the witness's trace shows each branch of the loop (BRANCHES below).

Conditions, from the witness and the oracle alone, asserted while the cases are built (``_solve``):
  * the witness's smallest decision margin (refine_solve_witness: `margin`) is at least MARGIN: tolerances and step quality
    relative to their threshold, comparisons between two costs in units of the step's model cost change (relative to the cost
    itself no converging run could keep 1e-3: its last accepted steps change the cost by little more than 1e-6 of it).  A float64
    reordering moves these quotients by about 1e-12;
  * witness and oracle agree on (iterations, termination);
  * a case is STABLE when the oracle's pose is within STABLE_POSE of the witness's.  A long walk over a noise map amplifies
    rounding and is not stable; such a case stays, with `capped` = the same scan under the largest iteration cap at which it is
    stable (UNSTABLE_CAPS; found by running the caps downwards once, checked here at the cap and at cap + 1).  The full-length run
    is then compared for (iterations, termination) and for a final cost not above the initial one only.  At most one case in ten.

FLOORS: per family the worst |oracle - witness| over the stable cases (the capped forms included): pose (absolute, divided by
max(1, |pose|_inf)), initial_cost and final_cost (relative), MEASURED (tests/test_refine_solver_cpu.py::
test_oracle_equals_the_witness_on_every_case prints them) and rounded up to one digit.  The CPU test holds the oracle to them,
the GPU tests hold the kernels to 16 times them (a kernel that adds in another order than the oracle).

Branches not reached, with the witness's reasoning:
  Z  (radius below 1e-32): the radius falls by 2, 4, 8 ... per rejection, so 1e4 -> below 1e-32 takes 15 rejections in a row.
     At a small radius the step is radius x (a length that does not depend on the weights: g and J'J both carry their square,
     the Jacobi scaling takes it out), at most some centimetres; after k rejections the radius is 1e4 / 2^(k (k + 1) / 2), 3e-10
     at k = 9 and 3e-20 at k = 12, so the step has fallen below 1e-8 (|x| + 1e-8) -- the parameter tolerance, tested first --
     before k = 13 even for a pose at the origin; and a step that short either finds the quadratic model exact and is accepted, or
     changes the cost by less than 1e-6 of it (the kPadding quantisation makes the cost piecewise constant below 3e-9 m) and
     ends the run by function tolerance.  The longest run of rejections in any case here is 9 (test_the_trace_census).
  I that recovers: the damped matrix J'J + D/radius of a finite J is positive definite and the model cost change of its solution
     is positive whenever g != 0, in exact arithmetic; with g == 0 the gradient tolerance ends the run before a step is tried.
     An invalid step therefore needs totals that are not finite -- and those stay not finite when the radius shrinks, which is the
     X of the overflowing weights -- or a factorisation that loses definiteness to its own rounding, which is a property of one
     solver's precision (the oracle's and the kernels' float64 Cholesky), not of the operation: the witness cannot state it.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from tests import grid_geometry_cases as G
from tests.grid_cases import scan_of

MAP_INDEX = (0, 3, 4, 5, 6)                # of grid_geometry_cases.maps()
ROOM_SLOTS, RANDOM_SLOTS = (0, 1, 2), (3, 4)
MAX_POINTS = 2400
COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049, 2400)
RANDOM_COUNTS = (3, 129, 1025)             # once more as uniform clouds over a random map
DEFAULT, HEAVY = (1.0, 0.1, 0.4, 100, True), (2.0, 10.0, 40.0, 100, False)
WEIGHTS = ((1.0, 0.1, 0.4), (2.0, 10.0, 40.0), (20.0, 1e-3, 1e-3), (1.0, 1e3, 1e-3), (1.0, 1e-3, 1e3))
CAPS = (1, 2, 3)
MARGIN = 1e-3
STABLE_POSE = 1e-11
GPU_FACTOR = 16.0

# name of the unstable case -> the largest max_num_iterations at which the oracle's pose stays within STABLE_POSE of the witness's
UNSTABLE_CAPS = {"landscape/random_33x57/side_y_low": 36}

# Seeds.  Where the seed that the pattern gives leaves some decision of the run closer than MARGIN to its threshold, or makes
# witness and oracle part ways, another one is used: the edge clouds' seeds per random map were chosen among 950 .. 989 that way
# (the second one keeps one unstable walk, on purpose: the capped form needs a case), two room scans have a seed of their own.
EDGE_SEEDS = {3: 955, 4: 951}
OWN_SEED = {"counts/room3": 1206, "landscape/room01_180x110/scan2_257": 1412}

# MEASURED: family -> (pose, initial_cost, final_cost), see the module's text
FLOORS = {
    "counts": (1e-13, 7e-15, 5e-15),
    "landscape": (2e-13, 7e-15, 4e-14),
    "steps": (4e-13, 2e-14, 3e-11),
    "branches": (5e-15, 3e-15, 2e-15),
}

# what the witness's trace must show somewhere in the family `branches`: name -> predicate on (trace, summary)
BRANCHES = {
    "a rejected step, then an accepted one": lambda t, s: "ra" in t or "rn" in t,
    "a non-monotonic acceptance": lambda t, s: "n" in t,
    "five non-monotonic acceptances in a row": lambda t, s: "nnnnn" in t,
    "the iteration limit at 100": lambda t, s: t.endswith("M") and s["iterations"] == 100,
    "function tolerance": lambda t, s: t.endswith("F"),
    "parameter tolerance": lambda t, s: t.endswith("P"),
    "gradient tolerance at iteration 0": lambda t, s: t == "G" and s["iterations"] == 0,
    "gradient tolerance after an accepted step": lambda t, s: t.endswith("aG"),
    "failure after five invalid steps": lambda t, s: t == "IIIIIX" and s["iterations"] == 5 and s["termination"] == 2,
}

_maps = None


def maps():
    global _maps
    if _maps is None:
        _maps = [G.maps()[i] for i in MAP_INDEX]
        assert [m.occ is not None for m in _maps] == [True, True, True, False, False]
    return _maps


def pose_distance(a, b):
    """max |a - b| / max(1, |b|_inf)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def cost_distance(a, w):
    """|a - w| / |w| for a float64 `a` and the witness's longdouble `w`; where `w` is 0 or not finite AS A FLOAT64 (weights that
    underflow or overflow a double) `a` has to be that very float64: 0 then, inf otherwise."""
    wf = float(np.float64(w))
    if wf == 0.0 or not math.isfinite(wf):
        return 0.0 if (a == wf or (math.isnan(a) and math.isnan(wf))) else math.inf
    return G.rel(a, w)


# ---- scans --------------------------------------------------------------------------------------------------------------------
def _scan(name, family, slot, target, start, pts, values):
    pts = np.ascontiguousarray(pts, np.float32)
    assert 1 <= pts.shape[0] <= MAX_POINTS, (name, pts.shape)
    return NS(name=name, family=family, slot=slot, target=np.asarray(target, np.float64)[:2].copy(), start=np.asarray(start, np.float64).copy(),
              pts=pts, values=tuple(values))


# true poses in the room's own frame; all of them see the walls of every crop
ROOM_POSES = ((0.8, -0.6, 0.35), (-2.0, 1.2, -1.9), (0.3, 0.2, 3.0), (3.1, -1.2, 0.9), (-0.5, 0.9, 1.4), (1.7, 0.4, -0.8), (-1.2, -0.7, 2.3))
SIGNS = ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))


def room_scan(name, family, slot, k, n, seed, values=DEFAULT, target_on_start=False):
    """n points of the room seen from ROOM_POSES[k], started 1.3 / 1.8 cells and 1.5 degrees off, signs by k."""
    m = maps()[slot]
    true = np.array(ROOM_POSES[k % len(ROOM_POSES)])
    pts = scan_of(m.occ - m.shift, true, n_points=n, seed=seed)
    assert pts.shape[0] == n, (name, pts.shape)
    shift = np.array([m.shift[0], m.shift[1], 0.0])
    start = true + shift + np.array([1.3 * m.res, 1.8 * m.res, math.radians(1.5)]) * SIGNS[k % 4]
    target = start[:2] if target_on_start else (true + shift)[:2] + np.array([0.02, -0.03])
    return _scan(name, family, slot, target, start, pts, values)


def uniform_cloud(name, family, slot, n, seed, outside=0.0, values=DEFAULT):
    """n world points, a fraction `outside` of them in a band of 10 cells around the map and the others uniform over it, seen
    from a pose near the map's middle; started 1.2 cells and 1 degree off."""
    m = maps()[slot]
    rng = np.random.default_rng(seed)
    ny, nx = m.cells.shape
    hi = np.array(m.max_xy)
    lo = hi - np.array([ny, nx]) * m.res
    n_out = int(round(outside * n))
    world = rng.uniform(lo, hi, (n, 2))
    for i in range(n_out):                                                         # push the first n_out across one side each
        axis, up = rng.integers(0, 2), rng.integers(0, 2)
        world[i, axis] = (hi[axis] + rng.uniform(0.5, 10.0) * m.res) if up else (lo[axis] - rng.uniform(0.5, 10.0) * m.res)
    world = world[rng.permutation(n)]
    pose = np.array([(hi[0] + lo[0]) / 2 - 0.07, (hi[1] + lo[1]) / 2 + 0.12, 0.4 + (0.01 * seed) % 3.0])
    c, s = math.cos(pose[2]), math.sin(pose[2])
    d = world - pose[:2]
    pts = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1).astype(np.float32)
    start = pose + np.array([1.2 * m.res, -1.2 * m.res, math.radians(1.0)])
    sc = _scan(name, family, slot, pose[:2] + np.array([0.02, 0.01]), start, pts, values)
    if outside:
        frac = G.outside_fraction(m, pose, pts)
        assert 0.10 <= frac <= 0.60, (name, frac)
    return sc


def counts_scans():
    out = [room_scan(f"counts/room{n}", "counts", ROOM_SLOTS[k % 3], k, n, OWN_SEED.get(f"counts/room{n}", 1200 + k)) for k, n in enumerate(COUNTS)]
    out += [uniform_cloud(f"counts/random{n}", "counts", RANDOM_SLOTS[k % 2], n, 1300 + k) for k, n in enumerate(RANDOM_COUNTS)]
    return out


LANDSCAPE_ROOM = ((0, 700), (2, 257), (3, 500))        # (ROOM_POSES index, points) per room map


def landscape_scans():
    out = []
    for slot in ROOM_SLOTS:
        for j, (k, n) in enumerate(LANDSCAPE_ROOM):
            stem = f"landscape/{maps()[slot].name}/scan{k}_{n}"
            for key, values in (("default", DEFAULT), ("heavy", HEAVY)):
                out.append(room_scan(f"{stem}/{key}", "landscape", slot, k + slot, n, OWN_SEED.get(stem, 1400 + 10 * slot + j), values, target_on_start=True))
    for slot in RANDOM_SLOTS:
        m = maps()[slot]
        for name, pose, pts in G.edge_clouds(slot, m, EDGE_SEEDS[slot]):
            out.append(_scan(f"landscape/{name}", "landscape", slot, pose[:2] + 0.03, pose, pts, DEFAULT))
        for j, frac in enumerate((0.15, 0.35, 0.55)):
            out.append(uniform_cloud(f"landscape/{m.name}/outside{int(100 * frac)}", "landscape", slot, 200 + 150 * j, 1500 + 10 * slot + j, outside=frac))
    return out


def matched_scans(base):
    """The landscape room scans once more, started where the oracle's correlative matcher puts them from their start pose as the
    prediction: the start ScanMatchFleet.scan_match hands its refinement.  `prediction` = that match scan's pose."""
    out = []
    for b in base:
        if b.family == "landscape" and b.slot in ROOM_SLOTS:
            m = maps()[b.slot]
            coarse = G.oracle_match(m, (b.slot, b.start, b.pts))[1]
            sc = _scan(f"{b.name}/matched", "landscape", b.slot, b.target, coarse, b.pts, b.values)
            sc.prediction = b.start.copy()
            out.append(sc)
    return out


def steps_scans(base):
    out = []
    for i, b in enumerate(base):
        for cap in CAPS:
            for nonmono in (True, False):
                w = WEIGHTS[(i + cap + (0 if nonmono else 2)) % len(WEIGHTS)]
                out.append(_scan(f"steps/{b.name}/cap{cap}{'n' if nonmono else 'm'}", "steps", b.slot, b.target, b.start, b.pts, w + (cap, nonmono)))
    return out


# The seeds of `branches`, found by a search with the witness over scans of these kinds (not repeated here).
def branches_scans():
    m = maps()
    out = []
    # a, five n in a row, seven r, then accepted again, F; and its monotonic twin, which rejects the first step the other accepts
    out.append(room_scan("branches/nnnnn_rrrrrrr_a_F", "branches", 1, 0, 700, 1600))
    out.append(room_scan("branches/monotonic_twin", "branches", 1, 0, 700, 1600, values=(1.0, 0.1, 0.4, 100, False)))
    # one point: a long walk with many rejections
    out.append(room_scan("branches/one_point", "branches", 0, 1, 1, 1601))
    # the iteration limit at 100: five points over noise
    out.append(uniform_cloud("branches/limit_100", "branches", 3, 5, 1609))
    # parameter tolerance: 2e6 cells away everything is flat, the priors alone pull the pose onto the target
    name, pose, pts = G.edge_clouds(3, m[3], EDGE_SEEDS[3])[-1]
    assert name.endswith("/far")
    out.append(_scan("branches/far_P", "branches", 3, pose[:2] + 0.03, pose, pts, DEFAULT))
    # gradient tolerance at iteration 0: by geometry (every tap outside the map, started on the target: g == 0 exactly) ...
    far = np.array([[500.0, 500.0], [501.0, 500.0], [500.5, 501.0]], np.float32)
    out.append(_scan("branches/G_geometry", "branches", 0, (0.4, -0.3), (0.4, -0.3, 0.2), far, DEFAULT))
    # ... and by weights whose squares underflow a double; failure by weights whose squares overflow it
    b = room_scan("branches/G_underflow", "branches", 2, 3, 65, 1603, values=(1e-200, 1e-200, 1e-200, 100, True))
    out.append(b)
    out.append(_scan("branches/X_overflow", "branches", 2, b.target, b.start, b.pts, (1e160, 1e160, 1e160, 100, True)))
    # weights so small that a diagonal entry of the scaled J'J lies below the LM floor of 1e-6 (what the mutant lm_no_floor needs):
    # a cloud outside the map off its target -- H is the priors' alone, one damped step, then the gradient tolerance -- and a room scan
    out.append(_scan("branches/lm_floor_far", "branches", 0, (0.4, -0.3), (0.7, -0.5, 0.3), far, (1e-5, 1e-4, 1e-4, 100, True)))
    out.append(room_scan("branches/lm_floor_room", "branches", 0, 3, 65, 1604, values=(1e-4, 1e-4, 1e-3, 100, True)))
    return out


# ---- the two references ---------------------------------------------------------------------------------------------------------
def witness_run(sc, values=None, start=None, mutant=None):
    from tests.witness.grid_witness import refine_solve_witness
    m = maps()[sc.slot]
    return refine_solve_witness(sc.target, sc.start if start is None else start, sc.pts, m.cells, m.res, m.max_xy, *(values or sc.values), mutant=mutant)


def oracle_run(sc, values=None, start=None):
    from oracle.binding import oracle_refine_match
    m = maps()[sc.slot]
    return oracle_refine_match(sc.target, sc.start if start is None else start, sc.pts, m.cells, m.res, m.max_xy, *(values or sc.values))


def _solve(sc, values=None, start=None):
    """Both references on a scan -> NS(values, start, w = (pose, summary, trace), o = (pose, summary), stable); the conditions
    that hold for every run -- margin, equal decisions -- asserted."""
    values = tuple(values or sc.values)
    start = sc.start if start is None else np.asarray(start, np.float64)
    w, o = witness_run(sc, values, start), oracle_run(sc, values, start)
    assert w[1]["margin"] >= MARGIN, (sc.name, values, w[1]["margin"], w[2])
    assert (w[1]["iterations"], w[1]["termination"]) == (o[1]["iterations"], o[1]["termination"]), (sc.name, values, w[1], o[1], w[2])
    return NS(values=values, start=start, w=w, o=o, stable=pose_distance(o[0], w[0]) <= STABLE_POSE)


_runs = {}


def solve(sc, values=None, start=None):
    """_solve, computed once per (scan, options, start pose) and never modified."""
    values = tuple(values or sc.values)
    s = sc.start if start is None else np.asarray(start, np.float64)
    key = (sc.name, values, s.tobytes())
    if key not in _runs:
        _runs[key] = _solve(sc, values, s)
    return _runs[key]


def _case(sc):
    run = solve(sc)
    sc.run, sc.capped = run, None
    if not run.stable:
        assert sc.name in UNSTABLE_CAPS, (sc.name, pose_distance(run.o[0], run.w[0]), run.w[2])
        cap = UNSTABLE_CAPS[sc.name]
        values = sc.values[:3] + (cap,) + sc.values[4:]
        sc.capped = solve(sc, values)
        assert sc.capped.stable and cap < run.w[1]["iterations"], (sc.name, cap)
        assert not solve(sc, sc.values[:3] + (cap + 1,) + sc.values[4:]).stable, (sc.name, cap + 1)
    else:
        assert sc.name not in UNSTABLE_CAPS, sc.name
    return sc


_cases = None


def cases():
    """Every case: NS(name, family, slot, target, start, pts, values, run, capped)."""
    global _cases
    if _cases is None:
        base = counts_scans() + landscape_scans()
        out = [_case(sc) for sc in base + steps_scans(base) + matched_scans(base) + branches_scans()]
        assert len({c.name for c in out}) == len(out)
        unstable = [c.name for c in out if c.capped is not None]
        assert 10 * len(unstable) <= len(out) and sorted(unstable) == sorted(UNSTABLE_CAPS), unstable
        _cases = out
    return _cases


def checked_runs(c):
    """The runs of a case that are compared in full (pose and costs): its own when stable, its capped form otherwise."""
    return [c.run] if c.capped is None else [c.capped]


def family(cases_, name):
    return [c for c in cases_ if c.family == name]


def options_of(values):
    from reflector_ekf_slam_amd.grid import CeresScanMatcherOptions2D
    return CeresScanMatcherOptions2D(*values)
