"""The refinement's solver on the CPU (tests/refine_solver_cases.py): the C oracle ogrid_refine_match against
grid_witness.refine_solve_witness -- a longdouble restatement with the Jacobian stacked, the derivative weights derived from the
value weights, Cramer's rule for the damped system -- iterate for iterate, on every family; the witness's own derivative side
against finite differences (no oracle involved); the census of the loop's branches; and the proof that the cases see each of
grid_witness.SOLVER_MUTANTS.

tests/test_refine_solver_gpu.py holds kg_refine and kgb_refine to the same witness on the same cases."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import grid_geometry_cases as G
from tests import refine_solver_cases as R
from tests.witness import grid_witness as W

LD = np.longdouble


@pytest.fixture(scope="module")
def cases(oracle_lib):
    return R.cases()


# ---------------------------------------------------------------------------------------------------------- W1 without the oracle
def test_derivative_weights_come_from_the_value_weights():
    """The derived weights are the derivative of _catmull_rom_weights: a five-point stencil is exact on a cubic."""
    t = np.linspace(0.05, 0.95, 19).astype(LD)
    h = LD(1) / 64
    f = W._catmull_rom_weights
    fd = (-f(t + 2 * h) + 8 * f(t + h) - 8 * f(t - h) + f(t - 2 * h)) / (12 * h)
    d = W._catmull_rom_derivative_weights(t)
    assert d.dtype == LD and np.abs(d - fd).max() < 1e-17
    assert np.abs(f(t).sum(0) - 1).max() < 1e-18 and np.abs(d.sum(0)).max() < 1e-18          # a partition of unity and its derivative


def smooth_residuals(pose, target, angle0, pts, m, w):
    """The n + 3 residuals at a longdouble pose with kPadding left out, from the VALUE weights alone (refine_cost_witness's
    statement): what the finite differences below differentiate."""
    x, y, th = (LD(v) for v in pose)
    c, s = np.cos(th), np.sin(th)
    p = np.asarray(pts, np.float64).astype(LD)
    r = (LD(m.max_xy[0]) - (c * p[:, 0] - s * p[:, 1] + x)) / LD(m.res) - LD(0.5)
    q = (LD(m.max_xy[1]) - (s * p[:, 0] + c * p[:, 1] + y)) / LD(m.res) - LD(0.5)
    rf, qf = np.floor(r), np.floor(q)
    tap = np.arange(-1, 3)
    cy = (rf.astype(np.int64)[None, :] + tap[:, None])[:, None, :]
    cx = (qf.astype(np.int64)[None, :] + tap[:, None])[None, :, :]
    ny, nx = m.cells.shape
    inside = (cx >= 0) & (cy >= 0) & (cx < nx) & (cy < ny)
    taps = np.where(inside, W.value_to_cost(m.cells[np.clip(cy, 0, ny - 1), np.clip(cx, 0, nx - 1)]), np.float32(0.9)).astype(LD)
    v = (W._catmull_rom_weights(r - rf)[:, None, :] * W._catmull_rom_weights(q - qf)[None, :, :] * taps).sum(axis=(0, 1))
    occ = LD(w[0]) / np.sqrt(LD(len(p))) * v
    return np.concatenate([occ, [LD(w[1]) * (x - LD(target[0])), LD(w[1]) * (y - LD(target[1])), LD(w[2]) * (th - LD(angle0))]]), (r - rf, q - qf)


@pytest.mark.parametrize("slot, weights", [(0, (1.0, 0.1, 0.4)), (1, (2.0, 10.0, 40.0)), (3, (20.0, 1e-3, 1e-3)), (4, (1.0, 1e-3, 1e3))])
def test_g_and_H_against_finite_differences_of_the_residuals(slot, weights):
    """refine_eval_witness(padding=False) against a Jacobian from central differences, in longdouble, of residuals that are
    built from the value weights alone.  Points whose 4 x 4 stencil stays in one cell under every displacement used: the
    bicubic is a cubic polynomial per cell, so the five-point stencil in x and in y is exact up to rounding; the angle by
    Richardson extrapolation of three central differences (error h^6; the step balances it against the rounding of a
    coordinate of some hundred cells divided by a step of 1/128 cell).  AGREEMENT REACHED (printed): H within 6.8e-15 of its
    largest entry, g within 6.0e-15 of the size of the terms it sums, on every map; asserted at 5e-14.  The eval mutants move H by
    more than 1e-6."""
    m = R.maps()[slot]
    base = [c for c in R.counts_scans() + R.landscape_scans() if c.slot == slot and len(c.pts) >= 64][0]
    pose, target, angle0 = base.start + np.array([0.003, -0.002, 0.001]), base.target, base.start[2] - 0.01
    reach = float(np.hypot(base.pts[:, 0], base.pts[:, 1]).max())
    h_cell, h_th = LD(1) / 20, LD(m.res / (32 * reach))                            # steps of 1/20 cell, and of at most 1/32 cell at the furthest point
    band = 2 * float(h_cell) + reach * float(h_th) / m.res + 0.01                  # the furthest a displacement moves a coordinate, in cells
    assert band < 0.15
    _, (tr, tq) = smooth_residuals(pose, target, angle0, base.pts, m, weights)
    keep = (tr > band) & (tr < 1 - band) & (tq > band) & (tq < 1 - band)
    pts = base.pts[keep]
    assert pts.shape[0] >= 20, pts.shape
    res = lambda dx=0, dy=0, dt=0: smooth_residuals((LD(pose[0]) + dx, LD(pose[1]) + dy, LD(pose[2]) + dt), target, angle0, pts, m, weights)[0]
    five = lambda f, h: (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
    central = lambda f, h: (f(h) - f(-h)) / (2 * h)
    hw = h_cell * LD(m.res)
    J = np.zeros((pts.shape[0] + 3, 3), LD)
    J[:, 0] = five(lambda d: res(dx=d), hw)
    J[:, 1] = five(lambda d: res(dy=d), hw)
    d1, d2, d4 = (central(lambda d: res(dt=d), h_th / k) for k in (1, 2, 4))
    J[:, 2] = (64 * d4 - 20 * d2 + d1) / 45                                       # Richardson: h^2 and h^4 terms eliminated
    r0 = res()
    cost, g, H = W.refine_eval_witness((LD(pose[0]), LD(pose[1]), LD(pose[2])), target, angle0, pts, m.cells, m.res, m.max_xy, *weights, padding=False)
    eg = float(np.abs(g - J.T @ r0).max() / (np.abs(J) * np.abs(r0)[:, None]).sum(0).max())        # against the size of the terms g sums: they cancel
    eH = float(np.abs(H - J.T @ J).max() / np.abs(H).max())
    exy = float(np.abs(H - J.T @ J)[:2, :2].max() / np.abs(H)[:2, :2].max())
    ec = float(abs(cost - LD(0.5) * (r0 @ r0)) / cost)
    print(f"{m.name}: {pts.shape[0]} points, cost {ec:.1e} g {eg:.1e} H {eH:.1e}, its x / y block {exy:.1e}")
    assert ec < 1e-17 and eg < 5e-14 and eH < 5e-14 and exy < 5e-14, (ec, eg, eH, exy)
    # the check can fail: each eval mutant moves g or H far beyond the agreement
    for mutant in W.SOLVER_MUTANTS[:3]:
        _, gm, Hm = W.refine_eval_witness((LD(pose[0]), LD(pose[1]), LD(pose[2])), target, angle0, pts, m.cells, m.res, m.max_xy, *weights, mutant=mutant,
                                          padding=False)
        assert float(np.abs(Hm - J.T @ J).max() / np.abs(H).max()) > 1e-6, mutant


def test_eval_witness_cost_is_the_cost_witness(cases):
    """The same cost, bit for bit, as refine_cost_witness -- at the start pose of every counts / landscape / branches case."""
    k = 0
    for c in cases:
        if c.family == "steps":
            continue
        m = R.maps()[c.slot]
        a = W.refine_eval_witness(c.start, c.target, c.start[2], c.pts, m.cells, m.res, m.max_xy, *c.values[:3])[0]
        b = W.refine_cost_witness(c.start, c.target, c.start[2], c.pts, m.cells, m.res, m.max_xy, *c.values[:3])
        assert a == b, (c.name, a, b)
        k += 1
    assert k >= 60


# ------------------------------------------------------------------------------------------------------- oracle against witness
def test_case_set_is_what_the_module_says(cases):
    fam = {f: R.family(cases, f) for f in R.FLOORS}
    assert len(fam["counts"]) == len(R.COUNTS) + len(R.RANDOM_COUNTS) and [len(c.pts) for c in fam["counts"]][:len(R.COUNTS)] == list(R.COUNTS)
    matched = [c for c in fam["landscape"] if hasattr(c, "prediction")]
    assert len(matched) == 3 * 3 * 2 and len(fam["landscape"]) == 2 * len(matched) + 2 * (10 + 3)
    assert all(1e-3 < np.abs(c.start - c.prediction).max() < 0.25 for c in matched)      # the matcher moved them, inside its window
    assert len(fam["steps"]) == 6 * (len(fam["counts"]) + len(fam["landscape"]) - len(matched))
    assert {c.values[:3] for c in fam["steps"]} == set(R.WEIGHTS) and {c.values[3:] for c in fam["steps"]} == {(k, b) for k in R.CAPS for b in (True, False)}
    assert {c.slot for c in cases} == set(range(5)) and max(len(c.pts) for c in cases) == R.MAX_POINTS
    for c in cases:
        assert c.run.w[1]["margin"] >= R.MARGIN
    first = [c for c in fam["steps"] if c.values[3] == 1]
    moved = [c for c in first if c.run.w[2] == "aM"]
    assert len(moved) >= len(first) // 2, (len(moved), len(first))                 # a cap of 1 mostly returns the first LM step itself
    print(f"{len(cases)} cases; smallest margin {min(c.run.w[1]['margin'] for c in cases):.4f}; unstable {[c.name for c in cases if c.capped]}")


def test_oracle_equals_the_witness_on_every_case(cases):
    """(iterations, termination) equal on every run (asserted when the cases are built); pose and both costs of every stable run
    within the recorded FLOORS; the full-length form of an unstable case for its decisions and a cost that does not rise."""
    worst = {f: [0.0, 0.0, 0.0, ""] for f in R.FLOORS}
    for c in cases:
        for run in R.checked_runs(c):
            w, o = run.w, run.o
            d = (R.pose_distance(o[0], w[0]), R.cost_distance(o[1]["initial_cost"], w[1]["initial_cost"]), R.cost_distance(o[1]["final_cost"], w[1]["final_cost"]))
            f = worst[c.family]
            for k in range(3):
                if d[k] > f[k]:
                    f[k] = d[k]
            if d[0] == f[0]:
                f[3] = c.name
        if c.capped is not None:
            assert (c.run.w[1]["iterations"], c.run.w[1]["termination"]) == (c.run.o[1]["iterations"], c.run.o[1]["termination"])
            assert c.run.o[1]["final_cost"] <= c.run.o[1]["initial_cost"] and c.run.w[1]["final_cost"] <= c.run.w[1]["initial_cost"]
    for f, v in worst.items():
        print(f"{f}: worst |oracle - witness| pose {v[0]:.2e} ({v[3]}) initial_cost {v[1]:.2e} final_cost {v[2]:.2e}; floors {R.FLOORS[f]}")
    for f, v in worst.items():
        assert all(v[k] <= R.FLOORS[f][k] for k in range(3)), (f, v, R.FLOORS[f])
        assert all(R.FLOORS[f][k] <= 4 * v[k] + 1e-17 for k in range(3)), (f, v, R.FLOORS[f])      # a floor is a measurement, not a budget


def run_length(trace, letter):
    best = cur = 0
    for ch in trace:
        cur = cur + 1 if ch == letter else 0
        best = max(best, cur)
    return best


def test_the_trace_census(cases):
    """Every reachable branch of the loop shows in the witness's traces of the family `branches`; the two that do not are the
    ones refine_solver_cases explains."""
    mine = {c.name: c for c in R.family(cases, "branches")}
    for what, seen in R.BRANCHES.items():
        hits = [n for n, c in mine.items() if seen(c.run.w[2], c.run.w[1])]
        print(f"{what}: {hits}")
        assert hits, what
    # the monotonic twin rejects the very step that the non-monotonic run accepts with the cost up
    a, b = mine["branches/nnnnn_rrrrrrr_a_F"].run.w[2], mine["branches/monotonic_twin"].run.w[2]
    k = next(i for i in range(min(len(a), len(b))) if a[i] != b[i])
    assert (a[k], b[k]) == ("n", "r") and "n" not in b, (a, b)
    # gradient tolerance both ways; the overflow takes the invalid-step branch and returns the start pose
    for name in ("branches/G_geometry", "branches/G_underflow", "branches/X_overflow"):
        c = mine[name]
        assert c.run.w[0].tobytes() == c.start.tobytes() == c.run.o[0].tobytes(), name
    assert float(mine["branches/G_underflow"].run.w[1]["initial_cost"]) == 0.0 and mine["branches/G_underflow"].run.w[1]["initial_cost"] > 0
    assert math.isinf(mine["branches/X_overflow"].run.o[1]["initial_cost"])
    # not reached anywhere: the radius floor, an invalid step outside the failure
    traces = [r.w[2] for c in cases for r in ([c.run] + ([c.capped] if c.capped else []))]
    assert not any(t.endswith("Z") for t in traces) and all("I" not in t or t == "IIIIIX" for t in traces)
    longest = max(run_length(t, "r") for t in traces)
    print(f"longest run of rejections: {longest} (15 in a row would be needed for the radius floor)")
    assert 5 <= longest < 15
    assert sum("n" in t for t in traces) >= 20 and sum(t.endswith("F") for t in traces) >= 40 and sum(t.endswith("P") for t in traces) >= 3


# ------------------------------------------------------------------------------------------------------------------ the mutants
def mutant_targets(cases, mutant):
    """The stable cases a mutant is tried on: the eval mutants on the capped steps of the small clouds (the first LM steps), the
    solver mutants on the full-length small clouds."""
    small = [c for c in cases if c.capped is None and len(c.pts) <= 129 and c.run.w[2] not in ("G", "IIIIIX")]
    if mutant in W.SOLVER_MUTANTS[:3]:
        return [c for c in small if c.family == "steps" and c.values[3] == 1]
    return [c for c in small if c.family != "steps"]


@pytest.mark.parametrize("mutant", W.SOLVER_MUTANTS)
def test_every_solver_mutant_moves_a_pose_beyond_the_gpu_bound(cases, mutant):
    """Each planted defect of the witness moves the pose of at least one stable case by more than the bound the GPU tests hold
    the kernels to (GPU_FACTOR x the family's pose floor): a kernel with that defect would fail there.

    MEASURED (largest pose change / GPU bound, cases that catch it): angle_dwx_sign 2.5e11 (55 of 62), dvdq_value_rows 1.7e11
    (58 of 62), angle_without_ninv 3.6e12 (54 of 62), jacobi_rescaled 1.1e5 (1 of 35), lm_no_floor 3.7e10 (2 of 35),
    rho_first_ratio 1.5e11 (28 of 35), radius_no_cap 2.6e11 (30 of 35), last_iterate 3.8e10 (6 of 35).  The Jacobi scaling
    cancels out of the step, (H + diag(H) / radius) d = -g whatever the scaling, unless the floor of the LM diagonal binds: only
    the two lm_floor cases of `branches` can see it or the floor, and they exist for that."""
    best, caught, tried = (0.0, ""), 0, 0
    for c in mutant_targets(cases, mutant):
        pose = R.witness_run(c, mutant=mutant)[0]
        factor = R.pose_distance(pose, c.run.w[0]) / (R.GPU_FACTOR * R.FLOORS[c.family][0])
        tried += 1
        caught += factor > 1
        if factor > best[0]:
            best = (factor, c.name)
    print(f"{mutant}: caught by {caught} of {tried} cases, largest pose change {best[0]:.3g} x the GPU bound ({best[1]})")
    assert caught >= 1 and best[0] > 100, (mutant, best)


# A FACT OF THE OLD NET, not a condition on the new one: which mutants stay within the bounds the suite held the refinement to
# before these cases -- pose within 1e-8 of the oracle (kernel tests), within 5e-3 of scipy (tests/test_grid_cpu.py) -- on the
# converging room runs of grid_geometry_cases (first room crop and the 0.1 m room, default options).
# (within 1e-8, within 5e-3).  The first column is for a defect of the kernel alone; a defect that the oracle shares -- the kernel
# was written from it line by line -- passed the 1e-8 comparison whatever it was, and only the second column stood against it.
OLD_NET = {"angle_dwx_sign": (False, False), "dvdq_value_rows": (False, False), "angle_without_ninv": (False, False),
           "jacobi_rescaled": (True, True), "lm_no_floor": (True, True), "rho_first_ratio": (False, True), "radius_no_cap": (False, False),
           "last_iterate": (True, True)}


def test_the_old_bounds_could_not_tell(oracle_lib):
    old = [c for c in G.cases() if c.kind == "room" and c.slot in (0, 3) and "default" in c.runs]
    assert len(old) >= 4
    table = {}
    for mutant in W.SOLVER_MUTANTS:
        worst = 0.0
        for c in old:
            m = G.maps()[c.slot]
            values, opose, _ = c.runs["default"]
            _, target, start, pts = c.refine
            pose = W.refine_solve_witness(target, start, pts, m.cells, m.res, m.max_xy, *values, mutant=mutant)[0]
            worst = max(worst, float(np.abs(pose - opose).max()))
        table[mutant] = (worst < 1e-8, worst < 5e-3)
        print(f"{mutant}: worst pose change on the old cases {worst:.2e}: passes 1e-8 {worst < 1e-8}, passes 5e-3 {worst < 5e-3}")
    assert table == OLD_NET, table
