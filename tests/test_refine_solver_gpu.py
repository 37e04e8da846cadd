"""The refinement's solver on the GPU (tests/refine_solver_cases.py) against grid_witness.refine_solve_witness, the longdouble
restatement whose derivative side is checked by finite differences and whose mutants these cases see
(tests/test_refine_solver_cpu.py), through every launch form:

  * GridFrontEnd.RefineMatch (kg_refine of csrc/rgrid.hip), one handle per map, sized for it;
  * ScanMatchFleet.refine (kgb_refine of csrc/rgrid_batch.hip), one handle with a grid slot per map: every run of an option set
    in ONE shuffled call -- a block of 1024 threads serves scans of 1 to 2400 points -- and every counts case alone;
  * ScanMatchFleet.scan_match for the landscape room scans under both reductions; the witness starts from the coarse pose that
    the call reports.

Asserted: (iterations, termination) equal to the witness's; pose, initial_cost and final_cost within GPU_FACTOR = 16 times the
family's recorded FLOORS (the worst |oracle - witness| of the family on the CPU); handle and fleet bit for bit; an unstable case in
its capped form within the bound and at full length for its decisions and a cost that does not rise; the start pose byte for byte
where the gradient tolerance ends the run at iteration 0, and with iterations == 5, termination == 2 where the weights overflow.
No number here comes from a kernel's output.

Measured on an MI355X (every test prints its worst ratio to the FLOOR -- the bound is 16 -- and the case that set it), as
pose / initial_cost / final_cost: RefineMatch counts 0.94 / 0.059 / 0.48, landscape 0.20 / 0.044 / 0.91, steps 0.94 / 0.021 /
0.0004, branches 0.34 / 0.27 / 0.48; the fleet's 38 calls the same figures, bit for bit; scan_match 0.0033 / 0.024 / 0.0073 under
both reductions.  The kernels are no further from the witness than the CPU oracle is ("Solver cases")."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_refine_cases as RC
from tests import refine_solver_cases as R

pytestmark = pytest.mark.gpu

QUANTITIES = ("pose", "initial_cost", "final_cost")


@pytest.fixture(scope="module")
def cases(oracle_lib):
    return R.cases()


@pytest.fixture(scope="module")
def single():
    """One GridFrontEnd per map, with room for that map and no more."""
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    hs = []
    for m in R.maps():
        g = GridFrontEnd(max_points=R.MAX_POINTS, max_cells=m.cells.size, max_candidates=1 << 14)
        g.SetGrid(m.cells, m.res, m.max_xy)
        hs.append(g)
    yield hs
    for g in hs:
        g.close()


def make_fleet(reduction=None):
    from reflector_ekf_slam_amd import fleet_match as M
    ms = R.maps()
    f = M.ScanMatchFleet(max_scans=128, max_points=R.MAX_POINTS, num_grids=len(ms), max_cells=max(x.cells.size for x in ms))
    if reduction is not None:
        f.set_reduction(M.REDUCE_ARRIVAL if reduction == "arrival" else M.REDUCE_LAUNCH)
    for slot, x in enumerate(ms):
        f.SetGrid(slot, x.cells, x.res, x.max_xy)
    return f


@pytest.fixture(scope="module")
def fleet():
    f = make_fleet()
    yield f
    f.close()


_single = {}


def single_refine(single, c, run):
    """GridFrontEnd.RefineMatch of a run of a case, computed once and shared (never modified)."""
    k = (c.name, run.values, run.start.tobytes())
    if k not in _single:
        _single[k] = single[c.slot].RefineMatch(c.target, run.start, c.pts, R.options_of(run.values))
    return _single[k]


class Worst:
    """The worst ratio to the family's floor per quantity, and the case that set it."""

    def __init__(self):
        self.ratio = {q: (0.0, "") for q in QUANTITIES}

    def see(self, name, ratios):
        for q, v in zip(QUANTITIES, ratios):
            if v > self.ratio[q][0]:
                self.ratio[q] = (v, name)

    def report(self, what):
        print(what + ": worst ratio to the floor (bound 16) " + ", ".join(f"{q} {v:.3g} ({n})" for q, (v, n) in self.ratio.items()))


def check_decisions(r, c, run):
    ws = run.w[1]
    assert getattr(r, "status", 0) == 0
    assert (r.iterations, r.termination) == (ws["iterations"], ws["termination"]), (c.name, run.values, r, ws, run.w[2])


def check_run(r, c, run, worst):
    """A kernel's result against the witness's run: decisions, then pose and costs within GPU_FACTOR times the family's floors."""
    check_decisions(r, c, run)
    wpose, ws, trace = run.w
    d = (R.pose_distance(r.pose_estimate, wpose), R.cost_distance(r.initial_cost, ws["initial_cost"]), R.cost_distance(r.final_cost, ws["final_cost"]))
    ratios = [d[k] / R.FLOORS[c.family][k] for k in range(3)]
    worst.see(c.name, ratios)
    assert all(v <= R.GPU_FACTOR for v in ratios), (c.name, run.values, trace, dict(zip(QUANTITIES, d)), R.FLOORS[c.family])
    if trace in ("G", "IIIIIX"):                                                   # no step taken: the start pose as it went in
        assert np.asarray(r.pose_estimate, np.float64).tobytes() == run.start.tobytes(), (c.name, r.pose_estimate, run.start)
        assert (r.iterations, r.termination) == ((0, 0) if trace == "G" else (5, 2)), (c.name, r)


def check_case(result_of, c, worst):
    """Every run of a case: the stable one in full; of an unstable case the capped form in full and the full-length form for
    its decisions and a cost that does not rise."""
    if c.capped is None:
        check_run(result_of(c.run), c, c.run, worst)
    else:
        check_run(result_of(c.capped), c, c.capped, worst)
        r = result_of(c.run)
        check_decisions(r, c, c.run)
        assert r.final_cost <= r.initial_cost, (c.name, r)


def runs_of(c):
    return [c.run] + ([c.capped] if c.capped is not None else [])


# ---------------------------------------------------------------------------------------------------------------- single form
@pytest.mark.parametrize("family", list(R.FLOORS))
def test_single_handle_against_the_witness(single, cases, family):
    mine = R.family(cases, family)
    assert len(mine) >= 10
    worst = Worst()
    for c in mine:
        check_case(lambda run: single_refine(single, c, run), c, worst)
    worst.report(f"GridFrontEnd.RefineMatch, {family}, {len(mine)} cases")


# ----------------------------------------------------------------------------------------------------------------- fleet form
def test_fleet_every_run_of_an_option_set_in_one_call(fleet, single, cases):
    groups = {}
    for c in cases:
        for run in runs_of(c):
            groups.setdefault(run.values, []).append((c, run))
    assert len(groups) >= 30 and max(len(g) for g in groups.values()) >= 40
    worst, results = Worst(), {}
    for k, (values, members) in enumerate(groups.items()):
        order = np.random.default_rng(70 + k).permutation(len(members))
        mine = [members[i] for i in order]
        res = fleet.refine([(c.slot, c.target, run.start, c.pts) for c, run in mine], R.options_of(values))
        assert len(res) == len(mine)
        for (c, run), r in zip(mine, res):
            want = single_refine(single, c, run)
            assert RC.same_refine_bits(r, want), (c.name, values, r, want)
            results[(c.name, run.values)] = r
    for c in cases:
        check_case(lambda run: results[(c.name, run.values)], c, worst)
    sizes = sorted({len(c.pts) for c in cases})
    assert sizes[0] == 1 and sizes[-1] == R.MAX_POINTS
    worst.report(f"ScanMatchFleet.refine, {len(groups)} calls, {len(results)} runs")


def test_fleet_each_counts_case_alone(fleet, single, cases):
    worst = Worst()
    mine = R.family(cases, "counts")
    for c in mine:
        res = fleet.refine([(c.slot, c.target, c.run.start, c.pts)], R.options_of(c.run.values))
        assert len(res) == 1 and RC.same_refine_bits(res[0], single_refine(single, c, c.run)), (c.name, res)
        check_case(lambda run: res[0], c, worst)
    assert [len(c.pts) for c in mine][:len(R.COUNTS)] == list(R.COUNTS) and all(c.capped is None for c in mine)
    worst.report("ScanMatchFleet.refine, one counts case per call")


@pytest.mark.parametrize("reduction", ["arrival", "launch"])
def test_fleet_scan_match_refines_from_its_own_coarse_pose(single, cases, reduction):
    """rgrid_batch_scan_match_*: the refinement starts from the launch's own correlative match; the witness starts there too."""
    mine = [c for c in cases if hasattr(c, "prediction")]
    assert len(mine) == 18
    f = make_fleet(reduction)
    try:
        worst = Worst()
        for values in sorted({c.values for c in mine}):
            group = [c for c in mine if c.values == values]
            res = f.scan_match([(c.slot, c.prediction, c.pts) for c in group], None, R.options_of(values))
            assert len(res) == len(group)
            for c, r in zip(group, res):
                assert r.status == 0 and np.abs(r.coarse.pose_estimate - c.start).max() < 1e-12, (c.name, r.coarse, c.start)     # the oracle's match
                run = R.solve(c, start=r.coarse.pose_estimate)                     # (the case's own run when the poses are equal in every bit)
                assert run.stable, (c.name, R.pose_distance(run.o[0], run.w[0]))
                check_run(r.fine, c, run, worst)
                assert RC.same_refine_bits(r.fine, single_refine(single, c, run)), (c.name, r.fine)
        worst.report(f"ScanMatchFleet.scan_match [{reduction}], {len(mine)} scans")
    finally:
        f.close()
