"""The grid matchers' geometry on the GPU (tests/grid_geometry_cases.py): maps with num_x_cells != num_y_cells and max.x != max.y,
clouds partly outside the map and clouds on its border, through both launch forms --

  * GridFrontEnd.Match / .RefineMatch (kg_discretize + kg_score, kg_refine of csrc/rgrid.hip), one handle per map, each sized
    for exactly its own map and the largest cloud;
  * ScanMatchFleet.match / .refine / .scan_match (kgb_match, kgb_best, kgb_refine of csrc/rgrid_batch.hip), one handle whose
    grid slots hold all the maps -- every slot another shape and another offset into the pool -- with every case in one call, in
    a shuffled order, under both reductions.

Against the oracle, with the bounds the project already holds these kernels to: the matcher's best and info equal, score within
1.2e-7 relative, pose within 1e-12 (fleet_match_cases.check_against_oracle); the refinement's (iterations, termination) equal,
pose within 1e-8, initial_cost within 1e-12 relative (tests/test_grid_gpu.py::test_refine_match_follows_the_oracle_iterate_for_iterate).
Against grid_witness.refine_cost_witness (longdouble): initial_cost at the start pose and final_cost at the kernel's OWN reported
pose within 1e-12 relative; the CPU oracle sits at ~4e-15 there (grid_geometry_cases.WITNESS_VS_ORACLE_ROOM), and the index
convention's transposes move these costs by more than 1e-6 (tests/test_grid_geometry_cpu.py).  The two forms bit for bit.

Measured on an MI355X (every test prints its figures): matcher scores equal to the oracle's in every bit; refined pose within
4.5e-15 of the oracle's, initial_cost within 4.0e-15 relative; against the witness initial_cost within 2.3e-16 and final_cost
within 2.5e-16 relative -- the kernels sit closer to the longdouble witness than the CPU oracle does."""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import fleet_match_cases as MC
from tests import fleet_refine_cases as RC
from tests import grid_geometry_cases as G

pytestmark = pytest.mark.gpu

MAX_POINTS = 700
POSE_TOL, COST_RTOL = 1e-8, 1e-12
KEYS = ("default", "heavy", "zero")


@pytest.fixture(scope="module")
def cases(oracle_lib):
    return G.cases()


@pytest.fixture(scope="module")
def single():
    """One GridFrontEnd per map, with room for that map and no more."""
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    hs = []
    for m in G.maps():
        g = GridFrontEnd(max_points=MAX_POINTS, max_cells=m.cells.size, max_candidates=1 << 14)
        g.SetGrid(m.cells, m.res, m.max_xy)
        hs.append(g)
    yield hs
    for g in hs:
        g.close()


@pytest.fixture(scope="module", params=["arrival", "launch"])
def fm(request):
    """One ScanMatchFleet with a grid slot per map; the pool's slot size is the largest map's."""
    from reflector_ekf_slam_amd import fleet_match as M
    ms = G.maps()
    m = M.ScanMatchFleet(max_scans=64, max_points=MAX_POINTS, num_grids=len(ms), max_cells=max(x.cells.size for x in ms))
    m.set_reduction(M.REDUCE_ARRIVAL if request.param == "arrival" else M.REDUCE_LAUNCH)
    for slot, x in enumerate(ms):
        m.SetGrid(slot, x.cells, x.res, x.max_xy)
    yield m
    m.close()


def values_of(c, key):
    return c.runs[key][0]


_single, _oracle = {}, {}


def single_match(single, c):
    """GridFrontEnd.Match of a case, computed once and shared (never modified)."""
    if c.name not in _single:
        _single[c.name] = single[c.slot].Match(c.match[1], c.match[2])
    return _single[c.name]


def single_refine(single, c, key, start=None):
    """GridFrontEnd.RefineMatch of a case under an option set, from the case's start pose or from `start`."""
    s = c.refine[2] if start is None else np.asarray(start, np.float64)
    k = (c.name, key, s.tobytes())
    if k not in _single:
        _single[k] = single[c.slot].RefineMatch(c.refine[1], s, c.refine[3], RC.options_of(values_of(c, key)))
    return _single[k]


def oracle_run(c, key, start=None):
    """The oracle's refinement (pose, summary) from the case's start pose (computed with the cases) or from `start`."""
    if start is None or np.asarray(start, np.float64).tobytes() == c.refine[2].tobytes():
        return c.runs[key][1:]
    s = np.asarray(start, np.float64)
    k = (c.name, key, s.tobytes())
    if k not in _oracle:
        _oracle[k] = G.oracle_refine(G.maps()[c.slot], (c.slot, c.refine[1], s, c.refine[3]), values_of(c, key))
    return _oracle[k]


def check_refine(r, c, key, start=None):
    """A refine result against the oracle and against the witness."""
    m = G.maps()[c.slot]
    values = values_of(c, key)
    s = c.refine[2] if start is None else np.asarray(start, np.float64)
    pose, summ = oracle_run(c, key, start)
    w0, w1 = G.witness_cost(m, c, s, values, start=s), G.witness_cost(m, c, r.pose_estimate, values, start=s)
    print(f"{c.name} [{key}] iterations {r.iterations}/{summ['iterations']} termination {r.termination}/{summ['termination']} "
          f"pose-oracle {np.abs(r.pose_estimate - pose).max():.2e} initial-oracle {G.rel(r.initial_cost, summ['initial_cost']):.2e} "
          f"initial-witness {G.rel(r.initial_cost, w0):.2e} final-witness {G.rel(r.final_cost, w1):.2e}")
    assert getattr(r, "status", 0) == 0
    assert (r.iterations, r.termination) == (summ["iterations"], summ["termination"]), (c.name, key, r, summ)
    assert np.abs(r.pose_estimate - pose).max() < POSE_TOL, (c.name, key, r.pose_estimate - pose)
    assert r.initial_cost == pytest.approx(summ["initial_cost"], rel=COST_RTOL) and r.final_cost == pytest.approx(summ["final_cost"], rel=POSE_TOL)
    assert r.final_cost <= r.initial_cost
    assert G.rel(r.initial_cost, w0) <= COST_RTOL and G.rel(r.final_cost, w1) <= COST_RTOL, (c.name, key, r, w0, w1)
    if values[3] == 0:                                                             # no iteration: the start pose comes back as it went in
        assert r.pose_estimate.tobytes() == s.tobytes() and (r.iterations, r.termination) == (0, 1) and r.final_cost == r.initial_cost


def shuffled(items, seed):
    order = np.random.default_rng(seed).permutation(len(items))
    assert len(items) < 2 or not np.array_equal(order, np.arange(len(items)))
    return [items[i] for i in order]


def with_key(cases, key):
    return [c for c in cases if key in c.runs]


# ---------------------------------------------------------------------------------------------------------------- single form
def test_single_match_against_the_oracle(single, cases):
    for c in cases:
        r = single_match(single, c)
        print(f"{c.name} best {r.best} score-oracle {abs(r.score - c.oracle_match[0]) / c.oracle_match[0]:.2e} "
              f"pose-oracle {np.abs(r.pose_estimate - c.oracle_match[1]).max():.2e}")
        MC.check_against_oracle(NS(status=0, **vars(r)), c.oracle_match)
    assert len({c.slot for c in cases}) == len(single) == 7


@pytest.mark.parametrize("key", KEYS)
def test_single_refine_against_the_oracle_and_the_witness(single, cases, key):
    mine = with_key(cases, key)
    assert len(mine) >= (20 if key == "zero" else 15)
    for c in mine:
        check_refine(single_refine(single, c, key), c, key)
    if key != "zero":
        assert any(np.abs(single_refine(single, c, key).pose_estimate - c.refine[2]).max() > 1e-3 for c in mine)       # it moved
        assert {c.slot for c in mine} == {0, 1, 2, 3, 4}
    else:
        assert {c.slot for c in mine} == {5, 6}


# ----------------------------------------------------------------------------------------------------------------- fleet form
def test_fleet_match_all_cases_in_one_call(fm, single, cases):
    mine = shuffled(cases, 41)
    res = fm.match([c.match for c in mine])
    assert len(res) == len(cases) == 40
    for c, r in zip(mine, res):
        MC.check_against_oracle(r, c.oracle_match)
        assert MC.same_bits(r, single_match(single, c)), (c.name, r, single_match(single, c))


@pytest.mark.parametrize("key", KEYS)
def test_fleet_refine_all_cases_in_one_call(fm, single, cases, key):
    mine = shuffled(with_key(cases, key), 42)
    res = fm.refine([c.refine for c in mine], RC.options_of(values_of(mine[0], key)))
    assert len(res) == len(mine)
    for c, r in zip(mine, res):
        check_refine(r, c, key)
        assert RC.same_refine_bits(r, single_refine(single, c, key)), (c.name, key, r, single_refine(single, c, key))


@pytest.mark.parametrize("key", KEYS)
def test_fleet_chained_match_then_refine(fm, single, cases, key):
    """rgrid_batch_scan_match_*: the refinement starts from the launch's own correlative match, not from the oracle's."""
    mine = shuffled(with_key(cases, key), 43)
    res = fm.scan_match([c.match for c in mine], None, RC.options_of(values_of(mine[0], key)))
    assert len(res) == len(mine)
    for c, r in zip(mine, res):
        coarse = single_match(single, c)
        assert r.status == 0 and MC.same_bits(r.coarse, coarse), (c.name, r.coarse, coarse)
        MC.check_against_oracle(r.coarse, c.oracle_match)
        check_refine(r.fine, c, key, start=coarse.pose_estimate)
        want = single_refine(single, c, key, start=coarse.pose_estimate)
        assert RC.same_refine_bits(r.fine, want), (c.name, key, r.fine, want)
