"""The grid matchers' geometry on the CPU (tests/grid_geometry_cases.py): the C oracle against the two numpy witnesses on maps
that are not square and clouds on the map's border, and the proof that these cases -- unlike the square room every other matcher
test uses -- tell the reference's index convention from its transposes (tests/witness/grid_witness.MUTANTS).

tests/test_grid_geometry_gpu.py holds the kernels to the same oracle and the same witness on the same cases."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import grid_geometry_cases as G
from tests.witness.grid_witness import MUTANTS, match_witness

COST_CHANGE = 1e-6             # a mutant "changes" a cost above this relative difference: 1e6 times the GPU tests' 1e-12


@pytest.fixture(scope="module")
def cases(oracle_lib):
    return G.cases()


_match = {}


def match_of(m, c, mutant=None):
    """match_witness on a case -> (best, score bits, pose), computed once per (case, mutant)."""
    key = (c.name, mutant)
    if key not in _match:
        score, pose, best = match_witness(c.match[1], c.match[2], m.cells, m.res, m.max_xy, angular_search_window=math.radians(15.0),
                                          mutant=mutant)          # (the oracle's default window; the witness's own is 0.26)
        _match[key] = (best, np.float32(score).tobytes(), np.asarray(pose, np.float64))
    return _match[key]


def start_cost(m, c, mutant=None):
    values = next(iter(c.runs.values()))[0] if c.kind == "edge" else G.OPTION_SETS["default"]
    return G.witness_cost(m, c, c.refine[2], values, mutant)


def test_case_set_is_what_the_module_says(cases):
    ms = G.maps()
    assert len(ms) == 7 and len(cases) == 5 * len(G.ROOM_SCANS) + 2 * len(G.EDGE_KINDS)
    for c in cases:
        assert c.runs and 1 <= c.match[2].shape[0] <= 700
        for values, pose, summ in c.runs.values():
            if c.kind == "room":
                assert summ["termination"] == 0 and 1 <= summ["iterations"] <= G.MAX_ORACLE_ITERATIONS
            else:
                assert values[3] == 0 and summ["iterations"] == 0 and summ["termination"] == 1 and np.array_equal(pose, c.refine[2])
    # both option sets survive the convergence filter somewhere on every room map, and some run moves the pose
    for slot, m in enumerate(ms):
        if m.occ is not None:
            assert {k for c in cases if c.slot == slot for k in c.runs} == set(G.OPTION_SETS), m.name
    assert any(np.abs(r[1] - c.refine[2]).max() > 1e-3 for c in cases for r in c.runs.values())
    # the far cloud is outside every tap yet inside the interpolator's padding
    far = [c for c in cases if c.name.endswith("/far")]
    assert len(far) == 2
    for c in far:
        m = ms[c.slot]
        w = G.world_of(c.refine[2], c.refine[3])
        cells_away = np.abs((np.array(m.max_xy) - w) / m.res).min()
        assert 1.9e6 < cells_away < 2.1e6 < 536870911


def test_oracle_costs_equal_the_witness(cases):
    """initial_cost at the start pose and final_cost at the oracle's own final pose against refine_cost_witness (longdouble).
    Bound: 100 times the recorded, measured worst difference (grid_geometry_cases.WITNESS_VS_ORACLE_*)."""
    worst = {"room": 0.0, "edge": 0.0}
    for c in cases:
        m = G.maps()[c.slot]
        for values, pose, summ in c.runs.values():
            d0 = G.rel(summ["initial_cost"], G.witness_cost(m, c, c.refine[2], values))
            d1 = G.rel(summ["final_cost"], G.witness_cost(m, c, pose, values))
            worst[c.kind] = max(worst[c.kind], d0, d1)
    print("witness vs oracle, worst relative difference:", worst)
    assert worst["room"] <= 100 * G.WITNESS_VS_ORACLE_ROOM and worst["edge"] <= 100 * G.WITNESS_VS_ORACLE_EDGE, worst


def test_oracle_match_equals_the_witness(cases):
    for c in cases:
        m = G.maps()[c.slot]
        score, pose, best, info = c.oracle_match
        wbest, wbits, wpose = match_of(m, c)
        assert best == wbest and np.float32(score).tobytes() == wbits and np.abs(pose - wpose).max() == 0.0, c.name
        assert info[2] == info[0] * (2 * info[1] + 1) ** 2


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_is_caught_on_every_map(cases, mutant):
    """Discrimination: on every non-square map some case changes the matcher's (best, score bits) and some case changes the
    cost by more than COST_CHANGE; over the whole set at least half of the cases catch the mutant, for both witnesses."""
    caught_match = caught_cost = 0
    for slot, m in enumerate(G.maps()):
        mine = [c for c in cases if c.slot == slot]
        by_match = [match_of(m, c, mutant)[:2] != match_of(m, c)[:2] for c in mine]
        by_cost = [G.rel(start_cost(m, c, mutant), start_cost(m, c)) > COST_CHANGE for c in mine]
        assert any(by_match) and any(by_cost), (m.name, mutant, by_match, by_cost)
        caught_match += sum(by_match)
        caught_cost += sum(by_cost)
    print(mutant, "caught by", caught_match, "(match) and", caught_cost, "(cost) of", len(cases), "cases")
    assert 2 * caught_match >= len(cases) and 2 * caught_cost >= len(cases), (mutant, caught_match, caught_cost, len(cases))


def test_the_square_room_cannot_tell(oracle_lib):
    """The negative control: on room_grid() -- 480 x 480, maxima (12, 12), the map of every older matcher test -- no mutant
    changes a candidate, a score bit or a cost.  That is why the cases above exist."""
    m = G.square_room()
    sq = G.square_cases()
    assert len(sq) >= 2 and all(c.runs for c in sq)
    for c in sq:
        score, pose, best, info = c.oracle_match
        assert (best, np.float32(score).tobytes()) == match_of(m, c)[:2]
        values, opose, summ = next(iter(c.runs.values()))
        for mutant in MUTANTS:
            assert match_of(m, c, mutant)[:2] == match_of(m, c)[:2], (c.name, mutant)
            for at in (c.refine[2], opose):
                assert G.witness_cost(m, c, at, values, mutant) == G.witness_cost(m, c, at, values), (c.name, mutant)
