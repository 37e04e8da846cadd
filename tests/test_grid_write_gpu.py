"""The grid's write path on the GPU against the independent witnesses (grow_witness + insert_witness of
tests/witness/grid_witness.py) on every case of tests/grid_write_cases.py, in both forms: GridFrontEnd (kg_grow, kg_ends, kg_hits,
kg_rays, kg_finish of csrc/rgrid.hip) and ScanMatchFleet.insert (kgb_insert of csrc/rgrid_batch.hip).  handle == witness,
fleet == witness, fleet == handle, and the CPU oracle as a third opinion; every assertion is exact equality of cells and limits.
tests/test_grid_write_cpu.py shows on the CPU what these cases can tell apart; no kernel with a planted defect runs here."""
from __future__ import annotations

import numpy as np
import pytest

from tests import grid_write_cases as WC
from tests.witness import grid_witness as W

pytestmark = pytest.mark.gpu

OK = 0
MAX_POINTS = {"ties": 4096, "growth": 128}


def fleet(family, num_grids, **kw):
    from reflector_ekf_slam_amd import fleet_match as M
    return M.ScanMatchFleet(max_scans=num_grids, max_points=MAX_POINTS.get(family, 2048), num_grids=num_grids,
                            max_cells=WC.max_cells_of(family), **kw)


def front_end(family):
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    return GridFrontEnd(max_points=MAX_POINTS.get(family, 2048), max_cells=WC.max_cells_of(family), max_candidates=1 << 16)


def options_of(opt):
    from reflector_ekf_slam_amd.grid import RangeDataInserterOptions
    return None if opt is None else RangeDataInserterOptions(opt[2], opt[0], opt[1])


def handle_chain(gf, ch):
    """SetGrid, then per scan GrowAsNeeded (where the chain grows) + Insert(grow=False) -> [(cells, limits)] after every scan."""
    gf.SetGrid(*ch.grid)
    out = []
    for (_, origin, ret, mis), opt in zip(ch.steps, ch.options):
        if ch.grow:
            gf.GrowAsNeeded(origin, ret, mis)
        gf.Insert(origin, ret, mis, options_of(opt), grow=False)
        out.append((gf.GetGrid(), gf.GetLimits()))
    return out


def fleet_family(m, chains, rng=None):
    """Fresh grids, then one insert call per step with every chain's scan of that step (shuffled by `rng`) -> {name: [(cells, limits)]}."""
    for ch in chains:
        m.SetGrid(ch.slot, *ch.grid)
    out = {ch.name: [] for ch in chains}
    for k in range(max(len(ch.steps) for ch in chains)):
        live = [ch for ch in chains if len(ch.steps) > k]
        (opt,) = {ch.options[k] for ch in live}                                    # a call has one option set
        order = np.arange(len(live)) if rng is None else rng.permutation(len(live))
        assert m.insert([live[i].steps[k] for i in order], options_of(opt)) == [OK] * len(live), k
        for ch in live:
            out[ch.name].append((m.GetGrid(ch.slot), m.GetLimits(ch.slot)))
    return out


def check(name, got, want):
    """got == want, both [(cells, limits)]: the message names the case, the number of differing cells and their bounding box."""
    assert len(got) == len(want), name
    for k, ((cells, lim), (wcells, wlim)) in enumerate(zip(got, want)):
        assert lim == wlim, f"{name} step {k}: limits {lim} != {wlim}"
        assert cells.shape == wcells.shape and np.array_equal(cells, wcells), WC.diff_report(f"{name} step {k}", cells, wcells)


@pytest.mark.parametrize("family", [f for f in WC.FAMILIES])
def test_both_forms_equal_the_witness(oracle_lib, family):
    chains = WC.FAMILIES[family]()
    assert (len(chains), sum(len(c.steps) for c in chains)) == WC.SIZES[family]
    want = {ch.name: [(c, lim) for c, lim, _ in WC.witness_chain(ch)] for ch in chains}
    gf = front_end(family)
    by_handle = {ch.name: handle_chain(gf, ch) for ch in chains}
    gf.close()
    for ch in chains:
        check(f"GridFrontEnd vs witness, {ch.name}", by_handle[ch.name], want[ch.name])
    m = fleet(family, len(chains))
    by_fleet = fleet_family(m, chains)
    for ch in chains:
        check(f"fleet vs witness, {ch.name}", by_fleet[ch.name], want[ch.name])
        check(f"fleet vs GridFrontEnd, {ch.name}", by_fleet[ch.name], by_handle[ch.name])
        check(f"fleet vs oracle, {ch.name}", by_fleet[ch.name], [(c, lim) for c, lim, _ in WC.oracle_chain(ch)])
    shuffled = fleet_family(m, chains, np.random.default_rng(17))                  # the same calls over fresh grids, scans in another order
    for ch in chains:
        check(f"fleet shuffled vs witness, {ch.name}", shuffled[ch.name], want[ch.name])
    if family == "counts":                                                         # each scan alone in its call
        for ch in chains:
            m.SetGrid(ch.slot, *ch.grid)
        for ch in chains:
            assert m.insert([ch.steps[0]]) == [OK], ch.name
            check(f"fleet alone vs witness, {ch.name}", [(m.GetGrid(ch.slot), m.GetLimits(ch.slot))], want[ch.name])
    m.close()


def test_the_loop_map_feeds_the_matchers_bit_for_bit():
    """The map the kernels built from three growing insertions == the witness-built map; on it GridFrontEnd.Match and
    ScanMatchFleet.match under both reductions return match_witness' best candidate and score bits, the pose within 1e-12."""
    from reflector_ekf_slam_amd import fleet_match as M
    ch = WC.loop()[0]
    cells, lim, _ = WC.witness_chain(ch)[-1]
    _, prediction, pts = WC.loop_match_scan()
    w_score, w_pose, w_best = W.match_witness(prediction, pts, cells, lim[2], (lim[3], lim[4]), angular_search_window=WC.MATCH_ANGULAR_WINDOW)
    gf, m = front_end("loop"), fleet("loop", 1)
    check("GridFrontEnd vs witness, loop", handle_chain(gf, ch)[-1:], [(cells, lim)])
    check("fleet vs witness, loop", fleet_family(m, [ch])[ch.name][-1:], [(cells, lim)])
    results = [("GridFrontEnd.Match", gf.Match(prediction, pts))]
    for mode, name in ((M.REDUCE_ARRIVAL, "arrival"), (M.REDUCE_LAUNCH, "launch")):
        m.set_reduction(mode)
        r = m.match([(0, prediction, pts)])[0]
        assert r.status == OK, (name, r)
        results.append((f"ScanMatchFleet.match/{name}", r))
    for name, r in results:
        assert tuple(r.best) == w_best and np.float32(r.score) == w_score, (name, r, w_best, w_score)
        assert np.float64(r.score) == np.float64(w_score), (name, r.score)          # nothing beyond the float32 bits
        assert np.abs(r.pose_estimate - np.array(w_pose)).max() < 1e-12, (name, r.pose_estimate, w_pose)
    m.close(); gf.close()
