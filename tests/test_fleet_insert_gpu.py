"""The fleet inserter on the GPU (kgb_insert of csrc/rgrid_batch.hip behind ScanMatchFleet.insert): every slot of a call -- cells,
limits and status -- exactly what a GridFrontEnd holds after GrowAsNeeded + Insert (the specification) and what the CPU oracle
computes.  Every assertion is exact equality: the result is a function of the grid and the scan only."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_insert_cases as IC
from tests import fleet_match_cases as MC
from tests import fleet_refine_cases as RC

pytestmark = pytest.mark.gpu

OK, INVALID, CAPACITY = IC.OK, IC.INVALID, IC.CAPACITY


def fleet(num_grids, max_points=2048, max_cells=120 * 120, **kw):
    from reflector_ekf_slam_amd import fleet_match as M
    return M.ScanMatchFleet(max_scans=num_grids, max_points=max_points, num_grids=num_grids, max_cells=max_cells, **kw)


def front_end(max_points=2048, max_cells=120 * 120):
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    return GridFrontEnd(max_points=max_points, max_cells=max_cells, max_candidates=1 << 18)


def set_grids(m, grids):
    for slot, (cells, res, max_xy) in enumerate(grids):
        m.SetGrid(slot, cells, res, max_xy)


def slots_of(m, n):
    return [(m.GetGrid(k), m.GetLimits(k)) for k in range(n)]


def same_slot(got, want):
    return got[1] == want[1] and got[0].shape == want[0].shape and np.array_equal(got[0], want[0])


def test_shape_sweep_in_any_order_and_alone(oracle_lib):
    grids, scans = IC.shape_case()
    m, gf = fleet(8), front_end()
    set_grids(m, grids)
    assert m.insert(scans) == [OK] * 8
    got = slots_of(m, 8)
    for k, scan in enumerate(scans):
        status, cells, lim = IC.handle_pair(gf, grids[k], scan)
        assert status == OK and same_slot(got[k], (cells, lim)), (k, np.count_nonzero(got[k][0] != cells))
        assert same_slot(got[k], IC.oracle_pair(grids[k], scan)), k
        assert (got[k][0] < 32768).all()
    assert np.array_equal(got[0][0], grids[0][0]) and np.count_nonzero(got[7][0] != grids[7][0]) > 1000
    set_grids(m, grids)                                                            # the same call reversed, over fresh grids
    assert m.insert(scans[::-1]) == [OK] * 8
    assert all(same_slot(a, b) for a, b in zip(slots_of(m, 8), got))
    set_grids(m, grids)                                                            # each scan alone
    for scan in scans:
        assert m.insert([scan]) == [OK]
    assert all(same_slot(a, b) for a, b in zip(slots_of(m, 8), got))
    m.close(); gf.close()


def test_exact_corner_crossings(oracle_lib):
    grids, scans = IC.corner_case()
    m = fleet(4)
    set_grids(m, grids)
    assert m.insert(scans) == [OK] * 4
    for k, scan in enumerate(scans):
        want = IC.oracle_pair(grids[k], scan)
        got = (m.GetGrid(k), m.GetLimits(k))
        assert same_slot(got, want), f"slot {k}: {np.count_nonzero(got[0] != want[0])} cells differ"
    m.close()


def test_growth_in_place_call_after_call(oracle_lib):
    case = IC.growth_case()
    m, gf = fleet(2, max_cells=IC.GROW_MAX_CELLS), front_end(max_cells=IC.GROW_MAX_CELLS)
    grids = [grid for grid, _ in case]
    set_grids(m, grids)
    factors = []
    for k in range(len(IC.GROW_FAR)):
        scans = [case[slot][1][k] for slot in range(2)]
        assert m.insert(scans) == [OK, OK]
        for slot in range(2):
            want = IC.oracle_pair(grids[slot], scans[slot])
            status, cells, lim = IC.handle_pair(gf, grids[slot], scans[slot])
            got = (m.GetGrid(slot), m.GetLimits(slot))
            assert status == OK and same_slot(got, want) and same_slot(got, (cells, lim)), (k, slot, got[1], want[1], lim)
            factors.append(want[0].shape[0] // grids[slot][0].shape[0])
            grids[slot] = (want[0], grids[slot][1], (want[1][3], want[1][4]))
    assert factors[:2] == [1, 1] and 4 in factors and 2 in factors
    assert all(grids[slot][0].shape[0] >= 8 * IC.GROW_SHAPES[slot][0] for slot in range(2))
    m.close(); gf.close()


def test_statuses_of_single_scans_leave_the_others_alone(oracle_lib):
    grids, scans, want_status = IC.status_case()
    m = fleet(6, max_points=IC.STATUS_MAX_POINTS, max_cells=IC.STATUS_MAX_CELLS)
    gf = front_end(max_points=IC.STATUS_MAX_POINTS, max_cells=IC.STATUS_MAX_CELLS)
    set_grids(m, grids)
    assert m.insert(scans) == want_status
    for k, scan in enumerate(scans):
        status, cells, lim = IC.handle_pair(gf, grids[k], scan)
        got = (m.GetGrid(k), m.GetLimits(k))
        assert status == want_status[k] and same_slot(got, (cells, lim)), k
    for k in (0, 1, 2):                                                            # refused before anything was touched
        assert same_slot((m.GetGrid(k), m.GetLimits(k)), (grids[k][0], IC.limits_of(*grids[k]))), k
    assert m.GetLimits(3)[0] == 2 * IC.STATUS_N and np.count_nonzero(m.GetGrid(3)) == np.count_nonzero(grids[3][0])   # grown, not inserted
    for k in (4, 5):
        assert same_slot((m.GetGrid(k), m.GetLimits(k)), IC.oracle_pair(grids[k], scans[k])), k
    m.close(); gf.close()


def test_whole_call_refusals_launch_nothing_and_leave_the_handle_usable(oracle_lib):
    from reflector_ekf_slam_amd.grid import RangeDataInserterOptions
    grids, scans = IC.shape_case()
    m = fleet(8)
    set_grids(m, grids[:4])                                                        # slots 4 .. 7 are not set
    before = slots_of(m, 4)
    twice = [scans[3], (scans[3][0],) + scans[5][1:]]
    refused = [lambda: m.submit_insert_code(twice), lambda: m.submit_insert_code([scans[1], scans[5]]),
               lambda: m.submit_insert_code([(8,) + scans[1][1:]]), lambda: m.submit_insert_code([(-1,) + scans[1][1:]]),
               lambda: m.submit_insert_code(scans[:4], RangeDataInserterOptions(True, 0.0, 0.49)),
               lambda: m.submit_insert_code(scans[:4], RangeDataInserterOptions(True, 1.0, 0.49)),
               lambda: m.submit_insert_code(scans[:4], RangeDataInserterOptions(True, 0.55, 0.0)),
               lambda: m.submit_insert_code(scans[:4], RangeDataInserterOptions(True, 0.55, 1.0)),
               lambda: m.submit_insert_code(scans[:4], RangeDataInserterOptions(True, float("nan"), 0.49)),
               lambda: m.submit_insert_code([scans[0]] * 9)]
    for k, call in enumerate(refused):
        assert call() == INVALID, k
        assert m.collect_insert_code() == (INVALID, [])                            # nothing is pending
    assert all(same_slot(a, b) for a, b in zip(slots_of(m, 4), before))
    # one pending submit: everything else waits for its collect
    match_scan = (1, np.array([0.5, 0.5, 0.1]), scans[6][2])
    assert m.submit_insert_code(scans[:4]) == OK
    assert m.submit_insert_code(scans[:4]) == INVALID and m.submit_code([match_scan]) == INVALID
    assert m.GetGrid_code(0)[0] == INVALID and m.GetLimits_code(0)[0] == INVALID
    assert m.SetGrid_code(0, *grids[0]) == INVALID
    assert m.collect_code() == (INVALID, []) and m.collect_refine_code() == (INVALID, []) and m.collect_scan_match_code() == (INVALID, [])
    assert m.collect_insert_code() == (OK, [OK] * 4)                               # ... and it was left pending
    after = slots_of(m, 4)
    for k in range(4):
        assert same_slot(after[k], IC.oracle_pair(grids[k], scans[k])), k
    assert m.submit_code([match_scan]) == OK                                       # a pending match is not collected by the inserter
    assert m.collect_insert_code() == (INVALID, [])
    rc, res = m.collect_code()
    assert rc == OK and res[0].status == OK
    assert m.insert([]) == []
    m.close()


def test_options_switch_the_tables_twice(oracle_lib):
    from reflector_ekf_slam_amd.grid import RangeDataInserterOptions
    grids, scans = IC.shape_case()
    m, gf = fleet(8), front_end()
    set_grids(m, grids)
    hits_only = RangeDataInserterOptions(False, 0.7, 0.4)
    now = list(grids)
    for options in (None, hits_only, None):
        assert m.insert(scans[3:], options) == [OK] * 5
        for k in range(3, 8):
            want = IC.oracle_pair(now[k], scans[k], options)
            status, cells, lim = IC.handle_pair(gf, now[k], scans[k], options)
            got = (m.GetGrid(k), m.GetLimits(k))
            assert status == OK and same_slot(got, want) and same_slot(got, (cells, lim)), (k, options)
            now[k] = (want[0], now[k][1], now[k][2])
    m.close(); gf.close()


def test_more_workgroups_than_compute_units_and_any_position(oracle_lib):
    grids, scans = IC.crowd_case()
    m = fleet(IC.CROWD, max_points=256, max_cells=64 * 64)
    set_grids(m, grids)
    assert m.insert(scans) == [OK] * IC.CROWD
    want = [IC.oracle_pair(grids[k], scans[k]) for k in range(IC.CROWD)]
    for k in range(IC.CROWD):
        got = (m.GetGrid(k), m.GetLimits(k))
        assert same_slot(got, want[k]), (k, np.count_nonzero(got[0] != want[k][0]))
    set_grids(m, grids)
    order = np.random.default_rng(9).permutation(IC.CROWD)
    assert m.insert([scans[k] for k in order]) == [OK] * IC.CROWD
    for k in range(IC.CROWD):
        assert same_slot((m.GetGrid(k), m.GetLimits(k)), want[k]), k
    m.close()


@pytest.mark.parametrize("start", [480, 240], ids=["resident", "grown"])
def test_the_inserted_map_feeds_the_matcher(oracle_lib, start):
    """Three consecutive inserts into one slot, then MapBuilder::ScanMatch on the batch against Match + RefineMatch of a GridFrontEnd
    that inserted the same scans; from 240 x 240 cells the first insertion doubles the grid."""
    from reflector_ekf_slam_amd import fleet_match as M
    max_xy, inserts, (prediction, pts) = IC.map_scene()
    res = 0.05
    first = (np.zeros((start, start), np.uint16), res, (max_xy[0] * start / 480, max_xy[1] * start / 480))
    m, gf = fleet(1, max_cells=480 * 480, max_rotations=512), front_end(max_cells=480 * 480)
    m.SetGrid(0, *first)
    gf.SetGrid(*first)
    grid = first
    for origin, world, misses in inserts:
        assert m.insert([(0, origin, world, misses)]) == [OK]
        gf.Insert(origin, world, misses)
        cells, lim = IC.oracle_pair(grid, (0, origin, world, misses))
        grid = (cells, res, (lim[3], lim[4]))
    lim = m.GetLimits(0)
    assert lim == gf.GetLimits() == IC.limits_of(*grid) and (lim[0], lim[1]) == (480, 480)
    gf._grid_shape = (lim[1], lim[0])
    got = m.GetGrid(0)
    assert np.array_equal(got, gf.GetGrid()) and np.array_equal(got, grid[0]) and np.count_nonzero(got) > 10000
    coarse = gf.Match(prediction, pts)
    fine = gf.RefineMatch(prediction[:2], coarse.pose_estimate, pts)
    for mode in (M.REDUCE_ARRIVAL, M.REDUCE_LAUNCH):
        m.set_reduction(mode)
        r = m.scan_match([(0, prediction, pts)])[0]
        assert r.status == OK and MC.same_bits(r.coarse, coarse) and RC.same_refine_bits(r.fine, fine), (mode, r, coarse, fine)
    assert MC.same_bits(m.match([(0, prediction, pts)])[0], coarse)
    m.close(); gf.close()
