"""The fleet voxel filters on the GPU (kgb_filter of csrc/rgrid_batch.hip behind ScanMatchFleet.filter): every scan of a call --
the two voxel-filtered clouds and the adaptively filtered returns -- exactly what a GridFrontEnd's three calls return (the
specification) and what the CPU oracle computes.  Every assertion is exact equality of counts and of the points' bit patterns."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_filter_scan_cases as FC
from tests import fleet_insert_cases as IC
from tests import fleet_match_cases as MC
from tests import fleet_refine_cases as RC

pytestmark = pytest.mark.gpu

OK, INVALID, CAPACITY, BUFFER = FC.OK, FC.INVALID, FC.CAPACITY, FC.BUFFER


def fleet(max_scans, max_points=2560, **kw):
    from reflector_ekf_slam_amd import fleet_match as M
    kw.setdefault("max_cells", 64)
    kw.setdefault("max_rotations", 1)
    return M.ScanMatchFleet(max_scans=max_scans, max_points=max_points, **kw)


def front_end(max_points=2560, max_cells=64, max_candidates=1 << 10):
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    return GridFrontEnd(max_points=max_points, max_cells=max_cells, max_candidates=max_candidates)


def check_call(m, gf, scans, size, options):
    """One call against the oracle and a GridFrontEnd, scan by scan -> the results."""
    got = m.filter(scans, size, options)
    assert len(got) == len(scans)
    for k, (r, scan) in enumerate(zip(got, scans)):
        want = FC.oracle_triple(scan, size, options)
        sizes = (k, r.returns.shape, r.misses.shape, r.filtered.shape, [w.shape for w in want])
        assert r.status == OK and FC.same_result(r, want), sizes
        if gf is not None:
            assert FC.same_result(r, FC.handle_triple(gf, scan, size, options)), sizes
    return got


def test_strides_at_three_sizes_in_any_order_and_alone(oracle_lib):
    scans = FC.stride_case()
    m, gf = fleet(len(scans)), front_end()
    for size in FC.STRIDE_SIZES:
        got = check_call(m, gf, scans, size, None)
        back = m.filter(scans[::-1], size)[::-1]                                   # the same call reversed
        assert all(FC.same_results(a, b) for a, b in zip(back, got)), size
        for k, scan in enumerate(scans):                                           # each scan alone
            assert FC.same_results(m.filter([scan], size)[0], got[k]), (size, k)
    m.close(); gf.close()


def test_rounding_signed_zeros_and_duplicates(oracle_lib):
    scans = FC.rounding_case()
    m, gf = fleet(len(scans)), front_end()
    got = check_call(m, gf, scans, FC.ROUND_RES, None)
    assert got[2].returns.shape[0] == got[2].misses.shape[0] == 4                                     # the first of a voxel, with its sign bits:
    assert np.signbit(got[2].returns[2]).all() and not np.signbit(got[2].misses[1]).any()             # (-0.0, -0.0) here, (0.0, 0.0) reversed
    assert got[3].returns.shape[0] == 1 and FC.same_cloud(got[3].returns, scans[3][0][:1])              # one voxel: its first point
    assert FC.same_cloud(got[4].returns, scans[4][0])                                                 # a voxel each: every point, in place
    assert FC.same_cloud(got[5].returns, scans[5][0]) and FC.same_cloud(got[5].misses, scans[5][1])   # the returns' voxels do not suppress misses
    m.close(); gf.close()


def test_hash_table_full_load_colliding_keys_and_three_voxels(oracle_lib):
    from reflector_ekf_slam_amd import fleet_match as M
    limit = M.filter_max_points()
    scans, options = FC.hash_case(limit)
    m, gf = fleet(len(scans), max_points=limit), front_end(max_points=limit)
    got = check_call(m, gf, scans, FC.HASH_SIZE, options)
    assert got[0].returns.shape[0] == limit and got[1].returns.shape[0] == 4096 and got[2].returns.shape[0] == 3
    m.close(); gf.close()


def test_range_gate(oracle_lib):
    scans, options = FC.gate_case()
    m, gf = fleet(len(scans)), front_end()
    got = check_call(m, gf, scans, 0.025, options)
    assert FC.same_cloud(got[0].filtered[:4], FC.ON_GATE)                                              # norm == max_range stays
    assert got[1].status == OK and got[1].filtered.shape[0] == 0 and got[1].returns.shape[0] > 0       # the gate removes everything
    assert FC.same_cloud(got[2].returns[:4], FC.PAST_GATE) and FC.same_cloud(got[2].filtered[:4], FC.AXIS_GATE)   # one ulp beyond goes
    assert got[2].filtered.shape[0] <= options.min_num_points                                          # ... and the rest is untouched
    m.close(); gf.close()


def test_every_path_of_the_adaptive_search_in_one_call(oracle_lib):
    scans, options, paths = FC.adaptive_case()
    m, gf = fleet(len(scans), max_points=8192), front_end(max_points=8192)
    got = check_call(m, gf, scans, FC.ADAPTIVE_SIZE, options)
    for r, scan, path in zip(got, scans, paths):
        dense = r.filtered.shape[0] >= options.min_num_points
        assert dense == (path[0] in ("first", "ladder")), path
    scans, options, _ = FC.fraction_case()
    got = check_call(m, gf, scans, FC.ADAPTIVE_SIZE, options)
    assert [r.filtered.shape[0] for r in got] == [2, 3, 3, 2]
    m.close(); gf.close()


def test_statuses_of_single_scans_leave_the_others_alone(oracle_lib):
    scans, want = FC.status_case()
    m = fleet(len(scans), max_points=FC.STATUS_MAX_POINTS)
    got = m.filter(scans)
    assert [r.status for r in got] == want
    for k, (r, scan) in enumerate(zip(got, scans)):
        if want[k] != OK:
            assert r.returns.shape == r.misses.shape == r.filtered.shape == (0, 2), k
            continue
        assert FC.same_result(r, FC.oracle_triple(scan)), k
        assert FC.same_results(m.filter([scan])[0], r), k                          # ... and equals its solo run
    assert got[5].returns.shape[0] == 0 and got[5].filtered.shape[0] == 0 and got[5].misses.shape[0] > 0
    assert [r.status for r in m.filter([scans[1], scans[2]])] == [CAPACITY, INVALID]   # a call without a single workgroup
    m.close()


def test_whole_call_refusals_and_the_pending_rule(oracle_lib):
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    scans = FC.stride_case()[2:6]
    m = fleet(4, max_cells=120 * 120, max_rotations=256)
    L, h = M._filter_lib(), m._h
    opt = M._FilterOptions(0.025, 0.9, 500.0, 100.0)
    packed = M.ScanMatchFleet.pack_filter(scans)
    negative, null = M.ScanMatchFleet.pack_filter(scans[:1]), M.ScanMatchFleet.pack_filter(scans[:1])
    negative[0][0].n_misses = -1
    null[0][0].returns_xy = None
    refused = [lambda: L.rgrid_batch_filter_submit(None, M.C.byref(opt), M.C.cast(packed[0], M.C.c_void_p), 4),
               lambda: L.rgrid_batch_filter_submit(h, None, M.C.cast(packed[0], M.C.c_void_p), 4),
               lambda: L.rgrid_batch_filter_submit(h, M.C.byref(opt), None, 4), lambda: L.rgrid_batch_filter_submit(h, M.C.byref(opt), None, 0),
               lambda: L.rgrid_batch_filter_submit(h, M.C.byref(opt), M.C.cast(packed[0], M.C.c_void_p), -1),
               lambda: m.submit_filter_code([scans[0]] * 5), lambda: m.submit_filter_packed_code(negative), lambda: m.submit_filter_packed_code(null),
               lambda: m.submit_filter_code(scans, 0.0), lambda: m.submit_filter_code(scans, -0.025), lambda: m.submit_filter_code(scans, float("nan")),
               lambda: m.submit_filter_code(scans, 0.025, AdaptiveVoxelFilterOptions(0.0, 500, 100.0)),
               lambda: m.submit_filter_code(scans, 0.025, AdaptiveVoxelFilterOptions(float("nan"), 500, 100.0))]
    for k, call in enumerate(refused):
        assert call() == INVALID, k
        assert m.collect_filter_code() == (INVALID, [])                            # nothing is pending
    # a handle with no grid set filters normally
    want = [FC.oracle_triple(s) for s in scans]
    got = m.filter(scans)
    assert all(r.status == OK and FC.same_result(r, w) for r, w in zip(got, want))
    # one pending submit: everything else waits for its collect
    grids, iscans = IC.shape_case()
    match_scan = (0, np.array([0.5, 0.5, 0.1]), iscans[6][2])
    assert m.submit_filter_code(scans) == OK
    assert m.submit_filter_code(scans) == INVALID and m.submit_code([match_scan]) == INVALID and m.submit_refine_code([]) == INVALID
    assert m.submit_scan_match_code([match_scan]) == INVALID and m.submit_insert_code([iscans[3]]) == INVALID
    assert m.SetGrid_code(0, *grids[0]) == INVALID and m.GetGrid_code(0)[0] == INVALID and m.GetLimits_code(0)[0] == INVALID
    assert m.collect_code() == (INVALID, []) and m.collect_refine_code() == (INVALID, []) and m.collect_scan_match_code() == (INVALID, [])
    assert m.collect_insert_code() == (INVALID, [])
    # too small a buffer: the counts, and the submit is left pending
    counts = [(w[0].shape[0], w[1].shape[0], w[2].shape[0]) for w in want]
    total = sum(sum(c) for c in counts)
    assert m.collect_filter_code(total - 1) == (BUFFER, counts) and m.collect_filter_code(0) == (BUFFER, counts)
    assert m.submit_filter_code(scans) == INVALID
    rc, got = m.collect_filter_code(total)                                         # exactly enough room
    assert rc == OK and all(r.status == OK and FC.same_result(r, w) for r, w in zip(got, want))
    assert m.collect_filter_code() == (INVALID, [])
    # a pending match is not collected by the filter
    m.SetGrid(0, *grids[0])
    assert m.submit_code([match_scan]) == OK
    assert m.submit_filter_code(scans) == INVALID and m.collect_filter_code() == (INVALID, [])
    rc, res = m.collect_code()
    assert rc == OK and res[0].status == OK
    assert m.filter([]) == []
    assert m.last_prepare_seconds() >= 0.0
    m.close()


def test_more_workgroups_than_compute_units_and_any_position(oracle_lib):
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    scans, options = FC.crowd_case(), AdaptiveVoxelFilterOptions(*FC.CROWD_OPTIONS)
    m = fleet(FC.CROWD, max_points=256)
    got = check_call(m, None, scans, 0.025, options)
    assert any(r.filtered.shape[0] < r.returns.shape[0] for r in got)
    order = np.random.default_rng(9).permutation(FC.CROWD)
    again = m.filter([scans[k] for k in order], 0.025, options)
    assert all(FC.same_results(again[j], got[k]) for j, k in enumerate(order))
    m.close()


def test_the_filtered_clouds_feed_the_rest_of_the_tick(oracle_lib):
    """filter -> scan_match on the adaptively filtered cloud -> insert of the voxel-filtered returns and misses moved by the refined
    pose, on the batch, against a GridFrontEnd doing VoxelFilter x 2, AdaptiveVoxelFilter, Match, RefineMatch, GrowAsNeeded + Insert."""
    import math

    from reflector_ekf_slam_amd.map_builder import RangeData, transform_range_data, yaw_of_quaternion_f32
    max_xy, inserts, (prediction, _) = IC.map_scene()
    res, n = 0.05, 480
    first = (np.zeros((n, n), np.uint16), res, max_xy)
    m, gf = fleet(1, max_points=4096, max_cells=n * n, max_rotations=512), front_end(max_points=4096, max_cells=n * n, max_candidates=1 << 18)
    m.SetGrid(0, *first)
    gf.SetGrid(*first)
    for origin, world, misses in inserts:
        assert m.insert([(0, origin, world, misses)]) == [OK]
        gf.Insert(origin, world, misses)
    # the tick: the third insertion's scan seen from the prediction's frame, raw (3000 returns after doubling, 60 misses)
    from tests.grid_cases import room_grid, scan_of
    _, _, occ = room_grid()
    true = np.array([0.2, 0.1, 0.4])
    ret = scan_of(occ, true, n_points=3000, seed=78)
    ang = np.random.default_rng(79).uniform(-math.pi, math.pi, 60)
    mis = np.stack([5.0 * np.cos(ang), 3.5 * np.sin(ang)], 1).astype(np.float32)

    def moved(pose, fr, fm):
        ha = np.float32(np.float32(0.5) * np.float32(pose[2]))                     # MapBuilder.AddRangeData's range_data_in_local2
        yaw = yaw_of_quaternion_f32(math.cos(float(ha)), math.sin(float(ha)))
        return transform_range_data(RangeData(np.zeros(2, np.float32), fr, fm), (pose[0], pose[1]), yaw)

    r = m.filter([(ret, mis)])[0]
    fr, fm, av = FC.handle_triple(gf, (ret, mis))
    assert r.status == OK and FC.same_result(r, (fr, fm, av)) and FC.same_result(r, FC.oracle_triple((ret, mis)))
    assert 500 <= av.shape[0] < fr.shape[0] < ret.shape[0]
    sm = m.scan_match([(0, prediction, r.filtered)])[0]
    coarse = gf.Match(prediction, av)
    fine = gf.RefineMatch(prediction[:2], coarse.pose_estimate, av)
    assert sm.status == OK and MC.same_bits(sm.coarse, coarse) and RC.same_refine_bits(sm.fine, fine)
    a, b = moved(sm.pose_estimate, r.returns, r.misses), moved(fine.pose_estimate, fr, fm)
    assert m.insert([(0, a.origin, a.returns, a.misses)]) == [OK]
    gf.Insert(b.origin, b.returns, b.misses)
    lim = m.GetLimits(0)
    assert lim == gf.GetLimits()
    gf._grid_shape = (lim[1], lim[0])
    cells = m.GetGrid(0)
    assert np.array_equal(cells, gf.GetGrid()) and np.count_nonzero(cells) > 10000
    m.close(); gf.close()
