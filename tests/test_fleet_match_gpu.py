"""The fleet scan matcher (rgrid_batch_* of include/rgrid.h, csrc/rgrid_batch.hip) on the GPU: every scan of a call against
oracle.binding.oracle_match and, bit for bit, against GridFrontEnd.Match.

Tolerances (tests/test_grid_gpu.py::test_match_identical_candidate_and_score): against the oracle identical best and info,
|score - oracle| <= 1.2e-7 score, pose within 1e-12; against the single handle exact equality of score bits, pose, best and
info -- the arithmetic is the same device code.  Every test on the shared handle runs with both forms of the reduction over the
rotated scans (rgrid_batch_set_reduction); the end-to-end test takes the default."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import fleet_match_cases as MC

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, EMPTY = -1, -4, -6


@pytest.fixture(scope="module")
def single():
    """One GridFrontEnd per grid slot of fleet_match_cases.grids()."""
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    hs = []
    for cells, res, max_xy, _ in MC.grids():
        g = GridFrontEnd(max_points=1024, max_cells=480 * 480, max_candidates=1 << 18)
        g.SetGrid(cells, res, max_xy)
        hs.append(g)
    yield hs
    for g in hs:
        g.close()


@pytest.fixture(scope="module", params=["arrival", "launch"])
def fm(request):
    from reflector_ekf_slam_amd import fleet_match as M
    m = M.ScanMatchFleet(max_scans=320, max_points=1024, num_grids=2, max_cells=480 * 480, max_rotations=512)
    m.set_reduction(M.REDUCE_ARRIVAL if request.param == "arrival" else M.REDUCE_LAUNCH)
    for slot, (cells, res, max_xy, _) in enumerate(MC.grids()):
        m.SetGrid(slot, cells, res, max_xy)
    yield m
    m.close()


_oracle_cache = {}


def oracle(key, scan, option_values=None):
    """The oracle's answer for a scan, computed once per session and shared (never modified)."""
    if key not in _oracle_cache:
        _oracle_cache[key] = MC.oracle_of(scan, option_values)
    return _oracle_cache[key]


def options_of(values):
    from reflector_ekf_slam_amd.grid import RealTimeCorrelativeScanMatcherOptions
    return RealTimeCorrelativeScanMatcherOptions(*values) if values else None


def single_match(single, scan, option_values=None):
    return single[scan[0]].Match(scan[1], scan[2], options_of(option_values))


def test_single_matcher_cases_in_one_call(fm, single, oracle_lib):
    scans, trues = MC.single_matcher_cases()
    res = fm.match(scans)
    assert len(res) == 4
    for k, (scan, true, r) in enumerate(zip(scans, trues, res)):
        o = oracle(("single", k), scan)
        MC.check_against_oracle(r, o)
        assert MC.same_bits(r, single_match(single, scan)), k
        assert np.abs(o[1][:2] - true[:2]).max() <= 0.1
    scan, values = MC.options_case()
    r, = fm.match([scan], options_of(values))
    o = oracle(("options",), scan, values)
    MC.check_against_oracle(r, o)
    assert r.info[1] == 4                                                          # ceil(0.35 / 0.1)
    assert MC.same_bits(r, single_match(single, scan, values))


def test_shapes_mixed_in_one_call_over_two_grids(fm, single, oracle_lib):
    scans = MC.shape_scans()
    assert [s[2].shape[0] for s in scans[:7]] == [1, 15, 16, 17, 33, 300, 900]
    assert 0.05 < MC.partly_outside_fraction(scans[7]) < 0.95
    assert MC.grids()[0][0][5, 100:140].min() >= 32768                             # update-marker cells in the 0.05 m grid
    values = (0.35, math.radians(15.0), 1e-1, 1e-1)                                # 0.35 m at 0.05 m: 15 x 15 = 225 candidates, two passes of 128
    res = fm.match(scans, options_of(values))
    for k, (scan, r) in enumerate(zip(scans, res)):
        MC.check_against_oracle(r, oracle(("shape", k), scan, values))
        assert MC.same_bits(r, single_match(single, scan, values)), k
    assert (res[0].info[1], res[1].info[1]) == (7, 4)                              # num_linear differs per scan ...
    assert len({r.info[0] for r in res}) >= 4                                      # ... and so does the rotation count
    assert res[8].info[0] > 256                                                    # (a reduction over more block bests than threads)
    for r in res[8:]:                                                              # wholly outside: kMinProbability everywhere
        assert r.best[1:] == (0, 0) and abs(r.score - 0.1) < 1e-6
    # the default window (one pass of 81 candidates) on the same scans
    res = fm.match(scans)
    for k, (scan, r) in enumerate(zip(scans, res)):
        MC.check_against_oracle(r, oracle(("shape_default", k), scan))
        assert MC.same_bits(r, single_match(single, scan)), k


def test_first_maximum_across_workgroups(fm, single, oracle_lib):
    far = np.array([[30.0, 30.0], [31.0, 29.0]], np.float32)
    scan = (0, np.array([0.1, -0.2, 0.3]), far)
    # both weights 0: every candidate of every rotated scan ties -> candidate id 0
    values = (0.2, math.radians(15.0), 0.0, 0.0)
    r, = fm.match([scan], options_of(values))
    o = oracle(("tie_all",), scan, values)
    MC.check_against_oracle(r, o)
    assert r.info[0] > 1 and r.best == (0, -r.info[1], -r.info[1]) == o[2]
    assert MC.same_bits(r, single_match(single, scan, values))
    # a rotation weight: the tie is within the middle rotated scan only -> its first candidate
    values = (0.2, math.radians(15.0), 0.0, 0.5)
    r, = fm.match([scan], options_of(values))
    o = oracle(("tie_rot",), scan, values)
    MC.check_against_oracle(r, o)
    assert r.best == ((r.info[0] - 1) // 2, -r.info[1], -r.info[1]) == o[2]
    assert MC.same_bits(r, single_match(single, scan, values))


def test_position_independence_and_more_work_than_the_chip_holds(fm, oracle_lib):
    base = MC.tile_scans(12, 64)
    order = np.random.default_rng(5).permutation(300) % 12
    res = fm.match([base[q] for q in order])
    assert len(res) == 300 and res[0].info[0] * 300 > 256 * 16                    # more workgroups than the chip holds at once
    alone = [fm.match([s])[0] for s in base]
    for k, s in enumerate(base):
        MC.check_against_oracle(alone[k], oracle(("tile", k), s))
    for q, r in zip(order, res):
        assert MC.same_bits(r, alone[q])
    others = [base[(k + 1) % 12] for k in range(40)]
    for k in (0, 5, 11):
        assert MC.same_bits(fm.match([base[k]] + others)[0], alone[k])            # first
        assert MC.same_bits(fm.match(others + [base[k]])[-1], alone[k])           # last


def test_per_scan_status_and_whole_call_refusals(fm):
    from reflector_ekf_slam_amd import fleet_match as M
    good = MC.tile_scans(3, 64)
    empty = (0, np.zeros(3), np.zeros((0, 2), np.float32))
    too_many = (0, np.zeros(3), np.zeros((fm.max_points + 1, 2), np.float32))
    overflow = (1, np.zeros(3), np.array([[5000.0, 5000.0]], np.float32))         # more rotated scans than max_rotations
    want = fm.match(good)
    res = fm.match([good[0], empty, good[1], too_many, overflow, good[2]])
    assert [r.status for r in res] == [0, EMPTY, 0, CAPACITY, CAPACITY, 0]
    for a, b in zip((res[0], res[2], res[5]), want):
        assert MC.same_bits(a, b)
    for r in (res[1], res[3], res[4]):
        assert r.score == 0.0 and not r.pose_estimate.any() and r.best == (0, 0, 0) and r.info == (0, 0, 0)
    assert M.pose_fixes(res)[1] is None and M.pose_fixes(res)[0] == tuple(res[0].pose_estimate)
    assert [r.status for r in fm.match([empty, too_many])] == [EMPTY, CAPACITY]  # a call that launches nothing
    assert fm.match([]) == []

    def still_works():
        assert all(MC.same_bits(a, b) for a, b in zip(fm.match(good), want))

    one = M.ScanMatchFleet(max_scans=2, max_points=64, num_grids=2, max_cells=480 * 480)
    cells, res05, max_xy, _ = MC.grids()[0]
    one.SetGrid(0, cells, res05, max_xy)
    assert one.submit_code([(1, good[0][1], good[0][2])]) == INVALID               # slot 1 is not set
    assert one.submit_code(good) == INVALID                                        # count > max_scans
    assert one.collect_code()[0] == INVALID                                        # nothing was submitted
    assert MC.same_bits(one.match(good[:1])[0], want[0])
    one.close()
    for slot in (-1, 2):
        assert fm.submit_code([good[0], (slot, good[1][1], good[1][2])]) == INVALID   # out of range
        still_works()
    assert fm.collect_code()[0] == INVALID                                         # collect without a submit
    still_works()
    fm.submit(good)
    assert fm.submit_code(good) == INVALID                                         # double submit
    assert fm.SetGrid_code(0, cells, res05, max_xy) == INVALID                     # ... and no grid changes under a launch
    assert all(MC.same_bits(a, b) for a, b in zip(fm.collect(), want))
    still_works()
    # windows whose counts no int holds, negative or NaN windows: rgrid_match's answer, for every scan of the call (options are per call)
    far = (0, np.zeros(3), np.array([[30.0, 30.0], [31.0, 29.0]], np.float32))
    for window in (dict(linear_search_window=1e12), dict(linear_search_window=-0.1), dict(angular_search_window=-0.1),
                   dict(angular_search_window=float("nan"))):
        res = fm.match([good[0], far], M.RealTimeCorrelativeScanMatcherOptions(**window))
        assert [r.status for r in res] == [CAPACITY, CAPACITY], window
        still_works()
    big = M.ScanMatchFleet(max_scans=1, max_points=64, max_cells=480 * 480, max_rotations=2000)
    big.SetGrid(0, cells, res05, max_xy)
    assert big.match(good[:1])[0].status == CAPACITY                               # max_rotations > 1024: rgrid_match's limit
    big.close()


def test_two_rounds_with_a_grid_changed_between_them(fm, single, oracle_lib):
    from oracle.binding import oracle_match
    scans = MC.tile_scans(12, 64)[:6]
    first = fm.match(scans)
    cells, res, max_xy, _ = MC.grids()[0]
    changed = np.ascontiguousarray(cells[::-1, ::-1])                              # the room turned by half a turn
    fm.SetGrid(0, changed, res, max_xy)
    single[0].SetGrid(changed, res, max_xy)
    try:
        second = fm.match(scans[::-1])[::-1]
        differs = 0
        for k, (scan, r) in enumerate(zip(scans, second)):
            if ("changed", k) not in _oracle_cache:
                _oracle_cache[("changed", k)] = oracle_match(scan[1], scan[2], changed, res, max_xy)
            MC.check_against_oracle(r, _oracle_cache[("changed", k)])
            assert MC.same_bits(r, single[0].Match(scan[1], scan[2]))
            differs += not MC.same_bits(r, first[k])
        assert differs == len(scans)                                               # nothing of the first round is left
    finally:
        fm.SetGrid(0, cells, res, max_xy)
        single[0].SetGrid(cells, res, max_xy)
    third = fm.match(scans)
    assert all(MC.same_bits(a, b) for a, b in zip(third, first))


def test_end_to_end_into_the_fleet_filter():
    """predict_poses -> ScanMatchFleet.match -> scan_event(pose_fix=...) -> submit for six members, against a twin fleet whose
    fixes come from six GridFrontEnd.Match calls: the same bits in mu and in the pose blocks."""
    from reflector_ekf_slam_amd import fleet as F
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    from tests import fleet_cases as FC
    from tests import fleet_pose_cases as PC
    from tests.grid_cases import scan_of
    ss = [PC.sessions()[i % 4] for i in range(6)]
    fleets = [F.ReflectorEKFSLAMFleet([s.options for s in ss], max_landmarks=32) for _ in (0, 1)]
    cells, res, max_xy, occ = MC.grids()[0]
    matcher = M.ScanMatchFleet(max_scans=6, max_points=256, num_grids=6, max_cells=480 * 480)
    handles = [GridFrontEnd(max_points=256, max_cells=480 * 480, max_candidates=1 << 16) for _ in range(6)]
    # the events that build each member's small map: up to every member's third scan
    warm = max(next(k for k in range(len(x.events)) if sum(ev[0] == FC.EV_SCAN for ev in x.events[:k]) == 3) for x in ss)
    for fl in fleets:
        for k in range(warm):
            fl.submit([FC.fev(i, s.events[k], with_fix=False) for i, s in enumerate(ss)])
    # every member's occupancy map: the room, centred where the member is now
    centre = fleets[0].poses()[1][:, :2].copy()
    for i in range(6):
        mx = (max_xy[0] + centre[i, 0], max_xy[1] + centre[i, 1])
        matcher.SetGrid(i, cells, res, mx)
        handles[i].SetGrid(cells, res, mx)
    rng = np.random.default_rng(31)
    ticks = matched = 0
    for k in range(warm, min(len(x.events) for x in ss)):
        if ticks == 4:
            break
        evs = [s.events[k] for s in ss]
        who = [i for i, ev in enumerate(evs) if ev[0] == FC.EV_SCAN]
        tick = [[FC.fev(i, ev, with_fix=False) for i, ev in enumerate(evs) if ev[0] != FC.EV_SCAN] for _ in (0, 1)]
        if who:
            t_now = fleets[0].poses()[0]
            times = np.array([evs[i][1] if i in who else t_now[i] for i in range(6)])
            pred = [fl.predict_poses(times)[0] for fl in fleets]
            assert np.array_equal(pred[0], pred[1])
            scans, trues = [], []
            for i in who:
                true = pred[0][i] + rng.normal(size=3) * (0.04, 0.04, 0.02)        # where the robot is: near the prediction
                local = true - np.array([centre[i, 0], centre[i, 1], 0.0])
                scans.append((i, pred[0][i], scan_of(occ, local, n_points=200, seed=300 + 10 * k + i)))
                trues.append(true)
            results = matcher.match(scans)
            fixes = M.pose_fixes(results)
            twin = [handles[i].Match(pose, pts) for i, pose, pts in scans]
            for i, r, t, true in zip(who, results, twin, trues):
                assert r.status == 0 and MC.same_bits(r, t)
                assert np.abs(r.pose_estimate[:2] - true[:2]).max() <= 0.2 and abs(r.pose_estimate[2] - true[2]) <= math.radians(15.0)
                matched += 1
            tick[0] += [F.scan_event(i, evs[i][1], evs[i][3], pose_fix=f) for i, f in zip(who, fixes)]
            tick[1] += [F.scan_event(i, evs[i][1], evs[i][3], pose_fix=tuple(t.pose_estimate)) for i, t in zip(who, twin)]
            ticks += 1
        for fl, events in zip(fleets, tick):
            fl.submit(events)
    assert ticks == 4 and matched >= 18 and fleets[0].n().min() > 3
    pa, pb = fleets[0].poses(), fleets[1].poses()
    assert all(np.array_equal(a, b) for a, b in zip(pa, pb))
    for i in range(6):
        assert FC.same_bits(FC.state_bits(fleets[0], i), FC.state_bits(fleets[1], i)), i
    for fl in fleets:
        fl.close()
    for h in handles:
        h.close()
    matcher.close()
