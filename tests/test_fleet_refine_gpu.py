"""The fleet refinement on the GPU (kgb_refine of csrc/rgrid_batch.hip behind ScanMatchFleet.refine and .scan_match): every scan
of a call bit for bit against GridFrontEnd.RefineMatch -- the specification -- and against oracle.binding.oracle_refine_match
with the tolerances of tests/test_grid_gpu.py::test_refine_match_follows_the_oracle_iterate_for_iterate (equal iterations and
termination, pose within 1e-8 or 1e-5 below 64 points, initial_cost within rel 1e-12, final_cost <= initial_cost)."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import fleet_match_cases as MC
from tests import fleet_refine_cases as RC

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, EMPTY = -1, -4, -6
MAX_POINTS = 2400


@pytest.fixture(scope="module")
def single():
    """One GridFrontEnd per grid slot of fleet_match_cases.grids()."""
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    hs = []
    for cells, res, max_xy, _ in MC.grids():
        g = GridFrontEnd(max_points=MAX_POINTS, max_cells=480 * 480, max_candidates=1 << 18)
        g.SetGrid(cells, res, max_xy)
        hs.append(g)
    yield hs
    for g in hs:
        g.close()


@pytest.fixture(scope="module")
def fm():
    from reflector_ekf_slam_amd import fleet_match as M
    m = M.ScanMatchFleet(max_scans=320, max_points=MAX_POINTS, num_grids=2, max_cells=480 * 480, max_rotations=512)
    for slot, (cells, res, max_xy, _) in enumerate(MC.grids()):
        m.SetGrid(slot, cells, res, max_xy)
    yield m
    m.close()


_shape_refine = None


def shape_refine_scans(single):
    """The shape case as refine scans: start poses from GridFrontEnd.Match, computed once and shared (never modified)."""
    global _shape_refine
    if _shape_refine is None:
        _shape_refine = [RC.refine_scan(s, single[s[0]].Match(s[1], s[2]).pose_estimate) for s in RC.shape_match_scans()]
    return _shape_refine


def single_refine(single, scan, opt=None):
    return single[scan[0]].RefineMatch(scan[1], scan[2], scan[3], opt)


@pytest.mark.parametrize("values", RC.OPTION_SETS, ids=["default", "heavy_monotonic", "three_iterations"])
def test_shape_sweep_bit_for_bit_in_any_order_and_alone(fm, single, values):
    opt = RC.options_of(values)
    scans = shape_refine_scans(single)
    assert len(scans) == len(RC.SHAPE_COUNTS) + 2
    want = [single_refine(single, s, opt) for s in scans]
    got = fm.refine(scans, opt)
    for k, (w, g) in enumerate(zip(want, got)):
        assert g.status == 0 and RC.same_refine_bits(g, w), (k, g, w)
    back = fm.refine(scans[::-1], opt)[::-1]                                       # other positions, the same launch block size
    alone = [fm.refine([s], opt)[0] for s in scans]                                # the launch's block size is the scan's own
    for k, w in enumerate(want):
        assert RC.same_refine_bits(back[k], w) and RC.same_refine_bits(alone[k], w), k
    if values == RC.OPTION_SETS[2]:
        assert any(g.termination == 1 and g.iterations == 3 for g in got)          # the iteration limit binds
    if values == RC.OPTION_SETS[0]:
        assert any(g.termination == 0 for g in got) and any(np.abs(g.pose_estimate - s[2]).max() > 1e-4 for g, s in zip(got, scans))


def test_against_the_oracle_in_one_batch_per_option_set(oracle_lib):
    from oracle.binding import oracle_refine_match
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import GridFrontEnd
    cells, res, max_xy, trials = RC.oracle_trials()
    assert [t[2].shape[0] for t in trials] == [3, 64, 500, 700, 2400, 5000]
    gf = GridFrontEnd(max_points=5000, max_cells=480 * 480, max_candidates=1 << 16)
    gf.SetGrid(cells, res, max_xy)
    m = M.ScanMatchFleet(max_scans=8, max_points=5000, num_grids=1, max_cells=480 * 480)
    m.SetGrid(0, cells, res, max_xy)
    scans = [(0, prediction[:2], gf.Match(prediction, pts).pose_estimate, pts) for _, prediction, pts in trials]
    far = (0, np.zeros(2), np.zeros(3), RC.FAR_CLOUD)
    for values in RC.OPTION_SETS:
        opt = RC.options_of(values)
        got = m.refine(scans + [far], opt)
        for trial, (s, r) in enumerate(zip(scans, got)):
            pose, summ = oracle_refine_match(s[1], s[2], s[3], cells, res, max_xy, opt.occupied_space_weight, opt.translation_weight,
                                             opt.rotation_weight, opt.max_num_iterations, opt.use_nonmonotonic_steps)
            assert r.status == 0
            assert (r.iterations, r.termination) == (summ["iterations"], summ["termination"]), (trial, values, r, summ)
            tol = 1e-8 if len(s[3]) >= 64 else 1e-5
            assert np.abs(r.pose_estimate - pose).max() < tol, (trial, r.pose_estimate - pose)
            assert r.initial_cost == pytest.approx(summ["initial_cost"], rel=1e-12) and r.final_cost == pytest.approx(summ["final_cost"], rel=tol)
            assert r.final_cost <= r.initial_cost
            assert RC.same_refine_bits(r, gf.RefineMatch(s[1], s[2], s[3], opt)), trial
        if not values:
            pose, summ = oracle_refine_match(far[1], far[2], far[3], cells, res, max_xy)
            r = got[-1]
            assert (r.iterations, r.termination) == (summ["iterations"], summ["termination"]) and np.abs(r.pose_estimate - pose).max() < 1e-12
            for (true, _, pts), r in zip(trials, got):
                if len(pts) >= 500:
                    assert np.abs(r.pose_estimate[:2] - true[:2]).max() < 0.03 and abs(r.pose_estimate[2] - true[2]) < 0.01
    m.close()
    gf.close()


@pytest.mark.parametrize("mode", ["arrival", "launch"])
def test_chained_match_then_refine(fm, single, mode):
    from reflector_ekf_slam_amd import fleet_match as M
    empty = (0, np.array([0.3, 0.2, 0.1]), np.zeros((0, 2), np.float32))
    shapes = MC.shape_scans()
    scans = MC.single_matcher_cases()[0] + shapes[:4] + [empty] + shapes[4:]
    at = 4 + 4
    fm.set_reduction(M.REDUCE_ARRIVAL if mode == "arrival" else M.REDUCE_LAUNCH)
    try:
        coarse = fm.match(scans)
        for round_ in range(2):                                                    # (twice: both staging segments)
            res = fm.scan_match(scans)
            assert len(res) == len(scans)
            for k, (s, c, r) in enumerate(zip(scans, coarse, res)):
                assert MC.same_bits(r.coarse, c), k
                if k == at:
                    continue
                assert r.status == 0 and r.fine.status == 0
                want = single[s[0]].RefineMatch(s[1][:2], c.pose_estimate, s[2])
                assert RC.same_refine_bits(r.fine, want), (k, r.fine, want)
                assert r.pose_estimate is r.fine.pose_estimate
            e = res[at]
            assert e.status == EMPTY == e.fine.status == e.coarse.status and RC.is_zero_refine(e.fine)
            assert e.coarse.score == 0.0 and not e.coarse.pose_estimate.any() and e.coarse.best == (0, 0, 0) and e.coarse.info == (0, 0, 0)
            assert M.pose_fixes(res)[at] is None and M.pose_fixes(res)[0] == tuple(res[0].fine.pose_estimate)
        # other options for both stages
        scan, mvalues = MC.options_case()
        mopt = M.RealTimeCorrelativeScanMatcherOptions(*mvalues)
        ropt = RC.options_of(RC.OPTION_SETS[1])
        r, = fm.scan_match([scan], mopt, ropt)
        c = single[scan[0]].Match(scan[1], scan[2], mopt)
        assert MC.same_bits(r.coarse, fm.match([scan], mopt)[0]) and r.coarse.pose_estimate.tobytes() == c.pose_estimate.tobytes()
        assert RC.same_refine_bits(r.fine, single[scan[0]].RefineMatch(scan[1][:2], c.pose_estimate, scan[2], ropt))
    finally:
        fm.set_reduction(M.REDUCE_ARRIVAL)


def test_many_scans_in_one_call_and_in_five(fm):
    base = MC.tile_scans(300, 64)
    scans = [(slot, pose[:2].copy(), pose, pts) for slot, pose, pts in base]
    opt = RC.options_of((1.0, 0.1, 0.4, 10, True))
    whole = fm.refine(scans, opt)
    assert len(whole) == 300 and all(r.status == 0 and 1 <= r.iterations <= 10 for r in whole)
    parts = [r for k in range(5) for r in fm.refine(scans[60 * k:60 * k + 60], opt)]
    assert all(RC.same_refine_bits(a, b) for a, b in zip(whole, parts))
    assert len({r.pose_estimate.tobytes() for r in whole}) == 300                  # (300 different answers, not one repeated)


def test_per_scan_status_and_whole_call_refusals(fm, single):
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import CeresScanMatcherOptions2D as RO
    mgood = MC.tile_scans(3, 64)
    rgood = [(slot, pose[:2].copy(), pose, pts) for slot, pose, pts in mgood]
    want_r = fm.refine(rgood)
    want_m = fm.match(mgood)
    want_s = fm.scan_match(mgood)
    for w, s in zip(want_r, rgood):
        assert RC.same_refine_bits(w, single_refine(single, s))

    def still_works():
        assert all(RC.same_refine_bits(a, b) for a, b in zip(fm.refine(rgood), want_r))
        got = fm.scan_match(mgood)
        assert all(MC.same_bits(a.coarse, b.coarse) and RC.same_refine_bits(a.fine, b.fine) for a, b in zip(got, want_s))

    # per-scan statuses
    rempty = (0, np.zeros(2), np.zeros(3), np.zeros((0, 2), np.float32))
    rtoo_many = (0, np.zeros(2), np.zeros(3), np.zeros((fm.max_points + 1, 2), np.float32))
    res = fm.refine([rgood[0], rempty, rgood[1], rtoo_many, rgood[2]])
    assert [r.status for r in res] == [0, EMPTY, 0, CAPACITY, 0]
    assert all(RC.same_refine_bits(a, b) for a, b in zip((res[0], res[2], res[4]), want_r))
    assert RC.is_zero_refine(res[1]) and RC.is_zero_refine(res[3])
    assert [r.status for r in fm.refine([rempty, rtoo_many])] == [EMPTY, CAPACITY]                     # a call that launches nothing
    assert fm.refine([]) == [] and fm.scan_match([]) == []
    mempty = (0, np.zeros(3), np.zeros((0, 2), np.float32))
    mtoo_many = (0, np.zeros(3), np.zeros((fm.max_points + 1, 2), np.float32))
    overflow = (1, np.zeros(3), np.array([[5000.0, 5000.0]], np.float32))          # more rotated scans than max_rotations
    res = fm.scan_match([mgood[0], mempty, mgood[1], mtoo_many, overflow, mgood[2]])
    assert [r.status for r in res] == [0, EMPTY, 0, CAPACITY, CAPACITY, 0] == [r.fine.status for r in res]
    for a, b in zip((res[0], res[2], res[5]), want_s):
        assert MC.same_bits(a.coarse, b.coarse) and RC.same_refine_bits(a.fine, b.fine)
    for r in (res[1], res[3], res[4]):
        assert RC.is_zero_refine(r.fine) and r.coarse.score == 0.0 and not r.coarse.pose_estimate.any()
    assert [r.status for r in fm.scan_match([mempty, mtoo_many])] == [EMPTY, CAPACITY]
    still_works()

    # whole-call refusals: what rgrid_batch_match_submit refuses ...
    for slot in (-1, 2):
        assert fm.submit_refine_code([rgood[0], (slot,) + rgood[1][1:]]) == INVALID
        assert fm.submit_scan_match_code([mgood[0], (slot,) + mgood[1][1:]]) == INVALID
    one = M.ScanMatchFleet(max_scans=2, max_points=64, num_grids=2, max_cells=480 * 480)
    cells, res05, max_xy, _ = MC.grids()[0]
    one.SetGrid(0, cells, res05, max_xy)
    assert one.submit_refine_code([(1,) + rgood[0][1:]]) == INVALID and one.submit_scan_match_code([(1,) + mgood[0][1:]]) == INVALID   # slot 1 is not set
    assert one.submit_refine_code(rgood) == INVALID and one.submit_scan_match_code(mgood) == INVALID                                   # count > max_scans
    assert one.collect_refine_code()[0] == INVALID and one.collect_scan_match_code()[0] == INVALID                                     # nothing was submitted
    assert RC.same_refine_bits(one.refine(rgood[:1])[0], want_r[0]) and RC.same_refine_bits(one.scan_match(mgood[:1])[0].fine, want_s[0].fine)
    one.close()
    still_works()
    # ... the refine options rgrid_refine_match refuses ...
    for bad in (RO(occupied_space_weight=0.0), RO(translation_weight=0.0), RO(rotation_weight=-1.0), RO(rotation_weight=float("nan")),
                RO(max_num_iterations=-1)):
        assert fm.submit_refine_code(rgood, bad) == INVALID and fm.submit_scan_match_code(mgood, None, bad) == INVALID, bad
        with pytest.raises(M.RgridError):
            single[0].RefineMatch(rgood[0][1], rgood[0][2], rgood[0][3], bad)
    still_works()
    assert fm.refine(rgood[:1], RO(max_num_iterations=0))[0].iterations == 0       # (0 iterations is allowed)
    # ... and a pending submit of any kind; a collect of another kind leaves it pending
    submits = {"match": lambda: fm.submit_code(mgood), "refine": lambda: fm.submit_refine_code(rgood),
               "scan_match": lambda: fm.submit_scan_match_code(mgood)}
    collects = {"match": fm.collect_code, "refine": fm.collect_refine_code, "scan_match": fm.collect_scan_match_code}
    for kind in submits:
        assert submits[kind]() == 0
        for other in submits:
            assert submits[other]() == INVALID, (kind, other)
        assert fm.SetGrid_code(0, cells, res05, max_xy) == INVALID                 # no grid changes under a launch
        with pytest.raises(M.RgridError):
            fm.set_reduction(M.REDUCE_LAUNCH)
        for other in collects:
            if other != kind:
                assert collects[other]()[0] == INVALID, (kind, other)
        rc, out = collects[kind]()
        assert rc == 0 and len(out) == 3
        if kind == "match":
            assert all(MC.same_bits(a, b) for a, b in zip(out, want_m))
        elif kind == "refine":
            assert all(RC.same_refine_bits(a, b) for a, b in zip(out, want_r))
        else:
            assert all(MC.same_bits(a.coarse, b.coarse) and RC.same_refine_bits(a.fine, b.fine) for a, b in zip(out, want_s))
        assert collects[kind]()[0] == INVALID                                      # collected: nothing is pending
    still_works()
    assert fm.last_prepare_seconds() > 0.0


def test_a_pending_submit_of_any_of_the_six_kinds_refuses_everything_but_its_own_collect():
    """Kind x kind over match, refine, scan_match, insert, filter and texture, each pending once with a launch and once as a submit
    whose every scan is refused (nothing is launched, the collect gives the per-scan statuses): every submit, every other collect,
    SetGrid, set_reduction, GetLimits and GetGrid are refused and leave it pending; its own collect succeeds once."""
    from reflector_ekf_slam_amd import fleet_match as M
    from tests import fleet_filter_scan_cases as FC
    from tests import fleet_texture_cases as TC
    grids = MC.grids()
    spare = 2                                                                      # the insert's slot: no match or texture names it
    m = M.ScanMatchFleet(max_scans=4, max_points=64, num_grids=3, max_cells=480 * 480)
    for slot in (0, 1, spare):
        m.SetGrid(slot, *grids[slot % 2][:3])
    mgood = MC.tile_scans(3, 64)
    rgood = [(slot, pose[:2].copy(), pose, pts) for slot, pose, pts in mgood]
    igood = [(spare, (0.0, 0.0), grids[0][3][:40].astype(np.float32), None)]
    fgood = [(pts, None) for _, _, pts in mgood]
    tgood = [0, 1, 0]
    # what each kind gives with nothing else going on, computed once
    want = {"match": m.match(mgood), "refine": m.refine(rgood), "scan_match": m.scan_match(mgood), "filter": m.filter(fgood),
            "texture": m.draw_textures(tgood)}
    assert m.insert(igood) == [0]
    inserted = m.GetGrid(spare)
    assert not np.array_equal(inserted, grids[0][0])
    m.SetGrid(spare, *grids[0][:3])
    same = {"match": lambda out, w: all(MC.same_bits(a, b) for a, b in zip(out, w)),
            "refine": lambda out, w: all(RC.same_refine_bits(a, b) for a, b in zip(out, w)),
            "scan_match": lambda out, w: all(MC.same_bits(a.coarse, b.coarse) and RC.same_refine_bits(a.fine, b.fine) for a, b in zip(out, w)),
            "filter": lambda out, w: all(FC.same_results(a, b) for a, b in zip(out, w)),
            "texture": lambda out, w: all(TC.same_texture(a, b) for a, b in zip(out, w))}
    submits = {"match": lambda: m.submit_code(mgood), "refine": lambda: m.submit_refine_code(rgood),
               "scan_match": lambda: m.submit_scan_match_code(mgood), "insert": lambda: m.submit_insert_code(igood),
               "filter": lambda: m.submit_filter_code(fgood), "texture": lambda: m.submit_texture_code(tgood)}
    collects = {"match": m.collect_code, "refine": m.collect_refine_code, "scan_match": m.collect_scan_match_code,
                "insert": m.collect_insert_code, "filter": m.collect_filter_code, "texture": m.collect_texture_code}
    # a submit of each kind that launches nothing, and the statuses its collect gives (the texture has no per-slot refusal: no slot)
    none, too_many, nan = np.zeros((0, 2), np.float32), np.zeros((65, 2), np.float32), np.array([[np.nan, 0.0]], np.float32)
    refused = {"match": (lambda: m.submit_code([(0, np.zeros(3), none), (0, np.zeros(3), too_many)]), [EMPTY, CAPACITY]),
               "refine": (lambda: m.submit_refine_code([(0, np.zeros(2), np.zeros(3), none), (0, np.zeros(2), np.zeros(3), too_many)]), [EMPTY, CAPACITY]),
               "scan_match": (lambda: m.submit_scan_match_code([(0, np.zeros(3), none), (0, np.zeros(3), too_many)]), [EMPTY, CAPACITY]),
               "insert": (lambda: m.submit_insert_code([(spare, (0.0, 0.0), nan, None), (0, (0.0, 0.0), np.array([[500.0, 0.0]], np.float32), None)]),
                          [INVALID, CAPACITY]),
               "filter": (lambda: m.submit_filter_code([(too_many, None), (nan, None)]), [CAPACITY, INVALID]),
               "texture": (lambda: m.submit_texture_code([]), [])}
    room = np.zeros(480 * 480, np.uint16)

    def everything_else_is_refused(kind):
        for other in submits:
            assert submits[other]() == INVALID, (kind, other)
        assert m.SetGrid_code(0, *grids[0][:3]) == INVALID                          # no grid changes under a launch
        with pytest.raises(M.RgridError):
            m.set_reduction(M.REDUCE_LAUNCH)
        assert m.GetLimits_code(0)[0] == INVALID and m.GetGrid_code(0)[0] == INVALID
        assert M._insert_lib().rgrid_batch_get_grid(m._h, 0, room.ctypes.data, room.size) == INVALID
        for other in collects:
            if other != kind:
                assert collects[other]()[0] == INVALID, (kind, other)

    for kind in submits:
        assert submits[kind]() == 0
        everything_else_is_refused(kind)
        rc, out = collects[kind]()                                                 # ... and all of that left it pending
        assert rc == 0 and len(out) == len(igood if kind == "insert" else mgood)
        if kind == "insert":
            assert out == [0] and np.array_equal(m.GetGrid(spare), inserted)
            m.SetGrid(spare, *grids[0][:3])
        else:
            assert same[kind](out, want[kind]), kind
        assert collects[kind]()[0] == INVALID                                      # collected: nothing is pending
        submit, statuses = refused[kind]
        assert submit() == 0
        everything_else_is_refused(kind)
        rc, out = collects[kind]()
        assert rc == 0 and [r if kind == "insert" else r.status for r in out] == statuses, kind
        assert collects[kind]()[0] == INVALID
    for slot in (0, 1, spare):                                                     # no refused scan touched its slot
        assert np.array_equal(m.GetGrid(slot), grids[slot % 2][0])
    for kind in want:
        assert submits[kind]() == 0
        rc, out = collects[kind]()
        assert rc == 0 and same[kind](out, want[kind]), kind
    m.close()


def test_end_to_end_into_the_fleet_filter():
    """predict_poses -> ScanMatchFleet.scan_match -> pose_fixes -> scan_event(pose_fix=...) -> submit for six members, against a
    twin fleet whose fixes come from six GridFrontEnd handles (Match, then RefineMatch): the same bits in mu and in the pose
    blocks.  The fix is the refined pose: in some tick it differs from the matcher's for every robot."""
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
    warm = max(next(k for k in range(len(x.events)) if sum(ev[0] == FC.EV_SCAN for ev in x.events[:k]) == 3) for x in ss)
    for fl in fleets:
        for k in range(warm):
            fl.submit([FC.fev(i, s.events[k], with_fix=False) for i, s in enumerate(ss)])
    centre = fleets[0].poses()[1][:, :2].copy()
    for i in range(6):
        mx = (max_xy[0] + centre[i, 0], max_xy[1] + centre[i, 1])
        matcher.SetGrid(i, cells, res, mx)
        handles[i].SetGrid(cells, res, mx)
    rng = np.random.default_rng(31)
    ticks = matched = all_moved = 0
    moved_robots = set()
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
                true = pred[0][i] + rng.normal(size=3) * (0.04, 0.04, 0.02)
                local = true - np.array([centre[i, 0], centre[i, 1], 0.0])
                scans.append((i, pred[0][i], scan_of(occ, local, n_points=200, seed=300 + 10 * k + i)))
                trues.append(true)
            results = matcher.scan_match(scans)
            fixes = M.pose_fixes(results)
            twin = []
            for i, pose, pts in scans:
                c = handles[i].Match(pose, pts)
                twin.append((c, handles[i].RefineMatch(pose[:2], c.pose_estimate, pts)))
            moved = 0
            for i, r, (c, f), fix, true in zip(who, results, twin, fixes, trues):
                assert r.status == 0 and MC.same_bits(r.coarse, c) and RC.same_refine_bits(r.fine, f)
                assert fix == tuple(f.pose_estimate)
                assert np.abs(f.pose_estimate[:2] - true[:2]).max() <= 0.2 and abs(f.pose_estimate[2] - true[2]) <= math.radians(15.0)
                if fix != tuple(c.pose_estimate):
                    moved += 1
                    moved_robots.add(i)
                matched += 1
            all_moved += moved == len(who)
            tick[0] += [F.scan_event(i, evs[i][1], evs[i][3], pose_fix=f) for i, f in zip(who, fixes)]
            tick[1] += [F.scan_event(i, evs[i][1], evs[i][3], pose_fix=tuple(f.pose_estimate)) for i, (_, f) in zip(who, twin)]
            ticks += 1
        for fl, events in zip(fleets, tick):
            fl.submit(events)
    assert ticks == 4 and matched >= 18 and fleets[0].n().min() > 3
    assert all_moved >= 1 and moved_robots == set(range(6))                        # with the refinement absent: 0 ticks, no robot
    pa, pb = fleets[0].poses(), fleets[1].poses()
    assert all(np.array_equal(a, b) for a, b in zip(pa, pb))
    for i in range(6):
        assert FC.same_bits(FC.state_bits(fleets[0], i), FC.state_bits(fleets[1], i)), i
    for fl in fleets:
        fl.close()
    for h in handles:
        h.close()
    matcher.close()
