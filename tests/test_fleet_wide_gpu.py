"""Fleet filter, wide scans on the GPU (-m gpu): k_fleet_step_wide against the longdouble JOINT witness on the cases of
tests/fleet_wide_cases.py, the bits of narrow members and of call patterns, which kernel a submit launches, the limits, the pose
track's counts, FleetNode(wide_scans=True), and whose match record last_match reads behind every kind of launch.

Worst figures of the lockstep run on an MI355X, as multiples of the suite's measured FP64 floor (bound: 16; printed by
test_every_case_against_the_joint_witness, run with -s): sigma 1.30 x (wide_L128_MM63_N0_omni), mu 12.26 x (wide_tall_L1_MM40: 40
observations of one reflector, n = 5), 4.39 x (wide_tall_L2_MM40), every other case below 2 x."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as FM
from tests import fleet_wide_cases as WC

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_TOO_MANY_OBS, ERR_BUFFER = -1, -3, -6


def test_every_case_against_the_joint_witness():
    """All cases as members of one wide-enabled fleet (one per capacity): lists equal the claim, sigma exactly symmetric, state
    within GPU_FACTOR x the measured floor of the joint longdouble witness."""
    worst_s, worst_m, misses = WC.run_lockstep(WC.all_cases())
    print(f"\nworst of {len(WC.all_cases())} wide cases: sigma {worst_s[0]:.2f} x the floor at {worst_s[1]}; mu {worst_m[0]:.2f} x at {worst_m[1]}")
    assert not misses, "\n".join(misses)
    assert 0 < worst_s[0] <= FC.GPU_FACTOR and 0 < worst_m[0] <= FC.GPU_FACTOR


# ---- the bits of narrow members beside a wide one ------------------------------------------------------------------------------
def two_wide_scans():
    """A plain member with a wide scan in each of two ticks, so that both ticks of its fleet are wide launches."""
    lms = FC.far_lattice(40)
    s0 = [("s", j, WC.spread(lms[j], j)) for j in range(40)]
    s1 = [("s", j, WC.spread(lms[j], j + 9)) for j in range(39, -1, -1)]
    return WC.built("wide_two_scans", lms, [s0, s1], 9780, False, fixes=[None, FM.FIX])


def narrow_members():
    """Narrow members of every kind: plain, plain with a fix, on the map with a fix (fix_first), on the map over two scans."""
    plain = [WC.on_std_map(c, False) for c in FC.plain_neighbours()]
    lms = FC.far_lattice(8)
    fixed = WC.built("narrow_fix_plain", lms, [[("s", j) for j in range(6)] + [("n", FM.new_lattice(1)[0])]], 9781, False, fixes=[FM.FIX])
    return plain + [fixed, FM.fix_cases()[2], FM.two_scan_case()]


@pytest.mark.parametrize("with_fix,with_map,track", [(f, m, t) for f in (False, True) for m in (False, True) for t in (False, True)])
def test_narrow_members_keep_their_bits_beside_a_wide_member(with_fix, with_map, track):
    narrow, wide = narrow_members(), two_wide_scans()
    fa = WC.make_fleet([wide] + narrow, wide=True, with_map=with_map, track=track)
    fb = WC.make_fleet(narrow, wide=False, with_map=with_map, track=track)
    try:
        for k in range(2):
            fa.submit([FC.fev(0, wide.events[k], with_fix)] + [FC.fev(1 + i, c.events[k], with_fix) for i, c in enumerate(narrow) if k < len(c.events)])
            fb.submit([FC.fev(i, c.events[k], with_fix) for i, c in enumerate(narrow) if k < len(c.events)])
            assert fa.wide_counts() == (k + 1, k + 1) and fb.wide_counts() == (0, 0)
            for i, c in enumerate(narrow):
                assert FC.same_bits(FC.state_bits(fa, 1 + i), FC.state_bits(fb, i)), (c.name, k)
                a, b = fa.last_match(1 + i), fb.last_match(i)
                assert all(np.array_equal(x, y) for x, y in zip(H.norm_match(a), H.norm_match(b))), (c.name, k)
        assert (fa.flags()[1:] == fb.flags()).all() and (fa.n()[1:] == fb.n()).all()
        assert int(fa.n()[0]) == wide.mu.shape[0]
    finally:
        fa.close()
        fb.close()


# ---- the bits of the wide member in every call pattern -------------------------------------------------------------------------
def wide_tick():
    """A member's tick: odometry, a wide scan (33 matched, 33 new), a following narrow scan."""
    c = next(c for c in WC.all_cases() if c.name.startswith("wideaug_"))
    odom = (FC.EV_ODOM, c.t + 0.05, c.vt, None, None)
    return c, [odom, c.events[0], c.events[1]]


def test_the_wide_member_has_the_same_bits_in_every_call_pattern():
    c, events = wide_tick()
    others = [x for x in WC.all_cases() if x.max_landmarks == 128 and x is not c][:7]
    runs = {}
    for name, members, at, split in (("alone", [c], 0, False), ("among 7", others[:3] + [c] + others[3:], 3, False), ("three submits", [c], 0, True)):
        fl = WC.make_fleet(members)
        try:
            mine = [FC.fev(at, ev) for ev in events]
            rest = [FC.fev(i, m.events[0]) for i, m in enumerate(members) if i != at]
            if split:
                for ev in mine:
                    fl.submit([ev])
                assert fl.wide_counts() == (1, 1)
            else:
                fl.submit(rest[:2] + mine[:1] + rest[2:4] + mine[1:] + rest[4:])
                assert fl.wide_counts()[0] == 1
            runs[name] = (FC.state_bits(fl, at), H.norm_match(fl.last_match(at)), int(fl.flags()[at]))
        finally:
            fl.close()
    ref = runs["alone"]
    assert ref[0][0].shape[0] == c.mu.shape[0] + 2 * 33 + 2
    for name, got in runs.items():
        assert FC.same_bits(got[0], ref[0]), name
        assert all(np.array_equal(x, y) for x, y in zip(got[1], ref[1])) and got[2] == ref[2], name


# ---- which kernel a submit launches ---------------------------------------------------------------------------------------------
def test_a_fleet_with_wide_scans_on_launches_the_narrow_kernels_for_narrow_scans():
    narrow = narrow_members()
    fa, fb = WC.make_fleet(narrow, wide=True), WC.make_fleet(narrow, wide=False)
    try:
        for k in range(2):
            for fl in (fa, fb):
                fl.submit([FC.fev(i, c.events[k]) for i, c in enumerate(narrow) if k < len(c.events)])
        assert fa.wide_counts() == (0, 0) == fb.wide_counts()
        for i, c in enumerate(narrow):
            assert FC.same_bits(FC.state_bits(fa, i), FC.state_bits(fb, i)), c.name
            assert all(np.array_equal(x, y) for x, y in zip(H.norm_match(fa.last_match(i)), H.norm_match(fb.last_match(i)))), c.name
        lms = np.asarray(FC.far_lattice(33), np.float32)
        fa.submit([(0, FC.EV_SCAN, 60.0, (0.0, 0.0, 0.0), lms)])
        assert fa.wide_counts() == (1, 1)
        fa.submit([(1, FC.EV_SCAN, 60.0, (0.0, 0.0, 0.0), lms[:32])])
        assert fa.wide_counts() == (1, 1)
    finally:
        fa.close()
        fb.close()


# ---- limits ----------------------------------------------------------------------------------------------------------------------
def _last_match_codes(fl, member, cap, wide):
    """-> (code, counts, the lists' buffers) of rfleet_get_last_match (wide = False) or rfleet_get_last_match_wide."""
    fleet = H.fleet_mod()
    sp, mp, nw = (np.full((max(cap, 1), 2), -7, np.int32), np.full((max(cap, 1), 2), -7, np.int32), np.full(max(cap, 1), -7, np.int32))
    ns, nm, nn = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    if wide:
        rc = fleet._wide_lib().rfleet_get_last_match_wide(fl._h, member, cap, C.byref(ns), sp.ctypes.data, C.byref(nm), mp.ctypes.data,
                                                          C.byref(nn), nw.ctypes.data)
    else:
        rc = fl._L.rfleet_get_last_match(fl._h, member, C.byref(ns), sp.ctypes.data, C.byref(nm), mp.ctypes.data, C.byref(nn), nw.ctypes.data)
    return rc, (ns.value, nm.value, nn.value), (sp, mp, nw)


def test_limits():
    fleet = H.fleet_mod()
    cases = narrow_members()[:3]
    far = np.asarray(FC.far_lattice(160), np.float32)
    cloud = lambda K: np.ascontiguousarray(np.concatenate([far, far + np.float32(0.25)])[:K])
    ev = lambda m, K, t=60.0: (m, FC.EV_SCAN, t, (0.0, 0.0, 0.0), cloud(K))
    off, on = WC.make_fleet(cases, wide=False), WC.make_fleet(cases, wide=True)
    try:
        before = [FC.state_bits(off, i) for i in range(3)]
        assert off.submit_code([FC.fev(0, cases[0].events[0]), ev(1, 33)]) == ERR_TOO_MANY_OBS
        assert all(FC.same_bits(FC.state_bits(off, i), before[i]) for i in range(3)) and off.wide_counts() == (0, 0)
        before = [FC.state_bits(on, i) for i in range(3)]
        assert on.submit_code([FC.fev(0, cases[0].events[0]), ev(1, 257)]) == ERR_TOO_MANY_OBS
        assert all(FC.same_bits(FC.state_bits(on, i), before[i]) for i in range(3)) and on.wide_counts() == (0, 0)
        assert (on.poses()[0] == [c.t for c in cases]).all()
        assert on.submit_code([ev(1, 256)]) == 0 and on.wide_counts() == (1, 1)
        L1 = (cases[1].mu.shape[0] - 3) // 2
        m = on.last_match(1)
        counts = tuple(len(x) for x in H.norm_match(m))
        assert sum(counts) == 128 - L1 + counts[0] and counts[2] == 128 - L1 and int(on.n()[1]) == 259          # room for 128 - L1, the rest dropped
        assert int(on.flags()[1]) & FC.FLAG_CAPACITY
        # the record of a wide scan through the old call and through a list that is too small: the counts, no list touched
        for wide_call, cap in ((False, 32), (True, 64)):
            rc, got, bufs = _last_match_codes(on, 1, cap, wide_call)
            assert rc == ERR_BUFFER and got == (counts[0], counts[1], counts[2]), (wide_call, rc, got)
            assert all((b == -7).all() for b in bufs)
        rc, got, bufs = _last_match_codes(on, 1, 256, True)
        assert rc == 0 and got == counts and np.array_equal(bufs[2][:got[2]], H.norm_match(m)[2])
        # a narrow record through the wide call; switching off keeps the wide record readable and refuses the next wide scan
        on.submit([FC.fev(0, cases[0].events[0])])
        rc, got, _ = _last_match_codes(on, 0, 4, True)
        assert rc == 0 and got == tuple(len(x) for x in H.norm_match(on.last_match(0)))
        on.wide_scans(False)
        assert on.submit_code([ev(2, 33, 61.0)]) == ERR_TOO_MANY_OBS
        assert tuple(len(x) for x in H.norm_match(on.last_match(1))) == counts
        lib = fleet._wide_lib()
        assert lib.rfleet_set_wide_scans(None, 1) == ERR_INVALID and lib.rfleet_wide_counts(None, None, None) == ERR_INVALID
        assert _last_match_codes(on, 7, 256, True)[0] == ERR_INVALID
    finally:
        off.close()
        on.close()


# ---- the pose track ---------------------------------------------------------------------------------------------------------------
def test_the_track_carries_the_wide_counts():
    c, events = wide_tick()
    m40 = next(x for x in WC.all_cases() if x.name == "wide_map_NS20_NM20")
    fl = WC.make_fleet([c, m40], track=True)
    try:
        fl.submit([FC.fev(0, ev) for ev in events] + [FC.fev(1, m40.events[0])])
        assert fl.wide_counts() == (1, 2)
        t, mu, sg = fl.poses()
        tr = fl.take_track()
        assert [len(x) for x in tr] == [3, 1]
        assert tr[0].kind.tolist() == [FC.EV_ODOM, FC.EV_SCAN, FC.EV_SCAN] and tr[0].K.tolist() == [0, 66, 1]
        assert (tr[0].n_state.tolist(), tr[0].n_map.tolist(), tr[0].n_new.tolist()) == ([0, 33, 0], [0, 0, 0], [0, 33, 1])
        assert tr[0].n.tolist() == [c.mu.shape[0], c.mu.shape[0] + 66, c.mu.shape[0] + 68]
        assert (tr[1].K[0], tr[1].n_state[0], tr[1].n_map[0], tr[1].n_new[0]) == (40, 20, 20, 0)
        for i in (0, 1):
            assert np.array_equal(tr[i].mu[-1], mu[i]) and np.array_equal(tr[i].sigma[-1], sg[i]) and tr[i].t[-1] == t[i]
    finally:
        fl.close()


# ---- the node -----------------------------------------------------------------------------------------------------------------------
def test_fleet_node_takes_the_34_plate_scan(oracle_lib, tmp_path):
    """The 34-plate scan of tests/test_fleet_node_gpu.py through FleetNode(wide_scans=True): processed, 34 centres logged, the member
    held to a single oracle Node on the same messages by that file's comparison; the default node still raises."""
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd.node_replay import FleetNode, synth_dump
    from tests import oracle_fleet_node as OF
    from tests import oracle_fleet_wide as OW
    meta = synth_dump(str(tmp_path / "r.npz"), synth.SessionConfig("node0", 40, 12, synth.DIFF, seed=31, speed=1.0, row_spacing=6.0),
                      max_scans=2).meta
    msgs = OW.plate_messages()
    fn = FleetNode([meta], wide_scans=True)
    plain = FleetNode([meta])
    try:
        assert fn.tick([], [(0, msgs[0])]) == [] and fn.tick([], [(0, msgs[1])]) == [0]
        assert fn.fleet.wide_counts() == (1, 1)
        assert [cl.shape for _, cl in fn.logs[0].observations] == [(OW.PLATES, 2)]
        node = OW.single_node(meta, msgs)
        assert OF.differences(fn, [node], pose_tol=1e-9, match_poses=False) == []
        got, want = fn.fleet.get_state(0, want_sigma=False), node.slam.GetState()
        assert int(fn.fleet.n()[0]) == node.slam.n == 3 + 2 * OW.PLATES and got.time == want.time
        assert float(np.abs(got.mu - want.mu).max()) < 1e-9 and int(fn.fleet.flags()[0]) == 0
        plain.tick([], [(0, msgs[0])])
        with pytest.raises(ValueError) as e:
            plain.tick([], [(0, msgs[1])])
        assert str(OW.PLATES) in str(e.value) and plain.fleet.wide_counts() == (0, 0)
    finally:
        for f in (fn, plain):
            f.detector.close(); f.fleet.close(); f.map_builder._fleet.close()


# ---- whose record is it ----------------------------------------------------------------------------------------------------------
def _alone(case, state, t, scan, fix=None, with_map=None):
    """last_match of a fresh one-member fleet that is set to `state` at time t and given `scan` alone."""
    fl = H.fleet_mod().ReflectorEKFSLAMFleet([FC.options_of(case)], wide_scans=scan is not None and len(scan) > 32)
    try:
        fl.set_state(0, t, state[0], state[1], (0.0, 0.0, 0.0))
        if with_map is not None:
            fl.set_map(*with_map)
        if scan is not None:
            fl.submit([(0, FC.EV_SCAN, t + 0.1, (0.0, 0.0, 0.0), scan) + (() if fix is None else (fix,))])
        return H.norm_match(fl.last_match(0))
    finally:
        fl.close()


def test_last_match_follows_the_launch_that_wrote_it():
    """Member 0's scans go through a plain, a fix, a map, a tracked and a wide launch, a narrow scan inside a wide launch, a plain
    launch again and a restore; after each, its last_match is that of a fresh fleet set to the same state and given that scan alone."""
    lms = FC.far_lattice(4)
    cases = [FC.crafted(f"whose_{i}", lms, [], [], seed=9790 + i) for i in range(3)]
    pts = FM.map_lattice(3)
    the_map = (np.asarray(pts, np.float32), np.tile(np.asarray(FM.IDENTITY), (3, 1)))
    no_map = (np.zeros((0, 2), np.float32), np.zeros((0, 4)))
    cloud = lambda *p: np.asarray(p, np.float32).reshape(-1, 2)
    by = lambda j, i: FM.near(lms[j], i)
    far = FC.far_lattice(40)[8:37]
    wide = cloud(*[by(j, j) for j in range(4)], *far)
    wide1 = cloud(*[by(j, j + 2) for j in range(4)], *FC.far_lattice(80)[44:73])
    assert wide.shape == wide1.shape == (33, 2)
    fl = WC.make_fleet(cases, wide=True, with_map=False)
    try:
        def step(scan, fix=None, with_map=None, others=()):
            before, t = FC.state_bits(fl, 0), float(fl.poses()[0][0])
            fl.submit([(0, FC.EV_SCAN, t + 0.1, (0.0, 0.0, 0.0), scan) + (() if fix is None else (fix,))] + list(others))
            got, want = H.norm_match(fl.last_match(0)), _alone(cases[0], before, t, scan, fix, with_map)
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (got, want)
            return tuple(len(x) for x in got)                 # (state pairs, map pairs, new)

        other = lambda m, scan: (m, FC.EV_SCAN, 60.0, (0.0, 0.0, 0.0), scan)
        assert step(cloud(by(0, 0), by(1, 1), (0.0, 2.5)), others=[other(2, cloud(by(2, 3)))]) == (2, 0, 1)              # plain
        snap = fl.snapshot([0])
        assert step(cloud(by(1, 2), by(2, 3)), fix=FM.FIX) == (2, 0, 0)                                                  # fix
        fl.set_map(*the_map)
        assert step(cloud(FM.near(pts[0], 1), by(3, 4), FM.near(pts[2], 2)), with_map=the_map) == (1, 2, 0)              # map
        fl.set_map(*no_map)
        fl.track(True)
        assert step(cloud(by(0, 5), FM.near(pts[1], 3), by(2, 6))) == (2, 0, 1)                                          # tracked: no map pairs
        fl.track(False)
        assert fl.wide_counts() == (0, 0)
        assert step(wide) == (4, 0, 29) and fl.wide_counts() == (1, 1)                                                   # wide
        assert step(cloud(by(3, 1), by(0, 2)), others=[other(1, wide1)]) == (2, 0, 0) and fl.wide_counts() == (2, 2)     # narrow in a wide launch
        assert len(H.norm_match(fl.last_match(1))[2]) == 29
        assert step(cloud(by(1, 3))) == (1, 0, 0) and fl.wide_counts() == (2, 2)                                         # plain again
        fl.restore(snap, [0])
        got = H.norm_match(fl.last_match(0))
        want = _alone(cases[0], FC.state_bits(fl, 0), float(fl.poses()[0][0]), None)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)) and [len(x) for x in got] == [0, 0, 0]               # restore: empty
    finally:
        fl.close()
