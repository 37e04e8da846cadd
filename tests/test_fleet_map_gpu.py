"""k_fleet_step_map on the GPU: the fleet's shared pre-loaded map (rfleet_set_map) against the longdouble witness with the map
branch and against oracle/ekf_oracle.c, on the cases of tests/fleet_map_cases.py.  Association lists (map pairs included), n and
flags are exact; the state holds within min(16 x the suite's FP64 floor, the absolute tolerances)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as MC
from tests.helpers import norm_match
from tests.witness import fleet_map_witness as MW

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not MW.available(), reason="numpy.longdouble has no 64-bit mantissa on this platform")]


def by_name():
    return {c.name: c for c in MC.all_cases()}


def lists_of(fl, i):
    return tuple(a.tolist() for a in norm_match(fl.last_match(i)))


def claimed(case, k):
    return tuple(a.tolist() for a in MC.want_lists(case, k))


def test_all_cases_in_lockstep():
    """Every case of tests/fleet_map_cases.py as a member of one fleet: lists, n and flags exact, the state within
    min(16 x the FP64 floor, the absolute tolerances) of the witness.

    Measured on the MI355X: worst 0.75 x the floor in sigma (mix_5_5_5_L5), 0.82 x in mu (fix_16_16).  fix_0_31 (n = 3, 31 map
    pairs and a pose fix) was 242 x in mu while the fix followed the reflector rows; with the fix in front of them (what
    k_fleet_step_map does for a member on the map) it is 0.56 x.  The nine nan cases (a NaN weighted distance
    never wins: the `dist == dist` in the lane loop of the map sweep) are among the cases; the single filter's sweep has no such
    compare yet, and nan_p0_q1, nan_p5_q69, nan_p5_q37 and nan_nearest_5_runner_up_69 come out as new reflectors there
    (tests/test_ekf_map_gpu.py, KNOWN_DIVERGENCES)."""
    worst_s, worst_m, misses = MC.run_lockstep(MC.all_cases())
    print(f"\nworst over {len(MC.all_cases())} map cases: sigma {worst_s[0]:.2f} x the FP64 floor at {worst_s[1]}, "
          f"mu {worst_m[0]:.2f} x at {worst_m[1]} (the bound is {FC.GPU_FACTOR:.0f} x); {len(misses)} misses")
    assert not misses, "\n".join(misses)


def test_a_member_without_the_map_is_the_same_bits_under_the_map_kernel():
    """A use = 0 member in a launch that takes k_fleet_step_map (its neighbour uses the map) against the same member in a fleet
    that never had a map (k_fleet_step; with a pose fix k_fleet_step_fix)."""
    cs = by_name()
    plain, user = cs["unused_map"], cs["mix_5_5_5_L5"]
    for fix in (None, MC.FIX):
        ev = plain.events[0][:4] + (fix,)
        a = H.make_fleet([user, plain])
        b = H.make_fleet([plain])
        try:
            a.set_map(user.map_xy, user.map_cov, members=[0])
            a.submit([FC.fev(0, user.events[0]), FC.fev(1, ev)])
            b.submit([FC.fev(0, ev)])
            assert lists_of(a, 0) == claimed(user, 0) and len(claimed(user, 0)[1]) == 5       # the launch did take the map kernel
            assert lists_of(a, 1) == lists_of(b, 0) and lists_of(a, 1)[1] == []
            assert FC.same_bits(FC.state_bits(a, 1), FC.state_bits(b, 0)), f"fix {fix}"
            assert a.map_size() == user.map_xy.shape[0]
        finally:
            a.close()
            b.close()


def test_a_map_member_does_not_depend_on_index_neighbours_or_batching():
    """The two-scan case alone at index 0, one scan per submit, against the same case at index 3 between other members, both
    scans in ONE submit (the second scan's state rows are reflectors the first one appended inside the same launch)."""
    cs = by_name()
    c = cs["two_scans"]
    others = [cs["mix_16_16_0_L16"], cs["fix_0_31"], cs["unused_map"], cs["mix_1_31_0_L128"]]
    alone = H.make_fleet([c])
    crowd = H.make_fleet(others[:3] + [c] + others[3:])
    wit = MC.map_witness_of(c)
    try:
        alone.set_map(c.map_xy, c.map_cov)
        crowd.set_map(c.map_xy, c.map_cov, members=[0, 1, 3, 4])
        for k, ev in enumerate(c.events):
            alone.submit([FC.fev(0, ev)])
            FC.feed(wit, ev)
            MC.check_member(alone, 0, c, k, wit)
        batch = [FC.fev(0, others[0].events[0]), FC.fev(3, c.events[0]), FC.fev(2, others[2].events[0]), FC.fev(1, others[1].events[0]),
                 FC.fev(3, c.events[1]), FC.fev(4, others[3].events[0])]
        crowd.submit(batch)
        MC.check_member(crowd, 3, c, 1, wit)
        assert lists_of(crowd, 3) == lists_of(alone, 0)
        assert FC.same_bits(FC.state_bits(crowd, 3), FC.state_bits(alone, 0))
    finally:
        alone.close()
        crowd.close()


def test_clearing_the_map_gives_a_fleet_that_never_had_one():
    cs = by_name()
    user, later = cs["mix_5_5_5_L5"], cs["unused_map"]            # `later` is written for a fleet without a map
    a = H.make_fleet([user, later])
    b = H.make_fleet([user, later])
    try:
        a.set_map(user.map_xy, user.map_cov)                      # every member uses it
        a.submit([FC.fev(0, user.events[0])])
        assert len(lists_of(a, 0)[1]) == 5
        a.set_map(np.zeros((0, 2), np.float32), np.zeros((0, 4)))
        assert a.map_size() == 0 and b.map_size() == 0
        a.submit([FC.fev(1, later.events[0])])
        b.submit([FC.fev(1, later.events[0])])
        assert lists_of(a, 1) == lists_of(b, 1) == claimed(later, 0)
        assert FC.same_bits(FC.state_bits(a, 1), FC.state_bits(b, 1))
        # and the member that did use it goes on as a plain member: its next scan has no map pairs
        a.submit([FC.fev(0, (FC.EV_SCAN, user.events[0][1] + 0.1, (0.0, 0.0, 0.0), user.events[0][3]))])
        assert lists_of(a, 0)[1] == []
    finally:
        a.close()
        b.close()


def test_replacing_the_map_holds_from_the_next_submit():
    """One pure-localisation member, the same cloud twice: on the first map its observations are map pairs; on the second map
    (the first one moved by 0.5 m) they are not, and become reflectors.  set_map itself changes nothing."""
    c = by_name()["size_M64"]
    moved = (c.map_xy + np.float32(0.5)).astype(np.float32)
    fl = H.make_fleet([c])
    wit = MC.map_witness_of(c)
    try:
        fl.set_map(c.map_xy, c.map_cov)
        fl.submit([FC.fev(0, c.events[0])])
        FC.feed(wit, c.events[0])
        MC.check_member(fl, 0, c, 0, wit)
        before, lists = FC.state_bits(fl, 0), lists_of(fl, 0)
        fl.set_map(moved, c.map_cov)
        assert fl.map_size() == 64 and FC.same_bits(FC.state_bits(fl, 0), before) and lists_of(fl, 0) == lists
        ev = (FC.EV_SCAN, c.events[0][1] + 0.1, (0.0, 0.0, 0.0), c.events[0][3])
        fl.submit([FC.fev(0, ev)])
        wit.set_map(moved, c.map_cov)
        FC.feed(wit, ev)
        K = c.events[0][3].shape[0]
        assert lists_of(fl, 0) == ([], [], list(range(K))) and wit.last_match == ([], [], list(range(K)))
        mu_ref, P_ref = wit.state()
        st = fl.get_state(0)
        es, em = H.rel_err(st.mu, st.sigma, mu_ref, P_ref)
        bs, bm = H.bounds_within_tolerances(mu_ref, P_ref, MC.SUITE)
        assert st.mu.shape[0] == 3 + 2 * K and es <= bs and em <= bm, (es, bs, em, bm)
    finally:
        fl.close()


def test_session_against_the_oracle():
    """The golden map session's first scans on four members of a fleet of seven: poses within 1e-9 m of oracle/ekf_oracle.c and its
    lists on every scan; the four members' states are the same bits."""
    s = MC.session()
    B = max(MC.SESSION_MEMBERS) + 1
    fl = H.fleet_mod().ReflectorEKFSLAMFleet([s.options] * B, max_landmarks=64)
    worst = 0.0
    try:
        fl.set_map(s.map_xy, s.map_cov, members=MC.SESSION_MEMBERS)
        for k, ev in enumerate(s.events):
            fl.submit([FC.fev(b, ev) for b in MC.SESSION_MEMBERS])
            if ev[0] != FC.EV_SCAN:
                continue
            sp, mp, nw, mu = s.records[k]
            _, poses, _ = fl.poses()
            n = fl.n()
            for b in MC.SESSION_MEMBERS:
                got = norm_match(fl.last_match(b))
                assert np.array_equal(got[0], sp) and np.array_equal(got[1], mp) and np.array_equal(got[2], nw), (k, b)
                assert int(n[b]) == mu.shape[0], (k, b)
                worst = max(worst, float(np.abs(poses[b] - mu[:3]).max()))
        print(f"\nmap session, {s.scans} scans on members {MC.SESSION_MEMBERS}: largest |pose - oracle| {worst:.3e}")
        assert worst < 1e-9
        assert not fl.flags().any()
        first = FC.state_bits(fl, MC.SESSION_MEMBERS[0])
        for b in MC.SESSION_MEMBERS[1:]:
            assert FC.same_bits(FC.state_bits(fl, b), first), b
        idle = [b for b in range(B) if b not in MC.SESSION_MEMBERS]
        assert all(int(n[b]) == 3 for b in idle)
    finally:
        fl.close()


def test_more_workgroups_than_compute_units_on_the_largest_map():
    """300 members, a 2048-point map, one scan each in one submit: every member's lists, three members against the witness."""
    cases = MC.big_fleet_cases()
    fl = H.make_fleet(cases, 8)
    try:
        fl.set_map(cases[0].map_xy, cases[0].map_cov)
        assert fl.map_size() == MC.BIG_M
        fl.submit([FC.fev(b, c.events[0]) for b, c in enumerate(cases)])
        n = fl.n()
        assert not fl.flags().any()
        for b, c in enumerate(cases):
            got = norm_match(fl.last_match(b))
            for a, want in zip(got, MC.want_lists(c, 0)):
                assert np.array_equal(a, want), (b, a.tolist(), want.tolist())
            assert int(n[b]) == 5
        for b in (0, 149, 299):
            wit = MC.map_witness_of(cases[b])
            FC.feed(wit, cases[b].events[0])
            MC.check_member(fl, b, cases[b], 0, wit)
    finally:
        fl.close()
