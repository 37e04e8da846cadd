"""Fleet filter, the shape sweep of the wide scans on the GPU (-m gpu): k_fleet_step_wide against the longdouble JOINT witness on the
tables of tests/fleet_wide_sweep_cases.py (every n mod 16 x every class of the last block, the classes of the appended rows, mixed
blocks with and without a fix), the narrow kernels' own shape sweep inside the wide kernel (bit for bit), two wide scans of one member
in one launch, and the pose track at swept shapes.

Worst figures on an MI355X, as multiples of this suite's measured FP64 floor (bound: 16; printed by the tests, run with -s): the
125 swept cases sigma 0.45 x (wsweep_L18_MM33_N30_diff scan 0), mu 1.65 x (wsweep_L28_MM96_N23_omni scan 1); two wide scans per
member sigma 0.16 x, mu 0.72 x (wtwo_L14_MM40_N1_diff).  No kernel line had to change."""
from __future__ import annotations

import copy

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as FM
from tests import fleet_track_cases as TC
from tests import fleet_wide_cases as WC
from tests import fleet_wide_sweep_cases as SC
from tests.test_fleet_wide_gpu import two_wide_scans

pytestmark = pytest.mark.gpu


# ---- 1. the sweep ------------------------------------------------------------------------------------------------------------------
def test_the_sweep_against_the_joint_witness():
    """Every case of the tables as a member of one wide-enabled fleet per capacity (128 and 48), one submit per tick: lists equal
    the claim, sigma exactly symmetric, flags, n, state within GPU_FACTOR x the measured floor of the joint longdouble witness."""
    cases = SC.sweep_cases()
    assert sorted({c.max_landmarks for c in cases}) == [SC.CAP_SMALL, 128]
    worst_s, worst_m, misses = WC.run_lockstep(cases, SC.SUITE)
    print(f"\nworst of {len(cases)} swept wide cases: sigma {worst_s[0]:.2f} x the floor at {worst_s[1]}; mu {worst_m[0]:.2f} x at {worst_m[1]}")
    assert not misses, "\n".join(misses)
    assert 0 < worst_s[0] <= FC.GPU_FACTOR and 0 < worst_m[0] <= FC.GPU_FACTOR


# ---- 2. the narrow sweep inside the wide kernel ------------------------------------------------------------------------------------
def narrow_sweep_members():
    """Every case of the narrow kernels' shape sweep as a member that does not use the map (copies: the sweep's own records stay)."""
    return [WC.on_std_map(copy.copy(c), False) for c in FC.sweep_cases()]


@pytest.mark.parametrize("track", [False, True])
def test_the_narrow_sweep_keeps_its_bits_inside_the_wide_kernel(track):
    """The loops of test_narrow_members_keep_their_bits_beside_a_wide_member over the shapes that found the narrow kernels' own edge
    cases: both ticks of the first fleet are wide launches (member 0), those of the second launch the narrow kernels."""
    narrow, wide = narrow_sweep_members(), two_wide_scans()
    assert len(narrow) >= 90 and all(len(c.events) == 2 for c in narrow)
    fa = WC.make_fleet([wide] + narrow, wide=True, track=track)
    fb = WC.make_fleet(narrow, wide=False, track=track)
    try:
        for k in range(2):
            fa.submit([FC.fev(0, wide.events[k])] + [FC.fev(1 + i, c.events[k]) for i, c in enumerate(narrow)])
            fb.submit([FC.fev(i, c.events[k]) for i, c in enumerate(narrow)])
            assert fa.wide_counts() == (k + 1, k + 1) and fb.wide_counts() == (0, 0)
            for i, c in enumerate(narrow):
                assert FC.same_bits(FC.state_bits(fa, 1 + i), FC.state_bits(fb, i)), (c.name, k)
                a, b = fa.last_match(1 + i), fb.last_match(i)
                assert all(np.array_equal(x, y) for x, y in zip(H.norm_match(a), H.norm_match(b))), (c.name, k)
                assert all(np.array_equal(x, y) for x, y in zip(H.norm_match(a), FM.want_lists(c, k))), (c.name, k)
            assert (fa.flags()[1:] == fb.flags()).all() and (fa.n()[1:] == fb.n()).all()
        assert int(fa.n()[0]) == wide.mu.shape[0]
    finally:
        fa.close()
        fb.close()


# ---- 3. two wide scans of one member in one launch ---------------------------------------------------------------------------------
def member_feed(c):
    """A member's messages: odometry (the state's velocity again, half a step on), then its scans."""
    return [(FC.EV_ODOM, c.t + 0.05, c.vt, None, None)] + list(c.events)


def test_two_wide_scans_of_one_member_in_one_launch():
    cases = [c for c in SC.all_cases() if c.kind == "wtwo"]
    assert len(cases) == 3
    feeds = [member_feed(c) for c in cases]
    # (a) one event per submit, every scan against the joint witness
    fa = WC.make_fleet(cases)
    worst_s, worst_m = (0.0, ""), (0.0, "")
    try:
        wits = [WC.joint_witness_of(c) for c in cases]
        for j in range(4):
            for i, c in enumerate(cases):
                fa.submit([FC.fev(i, feeds[i][j])])
                FC.feed(wits[i], feeds[i][j])
                if j > 0:
                    fs, fm = FM.check_member(fa, i, c, j - 1, wits[i], SC.SUITE)
                    worst_s, worst_m = max(worst_s, (fs, f"{c.name} scan {j - 1}")), max(worst_m, (fm, f"{c.name} scan {j - 1}"))
        assert fa.wide_counts() == (6, 6)
        ref = [(FC.state_bits(fa, i), int(fa.flags()[i]), int(fa.n()[i])) for i in range(3)]
    finally:
        fa.close()
    print(f"\ntwo wide scans per member: sigma {worst_s[0]:.2f} x the floor at {worst_s[1]}; mu {worst_m[0]:.2f} x at {worst_m[1]}")
    assert 0 < worst_s[0] <= FC.GPU_FACTOR and 0 < worst_m[0] <= FC.GPU_FACTOR
    # (b) everything in ONE submit: n, n16, s_mu0 and the record are carried from event to event inside the kernel
    fb = WC.make_fleet(cases)
    try:
        fb.submit([FC.fev(i, feeds[i][j]) for j in range(4) for i in range(3)])
        assert fb.wide_counts() == (1, 6)
        for i, c in enumerate(cases):
            assert FC.same_bits(FC.state_bits(fb, i), ref[i][0]), c.name
            assert (int(fb.flags()[i]), int(fb.n()[i])) == ref[i][1:], c.name
            assert int(fb.n()[i]) == c.n + 2 * sum(len(c.expect[k][2]) for k in range(3)), c.name
            got = H.norm_match(fb.last_match(i))
            assert all(np.array_equal(x, y) for x, y in zip(got, FM.want_lists(c, 2))), (c.name, "the record is the last scan's")
    finally:
        fb.close()


# ---- 4. the track at swept shapes ------------------------------------------------------------------------------------------------
def test_the_track_at_swept_shapes():
    """Eight sweep members, one per n mod 16, on the map and off it, with and without a fix: odometry, the wide scan and the narrow
    scan of every member in one tracked submit against a tracked fleet fed one message per submit, record by record and bit for
    bit; the final states are an untracked fleet's."""
    members = SC.track_members()
    feeds = [member_feed(c) for c in members]
    fl, tw, un = WC.make_fleet(members, track=True), WC.make_fleet(members, track=True), WC.make_fleet(members)
    try:
        want = TC.twin_records(tw, [(m, ev) for m, f in enumerate(feeds) for ev in f])
        everything = [FC.fev(m, f[j]) for j in range(3) for m, f in enumerate(feeds)]
        fl.submit(everything)
        un.submit(everything)
        assert fl.wide_counts() == (1, 8) == un.wide_counts() and tw.wide_counts() == (8, 8)
        tracks = fl.take_track()
        for m, c in enumerate(members):
            TC.assert_records(tracks[m], want[m], c.name)
            assert tracks[m].kind.tolist() == [FC.EV_ODOM, FC.EV_SCAN, FC.EV_SCAN] and tracks[m].K[1] == len(c.events[0][3]) > 32
            assert (tracks[m].n_state[1], tracks[m].n_map[1], tracks[m].n_new[1]) == tuple(len(x) for x in c.expect[0]), c.name
            assert TC.last_record_is_the_slot(fl, tracks[m], m)
            assert FC.same_bits(FC.state_bits(fl, m), FC.state_bits(un, m)) and FC.same_bits(FC.state_bits(fl, m), FC.state_bits(tw, m)), c.name
        assert (fl.flags() == un.flags()).all() and (fl.n() == un.n()).all()
    finally:
        for f in (fl, tw, un):
            f.close()
