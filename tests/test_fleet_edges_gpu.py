"""k_fleet_step at the shapes and edges where an indexing slip is silent, against the longdouble witness
(tests/witness/fleet_witness.py) on the cases of tests/fleet_cases.py.

Association lists, n and flags must be identical; max|dsigma| / max|sigma_ref| and max|dmu| / max(1, max|mu_ref|) must stay
within 16 x the FP64 noise floor that tests/test_fleet_edges_cpu.py measures between the CPU restatements and the witness
(fleet_harness.check_member, fleet_cases.gpu_bounds; never looser than the 1e-9 / 1e-11 of tests/test_fleet_gpu.py).  The kernel sums in another order
than either CPU restatement (4-deep MFMA chains, Gauss-Jordan without pivoting) at the same depth, so a single-digit factor
is what rounding explains; the planted defects of the CPU module exceed the bound by 1e7 and more."""
from __future__ import annotations

import copy

import numpy as np
import pytest

from reflector_ekf_slam_amd import synth
from reflector_ekf_slam_amd import session as S
from tests import fleet_cases as FC
from tests.fleet_harness import fleet_mod, make_fleet, run_lockstep
from tests.helpers import make_gpu, make_oracle, norm_match
from tests.witness import fleet_witness as FW

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not FW.available(), reason="numpy.longdouble has no 64-bit mantissa here")]


def test_shape_sweep_in_one_fleet():
    """Every sweep case a member of one fleet: one submit carries every member's scan, a second one every member's follow-up
    scan (one more reflector: a stale row written past n by the first scan would show here)."""
    cases = FC.sweep_cases()
    assert all(c.max_landmarks == 128 and len(c.events) == 2 for c in cases)
    worst_s, worst_m = run_lockstep(cases, FC.SUITE)
    print(f"\nsweep of {len(cases)} members: worst sigma error {worst_s[0]:.2f} x the FP64 floor ({worst_s[1]}), "
          f"worst mu error {worst_m[0]:.2f} x ({worst_m[1]}); the bound is {FC.GPU_FACTOR:.0f} x")


def test_crafted_cases():
    """Gate to the last float32 ulp, exact ties, small and full maps, duplicates, the heading wrap with time going backwards."""
    cases = [c for c in FC.crafted_cases() if c.max_landmarks == 128]
    assert len(cases) >= 17
    worst_s, worst_m = run_lockstep(cases, FC.SUITE)
    print(f"\n{len(cases)} crafted cases: worst sigma error {worst_s[0]:.2f} x the FP64 floor ({worst_s[1]}), "
          f"worst mu error {worst_m[0]:.2f} x ({worst_m[1]})")


@pytest.mark.parametrize("room", [1, 2])
def test_capacity_partial_and_full(room):
    """Room for `room` of 5 new observations, interleaved with matched ones; then 3 new + 8 matched on the full member: as the
    witness fed the scans with the dropped observations removed, and as a single-filter handle without auto-grow."""
    c = next(c for c in FC.capacity_cases() if c.room == room)
    n_max = 3 + 2 * c.max_landmarks
    assert c.flags == FC.FLAG_CAPACITY
    run_lockstep([c], FC.SUITE, max_landmarks=c.max_landmarks)
    fl = make_fleet([c], c.max_landmarks)
    g = make_gpu(c.model, c.t, c.mu[:3], FC.LIN_COV, FC.ANG_COV, FC.OBS_COV, max_landmarks=c.max_landmarks)
    g.set_state(c.t, c.mu, c.P, c.vt)
    for ev in c.events:
        fl.submit([FC.fev(0, ev)])
        FC.feed(g, ev)
        a, b = norm_match(fl.last_match(0)), norm_match(g.last_match())
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert int(fl.n()[0]) == n_max and fl.flags()[0] & FC.FLAG_CAPACITY and g.flags() & FC.FLAG_CAPACITY
    sa, sb = fl.get_state(0), g.GetState()
    assert sa.mu.shape[0] == sb.mu.shape[0] == n_max
    assert float(np.abs(sa.mu - sb.mu).max()) < FC.MU_TOL and float(np.abs(sa.sigma - sb.sigma).max()) < FC.SIGMA_TOL
    fl.close()
    g.close()


def test_singular_flag_is_a_members_own():
    sing, (a, b) = FC.singular_case(), FC.plain_neighbours()
    cases = [a, sing, b]

    def run(skip):
        fl = make_fleet(cases)
        fl.submit([FC.fev(i, c.events[0]) for i, c in enumerate(cases) if i != skip])
        out = [FC.state_bits(fl, i) for i in range(3)], fl.flags().copy(), fl.n().copy(), norm_match(fl.last_match(1))
        fl.close()
        return out

    states, flags, n, rec = run(None)
    assert flags[1] == FC.FLAG_SINGULAR and flags[0] == 0 and flags[2] == 0
    assert n[1] == sing.mu.shape[0] and np.array_equal(rec[0], np.asarray(sing.expect[0][0], np.int32))
    assert np.isfinite(states[1][0]).all() and np.isfinite(states[1][1]).all()          # a numeric flag: nothing else happens
    states2, flags2, _, _ = run(1)
    assert flags2[1] == 0
    for i in (0, 2):
        assert FC.same_bits(states[i], states2[i]), f"member {i} felt its neighbour's singular scan"


def test_several_scans_per_launch():
    """One session per model, each in three forms: one event per submit, chunks of 2, 3, 5 and 17 events regardless of kind
    (launches with several scans, appending ones included), the whole session in one submit."""
    sessions = [synth.make_session(synth.SessionConfig(f"multi{m}", 48, 16, m, seed=7400 + m), max_scans=150) for m in (synth.DIFF, synth.OMNI)]
    evs = [FC.events_of(s) for s in sessions]
    fl = fleet_mod().ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions for _ in range(3)], max_landmarks=128)
    chunks_with_scans, appended_inside = 0, 0
    for si, e in enumerate(evs):
        a, b, c = 3 * si, 3 * si + 1, 3 * si + 2
        for ev in e:
            fl.submit([FC.fev(a, ev)])
        pos, q = 0, 0
        while pos < len(e):
            size = (2, 3, 5, 17)[q % 4]
            chunk = e[pos: pos + size]
            n_before = int(fl.n()[b])
            fl.submit([FC.fev(b, ev) for ev in chunk])
            scans = sum(1 for ev in chunk if ev[0] == synth.EV_SCAN)
            chunks_with_scans += scans >= 2
            appended_inside += scans >= 2 and int(fl.n()[b]) > n_before
            pos, q = pos + size, q + 1
        fl.submit([FC.fev(c, ev) for ev in e])
    assert chunks_with_scans >= 10 and appended_inside >= 2
    for si, s in enumerate(sessions):
        o = make_oracle(s.config.odom_model, s.init_time, s.init_pose, s.config.sigma_v ** 2, s.config.sigma_w ** 2, s.config.sigma_obs ** 2)
        for ev in evs[si]:
            FC.feed(o, ev)
        mo, Po = o.state()
        ref = FC.state_bits(fl, 3 * si)
        assert ref[0].shape == mo.shape and 3 < mo.shape[0] <= 99
        assert float(np.abs(ref[0] - mo).max()) < FC.MU_TOL and float(np.abs(ref[1] - Po).max()) < FC.SIGMA_TOL
        for form in (1, 2):
            assert FC.same_bits(FC.state_bits(fl, 3 * si + form), ref), f"session {si}: form {'abc'[form]} gives other bits than one event per submit"
        recs = [norm_match(fl.last_match(3 * si + form)) for form in range(3)]
        for r in recs[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(r, recs[0]))
    assert not fl.flags().any()
    # the record is the LAST scan's: `scan, odom` leaves that scan's, `scan, empty scan` an empty one
    t = float(fl.poses()[0][0])
    last_scan = [ev for ev in evs[0] if ev[0] == synth.EV_SCAN][-1]
    cloud = last_scan[3]
    fl.submit([(0, synth.EV_SCAN, t + 0.1, (0.0, 0.0, 0.0), cloud), (0, synth.EV_ODOM, t + 0.12, (0.3, 0.0, 0.05), None)])
    fl.submit([(1, synth.EV_SCAN, t + 0.1, (0.0, 0.0, 0.0), cloud)])
    sp, _, nw = norm_match(fl.last_match(0))
    sp1, _, nw1 = norm_match(fl.last_match(1))
    assert sp.shape[0] + nw.shape[0] == cloud.shape[0] and np.array_equal(sp, sp1) and np.array_equal(nw, nw1)
    fl.submit([(0, synth.EV_SCAN, t + 0.2, (0.0, 0.0, 0.0), cloud), (0, synth.EV_SCAN, t + 0.3, (0.0, 0.0, 0.0), np.zeros((0, 2), np.float32))])
    sp, _, nw = norm_match(fl.last_match(0))
    assert sp.shape[0] == 0 and nw.shape[0] == 0
    fl.close()


def test_staging_ring_goes_round_and_grows():
    """Forty submits without a getter in between (five times round the ring of 8 segments); the submits of the first round
    need less than 4096 bytes, those of the second between 4096 and 8192, the later ones more than 8192, so every segment
    grows twice.  Same bits as a run that synchronises after every submit."""
    base = next(c for c in FC.map_cases() if c.name == "map_L128_K32_all_matched")
    B = 48
    cloud = base.events[0][3]
    assert cloud.shape[0] == 32

    def need(members):                                    # bytes of a segment, as rfleet_api.hip lays it out (events 48 B, obs 8 B)
        return members * (48 + 8 * 32 + 8) + 16

    assert need(8) < 4096 < need(24) < 8192 < need(48)

    def run(synchronise):
        fl = make_fleet([base] * B)
        for q in range(40):
            members = 8 if q < 8 else 24 if q < 16 else 48
            fl.submit([(b, FC.EV_SCAN, base.t + 0.1 * (q + 1), (0.0, 0.0, 0.0), cloud) for b in range(members)])
            if synchronise:
                fl.sync()
        out = [FC.state_bits(fl, b) for b in (0, 7, 8, 23, 24, 47)], fl.flags().copy()
        fl.close()
        return out

    free, fflags = run(False)
    sync, sflags = run(True)
    assert not fflags.any() and not sflags.any()
    for a, b in zip(free, sync):
        assert FC.same_bits(a, b)
    assert FC.same_bits(free[0], free[1]) and FC.same_bits(free[2], free[3]) and FC.same_bits(free[4], free[5])
    assert not FC.same_bits(free[0], free[2])


def test_dropped_events_and_use_imu():
    a, b = FC.plain_neighbours()
    imu = copy.copy(a)
    imu.use_imu, imu.name = True, "use_imu"
    cases = [a, imu, b]
    fl = make_fleet(cases)
    # a submit whose every event is dropped on the host: no launch, nothing moves
    before = [FC.state_bits(fl, i) for i in range(3)]
    t0, mu0, s0 = fl.poses()
    assert fl.submit_code([(0, FC.EV_ODOM, a.t - 0.5, (0.4, 0.0, 0.1), None), (1, FC.EV_ODOM, imu.t + 0.05, (0.4, 0.0, 0.1), None),
                           (0, FC.EV_ODOM, a.t - 0.1, (0.2, 0.0, 0.0), None)]) == 0
    t1, mu1, s1 = fl.poses()
    assert np.array_equal(t0, t1) and np.array_equal(mu0, mu1) and np.array_equal(s0, s1) and np.array_equal(fl.n(), [c.mu.shape[0] for c in cases])
    for i in range(3):
        assert FC.same_bits(FC.state_bits(fl, i), before[i])
    # odom(stale), odom, scan in ONE submit == the three calls made separately (member 0 here, member 2 there)
    scan = a.events[0]
    trio = [(FC.EV_ODOM, a.t - 0.2, (0.9, 0.0, 0.3), None), (FC.EV_ODOM, a.t + 0.04, (0.5, 0.0, 0.2), None), scan]
    fl.submit([FC.fev(0, ev) for ev in trio] + [FC.fev(1, ev) for ev in trio])
    fl2 = make_fleet([a])
    for ev in trio:
        fl2.submit([FC.fev(0, ev)])
    assert FC.same_bits(FC.state_bits(fl, 0), FC.state_bits(fl2, 0)) and fl.poses()[0][0] == fl2.poses()[0][0] == scan[1]
    fl2.close()
    # the use_imu member: odometry moved neither time nor pose; its scan is the oracle's with vt = 0
    o = FC.oracle_of(a)                                    # a's state, vt = 0 (crafted cases stand still)
    assert tuple(a.vt) == (0.0, 0.0, 0.0)
    FC.feed(o, scan)
    st = fl.get_state(1)
    mo, Po = o.state()
    assert st.time == scan[1] and st.mu.shape == mo.shape
    assert float(np.abs(st.mu - mo).max()) < FC.MU_TOL and float(np.abs(st.sigma - Po).max()) < FC.SIGMA_TOL
    es, _, en = norm_match(o.last_match())
    sp, _, nw = norm_match(fl.last_match(1))
    assert np.array_equal(sp, es) and np.array_equal(nw, en)
    assert not FC.same_bits(FC.state_bits(fl, 0), FC.state_bits(fl, 1))             # member 0 did move on its odometry
    t2 = fl.poses()[0].copy()
    fl.submit([(1, FC.EV_ODOM, scan[1] + 0.5, (1.0, 0.0, 0.5), None), (2, FC.EV_ODOM, b.t + 0.5, (1.0, 0.0, 0.5), None)])
    t3, mu3, _ = fl.poses()
    assert t3[1] == t2[1] and np.array_equal(mu3[1], st.mu[:3]) and t3[2] == b.t + 0.5 and not np.array_equal(mu3[2], b.mu[:3])
    o.close()
    fl.close()
