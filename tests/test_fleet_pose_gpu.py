"""k_fleet_step's pose fixes (the reference's USE_GPS branch) and rfleet_predict_poses on the GPU: sessions against the C oracle
on every scan, the shape cases of tests/fleet_pose_cases.py against the longdouble witness, bit-identity under every call
pattern, parity with the single filter's gps_pose3, the MM == 0 quirk and the argument checks.

Tolerances: MU_TOL = 1e-9 / SIGMA_TOL = 1e-11 of tests/test_fleet_gpu.py against the oracle and the single filter; against the
witness 16 x the FP64 floor tests/test_fleet_pose_cpu.py measures on these cases (fleet_harness.check_member with fleet_pose_cases.SUITE)."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_pose_cases as PC
from tests.fleet_harness import fleet_mod, make_fleet, run_lockstep
from tests.helpers import make_gpu, make_oracle, norm_match
from tests.witness import fleet_pose_witness as PW

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not PW.available(), reason="numpy.longdouble has no 64-bit mantissa here")
PREDICT_MU_TOL, PREDICT_SIGMA_TOL = 1e-12, 1e-13      # tests/test_ekf_gpu.py::test_predict_state_full_omni_with_landmarks


def session_fleet(ss, copies=1):
    return fleet_mod().ReflectorEKFSLAMFleet([s.options for s in ss for _ in range(copies)], max_landmarks=32)


@pytest.fixture(scope="module")
def sessions_run():
    """The four sessions as one fleet, one tick = the same event index of every member, one submit; checked on every scan."""
    ss = PC.sessions()
    fl = session_fleet(ss)
    worst_mu, bad, scans = 0.0, [], 0
    for k in range(max(len(s.events) for s in ss)):
        fl.submit([FC.fev(i, s.events[k]) for i, s in enumerate(ss) if k < len(s.events)])
        for i, s in enumerate(ss):
            if k >= len(s.events) or s.events[k][0] != FC.EV_SCAN:
                continue
            scans += 1
            sp, mp, nw = norm_match(fl.last_match(i))
            es, en, mo = s.records[k]
            if not (np.array_equal(sp, es) and np.array_equal(nw, en) and mp.shape[0] == 0):
                bad.append((i, k, s.margins[k]))
                continue
            mu = fl.get_state(i, want_sigma=False).mu
            assert mu.shape == mo.shape, (i, k, mu.shape, mo.shape)
            worst_mu = max(worst_mu, float(np.abs(mu - mo).max()))
    finals = [FC.state_bits(fl, i) for i in range(len(ss))]
    flags = fl.flags().copy()
    yield dict(fleet=fl, finals=finals, worst_mu=worst_mu, bad=bad, flags=flags, scans=scans)
    fl.close()


def test_sessions_match_the_oracle_on_every_scan(sessions_run):
    ss, r = PC.sessions(), sessions_run
    for i, k, mg in r["bad"][:4]:
        print(f"member {i} event {k}: association differs; oracle margins per observation: {mg}")
    assert not r["bad"], f"{len(r['bad'])} scans with other associations than the oracle"
    assert r["scans"] == sum(1 for s in ss for ev in s.events if ev[0] == FC.EV_SCAN)          # no scan left out
    print(f"\nmax |mu - oracle| over {r['scans']} scans of 4 members: {r['worst_mu']:.3e}")
    assert r["worst_mu"] < FC.MU_TOL
    worst_s = 0.0
    for i, s in enumerate(ss):
        assert r["finals"][i][0].shape == s.mu.shape
        assert float(np.abs(r["finals"][i][0] - s.mu).max()) < FC.MU_TOL
        worst_s = max(worst_s, float(np.abs(r["finals"][i][1] - s.P).max()))
    print(f"max |sigma - oracle| at the end: {worst_s:.3e}")
    assert worst_s < FC.SIGMA_TOL
    assert not r["flags"].any()


@needs_ld
def test_shape_cases_in_one_fleet():
    """0, 5, 15, 17, 63, 65 and 67 rows of the joint system, n mod 16 in {3, 15, 1}, both models, and the heading cases (yaw across
    +-pi, a fix behind a Predict with negative dt), all members of ONE fleet."""
    cases = PC.shape_cases() + PC.heading_fix_cases()
    worst_s, worst_m = run_lockstep(cases, PC.SUITE)
    print(f"\n{len(cases)} pose cases: worst sigma error {worst_s[0]:.2f} x the FP64 floor ({worst_s[1]}), "
          f"worst mu error {worst_m[0]:.2f} x ({worst_m[1]}); the bound is {FC.GPU_FACTOR:.0f} x")


@needs_ld
@pytest.mark.parametrize("room", [1, 2])
def test_fix_scan_that_fills_the_map(room):
    c = next(c for c in PC.capacity_fix_cases() if c.room == room)
    run_lockstep([c], PC.SUITE, max_landmarks=c.max_landmarks)


def test_call_pattern_and_neighbours_do_not_change_the_bits(sessions_run):
    ss, ref = PC.sessions(), sessions_run["finals"]
    F = fleet_mod()
    # one submit per event, alone
    fl = F.ReflectorEKFSLAMFleet([ss[0].options], max_landmarks=32)
    for ev in ss[0].events:
        fl.submit([FC.fev(0, ev)])
    assert FC.same_bits(FC.state_bits(fl, 0), ref[0]), "a fleet of one, one event per submit, gives other bits"
    fl.close()
    # every event of every member in ONE submit
    fl = session_fleet(ss)
    fl.submit([FC.fev(i, ev) for i, s in enumerate(ss) for ev in s.events])
    for i in range(len(ss)):
        assert FC.same_bits(FC.state_bits(fl, i), ref[i]), f"member {i}: one submit for the whole session gives other bits"
    fl.close()
    # shuffled ticks, every session twice: member 2 i with its fixes, member 2 i + 1 without them
    fl = session_fleet(ss, copies=2)
    rng = np.random.default_rng(11)
    for k in range(max(len(s.events) for s in ss)):
        tick = [FC.fev(2 * i + c, s.events[k], with_fix=(c == 0)) for i, s in enumerate(ss) for c in (0, 1) if k < len(s.events)]
        fl.submit([tick[q] for q in rng.permutation(len(tick))])
    for i in range(len(ss)):
        assert FC.same_bits(FC.state_bits(fl, 2 * i), ref[i]), f"member {i}: shuffling and fix-less neighbours changed the bits"
    assert FC.same_bits(FC.state_bits(fl, 5), ref[2])                      # the session without fixes is its own twin
    assert not FC.same_bits(FC.state_bits(fl, 1), ref[0])                  # ... and a fix does move a member
    fl.close()
    # has_pose_fix = 0 with garbage in pose_fix: the bits of a plain scan
    fl = F.ReflectorEKFSLAMFleet([ss[2].options], max_landmarks=32)
    arr, count, keep = F.ReflectorEKFSLAMFleet.pack([FC.fev(0, ev) for ev in ss[2].events])
    for q in range(count):
        assert arr[q].has_pose_fix == 0
        arr[q].pose_fix[0], arr[q].pose_fix[1], arr[q].pose_fix[2] = math.nan, 1e300, -math.inf
    fl.submit_packed((arr, count, keep))
    assert FC.same_bits(FC.state_bits(fl, 0), ref[2]), "pose_fix was read although has_pose_fix is 0"
    fl.close()


@pytest.mark.parametrize("which", [0, 3])
def test_against_the_single_filter(which):
    s = PC.sessions()[which]
    cfg = s.sess.config
    fl = fleet_mod().ReflectorEKFSLAMFleet([s.options], max_landmarks=32)
    m = fl.member(0)
    g = make_gpu(cfg.odom_model, s.sess.init_time, s.sess.init_pose, cfg.sigma_v ** 2, cfg.sigma_w ** 2, cfg.sigma_obs ** 2, max_landmarks=32)
    worst = 0.0
    for ev in s.events:
        FC.feed(m, ev)
        FC.feed(g, ev)
        if ev[0] == FC.EV_SCAN:
            a, b = norm_match(m.last_match()), norm_match(g.last_match())
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), ev[1]
            ma, mb = m.mu(), g.mu()
            assert ma.shape == mb.shape
            worst = max(worst, float(np.abs(ma - mb).max()))
    sa, sb = m.GetState(), g.GetState()
    print(f"\nfleet member vs single filter with fixes: max |dmu| {worst:.3e}, final |dsigma| {np.abs(sa.sigma - sb.sigma).max():.3e}")
    assert worst < FC.MU_TOL
    assert float(np.abs(sa.sigma - sb.sigma).max()) < FC.SIGMA_TOL
    fl.close()
    g.close()


def test_fix_without_a_match_is_ignored():
    """MM == 0: the reference's pose rows sit inside `if (MM > 0)`.  Same scan with and without a fix: the same bits, new
    reflectors appended in both."""
    cases = [c for c in PC.shape_cases() if c.MM == 0]
    assert len(cases) >= 4 and any(c.mu.shape[0] == 3 for c in cases)
    fl = make_fleet([c for c in cases for _ in (0, 1)])
    fl.submit([FC.fev(2 * i + q, c.events[0], with_fix=(q == 0)) for i, c in enumerate(cases) for q in (0, 1)])
    n = fl.n()
    for i, c in enumerate(cases):
        assert n[2 * i] == n[2 * i + 1] == c.mu.shape[0] + 2 * c.N2 and c.N2 > 0
        assert FC.same_bits(FC.state_bits(fl, 2 * i), FC.state_bits(fl, 2 * i + 1)), c.name
    # an empty scan with a fix is a Predict
    t = float(fl.poses()[0][0])
    fl.submit([(0, FC.EV_SCAN, t + 0.1, (0.0, 0.0, 0.0), np.zeros((0, 2), np.float32), (1.0, 2.0, 0.5)),
               (1, FC.EV_SCAN, t + 0.1, (0.0, 0.0, 0.0), np.zeros((0, 2), np.float32))])
    assert FC.same_bits(FC.state_bits(fl, 0), FC.state_bits(fl, 1))
    fl.close()


def test_boundaries(sessions_run):
    fl, F = sessions_run["fleet"], fleet_mod()
    B = len(fl)
    before = [FC.state_bits(fl, b) for b in range(B)]
    tb, mb, sb = fl.poses()
    t1 = float(tb.max()) + 1.0
    cloud = np.array([[1.0, 0.5], [2.0, -0.5]], np.float32)
    good = (0, FC.EV_ODOM, t1, (0.5, 0.0, 0.1), None)
    odom_fix = F.RfleetEvent()
    odom_fix.member, odom_fix.kind, odom_fix.t, odom_fix.has_pose_fix = 1, FC.EV_ODOM, t1, 1
    assert fl.submit_code([good, odom_fix]) == -1
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf), (0.0, 0.0, math.nan)):
        assert fl.submit_code([good, (2, FC.EV_SCAN, t1, (0.0, 0.0, 0.0), cloud, bad)]) == -1
    ta, ma, sa = fl.poses()
    assert np.array_equal(ta, tb) and np.array_equal(ma, mb) and np.array_equal(sa, sb)
    for b in range(B):
        assert FC.same_bits(FC.state_bits(fl, b), before[b])
    assert fl.submit_code([(2, FC.EV_SCAN, t1, (0.0, 0.0, 0.0), cloud, (float(mb[2][0]), float(mb[2][1]), float(mb[2][2])))]) == 0
    assert fl.poses()[0][2] == t1
    for b in (0, 1, 3):
        assert FC.same_bits(FC.state_bits(fl, b), before[b])


def test_predict_poses(sessions_run):
    """Runs after test_boundaries has moved member 2: every member's own state is what the oracle is given."""
    ss, fl = PC.sessions(), sessions_run["fleet"]
    B = len(fl)
    before = [FC.state_bits(fl, b) for b in range(B)]
    t_state = fl.poses()[0].copy()
    for dts in (np.array([0.07, 0.013, 0.2, 0.05]), np.array([-0.05, 0.0, -0.2, 0.31])):        # (dt < 0: no test, as rekf_predict_state)
        mu, sg = fl.predict_poses(t_state + dts)
        for b, s in enumerate(ss):
            cfg = s.sess.config
            o = make_oracle(cfg.odom_model, s.sess.init_time, s.sess.init_pose, cfg.sigma_v ** 2, cfg.sigma_w ** 2, cfg.sigma_obs ** 2)
            o.set_state(float(t_state[b]), before[b][0], before[b][1], s.vt)
            mp, Pp = o.predict_state(float(t_state[b] + dts[b]), full=True)
            o.close()
            assert float(np.abs(mu[b] - mp[:3]).max()) < PREDICT_MU_TOL, (b, mu[b], mp[:3])
            assert float(np.abs(sg[b] - Pp[:3, :3]).max()) < PREDICT_SIGMA_TOL, b
            if dts[b] != 0.0 and np.abs(s.vt).max() > 0:
                assert float(np.abs(mu[b] - before[b][0][:3]).max()) > 1e-6               # it did predict
    m = fl.member(1)
    pm, pP = m.PredictState(float(t_state[1]) + 0.013)
    assert np.array_equal(pm, fl.predict_poses(t_state + 0.013)[0][1]) and pP.shape == (3, 3)
    for b in range(B):
        assert FC.same_bits(FC.state_bits(fl, b), before[b]), "predict_poses moved a member"
    assert np.array_equal(fl.poses()[0], t_state)
    # between a submit and the getters: it sees that submit
    t2 = float(t_state[0]) + 0.1
    want_mu, want_P = fl.predict_poses(np.where(np.arange(B) == 0, t2, t_state))
    fl.submit([(0, FC.EV_ODOM, t2, tuple(float(v) for v in ss[0].vt), None)])
    got_mu, got_P = fl.predict_poses(np.where(np.arange(B) == 0, t2, t_state))                   # dt = 0 for member 0 now
    _, pose_mu, pose_P = fl.poses()
    assert float(np.abs(got_mu[0] - pose_mu[0]).max()) < 1e-15 and np.array_equal(got_P[0], pose_P[0])
    assert float(np.abs(got_mu[0] - want_mu[0]).max()) < PREDICT_MU_TOL and float(np.abs(got_P[0] - want_P[0]).max()) < PREDICT_SIGMA_TOL
    assert float(np.abs(got_mu[0] - before[0][0][:3]).max()) > 1e-4
