"""Fleet filter (include/rfleet.h, k_fleet_step) against the CPU oracle and the single filter.

Tolerances as in test_ekf_gpu.py / test_ekf_moving_gpu.py: association lists identical, |mu - oracle| < 1e-9,
|sigma - oracle| < 1e-11.  Bit-identity is asked wherever only the call pattern or the fleet's composition changes:
a member's arithmetic depends on its own state and events, nothing else."""
from __future__ import annotations

import numpy as np
import pytest

from reflector_ekf_slam_amd import synth
from reflector_ekf_slam_amd import session as S
from tests.fleet_cases import events_of, feed, fev, margins, same_bits, state_bits
from tests.fleet_harness import fleet_mod
from tests.helpers import make_gpu, make_oracle, norm_match

pytestmark = pytest.mark.gpu

MU_TOL, SIGMA_TOL = 1e-9, 1e-11
FLAG_CAPACITY = 1

# (landmarks, observations per scan, odometry model), seeds 7000 + index
HETERO = [(128, 16, synth.DIFF), (128, 16, synth.OMNI), (64, 8, synth.DIFF), (96, 32, synth.DIFF), (32, 8, synth.OMNI),
          (128, 32, synth.DIFF)]


def oracle_for(sess):
    cfg = sess.config
    return make_oracle(cfg.odom_model, sess.init_time, sess.init_pose, cfg.sigma_v ** 2, cfg.sigma_w ** 2, cfg.sigma_obs ** 2)


@pytest.fixture(scope="module")
def hetero():
    sessions = []
    for i, (L, K, model) in enumerate(HETERO):
        sessions.append(synth.make_session(synth.SessionConfig(f"fleet{i}", L, K, model, seed=7000 + i)))
    return sessions, [events_of(s) for s in sessions]


@pytest.fixture(scope="module")
def hetero_run(hetero):
    """Test 1's run: one tick = the same event index of every member still running, one submit; checked every scan."""
    sessions, evs = hetero
    F = fleet_mod()
    fl = F.ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions], max_landmarks=128)
    oracles = [oracle_for(s) for s in sessions]
    worst_mu, bad = 0.0, []
    for k in range(max(len(e) for e in evs)):
        tick, preds = [], {}
        for i, e in enumerate(evs):
            if k < len(e):
                tick.append(fev(i, e[k]))
                if e[k][0] == synth.EV_SCAN:
                    preds[i] = oracles[i].predict_state(e[k][1])[0]
                feed(oracles[i], e[k])
        fl.submit(tick)
        for i in preds:
            sp, mp, nw = norm_match(fl.last_match(i))
            es, em, en = norm_match(oracles[i].last_match())
            if not (np.array_equal(sp, es) and np.array_equal(nw, en) and mp.shape[0] == 0 and em.shape[0] == 0):
                bad.append((i, k, margins(preds[i], evs[i][k][3])))
                continue
            mu, mo = fl.get_state(i, want_sigma=False).mu, oracles[i].mu()
            assert mu.shape == mo.shape, (i, k, mu.shape, mo.shape)
            worst_mu = max(worst_mu, float(np.abs(mu - mo).max()))
    finals = [state_bits(fl, i) for i in range(len(sessions))]
    flags, ns = fl.flags().copy(), fl.n().copy()
    fl.close()
    return dict(finals=finals, oracles=oracles, worst_mu=worst_mu, bad=bad, flags=flags, n=ns)


def test_heterogeneous_fleet_matches_oracle_every_scan(hetero, hetero_run):
    r = hetero_run
    for i, k, mg in r["bad"][:4]:
        print(f"member {i} event {k}: association differs; oracle margins (|d1 - 0.6|, d2 - d1) per observation: {mg}")
    assert not r["bad"], f"{len(r['bad'])} scans with other associations than the oracle"
    print(f"max |mu - oracle| over every scan of 6 members: {r['worst_mu']:.3e}")
    assert r["worst_mu"] < MU_TOL
    worst_s = 0.0
    for i, (L, _, _) in enumerate(HETERO):
        mo, Po = r["oracles"][i].state()
        assert r["n"][i] == mo.shape[0] and 65 <= r["n"][i] <= 3 + 2 * L      # (inside the capacity: every reflector the session meets)
        worst_s = max(worst_s, float(np.abs(r["finals"][i][1] - Po).max()))
        assert float(np.abs(r["finals"][i][0] - mo).max()) < MU_TOL
    print(f"max |sigma - oracle| at the end: {worst_s:.3e}")
    assert worst_s < SIGMA_TOL
    assert not r["flags"].any()


def test_call_pattern_does_not_change_the_bits(hetero, hetero_run):
    """All events between two scans of ALL members in one submit, nothing read until the end."""
    sessions, evs = hetero
    F = fleet_mod()
    fl = F.ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions], max_landmarks=128)
    pos = [0] * len(evs)
    while any(pos[i] < len(evs[i]) for i in range(len(evs))):
        batch = []
        for i, e in enumerate(evs):
            while pos[i] < len(e):
                ev = e[pos[i]]
                batch.append(fev(i, ev))
                pos[i] += 1
                if ev[0] == synth.EV_SCAN:
                    break
        fl.submit(batch)
    for i in range(len(evs)):
        got = state_bits(fl, i)
        assert same_bits(got, hetero_run["finals"][i]), f"member {i}: batching changed the result"
        mo, Po = hetero_run["oracles"][i].state()
        assert float(np.abs(got[0] - mo).max()) < MU_TOL and float(np.abs(got[1] - Po).max()) < SIGMA_TOL
    fl.close()


def test_composition_does_not_change_the_bits(hetero, hetero_run):
    sessions, evs = hetero
    F = fleet_mod()
    ref = hetero_run["finals"][0]
    # alone
    fl = F.ReflectorEKFSLAMFleet([S.options_for(sessions[0])], max_landmarks=128)
    for ev in evs[0]:
        fl.submit([fev(0, ev)])
    assert same_bits(state_bits(fl, 0), ref), "a fleet of one gives other bits"
    fl.close()
    # member 37 of 64, the others on other seeds (shorter sessions), then with the members' events in shuffled order
    others = [synth.make_session(synth.SessionConfig(f"o{j}", 24 + 8 * j, 8, synth.DIFF if j & 1 else synth.OMNI, seed=7100 + j),
                                 max_scans=150) for j in range(4)]
    oev = [events_of(s) for s in others]
    for shuffle in (False, True):
        rng = np.random.default_rng(5)
        opts = [S.options_for(sessions[0]) if b == 37 else S.options_for(others[b % 4]) for b in range(64)]
        fl = F.ReflectorEKFSLAMFleet(opts, max_landmarks=128)
        for k in range(len(evs[0])):
            tick = [fev(b, evs[0][k]) if b == 37 else fev(b, oev[b % 4][k]) for b in range(64) if b == 37 or k < len(oev[b % 4])]
            if shuffle:
                tick = [tick[q] for q in rng.permutation(len(tick))]
            fl.submit(tick)
        assert same_bits(state_bits(fl, 37), ref), f"member 37 of 64 (shuffle={shuffle}) gives other bits"
        a, b = state_bits(fl, 1), state_bits(fl, 5)
        assert same_bits(a, b)
        fl.close()


def test_more_members_than_cus():
    F = fleet_mod()
    seeds, clones, scans = 8, 64, 200
    sessions = [synth.make_session(synth.SessionConfig(f"c2_{i}", 128, 16, synth.DIFF, seed=7000 + i)) for i in range(seeds)]
    oracles, steady = [], []
    for s in sessions:
        o = oracle_for(s)
        S.replay(s, o)
        oracles.append(o)
        steady.append(synth.steady_state_scans(s, scans))
    B = seeds * clones
    fl = F.ReflectorEKFSLAMFleet([S.options_for(sessions[b % seeds]) for b in range(B)], max_landmarks=128)
    for b in range(B):
        o = oracles[b % seeds]
        mu, P = o.state()
        fl.set_state(b, o.time, mu, P, o.vt())
    for k in range(scans):
        fl.submit([(b, synth.EV_SCAN, steady[b % seeds][k][0], (0.0, 0.0, 0.0), steady[b % seeds][k][1]) for b in range(B)])
    for i in range(seeds):
        for t, cloud in steady[i]:
            oracles[i].handle_observation(t, cloud)
    assert not fl.flags().any()
    for i in range(seeds):
        first = state_bits(fl, i)
        for c in (1, 17, clones - 1):
            assert same_bits(state_bits(fl, i + seeds * c), first), f"seed {i}: clone {c} differs from clone 0"
        mo, Po = oracles[i].state()
        assert float(np.abs(first[0] - mo).max()) < MU_TOL
        assert float(np.abs(first[1] - Po).max()) < SIGMA_TOL
    _, mu3, _ = fl.poses()
    for b in range(B):
        assert np.array_equal(mu3[b], mu3[b % seeds])
    fl.close()


def test_against_the_single_filter():
    F = fleet_mod()
    sess = synth.make_session(synth.C2)
    cfg = sess.config
    fl = F.ReflectorEKFSLAMFleet([S.options_for(sess)], max_landmarks=128)
    m = fl.member(0)
    g = make_gpu(cfg.odom_model, sess.init_time, sess.init_pose, cfg.sigma_v ** 2, cfg.sigma_w ** 2, cfg.sigma_obs ** 2, max_landmarks=128)
    worst = 0.0
    for ev in events_of(sess):
        feed(m, ev)
        feed(g, ev)
        if ev[0] == synth.EV_SCAN:
            a, b = norm_match(m.last_match()), norm_match(g.last_match())
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), ev[1]
            ma, mb = m.mu(), g.mu()
            assert ma.shape == mb.shape
            worst = max(worst, float(np.abs(ma - mb).max()))
    sa, sb = m.GetState(), g.GetState()
    print(f"fleet member vs single filter over C2: max |dmu| {worst:.3e}, final |dsigma| {np.abs(sa.sigma - sb.sigma).max():.3e}")
    assert worst < MU_TOL
    assert float(np.abs(sa.sigma - sb.sigma).max()) < SIGMA_TOL
    fl.close()
    g.close()


def test_capacity_is_a_members_own_affair():
    F = fleet_mod()
    cfgs = [synth.SessionConfig("cap0", 32, 8, synth.DIFF, seed=7200), synth.SessionConfig("cap1", 64, 8, synth.DIFF, seed=7201),
            synth.SessionConfig("cap2", 40, 8, synth.OMNI, seed=7202)]
    sessions = [synth.make_session(c) for c in cfgs]
    evs = [events_of(s) for s in sessions]

    def run(skip=None):
        fl = F.ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions], max_landmarks=48)
        for k in range(max(len(e) for e in evs)):
            tick = [fev(i, e[k]) for i, e in enumerate(evs) if k < len(e) and i != skip]
            if tick:
                fl.submit(tick)
        out = [state_bits(fl, i) for i in range(3)], fl.n().copy(), fl.flags().copy()
        fl.close()
        return out

    states, n, flags = run()
    assert n[1] == 99 and flags[1] & FLAG_CAPACITY
    assert flags[0] == 0 and flags[2] == 0 and 3 < n[0] <= 67 and 3 < n[2] <= 83
    c = cfgs[1]
    g = make_gpu(c.odom_model, sessions[1].init_time, sessions[1].init_pose, c.sigma_v ** 2, c.sigma_w ** 2, c.sigma_obs ** 2, max_landmarks=48)
    for ev in evs[1]:
        feed(g, ev)
    st = g.GetState()
    assert st.mu.shape[0] == 99 and g.flags() & FLAG_CAPACITY
    assert float(np.abs(states[1][0] - st.mu).max()) < MU_TOL
    assert float(np.abs(states[1][1] - st.sigma).max()) < SIGMA_TOL
    g.close()
    states2, n2, flags2 = run(skip=1)
    assert n2[1] == 3 and flags2[1] == 0
    for i in (0, 2):
        assert same_bits(states[i], states2[i]), f"member {i} felt its neighbour's overflow"


def test_boundaries():
    F = fleet_mod()
    sess = synth.make_session(synth.SessionConfig("bnd", 24, 8, synth.DIFF, seed=7300), max_scans=60)
    ev = events_of(sess)
    B = 3
    fl = F.ReflectorEKFSLAMFleet([S.options_for(sess)] * B, max_landmarks=32)
    o = oracle_for(sess)
    for e in ev:
        fl.submit([fev(b, e) for b in range(B)])
        feed(o, e)
    # set_state / GetState round trip on member 1; members 0 and 2 untouched
    before = [state_bits(fl, b) for b in range(B)]
    mo, Po = o.state()
    rng = np.random.default_rng(3)
    A = rng.normal(size=(mo.shape[0], mo.shape[0])) * 1e-2
    P2 = A @ A.T + Po
    P2 = np.tril(P2) + np.tril(P2, -1).T
    mu2 = mo + 0.01
    fl.set_state(1, o.time + 0.5, mu2, P2, (0.1, 0.0, 0.02))
    st = fl.get_state(1)
    assert st.time == o.time + 0.5 and np.array_equal(st.mu, mu2) and np.array_equal(st.sigma, P2)
    assert same_bits(state_bits(fl, 0), before[0]) and same_bits(state_bits(fl, 2), before[2])
    fl.set_state(1, o.time, mo, Po, o.vt())
    # stale odometry is dropped, an empty scan is a Predict: as the oracle
    t_last = o.time
    for filt in (fl.member(1), o):
        filt.handle_odometry(t_last - 0.05, 0.3, 0.0, 0.1)
        filt.handle_odometry(t_last + 0.02, 0.4, 0.0, 0.05)
        filt.handle_observation(t_last + 0.1, np.zeros((0, 2), np.float32))
    st = fl.get_state(1)
    mo, Po = o.state()
    assert st.time == o.time
    assert float(np.abs(st.mu - mo).max()) < MU_TOL and float(np.abs(st.sigma - Po).max()) < SIGMA_TOL
    sp, mp, nw = norm_match(fl.last_match(1))
    assert sp.shape[0] == 0 and nw.shape[0] == 0
    # one bad event in a submit: its code, and nobody moves
    before = [state_bits(fl, b) for b in range(B)]
    tb = fl.poses()[0].copy()
    good = (0, synth.EV_ODOM, t_last + 1.0, (0.5, 0.0, 0.1), None)
    cloud33 = np.zeros((33, 2), np.float32)
    bad_xy = F.RfleetEvent()
    bad_xy.member, bad_xy.kind, bad_xy.t, bad_xy.K, bad_xy.xy = 2, synth.EV_SCAN, t_last + 1.0, 4, None
    assert fl.submit_code([good, (B, synth.EV_ODOM, t_last + 1.0, (0.0, 0.0, 0.0), None)]) == -1
    assert fl.submit_code([good, (2, synth.EV_SCAN, t_last + 1.0, (0.0, 0.0, 0.0), cloud33)]) == -3
    assert fl.submit_code([good, bad_xy]) == -1
    assert np.array_equal(fl.poses()[0], tb)
    for b in range(B):
        assert same_bits(state_bits(fl, b), before[b])
    # poses() is every member's GetState pose and pose block, bit for bit
    fl.submit([good])
    t, mu3, s33 = fl.poses()
    for b in range(B):
        st = fl.get_state(b)
        assert t[b] == st.time and np.array_equal(mu3[b], st.mu[:3]) and np.array_equal(s33[b], st.sigma[:3, :3])
    assert fl.member(0).sync_code() == 0
    fl.close()
