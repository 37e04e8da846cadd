"""The fleet's pose track on the GPU (-m gpu): every member's pose after every message, written by the step launch itself
(k_fleet_step_track) and read with ``take_track``.

Every record is held to the UNTRACKED TWIN of tests/fleet_track_cases.py -- a second fleet without tracking given the same events
one per submit -- bit for bit in mu, sigma and n; nothing the tracked path computes serves as its own expectation.  Against the CPU
oracle (the node test) the bound is the project's 1e-9 (tests/test_fleet_node_gpu.py)."""
from __future__ import annotations

import copy

import numpy as np
import pytest

from reflector_ekf_slam_amd import synth
from reflector_ekf_slam_amd import session as S
from tests import fleet_cases as FC
from tests import fleet_track_cases as TC
from tests import oracle_fleet_node as OF
from tests.fleet_harness import fleet_mod, make_fleet

pytestmark = pytest.mark.gpu

REKF_ERR_INVALID, REKF_ERR_BUFFER = -1, -6


def test_the_error_codes_are_rekf_h():
    import os
    import re
    from tests.fleet_harness import ROOT
    text = open(os.path.join(ROOT, "include", "rekf.h")).read()
    assert int(re.search(r"REKF_ERR_INVALID\s*=\s*(-?\d+)", text).group(1)) == REKF_ERR_INVALID
    assert int(re.search(r"REKF_ERR_BUFFER\s*=\s*(-?\d+)", text).group(1)) == REKF_ERR_BUFFER


# ---- 1. every event, every chunking ---------------------------------------------------------------------------------------------------
def test_every_event_in_every_chunking():
    """Two sessions whose maps are still being built (n grows inside launches), each fed to three tracked members: one event per
    submit, chunks of 2 / 3 / 5 / 17 events regardless of kind, the whole session in one submit."""
    sessions = [synth.make_session(synth.SessionConfig(f"track{m}", 24, 8, m, seed=7800 + m), max_scans=30) for m in (synth.DIFF, synth.OMNI)]
    evs = [FC.events_of(s) for s in sessions]
    F = fleet_mod()
    tw = F.ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions], max_landmarks=128)
    want = TC.twin_records(tw, [(si, ev) for si, e in enumerate(evs) for ev in e])
    fl = F.ReflectorEKFSLAMFleet([S.options_for(s) for s in sessions for _ in range(3)], max_landmarks=128)
    fl.track(True, 100000)
    chunks_with_scans, appended_inside = 0, 0
    per_launch = {}
    for si, e in enumerate(evs):
        a, b, c = 3 * si, 3 * si + 1, 3 * si + 2
        for ev in e:
            fl.submit([FC.fev(a, ev)])
        pos, q, parts = 0, 0, []
        while pos < len(e):
            size = (2, 3, 5, 17)[q % 4]
            chunk = e[pos: pos + size]
            n_before = int(fl.n()[b])
            fl.submit([FC.fev(b, ev) for ev in chunk])
            part, = fl.take_track([b])
            assert len(part) == len(chunk) and TC.last_record_is_the_slot(fl, part, b), (si, pos)   # the last record of each launch
            scans = sum(1 for ev in chunk if ev[0] == synth.EV_SCAN)
            chunks_with_scans += scans >= 2
            appended_inside += scans >= 2 and int(fl.n()[b]) > n_before
            assert int(part.n[0]) >= n_before and (np.diff(part.n) >= 0).all()
            parts.append(part)
            pos, q = pos + size, q + 1
        per_launch[b] = TC.concat(parts)
        fl.submit([FC.fev(c, ev) for ev in e])
    assert chunks_with_scans >= 2 and appended_inside >= 1
    tracks = fl.take_track()
    for si in range(2):
        a, b, c = 3 * si, 3 * si + 1, 3 * si + 2
        assert len(tracks[b]) == 0 and tracks[b].lost == 0
        assert max(w.n for w in want[si]) > 3 + 2 * 8                            # the map grew behind the first scan
        for form, tr in (("one per submit", tracks[a]), ("chunks", per_launch[b]), ("whole session", tracks[c])):
            TC.assert_records(tr, want[si], f"session {si}, {form}")
            assert tr.lost == 0
        assert TC.last_record_is_the_slot(fl, tracks[c], c)
        ref = FC.state_bits(tw, si)                                              # tracking changes no result
        for m in (a, b, c):
            assert FC.same_bits(FC.state_bits(fl, m), ref), (si, m)
    assert not fl.flags().any() and not tw.flags().any()
    fl.close()
    tw.close()


# ---- 2. fix and map ------------------------------------------------------------------------------------------------------------------
def test_pose_fix_and_shared_map_in_one_tracked_fleet(oracle_lib):
    """Member 0 has a pose fix on every scan, member 1 localises against the shared map, member 2 beside it runs the same messages
    without the map; one tracked submit per tick (a member's messages up to its next scan)."""
    from tests import fleet_map_cases as MC
    from tests import fleet_pose_cases as PC
    pose = PC.sessions()[0]
    assert pose.policy == "every"
    ms = MC.session()
    feeds = [pose.events[:120], ms.events[:120], ms.events[:120]]
    assert all(sum(ev[0] == FC.EV_SCAN for ev in f) >= 10 for f in feeds)
    F = fleet_mod()

    def make():
        fleet = F.ReflectorEKFSLAMFleet([pose.options, ms.options, ms.options], max_landmarks=64)
        fleet.set_map(ms.map_xy, ms.map_cov, members=[1])
        return fleet

    tw, fl = make(), make()
    want = TC.twin_records(tw, [(m, ev) for m, f in enumerate(feeds) for ev in f])
    fl.track()
    pos = [0, 0, 0]
    while any(p < len(f) for p, f in zip(pos, feeds)):
        tick = []
        for m, f in enumerate(feeds):
            while pos[m] < len(f):
                ev = f[pos[m]]
                pos[m] += 1
                tick.append(FC.fev(m, ev))
                if ev[0] == FC.EV_SCAN:
                    break
        fl.submit(tick)
    tracks = fl.take_track()
    for m in range(3):
        TC.assert_records(tracks[m], want[m], f"member {m}")
        assert FC.same_bits(FC.state_bits(fl, m), FC.state_bits(tw, m))
    assert sum(w.n_map for w in want[1]) > 0 and int(tracks[1].n_map.sum()) == sum(w.n_map for w in want[1])
    assert not tracks[0].n_map.any() and not tracks[2].n_map.any()
    assert tracks[1].mu.tobytes() != tracks[2].mu.tobytes()
    fl.close()
    tw.close()


# ---- 3. dropped and empty --------------------------------------------------------------------------------------------------------------
def test_dropped_messages_and_empty_scans():
    a, b = FC.plain_neighbours()
    imu = copy.copy(a)
    imu.use_imu, imu.name = True, "use_imu"
    cases = [a, imu, b]
    fl, tw = make_fleet(cases), make_fleet(cases)
    fl.track()
    t0, mu0, sg0 = fl.poses()
    empty = np.zeros((0, 2), np.float32)
    calls = [
        # every event is dropped on the host: stale odometry twice, a use_imu member's odometry
        [(0, (FC.EV_ODOM, a.t - 0.5, (0.4, 0.0, 0.1), None)), (1, (FC.EV_ODOM, imu.t + 0.05, (0.4, 0.0, 0.1), None)),
         (0, (FC.EV_ODOM, a.t - 0.1, (0.2, 0.0, 0.0), None))],
        # stale, good, a scan with K = 0 (a Predict), stale again, the member's scan -- and the use_imu member's odometry between scans
        [(0, (FC.EV_ODOM, a.t - 0.2, (0.9, 0.0, 0.3), None)), (0, (FC.EV_ODOM, a.t + 0.04, (0.5, 0.0, 0.2), None)),
         (0, (FC.EV_SCAN, a.t + 0.06, (0.0, 0.0, 0.0), empty)), (0, (FC.EV_ODOM, a.t + 0.05, (0.7, 0.0, 0.0), None)),
         (0, a.events[0]),
         (1, (FC.EV_SCAN, imu.t + 0.02, (0.0, 0.0, 0.0), empty)), (1, (FC.EV_ODOM, imu.t + 0.03, (0.4, 0.0, 0.1), None)), (1, a.events[0]),
         (2, (FC.EV_ODOM, b.t + 0.5, (1.0, 0.0, 0.5), None))],
    ]
    want = TC.twin_records(tw, [x for call in calls for x in call], use_imu={1})
    first = fl.submit_code([FC.fev(m, ev) for m, ev in calls[0]])
    assert first == 0
    got0 = fl.take_track()
    assert [len(g) for g in got0] == [2, 1, 0]
    for m, g in enumerate(got0[:2]):                                             # before the first record: poses() before the submit
        for r in range(len(g)):
            assert g.dropped[r] == 1 and g.mu[r].tobytes() == mu0[m].tobytes() and g.sigma[r].tobytes() == sg0[m].tobytes()
            assert g.n[r] == cases[m].mu.shape[0] and g.kind[r] == FC.EV_ODOM
    assert list(got0[0].t) == [a.t - 0.5, a.t - 0.1] and list(got0[1].t) == [imu.t + 0.05]
    assert np.array_equal(fl.poses()[0], t0)                                      # no member's time moved
    fl.submit([FC.fev(m, ev) for m, ev in calls[1]])
    got1 = fl.take_track()
    tracks = [TC.concat([x, y]) for x, y in zip(got0, got1)]
    for m in range(3):
        TC.assert_records(tracks[m], want[m], cases[m].name)
        assert FC.same_bits(FC.state_bits(fl, m), FC.state_bits(tw, m))           # state and time: an untracked fleet's after the same calls
    assert np.array_equal(fl.poses()[0], tw.poses()[0])
    assert list(tracks[0].dropped) == [1, 1, 1, 0, 0, 1, 0] and list(tracks[1].dropped) == [1, 0, 1, 0] and list(tracks[2].dropped) == [0]
    # a dropped record repeats the record before it, with the message's stamp
    for tr in tracks[:2]:
        for r in range(1, len(tr)):
            if tr.dropped[r]:
                assert tr.mu[r].tobytes() == tr.mu[r - 1].tobytes() and tr.sigma[r].tobytes() == tr.sigma[r - 1].tobytes() and tr.n[r] == tr.n[r - 1]
    # the K = 0 scan's record is the Predict's pose: what an odometry-less Predict to that stamp gives (the twin's, and it moved)
    k0 = tracks[0]
    assert k0.kind[4] == FC.EV_SCAN and k0.K[4] == 0 and (k0.n_state[4], k0.n_new[4]) == (0, 0)
    assert k0.mu[4].tobytes() != k0.mu[3].tobytes() and k0.sigma[4].tobytes() != k0.sigma[3].tobytes()
    fresh = make_fleet([a])
    fresh.submit([FC.fev(0, calls[1][1][1])])
    mu_p, sg_p = fresh.predict_poses([a.t + 0.06])
    assert float(np.abs(mu_p[0] - k0.mu[4]).max()) < 1e-12 and float(np.abs(sg_p[0] - k0.sigma[4]).max()) < 1e-12 and k0.t[4] == a.t + 0.06
    fresh.close()
    fl.close()
    tw.close()


# ---- 4. ring and bound -------------------------------------------------------------------------------------------------------------------
def test_track_goes_round_the_ring_and_the_log_is_bounded():
    """Forty tracked submits without a getter (five times round the ring of eight segments, sizes as in
    test_staging_ring_goes_round_and_grows, the track area in them), then ONE take: every record, in order, as a run that
    synchronises and takes after every submit."""
    base = next(c for c in FC.map_cases() if c.name == "map_L128_K32_all_matched")
    B = 48
    cloud = base.events[0][3]

    def run(synchronise):
        fl = make_fleet([base] * B)
        fl.track()
        parts = [[] for _ in range(B)]
        for q in range(40):
            members = 8 if q < 8 else 24 if q < 16 else 48
            fl.submit([(b, FC.EV_SCAN, base.t + 0.1 * (q + 1), (0.0, 0.0, 0.0), cloud) for b in range(members)])
            if synchronise:
                for b, p in enumerate(fl.take_track()):
                    parts[b].append(p)
        for b, p in enumerate(fl.take_track()):
            parts[b].append(p)
        out = [TC.concat(p) for p in parts], [FC.state_bits(fl, b) for b in (0, 8, 24)]
        fl.close()
        return out

    free, fbits = run(False)
    sync, sbits = run(True)
    assert [len(t) for t in free] == [40] * 8 + [32] * 16 + [24] * 24
    for b in range(B):
        f, s = free[b], sync[b]
        assert f.lost == 0 and len(f) == len(s)
        for k in ("t", "kind", "K", "dropped", "mu", "sigma", "n", "flags", "n_state", "n_map", "n_new"):
            assert getattr(f, k).tobytes() == getattr(s, k).tobytes(), (b, k)
        assert (np.diff(f.t) > 0).all() and (f.n_state == 32).all() and (f.K == 32).all()
    for x, y in zip(fbits, sbits):
        assert FC.same_bits(x, y)
    assert free[0].mu[-1].tobytes() != free[0].mu[0].tobytes()
    # the bound: ten events per member, four records kept -- the four NEWEST
    a, b = FC.plain_neighbours()
    fl, tw = make_fleet([a, b]), make_fleet([a, b])
    fl.track(True, 4)
    feed = [(m, (FC.EV_ODOM, c.t + 0.01 * (k + 1), (0.3 + 0.01 * k, 0.0, 0.05), None)) for k in range(10) for m, c in enumerate((a, b))]
    want = TC.twin_records(tw, feed)
    fl.submit([FC.fev(m, ev) for m, ev in feed[:8]])
    fl.submit([FC.fev(m, ev) for m, ev in feed[8:]])
    for m, tr in enumerate(fl.take_track()):
        assert tr.lost == 6
        TC.assert_records(tr, want[m][-4:], f"bounded {m}")
    assert [t.lost for t in fl.take_track()] == [0, 0]
    fl.close()
    tw.close()


# ---- 5. take semantics --------------------------------------------------------------------------------------------------------------------
def test_take_semantics():
    a, b = FC.plain_neighbours()
    cases = [a, b, a]
    fl, tw = make_fleet(cases), make_fleet(cases)
    F = fleet_mod()
    assert all(len(t) == 0 for t in fl.take_track())                             # tracking off: zero counts
    fl.submit([(0, FC.EV_ODOM, a.t + 0.01, (0.3, 0.0, 0.05), None)])             # not tracked
    fl.track()
    feed = [(m, (FC.EV_ODOM, c.t + 0.02 + 0.01 * k, (0.3, 0.0, 0.05 * (m + 1)), None)) for k in range(3) for m, c in enumerate(cases)]
    feed += [(2, a.events[0])]
    tw.submit([(0, FC.EV_ODOM, a.t + 0.01, (0.3, 0.0, 0.05), None)])
    want = TC.twin_records(tw, feed)
    fl.submit([FC.fev(m, ev) for m, ev in feed])
    counts = np.full(3, -7, np.int32)
    out = np.zeros(16, F.TRACK_DTYPE)
    out["t"] = -1.0
    lost = np.zeros(3, np.int64)
    # too small: the counts, no output touched, nothing removed
    assert fl.take_track_code(None, counts, out[:9], 9, lost) == REKF_ERR_BUFFER
    assert counts.tolist() == [3, 3, 4] and (out["t"] == -1.0).all()
    # refused lists
    assert fl.take_track_code([0, 0], counts, out, 16, None) == REKF_ERR_INVALID
    assert fl.take_track_code([0, 3], counts, out, 16, None) == REKF_ERR_INVALID
    assert fl.take_track_code([-1], counts, out, 16, None) == REKF_ERR_INVALID
    assert fl.take_track_code([0, 1], counts, out, -1, None) == REKF_ERR_INVALID
    assert fl.take_track_code([0, 1], None, out, 16, None) == REKF_ERR_INVALID
    assert (out["t"] == -1.0).all()
    # a subset in a given order
    two = fl.take_track([2, 0])
    TC.assert_records(two[0], want[2], "member 2 of [2, 0]")
    TC.assert_records(two[1], want[0], "member 0 of [2, 0]")
    assert (two[0].n_state[-1], two[0].n_new[-1]) == (2, 1) and two[0].K[-1] == 3
    # the second call with room returns everything that is left; a second take is empty
    assert fl.take_track_code(None, counts, out, 16, lost) == 0 and counts.tolist() == [0, 3, 0] and not lost.any()
    assert out["t"][:3].tolist() == [w.t for w in want[1]] and out["mu3"][:3].tobytes() == np.array([w.mu for w in want[1]]).tobytes()
    assert out["member"][:3].tolist() == [1, 1, 1] and (out["t"][3:] == -1.0).all()
    assert all(len(t) == 0 for t in fl.take_track())
    # set_state logs nothing; tracking switched off logs nothing for later submits and keeps what was logged
    fl.submit([(1, FC.EV_ODOM, b.t + 0.2, (0.3, 0.0, 0.05), None)])
    fl.set_state(1, b.t, b.mu, b.P, b.vt)
    fl.track(False)
    fl.submit([(1, FC.EV_ODOM, b.t + 0.3, (0.3, 0.0, 0.05), None), (0, FC.EV_ODOM, a.t + 0.3, (0.3, 0.0, 0.05), None)])
    fl.set_state(0, a.t, a.mu, a.P, a.vt)
    left = fl.take_track()
    assert [len(t) for t in left] == [0, 1, 0] and left[1].t[0] == b.t + 0.2
    fl.close()
    tw.close()


# ---- 6. more workgroups than compute units ------------------------------------------------------------------------------------------------------
def test_three_hundred_members_in_one_tracked_submit():
    B = 300
    lms = FC.far_lattice(3)
    rng = np.random.default_rng(8100)
    cases = []
    for i in range(B):
        cloud = [(lms[i % 3][0] + (i % 7 - 3) / 256, lms[i % 3][1] + (i % 5 - 2) / 256), (-1.0 - (i % 4) * 0.25, 0.5 + (i % 3) * 0.125)]
        c = FC._case(f"m{i}", "track", FC.DIFF if i & 1 else FC.OMNI, np.concatenate([[0.0, 0.0, 0.0], np.asarray(lms).reshape(-1)]),
                     FC.dense_spd(9, np.random.default_rng(8200 + i), 1e-3), (0.0, 0.0, 0.0), 50.0,
                     [(FC.EV_ODOM, 50.05, (0.2 + 0.001 * i, 0.0, float(rng.uniform(-0.1, 0.1))), None),
                      (FC.EV_SCAN, 50.1, (0.0, 0.0, 0.0), np.asarray(cloud, np.float32)),
                      (FC.EV_ODOM, 50.15, (0.3, 0.0, 0.1), None)], {})
        cases.append(c)
    fl, tw = make_fleet(cases, max_landmarks=4), make_fleet(cases, max_landmarks=4)
    fl.track()
    want = {m: [] for m in range(B)}
    for k in range(3):                                                           # the twin's three submits, a getter round after each
        tw.submit([FC.fev(m, c.events[k]) for m, c in enumerate(cases)])
        _, mu, sg = tw.poses()
        n, flags = tw.n(), tw.flags()
        for m, c in enumerate(cases):
            ev = c.events[k]
            ns = nn = 0
            if k == 1 and m % 25 == 0:
                rec = tw.last_match(m)
                ns, nn = rec.state_obs_match_ids.shape[0], rec.new_ids.shape[0]
                assert (ns, nn) == (1, 1)
            elif k == 1:
                ns, nn = 1, 1                                                    # (by construction; every 25th member is read back)
            want[m].append(TC.NS(t=ev[1], kind=ev[0], K=2 if k == 1 else 0, dropped=0, mu=mu[m].copy(), sigma=sg[m].copy(), n=int(n[m]),
                                 flags=int(flags[m]), n_state=ns, n_map=0, n_new=nn))
    fl.submit([FC.fev(m, ev) for k in range(3) for m, c in enumerate(cases) for ev in [c.events[k]]])
    tracks = fl.take_track()
    for m in range(B):
        TC.assert_records(tracks[m], want[m], f"member {m}")
    assert (tracks[0].n == [9, 11, 11]).all() and TC.last_record_is_the_slot(fl, tracks[B - 1], B - 1)
    for m in (0, 149, 299):
        assert FC.same_bits(FC.state_bits(fl, m), FC.state_bits(tw, m))
    fl.close()
    tw.close()


# ---- 7. the node ----------------------------------------------------------------------------------------------------------------------------
NODE_SHAPES = ((14, 1440), (12, 2880), (9, 1440))      # tests/test_fleet_node_gpu.py's dumps
NODE_START = (0, 3, 1)


def test_fleet_node_pose_log_against_three_oracle_nodes(oracle_lib, tmp_path):
    from reflector_ekf_slam_amd.node_replay import FleetNode, Node, synth_dump
    from tests.oracle_node import oracle_backend
    cfgs = [synth.SessionConfig(f"node{i}", 40, 12, synth.DIFF, seed=31 + i, speed=1.0, row_spacing=6.0) for i in range(3)]
    dumps = [synth_dump(str(tmp_path / f"robot{i}.npz"), cfg, max_scans=n, n_beams=beams) for i, (cfg, (n, beams)) in enumerate(zip(cfgs, NODE_SHAPES))]
    nodes = []
    for d in dumps:
        node = Node(d.meta, OF.recording(oracle_backend()))
        node.run(d)
        nodes.append(node)
    fn = FleetNode([d.meta for d in dumps], pose_log=True)
    fn.run(dumps, NODE_START)
    assert OF.differences(fn, nodes, pose_tol=1e-9, match_poses=False) == []
    for m, node in enumerate(nodes):
        log, want = fn.logs[m], node.log.path
        assert len(log.pose_log) == len(want) > len(log.path) > 0                # as many entries as the node's path
        assert [e[0] for e in log.pose_log] == [p[0] for p in want]              # the stamps
        err = float(np.abs(np.array([e[1:4] for e in log.pose_log]) - np.array([p[1:] for p in want])).max())
        print(f"robot {m}: {len(want)} entries, max|pose - oracle node| = {err:.3e}")
        assert err < 1e-9
        by_stamp = {e[0]: e for e in log.pose_log}
        for p in log.path:                                                       # the scan entries: the bits of the same node's path
            assert by_stamp[p[0]][:4] == p
        t_end, _, sg_end = fn.fleet.poses()
        assert log.pose_log[-1][0] == t_end[m] and np.array_equal(log.pose_log[-1][4], sg_end[m])   # the covariance beside the last entry
    assert all(len(t) == 0 for t in fn.fleet.take_track())
    fn.detector.close()
    fn.fleet.close()
    fn.map_builder._fleet.close()
