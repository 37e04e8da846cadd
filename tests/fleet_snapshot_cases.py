"""The shapes and contents of the snapshot / restore tests (tests/test_fleet_snapshot_cpu.py, tests/test_fleet_snapshot_gpu.py).

State dimensions NS: no reflector (3), one (5), both sides of the 16-column panel edge (15, 17), both sides of 32 (31, 33), the last
panel partial and full at capacity (257, 259; ld = 272).  Fleets of max_landmarks 128 (ld 272), 7 (n_max 17, ld 32) and 8 (n_max 19),
B = 1 and 8; member lists all, one and a permuted subset.

Two kinds of content.  INDEX-CODED: every entry of a member's mean and of the lower triangle of its covariance is a distinct value
that encodes (member, row, column), exact in FP64, and the upper triangle handed to set_state holds the negated values, so a
transposed, shifted, mirrored or cross-member entry shows.  REAL: short synthetic sessions (reflector_ekf_slam_amd.synth, as the
other fleet tests use them) grouped into ticks of several messages per member; on a fleet of max_landmarks 7 the first scan of a
member already raises REKF_FLAGBIT_CAPACITY.

An entry (what the witness packs) is a record member, t, vt, n, flags, mu, sigma."""
from __future__ import annotations

from types import SimpleNamespace as NS_

import numpy as np

from tests import fleet_cases as FC

NS = (3, 5, 15, 17, 31, 33, 257, 259)
LISTS = {"all": None, "one": [3], "permuted": [5, 2, 7]}
FLAG_CAPACITY = 1

# (name, max_landmarks, the members' state dimensions)
CODED_FLEETS = (("ml128_B8", 128, NS),
                ("ml7_B8", 7, (3, 5, 15, 17, 17, 15, 5, 3)),
                ("ml8_B8", 8, (19, 17, 3, 15, 5, 19, 17, 3)),
                ("ml128_B1", 128, (259,)),
                ("ml8_B1", 8, (17,)),
                ("ml7_B1", 7, (17,)))


def coded_entry(member, n, salt=0):
    """The index-coded state of `member` at dimension n.  `salt` tells two fleets' contents apart."""
    i = np.arange(n, dtype=np.float64)
    mu = 1e6 * (member + 1) + 1e3 * i + 0.25 + salt
    low = 1e6 * (member + 1) + 1e3 * i[:, None] + i[None, :] + 0.5 + salt          # (row, column)
    sigma = np.where(i[:, None] >= i[None, :], low, -low.T)                        # the upper triangle: the mirrored entry, negated
    return NS_(member=member, t=100.0 + member + 0.125 * salt, vt=np.array([0.5 + member, -0.25 * member, 0.01 * (member + 1) + salt]),
               n=n, flags=0, mu=mu, sigma=sigma)


def coded_entries(dims, salt=0):
    return [coded_entry(b, n, salt) for b, n in enumerate(dims)]


def mirrored(sigma):
    low = np.tril(sigma)
    return low + np.tril(low, -1).T


def listed(entries, members):
    return list(entries) if members is None else [entries[b] for b in members]


def lists_for(B):
    """The member lists a fleet of B members is asked for."""
    return {"all": None, "one": [0]} if B == 1 else dict(LISTS)


def set_coded(fl, entries):
    for e in entries:
        fl.set_state(e.member, e.t, e.mu, e.sigma, e.vt)


# ---- real content: short synthetic sessions ---------------------------------------------------------------------------------------
SESSION_SCANS = 24            # scans per session
SCANS_PER_TICK = 3            # a tick = a member's messages up to and including its next SCANS_PER_TICK scans
T = SESSION_SCANS // SCANS_PER_TICK // 2      # ticks before the snapshot, and after it
WORLD = 40                    # reflectors of a session's world
OBS = 8                       # observations per scan

_sessions = {}


def sessions(B):
    """B short sessions (seeds 8800 + i; DIFF and OMNI alternate; 2 m/s, so new reflectors come into range all the way)."""
    if B not in _sessions:
        from reflector_ekf_slam_amd import synth
        _sessions[B] = [synth.make_session(synth.SessionConfig(f"snap{i}", WORLD, OBS, synth.DIFF if i % 2 == 0 else synth.OMNI, seed=8800 + i,
                                                               speed=2.0, row_spacing=6.0), max_scans=SESSION_SCANS + 1) for i in range(B)]
    return _sessions[B]


def options(B):
    from reflector_ekf_slam_amd import session as S
    return [S.options_for(s) for s in sessions(B)]


def ticks(B, pose_fix=False):
    """-> 2 T ticks; a tick is the list of fleet events (member, kind, t, v, cloud[, fix]) of one submit.  pose_fix: every second scan
    carries a fix, the session's true pose of that message."""
    from reflector_ekf_slam_amd import synth
    per_member = []
    for i, s in enumerate(sessions(B)):
        evs, first, scans = [], True, 0
        chunks = []
        for e in range(s.n_events):
            if s.ev_type[e] == synth.EV_ODOM:
                evs.append((i, FC.EV_ODOM, float(s.ev_time[e]), tuple(float(v) for v in s.odom[e]), None))
                continue
            if first:                                       # (the node's first scan only constructs the filter)
                first = False
                continue
            ev = (i, FC.EV_SCAN, float(s.ev_time[e]), (0.0, 0.0, 0.0), np.ascontiguousarray(s.obs_of(e), np.float32))
            if pose_fix and scans % 2 == 1:
                ev = ev + (tuple(float(v) for v in s.true_pose[e]),)
            evs.append(ev)
            scans += 1
            if scans % SCANS_PER_TICK == 0:
                chunks.append(evs)
                evs = []
        per_member.append(chunks[: 2 * T])
    return [[ev for chunks in per_member for ev in chunks[k]] for k in range(2 * T)]


def last_stamp_and_velocity(tick_list, B, opts):
    """What the host's mirror holds behind the ticks: each member's last message time and last odometry velocity (zero before any)."""
    t = [float(o.init_time) for o in opts]
    vt = [np.zeros(3) for _ in range(B)]
    for tick in tick_list:
        for ev in tick:
            m = ev[0]
            assert ev[2] >= t[m]                           # (no stale message in these sessions: none is dropped)
            t[m] = ev[2]
            if ev[1] == FC.EV_ODOM:
                vt[m] = np.array(ev[3], np.float64)
    return t, vt


def shared_map(B):
    """A pre-loaded map for the fleet: every second reflector of member 0's world, float32, with weights 0.01 I (the map gate of
    0.05 on sqrt(d W d^T) is then 0.5 m: member 0 map-matches some observations and appends the others)."""
    xy = np.ascontiguousarray(sessions(B)[0].landmarks[::2], np.float32)
    cov = np.tile(np.array([[0.01, 0.0], [0.0, 0.01]]), (xy.shape[0], 1, 1))
    return xy, cov


def wide_cloud(k):
    """A scan of 40 observations (wider than MAX_OBS = 32): a lattice 1.5 m apart, far from every session's world, jittered per k."""
    g = np.random.default_rng(990 + k)
    ij = np.stack(np.meshgrid(np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    return np.ascontiguousarray(np.array([300.0, 300.0]) + 1.5 * ij + g.normal(size=ij.shape) * 0.01, np.float32)


# ---- restore over a used member: crafted scans of a robot that stands still ---------------------------------------------------------
def lattice_scan(count, k, origin=(2.0, -4.0)):
    """The first `count` points of a lattice 1.5 m apart (far beyond the 0.6 gate of one another), with a little noise per scan k."""
    g = np.random.default_rng(500 + k)
    ij = np.stack(np.meshgrid(np.arange(4), np.arange(5), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)[:count]
    return np.ascontiguousarray(np.asarray(origin) + 1.5 * ij + g.normal(size=ij.shape) * 0.005, np.float32)


def grow_events(member, t0, counts, origin=(2.0, -4.0)):
    """One odometry message and one scan per entry of `counts` (the reflectors the scan sees): n grows to 3 + 2 max(counts)."""
    out = []
    for k, c in enumerate(counts):
        t = t0 + 0.1 * (k + 1)
        out.append([(member, FC.EV_ODOM, t - 0.05, (0.02, 0.0, 0.01), None),
                    (member, FC.EV_SCAN, t, (0.0, 0.0, 0.0), lattice_scan(c, k, origin))])
    return out
