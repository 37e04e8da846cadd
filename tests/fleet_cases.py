"""Cases of the fleet filter's shape sweep and edge tests, shared by tests/test_fleet_edges_cpu.py (the cases and the three
CPU references against each other) and tests/test_fleet_edges_gpu.py (k_fleet_step against the longdouble witness).

A case is a plain record: the filter's options, ``max_landmarks``, a state (t, mu, P, vt) to write with ``set_state``, a list
of events ``(kind, t, (vx, vy, wz), cloud or None)``, with the pose fix of a scan or None as an optional fifth element
(tests/fleet_pose_cases.py), and what the case claims about itself: per scan the association lists
(``expect``) and per observation the margins |d1 - 0.6| and d2 - d1 of ReflectorMatch's state branch (``margins``).
numpy only; nothing here needs a GPU.

Shape sweep.  One scan on a set state (and a second one that appends one more reflector, so that rows written past n by the
first become visible).  n = 3 + 2 L is odd, so n + 2 N2 never equals a multiple of 16; the three positions of the appended
rows [n, n + 2 N2) against the 16-row tile that holds row n are therefore
    inside    n + 2 N2 <  n16 - 1
    edge      n + 2 N2 == n16 - 1     (the last state row is row n16 - 2: as close to the edge as an odd n comes)
    straddle  n + 2 N2 == n16 + 1     (a reflector's x in row n16 - 1, its y in the first row of the next tile)
    cross     n + 2 N2 >  n16 + 1
with n16 = roundup(n, 16), next to the plain N2 = 0 and N2 = 1.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from oracle.ekf_numpy import NumpyEKF

DIFF, OMNI = 0, 1
EV_ODOM, EV_SCAN = 0, 1
GATE = 0.6
LIN_COV, ANG_COV, OBS_COV = 0.05 ** 2, 0.08 ** 2, 0.05 ** 2      # launch/slam.launch:21-23, squared
MARGIN_MIN = 1e-3
FLAG_CAPACITY, FLAG_SINGULAR = 1, 2

# ---- the FP64 noise floor --------------------------------------------------------------------------------------------------
# Measured by tests/test_fleet_edges_cpu.py::test_fp64_floor (run it with -s to see the figures): over every scan of every sweep
# and crafted case, the larger error of the two FP64 CPU restatements (oracle/ekf_oracle.c, oracle/ekf_numpy.py) against the
# longdouble witness, as max|dsigma| / max|sigma_ref| and max|dmu| / max(1, max|mu_ref|).  The recorded values are the measured
# maxima rounded up to two digits; the test fails if a re-measurement exceeds them.  (sigma: the update subtracts K H P from a
# P several times larger, with cond(S) in the low thousands; numpy.linalg.inv is the less accurate of the two.)  The GPU bound is GPU_FACTOR times these.
FP64_FLOOR_SIGMA = 1.6e-11    # measured 1.569e-11
FP64_FLOOR_MU = 1.7e-16       # measured 1.613e-16
FP64_FLOOR_SIGMA_CASE = "sweep_L75_MM24_N6_omni scan 0 (numpy)"
FP64_FLOOR_MU_CASE = "sweep_L128_MM32_N0_diff scan 1 (oracle)"
GPU_FACTOR = 16.0
MU_TOL, SIGMA_TOL = 1e-9, 1e-11          # the absolute tolerances of tests/test_fleet_gpu.py: the bound is never looser


def gpu_bounds(mu_ref, P_ref, suite):
    """The GPU test's bounds on (max|dsigma| / max|sigma_ref|, max|dmu| / max(1, max|mu_ref|)): GPU_FACTOR x the suite's FP64
    floor, and never looser than the absolute tolerances (which bind only where the covariance is large, e.g. far new reflectors)."""
    smax, mmax = float(np.abs(P_ref).max()), max(1.0, float(np.abs(mu_ref).max()))
    return min(GPU_FACTOR * suite.floor_sigma, SIGMA_TOL / smax), min(GPU_FACTOR * suite.floor_mu, MU_TOL / mmax)


# ---- helpers shared with tests/test_fleet_gpu.py ---------------------------------------------------------------------------
def events_of(sess, stop=None):
    """The session's messages as the node hands them over (the first scan only constructs the filter: session.replay)."""
    from reflector_ekf_slam_amd import synth
    out, first = [], True
    for e in range(sess.n_events if stop is None else min(stop, sess.n_events)):
        if sess.ev_type[e] == synth.EV_ODOM:
            out.append((synth.EV_ODOM, float(sess.ev_time[e]), tuple(float(v) for v in sess.odom[e]), None))
        elif first:
            first = False
        else:
            out.append((synth.EV_SCAN, float(sess.ev_time[e]), (0.0, 0.0, 0.0), np.ascontiguousarray(sess.obs_of(e), np.float32)))
    return out


def feed(filt, ev):
    """One event to a filter with the snake_case interface (oracle, numpy, witness, fleet member, single filter)."""
    if ev[0] == EV_ODOM:
        filt.handle_odometry(ev[1], *ev[2])
    elif len(ev) == 4 or ev[4] is None:
        filt.handle_observation(ev[1], ev[3])
    else:
        filt.handle_observation(ev[1], ev[3], np.asarray(ev[4], np.float64))


def fev(member, ev, with_fix=True):
    """The event as ReflectorEKFSLAMFleet.pack takes it: a 5-tuple, or a 6-tuple when it carries a fix."""
    if with_fix and len(ev) > 4 and ev[4] is not None:
        return (member, *ev[:4], tuple(ev[4]))
    return (member, *ev[:4])


def margins(mu_pred, cloud):
    """Per observation (|d1 - 0.6|, d2 - d1) of ReflectorMatch's state branch at the predicted mean (float32 / FP64 as cc:426-451)."""
    out = []
    L = (mu_pred.shape[0] - 3) // 2
    c, s = np.cos(mu_pred[2]), np.sin(mu_pred[2])
    for p in np.asarray(cloud, np.float32).reshape(-1, 2):
        gx = np.float32(float(p[0]) * c - float(p[1]) * s + mu_pred[0])
        gy = np.float32(float(p[0]) * s + float(p[1]) * c + mu_pred[1])
        if L == 0:
            out.append((np.inf, np.inf))
            continue
        lm = mu_pred[3:].reshape(-1, 2).astype(np.float32)
        ex, ey = (gx - lm[:, 0]).astype(np.float64), (gy - lm[:, 1]).astype(np.float64)
        dd = np.sort(np.sqrt(ex * ex + ey * ey))
        out.append((abs(dd[0] - 0.6), dd[1] - dd[0] if L > 1 else np.inf))
    return out


def state_bits(fl, i):
    st = fl.get_state(i)
    return st.mu.copy(), np.array(st.sigma, order="F", copy=True)


def same_bits(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- references of a case ---------------------------------------------------------------------------------------------------
def options_of(case):
    from reflector_ekf_slam_amd import EKFOptions
    return EKFOptions(use_imu=bool(case.use_imu), init_time=float(case.t), init_pose=tuple(float(v) for v in case.mu[:3]),
                      odom_model=int(case.model), linear_velocity_cov=LIN_COV, angular_velocity_cov=ANG_COV,
                      observation_cov=OBS_COV)


def numpy_of(case):
    ek = NumpyEKF(case.model, case.t, case.mu[:3], LIN_COV, ANG_COV, OBS_COV)
    ek.mu, ek.sigma, ek.vt = case.mu.copy(), case.P.copy(), np.array(case.vt, np.float64)
    return ek


def oracle_of(case):
    from oracle.binding import OracleEKF
    o = OracleEKF(case.model, case.t, case.mu[:3], LIN_COV, ANG_COV, OBS_COV)
    o.set_state(case.t, case.mu, case.P, case.vt)
    return o


def witness_of(case):
    from tests.witness.fleet_witness import WitnessEKF
    w = WitnessEKF(case.model, case.t, case.mu[:3], LIN_COV, ANG_COV, OBS_COV)
    w.set_state(case.t, case.mu, case.P, case.vt)
    return w


# What differs between the fleet's test suites, for tests/fleet_harness.py: the measured floors and the witnesses (the first is
# the one the GPU is held to).
SUITE = NS(name="plain", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU, witnesses={"witness": witness_of})


def kept_cloud(case, k):
    """Scan k's cloud as a filter WITHOUT capacity limit has to see it: the observations the capacity guard drops removed."""
    cloud = case.events[k][3]
    keep = case.kept.get(k)
    return cloud if keep is None else np.ascontiguousarray(cloud[keep])


def reference_events(case):
    """The case's events for a reference that knows no capacity (dropped observations removed) and no use_imu switch; a
    fix stays."""
    out = []
    for k, ev in enumerate(case.events):
        if ev[0] == EV_ODOM and case.use_imu:
            continue
        out.append((ev[0], ev[1], ev[2], kept_cloud(case, k) if ev[0] == EV_SCAN else None, *ev[4:]))
    return out


def map_back(case, k, pairs, new):
    """Association lists of the truncated scan k in the numbering of the scan as submitted."""
    keep = case.kept.get(k)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2).copy()
    new = np.asarray(new, np.int32).reshape(-1).copy()
    if keep is not None:
        keep = np.asarray(keep)
        if pairs.shape[0]:
            pairs[:, 0] = keep[pairs[:, 0]]
        new = keep[new].astype(np.int32)
    return pairs, new


# ---- building blocks --------------------------------------------------------------------------------------------------------
def dense_spd(n, rng, scale, d_lo=1e-4, d_hi=1e-3):
    """P = A A^T * s + D: dense, exactly symmetric, diagonal about `scale` + [d_lo, d_hi]."""
    A = rng.normal(size=(n, n))
    P = (A @ A.T) * (scale / n) + np.diag(rng.uniform(d_lo, d_hi, size=n))
    return np.tril(P) + np.tril(P, -1).T


def predict_pose(model, mu3, vt, dt):
    x, y, th = (float(v) for v in mu3)
    vx, vy, w = vt
    if model == DIFF:
        half = th + w * dt / 2
        x, y = x + vx * dt * math.cos(half), y + vx * dt * math.sin(half)
    else:
        x, y = x + (vx * math.cos(th) - vy * math.sin(th)) * dt, y + (vx * math.sin(th) + vy * math.cos(th)) * dt
    th = th + w * dt
    return x, y, math.atan2(math.sin(th), math.cos(th))


def to_local(pose, g):
    x, y, th = pose
    c, s = math.cos(th), math.sin(th)
    dx, dy = g[0] - x, g[1] - y
    return (dx * c + dy * s, -dx * s + dy * c)


def innovation_cov(mu_p, P_p, pairs):
    m = 2 * len(pairs)
    H = np.zeros((m, mu_p.shape[0]))
    c, s = math.cos(mu_p[2]), math.sin(mu_p[2])
    for i, (_, g) in enumerate(pairs):
        dx, dy = mu_p[3 + 2 * g] - mu_p[0], mu_p[4 + 2 * g] - mu_p[1]
        H[2 * i, 0:3] = [-c, -s, -dx * s + dy * c]
        H[2 * i + 1, 0:3] = [s, -c, -dx * c - dy * s]
        H[2 * i: 2 * i + 2, 3 + 2 * g: 5 + 2 * g] = [[c, s], [-s, c]]
    return H @ P_p @ H.T + OBS_COV * np.eye(m)


def _case(name, kind, model, mu, P, vt, t, events, expect, max_landmarks=128, use_imu=False, kept=None, **tags):
    return NS(name=name, kind=kind, model=model, use_imu=use_imu, max_landmarks=max_landmarks, t=float(t),
              mu=np.asarray(mu, np.float64), P=np.asarray(P, np.float64), vt=tuple(float(v) for v in vt), events=events,
              expect=expect, kept=kept or {}, margins={}, cond_S={}, **tags)


def annotate(case):
    """Fills case.margins[k] and case.cond_S[k] for every scan event k from a run of oracle/ekf_numpy.py over the reference
    events (predicted mean and covariance of each scan)."""
    ek = numpy_of(case)
    for k, ev in enumerate(case.events):
        if ev[0] == EV_ODOM:
            if not case.use_imu:
                ek.handle_odometry(ev[1], *ev[2])
            continue
        cloud = kept_cloud(case, k)
        mu_p, P_p = ek.predict_state(ev[1])
        case.margins[k] = margins(mu_p, cloud)
        pairs = [(l, g) for l, g in np.asarray(case.expect[k][0]).reshape(-1, 2) if True]
        if len(pairs) and not getattr(case, "singular", False):
            case.cond_S[k] = float(np.linalg.cond(innovation_cov(mu_p, P_p, pairs)))
        if getattr(case, "singular", False):
            break
        ek.handle_observation(ev[1], cloud)
    return case


# ---- the shape sweep --------------------------------------------------------------------------------------------------------
MM_LISTED = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32)
N_LISTED = (5, 15, 17, 31, 33, 127, 129, 255, 257, 259)
# (m4 % 8 class, m16) -> matched counts of MM_LISTED that fall into it; m = 2 MM, m4 = roundup(m, 4), m16 = roundup(m, 16)
M_CLASSES = {("lt8", 16): (1, 2), ("0", 16): (3, 4, 7, 8), ("4", 16): (5,), ("0", 32): (15, 16), ("4", 32): (9,),
             ("0", 48): (23, 24), ("4", 48): (17,), ("0", 64): (31, 32), ("4", 64): (25,)}
GRID, PITCH, JITTER = 12, 2.0, 0.2          # 144 lattice cells, reflectors at least 1.6 m apart


def m_class(MM):
    m = 2 * MM
    m4, m16 = (m + 3) & ~3, (m + 15) & ~15
    return ("lt8" if m4 < 8 else str(m4 % 8), m16)


def n2_class(n, N2):
    if N2 <= 1:
        return str(N2)
    n16, na = (n + 15) & ~15, n + 2 * N2
    return "inside" if na < n16 - 1 else "edge" if na == n16 - 1 else "straddle" if na == n16 + 1 else "cross"


def n2_for(n, cls, MM):
    """New count that puts n + 2 N2 into class `cls`, or None when n, the 32-observation limit or the capacity forbid it."""
    n16, L = (n + 15) & ~15, (n - 3) // 2
    e = n16 - n                              # odd, 1 .. 15
    N2 = {"0": 0, "1": 1, "inside": (e - 3) // 2, "edge": (e - 1) // 2, "straddle": (e + 1) // 2, "cross": (e + 1) // 2 + 2}[cls]
    if N2 < 0 or MM + N2 > 32 or L + N2 > 128 or n2_class(n, N2) != cls:
        return None
    return N2


def sweep_case(L, MM, N2, model, seed, scale=None, name="sweep"):
    rng = np.random.default_rng(seed)
    n = 3 + 2 * L
    cells = rng.permutation(GRID * GRID)
    pts = np.stack([cells % GRID, cells // GRID], -1) * PITCH + rng.uniform(-JITTER, JITTER, size=(GRID * GRID, 2))
    pts = pts.astype(np.float32).astype(np.float64)
    lm, free = pts[:L], pts[L:]
    if L > 1:                                            # new points: only cells whose two nearest reflectors are not nearly equidistant
        d = np.sort(np.hypot(lm[None, :, 0] - free[:, None, 0], lm[None, :, 1] - free[:, None, 1]), axis=1)
        free = free[d[:, 1] - d[:, 0] >= 0.05]
    assert free.shape[0] > N2, (L, N2)
    mu = np.zeros(n)
    mu[0:2] = 0.5 * GRID * PITCH + rng.uniform(-1.5, 1.5, size=2)
    mu[2] = rng.uniform(-3.0, 3.0)
    mu[3:] = lm.reshape(-1)
    if scale is None:
        P = dense_spd(n, rng, 10.0 ** rng.uniform(-3.7, -2.3))   # diagonal 3e-4 .. 6e-3: cond(S) stays in the hundreds
    else:
        P = dense_spd(n, rng, scale, 1e-4, 2e-4)
    vt = (rng.uniform(0.2, 1.0), rng.uniform(-0.3, 0.3) if model == OMNI else 0.0, rng.uniform(-0.4, 0.4))
    t0, dt = 100.0, 0.1
    pose = predict_pose(model, mu[:3], vt, dt)
    matched = rng.choice(L, size=MM, replace=False)
    slots = rng.permutation(MM + N2)
    cloud = np.zeros((MM + N2, 2), np.float32)
    pairs, new = [], []
    for q in range(MM + N2):
        if slots[q] < MM:
            g = lm[matched[slots[q]]] + rng.uniform(-2e-3, 2e-3, size=2)
            pairs.append((q, int(matched[slots[q]])))
        else:
            g = free[slots[q] - MM]
            new.append(q)
        cloud[q] = to_local(pose, g)
    events = [(EV_SCAN, t0 + dt, (0.0, 0.0, 0.0), cloud)]
    expect = {0: (pairs, new)}
    case = _case(f"{name}_L{L}_MM{MM}_N{N2}_{'diff' if model == DIFF else 'omni'}", "sweep", model, mu, P, vt, t0, events, expect,
                 L=L, MM=MM, N2=N2, n=n)
    case.kind = name
    # the second scan, on the posterior: one more reflector (or, on a full map, one matched observation)
    ek = numpy_of(case)
    ek.handle_observation(events[0][1], cloud)
    pose2 = ek.predict_state(t0 + 2 * dt)[0][:3]
    if L + N2 < 128:
        cloud2 = np.array([to_local(pose2, free[N2])], np.float32)
        expect[1] = ([], [0])
    else:
        cloud2 = np.array([to_local(pose2, ek.mu[3:5])], np.float32)
        expect[1] = ([(0, 0)], [])
    events.append((EV_SCAN, t0 + 2 * dt, (0.0, 0.0, 0.0), cloud2))
    annotate(case)
    for k in (0, 1):
        for a, b in case.margins[k]:
            assert a >= MARGIN_MIN and b >= MARGIN_MIN, (case.name, k, a, b)       # no sweep case is excused: zero by construction
    return case


def sweep_shapes():
    """(L, MM, N2, model) of every sweep case.  Every (n mod 16) x (m class) combination, every listed n and MM, every N2 class."""
    shapes, seen = [], set()

    def add(L, MM, cls):
        N2 = n2_for(3 + 2 * L, cls, MM)
        if N2 is None or MM > L or (L, MM, N2) in seen:
            return False
        seen.add((L, MM, N2))
        shapes.append((L, MM, N2, DIFF if len(shapes) % 2 == 0 else OMNI))
        return True

    n2_cycle = ("0", "1", "inside", "edge", "straddle", "cross")
    q = 0
    for k in range(8):                                   # L mod 8 <-> n mod 16
        Ls = [L for L in range(k if k else 8, 129, 8)]
        for ci, (cls, mms) in enumerate(sorted(M_CLASSES.items(), key=str)):
            MM = mms[(k + ci) % len(mms)]
            cand = [L for L in Ls if L >= MM]
            L = cand[(k * 3 + ci * 5) % len(cand)]
            for tries in range(6):
                if add(L, MM, n2_cycle[(q + tries) % 6]):
                    break
            else:
                raise AssertionError((L, MM))
            q += 1
    for i, nv in enumerate(N_LISTED):                    # every listed n, with a small and a large scan and two N2 classes
        L = (nv - 3) // 2
        for j, MM in enumerate((MM_LISTED[(3 * i) % 16], MM_LISTED[(3 * i + 8) % 16], 32)):
            MM = min(MM, L)
            for tries in range(6):
                if add(L, MM, n2_cycle[(i + 2 * j + tries) % 6]):
                    break
    for i, MM in enumerate(MM_LISTED):                   # every listed MM with every N2 class somewhere
        L = max(MM, (9, 22, 43, 60, 77, 94, 111)[i % 7])
        for tries in range(6):
            if add(L, MM, n2_cycle[(i + tries) % 6]):
                break
    return shapes


def pin_cases():
    """Small shapes (n <= 33, m <= 16) with a small covariance, for the mpmath pin of the witness: cond(S) <= 100, so that
    longdouble's own rounding (2^-64 = 5.4e-20, times cond(S)) stays below 1e-17."""
    shapes = [(1, 1, 1), (2, 2, 0), (6, 3, 1), (7, 4, 2), (14, 5, 0), (15, 3, 3), (10, 4, 0), (12, 2, 4)]
    return [sweep_case(L, MM, N2, DIFF if i & 1 else OMNI, 9500 + i, scale=5e-5, name="pin") for i, (L, MM, N2) in enumerate(shapes)]


_sweep = None


def sweep_cases():
    global _sweep
    if _sweep is None:
        _sweep = [sweep_case(L, MM, N2, model, 9000 + i) for i, (L, MM, N2, model) in enumerate(sweep_shapes())]
    return _sweep


# ---- crafted cases: pose (0, 0, 0), nothing moves in Predict (vt = 0), so obs_to_global is exact --------------------------------
def far_lattice(count):
    """Integer lattice points, pitch 2 m, none within 3 m of the origin: float32-exact reflectors that take no part."""
    pts = [(2.0 * ix, 2.0 * iy) for iy in range(-6, 7) for ix in range(-6, 7) if max(abs(ix), abs(iy)) >= 2]
    assert count <= len(pts)
    return pts[:count]


def crafted(name, lms, clouds, expect, model=DIFF, seed=1, scale=1e-3, **kw):
    """lms: list of (x, y); clouds: one cloud per scan (pose at the origin: sensor frame == global frame)."""
    L = len(lms)
    mu = np.zeros(3 + 2 * L)
    mu[3:] = np.asarray(lms, np.float64).reshape(-1)
    P = dense_spd(3 + 2 * L, np.random.default_rng(seed), scale)
    events = [(EV_SCAN, 50.0 + 0.1 * (k + 1), (0.0, 0.0, 0.0), np.asarray(c, np.float32).reshape(-1, 2)) for k, c in enumerate(clouds)]
    return annotate(_case(name, "crafted", model, mu, P, (0.0, 0.0, 0.0), 50.0, events, dict(enumerate(expect)), **kw))


def gate_cases():
    below, at = np.nextafter(np.float32(0.6), np.float32(0)), np.float32(0.6)
    assert float(below) < 0.6 < float(at)
    out = []
    for L in (1, 128):
        lms = far_lattice(L - 1) + [(0.0, 0.0)]                  # the gate reflector is the LAST one
        j = L - 1
        cloud = [(below, 0), (0, at), (-at, 0), (0, -below)]
        # a map of 128 is full: its two observations AT the gate are new, so the capacity guard drops them and raises its flag
        full = L == 128
        out.append(crafted(f"gate_L{L}", lms, [cloud], [([(0, j), (3, j)], [] if full else [1, 2])], seed=20 + L,
                           kept={0: [0, 3]} if full else None, flags=FLAG_CAPACITY if full else 0,
                           gate=[float(below), float(at), float(at), float(below)]))
    return out


def tie_cases():
    out = []

    def tie(name, idx, offs, obs, winner, seed, L=128):
        lms = far_lattice(L)
        for j, o in zip(idx, offs):
            lms[j] = (obs[0] + o[0], obs[1] + o[1])
        exp = ([(0, winner)], []) if winner is not None else ([], [0])
        out.append(crafted(name, lms, [[obs]], [exp], seed=seed, tie=list(idx)))

    g = (0.25, 0.0)
    tie("tie_5_69_same_lane", (5, 69), ((0.375, 0), (-0.375, 0)), g, 5, 31)
    tie("tie_2_65_lower_index_higher_lane", (2, 65), ((0, 0.375), (0.375, 0)), g, 2, 32)
    tie("tie_63_64", (63, 64), ((-0.375, 0), (0, -0.375)), g, 63, 33)
    tie("tie_0_127", (0, 127), ((0.25, 0.25), (-0.25, 0.25)), g, 0, 34)
    tie("tie_three_way_10_74_100", (10, 74, 100), ((0.375, 0), (-0.375, 0), (0, 0.375)), g, 10, 35)
    # both candidates outside the gate: the observation is new, so this map leaves it room (a full one would drop it)
    tie("tie_outside_gate_3_67", (3, 67), ((0.75, 0), (-0.75, 0)), g, None, 36, L=100)
    return out


def map_cases():
    out = []
    new32 = far_lattice(32)
    out.append(crafted("map_L0_K32_all_new", [], [new32], [([], list(range(32)))], seed=41))
    out.append(crafted("map_L1", [(2.0, 1.0)], [[(4.0, -2.0), (2.0 + 1 / 64, 1.0 - 1 / 128), (-3.0, 1.5)]], [([(1, 0)], [0, 2])], seed=42))
    lms = far_lattice(128)
    ids = [4 * i + (i % 3) for i in range(32)]
    cloud = [(lms[j][0] + (i % 5 - 2) / 256, lms[j][1] - (i % 7 - 3) / 256) for i, j in enumerate(ids)]
    out.append(crafted("map_L128_K32_all_matched", lms, [cloud], [([(i, j) for i, j in enumerate(ids)], [])], seed=43))
    return out


def duplicate_cases():
    lms = far_lattice(128)
    ids = [127, 5, 0, 127, 64, 0, 100, 127]
    cloud = [(lms[j][0] + (i - 3) / 128, lms[j][1] + (i % 3 - 1) / 64) for i, j in enumerate(ids)]
    a = crafted("dup_127x3_0x2", lms, [cloud], [([(i, j) for i, j in enumerate(ids)], [])], seed=51)
    lms8 = far_lattice(8)
    cloud = [(lms8[3][0] + (i % 8 - 4) / 512, lms8[3][1] + (i // 8 - 2) / 512) for i in range(32)]
    b = crafted("dup_32_on_one", lms8, [cloud], [([(i, 3) for i in range(32)], [])], seed=52)
    return [a, b]


def heading_cases():
    """theta within 1e-3 of +-pi: odometry carries it across the wrap, the scan's correction carries it back; then time goes
    backwards once (a scan stamped before the state: negative dt, the reference's Q8)."""
    out = []
    for sign in (1.0, -1.0):
        rng = np.random.default_rng(60 + int(sign))
        L = 16
        lms = np.asarray(far_lattice(L), np.float64) + 8.0
        mu = np.zeros(3 + 2 * L)
        mu[0:3] = (8.0, 8.0, sign * (math.pi - 5e-4))
        mu[3:] = lms.reshape(-1)
        A = rng.normal(size=(mu.shape[0], mu.shape[0]))
        P = (A @ A.T) * (1e-5 / mu.shape[0]) + np.diag([1e-3, 1e-3, 1e-2] + [1e-4] * (2 * L))
        P = np.tril(P) + np.tril(P, -1).T
        w = sign * 0.02                                       # 0.1 s of it: 2e-3 rad, across the wrap
        true = (8.0, 8.0, sign * (math.pi - 1.5e-3))          # where the robot really is: back on the first side
        ids = [0, 3, 5, 8, 11, 15]
        cloud = np.array([to_local(true, lms[j]) for j in ids], np.float32)
        events = [(EV_ODOM, 70.0, (0.0, 0.0, w), None), (EV_ODOM, 70.1, (0.0, 0.0, 0.0), None),
                  (EV_SCAN, 70.2, (0.0, 0.0, 0.0), cloud), (EV_SCAN, 70.15, (0.0, 0.0, 0.0), cloud[:4].copy())]
        pairs = [(i, j) for i, j in enumerate(ids)]
        case = _case(f"heading_{'plus' if sign > 0 else 'minus'}_pi", "crafted", DIFF, mu, P, (0.0, 0.0, 0.0), 69.9, events,
                     {2: (pairs, []), 3: (pairs[:4], [])}, heading=sign)
        out.append(annotate(case))
    return out


def capacity_cases():
    """A map of 10 with room for 1 and for 2 of a scan's 5 new observations, matched and new interleaved; then a scan of 3 new and
    8 matched observations on the full member.  `kept` lists, per scan, what the capacity guard lets through."""
    out = []
    for room in (1, 2):
        lms = far_lattice(10)
        extra = far_lattice(40)[20:28]
        kinds1 = ["n", "m", "n", "n", "m", "n", "m", "n", "m"]
        m_ids, cloud1, pairs1, new1 = [2, 7, 0, 9], [], [], []
        for q, kd in enumerate(kinds1):
            if kd == "m":
                j = m_ids[len(pairs1)]
                cloud1.append((lms[j][0] + 1 / 128, lms[j][1] - 1 / 256))
                pairs1.append((q, j))
            else:
                cloud1.append(extra[len(new1)])
                new1.append(q)
        keep1 = sorted([q for q, _ in pairs1] + new1[:room])
        kinds2 = ["m", "n", "m", "m", "n", "m", "m", "m", "n", "m", "m"]
        cloud2, pairs2, new2 = [], [], []
        for q, kd in enumerate(kinds2):
            if kd == "m":
                j = len(pairs2) + 1
                cloud2.append((lms[j][0] - 1 / 256, lms[j][1] + 1 / 128))
                pairs2.append((q, j))
            else:
                cloud2.append(extra[5 + len(new2)])
                new2.append(q)
        keep2 = [q for q, _ in pairs2]
        out.append(crafted(f"capacity_room{room}", lms, [cloud1, cloud2], [(pairs1, new1[:room]), (pairs2, [])], seed=70 + room,
                           max_landmarks=10 + room, kept={0: keep1, 1: keep2}, room=room, flags=FLAG_CAPACITY))
    return out


def singular_case():
    """The covariance is made indefinite in reflector 3's block: the FIRST pivot of S is negative (about -0.8), far
    from zero, so Gauss-Jordan stays finite.  Only the flag is specified."""
    lms = far_lattice(8)
    cloud = [(lms[3][0] + 1 / 64, lms[3][1]), (lms[6][0], lms[6][1] - 1 / 64)]
    c = crafted("singular_block3", lms, [cloud], [([(0, 3), (1, 6)], [])], seed=80, singular=True)
    c.P[9, 9] = c.P[10, 10] = -1.0
    return c


def plain_neighbours():
    lms = far_lattice(12)
    out = []
    for s in (81, 82):
        cloud = [(lms[1][0] + 1 / 64, lms[1][1]), (lms[8][0], lms[8][1] - 1 / 64), (-1.0, 0.5)]
        out.append(crafted(f"neighbour_{s}", lms, [cloud], [([(0, 1), (1, 8)], [2])], seed=s, model=OMNI if s & 1 else DIFF))
    return out


_crafted = None


def crafted_cases():
    """Every crafted case that is compared with the witness (the singular one is not: see singular_case)."""
    global _crafted
    if _crafted is None:
        _crafted = gate_cases() + tie_cases() + map_cases() + duplicate_cases() + heading_cases() + capacity_cases() + plain_neighbours()
    return _crafted
