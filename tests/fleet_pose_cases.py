"""Cases of the fleet filter's pose fixes (the reference's USE_GPS branch, reflector_ekf_slam_gps.cc:305-340), shared by
tests/test_fleet_pose_cpu.py (the cases and the CPU references against each other) and tests/test_fleet_pose_gpu.py
(k_fleet_step against them).  Built on tests/fleet_cases.py: a case is that module's record, every event with its fifth
element ``(kind, t, (vx, vy, wz), cloud or None, fix or None)``; feeding and packing them is that module's ``feed`` / ``fev``.

A fix is the pose of ``predict_state(t)`` of oracle/ekf_numpy.py on the case's own events, plus seeded noise of
(0.05 m, 0.05 m, 0.017 rad): what a scan matcher started from that pose hands back.

Shape cases: one scan with a fix on a dense random SPD covariance (fleet_cases.sweep_case), then the sweep's follow-up scan,
also with a fix: it appends one reflector and matches none, so its fix has to be ignored.  MM runs over the row counts of
the joint system that matter to the kernel -- 0 (no rows), 1 (5), 6 / 7 (15 / 17: either side of a 16-row tile), 30 (63),
31 (65) and 32 (67: more than S in LDS holds; n = 67 is the smallest state in which 32 pairs match) -- each at the smallest
maps with n mod 16 in {3, 15, 1} (n = 3 + 2 L is odd: 15 and 1 are as close to a multiple of 16 as it comes).
"""
from __future__ import annotations

import copy
import math
from types import SimpleNamespace as NS

import numpy as np

from tests import fleet_cases as FC

EV_ODOM, EV_SCAN = FC.EV_ODOM, FC.EV_SCAN
FIX_SIGMA = (0.05, 0.05, 0.017)
SESSION_MARGIN_MIN = 1e-6

# ---- the FP64 noise floor of these cases -------------------------------------------------------------------------------------
# Measured by tests/test_fleet_pose_cpu.py::test_fp64_floor as tests/test_fleet_edges_cpu.py does for the plain update: the
# larger error of oracle/ekf_oracle.c and oracle/ekf_numpy.py against the longdouble witness over every scan of every case
# below.  Recorded = measured, rounded up to two digits; the test fails when a re-measurement exceeds it or falls below half.
FP64_FLOOR_SIGMA = 9.5e-12    # measured 9.498e-12 (pose_L32_MM32_N0_omni_fix scan 1, oracle)
FP64_FLOOR_MU = 3.0e-16       # measured 2.962e-16 (capacity_room1_fix scan 1, numpy)


def pose_witness_of(case, form="joint"):
    from tests.witness.fleet_pose_witness import PoseWitnessEKF
    w = PoseWitnessEKF(case.model, case.t, case.mu[:3], FC.LIN_COV, FC.ANG_COV, FC.OBS_COV, form=form)
    w.set_state(case.t, case.mu, case.P, case.vt)
    return w


SUITE = NS(name="pose", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU,
           witnesses={"witness": pose_witness_of, "two_step": lambda case: pose_witness_of(case, "two_step")})


def attach_fixes(case, seed, which=None, offset=None):
    """Gives the scans of `case` (all, or those with index in `which`) a fix: the numpy filter's predicted pose + seeded noise
    (+ offset), and re-annotates the margins on the run WITH fixes.  Returns the case (a copy; fleet_cases' own stay as they are)."""
    case = copy.copy(case)
    case.events = [tuple(ev[:4]) + (None,) for ev in case.events]
    case.margins, case.cond_S = {}, {}
    rng = np.random.default_rng(seed)
    ek = FC.numpy_of(case)
    for k, ev in enumerate(case.events):
        if ev[0] == EV_ODOM:
            if not case.use_imu:
                ek.handle_odometry(ev[1], *ev[2])
            continue
        cloud = FC.kept_cloud(case, k)
        mu_p, _ = ek.predict_state(ev[1])
        fix = None
        if which is None or k in which:
            fix = mu_p[:3] + rng.normal(size=3) * FIX_SIGMA + (0.0 if offset is None else np.asarray(offset))
            fix[2] = math.atan2(math.sin(fix[2]), math.cos(fix[2]))
            fix = tuple(float(v) for v in fix)
            case.events[k] = tuple(ev[:4]) + (fix,)
        case.margins[k] = FC.margins(mu_p, cloud)
        ek.handle_observation(ev[1], cloud, None if fix is None else np.asarray(fix))
    case.name = case.name + "_fix"
    return case


# ---- shape cases -------------------------------------------------------------------------------------------------------------
# (L, MM, N2): n = 3 + 2 L; n mod 16 = 3 <-> L mod 8 = 0, 15 <-> 6, 1 <-> 7
SHAPES = [(0, 0, 3), (8, 0, 2), (6, 0, 1), (7, 0, 4),
          (8, 1, 0), (6, 1, 1), (7, 1, 2),
          (8, 6, 1), (6, 6, 0), (7, 6, 2), (8, 7, 0), (14, 7, 1), (7, 7, 3),
          (32, 30, 2), (30, 30, 0), (31, 30, 1), (32, 31, 1), (38, 31, 0), (31, 31, 1),
          (32, 32, 0), (38, 32, 0), (39, 32, 0)]

_shape = None


def shape_cases():
    global _shape
    if _shape is None:
        _shape = []
        for i, (L, MM, N2) in enumerate(SHAPES):
            base = FC.sweep_case(L, MM, N2, FC.DIFF if i % 2 == 0 else FC.OMNI, 9700 + i, name="pose")
            _shape.append(attach_fixes(base, 9800 + i))
    return _shape


# ---- crafted cases -----------------------------------------------------------------------------------------------------------
def heading_fix_cases():
    """theta within 1e-3 of +-pi.  Odometry carries the state's heading across the wrap; the fix's yaw is on the FIRST side, so
    z - mu0 is about -+(2 pi - 2e-3) and only the wrapped innovation is small.  Then odometry with a velocity, and a scan with
    a fix stamped BEFORE that odometry message: a Predict with negative dt in front of a fix."""
    out = []
    for sign in (1.0, -1.0):
        rng = np.random.default_rng(160 + int(sign))
        L = 16
        lms = np.asarray(FC.far_lattice(L), np.float64) + 8.0
        mu = np.zeros(3 + 2 * L)
        mu[0:3] = (8.0, 8.0, sign * (math.pi - 5e-4))
        mu[3:] = lms.reshape(-1)
        A = rng.normal(size=(mu.shape[0], mu.shape[0]))
        P = (A @ A.T) * (1e-5 / mu.shape[0]) + np.diag([1e-3, 1e-3, 1e-2] + [1e-4] * (2 * L))
        P = np.tril(P) + np.tril(P, -1).T
        w = sign * 0.02                                       # 0.1 s of it: 2e-3 rad, across the wrap
        true = (8.0, 8.0, sign * (math.pi - 1.5e-3))          # where the robot really is: back on the first side
        ids = [0, 3, 5, 8, 11, 15]
        cloud = np.array([FC.to_local(true, lms[j]) for j in ids], np.float32)
        true2 = (8.004, 8.0, sign * (math.pi - 1.2e-3))
        cloud2 = np.array([FC.to_local(true2, lms[j]) for j in ids[:4]], np.float32)
        fix1 = (true[0] + 0.03, true[1] - 0.02, true[2] + sign * 4e-4)
        fix2 = (true2[0] - 0.01, true2[1] + 0.04, true2[2] - sign * 6e-4)
        events = [(EV_ODOM, 70.0, (0.0, 0.0, w), None, None), (EV_ODOM, 70.1, (0.0, 0.0, 0.0), None, None),
                  (EV_SCAN, 70.2, (0.0, 0.0, 0.0), cloud, fix1), (EV_ODOM, 70.3, (0.2, 0.0, sign * 0.01), None, None),
                  (EV_SCAN, 70.25, (0.0, 0.0, 0.0), cloud2, fix2)]
        pairs = [(i, j) for i, j in enumerate(ids)]
        case = FC._case(f"heading_fix_{'plus' if sign > 0 else 'minus'}_pi", "crafted", FC.DIFF, mu, P, (0.0, 0.0, 0.0), 69.9, events,
                        {2: (pairs, []), 4: (pairs[:4], [])}, heading=sign)
        ek = FC.numpy_of(case)
        for k, ev in enumerate(events):
            if ev[0] == EV_SCAN:
                case.margins[k] = FC.margins(ek.predict_state(ev[1])[0], ev[3])
            FC.feed(ek, ev)
        out.append(case)
    return out


def capacity_fix_cases():
    """fleet_cases.capacity_cases with a fix on both scans: the first appends up to the capacity and drops the rest, the
    second meets the full map."""
    return [attach_fixes(c, 9900 + c.room) for c in FC.capacity_cases()]


_crafted = None


def crafted_cases():
    global _crafted
    if _crafted is None:
        _crafted = heading_fix_cases() + capacity_fix_cases()
    return _crafted


# ---- sessions ------------------------------------------------------------------------------------------------------------------
# (landmarks, observations per scan, model, which scans carry a fix)
SESSIONS = [(24, 8, FC.DIFF, "every"), (32, 12, FC.DIFF, "third"), (24, 8, FC.DIFF, "never"), (32, 8, FC.OMNI, "every")]
SESSION_SCANS = 40
_sessions = None


def sessions():
    """-> list of records (sess, options, events, margins per scan index, oracle final state, per-scan oracle records): the four
    sessions as the C oracle ran them, fixes drawn from its own PredictState."""
    global _sessions
    if _sessions is not None:
        return _sessions
    from reflector_ekf_slam_amd import synth
    from reflector_ekf_slam_amd import session as S
    from tests.helpers import make_oracle, norm_match
    out = []
    for i, (L, K, model, policy) in enumerate(SESSIONS):
        sess = synth.make_session(synth.SessionConfig(f"posefleet{i}", L, K, model, seed=7600 + i), max_scans=SESSION_SCANS)
        cfg = sess.config
        o = make_oracle(cfg.odom_model, sess.init_time, sess.init_pose, cfg.sigma_v ** 2, cfg.sigma_w ** 2, cfg.sigma_obs ** 2)
        rng = np.random.default_rng(7700 + i)
        events, margins, records, scan = [], {}, {}, 0
        for k, ev in enumerate(FC.events_of(sess)):
            if ev[0] == EV_ODOM:
                events.append(tuple(ev) + (None,))
            else:
                mu_p = o.predict_state(ev[1])[0]
                fix = None
                if policy == "every" or (policy == "third" and scan % 3 == 0):
                    fix = mu_p[:3] + rng.normal(size=3) * FIX_SIGMA
                    fix = (float(fix[0]), float(fix[1]), math.atan2(math.sin(fix[2]), math.cos(fix[2])))
                events.append(tuple(ev) + (fix,))
                margins[k] = FC.margins(mu_p, ev[3])
                scan += 1
            FC.feed(o, events[-1])
            if ev[0] == EV_SCAN:
                sp, _, nw = norm_match(o.last_match())
                records[k] = (sp, nw, o.mu())
        mo, Po = o.state()
        out.append(NS(sess=sess, options=S.options_for(sess), events=events, margins=margins, records=records, mu=mo, P=Po,
                      time=o.time, vt=o.vt(), policy=policy, model=model))
        o.close()
    _sessions = out
    return out
