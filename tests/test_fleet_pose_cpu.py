"""The fleet filter's pose fixes, what can be checked without a GPU: the cases of tests/fleet_pose_cases.py against the three CPU
references (oracle/ekf_oracle.c, oracle/ekf_numpy.py, the longdouble witness with pose rows), the exactness of the two-step
form k_fleet_step computes, the FP64 floor that sets the GPU bound, planted defects against that bound, and the C ABI."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_pose_cases as PC
from tests.fleet_harness import HEADER, ROOT, _lib
from tests.witness import fleet_pose_witness as PW

needs_ld = pytest.mark.skipif(not PW.available(), reason="numpy.longdouble has no 64-bit mantissa on this platform")


@pytest.fixture(scope="module")
def all_cases():
    return PC.shape_cases() + PC.crafted_cases()


@pytest.fixture(scope="module")
def reference_runs(all_cases):
    """Per case and scan event: ([joint witness state, two-step witness state], oracle state, numpy state)."""
    return {c.name: H.run_references(c, PC.SUITE) for c in all_cases}


@needs_ld
def test_cases_are_what_they_claim(all_cases, reference_runs):
    assert len(reference_runs) == len(all_cases) == len({c.name for c in all_cases})
    shapes = PC.shape_cases()
    assert {c.MM for c in shapes} == {0, 1, 6, 7, 30, 31, 32}
    for MM in (0, 1, 6, 7, 30, 31, 32):
        assert {c.n % 16 for c in shapes if c.MM == MM} >= ({3, 15, 1} if MM != 32 else {3}), MM
    assert any(c.MM == 32 and c.n == 67 for c in shapes)
    assert {c.model for c in shapes} == {FC.DIFF, FC.OMNI}
    for c in shapes:
        assert len(c.events) == 2 and all(ev[4] is not None for ev in c.events)
        assert len(c.expect[0][0]) == c.MM and len(c.expect[0][1]) == c.N2
        assert c.expect[1][0] == [] and len(c.expect[1][1]) == 1          # the follow-up scan matches nothing: its fix is ignored
        for k in (0, 1):
            assert all(a >= FC.MARGIN_MIN and b >= FC.MARGIN_MIN for a, b in c.margins[k]), (c.name, k)
    for c in PC.heading_fix_cases():
        sg = c.heading
        w = PC.pose_witness_of(c)
        for ev in c.events[:2]:
            FC.feed(w, ev)
        w.predict(c.events[2][1] - w.time)
        th, z = float(w.mu[2]), c.events[2][4][2]
        assert th * sg < 0 and z * sg > 0 and abs(z - th) > 6.0               # state and fix on either side of +-pi
        assert abs(float(PW.yaw_innovation(np.longdouble(z) - w.mu[2]))) < 5e-3
        assert c.events[4][1] < c.events[3][1] and c.events[3][0] == FC.EV_ODOM and c.events[4][4] is not None
    for c in PC.capacity_fix_cases():
        assert c.flags == FC.FLAG_CAPACITY and c.kept and all(ev[4] is not None for ev in c.events)
        assert len(c.expect[0][1]) == c.room and len(c.expect[1][0]) == 8


@needs_ld
def test_two_step_form_equals_the_joint_form(all_cases, reference_runs):
    """The exactness k_fleet_step relies on: the forms differ by longdouble round-off only.  That is 2^-64 = 5.4e-20 times the
    amplification of the solve and of the subtraction P - K W^T, which fleet_cases bounds by cond(S) < 1e5 for these
    covariances: 5.4e-15, taken as 1e-14 -- three orders below the FP64 floor, where an inexact form would show at 1e-3 and more
    (the second step moves the pose by centimetres)."""
    worst = (0.0, "")
    for c in all_cases:
        for k, ((wj, wt), _, _) in reference_runs[c.name].items():
            es, em = H.rel_err(wt[0], wt[1], *wj)
            worst = max(worst, (max(es, em), f"{c.name} scan {k}"))
    print(f"\ntwo-step against joint form over {len(all_cases)} cases: worst relative difference {worst[0]:.2e} at {worst[1]}")
    assert worst[0] < 1e-14


@needs_ld
def test_fp64_floor(all_cases, reference_runs):
    H.measure_floor(all_cases, reference_runs, PC.SUITE)


@needs_ld
@pytest.mark.parametrize("mutation", PW.POSE_MUTATIONS)
def test_the_bound_can_fail(mutation):
    """One planted defect per slip the pose phase invites; each moves the state by at least 1000 x the GPU bound."""
    shapes = PC.shape_cases()
    if mutation == "unwrapped_yaw":
        c, k = PC.heading_fix_cases()[0], 2
    elif mutation == "no_pose_noise":
        c, k = next(c for c in shapes if c.MM == 7), 0
    else:
        c, k = next(c for c in shapes if c.MM == 0 and c.mu.shape[0] > 3), 0
    good, bad = PC.pose_witness_of(c), PC.pose_witness_of(c)
    for ev in c.events[:k]:
        FC.feed(good, ev)
        FC.feed(bad, ev)
    ev = c.events[k]
    good.handle_observation(ev[1], ev[3], ev[4])
    bad.handle_observation(ev[1], ev[3], ev[4], mutate=mutation)
    es, em = H.rel_err(bad.mu, bad.sigma, good.mu, good.sigma)
    bs, bm = FC.gpu_bounds(good.mu, good.sigma, PC.SUITE)
    print(f"\n{mutation} on {c.name}: sigma moves by {es / bs:.3g} x its GPU bound, mu by {em / bm:.3g} x")
    assert max(es / bs, em / bm) >= 1000


def test_sessions_have_association_margins():
    """Every scan of the sessions the GPU test runs has |d1 - 0.6| and d2 - d1 of at least 1e-6 in the oracle, so that the GPU
    test leaves out no scan."""
    ss = PC.sessions()
    assert [s.policy for s in ss] == ["every", "third", "never", "every"] and ss[3].model == FC.OMNI
    worst = np.inf
    for s in ss:
        scans = [k for k, ev in enumerate(s.events) if ev[0] == FC.EV_SCAN]
        fixes = [k for k in scans if s.events[k][4] is not None]
        assert len(scans) >= 30 and sorted(s.margins) == scans
        assert len(fixes) == {"every": len(scans), "third": (len(scans) + 2) // 3, "never": 0}[s.policy]
        assert any(len(s.records[k][0]) > 0 for k in fixes) or s.policy == "never"
        for k in scans:
            for a, b in s.margins[k]:
                worst = min(worst, a, b)
        assert s.mu.shape[0] > 3 + 2 * 8
    print(f"\nsmallest association margin over the four sessions: {worst:.3e}")
    assert worst >= PC.SESSION_MARGIN_MIN


def test_numpy_and_oracle_agree_on_the_sessions():
    from oracle.ekf_numpy import NumpyEKF
    for s in PC.sessions():
        cfg = s.sess.config
        e = NumpyEKF(cfg.odom_model, s.sess.init_time, s.sess.init_pose, cfg.sigma_v ** 2, cfg.sigma_w ** 2, cfg.sigma_obs ** 2)
        for ev in s.events:
            FC.feed(e, ev)
        assert e.mu.shape == s.mu.shape
        assert float(np.abs(e.mu - s.mu).max()) < FC.MU_TOL and float(np.abs(e.sigma - s.P).max()) < FC.SIGMA_TOL


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_predict_poses_and_sizeof_event_are_exported():
    L = _lib()
    assert hasattr(L, "rfleet_predict_poses") and hasattr(L, "rfleet_sizeof_event")
    text = open(HEADER).read()
    assert re.search(r"int\s+rfleet_predict_poses\s*\(", text) and re.search(r"#define\s+RFLEET_ABI_VERSION\s+2\b", text)
    assert L.rfleet_abi_version() == 2


def test_event_layout_is_the_c_structs():
    """ctypes' RfleetEvent against struct rfleet_event as a C compiler lays it out (a probe compiled from include/rfleet.h) and
    against the library's own sizeof."""
    from reflector_ekf_slam_amd import fleet
    E = fleet.RfleetEvent
    assert _lib().rfleet_sizeof_event() == C.sizeof(E)
    names = [f[0] for f in E._fields_]
    assert names == ["member", "kind", "t", "v", "xy", "K", "has_pose_fix", "pose_fix"]
    text = open(HEADER).read()
    body = re.search(r"typedef struct rfleet_event \{(.*?)\} rfleet_event;", text, re.S).group(1)
    declared = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert declared == names, declared
    import shutil
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:                                             # (the library's own sizeof and the field list have been checked)
        return
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as fh:
            fh.write('#include <stddef.h>\n#include <stdio.h>\n#include "rfleet.h"\nint main(void) { printf("%zu", sizeof(rfleet_event));\n'
                     + "".join(f' printf(" %zu", offsetof(rfleet_event, {n}));\n' for n in names) + " return 0; }\n")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(E)] + [getattr(E, n).offset for n in names], got


def test_new_argument_checks_come_before_any_hip_call():
    L = _lib()
    buf = (C.c_double * 16)()
    assert L.rfleet_predict_poses(None, buf, buf, buf) == -1
    assert L.rfleet_predict_poses(None, None, None, None) == -1


def test_pack_takes_five_and_six_tuples():
    from reflector_ekf_slam_amd import fleet
    cloud = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32)
    five = fleet.scan_event(3, 1.5, cloud)
    six = fleet.scan_event(3, 1.5, cloud, pose_fix=(0.25, -0.5, 3.0))
    assert len(five) == 5 and len(six) == 6
    arr, count, keep = fleet.ReflectorEKFSLAMFleet.pack([five, six, fleet.odom_event(1, 1.0, 0.1, 0.0, 0.2), five + (None,)])
    assert count == 4 and len(keep) == 3
    assert [arr[i].has_pose_fix for i in range(4)] == [0, 1, 0, 0]
    assert tuple(arr[1].pose_fix) == (0.25, -0.5, 3.0) and arr[1].K == 2 and arr[0].K == 2 and arr[1].member == 3
    for name in ("predict_poses",):
        assert callable(getattr(fleet.ReflectorEKFSLAMFleet, name))
    assert callable(fleet.FleetMember.PredictState)
