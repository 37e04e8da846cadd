"""What the fleet filter's test suites share: the error formula, the gate on the GPU results (check_member, run_lockstep), the
gate on the CPU references (run_references, measure_floor) and the library handles.

A suite is the record ``SUITE`` of its case module (tests/fleet_cases.py: the plain update; tests/fleet_pose_cases.py: pose
fixes): ``name``, the measured FP64 floors ``floor_sigma`` / ``floor_mu`` and ``witnesses`` (name -> factory taking a case; the
first is the one the GPU is held to).  A fleet feature's tests are its cases, its witness rows, its SUITE and its tests."""
from __future__ import annotations

import os

import numpy as np

from tests import fleet_cases as FC
from tests.helpers import norm_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rfleet.h")


def fleet_mod():
    from reflector_ekf_slam_amd import fleet
    return fleet


def _lib():
    return fleet_mod().rfleet()


def rel_err(mu, P, mu_ref, P_ref):
    """(max|dsigma| / max|sigma_ref|, max|dmu| / max(1, max|mu_ref|)) against a longdouble witness's state."""
    es = float(np.abs(np.asarray(P, np.longdouble) - P_ref).max() / np.abs(P_ref).max())
    em = float(np.abs(np.asarray(mu, np.longdouble) - mu_ref).max() / max(1.0, float(np.abs(mu_ref).max())))
    return es, em


def bounds_within_tolerances(mu_ref, P_ref, suite):
    """-> fleet_cases.gpu_bounds, after asserting that they are never looser than the absolute tolerances of tests/test_fleet_gpu.py."""
    bs, bm = FC.gpu_bounds(mu_ref, P_ref, suite)
    assert bs * float(np.abs(P_ref).max()) <= FC.SIGMA_TOL * (1 + 1e-12) and bs <= FC.GPU_FACTOR * suite.floor_sigma
    assert bm * max(1.0, float(np.abs(mu_ref).max())) <= FC.MU_TOL * (1 + 1e-12) and bm <= FC.GPU_FACTOR * suite.floor_mu
    return bs, bm


# ---- the GPU side -----------------------------------------------------------------------------------------------------------
def make_fleet(cases, max_landmarks=128):
    fl = fleet_mod().ReflectorEKFSLAMFleet([FC.options_of(c) for c in cases], max_landmarks=max_landmarks)
    for i, c in enumerate(cases):
        fl.set_state(i, c.t, c.mu, c.P, c.vt)
    return fl


def check_member(fl, i, case, k, wit, suite):
    """Member i after scan event k of its case against the witness `wit` (already fed the same events).  -> (sigma error,
    mu error) as multiples of the suite's FP64 floor."""
    sp, mp, nw = norm_match(fl.last_match(i))
    want_p, want_n = case.expect[k]
    assert mp.shape[0] == 0
    assert np.array_equal(sp, np.asarray(want_p, np.int32).reshape(-1, 2)), (case.name, k, sp.tolist(), want_p)
    assert np.array_equal(nw, np.asarray(want_n, np.int32).reshape(-1)), (case.name, k, nw.tolist(), want_n)
    mu_ref, P_ref = wit.state()
    st = fl.get_state(i)
    assert st.mu.shape[0] == mu_ref.shape[0] == int(fl.n()[i]), (case.name, k, st.mu.shape, mu_ref.shape)
    assert int(fl.flags()[i]) == getattr(case, "flags", 0), (case.name, k, int(fl.flags()[i]))
    assert np.array_equal(st.sigma, st.sigma.T), (case.name, k, "sigma is not exactly symmetric as returned")
    es, em = rel_err(st.mu, st.sigma, mu_ref, P_ref)
    bs, bm = bounds_within_tolerances(mu_ref, P_ref, suite)
    print(f"  {case.name} scan {k}: sigma {es / suite.floor_sigma:.2f} x the floor, mu {em / suite.floor_mu:.2f} x")
    assert es <= bs, f"{case.name} scan {k}: sigma off by {es:.3e} = {es / suite.floor_sigma:.1f} x the FP64 floor (bound {bs:.3e})"
    assert em <= bm, f"{case.name} scan {k}: mu off by {em:.3e} = {em / suite.floor_mu:.1f} x the FP64 floor (bound {bm:.3e})"
    return es / suite.floor_sigma, em / suite.floor_mu


def run_lockstep(cases, suite, max_landmarks=128):
    """All cases as members of ONE fleet; tick k submits event k of every member in one call; every scan is checked.
    -> the worst (sigma error, where), (mu error, where), as multiples of the floor."""
    fl = make_fleet(cases, max_landmarks)
    witness_of = next(iter(suite.witnesses.values()))
    wits = [witness_of(c) for c in cases]
    refs = [FC.reference_events(c) for c in cases]
    worst_s, worst_m = (0.0, ""), (0.0, "")
    try:
        for k in range(max(len(c.events) for c in cases)):
            fl.submit([FC.fev(i, c.events[k]) for i, c in enumerate(cases) if k < len(c.events)])
            for i, c in enumerate(cases):
                if k >= len(c.events):
                    continue
                FC.feed(wits[i], refs[i][k])
                if c.events[k][0] == FC.EV_SCAN:
                    fs, fm = check_member(fl, i, c, k, wits[i], suite)
                    worst_s, worst_m = max(worst_s, (fs, f"{c.name} scan {k}")), max(worst_m, (fm, f"{c.name} scan {k}"))
    finally:
        fl.close()
    return worst_s, worst_m


# ---- the CPU side -----------------------------------------------------------------------------------------------------------
def run_references(case, suite):
    """Feeds the case's reference events to oracle/ekf_oracle.c, oracle/ekf_numpy.py and the suite's witnesses; -> per scan
    event k: ([witness states, in the suite's order], oracle state, numpy state).  Checks the association lists of all of them
    against the case's claim."""
    o, e = FC.oracle_of(case), FC.numpy_of(case)
    wits = {who: make(case) for who, make in suite.witnesses.items()}
    out = {}
    k_of = [k for k, ev in enumerate(case.events) if not (ev[0] == FC.EV_ODOM and case.use_imu)]
    for k, ev in zip(k_of, FC.reference_events(case)):
        for f in (o, e, *wits.values()):
            FC.feed(f, ev)
        if ev[0] != FC.EV_SCAN:
            continue
        want_p, want_n = case.expect[k]
        want_p, want_n = np.asarray(want_p, np.int32).reshape(-1, 2), np.asarray(want_n, np.int32).reshape(-1)
        so, _, no = norm_match(o.last_match())
        lists = {"oracle": FC.map_back(case, k, so, no), "numpy": FC.map_back(case, k, e.last_match[1], e.last_match[2])}
        lists.update((who, FC.map_back(case, k, *w.last_match)) for who, w in wits.items())
        for who, (p, nw) in lists.items():
            assert np.array_equal(p, want_p) and np.array_equal(nw, want_n), (case.name, k, who, p.tolist(), nw.tolist())
        # the references know no capacity: a claimed "new" must fit the member's map, a dropped one must meet a full map
        states = [w.state() for w in wits.values()]
        L_after = (states[0][0].shape[0] - 3) // 2
        assert L_after <= case.max_landmarks, (case.name, k, L_after, case.max_landmarks)
        if k in case.kept:
            assert L_after == case.max_landmarks and len(case.kept[k]) < len(case.events[k][3]) and case.flags == FC.FLAG_CAPACITY
        out[k] = (states, o.state(), (e.mu.copy(), e.sigma.copy()))
    o.close()
    return out


def measure_floor(cases, runs, suite):
    """The larger error of the two FP64 references against the suite's first witness over every scan of `runs` (name ->
    run_references' result) must be the suite's recorded floor: not above it, not below half of it; and the GPU bound it sets is
    nowhere looser than the absolute tolerances."""
    ws, wm = (0.0, ""), (0.0, "")
    for c in cases:
        for k, (wits, orc, npy) in runs[c.name].items():
            for who, (mu, P) in (("oracle", orc), ("numpy", npy)):
                es, em = rel_err(mu, P, *wits[0])
                ws, wm = max(ws, (es, f"{c.name} scan {k} ({who})")), max(wm, (em, f"{c.name} scan {k} ({who})"))
            bounds_within_tolerances(*wits[0], suite)
    print(f"\nFP64 floor over {len(cases)} {suite.name} cases: sigma {ws[0]:.3e} at {ws[1]}; mu {wm[0]:.3e} at {wm[1]}")
    print(f"recorded: sigma {suite.floor_sigma:.3e}, mu {suite.floor_mu:.3e}")
    assert ws[0] <= suite.floor_sigma and wm[0] <= suite.floor_mu
    assert ws[0] >= suite.floor_sigma / 2 and wm[0] >= suite.floor_mu / 2, "the recorded floor is stale: far above what is measured"
