"""Every launch form of the single filter at the shapes and edges where an indexing slip is silent, against the longdouble witness
(tests/witness/fleet_witness.py, tests/witness/fleet_pose_witness.py) on the cases of tests/ekf_shape_cases.py -- random dense
SPD states written with set_state, so that a gathered element of P without its pending rank-m correction, a write-ahead panel taken
when it should not be, or a slip at a 16-row workgroup edge of k_mid, a 64-row tile edge of the downdate or the NBR = 2 | 4
switch moves the result by many orders of magnitude more than the bound (tests/test_ekf_shapes_cpu.py plants each of them).

Each case runs from a fresh handle in six call patterns (one handle alive at a time, REKF_* set before it is created):
    reader                 last_match() and GetState() after every scan; checked after every scan
    reader_grid_off        the same with debug_set_grid(False): the front end as a launch of its own
    node                   pose() after every scan; checked at the end
    pipelined              no read until after the last scan: the speculative one-launch form
    pipelined_spec_off     REKF_SPEC=0
    pipelined_two_launch   REKF_SCAN_LAUNCH=0
Association lists, n, flags and sync_code() must be the witness's / the case's; sigma as returned exactly symmetric;
max|dsigma| / max|sigma_ref| and max|dmu| / max(1, max|mu_ref|) within fleet_cases.GPU_FACTOR (16) x the FP64 floor that
tests/test_ekf_shapes_cpu.py measures (never looser than the 1e-9 / 1e-11 of tests/test_ekf_gpu.py).  The three pipelined forms
end on the same bits, and so do the two readers.  rekf_debug_counters (include/rekf_debug.h) is read once at the end of every
run and must show that the path the pattern is about ran (`_check_counters` says what the host's rules make of each kind).

The cases of the fleet's sweep and its crafted cases (tests/fleet_cases.py; about 100 further shapes, gates to the last float32
ulp, exact ties, duplicates, the heading wrap) run through a single-filter handle in the reader pattern, with their own floors.

run_pattern serves tests/test_ekf_map_gpu.py as well: a case with a map (``map_xy`` / ``map_cov``) has it set on the handle, and all
three lists of last_match() are compared with the case's claim (no map pair for a case without a map).

Out of scope, as in tests/ekf_shape_cases.py: exclusive handles."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import ekf_shape_cases as EC
from tests import fleet_cases as FC
from tests.fleet_harness import bounds_within_tolerances, rel_err
from tests.helpers import norm_match
from tests.witness import fleet_witness as FW

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not FW.available(), reason="numpy.longdouble has no 64-bit mantissa here")]

PATTERNS = {"reader": dict(read="reader"), "reader_grid_off": dict(read="reader", grid=False), "node": dict(read="node"),
            "pipelined": dict(read=None), "pipelined_spec_off": dict(read=None, spec=False),
            "pipelined_two_launch": dict(read=None, scan_launch=False)}
WORST = {}                                                      # suite name -> worst (sigma, mu) over the module, as multiples of the suite's floor
_witness = {}


def witness_run(case, suite):
    """-> per scan event k the witness's (mu, P) after it: computed once per case, shared by its patterns, never changed."""
    key = (suite.name, case.name)                               # (two case modules may use one name: fleet_cases' and fleet_map_cases' ties)
    if key not in _witness:
        w = next(iter(suite.witnesses.values()))(case)
        out = {}
        k_of = [k for k, ev in enumerate(case.events) if not (ev[0] == FC.EV_ODOM and case.use_imu)]
        for k, ev in zip(k_of, FC.reference_events(case)):
            FC.feed(w, ev)
            if ev[0] == FC.EV_SCAN:
                got = w.last_match if len(w.last_match) == 3 else (w.last_match[0], [], w.last_match[1])
                pairs, new = FC.map_back(case, k, got[0], got[2])
                mapped, _ = FC.map_back(case, k, got[1], [])
                want_p, want_m, want_n = EC.claim3(case, k)
                assert np.array_equal(pairs, np.asarray(want_p, np.int32).reshape(-1, 2)), (case.name, k)
                assert np.array_equal(mapped, np.asarray(want_m, np.int32).reshape(-1, 2)), (case.name, k)
                assert np.array_equal(new, np.asarray(want_n, np.int32).reshape(-1)), (case.name, k)
                out[k] = w.state()
        _witness[key] = out
    return _witness[key]


def _counters(g):
    out = (C.c_longlong * 32)()
    assert g._L.rekf_debug_counters(g._h, out) == 0
    return list(out)


def _check_match(g, case, k, what):
    sp, mp, nw = norm_match(g.last_match())
    want_p, want_m, want_n = EC.claim3(case, k)
    assert np.array_equal(mp, np.asarray(want_m, np.int32).reshape(-1, 2)), (what, k, mp.tolist(), want_m)
    assert np.array_equal(sp, np.asarray(want_p, np.int32).reshape(-1, 2)), (what, k, sp.tolist(), want_p)
    assert np.array_equal(nw, np.asarray(want_n, np.int32).reshape(-1)), (what, k, nw.tolist(), want_n)


def _check_state(st, ref, suite, what):
    """The state as returned against the witness's.  -> (sigma error, mu error) as multiples of the suite's floor."""
    mu_ref, P_ref = ref
    assert st.mu.shape[0] == mu_ref.shape[0], (what, st.mu.shape, mu_ref.shape)
    assert np.array_equal(st.sigma, st.sigma.T), (what, "sigma is not exactly symmetric as returned")
    es, em = rel_err(st.mu, st.sigma, mu_ref, P_ref)
    bs, bm = bounds_within_tolerances(mu_ref, P_ref, suite)
    fs, fm = es / suite.floor_sigma, em / suite.floor_mu
    if es > bs or em > bm:
        d = np.abs(np.asarray(st.sigma, np.longdouble) - P_ref)
        r, c = np.unravel_index(int(np.argmax(d)), d.shape)
        dm = int(np.argmax(np.abs(np.asarray(st.mu, np.longdouble) - mu_ref)))
        print(f"  {what}: worst sigma element ({r}, {c}), rows off by more than the bound: "
              f"{np.nonzero(d.max(axis=1) > bs * float(np.abs(P_ref).max()))[0].tolist()[:40]}; worst mu row {dm}")
    assert es <= bs, f"{what}: sigma off by {es:.3e} = {fs:.1f} x the FP64 floor (bound {bs:.3e})"
    assert em <= bm, f"{what}: mu off by {em:.3e} = {fm:.1f} x the FP64 floor (bound {bm:.3e})"
    ws, wm = WORST.get(suite.name, ((0.0, ""), (0.0, "")))          # (of the states that hold the bound: a miss is its own test's failure)
    WORST[suite.name] = (max(ws, (fs, what)), max(wm, (fm, what)))
    return fs, fm


def run_pattern(case, pattern, monkeypatch, suite):
    """One case through one call pattern on a fresh handle.  -> the final state's bits and the path counters."""
    from reflector_ekf_slam_amd import ReflectorEKFSLAM
    kw = PATTERNS[pattern]
    monkeypatch.setenv("REKF_SPEC", "1" if kw.get("spec", True) else "0")
    monkeypatch.setenv("REKF_SCAN_LAUNCH", "1" if kw.get("scan_launch", True) else "0")
    monkeypatch.delenv("REKF_EXCLUSIVE", raising=False)
    refs = witness_run(case, suite)
    cap = getattr(case, "cap", case.max_landmarks)
    g = ReflectorEKFSLAM(FC.options_of(case), max_landmarks=cap, auto_grow=bool(getattr(case, "auto_grow", False)))
    try:
        if getattr(case, "map_xy", None) is not None and getattr(case, "use", True):
            g.set_map(case.map_xy, case.map_cov)
        g.set_state(case.t, case.mu, case.P, case.vt)
        if kw.get("grid", True) is False:
            g.debug_set_grid(False)
        last = None
        for k, ev in enumerate(case.events):
            FC.feed(g, ev)
            if ev[0] != FC.EV_SCAN:
                continue
            last = k
            what = f"{case.name} scan {k} {pattern}"
            if kw["read"] == "reader":
                _check_match(g, case, k, what)
                _check_state(g.GetState(), refs[k], suite, what)
            elif kw["read"] == "node":
                t, p, P3 = g.pose()
                assert t == ev[1] and np.isfinite(p).all() and np.isfinite(P3).all(), what
        cnt = _counters(g)
        what = f"{case.name} scan {last} {pattern}"
        _check_match(g, case, last, what)
        assert g.flags() == getattr(case, "flags", 0), (what, g.flags())
        # (rekf_sync reports a sticky flag once, as its error code: REKF_ERR_CAPACITY where the case expects the capacity flag)
        assert g.sync_code() == (-4 if getattr(case, "flags", 0) & FC.FLAG_CAPACITY else 0), what
        st = g.GetState()
        assert g.n == refs[last][0].shape[0], (what, g.n)
        _check_state(st, refs[last], suite, what)
        return NS(mu=st.mu, sigma=st.sigma, cnt=cnt, cap=g.max_landmarks)
    finally:
        g.close()


def _same_bits(a, b):
    return a.mu.shape == b.mu.shape and np.array_equal(a.mu, b.mu) and np.array_equal(a.sigma, b.sigma)


def _check_counters(case, runs):
    """What rekf_debug_counters must show after each pattern.  [18] scans k_mid matched itself through the match grid; [20] scans
    whose speculative match record was taken; [22] scans that met a pending downdate, [23] of those, the ones that computed its
    correction themselves (no write-ahead panel); [24] > 0: the one-launch form ran."""
    c = {p: r.cnt for p, r in runs.items()}
    line = "; ".join(f"{p} " + " ".join(f"[{i}] {c[p][i]}" for i in (18, 20, 21, 22, 23, 24)) for p in runs)
    print(f"  {case.name}: {line}")
    # a scan of more than 64 innovation rows runs as block steps: matched by k_compact_wide (no match grid, no speculation, no
    # write-ahead panel), through the two-launch chain
    blocks = [2 * len(ev[3]) + (3 if len(ev) > 4 and ev[4] is not None else 0) > 64 for ev in case.events]
    staged = [len(ev[3]) > 64 for ev in case.events]
    p4, p5, p6 = c["pipelined"], c["pipelined_spec_off"], c["pipelined_two_launch"]
    if all(blocks):
        # (the pose case of 65 rows: every scan in block steps)
        assert p4[24] == 0 and p4[22] == 0 and p4[20] == 0 and p5[24] == 0, line
    elif case.kind == "wide":
        # scan 1 in block steps, scan 2 a whole scan: it takes scan 1's last downdate along as a role of its own launch (there is no
        # panel of a wide scan: a miss) -- unless scan 1 was staged through HBM, whose downdate is not held back
        if staged[0]:
            assert p4[24] == 0 and p4[22] == 0 and p5[24] == 0, line
        else:
            assert p4[24] > 0 and p4[22] == 1 and p4[23] == 1 and p5[24] > 0 and p5[22] == 1, line
        assert p4[20] == 0, line                               # (two scans: nothing to speculate for)
    else:
        # Scans 2, 3 and 4 meet a pending downdate -- on a filter that is full, or one that can grow but whose scan 1 appended nothing
        # (the early n says so in time).  Where scan 1 appended reflectors, its k_augment is pending with its downdate and scan 2 goes
        # through the two-launch chain (k_dd_front, k_augment, k_mid): scans 3 and 4 are left.
        met = 3 if case.N2 == 0 else 2
        # A panel is taken for the SAME set of reflectors: by scan 2 on a full filter (a filter that can grow runs scan 1 as
        # k_mid<NBR, 1>, which leaves no panel: a miss) and by scan 4 where its three observations are all of scan 3's set (MM = 1).
        hits = (1 if case.cap == case.L else 0) + (1 if case.MM == 1 else 0)
        for p in (p4, p5):
            assert p[24] > 0 and p[22] == met and p[23] == met - hits and p[23] >= 1, line
        assert p4[20] >= 1, line
        if case.cap == case.L:
            assert p4[22] >= 3 and p4[22] - p4[23] >= 1, line      # (a four-scan full-filter case: the hit at scan 2)
    assert p5[20] == 0 and p6[24] == 0 and p6[20] == 0 and p6[22] == 0, line
    # the match grid serves host-predicted whole scans: behind set_state (scan 1 of every pattern) and behind a read of the state or
    # the pose -- but not the scan whose front end rides in k_dd_front (the node's scan 2 behind an appending scan 1)
    whole = sum(1 for b in blocks if not b)
    assert c["reader"][18] == whole and c["node"][18] == whole - (1 if case.N2 else 0) and c["reader_grid_off"][18] == 0, line
    assert p4[18] == p5[18] == p6[18] == (0 if blocks[0] else 1), line


def _run_case(case, monkeypatch):
    runs = {p: run_pattern(case, p, monkeypatch, EC.SUITE) for p in PATTERNS}
    assert _same_bits(runs["pipelined"], runs["pipelined_spec_off"]), f"{case.name}: REKF_SPEC=0 ends on other bits than the pipelined run"
    assert _same_bits(runs["pipelined"], runs["pipelined_two_launch"]), f"{case.name}: REKF_SCAN_LAUNCH=0 ends on other bits than the pipelined run"
    assert _same_bits(runs["reader"], runs["reader_grid_off"]), f"{case.name}: the reader without the match grid ends on other bits"
    _check_counters(case, runs)
    return runs


def _ids(kind):
    return [c.name for c in EC.cases() if c.kind == kind]


@pytest.mark.parametrize("name", _ids("sweep"))
def test_full_filter_sweep(name, monkeypatch):
    """The one-launch pipeline on a full filter: nothing pending, a write-ahead panel hit, two misses, duplicate row pairs."""
    _run_case(EC.case_named(name), monkeypatch)


@pytest.mark.parametrize("name", _ids("capacity"))
def test_full_filter_drops_far_observations(name, monkeypatch):
    """K observations of which MM match: the host sizes the launch by K, the update has 2 MM rows; the sticky capacity flag."""
    _run_case(EC.case_named(name), monkeypatch)


@pytest.mark.parametrize("name", _ids("growing"))
def test_growing_filter(name, monkeypatch):
    """k_mid<*, 1>, k_augment and the early n; new rows up to, across and beyond the 16-row (and 64-row) edge."""
    c = EC.case_named(name)
    runs = _run_case(c, monkeypatch)
    for p, r in runs.items():
        assert r.cap == (2 * c.cap if c.auto_grow else c.cap), (name, p, r.cap)


@pytest.mark.parametrize("name", _ids("wide"))
def test_wide_scans_in_block_steps(name, monkeypatch):
    _run_case(EC.case_named(name), monkeypatch)


@pytest.mark.parametrize("name", _ids("pose"))
def test_pose_fix_rows_jointly(name, monkeypatch):
    """31 | 33 rows (the NBR switch), 63 rows in one pass, 65 rows in block steps of 30 pairs."""
    _run_case(EC.case_named(name), monkeypatch)


FLEET_CHUNKS = 4


@pytest.mark.parametrize("chunk", range(FLEET_CHUNKS))
def test_fleet_sweep_cases_through_a_single_filter(chunk, monkeypatch):
    cases = FC.sweep_cases()[chunk::FLEET_CHUNKS]
    assert len(cases) >= 25
    for c in cases:
        run_pattern(c, "reader", monkeypatch, FC.SUITE)


def test_fleet_crafted_cases_through_a_single_filter(monkeypatch):
    cases = [c for c in FC.crafted_cases() if c.max_landmarks == 128]
    assert len(cases) >= 17
    for c in cases:
        run_pattern(c, "reader", monkeypatch, FC.SUITE)


def test_worst_multiples_of_the_floor():
    """Reports what the tests above measured (run the module with -s); the figures are in DESIGN.md section 6."""
    for suite, (ws, wm) in WORST.items():
        print(f"\n{suite} cases: worst sigma error {ws[0]:.2f} x the FP64 floor ({ws[1]}), worst mu error {wm[0]:.2f} x ({wm[1]}); "
              f"the bound is {FC.GPU_FACTOR:.0f} x")
        assert ws[0] <= FC.GPU_FACTOR and wm[0] <= FC.GPU_FACTOR
