"""The single filter's map cases (tests/ekf_map_cases.py) against the three CPU references (oracle/ekf_oracle.c,
oracle/ekf_numpy.py and the longdouble witness with the map branch), so that tests/test_ekf_map_gpu.py is about the kernels only:
the cases are what the module says, the references agree on every list of every scan, the FP64 noise floor that sets the GPU
bound is measured here, and the bound is shown to fail on the planted defects of tests/witness/fleet_map_witness.py."""
from __future__ import annotations

import collections

import numpy as np
import pytest

from tests import ekf_map_cases as XC
from tests import ekf_shape_cases as EC
from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as MC
from tests.witness import fleet_map_witness as MW

pytestmark = pytest.mark.skipif(not MW.available(), reason="numpy.longdouble has no 64-bit mantissa on this platform")


@pytest.fixture(scope="module")
def all_cases():
    return XC.cases()


@pytest.fixture(scope="module")
def reference_runs(all_cases, oracle_lib):
    """Every case through oracle, numpy and witness (fleet_map_cases.run_references asserts that all three give the three claimed
    lists on every scan)."""
    return {c.name: MC.run_references(c, XC.SUITE) for c in all_cases}


def test_references_agree_on_every_list(all_cases, reference_runs):
    assert len(reference_runs) == len(all_cases) == len({c.name for c in all_cases})
    for c in all_cases:
        assert sorted(reference_runs[c.name]) == list(range(len(c.events))), c.name
        n_end = reference_runs[c.name][len(c.events) - 1][0][0][0].shape[0]
        assert n_end == 3 + 2 * (c.L + c.N2), (c.name, n_end)


def test_the_case_list(all_cases):
    by_kind = collections.defaultdict(list)
    for c in all_cases:
        by_kind[c.kind].append(c)
    assert set(by_kind) == {"mix", "pure", "growing", "wide", "pose", "weights"}
    assert max(c.L + c.N2 for c in all_cases) <= 200
    shape = lambda c: (c.L, c.MM, c.Mm)                                  # noqa: E731
    rows = lambda c: [XC.rows_of(c, k) for k in range(len(c.events))]      # noqa: E731
    steps = lambda c: [XC.block_steps(c, k) for k in range(len(c.events))]    # noqa: E731
    mix = by_kind["mix"]
    assert [shape(c) for c in mix] == XC.MIX_SHAPES == [(33, 31, 1), (33, 1, 31), (33, 16, 16), (33, 15, 1), (33, 16, 1), (30, 7, 8),
                                                        (31, 8, 8), (64, 0, 17), (127, 24, 8), (127, 0, 32), (200, 16, 16)]
    assert all(c.cap == c.L and len(c.events) == 4 and all(s is None for s in steps(c)) for c in mix)
    for c in mix:
        assert [(len(c.expect[k][0]), len(c.expect[k][1])) for k in range(3)] == [(c.MM, c.Mm)] * 3 and rows(c)[:3] == [2 * c.K] * 3, c.name
    by = {c.name: c for c in all_cases}
    assert rows(by["map_mix_L33_S15_M1_omni"]) == [32] * 4 and rows(by["map_mix_L33_S16_M1_diff"]) == [34] * 4       # the NBR switch
    assert by["map_mix_L30_S7_M8_omni"].n == 63 and by["map_mix_L31_S8_M8_diff"].n == 65
    assert {c.n % 16 for c in mix} == {5, 15, 1, 3} and {c.n % 64 for c in mix} >= {63, 1, 5}
    # pure: n = 3 on a handle of capacity 8
    pure = by_kind["pure"]
    assert [c.Mm for c in pure[:4]] == [1, 16, 17, 32] and all(c.L == 0 and c.n == 3 and c.cap == 8 and c.mu.shape[0] == 3 for c in pure)
    assert [rows(c)[0] for c in pure[:4]] == [2, 32, 34, 64]
    c = pure[4]
    assert [tuple(len(v) for v in c.expect[k]) for k in range(2)] == [(0, 3, 3), (3, 2, 0)] and c.N2 == 3
    assert sorted(g for _, g in c.expect[1][0]) == [0, 1, 2]
    # growing: cap = L + 8, scan 1 = NS + Mm + N2 new, n = 15 mod 16
    grow = by_kind["growing"]
    assert [(c.L, c.MM, c.Mm, c.N2) for c in grow] == [(14, 4, 4, 3), (30, 8, 8, 1), (62, 12, 12, 3)]
    for c in grow:
        assert c.cap == c.L + 8 and not c.auto_grow and c.n % 16 == 15 and tuple(len(v) for v in c.expect[0]) == (c.MM, c.Mm, c.N2)
        assert all(len(c.expect[k][2]) == 0 for k in (1, 2, 3)) and c.L + c.N2 - 1 in [g for _, g in c.expect[2][0]], c.name
    assert [c.n2_class for c in grow] == ["cross", "straddle", "cross"]
    # wide: which block step holds what (state pairs, map pairs)
    wide = by_kind["wide"]
    assert all(c.L == 128 and c.cap == 128 and c.n == 259 and len(c.events) == 2 for c in wide)
    assert [len(c.events[0][3]) for c in wide] == [33, 40, 64, 65]
    assert [steps(c)[0] for c in wide] == [[(32, 0), (0, 1)], [(20, 12), (0, 8)], [(0, 32), (0, 32)], [(32, 0), (1, 31), (0, 1)]]
    assert all(steps(c)[1] is None and tuple(len(v) for v in c.expect[1]) == (1, 1, 0) for c in wide)
    assert [len(c.events[0][3]) > 64 for c in wide] == [False, False, False, True]          # staged through HBM
    # pose: a fix on every scan
    pose = by_kind["pose"]
    assert [shape(c) for c in pose] == [(33, 7, 7), (33, 7, 8), (64, 15, 15), (64, 1, 30)]
    assert all(len(ev) == 5 and ev[4] is not None for c in pose for ev in c.events)
    assert [rows(c)[0] for c in pose] == [31, 33, 63, 65] and all(s is None for c in pose[:3] for s in steps(c))
    assert steps(pose[3]) == [[(1, 29), (0, 1)]] * 3 + [[(3, 27), (0, 1)]]                  # every scan in steps of 30 pairs
    assert all(len(ev) == 4 for c in all_cases if c.kind != "pose" for ev in c.events)
    # weights
    wts = by_kind["weights"]
    assert [shape(c) for c in wts] == [(64, 8, 8)] * 2 and [c.non_symmetric for c in wts] == [False, True]
    for c in wts:
        S = c.map_cov.reshape(-1, 2, 2)
        sym = [j for j in range(S.shape[0]) if S[j, 0, 1] == S[j, 1, 0]]
        ev = np.array([np.linalg.eigvalsh(S[j]) for j in sym])
        assert ev.min() >= 0.25 * (1 - 1e-12) and ev.max() <= 4.0 * (1 + 1e-12) and ev.max() == 4.0, c.name
        assert max(MC.weight_scale(s) for s in c.map_cov[sym]) == 2.0
        assert len(sym) == S.shape[0] - (1 if c.non_symmetric else 0) and np.abs(S[:, 0, 1]).max() > 0.1
    c = wts[1]
    assert c.map_cov[c.Mm].tolist() == list(XC.NON_SYMMETRIC) and [g for _, g in c.expect[3][1]].count(c.Mm) == 3
    assert all((c.map_cov == np.asarray(MC.IDENTITY)).all() for c in all_cases if c.kind != "weights")
    print(f"\n{len(all_cases)} cases:", {k: len(v) for k, v in by_kind.items()})


def test_cases_are_what_they_claim(all_cases):
    worst = np.inf
    for c in all_cases:
        assert c.n == 3 + 2 * c.L == c.mu.shape[0] and c.use and c.flags == 0 and not c.kept, c.name
        assert c.vt[0] != 0 and c.vt[2] != 0 and [ev[1] for ev in c.events] == [EC.T0 + EC.DT * (k + 1) for k in range(len(c.events))]
        assert np.array_equal(c.P, c.P.T) and c.map_xy.dtype == np.float32
        # the geometry: map points, reflectors and new points are different lattice cells
        news = []
        for k, ev in enumerate(c.events):
            w = MC.map_witness_of(c)
            for ev2 in c.events[:k]:
                FC.feed(w, ev2)
            w.predict(ev[1] - w.time)                              # (the pose the scan is matched at)
            sp, mp, nw = c.expect[k]
            assert sorted([q for q, _ in sp] + [q for q, _ in mp] + list(nw)) == list(range(len(ev[3]))), (c.name, k)
            glob = np.array([w.to_global(p) for p in ev[3]], np.float64).reshape(-1, 2)
            for q, j in mp:                                        # within 2 mm (per axis) of its map point, up to float32 rounding
                assert np.abs(glob[q] - c.map_xy[j]).max() <= 2e-3 + 1e-5, (c.name, k, q)
            news += [glob[q] for q in nw]
        w = MC.map_witness_of(c)
        for ev in c.events:
            FC.feed(w, ev)
        lm = w.mu[3:].astype(np.float64).reshape(-1, 2)            # every reflector the case ever has
        for pts in (lm, np.array(news).reshape(-1, 2)):
            if pts.shape[0]:
                d = np.hypot(c.map_xy[:, None, 0] - pts[None, :, 0], c.map_xy[:, None, 1] - pts[None, :, 1])
                assert d.min() >= 1.6 - 0.02, (c.name, d.min())     # (1.6 m between lattice cells; reflector means move by millimetres)
        dm = np.hypot(c.map_xy[:, None, 0] - c.map_xy[None, :, 0], c.map_xy[:, None, 1] - c.map_xy[None, :, 1]) + 10 * np.eye(c.map_xy.shape[0])
        assert dm.min() >= 1.6 - 1e-5, c.name
        # the margins recorded at generation: both of the state branch and both of the map branch, for every observation
        for k in range(len(c.events)):
            assert len(c.margins[k]) == len(c.map_margins[k]) == len(c.events[k][3])
            mapped = {q for q, _ in c.expect[k][1]}
            for q, ((sa, sb), (a, b, inside)) in enumerate(zip(c.margins[k], c.map_margins[k])):
                assert min(sa, sb, a, b) >= FC.MARGIN_MIN and inside == (q in mapped), (c.name, k, q)
                worst = min(worst, sa, sb, a, b)
        if c.kind == "wide" or c.name == "map_pure_mapping_diff":
            continue
        # the four scans
        assert len(c.events) == 4
        st = [[g for _, g in c.expect[k][0]] for k in range(4)]
        mp = [[g for _, g in c.expect[k][1]] for k in range(4)]
        assert sorted(mp[0]) == sorted(mp[1]) == list(range(c.Mm)) and (c.Mm < 2 or mp[0] != mp[1]), c.name
        assert set(st[0]) == set(st[1]) and len(st[1]) == c.MM and (c.MM < 2 or st[0] != st[1]), c.name
        assert sorted(mp[2]) == list(range(c.Mm, 2 * c.Mm)) and len(set(st[2])) == c.MM and (c.MM == 0 or set(st[2]) != set(st[0])), c.name
        assert set(mp[3]) <= set(mp[2]) and mp[3].count(c.Mm) == 3 and len(set(mp[3])) == len(mp[3]) - 2, c.name
        if c.MM:
            tri = EC.triple_of(c.L)
            assert set(st[3]) <= set(st[2]) and st[3].count(tri) == 3 and (3 + 2 * tri) % 16 == 15, c.name
            want = EC.musts(c.L)
            both = set(st[0]) | set(st[2])
            assert len(both & set(want)) >= min(len(want), c.MM) and (c.MM < len(want) or set(want) <= both), (c.name, want, st)
        assert XC.rows_of(c, 3) <= XC.rows_of(c, 0) or c.K < 6, c.name
    print(f"\nsmallest margin of any observation of any scan: {worst:.3e} m")
    assert worst >= FC.MARGIN_MIN


def test_fp64_floor(all_cases, reference_runs):
    H.measure_floor(all_cases, reference_runs, XC.SUITE)
    print(f"recorded at: sigma {XC.FP64_FLOOR_SIGMA_CASE}, mu {XC.FP64_FLOOR_MU_CASE}")
    assert XC.SUITE.floor_sigma == XC.FP64_FLOOR_SIGMA and XC.SUITE.floor_mu == XC.FP64_FLOOR_MU


def _defect_shows(case, k, mutation, suite):
    """-> (lists differ, largest error over its GPU bound) of the witness with `mutation` planted in scan k of `case`."""
    good, bad = MC.map_witness_of(case), MC.map_witness_of(case)
    for ev in FC.reference_events(case)[:k]:
        FC.feed(good, ev)
        FC.feed(bad, ev)
    ev = FC.reference_events(case)[k]
    fix = ev[4] if len(ev) > 4 else None
    good.handle_observation(ev[1], ev[3], fix)
    bad.handle_observation(ev[1], ev[3], fix, mutate=mutation)
    if good.last_match != bad.last_match:
        return True, np.inf
    es, em = H.rel_err(bad.mu, bad.sigma, good.mu, good.sigma)
    bs, bm = FC.gpu_bounds(good.mu, good.sigma, suite)
    return False, max(es / bs, em / bm)


# the dense cases each row defect is planted in: one of kind mix, one of kind wide (the step that holds both kinds of pairs)
ROW_DEFECT_CASES = ("map_mix_L33_S16_M16_diff", "map_wide_L128_S20_M20_omni")
# The two defects of the MATCH cannot show on this module's geometry: a map point is at least 1.6 m from every reflector (no
# observation is inside both gates, so the order of the branches decides nothing) and a map observation is within 2 mm of its
# point under weights whose scale is at most 2 (the weighted and the Euclidean distance are on the same side of 0.05).  They are
# caught by the cases of tests/fleet_map_cases.py written for them, which tests/test_ekf_map_gpu.py runs through a single handle
# (test_fleet_map_cases_through_a_single_filter, test_branch_order_cases_through_a_single_filter).
MATCH_DEFECT_CASES = {"state_gate_first": "branches_room", "threshold_unweighted": "weight_anisotropic"}


@pytest.mark.parametrize("mutation", MW.MAP_MUTATIONS)
def test_planted_defects_are_caught(mutation, all_cases):
    """Each planted defect of the witness changes the lists, or moves the state beyond the GPU bound, on the case named here."""
    assert set(MW.MAP_MUTATIONS) == {"map_rows_landmark_cols", "map_rows_first"} | set(MATCH_DEFECT_CASES)
    if mutation in MATCH_DEFECT_CASES:
        for c in all_cases:
            lists, ratio = _defect_shows(c, 0, mutation, XC.SUITE)
            assert not lists and ratio == 0.0, (c.name, mutation)      # (as reasoned above: it cannot show here)
        where = MATCH_DEFECT_CASES[mutation]
        c = next(c for c in MC.all_cases() if c.name == where)
        assert c.use
        lists, ratio = _defect_shows(c, 0, mutation, MC.SUITE)
        print(f"\n{mutation}: cannot show on the dense cases; on {where} (the fleet layer): the lists differ")
        assert lists
        return
    for where in ROW_DEFECT_CASES:
        c = XC.case_named(where)
        assert c.kind in ("mix", "wide") and c.MM >= 16 and c.Mm >= 16
        lists, ratio = _defect_shows(c, 0, mutation, XC.SUITE)
        print(f"\n{mutation} on {where} scan 0: the state moves by {ratio:.3g} x its GPU bound")
        assert not lists and ratio > 1.0
