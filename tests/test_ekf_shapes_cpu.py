"""The single filter's shape cases (tests/ekf_shape_cases.py) against the three CPU references (oracle/ekf_oracle.c,
oracle/ekf_numpy.py and the longdouble witness), so that tests/test_ekf_shapes_gpu.py is about the kernels only: the cases are
what they claim to be, the references agree on every association list, the FP64 noise floor that sets the GPU bound is measured
here, and the bound is shown to be able to fail on each kind of slip the single filter's launch forms could make."""
from __future__ import annotations

import collections

import numpy as np
import pytest

from tests import ekf_shape_cases as EC
from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests.witness import fleet_witness as FW

pytestmark = pytest.mark.skipif(not FW.available(), reason="numpy.longdouble has no 64-bit mantissa on this platform")


@pytest.fixture(scope="module")
def all_cases():
    return EC.cases()


@pytest.fixture(scope="module")
def reference_runs(all_cases, oracle_lib):
    """Every case through oracle, numpy and witness (fleet_harness.run_references asserts that all three give the claimed
    association lists on every scan)."""
    return {c.name: H.run_references(c, EC.SUITE) for c in all_cases}


def test_references_agree_on_every_association(all_cases, reference_runs):
    assert len(reference_runs) == len(all_cases) == len({c.name for c in all_cases})
    for c in all_cases:
        assert sorted(reference_runs[c.name]) == list(range(len(c.events))), c.name
        n_end = reference_runs[c.name][len(c.events) - 1][0][0][0].shape[0]
        assert n_end == 3 + 2 * (c.L + c.N2), (c.name, n_end)


def test_sweep_coverage(all_cases):
    by_kind = collections.defaultdict(list)
    for c in all_cases:
        by_kind[c.kind].append(c)
    sweep = by_kind["sweep"]
    assert len(sweep) <= 60 and [(c.L, c.K) for c in sweep] == EC.SWEEP_SHAPES
    per_L, per_K = collections.defaultdict(set), collections.defaultdict(set)
    for c in sweep:
        per_L[c.L].add(c.K)
        per_K[c.K].add(c.L)
    assert set(per_L) == set(EC.L_LISTED) | set(EC.L_RESIDUES) and set(per_K) == set(EC.K_LISTED)
    for L, ks in per_L.items():
        assert len(ks) >= 2 and min(ks) <= 16, (L, ks)
        if L > 17:
            assert max(ks) >= 17, (L, ks)
    assert all(len(ls) >= 3 for ls in per_K.values()), per_K
    nbr = collections.defaultdict(set)
    for c in sweep:
        nbr[c.n % 16].add(2 if 2 * c.K <= 32 else 4)
    assert set(nbr) == set(range(1, 16, 2)) and all(v == {2, 4} for v in nbr.values()), dict(nbr)
    assert [c.model for c in sweep] == [FC.DIFF if i % 2 == 0 else FC.OMNI for i in range(len(sweep))]
    assert {(c.L, c.K, c.MM) for c in by_kind["capacity"]} == {(L, K, MM) for L, K, MM in EC.CAPACITY_SHAPES}
    assert {(K, MM) for _, K, MM in EC.CAPACITY_SHAPES} == {(K, MM) for K in (16, 17, 32) for MM in (1, K - 1)}
    grow = [c for c in by_kind["growing"] if not c.auto_grow]
    assert {(c.L, c.n2_class) for c in grow} == {(L, cls) for L in (6, 14, 30, 62, 126) for cls in ("edge", "straddle", "cross")}
    auto = [c for c in by_kind["growing"] if c.auto_grow]
    assert len(auto) == 1 and auto[0].cap == 8 and auto[0].L == 7 and auto[0].N2 == 4 and auto[0].L + auto[0].N2 > auto[0].cap
    assert {(c.L, c.K) for c in by_kind["wide"]} == {(L, K) for L in (128, 200) for K in (33, 64, 65)}
    assert [(c.L, c.K) for c in by_kind["pose"]] == [(31, 14), (31, 15), (64, 30), (64, 31)]
    assert all(len(ev) == 5 and ev[4] is not None for c in by_kind["pose"] for ev in c.events)
    print(f"\n{len(all_cases)} cases:", {k: len(v) for k, v in by_kind.items()})


def test_cases_are_what_they_claim(all_cases):
    below, worst_cond = 0, 0.0
    for c in all_cases:
        full = c.kind in ("sweep", "capacity", "wide", "pose")
        assert (c.cap == c.L) == full and c.n == 3 + 2 * c.L == c.mu.shape[0], c.name
        assert c.vt[0] != 0 and c.vt[2] != 0 and [ev[1] for ev in c.events] == [EC.T0 + EC.DT * (k + 1) for k in range(len(c.events))]
        d = np.diag(c.P)
        assert 1e-4 <= d.min() and d.max() <= 1e-1 and np.array_equal(c.P, c.P.T), c.name
        lm = c.mu[3:].reshape(-1, 2)
        assert np.array_equal(lm, lm.astype(np.float32).astype(np.float64))
        dd = np.hypot(lm[:, None, 0] - lm[None, :, 0], lm[:, None, 1] - lm[None, :, 1]) + 10 * np.eye(lm.shape[0])
        assert dd.min() >= 1.5, c.name
        for k, ms in c.margins.items():
            assert len(ms) == len(FC.kept_cloud(c, k))
            below += sum(1 for a, b in ms if a < FC.MARGIN_MIN or b < FC.MARGIN_MIN)
        worst_cond = max(worst_cond, max(c.cond_S.values()))
        assert (c.flags == FC.FLAG_CAPACITY) == (c.kind == "capacity") and bool(c.kept) == (c.kind == "capacity")
        if c.kind == "wide":
            assert [len(ev[3]) for ev in c.events] == [c.K, 2] and len(c.expect[0][0]) == c.K
            assert {0, c.L - 1, 6, 30, c.L - 2} <= {g for _, g in c.expect[0][0]}
            continue
        assert len(c.events) == 4
        sets = [[g for _, g in c.expect[k][0]] for k in range(4)]
        order = [[g for _, g in sorted(c.expect[k][0])] for k in range(2)]
        assert len(c.events[0][3]) == c.K and len(sets[0]) == c.MM and len(c.expect[0][1]) == c.N2, c.name
        # scan 2: the same reflectors (a panel hit); in another order wherever there is more than one
        assert set(sets[1]) == set(sets[0]) and len(sets[1]) == c.MM and (c.MM < 2 or order[0] != order[1]), c.name
        # scan 3: another set of the same size (a miss)
        assert len(set(sets[2])) == c.MM and set(sets[2]) != set(sets[0]), c.name
        # scan 4: from scan 3's set, one reflector three times
        tri = EC.triple_of(c.L)
        cnt = collections.Counter(sets[3])
        assert set(sets[3]) <= set(sets[2]) and cnt[tri] == 3 and len(cnt) < len(sets[3]) and len(sets[3]) == max(3, c.MM), c.name
        if c.L > 6:
            assert tri == 6 and (3 + 2 * tri) % 16 == 15
        both = set(sets[0]) | set(sets[2])
        want = EC.musts(c.L)
        # (L = 6 and 7: three wanted reflectors and a set of three; scan 1 gives one up so that scan 3's set differs)
        assert c.L <= 7 or len(both & set(want)) >= min(len(want), c.MM) and (c.MM < len(want) or set(want) <= both), (c.name, want, sets)
        if c.L > 30 and c.MM >= 4:
            assert 30 in set(sets[0]) and (3 + 2 * 30) % 64 == 63
        if c.N2:                                               # the grown state: scan 3 matches what scan 1 appended
            assert c.MM < 2 or c.L + c.N2 - 1 in sets[2], (c.name, sets[2])
    print(f"\nobservations below the {FC.MARGIN_MIN} margin: {below}; largest cond(S): {worst_cond:.3g}")
    assert below == 0 and worst_cond < 1e5


def test_pose_witness_agrees_with_the_oracles_joint_update(all_cases, reference_runs):
    """The single filter applies the three pose rows jointly with the reflector rows, as oracle/ekf_oracle.c does; the joint form
    of tests/witness/fleet_pose_witness.py is its witness.  On the pose cases (31, 33, 63 and 65 rows) the two agree to the floor."""
    for c in (c for c in all_cases if c.kind == "pose"):
        for k, (wits, orc, npy) in reference_runs[c.name].items():
            es, em = H.rel_err(*orc, *wits[0])
            print(f"  {c.name} scan {k}: oracle against the joint witness: sigma {es:.3e}, mu {em:.3e}")
            assert es <= EC.SUITE.floor_sigma and em <= EC.SUITE.floor_mu


def test_fp64_floor(all_cases, reference_runs):
    H.measure_floor(all_cases, reference_runs, EC.SUITE)
    print(f"recorded at: sigma {EC.FP64_FLOOR_SIGMA_CASE}, mu {EC.FP64_FLOOR_MU_CASE}")
    assert EC.SUITE.floor_sigma == EC.FP64_FLOOR_SIGMA and EC.SUITE.floor_mu == EC.FP64_FLOOR_MU


def _own_row(c, k):
    """A row of the last, partly filled 16-row workgroup that belongs to no reflector scan k matches (else the state's last row)."""
    in_R = {g for _, g in c.expect[k][0]}
    for row in range(c.n - 1, 16 * ((c.n - 1) // 16) - 1, -1):
        if row >= 3 and (row - 3) // 2 not in in_R:
            return row
    return c.n - 1


# mutation -> (case, scan it is planted in, where)
def _plant(mutation):
    if mutation == "stale_gather":
        c = EC.case_named("single_L31_K16_diff")
        assert 6 in {g for _, g in c.expect[1][0]}
        return [(c, 1, (3 + 2 * 6, 2))]                          # the 16-row straddler's first row against pose row 2
    if mutation == "stale_own_row":
        c = EC.case_named("single_L33_K16_diff")              # n = 69: the last workgroup holds rows 64 .. 68
        row = _own_row(c, 1)
        assert row >= 64
        return [(c, 1, (row, 2))]
    if mutation == "skip_tile64":
        c = EC.case_named("single_L94_K16_diff")              # n = 191: three tile rows
        return [(c, 0, (2, 0))]
    if mutation == "border_strip":
        return [(EC.case_named("single_L31_K16_diff"), 0, None), (EC.case_named("single_L63_K15_diff"), 0, None)]    # n = 65, 129
    if mutation == "w_row_shift":
        c = EC.case_named("single_L63_K15_diff")
        assert 30 in {g for _, g in c.expect[0][0]}
        return [(c, 0, (63, 3))]                                 # row 63 | 64: the 64-row straddler
    if mutation == "k_pad_col":
        c = EC.case_named("single_L30_K15_diff")
        assert (2 * c.K) % 4 == 2
        return [(c, 0, None)]
    c = EC.case_named("single_wide_L128_K33_diff")
    return [(c, 0, None)]


@pytest.mark.parametrize("mutation", FW.SINGLE_MUTATIONS)
def test_the_bound_can_fail(mutation):
    """One planted defect per kind of slip, on the case designed for it: the mutated witness leaves the clean one by more than
    the case's GPU bound."""
    for c, scan, where in _plant(mutation):
        if mutation == "border_strip":
            assert c.n % 64 == 1
        good, bad = FC.witness_of(c), FC.witness_of(c)
        for k, ev in enumerate(FC.reference_events(c)[:scan + 1]):
            good.handle_observation(ev[1], ev[3])
            bad.handle_observation(ev[1], ev[3], **(dict(mutate=mutation, where=where) if k == scan else {}))
        es, em = H.rel_err(bad.mu, bad.sigma, good.mu, good.sigma)
        bs, bm = FC.gpu_bounds(good.mu, good.sigma, EC.SUITE)
        print(f"\n{mutation} on {c.name} scan {scan}: sigma moves by {es:.3e} = {es / bs:.3g} x the GPU bound {bs:.3e}; "
              f"mu by {em:.3e} = {em / bm:.3g} x its bound")
        assert es > bs
