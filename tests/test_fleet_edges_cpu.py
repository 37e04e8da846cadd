"""The fleet filter's sweep and edge cases against the three CPU references (oracle/ekf_oracle.c, oracle/ekf_numpy.py and the
longdouble witness), so that tests/test_fleet_edges_gpu.py is about the kernel only: the cases are what they claim to be, the
references agree, the FP64 noise floor that sets the GPU bound is measured here, and the bound is shown to be able to fail."""
from __future__ import annotations

import collections

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests.witness import fleet_witness as FW

pytestmark = pytest.mark.skipif(not FW.available(), reason="numpy.longdouble has no 64-bit mantissa on this platform")


@pytest.fixture(scope="module")
def all_cases():
    return FC.sweep_cases() + FC.crafted_cases()


@pytest.fixture(scope="module")
def reference_runs(all_cases):
    return {c.name: H.run_references(c, FC.SUITE) for c in all_cases}


def test_associations_agree_and_are_the_claimed_ones(all_cases, reference_runs):
    assert len(reference_runs) == len(all_cases) == len({c.name for c in all_cases})
    c = FC.singular_case()                                     # no update possible in the witness: the association alone
    w = FC.witness_of(c)
    w.predict(c.events[0][1] - c.t)
    assert w.match(c.events[0][3]) == ([tuple(p) for p in c.expect[0][0]], list(c.expect[0][1]))
    with pytest.raises(ArithmeticError):
        FC.witness_of(c).handle_observation(c.events[0][1], c.events[0][3])
    S = FC.innovation_cov(c.mu, c.P, c.expect[0][0])
    assert -2.0 < S[0, 0] < -0.1 and np.isfinite(S).all()


def test_sweep_coverage():
    cs = FC.sweep_cases()
    assert 100 <= len(cs) <= 150
    combos = collections.Counter((c.n % 16, FC.m_class(c.MM)) for c in cs)
    table = collections.defaultdict(dict)
    for (r, mc), cnt in combos.items():
        table[r][mc] = cnt
    print("\nsweep coverage: rows n mod 16, columns (m4 % 8 class, m16); cells = cases")
    cols = sorted(FC.M_CLASSES, key=str)
    print("      " + " ".join(f"{c[0]:>3}/{c[1]:<2}" for c in cols))
    for r in range(1, 16, 2):
        print(f"  {r:3d} " + " ".join(f"{table[r].get(c, 0):6d}" for c in cols))
        for c in cols:
            assert table[r].get(c, 0) >= 1, (r, c)
    assert set(FC.MM_LISTED) <= {c.MM for c in cs}
    assert set(FC.N_LISTED) <= {c.n for c in cs}
    n2 = collections.Counter(FC.n2_class(c.n, c.N2) for c in cs)
    print("  N2 classes:", dict(n2), " models:", dict(collections.Counter(c.model for c in cs)))
    assert all(n2[k] >= 8 for k in ("0", "1", "inside", "edge", "straddle", "cross"))
    assert {c.model for c in cs} == {FC.DIFF, FC.OMNI}
    below = 0
    for c in cs:
        assert all(v != 0 for v in c.vt[::2]) and c.events[0][1] > c.t and c.max_landmarks == 128
        d = np.diag(c.P)
        assert 1e-4 <= d.min() and d.max() <= 1e-1 and np.array_equal(c.P, c.P.T)
        lm = c.mu[3:].reshape(-1, 2)
        assert np.array_equal(lm, lm.astype(np.float32).astype(np.float64))
        if lm.shape[0] > 1:
            dd = np.hypot(lm[:, None, 0] - lm[None, :, 0], lm[:, None, 1] - lm[None, :, 1]) + 10 * np.eye(lm.shape[0])
            assert dd.min() >= 1.5
        assert len(c.expect[0][0]) == c.MM and len(c.expect[0][1]) == c.N2
        for k in (0, 1):
            below += sum(1 for a, b in c.margins[k] if a < FC.MARGIN_MIN or b < FC.MARGIN_MIN)
            for (a, _), q in zip(c.margins[k], range(len(c.margins[k]))):
                if q in c.expect[k][1]:
                    assert a >= 1.5 - FC.GATE - 0.05, (c.name, k, q, a)    # new observations: 1.5 m from every reflector
        assert max(c.cond_S.values()) < 1e5, (c.name, c.cond_S)
    print(f"  observations below the {FC.MARGIN_MIN} margin: {below}; largest cond(S): {max(max(c.cond_S.values()) for c in cs):.3g}")
    assert below == 0


def test_crafted_cases_are_exact():
    for c in FC.gate_cases():
        w = FC.witness_of(c)
        w.predict(c.events[0][1] - c.t)
        d1 = [float(w.distances(p).min()) for p in c.events[0][3]]
        lo, hi = float(np.nextafter(np.float32(0.6), np.float32(0))), float(np.float32(0.6))
        assert d1 == c.gate and set(d1) == {lo, hi} and lo < 0.6 < hi and np.nextafter(np.float32(lo), np.float32(1)) == np.float32(hi)
    for c in FC.tie_cases():
        w = FC.witness_of(c)
        w.predict(c.events[0][1] - c.t)
        d = w.distances(c.events[0][3][0])
        tied = [d[j] for j in c.tie]
        assert all(v == tied[0] for v in tied) and tied[0] == d.min(), (c.name, tied)
        assert np.sort(d)[len(tied)] > tied[0] + 1.0
        assert (tied[0] < FC.GATE) == (len(c.expect[0][0]) == 1)
        if c.expect[0][0]:
            assert c.expect[0][0][0][1] == min(c.tie)
    for c in FC.heading_cases():
        w = FC.witness_of(c)
        th = [float(w.mu[2])]
        for ev in c.events:
            FC.feed(w, ev)
            th.append(float(w.mu[2]))
        sg = c.heading
        assert abs(abs(th[0]) - np.pi) < 1e-3 and th[0] * sg > 0
        assert th[1] * sg < 0 and abs(abs(th[1]) - np.pi) < 3e-3, th             # Predict carried it across
        assert th[3] * sg > 0 and abs(abs(th[3]) - np.pi) < 3e-3, th             # the update's correction carried it back
        assert c.events[3][1] < c.events[2][1]                                   # time goes backwards once
    for c in FC.capacity_cases():
        assert c.mu.shape[0] == 23 and c.max_landmarks == 10 + c.room
        assert [q for q in range(9) if q not in [p[0] for p in c.expect[0][0]]] == [0, 2, 3, 5, 7]
        assert len(c.expect[0][1]) == c.room and len(c.expect[1][0]) == 8 and len(c.events[1][3]) == 11


def test_witness_is_pinned_by_mpmath():
    """Small shapes once more in mpmath at 40 digits (the same dense formulas on another number type): the longdouble witness
    agrees at the 1e-17 relative level, so its own error is far below the FP64 floor it measures."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    kit = FW.Kit(mp)
    small = FC.pin_cases()
    assert len(small) >= 6 and all(c.n <= 33 and 2 * c.MM <= 16 and max(c.cond_S.values()) <= 100 for c in small)
    worst = 0.0
    for c in small:
        w = FC.witness_of(c)
        h = FW.WitnessEKF(c.model, c.t, c.mu[:3], FC.LIN_COV, FC.ANG_COV, FC.OBS_COV, kit=kit)
        h.set_state(c.t, c.mu, c.P, c.vt)
        for ev in FC.reference_events(c):
            FC.feed(w, ev)
            FC.feed(h, ev)
        assert w.last_match == h.last_match
        smax = max(abs(v) for v in h.sigma.ravel())
        es = max(abs(mp.mpf(float(a)) + mp.mpf(float(a - np.longdouble(float(a)))) - b) for a, b in zip(w.sigma.ravel(), h.sigma.ravel())) / smax
        mmax = max(1, max(abs(v) for v in h.mu))
        em = max(abs(mp.mpf(float(a)) + mp.mpf(float(a - np.longdouble(float(a)))) - b) for a, b in zip(w.mu, h.mu)) / mmax
        print(f"  {c.name}: cond(S) {max(c.cond_S.values()):.0f}, sigma {float(es):.2e}, mu {float(em):.2e}")
        worst = max(worst, float(es), float(em))
    print(f"\nlongdouble witness against mpmath (40 digits), {len(small)} small cases: worst relative error {worst:.2e}")
    assert worst < 1e-17


def test_fp64_floor(all_cases, reference_runs):
    H.measure_floor(all_cases, reference_runs, FC.SUITE)
    print(f"recorded at: sigma {FC.FP64_FLOOR_SIGMA_CASE}, mu {FC.FP64_FLOOR_MU_CASE}")
    for c in all_cases:
        if c.kind == "sweep":                                  # in the sweep the floor is what binds, not the absolute tolerance
            for k, (wits, _, _) in reference_runs[c.name].items():
                assert FC.gpu_bounds(*wits[0], FC.SUITE) == (FC.GPU_FACTOR * FC.FP64_FLOOR_SIGMA, FC.GPU_FACTOR * FC.FP64_FLOOR_MU), (c.name, k)


def pick(cs, pred):
    return next(c for c in cs if pred(c))


@pytest.mark.parametrize("mutation", FW.MUTATIONS)
def test_the_bound_can_fail(mutation):
    """One planted defect per kind of indexing slip: each moves sigma by at least 100 x the GPU bound."""
    cs = FC.sweep_cases()
    if mutation == "drop_last4":
        c, where = pick(cs, lambda c: FC.m_class(c.MM)[0] == "4" and c.n > 64), None
    elif mutation == "skip_tile":
        c = pick(cs, lambda c: c.n >= 100 and c.MM >= 8)
        where = (c.n // 16 - 1, 2)
    elif mutation == "w_row_shift":
        c = pick(cs, lambda c: c.n >= 40 and c.MM >= 4)
        where = (c.n // 2, 3)
    else:
        c, where = pick(cs, lambda c: c.MM % 2 == 1 and c.MM >= 3), None
    good, bad = FC.witness_of(c), FC.witness_of(c)
    ev = c.events[0]
    good.handle_observation(ev[1], ev[3])
    bad.handle_observation(ev[1], ev[3], mutate=mutation, where=where)
    es, _ = H.rel_err(bad.mu, bad.sigma, good.mu, good.sigma)
    bound, _ = FC.gpu_bounds(good.mu, good.sigma, FC.SUITE)
    print(f"\n{mutation} on {c.name}: sigma moves by {es:.3e} = {es / bound:.3g} x the GPU bound {bound:.3e}")
    assert es >= 100 * bound
