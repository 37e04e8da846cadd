"""The fleet filter's shared pre-loaded map, what can be checked without a GPU: the cases of tests/fleet_map_cases.py against the
three CPU references (oracle/ekf_oracle.c, oracle/ekf_numpy.py, the longdouble witness with the map branch), the margins of
every claimed association, the FP64 floor that sets the GPU bound, planted defects against lists and bound, and the C ABI."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as MC
from tests.fleet_harness import HEADER, _lib
from tests.witness import fleet_map_witness as MW

needs_ld = pytest.mark.skipif(not MW.available(), reason="numpy.longdouble has no 64-bit mantissa on this platform")


@pytest.fixture(scope="module")
def all_cases():
    return MC.all_cases()


@pytest.fixture(scope="module")
def reference_runs(all_cases):
    """Per case and scan: ([witness state], oracle state, numpy state); the lists of all three are checked on the way."""
    return {c.name: MC.run_references(c) for c in all_cases}


@needs_ld
def test_cases_are_what_they_claim(all_cases, reference_runs):
    assert len(reference_runs) == len(all_cases) == len({c.name for c in all_cases})
    by = {c.name: c for c in all_cases}
    # map sizes at the wave sweep's edges, the matched points at 0, 63, 64 and M_ - 1
    assert [c.map_xy.shape[0] for c in MC.size_cases()] == [1, 63, 64, 65, 129, 2048]
    for c in MC.size_cases():
        M_ = c.map_xy.shape[0]
        assert c.mu.shape[0] == 3 and [j for _, j in c.expect[0][1]] == sorted({j for j in (0, 63, 64, M_ - 1) if j < M_})
    # ties: exactly equal weighted distances, the lower index claimed
    from tests.witness.fleet_map_witness import weighted_distances
    for c in MC.tie_cases():
        p = c.events[0][3][0]
        dw, _ = weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]))
        assert len({float(dw[j]) for j in c.tie}) == 1 and float(dw[c.tie[0]]) == float(dw.min()), c.name
        if c.expect[0][1]:
            assert c.expect[0][1][0][1] == min(c.tie) and dw.min() < MC.MAP_GATE
        else:
            assert dw.min() >= MC.MAP_GATE + MC.MARGIN_MIN and c.expect[0][2] == [0]
    assert any(c.tie[1] - c.tie[0] == 64 for c in MC.tie_cases()) and any(c.tie[1] - c.tie[0] == 1 for c in MC.tie_cases())
    # row mixes, each with the smallest state (n = 3 when no state row exists) and with L = 128
    mixes = MC.mix_cases()
    assert {c.mix for c in mixes} == set(MC.MIXES) and {c.L for c in mixes if c.mix[0] == 0} == {0, 128}
    for c in mixes:
        ns, nm, nn = c.mix
        sp, mp, nw = c.expect[0]
        assert (len(sp), len(mp)) == (ns, nm) and c.mu.shape[0] == 3 + 2 * c.L and c.events[0][3].shape[0] == ns + nm + nn
        assert len(nw) == (nn if c.L < 128 else 0) and c.flags == (FC.FLAG_CAPACITY if c.L == 128 and nn else 0)
    assert by["branches_room"].expect[0] == ([(1, 1)], [(0, 2)], [2]) and by["branches_full"].expect[0] == ([(1, 1)], [(0, 2)], [])
    assert by["branches_full"].flags == FC.FLAG_CAPACITY and by["branches_room"].flags == 0
    # observation 0 of the branch cases is inside BOTH gates, observation 1 inside the state gate only
    c = by["branches_room"]
    w = MC.map_witness_of(c)
    w.predict(c.events[0][1] - w.time)
    d = [float(w.distances(p).min()) for p in c.events[0][3]]
    assert d[0] < 0.6 and c.map_margins[0][0][2] and d[1] < 0.6 and not c.map_margins[0][1][2] and d[2] > 0.6
    # the weights: the weighted nearest point is not the Euclidean nearest; a non-symmetric weight
    c = by["weight_anisotropic"]
    p = c.events[0][3][0]
    dw, de = weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]))
    assert int(np.argmin(dw)) == 7 and int(np.argmin(de)) == 3 and c.expect[0][1][0] == (0, 7)
    S = by["weight_non_symmetric"].map_cov[0]
    assert S[1] != S[2]
    assert [c.rows for c in MC.fix_cases()] == [5, 65, 67] and all(c.events[0][4] is not None for c in MC.fix_cases())
    assert not by["unused_map"].use and by["unused_map"].expect[0][1] == [] and len(by["unused_map"].expect[0][2]) == 10
    c = by["two_scans"]
    assert c.mu.shape[0] == 3 and len(c.expect[0][2]) == 3 and [j for _, j in c.expect[1][0]] == [0, 1, 2] and len(c.expect[1][1]) == 2


@needs_ld
def test_nan_cases_are_what_they_claim(all_cases, reference_runs):
    """The NaN rule (a NaN weighted distance never wins; all NaN: on to the state branch).  The three references give the claimed
    lists on every nan case (reference_runs asserts that for every case; said here by name), the distances that are NaN are
    exactly those of the points the case names, and the (p, q) pairs are the ones the wave sweep of 64 lanes can get wrong."""
    nan = MC.nan_cases()
    by = {c.name: c for c in all_cases}
    assert len(nan) == 9 and all(c.name in by and c.name in reference_runs for c in nan)
    assert [(c.nan_at[0], c.expect[0][1][0][1]) for c in nan[:5]] == [(0, 1), (5, 69), (5, 37), (70, 3), (64, 0)] == list(MC.NAN_PQ)
    for c in nan:
        assert sorted(reference_runs[c.name]) == [0] and len(c.events) == 1
        for q, p in enumerate(c.events[0][3]):
            dw, _ = MW.weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]))
            bad = np.nonzero(np.isnan(dw))[0].tolist()
            assert bad in ([], c.nan_at), (c.name, q, bad)
            pair = [j for i, j in c.expect[0][1] if i == q]
            if pair:                                           # the first minimum over the numbers, inside the gate
                assert pair[0] not in bad and dw[pair[0]] == np.nanmin(dw) < MC.MAP_GATE and int(np.nanargmin(dw)) == pair[0]
            else:
                assert len(bad) == dw.shape[0] or np.nanmin(dw) >= MC.MAP_GATE + MC.MARGIN_MIN
        assert any(np.isnan(MW.weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]))[0]).any() for p in c.events[0][3])
    # same lane a stride later; a lane whose result reaches lane 0 through lane 5 in the xor butterfly (32, 16, 8, 4, 2, 1)
    assert 69 % 64 == 5 and 37 ^ 32 == 5 and 64 % 64 == 0 and 70 % 64 != 3
    c = by["nan_nearest_5_runner_up_69"]
    p = c.events[0][3][0]
    _, de = MW.weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]))
    assert int(np.argmin(de)) == 5 and c.expect[0] == ([], [(0, 69)], []) and float(de[69]) == 3 / 64
    c = by["nan_everywhere"]
    assert c.mu.shape[0] == 7 and c.expect[0] == ([(0, 0)], [], [1]) and (c.map_cov == np.asarray(MC.INDEFINITE)).all()
    assert float(np.hypot(*(c.events[0][3][0] - c.mu[3:5]))) <= 2e-3
    assert by["nan_M1"].map_xy.shape[0] == 1 and by["nan_M1"].expect[0] == ([], [], [0])
    c = by["nan_semi_definite_66"]
    assert c.map_cov[66].tolist() == [1.0, 0.0, 0.0, -1 / 1024] and c.expect[0] == ([], [(0, 66)], [1])
    d0, d1 = c.events[0][3][0] - c.map_xy[66], c.events[0][3][1] - c.map_xy[66]
    assert d0.tolist() == [1 / 64, 0.0] and d1.tolist() == [0.0, 1 / 64]


def test_margins(all_cases):
    """Every claimed association is clear of its thresholds: the best weighted distance at least MARGIN_MIN metres (scaled by the
    weight) from 0.05, inside the gate the second best that far behind (ties excepted: they are the point of their cases;
    outside the gate the index of the best point decides nothing), and for an observation that reaches the state branch |d1 - 0.6| at least MARGIN_MIN and, inside that gate, d2 - d1 too.
    A map point whose weighted distance is NaN is skipped (fleet_map_cases.map_margins leaves it out by name: it can never be the
    pair); the best and the second best are those of the remaining points, and no case is excused.  Where every point is skipped
    the map margins are infinite and the state margins decide."""
    worst = np.inf
    skipped = 0
    for c in all_cases:
        for k in c.map_margins:
            mapped, in_state = {i for i, _ in c.expect[k][1]}, {i for i, _ in c.expect[k][0]}
            keep = c.kept.get(k)
            for p in FC.kept_cloud(c, k):
                dw, _ = MW.weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]))
                n_nan = int(np.isnan(dw).sum())
                assert n_nan == 0 or hasattr(c, "nan_at"), (c.name, k)
                skipped += n_nan
            for q, (a, b, inside) in enumerate(c.map_margins[k]):
                i = q if keep is None else keep[q]
                assert inside == (i in mapped), (c.name, k, i)
                assert a >= MC.MARGIN_MIN, (c.name, k, i, a)
                if inside and not hasattr(c, "tie"):
                    assert b >= MC.MARGIN_MIN, (c.name, k, i, b)
                worst = min(worst, a)
                if not inside:
                    sa, sb = c.margins[k][q]
                    assert sa >= MC.MARGIN_MIN and (sb >= MC.MARGIN_MIN or i not in in_state), (c.name, k, i, sa, sb)
    print(f"\nsmallest distance of a best weighted distance from the map gate, in metres: {worst:.3e}; NaN distances skipped: {skipped}")
    assert skipped == 5 + 1 + 2 * 129 + 1 + 1


@needs_ld
def test_fp64_floor(all_cases, reference_runs):
    H.measure_floor(all_cases, reference_runs, MC.SUITE)


def _defect_shows(case, k, mutation):
    """-> (lists differ, largest error over its GPU bound) of the witness with `mutation` planted in scan k of `case`."""
    good, bad = MC.map_witness_of(case), MC.map_witness_of(case)
    for ev in FC.reference_events(case)[:k]:
        FC.feed(good, ev)
        FC.feed(bad, ev)
    ev = FC.reference_events(case)[k]
    good.handle_observation(ev[1], ev[3], ev[4])
    bad.handle_observation(ev[1], ev[3], ev[4], mutate=mutation)
    if good.last_match != bad.last_match:
        return True, np.inf
    es, em = H.rel_err(bad.mu, bad.sigma, good.mu, good.sigma)
    bs, bm = FC.gpu_bounds(good.mu, good.sigma, MC.SUITE)
    return False, max(es / bs, em / bm)


@needs_ld
@pytest.mark.parametrize("mutation", MW.MAP_MUTATIONS)
def test_planted_defects_are_caught(mutation, all_cases):
    """Each planted defect changes the association lists of at least one case, or moves its state beyond the GPU bound."""
    by = {c.name: c for c in all_cases}
    where = {"map_rows_landmark_cols": "mix_16_16_0_L16", "state_gate_first": "branches_room",
             "threshold_unweighted": "weight_anisotropic", "map_rows_first": "mix_16_16_0_L16"}[mutation]
    lists, ratio = _defect_shows(by[where], 0, mutation)
    print(f"\n{mutation} on {where}: " + ("the lists differ" if lists else f"the state moves by {ratio:.3g} x its GPU bound"))
    assert lists or ratio > 1.0
    if mutation in ("state_gate_first", "threshold_unweighted"):
        assert lists


def test_the_subtraction_order_cannot_be_seen():
    """`map - g` taken as `g - map` in float32: round-to-nearest is symmetric, so fl(a - b) == -fl(b - a) exactly, and
    (delta S) delta^T is even in delta (every product changes sign twice or not at all, exactly).  No rounding case can show this
    defect, so it is not among MAP_MUTATIONS; this test states the identity on random bits instead."""
    rng = np.random.default_rng(5)
    a = rng.normal(size=4096).astype(np.float32) * np.float32(50.0)
    b = (a + rng.normal(size=4096).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    assert np.array_equal((a - b).astype(np.float32), -((b - a).astype(np.float32)))
    S = rng.normal(size=(4096, 4))
    dx, dy = (a - b).astype(np.float64), (b - a).astype(np.float64)[::-1].copy()
    for sx, sy in ((dx, dy), (-dx, -dy)):
        t0, t1 = sx * S[:, 0] + sy * S[:, 2], sx * S[:, 1] + sy * S[:, 3]
        v = t0 * sx + t1 * sy
        if sx is dx:
            ref = v
    assert np.array_equal(ref, v)


def test_transposed_weight_is_the_same_distance(all_cases):
    """The weight read column-major (S[1] and S[2] swapped): delta S delta^T == delta S^T delta^T, so this slip changes the
    weighted distance by FP64 round-off only, and neither a list with a margin nor a bound can see it.  What the non-symmetric
    case pins is that such a weight is handled at all; this test measures the round-off over every observation and map point."""
    worst = 0.0
    for c in all_cases:
        if not c.use:
            continue
        for p in c.events[0][3]:
            a, _ = MW.weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]))
            b, _ = MW.weighted_distances(c.map_xy, c.map_cov, np.float32(p[0]), np.float32(p[1]), column_major=True)
            ok = ~(np.isnan(a) | np.isnan(b))                    # (a NaN distance is NaN either way: nan_cases)
            assert np.array_equal(np.isnan(a), np.isnan(b))
            if ok.any():
                worst = max(worst, float(np.abs(a[ok] - b[ok]).max() / a[ok].max()))
    print(f"\nrow-major against column-major weights: largest relative difference of a distance {worst:.2e}")
    assert worst < 1e-15
    assert "cov_column_major" in MW.UNOBSERVABLE_MUTATIONS and "cov_column_major" not in MW.MAP_MUTATIONS


def test_session_is_what_the_gpu_test_needs():
    s = MC.session()
    scans = [k for k, ev in enumerate(s.events) if ev[0] == FC.EV_SCAN]
    assert len(scans) == s.scans == MC.SESSION_SCANS <= 60 and s.map_xy.shape == (8, 2) and sorted(s.records) == scans
    assert sum(len(s.records[k][1]) for k in scans) > 100 and sum(len(s.records[k][0]) for k in scans) > 100
    assert len(set(MC.SESSION_MEMBERS)) == 4


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_map_calls_and_keeps_the_abi_version():
    text = open(HEADER).read()
    assert re.search(r"int\s+rfleet_set_map\s*\(\s*rfleet_t\s*\*\s*f\s*,\s*const\s+float\s*\*\s*xy\s*,\s*const\s+double\s*\*\s*cov\s*,\s*int\s+M\s*,"
                     r"\s*const\s+unsigned\s+char\s*\*\s*use", text)
    assert re.search(r"int\s+rfleet_get_map_size\s*\(\s*rfleet_t\s*\*\s*f\s*,\s*int\s*\*\s*M\s*\)", text)
    assert re.search(r"#define\s+RFLEET_MAX_MAP_POINTS\s+2048\b", text) and re.search(r"#define\s+RFLEET_ABI_VERSION\s+2\b", text)
    assert "n_map is always 0" not in text and "*n_map is always 0" not in text
    assert _lib().rfleet_abi_version() == 2


def test_set_map_refusals_come_before_any_hip_call():
    """Every refusal of rfleet_set_map with its code, on a machine without a device: nothing here may reach HIP.  The handle is a
    dummy the library must not look into before it has refused."""
    from reflector_ekf_slam_amd import fleet
    L = fleet._map_lib()
    xy = np.zeros((4, 2), np.float32)
    cov = np.tile(np.asarray(MC.IDENTITY), (4, 1))
    INVALID, UNSUPPORTED = -1, L.rfleet_set_map(C.c_void_p(1), xy.ctypes.data, cov.ctypes.data, 2049, None)   # (refused before it reads)
    m = C.c_int(7)
    assert L.rfleet_set_map(None, xy.ctypes.data, cov.ctypes.data, 4, None) == INVALID
    assert L.rfleet_set_map(None, None, None, 0, None) == INVALID
    assert L.rfleet_get_map_size(None, C.byref(m)) == INVALID and L.rfleet_get_map_size(C.c_void_p(1), None) == INVALID
    dummy = C.c_void_p(1)
    assert L.rfleet_set_map(dummy, xy.ctypes.data, cov.ctypes.data, -1, None) == INVALID
    assert L.rfleet_set_map(dummy, None, cov.ctypes.data, 4, None) == INVALID
    assert L.rfleet_set_map(dummy, xy.ctypes.data, None, 4, None) == INVALID
    assert UNSUPPORTED != INVALID and UNSUPPORTED < 0
    text = open(H.HEADER.replace("rfleet.h", "rekf.h")).read()
    assert int(re.search(r"REKF_ERR_UNSUPPORTED\s*=\s*(-?\d+)", text).group(1)) == UNSUPPORTED
    assert int(re.search(r"REKF_ERR_INVALID\s*=\s*(-?\d+)", text).group(1)) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        x = xy.copy()
        x[3, 1] = bad
        assert L.rfleet_set_map(dummy, x.ctypes.data, cov.ctypes.data, 4, None) == INVALID
        s = cov.copy()
        s[2, 1] = bad
        assert L.rfleet_set_map(dummy, xy.ctypes.data, s.ctypes.data, 4, None) == INVALID


def test_the_binding_looks_the_map_calls_up_lazily(monkeypatch):
    """rfleet() itself does not ask for the new symbols (a library of ABI version 2 without them keeps serving everything else);
    _map_lib() does, once, and raises LibraryMissing when they are absent."""
    from reflector_ekf_slam_amd import _lib as base
    from reflector_ekf_slam_amd import fleet

    real = fleet.rfleet()

    class Old:
        """A library handle of ABI version 2 from before the map calls."""
        def __getattr__(self, name):
            if name in ("rfleet_set_map", "rfleet_get_map_size"):
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(fleet._map_lib, "ready", None)
    monkeypatch.setattr(fleet.rfleet, "ready", Old())
    with pytest.raises(base.LibraryMissing):
        fleet._map_lib()
    monkeypatch.setattr(fleet.rfleet, "ready", real)
    got = fleet._map_lib()
    assert got is real and fleet._map_lib.ready is real and got.rfleet_set_map.argtypes is not None
    assert callable(fleet.ReflectorEKFSLAMFleet.set_map) and callable(fleet.ReflectorEKFSLAMFleet.map_size)
    assert not hasattr(fleet.FleetMember, "set_map")
