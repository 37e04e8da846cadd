"""Cases of the fleet filter's shared pre-loaded map (rfleet_set_map; reference reflector_ekf_slam.cc:401-425, :279-302), shared by
tests/test_fleet_map_cpu.py (the cases and the three CPU references against each other) and tests/test_fleet_map_gpu.py
(k_fleet_step_map against the longdouble witness with the map branch).  Built on tests/fleet_cases.py: a case is that module's
record plus ``map_xy`` / ``map_cov`` (the fleet's map while the case runs), ``use`` (the member's switch) and, per scan, the claimed
lists ``expect[k] = (state_pairs, map_pairs, new_ids)``.

Every crafted case has its pose at the origin and no velocity, so the first scan's sensor frame is the global frame and every
coordinate is a float32-exact dyadic number.  Three lattices that cannot be confused: reflectors of the state on EVEN metres
(fleet_cases.far_lattice), map points on ODD metres (sqrt 2 from any of those), new observations on (odd, even) (1 m from both).
A scan is written as tokens, which are the claim: ("m", j) an observation 0.014 m or less from map point j, ("s", j) the same
from reflector j of the state, ("n", point); a token may carry its own point.

nan_cases: a weighted distance that is NaN (an indefinite weight) never wins, wherever it stands -- the one rule of the three
references, the fleet kernel and (where tests/test_ekf_map_gpu.py does not list a divergence) the single filter.

A fleet has ONE map, so the lockstep run (run_lockstep) makes all cases members of one fleet per capacity and walks them group by
group, replacing the map in between; a case with ``use = False`` sits in the fleet while the map is set and must not see it.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace as NS

import numpy as np

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests.helpers import norm_match

EV_ODOM, EV_SCAN = FC.EV_ODOM, FC.EV_SCAN
MAP_GATE = 0.05
MARGIN_MIN = FC.MARGIN_MIN
IDENTITY = (1.0, 0.0, 0.0, 1.0)
FIX = (0.02, -0.03, 0.01)

# ---- the FP64 noise floor of these cases -------------------------------------------------------------------------------------
# Measured by tests/test_fleet_map_cpu.py::test_fp64_floor as tests/test_fleet_edges_cpu.py does for the plain update: the larger
# error of oracle/ekf_oracle.c and oracle/ekf_numpy.py against the longdouble witness over every scan of every case below.
# Recorded = measured, rounded up to two digits; the test fails when a re-measurement exceeds it or falls below half.
FP64_FLOOR_SIGMA = 2.9e-12    # measured 2.849e-12 (fix_0_31 scan 0, numpy)
FP64_FLOOR_MU = 1.1e-16       # measured 1.005e-16 (fix_0_31 scan 0, oracle)


def map_witness_of(case):
    from tests.witness.fleet_map_witness import MapWitnessEKF
    w = MapWitnessEKF(case.model, case.t, case.mu[:3], FC.LIN_COV, FC.ANG_COV, FC.OBS_COV)
    w.set_state(case.t, case.mu, case.P, case.vt)
    if case.use:
        w.set_map(case.map_xy, case.map_cov)
    return w


def oracle_of(case):
    o = FC.oracle_of(case)
    if case.use:
        o.set_map(case.map_xy, case.map_cov)
    return o


def numpy_of(case):
    e = FC.numpy_of(case)
    if case.use:
        e.set_map(case.map_xy, case.map_cov)
    return e


SUITE = NS(name="map", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU, witnesses={"witness": map_witness_of})


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def map_lattice(M):
    """M points on odd metres, the nearest rings first (a small map is around the robot), row-major inside a ring."""
    pts = [(2.0 * ix + 1.0, 2.0 * iy + 1.0) for iy in range(-23, 23) for ix in range(-23, 23)]
    pts.sort(key=lambda p: max(abs(p[0]), abs(p[1])))
    assert M <= len(pts)
    return pts[:M]


def new_lattice(count):
    pts = [(2.0 * ix + 1.0, 2.0 * iy) for iy in range(-3, 4) for ix in range(-4, 4)]
    assert count <= len(pts)
    return pts[:count]


def near(p, i):
    return (p[0] + (i % 5 - 2) / 256, p[1] - (i % 7 - 3) / 256)


def weight_scale(S):
    """sqrt of the largest eigenvalue of the symmetric part: how far the weighted distance moves per metre."""
    S = np.asarray(S, np.float64).reshape(2, 2)
    return math.sqrt(max(float(np.linalg.eigvalsh((S + S.T) / 2).max()), 0.0))


def build(name, lms, map_pts, scans, seed, map_cov=None, use=True, max_landmarks=128, fixes=None, scale=1e-3, **tags):
    """lms: the state's reflectors; map_pts / map_cov: the fleet's map; scans: one token list per scan."""
    M_ = len(map_pts)
    map_xy = np.asarray(map_pts, np.float32).reshape(-1, 2)
    assert np.array_equal(map_xy.astype(np.float64), np.asarray(map_pts, np.float64).reshape(-1, 2)), "map points are float32-exact"
    cov = np.tile(np.asarray(IDENTITY), (M_, 1)) if map_cov is None else np.asarray(map_cov, np.float64).reshape(M_, 4)
    L = len(lms)
    mu = np.zeros(3 + 2 * L)
    mu[3:] = np.asarray(lms, np.float64).reshape(-1)
    P = FC.dense_spd(3 + 2 * L, np.random.default_rng(seed), scale)
    events, expect, kept, flags, L_now = [], {}, {}, 0, L
    for k, toks in enumerate(scans):
        cloud, sp, mp, nw, keep = [], [], [], [], []
        for i, tok in enumerate(toks):
            kind, arg = tok[0], tok[1]
            if kind == "m":
                cloud.append(tok[2] if len(tok) > 2 else near(map_pts[arg], i))
                mp.append((i, arg))
                keep.append(i)
            elif kind == "s":
                cloud.append(tok[2] if len(tok) > 2 else near(lms[arg], i))
                sp.append((i, arg))
                keep.append(i)
            else:
                cloud.append(arg)
                if L_now < max_landmarks:
                    nw.append(i)
                    keep.append(i)
                    L_now += 1
                else:
                    flags = FC.FLAG_CAPACITY
        fix = None if fixes is None else fixes[k]
        events.append((EV_SCAN, 50.0 + 0.1 * (k + 1), (0.0, 0.0, 0.0), np.asarray(cloud, np.float32).reshape(-1, 2), fix))
        expect[k] = (sp, mp, nw)
        if len(keep) < len(toks):
            kept[k] = keep
    case = FC._case(name, "map", FC.DIFF if seed % 2 == 0 else FC.OMNI, mu, P, (0.0, 0.0, 0.0), 50.0, events, expect,
                    max_landmarks=max_landmarks, kept=kept, flags=flags, map_xy=map_xy, map_cov=cov, use=use, map_margins={}, **tags)
    return annotate(case)


def map_margins(case, mu_pred, cloud):
    """Per observation (|d1 - 0.05|, d2 - d1) of ReflectorMatch's map branch at the predicted mean, each divided by the weight's
    scale (a distance in metres), and whether the best point is inside the gate.  d1 and d2 are taken over the points whose
    distance is a number: a NaN never wins (nan_cases); (inf, inf, False) where every distance is NaN."""
    from tests.witness.fleet_map_witness import weighted_distances
    out = []
    c, s = math.cos(mu_pred[2]), math.sin(mu_pred[2])
    scales = np.array([weight_scale(S) for S in case.map_cov])
    for p in np.asarray(cloud, np.float32).reshape(-1, 2):
        gx = np.float32(float(p[0]) * c - float(p[1]) * s + mu_pred[0])
        gy = np.float32(float(p[0]) * s + float(p[1]) * c + mu_pred[1])
        dw, _ = weighted_distances(case.map_xy, case.map_cov, gx, gy)
        valid = np.nonzero(~np.isnan(dw))[0]                  # a NaN distance (an indefinite weight) never wins: such a point is
        if valid.shape[0] == 0:                               # skipped, and where every point is one the map decides nothing
            out.append((np.inf, np.inf, False))
            continue
        order = valid[np.argsort(dw[valid], kind="stable")]
        j1 = int(order[0])
        a = abs(dw[j1] - MAP_GATE) / scales[j1]
        b = np.inf
        if order.shape[0] > 1:
            j2 = int(order[1])
            b = (dw[j2] - dw[j1]) / max(scales[j1], scales[j2])
        out.append((float(a), float(b), bool(dw[j1] < MAP_GATE)))
    return out


def annotate(case):
    """case.map_margins[k] and case.margins[k] (the state branch's, fleet_cases.margins) for every scan, from a run of
    oracle/ekf_numpy.py over the reference events."""
    ek = numpy_of(case)
    for k, ev in enumerate(case.events):
        cloud = FC.kept_cloud(case, k)
        mu_p, _ = ek.predict_state(ev[1])
        case.margins[k] = FC.margins(mu_p, cloud)
        case.map_margins[k] = map_margins(case, mu_p, cloud) if case.use else []
        ek.handle_observation(ev[1], cloud, None if ev[4] is None else np.asarray(ev[4]))
    return case


def shuffled(tokens, seed):
    order = np.random.default_rng(seed).permutation(len(tokens))
    return [tokens[i] for i in order]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 129, 2048)
MIXES = ((0, 1, 0), (0, 32, 0), (16, 16, 0), (31, 1, 0), (1, 31, 0), (0, 0, 8), (5, 5, 5))
STD_MAP = 64


def size_cases():
    """Map sizes at the edges of the wave sweep (64 lanes), the matched points at indices 0, 63, 64 and M_ - 1; n = 3."""
    out = []
    for M_ in SIZES:
        ids = sorted({j for j in (0, 63, 64, M_ - 1) if j < M_})
        out.append(build(f"size_M{M_}", [], map_lattice(M_), [[("m", j) for j in ids]], seed=200 + len(out), ids=ids))
    return out


def tie_cases():
    """Two map points at exactly the same weighted distance from the observation g (offsets of 1/64 m, identity weight): the lower
    index wins -- in the same lane a stride later (j, j + 64), in neighbouring lanes, across the first stride's end; and a tie
    outside the gate, which is no map pair."""
    out = []
    g = (0.25, 0.0)

    def tie(name, M_, idx, offs, winner, seed):
        pts = map_lattice(M_)
        for j, o in zip(idx, offs):
            pts[j] = (g[0] + o[0], g[1] + o[1])
        tok = ("m", winner, g) if winner is not None else ("n", g)
        out.append(build(name, [], pts, [[tok]], seed=seed, tie=list(idx)))

    e = 1 / 64
    tie("tie_5_69_same_lane", 129, (5, 69), ((e, 0), (-e, 0)), 5, 211)
    tie("tie_10_11_neighbour_lanes", 129, (10, 11), ((0, e), (e, 0)), 10, 212)
    tie("tie_63_64", 65, (63, 64), ((-e, 0), (0, -e)), 63, 213)
    tie("tie_100_1124_2047", 2048, (100, 1124, 2047), ((e, 0), (0, e), (-e, 0)), 100, 214)
    tie("tie_outside_gate_3_67", 129, (3, 67), ((4 * e, 0), (-4 * e, 0)), None, 215)
    return out


def mix_cases():
    """(n_state, n_map, n_new) on the standard map: each at the smallest state that holds it (n = 3 when n_state = 0: pure
    localisation) and at L = 128, where new observations meet a full member (capacity flag)."""
    out = []
    pts = map_lattice(STD_MAP)
    for q, (ns, nm, nn) in enumerate(MIXES):
        for L in (ns, 128):
            lms = FC.far_lattice(L)
            sid = [(4 * i + i % 3) if L == 128 else i for i in range(ns)]
            mid = [2 * i + (i % 2 if nm < 32 else 0) for i in range(nm)]
            toks = [("s", j) for j in sid] + [("m", j) for j in mid] + [("n", p) for p in new_lattice(nn)]
            out.append(build(f"mix_{ns}_{nm}_{nn}_L{L}", lms, pts, [shuffled(toks, 300 + q)], seed=220 + 2 * q + (L == 128),
                             mix=(ns, nm, nn), L=L))
    return out


def branch_cases():
    """The order of the branches.  Reflector 0 of the state lies 0.25 m from map point 2, reflector 1 0.25 m from map point 5:
    observation 0 is inside both gates (the map wins), observation 1 inside the state gate and 0.125 m from the map point (the
    state), observation 2 outside both: new, with room and without."""
    pts = map_lattice(8)
    lms = [(pts[2][0] + 0.25, pts[2][1]), (pts[5][0] + 0.25, pts[5][1])] + FC.far_lattice(2)
    toks = [("m", 2, (pts[2][0] + 1 / 256, pts[2][1])), ("s", 1, (pts[5][0] + 0.125, pts[5][1])), ("n", new_lattice(1)[0])]
    return [build("branches_room", lms, pts, [toks], seed=240, max_landmarks=6),
            build("branches_full", lms, pts, [toks], seed=241, max_landmarks=4)]


def weight_cases():
    out = []
    # anisotropic: the weighted nearest point (7, at 1/32 m along x) is not the Euclidean nearest (3, at 1/128 m along y, ten
    # times as far in the weight); point 5 has a weight of 1/4: 0.078 m away and inside the gate
    pts = map_lattice(8)
    g = (0.5, 0.25)
    pts[7], pts[3] = (g[0] + 1 / 32, g[1]), (g[0], g[1] + 1 / 128)
    cov = [[1.0, 0.0, 0.0, 100.0]] * 8
    cov[5] = [0.25, 0.0, 0.0, 0.25]
    toks = [("m", 7, g), ("m", 5, (pts[5][0] + 5 / 64, pts[5][1]))]
    out.append(build("weight_anisotropic", [], pts, [toks], seed=250, map_cov=cov))
    # non-symmetric: delta S delta^T = dx^2 + 0.25 dx dy + 2 dy^2; (1/64, 1/64) is inside the gate (0.0282), (1/32, 1/32) outside (0.0563)
    pts = map_lattice(8)
    toks = [("m", 4, (pts[4][0] + 1 / 64, pts[4][1] + 1 / 64)), ("n", (pts[6][0] + 1 / 32, pts[6][1] + 1 / 32))]
    out.append(build("weight_non_symmetric", [], pts, [toks], seed=251, map_cov=[[1.0, 0.5, -0.25, 2.0]] * 8))
    # the gate itself, identity weight: 3/64 = 0.0469 inside, 7/128 = 0.0547 outside
    pts = map_lattice(8)
    toks = [("m", 1, (pts[1][0] + 3 / 64, pts[1][1])), ("n", (pts[6][0], pts[6][1] - 7 / 128))]
    out.append(build("weight_gate", [], pts, [toks], seed=252))
    return out


def fix_cases():
    """A pose fix on a scan with map rows only (5 and 65 rows of the joint system) and with both kinds (67 rows)."""
    pts = map_lattice(STD_MAP)
    out = [build("fix_0_1", [], pts, [[("m", 9)]], seed=260, fixes=[FIX], rows=5),
           build("fix_0_31", [], pts, [[("m", 2 * i) for i in range(31)]], seed=261, fixes=[FIX], rows=65)]
    toks = [("s", i) for i in range(16)] + [("m", 3 * i) for i in range(16)]
    out.append(build("fix_16_16", FC.far_lattice(16), pts, [shuffled(toks, 262)], seed=262, fixes=[FIX], rows=67))
    return out


def unused_case():
    """A member that does not use the map, beside members that do: its five observations next to map points are new reflectors."""
    pts = map_lattice(STD_MAP)
    lms = FC.far_lattice(5)
    toks = [("s", i) for i in range(5)] + [("n", near(pts[2 * i], i)) for i in range(5)] + [("n", p) for p in new_lattice(5)]
    return build("unused_map", lms, pts, [shuffled(toks, 270)], seed=270, use=False)


def two_scan_case():
    """Pure localisation that also maps: scan 0 matches three map points and appends three reflectors, scan 1 sees those three
    again (state rows of reflectors the first scan appended) and two map points."""
    pts = map_lattice(STD_MAP)
    A, B, C = new_lattice(3)
    s0 = [("m", 1), ("n", A), ("m", 4), ("n", B), ("n", C), ("m", 9)]
    s1 = [("s", 0, A), ("m", 4), ("s", 1, B), ("m", 12), ("s", 2, C)]
    return build("two_scans", [], pts, [s0, s1], seed=280)


INDEFINITE = (-1.0, 0.0, 0.0, -1.0)
NAN_PQ = ((0, 1), (5, 69), (5, 37), (70, 3), (64, 0))


def nan_cases():
    """A weighted distance that is NaN: sqrt(e S e^T) with e S e^T < 0 for an indefinite weight S.  The reference's std::sort with
    `<=` is undefined there (cc:414-419); the rule of this project (DESIGN.md, quirk register): a NaN distance never wins, wherever
    it stands; the map pair is the first minimum in index order over the distances that are numbers, if that is < 0.05; if every
    distance is NaN the observation goes on to the state branch.  129 points, identity weights, point p with the weight -I, one
    observation 1/64 m from point q: p in lane p of the wave sweep, q in the same lane a stride later (5, 69), in a lane whose
    result reaches lane 0 through lane p (5, 37), in front of p (70, 3; 64, 0) and right behind index 0 (0, 1).  n = 3 unless stated.
    Every claim is checked against MapWitnessEKF.match3 here."""
    out = []
    e = 1 / 64

    def cov_with(M_, bad):
        cov = [list(IDENTITY) for _ in range(M_)]
        for j, S in bad.items():
            cov[j] = list(S)
        return cov

    for p, q in NAN_PQ:
        pts = map_lattice(129)
        out.append(build(f"nan_p{p}_q{q}", [], pts, [[("m", q, (pts[q][0] + e, pts[q][1]))]], seed=290 + len(out),
                         map_cov=cov_with(129, {p: INDEFINITE}), nan_at=[p]))
    # the nearest point itself is the NaN: the runner-up, 3/64 m away and a stride later in the same lane, is the match
    pts = map_lattice(129)
    g = (0.25, 0.0)
    pts[5], pts[69] = (g[0] + e, g[1]), (g[0] - 3 * e, g[1])
    out.append(build("nan_nearest_5_runner_up_69", [], pts, [[("m", 69, g)]], seed=295, map_cov=cov_with(129, {5: INDEFINITE}), nan_at=[5]))
    # every distance NaN: the state branch decides (a state pair, a new reflector), also for the observation right at a map point
    pts = map_lattice(129)
    lms = FC.far_lattice(2)
    toks = [("s", 0, (lms[0][0] + 1 / 512, lms[0][1])), ("n", (pts[7][0] + e, pts[7][1]))]
    out.append(build("nan_everywhere", lms, pts, [toks], seed=296, map_cov=[list(INDEFINITE)] * 129, nan_at=list(range(129))))
    pts = map_lattice(1)
    out.append(build("nan_M1", [], pts, [[("n", (pts[0][0] + e, pts[0][1]))]], seed=297, map_cov=[list(INDEFINITE)], nan_at=[0]))
    # semi-indefinite: e S e^T = ex^2 - ey^2 / 1024 -- a number (1/64, inside the gate) along x, NaN along y (no pair: new)
    pts = map_lattice(129)
    toks = [("m", 66, (pts[66][0] + e, pts[66][1])), ("n", (pts[66][0], pts[66][1] + e))]
    out.append(build("nan_semi_definite_66", [], pts, [toks], seed=298, map_cov=cov_with(129, {66: (1.0, 0.0, 0.0, -1 / 1024)}), nan_at=[66]))
    for c in out:
        w = map_witness_of(c)
        w.predict(c.events[0][1] - w.time)
        got = w.match3(np.asarray(c.events[0][3], np.float32))
        assert got == tuple(c.expect[0]), (c.name, got, c.expect[0])
    return out


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = (size_cases() + tie_cases() + mix_cases() + branch_cases() + weight_cases() + fix_cases() + [unused_case(), two_scan_case()] +
                  nan_cases())
    return _cases


# ---- the CPU side ------------------------------------------------------------------------------------------------------------
def map_back3(case, k, sp, mp, nw):
    """The three lists of the truncated scan k in the numbering of the scan as submitted."""
    sp, nw = FC.map_back(case, k, sp, nw)
    mp, _ = FC.map_back(case, k, mp, [])
    return sp, mp, nw


def want_lists(case, k):
    sp, mp, nw = case.expect[k]
    return (np.asarray(sp, np.int32).reshape(-1, 2), np.asarray(mp, np.int32).reshape(-1, 2), np.asarray(nw, np.int32).reshape(-1))


def run_references(case, suite=SUITE):
    """fleet_harness.run_references with the map: -> per scan k ([witness state], oracle state, numpy state); the three lists of
    the oracle, ekf_numpy and the witness are checked against the case's claim."""
    o, e, w = oracle_of(case), numpy_of(case), map_witness_of(case)
    out = {}
    for k, ev in enumerate(FC.reference_events(case)):
        for f in (o, e, w):
            FC.feed(f, ev)
        so, mo, no = norm_match(o.last_match())
        lists = {"oracle": (so, mo, no), "numpy": (e.last_match[1], e.last_match[0], e.last_match[2]), "witness": w.last_match}
        for who, got in lists.items():
            got = map_back3(case, k, *got)
            for a, b in zip(got, want_lists(case, k)):
                assert np.array_equal(a, b), (case.name, k, who, [g.tolist() for g in got], case.expect[k])
        L_after = (w.mu.shape[0] - 3) // 2
        assert L_after <= case.max_landmarks, (case.name, k, L_after)
        if k in case.kept:
            assert L_after == case.max_landmarks and case.flags == FC.FLAG_CAPACITY
        out[k] = ([w.state()], o.state(), (e.mu.copy(), e.sigma.copy()))
    o.close()
    return out


# ---- the GPU side ------------------------------------------------------------------------------------------------------------
def check_member(fl, i, case, k, wit, suite=SUITE):
    """fleet_harness.check_member with the map pairs: member i after scan k against the witness; -> the errors as multiples of
    the suite's floor."""
    got = norm_match(fl.last_match(i))
    for a, b, what in zip((got[0], got[1], got[2]), want_lists(case, k), ("state", "map", "new")):
        assert np.array_equal(a, b), (case.name, k, what, a.tolist(), b.tolist())
    mu_ref, P_ref = wit.state()
    st = fl.get_state(i)
    assert st.mu.shape[0] == mu_ref.shape[0] == int(fl.n()[i]), (case.name, k, st.mu.shape, mu_ref.shape)
    assert int(fl.flags()[i]) == case.flags, (case.name, k, int(fl.flags()[i]))
    assert np.array_equal(st.sigma, st.sigma.T), (case.name, k)
    es, em = H.rel_err(st.mu, st.sigma, mu_ref, P_ref)
    bs, bm = H.bounds_within_tolerances(mu_ref, P_ref, suite)
    print(f"  {case.name} scan {k}: sigma {es / suite.floor_sigma:.2f} x the floor, mu {em / suite.floor_mu:.2f} x")
    assert es <= bs, f"{case.name} scan {k}: sigma off by {es:.3e} = {es / suite.floor_sigma:.1f} x the FP64 floor (bound {bs:.3e})"
    assert em <= bm, f"{case.name} scan {k}: mu off by {em:.3e} = {em / suite.floor_mu:.1f} x the FP64 floor (bound {bm:.3e})"
    return es / suite.floor_sigma, em / suite.floor_mu


def map_key(case):
    return (case.map_xy.tobytes(), case.map_cov.tobytes())


def run_lockstep(cases, suite=SUITE):
    """All cases of one capacity as members of ONE fleet.  The fleet has one map, so the cases run group by group (a group = the
    cases built on the same map, users or not): set_map for the group's users, then tick k
    submits event k of every member of the group in one call, and every scan is checked.
    A member that misses a check is recorded and the run goes on, so that one miss does not hide the cases behind it.
    -> the worst (sigma error, where), (mu error, where) of the members that passed, as multiples of the floor, and the misses."""
    worst_s, worst_m, misses = (0.0, ""), (0.0, ""), []
    for cap in sorted({c.max_landmarks for c in cases}):
        members = [c for c in cases if c.max_landmarks == cap]
        fl = H.make_fleet(members, cap)
        wits = [map_witness_of(c) for c in members]
        refs = [FC.reference_events(c) for c in members]
        groups = {}
        for i, c in enumerate(members):
            groups.setdefault(map_key(c), []).append(i)
        try:
            for ids in groups.values():
                first = members[ids[0]]
                fl.set_map(first.map_xy, first.map_cov, members=[i for i in ids if members[i].use])
                assert fl.map_size() == first.map_xy.shape[0]
                for k in range(max(len(members[i].events) for i in ids)):
                    fl.submit([FC.fev(i, members[i].events[k]) for i in ids if k < len(members[i].events)])
                    for i in ids:
                        c = members[i]
                        if k >= len(c.events):
                            continue
                        FC.feed(wits[i], refs[i][k])
                        try:
                            fs, fm = check_member(fl, i, c, k, wits[i], suite)
                        except AssertionError as err:
                            misses.append(str(err))
                            continue
                        worst_s, worst_m = max(worst_s, (fs, f"{c.name} scan {k}")), max(worst_m, (fm, f"{c.name} scan {k}"))
        finally:
            fl.close()
    return worst_s, worst_m, misses


# ---- the session -------------------------------------------------------------------------------------------------------------
SESSION_SCANS = 60
SESSION_MEMBERS = (0, 3, 4, 6)           # of a fleet of 7
_session = None


def session():
    """The golden map session (tests/golden/map_L24_obs8.npz: an 8-point map, 24 reflectors, 8 observations per scan) cut to its
    first SESSION_SCANS scans, as oracle/ekf_oracle.c runs it: -> record (options, map, events, per scan event k (state pairs, map
    pairs, new ids, mu) of the oracle)."""
    global _session
    if _session is not None:
        return _session
    from reflector_ekf_slam_amd import EKFOptions, synth
    from tests.helpers import make_oracle
    g = np.load(os.path.join(H.ROOT, "tests", "golden", "map_L24_obs8.npz"))
    lin, ang, obs = float(g["lin_cov"]), float(g["ang_cov"]), float(g["obs_cov"])
    events, first, scans = [], True, 0
    for e in range(g["ev_type"].shape[0]):
        if g["ev_type"][e] == synth.EV_ODOM:
            events.append((EV_ODOM, float(g["ev_time"][e]), tuple(float(v) for v in g["odom"][e]), None))
        elif first:
            first = False
        else:
            if scans == SESSION_SCANS:
                break
            events.append((EV_SCAN, float(g["ev_time"][e]), (0.0, 0.0, 0.0),
                           np.ascontiguousarray(g["obs"][g["obs_off"][e]: g["obs_off"][e + 1]], np.float32)))
            scans += 1
    o = make_oracle(int(g["odom_model"]), float(g["init_time"]), g["init_pose"], lin, ang, obs)
    o.set_map(g["map_xy"], g["map_cov"])
    records = {}
    for k, ev in enumerate(events):
        FC.feed(o, ev)
        if ev[0] == EV_SCAN:
            records[k] = (*norm_match(o.last_match()), o.mu())
    o.close()
    options = EKFOptions(use_imu=False, init_time=float(g["init_time"]), init_pose=tuple(float(v) for v in g["init_pose"]),
                         odom_model=int(g["odom_model"]), linear_velocity_cov=lin, angular_velocity_cov=ang, observation_cov=obs)
    _session = NS(options=options, map_xy=np.asarray(g["map_xy"], np.float32), map_cov=np.asarray(g["map_cov"], np.float64),
                  events=events, records=records, scans=scans)
    return _session


# ---- the large fleet ---------------------------------------------------------------------------------------------------------
BIG_B, BIG_M = 300, 2048


def big_fleet_cases():
    """300 pure-localisation members on one 2048-point map, one scan each: four map points chosen by the member's index (index 0,
    the last one and the strides' ends among them) and one new observation."""
    pts = map_lattice(BIG_M)
    out = []
    for b in range(BIG_B):
        ids = sorted({(7 * b) % BIG_M, (64 * b + 63) % BIG_M, BIG_M - 1 - b, (b * b) % BIG_M})
        toks = [("m", j) for j in ids] + [("n", new_lattice(1 + b % 5)[b % 5])]
        case = FC._case(f"big_{b}", "map", FC.DIFF, np.zeros(3), FC.dense_spd(3, np.random.default_rng(4000 + b), 1e-3), (0.0, 0.0, 0.0),
                        50.0, [], {}, flags=0, map_xy=None, map_cov=None, use=True, map_margins={})
        cloud = [near(pts[t[1]], i) if t[0] == "m" else t[1] for i, t in enumerate(toks)]
        case.events = [(EV_SCAN, 50.1, (0.0, 0.0, 0.0), np.asarray(cloud, np.float32), None)]
        case.expect = {0: ([], [(i, j) for i, j in enumerate(ids)], [len(ids)])}
        out.append(case)
    xy = np.asarray(pts, np.float32)
    cov = np.tile(np.asarray(IDENTITY), (BIG_M, 1))
    for c in out:
        c.map_xy, c.map_cov = xy, cov
    return out
