"""Cases of the fleet filter's wide scans (rfleet_set_wide_scans: 32 < K <= 256 observations, applied in exact block steps of 32
pairs by k_fleet_step_wide), shared by tests/test_fleet_wide_cpu.py (the cases, the CPU references and the two forms of the witness
against each other) and tests/test_fleet_wide_gpu.py (the kernel against the longdouble JOINT witness).

Built on tests/fleet_cases.py and tests/fleet_map_cases.py: a case is their record -- a dense SPD state to write with ``set_state``,
events, ``map_xy`` / ``map_cov`` / ``use`` and per scan the claimed lists ``expect[k] = (state_pairs, map_pairs, new_ids)``.  Every
case carries the SAME 64-point map, so that all of them are members of one fleet; ``use`` says whether the member matches against it.
The shapes are the smallest at which the block loop, the lists and the record can go wrong; exactly one case has MM = 256.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as FM

EV_ODOM, EV_SCAN = FC.EV_ODOM, FC.EV_SCAN
BLOCK = 32
STD_MAP = FM.STD_MAP
FIX = FM.FIX

# ---- the FP64 noise floor of these cases -------------------------------------------------------------------------------------
# Measured by tests/test_fleet_wide_cpu.py::test_fp64_floor as the other fleet suites do: the largest error against the longdouble
# JOINT witness over every scan of every case below of oracle/ekf_oracle.c and oracle/ekf_numpy.py (joint form, FP64) and of the
# BLOCK-form witness run in FP64 (tests/witness/fleet_wide_witness.F64Kit: the block order's own round-off).  Recorded = measured,
# rounded up to two digits; the test fails when a re-measurement exceeds it or falls below half.  The GPU bound is GPU_FACTOR x these.
FP64_FLOOR_SIGMA = 3.9e-12    # measured 3.83e-12 (wide1_L77_MM31_N9_omni scan 0, oracle)
FP64_FLOOR_MU = 3.6e-15       # measured 3.559e-15 (wide_tall_L1_MM40 scan 0, block form in FP64)


def joint_witness_of(case):
    return FM.map_witness_of(case)


def block_witness_of(case, kit=None):
    from tests.witness.fleet_wide_witness import BlockWitnessEKF
    from tests.witness.fleet_witness import LDKIT
    w = BlockWitnessEKF(case.model, case.t, case.mu[:3], FC.LIN_COV, FC.ANG_COV, FC.OBS_COV, kit=kit or LDKIT)
    w.set_state(case.t, case.mu, case.P, case.vt)
    if case.use:
        w.set_map(case.map_xy, case.map_cov)
    return w


SUITE = NS(name="wide", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU, witnesses={"witness": joint_witness_of, "block": block_witness_of})


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def std_map():
    pts = FM.map_lattice(STD_MAP)
    return np.asarray(pts, np.float32).reshape(-1, 2), np.tile(np.asarray(FM.IDENTITY), (STD_MAP, 1))


def on_std_map(case, use):
    """Gives a fleet_cases case the record of a map case: the standard map, the switch, three lists per scan."""
    case.map_xy, case.map_cov = std_map()
    case.use, case.map_margins = use, {}
    case.flags = getattr(case, "flags", 0)
    case.expect = {k: (sp, [], nw) for k, (sp, nw) in case.expect.items()}
    case.events = [(*ev[:4], None) for ev in case.events]
    return case


def sweep(L, MM, N2, model, seed, name):
    """fleet_cases.sweep_case (a dense SPD state at a random pose, one scan of MM matched and N2 new observations in random order,
    then a narrow scan on the posterior) as a member that does not use the map."""
    return on_std_map(FC.sweep_case(L, MM, N2, model, seed, name=name), False)


def built(name, lms, scans, seed, use, **kw):
    """fleet_map_cases.build on the standard map (pose at the origin: sensor frame == global frame, float32-exact points)."""
    return FM.build(name, lms, FM.map_lattice(STD_MAP), scans, seed, use=use, **kw)


def spread(p, i):
    """Observation i of a reflector seen many times: 64 distinct float32-exact points within 0.02 m of p."""
    return (p[0] + (i % 8 - 4) / 256, p[1] + ((i // 8) % 8 - 4) / 256)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def boundary_cases():
    """MM at the block boundaries on n = 259, DIFF and OMNI in turn; and MM = 256: every reflector of a full member seen twice
    (ReflectorMatch has no mutual exclusion), eight full blocks."""
    out = [sweep(128, MM, 0, FC.DIFF if i % 2 == 0 else FC.OMNI, 9700 + i, "wide") for i, MM in enumerate((33, 63, 64, 65, 96, 97))]
    lms = FC.far_lattice(128)
    toks = FM.shuffled([("s", j, spread(lms[j], j + 3 * r)) for j in range(128) for r in range(2)], 9710)
    out.append(built("wide_L128_MM256_twice", lms, [toks], 9710, False, MM=256))
    return out


def one_block_cases():
    """K > 32 but one block: K = 33 with MM = 32 and one new; K = 40 with MM = 31 and nine new."""
    return [sweep(60, 32, 1, FC.DIFF, 9720, "wide1"), sweep(77, 31, 9, FC.OMNI, 9721, "wide1")]


def tall_cases():
    """m larger than n: 40 observations of one reflector (n = 5) and of two in turn (n = 7); two blocks of 64 and 16 rows."""
    out = []
    for L in (1, 2):
        lms = FC.far_lattice(L)
        toks = [("s", i % L, spread(lms[i % L], i)) for i in range(40)]
        out.append(built(f"wide_tall_L{L}_MM40", lms, [toks], 9730 + L, False))
    return out


def augment_cases():
    far = FC.far_lattice(160)
    out = [built("wide_new100_from_n3", [], [[("n", p) for p in far[:100]]], 9740, False),
           sweep(60, 33, 33, FC.DIFF, 9741, "wideaug"),
           built("wide_new140_capacity", [], [[("n", p) for p in far[:140]]], 9742, False),
           built("wide_new40_room1", far[:10], [[("n", p) for p in far[100:140]]], 9743, False, max_landmarks=11)]
    assert out[2].flags == FC.FLAG_CAPACITY and len(out[2].expect[0][2]) == 128
    assert out[3].flags == FC.FLAG_CAPACITY and len(out[3].expect[0][2]) == 1
    return out


def map_member_cases():
    """Members on the map.  NS = 20 with 20 map pairs: block 0 mixed, block 1 map rows only; NS = 32 and 33: the first map row is
    row 0 of block 1 and row 2 of block 1; map pairs only (pure localisation, n stays 3)."""
    out = []
    for q, (ns, nm) in enumerate(((20, 20), (32, 8), (33, 7))):
        toks = [("s", j) for j in range(ns)] + [("m", (3 * j) % STD_MAP) for j in range(nm)]
        out.append(built(f"wide_map_NS{ns}_NM{nm}", FC.far_lattice(ns + 2), [FM.shuffled(toks, 9750 + q)], 9750 + q, True))
    pts = FM.map_lattice(STD_MAP)
    toks = [("m", j, spread(pts[j], j)) for j in range(40)]
    out.append(built("wide_map_only_MM40", [], [toks], 9754, True))
    return out


def fix_cases():
    """A pose fix on a wide scan: phase P behind the last block (plain member, MM = 33 and 65), in front of the first with every
    block corrected (a member on the map, MM = 40), and on a wide scan without a match (ignored)."""
    out = []
    for q, MM in enumerate((33, 65)):
        lms = FC.far_lattice(MM + 5)
        out.append(built(f"wide_fix_plain_MM{MM}", lms, [[("s", j) for j in range(MM)]], 9760 + q, False, fixes=[FIX]))
    toks = [("s", j) for j in range(20)] + [("m", 2 * j) for j in range(20)]
    out.append(built("wide_fix_map_MM40", FC.far_lattice(24), [FM.shuffled(toks, 9763)], 9763, True, fixes=[FIX]))
    out.append(built("wide_fix_unmatched_K40", [], [[("n", p) for p in FC.far_lattice(40)]], 9764, False, fixes=[FIX]))
    return out


def heading_case():
    """The heading 5e-4 short of pi, the robot really 1e-3 beyond it: block 0 of two carries the mean across pi, so a wrap between
    the blocks would make the second block's correction see a jump of 2 pi."""
    rng = np.random.default_rng(9770)
    L, MM = 48, 40
    lms = np.asarray(FC.far_lattice(L), np.float64) + 8.0
    n = 3 + 2 * L
    mu = np.zeros(n)
    mu[0:3] = (8.0, 8.0, math.pi - 5e-4)
    mu[3:] = lms.reshape(-1)
    A = rng.normal(size=(n, n))
    P = (A @ A.T) * (1e-5 / n) + np.diag([1e-3, 1e-3, 1e-3] + [1e-4] * (2 * L))
    P = np.tril(P) + np.tril(P, -1).T
    true = (8.0, 8.0, -math.pi + 1e-3)
    cloud = np.array([FC.to_local(true, lms[j]) for j in range(MM)], np.float32)
    case = FC._case("wide_heading_across_pi", "crafted", FC.DIFF, mu, P, (0.0, 0.0, 0.0), 70.0, [(EV_SCAN, 70.1, (0.0, 0.0, 0.0), cloud)],
                    {0: ([(i, i) for i in range(MM)], [])})
    return on_std_map(FC.annotate(case), False)


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = boundary_cases() + one_block_cases() + tall_cases() + augment_cases() + map_member_cases() + fix_cases() + [heading_case()]
        assert len({c.name for c in _cases}) == len(_cases)
        assert sum(len(c.expect[0][0]) + len(c.expect[0][1]) == 256 for c in _cases) == 1
    return _cases


def counts(case, k=0):
    sp, mp, nw = case.expect[k]
    return len(sp), len(mp), len(nw)


# ---- the CPU side ------------------------------------------------------------------------------------------------------------
_runs = None


def runs():
    """name -> per scan k ([joint witness state, block witness state], oracle state, numpy state, FP64 block-form state): computed
    once and shared by the CPU tests.  The association lists of every reference are checked against the case's claim."""
    global _runs
    if _runs is not None:
        return _runs
    from tests.witness.fleet_wide_witness import F64Kit
    _runs = {}
    for c in all_cases():
        base = FM.run_references(c, SUITE)                       # oracle, numpy, joint witness: lists checked there
        wb, w64 = block_witness_of(c), block_witness_of(c, F64Kit())
        out = {}
        for k, ev in enumerate(FC.reference_events(c)):
            for w in (wb, w64):
                FC.feed(w, ev)
                got = FM.map_back3(c, k, *w.last_match)
                for a, b in zip(got, FM.want_lists(c, k)):
                    assert np.array_equal(a, b), (c.name, k, "block witness")
            (wj,), orc, npy = base[k]
            out[k] = ([wj, wb.state()], orc, npy, w64.state())
        _runs[c.name] = out
    return _runs


def measure_floor(cases, all_runs, suite=SUITE):
    """fleet_harness.measure_floor with a third FP64 reference, the block-form witness in FP64: the largest error against the joint
    longdouble witness must be the recorded floor (not above it, not below half of it), and the GPU bound it sets is nowhere
    looser than the absolute tolerances."""
    ws, wm = (0.0, ""), (0.0, "")
    for c in cases:
        for k, (wits, orc, npy, b64) in all_runs[c.name].items():
            for who, (mu, P) in (("oracle", orc), ("numpy", npy), ("block fp64", b64)):
                es, em = H.rel_err(mu, P, *wits[0])
                ws, wm = max(ws, (es, f"{c.name} scan {k} ({who})")), max(wm, (em, f"{c.name} scan {k} ({who})"))
            H.bounds_within_tolerances(*wits[0], suite)
    print(f"\nFP64 floor over {len(cases)} {suite.name} cases: sigma {ws[0]:.3e} at {ws[1]}; mu {wm[0]:.3e} at {wm[1]}")
    print(f"recorded: sigma {suite.floor_sigma:.3e}, mu {suite.floor_mu:.3e}")
    assert ws[0] <= suite.floor_sigma and wm[0] <= suite.floor_mu
    assert ws[0] >= suite.floor_sigma / 2 and wm[0] >= suite.floor_mu / 2, "the recorded floor is stale: far above what is measured"
    return ws, wm


# ---- the GPU side ------------------------------------------------------------------------------------------------------------
def make_fleet(cases, max_landmarks=128, wide=True, with_map=True, track=False):
    fl = H.fleet_mod().ReflectorEKFSLAMFleet([FC.options_of(c) for c in cases], max_landmarks=max_landmarks, wide_scans=wide)
    for i, c in enumerate(cases):
        fl.set_state(i, c.t, c.mu, c.P, c.vt)
    if with_map:
        fl.set_map(*std_map(), members=[i for i, c in enumerate(cases) if c.use])
    if track:
        fl.track(True)
    return fl


def run_lockstep(cases, suite=SUITE):
    """All cases of one capacity as members of ONE wide-enabled fleet on the standard map; tick k submits event k of every member
    in one call (a wide launch when any of them is wide) and every scan is checked against the JOINT witness.  A miss is recorded
    and the run goes on.  -> the worst (sigma error, where), (mu error, where) as multiples of the floor, and the misses."""
    worst_s, worst_m, misses = (0.0, ""), (0.0, ""), []
    for cap in sorted({c.max_landmarks for c in cases}):
        members = [c for c in cases if c.max_landmarks == cap]
        fl = make_fleet(members, cap)
        wits = [joint_witness_of(c) for c in members]
        refs = [FC.reference_events(c) for c in members]
        try:
            for k in range(max(len(c.events) for c in members)):
                fl.submit([FC.fev(i, c.events[k]) for i, c in enumerate(members) if k < len(c.events)])
                for i, c in enumerate(members):
                    if k >= len(c.events):
                        continue
                    FC.feed(wits[i], refs[i][k])
                    try:
                        fs, fm = FM.check_member(fl, i, c, k, wits[i], suite)
                    except AssertionError as err:
                        misses.append(str(err))
                        continue
                    worst_s, worst_m = max(worst_s, (fs, f"{c.name} scan {k}")), max(worst_m, (fm, f"{c.name} scan {k}"))
        finally:
            fl.close()
    return worst_s, worst_m, misses
