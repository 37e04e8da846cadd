"""The shape sweep of the fleet filter's wide scans (k_fleet_step_wide, csrc/fleet_wide.hip), shared by
tests/test_fleet_wide_sweep_cpu.py (the table's claims, the CPU references, the two forms of the witness, the planted defects) and
tests/test_fleet_wide_sweep_gpu.py (the kernel against the longdouble JOINT witness).

tests/fleet_wide_cases.py holds 24 hand-picked shapes; this module enumerates them from tables, as fleet_cases.sweep_shapes does for
the narrow kernels.  One builder (wide_case) gives what neither fleet_cases.sweep_case (MM <= L) nor fleet_map_cases.build (the
origin, no motion) can: a dense SPD state at a random pose that MOVES in Predict (vt != 0, both models), scans of MM matched
observations over L reflectors with MM > L (a reflector seen several times: distinct float32 points a few millimetres apart, mapped
through the PREDICTED pose), NM pairs on the standard 64-point map, N2 new points, all shuffled, an optional fix, and further scans
on the posterior.  The record is the one fleet_wide_cases.on_std_map / fleet_map_cases.build produce.

The plain table (sweep_shapes): every n mod 16 x every class of the LAST block (m_group of MMlast = MM - 32 (blocks - 1)), 2 and 3
blocks in turn, DIFF and OMNI in turn, the classes of the appended rows (N2_CLASSES) in a cycle, one case of 5 blocks, four cases
with a fix (one of them with the heading carried across pi by the blocks, in front of phase P).  The map table (map_shapes): NS in
MAP_NS, each with and without a fix.  two_wide_cases: two wide scans and a narrow one per member, for one launch.

No case is excused from the margin condition: every observation's margins / map_margins under oracle/ekf_numpy.py are at least
MARGIN_MIN (asserted by the builder; the seeds were chosen on the CPU until it held).  numpy only; nothing here needs a GPU.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from tests import fleet_cases as FC
from tests import fleet_map_cases as FM
from tests import fleet_wide_cases as WC

EV_SCAN = FC.EV_SCAN
DIFF, OMNI = FC.DIFF, FC.OMNI
BLOCK = WC.BLOCK
MARGIN_MIN = FC.MARGIN_MIN
GRID, PITCH, JITTER = 12, 2.0, 0.2       # reflectors around EVEN metres, 1.1 m or more from the map's odd metres and 1.6 m from each other
FIX_OFFSET = (0.02, -0.03, 0.01)         # the fix stands this far from the pose the scan was taken at
CAP_SMALL = 48                           # the capacity of the fleet that holds the two capacity classes

# ---- the FP64 noise floor of these cases -------------------------------------------------------------------------------------
# Measured by tests/test_fleet_wide_sweep_cpu.py::test_fp64_floor with fleet_wide_cases.measure_floor: the largest error against the
# longdouble JOINT witness over every scan of every case below of oracle/ekf_oracle.c, oracle/ekf_numpy.py and the BLOCK-form
# witness run in FP64.  Recorded = measured, rounded up to two digits; the test fails when a re-measurement exceeds it or falls below
# half.  The GPU bound is fleet_cases.GPU_FACTOR x these.  fleet_wide_cases.FP64_FLOOR_* are that suite's and do not move.
FP64_FLOOR_SIGMA = 9.6e-11    # measured 9.503e-11 (wsweep_L30_MM69_N34_omni scan 0, oracle)
FP64_FLOOR_MU = 1.5e-14       # measured 1.495e-14 (wsweep_L70_MM33_N1_diff scan 1, block form in FP64)
# block form against joint form, both in longdouble, worst over all_cases(): measured 1.03e-13 (sigma, wsweep_L18_MM79_N33_omni scan 1)
# and 1.9e-17 (mu, wsweep_L33_MM49_N15_diff scan 0); recorded = what the CPU test asserts, about twice and five times the measured
BLOCK_VS_JOINT_SIGMA = 2e-13
BLOCK_VS_JOINT_MU = 1e-16

SUITE = NS(name="wide sweep", floor_sigma=FP64_FLOOR_SIGMA, floor_mu=FP64_FLOOR_MU,
           witnesses={"witness": WC.joint_witness_of, "block": WC.block_witness_of})


# ---- the builder -------------------------------------------------------------------------------------------------------------
def scan(MM=0, NM=0, N2=0, fix=False, see=(), twice=False):
    """One scan's specification: MM observations of the state's reflectors (those of `see` first), NM of map points (`twice`: half
    as many points, each seen twice), N2 new points, a fix or none."""
    return NS(MM=MM, NM=NM, N2=N2, fix=fix, see=tuple(see), twice=twice)


def wrap(a):
    return math.atan2(math.sin(a), math.cos(a))


def wide_case(name, L, scans, model, seed, use=False, max_landmarks=128, heading=None, turn=0.0, fix_offset=FIX_OFFSET, **tags):
    """heading: the PREDICTED heading of scan 0 (the prior's is set so that Predict arrives there); turn: scan 0 was taken at the
    predicted pose turned by this much, so that the update has to carry the heading there; fix_offset: where a fix stands against
    the pose its scan was taken at."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * L
    cells = rng.permutation(GRID * GRID)
    pts = (np.stack([cells % GRID, cells // GRID], -1) - GRID // 2) * PITCH + rng.uniform(-JITTER, JITTER, size=(GRID * GRID, 2))
    pts = pts.astype(np.float32).astype(np.float64)
    free = [p for p in pts[L:]]
    mu = np.zeros(n)
    mu[0:2] = rng.uniform(-1.5, 1.5, size=2)
    mu[2] = rng.uniform(-3.0, 3.0)
    mu[3:] = pts[:L].reshape(-1)
    # fleet_cases.sweep_case's scale (diagonal 3e-4 .. 6e-3) keeps cond(S) in the hundreds for a scan of 32 pairs at most.  The largest
    # eigenvalue of H P H^T grows with the number of rows, so the whole covariance shrinks with the widest scan's pairs (a scalar
    # factor: P stays exactly symmetric): cond(S) of the JOINT system stays in the thousands, and the FP64 floor measures the order of
    # the arithmetic, not one ill-conditioned case.  (Measured without the factor: cond(S) up to 2.4e4, FP64 sigma error 7.6e-10.)
    widest = max(sp.MM + sp.NM for sp in scans)
    P = FC.dense_spd(n, rng, 10.0 ** rng.uniform(-3.7, -2.3)) * min(1.0, BLOCK / max(widest, 1))
    vt = (rng.uniform(0.2, 1.0), rng.uniform(-0.3, 0.3) if model == OMNI else 0.0, rng.uniform(-0.4, 0.4))
    t0, dt = 100.0, 0.1
    if heading is not None:
        mu[2] = heading - vt[2] * dt
    map_xy, map_cov = WC.std_map()
    map_pts = FM.map_lattice(FM.STD_MAP)
    s0 = scans[0]
    case = FC._case(f"{name}_L{L}_MM{s0.MM + s0.NM}_N{s0.N2}_{'diff' if model == DIFF else 'omni'}", name, model, mu, P, vt, t0, [], {},
                    max_landmarks=max_landmarks, flags=0, map_xy=map_xy, map_cov=map_cov, use=use, map_margins={}, L=L, n=n,
                    specs=list(scans), **tags)
    assert s0.NM == 0 or use
    ek = FM.numpy_of(case)
    for k, sp in enumerate(scans):
        t = t0 + dt * (k + 1)
        mu_p = ek.predict_state(t)[0]
        pose = (float(mu_p[0]), float(mu_p[1]), float(mu_p[2]) + (turn if k == 0 else 0.0))
        lm = np.asarray(mu_p[3:], np.float64).reshape(-1, 2)
        Ln = lm.shape[0]
        assert sp.MM == 0 or Ln > 0
        first = [j for j in sp.see]
        order = first + [int(j) for j in rng.permutation(Ln) if int(j) not in first]
        toks = [("s", order[i % Ln], WC.spread(lm[order[i % Ln]], order[i % Ln] + 9 * (i // Ln))) for i in range(sp.MM)]
        morder = rng.permutation(FM.STD_MAP)
        distinct = min(FM.STD_MAP, max(1, (sp.NM + 1) // 2 if sp.twice else sp.NM))
        for i in range(sp.NM):
            j = int(morder[i % distinct])
            toks.append(("m", j, WC.spread(map_pts[j], j + 9 * (i // distinct))))
        if sp.N2:                                        # new points: only cells whose two nearest reflectors are not nearly equidistant
            ok = []
            for p in free:
                d = np.sort(np.hypot(lm[:, 0] - p[0], lm[:, 1] - p[1])) if Ln else np.array([np.inf])
                if d[0] > 1.0 and (Ln < 2 or d[1] - d[0] >= 0.05):
                    ok.append(p)
            assert len(ok) >= sp.N2, (case.name, k, len(ok), sp.N2)
            for p in ok[:sp.N2]:
                toks.append(("n", None, (float(p[0]), float(p[1]))))
            used = {(float(p[0]), float(p[1])) for p in ok[:sp.N2]}
            free = [p for p in free if (float(p[0]), float(p[1])) not in used]
        toks = FM.shuffled(toks, seed + 1000 * (k + 1))
        cloud = np.array([FC.to_local(pose, tok[2]) for tok in toks], np.float32).reshape(-1, 2)
        assert len({row.tobytes() for row in cloud}) == len(toks), (case.name, k, "observations are distinct float32 points")
        spairs, mpairs, new, keep, L_now = [], [], [], [], Ln
        for q, tok in enumerate(toks):
            if tok[0] == "s":
                spairs.append((q, tok[1]))
                keep.append(q)
            elif tok[0] == "m":
                mpairs.append((q, tok[1]))
                keep.append(q)
            elif L_now < max_landmarks:
                new.append(q)
                keep.append(q)
                L_now += 1
            else:
                case.flags = FC.FLAG_CAPACITY
        fix = None
        if sp.fix:
            fix = (pose[0] + fix_offset[0], pose[1] + fix_offset[1], wrap(pose[2] + fix_offset[2]))
        case.events.append((EV_SCAN, t, (0.0, 0.0, 0.0), cloud, fix))
        case.expect[k] = (spairs, mpairs, new)
        if len(keep) < len(toks):
            case.kept[k] = keep
        kept = FC.kept_cloud(case, k)
        case.margins[k] = FC.margins(mu_p, kept)
        case.map_margins[k] = FM.map_margins(case, mu_p, kept) if use else []
        for a, b in case.margins[k]:
            assert a >= MARGIN_MIN and b >= MARGIN_MIN, (case.name, k, a, b)
        for a, b, _inside in case.map_margins[k]:
            assert a >= MARGIN_MIN and b >= MARGIN_MIN, (case.name, k, "map", a, b)
        ek.handle_observation(t, kept, None if fix is None else np.asarray(fix))
    return case


def narrow_behind(case_L, N2_kept, use, cap):
    """The narrow scan behind a wide one, as fleet_cases.sweep_case appends it: one more reflector (on a full member: one matched
    observation), and one map pair for a member on the map -- rows written past n by the wide scan become visible."""
    room = case_L + N2_kept < cap
    return scan(MM=0 if room else 1, N2=1 if room else 0, NM=1 if use else 0)


# ---- the classes -------------------------------------------------------------------------------------------------------------
MMLAST_LISTED = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32)
N2_CLASSES = ("0", "1", "edge", "straddle", "panels3", "over32", "to_capacity", "over_capacity")
MAP_NS = (0, 1, 31, 32, 33, 63, 64, 65)


def m_group(MMlast):
    """(m4 < 8, m4 mod 8, m mod 4, m16) of the last block's m = 2 MMlast rows: phase E's k-steps, phase F's loop with and without its
    tail, the padded fourth row of a k-step, the panel columns rewritten."""
    m = 2 * MMlast
    m4, m16 = (m + 3) & ~3, (m + 15) & ~15
    return (m4 < 8, m4 % 8, m % 4, m16)


def m_groups():
    out = {}
    for v in MMLAST_LISTED:
        out.setdefault(m_group(v), []).append(v)
    return out


def last_block(MM):
    """-> (blocks, MMlast) of MM matched pairs."""
    blocks = (MM + BLOCK - 1) // BLOCK
    return blocks, MM - BLOCK * (blocks - 1)


def n2_classes(L, N2, cap):
    """Every class of N2_CLASSES that a scan of N2 new observations on L reflectors holds (N2: as submitted)."""
    n = 3 + 2 * L
    n16 = (n + 15) & ~15
    kept = min(N2, cap - L)
    na = n + 2 * kept
    out = {"0"} if N2 == 0 else {"1"} if N2 == 1 else set()
    if kept >= 1 and na == n16 - 1:
        out.add("edge")
    if na == n16 + 1:
        out.add("straddle")
    if sum(1 for e in range(n16, na, 16)) >= 3:
        out.add("panels3")
    if kept > 32:
        out.add("over32")
    if N2 >= 1 and L + N2 == cap:
        out.add("to_capacity")
    if L + N2 > cap:
        out.add("over_capacity")
    return out


def n2_for(L, cls, q):
    """-> (N2 as submitted, capacity) that puts a scan on L reflectors into class `cls`, or None where n forbids it."""
    n = 3 + 2 * L
    e = ((n + 15) & ~15) - n                     # odd, 1 .. 15
    cap = CAP_SMALL if cls in ("to_capacity", "over_capacity") else 128
    if cls in ("to_capacity", "over_capacity") and L >= CAP_SMALL - 1:
        return None
    N2 = {"0": 0, "1": 1, "edge": (e - 1) // 2, "straddle": (e + 1) // 2, "panels3": (e + 1) // 2 + 16, "over32": 33 + q % 3,
          "to_capacity": CAP_SMALL - L, "over_capacity": CAP_SMALL - L + 3}[cls]
    if cls not in n2_classes(L, N2, cap):
        return None
    return N2, cap


# ---- the plain table ---------------------------------------------------------------------------------------------------------
def sweep_shapes():
    """One record (L, MM, N2, cls, cap, model) per plain case: every n mod 16 x every group of the last block, 2 and 3 blocks in
    turn, the N2 classes in a cycle, DIFF and OMNI in turn; and one case of 5 blocks at n = 29."""
    shapes = []
    groups = sorted(m_groups().items())
    q = 0
    for k in range(8):                                   # L mod 8 <-> n mod 16
        for gi, (_grp, lasts) in enumerate(groups):
            MMlast = lasts[(k + gi) % len(lasts)]
            blocks = 2 + (k + gi) % 2
            for tries in range(len(N2_CLASSES)):
                cls = N2_CLASSES[(q + tries) % len(N2_CLASSES)]
                hi = CAP_SMALL - 2 if cls in ("to_capacity", "over_capacity") else 80
                cand = [L for L in range(6, hi + 1) if L % 8 == k]
                L = cand[(k * 3 + gi * 5) % len(cand)]
                got = n2_for(L, cls, q)
                if got is not None:
                    break
            else:
                raise AssertionError((k, gi))
            shapes.append(NS(L=L, MM=BLOCK * (blocks - 1) + MMlast, N2=got[0], cls=cls, cap=got[1], model=DIFF if q % 2 == 0 else OMNI))
            q += 1
    shapes.append(NS(L=13, MM=4 * BLOCK + 7, N2=2, cls="straddle", cap=128, model=DIFF))
    return shapes


# seeds: 9800 + the shape's index (+ what SEED_BUMP lists: chosen on the CPU until every margin held)
SEED_BUMP = {("map", 2, False): 7, ("map", 4, False): 7, ("map", 5, False): 28, ("map", 5, True): 14}
FIXED_PLAIN = (5, 31, 58, 83)            # the shapes of the plain table that run once more with a fix; the last one across pi


def plain_case(i, s, fix=False, **kw):
    kept = min(s.N2, s.cap - s.L)
    seed = 9800 + i + (400 if fix else 0) + SEED_BUMP.get((i, fix), 0)
    return wide_case("wsweepfix" if fix else "wsweep", s.L, [scan(MM=s.MM, N2=s.N2, fix=fix), narrow_behind(s.L, kept, False, s.cap)], s.model,
                     seed, max_landmarks=s.cap, cls=s.cls, MM=s.MM, N2=s.N2, NSn=s.MM, fixed=fix, **kw)


# ---- the map table -----------------------------------------------------------------------------------------------------------
def map_shapes():
    """(NS, NM, L, N2, twice): MM = NS + NM makes two or three blocks with a last block of MMLAST_LISTED; L covers all eight
    residues; NS > L means reflectors seen several times."""
    return [NS(NSn=0, NM=34, L=7, N2=0, twice=False), NS(NSn=1, NM=40, L=8, N2=2, twice=True), NS(NSn=31, NM=36, L=9, N2=1, twice=False),
            NS(NSn=32, NM=17, L=10, N2=3, twice=False), NS(NSn=33, NM=24, L=20, N2=0, twice=True), NS(NSn=63, NM=6, L=21, N2=2, twice=False),
            NS(NSn=64, NM=15, L=38, N2=1, twice=False), NS(NSn=65, NM=30, L=43, N2=4, twice=True)]


def map_case(i, s, fix):
    seed = 10300 + 2 * i + int(fix) + SEED_BUMP.get(("map", i, fix), 0)
    return wide_case("wmapfix" if fix else "wmap", s.L, [scan(MM=s.NSn, NM=s.NM, N2=s.N2, fix=fix, twice=s.twice), narrow_behind(s.L, s.N2, True, 128)],
                     OMNI if i % 2 else DIFF, seed, use=True, cls="map", MM=s.NSn + s.NM, N2=s.N2, NSn=s.NSn, fixed=fix)


# ---- two wide scans of one member --------------------------------------------------------------------------------------------
def two_wide_cases():
    """Three members at n mod 16 = 15, 1 and 9.  Scan 0 matches 40 observations (reflectors seen several times) and appends across
    a panel edge (straddle, panels3, panels3); scan 1 matches the appended reflectors among others, 36 to 44 observations, and
    appends again; a narrow scan follows.  The third member is on the map and has a fix on its second scan."""
    out = []
    for q, (L, N2a, use) in enumerate(((14, 1, False), (7, 24, False), (11, 20, True))):
        n = 3 + 2 * L
        assert n % 16 == (15, 1, 9)[q] and ("straddle" if q == 0 else "panels3") in n2_classes(L, N2a, 128)
        new_ids = range(L, L + N2a)
        s0 = scan(MM=40 - (6 if use else 0), NM=6 if use else 0, N2=N2a)
        s1 = scan(MM=36 + 4 * q - (5 if use else 0), NM=5 if use else 0, N2=3 + q, see=new_ids, fix=use)
        s2 = scan(MM=3, N2=1, NM=1 if use else 0)
        out.append(wide_case("wtwo", L, [s0, s1, s2], OMNI if q % 2 else DIFF, 10400 + q + SEED_BUMP.get(("two", q), 0), use=use, cls="two",
                             MM=40, N2=N2a, NSn=s0.MM, fixed=False))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
_sweep = _two = None


def sweep_cases():
    """The plain table, its four cases with a fix, and the map table with and without a fix."""
    global _sweep
    if _sweep is None:
        shapes = sweep_shapes()
        out = [plain_case(i, s) for i, s in enumerate(shapes)]
        for j, i in enumerate(FIXED_PLAIN):
            kw = dict(heading=math.pi - 5e-4, turn=1.5e-3) if j == len(FIXED_PLAIN) - 1 else {}
            out.append(plain_case(i, shapes[i], fix=True, **kw))
        for i, s in enumerate(map_shapes()):
            out += [map_case(i, s, False), map_case(i, s, True)]
        assert len({c.name for c in out}) == len(out)
        _sweep = out
    return _sweep


def all_cases():
    global _two
    if _two is None:
        _two = two_wide_cases()
    return sweep_cases() + _two


def track_members():
    """Eight sweep members, one per n mod 16, for the track test: two on the map, two with a fix among them."""
    out, seen = [], set()
    quota = [lambda c: c.fixed and c.use, lambda c: c.fixed and c.use, lambda c: c.fixed and not c.use, lambda c: c.use and not c.fixed,
             lambda c: c.use and not c.fixed, lambda c: c.cls == "over32", lambda c: c.cls == "panels3", lambda c: True]
    for want in quota:
        for c in sweep_cases():
            if c.n % 16 not in seen and c.max_landmarks == 128 and want(c):
                out.append(c)
                seen.add(c.n % 16)
                break
    assert len(out) == 8 and len(seen) == 8, sorted(seen)
    return out


# ---- the CPU side ------------------------------------------------------------------------------------------------------------
_runs = None


def runs():
    """fleet_wide_cases.runs over all_cases(): name -> per scan k ([joint witness state, block witness state], oracle state, numpy
    state, FP64 block-form state), computed once; every reference's association lists are checked against the case's claim."""
    global _runs
    if _runs is not None:
        return _runs
    from tests.witness.fleet_wide_witness import F64Kit
    _runs = {}
    for c in all_cases():
        base = FM.run_references(c, SUITE)
        wb, w64 = WC.block_witness_of(c), WC.block_witness_of(c, F64Kit())
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
