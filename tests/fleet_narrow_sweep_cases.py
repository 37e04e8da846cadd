"""The shape sweep of the fleet filter's three other narrow compiles -- k_fleet_step_fix, k_fleet_step_map and k_fleet_step_track
(csrc/fleet_kernels.hip: one body, four compiles, each with its own register allocation, its own LDS layout and code the others
drop) -- shared by tests/test_fleet_narrow_sweep_cpu.py (the tables' claims, the margins, the CPU references, the floors, six
planted defects) and tests/test_fleet_narrow_sweep_gpu.py (the kernels against the longdouble witnesses, and bit for bit against
each other).  k_fleet_step has fleet_cases.sweep_shapes; what the other three had is listed in DESIGN.md 10.

The fix table (fix_cases): members of a fleet WITHOUT a map, every scan with a fix, so that every submit takes k_fleet_step_fix.
Every n mod 16 x every class of fleet_cases.M_CLASSES, the classes of the appended rows in a cycle, built by
fleet_cases.sweep_case and fleet_pose_cases.attach_fixes: scan 0 carries a fix behind phases C-F, the follow-up scan appends one
reflector, matches nothing and carries a fix that has to be ignored (on a full member, n = 259, it matches one reflector and the fix
counts).  Four more shapes have the predicted heading 5e-4 short of +-pi, the scan taken 1.5e-3 beyond it and the fix's yaw 1e-2
beyond that: phases C-F carry the heading across pi in front of phase P.

The map table (map_cases): members on fleet_wide_cases.std_map(), built by fleet_wide_sweep_cases.wide_case with narrow scans -- a
random pose that MOVES in Predict, both models, shuffled tokens, NS state pairs, NM map pairs and N2 new points, a fix at
FIX_OFFSET from the pose for about half of the shapes (fix_first: phase P in front of phase C, rows at s_mu0, the innovations
corrected) -- then pure localisation that moves (L = 0) and one member per residue that does not use the map.

No case is excused from the margin condition (every margin of every scan >= MARGIN_MIN, asserted by the builders and again by the
CPU test; SEED_BUMP lists the seeds that had to move).  numpy only; nothing here needs a GPU.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

from tests import fleet_cases as FC
from tests import fleet_harness as H
from tests import fleet_map_cases as FM
from tests import fleet_pose_cases as PC
from tests import fleet_wide_sweep_cases as SC

DIFF, OMNI = FC.DIFF, FC.OMNI
MARGIN_MIN = FC.MARGIN_MIN
N_MAX = 163                                  # no state is larger, but for the named exceptions at n = 257 and n = 259
RESIDUES = (1, 3, 5, 7, 9, 11, 13, 15)
N2_CYCLE = ("0", "1", "inside", "edge", "straddle", "cross")

# ---- the FP64 noise floors of these cases ------------------------------------------------------------------------------------
# Measured by tests/test_fleet_narrow_sweep_cpu.py::test_fp64_floors as every fleet suite does (fleet_harness.measure_floor): the
# larger error of oracle/ekf_oracle.c and oracle/ekf_numpy.py against the suite's longdouble witness over every scan of its cases.
# Recorded = measured, rounded up to two digits; the test fails when a re-measurement exceeds it or falls below half.  The GPU bound
# is fleet_cases.GPU_FACTOR x these.  The floors of fleet_cases, fleet_pose_cases, fleet_map_cases and the wide suites do not move.
FIX_FLOOR_SIGMA = 1.4e-11     # measured 1.318e-11 (nfix_L42_MM23_N3_diff_fix scan 1, numpy)
FIX_FLOOR_MU = 1.4e-16        # measured 1.334e-16 (nfix_L128_MM32_N0_omni_fix scan 1, numpy)
MAP_FLOOR_SIGMA = 1.2e-11     # measured 1.116e-11 (nplainfix_L36_MM31_N1_omni scan 0, numpy)
MAP_FLOOR_MU = 1.9e-15        # measured 1.839e-15 (nmap_L41_MM17_N1_omni scan 1, numpy)

FIX_SUITE = NS(name="narrow sweep, fix", floor_sigma=FIX_FLOOR_SIGMA, floor_mu=FIX_FLOOR_MU, witnesses={"witness": PC.pose_witness_of})
MAP_SUITE = NS(name="narrow sweep, map", floor_sigma=MAP_FLOOR_SIGMA, floor_mu=MAP_FLOOR_MU, witnesses={"witness": FM.map_witness_of})


# ---- the fix table -----------------------------------------------------------------------------------------------------------
FIX_LARGE = {(7, 3): 127, (0, 3): 128}       # (L mod 8, index of the M class) -> L: the shapes kept at n = 257 (MM = 31) and n = 259 (32)


def fix_shapes():
    """(L, MM, N2, model) as fleet_cases.sweep_shapes enumerates them: every n mod 16 x every class of fleet_cases.M_CLASSES, the
    class of the appended rows in a cycle (the next class where n, the 32 observations or the capacity forbid one), DIFF and OMNI
    in turn, n <= N_MAX but for FIX_LARGE."""
    shapes, seen = [], set()
    q = 0
    for k in range(8):                                   # L mod 8 <-> n mod 16
        Ls = [L for L in range(k if k else 8, (N_MAX - 3) // 2 + 1, 8)]
        for ci, (cls, mms) in enumerate(sorted(FC.M_CLASSES.items(), key=str)):
            MM = mms[(k + ci) % len(mms)]
            cand = [L for L in Ls if L >= MM]
            L = FIX_LARGE.get((k, ci), cand[(k * 3 + ci * 5) % len(cand)])
            for tries in range(6):
                N2 = FC.n2_for(3 + 2 * L, N2_CYCLE[(q + tries) % 6], MM)
                if N2 is not None and (L, MM, N2) not in seen:
                    break
            else:
                raise AssertionError((L, MM))
            seen.add((L, MM, N2))
            shapes.append((L, MM, N2, DIFF if len(shapes) % 2 == 0 else OMNI))
            q += 1
    return shapes


# (L, MM, N2, model, sign): the predicted heading is sign (pi - 5e-4), the scan was taken 1.5e-3 further on (beyond pi), the fix's yaw
# stands 1e-2 beyond that.  n mod 16 = 5, 9, 13, 15: fleet_pose_cases.heading_fix_cases stand at n = 35 (3).
HEADING_SHAPES = ((9, 6, 3, DIFF, 1.0), (19, 15, 4, OMNI, -1.0), (29, 17, 0, DIFF, -1.0), (38, 32, 0, OMNI, 1.0))
HEADING_SHORT, HEADING_TURN, HEADING_FIX = 5e-4, 1.5e-3, 1e-2


def as_plain(case):
    """A fleet_wide_sweep_cases.wide_case record of a member without a map as fleet_cases' record: two lists per scan."""
    assert not case.use and all(len(mp) == 0 for _sp, mp, _nw in case.expect.values())
    case.expect = {k: (sp, nw) for k, (sp, _mp, nw) in case.expect.items()}
    return case


def heading_case(i, L, MM, N2, model, sign):
    off = (SC.FIX_OFFSET[0], SC.FIX_OFFSET[1], sign * HEADING_FIX)
    kept = min(N2, 128 - L)
    c = SC.wide_case("nfixpi", L, [SC.scan(MM=MM, N2=N2, fix=True), SC.scan(MM=0, N2=1, fix=True)], model, 11900 + i + SEED_BUMP.get(("pi", i), 0),
                     heading=sign * (math.pi - HEADING_SHORT), turn=sign * HEADING_TURN, fix_offset=off, cls="heading", MM=MM, N2=N2, sign=sign)
    assert kept == N2
    return as_plain(c)


# ---- the map table -----------------------------------------------------------------------------------------------------------
MAP_NS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31)
MAP_N2_CYCLE = ("0", "1", "edge", "straddle", "cross")
MAP_PER_NS = 5                               # shapes per NS; 11 and 8 are coprime, so each meets five different residues
MAP_LARGE = {16: False, 32: True}            # the two shapes kept at n = 259 (L = 128, NS = 8 and 31) -> the one variant each runs in
LOCALISE_NM = (1, 31, 32)


def boundary_positions(ns):
    """Where the first map row 2 NS stands: (inside a group of 4 rows, inside a tile of 16 rows) as the offsets 2 NS mod 4 and
    2 NS mod 16, and the tile."""
    return (2 * ns) % 4, (2 * ns) % 16, (2 * ns) // 16


def map_shapes():
    """One record (L, NSn, NM, N2, cls, model, variants) per shape of the members on the map: NS runs over MAP_NS and n mod 16 over all
    residues together (shape i: MAP_NS[i mod 11], L mod 8 = i mod 8); NS + NM runs over the classes of fleet_cases.M_CLASSES in a
    cycle (the next class that holds a count above NS: every member has a map pair); N2 over MAP_N2_CYCLE; every second shape runs
    once more with a fix (`variants`)."""
    classes = sorted(FC.M_CLASSES.items(), key=str)
    shapes = []
    for i in range(MAP_PER_NS * len(MAP_NS)):
        ns, k = MAP_NS[i % len(MAP_NS)], i % 8
        for tries in range(len(classes)):
            mms = [v for v in classes[(i + tries) % len(classes)][1] if v > ns]
            if mms:
                break
        MMt = mms[i % len(mms)]
        cand = [L for L in range(k if k else 8, (N_MAX - 3) // 2 + 1, 8) if L >= max(ns, 1)]
        L = 128 if i in MAP_LARGE else cand[(i * 3) % len(cand)]
        assert L % 8 == k
        for tries in range(len(MAP_N2_CYCLE)):
            cls = MAP_N2_CYCLE[(i + tries) % len(MAP_N2_CYCLE)]
            N2 = FC.n2_for(3 + 2 * L, cls, MMt)
            if N2 is not None:
                break
        else:
            raise AssertionError((L, MMt))
        variants = (MAP_LARGE[i],) if i in MAP_LARGE else (False, True) if i % 2 == 0 else (False,)
        shapes.append(NS(L=L, NSn=ns, NM=MMt - ns, N2=N2, cls=cls, model=DIFF if i % 2 == 0 else OMNI, variants=variants))
    return shapes


# (L, MM, N2, fix) of the members that do not use the map, one per residue: plain members under k_fleet_step_map, four with a fix
# (phase P behind phase F in the map compile)
UNUSED_SHAPES = ((7, 5, 1, False), (16, 9, 2, True), (9, 1, 3, False), (26, 17, 4, True), (11, 8, 0, False), (36, 31, 1, True),
                 (45, 25, 2, False), (38, 32, 0, True))

# seeds: the table's base + the shape's index (+ what SEED_BUMP lists: moved on the CPU until every margin held)
SEED_BUMP = {("map", 12, False): 7, ("map", 16, False): 7, ("map", 19, False): 7, ("map", 22, False): 7, ("map", 30, True): 7, ("map", 34, True): 7,
             ("map", 37, False): 7, ("map", 42, True): 7, ("map", 52, True): 7, ("map", 53, False): 7, ("map", 54, False): 21}


def map_case(i, s, fix):
    seed = 11000 + 2 * i + int(fix) + SEED_BUMP.get(("map", i, fix), 0)
    return SC.wide_case("nmapfix" if fix else "nmap", s.L, [SC.scan(MM=s.NSn, NM=s.NM, N2=s.N2, fix=fix), SC.narrow_behind(s.L, s.N2, True, 128)],
                        s.model, seed, use=True, cls=s.cls, MM=s.NSn + s.NM, N2=s.N2, NSn=s.NSn, NMn=s.NM, fixed=fix, table="map")


def localise_case(i, NM, fix):
    seed = 11400 + 2 * i + int(fix) + SEED_BUMP.get(("loc", i, fix), 0)
    return SC.wide_case("nlocfix" if fix else "nloc", 0, [SC.scan(NM=NM, fix=fix), SC.narrow_behind(0, 0, True, 128)], OMNI if i % 2 else DIFF, seed,
                        use=True, cls="0", MM=NM, N2=0, NSn=0, NMn=NM, fixed=fix, table="localise")


def unused_case(i, L, MM, N2, fix):
    seed = 11500 + i + SEED_BUMP.get(("unused", i), 0)
    return SC.wide_case("nplainfix" if fix else "nplain", L, [SC.scan(MM=MM, N2=N2, fix=fix), SC.narrow_behind(L, N2, False, 128)],
                        OMNI if i % 2 else DIFF, seed, use=False, cls=FC.n2_class(3 + 2 * L, N2), MM=MM, N2=N2, NSn=MM, NMn=0, fixed=fix, table="unused")


# ---- the cases ---------------------------------------------------------------------------------------------------------------
_fix = _map = None


def fix_cases():
    """The fix table and the four heading shapes."""
    global _fix
    if _fix is None:
        out = []
        for i, (L, MM, N2, model) in enumerate(fix_shapes()):
            base = FC.sweep_case(L, MM, N2, model, 11700 + i + SEED_BUMP.get(("fix", i), 0), name="nfix")
            c = PC.attach_fixes(base, 11800 + i)
            c.cls = "sweep"
            out.append(c)
        out += [heading_case(i, *s) for i, s in enumerate(HEADING_SHAPES)]
        assert len({c.name for c in out}) == len(out)
        _fix = out
    return _fix


def map_cases():
    """The members on the map (each shape without a fix, every second one once more with one), pure localisation that moves, and
    the members that do not use the map."""
    global _map
    if _map is None:
        out = []
        for i, s in enumerate(map_shapes()):
            out += [map_case(i, s, fix) for fix in s.variants]
        for i, NM in enumerate(LOCALISE_NM):
            out += [localise_case(i, NM, False), localise_case(i, NM, True)]
        out += [unused_case(i, *s) for i, s in enumerate(UNUSED_SHAPES)]
        assert len({c.name for c in out}) == len(out)
        _map = out
    return _map


def pattern_members():
    """Eight members of the map table, one per n mod 16, four with a fix, all on the map: for the call-pattern test."""
    out, seen = [], set()
    for want_fix in (True, False):
        for c in map_cases():
            if c.table == "map" and c.fixed == want_fix and c.n % 16 not in seen and c.n <= N_MAX and sum(x.fixed == want_fix for x in out) < 4:
                out.append(c)
                seen.add(c.n % 16)
    assert len(out) == 8 and len(seen) == 8 and sum(c.fixed for c in out) == 4, sorted(seen)
    return out


# ---- the CPU side ------------------------------------------------------------------------------------------------------------
_fix_runs = _map_runs = None


def fix_runs():
    """name -> fleet_harness.run_references' result (per scan: [joint pose witness state], oracle state, numpy state); the lists of
    all three are checked against the case's claim there."""
    global _fix_runs
    if _fix_runs is None:
        _fix_runs = {c.name: H.run_references(c, FIX_SUITE) for c in fix_cases()}
    return _fix_runs


def map_runs():
    """name -> fleet_map_cases.run_references' result, likewise."""
    global _map_runs
    if _map_runs is None:
        _map_runs = {c.name: FM.run_references(c, MAP_SUITE) for c in map_cases()}
    return _map_runs
