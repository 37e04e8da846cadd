"""Cases of the voxel filters against tests/witness/voxel_witness.py, shared by tests/test_voxel_witness_cpu.py (oracle == witness,
the cases reach their edges, planted defects of the witness are seen) and tests/test_voxel_witness_gpu.py (GridFrontEnd.VoxelFilter,
GridFrontEnd.AdaptiveVoxelFilter and ScanMatchFleet.filter == witness).  Every comparison is exact: count, order and bit patterns.

A case is one scan with its parameters: ``Case(name, returns, misses, size, options, label)``; ``options`` is
(max_length, min_num_points, max_range) and ``label`` the path the WITNESS's adaptive search takes on VoxelFilter(size)(returns)
(None where the family is not about the search).  The families of tests/fleet_filter_scan_cases.py are re-used as they are; the
families below are aimed at what those leave open.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import fleet_filter_scan_cases as FC
from tests.witness import voxel_witness as W

F32 = np.float32
Case = namedtuple("Case", "name returns misses size options label")
DEFAULT = (0.9, 500.0, 100.0)
FLEET_LIMIT = 8192                   # ScanMatchFleet.filter: one workgroup's points
SMALL_HANDLE, LARGE_HANDLE = 1021, 12288   # max_points of the two GridFrontEnds; 1021 is no multiple of 8 (kg_first's read group)
BLOCK, GROUP, TILE, WAVE = 256, 8, 1024, 64


def empty():
    return np.zeros((0, 2), np.float32)


# ---- the families of fleet_filter_scan_cases ---------------------------------------------------------------------------
def reused_cases():
    out = []
    for size in FC.STRIDE_SIZES:
        out += [Case(f"stride/{size}/{k}", r, m, size, DEFAULT, None) for k, (r, m) in enumerate(FC.stride_case())]
    out += [Case(f"rounding/{k}", r, m, FC.ROUND_RES, DEFAULT, None) for k, (r, m) in enumerate(FC.rounding_case())]
    scans, opt = FC.hash_case(FLEET_LIMIT)
    out += [Case(f"hash/{k}", r, m, FC.HASH_SIZE, FC.option_values(opt), None) for k, (r, m) in enumerate(scans)]
    scans, opt = FC.gate_case()
    out += [Case(f"gate/{k}", r, m, 0.025, FC.option_values(opt), None) for k, (r, m) in enumerate(scans)]
    scans, opt, paths = FC.adaptive_case()
    out += [Case(f"adaptive/{k}", r, m, FC.ADAPTIVE_SIZE, FC.ADAPTIVE_OPTIONS, p) for k, ((r, m), p) in enumerate(zip(scans, paths))]
    scans, opt, _ = FC.fraction_case()
    out += [Case(f"fraction/{k}", r, m, FC.ADAPTIVE_SIZE, FC.FRACTION_OPTIONS, None) for k, (r, m) in enumerate(scans)]
    out += [Case(f"crowd/{k}", r, m, 0.025, FC.CROWD_OPTIONS, None) for k, (r, m) in enumerate(FC.crowd_case())]
    return out


# ---- division: float32 against double ------------------------------------------------------------------------------------
DIVISION_SIZES = (0.025, 0.05, 0.11, 0.9)
DIVISION_MIN = 8                     # points per size whose key differs between the two divisions
HALF_SIZE = 0.11                     # no power of two: v / size is rounded, and some quotients round to k + 0.5 exactly


def _near_half(size, k):
    """float32 values within 3 ulp of (k + 0.5) * size: where a quotient's last bit decides the voxel."""
    v = F32((k + 0.5) * float(F32(size)))
    up, down = [v], []
    for _ in range(3):
        up.append(np.nextafter(up[-1], F32(np.inf)))
        down.append(np.nextafter((down or [v])[-1], F32(-np.inf)))
    return np.array(down[::-1] + up, np.float32)


def division_points(size, want=DIVISION_MIN):
    """-> (differing, halves): float32 coordinates whose voxel index differs between float32 and double division, both signs, and
    coordinates whose float32 quotient is exactly k + 0.5.  A search: voxel borders are walked outwards until enough are found."""
    differ, halves = {1: [], -1: []}, {1: [], -1: []}
    k = 0
    while min(len(differ[1]), len(differ[-1])) < want // 2 or (size == HALF_SIZE and min(len(halves[1]), len(halves[-1])) < 4):
        for sign in (1, -1):
            v = _near_half(size, k) * F32(sign)
            a, b = W.cell_index(v, size), W.cell_index(v, size, "double_division")
            differ[sign] += v[a != b].tolist()
            q = (v / F32(size)).astype(np.float64)
            halves[sign] += v[np.abs(q) - np.floor(np.abs(q)) == 0.5].tolist()
        k += 1
        assert k < 200000, "no float32/double disagreement found"
    return (np.array(differ[1][:want // 2] + differ[-1][:want // 2], np.float32),
            np.array(halves[1][:4] + halves[-1][:4], np.float32))


def _probe_cloud(xs, size, row0):
    """Each special x with two plain points behind it, one in the middle of either voxel it could fall into, all three in a row of
    their own: exactly one of the two plain points goes, and which one says where the special point was put."""
    pts = []
    s = float(F32(size))
    for j, x in enumerate(xs.tolist()):
        y = (row0 + j) * s
        k = np.floor(x / s)
        pts += [[x, y], [k * s, y + 0.1 * s], [(k + 1) * s, y - 0.1 * s]]
    return np.array(pts, np.float32)


def division_cases():
    out = []
    for size in DIVISION_SIZES:
        differ, halves = division_points(size)
        xs = np.concatenate([differ, halves]) if size == HALF_SIZE else differ
        cloud = _probe_cloud(xs, size, 3)
        out.append(Case(f"division/{size}", cloud, cloud[:, ::-1].copy(), size, DEFAULT, None))       # the misses: the same in y
    return out


# ---- range gate: float32 norm against double -------------------------------------------------------------------------------
def gate_norm_case():
    """Points whose float32 norm is max_range exactly while their norm in double is beyond it: they stay.  min_num_points is the
    number that stays, so `size <= min_num_points` holds with equality: sparse."""
    rng = np.random.default_rng(1301)
    found = np.zeros((0, 2), np.float32)
    for _ in range(50):
        p = rng.uniform(-1, 1, (20000, 2))
        p = (p / np.linalg.norm(p, axis=1)[:, None] * FC.GATE_RANGE).astype(np.float32)
        d = p.astype(np.float64)
        pick = (FC.norm_f32(p) <= F32(FC.GATE_RANGE)) & (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) > FC.GATE_RANGE)
        found = np.concatenate([found, p[pick]])
        if found.shape[0] >= 16:
            break
    assert found.shape[0] >= 16
    inside = rng.uniform(-3, 3, (40, 2)).astype(np.float32)
    cloud = np.concatenate([found[:16], FC.PAST_GATE, inside])
    return [Case("gate/norm", cloud, None, 0.0005, (0.9, 56.0, FC.GATE_RANGE), ("sparse",))]


# ---- kg_first: block borders and the read group ----------------------------------------------------------------------------
FIRST_COUNTS = (255, 256, 257, 263, 264, 265, 511, 512, 513)
FIRST_SIZE = 0.05
FIRST_KINDS = ("borders", "ends", "tail", "one", "distinct")


def _distinct(n, rng, size=FIRST_SIZE):
    """n points in n different voxels, each well inside its own."""
    i = rng.permutation(n)
    centre = np.stack([(i % 64) - 32, (i // 64) - 3], 1) * float(F32(size))
    return (centre + rng.uniform(-0.3, 0.3, (n, 2)) * size).astype(np.float32)


def _twin(cloud, a, b, rng, size=FIRST_SIZE):
    """Point b moves into point a's voxel, with other bits."""
    s = float(F32(size))
    centre = np.round(cloud[a].astype(np.float64) / s) * s
    cloud[b] = (centre + rng.uniform(-0.3, 0.3, 2) * size).astype(np.float32)


def first_pairs(kind, n):
    """The (first, twin) index pairs of a kind at n points."""
    if kind == "borders":
        return [(b - 1, b) for b in range(BLOCK, n, BLOCK)]
    if kind == "ends":
        return [(0, n - 1)]
    if kind == "tail":
        g = GROUP * ((n - 1) // GROUP)                         # the last group read; a pair needs two points in it
        return [(g, n - 1)] if n - 1 > g else [(n - 2, n - 1)]
    return []


def first_cloud(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "one":
        return (rng.uniform(-0.3, 0.3, (n, 2)) * FIRST_SIZE + np.array([7, -4]) * FIRST_SIZE).astype(np.float32)
    cloud = _distinct(n, rng)
    for a, b in first_pairs(kind, n):
        _twin(cloud, a, b, rng)
    return cloud


def first_cases():
    out = []
    for n in FIRST_COUNTS + (SMALL_HANDLE,):
        for j, kind in enumerate(FIRST_KINDS):
            c = first_cloud(kind, n, 1400 + 10 * n + j)
            out.append(Case(f"first/{kind}/{n}", c, c[::-1].copy(), FIRST_SIZE, (0.9, 100.0, 100.0), None))
    return out


# ---- kg_compact: lanes, waves and tiles ------------------------------------------------------------------------------------
COMPACT_COUNTS = (1023, 1024, 1025, 2047, 2049)
COMPACT_KINDS = ("lanes", "waves", "tiles")
COMPACT_RANGE = 50.0


def compact_keep(kind, n):
    i = np.arange(n)
    if kind == "lanes":
        keep = (i % WAVE == 0) | (i % WAVE == WAVE - 1)
    elif kind == "waves":
        keep = (i % TILE < WAVE) | (i % TILE >= TILE - WAVE)
    else:
        keep = (i < TILE) | (i >= 2 * TILE)                    # a third tile exists at 2049 only; below, the second goes whole
    keep[0] = True
    return keep


def compact_cases():
    """Two clouds per (kind, n): `v` where the dropped points repeat point 0's voxel (VoxelFilter compacts), `g` where they lie
    beyond max_range (the gate compacts; min_num_points is high, so the gated cloud is the answer)."""
    out = []
    for n in COMPACT_COUNTS:
        for j, kind in enumerate(COMPACT_KINDS):
            rng = np.random.default_rng(1500 + 10 * n + j)
            keep = compact_keep(kind, n)
            v = _distinct(n, rng)
            for b in np.nonzero(~keep)[0]:
                _twin(v, 0, b, rng)
            g = _distinct(n, rng)
            far = 2 * np.pi * rng.permutation(n) / n                   # 0.18 m apart and more: VoxelFilter in front keeps them all
            g[~keep] = np.stack([60.0 * np.cos(far), 60.0 * np.sin(far)], 1).astype(np.float32)[~keep]
            out.append(Case(f"compact/v/{kind}/{n}", v, None, FIRST_SIZE, (0.9, 5000.0, 100.0), ("sparse",)))
            out.append(Case(f"compact/g/{kind}/{n}", g, None, 0.0005, (0.9, 5000.0, COMPACT_RANGE), ("sparse",)))
    return out


# ---- the host's walk of the search ---------------------------------------------------------------------------------------
# The walk evaluates the bisection tree 5 levels per round trip for ni <= 4096 points behind the gate, 3 for ni <= 8192, 2 above,
# and a trace has 3 or 4 letters: a second batch is needed by 4-letter traces in the middle class and by every ladder trace in the
# upper one.  (kind, points behind the gate, points the gate removes in front, seed, max_length, min_num_points as a fraction of
# the points, the WITNESS's label).  tests/test_voxel_witness_cpu.py asserts the labels.
WALK_SIZE = 0.0005
WALK_RANGE = 40.0
WALK = (
    # ni <= 4096: one batch
    ("uniform", 4096, 5, 4103, 0.9, 0.45, ("ladder", 1, "RRAR")),
    ("blob", 4096, 0, 4103, 0.9, 0.40, ("ladder", 2, "RRRR")),
    # 4096 < ni <= 8192: three levels, then one
    ("uniform", 4097, 3, 4104, 0.9, 0.45, ("ladder", 1, "RRAR")),           # accepted in the first batch only: the parked slice
    ("blob", 4097, 0, 4104, 0.9, 0.35, ("ladder", 2, "RRAA")),              # in both
    ("walls", 4097, 0, 4104, 0.9, 0.10, ("ladder", 2, "RRRA")),             # in the second only
    ("walls", 4097, 0, 4104, 0.9, 0.65, ("ladder", 5, "RRRR")),             # in neither: the rung's own cloud, parked
    ("uniform", 6000, 0, 6007, 0.9, 0.30, ("ladder", 1, "RRAA")),
    ("uniform", 8192, 7, 8199, 0.9, 0.25, ("ladder", 1, "RRAR")),
    ("uniform", 8192, 0, 8199, 0.9, 0.70, ("ladder", 2, "RRRR")),
    ("blob", 8192, 0, 8199, 0.9, 0.50, ("ladder", 3, "RRAA")),
    ("walls", 8192, 0, 8199, 0.9, 0.40, ("ladder", 5, "RRRA")),
    # ni > 8192: two levels, then two
    ("uniform", 8193, 2, 8200, 0.9, 0.25, ("ladder", 1, "RRAR")),           # only the second batch accepts
    ("blob", 8193, 0, 8200, 0.9, 0.10, ("ladder", 1, "RRRR")),              # neither
    ("walls", 8193, 0, 8200, 0.9, 0.65, ("ladder", 6, "RRAA")),
    ("uniform", 9000, 0, 9007, 0.9, 0.10, ("ladder", 1, "AAR")),            # only the first: the parked slice
    ("uniform", 9000, 0, 9007, 0.9, 0.60, ("ladder", 2, "RRAA")),
    ("uniform", 9000, 0, 9007, 0.9, 0.65, ("ladder", 2, "RRRA")),
    ("blob", 9000, 0, 9007, 0.9, 0.55, ("ladder", 3, "RRRR")),
    ("walls", 9000, 0, 9007, 0.9, 0.10, ("ladder", 4, "RAA")),              # both
    ("uniform", 12000, 0, 12007, 0.9, 0.10, ("ladder", 1, "ARR")),
    ("uniform", 12000, 0, 12007, 0.9, 0.20, ("ladder", 1, "RRRA")),
    ("blob", 12000, 0, 12007, 0.9, 0.65, ("ladder", 4, "RAA")),
    ("walls", 12000, 0, 12007, 0.9, 0.35, ("ladder", 5, "RRRR")),
    ("uniform", 12000, 0, 12007, 0.9, 0.05, ("first",)),
    # other ladders
    ("uniform", 9000, 0, 9007, 5.0, 0.30, ("ladder", 4, "RAA")),
    ("uniform", 9000, 0, 9007, 0.3, 0.60, ("ladder", 1, "AAR")),
    ("blob", 3000, 0, 3007, 5.0, 0.50, ("ladder", 5, "RAA")),
    ("blob", 3000, 0, 3007, 0.3, 0.50, ("ladder", 1, "RAA")),
)
NOTHING_POINTS, NOTHING_SIZE = 9000, 0.00005     # ni > 8192 and no size dense enough: 9000 points at 2000 positions


def _walk_cloud(kind, n, front, seed):
    pts = W.voxel_filter(FC.point_set(kind, n + 64, seed, 1.0), WALK_SIZE)[:n]     # VoxelFilter(WALK_SIZE) in front keeps every point
    assert pts.shape[0] == n
    if front:
        ang = np.random.default_rng(seed + 1).uniform(0, 2 * np.pi, front)
        pts = np.concatenate([np.stack([45.0 * np.cos(ang), 45.0 * np.sin(ang)], 1).astype(np.float32), pts])
    return pts


def walk_cases():
    out = []
    for k, (kind, n, front, seed, maxl, frac, label) in enumerate(WALK):
        name = f"walk/{k}/{kind}/{n}/{maxl}/{frac}"
        out.append(Case(name, _walk_cloud(kind, n, front, seed), None, WALK_SIZE, (maxl, float(int(frac * n)), WALK_RANGE),
                        label))
    rng = np.random.default_rng(1601)
    spots = rng.uniform(-12, 12, (2000, 2))
    m = NOTHING_POINTS + 100
    crowd = W.voxel_filter((spots[rng.integers(0, 2000, m)] + rng.uniform(-0.001, 0.001, (m, 2))).astype(np.float32), NOTHING_SIZE)[:NOTHING_POINTS]
    assert crowd.shape[0] == NOTHING_POINTS
    out.append(Case("walk/nothing", crowd, None, NOTHING_SIZE, (0.9, 5000.0, WALK_RANGE), ("nothing", 7)))
    return out


# ---- counts that meet min_num_points exactly, and a bisection that ends on the tolerance itself -----------------------------
TIE_LENGTH = 5.0                     # 5 * 2**-k: low * 1.25 and low * 1.375 are exact, so (high - low) / low is float32(0.1) itself


def tie_cases():
    """min_num_points equal to a count the search compares it with: the number of points behind the gate (sparse, by <=), the
    count at max_length (first, by >=) -- and a trace RAR at a max_length whose fourth test is 0.1f > 0.1f, with min_num_points
    such that a fourth candidate would be accepted."""
    p = FC.point_set("uniform", 3000, 1701, 1.0)
    at_max = float(W.voxel_filter(p, F32(0.9)).shape[0])
    low = F32(TIE_LENGTH) / F32(8)                               # rung 3
    fourth = float(W.voxel_filter(p, low * F32(1.3125)).shape[0])
    return [Case("tie/size", p, None, WALK_SIZE, (0.9, 3000.0, 100.0), ("sparse",)),
            Case("tie/first", p, None, WALK_SIZE, (0.9, at_max, 100.0), ("first",)),
            Case("tie/tolerance", p, None, WALK_SIZE, (TIE_LENGTH, fourth, 100.0), ("ladder", 3, "RAR"))]


FAMILIES = (reused_cases, division_cases, gate_norm_case, first_cases, compact_cases, walk_cases, tie_cases)
_cases = None


def all_cases():
    """Every case, built once."""
    global _cases
    if _cases is None:
        _cases = [c for family in FAMILIES for c in family()]
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


_witness = {}


def witness_of(case, mutant=None):
    """-> (returns, misses, filtered, label) of the witness, computed once per case and mutant."""
    key = (case.name, mutant)
    if key not in _witness:
        _witness[key] = W.filter_scan(case.returns, case.misses, case.size, *case.options, mutant=mutant)
    return _witness[key]


def fleet_groups(cases=None):
    """The cases ScanMatchFleet.filter can take (one workgroup's points), grouped by what one call shares: size and options."""
    groups = {}
    for c in all_cases() if cases is None else cases:
        if max(c.returns.shape[0], FC.misses_of((c.returns, c.misses)).shape[0]) <= FLEET_LIMIT:
            groups.setdefault((c.size, c.options), []).append(c)
    return groups


# What the CPU run measured (tests/test_voxel_witness_cpu.py prints and asserts it): the first case that sees each planted defect.
EQUIVALENT = {
    "ladder_ge": "high = float(max_length) * 2**-k meets 1e-2f * max_length only if 2**k * 1e-2f * max_length / float(max_length) "
                 "== 1, and that factor is within 1e-7 of 0.64 or 1.28: `>=` and `>` never differ",
}
