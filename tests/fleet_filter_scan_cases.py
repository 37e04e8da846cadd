"""Cases of the fleet voxel filters (rgrid_batch_filter_* of include/rgrid.h, ScanMatchFleet.filter), shared by
tests/test_fleet_filter_scan_cpu.py and tests/test_fleet_filter_scan_gpu.py.

A scan is ``(returns_xy, misses_xy_or_None)`` as ``ScanMatchFleet.submit_filter`` takes it.  The specification of a scan's result is
the three single calls -- VoxelFilter(size) of the returns, VoxelFilter(size) of the misses, AdaptiveVoxelFilter(options) of the
first: ``oracle_triple`` gives them from the CPU oracle, ``handle_triple`` from a GridFrontEnd.  Every comparison is exact, on the
points' bit patterns.
"""
from __future__ import annotations

import numpy as np

OK, INVALID, CAPACITY, BUFFER = 0, -1, -4, -5
WG_THREADS, WAVE = 1024, 64         # kgb_filter: a thread holds points tid, tid + 1024, ...; the compaction scans tiles of 1024 by waves of 64
F32 = np.float32


def bits(cloud):
    return np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 2).view(np.uint32)


def same_cloud(a, b):
    """Same number of points, same bit patterns (-0.0 is not 0.0)."""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def option_values(options=None):
    return (0.9, 500.0, 100.0) if options is None else (options.max_length, options.min_num_points, options.max_range)


def misses_of(scan):
    return np.zeros((0, 2), np.float32) if scan[1] is None else np.ascontiguousarray(scan[1], dtype=np.float32).reshape(-1, 2)


def oracle_triple(scan, size=0.025, options=None):
    """-> (fr, fm, av) of the CPU oracle."""
    from oracle.binding import oracle_adaptive_voxel_filter, oracle_voxel_filter
    fr = oracle_voxel_filter(scan[0], size)
    return fr, oracle_voxel_filter(misses_of(scan), size), oracle_adaptive_voxel_filter(fr, *option_values(options))


def handle_triple(gf, scan, size=0.025, options=None):
    """-> (fr, fm, av) of a GridFrontEnd's three calls."""
    fr = gf.VoxelFilter(scan[0], size)
    return fr, gf.VoxelFilter(misses_of(scan), size), gf.AdaptiveVoxelFilter(fr, options)


def same_result(result, triple):
    return same_cloud(result.returns, triple[0]) and same_cloud(result.misses, triple[1]) and same_cloud(result.filtered, triple[2])


def same_results(a, b):
    return a.status == b.status and same_result(a, (b.returns, b.misses, b.filtered))


def search_path(points, max_length=0.9, min_num_points=500.0, max_range=100.0):
    """AdaptiveVoxelFilter::Filter (voxel_filter.cc:15-76) restated with the oracle's voxel filter doing the counting ->
    (label, filtered cloud).  Labels: ("sparse",), ("first",), ("ladder", rung, trace) with a letter per bisection step (A the
    candidate was dense enough and became the result, R it was not), ("nothing", rungs tried)."""
    from oracle.binding import oracle_voxel_filter as vf
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    p = p[np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) <= F32(max_range)]
    if p.shape[0] <= min_num_points:
        return ("sparse",), p
    maxl = F32(max_length)
    out = vf(p, maxl)
    if out.shape[0] >= min_num_points:
        return ("first",), out
    high, rung = maxl, 0
    while high > F32(1e-2) * maxl:
        rung += 1
        low = high / F32(2)
        out = vf(p, low)
        if out.shape[0] >= min_num_points:
            trace = ""
            while (high - low) / low > F32(1e-1):
                mid = (low + high) / F32(2)
                cand = vf(p, mid)
                if cand.shape[0] >= min_num_points:
                    low, out, trace = mid, cand, trace + "A"
                else:
                    high, trace = mid, trace + "R"
            return ("ladder", rung, trace), out
        high = high / F32(2)
    return ("nothing", rung), out


# ---- 1. strides ------------------------------------------------------------------------------------------------------
STRIDE_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
STRIDE_MISSES = (1025, None, 2049, 63, 1, 1024, 65, 64, 1023)      # the same set in another order; None stands for 0
STRIDE_SIZES = (0.025, 0.11, 0.9)


def cloud(rng, n, half=2.0):
    """n points uniform in +-half metres, every seventh rounded to one decimal (such points share voxels and voxel borders)."""
    p = rng.uniform(-half, half, (n, 2))
    p[::7] = np.round(p[::7], 1)
    return p.astype(np.float32)


_stride = None


def stride_case():
    global _stride
    if _stride is None:
        rng = np.random.default_rng(1201)
        _stride = [(cloud(rng, nr), None if nm is None else cloud(rng, nm)) for nr, nm in zip(STRIDE_COUNTS, STRIDE_MISSES)]
    return _stride


# ---- 2. rounding and duplicates --------------------------------------------------------------------------------------
ROUND_RES = 0.25                     # a power of two: v / res is exact


def rounding_case():
    """-> scans for one call at size ROUND_RES: half-way coordinates of both signs, signed zeros, one voxel, a voxel per point, returns
    and misses in the same voxels."""
    rng = np.random.default_rng(1202)
    k = np.arange(-6, 6)
    half = ((k + 0.5) * ROUND_RES).astype(np.float32)                  # lroundf rounds these away from zero
    whole = (np.arange(-7, 8) * ROUND_RES).astype(np.float32)
    hx, hy = np.meshgrid(half, half, indexing="ij")
    wx, wy = np.meshgrid(whole, whole, indexing="ij")
    halves = np.stack([hx.ravel(), hy.ravel()], 1)
    wholes = np.stack([wx.ravel(), wy.ravel()], 1)
    both = np.concatenate([halves, wholes])                            # every half-way point first: it takes the voxel of a whole one
    mixed = np.concatenate([wholes, halves])[rng.permutation(both.shape[0])]
    zeros = np.array([[-0.0, 0.2], [0.0, 0.2], [0.2, -0.0], [0.2, 0.0], [-0.0, -0.0], [0.0, 0.0], [-0.2, 0.0]], np.float32)
    one_voxel = rng.uniform(0.01, 0.1, (500, 2)).astype(np.float32)
    g = np.arange(-20, 20)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    own = (np.stack([gx.ravel(), gy.ravel()], 1) * ROUND_RES).astype(np.float32)[rng.permutation(1600)]
    shared_ret = own[:700]
    shared_mis = (own[:700][::-1] + np.float32(0.05)).astype(np.float32)   # the same voxels, other points, another order
    return [(both, halves), (mixed, None), (zeros, zeros[::-1]), (one_voxel, one_voxel[:1]), (own, None), (shared_ret, shared_mis)]


# ---- 3. hash stress ----------------------------------------------------------------------------------------------------
HASH_SIZE = 0.025


def hash_case(limit):
    """-> (scans, options): `limit` points in distinct voxels; 4096 points whose voxel indices are multiples of 1024 (x) and 4096 (y);
    8192 points in three voxels."""
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    rng = np.random.default_rng(1203)
    i = rng.permutation(limit)
    distinct = np.stack([(i % 128) * 0.05, (i // 128) * 0.05 - 1.0], 1).astype(np.float32)
    a, b = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    strided = np.stack([a.ravel() * 1024 * HASH_SIZE, (b.ravel() - 32) * 4096 * HASH_SIZE], 1).astype(np.float32)[rng.permutation(4096)]
    centres = np.array([[0.5, 0.5], [-3.0, 1.0], [2.0, -2.0]])
    three = (centres[rng.integers(0, 3, 8192)] + rng.uniform(-0.005, 0.005, (8192, 2))).astype(np.float32)
    return [(distinct, distinct[::-1]), (strided, None), (three, three[:100])], AdaptiveVoxelFilterOptions(0.9, 500, 1.0e4)


def voxel_index(v, size):
    """(int)lroundf(v / size) away from ties (numpy's rint rounds ties to even: not for half-way values)."""
    return np.rint(np.asarray(v, np.float32) / F32(size)).astype(np.int64)


# ---- 4. range gate -----------------------------------------------------------------------------------------------------
GATE_RANGE = 5.0
ON_GATE = np.array([[3.0, 4.0], [-3.0, 4.0], [4.0, -3.0], [-4.0, -3.0]], np.float32)                 # norm exactly 5
PAST_GATE = np.where(np.abs(ON_GATE) == 4.0, np.nextafter(ON_GATE, np.float32(np.inf) * np.sign(ON_GATE)), ON_GATE).astype(np.float32)   # one ulp beyond


def norm_f32(p):
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2)
    return np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])


AXIS_GATE = np.array([[0.0, 5.0], [5.0, 0.0], [0.0, -5.0], [-5.0, 0.0]], np.float32)


def gate_case():
    """-> (scans, options): points on the gate in front of a cloud that is searched; a gate that removes everything; points one ulp
    past the gate and points on it in front of a cloud of which the gate leaves no more than min_num_points points."""
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    rng = np.random.default_rng(1204)
    searched = np.concatenate([ON_GATE, rng.uniform(-6.0, 6.0, (600, 2)).astype(np.float32)])
    ang = rng.uniform(-np.pi, np.pi, 300)
    ring = np.stack([7.0 * np.cos(ang), 7.0 * np.sin(ang)], 1).astype(np.float32)
    few = np.concatenate([PAST_GATE, AXIS_GATE, rng.uniform(-2.0, 2.0, (30, 2)).astype(np.float32), ring])
    return [(searched, ring), (ring, None), (few, None)], AdaptiveVoxelFilterOptions(0.9, 200, GATE_RANGE)


# ---- 5. every path of the adaptive search ------------------------------------------------------------------------------
def point_set(kind, n, seed, scale=1.0):
    """The wall-like, uniform and blob-like sets of test_adaptive_voxel_filter_search_paths, scaled; "repeated": n / 4 positions,
    four points within 2 mm of each."""
    rng = np.random.default_rng(seed)
    if kind == "walls":
        t = rng.uniform(0, 4, n)
        side = np.floor(t).astype(int)
        u = (t - side) * 16 - 8
        pts = np.stack([np.where(side % 2 == 0, u, np.where(side == 1, 8.0, -8.0)), np.where(side % 2 == 1, u, np.where(side == 0, -8.0, 8.0))], 1)
        pts += rng.normal(0, 0.01, pts.shape)
    elif kind == "uniform":
        pts = rng.uniform(-12, 12, (n, 2))
    elif kind == "blob":
        pts = rng.normal(0, 2.5, (n, 2))
    else:
        pts = np.tile(rng.uniform(-12, 12, (n // 4, 2)), (4, 1))[rng.permutation(n // 4 * 4)] + rng.uniform(-0.001, 0.001, (n // 4 * 4, 2))
    return (pts.astype(np.float32) * np.float32(scale)).astype(np.float32)


# One call has one set of options, so the paths come from the clouds: their extent decides where the search ends.
# (kind, points, seed, scale, the path the ORACLE takes: tests/test_fleet_filter_scan_cpu.py asserts it)
ADAPTIVE_SIZE = 0.0005               # the voxel filter in front keeps (nearly) every point, the repeated ones too
ADAPTIVE_OPTIONS = (0.9, 400.0, 1000.0)
ADAPTIVE = (
    ("uniform", 300, 3, 1.0, ("sparse",)),
    ("uniform", 1500, 1507, 1.5, ("first",)),
    ("walls", 2600, 2607, 3.0, ("ladder", 1, "AAR")),
    ("blob", 1000, 1007, 1.5, ("ladder", 1, "ARR")),
    ("walls", 1000, 1007, 0.4, ("ladder", 4, "RAR")),
    ("blob", 600, 607, 0.1, ("ladder", 5, "RRAA")),
    ("uniform", 600, 607, 0.05, ("ladder", 5, "ARA")),
    ("uniform", 1000, 1007, 0.1, ("ladder", 3, "RRRR")),          # the bisection accepts nothing: the rung's cloud stays
    ("walls", 600, 607, 0.02, ("nothing", 7)),
    ("repeated", 1200, 6, 1.0, ("nothing", 7)),                   # 300 positions: fewer than min_num_points at every size tried
    ("uniform", 8192, 9, 0.1, ("ladder", 3, "RRRA")),
)
FRACTION_OPTIONS = (0.9, 2.5, 1000.0)                             # a min_num_points that is no integer: the comparisons are in double
FRACTION = (np.array([[0.0, 0.0], [5.0, 5.0]], np.float32),                       # 2 <= 2.5: sparse
            np.array([[0.0, 0.0], [5.0, 5.0], [-5.0, 3.0]], np.float32),          # 3 voxels at max_length: first
            np.array([[0.0, 0.0], [0.2, 0.0], [-5.0, 3.0]], np.float32),          # two share a voxel until the ladder separates them
            np.array([[0.0, 0.0], [0.001, 0.0], [-5.0, 3.0]], np.float32))        # ... and never do: nothing dense enough
FRACTION_PATHS = ("sparse", "first", "ladder", "nothing")


def adaptive_case():
    """-> (scans, options, paths) of one call."""
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    return ([(point_set(kind, n, seed, scale), None) for kind, n, seed, scale, _ in ADAPTIVE], AdaptiveVoxelFilterOptions(*ADAPTIVE_OPTIONS),
            [path for *_, path in ADAPTIVE])


def fraction_case():
    from reflector_ekf_slam_amd.grid import AdaptiveVoxelFilterOptions
    return [(p, None) for p in FRACTION], AdaptiveVoxelFilterOptions(*FRACTION_OPTIONS), FRACTION_PATHS


# ---- 6. statuses -------------------------------------------------------------------------------------------------------
STATUS_MAX_POINTS = 256


def status_case():
    """-> (scans, statuses): more returns than the handle's max_points, more misses than that, a NaN, an infinity (among the misses),
    no returns but misses, and healthy scans in between."""
    rng = np.random.default_rng(1206)
    nan = cloud(rng, 100); nan[57, 1] = np.nan
    inf = cloud(rng, 90); inf[3, 0] = -np.inf
    scans = [(cloud(rng, 200), cloud(rng, 50)), (cloud(rng, STATUS_MAX_POINTS + 1), None), (nan, cloud(rng, 10)), (cloud(rng, 256), cloud(rng, 256)),
             (cloud(rng, 40), inf), (np.zeros((0, 2), np.float32), cloud(rng, 120)), (cloud(rng, 10), cloud(rng, STATUS_MAX_POINTS + 1)),
             (cloud(rng, 130), None)]
    return scans, [OK, CAPACITY, INVALID, OK, INVALID, OK, CAPACITY, OK]


# ---- 8. crowd ------------------------------------------------------------------------------------------------------------
CROWD = 320
CROWD_OPTIONS = (0.9, 50.0, 100.0)                                  # 100 to 200 returns: the search runs in every workgroup


def crowd_case():
    """More workgroups than an MI355X has compute units: CROWD scans of 100 to 200 returns and as many misses."""
    rng = np.random.default_rng(1208)
    scans = []
    for _ in range(CROWD):
        n = int(rng.integers(100, 201))
        scans.append((cloud(rng, n, 3.0), cloud(rng, n, 3.0)))
    return scans
