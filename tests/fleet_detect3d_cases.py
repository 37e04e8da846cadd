"""Case builders shared by tests/test_fleet_detect3d_cpu.py and tests/test_fleet_detect3d_gpu.py: the clouds the fleet 3D detector
(rdet3d_batch_*, csrc/det3d_batch.hip) is held to, each with what it claims (the oracle's counts: K accepted clusters, M survivors of the
intensity gate, M2 survivors of the outlier removal, or the refusal), and the end-to-end sessions.  The CPU suite checks the claims under
oracle/detect3d_oracle.c and tests/witness/detect3d_witness.py; the GPU suite holds the kernel to the oracle bit for bit.
Reference: src/reflector_detect/point_cloud/point_cloud_reflector_detect.cc:9-106."""
import functools

import numpy as np

MAX_BRIGHT = 5120            # rdet3d_batch_max_bright(): det3d.hip's MFAST
MAX_CENTERS = 256
CAPACITY, BUFFER = -4, -5
SIZES = (0, 1, 30, 31, 32, 63, 64, 65, 1023, 1024, 1025)
S2B_OTHER = (0.3, -0.2, 0.7)
E2E_MEMBERS, E2E_TICKS, E2E_MAX_OBS = 6, 40, 32


def _blob(center, n, spread, rng, intensity=200.0):
    p = rng.normal(0, spread, size=(n, 3)) + np.asarray(center)
    return np.concatenate([p, np.full((n, 1), intensity)], -1)


def _scene(rng, n_clusters, dim=2000, per=(8, 60), spread=0.03, extent=10.0, outliers=30):
    """(the builder of tests/test_detect3d_paths_gpu.py)"""
    parts = [_blob((0, 0, 0), dim, extent / 2, rng, intensity=20.0)]
    for _ in range(n_clusters):
        parts.append(_blob(rng.uniform(-extent, extent, 3) * np.array([1, 1, 0.05]), int(rng.integers(*per)), spread, rng))
    if outliers:
        o = rng.uniform(-extent, extent, (outliers, 3)) * np.array([1, 1, 0.05])
        parts.append(np.concatenate([o, np.full((outliers, 1), 230.0)], -1))
    c = np.concatenate(parts).astype(np.float32)
    return c[rng.permutation(c.shape[0])]


def _stack(center, n, intensity=200.0):
    return np.concatenate([np.tile(np.asarray(center, np.float64), (n, 1)), np.full((n, 1), intensity)], -1)


def _bright_exactly(rng, m, dim=300):
    """m bright points (tight blobs of up to 40 and a few strays) among `dim` dim ones, shuffled."""
    parts = [_blob((0, 0, 0), dim, 5.0, rng, intensity=20.0)]
    left, k = m, 0
    while left > 0:
        n = min(left, 40 if k % 3 else 23)
        parts.append(_blob((1.5 * (k % 9) - 6.0, 1.3 * (k // 9) - 4.0, 0.3), n, 0.03 if n > 1 else 0.0, rng))
        left -= n
        k += 1
    c = np.concatenate(parts).astype(np.float32)
    return c[rng.permutation(c.shape[0])]


def _lattice(n_blobs, rng):
    """blobs of 16 coincident points on a 17-wide integer lattice: every point has 15 neighbours at 0 and 15 at exactly 1, so every mean
    distance is exactly 0.5 and every point is kept; all accepted clusters have one size: the order is by label alone."""
    pts = np.concatenate([_stack((i % 17, i // 17, 0.0), 16) for i in range(n_blobs)])
    return pts[rng.permutation(pts.shape[0])].astype(np.float32)


def _line(rng, shuffled):
    line = np.stack([0.15 * np.arange(150), np.full(150, -3.0), np.full(150, 0.5), np.full(150, 200.0)], -1)
    c = np.concatenate([line, _blob((4.0, 5.0, 0.3), 40, 0.03, rng)]).astype(np.float32)
    return c[rng.permutation(c.shape[0])] if shuffled else c


def _case(name, cloud, intensity_min=160.0, s2b=(0.0, 0.0, 0.0), witness=True, **claims):
    return dict(name=name, cloud=np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4), intensity_min=float(intensity_min),
                s2b=tuple(float(v) for v in s2b), witness=witness, claims=claims)


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of dict(name, cloud, intensity_min, s2b, witness, claims).  claims: any of K, M, M2, status (a per-cloud refusal)."""
    from reflector_ekf_slam_amd import synth
    rng = np.random.default_rng(2103)
    out = []
    base = _scene(rng, 14, dim=1500)
    for n in SIZES:                                                   # N = n: a scene cut off after n points
        out.append(_case(f"N_{n}", base[:n]))
    for n in SIZES:                                                   # M = n: exactly n survivors of the gate
        if n:
            out.append(_case(f"M_{n}", _bright_exactly(rng, n), M=n))
    out.append(_case("nothing_bright", _blob((0, 0, 0), 700, 5.0, rng, intensity=20.0), M=0, K=0))
    out.append(_case("one_bright_point", np.concatenate([_blob((0, 0, 0), 100, 5.0, rng, intensity=20.0), [[1.0, 2.0, 0.1, 250.0]]]), M=1, K=0))
    out.append(_case("bright_in_last_tile", np.concatenate([_blob((0, 0, 0), 40000 - 73, 6.0, rng, 20.0), _blob((3, 3, 0.2), 40, 0.03, rng),
                                                            _blob((-4, 2, 0.4), 33, 0.03, rng)]), M=73, K=2))
    out.append(_case("thirty_clusters", _scene(rng, 30)))
    out.append(_case("twelve_clusters_moved", _scene(rng, 12), intensity_min=100.0, s2b=S2B_OTHER))
    out.append(_case("twenty_clusters_high_gate", _scene(rng, 20), intensity_min=215.0, s2b=(-1.5, 0.25, -2.9)))
    g = np.random.Generator(np.random.PCG64(3))
    lms = synth.make_world(synth.C4, g)
    out.append(_case("world_16_rings", synth.make_point_cloud(lms, (34.4, 34.0, 1.15), g), M=3632, K=89))
    # the size gate [4, 160] from both sides
    out.append(_case("gate_160_161", np.concatenate([_stack((1.0, 2.0, 0.3), 160), _stack((-3.0, 0.5, 0.2), 161)])[rng.permutation(321)],
                     M=321, M2=321, K=1))
    out.append(_case("gate_3_4_5", np.concatenate([_blob((0, 0, 0), 200, 5.0, rng, 20.0), _blob((2, 2, 0.1), 3, 0.01, rng),
                                                   _blob((-2, 1, 0.1), 4, 0.01, rng), _blob((0, -3, 0.1), 5, 0.01, rng)]), M=12, M2=12, K=2))
    # equal sizes and the limit of 256 clusters
    out.append(_case("lattice_256", _lattice(256, rng), M=4096, M2=4096, K=256))
    out.append(_case("lattice_257", _lattice(257, rng), M=4112, status=CAPACITY))
    # a component whose graph is 150 hops across
    out.append(_case("line_shuffled", _line(rng, True), M=190, K=2))
    out.append(_case("line_in_order", _line(rng, False), M=190, K=2))
    # the cluster tolerance: squared float32 distance < (float) 0.04
    for d, k in ((0.19999, 1), (0.2, 2), (0.20001, 2)):
        out.append(_case(f"tolerance_{d}", np.concatenate([_stack((0.0, 0.0, 0.0), 20), _stack((d, 0.0, 0.0), 20)]), M=40, M2=40, K=k))
    c = _scene(rng, 20)
    c[100:110, :3] = np.nan
    c[200:240, :3] = c[200, :3]
    c[100:110, 3] = 200.0
    out.append(_case("non_finite_and_coincident", c, witness=False))
    # the cap: exactly MAX_BRIGHT survivors run, one more is refused with the true count
    big = _scene(rng, 104, dim=3000, per=(40, 70), outliers=200)
    bright = np.flatnonzero(big[:, 3] > 170.0)
    assert bright.size > MAX_BRIGHT + 100
    keep = np.ones(big.shape[0], bool)
    keep[bright[MAX_BRIGHT:]] = False
    out.append(_case("exactly_max_bright", big[keep], intensity_min=170.0, M=MAX_BRIGHT))
    keep[bright[MAX_BRIGHT]] = True
    out.append(_case("max_bright_plus_1", big[keep], intensity_min=170.0, M=MAX_BRIGHT + 1, status=CAPACITY))
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


_ORACLE = {}


def oracle(case, max_centers=MAX_CENTERS):
    """-> (status, centres [K, 2], M, M2) as the fleet detector must report the cloud: the oracle's centres, or the per-cloud refusal
    (more than MAX_BRIGHT survivors: the batch's own cap, with the oracle's count; more than 256 clusters: the oracle's -2).  Computed
    once per (case, max_centers) and shared."""
    from oracle.binding import oracle_detect3d
    key = (case["name"], max_centers)
    if key not in _ORACLE:
        none = np.zeros((0, 2), np.float32)
        try:
            c, m, m2 = oracle_detect3d(case["cloud"], case["intensity_min"], case["s2b"], max_centers=MAX_CENTERS)
            if m > MAX_BRIGHT:
                res = (CAPACITY, none, m, m2)
            elif c.shape[0] > max_centers:
                res = (BUFFER, none, m, m2)
            else:
                res = (0, c, m, m2)
        except ValueError:
            m = int((case["cloud"][:, 3].astype(np.float64) > case["intensity_min"]).sum())
            res = (CAPACITY, none, m, None)
        _ORACLE[key] = res
    return _ORACLE[key]


# ---- many small clouds in one launch
def many_small(count=300):
    """`count` members, a cloud of 150..400 points each with one or two tight blobs (and per-member gates and transforms)."""
    rng = np.random.default_rng(515)
    out = []
    for m in range(count):
        n_dim = 150 + (m * 7) % 200
        parts = [_blob((0, 0, 0), n_dim, 4.0, rng, 20.0), _blob((1.0 + 0.01 * m, -2.0, 0.2), 12 + m % 30, 0.02, rng)]
        if m % 3 == 0:
            parts.append(_blob((-3.0, 0.5 + 0.01 * m, 0.4), 5 + m % 11, 0.02, rng))
        c = np.concatenate(parts).astype(np.float32)
        out.append(_case(f"small_{m}", c[rng.permutation(c.shape[0])], intensity_min=150.0 + (m % 4) * 10.0,
                         s2b=(0.01 * (m % 5), -0.02 * (m % 3), 0.1 * (m % 7))))
    return out


# ---- end to end: six robots, forty ticks, one 16-ring sweep of 14 400 points per robot and tick
def e2e_sessions():
    from tests import fleet_detect_cases
    return fleet_detect_cases.e2e_sessions()


def e2e_ticks(sessions):
    """-> ticks: [per member: (odometry event indices, scan event index, cloud)], E2E_TICKS of them."""
    from reflector_ekf_slam_amd import synth
    rngs = [np.random.Generator(np.random.PCG64(177 + i)) for i in range(len(sessions))]
    pos = [0] * len(sessions)
    ticks = []
    for _ in range(E2E_TICKS):
        tick = []
        for i, s in enumerate(sessions):
            od = []
            while s.ev_type[pos[i]] == synth.EV_ODOM:
                od.append(pos[i]); pos[i] += 1
            e = pos[i]; pos[i] += 1
            tick.append((od, e, synth.make_point_cloud(s.landmarks, s.true_pose[e], rngs[i], n_az=900, max_range=12.0)))
        ticks.append(tick)
    return ticks
