"""Cases of the 3D detector sweep: cluster sizes, arrival orders, rankings, Morton stretches and survivor counts that the other 3D
fixtures (random scenes with clusters of at most about 70 points; tests/fleet_detect3d_cases.py, tests/test_detect3d_paths_gpu.py)
never produce, each with its claims.  tests/test_detect3d_sweep_cpu.py holds the C oracle to the witness on every case, every case
to its claims and shows which planted defect which case catches; tests/test_detect3d_sweep_gpu.py holds both kernel chains of
csrc/det3d.hip and the batch kernel of csrc/det3d_batch.hip to the oracle bit for bit.
Reference: src/reflector_detect/point_cloud/point_cloud_reflector_detect.cc:9-106.

A case is fleet_detect3d_cases._case: ``dict(name, cloud, intensity_min, s2b, witness, claims)``.  Claims (all checked by
``check_claims`` on the WITNESS's detail output when the table is generated, so a case that does not hold the edge it names fails
on the CPU):
  M, M2, K          survivors of the gate, of the outlier removal, accepted clusters;
  status            the per-cloud refusal (257 accepted clusters);
  sizes             the sizes of ALL components of the kept points, accepted or not, sorted;
  order_sensitive   for every accepted cluster of 64 members or more the float32 x-sum in ascending-x order differs in bits from
                    the sum in arrival order (and so does the centre the witness would give);
  members           {root node: member nodes} -- a node is a survivor's position among the gate's survivors, in arrival order;
  roots             nodes that are roots (first members) of accepted clusters;
  last_64           a cluster lies wholly within the last 64 nodes;
  reversed_x        the cluster with this root arrives in strictly descending x;
  rows              the input rows of a cluster's members (they cross an input tile of 1024 rows);
  interleaved       the labels of every two equal-size groups interleave;
  tie_d2            the squared float32 distance between the two stacks IS (float) 0.04;
  dist_equals_thr   every mean distance equals the threshold;
  stretch           on the INITIAL sorting grid (a fresh handle's first cloud) the members of the cluster with this root lie in all four
                    cells around the grid's centre, and more than `stretch` Morton-sorted positions lie between its first and last.

How exact sizes are had: the outlier removal takes about a quarter of a Gaussian blob, so STRAYS isolated bright points tens of metres
apart lift mean + 0.5 sigma of the mean-neighbour distances to metres: every blob point is kept, exactly the strays go.

All coordinates of a cloud's bright points are distinct (asserted), except in the two `ties` cases, which are stacks of coincident points.  No case is witness=False: the kd-tree witness takes 0.2 s on the
largest cloud (8193 survivors) and under two seconds on the whole table."""
from __future__ import annotations

import functools

import numpy as np

from tests import fleet_detect3d_cases as FC
from tests.fleet_detect3d_cases import CAPACITY, MAX_BRIGHT, _case

f32 = np.float32
DIM, STRAY = -1, -2
STRAYS, STRAY_PITCH = 40, 50.0
SPREAD = 0.012
FAMILIES = ("sizes", "arrival", "rank", "stretch", "tiles", "ties")
SIZES_ALL = (3, 4, 5, 63, 64, 65, 127, 128, 129, 157, 158, 159, 160, 161)
SIZES_ALONE = (65, 129, 160)
RANK_K = (63, 64, 65, 77, 255, 256, 257)
TILES_M = tuple(m + d for m in (32, 64, 96, 2048, 4096, 5120, 8192) for d in (-1, 0, 1))
GRID_G, GRID_X0, GRID_INV = 128, -32.0, 2.0  # det3d.hip: the grid of a fresh handle's first cloud (gx0 = gy0 = -32, 128 cells of 0.5 m)
STRETCH_MIN = 2048                           # k3_clusters gathers 1024 sorted positions a round: more than 2048 is three rounds


# ---------------------------------------------------------------------------------------------------------------- helpers
def sum_f32(v):
    """float32 running sum in the given order (compute3DCentroid)."""
    s = f32(0.0)
    for x in np.asarray(v, f32):
        s = f32(s + x)
    return s


def sensitive(x):
    """The float32 sum of x in the given (arrival) order differs in bits from the sum in ascending order."""
    x = np.asarray(x, f32)
    return sum_f32(x).tobytes() != sum_f32(np.sort(x, kind="stable")).tobytes()


def cell_code(x, y, gx0=GRID_X0, gy0=GRID_X0, ginv=GRID_INV, G=GRID_G):
    """det3d.hip's cell_code restated: float32 (x - gx0) * ginv clamped to [0, G - 1], truncated, bits interleaved (x even, y odd)."""
    def cell(v, g0):
        f = (np.asarray(v, f32) - f32(g0)) * f32(ginv)
        return np.minimum(np.maximum(f, f32(0.0)), f32(G - 1)).astype(np.int64)

    def spread(c):
        c = (c | (c << 4)) & 0x0F0F
        c = (c | (c << 2)) & 0x3333
        return (c | (c << 1)) & 0x5555
    return spread(cell(x, gx0)) | (spread(cell(y, gy0)) << 1)


def stray_points(n=STRAYS):
    k = np.arange(n)
    return np.stack([60.0 + STRAY_PITCH * (k % 7), -120.0 + STRAY_PITCH * (k // 7), 0.1 * (k % 3)], -1)


def lattice(k, pitch=1.5, per_row=5, x0=-4.0, y0=-3.0, z=0.3):
    return (x0 + pitch * (k % per_row), y0 + pitch * (k // per_row), z)


def fill(rng, tags, blobs, dim_spread=5.0):
    """The cloud whose row r is a member of blob tags[r] (>= 0), a stray or a dim point.  blobs[b]: (centre, spread) -- Gaussian points,
    drawn again until a blob of 64 or more is order-sensitive in ITS arrival order -- or an array of explicit points in arrival order."""
    tags = np.asarray(tags)
    cloud = np.zeros((tags.size, 4))
    nd = int((tags == DIM).sum())
    cloud[tags == DIM, :3] = rng.normal(0, dim_spread, (nd, 3))
    cloud[tags == DIM, 3] = 20.0
    ns = int((tags == STRAY).sum())
    cloud[tags == STRAY, :3] = stray_points(ns)
    cloud[tags == STRAY, 3] = 230.0
    for b, spec in enumerate(blobs):
        rows = np.flatnonzero(tags == b)
        if isinstance(spec, np.ndarray):
            pts = spec
        else:
            centre, spread = spec
            for _ in range(50):
                pts = (rng.normal(0, spread, (rows.size, 3)) + np.asarray(centre)).astype(f32)
                if rows.size < 64 or sensitive(pts[:, 0]):
                    break
            else:
                raise AssertionError("no order-sensitive draw")
        assert pts.shape == (rows.size, 3), (b, pts.shape, rows.size)
        cloud[rows, :3] = pts
        cloud[rows, 3] = 200.0
    cloud = cloud.astype(f32)
    bright = cloud[tags != DIM, :3]
    assert np.unique(bright, axis=0).shape[0] == bright.shape[0]
    return cloud


def shuffled_tags(rng, sizes, dim, strays):
    tags = np.concatenate([np.full(n, b) for b, n in enumerate(sizes)] + [np.full(strays, STRAY), np.full(dim, DIM)])
    return tags[rng.permutation(tags.size)]


def weave(rng, bright_tags, dim):
    """The bright rows in the given order with `dim` dim rows at random places between them: the nodes are the bright rows' positions."""
    tags = np.full(len(bright_tags) + dim, DIM)
    at = np.sort(rng.choice(tags.size, len(bright_tags), replace=False))
    tags[at] = bright_tags
    return tags


def strays_for(sizes):
    """40 strays; 12 where the blobs hold fewer than 200 points (a third of the cloud as strays would lift the threshold above the
    innermost strays' own distances, and those would be kept)."""
    return STRAYS if sum(sizes) >= 200 else 12


def exact(rng, sizes, dim=500, centres=None, spread=SPREAD, **kw):
    """Blobs of exactly these sizes (shuffled among strays and dim points), on a lattice of 1.5 m."""
    centres = centres or [lattice(k, **kw) for k in range(len(sizes))]
    return fill(rng, shuffled_tags(rng, sizes, dim, strays_for(sizes)), [(c, spread) for c in centres])


def size_claims(sizes):
    strays = strays_for(sizes)
    acc = [n for n in sizes if 4 <= n <= 160]
    return dict(M=sum(sizes) + strays, M2=sum(sizes), K=len(acc), sizes=sorted(sizes), order_sensitive=any(n >= 64 for n in acc))


# ---------------------------------------------------------------------------------------------------------------- the families
def _sizes(rng):
    out = [_case("sizes_all", exact(rng, SIZES_ALL), **size_claims(SIZES_ALL))]
    for n in SIZES_ALONE:                                            # (129 behind another gate and a turned sensor_to_base_link)
        other = dict(intensity_min=100.0, s2b=FC.S2B_OTHER) if n == 129 else {}
        out.append(_case(f"sizes_alone_{n}", exact(rng, (n,), dim=300), **other, **size_claims((n,))))
    return out


def _arrival(rng):
    out = []
    # two clusters of 80 whose members alternate: nodes 2k and 2k + 1, every run of one component has length 1
    bright = [k % 2 for k in range(160)] + [STRAY] * strays_for((80, 80))
    cloud = fill(rng, weave(rng, bright, 400), [((1.0, 2.0, 0.3), SPREAD), ((-2.0, -1.0, 0.2), SPREAD)])
    out.append(_case("arrival_alternating_80_80", cloud, **size_claims((80, 80)),
                     members={0: list(range(0, 160, 2)), 1: list(range(1, 160, 2))}))
    # roots 63 and 64 (alternating members from there), and a cluster wholly within the last 64 nodes of more than 1024
    bright = [0] * 63 + [1 + k % 2 for k in range(40)]
    sizes = [63, 20, 20]
    for b in range(25):
        bright += [3 + b] * 40
        sizes.append(40)
    bright += [STRAY] * STRAYS + [28] * 30
    sizes.append(30)
    cloud = fill(rng, weave(rng, bright, 700), [(lattice(k, per_row=6), SPREAD) for k in range(len(sizes))])
    m = len(bright)
    out.append(_case("arrival_roots_63_64_last_64", cloud, **size_claims(sizes), roots=[0, 63, 64, m - 30],
                     members={63: list(range(63, 103, 2)), 64: list(range(64, 103, 2)), m - 30: list(range(m - 30, m))}, last_64=m - 30))
    assert m > 1024
    # a line of 100 points, 0.05 m apart, that arrives from its far end: the spatial order exactly reversed
    n = 100
    for _ in range(50):
        line = np.stack([3.7 - 0.05 * np.arange(n) + rng.uniform(-0.01, 0.01, n), rng.normal(1.3, 0.01, n), rng.normal(0.4, 0.01, n)], -1).astype(f32)
        if sensitive(line[:, 0]) and np.all(np.diff(line[:, 0]) < 0):
            break
    bright = [0] * n + [1] * 30 + [STRAY] * strays_for((100, 30))
    cloud = fill(rng, weave(rng, bright, 400), [line, ((-3.0, -2.0, 0.2), SPREAD)])
    out.append(_case("arrival_reversed_line_100", cloud, **size_claims((100, 30)), reversed_x=0, members={0: list(range(n))}))
    # 40 members on input rows 1004 .. 1043: the bright run crosses the 1024-row input tile
    for N in (2048, 2049):
        tags = np.full(N, DIM)
        tags[1004:1044] = 0
        free = np.concatenate([np.arange(1004), np.arange(1044, N)])
        other = rng.choice(free, 20 + strays_for((40, 20)), replace=False)
        tags[other[:20]] = 1
        tags[other[20:]] = STRAY
        cloud = fill(rng, tags, [((2.0, 1.0, 0.3), SPREAD), ((-1.0, 3.0, 0.2), SPREAD)])
        out.append(_case(f"arrival_rows_1004_1043_of_{N}", cloud, **size_claims((40, 20)), rows=list(range(1004, 1044))))
    return out


def _rank(rng):
    groups = [12] * 5 + [9] * 6 + [6] * 7
    out = [_case("rank_equal_size_groups", exact(rng, groups, pitch=0.6, per_row=6), **size_claims(groups), interleaved=True)]
    for K in RANK_K:
        sizes = [4 + (7 * i + i // 17) % (8 if K < 200 else 6) for i in range(K)]
        cloud = exact(rng, sizes, dim=600, pitch=0.6, per_row=17, x0=-5.0, y0=-5.0)
        cl = size_claims(sizes)
        if K > FC.MAX_CENTERS:
            cl["status"] = CAPACITY
        out.append(_case(f"rank_K_{K}", cloud, **cl))
    return out


def _stretch(rng):
    out = []
    for n in (60, 160):
        sizes = [n] + [31] * 72
        centres = [(0.0, 0.0, 0.3)]
        for k in range(36):
            x, y = 3.0 + 4.0 * (k % 6), 3.0 + 4.0 * (k // 6)
            centres += [(x, -y, 0.3), (-x, y, 0.3)]                  # the two middle quadrants of the Morton order
        bright = [0] * n
        rest = np.concatenate([np.full(31, b) for b in range(1, 73)] + [np.full(STRAYS, STRAY)])
        tags = weave(rng, np.concatenate([bright, rest])[rng.permutation(n + rest.size)], 500)
        cloud = fill(rng, tags, [(c, SPREAD) for c in centres])
        root = int(np.flatnonzero(tags[tags != DIM] == 0)[0])
        out.append(_case(f"stretch_{n}", cloud, **size_claims(sizes), stretch=(root, STRETCH_MIN)))
    return out


def _tiles(rng):
    return [_case(f"tiles_M_{m}", FC._bright_exactly(rng, m), M=m) for m in TILES_M]


def tie_offset():
    """-> float32 (dx, dy) with ((dx * dx) + dy * dy) + 0 == (float) 0.04 in float32 arithmetic: a pair EXACTLY on the cluster tolerance."""
    tol2 = f32(0.2 * 0.2)
    for k in range(1, 4000):
        dy = f32(k) * f32(2.0 ** -16)
        dx = np.sqrt(f32(tol2 - f32(dy * dy)))
        for _ in range(8):
            if f32(f32(dx * dx) + f32(dy * dy)) == tol2:
                return dx, dy
            dx = np.nextafter(dx, f32(0.0 if f32(f32(dx * dx) + f32(dy * dy)) > tol2 else 1.0))
    raise AssertionError("no pair on the tolerance")


def _ties(rng):
    """The two comparisons no cloud of distinct random coordinates decides: these two cases hold COINCIDENT points (stacks), and say so."""
    stack = FC._stack
    dx, dy = tie_offset()
    out = [_case("ties_pair_on_the_tolerance", np.concatenate([stack((0.0, 0.0, 0.0), 20), stack((float(dx), float(dy), 0.0), 20)]),
                 M=40, M2=40, K=2, sizes=[20, 20], tie_d2=True)]
    # stacks of 31 and more: every mean distance is 0, so is the threshold: dist > thr keeps all, dist >= thr none
    sizes = (31, 64, 129, 160, 161)
    pts = np.concatenate([stack(lattice(k), n) for k, n in enumerate(sizes)])
    out.append(_case("ties_threshold_equals_every_distance", pts[rng.permutation(pts.shape[0])], M=sum(sizes), M2=sum(sizes), K=4,
                     sizes=sorted(sizes), dist_equals_thr=True))
    return out


# ---------------------------------------------------------------------------------------------------------------- claims
_DETAIL = {}


def detail(case):
    """The witness's detail output for a case, computed once and shared (None for a case with witness=False: there is none today)."""
    from tests.witness.detect3d_witness import detect3d_witness_detail
    if not case["witness"]:
        return None
    if case["name"] not in _DETAIL:
        _DETAIL[case["name"]] = detect3d_witness_detail(case["cloud"], case["intensity_min"], case["s2b"])
    return _DETAIL[case["name"]]


def stretch_of(case, d, root):
    """-> (the four cells' codes the cluster has members in, a lower bound of last - first + 1 in the Morton-sorted copy on the
    initial grid: the survivors whose code lies strictly between the cluster's smallest and largest, and those two members)."""
    pts = case["cloud"][d.rows]
    code = cell_code(pts[:, 0], pts[:, 1])
    mem = next(nodes for nodes, _ in d.components if int(nodes[0]) == root)
    lo, hi = int(code[mem].min()), int(code[mem].max())
    return sorted(set(int(c) for c in code[mem])), int(((code > lo) & (code < hi)).sum()) + 2


def check_claims(case, d=None):
    cl, name = case["claims"], case["name"]
    gate = int((case["cloud"][:, 3].astype(np.float64) > case["intensity_min"]).sum())
    if "M" in cl:
        assert gate == cl["M"], (name, gate)
    d = d if d is not None else detail(case)
    if d is None:
        assert set(cl) <= {"M"}, name
        return
    pts = case["cloud"][d.rows]
    comps = {int(nodes[0]): nodes for nodes, _ in d.components}
    accepted = [d.components[k][0] for k in d.order]
    for key, got in (("M", d.M), ("M2", d.M2), ("K", d.centers.shape[0])):
        if key in cl:
            assert got == cl[key], (name, key, got, cl[key])
    if "sizes" in cl:
        assert sorted(n.size for n, _ in d.components) == cl["sizes"], name
        assert [n.size for n in accepted] == sorted((n for n in cl["sizes"] if 4 <= n <= 160), reverse=True), name
    if cl.get("order_sensitive"):
        big = [n for n in accepted if n.size >= 64]
        assert big, name
        for n in big:
            assert sensitive(pts[n, 0]), (name, n.size)
    for root, nodes in cl.get("members", {}).items():
        assert root in comps and comps[root].tolist() == list(nodes), (name, root)
    for root in cl.get("roots", []):
        assert any(int(n[0]) == root for n in accepted), (name, root)
    if "last_64" in cl:
        assert d.M > 1024 and comps[cl["last_64"]].min() >= d.M - 64, name
    if "reversed_x" in cl:
        assert np.all(np.diff(pts[comps[cl["reversed_x"]], 0]) < 0), name
    if "rows" in cl:
        assert any(d.rows[n].tolist() == cl["rows"] for n in accepted), name
        assert cl["rows"][0] < 1024 <= cl["rows"][-1]
    if cl.get("interleaved"):
        by = {}
        for n in accepted:
            by.setdefault(n.size, []).append(int(n[0]))
        assert len(by) >= 3 and all(len(v) >= 3 for v in by.values()), name
        spans = [(min(v), max(v)) for v in by.values()]
        assert all(a[0] < b[1] and b[0] < a[1] for a in spans for b in spans), (name, spans)
    if cl.get("tie_d2"):
        first, second = sorted(comps)                                # (the two stacks' roots)
        dxy = (pts[first] - pts[second]).astype(f32)
        assert f32(f32(f32(dxy[0] * dxy[0]) + f32(dxy[1] * dxy[1])) + f32(dxy[2] * dxy[2])) == f32(0.2 * 0.2), name
    if cl.get("dist_equals_thr"):
        assert np.all(d.dist.astype(np.float64) == d.thr), name
    if "stretch" in cl:
        root, least = cl["stretch"]
        cells, length = stretch_of(case, d, root)
        centre = [int(cell_code(x, y)) for x, y in ((-0.1, -0.1), (0.1, -0.1), (-0.1, 0.1), (0.1, 0.1))]
        assert cells == sorted(centre), (name, cells)
        assert length > least, (name, length)


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of cases, every one checked against its claims."""
    rng = np.random.default_rng(3107)
    out = []
    for family in (_sizes, _arrival, _rank, _stretch, _tiles, _ties):
        out += family(rng)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names) and all(n.split("_")[0] in FAMILIES for n in names)
    for c in out:
        assert c["claims"], c["name"]
        check_claims(c)
    return tuple(out)


def family(name):
    return tuple(c for c in cases() if c["name"].startswith(name + "_"))


def oracle(case, max_centers=FC.MAX_CENTERS):
    """(status, centres, M, M2) as fleet_detect3d_cases.oracle states them (the BATCH's answer: more than MAX_BRIGHT survivors is refused)."""
    return FC.oracle(case, max_centers)


_SINGLE = {}


def oracle_single(case):
    """(status, centres, M) as a single handle must answer: the oracle's centres whatever M, the capacity refusal beyond 256 clusters."""
    from oracle.binding import oracle_detect3d
    if case["name"] not in _SINGLE:
        try:
            c, m, _ = oracle_detect3d(case["cloud"], case["intensity_min"], case["s2b"])
            _SINGLE[case["name"]] = (0, c, m)
        except ValueError:
            m = int((case["cloud"][:, 3].astype(np.float64) > case["intensity_min"]).sum())
            _SINGLE[case["name"]] = (CAPACITY, np.zeros((0, 2), f32), m)
    return _SINGLE[case["name"]]
