"""The 3D detector sweep on the CPU (cases: tests/detect3d_sweep_cases.py): every case's claims hold on the witness's detail output;
oracle/detect3d_oracle.c equals the independent witness tests/witness/detect3d_witness.py BIT FOR BIT on every case (centres, M, M2);
the table holds every size, count and edge it was built for; and eight one-line defects, each planted in a scratch build of the oracle,
change the centres or counts of at least one sweep case -- CAUGHT_BY records which, and which the 3D cases that existed before do.
Nothing here launches a kernel.  Reference: src/reflector_detect/point_cloud/point_cloud_reflector_detect.cc:9-106."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import detect3d_sweep_cases as SC
from tests import fleet_detect3d_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_C = os.path.join(ROOT, "oracle", "detect3d_oracle.c")

SUM_LOOP = """            for (int i = 0; i < M2; ++i)                                 /* ascending index order */
                if (label[i] == c) { cx += q[3 * i]; cy += q[3 * i + 1]; cz += q[3 * i + 2]; }
"""
# the members gathered and sorted by x (insertion sort, stable), then summed in that order; `queue` is free by then
SUM_BY_X = """            { int n_ = 0;
              for (int i = 0; i < M2; ++i) if (label[i] == c) queue[n_++] = i;
              if (%s)
                  for (int a_ = 1; a_ < n_; ++a_) { const int v_ = queue[a_]; int b_ = a_;
                      while (b_ > 0 && q[3 * queue[b_ - 1]] > q[3 * v_]) { queue[b_] = queue[b_ - 1]; --b_; } queue[b_] = v_; }
              for (int k_ = 0; k_ < n_; ++k_) { const int i = queue[k_]; cx += q[3 * i]; cy += q[3 * i + 1]; cz += q[3 * i + 2]; } }
"""
# defect -> (the oracle's text, what a slip would leave in its place)
DEFECTS = {
    "sum_ascending_x": (SUM_LOOP, SUM_BY_X % "1"),
    "sum_ascending_x_over_128": (SUM_LOOP, SUM_BY_X % "n_ > 128"),
    "size_gate_below_160": ("qn <= O3_MAX", "qn < O3_MAX"),
    "size_gate_above_4": ("qn >= O3_MIN", "qn > O3_MIN"),
    "ties_by_largest_member": ("if (queue[k] < mn) mn = queue[k];", "if (queue[k] > mn) mn = queue[k];"),
    "dist_ge_thr": ("if (!(dist[i] > thr))", "if (!(dist[i] >= thr))"),
    "tolerance_le": ("d2f(q + 3 * s, q + 3 * j) < tol2", "d2f(q + 3 * s, q + 3 * j) <= tol2"),
    "thirty_smallest": ("for (int k = 1; k < O3_MEAN_K + 1; ++k) dist_sum", "for (int k = 1; k < O3_MEAN_K; ++k) dist_sum"),
}

# MEASURED (test_every_planted_defect_is_caught prints the full lists): the sweep cases each defect changes, and whether any cloud of
# fleet_detect3d_cases.cases() ("fleet") or of test_detect3d_paths_gpu._clouds() ("paths": the only clouds the long chain saw) does.
CAUGHT_BY = {
    "sum_ascending_x": dict(sweep=("sizes_all", "sizes_alone_65", "sizes_alone_129", "sizes_alone_160", "arrival_alternating_80_80",
                                   "arrival_roots_63_64_last_64", "arrival_reversed_line_100", "arrival_rows_1004_1043_of_2048", "rank_K_256",
                                   "stretch_60", "stretch_160", "tiles_M_8193"), fleet=True, paths=True),
    "sum_ascending_x_over_128": dict(sweep=("sizes_all", "sizes_alone_129", "sizes_alone_160", "stretch_160"), fleet=True, paths=True),
    "size_gate_below_160": dict(sweep=("sizes_all", "sizes_alone_160", "stretch_160", "ties_threshold_equals_every_distance"), fleet=True, paths=False),
    "size_gate_above_4": dict(sweep=("sizes_all", "rank_K_63", "rank_K_64", "rank_K_65", "rank_K_77", "rank_K_255", "rank_K_256", "rank_K_257"),
                              fleet=True, paths=True),
    "ties_by_largest_member": dict(sweep=("rank_equal_size_groups", "rank_K_63", "rank_K_64", "rank_K_65", "rank_K_77", "rank_K_255", "rank_K_256",
                                          "stretch_60", "stretch_160", "tiles_M_8193"), fleet=True, paths=True),
    "dist_ge_thr": dict(sweep=("ties_pair_on_the_tolerance", "ties_threshold_equals_every_distance"), fleet=True, paths=False),
    "tolerance_le": dict(sweep=("ties_pair_on_the_tolerance",), fleet=False, paths=False),
    "thirty_smallest": dict(sweep=("tiles_M_2047", "tiles_M_2048"), fleet=True, paths=True),
}
# the older clouds that hold a cluster of more than 128 points: the simulated worlds (a reflector close to the lidar), and no other
OVER_128_OLDER = ("world_16_rings", "paths_world_16_rings", "paths_world_32_rings")


def _run(lib, case):
    """One cloud through a build of the oracle -> (K or the refusal, centres' bytes, M, M2)."""
    pts = case["cloud"]
    out = np.zeros((FC.MAX_CENTERS, 2), np.float32)
    s2b = (C.c_double * 3)(*case["s2b"])
    m, m2 = C.c_int(0), C.c_int(0)
    k = lib.od3_handle_cloud_ex(C.c_double(case["intensity_min"]), s2b, pts.ctypes.data_as(C.c_void_p), pts.shape[0],
                                out.ctypes.data_as(C.c_void_p), FC.MAX_CENTERS, C.byref(m), C.byref(m2))
    return k, out[:max(k, 0)].tobytes(), m.value, m2.value


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """-> {defect or None: a scratch build of oracle/detect3d_oracle.c with that one text replaced}, compiled as oracle/Makefile does."""
    text = open(ORACLE_C).read()
    d = tmp_path_factory.mktemp("oracle3d")
    libs = {}
    for name, (old, new) in [(None, ("", ""))] + list(DEFECTS.items()):
        if name is not None:
            assert text.count(old) == 1, name
        src = d / f"o3_{name}.c"
        src.write_text(text.replace(old, new) if name else text)
        so = str(d / f"o3_{name}.so")
        subprocess.run([os.environ.get("CC", "gcc"), "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c11", str(src), "-o", so, "-lm"],
                       check=True, capture_output=True)
        libs[name] = C.CDLL(so)
        libs[name].od3_handle_cloud_ex.restype = C.c_int
    return libs


def _older_clouds():
    """The 3D clouds that existed before the sweep, as cases: those of the fleet suite and those both chains were forced through."""
    from tests import test_detect3d_paths_gpu as P
    fleet = [c for c in FC.cases() if np.isfinite(c["cloud"]).all()]
    paths = [FC._case("paths_" + k, v) for k, v in P._clouds().items() if np.isfinite(v).all()]
    return fleet, paths


def test_every_case_is_what_it_claims_to_be():
    for c in SC.cases():
        assert c["claims"] and c["witness"], c["name"]
        SC.check_claims(c)


def test_oracle_equals_the_witness_on_every_case(oracle_lib):
    for c in SC.cases():
        d = SC.detail(c)
        status, cen, m = SC.oracle_single(c)
        assert status == c["claims"].get("status", 0), c["name"]
        assert m == d.M, c["name"]
        if status:
            assert d.centers.shape[0] > FC.MAX_CENTERS and m <= FC.MAX_BRIGHT, c["name"]     # (refused for its clusters alone)
            continue
        m2 = SC.oracle(c)[3]
        assert m2 == d.M2 and cen.shape == d.centers.shape, (c["name"], m2, d.M2, cen.shape, d.centers.shape)
        assert np.array_equal(cen.view(np.uint32), d.centers.view(np.uint32)), c["name"]


def test_the_table_holds_what_it_was_built_for():
    cases = SC.cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for f in SC.FAMILIES:
        assert SC.family(f), f
    acc = lambda c: [n.size for n, ok in SC.detail(c).components if ok]
    every = lambda c: [n.size for n, _ in SC.detail(c).components]
    by = {c["name"]: c for c in cases}
    # sizes: all of them in one cloud (3 and 161 as components that are refused), 65 / 129 / 160 alone
    assert sorted(every(by["sizes_all"])) == sorted(SC.SIZES_ALL) and sorted(acc(by["sizes_all"])) == [n for n in SC.SIZES_ALL if 4 <= n <= 160]
    for n in SC.SIZES_ALONE:
        assert acc(by[f"sizes_alone_{n}"]) == [n]
    # every place count of arrival_places<1 | 2 | 3> and every scalar tail (size % 4) on a large cluster
    big = sorted(n for c in cases for n in acc(c) if n > 64)
    assert {65, 80, 100, 127, 128} <= set(big) and {129, 157, 158, 159, 160} <= set(big) and {n % 4 for n in big if n > 128} == {0, 1, 2, 3}
    # order-sensitive sums: every accepted cluster of 64 or more outside the stacks
    n_sensitive = 0
    for c in cases:
        d = SC.detail(c)
        pts = c["cloud"][d.rows]
        for k in d.order:
            nodes = d.components[k][0]
            if nodes.size >= 64 and not c["name"].startswith(("ties", "tiles")):
                assert c["claims"].get("order_sensitive") and SC.sensitive(pts[nodes, 0]), (c["name"], nodes.size)
                n_sensitive += 1
    assert n_sensitive >= 16
    # ranks
    ks = {SC.detail(c).centers.shape[0] for c in SC.family("rank")}
    assert set(SC.RANK_K) <= ks and {63, 64, 65, 77, 255, 256} <= ks
    for k in (255, 256, 257):
        assert len(set(acc(by[f"rank_K_{k}"]))) >= 5
    assert by["rank_K_257"]["claims"]["status"] == FC.CAPACITY
    # stretches: both, beyond two gather rounds on the initial grid
    for c in SC.family("stretch"):
        root, least = c["claims"]["stretch"]
        cells, length = SC.stretch_of(c, SC.detail(c), root)
        assert len(cells) == 4 and length > least == 2048, (c["name"], cells, length)
    assert [max(acc(c)) for c in SC.family("stretch")] == [60, 160]
    # survivor counts: the tile, prefetch, statistics-round, chain and query-deal edges from both sides
    ms = [SC.detail(c).M for c in SC.family("tiles")]
    assert ms == list(SC.TILES_M) == [31, 32, 33, 63, 64, 65, 95, 96, 97, 2047, 2048, 2049, 4095, 4096, 4097, 5119, 5120, 5121, 8191, 8192, 8193]
    assert SC.cell_code(np.float32(-32.0), np.float32(-32.0)) == 0 and SC.cell_code(np.float32(31.99), np.float32(-32.0)) == 0x1555
    assert SC.cell_code(np.float32(1e9), np.float32(1e9)) == 0x3FFF and SC.cell_code(np.float32(-0.1), np.float32(0.1)) == 9557


def test_every_planted_defect_is_caught(builds):
    """Each defect, planted in a scratch build of the oracle, against the unchanged build on every sweep case and on the older 3D clouds."""
    fleet, paths = _older_clouds()
    groups = {"sweep": list(SC.cases()), "fleet": fleet, "paths": paths}
    jobs = [(b, g, k) for b in builds for g, cs in groups.items() for k in range(len(cs))]
    jobs.sort(key=lambda j: -groups[j[1]][j[2]]["cloud"].shape[0])                       # (the big clouds first: none is left for the end)
    with ThreadPoolExecutor(8) as pool:                      # (the oracle's loops run outside the interpreter's lock)
        res = dict(zip(jobs, pool.map(lambda j: _run(builds[j[0]], groups[j[1]][j[2]]), jobs)))
    run = lambda b: {g: [res[(b, g, k)] for k in range(len(cs))] for g, cs in groups.items()}
    base = run(None)
    planted = {defect: run(defect) for defect in DEFECTS}
    # the scratch build without a defect IS the oracle
    for c, got in zip(groups["sweep"], base["sweep"]):
        status, cen, m = SC.oracle_single(c)
        assert (got[0] == -2) == (status != 0) and got[2] == m and (status or got[1] == cen.tobytes()), c["name"]
    found = {}
    for defect in DEFECTS:
        found[defect] = {g: [c["name"] for c, want, have in zip(cs, base[g], planted[defect][g]) if have != want] for g, cs in groups.items()}
        print(f"{defect}: sweep {found[defect]['sweep']}; fleet {found[defect]['fleet']}; paths {found[defect]['paths']}")
    for defect, caught in found.items():
        assert caught["sweep"], defect
        rec = CAUGHT_BY[defect]
        missing = [n for n in rec["sweep"] if n not in caught["sweep"]]
        assert not missing, (defect, missing)
        assert bool(caught["fleet"]) == rec["fleet"] and bool(caught["paths"]) == rec["paths"], (defect, caught["fleet"], caught["paths"])
    # the summation order of a cluster larger than 128 was expected to be invisible to the older clouds.  It is not quite: the two simulated
    # worlds hold such a cluster, and world_32_rings took the long chain -- one cluster, one arrival order, one stretch; every other older
    # cloud is blind to it
    over = found["sum_ascending_x_over_128"]
    assert tuple(over["fleet"] + over["paths"]) == OVER_128_OLDER
