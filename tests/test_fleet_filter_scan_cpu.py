"""The fleet voxel filters' C ABI and Python layer without a GPU (rgrid_batch_filter_* of include/rgrid.h, ScanMatchFleet.filter):
the header declares what the library exports, the ctypes mirrors agree with it, a library without the calls is reported on their
first use only -- and the conditions the GPU cases of tests/fleet_filter_scan_cases.py rely on hold in the oracle."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fleet_filter_scan_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rgrid_batch_filter_submit", "rgrid_batch_filter_collect", "rgrid_batch_filter_max_points", "rgrid_batch_sizeof_filter_scan")


def _header():
    text = open(os.path.join(ROOT, "include", "rgrid.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _fields(h, name):
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", h, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]


def test_header_declares_the_calls_and_the_two_structures():
    h = _header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
    assert _fields(h, "rgrid_filter_options") == ["float voxel_filter_size", "double adaptive_max_length, adaptive_min_num_points, adaptive_max_range"]
    assert _fields(h, "rgrid_batch_filter_scan") == ["int n_returns, n_misses", "const float *returns_xy, *misses_xy"]
    assert re.search(r"rgrid_batch_filter_collect\s*\(\s*rgrid_batch_t\s*\*b,\s*int\s*\*status,\s*int\s*\*counts,\s*float\s*\*out_xy,\s*long\s+out_cap_points\s*\)", h)
    assert re.search(r"rgrid_batch_filter_max_points\s*\(\s*void\s*\)", h) and re.search(r"rgrid_batch_sizeof_filter_scan\s*\(\s*void\s*\)", h)


def test_library_exports_them_and_agrees_on_the_layout():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._filter_lib()
    assert not [n for n in NEW if not hasattr(L, n)]
    S, O = M.RgridBatchFilterScan, M._FilterOptions
    assert L.rgrid_batch_sizeof_filter_scan() == C.sizeof(S) == 24
    assert [f[0] for f in S._fields_] == ["n_returns", "n_misses", "returns_xy", "misses_xy"]
    assert (S.n_misses.offset, S.returns_xy.offset, S.misses_xy.offset) == (4, 8, 16)
    assert [f[0] for f in O._fields_] == ["voxel_filter_size", "adaptive_max_length", "adaptive_min_num_points", "adaptive_max_range"]
    assert C.sizeof(O) == 32 and O.adaptive_max_length.offset == 8
    # ScanMatchFleet's default max_points fits one workgroup; the Python helper reports the same limit
    assert L.rgrid_batch_filter_max_points() == M.filter_max_points() >= 8192


def test_abi_version_stays_4():
    from reflector_ekf_slam_amd import fleet_match, grid
    assert int(re.search(r"#define\s+RGRID_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4 == grid.RGRID_ABI_VERSION
    assert fleet_match._filter_lib().rgrid_abi_version() == 4


def test_null_handles_are_refused_with_a_code():
    from reflector_ekf_slam_amd import fleet_match as M
    L = M._filter_lib()
    opt, scan = M._FilterOptions(0.025, 0.9, 500.0, 100.0), M.RgridBatchFilterScan()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    assert L.rgrid_batch_filter_submit(None, C.byref(opt), C.addressof(scan), 1) == M.RGRID_ERR_INVALID
    assert L.rgrid_batch_filter_collect(None, a, a, a, 4) == M.RGRID_ERR_INVALID


class _Without:
    """The built library seen through a filter: without the names in `hidden`, with `replaced` in place of others."""

    def __init__(self, real, hidden=(), replaced=None):
        self._real, self._hidden, self._replaced = real, set(hidden), dict(replaced or {})

    def __getattr__(self, name):
        if name in self._hidden:
            raise AttributeError(name)
        if name in self._replaced:
            return self._replaced[name]
        return getattr(self._real, name)


def test_a_library_without_the_calls_is_reported_by_them_only(monkeypatch):
    from reflector_ekf_slam_amd import _lib
    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.grid import _MatchOptions
    real = M._batch_lib()
    refine, insert = M._refine_lib(), M._insert_lib()
    for hidden in (NEW, NEW[2:3]):
        old = _Without(real, hidden)
        monkeypatch.setattr(M._batch_lib, "ready", old)
        monkeypatch.setattr(M._refine_lib, "ready", None)
        monkeypatch.setattr(M._insert_lib, "ready", None)
        monkeypatch.setattr(M._filter_lib, "ready", None)
        m = object.__new__(M.ScanMatchFleet)                       # a handle as an older library would have made it
        m._L, m._h, m._pending = old, None, None
        for call in (lambda: m.submit_filter_code([]), m.collect_filter_code, lambda: m.filter([]), M.filter_max_points):
            with pytest.raises(_lib.LibraryMissing) as e:
                call()
            assert hidden[0] in str(e.value)
        # the calls it has keep working
        assert M._batch_lib() is old and M._refine_lib() is old and M._insert_lib() is old
        assert m.submit_packed_code(M.ScanMatchFleet.pack([])) == M.RGRID_ERR_INVALID      # (a null handle: refused by the library itself)
        assert m.submit_refine_code([]) == M.RGRID_ERR_INVALID and m.submit_insert_code([]) == M.RGRID_ERR_INVALID
        assert old.rgrid_batch_match_submit(None, C.byref(_MatchOptions(0.2, 0.26, 0.1, 0.1)), None, 0) == M.RGRID_ERR_INVALID
    # a library whose structure has another size
    monkeypatch.setattr(M._batch_lib, "ready", _Without(real, (), {"rgrid_batch_sizeof_filter_scan": lambda: 16}))
    monkeypatch.setattr(M._filter_lib, "ready", None)
    with pytest.raises(_lib.LibraryMissing) as e:
        M._filter_lib()
    assert "16" in str(e.value) and "24" in str(e.value)
    monkeypatch.setattr(M._batch_lib, "ready", real)
    monkeypatch.setattr(M._refine_lib, "ready", refine)
    monkeypatch.setattr(M._insert_lib, "ready", insert)
    monkeypatch.setattr(M._filter_lib, "ready", None)
    assert M._filter_lib() is real


def test_package_exports_and_packing():
    import reflector_ekf_slam_amd as R
    from reflector_ekf_slam_amd import fleet_match as M
    assert R.RgridBatchFilterScan is M.RgridBatchFilterScan and R.FleetFilterResult is M.FleetFilterResult
    assert R.gravity_aligned_scans is M.gravity_aligned_scans
    for name in ("pack_filter", "submit_filter_packed_code", "submit_filter_code", "submit_filter", "collect_filter_code", "collect_filter", "filter"):
        assert callable(getattr(M.ScanMatchFleet, name)), name
    ret = np.arange(6, dtype=np.float64).reshape(3, 2) + 0.1                       # converted to float32
    arr, count, keep = M.ScanMatchFleet.pack_filter([(ret, None), (np.zeros((0, 2)), [[1.0, 2.0]])])
    assert count == 2 and (arr[0].n_returns, arr[0].n_misses) == (3, 0)
    assert arr[0].returns_xy == keep[0].ctypes.data and keep[0].dtype == np.float32 and np.array_equal(keep[0], ret.astype(np.float32))
    assert arr[0].misses_xy is None
    assert (arr[1].n_returns, arr[1].n_misses) == (0, 1) and arr[1].returns_xy is None and arr[1].misses_xy == keep[3].ctypes.data
    assert keep[3].dtype == np.float32 and keep[3].tolist() == [[1.0, 2.0]]
    assert M.ScanMatchFleet.pack_filter([])[1] == 0
    o = M._filter_options(0.025, None)
    assert (o.voxel_filter_size, o.adaptive_max_length, o.adaptive_min_num_points, o.adaptive_max_range) == (np.float32(0.025), 0.9, 500.0, 100.0)


def test_gravity_aligned_scans_apply_the_map_builders_own_rotation():
    import math

    from reflector_ekf_slam_amd import fleet_match as M
    from reflector_ekf_slam_amd.map_builder import RangeData, rigid2f_apply, yaw_of_quaternion_f32
    rng = np.random.default_rng(5)
    rds = [RangeData(np.zeros(2, np.float32), FC.cloud(rng, 50), FC.cloud(rng, 7)), RangeData(np.zeros(2, np.float32), FC.cloud(rng, 9), np.zeros((0, 2), np.float32))]
    poses = [(1.0, -2.0, 0.7), (0.0, 0.5, -2.9)]
    scans = M.gravity_aligned_scans(rds, poses)
    for (ret, mis), rd, pose in zip(scans, rds, poses):
        yaw = yaw_of_quaternion_f32(math.cos(pose[2] / 2), math.sin(pose[2] / 2))
        assert FC.same_cloud(ret, rigid2f_apply((0.0, 0.0), yaw, rd.returns)) and FC.same_cloud(mis, rigid2f_apply((0.0, 0.0), yaw, rd.misses))
        assert ret.dtype == np.float32 and ret.shape == rd.returns.shape and mis.shape == rd.misses.shape


# ---- the conditions the GPU cases rely on, shown in the oracle -------------------------------------------------------------
def test_stride_counts_sit_on_both_sides_of_the_kernels_strides():
    scans = FC.stride_case()
    nr = [s[0].shape[0] for s in scans]
    nm = [0 if s[1] is None else s[1].shape[0] for s in scans]
    assert tuple(nr) == FC.STRIDE_COUNTS and sorted(nm) == sorted(nr) and nm != nr and any(s[1] is None for s in scans)
    for counts in (nr, nm):
        assert {0, 1, FC.WAVE - 1, FC.WAVE, FC.WAVE + 1, FC.WG_THREADS - 1, FC.WG_THREADS, FC.WG_THREADS + 1} <= set(counts)
        assert max(counts) > 2 * FC.WG_THREADS                                       # a thread with three points, a third tile
    assert all(np.array_equal(s[0][::7], np.round(s[0][::7], 1).astype(np.float32)) for s in scans)


def test_stride_clouds_lose_points_at_every_size_and_differently(oracle_lib):
    from oracle.binding import oracle_voxel_filter
    big = FC.stride_case()[-1][0]
    kept = [oracle_voxel_filter(big, size).shape[0] for size in FC.STRIDE_SIZES]
    assert big.shape[0] > kept[0] > kept[1] > kept[2] > 1


def test_rounding_case_conditions(oracle_lib):
    from oracle.binding import oracle_voxel_filter
    res = FC.ROUND_RES
    (both, halves), (mixed, _), (zeros, zeros_rev), (one_voxel, _), (own, _), (shared_ret, shared_mis) = FC.rounding_case()
    q = halves / np.float32(res)
    assert np.array_equal(q, np.floor(q) + 0.5) and (q > 0).any() and (q < 0).any()                  # exactly half-way, both signs
    # half away from zero: a half-way point in front takes the voxel of the whole point further out, which then goes
    fr = oracle_voxel_filter(both, res)
    away = (np.sign(halves) * np.ceil(np.abs(halves) / np.float32(res)) * np.float32(res)).astype(np.float32)
    gone = {tuple(p) for p in away.tolist()}
    assert FC.same_cloud(fr[:halves.shape[0]], halves) and not any(tuple(p) in gone for p in fr[halves.shape[0]:].tolist())
    assert halves.shape[0] < fr.shape[0] < both.shape[0] and 0 < oracle_voxel_filter(mixed, res).shape[0] < mixed.shape[0]
    assert np.signbit(zeros[0, 0]) and not np.signbit(zeros[1, 0])
    assert FC.bits(oracle_voxel_filter(zeros, res)).tolist() == FC.bits(zeros[[0, 2, 4, 6]]).tolist()      # the first of a voxel, with its sign bit
    assert not FC.same_cloud(oracle_voxel_filter(zeros_rev, res), oracle_voxel_filter(zeros, res))
    assert oracle_voxel_filter(one_voxel, res).shape[0] == 1 and one_voxel.shape[0] == 500
    assert FC.same_cloud(oracle_voxel_filter(own, res), own) and own.shape[0] > FC.WG_THREADS
    vr, vm = FC.voxel_index(shared_ret, res), FC.voxel_index(shared_mis, res)
    assert {tuple(v) for v in vr.tolist()} == {tuple(v) for v in vm.tolist()}
    assert FC.same_cloud(oracle_voxel_filter(shared_ret, res), shared_ret) and FC.same_cloud(oracle_voxel_filter(shared_mis, res), shared_mis)


def test_hash_case_conditions(oracle_lib):
    from oracle.binding import oracle_voxel_filter
    from reflector_ekf_slam_amd import fleet_match as M
    limit = M.filter_max_points()
    (distinct, _), (strided, _), (three, _) = FC.hash_case(limit)[0]
    assert distinct.shape[0] == limit and FC.same_cloud(oracle_voxel_filter(distinct, FC.HASH_SIZE), distinct)
    v = FC.voxel_index(strided, FC.HASH_SIZE)
    assert strided.shape[0] == 4096 and not (v[:, 0] % 1024).any() and not (v[:, 1] % 4096).any()
    assert len({tuple(p) for p in v.tolist()}) == 4096
    assert three.shape[0] == 8192 and oracle_voxel_filter(three, FC.HASH_SIZE).shape[0] == 3


def test_gate_case_conditions(oracle_lib):
    from oracle.binding import oracle_voxel_filter
    scans, opt = FC.gate_case()
    limit = np.float32(opt.max_range)
    assert (FC.norm_f32(FC.ON_GATE) == limit).all() and (FC.norm_f32(FC.PAST_GATE) == np.nextafter(limit, np.float32(np.inf))).all()
    paths = []
    for scan in scans:
        fr = oracle_voxel_filter(scan[0], 0.025)
        label, out = FC.search_path(fr, *FC.option_values(opt))
        assert FC.same_cloud(out, FC.oracle_triple(scan, 0.025, opt)[2])
        paths.append((label[0], int((FC.norm_f32(fr) <= limit).sum()), out))
    assert paths[0][0] == "ladder" and paths[0][1] > opt.min_num_points
    assert FC.same_cloud(paths[0][2][:4], FC.ON_GATE)                                                # norm == max_range stays
    assert paths[1][1] == 0 and paths[1][2].shape[0] == 0                                            # the gate removes everything
    assert paths[2][0] == "sparse" and 0 < paths[2][1] <= opt.min_num_points < scans[2][0].shape[0]  # untouched behind the gate
    assert FC.same_cloud(oracle_voxel_filter(scans[2][0], 0.025)[:4], FC.PAST_GATE)                  # one ulp beyond: they reach the gate ...
    assert FC.same_cloud(paths[2][2][:4], FC.AXIS_GATE) and (FC.norm_f32(FC.AXIS_GATE) == limit).all()   # ... and go; the next four stay


def test_adaptive_cases_take_every_path_in_the_oracle(oracle_lib):
    from oracle.binding import oracle_voxel_filter
    scans, opt, want = FC.adaptive_case()
    got = []
    for scan in scans:
        fr = oracle_voxel_filter(scan[0], FC.ADAPTIVE_SIZE)
        label, out = FC.search_path(fr, *FC.ADAPTIVE_OPTIONS)
        assert FC.same_cloud(out, FC.oracle_triple(scan, FC.ADAPTIVE_SIZE, opt)[2])                 # the restatement is the oracle's search
        got.append(label)
    assert got == want
    sizes = [s[0].shape[0] for s in scans]
    assert all(300 <= n <= 2600 for n in sizes[:-1]) and sizes[-1] == 8192
    ladders = [p for p in got if p[0] == "ladder"]
    assert ("sparse",) in got and ("first",) in got and ("nothing", 7) in got
    for rungs in ((1,), (4, 5, 6, 7)):                                                               # rung 1 and a deep one: three steps or more, both outcomes
        assert any(p[1] in rungs and len(p[2]) >= 3 and "A" in p[2] and "R" in p[2] for p in ladders), rungs
    assert any(set(p[2]) == {"R"} for p in ladders)                                                  # the bisection accepts nothing
    repeated = scans[[k for k, c in enumerate(FC.ADAPTIVE) if c[0] == "repeated"][0]][0]
    assert repeated.shape[0] // 4 < FC.ADAPTIVE_OPTIONS[1] < oracle_voxel_filter(repeated, FC.ADAPTIVE_SIZE).shape[0]
    scans, opt, want = FC.fraction_case()
    assert opt.min_num_points == 2.5
    got = [FC.search_path(oracle_voxel_filter(s[0], FC.ADAPTIVE_SIZE), *FC.FRACTION_OPTIONS) for s in scans]
    assert tuple(g[0][0] for g in got) == want
    assert [g[1].shape[0] for g in got] == [2, 3, 3, 2]


def test_status_and_crowd_case_conditions():
    scans, want = FC.status_case()
    assert sorted(set(want)) == [FC.CAPACITY, FC.INVALID, FC.OK] and want[0] == want[-1] == FC.OK
    for (ret, mis), status in zip(scans, want):
        pts = np.concatenate([ret, FC.misses_of((ret, mis))])
        assert (status == FC.INVALID) == (not np.isfinite(pts).all())
        assert (status == FC.CAPACITY) == (max(ret.shape[0], FC.misses_of((ret, mis)).shape[0]) > FC.STATUS_MAX_POINTS)
    assert any(np.isnan(s[0]).any() for s in scans) and any(s[1] is not None and np.isinf(s[1]).any() for s in scans)
    assert any(s[0].shape[0] == 0 and s[1] is not None for s in scans)
    assert any(s[0].shape[0] == FC.STATUS_MAX_POINTS for s in scans)                                 # exactly max_points is fine
    crowd = FC.crowd_case()
    assert len(crowd) == FC.CROWD >= 300 and all(100 <= s[0].shape[0] <= 200 and s[1].shape[0] == s[0].shape[0] for s in crowd)
    assert all(s[0].shape[0] > FC.CROWD_OPTIONS[1] for s in crowd)
