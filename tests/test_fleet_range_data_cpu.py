"""rdet2d_batch_get_range_data_all, what can be checked without a GPU: the header declares what the library exports, the refusals
that come before any HIP call and before the handle is read, the lazy loader, and the cases of tests/fleet_range_data_cases.py held
to what they claim under the oracle alone."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fleet_range_data_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def test_header_declares_the_call_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "rdet.h")).read()
    assert re.search(r"int\s+rdet2d_batch_get_range_data_all\s*\(\s*rdet2d_batch_t\s*\*\s*b\s*,\s*const\s+int\s*\*\s*members\s*,\s*int\s+count\s*,\s*"
                     r"int\s*\*\s*counts\s*,\s*float\s*\*\s*origins_xy\s*,\s*float\s*\*\s*returns_xy\s*,\s*long\s+cap_points\s*\)\s*;", text)
    assert re.search(r"#define\s+RDET_ABI_VERSION\s+1\b", text)
    assert int(re.search(r"RDET_ERR_INVALID\s*=\s*(-?\d+)", text).group(1)) == INVALID
    assert re.search(r"int\s+rdet2d_batch_get_range_data\s*\(", text)                  # the per-member getter stays


def test_library_exports_the_call():
    from reflector_ekf_slam_amd import _lib as base
    path = base.lib_path("librdet.so")
    assert hasattr(C.CDLL(path), "rdet2d_batch_get_range_data_all")
    names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rdet2d_batch_get_range_data_all\b", names)
    assert C.CDLL(path).rdet_abi_version() == 1


def test_refusals_come_before_any_hip_call():
    """A null handle, and what is refused before the handle is read (the handle is a dummy the library must not look into)."""
    from reflector_ekf_slam_amd.fleet_detect import _range_data_lib
    call = _range_data_lib().rdet2d_batch_get_range_data_all
    counts, origins, rows = np.full(4, 77, np.int32), np.full(8, -5.0, np.float32), np.full(64, -5.0, np.float32)
    mem = np.arange(4, dtype=np.int32)
    dummy = C.c_void_p(1)
    assert call(None, mem.ctypes.data, 4, counts.ctypes.data, origins.ctypes.data, rows.ctypes.data, 32) == INVALID
    assert call(None, None, 0, None, None, None, 0) == INVALID
    assert call(dummy, mem.ctypes.data, -1, counts.ctypes.data, origins.ctypes.data, rows.ctypes.data, 32) == INVALID      # count < 0
    assert call(dummy, mem.ctypes.data, 4, None, origins.ctypes.data, rows.ctypes.data, 32) == INVALID                    # no counts
    assert call(dummy, mem.ctypes.data, 4, counts.ctypes.data, origins.ctypes.data, rows.ctypes.data, -1) == INVALID      # cap_points < 0
    assert (counts == 77).all() and (origins == -5.0).all() and (rows == -5.0).all()


def test_the_binding_looks_the_call_up_lazily(monkeypatch):
    from reflector_ekf_slam_amd import _lib as base
    from reflector_ekf_slam_amd import fleet_detect as D
    real = D._batch_lib()

    class Old:
        """A built library from before rdet2d_batch_get_range_data_all."""
        def __getattr__(self, name):
            if name == "rdet2d_batch_get_range_data_all":
                raise AttributeError(name)
            return getattr(real, name)

    old = Old()
    monkeypatch.setattr(D._range_data_lib, "ready", None)
    monkeypatch.setattr(D._batch_lib, "ready", old)
    with pytest.raises(base.LibraryMissing) as e:
        D._range_data_lib()
    assert "rdet2d_batch_get_range_data_all" in str(e.value) and "librdet.so" in str(e.value) and D._range_data_lib.ready is None
    assert D._batch_lib() is old and old.rdet2d_batch_get_range_data(None, 0, None, None, 0, None) == INVALID   # every other call keeps working
    fl = object.__new__(D.LaserReflectorDetectFleet)                 # a handle as an older library would have made it
    fl._L, fl._h, fl.B, fl.max_beams = old, None, 2, 16
    with pytest.raises(base.LibraryMissing):
        fl.range_data()
    monkeypatch.setattr(D._batch_lib, "ready", real)
    got = D._range_data_lib()
    assert got is real and got.rdet2d_batch_get_range_data_all.argtypes is not None
    assert callable(D.LaserReflectorDetectFleet.range_data) and callable(D.LaserReflectorDetectFleet.GetRangeData)
    assert "range_data(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def test_a_scan_has_exactly_the_valid_beams_asked_for():
    for k, n in ((0, 0), (0, 50), (1, 1), (7, 7), (257, 400), (8192, 8192)):
        sc = RC.scan_with_valid(k, n, 9)
        valid = (sc.ranges >= np.float32(sc.range_min)) & (sc.ranges <= np.float32(sc.range_max))
        assert sc.ranges.shape == sc.intensities.shape == (n,) and int(valid.sum()) == k
        if n - k >= 2:
            assert (sc.ranges[~valid] < sc.range_min).any() and (sc.ranges[~valid] > sc.range_max).any()


def test_cases_cover_what_they_claim(oracle_lib):
    T = RC.TILE
    src = open(os.path.join(ROOT, "reflector_ekf_slam_amd", "csrc", "det_batch_host.h")).read()
    threads = int(re.search(r"#define\s+RDET2DB_RANGE_THREADS\s+(\d+)", src).group(1))
    assert re.search(r"#define\s+RDET2DB_RANGE_TILE\s+\(2 \* RDET2DB_RANGE_THREADS\)", src) and 2 * threads == T
    E = RC.EDGE_COUNTS
    assert {0, 1, 255, 256, 257, 8192, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1} <= set(E)
    assert E[0] % 2 == 1 and E[1] == 8192 == RC.MAX_BEAMS                           # an odd count in front of the largest
    assert RC.workgroups(E[:2]) == 1 + 8192 // T + 1 and RC.workgroups((0, 8192)) == 8192 // T   # ... costs it one workgroup more
    offsets = np.concatenate([[0], np.cumsum(E)[:-1]])
    assert {(int(o) & 1, n & 1) for o, n in zip(offsets, E) if n} == {(0, 0), (0, 1), (1, 0), (1, 1)}   # every parity of offset and count
    P = RC.PERMUTED
    assert len(set(P)) == len(P) < len(E) and list(P) != sorted(P) and 0 in [E[m] for m in P]
    members, ticks = RC.edge_case()
    rows = RC.expected_rows(members, ticks)[0]
    assert [r.shape[0] for r in rows] == list(E)
    assert len({m["s2b"][:2] for m in members}) == len(members)                     # every origin is its member's
    # rows of different members differ: a row copied from the wrong member shows
    assert len({rows[m][:1].tobytes() for m in range(len(E)) if E[m]}) == sum(1 for n in E if n)
    members, ticks = RC.history_case()
    after = RC.expected_rows(members, ticks)
    assert [r.shape[0] for r in after[0]] == list(RC.HISTORY_COUNTS) and [r.shape[0] for r in after[1]] == list(RC.HISTORY_AFTER)
    assert after[1][0] is after[0][0] and after[1][2] is after[0][2]                # the member that sat out and the malformed one keep theirs
    assert [m for m, _ in ticks[1]["scans"]] == [1, 2, 3] and ticks[1]["scans"][0][1].ranges.shape[0] == 0
    counts = RC.many_counts()
    assert len(counts) == RC.MANY == 300 and set(counts) == set(range(65))
    members, ticks = RC.many_case()
    assert [r.shape[0] for r in RC.expected_rows(members, ticks)[0]] == counts
