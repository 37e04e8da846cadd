"""Fleet filter, what can be checked without a GPU: the C ABI of librfleet.so against include/rfleet.h, the argument checks
that come before any HIP call, and the staleness guard of profiles/fleet_bench.json (by content, like profiles/MANIFEST.json)."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import re

from tests.fleet_harness import HEADER, ROOT, _lib

FLEET_SOURCES = ["include/rfleet.h", "reflector_ekf_slam_amd/csrc/fleet_dev.h", "reflector_ekf_slam_amd/csrc/fleet_host.h", "reflector_ekf_slam_amd/csrc/fleet_kernels.hip",
                 "reflector_ekf_slam_amd/csrc/rfleet_api.hip", "reflector_ekf_slam_amd/fleet.py", "scripts/fleet_bench.py"]


def test_every_declared_symbol_is_exported():
    text = open(HEADER).read()
    names = sorted(set(re.findall(r"\b(rfleet_[a-z0-9_]+)\s*\(", text)))
    assert len(names) >= 13, names
    L = _lib()
    for name in names:
        assert hasattr(L, name), f"{name} is declared in include/rfleet.h but librfleet.so does not export it"


def test_abi_version_agrees():
    from reflector_ekf_slam_amd import fleet
    macro = int(re.search(r"#define\s+RFLEET_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert macro == fleet.RFLEET_ABI_VERSION == _lib().rfleet_abi_version()
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+RFLEET_MAX_LANDMARKS\s+(\d+)", text).group(1)) == fleet.MAX_LANDMARKS
    assert int(re.search(r"#define\s+RFLEET_MAX_OBS\s+(\d+)", text).group(1)) == fleet.MAX_OBS


def test_null_handles_are_refused():
    L = _lib()
    buf = (C.c_double * 16)()
    ibuf = (C.c_int * 16)()
    assert L.rfleet_sync(None) == -1
    assert L.rfleet_submit(None, None, 0) == -1
    assert L.rfleet_get_poses(None, buf, buf, buf) == -1
    assert L.rfleet_get_n(None, ibuf) == -1
    assert L.rfleet_get_flags(None, ibuf) == -1
    assert L.rfleet_get_state(None, 0, None, None, None, 0, None, 0) == -1
    assert L.rfleet_set_state(None, 0, 0.0, 3, buf, buf, None) == -1
    assert L.rfleet_get_last_match(None, 0, None, None, None, None, None, None) == -1
    assert L.rfleet_size(None, None, None) == -1
    L.rfleet_destroy(None)


def test_create_checks_its_arguments_before_any_hip_call():
    from reflector_ekf_slam_amd import _lib as base
    L = _lib()
    opts = (base.RekfOptions * 2)()
    h = C.c_void_p()
    assert L.rfleet_create(C.cast(opts, C.c_void_p), 0, 16, 0, C.byref(h)) == -1 and not h.value
    assert L.rfleet_create(C.cast(opts, C.c_void_p), 2, 129, 0, C.byref(h)) == -7 and not h.value
    assert L.rfleet_create(C.cast(opts, C.c_void_p), 2, 0, 0, C.byref(h)) == -1 and not h.value
    assert L.rfleet_create(None, 2, 16, 0, C.byref(h)) == -1 and not h.value
    assert L.rfleet_create(C.cast(opts, C.c_void_p), 2, 16, 0, None) == -1


def test_package_exports_the_fleet():
    import reflector_ekf_slam_amd as pkg
    from reflector_ekf_slam_amd import fleet
    assert pkg.ReflectorEKFSLAMFleet is fleet.ReflectorEKFSLAMFleet
    for name in ("submit", "poses", "n", "flags", "sync", "close", "member"):
        assert callable(getattr(fleet.ReflectorEKFSLAMFleet, name))
    for name in ("handle_odometry", "handle_observation", "mu", "last_match", "GetState", "set_state", "flags", "sync_code"):
        assert callable(getattr(fleet.FleetMember, name))


def test_fleet_bench_describes_the_tree():
    """profiles/fleet_bench.json was measured on the fleet sources of this tree (SHA-256 by content)."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "fleet_bench.json")))
    sums = rec["_sources_sha256"]
    assert sorted(sums) == sorted(FLEET_SOURCES)
    for rel in FLEET_SOURCES:
        have = hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
        assert have == sums[rel], f"{rel} changed since profiles/fleet_bench.json was measured: measure again (scripts/fleet_bench.py)"
