"""The linked fleet tick, what can be checked without a GPU: the three headers against the two libraries and the binding (the
calls, struct rlink's size and field offsets, the untouched ABI versions), the package's exports, ``linked_scan_events``' omission rule
over a link built by hand, the argument checks that come before any HIP call, and the reflector counts of the scans the GPU suite
builds (tests/fleet_link_cases.py) under the CPU oracle."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FLEET_CALLS = ("rfleet_submit_linked", "rfleet_link_status", "rfleet_link_counts", "rfleet_sizeof_link")
DET_CALLS = ("rdet2d_batch_link", "rdet3d_batch_link", "rdet_sizeof_link")


def _header(name):
    return open(os.path.join(INCLUDE, name)).read()


def test_the_headers_declare_the_calls_and_the_libraries_export_them():
    from reflector_ekf_slam_amd import detect, fleet
    rfleet_h, rdet_h = _header("rfleet.h"), _header("rdet.h")
    for name in FLEET_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, rfleet_h), name
        assert hasattr(fleet.rfleet(), name), f"{name} is declared in include/rfleet.h but librfleet.so does not export it"
    for name in DET_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, rdet_h), name
        assert hasattr(detect._rdet(), name), f"{name} is declared in include/rdet.h but librdet.so does not export it"
    assert re.search(r"RFLEET_EV_SCAN_LINKED\s*=\s*2\b", rfleet_h) and fleet.EV_SCAN_LINKED == 2
    # neither library's header includes the other's: both include the link's
    includes = lambda text: re.findall(r'^#include\s+[<"]([^>"]+)[>"]', text, re.M)
    assert includes(rfleet_h) == ["rekf.h", "rlink.h"] and includes(rdet_h) == ["rlink.h"] and includes(_header("rlink.h")) == []


def test_the_abi_versions_are_unchanged():
    from reflector_ekf_slam_amd import detect, fleet
    assert int(re.search(r"#define\s+RFLEET_ABI_VERSION\s+(\d+)", _header("rfleet.h")).group(1)) == 2 == fleet.rfleet().rfleet_abi_version()
    assert int(re.search(r"#define\s+RDET_ABI_VERSION\s+(\d+)", _header("rdet.h")).group(1)) == 1 == detect._rdet().rdet_abi_version()
    assert fleet.RFLEET_ABI_VERSION == 2
    assert fleet.rfleet().rfleet_sizeof_event() == C.sizeof(fleet.RfleetEvent) == 80       # rfleet_event keeps its layout


def test_struct_rlink_agrees_with_the_binding(tmp_path):
    """sizeof and every field's offset, from a C program compiled against include/rlink.h, and both libraries' sizeof calls."""
    from reflector_ekf_slam_amd import _lib, detect, fleet
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("hipcc")
    if cc is None:
        pytest.skip("needs a C compiler")
    fields = [name for name, _ in _lib.Rlink._fields_]
    src = tmp_path / "rlink_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rlink.h"\nint main(void) {\n  printf("%zu", sizeof(rlink));\n'
                   + "".join('  printf(" %%zu", offsetof(rlink, %s));\n' % f for f in fields) + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "rlink_layout")
    subprocess.run([cc, "-x", "c", "-I", INCLUDE, str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.Rlink) == fleet.rfleet().rfleet_sizeof_link() == detect._rdet().rdet_sizeof_link()
    assert got[1:] == [getattr(_lib.Rlink, f).offset for f in fields]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct rlink \{(.*?)\} rlink;", _header("rlink.h"), re.S).group(1), flags=re.S)
    assert re.findall(r"\b(\w+)\s*(?:,|;)", body) == fields   # every field, in the header's order


def test_the_package_exports():
    import reflector_ekf_slam_amd as pkg
    from reflector_ekf_slam_amd import _lib, fleet, fleet_detect
    assert pkg.DetectLink is fleet_detect.DetectLink and pkg.linked_scan_events is fleet_detect.linked_scan_events
    assert pkg.linked_scan_event is fleet.linked_scan_event
    for cls in (fleet_detect.LaserReflectorDetectFleet, fleet_detect.PointCloudReflectorDetectFleet):
        assert callable(cls.link) and callable(cls.link_code)
    for name in ("submit_linked", "submit_linked_code", "link_status", "link_counts"):
        assert callable(getattr(fleet.ReflectorEKFSLAMFleet, name))
    # the calls sit behind lazily resolved features of their own
    for feature, names in ((fleet._link_lib, FLEET_CALLS[:3]), (fleet_detect._link2_lib, DET_CALLS[:1]), (fleet_detect._link3_lib, DET_CALLS[1:2])):
        assert isinstance(feature, _lib.Feature) and tuple(feature.names) == tuple(names) and feature() is not None


def test_a_library_without_the_calls_still_loads_and_the_methods_say_so(monkeypatch):
    from reflector_ekf_slam_amd import _lib, fleet

    class Older:                                              # a librfleet.so from before the linked submit
        def __getattr__(self, name):
            if name in FLEET_CALLS:
                raise AttributeError(name)
            return getattr(fleet.rfleet(), name)

    older = _lib.Feature(lambda: Older(), "librfleet.so", fleet._link_lib.names, fleet._link_lib.sizes, fleet._link_lib.declare)
    monkeypatch.setattr(fleet, "_link_lib", older)
    flt = fleet.ReflectorEKFSLAMFleet.__new__(fleet.ReflectorEKFSLAMFleet)
    flt._h = None
    for call in (lambda: flt.submit_linked([], None), flt.link_status, flt.link_counts):
        with pytest.raises(_lib.LibraryMissing, match="rfleet_submit_linked"):
            call()


def _hand_link(members, stamps, status, records):
    from reflector_ekf_slam_amd import _lib
    from reflector_ekf_slam_amd.fleet_detect import DetectLink
    keep = (np.asarray(members, np.int32), np.asarray(stamps, np.float64), np.asarray(status, np.int32), np.asarray(records, np.int32))
    raw = _lib.Rlink()
    raw.count = len(members)
    raw.member, raw.stamp, raw.host_status, raw.record = (a.ctypes.data for a in keep)
    return DetectLink(raw, keep)


def test_linked_scan_events_omits_exactly_the_entries_with_a_host_status():
    from reflector_ekf_slam_amd import fleet, linked_scan_events
    link = _hand_link([4, 0, 2, 7, 1], [1.5, 1.25, 1.75, 2.0, 2.25], [0, -3, 0, 0, -3], [0, -1, -1, 3, -1])
    assert len(link) == 5 and link.members.tolist() == [4, 0, 2, 7, 1] and link.status.tolist() == [0, -3, 0, 0, -3]
    assert link.stamps.tolist() == [1.5, 1.25, 1.75, 2.0, 2.25] and link.records.tolist() == [0, -1, -1, 3, -1]
    ev = linked_scan_events(link)
    assert ev == [(4, 2, 1.5, (0.0, 0.0, 0.0), 0), (2, 2, 1.75, (0.0, 0.0, 0.0), 2), (7, 2, 2.0, (0.0, 0.0, 0.0), 3)]   # an entry without a record stays
    fixes = [(1.0, 2.0, 0.5), (9.0, 9.0, 9.0), None, (0.0, -1.0, 0.25), None]
    ev = linked_scan_events(link, fixes)
    assert [e[0] for e in ev] == [4, 2, 7] and ev[0][5] == (1.0, 2.0, 0.5) and len(ev[1]) == 5 and ev[2][5] == (0.0, -1.0, 0.25)
    with pytest.raises(ValueError):
        linked_scan_events(link, fixes[:4])
    assert linked_scan_events(_hand_link([], [], [], [])) == []
    arr, count, _ = fleet.ReflectorEKFSLAMFleet.pack(ev)      # the entry travels in K, without observations
    assert count == 3 and [arr[i].kind for i in range(3)] == [2, 2, 2] and [arr[i].K for i in range(3)] == [0, 2, 3]
    assert [arr[i].xy for i in range(3)] == [None] * 3 and [arr[i].has_pose_fix for i in range(3)] == [1, 0, 1]


def test_null_handles_are_refused_before_any_hip_call():
    from reflector_ekf_slam_amd import _lib, fleet, fleet_detect
    L = fleet._link_lib()
    raw = _lib.Rlink()
    n = C.c_long()
    assert L.rfleet_submit_linked(None, None, 0, C.addressof(raw)) == -1
    assert L.rfleet_link_status(None, None, None, None, 0) == -1 and L.rfleet_link_counts(None, C.byref(n), None, None, None) == -1
    assert fleet_detect._link2_lib().rdet2d_batch_link(None, C.addressof(raw)) == -1
    assert fleet_detect._link3_lib().rdet3d_batch_link(None, C.addressof(raw)) == -1


def test_the_gpu_suites_scans_hold_the_counts_they_claim(oracle_lib):
    from oracle.binding import OracleDetect2D
    from tests.detect_cases import S2B, plate_scan
    from tests.fleet_link_cases import plates
    for n_beams, counts in ((720, (0, 1, 2, 5, 7, 31, 32, 33)), (2048, (1, 5, 20, 32, 33, 64, 65))):
        for k in counts:
            _, centres = OracleDetect2D(sensor_to_base_link=S2B).handle_scan(plate_scan(n_beams, plates(k, n_beams), stamp=1.0))
            assert centres.shape[0] == k, (n_beams, k)
