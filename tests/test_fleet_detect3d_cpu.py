"""CPU suite of the fleet 3D detector: the header and the built library declare and export rdet3d_batch_*, the ctypes layout of struct
rdet3d_cloud, the module without a GPU (and without the library), the refusals that come before any HIP call, the event builders, and the
GPU cases of tests/fleet_detect3d_cases.py held to their stated counts under the oracle and the witness.  Nothing here launches a kernel."""
import ctypes as C
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import fleet_detect3d_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("create", "destroy", "set_sensor_to_base_link", "staging", "submit", "collect", "max_bright", "sizeof_cloud", "last_hip_error")


def test_header_declares_and_library_exports_the_batch_calls():
    from reflector_ekf_slam_amd import fleet_detect
    text = open(os.path.join(ROOT, "include", "rdet.h")).read()
    assert re.search(r"#define RDET_ABI_VERSION 1\b", text)
    for s in SYMBOLS:
        assert re.search(r"\brdet3d_batch_%s\s*\(" % s, text), s
    body = re.search(r"typedef struct rdet3d_cloud \{(.*?)\} rdet3d_cloud;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int": C.c_int, "double": C.c_double, "const float": C.c_void_p}
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const float|int|double)\s+(.*)$", decl, flags=re.S)
        assert m, decl
        for name in m.group(2).split(","):
            name = name.strip()
            assert name.startswith("*") == (m.group(1) == "const float"), decl
            declared.append((name.lstrip("*"), kinds[m.group(1)]))
    assert declared == list(fleet_detect.Rdet3dCloud._fields_)
    assert C.sizeof(fleet_detect.Rdet3dCloud) == 32 and fleet_detect.Rdet3dCloud.xyzi.offset == 16
    L = fleet_detect._batch3_lib()                        # (checks rdet3d_batch_sizeof_cloud() on load)
    for s in SYMBOLS:
        assert hasattr(L, "rdet3d_batch_" + s), s
    assert L.rdet3d_batch_sizeof_cloud() == C.sizeof(fleet_detect.Rdet3dCloud)
    assert L.rdet3d_batch_max_bright() == FC.MAX_BRIGHT == fleet_detect.PointCloudReflectorDetectFleet.max_bright()


def test_module_imports_without_a_gpu_and_reports_a_missing_library_on_first_use(monkeypatch):
    import reflector_ekf_slam_amd
    from reflector_ekf_slam_amd import _lib, detect, fleet_detect
    assert reflector_ekf_slam_amd.PointCloudReflectorDetectFleet is fleet_detect.PointCloudReflectorDetectFleet
    assert reflector_ekf_slam_amd.cloud_events is fleet_detect.cloud_events
    monkeypatch.setattr(fleet_detect._batch3_lib, "ready", None)
    monkeypatch.setattr(detect._rdet, "ready", None)
    monkeypatch.setattr(_lib, "lib_path", lambda name: os.path.join(ROOT, "no_such_dir", name))
    with pytest.raises(_lib.LibraryMissing):
        fleet_detect.PointCloudReflectorDetectFleet([detect.PointCloudOptions()])
    monkeypatch.setattr(detect._rdet, "ready", NS())       # a library built before the batch calls existed
    with pytest.raises(_lib.LibraryMissing):
        fleet_detect.PointCloudReflectorDetectFleet([detect.PointCloudOptions()])
    wrong = NS(rdet3d_batch_create=None, rdet3d_batch_sizeof_cloud=lambda: 24)    # ... or with another struct rdet3d_cloud
    monkeypatch.setattr(detect._rdet, "ready", wrong)
    with pytest.raises(_lib.LibraryMissing):
        fleet_detect.PointCloudReflectorDetectFleet([detect.PointCloudOptions()])
    assert fleet_detect._batch3_lib.ready is None


def test_refusals_in_front_of_any_hip_call():
    from reflector_ekf_slam_amd import fleet_detect
    from reflector_ekf_slam_amd.detect import PointCloudOptions, RdetError
    L = fleet_detect._batch3_lib()
    o, s, h = (fleet_detect.Rdet3dOptions * 1)(), (C.c_double * 3)(), C.c_void_p()
    po, ps = C.cast(o, C.c_void_p), C.cast(s, C.c_void_p)
    assert L.rdet3d_batch_create(po, ps, 0, 64, 0, C.byref(h)) == -1
    assert L.rdet3d_batch_create(po, ps, -1, 64, 0, C.byref(h)) == -1
    assert L.rdet3d_batch_create(po, ps, 1, 0, 0, C.byref(h)) == -1
    assert L.rdet3d_batch_create(None, ps, 1, 64, 0, C.byref(h)) == -1
    assert L.rdet3d_batch_create(po, None, 1, 64, 0, C.byref(h)) == -1
    assert L.rdet3d_batch_create(po, ps, 1, 64, 0, None) == -1
    assert not h.value
    p = C.c_void_p()
    arr = (fleet_detect.Rdet3dCloud * 1)()
    assert L.rdet3d_batch_submit(None, None, 0) == -1
    assert L.rdet3d_batch_submit(None, C.cast(arr, C.c_void_p), 1) == -1
    assert L.rdet3d_batch_collect(None, None, None, None, 0, None, None) == -1
    assert L.rdet3d_batch_staging(None, 0, C.byref(p)) == -1 and not p.value
    assert L.rdet3d_batch_set_sensor_to_base_link(None, 0, ps) == -1
    assert L.rdet3d_batch_last_hip_error(None) == b""
    L.rdet3d_batch_destroy(None)
    with pytest.raises(RdetError) as e:
        fleet_detect.PointCloudReflectorDetectFleet([])
    assert e.value.code == -1
    with pytest.raises(RdetError):
        fleet_detect.PointCloudReflectorDetectFleet([PointCloudOptions()], max_points=0)


def test_pack_and_the_event_builders():
    from reflector_ekf_slam_amd import Observation, PointCloud, cloud_events, fleet, scan_events
    from reflector_ekf_slam_amd.fleet_detect import PointCloudReflectorDetectFleet
    pts = np.arange(20, dtype=np.float32).reshape(5, 4)
    arr, count, keep = PointCloudReflectorDetectFleet.pack([(3, 2.5, pts), (1, PointCloud(2.6, np.zeros((0, 4)))), (0, 2.7, pts.tolist())])
    assert count == 3 and arr[0].member == 3 and arr[0].stamp == 2.5 and arr[0].N == 5 and arr[0].xyzi == pts.ctypes.data
    assert arr[1].member == 1 and arr[1].stamp == 2.6 and arr[1].N == 0 and arr[1].xyzi is None
    assert arr[2].N == 5 and arr[2].xyzi == keep[2].ctypes.data and keep[2].dtype == np.float32
    with pytest.raises(ValueError):
        PointCloudReflectorDetectFleet.pack([(0, 1.0, np.zeros(6, np.float32))])
    big = np.arange(2 * 40, dtype=np.float32).reshape(40, 2)          # more centres than the fleet filter takes: the caller's call
    none = np.zeros((0, 2), np.float32)
    obs = [(0, Observation(1.5, big)), (-4, Observation(1.6, none)), (0, Observation(1.7, none)), (-5, Observation(1.8, none))]
    triples = [(5, 1.5, pts), (2, 1.6, pts), (7, 1.7, pts), (0, 1.8, pts)]
    pairs = [(m, PointCloud(t, c)) for m, t, c in triples]
    for ev in (cloud_events(triples, obs), scan_events(pairs, obs), cloud_events(pairs, obs)):
        assert [e[0] for e in ev] == [5, 7] and [e[1] for e in ev] == [fleet.EV_SCAN] * 2 and [e[2] for e in ev] == [1.5, 1.7]
        assert ev[0][4] is big and ev[1][4].shape == (0, 2) and ev[0] == fleet.scan_event(5, 1.5, big)
    assert cloud_events([], []) == []
    with pytest.raises(ValueError):
        cloud_events(triples, obs[:2])


def test_cases_do_what_they_claim_under_the_oracle_and_the_witness(oracle_lib):
    """Every cloud of the GPU suite: the counts its builder states, the refusals, and the witness's centres bit for bit wherever the
    witness is defined (finite coordinates, no refusal)."""
    from tests.witness.detect3d_witness import detect3d_witness
    names = [c["name"] for c in FC.cases()]
    assert len(set(names)) == len(names) and all(f"N_{n}" in names for n in FC.SIZES) and all(f"M_{n}" in names for n in FC.SIZES[1:])
    n_witness = 0
    for c in FC.cases():
        status, cen, m, m2 = FC.oracle(c)
        cl = c["claims"]
        assert status == cl.get("status", 0), c["name"]
        for key, got in (("K", cen.shape[0]), ("M", m), ("M2", m2)):
            if key in cl:
                assert got == cl[key], (c["name"], key, got, cl[key])
        if c["name"].startswith("N_"):
            assert c["cloud"].shape[0] == int(c["name"][2:])
        if c["witness"] and status == 0:
            wc, wm, wm2 = detect3d_witness(c["cloud"], c["intensity_min"], c["s2b"])
            assert (wm, wm2) == (m, m2) and wc.shape == cen.shape and np.array_equal(wc.view(np.uint32), cen.view(np.uint32)), c["name"]
            n_witness += 1
    assert n_witness >= len(names) - 3
    # the outlier removal is at work from 31 survivors on, and not below
    assert FC.oracle(FC.by_name("M_30"))[3] == 30 and FC.oracle(FC.by_name("M_31"))[3] < 31 and FC.oracle(FC.by_name("M_32"))[3] < 32
    # the line survives as one component: 168 kept points = 128 of the line + the blob of 40, two clusters
    for name in ("line_shuffled", "line_in_order"):
        assert FC.oracle(FC.by_name(name))[3] == 168
    # all of one size: the order of the 256 centres is the order of their first points
    lat = FC.by_name("lattice_256")
    cen = FC.oracle(lat)[1]
    first = {}
    for i, p in enumerate(lat["cloud"]):
        first.setdefault((p[0], p[1]), i)
    assert [first[(x, y)] for x, y in cen] == sorted(first.values()) and len(first) == 256
    assert FC.oracle(FC.by_name("max_bright_plus_1"))[2] == FC.MAX_BRIGHT + 1
    # per-member gates and transforms matter
    moved = FC.by_name("twelve_clusters_moved")
    plain = dict(moved, name="twelve_clusters_plain", intensity_min=160.0, s2b=(0.0, 0.0, 0.0))
    assert FC.oracle(moved)[1].tobytes() != FC.oracle(plain)[1].tobytes()
    # a small buffer is that cloud's RDET_ERR_BUFFER
    assert FC.oracle(FC.by_name("thirty_clusters"), max_centers=3)[0] == FC.BUFFER


def test_many_small_and_end_to_end_clouds_stay_within_their_stated_conditions(oracle_lib):
    from oracle.binding import oracle_detect3d
    small = FC.many_small()
    assert len(small) == 300
    for c in small:
        status, cen, m, _ = FC.oracle(c)
        assert status == 0 and 1 <= cen.shape[0] <= 2 and m < 64, c["name"]
    sessions = FC.e2e_sessions()
    ticks = FC.e2e_ticks(sessions)
    assert len(sessions) == FC.E2E_MEMBERS and len(ticks) == FC.E2E_TICKS
    kmax, mmax, total = 0, 0, 0
    for tick in ticks:
        for od, e, cloud in tick:
            assert cloud.shape == (14400, 4)
            cen, m, _ = oracle_detect3d(cloud)
            kmax, mmax, total = max(kmax, cen.shape[0]), max(mmax, m), total + cen.shape[0]
    print(f"end to end: K <= {kmax}, M <= {mmax}, {total} centres")
    assert kmax <= FC.E2E_MAX_OBS and mmax <= FC.MAX_BRIGHT and total > 6 * 40 * 3, (kmax, mmax, total)
