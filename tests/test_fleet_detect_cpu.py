"""CPU suite of the fleet detector: the ctypes layout of struct rdet2d_scan, the module without a GPU (and without the library),
scan_events, the refusals that come before any HIP call, and the GPU cases of tests/fleet_detect_cases.py held to their stated
conditions under the oracle alone.  Nothing here launches a kernel."""
import ctypes as C
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import fleet_detect_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rdet2d_scan_layout_follows_the_header():
    from reflector_ekf_slam_amd import fleet_detect
    text = open(os.path.join(ROOT, "include", "rdet.h")).read()
    body = re.search(r"typedef struct rdet2d_scan \{(.*?)\} rdet2d_scan;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int": C.c_int, "double": C.c_double, "float": C.c_float, "const float": C.c_void_p}
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const float|int|double|float)\s+(.*)$", decl, flags=re.S)
        assert m, decl
        for name in m.group(2).split(","):
            name = name.strip()
            assert name.startswith("*") == (m.group(1) == "const float"), decl
            declared.append((name.lstrip("*"), kinds[m.group(1)]))
    assert declared == list(fleet_detect.Rdet2dScan._fields_)
    assert C.sizeof(fleet_detect.Rdet2dScan) == 64 and fleet_detect.Rdet2dScan.ranges.offset == 40
    L = fleet_detect._batch_lib()                         # (checks rdet2d_batch_sizeof_scan() on load)
    assert L.rdet2d_batch_sizeof_scan() == C.sizeof(fleet_detect.Rdet2dScan)


def test_module_imports_without_a_gpu_and_reports_a_missing_library(monkeypatch):
    import reflector_ekf_slam_amd
    from reflector_ekf_slam_amd import _lib, detect, fleet_detect
    assert reflector_ekf_slam_amd.LaserReflectorDetectFleet is fleet_detect.LaserReflectorDetectFleet
    assert reflector_ekf_slam_amd.scan_events is fleet_detect.scan_events
    monkeypatch.setattr(fleet_detect._batch_lib, "ready", None)
    monkeypatch.setattr(detect._rdet, "ready", None)
    monkeypatch.setattr(_lib, "lib_path", lambda name: os.path.join(ROOT, "no_such_dir", name))
    with pytest.raises(_lib.LibraryMissing):
        fleet_detect.LaserReflectorDetectFleet([detect.ReflectorDetectOptions()])
    monkeypatch.setattr(detect._rdet, "ready", NS())       # a library built before the batch calls existed
    with pytest.raises(_lib.LibraryMissing):
        fleet_detect.LaserReflectorDetectFleet([detect.ReflectorDetectOptions()])


def test_refusals_in_front_of_any_hip_call():
    from reflector_ekf_slam_amd import fleet_detect
    from reflector_ekf_slam_amd.detect import RdetError, ReflectorDetectOptions
    L = fleet_detect._batch_lib()
    o, s, h = (fleet_detect.Rdet2dOptions * 1)(), (C.c_double * 3)(), C.c_void_p()
    po, ps = C.cast(o, C.c_void_p), C.cast(s, C.c_void_p)
    assert L.rdet2d_batch_create(po, ps, 0, 64, 0, C.byref(h)) == -1
    assert L.rdet2d_batch_create(po, ps, 1, 0, 0, C.byref(h)) == -1
    assert L.rdet2d_batch_create(None, ps, 1, 64, 0, C.byref(h)) == -1
    assert L.rdet2d_batch_create(po, None, 1, 64, 0, C.byref(h)) == -1
    assert L.rdet2d_batch_create(po, ps, 1, 64, 0, None) == -1
    assert not h.value
    assert L.rdet2d_batch_submit(None, None, 0) == -1
    assert L.rdet2d_batch_collect(None, None, None, None, 0, None) == -1
    assert L.rdet2d_batch_staging(None, 0, None, None) == -1
    assert L.rdet2d_batch_last_hip_error(None) == b""
    L.rdet2d_batch_destroy(None)
    with pytest.raises(RdetError) as e:
        fleet_detect.LaserReflectorDetectFleet([])
    assert e.value.code == -1
    with pytest.raises(RdetError):
        fleet_detect.LaserReflectorDetectFleet([ReflectorDetectOptions()], max_beams=0)


def test_scan_events_filters_by_status_and_truncates_nothing():
    from reflector_ekf_slam_amd import Observation, fleet, scan_events
    big = np.arange(2 * 40, dtype=np.float32).reshape(40, 2)          # more centres than the fleet filter takes: the caller's call
    scans = [(5, None), (2, None), (7, None), (0, None)]
    obs = [(0, Observation(1.5, big)), (-3, Observation(1.6, np.zeros((0, 2), np.float32))),
           (0, Observation(1.7, np.zeros((0, 2), np.float32))), (-5, Observation(1.8, np.zeros((0, 2), np.float32)))]
    ev = scan_events(scans, obs)
    assert [e[0] for e in ev] == [5, 7] and [e[1] for e in ev] == [fleet.EV_SCAN] * 2 and [e[2] for e in ev] == [1.5, 1.7]
    assert ev[0][4] is big and ev[0][4].shape[0] > fleet.MAX_OBS and ev[1][4].shape == (0, 2)
    assert ev[0] == fleet.scan_event(5, 1.5, big)
    assert scan_events([], []) == []
    with pytest.raises(ValueError):
        scan_events(scans, obs[:2])
    arr, count, keep = fleet.ReflectorEKFSLAMFleet.pack(ev)           # ... and they are what the fleet filter packs
    assert count == 2 and arr[0].member == 5 and arr[0].K == 40 and arr[1].K == 0


def test_pack_fills_the_records():
    from reflector_ekf_slam_amd.detect import LaserScan
    from reflector_ekf_slam_amd.fleet_detect import LaserReflectorDetectFleet
    r = np.arange(5, dtype=np.float32)
    msg = LaserScan(2.5, -1.0, 1.0, 0.5, 0.1, 0.05, 30.0, r, list(range(5)))
    arr, count, keep = LaserReflectorDetectFleet.pack([(3, msg), (1, LaserScan(2.6, -1.0, 1.0, 0.5, 0.1, 0.05, 30.0, [], []))])
    assert count == 2 and arr[0].member == 3 and arr[0].stamp == 2.5 and arr[0].N == 5 and arr[0].ranges == r.ctypes.data
    assert arr[0].intensities == keep[0][1].ctypes.data and keep[0][1].dtype == np.float32
    assert arr[0].angle_increment == 0.5 and arr[0].range_max == 30.0
    assert arr[1].N == 0 and arr[1].ranges is None
    with pytest.raises(ValueError):
        LaserReflectorDetectFleet.pack([(0, LaserScan(2.5, -1.0, 1.0, 0.5, 0.1, 0.05, 30.0, r, r[:3]))])


def test_cases_stay_within_their_stated_conditions(oracle_lib):
    """Files 1, 2 and 7 under the oracle alone: a reflector wherever a case claims one, more lidars in the one call than cached tables,
    odometry that matters, and no scan of the end-to-end run with more centres than the fleet filter takes."""
    from oracle.binding import OracleDetect2D
    members, ticks, claims = FC.shapes_case()
    res = FC.oracle_ticks(members, ticks)[0]
    assert len(res) == 28 and all(r[0] == 0 for r in res)
    for m, (r, claim) in enumerate(zip(res, claims)):
        assert (r[2].shape[0] >= 1) == claim, (m, r[2].shape[0], claim)
    assert [sc.ranges.shape[0] for _, sc in ticks[0]["scans"]][-8:] == list(FC.RAGGED_N)
    assert len({(sc.ranges.shape[0], sc.angle_min, sc.angle_increment) for _, sc in ticks[0]["scans"]}) == 11
    assert max(r[2].shape[0] for r in res) <= 256

    members, ticks = FC.odometry_case()
    res = FC.oracle_ticks(members, ticks)
    assert len({r[2].tobytes() for r in res[0][:6]}) == 6              # six odometry histories, six different answers to ONE scan
    assert len({r[2].tobytes() for r in res[2]}) == 7
    assert all(r[0] == 0 and r[2].shape[0] >= 10 for tick in res for r in tick)
    left_out = set(range(7)) - {m for m, _ in ticks[1]["scans"]}
    assert left_out == {1, 3, 6} and {m for m, _ in ticks[2]["scans"]} == set(range(7))

    members, ticks = FC.many_case()
    res = FC.oracle_ticks(members, ticks, want_returns=False)[0]
    assert len(res) == 300 and all(r[0] == 0 and 1 <= r[2].shape[0] <= 2 for r in res)

    sessions = FC.e2e_sessions()
    e2e = FC.e2e_ticks(sessions)
    assert len(sessions) == 6 and len(e2e) == 40 and len({s.config.seed for s in sessions}) == 6
    kmax, total = 0, 0
    for i, s in enumerate(sessions):
        o = OracleDetect2D(sensor_to_base_link=FC.S2B)
        for tick in e2e:
            od, e, sc = tick[i]
            assert sc.ranges.shape[0] == 2880
            for ev in od:
                o.handle_odometry(*FC.e2e_odom_tuple(s, ev))
            t, c = o.handle_scan(sc)
            kmax, total = max(kmax, c.shape[0]), total + c.shape[0]
        o.close()
    assert kmax <= FC.MAX_OBS and total > 6 * 40 * 3
