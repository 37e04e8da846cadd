"""The 2D detector sweep on the GPU (cases: tests/detect2d_sweep_cases.py): k_det2d (one handle), k_det2d_batch and
k_det2d_batch_range_data (the fleet) against the independent witness tests/witness/detect2d_witness.py, computed here, BIT FOR BIT:
centres, observation time and de-skewed returns.  The oracle is not consulted.  Nothing has a tolerance; the cases that claim a NaN
centre compare with equal_nan."""
import numpy as np
import pytest

from tests import detect2d_sweep_cases as SC

pytestmark = pytest.mark.gpu

CASES = SC.all_cases()


@pytest.fixture(scope="module")
def results():
    return SC.witness_results(CASES)


def _msg(sc):
    from reflector_ekf_slam_amd.detect import LaserScan
    return LaserScan(sc.stamp, sc.angle_min, sc.angle_max, sc.angle_increment, sc.scan_time, sc.range_min, sc.range_max, sc.ranges, sc.intensities)


def _odometry(rec):
    from reflector_ekf_slam_amd import OdometryData
    t, px, py, qz, qw, vx, vy, wz = rec
    return OdometryData(t, (vx, vy, 0.0), (0.0, 0.0, wz), (px, py, 0.0), (qw, 0.0, 0.0, qz))


def _options(c):
    from reflector_ekf_slam_amd.detect import ReflectorDetectOptions
    return ReflectorDetectOptions(**SC.options(c))


def _same(got, want, nan=False):
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want, equal_nan=nan)


def _handle_scan(det, c):
    """-> (time, centres, returns) of one HandleLaserScan + GetRangeData, or the error's code."""
    from reflector_ekf_slam_amd.detect import RdetError
    try:
        obs = det.HandleLaserScan(_msg(c["scan"]))
    except RdetError as e:
        return e.code
    return obs.time_, obs.cloud_, det.GetRangeData().returns


def _check(c, got, want, where=""):
    name = (c["name"], where)
    if want == SC.BAD_SCAN or not isinstance(got, tuple):
        assert got == want, name
        return
    t, cen, ret = got
    assert t == c["scan"].stamp, name
    assert _same(cen, want[0], SC.claims_nan(c)), (name, cen.shape, want[0].shape)
    assert _same(ret, want[2]), (name, ret.shape, want[2].shape)


def test_single_handle_every_case(results):
    from reflector_ekf_slam_amd.detect import LaserReflectorDetect
    for c in CASES:
        det = LaserReflectorDetect(_options(c), max_beams=8192, sensor_to_base_link=c["s2b"])
        for rec in c["odom"]:
            det.HandleOdometryData(_odometry(rec))
        _check(c, _handle_scan(det, c), results[c["name"]])
        det.close()


def test_one_handle_through_changing_geometries(results):
    """The handle caches ONE beam-angle table, keyed by (N, angle_min, angle_increment): a scanner, another, the first again, two more,
    the second again.  Every answer is the witness's, and a repeat is its first answer."""
    from reflector_ekf_slam_amd.detect import LaserReflectorDetect
    by_name = {c["name"]: c for c in CASES}
    order = ["A1", "A2", "A1", "A3", "A5", "A2"]
    assert all(not by_name[n]["odom"] and by_name[n]["s2b"] == SC.S2B and not by_name[n]["opts"] for n in order)
    det = LaserReflectorDetect(_options(by_name["A1"]), max_beams=8192, sensor_to_base_link=SC.S2B)
    first = {}
    for k, n in enumerate(order):
        got = _handle_scan(det, by_name[n])
        _check(by_name[n], got, results[n], k)
        if n in first:
            assert got[1].tobytes() == first[n][1].tobytes() and got[2].tobytes() == first[n][2].tobytes(), (n, k)
        first.setdefault(n, got)
    det.close()


def test_fleet_every_case_in_one_call(results):
    """Every case a member of one fleet, one ``detect``: more lidars than cached angle tables.  Then GetRangeData per member, one
    ``range_data`` over all members, the same over the members in reversed order, and two more calls that make the table cache replace
    an entry."""
    from reflector_ekf_slam_amd import LaserReflectorDetectFleet
    B = len(CASES)
    fl = LaserReflectorDetectFleet([_options(c) for c in CASES], max_beams=8192,
                                   sensor_to_base_link=np.array([c["s2b"] for c in CASES], dtype=np.float64))
    for m, c in enumerate(CASES):
        for rec in c["odom"]:
            fl.HandleOdometryData(m, _odometry(rec))
    got = fl.detect([(m, _msg(c["scan"])) for m, c in enumerate(CASES)])
    assert len(got) == B
    ok = []
    for m, (c, (status, obs)) in enumerate(zip(CASES, got)):
        want = results[c["name"]]
        assert obs.time_ == c["scan"].stamp, c["name"]
        if want == SC.BAD_SCAN:
            assert status == SC.BAD_SCAN and obs.cloud_.shape == (0, 2), c["name"]
            continue
        ok.append(m)
        assert status == 0, (c["name"], status)
        assert _same(obs.cloud_, want[0], SC.claims_nan(c)), (c["name"], obs.cloud_.shape, want[0].shape)
    assert len(ok) == B - 1
    for m in ok:
        assert _same(fl.GetRangeData(m).returns, results[CASES[m]["name"]][2]), CASES[m]["name"]
    forward = fl.range_data()
    assert len(forward) == B
    for m in ok:
        assert _same(forward[m].returns, results[CASES[m]["name"]][2]), CASES[m]["name"]
    backward = fl.range_data(list(range(B))[::-1])
    for m, r in zip(range(B), backward[::-1]):
        assert r.returns.tobytes() == forward[m].returns.tobytes() and r.origin.tobytes() == forward[m].origin.tobytes(), CASES[m]["name"]
    # the one-call fleet kept eight tables and gave the ninth lidar's members their own.  A call of that lidar alone now replaces a kept
    # table, and the next call of everybody has to build the replaced one again: the same bits (the trim is idempotent: same odometry)
    names = [c["name"] for c in CASES]
    m65 = names.index("B_N65")
    (status, obs), = fl.detect([(m65, _msg(CASES[m65]["scan"]))])
    assert status == 0 and _same(obs.cloud_, results["B_N65"][0])
    again = fl.detect([(m, _msg(c["scan"])) for m, c in enumerate(CASES)])
    for name, (s0, o0), (s1, o1) in zip(names, got, again):
        assert s0 == s1 and o0.time_ == o1.time_ and o0.cloud_.tobytes() == o1.cloud_.tobytes(), name
    for m, r in enumerate(fl.range_data()):
        assert r.returns.tobytes() == forward[m].returns.tobytes(), names[m]
    fl.close()
