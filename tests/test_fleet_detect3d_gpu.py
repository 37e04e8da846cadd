"""GPU suite of the fleet 3D detector (rdet3d_batch_* / PointCloudReflectorDetectFleet, csrc/det3d_batch.hip): B robots' clouds through
ONE launch of k_det3d_batch against oracle/detect3d_oracle.c and against a PointCloudReflectorDetect handle given the same cloud.  The
contract is BIT IDENTITY: status, K and the uint32 views of the centres."""
import ctypes as C

import numpy as np
import pytest

from tests import fleet_detect3d_cases as FC

pytestmark = pytest.mark.gpu
INVALID = -1


def _fleet(cases, max_points=None):
    from reflector_ekf_slam_amd import PointCloudReflectorDetectFleet
    from reflector_ekf_slam_amd.detect import PointCloudOptions
    mp = max_points or max(max(c["cloud"].shape[0] for c in cases), 1)
    return PointCloudReflectorDetectFleet([PointCloudOptions(c["intensity_min"]) for c in cases], max_points=mp,
                                          sensor_to_base_link=np.array([c["s2b"] for c in cases], dtype=np.float64))


def _same(got, want, stamp, where):
    """One cloud's (status, Observation) against (status, centres, M, M2) of FC.oracle."""
    status, obs = got
    assert status == want[0], (where, status, want[0])
    assert obs.time_ == stamp, where
    assert obs.cloud_.shape == want[1].shape, (where, obs.cloud_.shape, want[1].shape)
    assert np.array_equal(obs.cloud_.view(np.uint32), want[1].view(np.uint32)), (where, float(np.abs(obs.cloud_ - want[1]).max()))


def _call(fl, cases, members, stamp0=10.0, max_centers=256, check=True):
    """Members `members` of the handle, in that order, in one call; against the oracle.  -> the results."""
    got = fl.detect([(m, stamp0 + 0.5 * i, cases[m]["cloud"]) for i, m in enumerate(members)], max_centers=max_centers)
    assert len(got) == len(members) == len(fl.last_n_bright)
    if check:
        for i, m in enumerate(members):
            want = FC.oracle(cases[m], max_centers)
            _same(got[i], want, stamp0 + 0.5 * i, (cases[m]["name"], i))
            assert fl.last_n_bright[i] == want[2], (cases[m]["name"], fl.last_n_bright[i], want[2])
    return got


@pytest.fixture(scope="module")
def everything(oracle_lib):
    cases = FC.cases()
    fl = _fleet(cases)
    yield cases, fl
    fl.close()


def test_every_case_in_one_launch_gives_the_oracles_centres(everything):
    cases, fl = everything
    got = _call(fl, cases, list(range(len(cases))))
    by = {c["name"]: g for c, g in zip(cases, got)}
    assert by["lattice_256"][1].cloud_.shape == (256, 2) and by["world_16_rings"][1].cloud_.shape == (89, 2)
    assert by["lattice_257"][0] == FC.CAPACITY and by["max_bright_plus_1"][0] == FC.CAPACITY
    assert by["exactly_max_bright"][0] == 0 and by["exactly_max_bright"][1].cloud_.shape[0] > 90
    assert by["N_0"] == (0, by["N_0"][1]) and by["N_0"][1].cloud_.shape == (0, 2) and by["N_0"][1].time_ == 10.0


def test_every_case_equals_a_single_handle(everything):
    """The same clouds through PointCloudReflectorDetect handles (one per distinct gate and transform): the same bits; the cloud the batch
    refuses for its survivors is the single handle's to serve, and the 257-cluster cloud is refused by both."""
    from oracle.binding import oracle_detect3d
    from reflector_ekf_slam_amd.detect import PointCloudOptions, PointCloudReflectorDetect, RdetError
    cases, fl = everything
    got = _call(fl, cases, list(range(len(cases))), check=False)
    handles = {}
    for c, (status, obs) in zip(cases, got):
        key = (c["intensity_min"], c["s2b"])
        if key not in handles:
            handles[key] = PointCloudReflectorDetect(PointCloudOptions(c["intensity_min"]), max_points=65536, sensor_to_base_link=c["s2b"])
        g = handles[key]
        if c["name"] == "lattice_257":
            with pytest.raises(RdetError) as e:
                g.HandlePointCloud(1.0, c["cloud"])
            assert e.value.code == FC.CAPACITY == status
            continue
        single = g.HandlePointCloud(1.0, c["cloud"])
        if c["name"] == "max_bright_plus_1":
            assert status == FC.CAPACITY and obs.cloud_.shape == (0, 2)
            want = oracle_detect3d(c["cloud"], c["intensity_min"], c["s2b"])[0]
            assert single.cloud_.shape == want.shape and np.array_equal(single.cloud_.view(np.uint32), want.view(np.uint32))
            continue
        assert status == 0 and obs.cloud_.shape == single.cloud_.shape, c["name"]
        assert np.array_equal(obs.cloud_.view(np.uint32), single.cloud_.view(np.uint32)), c["name"]
    assert len(handles) >= 4
    for g in handles.values():
        g.close()


def test_alone_first_last_and_permuted(everything):
    cases, fl = everything
    idx = {c["name"]: i for i, c in enumerate(cases)}
    pick = [idx[n] for n in ("thirty_clusters", "M_31", "line_shuffled", "lattice_256", "twelve_clusters_moved", "N_0", "gate_160_161",
                             "non_finite_and_coincident", "tolerance_0.2", "N_1025")]
    for m in pick:
        _call(fl, cases, [m])                                           # alone
    rest = [m for m in range(len(cases)) if m not in pick[:2]]
    _call(fl, cases, [pick[0]] + rest + [pick[1]])                      # first / last
    _call(fl, cases, [pick[1]] + rest[::-1] + [pick[0]])
    order = list(np.random.default_rng(5).permutation(len(cases)))
    _call(fl, cases, [int(m) for m in order])                          # permuted


def test_members_that_sit_ticks_out_keep_working(everything):
    cases, fl = everything
    B = len(cases)
    _call(fl, cases, list(range(0, B, 2)))
    _call(fl, cases, [])
    _call(fl, cases, list(range(1, B, 3)))
    _call(fl, cases, [B - 1, 0])
    _call(fl, cases, list(range(B)))


def test_clouds_written_into_the_staging_slices_equal_the_copied_ones(everything):
    cases, fl = everything
    copied = _call(fl, cases, list(range(len(cases))))
    clouds = []
    for m, c in enumerate(cases):
        view = fl.staging(m)
        assert view.shape == (fl.max_points, 4) and view.dtype == np.float32
        n = c["cloud"].shape[0]
        view[:n] = c["cloud"]
        clouds.append((m, 3.0 + m, view[:n]))
    arr, count, keep = fl.pack(clouds)
    assert all(arr[m].xyzi == fl.staging(m).ctypes.data for m in range(count) if arr[m].N)       # read in place: the slice's own address
    staged = fl.detect(clouds)
    for m, (a, b) in enumerate(zip(copied, staged)):
        assert a[0] == b[0] and b[1].time_ == 3.0 + m and a[1].cloud_.tobytes() == b[1].cloud_.tobytes(), cases[m]["name"]
    # a member's slice is its own: the neighbours' clouds are where they were put
    for m, c in enumerate(cases):
        assert np.array_equal(fl.staging(m)[: c["cloud"].shape[0]], c["cloud"], equal_nan=True)


def test_three_hundred_small_clouds_in_one_launch(oracle_lib):
    """More workgroups than the chip has CUs: a queued workgroup needs nothing from a running one."""
    cases = FC.many_small()
    fl = _fleet(cases)
    got = _call(fl, cases, list(range(len(cases))))
    assert len(got) == 300 and all(st == 0 and 1 <= ob.cloud_.shape[0] <= 2 for st, ob in got)
    _call(fl, cases, list(range(299, -1, -1)))
    fl.close()


def test_per_cloud_errors_are_data_and_the_handle_goes_on(oracle_lib):
    """The over-cap and the over-256 clouds in the middle of a call whose other clouds are right; RDET_ERR_BUFFER at a small max_centers;
    the handle is usable after every one of them."""
    names = ["thirty_clusters", "M_64", "max_bright_plus_1", "line_in_order", "lattice_257", "gate_3_4_5", "world_16_rings"]
    cases = [FC.by_name(n) for n in names]
    fl = _fleet(cases)
    got = _call(fl, cases, list(range(len(cases))))
    assert [g[0] for g in got] == [0, 0, FC.CAPACITY, 0, FC.CAPACITY, 0, 0]
    assert fl.last_n_bright[2] == FC.MAX_BRIGHT + 1 and got[2][1].cloud_.shape == (0, 2) and got[4][1].cloud_.shape == (0, 2)
    got = _call(fl, cases, list(range(len(cases))), max_centers=3)
    assert [g[0] for g in got] == [FC.BUFFER, 0, FC.CAPACITY, 0, FC.CAPACITY, 0, FC.BUFFER]
    assert all(g[1].cloud_.shape == (0, 2) for g in got if g[0] != 0) and got[3][1].cloud_.shape == (2, 2)
    got = _call(fl, cases, list(range(len(cases))), max_centers=0)
    assert [g[0] for g in got] == [FC.BUFFER, FC.BUFFER, FC.CAPACITY, FC.BUFFER, FC.CAPACITY, FC.BUFFER, FC.BUFFER]
    _call(fl, cases, list(range(len(cases))), max_centers=1000)       # (capped at RDET_MAX_CENTERS)
    _call(fl, cases, [4, 2])
    _call(fl, cases, list(range(len(cases))))
    fl.close()


def test_whole_call_refusals_change_nothing_and_leave_a_pending_submit_collectable(oracle_lib):
    from reflector_ekf_slam_amd import fleet_detect
    names = ["thirty_clusters", "M_65", "line_shuffled"]
    cases = [FC.by_name(n) for n in names]
    fl = _fleet(cases, max_points=4000)
    L = fl._L
    good = [(m, 1.0 + m, cases[m]["cloud"]) for m in range(3)]
    cl = [c["cloud"] for c in cases]
    too_long = np.zeros((4001, 4), np.float32)

    def refusals(pending):
        assert fl.submit_code([(3, 1.0, cl[0])]) == INVALID                                  # a member out of range
        assert fl.submit_code([(-1, 1.0, cl[0])]) == INVALID
        assert fl.submit_code([(0, 1.0, cl[0]), (1, 1.0, cl[1]), (0, 1.0, cl[2])]) == INVALID    # named twice
        assert fl.submit_code([(0, 1.0, cl[0]), (1, 1.0, too_long)]) == (INVALID if pending else FC.CAPACITY)
        arr, count, keep = fl.pack(good)
        assert L.rdet3d_batch_submit(fl._h, C.cast(arr, C.c_void_p), -1) == INVALID
        assert L.rdet3d_batch_submit(fl._h, None, 2) == INVALID
        arr[1].N = -1
        assert L.rdet3d_batch_submit(fl._h, C.cast(arr, C.c_void_p), 3) == INVALID
        arr[1].N, arr[1].xyzi = 5, None
        assert L.rdet3d_batch_submit(fl._h, C.cast(arr, C.c_void_p), 3) == INVALID

    refusals(False)
    rc, out = fl.collect_code()
    assert rc == INVALID and out == []                                                       # nothing was submitted
    assert fl.submit_code(good) == 0
    assert fl.submit_code(good) == INVALID                                                   # a second submit before collect
    assert fl.submit_code([]) == INVALID
    refusals(True)
    assert L.rdet3d_batch_collect(fl._h, None, None, None, 0, None, None) == INVALID         # null result arrays: still outstanding
    assert L.rdet3d_batch_collect(fl._h, None, None, None, -1, None, None) == INVALID
    got = fl.collect()                                                                       # ... and the pending submit is all there
    for m in range(3):
        _same(got[m], FC.oracle(cases[m]), 1.0 + m, names[m])
    assert fl.collect_code()[0] == INVALID
    # staging and set_sensor_to_base_link refuse what is out of range; a new transform is the next call's
    p = C.c_void_p()
    assert L.rdet3d_batch_staging(fl._h, 3, C.byref(p)) == INVALID and L.rdet3d_batch_staging(fl._h, -1, C.byref(p)) == INVALID
    assert L.rdet3d_batch_staging(fl._h, 0, None) == INVALID
    s = np.array(FC.S2B_OTHER, np.float64)
    assert L.rdet3d_batch_set_sensor_to_base_link(fl._h, 3, s.ctypes.data) == INVALID
    assert L.rdet3d_batch_set_sensor_to_base_link(fl._h, 0, None) == INVALID
    fl.SetSensorToBaseLinkTransform(1, FC.S2B_OTHER)
    moved = dict(cases[1], name="M_65_moved", s2b=FC.S2B_OTHER)
    got = fl.detect(good)
    _same(got[0], FC.oracle(cases[0]), 1.0, "unmoved")
    _same(got[1], FC.oracle(moved), 2.0, "moved")
    assert got[1][1].cloud_.tobytes() != FC.oracle(cases[1])[1].tobytes()
    assert fl.detect([]) == [] and fleet_detect.PointCloudReflectorDetectFleet.max_bright() == FC.MAX_BRIGHT
    fl.close()


def test_fleet_3d_detector_feeds_the_fleet_filter_end_to_end(oracle_lib):
    """Six robots, 40 ticks of one 14 400-point sweep each: every tick detect -> scan_events -> ReflectorEKFSLAMFleet.submit, against the
    oracle's centres through one OracleEKF per member.  Centres bit for bit on every cloud, n equal, max|mu - oracle| < 1e-9 (identical
    observations in: FP64 round-off out, the bound of the 2D end-to-end tests)."""
    from oracle.binding import OracleEKF, oracle_detect3d
    from reflector_ekf_slam_amd import PointCloud, PointCloudReflectorDetectFleet, ReflectorEKFSLAMFleet, scan_events
    from reflector_ekf_slam_amd import session as S
    from reflector_ekf_slam_amd.detect import PointCloudOptions
    from reflector_ekf_slam_amd.fleet import odom_event
    sessions = FC.e2e_sessions()
    ticks = FC.e2e_ticks(sessions)
    B = len(sessions)
    opts = [S.options_for(s) for s in sessions]
    det = PointCloudReflectorDetectFleet([PointCloudOptions()] * B, max_points=14400)
    flt = ReflectorEKFSLAMFleet(opts, max_landmarks=64)
    oekf = [OracleEKF(o.odom_model, s.init_time, s.init_pose, o.linear_velocity_cov, o.angular_velocity_cov, o.observation_cov)
            for o, s in zip(opts, sessions)]
    n_clouds = 0
    for k, tick in enumerate(ticks):
        events, clouds = [], []
        for i, (od, e, cloud) in enumerate(tick):
            s = sessions[i]
            for ev in od:
                t = float(s.ev_time[ev])
                events.append(odom_event(i, t, *s.odom[ev]))
                oekf[i].handle_odometry(t, *s.odom[ev])
            clouds.append((i, PointCloud(float(s.ev_time[e]), cloud)))
        obs = det.detect(clouds)
        for i, (status, ob) in enumerate(obs):
            co = oracle_detect3d(tick[i][2])[0]
            assert status == 0 and ob.time_ == clouds[i][1].stamp and ob.cloud_.shape == co.shape, (k, i)
            assert np.array_equal(ob.cloud_.view(np.uint32), co.view(np.uint32)), (k, i)
            assert co.shape[0] <= FC.E2E_MAX_OBS, (k, i, co.shape[0])        # no refused submit can hide behind a skipped cloud
            if k > 0:
                oekf[i].handle_observation(ob.time_, co)
        n_clouds += len(obs)
        if k == 0:                                                      # the first scan only starts the node (src/ros_node.cc:566-579)
            flt.submit(events)
            continue
        sev = scan_events(clouds, obs)
        assert len(sev) == B
        flt.submit(events + sev)
    assert n_clouds == B * FC.E2E_TICKS
    flt.sync()
    assert not flt.flags().any()
    n = flt.n()
    for i in range(B):
        assert int(n[i]) == oekf[i].mu().shape[0] and n[i] > 3 + 2 * 3, (i, n[i])
        assert np.abs(flt.get_state(i, want_sigma=False).mu - oekf[i].mu()).max() < 1e-9, i
    det.close(); flt.close()
