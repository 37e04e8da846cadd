"""GPU suite of the linked fleet tick (rdet2d_batch_link / rdet3d_batch_link -> rfleet_submit_linked, csrc/fleet_link.hip): the
detector's centres reach the filter on the device, through k_fleet_bind, without the host seeing them.

Every test drives twin fleets: a detector and a filter on the linked route (submit -> link -> submit_linked) and a second detector
and filter on the composed one (detect -> scan_events -> submit), fed the same messages.  The bind only moves bytes and a count, so
every comparison is BIT FOR BIT: poses, last_match, mu, sigma, n, flags, and the centres collect returns afterwards."""
import numpy as np
import pytest

from tests.detect_cases import S2B, plate_scan
from tests.fleet_link_cases import plates as _plates

pytestmark = pytest.mark.gpu

INVALID, TOO_MANY_OBS, DET_CAPACITY = -1, -3, -4


def _msg(sc):
    from reflector_ekf_slam_amd.detect import LaserScan
    return LaserScan(sc.stamp, sc.angle_min, sc.angle_max, sc.angle_increment, sc.scan_time, sc.range_min, sc.range_max, sc.ranges,
                     sc.intensities)


def _scan(k, n_beams, stamp, first=10, r0=3.0):
    return _msg(plate_scan(n_beams, _plates(k, n_beams, first, r0), stamp=stamp))


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_match(a, b, where):
    for name in ("map_obs_match_ids", "state_obs_match_ids", "new_ids"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (where, name)


def _same_fleets(flt, flt2, where, full=False):
    """poses and last_match of every member; full: also mu, sigma, n and flags."""
    got, want = flt.poses(), flt2.poses()
    for g, w in zip(got, want):
        assert _bits(g) == _bits(w), where
    for b in range(flt.B):
        _same_match(flt.last_match(b), flt2.last_match(b), (where, b))
    if full:
        assert np.array_equal(flt.n(), flt2.n()) and np.array_equal(flt.flags(), flt2.flags()), where
        for b in range(flt.B):
            s, s2 = flt.get_state(b), flt2.get_state(b)
            assert s.time == s2.time and _bits(s.mu) == _bits(s2.mu) and _bits(s.sigma) == _bits(s2.sigma), (where, b)


def _same_obs(obs, obs2, where):
    assert len(obs) == len(obs2), where
    for i, ((st, o), (st2, o2)) in enumerate(zip(obs, obs2)):
        assert st == st2 and o.time_ == o2.time_ and o.cloud_.shape == o2.cloud_.shape and _bits(o.cloud_) == _bits(o2.cloud_), (where, i)


def _states(flt):
    return [(s.time, _bits(s.mu), _bits(s.sigma)) for s in (flt.get_state(b) for b in range(flt.B))]


class Twins:
    """A detector and a filter on the linked route, a detector and a filter on the composed one."""

    def __init__(self, B, max_beams, wide=False, max_landmarks=64):
        from reflector_ekf_slam_amd import EKFOptions, LaserReflectorDetectFleet, ReflectorEKFSLAMFleet
        from reflector_ekf_slam_amd.detect import ReflectorDetectOptions
        self.B = B
        self.det, self.det2 = (LaserReflectorDetectFleet([ReflectorDetectOptions()] * B, max_beams=max_beams, sensor_to_base_link=S2B)
                               for _ in range(2))
        self.flt, self.flt2 = (ReflectorEKFSLAMFleet([EKFOptions(init_time=0.0)] * B, max_landmarks=max_landmarks, wide_scans=wide)
                               for _ in range(2))
        self.yaw = [0.0] * B
        self.pos = [[0.0, 0.0] for _ in range(B)]
        self.t_odom = [0.0] * B

    def close(self):
        for h in (self.det, self.det2, self.flt, self.flt2):
            h.close()

    def odometry(self, member, t, vx=0.05, wz=0.02):
        """One odometry message to both detectors; -> the filter's event."""
        import math
        from reflector_ekf_slam_amd import OdometryData
        from reflector_ekf_slam_amd.fleet import odom_event
        dt = t - self.t_odom[member]
        self.pos[member][0] += vx * dt * math.cos(self.yaw[member])
        self.pos[member][1] += vx * dt * math.sin(self.yaw[member])
        self.yaw[member] += wz * dt
        self.t_odom[member] = t
        y = self.yaw[member]
        msg = OdometryData(t, (vx, 0.0, 0.0), (0.0, 0.0, wz), (self.pos[member][0], self.pos[member][1], 0.0),
                           (math.cos(y / 2), 0.0, 0.0, math.sin(y / 2)))
        self.det.HandleOdometryData(member, msg)
        self.det2.HandleOdometryData(member, msg)
        return odom_event(member, t, vx, 0.0, wz)

    def linked(self, scans, events, fixes=None):
        """The linked half of a tick, without a wait: -> the link."""
        from reflector_ekf_slam_amd import linked_scan_events
        self.det.submit(scans)
        link = self.det.link()
        self.flt.submit_linked(events + linked_scan_events(link, fixes), link)
        return link

    def composed(self, scans, events, fixes=None, empty=()):
        """The composed half: detect, one scan_event per scan with status 0 (``empty``: members whose scan is handed over without its
        centres), submit.  -> the observations."""
        from reflector_ekf_slam_amd.fleet import scan_event
        obs = self.det2.detect(scans)
        sev = [scan_event(m, o.time_, o.cloud_[:0] if m in empty else o.cloud_, None if fixes is None else fixes[i])
               for i, ((m, _), (st, o)) in enumerate(zip(scans, obs)) if st == 0]
        self.flt2.submit(events + sev)
        return obs

    def tick(self, scans, events, where, fixes=None, empty=()):
        self.linked(scans, events, fixes)
        obs2 = self.composed(scans, events, fixes, empty)
        _same_fleets(self.flt, self.flt2, where)             # (poses(): the linked tick's one wait)
        obs = self.det.collect()
        _same_obs(obs, obs2, where)
        return obs


def test_linked_equals_composed_2d():
    """B = 5, 720 beams, eight ticks with odometry in between.  Tick 3 holds, in one call: a member without a scan, one whose scan has
    N = 0, a malformed scan and a scan with no reflector."""
    B, NB = 5, 720
    tw = Twins(B, NB)
    try:
        for k in range(8):
            t = 1.0 + 0.5 * k
            events = [tw.odometry(b, t - 0.3 + 0.1 * j) for b in range(B) for j in range(3)]
            scans = [(b, _scan(1 + (b + k) % 5, NB, t, first=10 + 3 * b)) for b in range(B)]
            if k == 3:
                import copy
                bad = copy.copy(scans[2][1])
                bad.range_max = bad.range_min                                    # malformed: data, status -3
                none = copy.copy(scans[1][1])
                none.ranges, none.intensities = none.ranges[:0], none.intensities[:0]
                scans = [(1, none), (2, bad), (3, _scan(0, NB, t)), (4, scans[4][1])]     # (member 0: no scan)
            link = tw.linked(scans, events)
            if k == 3:
                assert link.status.tolist() == [0, -3, 0, 0] and link.records.tolist() == [-1, -1, 2, 3] and link.members.tolist() == [1, 2, 3, 4]
            obs2 = tw.composed(scans, events)
            _same_fleets(tw.flt, tw.flt2, k)
            taken, status, seen = tw.flt.link_status()
            want_K = [o.cloud_.shape[0] for st, o in obs2 if st == 0]
            assert taken.tolist() == want_K and seen.tolist() == want_K and not status.any(), k
            _same_obs(tw.det.collect(), obs2, k)
        _same_fleets(tw.flt, tw.flt2, "end", full=True)
        assert tw.flt.n().max() > 3
        submits, binds, scans_, emptied = tw.flt.link_counts()
        assert (submits, binds, emptied) == (8, 8, 0) and scans_ == 7 * 5 + 3
    finally:
        tw.close()


@pytest.mark.parametrize("wide", [False, True])
def test_the_edges_of_K(wide):
    """Narrow: members see 1, 31, 32 and 33 centres; the member with 33 is emptied with REKF_ERR_TOO_MANY_OBS and equals the twin's
    empty scan at the same stamp.  Wide: 32, 33, 64 and 65; before that a tick with every K <= 32, which the twin sends through the
    narrow launch and the linked fleet through the wide one."""
    NB = 2048 if wide else 720
    counts = (32, 33, 64, 65) if wide else (1, 31, 32, 33)
    tw = Twins(4, NB, wide=wide, max_landmarks=128)
    try:
        if wide:
            scans = [(b, _scan(k, NB, 1.0)) for b, k in enumerate((32, 20, 5, 1))]
            tw.tick(scans, [tw.odometry(b, 0.9) for b in range(4)], "narrow counts on a wide fleet")
            assert tw.flt.wide_counts() == (1, 0) and tw.flt2.wide_counts() == (0, 0)
        scans = [(b, _scan(k, NB, 2.0)) for b, k in enumerate(counts)]
        events = [tw.odometry(b, 1.9) for b in range(4)]
        tw.linked(scans, events)
        obs2 = tw.composed(scans, events, empty=() if wide else (3,))
        assert [o.cloud_.shape[0] for _, o in obs2] == list(counts)
        _same_fleets(tw.flt, tw.flt2, "edges", full=True)
        taken, status, seen = tw.flt.link_status()
        assert seen.tolist() == list(counts)
        if wide:
            assert taken.tolist() == list(counts) and not status.any()
            assert tw.flt.wide_counts()[0] == 2 and tw.flt2.wide_counts() == (1, 3)
        else:
            assert taken.tolist() == [1, 31, 32, 0] and status.tolist() == [0, 0, 0, TOO_MANY_OBS]
            assert tw.flt.link_counts()[3] == 1
            assert tw.flt.n().tolist() == [3 + 2 * 1, 3 + 2 * 31, 3 + 2 * 32, 3]
        _same_obs(tw.det.collect(), obs2, "edges")
    finally:
        tw.close()


RECORD = np.dtype([("K", "<i4"), ("n_returns", "<i4"), ("err", "<i4"), ("n_runs", "<i4"), ("centers", "<f4", (256, 2))])


class DeviceBytes:
    """A numpy array's bytes in device memory of the runtime the libraries use (hipMalloc + a synchronous copy + a device
    synchronisation): nothing is in flight when it returns."""

    def __init__(self, array):
        import ctypes as C
        self.hip = C.CDLL("libamdhip64.so")                  # (already mapped: librfleet.so links it)
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        p = C.c_void_p()
        assert self.hip.hipSetDevice(0) == 0 and self.hip.hipMalloc(C.byref(p), raw.size) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(self.ptr, raw.ctypes.data, raw.size, 1) == 0 and self.hip.hipDeviceSynchronize() == 0   # 1: host to device

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None


def _planted_link(records, members, stamps):
    """An rlink over records the test put into device memory itself (``records``: a DeviceBytes): no event to wait for, nobody to tell."""
    from reflector_ekf_slam_amd import _lib
    from reflector_ekf_slam_amd.fleet_detect import DetectLink
    n = len(members)
    keep = (np.asarray(members, np.int32), np.asarray(stamps, np.float64), np.zeros(n, np.int32), np.arange(n, dtype=np.int32), records)
    raw = _lib.Rlink()
    raw.count, raw.device = n, 0
    raw.member, raw.stamp, raw.host_status, raw.record = (a.ctypes.data for a in keep[:4])
    raw.records, raw.record_bytes = records.ptr, RECORD.itemsize
    raw.k_off, raw.err_off, raw.centers_off, raw.max_centers = RECORD.fields["K"][1], RECORD.fields["err"][1], RECORD.fields["centers"][1], 256
    raw.ready = raw.consumed = None
    return DetectLink(raw, keep)


def test_planted_records():
    """A link the test fabricates: err = -4, K = 300, K = -7 and K = 40 are emptied with the statuses of the table, a valid entry is
    applied as the same centres through scan_event, and host scans with observations of their own sit on both sides of every emptied
    entry in the call: a read or write outside a reserved range would move one of them."""
    from reflector_ekf_slam_amd import EKFOptions, ReflectorEKFSLAMFleet
    from reflector_ekf_slam_amd.fleet import linked_scan_event, scan_event
    B = 8
    rng = np.random.default_rng(11)
    xy = lambda k, at: (rng.uniform(-0.2, 0.2, (k, 2)) + np.array([3.0 + at, 0.5 * at])).astype(np.float32)
    rec = np.zeros(5, RECORD)
    rec["centers"] = np.nan
    rec["K"] = [2, 300, -7, 5, 40]
    rec["err"] = [DET_CAPACITY, 0, 0, 0, 0]
    rec["centers"][0, :2] = xy(2, 0)
    rec["centers"][3, :5] = xy(5, 3)
    rec["centers"][4, :40] = xy(40, 4)
    records = DeviceBytes(rec)
    link = _planted_link(records, [1, 3, 5, 6, 7], [1.0] * 5)
    sentinel = {m: xy(3 + m, m) for m in (0, 2, 4)}
    flt, flt2 = (ReflectorEKFSLAMFleet([EKFOptions(init_time=0.0)] * B, max_landmarks=64) for _ in range(2))
    try:
        for tick in range(2):                                 # (the second tick matches against the first one's landmarks)
            t = 1.0 + tick
            ev = [scan_event(0, t, sentinel[0]), linked_scan_event(1, t, 0), scan_event(2, t, sentinel[2]), linked_scan_event(3, t, 1),
                  scan_event(4, t, sentinel[4]), linked_scan_event(5, t, 2), linked_scan_event(6, t, 3), linked_scan_event(7, t, 4)]
            flt.submit_linked(ev, link)
            none = np.zeros((0, 2), np.float32)
            flt2.submit([scan_event(0, t, sentinel[0]), scan_event(1, t, none), scan_event(2, t, sentinel[2]), scan_event(3, t, none),
                         scan_event(4, t, sentinel[4]), scan_event(5, t, none), scan_event(6, t, rec["centers"][3, :5].copy()),
                         scan_event(7, t, none)])
            _same_fleets(flt, flt2, tick, full=True)
            taken, status, seen = flt.link_status()
            assert taken.tolist() == [0, 0, 0, 5, 0] and seen.tolist() == [2, 300, -7, 5, 40]
            assert status.tolist() == [DET_CAPACITY, DET_CAPACITY, DET_CAPACITY, 0, TOO_MANY_OBS]
        assert flt.n().tolist() == [3 + 2 * 3, 3, 3 + 2 * 5, 3, 3 + 2 * 7, 3, 3 + 2 * 5, 3]
        assert flt.link_counts() == (2, 2, 10, 8)
    finally:
        flt.close(); flt2.close()
        records.free()


def test_with_a_shared_map_and_with_a_pose_fix():
    """B = 3: a tick on a fleet with a shared pre-loaded map, then a tick whose linked scans carry pose fixes."""
    B, NB = 3, 720
    tw = Twins(B, NB)
    try:
        scans = [(b, _scan(3 + b, NB, 1.0, first=10 + 5 * b)) for b in range(B)]
        events = [tw.odometry(b, 0.9, vx=0.0, wz=0.0) for b in range(B)]                   # (standing still: the centres are the map's points)
        seen = tw.det2.detect(scans)[0][1].cloud_                               # member 0's centres: the hall's map
        assert seen.shape[0] == 3
        for f in (tw.flt, tw.flt2):
            f.set_map(seen, np.tile(np.eye(2), (seen.shape[0], 1, 1)), members=[0, 1])
        tw.tick(scans, events, "map")
        assert len(tw.flt2.last_match(0).map_obs_match_ids) > 0 and len(tw.flt2.last_match(2).map_obs_match_ids) == 0
        scans = [(b, _scan(3 + b, NB, 2.0, first=10 + 5 * b)) for b in range(B)]
        fixes = [(0.01, -0.02, 0.005), None, (0.03, 0.01, -0.01)]
        tw.tick(scans, [tw.odometry(b, 1.9) for b in range(B)], "fix", fixes=fixes)
        _same_fleets(tw.flt, tw.flt2, "end", full=True)
    finally:
        tw.close()


def test_two_ticks_in_flight():
    """det.submit; flt.submit_linked; det.collect; det.submit (other scans); flt.submit_linked; flt.poses() with no wait of the fleet
    in between, and 40 odometry events per member in front of the first scan: the second detector launch must not overwrite a record
    -- nor the second submit's host clear one -- before the first bind has read it."""
    B, NB = 4, 720
    tw = Twins(B, NB)
    try:
        ev1 = [tw.odometry(b, 0.02 * (j + 1)) for b in range(B) for j in range(40)]
        s1 = [(b, _scan(4 + b, NB, 1.0, first=12)) for b in range(B)]
        ev2 = [tw.odometry(b, 1.5) for b in range(B)]
        s2 = [(0, _scan(0, NB, 2.0)), (1, _scan(2, NB, 2.0, first=200, r0=4.0))]
        empty = _scan(3, NB, 2.0)
        empty.ranges, empty.intensities = empty.ranges[:0], empty.intensities[:0]
        s2 += [(2, empty), (3, _scan(7, NB, 2.0, first=300, r0=3.5))]
        tw.linked(s1, ev1)
        obs1 = tw.det.collect()
        tw.linked(s2, ev2)
        got = tw.flt.poses()
        obs2 = tw.det.collect()
        _same_obs(obs1, tw.composed(s1, ev1), 1)
        _same_obs(obs2, tw.composed(s2, ev2), 2)
        for g, w in zip(got, tw.flt2.poses()):
            assert _bits(g) == _bits(w)
        _same_fleets(tw.flt, tw.flt2, "end", full=True)
        assert tw.flt.link_status()[0].tolist() == [0, 2, 0, 7] and tw.flt.link_counts()[:3] == (2, 2, 8)
    finally:
        tw.close()


def test_3d():
    """B = 3 clouds of a few hundred points, two ticks; the second holds a cloud with no survivor of the intensity gate and one
    with N = 0."""
    from reflector_ekf_slam_amd import (EKFOptions, PointCloudReflectorDetectFleet, ReflectorEKFSLAMFleet, cloud_events,
                                        linked_scan_events)
    from reflector_ekf_slam_amd.detect import PointCloudOptions
    from tests import fleet_detect3d_cases as F3
    small = F3.many_small(5)
    dim = F3.by_name("nothing_bright")["cloud"]
    det, det2 = (PointCloudReflectorDetectFleet([PointCloudOptions(150.0)] * 3, max_points=1024) for _ in range(2))
    flt, flt2 = (ReflectorEKFSLAMFleet([EKFOptions(init_time=0.0)] * 3, max_landmarks=32) for _ in range(2))
    try:
        ticks = [[(0, 1.0, small[0]["cloud"]), (1, 1.0, small[1]["cloud"]), (2, 1.0, small[2]["cloud"])],
                 [(2, 2.0, small[3]["cloud"]), (0, 2.0, dim), (1, 2.0, dim[:0])]]
        for k, clouds in enumerate(ticks):
            det.submit(clouds)
            link = det.link()
            assert link.members.tolist() == [c[0] for c in clouds] and not link.status.any()
            assert link.records.tolist() == ([0, 1, 2] if k == 0 else [0, 1, -1])
            flt.submit_linked(linked_scan_events(link), link)
            obs2 = det2.detect(clouds)
            flt2.submit(cloud_events(clouds, obs2))
            _same_fleets(flt, flt2, k, full=True)
            taken, status, seen = flt.link_status()
            assert taken.tolist() == [o.cloud_.shape[0] for _, o in obs2] and not status.any()
            _same_obs(det.collect(), obs2, k)
        assert flt.n().min() > 3 and obs2[1][1].cloud_.shape[0] == 0
    finally:
        for h in (det, det2, flt, flt2):
            h.close()


def test_refusals_change_nothing():
    """An entry used twice, a wrong member, an entry with a host status, an index outside the link, a tracked fleet, a linked scan
    through rfleet_submit, and link() without a submit: each has its code, and every member's state is what it was."""
    import copy
    from reflector_ekf_slam_amd import linked_scan_events
    from reflector_ekf_slam_amd.fleet import linked_scan_event, odom_event
    B, NB = 3, 720
    tw = Twins(B, NB)
    try:
        assert tw.det.link_code()[0] == INVALID                                  # nothing submitted
        tw.tick([(b, _scan(2 + b, NB, 1.0)) for b in range(B)], [tw.odometry(b, 0.9) for b in range(B)], 0)
        assert tw.det.link_code()[0] == INVALID                                  # collected
        before = _states(tw.flt)
        bad = _scan(2, NB, 2.0)
        bad.range_max = bad.range_min
        tw.det.submit([(0, _scan(2, NB, 2.0)), (1, bad), (2, _scan(3, NB, 2.0))])
        link = tw.det.link()
        good = linked_scan_events(link)
        assert [e[0] for e in good] == [0, 2] and link.status.tolist() == [0, -3, 0]
        calls = {"used twice": good + [linked_scan_event(0, 2.5, 0)],
                 "wrong member": [linked_scan_event(1, 2.0, 0)],
                 "host status": [linked_scan_event(1, 2.0, 1)],
                 "outside the link": good + [linked_scan_event(0, 2.5, 3)],
                 "negative entry": [linked_scan_event(0, 2.0, -1)]}
        moved = [odom_event(0, 1.9, 0.05, 0.0, 0.02)]                            # (a good event in front: it must not be applied either)
        for name, ev in calls.items():
            assert tw.flt.submit_linked_code(moved + ev, link) == INVALID, name
            assert _states(tw.flt) == before, name
        other = copy.copy(link)
        other.raw = type(link.raw).from_buffer_copy(link.raw)
        other.raw.device = link.raw.device + 1
        assert tw.flt.submit_linked_code(good, other) == INVALID and tw.flt.submit_linked_code(good, None) == INVALID
        assert tw.flt.submit_code(good) == INVALID                               # rfleet_submit refuses the kind
        tw.flt.track(True)
        assert tw.flt.submit_linked_code(good, link) == INVALID
        tw.flt.track(False)
        assert _states(tw.flt) == before
        assert tw.flt.link_counts()[0] == 1
        tw.flt.submit_linked(good, link)                                         # and the link is still good
        assert tw.flt.link_status()[0].tolist() == [2, 3]
        tw.det.collect()
    finally:
        tw.close()
