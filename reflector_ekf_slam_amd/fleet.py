"""Fleet filter: many small reflector EKF-SLAM sessions advanced by ONE kernel launch per call (include/rfleet.h).

``ReflectorEKFSLAMFleet(options_list)`` holds B independent filters (at most 128 reflectors each).  ``submit(events)`` hands
over any number of odometry / scan messages of any subset of members and enqueues one launch of k_fleet_step (one workgroup
per member with events); ``poses()`` reads all poses back.  A scan may carry an absolute pose fix (the reference's USE_GPS
deployment: ``predict_poses(times)`` -> scan matcher -> ``scan_event(..., pose_fix=matched_pose)``).  ``set_map(xy, cov)`` gives the
fleet ONE pre-loaded reflector map that its members localise against (the reference's LoadMapFromTxtFile deployment).  ``member(i)`` is a view with the snake_case filter interface of
``ReflectorEKFSLAM`` (each call a one-event submit), for code that drives one robot at a time.

What the node publishes after a scan comes from ONE more launch (k_fleet_reflectors), without a copy of any covariance matrix:
``marker_ellipses()`` (ReflectorToRosMarkers' covariance ellipses), ``landmarks()`` and ``save_map_txt`` (SaveReflectorResult).
The node's tick: detect -> predict_poses -> match -> fleet.submit -> marker_ellipses.

The pose and path stream (the node publishes the pose with its covariance after every odometry message and every scan that saw
reflectors) comes out of the step launch itself: after ``track()`` every ``submit`` also leaves one record per message -- the pose
AFTER that message -- in pinned host memory, and ``take_track()`` reads them with one synchronisation and no launch.

A scan of more than ``MAX_OBS`` observations is refused unless the fleet was made with ``wide_scans=True`` (or ``wide_scans()`` was
called): then scans of up to ``MAX_OBS_WIDE`` observations are taken, applied in exact block steps of 32 pairs by a kernel of its own
(k_fleet_step_wide), which a submit launches only when it holds such a scan; ``wide_counts()`` tells how often that happened.

The fleet's own state goes out and comes back as a fleet: ``snapshot(members)`` packs the listed members' full states (n, flags, time,
velocity, mean, the covariance's lower triangle) into one ``FleetSnapshot`` blob with ONE launch (k_fleet_pack), ``restore(snap, members)``
puts a blob's entries into any members of any fleet whose capacity holds them with ONE launch (k_fleet_unpack), zeros beyond n included:
a checkpoint (``save`` / ``load``), robots that move between fleets, a fleet seeded from yesterday's maps.

A tick whose scans come from a detector fleet needs no host between the two launches: ``submit_linked(events, det.link())`` takes
``linked_scan_event``s -- scans whose centres the detector's launch is still producing -- makes the fleet's stream wait for that launch
and lets ONE launch of k_fleet_bind move every scan's centres and count into the call's segment on the device, in front of the step
launch.  The tick: ``det.submit(scans)`` -> ``flt.submit_linked(odometry + fleet_detect.linked_scan_events(det.link()), link)`` ->
``flt.poses()`` (the one wait) -> ``det.collect()``.  ``link_status()`` tells which scans a bind left empty and why.

All arithmetic happens in the HIP kernel behind librfleet.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .ekf_slam import Map, ReflectorMatchResult, RekfError, State, loaded_map_rows, reflector_map_txt

RFLEET_ABI_VERSION = 2        # must equal RFLEET_ABI_VERSION of include/rfleet.h and rfleet_abi_version() of the built library
MAX_LANDMARKS = 128
MAX_OBS = 32
MAX_OBS_WIDE = 256            # per scan on a fleet with wide scans switched on (RFLEET_MAX_OBS_WIDE)
MAX_MAP_POINTS = 2048
EV_ODOM, EV_SCAN = 0, 1
EV_SCAN_LINKED = 2            # a scan of ``submit_linked`` whose observations are an entry of a detector fleet's link


class RfleetEvent(C.Structure):
    """struct rfleet_event (include/rfleet.h)."""
    _fields_ = [("member", C.c_int), ("kind", C.c_int), ("t", C.c_double), ("v", C.c_double * 3),
                ("xy", C.c_void_p), ("K", C.c_int), ("has_pose_fix", C.c_int), ("pose_fix", C.c_double * 3)]


def _declare_rfleet(L):
    """librfleet.so with argtypes set.  Raises LibraryMissing when it was not built or speaks another ABI version."""
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.rfleet_last_hip_error.restype = C.c_char_p
    L.rfleet_last_hip_error.argtypes = [vp]
    L.rfleet_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.rfleet_destroy.argtypes = [vp]
    L.rfleet_destroy.restype = None
    L.rfleet_submit.argtypes = [vp, vp, C.c_int]
    L.rfleet_get_poses.argtypes = [vp, vp, vp, vp]
    L.rfleet_predict_poses.argtypes = [vp, vp, vp, vp]
    L.rfleet_get_n.argtypes = [vp, vp]
    L.rfleet_get_flags.argtypes = [vp, vp]
    L.rfleet_get_state.argtypes = [vp, C.c_int, vp, ip, vp, C.c_long, vp, C.c_long]
    L.rfleet_set_state.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp, vp, vp]
    L.rfleet_get_last_match.argtypes = [vp, C.c_int, ip, vp, ip, vp, ip, vp]
    L.rfleet_sync.argtypes = [vp]
    L.rfleet_size.argtypes = [vp, ip, ip]


rfleet = _lib.Library("librfleet.so", ("rfleet_abi_version", RFLEET_ABI_VERSION), _declare_rfleet, [("rfleet_sizeof_event", RfleetEvent)])


def _declare_map(L):
    """``rfleet()`` with the argtypes of the map calls set.  They were added without a new ABI version and are looked up by name:
    raises LibraryMissing when the built library has none; every other call keeps working then."""
    L.rfleet_set_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.rfleet_get_map_size.argtypes = [C.c_void_p, C.POINTER(C.c_int)]


_map_lib = _lib.Feature(rfleet, "librfleet.so", ("rfleet_set_map", "rfleet_get_map_size"), (), _declare_map)


def _declare_reflectors(L):
    """``rfleet()`` with the argtypes of rfleet_get_reflectors set.  It was added without a new ABI version and is looked up by name:
    raises LibraryMissing when the built library has none; every other call keeps working then."""
    L.rfleet_get_reflectors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]


_reflectors_lib = _lib.Feature(rfleet, "librfleet.so", ("rfleet_get_reflectors",), (), _declare_reflectors)


def _declare_wide(L):
    """``rfleet()`` with the argtypes of the wide-scan calls set.  They were added without a new ABI version and are looked up by
    name: raises LibraryMissing when the built library has none; every other call keeps working then."""
    ip = C.POINTER(C.c_int)
    L.rfleet_set_wide_scans.argtypes = [C.c_void_p, C.c_int]
    L.rfleet_get_last_match_wide.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, C.c_void_p, ip, C.c_void_p, ip, C.c_void_p]
    L.rfleet_wide_counts.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]


_wide_lib = _lib.Feature(rfleet, "librfleet.so", ("rfleet_set_wide_scans", "rfleet_get_last_match_wide", "rfleet_wide_counts"), (),
                         _declare_wide)


class RfleetTrackRec(C.Structure):
    """struct rfleet_track_rec (include/rfleet.h)."""
    _fields_ = [("t", C.c_double), ("mu3", C.c_double * 3), ("sigma3x3", C.c_double * 9), ("member", C.c_int), ("kind", C.c_int),
                ("K", C.c_int), ("dropped", C.c_int), ("n", C.c_int), ("flags", C.c_int), ("n_state", C.c_int), ("n_map", C.c_int),
                ("n_new", C.c_int), ("pad_", C.c_int)]


TRACK_DTYPE = np.dtype([("t", "<f8"), ("mu3", "<f8", (3,)), ("sigma3x3", "<f8", (9,)), ("member", "<i4"), ("kind", "<i4"), ("K", "<i4"),
                        ("dropped", "<i4"), ("n", "<i4"), ("flags", "<i4"), ("n_state", "<i4"), ("n_map", "<i4"), ("n_new", "<i4"),
                        ("pad_", "<i4")])
assert TRACK_DTYPE.itemsize == C.sizeof(RfleetTrackRec)


def _declare_track(L):
    """``rfleet()`` with the argtypes of the pose track's calls set.  They were added without a new ABI version and are looked up by
    name: raises LibraryMissing when the built library has none; every other call keeps working then."""
    L.rfleet_set_tracking.argtypes = [C.c_void_p, C.c_int, C.c_long]
    L.rfleet_take_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]


_track_lib = _lib.Feature(rfleet, "librfleet.so", ("rfleet_set_tracking", "rfleet_take_track"), [("rfleet_sizeof_track_rec", RfleetTrackRec)],
                          _declare_track)


class RfleetSnapshotHdr(C.Structure):
    """struct rfleet_snapshot_hdr (include/rfleet.h)."""
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_int), ("count", C.c_int), ("bytes", C.c_long)]


class RfleetSnapshotMember(C.Structure):
    """struct rfleet_snapshot_member (include/rfleet.h)."""
    _fields_ = [("t", C.c_double), ("vt", C.c_double * 3), ("member", C.c_int), ("n", C.c_int), ("flags", C.c_int), ("pad_", C.c_int),
                ("off", C.c_long)]


SNAPSHOT_MAGIC = b"RFLTSNAP"
SNAPSHOT_VERSION = 1
SNAPSHOT_HDR_DTYPE = np.dtype([("magic", "S8"), ("version", "<i4"), ("count", "<i4"), ("bytes", "<i8")])
SNAPSHOT_MEMBER_DTYPE = np.dtype([("t", "<f8"), ("vt", "<f8", (3,)), ("member", "<i4"), ("n", "<i4"), ("flags", "<i4"), ("pad_", "<i4"),
                                  ("off", "<i8")])
assert SNAPSHOT_HDR_DTYPE.itemsize == C.sizeof(RfleetSnapshotHdr) and SNAPSHOT_MEMBER_DTYPE.itemsize == C.sizeof(RfleetSnapshotMember)


def _declare_snapshot(L):
    """``rfleet()`` with the argtypes of the snapshot calls set.  They were added without a new ABI version and are looked up by
    name: raises LibraryMissing when the built library has none; every other call keeps working then."""
    lp = C.POINTER(C.c_long)
    L.rfleet_snapshot.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_long, lp]
    L.rfleet_restore.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int]
    L.rfleet_snapshot_peek.argtypes = [C.c_void_p, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int)]


_snapshot_lib = _lib.Feature(rfleet, "librfleet.so", ("rfleet_snapshot", "rfleet_restore", "rfleet_snapshot_peek"),
                             [("rfleet_sizeof_snapshot_member", RfleetSnapshotMember), ("rfleet_sizeof_snapshot_hdr", RfleetSnapshotHdr)],
                             _declare_snapshot)


def _declare_link(L):
    """``rfleet()`` with the argtypes of the linked submit's calls set.  They were added without a new ABI version and are looked up
    by name: raises LibraryMissing when the built library has none; every other call keeps working then."""
    lp = C.POINTER(C.c_long)
    L.rfleet_submit_linked.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.rfleet_link_status.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.rfleet_link_counts.argtypes = [C.c_void_p, lp, lp, lp, lp]


_link_lib = _lib.Feature(rfleet, "librfleet.so", ("rfleet_submit_linked", "rfleet_link_status", "rfleet_link_counts"),
                         [("rfleet_sizeof_link", _lib.Rlink)], _declare_link)


class FleetSnapshot:
    """The full states of some members of a fleet as ONE blob of bytes (``blob``, np.uint8; the layout is include/rfleet.h's): what
    ``ReflectorEKFSLAMFleet.snapshot`` returns and ``restore`` takes.  Entry g is the g-th member listed.  Views of the blob:

        members [G]      the index each entry was taken from
        t [G], vt [G, 3] state time and last odometry velocity
        n [G], flags [G] state dimension and sticky REKF_FLAGBIT_* bits
        mu(g) [n]        the mean
        triangle(g)      the covariance's packed lower triangle, n (n + 1) / 2 doubles, column-major: column j holds rows j .. n-1

    and, computed on demand, ``sigma(g)`` (the mirrored dense matrix) and ``state(g)`` (a ``State``).  ``save(path)`` writes the
    blob's bytes and nothing else; ``FleetSnapshot.load(path)`` reads and validates them."""

    def __init__(self, blob, validate: bool = True):
        self.blob = blob if (type(blob) is np.ndarray and blob.dtype == np.uint8 and blob.ndim == 1 and blob.flags.c_contiguous) \
            else np.frombuffer(bytes(blob), np.uint8).copy()
        if validate:
            count, max_n = C.c_int(), C.c_int()
            rc = _snapshot_lib().rfleet_snapshot_peek(self.blob.ctypes.data if self.blob.size else None, self.blob.size,
                                                      C.byref(count), C.byref(max_n))
            if rc != 0:
                raise RekfError(rc, "rfleet_snapshot_peek")
        hdr = self.blob[:SNAPSHOT_HDR_DTYPE.itemsize].view(SNAPSHOT_HDR_DTYPE)[0]
        self._entries = self.blob[SNAPSHOT_HDR_DTYPE.itemsize:][: int(hdr["count"]) * SNAPSHOT_MEMBER_DTYPE.itemsize].view(SNAPSHOT_MEMBER_DTYPE)

    def __len__(self):
        return self._entries.shape[0]

    members = property(lambda self: self._entries["member"])
    t = property(lambda self: self._entries["t"])
    vt = property(lambda self: self._entries["vt"])
    n = property(lambda self: self._entries["n"])
    flags = property(lambda self: self._entries["flags"])

    @property
    def max_n(self) -> int:
        return int(self.n.max()) if len(self) else 0

    def _doubles(self, g, at, k):
        off = int(self._entries["off"][g]) + 8 * at
        return self.blob[off: off + 8 * k].view(np.float64)

    def mu(self, g: int) -> np.ndarray:
        return self._doubles(g, 0, int(self.n[g]))

    def triangle(self, g: int) -> np.ndarray:
        n = int(self.n[g])
        return self._doubles(g, n, n * (n + 1) // 2)

    def sigma(self, g: int) -> np.ndarray:
        n = int(self.n[g])
        s = np.zeros((n, n))
        cols, rows = np.triu_indices(n)                     # (row-major order of the upper triangle = column-major of the lower)
        s[rows, cols] = self.triangle(g)
        s[cols, rows] = s[rows, cols]
        return s

    def state(self, g: int) -> State:
        return State(float(self.t[g]), self.mu(g).copy(), self.sigma(g))

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.blob.tobytes())

    @classmethod
    def load(cls, path) -> "FleetSnapshot":
        with open(path, "rb") as f:
            return cls(np.frombuffer(f.read(), np.uint8).copy())


_TRACK_FIELDS = ("t", "kind", "K", "dropped", "mu", "sigma", "n", "flags", "n_state", "n_map", "n_new")


class MemberTrack:
    """One member's part of ``take_track``: R records, oldest first, each the member's state AFTER one message.

        t [R]            the messages' stamps
        kind [R]         EV_ODOM / EV_SCAN
        K [R]            observations of a scan message
        dropped [R]      1: a message the filter ignores (stale or use_imu odometry); the record repeats the state before it
        mu [R, 3], sigma [R, 3, 3] (oriented as ``poses()`` returns it)
        n [R], flags [R] state dimension and sticky REKF_FLAGBIT_* after the message
        n_state, n_map, n_new [R]   the scan's match counts (zero for odometry)
        lost             records the bounded log discarded since the previous take

    The arrays are views of rows [at, at + R) of one array per field that the members of a take share, made when they are read."""
    __slots__ = ("_cols", "_at", "_R", "lost")

    def __init__(self, t, kind, K, dropped, mu, sigma, n, flags, n_state, n_map, n_new, lost=0, at=0, rows=None):
        self._cols = (t, kind, K, dropped, mu, sigma, n, flags, n_state, n_map, n_new)
        self._at = at
        self._R = len(t) - at if rows is None else rows
        self.lost = lost

    def __len__(self):
        return self._R


def _track_field(i):
    return property(lambda self: self._cols[i][self._at: self._at + self._R])


for _i, _name in enumerate(_TRACK_FIELDS):
    setattr(MemberTrack, _name, _track_field(_i))


def odom_event(member, t, vx, vy, wz):
    return (int(member), EV_ODOM, float(t), (float(vx), float(vy), float(wz)), None)


def scan_event(member, t, cloud, pose_fix=None):
    """pose_fix: (x, y, yaw) of an absolute pose observation taken at the scan's time (reflector_ekf_slam_gps.cc:305-340), or None."""
    if pose_fix is None:
        return (int(member), EV_SCAN, float(t), (0.0, 0.0, 0.0), cloud)
    return (int(member), EV_SCAN, float(t), (0.0, 0.0, 0.0), cloud, tuple(float(v) for v in pose_fix))


def linked_scan_event(member, t, entry, pose_fix=None):
    """A scan whose observations are entry ``entry`` of the link handed to ``submit_linked`` (a detector fleet's ``link()``): the
    filter's host never sees them.  ``t``: the entry's stamp; pose_fix as for ``scan_event``."""
    if pose_fix is None:
        return (int(member), EV_SCAN_LINKED, float(t), (0.0, 0.0, 0.0), int(entry))
    return (int(member), EV_SCAN_LINKED, float(t), (0.0, 0.0, 0.0), int(entry), tuple(float(v) for v in pose_fix))


class ReflectorEKFSLAMFleet(_lib.Handle):
    """B independent ekf::ReflectorEKFSLAM filters on one MI355X, one kernel launch per ``submit``."""
    _destroy = "rfleet_destroy"
    _map = None                   # (Map, per-member switch or None) of the last successful set_map
    _wide = False                 # wide_scans() has been called: records may be wider than MAX_OBS

    def __init__(self, options_list, max_landmarks: int = MAX_LANDMARKS, device: int = 0, wide_scans: bool = False):
        self._L = rfleet()
        self._h = None
        self.options = list(options_list)
        B = len(self.options)
        arr = (_lib.RekfOptions * max(B, 1))()
        for i, options in enumerate(self.options):
            o = arr[i]
            o.odom_model = int(options.odom_model)
            o.use_imu = 1 if options.use_imu else 0
            o.init_time = float(options.init_time)
            for k in range(3):
                o.init_pose[k] = float(options.init_pose[k])
            o.linear_velocity_cov = float(options.linear_velocity_cov)
            o.angular_velocity_cov = float(options.angular_velocity_cov)
            o.observation_cov = float(options.observation_cov)
        h = C.c_void_p()
        rc = self._L.rfleet_create(C.cast(arr, C.c_void_p), B, int(max_landmarks), int(device), C.byref(h))
        if rc != 0:
            raise RekfError(rc, "rfleet_create")
        self._h = h
        self.B = B
        self.max_landmarks = int(max_landmarks)
        if wide_scans:
            self.wide_scans(True)

    def __len__(self):
        return self.B

    def _error(self, rc, where):
        return RekfError(rc, where, self._L.rfleet_last_hip_error(self._h).decode())

    # -- the fleet interface --------------------------------------------------
    @staticmethod
    def pack(events):
        """events: iterable of (member, kind, t, (vx, vy, wz), cloud or None[, pose fix (x, y, yaw) or None]) -- see
        ``odom_event`` / ``scan_event`` -- or ``RfleetEvent``s.  -> (ctypes array, the float32 arrays it points into): reusable with ``submit_packed``."""
        events = list(events)
        arr = (RfleetEvent * max(len(events), 1))()
        keep = []
        for i, ev in enumerate(events):
            if isinstance(ev, RfleetEvent):
                arr[i] = ev
                continue
            member, kind, t, v, cloud = ev[:5]
            fix = ev[5] if len(ev) > 5 else None
            e = arr[i]
            e.member, e.kind, e.t = int(member), int(kind), float(t)
            e.v[0], e.v[1], e.v[2] = float(v[0]), float(v[1]), float(v[2])
            if kind == EV_SCAN and cloud is not None:
                if not (type(cloud) is np.ndarray and cloud.dtype == np.float32 and cloud.flags.c_contiguous):
                    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
                if cloud.size & 1:
                    raise ValueError("observations are (x, y) pairs")
                keep.append(cloud)
                e.xy = cloud.ctypes.data if cloud.size else None
                e.K = cloud.size >> 1
            elif kind == EV_SCAN_LINKED:
                e.K = int(cloud)                             # (the entry of the link: ``linked_scan_event``)
            if fix is not None:
                e.has_pose_fix = 1
                e.pose_fix[0], e.pose_fix[1], e.pose_fix[2] = float(fix[0]), float(fix[1]), float(fix[2])
        return arr, len(events), keep

    def submit_code(self, events) -> int:
        arr, count, _keep = self.pack(events)
        return self._L.rfleet_submit(self._h, C.cast(arr, C.c_void_p), count)

    def submit(self, events):
        """Apply the events (a member's in the order given) with ONE kernel launch; returns without waiting for it."""
        rc = self.submit_code(events)
        if rc != 0:
            self._chk(rc, "rfleet_submit")

    def submit_packed(self, packed):
        rc = self._L.rfleet_submit(self._h, C.cast(packed[0], C.c_void_p), packed[1])
        if rc != 0:
            self._chk(rc, "rfleet_submit")

    # -- the detector's centres bound on the device ------------------------------------
    def submit_linked_code(self, events, link) -> int:
        """rfleet_submit_linked as it is: ``link`` a ``fleet_detect.DetectLink``, a ``_lib.Rlink`` or None."""
        arr, count, _keep = self.pack(events)
        raw = getattr(link, "raw", link)
        return _link_lib().rfleet_submit_linked(self._h, C.cast(arr, C.c_void_p), count, None if raw is None else C.addressof(raw))

    def submit_linked(self, events, link):
        """``submit`` for a call that holds ``linked_scan_event``s (``fleet_detect.linked_scan_events(link)``): scans whose centres
        the detector fleet's launch is still producing.  The host waits for nothing and never sees the centres: the fleet's stream
        waits for the detector's launch, ONE launch of k_fleet_bind moves every linked scan's centres and count into the call's
        segment, and the step launch follows.  A scan whose record holds an error or more centres than the fleet takes is applied as
        an EMPTY scan (``link_status`` tells).  Everything is validated first; events of the other kinds may be mixed in."""
        rc = self.submit_linked_code(events, link)
        if rc != 0:
            self._chk(rc, "rfleet_submit_linked")

    def link_status(self):
        """-> (taken [S], status [S], K_seen [S]) of the S linked scans of the last ``submit_linked`` that held one, in event order:
        the centres the filter took, 0 or why it took none (the record's own error, -4 for a count outside the record, -3 for more
        than the fleet takes), and the count as read.  Synchronises."""
        L = _link_lib()
        cap = 64
        while True:
            out = np.zeros((3, cap), np.int32)
            n = L.rfleet_link_status(self._h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, cap)
            if n != -6:                                      # (REKF_ERR_BUFFER: more linked scans than ``cap``)
                break
            cap *= 4
        if n < 0:
            self._chk(n, "rfleet_link_status")
        return out[0, :n].copy(), out[1, :n].copy(), out[2, :n].copy()

    def link_counts(self):
        """-> (linked submits, launches of k_fleet_bind, linked scans, linked scans a bind left empty) since the fleet was made.
        Host counters; the last is brought up to date by ``link_status``."""
        v = [C.c_long() for _ in range(4)]
        self._chk(_link_lib().rfleet_link_counts(self._h, *(C.byref(x) for x in v)), "rfleet_link_counts")
        return tuple(int(x.value) for x in v)

    def poses(self):
        """-> (t [B], mu [B, 3], sigma [B, 3, 3]) of all members.  Synchronises; no copy of any state."""
        t = np.zeros(self.B)
        mu = np.zeros((self.B, 3))
        sg = np.zeros((self.B, 9))
        self._chk(self._L.rfleet_get_poses(self._h, t.ctypes.data, mu.ctypes.data, sg.ctypes.data), "rfleet_get_poses")
        return t, mu, sg.reshape(self.B, 3, 3).transpose(0, 2, 1).copy()

    def predict_poses(self, times):
        """PredictState's pose block of every member at ``times`` (a scalar or [B]): -> (mu [B, 3], sigma [B, 3, 3]), from each
        member's state time with its last odometry velocity.  Non-mutating; synchronises, launches nothing."""
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(times, dtype=np.float64), (self.B,)))
        mu = np.zeros((self.B, 3))
        sg = np.zeros((self.B, 9))
        self._chk(self._L.rfleet_predict_poses(self._h, t.ctypes.data, mu.ctypes.data, sg.ctypes.data), "rfleet_predict_poses")
        return mu, sg.reshape(self.B, 3, 3).transpose(0, 2, 1).copy()

    def n(self) -> np.ndarray:
        out = np.zeros(self.B, np.int32)
        self._chk(self._L.rfleet_get_n(self._h, out.ctypes.data), "rfleet_get_n")
        return out

    def flags(self) -> np.ndarray:
        """Sticky REKF_FLAGBIT_* bits per member, not cleared."""
        out = np.zeros(self.B, np.int32)
        self._chk(self._L.rfleet_get_flags(self._h, out.ctypes.data), "rfleet_get_flags")
        return out

    def sync(self):
        self._chk(self._L.rfleet_sync(self._h), "rfleet_sync")

    def member(self, i: int) -> "FleetMember":
        if not 0 <= int(i) < self.B:
            raise IndexError(i)
        return FleetMember(self, int(i))

    # -- per member -------------------------------------------------------------
    def get_state(self, i: int, want_sigma: bool = True) -> State:
        n = int(self.n()[i])
        mu = np.zeros(n)
        sig = np.zeros((n, n), order="F") if want_sigma else None
        t = C.c_double()
        nn = C.c_int()
        self._chk(self._L.rfleet_get_state(self._h, int(i), C.addressof(t), C.byref(nn), mu.ctypes.data, n,
                                           sig.ctypes.data if want_sigma else None, n * n if want_sigma else 0),
                  "rfleet_get_state")
        return State(t.value, mu, sig)

    def set_state(self, i: int, t, mu, sigma, vt=None):
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        n = mu.shape[0]
        flat = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).T).reshape(-1)   # column-major bytes
        v = None
        if vt is not None:
            vv = np.ascontiguousarray(vt, dtype=np.float64)
            v = vv.ctypes.data
        self._chk(self._L.rfleet_set_state(self._h, int(i), float(t), n, mu.ctypes.data, flat.ctypes.data, v),
                  "rfleet_set_state")

    def last_match(self, i: int) -> ReflectorMatchResult:
        """The member's last scan (a wide one too: the lists are sized for ``MAX_OBS_WIDE`` once wide scans were switched on)."""
        cap = MAX_OBS_WIDE if self._wide else MAX_OBS
        sp = np.zeros((cap, 2), np.int32)
        mp = np.zeros((cap, 2), np.int32)
        nw = np.zeros((cap,), np.int32)
        ns, nm, nn = C.c_int(), C.c_int(), C.c_int()
        if self._wide:
            self._chk(_wide_lib().rfleet_get_last_match_wide(self._h, int(i), cap, C.byref(ns), sp.ctypes.data, C.byref(nm),
                                                             mp.ctypes.data, C.byref(nn), nw.ctypes.data), "rfleet_get_last_match_wide")
        else:
            self._chk(self._L.rfleet_get_last_match(self._h, int(i), C.byref(ns), sp.ctypes.data, C.byref(nm), mp.ctypes.data,
                                                    C.byref(nn), nw.ctypes.data), "rfleet_get_last_match")
        return ReflectorMatchResult(mp[: nm.value].copy(), sp[: ns.value].copy(), nw[: nn.value].copy())

    # -- wide scans -----------------------------------------------------------------
    def wide_scans(self, on: bool = True):
        """Switches wide scans on or off for every later ``submit``: on, a scan may hold up to ``MAX_OBS_WIDE`` observations (more
        raises, before anything moves); off (the default), more than ``MAX_OBS`` raises as ever.  Switching on allocates the members'
        wide match records and launches nothing; a submit without a wide scan launches exactly what it launched before."""
        self._chk(_wide_lib().rfleet_set_wide_scans(self._h, 1 if on else 0), "rfleet_set_wide_scans")
        self._wide = self._wide or bool(on)                  # (records written while it was on stay readable)

    def wide_counts(self):
        """-> (launches of k_fleet_step_wide, scans wider than ``MAX_OBS`` submitted) since the fleet was made.  Host counters."""
        a, b = C.c_long(), C.c_long()
        self._chk(_wide_lib().rfleet_wide_counts(self._h, C.byref(a), C.byref(b)), "rfleet_wide_counts")
        return int(a.value), int(b.value)

    # -- the shared pre-loaded map ------------------------------------------------
    def set_map_code(self, xy, cov, members=None) -> int:
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, 4)
        if xy.shape[0] != cov.shape[0]:
            raise ValueError("one 2 x 2 weight per map point")
        use = None
        if members is not None:
            use = np.zeros(self.B, np.uint8)
            use[np.asarray(list(members), np.int64)] = 1
        M = xy.shape[0]
        rc = _map_lib().rfleet_set_map(self._h, xy.ctypes.data if M else None, cov.ctypes.data if M else None, M,
                                       None if use is None else use.ctypes.data)
        if rc == 0:                                          # (kept for save_map_txt: the saved map lists the pre-loaded points first)
            self._map = (Map(xy.copy(), cov.reshape(-1, 2, 2).copy()), use) if M else None
        return rc

    def set_map(self, xy, cov, members=None):
        """The fleet's pre-loaded reflector map (sensor::Map as LoadMapFromTxtFile leaves it): xy [M, 2] float32, cov [M, 2, 2]
        weights, M <= MAX_MAP_POINTS; an empty map clears it.  ``members``: the indices of the members that match against it
        (None = all).  Synchronises; holds from the next ``submit``.  The map is the fleet's: a member has no map of its own."""
        rc = self.set_map_code(xy, cov, members)
        if rc != 0:
            self._chk(rc, "rfleet_set_map")

    def map_size(self) -> int:
        M = C.c_int()
        self._chk(_map_lib().rfleet_get_map_size(self._h, C.byref(M)), "rfleet_get_map_size")
        return M.value

    def loaded_map(self, i: int) -> Map | None:
        """The pre-loaded map member i matches against (``set_map``), or None."""
        if self._map is None or (self._map[1] is not None and not self._map[1][int(i)]):
            return None
        return self._map[0]

    # -- the pose track: every member's pose after every message, written by the step launch itself -----------------
    def track(self, on: bool = True, max_records: int = 0):
        """Switches the pose track on or off for every later ``submit``: the launch then also leaves one record per message in
        pinned host memory (no further launch, no synchronisation).  ``max_records`` bounds the host-side log per member (0 = 1024):
        when it is full the oldest record goes and is counted in ``lost``.  Switching off keeps what is logged."""
        self._chk(_track_lib().rfleet_set_tracking(self._h, 1 if on else 0, int(max_records)), "rfleet_set_tracking")

    def take_track_code(self, members, counts, out, cap_rows, lost) -> int:
        """rfleet_take_track as it is (for tests): numpy arrays or None."""
        mem = None if members is None else np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        count = self.B if mem is None else mem.shape[0]
        return _track_lib().rfleet_take_track(self._h, None if mem is None else mem.ctypes.data, count,
                                              None if counts is None else counts.ctypes.data, None if out is None else out.ctypes.data,
                                              int(cap_rows), None if lost is None else lost.ctypes.data)

    def take_track(self, members=None):
        """-> a list of ``MemberTrack``, one per listed member (None = all, in order): the records logged since the previous take,
        oldest first; they leave the log.  One synchronisation and no launch, whatever the number of members and messages."""
        count = self.B if members is None else len(np.asarray(members).reshape(-1))
        counts = np.zeros(max(count, 1), np.int32)
        lost = np.zeros(max(count, 1), np.int64)
        rc = self.take_track_code(members, counts, None, 0, None)                      # the sizing call
        if rc != 0:
            self._chk(rc, "rfleet_take_track")
        rows = int(counts[:count].sum())
        out = np.zeros(max(rows, 1), TRACK_DTYPE)
        rc = self.take_track_code(members, counts, out, rows, lost)
        if rc != 0:
            self._chk(rc, "rfleet_take_track")
        out = out[:rows]
        cols = [np.ascontiguousarray(out[k]) for k in ("t", "kind", "K", "dropped", "mu3")]      # one copy per field, members are slices
        cols.append(out["sigma3x3"].reshape(-1, 3, 3).transpose(0, 2, 1).copy())
        cols += [np.ascontiguousarray(out[k]) for k in ("n", "flags", "n_state", "n_map", "n_new")]
        res, at = [], 0
        for k, ls in zip(counts[:count].tolist(), lost[:count].tolist()):
            res.append(MemberTrack(*cols, ls, at, k))
            at += k
        return res

    # -- the fleet's own state: out as one blob with one launch, back in with one launch -----------------
    def snapshot_code(self, members, out, cap_bytes, size) -> int:
        """rfleet_snapshot as it is (for tests): numpy arrays or None, ``size`` a ctypes.c_long."""
        mem = None if members is None else np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        count = self.B if mem is None else mem.shape[0]
        if count == 0:
            mem = np.zeros(1, np.int32)                      # (an empty list is still a list: a pointer that is not NULL)
        return _snapshot_lib().rfleet_snapshot(self._h, None if mem is None else mem.ctypes.data, count,
                                               None if out is None else out.ctypes.data, int(cap_bytes), C.byref(size))

    def snapshot(self, members=None) -> FleetSnapshot:
        """The full states of the listed members (None = all, in order) -- n, flags, time, velocity, mean, the covariance's lower
        triangle -- as one ``FleetSnapshot``: a size call, one buffer, ONE launch of k_fleet_pack whatever the number of members.
        Every event submitted before is in it; nothing in the fleet changes."""
        size = C.c_long()
        rc = self.snapshot_code(members, None, 0, size)                                # the sizing call
        if rc != 0:
            self._chk(rc, "rfleet_snapshot")
        blob = np.zeros(size.value, np.uint8)
        rc = self.snapshot_code(members, blob, blob.size, size)
        if rc != 0:
            self._chk(rc, "rfleet_snapshot")
        return FleetSnapshot(blob[: size.value], validate=False)

    def restore_code(self, snap, members=None) -> int:
        blob = snap.blob if isinstance(snap, FleetSnapshot) else np.ascontiguousarray(snap, dtype=np.uint8).reshape(-1)
        mem = None if members is None else np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        if mem is None:
            count = int(blob[12:16].view(np.int32)[0]) if blob.size >= 16 else 0
        else:
            count = mem.shape[0]
            if count == 0:
                mem = np.zeros(1, np.int32)
        return _snapshot_lib().rfleet_restore(self._h, blob.ctypes.data if blob.size else None, blob.size,
                                              None if mem is None else mem.ctypes.data, count)

    def restore(self, snap, members=None):
        """Entry g of ``snap`` (a ``FleetSnapshot``, of this fleet or another) becomes member ``members[g]`` (None: the index it was
        taken from): n, flags, time, velocity, mean and covariance from the blob, zeros beyond n, a last-match record of zero counts.
        Everything is validated before anything moves (every n must fit this fleet's capacity, targets distinct); then one copy to
        the device and ONE launch of k_fleet_unpack.  Members not listed keep every bit; the pose track logs nothing."""
        rc = self.restore_code(snap, members)
        if rc != 0:
            self._chk(rc, "rfleet_restore")

    # -- what the node publishes: the reflectors of any list of members in one launch ----------------
    def reflectors(self, members=None, ellipses=True, xy=False, cov=False):
        """-> (counts [len(members)], ellipses [R, 5] or None, xy [R, 2] or None, cov [R, 2, 2] or None): the rows of the listed
        members (None = all, in order) one after the other, R = counts.sum().  ONE launch behind everything submitted and one
        synchronisation, whatever the number of members; no copy of any state."""
        L = _reflectors_lib()
        if members is None:
            mem, count = None, self.B
        else:
            mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
            count = mem.shape[0]
        cap = count * self.max_landmarks
        counts = np.zeros(max(count, 1), np.int32)
        e = np.empty((cap, 5)) if ellipses else None
        p = np.empty((cap, 2)) if xy else None
        c = np.empty((cap, 2, 2)) if cov else None
        rc = L.rfleet_get_reflectors(self._h, None if mem is None else mem.ctypes.data, count, counts.ctypes.data,
                                     None if e is None else e.ctypes.data, None if p is None else p.ctypes.data,
                                     None if c is None else c.ctypes.data, cap)
        if rc != 0:
            self._chk(rc, "rfleet_get_reflectors")
        counts = counts[:count]
        R = int(counts.sum())
        return counts, None if e is None else e[:R], None if p is None else p[:R], None if c is None else c[:R]

    @staticmethod
    def _per_member(counts, rows):
        out, at = [], 0
        for k in counts.tolist():
            out.append(rows[at: at + k])
            at += k
        return out

    def marker_ellipses(self, members=None):
        """ReflectorToRosMarkers' covariance ellipses (src/ros_node.cc:736-791) of the listed members (None = all): a list of
        [L_b, 5] arrays {mx, my, angle, x_len, y_len}, the bits ``ReflectorEKFSLAM.marker_ellipses`` gives for the same state."""
        counts, e, _, _ = self.reflectors(members, ellipses=True)
        return self._per_member(counts, e)

    def landmarks(self, members=None):
        """-> a list of (xy [L_b, 2], cov [L_b, 2, 2]) of the listed members (None = all): each reflector's mean and its
        covariance block as ``get_state`` mirrors it."""
        counts, _, p, c = self.reflectors(members, ellipses=False, xy=True, cov=True)
        return list(zip(self._per_member(counts, p), self._per_member(counts, c)))

    def save_map_txt(self, member: int, path: str, reference_bytes: bool = False):
        """SaveReflectorResult (src/ros_node.cc:75-140) for one member, the bytes of ``ekf_slam.save_map_txt`` on its state: the
        shared pre-loaded map's points first when the member uses one, then the member's reflectors."""
        if not 0 <= int(member) < self.B:
            raise IndexError(member)
        (xy, cov), = self.landmarks([int(member)])
        pts, covs = loaded_map_rows(self.loaded_map(member))
        n_loaded = len(pts)
        pts.extend(xy)
        covs.extend(cov.reshape(-1, 4))
        with open(path, "wb") as f:
            f.write(reflector_map_txt(pts, covs, n_loaded, reference_bytes))


class FleetMember:
    """One member of a fleet with the snake_case filter interface; every message is a one-event ``submit``."""

    def __init__(self, fleet: ReflectorEKFSLAMFleet, index: int):
        self.fleet = fleet
        self.index = index

    def handle_odometry(self, t, vx, vy, wz):
        self.fleet.submit([odom_event(self.index, t, vx, vy, wz)])

    def handle_observation(self, t, cloud, gps_pose=None):
        self.fleet.submit([scan_event(self.index, t, cloud, gps_pose)])

    def PredictState(self, t):
        """-> (mu3, sigma 3 x 3): the pose block of PredictState(t).  Evaluates every member's (host arithmetic on B poses)."""
        t_now = self.fleet.poses()[0]
        t_now[self.index] = float(t)
        mu, sg = self.fleet.predict_poses(t_now)
        return mu[self.index].copy(), sg[self.index].copy()

    @property
    def n(self) -> int:
        return int(self.fleet.n()[self.index])

    def mu(self) -> np.ndarray:
        return self.fleet.get_state(self.index, want_sigma=False).mu

    def GetState(self) -> State:
        return self.fleet.get_state(self.index)

    def set_state(self, t, mu, sigma, vt=None):
        self.fleet.set_state(self.index, t, mu, sigma, vt)

    def last_match(self) -> ReflectorMatchResult:
        return self.fleet.last_match(self.index)

    def wide_scans(self, on: bool = True):
        """The switch is the fleet's: it holds for every member."""
        self.fleet.wide_scans(on)

    def marker_ellipses(self) -> np.ndarray:
        return self.fleet.marker_ellipses([self.index])[0]

    def pose(self):
        t, mu, sg = self.fleet.poses()
        return float(t[self.index]), mu[self.index].copy(), sg[self.index].copy()

    def flags(self) -> int:
        return int(self.fleet.flags()[self.index])

    def sync(self):
        self.fleet.sync()

    def sync_code(self) -> int:
        return self.fleet._L.rfleet_sync(self.fleet._h)

