"""Fleet detectors: the 2D and the 3D reflector detector for many robots, ONE kernel launch per tick (rdet2d_batch_* and
rdet3d_batch_* of include/rdet.h).

``LaserReflectorDetectFleet(options_list)`` holds B members, each a reflector_detect::LaserReflectorDetect with its own options,
sensor_to_base_link and odometry.  ``submit(scans)`` takes at most one ``LaserScan`` per member and enqueues one launch of
k_det2d_batch (one workgroup per scan); ``collect()`` waits and returns ``(status, Observation)`` per scan, in the order given.
``scan_events`` turns a tick's result into the events ``ReflectorEKFSLAMFleet.submit`` takes; ``range_data(members)`` is GetRangeData
of any list of members -- what ``FleetMapBuilder.AddRangeData`` takes -- from ONE launch of k_det2d_batch_range_data.

``PointCloudReflectorDetectFleet(options_list)`` is the same for reflector_detect::PointCloudReflectorDetect: ``submit(clouds)`` takes
at most one cloud per member, ``(member, stamp, xyzi)`` or ``(member, PointCloud)``, and enqueues one launch of k_det3d_batch (one
workgroup per cloud).  ``scan_events`` takes its ticks in the second form, ``cloud_events`` in the first.

All arithmetic happens in the HIP kernels behind librdet.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, fleet
from .detect import MAX_CENTERS, LaserScan, RangeData, Rdet2dOptions, Rdet3dOptions, RdetError, _as_f32, _rdet
from .ekf_slam import Observation, OdometryData

MAX_BEAMS = 8192
RDET_ERR_BAD_SCAN = -3


class Rdet2dScan(C.Structure):
    """struct rdet2d_scan (include/rdet.h)."""
    _fields_ = [("member", C.c_int), ("stamp", C.c_double), ("angle_min", C.c_float), ("angle_max", C.c_float),
                ("angle_increment", C.c_float), ("scan_time", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float),
                ("ranges", C.c_void_p), ("intensities", C.c_void_p), ("N", C.c_int)]


class Rdet3dCloud(C.Structure):
    """struct rdet3d_cloud (include/rdet.h)."""
    _fields_ = [("member", C.c_int), ("stamp", C.c_double), ("xyzi", C.c_void_p), ("N", C.c_int)]


@dataclass
class PointCloud:
    """What HandlePointCloud reads of a sensor_msgs::PointCloud2: the stamp and N points (x, y, z, intensity)."""
    stamp: float
    xyzi: np.ndarray


def _declare_batch(L):
    """librdet.so with the rdet2d_batch_* argtypes set.  Raises LibraryMissing when it was not built, or was built without them."""
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.rdet2d_batch_last_hip_error.restype = C.c_char_p
    L.rdet2d_batch_last_hip_error.argtypes = [vp]
    L.rdet2d_batch_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.rdet2d_batch_destroy.argtypes = [vp]
    L.rdet2d_batch_destroy.restype = None
    L.rdet2d_batch_set_sensor_to_base_link.argtypes = [vp, C.c_int, vp]
    L.rdet2d_batch_handle_odometry.argtypes = [vp, C.c_int, C.c_double, vp, vp, C.c_double, C.c_double, C.c_double]
    L.rdet2d_batch_staging.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.rdet2d_batch_submit.argtypes = [vp, vp, C.c_int]
    L.rdet2d_batch_collect.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    L.rdet2d_batch_get_range_data.argtypes = [vp, C.c_int, vp, vp, C.c_int, ip]


_batch_lib = _lib.Feature(_rdet, "librdet.so", ("rdet2d_batch_create",), [("rdet2d_batch_sizeof_scan", Rdet2dScan)], _declare_batch)


def _declare_range_data(L):
    """``_batch_lib()`` with the argtypes of rdet2d_batch_get_range_data_all set.  It was added without a new ABI version and is
    looked up by name: raises LibraryMissing when the built library has none; every other call keeps working then."""
    L.rdet2d_batch_get_range_data_all.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]


_range_data_lib = _lib.Feature(_batch_lib, "librdet.so", ("rdet2d_batch_get_range_data_all",), (), _declare_range_data)


def _declare_batch3(L):
    """librdet.so with the rdet3d_batch_* argtypes set.  Raises LibraryMissing when it was not built, or was built without them."""
    vp = C.c_void_p
    L.rdet3d_batch_last_hip_error.restype = C.c_char_p
    L.rdet3d_batch_last_hip_error.argtypes = [vp]
    L.rdet3d_batch_max_bright.restype = C.c_int
    L.rdet3d_batch_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.rdet3d_batch_destroy.argtypes = [vp]
    L.rdet3d_batch_destroy.restype = None
    L.rdet3d_batch_set_sensor_to_base_link.argtypes = [vp, C.c_int, vp]
    L.rdet3d_batch_staging.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.rdet3d_batch_submit.argtypes = [vp, vp, C.c_int]
    L.rdet3d_batch_collect.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]


_batch3_lib = _lib.Feature(_rdet, "librdet.so", ("rdet3d_batch_create",), [("rdet3d_batch_sizeof_cloud", Rdet3dCloud)], _declare_batch3)


def _declare_link2(L):
    """``_batch_lib()`` with the argtypes of rdet2d_batch_link set.  It was added without a new ABI version and is looked up by name:
    raises LibraryMissing when the built library has none; every other call keeps working then."""
    L.rdet2d_batch_link.argtypes = [C.c_void_p, C.c_void_p]


def _declare_link3(L):
    """``_batch3_lib()`` with the argtypes of rdet3d_batch_link set; as ``_declare_link2``."""
    L.rdet3d_batch_link.argtypes = [C.c_void_p, C.c_void_p]


_link2_lib = _lib.Feature(_batch_lib, "librdet.so", ("rdet2d_batch_link",), [("rdet_sizeof_link", _lib.Rlink)], _declare_link2)
_link3_lib = _lib.Feature(_batch3_lib, "librdet.so", ("rdet3d_batch_link",), [("rdet_sizeof_link", _lib.Rlink)], _declare_link3)


class DetectLink:
    """One outstanding submit of a detector fleet as the fleet filter takes it (``ReflectorEKFSLAMFleet.submit_linked``): ``raw`` the
    ``struct rlink`` (include/rlink.h), and copies of what the detector's host knows per entry -- ``members``, ``stamps``, ``status``
    (0, or what ``collect`` will report from the host alone, e.g. -3 for a malformed scan) and ``records`` (-1: no workgroup runs for
    the entry, it is empty).  ``raw`` points into the detector's handle: it holds until that detector's next submit."""

    def __init__(self, raw, owner=None):
        self.raw, self._owner = raw, owner
        n = int(raw.count)

        def column(address, tp, dtype):
            return np.array((tp * n).from_address(address), dtype=dtype) if n else np.zeros(0, dtype)

        self.members = column(raw.member, C.c_int, np.int32)
        self.stamps = column(raw.stamp, C.c_double, np.float64)
        self.status = column(raw.host_status, C.c_int, np.int32)
        self.records = column(raw.record, C.c_int, np.int32)

    def __len__(self):
        return int(self.raw.count)


def linked_scan_events(link, pose_fixes=None):
    """The ``ReflectorEKFSLAMFleet.submit_linked`` events of one tick whose scans are still being detected: one
    ``fleet.linked_scan_event`` per entry of ``link`` with host status 0 -- the omission rule of ``scan_events``, as far as the host can
    apply it: what only the launch knows (the kernel's own error, too many centres) empties the scan on the device instead.
    ``pose_fixes``: None, or per ENTRY an (x, y, yaw) or None."""
    if pose_fixes is not None and len(pose_fixes) != len(link):
        raise ValueError("one pose fix (or None) per entry of the link")
    return [fleet.linked_scan_event(int(link.members[i]), float(link.stamps[i]), i, None if pose_fixes is None else pose_fixes[i])
            for i in range(len(link)) if link.status[i] == 0]


def cloud_events(clouds, observations):
    """``scan_events`` for a 3D tick given as ``PointCloudReflectorDetectFleet.submit`` takes it in its first form
    ([(member, stamp, xyzi), ...]): one ``fleet.scan_event`` per cloud with status 0, nothing truncated."""
    clouds, observations = list(clouds), list(observations)
    if len(clouds) != len(observations):
        raise ValueError("one observation per cloud")
    return [fleet.scan_event(c[0], obs.time_, obs.cloud_) for c, (status, obs) in zip(clouds, observations) if status == 0]


def scan_events(scans, observations):
    """The ``ReflectorEKFSLAMFleet.submit`` events of one tick: ``scans`` as given to ``submit`` ([(member, LaserScan), ...]),
    ``observations`` as ``collect`` returned them ([(status, Observation), ...]).  One ``fleet.scan_event`` per scan with status 0;
    nothing is truncated (a scan with more than RFLEET_MAX_OBS centres is the fleet filter's REKF_ERR_TOO_MANY_OBS unless the filter
    fleet has wide scans switched on, ``ReflectorEKFSLAMFleet.wide_scans``, which takes the detector's 256: the caller's call)."""
    scans, observations = list(scans), list(observations)
    if len(scans) != len(observations):
        raise ValueError("one observation per scan")
    return [fleet.scan_event(member, obs.time_, obs.cloud_) for (member, _), (status, obs) in zip(scans, observations) if status == 0]



class _DetectFleet(_lib.Handle):
    """What the two detector fleets share: a handle of the ``_prefix`` calls, made for one ``_Options`` per member, whose submit
    takes the records of ``pack``."""
    _prefix = _Options = _link_lib = None

    def _create(self, L, opts, capacity, device, sensor_to_base_link):
        """The handle for ``opts`` (one ``_Options`` per member); ``sensor_to_base_link``: None, one (x, y, yaw) for all, or [B, 3]."""
        self._L, self._h = L, None
        B = len(opts)
        arr = (self._Options * max(B, 1))(*opts)
        if sensor_to_base_link is None:
            s2b = np.zeros((B, 3))
        else:
            s2b = np.array(sensor_to_base_link, dtype=np.float64)
            s2b = np.ascontiguousarray(np.broadcast_to(s2b, (B, 3))) if s2b.ndim == 1 else np.ascontiguousarray(s2b.reshape(B, 3))
        h = C.c_void_p()
        rc = self._call("create")(C.cast(arr, C.c_void_p), s2b.ctypes.data if B else None, B, int(capacity), int(device), C.byref(h))
        if rc != 0:
            raise RdetError(rc, self._prefix + "_create")
        self._h = h
        self.B = B
        self._s2b = s2b
        self._pending = None          # the submit that has not been collected: (records, arrays they point into, count)
        self._staging = {}

    def _call(self, name):
        return getattr(self._L, f"{self._prefix}_{name}")

    def close(self):
        if self._h:
            self._staging = {}
        super().close()

    def __len__(self):
        return self.B

    def _error(self, rc, where):
        detail = self._call("last_hip_error")(self._h).decode() if rc == -2 else ""
        return RdetError(rc, where + (": " + detail if detail else ""))

    # -- per member ---------------------------------------------------------
    def SetSensorToBaseLinkTransform(self, member: int, xyyaw):
        """Takes the transform already projected with ``detect.project2d`` (x, y, yaw)."""
        v = np.ascontiguousarray(xyyaw, dtype=np.float64).reshape(3)
        self._chk(self._call("set_sensor_to_base_link")(self._h, int(member), v.ctypes.data), "SetSensorToBaseLinkTransform")
        self._s2b[int(member)] = v

    # -- the fleet interface --------------------------------------------------
    def submit_code(self, scans) -> int:
        arr, count, keep = self.pack(scans)
        return self._submitted(self._call("submit")(self._h, C.cast(arr, C.c_void_p), count), (arr, keep, count))

    def submit(self, scans):
        """One scan of any subset of members, at most one per member: ONE kernel launch; returns without waiting for it."""
        self._chk(self.submit_code(scans), self._prefix + "_submit")

    def _collect(self, max_centers, *more):
        """``collect_code`` with the addresses of the class's further per-scan result arrays in ``more``."""
        count = self._pending[2] if self._pending else 0
        n = max(count, 1)
        mc = max(0, min(int(max_centers), MAX_CENTERS))
        status, K, t = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
        cen = np.zeros((n, max(mc, 1), 2), np.float32)
        rc = self._call("collect")(self._h, status.ctypes.data, K.ctypes.data, cen.ctypes.data, mc, t.ctypes.data, *more)
        if self._collected(rc) != 0:
            return rc, []
        return 0, [(int(status[i]), Observation(float(t[i]), cen[i, : int(K[i])].copy())) for i in range(count)]

    def collect(self, max_centers: int = MAX_CENTERS):
        """Waits for the launch: [(status, Observation)] in the order of the submit, status 0 or the entry's own error."""
        rc, out = self.collect_code(max_centers)
        self._chk(rc, self._prefix + "_collect")
        return out

    def detect(self, scans, max_centers: int = MAX_CENTERS):
        self.submit(scans)
        return self.collect(max_centers)

    def link_code(self):
        """-> (rc, ``_lib.Rlink``) of the class's ``_link`` call on the submit that has not been collected."""
        raw = _lib.Rlink()
        return getattr(self._link_lib(), self._prefix + "_link")(self._h, C.addressof(raw)), raw

    def link(self) -> DetectLink:
        """The submit that has not been collected as ``ReflectorEKFSLAMFleet.submit_linked`` takes it: launches nothing, waits for
        nothing.  Valid between ``submit`` and ``collect`` (raises otherwise); ``collect`` afterwards is still how the host gets the
        centres, and behind the filter's own wait it returns at once."""
        rc, raw = self.link_code()
        self._chk(rc, self._prefix + "_link")
        return DetectLink(raw, self)


class LaserReflectorDetectFleet(_DetectFleet):
    """B reflector_detect::LaserReflectorDetect on one MI355X, one kernel launch per ``submit``."""
    _prefix, _destroy, _Options = "rdet2d_batch", "rdet2d_batch_destroy", Rdet2dOptions
    _link_lib = _link2_lib        # (looked up on the first ``link()``: a library without it still serves everything else)

    def __init__(self, options_list, max_beams: int = MAX_BEAMS, device: int = 0, sensor_to_base_link=None):
        L = _batch_lib()
        self.options = list(options_list)
        opts = [Rdet2dOptions(o.intensity_min, o.reflector_min_length, o.reflector_length_error, o.range_min, o.range_max) for o in self.options]
        self._create(L, opts, max_beams, device, sensor_to_base_link)
        self.max_beams = int(max_beams)

    def HandleOdometryData(self, member: int, msg: OdometryData):
        pos = (C.c_double * 2)(float(msg.position[0]), float(msg.position[1]))
        q = (C.c_double * 2)(float(msg.orientation[3]), float(msg.orientation[0]))     # (z, w)
        self._chk(self._L.rdet2d_batch_handle_odometry(self._h, int(member), float(msg.time), C.addressof(pos), C.addressof(q),
                                                       float(msg.linear_velocity[0]), float(msg.linear_velocity[1]),
                                                       float(msg.angular_velocity[2])), "HandleOdometryData")

    def staging(self, member: int):
        """(ranges, intensities): numpy views of the member's slice of the staging area (``max_beams`` float32 each).  A LaserScan
        whose arrays are leading slices of these views is read in place by the kernel, without a copy."""
        member = int(member)
        if member not in self._staging:
            r, i = C.c_void_p(), C.c_void_p()
            self._chk(self._L.rdet2d_batch_staging(self._h, member, C.byref(r), C.byref(i)), "staging")
            tp = C.c_float * self.max_beams
            self._staging[member] = (np.ctypeslib.as_array(tp.from_address(r.value)), np.ctypeslib.as_array(tp.from_address(i.value)))
        return self._staging[member]

    def GetRangeData(self, member: int) -> RangeData:
        n = C.c_int()
        origin = (C.c_float * 2)()
        self._chk(self._L.rdet2d_batch_get_range_data(self._h, int(member), C.addressof(origin), None, 0, C.byref(n)), "GetRangeData")
        ret = np.zeros((max(n.value, 1), 2), np.float32)
        self._chk(self._L.rdet2d_batch_get_range_data(self._h, int(member), C.addressof(origin), ret.ctypes.data, ret.shape[0], C.byref(n)),
                  "GetRangeData")
        return RangeData(np.array(origin[:], dtype=np.float32), ret[: n.value].copy())

    def range_data_code(self, members=None):
        """-> (rc, counts [len(members)], origins [len(members), 2], rows [sum of counts, 2]) of ONE
        rdet2d_batch_get_range_data_all with room for ``max_beams`` rows per listed member (None = all, in order)."""
        L = _range_data_lib()
        if members is None:
            mem, count = None, self.B
        else:
            mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
            count = mem.shape[0]
        cap = count * self.max_beams
        counts = np.zeros(max(count, 1), np.int32)
        origins = np.zeros((max(count, 1), 2), np.float32)
        rows = np.empty((max(cap, 1), 2), np.float32)
        rc = L.rdet2d_batch_get_range_data_all(self._h, None if mem is None else mem.ctypes.data, count, counts.ctypes.data,
                                               origins.ctypes.data, rows.ctypes.data, cap)
        if rc != 0:
            return rc, counts[:0], origins[:0], rows[:0]
        counts = counts[:count]
        return 0, counts, origins[:count], rows[: int(counts.sum())]

    def range_data(self, members=None):
        """``GetRangeData`` of the listed members (None = all, in order): a list of ``RangeData``, the bits ``GetRangeData(member)``
        gives for each.  ONE launch (k_det2d_batch_range_data) and ONE synchronisation whatever the number of members."""
        rc, counts, origins, rows = self.range_data_code(members)
        self._chk(rc, "rdet2d_batch_get_range_data_all")
        out, at = [], 0
        for g, n in enumerate(counts.tolist()):
            out.append(RangeData(origins[g].copy(), rows[at: at + n].copy()))
            at += n
        return out

    @staticmethod
    def pack(scans):
        """scans: iterable of (member, LaserScan).  -> (ctypes array of rdet2d_scan, count, the float32 arrays it points into)."""
        scans = list(scans)
        arr = (Rdet2dScan * max(len(scans), 1))()
        keep = []
        for i, (member, msg) in enumerate(scans):
            ranges, inten = _as_f32(msg.ranges), _as_f32(msg.intensities)
            if ranges.shape != inten.shape or ranges.ndim != 1:
                raise ValueError("ranges and intensities are one-dimensional and of one length")
            keep.append((ranges, inten))
            s = arr[i]
            s.member, s.stamp = int(member), float(msg.stamp)
            s.angle_min, s.angle_max, s.angle_increment = float(msg.angle_min), float(msg.angle_max), float(msg.angle_increment)
            s.scan_time, s.range_min, s.range_max = float(msg.scan_time), float(msg.range_min), float(msg.range_max)
            s.N = ranges.shape[0]
            s.ranges = ranges.ctypes.data if s.N else None
            s.intensities = inten.ctypes.data if s.N else None
        return arr, len(scans), keep

    def collect_code(self, max_centers: int = MAX_CENTERS):
        """-> (rc, [(status, Observation)]) of the submit that has not been collected."""
        return self._collect(max_centers)

    def collect(self, max_centers: int = MAX_CENTERS):
        """Waits for the launch: [(status, Observation)] in the order of the submitted scans.  status 0, or the scan's own error
        (-3: a malformed message, K = 0; -5: more centres than ``max_centers``; -4: more than 256 reflectors)."""
        return super().collect(max_centers)


class PointCloudReflectorDetectFleet(_DetectFleet):
    """B reflector_detect::PointCloudReflectorDetect on one MI355X, one kernel launch per ``submit``."""
    _prefix, _destroy, _Options = "rdet3d_batch", "rdet3d_batch_destroy", Rdet3dOptions
    _link_lib = _link3_lib

    def __init__(self, options_list, max_points: int = 65536, device: int = 0, sensor_to_base_link=None):
        L = _batch3_lib()
        self.options_list = list(options_list)
        self._create(L, [Rdet3dOptions(o.intensity_min) for o in self.options_list], max_points, device, sensor_to_base_link)
        self.max_points = int(max_points)
        self.sensor_to_base_link = self._s2b          # (the public name of this class; one array)
        self.last_n_bright = []       # the survivors of the intensity gate, per cloud of the last collect

    @staticmethod
    def max_bright() -> int:
        """Survivors of the intensity gate a cloud may have (more: status -4, and the cloud goes through a PointCloudReflectorDetect)."""
        return int(_batch3_lib().rdet3d_batch_max_bright())

    def staging(self, member: int):
        """A (max_points, 4) float32 numpy view of the member's slice of the staging area.  A cloud that is a leading slice of this
        view is read in place by the kernel, without a copy."""
        member = int(member)
        if member not in self._staging:
            p = C.c_void_p()
            self._chk(self._L.rdet3d_batch_staging(self._h, member, C.byref(p)), "staging")
            tp = C.c_float * (4 * self.max_points)
            self._staging[member] = np.ctypeslib.as_array(tp.from_address(p.value)).reshape(self.max_points, 4)
        return self._staging[member]

    @staticmethod
    def pack(clouds):
        """clouds: iterable of (member, stamp, xyzi) or (member, PointCloud).  -> (ctypes array of rdet3d_cloud, count, the float32
        arrays it points into)."""
        clouds = list(clouds)
        arr = (Rdet3dCloud * max(len(clouds), 1))()
        keep = []
        for i, item in enumerate(clouds):
            member, stamp, xyzi = (item[0], item[1].stamp, item[1].xyzi) if len(item) == 2 else item
            pts = _as_f32(xyzi)
            if pts.size & 3:
                raise ValueError("points are (x, y, z, intensity) quadruples")
            keep.append(pts)
            c = arr[i]
            c.member, c.stamp, c.N = int(member), float(stamp), pts.size >> 2
            c.xyzi = pts.ctypes.data if c.N else None
        return arr, len(clouds), keep

    # (the 2D names with ``clouds`` for ``scans``: the keyword is this class's)
    def submit_code(self, clouds) -> int:
        return super().submit_code(clouds)

    def submit(self, clouds):
        """One cloud of any subset of members, at most one per member: ONE kernel launch; returns without waiting for it."""
        super().submit(clouds)

    def detect(self, clouds, max_centers: int = MAX_CENTERS):
        return super().detect(clouds, max_centers)

    def collect_code(self, max_centers: int = MAX_CENTERS):
        """-> (rc, [(status, Observation)]) of the submit that has not been collected."""
        nb = np.zeros(max(self._pending[2] if self._pending else 0, 1), np.int32)
        rc, out = self._collect(max_centers, nb.ctypes.data)
        if rc == 0:
            self.last_n_bright = [int(v) for v in nb[:len(out)]]
        return rc, out

    def collect(self, max_centers: int = MAX_CENTERS):
        """Waits for the launch: [(status, Observation)] in the order of the submitted clouds.  status 0, or the cloud's own error
        (-4: more than ``max_bright()`` survivors of the intensity gate -- ``last_n_bright`` holds the count -- or more than 256
        reflectors; -5: more centres than ``max_centers``)."""
        return super().collect(max_centers)
