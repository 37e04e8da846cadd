"""ctypes loader for the C-ABI libraries built from csrc/ (include/rekf.h, include/rdet.h).

There is deliberately NO fallback: if the HIP extension is missing or does not
load, importing the product path raises.  Build with ``python __graft_entry__.py``
(or ``make -C reflector_ekf_slam_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
MAX_OBS = 256
REKF_ABI_VERSION = 7          # must equal REKF_ABI_VERSION of include/rekf.h and rekf_abi_version() of the built library


class RekfOptions(C.Structure):
    """struct rekf_options (include/rekf.h) == ekf::EKFOptions (ekf_slam_interface.h:28-41)."""
    _fields_ = [("odom_model", C.c_int), ("use_imu", C.c_int), ("init_time", C.c_double),
                ("init_pose", C.c_double * 3), ("linear_velocity_cov", C.c_double),
                ("angular_velocity_cov", C.c_double), ("observation_cov", C.c_double)]


class Rlink(C.Structure):
    """struct rlink (include/rlink.h): one outstanding submit of a fleet detector as librfleet.so reads it.  Neither library's
    binding owns it."""
    _fields_ = [("count", C.c_int), ("device", C.c_int), ("member", C.c_void_p), ("stamp", C.c_void_p), ("host_status", C.c_void_p),
                ("record", C.c_void_p), ("records", C.c_void_p), ("record_bytes", C.c_long), ("k_off", C.c_int), ("err_off", C.c_int),
                ("centers_off", C.c_int), ("max_centers", C.c_int), ("ready", C.c_void_p), ("consumed", C.c_void_p)]


class LibraryMissing(RuntimeError):
    pass


def lib_path(name: str) -> str:
    return os.path.join(_HERE, name)


_REBUILD = "rebuild it (python __graft_entry__.py); there is no CPU fallback"


class _Loader:
    """A library with its argtypes set, made on the first call and kept in ``ready``; a call that raises leaves ``ready`` None."""
    ready = None

    def __call__(self):
        if self.ready is None:
            self.ready = self._load()
        return self.ready

    def _checked(self, L, name):
        """L after the by-name and structure-size checks and ``declare``."""
        missing = [n for n in (*self.names, *(call for call, _ in self.sizes)) if not hasattr(L, n)]
        if missing:
            raise LibraryMissing(f"{name} has no {', '.join(missing)}: {_REBUILD}")
        for call, struct in self.sizes:
            have = getattr(L, call)()
            if have != C.sizeof(struct):
                raise LibraryMissing(f"{name}: {call}() is {have} bytes, this package packs {struct.__name__} in {C.sizeof(struct)}: {_REBUILD}")
        self.declare(L)
        return L


class Library(_Loader):
    """Root loader of ``file_name``: the file exists, loads, answers ``abi = (call, version)`` when one is given, and agrees on every
    ``(sizeof call, ctypes.Structure)`` of ``sizes``; then ``declare(L)`` sets the argtypes."""

    def __init__(self, file_name, abi, declare, sizes=()):
        self.file_name, self.abi, self.declare, self.names, self.sizes = file_name, abi, declare, (), sizes
        self.__doc__ = declare.__doc__

    def _load(self):
        path = lib_path(self.file_name)
        if not os.path.exists(path):
            raise LibraryMissing(f"{path} not found, the HIP extension is not built: {_REBUILD}")
        L = C.CDLL(path)
        if self.abi is not None:
            have = getattr(L, self.abi[0])()
            if have != self.abi[1]:
                raise LibraryMissing(f"{path} has ABI version {have}, this package speaks {self.abi[1]}: {_REBUILD}")
        return self._checked(L, path)


class Feature(_Loader):
    """Calls that were added to a library without a new ABI version and are looked up by name: ``base()`` (a Library or a Feature)
    must have every one of ``names`` and agree on every ``(sizeof call, ctypes.Structure)`` of ``sizes``; then ``declare(L)`` sets
    their argtypes.  A library without them is reported on their first use only; every other call keeps working."""

    def __init__(self, base, library_name, names, sizes, declare):
        self.base, self.library_name, self.names, self.sizes, self.declare = base, library_name, names, sizes, declare
        self.__doc__ = declare.__doc__

    def _load(self):
        return self._checked(self.base(), self.library_name)


class Handle:
    """Owner of one C handle: ``_L`` the library, ``_h`` the handle, ``_destroy`` the name of the call that frees it.  A class
    says in ``_error`` which exception ``_chk`` raises for a code; one with submit/collect pairs keeps the submit that has not been
    collected in ``_pending``."""
    _L = _h = _destroy = _pending = None

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _error(self, rc, where):
        return RuntimeError(f"{where}: error {rc}")

    def _chk(self, rc, where):
        if rc != 0:
            raise self._error(rc, where)

    def _submitted(self, rc, pending):
        """The tail of a submit: one that returned 0 is the pending one."""
        if rc == 0:
            self._pending = pending
        return rc

    def _collected(self, rc):
        """The head of a collect: one that returned 0 has taken the pending submit."""
        if rc == 0:
            self._pending = None
        return rc


def _declare_rekf(L):
    """librekf.so with argtypes set.  Raises LibraryMissing when it was not built or speaks another ABI version."""
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.rekf_strerror.restype = C.c_char_p
    L.rekf_strerror.argtypes = [C.c_int]
    L.rekf_last_hip_error.restype = C.c_char_p
    L.rekf_last_hip_error.argtypes = [vp]
    L.rekf_create.argtypes = [C.POINTER(RekfOptions), C.c_int, C.c_int, C.POINTER(vp)]
    L.rekf_destroy.argtypes = [vp]
    L.rekf_destroy.restype = None
    L.rekf_set_map.argtypes = [vp, vp, vp, C.c_int]
    L.rekf_handle_odometry.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double]
    L.rekf_handle_observation.argtypes = [vp, C.c_double, vp, C.c_int, vp]
    L.rekf_predict_state.argtypes = [vp, C.c_double, dp, dp]
    L.rekf_predict_state_full.argtypes = [vp, C.c_double, dp, ip, vp, C.c_long, vp, C.c_long]
    L.rekf_get_flags.argtypes = [vp, ip]
    L.rekf_get_time.argtypes = [vp, dp]
    L.rekf_get_pose.argtypes = [vp, vp, vp, vp]          # (double *: plain addresses of a preallocated buffer, ekf_slam.py -- the per-call path)
    L.rekf_get_n.argtypes = [vp, ip]
    L.rekf_get_marker_ellipses.argtypes = [vp, vp, C.c_int, ip]
    L.rekf_get_state.argtypes = [vp, dp, ip, vp, C.c_long, vp, C.c_long]
    L.rekf_set_state.argtypes = [vp, C.c_double, C.c_int, vp, vp, vp]
    L.rekf_get_last_match.argtypes = [vp, ip, vp, ip, vp, ip, vp]
    L.rekf_sync.argtypes = [vp]
    L.rekf_profile_enable.argtypes = [vp, C.c_int]
    L.rekf_profile_read.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_long)]
    L.rekf_profile_reset.argtypes = [vp]
    L.rekf_profile_samples.argtypes = [vp, vp, C.c_long, C.POINTER(C.c_long)]
    L.rekf_stream.restype = vp
    L.rekf_stream.argtypes = [vp]
    L.rekf_device_layout.argtypes = [vp, ip, ip, C.POINTER(vp), C.POINTER(vp)]
    L.rekf_reserve.argtypes = [vp, C.c_int]
    L.rekf_set_auto_grow.argtypes = [vp, C.c_int]
    L.rekf_set_exclusive.argtypes = [vp, C.c_int]
    L.rekf_get_capacity.argtypes = [vp, ip]
    L.rekf_debug_time_kernel.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    if hasattr(L, "rekf_debug_inject_failure"):           # (absent from older builds that scripts/gpu_ab.py compares against)
        L.rekf_debug_inject_failure.argtypes = [vp, C.c_int]
    if hasattr(L, "rekf_debug_set_grid"):
        L.rekf_debug_set_grid.argtypes = [vp, C.c_int, C.c_double, C.c_int]


rekf = Library("librekf.so", ("rekf_abi_version", REKF_ABI_VERSION), _declare_rekf)
