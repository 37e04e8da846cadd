"""Fleet scan matcher: scan_matching::RealTimeCorrelativeScanMatcher2D::Match for one scan of many robots, ONE kernel launch per
call (rgrid_batch_* of include/rgrid.h), against resident probability grids that any number of the scans may share.

``ScanMatchFleet(max_scans)`` holds ``num_grids`` grid slots (``SetGrid``).  ``submit(scans)`` takes ``(grid_slot, initial_pose,
points_xy)`` per scan and enqueues one launch of kgb_match (one workgroup per scan and rotated scan); ``collect()`` waits and
returns one ``FleetMatchResult`` per scan, in the order given: the ``grid.MatchResult`` that ``GridFrontEnd.Match`` returns for
that scan, bit for bit, plus a ``status``.  ``pose_fixes`` turns a tick's results into the ``pose_fix`` arguments of
``fleet.scan_event``: the reference's USE_GPS deployment is ``fleet.predict_poses(times)`` -> ``matcher.match(...)`` ->
``fleet.scan_event(member, t, cloud, pose_fix=...)`` -> ``fleet.submit``.

The second step of the reference's ``MapBuilder::ScanMatch`` (map_builder.cc:34-55), ``CeresScanMatcher2D::Match``, is here for a
batch too: ``refine(scans)`` takes ``(grid_slot, target_translation, initial_pose, points_xy)`` per scan and runs ONE launch of
kgb_refine (one workgroup per scan), each result the bits of ``GridFrontEnd.RefineMatch``; ``scan_match(scans)`` takes what
``match`` takes and chains both steps on the handle's stream without a host wait between them, returning per scan a
``FleetScanMatchResult`` with ``.coarse`` (the match) and ``.fine`` (the refinement).  ``pose_fixes`` of those yields the refined
poses: the fix the reference's node fuses.  A handle has one pending submit at a time, of any kind.

The step after it, ``MapBuilder::InsertIntoSubmap`` (map_builder.cc:110-120), is ``insert(scans)``: ``(grid_slot, origin_xy,
returns_xy, misses_xy_or_None)`` per scan, each into its OWN slot (a call names a slot once), ONE launch of kgb_insert (one
workgroup per scan): the slot then holds the cells and limits ``GridFrontEnd.Insert`` (GrowAsNeeded + Insert) leaves, bit for bit,
and the map never leaves the device between ticks.  ``GetGrid(slot)`` / ``GetLimits(slot)`` read a slot back.

The stage in front of all that, the filters of ``MapBuilder::AddRangeData`` (map_builder.cc:30-31,73), is ``filter(scans)``:
``(returns_xy, misses_xy_or_None)`` per scan, already gravity-aligned (``gravity_aligned_scans`` turns raw range data and EKF poses
into such scans), ONE launch of kgb_filter (one workgroup per scan) and one wait: per scan a ``FleetFilterResult`` with the two
voxel-filtered clouds and the adaptively filtered returns, the bits of ``GridFrontEnd.VoxelFilter`` (twice) and
``GridFrontEnd.AdaptiveVoxelFilter``.  It needs no grid.

The way out of the mapper, ``MapBuilder::ToSubmapTexture`` (map_builder.cc:128-134), is ``draw_textures(slots)``: ONE launch of
kgb_texture (one workgroup per named slot) and one wait turn resident slots into what the reference publishes -- per slot a
``FleetTexture`` with the ``(cells, box, slice_max)`` that ``GridFrontEnd.DrawTexture`` returns for the same grid, byte for byte;
``submap_textures(slots, submap_origins)`` gives the reference's ``SubmapTexture`` fields as ``MapBuilder.ToSubmapTexture`` does.
The slots are only read and stay on the device.

What a node publishes and saves is one step further, ``Node::PublishMap`` / ``Node::HandleSaveMap`` (src/ros_node.cc:845-863,947-1001):
``occupancy_grids(slots, submap_origins, mode)`` is ONE launch of kgb_occupancy (one workgroup per named slot) and one wait -- per slot
a ``FleetOccupancyGrid`` with the ``grid.OccupancyGrid`` that ``GridFrontEnd.OccupancyGrid`` returns for the same grid, byte for byte,
plus a ``status``: the reference's cairo painting of the texture as nav_msgs::OccupancyGrid data (mode OCCUPANCY) or as the bytes of
the saved PGM (mode IMAGE).

The reference's entry point itself, ``MapBuilder::AddRangeData`` (map_builder.cc:57-108), for one scan of every robot is
``add_range_data(range_datas, ekf_poses, slots)``: ONE C call (rgrid_batch_add_range_data) runs the five stages above -- the gravity
alignment of the raw clouds on the device inside the filter's launch, the match and the refinement for the robots that have a
submap, the insert (a robot's first scan creates its 100 x 100 submap), and ``range_data_in_local.returns`` from the raw returns that
are still on the device -- with at most five launches and three waits whatever the number of robots (``last_call_counts``).  Per
robot it gives what ``GridFrontEnd.AddRangeData`` gives for the same scans, bit for bit.  ``map_builder.FleetMapBuilder`` is the
reference's interface over it.

All arithmetic happens in the HIP kernel behind librgrid.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from .grid import (IMAGE, OCCUPANCY, AdaptiveVoxelFilterOptions, CeresScanMatcherOptions2D, MatchResult, OccupancyGrid, RangeDataInserterOptions, RealTimeCorrelativeScanMatcherOptions, RefineResult,
                   RgridError, _lib_rgrid, _MapBuilderOptionsC, _MatchOptions, _RefineOptions, _RefineSummary)

RGRID_OK, RGRID_ERR_INVALID, RGRID_ERR_CAPACITY, RGRID_ERR_EMPTY = 0, -1, -4, -6
RGRID_ERR_BUFFER = -5
REDUCE_ARRIVAL, REDUCE_LAUNCH = 0, 1        # rgrid_batch_set_reduction
SCAN_INSERTED, SCAN_DROPPED_EMPTY, SCAN_FILTERED_EMPTY = 0, 1, 2    # status of a scan of add_range_data (RGRID_SCAN_*)


class RgridBatchScan(C.Structure):
    """struct rgrid_batch_scan (include/rgrid.h)."""
    _fields_ = [("grid", C.c_int), ("n", C.c_int), ("points_xy", C.c_void_p), ("initial_pose", C.c_double * 3)]


class RgridBatchRefineScan(C.Structure):
    """struct rgrid_batch_refine_scan (include/rgrid.h)."""
    _fields_ = [("grid", C.c_int), ("n", C.c_int), ("points_xy", C.c_void_p), ("target_translation", C.c_double * 2),
                ("initial_pose", C.c_double * 3)]


class RgridBatchInsertScan(C.Structure):
    """struct rgrid_batch_insert_scan (include/rgrid.h)."""
    _fields_ = [("grid", C.c_int), ("n_returns", C.c_int), ("n_misses", C.c_int), ("returns_xy", C.c_void_p), ("misses_xy", C.c_void_p),
                ("origin_xy", C.c_float * 2)]


class _InsertOptions(C.Structure):
    """struct rgrid_insert_options (include/rgrid.h)."""
    _fields_ = [("hit_probability", C.c_float), ("miss_probability", C.c_float), ("insert_free_space", C.c_int)]


class RgridBatchFilterScan(C.Structure):
    """struct rgrid_batch_filter_scan (include/rgrid.h)."""
    _fields_ = [("n_returns", C.c_int), ("n_misses", C.c_int), ("returns_xy", C.c_void_p), ("misses_xy", C.c_void_p)]


class RgridBatchRangeData(C.Structure):
    """struct rgrid_batch_range_data (include/rgrid.h)."""
    _fields_ = [("grid", C.c_int), ("n_returns", C.c_int), ("n_misses", C.c_int), ("returns_xy", C.c_void_p), ("misses_xy", C.c_void_p),
                ("origin_xy", C.c_float * 2), ("ekf_pose", C.c_double * 3)]


@dataclass
class FleetRangeDataResult:
    """What rgrid_batch_add_range_data returns for one scan: ``code`` RGRID_OK or the scan's own error, ``status`` SCAN_INSERTED /
    SCAN_DROPPED_EMPTY / SCAN_FILTERED_EMPTY, ``local_pose`` (x, y, yaw), ``origin_in_local`` the origin of range_data_in_local2 (the
    submap's origin when the scan created its slot), ``returns_in_local`` (n_returns, 2) float32, zero unless inserted."""
    code: int
    status: int
    local_pose: np.ndarray
    origin_in_local: tuple
    returns_in_local: np.ndarray


class _FilterOptions(C.Structure):
    """struct rgrid_filter_options (include/rgrid.h)."""
    _fields_ = [("voxel_filter_size", C.c_float), ("adaptive_max_length", C.c_double), ("adaptive_min_num_points", C.c_double),
                ("adaptive_max_range", C.c_double)]


@dataclass
class FleetFilterResult:
    """The filter stage of MapBuilder::AddRangeData for one scan: ``returns`` = VoxelFilter(size).Filter(returns), ``misses`` =
    VoxelFilter(size).Filter(misses), ``filtered`` = AdaptiveVoxelFilter(options).Filter(``returns``); (k, 2) float32 each."""
    status: int                      # RGRID_OK, -4 more points than the handle or one workgroup holds, -1 a non-finite coordinate (clouds empty then)
    returns: np.ndarray
    misses: np.ndarray
    filtered: np.ndarray


@dataclass
class FleetTexture:
    """ProbabilityGrid::DrawToSubmapTexture of one slot, the three things ``GridFrontEnd.DrawTexture`` returns (and unpacks like
    them): ``cells`` uint8 (height, width, 2) = (value, alpha) per cell of the known-cells box, ``box`` = (offset_x, offset_y,
    width, height), ``slice_max`` = (x, y)."""
    cells: np.ndarray
    box: tuple
    slice_max: tuple

    def __iter__(self):
        return iter((self.cells, self.box, self.slice_max))


@dataclass
class FleetOccupancyGrid(OccupancyGrid):
    status: int = 0                  # RGRID_OK, or -4: the slot lies outside the painting's domain (data is empty, origin zero then)


@dataclass
class FleetMatchResult(MatchResult):
    status: int = 0                  # RGRID_OK, or the scan's own error: -6 empty cloud, -4 more points / rotated scans than the handle holds


@dataclass
class FleetRefineResult(RefineResult):
    status: int = 0                  # RGRID_OK, -6 empty cloud, -4 more points than the handle holds (all other fields zero then)


@dataclass
class FleetScanMatchResult:
    """MapBuilder::ScanMatch for one scan: the correlative match and the refinement started from it."""
    coarse: FleetMatchResult
    fine: FleetRefineResult

    @property
    def pose_estimate(self):
        return self.fine.pose_estimate

    @property
    def status(self):
        return self.coarse.status


def _declare_batch(L):
    """librgrid.so with the rgrid_batch_* argtypes set.  Raises LibraryMissing when it was not built, or was built without them."""
    vp = C.c_void_p
    L.rgrid_batch_last_hip_error.restype = C.c_char_p
    L.rgrid_batch_last_hip_error.argtypes = [vp]
    L.rgrid_batch_last_prepare_seconds.restype = C.c_double
    L.rgrid_batch_last_prepare_seconds.argtypes = [vp]
    L.rgrid_batch_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(vp)]
    L.rgrid_batch_destroy.argtypes = [vp]
    L.rgrid_batch_destroy.restype = None
    L.rgrid_batch_set_grid.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    L.rgrid_batch_set_reduction.argtypes = [vp, C.c_int]
    L.rgrid_batch_match_submit.argtypes = [vp, C.POINTER(_MatchOptions), vp, C.c_int]
    L.rgrid_batch_match_collect.argtypes = [vp, vp, vp, vp, vp, vp]


_batch_lib = _lib.Feature(_lib_rgrid, "librgrid.so", ("rgrid_batch_create",), [("rgrid_batch_sizeof_scan", RgridBatchScan)], _declare_batch)


def _declare_refine(L):
    """``_batch_lib()`` with the argtypes of the refine and match-plus-refine calls set.  Raises LibraryMissing when the built library
    has no such calls (the ABI version does not tell: they are looked up by name); the match calls keep working then."""
    vp = C.c_void_p
    L.rgrid_batch_refine_submit.argtypes = [vp, C.POINTER(_RefineOptions), vp, C.c_int]
    L.rgrid_batch_refine_collect.argtypes = [vp, vp, vp, vp]
    L.rgrid_batch_scan_match_submit.argtypes = [vp, C.POINTER(_MatchOptions), C.POINTER(_RefineOptions), vp, C.c_int]
    L.rgrid_batch_scan_match_collect.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]


_refine_lib = _lib.Feature(_batch_lib, "librgrid.so",
                           ("rgrid_batch_refine_submit", "rgrid_batch_refine_collect", "rgrid_batch_scan_match_submit", "rgrid_batch_scan_match_collect"),
                           [("rgrid_batch_sizeof_refine_scan", RgridBatchRefineScan)], _declare_refine)


def _declare_insert(L):
    """``_batch_lib()`` with the argtypes of the insert calls and the slot read-backs set.  Raises LibraryMissing when the built
    library has no such calls or packs another structure (they are looked up by name); every other call keeps working then."""
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.rgrid_batch_insert_submit.argtypes = [vp, C.POINTER(_InsertOptions), vp, C.c_int]
    L.rgrid_batch_insert_collect.argtypes = [vp, vp]
    L.rgrid_batch_get_limits.argtypes = [vp, C.c_int, ip, ip, dp, dp, dp]
    L.rgrid_batch_get_grid.argtypes = [vp, C.c_int, vp, C.c_long]


_insert_lib = _lib.Feature(_batch_lib, "librgrid.so",
                           ("rgrid_batch_insert_submit", "rgrid_batch_insert_collect", "rgrid_batch_get_limits", "rgrid_batch_get_grid"),
                           [("rgrid_batch_sizeof_insert_scan", RgridBatchInsertScan)], _declare_insert)


def _declare_filter(L):
    """``_batch_lib()`` with the argtypes of the filter calls set.  Raises LibraryMissing when the built library has no such calls or
    packs another structure (they are looked up by name); every other call keeps working then."""
    vp = C.c_void_p
    L.rgrid_batch_filter_max_points.restype = C.c_int
    L.rgrid_batch_filter_max_points.argtypes = []
    L.rgrid_batch_filter_submit.argtypes = [vp, C.POINTER(_FilterOptions), vp, C.c_int]
    L.rgrid_batch_filter_collect.argtypes = [vp, vp, vp, vp, C.c_long]


_filter_lib = _lib.Feature(_batch_lib, "librgrid.so", ("rgrid_batch_filter_submit", "rgrid_batch_filter_collect", "rgrid_batch_filter_max_points"),
                           [("rgrid_batch_sizeof_filter_scan", RgridBatchFilterScan)], _declare_filter)


def _declare_texture(L):
    """``_batch_lib()`` with the argtypes of the texture calls set.  Raises LibraryMissing when the built library has no such calls
    (they are looked up by name); every other call keeps working then."""
    vp = C.c_void_p
    L.rgrid_batch_texture_submit.argtypes = [vp, vp, C.c_int]
    L.rgrid_batch_texture_collect.argtypes = [vp, vp, vp, vp, vp, C.c_long]


_texture_lib = _lib.Feature(_batch_lib, "librgrid.so", ("rgrid_batch_texture_submit", "rgrid_batch_texture_collect"), (), _declare_texture)


def _declare_occupancy(L):
    """``_batch_lib()`` with the argtypes of the occupancy calls set.  Raises LibraryMissing when the built library has no such calls
    (they are looked up by name); every other call keeps working then."""
    vp = C.c_void_p
    L.rgrid_batch_occupancy_submit.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    L.rgrid_batch_occupancy_collect.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_long]


_occupancy_lib = _lib.Feature(_batch_lib, "librgrid.so", ("rgrid_batch_occupancy_submit", "rgrid_batch_occupancy_collect"), (), _declare_occupancy)


def _declare_range_data(L):
    """``_batch_lib()`` with the argtypes of rgrid_batch_add_range_data and rgrid_batch_last_call_counts set.  Raises LibraryMissing
    when the built library has no such calls or packs another structure (they are looked up by name); every other call keeps working
    then."""
    vp = C.c_void_p
    L.rgrid_batch_add_range_data.argtypes = [vp, C.POINTER(_MapBuilderOptionsC), vp, C.c_int, vp, vp, vp, vp, vp, C.c_long]
    L.rgrid_batch_last_call_counts.argtypes = [vp, vp]


_range_data_lib = _lib.Feature(_batch_lib, "librgrid.so", ("rgrid_batch_add_range_data", "rgrid_batch_last_call_counts"),
                               [("rgrid_batch_sizeof_range_data", RgridBatchRangeData)], _declare_range_data)


def _map_builder_options(o):
    """struct rgrid_map_builder_options of a ``map_builder.MapBuilderOptions`` (None: the defaults), as GridFrontEnd.AddRangeData packs it."""
    if o is None:
        from .map_builder import MapBuilderOptions
        o = MapBuilderOptions()
    m, r = o.real_time_scan_matcher_options, o.ceres_scan_matcher_options
    a, ins = o.adaptive_voxel_options, o.range_data_inserter_options
    return _MapBuilderOptionsC(o.resolution, o.voxel_filter_size, a.max_length, a.min_num_points, a.max_range, _match_options(m), _refine_options(r),
                               ins.hit_probability, ins.miss_probability, 1 if ins.insert_free_space else 0)


def filter_max_points() -> int:
    """Points per cloud one workgroup of kgb_filter holds (rgrid_batch_filter_max_points)."""
    return int(_filter_lib().rgrid_batch_filter_max_points())


def _filter_options(voxel_filter_size, o):
    o = o or AdaptiveVoxelFilterOptions()
    return _FilterOptions(float(voxel_filter_size), float(o.max_length), float(o.min_num_points), float(o.max_range))


def gravity_aligned_scans(range_datas, ekf_poses):
    """``(returns, misses)`` of every ``map_builder.RangeData`` rotated into the gravity-aligned frame of its EKF pose ``(x, y, yaw)``,
    as MapBuilder::AddRangeData does before it filters (map_builder.cc:20-28, with map_builder.py's own arithmetic): the scans
    ``ScanMatchFleet.filter`` takes.  The kernel does not rotate."""
    from .map_builder import rigid2f_apply, yaw_of_quaternion_f32
    scans = []
    for rd, pose in zip(range_datas, ekf_poses):
        theta = float(pose[2])
        yaw = yaw_of_quaternion_f32(math.cos(theta / 2), math.sin(theta / 2))
        misses = np.zeros((0, 2), np.float32) if rd.misses is None else rd.misses
        scans.append((rigid2f_apply((0.0, 0.0), yaw, rd.returns), rigid2f_apply((0.0, 0.0), yaw, misses)))
    return scans


def _insert_options(o):
    o = o or RangeDataInserterOptions()
    return _InsertOptions(float(o.hit_probability), float(o.miss_probability), 1 if o.insert_free_space else 0)


def _refine_options(o):
    o = o or CeresScanMatcherOptions2D()
    return _RefineOptions(o.occupied_space_weight, o.translation_weight, o.rotation_weight, int(o.max_num_iterations),
                          1 if o.use_nonmonotonic_steps else 0)


def _match_options(o):
    o = o or RealTimeCorrelativeScanMatcherOptions()
    return _MatchOptions(o.linear_search_window, o.angular_search_window, o.translation_delta_cost_weight, o.rotation_delta_cost_weight)


def _refine_results(count, status, pose, summ):
    return [FleetRefineResult(pose[i].copy(), float(summ[i].initial_cost), float(summ[i].final_cost), int(summ[i].iterations),
                              int(summ[i].termination), int(status[i])) for i in range(count)]


def pose_fixes(results):
    """Per scan ``(x, y, yaw)`` of the matched pose -- the refined one for ``scan_match``'s results -- or None when its status is
    not OK: the ``pose_fix`` of ``fleet.scan_event``."""
    return [tuple(float(v) for v in r.pose_estimate) if r.status == RGRID_OK else None for r in results]


class ScanMatchFleet(_lib.Handle):
    """One batch handle of include/rgrid.h: the real-time correlative scan matcher for up to ``max_scans`` scans per launch."""
    _destroy = "rgrid_batch_destroy"

    def __init__(self, max_scans: int, max_points: int = 8192, num_grids: int = 1, max_cells: int = 1024 * 1024,
                 max_rotations: int = 256, device: int = 0):
        self._L = _batch_lib()
        self._h = None
        h = C.c_void_p()
        rc = self._L.rgrid_batch_create(int(max_scans), int(max_points), int(num_grids), int(max_cells), int(max_rotations),
                                        int(device), C.byref(h))
        if rc != 0:
            raise RgridError(rc, "rgrid_batch_create")
        self._h = h
        self.max_scans, self.max_points, self.num_grids = int(max_scans), int(max_points), int(num_grids)
        self._pending = None          # the submit that has not been collected: its scan count
        self._set_slots = set()       # the slots SetGrid has filled: what draw_textures draws by default

    def _error(self, rc, where):
        return RgridError(rc, where, self._L.rgrid_batch_last_hip_error(self._h).decode() if rc == -2 else
                          self._L.rgrid_strerror(rc).decode())

    # -- grids ----------------------------------------------------------------
    def SetGrid_code(self, slot: int, cells, resolution: float, max_xy) -> int:
        g = np.ascontiguousarray(cells, dtype=np.uint16)
        if g.ndim != 2:
            raise ValueError("cells is a (num_y_cells, num_x_cells) array")
        rc = self._L.rgrid_batch_set_grid(self._h, int(slot), g.ctypes.data, g.shape[1], g.shape[0], float(resolution),
                                          float(max_xy[0]), float(max_xy[1]))
        if rc == 0:
            self._set_slots.add(int(slot))
        return rc

    def SetGrid(self, slot: int, cells, resolution: float, max_xy):
        """``GridFrontEnd.SetGrid`` for grid slot ``slot``: uint16 (num_y_cells, num_x_cells) correspondence-cost values,
        MapLimits resolution and max corner.  Not between a submit and its collect."""
        self._chk(self.SetGrid_code(slot, cells, resolution, max_xy), "rgrid_batch_set_grid")

    def set_reduction(self, mode: int):
        """REDUCE_ARRIVAL (default): the arg-max over a scan's rotated scans inside the one launch; REDUCE_LAUNCH: in a second one."""
        self._chk(self._L.rgrid_batch_set_reduction(self._h, int(mode)), "rgrid_batch_set_reduction")

    # -- the fleet interface --------------------------------------------------
    @staticmethod
    def pack(scans):
        """scans: iterable of (grid_slot, initial_pose, points_xy).  -> (ctypes array of rgrid_batch_scan, count, the arrays it points into)."""
        scans = list(scans)
        arr = (RgridBatchScan * max(len(scans), 1))()
        keep = []
        for i, (slot, pose, points) in enumerate(scans):
            pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
            keep.append(pts)
            s = arr[i]
            s.grid, s.n = int(slot), pts.shape[0]
            s.points_xy = pts.ctypes.data if s.n else None
            s.initial_pose[0], s.initial_pose[1], s.initial_pose[2] = float(pose[0]), float(pose[1]), float(pose[2])
        return arr, len(scans), keep

    def submit_packed_code(self, packed, options: RealTimeCorrelativeScanMatcherOptions | None = None) -> int:
        """``submit_code`` for what ``pack`` returned (reusable: the points are copied by the call)."""
        co = _match_options(options)
        return self._submitted(self._L.rgrid_batch_match_submit(self._h, C.byref(co), C.cast(packed[0], C.c_void_p), packed[1]), packed[1])

    def submit_code(self, scans, options: RealTimeCorrelativeScanMatcherOptions | None = None) -> int:
        return self.submit_packed_code(self.pack(scans), options)

    def submit(self, scans, options: RealTimeCorrelativeScanMatcherOptions | None = None):
        """One scan per entry, any grid slot each, the same options for all: ONE kernel launch; returns without waiting for it."""
        self._chk(self.submit_code(scans, options), "rgrid_batch_match_submit")

    def collect_code(self):
        """-> (rc, [FleetMatchResult]) of the submit that has not been collected."""
        count = self._pending or 0
        n = max(count, 1)
        status, pose, score = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros(n)
        best, info = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.int32)
        rc = self._collected(self._L.rgrid_batch_match_collect(self._h, status.ctypes.data, pose.ctypes.data, score.ctypes.data,
                                                               best.ctypes.data, info.ctypes.data))
        if rc != 0:
            return rc, []
        return 0, [FleetMatchResult(float(score[i]), pose[i].copy(), tuple(int(v) for v in best[i]), tuple(int(v) for v in info[i]),
                                    int(status[i])) for i in range(count)]

    def collect(self):
        """Waits for the launch: one FleetMatchResult per submitted scan, in order."""
        rc, out = self.collect_code()
        self._chk(rc, "rgrid_batch_match_collect")
        return out

    def match(self, scans, options: RealTimeCorrelativeScanMatcherOptions | None = None):
        self.submit(scans, options)
        return self.collect()

    # -- CeresScanMatcher2D::Match for a batch -----------------------------------
    @staticmethod
    def pack_refine(scans):
        """scans: iterable of (grid_slot, target_translation, initial_pose, points_xy).  -> (ctypes array of rgrid_batch_refine_scan,
        count, the arrays it points into)."""
        scans = list(scans)
        arr = (RgridBatchRefineScan * max(len(scans), 1))()
        keep = []
        for i, (slot, target, pose, points) in enumerate(scans):
            pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
            keep.append(pts)
            s = arr[i]
            s.grid, s.n = int(slot), pts.shape[0]
            s.points_xy = pts.ctypes.data if s.n else None
            s.target_translation[0], s.target_translation[1] = float(target[0]), float(target[1])
            s.initial_pose[0], s.initial_pose[1], s.initial_pose[2] = float(pose[0]), float(pose[1]), float(pose[2])
        return arr, len(scans), keep

    def submit_refine_packed_code(self, packed, options: CeresScanMatcherOptions2D | None = None) -> int:
        co = _refine_options(options)
        return self._submitted(_refine_lib().rgrid_batch_refine_submit(self._h, C.byref(co), C.cast(packed[0], C.c_void_p), packed[1]), packed[1])

    def submit_refine_code(self, scans, options: CeresScanMatcherOptions2D | None = None) -> int:
        return self.submit_refine_packed_code(self.pack_refine(scans), options)

    def submit_refine(self, scans, options: CeresScanMatcherOptions2D | None = None):
        """One scan per entry, any grid slot each, the same options for all: ONE launch of kgb_refine; returns without waiting."""
        self._chk(self.submit_refine_code(scans, options), "rgrid_batch_refine_submit")

    def collect_refine_code(self):
        """-> (rc, [FleetRefineResult]) of the refine submit that has not been collected."""
        count = self._pending or 0
        n = max(count, 1)
        status, pose, summ = np.zeros(n, np.int32), np.zeros((n, 3)), (_RefineSummary * n)()
        rc = self._collected(_refine_lib().rgrid_batch_refine_collect(self._h, status.ctypes.data, pose.ctypes.data, C.cast(summ, C.c_void_p)))
        if rc != 0:
            return rc, []
        return 0, _refine_results(count, status, pose, summ)

    def collect_refine(self):
        rc, out = self.collect_refine_code()
        self._chk(rc, "rgrid_batch_refine_collect")
        return out

    def refine(self, scans, options: CeresScanMatcherOptions2D | None = None):
        self.submit_refine(scans, options)
        return self.collect_refine()

    # -- MapBuilder::ScanMatch for a batch: match, then refine, no host wait between them ---
    def submit_scan_match_packed_code(self, packed, match_options: RealTimeCorrelativeScanMatcherOptions | None = None,
                                      refine_options: CeresScanMatcherOptions2D | None = None) -> int:
        """``submit_scan_match_code`` for what ``pack`` returned."""
        cm, cr = _match_options(match_options), _refine_options(refine_options)
        return self._submitted(_refine_lib().rgrid_batch_scan_match_submit(self._h, C.byref(cm), C.byref(cr), C.cast(packed[0], C.c_void_p), packed[1]),
                               packed[1])

    def submit_scan_match_code(self, scans, match_options=None, refine_options=None) -> int:
        return self.submit_scan_match_packed_code(self.pack(scans), match_options, refine_options)

    def submit_scan_match(self, scans, match_options: RealTimeCorrelativeScanMatcherOptions | None = None,
                          refine_options: CeresScanMatcherOptions2D | None = None):
        """scans as ``submit`` takes them: the match's launch and the refinement's, back to back on the handle's stream; the
        refinement starts from each scan's matched pose with target_translation = initial_pose[:2] (map_builder.cc:49-53)."""
        self._chk(self.submit_scan_match_code(scans, match_options, refine_options), "rgrid_batch_scan_match_submit")

    def collect_scan_match_code(self):
        """-> (rc, [FleetScanMatchResult]) of the match-plus-refine submit that has not been collected."""
        count = self._pending or 0
        n = max(count, 1)
        status, coarse, score = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros(n)
        best, info = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.int32)
        pose, summ = np.zeros((n, 3)), (_RefineSummary * n)()
        rc = self._collected(_refine_lib().rgrid_batch_scan_match_collect(
            self._h, status.ctypes.data, coarse.ctypes.data, score.ctypes.data, best.ctypes.data, info.ctypes.data, pose.ctypes.data,
            C.cast(summ, C.c_void_p)))
        if rc != 0:
            return rc, []
        fine = _refine_results(count, status, pose, summ)
        return 0, [FleetScanMatchResult(FleetMatchResult(float(score[i]), coarse[i].copy(), tuple(int(v) for v in best[i]),
                                                         tuple(int(v) for v in info[i]), int(status[i])), fine[i]) for i in range(count)]

    def collect_scan_match(self):
        rc, out = self.collect_scan_match_code()
        self._chk(rc, "rgrid_batch_scan_match_collect")
        return out

    def scan_match(self, scans, match_options: RealTimeCorrelativeScanMatcherOptions | None = None,
                   refine_options: CeresScanMatcherOptions2D | None = None):
        self.submit_scan_match(scans, match_options, refine_options)
        return self.collect_scan_match()

    # -- MapBuilder::InsertIntoSubmap for a batch: grow and insert, each scan into its own slot ---
    @staticmethod
    def pack_insert(scans):
        """scans: iterable of (grid_slot, origin_xy, returns_xy, misses_xy_or_None).  -> (ctypes array of rgrid_batch_insert_scan,
        count, the arrays it points into)."""
        scans = list(scans)
        arr = (RgridBatchInsertScan * max(len(scans), 1))()
        keep = []
        for i, (slot, origin, returns, misses) in enumerate(scans):
            ret = np.ascontiguousarray(returns, dtype=np.float32).reshape(-1, 2)
            mis = np.zeros((0, 2), np.float32) if misses is None else np.ascontiguousarray(misses, dtype=np.float32).reshape(-1, 2)
            keep += [ret, mis]
            s = arr[i]
            s.grid, s.n_returns, s.n_misses = int(slot), ret.shape[0], mis.shape[0]
            s.returns_xy = ret.ctypes.data if s.n_returns else None
            s.misses_xy = mis.ctypes.data if s.n_misses else None
            s.origin_xy[0], s.origin_xy[1] = float(origin[0]), float(origin[1])
        return arr, len(scans), keep

    def submit_insert_packed_code(self, packed, options: RangeDataInserterOptions | None = None) -> int:
        """``submit_insert_code`` for what ``pack_insert`` returned (reusable: the points are copied by the call)."""
        co = _insert_options(options)
        return self._submitted(_insert_lib().rgrid_batch_insert_submit(self._h, C.byref(co), C.cast(packed[0], C.c_void_p), packed[1]), packed[1])

    def submit_insert_code(self, scans, options: RangeDataInserterOptions | None = None) -> int:
        return self.submit_insert_packed_code(self.pack_insert(scans), options)

    def submit_insert(self, scans, options: RangeDataInserterOptions | None = None):
        """One scan per entry, each into a slot of its own, the same options for all: ONE launch of kgb_insert; returns without waiting."""
        self._chk(self.submit_insert_code(scans, options), "rgrid_batch_insert_submit")

    def collect_insert_code(self):
        """-> (rc, [status]) of the insert submit that has not been collected."""
        count = self._pending or 0
        status = np.zeros(max(count, 1), np.int32)
        rc = self._collected(_insert_lib().rgrid_batch_insert_collect(self._h, status.ctypes.data))
        if rc != 0:
            return rc, []
        return 0, [int(v) for v in status[:count]]

    def collect_insert(self):
        """Waits for the launch: one status per submitted scan, in order -- RGRID_OK, or the first code GrowAsNeeded + Insert give
        for that scan (-1 a non-finite coordinate, -4 growth beyond max_cells / more points than max_points).  Raises only for what
        concerns the whole call."""
        rc, out = self.collect_insert_code()
        self._chk(rc, "rgrid_batch_insert_collect")
        return out

    def insert(self, scans, options: RangeDataInserterOptions | None = None):
        self.submit_insert(scans, options)
        return self.collect_insert()

    # -- the filter stage of MapBuilder::AddRangeData for a batch: two voxel filters and the adaptive filter per scan ---
    @staticmethod
    def pack_filter(scans):
        """scans: iterable of (returns_xy, misses_xy_or_None).  -> (ctypes array of rgrid_batch_filter_scan, count, the arrays it
        points into)."""
        scans = list(scans)
        arr = (RgridBatchFilterScan * max(len(scans), 1))()
        keep = []
        for i, (returns, misses) in enumerate(scans):
            ret = np.ascontiguousarray(returns, dtype=np.float32).reshape(-1, 2)
            mis = np.zeros((0, 2), np.float32) if misses is None else np.ascontiguousarray(misses, dtype=np.float32).reshape(-1, 2)
            keep += [ret, mis]
            s = arr[i]
            s.n_returns, s.n_misses = ret.shape[0], mis.shape[0]
            s.returns_xy = ret.ctypes.data if s.n_returns else None
            s.misses_xy = mis.ctypes.data if s.n_misses else None
        return arr, len(scans), keep

    def submit_filter_packed_code(self, packed, voxel_filter_size: float = 0.025, options: AdaptiveVoxelFilterOptions | None = None) -> int:
        """``submit_filter_code`` for what ``pack_filter`` returned (reusable: the points are copied by the call)."""
        co = _filter_options(voxel_filter_size, options)
        rc = self._submitted(_filter_lib().rgrid_batch_filter_submit(self._h, C.byref(co), C.cast(packed[0], C.c_void_p), packed[1]), packed[1])
        if rc == 0:
            self._filter_room = sum(2 * packed[0][i].n_returns + packed[0][i].n_misses for i in range(packed[1]))
        return rc

    def submit_filter_code(self, scans, voxel_filter_size: float = 0.025, options: AdaptiveVoxelFilterOptions | None = None) -> int:
        return self.submit_filter_packed_code(self.pack_filter(scans), voxel_filter_size, options)

    def submit_filter(self, scans, voxel_filter_size: float = 0.025, options: AdaptiveVoxelFilterOptions | None = None):
        """One scan per entry, the same sizes and options for all: ONE launch of kgb_filter; returns without waiting."""
        self._chk(self.submit_filter_code(scans, voxel_filter_size, options), "rgrid_batch_filter_submit")

    def collect_filter_code(self, out_cap_points: int | None = None):
        """-> (rc, [FleetFilterResult]) of the filter submit that has not been collected.  ``out_cap_points`` (default: what always
        suffices) is the room offered for the clouds: when it is too small the answer is (RGRID_ERR_BUFFER, [(|fr|, |fm|, |av|) per
        scan]) and the submit stays pending."""
        count = self._pending or 0
        n = max(count, 1)
        room = int(getattr(self, "_filter_room", 0) if out_cap_points is None else out_cap_points)
        status, counts, out = np.zeros(n, np.int32), np.zeros((n, 3), np.int32), np.zeros((max(room, 1), 2), np.float32)
        rc = self._collected(_filter_lib().rgrid_batch_filter_collect(self._h, status.ctypes.data, counts.ctypes.data, out.ctypes.data, room))
        if rc == RGRID_ERR_BUFFER:
            return rc, [tuple(int(v) for v in counts[i]) for i in range(count)]
        if rc != 0:
            return rc, []
        results, at = [], 0
        for i in range(count):
            clouds = []
            for k in counts[i]:
                clouds.append(out[at:at + k].copy())
                at += int(k)
            results.append(FleetFilterResult(int(status[i]), *clouds))
        return 0, results

    def collect_filter(self, out_cap_points: int | None = None):
        """Waits for the launch: one FleetFilterResult per submitted scan, in order.  Raises only for what concerns the whole call."""
        rc, out = self.collect_filter_code(out_cap_points)
        self._chk(rc, "rgrid_batch_filter_collect")
        return out

    def filter(self, scans, voxel_filter_size: float = 0.025, options: AdaptiveVoxelFilterOptions | None = None):
        self.submit_filter(scans, voxel_filter_size, options)
        return self.collect_filter()

    # -- MapBuilder::ToSubmapTexture for a batch: the known-cells box and its (value, alpha) bytes of every named slot ---
    def set_slots(self):
        """The slots that have been set, in ascending order."""
        return sorted(getattr(self, "_set_slots", ()))

    def submit_texture_code(self, slots) -> int:
        """-> the code of rgrid_batch_texture_submit for the named slots (any order, a slot any number of times)."""
        L = _texture_lib()
        ids = np.ascontiguousarray([int(k) for k in slots], dtype=np.int32)
        room = 0                                                                   # what collect's buffer must hold at most
        for k in ids:
            rc, lim = self.GetLimits_code(int(k)) if 0 <= k < self.num_grids else (RGRID_ERR_INVALID, None)
            room += 2 * lim[0] * lim[1] if rc == 0 else 0
        rc = self._submitted(L.rgrid_batch_texture_submit(self._h, ids.ctypes.data if ids.size else None, int(ids.size)), int(ids.size))
        if rc == 0:
            self._texture_room = room
        return rc

    def submit_texture(self, slots):
        """ONE launch of kgb_texture, one workgroup per named slot; returns without waiting.  The slots are only read."""
        self._chk(self.submit_texture_code(slots), "rgrid_batch_texture_submit")

    def collect_texture_code(self, cap: int | None = None):
        """-> (rc, [FleetTexture]) of the texture submit that has not been collected.  ``cap`` (default: what always suffices, from
        the slots' limits) is the room offered for the bytes: when it is too small the answer is (RGRID_ERR_BUFFER, [(box,
        slice_max, offset) per slot]) and the submit stays pending."""
        L = _texture_lib()
        count = self._pending or 0
        n = max(count, 1)
        room = int(getattr(self, "_texture_room", 0) if cap is None else cap)
        boxes, sm, offs = np.zeros((n, 4), np.int32), np.zeros((n, 2)), np.zeros(n, dtype=C.c_long)
        out = np.empty(max(room, 1), np.uint8)
        rc = self._collected(L.rgrid_batch_texture_collect(self._h, boxes.ctypes.data, sm.ctypes.data, offs.ctypes.data, out.ctypes.data, room))
        if rc == RGRID_ERR_BUFFER:
            return rc, [(tuple(int(v) for v in boxes[i]), (float(sm[i, 0]), float(sm[i, 1])), int(offs[i])) for i in range(count)]
        if rc != 0:
            return rc, []
        results = []
        for i in range(count):
            w, h, at = int(boxes[i, 2]), int(boxes[i, 3]), int(offs[i])
            # (a view: the textures of a call share the one buffer the library filled, and nothing else holds it)
            results.append(FleetTexture(out[at:at + 2 * w * h].reshape(h, w, 2), tuple(int(v) for v in boxes[i]),
                                        (float(sm[i, 0]), float(sm[i, 1]))))
        return 0, results

    def collect_texture(self, cap: int | None = None):
        """Waits for the launch: one FleetTexture per named slot, in order."""
        rc, out = self.collect_texture_code(cap)
        self._chk(rc, "rgrid_batch_texture_collect")
        return out

    def draw_textures(self, slots=None):
        """``GridFrontEnd.DrawTexture`` of every named slot (default: every slot that has been set) in ONE launch: a list of
        FleetTexture, in the order named."""
        self.submit_texture(self.set_slots() if slots is None else slots)
        return self.collect_texture()

    def submap_textures(self, slots, submap_origins):
        """``MapBuilder.ToSubmapTexture`` per named slot: a dict with the reference's SubmapTexture fields (grid_2d.h:16-24) --
        ``cells`` the raw (value, alpha) bytes, ``width``, ``height``, ``resolution``, ``slice_pose`` and ``global_pose`` as (x, y)
        translations.  ``submap_origins[i]`` is the local_pose translation of the submap in ``slots[i]`` (submap_2d.cc:18-24)."""
        slots = [int(k) for k in slots]
        origins = [(float(o[0]), float(o[1])) for o in submap_origins]
        if len(origins) != len(slots):
            raise ValueError("one submap origin per named slot")
        resolutions = [self.GetLimits(k)[2] for k in slots]
        out = []
        for tex, resolution, (ox, oy) in zip(self.draw_textures(slots), resolutions, origins):
            out.append({"cells": tex.cells, "width": tex.box[2], "height": tex.box[3], "resolution": resolution,
                        "slice_pose": (tex.slice_max[0] - ox, tex.slice_max[1] - oy), "global_pose": (ox, oy)})
        return out

    # -- Node::PublishMap / HandleSaveMap for a batch: the painted texture of every named slot ---------------------------
    def submit_occupancy_code(self, slots, submap_origins, mode: int = OCCUPANCY) -> int:
        """-> the code of rgrid_batch_occupancy_submit for the named slots (any order, a slot any number of times);
        ``submap_origins[i]`` is the local_pose translation of the submap in ``slots[i]``."""
        L = _occupancy_lib()
        ids = np.ascontiguousarray([int(k) for k in slots], dtype=np.int32)
        origins = np.ascontiguousarray([(float(o[0]), float(o[1])) for o in submap_origins], dtype=np.float64).reshape(-1, 2)
        if origins.shape[0] != ids.size:
            raise ValueError("one submap origin per named slot")
        room, resolutions = 0, []                                                  # what collect's buffer must hold at most
        for k in ids:
            rc, lim = self.GetLimits_code(int(k)) if 0 <= k < self.num_grids else (RGRID_ERR_INVALID, None)
            room += (lim[0] + 11) * (lim[1] + 11) if rc == 0 else 0
            resolutions.append(lim[2] if rc == 0 else 0.0)
        rc = self._submitted(L.rgrid_batch_occupancy_submit(self._h, int(mode), ids.ctypes.data if ids.size else None,
                                                            origins.ctypes.data if ids.size else None, int(ids.size)), int(ids.size))
        if rc == 0:
            self._occupancy_room, self._occupancy_mode, self._occupancy_resolutions = room, int(mode), resolutions
        return rc

    def submit_occupancy(self, slots, submap_origins, mode: int = OCCUPANCY):
        """ONE launch of kgb_occupancy, one workgroup per named slot; returns without waiting.  The slots are only read."""
        self._chk(self.submit_occupancy_code(slots, submap_origins, mode), "rgrid_batch_occupancy_submit")

    def collect_occupancy_code(self, cap: int | None = None):
        """-> (rc, [FleetOccupancyGrid]) of the occupancy submit that has not been collected.  ``cap`` (default: what always
        suffices, from the slots' limits) is the room offered for the bytes: when it is too small the answer is (RGRID_ERR_BUFFER,
        [(status, size, origin, box, offset) per slot]) and the submit stays pending."""
        L = _occupancy_lib()
        count = self._pending or 0
        n = max(count, 1)
        room = int(getattr(self, "_occupancy_room", 0) if cap is None else cap)
        mode = getattr(self, "_occupancy_mode", OCCUPANCY)
        status, sizes, origins = np.zeros(n, np.int32), np.zeros((n, 2), np.int32), np.zeros((n, 2))
        boxes, offs = np.zeros((n, 4), np.int32), np.zeros(n, dtype=C.c_long)
        out = np.empty(max(room, 1), np.int8 if mode == OCCUPANCY else np.uint8)
        rc = self._collected(L.rgrid_batch_occupancy_collect(self._h, status.ctypes.data, sizes.ctypes.data, origins.ctypes.data,
                                                             boxes.ctypes.data, offs.ctypes.data, out.ctypes.data, room))
        if rc == RGRID_ERR_BUFFER:
            return rc, [(int(status[i]), tuple(int(v) for v in sizes[i]), (float(origins[i, 0]), float(origins[i, 1])),
                         tuple(int(v) for v in boxes[i]), int(offs[i])) for i in range(count)]
        if rc != 0:
            return rc, []
        results = []
        for i in range(count):
            sx, sy, at = int(sizes[i, 0]), int(sizes[i, 1]), int(offs[i])
            # (a view: the images of a call share the one buffer the library filled, and nothing else holds it)
            results.append(FleetOccupancyGrid(out[at:at + sx * sy].reshape(sy, sx), self._occupancy_resolutions[i],
                                              (float(origins[i, 0]), float(origins[i, 1])), tuple(int(v) for v in boxes[i]), int(status[i])))
        return 0, results

    def collect_occupancy(self, cap: int | None = None):
        """Waits for the launch: one FleetOccupancyGrid per named slot, in order."""
        rc, out = self.collect_occupancy_code(cap)
        self._chk(rc, "rgrid_batch_occupancy_collect")
        return out

    def occupancy_grids(self, slots, submap_origins, mode: int = OCCUPANCY):
        """``GridFrontEnd.OccupancyGrid`` of every named slot in ONE launch: a list of FleetOccupancyGrid, in the order named."""
        self.submit_occupancy(slots, submap_origins, mode)
        return self.collect_occupancy()

    # -- MapBuilder::AddRangeData for a batch: every stage above in ONE C call ------------------------------------------------
    @staticmethod
    def pack_range_data(range_datas, ekf_poses, slots=None):
        """One ``map_builder.RangeData`` (tracking frame) and one EKF pose (x, y, yaw) per scan, scan i into slot ``slots[i]``
        (default: slot i).  -> (ctypes array of rgrid_batch_range_data, count, the arrays it points into)."""
        range_datas, ekf_poses = list(range_datas), list(ekf_poses)
        slots = list(range(len(range_datas))) if slots is None else [int(k) for k in slots]
        if not len(range_datas) == len(ekf_poses) == len(slots):
            raise ValueError("one EKF pose and one slot per scan")
        arr = (RgridBatchRangeData * max(len(range_datas), 1))()
        keep = []
        for i, (rd, pose, slot) in enumerate(zip(range_datas, ekf_poses, slots)):
            ret = np.ascontiguousarray(rd.returns, dtype=np.float32).reshape(-1, 2)
            mis = np.zeros((0, 2), np.float32) if rd.misses is None else np.ascontiguousarray(rd.misses, dtype=np.float32).reshape(-1, 2)
            keep += [ret, mis]
            s = arr[i]
            s.grid, s.n_returns, s.n_misses = slot, ret.shape[0], mis.shape[0]
            s.returns_xy = ret.ctypes.data if s.n_returns else None
            s.misses_xy = mis.ctypes.data if s.n_misses else None
            s.origin_xy[0], s.origin_xy[1] = float(rd.origin[0]), float(rd.origin[1])
            s.ekf_pose[0], s.ekf_pose[1], s.ekf_pose[2] = float(pose[0]), float(pose[1]), float(pose[2])
        return arr, len(range_datas), keep

    def add_range_data_packed_code(self, packed, options=None, cap_points: int | None = None, want_returns: bool = True):
        """``add_range_data_code`` for what ``pack_range_data`` returned.  ``cap_points`` (default: the sum of the counts) is the room
        offered for the returns; without ``want_returns`` the raw returns are not transformed at all."""
        L = _range_data_lib()
        arr, count, _ = packed
        n = max(count, 1)
        co = _map_builder_options(options)
        total = sum(arr[i].n_returns for i in range(count))
        room = total if cap_points is None else int(cap_points)
        codes, status, poses = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3))
        origins, out = np.zeros((n, 2), np.float32), np.zeros((max(room, total, 1), 2), np.float32)
        rc = L.rgrid_batch_add_range_data(self._h, C.byref(co), C.cast(arr, C.c_void_p), count, codes.ctypes.data, status.ctypes.data,
                                          poses.ctypes.data, origins.ctypes.data, out.ctypes.data if want_returns else None, room)
        if rc != 0:
            return rc, []
        results, at = [], 0
        for i in range(count):
            k = arr[i].n_returns
            results.append(FleetRangeDataResult(int(codes[i]), int(status[i]), poses[i].copy(), (float(origins[i, 0]), float(origins[i, 1])),
                                                out[at:at + k].copy()))
            at += k
            if codes[i] == 0 and status[i] == SCAN_INSERTED:
                self._set_slots.add(int(arr[i].grid))
        return 0, results

    def add_range_data_code(self, range_datas, ekf_poses, slots=None, options=None):
        """-> (rc, [FleetRangeDataResult]): rc concerns the whole call (RGRID_ERR_INVALID, RGRID_ERR_BUFFER: nothing was launched),
        a scan's own error is its result's ``code``."""
        return self.add_range_data_packed_code(self.pack_range_data(range_datas, ekf_poses, slots), options)

    def add_range_data(self, range_datas, ekf_poses, slots=None, options=None, times=None):
        """``MapBuilder.AddRangeData`` for one scan of every robot in ONE call: per scan a ``map_builder.MatchingResult`` -- ``local_pose``
        and ``range_data_in_local.returns`` the bits ``GridFrontEnd.AddRangeData`` returns for that robot; ``range_data_in_local``'s origin
        and misses are not computed (None) -- or None where the reference returns nullptr (no returns, nothing left after the
        filters).  A scan's own error raises RgridError after the whole call has run; ``add_range_data_code`` hands the codes out."""
        from .map_builder import MatchingResult, RangeData
        rc, results = self.add_range_data_code(range_datas, ekf_poses, slots, options)
        self._chk(rc, "rgrid_batch_add_range_data")
        for i, r in enumerate(results):
            if r.code != 0:
                raise self._error(r.code, f"rgrid_batch_add_range_data: scan {i}")
        times = [None] * len(results) if times is None else list(times)
        return [MatchingResult(t, r.local_pose, RangeData(None, r.returns_in_local, None)) if r.status == SCAN_INSERTED else None
                for t, r in zip(times, results)]

    def last_call_counts(self):
        """(kernel launches, stream synchronisations) of the last ``add_range_data``: independent of the number of scans."""
        out = (C.c_int * 2)()
        self._chk(_range_data_lib().rgrid_batch_last_call_counts(self._h, C.cast(out, C.c_void_p)), "rgrid_batch_last_call_counts")
        return int(out[0]), int(out[1])

    def GetLimits_code(self, slot: int):
        nx, ny = C.c_int(), C.c_int()
        res, mx, my = C.c_double(), C.c_double(), C.c_double()
        rc = _insert_lib().rgrid_batch_get_limits(self._h, int(slot), C.byref(nx), C.byref(ny), C.byref(res), C.byref(mx), C.byref(my))
        return rc, (nx.value, ny.value, res.value, mx.value, my.value)

    def GetLimits(self, slot: int):
        """MapLimits of slot ``slot`` as ``GridFrontEnd.GetLimits`` gives them: (num_x_cells, num_y_cells, resolution, max_x, max_y)."""
        rc, lim = self.GetLimits_code(slot)
        self._chk(rc, "rgrid_batch_get_limits")
        return lim

    def GetGrid_code(self, slot: int):
        rc, lim = self.GetLimits_code(slot)
        if rc != 0:
            return rc, None
        out = np.zeros((lim[1], lim[0]), np.uint16)
        rc = _insert_lib().rgrid_batch_get_grid(self._h, int(slot), out.ctypes.data, out.size)
        return rc, (out if rc == 0 else None)

    def GetGrid(self, slot: int) -> np.ndarray:
        """The cells of slot ``slot``: uint16 (num_y_cells, num_x_cells).  Not between a submit and its collect."""
        rc, out = self.GetGrid_code(slot)
        self._chk(rc, "rgrid_batch_get_grid")
        return out

    def last_prepare_seconds(self) -> float:
        """Host time the last submit (of any kind) spent before its launch: initial rotations, search parameters, rotation tables, packing."""
        return float(self._L.rgrid_batch_last_prepare_seconds(self._h))
