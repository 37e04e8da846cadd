/* rgrid.h -- C ABI of the MI355X-native grid-mapper front-end: the step right after
 * the hot path, which consumes the detector's de-skewed returns (rdet2d_get_range_data) and the EKF pose.
 *
 * It replaces, in the reference (ShihanWang/reflector_ekf_slam):
 *   sensor::VoxelFilter::Filter                 src/sensor/voxel_filter.cc:81-95   (called from map_builder.cc:30-31)
 *   sensor::AdaptiveVoxelFilter::Filter         src/sensor/voxel_filter.cc:116-120 (map_builder.cc:73)
 *   scan_matching::RealTimeCorrelativeScanMatcher2D::Match
 *                                               src/scan_matching/real_time_correlative_scan_matcher_2d.cc:84-118
 *                                               (map_builder.cc:43) with its helpers SearchParameters,
 *                                               GenerateRotatedScans, DiscretizeScans
 *                                               (correlative_scan_matcher_2d.cc:10-123)
 *   mapping::ProbabilityGridRangeDataInserter2D::Insert
 *                                               src/mapping/probability_grid_range_data_inserter_2d.cc:40-114
 *                                               (map_builder.cc: range_data_inserter_->Insert); its GrowAsNeeded /
 *                                               Grid2D::GrowLimits step (:20-38, src/mapping/grid_2d.cc:59-99) is
 *                                               rgrid_grow_as_needed
 *   scan_matching::CeresScanMatcher2D::Match    src/scan_matching/ceres_scan_matcher_2d.cc:26-62 (map_builder.cc:49-53) with
 *                                               occupied_space_cost_function_2d.cc:25-52 and the translation / rotation
 *                                               delta functors -- the Ceres solve restated (Ceres is not a pinned
 *                                               dependency of the reference: parity with a Ceres build is unpinned)
 *   mapping::ProbabilityGrid::DrawToSubmapTexture
 *                                               src/mapping/probability_grid.cc:86-131 (Submap2D::GetMapTextureData,
 *                                               MapBuilder::ToSubmapTexture, map_builder.cc:128-134) without the gzip
 *                                               container
 * Not covered: Submap2D::Finish / ComputeCroppedGrid (never called by the reference's node), IO.
 *
 * Conventions as in rekf.h / rdet.h: opaque handles, plain pointers and sizes, 0 / negative error codes,
 * caller owns every buffer, a handle is not thread-safe, calls synchronise before returning.
 */
#ifndef RGRID_H_
#define RGRID_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGRID_ABI_VERSION 4

enum {
    RGRID_OK = 0,
    RGRID_ERR_INVALID = -1,       /* bad argument */
    RGRID_ERR_HIP = -2,           /* a HIP runtime call failed */
    RGRID_ERR_CAPACITY = -4,      /* more points / cells / candidates than the handle was created for */
    RGRID_ERR_BUFFER = -5,        /* caller buffer too small */
    RGRID_ERR_EMPTY = -6          /* empty point cloud (the reference CHECK-fails, real_time_...cc:33) */
};

typedef struct rgrid rgrid_t;

/* scan_matching::RealTimeCorrelativeScanMatcherOptions (real_time_correlative_scan_matcher_2d.h:34-40);
 * defaults in the reference's caller: 0.2 m, 15 deg (in radians here), 1e-1, 1e-1 (src/ros_node.cc:329-344). */
typedef struct rgrid_match_options {
    double linear_search_window;
    double angular_search_window;
    double translation_delta_cost_weight;
    double rotation_delta_cost_weight;
} rgrid_match_options;

/* One handle = one HIP stream + device buffers for up to max_points points, max_cells grid cells and
 * max_candidates search candidates (num_scans * (2 * num_linear + 1)^2). */
int rgrid_create(int max_points, int max_cells, int max_candidates, int device, rgrid_t **out);
void rgrid_destroy(rgrid_t *h);

/* sensor::VoxelFilter(resolution).Filter(points): the first point that falls into every voxel, input
 * order kept (voxel_filter.cc:81-95).  out_xy holds out_cap points; *m = points written. */
int rgrid_voxel_filter(rgrid_t *h, const float *xy, int n, float resolution, float *out_xy, int out_cap, int *m);

/* sensor::AdaptiveVoxelFilter(options).Filter(points) (voxel_filter.cc:15-76,116-120): range gate, then the
 * coarsest voxel size <= max_length (bisection to 10 %) that still leaves min_num_points points.
 * Reference defaults: 0.9, 500, 100 (src/ros_node.cc:312-322). */
int rgrid_adaptive_voxel_filter(rgrid_t *h, const float *xy, int n, double max_length, double min_num_points,
                                double max_range, float *out_xy, int out_cap, int *m);

/* The probability grid the matcher scores against (mapping::ProbabilityGrid / Grid2D): correspondence-cost cell
 * values as the reference stores them (uint16, 0 = unknown, grid_2d.h:83-91), flat index num_x_cells * y + x
 * (grid_2d.h:102-106), MapLimits (resolution, max.x, max.y) (map_limits.h:24-45).  The cells are copied to the
 * device and stay resident until the next call. */
int rgrid_set_grid(rgrid_t *h, const uint16_t *cells, int num_x_cells, int num_y_cells, double resolution,
                   double max_x, double max_y);

/* ProbabilityGridRangeDataInserter2D::Insert (src/mapping/probability_grid_range_data_inserter_2d.cc:40-114) on the
 * resident grid: the cell of every return gets the hit table, every cell on the rays origin -> return and
 * origin -> miss the miss table (RayToPixelMask, ray_to_pixel_mask.cc:17-168, sub-pixel scale 1000), a cell is
 * updated at most once per insertion and hits win (probability_grid.cc:38-53), then FinishUpdate (grid_2d.cc:20-29).
 * hit / miss probabilities: the reference's options are float (0.55 / 0.49, src/ros_node.cc:390-396).
 * GrowAsNeeded is a call of its own (rgrid_grow_as_needed, to be made first as CastRays does, :45): here a point
 * outside the grid returns RGRID_ERR_CAPACITY and leaves the grid untouched.
 * The grid must be in the finished state (no cell with the update marker 0x8000 set). */
int rgrid_insert(rgrid_t *h, const float origin_xy[2], const float *returns_xy, int n_returns, const float *misses_xy,
                 int n_misses, float hit_probability, float miss_probability, int insert_free_space);

/* GrowAsNeeded (probability_grid_range_data_inserter_2d.cc:20-38): the float bounding box of origin, returns and
 * misses, padded by 1e-6, and Grid2D::GrowLimits (src/mapping/grid_2d.cc:59-99) for its two corners -- the grid
 * doubles in both directions (old cells in the middle, new cells unknown, max += resolution * (ny / 2, nx / 2))
 * until it contains the corner.  RGRID_ERR_CAPACITY (grid untouched) if that needs more than max_cells cells;
 * non-finite coordinates are RGRID_ERR_INVALID (the reference would loop forever). */
int rgrid_grow_as_needed(rgrid_t *h, const float origin_xy[2], const float *returns_xy, int n_returns,
                         const float *misses_xy, int n_misses);

/* MapLimits of the resident grid (any pointer may be NULL). */
int rgrid_get_limits(rgrid_t *h, int *num_x_cells, int *num_y_cells, double *resolution, double *max_x, double *max_y);

/* Copy of the resident grid cells (num_x_cells * num_y_cells values, same layout as rgrid_set_grid). */
int rgrid_get_grid(rgrid_t *h, uint16_t *cells, long cap);

/* RealTimeCorrelativeScanMatcher2D::Match (real_time_correlative_scan_matcher_2d.cc:84-118):
 * initial_pose = (x, y, rotation angle); points in the tracking frame; pose_estimate = (x, y, angle) of the best
 * candidate (first maximum in the reference's candidate order); returns its score in *score.
 * best3 (nullable) = (scan_index, x_index_offset, y_index_offset); info3 (nullable) = (num_scans,
 * num_linear_perturbations, num_candidates).  RGRID_ERR_CAPACITY, before any launch, also for a search window that is
 * negative or NaN or whose candidate count no int holds: the check rgrid_batch_match_submit makes per scan. */
int rgrid_match(rgrid_t *h, const rgrid_match_options *opt, const double initial_pose[3], const float *points_xy,
                int n, double pose_estimate[3], double *score, int best3[3], int info3[3]);

/* ProbabilityGrid::DrawToSubmapTexture (probability_grid.cc:86-131): the resident grid cropped to the bounding box of its
 * known cells, two bytes per cell (value, alpha), x fastest -- the string the reference gzips into SubmapTexture::cells.
 * box = (offset_x, offset_y, width, height) in cells; slice_max = limits.max - resolution * (offset_y, offset_x), the
 * translation of SubmapTexture::slice_pose before local_pose^-1 is applied (:122-126).  cells needs
 * 2 * width * height bytes (at most 2 * num_x_cells * num_y_cells); RGRID_ERR_BUFFER reports the box it would need. */
int rgrid_draw_texture(rgrid_t *h, uint8_t *cells, long cap, int box[4], double slice_max[2]);

/* scan_matching::CeresScanMatcherOptions2D (ceres_scan_matcher_2d.h:16-22) + the two ceres::Solver::Options fields the
 * reference sets (src/ros_node.cc:350-377): defaults 1.0, 0.1, 0.4, 100 iterations, non-monotonic steps on. */
typedef struct rgrid_refine_options {
    double occupied_space_weight;
    double translation_weight;
    double rotation_weight;
    int max_num_iterations;
    int use_nonmonotonic_steps;
} rgrid_refine_options;

/* What the reference reads of ceres::Solver::Summary, reduced: termination 0 = CONVERGENCE, 1 = NO_CONVERGENCE
 * (iteration limit), 2 = FAILURE (five invalid steps in a row). */
typedef struct rgrid_refine_summary {
    double initial_cost;
    double final_cost;
    int iterations;
    int termination;
} rgrid_refine_summary;

/* CeresScanMatcher2D::Match (ceres_scan_matcher_2d.cc:26-62) against the resident grid: minimises over (x, y, angle)
 *   sum_i (occupied_space_weight / sqrt(n) * bicubic correspondence cost at point i)^2
 *   + (translation_weight * (xy - target_translation))^2 + (rotation_weight * (angle - initial angle))^2
 * with Ceres' Levenberg-Marquardt trust-region loop at its default tolerances.  initial_pose_estimate = the
 * correlative matcher's answer, target_translation = the prediction's translation (map_builder.cc:49-53).
 * summary may be NULL. */
int rgrid_refine_match(rgrid_t *h, const rgrid_refine_options *opt, const double target_translation[2],
                       const double initial_pose[3], const float *points_xy, int n, double pose_estimate[3],
                       rgrid_refine_summary *summary);

/* mapping::MapBuilderOptions (include/mapping/map_builder.h:22-30), flattened; defaults = src/ros_node.cc:299-396:
 * 0.05, 0.025, {0.9, 500, 100}, {0.2, 15 deg in rad, 0.1, 0.1}, {1, 0.1, 0.4, 100, 1}, 0.55, 0.49, 1. */
typedef struct rgrid_map_builder_options {
    float resolution;
    float voxel_filter_size;
    double adaptive_max_length, adaptive_min_num_points, adaptive_max_range;
    rgrid_match_options match;
    rgrid_refine_options refine;
    float hit_probability, miss_probability;
    int insert_free_space;
} rgrid_map_builder_options;

enum { RGRID_SCAN_INSERTED = 0, RGRID_SCAN_DROPPED_EMPTY = 1, RGRID_SCAN_FILTERED_EMPTY = 2 };

/* mapping::MapBuilder::AddRangeData (src/mapping/map_builder.cc:57-108) in one call, on the handle's resident grid (created
 * on the first call as MapBuilder::CreateGrid does, :112-126: 100 x 100 cells around the first origin): gravity
 * alignment + voxel filters (:20-32), adaptive filter (:72-73), ScanMatch = correlative match + refinement (:34-55),
 * InsertIntoSubmap = grow + insert (:110-120).  range_data (origin, returns, misses) is in the tracking frame, ekf_pose =
 * (x, y, yaw) as the node builds it (src/ros_node.cc:547-549).  local_pose = Project2D(MatchingResult::local_pose);
 * returns_in_local (nullable, 2 * n_returns floats) = MatchingResult::range_data_in_local.returns.  *status tells what the
 * reference would have returned: a result (RGRID_SCAN_INSERTED) or nullptr (the other two). */
int rgrid_add_range_data(rgrid_t *h, const rgrid_map_builder_options *opt, const float origin_xy[2], const float *returns_xy,
                         int n_returns, const float *misses_xy, int n_misses, const double ekf_pose[3], double local_pose[3],
                         float *returns_in_local, int *status);

/* ---- fleet scan matcher: RealTimeCorrelativeScanMatcher2D::Match for one scan of many robots, one launch per call
 * (csrc/rgrid_batch.hip).  A batch handle owns one HIP stream, num_grids resident grids of up to max_cells cells that any
 * number of scans may share, and staging for max_scans scans of up to max_points points each.  Every scan's pose_estimate,
 * score, best3 and info3 are exactly what rgrid_match returns for that scan, that grid and those options. */
typedef struct rgrid_batch rgrid_batch_t;
typedef struct rgrid_batch_scan {      /* one scan of a call */
    int grid;                          /* resident grid slot it is matched against */
    int n;                             /* points */
    const float *points_xy;            /* tracking frame, 2*n floats */
    double initial_pose[3];            /* x, y, angle */
} rgrid_batch_scan;

/* max_rotations: rotated scans a single scan may need (2 * num_angular + 1); rgrid_match's limit of 1024 holds here too.
 * RGRID_ERR_CAPACITY when one staging segment -- 280 * max_scans + 8 * max_scans * (2 * R + 2 * max_points) bytes plus alignment,
 * R = min(max_rotations, 1024): the records, rotation tables and rotated points of a match AND the records and raw points of a
 * refinement, reserved for every handle -- would exceed 2^31 - 1 bytes, or max_points exceeds 16384. */
int rgrid_batch_create(int max_scans, int max_points, int num_grids, long max_cells, int max_rotations, int device,
                       rgrid_batch_t **out);
void rgrid_batch_destroy(rgrid_batch_t *b);

/* rgrid_set_grid for slot `grid`.  RGRID_ERR_INVALID between a submit (of any kind) and its collect. */
int rgrid_batch_set_grid(rgrid_batch_t *b, int grid, const uint16_t *cells, int num_x_cells, int num_y_cells,
                         double resolution, double max_x, double max_y);

/* Enqueues the match of scans[0 .. count) and returns without waiting.  The whole call is refused with RGRID_ERR_INVALID, and
 * nothing is launched, for a null pointer, count outside [0, max_scans], a grid slot out of range or not yet set, or a submit
 * that has not been collected.  What belongs to one scan is reported by collect in status[j] and leaves the other scans
 * untouched: RGRID_ERR_EMPTY (n == 0), RGRID_ERR_CAPACITY (n > max_points, more rotated scans than max_rotations or 1024).
 * The points are copied before the call returns. */
int rgrid_batch_match_submit(rgrid_batch_t *b, const rgrid_match_options *opt, const rgrid_batch_scan *scans, int count);

/* Waits for the handle's stream and hands out the results of the pending submit, in its order: status (count), pose_estimates
 * (3 * count), scores (count), best3 / info3 (3 * count each, nullable) as rgrid_match defines them; entries of a scan whose
 * status is not RGRID_OK are zero.  RGRID_ERR_INVALID without a pending submit. */
int rgrid_batch_match_collect(rgrid_batch_t *b, int *status, double *pose_estimates, double *scores, int *best3, int *info3);

/* Where the arg-max over a scan's rotated scans is taken: by the workgroup of that scan that finishes last, inside the one
 * launch (the default), or by a second launch with one workgroup per scan.  The results are the same bits.
 * RGRID_ERR_INVALID between a submit and its collect. */
enum { RGRID_BATCH_REDUCE_ARRIVAL = 0, RGRID_BATCH_REDUCE_LAUNCH = 1 };
int rgrid_batch_set_reduction(rgrid_batch_t *b, int mode);

/* Host seconds the last submit, of whichever kind, spent before its launch (initial rotations, search parameters, rotation
 * tables, packing). */
double rgrid_batch_last_prepare_seconds(rgrid_batch_t *b);

/* ---- fleet refinement: CeresScanMatcher2D::Match for one scan of many robots, one launch per call (kgb_refine, one workgroup
 * per scan, csrc/rgrid_batch.hip).  Every scan's pose_estimate and summary are exactly what rgrid_refine_match returns for that
 * scan, that grid and those options.  A handle has ONE pending submit at a time, of any kind, and each kind has its own collect:
 * a collect of another kind than the pending submit is RGRID_ERR_INVALID and leaves the submit pending.  The ABI version stays 4:
 * a caller that may meet an older library looks for these symbols. */
typedef struct rgrid_batch_refine_scan {   /* one scan of a refine call */
    int grid;                              /* resident grid slot it is refined against */
    int n;                                 /* points */
    const float *points_xy;                /* tracking frame, 2*n floats */
    double target_translation[2];          /* the prediction's translation */
    double initial_pose[3];                /* the correlative matcher's answer */
} rgrid_batch_refine_scan;

/* Enqueues the refinement of scans[0 .. count) and returns without waiting.  Refused as a whole with RGRID_ERR_INVALID, nothing
 * launched and the handle still usable, for what rgrid_batch_match_submit refuses as a whole, a pending submit of any kind, and
 * the options rgrid_refine_match refuses (a weight not > 0, max_num_iterations < 0).  Per scan, in collect's status[j]:
 * RGRID_ERR_EMPTY (n == 0), RGRID_ERR_CAPACITY (n > max_points); such a scan gets no workgroup.  The points are copied before
 * the call returns. */
int rgrid_batch_refine_submit(rgrid_batch_t *b, const rgrid_refine_options *opt, const rgrid_batch_refine_scan *scans, int count);

/* Waits and hands out the pending refine submit's results in its order: status (count), pose_estimates (3 * count), summaries
 * (count, nullable); entries of a scan whose status is not RGRID_OK are zero. */
int rgrid_batch_refine_collect(rgrid_batch_t *b, int *status, double *pose_estimates, rgrid_refine_summary *summaries);

/* MapBuilder::ScanMatch (map_builder.cc:34-55) for a batch: the correlative match, then the refinement started from the match's
 * pose estimate with target_translation = initial_pose[0:2] -- two launches on the handle's stream (three with
 * RGRID_BATCH_REDUCE_LAUNCH) and NO host synchronisation between them: the refinement decodes each scan's winning candidate on
 * the device.  Whole-call refusals: those of both submits above.  Per-scan statuses: rgrid_batch_match_submit's; a scan whose
 * status is not RGRID_OK is neither matched nor refined. */
int rgrid_batch_scan_match_submit(rgrid_batch_t *b, const rgrid_match_options *mopt, const rgrid_refine_options *ropt,
                                  const rgrid_batch_scan *scans, int count);

/* Both stages' results: status, coarse_poses, scores, best3, info3 as rgrid_batch_match_collect gives them (best3 / info3
 * nullable), pose_estimates (3 * count) and summaries (count, nullable) as rgrid_batch_refine_collect gives them. */
int rgrid_batch_scan_match_collect(rgrid_batch_t *b, int *status, double *coarse_poses, double *scores, int *best3, int *info3,
                                   double *pose_estimates, rgrid_refine_summary *summaries);

/* ---- fleet inserter: ProbabilityGridRangeDataInserter2D::Insert with its GrowAsNeeded (MapBuilder::InsertIntoSubmap,
 * map_builder.cc:110-120) for one scan of many robots, each into its own resident slot, ONE launch per call (kgb_insert, one
 * workgroup per scan, csrc/rgrid_batch.hip).  The specification is the pair of single calls: after collect, slot scans[j].grid
 * holds the cells (bit for bit) and the limits that an rgrid_t holding the same grid, created with the batch's max_cells, holds
 * after rgrid_grow_as_needed(...) followed by rgrid_insert(...), and status[j] is the first code of that pair that is not RGRID_OK:
 *   RGRID_ERR_INVALID   a non-finite coordinate (slot untouched);
 *   RGRID_ERR_CAPACITY  growth beyond max_cells (slot untouched); n_returns or n_misses above max_points, or an end point outside
 *                       the grid after growth (slot grown as the pair grows it, nothing inserted);
 *   RGRID_OK            otherwise, a scan with neither returns nor misses included.
 * Other scans of the call are unaffected.  The map stays on the device: a later match, refine or scan_match submit reads the
 * inserted cells and the grown limits.  The ABI version stays 4: a caller that may meet an older library looks for these symbols. */
typedef struct rgrid_insert_options { float hit_probability, miss_probability; int insert_free_space; } rgrid_insert_options;
typedef struct rgrid_batch_insert_scan {   /* 40 bytes on LP64 */
    int grid;                              /* resident slot the scan is inserted into */
    int n_returns, n_misses;
    const float *returns_xy, *misses_xy;   /* frame of the grid, 2*n floats each, NULL when n == 0 */
    float origin_xy[2];
} rgrid_batch_insert_scan;

/* Enqueues the insertion of scans[0 .. count) and returns without waiting; the points are copied before the call returns.  Refused
 * as a whole with RGRID_ERR_INVALID, nothing launched and the handle still usable: a null b, opt or scans, count outside
 * [0, max_scans], a slot out of range or not yet set, a negative point count, a null pointer with a positive count, a probability
 * not strictly inside (0, 1), a pending submit of any kind, and TWO SCANS NAMING THE SAME SLOT -- the reference inserts one after
 * the other with FinishUpdate in between, two insertions into one grid in one launch have no reference meaning: robots that share a
 * map insert in consecutive calls.  The two lookup tables stay on the device and are rebuilt only when the probabilities change. */
int rgrid_batch_insert_submit(rgrid_batch_t *b, const rgrid_insert_options *opt, const rgrid_batch_insert_scan *scans, int count);

/* Waits and hands out status (count) of the pending insert submit, in its order.  RGRID_ERR_INVALID without one, or while a submit
 * of another kind is pending (which stays pending). */
int rgrid_batch_insert_collect(rgrid_batch_t *b, int *status);

/* rgrid_get_limits / rgrid_get_grid for slot `grid` (any pointer of get_limits may be NULL; get_grid: RGRID_ERR_BUFFER when cap is
 * below num_x_cells * num_y_cells).  RGRID_ERR_INVALID for a slot not yet set and between a submit (of any kind) and its collect. */
int rgrid_batch_get_limits(rgrid_batch_t *b, int grid, int *num_x_cells, int *num_y_cells, double *resolution, double *max_x,
                           double *max_y);
int rgrid_batch_get_grid(rgrid_batch_t *b, int grid, uint16_t *cells, long cap);

/* ---- fleet voxel filters: the filter stage of MapBuilder::AddRangeData (map_builder.cc:30-31,73) for one scan of many robots,
 * ONE launch and ONE synchronisation per call (kgb_filter, one workgroup per scan, csrc/rgrid_batch.hip).  The specification is
 * the single calls: for scan j, fr = rgrid_voxel_filter(returns, voxel_filter_size), fm = rgrid_voxel_filter(misses,
 * voxel_filter_size) -- a filter of its own: the returns' voxels do not suppress misses -- and av = rgrid_adaptive_voxel_filter(fr,
 * adaptive_max_length, adaptive_min_num_points, adaptive_max_range), each the same points in input order with the input's bit
 * patterns.  The points are float32 xy, already in the gravity-aligned frame: nothing is rotated here.  The filter needs no grid:
 * it works on a handle whose slots were never set.  Its staging is allocated by the handle's first filter submit.  Finite
 * coordinates whose voxel index (int)lroundf(v / size) no int holds are outside the contract, as they are for rgrid_voxel_filter.
 * The ABI version stays 4: a caller that may meet an older library looks for these symbols. */
typedef struct rgrid_filter_options { float voxel_filter_size; double adaptive_max_length, adaptive_min_num_points, adaptive_max_range; } rgrid_filter_options;
typedef struct rgrid_batch_filter_scan {   /* 24 bytes on LP64 */
    int n_returns, n_misses;
    const float *returns_xy, *misses_xy;   /* 2*n floats each, NULL when n == 0 */
} rgrid_batch_filter_scan;

/* Enqueues the filters of scans[0 .. count) and returns without waiting; the points are copied before the call returns.  Refused as
 * a whole with RGRID_ERR_INVALID, nothing launched and the handle still usable: a null b, opt or scans, count outside
 * [0, max_scans], a negative point count, a null pointer with a positive count, voxel_filter_size or adaptive_max_length not > 0
 * (NaN included), a pending submit of any kind.  Per scan, in collect's status[j], the other scans unaffected, no workgroup and
 * counts 0 for such a scan: RGRID_ERR_CAPACITY (n_returns or n_misses above min(max_points, rgrid_batch_filter_max_points())),
 * RGRID_ERR_INVALID (a non-finite coordinate: the reference's lround of it is undefined).  A scan without returns is RGRID_OK with
 * counts (0, |fm|, 0): whether AddRangeData would drop it is the caller's decision. */
int rgrid_batch_filter_submit(rgrid_batch_t *b, const rgrid_filter_options *opt, const rgrid_batch_filter_scan *scans, int count);

/* Waits once and hands out the pending filter submit's results in its order: status (count), counts (3 * count: |fr|, |fm|, |av| of
 * every scan) and the clouds, consecutively in out_xy: scan 0's fr, fm, av, then scan 1's, ...; the offsets follow from counts.
 * RGRID_ERR_BUFFER when out_cap_points is below the sum of counts: status and counts are filled and the submit is LEFT PENDING, the
 * caller comes again with room; out_cap_points = sum of 2 * n_returns + n_misses always suffices.  RGRID_ERR_INVALID without a
 * pending filter submit (a pending submit of another kind stays pending). */
int rgrid_batch_filter_collect(rgrid_batch_t *b, int *status, int *counts, float *out_xy, long out_cap_points);

/* Points per cloud one workgroup of kgb_filter holds (8192: 8 B of voxel keys and two 4 B table slots per point in LDS). */
int rgrid_batch_filter_max_points(void);

/* ---- fleet texture: MapBuilder::ToSubmapTexture (map_builder.cc:128-134 -> ProbabilityGrid::DrawToSubmapTexture,
 * probability_grid.cc:86-131) for the resident slots of many robots, ONE launch and ONE synchronisation per call (kgb_texture, one
 * workgroup per named slot, csrc/rgrid_batch.hip).  The specification is the single call: for every named slot, box, slice_max and
 * the bytes are exactly what rgrid_draw_texture returns from an rgrid_t holding the same grid -- the box of the cells whose raw
 * value is not 0 as (offset_x, offset_y, width, height), (0, 0, 1, 1) and the one pair (0, 0) when there is none; two bytes
 * (value, alpha) per cell of the box, x fastest; slice_max = limits.max - resolution * (offset_y, offset_x).  The call only reads
 * the slots, which stay on the device.  The slots are named by a plain array of ints: a slot index is all a texture needs, a
 * record of one field would only make the caller pack what it already has.  The table of byte pairs is uploaded by the handle's
 * first texture submit; the output area (pinned host memory the kernel writes, 2 * num_x_cells * num_y_cells bytes per named slot)
 * and the box records are allocated by it too and grow only when a later call needs more: a steady-state call allocates nothing.
 * The ABI version stays 4: a caller that may meet an older library looks for these symbols. */

/* Enqueues the textures of slots grids[0 .. count) and returns without waiting.  Refused as a whole with RGRID_ERR_INVALID, nothing
 * launched and the handle still usable: a null b, a null grids with count > 0, count outside [0, max_scans], a slot out of range or
 * not yet set, a pending submit of any kind.  The same slot may be named more than once.  count == 0 is a submit with nothing
 * launched. */
int rgrid_batch_texture_submit(rgrid_batch_t *b, const int *grids, int count);

/* Waits once and hands out the pending texture submit's results in its order: boxes (4 * count), slice_max (2 * count), offsets
 * (count: the byte in `cells` where texture j starts) and the textures back to back in `cells`, 2 * width * height bytes each.
 * RGRID_ERR_BUFFER when cap is below their sum, or cells is NULL with a sum that is not 0: boxes, slice_max and offsets are filled
 * and the submit is LEFT PENDING, the caller comes again with room; cap = sum of 2 * num_x_cells * num_y_cells always suffices.
 * RGRID_ERR_INVALID without a pending texture submit (a pending submit of another kind stays pending). */
int rgrid_batch_texture_collect(rgrid_batch_t *b, int *boxes, double *slice_max, long *offsets, uint8_t *cells, long cap);

/* ---- occupancy grid and saved map: Node::PublishMap (src/ros_node.cc:845-863: ToSubmapTexture -> io::FillSubmapSlice ->
 * io::PaintSubmapSlices, src/io/submap_painter.cc:44-112 -> Node::CreateOccupancyGridMsg, ros_node.cc:897-945) and the image of
 * Node::HandleSaveMap (:947-1001, WritePgm :865-881) for the resident grid, without cairo.  The reference paints the texture onto a
 * background of red 128 through a transform that is a turn by 90 degrees and a translation; inside the domain below the painting is a
 * closed form (pinned against libcairo by tests/test_occupancy_cpu.py): the image has size = (height + 10, width + 10)
 * of the texture -- or 11 where the reference's float32 bounding box rounds up, the extra column or row at the far end -- texture pixel
 * (u, v) lies at image pixel (height + 4 - v, u + 5) with red = min(255, value + mul8(255 - alpha, 128)), everything else is background.
 * mode 0: the occupancy values in message order (nav_msgs::OccupancyGrid::data: image rows bottom-up; -1 where nothing was observed,
 * else RoundToInt((1. - red / 255.) * 100.)); mode 1: the red bytes in image order, the body of the PGM.  Another mode is
 * RGRID_ERR_INVALID.  size = (width, height) of the image, origin = info.origin.position = the YAML origin of the saved map
 * (-origin.x * resolution, (-height + origin.y) * resolution), box = the known-cells box as rgrid_draw_texture gives it.
 * submap_origin = the translation of the submap's local pose (the float origin cast to double, submap_2d.cc:18-24): the reference's
 * slice_pose is slice_max - submap_origin, and adding it back is not always slice_max.
 * Domain: both |translation / resolution| below 16384 pixels and both image sides at most 32767 (cairo's limit); outside it the call
 * is RGRID_ERR_CAPACITY with box filled and nothing else written.  out needs size[0] * size[1] bytes -- (num_x_cells + 11) *
 * (num_y_cells + 11) always suffices; RGRID_ERR_BUFFER reports size, origin and box.
 * The ABI version stays 4: a caller that may meet an older library looks for these symbols. */
int rgrid_occupancy_grid(rgrid_t *h, int mode, const double submap_origin[2], int8_t *out, long cap,
                         int size[2], double origin[2], int box[4]);

/* ---- fleet occupancy grid: the above for the resident slots of many robots, ONE launch and ONE synchronisation per call
 * (kgb_occupancy, one workgroup per named slot, csrc/rgrid_batch.hip).  The specification is the single call: for every named slot,
 * size, origin, box and the bytes are exactly what rgrid_occupancy_grid returns from an rgrid_t holding the same grid.  The kernel
 * finds the box, looks every cell of it up in the byte table of the call's mode and writes the turned block into pinned host memory;
 * collect puts the frame of background around it in the copy it makes anyway.  The call only reads the slots.  The two byte tables are
 * uploaded by the handle's first occupancy submit; the output area (num_x_cells * (num_y_cells rounded up to 16) bytes per named slot)
 * and the box records are allocated by it too and grow only when a later call needs more. */

/* Enqueues the occupancy grids (mode 0) or images (mode 1) of slots grids[0 .. count), submap_origins = 2 * count doubles, and returns
 * without waiting.  Refused as a whole with RGRID_ERR_INVALID, nothing launched and the handle still usable: what
 * rgrid_batch_texture_submit refuses, a null submap_origins with count > 0, another mode.  The same slot may be named more than once.
 * count == 0 is a submit with nothing launched. */
int rgrid_batch_occupancy_submit(rgrid_batch_t *b, int mode, const int *grids, const double *submap_origins, int count);

/* Waits once and hands out the pending occupancy submit's results in its order: status (count), sizes (2 * count), origins
 * (2 * count), boxes (4 * count), offsets (count: the byte in `out` where image j starts) and the images back to back in `out`,
 * sizes[2j] * sizes[2j + 1] bytes each.  A slot outside the domain has status RGRID_ERR_CAPACITY, size (0, 0), origin (0, 0) and no
 * bytes; its neighbours are unaffected.  RGRID_ERR_BUFFER when cap is below the sum, or out is NULL with a sum that is not 0: all but
 * the bytes is filled and the submit is LEFT PENDING, the caller comes again with room; cap = sum of (num_x_cells + 11) *
 * (num_y_cells + 11) always suffices.  RGRID_ERR_INVALID without a pending occupancy submit (a pending submit of another kind stays
 * pending). */
int rgrid_batch_occupancy_collect(rgrid_batch_t *b, int *status, int *sizes, double *origins, int *boxes,
                                  long *offsets, int8_t *out, long cap);

/* ---- fleet MapBuilder: mapping::MapBuilder::AddRangeData (src/mapping/map_builder.cc:57-108) for one scan of every robot in ONE
 * call, each robot in its own resident slot.  The specification is the single handle: robot j's status, local_pose, returns_in_local
 * and, after the call, its slot's cells and limits (rgrid_batch_get_grid / rgrid_batch_get_limits) are the bits an rgrid_t created
 * with the batch's max_points and max_cells (and max_candidates large enough) gives and holds after the same scans through
 * rgrid_add_range_data with the same options.  Nothing has a tolerance.
 * Stages: (1) kgb_filter rotates the raw returns and misses into the gravity-aligned frame ON THE DEVICE as it loads them -- per point
 * (c x - s y) + 0, (s x + c y) + 0 with the host's float (cos, sin) of the scan -- and filters them; (2) the host decides from the
 * counts; (3) kgb_match and kgb_refine, for the scans whose slot has a grid, on the adaptively filtered clouds where the filter wrote
 * them; (4) the host composes the poses (double cos / sin / atan2 of the host's libm: the device has no bit-identical ones, which is
 * why the call waits between its stages) and moves the filtered clouds into the insert's segment; (5) kgb_insert and kgb_to_local --
 * the RAW returns, still on the device from (1), through Rigid2f(pose_estimate.cast<float>()) into pinned host memory.  At most 5
 * kernel launches (6 with RGRID_BATCH_REDUCE_LAUNCH) and 3 stream synchronisations per call whatever count is;
 * rgrid_batch_last_call_counts reports both for the last call.  Not counted: a slot's creation is one hipMemsetAsync of 100 x 100 cells
 * on the handle's stream, and the handle's first call allocates its staging and uploads the insert's two lookup tables as the first
 * filter and insert submits do.
 * A slot that was never set is created as MapBuilder::CreateGrid creates it (:112-126: 100 x 100 unknown cells around the scan's origin
 * in local, resolution = opt->resolution, read only then -- an existing slot keeps its own), before growth: a scan whose growth fails
 * leaves the slot created.  Its scan is not matched, its estimate is the prediction.
 * Per scan: codes[j] = RGRID_OK or the first error of the scan's own stages, the other scans unaffected -- RGRID_ERR_CAPACITY (a cloud
 * above min(max_points, rgrid_batch_filter_max_points()); the match's or the insert's own capacity rules; creation with max_cells <
 * 10000), RGRID_ERR_INVALID (a non-finite raw coordinate: the single handle is not the reference for such a scan; creation with a
 * resolution not > 0).  status[j] = RGRID_SCAN_INSERTED, RGRID_SCAN_DROPPED_EMPTY or RGRID_SCAN_FILTERED_EMPTY with
 * rgrid_add_range_data's meaning; with a code it is never RGRID_SCAN_INSERTED.  local_poses (3 * count) = what rgrid_add_range_data
 * returns in local_pose, zero for a scan that did not get that far.  origins_in_local (2 * count) = the origin of range_data_in_local2
 * (the gravity-aligned origin through Embed3D(pose_estimate_2d.cast<float>())): for a scan that creates its slot, the submap's origin,
 * which rgrid_batch_occupancy_submit wants later.  returns_in_local (nullable, cap_points rows of room): scan j's n_returns rows at the
 * prefix sum of the n_returns before it; rows of scans that were not inserted are left untouched.
 * The whole call is RGRID_ERR_BUFFER, before anything is launched, when returns_in_local is given and cap_points is below the sum of
 * n_returns.  It is RGRID_ERR_INVALID, nothing launched and the handle still usable, for: a null b, opt, scans, codes, status,
 * local_poses or origins_in_local; count outside [0, max_scans]; a slot out of range; a negative point count or a null pointer with a
 * positive one; two scans naming one slot (rgrid_batch_insert_submit's rule); voxel_filter_size or adaptive_max_length not > 0, the
 * refinement options rgrid_refine_match refuses, a probability not strictly inside (0, 1); a pending submit of any kind.  The call is
 * synchronous: nothing is pending when it returns.  Coordinates whose voxel index no int holds are outside the contract.
 * The ABI version stays 4: a caller that may meet an older library looks for these symbols. */
typedef struct rgrid_batch_range_data {   /* 64 bytes on LP64 */
    int grid;                              /* the robot's resident slot; may be a slot that was never set */
    int n_returns, n_misses;
    const float *returns_xy, *misses_xy;   /* tracking frame, NULL when n == 0 */
    float origin_xy[2];
    double ekf_pose[3];                    /* x, y, yaw as the node builds it */
} rgrid_batch_range_data;

int rgrid_batch_add_range_data(rgrid_batch_t *b, const rgrid_map_builder_options *opt, const rgrid_batch_range_data *scans, int count,
                               int *codes, int *status, double *local_poses, float *origins_in_local, float *returns_in_local,
                               long cap_points);
int rgrid_batch_sizeof_range_data(void);

/* (kernel launches, stream synchronisations) of the handle's last rgrid_batch_add_range_data that was not refused as a whole;
 * (0, 0) before the first and after a call without scans. */
int rgrid_batch_last_call_counts(rgrid_batch_t *b, int launches_syncs[2]);

int rgrid_batch_sizeof_scan(void);
int rgrid_batch_sizeof_refine_scan(void);
int rgrid_batch_sizeof_insert_scan(void);
int rgrid_batch_sizeof_filter_scan(void);
const char *rgrid_batch_last_hip_error(rgrid_batch_t *b);

const char *rgrid_strerror(int code);
const char *rgrid_last_hip_error(rgrid_t *h);
int rgrid_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RGRID_H_ */
