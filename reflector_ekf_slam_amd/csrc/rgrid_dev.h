// rgrid_dev.h -- what the two correlative scan matchers share: rgrid.hip (one handle, one scan: kg_discretize, kg_score, kg_best)
// and rgrid_batch.hip (one scan of many robots, one launch: kgb_match).
//
// Host side, ONE text: what RealTimeCorrelativeScanMatcher2D::Match does before and after its candidate loop (plan_match,
// rotation_table, decode_best) and G_TRY, the status macro of both handles.  Each caller adds only its own capacity limits.
// Device side, two texts by measurement: BestRec, value_to_probability and rotation_cs are compiled by both files, but the
// discretisation's index formula and the first-maximum comparison are written out inside kg_discretize / kg_score / kg_best --
// calling them through the two functions below changed kg_score's instruction schedule -- and cell_index_of / best_before restate
// them for rgrid_batch.hip.  tests/test_fleet_match_gpu.py holds the two matchers together bit for bit.
// The two range-data inserters (rgrid_insert / rgrid_grow_as_needed and kgb_insert) share the text further down.
//
// The host steps AROUND the kernels are one text too, called by both handles: the checks and the refinement's launch shape (below
// G_TRY), insert_tables, the tables built on first use (resident_*), box_of_known / slice_max_of, and AddRangeData's compositions and
// CreateGrid's limits at the end of this file (tests/cpp/range_data_host.cpp drives them without a GPU).  rgrid.hip's voxel filter, by the
// same measurement as kg_score above: kg_keys and kg_keys_b call one body (voxel_keys: their instructions did not change), kg_first and
// kg_first_b stay two texts -- through a common body, with or without __restrict__, both came out with an operand pair swapped.
#pragma once
#include "../../include/rgrid.h"
#include "rgrid_refine_dev.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

// a failed HIP call: its text into the handle's (rgrid_t / rgrid_batch_t) hip_error, RGRID_ERR_HIP to the caller
#define G_TRY(h, expr)                                                              \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) {                                                     \
            if (h) (h)->hip_error = std::string(#expr) + ": " + hipGetErrorString(e_); \
            return RGRID_ERR_HIP;                                                   \
        }                                                                           \
    } while (0)

namespace {

// ---- what both handles refuse, ONE text (inline: a handle need not call every one); every comparison refuses a NaN option
inline bool two_clouds_ok(const float *ret, int n_ret, const float *mis, int n_mis) { return n_ret >= 0 && n_mis >= 0 && (n_ret == 0 || ret) && (n_mis == 0 || mis); }
inline bool refine_options_ok(const rgrid_refine_options *o) { return o->occupied_space_weight > 0. && o->translation_weight > 0. && o->rotation_weight > 0. && o->max_num_iterations >= 0; }
inline bool insert_options_ok(float hit, float miss) { return hit > 0.f && hit < 1.f && miss > 0.f && miss < 1.f; }
inline bool filter_options_ok(const rgrid_filter_options *o) { return o->voxel_filter_size > 0.f && o->adaptive_max_length > 0.; }
// ---- the refinement's launch shape: RefineArgs without the poses, and the thread count: no idle waves in the barriers and the sums
void refine_args(RefineArgs &A, int nx, int ny, double resolution, double max_x, double max_y, const rgrid_refine_options *opt, int n)
{
    std::memset(&A, 0, sizeof(A));
    A.nx = nx; A.ny = ny; A.n = n; A.max_iter = opt->max_num_iterations; A.max_nonmono = opt->use_nonmonotonic_steps ? 5 : 0;
    A.res = resolution; A.max_x = max_x; A.max_y = max_y;
    A.w_occ = opt->occupied_space_weight; A.w_t = opt->translation_weight; A.w_r = opt->rotation_weight;
}
int refine_threads(int n) { const int t = ((n + 63) / 64) * 64; return t < 1024 ? t : 1024; }

struct BestRec { float score; int id; };

__device__ static inline float value_to_probability(unsigned v16)
{
#pragma clang fp contract(off)
    // probability_values.cc:11-20 (the table entry, recomputed: same two float operations), probability_values.h:53-57
    const float kMinProbability = 0.1f, kMaxProbability = 1.f - kMinProbability;
    const float lower = 1.f - kMaxProbability, upper = 1.f - kMinProbability;
    const unsigned v = v16 & 32767u;
    float cost = upper;
    if (v != 0) {
        const float kScale = (upper - lower) / (32768 - 2.f);
        cost = (float)v * kScale + (lower - kScale);
    }
    return 1.f - cost;
}

// MapLimits::GetCellIndex (map_limits.h:47-55): (x index from y, y index from x), double arithmetic, lround (= kg_discretize)
__device__ static inline int2 cell_index_of(double max_x, double max_y, double resolution, float px, float py)
{
#pragma clang fp contract(off)
    return make_int2((int)lround((max_y - (double)py) / resolution - 0.5),
                     (int)lround((max_x - (double)px) / resolution - 0.5));
}

// first maximum of std::max_element in the reference's candidate order: a higher score wins, at equal score the smaller id
// (= kg_score / kg_best)
__device__ static inline bool best_before(float os, int oi, float best, int bid)
{
    return os > best || (os == best && oi < bid);
}

// Project2D(Rigid3f::Rotation(AngleAxisf(angle, UnitZ))) as a (cos, sin) pair, restating Eigen 3.3 in float32:
// Quaternionf(AngleAxisf) = (cos(a/2), 0, 0, sin(a/2)); GetYaw (transform.h:27-33) = atan2 of q * UnitX with
// Eigen's  v + w*uv + vec x uv,  uv = 2 (vec x v); Rotation2Df(yaw) rotates with (cos yaw, sin yaw).  Host libm.
void rotation_cs(float angle, float *c, float *s)
{
#pragma clang fp contract(off)
    const float ha = 0.5f * angle;
    const float w = std::cos(ha), z = std::sin(ha);
    const float uvy = z + z;
    const float dx = (1.f + w * 0.f) + (0.f * 0.f - z * uvy);
    const float dy = (0.f + w * uvy) + (z * 0.f - 0.f * 0.f);
    const float yaw = std::atan2(dy, dx);
    *c = std::cos(yaw); *s = std::sin(yaw);
}

// SearchParameters of one Match (correlative_scan_matcher_2d.cc:10-40) and the resolution they were made for
struct MatchPlan {
    double res, step;
    int num_angular, num_scans, num_linear;
    long long ncand;
};

// What Match does before its candidate loop: the n points rotated by the initial rotation into rotated_out (2 n floats) and the
// search parameters.  RGRID_ERR_CAPACITY (plan untouched) for a window whose counts are negative or NaN, or give more candidates
// than an int holds (candidate ids are ints): checked as doubles, before any conversion.
int plan_match(const rgrid_match_options *opt, double res, const double initial_pose[3], const float *points_xy, int n,
               float *rotated_out, MatchPlan *plan)
{
#pragma clang fp contract(off)
    // initial rotation of the cloud (real_time_correlative_scan_matcher_2d.cc:91-97), host float32
    float c0, s0;
    rotation_cs((float)initial_pose[2], &c0, &s0);
    float max_scan_range = 3.f * (float)res;                                             // correlative_scan_matcher_2d.cc:18-24
    for (int i = 0; i < n; ++i) {
        const float x = points_xy[2 * i], y = points_xy[2 * i + 1];
        const float rx = c0 * x - s0 * y, ry = s0 * x + c0 * y;
        rotated_out[2 * i] = rx; rotated_out[2 * i + 1] = ry;
        const float range = std::sqrt(rx * rx + ry * ry);
        if (range > max_scan_range) max_scan_range = range;
    }
    const double kSafetyMargin = 1. - 1e-3;
    const double step = kSafetyMargin * std::acos(1. - (res * res) / (2. * (double)(max_scan_range * max_scan_range)));   // :25-28
    const double num_angular_d = std::ceil(opt->angular_search_window / step);           // :29-31
    const double num_linear_d = std::ceil(opt->linear_search_window / res);              // :33-34
    const double W_d = 2. * num_linear_d + 1.;
    if (!(num_angular_d >= 0. && num_linear_d >= 0. && (2. * num_angular_d + 1.) * W_d * W_d <= 2147483647.)) return RGRID_ERR_CAPACITY;
    plan->res = res; plan->step = step;
    plan->num_angular = (int)num_angular_d; plan->num_scans = 2 * plan->num_angular + 1; plan->num_linear = (int)num_linear_d;
    const long long W = 2LL * plan->num_linear + 1;
    plan->ncand = (long long)plan->num_scans * W * W;
    return RGRID_OK;
}

// GenerateRotatedScans' rotations (:90-94) as num_scans (cos, sin) pairs: delta_theta accumulated in double, evaluated in float32
void rotation_table(const MatchPlan &plan, float *cs_out)
{
#pragma clang fp contract(off)
    double delta_theta = -plan.num_angular * plan.step;
    for (int s = 0; s < plan.num_scans; ++s, delta_theta += plan.step) rotation_cs((float)delta_theta, &cs_out[2 * s], &cs_out[2 * s + 1]);
}

// The winning candidate id -> sxy = (scan, x offset, y offset) -> the pose estimate (:106-110).  Integer division, int -> double,
// one multiply and one add per component, no libm: the host (decode_best) and the device (kgb_refine, which starts the refinement
// from the match's winner without a host round trip) get the same bits from this one text.
__host__ __device__ static inline void decode_candidate(int num_linear, int num_angular, double res, double step, const double initial_pose[3],
                                                        int id, int sxy[3], double pose_estimate[3])
{
#pragma clang fp contract(off)
    const int W = 2 * num_linear + 1;
    const int scan = id / (W * W), r = id - scan * (W * W);
    const int xo = r / W - num_linear, yo = r - (r / W) * W - num_linear;
    const double x = -yo * res, y = -xo * res, orientation = (scan - num_angular) * step;
    pose_estimate[0] = initial_pose[0] + x;
    pose_estimate[1] = initial_pose[1] + y;
    pose_estimate[2] = initial_pose[2] + orientation;
    sxy[0] = scan; sxy[1] = xo; sxy[2] = yo;
}

// What Match does after its candidate loop (:106-110); best3 and info3 may be null
void decode_best(const MatchPlan &plan, const double initial_pose[3], const BestRec &best, double pose_estimate[3], double *score, int *best3, int *info3)
{
    int sxy[3];
    decode_candidate(plan.num_linear, plan.num_angular, plan.res, plan.step, initial_pose, best.id, sxy, pose_estimate);
    *score = (double)best.score;
    if (best3) { best3[0] = sxy[0]; best3[1] = sxy[1]; best3[2] = sxy[2]; }
    if (info3) { info3[0] = plan.num_scans; info3[1] = plan.num_linear; info3[2] = (int)plan.ncand; }
}

// ---- range-data inserter: what rgrid_insert / rgrid_grow_as_needed (rgrid.hip) and rgrid_batch_insert_submit (rgrid_batch.hip)
// share.  Host side, ONE text: the lookup tables and GrowAsNeeded's decision.  Device side: the record of one insertion, the table
// application and the superscaled cell index (kg_ends, kg_hits, kg_rays and kgb_insert call the same three texts; the ray walk is
// kg_rays' own and restated in kgb_insert).
//
// ApplyLookupTable (probability_grid.cc:38-53): a cell without the update marker takes table[cell] (which carries the
// marker).  Concurrent lanes may race on one cell, but within a phase (hits, then misses: separate launches, or one workgroup's
// barrier between them) every writer stores the SAME value table[original], and a reader sees either the original or the marked
// value: the plain 16-bit load/store pair gives the reference's result without atomics.
struct InsertArgs {
    int nx, ny, n_ret, n_miss;
    double max_x, max_y, rs;           // rs = resolution / 1000 (superscaled limits, :48-53)
    float ox, oy;
};
constexpr int SUBPX = 1000;
constexpr unsigned MARKER = 32768u;

__device__ static inline void apply_table(unsigned short *cells, int nx, int cx, int cy, const unsigned short *__restrict__ table)
{
    unsigned short *c = cells + (size_t)nx * cy + cx;
    const unsigned short v = *c;
    if (v < MARKER) *c = table[v];
}
__device__ static inline bool super_index(const InsertArgs &A, float px, float py, int &ix, int &iy)
{
    // superscaled MapLimits::GetCellIndex (map_limits.h:47-55): x index from y, y index from x
    ix = (int)lround((A.max_y - (double)py) / A.rs - 0.5);
    iy = (int)lround((A.max_x - (double)px) / A.rs - 0.5);
    return ix >= 0 && iy >= 0 && (long long)ix < (long long)A.nx * SUBPX && (long long)iy < (long long)A.ny * SUBPX;
}

// ComputeLookupTableToApplyCorrespondenceCostOdds(Odds(probability)) (probability_values.cc:76-96), host float32
void lookup_table(float probability, unsigned short *table)
{
#pragma clang fp contract(off)
    const float kMinProbability = 0.1f, kMaxProbability = 1.f - kMinProbability;
    const float lower = 1.f - kMaxProbability, upper = 1.f - kMinProbability;
    auto cost_to_value = [&](float c) -> unsigned short {                        // BoundedFloatToValue (probability_values.h:15-29)
        float cl = c;
        if (cl > upper) cl = upper;
        if (cl < lower) cl = lower;
        return (unsigned short)((int)std::lround((cl - lower) * (32766.f / (upper - lower))) + 1);
    };
    const float odds = probability / (1.f - probability);
    {
        const float p = odds / (odds + 1.f);
        table[0] = (unsigned short)(cost_to_value(1.f - p) + MARKER);
    }
    const float kScale = (upper - lower) / (32768 - 2.f);
    for (int cell = 1; cell != 32768; ++cell) {
        const float cost = cell * kScale + (lower - kScale);                     // kValueToCorrespondenceCost[cell]
        const float pc = 1.f - cost;
        const float o = odds * (pc / (1.f - pc));
        const float p = o / (o + 1.f);
        table[cell] = (unsigned short)(cost_to_value(1.f - p) + MARKER);
    }
}

// A table on the device from the host's: allocates when d_table is null, uploads, and only then publishes the pointer -- a failed upload
// frees what it allocated, so a table that is built on first use is built again by the next call
template <typename T>
hipError_t upload_table(T *&d_table, const T *table, size_t n)
{
    T *d = d_table;
    hipError_t e = d ? hipSuccess : hipMalloc((void **)&d, sizeof(T) * n);
    if (e == hipSuccess && (e = hipMemcpy(d, table, sizeof(T) * n, hipMemcpyHostToDevice)) == hipSuccess) d_table = d;
    else if (d != d_table) (void)hipFree(d);
    return e;
}
// The inserter's two resident tables (uint16[32768] each, allocated with the handle) for a (hit, miss) pair.  They only depend on the two
// options: tab_hit_p / tab_miss_p remember the pair they hold and change only after BOTH uploads succeeded.
hipError_t insert_tables(float hit, float miss, unsigned short *d_hit, unsigned short *d_miss, float &tab_hit_p, float &tab_miss_p)
{
    if (!(hit != tab_hit_p || miss != tab_miss_p)) return hipSuccess;
    std::vector<unsigned short> t(32768);
    lookup_table(hit, t.data());
    hipError_t e = upload_table(d_hit, t.data(), t.size());
    if (e != hipSuccess) return e;
    lookup_table(miss, t.data());
    if ((e = upload_table(d_miss, t.data(), t.size())) == hipSuccess) { tab_hit_p = hit; tab_miss_p = miss; }
    return e;
}

// (value, alpha) of every cell value: 128 - ProbabilityToLogOddsInteger(GetProbability) (probability_grid.cc:97-114,
// submaps.h:22-41), host float32 with the same libm a CPU build uses; entry = value | alpha << 8
void texture_table(unsigned short *table)
{
#pragma clang fp contract(off)
    const float kMinP = 0.1f, kMaxP = 1.f - kMinP;
    const float kMaxLogOdds = std::log(kMaxP / (1.f - kMaxP)), kMinLogOdds = std::log(kMinP / (1.f - kMinP));
    const float lower = 1.f - kMaxP, upper = 1.f - kMinP, kScale = (upper - lower) / (32768 - 2.f);
    table[0] = 0;                                                                // unknown: (0, 0)
    for (int v = 1; v < 32768; ++v) {
        const float cost = (float)v * kScale + (lower - kScale);
        const float p = 1.f - cost;
        const float logit = std::log(p / (1.f - p));
        const int li = (int)std::lround((logit - kMinLogOdds) * 254.f / (kMaxLogOdds - kMinLogOdds)) + 1;
        const int delta = 128 - li;
        const unsigned alpha = (unsigned)(delta > 0 ? 0 : -delta) & 255u, value = (unsigned)(delta > 0 ? delta : 0) & 255u;
        table[v] = (unsigned short)(value | ((value || alpha) ? alpha : 1u) << 8);
    }
}
hipError_t resident_texture_table(unsigned short *&d_table)
{
    if (d_table) return hipSuccess;
    std::vector<unsigned short> t(32768);
    texture_table(t.data());
    return upload_table(d_table, t.data(), t.size());
}

// ---- occupancy grid and saved map: what rgrid_occupancy_grid (rgrid.hip) and rgrid_batch_occupancy_* (rgrid_batch.hip) share.
// The reference paints the submap texture with cairo (io::PaintSubmapSlices, src/io/submap_painter.cc:44-91) and reads the
// painting back as nav_msgs::OccupancyGrid (Node::CreateOccupancyGridMsg, src/ros_node.cc:897-945) or as a PGM (Node::WritePgm,
// :865-881).  The painting is the texture turned by 90 degrees inside a frame of background: texture pixel (u, v)
// of a w x h texture lands at image pixel (h + 4 - v, u + 5).  Host side, ONE text: the two byte tables, the image's size and origin
// (cairo's matrix arithmetic and Eigen's float32 box, replayed) and the copy of the device's rows into the frame.  Device side,
// ONE text: the interior block, w rows of h bytes, row u column h - 1 - v = table[cell (x0 + u, y0 + v)].

// The two byte tables, composed from texture_table: cairo's OVER of the premultiplied pixel (alpha, value, observed, 0) onto the
// background (255, 128, 0, 0) leaves red = min(255, value + mul8(255 - alpha, 128)) with pixman's mul8; occupancy is -1 where
// nothing was observed, else RoundToInt((1. - red / 255.) * 100.).
void occupancy_tables(signed char *occupancy, unsigned char *red)
{
#pragma clang fp contract(off)
    std::vector<unsigned short> tex(32768);
    texture_table(tex.data());
    for (int v = 0; v < 32768; ++v) {
        const unsigned value = tex[(size_t)v] & 255u, alpha = tex[(size_t)v] >> 8;
        const unsigned t = (255u - alpha) * 128u + 128u;
        const unsigned over = value + ((t + (t >> 8)) >> 8);
        red[v] = (unsigned char)(over > 255u ? 255u : over);
        occupancy[v] = (value == 0u && alpha == 0u) ? (signed char)-1 : (signed char)std::lround((1. - red[v] / 255.) * 100.);
    }
}
hipError_t resident_occupancy_tables(unsigned char *&d_tables)                     // occupancy, then red: 2 * 32768 bytes
{
    if (d_tables) return hipSuccess;
    std::vector<unsigned char> t(2 * 32768);
    occupancy_tables(reinterpret_cast<signed char *>(t.data()), t.data() + 32768);
    return upload_table(d_tables, t.data(), t.size());
}

// Grid2D::ComputeCroppedLimits' box (offset_x, offset_y, width, height) (grid_2d.cc:36-48) from the known cells' (min x, min y, max x,
// max y) as kg_known_box leaves them; nothing known (max x < 0): offset 0, CellLimits(1, 1) (:39-44)
inline void box_of_known(const int known[4], int box[4])
{
    const bool any = known[2] >= 0;
    box[0] = any ? known[0] : 0; box[1] = any ? known[1] : 0; box[2] = any ? known[2] - known[0] + 1 : 1; box[3] = any ? known[3] - known[1] + 1 : 1;
}
// limits.max - resolution * (offset_y, offset_x): the translation of SubmapTexture::slice_pose (probability_grid.cc:122-123)
inline void slice_max_of(const int box[4], double resolution, double max_x, double max_y, double slice_max[2])
{
#pragma clang fp contract(off)
    slice_max[0] = max_x - resolution * box[1]; slice_max[1] = max_y - resolution * box[0];
}

// cairo_matrix_t and cairo_matrix_multiply(r, a, b) as cairo 1.16 writes them out: every cairo_scale / cairo_transform call
// replaces the CTM by (new matrix) * CTM
struct CairoMatrix { double xx, yx, xy, yy, x0, y0; };
CairoMatrix cairo_multiply(const CairoMatrix &a, const CairoMatrix &b)
{
#pragma clang fp contract(off)
    CairoMatrix r;
    r.xx = a.xx * b.xx + a.yx * b.xy;
    r.yx = a.xx * b.yx + a.yx * b.yy;
    r.xy = a.xy * b.xx + a.yy * b.xy;
    r.yy = a.xy * b.yx + a.yy * b.yy;
    r.x0 = a.x0 * b.xx + a.y0 * b.xy + b.x0;
    r.y0 = a.x0 * b.yx + a.y0 * b.yy + b.y0;
    return r;
}

// What the host knows of one painted texture
struct OccupancyFrame {
    int size[2];          // the image: width, height
    double origin[2];     // OccupancyGrid::info.origin.position = the saved map's YAML origin
};

enum { OCC_MODE_OCCUPANCY = 0, OCC_MODE_IMAGE = 1 };

// PaintSubmapSlices' first pass (submap_painter.cc:48-73) and the origin of CreateOccupancyGridMsg (ros_node.cc:914-917) for the
// texture of box (offset_x, offset_y, width, height) of a grid with the given limits, in a submap whose local pose has translation
// submap_origin.  RGRID_ERR_CAPACITY outside the domain in which the painting is the closed form above: the translation at or beyond
// 16384 pixels (a float32 ulp of the corner coordinates above 1/1024 pixel) or an image side above cairo's 32767.
int occupancy_frame(const int box[4], double resolution, double max_x, double max_y, const double submap_origin[2], OccupancyFrame *out)
{
#pragma clang fp contract(off)
    const double r = resolution;
    // slice_pose = local_pose^-1 * Translation(slice_max) (probability_grid.cc:122-126), submap.pose * submap.slice_pose puts it back
    double slice_max[2];
    slice_max_of(box, r, max_x, max_y, slice_max);
    const double t[2] = {(slice_max[0] - submap_origin[0]) + submap_origin[0], (slice_max[1] - submap_origin[1]) + submap_origin[1]};
    if (!(std::fabs(t[0] / r) < 16384.) || !(std::fabs(t[1] / r) < 16384.)) return RGRID_ERR_CAPACITY;
    CairoMatrix ctm = {1., 0., 0., 1., 0., 0.};
    ctm = cairo_multiply(CairoMatrix{1. / r, 0., 0., 1. / r, 0., 0.}, ctm);        // cairo_scale(1 / resolution)
    ctm = cairo_multiply(CairoMatrix{0., 1., -1., -0., t[0], -t[1]}, ctm);         // cairo_transform(homo(1,0), homo(0,0), -homo(1,1), -homo(0,1), ...)
    ctm = cairo_multiply(CairoMatrix{r, 0., 0., r, 0., 0.}, ctm);                  // cairo_scale(submap_resolution)
    float lo[2] = {0.f, 0.f}, hi[2] = {0.f, 0.f};
    for (int c = 0; c < 4; ++c) {                                                  // Eigen::AlignedBox2f::extend of the four corners
        const double x = (c & 1) ? (double)box[2] : 0., y = (c & 2) ? (double)box[3] : 0.;
        const double dx = ctm.xx * x + ctm.xy * y, dy = ctm.yx * x + ctm.yy * y;   // cairo_matrix_transform_distance ...
        const float p[2] = {(float)(dx + ctm.x0), (float)(dy + ctm.y0)};           // ... + the translation, then Vector2f(x, y)
        for (int a = 0; a < 2; ++a) {
            if (c == 0 || p[a] < lo[a]) lo[a] = p[a];
            if (c == 0 || p[a] > hi[a]) hi[a] = p[a];
        }
    }
    float org[2];
    for (int a = 0; a < 2; ++a) {
        const float extent = hi[a] - lo[a];
        const double side = std::ceil(extent) + 10;                                // ceil(sizes()) + 2 * kPaddingPixel
        if (!(side <= 32767.)) return RGRID_ERR_CAPACITY;
        out->size[a] = (int)side;
        org[a] = -lo[a] + 5.f;
    }
    out->origin[0] = (double)(-org[0]) * r;
    out->origin[1] = (double)((float)(-out->size[1]) + org[1]) * r;                // int + float: a float32 sum
    return RGRID_OK;
}

// Bytes between two rows of the interior block as the device writes it: rows start 16-byte aligned
__host__ __device__ static inline int occupancy_stride(int h) { return (h + 15) & ~15; }
// ... and what a grid of nx x ny cells needs at most for it (any box inside it)
size_t occupancy_block_bytes(int nx, int ny) { return (size_t)nx * (size_t)occupancy_stride(ny); }

// The image from the block: background everywhere (-1, or red 128), then row u of the block at image row u + 5, columns 5 .. h + 4;
// the occupancy message lists the image's rows bottom-up (ros_node.cc:927).  A quirk row or column (size = side + 11) lies at the
// far end and keeps the background.
void occupancy_paint(int mode, const unsigned char *block, int w, int h, const int size[2], unsigned char *out)
{
    const size_t W = (size_t)size[0], H = (size_t)size[1];
    std::memset(out, mode == OCC_MODE_OCCUPANCY ? 0xff : 128, W * H);
    const size_t stride = (size_t)occupancy_stride(h);
    for (int u = 0; u < w; ++u) {
        const size_t Y = (size_t)u + 5, row = mode == OCC_MODE_OCCUPANCY ? H - 1 - Y : Y;
        std::memcpy(out + row * W + 5, block + stride * (size_t)u, (size_t)h);
    }
}

// The known-cells box of one slot, by one workgroup of KGT_THREADS threads (kgb_texture's and kgb_occupancy's phase 1): the slot is
// walked as ONE array of n = nx * ny cells -- the cells in front of the first 16-byte boundary and behind the last one singly, the
// eight-cell vectors between them whole.  Per-thread min / max, wave shuffles, LDS (s_box) across the waves; ends behind a barrier
// with the box in every thread, wave-uniform: (0, 0, 1, 1) when no cell is known (grid_2d.cc:39-44).
#define KGT_THREADS 512
#define KGT_WAVES (KGT_THREADS / 64)
#define KGT_PF 4                          // 16-byte vectors of cells a thread has in flight in phase 1
__device__ static inline void known_box_of_slot(const unsigned short *__restrict__ cells, int nx, int n, int (*s_box)[4], int &bx0, int &by0,
                                                int &bw, int &bh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the columns [x0, x1] and the linear indices [k0, k1] the known cells span; the rows follow from k0 and k1
    int x0 = 0x7fffffff, x1 = -1, k0 = 0x7fffffff, k1 = -1;
    auto see = [&](int k, int x) { x0 = min(x0, x); x1 = max(x1, x); k0 = min(k0, k); k1 = max(k1, k); };
    const int to_boundary = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(cells) & 15u)) & 15u) >> 1);
    const int head = min(n, to_boundary), nvec = (n - head) >> 3, tail = head + 8 * nvec;
    for (int k = tid; k < head; k += KGT_THREADS)
        if (cells[k] != 0) see(k, k % nx);
    for (int k = tail + tid; k < n; k += KGT_THREADS)
        if (cells[k] != 0) see(k, k % nx);
    const uint4 *__restrict__ vec = reinterpret_cast<const uint4 *>(cells + head);
    for (int v0 = 0; v0 < nvec; v0 += KGT_THREADS * KGT_PF) {
        uint4 q[KGT_PF];
#pragma unroll
        for (int u = 0; u < KGT_PF; ++u) {
            const int v = v0 + u * KGT_THREADS + tid;
            q[u] = v < nvec ? vec[v] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < KGT_PF; ++u) {
            if ((q[u].x | q[u].y | q[u].z | q[u].w) == 0u) continue;                // eight unknown cells (or none at all)
            const unsigned w32[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
            const int k = head + 8 * (v0 + u * KGT_THREADS + tid);
            int x = k % nx;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (((w32[c >> 1] >> (16 * (c & 1))) & 0xffffu) != 0u) see(k + c, x);
                if (++x == nx) x = 0;                                              // the vector runs on into the next row
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64)); x1 = max(x1, __shfl_xor(x1, off, 64));
        k0 = min(k0, __shfl_xor(k0, off, 64)); k1 = max(k1, __shfl_xor(k1, off, 64));
    }
    if (lane == 0) { s_box[wave][0] = x0; s_box[wave][1] = x1; s_box[wave][2] = k0; s_box[wave][3] = k1; }
    __syncthreads();
    for (int w = 0; w < KGT_WAVES; ++w) {
        x0 = min(x0, s_box[w][0]); x1 = max(x1, s_box[w][1]); k0 = min(k0, s_box[w][2]); k1 = max(k1, s_box[w][3]);
    }
    int y0 = 0, y1 = 0;
    if (x1 < 0) { x0 = 0; x1 = 0; }                                                // nothing known: offset 0, CellLimits(1, 1) (grid_2d.cc:39-44)
    else { y0 = k0 / nx; y1 = k1 / nx; }
    bx0 = __builtin_amdgcn_readfirstlane(x0); by0 = __builtin_amdgcn_readfirstlane(y0);
    bw = __builtin_amdgcn_readfirstlane(x1 - x0 + 1); bh = __builtin_amdgcn_readfirstlane(y1 - y0 + 1);
}

// The interior block of the image, a transposition with a column flip, through LDS tiles of OCC_T x OCC_T bytes so that both
// global sides run along memory: a wave reads 64 consecutive cells of one grid row (128 B), looks each up in the byte table and
// writes the bytes down one tile COLUMN; behind the barrier a lane takes 16 consecutive bytes of one tile ROW and stores them as one
// aligned 16-byte vector, four lanes per 64-byte row segment.  Tile rows are OCC_PITCH = 72 bytes apart: the byte stores of a wave go
// to dwords 18 apart, so the 64 lanes fall on 32 different dwords' banks, two lanes each (lanes l and l + 32 when the dword address
// is taken mod 64, l and l + 16 when it is taken mod 32 as the guide gives it for stores): never more than a 2-way conflict, which a
// store does not pay for -- and a row's 16 bytes are two aligned 8-byte loads.  The store phase has work for OCC_T * 4 = 256 threads:
// in kgb_occupancy's workgroup of 512 four waves wait at the barrier meanwhile (a wider store side was not tried, no number).  Tiles are laid over the OUTPUT (u0, c0 multiples of 64), so every vector store is aligned whatever h is; columns
// h .. stride - 1 of a row are padding and get 0.  The workgroup (any multiple of 64 threads) takes tiles first, first + step, ...
#define OCC_T 64
#define OCC_PITCH 72
__device__ static inline void occupancy_tiles(const unsigned short *__restrict__ cells, int nx, int x0, int y0, int w, int h,
                                              const unsigned char *__restrict__ table, unsigned char *__restrict__ out,
                                              unsigned char (*tile)[OCC_PITCH], int first, int step)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int stride = occupancy_stride(h);
    const int tiles_u = (w + OCC_T - 1) / OCC_T, tiles_c = (stride + OCC_T - 1) / OCC_T;
    for (int t = first; t < tiles_u * tiles_c; t += step) {
        const int u0 = OCC_T * (t % tiles_u), c0 = OCC_T * (t / tiles_u);          // u fastest: neighbouring tiles read on along the grid's rows
        const int u = u0 + lane;
        for (int r = wave; r < OCC_T; r += waves) {
            const int v = h - 1 - (c0 + r);                                        // the column flip
            unsigned char byte = 0;
            if (v >= 0 && u < w) byte = table[cells[(size_t)nx * (size_t)(y0 + v) + (size_t)(x0 + u)] & 32767u];
            tile[lane][r] = byte;
        }
        __syncthreads();
        for (int q = tid; q < OCC_T * (OCC_T / 16); q += blockDim.x) {
            const int ul = q >> 2, c = c0 + 16 * (q & 3);
            if (u0 + ul < w && c < stride) {
                const uint2 *src = reinterpret_cast<const uint2 *>(&tile[ul][16 * (q & 3)]);
                const uint2 a = src[0], b = src[1];
                *reinterpret_cast<uint4 *>(out + (size_t)stride * (size_t)(u0 + ul) + (size_t)c) = make_uint4(a.x, a.y, b.x, b.y);
            }
        }
        __syncthreads();
    }
}

// Grid2D::GrowLimits(point) on the limits only (grid_2d.cc:64-75,93); false if the grown grid exceeds `max_cells`
bool grow_limits_for(float px, float py, double res, long long max_cells, int &nx, int &ny, double &max_x, double &max_y, int &off_x, int &off_y)
{
#pragma clang fp contract(off)
    for (;;) {
        const long ix = std::lround((max_y - (double)py) / res - 0.5), iy = std::lround((max_x - (double)px) / res - 0.5);
        if (ix >= 0 && iy >= 0 && ix < nx && iy < ny) return true;
        if (4ll * nx * ny > max_cells) return false;
        const int xo = nx / 2, yo = ny / 2;
        max_x = max_x + res * (double)yo;
        max_y = max_y + res * (double)xo;
        nx *= 2; ny *= 2; off_x += xo; off_y += yo;
    }
}

// The limits of a grid after GrowAsNeeded (probability_grid_range_data_inserter_2d.cc:20-38): nx, ny, max_x, max_y go in as the
// grid has them and come out grown, (off_x, off_y) is where the old cell (0, 0) lies in the grown grid -- several doublings are one
// move.  RGRID_ERR_INVALID for a non-finite coordinate (the reference would loop forever), RGRID_ERR_CAPACITY when the grown grid
// would exceed max_cells; the limits are untouched then.
int plan_growth(const float origin_xy[2], const float *returns_xy, int n_returns, const float *misses_xy, int n_misses, double res,
                long long max_cells, int &nx, int &ny, double &max_x, double &max_y, int &off_x, int &off_y)
{
    // Eigen::AlignedBox2f(origin).extend(every return and miss)  (:23-33)
    float lo[2] = {origin_xy[0], origin_xy[1]}, hi[2] = {origin_xy[0], origin_xy[1]};
    auto extend = [&](const float *p, int n) {
        for (int i = 0; i < 2 * n; ++i) {
            const float v = p[i];
            if (!std::isfinite(v)) return false;
            if (v < lo[i & 1]) lo[i & 1] = v;
            if (v > hi[i & 1]) hi[i & 1] = v;
        }
        return true;
    };
    if (!std::isfinite(lo[0]) || !std::isfinite(lo[1]) || !extend(returns_xy, n_returns) || !extend(misses_xy, n_misses)) return RGRID_ERR_INVALID;
    const float pad = 1e-6f;                                                        // kPadding (:25)
    int gnx = nx, gny = ny, gox = 0, goy = 0;
    double gmx = max_x, gmy = max_y;
    if (!grow_limits_for(lo[0] - pad, lo[1] - pad, res, max_cells, gnx, gny, gmx, gmy, gox, goy) ||
        !grow_limits_for(hi[0] + pad, hi[1] + pad, res, max_cells, gnx, gny, gmx, gmy, gox, goy))
        return RGRID_ERR_CAPACITY;
    nx = gnx; ny = gny; max_x = gmx; max_y = gmy; off_x = gox; off_y = goy;
    return RGRID_OK;
}

// ---- MapBuilder::AddRangeData's rigid transforms: what rgrid_add_range_data (rgrid.hip) and rgrid_batch_add_range_data
// (rgrid_batch.hip) share.  Host side, ONE text: the reference's float32 round trips through Eigen quaternions restated operation by
// operation (as in reflector_ekf_slam_amd/map_builder.py), host libm in double.  Device side: kgb_filter<true> and kgb_to_local apply
// rigid2f_apply's per-point line with the (cos, sin) pair rigid2f_cs gives the host.
float yaw_of_quaternion_f32(float w, float z)          // transform::GetYaw(Quaternionf(w,0,0,z)): q * UnitX = (1 - z 2z, w 2z, 0)
{
#pragma clang fp contract(off)
    const float two_z = z + z;
    const float y = w * two_z, x = 1.f - z * two_z;
    return (float)std::atan2((double)y, (double)x);
}
double yaw_of_quaternion_f64(double w, double z)
{
#pragma clang fp contract(off)
    const double two_z = z + z;
    return std::atan2(w * two_z, 1.0 - z * two_z);
}
void rigid2f_cs(float yaw, float *c, float *s)          // Rotation2Df(yaw)'s matrix entries
{
    *c = (float)std::cos((double)yaw); *s = (float)std::sin((double)yaw);
}
// one point through Rigid2f(t, Rotation2Df): the line the device restates, host and device from this one text
__host__ __device__ static inline void rigid2f_point(float c, float s, float tx, float ty, float x, float y, float &ox, float &oy)
{
#pragma clang fp contract(off)
    ox = (c * x - s * y) + tx;
    oy = (s * x + c * y) + ty;
}
void rigid2f_apply(float tx, float ty, float yaw, const float *in, int n, float *out)   // Rigid2f(t, Rotation2Df(yaw)) * p
{
    float c, s;
    rigid2f_cs(yaw, &c, &s);
    for (int i = 0; i < n; ++i) rigid2f_point(c, s, tx, ty, in[2 * i], in[2 * i + 1], out[2 * i], out[2 * i + 1]);
}

// the caller's quaternion of an EKF yaw (src/ros_node.cc:548) and the gravity alignment's yaw (map_builder.cc:20-28): Rotation(q)
// .cast<float>() -> Project2D -> GetYaw
void gravity_alignment(double theta, double &qw, double &qz, float &yaw_g)
{
    qw = std::cos(theta / 2); qz = std::sin(theta / 2);
    yaw_g = yaw_of_quaternion_f32((float)qw, (float)qz);
}
// What AddRangeData makes of ScanMatch's answer est (map_builder.cc:86-94).  pose_estimate = Embed3D(est) * gravity_alignment, a
// quaternion product about z in double: local_pose is its projection, yaw_f32 the yaw of pose_estimate.cast<float>() (the raw returns);
// yaw2 is the yaw of Embed3D(est.cast<float>()) (the filtered data): AngleAxisf -> Quaternionf, cos / sin of the float32 half angle.
void compose_pose_estimate(const double est[3], double qw, double qz, double local_pose[3], float &yaw_f32, float &yaw2)
{
#pragma clang fp contract(off)
    const double aw = std::cos(0.5 * est[2]), az = std::sin(0.5 * est[2]);
    const double pw = aw * qw - az * qz, pz = aw * qz + az * qw;
    local_pose[0] = est[0]; local_pose[1] = est[1]; local_pose[2] = yaw_of_quaternion_f64(pw, pz);
    yaw_f32 = yaw_of_quaternion_f32((float)pw, (float)pz);
    const float af = (float)est[2], ha = 0.5f * af;
    yaw2 = yaw_of_quaternion_f32((float)std::cos((double)ha), (float)std::sin((double)ha));
}
// the scan's origin (tracking frame) in the local frame: through the gravity alignment, then through Embed3D(est.cast<float>())
void origin_in_local(const float origin_xy[2], float yaw_g, const double est[3], float yaw2, float out[2])
{
    float org[2];
    rigid2f_apply(0.f, 0.f, yaw_g, origin_xy, 1, org);
    rigid2f_apply((float)est[0], (float)est[1], yaw2, org, 1, out);
}
// MapBuilder::CreateGrid (map_builder.cc:112-126): the limits of the submap the first inserted scan creates, kInitialSubmapSize = 100
// cells a side around its origin in local; `float resolution = options_.resolution`.  RGRID_ERR_CAPACITY when the handle holds fewer
// cells, RGRID_ERR_INVALID for a resolution that is not > 0 (NaN included); the outputs are untouched then.
int initial_submap_limits(float options_resolution, const float origin_local[2], long long max_cells, int &nx, int &ny, double &resolution,
                          double &max_x, double &max_y)
{
#pragma clang fp contract(off)
    const int n0 = 100;
    const double r = (double)options_resolution, half = 0.5 * n0 * r;
    if ((long long)n0 * n0 > max_cells) return RGRID_ERR_CAPACITY;
    if (!(r > 0.)) return RGRID_ERR_INVALID;
    nx = n0; ny = n0; resolution = r; max_x = (double)origin_local[0] + half; max_y = (double)origin_local[1] + half;
    return RGRID_OK;
}

}  // namespace
