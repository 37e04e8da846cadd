// rgrid_dev.h -- what the two correlative scan matchers share: rgrid.hip (one handle, one scan: kg_discretize, kg_score, kg_best)
// and rgrid_batch.hip (one scan of many robots, one launch: kgb_match).
//
// Host side, ONE text: what RealTimeCorrelativeScanMatcher2D::Match does before and after its candidate loop (plan_match,
// rotation_table, decode_best) and G_TRY, the status macro of both handles.  Each caller adds only its own capacity limits.
// Device side, two texts by measurement: BestRec, value_to_probability and rotation_cs are compiled by both files, but the
// discretisation's index formula and the first-maximum comparison are written out inside kg_discretize / kg_score / kg_best --
// calling them through the two functions below changed kg_score's instruction schedule -- and cell_index_of / best_before restate
// them for rgrid_batch.hip.  tests/test_fleet_match_gpu.py holds the two matchers together bit for bit.
// The two range-data inserters (rgrid_insert / rgrid_grow_as_needed and kgb_insert) share the text at the end of this file.
#pragma once
#include "../../include/rgrid.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

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

}  // namespace
