// rgrid_dev.h -- what the two correlative scan matchers share: rgrid.hip (one handle, one scan: kg_discretize, kg_score, kg_best)
// and rgrid_batch.hip (one scan of many robots, one launch: kgb_match).
//
// Host side, ONE text: what RealTimeCorrelativeScanMatcher2D::Match does before and after its candidate loop (plan_match,
// rotation_table, decode_best) and G_TRY, the status macro of both handles.  Each caller adds only its own capacity limits.
// Device side, two texts by measurement: BestRec, value_to_probability and rotation_cs are compiled by both files, but the
// discretisation's index formula and the first-maximum comparison are written out inside kg_discretize / kg_score / kg_best --
// calling them through the two functions below changed kg_score's instruction schedule -- and cell_index_of / best_before restate
// them for rgrid_batch.hip.  tests/test_fleet_match_gpu.py holds the two matchers together bit for bit.
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

}  // namespace
