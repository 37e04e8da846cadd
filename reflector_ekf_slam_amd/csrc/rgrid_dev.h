// rgrid_dev.h -- what the two correlative scan matchers share: rgrid.hip (one handle, one scan: kg_discretize, kg_score, kg_best)
// and rgrid_batch.hip (one scan of many robots, one launch: kgb_match).
//
// BestRec, value_to_probability and rotation_cs moved here from rgrid.hip word for word, and both files compile them: rgrid.hip's
// device code is the same instruction for instruction as before the move.  The discretisation's index formula and the
// first-maximum comparison are written out inside kg_discretize / kg_score / kg_best; calling them through the two functions below
// changed kg_score's instruction schedule, so rgrid.hip keeps its own text and cell_index_of / best_before restate it for
// rgrid_batch.hip.  tests/test_fleet_match_gpu.py holds the two matchers together bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

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

}  // namespace
