// det3d_batch.hip -- the 3D (point cloud) reflector detector for a fleet: B robots' clouds detected by ONE launch (rdet3d_batch_* of
// include/rdet.h).
//
// Every member of a batch handle is one reflector_detect::PointCloudReflectorDetect (reference
// src/reflector_detect/point_cloud/point_cloud_reflector_detect.cc:9-106; the PCL semantics are spelled out in det3d.hip's header and
// DESIGN.md section 4): its own intensity gate and sensor_to_base_link.  k_det3d_batch runs ONE workgroup of 1024 threads per cloud, and
// that workgroup does the whole of HandlePointCloud for its cloud in its CU's LDS: the gate with its order-preserving compaction, the 31
// nearest neighbours of every survivor, the FP64 statistics, the components of the 0.2 m graph, the size gate, the order and the float32
// centroids.  Nothing crosses a workgroup: no atomics between workgroups, no counters, nothing in global memory that a second workgroup
// touches, nobody waits for anybody.  (det3d.hip spreads ONE cloud over the chip in five launches, every edge of that chain all-to-all.)
//
// A workgroup holds at most RDET3DB_MAX_BRIGHT = 5120 survivors of the gate (det3d.hip's MFAST: what the single detector serves with its
// short chain); a cloud with more is reported with RDET_ERR_CAPACITY and its true count, and goes through an rdet3d_t.
//
// The arithmetic is det3d.hip's, restated: that file's helpers live in its anonymous namespace and the file is pinned by the profile
// manifest.  tests/test_fleet_detect3d_gpu.py holds the two together bit for bit (against the oracle and against a single handle).
//
// The neighbour searches: nodes keep their ARRIVAL order (no sort); every 64 consecutive nodes get a bounding box (a lidar's consecutive
// returns lie on one post, so the boxes are small), one wave takes one query with the candidates one per lane, tiles are opened nearest
// first and only while their box is nearer than the query's current 31st distance (k3_knn's scheme on LDS).  The multiset of the 31
// smallest distances is exact whatever the boxes are.
//
// Here: the kernel, the handle's buffers, the copies and the launch.  The host's rules that need no HIP call are det_batch_host.h's
// (tested without a GPU), create / destroy / link / collect as both detector handles make them det_batch_dev.h's.
#include "det_batch_dev.h"         // det_batch_host.h: Cloud3Rec and the host's rules

#include <cmath>
#include <cstdio>

namespace host = det_batch_host;
namespace dev = det_batch_dev;

namespace {

constexpr int MEAN_K = 30;                    // point_cloud_reflector_detect.cc:45
constexpr int KNN = MEAN_K + 1;
constexpr double STD_MUL = 0.5;               // :46
constexpr float TOL2 = (float)(0.2 * 0.2);    // :69 (FLANN radius search: squared distance < r^2)
constexpr int MIN_SZ = 4, MAX_SZ = 160;       // :70-71
constexpr int TILE = det_batch_host::CLOUD_TILE;      // nodes per bounding box = candidates per step (64)
constexpr int MAX_TILES = RDET3DB_MAX_BRIGHT / TILE;      // 80
constexpr float BOX_MARGIN = 0.9999f;         // box distance^2 * margin < bound  <=>  "some point of the box may matter"
constexpr int KNN_FEW = 6;                    // a step with at most this many admissible candidates inserts them one by one

using det_batch_host::Cloud3Rec;

// What a cloud hands back, in pinned host memory: plain stores, published by the end of the kernel
struct Cloud3Out {
    int K, err, M, pad;
    float2 centers[RDET_MAX_CENTERS];
};

struct Batch3Bufs {
    const Cloud3Rec *recs;         // [clouds that run]
    const float *stage;            // [B][4 * max_points]: x, y, z, intensity of member m's cloud
    Cloud3Out *out;                // [count], pinned host memory
    int max_points;
    int cap;                       // nodes the dynamic LDS of this launch holds (a multiple of 64, <= RDET3DB_MAX_BRIGHT)
};

__device__ static float d2f(float ax, float ay, float az, float bx, float by, float bz)
{
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    float r = dx * dx;           // FLANN L2_Simple: float accumulation over x, y, z
    r += dy * dy;
    r += dz * dz;
    return r;
}

// squared distance from a point to a box (a lower bound of d2f to every point inside it, up to rounding: BOX_MARGIN)
__device__ static inline float box_d2(float px, float py, float pz, float x0, float y0, float z0, float x1, float y1, float z1)
{
    const float dx = fmaxf(fmaxf(x0 - px, px - x1), 0.f);
    const float dy = fmaxf(fmaxf(y0 - py, py - y1), 0.f);
    const float dz = fmaxf(fmaxf(z0 - pz, pz - z1), 0.f);
    return dx * dx + dy * dy + dz * dz;
}

// lane ^ J exchanges without the LDS crossbar: DPP quad permutes, row shifts under bank masks, gfx950's permlane swaps (det3d.hip)
template <int CTRL, int BANK>
__device__ static inline int b3_dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, BANK, false); }
template <int J>
__device__ static inline float lane_xor(float f, int lane)
{
    const int v = __float_as_int(f);
    int r;
    if (J == 1) r = __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);
    else if (J == 2) r = __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);
    else if (J == 4) r = b3_dpp<0x114, 0xA>(b3_dpp<0x104, 0x5>(v, v), v);
    else if (J == 8) r = b3_dpp<0x118, 0xC>(b3_dpp<0x108, 0x3>(v, v), v);
    else if (J == 16) { const auto p = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false); r = (int)((lane & 16) ? p[0] : p[1]); }
    else { const auto p = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false); r = (int)((lane & 32) ? p[0] : p[1]); }
    return __int_as_float(r);
}
template <int J>
__device__ static inline double lane_xor_f64(double v, int lane)
{
    const float lo = lane_xor<J>(__int_as_float(__double2loint(v)), lane), hi = lane_xor<J>(__int_as_float(__double2hiint(v)), lane);
    return __hiloint2double(__float_as_int(hi), __float_as_int(lo));
}
// the sum of one double per lane, in every lane: partners 1, 2, 4, ... 32 apart add up (k3_cc_min's butterfly)
__device__ static inline double wave_sum_f64(double v, int lane)
{
    v += lane_xor_f64<1>(v, lane); v += lane_xor_f64<2>(v, lane); v += lane_xor_f64<4>(v, lane);
    v += lane_xor_f64<8>(v, lane); v += lane_xor_f64<16>(v, lane); v += lane_xor_f64<32>(v, lane);
    return v;
}
__device__ static inline float wave_min_f32(float v, int lane)
{
    v = fminf(v, lane_xor<1>(v, lane)); v = fminf(v, lane_xor<2>(v, lane)); v = fminf(v, lane_xor<4>(v, lane));
    v = fminf(v, lane_xor<8>(v, lane)); v = fminf(v, lane_xor<16>(v, lane)); v = fminf(v, lane_xor<32>(v, lane));
    return v;
}
__device__ static inline float wave_max_f32(float v, int lane)
{
    v = fmaxf(v, lane_xor<1>(v, lane)); v = fmaxf(v, lane_xor<2>(v, lane)); v = fmaxf(v, lane_xor<4>(v, lane));
    v = fmaxf(v, lane_xor<8>(v, lane)); v = fmaxf(v, lane_xor<16>(v, lane)); v = fmaxf(v, lane_xor<32>(v, lane));
    return v;
}
__device__ static inline float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// one compare-exchange stage of a bitonic network over the lanes (det3d.hip): min or max as ONE v_med3_f32 against -inf / +inf
template <int K, int J, bool DESC>
__device__ static inline float bitonic_stage(float v, int lane)
{
    const float o = lane_xor<J>(v, lane);
    const bool asc = (K == 64) ? !DESC : (((lane & K) == 0) != DESC);
    return __builtin_amdgcn_fmed3f(v, o, (asc == ((lane & J) == 0)) ? -INFINITY : INFINITY);
}
template <bool DESC>
__device__ static inline float wave_sort64(float v, int lane)
{
#define B3_STG(K, J) v = bitonic_stage<K, J, DESC>(v, lane);
    B3_STG(2, 1)
    B3_STG(4, 2) B3_STG(4, 1)
    B3_STG(8, 4) B3_STG(8, 2) B3_STG(8, 1)
    B3_STG(16, 8) B3_STG(16, 4) B3_STG(16, 2) B3_STG(16, 1)
    B3_STG(32, 16) B3_STG(32, 8) B3_STG(32, 4) B3_STG(32, 2) B3_STG(32, 1)
    B3_STG(64, 32) B3_STG(64, 16) B3_STG(64, 8) B3_STG(64, 4) B3_STG(64, 2) B3_STG(64, 1)
#undef B3_STG
    return v;
}
// S ascending, D DESCENDING by lane -> the 64 smallest of both, ascending by lane
__device__ static inline float wave_merge64(float S, float D, int lane)
{
    float c = fminf(S, D);
    c = bitonic_stage<64, 32, false>(c, lane); c = bitonic_stage<64, 16, false>(c, lane); c = bitonic_stage<64, 8, false>(c, lane);
    c = bitonic_stage<64, 4, false>(c, lane); c = bitonic_stage<64, 2, false>(c, lane); c = bitonic_stage<64, 1, false>(c, lane);
    return c;
}
// the lane with the smallest v (>= 0 or +inf) among the lanes of `set`
__device__ static inline int nearest_of(unsigned long long set, float v, int lane)
{
    const bool in = (set >> lane) & 1ull;
    const float w = in ? v : INFINITY;
    const float mn = wave_min_f32(w, lane);
    return __ffsll((long long)__ballot(in && w == mn)) - 1;
}

// ---- union-find on LDS.  Only roots are ever hooked, under SMALLER roots, so a component's final root is its smallest node whatever the
// interleaving; every value parent[x] has ever held is an ancestor of x for good, so a racing path-halving store is harmless.
__device__ static inline int uf_ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ static inline void uf_st(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ static int uf_find(int *parent, int x)
{
    int p = uf_ld(&parent[x]);
    while (p != x) {
        const int gp = uf_ld(&parent[p]);
        if (gp != p) uf_st(&parent[x], gp);                      // path halving
        x = p; p = gp;
    }
    return x;
}
__device__ static void uf_union(int *parent, int a, int b)
{
    a = uf_find(parent, a); b = uf_find(parent, b);
    while (a != b) {
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(&parent[hi], hi, lo);          // (LDS: this workgroup's own)
        if (old == hi) return;
        const int up = uf_find(parent, old);                     // hi has a parent (< hi): on from there
        if (hi == a) a = up; else b = up;
    }
}

// order-preserving compaction of one flag per thread, one tile of 1024 per call: this thread's position among the flagged ones, `base`
// included; base grows by the tile's count in every thread alike.  ONE barrier per call: the wave counts alternate between two LDS rows.
__device__ static inline int tile_compact(bool flag, int (*wsum)[16], int parity, int &base)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long bal = __ballot(flag);
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    if (lane == 0) wsum[parity][wave] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { const int c = wsum[parity][w]; if (w < wave) off += c; tot += c; }
    base += tot;
    return off + __popcll(bal & lt);
}

// the bounding boxes of every 64 consecutive nodes; `masked`: without the nodes whose label is -1 (SOR's outliers).  NaN coordinates
// are left out by fminf / fmaxf (their distances are NaN: no neighbour of anything); a tile without a point gets an empty box (+inf, -inf).
__device__ static inline void tile_boxes(const float *X, const float *Y, const float *Z, const int *label, bool masked, int M, float (*box)[6])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntiles = (M + TILE - 1) / TILE;
    for (int t = wave; t < ntiles; t += 16) {
        const int j = TILE * t + lane;
        const bool in = j < M && !(masked && label[j] < 0);
        const float x = in ? X[j] : NAN, y = in ? Y[j] : NAN, z = in ? Z[j] : NAN;
        const float x0 = wave_min_f32(fminf(x, INFINITY), lane), y0 = wave_min_f32(fminf(y, INFINITY), lane), z0 = wave_min_f32(fminf(z, INFINITY), lane);
        const float x1 = wave_max_f32(fmaxf(x, -INFINITY), lane), y1 = wave_max_f32(fmaxf(y, -INFINITY), lane), z1 = wave_max_f32(fmaxf(z, -INFINITY), lane);
        if (lane == 0) { box[t][0] = x0; box[t][1] = y0; box[t][2] = z0; box[t][3] = x1; box[t][4] = y1; box[t][5] = z1; }
    }
}

// ================================================================================================
// One workgroup per cloud.  Dynamic LDS: x | y | z | dist | label, B.cap nodes each (dist becomes the components' sizes).
// ================================================================================================
__global__ __launch_bounds__(1024) void k_det3d_batch(Batch3Bufs B)
{
    extern __shared__ float lds_dyn[];
    __shared__ Cloud3Rec s_rec;
    __shared__ int s_wsum[2][16];
    __shared__ float s_box[MAX_TILES][6];
    __shared__ double s_red[2][4];
    __shared__ int s_root[RDET_MAX_CENTERS], s_size[RDET_MAX_CENTERS], s_order[RDET_MAX_CENTERS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    static_assert(sizeof(Cloud3Rec) % 4 == 0 && sizeof(Cloud3Rec) / 4 <= 1024, "the record is copied one word per thread");
    if (tid < (int)(sizeof(Cloud3Rec) / 4)) ((unsigned *)&s_rec)[tid] = ((const unsigned *)(B.recs + blockIdx.x))[tid];
    __syncthreads();
    const Cloud3Rec &A = s_rec;
    Cloud3Out *const out = B.out + A.slot;
    const int N = A.N, cap = B.cap;
    float *const X = lds_dyn, *const Y = X + cap, *const Z = Y + cap, *const D = Z + cap;
    int *const label = (int *)(D + cap);
    int *const cnt = (int *)D;
    if (N <= 0 || N > B.max_points) {                    // (the host launches no such cloud: a bound, not a path)
        if (tid == 0) { out->K = 0; out->err = 0; out->M = 0; out->pad = 0; }
        return;
    }

    // ---- 1. the gate (:31-39): (double) intensity > intensity_min, compacted in arrival order, tiles of 1024 points
    int M = 0;
    {
        const float4 *const cloud = (const float4 *)(B.stage + (size_t)A.member * 4 * (size_t)B.max_points);
        const double imin = A.intensity_min;
        const int ntile = (N + 1023) / 1024;
        for (int t = 0; t < ntile; ++t) {
            const int i = 1024 * t + tid;
            const float4 p = (i < N) ? cloud[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            const bool flag = i < N && (double)p.w > imin;
            const int pos = tile_compact(flag, s_wsum, t & 1, M);
            if (flag && pos < cap) { X[pos] = p.x; Y[pos] = p.y; Z[pos] = p.z; }
        }
    }
    if (M > cap || M > RDET3DB_MAX_BRIGHT) {             // (cap < 5120 only when N <= cap: then M <= cap)
        if (tid == 0) { out->K = 0; out->err = RDET_ERR_CAPACITY; out->M = M; out->pad = 0; }
        return;
    }
    __syncthreads();
    const int ntiles = (M + TILE - 1) / TILE;

    // ---- 2. StatisticalOutlierRemoval part 1 (:43-47): the mean distance to the 30 nearest neighbours
    if (M >= KNN) {
        tile_boxes(X, Y, Z, label, false, M, s_box);
        __syncthreads();
        for (int q = wave; q < M; q += 16) {
            const float qx = X[q], qy = Y[q], qz = Z[q];
            const int t_own = q >> 6;
            float S;
            {
                const int j = TILE * t_own + lane;
                const int jj = j < M ? j : q;
                const float d2 = d2f(qx, qy, qz, X[jj], Y[jj], Z[jj]);
                S = wave_sort64<false>((j < M && d2 == d2) ? d2 : INFINITY, lane);
            }
            float bound = lane_value(S, KNN - 1);
            for (int r0 = 0; r0 < ntiles; r0 += 64) {
                const int t = r0 + lane;
                float db = INFINITY;
                if (t < ntiles && t != t_own)
                    db = box_d2(qx, qy, qz, s_box[t][0], s_box[t][1], s_box[t][2], s_box[t][3], s_box[t][4], s_box[t][5]) * BOX_MARGIN;
                unsigned long long todo = __ballot(db < bound);
                while (todo) {
                    const int tl = nearest_of(todo, db, lane);
                    todo &= ~(1ull << tl);
                    const int j = TILE * (r0 + tl) + lane;
                    const int jj = j < M ? j : q;
                    const float d2 = d2f(qx, qy, qz, X[jj], Y[jj], Z[jj]);
                    const float d = (j < M && d2 == d2) ? d2 : INFINITY;
                    unsigned long long adm = __ballot(d < bound);
                    if (adm == 0ull) continue;
                    if (__popcll(adm) <= KNN_FEW) {
                        while (adm) {
                            const int l = __ffsll((long long)adm) - 1;
                            adm &= adm - 1;
                            const float x = lane_value(d, l);
                            if (!(x < bound)) continue;
                            const int pos = __popcll(__ballot(S <= x));           // S is ascending: a prefix of the lanes keeps its place
                            const float sh = __int_as_float(b3_dpp<0x138, 0xf>(__float_as_int(S), __float_as_int(S)));   // wave_shr:1
                            S = (lane < pos) ? S : ((lane == pos) ? x : sh);
                            bound = lane_value(S, KNN - 1);
                        }
                    } else {
                        S = wave_merge64(S, wave_sort64<true>(d, lane), lane);
                        bound = lane_value(S, KNN - 1);
                    }
                    todo &= __ballot(db < bound);
                }
            }
            const float sq = sqrtf(S);
            double dist_sum = 0;
#pragma unroll
            for (int k = 1; k < KNN; ++k) dist_sum += (double)lane_value(sq, k);   // k = 0 is the query itself; ascending
            if (lane == 0) D[q] = (float)(dist_sum / MEAN_K);
        }
    } else {
        for (int j = tid; j < M; j += 1024) D[j] = 0.f;          // fewer than MeanK+1 points: every search "failed"
    }
    __syncthreads();

    // ---- 3. part 2: mean and (n-1)-variance of the M distances in FP64, in k3_cc_min's order (256 threads, sixteen consecutive nodes a
    // thread and round; a butterfly over the lanes; the four waves in turn; sq += v * v contracted as that file's build contracts it)
    double thr;
    {
        if (tid < 256) {
            double sum = 0, sq = 0;
            for (int base = 16 * tid; base < M; base += 16 * 256) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const double v = (base + j < M) ? (double)D[base + j] : 0.0;
                    sum += v; sq = fma(v, v, sq);
                }
            }
            sum = wave_sum_f64(sum, lane); sq = wave_sum_f64(sq, lane);
            if (lane == 0) { s_red[0][wave] = sum; s_red[1][wave] = sq; }
        }
        __syncthreads();
        {
#pragma clang fp contract(off)
            double r0 = s_red[0][0], r1 = s_red[1][0];
#pragma unroll
            for (int w = 1; w < 4; ++w) { r0 += s_red[0][w]; r1 += s_red[1][w]; }
            const double valid = (M >= KNN) ? (double)M : 0.0;
            const double mean = r0 / valid;
            const double variance = (r1 - r0 * r0 / valid) / (valid - 1);
            thr = mean + STD_MUL * sqrt(variance);               // (0.5 * x is exact: contracted or not, the same bits; NaN keeps everything)
        }
    }

    // ---- 4. EuclideanClusterExtraction (:65-74) as the components of the radius graph over the nodes SOR keeps
    for (int j = tid; j < M; j += 1024) label[j] = ((double)D[j] > thr) ? -1 : j;
    __syncthreads();
    tile_boxes(X, Y, Z, label, true, M, s_box);
    __syncthreads();
    for (int q = wave; q < M; q += 16) {
        if (uf_ld(&label[q]) < 0) continue;                       // (an outlier stays one: wave-uniform)
        const float qx = X[q], qy = Y[q], qz = Z[q];
        const int t_last = q >> 6;                                // every edge is met from its larger end
        for (int r0 = 0; r0 <= t_last; r0 += 64) {
            const int t = r0 + lane;
            float db = INFINITY;
            if (t <= t_last) db = box_d2(qx, qy, qz, s_box[t][0], s_box[t][1], s_box[t][2], s_box[t][3], s_box[t][4], s_box[t][5]) * BOX_MARGIN;
            unsigned long long todo = __ballot(db < TOL2);
            while (todo) {
                const int tl = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int j = TILE * (r0 + tl) + lane;
                if (j < q && uf_ld(&label[j]) >= 0 && d2f(qx, qy, qz, X[j], Y[j], Z[j]) < TOL2) uf_union(label, q, j);
            }
        }
    }
    __syncthreads();
    // every node's final root; the sizes' array (the distances are done with)
    for (int j = tid; j < M; j += 1024) {
        cnt[j] = 0;
        if (uf_ld(&label[j]) >= 0) uf_st(&label[j], uf_find(label, j));
    }
    __syncthreads();
    for (int j = tid; j < M; j += 1024) {
        const int r = label[j];
        if (r >= 0) atomicAdd(&cnt[r], 1);
    }
    __syncthreads();

    // ---- 5. the size gate (:70-71) and the order: size descending, then label (= smallest node) ascending
    int nacc = 0;
    {
        const int nt = (M + 1023) / 1024;
        for (int t = 0; t < nt; ++t) {
            const int j = 1024 * t + tid;
            const int sz = (j < M && label[j] == j) ? cnt[j] : 0;
            const bool acc = sz >= MIN_SZ && sz <= MAX_SZ;
            const int pos = tile_compact(acc, s_wsum, t & 1, nacc);
            if (acc && pos < RDET_MAX_CENTERS) { s_root[pos] = j; s_size[pos] = sz; }
        }
    }
    __syncthreads();
    if (nacc > RDET_MAX_CENTERS) {
        if (tid == 0) { out->K = 0; out->err = RDET_ERR_CAPACITY; out->M = M; out->pad = 0; }
        return;
    }
    if (tid < nacc) {
        const int sz = s_size[tid];
        int rank = 0;
        for (int d = 0; d < nacc; ++d) {
            const int sd = s_size[d];
            rank += (sd > sz || (sd == sz && d < tid)) ? 1 : 0;  // (the table is in label order)
        }
        s_order[rank] = tid;
    }
    __syncthreads();

    // ---- 6. compute3DCentroid (:77-97): float32 running sums in node order, / count, Rigid2f to base_link.  One wave per component.
    for (int r = wave; r < nacc; r += 16) {
#pragma clang fp contract(off)
        const int c = s_order[r];
        const int root = s_root[c], size = s_size[c];
        float cx = 0.f, cy = 0.f;
        int count = 0;
        for (int j0 = root & ~63; j0 < M && count < size; j0 += 64) {
            const int j = j0 + lane;
            const bool mem = j < M && label[j] == root;
            const float vx = mem ? X[j] : 0.f, vy = mem ? Y[j] : 0.f;
            unsigned long long mask = __ballot(mem);
            count += __popcll(mask);
            while (mask) {                                       // (the ballot is wave-uniform: scalar loop, v_readlane)
                const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
                mask &= mask - 1;
                cx += lane_value(vx, b);
                cy += lane_value(vy, b);
            }
        }
        cx /= (float)size; cy /= (float)size;                    // :94
        if (lane == 0) out->centers[r] = make_float2((A.cs * cx + (-A.sn) * cy) + A.sx, (A.sn * cx + A.cs * cy) + A.sy);   // :96
    }
    if (tid == 0) { out->K = nacc; out->err = 0; out->M = M; out->pad = 0; }
}

constexpr size_t LDS_PER_NODE = 4 * sizeof(float) + sizeof(int);

}  // namespace

// =================================================================================================
// The handle
struct rdet3d_batch : dev::Handle {
    int max_points = 0;
    std::vector<host::Member3d> m;
    // the staging area the host writes and the kernel reads in place: fine-grained DEVICE memory through the PCIe BAR where the platform
    // maps it, else pinned host memory (host_visible.h)
    batch_host::Staging<float> stage;  // [B][4 * max_points]
    batch_host::Pinned<Cloud3Rec> recs; // [B]
    batch_host::Pinned<Cloud3Out> out; // [B]
};

extern "C" {

int rdet3d_batch_sizeof_cloud(void) { return (int)sizeof(rdet3d_cloud); }

int rdet3d_batch_max_bright(void) { return RDET3DB_MAX_BRIGHT; }

const char *rdet3d_batch_last_hip_error(rdet3d_batch_t *b) { return b ? b->hip_error.c_str() : ""; }

int rdet3d_batch_create(const rdet3d_options *opts, const double *s2b_xyyaw, int B, int max_points, int device, rdet3d_batch_t **out)
{
    if (!opts || !s2b_xyyaw || !out || B < 1 || max_points < 1) return RDET_ERR_INVALID;
    *out = nullptr;
    rdet3d_batch_t *b = dev::make<rdet3d_batch>(opts, s2b_xyyaw, B, device);
    if (!b) return RDET_ERR_INVALID;
    b->max_points = max_points;
    const size_t np = (size_t)max_points, nB = (size_t)B;
    int rc = [&]() -> int {
        DETB_TRY(b, hipSetDevice(device));
        DETB_TRY(b, hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        DETB_TRY(b, b->stage.alloc(4 * np * nB));
        DETB_TRY(b, b->recs.alloc(nB));
        DETB_TRY(b, b->out.alloc(nB));
        std::memset(b->out.h, 0, sizeof(Cloud3Out) * nB);
        DETB_TRY(b, hipFuncSetAttribute((const void *)k_det3d_batch, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(LDS_PER_NODE * RDET3DB_MAX_BRIGHT)));
        return RDET_OK;
    }();
    if (rc != RDET_OK) { std::fprintf(stderr, "rdet3d_batch_create: %s\n", b->hip_error.c_str()); rdet3d_batch_destroy(b); return rc; }
    *out = b;
    return RDET_OK;
}

void rdet3d_batch_destroy(rdet3d_batch_t *b)
{
    if (!b) return;
    dev::destroy(b, b->stage, b->recs, b->out);
    delete b;
}

int rdet3d_batch_set_sensor_to_base_link(rdet3d_batch_t *b, int member, const double xyyaw[3]) { return dev::set_sensor_to_base_link(b, member, xyyaw); }

int rdet3d_batch_staging(rdet3d_batch_t *b, int member, float **xyzi)
{
    if (!b || !xyzi || member < 0 || member >= b->B) return RDET_ERR_INVALID;
    *xyzi = b->stage.h + (size_t)member * 4 * (size_t)b->max_points;
    return RDET_OK;
}

int rdet3d_batch_submit(rdet3d_batch_t *b, const rdet3d_cloud *clouds, int count)
{
    if (!b || count < 0 || (count > 0 && !clouds) || b->outstanding) return RDET_ERR_INVALID;
    int rc = host::validate_clouds(clouds, count, b->B, b->max_points, b->seen);
    bool linked = false;
    if (rc == RDET_OK) rc = dev::begin_submit(b, &linked);
    if (rc != RDET_OK) return rc;
    int cap = 0;
    const int n_run = host::pack_clouds(clouds, count, b->m, *b, b->recs.h, &cap);
    for (int i = 0; i < count; ++i) {
        const rdet3d_cloud &c = clouds[i];
        if (!linked) std::memset(&b->out.h[i], 0, 4 * sizeof(int));
        float *dst = b->stage.h + (size_t)c.member * 4 * (size_t)b->max_points;     // the cloud into the member's slice, unless it was received there
        if (c.N > 0 && c.xyzi != dst) std::memcpy(dst, c.xyzi, sizeof(float) * 4 * (size_t)c.N);
    }
    b->outstanding = true;
    if (n_run > 0) {
        __atomic_thread_fence(__ATOMIC_SEQ_CST);              // write-combined stores drained before the doorbell
        Batch3Bufs Bf;
        Bf.recs = b->recs.dv; Bf.stage = b->stage.dv; Bf.out = b->out.dv; Bf.max_points = b->max_points;
        Bf.cap = cap;
        hipLaunchKernelGGL(k_det3d_batch, dim3((unsigned)n_run), dim3(1024), LDS_PER_NODE * (size_t)cap, b->stream, Bf);
        DETB_TRY(b, hipGetLastError());
    }
    return RDET_OK;
}

int rdet3d_batch_link(rdet3d_batch_t *b, rlink *out) { return b ? dev::link(b, b->out.dv, out) : RDET_ERR_INVALID; }

int rdet_sizeof_link(void) { return (int)sizeof(rlink); }     // (of both detectors' links: the library's one copy)

int rdet3d_batch_collect(rdet3d_batch_t *b, int *status, int *K, float *centers_xy, int max_centers, double *obs_time, int *n_bright)
{
    if (!b) return RDET_ERR_INVALID;
    return dev::collect(b, b->out.h, status, K, centers_xy, max_centers, obs_time, [&](int i, const Cloud3Out *o) {
        if (n_bright) n_bright[i] = o ? o->M : 0;
    });
}

}  // extern "C"

