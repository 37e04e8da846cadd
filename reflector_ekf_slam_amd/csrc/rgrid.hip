// rgrid.hip -- MI355X-native grid-mapper front-end behind include/rgrid.h.
//
// Replaces, in the reference: sensor::VoxelFilter / AdaptiveVoxelFilter (src/sensor/voxel_filter.cc:12-120) and
// scan_matching::RealTimeCorrelativeScanMatcher2D::Match with SearchParameters / GenerateRotatedScans /
// DiscretizeScans (src/scan_matching/real_time_correlative_scan_matcher_2d.cc:20-136,
// correlative_scan_matcher_2d.cc:10-123), scored against a mapping::ProbabilityGrid given by its uint16 cells.
//
// Split of work.  Host (O(points) + O(scans), same libm as a CPU build, so every transcendental the
// discretisation depends on is bit-identical to a CPU run): the initial rotation of the cloud, the search
// parameters, one (cos, sin) pair per rotated scan.  Device (O(scans * points) + O(candidates * points)):
//   kg_discretize  rotate, translate and discretise every point of every scan into cell indices   (:86-123)
//   kg_score       one workgroup per rotated scan, one lane per translation candidate: float32 sum of the cell
//                  probabilities in point order (:20-36), the exp(-(.)^2) penalty (:127-133), workgroup arg-max with
//                  the first-maximum rule of std::max_element (:104-105)
//   kg_best        arg-max over the workgroups
// and for the voxel filters: kg_keys (voxel of every point), kg_first (a point survives iff no EARLIER point
// shares its voxel: all-pairs, the candidates arrive through the scalar cache), kg_compact (order-preserving
// ballot-scan compaction; also the range gate of the adaptive filter).  The bisection over voxel sizes of the
// adaptive filter (:47-73) stays on the host: a dozen dependent decisions on one integer each.
// The host steps this handle has in common with the fleet handle (rgrid_batch.hip) are rgrid_dev.h's, one text for both.
#include "../../include/rgrid.h"
#include "batch_host.h"
#include "rgrid_dev.h"
#include "rgrid_refine_dev.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace {

// ---- voxel filter -----------------------------------------------------------------------------------
// The voxel of point i = blockIdx.x * 256 + threadIdx.x and its flag in slice `slice` of key / keep: the body of kg_keys (one slice) and kg_keys_b
__device__ static inline void voxel_keys(const float *__restrict__ xy, int n, float res, size_t slice, int2 *__restrict__ key, unsigned char *__restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // GetCellIndex (voxel_filter.cc:105-110): RoundToInt(point / resolution), float division, lround
    key[slice + i] = make_int2((int)lroundf(xy[2 * i] / res), (int)lroundf(xy[2 * i + 1] / res));
    keep[slice + i] = 1;                                               // kg_first clears it when an earlier point shares the voxel
}

__global__ __launch_bounds__(256) void kg_keys(const float *__restrict__ xy, int n, float res, int2 *__restrict__ key,
                                               unsigned char *__restrict__ keep)
{
    voxel_keys(xy, n, res, 0, key, keep);
}

// Workgroup (bi, bj), bj <= bi: the 256 points i of block bi against the 256 candidates j of block bj (j < i).
// A point that finds an earlier point in its voxel clears its flag (several workgroups may: same value).
__global__ __launch_bounds__(256) void kg_first(const int2 *__restrict__ key, int n, unsigned char *__restrict__ keep)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const int i = bi * 256 + threadIdx.x;
    const bool live = i < n;
    const int2 k = live ? key[i] : make_int2(0, 0);
    bool dup = false;
    const int jbase = bj * 256, jend = min(n, jbase + 256);
    for (int j0 = jbase; j0 < jend; j0 += 8) {
        int2 c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = key[j0 + u];   // uniform, CONTIGUOUS addresses: one s_load_dwordx16 (a clamp per element would
                                                           // split it into eight loads); entries past n are padding, masked by j0 + u < i
#pragma unroll
        for (int u = 0; u < 8; ++u) dup |= (j0 + u < i) && c[u].x == k.x && c[u].y == k.y;
    }
    if (live && dup) keep[i] = 0;                                     // unordered_set::insert(...).second == false (:89-93)
}

// Batched variants for the adaptive filter's search: blockIdx.z / blockIdx.y picks one of up to VOX_BATCH voxel sizes,
// slice r of `key` / `keep` holds its keys / first-occurrence flags; kg_count_b sums a slice.
constexpr int VOX_BATCH = 32;
struct VoxBatch { int r; float res[VOX_BATCH]; };
__global__ __launch_bounds__(256) void kg_keys_b(const float *__restrict__ xy, int n, VoxBatch B, int2 *__restrict__ key,
                                                 unsigned char *__restrict__ keep)
{
    const int r = blockIdx.y;
    voxel_keys(xy, n, B.res[r], (size_t)r * n, key, keep);
}
__global__ __launch_bounds__(256) void kg_first_b(const int2 *__restrict__ key_all, int n, unsigned char *__restrict__ keep_all)
{
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const int2 *__restrict__ key = key_all + (size_t)blockIdx.z * n;
    const int i = bi * 256 + threadIdx.x;
    const bool live = i < n;
    const int2 k = live ? key[i] : make_int2(0, 0);
    bool dup = false;
    const int jbase = bj * 256, jend = min(n, jbase + 256);
    for (int j0 = jbase; j0 < jend; j0 += 8) {
        int2 c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = key[j0 + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) dup |= (j0 + u < i) && c[u].x == k.x && c[u].y == k.y;
    }
    if (live && dup) keep_all[(size_t)blockIdx.z * n + i] = 0;
}
__global__ __launch_bounds__(256) void kg_count_b(const unsigned char *__restrict__ keep_all, int n, int *__restrict__ counts)
{
    __shared__ int ws[4];
    const unsigned char *keep = keep_all + (size_t)blockIdx.x * n;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += 256) c += keep[i];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ __launch_bounds__(256) void kg_range_gate(const float *__restrict__ xy, int n, float max_range,
                                                     unsigned char *__restrict__ keep)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xy[2 * i], y = xy[2 * i + 1];
    keep[i] = (sqrtf(x * x + y * y) <= max_range) ? 1 : 0;           // FilterByMaxRange (:15-27): point.norm() <= max_range
}

// order-preserving compaction of the kept points, one workgroup, ballot scan per 1024-point tile
__global__ __launch_bounds__(1024) void kg_compact(const float *__restrict__ xy, const unsigned char *__restrict__ keep, int n,
                                                   float *__restrict__ out, int *__restrict__ count)
{
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += 1024) {
        const int i = t0 + tid;
        const bool k = i < n && keep[i];
        const unsigned long long bal = __ballot(k);
        const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = wsum[w]; if (w < wave) off += c; tot += c; }
        if (k) { const int pos = off + __popcll(bal & lt); out[2 * pos] = xy[2 * i]; out[2 * pos + 1] = xy[2 * i + 1]; }
        __syncthreads();
        if (tid == 0) base += tot;
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

// ---- correlative scan matcher ---------------------------------------------------------------------
struct MatchArgs {
    int n, num_scans, num_linear, nx, ny;
    float tx, ty;                      // Eigen::Translation2f(initial translation)
    double resolution, max_x, max_y;
    double num_angular_d, step;        // orientation = (scan - num_angular) * step
    double wt, wr;
};

__global__ __launch_bounds__(256) void kg_discretize(MatchArgs A, const float *__restrict__ rot0, const float *__restrict__ cs,
                                                     int2 *__restrict__ idx)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.num_scans * A.n) return;
    const int scan = e / A.n, p = e - scan * A.n;
    const float c = cs[2 * scan], s = cs[2 * scan + 1];
    const float x = rot0[2 * p], y = rot0[2 * p + 1];
    const float rx = c * x - s * y, ry = s * x + c * y;                         // Rotation2Df * point (:95-98)
    const float px = rx + A.tx, py = ry + A.ty;                                 // Affine2f(initial_translation) * point (:117-118)
    // MapLimits::GetCellIndex (map_limits.h:47-55): (x index from y, y index from x), double arithmetic, lround
    idx[e] = make_int2((int)lround((A.max_y - (double)py) / A.resolution - 0.5),
                       (int)lround((A.max_x - (double)px) / A.resolution - 0.5));
}

// One workgroup per rotated scan, one lane per translation candidate of that scan.  The discretised point is the
// same for the whole workgroup: its indices come through the scalar cache; the float32 sum has to run in point
// order (:27-33), so the parallelism inside a candidate is in the LOADS: the cell values of sixteen points are in
// flight before their sixteen additions.
#define KG_PF 16
__global__ __launch_bounds__(128) void kg_score(MatchArgs A, const int2 *__restrict__ idx, const unsigned short *__restrict__ cells,
                                                BestRec *__restrict__ block_best)
{
#pragma clang fp contract(off)
    __shared__ float s_sc[2];
    __shared__ int s_id[2];
    const int scan = blockIdx.x;
    const int W = 2 * A.num_linear + 1, WW = W * W;
    const int2 *__restrict__ di = idx + (size_t)scan * A.n;
    const double orientation = ((double)scan - A.num_angular_d) * A.step;
    float best = -1.f; int bid = 0x7fffffff;
    for (int r0 = 0; r0 < WW; r0 += 128) {                                         // 81 candidates per scan with the default window: one pass
        const int r = r0 + threadIdx.x;
        const bool live = r < WW;
        const int xo = (live ? r / W : 0) - A.num_linear, yo = (live ? r - (r / W) * W : 0) - A.num_linear;   // order: x offset, y offset (:64-74)
        float sum = 0.f;
        for (int p0 = 0; p0 < A.n; p0 += KG_PF) {                                  // ComputeCandidateScore (:20-36), point order
            unsigned short v[KG_PF];
            bool in[KG_PF];
#pragma unroll
            for (int u = 0; u < KG_PF; ++u) {
                const int2 c = di[p0 + u];                                         // uniform, contiguous: wide scalar loads (d_idx is padded by KG_PF)
                const int cx = c.x + xo, cy = c.y + yo;
                in[u] = cx >= 0 && cy >= 0 && cx < A.nx && cy < A.ny;
                v[u] = cells[in[u] ? A.nx * cy + cx : 0];                          // unconditional load (clamped address): a predicated
                                                                                   // one is compiled to a branch + wait per point
            }
#pragma unroll
            for (int u = 0; u < KG_PF; ++u)
                if (p0 + u < A.n) sum += in[u] ? value_to_probability(v[u]) : 0.1f;   // outside the grid: kMinProbability
        }
        sum /= (float)A.n;
        const double x = -yo * A.resolution, y = -xo * A.resolution;              // Candidate2D (correlative_scan_matcher_2d.h:62-66)
        const double a = hypot(x, y) * A.wt + fabs(orientation) * A.wr;
        const float score = (float)((double)sum * exp(-(a * a)));                  // :127-133
        const int id = scan * WW + r;
        if (live && (score > best || (score == best && id < bid))) { best = score; bid = id; }
    }
    // workgroup arg-max, first maximum (smaller id wins a tie)
    for (int off = 32; off >= 1; off >>= 1) {
        const float os = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bid, off, 64);
        if (os > best || (os == best && oi < bid)) { best = os; bid = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_sc[wave] = best; s_id[wave] = bid; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_sc[1] > best || (s_sc[1] == best && s_id[1] < bid)) { best = s_sc[1]; bid = s_id[1]; }
        block_best[blockIdx.x].score = best;
        block_best[blockIdx.x].id = bid;
    }
}

__global__ __launch_bounds__(256) void kg_best(const BestRec *__restrict__ block_best, int nblocks, BestRec *__restrict__ out)
{
    __shared__ float s_sc[256];
    __shared__ int s_id[256];
    float best = -1.f; int bid = 0x7fffffff;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        const BestRec r = block_best[b];
        if (r.score > best || (r.score == best && r.id < bid)) { best = r.score; bid = r.id; }
    }
    s_sc[threadIdx.x] = best; s_id[threadIdx.x] = bid;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const float os = s_sc[threadIdx.x + off]; const int oi = s_id[threadIdx.x + off];
            if (os > s_sc[threadIdx.x] || (os == s_sc[threadIdx.x] && oi < s_id[threadIdx.x])) { s_sc[threadIdx.x] = os; s_id[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out->score = s_sc[0]; out->id = s_id[0]; }
}

// ---- range-data inserter --------------------------------------------------------------------------
// InsertArgs, apply_table and super_index are rgrid_dev.h's (shared with kgb_insert of rgrid_batch.hip), with the note on the
// races inside a phase.

// end points of all rays (returns first, then misses); *bad = 1 if anything lies outside the grid
__global__ __launch_bounds__(256) void kg_ends(InsertArgs A, const float *__restrict__ ret, const float *__restrict__ mis,
                                               int2 *__restrict__ ends, int *__restrict__ bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = A.n_ret + A.n_miss;
    if (i > n) return;
    int ix, iy;
    bool ok;
    if (i == n) ok = super_index(A, A.ox, A.oy, ix, iy);                        // the origin (:54-55)
    else {
        const float *p = (i < A.n_ret) ? ret + 2 * i : mis + 2 * (i - A.n_ret);
        ok = super_index(A, p[0], p[1], ix, iy);
    }
    ends[i] = make_int2(ix, iy);
    if (!ok) *bad = 1;
}
__global__ __launch_bounds__(256) void kg_hits(InsertArgs A, const int2 *__restrict__ ends, const int *__restrict__ bad,
                                               unsigned short *cells, const unsigned short *__restrict__ hit_table)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (*bad || i >= A.n_ret) return;
    apply_table(cells, A.nx, ends[i].x / SUBPX, ends[i].y / SUBPX, hit_table);   // (:59-62)
}
// One WAVE per ray.  RayToPixelMask (ray_to_pixel_mask.cc:17-168) walks the ray pixel column by pixel column and
// carries a sub-pixel ordinate `sub_y` (in units of 1 / (2 * 1000 * dx)); that recurrence has a closed form --
// with A(X) = A0 + dy * (first_pixel + 2000 * (X - X0)) the absolute ordinate at the right border of column X
// (dy * last_pixel instead of the full 2000 for the last column), column X covers the rows
//   dy > 0:  floor(A(X-1) / den) .. ceil(A(X) / den) - 1        (`while (sub_y > den)` / `if (sub_y == den)`)
//   dy <= 0: ceil(A(X-1) / den) - 1 .. floor(A(X) / den)        (`while (sub_y < 0)`  / `if (sub_y == 0)`)
// (first column: from the begin pixel's row) -- so the columns are independent.  Lanes take 64 columns at a time,
// a wave prefix sum of the rows per column flattens them into one pixel list, and the lanes share that list evenly:
// every lane has work whatever the slope.  The reference de-duplicates consecutive pixels; applying the table twice
// is a no-op, so no de-duplication here.
__global__ __launch_bounds__(256) void kg_rays(InsertArgs A, const int2 *__restrict__ ends, const int *__restrict__ bad,
                                               unsigned short *cells, const unsigned short *__restrict__ miss_table)
{
    __shared__ int s_pref[4][65], s_lo[4][64], s_step[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    const int n = A.n_ret + A.n_miss;
    if (*bad || i >= n) return;
    const long long S = SUBPX;
    long long bx = ends[n].x, by = ends[n].y, ex = ends[i].x, ey = ends[i].y;
    if (bx > ex) { long long t = bx; bx = ex; ex = t; t = by; by = ey; ey = t; }   // ordered by x (:24-27)
    const int X0 = (int)(bx / S), X1 = (int)(ex / S);
    if (X0 == X1) {                                                               // one pixel column (:35-47)
        const int y0 = (int)((by < ey ? by : ey) / S), y1 = (int)((by < ey ? ey : by) / S);
        for (int y = y0 + lane; y <= y1; y += 64) apply_table(cells, A.nx, X0, y, miss_table);
        return;
    }
    const long long dx = ex - bx, dy = ey - by, den = 2 * S * dx;
    const long long A0 = (2 * (by % S) + 1) * dx + (by / S) * den;                // absolute ordinate of the begin point (:64)
    const long long first_pixel = 2 * S - 2 * (bx % S) - 1, last_pixel = 2 * (ex % S) + 1;
    const bool up = dy > 0;
    auto a_out = [&](int X) -> long long {                                        // ordinate at the right border of column X
        return A0 + dy * (first_pixel + 2 * S * (long long)(X - X0) + ((X == X1) ? last_pixel - 2 * S : 0));
    };
    auto fdiv = [&](long long a) -> long long { return a / den; };                // a >= 0 inside the grid
    auto cdiv = [&](long long a) -> long long { return (a + den - 1) / den; };
    for (int Xc = X0; Xc <= X1; Xc += 64) {
        const int X = Xc + lane;
        int lo = 0, cnt = 0, step = 1;
        if (X <= X1) {
            const long long ao = a_out(X);
            int r_in, r_out;
            if (up) { r_in = (X == X0) ? (int)(by / S) : (int)fdiv(a_out(X - 1)); r_out = (int)cdiv(ao) - 1; cnt = r_out - r_in + 1; }
            else { r_in = (X == X0) ? (int)(by / S) : (int)cdiv(a_out(X - 1)) - 1; r_out = (int)fdiv(ao); cnt = r_in - r_out + 1; step = -1; }
            if (cnt < 1) cnt = 1;                                                 // the column's entry pixel is always visited
            lo = r_in;
        }
        // exclusive prefix sum of cnt over the wave
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
        s_pref[wave][lane + 1] = incl; s_lo[wave][lane] = lo; s_step[wave][lane] = step;
        if (lane == 0) s_pref[wave][0] = 0;
        __builtin_amdgcn_wave_barrier();
        const int total = s_pref[wave][64];
        for (int p = lane; p < total; p += 64) {
            int a = 0, b = 63;                                                    // column c with pref[c] <= p < pref[c+1]
            while (a < b) { const int mid = (a + b + 1) >> 1; if (s_pref[wave][mid] <= p) a = mid; else b = mid - 1; }
            const int row = s_lo[wave][a] + s_step[wave][a] * (p - s_pref[wave][a]);
            apply_table(cells, A.nx, Xc + a, row, miss_table);
        }
        __builtin_amdgcn_wave_barrier();
    }
}
__global__ __launch_bounds__(256) void kg_finish(unsigned short *cells, long long ncells, const int *__restrict__ bad)
{
    if (*bad) return;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < ncells && cells[k] >= MARKER) cells[k] -= MARKER;                    // Grid2D::FinishUpdate (grid_2d.cc:20-29)
}

// Grid2D::GrowLimits' cell copy (grid_2d.cc:81-91): every cell of the grown grid in one pass -- the old value
// inside the window at (off_x, off_y), unknown (0) outside
__global__ __launch_bounds__(256) void kg_grow(const unsigned short *__restrict__ old_cells, int nx, int ny, unsigned short *__restrict__ new_cells,
                                               int nnx, int nny, int off_x, int off_y)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= nnx) return;
    const int ox = x - off_x, oy = y - off_y;
    const bool in = ox >= 0 && oy >= 0 && ox < nx && oy < ny;
    new_cells[(size_t)y * nnx + x] = in ? old_cells[(size_t)oy * nx + ox] : (unsigned short)0;
}

// ---------------------------------------------------------------------------------------------------------------
// CeresScanMatcher2D::Match (src/scan_matching/ceres_scan_matcher_2d.cc:26-62) -- the whole Levenberg-Marquardt solve in
// ONE workgroup: a 3-parameter problem whose only wide part is the sum over the points (a few hundred after the
// adaptive voxel filter).  Every iteration the threads evaluate their points at the candidate pose (bicubic
// interpolation of the correspondence cost, 16 cell reads, analytic chain rule instead of Ceres' jets) and reduce
// 1/2|r|^2, J'r and J'J (10 doubles) through shuffles + LDS; thread 0 then runs the scalar trust-region logic on a
// state that lives in LDS (so the kernel fits 1024 threads: one point per thread up to 1024 points) and publishes
// the next candidate -- no host round trip, no second launch.
// Ceres is not in the image and not pinned by the reference: the algorithm is restated from its published sources
// (DESIGN.md 4b lists them); parity with a Ceres build is unpinned.  The device functions and records are rgrid_refine_dev.h's,
// shared with kgb_refine (rgrid_batch.hip).
__global__ __launch_bounds__(1024) void kg_refine(RefineArgs A, const unsigned short *__restrict__ cells, const float *__restrict__ pts,
                                                  RefineOut *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double part[16][10];
    __shared__ RefineState st;
    const int nw = blockDim.x >> 6;
    refine_eval(A, cells, pts, A.x0, A.y0, A.a0, part);                          // IterationZero
    __syncthreads();
    double S[10];
    if (threadIdx.x < 64) {
        const double x[3] = {A.x0, A.y0, A.a0};
        refine_totals(A, part, nw, x, S);
    }
    if (threadIdx.x == 0) {                                                     // = refine_begin of rgrid_refine_dev.h (kgb_refine's): edit both
        const double x[3] = {A.x0, A.y0, A.a0};
        for (int k = 0; k < 3; ++k) { st.x[k] = st.xc[k] = st.best[k] = x[k]; st.g[k] = S[1 + k]; }
        for (int k = 0; k < 6; ++k) st.H[k] = S[4 + k];
        st.s[0] = 1. / (1. + sqrt(S[4])); st.s[1] = 1. / (1. + sqrt(S[7])); st.s[2] = 1. / (1. + sqrt(S[9]));   // Jacobi scaling, fixed
        st.x_cost = st.initial_cost = 0.5 * S[0];
        st.x_norm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        st.gmax = fmax(fabs(S[1]), fmax(fabs(S[2]), fabs(S[3])));
        st.radius = 1e4; st.decrease = 2.; st.mcc = 0.; st.min_cost = INFINITY;
        st.ev_min = st.ev_cur = st.ev_ref = st.ev_cand = st.x_cost; st.acc_ref = st.acc_cand = 0.;
        st.nonmono = st.invalid = st.iter = 0; st.termination = 1; st.successful = 1; st.done = 0;
        refine_next_candidate(A, st);
    }
    __syncthreads();
#ifdef RGRID_DEBUG_TIMING
    if (threadIdx.x < 8) edbg[threadIdx.x] = 0;
    __syncthreads();
    long long dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = pinned_clock();
#endif
    while (!st.done) {
        const double c0 = st.xc[0], c1 = st.xc[1], c2 = st.xc[2];
        RT_MARK(0);                                                              // loop head: LDS read of the candidate
        refine_eval(A, cells, pts, c0, c1, c2, part);
        RT_MARK(1);                                                              // evaluation + wave reduction
        __syncthreads();
        RT_MARK(2);                                                              // barrier
        if (threadIdx.x < 64) {
            const double xc[3] = {c0, c1, c2};
            refine_totals(A, part, nw, xc, S);
        }
        if (threadIdx.x == 0) {
            RT_MARK(3);
            refine_judge(A, st, S);
            RT_MARK(4);
            if (!st.done) refine_next_candidate(A, st);
            RT_MARK(5);
        }
        __syncthreads();
        RT_MARK(6);
    }
    if (threadIdx.x == 0) {
        out->pose[0] = st.best[0]; out->pose[1] = st.best[1]; out->pose[2] = st.best[2];
        out->initial_cost = st.initial_cost; out->final_cost = st.min_cost; out->iterations = st.iter; out->termination = st.termination;
#ifdef RGRID_DEBUG_TIMING
        for (int k = 0; k < 8; ++k) { out->dbg[k] = dbg[k]; out->dbg[8 + k] = edbg[k]; }
#endif
    }
}

// ProbabilityGrid::DrawToSubmapTexture (probability_grid.cc:86-131): bounding box of the known cells
// (Grid2D::ComputeCroppedLimits -- the box ApplyLookupTable keeps is the box of the cells that are not 0) ...
__global__ __launch_bounds__(256) void kg_known_box(const unsigned short *__restrict__ cells, int nx, int ny, int *__restrict__ box)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const bool known = x < nx && cells[(size_t)nx * y + x] != 0;
    const unsigned long long m = __ballot(known);
    if (m == 0) return;
    if ((threadIdx.x & 63) == 0) {                                               // one lane per wave: its lanes' x range, the row
        const int base = blockIdx.x * 256 + (threadIdx.x & ~63);
        atomicMin(&box[0], base + __ffsll((long long)m) - 1);
        atomicMax(&box[2], base + 63 - __clzll((long long)m));
        atomicMin(&box[1], y);
        atomicMax(&box[3], y);
    }
}
// ... and two bytes (value, alpha) per cell of that window, x fastest, through a 32768-entry table of byte pairs
__global__ __launch_bounds__(256) void kg_texture(const unsigned short *__restrict__ cells, int nx, int x0, int y0, int w,
                                                  const unsigned short *__restrict__ table, unsigned short *__restrict__ out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < w) out[(size_t)w * y + x] = table[cells[(size_t)nx * (y0 + y) + (x0 + x)] & 32767u];
}

// The interior block of the painted texture (Node::PublishMap / HandleSaveMap) for the box kg_known_box found: the
// device text of kgb_occupancy's phase 2, the tiles spread over the launch's workgroups
__global__ __launch_bounds__(256) void kg_occupancy(const unsigned short *__restrict__ cells, int nx, int x0, int y0, int w, int hh,
                                                    const unsigned char *__restrict__ table, unsigned char *__restrict__ out)
{
    __shared__ __align__(16) unsigned char s_tile[OCC_T][OCC_PITCH];
    occupancy_tiles(cells, nx, x0, y0, w, hh, table, out, s_tile, (int)blockIdx.x, (int)gridDim.x);
}

}  // namespace

using batch_host::Device;
using batch_host::Host;

// The buffers are batch_host.h's aggregates (Host: pinned, default flags): rgrid_create allocates them, rgrid_destroy releases every one.
struct rgrid {
    int max_points = 0, max_cells = 0, max_candidates = 0, device = 0;
    hipStream_t stream = nullptr;
    Device<float> d_in, d_a, d_b, d_cs, d_mis;        // points in / two result buffers / per-scan (cos, sin) / misses of an insertion
    Host<float> h_pts;
    Device<int2> d_key, d_idx, d_ends, d_key_b;       // d_key_b: VOX_BATCH key slices (adaptive filter search)
    Device<unsigned char> d_keep, d_keep_b;           // d_keep_b: VOX_BATCH + 1 flag slices (the last one parks the current result)
    Device<int> d_counts, d_count, d_bad, d_box;
    Host<int> h_counts, h_count, h_box;
    Device<unsigned short> d_cells, d_hit, d_miss;    // grid; hit / miss lookup tables (uint16[32768])
    Device<unsigned short> d_cells2, d_tex;           // target of a growth (then swapped with d_cells) and texture staging; the texture's table
    Device<unsigned char> d_occ_tables;               // the occupancy grid's two byte tables (occupancy, then red), built on first use
    Device<unsigned char> d_occ;                      // ... and its interior block on the device, occ_bytes long, grown when a grid needs more
    size_t occ_bytes = 0;
    std::vector<unsigned char> h_occ;                 // the block on the host
    float tab_hit_p = -1.f, tab_miss_p = -1.f;        // probabilities the resident tables were built for
    Device<BestRec> d_bb, d_best;
    Host<BestRec> h_best;
    Device<RefineOut> d_refine;
    Host<RefineOut> h_refine;
    int nx = 0, ny = 0;                               // the grid
    double resolution = 0., max_x = 0., max_y = 0.;
    bool have_grid = false;
    std::string hip_error;
};

namespace {

// VoxelFilter(res).Filter on the device buffer `src` (n points) into `dst`; *m = survivors (synchronises)
int voxel_pass(rgrid_t *h, const float *src, int n, float res, float *dst, int *m)
{
    if (n == 0) { *m = 0; return RGRID_OK; }
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(kg_keys, dim3(blocks), dim3(256), 0, h->stream, src, n, res, h->d_key.d, h->d_keep.d);
    hipLaunchKernelGGL(kg_first, dim3(blocks, blocks), dim3(256), 0, h->stream, h->d_key.d, n, h->d_keep.d);
    hipLaunchKernelGGL(kg_compact, dim3(1), dim3(1024), 0, h->stream, src, h->d_keep.d, n, dst, h->d_count.d);
    G_TRY(h, hipMemcpyAsync(h->h_count.h, h->d_count.d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    *m = *h->h_count.h;
    return RGRID_OK;
}

// Survivor counts of VoxelFilter(res[r]) for r < R <= VOX_BATCH on the device cloud `src`, one round trip; the
// first-occurrence flags stay in slice r of d_keep_b for voxel_emit
int voxel_counts(rgrid_t *h, const float *src, int n, const float *res, int R, int *counts)
{
    VoxBatch B;
    B.r = R;
    for (int r = 0; r < R; ++r) B.res[r] = res[r];
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(kg_keys_b, dim3(blocks, R), dim3(256), 0, h->stream, src, n, B, h->d_key_b.d, h->d_keep_b.d);
    hipLaunchKernelGGL(kg_first_b, dim3(blocks, blocks, R), dim3(256), 0, h->stream, h->d_key_b.d, n, h->d_keep_b.d);
    hipLaunchKernelGGL(kg_count_b, dim3(R), dim3(256), 0, h->stream, h->d_keep_b.d, n, h->d_counts.d);
    G_TRY(h, hipMemcpyAsync(h->h_counts.h, h->d_counts.d, sizeof(int) * R, hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    for (int r = 0; r < R; ++r) counts[r] = h->h_counts.h[r];
    return RGRID_OK;
}

int upload_points(rgrid_t *h, const float *xy, int n)
{
    std::memcpy(h->h_pts.h, xy, sizeof(float) * 2 * (size_t)n);
    G_TRY(h, hipMemcpyAsync(h->d_in.d, h->h_pts.h, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    return RGRID_OK;
}

int download_points(rgrid_t *h, const float *d_src, int m, float *out_xy, int out_cap)
{
    if (m > out_cap) return RGRID_ERR_BUFFER;
    if (m > 0) {
        G_TRY(h, hipMemcpyAsync(h->h_pts.h, d_src, sizeof(float) * 2 * (size_t)m, hipMemcpyDeviceToHost, h->stream));
        G_TRY(h, hipStreamSynchronize(h->stream));
        std::memcpy(out_xy, h->h_pts.h, sizeof(float) * 2 * (size_t)m);
    }
    return RGRID_OK;
}

// Grid2D::ComputeCroppedLimits of the resident grid: kg_known_box and its round trip, box = (offset_x, offset_y, width, height)
int known_box(rgrid_t *h, int box[4])
{
    h->h_box.h[0] = h->h_box.h[1] = INT_MAX; h->h_box.h[2] = h->h_box.h[3] = -1;
    G_TRY(h, hipMemcpyAsync(h->d_box.d, h->h_box.h, 4 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(kg_known_box, dim3((h->nx + 255) / 256, h->ny), dim3(256), 0, h->stream, h->d_cells.d, h->nx, h->ny, h->d_box.d);
    G_TRY(h, hipMemcpyAsync(h->h_box.h, h->d_box.d, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    box_of_known(h->h_box.h, box);
    return RGRID_OK;
}

}  // namespace

extern "C" {

int rgrid_abi_version(void) { return RGRID_ABI_VERSION; }

int rgrid_draw_texture(rgrid_t *h, uint8_t *cells, long cap, int box[4], double slice_max[2])
{
    if (!h || !cells || !box || !slice_max || !h->have_grid) return RGRID_ERR_INVALID;
    G_TRY(h, hipSetDevice(h->device));
    G_TRY(h, resident_texture_table(h->d_tex.d));
    const int rc = known_box(h, box);
    if (rc != RGRID_OK) return rc;
    const int x0 = box[0], y0 = box[1], w = box[2], hh = box[3];
    slice_max_of(box, h->resolution, h->max_x, h->max_y, slice_max);
    if (2l * w * hh > cap) return RGRID_ERR_BUFFER;
    hipLaunchKernelGGL(kg_texture, dim3((w + 255) / 256, hh), dim3(256), 0, h->stream, h->d_cells.d, h->nx, x0, y0, w, h->d_tex.d, h->d_cells2.d);
    G_TRY(h, hipGetLastError());
    G_TRY(h, hipMemcpyAsync(cells, h->d_cells2.d, 2 * (size_t)w * hh, hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    return RGRID_OK;
}

int rgrid_occupancy_grid(rgrid_t *h, int mode, const double submap_origin[2], int8_t *out, long cap, int size[2], double origin[2], int box[4])
{
    if (!h || !submap_origin || !out || !size || !origin || !box || !h->have_grid || (mode != OCC_MODE_OCCUPANCY && mode != OCC_MODE_IMAGE))
        return RGRID_ERR_INVALID;
    G_TRY(h, hipSetDevice(h->device));
    G_TRY(h, resident_occupancy_tables(h->d_occ_tables.d));
    const size_t need = occupancy_block_bytes(h->nx, h->ny);
    if (need > h->occ_bytes) {
        h->d_occ.release();
        h->occ_bytes = 0;
        G_TRY(h, h->d_occ.alloc(need));
        h->occ_bytes = need;
    }
    int rc = known_box(h, box);
    if (rc != RGRID_OK) return rc;
    const int x0 = box[0], y0 = box[1], w = box[2], hh = box[3];
    OccupancyFrame F;
    rc = occupancy_frame(box, h->resolution, h->max_x, h->max_y, submap_origin, &F);
    if (rc != RGRID_OK) return rc;                                                // outside the domain: no image
    size[0] = F.size[0]; size[1] = F.size[1]; origin[0] = F.origin[0]; origin[1] = F.origin[1];
    if ((long)F.size[0] * F.size[1] > cap) return RGRID_ERR_BUFFER;
    const int stride = occupancy_stride(hh);
    const int tiles = ((w + OCC_T - 1) / OCC_T) * ((stride + OCC_T - 1) / OCC_T);
    hipLaunchKernelGGL(kg_occupancy, dim3((unsigned)(tiles < 65536 ? tiles : 65536)), dim3(256), 0, h->stream, h->d_cells.d, h->nx, x0, y0, w, hh,
                       h->d_occ_tables.d + (mode == OCC_MODE_IMAGE ? 32768 : 0), h->d_occ.d);
    G_TRY(h, hipGetLastError());
    const size_t bytes = (size_t)stride * (size_t)w;
    if (h->h_occ.size() < bytes) h->h_occ.resize(bytes);
    G_TRY(h, hipMemcpyAsync(h->h_occ.data(), h->d_occ.d, bytes, hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    occupancy_paint(mode, h->h_occ.data(), w, hh, F.size, reinterpret_cast<unsigned char *>(out));
    return RGRID_OK;
}

int rgrid_refine_match(rgrid_t *h, const rgrid_refine_options *opt, const double target_translation[2], const double initial_pose[3],
                       const float *points_xy, int n, double pose_estimate[3], rgrid_refine_summary *summary)
{
    if (!h || !opt || !target_translation || !initial_pose || !pose_estimate || n < 0 || (n > 0 && !points_xy)) return RGRID_ERR_INVALID;
    if (!h->have_grid || !refine_options_ok(opt)) return RGRID_ERR_INVALID;
    if (n == 0) return RGRID_ERR_EMPTY;
    if (n > h->max_points) return RGRID_ERR_CAPACITY;
    G_TRY(h, hipSetDevice(h->device));
    if (upload_points(h, points_xy, n) != RGRID_OK) return RGRID_ERR_HIP;
    RefineArgs A;
    refine_args(A, h->nx, h->ny, h->resolution, h->max_x, h->max_y, opt, n);
    A.tx = target_translation[0]; A.ty = target_translation[1];
    A.x0 = initial_pose[0]; A.y0 = initial_pose[1]; A.a0 = initial_pose[2];
    hipLaunchKernelGGL(kg_refine, dim3(1), dim3(refine_threads(n)), 0, h->stream, A, h->d_cells.d, h->d_in.d, h->d_refine.d);
    G_TRY(h, hipGetLastError());
    G_TRY(h, hipMemcpyAsync(h->h_refine.h, h->d_refine.d, sizeof(RefineOut), hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    pose_estimate[0] = h->h_refine.h->pose[0]; pose_estimate[1] = h->h_refine.h->pose[1]; pose_estimate[2] = h->h_refine.h->pose[2];
    if (summary) {
        summary->initial_cost = h->h_refine.h->initial_cost; summary->final_cost = h->h_refine.h->final_cost;
        summary->iterations = h->h_refine.h->iterations; summary->termination = h->h_refine.h->termination;
    }
    return RGRID_OK;
}

#ifdef RGRID_DEBUG_TIMING
int rgrid_debug_refine_cycles(rgrid_t *h, long long out[16])
{
    for (int k = 0; k < 16; ++k) out[k] = h->h_refine.h->dbg[k];
    return RGRID_OK;
}
#endif

const char *rgrid_strerror(int code)
{
    switch (code) {
    case RGRID_OK: return "ok";
    case RGRID_ERR_INVALID: return "invalid argument";
    case RGRID_ERR_HIP: return "HIP runtime error";
    case RGRID_ERR_CAPACITY: return "capacity of the handle exceeded";
    case RGRID_ERR_BUFFER: return "caller buffer too small";
    case RGRID_ERR_EMPTY: return "empty point cloud";
    default: return "unknown error";
    }
}

const char *rgrid_last_hip_error(rgrid_t *h) { return h ? h->hip_error.c_str() : ""; }

int rgrid_create(int max_points, int max_cells, int max_candidates, int device, rgrid_t **out)
{
    if (!out || max_points < 1 || max_cells < 1 || max_candidates < 1) return RGRID_ERR_INVALID;
    *out = nullptr;
    rgrid_t *h = new (std::nothrow) rgrid();
    if (!h) return RGRID_ERR_INVALID;
    h->max_points = max_points; h->max_cells = max_cells; h->max_candidates = max_candidates; h->device = device;
    const size_t np = (size_t)max_points;
    // discretised scans: every candidate's scan must fit: num_scans <= max_candidates, num_scans * n <= np * scans_cap
    int rc = [&]() -> int {
        G_TRY(h, hipSetDevice(device));
        G_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        G_TRY(h, h->d_in.alloc(2 * np)); G_TRY(h, h->d_a.alloc(2 * np)); G_TRY(h, h->d_b.alloc(2 * np));
        G_TRY(h, h->d_key.alloc(np + 8)); G_TRY(h, hipMemset(h->d_key.d, 0, 8 * np + 64)); G_TRY(h, h->d_keep.alloc(np));   // + one read-ahead group (64 bytes)
        G_TRY(h, h->d_key_b.alloc(np * VOX_BATCH + 8)); G_TRY(h, hipMemset(h->d_key_b.d, 0, 8 * np * VOX_BATCH + 64)); G_TRY(h, h->d_keep_b.alloc(np * (VOX_BATCH + 1)));
        G_TRY(h, h->d_counts.alloc(VOX_BATCH)); G_TRY(h, h->h_counts.alloc(VOX_BATCH));
        G_TRY(h, h->d_cs.alloc(2 * (size_t)max_candidates));
        G_TRY(h, h->d_idx.alloc(np * 1024 + 64));                                // up to 1024 rotated scans of max_points points (+ read-ahead pad)
        G_TRY(h, hipMemset(h->d_idx.d, 0, 8 * (np * 1024 + 64)));
        G_TRY(h, h->d_cells.alloc((size_t)max_cells)); G_TRY(h, h->d_cells2.alloc((size_t)max_cells));
        G_TRY(h, h->d_hit.alloc(32768)); G_TRY(h, h->d_miss.alloc(32768));
        G_TRY(h, h->d_mis.alloc(2 * np)); G_TRY(h, h->d_ends.alloc(2 * np + 1)); G_TRY(h, h->d_bad.alloc(1));
        G_TRY(h, h->d_bb.alloc(1024));                                           // one record per rotated scan
        G_TRY(h, h->d_best.alloc(1)); G_TRY(h, h->d_count.alloc(1));
        G_TRY(h, h->h_pts.alloc(2 * np)); G_TRY(h, h->h_count.alloc(1)); G_TRY(h, h->h_best.alloc(1));
        G_TRY(h, h->d_box.alloc(4)); G_TRY(h, h->h_box.alloc(4));
        G_TRY(h, h->d_refine.alloc(1)); G_TRY(h, h->h_refine.alloc(1));
        return RGRID_OK;
    }();
    if (rc != RGRID_OK) { std::fprintf(stderr, "rgrid_create: %s\n", h->hip_error.c_str()); rgrid_destroy(h); return rc; }
    *out = h;
    return RGRID_OK;
}

void rgrid_destroy(rgrid_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    batch_host::release_all(h->d_in, h->d_a, h->d_b, h->d_cs, h->d_mis, h->h_pts, h->d_key, h->d_idx, h->d_ends, h->d_key_b, h->d_keep, h->d_keep_b, h->d_counts,
                            h->d_count, h->d_bad, h->d_box, h->h_counts, h->h_count, h->h_box, h->d_cells, h->d_hit, h->d_miss, h->d_cells2, h->d_tex,
                            h->d_occ_tables, h->d_occ, h->d_bb, h->d_best, h->h_best, h->d_refine, h->h_refine);   // the struct's members, in its order
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int rgrid_voxel_filter(rgrid_t *h, const float *xy, int n, float resolution, float *out_xy, int out_cap, int *m)
{
    if (!h || !m || n < 0 || (n > 0 && !xy) || !(resolution > 0.f) || out_cap < 0 || (out_cap > 0 && !out_xy)) return RGRID_ERR_INVALID;
    *m = 0;
    if (n == 0) return RGRID_OK;
    if (n > h->max_points) return RGRID_ERR_CAPACITY;
    G_TRY(h, hipSetDevice(h->device));
    int rc = upload_points(h, xy, n);
    if (rc != RGRID_OK) return rc;
    int cnt = 0;
    rc = voxel_pass(h, h->d_in.d, n, resolution, h->d_a.d, &cnt);
    if (rc != RGRID_OK) return rc;
    rc = download_points(h, h->d_a.d, cnt, out_xy, out_cap);
    if (rc != RGRID_OK) return rc;
    *m = cnt;
    return RGRID_OK;
}

int rgrid_adaptive_voxel_filter(rgrid_t *h, const float *xy, int n, double max_length, double min_num_points,
                                double max_range, float *out_xy, int out_cap, int *m)
{
    if (!h || !m || n < 0 || (n > 0 && !xy) || !(max_length > 0.) || out_cap < 0 || (out_cap > 0 && !out_xy)) return RGRID_ERR_INVALID;
    *m = 0;
    if (n == 0) return RGRID_OK;
    if (n > h->max_points) return RGRID_ERR_CAPACITY;
    G_TRY(h, hipSetDevice(h->device));
    int rc = upload_points(h, xy, n);
    if (rc != RGRID_OK) return rc;
    // FilterByMaxRange (voxel_filter.cc:15-27) -> d_key is free here, the gated cloud goes to d_in's twin: reuse d_b as "in"
    hipLaunchKernelGGL(kg_range_gate, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_in.d, n, (float)max_range, h->d_keep.d);
    hipLaunchKernelGGL(kg_compact, dim3(1), dim3(1024), 0, h->stream, h->d_in.d, h->d_keep.d, n, h->d_b.d, h->d_count.d);
    G_TRY(h, hipMemcpyAsync(h->h_count.h, h->d_count.d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    const int ni = *h->h_count.h;
    const float *src = h->d_b.d;                 // the gated cloud
    int cnt = ni;
    const float *final_buf = src;
    // AdaptivelyVoxelFiltered (voxel_filter.cc:29-76).  Its decisions only need the survivor COUNT of a voxel size, and
    // the sizes it can ask for are known in advance: the halving ladder (:47-48) and, between the bracketing pair, the
    // bisection tree (:57-70).  So the ladder is one batched launch and the tree is evaluated a few levels at a time
    // (every node of those levels at once), the host walks the answers: 3-4 round trips instead of a dozen, and the
    // point set is compacted once, for the size the search ends on.
    if (!((double)ni <= min_num_points)) {                                         // :33-37
        const float maxl = (float)max_length;
        float ladder[VOX_BATCH];
        int counts[VOX_BATCH];
        int R = 0;
        ladder[R++] = maxl;                                                        // :38
        for (float high = maxl; high > 1e-2f * maxl && R < VOX_BATCH; high /= 2.f) ladder[R++] = high / 2.f;   // :47-50
        rc = voxel_counts(h, src, ni, ladder, R, counts);
        if (rc != RGRID_OK) return rc;
        int slot = R - 1;                                                          // nothing dense enough: the last size tried (:75)
        if ((double)counts[0] >= min_num_points) slot = 0;                         // :39-43
        else {
            int k = 1;
            while (k < R && !((double)counts[k] >= min_num_points)) ++k;
            if (k < R) {
                slot = k;
                float low = ladder[k], high = (k == 1) ? maxl : ladder[k - 1];     // high of that iteration = the previous low
                unsigned char *park = h->d_keep_b.d + (size_t)VOX_BATCH * ni;        // `result` while later batches reuse the slices
                bool parked = false;
                const int depth = ni <= 4096 ? 5 : (ni <= 8192 ? 3 : 2);
                while ((high - low) / low > 1e-1f) {                               // :57
                    // the next `depth` levels of the bisection tree under (low, high), breadth first
                    struct Node { float low, high, mid; int yes, no; };
                    Node nodes[VOX_BATCH];
                    int nn = 0, level_begin = 0;
                    nodes[nn++] = Node{low, high, (low + high) / 2.f, -1, -1};
                    for (int lv = 1; lv < depth; ++lv) {
                        const int level_end = nn;
                        for (int q = level_begin; q < level_end; ++q) {
                            const Node nd = nodes[q];
                            if ((nd.high - nd.mid) / nd.mid > 1e-1f && nn < VOX_BATCH) {          // count(mid) >= min: low = mid
                                nodes[q].yes = nn; nodes[nn++] = Node{nd.mid, nd.high, (nd.mid + nd.high) / 2.f, -1, -1};
                            }
                            if ((nd.mid - nd.low) / nd.low > 1e-1f && nn < VOX_BATCH) {            // else: high = mid
                                nodes[q].no = nn; nodes[nn++] = Node{nd.low, nd.mid, (nd.low + nd.mid) / 2.f, -1, -1};
                            }
                        }
                        level_begin = level_end;
                    }
                    float mids[VOX_BATCH];
                    for (int q = 0; q < nn; ++q) mids[q] = nodes[q].mid;
                    if (!parked) {                                                 // `result` lives in a slice the batch overwrites
                        G_TRY(h, hipMemcpyAsync(park, h->d_keep_b.d + (size_t)slot * ni, (size_t)ni, hipMemcpyDeviceToDevice, h->stream));
                        parked = true;
                    }
                    rc = voxel_counts(h, src, ni, mids, nn, counts);
                    if (rc != RGRID_OK) return rc;
                    int q = 0, chosen = -1;
                    while (q >= 0) {
                        const bool dense = (double)counts[q] >= min_num_points;
                        if (dense) { low = nodes[q].mid; chosen = q; } else high = nodes[q].mid;
                        q = dense ? nodes[q].yes : nodes[q].no;                    // -1: the loop condition failed there, or the depth ran out
                    }
                    if (chosen >= 0) {                                             // result = candidate (:63-66)
                        slot = chosen; parked = false;
                    }
                }
                if (parked) slot = VOX_BATCH;
            }
        }
        hipLaunchKernelGGL(kg_compact, dim3(1), dim3(1024), 0, h->stream, src, h->d_keep_b.d + (size_t)slot * ni, ni, h->d_a.d, h->d_count.d);
        G_TRY(h, hipMemcpyAsync(h->h_count.h, h->d_count.d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        G_TRY(h, hipStreamSynchronize(h->stream));
        cnt = *h->h_count.h;
        final_buf = h->d_a.d;
    }
    rc = download_points(h, final_buf, cnt, out_xy, out_cap);
    if (rc != RGRID_OK) return rc;
    *m = cnt;
    return RGRID_OK;
}

int rgrid_set_grid(rgrid_t *h, const uint16_t *cells, int num_x_cells, int num_y_cells, double resolution,
                   double max_x, double max_y)
{
    if (!h || !cells || num_x_cells < 1 || num_y_cells < 1 || !(resolution > 0.)) return RGRID_ERR_INVALID;
    if ((long long)num_x_cells * num_y_cells > h->max_cells) return RGRID_ERR_CAPACITY;
    G_TRY(h, hipSetDevice(h->device));
    G_TRY(h, hipMemcpyAsync(h->d_cells.d, cells, sizeof(uint16_t) * (size_t)num_x_cells * num_y_cells, hipMemcpyHostToDevice, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    h->nx = num_x_cells; h->ny = num_y_cells; h->resolution = resolution; h->max_x = max_x; h->max_y = max_y;
    h->have_grid = true;
    return RGRID_OK;
}

int rgrid_insert(rgrid_t *h, const float origin_xy[2], const float *returns_xy, int n_returns, const float *misses_xy,
                 int n_misses, float hit_probability, float miss_probability, int insert_free_space)
{
    if (!h || !origin_xy || !two_clouds_ok(returns_xy, n_returns, misses_xy, n_misses)) return RGRID_ERR_INVALID;
    if (!h->have_grid || !insert_options_ok(hit_probability, miss_probability)) return RGRID_ERR_INVALID;
    if (n_returns > h->max_points || n_misses > h->max_points) return RGRID_ERR_CAPACITY;
    G_TRY(h, hipSetDevice(h->device));
    G_TRY(h, insert_tables(hit_probability, miss_probability, h->d_hit.d, h->d_miss.d, h->tab_hit_p, h->tab_miss_p));
    if (n_returns > 0) {
        if (upload_points(h, returns_xy, n_returns) != RGRID_OK) return RGRID_ERR_HIP;
        G_TRY(h, hipStreamSynchronize(h->stream));                                   // h_pts is reused for the misses below
    }
    if (n_misses > 0) {
        std::memcpy(h->h_pts.h, misses_xy, sizeof(float) * 2 * (size_t)n_misses);
        G_TRY(h, hipMemcpyAsync(h->d_mis.d, h->h_pts.h, sizeof(float) * 2 * (size_t)n_misses, hipMemcpyHostToDevice, h->stream));
    }
    G_TRY(h, hipMemsetAsync(h->d_bad.d, 0, sizeof(int), h->stream));
    InsertArgs A;
    A.nx = h->nx; A.ny = h->ny; A.n_ret = n_returns; A.n_miss = n_misses;
    A.max_x = h->max_x; A.max_y = h->max_y; A.rs = h->resolution / SUBPX;
    A.ox = origin_xy[0]; A.oy = origin_xy[1];
    const int n = n_returns + n_misses;
    hipLaunchKernelGGL(kg_ends, dim3((n + 1 + 255) / 256), dim3(256), 0, h->stream, A, h->d_in.d, h->d_mis.d, h->d_ends.d, h->d_bad.d);
    if (n_returns > 0)
        hipLaunchKernelGGL(kg_hits, dim3((n_returns + 255) / 256), dim3(256), 0, h->stream, A, h->d_ends.d, h->d_bad.d, h->d_cells.d, h->d_hit.d);
    if (insert_free_space && n > 0)
        hipLaunchKernelGGL(kg_rays, dim3((n + 3) / 4), dim3(256), 0, h->stream, A, h->d_ends.d, h->d_bad.d, h->d_cells.d, h->d_miss.d);
    const long long ncells = (long long)h->nx * h->ny;
    hipLaunchKernelGGL(kg_finish, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, h->stream, h->d_cells.d, ncells, h->d_bad.d);
    G_TRY(h, hipMemcpyAsync(h->h_count.h, h->d_bad.d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    return *h->h_count.h ? RGRID_ERR_CAPACITY : RGRID_OK;
}

int rgrid_grow_as_needed(rgrid_t *h, const float origin_xy[2], const float *returns_xy, int n_returns, const float *misses_xy,
                         int n_misses)
{
    if (!h || !origin_xy || !two_clouds_ok(returns_xy, n_returns, misses_xy, n_misses) || !h->have_grid) return RGRID_ERR_INVALID;
    // the bounding box and Grid2D::GrowLimits for its corners, on the limits only (plan_growth of rgrid_dev.h)
    int nx = h->nx, ny = h->ny, off_x = 0, off_y = 0;
    double max_x = h->max_x, max_y = h->max_y;
    const int rc = plan_growth(origin_xy, returns_xy, n_returns, misses_xy, n_misses, h->resolution, h->max_cells, nx, ny, max_x, max_y, off_x, off_y);
    if (rc != RGRID_OK) return rc;
    if (nx == h->nx && ny == h->ny) return RGRID_OK;
    G_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(kg_grow, dim3((nx + 255) / 256, ny), dim3(256), 0, h->stream, h->d_cells.d, h->nx, h->ny, h->d_cells2.d, nx, ny, off_x, off_y);
    G_TRY(h, hipGetLastError());
    G_TRY(h, hipStreamSynchronize(h->stream));
    std::swap(h->d_cells.d, h->d_cells2.d);
    h->nx = nx; h->ny = ny; h->max_x = max_x; h->max_y = max_y;
    return RGRID_OK;
}

int rgrid_get_limits(rgrid_t *h, int *num_x_cells, int *num_y_cells, double *resolution, double *max_x, double *max_y)
{
    if (!h || !h->have_grid) return RGRID_ERR_INVALID;
    if (num_x_cells) *num_x_cells = h->nx;
    if (num_y_cells) *num_y_cells = h->ny;
    if (resolution) *resolution = h->resolution;
    if (max_x) *max_x = h->max_x;
    if (max_y) *max_y = h->max_y;
    return RGRID_OK;
}

int rgrid_get_grid(rgrid_t *h, uint16_t *cells, long cap)
{
    if (!h || !cells || !h->have_grid) return RGRID_ERR_INVALID;
    const long long ncells = (long long)h->nx * h->ny;
    if (cap < ncells) return RGRID_ERR_BUFFER;
    G_TRY(h, hipSetDevice(h->device));
    G_TRY(h, hipMemcpyAsync(cells, h->d_cells.d, sizeof(uint16_t) * (size_t)ncells, hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));
    return RGRID_OK;
}

int rgrid_match(rgrid_t *h, const rgrid_match_options *opt, const double initial_pose[3], const float *points_xy,
                int n, double pose_estimate[3], double *score, int best3[3], int info3[3])
{
#pragma clang fp contract(off)
    if (!h || !opt || !initial_pose || !pose_estimate || !score || n < 0 || (n > 0 && !points_xy)) return RGRID_ERR_INVALID;
    if (!h->have_grid) return RGRID_ERR_INVALID;
    if (n == 0) return RGRID_ERR_EMPTY;
    if (n > h->max_points) return RGRID_ERR_CAPACITY;
    G_TRY(h, hipSetDevice(h->device));
    MatchPlan P;
    if (plan_match(opt, h->resolution, initial_pose, points_xy, n, h->h_pts.h, &P) != RGRID_OK || P.num_scans > 1024 || P.ncand > h->max_candidates)
        return RGRID_ERR_CAPACITY;
    std::vector<float> cs(2 * (size_t)P.num_scans);
    rotation_table(P, cs.data());
    G_TRY(h, hipMemcpyAsync(h->d_in.d, h->h_pts.h, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    G_TRY(h, hipMemcpyAsync(h->d_cs.d, cs.data(), sizeof(float) * cs.size(), hipMemcpyHostToDevice, h->stream));
    MatchArgs A;
    A.n = n; A.num_scans = P.num_scans; A.num_linear = P.num_linear; A.nx = h->nx; A.ny = h->ny;
    A.tx = (float)initial_pose[0]; A.ty = (float)initial_pose[1];
    A.resolution = P.res; A.max_x = h->max_x; A.max_y = h->max_y;
    A.num_angular_d = (double)P.num_angular; A.step = P.step;
    A.wt = opt->translation_delta_cost_weight; A.wr = opt->rotation_delta_cost_weight;
    const int nb_d = (P.num_scans * n + 255) / 256, nb_s = P.num_scans;
    hipLaunchKernelGGL(kg_discretize, dim3(nb_d), dim3(256), 0, h->stream, A, h->d_in.d, h->d_cs.d, h->d_idx.d);
    hipLaunchKernelGGL(kg_score, dim3(nb_s), dim3(128), 0, h->stream, A, h->d_idx.d, h->d_cells.d, h->d_bb.d);
    hipLaunchKernelGGL(kg_best, dim3(1), dim3(256), 0, h->stream, h->d_bb.d, nb_s, h->d_best.d);
    G_TRY(h, hipMemcpyAsync(h->h_best.h, h->d_best.d, sizeof(BestRec), hipMemcpyDeviceToHost, h->stream));
    G_TRY(h, hipStreamSynchronize(h->stream));                                            // cs stays alive until here
    decode_best(P, initial_pose, *h->h_best.h, pose_estimate, score, best3, info3);
    return RGRID_OK;
}

// ---- mapping::MapBuilder::AddRangeData (src/mapping/map_builder.cc:57-108) as one call ------------------------------
// Host side = what the reference's host does between the steps: a few rigid transforms (its float32 round trips
// through Eigen quaternions restated operation by operation, as in reflector_ekf_slam_amd/map_builder.py) and the
// decisions; every per-point / per-cell step is one of the entry points above.  The transforms and compositions themselves are
// rgrid_dev.h's, shared with rgrid_batch_add_range_data.
int rgrid_add_range_data(rgrid_t *h, const rgrid_map_builder_options *opt, const float origin_xy[2], const float *returns_xy,
                         int n_returns, const float *misses_xy, int n_misses, const double ekf_pose[3], double local_pose[3],
                         float *returns_in_local, int *status)
{
#pragma clang fp contract(off)
    if (!h || !opt || !origin_xy || !ekf_pose || !local_pose || !two_clouds_ok(returns_xy, n_returns, misses_xy, n_misses)) return RGRID_ERR_INVALID;
    if (status) *status = RGRID_SCAN_DROPPED_EMPTY;
    if (n_returns == 0) return RGRID_OK;                                          // "Dropped empty horizontal range data." (:63-67)
    if (n_returns > h->max_points || n_misses > h->max_points) return RGRID_ERR_CAPACITY;
    // TransformToGravityAlignedFrameAndFilter (:20-32): Rotation(q).cast<float>() -> Project2D -> Rigid2f(0, GetYaw)
    double qw, qz;
    float yaw_g;
    gravity_alignment(ekf_pose[2], qw, qz, yaw_g);
    std::vector<float> ret((size_t)2 * n_returns), mis((size_t)2 * (n_misses > 0 ? n_misses : 1)), fr((size_t)2 * n_returns),
        fm((size_t)2 * (n_misses > 0 ? n_misses : 1)), av((size_t)2 * n_returns);
    rigid2f_apply(0.f, 0.f, yaw_g, returns_xy, n_returns, ret.data());
    if (n_misses > 0) rigid2f_apply(0.f, 0.f, yaw_g, misses_xy, n_misses, mis.data());
    int nfr = 0, nfm = 0, nav = 0;
    int rc = rgrid_voxel_filter(h, ret.data(), n_returns, opt->voxel_filter_size, fr.data(), n_returns, &nfr);
    if (rc != RGRID_OK) return rc;
    if (n_misses > 0) { rc = rgrid_voxel_filter(h, mis.data(), n_misses, opt->voxel_filter_size, fm.data(), n_misses, &nfm); if (rc != RGRID_OK) return rc; }
    // pose_prediction = Project2D(ekf_pose * gravity_alignment.inverse()): the rotations cancel (:70-71)
    const double prediction[3] = {ekf_pose[0], ekf_pose[1], 0.0};
    rc = rgrid_adaptive_voxel_filter(h, fr.data(), nfr, opt->adaptive_max_length, opt->adaptive_min_num_points, opt->adaptive_max_range,
                                     av.data(), n_returns, &nav);
    if (rc != RGRID_OK) return rc;
    if (status) *status = RGRID_SCAN_FILTERED_EMPTY;
    if (nav == 0) return RGRID_OK;                                               // (:74-77)
    double est[3] = {prediction[0], prediction[1], prediction[2]};               // ScanMatch (:34-55): no submap yet -> the prediction
    if (h->have_grid) {
        double coarse[3], score = 0;
        rc = rgrid_match(h, &opt->match, prediction, av.data(), nav, coarse, &score, nullptr, nullptr);
        if (rc != RGRID_OK) return rc;
        rc = rgrid_refine_match(h, &opt->refine, prediction, coarse, av.data(), nav, est, nullptr);
        if (rc != RGRID_OK) return rc;
    }
    // pose_estimate = Embed3D(pose_estimate_2d) * gravity_alignment (:86-87): the raw returns move by it (:89-90), the filtered data by yaw2 (:92-94)
    float yaw_f32, yaw2, org2[2];
    compose_pose_estimate(est, qw, qz, local_pose, yaw_f32, yaw2);
    if (returns_in_local) rigid2f_apply((float)est[0], (float)est[1], yaw_f32, returns_xy, n_returns, returns_in_local);
    origin_in_local(origin_xy, yaw_g, est, yaw2, org2);
    rigid2f_apply((float)est[0], (float)est[1], yaw2, fr.data(), nfr, ret.data());
    if (nfm > 0) rigid2f_apply((float)est[0], (float)est[1], yaw2, fm.data(), nfm, mis.data());
    if (!h->have_grid) {                                                          // InsertIntoSubmap / CreateGrid (:110-126)
        int nx, ny;
        double resolution, max_x, max_y;
        rc = initial_submap_limits(opt->resolution, org2, h->max_cells, nx, ny, resolution, max_x, max_y);
        if (rc != RGRID_OK) return rc;
        G_TRY(h, hipSetDevice(h->device));
        G_TRY(h, hipMemsetAsync(h->d_cells.d, 0, sizeof(uint16_t) * (size_t)nx * ny, h->stream));
        G_TRY(h, hipStreamSynchronize(h->stream));
        h->nx = nx; h->ny = ny; h->resolution = resolution; h->max_x = max_x; h->max_y = max_y;
        h->have_grid = true;
    }
    rc = rgrid_grow_as_needed(h, org2, ret.data(), nfr, nfm > 0 ? mis.data() : nullptr, nfm);
    if (rc != RGRID_OK) return rc;
    rc = rgrid_insert(h, org2, ret.data(), nfr, nfm > 0 ? mis.data() : nullptr, nfm, opt->hit_probability, opt->miss_probability,
                      opt->insert_free_space);
    if (rc != RGRID_OK) return rc;
    if (status) *status = RGRID_SCAN_INSERTED;
    return RGRID_OK;
}

}  // extern "C"
