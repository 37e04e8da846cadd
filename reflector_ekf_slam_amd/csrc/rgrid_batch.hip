// rgrid_batch.hip -- the real-time correlative scan matcher for a fleet: one scan of each of B robots matched by ONE launch
// (rgrid_batch_* of include/rgrid.h), against resident probability grids that any number of the scans may share.
//
// Every scan of a call is one scan_matching::RealTimeCorrelativeScanMatcher2D::Match (reference
// src/scan_matching/real_time_correlative_scan_matcher_2d.cc:84-118) and gives the bits rgrid_match gives: the host plans each
// scan and decodes its winner through the functions rgrid_match calls (plan_match, rotation_table, decode_best of rgrid_dev.h:
// one text), the device does what kg_discretize, kg_score and kg_best do (a text of its own) -- in
//   kgb_match   ONE workgroup per (scan, rotated scan): a call of B default-option scans is about 107 B workgroups.  The
//               workgroup discretises its own rotated scan into LDS (kg_discretize's arithmetic, 8 B per point), then scores its
//               (2 num_linear + 1)^2 translation candidates as kg_score does: one lane per candidate, passes of 128, the float32
//               sum in point order with the cell values of sixteen points in flight before their additions, the FP64 exp penalty.
// Nobody waits for anybody.  The arg-max over a scan's rotated scans is taken by whichever of its workgroups finishes LAST: every
// workgroup writes its best through to memory, waits for the acknowledgement, and only then counts itself in on the scan's
// arrival counter; the one that reads num_scans - 1 there knows all of them have landed, reads them past its own L2 (the XCDs'
// L2s are not coherent inside a launch), reduces, resets the counter and writes the scan's result slot (k3f_front's hand-over,
// det3d.hip).  A batch larger than the chip queues workgroups, and a queued workgroup needs nothing from a running one.
// rgrid_batch_set_reduction(RGRID_BATCH_REDUCE_LAUNCH) takes the arg-max in a second launch, kgb_best, instead (one workgroup per
// scan): the form this was measured against.
//
// The second step of MapBuilder::ScanMatch, CeresScanMatcher2D::Match, for a batch is kgb_refine further down: one workgroup per
// scan runs kg_refine's solve (the device text of rgrid_refine_dev.h), alone (rgrid_batch_refine_*) or right behind the match on the
// same stream, starting from the winner the match published (rgrid_batch_scan_match_*).
//
// MapBuilder::AddRangeData itself for a batch is rgrid_batch_add_range_data at the end of this file: the stages above -- the filter
// (kgb_filter<true>, which rotates the raw clouds into the gravity-aligned frame as it loads them), match and refinement, the
// insert -- in ONE synchronous call, with the host composing the poses between them as rgrid_add_range_data does, and kgb_to_local
// for the raw returns in the local frame.  It packs, stages and launches through the functions the single-kind
// submits call; there is one text of each, and the host steps it has in common with the single handle (checks, launch shapes, resident
// tables, slice_max_of, AddRangeData's compositions) are rgrid_dev.h's.
//
// Per-call data -- a record per scan, the workgroup -> (record, rotation) map, the rotation tables and the rotated points --
// is packed into one of two staging segments that the kernel reads in place: fine-grained device memory the host writes
// directly where the platform maps it, else pinned host memory (host_visible.h).  Results land in pinned host memory, a slot
// per scan, published by the end of the launch.
#include "../../include/rgrid.h"
#include "batch_host.h"
#include "rgrid_dev.h"
#include "rgrid_refine_dev.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace {

#define KGB_PF 16                         // points whose cell values are in flight together (= KG_PF of rgrid.hip)
#define KGB_THREADS 128
#define KGB_MAX_ROT 1024                  // rgrid_match's limit on rotated scans
#define KGB_SEGMENTS 2
#define KGB_MAX_POINTS 16384             // 8 B of LDS per point: 128 KB of gfx950's 160 KB

// One runnable scan of a call.  An array of these lies at the start of the call's segment; offsets count from the segment's start.
struct BatchRec {
    double resolution, max_x, max_y;      // MapLimits of its grid
    double num_angular_d, step;           // orientation = (rotation - num_angular) * step
    double wt, wr;
    long long cells_off;                  // its grid's first cell in the grid pool
    int n, num_scans, num_linear, nx, ny;
    int pts_off;                          // float2 index of its rotated points (n of them)
    int cs_off;                           // float2 index of its (cos, sin) table (num_scans of them)
    float tx, ty;                         // Eigen::Translation2f(initial translation)
};

struct BatchBufs {
    const unsigned char *seg;             // the call's segment: BatchRec[nrec] | int2 wgmap[nwg] | float2 area
    int wgmap_off;                        // byte offset of the workgroup map
    int f2_off;                           // byte offset of the float2 area
    const unsigned short *cells;          // grid pool, num_grids * max_cells
    unsigned long long *bb;               // [max_scans][max_rotations]: block bests as (score bits << 32 | id)
    int *arrived;                         // [max_scans]: arrival counters, 0 between launches
    BestRec *out;                         // [max_scans], pinned host memory
    int max_rotations;
};

__device__ static inline unsigned long long best_bits(float score, int id)
{
    return ((unsigned long long)__float_as_uint(score) << 32) | (unsigned)id;
}

// workgroup arg-max of (best, bid) with the first-maximum rule; the result is valid in thread 0
__device__ static inline void wg_first_max(float &best, int &bid, float *s_sc, int *s_id)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const float os = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bid, off, 64);
        if (best_before(os, oi, best, bid)) { best = os; bid = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_sc[wave] = best; s_id[wave] = bid; }
    __syncthreads();
    if (threadIdx.x == 0 && best_before(s_sc[1], s_id[1], best, bid)) { best = s_sc[1]; bid = s_id[1]; }
}

// arg-max over the block bests of one scan (all KGB_THREADS threads), read past this CU's caches when DEV
template <bool DEV>
__device__ static inline void reduce_scan(const unsigned long long *bb, int num_scans, BestRec *out, float *s_sc, int *s_id)
{
    float best = -1.f; int bid = 0x7fffffff;
    for (int b = threadIdx.x; b < num_scans; b += KGB_THREADS) {
        const unsigned long long v = DEV ? __hip_atomic_load(&bb[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : bb[b];
        const float os = __uint_as_float((unsigned)(v >> 32));
        const int oi = (int)(unsigned)v;
        if (best_before(os, oi, best, bid)) { best = os; bid = oi; }
    }
    __syncthreads();                                                               // s_sc / s_id are free again
    wg_first_max(best, bid, s_sc, s_id);
    if (threadIdx.x == 0) { out->score = best; out->id = bid; }
}

template <bool ARRIVAL>
__global__ __launch_bounds__(KGB_THREADS) void kgb_match(BatchBufs B)
{
#pragma clang fp contract(off)
    extern __shared__ int2 s_idx[];                                                // the rotated scan's cell indices, padded to KGB_PF
    __shared__ float s_sc[2];
    __shared__ int s_id[2];
    __shared__ int s_last;
    const int2 wg = reinterpret_cast<const int2 *>(B.seg + B.wgmap_off)[blockIdx.x];
    const int rec = wg.x, scan = wg.y;
    const BatchRec &A = reinterpret_cast<const BatchRec *>(B.seg)[rec];
    const float2 *__restrict__ f2 = reinterpret_cast<const float2 *>(B.seg + B.f2_off);
    const int n = A.n, num_linear = A.num_linear, nx = A.nx, ny = A.ny;
    const unsigned short *__restrict__ cells = B.cells + A.cells_off;
    // ---- kg_discretize for this rotated scan (correlative_scan_matcher_2d.cc:86-123)
    {
        const float2 cs = f2[A.cs_off + scan];
        const float c = cs.x, s = cs.y, tx = A.tx, ty = A.ty;
        const double max_x = A.max_x, max_y = A.max_y, resolution = A.resolution;
        const int npad = (n + KGB_PF - 1) / KGB_PF * KGB_PF;
        for (int p = threadIdx.x; p < npad; p += KGB_THREADS) {
            int2 v = make_int2(0, 0);
            if (p < n) {
                const float2 pt = f2[A.pts_off + p];
                const float x = pt.x, y = pt.y;
                const float rx = c * x - s * y, ry = s * x + c * y;                  // Rotation2Df * point (:95-98)
                const float px = rx + tx, py = ry + ty;                             // Affine2f(initial_translation) * point (:117-118)
                v = cell_index_of(max_x, max_y, resolution, px, py);
            }
            s_idx[p] = v;
        }
    }
    __syncthreads();
    // ---- kg_score: one lane per translation candidate of this rotated scan
    const int W = 2 * num_linear + 1, WW = W * W;
    const double orientation = ((double)scan - A.num_angular_d) * A.step;
    const double resolution = A.resolution, wt = A.wt, wr = A.wr;
    float best = -1.f; int bid = 0x7fffffff;
    for (int r0 = 0; r0 < WW; r0 += KGB_THREADS) {                                  // 81 candidates per scan with the default window: one pass
        const int r = r0 + threadIdx.x;
        const bool live = r < WW;
        const int xo = (live ? r / W : 0) - num_linear, yo = (live ? r - (r / W) * W : 0) - num_linear;   // order: x offset, y offset (:64-74)
        float sum = 0.f;
        for (int p0 = 0; p0 < n; p0 += KGB_PF) {                                    // ComputeCandidateScore (:20-36), point order
            unsigned short v[KGB_PF];
            bool in[KGB_PF];
#pragma unroll
            for (int u = 0; u < KGB_PF; ++u) {
                const int2 c = s_idx[p0 + u];                                       // the same address in every lane: an LDS broadcast
                const int cx = c.x + xo, cy = c.y + yo;
                in[u] = cx >= 0 && cy >= 0 && cx < nx && cy < ny;
                v[u] = cells[in[u] ? nx * cy + cx : 0];                             // unconditional load (clamped address), as kg_score
            }
#pragma unroll
            for (int u = 0; u < KGB_PF; ++u)
                if (p0 + u < n) sum += in[u] ? value_to_probability(v[u]) : 0.1f;    // outside the grid: kMinProbability
        }
        sum /= (float)n;
        const double x = -yo * resolution, y = -xo * resolution;                    // Candidate2D (correlative_scan_matcher_2d.h:62-66)
        const double a = hypot(x, y) * wt + fabs(orientation) * wr;
        const float score = (float)((double)sum * exp(-(a * a)));                   // :127-133
        const int id = scan * WW + r;
        if (live && best_before(score, id, best, bid)) { best = score; bid = id; }
    }
    wg_first_max(best, bid, s_sc, s_id);
    unsigned long long *bb = B.bb + (size_t)rec * B.max_rotations;
    if (!ARRIVAL) {
        if (threadIdx.x == 0) bb[scan] = best_bits(best, bid);                      // kgb_best reads it after the kernel boundary
        return;
    }
    // ---- the workgroup of this scan that arrives last takes the arg-max over the rotated scans
    if (threadIdx.x == 0) {
        __hip_atomic_store(&bb[scan], best_bits(best, bid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                            // the store has been acknowledged
        const int before = __hip_atomic_fetch_add(&B.arrived[rec], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = before == A.num_scans - 1;
        if (s_last) __hip_atomic_store(&B.arrived[rec], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (for the next call)
    }
    __syncthreads();
    if (!s_last) return;
    reduce_scan<true>(bb, A.num_scans, &B.out[rec], s_sc, s_id);
}

// RGRID_BATCH_REDUCE_LAUNCH: one workgroup per scan after kgb_match<false>
__global__ __launch_bounds__(KGB_THREADS) void kgb_best(BatchBufs B)
{
    __shared__ float s_sc[2];
    __shared__ int s_id[2];
    const int rec = blockIdx.x;
    const BatchRec &A = reinterpret_cast<const BatchRec *>(B.seg)[rec];
    reduce_scan<false>(B.bb + (size_t)rec * B.max_rotations, A.num_scans, &B.out[rec], s_sc, s_id);
}

// ---------------------------------------------------------------------------------------------------------------
// CeresScanMatcher2D::Match for a batch: ONE workgroup per scan runs the whole of kg_refine (rgrid.hip) for its scan, against
// the scan's resident grid slot and its raw tracking-frame points in the call's segment.  The device text is rgrid_refine_dev.h's.
// One runnable scan of a refine call; an array of these lies at rrec_off of the call's segment.
struct RefineRec {
    RefineArgs A;                         // grid limits, weights, n; the poses too when the host knows them (match_rec < 0)
    long long cells_off;                  // its grid's first cell in the grid pool
    double plan_res, plan_step, ip[3];    // chained form: decode_candidate's inputs (the match's plan, the prediction)
    int pts_off;                          // float2 index of its raw points in the raw area (A.n of them)
    int match_rec;                        // chained form: the match's record whose winner is the start pose; else -1
    int num_linear, num_angular;
};

struct RefineBufs {
    const unsigned char *seg;             // the call's segment: ... | RefineRec[nrec] at rrec_off | raw float2 points at raw_off
    int rrec_off, raw_off;
    const unsigned short *cells;          // grid pool
    const BestRec *best;                  // [max_scans]: where kgb_match / kgb_best publish a scan's winner
    RefineOut *out;                       // [max_scans], pinned host memory
};

// The launch's block size is the largest scan's thread count.  A workgroup sums with ITS scan's count T = min(1024, roundup64(n))
// and nw = T / 64 wave partials, as rgrid_refine_match launches kg_refine for that scan: waves above T evaluate nothing and write
// no partial sums, but stand in every barrier to the last one.  No workgroup waits for another.
__global__ __launch_bounds__(1024) void kgb_refine(RefineBufs B)
{
#pragma clang fp contract(off)
    __shared__ double part[16][10];
    __shared__ RefineState st;
    const RefineRec &R = reinterpret_cast<const RefineRec *>(B.seg + B.rrec_off)[blockIdx.x];
    RefineArgs A = R.A;
    if (R.match_rec >= 0) {                                                      // MapBuilder::ScanMatch (map_builder.cc:49-53)
        const double ip[3] = {R.ip[0], R.ip[1], R.ip[2]};
        int sxy[3];
        double pose[3];
        decode_candidate(R.num_linear, R.num_angular, R.plan_res, R.plan_step, ip, B.best[R.match_rec].id, sxy, pose);
        A.tx = ip[0]; A.ty = ip[1];
        A.x0 = pose[0]; A.y0 = pose[1]; A.a0 = pose[2];
    }
    const unsigned short *__restrict__ cells = B.cells + R.cells_off;
    const float *__restrict__ pts = reinterpret_cast<const float *>(B.seg + B.raw_off) + 2 * (size_t)R.pts_off;
    const unsigned T = (unsigned)min(1024, ((A.n + 63) / 64) * 64);
    const int nw = (int)(T >> 6);
    const bool live = threadIdx.x < T;                                           // whole waves: T is a multiple of 64
    if (live) refine_eval_strided(A, cells, pts, A.x0, A.y0, A.a0, part, T);     // IterationZero
    __syncthreads();
    double S[10];
    if (threadIdx.x < 64) {
        const double x[3] = {A.x0, A.y0, A.a0};
        refine_totals(A, part, nw, x, S);
    }
    if (threadIdx.x == 0) refine_begin(A, st, S);
    __syncthreads();
    while (!st.done) {
        const double c0 = st.xc[0], c1 = st.xc[1], c2 = st.xc[2];
        if (live) refine_eval_strided(A, cells, pts, c0, c1, c2, part, T);
        __syncthreads();
        if (threadIdx.x < 64) {
            const double xc[3] = {c0, c1, c2};
            refine_totals(A, part, nw, xc, S);
        }
        if (threadIdx.x == 0) {
            refine_judge(A, st, S);
            if (!st.done) refine_next_candidate(A, st);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        RefineOut *out = &B.out[blockIdx.x];
        out->pose[0] = st.best[0]; out->pose[1] = st.best[1]; out->pose[2] = st.best[2];
        out->initial_cost = st.initial_cost; out->final_cost = st.min_cost; out->iterations = st.iter; out->termination = st.termination;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// ProbabilityGridRangeDataInserter2D::Insert for a batch (GrowAsNeeded, the hit and miss tables, FinishUpdate:
// probability_grid_range_data_inserter_2d.cc:20-114, MapBuilder::InsertIntoSubmap, map_builder.cc:110-120): ONE workgroup per
// scan does, in its own grid slot, what rgrid_grow_as_needed + rgrid_insert do with kg_grow, kg_ends, kg_hits, kg_rays and
// kg_finish.  A call names a slot at most once, so the workgroup owns its grid for the whole launch and the order the reference
// needs -- growth, hits, misses, finish -- is a workgroup barrier: no workgroup waits for another.  DESIGN.md 10.4.
#define KGI_THREADS 1024
#define KGI_WAVES (KGI_THREADS / 64)
#define KGI_GROW_PER 8                    // cells a thread holds in registers per step of the in-place move

// One runnable scan of an insert call; an array of these lies at the start of the call's segment.
struct InsertRec {
    InsertArgs A;                         // limits AFTER the growth the host decided, counts, origin
    long long cells_off;                  // its grid's first cell in the grid pool
    int old_nx, old_ny, off_x, off_y;     // the grid as it lies there now and where its cell (0, 0) goes; no growth: old_nx == A.nx
    int ret_off, mis_off;                 // float2 index of its returns in the float2 area, of its misses in the raw area
};
static_assert(sizeof(InsertRec) <= sizeof(BatchRec), "the insert records lie where a match's records lie");

struct InsertBufs {
    const unsigned char *seg;             // the call's segment: InsertRec[nrec] | ... | returns at f2_off | ... | misses at raw_off
    int f2_off, raw_off;
    unsigned short *cells;                // grid pool: read AND written, phase after phase -- no __restrict__, no const
    const unsigned short *hit, *miss;     // the handle's two lookup tables
    int *bad;                             // [max_scans], pinned host memory: 1 = an end point outside the grid, nothing inserted
    int free_space;
};

// the workgroup's cell stores have been acknowledged, then the barrier: the next phase's loads, from any wave, see them
__device__ static inline void cells_barrier()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__global__ __launch_bounds__(KGI_THREADS) void kgb_insert(InsertBufs B)
{
#pragma clang fp contract(off)
    __shared__ int s_pref[KGI_WAVES][65], s_lo[KGI_WAVES][64], s_step[KGI_WAVES][64];
    __shared__ int s_box[KGI_WAVES][4];
    const InsertRec &R = reinterpret_cast<const InsertRec *>(B.seg)[blockIdx.x];
    const InsertArgs A = R.A;
    unsigned short *cells = B.cells + R.cells_off;
    const float *ret = reinterpret_cast<const float *>(B.seg + B.f2_off) + 2 * (size_t)R.ret_off;
    const float *mis = reinterpret_cast<const float *>(B.seg + B.raw_off) + 2 * (size_t)R.mis_off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n_ret + A.n_miss;
    // ---- kg_ends' flag: is the origin or any end point outside the (grown) grid?  Along the way, the box of cells they span.
    int bx_i, by_i;
    bool out = !super_index(A, A.ox, A.oy, bx_i, by_i);                            // the origin (:54-55)
    int x0 = bx_i / SUBPX, x1 = x0, y0 = by_i / SUBPX, y1 = y0;
    for (int i = tid; i < n; i += KGI_THREADS) {
        const float *p = (i < A.n_ret) ? ret + 2 * i : mis + 2 * (i - A.n_ret);
        int ix, iy;
        out |= !super_index(A, p[0], p[1], ix, iy);
        const int cx = ix / SUBPX, cy = iy / SUBPX;
        x0 = min(x0, cx); x1 = max(x1, cx); y0 = min(y0, cy); y1 = max(y1, cy);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64)); x1 = max(x1, __shfl_xor(x1, off, 64));
        y0 = min(y0, __shfl_xor(y0, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
    }
    if (lane == 0) { s_box[wave][0] = x0; s_box[wave][1] = x1; s_box[wave][2] = y0; s_box[wave][3] = y1; }
    const bool bad = __syncthreads_or(out);
    for (int w = 0; w < KGI_WAVES; ++w) {
        x0 = min(x0, s_box[w][0]); x1 = max(x1, s_box[w][1]); y0 = min(y0, s_box[w][2]); y1 = max(y1, s_box[w][3]);
    }
    // the same in every lane: kept in scalar registers through the phases (the kernel runs at 128 VGPRs)
    x0 = __builtin_amdgcn_readfirstlane(x0); x1 = __builtin_amdgcn_readfirstlane(x1);
    y0 = __builtin_amdgcn_readfirstlane(y0); y1 = __builtin_amdgcn_readfirstlane(y1);
    bx_i = __builtin_amdgcn_readfirstlane(bx_i); by_i = __builtin_amdgcn_readfirstlane(by_i);
    // ---- kg_grow in place (Grid2D::GrowLimits, grid_2d.cc:81-91).  Old cell (x, y) goes to (y + off_y) * nnx + x + off_x, never
    // below its old index y * nx + x: walking the old cells in DESCENDING chunks -- all threads read, barrier, all write, barrier --
    // a write lands only on a cell that has been read already (its own chunk's or a higher one's) or on one beyond the old grid.
    if (R.old_nx != A.nx) {
        const int onx = R.old_nx, ony = R.old_ny, nnx = A.nx, nny = A.ny, off_x = R.off_x, off_y = R.off_y;
        const int total = onx * ony, chunk = KGI_THREADS * KGI_GROW_PER;
        for (int hi = total; hi > 0; hi -= chunk) {
            unsigned short v[KGI_GROW_PER];
#pragma unroll
            for (int u = 0; u < KGI_GROW_PER; ++u) {
                const int k = hi - chunk + u * KGI_THREADS + tid;
                v[u] = k >= 0 ? cells[k] : (unsigned short)0;
            }
            cells_barrier();                                                       // (the loads have arrived too: vmcnt counts both)
#pragma unroll
            for (int u = 0; u < KGI_GROW_PER; ++u) {
                const int k = hi - chunk + u * KGI_THREADS + tid;
                if (k >= 0) {
                    const int y = k / onx, x = k - y * onx;
                    cells[(y + off_y) * nnx + (x + off_x)] = v[u];
                }
            }
            cells_barrier();
        }
        for (int y = wave; y < nny; y += KGI_WAVES) {                              // unknown (0) outside the window
            const bool row_in = y >= off_y && y < off_y + ony;
            for (int x = lane; x < nnx; x += 64)
                if (!(row_in && x >= off_x && x < off_x + onx)) cells[y * nnx + x] = 0;
        }
        cells_barrier();
    }
    if (bad) {                                                                     // rgrid_insert's RGRID_ERR_CAPACITY: grown, nothing inserted
        if (tid == 0) B.bad[blockIdx.x] = 1;
        return;
    }
    // ---- kg_hits (:59-62)
    for (int i = tid; i < A.n_ret; i += KGI_THREADS) {
        int ix, iy;
        super_index(A, ret[2 * i], ret[2 * i + 1], ix, iy);
        apply_table(cells, A.nx, ix / SUBPX, iy / SUBPX, B.hit);
    }
    cells_barrier();
    // ---- kg_rays: one WAVE per ray, the waves stride over origin -> return and origin -> miss.  The walk is kg_rays' text
    // (rgrid.hip, where the closed form is derived), with the end point computed here and `continue` for its `return`.
    if (B.free_space) {
        for (int i = wave; i < n; i += KGI_WAVES) {
            const float *p = (i < A.n_ret) ? ret + 2 * i : mis + 2 * (i - A.n_ret);
            int ex_i, ey_i;
            super_index(A, p[0], p[1], ex_i, ey_i);
            ex_i = __builtin_amdgcn_readfirstlane(ex_i); ey_i = __builtin_amdgcn_readfirstlane(ey_i);   // the wave's ray: scalar from here on
            const long long S = SUBPX;
            long long bx = bx_i, by = by_i, ex = ex_i, ey = ey_i;
            if (bx > ex) { long long t = bx; bx = ex; ex = t; t = by; by = ey; ey = t; }   // ordered by x (:24-27)
            const int X0 = (int)(bx / S), X1 = (int)(ex / S);
            if (X0 == X1) {                                                           // one pixel column (:35-47)
                const int ya = (int)((by < ey ? by : ey) / S), yb = (int)((by < ey ? ey : by) / S);
                for (int y = ya + lane; y <= yb; y += 64) apply_table(cells, A.nx, X0, y, B.miss);
                continue;
            }
            const long long dx = ex - bx, dy = ey - by, den = 2 * S * dx;
            const long long A0 = (2 * (by % S) + 1) * dx + (by / S) * den;            // absolute ordinate of the begin point (:64)
            const long long first_pixel = 2 * S - 2 * (bx % S) - 1, last_pixel = 2 * (ex % S) + 1;
            const bool up = dy > 0;
            auto a_out = [&](int X) -> long long {                                    // ordinate at the right border of column X
                return A0 + dy * (first_pixel + 2 * S * (long long)(X - X0) + ((X == X1) ? last_pixel - 2 * S : 0));
            };
            auto fdiv = [&](long long a) -> long long { return a / den; };            // a >= 0 inside the grid
            auto cdiv = [&](long long a) -> long long { return (a + den - 1) / den; };
            for (int Xc = X0; Xc <= X1; Xc += 64) {
                const int X = Xc + lane;
                int lo = 0, cnt = 0, step = 1;
                if (X <= X1) {
                    const long long ao = a_out(X);
                    int r_in, r_out;
                    if (up) { r_in = (X == X0) ? (int)(by / S) : (int)fdiv(a_out(X - 1)); r_out = (int)cdiv(ao) - 1; cnt = r_out - r_in + 1; }
                    else { r_in = (X == X0) ? (int)(by / S) : (int)cdiv(a_out(X - 1)) - 1; r_out = (int)fdiv(ao); cnt = r_in - r_out + 1; step = -1; }
                    if (cnt < 1) cnt = 1;                                             // the column's entry pixel is always visited
                    lo = r_in;
                }
                int incl = cnt;                                                       // exclusive prefix sum of cnt over the wave
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
                s_pref[wave][lane + 1] = incl; s_lo[wave][lane] = lo; s_step[wave][lane] = step;
                if (lane == 0) s_pref[wave][0] = 0;
                __builtin_amdgcn_wave_barrier();
                const int total = s_pref[wave][64];
                for (int q = lane; q < total; q += 64) {
                    int a = 0, b = 63;                                                // column c with pref[c] <= q < pref[c+1]
                    while (a < b) { const int mid = (a + b + 1) >> 1; if (s_pref[wave][mid] <= q) a = mid; else b = mid - 1; }
                    const int row = s_lo[wave][a] + s_step[wave][a] * (q - s_pref[wave][a]);
                    apply_table(cells, A.nx, Xc + a, row, B.miss);
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    cells_barrier();
    // ---- kg_finish (Grid2D::FinishUpdate, grid_2d.cc:20-29) over the box the origin and the end points span: every ray lies
    // inside it, and the grid came in finished
    for (int y = y0 + wave; y <= y1; y += KGI_WAVES)
        for (int x = x0 + lane; x <= x1; x += 64) {
            unsigned short *c = cells + (size_t)A.nx * y + x;
            const unsigned short v = *c;
            if (v >= MARKER) *c = (unsigned short)(v - MARKER);
        }
    if (tid == 0) B.bad[blockIdx.x] = 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The filter stage of MapBuilder::AddRangeData for a batch (map_builder.cc:30-31,73): ONE workgroup per scan computes
// VoxelFilter(size).Filter(returns), VoxelFilter(size).Filter(misses) and AdaptiveVoxelFilter(options).Filter of the first,
// the whole search over voxel sizes included (voxel_filter.cc:15-76), and writes the three clouds -- the points rgrid_voxel_filter
// and rgrid_adaptive_voxel_filter return, input order and input bits.  DESIGN.md 10.5.
//
// First occurrence per voxel comes from an insert-only open-addressing hash table in LDS.  A slot holds a point index.  A point
// walks its probe sequence to the first slot that is empty -- it claims it by compare-and-swap -- or whose holder has its own
// voxel key -- it lowers the slot to its index (atomic min).  A claimed slot keeps its key for the rest of the pass (holders only
// change within one voxel, nothing is freed), so every point of a voxel stops at the same slot, and after the barrier that slot
// holds the voxel's smallest index: point i survives iff its slot holds i, whatever the hash and the order of the threads.
// The table has at least two slots per point, so a probe always meets an empty slot.
// A thread keeps its points (i = u * 1024 + tid, u < 8) and their slots in registers and a cloud's subset as a bit per point:
// the range gate and every candidate size of the search are masks over the returns, nothing is compacted between passes.
#define KGF_THREADS 1024
#define KGF_WAVES (KGF_THREADS / 64)
#define KGF_PER 8                         // points per thread
#define KGF_MAX_POINTS (KGF_THREADS * KGF_PER)   // 8192: 8 B of keys + 2 slots of 4 B per point = 128 KB of gfx950's 160 KB
#define KGF_EMPTY 0x7fffffff
#define KGF_SCRATCH 256                   // bytes in front of the keys: three counters, two rows of wave sums

// One runnable scan of a filter call; an array of these lies at the start of the filter's input staging.  Offsets count points.
struct FilterRec {
    int n_ret, n_mis;
    int ret_off, mis_off;                 // its returns and misses in the input points
    int out_off;                          // its three output clouds: fr at out_off (room n_ret), fm behind it (n_mis), av behind that (n_ret)
    int pad;
};

struct FilterBufs {
    const unsigned char *in;              // FilterRec[nrec] | float2 points at pts_off
    int pts_off;
    int key_cap;                          // points the launch's key area holds (the largest cloud, padded to 16)
    float2 *out;                          // pinned host memory
    int *counts;                          // [nrec][3]: |fr|, |fm|, |av|, pinned host memory
    double min_pts;
    float vsize, maxl, max_range;
};

// slots of a cloud's table: a power of two, at least two per point
__host__ __device__ static inline int kgf_table_size(int n)
{
    int s = 64;
    while (s < 2 * n) s <<= 1;
    return s;
}

__device__ static inline unsigned kgf_hash(int kx, int ky)
{
    unsigned h = (unsigned)kx * 0x9E3779B1u + (unsigned)ky * 0x85EBCA77u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 13;
    return h;
}

// Workgroup sum of the set bits of `mask`, read by every thread from LDS after the barrier.  Count k adds into counter k % 3;
// behind its barrier thread 0 zeroes the counter of count k - 1 (everybody has read it: they are all past this barrier), which
// count k + 2 adds into only behind the next count's barrier.
__device__ __forceinline__ int kgf_count(int *s_cnt, int &turn, unsigned mask)
{
    int c = __popc(mask);
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[turn], c);
    __syncthreads();
    const int m = *(volatile int *)&s_cnt[turn];
    if (threadIdx.x == 0) s_cnt[(turn + 2) % 3] = 0;
    turn = (turn + 1) % 3;
    return m;
}

// VoxelFilter(res).Filter of the points whose bit is set in `in` (all of them below n): -> the survivors' bits, m = their number
__device__ __forceinline__ unsigned kgf_pass(const float (&px)[KGF_PER], const float (&py)[KGF_PER], unsigned in, float res, int n, int2 *key,
                                             int *tab, int *s_cnt, int &turn, int &m)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int S = kgf_table_size(n), mask = S - 1;
    int4 *t4 = reinterpret_cast<int4 *>(tab);
    for (int q = tid; q < S / 4; q += KGF_THREADS) t4[q] = make_int4(KGF_EMPTY, KGF_EMPTY, KGF_EMPTY, KGF_EMPTY);
    int kx[KGF_PER], ky[KGF_PER], slot[KGF_PER];
#pragma unroll
    for (int u = 0; u < KGF_PER; ++u) {
        if (u * KGF_THREADS >= n) break;
        if (in >> u & 1u) {
            // GetCellIndex (voxel_filter.cc:105-110): RoundToInt(point / resolution), float division, lround
            kx[u] = (int)lroundf(px[u] / res); ky[u] = (int)lroundf(py[u] / res);
            key[u * KGF_THREADS + tid] = make_int2(kx[u], ky[u]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < KGF_PER; ++u) {
        if (u * KGF_THREADS >= n) break;
        if (in >> u & 1u) {
            const int i = u * KGF_THREADS + tid;
            int s = (int)(kgf_hash(kx[u], ky[u]) & (unsigned)mask);
            for (;;) {
                int cur = __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (cur == KGF_EMPTY) {
                    cur = atomicCAS(&tab[s], KGF_EMPTY, i);
                    if (cur == KGF_EMPTY) break;                                   // claimed: unordered_set::insert(...).second (:89-93)
                }
                const int2 k = key[cur];                                           // somebody holds it: its voxel ...
                if (k.x == kx[u] && k.y == ky[u]) {                                // ... is this point's: the smaller index stays
                    if (i < cur) atomicMin(&tab[s], i);
                    break;
                }
                s = (s + 1) & mask;
            }
            slot[u] = s;
        }
    }
    __syncthreads();
    unsigned keep = 0;
#pragma unroll
    for (int u = 0; u < KGF_PER; ++u) {
        if (u * KGF_THREADS >= n) break;
        if ((in >> u & 1u) && tab[slot[u]] == u * KGF_THREADS + tid) keep |= 1u << u;
    }
    m = kgf_count(s_cnt, turn, keep);                                              // its barrier: the table and the keys are free again
    return keep;
}

// order-preserving ballot-scan compaction (kg_compact) of the points whose bit is set in `keep`, a tile of 1024 points per step
__device__ __forceinline__ int kgf_emit(const float (&px)[KGF_PER], const float (&py)[KGF_PER], unsigned keep, int n, float2 *out, int *s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    __syncthreads();                                                               // the wave sums of an earlier call have been read
    int base = 0;
#pragma unroll
    for (int u = 0; u < KGF_PER; ++u) {
        if (u * KGF_THREADS >= n) break;
        const bool k = keep >> u & 1u;
        const unsigned long long bal = __ballot(k);
        int *row = s_w + (u & 1) * KGF_WAVES;                                      // two rows in turn: one barrier per tile
        if (lane == 0) row[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < KGF_WAVES; ++w) { const int c = row[w]; if (w < wave) off += c; tot += c; }
        if (k) out[off + __popcll(bal & lt)] = make_float2(px[u], py[u]);
        base += tot;
    }
    return base;
}

// ROT: the point goes through Rigid2f(0, Rotation2Df(yaw)) on its way into the registers, rgrid_add_range_data's gravity alignment
// (map_builder.cc:20-28) with the host's (cos, sin) -- the translation of 0 is added as the host adds it (it turns a -0 sum into +0)
template <bool ROT>
__device__ __forceinline__ unsigned kgf_load(const float2 *__restrict__ src, int n, float (&px)[KGF_PER], float (&py)[KGF_PER], float c, float s)
{
    unsigned in = 0;
#pragma unroll
    for (int u = 0; u < KGF_PER; ++u) {
        const int i = u * KGF_THREADS + (int)threadIdx.x;
        px[u] = 0.f; py[u] = 0.f;
        if (i < n) {
            const float2 p = src[i];
            if (ROT) rigid2f_point(c, s, 0.f, 0.f, p.x, p.y, px[u], py[u]);
            else { px[u] = p.x; py[u] = p.y; }
            in |= 1u << u;
        }
    }
    return in;
}

// ROT = false: rgrid_batch_filter_submit's kernel, the clouds as they come (`rot` is not read).  ROT = true: the first stage of
// rgrid_batch_add_range_data, raw tracking-frame clouds and one (cos, sin) per record in `rot`.
template <bool ROT>
__global__ __launch_bounds__(KGF_THREADS) void kgb_filter(FilterBufs B, const float2 *__restrict__ rot)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char kgf_lds[];
    int *s_cnt = reinterpret_cast<int *>(kgf_lds);                                 // [3]
    int *s_w = s_cnt + 4;                                                          // [2][KGF_WAVES]
    int2 *key = reinterpret_cast<int2 *>(kgf_lds + KGF_SCRATCH);
    int *tab = reinterpret_cast<int *>(kgf_lds + KGF_SCRATCH + sizeof(int2) * (size_t)B.key_cap);
    const FilterRec R = reinterpret_cast<const FilterRec *>(B.in)[blockIdx.x];
    const float2 *__restrict__ pin = reinterpret_cast<const float2 *>(B.in + B.pts_off);
    float2 *out = B.out + R.out_off;
    if (threadIdx.x == 0) { s_cnt[0] = 0; s_cnt[1] = 0; s_cnt[2] = 0; }            // (the first pass's first barrier publishes them)
    int turn = 0;
    float px[KGF_PER], py[KGF_PER];
    float rc = 1.f, rs = 0.f;
    if (ROT) { const float2 cs = rot[blockIdx.x]; rc = cs.x; rs = cs.y; }
    // ---- VoxelFilter(voxel_filter_size).Filter(returns) (map_builder.cc:30)
    const int nr = R.n_ret;
    unsigned in = kgf_load<ROT>(pin + R.ret_off, nr, px, py, rc, rs);
    int m;
    const unsigned fr = kgf_pass(px, py, in, B.vsize, nr, key, tab, s_cnt, turn, m);
    const int n_fr = kgf_emit(px, py, fr, nr, out, s_w);
    // ---- AdaptiveVoxelFilter(options).Filter(fr) (map_builder.cc:73): FilterByMaxRange (voxel_filter.cc:15-27) ...
    unsigned gate = 0;
#pragma unroll
    for (int u = 0; u < KGF_PER; ++u)
        if ((fr >> u & 1u) && sqrtf(px[u] * px[u] + py[u] * py[u]) <= B.max_range) gate |= 1u << u;
    const int ni = kgf_count(s_cnt, turn, gate);
    // ... and AdaptivelyVoxelFiltered (:29-76), one candidate size after the other; every decision from a count read from LDS
    unsigned av = gate;
    const double min_pts = B.min_pts;
    if (!((double)ni <= min_pts)) {                                                // :33-37 already sparse enough
        const float maxl = B.maxl;
        av = kgf_pass(px, py, gate, maxl, nr, key, tab, s_cnt, turn, m);            // :38
        if (!((double)m >= min_pts)) {                                             // :39-43
            for (float high = maxl; high > 1e-2f * maxl; high /= 2.f) {            // :47-48
                float low = high / 2.f;
                av = kgf_pass(px, py, gate, low, nr, key, tab, s_cnt, turn, m);
                if ((double)m >= min_pts) {
                    while ((high - low) / low > 1e-1f) {                           // :57 bisection to 10 %
                        const float mid = (low + high) / 2.f;
                        const unsigned cand = kgf_pass(px, py, gate, mid, nr, key, tab, s_cnt, turn, m);
                        if ((double)m >= min_pts) { low = mid; av = cand; } else high = mid;
                    }
                    break;
                }
            }                                                                      // nothing dense enough: the last size tried (:75)
        }
    }
    const int n_av = kgf_emit(px, py, av, nr, out + nr + R.n_mis, s_w);
    // ---- VoxelFilter(voxel_filter_size).Filter(misses) (map_builder.cc:31): a fresh filter, a fresh table
    const int nm = R.n_mis;
    in = kgf_load<ROT>(pin + R.mis_off, nm, px, py, rc, rs);
    const unsigned fm = kgf_pass(px, py, in, B.vsize, nm, key, tab, s_cnt, turn, m);
    const int n_fm = kgf_emit(px, py, fm, nm, out + nr, s_w);
    if (threadIdx.x == 0) { int *c = B.counts + 3 * blockIdx.x; c[0] = n_fr; c[1] = n_fm; c[2] = n_av; }
}

// ---------------------------------------------------------------------------------------------------------------
// MatchingResult::range_data_in_local.returns for a batch (map_builder.cc:89-90): every inserted scan's RAW returns, still lying
// where the filter read them, through Rigid2f(pose_estimate.cast<float>()) -- rigid2f_apply's line with the host's (cos, sin) and
// translation -- compactly into pinned host memory.  One float2 per lane, consecutive lanes consecutive points.  A workgroup is a
// tile of KGL_THREADS points of one scan, named by a table as kgb_match's workgroups are: a scan of n points costs
// ceil(n / KGL_THREADS) workgroups whatever its neighbours' sizes.  DESIGN.md 10.10.
#define KGL_THREADS 256

struct ToLocalRec {
    int src_off;                          // its raw returns in the filter's input points
    int dst_off;                          // its rows in the output
    int n, pad;
    float c, s, tx, ty;
};

struct ToLocalBufs {
    const unsigned char *tab;             // ToLocalRec[nrec] | int2 (record, tile) per workgroup at wgmap_off
    int wgmap_off;
    const float2 *src;                    // the filter's input points
    float2 *out;                          // pinned host memory
};

__global__ __launch_bounds__(KGL_THREADS) void kgb_to_local(ToLocalBufs B)
{
    const int2 wg = reinterpret_cast<const int2 *>(B.tab + B.wgmap_off)[blockIdx.x];
    const ToLocalRec R = reinterpret_cast<const ToLocalRec *>(B.tab)[wg.x];
    const int i = wg.y * KGL_THREADS + (int)threadIdx.x;
    if (i >= R.n) return;
    const float2 p = B.src[R.src_off + i];
    float2 o;
    rigid2f_point(R.c, R.s, R.tx, R.ty, p.x, p.y, o.x, o.y);
    B.out[R.dst_off + i] = o;
}

// ---------------------------------------------------------------------------------------------------------------
// MapBuilder::ToSubmapTexture for a batch (Submap2D::GetMapTextureData -> ProbabilityGrid::DrawToSubmapTexture,
// probability_grid.cc:86-131, with Grid2D::ComputeCroppedLimits, grid_2d.cc:36-48): ONE workgroup per named slot does what
// rgrid_draw_texture does with kg_known_box, a round trip to the host and kg_texture.  Phase 1 reduces the slot's nx * ny cells to
// the box of its known cells (raw value not 0) inside the workgroup -- per-thread min / max, wave shuffles, LDS across the waves:
// no atomics, nothing to clear before the launch.  Phase 2, behind the barrier, writes the (value, alpha) pairs of the box
// compactly (stride = width) to the start of the slot's region of the output area.  The launch only reads the pool, so a slot may
// be named more than once and no workgroup waits for another.  DESIGN.md 10.7.
//
// Both phases move 16 bytes per lane where they can.  A slot starts grid * max_cells cells into the pool, which is 2-byte aligned
// and no more when max_cells is odd: phase 1 walks the slot as ONE array of nx * ny cells -- the cells in front of the first
// 16-byte boundary and behind the last one singly, the eight-cell vectors between them whole -- and never touches the stale
// max_cells - nx * ny cells behind it.  Phase 2 gathers single cells (a row of the box starts anywhere) and stores eight pairs at
// once: the region's start is 16-byte aligned by the host's prefix sum, the last w * h mod 8 pairs go singly.
// One named slot of a texture call; an array of these lies at the start of the call's segment.
struct TextureRec {
    long long cells_off;                  // its grid's first cell in the grid pool
    long long out_off;                    // its region's first pair in the output area (a multiple of 8)
    int nx, ny;
};
static_assert(sizeof(TextureRec) <= sizeof(BatchRec), "the texture records lie where a match's records lie");

struct TextureBufs {
    const unsigned char *seg;             // the call's segment: TextureRec[nrec]
    const unsigned short *cells;          // grid pool
    const unsigned short *table;          // texture_table: value | alpha << 8 per cell value
    unsigned short *out;                  // pinned host memory: a region of nx * ny pairs (rounded up to 8) per record
    int *box;                             // [nrec][4]: offset_x, offset_y, width, height, pinned host memory
};

__global__ __launch_bounds__(KGT_THREADS) void kgb_texture(TextureBufs B)
{
    __shared__ int s_box[KGT_WAVES][4];
    const TextureRec R = reinterpret_cast<const TextureRec *>(B.seg)[blockIdx.x];
    const unsigned short *__restrict__ cells = B.cells + R.cells_off;
    const int nx = R.nx, tid = threadIdx.x;
    // ---- phase 1: the box of the known cells (known_box_of_slot, rgrid_dev.h)
    int x0, y0, w, h;
    known_box_of_slot(cells, nx, R.nx * R.ny, s_box, x0, y0, w, h);
    if (tid == 0) { int *box = B.box + 4 * blockIdx.x; box[0] = x0; box[1] = y0; box[2] = w; box[3] = h; }
    // ---- phase 2: pair o of the texture is cell (x0 + o % w, y0 + o / w); eight pairs per store
    const unsigned short *__restrict__ table = B.table;
    const unsigned short *__restrict__ win = cells + (size_t)nx * y0 + x0;         // the box's first cell: all of it lies inside the slot
    unsigned short *out = B.out + R.out_off;
    const int total = w * h, nout = total >> 3;
    for (int v = tid; v < nout; v += KGT_THREADS) {
        const int o = 8 * v;
        int yy = o / w, xx = o - yy * w;
        unsigned p[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            p[c] = win[nx * yy + xx];
            if (++xx == w) { xx = 0; ++yy; }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) p[c] = table[p[c] & 32767u];
        reinterpret_cast<uint4 *>(out)[v] = make_uint4(p[0] | p[1] << 16, p[2] | p[3] << 16, p[4] | p[5] << 16, p[6] | p[7] << 16);
    }
    for (int o = 8 * nout + tid; o < total; o += KGT_THREADS) {
        const int yy = o / w, xx = o - yy * w;
        out[o] = table[win[nx * yy + xx] & 32767u];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Node::PublishMap / Node::HandleSaveMap for a batch (src/ros_node.cc:845-863,947-1001): the painting of every named slot's
// texture, ONE workgroup per named slot.  Phase 1 is kgb_texture's (known_box_of_slot); phase 2 writes the interior block of the
// image -- the box turned by 90 degrees, every cell through the byte table of the call's mode -- to the slot's region of the output
// area (occupancy_tiles, rgrid_dev.h).  The frame around the block, the row order of the message and the image's size and origin
// are the host's, in the copy collect makes anyway.  The launch only reads the pool: no atomics, no workgroup waits for another, a
// slot may be named more than once.  DESIGN.md 10.8.
struct OccupancyRec {
    long long cells_off;                  // its grid's first cell in the grid pool
    long long out_off;                    // its region's first byte in the output area (a multiple of 16)
    int nx, ny;
};
static_assert(sizeof(OccupancyRec) <= sizeof(BatchRec), "the occupancy records lie where a match's records lie");

struct OccupancyBufs {
    const unsigned char *seg;             // the call's segment: OccupancyRec[nrec]
    const unsigned short *cells;          // grid pool
    const unsigned char *table;           // the byte table of the call's mode, 32768 entries
    unsigned char *out;                   // pinned host memory: a region of nx * occupancy_stride(ny) bytes per record
    int *box;                             // [nrec][4]: offset_x, offset_y, width, height, pinned host memory
};

__global__ __launch_bounds__(KGT_THREADS) void kgb_occupancy(OccupancyBufs B)
{
    __shared__ int s_box[KGT_WAVES][4];
    __shared__ __align__(16) unsigned char s_tile[OCC_T][OCC_PITCH];
    const OccupancyRec R = reinterpret_cast<const OccupancyRec *>(B.seg)[blockIdx.x];
    const unsigned short *__restrict__ cells = B.cells + R.cells_off;
    int x0, y0, w, h;
    known_box_of_slot(cells, R.nx, R.nx * R.ny, s_box, x0, y0, w, h);
    if (threadIdx.x == 0) { int *box = B.box + 4 * blockIdx.x; box[0] = x0; box[1] = y0; box[2] = w; box[3] = h; }
    occupancy_tiles(cells, R.nx, x0, y0, w, h, B.table, B.out + R.out_off, s_tile, 0, 1);
}

struct GridSlot {
    bool set = false;
    int nx = 0, ny = 0;
    double resolution = 0., max_x = 0., max_y = 0.;
};

// what collect needs of a submitted scan
struct Pending {
    int status, rec;
    MatchPlan plan;
    double pose[3];
};

// what a packed match launches with
struct MatchWork { int nrec, nwg, nf2, n_max; };

enum { KIND_MATCH = 1, KIND_REFINE = 2, KIND_SCAN_MATCH = 3, KIND_INSERT = 4, KIND_FILTER = 5, KIND_TEXTURE = 6, KIND_OCCUPANCY = 7 };  // the pending submit

// what collect needs of a scan of a filter submit
struct FilterPending { int status, rec, out_off, n_ret, n_mis; };

// what rgrid_batch_add_range_data hands from stage to stage for one scan
struct RangeScan {
    int code, status;
    int frec;                             // its filter record, -1 without one
    int src_off, out_off;                 // its raw returns in the filter's input points, its three clouds in the filter's output
    int n_fr, n_fm, n_av;
    int mrec;                             // its place among the scans that are matched, -1 without a grid
    int dst_off;                          // its rows in kgb_to_local's output
    bool packed;                          // the insert has a record for it: b->sub[j] is its Pending
    double est[3];                        // MapBuilder::ScanMatch's answer: the refinement's, or the prediction without a grid
};

// what collect needs of a named slot of a texture submit
struct TexturePending { int grid; long long out_off; };

// what collect needs of a named slot of an occupancy submit
struct OccupancyPending { int grid; long long out_off; double submap_origin[2]; };

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

struct rgrid_batch {
    int max_scans = 0, max_points = 0, num_grids = 0, max_rotations = 0, device = 0;
    long max_cells = 0;
    int mode = RGRID_BATCH_REDUCE_ARRIVAL;
    hipStream_t stream = nullptr;
    // the staging segments the kernels read in place, used in turn, and a segment's image in ordinary memory (rotated points are
    // read back while packing)
    struct {
        batch_host::Staging<unsigned char> buf[KGB_SEGMENTS];
        size_t wgmap_off = 0, f2_off = 0, rrec_off = 0, raw_off = 0;
        std::vector<unsigned char> pack;
        unsigned long long n_taken = 0;
    } seg;
    batch_host::Device<unsigned short> cells;   // grid pool
    std::vector<GridSlot> grids;
    // the matcher and the refinement: a result slot per scan
    struct {
        batch_host::Device<unsigned long long> bb;   // [max_scans][max_rotations] block bests
        batch_host::Device<int> arrived;             // [max_scans] arrival counters
        batch_host::Pinned<BestRec> best;
        batch_host::Pinned<RefineOut> fine;
    } res;
    // the inserter: the two lookup tables (uint16[32768] each) and the probabilities they were built for, a flag per record
    struct {
        batch_host::Device<unsigned short> hit, miss;
        float tab_hit_p = -1.f, tab_miss_p = -1.f;
        batch_host::Pinned<int> bad;
        std::vector<unsigned long long> slot_call;   // the insert submit that named a slot last (a call names a slot once)
        unsigned long long n_calls = 0;
    } ins;
    // the filter: its own staging, allocated by the first filter submit (filter_staging) -- records and input points the kernel
    // reads in place, output points and counts
    struct {
        batch_host::Staging<unsigned char> in;
        size_t pts_off = 0;
        batch_host::Pinned<float2> out;
        batch_host::Pinned<int> cnt;         // allocated last: it marks the staging as complete
        std::vector<FilterPending> sub;
        size_t rot_off = 0;                  // a (cos, sin) per record behind the input points: what kgb_filter<true> rotates by
    } fil;
    // AddRangeData (range_data_staging, allocated by the first rgrid_batch_add_range_data): kgb_to_local's records and workgroup
    // table, its output rows; per scan what the stages hand on; the moved clouds of one scan on their way into the insert's segment
    struct {
        batch_host::Staging<unsigned char> tab;
        size_t wgmap_off = 0;
        batch_host::Pinned<float2> out;      // allocated last: it marks the staging as complete
        std::vector<RangeScan> scan;
        std::vector<rgrid_batch_scan> match;
        std::vector<float> ret, mis;
        int last_counts[2] = {0, 0};         // launches, synchronisations of the last call
    } ard;
    unsigned long long n_launches = 0, n_syncs = 0;   // kernels launched (launch_*) and streams waited for (collect_head) so far
    // the texture (texture_staging): the (value, alpha) table (uint16[32768]) on the device, uploaded by the first texture submit;
    // the output area and the box records, allocated by the first texture submit, the area grown only when a call needs more
    struct {
        batch_host::Device<unsigned short> table;
        batch_host::Pinned<unsigned short> out;
        size_t out_pairs = 0;
        batch_host::Pinned<int> box;
        std::vector<TexturePending> sub;
    } tex;
    // the occupancy grid (occupancy_staging): the two byte tables (occupancy, then red: 2 * 32768 bytes) on the device, uploaded by
    // the first occupancy submit; the output area and the box records, allocated by it too, the area grown only when a call needs more
    struct {
        batch_host::Device<unsigned char> tables;
        batch_host::Pinned<unsigned char> out;
        size_t out_bytes = 0;
        batch_host::Pinned<int> box;
        std::vector<OccupancyPending> sub;
        std::vector<OccupancyFrame> frame;   // filled by collect
        int mode = 0;                        // of the pending submit
    } occ;
    // the submit that has not been collected
    bool outstanding = false;
    int kind = 0;                          // its KIND_*
    int sub_count = 0;
    std::vector<Pending> sub;
    double prepare_seconds = 0.;
    std::string hip_error;
};

namespace {

bool slot_ok(const rgrid_batch_t *b, int grid) { return grid >= 0 && grid < b->num_grids && b->grids[(size_t)grid].set; }

// a slot's first cell in the grid pool
long long cells_offset(const rgrid_batch_t *b, int grid) { return (long long)grid * (long long)b->max_cells; }

// one cloud of a scan of a match or a refine submit, into a set slot
bool cloud_ok(const rgrid_batch_t *b, int grid, const float *points_xy, int n) { return slot_ok(b, grid) && n >= 0 && (n == 0 || points_xy); }

// The segments are used in turn, and the turn passes once per launch that reads one.  next_segment is the one that launch will read
// (a submit may write points straight into it before it knows whether it has anything to launch); take_segment is next_segment for
// a submit that does launch.
int next_segment(const rgrid_batch_t *b) { return (int)(b->seg.n_taken % KGB_SEGMENTS); }
int take_segment(rgrid_batch_t *b) { return (int)(b->seg.n_taken++ % KGB_SEGMENTS); }

double seconds_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

// The end of every submit, after the caller has packed `count` scans into `nrec` records and staged them.  A submit without a
// record launches nothing and is pending all the same: its collect gives the per-scan statuses.  A launch that fails leaves
// nothing pending.
template <typename Launch>
int submit_tail(rgrid_batch_t *b, int kind, int count, int nrec, std::chrono::steady_clock::time_point t_begin, Launch launch)
{
    b->sub_count = count;
    if (nrec > 0) __atomic_thread_fence(__ATOMIC_SEQ_CST);      // write-combined stores drained before the doorbell
    b->prepare_seconds = seconds_since(t_begin);
    if (nrec > 0) {
        launch();
        G_TRY(b, hipGetLastError());
    }
    b->outstanding = true; b->kind = kind;
    return RGRID_OK;
}

// The start of every collect: the pending submit is of `kind` and, unless it had no scans, the caller has its required outputs;
// gives its scan count and waits for the launch.  With clear_first nothing is pending from here on, a HIP error in the wait
// included; without, the caller clears `outstanding` itself once it knows the results fit (RGRID_ERR_BUFFER leaves the submit
// pending, and the next collect waits again).
int collect_head(rgrid_batch_t *b, int kind, bool outputs, bool clear_first, int *count)
{
    if (!b || !b->outstanding || b->kind != kind) return RGRID_ERR_INVALID;
    *count = b->sub_count;
    if (*count > 0 && !outputs) return RGRID_ERR_INVALID;
    if (clear_first) b->outstanding = false;
    G_TRY(b, hipSetDevice(b->device));
    ++b->n_syncs;
    G_TRY(b, hipStreamSynchronize(b->stream));
    return RGRID_OK;
}

// scan j's entry for collect, zeroed and without a record
Pending &fresh_pending(rgrid_batch_t *b, int j)
{
    Pending &P = b->sub[(size_t)j];
    std::memset(&P, 0, sizeof(P));
    P.rec = -1;
    return P;
}

// the whole-call conditions on the scans of a match (or match-plus-refine) submit
bool match_scans_ok(const rgrid_batch_t *b, const rgrid_batch_scan *scans, int count)
{
    for (int j = 0; j < count; ++j)
        if (!cloud_ok(b, scans[j].grid, scans[j].points_xy, scans[j].n)) return false;
    return true;
}

// Plans every scan of a match into b->sub and the segment's image: records, workgroup map, rotated points, rotation tables
MatchWork pack_match(rgrid_batch_t *b, const rgrid_match_options *opt, const rgrid_batch_scan *scans, int count)
{
#pragma clang fp contract(off)
    const int rot_cap = b->max_rotations < KGB_MAX_ROT ? b->max_rotations : KGB_MAX_ROT;
    BatchRec *recs = reinterpret_cast<BatchRec *>(b->seg.pack.data());
    int2 *wgmap = reinterpret_cast<int2 *>(b->seg.pack.data() + b->seg.wgmap_off);
    float *f2 = reinterpret_cast<float *>(b->seg.pack.data() + b->seg.f2_off);
    int nrec = 0, nwg = 0, nf2 = 0, n_max = 0;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_scan &s = scans[j];
        const GridSlot &g = b->grids[(size_t)s.grid];
        Pending &P = fresh_pending(b, j);
        if (s.n == 0) { P.status = RGRID_ERR_EMPTY; continue; }
        if (s.n > b->max_points || b->max_rotations > KGB_MAX_ROT) { P.status = RGRID_ERR_CAPACITY; continue; }
        const int n = s.n;
        // the search plan rgrid_match makes; on top of it this handle's own limits: its rotations, a linear window of 16383 cells
        float *pts = f2 + 2 * (size_t)nf2;
        MatchPlan &M = P.plan;
        if (plan_match(opt, g.resolution, s.initial_pose, s.points_xy, n, pts, &M) != RGRID_OK || M.num_scans > rot_cap || M.num_linear > 16383) {
            P.status = RGRID_ERR_CAPACITY;
            continue;
        }
        const int num_scans = M.num_scans;
        const int pts_off = nf2;
        nf2 += n;
        rotation_table(M, f2 + 2 * (size_t)nf2);
        const int cs_off = nf2;
        nf2 += num_scans;
        BatchRec &A = recs[nrec];
        A.resolution = M.res; A.max_x = g.max_x; A.max_y = g.max_y;
        A.num_angular_d = (double)M.num_angular; A.step = M.step;
        A.wt = opt->translation_delta_cost_weight; A.wr = opt->rotation_delta_cost_weight;
        A.cells_off = cells_offset(b, s.grid);
        A.n = n; A.num_scans = num_scans; A.num_linear = M.num_linear; A.nx = g.nx; A.ny = g.ny;
        A.pts_off = pts_off; A.cs_off = cs_off;
        A.tx = (float)s.initial_pose[0]; A.ty = (float)s.initial_pose[1];
        for (int r = 0; r < num_scans; ++r) wgmap[nwg + r] = make_int2(nrec, r);
        nwg += num_scans;
        if (n > n_max) n_max = n;
        P.status = RGRID_OK; P.rec = nrec;
        std::memcpy(P.pose, s.initial_pose, sizeof(double) * 3);
        ++nrec;
    }
    return MatchWork{nrec, nwg, nf2, n_max};
}

// the match's image into segment k: three forward copies, nothing is read back from it
void stage_match(rgrid_batch_t *b, int k, const MatchWork &W)
{
    unsigned char *to = b->seg.buf[k].h;
    const unsigned char *from = b->seg.pack.data();
    std::memcpy(to, from, sizeof(BatchRec) * (size_t)W.nrec);
    std::memcpy(to + b->seg.wgmap_off, from + b->seg.wgmap_off, sizeof(int2) * (size_t)W.nwg);
    std::memcpy(to + b->seg.f2_off, from + b->seg.f2_off, sizeof(float2) * (size_t)W.nf2);
}

void launch_match(rgrid_batch_t *b, int k, const MatchWork &W)
{
    BatchBufs Bf;
    Bf.seg = b->seg.buf[k].dv; Bf.wgmap_off = (int)b->seg.wgmap_off; Bf.f2_off = (int)b->seg.f2_off;
    Bf.cells = b->cells.d; Bf.bb = b->res.bb.d; Bf.arrived = b->res.arrived.d; Bf.out = b->res.best.dv;
    Bf.max_rotations = b->max_rotations < KGB_MAX_ROT ? b->max_rotations : KGB_MAX_ROT;
    const size_t lds = sizeof(int2) * (size_t)((W.n_max + KGB_PF - 1) / KGB_PF * KGB_PF);
    b->n_launches += b->mode == RGRID_BATCH_REDUCE_ARRIVAL ? 1 : 2;
    if (b->mode == RGRID_BATCH_REDUCE_ARRIVAL) {
        hipLaunchKernelGGL(kgb_match<true>, dim3((unsigned)W.nwg), dim3(KGB_THREADS), lds, b->stream, Bf);
    } else {
        hipLaunchKernelGGL(kgb_match<false>, dim3((unsigned)W.nwg), dim3(KGB_THREADS), lds, b->stream, Bf);
        hipLaunchKernelGGL(kgb_best, dim3((unsigned)W.nrec), dim3(KGB_THREADS), 0, b->stream, Bf);
    }
}

// Refine record `rec` of a call that launches from segment k: everything but the start pose (or the plan it is decoded with) and
// match_rec, which the caller fills in.  The record goes into the segment's image, the raw points forward, straight into the segment
// at point `nraw`; `threads` becomes the largest scan's thread count.
RefineRec &pack_refine(rgrid_batch_t *b, int k, int rec, const rgrid_refine_options *opt, int grid, const float *points_xy, int n, int &nraw, int &threads)
{
    RefineRec &R = reinterpret_cast<RefineRec *>(b->seg.pack.data() + b->seg.rrec_off)[rec];
    std::memset(&R, 0, sizeof(R));
    const GridSlot &g = b->grids[(size_t)grid];
    refine_args(R.A, g.nx, g.ny, g.resolution, g.max_x, g.max_y, opt, n);
    R.cells_off = cells_offset(b, grid);
    R.pts_off = nraw;
    std::memcpy(reinterpret_cast<float *>(b->seg.buf[k].h + b->seg.raw_off) + 2 * (size_t)nraw, points_xy, sizeof(float) * 2 * (size_t)n);
    nraw += n;
    if (refine_threads(n) > threads) threads = refine_threads(n);
    return R;
}

// one workgroup per refine record of segment k, `threads` = the largest scan's thread count
void launch_refine(rgrid_batch_t *b, int k, int nrec, int threads)
{
    RefineBufs Rf;
    Rf.seg = b->seg.buf[k].dv; Rf.rrec_off = (int)b->seg.rrec_off; Rf.raw_off = (int)b->seg.raw_off;
    Rf.cells = b->cells.d; Rf.best = b->res.best.dv; Rf.out = b->res.fine.dv;
    ++b->n_launches;
    hipLaunchKernelGGL(kgb_refine, dim3((unsigned)nrec), dim3((unsigned)threads), 0, b->stream, Rf);
}

void zero3(double *p) { p[0] = p[1] = p[2] = 0.; }
void zero3(int *p) { if (p) p[0] = p[1] = p[2] = 0; }

// scan j's match outputs from its result record (all zero when it had none); best3 and info3 may be absent
void match_result(const rgrid_batch_t *b, int j, double *poses, double *scores, int *best3, int *info3)
{
    const Pending &P = b->sub[(size_t)j];
    int *best = best3 ? &best3[3 * j] : nullptr, *info = info3 ? &info3[3 * j] : nullptr;
    zero3(&poses[3 * j]);
    scores[j] = 0.;
    zero3(best);
    zero3(info);
    if (P.status == RGRID_OK) decode_best(P.plan, P.pose, b->res.best.h[P.rec], &poses[3 * j], &scores[j], best, info);
}

// a scan's refine outputs from its result record (all zero when it had none)
void refine_result(const rgrid_batch_t *b, const Pending &P, double *pose, rgrid_refine_summary *summary)
{
    zero3(pose);
    if (summary) std::memset(summary, 0, sizeof(*summary));
    if (P.status != RGRID_OK) return;
    const RefineOut &o = b->res.fine.h[P.rec];
    pose[0] = o.pose[0]; pose[1] = o.pose[1]; pose[2] = o.pose[2];
    if (summary) { summary->initial_cost = o.initial_cost; summary->final_cost = o.final_cost; summary->iterations = o.iterations; summary->termination = o.termination; }
}

// how far an insert's packing has come: records, returns and misses in segment k
struct InsertWork { int k, nrec, nret, nmis; };

// Plans scan j of an insert into b->sub[j], its slot's limits and the segment's image; the points go forward, straight into
// segment W.k (they are read here for the last time: the caller may reuse their memory for the next scan).
void pack_insert_scan(rgrid_batch_t *b, InsertWork &W, const rgrid_batch_insert_scan &s, int j)
{
    InsertRec *recs = reinterpret_cast<InsertRec *>(b->seg.pack.data());
    float *ret = reinterpret_cast<float *>(b->seg.buf[W.k].h + b->seg.f2_off), *mis = reinterpret_cast<float *>(b->seg.buf[W.k].h + b->seg.raw_off);
    int &nrec = W.nrec, &nret = W.nret, &nmis = W.nmis;
    GridSlot &g = b->grids[(size_t)s.grid];
    Pending &P = fresh_pending(b, j);
    // rgrid_grow_as_needed: on the host, from the points that are copied anyway; the move itself is the workgroup's first phase
    int nx = g.nx, ny = g.ny, off_x = 0, off_y = 0;
    double max_x = g.max_x, max_y = g.max_y;
    P.status = plan_growth(s.origin_xy, s.returns_xy, s.n_returns, s.misses_xy, s.n_misses, g.resolution, (long long)b->max_cells, nx, ny,
                           max_x, max_y, off_x, off_y);
    if (P.status != RGRID_OK) return;                                          // the slot stays as it is
    // rgrid_insert: more points than the handle stages.  The pair has grown the grid by then, so this scan's workgroup grows it too
    const bool fits = s.n_returns <= b->max_points && s.n_misses <= b->max_points;
    if (!fits) P.status = RGRID_ERR_CAPACITY;
    if (!fits && nx == g.nx && ny == g.ny) return;
    InsertRec &R = recs[nrec];
    std::memset(&R, 0, sizeof(R));
    R.A.nx = nx; R.A.ny = ny; R.A.n_ret = fits ? s.n_returns : 0; R.A.n_miss = fits ? s.n_misses : 0;
    R.A.max_x = max_x; R.A.max_y = max_y; R.A.rs = g.resolution / SUBPX;
    R.A.ox = s.origin_xy[0]; R.A.oy = s.origin_xy[1];
    R.cells_off = cells_offset(b, s.grid);
    R.old_nx = g.nx; R.old_ny = g.ny; R.off_x = off_x; R.off_y = off_y;
    R.ret_off = nret; R.mis_off = nmis;
    if (R.A.n_ret > 0) std::memcpy(ret + 2 * (size_t)nret, s.returns_xy, sizeof(float) * 2 * (size_t)R.A.n_ret);   // forward, straight into the segment
    if (R.A.n_miss > 0) std::memcpy(mis + 2 * (size_t)nmis, s.misses_xy, sizeof(float) * 2 * (size_t)R.A.n_miss);
    nret += R.A.n_ret; nmis += R.A.n_miss;
    g.nx = nx; g.ny = ny; g.max_x = max_x; g.max_y = max_y;                    // what later submits' records are filled from
    P.rec = nrec;
    ++nrec;
}

// The lookup tables of an insert (they only depend on the two probabilities) and its next segment
int begin_insert(rgrid_batch_t *b, const rgrid_insert_options *opt, InsertWork &W)
{
    G_TRY(b, hipSetDevice(b->device));
    G_TRY(b, insert_tables(opt->hit_probability, opt->miss_probability, b->ins.hit.d, b->ins.miss.d, b->ins.tab_hit_p, b->ins.tab_miss_p));
    W = InsertWork{next_segment(b), 0, 0, 0};
    return RGRID_OK;
}

// the packed records into their segment, which is taken when there are any
void stage_insert(rgrid_batch_t *b, const InsertWork &W)
{
    if (W.nrec == 0) return;
    take_segment(b);
    std::memcpy(b->seg.buf[W.k].h, b->seg.pack.data(), sizeof(InsertRec) * (size_t)W.nrec);
}

void launch_insert(rgrid_batch_t *b, const rgrid_insert_options *opt, const InsertWork &W)
{
    InsertBufs If;
    If.seg = b->seg.buf[W.k].dv; If.f2_off = (int)b->seg.f2_off; If.raw_off = (int)b->seg.raw_off;
    If.cells = b->cells.d; If.hit = b->ins.hit.d; If.miss = b->ins.miss.d; If.bad = b->ins.bad.dv; If.free_space = opt->insert_free_space ? 1 : 0;
    ++b->n_launches;
    hipLaunchKernelGGL(kgb_insert, dim3((unsigned)W.nrec), dim3(KGI_THREADS), 0, b->stream, If);
}

// A slot at most once per call: two insertions into one grid in one launch have no reference meaning (FinishUpdate lies between).
// The call is counted, and its slots marked, before anything else can refuse it.
template <typename Scan>
bool slots_named_once(rgrid_batch_t *b, const Scan *scans, int count)
{
    ++b->ins.n_calls;
    for (int j = 0; j < count; ++j) {
        unsigned long long &seen = b->ins.slot_call[(size_t)scans[j].grid];
        if (seen == b->ins.n_calls) return false;
        seen = b->ins.n_calls;
    }
    return true;
}

// scan j's status of an insert whose launch has been waited for
int insert_status(const rgrid_batch_t *b, int j)
{
    const Pending &P = b->sub[(size_t)j];
    return (P.status == RGRID_OK && b->ins.bad.h[P.rec]) ? RGRID_ERR_CAPACITY : P.status;   // an end point outside the grid after growth
}

// points per cloud of a filter submit: what the handle stages and what one workgroup of kgb_filter holds
int filter_point_cap(const rgrid_batch_t *b) { return b->max_points < KGF_MAX_POINTS ? b->max_points : KGF_MAX_POINTS; }

// the lround of a non-finite coordinate is undefined in the reference: such a scan is refused
bool all_finite(const float *v, size_t n)
{
    unsigned bad = 0;
    for (size_t i = 0; i < n; ++i) {
        unsigned u;
        std::memcpy(&u, v + i, sizeof(u));
        bad |= (unsigned)((u & 0x7f800000u) == 0x7f800000u);
    }
    return !bad;
}

// The filter's staging: records and input points for max_scans scans of two clouds, three output clouds per scan, three counts.
// A call that fails part-way keeps what it allocated, and the next one goes on from there.
int filter_staging(rgrid_batch_t *b)
{
    const size_t nS = (size_t)b->max_scans, nP = (size_t)filter_point_cap(b);
    b->fil.pts_off = align_up(sizeof(FilterRec) * nS, 256);
    b->fil.rot_off = b->fil.pts_off + sizeof(float2) * 2 * nS * nP;
    const size_t in_bytes = b->fil.rot_off + sizeof(float2) * nS, out_points = 3 * nS * nP;
    if (out_points > 0x7fffffffu) return RGRID_ERR_CAPACITY;                       // a record's offsets are ints
    if (b->seg.pack.size() < sizeof(FilterRec) * nS) b->seg.pack.resize(sizeof(FilterRec) * nS);
    b->fil.sub.resize(nS);
    if (!b->fil.in.h) G_TRY(b, b->fil.in.alloc(in_bytes));
    if (!b->fil.out.h) G_TRY(b, b->fil.out.alloc(out_points));
    // the keys and the table of an 8192-point cloud: 128 KB of LDS, above the 64 KB a launch gets unasked
    const int lds_max = (int)(KGF_SCRATCH + sizeof(int2) * (KGF_MAX_POINTS + 16) + sizeof(int) * (size_t)kgf_table_size(KGF_MAX_POINTS));
    G_TRY(b, hipFuncSetAttribute((const void *)kgb_filter<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    G_TRY(b, hipFuncSetAttribute((const void *)kgb_filter<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    G_TRY(b, b->fil.cnt.alloc(3 * nS));
    std::memset(b->fil.cnt.h, 0, sizeof(int) * 3 * nS);
    return RGRID_OK;
}

// how far a filter's packing has come: records, input points, output points, the largest cloud
struct FilterWork { int nrec, nin, nout, n_max; };

// the filter's staging (made by the handle's first filter) and an empty packing
int begin_filter(rgrid_batch_t *b, FilterWork &W)
{
    G_TRY(b, hipSetDevice(b->device));
    if (!b->fil.cnt.h) {
        const int rc = filter_staging(b);
        if (rc != RGRID_OK) return rc;
    }
    W = FilterWork{0, 0, 0, 0};
    return RGRID_OK;
}

// Scan j of a filter into b->fil.sub[j] and, when it can run, into a record (in the image of a match's records: free between
// submits) with its points forward, straight into the staging.  Gives the record, or null with the scan's status set.
FilterRec *pack_filter_scan(rgrid_batch_t *b, FilterWork &W, int j, const float *returns_xy, int n_returns, const float *misses_xy, int n_misses)
{
    const int cap = filter_point_cap(b);
    float *pts = reinterpret_cast<float *>(b->fil.in.h + b->fil.pts_off);
    FilterPending &P = b->fil.sub[(size_t)j];
    P.status = RGRID_OK; P.rec = -1; P.out_off = 0; P.n_ret = n_returns; P.n_mis = n_misses;
    if (n_returns > cap || n_misses > cap) { P.status = RGRID_ERR_CAPACITY; return nullptr; }
    if (!all_finite(returns_xy, 2 * (size_t)n_returns) || !all_finite(misses_xy, 2 * (size_t)n_misses)) { P.status = RGRID_ERR_INVALID; return nullptr; }
    FilterRec &R = reinterpret_cast<FilterRec *>(b->seg.pack.data())[W.nrec];
    R.n_ret = n_returns; R.n_mis = n_misses; R.ret_off = W.nin; R.mis_off = W.nin + n_returns; R.out_off = W.nout; R.pad = 0;
    if (n_returns > 0) std::memcpy(pts + 2 * (size_t)R.ret_off, returns_xy, sizeof(float) * 2 * (size_t)n_returns);   // forward, straight into the staging
    if (n_misses > 0) std::memcpy(pts + 2 * (size_t)R.mis_off, misses_xy, sizeof(float) * 2 * (size_t)n_misses);
    W.nin += n_returns + n_misses;
    W.nout += 2 * n_returns + n_misses;
    if (n_returns > W.n_max) W.n_max = n_returns;
    if (n_misses > W.n_max) W.n_max = n_misses;
    P.rec = W.nrec; P.out_off = R.out_off;
    ++W.nrec;
    return &R;
}

// the packed records into the staging (its own: no segment is taken)
void stage_filter(rgrid_batch_t *b, const FilterWork &W)
{
    std::memcpy(b->fil.in.h, b->seg.pack.data(), sizeof(FilterRec) * (size_t)W.nrec);
}

// one workgroup per record; ROT: every record has its (cos, sin) at rot_off of the staging
template <bool ROT>
void launch_filter(rgrid_batch_t *b, const rgrid_filter_options *opt, const FilterWork &W)
{
    FilterBufs Ff;
    Ff.in = b->fil.in.dv; Ff.pts_off = (int)b->fil.pts_off; Ff.key_cap = (W.n_max + 15) / 16 * 16 + 16;
    Ff.out = b->fil.out.dv; Ff.counts = b->fil.cnt.dv;
    Ff.min_pts = opt->adaptive_min_num_points;
    Ff.vsize = opt->voxel_filter_size; Ff.maxl = (float)opt->adaptive_max_length; Ff.max_range = (float)opt->adaptive_max_range;
    const size_t lds = KGF_SCRATCH + sizeof(int2) * (size_t)Ff.key_cap + sizeof(int) * (size_t)kgf_table_size(W.n_max);
    const float2 *rot = ROT ? reinterpret_cast<const float2 *>(b->fil.in.dv + b->fil.rot_off) : nullptr;
    ++b->n_launches;
    hipLaunchKernelGGL(kgb_filter<ROT>, dim3((unsigned)W.nrec), dim3(KGF_THREADS), lds, b->stream, Ff, rot);
}

// The staging of a texture or an occupancy call that writes `need` elements: the box records once, the output area when it is too small
template <typename T>
int export_staging(rgrid_batch_t *b, batch_host::Pinned<int> &box, batch_host::Pinned<T> &out, size_t &have, size_t need)
{
    if (!box.h) G_TRY(b, box.alloc(4 * (size_t)b->max_scans));
    if (need > have) {                                                             // it never shrinks
        G_TRY(b, hipStreamSynchronize(b->stream));                                 // (nothing is pending: the area is idle)
        out.release();
        have = 0;
        G_TRY(b, out.alloc(need));
        have = need;
    }
    return RGRID_OK;
}

// MapBuilder::ScanMatch for scans that passed match_scans_ok: the match's records, a refine record per match record (same index:
// the start pose is the match's winner, decoded on the device), both launches behind each other, KIND_SCAN_MATCH pending
int submit_scan_match(rgrid_batch_t *b, const rgrid_match_options *mopt, const rgrid_refine_options *ropt, const rgrid_batch_scan *scans, int count)
{
    const auto t_begin = std::chrono::steady_clock::now();
    const MatchWork W = pack_match(b, mopt, scans, count);
    int k = 0, nraw = 0, threads = 0;
    if (W.nrec > 0) {
        G_TRY(b, hipSetDevice(b->device));
        k = take_segment(b);
        for (int j = 0; j < count; ++j) {
            const Pending &P = b->sub[(size_t)j];
            if (P.status != RGRID_OK) continue;
            const rgrid_batch_scan &s = scans[j];
            RefineRec &R = pack_refine(b, k, P.rec, ropt, s.grid, s.points_xy, s.n, nraw, threads);
            R.plan_res = P.plan.res; R.plan_step = P.plan.step;
            R.ip[0] = s.initial_pose[0]; R.ip[1] = s.initial_pose[1]; R.ip[2] = s.initial_pose[2];
            R.match_rec = P.rec; R.num_linear = P.plan.num_linear; R.num_angular = P.plan.num_angular;
        }
        stage_match(b, k, W);
        std::memcpy(b->seg.buf[k].h + b->seg.rrec_off, b->seg.pack.data() + b->seg.rrec_off, sizeof(RefineRec) * (size_t)W.nrec);
    }
    return submit_tail(b, KIND_SCAN_MATCH, count, W.nrec, t_begin, [&] {
        launch_match(b, k, W);                                // the stream orders the refinement behind the match: no host wait between them
        launch_refine(b, k, W.nrec, threads);
    });
}

// tiles of KGL_THREADS points a cloud of the largest size has
int to_local_tiles(const rgrid_batch_t *b) { return (filter_point_cap(b) + KGL_THREADS - 1) / KGL_THREADS; }

// AddRangeData's own staging: kgb_to_local's records and workgroup table for max_scans scans, its output rows, the host's per-scan
// notes.  A call that fails part-way keeps what it allocated, and the next one goes on from there.
int range_data_staging(rgrid_batch_t *b)
{
    const size_t nS = (size_t)b->max_scans, nP = (size_t)filter_point_cap(b);
    b->ard.wgmap_off = align_up(sizeof(ToLocalRec) * nS, 256);
    b->ard.scan.resize(nS);
    b->ard.match.resize(nS);
    b->ard.ret.resize(2 * nP);
    b->ard.mis.resize(2 * nP);
    if (!b->ard.tab.h) G_TRY(b, b->ard.tab.alloc(b->ard.wgmap_off + sizeof(int2) * nS * (size_t)to_local_tiles(b)));
    G_TRY(b, b->ard.out.alloc(nS * nP));
    return RGRID_OK;
}

// one workgroup per (record, tile) of the table in the staging
void launch_to_local(rgrid_batch_t *b, int nwg)
{
    ToLocalBufs Lf;
    Lf.tab = b->ard.tab.dv; Lf.wgmap_off = (int)b->ard.wgmap_off;
    Lf.src = reinterpret_cast<const float2 *>(b->fil.in.dv + b->fil.pts_off); Lf.out = b->ard.out.dv;
    ++b->n_launches;
    hipLaunchKernelGGL(kgb_to_local, dim3((unsigned)nwg), dim3(KGL_THREADS), 0, b->stream, Lf);
}

}  // namespace

extern "C" {

int rgrid_batch_sizeof_scan(void) { return (int)sizeof(rgrid_batch_scan); }

int rgrid_batch_sizeof_refine_scan(void) { return (int)sizeof(rgrid_batch_refine_scan); }

int rgrid_batch_sizeof_insert_scan(void) { return (int)sizeof(rgrid_batch_insert_scan); }

const char *rgrid_batch_last_hip_error(rgrid_batch_t *b) { return b ? b->hip_error.c_str() : ""; }

double rgrid_batch_last_prepare_seconds(rgrid_batch_t *b) { return b ? b->prepare_seconds : 0.; }

int rgrid_batch_create(int max_scans, int max_points, int num_grids, long max_cells, int max_rotations, int device,
                       rgrid_batch_t **out)
{
    if (!out) return RGRID_ERR_INVALID;
    *out = nullptr;
    if (max_scans < 1 || max_points < 1 || num_grids < 1 || max_cells < 1 || max_rotations < 1) return RGRID_ERR_INVALID;
    // every offset into a segment and every workgroup index is an int
    const size_t nS = (size_t)max_scans, nP = (size_t)max_points, nR = (size_t)(max_rotations < KGB_MAX_ROT ? max_rotations : KGB_MAX_ROT);
    const size_t wgmap_off = align_up(sizeof(BatchRec) * nS, 256), f2_off = align_up(wgmap_off + sizeof(int2) * nS * nR, 256);
    const size_t rrec_off = align_up(f2_off + sizeof(float2) * nS * (nR + nP), 256), raw_off = align_up(rrec_off + sizeof(RefineRec) * nS, 256);
    const size_t seg_bytes = raw_off + sizeof(float2) * nS * nP;
    if (seg_bytes > 0x7fffffffu || (size_t)max_cells > 0x7fffffffu || max_points > KGB_MAX_POINTS) return RGRID_ERR_CAPACITY;
    rgrid_batch_t *b = new (std::nothrow) rgrid_batch();
    if (!b) return RGRID_ERR_INVALID;
    b->max_scans = max_scans; b->max_points = max_points; b->num_grids = num_grids; b->max_cells = max_cells;
    b->max_rotations = max_rotations; b->device = device;
    b->seg.wgmap_off = wgmap_off; b->seg.f2_off = f2_off; b->seg.rrec_off = rrec_off; b->seg.raw_off = raw_off;
    b->grids.resize((size_t)num_grids);
    b->ins.slot_call.assign((size_t)num_grids, 0ull);
    b->sub.resize(nS);
    b->seg.pack.resize(raw_off);           // (the raw points go straight into the segment)
    int rc = [&]() -> int {
        G_TRY(b, hipSetDevice(device));
        G_TRY(b, hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        // both segments of one kind: host-visible device memory is tried for the second only when the first got it, and must not fail then
        G_TRY(b, b->seg.buf[0].alloc(seg_bytes));
        G_TRY(b, b->seg.buf[0].in_vram ? b->seg.buf[1].alloc(seg_bytes) : b->seg.buf[1].alloc_pinned(seg_bytes));
        if (b->seg.buf[0].in_vram && !b->seg.buf[1].in_vram) { b->hip_error = "host-visible device memory: second segment refused"; return RGRID_ERR_HIP; }
        G_TRY(b, b->res.best.alloc(nS));
        std::memset(b->res.best.h, 0, sizeof(BestRec) * nS);
        G_TRY(b, b->res.fine.alloc(nS));
        std::memset(b->res.fine.h, 0, sizeof(RefineOut) * nS);
        G_TRY(b, b->ins.bad.alloc(nS));
        std::memset(b->ins.bad.h, 0, sizeof(int) * nS);
        G_TRY(b, b->ins.hit.alloc(32768)); G_TRY(b, b->ins.miss.alloc(32768));
        G_TRY(b, b->cells.alloc((size_t)num_grids * (size_t)max_cells));
        G_TRY(b, b->res.bb.alloc(nS * nR));
        G_TRY(b, b->res.arrived.alloc(nS));
        G_TRY(b, hipMemsetAsync(b->res.arrived.d, 0, sizeof(int) * nS, b->stream));
        // the rotated scan's indices in LDS: 8 B per point, 64 KB at 8192 points
        const int lds_max = (int)(sizeof(int2) * (nP + KGB_PF));
        G_TRY(b, hipFuncSetAttribute((const void *)kgb_match<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        G_TRY(b, hipFuncSetAttribute((const void *)kgb_match<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        return RGRID_OK;
    }();
    if (rc != RGRID_OK) { std::fprintf(stderr, "rgrid_batch_create: %s\n", b->hip_error.c_str()); rgrid_batch_destroy(b); return rc; }
    *out = b;
    return RGRID_OK;
}

void rgrid_batch_destroy(rgrid_batch_t *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    batch_host::release_all(b->cells, b->res.bb, b->res.arrived, b->ins.hit, b->ins.miss, b->tex.table, b->occ.tables, b->seg.buf[0], b->seg.buf[1],
                            b->res.best, b->res.fine, b->ins.bad, b->fil.in, b->fil.out, b->fil.cnt, b->ard.tab, b->ard.out, b->tex.out, b->tex.box,
                            b->occ.out, b->occ.box);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int rgrid_batch_set_reduction(rgrid_batch_t *b, int mode)
{
    if (!b || b->outstanding || (mode != RGRID_BATCH_REDUCE_ARRIVAL && mode != RGRID_BATCH_REDUCE_LAUNCH)) return RGRID_ERR_INVALID;
    b->mode = mode;
    return RGRID_OK;
}

int rgrid_batch_set_grid(rgrid_batch_t *b, int grid, const uint16_t *cells, int num_x_cells, int num_y_cells, double resolution,
                         double max_x, double max_y)
{
    if (!b || !cells || grid < 0 || grid >= b->num_grids || num_x_cells < 1 || num_y_cells < 1 || !(resolution > 0.) || b->outstanding)
        return RGRID_ERR_INVALID;
    if ((long long)num_x_cells * num_y_cells > (long long)b->max_cells) return RGRID_ERR_CAPACITY;
    G_TRY(b, hipSetDevice(b->device));
    G_TRY(b, hipMemcpyAsync(b->cells.d + cells_offset(b, grid), cells, sizeof(uint16_t) * (size_t)num_x_cells * num_y_cells,
                            hipMemcpyHostToDevice, b->stream));
    G_TRY(b, hipStreamSynchronize(b->stream));
    GridSlot &g = b->grids[(size_t)grid];
    g.set = true; g.nx = num_x_cells; g.ny = num_y_cells; g.resolution = resolution; g.max_x = max_x; g.max_y = max_y;
    return RGRID_OK;
}

int rgrid_batch_match_submit(rgrid_batch_t *b, const rgrid_match_options *opt, const rgrid_batch_scan *scans, int count)
{
    if (!b || !opt || count < 0 || count > b->max_scans || (count > 0 && !scans) || b->outstanding) return RGRID_ERR_INVALID;
    if (!match_scans_ok(b, scans, count)) return RGRID_ERR_INVALID;
    const auto t_begin = std::chrono::steady_clock::now();
    const MatchWork W = pack_match(b, opt, scans, count);
    int k = 0;
    if (W.nrec > 0) {
        G_TRY(b, hipSetDevice(b->device));
        k = take_segment(b);
        stage_match(b, k, W);
    }
    return submit_tail(b, KIND_MATCH, count, W.nrec, t_begin, [&] { launch_match(b, k, W); });
}

int rgrid_batch_match_collect(rgrid_batch_t *b, int *status, double *pose_estimates, double *scores, int *best3, int *info3)
{
    int count = 0;
    const int rc = collect_head(b, KIND_MATCH, status && pose_estimates && scores, true, &count);
    if (rc != RGRID_OK) return rc;
    for (int j = 0; j < count; ++j) {
        status[j] = b->sub[(size_t)j].status;
        match_result(b, j, pose_estimates, scores, best3, info3);
    }
    return RGRID_OK;
}

int rgrid_batch_refine_submit(rgrid_batch_t *b, const rgrid_refine_options *opt, const rgrid_batch_refine_scan *scans, int count)
{
    if (!b || !opt || count < 0 || count > b->max_scans || (count > 0 && !scans) || b->outstanding || !refine_options_ok(opt)) return RGRID_ERR_INVALID;
    for (int j = 0; j < count; ++j)
        if (!cloud_ok(b, scans[j].grid, scans[j].points_xy, scans[j].n)) return RGRID_ERR_INVALID;
    const auto t_begin = std::chrono::steady_clock::now();
    const int k = next_segment(b);
    int nrec = 0, nraw = 0, threads = 0;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_refine_scan &s = scans[j];
        Pending &P = fresh_pending(b, j);
        if (s.n == 0) { P.status = RGRID_ERR_EMPTY; continue; }
        if (s.n > b->max_points) { P.status = RGRID_ERR_CAPACITY; continue; }
        RefineRec &R = pack_refine(b, k, nrec, opt, s.grid, s.points_xy, s.n, nraw, threads);
        R.A.tx = s.target_translation[0]; R.A.ty = s.target_translation[1];
        R.A.x0 = s.initial_pose[0]; R.A.y0 = s.initial_pose[1]; R.A.a0 = s.initial_pose[2];
        R.match_rec = -1;
        P.status = RGRID_OK; P.rec = nrec;
        ++nrec;
    }
    if (nrec > 0) {
        G_TRY(b, hipSetDevice(b->device));
        take_segment(b);
        std::memcpy(b->seg.buf[k].h + b->seg.rrec_off, b->seg.pack.data() + b->seg.rrec_off, sizeof(RefineRec) * (size_t)nrec);
    }
    return submit_tail(b, KIND_REFINE, count, nrec, t_begin, [&] { launch_refine(b, k, nrec, threads); });
}

int rgrid_batch_refine_collect(rgrid_batch_t *b, int *status, double *pose_estimates, rgrid_refine_summary *summaries)
{
    int count = 0;
    const int rc = collect_head(b, KIND_REFINE, status && pose_estimates, true, &count);
    if (rc != RGRID_OK) return rc;
    for (int j = 0; j < count; ++j) {
        status[j] = b->sub[(size_t)j].status;
        refine_result(b, b->sub[(size_t)j], &pose_estimates[3 * j], summaries ? &summaries[j] : nullptr);
    }
    return RGRID_OK;
}

int rgrid_batch_scan_match_submit(rgrid_batch_t *b, const rgrid_match_options *mopt, const rgrid_refine_options *ropt,
                                  const rgrid_batch_scan *scans, int count)
{
    if (!b || !mopt || !ropt || count < 0 || count > b->max_scans || (count > 0 && !scans) || b->outstanding || !refine_options_ok(ropt))
        return RGRID_ERR_INVALID;
    if (!match_scans_ok(b, scans, count)) return RGRID_ERR_INVALID;
    return submit_scan_match(b, mopt, ropt, scans, count);
}

int rgrid_batch_scan_match_collect(rgrid_batch_t *b, int *status, double *coarse_poses, double *scores, int *best3, int *info3,
                                   double *pose_estimates, rgrid_refine_summary *summaries)
{
    int count = 0;
    const int rc = collect_head(b, KIND_SCAN_MATCH, status && coarse_poses && scores && pose_estimates, true, &count);
    if (rc != RGRID_OK) return rc;
    for (int j = 0; j < count; ++j) {
        status[j] = b->sub[(size_t)j].status;
        match_result(b, j, coarse_poses, scores, best3, info3);
        refine_result(b, b->sub[(size_t)j], &pose_estimates[3 * j], summaries ? &summaries[j] : nullptr);
    }
    return RGRID_OK;
}

int rgrid_batch_get_limits(rgrid_batch_t *b, int grid, int *num_x_cells, int *num_y_cells, double *resolution, double *max_x, double *max_y)
{
    if (!b || !slot_ok(b, grid) || b->outstanding) return RGRID_ERR_INVALID;
    const GridSlot &g = b->grids[(size_t)grid];
    if (num_x_cells) *num_x_cells = g.nx;
    if (num_y_cells) *num_y_cells = g.ny;
    if (resolution) *resolution = g.resolution;
    if (max_x) *max_x = g.max_x;
    if (max_y) *max_y = g.max_y;
    return RGRID_OK;
}

int rgrid_batch_get_grid(rgrid_batch_t *b, int grid, uint16_t *cells, long cap)
{
    if (!b || !cells || !slot_ok(b, grid) || b->outstanding) return RGRID_ERR_INVALID;
    const GridSlot &g = b->grids[(size_t)grid];
    const long long ncells = (long long)g.nx * g.ny;
    if (cap < ncells) return RGRID_ERR_BUFFER;
    G_TRY(b, hipSetDevice(b->device));
    G_TRY(b, hipMemcpyAsync(cells, b->cells.d + cells_offset(b, grid), sizeof(uint16_t) * (size_t)ncells, hipMemcpyDeviceToHost, b->stream));
    G_TRY(b, hipStreamSynchronize(b->stream));
    return RGRID_OK;
}

int rgrid_batch_insert_submit(rgrid_batch_t *b, const rgrid_insert_options *opt, const rgrid_batch_insert_scan *scans, int count)
{
    // (scans == NULL is refused at count == 0 too, unlike the match, the refinement and the texture: callers may rely on it)
    if (!b || !opt || !scans || count < 0 || count > b->max_scans || b->outstanding) return RGRID_ERR_INVALID;
    if (!insert_options_ok(opt->hit_probability, opt->miss_probability)) return RGRID_ERR_INVALID;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_insert_scan &s = scans[j];
        if (!slot_ok(b, s.grid) || !two_clouds_ok(s.returns_xy, s.n_returns, s.misses_xy, s.n_misses)) return RGRID_ERR_INVALID;
    }
    if (!slots_named_once(b, scans, count)) return RGRID_ERR_INVALID;
    const auto t_begin = std::chrono::steady_clock::now();
    InsertWork W;
    const int rc = begin_insert(b, opt, W);
    if (rc != RGRID_OK) return rc;
    for (int j = 0; j < count; ++j) pack_insert_scan(b, W, scans[j], j);
    stage_insert(b, W);
    return submit_tail(b, KIND_INSERT, count, W.nrec, t_begin, [&] { launch_insert(b, opt, W); });
}

int rgrid_batch_insert_collect(rgrid_batch_t *b, int *status)
{
    int count = 0;
    const int rc = collect_head(b, KIND_INSERT, status != nullptr, true, &count);
    if (rc != RGRID_OK) return rc;
    for (int j = 0; j < count; ++j) status[j] = insert_status(b, j);
    return RGRID_OK;
}

int rgrid_batch_filter_max_points(void) { return KGF_MAX_POINTS; }

int rgrid_batch_sizeof_filter_scan(void) { return (int)sizeof(rgrid_batch_filter_scan); }

int rgrid_batch_filter_submit(rgrid_batch_t *b, const rgrid_filter_options *opt, const rgrid_batch_filter_scan *scans, int count)
{
    // (scans == NULL is refused at count == 0 too, as by the inserter)
    if (!b || !opt || !scans || count < 0 || count > b->max_scans || b->outstanding) return RGRID_ERR_INVALID;
    if (!filter_options_ok(opt)) return RGRID_ERR_INVALID;
    for (int j = 0; j < count; ++j)
        if (!two_clouds_ok(scans[j].returns_xy, scans[j].n_returns, scans[j].misses_xy, scans[j].n_misses)) return RGRID_ERR_INVALID;
    const auto t_begin = std::chrono::steady_clock::now();
    FilterWork W;
    const int rc = begin_filter(b, W);
    if (rc != RGRID_OK) return rc;
    for (int j = 0; j < count; ++j) pack_filter_scan(b, W, j, scans[j].returns_xy, scans[j].n_returns, scans[j].misses_xy, scans[j].n_misses);
    stage_filter(b, W);
    return submit_tail(b, KIND_FILTER, count, W.nrec, t_begin, [&] { launch_filter<false>(b, opt, W); });
}

int rgrid_batch_filter_collect(rgrid_batch_t *b, int *status, int *counts, float *out_xy, long out_cap_points)
{
    if (out_cap_points < 0) return RGRID_ERR_INVALID;
    int count = 0;
    const int rc = collect_head(b, KIND_FILTER, status && counts, false, &count);
    if (rc != RGRID_OK) return rc;
    long total = 0;
    for (int j = 0; j < count; ++j) {
        const FilterPending &P = b->fil.sub[(size_t)j];
        status[j] = P.status;
        for (int c = 0; c < 3; ++c) total += counts[3 * j + c] = P.rec >= 0 ? b->fil.cnt.h[3 * P.rec + c] : 0;
    }
    if (total > out_cap_points || (total > 0 && !out_xy)) return RGRID_ERR_BUFFER;         // the submit stays pending: come again with room
    b->outstanding = false;
    float *dst = out_xy;
    for (int j = 0; j < count; ++j) {
        const FilterPending &P = b->fil.sub[(size_t)j];
        if (P.rec < 0) continue;
        const int off[3] = {P.out_off, P.out_off + P.n_ret, P.out_off + P.n_ret + P.n_mis};   // fr, fm, av as the kernel laid them out
        for (int c = 0; c < 3; ++c) {
            const size_t k = (size_t)counts[3 * j + c];
            if (k > 0) std::memcpy(dst, b->fil.out.h + off[c], sizeof(float2) * k);
            dst += 2 * k;
        }
    }
    return RGRID_OK;
}

int rgrid_batch_texture_submit(rgrid_batch_t *b, const int *grids, int count)
{
    if (!b || count < 0 || count > b->max_scans || (count > 0 && !grids) || b->outstanding) return RGRID_ERR_INVALID;
    size_t pairs = 0;
    for (int j = 0; j < count; ++j) {
        if (!slot_ok(b, grids[j])) return RGRID_ERR_INVALID;
        const GridSlot &g = b->grids[(size_t)grids[j]];
        pairs += align_up((size_t)g.nx * (size_t)g.ny, 8);                          // every region starts on a 16-byte boundary
    }
    const auto t_begin = std::chrono::steady_clock::now();
    int k = 0;
    if (count > 0) {                                                               // (a call without a slot allocates nothing and takes no segment)
        G_TRY(b, hipSetDevice(b->device));
        G_TRY(b, resident_texture_table(b->tex.table.d));
        b->tex.sub.resize((size_t)b->max_scans);
        const int rc = export_staging(b, b->tex.box, b->tex.out, b->tex.out_pairs, pairs);
        if (rc != RGRID_OK) return rc;
        k = take_segment(b);
        TextureRec *recs = reinterpret_cast<TextureRec *>(b->seg.pack.data());
        long long at = 0;
        for (int j = 0; j < count; ++j) {
            const GridSlot &g = b->grids[(size_t)grids[j]];
            TextureRec &R = recs[j];
            R.cells_off = cells_offset(b, grids[j]);
            R.out_off = at; R.nx = g.nx; R.ny = g.ny;
            b->tex.sub[(size_t)j] = TexturePending{grids[j], at};
            at += (long long)align_up((size_t)g.nx * (size_t)g.ny, 8);
        }
        std::memcpy(b->seg.buf[k].h, recs, sizeof(TextureRec) * (size_t)count);
    }
    return submit_tail(b, KIND_TEXTURE, count, count, t_begin, [&] {
        TextureBufs Tf;
        Tf.seg = b->seg.buf[k].dv; Tf.cells = b->cells.d; Tf.table = b->tex.table.d; Tf.out = b->tex.out.dv; Tf.box = b->tex.box.dv;
        hipLaunchKernelGGL(kgb_texture, dim3((unsigned)count), dim3(KGT_THREADS), 0, b->stream, Tf);
    });
}

int rgrid_batch_texture_collect(rgrid_batch_t *b, int *boxes, double *slice_max, long *offsets, uint8_t *cells, long cap)
{
    int count = 0;
    const int rc = collect_head(b, KIND_TEXTURE, boxes && slice_max && offsets, false, &count);   // the one wait: the kernel wrote boxes and pairs into host memory
    if (rc != RGRID_OK) return rc;
    long total = 0;
    for (int j = 0; j < count; ++j) {
        const GridSlot &g = b->grids[(size_t)b->tex.sub[(size_t)j].grid];
        const int *box = b->tex.box.h + 4 * j;
        for (int c = 0; c < 4; ++c) boxes[4 * j + c] = box[c];
        slice_max_of(box, g.resolution, g.max_x, g.max_y, &slice_max[2 * j]);
        offsets[j] = total;
        total += 2l * box[2] * box[3];
    }
    if (total > cap || (total > 0 && !cells)) return RGRID_ERR_BUFFER;             // the submit stays pending: come again with room
    b->outstanding = false;
    for (int j = 0; j < count; ++j)
        std::memcpy(cells + offsets[j], b->tex.out.h + b->tex.sub[(size_t)j].out_off, 2 * (size_t)boxes[4 * j + 2] * (size_t)boxes[4 * j + 3]);
    return RGRID_OK;
}

int rgrid_batch_occupancy_submit(rgrid_batch_t *b, int mode, const int *grids, const double *submap_origins, int count)
{
    if (!b || count < 0 || count > b->max_scans || (count > 0 && (!grids || !submap_origins)) || b->outstanding) return RGRID_ERR_INVALID;
    if (mode != OCC_MODE_OCCUPANCY && mode != OCC_MODE_IMAGE) return RGRID_ERR_INVALID;
    size_t bytes = 0;
    for (int j = 0; j < count; ++j) {
        if (!slot_ok(b, grids[j])) return RGRID_ERR_INVALID;
        const GridSlot &g = b->grids[(size_t)grids[j]];
        bytes += occupancy_block_bytes(g.nx, g.ny);                                // a multiple of 16: every region starts on a 16-byte boundary
    }
    const auto t_begin = std::chrono::steady_clock::now();
    int k = 0;
    if (count > 0) {                                                               // (a call without a slot allocates nothing and takes no segment)
        G_TRY(b, hipSetDevice(b->device));
        G_TRY(b, resident_occupancy_tables(b->occ.tables.d));
        b->occ.sub.resize((size_t)b->max_scans); b->occ.frame.resize((size_t)b->max_scans);
        const int rc = export_staging(b, b->occ.box, b->occ.out, b->occ.out_bytes, bytes);
        if (rc != RGRID_OK) return rc;
        k = take_segment(b);
        OccupancyRec *recs = reinterpret_cast<OccupancyRec *>(b->seg.pack.data());
        long long at = 0;
        for (int j = 0; j < count; ++j) {
            const GridSlot &g = b->grids[(size_t)grids[j]];
            OccupancyRec &R = recs[j];
            R.cells_off = cells_offset(b, grids[j]);
            R.out_off = at; R.nx = g.nx; R.ny = g.ny;
            b->occ.sub[(size_t)j] = OccupancyPending{grids[j], at, {submap_origins[2 * j], submap_origins[2 * j + 1]}};
            at += (long long)occupancy_block_bytes(g.nx, g.ny);
        }
        std::memcpy(b->seg.buf[k].h, recs, sizeof(OccupancyRec) * (size_t)count);
        b->occ.mode = mode;
    }
    return submit_tail(b, KIND_OCCUPANCY, count, count, t_begin, [&] {
        OccupancyBufs Of;
        Of.seg = b->seg.buf[k].dv; Of.cells = b->cells.d; Of.table = b->occ.tables.d + (mode == OCC_MODE_IMAGE ? 32768 : 0);
        Of.out = b->occ.out.dv; Of.box = b->occ.box.dv;
        hipLaunchKernelGGL(kgb_occupancy, dim3((unsigned)count), dim3(KGT_THREADS), 0, b->stream, Of);
    });
}

int rgrid_batch_occupancy_collect(rgrid_batch_t *b, int *status, int *sizes, double *origins, int *boxes, long *offsets, int8_t *out, long cap)
{
    int count = 0;
    const int rc = collect_head(b, KIND_OCCUPANCY, status && sizes && origins && boxes && offsets, false, &count);   // the one wait: the kernel wrote boxes and blocks into host memory
    if (rc != RGRID_OK) return rc;
    long total = 0;
    for (int j = 0; j < count; ++j) {
        const OccupancyPending &P = b->occ.sub[(size_t)j];
        const GridSlot &g = b->grids[(size_t)P.grid];
        const int *box = b->occ.box.h + 4 * j;
        OccupancyFrame &F = b->occ.frame[(size_t)j];
        for (int c = 0; c < 4; ++c) boxes[4 * j + c] = box[c];
        status[j] = occupancy_frame(box, g.resolution, g.max_x, g.max_y, P.submap_origin, &F);
        if (status[j] != RGRID_OK) F = OccupancyFrame{{0, 0}, {0., 0.}};           // outside the domain: no image
        sizes[2 * j] = F.size[0]; sizes[2 * j + 1] = F.size[1];
        origins[2 * j] = F.origin[0]; origins[2 * j + 1] = F.origin[1];
        offsets[j] = total;
        total += (long)F.size[0] * F.size[1];
    }
    if (total > cap || (total > 0 && !out)) return RGRID_ERR_BUFFER;               // the submit stays pending: come again with room
    b->outstanding = false;
    for (int j = 0; j < count; ++j)
        if (status[j] == RGRID_OK)
            occupancy_paint(b->occ.mode, b->occ.out.h + b->occ.sub[(size_t)j].out_off, boxes[4 * j + 2], boxes[4 * j + 3], &sizes[2 * j],
                            reinterpret_cast<unsigned char *>(out) + offsets[j]);
    return RGRID_OK;
}

int rgrid_batch_sizeof_range_data(void) { return (int)sizeof(rgrid_batch_range_data); }

int rgrid_batch_last_call_counts(rgrid_batch_t *b, int launches_syncs[2])
{
    if (!b || !launches_syncs) return RGRID_ERR_INVALID;
    launches_syncs[0] = b->ard.last_counts[0]; launches_syncs[1] = b->ard.last_counts[1];
    return RGRID_OK;
}

// mapping::MapBuilder::AddRangeData (map_builder.cc:57-108) for one scan of every robot: rgrid_add_range_data's steps, each of them
// the batch's own stage -- the single-kind submits' packing and launches, a collect_head per wait -- with the host doing between
// them what rgrid_add_range_data's host does, through the same functions (rgrid_dev.h).  DESIGN.md 10.10.
int rgrid_batch_add_range_data(rgrid_batch_t *b, const rgrid_map_builder_options *opt, const rgrid_batch_range_data *scans, int count,
                               int *codes, int *status, double *local_poses, float *origins_in_local, float *returns_in_local, long cap_points)
{
#pragma clang fp contract(off)
    if (!b || !opt || !scans || !codes || !status || !local_poses || !origins_in_local) return RGRID_ERR_INVALID;
    if (count < 0 || count > b->max_scans || b->outstanding) return RGRID_ERR_INVALID;
    const rgrid_filter_options fopt = {opt->voxel_filter_size, opt->adaptive_max_length, opt->adaptive_min_num_points, opt->adaptive_max_range};
    const rgrid_insert_options iopt = {opt->hit_probability, opt->miss_probability, opt->insert_free_space};
    if (!filter_options_ok(&fopt) || !refine_options_ok(&opt->refine) || !insert_options_ok(iopt.hit_probability, iopt.miss_probability)) return RGRID_ERR_INVALID;
    long total = 0;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_range_data &s = scans[j];
        if (s.grid < 0 || s.grid >= b->num_grids || !two_clouds_ok(s.returns_xy, s.n_returns, s.misses_xy, s.n_misses)) return RGRID_ERR_INVALID;
        total += s.n_returns;
    }
    if (!slots_named_once(b, scans, count)) return RGRID_ERR_INVALID;
    if (returns_in_local && cap_points < total) return RGRID_ERR_BUFFER;
    b->ard.last_counts[0] = b->ard.last_counts[1] = 0;
    if (count == 0) return RGRID_OK;
    const unsigned long long launches0 = b->n_launches, syncs0 = b->n_syncs;
    auto t_begin = std::chrono::steady_clock::now();
    int waited = 0;
    // ---- 1. gravity alignment and the three filters: one launch of kgb_filter<true>, one wait
    FilterWork F;
    int rc = begin_filter(b, F);
    if (rc != RGRID_OK) return rc;
    if (!b->ard.out.h && (rc = range_data_staging(b)) != RGRID_OK) return rc;     // the first call of this handle
    float2 *rot = reinterpret_cast<float2 *>(b->fil.in.h + b->fil.rot_off);
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_range_data &s = scans[j];
        RangeScan &S = b->ard.scan[(size_t)j];
        std::memset(&S, 0, sizeof(S));
        S.frec = S.mrec = -1;
        codes[j] = RGRID_OK; status[j] = RGRID_SCAN_DROPPED_EMPTY;
        zero3(&local_poses[3 * j]);
        origins_in_local[2 * j] = origins_in_local[2 * j + 1] = 0.f;
        if (s.n_returns == 0) continue;                                          // "Dropped empty horizontal range data." (:63-67)
        const FilterRec *R = pack_filter_scan(b, F, j, s.returns_xy, s.n_returns, s.misses_xy, s.n_misses);
        if (!R) { codes[j] = b->fil.sub[(size_t)j].status; continue; }
        double qw, qz;
        float yaw_g, c, sn;
        gravity_alignment(s.ekf_pose[2], qw, qz, yaw_g);
        rigid2f_cs(yaw_g, &c, &sn);
        S.frec = b->fil.sub[(size_t)j].rec; S.src_off = R->ret_off; S.out_off = R->out_off;
        rot[S.frec] = make_float2(c, sn);
    }
    if (F.nrec > 0) {
        stage_filter(b, F);
        if ((rc = submit_tail(b, KIND_FILTER, count, F.nrec, t_begin, [&] { launch_filter<true>(b, &fopt, F); })) != RGRID_OK) return rc;
        if ((rc = collect_head(b, KIND_FILTER, true, true, &waited)) != RGRID_OK) return rc;
    }
    // ---- 2. the decisions (:61-77), 3. ScanMatch for the scans that have a grid: the adaptively filtered clouds read where the
    // filter wrote them, the prediction (x, y, 0) -- the rotations cancel (:70-71) -- as start; two launches, one wait
    int nm = 0;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_range_data &s = scans[j];
        RangeScan &S = b->ard.scan[(size_t)j];
        if (S.frec < 0) continue;
        const int *c = b->fil.cnt.h + 3 * S.frec;
        S.n_fr = c[0]; S.n_fm = c[1]; S.n_av = c[2];
        status[j] = RGRID_SCAN_FILTERED_EMPTY;
        S.est[0] = s.ekf_pose[0]; S.est[1] = s.ekf_pose[1]; S.est[2] = 0.0;
        if (S.n_av == 0 || !b->grids[(size_t)s.grid].set) continue;              // (:74-77); no submap yet -> the prediction (:34-55)
        rgrid_batch_scan &m = b->ard.match[(size_t)nm];
        m.grid = s.grid; m.n = S.n_av;
        m.points_xy = reinterpret_cast<const float *>(b->fil.out.h + S.out_off + s.n_returns + s.n_misses);
        m.initial_pose[0] = S.est[0]; m.initial_pose[1] = S.est[1]; m.initial_pose[2] = S.est[2];
        S.mrec = nm++;
    }
    if (nm > 0) {
        if ((rc = submit_scan_match(b, &opt->match, &opt->refine, b->ard.match.data(), nm)) != RGRID_OK) return rc;
        if ((rc = collect_head(b, KIND_SCAN_MATCH, true, true, &waited)) != RGRID_OK) return rc;
        for (int j = 0; j < count; ++j) {                                        // (the insert's packing reuses b->sub)
            RangeScan &S = b->ard.scan[(size_t)j];
            if (S.mrec < 0) continue;
            const Pending &P = b->sub[(size_t)S.mrec];
            if (P.status != RGRID_OK) { codes[j] = P.status; continue; }
            refine_result(b, P, S.est, nullptr);
        }
    }
    // ---- 4. the pose compositions (rgrid_dev.h's, as in rgrid_add_range_data) and the insert's packing: the filtered clouds moved by
    // Embed3D(pose_estimate_2d.cast<float>()) on their way from the filter's output into the insert's segment
    t_begin = std::chrono::steady_clock::now();
    InsertWork I;
    if ((rc = begin_insert(b, &iopt, I)) != RGRID_OK) return rc;
    ToLocalRec *lrecs = reinterpret_cast<ToLocalRec *>(b->ard.tab.h);
    int2 *wgmap = reinterpret_cast<int2 *>(b->ard.tab.h + b->ard.wgmap_off);
    int nl = 0, nwg = 0, ndst = 0;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_range_data &s = scans[j];
        RangeScan &S = b->ard.scan[(size_t)j];
        if (S.frec < 0 || S.n_av == 0 || codes[j] != RGRID_OK) continue;
        const double *est = S.est;
        double qw, qz;
        float yaw_g;
        gravity_alignment(s.ekf_pose[2], qw, qz, yaw_g);
        // pose_estimate = Embed3D(pose_estimate_2d) * gravity_alignment (:86-87); the filtered data moves by yaw2 (:92-94)
        float yaw_f32, yaw2, org2[2];
        compose_pose_estimate(est, qw, qz, &local_poses[3 * j], yaw_f32, yaw2);
        origin_in_local(s.origin_xy, yaw_g, est, yaw2, org2);
        origins_in_local[2 * j] = org2[0]; origins_in_local[2 * j + 1] = org2[1];
        const float *fr = reinterpret_cast<const float *>(b->fil.out.h + S.out_off), *fm = fr + 2 * (size_t)s.n_returns;
        rigid2f_apply((float)est[0], (float)est[1], yaw2, fr, S.n_fr, b->ard.ret.data());
        if (S.n_fm > 0) rigid2f_apply((float)est[0], (float)est[1], yaw2, fm, S.n_fm, b->ard.mis.data());
        GridSlot &g = b->grids[(size_t)s.grid];
        if (!g.set) {                                                            // InsertIntoSubmap / CreateGrid (:110-126)
            codes[j] = initial_submap_limits(opt->resolution, org2, (long long)b->max_cells, g.nx, g.ny, g.resolution, g.max_x, g.max_y);
            if (codes[j] != RGRID_OK) continue;                                  // the slot stays unset
            G_TRY(b, hipMemsetAsync(b->cells.d + cells_offset(b, s.grid), 0, sizeof(uint16_t) * (size_t)g.nx * g.ny, b->stream));
            g.set = true;
        }
        rgrid_batch_insert_scan is;
        is.grid = s.grid; is.n_returns = S.n_fr; is.n_misses = S.n_fm;
        is.returns_xy = b->ard.ret.data(); is.misses_xy = S.n_fm > 0 ? b->ard.mis.data() : nullptr;
        is.origin_xy[0] = org2[0]; is.origin_xy[1] = org2[1];
        pack_insert_scan(b, I, is, j);
        const Pending &P = b->sub[(size_t)j];
        if (P.status != RGRID_OK) { codes[j] = P.status; continue; }
        S.packed = true;
        if (!returns_in_local) continue;
        // range_data_in_local.returns = the RAW returns through pose_estimate.cast<float>() (:89-90): kgb_to_local's record
        ToLocalRec L;
        L.src_off = S.src_off; L.dst_off = S.dst_off = ndst; L.n = s.n_returns; L.pad = 0;
        rigid2f_cs(yaw_f32, &L.c, &L.s);
        L.tx = (float)est[0]; L.ty = (float)est[1];
        lrecs[nl] = L;
        for (int t = 0; t * KGL_THREADS < s.n_returns; ++t) wgmap[nwg++] = make_int2(nl, t);
        ndst += s.n_returns;
        ++nl;
    }
    // ---- 5. the insert and the raw returns: two launches behind each other, one wait
    stage_insert(b, I);
    if (I.nrec > 0) {
        rc = submit_tail(b, KIND_INSERT, count, I.nrec, t_begin, [&] {
            launch_insert(b, &iopt, I);
            if (nwg > 0) launch_to_local(b, nwg);
        });
        if (rc != RGRID_OK) return rc;
        if ((rc = collect_head(b, KIND_INSERT, true, true, &waited)) != RGRID_OK) return rc;
    }
    long at = 0;
    for (int j = 0; j < count; ++j) {
        const RangeScan &S = b->ard.scan[(size_t)j];
        const long n = scans[j].n_returns;
        if (S.packed) {
            const int st = insert_status(b, j);
            if (st != RGRID_OK) codes[j] = st;
            else {
                status[j] = RGRID_SCAN_INSERTED;
                if (returns_in_local) std::memcpy(returns_in_local + 2 * at, b->ard.out.h + S.dst_off, sizeof(float2) * (size_t)n);
            }
        }
        at += n;
    }
    b->ard.last_counts[0] = (int)(b->n_launches - launches0); b->ard.last_counts[1] = (int)(b->n_syncs - syncs0);
    return RGRID_OK;
}

}  // extern "C"
