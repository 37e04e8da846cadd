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
// Per-call data -- a record per scan, the workgroup -> (record, rotation) map, the rotation tables and the rotated points --
// is packed into one of two staging segments that the kernel reads in place: fine-grained device memory the host writes
// directly where the platform maps it, else pinned host memory (host_visible.h).  Results land in pinned host memory, a slot
// per scan, published by the end of the launch.
#include "../../include/rgrid.h"
#include "host_visible.h"
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

enum { KIND_MATCH = 1, KIND_REFINE = 2, KIND_SCAN_MATCH = 3 };                   // the pending submit

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// what rgrid_refine_match refuses (the reference CHECK_GTs the weights, ceres_scan_matcher_2d.cc:37,47,52)
bool refine_options_ok(const rgrid_refine_options *o)
{
    return o->occupied_space_weight > 0. && o->translation_weight > 0. && o->rotation_weight > 0. && o->max_num_iterations >= 0;
}

// RefineArgs as rgrid_refine_match fills them, without the poses
void refine_args(RefineArgs &A, const GridSlot &g, const rgrid_refine_options *opt, int n)
{
    std::memset(&A, 0, sizeof(A));
    A.nx = g.nx; A.ny = g.ny; A.n = n; A.max_iter = opt->max_num_iterations; A.max_nonmono = opt->use_nonmonotonic_steps ? 5 : 0;
    A.res = g.resolution; A.max_x = g.max_x; A.max_y = g.max_y;
    A.w_occ = opt->occupied_space_weight; A.w_t = opt->translation_weight; A.w_r = opt->rotation_weight;
}

int refine_threads(int n) { const int t = ((n + 63) / 64) * 64; return t < 1024 ? t : 1024; }   // = rgrid_refine_match's

}  // namespace

struct rgrid_batch {
    int max_scans = 0, max_points = 0, num_grids = 0, max_rotations = 0, device = 0;
    long max_cells = 0;
    int mode = RGRID_BATCH_REDUCE_ARRIVAL;
    hipStream_t stream = nullptr;
    // staging segments the kernels read in place
    unsigned char *h_seg[KGB_SEGMENTS] = {nullptr, nullptr};
    const unsigned char *dv_seg[KGB_SEGMENTS] = {nullptr, nullptr};
    bool seg_in_vram = false;
    size_t seg_bytes = 0, wgmap_off = 0, f2_off = 0, rrec_off = 0, raw_off = 0;
    std::vector<unsigned char> pack;       // the segment's image in ordinary memory (rotated points are read back while packing)
    unsigned long long n_submit = 0;
    unsigned short *d_cells = nullptr;     // grid pool
    unsigned long long *d_bb = nullptr;
    int *d_arrived = nullptr;
    BestRec *h_out = nullptr, *dv_out = nullptr;
    RefineOut *h_rout = nullptr, *dv_rout = nullptr;
    std::vector<GridSlot> grids;
    bool outstanding = false;
    int kind = 0;                          // KIND_* of the outstanding submit
    int sub_count = 0;
    std::vector<Pending> sub;
    double prepare_seconds = 0.;
    std::string hip_error;
};

namespace {

// the whole-call conditions on the scans of a match (or match-plus-refine) submit
bool match_scans_ok(const rgrid_batch_t *b, const rgrid_batch_scan *scans, int count)
{
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_scan &s = scans[j];
        if (s.grid < 0 || s.grid >= b->num_grids || !b->grids[(size_t)s.grid].set || s.n < 0 || (s.n > 0 && !s.points_xy)) return false;
    }
    return true;
}

// Plans every scan of a match into b->sub and the segment's image b->pack: records, workgroup map, rotated points, rotation tables
MatchWork pack_match(rgrid_batch_t *b, const rgrid_match_options *opt, const rgrid_batch_scan *scans, int count)
{
#pragma clang fp contract(off)
    const int rot_cap = b->max_rotations < KGB_MAX_ROT ? b->max_rotations : KGB_MAX_ROT;
    BatchRec *recs = reinterpret_cast<BatchRec *>(b->pack.data());
    int2 *wgmap = reinterpret_cast<int2 *>(b->pack.data() + b->wgmap_off);
    float *f2 = reinterpret_cast<float *>(b->pack.data() + b->f2_off);
    int nrec = 0, nwg = 0, nf2 = 0, n_max = 0;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_scan &s = scans[j];
        const GridSlot &g = b->grids[(size_t)s.grid];
        Pending &P = b->sub[(size_t)j];
        std::memset(&P, 0, sizeof(P));
        P.rec = -1;
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
        A.cells_off = (long long)s.grid * (long long)b->max_cells;
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
    std::memcpy(b->h_seg[k], b->pack.data(), sizeof(BatchRec) * (size_t)W.nrec);
    std::memcpy(b->h_seg[k] + b->wgmap_off, b->pack.data() + b->wgmap_off, sizeof(int2) * (size_t)W.nwg);
    std::memcpy(b->h_seg[k] + b->f2_off, b->pack.data() + b->f2_off, sizeof(float2) * (size_t)W.nf2);
}

void launch_match(rgrid_batch_t *b, int k, const MatchWork &W)
{
    BatchBufs Bf;
    Bf.seg = b->dv_seg[k]; Bf.wgmap_off = (int)b->wgmap_off; Bf.f2_off = (int)b->f2_off;
    Bf.cells = b->d_cells; Bf.bb = b->d_bb; Bf.arrived = b->d_arrived; Bf.out = b->dv_out;
    Bf.max_rotations = b->max_rotations < KGB_MAX_ROT ? b->max_rotations : KGB_MAX_ROT;
    const size_t lds = sizeof(int2) * (size_t)((W.n_max + KGB_PF - 1) / KGB_PF * KGB_PF);
    if (b->mode == RGRID_BATCH_REDUCE_ARRIVAL) {
        hipLaunchKernelGGL(kgb_match<true>, dim3((unsigned)W.nwg), dim3(KGB_THREADS), lds, b->stream, Bf);
    } else {
        hipLaunchKernelGGL(kgb_match<false>, dim3((unsigned)W.nwg), dim3(KGB_THREADS), lds, b->stream, Bf);
        hipLaunchKernelGGL(kgb_best, dim3((unsigned)W.nrec), dim3(KGB_THREADS), 0, b->stream, Bf);
    }
}

// one workgroup per refine record of segment k, `threads` = the largest scan's thread count
void launch_refine(rgrid_batch_t *b, int k, int nrec, int threads)
{
    RefineBufs Rf;
    Rf.seg = b->dv_seg[k]; Rf.rrec_off = (int)b->rrec_off; Rf.raw_off = (int)b->raw_off;
    Rf.cells = b->d_cells; Rf.best = b->dv_out; Rf.out = b->dv_rout;
    hipLaunchKernelGGL(kgb_refine, dim3((unsigned)nrec), dim3((unsigned)threads), 0, b->stream, Rf);
}

double seconds_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

void zero3(double *p) { p[0] = p[1] = p[2] = 0.; }
void zero3(int *p) { if (p) p[0] = p[1] = p[2] = 0; }

// a scan's refine outputs from its result record (all zero when it had none)
void refine_result(const rgrid_batch_t *b, const Pending &P, double *pose, rgrid_refine_summary *summary)
{
    zero3(pose);
    if (summary) std::memset(summary, 0, sizeof(*summary));
    if (P.status != RGRID_OK) return;
    const RefineOut &o = b->h_rout[P.rec];
    pose[0] = o.pose[0]; pose[1] = o.pose[1]; pose[2] = o.pose[2];
    if (summary) { summary->initial_cost = o.initial_cost; summary->final_cost = o.final_cost; summary->iterations = o.iterations; summary->termination = o.termination; }
}

}  // namespace

extern "C" {

int rgrid_batch_sizeof_scan(void) { return (int)sizeof(rgrid_batch_scan); }

int rgrid_batch_sizeof_refine_scan(void) { return (int)sizeof(rgrid_batch_refine_scan); }

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
    b->wgmap_off = wgmap_off; b->f2_off = f2_off; b->rrec_off = rrec_off; b->raw_off = raw_off; b->seg_bytes = seg_bytes;
    b->grids.resize((size_t)num_grids);
    b->sub.resize(nS);
    b->pack.resize(raw_off);               // (the raw points go straight into the segment)
    int rc = [&]() -> int {
        G_TRY(b, hipSetDevice(device));
        G_TRY(b, hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        for (int k = 0; k < KGB_SEGMENTS; ++k) {
            b->h_seg[k] = (k == 0 || b->seg_in_vram) ? (unsigned char *)host_visible::alloc(seg_bytes) : nullptr;
            if (b->h_seg[k]) {
                b->seg_in_vram = true;
                b->dv_seg[k] = b->h_seg[k];
            } else {
                if (k > 0 && b->seg_in_vram) { b->hip_error = "host-visible device memory: second segment refused"; return RGRID_ERR_HIP; }
                void *dv = nullptr;
                G_TRY(b, hipHostMalloc((void **)&b->h_seg[k], seg_bytes, hipHostMallocMapped | hipHostMallocCoherent));
                G_TRY(b, hipHostGetDevicePointer(&dv, b->h_seg[k], 0)); b->dv_seg[k] = (const unsigned char *)dv;
            }
        }
        void *dv = nullptr;
        G_TRY(b, hipHostMalloc((void **)&b->h_out, sizeof(BestRec) * nS, hipHostMallocMapped | hipHostMallocCoherent));
        G_TRY(b, hipHostGetDevicePointer(&dv, b->h_out, 0)); b->dv_out = (BestRec *)dv;
        std::memset(b->h_out, 0, sizeof(BestRec) * nS);
        G_TRY(b, hipHostMalloc((void **)&b->h_rout, sizeof(RefineOut) * nS, hipHostMallocMapped | hipHostMallocCoherent));
        G_TRY(b, hipHostGetDevicePointer(&dv, b->h_rout, 0)); b->dv_rout = (RefineOut *)dv;
        std::memset(b->h_rout, 0, sizeof(RefineOut) * nS);
        G_TRY(b, hipMalloc((void **)&b->d_cells, sizeof(unsigned short) * (size_t)num_grids * (size_t)max_cells));
        G_TRY(b, hipMalloc((void **)&b->d_bb, sizeof(unsigned long long) * nS * nR));
        G_TRY(b, hipMalloc((void **)&b->d_arrived, sizeof(int) * nS));
        G_TRY(b, hipMemsetAsync(b->d_arrived, 0, sizeof(int) * nS, b->stream));
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
    (void)hipFree(b->d_cells); (void)hipFree(b->d_bb); (void)hipFree(b->d_arrived);
    for (int k = 0; k < KGB_SEGMENTS; ++k)
        if (b->h_seg[k]) { if (b->seg_in_vram) (void)hipFree(b->h_seg[k]); else (void)hipHostFree(b->h_seg[k]); }
    if (b->h_out) (void)hipHostFree(b->h_out);
    if (b->h_rout) (void)hipHostFree(b->h_rout);
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
    G_TRY(b, hipMemcpyAsync(b->d_cells + (size_t)grid * (size_t)b->max_cells, cells, sizeof(uint16_t) * (size_t)num_x_cells * num_y_cells,
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
    b->sub_count = count;
    if (W.nrec == 0) {
        b->outstanding = true; b->kind = KIND_MATCH;
        b->prepare_seconds = seconds_since(t_begin);
        return RGRID_OK;
    }
    G_TRY(b, hipSetDevice(b->device));
    const int k = (int)(b->n_submit++ % KGB_SEGMENTS);
    stage_match(b, k, W);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);                  // write-combined stores drained before the doorbell
    b->prepare_seconds = seconds_since(t_begin);
    launch_match(b, k, W);
    G_TRY(b, hipGetLastError());
    b->outstanding = true; b->kind = KIND_MATCH;
    return RGRID_OK;
}

int rgrid_batch_match_collect(rgrid_batch_t *b, int *status, double *pose_estimates, double *scores, int *best3, int *info3)
{
    if (!b || !b->outstanding || b->kind != KIND_MATCH) return RGRID_ERR_INVALID;
    const int count = b->sub_count;
    if (count > 0 && (!status || !pose_estimates || !scores)) return RGRID_ERR_INVALID;
    b->outstanding = false;
    G_TRY(b, hipSetDevice(b->device));
    G_TRY(b, hipStreamSynchronize(b->stream));
    for (int j = 0; j < count; ++j) {
        const Pending &P = b->sub[(size_t)j];
        status[j] = P.status;
        pose_estimates[3 * j] = pose_estimates[3 * j + 1] = pose_estimates[3 * j + 2] = 0.;
        scores[j] = 0.;
        if (best3) best3[3 * j] = best3[3 * j + 1] = best3[3 * j + 2] = 0;
        if (info3) info3[3 * j] = info3[3 * j + 1] = info3[3 * j + 2] = 0;
        if (P.status != RGRID_OK) continue;
        decode_best(P.plan, P.pose, b->h_out[P.rec], &pose_estimates[3 * j], &scores[j], best3 ? &best3[3 * j] : nullptr,
                    info3 ? &info3[3 * j] : nullptr);
    }
    return RGRID_OK;
}

int rgrid_batch_refine_submit(rgrid_batch_t *b, const rgrid_refine_options *opt, const rgrid_batch_refine_scan *scans, int count)
{
    if (!b || !opt || count < 0 || count > b->max_scans || (count > 0 && !scans) || b->outstanding || !refine_options_ok(opt)) return RGRID_ERR_INVALID;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_refine_scan &s = scans[j];
        if (s.grid < 0 || s.grid >= b->num_grids || !b->grids[(size_t)s.grid].set || s.n < 0 || (s.n > 0 && !s.points_xy)) return RGRID_ERR_INVALID;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    const int k = (int)(b->n_submit % KGB_SEGMENTS);
    RefineRec *rr = reinterpret_cast<RefineRec *>(b->pack.data() + b->rrec_off);
    float *raw = reinterpret_cast<float *>(b->h_seg[k] + b->raw_off);
    int nrec = 0, nraw = 0, threads = 0;
    for (int j = 0; j < count; ++j) {
        const rgrid_batch_refine_scan &s = scans[j];
        Pending &P = b->sub[(size_t)j];
        std::memset(&P, 0, sizeof(P));
        P.rec = -1;
        if (s.n == 0) { P.status = RGRID_ERR_EMPTY; continue; }
        if (s.n > b->max_points) { P.status = RGRID_ERR_CAPACITY; continue; }
        RefineRec &R = rr[nrec];
        std::memset(&R, 0, sizeof(R));
        refine_args(R.A, b->grids[(size_t)s.grid], opt, s.n);
        R.A.tx = s.target_translation[0]; R.A.ty = s.target_translation[1];
        R.A.x0 = s.initial_pose[0]; R.A.y0 = s.initial_pose[1]; R.A.a0 = s.initial_pose[2];
        R.cells_off = (long long)s.grid * (long long)b->max_cells;
        R.pts_off = nraw; R.match_rec = -1;
        std::memcpy(raw + 2 * (size_t)nraw, s.points_xy, sizeof(float) * 2 * (size_t)s.n);   // forward, straight into the segment
        nraw += s.n;
        if (refine_threads(s.n) > threads) threads = refine_threads(s.n);
        P.status = RGRID_OK; P.rec = nrec;
        ++nrec;
    }
    b->sub_count = count;
    if (nrec == 0) {
        b->outstanding = true; b->kind = KIND_REFINE;
        b->prepare_seconds = seconds_since(t_begin);
        return RGRID_OK;
    }
    G_TRY(b, hipSetDevice(b->device));
    ++b->n_submit;
    std::memcpy(b->h_seg[k] + b->rrec_off, rr, sizeof(RefineRec) * (size_t)nrec);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);                  // write-combined stores drained before the doorbell
    b->prepare_seconds = seconds_since(t_begin);
    launch_refine(b, k, nrec, threads);
    G_TRY(b, hipGetLastError());
    b->outstanding = true; b->kind = KIND_REFINE;
    return RGRID_OK;
}

int rgrid_batch_refine_collect(rgrid_batch_t *b, int *status, double *pose_estimates, rgrid_refine_summary *summaries)
{
    if (!b || !b->outstanding || b->kind != KIND_REFINE) return RGRID_ERR_INVALID;
    const int count = b->sub_count;
    if (count > 0 && (!status || !pose_estimates)) return RGRID_ERR_INVALID;
    b->outstanding = false;
    G_TRY(b, hipSetDevice(b->device));
    G_TRY(b, hipStreamSynchronize(b->stream));
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
    const auto t_begin = std::chrono::steady_clock::now();
    const MatchWork W = pack_match(b, mopt, scans, count);
    b->sub_count = count;
    if (W.nrec == 0) {
        b->outstanding = true; b->kind = KIND_SCAN_MATCH;
        b->prepare_seconds = seconds_since(t_begin);
        return RGRID_OK;
    }
    G_TRY(b, hipSetDevice(b->device));
    const int k = (int)(b->n_submit++ % KGB_SEGMENTS);
    // a refine record per match record, same index: the start pose is the match's winner, decoded on the device
    RefineRec *rr = reinterpret_cast<RefineRec *>(b->pack.data() + b->rrec_off);
    float *raw = reinterpret_cast<float *>(b->h_seg[k] + b->raw_off);
    int nraw = 0, threads = 0;
    for (int j = 0; j < count; ++j) {
        const Pending &P = b->sub[(size_t)j];
        if (P.status != RGRID_OK) continue;
        const rgrid_batch_scan &s = scans[j];
        RefineRec &R = rr[P.rec];
        std::memset(&R, 0, sizeof(R));
        refine_args(R.A, b->grids[(size_t)s.grid], ropt, s.n);
        R.cells_off = (long long)s.grid * (long long)b->max_cells;
        R.plan_res = P.plan.res; R.plan_step = P.plan.step;
        R.ip[0] = s.initial_pose[0]; R.ip[1] = s.initial_pose[1]; R.ip[2] = s.initial_pose[2];
        R.pts_off = nraw; R.match_rec = P.rec; R.num_linear = P.plan.num_linear; R.num_angular = P.plan.num_angular;
        std::memcpy(raw + 2 * (size_t)nraw, s.points_xy, sizeof(float) * 2 * (size_t)s.n);
        nraw += s.n;
        if (refine_threads(s.n) > threads) threads = refine_threads(s.n);
    }
    stage_match(b, k, W);
    std::memcpy(b->h_seg[k] + b->rrec_off, rr, sizeof(RefineRec) * (size_t)W.nrec);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);                  // write-combined stores drained before the doorbell
    b->prepare_seconds = seconds_since(t_begin);
    launch_match(b, k, W);                                    // the stream orders the refinement behind the match: no host wait between them
    launch_refine(b, k, W.nrec, threads);
    G_TRY(b, hipGetLastError());
    b->outstanding = true; b->kind = KIND_SCAN_MATCH;
    return RGRID_OK;
}

int rgrid_batch_scan_match_collect(rgrid_batch_t *b, int *status, double *coarse_poses, double *scores, int *best3, int *info3,
                                   double *pose_estimates, rgrid_refine_summary *summaries)
{
    if (!b || !b->outstanding || b->kind != KIND_SCAN_MATCH) return RGRID_ERR_INVALID;
    const int count = b->sub_count;
    if (count > 0 && (!status || !coarse_poses || !scores || !pose_estimates)) return RGRID_ERR_INVALID;
    b->outstanding = false;
    G_TRY(b, hipSetDevice(b->device));
    G_TRY(b, hipStreamSynchronize(b->stream));
    for (int j = 0; j < count; ++j) {
        const Pending &P = b->sub[(size_t)j];
        status[j] = P.status;
        zero3(&coarse_poses[3 * j]);
        scores[j] = 0.;
        zero3(best3 ? &best3[3 * j] : nullptr);
        zero3(info3 ? &info3[3 * j] : nullptr);
        refine_result(b, P, &pose_estimates[3 * j], summaries ? &summaries[j] : nullptr);
        if (P.status != RGRID_OK) continue;
        decode_best(P.plan, P.pose, b->h_out[P.rec], &coarse_poses[3 * j], &scores[j], best3 ? &best3[3 * j] : nullptr,
                    info3 ? &info3[3 * j] : nullptr);
    }
    return RGRID_OK;
}

}  // extern "C"
