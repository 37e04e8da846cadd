// det2d_batch.hip -- the 2D reflector detector for a fleet: B robots' scans detected by ONE launch (rdet2d_batch_* of include/rdet.h).
//
// Every member of a batch handle is one reflector_detect::LaserReflectorDetect (reference
// src/reflector_detect/laser/laser_reflector_detect.cc:23-316 with the PoseExtrapolator of pose_extrapolator.cc): its own options,
// sensor_to_base_link and odometry.  k_det2d_batch runs ONE workgroup of 1024 threads per scan, and that workgroup does the whole
// of HandleLaserScan for its scan: flags and points, the run state machine, the gates, the first/last-run wrap, the de-skew of
// every valid beam, what every candidate beam adds to its centre, and the ordered float32 sums.  Nothing crosses a workgroup:
// no atomics between workgroups, no counters, nobody waits for anybody -- a batch larger than the chip queues workgroups, and a
// queued workgroup needs nothing from a running one.  (k_det2d of det2d.hip spreads ONE scan over N / 256 + 1 workgroups and lets
// workgroup 0 wait for the others inside the launch; with hundreds of scans in a grid the waiting workgroups could hold the CUs
// their producers need.)
//
// The arithmetic is k_det2d's, restated: the device helpers of det2d.hip live in its anonymous namespace, and that file is pinned
// by the profile manifest.  tests/test_fleet_detect_gpu.py holds the two copies together bit for bit (against the oracle and
// against the single-handle detector); they move into one shared header the next time the detectors are re-profiled.
//
// Per beam the workgroup keeps 15 B in LDS (range, point, last valid beam, flags) plus the run tables: 141 KB at the 8192-beam
// limit.  The contributions to the centres (8 B per beam) go to a per-member slice in device memory that only this workgroup
// touches, ordered by a __syncthreads(); the de-skewed returns go straight to the member's point-cloud buffer, compacted.
//
// Here: the kernels, the handle's buffers, the copies and the launches.  The host's rules that need no HIP call are det_batch_host.h's
// (tested without a GPU), create / destroy / link / collect as both detector handles make them det_batch_dev.h's.
#include "det_batch_dev.h"         // det_batch_host.h: BatchRec, RangeRec and the host's rules

#include <cmath>
#include <cstdio>

namespace host = det_batch_host;
namespace dev = det_batch_dev;

namespace {

using det_batch_host::BatchRec;
using det_batch_host::Odom;
using det_batch_host::RangeRec;

struct R2d { double x, y, a; };
struct R2f { float x, y, a; };

// What a scan hands back, in pinned host memory: plain stores, published by the end of the kernel
struct BatchOut {
    int K, n_returns, err, n_runs;
    float2 centers[RDET_MAX_CENTERS];
};

struct BatchBufs {
    const BatchRec *recs;          // [count]
    const float *stage;            // [B][2][max_beams]: ranges | intensities of member m
    const float *tables;           // [RDET2DB_TABLES + B][3][max_beams]: angle | cos | sin
    unsigned long long *contrib;   // [B][max_beams] float2 bits: the point a beam would add to its cluster's centre
    float2 *returns;               // [B][max_beams]: de-skewed point cloud in point_cloud order (GetRangeData)
    BatchOut *out;                 // [count], pinned host memory
    int max_beams;
};

// the contributions are written and read by the same workgroup, through device memory: write-through / cache-bypassing accesses
__device__ static void publish_u64(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ static unsigned long long fetch_u64(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ static unsigned long long f2_bits(float2 v)
{
    return (unsigned long long)__float_as_uint(v.x) | ((unsigned long long)__float_as_uint(v.y) << 32);
}
__device__ static float2 bits_f2(unsigned long long b)
{
    return make_float2(__uint_as_float((unsigned)b), __uint_as_float((unsigned)(b >> 32)));
}

// ---- Rigid2 algebra (rigid_transform.h:46-51,62-67,87-102), no FMA contraction -------------
__device__ static R2d r2_inverse_cs(double c, double s, R2d r)
{
#pragma clang fp contract(off)
    R2d o;
    o.a = -r.a;
    o.x = -(c * r.x + s * r.y);
    o.y = -((-s) * r.x + c * r.y);
    return o;
}
__device__ static R2d r2_mul_cs(double lc, double ls, R2d l, R2d r)   // l with cos/sin(l.a) given
{
#pragma clang fp contract(off)
    R2d o;
    o.x = (lc * r.x + (-ls) * r.y) + l.x;
    o.y = (ls * r.x + lc * r.y) + l.y;
    o.a = l.a + r.a;
    return o;
}
__device__ static R2f r2_cast(R2d r)
{
    R2f o; o.x = (float)r.x; o.y = (float)r.y; o.a = (float)r.a; return o;
}
#include "glibc_sincosf.h"     // float32 sin / cos with the host libm's bits

__device__ static float2 r2f_apply_cs(float c, float s, float tx, float ty, float px, float py)
{
#pragma clang fp contract(off)
    float2 o;
    o.x = (c * px + (-s) * py) + tx;
    o.y = (s * px + c * py) + ty;
    return o;
}
__device__ static float2 r2f_apply(R2f r, float px, float py)
{
    float s, c;
    glibc_sincosf(r.a, &s, &c);
    return r2f_apply_cs(c, s, r.x, r.y, px, py);
}

// ---- PoseExtrapolator (pose_extrapolator.cc:34-84,102-129): the sample selection and the one straight-line evaluation of
// det2d.hip's extrapolator_pose ----------------------------------------------------------------
__device__ static R2d extrapolator_pose(const BatchRec &A, double time, double *c_out, double *s_out)
{
#pragma clang fp contract(off)
    R2d o = {0, 0, 0};
    *c_out = 1.0; *s_out = 0.0;
    if (A.n_odom == 0) return o;
    // time <= front: the first sample; t >= back, or in between: always the LAST sample (:76-82, Q14)
    const bool uf = time <= A.front.time;
    const double st_time = uf ? A.front.time : A.back.time, px = uf ? A.front.px : A.back.px, py = uf ? A.front.py : A.back.py;
    const double yaw = uf ? A.front.yaw : A.back.yaw, vx = uf ? A.front.vx : A.back.vx, vy = uf ? A.front.vy : A.back.vy;
    const double wz = uf ? A.front.wz : A.back.wz;
    const bool past = st_time <= time;                               // :36-50, else :51-66
    const double delta_t = past ? st_time - time : time - st_time;
    const double now_yaw = yaw - wz * delta_t;                       // sign as in the reference for both (Q14)
    double s, c;
    sincos(now_yaw, &s, &c);
    const double sg = past ? -1.0 : 1.0;
    const double ax = vx * delta_t, ay = vy * delta_t;
    o.x = (px + sg * (ax * c)) - sg * (ay * s);
    o.y = (py + sg * (ax * s)) + sg * (ay * c);
    o.a = now_yaw;
    *c_out = c; *s_out = s;
    return o;
}

// ---- block-wide exclusive scans over 1024 per-thread values: six DPP steps in the wave, the 16 wave totals through an LDS
// slot that each scan of the kernel uses once (one barrier per scan) ----------------------------
struct ScanSum { static constexpr int id = 0; __device__ static int f(int a, int b) { return a + b; } };
struct ScanMax { static constexpr int id = -1; __device__ static int f(int a, int b) { return max(a, b); } };   // values >= -1
template <class Op, int CTRL, int ROW_MASK> __device__ static int dpp_step(int v)
{
    return Op::f(v, __builtin_amdgcn_update_dpp(Op::id, v, CTRL, ROW_MASK, 0xf, false));
}
template <class Op> __device__ static int wave_incl_scan(int v)
{
    v = dpp_step<Op, 0x111, 0xf>(v);        // row_shr:1
    v = dpp_step<Op, 0x112, 0xf>(v);        // row_shr:2
    v = dpp_step<Op, 0x114, 0xf>(v);        // row_shr:4
    v = dpp_step<Op, 0x118, 0xf>(v);        // row_shr:8
    v = dpp_step<Op, 0x142, 0xa>(v);        // row_bcast:15 into rows 1 and 3
    v = dpp_step<Op, 0x143, 0xc>(v);        // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ static int block_excl_sum(int v, int *lds, int *total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int incl = wave_incl_scan<ScanSum>(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { const int c = lds[w]; if (w < wave) base += c; tot += c; }
    if (total) *total = tot;
    return base + incl - v;
}
__device__ static int block_excl_max(int v, int *lds, int *total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int incl = wave_incl_scan<ScanMax>(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int base = -1, tot = -1;
#pragma unroll
    for (int w = 0; w < 16; ++w) { const int c = lds[w]; if (w < wave) base = max(base, c); tot = max(tot, c); }
    if (total) *total = tot;
    const int prev = __builtin_amdgcn_update_dpp(-1, incl, 0x138, 0xf, 0xf, false);   // wave_shr:1: inclusive value of the previous lane
    return max(base, prev);
}

// ================================================================================================
// One workgroup per scan.  s_fl bits: 1 valid, 2 bright (after the "a point exists" guard), 4 bright before it,
// 8 the beam has a contribution in `contrib`, 16 intensity above the gate.
// ================================================================================================
__global__ __launch_bounds__(1024) void k_det2d_batch(BatchBufs B)
{
    __shared__ float s_rg[RDET2DB_MAX_BEAMS];
    __shared__ float2 s_pt[RDET2DB_MAX_BEAMS];          // point in base_link (valid beams)
    __shared__ short s_lv[RDET2DB_MAX_BEAMS];           // last valid beam <= i (point_cloud.back() at beam i), -1 if none
    __shared__ unsigned char s_fl[RDET2DB_MAX_BEAMS];
    __shared__ short s_rf[RDET2DB_MAX_BEAMS / 2 + 4], s_rl[RDET2DB_MAX_BEAMS / 2 + 4];   // first / last beam of run r
    __shared__ int lds_scan[5][16];                     // one slot per block scan (no barrier to recycle it)
    __shared__ int s_tot[4];
    __shared__ int s_cl[4 * RDET_MAX_CENTERS + 8];      // cluster segments: first0,last0,first1,last1
    __shared__ double s_inv[5];                         // inverse of the scan-end pose, cos / sin of its angle
    __shared__ float s_tb[4];                           // the same as Rigid2f with cos / sin

    __shared__ BatchRec s_rec;                          // this scan's record (it lies in host memory: fetched once)

    BatchOut *const out = B.out + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    static_assert(sizeof(BatchRec) % 4 == 0 && sizeof(BatchRec) / 4 <= 1024, "the record is copied one word per thread");
    if (tid < (int)(sizeof(BatchRec) / 4)) ((unsigned *)&s_rec)[tid] = ((const unsigned *)(B.recs + blockIdx.x))[tid];
    __syncthreads();
    const BatchRec &A = s_rec;
    const int N = A.N;
    if (!A.run || N <= 0 || N > RDET2DB_MAX_BEAMS || N > B.max_beams) {      // (the host refuses such N: a bound, not a path)
        if (tid == 0) { out->K = 0; out->n_returns = 0; out->err = 0; out->n_runs = 0; }
        return;
    }
    const size_t mb = (size_t)B.max_beams;
    const float *const ranges = B.stage + (size_t)A.member * 2 * mb, *const intens = ranges + mb;
    const float *const ang = B.tables + (size_t)A.table * 3 * mb, *const cosv = ang + mb, *const sinv = cosv + mb;
    unsigned long long *const contrib = B.contrib + (size_t)A.member * mb;
    float2 *const returns = B.returns + (size_t)A.member * mb;

    const int CH = (N + 1023) / 1024;
    const int b0 = tid * CH, b1 = min(N, b0 + CH);
    constexpr int MAXCH = RDET2DB_MAX_BEAMS / 1024;

    // ---- pass 1: points, validity, brightness (:63-83), beam i = tid + 1024 q so that a wave reads whole lines
    {
        float rr[MAXCH], ii[MAXCH], cc[MAXCH], ss[MAXCH];
#pragma unroll
        for (int q = 0; q < MAXCH; ++q) {
            const int i = tid + 1024 * q;
            const bool in = i < N;
            rr[q] = in ? ranges[i] : 0.f; ii[q] = in ? intens[i] : 0.f; cc[q] = in ? cosv[i] : 0.f; ss[q] = in ? sinv[i] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < MAXCH; ++q) {
#pragma clang fp contract(off)
            const int i = tid + 1024 * q;
            if (i >= N) continue;
            const float range = rr[q];
            unsigned char f = 0;
            s_rg[i] = range;
            if (range >= A.msg_range_min && range <= A.msg_range_max) {
                f |= 1;
                s_pt[i] = r2f_apply_cs(A.s2b_c, A.s2b_s, A.s2b_x, A.s2b_y, range * cc[q], range * ss[q]);
            }
            if ((double)ii[q] > A.intensity_min) {
                f |= 16;
                if (A.opt_range_min <= range && range <= A.opt_range_max) f |= 4;
            }
            s_fl[i] = f;
        }
    }
    __syncthreads();
    // from here a thread owns CH <= 8 consecutive beams
    unsigned char fl[MAXCH];
    int prevb_r[MAXCH];
    int cnt_valid = 0, last_valid = -1;
#pragma unroll
    for (int q = 0; q < MAXCH; ++q) {
        const int i = b0 + q;
        fl[q] = 0;
        if (q >= CH || i >= b1) continue;
        fl[q] = s_fl[i];
        if (fl[q] & 1) { ++cnt_valid; last_valid = i; }
    }
    int n_cloud, last_valid_all;
    const int cloud_base = block_excl_sum(cnt_valid, lds_scan[0], &n_cloud);
    int lv = block_excl_max(last_valid, lds_scan[1], &last_valid_all);
    // ---- pass 2: point_cloud.back(), guarded bright flag, previous bright beam
    int last_bright = -1;
#pragma unroll
    for (int q = 0; q < MAXCH; ++q) {
        const int i = b0 + q;
        if (q >= CH || i >= b1) continue;
        unsigned char f = fl[q];
        if (f & 1) lv = i;
        s_lv[i] = (short)lv;
        if ((f & 4) && lv >= 0) { f |= 2; last_bright = i; s_fl[i] = f; }      // (bit 2 to LDS: the per-beam pass looks three beams ahead)
        fl[q] = f;
    }
    int last_bright_all;
    int pb = block_excl_max(last_bright, lds_scan[2], &last_bright_all);
    // ---- pass 3: run starts (:85-169) and run index
    int n_start = 0;
    unsigned start_mask = 0;
#pragma unroll
    for (int q = 0; q < MAXCH; ++q) {
        const int i = b0 + q;
        prevb_r[q] = -1;
        if (q >= CH || i >= b1 || !(fl[q] & 2)) continue;
        prevb_r[q] = pb;
        bool start = pb < 0;
        if (!start && i - pb != 1) {
            const int nx = (i + 1 < N) ? i + 1 : i;
            const bool gap = (i - pb < 4) && (fabs((double)(s_rg[i] - s_rg[pb])) < 0.3) && (s_fl[nx] & 16);   // :111
            start = !gap;
        }
        if (start) start_mask |= 1u << q;
        n_start += start ? 1 : 0;
        pb = i;
    }
    int n_runs;
    int rid = block_excl_sum(n_start, lds_scan[3], &n_runs);
#pragma unroll
    for (int q = 0; q < MAXCH; ++q) {
        const int i = b0 + q;
        if (q >= CH || i >= b1 || !(fl[q] & 2)) continue;
        if (start_mask & (1u << q)) {      // start of run `rid`
            s_rf[rid] = (short)i;
            if (prevb_r[q] >= 0) s_rl[rid - 1] = (short)prevb_r[q];
            ++rid;
        }
    }
    if (tid == 0 && n_runs > 0) s_rl[n_runs - 1] = (short)last_bright_all;
    __syncthreads();

    // ---- gate the closed runs (:147-156), compact the accepted ones
    const int n_closed = (n_runs > 0) ? n_runs - 1 : 0;
    const int RCH = (n_closed + 1023) / 1024;
    const int r0 = tid * RCH, r1 = min(n_closed, r0 + RCH);
    int n_acc_local = 0;
    unsigned acc_mask = 0;
    for (int r = r0; r < r1; ++r) {
#pragma clang fp contract(off)
        const int fi = s_rf[r], li = s_rl[r];
        const float2 pf = s_pt[s_lv[fi]], pl = s_pt[s_lv[li]];
        const float len = hypotf(pf.x - pl.x, pf.y - pl.y);
        const bool ok = (A.is_circle && fi == 0) || (fabs((double)len - A.min_length) < A.length_error);
        if (ok) { acc_mask |= 1u << (r - r0); ++n_acc_local; }
    }
    int n_acc;
    int cidx = block_excl_sum(n_acc_local, lds_scan[4], &n_acc);
    for (int r = r0; r < r1; ++r) {
        if (!(acc_mask & (1u << (r - r0)))) continue;
        if (cidx < RDET_MAX_CENTERS) {
            s_cl[4 * cidx + 0] = s_rf[r]; s_cl[4 * cidx + 1] = s_rl[r];
            s_cl[4 * cidx + 2] = -1; s_cl[4 * cidx + 3] = -1;
        }
        ++cidx;
    }
    __syncthreads();

    // ---- last / first reflector (:178-236), one lane; meanwhile wave 1 takes the scan-end pose (:252-253, :299) and its inverse
    if (tid == 0) {
#pragma clang fp contract(off)
        int n_cl = n_acc, off = 0, err = 0;
        if (n_acc > RDET_MAX_CENTERS) { err = RDET_ERR_CAPACITY; n_cl = RDET_MAX_CENTERS; }
        if (n_runs > 0 && !err) {
            const int Lr = n_runs - 1;
            const int lf = s_rf[Lr], ll = s_rl[Lr];
            const float2 last_first_pt = s_pt[s_lv[lf]], last_pt = s_pt[s_lv[ll]];
            const float len = hypotf(last_first_pt.x - last_pt.x, last_first_pt.y - last_pt.y);
            const bool len_ok = fabs((double)len - A.min_length) < A.length_error;
            if (n_cl > 0) {
                const int first_id = s_cl[0];
                const float2 first_pt = s_pt[s_lv[s_cl[0]]];
                const float2 first_last_pt = s_pt[s_lv[s_cl[1]]];
                const float dx = last_pt.x - first_pt.x, dy = last_pt.y - first_pt.y;
                if (A.is_circle && first_id == 0 && ll == N - 1 && sqrtf(dx * dx + dy * dy) < 0.1) {   // :188-195
                    s_cl[2] = lf; s_cl[3] = ll;
                } else if (len_ok) {                                                                   // :196-204
                    if (n_cl < RDET_MAX_CENTERS) {
                        s_cl[4 * n_cl + 0] = lf; s_cl[4 * n_cl + 1] = ll; s_cl[4 * n_cl + 2] = -1; s_cl[4 * n_cl + 3] = -1;
                        ++n_cl;
                    } else err = RDET_ERR_CAPACITY;
                }
                if (A.is_circle && ll == 0) {                                                          // :205-214
                    const float fx = first_last_pt.x - last_first_pt.x, fy = first_last_pt.y - last_first_pt.y;
                    if (fabs((double)sqrtf(fx * fx + fy * fy) - A.min_length) >= A.length_error) off = 1;
                }
            } else if (len_ok) {                                                                        // :216-224
                s_cl[0] = lf; s_cl[1] = ll; s_cl[2] = -1; s_cl[3] = -1;
                n_cl = 1;
            }
        }
        // (no bright beam at all: the reference touches an empty deque, :226 -- defined as no reflectors)
        int K = n_cl - off;
        if (K < 0) K = 0;
        if (n_cloud == 0) K = 0;
        s_tot[0] = K; s_tot[1] = off; s_tot[2] = err;
    }
    if (wave == 1 && last_valid_all >= 0) {
        double c, s;
        const R2d mtp = extrapolator_pose(A, (double)(float)(A.first_point_time + last_valid_all * A.point_delta_t), &c, &s);
        const R2d inv = r2_inverse_cs(c, s, mtp);
        const R2f tb = r2_cast(inv);
        float tc, ts;
        glibc_sincosf(tb.a, &ts, &tc);
        if (lane == 0) {
            s_inv[0] = inv.x; s_inv[1] = inv.y; s_inv[2] = inv.a; s_inv[3] = c; s_inv[4] = -s;
            s_tb[0] = tb.x; s_tb[1] = tb.y; s_tb[2] = tc; s_tb[3] = ts;
        }
    }
    __syncthreads();
    const int K = s_tot[0], off = s_tot[1];

    // ---- per beam: the de-skewed return of every valid beam (:246-258), compacted into point_cloud order, and, for every beam
    // that COULD belong to a cluster (a bright beam, or a finite beam with a bright beam at most three ahead -- the only beams a
    // bridged gap can hold, :111), the point it would add to its cluster's centre (:277-299).  All of the FP64 trigonometry.
    if (last_valid_all >= 0) {
        int c = cloud_base;
#pragma unroll 1
        for (int i = b0; i < b1; ++i) {
            const unsigned char f = s_fl[i];
            const bool valid = f & 1, bright = f & 2;
            const float rgj = s_rg[i];
            // a gap beam (:115-130) is re-projected from the NEXT bright beam's accumulated angle
            int ahead = 0;
            if (!bright && !isinf(rgj)) {
#pragma unroll
                for (int d = 3; d >= 1; --d)
                    if (i + d < N && (s_fl[i + d] & 2)) ahead = d;
            }
            if (!valid && !bright && !ahead) continue;
            const float tj = (float)(A.first_point_time + i * A.point_delta_t);             // :66 (stored in a Vector3f)
            double pc, ps;
            const R2d pose_j = extrapolator_pose(A, (double)tj, &pc, &ps);
            const float2 pt_j = valid ? s_pt[i] : make_float2(0.f, 0.f);
            if (valid) {                                                                    // de-skew (:246-258)
                const R2d inv = {s_inv[0], s_inv[1], s_inv[2]};
                const R2f rel = r2_cast(r2_mul_cs(s_inv[3], s_inv[4], inv, pose_j));
                returns[c++] = r2f_apply(rel, pt_j.x, pt_j.y);
            }
            float2 p = pt_j;
            R2d pose_p = pose_j;
            bool has = false;
            if (bright) {
                has = true;
                if (!valid) {                   // bright beyond the message's own range limits: point_cloud.back() (:87)
                    const int lvb = s_lv[i];
                    p = s_pt[lvb];
                    double c2, s2;
                    pose_p = extrapolator_pose(A, (double)(float)(A.first_point_time + lvb * A.point_delta_t), &c2, &s2);
                }
            } else if (ahead) {
#pragma clang fp contract(off)
                has = true;
                const float a_next = ang[i + ahead];
                const float angle_gap = a_next - A.angle_increment * (float)ahead;          // :117
                float gs, gc;
                glibc_sincosf(angle_gap, &gs, &gc);
                p = r2f_apply_cs(A.s2b_c, A.s2b_s, A.s2b_x, A.s2b_y, rgj * gc, rgj * gs);
            }
            if (has) {
                const R2f pose = r2_cast(pose_p);                                           // :287,:293
                const float2 po = r2f_apply(pose, p.x, p.y);
                publish_u64(contrib + i, f2_bits(r2f_apply_cs(s_tb[2], s_tb[3], s_tb[0], s_tb[1], po.x, po.y)));
                s_fl[i] = f | 8;
            }
        }
    }
    __syncthreads();      // (waits for this workgroup's stores: the contributions are in device memory)

    // ---- per cluster: the float32 running sum in beam order that the reference takes (:300-305), one wave per cluster
    {
#pragma clang fp contract(off)
        for (int c = wave; c < K; c += 16) {
            const int k = c + off;
            float cx = 0.f, cy = 0.f;
            int count = 0;
            for (int seg = 0; seg < 2; ++seg) {
                const int fi = s_cl[4 * k + 2 * seg], li = s_cl[4 * k + 2 * seg + 1];
                if (fi < 0) continue;
                for (int j0 = fi; j0 <= li; j0 += 64) {
                    const int j = min(j0 + lane, N - 1);
                    const bool mem = j0 + lane <= li && (s_fl[j] & 8);
                    const float2 v = mem ? bits_f2(fetch_u64(contrib + j)) : make_float2(0.f, 0.f);
                    unsigned long long mask = __ballot(mem);
                    count += __popcll(mask);
                    while (mask) {                      // (the ballot is wave-uniform: scalar loop, v_readlane)
                        const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
                        mask &= mask - 1;
                        cx += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), b));
                        cy += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), b));
                    }
                }
            }
            if (lane == 0) out->centers[c] = make_float2(cx / (float)count, cy / (float)count);   // :305
        }
    }
    if (tid == 0) { out->K = K; out->n_returns = n_cloud; out->err = s_tot[2]; out->n_runs = n_runs; }
}

// ================================================================================================
// GetRangeData of any list of members in ONE launch (rdet2d_batch_get_range_data_all): k_det2d_batch left member m's de-skewed
// returns at returns[m * max_beams ...]; this kernel copies the rows of the listed members, one member's behind the other's, into
// pinned host memory, which the end of the launch publishes.  The host knows every count (collect stored last_n_returns), so it
// builds the records and a workgroup table (record, tile) as kgb_to_local's callers do: a workgroup is a tile of one member's rows,
// no workgroup waits for another, there is no atomic and nothing to clear.
//
// A lane moves two points, 16 bytes.  The destination of a record is 16-byte aligned only when the counts in front of it sum to an
// even number, so a record's pairs are laid on the DESTINATION's 16-byte grid: with lead = dst_off & 1, lane p of the record holds
// the slots j = 2p and 2p + 1 of row i = j - lead; the one row in front of the first boundary and the one behind the last go as
// 8-byte stores, every pair between them as one 16-byte store.  The load of a pair is one 16-byte load when the source is on the
// same grid ((src_off + i) even), else two 8-byte loads: uniform over the record.  A member with n rows costs
// ceil((n + lead) / RDET2DB_RANGE_TILE) workgroups, an empty one none.
struct RangeBufs {
    const RangeRec *recs;          // [records], pinned host memory
    const int2 *wgmap;             // (record, tile) per workgroup, pinned host memory
    const float2 *returns;         // k_det2d_batch's [B][max_beams]
    float2 *out;                   // pinned host memory, [B * max_beams]
};

__global__ __launch_bounds__(RDET2DB_RANGE_THREADS) void k_det2d_batch_range_data(RangeBufs B)
{
    const int2 wg = B.wgmap[blockIdx.x];
    const RangeRec R = B.recs[wg.x];
    const int lead = (int)(R.dst_off & 1);
    const int j0 = wg.y * RDET2DB_RANGE_TILE + 2 * (int)threadIdx.x, end = R.n + lead;      // slots [lead, end) hold rows
    if (j0 >= end) return;
    const int i0 = j0 - lead;                                                               // (-1 for the slot in front of the first row)
    const float2 *__restrict__ src = B.returns + R.src_off;
    float2 *__restrict__ dst = B.out + R.dst_off;
    const bool lo = j0 >= lead, hi = j0 + 1 < end;
    if (lo && hi) {
        float4 v;
        if (((R.src_off + i0) & 1) == 0) v = *reinterpret_cast<const float4 *>(src + i0);
        else { const float2 a = src[i0], b = src[i0 + 1]; v = make_float4(a.x, a.y, b.x, b.y); }
        *reinterpret_cast<float4 *>(dst + i0) = v;                                          // (dst_off + i0 = dst_off - lead + j0: even)
    } else if (lo) dst[i0] = src[i0];
    else if (hi) dst[i0 + 1] = src[i0 + 1];
}

}  // namespace

// =================================================================================================
// The handle
struct rdet2d_batch : dev::Handle {
    int max_beams = 0;
    std::vector<host::Member2d> m;
    // the staging area the host writes and the kernel reads in place: fine-grained DEVICE memory through the PCIe BAR where
    // the platform maps it, else pinned host memory (host_visible.h)
    batch_host::Staging<float> stage;  // [B][2][max_beams]
    batch_host::Pinned<BatchRec> recs; // [B]
    batch_host::Pinned<BatchOut> out;  // [B]
    batch_host::Host<float> h_tables;  // pinned image of d_tables
    batch_host::Device<float> d_tables;   // [RDET2DB_TABLES + B][3][max_beams]: the cached tables, then one per member for a call with more lidars than those
    batch_host::Device<unsigned long long> d_contrib;
    batch_host::Device<float2> d_returns;
    host::TableCache tables;
    std::vector<host::TableUse> use;   // [B]: the tables of the call being submitted
    // rdet2d_batch_get_range_data_all, allocated by its first call that launches: the rows of a call, and its records with the
    // workgroup table behind them
    batch_host::Pinned<float2> rd_out;           // [B][max_beams]
    batch_host::Pinned<unsigned char> rd_tab;    // RangeRec[B] | RangeTile[B * range_tiles]
};

namespace {

// ---- 4 of submit: every scan that runs into its member's staging slice, unless it was received there; the tables plan_tables
// wants filled into the pinned image and from there to the device, on the stream
int submit_stage(rdet2d_batch *b, const rdet2d_scan *scans, int count)
{
    const size_t mb = (size_t)b->max_beams;
    for (int i = 0; i < count; ++i) {
        if (!b->sub_runs[(size_t)i]) continue;
        const rdet2d_scan &s = scans[i];
        float *sr = b->stage.h + (size_t)s.member * 2 * mb, *si = sr + mb;
        if (s.ranges != sr) std::memcpy(sr, s.ranges, sizeof(float) * (size_t)s.N);
        if (s.intensities != si) std::memcpy(si, s.intensities, sizeof(float) * (size_t)s.N);
        if (!b->use[(size_t)i].fill) continue;
        const size_t at = (size_t)b->use[(size_t)i].table * 3 * mb;
        host::fill_angle_table(b->h_tables.h + at, mb, s.angle_min, s.angle_increment, s.N);
        for (size_t part = 0; part < 3; ++part)
            DETB_TRY(b, hipMemcpyAsync(b->d_tables.d + at + part * mb, b->h_tables.h + at + part * mb, sizeof(float) * (size_t)s.N,
                                       hipMemcpyHostToDevice, b->stream));
    }
    return RDET_OK;
}

// ---- 5 of submit: one workgroup per scan of the call (a scan that does not run clears its record), and the submit is outstanding
int submit_launch(rdet2d_batch *b, int count, int n_run, bool linked)
{
    b->outstanding = true;
    if (n_run > 0) {
        __atomic_thread_fence(__ATOMIC_SEQ_CST);              // write-combined stores drained before the doorbell
        BatchBufs Bf;
        Bf.recs = b->recs.dv; Bf.stage = b->stage.dv; Bf.tables = b->d_tables.d; Bf.contrib = b->d_contrib.d;
        Bf.returns = b->d_returns.d; Bf.out = b->out.dv; Bf.max_beams = b->max_beams;
        hipLaunchKernelGGL(k_det2d_batch, dim3((unsigned)count), dim3(1024), 0, b->stream, Bf);
        DETB_TRY(b, hipGetLastError());
    } else if (!linked) {
        for (int i = 0; i < count; ++i) std::memset(&b->out.h[i], 0, 4 * sizeof(int));
    }
    return RDET_OK;
}

}  // namespace

extern "C" {

int rdet2d_batch_sizeof_scan(void) { return (int)sizeof(rdet2d_scan); }

const char *rdet2d_batch_last_hip_error(rdet2d_batch_t *b) { return b ? b->hip_error.c_str() : ""; }

int rdet2d_batch_create(const rdet2d_options *opts, const double *s2b_xyyaw, int B, int max_beams, int device, rdet2d_batch_t **out)
{
    if (!opts || !s2b_xyyaw || !out || B < 1 || max_beams < 1) return RDET_ERR_INVALID;
    *out = nullptr;
    rdet2d_batch_t *b = dev::make<rdet2d_batch>(opts, s2b_xyyaw, B, device);
    if (!b) return RDET_ERR_INVALID;
    b->max_beams = max_beams;
    b->use.reserve((size_t)B);
    const size_t nb = (size_t)max_beams, nB = (size_t)B;
    int rc = [&]() -> int {
        DETB_TRY(b, hipSetDevice(device));
        DETB_TRY(b, hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        DETB_TRY(b, b->stage.alloc(nb * 2 * nB));
        DETB_TRY(b, b->recs.alloc(nB));
        DETB_TRY(b, b->out.alloc(nB));
        std::memset(b->out.h, 0, sizeof(BatchOut) * nB);
        DETB_TRY(b, b->h_tables.alloc(nb * 3 * (RDET2DB_TABLES + nB)));
        DETB_TRY(b, b->d_tables.alloc(nb * 3 * (RDET2DB_TABLES + nB)));
        DETB_TRY(b, b->d_contrib.alloc(nb * nB));
        DETB_TRY(b, b->d_returns.alloc(nb * nB));
        return RDET_OK;
    }();
    if (rc != RDET_OK) { std::fprintf(stderr, "rdet2d_batch_create: %s\n", b->hip_error.c_str()); rdet2d_batch_destroy(b); return rc; }
    *out = b;
    return RDET_OK;
}

void rdet2d_batch_destroy(rdet2d_batch_t *b)
{
    if (!b) return;
    dev::destroy(b, b->d_tables, b->d_contrib, b->d_returns, b->h_tables, b->stage, b->recs, b->out, b->rd_out, b->rd_tab);
    delete b;
}

int rdet2d_batch_set_sensor_to_base_link(rdet2d_batch_t *b, int member, const double xyyaw[3]) { return dev::set_sensor_to_base_link(b, member, xyyaw); }

int rdet2d_batch_handle_odometry(rdet2d_batch_t *b, int member, double t, const double pos_xy[2], const double quat_zw[2],
                                 double vx, double vy, double wz)
{
    if (!b || !pos_xy || !quat_zw || member < 0 || member >= b->B) return RDET_ERR_INVALID;
    b->m[(size_t)member].odom.push_back(Odom{t, pos_xy[0], pos_xy[1], 2 * std::atan2(quat_zw[0], quat_zw[1]), vx, vy, wz});   // pose_extrapolator.cc:28-32, yaw :36
    return RDET_OK;
}

int rdet2d_batch_staging(rdet2d_batch_t *b, int member, float **ranges, float **intensities)
{
    if (!b || !ranges || !intensities || member < 0 || member >= b->B) return RDET_ERR_INVALID;
    *ranges = b->stage.h + (size_t)member * 2 * (size_t)b->max_beams;
    *intensities = *ranges + b->max_beams;
    return RDET_OK;
}

int rdet2d_batch_submit(rdet2d_batch_t *b, const rdet2d_scan *scans, int count)
{
    if (!b || count < 0 || (count > 0 && !scans) || b->outstanding) return RDET_ERR_INVALID;
    int rc = host::validate_scans(scans, count, b->B, b->max_beams, b->seen);           // 1
    bool linked = false;
    if (rc == RDET_OK) rc = dev::begin_submit(b, &linked);
    if (rc != RDET_OK) return rc;
    host::plan_tables(b->tables, scans, count, b->use);                                 // 2
    const int n_run = host::pack_scans(scans, count, b->m, b->use, *b, b->recs.h);      // 3
    rc = submit_stage(b, scans, count);                                                 // 4
    if (rc != RDET_OK) { b->tables = host::TableCache(); return rc; }                   // (a table planned and not uploaded)
    return submit_launch(b, count, n_run, linked);                                      // 5
}

int rdet2d_batch_link(rdet2d_batch_t *b, rlink *out) { return b ? dev::link(b, b->out.dv, out) : RDET_ERR_INVALID; }

int rdet2d_batch_collect(rdet2d_batch_t *b, int *status, int *K, float *centers_xy, int max_centers, double *obs_time)
{
    if (!b) return RDET_ERR_INVALID;
    return dev::collect(b, b->out.h, status, K, centers_xy, max_centers, obs_time, [&](int i, const BatchOut *o) {
        if (o) b->m[(size_t)b->sub_member[(size_t)i]].last_n_returns = o->n_returns;
    });
}

int rdet2d_batch_get_range_data(rdet2d_batch_t *b, int member, float origin_xy[2], float *returns_xy, int cap_points, int *n_returns)
{
    if (!b || !n_returns || member < 0 || member >= b->B || b->outstanding) return RDET_ERR_INVALID;
    const host::Member2d &M = b->m[(size_t)member];
    if (origin_xy) { origin_xy[0] = (float)M.s2b[0]; origin_xy[1] = (float)M.s2b[1]; }   // :243
    *n_returns = M.last_n_returns;
    if (returns_xy) {
        if (cap_points < M.last_n_returns) return RDET_ERR_BUFFER;
        if (M.last_n_returns > 0) {
            DETB_TRY(b, hipSetDevice(b->device));
            DETB_TRY(b, hipStreamSynchronize(b->stream));
            DETB_TRY(b, hipMemcpy(returns_xy, b->d_returns.d + (size_t)member * (size_t)b->max_beams,
                                  sizeof(float) * 2 * (size_t)M.last_n_returns, hipMemcpyDeviceToHost));
        }
    }
    return RDET_OK;
}

int rdet2d_batch_get_range_data_all(rdet2d_batch_t *b, const int *members, int count, int *counts, float *origins_xy, float *returns_xy,
                                    long cap_points)
{
    if (!b || count < 0 || (count > 0 && !counts) || cap_points < 0 || b->outstanding) return RDET_ERR_INVALID;
    if (!host::members_named_once(members, count, b->B, b->seen)) return RDET_ERR_INVALID;
    if (count == 0) return RDET_OK;
    const long total = host::range_counts(members, count, b->max_beams, b->m, counts);
    if (returns_xy && cap_points < total) return RDET_ERR_BUFFER;
    if (origins_xy)
        for (int g = 0; g < count; ++g) {
            const host::Member2d &M = b->m[(size_t)(members ? members[g] : g)];
            origins_xy[2 * g] = (float)M.s2b[0]; origins_xy[2 * g + 1] = (float)M.s2b[1];   // :243
        }
    if (!returns_xy || total == 0) return RDET_OK;
    DETB_TRY(b, hipSetDevice(b->device));
    const size_t wgmap_off = host::range_table_off(b->B);
    if (!b->rd_out.h) DETB_TRY(b, b->rd_out.alloc((size_t)b->max_beams * (size_t)b->B));
    if (!b->rd_tab.h) DETB_TRY(b, b->rd_tab.alloc(wgmap_off + sizeof(int2) * host::range_tiles(b->max_beams) * (size_t)b->B));
    static_assert(sizeof(host::RangeTile) == sizeof(int2), "the kernel reads a workgroup's (record, tile) as an int2");
    const int nwg = host::range_data_plan(members, counts, count, b->max_beams, reinterpret_cast<RangeRec *>(b->rd_tab.h),
                                          reinterpret_cast<host::RangeTile *>(b->rd_tab.h + wgmap_off));
    __atomic_thread_fence(__ATOMIC_SEQ_CST);                  // the records and the table are written before the doorbell
    RangeBufs Rf;
    Rf.recs = reinterpret_cast<const RangeRec *>(b->rd_tab.dv);
    Rf.wgmap = reinterpret_cast<const int2 *>(b->rd_tab.dv + wgmap_off);
    Rf.returns = b->d_returns.d; Rf.out = b->rd_out.dv;
    hipLaunchKernelGGL(k_det2d_batch_range_data, dim3((unsigned)nwg), dim3(RDET2DB_RANGE_THREADS), 0, b->stream, Rf);
    DETB_TRY(b, hipGetLastError());
    DETB_TRY(b, hipStreamSynchronize(b->stream));
    std::memcpy(returns_xy, b->rd_out.h, sizeof(float2) * (size_t)total);
    return RDET_OK;
}

}  // extern "C"
