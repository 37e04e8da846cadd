// rgrid_refine_dev.h -- the device text of CeresScanMatcher2D::Match that its two kernels share: kg_refine of rgrid.hip (one
// handle, one scan, one workgroup) and kgb_refine of rgrid_batch.hip (one scan of many robots, one workgroup each, one launch).
//
// ONE text: the per-point arithmetic (value_to_cost, hermite, wave_sum_f64, the evaluation loop), the first wave's totals and
// thread 0's trust-region logic (refine_next_candidate, refine_judge, chol3) with the records they work on.  The kernels differ
// only in where RefineArgs, the cells and the points come from, and in the thread count that shares a scan's points: kg_refine's
// workgroup IS min(1024, roundup64(n)) threads, kgb_refine's workgroup may be larger than its own scan's count and sums with the
// scan's.  Moving the text here left kg_refine's instructions as they were; refine_begin is the one exception,
// by measurement: kg_refine keeps thread 0's first block written out (calling it through refine_begin reordered operands in
// kg_refine), and refine_begin restates that block for kgb_refine.  tests/test_fleet_refine_gpu.py holds the two together bit
// for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace {

struct RefineArgs {
    int nx, ny, n, max_iter, max_nonmono;
    double res, max_x, max_y, w_occ, w_t, w_r, tx, ty, x0, y0, a0;
};
struct RefineOut {
    double pose[3]; double initial_cost, final_cost; int iterations, termination;
#ifdef RGRID_DEBUG_TIMING
    long long dbg[16];                                 // cycles per phase, summed over the iterations (thread 0)
#endif
};
#ifdef RGRID_DEBUG_TIMING
__device__ static inline long long pinned_clock() { __builtin_amdgcn_sched_barrier(0); const long long t = clock64(); __builtin_amdgcn_sched_barrier(0); return t; }
#define RT_MARK(k) do { if (threadIdx.x == 0) { const long long t_ = pinned_clock(); dbg[k] += t_ - tprev; tprev = t_; } } while (0)
#else
#define RT_MARK(k) do { } while (0)
#endif
struct RefineState {
    double x[3], xc[3], g[3], H[6], s[3], best[3];
    double x_cost, x_norm, gmax, radius, decrease, mcc, min_cost, initial_cost;
    double ev_min, ev_cur, ev_ref, ev_cand, acc_ref, acc_cand;              // TrustRegionStepEvaluator
    int nonmono, invalid, iter, termination, successful, done;
};
constexpr double REFINE_PAD = 536870911.0;                                      // kPadding = INT_MAX / 4 (occupied_space_cost_function_2d.cc:57)

__device__ static inline float value_to_cost(unsigned v16)
{
#pragma clang fp contract(off)
    const float kMinProbability = 0.1f, kMaxProbability = 1.f - kMinProbability;
    const float lower = 1.f - kMaxProbability, upper = 1.f - kMinProbability;
    const unsigned v = v16 & 32767u;
    const float kScale = (upper - lower) / (32768 - 2.f);
    const float c = (float)v * kScale + (lower - kScale);
    return v == 0 ? upper : c;
}
__device__ static inline void hermite(double p0, double p1, double p2, double p3, double x, double &f, double &dfdx)
{
#pragma clang fp contract(off)
    const double a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3);                    // ceres::CubicHermiteSpline
    const double b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3);
    const double c = 0.5 * (-p0 + p2);
    f = p1 + x * (c + x * (b + x * a));
    dfdx = c + x * (2.0 * b + 3.0 * a * x);
}
// All-lanes sum of a double over the wave without touching LDS: DPP inside rows of 16 (quad permutes, half-row and row
// mirror), then gfx950's v_permlane16_swap / v_permlane32_swap across the rows (each returns both halves of the exchange,
// so one instruction pair per step serves the low and the high dword).  Six steps, no ds_bpermute, no waitcnt.
template <int CTRL>
__device__ static inline double mov_dpp_f64(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ static inline double wave_sum_f64(double v)
{
    v += mov_dpp_f64<0xB1>(v);                          // quad_perm [1,0,3,2]: lane ^ 1
    v += mov_dpp_f64<0x4E>(v);                          // quad_perm [2,3,0,1]: lane ^ 2
    v += mov_dpp_f64<0x141>(v);                         // row_half_mirror: the other quad of the half row
    v += mov_dpp_f64<0x140>(v);                         // row_mirror: the other half row
    {
        auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(v), (unsigned)__double2loint(v), false, false);
        auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(v), (unsigned)__double2hiint(v), false, false);
        v = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);      // rows 0+1, 2+3
    }
    {
        auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(v), (unsigned)__double2loint(v), false, false);
        auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(v), (unsigned)__double2hiint(v), false, false);
        v = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);      // both halves of the wave
    }
    return v;
}

// Partial sums of this wave into part[wave][]: [0] = |r|^2, [1..3] = J'r, [4..9] = J'J (xx xy xt yy yt tt)
#ifdef RGRID_DEBUG_TIMING
__shared__ long long edbg[8];
#define ET_MARK(k) do { if (threadIdx.x == 0) { const long long t_ = pinned_clock(); edbg[k] += t_ - et; et = t_; } } while (0)
#else
#define ET_MARK(k) do { } while (0)
#endif
// `stride` = the threads that share the scan's points: the workgroup's size in kg_refine, the scan's own thread count in kgb_refine
__device__ static inline void refine_eval_strided(const RefineArgs &A, const unsigned short *__restrict__ cells, const float *__restrict__ pts,
                                                  const double p0, const double p1, const double p2, double (*part)[10], const unsigned stride)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef RGRID_DEBUG_TIMING
    long long et = pinned_clock();
#endif
    double sn, cs;
    sincos(p2, &sn, &cs);
    ET_MARK(0);
    const double scale = A.w_occ / sqrt((double)A.n);
    const double ninv = -1.0 / A.res;                                            // d(row) / d(world x): Jet / scalar = * (1 / scalar)
    double acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.;
    for (int i = tid; i < A.n; i += stride) {
        const float2 pt = reinterpret_cast<const float2 *>(pts)[i];
        const double px = (double)pt.x, py = (double)pt.y;
        const double wx = cs * px - sn * py + p0, wy = sn * px + cs * py + p1;
        const double dwx = -sn * px - cs * py, dwy = cs * px - sn * py;          // d world / d angle
        const double r = (A.max_x - wx) / A.res - 0.5 + REFINE_PAD, q = (A.max_y - wy) / A.res - 0.5 + REFINE_PAD;
        const double rf = floor(r), qf = floor(q);
        // cell (x = col, y = row) of the interpolation's base corner, as int32 (clamped far outside the grid first)
        const int row = (int)fmin(fmax(rf - REFINE_PAD, -8.), (double)A.ny + 8.), col = (int)fmin(fmax(qf - REFINE_PAD, -8.), (double)A.nx + 8.);
        double f[4], dq[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double v[4];
            const int y = row - 1 + a;
            const int yc = min(max(y, 0), A.ny - 1);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int x = col - 1 + b;
                const bool in = x >= 0 && y >= 0 && x < A.nx && y < A.ny;        // GridArrayAdapter::GetValue (:69-81)
                const float cv = value_to_cost(cells[A.nx * yc + min(max(x, 0), A.nx - 1)]);   // unconditional clamped load, select after
                v[b] = (double)(in ? cv : 0.9f);
            }
            hermite(v[0], v[1], v[2], v[3], q - qf, f[a], dq[a]);
        }
        ET_MARK(1);
        double val, dvdr, dvdq, unused;
        hermite(f[0], f[1], f[2], f[3], r - rf, val, dvdr);
        hermite(dq[0], dq[1], dq[2], dq[3], r - rf, dvdq, unused);
        const double ri = scale * val;
        const double J0 = scale * (dvdr * ninv), J1 = scale * (dvdq * ninv);
        const double J2 = scale * (dvdr * (dwx * ninv) + dvdq * (dwy * ninv));
        acc[0] += ri * ri;
        acc[1] += J0 * ri; acc[2] += J1 * ri; acc[3] += J2 * ri;
        acc[4] += J0 * J0; acc[5] += J0 * J1; acc[6] += J0 * J2; acc[7] += J1 * J1; acc[8] += J1 * J2; acc[9] += J2 * J2;
        ET_MARK(2);
    }
    ET_MARK(3);
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = wave_sum_f64(acc[k]);
    if (lane == 0)
        for (int k = 0; k < 10; ++k) part[wave][k] = acc[k];
    ET_MARK(4);
}
__device__ __attribute__((unused)) static void refine_eval(const RefineArgs &A, const unsigned short *__restrict__ cells, const float *__restrict__ pts,
                                   const double p0, const double p1, const double p2, double (*part)[10])
{
    refine_eval_strided(A, cells, pts, p0, p1, p2, part, blockDim.x);
}
__device__ static inline bool chol3(const double A[6], const double b[3], double y[3])
{
#pragma clang fp contract(off)
    const double l00 = sqrt(A[0]);
    if (!(l00 > 0.)) return false;
    const double l10 = A[1] / l00, l20 = A[2] / l00;
    const double d1 = A[3] - l10 * l10;
    if (!(d1 > 0.)) return false;
    const double l11 = sqrt(d1), l21 = (A[4] - l20 * l10) / l11;
    const double d2 = A[5] - l20 * l20 - l21 * l21;
    if (!(d2 > 0.)) return false;
    const double l22 = sqrt(d2);
    const double z0 = b[0] / l00, z1 = (b[1] - l10 * z0) / l11, z2 = (b[2] - l20 * z0 - l21 * z1) / l22;
    y[2] = z2 / l22; y[1] = (z1 - l21 * y[2]) / l11; y[0] = (z0 - l10 * y[1] - l20 * y[2]) / l00;
    return isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]);
}
// First wave: totals of an evaluation at pose p (the wave partials + the translation / rotation delta blocks,
// translation_delta_cost_functor_2d.h:24-29, rotation_delta_cost_functor_2d.h:24-28)
__device__ static void refine_totals(const RefineArgs &A, const double (*part)[10], int nw, const double p[3], double S[10])
{
#pragma clang fp contract(off)
    // called by the whole first wave: lane k < 10 adds sum k over the waves (in wave order), lane 0 collects them
    {
        const int lane = threadIdx.x & 63, k = lane < 10 ? lane : 0;
        double v = 0.;
        for (int w = 0; w < nw; ++w) v += part[w][k];
#pragma unroll
        for (int q = 0; q < 10; ++q) S[q] = __shfl(v, q, 64);
    }
    const double r0 = A.w_t * (p[0] - A.tx), r1 = A.w_t * (p[1] - A.ty), r2 = A.w_r * (p[2] - A.a0);
    S[0] += r0 * r0 + r1 * r1 + r2 * r2;
    S[1] += A.w_t * r0; S[2] += A.w_t * r1; S[3] += A.w_r * r2;
    S[4] += A.w_t * A.w_t; S[7] += A.w_t * A.w_t; S[9] += A.w_r * A.w_r;
}
// Thread 0: TrustRegionMinimizer's loop head up to the next candidate -- FinalizeIterationAndCheckIfMinimizerCanContinue,
// LevenbergMarquardtStrategy::ComputeStep on the column-scaled Jacobian (through the normal equations), the model cost
// change; invalid steps shrink the radius and retry without a new evaluation.  Sets st.xc / st.mcc or st.done.
__device__ static void refine_next_candidate(const RefineArgs &A, RefineState &st)
{
#pragma clang fp contract(off)
    for (;;) {
        if (st.successful && st.x_cost < st.min_cost) { st.min_cost = st.x_cost; st.best[0] = st.x[0]; st.best[1] = st.x[1]; st.best[2] = st.x[2]; }
        if (st.iter >= A.max_iter) { st.termination = 1; st.done = 1; return; }
        if (st.successful && st.gmax <= 1e-10) { st.termination = 0; st.done = 1; return; }
        if (st.radius < 1e-32) { st.termination = 0; st.done = 1; return; }
        ++st.iter;
        const double s0 = st.s[0], s1 = st.s[1], s2 = st.s[2];
        const double Hs[6] = {s0 * st.H[0] * s0, s0 * st.H[1] * s1, s0 * st.H[2] * s2, s1 * st.H[3] * s1, s1 * st.H[4] * s2, s2 * st.H[5] * s2};
        const double gs[3] = {s0 * st.g[0], s1 * st.g[1], s2 * st.g[2]};
        double M[6] = {Hs[0], Hs[1], Hs[2], Hs[3], Hs[4], Hs[5]}, y[3], step[3] = {0., 0., 0.};
        M[0] += fmin(fmax(Hs[0], 1e-6), 1e32) / st.radius; M[3] += fmin(fmax(Hs[3], 1e-6), 1e32) / st.radius; M[5] += fmin(fmax(Hs[5], 1e-6), 1e32) / st.radius;
        double mcc = -1.;
        if (chol3(M, gs, y)) {
            step[0] = -y[0]; step[1] = -y[1]; step[2] = -y[2];
            const double Hd[3] = {Hs[0] * step[0] + Hs[1] * step[1] + Hs[2] * step[2], Hs[1] * step[0] + Hs[3] * step[1] + Hs[4] * step[2],
                                  Hs[2] * step[0] + Hs[4] * step[1] + Hs[5] * step[2]};
            mcc = -(step[0] * gs[0] + step[1] * gs[1] + step[2] * gs[2]) - 0.5 * (step[0] * Hd[0] + step[1] * Hd[1] + step[2] * Hd[2]);
        }
        if (!(mcc > 0.)) {                                                       // HandleInvalidStep
            st.successful = 0;
            if (++st.invalid >= 5) { st.termination = 2; st.done = 1; return; }
            st.radius /= st.decrease; st.decrease *= 2.;
            continue;
        }
        st.invalid = 0;
        st.mcc = mcc;
        st.xc[0] = st.x[0] + step[0] * s0; st.xc[1] = st.x[1] + step[1] * s1; st.xc[2] = st.x[2] + step[2] * s2;
        return;
    }
}
// Thread 0: the candidate's evaluation is in -- tolerances, step quality, accept / reject (HandleSuccessfulStep /
// HandleUnsuccessfulStep, LevenbergMarquardtStrategy::StepAccepted / StepRejected, TrustRegionStepEvaluator)
__device__ static void refine_judge(const RefineArgs &A, RefineState &st, const double S[10])
{
#pragma clang fp contract(off)
    const double c_cost = 0.5 * S[0];
    const double d0 = st.x[0] - st.xc[0], d1 = st.x[1] - st.xc[1], d2 = st.x[2] - st.xc[2];
    if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) <= 1e-8 * (st.x_norm + 1e-8)) { st.termination = 0; st.done = 1; return; }   // ParameterToleranceReached
    if (fabs(st.x_cost - c_cost) <= 1e-6 * st.x_cost) { st.termination = 0; st.done = 1; return; }                      // FunctionToleranceReached
    const double rho = fmax((st.ev_cur - c_cost) / st.mcc, (st.ev_ref - c_cost) / (st.acc_ref + st.mcc));               // StepQuality
    if (rho > 1e-3) {
        st.x[0] = st.xc[0]; st.x[1] = st.xc[1]; st.x[2] = st.xc[2];
        st.g[0] = S[1]; st.g[1] = S[2]; st.g[2] = S[3];
        for (int k = 0; k < 6; ++k) st.H[k] = S[4 + k];
        st.x_norm = sqrt(st.x[0] * st.x[0] + st.x[1] * st.x[1] + st.x[2] * st.x[2]);
        st.x_cost = c_cost;
        st.gmax = fmax(fabs(S[1]), fmax(fabs(S[2]), fabs(S[3])));
        st.successful = 1;
        const double t = 2. * rho - 1.;
        st.radius = fmin(1e16, st.radius / fmax(1. / 3., 1. - t * t * t));
        st.decrease = 2.;
        st.ev_cur = c_cost; st.acc_cand += st.mcc; st.acc_ref += st.mcc;
        if (st.ev_cur < st.ev_min) { st.ev_min = st.ev_cur; st.nonmono = 0; st.ev_cand = st.ev_cur; st.acc_cand = 0.; }
        else { ++st.nonmono; if (st.ev_cur > st.ev_cand) { st.ev_cand = st.ev_cur; st.acc_cand = 0.; } }
        if (st.nonmono == A.max_nonmono) { st.ev_ref = st.ev_cand; st.acc_ref = st.acc_cand; }
    } else {
        st.successful = 0;
        st.radius /= st.decrease; st.decrease *= 2.;
    }
}
// Thread 0 after IterationZero: the solver's state from the totals S of the start pose, up to the first candidate (= the block
// of kg_refine between its first two barriers)
__device__ static inline void refine_begin(const RefineArgs &A, RefineState &st, const double S[10])
{
#pragma clang fp contract(off)
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

}  // namespace
