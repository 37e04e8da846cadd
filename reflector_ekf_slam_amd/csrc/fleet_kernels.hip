#if defined(FLEET_POSE_PHASE)
// ---- phase P's statements (see below), pasted by the kernel's body where the pose rows are due: a rank-3 step on (s_mu, P) as they
// stand, linearised at the pose s_p0; FLEET_POSE_WRAP: normalise the heading behind it
                for (int idx = tid; idx < 4 * n16; idx += RFLEET_THREADS) {
                    const int k = idx / n16, r = idx - k * n16;
                    s_W2[k * FLEET_LD_MAX + r] = (k < 3 && r < n) ? rekf_plower(P, (int)ld, r, k) : 0.0;
                }
                if (tid == 64) {
#pragma clang fp contract(off)
                    const double e0 = L.fix[fix_off] - s_p0[0], e1 = L.fix[fix_off + 1] - s_p0[1];
                    const double e2 = fleet_yaw_innovation(L.fix[fix_off + 2] - s_p0[2]);
                    s_in2[0] = e0 - (s_mu[0] - s_p0[0]);
                    s_in2[1] = e1 - (s_mu[1] - s_p0[1]);
                    s_in2[2] = e2 - (s_mu[2] - s_p0[2]);
                }
                if (tid == 0) {
#pragma clang fp contract(off)
                    // S2 = P1[0:3, 0:3] + R (gps.cc:312-316), inverted by Gauss-Jordan without pivoting as phase D does
                    double A[9];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) A[3 * i + j] = rekf_plower(P, (int)ld, i, j);
                    A[0] += 0.05 * 0.05; A[4] += 0.05 * 0.05; A[8] += 0.017 * 0.017;
                    bool bad = false;
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        const double piv = A[3 * p + p];
                        bad = bad || !(piv > 0.0);
                        const double inv = 1.0 / piv;
                        double col[3], row[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) { col[q] = A[3 * q + p]; row[q] = A[3 * p + q]; }
#pragma unroll
                        for (int i = 0; i < 3; ++i)
#pragma unroll
                            for (int j = 0; j < 3; ++j) {
                                double v;
                                if (i == p) v = (j == p) ? inv : row[j] * inv;
                                else if (j == p) v = -col[i] * inv;
                                else v = A[3 * i + j] - col[i] * (row[j] * inv);
                                A[3 * i + j] = v;
                            }
                    }
                    if (bad) s_flags |= REKF_FLAG_SINGULAR;
#pragma unroll
                    for (int q = 0; q < 9; ++q) s_Si2[q] = A[q];
                }
                __syncthreads();
                for (int r = tid; r < n16; r += RFLEET_THREADS) {                             // K2 = W2 S2^-1, mu2 = mu1 + K2 innov2
#pragma clang fp contract(off)
                    const double w0 = s_W2[r], w1 = s_W2[FLEET_LD_MAX + r], w2 = s_W2[2 * FLEET_LD_MAX + r];
                    double k[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double acc = w0 * s_Si2[c];
                        acc += w1 * s_Si2[3 + c];
                        acc += w2 * s_Si2[6 + c];
                        k[c] = acc;
                        s_K2[c * FLEET_LD_MAX + r] = acc;
                    }
                    s_K2[3 * FLEET_LD_MAX + r] = 0.0;
                    if (r < n) {
                        double acc = k[0] * s_in2[0];
                        acc += k[1] * s_in2[1];
                        acc += k[2] * s_in2[2];
                        s_mu[r] += acc;
                    }
                }
                __syncthreads();
                if (FLEET_POSE_WRAP && tid == 0) {                                            // the update's one heading wrap
                    double sn, cs;
                    rekf_sincos(s_mu[2], &sn, &cs);
                    s_mu[2] = atan2(sn, cs);
                }
                {
                    const int nI = n16 >> 4;
                    const int lr = lane & 15, lk = lane >> 4;
                    int cntr = 0;
                    for (int I = 0; I < nI; ++I)
                        for (int J = 0; J <= I; ++J, ++cntr) {
                            if ((cntr & (RFLEET_THREADS / 64 - 1)) != w) continue;
                            v4d acc = {0, 0, 0, 0};
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_W2[lk * FLEET_LD_MAX + 16 * J + lr], s_K2[lk * FLEET_LD_MAX + 16 * I + lr], acc, 0, 0, 0);
                            const int i = 16 * I + lr;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int j = 16 * J + lk + 4 * r;
                                if (i < n && j <= i) P[i + (size_t)j * ld] -= acc[r];
                            }
                        }
                }
                __syncthreads();
#elif !defined(FLEET_STEP_KERNEL)
// fleet_kernels.hip -- k_fleet_step: many small EKF-SLAM filters, ONE workgroup per filter, one launch per rfleet_submit.
//
// The single filter's kernels (ekf_kernels.hip) spread one scan of an n = 2051 filter over 130 workgroups.  A fleet member is
// small (n <= 259, m <= 64): its whole scan -- Predict, ReflectorMatch's state branch, the joint update, the augmentation
// (reference reflector_ekf_slam.cc:154-206, :370-455, :229-368) -- fits one workgroup, which walks the member's events of the call
// in order, eagerly and in place.  Members are independent: no workgroup waits for another one, nothing spins, and a fleet larger
// than the chip simply queues workgroups.  A member's arithmetic depends on its own state and events only -- not on the grid, the
// member's index or how its events were batched -- so its results are the same bits in any fleet and any call pattern.
//
// Phases of a scan event (workgroup barriers between them; W / Kn are the member's own scratch in HBM, see fleet_dev.h):
//   A  Predict: motion terms (ekf_dev.h: the single filter's doubles), columns 0, 1 of P against column 2, pose block, pose
//   B  match: wave per observation, lanes sweep the landmarks, first minimum of the FP64 distance of float32 differences (cc:426-451);
//      ordered compaction, capacity guard (the first (n_max - n) / 2 new observations are appended).  k_fleet_step_map, for a member
//      that uses the fleet's pre-loaded map, tries the map first (cc:401-425): lanes sweep the map points in global memory, first
//      minimum of the weighted FP64 distance of float32 differences, `< 0.05`; the compaction puts state pairs before map pairs
//   C  H rows (<= 5 non-zeros each; a map pair's rows have the three pose entries only, cc:279-302), W = P H^T gathered from the
//      lower triangle, S = H W + Q into LDS
//   D  S^-1 in LDS: Gauss-Jordan without pivoting (S is SPD; a non-positive pivot raises REKF_FLAG_SINGULAR)
//   E  K = W S^-1 on v_mfma_f64_16x16x4_f64 (S^-1 from LDS), mean update, heading wrap
//   F  P -= K W^T on the lower triangle, 16 x 16 tiles on v_mfma_f64_16x16x4_f64, tiles dealt to the waves
//   P  the scan's pose fix, if it has one and matched a reflector (gps.cc:305-340): a rank-3 step on what C-F left, see below
//   G  augmentation rows and means (cc:311-364)
// and, once per launch, the pose, pose block, n and flags into the member's slot in pinned host memory.
// k_fleet_step_track (a handle that tracks, rfleet_set_tracking) also leaves ONE FleetTrackRec per event, at the end of every pass of
// the event loop: what the slot would hold if the launch ended there, see fleet_track_write.
//
// FP64 MFMA operand layout (16x16x4): lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register r of lane l is
// D[(l >> 4) + 4 r][l & 15].  Phases E and F compute the TRANSPOSED tile (D = B-side rows along the lanes) so that the 16 lanes of
// a group store 128 contiguous bytes of a column of Kn / P.
//
// Phase P.  The reference stacks three pose rows H = [I3 0] with noise R = diag(0.05^2, 0.05^2, 0.017^2) under the reflector rows
// and solves the joint system: up to 67 rows, more than S in LDS and the W / Kn panels hold.  The noise of the joint system is
// block-diagonal between reflector rows and pose rows, so the joint update EQUALS the reflector update (C-F: mu0 -> mu1, P1)
// followed by the pose rows' update at the same linearisation point, whose innovation is taken against the mean C-F left:
//   innov2 = wrap(z - mu0[0:3]) - (mu1[0:3] - mu0[0:3]),   S2 = P1[0:3, 0:3] + R,   K2 = P1[:, 0:3] S2^-1,
//   mu2 = mu1 + K2 innov2,   P2 = P1 - K2 P1[0:3, :]
// (the heading is normalised once, after both).  W2 = P1[:, 0:3] is three contiguous columns of the lower triangle; W2 and K2
// (n x 4, k padded 3 -> 4 with zeros) sit in LDS, in the space S^-1 has left, and the downdate walks phase F's tiles with one
// MFMA each.  A scan without a fix runs C-F as it always did.
#include "fleet_dev.h"

// The kernel's body stands once, below the `#else`, and is compiled four times by this file including itself: k_fleet_step for a
// launch in which no scan carries a fix (the host knows), k_fleet_step_fix otherwise, and k_fleet_step_map (map branch and phase P)
// for a launch in which a member with events matches against a non-empty pre-loaded map, with or without fixes.  In the first two
// every map statement is a discarded one and the map's LDS variables do not exist.  Phase P's statements stand once too, at the
// head of the file, and are pasted the same way: behind phase F, and -- in k_fleet_step_map, for a member on the map -- in front of
// phase C (the pose rows first: see there).  In k_fleet_step phase P and its tests are
// discarded statements, and as a plain (non-template) kernel of that name it compiles to the code it had before phase P existed
// (a template's instantiation does not: its LDS variables get other names and another layout, and the common path lost 0.7 %).
// Both kernels compute a member's plain scans with the same arithmetic (tests/test_fleet_pose_gpu.py: the same bits beside
// neighbours with and without fixes).  k_fleet_step_track is k_fleet_step_map's body plus the records, launched whenever the handle
// tracks (a member without fix and map computes the same bits under that body: tests/test_fleet_map_gpu.py); in the other three every
// tracking statement is a discarded one and s_trk does not exist.
#define FLEET_STEP_KERNEL k_fleet_step
#define FLEET_STEP_FIX false
#define FLEET_STEP_MAP false
#define FLEET_STEP_TRACK false
#include "fleet_kernels.hip"
#undef FLEET_STEP_KERNEL
#undef FLEET_STEP_FIX
#undef FLEET_STEP_MAP
#undef FLEET_STEP_TRACK
#define FLEET_STEP_KERNEL k_fleet_step_fix
#define FLEET_STEP_FIX true
#define FLEET_STEP_MAP false
#define FLEET_STEP_TRACK false
#include "fleet_kernels.hip"
#undef FLEET_STEP_KERNEL
#undef FLEET_STEP_FIX
#undef FLEET_STEP_MAP
#undef FLEET_STEP_TRACK
#define FLEET_STEP_KERNEL k_fleet_step_map
#define FLEET_STEP_FIX true
#define FLEET_STEP_MAP true
#define FLEET_STEP_TRACK false
#include "fleet_kernels.hip"
#undef FLEET_STEP_KERNEL
#undef FLEET_STEP_FIX
#undef FLEET_STEP_MAP
#undef FLEET_STEP_TRACK
#define FLEET_STEP_KERNEL k_fleet_step_track
#define FLEET_STEP_FIX true
#define FLEET_STEP_MAP true
#define FLEET_STEP_TRACK true
#include "fleet_kernels.hip"
#undef FLEET_STEP_KERNEL
#undef FLEET_STEP_FIX
#undef FLEET_STEP_MAP
#undef FLEET_STEP_TRACK

hipError_t rfleet_launch_step(const FleetDev &d, const FleetLaunch &l, hipStream_t s)
{
    if (l.G <= 0) return hipSuccess;
    if (l.track) hipLaunchKernelGGL(k_fleet_step_track, dim3((unsigned)l.G), dim3(RFLEET_THREADS), 0, s, d, l);
    else if (l.M_map > 0) hipLaunchKernelGGL(k_fleet_step_map, dim3((unsigned)l.G), dim3(RFLEET_THREADS), 0, s, d, l);
    else if (l.fix) hipLaunchKernelGGL(k_fleet_step_fix, dim3((unsigned)l.G), dim3(RFLEET_THREADS), 0, s, d, l);
    else hipLaunchKernelGGL(k_fleet_step, dim3((unsigned)l.G), dim3(RFLEET_THREADS), 0, s, d, l);
    return hipGetLastError();
}

#else  // ---- the kernel's body: FLEET_STEP_KERNEL, FLEET_STEP_FIX, FLEET_STEP_MAP, FLEET_STEP_TRACK

__global__ __launch_bounds__(RFLEET_THREADS) void FLEET_STEP_KERNEL(FleetDev d, FleetLaunch L)
{
    constexpr bool FIX = FLEET_STEP_FIX;
    constexpr bool MAP = FLEET_STEP_MAP;
    constexpr bool TRACK = FLEET_STEP_TRACK;
    __shared__ double s_mu[FLEET_LD_MAX];
    __shared__ double s_S[64 * FLEET_SLD];
    __shared__ double s_hv[64][5];
    __shared__ int s_hc[64][5];
    __shared__ double s_dz[64], s_col[64], s_row[64];
    __shared__ float s_obs[2 * RFLEET_MAX_OBS_DEV], s_gx[RFLEET_MAX_OBS_DEV], s_gy[RFLEET_MAX_OBS_DEV];
    __shared__ int s_kind[RFLEET_MAX_OBS_DEV], s_idx[RFLEET_MAX_OBS_DEV];
    __shared__ int s_pairs[2 * RFLEET_MAX_OBS_DEV], s_new[RFLEET_MAX_OBS_DEV];
    __shared__ int s_cnt[2], s_flags;
    __shared__ double s_mu0[FLEET_LD_MAX];                // the linearisation point of a scan whose pose rows go first (k_fleet_step_map)
    __shared__ int s_cntm;                                // map pairs of the scan (k_fleet_step_map; unused and absent elsewhere)
    __shared__ Motion s_mo;
    __shared__ FleetEvent s_ev;
    __shared__ double s_cs[2];
    __shared__ double s_Gp[RFLEET_MAX_OBS_DEV][6], s_Sxi[9], s_RQR[4];
    __shared__ double s_p0[3], s_in2[3], s_Si2[9];       // phase P: the linearisation pose, innov2, S2^-1
    __shared__ double s_trk[16];                          // one FleetTrackRec (k_fleet_step_track; unused and absent elsewhere)
    double *const s_W2 = s_S, *const s_K2 = s_S + 4 * FLEET_LD_MAX;     // phase P: W2, K2 as [4][FLEET_LD_MAX] (S^-1 is dead by then)
    static_assert(8 * FLEET_LD_MAX <= 64 * FLEET_SLD, "W2 and K2 live in S's space");

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = blockIdx.x;
    if (g >= L.G) return;
    const int mem = L.members[g];
    const size_t ld = (size_t)d.ld;
    double *mu_g = d.mu + (size_t)mem * ld;
    double *P = d.P + (size_t)mem * ld * ld;
    double *W = d.W + (size_t)mem * ld * RFLEET_PANEL_COLS;
    double *Kn = d.Kn + (size_t)mem * ld * RFLEET_PANEL_COLS;
    FleetMemberCtl *ctl = d.ctl + mem;
    const FleetMemberOpt opt = d.opt[mem];
    int n = ctl->n;
    if (tid == 0) s_flags = ctl->flags;
    for (int i = tid; i < n; i += RFLEET_THREADS) s_mu[i] = mu_g[i];
    const int e0 = L.ev_begin[g], e1 = L.ev_begin[g + 1];
    bool rec_new = false;             // a scan of this call has rewritten the match record
    int recK = 0, rec_ns = 0, rec_nn = 0;
    [[maybe_unused]] int rec_nm = 0;
    [[maybe_unused]] bool use_map = false;                // this member matches against the fleet's map
    if constexpr (MAP) use_map = L.M_map > 0 && L.map_use[mem] != 0;
    __syncthreads();

    for (int e = e0; e < e1; ++e) {
        // ---- A: Predict (cc:154-206)
        if (tid == 0) {
            s_ev = L.ev[e];
            motion_terms_of(opt.model, s_ev.dt, s_ev.vt[0], s_ev.vt[1], s_ev.vt[2], opt.lin_cov, opt.ang_cov, s_mu[2], s_mo);
        }
        __syncthreads();
        const int kind = s_ev.kind, K = s_ev.K, obs_off = s_ev.obs_off;    // (thread 0 rewrites s_ev at the top of the next event)
        int fix_off = -1;
        if constexpr (FIX) fix_off = s_ev.fix_off;
        if constexpr (TRACK) {
            if (kind == 2) {                              // a message the host dropped: nothing moves, the record is the state as it stands
                fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, 0, 0, 0);
                continue;
            }
        }
        {
#pragma clang fp contract(off)
            const double a = s_mo.a, b = s_mo.b;
            for (int r = 3 + tid; r < n; r += RFLEET_THREADS) {     // columns 0, 1 (= rows 0, 1: the lower triangle is the only copy)
                const double p2 = P[r + 2 * ld];
                P[r] = P[r] + a * p2;
                P[r + ld] = P[r + ld] + b * p2;
            }
            if (tid == 0) {
                double C[9];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) C[i + 3 * j] = rekf_plower(P, (int)ld, i, j);
                corner_predict(C, 3, s_mo);
                for (int j = 0; j < 3; ++j)
                    for (int i = j; i < 3; ++i) P[i + j * ld] = C[i + 3 * j];
                s_mu[0] += s_mo.d[0]; s_mu[1] += s_mo.d[1]; s_mu[2] += s_mo.d[2];      // cc:180/:204
                double sn, cs;
                rekf_sincos(s_mu[2], &sn, &cs);
                s_mu[2] = atan2(sn, cs);                                              // cc:181/:205
            }
        }
        __syncthreads();
        if (kind != 1) {
            if constexpr (TRACK) fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, 0, 0, 0);
            continue;
        }
        rec_new = true; recK = K; rec_ns = 0; rec_nn = 0;
        if constexpr (MAP) rec_nm = 0;
        if (K <= 0) {                                                                 // cc:235-236: an empty scan is a Predict
            if constexpr (TRACK) fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, 0, 0, 0);
            continue;
        }

        // ---- B: ReflectorMatch, state branch (cc:370-455)
        if (tid < 2 * K) s_obs[tid] = L.obs[obs_off + tid];
        if (tid == 64) rekf_sincos(s_mu[2], &s_cs[1], &s_cs[0]);
        __syncthreads();
        if (tid < K) fleet_obs_to_global(s_mu[0], s_mu[1], s_cs[0], s_cs[1], s_obs[2 * tid], s_obs[2 * tid + 1], s_gx[tid], s_gy[tid]);
        __syncthreads();
        {
#pragma clang fp contract(off)
            const int M = (n - 3) / 2;
            for (int i = w; i < K; i += RFLEET_THREADS / 64) {
                const float gx = s_gx[i], gy = s_gy[i];
                if constexpr (MAP) {
                    if (use_map) {                                                            // cc:401-425: the map first
                        double best = 0; int bj = -1;
                        for (int j = lane; j < L.M_map; j += 64) {
                            const double *S = L.map_cov + 4 * (size_t)j;                      // cc:407
                            const float ex = L.map_xy[2 * j] - gx, ey = L.map_xy[2 * j + 1] - gy;    // cc:408 (map - g, float32)
                            const double dx = (double)ex, dy = (double)ey;
                            const double t0 = dx * S[0] + dy * S[2];                          // cc:411: (delta sigma) delta^T
                            const double t1 = dx * S[1] + dy * S[3];
                            const double dist = sqrt(t0 * dx + t1 * dy);
                            // a NaN distance (an indefinite S) never wins, wherever it stands: a lane that saw nothing else keeps bj < 0
                            if (dist == dist && (bj < 0 || dist < best)) { best = dist; bj = j; }
                        }
                        for (int off = 32; off > 0; off >>= 1) {
                            const double ob = __shfl_xor(best, off, 64);
                            const int oj = __shfl_xor(bj, off, 64);
                            if (oj >= 0 && (bj < 0 || ob < best || (ob == best && oj < bj))) { best = ob; bj = oj; }
                        }
                        const int hit = __shfl((bj >= 0 && best < 0.05) ? bj : -1, 0, 64);    // cc:420; lane 0 decides for the wave
                        if (hit >= 0) {
                            if (lane == 0) { s_kind[i] = 0; s_idx[i] = hit; }
                            continue;
                        }
                    }
                }
                double best = 0; int bj = -1;
                for (int j = lane; j < M; j += 64) {
                    const float lx = (float)s_mu[3 + 2 * j], ly = (float)s_mu[4 + 2 * j];     // cc:431
                    const float ex = gx - lx, ey = gy - ly;                                   // cc:433
                    const double dx = (double)ex, dy = (double)ey;
                    const double dist = sqrt(dx * dx + dy * dy);                              // cc:437
                    if (bj < 0 || dist < best) { best = dist; bj = j; }
                }
                for (int off = 32; off > 0; off >>= 1) {                                      // first minimum: ties go to the lower index
                    const double ob = __shfl_xor(best, off, 64);
                    const int oj = __shfl_xor(bj, off, 64);
                    if (oj >= 0 && (bj < 0 || ob < best || (ob == best && oj < bj))) { best = ob; bj = oj; }
                }
                if (lane == 0) { s_kind[i] = (bj >= 0 && best < 0.6) ? 1 : 2; s_idx[i] = bj; }   // cc:446
            }
        }
        __syncthreads();
        if (tid == 0) {
            int ns = 0, nn = 0;
            const int room = (d.n_max - n) / 2;
            bool over = false;
            for (int i = 0; i < K; ++i) {
                if (s_kind[i] == 1) { s_pairs[2 * ns] = i; s_pairs[2 * ns + 1] = s_idx[i]; ++ns; }
                else if (MAP && s_kind[i] == 0) continue;                                     // (a map pair: listed below)
                else if (nn < room) s_new[nn++] = i;
                else over = true;                                                             // capacity guard (ours)
            }
            if (over) s_flags |= REKF_FLAG_CAPACITY;
            s_cnt[0] = ns; s_cnt[1] = nn;
            if constexpr (MAP) {                                                              // map pairs behind the state pairs
                int nm = 0;
                for (int i = 0; i < K; ++i)
                    if (s_kind[i] == 0) { s_pairs[2 * (ns + nm)] = i; s_pairs[2 * (ns + nm) + 1] = s_idx[i]; ++nm; }
                s_cntm = nm;
            }
        }
        __syncthreads();
        int n_pairs = s_cnt[0];
        [[maybe_unused]] const int NS = n_pairs;                                              // rows [2 NS, m) are the map pairs'
        if constexpr (MAP) n_pairs += s_cntm;
        const int MM = n_pairs, N2 = s_cnt[1], m = 2 * MM;
        rec_ns = NS; rec_nn = N2;
        if constexpr (MAP) rec_nm = MM - NS;
        // A member on the map takes its fix BEFORE the reflector rows (same linearisation point, same joint update: the two groups of
        // rows have independent noise).  Map rows pin the pose; behind them P1's pose block is what a large cancellation left, and
        // phase P's gain would carry that error into the mean (2.7e-14 at 31 map pairs), while P0's pose block is well conditioned.
#if FLEET_STEP_MAP
        const bool fix_first = use_map && fix_off >= 0 && MM > 0;
#else
        constexpr bool fix_first = false;                     // (a variable here gives k_fleet_step_fix another schedule)
#endif

        if (MM > 0) {
            if constexpr (MAP) if (fix_first) {
                const int n16 = (n + 15) & ~15;
                for (int i = tid; i < n; i += RFLEET_THREADS) s_mu0[i] = s_mu[i];
                if (tid < 3) s_p0[tid] = s_mu[tid];
                __syncthreads();
#define FLEET_POSE_PHASE
#define FLEET_POSE_WRAP false
#include "fleet_kernels.hip"
#undef FLEET_POSE_PHASE
#undef FLEET_POSE_WRAP
            }
            // ---- C: H rows, W = P H^T, S = H W + Q (cc:246-305)
            if (tid < MM) {
#pragma clang fp contract(off)
                const int i = tid, local_id = s_pairs[2 * i], gid = s_pairs[2 * i + 1];
                const double c = s_cs[0], s = s_cs[1];                                        // cc:252-253
                double dx, dy;
                int col = 3 + 2 * gid;
                if constexpr (MAP) {
                    const double *mu_l = fix_first ? s_mu0 : s_mu;                            // the rows' linearisation point
                    if (i >= NS) {                                                            // cc:279-302: the landmark is a map point
                        dx = (double)L.map_xy[2 * gid] - mu_l[0]; dy = (double)L.map_xy[2 * gid + 1] - mu_l[1];    // cc:282
                        col = 0;                                                              // (entries 3, 4 of a map row are never read)
                    } else { dx = mu_l[3 + 2 * gid] - mu_l[0]; dy = mu_l[4 + 2 * gid] - mu_l[1]; }
                } else { dx = s_mu[3 + 2 * gid] - s_mu[0]; dy = s_mu[4 + 2 * gid] - s_mu[1]; }
                s_dz[2 * i] = (double)s_obs[2 * local_id] - (dx * c + dy * s);                // cc:265-270
                s_dz[2 * i + 1] = (double)s_obs[2 * local_id + 1] - (-dx * s + dy * c);
                for (int rr = 0; rr < 2; ++rr) {
                    int *hc = s_hc[2 * i + rr];
                    hc[0] = 0; hc[1] = 1; hc[2] = 2; hc[3] = col; hc[4] = col + 1;
                }
                double *h0 = s_hv[2 * i], *h1 = s_hv[2 * i + 1];
                h0[0] = -c; h0[1] = -s; h0[2] = -dx * s + dy * c; h0[3] = c;  h0[4] = s;      // cc:272-275
                h1[0] = s;  h1[1] = -c; h1[2] = -dx * c - dy * s; h1[3] = -s; h1[4] = c;
                if constexpr (MAP) if (fix_first) {                                           // the innovation against what the fix moved
                    const int nq = i < NS ? 5 : 3;
                    double a0 = 0, a1 = 0;
                    for (int q = 0; q < nq; ++q) {
                        const int cq = s_hc[2 * i][q];
                        const double dm = s_mu[cq] - s_mu0[cq];
                        a0 += h0[q] * dm; a1 += h1[q] * dm;
                    }
                    s_dz[2 * i] -= a0; s_dz[2 * i + 1] -= a1;
                }
            }
            if constexpr (FIX) {
                if (fix_off >= 0 && tid >= 64 && tid < 67) s_p0[tid - 64] = s_mu[tid - 64];   // mu0's pose, for phase P
            }
            __syncthreads();
            const int n16 = (n + 15) & ~15, m16 = (m + 15) & ~15, m4 = (m + 3) & ~3;
            for (int idx = tid; idx < n16 * m16; idx += RFLEET_THREADS) {
#pragma clang fp contract(off)
                const int j = idx / n16, r = idx - j * n16;
                double v = 0;
                if (r < n && j < m) {
                    int nq = 5;                                                               // a map row: the three pose entries (cc:300)
                    if constexpr (MAP) nq = j < 2 * NS ? 5 : 3;
                    for (int q = 0; q < nq; ++q) v += rekf_plower(P, (int)ld, r, s_hc[j][q]) * s_hv[j][q];
                }
                W[r + j * ld] = v;
            }
            __syncthreads();
            for (int idx = tid; idx < 64 * 64; idx += RFLEET_THREADS) {
#pragma clang fp contract(off)
                const int i = idx >> 6, j = idx & 63;
                double v = 0;
                if (i < m && j < m) {
                    int nq = 5;
                    if constexpr (MAP) nq = i < 2 * NS ? 5 : 3;
                    for (int q = 0; q < nq; ++q) v += s_hv[i][q] * W[s_hc[i][q] + j * ld];
                    if (i == j) v += opt.obs_cov;                                             // cc:276
                }
                s_S[i * FLEET_SLD + j] = v;
            }
            __syncthreads();
            // ---- D: S^-1 in place
            for (int p = 0; p < m; ++p) {
                if (tid < m) { s_col[tid] = s_S[tid * FLEET_SLD + p]; s_row[tid] = s_S[p * FLEET_SLD + tid]; }
                __syncthreads();
                const double piv = s_col[p];
                if (tid == 0 && !(piv > 0.0)) s_flags |= REKF_FLAG_SINGULAR;
                const double inv = 1.0 / piv;
                for (int idx = tid; idx < m * m; idx += RFLEET_THREADS) {
                    const int i = idx / m, j = idx - i * m;
                    double v;
                    if (i == p) v = (j == p) ? inv : s_row[j] * inv;
                    else if (j == p) v = -s_col[i] * inv;
                    else v = s_S[i * FLEET_SLD + j] - s_col[i] * (s_row[j] * inv);
                    s_S[i * FLEET_SLD + j] = v;
                }
                __syncthreads();
            }
            // ---- E: K = W S^-1 (transposed tiles: rows of the state along the lanes), mean update (cc:306-307)
            {
                const int nI = n16 >> 4, nJ = m16 >> 4;
                const int lr = lane & 15, lk = lane >> 4;
                for (int t = w; t < nI * nJ; t += RFLEET_THREADS / 64) {
                    const int I = t / nJ, Jb = t - I * nJ;
                    v4d acc = {0, 0, 0, 0};
                    for (int k0 = 0; k0 < m4; k0 += 4) {
                        const double a = s_S[(k0 + lk) * FLEET_SLD + 16 * Jb + lr];
                        const double b = W[(16 * I + lr) + (size_t)(k0 + lk) * ld];
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) Kn[(16 * I + lr) + (size_t)(16 * Jb + lk + 4 * r) * ld] = acc[r];
                }
            }
            __syncthreads();
            for (int r = tid; r < n; r += RFLEET_THREADS) {
#pragma clang fp contract(off)
                double acc = 0;
                for (int j = 0; j < m; ++j) acc += Kn[r + j * ld] * s_dz[j];
                s_mu[r] += acc;
            }
            __syncthreads();
            if (tid == 0 && (!FIX || fix_off < 0 || fix_first)) {                             // (with a fix behind the rows: after phase P)
                double sn, cs;
                rekf_sincos(s_mu[2], &sn, &cs);
                s_mu[2] = atan2(sn, cs);
            }
            // ---- F: P -= K W^T, lower triangle (cc:308)
            {
                const int nI = n16 >> 4;
                const int lr = lane & 15, lk = lane >> 4;
                int cntr = 0;
                for (int I = 0; I < nI; ++I)
                    for (int J = 0; J <= I; ++J, ++cntr) {
                        if ((cntr & (RFLEET_THREADS / 64 - 1)) != w) continue;
                        v4d acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
                        const double *wa = W + 16 * J + lr + (size_t)lk * ld;
                        const double *kb = Kn + 16 * I + lr + (size_t)lk * ld;
                        int k0 = 0;
                        for (; k0 + 8 <= m4; k0 += 8) {
                            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[(size_t)k0 * ld], kb[(size_t)k0 * ld], acc0, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[(size_t)(k0 + 4) * ld], kb[(size_t)(k0 + 4) * ld], acc1, 0, 0, 0);
                        }
                        if (k0 < m4) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[(size_t)k0 * ld], kb[(size_t)k0 * ld], acc0, 0, 0, 0);
                        const v4d acc = acc0 + acc1;
                        const int i = 16 * I + lr;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int j = 16 * J + lk + 4 * r;
                            if (i < n && j <= i) P[i + (size_t)j * ld] -= acc[r];
                        }
                    }
            }
            __syncthreads();
            // ---- P: the pose fix (gps.cc:305-340) as a rank-3 step on mu1 = s_mu (heading not yet wrapped), P1 = P
            if constexpr (FIX) if (fix_off >= 0 && !fix_first) {
#define FLEET_POSE_PHASE
#define FLEET_POSE_WRAP true
#include "fleet_kernels.hip"
#undef FLEET_POSE_PHASE
#undef FLEET_POSE_WRAP
            }
        }

        // ---- G: augmentation (cc:311-364)
        if (N2 > 0) {
            {
#pragma clang fp contract(off)
                if (tid == 0) {
                    rekf_sincos(s_mu[2], &s_cs[1], &s_cs[0]);                                 // cc:323-324
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) s_Sxi[i * 3 + j] = rekf_plower(P, (int)ld, i, j);   // cc:322
                }
                __syncthreads();
                const double c = s_cs[0], s = s_cs[1];
                if (tid < N2) {
                    const int local_id = s_new[tid];                                          // cc:338
                    const float fx = s_obs[2 * local_id], fy = s_obs[2 * local_id + 1];
                    float gx, gy;
                    fleet_obs_to_global(s_mu[0], s_mu[1], c, s, fx, fy, gx, gy);              // cc:339
                    s_mu[n + 2 * tid] = (double)gx;                                           // cc:341-342
                    s_mu[n + 2 * tid + 1] = (double)gy;
                    const double rx = (double)fx, ry = (double)fy;
                    s_Gp[tid][0] = 1.; s_Gp[tid][1] = 0.; s_Gp[tid][2] = -rx * s - ry * c;    // cc:347
                    s_Gp[tid][3] = 0.; s_Gp[tid][4] = 1.; s_Gp[tid][5] = rx * c - ry * s;
                }
                if (tid == 64) {
                    const double q = opt.obs_cov;                                             // Gz Qt Gz^T, Gz = R(theta) (cc:349,354)
                    s_RQR[0] = c * q * c + (-s) * q * (-s); s_RQR[1] = c * q * s + (-s) * q * c;
                    s_RQR[2] = s * q * c + c * q * (-s);    s_RQR[3] = s * q * s + c * q * c;
                }
            }
            __syncthreads();
            for (int idx = tid; idx < n * N2; idx += RFLEET_THREADS) {                        // sigma_mx (cc:355-357), below the diagonal
#pragma clang fp contract(off)
                const int a = idx / n, col = idx - a * n;
                const double q0 = rekf_plower(P, (int)ld, col, 0), q1 = rekf_plower(P, (int)ld, col, 1), q2 = rekf_plower(P, (int)ld, col, 2);
                for (int rr = 0; rr < 2; ++rr) {
                    double acc = 0;
                    acc += s_Gp[a][rr * 3 + 0] * q0;
                    acc += s_Gp[a][rr * 3 + 1] * q1;
                    acc += s_Gp[a][rr * 3 + 2] * q2;
                    P[(size_t)(n + 2 * a + rr) + (size_t)col * ld] = acc;
                }
            }
            for (int idx = tid; idx < N2 * N2; idx += RFLEET_THREADS) {                       // sigma_mm (cc:354,358)
#pragma clang fp contract(off)
                const int a = idx / N2, b = idx - a * N2;
                for (int rr = 0; rr < 2; ++rr)
                    for (int cc = 0; cc < 2; ++cc) {
                        const size_t gi = (size_t)(n + 2 * a + rr), gj = (size_t)(n + 2 * b + cc);
                        if (gi < gj) continue;
                        double acc = 0;
                        for (int k = 0; k < 3; ++k) {
                            double t = 0;
                            for (int l = 0; l < 3; ++l) t += s_Gp[a][rr * 3 + l] * s_Sxi[l * 3 + k];
                            acc += t * s_Gp[b][cc * 3 + k];
                        }
                        P[gi + gj * ld] = acc + s_RQR[rr * 2 + cc];
                    }
            }
            n += 2 * N2;                                                                      // cc:360-363
            __syncthreads();
        }
        if constexpr (TRACK) fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, rec_ns, rec_nn, rec_nm);
    }

    // ---- the member's state, record and host slot
    __syncthreads();
    for (int i = tid; i < n; i += RFLEET_THREADS) mu_g[i] = s_mu[i];
    FleetPoseSlot *slot = d.pose + mem;
    if (tid < 3) slot->mu3[tid] = s_mu[tid];
    else if (tid < 12) slot->C9[tid - 3] = rekf_plower(P, (int)ld, (tid - 3) % 3, (tid - 3) / 3);
    else if (tid == 12) { slot->n = n; slot->flags = s_flags; ctl->n = n; ctl->flags = s_flags; }
    if (rec_new) {
        if (tid == 13) { ctl->K = recK; ctl->n_state = rec_ns; ctl->n_new = rec_nn; }
        if (tid >= 64 && tid < 64 + 2 * rec_ns) ctl->state_pairs[tid - 64] = s_pairs[tid - 64];
        if (tid >= 128 && tid < 128 + rec_nn) ctl->new_ids[tid - 128] = s_new[tid - 128];
        if constexpr (MAP) {
            if (tid == 14) ctl->n_map = rec_nm;
            if (tid >= 192 && tid < 192 + 2 * rec_nm) ctl->map_pairs[tid - 192] = s_pairs[2 * rec_ns + tid - 192];
        }
    }
}

#endif
