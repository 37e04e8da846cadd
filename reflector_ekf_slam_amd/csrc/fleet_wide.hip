// fleet_wide.hip -- k_fleet_step_wide: the fleet step for a submit that holds at least one scan of more than RFLEET_MAX_OBS_DEV
// observations (rfleet_set_wide_scans).  ONE launch per rfleet_submit and one workgroup per member with events, as the four kernels
// of fleet_kernels.hip; it is a kernel and a file of its own so that those four stay the code they were.
//
// A wide scan (32 < K <= RFLEET_MAX_OBS_WIDE_DEV) is matched ONCE, against the state behind Predict (mu0, P0), and its MM pairs are
// applied in ceil(MM / 32) exact block steps of 32 pairs: every row is linearised at mu0 (cos / sin of mu0's heading) and block b's
// innovation is corrected by what the blocks before it moved,
//   dz_b = z_b - h_b(mu0) - H_b (mu_b - mu0),   W_b = P_b H_b^T,   S_b = H_b W_b + q I,   K_b = W_b S_b^-1,
//   mu_b+1 = mu_b + K_b dz_b,   P_b+1 = P_b - K_b W_b^T.
// The observation noise is q I, so the sequence EQUALS the reference's joint update of all MM pairs.  This is the arithmetic phase P
// and k_fleet_step_map's fix_first path already use for a group of rows at an earlier linearisation point (s_mu0); the loop only
// repeats phases C-F.  The heading is normalised once, behind the last block (behind phase P where a fix follows); a fix of a member
// on the map goes in front of the first block and every block is corrected against s_mu0.  Whether a row is a state row (5 entries)
// or a map row (3) goes by the pair's GLOBAL index against NS.  W / Kn (ld x 64) are reused per block.  The augmentation runs once,
// behind everything, over up to 128 new observations.
//
// The launch also carries the call's narrow scans, odometry events and dropped messages of every member.  For those the loop runs
// one block with mu0 = mu and no correction term, and every statement stands as in fleet_kernels.hip's body, in the same order under
// the same `fp contract(off)` regions: the same bits (tests/test_fleet_wide_gpu.py), the guarantee k_fleet_step_track gives.
//
// Fix, map and track are chosen at RUN TIME from L.fix, L.M_map / L.map_use and L.track: the wide launch is the rare path and one
// kernel serves all of them; what that costs is in DESIGN.md 10.13.  The match record of a wide launch goes into FleetWideRec.
//
// Phase P's statements are fleet_kernels.hip's own (pasted by inclusion, as that file pastes them into its body).
#include "fleet_dev.h"

#define FLEET_BLOCK_PAIRS 32     // pairs per block step: m <= 64 rows, what S in LDS and the W / Kn panels hold

__global__ __launch_bounds__(RFLEET_THREADS) void k_fleet_step_wide(FleetDev d, FleetLaunch L, FleetWideRec *wrec)
{
    constexpr int KW = RFLEET_MAX_OBS_WIDE_DEV;
    const bool FIX = L.fix != nullptr;
    const bool MAP = L.M_map > 0;
    const bool TRACK = L.track != nullptr;
    __shared__ double s_mu[FLEET_LD_MAX];
    __shared__ double s_S[64 * FLEET_SLD];
    __shared__ double s_hv[64][5];
    __shared__ int s_hc[64][5];
    __shared__ double s_dz[64], s_col[64], s_row[64];
    __shared__ float s_obs[2 * KW], s_gx[KW], s_gy[KW];
    __shared__ int s_kind[KW], s_idx[KW];
    __shared__ int s_pairs[2 * KW], s_new[KW];
    __shared__ int s_cnt[2], s_flags;
    __shared__ double s_mu0[FLEET_LD_MAX];                // the linearisation point of a scan of several groups of rows
    __shared__ int s_cntm;
    __shared__ Motion s_mo;
    __shared__ FleetEvent s_ev;
    __shared__ double s_cs[2];
    __shared__ double s_Gp[RFLEET_MAX_NEW_WIDE_DEV][6], s_Sxi[9], s_RQR[4];
    __shared__ double s_p0[3], s_in2[3], s_Si2[9];
    __shared__ double s_trk[16];
    double *const s_W2 = s_S, *const s_K2 = s_S + 4 * FLEET_LD_MAX;
    static_assert(8 * FLEET_LD_MAX <= 64 * FLEET_SLD, "W2 and K2 live in S's space");
    static_assert(2 * KW <= RFLEET_THREADS, "one thread per float of a scan");

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
    bool rec_new = false;
    int recK = 0, rec_ns = 0, rec_nn = 0, rec_nm = 0;
    bool use_map = false;
    if (MAP) use_map = L.map_use[mem] != 0;
    __syncthreads();

    for (int e = e0; e < e1; ++e) {
        // ---- A: Predict (cc:154-206)
        if (tid == 0) {
            s_ev = L.ev[e];
            motion_terms_of(opt.model, s_ev.dt, s_ev.vt[0], s_ev.vt[1], s_ev.vt[2], opt.lin_cov, opt.ang_cov, s_mu[2], s_mo);
        }
        __syncthreads();
        const int kind = s_ev.kind, obs_off = s_ev.obs_off;
        const int K = s_ev.K < KW ? s_ev.K : KW;                                      // (the host refuses K > KW: the lists hold KW)
        int fix_off = -1;
        if (FIX) fix_off = s_ev.fix_off;
        if (TRACK) {
            if (kind == 2) {
                fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, 0, 0, 0);
                continue;
            }
        }
        {
#pragma clang fp contract(off)
            const double a = s_mo.a, b = s_mo.b;
            for (int r = 3 + tid; r < n; r += RFLEET_THREADS) {
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
                s_mu[0] += s_mo.d[0]; s_mu[1] += s_mo.d[1]; s_mu[2] += s_mo.d[2];
                double sn, cs;
                rekf_sincos(s_mu[2], &sn, &cs);
                s_mu[2] = atan2(sn, cs);
            }
        }
        __syncthreads();
        if (kind != 1) {
            if (TRACK) fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, 0, 0, 0);
            continue;
        }
        rec_new = true; recK = K; rec_ns = 0; rec_nn = 0; rec_nm = 0;
        if (K <= 0) {
            if (TRACK) fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, 0, 0, 0);
            continue;
        }

        // ---- B: ReflectorMatch (cc:370-455), ONCE over all K observations
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
                if (use_map) {                                                                // cc:401-425: the map first
                    double best = 0; int bj = -1;
                    for (int j = lane; j < L.M_map; j += 64) {
                        const double *S = L.map_cov + 4 * (size_t)j;
                        const float ex = L.map_xy[2 * j] - gx, ey = L.map_xy[2 * j + 1] - gy;
                        const double dx = (double)ex, dy = (double)ey;
                        const double t0 = dx * S[0] + dy * S[2];
                        const double t1 = dx * S[1] + dy * S[3];
                        const double dist = sqrt(t0 * dx + t1 * dy);
                        if (dist == dist && (bj < 0 || dist < best)) { best = dist; bj = j; }
                    }
                    for (int off = 32; off > 0; off >>= 1) {
                        const double ob = __shfl_xor(best, off, 64);
                        const int oj = __shfl_xor(bj, off, 64);
                        if (oj >= 0 && (bj < 0 || ob < best || (ob == best && oj < bj))) { best = ob; bj = oj; }
                    }
                    const int hit = __shfl((bj >= 0 && best < 0.05) ? bj : -1, 0, 64);
                    if (hit >= 0) {
                        if (lane == 0) { s_kind[i] = 0; s_idx[i] = hit; }
                        continue;
                    }
                }
                double best = 0; int bj = -1;
                for (int j = lane; j < M; j += 64) {
                    const float lx = (float)s_mu[3 + 2 * j], ly = (float)s_mu[4 + 2 * j];
                    const float ex = gx - lx, ey = gy - ly;
                    const double dx = (double)ex, dy = (double)ey;
                    const double dist = sqrt(dx * dx + dy * dy);
                    if (bj < 0 || dist < best) { best = dist; bj = j; }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const double ob = __shfl_xor(best, off, 64);
                    const int oj = __shfl_xor(bj, off, 64);
                    if (oj >= 0 && (bj < 0 || ob < best || (ob == best && oj < bj))) { best = ob; bj = oj; }
                }
                if (lane == 0) { s_kind[i] = (bj >= 0 && best < 0.6) ? 1 : 2; s_idx[i] = bj; }
            }
        }
        __syncthreads();
        if (tid == 0) {                                   // the narrow kernel's record order: state pairs, map pairs, new ids
            int ns = 0, nn = 0;
            const int room = (d.n_max - n) / 2;
            bool over = false;
            for (int i = 0; i < K; ++i) {
                if (s_kind[i] == 1) { s_pairs[2 * ns] = i; s_pairs[2 * ns + 1] = s_idx[i]; ++ns; }
                else if (s_kind[i] == 0) continue;
                else if (nn < room) s_new[nn++] = i;
                else over = true;
            }
            if (over) s_flags |= REKF_FLAG_CAPACITY;
            s_cnt[0] = ns; s_cnt[1] = nn;
            int nm = 0;
            for (int i = 0; i < K; ++i)
                if (s_kind[i] == 0) { s_pairs[2 * (ns + nm)] = i; s_pairs[2 * (ns + nm) + 1] = s_idx[i]; ++nm; }
            s_cntm = nm;
        }
        __syncthreads();
        const int NS = s_cnt[0];
        const int MM = NS + s_cntm, N2 = s_cnt[1];
        rec_ns = NS; rec_nn = N2; rec_nm = MM - NS;
        const bool fix_first = use_map && fix_off >= 0 && MM > 0;
        const int n_blocks = (MM + FLEET_BLOCK_PAIRS - 1) / FLEET_BLOCK_PAIRS;       // exactly these steps, no empty one
        const bool lin0 = fix_first || n_blocks > 1;                                  // rows are linearised at s_mu0, not at s_mu
        const int n16 = (n + 15) & ~15;

        if (MM > 0) {
            if (lin0) {
                for (int i = tid; i < n; i += RFLEET_THREADS) s_mu0[i] = s_mu[i];
                if (fix_first && tid < 3) s_p0[tid] = s_mu[tid];
                __syncthreads();
            }
            if (fix_first) {
#define FLEET_POSE_PHASE
#define FLEET_POSE_WRAP false
#include "fleet_kernels.hip"
#undef FLEET_POSE_PHASE
#undef FLEET_POSE_WRAP
            }
            for (int blk = 0; blk < n_blocks; ++blk) {
                const int base = blk * FLEET_BLOCK_PAIRS;                             // the block's first pair, GLOBAL index
                const int MMb = (MM - base) < FLEET_BLOCK_PAIRS ? (MM - base) : FLEET_BLOCK_PAIRS;
                const int m = 2 * MMb;
                const int NSb = NS - base;                                            // rows [0, 2 NSb) of this block are state rows
                const bool last = blk == n_blocks - 1;
                const bool correct = fix_first || blk > 0;                            // something has moved the mean off s_mu0
                // ---- C: H rows, W = P H^T, S = H W + Q (cc:246-305)
                if (tid < MMb) {
#pragma clang fp contract(off)
                    const int i = tid, local_id = s_pairs[2 * (base + i)], gid = s_pairs[2 * (base + i) + 1];
                    const double c = s_cs[0], s = s_cs[1];
                    double dx, dy;
                    int col = 3 + 2 * gid;
                    const double *mu_l = lin0 ? s_mu0 : s_mu;
                    if (i >= NSb) {
                        dx = (double)L.map_xy[2 * gid] - mu_l[0]; dy = (double)L.map_xy[2 * gid + 1] - mu_l[1];
                        col = 0;
                    } else { dx = mu_l[3 + 2 * gid] - mu_l[0]; dy = mu_l[4 + 2 * gid] - mu_l[1]; }
                    s_dz[2 * i] = (double)s_obs[2 * local_id] - (dx * c + dy * s);
                    s_dz[2 * i + 1] = (double)s_obs[2 * local_id + 1] - (-dx * s + dy * c);
                    for (int rr = 0; rr < 2; ++rr) {
                        int *hc = s_hc[2 * i + rr];
                        hc[0] = 0; hc[1] = 1; hc[2] = 2; hc[3] = col; hc[4] = col + 1;
                    }
                    double *h0 = s_hv[2 * i], *h1 = s_hv[2 * i + 1];
                    h0[0] = -c; h0[1] = -s; h0[2] = -dx * s + dy * c; h0[3] = c;  h0[4] = s;
                    h1[0] = s;  h1[1] = -c; h1[2] = -dx * c - dy * s; h1[3] = -s; h1[4] = c;
                    if (correct) {                                                    // the innovation against what has moved
                        const int nq = i < NSb ? 5 : 3;
                        double a0 = 0, a1 = 0;
                        for (int q = 0; q < nq; ++q) {
                            const int cq = s_hc[2 * i][q];
                            const double dm = s_mu[cq] - s_mu0[cq];
                            a0 += h0[q] * dm; a1 += h1[q] * dm;
                        }
                        s_dz[2 * i] -= a0; s_dz[2 * i + 1] -= a1;
                    }
                }
                if (FIX) {
                    if (fix_off >= 0 && blk == 0 && tid >= 64 && tid < 67) s_p0[tid - 64] = s_mu[tid - 64];
                }
                __syncthreads();
                const int m16 = (m + 15) & ~15, m4 = (m + 3) & ~3;
                for (int idx = tid; idx < n16 * m16; idx += RFLEET_THREADS) {
#pragma clang fp contract(off)
                    const int j = idx / n16, r = idx - j * n16;
                    double v = 0;
                    if (r < n && j < m) {
                        const int nq = j < 2 * NSb ? 5 : 3;
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
                        const int nq = i < 2 * NSb ? 5 : 3;
                        for (int q = 0; q < nq; ++q) v += s_hv[i][q] * W[s_hc[i][q] + j * ld];
                        if (i == j) v += opt.obs_cov;
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
                // ---- E: K = W S^-1, mean update (cc:306-307)
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
                if (tid == 0 && last && (!FIX || fix_off < 0 || fix_first)) {         // ONE wrap, behind the last block
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
            }
            // ---- P: the pose fix behind the last block (a plain member), on mu = s_mu (heading not yet wrapped) and P as they stand
            if (FIX) if (fix_off >= 0 && !fix_first) {
#define FLEET_POSE_PHASE
#define FLEET_POSE_WRAP true
#include "fleet_kernels.hip"
#undef FLEET_POSE_PHASE
#undef FLEET_POSE_WRAP
            }
        }

        // ---- G: augmentation (cc:311-364), once, over all new observations
        if (N2 > 0) {
            {
#pragma clang fp contract(off)
                if (tid == 0) {
                    rekf_sincos(s_mu[2], &s_cs[1], &s_cs[0]);
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) s_Sxi[i * 3 + j] = rekf_plower(P, (int)ld, i, j);
                }
                __syncthreads();
                const double c = s_cs[0], s = s_cs[1];
                if (tid < N2) {
                    const int local_id = s_new[tid];
                    const float fx = s_obs[2 * local_id], fy = s_obs[2 * local_id + 1];
                    float gx, gy;
                    fleet_obs_to_global(s_mu[0], s_mu[1], c, s, fx, fy, gx, gy);
                    s_mu[n + 2 * tid] = (double)gx;
                    s_mu[n + 2 * tid + 1] = (double)gy;
                    const double rx = (double)fx, ry = (double)fy;
                    s_Gp[tid][0] = 1.; s_Gp[tid][1] = 0.; s_Gp[tid][2] = -rx * s - ry * c;
                    s_Gp[tid][3] = 0.; s_Gp[tid][4] = 1.; s_Gp[tid][5] = rx * c - ry * s;
                }
                if (tid == 64) {
                    const double q = opt.obs_cov;
                    s_RQR[0] = c * q * c + (-s) * q * (-s); s_RQR[1] = c * q * s + (-s) * q * c;
                    s_RQR[2] = s * q * c + c * q * (-s);    s_RQR[3] = s * q * s + c * q * c;
                }
            }
            __syncthreads();
            for (int idx = tid; idx < n * N2; idx += RFLEET_THREADS) {
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
            for (int idx = tid; idx < N2 * N2; idx += RFLEET_THREADS) {
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
            n += 2 * N2;
            __syncthreads();
        }
        if (TRACK) fleet_track_write(L.track + e, s_trk, s_mu, P, (int)ld, n, &s_flags, rec_ns, rec_nn, rec_nm);
    }

    // ---- the member's state, the wide record and the host slot
    __syncthreads();
    for (int i = tid; i < n; i += RFLEET_THREADS) mu_g[i] = s_mu[i];
    FleetPoseSlot *slot = d.pose + mem;
    if (tid < 3) slot->mu3[tid] = s_mu[tid];
    else if (tid < 12) slot->C9[tid - 3] = rekf_plower(P, (int)ld, (tid - 3) % 3, (tid - 3) / 3);
    else if (tid == 12) { slot->n = n; slot->flags = s_flags; ctl->n = n; ctl->flags = s_flags; }
    if (rec_new) {
        FleetWideRec *rec = wrec + mem;
        if (tid == 13) { rec->K = recK; rec->n_state = rec_ns; rec->n_map = rec_nm; rec->n_new = rec_nn; }
        for (int i = tid; i < 2 * rec_ns; i += RFLEET_THREADS) rec->state_pairs[i] = s_pairs[i];
        for (int i = tid; i < 2 * rec_nm; i += RFLEET_THREADS) rec->map_pairs[i] = s_pairs[2 * rec_ns + i];
        for (int i = tid; i < rec_nn; i += RFLEET_THREADS) rec->new_ids[i] = s_new[i];
    }
}

hipError_t rfleet_launch_step_wide(const FleetDev &d, const FleetLaunch &l, FleetWideRec *wrec, hipStream_t s)
{
    if (l.G <= 0) return hipSuccess;
    if (!wrec) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fleet_step_wide, dim3((unsigned)l.G), dim3(RFLEET_THREADS), 0, s, d, l, wrec);
    return hipGetLastError();
}
