// fleet_reflectors.hip -- k_fleet_reflectors: what the node publishes of the filter after a scan (src/ros_node.cc:736-791 marker
// ellipses, :75-140 the saved reflector map), for any list of members of a fleet in ONE launch and without a copy of any
// covariance matrix.
//
// One workgroup per listed member, one lane per reflector (at most 128: two waves).  Lane i reads its reflector's 2 x 2 block from
// the member's LOWER triangle and its mean, and writes up to three compact outputs into pinned host memory, which the end of the
// launch publishes (as FleetPoseSlot): a member's rows follow those of the member listed before it.  Each workgroup finds its own
// first row by summing the reflector counts of the members listed in front of it (ctl[m].n: a few hundred ints from L2), so no
// workgroup waits for another, there is no atomic, no host-side prefix and nothing to clear.
//
// The ellipse arithmetic is k_ellipses' (ekf_kernels.hip), restated operation for operation: the single filter's sources are
// pinned by content, so the text cannot be shared; tests/test_fleet_reflectors_gpu.py holds the two to the same bits.
#include "fleet_reflectors.h"

__device__ __forceinline__ int fleet_reflectors_of(const FleetDev &d, int mem)
{
    int L = (d.ctl[mem].n - 3) / 2;
    const int L_max = (d.n_max - 3) / 2;
    L = L < 0 ? 0 : L;
    return L > L_max ? L_max : L;                       // (never true for a state the fleet's own kernels wrote: keeps every store inside the buffers)
}

__global__ __launch_bounds__(RFLEET_REFLECTOR_THREADS) void k_fleet_reflectors(FleetDev d, FleetReflectorsLaunch L)
{
#pragma clang fp contract(off)
    __shared__ int s_part[RFLEET_REFLECTOR_THREADS / 64];
    __shared__ double s_ell[5 * RFLEET_REFLECTOR_THREADS];
    const int tid = threadIdx.x;
    const int g = blockIdx.x;
    if (g >= L.count) return;

    // ---- the first row of this member: the reflectors of the members listed in front of it
    int acc = 0;
    for (int j = tid; j < g; j += RFLEET_REFLECTOR_THREADS) acc += fleet_reflectors_of(d, L.members ? L.members[j] : j);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    long off = 0;
    for (int w = 0; w < RFLEET_REFLECTOR_THREADS / 64; ++w) off += s_part[w];

    const int mem = L.members ? L.members[g] : g;
    const int Lm = fleet_reflectors_of(d, mem);
    if (tid == 0) L.counts[g] = Lm;
    if (Lm == 0) return;

    const size_t ld = (size_t)d.ld;
    const double *P = d.P + (size_t)mem * ld * ld;
    const double *mu = d.mu + (size_t)mem * ld;
    const bool live = tid < Lm;
    const long row = off + tid;
    if (live) {
        const int id = 3 + 2 * tid;
        const double a = P[id + id * ld], c = P[(id + 1) + id * ld], dd = P[(id + 1) + (id + 1) * ld];
        const double b = c;                               // sigma(id, id+1): P is stored as its lower triangle
        const double mx = mu[id], my = mu[id + 1];
        if (row < L.cap_rows) {
            if (L.xy2) { L.xy2[2 * row] = mx; L.xy2[2 * row + 1] = my; }
            if (L.cov4) { L.cov4[4 * row] = a; L.cov4[4 * row + 1] = b; L.cov4[4 * row + 2] = c; L.cov4[4 * row + 3] = dd; }
        }
        if (L.ell5) {
            // Eigen 3.3's RealSchur on the 2 x 2 block T = [[a, b], [c, d]] (k_ellipses: src/ros_node.cc:759-761)
            double d0, d1, vx, vy;
            if (fabs(c) <= 2.220446049250313e-16 * (fabs(a) + fabs(dd))) {
                d0 = a; d1 = dd; vx = 1.0; vy = 0.0;
            } else {
                const double p = 0.5 * (a - dd);
                const double q = p * p + c * b;
                const double z = sqrt(fabs(q));
                const double pz = (p >= 0.0) ? p + z : p - z;
                d0 = dd + pz;
                d1 = (pz != 0.0) ? dd - c * b / pz : d0;
                vx = pz; vy = c;
            }
            double *o = s_ell + 5 * tid;
            o[0] = mx;
            o[1] = my;
            o[2] = atan2(vy, vx);
            o[3] = 2.0 * sqrt(d0 * 5.991);
            o[4] = 2.0 * sqrt(d1 * 5.991);
        }
    }
    if (L.ell5) {                                         // five doubles per lane: through LDS, so that consecutive lanes store consecutive addresses
        __syncthreads();
        double *out = L.ell5 + 5 * off;
        for (int k = tid; k < 5 * Lm; k += RFLEET_REFLECTOR_THREADS)
            if (off + k / 5 < L.cap_rows) out[k] = s_ell[k];
    }
}

hipError_t rfleet_launch_reflectors(const FleetDev &d, const FleetReflectorsLaunch &l, hipStream_t s)
{
    if (l.count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fleet_reflectors, dim3((unsigned)l.count), dim3(RFLEET_REFLECTOR_THREADS), 0, s, d, l);
    return hipGetLastError();
}
