// fleet_snapshot.hip -- k_fleet_pack / k_fleet_unpack: the full states of any list of members of a fleet between the members' device
// arrays and ONE contiguous staging buffer, in ONE launch each (rfleet_snapshot / rfleet_restore, include/rfleet.h).
//
// A member's payload is mu[0:n] followed by the packed lower triangle of P[0:n, 0:n], column-major: column j holds rows j .. n-1, so
// it starts at j n - j (j - 1) / 2 doubles into the triangle.  The grid is a host-built table of (listed member, panel of 16 columns)
// records: a workgroup reads its record and nothing of any other workgroup, so none waits for another and nothing is atomic.  Inside
// a panel wave w takes columns w, w + 4, ... and its lanes walk the rows of the column: the run P[j + j ld .. n-1 + j ld] in the
// member's array and the column's run in the payload are both contiguous, lane k of a wave at double k, so every load and store is
// one coalesced 512-byte access per wave (8 bytes per lane: a packed column starts at any multiple of 8, which rules out wider ones).
// Panel 0's workgroup also moves mu; in the unpack it also writes n, the flags and the cleared match record of FleetMemberCtl.
//
// The unpack walks the panels of the TARGET's ld = roundup(n_max, 16) and writes zeros where the payload has nothing: mu[n:ld] and
// every lower-triangle entry with a row or column index >= n, which is what rfleet_create left there and no step kernel writes.
// The staging buffer is ordinary device memory and every store is a plain vector store.  member ld ld is formed in size_t.
#include "fleet_snapshot.h"

// the record as the host built it, refused whole when it does not fit this fleet or the buffer (never true for a table of
// rfleet_api.hip: keeps every load and store inside the arrays)
__device__ __forceinline__ bool fleet_snap_rec_ok(const FleetDev &d, const FleetSnapLaunch &L, const FleetSnapRec &r)
{
    if (r.member < 0 || r.member >= d.B || r.n < 3 || r.n > d.n_max || r.panel < 0 || r.panel >= d.ld / RFLEET_SNAP_PANEL || r.off < 0 || r.off > L.cap)
        return false;
    const long n = r.n;
    return r.off + n + n * (n + 1) / 2 <= L.cap;
}

__global__ __launch_bounds__(RFLEET_SNAP_THREADS) void k_fleet_pack(FleetDev d, FleetSnapLaunch L)
{
    if ((int)blockIdx.x >= L.count) return;
    const FleetSnapRec r = L.rec[blockIdx.x];
    if (!fleet_snap_rec_ok(d, L, r)) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = r.n;
    const size_t ld = (size_t)d.ld;
    const double *P = d.P + (size_t)r.member * ld * ld;
    double *out = L.buf + r.off;
    if (r.panel == 0) {
        const double *mu = d.mu + (size_t)r.member * ld;
        for (int i = tid; i < n; i += RFLEET_SNAP_THREADS) out[i] = mu[i];
    }
    double *tri = out + n;
    for (int c = wave; c < RFLEET_SNAP_PANEL; c += RFLEET_SNAP_THREADS / 64) {
        const int j = r.panel * RFLEET_SNAP_PANEL + c;
        if (j >= n) break;
        const double *src = P + (size_t)j + (size_t)j * ld;
        double *dst = tri + ((long)j * n - (long)j * (j - 1) / 2);
        for (int k = lane; k < n - j; k += 64) dst[k] = src[k];
    }
}

__global__ __launch_bounds__(RFLEET_SNAP_THREADS) void k_fleet_unpack(FleetDev d, FleetSnapLaunch L)
{
    if ((int)blockIdx.x >= L.count) return;
    const FleetSnapRec r = L.rec[blockIdx.x];
    if (!fleet_snap_rec_ok(d, L, r)) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = r.n;
    const int ldi = d.ld;
    const size_t ld = (size_t)ldi;
    double *P = d.P + (size_t)r.member * ld * ld;
    const double *in = L.buf + r.off;
    if (r.panel == 0) {
        double *mu = d.mu + (size_t)r.member * ld;
        for (int i = tid; i < ldi; i += RFLEET_SNAP_THREADS) mu[i] = i < n ? in[i] : 0.0;
        if (tid == 0) {                                   // the member's record as at rfleet_create: all counts zero
            FleetMemberCtl &c = d.ctl[r.member];
            c.n = n;
            c.flags = r.flags;
            c.K = 0; c.n_state = 0; c.n_new = 0; c.n_map = 0;
        }
    }
    const double *tri = in + n;
    for (int c = wave; c < RFLEET_SNAP_PANEL; c += RFLEET_SNAP_THREADS / 64) {
        const int j = r.panel * RFLEET_SNAP_PANEL + c;
        if (j >= ldi) break;
        double *dst = P + (size_t)j + (size_t)j * ld;      // rows j .. ld-1 of column j
        const int have = j < n ? n - j : 0;                // rows the payload holds of this column
        const double *src = tri + ((long)j * n - (long)j * (j - 1) / 2);    // (not read when have == 0)
        for (int k = lane; k < ldi - j; k += 64) dst[k] = k < have ? src[k] : 0.0;
    }
}

hipError_t rfleet_launch_pack(const FleetDev &d, const FleetSnapLaunch &l, hipStream_t s)
{
    if (l.count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fleet_pack, dim3((unsigned)l.count), dim3(RFLEET_SNAP_THREADS), 0, s, d, l);
    return hipGetLastError();
}

hipError_t rfleet_launch_unpack(const FleetDev &d, const FleetSnapLaunch &l, hipStream_t s)
{
    if (l.count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fleet_unpack, dim3((unsigned)l.count), dim3(RFLEET_SNAP_THREADS), 0, s, d, l);
    return hipGetLastError();
}
