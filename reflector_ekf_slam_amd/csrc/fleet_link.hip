// fleet_link.hip -- k_fleet_bind: the hand-over of a fleet detector's centres to the fleet filter on the device (rfleet_submit_linked,
// include/rfleet.h; the protocol and the taking rule: fleet_link.h, include/rlink.h).
//
// The launch sits on the fleet's stream behind hipStreamWaitEvent(ready) and in front of the step launch of the same submit.  One
// workgroup of ONE wave per linked scan that has a record: it reads K and err from the detector's record once, applies
// fleet_link_take, and its lanes copy the `taken` centres into the range of the segment's obs area the host reserved for the scan --
// lane k moves pairs k, k + 64, ...: 8 bytes a lane, one coalesced 512-byte access a wave.  Lane 0 then stores `taken` into the
// scan's FleetEvent::K, which the host packed as 0, and {taken, status, K as read} into the scan's status record.  The step kernel
// that follows on the stream reads the event and the observations from the segment exactly as if the host had packed them.
//
// A workgroup reads its own table row and its own record and writes its own event, range and status record: no workgroup waits for
// another, nothing is atomic, there is no LDS.  Source and destination are pinned host memory; every store is a plain vector store.
// taken <= max_obs (the floats reserved) and taken <= max_centers (the pairs a record holds) by the rule itself: no access leaves
// either range whatever a record holds.
#include "fleet_dev.h"
#include "fleet_link.h"

__global__ __launch_bounds__(64) void k_fleet_bind(FleetBindLaunch L)
{
    if ((int)blockIdx.x >= L.n_bind) return;
    const FleetBindRec r = L.bind[blockIdx.x];
    const char *rec = L.records + (size_t)r.record * (size_t)L.record_bytes;
    const int K = *reinterpret_cast<const int *>(rec + L.k_off), err = *reinterpret_cast<const int *>(rec + L.err_off);
    int status;
    const int taken = fleet_link_take(K, err, L.max_centers, L.max_obs, &status);
    const float2 *__restrict__ src = reinterpret_cast<const float2 *>(rec + L.centers_off);
    float2 *__restrict__ dst = reinterpret_cast<float2 *>(L.obs + r.obs_off);      // (obs_off is even, the area 16-byte aligned)
    for (int k = threadIdx.x; k < taken; k += 64) dst[k] = src[k];
    if (threadIdx.x == 0) {
        L.ev[r.ev_at].K = taken;
        FleetLinkStatus st;
        st.taken = taken; st.status = status; st.K_seen = K; st.pad_ = 0;
        L.status[r.slot] = st;
    }
}

hipError_t rfleet_launch_bind(const FleetBindLaunch &l, hipStream_t s)
{
    if (l.n_bind <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fleet_bind, dim3((unsigned)l.n_bind), dim3(64), 0, s, l);
    return hipGetLastError();
}
