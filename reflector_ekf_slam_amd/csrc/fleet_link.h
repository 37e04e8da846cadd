// fleet_link.h -- what the host side of a linked submit (fleet_host.h, rfleet_api.hip) and k_fleet_bind (fleet_link.hip) share: the
// table a bind launch walks, the status record it leaves, and the ONE taking rule, compiled for host and device (tests/cpp/
// fleet_link_host.cpp runs this text without a GPU).
//
// A linked scan (RFLEET_EV_SCAN_LINKED of rfleet.h) is a scan whose observations are still being detected when the filter's submit
// is packed: the host knows its member, stamp and dt, and reserves 2 * max_obs floats of the segment's obs area for it, with K = 0
// in its FleetEvent.  In front of the step launch one workgroup of k_fleet_bind per such scan reads K and err from the detector's
// record (include/rlink.h), decides how many centres are taken, copies them into the reserved range, stores the count into the
// FleetEvent and tells the host what it did.  A scan that is not taken stays the empty scan the host packed: a Predict to its stamp.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define FLEET_LINK_HD __host__ __device__
#else
#define FLEET_LINK_HD
#endif

// the two codes the rule may hand out beside a record's own err (rdet.h's RDET_ERR_CAPACITY, rekf.h's REKF_ERR_TOO_MANY_OBS: neither
// header is included here; fleet_host.h holds the second against rekf.h)
#define FLEET_LINK_ERR_CAPACITY (-4)
#define FLEET_LINK_ERR_TOO_MANY_OBS (-3)

// one linked scan that has a record: which packed event it is, where its reserved floats start, which record, which status slot
struct FleetBindRec {
    int ev_at;               // index into the segment's FleetEvent[E]
    int obs_off;             // index of the first reserved float in the segment's obs area
    int record;              // the detector's output record
    int slot;                // index into the status records: the scan's position among the call's linked scans
};

// what a bind leaves for the host per linked scan, in pinned host memory
struct FleetLinkStatus {
    int taken;               // centres handed to the step kernel
    int status;              // 0, the record's err, FLEET_LINK_ERR_CAPACITY or FLEET_LINK_ERR_TOO_MANY_OBS
    int K_seen;              // K as read from the record
    int pad_;
};

// The taking rule, K and err read once from the record:
//   err != 0                         -> status err,                          taken 0
//   K < 0 || K > max_centers         -> status FLEET_LINK_ERR_CAPACITY,      taken 0
//   K > max_obs                      -> status FLEET_LINK_ERR_TOO_MANY_OBS,  taken 0
//   otherwise                        -> status 0,                            taken K
FLEET_LINK_HD inline int fleet_link_take(int K, int err, int max_centers, int max_obs, int *status)
{
    if (err != 0) { *status = err; return 0; }
    if (K < 0 || K > max_centers) { *status = FLEET_LINK_ERR_CAPACITY; return 0; }
    if (K > max_obs) { *status = FLEET_LINK_ERR_TOO_MANY_OBS; return 0; }
    *status = 0;
    return K;
}

#if defined(__HIPCC__) || defined(__HIP__)
struct FleetEvent;

struct FleetBindLaunch {     // one launch of k_fleet_bind: n_bind workgroups of 64 lanes
    const FleetBindRec *bind;           // [n_bind], in the call's ring segment
    FleetEvent *ev;                     // the segment's FleetEvent[E]
    float *obs;                         // the segment's obs area
    FleetLinkStatus *status;            // [linked scans of the call], pinned host memory
    const char *records;                // rlink::records
    long record_bytes;
    int k_off, err_off, centers_off, max_centers;
    int max_obs;                        // floats / 2 reserved per linked scan
    int n_bind;
};

hipError_t rfleet_launch_bind(const FleetBindLaunch &l, hipStream_t s);
#endif
