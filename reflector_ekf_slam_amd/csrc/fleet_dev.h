// fleet_dev.h -- device-side layout shared by the fleet kernel (fleet_kernels.hip) and its C-ABI host (rfleet_api.hip).
//
// A fleet is B independent small filters (n <= 259) advanced by ONE launch per rfleet_submit: one workgroup per member
// with events in the call.  Per member, sized once at rfleet_create for n_max = 3 + 2 max_landmarks:
//
//   mu  [ld]             state mean
//   P   [ld x ld]        covariance, column-major, LOWER TRIANGLE valid (as ekf_dev.h), ld = roundup(n_max, 16): a C2-sized member
//                        has 0.59 MB of covariance instead of the single filter's 0.82 MB (ld = roundup(n_max, 64))
//   W   [ld x 64]        W = P H^T = (H P)^T of the current scan (P is exactly symmetric), column-major; rows [n, roundup(n, 16))
//                        and columns [m, roundup(m, 16)) are written as zeros, nothing beyond them is read
//   Kn  [ld x 64]        K = W S^-1, same shape and padding
//   ctl                  FleetMemberCtl: n, sticky flags, the last scan's ReflectorMatchResult
// and per FLEET, shared by its members (rfleet_set_map): the pre-loaded reflector map, M_ points as float32 (x, y) and M_ row-major
// 2 x 2 FP64 weights, read from global memory by every workgroup of k_fleet_step_map (<= 80 KB: it stays in L2), and one byte per
// member that says whether the member matches against it.
// W and Kn are scratch of the member's own workgroup: written and read inside one launch by that workgroup only.
// Time and the last odometry velocity live on the HOST (rfleet_api.hip): an event arrives with its dt and velocity.
#pragma once
#include "ekf_dev.h"

#define RFLEET_MAX_OBS_DEV 32
#define RFLEET_MAX_OBS_WIDE_DEV 256       // k_fleet_step_wide (fleet_wide.hip): observations of a wide scan
#define RFLEET_MAX_NEW_WIDE_DEV 128       // ... and what it can append at once: (n_max - 3) / 2 at most
#define RFLEET_PANEL_COLS 64
#define RFLEET_THREADS 512

struct FleetEvent {          // one Predict (+ scan) of one member, as the host packs it into the staging ring
    double dt;               // t - state time
    double vt[3];            // vt_ this Predict uses
    int kind;                // 0 odometry (Predict only), 1 scan, 2 (tracked launches only) a message the host dropped: no Predict, a record
    int K;                   // observations (scan)
    int obs_off;             // index of the scan's first float in FleetLaunch::obs
    int fix_off;             // index of the scan's pose fix (x, y, yaw) in FleetLaunch::fix, -1: the scan has none
};

struct FleetMemberCtl {
    int n;                   // state dimension 3 + 2 L
    int flags;               // sticky REKF_FLAG_*
    int K, n_state, n_new;   // the last scan's record
    int n_map;               // written by k_fleet_step_map only: the host knows which kernel wrote a member's last record
    int pad_[2];
    int state_pairs[2 * RFLEET_MAX_OBS_DEV];
    int new_ids[RFLEET_MAX_OBS_DEV];
    int map_pairs[2 * RFLEET_MAX_OBS_DEV];    // (observation, map point), k_fleet_step_map only
};

// The match record of a member whose last scan went through a WIDE launch (k_fleet_step_wide), narrow scans of that launch included:
// a device array of its own [B], allocated by rfleet_set_wide_scans.  FleetMemberCtl keeps its layout; the host remembers per
// member which kind of launch wrote its last record.
struct FleetWideRec {
    int K, n_state, n_map, n_new;
    int state_pairs[2 * RFLEET_MAX_OBS_WIDE_DEV];
    int map_pairs[2 * RFLEET_MAX_OBS_WIDE_DEV];
    int new_ids[RFLEET_MAX_OBS_WIDE_DEV];
};

struct FleetMemberOpt { double lin_cov, ang_cov, obs_cov; int model; int pad_; };

// what a launch leaves for the host in pinned memory, per member: read after a stream synchronisation, no copy of the state
struct FleetPoseSlot { double mu3[3]; double C9[9]; int n; int flags; double pad_[3]; };

// what a TRACKED launch leaves per packed event, in the launch's own ring segment (pinned host memory): the slot's content as it
// would be if the launch ended behind that event, and the scan's match counts (zero for odometry).  One 128-byte line per event.
struct alignas(128) FleetTrackRec {
    double mu3[3]; double C9[9];
    int n, flags;
    int n_state, n_new, n_map;
    int pad_[3];
};
static_assert(sizeof(FleetTrackRec) == 128, "one record is one 128-byte line");

struct FleetDev {
    double *mu;              // [B][ld]
    double *P;               // [B][ld * ld]
    double *W, *Kn;          // [B][ld * RFLEET_PANEL_COLS]
    FleetMemberCtl *ctl;     // [B]
    const FleetMemberOpt *opt;   // [B]
    FleetPoseSlot *pose;     // [B], pinned host memory
    int ld, n_max, B, pad_;
};

struct FleetLaunch {         // one rfleet_submit: G members with events, member members[g] owns events [ev_begin[g], ev_begin[g + 1])
    const int *members;
    const int *ev_begin;
    const FleetEvent *ev;
    const float *obs;
    const double *fix;       // the pose fixes of the call's scans, three doubles each; NULL when no scan of the call has one
    int G, pad_;
    // the shared map (k_fleet_step_map only; behind everything else, so that no argument of the other two kernels moves)
    const float *map_xy;     // [M_map][2]
    const double *map_cov;   // [M_map][4], row-major 2 x 2
    const unsigned char *map_use;   // [B]: non-zero = the member matches against the map
    int M_map, pad2_;        // M_map > 0 selects k_fleet_step_map
    // the pose track (k_fleet_step_track only; appended the same way)
    FleetTrackRec *track;    // [events of the call]: event e writes track[e]; non-NULL selects k_fleet_step_track
};

hipError_t rfleet_launch_step(const FleetDev &d, const FleetLaunch &l, hipStream_t s);
// a submit that holds a scan wider than RFLEET_MAX_OBS_DEV: k_fleet_step_wide, whatever l.fix, l.M_map and l.track say (fleet_wide.hip)
hipError_t rfleet_launch_step_wide(const FleetDev &d, const FleetLaunch &l, FleetWideRec *wrec, hipStream_t s);

// ---- what the step kernels of fleet_kernels.hip and fleet_wide.hip share on the device
typedef double v4d __attribute__((ext_vector_type(4)));

#define FLEET_SLD 65             // row stride of S in LDS (odd: a column walk touches every bank)
#define FLEET_LD_MAX 272         // roundup(3 + 2 * 128, 16)

__device__ static inline void fleet_obs_to_global(double x, double y, double c, double s, float px, float py, float &gx, float &gy)
{
#pragma clang fp contract(off)
    // cc:389-393 / :327-331: evaluated in double, rounded to float32 on assignment
    gx = (float)((double)px * c - (double)py * s + x);
    gy = (float)((double)px * s + (double)py * c + y);
}

// gps.cc:320-328: the yaw difference as quaternion (w, 0, 0, z) -> angle-axis z (reference transform.h:46-70)
__device__ static inline double fleet_yaw_innovation(double delta_theta)
{
#pragma clang fp contract(off)
    double w = cos(delta_theta / 2), z = sin(delta_theta / 2);
    const double nrm = sqrt(w * w + z * z);
    w /= nrm; z /= nrm;
    if (w < 0.) { w = -w; z = -z; }
    const double angle = 2. * atan2(fabs(z), w);
    const double scale = angle < 1e-7 ? 2. : angle / sin(angle / 2.);
    return scale * z;
}

// One event's record of a tracked launch: the pose, the pose block of the lower triangle, n, the flags and the scan's match counts,
// staged in LDS and stored by lanes 0-15 of wave 0, 8 bytes each: ONE 128-byte line of the launch's ring segment in pinned host
// memory.  The host sized the area for one record per packed event, so nothing counts and nothing can overflow.  The leading barrier
// orders the reads behind the event's last write to s_mu, s_flags and P's corner (whichever phase that was); the next pass has
// barriers of its own before anything here is staged again.
__device__ static inline void fleet_track_write(FleetTrackRec *rec, double *s_trk, const double *s_mu, const double *P, int ld, int n,
                                                const int *s_flags, int n_state, int n_new, int n_map)
{
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < 3) s_trk[tid] = s_mu[tid];
    else if (tid < 12) s_trk[tid] = rekf_plower(P, ld, (tid - 3) % 3, (tid - 3) / 3);
    else if (tid == 12) {
        int *q = (int *)(s_trk + 12);                       // FleetTrackRec's integers, in its order
        q[0] = n; q[1] = *s_flags; q[2] = n_state; q[3] = n_new; q[4] = n_map; q[5] = 0; q[6] = 0; q[7] = 0;
    }
    __syncthreads();
    if (tid < 16) ((double *)rec)[tid] = s_trk[tid];
}
