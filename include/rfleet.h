/*
 * rfleet.h -- C ABI of the fleet filter (librfleet.so): many small reflector EKF-SLAM sessions advanced by ONE kernel
 * launch per call.
 *
 * rekf.h serves one large filter per handle.  A fleet host (one hall, many AGVs, each with a few dozen to ~100 reflectors
 * in its own map) hands over this tick's messages of ALL robots in one rfleet_submit and reads all poses back: each member
 * with events in the call is advanced by one workgroup of one launch (csrc/fleet_kernels.hip), whatever the number of members.
 *
 * Per member the semantics are the single filter's (reference reflector_ekf_slam.cc): Predict (DIFF / OMNI), ReflectorMatch's
 * map and state branches, the joint EKF update, landmark augmentation, and the odometry quirks (a message with t < state time is
 * dropped, use_imu ignores odometry, an empty scan is a Predict).
 *
 * Conventions: as rekf.h -- opaque handle, one HIP stream per handle, NOT thread-safe, caller-owned host buffers borrowed
 * for the duration of the call, 0 or a negative REKF_ERR_* code, nothing calls exit().  rekf_options, the REKF_ERR_* codes
 * and the REKF_FLAGBIT_* bits are rekf.h's.
 *
 * Capacity is fixed at rfleet_create (max_landmarks <= RFLEET_MAX_LANDMARKS, else REKF_ERR_UNSUPPORTED).  A member that
 * outgrows it drops the extra reflectors of a scan -- the first (n_max - n) / 2 new observations, in observation order, are
 * appended -- and raises its OWN sticky REKF_FLAGBIT_CAPACITY, like a rekf_create handle without auto-grow.
 *
 * The USE_GPS deployment (reference reflector_ekf_slam_gps.cc:305-340, src/ros_node.cc:450-478) is served per member: a scan
 * event may carry an absolute pose fix (x, y, yaw), which rides on the scan's update as three extra rows H = [I3 0] with the
 * fixed noise diag(0.05^2, 0.05^2, 0.017^2) and the reference's quaternion -> angle-axis yaw innovation; as there, the rows
 * exist only when the scan matched at least one reflector (a fix on a scan without a match, an empty one included, is
 * ignored).  rfleet_predict_poses is PredictState's pose block for every member: the pose a scan matcher starts from.
 *
 * The localisation deployment (LoadMapFromTxtFile; reflector_ekf_slam.cc:401-425, :279-302) is served by ONE pre-loaded reflector
 * map per fleet, shared by its members (one hall): rfleet_set_map.  A member that uses it tries the map first (weighted distance
 * < 0.05), then its own state (< 0.6); a map-matched observation corrects the pose through rows without a landmark block.
 *
 * What the node publishes of the filter after a scan (src/ros_node.cc:736-791 ReflectorToRosMarkers' covariance ellipses, :75-140
 * SaveReflectorResult's positions and 2 x 2 blocks) is served for any list of members by ONE launch and without a copy of any
 * covariance matrix: rfleet_get_reflectors.
 *
 * What the node publishes of the pose (src/ros_node.cc:627-660, :517-545: the pose with its 3 x 3 covariance and ekf_path_ after
 * every odometry message and every scan that saw reflectors; StatePosetoRosPose :796-819) is served by the pose track: with
 * rfleet_set_tracking on, the ONE launch of an rfleet_submit also leaves a record per message -- the pose, its covariance, n, the
 * flags and the scan's match counts AFTER that message -- in pinned host memory, and rfleet_take_track hands the records over per
 * member with one synchronisation and no launch.  A message the filter drops (stale odometry, odometry of a use_imu member) gets a
 * record of the unchanged pose, as the node publishes it.
 *
 * A scan of more than RFLEET_MAX_OBS observations (an open hall, a 360 degree lidar: both fleet detectors hand over up to 256
 * centres) is served on a fleet that has called rfleet_set_wide_scans, up to RFLEET_MAX_OBS_WIDE: the scan is matched once and its
 * pairs are applied in exact block steps of 32, which equals the reference's joint update (csrc/fleet_wide.hip).  A submit that
 * holds such a scan takes one launch of a kernel of its own; every other submit launches what it always did.
 *
 * A service hands its state over and takes it back as a fleet (a checkpoint, robots that move to another fleet, yesterday's maps with
 * their full covariances): rfleet_snapshot packs the full states of any list of members -- n, flags, time, velocity, mean and the
 * covariance's lower triangle -- into one self-describing blob with ONE launch, and rfleet_restore puts a blob's entries into any
 * members of any fleet whose capacity holds them with ONE launch, zeros beyond n included (csrc/fleet_snapshot.hip).
 *
 * Deliberately OUT OF SCOPE (use a rekf handle): a map per member, a map of more than RFLEET_MAX_MAP_POINTS points, scans
 * wider than RFLEET_MAX_OBS on a fleet that has not called rfleet_set_wide_scans, wider than RFLEET_MAX_OBS_WIDE on one that has,
 * auto-grow, PredictState's landmark part (the full state).
 *
 * The covariance of a member lives on the device as its lower triangle; the getters mirror it (as rekf_get_state does).
 */
#ifndef RFLEET_H_
#define RFLEET_H_

#include "rekf.h"
#include "rlink.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RFLEET_ABI_VERSION 2
#define RFLEET_MAX_LANDMARKS 128     /* per member: n <= 259 */
#define RFLEET_MAX_OBS 32            /* per scan: one joint update, m <= 64 innovation rows */
#define RFLEET_MAX_OBS_WIDE 256      /* per scan on a fleet with rfleet_set_wide_scans on: block steps of RFLEET_MAX_OBS pairs */
#define RFLEET_MAX_MAP_POINTS 2048   /* the fleet's shared pre-loaded map */

typedef struct rfleet rfleet_t;

/* RFLEET_EV_SCAN_LINKED: a scan of rfleet_submit_linked whose observations a fleet detector's launch is still producing (below) */
enum { RFLEET_EV_ODOM = 0, RFLEET_EV_SCAN = 1, RFLEET_EV_SCAN_LINKED = 2 };

typedef struct rfleet_event {
    int member;          /* 0 .. B-1 */
    int kind;            /* RFLEET_EV_* */
    double t;
    double v[3];         /* ODOM: vx, vy, wz */
    const float *xy;     /* SCAN: K robot-frame points (x, y pairs) */
    int K;
    int has_pose_fix;    /* SCAN: non-zero = pose_fix holds an absolute pose observation of this scan's time */
    double pose_fix[3];  /* x, y, yaw (read only when has_pose_fix is set) */
} rfleet_event;

/* B members, opts[i] for member i (each starts as ReflectorEKFSLAM(opts[i]) does: n = 3, zero covariance).  B = 0,
 * max_landmarks outside 1 .. RFLEET_MAX_LANDMARKS or a null pointer are refused before any HIP call. */
int rfleet_create(const rekf_options *opts, int B, int max_landmarks, int device, rfleet_t **out);
void rfleet_destroy(rfleet_t *f);

/* Any number of events for any subset of members; a member's events are applied in the order given
 * (HandleOdometryMessage / HandleObservationMessage each).  EVERYTHING is validated first: on an error return (a member out
 * of range, an unknown kind, K < 0, K > RFLEET_MAX_OBS = REKF_ERR_TOO_MANY_OBS (K > RFLEET_MAX_OBS_WIDE with rfleet_set_wide_scans
 * on), K > 0 with a null xy, has_pose_fix on an odometry event, a non-finite component of a fix) no member has moved.
 * Packs the events into a pinned staging ring, enqueues ONE kernel launch and returns; consecutive calls do not synchronise. */
int rfleet_submit(rfleet_t *f, const rfleet_event *ev, int count);

/* All getters synchronise.  sigma3x3 / sigma are column-major. */
int rfleet_get_poses(rfleet_t *f, double *t /*[B]*/, double *mu3 /*[B][3]*/, double *sigma3x3 /*[B][9]*/);
/* PredictState's pose block (cc:97-152) of every member, from the member's state time to t[b] with its last odometry velocity:
 * the pose and 3 x 3 covariance a scan matcher starts from.  Non-mutating.  Synchronises like the getters, then evaluates on
 * the host; launches nothing.  As rekf_predict_state: t[b] before the state time gives a negative dt (no test), a use_imu
 * member's velocity is the zero it was created with.  sigma3x3 may be NULL. */
int rfleet_predict_poses(rfleet_t *f, const double *t /*[B]*/, double *mu3 /*[B][3]*/, double *sigma3x3 /*[B][9]*/);
int rfleet_get_n(rfleet_t *f, int *n /*[B]*/);
int rfleet_get_flags(rfleet_t *f, int *flags /*[B], sticky REKF_FLAGBIT_* per member, not cleared*/);
/* As rekf_get_state: mu (n) and sigma (n x n, ld = n) may each be NULL; caps in doubles (REKF_ERR_BUFFER when too small). */
int rfleet_get_state(rfleet_t *f, int member, double *t, int *n, double *mu, long mu_cap, double *sigma, long sigma_cap);
/* As rekf_set_state: only the lower triangle of sigma is used; vt3 = nullable last odometry velocity. */
int rfleet_set_state(rfleet_t *f, int member, double t, int n, const double *mu, const double *sigma, const double *vt3);
/* The member's last scan: pairs are (observation, landmark); buffers hold RFLEET_MAX_OBS entries (pairs: twice that).
 * Any pointer may be NULL.  map_pairs are (observation, map point); *n_map is 0 for a member that does not use the map.
 * When a count exceeds RFLEET_MAX_OBS (the record of a wide scan): REKF_ERR_BUFFER, the three counts written, no list touched. */
int rfleet_get_last_match(rfleet_t *f, int member, int *n_state, int *state_pairs, int *n_map, int *map_pairs, int *n_new, int *new_ids);
/* map_ as LoadMapFromTxtFile leaves it, shared by the fleet: M points (float32 xy) and M row-major 2x2 weights, as rekf_set_map.
 * use[b] != 0: member b matches against it (NULL = every member).  M = 0 clears the map.  Synchronises, replaces the device copy;
 * takes effect with the next rfleet_submit.  A null handle, M < 0, M > 0 with a null xy or cov, or a non-finite coordinate or
 * weight is REKF_ERR_INVALID, M > RFLEET_MAX_MAP_POINTS is REKF_ERR_UNSUPPORTED, both before any HIP call; a refused call
 * leaves the old map in place.  (Added without a new RFLEET_ABI_VERSION: a binding looks the two calls up by name.) */
int rfleet_set_map(rfleet_t *f, const float *xy, const double *cov, int M, const unsigned char *use /*[B], nullable*/);
int rfleet_get_map_size(rfleet_t *f, int *M);
/* The reflectors of the listed members, compact and in the order listed: counts[g] rows of members[g] follow those of members[g - 1].
 * members NULL = all B members in order (count must be B).  Each output may be NULL: ellipses5 = the marker ellipse {mx, my, angle,
 * x_len, y_len} of rekf_get_marker_ellipses (the same bits), xy2 = the reflector's mean, cov4 = its covariance block row-major
 * (a, b, c, d) with b = c, as rfleet_get_state mirrors it.  cap_rows = the rows each given output holds (with no output given
 * it is not looked at: the call returns the counts).
 * Enqueues ONE launch behind whatever rfleet_submit has enqueued and synchronises once: every event submitted before is in it.
 * counts is written on success AND with REKF_ERR_BUFFER (the rows do not fit cap_rows: no output is touched, counts sizes the
 * second call).  REKF_ERR_INVALID before any HIP call and before the handle is read: a null handle, count < 0, count > 0 with null
 * counts, cap_rows < 0, an output given with cap_rows == 0 and count > 0; after the handle is read and before any launch: a member
 * outside 0 .. B-1, a member listed twice, members NULL with count != B.  count == 0 with a list is REKF_OK and does nothing.
 * (Added without a new RFLEET_ABI_VERSION: a binding looks the call up by name.) */
int rfleet_get_reflectors(rfleet_t *f, const int *members, int count,   /* members NULL = all B, in order */
                          int *counts /*[count]*/, double *ellipses5, double *xy2, double *cov4, long cap_rows);
/* The pose track.  One record per message of a tracked rfleet_submit: the member's pose, pose covariance (column-major, as
 * rfleet_get_poses), state dimension and sticky flags AFTER that message, and for a scan its match counts (zero otherwise).  The
 * record of a member's last message of a call is what rfleet_get_poses reads behind that call, bit for bit.  dropped = 1: a message
 * the filter ignores (odometry with t < state time, odometry of a use_imu member); its record repeats the state before it, and the
 * member's state, time and last velocity stay untouched, as without tracking. */
typedef struct rfleet_track_rec {
    double t;            /* the message's stamp */
    double mu3[3];
    double sigma3x3[9];  /* column-major */
    int member;
    int kind;            /* RFLEET_EV_* */
    int K;               /* SCAN: observations of the message */
    int dropped;
    int n;
    int flags;
    int n_state, n_map, n_new;
    int pad_;
} rfleet_track_rec;

/* on != 0: every later rfleet_submit is tracked (ONE launch, as before; its ring segment holds 128 more bytes per message, and a call
 * whose every message is dropped still launches, for the records).  Off at rfleet_create.  max_records bounds the HOST-side log per
 * member: when a member's log is full the oldest record is discarded and counted; 0 = the default of 1024; a smaller bound than
 * before trims at once.  Switching off keeps what is logged, records of calls already submitted included.  rfleet_set_state logs
 * nothing.  REKF_ERR_INVALID for a null handle or max_records < 0; no HIP call, no synchronisation.
 * (Added without a new RFLEET_ABI_VERSION: a binding looks the three calls up by name.) */
int rfleet_set_tracking(rfleet_t *f, int on, long max_records);
/* The records of the listed members, compact and in the order listed, each member's oldest first; they leave the log.  members NULL =
 * all B members in order (count must be B).  Synchronises once, launches nothing.  counts[g] is written on success AND with
 * REKF_ERR_BUFFER (the records do not fit cap_rows: out is not touched, nothing leaves the log, counts sizes the second call).
 * out NULL: the call that asks for the counts (nothing leaves the log).  lost (nullable): lost[g] = records of members[g] discarded
 * since the previous take that handed records over.  With tracking never switched on every count is zero.
 * REKF_ERR_INVALID as rfleet_get_reflectors: a null handle, count < 0, count > 0 with null counts, cap_rows < 0, a member outside
 * 0 .. B-1, a member listed twice, members NULL with count != B.  count == 0 with a list is REKF_OK and does nothing. */
int rfleet_take_track(rfleet_t *f, const int *members, int count, int *counts /*[count]*/, rfleet_track_rec *out, long cap_rows,
                      long *lost /*[count], nullable*/);
/* Wide scans.  on != 0: every later rfleet_submit accepts scans of up to RFLEET_MAX_OBS_WIDE observations (K beyond that is
 * REKF_ERR_TOO_MANY_OBS, validated before anything moves).  Off at rfleet_create: K > RFLEET_MAX_OBS is refused as ever.  Switching
 * on allocates the members' wide match records (once) and launches nothing; switching off keeps the records readable.  A submit
 * WITHOUT a scan wider than RFLEET_MAX_OBS launches exactly the kernel it launched before, switch on or off; one WITH such a scan is
 * ONE launch of k_fleet_step_wide, which also carries the call's narrow scans, odometry and fixes, with the same bits for those.
 * Per member: Predict and ReflectorMatch once over all K observations, the MM pairs in ceil(MM / 32) block steps (rows linearised
 * at the state behind Predict, the innovation corrected by what the blocks before moved, the heading normalised once), the pose fix
 * as a step of its own, the augmentation once (the first (n_max - n) / 2 new observations, REKF_FLAGBIT_CAPACITY beyond).
 * REKF_ERR_INVALID for a null handle, REKF_ERR_HIP (rfleet_last_hip_error) when the records cannot be allocated.
 * (Added without a new RFLEET_ABI_VERSION: a binding looks the three calls up by name.) */
int rfleet_set_wide_scans(rfleet_t *f, int on);
/* rfleet_get_last_match with caller-sized lists: they hold cap entries (pairs: 2 cap).  REKF_ERR_BUFFER when a count exceeds cap:
 * the three counts are written and no list is touched.  Serves the records of narrow scans too. */
int rfleet_get_last_match_wide(rfleet_t *f, int member, int cap, int *n_state, int *state_pairs, int *n_map, int *map_pairs,
                               int *n_new, int *new_ids);
/* Host counters since rfleet_create: launches of k_fleet_step_wide, scans with K > RFLEET_MAX_OBS submitted.  No HIP call. */
int rfleet_wide_counts(rfleet_t *f, long *launches, long *scans);
/* sizeof(rfleet_track_rec) as the library was compiled */
int rfleet_sizeof_track_rec(void);
/* Snapshot and restore of full member states.  A snapshot is ONE caller-owned blob of bytes, position-independent and self-describing
 * (it can be written to a file as it is): rfleet_snapshot_hdr, then `count` rfleet_snapshot_member entries in the order listed, then
 * per entry at byte offset `off` its doubles -- mu[0:n], then the packed lower triangle of the covariance, n (n + 1) / 2 doubles,
 * column-major: column j holds rows j .. n-1 -- the payloads in the entries' order, one behind the other without gaps.  A member's
 * whole state is that, its sticky flags and the host's time and last odometry velocity: the fleet holds zeros beyond n. */
#define RFLEET_SNAPSHOT_MAGIC "RFLTSNAP"   /* the header's 8 bytes, no terminator */
#define RFLEET_SNAPSHOT_VERSION 1
typedef struct rfleet_snapshot_hdr {
    char magic[8];
    int version;         /* RFLEET_SNAPSHOT_VERSION */
    int count;           /* entries */
    long bytes;          /* the blob's size */
} rfleet_snapshot_hdr;
typedef struct rfleet_snapshot_member {
    double t;            /* state time */
    double vt[3];        /* last odometry velocity */
    int member;          /* the index it was taken from */
    int n;               /* state dimension 3 + 2 L */
    int flags;           /* sticky REKF_FLAGBIT_* */
    int pad_;
    long off;            /* byte offset of the member's doubles from the blob's start, a multiple of 8 */
} rfleet_snapshot_member;
/* The listed members' states into out, in the order listed (members NULL = all B members in order, count must be B).  Every event
 * submitted before the call is in the snapshot; the call changes nothing in the fleet.  Synchronises (the pose slots hold each member's
 * n), enqueues ONE launch of k_fleet_pack (csrc/fleet_snapshot.hip) whatever count is, copies the payload out and synchronises again; the
 * host writes the header and the entries.  *bytes = the blob's size, always written on REKF_OK and REKF_ERR_BUFFER.  out NULL: only
 * *bytes is written and nothing is launched.  cap_bytes < *bytes: REKF_ERR_BUFFER, out untouched.
 * REKF_ERR_INVALID before any HIP call and before the handle is read: a null handle, count < 0, null bytes, cap_bytes < 0; after the
 * handle is read and before any HIP call: a member outside 0 .. B-1, a member listed twice, members NULL with count != B.  count == 0
 * with a list is REKF_OK: a blob of the header alone.  (Added without a new RFLEET_ABI_VERSION: a binding looks the calls up by name.) */
int rfleet_snapshot(rfleet_t *f, const int *members, int count, void *out, long cap_bytes, long *bytes);
/* Entry g of the blob becomes member members[g] (members NULL: the index it was taken from); count must equal the blob's count.
 * EVERYTHING is validated on the host before anything moves and before any HIP call -- the blob as rfleet_snapshot_peek does, every n
 * <= the TARGET fleet's 3 + 2 max_landmarks, targets inside 0 .. B-1 and distinct -- and a refused call (REKF_ERR_INVALID) leaves every
 * member as it was.  Then: one synchronisation, one copy of the payload to the device, ONE launch of k_fleet_unpack, one synchronisation.
 * A target then holds n, flags, mu[0:n] and the triangle from the blob, ZERO beyond n (as a member created fresh and grown to that
 * state), its pose slot as rfleet_get_poses reads it, the blob's time and velocity, and a last-match record of zero counts.  The pose
 * track logs nothing; members not listed keep every bit; the fleet's map, options, tracking and wide-scan switches are not touched.
 * REKF_ERR_HIP when the device staging buffer cannot be allocated: nothing has moved. */
int rfleet_restore(rfleet_t *f, const void *blob, long bytes, const int *members, int count);
/* The validation of a blob alone, pure host, no handle: the magic, the version, `bytes` against the header, every entry's n odd,
 * >= 3 and <= 3 + 2 RFLEET_MAX_LANDMARKS, its member >= 0, its off a multiple of 8, at or behind the end of the entry before it (the
 * first: of the entries) and its payload inside the blob.  count, max_n (0 for an empty blob): nullable.  REKF_ERR_INVALID otherwise. */
int rfleet_snapshot_peek(const void *blob, long bytes, int *count, int *max_n);
/* sizeof(rfleet_snapshot_member) / sizeof(rfleet_snapshot_hdr) as the library was compiled */
int rfleet_sizeof_snapshot_member(void);
int rfleet_sizeof_snapshot_hdr(void);
/* The detector's centres bound to the filter on the device.  rfleet_submit with one more kind of event: RFLEET_EV_SCAN_LINKED is a
 * scan whose observations are entry ev.K of `link` (include/rlink.h: one outstanding submit of a fleet detector, rdet2d_batch_link /
 * rdet3d_batch_link of rdet.h, or records the caller planted).  Its xy is not looked at, its t is used as given (the entry's stamp is
 * the caller's to copy), has_pose_fix / pose_fix work as for a scan; events of the other two kinds may be mixed in freely.  The host
 * never sees the centres and waits for nothing: the fleet's stream waits for link->ready (when not NULL), ONE launch of k_fleet_bind
 * (csrc/fleet_link.hip), one 64-lane workgroup per linked scan whose entry has a record, copies the centres into the segment and
 * stores their count into the packed event, link->consumed (when not NULL) is recorded behind it, and the step launch follows: two
 * launches per call instead of one, and no kernel of rfleet_submit differs.  Per linked scan the bind reads K and err from the
 * record once and takes the scan or leaves it EMPTY -- a Predict to its stamp, as a scan with K = 0 is:
 *     err != 0                             status err                       taken 0
 *     K < 0 or K > link->max_centers       status -4 (RDET_ERR_CAPACITY)    taken 0
 *     K > RFLEET_MAX_OBS (_WIDE)           status REKF_ERR_TOO_MANY_OBS     taken 0      (what rfleet_submit refuses on the host)
 *     otherwise                            status 0                         taken K
 * so the state and the host's time mirror stay well defined whatever a record holds; rfleet_link_status tells the host afterwards.
 * An entry with record == -1 is packed as the empty scan the detector's host knows it to be and needs no bind.
 * On a fleet with rfleet_set_wide_scans on, a call that holds a linked scan with a record takes k_fleet_step_wide -- the host cannot
 * know whether K > RFLEET_MAX_OBS -- with the same bits for narrow scans; rfleet_wide_counts counts that launch, and counts scans
 * only as far as the host knows them: a linked scan that turns out wide is not in `scans`.
 * EVERYTHING is validated first and a refused call (REKF_ERR_INVALID) touches nothing: what rfleet_submit refuses, a linked scan with
 * a null or malformed link, an entry index outside the link, an entry named twice, an entry whose member differs from the event's,
 * an entry with host_status != 0, a link of another device, a linked scan on a fleet with rfleet_set_tracking on (the track's K is
 * the host's).  link may be NULL when no event is linked: the call is rfleet_submit.  The link's host arrays are read during the call
 * only.  (Added without a new RFLEET_ABI_VERSION: a binding looks the three calls up by name.) */
int rfleet_submit_linked(rfleet_t *f, const rfleet_event *ev, int count, const rlink *link);
/* What the binds of the LAST rfleet_submit_linked that held a linked scan did, one record per linked scan in event order: taken,
 * status and K as read from the record (0, 0, 0 for an entry without a record).  Synchronises.  Returns the number of records
 * (>= 0; 0 before any linked submit), REKF_ERR_BUFFER when cap holds fewer (nothing written), REKF_ERR_INVALID for a null handle or
 * cap < 0.  Each output may be NULL. */
int rfleet_link_status(rfleet_t *f, int *taken, int *status, int *K_seen, int cap);
/* Host counters since rfleet_create: calls that held a linked scan, launches of k_fleet_bind, linked scans submitted, and linked scans
 * a bind left empty (status != 0) -- that one is updated when rfleet_link_status reads a submit's records, once per submit.  No HIP call. */
int rfleet_link_counts(rfleet_t *f, long *submits, long *binds, long *scans, long *emptied);
/* sizeof(rlink) as the library was compiled */
int rfleet_sizeof_link(void);
/* Wait for all enqueued work.  REKF_ERR_HIP when the device reported an error. */
int rfleet_sync(rfleet_t *f);
int rfleet_size(rfleet_t *f, int *B, int *max_landmarks);
const char *rfleet_last_hip_error(rfleet_t *f);
int rfleet_abi_version(void);
/* sizeof(rfleet_event) as the library was compiled: a binding checks its own layout against it */
int rfleet_sizeof_event(void);

#ifdef __cplusplus
}
#endif
#endif /* RFLEET_H_ */
