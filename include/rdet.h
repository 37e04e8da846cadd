/*
 * rdet.h -- C ABI of the MI355X-native reflector detectors (librdet.so).
 *
 * Drop-in boundary underneath the reference's C++ interface
 * reflector_detect::ReflectorDetectInterface
 * (reference include/reflector_detect/reflector_detect_interface.h:23-38) and its two
 * implementations LaserReflectorDetect (src/reflector_detect/laser/laser_reflector_detect.cc)
 * and PointCloudReflectorDetect (src/reflector_detect/point_cloud/point_cloud_reflector_detect.cc).
 * The ROS message types do not cross this boundary: the C++ adapter
 * (include/reflector_ekf_slam_amd/detect_adapter.hpp) unpacks sensor_msgs::LaserScan /
 * PointCloud2 into the plain arrays below.
 *
 * Conventions: opaque handles, caller-owned HOST buffers borrowed for the call, 0 / negative
 * error code, never exit() (the reference exit(-1)s on malformed scans,
 * laser_reflector_detect.cc:27-38), not thread-safe, one HIP stream per handle.  Both
 * handle_* calls are synchronous because the reference interface returns the Observation.
 *
 * rdet2d_batch_* is the 2D detector for a fleet host: B members (robots), each with its own options,
 * sensor_to_base_link and pose extrapolator, and ONE kernel launch per tick that detects one scan
 * of every member that has one (one workgroup per scan, no workgroup waits for another).  submit
 * enqueues and returns, collect waits and hands the results back in the order of the call.
 */
#ifndef RDET_H_
#define RDET_H_

#include "rlink.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDET_ABI_VERSION 1
#define RDET_MAX_CENTERS 256     /* most reflectors one scan / cloud may yield */

enum {
    RDET_OK = 0,
    RDET_ERR_INVALID = -1,       /* bad argument */
    RDET_ERR_HIP = -2,
    RDET_ERR_BAD_SCAN = -3,      /* range_min/max or angle fields malformed (reference: exit(-1)) */
    RDET_ERR_CAPACITY = -4,      /* more beams / points / reflectors than the handle was created for */
    RDET_ERR_BUFFER = -5
};

/* reflector_detect::ReflectorDetectOptions (laser_reflector_detect.h:8-15) */
typedef struct rdet2d_options {
    double intensity_min;
    double reflector_min_length;
    double reflector_length_error;
    float range_min;
    float range_max;
} rdet2d_options;

typedef struct rdet2d rdet2d_t;

/* LaserReflectorDetect(options) + SetSensorToBaseLinkTransform(pose): the transform is passed
 * already projected to 2D (transform::Project2D, transform.h:93-98): x, y, yaw. */
int rdet2d_create(const rdet2d_options *opt, const double sensor_to_base_link_xyyaw[3],
                  int max_beams, int device, rdet2d_t **out);
void rdet2d_destroy(rdet2d_t *h);
int rdet2d_set_sensor_to_base_link(rdet2d_t *h, const double xyyaw[3]);

/* HandleOdometryData (laser_reflector_detect.cc:318-322 -> pose_extrapolator.cc:28-32).
 * quat_zw = (orientation.z, orientation.w): the only components the extrapolator reads. */
int rdet2d_handle_odometry(rdet2d_t *h, double t, const double pos_xy[2], const double quat_zw[2],
                           double vx, double vy, double wz);

/* HandleLaserScan (laser_reflector_detect.cc:23-316).  The scalar arguments are the
 * sensor_msgs::LaserScan header fields; ranges / intensities hold N beams.
 * Out: K reflector centres (base_link frame, de-skewed to the scan end) in centers_xy
 * (capacity max_centers pairs), obs_time = observation.time_. */
int rdet2d_handle_scan(rdet2d_t *h, double stamp, float angle_min, float angle_max,
                       float angle_increment, float scan_time, float range_min, float range_max,
                       const float *ranges, const float *intensities, int N,
                       float *centers_xy, int max_centers, int *K, double *obs_time);

/* GetRangeData (laser_reflector_detect.h:24): origin + de-skewed returns of the last scan. */
int rdet2d_get_range_data(rdet2d_t *h, float origin_xy[2], float *returns_xy, int cap_points,
                          int *n_returns);

/* ---- the 2D detector for many robots: one launch per tick (csrc/det2d_batch.hip) ----------------
 * Member m of a batch handle is one LaserReflectorDetect: options opts[m], sensor_to_base_link
 * s2b_xyyaw[m], its own odometry.  Results are bit for bit those of B rdet2d handles. */
typedef struct rdet2d_batch rdet2d_batch_t;

/* one sensor_msgs::LaserScan of one member (the fields HandleLaserScan reads) */
typedef struct rdet2d_scan {
    int member;                       /* 0 .. B-1 */
    double stamp;
    float angle_min, angle_max, angle_increment, scan_time, range_min, range_max;
    const float *ranges, *intensities;
    int N;
} rdet2d_scan;

/* B >= 1 members, scans of at most max_beams (<= 8192 are detected) beams.  Refused before any HIP
 * call: null pointers, B < 1, max_beams < 1. */
int rdet2d_batch_create(const rdet2d_options *opts, const double *s2b_xyyaw, int B, int max_beams,
                        int device, rdet2d_batch_t **out);
void rdet2d_batch_destroy(rdet2d_batch_t *b);
int rdet2d_batch_set_sensor_to_base_link(rdet2d_batch_t *b, int member, const double xyyaw[3]);
int rdet2d_batch_handle_odometry(rdet2d_batch_t *b, int member, double t, const double pos_xy[2],
                                 const double quat_zw[2], double vx, double vy, double wz);

/* The member's slice of the device-visible staging area (max_beams floats each).  A scan whose
 * ranges / intensities pointers are these is read in place by the kernel: a driver may receive
 * straight into them.  They stay valid for the life of the handle; do not write them between
 * submit and collect. */
int rdet2d_batch_staging(rdet2d_batch_t *b, int member, float **ranges, float **intensities);

/* At most one scan per member.  Everything is validated first: a member out of range or named
 * twice, N < 0, N > 0 with a null pointer, count < 0, null scans with count > 0, a submit that has
 * not been collected (RDET_ERR_INVALID), N > max_beams or N > 8192 (RDET_ERR_CAPACITY) refuse the
 * WHOLE call and change nothing (no odometry trimmed).  A call may mix lidars.  A malformed message (range_min < 0, range_max <= range_min,
 * angle_increment < 0 with angle_max <= angle_min) is data: that scan's status becomes
 * RDET_ERR_BAD_SCAN with K = 0, the others run.  Enqueues one launch and returns. */
int rdet2d_batch_submit(rdet2d_batch_t *b, const rdet2d_scan *scans, int count);

/* Waits for the launch; status / K / obs_time (= stamp) / centres of scan i of the submit at
 * index i (centres at centers_xy + 2 * max_centers * i).  max_centers is capped at
 * RDET_MAX_CENTERS; a scan with more centres than max_centers gets RDET_ERR_BUFFER and K = 0.
 * centers_xy may be null when max_centers is 0, obs_time may be null.  RDET_ERR_INVALID when
 * nothing is submitted, RDET_ERR_HIP (text: rdet2d_batch_last_hip_error) on a device error. */
int rdet2d_batch_collect(rdet2d_batch_t *b, int *status, int *K, float *centers_xy, int max_centers,
                         double *obs_time);

/* GetRangeData of the member's last detected scan (members that were not in a call keep theirs).
 * RDET_ERR_INVALID between submit and collect. */
int rdet2d_batch_get_range_data(rdet2d_batch_t *b, int member, float origin_xy[2],
                                float *returns_xy, int cap_points, int *n_returns);

/* GetRangeData of any list of members in ONE launch and ONE synchronisation (members NULL = all B, in
 * order; added without a new ABI version: look it up by name).  For every listed member counts[g],
 * origins_xy[2 g ..] and its rows are the bits rdet2d_batch_get_range_data(b, members[g], ...) gives
 * at that moment; the rows lie compactly in returns_xy, members[g]'s behind members[g-1]'s.
 * counts is written on success and on RDET_ERR_BUFFER (cap_points below the sum of the counts: no row
 * and no origin is touched, counts sizes the second call).  returns_xy NULL: counts and origins only,
 * nothing is launched or waited for (cap_points is not looked at beyond its sign).  origins_xy may be
 * NULL.  RDET_ERR_INVALID before any HIP call: a null handle, count < 0, null counts with count > 0,
 * cap_points < 0, a member out of range or listed twice, members NULL with count != B, a submit that
 * has not been collected.  count == 0 is RDET_OK and does nothing; a zero sum of counts launches
 * nothing.  The handle's first launching call allocates B * max_beams points of pinned host memory. */
int rdet2d_batch_get_range_data_all(rdet2d_batch_t *b, const int *members, int count, int *counts,
                                    float *origins_xy, float *returns_xy, long cap_points);
/* The submit that has not been collected, as a consumer on the same device needs to see it (include/rlink.h; the fleet filter's
 * rfleet_submit_linked takes one): valid only between submit and collect, RDET_ERR_INVALID otherwise or for a null pointer.  Launches
 * nothing and waits for nothing: records the handle's `ready` event on its stream behind the submit's launch, fills *out -- the
 * host arrays (member, stamp, the host's own status such as RDET_ERR_BAD_SCAN, the record index or -1 for an entry no workgroup runs
 * for: N = 0 or a malformed message) stay valid until the NEXT submit, the records until the handle is destroyed -- and remembers
 * that a link was taken: the next submit then makes the handle's STREAM (not the host) wait for `consumed`, which the consumer
 * records once it has read the records, before its kernel overwrites them, and destroy waits for it on the host.  A consumer that
 * never records `consumed` is not waited for.  collect is unchanged: it is still how the host gets the centres, the statuses and
 * the range data, and behind the consumer's own synchronisation it returns without waiting.
 * (Added without a new RDET_ABI_VERSION, as rdet3d_batch_link below: a binding looks them up by name.) */
int rdet2d_batch_link(rdet2d_batch_t *b, rlink *out);
int rdet2d_batch_sizeof_scan(void);
const char *rdet2d_batch_last_hip_error(rdet2d_batch_t *b);

/* reflector_detect::PointCloudOptions (point_cloud_reflector_detect.h:37-40) */
typedef struct rdet3d_options {
    double intensity_min;
} rdet3d_options;

typedef struct rdet3d rdet3d_t;

int rdet3d_create(const rdet3d_options *opt, const double sensor_to_base_link_xyyaw[3],
                  int max_points, int device, rdet3d_t **out);
void rdet3d_destroy(rdet3d_t *h);

/* HandlePointCloud (point_cloud_reflector_detect.cc:9-106): xyzi = N points (x, y, z,
 * intensity) as pcl::fromROSMsg would deliver them.  Out: K centres in base_link. */
int rdet3d_handle_cloud(rdet3d_t *h, double stamp, const float *xyzi, int N,
                        float *centers_xy, int max_centers, int *K, double *obs_time);

/* The same in two halves, for a caller that wants the next cloud's copy and launches to run while the device is still on this one
 * (a node whose callback hands clouds over back to back; the reference's own callback, point_cloud_reflector_detect.cc:9-106, is the
 * synchronous call above).  rdet3d_submit: the cloud into device memory and the kernels enqueued, no waiting.  rdet3d_collect: the
 * centres of the OLDEST cloud submitted and not yet collected (blocks until they are there).  At most two clouds may be submitted and
 * not collected (a third submit returns RDET_ERR_INVALID, as does a collect with nothing submitted, or rdet3d_handle_cloud in
 * between); results are those of rdet3d_handle_cloud called in the same order. */
int rdet3d_submit(rdet3d_t *h, double stamp, const float *xyzi, int N, int max_centers);
int rdet3d_collect(rdet3d_t *h, float *centers_xy, int max_centers, int *K, double *obs_time);

/* ---- the 3D detector for many robots: one launch per tick (csrc/det3d_batch.hip) ----------------
 * Member m of a batch handle is one PointCloudReflectorDetect: options opts[m], sensor_to_base_link
 * s2b_xyyaw[m] (HandlePointCloud reads no odometry).  One workgroup per cloud, no workgroup waits
 * for another.  Results are bit for bit those of B rdet3d handles. */
typedef struct rdet3d_batch rdet3d_batch_t;

/* one cloud of one member: N points (x, y, z, intensity) */
typedef struct rdet3d_cloud {
    int member;                       /* 0 .. B-1 */
    double stamp;
    const float *xyzi;
    int N;
} rdet3d_cloud;

/* B >= 1 members, clouds of at most max_points points.  Refused before any HIP call: null
 * pointers, B < 1, max_points < 1. */
int rdet3d_batch_create(const rdet3d_options *opts, const double *s2b_xyyaw, int B, int max_points,
                        int device, rdet3d_batch_t **out);
void rdet3d_batch_destroy(rdet3d_batch_t *b);
int rdet3d_batch_set_sensor_to_base_link(rdet3d_batch_t *b, int member, const double xyyaw[3]);

/* The member's slice of the device-visible staging area (4 * max_points floats).  A cloud whose
 * xyzi pointer is this is read in place by the kernel.  It stays valid for the life of the handle;
 * do not write it between submit and collect. */
int rdet3d_batch_staging(rdet3d_batch_t *b, int member, float **xyzi);

/* At most one cloud per member.  Everything is validated first: a null b, null clouds with
 * count > 0, count < 0, a member out of range or named twice, N < 0, N > 0 with a null pointer, a
 * submit that has not been collected (RDET_ERR_INVALID), N > max_points (RDET_ERR_CAPACITY) refuse
 * the WHOLE call and change nothing.  Enqueues one launch and returns. */
int rdet3d_batch_submit(rdet3d_batch_t *b, const rdet3d_cloud *clouds, int count);

/* Waits for the launch; status / K / obs_time (= stamp) / n_bright (the survivors of the intensity
 * gate) / centres of cloud i of the submit at index i (centres at centers_xy + 2 * max_centers * i).
 * max_centers is capped at RDET_MAX_CENTERS.  Per-cloud statuses are data, the other clouds run:
 * RDET_ERR_CAPACITY with K = 0 for more than rdet3d_batch_max_bright() survivors of the gate
 * (n_bright holds the true count: send that cloud through an rdet3d_t) or more than 256 accepted
 * clusters, RDET_ERR_BUFFER with K = 0 for more accepted clusters than max_centers.  centers_xy may
 * be null when max_centers is 0; obs_time and n_bright may be null. */
int rdet3d_batch_collect(rdet3d_batch_t *b, int *status, int *K, float *centers_xy, int max_centers,
                         double *obs_time, int *n_bright);
/* As rdet2d_batch_link: record -1 for a cloud with N = 0. */
int rdet3d_batch_link(rdet3d_batch_t *b, rlink *out);
int rdet_sizeof_link(void);           /* sizeof(rlink) as the library was compiled */
int rdet3d_batch_max_bright(void);    /* 5120 */
int rdet3d_batch_sizeof_cloud(void);
const char *rdet3d_batch_last_hip_error(rdet3d_batch_t *b);

const char *rdet_strerror(int code);
int rdet_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RDET_H_ */
