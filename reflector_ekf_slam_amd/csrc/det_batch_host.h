// det_batch_host.h -- what the fleet detectors' host side (det2d_batch.hip, det3d_batch.hip) does without a HIP call: plain C++17 over
// rdet.h's structs, built and run without a GPU by tests/cpp/det_batch_host.cpp.  Here are the records the kernels read (one
// definition for the host that packs them and the kernel that fetches them), and every rule of the two handles that is not a copy,
// an event or a launch:
//   check_members       one entry per member, inside 0 .. B-1; the `seen` scratch is all zero again on every exit
//   SubmitState         the submit that has not been collected, fill_link (include/rlink.h) and the collect rule
//   2D submit, 1-3 of 5 validate_scans, plan_tables (the cached beam-angle tables), pack_scans / pack_scan (the record, the odometry trim);
//                       fill_angle_table for step 4 (4: the staging copies and table uploads, 5: the launch and the commit -- det2d_batch.hip)
//   3D submit           validate_clouds, pack_clouds (records compacted over the clouds that run, the launch's LDS capacity)
//   range data          range_counts, range_data_plan: the records and the (record, tile) workgroup table of get_range_data_all
#pragma once
#include "../../include/rdet.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#define RDET2DB_MAX_BEAMS 8192            // a workgroup holds its whole scan in LDS
#define RDET2DB_TABLES 8                  // cached beam-angle tables
#define RDET2DB_RANGE_THREADS 256
#define RDET2DB_RANGE_TILE (2 * RDET2DB_RANGE_THREADS)    // rows (slots) per workgroup of k_det2d_batch_range_data
#define RDET3DB_MAX_BRIGHT 5120           // survivors of the gate a workgroup of k_det3d_batch holds

namespace det_batch_host {

// PoseExtrapolator sample (see det2d.hip): yaw = 2 atan2(q.z, q.w) taken once on the host
struct Odom {
    double time, px, py, yaw, vx, vy, wz;
};

// One scan of a call: everything k_det2d_batch needs that is not a beam.  An array of these, indexed by blockIdx.x, lies in
// the call's staging segment.
struct BatchRec {
    // options (laser_reflector_detect.h:8-15)
    double intensity_min, min_length, length_error;
    double first_point_time, point_delta_t;
    // pose extrapolator state: 0, 1 or 2 samples (front, back)
    Odom front, back;
    int n_odom;
    float opt_range_min, opt_range_max;
    // message header
    float msg_range_min, msg_range_max, angle_increment;
    int N, is_circle;
    int member;                    // whose staging slice, scratch slice and point-cloud buffer
    int table;                     // which cached beam-angle table
    int run;                       // 0: nothing to detect (N == 0 or a malformed message): the slot is cleared
    // sensor_to_base_link as Rigid2f + host-evaluated cos/sin of its angle
    float s2b_x, s2b_y, s2b_a, s2b_c, s2b_s;
};

// One member's rows of a get_range_data_all call
struct RangeRec {
    long long src_off;             // the member's first row in `returns` (member * max_beams)
    long long dst_off;             // its first row in the output
    int n, pad;
};
struct RangeTile { int record, tile; };       // one workgroup of k_det2d_batch_range_data (the kernel reads it as an int2)

// One cloud of a call: an array of these, indexed by blockIdx.x, lies in pinned host memory.
struct Cloud3Rec {
    double intensity_min;
    double stamp;
    int member;                    // whose staging slice
    int N;
    int slot;                      // the cloud's index in the call: where its result goes
    int pad;
    float sx, sy, cs, sn;          // sensor_to_base_link as Rigid2f, cos / sin of its angle by the host's libm
};
constexpr int CLOUD_TILE = 64;     // k_det3d_batch's nodes per bounding box: the launch's LDS holds a multiple of it

struct Member2d {
    rdet2d_options opt;
    double s2b[3];
    std::vector<Odom> odom;        // PoseExtrapolator::odometry_data_
    int last_n_returns = 0;
};
struct Member3d { rdet3d_options opt; double s2b[3]; };

// The submit that has not been collected, one entry per scan / cloud of the call, and what rlink's host arrays point into (valid
// until the next submit): member, stamp, the status the host alone reports (3D: always 0), whether a workgroup runs for the entry,
// and the record index fill_link makes of that.  `seen` is check_members' scratch.
struct SubmitState {
    bool outstanding = false;
    int sub_count = 0;
    std::vector<int> sub_member, sub_status, sub_runs, sub_record;
    std::vector<double> sub_stamp;
    std::vector<char> seen;
    void size(int B)
    {
        sub_member.resize((size_t)B); sub_runs.resize((size_t)B); sub_record.resize((size_t)B); sub_stamp.resize((size_t)B);
        sub_status.assign((size_t)B, RDET_OK); seen.assign((size_t)B, 0);
    }
};

namespace {   // (a handle's translation unit exports its C functions and nothing else)

// The first of `count` entries whose member (member_of(g)) is outside 0 .. B-1 or was named by an entry before it; `count` when every
// entry names a member of its own.  (More than B entries: one of them is such an entry.)  seen [B] is all zero before and behind.
template <typename MemberOf>
inline int check_members(int count, int B, std::vector<char> &seen, MemberOf &&member_of)
{
    int bad = count;
    for (int g = 0; g < count && bad == count; ++g) {
        const int m = member_of(g);
        if (m < 0 || m >= B || seen[(size_t)m]) bad = g;
        else seen[(size_t)m] = 1;
    }
    for (int g = 0; g < bad; ++g) seen[(size_t)member_of(g)] = 0;
    return bad;
}

// `members` names each of its `count` members once, or is NULL with count == B (all members in order)
inline bool members_named_once(const int *members, int count, int B, std::vector<char> &seen)
{
    if (!members) return count == B;
    return count <= B && check_members(count, B, seen, [&](int g) { return members[g]; }) == count;
}

// ---- 1: validate the whole call, nothing changes before every entry has passed.  The first offending entry in call order decides:
// entry_code(e) is what the entry's own fields are refused with (asked of an entry only when its member is fine)
template <typename Entry, typename Code>
inline int validate(const Entry *e, int count, int B, std::vector<char> &seen, Code &&entry_code)
{
    const int bad = check_members(count, B, seen, [&](int i) { return e[i].member; });
    for (int i = 0; i < bad; ++i)
        if (const int rc = entry_code(e[i])) return rc;
    return bad < count ? RDET_ERR_INVALID : RDET_OK;
}
inline int validate_scans(const rdet2d_scan *scans, int count, int B, int max_beams, std::vector<char> &seen)
{
    return validate(scans, count, B, seen, [&](const rdet2d_scan &s) {
        if (s.N < 0 || (s.N > 0 && (!s.ranges || !s.intensities))) return (int)RDET_ERR_INVALID;
        return (s.N > max_beams || s.N > RDET2DB_MAX_BEAMS) ? (int)RDET_ERR_CAPACITY : (int)RDET_OK;
    });
}
inline int validate_clouds(const rdet3d_cloud *clouds, int count, int B, int max_points, std::vector<char> &seen)
{
    return validate(clouds, count, B, seen, [&](const rdet3d_cloud &c) {
        if (c.N < 0 || (c.N > 0 && !c.xyzi)) return (int)RDET_ERR_INVALID;
        return c.N > max_points ? (int)RDET_ERR_CAPACITY : (int)RDET_OK;
    });
}

// ---- 2 (2D): the beam-angle table of every scan that runs.  One table per lidar (N, angle_min, angle_increment by their bits);
// RDET2DB_TABLES of them are kept, the least recently used is replaced -- but never one this call still needs, and a call with more
// lidars than cached tables gives the scan its member's own slot RDET2DB_TABLES + member, which is not kept.
struct Table {
    int N = -1;
    float angle_min = 0.f, inc = 0.f;
    unsigned long long used = 0;       // the submit that used it last
};
struct TableCache {
    Table tab[RDET2DB_TABLES];
    unsigned long long n_submit = 0;
};
struct TableUse { int table; bool fill, cached; };      // of one scan: which table, step 4 fills and uploads it, it is kept

inline bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

inline bool malformed(const rdet2d_scan &s)
{
    if (s.range_min < 0 || s.range_max <= s.range_min) return true;              // :27-32
    return s.angle_increment < 0.f && s.angle_max <= s.angle_min;                // :33-38
}

inline int find_table(const TableCache &c, const rdet2d_scan &s)
{
    for (int t = 0; t < RDET2DB_TABLES; ++t)
        if (c.tab[t].N == s.N && same_bits(c.tab[t].angle_min, s.angle_min) && same_bits(c.tab[t].inc, s.angle_increment)) return t;
    return -1;
}

inline void plan_tables(TableCache &c, const rdet2d_scan *scans, int count, std::vector<TableUse> &use)
{
    ++c.n_submit;
    use.assign((size_t)count, TableUse{0, false, false});
    // the tables this call needs and already has: none of them may be the one that is replaced
    for (int i = 0; i < count; ++i) {
        const int t = (scans[i].N == 0 || malformed(scans[i])) ? -1 : find_table(c, scans[i]);
        if (t >= 0) c.tab[t].used = c.n_submit;
    }
    for (int i = 0; i < count; ++i) {
        const rdet2d_scan &s = scans[i];
        if (s.N == 0 || malformed(s)) continue;                                 // (touches no table)
        TableUse &u = use[(size_t)i];
        u.table = find_table(c, s);
        u.cached = true;
        if (u.table < 0) {
            int lru = 0;
            for (int t = 1; t < RDET2DB_TABLES; ++t)
                if (c.tab[t].used < c.tab[lru].used) lru = t;                   // least recently used
            u.fill = true;
            u.cached = c.tab[lru].used != c.n_submit;                           // ... unless this call uses all of them
            u.table = u.cached ? lru : RDET2DB_TABLES + s.member;
            if (u.cached) { c.tab[lru].N = s.N; c.tab[lru].angle_min = s.angle_min; c.tab[lru].inc = s.angle_increment; }
        }
        if (u.cached) c.tab[u.table].used = c.n_submit;
    }
}

// a table's three parts (angle | cos | sin, `stride` floats apart): the float32 accumulation of :51/:175 and its cos/sin (:68), host libm
inline void fill_angle_table(float *ta, size_t stride, float angle_min, float angle_increment, int N)
{
    float *tc = ta + stride, *ts = tc + stride;
    float angle = angle_min;
    for (int k = 0; k < N; ++k) {
        ta[k] = angle; tc[k] = cosf(angle); ts[k] = sinf(angle);
        angle += angle_increment;
    }
}

// ---- 3 (2D): scan s of member M into its record; -> the host's status of the scan.  A malformed message is data: RDET_ERR_BAD_SCAN,
// nothing runs and the member keeps its odometry and its range data.  N == 0: nothing runs, the member's range data is empty.
inline int pack_scan(const rdet2d_scan &s, Member2d &M, int table, BatchRec &A)
{
    std::memset(&A, 0, sizeof(A));
    A.member = s.member;
    if (malformed(s)) return RDET_ERR_BAD_SCAN;
    if (s.N == 0) { M.last_n_returns = 0; return RDET_OK; }
    const int N = s.N;
    A.run = 1;
    A.intensity_min = M.opt.intensity_min;
    A.min_length = M.opt.reflector_min_length;
    A.length_error = M.opt.reflector_length_error;
    A.opt_range_min = M.opt.range_min; A.opt_range_max = M.opt.range_max;
    A.msg_range_min = s.range_min; A.msg_range_max = s.range_max;
    A.angle_increment = s.angle_increment;
    const double last_point_time = s.stamp;                                     // :48
    A.point_delta_t = (double)(s.scan_time / (float)N);                         // :49 (float / size_t)
    A.first_point_time = last_point_time - s.scan_time;                         // :50
    A.N = N;
    A.is_circle = ((s.angle_max - s.angle_min - 2 * M_PI) < 1e-6) ? 1 : 0;      // :55
    A.s2b_x = (float)M.s2b[0]; A.s2b_y = (float)M.s2b[1]; A.s2b_a = (float)M.s2b[2];   // :54
    A.s2b_c = cosf(A.s2b_a); A.s2b_s = sinf(A.s2b_a);
    // TrimDataByTime(first_point_time) (:52-53 -> pose_extrapolator.cc:12-26): at least one sample stays
    size_t drop = 0;
    while (M.odom.size() - drop > 1 && M.odom[drop].time < A.first_point_time) ++drop;
    if (drop) M.odom.erase(M.odom.begin(), M.odom.begin() + (long)drop);
    A.n_odom = (int)(M.odom.size() > 2 ? 2 : M.odom.size());
    if (!M.odom.empty()) { A.front = M.odom.front(); A.back = M.odom.back(); }
    A.table = table;
    return RDET_OK;
}

// every scan of a validated call: record i is scan i's; -> the scans that run
inline int pack_scans(const rdet2d_scan *scans, int count, std::vector<Member2d> &m, const std::vector<TableUse> &use, SubmitState &st,
                      BatchRec *recs)
{
    int n_run = 0;
    for (int i = 0; i < count; ++i) {
        const rdet2d_scan &s = scans[i];
        st.sub_member[(size_t)i] = s.member;
        st.sub_stamp[(size_t)i] = s.stamp;                                          // :26 (USE_CORRECT_TIME undefined)
        st.sub_status[(size_t)i] = pack_scan(s, m[(size_t)s.member], use[(size_t)i].table, recs[i]);
        n_run += st.sub_runs[(size_t)i] = (st.sub_status[(size_t)i] == RDET_OK && s.N > 0) ? 1 : 0;
    }
    st.sub_count = count;
    return n_run;
}

// ---- 3D: every cloud of a validated call; a cloud with N == 0 has no workgroup, so the records are compacted over the clouds that
// run and carry their cloud's index.  -> the clouds that run; *cap: the nodes the launch's LDS holds (no cloud has more survivors
// than points: the largest N rounded up to whole tiles, at most RDET3DB_MAX_BRIGHT)
inline int pack_clouds(const rdet3d_cloud *clouds, int count, const std::vector<Member3d> &m, SubmitState &st, Cloud3Rec *recs, int *cap)
{
    int n_run = 0, n_max = 0;
    for (int i = 0; i < count; ++i) {
        const rdet3d_cloud &c = clouds[i];
        const Member3d &M = m[(size_t)c.member];
        st.sub_stamp[(size_t)i] = c.stamp;                                          // observation.time_ (:97)
        st.sub_member[(size_t)i] = c.member;
        st.sub_runs[(size_t)i] = c.N > 0 ? 1 : 0;
        if (c.N == 0) continue;
        Cloud3Rec &A = recs[n_run++];
        std::memset(&A, 0, sizeof(A));
        A.intensity_min = M.opt.intensity_min;
        A.stamp = c.stamp;
        A.member = c.member; A.N = c.N; A.slot = i;
        A.sx = (float)M.s2b[0]; A.sy = (float)M.s2b[1];
        const float sa = (float)M.s2b[2];
        A.cs = cosf(sa); A.sn = sinf(sa);
        if (c.N > n_max) n_max = c.N;
    }
    st.sub_count = count;
    *cap = (n_max + CLOUD_TILE - 1) / CLOUD_TILE * CLOUD_TILE;
    if (*cap > RDET3DB_MAX_BRIGHT) *cap = RDET3DB_MAX_BRIGHT;
    return n_run;
}

// ---- the outstanding submit as an rlink: entry i's record is record i when a workgroup runs for it, else -1 (K = 0 is known)
inline void fill_link(SubmitState &st, int device, const void *records, long record_bytes, int k_off, int err_off, int centers_off,
                      void *ready, void *consumed, rlink *out)
{
    for (int i = 0; i < st.sub_count; ++i) st.sub_record[(size_t)i] = st.sub_runs[(size_t)i] ? i : -1;
    std::memset(out, 0, sizeof(*out));
    out->count = st.sub_count;
    out->device = device;
    out->member = st.sub_member.data();
    out->stamp = st.sub_stamp.data();
    out->host_status = st.sub_status.data();
    out->record = st.sub_record.data();
    out->records = records;
    out->record_bytes = record_bytes;
    out->k_off = k_off; out->err_off = err_off; out->centers_off = centers_off;
    out->max_centers = RDET_MAX_CENTERS;
    out->ready = ready;
    out->consumed = consumed;
}

// ---- collect.  What a call must bring:
inline bool collect_args_ok(int count, const int *status, const int *K, const float *centers_xy, int max_centers)
{
    return max_centers >= 0 && (count == 0 || (status && K && (max_centers == 0 || centers_xy)));
}
// ... and the rule, over records that have int K, int err and (x, y) float pairs `centers` (out[i] is entry i's): the host's status
// stands; an entry that did not run has K = 0; a record's err becomes the status, K = 0; more centres than max_centers (at most
// RDET_MAX_CENTERS) is RDET_ERR_BUFFER, K = 0.  each(i, record) for every entry, record NULL for one that did not run.
template <typename Out, typename Each>
inline void collect(const SubmitState &st, const Out *out, int *status, int *K, float *centers_xy, int max_centers, double *obs_time, Each &&each)
{
    if (max_centers > RDET_MAX_CENTERS) max_centers = RDET_MAX_CENTERS;
    for (int i = 0; i < st.sub_count; ++i) {
        const Out &o = out[i];
        K[i] = 0;
        status[i] = st.sub_status[(size_t)i];
        if (obs_time) obs_time[i] = st.sub_stamp[(size_t)i];
        each(i, st.sub_runs[(size_t)i] ? &o : nullptr);
        if (!st.sub_runs[(size_t)i]) continue;
        if (o.err) { status[i] = o.err; continue; }
        if (o.K > max_centers) { status[i] = RDET_ERR_BUFFER; continue; }
        K[i] = o.K;
        if (o.K > 0) std::memcpy(centers_xy + (size_t)2 * (size_t)max_centers * (size_t)i, o.centers, sizeof(o.centers[0]) * (size_t)o.K);
    }
}

// ---- get_range_data_all.  rd_tab is RangeRec[B] | RangeTile[B * range_tiles], the table at the next 256-byte boundary
inline size_t range_tiles(int max_beams) { return ((size_t)max_beams + 1 + RDET2DB_RANGE_TILE - 1) / RDET2DB_RANGE_TILE; }   // (max_beams rows behind an odd offset)
inline size_t range_table_off(int B) { return (sizeof(RangeRec) * (size_t)B + 255) / 256 * 256; }

// counts[g] = the rows of the g-th listed member; -> their sum
inline long range_counts(const int *members, int count, int max_beams, const std::vector<Member2d> &m, int *counts)
{
    long total = 0;
    for (int g = 0; g < count; ++g) {
        int n = m[(size_t)(members ? members[g] : g)].last_n_returns;
        n = n < 0 ? 0 : (n > max_beams ? max_beams : n);                   // (never true for a count k_det2d_batch wrote: keeps every access inside the buffers)
        total += counts[g] = n;
    }
    return total;
}
// one record per listed member with rows, its rows behind those of the members before it; a record behind an odd offset has its
// pairs on the destination's 16-byte grid (lead = dst_off & 1 slots in front), so it costs ceil((n + lead) / RDET2DB_RANGE_TILE)
// workgroups.  -> the workgroups
inline int range_data_plan(const int *members, const int *counts, int count, int max_beams, RangeRec *recs, RangeTile *wgmap)
{
    int nrec = 0, nwg = 0;
    long long at = 0;
    for (int g = 0; g < count; ++g) {
        if (counts[g] == 0) continue;
        RangeRec &R = recs[nrec];
        R.src_off = (long long)(members ? members[g] : g) * (long long)max_beams;
        R.dst_off = at;
        R.n = counts[g]; R.pad = 0;
        const int slots = counts[g] + (int)(at & 1);
        for (int t = 0; t * RDET2DB_RANGE_TILE < slots; ++t) wgmap[nwg++] = RangeTile{nrec, t};
        at += counts[g];
        ++nrec;
    }
    return nwg;
}

}  // namespace
}  // namespace det_batch_host
