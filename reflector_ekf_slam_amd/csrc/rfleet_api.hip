// rfleet_api.hip -- host side of the fleet filter (include/rfleet.h): validation, the host's time / velocity mirror,
// the pinned staging ring, one launch of k_fleet_step per rfleet_submit, the fleet's shared pre-loaded map.
//
// Time and vt_ are host state: HandleOdometryMessage's `t < state time` test (cc:211-212) and the use_imu switch are decided
// here, before packing, and every packed event carries its own dt and velocity.  A call's events are grouped by member (stable:
// a member's events keep their order) into one segment of a ring of pinned buffers, which the kernel reads in place; a
// segment is reused only after the launch that read it has finished (one hipEvent per segment), so consecutive submits
// do not synchronise until the ring has gone round.
//
// The map (rfleet_set_map) is one device buffer per fleet and a byte per member.  A submit takes k_fleet_step_map only when a member
// with events in it uses a non-empty map.  The other two kernels never touch FleetMemberCtl::n_map / map_pairs, so the host
// remembers per member whether its last scan's record was written by the map kernel (map_rec).
//
// rfleet_get_reflectors is one launch of k_fleet_reflectors (fleet_reflectors.hip) behind whatever has been submitted, into a pinned
// buffer sized at rfleet_create for B x max_landmarks rows, one synchronisation, and a host copy of the rows into the caller's arrays.
//
// The pose track (rfleet_set_tracking / rfleet_take_track).  A tracked submit appends one FleetTrackRec per packed event to its ring
// segment and launches k_fleet_step_track, which fills them; the host keeps beside the segment what it knows of each event (stamp,
// member, kind, K, dropped).  The messages the untracked path drops before packing (stale odometry, odometry of a use_imu member) are
// packed as events of kind 2, which move nothing and only write their record.  Records move from a segment into the per-member host
// log (bounded: the oldest goes, counted) wherever a segment's launch is known to have finished: before the segment is reused and in
// rfleet_sync, which every getter calls -- oldest segment first, so a member's records stay in order.  The untracked submit keeps its
// segment layout, its "every event dropped => no launch" and its kernels.
//
// Wide scans (rfleet_set_wide_scans).  A submit that holds at least one scan of more than RFLEET_MAX_OBS observations launches
// k_fleet_step_wide (fleet_wide.hip) instead of one of the four kernels above, with the same segment and the same FleetLaunch; every
// other submit launches what it always did.  That kernel writes the match record of every member with a scan in the call into the
// member's FleetWideRec, so the host remembers per member which kind of launch wrote its last record (rec_wide), as map_rec does.
//
// Snapshot and restore (rfleet_snapshot / rfleet_restore / rfleet_snapshot_peek).  The blob's header and entries are written and read
// by the host; the payloads move between the members' arrays and ONE device staging buffer (allocated on first use, grown to what a
// call needs, freed in rfleet_destroy) by one launch of k_fleet_pack / k_fleet_unpack (fleet_snapshot.hip) over a host-built table of
// (member, panel) records that sits in front of the payload in the same buffer.  Every copy goes through the handle's stream and is
// followed by a synchronisation: the stream is non-blocking, so a legacy hipMemcpy would not be ordered behind it.
#include "fleet_dev.h"
#include "fleet_reflectors.h"
#include "fleet_snapshot.h"
#include "../../include/rfleet.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {
constexpr int kSegs = 8;
constexpr long kTrackDefault = 1024;        // records per member the host log holds when rfleet_set_tracking is given 0

// One member's host-side log: the records [head, buf.size()) of a vector that is appended to and, when the bound discards from the
// front, compacted now and then -- no allocation per record.
struct TrackLog {
    std::vector<rfleet_track_rec> buf;
    size_t head = 0;
    size_t size() const { return buf.size() - head; }
    void clear() { buf.clear(); head = 0; }
    long trim(long max_records)             // -> records discarded
    {
        long gone = 0;
        while ((long)size() > max_records) { ++head; ++gone; }
        if (head >= 256 && head >= buf.size() / 2) {
            buf.erase(buf.begin(), buf.begin() + (long)head);
            head = 0;
        }
        return gone;
    }
};

struct TrackMeta {                          // what the host knows of a packed event of a tracked submit
    double t;
    int member, kind, K, dropped;
};

struct Segment {
    char *host = nullptr;
    char *dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool busy = false;
    // a tracked submit: its records (n_track of them, in the segment at `track`) wait here until the launch is known to have finished
    int n_track = 0;
    const FleetTrackRec *track = nullptr;
    std::vector<TrackMeta> meta;
};
}  // namespace

struct rfleet {
    int B = 0, max_landmarks = 0, n_max = 0, ld = 0, device = 0;
    hipStream_t stream = nullptr;
    FleetDev dev{};
    FleetPoseSlot *pose_host = nullptr;
    std::vector<rekf_options> opts;
    std::vector<double> time, vt;           // the host's mirror: state time [B], vt_ [B][3]
    Segment seg[kSegs];
    int next_seg = 0;
    std::string hip_error;
    // the shared map: device copies, the host's copy of the per-member switch, and who wrote each member's last match record
    float *map_xy = nullptr;
    double *map_cov = nullptr;
    unsigned char *map_use_dev = nullptr;
    int M_map = 0;
    std::vector<unsigned char> map_use, map_rec;
    // rfleet_get_reflectors: ONE pinned allocation, ell5 [R][5] | xy2 [R][2] | cov4 [R][4] | counts [B] | members [B], R = B max_landmarks
    char *refl_host = nullptr, *refl_dev = nullptr;
    std::vector<int> scanned;               // scratch of rfleet_submit: members with a scan event in the call
    // scratch of rfleet_submit (kept to avoid per-call allocation)
    std::vector<int> cnt, pos, order;
    std::vector<double> time_tmp, vt_tmp;
    std::vector<double> stage;
    // the pose track: the switch, the bound per member, the per-member log and what it has discarded since the last take
    bool tracking = false;
    long track_max = kTrackDefault;
    std::vector<TrackLog> track_log;
    std::vector<long> track_lost;
    std::vector<unsigned char> dropped;     // scratch of a tracked rfleet_submit: event i is one the untracked path drops
    // wide scans: the switch, the members' wide match records (device, allocated when first switched on), who wrote each member's
    // last record, and the host counters of rfleet_wide_counts
    bool wide = false;
    FleetWideRec *wide_rec = nullptr;
    std::vector<unsigned char> rec_wide;
    long wide_launches = 0, wide_scans = 0;
    // snapshot / restore: the device staging buffer (table | payload), and the host's scratch for the table and the payload offsets
    char *snap_dev = nullptr;
    size_t snap_cap = 0;
    std::vector<FleetSnapRec> snap_rec;
    std::vector<long> snap_off;
};

#define FLEET_HIP(f, call)                                                     \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            (f)->hip_error = std::string(#call) + ": " + hipGetErrorString(e_); \
            return REKF_ERR_HIP;                                               \
        }                                                                      \
    } while (0)

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
static size_t align128(size_t v) { return (v + 127) & ~(size_t)127; }

static void track_push(rfleet *f, int member, const rfleet_track_rec &r)
{
    TrackLog &log = f->track_log[(size_t)member];
    log.buf.push_back(r);
    f->track_lost[(size_t)member] += log.trim(f->track_max);
}

// the records of a segment whose launch has finished, into the members' logs
static void track_harvest(rfleet *f, Segment &s)
{
    for (int e = 0; e < s.n_track; ++e) {
        const FleetTrackRec &d = s.track[e];
        const TrackMeta &m = s.meta[(size_t)e];
        rfleet_track_rec r{};
        r.t = m.t;
        memcpy(r.mu3, d.mu3, sizeof(r.mu3));
        memcpy(r.sigma3x3, d.C9, sizeof(r.sigma3x3));
        r.member = m.member; r.kind = m.kind; r.K = m.K; r.dropped = m.dropped;
        r.n = d.n; r.flags = d.flags;
        r.n_state = d.n_state; r.n_map = d.n_map; r.n_new = d.n_new;
        track_push(f, m.member, r);
    }
    s.n_track = 0;
}

// the pinned buffer of rfleet_get_reflectors: byte offsets of its parts
static size_t refl_rows(const rfleet *f) { return (size_t)f->B * (size_t)f->max_landmarks; }
static size_t refl_off_xy(const rfleet *f) { return sizeof(double) * 5 * refl_rows(f); }
static size_t refl_off_cov(const rfleet *f) { return sizeof(double) * 7 * refl_rows(f); }
static size_t refl_off_counts(const rfleet *f) { return sizeof(double) * 11 * refl_rows(f); }
static size_t refl_off_members(const rfleet *f) { return refl_off_counts(f) + sizeof(int) * (size_t)f->B; }
static size_t refl_bytes(const rfleet *f) { return refl_off_members(f) + sizeof(int) * (size_t)f->B; }

extern "C" {

int rfleet_abi_version(void) { return RFLEET_ABI_VERSION; }

int rfleet_sizeof_event(void) { return (int)sizeof(rfleet_event); }

int rfleet_sizeof_track_rec(void) { return (int)sizeof(rfleet_track_rec); }

const char *rfleet_last_hip_error(rfleet_t *f) { return f ? f->hip_error.c_str() : ""; }

void rfleet_destroy(rfleet_t *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (Segment &s : f->seg) {
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.host) (void)hipHostFree(s.host);
    }
    if (f->dev.mu) (void)hipFree(f->dev.mu);
    if (f->dev.P) (void)hipFree(f->dev.P);
    if (f->dev.W) (void)hipFree(f->dev.W);
    if (f->dev.Kn) (void)hipFree(f->dev.Kn);
    if (f->dev.ctl) (void)hipFree(f->dev.ctl);
    if (f->dev.opt) (void)hipFree((void *)f->dev.opt);
    if (f->pose_host) (void)hipHostFree(f->pose_host);
    if (f->refl_host) (void)hipHostFree(f->refl_host);
    if (f->map_xy) (void)hipFree(f->map_xy);
    if (f->map_cov) (void)hipFree(f->map_cov);
    if (f->map_use_dev) (void)hipFree(f->map_use_dev);
    if (f->wide_rec) (void)hipFree(f->wide_rec);
    if (f->snap_dev) (void)hipFree(f->snap_dev);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

static int fleet_create_body(rfleet_t *f, const rekf_options *opts)
{
    const int B = f->B;
    const size_t ld = (size_t)f->ld;
    FLEET_HIP(f, hipSetDevice(f->device));
    FLEET_HIP(f, hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    FLEET_HIP(f, hipMalloc((void **)&f->dev.mu, sizeof(double) * ld * B));
    FLEET_HIP(f, hipMalloc((void **)&f->dev.P, sizeof(double) * ld * ld * B));
    FLEET_HIP(f, hipMalloc((void **)&f->dev.W, sizeof(double) * ld * RFLEET_PANEL_COLS * B));
    FLEET_HIP(f, hipMalloc((void **)&f->dev.Kn, sizeof(double) * ld * RFLEET_PANEL_COLS * B));
    FLEET_HIP(f, hipMalloc((void **)&f->dev.ctl, sizeof(FleetMemberCtl) * B));
    FLEET_HIP(f, hipMalloc((void **)&f->dev.opt, sizeof(FleetMemberOpt) * B));
    FLEET_HIP(f, hipHostMalloc((void **)&f->pose_host, sizeof(FleetPoseSlot) * B, hipHostMallocDefault));
    FLEET_HIP(f, hipHostGetDevicePointer((void **)&f->dev.pose, f->pose_host, 0));
    FLEET_HIP(f, hipHostMalloc((void **)&f->refl_host, refl_bytes(f), hipHostMallocDefault));
    FLEET_HIP(f, hipHostGetDevicePointer((void **)&f->refl_dev, f->refl_host, 0));
    FLEET_HIP(f, hipMemset(f->dev.mu, 0, sizeof(double) * ld * B));
    FLEET_HIP(f, hipMemset(f->dev.P, 0, sizeof(double) * ld * ld * B));
    FLEET_HIP(f, hipMemset(f->dev.W, 0, sizeof(double) * ld * RFLEET_PANEL_COLS * B));
    FLEET_HIP(f, hipMemset(f->dev.Kn, 0, sizeof(double) * ld * RFLEET_PANEL_COLS * B));
    std::vector<FleetMemberCtl> ctl((size_t)B);
    std::vector<FleetMemberOpt> dopt((size_t)B);
    std::vector<double> mu(ld * B, 0.0);
    memset(ctl.data(), 0, sizeof(FleetMemberCtl) * B);
    memset(f->pose_host, 0, sizeof(FleetPoseSlot) * B);
    for (int i = 0; i < B; ++i) {
        const rekf_options &o = opts[i];
        ctl[i].n = 3;
        dopt[i].lin_cov = o.linear_velocity_cov;
        dopt[i].ang_cov = o.angular_velocity_cov;
        dopt[i].obs_cov = o.observation_cov;
        dopt[i].model = (o.odom_model == REKF_ODOM_DIFF) ? 0 : 1;          // cc:13-32: anything else is OMNI
        dopt[i].pad_ = 0;
        for (int k = 0; k < 3; ++k) {
            mu[(size_t)i * ld + k] = o.init_pose[k];
            f->pose_host[i].mu3[k] = o.init_pose[k];
        }
        f->pose_host[i].n = 3;
        f->time[i] = o.init_time;
    }
    FLEET_HIP(f, hipMemcpy(f->dev.ctl, ctl.data(), sizeof(FleetMemberCtl) * B, hipMemcpyHostToDevice));
    FLEET_HIP(f, hipMemcpy((void *)f->dev.opt, dopt.data(), sizeof(FleetMemberOpt) * B, hipMemcpyHostToDevice));
    FLEET_HIP(f, hipMemcpy(f->dev.mu, mu.data(), sizeof(double) * ld * B, hipMemcpyHostToDevice));
    for (Segment &s : f->seg) FLEET_HIP(f, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    return REKF_OK;
}

int rfleet_create(const rekf_options *opts, int B, int max_landmarks, int device, rfleet_t **out)
{
    if (!out) return REKF_ERR_INVALID;
    *out = nullptr;
    if (!opts || B < 1 || B > (1 << 16) || max_landmarks < 1 || device < 0) return REKF_ERR_INVALID;
    if (max_landmarks > RFLEET_MAX_LANDMARKS) return REKF_ERR_UNSUPPORTED;
    rfleet_t *f = new rfleet;
    f->B = B;
    f->max_landmarks = max_landmarks;
    f->n_max = 3 + 2 * max_landmarks;
    f->ld = (f->n_max + 15) & ~15;
    f->device = device;
    f->dev.ld = f->ld;
    f->dev.n_max = f->n_max;
    f->dev.B = B;
    f->opts.assign(opts, opts + B);
    f->time.assign((size_t)B, 0.0);
    f->vt.assign((size_t)3 * B, 0.0);
    f->cnt.resize((size_t)B);
    f->pos.resize((size_t)B);
    f->map_use.assign((size_t)B, 0);
    f->map_rec.assign((size_t)B, 0);
    f->rec_wide.assign((size_t)B, 0);
    f->track_log.resize((size_t)B);
    f->track_lost.assign((size_t)B, 0);
    const int rc = fleet_create_body(f, opts);
    if (rc != REKF_OK) {
        rfleet_destroy(f);
        return rc;
    }
    *out = f;
    return REKF_OK;
}

int rfleet_size(rfleet_t *f, int *B, int *max_landmarks)
{
    if (!f) return REKF_ERR_INVALID;
    if (B) *B = f->B;
    if (max_landmarks) *max_landmarks = f->max_landmarks;
    return REKF_OK;
}

int rfleet_sync(rfleet_t *f)
{
    if (!f) return REKF_ERR_INVALID;
    FLEET_HIP(f, hipSetDevice(f->device));
    FLEET_HIP(f, hipStreamSynchronize(f->stream));
    for (int i = 0; i < kSegs; ++i) {                                      // (from the oldest segment: a member's records stay in order)
        Segment &s = f->seg[(f->next_seg + i) % kSegs];
        s.busy = false;
        if (s.n_track) track_harvest(f, s);
    }
    return REKF_OK;
}

int rfleet_submit(rfleet_t *f, const rfleet_event *ev, int count)
{
    if (!f || count < 0 || (count > 0 && !ev)) return REKF_ERR_INVALID;
    // ---- validate everything before anything moves
    const int max_obs = f->wide ? RFLEET_MAX_OBS_WIDE : RFLEET_MAX_OBS;
    for (int i = 0; i < count; ++i) {
        const rfleet_event &e = ev[i];
        if (e.member < 0 || e.member >= f->B) return REKF_ERR_INVALID;
        if (e.kind != RFLEET_EV_ODOM && e.kind != RFLEET_EV_SCAN) return REKF_ERR_INVALID;
        if (e.kind == RFLEET_EV_SCAN) {
            if (e.K < 0) return REKF_ERR_INVALID;
            if (e.K > max_obs) return REKF_ERR_TOO_MANY_OBS;
            if (e.K > 0 && !e.xy) return REKF_ERR_INVALID;
            if (e.has_pose_fix && !(std::isfinite(e.pose_fix[0]) && std::isfinite(e.pose_fix[1]) && std::isfinite(e.pose_fix[2])))
                return REKF_ERR_INVALID;
        } else if (e.has_pose_fix) {
            return REKF_ERR_INVALID;                                       // a fix belongs to a scan
        }
    }
    if (count == 0) return REKF_OK;
    // ---- which events reach the device (on a copy of the mirror: committed behind the launch)
    const int B = f->B;
    const bool tracked = f->tracking;
    if (tracked) f->dropped.assign((size_t)count, 0);
    f->time_tmp = f->time;
    f->vt_tmp = f->vt;
    f->order.clear();
    f->scanned.clear();
    std::fill(f->cnt.begin(), f->cnt.end(), 0);
    size_t n_obs = 0, n_fix = 0;
    long n_wide = 0;                                                       // scans of the call with K > RFLEET_MAX_OBS
    std::vector<double> &dts = f->stage;
    dts.resize((size_t)count * 4);
    for (int i = 0; i < count; ++i) {
        const rfleet_event &e = ev[i];
        const int b = e.member;
        if (e.kind == RFLEET_EV_ODOM) {
            if (f->opts[b].use_imu || e.t < f->time_tmp[b]) {              // cc:213-223: odometry is ignored with use_imu; cc:211-212
                if (!tracked) continue;
                f->dropped[(size_t)i] = 1;                                 // (the node still publishes the unchanged pose: a record, no Predict)
                for (int k = 0; k < 4; ++k) dts[4 * (size_t)i + k] = 0.0;
                f->cnt[b]++;
                f->order.push_back(i);
                continue;
            }
            for (int k = 0; k < 3; ++k) f->vt_tmp[3 * b + k] = e.v[k];     // cc:216
        } else {
            n_obs += (size_t)e.K;
            n_fix += e.has_pose_fix ? 1 : 0;
            n_wide += e.K > RFLEET_MAX_OBS ? 1 : 0;
            f->scanned.push_back(b);
        }
        dts[4 * (size_t)i] = e.t - f->time_tmp[b];                         // cc:217-218 / :232-233
        for (int k = 0; k < 3; ++k) dts[4 * (size_t)i + 1 + k] = f->vt_tmp[3 * b + k];
        f->time_tmp[b] = e.t;
        f->cnt[b]++;
        f->order.push_back(i);
    }
    const int E = (int)f->order.size();
    if (E == 0) return REKF_OK;
    int G = 0;
    bool with_map = false;                                                 // a member with events matches against a non-empty map
    for (int b = 0; b < B; ++b) {
        G += f->cnt[b] > 0;
        with_map = with_map || (f->cnt[b] > 0 && f->M_map > 0 && f->map_use[b]);
    }
    // ---- a ring segment: members[G] | ev_begin[G + 1] | events[E] | fix[3 n_fix] | obs[2 n_obs]
    const size_t off_mem = 0, off_beg = align16(off_mem + sizeof(int) * G), off_ev = align16(off_beg + sizeof(int) * (G + 1));
    const size_t off_fix = align16(off_ev + sizeof(FleetEvent) * E), off_obs = align16(off_fix + sizeof(double) * 3 * n_fix);
    size_t need = align16(off_obs + sizeof(float) * 2 * n_obs + 16);
    const size_t off_track = align128(need);                               // a tracked submit: | track[E], one 128-byte line each
    if (tracked) need = off_track + sizeof(FleetTrackRec) * (size_t)E;
    FLEET_HIP(f, hipSetDevice(f->device));
    Segment &s = f->seg[f->next_seg];
    if (s.busy) {
        FLEET_HIP(f, hipEventSynchronize(s.done));
        s.busy = false;
    }
    if (s.n_track) track_harvest(f, s);                                    // (the oldest segment: every later record comes behind these)
    if (s.cap < need) {
        size_t cap = s.cap ? s.cap : 4096;
        while (cap < need) cap *= 2;
        char *h = nullptr, *dv = nullptr;
        FLEET_HIP(f, hipHostMalloc((void **)&h, cap, hipHostMallocDefault));
        hipError_t e_ = hipHostGetDevicePointer((void **)&dv, h, 0);
        if (e_ != hipSuccess) {
            (void)hipHostFree(h);
            f->hip_error = std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e_);
            return REKF_ERR_HIP;
        }
        if (s.host) (void)hipHostFree(s.host);
        s.host = h; s.dev = dv; s.cap = cap;
    }
    int *members = (int *)(s.host + off_mem), *ev_begin = (int *)(s.host + off_beg);
    FleetEvent *pev = (FleetEvent *)(s.host + off_ev);
    double *pfix = (double *)(s.host + off_fix);
    float *pobs = (float *)(s.host + off_obs);
    int g = 0, acc = 0;
    for (int b = 0; b < B; ++b) {
        if (f->cnt[b] == 0) continue;
        members[g] = b;
        ev_begin[g] = acc;
        f->pos[b] = acc;
        acc += f->cnt[b];
        ++g;
    }
    ev_begin[G] = acc;
    size_t obs_at = 0;
    int fix_at = 0;
    if (tracked) s.meta.resize((size_t)E);
    for (int q = 0; q < E; ++q) {
        const int i = f->order[q];
        const rfleet_event &e = ev[i];
        const int at = f->pos[e.member]++;
        FleetEvent &pe = pev[at];
        if (tracked) {
            const int dr = f->dropped[(size_t)i];
            s.meta[(size_t)at] = TrackMeta{e.t, e.member, e.kind, e.kind == RFLEET_EV_SCAN ? e.K : 0, dr};
            if (dr) {
                pe = FleetEvent{0.0, {0.0, 0.0, 0.0}, 2, 0, (int)obs_at, -1};
                continue;
            }
        }
        pe.dt = dts[4 * (size_t)i];
        for (int k = 0; k < 3; ++k) pe.vt[k] = dts[4 * (size_t)i + 1 + k];
        pe.kind = (e.kind == RFLEET_EV_SCAN) ? 1 : 0;
        pe.K = (e.kind == RFLEET_EV_SCAN) ? e.K : 0;
        pe.obs_off = (int)obs_at;
        pe.fix_off = -1;
        if (e.kind == RFLEET_EV_SCAN && e.has_pose_fix) {
            pe.fix_off = fix_at;
            for (int k = 0; k < 3; ++k) pfix[fix_at + k] = e.pose_fix[k];
            fix_at += 3;
        }
        if (pe.K > 0) {
            memcpy(pobs + obs_at, e.xy, sizeof(float) * 2 * (size_t)pe.K);
            obs_at += 2 * (size_t)pe.K;
        }
    }
    FleetLaunch L{};
    L.members = (const int *)(s.dev + off_mem);
    L.ev_begin = (const int *)(s.dev + off_beg);
    L.ev = (const FleetEvent *)(s.dev + off_ev);
    L.obs = (const float *)(s.dev + off_obs);
    L.fix = n_fix ? (const double *)(s.dev + off_fix) : nullptr;      // (NULL selects the kernel without the pose phase)
    L.G = G;
    if (with_map) {                                                        // (M_map > 0 selects the kernel with the map branch)
        L.map_xy = f->map_xy;
        L.map_cov = f->map_cov;
        L.map_use = f->map_use_dev;
        L.M_map = f->M_map;
    }
    if (tracked) L.track = (FleetTrackRec *)(s.dev + off_track);           // (non-NULL selects k_fleet_step_track, the map kernel's body)
    if (n_wide > 0) FLEET_HIP(f, rfleet_launch_step_wide(f->dev, L, f->wide_rec, f->stream));   // (fix, map and track: chosen in the kernel)
    else FLEET_HIP(f, rfleet_launch_step(f->dev, L, f->stream));
    if (tracked) {
        s.n_track = E;
        s.track = (const FleetTrackRec *)(s.host + off_track);
    }
    for (int b : f->scanned) {
        f->map_rec[b] = (with_map || tracked) ? 1 : 0;
        f->rec_wide[b] = n_wide > 0 ? 1 : 0;
    }
    if (n_wide > 0) {
        f->wide_launches += 1;
        f->wide_scans += n_wide;
    }
    f->time.swap(f->time_tmp);
    f->vt.swap(f->vt_tmp);
    FLEET_HIP(f, hipEventRecord(s.done, f->stream));
    s.busy = true;
    f->next_seg = (f->next_seg + 1) % kSegs;
    return REKF_OK;
}

int rfleet_get_poses(rfleet_t *f, double *t, double *mu3, double *sigma3x3)
{
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    for (int b = 0; b < f->B; ++b) {
        const FleetPoseSlot &p = f->pose_host[b];
        if (t) t[b] = f->time[b];
        if (mu3) memcpy(mu3 + 3 * (size_t)b, p.mu3, sizeof(double) * 3);
        if (sigma3x3) memcpy(sigma3x3 + 9 * (size_t)b, p.C9, sizeof(double) * 9);
    }
    return REKF_OK;
}

int rfleet_predict_poses(rfleet_t *f, const double *t, double *mu3, double *sigma3x3)
{
#pragma clang fp contract(off)
    if (!f || !t || !mu3) return REKF_ERR_INVALID;
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    for (int b = 0; b < f->B; ++b) {
        const FleetPoseSlot &p = f->pose_host[b];
        const rekf_options &o = f->opts[b];
        const double *vt = &f->vt[3 * (size_t)b];
        double C[9];
        memcpy(C, p.C9, sizeof(C));
        Motion mo;
        motion_terms_of((o.odom_model == REKF_ODOM_DIFF) ? 0 : 1, t[b] - f->time[b], vt[0], vt[1], vt[2], o.linear_velocity_cov,
                        o.angular_velocity_cov, p.mu3[2], mo);                 // cc:100-150
        corner_predict(C, 3, mo);
        double *m = mu3 + 3 * (size_t)b;
        m[0] = p.mu3[0] + mo.d[0];
        m[1] = p.mu3[1] + mo.d[1];
        const double th = p.mu3[2] + mo.d[2];
        m[2] = atan2(sin(th), cos(th));
        if (sigma3x3) memcpy(sigma3x3 + 9 * (size_t)b, C, sizeof(C));
    }
    return REKF_OK;
}

int rfleet_get_n(rfleet_t *f, int *n)
{
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    if (!n) return REKF_ERR_INVALID;
    for (int b = 0; b < f->B; ++b) n[b] = f->pose_host[b].n;
    return REKF_OK;
}

int rfleet_get_flags(rfleet_t *f, int *flags)
{
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    if (!flags) return REKF_ERR_INVALID;
    for (int b = 0; b < f->B; ++b) flags[b] = f->pose_host[b].flags;
    return REKF_OK;
}

int rfleet_get_state(rfleet_t *f, int member, double *t, int *n_out, double *mu, long mu_cap, double *sigma, long sigma_cap)
{
    if (!f || member < 0 || member >= f->B) return REKF_ERR_INVALID;
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    const int n = f->pose_host[member].n;
    const size_t ld = (size_t)f->ld;
    if (t) *t = f->time[member];
    if (n_out) *n_out = n;
    if (mu) {
        if (mu_cap < n) return REKF_ERR_BUFFER;
        FLEET_HIP(f, hipMemcpy(mu, f->dev.mu + (size_t)member * ld, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    if (sigma) {
        if (sigma_cap < (long)n * n) return REKF_ERR_BUFFER;
        std::vector<double> tmp(ld * n);
        FLEET_HIP(f, hipMemcpy(tmp.data(), f->dev.P + (size_t)member * ld * ld, sizeof(double) * ld * n, hipMemcpyDeviceToHost));
        for (int j = 0; j < n; ++j)
            for (int i = j; i < n; ++i) {
                const double v = tmp[i + j * ld];
                sigma[i + (size_t)j * n] = v;
                sigma[j + (size_t)i * n] = v;
            }
    }
    return REKF_OK;
}

int rfleet_set_state(rfleet_t *f, int member, double t, int n, const double *mu, const double *sigma, const double *vt3)
{
    if (!f || member < 0 || member >= f->B || !mu || !sigma) return REKF_ERR_INVALID;
    if (n < 3 || n > f->n_max || ((n - 3) & 1)) return REKF_ERR_INVALID;
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    const size_t ld = (size_t)f->ld;
    std::vector<double> tmp(ld * n, 0.0);
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) tmp[i + j * ld] = sigma[i + (size_t)j * n];
    FLEET_HIP(f, hipMemcpy(f->dev.mu + (size_t)member * ld, mu, sizeof(double) * n, hipMemcpyHostToDevice));
    FLEET_HIP(f, hipMemcpy(f->dev.P + (size_t)member * ld * ld, tmp.data(), sizeof(double) * ld * n, hipMemcpyHostToDevice));
    FLEET_HIP(f, hipMemcpy(&f->dev.ctl[member].n, &n, sizeof(int), hipMemcpyHostToDevice));
    FleetPoseSlot &p = f->pose_host[member];
    for (int k = 0; k < 3; ++k) p.mu3[k] = mu[k];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) p.C9[i + 3 * j] = (i >= j) ? sigma[i + (size_t)j * n] : sigma[j + (size_t)i * n];
    p.n = n;
    f->time[member] = t;
    if (vt3)
        for (int k = 0; k < 3; ++k) f->vt[3 * (size_t)member + k] = vt3[k];
    return REKF_OK;
}

// the member's last match record, whichever kind of launch wrote it: counts, then the lists if every count fits `cap`
static int last_match_body(rfleet_t *f, int member, int cap, int *n_state, int *state_pairs, int *n_map, int *map_pairs, int *n_new,
                           int *new_ids)
{
    if (!f || member < 0 || member >= f->B || cap < 0) return REKF_ERR_INVALID;
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    int ns, nm, nn;
    const int *sp, *mp, *nw;
    FleetMemberCtl c;
    std::vector<FleetWideRec> wr;
    if (f->rec_wide[member]) {
        wr.resize(1);
        FLEET_HIP(f, hipMemcpy(wr.data(), f->wide_rec + member, sizeof(FleetWideRec), hipMemcpyDeviceToHost));
        ns = wr[0].n_state; nm = wr[0].n_map; nn = wr[0].n_new;
        sp = wr[0].state_pairs; mp = wr[0].map_pairs; nw = wr[0].new_ids;
    } else {
        FLEET_HIP(f, hipMemcpy(&c, f->dev.ctl + member, sizeof(c), hipMemcpyDeviceToHost));
        ns = c.n_state; nn = c.n_new;
        nm = f->map_rec[member] ? c.n_map : 0;                             // (only the map kernel writes the map part of a record)
        sp = c.state_pairs; mp = c.map_pairs; nw = c.new_ids;
    }
    if (n_state) *n_state = ns;
    if (n_map) *n_map = nm;
    if (n_new) *n_new = nn;
    if (ns > cap || nm > cap || nn > cap) return REKF_ERR_BUFFER;          // (the counts size the second call; no list is touched)
    if (map_pairs) memcpy(map_pairs, mp, sizeof(int) * 2 * (size_t)nm);
    if (state_pairs) memcpy(state_pairs, sp, sizeof(int) * 2 * (size_t)ns);
    if (new_ids) memcpy(new_ids, nw, sizeof(int) * (size_t)nn);
    return REKF_OK;
}

int rfleet_get_last_match(rfleet_t *f, int member, int *n_state, int *state_pairs, int *n_map, int *map_pairs, int *n_new, int *new_ids)
{
    return last_match_body(f, member, RFLEET_MAX_OBS, n_state, state_pairs, n_map, map_pairs, n_new, new_ids);
}

int rfleet_get_last_match_wide(rfleet_t *f, int member, int cap, int *n_state, int *state_pairs, int *n_map, int *map_pairs, int *n_new,
                               int *new_ids)
{
    return last_match_body(f, member, cap, n_state, state_pairs, n_map, map_pairs, n_new, new_ids);
}

int rfleet_set_wide_scans(rfleet_t *f, int on)
{
    if (!f) return REKF_ERR_INVALID;
    if (on && !f->wide_rec) {                                              // (allocates once; launches nothing)
        FLEET_HIP(f, hipSetDevice(f->device));
        FleetWideRec *p = nullptr;
        FLEET_HIP(f, hipMalloc((void **)&p, sizeof(FleetWideRec) * (size_t)f->B));
        hipError_t e_ = hipMemset(p, 0, sizeof(FleetWideRec) * (size_t)f->B);
        if (e_ == hipSuccess) e_ = hipDeviceSynchronize();                 // (the handle's stream does not wait for the null stream)
        if (e_ != hipSuccess) {
            (void)hipFree(p);
            f->hip_error = std::string("rfleet_set_wide_scans: ") + hipGetErrorString(e_);
            return REKF_ERR_HIP;
        }
        f->wide_rec = p;
    }
    f->wide = on != 0;
    return REKF_OK;
}

int rfleet_wide_counts(rfleet_t *f, long *launches, long *scans)
{
    if (!f) return REKF_ERR_INVALID;
    if (launches) *launches = f->wide_launches;
    if (scans) *scans = f->wide_scans;
    return REKF_OK;
}

int rfleet_set_map(rfleet_t *f, const float *xy, const double *cov, int M, const unsigned char *use)
{
    if (!f || M < 0 || (M > 0 && (!xy || !cov))) return REKF_ERR_INVALID;
    if (M > RFLEET_MAX_MAP_POINTS) return REKF_ERR_UNSUPPORTED;
    for (int i = 0; i < 2 * M; ++i)
        if (!std::isfinite(xy[i])) return REKF_ERR_INVALID;
    for (int i = 0; i < 4 * M; ++i)
        if (!std::isfinite(cov[i])) return REKF_ERR_INVALID;
    const int rc = rfleet_sync(f);                                         // no launch reads the old copy any more
    if (rc != REKF_OK) return rc;
    const size_t B = (size_t)f->B;
    std::vector<unsigned char> want(B, 1);
    if (use)
        for (size_t b = 0; b < B; ++b) want[b] = use[b] ? 1 : 0;
    float *nxy = nullptr;
    double *ncov = nullptr;
    if (M > 0) {                                                           // the new copy first: a failure leaves the old map in place
        hipError_t e_ = hipMalloc((void **)&nxy, sizeof(float) * 2 * (size_t)M);
        if (e_ == hipSuccess) e_ = hipMalloc((void **)&ncov, sizeof(double) * 4 * (size_t)M);
        if (e_ == hipSuccess && !f->map_use_dev) e_ = hipMalloc((void **)&f->map_use_dev, B);
        if (e_ == hipSuccess) e_ = hipMemcpy(nxy, xy, sizeof(float) * 2 * (size_t)M, hipMemcpyHostToDevice);
        if (e_ == hipSuccess) e_ = hipMemcpy(ncov, cov, sizeof(double) * 4 * (size_t)M, hipMemcpyHostToDevice);
        if (e_ == hipSuccess) e_ = hipMemcpy(f->map_use_dev, want.data(), B, hipMemcpyHostToDevice);
        if (e_ != hipSuccess) {
            if (nxy) (void)hipFree(nxy);
            if (ncov) (void)hipFree(ncov);
            if (f->map_use_dev) (void)hipMemcpy(f->map_use_dev, f->map_use.data(), B, hipMemcpyHostToDevice);
            f->hip_error = std::string("rfleet_set_map: ") + hipGetErrorString(e_);
            return REKF_ERR_HIP;
        }
    }
    if (f->map_xy) (void)hipFree(f->map_xy);
    if (f->map_cov) (void)hipFree(f->map_cov);
    f->map_xy = nxy;
    f->map_cov = ncov;
    f->M_map = M;
    f->map_use.swap(want);
    return REKF_OK;
}

int rfleet_get_map_size(rfleet_t *f, int *M)
{
    if (!f || !M) return REKF_ERR_INVALID;
    *M = f->M_map;
    return REKF_OK;
}

int rfleet_set_tracking(rfleet_t *f, int on, long max_records)
{
    if (!f || max_records < 0) return REKF_ERR_INVALID;
    f->tracking = on != 0;
    f->track_max = max_records ? max_records : kTrackDefault;
    for (int b = 0; b < f->B; ++b) {                                       // a smaller bound holds for what is logged already
        f->track_lost[(size_t)b] += f->track_log[(size_t)b].trim(f->track_max);
    }
    return REKF_OK;
}

int rfleet_take_track(rfleet_t *f, const int *members, int count, int *counts, rfleet_track_rec *out, long cap_rows, long *lost)
{
    if (!f || count < 0 || (count > 0 && !counts) || cap_rows < 0) return REKF_ERR_INVALID;
    const int B = f->B;
    if (!members && count != B) return REKF_ERR_INVALID;
    if (members) {
        if (count > B) return REKF_ERR_INVALID;                            // (more than B members: one is listed twice)
        std::fill(f->cnt.begin(), f->cnt.end(), 0);
        for (int g = 0; g < count; ++g) {
            if (members[g] < 0 || members[g] >= B || f->cnt[members[g]]++) return REKF_ERR_INVALID;
        }
    }
    if (count == 0) return REKF_OK;
    const int rc = rfleet_sync(f);                                         // (harvests every outstanding segment)
    if (rc != REKF_OK) return rc;
    long rows = 0;
    for (int g = 0; g < count; ++g) {
        const int b = members ? members[g] : g;
        counts[g] = (int)f->track_log[(size_t)b].size();
        rows += counts[g];
        if (lost) lost[g] = f->track_lost[(size_t)b];
    }
    if (!out) return REKF_OK;                                              // (no output given: the call that asks for the counts)
    if (rows > cap_rows) return REKF_ERR_BUFFER;
    for (int g = 0; g < count; ++g) {
        const int b = members ? members[g] : g;
        TrackLog &log = f->track_log[(size_t)b];
        out = std::copy(log.buf.begin() + (long)log.head, log.buf.end(), out);
        log.clear();
        f->track_lost[(size_t)b] = 0;
    }
    return REKF_OK;
}

int rfleet_get_reflectors(rfleet_t *f, const int *members, int count, int *counts, double *ellipses5, double *xy2, double *cov4, long cap_rows)
{
    if (!f || count < 0 || (count > 0 && !counts) || cap_rows < 0) return REKF_ERR_INVALID;
    if (count > 0 && cap_rows == 0 && (ellipses5 || xy2 || cov4)) return REKF_ERR_INVALID;   // (every member can hold a reflector)
    const int B = f->B;
    if (!members && count != B) return REKF_ERR_INVALID;
    if (members) {
        if (count > B) return REKF_ERR_INVALID;                            // (more than B members: one is listed twice)
        std::fill(f->cnt.begin(), f->cnt.end(), 0);
        for (int g = 0; g < count; ++g) {
            if (members[g] < 0 || members[g] >= B || f->cnt[members[g]]++) return REKF_ERR_INVALID;
        }
    }
    if (count == 0) return REKF_OK;
    FLEET_HIP(f, hipSetDevice(f->device));
    const size_t R = refl_rows(f);
    const int *h_counts = (const int *)(f->refl_host + refl_off_counts(f));
    FleetReflectorsLaunch L{};
    if (members) {                                                         // (no launch reads the list any more: every call ends in a synchronisation)
        memcpy(f->refl_host + refl_off_members(f), members, sizeof(int) * (size_t)count);
        L.members = (const int *)(f->refl_dev + refl_off_members(f));
    }
    L.count = count;
    L.cap_rows = cap_rows < (long)R ? cap_rows : (long)R;
    L.counts = (int *)(f->refl_dev + refl_off_counts(f));
    L.ell5 = ellipses5 ? (double *)f->refl_dev : nullptr;
    L.xy2 = xy2 ? (double *)(f->refl_dev + refl_off_xy(f)) : nullptr;
    L.cov4 = cov4 ? (double *)(f->refl_dev + refl_off_cov(f)) : nullptr;
    FLEET_HIP(f, rfleet_launch_reflectors(f->dev, L, f->stream));
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    long rows = 0;
    for (int g = 0; g < count; ++g) {
        counts[g] = h_counts[g];
        rows += h_counts[g];
    }
    if (rows > cap_rows && (ellipses5 || xy2 || cov4)) return REKF_ERR_BUFFER;    // (no output given: the call that asks for the counts)
    if (ellipses5) memcpy(ellipses5, f->refl_host, sizeof(double) * 5 * (size_t)rows);
    if (xy2) memcpy(xy2, f->refl_host + refl_off_xy(f), sizeof(double) * 2 * (size_t)rows);
    if (cov4) memcpy(cov4, f->refl_host + refl_off_cov(f), sizeof(double) * 4 * (size_t)rows);
    return REKF_OK;
}

int rfleet_sizeof_snapshot_member(void) { return (int)sizeof(rfleet_snapshot_member); }

int rfleet_sizeof_snapshot_hdr(void) { return (int)sizeof(rfleet_snapshot_hdr); }

// entry g of a blob (a blob need not be aligned: a file's bytes)
static rfleet_snapshot_member snap_entry(const void *blob, int g)
{
    rfleet_snapshot_member m;
    memcpy(&m, (const char *)blob + sizeof(rfleet_snapshot_hdr) + sizeof(m) * (size_t)g, sizeof(m));
    return m;
}

// what rfleet_snapshot_peek promises of a blob; pure host
static int snap_validate(const void *blob, long bytes, rfleet_snapshot_hdr *hdr, int *max_n)
{
    if (!blob || bytes < (long)sizeof(rfleet_snapshot_hdr)) return REKF_ERR_INVALID;
    rfleet_snapshot_hdr h;
    memcpy(&h, blob, sizeof(h));
    if (memcmp(h.magic, RFLEET_SNAPSHOT_MAGIC, sizeof(h.magic)) != 0 || h.version != RFLEET_SNAPSHOT_VERSION) return REKF_ERR_INVALID;
    if (h.count < 0 || h.bytes != bytes) return REKF_ERR_INVALID;
    long end = (long)sizeof(h) + (long)sizeof(rfleet_snapshot_member) * h.count;
    if (end > bytes) return REKF_ERR_INVALID;
    int widest = 0;
    for (int g = 0; g < h.count; ++g) {
        const rfleet_snapshot_member m = snap_entry(blob, g);
        if (m.n < 3 || !(m.n & 1) || m.n > 3 + 2 * RFLEET_MAX_LANDMARKS || m.member < 0) return REKF_ERR_INVALID;
        if (m.off < end || (m.off & 7)) return REKF_ERR_INVALID;          // (in order: behind the entries and behind the payload before it)
        const long size = (long)sizeof(double) * fleet_snap_doubles(m.n);
        if (m.off > bytes - size) return REKF_ERR_INVALID;
        end = m.off + size;
        widest = std::max(widest, m.n);
    }
    if (hdr) *hdr = h;
    if (max_n) *max_n = widest;
    return REKF_OK;
}

// the device staging buffer holds `need` bytes; a failed allocation leaves the old one in place
static int snap_reserve(rfleet_t *f, size_t need)
{
    if (f->snap_cap >= need) return REKF_OK;
    size_t cap = f->snap_cap ? f->snap_cap : (size_t)1 << 16;
    while (cap < need) cap *= 2;
    char *p = nullptr;
    FLEET_HIP(f, hipMalloc((void **)&p, cap));
    if (f->snap_dev) (void)hipFree(f->snap_dev);
    f->snap_dev = p;
    f->snap_cap = cap;
    return REKF_OK;
}

int rfleet_snapshot_peek(const void *blob, long bytes, int *count, int *max_n)
{
    rfleet_snapshot_hdr h;
    const int rc = snap_validate(blob, bytes, &h, max_n);
    if (rc == REKF_OK && count) *count = h.count;
    return rc;
}

int rfleet_snapshot(rfleet_t *f, const int *members, int count, void *out, long cap_bytes, long *bytes)
{
    if (!f || count < 0 || !bytes || cap_bytes < 0) return REKF_ERR_INVALID;
    const int B = f->B;
    if (!members && count != B) return REKF_ERR_INVALID;
    if (members) {
        if (count > B) return REKF_ERR_INVALID;                            // (more than B members: one is listed twice)
        std::fill(f->cnt.begin(), f->cnt.end(), 0);
        for (int g = 0; g < count; ++g) {
            if (members[g] < 0 || members[g] >= B || f->cnt[members[g]]++) return REKF_ERR_INVALID;
        }
    }
    const long head = (long)sizeof(rfleet_snapshot_hdr) + (long)sizeof(rfleet_snapshot_member) * count;
    long total = head;
    if (count > 0) {
        const int rc = rfleet_sync(f);                                     // (the pose slots hold every member's n and flags)
        if (rc != REKF_OK) return rc;
        f->snap_off.resize((size_t)count);
        for (int g = 0; g < count; ++g) {
            const int n = f->pose_host[members ? members[g] : g].n;
            if (n < 3 || n > f->n_max) {
                f->hip_error = "rfleet_snapshot: a member's pose slot holds a state dimension outside 3 .. n_max";
                return REKF_ERR_HIP;
            }
            f->snap_off[(size_t)g] = total;
            total += (long)sizeof(double) * fleet_snap_doubles(n);
        }
    }
    *bytes = total;
    if (!out) return REKF_OK;                                              // (the call that asks for the size)
    if (cap_bytes < total) return REKF_ERR_BUFFER;
    rfleet_snapshot_hdr h;
    memcpy(h.magic, RFLEET_SNAPSHOT_MAGIC, sizeof(h.magic));
    h.version = RFLEET_SNAPSHOT_VERSION;
    h.count = count;
    h.bytes = total;
    if (count > 0) {
        f->snap_rec.clear();
        for (int g = 0; g < count; ++g) {
            const int b = members ? members[g] : g;
            const int n = f->pose_host[b].n;
            const long off = (f->snap_off[(size_t)g] - head) / (long)sizeof(double);
            for (int p = 0; p < (n + RFLEET_SNAP_PANEL - 1) / RFLEET_SNAP_PANEL; ++p) f->snap_rec.push_back(FleetSnapRec{b, p, n, 0, off});
        }
        const size_t table = align128(sizeof(FleetSnapRec) * f->snap_rec.size()), payload = (size_t)(total - head);
        FLEET_HIP(f, hipSetDevice(f->device));
        const int rr = snap_reserve(f, table + payload);
        if (rr != REKF_OK) return rr;
        FleetSnapLaunch L{};
        L.rec = (const FleetSnapRec *)f->snap_dev;
        L.buf = (double *)(f->snap_dev + table);
        L.cap = (long)(payload / sizeof(double));
        L.count = (int)f->snap_rec.size();
        FLEET_HIP(f, hipMemcpyAsync(f->snap_dev, f->snap_rec.data(), sizeof(FleetSnapRec) * f->snap_rec.size(), hipMemcpyHostToDevice, f->stream));
        FLEET_HIP(f, rfleet_launch_pack(f->dev, L, f->stream));
        FLEET_HIP(f, hipMemcpyAsync((char *)out + head, L.buf, payload, hipMemcpyDeviceToHost, f->stream));
        const int rc = rfleet_sync(f);
        if (rc != REKF_OK) return rc;
    }
    memcpy(out, &h, sizeof(h));
    for (int g = 0; g < count; ++g) {
        const int b = members ? members[g] : g;
        rfleet_snapshot_member m;
        memset(&m, 0, sizeof(m));
        m.t = f->time[(size_t)b];
        for (int k = 0; k < 3; ++k) m.vt[k] = f->vt[3 * (size_t)b + k];
        m.member = b;
        m.n = f->pose_host[b].n;
        m.flags = f->pose_host[b].flags;
        m.off = f->snap_off[(size_t)g];
        memcpy((char *)out + sizeof(h) + sizeof(m) * (size_t)g, &m, sizeof(m));
    }
    return REKF_OK;
}

int rfleet_restore(rfleet_t *f, const void *blob, long bytes, const int *members, int count)
{
    if (!f || !blob || bytes < 0 || count < 0) return REKF_ERR_INVALID;
    rfleet_snapshot_hdr h;
    const int rv = snap_validate(blob, bytes, &h, nullptr);
    if (rv != REKF_OK) return rv;
    const int B = f->B;
    if (count != h.count || count > B) return REKF_ERR_INVALID;            // (more than B entries: two share a target)
    std::fill(f->cnt.begin(), f->cnt.end(), 0);
    for (int g = 0; g < count; ++g) {
        const rfleet_snapshot_member m = snap_entry(blob, g);
        const int b = members ? members[g] : m.member;
        if (m.n > f->n_max || b < 0 || b >= B || f->cnt[b]++) return REKF_ERR_INVALID;
    }
    if (count == 0) return REKF_OK;
    const int rc = rfleet_sync(f);                                         // no launch touches a target any more
    if (rc != REKF_OK) return rc;
    // ---- the payload's span in the blob, the table of (target, panel of the target's ld) records
    const rfleet_snapshot_member first = snap_entry(blob, 0), last = snap_entry(blob, count - 1);
    const long lo = first.off, hi = last.off + (long)sizeof(double) * fleet_snap_doubles(last.n);
    const int panels = f->ld / RFLEET_SNAP_PANEL;
    f->snap_rec.clear();
    for (int g = 0; g < count; ++g) {
        const rfleet_snapshot_member m = snap_entry(blob, g);
        const int b = members ? members[g] : m.member;
        for (int p = 0; p < panels; ++p) f->snap_rec.push_back(FleetSnapRec{b, p, m.n, m.flags, (m.off - lo) / (long)sizeof(double)});
    }
    const size_t table = align128(sizeof(FleetSnapRec) * f->snap_rec.size()), payload = (size_t)(hi - lo);
    FLEET_HIP(f, hipSetDevice(f->device));
    const int rr = snap_reserve(f, table + payload);
    if (rr != REKF_OK) return rr;
    FleetSnapLaunch L{};
    L.rec = (const FleetSnapRec *)f->snap_dev;
    L.buf = (double *)(f->snap_dev + table);
    L.cap = (long)(payload / sizeof(double));
    L.count = (int)f->snap_rec.size();
    FLEET_HIP(f, hipMemcpyAsync(f->snap_dev, f->snap_rec.data(), sizeof(FleetSnapRec) * f->snap_rec.size(), hipMemcpyHostToDevice, f->stream));
    FLEET_HIP(f, hipMemcpyAsync(L.buf, (const char *)blob + lo, payload, hipMemcpyHostToDevice, f->stream));
    FLEET_HIP(f, rfleet_launch_unpack(f->dev, L, f->stream));
    const int rs = rfleet_sync(f);
    if (rs != REKF_OK) return rs;
    // ---- the host's part of a member: time, velocity, the pose slot as a launch would have left it, who wrote its match record
    for (int g = 0; g < count; ++g) {
        const rfleet_snapshot_member m = snap_entry(blob, g);
        const int b = members ? members[g] : m.member;
        const char *pay = (const char *)blob + m.off;
        FleetPoseSlot &p = f->pose_host[b];
        memcpy(p.mu3, pay, sizeof(p.mu3));
        for (int j = 0; j < 3; ++j)
            for (int i = j; i < 3; ++i) {
                double v;
                memcpy(&v, pay + sizeof(double) * (size_t)(m.n + ((long)j * m.n - (long)j * (j - 1) / 2) + (i - j)), sizeof(v));
                p.C9[i + 3 * j] = v;
                p.C9[j + 3 * i] = v;
            }
        p.n = m.n;
        p.flags = m.flags;
        f->time[(size_t)b] = m.t;
        for (int k = 0; k < 3; ++k) f->vt[3 * (size_t)b + k] = m.vt[k];
        f->map_rec[(size_t)b] = 0;
        f->rec_wide[(size_t)b] = 0;
    }
    return REKF_OK;
}

}  // extern "C"
