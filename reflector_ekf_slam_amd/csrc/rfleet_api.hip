// rfleet_api.hip -- host side of the fleet filter (include/rfleet.h): the handle and its buffers, the host's time / velocity mirror,
// the pinned staging ring, one launch per rfleet_submit, the fleet's shared pre-loaded map, the getters.
//
// rfleet_submit is five steps, one function each.  Validate, plan, lay out and pack need no HIP call and stand in fleet_host.h, which
// describes them and the segment (tests/cpp/fleet_submit_host.cpp runs them without a GPU).  Time and vt_ are host state: the plan
// decides HandleOdometryMessage's `t < state time` test (cc:211-212) and the use_imu switch on a copy of the mirror, and every packed
// event carries its own dt and velocity.  The fifth, submit_launch, takes a segment of a ring of pinned buffers, which the kernel
// reads in place -- reused only after the launch that read it has finished (one hipEvent per segment), so consecutive submits do not
// synchronise until the ring has gone round --, grows it, packs, fills FleetLaunch, launches and commits: who wrote the scanned
// members' match records, the wide counters, the mirror, the segment's event.  The steps' scratch lives on the handle.
//
// The buffers are batch_host.h's aggregates, held by value and released by rfleet_destroy's release_all: Device for the members'
// arrays (FleetDev is filled from them), the map, the wide records and the snapshot staging; PinnedDefault (default flags, then its
// device pointer) for the pose slots, the reflector rows and every ring segment.  What grows or is replaced goes through
// batch_host's reserve / replace: the new one first, the old one released only after everything that can fail has succeeded.
//
// The map (rfleet_set_map) is one device buffer per fleet and a byte per member.  A submit takes k_fleet_step_map only when a member
// with events in it uses a non-empty map.  The other two kernels never touch FleetMemberCtl::n_map / map_pairs, so the host remembers
// per member who wrote its last scan's record: last_rec (fleet_host.h's LastRec), written by the commit and rfleet_restore, read by
// last_match_body.
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
// member's FleetWideRec: LastRec::Wide.
//
// Snapshot and restore (rfleet_snapshot / rfleet_restore / rfleet_snapshot_peek).  The blob's header and entries are written and read
// by the host; the payloads move between the members' arrays and ONE device staging buffer (allocated on first use, grown to what a
// call needs) by one launch of k_fleet_pack / k_fleet_unpack (fleet_snapshot.hip) over a host-built table of (member, panel) records
// that sits in front of the payload in the same buffer; snap_stage is the device half both calls share.  Every copy goes through
// the handle's stream and is followed by a synchronisation: the stream is non-blocking, so a legacy hipMemcpy would not be ordered
// behind it.
//
// A linked submit (rfleet_submit_linked; include/rlink.h, fleet_link.h) is rfleet_submit's five steps with the link handed to the
// first four.  Step five then puts, in front of the step launch and on the same stream: a wait for the detector's `ready` event, ONE
// launch of k_fleet_bind (fleet_link.hip) over the segment's FleetBindRec table -- it writes the centres and the counts into the
// segment the step kernel is about to read --, and the record of the detector's `consumed` event.  The host waits for nothing.  The
// binds' status records go to one pinned buffer on the handle (link_stat), which only the device writes: what the host knows by itself
// (an entry without a record) it keeps in link_known, so a bind of an earlier call that is still in flight cannot overwrite it.
#include "batch_host.h"
#include "fleet_host.h"
#include "fleet_reflectors.h"

#include <string>

using namespace batch_host;
using namespace fleet_host;

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

struct Segment {
    PinnedDefault<char> buf;
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
    FleetDev dev{};                         // the kernels' view of the next six and `pose`
    Device<double> mu, P, W, Kn;
    Device<FleetMemberCtl> ctl; Device<FleetMemberOpt> opt;
    PinnedDefault<FleetPoseSlot> pose;
    std::vector<rekf_options> opts;
    std::vector<double> time, vt;           // the host's mirror: state time [B], vt_ [B][3]
    Segment seg[kSegs];
    int next_seg = 0;
    std::string hip_error;
    // the shared map: device copies and the host's copy of the per-member switch
    Device<float> map_xy; Device<double> map_cov;
    Device<unsigned char> map_use_dev;
    int M_map = 0;
    std::vector<unsigned char> map_use;
    std::vector<LastRec> last_rec;          // [B]: where each member's last match record lives
    // rfleet_get_reflectors: ONE pinned allocation, ell5 [R][5] | xy2 [R][2] | cov4 [R][4] | counts [B] | members [B], R = B max_landmarks
    PinnedDefault<char> refl;
    SubmitScratch sub;                      // scratch of rfleet_submit; sub.cnt also serves the member-list checks
    // the pose track: the switch, the bound per member, the per-member log and what it has discarded since the last take
    bool tracking = false;
    long track_max = kTrackDefault;
    std::vector<TrackLog> track_log;
    std::vector<long> track_lost;
    // wide scans: the switch, the members' wide match records (allocated when first switched on), rfleet_wide_counts' counters
    bool wide = false;
    Device<FleetWideRec> wide_rec;
    long wide_launches = 0, wide_scans = 0;
    // linked submits: the binds' status records (device-written), the last linked call's scans (1 = the host knows the scan is empty),
    // whether that call's emptied scans are counted yet, rfleet_link_counts' counters
    PinnedDefault<FleetLinkStatus> link_stat;
    size_t link_stat_cap = 0;
    std::vector<unsigned char> link_known, link_known_next;
    bool link_counted = true;
    long link_submits = 0, link_binds = 0, link_scans = 0, link_emptied = 0;
    // snapshot / restore: the device staging buffer (table | payload); host scratch: the table, the payload offsets, a restore's targets
    Device<char> snap;
    size_t snap_cap = 0;
    std::vector<FleetSnapRec> snap_rec;
    std::vector<long> snap_off;
    std::vector<int> snap_target;
};

#define FLEET_HIP(f, ...)                                                      \
    do {                                                                       \
        hipError_t e_ = (__VA_ARGS__);                                         \
        if (e_ != hipSuccess) {                                                \
            (f)->hip_error = std::string(#__VA_ARGS__) + ": " + hipGetErrorString(e_); \
            return REKF_ERR_HIP;                                               \
        }                                                                      \
    } while (0)

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
        TrackLog &log = f->track_log[(size_t)m.member];
        log.buf.push_back(r);
        f->track_lost[(size_t)m.member] += log.trim(f->track_max);
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
        s.buf.release();
    }
    release_all(f->mu, f->P, f->W, f->Kn, f->ctl, f->opt, f->pose, f->refl, f->map_xy, f->map_cov, f->map_use_dev, f->wide_rec, f->snap,
                f->link_stat);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

static int fleet_create_body(rfleet_t *f, const rekf_options *opts)
{
    const int B = f->B;
    const size_t ld = (size_t)f->ld;
    FLEET_HIP(f, hipSetDevice(f->device));
    FLEET_HIP(f, hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    FLEET_HIP(f, f->mu.alloc(ld * B));
    FLEET_HIP(f, f->P.alloc(ld * ld * B));
    FLEET_HIP(f, f->W.alloc(ld * RFLEET_PANEL_COLS * B));
    FLEET_HIP(f, f->Kn.alloc(ld * RFLEET_PANEL_COLS * B));
    FLEET_HIP(f, f->ctl.alloc((size_t)B));
    FLEET_HIP(f, f->opt.alloc((size_t)B));
    FLEET_HIP(f, f->pose.alloc((size_t)B));
    FLEET_HIP(f, f->refl.alloc(refl_bytes(f)));
    f->dev.mu = f->mu.d; f->dev.P = f->P.d; f->dev.W = f->W.d; f->dev.Kn = f->Kn.d;
    f->dev.ctl = f->ctl.d; f->dev.opt = f->opt.d; f->dev.pose = f->pose.dv;
    FLEET_HIP(f, hipMemset(f->dev.mu, 0, sizeof(double) * ld * B));
    FLEET_HIP(f, hipMemset(f->dev.P, 0, sizeof(double) * ld * ld * B));
    FLEET_HIP(f, hipMemset(f->dev.W, 0, sizeof(double) * ld * RFLEET_PANEL_COLS * B));
    FLEET_HIP(f, hipMemset(f->dev.Kn, 0, sizeof(double) * ld * RFLEET_PANEL_COLS * B));
    std::vector<FleetMemberCtl> ctl((size_t)B);
    std::vector<FleetMemberOpt> dopt((size_t)B);
    std::vector<double> mu(ld * B, 0.0);
    memset(ctl.data(), 0, sizeof(FleetMemberCtl) * B);
    memset(f->pose.h, 0, sizeof(FleetPoseSlot) * B);
    for (int i = 0; i < B; ++i) {
        const rekf_options &o = opts[i];
        ctl[i].n = 3;
        dopt[i] = FleetMemberOpt{o.linear_velocity_cov, o.angular_velocity_cov, o.observation_cov, odom_model_of(o), 0};
        for (int k = 0; k < 3; ++k) {
            mu[(size_t)i * ld + k] = o.init_pose[k];
            f->pose.h[i].mu3[k] = o.init_pose[k];
        }
        f->pose.h[i].n = 3;
        f->time[i] = o.init_time;
    }
    FLEET_HIP(f, hipMemcpy(f->dev.ctl, ctl.data(), sizeof(FleetMemberCtl) * B, hipMemcpyHostToDevice));
    FLEET_HIP(f, hipMemcpy(f->opt.d, dopt.data(), sizeof(FleetMemberOpt) * B, hipMemcpyHostToDevice));
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
    f->dev.ld = f->ld; f->dev.n_max = f->n_max; f->dev.B = B;
    f->opts.assign(opts, opts + B);
    f->time.assign((size_t)B, 0.0);
    f->vt.assign((size_t)3 * B, 0.0);
    f->sub.cnt.resize((size_t)B);
    f->sub.pos.resize((size_t)B);
    f->map_use.assign((size_t)B, 0);
    f->last_rec.assign((size_t)B, LastRec::None);
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

// ---- step 5 of a submit: a ring segment of p.need bytes, the launch over it, and the commit
static int submit_launch(rfleet_t *f, const rfleet_event *ev, const SubmitPlan &p, const rlink *link = nullptr)
{
    FLEET_HIP(f, hipSetDevice(f->device));
    if ((size_t)p.n_linked > f->link_stat_cap) {                           // (a bind in flight writes the old buffer: wait before it goes)
        const int rc = rfleet_sync(f);
        if (rc != REKF_OK) return rc;
        FLEET_HIP(f, reserve(f->link_stat, f->link_stat_cap, (size_t)p.n_linked, 256));
    }
    Segment &s = f->seg[f->next_seg];
    if (s.busy) {
        FLEET_HIP(f, hipEventSynchronize(s.done));
        s.busy = false;
    }
    if (s.n_track) track_harvest(f, s);                                    // (the oldest segment: every later record comes behind these)
    FLEET_HIP(f, reserve(s.buf, s.cap, p.need, 4096));
    submit_pack(ev, p, f->sub, s.buf.h, s.meta, link, &f->link_known_next);
    const char *dv = s.buf.dv;
    FleetLaunch L{};
    L.members = (const int *)(dv + p.off_mem);
    L.ev_begin = (const int *)(dv + p.off_beg);
    L.ev = (const FleetEvent *)(dv + p.off_ev);
    L.obs = (const float *)(dv + p.off_obs);
    L.fix = p.n_fix ? (const double *)(dv + p.off_fix) : nullptr;         // (NULL selects the kernel without the pose phase)
    L.G = p.G;
    if (p.with_map) {                                                      // (M_map > 0 selects the kernel with the map branch)
        L.map_xy = f->map_xy.d;
        L.map_cov = f->map_cov.d;
        L.map_use = f->map_use_dev.d;
        L.M_map = f->M_map;
    }
    if (p.tracked) L.track = (FleetTrackRec *)(s.buf.dv + p.off_track);    // (non-NULL selects k_fleet_step_track, the map kernel's body)
    if (p.n_bind > 0) {                                                    // the centres and the counts into the segment, on the device
        if (link->ready) FLEET_HIP(f, hipStreamWaitEvent(f->stream, (hipEvent_t)link->ready, 0));
        FleetBindLaunch Lb{};
        Lb.bind = (const FleetBindRec *)(dv + p.off_bind);
        Lb.ev = (FleetEvent *)(s.buf.dv + p.off_ev);
        Lb.obs = (float *)(s.buf.dv + p.off_obs);
        Lb.status = f->link_stat.dv;
        Lb.records = (const char *)link->records;
        Lb.record_bytes = link->record_bytes;
        Lb.k_off = link->k_off; Lb.err_off = link->err_off; Lb.centers_off = link->centers_off; Lb.max_centers = link->max_centers;
        Lb.max_obs = p.max_obs;
        Lb.n_bind = p.n_bind;
        FLEET_HIP(f, rfleet_launch_bind(Lb, f->stream));
    }
    if (p.n_linked > 0 && link->consumed) FLEET_HIP(f, hipEventRecord((hipEvent_t)link->consumed, f->stream));
    if (p.wide_launch) FLEET_HIP(f, rfleet_launch_step_wide(f->dev, L, f->wide_rec.d, f->stream));   // (fix, map and track: chosen in the kernel)
    else FLEET_HIP(f, rfleet_launch_step(f->dev, L, f->stream));
    // ---- commit: the launch is in the stream
    if (p.tracked) {
        s.n_track = p.E;
        s.track = (const FleetTrackRec *)(s.buf.h + p.off_track);
    }
    for (int b : f->sub.scanned) f->last_rec[(size_t)b] = p.rec;
    f->wide_launches += p.wide_launch;
    if (p.n_linked > 0) {
        f->link_known.swap(f->link_known_next);
        f->link_counted = false;
        f->link_submits += 1;
        f->link_binds += p.n_bind > 0;
        f->link_scans += p.n_linked;
    }
    f->wide_scans += p.n_wide;
    f->time.swap(f->sub.time);
    f->vt.swap(f->sub.vt);
    FLEET_HIP(f, hipEventRecord(s.done, f->stream));
    s.busy = true;
    f->next_seg = (f->next_seg + 1) % kSegs;
    return REKF_OK;
}

int rfleet_submit(rfleet_t *f, const rfleet_event *ev, int count)
{
    if (!f || count < 0 || (count > 0 && !ev)) return REKF_ERR_INVALID;
    const int rc = submit_validate(ev, count, f->B, f->wide);
    if (rc != REKF_OK || count == 0) return rc;
    SubmitPlan p = submit_plan(ev, count, f->opts, f->time, f->vt, f->tracking, f->M_map, f->map_use, f->sub, nullptr, f->wide);
    if (p.E == 0) return REKF_OK;                                          // (every event dropped, untracked: no launch)
    submit_layout(p);
    return submit_launch(f, ev, p);
}

int rfleet_submit_linked(rfleet_t *f, const rfleet_event *ev, int count, const rlink *link)
{
    if (!f || count < 0 || (count > 0 && !ev)) return REKF_ERR_INVALID;
    const int rc = submit_validate(ev, count, f->B, f->wide, link, f->device, f->tracking, &f->sub);
    if (rc != REKF_OK || count == 0) return rc;
    SubmitPlan p = submit_plan(ev, count, f->opts, f->time, f->vt, f->tracking, f->M_map, f->map_use, f->sub, link, f->wide);
    if (p.E == 0) return REKF_OK;                                          // (every event dropped, untracked: no launch)
    submit_layout(p);
    return submit_launch(f, ev, p, link);
}

int rfleet_sizeof_link(void) { return (int)sizeof(rlink); }

int rfleet_link_status(rfleet_t *f, int *taken, int *status, int *K_seen, int cap)
{
    if (!f || cap < 0) return REKF_ERR_INVALID;
    const int n = (int)f->link_known.size();
    if (n > cap) return REKF_ERR_BUFFER;
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    long emptied = 0;
    for (int i = 0; i < n; ++i) {
        const FleetLinkStatus st = f->link_known[(size_t)i] ? FleetLinkStatus{0, 0, 0, 0} : f->link_stat.h[i];
        if (taken) taken[i] = st.taken;
        if (status) status[i] = st.status;
        if (K_seen) K_seen[i] = st.K_seen;
        emptied += st.status != 0;
    }
    if (!f->link_counted) f->link_emptied += emptied;
    f->link_counted = true;
    return n;
}

int rfleet_link_counts(rfleet_t *f, long *submits, long *binds, long *scans, long *emptied)
{
    if (!f) return REKF_ERR_INVALID;
    if (submits) *submits = f->link_submits;
    if (binds) *binds = f->link_binds;
    if (scans) *scans = f->link_scans;
    if (emptied) *emptied = f->link_emptied;
    return REKF_OK;
}

int rfleet_get_poses(rfleet_t *f, double *t, double *mu3, double *sigma3x3)
{
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    for (int b = 0; b < f->B; ++b) {
        const FleetPoseSlot &p = f->pose.h[b];
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
        const FleetPoseSlot &p = f->pose.h[b];
        const rekf_options &o = f->opts[b];
        const double *vt = &f->vt[3 * (size_t)b];
        double C[9];
        memcpy(C, p.C9, sizeof(C));
        Motion mo;
        motion_terms_of(odom_model_of(o), t[b] - f->time[b], vt[0], vt[1], vt[2], o.linear_velocity_cov,
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
    for (int b = 0; b < f->B; ++b) n[b] = f->pose.h[b].n;
    return REKF_OK;
}

int rfleet_get_flags(rfleet_t *f, int *flags)
{
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    if (!flags) return REKF_ERR_INVALID;
    for (int b = 0; b < f->B; ++b) flags[b] = f->pose.h[b].flags;
    return REKF_OK;
}

int rfleet_get_state(rfleet_t *f, int member, double *t, int *n_out, double *mu, long mu_cap, double *sigma, long sigma_cap)
{
    if (!f || member < 0 || member >= f->B) return REKF_ERR_INVALID;
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    const int n = f->pose.h[member].n;
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
    pose_slot_from_lower(f->pose.h[member], mu, n, [&](int i, int j) { return sigma[i + (size_t)j * n]; });
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
    auto read = [&](const auto &r, int n_map) { ns = r.n_state; nm = n_map; nn = r.n_new; sp = r.state_pairs; mp = r.map_pairs; nw = r.new_ids; };
    const LastRec rec = f->last_rec[(size_t)member];
    FleetMemberCtl c;
    std::vector<FleetWideRec> wr(rec == LastRec::Wide ? 1 : 0);
    if (rec == LastRec::Wide) {
        FLEET_HIP(f, hipMemcpy(wr.data(), f->wide_rec.d + member, sizeof(FleetWideRec), hipMemcpyDeviceToHost));
        read(wr[0], wr[0].n_map);
    } else {
        FLEET_HIP(f, hipMemcpy(&c, f->dev.ctl + member, sizeof(c), hipMemcpyDeviceToHost));
        read(c, rec == LastRec::NarrowMap ? c.n_map : 0);                  // (only the map kernel writes the map part of a record)
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
    if (on && !f->wide_rec.d) {                                            // (allocates once; launches nothing)
        FLEET_HIP(f, hipSetDevice(f->device));
        const size_t B = (size_t)f->B;
        auto zeroed = [B](Device<FleetWideRec> &w) {
            const hipError_t e_ = hipMemset(w.d, 0, sizeof(FleetWideRec) * B);
            return e_ == hipSuccess ? hipDeviceSynchronize() : e_;         // (the handle's stream does not wait for the null stream)
        };
        FLEET_HIP(f, replace(f->wide_rec, B, zeroed));
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
    if (M > 0) {                                                           // the new copy first: a failure leaves the old map in place
        const size_t n_xy = 2 * (size_t)M, n_cov = 4 * (size_t)M;
        const hipError_t e = replace(f->map_xy, n_xy, [&](Device<float> &nxy) {
            return replace(f->map_cov, n_cov, [&](Device<double> &ncov) {
                hipError_t e_ = f->map_use_dev.d ? hipSuccess : f->map_use_dev.alloc(B);
                if (e_ == hipSuccess) e_ = hipMemcpy(nxy.d, xy, sizeof(float) * n_xy, hipMemcpyHostToDevice);
                if (e_ == hipSuccess) e_ = hipMemcpy(ncov.d, cov, sizeof(double) * n_cov, hipMemcpyHostToDevice);
                if (e_ == hipSuccess) e_ = hipMemcpy(f->map_use_dev.d, want.data(), B, hipMemcpyHostToDevice);
                return e_;
            });
        });
        if (e != hipSuccess) {
            if (f->map_use_dev.d) (void)hipMemcpy(f->map_use_dev.d, f->map_use.data(), B, hipMemcpyHostToDevice);
            f->hip_error = std::string("rfleet_set_map: ") + hipGetErrorString(e);
            return REKF_ERR_HIP;
        }
    } else {
        release_all(f->map_xy, f->map_cov);
    }
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
    if (!members_named_once(members, count, f->B, f->sub.cnt)) return REKF_ERR_INVALID;
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
    if (!members_named_once(members, count, f->B, f->sub.cnt)) return REKF_ERR_INVALID;
    if (count == 0) return REKF_OK;
    FLEET_HIP(f, hipSetDevice(f->device));
    const size_t R = refl_rows(f);
    const int *h_counts = (const int *)(f->refl.h + refl_off_counts(f));
    FleetReflectorsLaunch L{};
    if (members) {                                                         // (no launch reads the list any more: every call ends in a synchronisation)
        memcpy(f->refl.h + refl_off_members(f), members, sizeof(int) * (size_t)count);
        L.members = (const int *)(f->refl.dv + refl_off_members(f));
    }
    L.count = count;
    L.cap_rows = cap_rows < (long)R ? cap_rows : (long)R;
    L.counts = (int *)(f->refl.dv + refl_off_counts(f));
    L.ell5 = ellipses5 ? (double *)f->refl.dv : nullptr;
    L.xy2 = xy2 ? (double *)(f->refl.dv + refl_off_xy(f)) : nullptr;
    L.cov4 = cov4 ? (double *)(f->refl.dv + refl_off_cov(f)) : nullptr;
    FLEET_HIP(f, rfleet_launch_reflectors(f->dev, L, f->stream));
    const int rc = rfleet_sync(f);
    if (rc != REKF_OK) return rc;
    long rows = 0;
    for (int g = 0; g < count; ++g) {
        counts[g] = h_counts[g];
        rows += h_counts[g];
    }
    if (rows > cap_rows && (ellipses5 || xy2 || cov4)) return REKF_ERR_BUFFER;    // (no output given: the call that asks for the counts)
    if (ellipses5) memcpy(ellipses5, f->refl.h, sizeof(double) * 5 * (size_t)rows);
    if (xy2) memcpy(xy2, f->refl.h + refl_off_xy(f), sizeof(double) * 2 * (size_t)rows);
    if (cov4) memcpy(cov4, f->refl.h + refl_off_cov(f), sizeof(double) * 4 * (size_t)rows);
    return REKF_OK;
}

int rfleet_sizeof_snapshot_member(void) { return (int)sizeof(rfleet_snapshot_member); }

int rfleet_sizeof_snapshot_hdr(void) { return (int)sizeof(rfleet_snapshot_hdr); }

// The device half of a snapshot and of a restore: the staging buffer holds f->snap_rec's table and `payload` bytes behind it (grown
// when it does not: a failed allocation leaves the old one in place), the table is on its way to the device, and L describes both.
static int snap_stage(rfleet_t *f, size_t payload, FleetSnapLaunch &L)
{
    const size_t rows = sizeof(FleetSnapRec) * f->snap_rec.size(), table = align128(rows);
    FLEET_HIP(f, hipSetDevice(f->device));
    FLEET_HIP(f, reserve(f->snap, f->snap_cap, table + payload, (size_t)1 << 16));
    L = FleetSnapLaunch{};
    L.rec = (const FleetSnapRec *)f->snap.d;
    L.buf = (double *)(f->snap.d + table);
    L.cap = (long)(payload / sizeof(double));
    L.count = (int)f->snap_rec.size();
    FLEET_HIP(f, hipMemcpyAsync(f->snap.d, f->snap_rec.data(), rows, hipMemcpyHostToDevice, f->stream));
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
    if (!members_named_once(members, count, f->B, f->sub.cnt)) return REKF_ERR_INVALID;
    const long head = (long)sizeof(rfleet_snapshot_hdr) + (long)sizeof(rfleet_snapshot_member) * count;
    long total = head;
    if (count > 0) {
        const int rc = rfleet_sync(f);                                     // (the pose slots hold every member's n and flags)
        if (rc != REKF_OK) return rc;
        f->snap_off.resize((size_t)count);
        for (int g = 0; g < count; ++g) {
            const int n = f->pose.h[members ? members[g] : g].n;
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
    rfleet_snapshot_hdr h{{}, RFLEET_SNAPSHOT_VERSION, count, total};
    memcpy(h.magic, RFLEET_SNAPSHOT_MAGIC, sizeof(h.magic));
    if (count > 0) {
        f->snap_rec.clear();
        for (int g = 0; g < count; ++g) {
            const int b = members ? members[g] : g;
            const int n = f->pose.h[b].n;
            const long off = (f->snap_off[(size_t)g] - head) / (long)sizeof(double);
            for (int p = 0; p < (n + RFLEET_SNAP_PANEL - 1) / RFLEET_SNAP_PANEL; ++p) f->snap_rec.push_back(FleetSnapRec{b, p, n, 0, off});
        }
        const size_t payload = (size_t)(total - head);
        FleetSnapLaunch L;
        const int rr = snap_stage(f, payload, L);
        if (rr != REKF_OK) return rr;
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
        m.n = f->pose.h[b].n;
        m.flags = f->pose.h[b].flags;
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
    if (count != h.count) return REKF_ERR_INVALID;
    if (count == 0) return REKF_OK;
    std::vector<int> &target = f->snap_target;                             // entry g's member: as listed, else the one it was taken from
    target.resize((size_t)count);
    for (int g = 0; g < count; ++g) {
        const rfleet_snapshot_member m = snap_entry(blob, g);
        if (m.n > f->n_max) return REKF_ERR_INVALID;
        target[(size_t)g] = members ? members[g] : m.member;
    }
    if (!members_named_once(target.data(), count, f->B, f->sub.cnt)) return REKF_ERR_INVALID;
    const int rc = rfleet_sync(f);                                         // no launch touches a target any more
    if (rc != REKF_OK) return rc;
    // ---- the payload's span in the blob, the table of (target, panel of the target's ld) records
    const rfleet_snapshot_member first = snap_entry(blob, 0), last = snap_entry(blob, count - 1);
    const long lo = first.off, hi = last.off + (long)sizeof(double) * fleet_snap_doubles(last.n);
    const int panels = f->ld / RFLEET_SNAP_PANEL;
    f->snap_rec.clear();
    for (int g = 0; g < count; ++g) {
        const rfleet_snapshot_member m = snap_entry(blob, g);
        const int b = target[(size_t)g];
        for (int p = 0; p < panels; ++p) f->snap_rec.push_back(FleetSnapRec{b, p, m.n, m.flags, (m.off - lo) / (long)sizeof(double)});
    }
    const size_t payload = (size_t)(hi - lo);
    FleetSnapLaunch L;
    const int rr = snap_stage(f, payload, L);
    if (rr != REKF_OK) return rr;
    FLEET_HIP(f, hipMemcpyAsync(L.buf, (const char *)blob + lo, payload, hipMemcpyHostToDevice, f->stream));
    FLEET_HIP(f, rfleet_launch_unpack(f->dev, L, f->stream));
    const int rs = rfleet_sync(f);
    if (rs != REKF_OK) return rs;
    // ---- the host's part of a member: time, velocity, the pose slot as a launch would have left it, who wrote its match record
    for (int g = 0; g < count; ++g) {
        const rfleet_snapshot_member m = snap_entry(blob, g);
        const int b = target[(size_t)g];
        const char *pay = (const char *)blob + m.off;
        pose_slot_from_lower(f->pose.h[b], pay, m.n, [&](int i, int j) {   // (column j of the packed triangle holds rows j .. n-1)
            double v;
            memcpy(&v, pay + sizeof(double) * (size_t)(m.n + ((long)j * m.n - (long)j * (j - 1) / 2) + (i - j)), sizeof(v));
            return v;
        });
        f->pose.h[b].flags = m.flags;
        f->time[(size_t)b] = m.t;
        for (int k = 0; k < 3; ++k) f->vt[3 * (size_t)b + k] = m.vt[k];
        f->last_rec[(size_t)b] = LastRec::None;
    }
    return REKF_OK;
}

}  // extern "C"
