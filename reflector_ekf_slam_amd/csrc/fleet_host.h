// fleet_host.h -- what the fleet filter's host side (rfleet_api.hip) does without a HIP call: plain C++ over fleet_dev.h's structs and
// rfleet.h's rfleet_event, built and run without a GPU by tests/cpp/fleet_submit_host.cpp.  The first four of rfleet_submit's steps:
//   1 submit_validate   every event, before anything moves; touches no state
//   2 submit_plan       which events reach the device, each with its dt and velocity, on a COPY of the time / velocity mirror;
//                       the per-member counts, n_obs, n_fix, n_wide, the scanned members, G, E, with_map, who will own the records
//   3 submit_layout     the byte offsets of the segment's parts and `need`
//   4 submit_pack       the segment's bytes into a given range of `need` bytes, and the TrackMeta of a tracked submit
// (5, submit_launch in rfleet_api.hip: take and grow the ring segment, fill FleetLaunch, launch, commit.)  A segment is
//   members[G] | ev_begin[G + 1] | FleetEvent[E] | fix[3 n_fix] | obs[2 n_obs]   each at the next 16-byte boundary, and for a tracked
// submit | FleetTrackRec[E] at the next 128-byte boundary; events grouped by member, stable: a member's events keep their order.
// A linked submit (rfleet_submit_linked: scans of kind RFLEET_EV_SCAN_LINKED, whose observations a fleet detector's launch is still
// producing; fleet_link.h) goes through the same four steps, given the rlink: a linked scan whose entry has a record reserves
// 2 * max_obs floats of obs (max_obs = 32, 256 on a fleet with wide scans on) and is packed with K = 0, and the segment grows a fifth
// part | FleetBindRec[n_bind] at the next 16-byte boundary behind obs's slack, which k_fleet_bind walks; an entry without a record
// (record == -1: the detector's host knows K = 0) is packed as the empty scan it is.  Without a linked scan nothing differs by a byte.
// Also here: the getters' member-list check, a snapshot blob's validation, a pose slot from a lower triangle, the odometry model.
#pragma once
#include "fleet_snapshot.h"
#include "fleet_link.h"
#include "../../include/rfleet.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace fleet_host {
namespace {

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t align128(size_t v) { return (v + 127) & ~(size_t)127; }

// FleetMemberOpt::model / motion_terms_of's model of a member's options (cc:13-32: anything but DIFF is OMNI)
inline int odom_model_of(const rekf_options &o) { return (o.odom_model == REKF_ODOM_DIFF) ? 0 : 1; }

// Where member b's last match record lives: FleetMemberCtl (a narrow launch; its map part is valid only when the map or the track
// kernel wrote it -- the other two never touch n_map / map_pairs) or FleetWideRec (a wide launch, narrow scans of it included).
// None: no scan yet, or a restore -- FleetMemberCtl's zero counts.
enum class LastRec : unsigned char { None, Narrow, NarrowMap, Wide };

struct TrackMeta { double t; int member, kind, K, dropped; };   // what the host knows of a packed event of a tracked submit

// the per-call scratch of a submit, kept on the handle: a steady-state submit allocates nothing
struct SubmitScratch {
    std::vector<int> cnt, pos;              // [B]: a member's events in the call; where its next event is packed
    std::vector<int> order, scanned;        // the events that reach the device, in call order; the members with a scan among them
    std::vector<double> time, vt;           // the mirror's copy: committed behind the launch
    std::vector<double> dts;                // [count][4]: dt and the velocity of event i
    std::vector<unsigned char> dropped;     // a tracked submit: event i is one the untracked path drops
    std::vector<unsigned char> link_used;   // a linked submit: entry k of the link is named by an event of the call
};

struct SubmitPlan {
    bool tracked = false, with_map = false; // with_map: a member with events matches against a non-empty map
    int E = 0, G = 0;                       // packed events; members with events
    size_t n_obs = 0, n_fix = 0, n_wide = 0;   // n_wide: scans of the call with K > RFLEET_MAX_OBS
    LastRec rec = LastRec::None;            // who owns the match record of every scanned member behind this launch
    size_t off_mem = 0, off_beg = 0, off_ev = 0, off_fix = 0, off_obs = 0, off_track = 0, need = 0;
    // a linked submit: linked scans of the call, those with a record (one workgroup of k_fleet_bind each), the pairs reserved for each
    int n_linked = 0, n_bind = 0, max_obs = RFLEET_MAX_OBS;
    bool wide_launch = false;               // k_fleet_step_wide: a scan known to be wide, or on a wide fleet one whose K only the device knows
    size_t off_bind = 0;
};

static_assert(FLEET_LINK_ERR_TOO_MANY_OBS == REKF_ERR_TOO_MANY_OBS, "fleet_link.h restates rekf.h's code");

// what rfleet_submit_linked asks of the link itself before any of its entries is looked at
inline bool link_well_formed(const rlink &l)
{
    if (l.count < 0) return false;
    if (l.count > 0 && (!l.member || !l.stamp || !l.host_status || !l.record)) return false;
    if (l.record_bytes <= 0 || (l.record_bytes & 7) || l.max_centers < 1) return false;
    if (l.k_off < 0 || (l.k_off & 3) || l.err_off < 0 || (l.err_off & 3) || l.centers_off < 0 || (l.centers_off & 7)) return false;
    if ((long)l.k_off + 4 > l.record_bytes || (long)l.err_off + 4 > l.record_bytes) return false;
    return (long)l.centers_off + 8 * (long)l.max_centers <= l.record_bytes;
}

// ---- 1: validate everything before anything moves
// link: the rlink of an rfleet_submit_linked (NULL: rfleet_submit, which refuses a linked scan); device, tracked: the fleet's;
// s: link_used is the scratch of the "an entry used twice" test.
inline int submit_validate(const rfleet_event *ev, int count, int B, bool wide, const rlink *link = nullptr, int device = 0,
                           bool tracked = false, SubmitScratch *s = nullptr)
{
    const int max_obs = wide ? RFLEET_MAX_OBS_WIDE : RFLEET_MAX_OBS;
    if (link) {
        if (!s || !link_well_formed(*link)) return REKF_ERR_INVALID;
        s->link_used.assign((size_t)link->count, 0);
    }
    for (int i = 0; i < count; ++i) {
        const rfleet_event &e = ev[i];
        if (e.member < 0 || e.member >= B) return REKF_ERR_INVALID;
        if (e.kind == RFLEET_EV_SCAN_LINKED) {
            // (TrackMeta::K is the host's: a tracked fleet takes no scan whose K only the device knows)
            if (!link || tracked || link->device != device) return REKF_ERR_INVALID;
            const int k = e.K;
            if (k < 0 || k >= link->count || s->link_used[(size_t)k]) return REKF_ERR_INVALID;
            s->link_used[(size_t)k] = 1;
            if (link->member[k] != e.member || link->host_status[k] != 0) return REKF_ERR_INVALID;
            if (link->record[k] < -1 || link->record[k] >= link->count || (link->record[k] >= 0 && !link->records)) return REKF_ERR_INVALID;
            if (e.has_pose_fix && !(std::isfinite(e.pose_fix[0]) && std::isfinite(e.pose_fix[1]) && std::isfinite(e.pose_fix[2])))
                return REKF_ERR_INVALID;
            continue;
        }
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
    return REKF_OK;
}

// ---- 2: which events reach the device; time [B] / vt [B][3] are the mirror.  p.E == 0 (every event dropped, untracked): no launch.
inline SubmitPlan submit_plan(const rfleet_event *ev, int count, const std::vector<rekf_options> &opts, const std::vector<double> &time,
                              const std::vector<double> &vt, bool tracked, int M_map, const std::vector<unsigned char> &map_use,
                              SubmitScratch &s, const rlink *link = nullptr, bool wide = false)
{
    SubmitPlan p;
    p.tracked = tracked;
    p.max_obs = wide ? RFLEET_MAX_OBS_WIDE : RFLEET_MAX_OBS;
    if (tracked) s.dropped.assign((size_t)count, 0);
    s.time = time;
    s.vt = vt;
    s.order.clear();
    s.scanned.clear();
    std::fill(s.cnt.begin(), s.cnt.end(), 0);
    s.dts.resize((size_t)count * 4);
    for (int i = 0; i < count; ++i) {
        const rfleet_event &e = ev[i];
        const int b = e.member;
        if (e.kind == RFLEET_EV_ODOM) {
            if (opts[b].use_imu || e.t < s.time[b]) {                      // cc:213-223: odometry is ignored with use_imu; cc:211-212
                if (!tracked) continue;
                s.dropped[(size_t)i] = 1;                                  // (the node still publishes the unchanged pose: a record, no Predict)
                for (int k = 0; k < 4; ++k) s.dts[4 * (size_t)i + k] = 0.0;
                s.cnt[b]++;
                s.order.push_back(i);
                continue;
            }
            for (int k = 0; k < 3; ++k) s.vt[3 * b + k] = e.v[k];          // cc:216
        } else if (e.kind == RFLEET_EV_SCAN_LINKED) {
            const bool bound = link->record[e.K] >= 0;                     // (e.K: the entry; the scan's own K is the device's to tell)
            p.n_linked += 1;
            p.n_bind += bound ? 1 : 0;
            p.n_obs += bound ? (size_t)p.max_obs : 0;
            p.n_fix += e.has_pose_fix ? 1 : 0;
            s.scanned.push_back(b);
        } else {
            p.n_obs += (size_t)e.K;
            p.n_fix += e.has_pose_fix ? 1 : 0;
            p.n_wide += e.K > RFLEET_MAX_OBS ? 1 : 0;
            s.scanned.push_back(b);
        }
        s.dts[4 * (size_t)i] = e.t - s.time[b];                            // cc:217-218 / :232-233
        for (int k = 0; k < 3; ++k) s.dts[4 * (size_t)i + 1 + k] = s.vt[3 * b + k];
        s.time[b] = e.t;
        s.cnt[b]++;
        s.order.push_back(i);
    }
    p.E = (int)s.order.size();
    for (size_t b = 0; b < s.cnt.size(); ++b) {
        p.G += s.cnt[b] > 0;
        p.with_map = p.with_map || (s.cnt[b] > 0 && M_map > 0 && map_use[b]);
    }
    p.wide_launch = p.n_wide > 0 || (wide && p.n_bind > 0);               // (K > 32 may come out of a record: the host cannot know)
    p.rec = p.wide_launch ? LastRec::Wide : (p.with_map || tracked) ? LastRec::NarrowMap : LastRec::Narrow;
    return p;
}

// ---- 3: the segment's parts
inline void submit_layout(SubmitPlan &p)
{
    p.off_beg = align16(p.off_mem + sizeof(int) * p.G);
    p.off_ev = align16(p.off_beg + sizeof(int) * (p.G + 1));
    p.off_fix = align16(p.off_ev + sizeof(FleetEvent) * p.E);
    p.off_obs = align16(p.off_fix + sizeof(double) * 3 * p.n_fix);
    p.need = align16(p.off_obs + sizeof(float) * 2 * p.n_obs + 16);
    p.off_track = align128(p.need);                                        // a tracked submit: | track[E], one 128-byte line each
    if (p.tracked) p.need = p.off_track + sizeof(FleetTrackRec) * (size_t)p.E;
    if (p.n_bind > 0) {                                                    // (never tracked: validated)
        p.off_bind = align16(p.need);
        p.need = p.off_bind + sizeof(FleetBindRec) * (size_t)p.n_bind;
    }
}

// ---- 4: the segment's bytes into seg[0, p.need) (the track area is the kernel's to write), meta[E] of a tracked submit
// link_known (a linked submit): per linked scan of the call, in event order, 1 = the host knows it is empty (no record, no bind)
inline void submit_pack(const rfleet_event *ev, const SubmitPlan &p, SubmitScratch &s, char *seg, std::vector<TrackMeta> &meta,
                        const rlink *link = nullptr, std::vector<unsigned char> *link_known = nullptr)
{
    int *members = (int *)(seg + p.off_mem), *ev_begin = (int *)(seg + p.off_beg);
    FleetEvent *pev = (FleetEvent *)(seg + p.off_ev);
    double *pfix = (double *)(seg + p.off_fix);
    float *pobs = (float *)(seg + p.off_obs);
    int g = 0, acc = 0;
    for (size_t b = 0; b < s.cnt.size(); ++b) {
        if (s.cnt[b] == 0) continue;
        members[g] = (int)b;
        ev_begin[g] = acc;
        s.pos[b] = acc;
        acc += s.cnt[b];
        ++g;
    }
    ev_begin[p.G] = acc;
    size_t obs_at = 0;
    int fix_at = 0, bind_at = 0, slot = 0;
    FleetBindRec *pbind = (FleetBindRec *)(seg + p.off_bind);
    if (link_known) link_known->clear();
    if (p.tracked) meta.resize((size_t)p.E);
    for (int q = 0; q < p.E; ++q) {
        const int i = s.order[q];
        const rfleet_event &e = ev[i];
        const int at = s.pos[e.member]++;
        FleetEvent &pe = pev[at];
        if (p.tracked) {
            const int dr = s.dropped[(size_t)i];
            meta[(size_t)at] = TrackMeta{e.t, e.member, e.kind, e.kind == RFLEET_EV_SCAN ? e.K : 0, dr};
            if (dr) {
                pe = FleetEvent{0.0, {0.0, 0.0, 0.0}, 2, 0, (int)obs_at, -1};
                continue;
            }
        }
        pe.dt = s.dts[4 * (size_t)i];
        for (int k = 0; k < 3; ++k) pe.vt[k] = s.dts[4 * (size_t)i + 1 + k];
        const bool linked = e.kind == RFLEET_EV_SCAN_LINKED;
        pe.kind = (e.kind == RFLEET_EV_SCAN || linked) ? 1 : 0;
        pe.K = (e.kind == RFLEET_EV_SCAN) ? e.K : 0;                       // (a linked scan: 0 until k_fleet_bind says otherwise)
        pe.obs_off = (int)obs_at;
        pe.fix_off = -1;
        if (linked) {
            const int record = link->record[e.K];
            if (link_known) link_known->push_back(record < 0);
            if (record >= 0) {
                pbind[bind_at++] = FleetBindRec{at, (int)obs_at, record, slot};
                obs_at += 2 * (size_t)p.max_obs;
            }
            ++slot;
        }
        if ((e.kind == RFLEET_EV_SCAN || linked) && e.has_pose_fix) {
            pe.fix_off = fix_at;
            for (int k = 0; k < 3; ++k) pfix[fix_at + k] = e.pose_fix[k];
            fix_at += 3;
        }
        if (pe.K > 0) {
            memcpy(pobs + obs_at, e.xy, sizeof(float) * 2 * (size_t)pe.K);
            obs_at += 2 * (size_t)pe.K;
        }
    }
}

// `members` names each of its `count` members once and inside 0 .. B-1, or is NULL with count == B (all members in order).
// cnt: scratch [B].
inline bool members_named_once(const int *members, int count, int B, std::vector<int> &cnt)
{
    if (!members) return count == B;
    if (count > B) return false;                                           // (more than B members: one is listed twice)
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int g = 0; g < count; ++g)
        if (members[g] < 0 || members[g] >= B || cnt[members[g]]++) return false;
    return true;
}

// a member's pose slot from its mean and a lower triangle: lower(i, j), i >= j, is the covariance's entry; flags stay
template <typename Lower>
inline void pose_slot_from_lower(FleetPoseSlot &p, const void *mu3, int n, Lower &&lower)
{
    memcpy(p.mu3, mu3, sizeof(p.mu3));
    for (int j = 0; j < 3; ++j)
        for (int i = j; i < 3; ++i) p.C9[i + 3 * j] = p.C9[j + 3 * i] = lower(i, j);
    p.n = n;
}

// entry g of a blob (a blob need not be aligned: a file's bytes)
inline rfleet_snapshot_member snap_entry(const void *blob, int g)
{
    rfleet_snapshot_member m;
    memcpy(&m, (const char *)blob + sizeof(rfleet_snapshot_hdr) + sizeof(m) * (size_t)g, sizeof(m));
    return m;
}

// what rfleet_snapshot_peek promises of a blob
inline int snap_validate(const void *blob, long bytes, rfleet_snapshot_hdr *hdr, int *max_n)
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

}  // namespace
}  // namespace fleet_host
