// Stand-alone driver of what a linked submit (rfleet_submit_linked, include/rfleet.h) does without a HIP call: csrc/fleet_host.h's
// submit_validate, submit_plan, submit_layout and submit_pack given an rlink, and csrc/fleet_link.h's fleet_link_take -- the very
// function k_fleet_bind compiles for the device.  Built host-only by tests/test_fleet_link_host_cpu.py's fixture and run without a
// GPU, against that test's own text of the rules.
//
//   fleet_link_host IN      IN holds records, each answered on stdout:
//     "take K err max_centers max_obs"          -> "take <taken> <status>"
//     "submit B wide tracked M_map device as_linked n_link link_device count", then B lines "use_imu time vx vy wz map_use", then
//     n_link lines "member stamp host_status record" (n_link = -1: no link, a NULL pointer), then per event one line
//     "member kind t vx vy wz K has_fix fx fy fyaw xy_null" followed by 2 K floats for a host scan (kind 2: K is the link's entry)
//       as_linked = 0: the steps called as rfleet_submit calls them (no link anywhere); 1: as rfleet_submit_linked does
//       -> "rc <code>", "mirror <time[B]> <vt[3B]>" (the handle's mirror behind the call: never touched), and when rc is 0
//          "plan E G n_obs n_fix n_wide with_map rec n_linked n_bind max_obs wide_launch", "cnt <B>", "scanned ...",
//          "next <time[B]> <vt[3B]>", "layout off_mem off_beg off_ev off_fix off_obs off_track off_bind need", "seg <2 need hex
//          digits>" (a heap buffer of exactly `need` bytes, pre-filled with 0xA5) and "known <0|1 per linked scan>"
#include "../../reflector_ekf_slam_amd/csrc/fleet_host.h"

#include <cstdio>
#include <string>

using namespace fleet_host;

static void print_mirror(const char *name, const std::vector<double> &time, const std::vector<double> &vt)
{
    std::printf("%s", name);
    for (double v : time) std::printf(" %a", v);
    for (double v : vt) std::printf(" %a", v);
    std::printf("\n");
}

static int run_take(FILE *f)
{
    int K, err, max_centers, max_obs, status = 12345;
    if (std::fscanf(f, "%d %d %d %d", &K, &err, &max_centers, &max_obs) != 4) return 4;
    const int taken = fleet_link_take(K, err, max_centers, max_obs, &status);
    std::printf("take %d %d\n", taken, status);
    return 0;
}

static int run_submit(FILE *f)
{
    int B, wide, tracked, M_map, device, as_linked, n_link, link_device, count;
    if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d", &B, &wide, &tracked, &M_map, &device, &as_linked, &n_link, &link_device, &count) != 9) return 4;
    std::vector<rekf_options> opts((size_t)B);
    std::vector<double> time((size_t)B), vt((size_t)3 * B);
    std::vector<unsigned char> map_use((size_t)B);
    for (int b = 0; b < B; ++b) {
        int imu, use;
        if (std::fscanf(f, "%d %la %la %la %la %d", &imu, &time[b], &vt[3 * b], &vt[3 * b + 1], &vt[3 * b + 2], &use) != 6) return 4;
        opts[b] = rekf_options{};
        opts[b].use_imu = imu;
        map_use[b] = (unsigned char)use;
    }
    const int nl = n_link < 0 ? 0 : n_link;
    std::vector<int> l_member((size_t)nl + 1), l_status((size_t)nl + 1), l_record((size_t)nl + 1);
    std::vector<double> l_stamp((size_t)nl + 1);
    for (int k = 0; k < nl; ++k)
        if (std::fscanf(f, "%d %la %d %d", &l_member[k], &l_stamp[k], &l_status[k], &l_record[k]) != 4) return 4;
    static char records[8];                                   // (never read by the host: only its address is looked at)
    rlink link{};
    link.count = nl; link.device = link_device;
    link.member = l_member.data(); link.stamp = l_stamp.data(); link.host_status = l_status.data(); link.record = l_record.data();
    link.records = records; link.record_bytes = 16 + 8 * 256;
    link.k_off = 0; link.err_off = 8; link.centers_off = 16; link.max_centers = 256;
    const rlink *lp = n_link < 0 ? nullptr : &link;
    std::vector<rfleet_event> ev((size_t)count);
    std::vector<std::vector<float>> clouds((size_t)count);
    for (int i = 0; i < count; ++i) {
        rfleet_event &e = ev[i];
        int xy_null;
        if (std::fscanf(f, "%d %d %la %la %la %la %d %d %la %la %la %d", &e.member, &e.kind, &e.t, &e.v[0], &e.v[1], &e.v[2], &e.K, &e.has_pose_fix,
                        &e.pose_fix[0], &e.pose_fix[1], &e.pose_fix[2], &xy_null) != 12)
            return 4;
        clouds[i].resize((size_t)(e.kind == RFLEET_EV_SCAN && e.K > 0 && !xy_null ? 2 * e.K : 0));
        for (float &v : clouds[i]) {
            double d;
            if (std::fscanf(f, "%la", &d) != 1) return 4;
            v = (float)d;
        }
        e.xy = clouds[i].empty() ? nullptr : clouds[i].data();
    }
    SubmitScratch s;
    s.cnt.resize((size_t)B);
    s.pos.resize((size_t)B);
    const int rc = as_linked ? submit_validate(ev.data(), count, B, wide != 0, lp, device, tracked != 0, &s)
                             : submit_validate(ev.data(), count, B, wide != 0);
    std::printf("rc %d\n", rc);
    SubmitPlan p;
    if (rc == REKF_OK)
        p = as_linked ? submit_plan(ev.data(), count, opts, time, vt, tracked != 0, M_map, map_use, s, lp, wide != 0)
                      : submit_plan(ev.data(), count, opts, time, vt, tracked != 0, M_map, map_use, s, nullptr, wide != 0);
    print_mirror("mirror", time, vt);
    if (rc != REKF_OK) return 0;
    std::printf("plan %d %d %zu %zu %zu %d %d %d %d %d %d\ncnt", p.E, p.G, p.n_obs, p.n_fix, p.n_wide, (int)p.with_map, (int)p.rec, p.n_linked,
                p.n_bind, p.max_obs, (int)p.wide_launch);
    for (int c : s.cnt) std::printf(" %d", c);
    std::printf("\nscanned");
    for (int b : s.scanned) std::printf(" %d", b);
    std::printf("\n");
    print_mirror("next", s.time, s.vt);
    submit_layout(p);
    std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu\nseg ", p.off_mem, p.off_beg, p.off_ev, p.off_fix, p.off_obs, p.off_track, p.off_bind, p.need);
    std::vector<TrackMeta> meta;
    std::vector<unsigned char> known;
    char *seg = new char[p.need];                             // exactly `need` bytes: a write past the end is a sanitizer's finding
    memset(seg, 0xA5, p.need);
    if (p.E > 0) {
        if (as_linked) submit_pack(ev.data(), p, s, seg, meta, lp, &known);
        else submit_pack(ev.data(), p, s, seg, meta);
    }
    for (size_t i = 0; i < p.need; ++i) std::printf("%02x", (unsigned)(unsigned char)seg[i]);
    delete[] seg;
    std::printf("\nknown");
    for (unsigned char k : known) std::printf(" %d", (int)k);
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 3;
    char what[16];
    int rc = 0;
    while (rc == 0 && std::fscanf(f, "%15s", what) == 1) {
        if (std::string(what) == "take") rc = run_take(f);
        else if (std::string(what) == "submit") rc = run_submit(f);
        else rc = 2;
    }
    std::fclose(f);
    return rc;
}
