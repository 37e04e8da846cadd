// Stand-alone driver of the steps of rfleet_submit that need no HIP call (csrc/fleet_host.h: submit_validate, submit_plan,
// submit_layout, submit_pack) and of members_named_once, built host-only by tests/test_fleet_submit_host_cpu.py's fixture and run
// without a GPU, against that test's own text of the segment's layout.
//
//   fleet_submit_host IN      IN holds records, each answered on stdout:
//     "members B count has_list m0 m1 ..."      -> "members <0|1>"
//     "submit B wide tracked M_map count", then B lines "use_imu time vx vy wz map_use", then per event one line
//     "member kind t vx vy wz K has_fix fx fy fyaw xy_null" followed by 2 K floats (doubles in %la, floats in %a)
//       -> "rc <code>", "mirror <time[B]> <vt[3B]>" (the handle's mirror behind the call: never touched), and when rc is 0
//          "plan E G n_obs n_fix n_wide with_map rec", "cnt <B>", "scanned ...", "next <time[B]> <vt[3B]>" (the mirror the commit
//          would put in place), "layout off_mem off_beg off_ev off_fix off_obs off_track need", "seg <2 need hex digits>" (a heap
//          buffer of exactly `need` bytes, pre-filled with 0xA5) and "meta n" + n lines "t member kind K dropped"
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

static int run_members(FILE *f)
{
    int B, count, has_list;
    if (std::fscanf(f, "%d %d %d", &B, &count, &has_list) != 3) return 4;
    std::vector<int> list((size_t)(has_list && count > 0 ? count : 0)), cnt((size_t)B);
    for (int &m : list)
        if (std::fscanf(f, "%d", &m) != 1) return 4;
    int none = 0;                                             // (an empty list is still a list: a pointer that is not NULL)
    const int *members = !has_list ? nullptr : list.empty() ? &none : list.data();
    std::printf("members %d\n", (int)members_named_once(members, count, B, cnt));
    return 0;
}

static int run_submit(FILE *f)
{
    int B, wide, tracked, M_map, count;
    if (std::fscanf(f, "%d %d %d %d %d", &B, &wide, &tracked, &M_map, &count) != 5) return 4;
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
    std::vector<rfleet_event> ev((size_t)count);
    std::vector<std::vector<float>> clouds((size_t)count);
    for (int i = 0; i < count; ++i) {
        rfleet_event &e = ev[i];
        int xy_null;
        if (std::fscanf(f, "%d %d %la %la %la %la %d %d %la %la %la %d", &e.member, &e.kind, &e.t, &e.v[0], &e.v[1], &e.v[2], &e.K, &e.has_pose_fix,
                        &e.pose_fix[0], &e.pose_fix[1], &e.pose_fix[2], &xy_null) != 12)
            return 4;
        clouds[i].resize((size_t)(e.K > 0 && !xy_null ? 2 * e.K : 0));
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
    const int rc = submit_validate(ev.data(), count, B, wide != 0);
    std::printf("rc %d\n", rc);
    SubmitPlan p;
    if (rc == REKF_OK) p = submit_plan(ev.data(), count, opts, time, vt, tracked != 0, M_map, map_use, s);
    print_mirror("mirror", time, vt);
    if (rc != REKF_OK) return 0;
    std::printf("plan %d %d %zu %zu %zu %d %d\ncnt", p.E, p.G, p.n_obs, p.n_fix, p.n_wide, (int)p.with_map, (int)p.rec);
    for (int c : s.cnt) std::printf(" %d", c);
    std::printf("\nscanned");
    for (int b : s.scanned) std::printf(" %d", b);
    std::printf("\n");
    print_mirror("next", s.time, s.vt);
    submit_layout(p);
    std::printf("layout %zu %zu %zu %zu %zu %zu %zu\nseg ", p.off_mem, p.off_beg, p.off_ev, p.off_fix, p.off_obs, p.off_track, p.need);
    std::vector<TrackMeta> meta;
    char *seg = new char[p.need];                             // exactly `need` bytes: a write past the end is a sanitizer's finding
    memset(seg, 0xA5, p.need);
    if (p.E > 0) submit_pack(ev.data(), p, s, seg, meta);     // (E == 0: rfleet_submit returns before it lays anything out)
    for (size_t i = 0; i < p.need; ++i) std::printf("%02x", (unsigned)(unsigned char)seg[i]);
    delete[] seg;
    std::printf("\nmeta %zu\n", meta.size());
    for (const TrackMeta &m : meta) std::printf("%a %d %d %d %d\n", m.t, m.member, m.kind, m.K, m.dropped);
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
        if (std::string(what) == "members") rc = run_members(f);
        else if (std::string(what) == "submit") rc = run_submit(f);
        else rc = 2;
    }
    std::fclose(f);
    return rc;
}
