// Stand-alone driver of the fleet detectors' host text (csrc/det_batch_host.h), built host-only by tests/test_det_batch_host_cpu.py's
// fixture and run without a GPU, against that test's own text of the rules.
//
//   det_batch_host IN      IN holds records, each answered on stdout.  Doubles travel as %la, floats as the 8 hex digits of their bits
//   (a NaN's payload and the sign of a zero arrive as written), records as the hex digits of their bytes.  A scan line is
//   "member stamp angle_min angle_max angle_increment scan_time range_min range_max N ranges_null intensities_null".
//     "members B count has_list m..."   -> "members ok first_bad scratch_zero next_ok": members_named_once, check_members over the same
//                                          list, whether the scratch is all zero behind them, and the whole fleet named once on that scratch
//     "validate2 B max_beams count" + count scan lines     -> "rc code scratch_zero next_rc" (next: one empty scan of every member)
//     "validate3 B max_points count" + count lines "member N null"     -> the same
//     "tables calls", per call "count" + count scan lines  -> per call "call n_submit", count lines "table fill cached" and
//                                                             RDET2DB_TABLES lines "N angle_min inc used": ONE cache through all calls
//     "angles angle_min angle_increment N stride"          -> "angles <3 N floats>": fill_angle_table's angle | cos | sin
//     "submit2 B count", B members "intensity_min min_length length_error range_min range_max s2b[3] last_n_returns n_odom" each with
//       n_odom lines of 7 doubles, count scan lines        -> steps 1-3 on a fresh cache: "rc code", and when 0 "n_run n", count lines
//                                                             "member stamp status runs table fill cached <BatchRec>", B lines
//                                                             "last_n_returns n_odom time..."
//     "submit3 B max_points count", B lines "intensity_min s2b[3]", count lines "member stamp N null"
//                                                          -> "rc code", and when 0 "n_run cap", count lines "member stamp runs",
//                                                             n_run lines "<Cloud3Rec>"
//     "range B max_beams count has_list m...", then B last_n_returns
//                                                          -> "ok 0|1", and when 1 "total tiles table_off", "counts ...",
//                                                             "recs n <RangeRec>...", "wgs n record:tile ..."
//     "collect count max_centers", count lines "host_status runs K err" -> count lines "status K seen_record <2 K floats>" and
//                                                             "untouched 0|1": nothing else of the centres was written
//     "collect_args count status K centers max_centers" (pointers as 0|1)   -> "args 0|1"
//     "link device count", count lines "member stamp host_status runs"  -> the rlink's fields, one line
#include "../../reflector_ekf_slam_amd/csrc/det_batch_host.h"

#include <cstdio>
#include <string>

using namespace det_batch_host;

static bool rd_float(FILE *f, float *v)
{
    unsigned u;
    if (std::fscanf(f, "%x", &u) != 1) return false;
    std::memcpy(v, &u, 4);
    return true;
}
static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
static void hex(const void *p, size_t n)
{
    for (size_t i = 0; i < n; ++i) std::printf("%02x", (unsigned)((const unsigned char *)p)[i]);
}
static bool all_zero(const std::vector<char> &v)
{
    for (char c : v) if (c) return false;
    return true;
}

static float some_floats[8];     // what a scan's pointers that are not NULL point at (the host text never reads through them)

static bool rd_scan(FILE *f, rdet2d_scan *s)
{
    int rn, in;
    if (std::fscanf(f, "%d %la", &s->member, &s->stamp) != 2) return false;
    if (!rd_float(f, &s->angle_min) || !rd_float(f, &s->angle_max) || !rd_float(f, &s->angle_increment) || !rd_float(f, &s->scan_time) ||
        !rd_float(f, &s->range_min) || !rd_float(f, &s->range_max))
        return false;
    if (std::fscanf(f, "%d %d %d", &s->N, &rn, &in) != 3) return false;
    s->ranges = rn ? nullptr : some_floats;
    s->intensities = in ? nullptr : some_floats;
    return true;
}

static int run_members(FILE *f)
{
    int B, count, has_list;
    if (std::fscanf(f, "%d %d %d", &B, &count, &has_list) != 3) return 4;
    std::vector<int> list((size_t)(has_list && count > 0 ? count : 0)), all((size_t)B);
    for (int &m : list)
        if (std::fscanf(f, "%d", &m) != 1) return 4;
    for (int g = 0; g < B; ++g) all[(size_t)g] = B - 1 - g;
    int none = 0;                                             // (an empty list is still a list: a pointer that is not NULL)
    const int *members = !has_list ? nullptr : list.empty() ? &none : list.data();
    std::vector<char> seen((size_t)B, 0);
    const int ok = members_named_once(members, count, B, seen);
    const int bad = has_list ? check_members(count, B, seen, [&](int g) { return list[(size_t)g]; }) : -1;
    const int zero = all_zero(seen);
    std::printf("members %d %d %d %d\n", ok, bad, zero, (int)members_named_once(all.data(), B, B, seen));
    return 0;
}

static int run_validate2(FILE *f)
{
    int B, max_beams, count;
    if (std::fscanf(f, "%d %d %d", &B, &max_beams, &count) != 3) return 4;
    std::vector<rdet2d_scan> scans((size_t)count), next((size_t)B);
    for (rdet2d_scan &s : scans)
        if (!rd_scan(f, &s)) return 4;
    for (int g = 0; g < B; ++g) { next[(size_t)g] = rdet2d_scan{}; next[(size_t)g].member = g; }
    std::vector<char> seen((size_t)B, 0);
    const int rc = validate_scans(scans.data(), count, B, max_beams, seen);
    const int zero = all_zero(seen);
    std::printf("rc %d %d %d\n", rc, zero, validate_scans(next.data(), B, B, max_beams, seen));
    return 0;
}

static int run_validate3(FILE *f)
{
    int B, max_points, count;
    if (std::fscanf(f, "%d %d %d", &B, &max_points, &count) != 3) return 4;
    std::vector<rdet3d_cloud> clouds((size_t)count), next((size_t)B);
    for (rdet3d_cloud &c : clouds) {
        int null;
        c = rdet3d_cloud{};
        if (std::fscanf(f, "%d %d %d", &c.member, &c.N, &null) != 3) return 4;
        c.xyzi = null ? nullptr : some_floats;
    }
    for (int g = 0; g < B; ++g) { next[(size_t)g] = rdet3d_cloud{}; next[(size_t)g].member = g; }
    std::vector<char> seen((size_t)B, 0);
    const int rc = validate_clouds(clouds.data(), count, B, max_points, seen);
    const int zero = all_zero(seen);
    std::printf("rc %d %d %d\n", rc, zero, validate_clouds(next.data(), B, B, max_points, seen));
    return 0;
}

static int run_tables(FILE *f)
{
    int calls;
    if (std::fscanf(f, "%d", &calls) != 1) return 4;
    TableCache cache;
    std::vector<TableUse> use;
    for (int c = 0; c < calls; ++c) {
        int count;
        if (std::fscanf(f, "%d", &count) != 1) return 4;
        std::vector<rdet2d_scan> scans((size_t)count);
        for (rdet2d_scan &s : scans)
            if (!rd_scan(f, &s)) return 4;
        plan_tables(cache, scans.data(), count, use);
        std::printf("call %llu\n", cache.n_submit);
        for (const TableUse &u : use) std::printf("%d %d %d\n", u.table, (int)u.fill, (int)u.cached);
        for (const Table &t : cache.tab) std::printf("%d %08x %08x %llu\n", t.N, bits(t.angle_min), bits(t.inc), t.used);
    }
    return 0;
}

static int run_submit2(FILE *f)
{
    int B, count;
    if (std::fscanf(f, "%d %d", &B, &count) != 2) return 4;
    std::vector<Member2d> m((size_t)B);
    for (Member2d &M : m) {
        int n_odom;
        if (std::fscanf(f, "%la %la %la", &M.opt.intensity_min, &M.opt.reflector_min_length, &M.opt.reflector_length_error) != 3) return 4;
        if (!rd_float(f, &M.opt.range_min) || !rd_float(f, &M.opt.range_max)) return 4;
        if (std::fscanf(f, "%la %la %la %d %d", &M.s2b[0], &M.s2b[1], &M.s2b[2], &M.last_n_returns, &n_odom) != 5) return 4;
        M.odom.resize((size_t)n_odom);
        for (Odom &o : M.odom)
            if (std::fscanf(f, "%la %la %la %la %la %la %la", &o.time, &o.px, &o.py, &o.yaw, &o.vx, &o.vy, &o.wz) != 7) return 4;
    }
    std::vector<rdet2d_scan> scans((size_t)count);
    for (rdet2d_scan &s : scans)
        if (!rd_scan(f, &s)) return 4;
    SubmitState st;
    st.size(B);
    const int rc = validate_scans(scans.data(), count, B, RDET2DB_MAX_BEAMS, st.seen);
    std::printf("rc %d\n", rc);
    if (rc != RDET_OK) return 0;
    TableCache cache;
    std::vector<TableUse> use;
    plan_tables(cache, scans.data(), count, use);
    BatchRec *recs = new BatchRec[(size_t)count];             // exactly `count` records: a write past the end is a sanitizer's finding
    std::memset(recs, 0xA5, sizeof(BatchRec) * (size_t)count);
    const int n_run = pack_scans(scans.data(), count, m, use, st, recs);
    std::printf("n_run %d\n", n_run);
    if (st.sub_count != count) return 5;
    for (int i = 0; i < count; ++i) {
        std::printf("%d %a %d %d %d %d %d ", st.sub_member[(size_t)i], st.sub_stamp[(size_t)i], st.sub_status[(size_t)i], st.sub_runs[(size_t)i],
                    use[(size_t)i].table, (int)use[(size_t)i].fill, (int)use[(size_t)i].cached);
        hex(&recs[i], sizeof(BatchRec));
        std::printf("\n");
    }
    delete[] recs;
    for (const Member2d &M : m) {
        std::printf("%d %zu", M.last_n_returns, M.odom.size());
        for (const Odom &o : M.odom) std::printf(" %a", o.time);
        std::printf("\n");
    }
    return 0;
}

static int run_submit3(FILE *f)
{
    int B, max_points, count;
    if (std::fscanf(f, "%d %d %d", &B, &max_points, &count) != 3) return 4;
    std::vector<Member3d> m((size_t)B);
    for (Member3d &M : m)
        if (std::fscanf(f, "%la %la %la %la", &M.opt.intensity_min, &M.s2b[0], &M.s2b[1], &M.s2b[2]) != 4) return 4;
    std::vector<rdet3d_cloud> clouds((size_t)count);
    for (rdet3d_cloud &c : clouds) {
        int null;
        c = rdet3d_cloud{};
        if (std::fscanf(f, "%d %la %d %d", &c.member, &c.stamp, &c.N, &null) != 4) return 4;
        c.xyzi = null ? nullptr : some_floats;
    }
    SubmitState st;
    st.size(B);
    const int rc = validate_clouds(clouds.data(), count, B, max_points, st.seen);
    std::printf("rc %d\n", rc);
    if (rc != RDET_OK) return 0;
    int running = 0;
    for (const rdet3d_cloud &c : clouds) running += c.N > 0;
    Cloud3Rec *recs = new Cloud3Rec[(size_t)running];         // exactly the clouds that run
    std::memset(recs, 0xA5, sizeof(Cloud3Rec) * (size_t)running);
    int cap = -1;
    const int n_run = pack_clouds(clouds.data(), count, m, st, recs, &cap);
    std::printf("%d %d\n", n_run, cap);
    if (st.sub_count != count || n_run != running) return 5;
    for (int i = 0; i < count; ++i) std::printf("%d %a %d\n", st.sub_member[(size_t)i], st.sub_stamp[(size_t)i], st.sub_runs[(size_t)i]);
    for (int r = 0; r < n_run; ++r) { hex(&recs[r], sizeof(Cloud3Rec)); std::printf("\n"); }
    delete[] recs;
    return 0;
}

static int run_range(FILE *f)
{
    int B, max_beams, count, has_list;
    if (std::fscanf(f, "%d %d %d %d", &B, &max_beams, &count, &has_list) != 4) return 4;
    std::vector<int> list((size_t)(has_list && count > 0 ? count : 0));
    for (int &m : list)
        if (std::fscanf(f, "%d", &m) != 1) return 4;
    std::vector<Member2d> m((size_t)B);
    for (Member2d &M : m)
        if (std::fscanf(f, "%d", &M.last_n_returns) != 1) return 4;
    int none = 0;
    const int *members = !has_list ? nullptr : list.empty() ? &none : list.data();
    std::vector<char> seen((size_t)B, 0);
    const int ok = members_named_once(members, count, B, seen);
    std::printf("ok %d\n", ok);
    if (!ok) return 0;
    std::vector<int> counts((size_t)count);
    const long total = range_counts(members, count, max_beams, m, counts.data());
    const size_t tiles = range_tiles(max_beams), off = range_table_off(B);
    std::printf("%ld %zu %zu\ncounts", total, tiles, off);
    for (int c : counts) std::printf(" %d", c);
    const size_t bytes = off + sizeof(RangeTile) * tiles * (size_t)B;      // what the handle allocates
    unsigned char *tab = new unsigned char[bytes];
    std::memset(tab, 0xA5, bytes);
    const int nwg = range_data_plan(members, counts.data(), count, max_beams, reinterpret_cast<RangeRec *>(tab),
                                    reinterpret_cast<RangeTile *>(tab + off));
    int nrec = 0;
    for (int c : counts) nrec += c > 0;
    std::printf("\nrecs %d", nrec);
    for (int r = 0; r < nrec; ++r) { std::printf(" "); hex(tab + sizeof(RangeRec) * (size_t)r, sizeof(RangeRec)); }
    std::printf("\nwgs %d", nwg);
    for (int w = 0; w < nwg; ++w) {
        const RangeTile &t = reinterpret_cast<const RangeTile *>(tab + off)[w];
        std::printf(" %d:%d", t.record, t.tile);
    }
    std::printf("\n");
    delete[] tab;
    return 0;
}

struct Out {                      // a record as the kernels write them: K, err and the centres, something else between
    int K, other, err, pad;
    float centers[RDET_MAX_CENTERS][2];
};

static int run_collect(FILE *f)
{
    int count, max_centers;
    if (std::fscanf(f, "%d %d", &count, &max_centers) != 2) return 4;
    SubmitState st;
    st.size(count > 0 ? count : 1);
    st.sub_count = count;
    std::vector<Out> out((size_t)count);
    for (int i = 0; i < count; ++i) {
        if (std::fscanf(f, "%d %d %d %d", &st.sub_status[(size_t)i], &st.sub_runs[(size_t)i], &out[(size_t)i].K, &out[(size_t)i].err) != 4) return 4;
        st.sub_stamp[(size_t)i] = 100.0 + i;
        for (int k = 0; k < RDET_MAX_CENTERS; ++k) { out[(size_t)i].centers[k][0] = (float)(1000 * i + k); out[(size_t)i].centers[k][1] = -(float)(1000 * i + k); }
    }
    const int cap = max_centers > RDET_MAX_CENTERS ? RDET_MAX_CENTERS : max_centers;
    const size_t n = (size_t)2 * (size_t)cap * (size_t)count;
    float *centers = new float[n];                            // exactly what rdet.h asks of the caller
    for (size_t k = 0; k < n; ++k) centers[k] = -7.f;
    std::vector<int> status((size_t)count, 99), K((size_t)count, 99), had((size_t)count, -1);
    std::vector<double> obs((size_t)count, 0.0);
    collect(st, out.data(), status.data(), K.data(), centers, max_centers, obs.data(), [&](int i, const Out *o) { had[(size_t)i] = o == &out[(size_t)i] ? 1 : o ? 2 : 0; });
    bool untouched = true;
    for (int i = 0; i < count; ++i) {
        if (obs[(size_t)i] != 100.0 + i) return 5;
        std::printf("%d %d %d", status[(size_t)i], K[(size_t)i], had[(size_t)i]);
        for (int k = 0; k < 2 * cap; ++k) {
            const float v = centers[(size_t)2 * (size_t)cap * (size_t)i + (size_t)k];
            if (k < 2 * K[(size_t)i]) std::printf(" %a", v);
            else untouched = untouched && v == -7.f;
        }
        std::printf("\n");
    }
    delete[] centers;
    std::printf("untouched %d\n", (int)untouched);
    return 0;
}

static int run_link(FILE *f)
{
    int device, count;
    if (std::fscanf(f, "%d %d", &device, &count) != 2) return 4;
    SubmitState st;
    st.size(count + 2);
    st.sub_count = count;
    for (int i = 0; i < count; ++i)
        if (std::fscanf(f, "%d %la %d %d", &st.sub_member[(size_t)i], &st.sub_stamp[(size_t)i], &st.sub_status[(size_t)i], &st.sub_runs[(size_t)i]) != 4) return 4;
    for (int &r : st.sub_record) r = 77;
    static char records, ready, consumed;
    rlink l;
    std::memset(&l, 0xA5, sizeof(l));
    fill_link(st, device, &records, 2064, 0, 8, 16, &ready, &consumed, &l);
    std::printf("link %d %d %d %d %d %d %ld %d %d %d %d %d %d records", l.count, l.device, (int)(l.member == st.sub_member.data()), (int)(l.stamp == st.sub_stamp.data()),
                (int)(l.host_status == st.sub_status.data()), (int)(l.record == st.sub_record.data()), l.record_bytes, l.k_off, l.err_off, l.centers_off,
                l.max_centers, (int)(l.records == &records && l.ready == &ready), (int)(l.consumed == &consumed));
    for (int r : st.sub_record) std::printf(" %d", r);
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
        const std::string w(what);
        if (w == "members") rc = run_members(f);
        else if (w == "validate2") rc = run_validate2(f);
        else if (w == "validate3") rc = run_validate3(f);
        else if (w == "tables") rc = run_tables(f);
        else if (w == "submit2") rc = run_submit2(f);
        else if (w == "submit3") rc = run_submit3(f);
        else if (w == "range") rc = run_range(f);
        else if (w == "collect") rc = run_collect(f);
        else if (w == "collect_args") {
            int count, s, k, c, mc;
            static int one;
            static float onef;
            if (std::fscanf(f, "%d %d %d %d %d", &count, &s, &k, &c, &mc) != 5) rc = 4;
            else std::printf("args %d\n", (int)collect_args_ok(count, s ? &one : nullptr, k ? &one : nullptr, c ? &onef : nullptr, mc));
        } else if (w == "angles") {
            float a0, inc;
            int N, stride;
            if (!rd_float(f, &a0) || !rd_float(f, &inc) || std::fscanf(f, "%d %d", &N, &stride) != 2) { rc = 4; continue; }
            float *t = new float[(size_t)2 * (size_t)stride + (size_t)N];      // three parts `stride` apart, the last one N long
            fill_angle_table(t, (size_t)stride, a0, inc, N);
            std::printf("angles");
            for (int part = 0; part < 3; ++part)
                for (int k = 0; k < N; ++k) std::printf(" %08x", bits(t[(size_t)part * (size_t)stride + (size_t)k]));
            std::printf("\n");
            delete[] t;
        } else if (w == "link") rc = run_link(f);
        else rc = 2;
    }
    std::fclose(f);
    return rc;
}
