// Stand-alone driver of the HOST text both grid handles call around their kernels (csrc/rgrid_dev.h: gravity_alignment,
// compose_pose_estimate, origin_in_local, initial_submap_limits, refine_threads and the option checks), built host-only by
// tests/test_range_data_host_cpu.py's fixture and run without a GPU, against reflector_ekf_slam_amd/map_builder.py's own arithmetic.
//
//   range_data_host poses IN     per line of IN "theta est_x est_y est_a origin_x origin_y resolution max_cells" (%la, max_cells %lld)
//                                one line "qw qz yaw_g  local_x local_y local_a  yaw_f32 yaw2  org_x org_y  rc nx ny resolution max_x
//                                max_y" (%a and %d) on stdout; the limits are zero where rc is not 0
//   range_data_host checks       "threads" and refine_threads(n) of the n the test lists; then per option check one line of three
//                                answers: a passing option, a zero one, a NaN one
#include "../../reflector_ekf_slam_amd/csrc/rgrid_dev.h"

#include <cstdio>
#include <limits>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "poses" && argc == 3) {
        FILE *f = std::fopen(argv[2], "r");
        if (!f) return 3;
        double theta, est[3], origin[2], resolution;
        long long max_cells;
        while (std::fscanf(f, "%la %la %la %la %la %la %la %lld", &theta, &est[0], &est[1], &est[2], &origin[0], &origin[1], &resolution, &max_cells) == 8) {
            double qw, qz, local_pose[3];
            float yaw_g, yaw_f32, yaw2, org[2];
            const float origin_xy[2] = {(float)origin[0], (float)origin[1]};
            gravity_alignment(theta, qw, qz, yaw_g);
            compose_pose_estimate(est, qw, qz, local_pose, yaw_f32, yaw2);
            origin_in_local(origin_xy, yaw_g, est, yaw2, org);
            int nx = 0, ny = 0;
            double r = 0., max_x = 0., max_y = 0.;
            const int rc = initial_submap_limits((float)resolution, org, max_cells, nx, ny, r, max_x, max_y);
            std::printf("%a %a %a  %a %a %a  %a %a  %a %a  %d %d %d %a %a %a\n", qw, qz, (double)yaw_g, local_pose[0], local_pose[1], local_pose[2],
                        (double)yaw_f32, (double)yaw2, (double)org[0], (double)org[1], rc, nx, ny, r, max_x, max_y);
        }
        std::fclose(f);
        return 0;
    }
    if (what == "checks") {
        std::printf("threads");
        for (int n : {1, 63, 64, 65, 1023, 1024, 1025, 16384}) std::printf(" %d", refine_threads(n));
        std::printf("\n");
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const float nanf = std::numeric_limits<float>::quiet_NaN();
        const rgrid_refine_options r_ok = {1., 0.1, 0.4, 100, 1}, r_zero = {1., 0., 0.4, 100, 1}, r_nan = {1., 0.1, nan, 100, 1};
        std::printf("refine %d %d %d\n", (int)refine_options_ok(&r_ok), (int)refine_options_ok(&r_zero), (int)refine_options_ok(&r_nan));
        std::printf("insert %d %d %d\n", (int)insert_options_ok(0.55f, 0.49f), (int)insert_options_ok(0.55f, 0.f), (int)insert_options_ok(nanf, 0.49f));
        const rgrid_filter_options f_ok = {0.025f, 0.9, 500., 100.}, f_zero = {0.f, 0.9, 500., 100.}, f_nan = {0.025f, nan, 500., 100.};
        std::printf("filter %d %d %d\n", (int)filter_options_ok(&f_ok), (int)filter_options_ok(&f_zero), (int)filter_options_ok(&f_nan));
        return 0;
    }
    return 2;
}
