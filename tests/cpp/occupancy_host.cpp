// Stand-alone driver of the occupancy grid's HOST text (csrc/rgrid_dev.h: occupancy_tables, occupancy_frame, occupancy_paint), built
// host-only by tests/test_occupancy_cpu.py and run without a GPU: the size / origin replay and the frame copy against the witness.
//
//   occupancy_host tables OUT          the two byte tables, 2 * 32768 bytes (occupancy, then red)
//   occupancy_host frames IN           per line of IN "x0 y0 w h resolution max_x max_y origin_x origin_y" (%d and %la) one line
//                                      "rc size_x size_y origin_x origin_y" (%d and %a) on stdout
//   occupancy_host paint MODE W H SX SY OUT
//                                      the image of a W x H block whose byte (u, c) is (31 u + 7 c + 1) & 255, rows stride apart
#include "../../reflector_ekf_slam_amd/csrc/rgrid_dev.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string what = argv[1];
    if (what == "tables") {
        std::vector<unsigned char> t(2 * 32768);
        occupancy_tables(reinterpret_cast<signed char *>(t.data()), t.data() + 32768);
        FILE *f = std::fopen(argv[2], "wb");
        if (!f) return 3;
        std::fwrite(t.data(), 1, t.size(), f);
        std::fclose(f);
        return 0;
    }
    if (what == "frames") {
        FILE *f = std::fopen(argv[2], "r");
        if (!f) return 3;
        int box[4];
        double r, mx, my, o[2];
        while (std::fscanf(f, "%d %d %d %d %la %la %la %la %la", &box[0], &box[1], &box[2], &box[3], &r, &mx, &my, &o[0], &o[1]) == 9) {
            OccupancyFrame F = {{0, 0}, {0., 0.}};
            const int rc = occupancy_frame(box, r, mx, my, o, &F);
            std::printf("%d %d %d %a %a\n", rc, F.size[0], F.size[1], F.origin[0], F.origin[1]);
        }
        std::fclose(f);
        return 0;
    }
    if (what == "paint" && argc == 8) {
        const int mode = std::atoi(argv[2]), w = std::atoi(argv[3]), h = std::atoi(argv[4]);
        const int size[2] = {std::atoi(argv[5]), std::atoi(argv[6])};
        const int stride = occupancy_stride(h);
        std::vector<unsigned char> block((size_t)stride * (size_t)w, 0xee), out((size_t)size[0] * (size_t)size[1]);   // exactly as long as needed
        for (int u = 0; u < w; ++u)
            for (int c = 0; c < h; ++c) block[(size_t)stride * u + c] = (unsigned char)((31 * u + 7 * c + 1) & 255);
        occupancy_paint(mode, block.data(), w, h, size, out.data());
        FILE *f = std::fopen(argv[7], "wb");
        if (!f) return 3;
        std::fwrite(out.data(), 1, out.size(), f);
        std::fclose(f);
        return 0;
    }
    return 2;
}
