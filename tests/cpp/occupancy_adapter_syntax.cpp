// Syntax check of the occupancy calls of include/reflector_ekf_slam_amd/rgrid.hpp (rekfpp::GridFrontEnd::OccupancyGrid, SaveMap):
// compiled -fsyntax-only by tests/test_occupancy_cpu.py, never run.
#include "reflector_ekf_slam_amd/rgrid.hpp"

int occupancy_adapter_syntax(rekfpp::GridFrontEnd &fe)
{
    const std::array<double, 2> origin = {0.3, 0.5};
    const rekfpp::GridFrontEnd::Occupancy grid = fe.OccupancyGrid(origin);
    const rekfpp::GridFrontEnd::Occupancy image = fe.OccupancyGrid(origin, 1);
    fe.SaveMap(origin, "map");
    return grid.width * grid.height + image.box[2] + (int)grid.data.size() + (int)(grid.origin_x + grid.origin_y + grid.resolution);
}
