// C++ user of RadarHIP::buildNearestField and RadarHIP::refinePoses (include/radarays_ros_amd/RadarHIP.hpp) -- compiled by
// tests/test_refine_host.py.  refinePoses works on buffers in HBM, which a caller allocates with the HIP runtime; this file has none and only
// shows that the calls, the record and the marshalling underneath are well-formed C++: with null buffers the library refuses the call and
// refinePoses returns false; a map of the wrong size is refused before the library is asked.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>

using namespace radarays_ros_amd;

static_assert(sizeof(rr_icp_rec) == 48 && sizeof(rr_field_config) == 32, "the record is 48 bytes, the grid 32");

int main()
{
    try {
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        rr_field_config grid = { 8, 8, 0.5f, 0.0f, 0.0f, 4, 1, 0 };
        const std::vector<uint32_t> none = radar.buildNearestField(std::vector<uint8_t>(7, 0), grid);
        const std::vector<uint32_t> table = radar.buildNearestField(std::vector<uint8_t>(64, 1), grid, 1);
        const bool ok = radar.refinePoses(nullptr, nullptr, 0, nullptr, 1, nullptr, grid, nullptr, 10);
        std::printf("buildNearestField: %zu and %zu entries; refinePoses on null buffers: %s\n", none.size(), table.size(), ok ? "taken" : "refused");
        return ok || !none.empty() ? 5 : 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
}
