// C++ user of RadarHIP::castMap and RadarHIP::scoreBeams (include/radarays_ros_amd/RadarHIP.hpp) -- compiled by tests/test_cast_host.py.
// Both work on buffers in HBM, which a caller allocates with the HIP runtime; this file has none and only shows that the calls, the record
// and the marshalling underneath are well-formed C++: with null buffers the library refuses the call and both return false.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>

using namespace radarays_ros_amd;

static_assert(sizeof(rr_beam_rec) == 32 && sizeof(rr_beam_config) == 32 && sizeof(rr_field_config) == 32, "the record, the beams and the grid: 32 bytes");

int main()
{
    try {
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        rr_field_config grid = { 8, 8, 0.5f, 0.0f, 0.0f, 4, 0, 0 };
        rr_beam_config beam = { 0, 64, 1, 6, 24, { 0, 0, 0 } };
        const bool cast = radar.castMap(nullptr, 1, nullptr, nullptr, grid, beam, nullptr);
        const bool scored = radar.scoreBeams(nullptr, nullptr, 1, nullptr, nullptr, grid, beam, nullptr);
        std::printf("castMap on null buffers: %s; scoreBeams on null buffers: %s\n", cast ? "taken" : "refused", scored ? "taken" : "refused");
        return cast || scored ? 5 : 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
}
