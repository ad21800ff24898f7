// C++ user of RadarHIP::filterStep (include/radarays_ros_amd/RadarHIP.hpp) -- compiled by tests/test_filter_host.py.  The method works on
// buffers in HBM, which a caller allocates with the HIP runtime; this file has none and only shows that the call, the two records and
// the marshalling underneath are well-formed C++: with null buffers the library refuses the step and filterStep returns false.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>

using namespace radarays_ros_amd;

static_assert(sizeof(rr_filter_config) == 32 && sizeof(rr_filter_summary) == 32, "both records are 32 bytes");

int main()
{
    try {
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        rr_field_config grid = { 8, 8, 0.5f, 0.0f, 0.0f, 4, 1, 0 };
        rr_filter_config fc = { 1u, 16u, 0u, 1u, 0u, 0.0f, 0.0f, 0u };
        const float still[4] = { 1.0f, 0.0f, 0.0f, 0.0f };
        rr_filter_summary summary, before = {};
        const bool ok = radar.filterStep(nullptr, nullptr, 0, nullptr, 1, nullptr, grid, nullptr, fc, still, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         summary, 0.5, &before);
        std::printf("filterStep on null buffers: %s\n", ok ? "taken" : "refused");
        return ok ? 5 : 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 3; }
}
