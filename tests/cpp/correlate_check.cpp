// C++ driver of RadarHIP::correlateScan (include/radarays_ros_amd/RadarHIP.hpp) -- used by tests/test_gpu_correlate.py: reads a scan, the
// yaws, the window's centre, a field and the search's settings from a binary file written by the test, searches, and writes the record and
// the winner's metric pose.  Only the C ABI underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <fstream>

using namespace radarays_ros_amd;

static_assert(sizeof(rr_corr_config) == 32 && sizeof(rr_corr_rec) == 112, "the config: 32 bytes; the record: seven 16-byte words");

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    // points, yaws, the grid's width, height, max_dist, gate; half_x, half_y, levels, capacity
    int32_t h[10];
    float g[3];          // cell, x0, y0
    double c[2];         // the window's centre
    f.read((char*)h, sizeof(h));
    f.read((char*)g, sizeof(g));
    f.read((char*)c, sizeof(c));
    if (!f || h[0] < 0 || h[1] < 1 || h[2] < 1 || h[3] < 1) { std::fprintf(stderr, "short input\n"); return 2; }
    std::vector<double> yaws((size_t)h[1]);
    std::vector<rr_radar_point> scan((size_t)h[0]);
    std::vector<uint16_t> field((size_t)h[2] * h[3]);
    f.read((char*)yaws.data(), (std::streamsize)(yaws.size() * sizeof(double)));
    f.read((char*)scan.data(), (std::streamsize)(scan.size() * sizeof(rr_radar_point)));
    f.read((char*)field.data(), (std::streamsize)(field.size() * sizeof(uint16_t)));
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        const rr_field_config grid = { h[2], h[3], g[0], g[1], g[2], h[4], h[5], 0 };
        const rr_corr_config corr = { h[6], h[7], h[8], h[9], { 0, 0, 0, 0 } };
        rr_corr_rec rec;
        double pose[3] = { 0, 0, 0 };
        if (!radar.correlateScan(scan, yaws, c[0], c[1], field, grid, corr, rec, pose)) {
            std::fprintf(stderr, "correlateScan failed: %s\n", radar.lastError().c_str()); return 4;
        }
        // no yaw, a short field, a window beyond its range and a reserved word are refused
        rr_corr_rec none;
        rr_corr_config bad = corr;
        bad.half_x = 2048;
        rr_corr_config reserved = corr;
        reserved.reserved_[3] = 1;
        if (radar.correlateScan(scan, {}, c[0], c[1], field, grid, corr, none)) { std::fprintf(stderr, "no yaw was taken\n"); return 5; }
        if (radar.correlateScan(scan, yaws, c[0], c[1], std::vector<uint16_t>(3, 0), grid, corr, none)) { std::fprintf(stderr, "a short field was taken\n"); return 5; }
        if (radar.correlateScan(scan, yaws, c[0], c[1], field, grid, bad, none)) { std::fprintf(stderr, "half_x 2048 was taken\n"); return 5; }
        if (radar.correlateScan(scan, yaws, c[0], c[1], field, grid, reserved, none)) { std::fprintf(stderr, "a reserved word was taken\n"); return 5; }
        if (radar.lastError().find("reserved_") == std::string::npos) { std::fprintf(stderr, "the refusal does not say why: %s\n", radar.lastError().c_str()); return 5; }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)&rec, sizeof(rec));
        o.write((const char*)pose, sizeof(pose));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
