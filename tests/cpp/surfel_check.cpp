// C++ driver of RadarHIP::surfacePoints and RadarHIP::registerSurfacePoints (include/radarays_ros_amd/RadarHIP.hpp) -- used by
// tests/test_gpu_surfels_cpp.py: reads clouds, a surfel config, initial states and the matcher's settings from a binary file written by the
// test, reduces every cloud to surface points, registers clouds 1.. against the surface points of cloud 0, and writes the counts, every
// cloud's records and the registration records.  Only the C ABI underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <fstream>

using namespace radarays_ros_amd;

static_assert(sizeof(rr_surfel_config) == 32 && sizeof(rr_surfel) == 32 && sizeof(rr_icp_rec) == 48, "the config and a surface point: 32 bytes; a record: 48");

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    // clouds, width, min_points, max_surfels, iterations, whether initial states follow; cell, max_ratio, gate; then every cloud's length
    int32_t h[6];
    float g[3];
    f.read((char*)h, sizeof(h));
    f.read((char*)g, sizeof(g));
    if (!f || h[0] < 2 || h[0] > 64) { std::fprintf(stderr, "short input\n"); return 2; }
    const size_t n = (size_t)h[0];
    std::vector<int32_t> lens(n);
    f.read((char*)lens.data(), (std::streamsize)(n * sizeof(int32_t)));
    std::vector<double> init(h[5] ? 4 * (n - 1) : 0);
    f.read((char*)init.data(), (std::streamsize)(init.size() * sizeof(double)));
    std::vector<std::vector<rr_radar_point>> clouds(n);
    for (size_t k = 0; k < n && f; k++) {
        if (lens[k] < 0 || lens[k] > 65536) { std::fprintf(stderr, "bad length\n"); return 2; }
        clouds[k].resize((size_t)lens[k]);
        f.read((char*)clouds[k].data(), (std::streamsize)(clouds[k].size() * sizeof(rr_radar_point)));
    }
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        // a context needs a map; this one is a single far-away triangle (only the cloud calls are used)
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        radar.loadParams({ RadarMaterial{}, RadarMaterial{ 0.0f, 1.0f, 1.0f, 1.0f } }, { 1 }, 0);
        RadarModelConfig cfg;
        cfg.n_cells = 64; cfg.n_samples = 4; cfg.include_motion = false;
        radar.updateDynCfg(cfg);
        radar.setBeamSamples({ 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0 });
        const rr_surfel_config sc = { g[0], h[1], h[2], g[1], { 0, 0, 0, 0 } };
        std::vector<std::vector<rr_surfel>> surfels;
        std::vector<uint32_t> counts;
        if (!radar.surfacePoints(clouds, sc, surfels, counts, h[3]) || surfels.size() != n || counts.size() != 2 * n) {
            std::fprintf(stderr, "surfacePoints failed: %s\n", radar.lastError().c_str()); return 4;
        }
        const std::vector<std::vector<rr_radar_point>> sources(clouds.begin() + 1, clouds.end());
        const std::vector<rr_icp_rec> recs = radar.registerSurfacePoints(sources, surfels[0], g[2], h[4], init);
        if (recs.size() != n - 1) { std::fprintf(stderr, "registerSurfacePoints failed: %s\n", radar.lastError().c_str()); return 4; }
        // no cloud, a reserved word, a cell beyond its range, an init of the wrong shape and a gate of 0 are refused
        std::vector<std::vector<rr_surfel>> none;
        std::vector<uint32_t> no_counts;
        rr_surfel_config reserved = sc, wide = sc;
        reserved.reserved_[2] = 1;
        wide.cell = 17.0f;
        if (radar.surfacePoints({}, sc, none, no_counts)) { std::fprintf(stderr, "no cloud was taken\n"); return 5; }
        if (radar.surfacePoints(clouds, wide, none, no_counts)) { std::fprintf(stderr, "a cell of 17 m was taken\n"); return 5; }
        if (radar.surfacePoints(clouds, reserved, none, no_counts) || !none.empty() || !no_counts.empty()) { std::fprintf(stderr, "a reserved word was taken\n"); return 5; }
        if (radar.lastError().find("reserved_") == std::string::npos) { std::fprintf(stderr, "the refusal does not say why: %s\n", radar.lastError().c_str()); return 5; }
        if (!radar.registerSurfacePoints({}, surfels[0]).empty()) { std::fprintf(stderr, "no source was taken\n"); return 5; }
        if (!radar.registerSurfacePoints(sources, surfels[0], g[2], h[4], std::vector<double>(3, 1.0)).empty()) { std::fprintf(stderr, "a short init was taken\n"); return 5; }
        if (!radar.registerSurfacePoints(sources, surfels[0], 0.0f, h[4]).empty()) { std::fprintf(stderr, "a gate of 0 was taken\n"); return 5; }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)counts.data(), (std::streamsize)(counts.size() * sizeof(uint32_t)));
        for (const auto& s : surfels) o.write((const char*)s.data(), (std::streamsize)(s.size() * sizeof(rr_surfel)));
        o.write((const char*)recs.data(), (std::streamsize)(recs.size() * sizeof(rr_icp_rec)));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
