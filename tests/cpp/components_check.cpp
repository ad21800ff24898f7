// C++ driver of RadarHIP::clusterImages and RadarHIP::segmentMap (include/radarays_ros_amd/RadarHIP.hpp) -- used by
// tests/test_gpu_components.py: reads polar images, a grid map and the two calls' settings from a binary file written by the test, clusters
// the images on the cylinder, segments the map, and writes the label planes, the counts, every image's records, the cleaned map and the
// segments' records.  Only the C ABI underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <fstream>

using namespace radarays_ros_amd;

static_assert(sizeof(rr_components_config) == 32 && sizeof(rr_component) == 80, "the config: 32 bytes; a record: five 16-byte words");

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    // images, n_cells, threshold, connectivity, min_pixels, max_components; the map's width, height, threshold, min_cells, connectivity
    int32_t h[11];
    f.read((char*)h, sizeof(h));
    if (!f || h[0] < 1 || h[1] < 1 || h[6] < 1 || h[7] < 1) { std::fprintf(stderr, "short input\n"); return 2; }
    const int n_angles = 400;
    std::vector<uint8_t> images((size_t)h[0] * h[1] * n_angles), occ((size_t)h[6] * h[7]);
    f.read((char*)images.data(), (std::streamsize)images.size());
    f.read((char*)occ.data(), (std::streamsize)occ.size());
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        RadarModelConfig cfg;
        cfg.n_cells = h[1];
        radar.updateDynCfg(cfg);
        std::vector<std::vector<rr_component>> clusters;
        std::vector<uint32_t> counts, labels;
        if (!radar.clusterImages(images, h[0], h[2], clusters, counts, &labels, h[3], h[4], h[5])) {
            std::fprintf(stderr, "clusterImages failed: %s\n", radar.lastError().c_str()); return 4;
        }
        const rr_field_config grid = { h[6], h[7], 0.25f, 0.0f, 0.0f, 8, 0, 0 };
        std::vector<rr_component> segments;
        const std::vector<uint8_t> clean = radar.segmentMap(occ, grid, h[8], segments, h[9], h[10]);
        if (clean.empty()) { std::fprintf(stderr, "segmentMap failed: %s\n", radar.lastError().c_str()); return 4; }
        // a threshold of 0, a short image buffer and a short map are refused
        std::vector<std::vector<rr_component>> none;
        std::vector<uint32_t> no_counts;
        if (radar.clusterImages(images, h[0], 0, none, no_counts)) { std::fprintf(stderr, "a threshold of 0 was taken\n"); return 5; }
        if (radar.clusterImages(std::vector<uint8_t>(7, 0), 1, 128, none, no_counts)) { std::fprintf(stderr, "a short image was taken\n"); return 5; }
        if (!radar.segmentMap(std::vector<uint8_t>(3, 0), grid, 1, segments).empty()) { std::fprintf(stderr, "a short map was taken\n"); return 5; }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)labels.data(), (std::streamsize)(labels.size() * sizeof(uint32_t)));
        o.write((const char*)counts.data(), (std::streamsize)(counts.size() * sizeof(uint32_t)));
        for (const auto& c : clusters) o.write((const char*)c.data(), (std::streamsize)(c.size() * sizeof(rr_component)));
        o.write((const char*)clean.data(), (std::streamsize)clean.size());
        segments.clear();
        radar.segmentMap(occ, grid, h[8], segments, h[9], h[10]);
        o.write((const char*)segments.data(), (std::streamsize)(segments.size() * sizeof(rr_component)));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
