// C++ driver of RadarHIP::optimizePoseGraph (include/radarays_ros_amd/RadarHIP.hpp) -- used by tests/test_gpu_graph_cpp.py: reads a config,
// states, fixed flags and edges from a binary file written by the test, optimises, and writes the states and the records.  Only the C ABI
// underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <fstream>

using namespace radarays_ros_amd;

static_assert(sizeof(rr_graph_edge) == 48 && sizeof(rr_graph_config) == 32 && sizeof(rr_graph_rec) == 32, "an edge: 48 bytes; a config and a record: 32");

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    // nodes, edges; the config; the states, the fixed flags, the edges
    int32_t h[2];
    rr_graph_config cfg;
    f.read((char*)h, sizeof(h));
    f.read((char*)&cfg, sizeof(cfg));
    if (!f || h[0] < 1 || h[0] > 4096 || h[1] < 0 || h[1] > 65536) { std::fprintf(stderr, "short input\n"); return 2; }
    std::vector<double> states(4 * (size_t)h[0]);
    std::vector<uint8_t> fixed((size_t)h[0]);
    std::vector<rr_graph_edge> edges((size_t)h[1]);
    f.read((char*)states.data(), (std::streamsize)(states.size() * sizeof(double)));
    f.read((char*)fixed.data(), (std::streamsize)fixed.size());
    f.read((char*)edges.data(), (std::streamsize)(edges.size() * sizeof(rr_graph_edge)));
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        // a context needs a map; this one is a single far-away triangle (only the graph call is used)
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        const std::vector<double> start(states);
        const std::vector<rr_graph_rec> recs = radar.optimizePoseGraph(states, fixed, edges, cfg);
        if (recs.size() != (size_t)cfg.iterations + 1) { std::fprintf(stderr, "optimizePoseGraph failed: %s\n", radar.lastError().c_str()); return 4; }
        // no node, states of the wrong shape, a reserved word, too many CG steps and a negative lambda are refused, and the states stay
        std::vector<double> x(start), none;
        rr_graph_config reserved = cfg, steps = cfg, lambda = cfg;
        reserved.reserved_[1] = 1;
        steps.cg_iterations = 1025;
        lambda.lambda = -1.0;
        if (!radar.optimizePoseGraph(none, {}, edges, cfg).empty()) { std::fprintf(stderr, "no node was taken\n"); return 5; }
        x.pop_back();
        if (!radar.optimizePoseGraph(x, fixed, edges, cfg).empty()) { std::fprintf(stderr, "short states were taken\n"); return 5; }
        x = start;
        if (!radar.optimizePoseGraph(x, fixed, edges, steps).empty()) { std::fprintf(stderr, "1025 CG steps were taken\n"); return 5; }
        if (!radar.optimizePoseGraph(x, fixed, edges, lambda).empty()) { std::fprintf(stderr, "a negative lambda was taken\n"); return 5; }
        if (!radar.optimizePoseGraph(x, fixed, edges, reserved).empty() || x != start) { std::fprintf(stderr, "a reserved word was taken\n"); return 5; }
        if (radar.lastError().find("reserved_") == std::string::npos) { std::fprintf(stderr, "the refusal does not say why: %s\n", radar.lastError().c_str()); return 5; }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)states.data(), (std::streamsize)(states.size() * sizeof(double)));
        o.write((const char*)recs.data(), (std::streamsize)(recs.size() * sizeof(rr_graph_rec)));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
