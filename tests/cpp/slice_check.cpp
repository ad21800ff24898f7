// C++ driver of RadarHIP::buildMeshMap (include/radarays_ros_amd/RadarHIP.hpp) -- used by tests/test_gpu_slice.py: reads a mesh, a grid, two
// bands and a skip list from a binary file written by the test, slices the mesh once with the skip list and the object plane and once in
// two calls that accumulate two bands, and writes the two maps and the plane.  Only the C ABI underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <fstream>

using namespace radarays_ros_amd;

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[5];                              // vertices, faces, width, height, skipped objects
    float geo[7];                                // cell, x0, y0, z_lo, z_hi of the first band, z_lo, z_hi of the second
    f.read((char*)hdr, sizeof(hdr)); f.read((char*)geo, sizeof(geo));
    if (!f || hdr[0] < 3 || hdr[1] < 1 || hdr[4] < 0) { std::fprintf(stderr, "short input\n"); return 2; }
    std::vector<float> verts(3 * (size_t)hdr[0]);
    std::vector<uint32_t> faces(3 * (size_t)hdr[1]), face_object((size_t)hdr[1]), skip((size_t)hdr[4]);
    f.read((char*)verts.data(), (std::streamsize)(verts.size() * sizeof(float)));
    f.read((char*)faces.data(), (std::streamsize)(faces.size() * sizeof(uint32_t)));
    f.read((char*)face_object.data(), (std::streamsize)(face_object.size() * sizeof(uint32_t)));
    f.read((char*)skip.data(), (std::streamsize)(skip.size() * sizeof(uint32_t)));
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        RadarHIP radar("map", "navtech", verts, faces, face_object, 0);
        rr_field_config grid = { hdr[2], hdr[3], geo[0], geo[1], geo[2], 8, 0, 0 };
        std::vector<uint32_t> objects;
        std::vector<uint8_t> first = radar.buildMeshMap(grid, geo[3], geo[4], skip, &objects);
        if (first.empty()) { std::fprintf(stderr, "slice failed: %s\n", radar.lastError().c_str()); return 4; }
        // the second band first, then the first band into the same map, nothing skipped
        std::vector<uint8_t> both = radar.buildMeshMap(grid, geo[5], geo[6]);
        if (!both.empty()) both = radar.buildMeshMap(grid, geo[3], geo[4], {}, nullptr, both);
        if (both.empty()) { std::fprintf(stderr, "accumulation failed: %s\n", radar.lastError().c_str()); return 4; }
        // an inverted band, an unknown object and a map of the wrong size are refused
        if (!radar.buildMeshMap(grid, geo[4] + 1.0f, geo[3]).empty()) { std::fprintf(stderr, "an inverted band was taken\n"); return 5; }
        if (!radar.buildMeshMap(grid, geo[3], geo[4], { (uint32_t)radar.objectCount() }).empty()) { std::fprintf(stderr, "an unknown object was taken\n"); return 5; }
        if (!radar.buildMeshMap(grid, geo[3], geo[4], {}, nullptr, std::vector<uint8_t>(3, 0)).empty()) { std::fprintf(stderr, "a short map was taken\n"); return 5; }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)first.data(), (std::streamsize)first.size());
        o.write((const char*)objects.data(), (std::streamsize)(objects.size() * sizeof(uint32_t)));
        o.write((const char*)both.data(), (std::streamsize)both.size());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
