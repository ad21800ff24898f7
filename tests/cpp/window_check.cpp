// C++ driver of RadarHIP::detectWindow (include/radarays_ros_amd/RadarHIP.hpp, over marshal.hpp) -- used by tests/test_window_cpp.py:
// reads one mono8 polar image, its shape and a list of rr_window_detect_config records from a binary file written by the test, detects
// the way a ROS-free caller would and writes, per config, the points and the mask.  Only the C ABI underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <cstring>
#include <fstream>

using namespace radarays_ros_amd;

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[4];                              // n_cells, n_angles, scroll_image, number of configs
    float res;
    f.read((char*)hdr, sizeof(hdr)); f.read((char*)&res, sizeof(res));
    if (!f || hdr[0] < 1 || hdr[1] < 1 || hdr[3] < 1 || hdr[3] > 64) { std::fprintf(stderr, "short or bad input\n"); return 2; }
    std::vector<rr_window_detect_config> cfgs((size_t)hdr[3]);
    f.read((char*)cfgs.data(), (std::streamsize)(cfgs.size() * sizeof(rr_window_detect_config)));
    ImagePtr img = std::make_shared<Image>();
    img->height = (uint32_t)hdr[0]; img->width = img->step = (uint32_t)hdr[1]; img->frame_id = "navtech"; img->stamp = 7.5;
    img->data.resize((size_t)img->height * img->width);
    f.read((char*)img->data.data(), (std::streamsize)img->data.size());
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        // a context needs a map; this one is a single far-away triangle (only the detector is used)
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        radar.loadParams({ RadarMaterial{}, RadarMaterial{ 0.0f, 1.0f, 1.0f, 1.0f } }, { 1 }, 0);
        RadarModelConfig cfg;
        cfg.n_cells = hdr[0]; cfg.scroll_image = hdr[2]; cfg.resolution = res; cfg.n_samples = 4; cfg.include_motion = false;
        radar.updateDynCfg(cfg);
        radar.setBeamSamples({ 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0 });
        std::ofstream o(argv[2], std::ios::binary);
        for (const rr_window_detect_config& c : cfgs) {
            std::vector<uint8_t> mask;
            bool ok = false;
            std::vector<rr_radar_point> pts = radar.detectWindow(img, c, &mask, &ok);
            if (!ok || mask.size() != img->data.size()) { std::fprintf(stderr, "detectWindow failed: %s\n", radar.lastError().c_str()); return 4; }
            // without the mask: the same points
            std::vector<rr_radar_point> again = radar.detectWindow(img, c);
            if (again.size() != pts.size() || (!pts.empty() && std::memcmp(again.data(), pts.data(), pts.size() * sizeof(rr_radar_point)) != 0)) {
                std::fprintf(stderr, "the points differ with and without the mask\n"); return 5;
            }
            const uint64_t n = pts.size();
            o.write((const char*)&n, sizeof(n));
            o.write((const char*)pts.data(), (std::streamsize)(pts.size() * sizeof(rr_radar_point)));
            o.write((const char*)mask.data(), (std::streamsize)mask.size());
        }
        // a refused config and an image of another shape give no points, not ok, and an error text
        rr_window_detect_config bad = cfgs[0];
        bad.train_range = 0; bad.train_azimuth = 0;
        bool ok = true;
        std::vector<uint8_t> mask(3, 1);
        if (!radar.detectWindow(img, bad, &mask, &ok).empty() || ok || !mask.empty() || radar.lastError().find("rr_detect_window") == std::string::npos) {
            std::fprintf(stderr, "a config without training cells was not refused\n"); return 6;
        }
        ImagePtr wrong = std::make_shared<Image>(*img);
        wrong->height -= 1; wrong->data.resize((size_t)wrong->height * wrong->width);
        ok = true;
        if (!radar.detectWindow(wrong, cfgs[0], nullptr, &ok).empty() || ok) { std::fprintf(stderr, "a wrong shape was converted\n"); return 6; }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
