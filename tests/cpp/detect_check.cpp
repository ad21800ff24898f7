// C++ driver of RadarHIP::detect / RadarHIP::toCartesian (include/radarays_ros_amd/RadarHIP.hpp) -- used by
// tests/test_gpu_detect_cpp.py: reads one mono8 polar image and its shape from a binary file written by the test, converts
// it the way a ROS-free caller would, writes the points and the Cartesian image.  Only the C ABI underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <fstream>

using namespace radarays_ros_amd;

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[5];                              // n_cells, n_angles, scroll_image, k, cartesian width
    float geo[2];                                // resolution, pixel size
    f.read((char*)hdr, sizeof(hdr)); f.read((char*)geo, sizeof(geo));
    ImagePtr img = std::make_shared<Image>();
    img->height = (uint32_t)hdr[0]; img->width = img->step = (uint32_t)hdr[1]; img->frame_id = "navtech"; img->stamp = 7.5;
    img->data.resize((size_t)img->height * img->width);
    f.read((char*)img->data.data(), (std::streamsize)img->data.size());
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        // a context needs a map; this one is a single far-away triangle (only the conversions are used)
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        radar.loadParams({ RadarMaterial{}, RadarMaterial{ 0.0f, 1.0f, 1.0f, 1.0f } }, { 1 }, 0);
        RadarModelConfig cfg;
        cfg.n_cells = hdr[0]; cfg.scroll_image = hdr[2]; cfg.resolution = geo[0]; cfg.n_samples = 4; cfg.include_motion = false;
        radar.updateDynCfg(cfg);
        radar.setBeamSamples({ 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0 });
        rr_detect_config det; rr_default_detect_config(&det);
        std::vector<rr_radar_point> cfar = radar.detect(img, det);
        det.method = 1; det.k = hdr[3];
        std::vector<rr_radar_point> kst = radar.detect(img, det);
        ImagePtr cart = radar.toCartesian(img, hdr[4], geo[1], true);
        if (cfar.empty() || kst.empty() || !cart) { std::fprintf(stderr, "conversion failed: %s\n", radar.lastError().c_str()); return 4; }
        if (cart->height != (uint32_t)hdr[4] || cart->width != (uint32_t)hdr[4] || cart->step != cart->width ||
            cart->encoding != "mono8" || cart->frame_id != "navtech" || cart->stamp != 7.5) { std::fprintf(stderr, "bad Cartesian image\n"); return 5; }
        // an image of another shape is refused, not converted
        ImagePtr wrong = std::make_shared<Image>(*img);
        wrong->height -= 1; wrong->data.resize((size_t)wrong->height * wrong->width);
        if (!radar.detect(wrong, det).empty() || radar.toCartesian(wrong, 8, 1.0f)) { std::fprintf(stderr, "a wrong shape was converted\n"); return 6; }
        std::ofstream o(argv[2], std::ios::binary);
        uint64_t n[2] = { cfar.size(), kst.size() };
        o.write((const char*)n, sizeof(n));
        o.write((const char*)cfar.data(), (std::streamsize)(cfar.size() * sizeof(rr_radar_point)));
        o.write((const char*)kst.data(), (std::streamsize)(kst.size() * sizeof(rr_radar_point)));
        o.write((const char*)cart->data.data(), (std::streamsize)cart->data.size());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
