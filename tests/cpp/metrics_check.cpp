// C++ driver of RadarHIP::compareImages (include/radarays_ros_amd/RadarHIP.hpp) -- used by tests/test_gpu_metrics.py: reads
// n mono8 polar images and one real image from a binary file written by the test, compares them the way a ROS-free caller
// would, writes the records.  Only the C ABI underneath.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <fstream>

using namespace radarays_ros_amd;

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[5];                              // n images, n_cells, n_angles, which, win_size
    f.read((char*)hdr, sizeof(hdr));
    auto read_image = [&]() {
        ImagePtr img = std::make_shared<Image>();
        img->height = (uint32_t)hdr[1]; img->width = img->step = (uint32_t)hdr[2];
        img->data.resize((size_t)img->height * img->width);
        f.read((char*)img->data.data(), (std::streamsize)img->data.size());
        return img;
    };
    ImagePtr real = read_image();
    std::vector<ImagePtr> imgs;
    for (int k = 0; k < hdr[0]; k++) imgs.push_back(read_image());
    if (!f) { std::fprintf(stderr, "short input\n"); return 2; }
    try {
        // a context needs a map; this one is a single far-away triangle (only the comparison is used)
        std::vector<float> verts = { 500, 0, 0, 500, 1, 0, 500, 0, 1 };
        RadarHIP radar("map", "navtech", verts, { 0, 1, 2 }, { 0 }, 0);
        radar.loadParams({ RadarMaterial{}, RadarMaterial{ 0.0f, 1.0f, 1.0f, 1.0f } }, { 1 }, 0);
        RadarModelConfig cfg;
        cfg.n_cells = hdr[1]; cfg.n_samples = 4; cfg.include_motion = false;
        radar.updateDynCfg(cfg);
        radar.setBeamSamples({ 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0 });
        std::vector<rr_image_metrics> rec = radar.compareImages(imgs, *real, (uint32_t)hdr[3], hdr[4]);
        if (rec.size() != imgs.size()) { std::fprintf(stderr, "comparison failed: %s\n", radar.lastError().c_str()); return 4; }
        // an image of another shape and an even window are refused, not compared
        ImagePtr wrong = std::make_shared<Image>(*imgs[0]);
        wrong->height -= 1; wrong->data.resize((size_t)wrong->height * wrong->width);
        if (!radar.compareImages({ wrong }, *real).empty() || !radar.compareImages(imgs, *real, RR_METRIC_SSIM, 8).empty()) {
            std::fprintf(stderr, "a bad call was answered\n"); return 6;
        }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)rec.data(), (std::streamsize)(rec.size() * sizeof(rr_image_metrics)));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
