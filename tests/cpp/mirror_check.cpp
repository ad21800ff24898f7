// C++ driver of the RadarHIP methods no other program under tests/cpp/ runs (include/radarays_ros_amd/RadarHIP.hpp) -- used by
// tests/test_gpu_cpp_mirror.py and tests/test_cpp_mirror_host.py.  `mirror_check in.bin out.bin` reads a scene, a config, a beam and
// the inputs of ONE group of calls ("sim", "notes" or "img"), makes the calls the way a ROS-free caller would and writes every result;
// `mirror_check --host in.bin out.bin` runs the static pathToEcho on given rows and needs no GPU.  Only the C ABI underneath.
// Both files are sequences of sections { char tag[16]; uint64 bytes; bytes }: a reader finds a result by its tag and knows its length.
// The constants of the calls (cell windows, Cartesian widths, shift ranges, descriptor and grid shapes) are stated here and again in the test.
#include <radarays_ros_amd/RadarHIP.hpp>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>

using namespace radarays_ros_amd;

namespace {

struct Fail { int code; std::string what; };

std::map<std::string, std::vector<uint8_t>> g_in;
std::ofstream g_out;

void read_sections(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Fail{ 2, std::string("cannot open ") + path };
    for (;;) {
        char tag[16]; uint64_t n = 0;
        f.read(tag, 16);
        if (f.gcount() == 0) break;
        f.read((char*)&n, 8);
        if (!f || tag[15] != 0 || n > ((uint64_t)1 << 30)) throw Fail{ 2, "bad section header" };
        std::vector<uint8_t> b(n);
        f.read((char*)b.data(), (std::streamsize)n);
        if (!f || g_in.count(tag)) throw Fail{ 2, std::string("short or repeated section ") + tag };
        g_in[tag] = std::move(b);
    }
}

template <typename T>
std::vector<T> in(const std::string& tag)
{
    auto it = g_in.find(tag);
    if (it == g_in.end() || it->second.size() % sizeof(T)) throw Fail{ 2, "input section " + tag + " is missing or has a ragged length" };
    std::vector<T> v(it->second.size() / sizeof(T));
    if (!v.empty()) std::memcpy(v.data(), it->second.data(), it->second.size());
    return v;
}

void put(const std::string& tag, const void* p, size_t bytes)
{
    char t[16] = { 0 };
    if (tag.size() > 15) throw Fail{ 2, "tag too long: " + tag };
    std::memcpy(t, tag.data(), tag.size());
    const uint64_t n = bytes;
    g_out.write(t, 16); g_out.write((const char*)&n, 8);
    if (bytes) g_out.write((const char*)p, (std::streamsize)bytes);
}
template <typename T> void put(const std::string& tag, const std::vector<T>& v) { put(tag, v.data(), v.size() * sizeof(T)); }
void put(const std::string& tag, const std::string& s) { put(tag, s.data(), s.size()); }
void put(const std::string& tag, const ImagePtr& im) { put(tag, im->data); }

// an answer was expected
void need(bool ok, const char* what, const RadarHIP& r)
{
    if (!ok) throw Fail{ 4, std::string(what) + " failed: " + r.lastError() };
}
// a refusal was expected: nothing came back, and lastError() says why (the text goes to the test)
void refused(bool nothing_came_back, const std::string& tag, const RadarHIP& r)
{
    if (!nothing_came_back) throw Fail{ 5, tag + ": a bad call was answered" };
    put(tag, r.lastError());
}

ImagePtr make_image(const uint8_t* px, uint32_t h, uint32_t w)
{
    ImagePtr im = std::make_shared<Image>();
    im->height = h; im->width = im->step = w; im->frame_id = "navtech";
    im->data.assign(px, px + (size_t)h * w);
    return im;
}

// the order of the "cfg" section (tests/mirror_io.py: CFG_FIELDS)
RadarModelConfig config_of(const std::vector<double>& v)
{
    if (v.size() != 26) throw Fail{ 2, "cfg must hold 26 values" };
    RadarModelConfig c;
    c.n_cells = (int)v[0]; c.n_samples = (int)v[1]; c.n_reflections = (int)v[2]; c.beam_width = v[3]; c.resolution = v[4];
    c.energy_max = v[5]; c.signal_max = v[6]; c.signal_denoising = (int)v[7];
    c.signal_denoising_triangular_width = (int)v[8]; c.signal_denoising_triangular_mode = v[9];
    c.signal_denoising_gaussian_width = (int)v[10]; c.signal_denoising_gaussian_mode = v[11];
    c.signal_denoising_mb_width = (int)v[12]; c.signal_denoising_mb_mode = v[13];
    c.ambient_noise = (int)v[14]; c.ambient_noise_at_signal_0 = v[15]; c.ambient_noise_at_signal_1 = v[16];
    c.ambient_noise_energy_max = v[17]; c.ambient_noise_energy_min = v[18]; c.ambient_noise_energy_loss = v[19];
    c.scroll_image = (int)v[20]; c.multipath_threshold = v[21]; c.record_multi_reflection = v[22] != 0; c.record_multi_path = v[23] != 0;
    c.beam_sample_dist = (int)v[24]; c.beam_sample_dist_normal_p_in_cone = v[25];
    c.include_motion = false;
    return c;
}

// ---- group "sim": the frame calls with side outputs, and the parameter batch with metrics ------------------------------------------
void group_sim(RadarHIP& radar, uint32_t n_cells)
{
    const uint32_t A = 400;
    ImagePtr first = radar.simulate(1.0);
    need((bool)first, "simulate", radar);
    put("sim0", first);
    // provenance: no stream, then rows shorter than the longest list (truncated rows, true counts)
    const auto ps = in<uint64_t>("prov_stride");
    auto pa = radar.simulateProvenance(2.0);
    need(pa && pa->echoes.empty() && pa->echo_stride == 0, "simulateProvenance(0)", radar);
    put("pa.img", pa->image); put("pa.lab", pa->labels); put("pa.fac", pa->faces); put("pa.cnt", pa->echo_counts);
    auto pb = radar.simulateProvenance(2.0, ps.at(0));
    need(pb && pb->echoes.size() == (size_t)A * ps[0], "simulateProvenance(stride)", radar);
    put("pb.img", pb->image); put("pb.lab", pb->labels); put("pb.fac", pb->faces); put("pb.cnt", pb->echo_counts); put("pb.ech", pb->echoes);
    // paths: the two-run path in the sensor frame, an explicit (short) stride in the map frame
    const auto ws = in<uint64_t>("wave_stride");
    auto wa = radar.simulatePaths(3.0);
    need(wa && wa->wave_stride > 0 && wa->waves.size() == (size_t)A * wa->wave_stride, "simulatePaths(0)", radar);
    put("wa.img", wa->image); put("wa.wav", wa->waves); put("wa.cnt", wa->wave_counts); put("wa.pas", wa->pass_counts);
    const uint64_t wa_stride = wa->wave_stride; put("wa.stride", &wa_stride, 8);
    auto wb = radar.simulatePaths(3.0, ws.at(0), true);
    need(wb && wb->wave_stride == ws[0] && wb->waves.size() == (size_t)A * ws[0], "simulatePaths(stride, map)", radar);
    put("wb.img", wb->image); put("wb.wav", wb->waves); put("wb.cnt", wb->wave_counts); put("wb.pas", wb->pass_counts);
    // pathToEcho on returned rows: for each azimuth asked for, every echo of its stream -> records of (azimuth, k, length, indices...)
    std::vector<int32_t> chains;
    for (int32_t az : in<int32_t>("chain_az")) {
        const rr_wave_rec* row = wa->waves.data() + (size_t)az * wa->wave_stride;
        for (int32_t k = 0; k < (int32_t)pa->echo_counts.at((size_t)az); k++) {
            const std::vector<int32_t> c = RadarHIP::pathToEcho(row, wa->wave_counts[(size_t)az], k);
            chains.push_back(az); chains.push_back(k); chains.push_back((int32_t)c.size());
            chains.insert(chains.end(), c.begin(), c.end());
        }
    }
    put("chains", chains);
    // Doppler: a resting sensor with the two-run path, a moving one with a short explicit stride
    const auto dg = in<float>("dop");          // gain, vx, vy, vz
    const auto ds = in<uint64_t>("dop_stride");
    auto da = radar.simulateDoppler(4.0, nullptr, dg.at(0));
    need(da && da->echo_stride > 0 && da->echo_vel.size() == (size_t)A * da->echo_stride, "simulateDoppler(0)", radar);
    put("da.img", da->image); put("da.vel", da->echo_vel); put("da.cel", da->echo_cells); put("da.cnt", da->echo_counts); put("da.vim", da->vel_image);
    const uint64_t da_stride = da->echo_stride; put("da.stride", &da_stride, 8);
    if (dg.size() != 4) throw Fail{ 2, "dop must be gain, vx, vy, vz" };
    auto db = radar.simulateDoppler(4.0, dg.data() + 1, dg[0], ds.at(0));
    need(db && db->echo_stride == ds[0] && db->echo_cells.size() == (size_t)A * ds[0], "simulateDoppler(stride, velocity)", radar);
    put("db.img", db->image); put("db.vel", db->echo_vel); put("db.cel", db->echo_cells); put("db.cnt", db->echo_counts); put("db.vim", db->vel_image);
    // the parameter batch with metrics: sets that differ in materials, n_reflections and one beam_width; with and without images
    const auto pm = in<float>("ps.mats"); const auto pn = in<int32_t>("ps.nref"); const auto pw = in<float>("ps.bw");
    const auto real_px = in<uint8_t>("real");
    if (real_px.size() != (size_t)n_cells * A) throw Fail{ 2, "real must be n_cells x 400" };
    ImagePtr real = make_image(real_px.data(), n_cells, A);
    const RadarParams cur = radar.getParams();
    const size_t n_sets = pn.size(), n_mat = cur.materials.size();
    if (pm.size() != n_sets * n_mat * 4 || pw.size() != n_sets) throw Fail{ 2, "ps.* do not agree" };
    std::vector<RadarParams> sets(n_sets, cur);
    for (size_t k = 0; k < n_sets; k++) {
        for (size_t m = 0; m < n_mat; m++) { const float* q = &pm[(k * n_mat + m) * 4]; sets[k].materials[m] = { q[0], q[1], q[2], q[3] }; }
        sets[k].model.n_reflections = (uint32_t)pn[k]; sets[k].model.beam_width = pw[k];
    }
    const uint32_t which = RR_METRIC_PSNR | RR_METRIC_SSIM | RR_METRIC_INFO;
    std::vector<ImagePtr> imgs; std::vector<rr_image_metrics> rec, rec_only;
    need(radar.simulateParamSetsMetrics(sets, 5.0, &imgs, *real, which, 7, &rec) && imgs.size() == n_sets && rec.size() == n_sets, "simulateParamSetsMetrics", radar);
    need(radar.simulateParamSetsMetrics(sets, 5.0, nullptr, *real, which, 7, &rec_only) && rec_only.size() == n_sets, "simulateParamSetsMetrics(no images)", radar);
    std::vector<uint8_t> flat;
    for (const ImagePtr& im : imgs) flat.insert(flat.end(), im->data.begin(), im->data.end());
    put("pm.img", flat); put("pm.rec", rec); put("pn.rec", rec_only);
    const std::vector<rr_image_metrics> cmp = radar.compareImages(imgs, *real, which, 7);
    need(cmp.size() == n_sets, "compareImages", radar);
    put("pm.cmp", cmp);
    ImagePtr last = radar.simulate(6.0);
    need((bool)last, "simulate (last)", radar);
    put("sim1", last);
}

// ---- group "notes": annotations across one RR_MAX_BATCH chunk -------------------------------------------------------------------------
// simulate() runs with include_motion and a per-azimuth table; simulateAnnotations takes one pose per frame, so it has to take the table
// out and simulate() has to put it back: s0 and s1 are the table's frame, the annotation images are the poses' frames
void group_notes(RadarHIP& radar)
{
    const auto poses = in<float>("poses");
    const size_t n = poses.size() / 7;
    if (n != (size_t)RR_MAX_BATCH + 1 || poses.size() % 7) throw Fail{ 2, "poses must be [RR_MAX_BATCH + 1][7]" };
    const std::vector<float> last(poses.end() - 7, poses.end());
    radar.updateTsm(last.data());
    ImagePtr before = radar.simulate(1.0);
    need((bool)before, "simulate", radar);
    put("s0", before);
    const uint32_t mask = RR_NOTE_DIRECT | RR_NOTE_GHOST;
    auto an = radar.simulateAnnotations(poses, 2.0, mask, false);
    need(an && an->images.empty() && an->notes.size() == n * radar.objectCount() && an->skipped.size() == n, "simulateAnnotations", radar);
    put("an.notes", an->notes); put("an.skip", an->skipped);
    auto ai = radar.simulateAnnotations(poses, 2.0, mask, true);
    need(ai && ai->images.size() == n && ai->n_objects == radar.objectCount(), "simulateAnnotations(images)", radar);
    std::vector<uint8_t> flat;
    for (const ImagePtr& im : ai->images) flat.insert(flat.end(), im->data.begin(), im->data.end());
    put("ai.notes", ai->notes); put("ai.skip", ai->skipped); put("ai.img", flat);
    auto a1 = radar.simulateAnnotations(last, 3.0, mask, true);
    need(a1 && a1->images.size() == 1 && a1->notes.size() == radar.objectCount(), "simulateAnnotations(one pose)", radar);
    put("a1.notes", a1->notes); put("a1.skip", a1->skipped); put("a1.img", a1->images[0]);
    std::vector<float> ragged(poses.begin(), poses.begin() + 8);
    refused(!radar.simulateAnnotations(ragged, 4.0), "rf.poses", radar);
    ImagePtr after = radar.simulate(5.0);
    need((bool)after, "simulate (after)", radar);
    put("s1", after);
}

// ---- group "img": the calls on given images and on the clouds detect() makes of them -----------------------------------------------------
void group_img(RadarHIP& radar, uint32_t n_cells)
{
    const uint32_t A = 400;
    const size_t npx = (size_t)n_cells * A;
    const auto px = in<uint8_t>("imgs");
    if (px.size() != 6 * npx) throw Fail{ 2, "imgs must be [6][n_cells][400]" };
    std::vector<ImagePtr> im;
    for (size_t k = 0; k < 6; k++) im.push_back(make_image(px.data() + k * npx, n_cells, A));
    const ImagePtr real = im[5];
    const std::vector<ImagePtr> three(im.begin(), im.begin() + 3), two(im.begin(), im.begin() + 2), five(im.begin(), im.begin() + 5);
    ImagePtr wrong = std::make_shared<Image>(*im[0]);
    wrong->height -= 1; wrong->data.resize((size_t)wrong->height * wrong->width);

    // azimuth registration: the default window (cell_end = -1), and (5, 64) with the curve
    const std::vector<rr_align_record> al = radar.alignImages(three, *real);
    need(al.size() == 3, "alignImages", radar);
    put("al.rec", al);
    std::vector<int64_t> curve;
    const std::vector<rr_align_record> al2 = radar.alignImages(three, *real, 5, 64, &curve);
    need(al2.size() == 3 && curve.size() == 3 * (size_t)A, "alignImages(window, curve)", radar);
    put("al2.rec", al2); put("al2.cur", curve);
    // translation registration: the real image rides as image n through one conversion
    std::vector<double> corr;
    const std::vector<rr_shift_record> sh = radar.registerTranslation(two, *real, 65, 0.25f, 3, true, &corr);
    need(sh.size() == 2 && corr.size() == 4, "registerTranslation(65, 3, bilinear)", radar);
    put("sh.rec", sh); put("sh.cor", corr);
    const std::vector<rr_shift_record> sh2 = radar.registerTranslation(two, *real, 64, 0.25f, 16, false);
    need(sh2.size() == 2, "registerTranslation(64, 16, nearest)", radar);
    put("sh2.rec", sh2);
    // place recognition: a database of five, the sixth image looked up
    rr_place_config pc{};
    pc.cell_begin = 0; pc.cell_end = (int)n_cells; pc.n_rings = 10; pc.n_sectors = 40;
    const std::vector<uint8_t> desc = radar.describeImages(five, pc);
    need(desc.size() == 5 * 400, "describeImages", radar);
    put("pl.desc", desc);
    const std::vector<rr_place_match> top3 = radar.localize(*real, desc, 5, pc, 3), top5 = radar.localize(*real, desc, 5, pc, 5);
    need(top3.size() == 3 && top5.size() == 5, "localize", radar);
    put("pl.top3", top3); put("pl.top5", top5);
    refused(radar.localize(*real, desc, 5, pc, 6).empty(), "rf.topk", radar);
    // sweep compensation on the points detect() makes of image 0
    rr_detect_config det; rr_default_detect_config(&det);
    const std::vector<rr_radar_point> pts = radar.detect(im[0], det);
    need(pts.size() >= 200, "detect (at least 200 points)", radar);
    put("dt.pts", pts);
    const auto az = in<float>("azposes"); const auto ref = in<float>("refpose"); const auto vel = in<float>("svel");
    if (ref.size() != 7 || vel.size() != 3) throw Fail{ 2, "refpose [7], svel [3]" };
    const std::vector<rr_sweep_rec> t0 = radar.sweepTable(az, ref.data()), t1 = radar.sweepTable(az, ref.data(), vel.data(), 0.03125f);
    need(t0.size() == A && t1.size() == A, "sweepTable", radar);
    put("sw.t0", t0); put("sw.t1", t1);
    const std::vector<rr_radar_point> cp0 = radar.compensatePointClouds(pts, t0), cp1 = radar.compensatePointClouds(pts, t1);
    need(cp0.size() == pts.size() && cp1.size() == pts.size(), "compensatePointClouds", radar);
    put("cp.0", cp0); put("cp.1", cp1);
    ImagePtr cc1 = radar.compensatedCartesian(im[0], t1, 65, 0.25f, false, 1), cc2 = radar.compensatedCartesian(im[0], t1, 65, 0.25f, true, 2);
    need(cc1 && cc2 && cc1->data.size() == 65 * 65 && cc2->width == 65 && cc2->height == 65, "compensatedCartesian", radar);
    put("cc.1", cc1); put("cc.2", cc2);
    // scan matching: three clouds of different sizes, the middle one empty, against the first 200 detections
    const std::vector<rr_radar_point> tgt(pts.begin(), pts.begin() + 200);
    const std::vector<std::vector<rr_radar_point>> clouds = { { cp1.begin(), cp1.begin() + 65 }, {}, { cp1.begin() + 20, cp1.begin() + 60 } };
    const auto init = in<double>("icp_init");
    const std::vector<rr_icp_rec> ia = radar.registerPointClouds(clouds, tgt, 1.5f, 4), ib = radar.registerPointClouds(clouds, tgt, 1.5f, 0, init),
                                  ic = radar.registerPointClouds(clouds, tgt, 1.5f, 4, init);
    need(ia.size() == 3 && ib.size() == 3 && ic.size() == 3, "registerPointClouds", radar);
    put("ic.a", ia); put("ic.b", ib); put("ic.c", ic);
    const auto hyp_pose = in<float>("hyp_pose");
    if (hyp_pose.size() != 7) throw Fail{ 2, "hyp_pose [7]" };
    const std::array<float, 7> fixed = RadarHIP::correctedPose(hyp_pose.data(), ic[0]);
    put("ic.pose", fixed.data(), sizeof(float) * 7);
    // likelihood field: two clouds of different sizes under two states and under none; 33 hypotheses, a scan of 65 points and an empty one
    rr_field_config fc{};
    fc.width = 64; fc.height = 48; fc.cell = 0.5f; fc.x0 = -16.0f; fc.y0 = -12.0f; fc.max_dist = 20; fc.gate = 2;
    const std::vector<std::vector<rr_radar_point>> keys = { { pts.begin(), pts.begin() + 65 }, { pts.begin() + 65, pts.begin() + 95 } };
    const auto states = in<double>("fstates");
    const std::vector<uint16_t> fa = radar.buildLikelihoodField(keys, states, fc), fb = radar.buildLikelihoodField(keys, {}, fc);
    need(fa.size() == 64 * 48 && fb.size() == 64 * 48, "buildLikelihoodField", radar);
    put("fd.a", fa); put("fd.b", fb);
    const auto hyps = in<float>("hyps");
    const std::vector<rr_radar_point> scan(pts.begin() + 100, pts.begin() + 165);
    const std::vector<rr_field_rec> sa = radar.scorePoses(scan, hyps, fa, fc), se = radar.scorePoses({}, hyps, fa, fc);
    need(sa.size() == 33 && se.size() == 33, "scorePoses (33 hypotheses; an empty scan scores zero)", radar);
    put("sc.a", sa); put("sc.e", se);
    // refusals, one bad input per family; the text of each goes to the test
    refused(radar.alignImages({ wrong }, *real).empty(), "rf.align", radar);
    refused(radar.registerTranslation({ wrong }, *real, 65, 0.25f, 3).empty(), "rf.shift", radar);
    refused(radar.describeImages({ wrong }, pc).empty(), "rf.desc", radar);
    refused(!radar.compensatedCartesian(wrong, t1, 65, 0.25f), "rf.cart", radar);
    const std::vector<rr_sweep_rec> short_table(t1.begin(), t1.end() - 1);
    refused(radar.compensatePointClouds(pts, short_table).empty(), "rf.table", radar);
    refused(!radar.compensatedCartesian(im[0], short_table, 65, 0.25f), "rf.carttab", radar);
    refused(radar.sweepTable(std::vector<float>(az.begin(), az.end() - 7), ref.data()).empty(), "rf.sweep", radar);
    refused(radar.registerPointClouds(clouds, tgt, 1.5f, 4, std::vector<double>(5, 1.0)).empty(), "rf.init", radar);
    refused(radar.buildLikelihoodField(keys, std::vector<double>(7, 1.0), fc).empty(), "rf.states", radar);
    refused(radar.scorePoses(scan, std::vector<float>(6, 1.0f), fa, fc).empty(), "rf.hyps", radar);
    refused(radar.localize(*real, std::vector<uint8_t>(desc.begin(), desc.end() - 1), 5, pc, 3).empty(), "rf.db", radar);
    // ... and the next valid call of each family answers as before
    put("al.again", radar.alignImages(three, *real));
    put("sh.again", radar.registerTranslation(two, *real, 65, 0.25f, 3, true));
    put("pl.again", radar.localize(*real, desc, 5, pc, 3));
    put("cp.again", radar.compensatePointClouds(pts, t1));
    ImagePtr cc = radar.compensatedCartesian(im[0], t1, 65, 0.25f, true, 2);
    need((bool)cc, "compensatedCartesian (again)", radar);
    put("cc.again", cc);
    put("ic.again", radar.registerPointClouds(clouds, tgt, 1.5f, 4, init));
    put("fd.again", radar.buildLikelihoodField(keys, states, fc));
    put("sc.again", radar.scorePoses(scan, hyps, fa, fc));
}

// ---- --host: pathToEcho on given rows, no context ---------------------------------------------------------------------------------------
void host_mode()
{
    const auto waves = in<rr_wave_rec>("waves");
    const auto n = in<uint64_t>("n");               // how many of the rows the list holds (a truncated list: fewer than its indices reach)
    std::vector<int32_t> chains;
    for (int32_t k : in<int32_t>("ks")) {
        const std::vector<int32_t> c = RadarHIP::pathToEcho(waves.data(), (size_t)n.at(0), k);
        chains.push_back(k); chains.push_back((int32_t)c.size());
        chains.insert(chains.end(), c.begin(), c.end());
    }
    put("chains", chains);
}

}  // namespace

int main(int argc, char** argv)
{
    const bool host = argc > 1 && std::string(argv[1]) == "--host";
    if (argc < (host ? 4 : 3)) { std::fprintf(stderr, "usage: %s [--host] in.bin out.bin\n", argv[0]); return 2; }
    try {
        read_sections(argv[host ? 2 : 1]);
        g_out.open(argv[host ? 3 : 2], std::ios::binary);
        if (!g_out) throw Fail{ 2, "cannot write the output file" };
        if (host) { host_mode(); put("done", std::string("host")); g_out.close(); return g_out ? 0 : 2; }
        const auto group = in<char>("group");
        const std::string g(group.begin(), group.end());
        const auto mats = in<float>("mats"); const auto objmat = in<int32_t>("objmat"); const auto pose = in<float>("pose");
        if (pose.size() != 7 || mats.size() % 4) throw Fail{ 2, "pose [7], mats [n][4]" };
        RadarHIP radar("map", "navtech", in<float>("verts"), in<uint32_t>("faces"), in<uint32_t>("fobj"), 0);
        std::vector<RadarMaterial> m(mats.size() / 4);
        for (size_t i = 0; i < m.size(); i++) m[i] = { mats[4 * i], mats[4 * i + 1], mats[4 * i + 2], mats[4 * i + 3] };
        radar.loadParams(m, std::vector<int>(objmat.begin(), objmat.end()), 0);
        RadarModelConfig cfg = config_of(in<double>("cfg"));
        if (g == "notes") {                        // a per-azimuth table under simulate(): the batch calls must not render with it
            cfg.include_motion = true;
            radar.setMotionPoses(in<float>("motion"));
        }
        radar.updateDynCfg(cfg);
        radar.setBeamSeed(11);                     // what a parameter set of another beam_width is drawn with
        radar.setBeamSamples(in<float>("beams"));
        radar.updateTsm(pose.data());
        if (g == "sim") group_sim(radar, (uint32_t)cfg.n_cells);
        else if (g == "notes") group_notes(radar);
        else if (g == "img") group_img(radar, (uint32_t)cfg.n_cells);
        else throw Fail{ 2, "unknown group " + g };
        put("done", g);                            // the last section: a reader knows the run came to its end
        g_out.close();
        if (!g_out) throw Fail{ 2, "writing the output failed" };
    } catch (const Fail& f) {
        std::fprintf(stderr, "%s\n", f.what.c_str());
        return f.code;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    return 0;
}
