// Host-side argument handling of the object annotations (include/radarays_mi355.h) -- used by tests/test_notes_host.py: needs no GPU.
// The record layout the kernels write in five 16-byte stores, the closed form of the scratch size, and what every entry point answers
// to a null context.  Only the C ABI underneath.
#include <radarays_mi355.h>

#include <cstddef>
#include <cstdio>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "notes_check: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

int main()
{
    static_assert(sizeof(rr_object_note) == 80, "five 16-byte stores");
    static_assert(offsetof(rr_object_note, bin_min) == 16 && offsetof(rr_object_note, peak) == 32 && offsetof(rr_object_note, sum_intensity) == 48 &&
                  offsetof(rr_object_note, x_min) == 56 && offsetof(rr_object_note, y_min) == 64 && offsetof(rr_object_note, reserved1_) == 72, "layout");
    CHECK((RR_NOTE_DIRECT | RR_NOTE_GHOST | RR_NOTE_MULTIPATH) == 7u);
    // 64 bytes per (frame, object) plus one bit per azimuth in whole words, the total a multiple of 16
    CHECK(rr_annotate_scratch_bytes(1, 1, 400) == 64 + 13 * 4 + 12);
    CHECK(rr_annotate_scratch_bytes(3, 5, 37) == 3 * 5 * (64 + 2 * 4) + 8);
    CHECK(rr_annotate_scratch_bytes(16, 1000, 400) == (size_t)16 * 1000 * (64 + 52));
    CHECK(rr_annotate_scratch_bytes(3, 8192 * 64, 64) == (size_t)3 * 8192 * 64 * 72);
    CHECK(rr_annotate_scratch_bytes(0, 1, 400) == 0 && rr_annotate_scratch_bytes(1, 0, 400) == 0 && rr_annotate_scratch_bytes(1, 1, 0) == 0);
    // a null context: -1, whatever else is passed, and nothing is touched
    rr_object_note note[2];
    uint32_t word[8] = { 7, 7, 7, 7, 7, 7, 7, 7 };
    uint8_t px[4] = { 7, 7, 7, 7 };
    float pose[7] = { 0, 0, 0, 1, 0, 0, 0 };
    rr_cartesian_config cc = { 2, 0, 1.0f, 0 };
    rr_radar_point pt = { 0, 0, 0, 0, 0, 0 };
    CHECK(rr_annotate_labels_device(nullptr, word, px, 1, 1, 1u, note, word, word, 1024, nullptr) == -1);
    CHECK(rr_annotate_labels(nullptr, word, px, 1, 1, 1u, note, word) == -1);
    CHECK(rr_label_points_device(nullptr, &pt, word, 1, 1, word, nullptr, nullptr, word, nullptr, nullptr, nullptr) == -1);
    CHECK(rr_polar_to_cartesian_labels_device(nullptr, word, 1, &cc, word, nullptr) == -1);
    CHECK(rr_polar_to_cartesian_labels(nullptr, word, 1, &cc, word) == -1);
    CHECK(rr_simulate_batch_annotations(nullptr, pose, 1, 1u, px, note, word) == -1);
    for (uint32_t w : word) CHECK(w == 7u);
    for (uint8_t b : px) CHECK(b == 7);
    std::puts("notes_check: ok");
    return 0;
}
