"""Object annotations without a GPU: the feature's header text and facades (names, prototypes and the record layout: tests/test_abi.py), what a null context
gets, the kernels' resource use -- and the numpy restatement of the definition (tests/notes_ref.py), which the GPU tests
(tests/test_gpu_notes.py) hold the kernels to, against closed forms on hand-made planes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import notes_ref as R
from radarays_ros_amd import native, radar
from radarays_ros_amd.native import LABEL_NONE, NOTE_DIRECT, NOTE_GHOST, NOTE_MULTIPATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
A, N = 40, 12          # azimuths and bins of the hand-made planes
GEO = dict(scroll=0, theta_min=0.0, theta_inc=float(np.float32(-2 * np.pi / A)), resolution=0.5)


def info(obj, pas=0, kind=0):
    return np.uint32(obj | pas << 24 | kind << 28)


def plane():
    return np.full((N, A), LABEL_NONE, np.uint32)


def one(labels, img=None, n_objects=2, mask=NOTE_DIRECT, **geo):
    return R.annotate_frame(labels, img, n_objects, mask, **dict(GEO, **geo))


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header and native_lib.lib().rr_abi_version() == 7
    section = header[header.index("---- object annotations"):header.index("---- translation registration")]
    assert section.count("UNPINNED") == 1
    for name, bit in (("RR_NOTE_DIRECT", 1), ("RR_NOTE_GHOST", 2), ("RR_NOTE_MULTIPATH", 4)):
        assert re.search(r"#define %s\s+%du" % (name, bit), section), name
    assert (NOTE_DIRECT, NOTE_GHOST, NOTE_MULTIPATH, native_lib.NOTE_ALL) == (1, 2, 4, 7)
    for word in ("rr_multi", "arameter batches", "elocities per object", "riented boxes"):          # what is out of scope is said
        assert word in section, word
    for m in ("annotate_labels", "annotate_labels_device", "label_points_device", "polar_to_cartesian_labels", "polar_to_cartesian_labels_device",
              "simulate_batch_annotations"):
        assert callable(getattr(native_lib.Context, m)), m
    assert callable(radar.RadarHIP.simulate_annotations)
    inc = os.path.join(ROOT, "include", "radarays_ros_amd")
    assert "simulateAnnotations" in open(os.path.join(inc, "RadarHIP.hpp")).read()
    assert "rr_simulate_batch_annotations" in open(os.path.join(inc, "marshal.hpp")).read()


def test_a_null_context_gets_minus_one(native_lib):
    L = native_lib.lib()
    w = np.full(64, 7, np.uint32)
    p = w.ctypes.data
    cc = native_lib.cartesian_config(2, 1.0, False)
    assert L.rr_annotate_labels_device(None, p, p, 1, 1, 1, p, p, p, 1024, None) == -1
    assert L.rr_annotate_labels(None, p, p, 1, 1, 1, p, p) == -1
    assert L.rr_label_points_device(None, p, p, 1, 1, p, None, None, p, None, None, None) == -1
    assert L.rr_polar_to_cartesian_labels_device(None, p, 1, ctypes.byref(cc), p, None) == -1
    assert L.rr_polar_to_cartesian_labels(None, p, 1, ctypes.byref(cc), p) == -1
    assert L.rr_simulate_batch_annotations(None, p, 1, 1, p, p, p) == -1
    assert (w == 7).all()
    assert L.rr_annotate_scratch_bytes(3, 5, 37) == 3 * 5 * (64 + 8) + 8 and L.rr_annotate_scratch_bytes(0, 5, 37) == 0


def test_wrappers_refuse_bad_arguments_before_the_library():
    for bad in (8, -1, "shadow", ["direct", "x"], None, True, 1.0):
        with pytest.raises(ValueError):
            native.note_mask(bad)
    assert native.note_mask(["direct", "ghost"]) == 3 and native.note_mask("multipath") == 4 and native.note_mask(7) == 7 and native.note_mask(0) == 0


def test_the_stand_alone_program_checks_the_argument_handling(native_lib, tmp_path):
    native_lib.build()
    exe = str(tmp_path / "notes_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "notes_check.cpp"), "-o", exe,
                    "-L", os.path.join(ROOT, "radarays_ros_amd"), "-lradarays_mi355", "-Wl,-rpath," + os.path.join(ROOT, "radarays_ros_amd")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "notes_check: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_notes_kernels_use_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-notes"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, name in ((r"ScratchSize \[bytes/lane\]", "scratch"), (r"LDS Size \[bytes/block\]", "lds")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    names = " ".join(rows)
    for k in ("k_note_init", "k_note_accum", "k_note_finish", "k_label_points", "k_cartesian_labels"):
        assert k in names, (k, sorted(rows))
    assert len(rows) == 5
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == (7688 if "k_note_accum" in name else 0), (name, u)          # the table DESIGN.md §20 states


def test_notes_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_notes.hip" in src and re.search(r"^resource-usage-notes:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for fn in ("launch_notes", "launch_label_points", "launch_cartesian_labels", "note_scratch_bytes"):
        assert len(re.findall(r"\b%s\(" % fn, launch)) == 1, fn
    assert "7,688" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the restatement against closed forms --------------------------------------------------------------------------------------------
def test_arc_wraps_through_azimuth_zero():
    lab = plane()
    for a in (38, 39, 0, 1, 2):
        lab[3, a] = info(0)
    n, skipped, _ = one(lab)
    assert (n[0]["az_begin"], n[0]["az_count"]) == (38, 5) and skipped == 0
    assert R.arc({38, 39, 0, 1, 2}, A) == (38, 5)
    assert (n[1]["az_begin"], n[1]["az_count"], n[1]["n_extent"]) == (0, 0, 0)          # an object nobody names


def test_two_equal_gaps_go_to_the_run_that_begins_lower():
    # occupied 0 and 20: the runs 1..19 and 21..39 are equally long; the run beginning at 1 is taken, the arc begins behind it
    lab = plane()
    lab[1, 0] = lab[1, 20] = info(0)
    n, _, _ = one(lab)
    assert (n[0]["az_begin"], n[0]["az_count"]) == (20, 21)
    # ... also when the other run passes through azimuth 0: occupied 10 and 30, runs 11..29 and 31..9; 11 < 31
    lab = plane()
    lab[1, 10] = lab[1, 30] = info(0)
    n, _, _ = one(lab)
    assert (n[0]["az_begin"], n[0]["az_count"]) == (30, 21)
    assert R.arc({0, 20}, A) == (20, 21) and R.arc({10, 30}, A) == (30, 21)
    # three equal runs: 0, 13.33 does not divide; use n_angles 39 through arc() alone
    assert R.arc({0, 13, 26}, 39) == (13, 27)


def test_every_azimuth_and_no_azimuth():
    lab = plane()
    lab[5, :] = info(1)
    n, _, _ = one(lab)
    assert (n[1]["az_begin"], n[1]["az_count"]) == (0, A) and (n[0]["az_begin"], n[0]["az_count"]) == (0, 0)
    assert n[0]["bin_min"] == 0xFFFFFFFF and n[0]["bin_max"] == 0 and n[0]["peak"] == n[0]["peak_bin"] == n[0]["peak_az"] == 0
    assert n[0]["x_min"] == np.inf and n[0]["x_max"] == -np.inf and n[0]["y_min"] == np.inf and n[0]["y_max"] == -np.inf
    assert R.arc(set(range(A)), A) == (0, A) and R.arc(set(), A) == (0, 0)


def test_the_fast_arcs_equal_the_walk_on_random_sets():
    rs = np.random.RandomState(3)
    for n_angles in (1, 2, 5, 37, 64):
        sets = [set(rs.choice(n_angles, rs.randint(0, n_angles + 1), replace=False).tolist()) for _ in range(60)] + [set(), set(range(n_angles))]
        ids = np.array([k for k, s in enumerate(sets) for _ in s], np.int64)
        az = np.array([a for s in sets for a in sorted(s)], np.int64)
        begin, count = R.arcs_by_object(ids, az, len(sets), n_angles)
        for k, s in enumerate(sets):
            assert (int(begin[k]), int(count[k])) == R.arc(s, n_angles), (n_angles, sorted(s))


def test_a_peak_tie_goes_to_the_lower_bin_then_the_lower_azimuth():
    lab, img = plane(), np.zeros((N, A), np.uint8)
    for b, a, z in ((7, 3, 200), (4, 9, 200), (4, 6, 200), (2, 1, 199), (9, 0, 10)):
        lab[b, a], img[b, a] = info(0), z
    n, _, _ = one(lab, img)
    assert (n[0]["peak"], n[0]["peak_bin"], n[0]["peak_az"]) == (200, 4, 6)
    assert n[0]["sum_intensity"] == 200 * 3 + 199 + 10 and (n[0]["bin_min"], n[0]["bin_max"]) == (2, 9)
    n, _, _ = one(lab, None)                             # no image: an image of zeros, the tie rule still places the peak
    assert (n[0]["peak"], n[0]["peak_bin"], n[0]["peak_az"], n[0]["sum_intensity"]) == (0, 2, 1, 0)


def test_a_scroll_moves_the_azimuths_not_the_bins():
    lab, img = plane(), np.zeros((N, A), np.uint8)
    lab[6, 2], img[6, 2] = info(0), 50                  # column 2 under scroll 5 holds azimuth 37
    lab[6, 5] = info(0)                                  # column 5 holds azimuth 0
    n, _, r = one(lab, img, scroll=5)
    assert (n[0]["az_begin"], n[0]["az_count"], n[0]["peak_az"], n[0]["peak_bin"]) == (37, 4, 37, 6)
    f32 = np.float32
    rr = f32((6 + 0.5) * 0.5)
    th = [f32(0.0) + f32(a) * f32(GEO["theta_inc"]) for a in (37, 0)]
    assert n[0]["x_max"] == max(rr * np.cos(t) for t in th) == rr and n[0]["x_min"] == min(rr * np.cos(t) for t in th)
    assert n[0]["y_min"] == f32(0.0) and n[0]["y_max"] == rr * np.sin(th[0]) > 0          # theta_inc < 0: azimuth 37 lies to the left
    assert np.all(r[0] == rr)


def test_an_id_beyond_n_objects_is_counted_not_dropped():
    lab = plane()
    lab[1, 1] = info(0)
    lab[2, 2] = info(2)
    lab[3, 3] = info(0xFFFFFE, 3, 1)
    n, skipped, _ = one(lab, n_objects=2)
    assert skipped == 2 and n[0]["n_direct"] == 1 and n[1]["n_direct"] == 0
    n, skipped, _ = one(lab, n_objects=3)
    assert skipped == 1 and n[2]["n_direct"] == 1


def test_the_classes_partition_the_labelled_pixels_and_the_mask_selects_the_extent():
    rs = np.random.RandomState(11)
    lab = plane()
    on = rs.rand(N, A) < 0.6
    lab[on] = (rs.randint(0, 3, on.sum()) | rs.randint(0, 4, on.sum()) << 24 | rs.randint(0, 2, on.sum()) << 28).astype(np.uint32)
    img = rs.randint(0, 256, (N, A)).astype(np.uint8)
    total = {}
    for mask in range(8):
        n, skipped, _ = one(lab, img, n_objects=3, mask=mask)
        assert skipped == 0 and int(n["n_direct"].sum() + n["n_ghost"].sum() + n["n_multipath"].sum()) == int(on.sum())
        want = sum(n[k] for k, bit in (("n_direct", 1), ("n_ghost", 2), ("n_multipath", 4)) if mask & bit)
        assert np.array_equal(n["n_extent"], want if mask else np.zeros(3, np.uint32))
        total[mask] = n["sum_intensity"].copy()
    assert np.array_equal(total[7], total[1] + total[2] + total[4])
    kind, pas = (lab[on] >> 28) & 1, (lab[on] >> 24) & 15
    cls = R.pixel_class(lab[on])
    assert np.array_equal(cls == 4, kind == 1) and np.array_equal(cls == 2, (kind == 0) & (pas > 0)) and np.array_equal(cls == 1, (kind == 0) & (pas == 0))
