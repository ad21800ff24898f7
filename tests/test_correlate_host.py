"""Correlative scan matching without a GPU: the level-from-level pyramid equals a brute-force window minimum; the look-up never exceeds the
true block minimum, at negative and beyond-edge coordinates too; the pruned search of the numpy restatement (tests/correlate_ref.py) equals
the exhaustive one on every case of the shared list, and a bound whose window is one cell too narrow is caught; the room case evaluates
far fewer bounds than it has nodes; offset 0 is rr_score_poses's score of the anchor state; configs are range-checked, the wrappers refuse
bad arguments before any call into the library, the entry points are declared, exported and in the build, the facades have the call, and
k_corr_expand uses neither scratch memory nor LDS."""
import os
import re
import subprocess

import numpy as np
import pytest

import correlate_ref as R
import field_ref as F
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_correlate_scratch_bytes", "rr_correlate_tile_sizes", "rr_field_pyramid_device", "rr_field_pyramid", "rr_correlate_scan_device",
       "rr_correlate_scan"]
CASES = R.all_cases()


def winner(rec):
    return int(rec["sum_d2"]), int(rec["rot"]), int(rec["dx"]), int(rec["dy"])


# ---- the pyramid and its look-up --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (5, 7), (37, 29)])
def test_the_pyramid_is_the_window_minimum(W, H):
    """... at every level up to 2^h beyond the grid's side, on an empty, a sparse and a dense map"""
    rs = np.random.RandomState(100 * W + H)
    for density, md in ((0.0, 5), (0.03, 9), (0.4, 3), (0.03, 255)):
        cfg = F.grid_cfg(W, H, md)
        fld = F.distance_field((rs.random_sample((H, W)) < density).astype(np.uint8), cfg)
        levels = min(R.MAX_LEVELS, int(np.ceil(np.log2(max(W, H)))) + 1)
        assert (1 << levels) > max(W, H) or levels == R.MAX_LEVELS
        got = R.pyramid(fld, cfg, levels)
        assert got.dtype == np.uint16 and got.shape == (levels + 1, H, W) and np.array_equal(got[0], fld)
        for h in range(levels + 1):
            assert np.array_equal(got[h], R.pyramid_brute(fld, cfg, h)), (W, H, density, h)
        assert np.all(got[levels][0, 0] == fld.min())         # the top plane's corner sees the whole grid


def test_the_lookup_is_admissible_everywhere():
    """Q_h(x, y) <= the true minimum of F over the 2^h block from (x, y): inside, at negative coordinates and beyond the far edges"""
    rs = np.random.RandomState(5)
    for W, H in ((5, 7), (37, 29)):
        cfg = F.grid_cfg(W, H, 9)
        fld = F.distance_field((rs.random_sample((H, W)) < 0.05).astype(np.uint8), cfg)
        planes = R.pyramid(fld, cfg, 5)
        for h in range(6):
            span = 1 << h
            y, x = np.mgrid[-span - 2:H + 3, -span - 2:W + 3]
            q, truth = R.lookup(planes[h], cfg, h, x, y), R.block_min(fld, cfg, h, x, y)
            assert np.all(q <= truth), (W, H, h)
            inside = (x >= 0) & (y >= 0) & (x < W) & (y < H)
            assert np.array_equal(q[inside], truth[inside])   # exact where the corner is a cell: only the clamp loosens the bound
            assert np.all(q[(x + span <= 0) | (x >= W)] == 81)


# ---- the search -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["label"] for c in CASES])
def test_the_pruned_search_equals_the_exhaustive_one(k):
    c = CASES[k]
    score, index, r, dx, dy = R.exhaustive_case(c)
    rec = R.search_case(c)
    assert winner(rec) == (score, r, dx, dy), c["label"]
    assert native.corr_node(rec, c["half_x"], c["half_y"]) == index
    assert rec["flags"] == 0 and rec["upper"] >= rec["sum_d2"]
    L = c["levels"]
    n_nodes = len(c["rot"]) * (2 * c["half_x"] + 1) * (2 * c["half_y"] + 1)
    assert np.all(rec["evaluated"][L + 1:] == 0) and np.all(rec["kept"][L + 1:] == 0)
    assert np.all(rec["kept"][:L + 1] >= 1) and np.all(rec["kept"] <= rec["evaluated"])
    assert np.all(rec["evaluated"][:L] <= 4 * rec["kept"][1:L + 1]) and rec["evaluated"][0] <= n_nodes
    if L == 0:
        assert rec["evaluated"][0] == n_nodes and rec["upper"] == score


def test_the_case_list_covers_what_it_says():
    labels = [c["label"] for c in CASES]
    assert len(set(labels)) == len(labels)
    assert {len(c["points"]) for c in CASES} >= {0, 1, 63, 64, 65, 130} and {len(c["rot"]) for c in CASES} >= {1, 3, 9}
    assert any(c["max_points"] < len(c["points"]) for c in CASES)
    assert any(c["half_x"] == 0 for c in CASES) and any(c["half_x"] != c["half_y"] for c in CASES)
    assert any((1 << c["levels"]) > 2 * max(c["half_x"], c["half_y"]) + 1 and c["half_x"] > 0 for c in CASES)
    by = {c["label"]: c for c in CASES}
    A = R.anchored(by["anchor west"]["points"], by["anchor west"]["rot"], by["anchor west"]["cfg"])
    assert A[0].max() < 0 and A[2].all()                                           # negative anchored cells, still usable
    assert not R.anchored(by["anchor far"]["points"], by["anchor far"]["rot"], by["anchor far"]["cfg"])[2].any()
    assert not R.anchored(by["nan state"]["points"], by["nan state"]["rot"], by["nan state"]["cfg"])[2][1].any()
    assert (~R.anchored(by["nan point"]["points"], by["nan point"]["rot"], by["nan point"]["cfg"])[2]).sum(axis=1).tolist() == [3, 3, 3]
    # the ties: every node of the empty map, and two equal minima of the mirror map of which the lower index wins
    c = by["empty map"]
    s = R.all_scores(R.anchored(c["points"], c["rot"], c["cfg"]), c["field"], c["cfg"], c["half_x"], c["half_y"])
    rec = R.search_case(c)
    assert len(np.unique(s)) == 1 and native.corr_node(rec, c["half_x"], c["half_y"]) == 0 and np.array_equal(rec["kept"], rec["evaluated"])
    c = by["mirror"]
    s = R.all_scores(R.anchored(c["points"], c["rot"], c["cfg"]), c["field"], c["cfg"], c["half_x"], c["half_y"]).reshape(-1)
    at = np.nonzero(s == s.min())[0]
    assert len(at) == 2 and native.corr_node(R.search_case(c), c["half_x"], c["half_y"]) == at[0] and R.search_case(c)["kept"][0] == 2


def test_a_bound_one_cell_too_narrow_is_caught():
    """the broken restatement: planes whose window is 2^h - 1 wide.  At least one case must give another winner than the exhaustive search"""
    caught = []
    for c in CASES:
        if c["levels"] == 0:
            continue
        planes = np.stack([R.pyramid_brute(c["field"], c["cfg"], h, shrink=1 if h else 0) for h in range(c["levels"] + 1)])
        score, _, r, dx, dy = R.exhaustive_case(c)
        if winner(R.search_case(c, planes=planes)) != (score, r, dx, dy):
            caught.append(c["label"])
    print("the broken bound is caught by:", caught)
    assert len(caught) >= 1


def test_the_room_case_prunes_almost_everything():
    """the case DESIGN.md §30 quotes: 72 x 52 cells, 9 yaws, +-12 x +-9 cells, 3 levels"""
    c = R.room_case(3)
    assert (c["cfg"].width, c["cfg"].height, len(c["rot"]), c["half_x"], c["half_y"]) == (72, 52, 9, 12, 9)
    n_nodes = 9 * 25 * 19
    assert n_nodes == 4275
    rec = R.search_case(c)
    score, _, r, dx, dy = R.exhaustive_case(c)
    assert winner(rec) == (score, r, dx, dy) == (0, 6, 5, -3)                       # the scan's pose: 5 and -3 cells, the seventh yaw
    print("room case: %d nodes; evaluated per level (3..0) %s, kept %s, U %d" %
          (n_nodes, rec["evaluated"][3::-1].tolist(), rec["kept"][3::-1].tolist(), rec["upper"]))
    assert rec["evaluated"][3] == 9 * 4 * 3 == 108
    assert rec["evaluated"].sum() < n_nodes
    assert rec["evaluated"][3::-1].tolist() == [108, 48, 32, 40] and rec["kept"][3::-1].tolist() == [12, 8, 10, 9]   # what DESIGN.md says


def test_offset_zero_is_the_anchor_states_score():
    """score(r, 0, 0) == field_ref.score's sum_d2 for the anchor state, and the winner's n_in and n_hit are that function's at half 0"""
    for c in CASES:
        A = R.anchored(c["points"], c["rot"], c["cfg"], c["max_points"])
        s = R.all_scores(A, c["field"], c["cfg"], 0, 0)[:, 0, 0]
        want = F.score(c["points"], c["rot"], c["field"], c["cfg"], max_points=c["max_points"])
        assert np.array_equal(s, want["sum_d2"].astype(np.int64)), c["label"]
        rec = R.search(A, R.pyramid(c["field"], c["cfg"], 0), c["cfg"], 0, 0, 0, 1)
        best = want[int(rec["rot"])]
        assert (rec["sum_d2"], rec["n_in"], rec["n_hit"]) == (best["sum_d2"], best["n_in"], best["n_hit"]) and rec["sum_d2"] == want["sum_d2"].min()


def test_overflow_gives_the_greedy_node():
    c = R.wide_case(4)
    full = R.search_case(c)
    cap = int(full["kept"][1:].max())
    assert cap > 1 and R.search_case(c, capacity=cap).tobytes() == full.tobytes()
    over = R.search_case(c, capacity=cap - 1)
    h = int(np.argmax(full["kept"][1:])) + 1
    assert over["flags"] == native.CORR_OVERFLOW and over["sum_d2"] == over["upper"] == full["upper"]
    assert over["kept"][h] == cap and np.all(over["kept"][:h] == 0) and np.all(over["evaluated"][:h] == 0)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def _unopened():
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=64)
    o.n_angles = 16
    return o


def test_corr_config_is_range_checked():
    k = native.corr_config(2047, 0, 8, 1 << 24)
    assert (k.half_x, k.half_y, k.levels, k.capacity, list(k.reserved_)) == (2047, 0, 8, 1 << 24, [0, 0, 0, 0])
    assert C_sizeof(native.RRCorrConfig) == 32 and native.CORR_DTYPE.itemsize == 112 and native.CORR_DTYPE.itemsize % 16 == 0
    good = dict(half_x=12, half_y=9, levels=3, capacity=100)
    for bad in (dict(half_x=-1), dict(half_x=2048), dict(half_y=-1), dict(half_y=2048), dict(levels=-1), dict(levels=9), dict(capacity=0),
                dict(capacity=(1 << 24) + 1), dict(levels=1.5), dict(half_x=True), dict(capacity="many")):
        with pytest.raises(ValueError):
            native.corr_config(**dict(good, **bad))
    with pytest.raises(ValueError):
        native._corr_cfg(native.corr_config(2047, 2047, 4, 10), n_rot=129)         # 129 * 4095 * 4095 >= 2^31: refused
    native._corr_cfg(native.corr_config(2047, 2047, 4, 10), n_rot=128)
    broken = native.corr_config(1, 1)
    broken.reserved_[2] = 1
    with pytest.raises(ValueError):
        native._corr_cfg(broken)
    with pytest.raises(ValueError):
        native._corr_cfg("wide")


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    g = native.field_config(8, 8, 0.5, 0.0, 0.0, 4, 1)
    k = native.corr_config(3, 3, 2, 64)
    pts, rot = F.points_of(np.zeros((3, 2))), np.zeros((2, 4), np.float32)
    fld, pyr = np.zeros((8, 8), np.uint16), np.zeros((3, 8, 8), np.uint16)
    for bad in ((fld.astype(np.uint8), g, 2), (np.zeros((8, 7), np.uint16), g, 2), (fld, g, 9), (fld, g, -1), (fld, g, True), (fld, "grid", 2)):
        with pytest.raises(ValueError):
            o.field_pyramid(*bad)
    for bad in ((None, g, 2, 16), (16, g, 2, None), (16, g, 9, 32), (17, g, 2, 32), (16, g, 2, 33)):
        with pytest.raises(ValueError):
            o.field_pyramid_device(*bad)
    for bad in ((np.zeros((3, 2)), rot, pyr), (pts, rot[:0], pyr), (pts, np.zeros((2, 3), np.float32), pyr), (pts, np.zeros((4097, 4), np.float32), pyr),
                (pts, rot, pyr[:2]), (pts, rot, fld), (pts, rot, pyr.astype(np.int16)), (pts, rot, np.zeros((3, 8, 7), np.uint16))):
        with pytest.raises(ValueError):
            o.correlate_scan(*bad, g, k)
    with pytest.raises(ValueError):
        o.correlate_scan(pts, rot, pyr, g, "wide")
    need = 1 << 20
    ok = (16, 16, 4, 16, 2, 16, g, k, 32, 64, need)
    for at, val in ((0, None), (1, None), (2, -1), (2, 65537), (3, None), (3, 18), (4, 0), (4, 4097), (5, None), (5, 17), (8, None), (8, 24), (9, None),
                    (9, 72), (10, 0), (10, True), (10, 1.5)):
        args = list(ok)
        args[at] = val
        with pytest.raises(ValueError):
            native.Context.correlate_scan_device(_NoLibrary(o), *args)


class _NoLibrary:
    """a context whose scratch size is answered without the library, and whose library must never be reached"""

    def __init__(self, o):
        self._h, self._L = o._h, o._L

    @staticmethod
    def correlate_scratch_bytes(n_rot, max_points, corr_cfg):
        return 4096

    def _ck(self, rc):
        raise AssertionError("the library was reached")


def test_entry_points_are_declared_exported_and_in_the_build(native_lib):
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header and native_lib.lib().rr_abi_version() == 7
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in native_lib.PROTOTYPES and hasattr(native_lib.lib(), n), n
    assert "rr_corr_config" in native.STRUCTS and "rr_corr_rec" in native.STRUCTS and "RR_CORR_OVERFLOW 1u" in header
    points_tile, tops, parents = native_lib.correlate_tile_sizes()
    assert points_tile == 64 and tops >= 1 and parents >= 1
    # the scratch: refused shapes give 0; the size grows with the cells and with the lists, of which there are at most two
    L = native_lib.lib()
    k = native.corr_config(10, 10, 3, 1000)
    size = lambda n_rot, mp, cfg: L.rr_correlate_scratch_bytes(n_rot, mp, cfg)      # noqa: E731
    base = size(4, 100, k)
    assert base >= 256 + 4 * 100 * 4 + 2 * 1000 * 8 and base % 16 == 0
    assert size(0, 100, k) == size(4097, 100, k) == size(4, -1, k) == size(4, 65537, k) == size(4, 100, None) == 0
    assert size(4, 100, native.corr_config(10, 10, 0, 1000)) < size(4, 100, native.corr_config(10, 10, 1, 1000)) < base
    assert size(4, 100, native.corr_config(10, 10, 8, 1000)) == base
    assert size(129, 1, native.corr_config(2047, 2047, 4, 10)) == 0 and size(128, 1, native.corr_config(2047, 2047, 4, 10)) > 0
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "rr_correlate.hip" in re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^resource-usage-correlate:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("correlate_tile_sizes", "correlate_scratch_bytes", "launch_field_pyramid", "launch_correlate"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^(int|void|size_t) %s\(" % n, images, re.M), n
    src = open(os.path.join(CSRC, "rr_correlate.hip")).read()
    for kern in ("k_corr_pyramid", "k_corr_cells", "k_corr_top", "k_corr_descent", "k_corr_expand", "k_corr_finish"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kern, src), kern
    assert "-ffp-contract=off" in mk


def test_the_facades_have_the_call():
    assert callable(radar.RadarHIP.correlateScan)
    doc = radar.RadarHIP.correlateScan.__doc__
    for word in ("sensor frame into the map frame", "levels = 0", "refinePoses"):
        assert word in doc, word
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("correlateScan", "rr_corr_rec", "rr_corr_config", "marshal::correlate_scan"):
        assert n in hpp, n
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    assert "rr_field_pyramid(" in marshal and "rr_correlate_scan(" in marshal
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "correlate_check.cpp")) and os.path.exists(os.path.join(ROOT, "tools", "probe_correlate.py"))
    for doc_file, words in (("INTEGRATION.md", NEW[2:]), ("README.md", ["correlateScan"]), ("DESIGN.md", ["## 30.", "k_corr_expand"]), ("BASELINE.md", ["## 27."])):
        text = open(os.path.join(ROOT, doc_file)).read()
        for word in words:
            assert word.replace("_device", "") in text or word in text, (doc_file, word)


def test_correlate_kernels_use_no_scratch_and_no_lds(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-correlate"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, name in ((r"ScratchSize \[bytes/lane\]", "scratch"), (r"LDS Size \[bytes/block\]", "lds"), (r"VGPRs", "vgprs")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    names = " ".join(rows)
    for k in ("k_corr_pyramid", "k_corr_cells", "k_corr_top", "k_corr_descent", "k_corr_expand", "k_corr_finish"):
        assert k in names, (k, sorted(rows))
    for name, u in rows.items():
        assert u["scratch"] == 0 and u["lds"] == 0, (name, u)
        assert u["vgprs"] <= 64, (name, u)                                             # eight waves per SIMD
