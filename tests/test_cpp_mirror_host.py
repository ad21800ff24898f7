"""tests/cpp/mirror_check.cpp without a GPU: it compiles with the warnings on, says so loudly when there is no device, and its --host mode
holds the static RadarHIP::pathToEcho (include/radarays_ros_amd/RadarHIP.hpp) to chains written out by hand and to the Python twin
radar.path_to_echo on hand-made wave lists (on the GPU, tests/test_gpu_cpp_mirror.py holds it to the echo log of tests/paths_ref.py)."""
import numpy as np
import pytest

import mirror_io as M
from common import golden_beams
from radarays_ros_amd import params, radar, scenes
from test_paths_host import hand_made


@pytest.fixture(scope="module")
def exe(tmp_path_factory, native_lib):
    return M.build_driver(tmp_path_factory.mktemp("mirror_host"), native_lib)


def host_chains(exe, tmp_path, waves, n, ks):
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    M.write_sections(inp, [("waves", waves), ("n", np.uint64([n])), ("ks", np.int32(ks))])
    r = M.run_driver(exe, ["--host", inp, out], timeout=60)
    assert r.returncode == 0, r.stderr
    res = M.Results(M.read_sections(out))
    assert res.text("done") == "host"
    got = M.parse_chains(res.arr("chains", np.int32), with_az=False)
    assert sorted(got) == sorted(ks)
    return got


def info(obj, p, br, e0, e1):
    return obj | p << 24 | br << 28 | e0 << 30 | e1 << 31


def test_driver_fails_loudly_without_gpu(exe, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    s = scenes.box12()
    cfg = params.kaist_preset(n_cells=200, n_reflections=2, ambient_noise=0)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    M.write_sections(inp, M.scene_sections("sim", s, params.kaist_materials(), cfg, golden_beams(50), scenes.default_pose("box12")))
    r = M.run_driver(exe, [inp, out], timeout=120)
    assert r.returncode == 6 and "no HIP device" in r.stderr and "no CPU fallback" in r.stderr
    with pytest.raises(ValueError):
        M.read_sections(out)                       # no closing section: nothing of it passes for a result


def test_driver_refuses_a_short_input(exe, tmp_path):
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    M.write_sections(inp, [("group", b"sim")])
    raw = open(inp, "rb").read()
    open(inp, "wb").write(raw[:-1])
    r = M.run_driver(exe, [inp, out], timeout=60)
    assert r.returncode == 2 and "short" in r.stderr
    M.write_sections(inp, [("waves", np.zeros(1, np.uint8)), ("n", np.uint64([1])), ("ks", np.int32([0]))])
    r = M.run_driver(exe, ["--host", inp, out], timeout=60)
    assert r.returncode == 2 and "ragged" in r.stderr


def test_section_reader_refuses_short_files(tmp_path):
    p = tmp_path / "s.bin"
    M.write_sections(p, [("a", np.arange(4, dtype=np.int32)), ("b", b"xy"), ("done", b"t")])
    res = M.Results(M.read_sections(p))
    assert res.arr("a", np.int32, (2, 2)).tolist() == [[0, 1], [2, 3]] and res.text("b") == "xy"
    with pytest.raises(ValueError):
        res.arr("a", np.int32, (5,))               # a short section does not reshape into the expected result
    with pytest.raises(ValueError):
        res.arr("b", np.int32)
    with pytest.raises(KeyError):
        res.raw("c")
    raw = open(p, "rb").read()
    for cut in (1, 2, 24, 30):                      # inside the last body, inside a header, inside an earlier body
        open(p, "wb").write(raw[:-cut])
        with pytest.raises(ValueError):
            M.read_sections(p)
    M.write_sections(p, [("a", b"1"), ("a", b"2"), ("done", b"")])
    with pytest.raises(ValueError):
        M.read_sections(p)
    M.write_sections(p, [("done", b""), ("a", b"1")])
    with pytest.raises(ValueError):
        M.read_sections(p)


def twin_chain(w, k):
    """radar.path_to_echo, an empty chain where it raises (no owner: IndexError from path_to_echo; a parent beyond the list: IndexError
    from path_to_wave; a chain past the pass limit: ValueError)"""
    try:
        return radar.path_to_echo(w, k)[0].tolist()
    except (IndexError, ValueError):
        return []


def test_path_to_echo_on_the_hand_made_list(exe, tmp_path, native_lib):
    """a wave that owns two echoes (info bits 30 and 31), echoes nobody owns, and a list cut before a parent"""
    w = hand_made(native_lib)                       # wave 2 (child of beam 0) owns echoes 1 and 2; beam 0 owns echo 0; nobody owns 3
    ks = [0, 1, 2, 3, 7, -1]
    got = host_chains(exe, tmp_path, w, len(w), ks)
    assert got == {0: [0], 1: [0, 2], 2: [0, 2], 3: [], 7: [], -1: []}
    for k in ks:
        assert got[k] == twin_chain(w, k), k
    for k in (3, 7):
        with pytest.raises(IndexError):
            radar.path_to_echo(w, k)
    # the list cut to its first two records: echo 0 is still owned by wave 0; the owner of echoes 1 and 2 is gone
    assert host_chains(exe, tmp_path, w, 2, [0, 1, 2]) == {0: [0], 1: [], 2: []}
    assert [twin_chain(w[:2], k) for k in (0, 1, 2)] == [[0], [], []]
    # a parent index beyond n: wave 2 re-parented to a record the list does not hold
    far = w.copy()
    far["parent"][2] = 9
    assert host_chains(exe, tmp_path, far, len(far), [0, 1, 2]) == {0: [0], 1: [], 2: []}
    assert [twin_chain(far, k) for k in (0, 1, 2)] == [[0], [], []]


@pytest.mark.parametrize("length,empty", [(15, False), (16, False), (17, True), (20, True)])
def test_path_to_echo_chain_length(exe, tmp_path, native_lib, length, empty):
    """a chain of `length` waves, one per pass, the last one owning echo 5: RR_WAVES_MAX_PASSES (16) waves are a chain, more are not a
    wave list and give an empty one"""
    assert native_lib.WAVES_MAX_PASSES == 16
    w = np.zeros(length + 1, native_lib.WAVE_DTYPE)
    w["echo"] = -1
    w["parent"][:length] = np.arange(length) - 1
    w["info"][:length] = [info(1, p % 16, 0 if p == 0 else 1, 0, 0) for p in range(length)]
    w["echo"][length - 1] = 5
    w["info"][length - 1] |= np.uint32(1 << 30)
    w["parent"][length] = -1                       # a beam beside the chain, owning nothing
    got = host_chains(exe, tmp_path, w, len(w), [5, 4, 6])
    assert got[4] == [] and got[6] == []
    assert got[5] == ([] if empty else list(range(length)))
    # The Python twin (radar.path_to_wave, not touched here) draws the line one wave later: it still answers a chain of 17 waves and
    # raises from 18 on.  The C++ side refuses 17 already, as its comment and RR_WAVES_MAX_PASSES say; the two agree up to 16.
    if length <= 17:
        assert radar.path_to_echo(w, 5)[0].tolist() == list(range(length))
    else:
        with pytest.raises(ValueError):
            radar.path_to_echo(w, 5)
