"""integration/: the ROS-typed RadarHIP backend + the line-anchored insertions that add it to a checkout of the reference.

ROS 1 / cv_bridge / rmagine are not in this image, so nothing here is COMPILED; what can be checked is: the patches apply
to the reference checkout they were made for (and to nothing else), the patched node declares what it uses and follows
the reference's own selection logic, every C-ABI call of the adapter matches the header's name and arity, and every
member / config field the adapter reads exists in the reference.  Needs /root/reference: skipped on the GPU box.
"""
import hashlib
import json
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "integration"))
import apply as integ  # noqa: E402

needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not on this machine")
# the marshalling the adapter shares with its ROS-free twin: the adapter includes it, so its text counts as the adapter's
MARSHAL = "../include/radarays_ros_amd/marshal.hpp"


def strip_cpp(text):
    """comments and string literals blanked (same length), for brace / token checks"""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i)); i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i) + 2
            out.append(re.sub(r"[^\n]", " ", text[i:j])); i = j
        elif c == '"' or c == "'":
            j = i + 1
            while text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + " " * (j - i - 1) + c); i = j + 1
        else:
            out.append(c); i += 1
    return "".join(out)


def header_prototypes():
    """name -> number of parameters, from include/radarays_mi355.h"""
    text = strip_cpp(open(os.path.join(ROOT, "include", "radarays_mi355.h")).read())
    protos = {}
    for m in re.finditer(r"\b(rr_\w+)\s*\(([^;{}]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else len(split_args(args))
    return protos


def split_args(s):
    depth, cur, out = 0, "", []
    for c in s:
        if c in "([{<" and not (c == "<" and " " in cur[-1:]):
            depth += c != "<"
        elif c in ")]}":
            depth -= 1
        if c == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += c
    out.append(cur)
    return out


def calls_of(text):
    """(name, n_args) for every rr_*(...) call in C++ source"""
    text = strip_cpp(text)
    found = []
    for m in re.finditer(r"\b(rr_\w+)\s*\(", text):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        inner = text[m.end():i - 1].strip()
        found.append((m.group(1), 0 if not inner else len(split_args(inner))))
    return found


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    dst = tmp_path_factory.mktemp("ref") / "radarays_ros"
    shutil.copytree(REF, dst, ignore=shutil.ignore_patterns(".git", "dat"))
    for r, _, fs in os.walk(dst):
        os.chmod(r, 0o755)
        for f in fs:
            os.chmod(os.path.join(r, f), 0o644)
    integ.apply(str(dst))
    return str(dst)


def test_patches_are_pure_insertions_and_hold_no_reference_text():
    for patch in integ.load_patches():
        assert set(patch) == {"file", "sha256", "n_lines", "about", "insertions"}
        assert len(patch["sha256"]) == 64
        for ins in patch["insertions"]:
            assert set(ins) == {"after_line", "why", "text"}          # nothing like "delete" / "context"
    if os.path.isdir(REF):                                            # and no inserted multi-line run is a run of the reference
        for patch in integ.load_patches():
            ref_lines = {l.strip() for l in open(os.path.join(REF, patch["file"])).read().split("\n") if len(l.strip()) > 12}
            for ins in patch["insertions"]:
                own = [l.strip() for l in ins["text"] if len(l.strip()) > 12]
                same = [l for l in own if l in ref_lines]
                # the pattern lines a CMake target shares with its sibling (add_dependencies' three variables, install's three
                # destinations) are what "following the pattern of radarays_gpu" means; anything beyond them would be a copy
                assert len(same) <= 6 and len(same) <= len(own) / 2, (patch["file"], ins["after_line"], same)


@needs_ref
def test_patch_refuses_any_other_file(tmp_path):
    for patch in integ.load_patches():
        text = open(os.path.join(REF, patch["file"]), newline="").read()
        assert hashlib.sha256(text.encode()).hexdigest() == patch["sha256"]
        assert len(text.split("\n")) in (patch["n_lines"], patch["n_lines"] + 1)
        with pytest.raises(ValueError):
            integ.patched_text(text + " ", patch)
        once = integ.patched_text(text, patch)
        with pytest.raises(ValueError):                               # not applied twice
            integ.patched_text(once, patch)
        # a pure insertion: deleting the inserted lines gives the file back
        kept = once.split("\n")
        for ins in sorted(patch["insertions"], key=lambda i: -i["after_line"]):
            shift = sum(len(j["text"]) for j in patch["insertions"] if j["after_line"] < ins["after_line"])
            a = ins["after_line"] + shift
            assert kept[a:a + len(ins["text"])] == ins["text"]
            del kept[a:a + len(ins["text"])]
        assert "\n".join(kept) == text


@needs_ref
def test_patched_node_follows_the_reference_selection_logic(tree):
    raw = open(os.path.join(tree, "src", "radar_simulator.cpp")).read()
    src = strip_cpp(raw)
    # balanced
    assert src.count("{") == src.count("}") and src.count("(") == src.count(")")
    assert len(re.findall(r"^\s*#\s*if", src, re.M)) == len(re.findall(r"^\s*#\s*endif", src, re.M))
    # declared before use, once, as the reference declares use_gpu / gpu_available (radar_simulator.cpp:118-123)
    for name in ("use_hip", "hip_available", "hip_devices", "hip_build_on_gpu"):
        uses = [m.start() for m in re.finditer(r"\b%s\b" % name, src)]
        decls = [m.start(1) for m in re.finditer(r"\b(?:bool|std::vector<int>)\s+(%s)\b" % name, src)]
        assert len(decls) == 1 and decls[0] == uses[0] and len(uses) >= 2, name
    assert not re.search(r"\bbackend\b", src)                          # round 4's snippet used an undeclared `backend`
    # the parameter is read like ~gpu is
    assert re.search(r'nh_p->param<bool>\(\s*"\s*\S*\s*"\s*,\s*use_hip\s*,\s*false\s*\)', src) and '"hip"' in raw
    # availability guards extended: HIP asked for but not built in -> message + return 0, like :133-143
    m = re.search(r"if\(use_hip && !hip_available\)\s*\{[^}]*return 0;\s*\}", src)
    assert m and "not available on your system" in raw[m.start():m.end()]
    # ... and neither of the reference's two guards can stop a HIP-only machine
    assert re.search(r"if\(use_hip\)\s*\{\s*use_gpu = false;\s*\}", src)
    assert re.search(r"if\(!use_hip\)\s*if\(!use_gpu && !cpu_available\)", src)
    # the arm: under its own definition, the reference's if / else chain as its else branch, same five leading arguments
    arm = re.search(r"if\(use_hip\)\s*\{\s*#if defined RADARAYS_WITH_HIP(.*?)#endif\s*\}\s*else\s*if\(!use_gpu\)", src, re.S)
    assert arm
    ctor = re.search(r"std::make_shared<RadarHIP>\(([^;]*)\);", arm.group(1), re.S)
    args = [a.strip() for a in ctor.group(1).split(",")]
    assert args[:5] == ["nh_p", "tf_buffer", "tf_listener", "map_frame", "sensor_frame"] and args[5] == "map_file"
    cpu = re.search(r"std::make_shared<RadarCPU>\(([^;]*)\);", src, re.S)
    assert [a.strip() for a in cpu.group(1).split(",")][:5] == args[:5]
    assert re.search(r"#if defined RADARAYS_WITH_HIP\s*#include <radarays_ros/RadarHIP.hpp>\s*#endif", src)
    # the constructor the node calls exists with that many parameters
    hpp = strip_cpp(open(os.path.join(tree, "include", "radarays_ros", "RadarHIP.hpp")).read())
    ctors = [split_args(m.group(1)) for m in re.finditer(r"\n\s*RadarHIP\(\s*\n(.*?)\n\s*\);", hpp, re.S)]
    assert any(len(c) == 8 and "map_file" in c[5] and "=" in c[6] and "=" in c[7] for c in ctors)


@needs_ref
def test_patched_cmake_follows_the_optional_backend_pattern(tree):
    text = open(os.path.join(tree, "CMakeLists.txt")).read()
    assert len(re.findall(r"^\s*if\(", text, re.M)) == len(re.findall(r"^\s*endif\(", text, re.M))
    assert text.count("(") == text.count(")")
    at = {k: text.index(k) for k in ("list(APPEND RADARAYS_ROS_LIBRARIES radarays_hip)", "catkin_package(",
                                     "add_library(radarays_hip", "add_library(radarays_gpu", "add_executable(radar_simulator",
                                     "target_compile_definitions(radar_simulator PUBLIC RADARAYS_WITH_HIP)")}
    assert at["list(APPEND RADARAYS_ROS_LIBRARIES radarays_hip)"] < at["catkin_package("]      # exported like radarays_gpu
    assert at["add_library(radarays_gpu"] < at["add_library(radarays_hip"] < at["add_executable(radar_simulator"]
    assert at["add_executable(radar_simulator"] < at["target_compile_definitions(radar_simulator PUBLIC RADARAYS_WITH_HIP)"]
    lib = text[at["add_library(radarays_hip"]:at["add_executable(radar_simulator"]]
    assert "src/radarays_ros/RadarHIP.cpp" in lib and "${RADARAYS_MI355_LIBRARY}" in lib and "${RADARAYS_MI355_INCLUDE_DIR}" in lib
    assert os.path.isfile(os.path.join(tree, "src", "radarays_ros", "RadarHIP.cpp"))
    # find_library finds the library where this repository builds it, find_path the header
    assert os.path.isfile(os.path.join(ROOT, "include", "radarays_mi355.h"))
    assert "PATH_SUFFIXES radarays_ros_amd" in text and os.path.isdir(os.path.join(ROOT, "radarays_ros_amd"))


def test_every_abi_call_of_the_adapter_matches_the_header():
    protos = header_prototypes()
    assert len(protos) >= 60
    seen = set()
    adapter = integ.NEW_FILES + [MARSHAL]
    for rel in adapter + ["../include/radarays_ros_amd/RadarHIP.hpp", "../tests/cpp/radar_hip_demo.cpp"]:
        for name, n in calls_of(open(os.path.join(ROOT, "integration", rel)).read()):
            assert name in protos, "%s: %s is not in radarays_mi355.h" % (rel, name)
            assert protos[name] == n, "%s: %s called with %d arguments, declared with %d" % (rel, name, n, protos[name])
            if rel in adapter:
                seen.add(name)
    # the ROS-typed adapter, with the marshalling header it includes, drives the multi-device object, the batch and the
    # parameter-set entry points
    assert {"rr_create_multi", "rr_multi_set_mesh", "rr_multi_set_mesh_gpu", "rr_multi_set_config", "rr_multi_set_materials",
            "rr_multi_set_beam_samples", "rr_multi_set_noise_offsets", "rr_multi_set_motion_poses", "rr_multi_simulate",
            "rr_multi_simulate_batch", "rr_simulate_param_sets", "rr_sample_cone_local", "rr_load_mesh_file", "rr_free_mesh",
            "rr_destroy_multi", "rr_abi_version"} <= seen


@needs_ref
def test_adapter_reads_only_what_the_reference_declares(tree):
    cpp = strip_cpp(open(os.path.join(tree, "src", "radarays_ros", "RadarHIP.cpp")).read())
    hpp = strip_cpp(open(os.path.join(tree, "include", "radarays_ros", "RadarHIP.hpp")).read())
    # dynamic-reconfigure fields: gen.add("<name>", ...) of cfg/RadarModel.cfg
    cfg_fields = set(re.findall(r'gen\.add\(\s*"(\w+)"', open(os.path.join(REF, "cfg", "RadarModel.cfg")).read()))
    # read by the adapter itself, or by fill_config of the marshalling header, which the adapter instantiates with m_cfg
    shared = strip_cpp(open(os.path.join(ROOT, "integration", MARSHAL)).read())
    fill = shared[shared.index("void fill_config("):]
    fill = fill[:fill.index("\n}")]
    assert re.search(r"marshal::fill_config\(\s*c\s*,\s*m_cfg\s*,", cpp)
    used = set(re.findall(r"\bm_cfg\.(\w+)", cpp)) | set(re.findall(r"\bcfg\.(\w+)", fill))
    assert len(used) >= 24 and used <= cfg_fields, used - cfg_fields
    # every field RadarCPU::simulate reads from m_cfg is marshalled (beam_width / n_samples / n_reflections travel via
    # m_params.model, Radar.cpp:213-215; n_cells.. via rr_config)
    cpu_reads = set(re.findall(r"\bm_cfg\.(\w+)", strip_cpp(open(os.path.join(REF, "src/radarays_ros/RadarCPU.cpp")).read())))
    assert cpu_reads <= used, cpu_reads - used
    # message fields
    def msg_fields(name):
        return {l.split()[1] for l in open(os.path.join(REF, "msg", name)).read().splitlines() if len(l.split()) >= 2}
    assert set(re.findall(r"\.model\.(\w+)", cpp + shared)) <= msg_fields("RadarModel.msg")
    assert {"velocity", "ambient", "diffuse", "specular"} == msg_fields("RadarMaterial.msg")
    assert msg_fields("RadarParams.msg") == {"materials", "model"} and msg_fields("RadarMaterials.msg") == {"data"}
    # protected members of Radar (Radar.hpp:66-105) and its methods
    radar_hpp = strip_cpp(open(os.path.join(REF, "include/radarays_ros/Radar.hpp")).read())
    own = set(re.findall(r"\b(m_\w+)\b\s*(?:=[^;]*)?;", hpp))
    for member in set(re.findall(r"\b(m_\w+|Tsm_last)\b", cpp)) - own:
        assert re.search(r"\b%s\b" % member, radar_hpp), member
    for method in ("updateTsm()", "updateTsm(ros::Time stamp)"):
        assert method in radar_hpp
    # motion mode follows RadarCPU.cpp:127 (`if(!m_cfg.include_motion)` around the single lookup): round 4's snippet
    # looked the pose up once more than the reference does
    sim = cpp[cpp.index("RadarHIP::simulate(ros::Time stamp)"):cpp.index("RadarHIP::simulateBatch")]
    assert re.search(r"if\(!m_cfg\.include_motion\)\s*\{\s*if\(!updateTsm\(\)\)", sim)
    assert len(re.findall(r"updateTsm\(", sim)) == 1                   # the per-azimuth lookups live in lookupSweep
    sweep = cpp[cpp.index("RadarHIP::lookupSweep"):cpp.index("RadarHIP::simulate(ros::Time stamp)")]
    assert "ros::spinOnce()" in sweep and "skipped[angle_id] = 1" in sweep
    # DirectedWave members used exist (radar_types.h:63-121)
    types = open(os.path.join(REF, "include/radarays_ros/radar_types.h")).read()
    for f in set(re.findall(r"\bwave\.(\w+)", cpp)):
        assert re.search(r"\b%s\b" % f, types), f
    # the output contract of RadarCPU.cpp:555-561
    assert '"mono8"' in open(os.path.join(tree, "src", "radarays_ros", "RadarHIP.cpp")).read()
    assert "header.stamp = stamp" in cpp and "header.frame_id = m_sensor_frame" in cpp


from oracle.refgen import generated_headers as _generated_headers  # noqa: E402


@needs_ref
def test_adapter_type_checks_against_the_reference_headers(tree, tmp_path):
    """g++ -fsyntax-only on the ROS-typed adapter: the reference's own Radar.hpp / radar_types.h, the headers catkin would
    generate derived from the reference's IDL at test time, and signature-only stand-ins for ROS / cv_bridge / rmagine
    (tests/cpp/ros_stubs/README.md: type-check scaffolding, not a build of the reference, pins nothing).  Also checked:
    the scaffolding is not vacuous -- a misspelt config field or a wrong rr_* arity fails to compile.  The config copy and
    the materials live in the marshalling header as templates: a misspelt field there fails only because the adapter
    instantiates them with the reference's generated types."""
    import subprocess
    gen_dir = str(tmp_path / "gen")
    _generated_headers(gen_dir)
    inc = os.path.join(ROOT, "include")
    bad_inc = tmp_path / "bad_include"          # first on the include path: a mutated copy of the header shadows the tree's
    (bad_inc / "radarays_ros_amd").mkdir(parents=True)
    shutil.copy(os.path.join(inc, "radarays_mi355.h"), bad_inc)          # what the header includes as "../radarays_mi355.h"
    base = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-I", str(bad_inc),
            "-I", os.path.join(ROOT, "tests", "cpp", "ros_stubs"), "-I", gen_dir, "-I", os.path.join(tree, "include"), "-I", inc]
    src = os.path.join(tree, "src", "radarays_ros", "RadarHIP.cpp")
    shared = bad_inc / "radarays_ros_amd" / "marshal.hpp"
    r = subprocess.run(base + [src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    text = {src: open(src).read(), shared: open(os.path.join(inc, "radarays_ros_amd", "marshal.hpp")).read()}
    p = tmp_path / "bad.cpp"
    for where, old, new, named, why in (
            (shared, "cfg.signal_max", "cfg.signal_maximum", "signal_maximum", "a config field that does not exist"),
            (p, "rr_multi_set_config(m_multi, &c)", "rr_multi_set_config(m_multi, &c, 1)", "rr_multi_set_config", "an rr_* call with one argument too many"),
            (shared, "m.velocity", "m.speed", "speed", "a message field that does not exist")):
        good = text[src if where == p else shared]
        bad = good.replace(old, new, 1)
        assert bad != good
        p.write_text(text[src])
        where.write_text(bad)
        rb = subprocess.run(base + [str(p)], capture_output=True, text=True)
        if where == shared:
            shared.unlink()
        assert rb.returncode != 0 and named in rb.stderr, (why, rb.stderr[-2000:])     # refused, and for that reason
