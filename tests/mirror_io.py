"""What tests/test_gpu_cpp_mirror.py and tests/test_cpp_mirror_host.py share: building tests/cpp/mirror_check.cpp, and the file format it
reads and writes -- sections of {char tag[16], uint64 byte count, bytes}, found by tag."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mirror_check.cpp")

# the order of the driver's "cfg" section (config_of in mirror_check.cpp)
CFG_FIELDS = ("n_cells", "n_samples", "n_reflections", "beam_width", "resolution", "energy_max", "signal_max", "signal_denoising",
              "signal_denoising_triangular_width", "signal_denoising_triangular_mode", "signal_denoising_gaussian_width",
              "signal_denoising_gaussian_mode", "signal_denoising_mb_width", "signal_denoising_mb_mode", "ambient_noise",
              "ambient_noise_at_signal_0", "ambient_noise_at_signal_1", "ambient_noise_energy_max", "ambient_noise_energy_min",
              "ambient_noise_energy_loss", "scroll_image", "multipath_threshold", "record_multi_reflection", "record_multi_path",
              "beam_sample_dist", "beam_sample_dist_normal_p_in_cone")


def build_driver(out_dir, native_lib):
    """mirror_check as the other drivers under tests/cpp are built, with the warnings on"""
    native_lib.build()
    exe = os.path.join(str(out_dir), "mirror_check")
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", lib_dir, "-lradarays_mi355", "-Wl,-rpath," + lib_dir], check=True)
    return exe


def write_sections(path, sections):
    """sections: (tag, bytes or array) pairs, in order"""
    with open(path, "wb") as f:
        for tag, data in sections:
            b = data if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).tobytes()
            t = tag.encode()
            assert len(t) <= 15, tag
            f.write(t.ljust(16, b"\0") + struct.pack("<Q", len(b)) + b)


def read_sections(path):
    """tag -> bytes.  A header or a body that runs past the end of the file, a tag that comes twice and a file without the driver's
    closing "done" section all raise: a short result cannot pass for another one."""
    raw = open(path, "rb").read()
    out, at = {}, 0
    while at < len(raw):
        if at + 24 > len(raw):
            raise ValueError("a section header runs past the end of the file at byte %d" % at)
        tag = raw[at:at + 16].rstrip(b"\0").decode()
        n = struct.unpack("<Q", raw[at + 16:at + 24])[0]
        at += 24
        if at + n > len(raw):
            raise ValueError("section %r says %d bytes, the file holds %d more" % (tag, n, len(raw) - at))
        if tag in out:
            raise ValueError("section %r comes twice" % tag)
        out[tag] = raw[at:at + n]
        at += n
    if "done" not in out or list(out)[-1] != "done":
        raise ValueError("the driver did not write its closing section: %s" % list(out))
    return out


class Results:
    """the sections of one driver run; arr() refuses a section whose length is not what the caller's shape says"""

    def __init__(self, sections):
        self.sections = sections

    def raw(self, tag):
        return self.sections[tag]                    # KeyError: the section is missing

    def arr(self, tag, dtype, shape=(-1,)):
        b = self.sections[tag]
        dt = np.dtype(dtype)
        if len(b) % dt.itemsize:
            raise ValueError("section %r: %d bytes are no whole number of %s" % (tag, len(b), dt))
        a = np.frombuffer(b, dt)
        if -1 not in shape and a.size != int(np.prod(shape)):
            raise ValueError("section %r holds %d elements, expected shape %s" % (tag, a.size, shape))
        return a.reshape(shape)

    def text(self, tag):
        return self.sections[tag].decode()


def scene_sections(group, scene, mats, cfg, beams, pose):
    """the sections every GPU run of the driver starts from"""
    return [("group", group.encode()),
            ("verts", np.asarray(scene["verts"], np.float32)), ("faces", np.asarray(scene["faces"], np.uint32)),
            ("fobj", np.asarray(scene["face_object_id"], np.uint32)),
            ("mats", np.asarray([m.astuple() for m in mats], np.float32)), ("objmat", np.asarray(scene["object_materials"], np.int32)),
            ("cfg", np.asarray([float(getattr(cfg, k)) for k in CFG_FIELDS], np.float64)),
            ("beams", np.asarray(beams, np.float32)), ("pose", np.asarray(pose, np.float32))]


def run_driver(exe, args, timeout):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def parse_chains(a, with_az):
    """the driver's "chains" section -> {(az, k) or k: [indices]}"""
    out, at, head = {}, 0, 3 if with_az else 2
    a = [int(v) for v in a]
    while at < len(a):
        if at + head > len(a) or at + head + a[at + head - 1] > len(a):
            raise ValueError("the chains section ends inside a record")
        key = (a[at], a[at + 1]) if with_az else a[at]
        if key in out:
            raise ValueError("chain %r comes twice" % (key,))
        n = a[at + head - 1]
        out[key] = a[at + head:at + head + n]
        at += head + n
    return out
