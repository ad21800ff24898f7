"""The staged round trip of the host forms (csrc/rr_stage.h), the part that needs no GPU: the count-truncated row scatter (csrc/rr_rows.h)
that writes a held row output into the caller's buffer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_scatter_under_asan(tmp_path):
    """scatter_rows under AddressSanitizer + UBSan (a stand-alone program, CPU only): counts of 0, below, equal to and above the device
    stride, a caller stride larger than the device stride, one row and many -- every caller byte outside the first min(count, d_stride)
    records of a row keeps its guard pattern, and nothing is read or written past either buffer."""
    if shutil.which("g++") is None:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "rows_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "radarays_ros_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "rows_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    assert "rows_check: ok" in r.stdout
