"""The scan primitives (queryengine_amd/csrc/qe_scan.h: launch_carry_scan, exclusive_scan, bitmap_ranks + bitmap_positions)
called directly by a stand-alone HIP program (tests/scan) and compared exactly with host loops: every trip, block and
threshold seam of the three shapes, at a few megabytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "tests", "scan")


@pytest.mark.gpu
def test_scan_primitives_match_host_loops(native_lib):
    exe = os.path.join(SCAN, "test_scan")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", SCAN], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scan primitives: all" in r.stdout and "checks passed" in r.stdout


def test_scan_primitives_program_builds(native_lib):
    subprocess.run(["make", "-C", SCAN], check=True)
    assert os.path.exists(os.path.join(SCAN, "test_scan"))
