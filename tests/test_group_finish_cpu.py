"""The group entry rules the GROUP BY finishers share (queryengine_amd/csrc/qe_group_finish.h) against values written out by
hand: the identity of an empty accumulator, the finish rule, the key and aggregate column images, insertion order and the fold
of the global aggregate's partials.  tests/group_finish_test.cpp is a host program with its own main, built with g++ against
the checkout's header and libqe_hip.so the way tests/test_expr_rules_cpu.py builds its program; no GPU is touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_finish_rules_against_hand_written_values(native_lib, tmp_path):
    from queryengine_amd import native
    csrc = os.path.dirname(native.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "group_finish_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", f"-I{csrc}", os.path.join(ROOT, "tests", "group_finish_test.cpp"), "-o", exe,
                    f"-L{csrc}", "-lqe_hip", f"-Wl,-rpath,{csrc}", f"-Wl,-rpath,{rocm}/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all group finish checks passed" in r.stdout
