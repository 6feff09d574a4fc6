"""The plan-time rules both expression evaluators share (queryengine_amd/csrc/qe_expr_rules.h) against values written out
by hand: conjunct splitting, the column-use pass and its errors, the string comparison plan, dictionary unions and the
integer-literal test.  tests/expr_rules_test.cpp is a host program with its own main, built with g++ against the
checkout's qe_internal.h and libqe_hip.so the way tools/dump_generated_sources.py builds its driver; no GPU is touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expression_rules_against_hand_written_values(native_lib, tmp_path):
    from queryengine_amd import native
    csrc = os.path.dirname(native.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "expr_rules_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{csrc}",
                    os.path.join(ROOT, "tests", "expr_rules_test.cpp"), "-o", exe, f"-L{csrc}", "-lqe_hip",
                    f"-Wl,-rpath,{csrc}", f"-Wl,-rpath,{rocm}/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all expression rule checks passed" in r.stdout
