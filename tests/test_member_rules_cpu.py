"""The set-membership rules both evaluators share (plan_member, the LIKE matcher, the hash-set builder of
queryengine_amd/csrc/qe_expr_rules.h) against values written out by hand.  tests/member_rules_test.cpp is a host program with
its own main, built and run the way test_expr_rules_cpu.py builds expr_rules_test.cpp; no GPU is touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_membership_rules_against_hand_written_values(native_lib, tmp_path):
    from queryengine_amd import native
    csrc = os.path.dirname(native.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "member_rules_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{csrc}",
                    os.path.join(ROOT, "tests", "member_rules_test.cpp"), "-o", exe, f"-L{csrc}", "-lqe_hip",
                    f"-Wl,-rpath,{csrc}", f"-Wl,-rpath,{rocm}/lib"], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("QE_IN_")}   # the program sets the switches it tests itself
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all membership rule checks passed" in r.stdout
