"""The launch plan of the matrix product (sfgwas_amd/csrc/mm_plan.hpp) is pure host arithmetic: tests/host/host_mmplan_test.cpp holds the plan of every
named case against the rows recorded from the statements matmul_accumulate held inline before, checks the invariants of every plan, the group-size
chooser of a caller's int8 tiles and the range plan of a whole product (mm_range_plan) against cases derived by hand.  No GPU, nothing of the library linked; built with AddressSanitizer + UBSan where the compiler has the runtimes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "host_mmplan_test.cpp")
    exe = str(tmp_path / "host_mmplan_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:           # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return exe


def test_mm_plan_cases_invariants_and_group_choosers(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr


def test_mm_plan_header_is_host_only(tmp_path):
    """the planner and the constants header compile as plain C++17 and pull in no HIP header"""
    for hdr in ("mm_plan.hpp", "consts.hpp"):
        path = os.path.join(ROOT, "sfgwas_amd", "csrc", hdr)
        deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", path], capture_output=True, text=True)
        assert deps.returncode == 0, deps.stderr
        assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout        # (the checkout's own path may spell anything)
