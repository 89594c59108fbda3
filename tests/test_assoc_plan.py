"""The association scan's host arithmetic (sfgwas_amd/csrc/assoc_plan.hpp: the batch rule, the plan of a call and of its multi-GPU parts, filter maps,
diag_bool, the active-baby tables, the .pgen descriptor layout) is pure: tests/host/host_assocplan_test.cpp holds it against a literal restatement of the
loops the scan held inline before and asserts the invariants directly.  No GPU, nothing of the library linked; built with AddressSanitizer + UBSan where the
compiler has the runtimes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "host_assocplan_test.cpp")
    exe = str(tmp_path / "host_assocplan_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:           # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return exe


def test_assoc_plan_batches_parts_maps_and_layouts(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr


def test_assoc_plan_header_is_host_only(tmp_path):
    """the header compiles as plain C++17 and pulls in no HIP header"""
    path = os.path.join(ROOT, "sfgwas_amd", "csrc", "assoc_plan.hpp")
    deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", path], capture_output=True, text=True)
    assert deps.returncode == 0, deps.stderr
    assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout        # (the checkout's own path may spell anything)
