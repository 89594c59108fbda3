"""The multi-GPU engine's host arithmetic (sfgwas_amd/csrc/mg_plan.hpp: the SNP-block shard, the sizes and the exchange schedule of one rank's Q' * X^T in its
three forms, the host-form offsets, the re-shard segment table) is pure: tests/host/host_mgplan_test.cpp holds it against a literal restatement of the
expressions and loops mgpu.hip held inline before and asserts the invariants directly.  No GPU, nothing of the library linked; built with AddressSanitizer +
UBSan where the compiler has the runtimes.  The pipelined form over fp64 rotation rows (one column per step) is held here only: on the committed chains the
engine takes the tile form whenever it pipelines."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "host_mgplan_test.cpp")
    exe = str(tmp_path / "host_mgplan_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe, src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:           # no sanitizer runtimes: the plain build must still succeed
        subprocess.check_call(base)
    return exe


def test_mg_plan_shards_contraction_plans_offsets_and_reshard_segments(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-4000:] + out.stderr[-4000:]


def test_mg_plan_header_is_host_only(tmp_path):
    """the header compiles as plain C++17 and pulls in no HIP header"""
    path = os.path.join(ROOT, "sfgwas_amd", "csrc", "mg_plan.hpp")
    deps = subprocess.run(["g++", "-std=c++17", "-x", "c++", "-M", path], capture_output=True, text=True)
    assert deps.returncode == 0, deps.stderr
    assert "hip" not in deps.stdout.replace(ROOT, "").lower(), deps.stdout        # (the checkout's own path may spell anything)
