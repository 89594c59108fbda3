"""CPU test of the host-side meeting point of the multi-GPU engine's rank threads (sfgwas_amd/csrc/rendezvous.hpp): tests/host/rendezvous_test.cpp built with g++ alone.

The bug it pins: when one rank failed at a call's agreement point while a peer was already waiting there, the waiter was released with `false` but its arrival
stayed counted, and the engine's next call released its first rank alone - which then read its peers' buffer pointers of the earlier call (wrong sums, or freed
device memory).  The program's scenario (c) fails against that struct; the engine now calls Rendezvous::reset() before every call's rank threads start."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rendezvous_releases_nobody_early_after_a_one_rank_failure(tmp_path):
    exe = str(tmp_path / "rendezvous_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sfgwas_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "rendezvous_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("OK")
    for n in (2, 3, 8):
        assert f"n = {n} ok" in r.stdout
