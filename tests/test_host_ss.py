"""The host mirror's share conversions (sfgwas_amd/host/gwas.hpp: mpc::SSToCMatMask / SSToCMatFinish / CMatToSSShares / CMatToSSFinish) driven by a C++ program the
way the Go callers would: two parties in one program, a fixed-point vector shared mod 2^128 - 159 turned into one ciphertext and back into shares, both within the
bound DESIGN.md section 12 derives (the two-party form of tests/test_gpu_rvec.py: the single ternary key and the error-free shares used here stay inside it)."""
import subprocess

import numpy as np
import pytest

import encrypt_ref as er
import oracle_lib as ol
from test_gpu_rvec import derived_bounds
from test_host_mirror import build

pytestmark = pytest.mark.gpu


def test_host_mirror_shares_to_ciphertext_and_back(tmp_path):
    from sfgwas_amd import capi
    capi.lib()
    exe = build("host_ss_test")
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    level, n_elem = 7, 3000
    s, pk = er.make_keypair(ring, 33)
    np.array([len(ol.Q_PN14), len(ol.P_PN14)] + ol.Q_PN14 + ol.P_PN14, dtype=np.uint64).tofile(tmp_path / "moduli.bin")
    pk.tofile(tmp_path / "pk.bin")
    ol.secret_ntt(ring, s).tofile(tmp_path / "sk.bin")
    np.frombuffer(er.TEST_KEY, dtype=np.uint64).tofile(tmp_path / "key.bin")
    (tmp_path / "case.txt").write_text(f"{level} {n_elem}\n")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stderr
    worst_ct, worst_ss = (float(v) for v in out.stdout.split()[1:3])
    bound_ct, bound_ss = derived_bounds(ol.Q_PN14, ol.P_PN14, level, 2.0 ** 34, 30)
    print(f"host mirror: shares -> CKKS {worst_ct:.3e} (bound {bound_ct:.3e}), CKKS -> shares {worst_ss:.3e} (bound {bound_ss:.3e})")
    assert worst_ct <= bound_ct
    assert worst_ss <= bound_ss
