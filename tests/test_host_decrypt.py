"""The host mirror's way back out (sfgwas_amd/host/gwas.hpp: DecodeFloatVector, DecryptFloatVectorDev, DecryptFloatMatrixDev) driven by a C++ program the way the
Go callers would: DecodeFloatVector(EncodeFloatVector(v)) within the encoder's rounding, DecryptFloatMatrix(EncryptFloatMatrixRow(v)) within the derived noise."""
import subprocess

import numpy as np
import pytest

import encrypt_ref as er
import oracle_lib as ol
from test_host_mirror import build

pytestmark = pytest.mark.gpu


def test_host_mirror_decode_and_decrypt_round_trips(tmp_path):
    from sfgwas_amd import capi
    capi.lib()
    exe = build("host_decrypt_test")
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    N, vrows, vlen, level, scale = ring.N, 2, ring.slots + 100, 3, 2.0 ** 34
    s, pk = er.make_keypair(ring, 32)
    np.array([len(ol.Q_PN14), len(ol.P_PN14)] + ol.Q_PN14 + ol.P_PN14, dtype=np.uint64).tofile(tmp_path / "moduli.bin")
    pk.tofile(tmp_path / "pk.bin")
    ol.secret_ntt(ring, s).tofile(tmp_path / "sk.bin")
    np.frombuffer(er.TEST_KEY, dtype=np.uint64).tofile(tmp_path / "key.bin")
    vals = np.random.default_rng(6).uniform(-10, 10, (vrows, vlen))
    vals.tofile(tmp_path / "vals.bin")
    (tmp_path / "case.txt").write_text(f"{vrows} {vlen} {level}\n")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stderr
    worst_code, worst_crypt = (float(x) for x in out.stdout.split()[1:3])
    # each of the N real coefficients moves a slot by at most its own error: 1/2 from the encoder's rounding; a fresh encryption under a ternary secret adds at most
    # ceil(19 (2N + 1) / P) + 2 (N + 1) (tests/test_gpu_encrypt.py NOISE_BOUND)
    noise = -(-19 * (2 * N + 1) // (ol.P_PN14[0] * ol.P_PN14[1])) + 2 * (N + 1)
    print(f"host mirror: decode(encode) {worst_code:.3e} (bound {0.5 * N / scale:.3e}), decrypt(encrypt) {worst_crypt:.3e} (bound {(noise + 0.5) * N / scale:.3e})")
    assert worst_code <= 0.5 * N / scale
    assert worst_crypt <= (noise + 0.5) * N / scale
