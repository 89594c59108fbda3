"""The host mirror's device encryption (sfgwas_amd/host/gwas.hpp: CAddFreshZeroDev, EncryptFloatMatrixRowDev, CZerosDev) driven by a C++ program the way the
Go callers would, against the same calls made through the C ABI under the same sampler key: every word, and the number of encryption indices spent."""
import subprocess

import numpy as np
import pytest

import encrypt_ref as er
import oracle_lib as ol
from test_host_mirror import build

pytestmark = pytest.mark.gpu


def test_host_mirror_fresh_zero_and_encrypt_matrix_rows(tmp_path):
    from sfgwas_amd import capi
    capi.lib()
    exe = build("host_encrypt_test")
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    N, rows, cols, level, vrows, vlen, vlevel = ring.N, 2, 2, 4, 2, ring.slots + 100, 3
    _, pk = er.make_keypair(ring, 32)
    np.array([len(ol.Q_PN14), len(ol.P_PN14)] + ol.Q_PN14 + ol.P_PN14, dtype=np.uint64).tofile(tmp_path / "moduli.bin")
    pk.tofile(tmp_path / "pk.bin")
    np.frombuffer(er.TEST_KEY, dtype=np.uint64).tofile(tmp_path / "key.bin")
    M = np.stack([np.stack([ring.fill_uniform(level, 700 + 10 * i + j) for j in range(cols)]) for i in range(rows)])
    M.tofile(tmp_path / "M.bin")
    vals = np.random.default_rng(6).uniform(-10, 10, (vrows, vlen))
    vals.tofile(tmp_path / "vals.bin")
    (tmp_path / "case.txt").write_text(f"{rows} {cols} {level} {vrows} {vlen} {vlevel}\n")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stderr
    nvec = 2                                                   # ceil(vlen / slots)
    assert int(out.stdout.split()[1]) == rows * cols + vrows * nvec + 2
    ctx = capi.Context(ol.Q_PN14, ol.P_PN14)
    try:
        ctx.load_public_key(pk); ctx.seed_encryptor(er.TEST_KEY)
        d = capi.DevArray.from_host(ctx, M)
        ctx.add_fresh_zero(d, level)
        assert np.array_equal(np.fromfile(tmp_path / "finished.bin", dtype=np.uint64).reshape(M.shape), d.host())
        d.free()
        padded = np.zeros((vrows, nvec * ring.slots)); padded[:, :vlen] = vals
        e = ctx.encrypt_vectors(padded.reshape(vrows * nvec, ring.slots), vlevel)
        assert np.array_equal(np.fromfile(tmp_path / "encrypted.bin", dtype=np.uint64).reshape(e.shape), e.host())
        e.free()
        z = capi.DevArray.from_host(ctx, np.zeros((2, 2, vlevel + 1, N), dtype=np.uint64))
        ctx.add_fresh_zero(z, vlevel)
        got = np.fromfile(tmp_path / "zeros.bin", dtype=np.uint64).reshape(z.shape)
        assert np.array_equal(got, z.host()) and got.any()
        z.free()
    finally:
        ctx.close()
