"""The host mirror's collective key generation (sfgwas_amd/host/gwas.hpp: mpc::CollectivePubKeyGenShare / Finish, CollectiveRotKeyGenShares / Finish,
CollectiveRelinKeyGenRound1 / Round2 / Finish, crypto::GenerateRotKeys) driven by a C++ program the way the Go callers would: two parties in one program, the keys
installed on a third context, a vector rotated and squared under them within the bounds DESIGN.md section 11 derives; the Galois set against a literal restatement."""
import subprocess

import numpy as np
import pytest

import keygen_ref as kr
import oracle_lib as ol
from test_gpu_keygen import derived_bounds
from test_host_mirror import build

pytestmark = pytest.mark.gpu


def test_host_mirror_two_party_key_generation(tmp_path):
    from sfgwas_amd import capi
    capi.lib()
    exe = build("host_keygen_test")
    ring = ol.Ring(14, ol.Q_PN14, ol.P_PN14)
    N, level, nrot, scale, vmax = ring.N, 2, 5, 2.0 ** 34, 4.0
    rnd = np.random.default_rng(77)
    s1, s2 = (rnd.integers(-1, 2, N) for _ in range(2))
    np.array([len(ol.Q_PN14), len(ol.P_PN14)] + ol.Q_PN14 + ol.P_PN14, dtype=np.uint64).tofile(tmp_path / "moduli.bin")
    for name, s in (("sk1", s1), ("sk2", s2), ("skS", s1 + s2)):
        kr.to_u64(kr.rows_of(ring, s)).tofile(tmp_path / (name + ".bin"))
    rnd.uniform(-vmax, vmax, ring.slots).tofile(tmp_path / "vals.bin")
    (tmp_path / "case.txt").write_text(f"{level} {nrot}\n")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stderr
    worst_rot, worst_sq, ngal = out.stdout.split()[1:4]
    bound_rot, bound_sq = derived_bounds(ol.Q_PN14, ol.P_PN14, level, scale, vmax)
    print(f"host mirror, keys made on the device: rotation {float(worst_rot):.3e} (bound {bound_rot:.3e}), square {float(worst_sq):.3e} (bound {bound_sq:.3e}), {ngal} Galois elements")
    assert int(ngal) == 212                                 # GenerateRotKeys(8192, 20, true): 211 distinct left shifts, plus the conjugate
    assert float(worst_rot) <= bound_rot
    assert float(worst_sq) <= bound_sq
