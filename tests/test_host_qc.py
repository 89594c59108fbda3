"""Quality control through the host mirror (sfgwas_amd/host/gwas.hpp, namespace gwas::qc), driven by a C++ program the way the Go callers of
gwas/qualcontrol.go would: every number it prints is compared with tests/qc_ref.py.  One individual is fully missing: 0 / 0 in the het rate must drop it,
not crash."""
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import qc_ref
from test_host_mirror import build

pytestmark = pytest.mark.gpu


def test_host_mirror_quality_control(tmp_path):
    from sfgwas_amd import capi
    capi.lib()
    exe = build("host_qc_test")
    rnd = np.random.default_rng(19)
    nrow, ncol = 211, 4133
    geno = rnd.choice(np.array([-1, 0, 1, 2, -9], dtype=np.int8), size=(nrow, ncol), p=[0.08, 0.42, 0.3, 0.18, 0.02])
    rf, cf = (rnd.random(nrow) < 0.8).astype(np.uint8), (rnd.random(ncol) < 0.7).astype(np.uint8)
    geno[17, :] = -1                                  # fully missing: missRate 1, hetRate 0 / 0
    geno[40, cf != 0] = -1                            # missing on every kept SNP only
    geno[41, :] = 1                                   # all het: above the upper bound
    pheno = rnd.integers(0, 2, nrow).astype(np.float64)
    num_snps, bounds = int(cf.sum()), (0.12, 0.25, 0.36)
    np.array([len(ol.Q_PN14), len(ol.P_PN14)] + ol.Q_PN14 + ol.P_PN14, dtype=np.uint64).tofile(tmp_path / "moduli.bin")
    geno.tofile(tmp_path / "geno.bin"); rf.tofile(tmp_path / "rowfilt.bin"); cf.tofile(tmp_path / "colfilt.bin"); pheno.tofile(tmp_path / "pheno.bin")
    (tmp_path / "case.txt").write_text(f"{nrow} {ncol} {num_snps} {bounds[0]!r} {bounds[1]!r} {bounds[2]!r}\n")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    got = {}
    for ln in lines[:-1]:
        got.setdefault(ln[0], []).append(np.array(ln[1:], dtype=np.int64))
    assert np.array_equal(got["snpmiss"][0], qc_ref.snp_miss_counts(geno))
    _, _, keep = qc_ref.individual_miss_and_het_filters(geno, cf, num_snps, *bounds)
    assert np.array_equal(got["ikeep"][0], keep.astype(np.int64))
    assert not keep[17] and not keep[40] and not keep[41] and 0 < keep.sum() < nrow
    want = qc_ref.snp_maf_and_hwe_counts(geno, rf, cf, pheno)
    for name, w in zip(("xsum", "xcount", "xsumctrl", "xcountctrl"), want[:4]):
        assert np.array_equal(got[name][0], w), name
    assert len(got["obsctrl"]) == 3 and all(np.array_equal(a, b) for a, b in zip(got["obsctrl"], want[4]))
    filt = qc_ref.filter_matrix(geno, rf, cf)
    f = got["filtered"][0]
    assert tuple(f[:2]) == filt.shape and np.array_equal(f[2:].reshape(filt.shape), filt)
