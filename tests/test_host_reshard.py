"""From quality control to the PCA on the sharded matrix through the host mirror (sfgwas_amd/host/gwas.hpp: gwas::qc::FilterResidentSharded, SketchSharded,
ColSumsSharded) and through the C-ABI, driven by a C++ program at world 3 on one device: every shard it prints is compared with tests/reshard_ref.py, the sketch
and the moments with numpy on the filtered matrix."""
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import qc_ref
import reshard_ref as rr
from sfgwas_amd.sharding import SLOTS
from test_host_mirror import build

pytestmark = pytest.mark.gpu


def test_host_mirror_filter_sketch_and_moments_on_the_sharded_matrix(tmp_path):
    from sfgwas_amd import capi
    capi.lib()
    exe = build("host_reshard_test")
    nrow, ncol, world, kp = 23, 2 * SLOTS + 131, 3, 6
    geno = rr.make_geno(nrow, ncol, 31)
    rf, cf = rr.make_filters(nrow, ncol, 31, p_row=0.8, p_col=0.6)
    rnd = np.random.default_rng(32)
    bucket, sgn = rnd.integers(0, kp, nrow).astype(np.int32), rnd.choice(np.array([-1, 1], dtype=np.int8), nrow)
    np.array([len(ol.Q_PN14), len(ol.P_PN14)] + ol.Q_PN14 + ol.P_PN14, dtype=np.uint64).tofile(tmp_path / "moduli.bin")
    geno.tofile(tmp_path / "geno.bin"); rf.tofile(tmp_path / "rowfilt.bin"); cf.tofile(tmp_path / "colfilt.bin")
    bucket.tofile(tmp_path / "bucket.bin"); sgn.tofile(tmp_path / "sgn.bin")
    (tmp_path / "case.txt").write_text(f"{nrow} {ncol} {world} {kp}\n")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stderr
    got = {}
    for ln in out.stdout.splitlines()[:-1]:
        w = ln.split()
        got.setdefault(w[0], []).append(np.array(w[1:], dtype=np.int64))
    for name, r, c in (("copy", None, None), ("filtered", rf, cf)):
        want = rr.windows(geno, r, c, world)
        assert len(got[name]) == world
        for i, a in enumerate(got[name]):
            assert a[0] == i
            if want[i] is None:
                assert tuple(a[1:]) == (0, 0)
            else:
                assert tuple(a[1:3]) == want[i].shape and np.array_equal(a[3:].reshape(want[i].shape), want[i]), f"{name}: shard {i}"
    filt = qc_ref.filter_matrix(geno, rf, cf).astype(np.int64)
    keep = rf != 0
    S = np.zeros((kp, filt.shape[0]), dtype=np.int64)
    S[bucket[keep], np.arange(filt.shape[0])] = sgn[keep]
    assert np.array_equal(got["sketch"][0].reshape(kp, -1), S @ filt)
    assert np.array_equal(got["xsum"][0], filt.sum(axis=0)) and np.array_equal(got["x2sum"][0], (filt * filt).sum(axis=0))
    seen = np.where(filt < 0, 0, filt)
    assert np.array_equal(got["colsum"][0], seen.sum(axis=0)) and np.array_equal(got["colsq"][0], (seen * seen).sum(axis=0))
