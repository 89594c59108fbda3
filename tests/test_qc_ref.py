"""tests/qc_ref.py (the checker of the device's quality-control scan) pinned against literal loops - one per loop of gwas/qualcontrol.go, written the way the
reference walks its rows - on a 7 x 9 matrix, and its row / column filter against the filtered_* fixtures of tests/golden/input_formats.npz."""
import math
import os

import numpy as np
import pytest

import qc_ref

FX = np.load(os.path.join(os.path.dirname(__file__), "golden", "input_formats.npz"))


def small_case():
    rnd = np.random.default_rng(3)
    geno = rnd.integers(-1, 3, (7, 9)).astype(np.int8)
    geno[2, :] = -1                                   # a fully missing individual
    geno[:, 4] = -7                                   # a fully missing SNP, and not -1: every negative value is missing
    geno[5, 0] = -128
    row_filter = np.array([1, 1, 1, 0, 1, 1, 1], dtype=np.uint8)
    col_filter = np.array([1, 0, 1, 1, 1, 1, 0, 1, 1], dtype=np.uint8)
    pheno = np.array([0, 1, 0, 0, 1, 0, 1], dtype=np.float64)
    return geno, row_filter, col_filter, pheno


def test_scan_counts_equal_a_literal_triple_loop():
    geno, rf, cf, pheno = small_case()
    ctrl = pheno < 1
    for use_rf, use_cf, use_ctrl in [(1, 1, 1), (0, 0, 0), (1, 0, 1), (0, 1, 0)]:
        col = np.zeros((2, 4, 9), dtype=np.uint32)
        miss, het = np.zeros(7, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
        for i in range(7):
            for j in range(9):
                if (use_rf and not rf[i]) or (use_cf and not cf[j]):
                    continue
                x = int(geno[i, j])
                k = 3 if x < 0 else x
                for c in range(2):
                    if c == 0 or (use_ctrl and ctrl[i]):
                        col[c, k, j] += 1
                miss[i] += x < 0
                het[i] += x == 1
        got = qc_ref.scan(geno, rf if use_rf else None, cf if use_cf else None, ctrl if use_ctrl else None)
        assert np.array_equal(got[0], col) and np.array_equal(got[1], miss) and np.array_equal(got[2], het)
        assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32


def test_scan_refuses_a_value_above_two_only_at_a_kept_position():
    geno, rf, cf, _ = small_case()
    geno[3, 2] = 3                                    # dropped row
    geno[0, 6] = 5                                    # dropped column
    qc_ref.scan(geno, rf, cf)
    with pytest.raises(ValueError, match="2 values above 2"):
        qc_ref.scan(geno)


def test_the_three_reference_loops_follow_from_the_counts():
    geno, rf, cf, pheno = small_case()
    # SNPMissFilter: every row, every SNP
    x_count = [0] * 9
    for indiv in geno:
        for j, x in enumerate(indiv):
            if int(x) >= 0:
                x_count[j] += 1
    assert list(qc_ref.snp_miss_counts(geno)) == x_count
    # IndividualMissAndHetFilters: rows as the column-filtered stream delivers them
    num_snps = int(cf.sum())
    bounds = (0.4, 0.1, 0.8)
    miss, het, keep = [0] * 7, [0] * 7, [False] * 7
    for idx, row in enumerate(geno[:, cf != 0]):
        for x in row:
            if x < 0:
                miss[idx] += 1
            if x == 1:
                het[idx] += 1
    for i in range(7):
        miss_rate = miss[i] / num_snps
        het_rate = het[i] / (num_snps - miss[i]) if num_snps != miss[i] else math.nan     # Go's float64 0 / 0
        keep[i] = miss_rate < bounds[0] and het_rate < bounds[2] and het_rate > bounds[1]
    got = qc_ref.individual_miss_and_het_filters(geno, cf, num_snps, *bounds)
    assert list(got[0]) == miss and list(got[1]) == het and list(got[2]) == keep
    assert not keep[2] and any(keep)                  # the fully missing individual is dropped, not everybody is
    # SNPMAFAndHWEFilters: the filtered stream, pheno read at the stream's row index
    rows = np.flatnonzero(rf)
    n = num_snps
    x_sum, x_cnt, x_sum_c, x_cnt_c, obs = [0] * n, [0] * n, [0] * n, [0] * n, [[0] * n for _ in range(3)]
    for i in rows:
        yi = int(pheno[i])
        for j, x in enumerate(geno[i, cf != 0]):
            snp = int(x)
            if snp >= 0:
                x_sum[j] += snp
                x_cnt[j] += 2
                if yi < 1:
                    x_sum_c[j] += snp
                    x_cnt_c[j] += 2
                    obs[snp][j] += 1
    got = qc_ref.snp_maf_and_hwe_counts(geno, rf, cf, pheno)
    assert [list(v) for v in got[:4]] == [x_sum, x_cnt, x_sum_c, x_cnt_c]
    assert [list(v) for v in got[4]] == obs


@pytest.mark.parametrize("k", range(6))
def test_filter_matrix_equals_the_filtered_fixtures(k):
    geno, rf, cf = FX[f"geno_{k}"], FX[f"rowfilt_{k}"], FX[f"colfilt_{k}"]
    assert np.array_equal(qc_ref.filter_matrix(geno, rf, cf), FX[f"filtered_{k}"])
    assert np.array_equal(qc_ref.filter_matrix(geno), geno)
    assert np.array_equal(qc_ref.filter_matrix(geno, rf, None), geno[rf != 0])
