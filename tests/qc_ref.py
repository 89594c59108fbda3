"""numpy restatement of the local genotype passes of the reference's quality control (gwas/qualcontrol.go) and of its row / column filter
(scripts/filterMatrix.py), the checker of sfg_geno_qc_scan / sfg_geno_filter and of the host mirror's gwas::qc.

  scan(geno, row_filter, col_filter, row_ctrl) -> col_counts [2][4][ncol], row_miss [nrow], row_het [nrow]   (the library's output contract)
  snp_miss_counts                  the per-SNP count of non-missing calls of SNPMissFilter
  individual_miss_and_het_filters  miss / het per individual and the float64 ikeep rule of IndividualMissAndHetFilters
  snp_maf_and_hwe_counts           xSum, xCount, xSumCtrl, xCountCtrl, genoObservedCtrl[0..2] of SNPMAFAndHWEFilters, compacted to the kept columns
  filter_matrix                    kept rows and columns, in order
"""
import numpy as np


def _mask(f, n):
    return np.ones(n, dtype=bool) if f is None else np.asarray(f) != 0


def scan(geno, row_filter=None, col_filter=None, row_ctrl=None):
    geno = np.asarray(geno, dtype=np.int8)
    nrow, ncol = geno.shape
    rk, ck = _mask(row_filter, nrow), _mask(col_filter, ncol)
    ctrl = np.zeros(nrow, dtype=bool) if row_ctrl is None else np.asarray(row_ctrl) != 0
    kept = rk[:, None] & ck[None, :]
    if (kept & (geno > 2)).any():
        raise ValueError(f"{int((kept & (geno > 2)).sum())} values above 2 at kept positions")
    col = np.zeros((2, 4, ncol), dtype=np.uint32)
    for c, rows in enumerate((rk, rk & ctrl)):
        m = rows[:, None] & ck[None, :]
        for k in range(3):
            col[c, k] = (m & (geno == k)).sum(axis=0)
        col[c, 3] = (m & (geno < 0)).sum(axis=0)
    row_miss = (kept & (geno < 0)).sum(axis=1).astype(np.uint32)
    row_het = (kept & (geno == 1)).sum(axis=1).astype(np.uint32)
    return col, row_miss, row_het


def snp_miss_counts(geno):
    """xCount of SNPMissFilter: per SNP, the calls that are not missing"""
    return scan(geno)[0][0, :3].sum(axis=0).astype(np.int64)


def individual_miss_and_het_filters(geno, col_filter, num_snps, ind_miss_bound, het_lower, het_upper):
    """over the SNPs that survived the first filter; missRate = miss / numSnps, hetRate = het / (numSnps - miss) in float64, strict inequalities;
    0 / 0 is NaN and compares false"""
    _, miss, het = scan(geno, None, col_filter)
    miss, het = miss.astype(np.int64), het.astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        miss_rate = miss.astype(np.float64) / np.float64(num_snps)
        het_rate = het.astype(np.float64) / (num_snps - miss).astype(np.float64)
        keep = (miss_rate < ind_miss_bound) & (het_rate < het_upper) & (het_rate > het_lower)
    return miss, het, keep


def snp_maf_and_hwe_counts(geno, row_filter, col_filter, pheno):
    """pheno: one value per ORIGINAL row; the control cohort is pheno < 1"""
    ctrl = np.asarray(pheno) < 1
    col, _, _ = scan(geno, row_filter, col_filter, ctrl)
    ck = _mask(col_filter, np.asarray(geno).shape[1])
    c = col[:, :, ck].astype(np.int64)
    x_sum, x_count = c[0, 1] + 2 * c[0, 2], 2 * c[0, :3].sum(axis=0)
    x_sum_ctrl, x_count_ctrl = c[1, 1] + 2 * c[1, 2], 2 * c[1, :3].sum(axis=0)
    return x_sum, x_count, x_sum_ctrl, x_count_ctrl, c[1, :3]


def filter_matrix(geno, row_filter=None, col_filter=None):
    geno = np.asarray(geno)
    return np.ascontiguousarray(geno[_mask(row_filter, geno.shape[0])][:, _mask(col_filter, geno.shape[1])])
