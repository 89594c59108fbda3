"""ctypes binding of libsfgwas_hip.so (the C-ABI declared in include/sfgwas_hip.h).

This is plumbing for tests and bench.py; the product is the shared library.  There is no CPU
fallback: if the library is missing or no GPU is present, calls fail loudly.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFG_LIB_PATH") or os.path.join(_HERE, "lib", "libsfgwas_hip.so")      # SFG_LIB_PATH: same-box A/B of two builds
AB_LIB_PATH = os.path.join(_HERE, "lib_ab", "libsfgwas_hip.so")      # the experimenters' build (`make -C sfgwas_amd/csrc ab`): superseded kernels + their A/B switches
# what the product library reads from the environment (sfgwas_amd/csrc/ctx.hip: read_config); every other SFG_* switch exists in the A/B build only
DEPLOYMENT_SWITCHES = {"SFG_MM_GROUP", "SFG_MM_ACC_BUDGET_MB", "SFG_ASSOC_ROTCACHE_MB", "SFG_KSW_BUDGET_MB", "SFG_ENC_BATCH", "SFG_UPLOAD_BLOCKING",
                       "SFG_MGPU_TRANSPORT", "SFG_MGPU_CACHE_GB", "SFG_RCCL_LIB", "SFG_ENABLE_TEST_HOOKS",
                       "SFG_TEST_SCRATCH_OOM", "SFG_TEST_TIE_BAND_LOG2", "SFG_MGPU_FORCE_COLLECTIVES"}


def ab_lib():
    """path of the A/B build, made on demand (a few minutes the first time; `make ab` is part of __graft_entry__.build)"""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "ab", "-j8"], stdout=subprocess.DEVNULL)
    return AB_LIB_PATH


def env_for(switches):
    """environment additions for a child process that sets `switches`: the A/B library when any of them is not a deployment switch"""
    e = {k: str(v) for k, v in switches.items()}
    if any(k.startswith("SFG_") and k not in DEPLOYMENT_SWITCHES for k in e):
        e["SFG_LIB_PATH"] = ab_lib()
    return e


class SfgConfig(C.Structure):
    """include/sfgwas_hip.h: sfg_config"""
    _fields_ = [("struct_size", C.c_uint32), ("mm_group", C.c_int), ("acc_budget_bytes", C.c_size_t), ("assoc_rotcache_bytes", C.c_size_t),
                ("ksw_budget_bytes", C.c_size_t), ("enc_batch", C.c_int), ("upload_blocking", C.c_int), ("mgpu_transport", C.c_char_p),
                ("mgpu_cache_bytes", C.c_size_t), ("rccl_lib", C.c_char_p)]

    def __init__(self, **kw):
        super().__init__()
        self.struct_size = C.sizeof(SfgConfig)
        for k, v in kw.items():
            setattr(self, k, v)

u64p = C.POINTER(C.c_uint64)
_lib = None

SFG_SQUARE = 1
SFG_TRANSPOSE = 2
SFG_STREAM_DIRECT = 4


class SfgError(RuntimeError):
    pass


def _ring_sig():
    """the general ring's entry points (include/sfgwas_hip.h: sfg_ring_*)"""
    vp, i, u64, sz = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t
    ip = C.POINTER(C.c_int)
    return {
        "sfg_ring_create": (i, [C.POINTER(vp), i, i, i, i, u64p, u64p]),
        "sfg_ring_destroy": (None, [vp]),
        "sfg_ring_last_error": (C.c_char_p, [vp]),
        "sfg_ring_synchronize": (i, [vp]),
        "sfg_ring_malloc": (i, [vp, C.POINTER(vp), sz]),
        "sfg_ring_free": (i, [vp, vp]),
        "sfg_ring_memcpy_h2d": (i, [vp, vp, vp, sz]),
        "sfg_ring_memcpy_d2h": (i, [vp, vp, vp, sz]),
        "sfg_ring_ntt_rows": (i, [vp, vp, i, ip]),
        "sfg_ring_intt_rows": (i, [vp, vp, i, ip]),
        "sfg_ring_load_rotkey": (i, [vp, u64, u64p, i]),
        "sfg_ring_has_rotkey": (i, [vp, u64]),
        "sfg_ring_load_relinkey": (i, [vp, u64p, i]),
        "sfg_ring_galois_for_rotation": (u64, [vp, i]),
        "sfg_ring_rotate_right_dev": (i, [vp, vp, vp, i, i, ip]),
        "sfg_ring_ct_galois_dev": (i, [vp, vp, vp, i, i, u64]),
        "sfg_ring_ct_add_dev": (i, [vp, vp, vp, vp, i, i]),
        "sfg_ring_ct_sub_dev": (i, [vp, vp, vp, vp, i, i]),
        "sfg_ring_ct_drop_level_dev": (i, [vp, vp, vp, i, i, i]),
        "sfg_ring_ct_mul_scalar_dev": (i, [vp, vp, u64p, vp, i, i]),
        "sfg_ring_ct_mul_scalar_add_dev": (i, [vp, vp, u64p, vp, i, i]),
        "sfg_ring_ct_add_scalar_dev": (i, [vp, vp, u64p, vp, i, i]),
        "sfg_ring_ct_add_plain_dev": (i, [vp, vp, vp, sz, vp, i, i]),
        "sfg_ring_ct_mul_plain_dev": (i, [vp, vp, vp, sz, vp, i, i]),
        "sfg_ring_ct_mulrelin_dev": (i, [vp, vp, vp, vp, i, i]),
        "sfg_ring_ct_rescale_dev": (i, [vp, vp, vp, i, i]),
        "sfg_ring_ct_innersum_dev": (i, [vp, vp, i, i, vp]),
        "sfg_ring_load_public_key": (i, [vp, u64p, i]),
        "sfg_ring_has_public_key": (i, [vp]),
        "sfg_ring_load_secret_key": (i, [vp, u64p, i]),
        "sfg_ring_seed_encryptor": (i, [vp, C.c_char_p]),
        "sfg_ring_encryptor_next_index": (i, [vp, u64p]),
        "sfg_ring_encrypt_explicit_dev": (i, [vp, vp, i, i, vp, vp, vp, vp]),
        "sfg_ring_ct_add_fresh_zero_dev": (i, [vp, vp, i, i]),
        "sfg_ring_encrypt_transcript_for_test": (i, [vp, u64, i, vp, vp, vp]),
        "sfg_ring_pcks_gen_share_dev": (i, [vp, vp, i, i, vp, vp, vp, vp]),
        "sfg_ring_pcks_finish_dev": (i, [vp, vp, i, i, vp, vp]),
        "sfg_ring_decode_coeffs": (i, [vp, vp, sz, i, i, C.c_double, C.POINTER(C.c_double)]),
        "sfg_ring_encode_vectors_dev": (i, [vp, C.POINTER(C.c_double), i, i, C.c_double, vp]),
        "sfg_ring_encrypt_vectors_dev": (i, [vp, C.POINTER(C.c_double), i, i, C.c_double, vp]),
        "sfg_ring_decode_vectors": (i, [vp, vp, sz, i, i, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "sfg_ring_decode_vectors_dev": (i, [vp, vp, sz, i, i, C.c_double, vp, vp]),
        "sfg_ring_decrypt_vectors": (i, [vp, vp, i, i, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "sfg_ring_load_secret_key_qp": (i, [vp, u64p, i]),
        "sfg_ring_ckg_gen_share_dev": (i, [vp, vp, vp, vp]),
        "sfg_ring_rtg_gen_shares_dev": (i, [vp, u64p, i, vp, vp, vp]),
        "sfg_ring_rkg_round1_dev": (i, [vp, vp, vp, vp, vp, vp, vp]),
        "sfg_ring_rkg_round2_dev": (i, [vp, vp, vp, vp, vp, vp, vp]),
        "sfg_ring_ckg_gen_share_sampled_dev": (i, [vp, vp, vp, u64p]),
        "sfg_ring_rtg_gen_shares_sampled_dev": (i, [vp, u64p, i, vp, vp, u64p]),
        "sfg_ring_rkg_round1_sampled_dev": (i, [vp, vp, vp, vp, u64p, u64p]),
        "sfg_ring_rkg_round2_sampled_dev": (i, [vp, vp, vp, u64, vp, u64p]),
        "sfg_ring_install_public_key_dev": (i, [vp, vp, vp]),
        "sfg_ring_install_rotkeys_dev": (i, [vp, u64p, i, vp, vp]),
        "sfg_ring_install_relinkey_dev": (i, [vp, vp, vp]),
        "sfg_ring_export_rotkey": (i, [vp, u64, u64p]),
        "sfg_ring_crp_fill_dev": (i, [vp, C.c_char_p, u64, sz, ip, vp]),
        "sfg_ring_refresh_gen_shares_dev": (i, [vp, vp, i, i, vp, vp, i, vp, vp, vp, vp]),
        "sfg_ring_refresh_finish_dev": (i, [vp, vp, i, i, vp, vp, vp, vp]),
        "sfg_ring_refresh_gen_shares_scaled_dev": (i, [vp, vp, i, i, C.c_double, C.c_double, vp, vp, i, vp, vp, vp, vp]),
        "sfg_ring_refresh_finish_scaled_dev": (i, [vp, vp, i, i, C.c_double, C.c_double, vp, vp, vp, vp]),
        "sfg_ring_matmul_dev": (i, [vp, vp, i, i, i, vp, sz, sz, sz, C.c_uint, C.c_double, vp]),
        "sfg_ring_matmul_accumulate_dev": (i, [vp, vp, i, i, i, vp, sz, sz, sz, C.c_uint, C.c_double, i, i, vp, C.POINTER(C.c_uint8)]),
        "sfg_ring_matmul_finalize_dev": (i, [vp, vp, C.POINTER(C.c_uint8), i, i, i, i, i, i, vp]),
        "sfg_ring_set_ws_budget_for_test": (i, [vp, sz]),
        "sfg_ring_encoder_resolved": (i, [vp, C.POINTER(C.c_ulonglong), i]),
        "sfg_ring_set_tie_band_for_test": (i, [vp, i]),
    }


def _sig(L):
    vp, i, u64, d, sz = C.c_void_p, C.c_int, C.c_uint64, C.c_double, C.c_size_t
    S = {
        "sfg_ctx_create": (i, [C.POINTER(vp), i, i, i, i, u64p, u64p, d]),
        "sfg_ctx_create_ex": (i, [C.POINTER(vp), i, i, i, i, u64p, u64p, d, vp]),
        "sfg_config_default": (None, [vp]),
        "sfg_mgpu_create_ex": (i, [C.POINTER(vp), C.POINTER(i), i, i, i, i, u64p, u64p, d, vp]),
        "sfg_mgpu_create_rank_ex": (i, [C.POINTER(vp), i, i, i, vp, i, i, i, u64p, u64p, d, vp]),
        "sfg_ctx_fork": (i, [vp, C.POINTER(vp)]),
        "sfg_ctx_destroy": (None, [vp]),
        "sfg_last_error": (C.c_char_p, [vp]),
        "sfg_ctx_synchronize": (i, [vp]),
        "sfg_ctx_set_stream": (i, [vp, vp]),
        "sfg_ctx_release_scratch": (i, [vp]),
        "sfg_ctx_scratch_bytes": (i, [vp, C.c_char_p, C.POINTER(C.c_size_t)]),
        "sfg_rotcache_invalidate": (i, [vp]),
        "sfg_ctx_use_own_stream": (i, [vp]),
        "sfg_ctx_encoder_inject_unsafe_for_test": (i, [vp, C.c_ulonglong]),
        "sfg_ctx_encoder_resolved": (i, [vp, C.POINTER(C.c_ulonglong)]),
        "sfg_ctx_encoder_unprovable": (i, [vp, C.POINTER(C.c_ulonglong)]),
        "sfg_ctx_load_rotkey": (i, [vp, u64, u64p, i]),
        "sfg_ctx_load_secret_key": (i, [vp, u64p, i]),
        "sfg_ctx_load_public_key": (i, [vp, u64p, i]),
        "sfg_ctx_has_public_key": (i, [vp]),
        "sfg_ctx_seed_encryptor": (i, [vp, C.c_char_p]),
        "sfg_ctx_encryptor_next_index": (i, [vp, C.POINTER(u64)]),
        "sfg_encrypt_explicit_dev": (i, [vp, vp, i, i, vp, vp, vp, vp]),
        "sfg_ct_add_fresh_zero_dev": (i, [vp, vp, i, i]),
        "sfg_encrypt_vectors_dev": (i, [vp, C.POINTER(d), i, i, vp]),
        "sfg_encrypt_transcript_for_test": (i, [vp, u64, i, vp, vp, vp]),
        "sfg_ctx_load_secret_key_qp": (i, [vp, u64p, i]),
        "sfg_ckg_gen_share_dev": (i, [vp, vp, vp, vp]),
        "sfg_rtg_gen_shares_dev": (i, [vp, u64p, i, vp, vp, vp]),
        "sfg_rkg_round1_dev": (i, [vp, vp, vp, vp, vp, vp, vp]),
        "sfg_rkg_round2_dev": (i, [vp, vp, vp, vp, vp, vp, vp]),
        "sfg_ckg_gen_share_sampled_dev": (i, [vp, vp, vp, C.POINTER(u64)]),
        "sfg_rtg_gen_shares_sampled_dev": (i, [vp, u64p, i, vp, vp, C.POINTER(u64)]),
        "sfg_rkg_round1_sampled_dev": (i, [vp, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)]),
        "sfg_rkg_round2_sampled_dev": (i, [vp, vp, vp, u64, vp, C.POINTER(u64)]),
        "sfg_ctx_install_public_key_dev": (i, [vp, vp, vp]),
        "sfg_ctx_install_rotkeys_dev": (i, [vp, u64p, i, vp, vp]),
        "sfg_ctx_install_relinkey_dev": (i, [vp, vp, vp]),
        "sfg_crp_fill_dev": (i, [vp, C.c_char_p, u64, sz, C.POINTER(i), vp]),
        "sfg_pcks_gen_share_dev": (i, [vp, vp, i, i, vp, vp, vp, vp]),
        "sfg_pcks_finish_dev": (i, [vp, vp, i, i, vp, vp]),
        "sfg_decode_vectors": (i, [vp, vp, sz, i, i, d, vp, vp]),
        "sfg_decode_vectors_dev": (i, [vp, vp, sz, i, i, d, vp, vp]),
        "sfg_decode_coeffs": (i, [vp, vp, sz, i, i, d, vp]),
        "sfg_pcks_finish_decode": (i, [vp, vp, i, i, d, vp, vp, vp]),
        "sfg_decrypt_vectors": (i, [vp, vp, i, i, d, vp, vp]),
        "sfg_ct_galois_dev": (i, [vp, vp, vp, i, i, u64]),
        "sfg_ct_mul_scalar_add_dev": (i, [vp, vp, u64p, vp, i, i]),
        "sfg_refresh_gen_shares_dev": (i, [vp, vp, i, i, vp, vp, i, vp, vp, vp, vp]),
        "sfg_refresh_finish_dev": (i, [vp, vp, i, i, vp, vp, vp, vp]),
        "sfg_refresh_gen_shares_scaled_dev": (i, [vp, vp, i, i, d, d, vp, vp, i, vp, vp, vp, vp]),
        "sfg_refresh_finish_scaled_dev": (i, [vp, vp, i, i, d, d, vp, vp, vp, vp]),
        "sfg_ckks_to_ss_share_dev": (i, [vp, vp, i, i, vp, i, vp, vp, vp]),
        "sfg_rvec_encode_dev": (i, [vp, i, u64p, vp, i, i, i, d, i, vp]),
        "sfg_rvec_decode_dev": (i, [vp, i, u64p, vp, sz, i, i, d, i, i, vp]),
        "sfg_ckks_to_ss_finish_dev": (i, [vp, i, u64p, vp, i, i, d, i, vp, vp, i, i, vp]),
        "sfg_geno_pack": (i, [vp, vp, C.POINTER(vp)]),
        "sfg_geno_unpack": (i, [vp, vp, C.POINTER(vp)]),
        "sfg_assoc_stream_bed": (i, [vp, C.c_char_p, sz, sz, vp, vp, sz, vp, i, i, i, C.c_uint, vp, sz, C.POINTER(sz), vp, vp]),
        "sfg_assoc_stream_pgen": (i, [vp, C.c_char_p, vp, vp, sz, vp, i, i, i, C.c_uint, vp, sz, C.POINTER(sz), vp, vp]),
        "sfg_assoc_pgen": (i, [vp, vp, sz, vp, vp, sz, vp, i, i, i, C.c_uint, vp, sz, C.POINTER(sz), vp, vp]),
        "sfg_ctx_has_rotkey": (i, [vp, u64]),
        "sfg_ctx_export_rotkey": (i, [vp, u64, u64p]),
        "sfg_galois_for_rotation": (u64, [vp, i]),
        "sfg_malloc": (i, [vp, C.POINTER(vp), sz]),
        "sfg_free": (i, [vp, vp]),
        "sfg_memcpy_h2d": (i, [vp, vp, vp, sz]),
        "sfg_memcpy_d2h": (i, [vp, vp, vp, sz]),
        "sfg_memcpy_d2d": (i, [vp, vp, vp, sz]),
        "sfg_ct_drop_level_dev": (i, [vp, vp, vp, i, i, i]),
        "sfg_ntt_rows": (i, [vp, vp, i, C.POINTER(i)]),
        "sfg_intt_rows": (i, [vp, vp, i, C.POINTER(i)]),
        "sfg_mac_dev": (i, [vp, vp, vp, vp, i, i, i, i, i]),
        "sfg_mac_i8_dev": (i, [vp, vp, vp, vp, i, i, i, i, i, i]),
        "sfg_i8_move_for_test": (i, [vp, vp, sz, i, sz, sz, i, i, i, i, i, i, i, i, vp, i, vp, sz, vp, sz, vp, sz, C.POINTER(i)]),
        "sfg_encode_diags_dev": (i, [vp, vp, sz, i, i, i, i, i, i, vp]),
        "sfg_encode_coeffs_host": (i, [vp, C.POINTER(d), i, C.POINTER(C.c_int64)]),
        "sfg_encode_vectors_dev": (i, [vp, C.POINTER(d), i, i, vp]),
        "sfg_ctx_encoder_near_ties": (i, [vp, C.POINTER(C.c_ulonglong), i]),
        "sfg_rotate_right_dev": (i, [vp, vp, vp, i, i, C.POINTER(i)]),
        "sfg_ct_add_dev": (i, [vp, vp, vp, vp, i, i]),
        "sfg_ct_sub_dev": (i, [vp, vp, vp, vp, i, i]),
        "sfg_ct_mul_scalar_dev": (i, [vp, vp, u64p, vp, i, i]),
        "sfg_ct_add_scalar_dev": (i, [vp, vp, u64p, vp, i, i]),
        "sfg_ct_add_plain_dev": (i, [vp, vp, vp, sz, vp, i, i]),
        "sfg_ctx_load_relinkey": (i, [vp, u64p, i]),
        "sfg_ct_mulrelin_dev": (i, [vp, vp, vp, vp, i, i]),
        "sfg_ct_mul_plain_dev": (i, [vp, vp, vp, sz, vp, i, i]),
        "sfg_ct_rescale_dev": (i, [vp, vp, vp, i, i]),
        "sfg_ct_innersum_dev": (i, [vp, vp, i, i, vp]),
        "sfg_geno_upload": (i, [vp, vp, sz, sz, sz, C.POINTER(vp)]),
        "sfg_geno_from_device": (i, [vp, vp, sz, sz, sz, C.POINTER(vp)]),
        "sfg_geno_free": (None, [vp, vp]),
        "sfg_geno_create": (i, [vp, sz, sz, C.POINTER(vp)]),
        "sfg_geno_write_rows": (i, [vp, vp, sz, sz, vp, sz]),
        "sfg_geno_compare_rows": (i, [vp, vp, C.c_uint, sz, sz, vp, sz, u64p]),
        "sfg_pinned_alloc": (i, [vp, C.POINTER(vp), sz]),
        "sfg_pinned_free": (i, [vp, vp]),
        "sfg_geno_set_plaintext_cache": (i, [vp, vp, C.c_size_t]),
        "sfg_geno_plaintext_cache_stats": (i, [vp, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "sfg_geno_from_bed": (i, [vp, vp, sz, sz, sz, vp, vp, C.POINTER(vp)]),
        "sfg_geno_dims": (i, [vp, C.POINTER(sz), C.POINTER(sz)]),
        "sfg_geno_layout": (i, [vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]),
        "sfg_pgen_dims": (i, [vp, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "sfg_geno_from_pgen": (i, [vp, vp, sz, sz, sz, vp, vp, C.POINTER(vp)]),
        "sfg_pgen_geno_counts": (i, [vp, vp, sz, vp, vp]),
        "sfg_geno_download": (i, [vp, vp, vp]),
        "sfg_geno_transpose": (i, [vp, vp, C.POINTER(vp)]),
        "sfg_geno_concat_cols": (i, [vp, C.POINTER(vp), i, C.POINTER(vp)]),
        "sfg_geno_colsums": (i, [vp, vp, C.POINTER(d), C.POINTER(d)]),
        "sfg_geno_qc_scan": (i, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "sfg_geno_filter": (i, [vp, vp, vp, vp, C.POINTER(vp)]),
        "sfg_mgpu_geno_qc_scan": (i, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "sfg_mgpu_geno_filter": (i, [vp, vp, vp, vp, C.POINTER(vp)]),
        "sfg_mgpu_sketch": (i, [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int8), i, C.POINTER(d), u64p, u64p]),
        "sfg_mgpu_geno_colsums": (i, [vp, vp, C.POINTER(d), C.POINTER(d)]),
        "sfg_matmul_resident_dev": (i, [vp, vp, i, i, i, vp, C.c_uint, vp]),
        "sfg_matmul_from_cache": (i, [vp, vp, i, i, i, C.c_char_p, i, vp]),
        "sfg_diagcache_header": (i, [vp, C.c_char_p, i, u64p]),
        "sfg_diagcache_write": (i, [vp, vp, C.c_uint, i, C.c_char_p, C.POINTER(C.c_int)]),
        "sfg_matmul_stream": (i, [vp, u64p, i, i, i, vp, sz, sz, sz, C.c_uint, u64p, C.POINTER(d), C.POINTER(d)]),
        "sfg_matmul_resident_range_dev": (i, [vp, vp, i, i, i, vp, C.c_uint, i, i, vp]),
        "sfg_matmul_accumulate_dev": (i, [vp, vp, i, i, i, vp, C.c_uint, i, i, i, i, i, vp]),
        "sfg_matmul_finalize_dev": (i, [vp, vp, i, i, i, i, i, i, vp]),
        "sfg_matmul_finalize_slots_dev": (i, [vp, vp, i, i, i, i, i, i, i, i, vp]),
        "sfg_reduce_rows_dev": (i, [vp, vp, sz, i]),
        "sfg_rotcache_layout": (i, [vp, i, i, C.POINTER(sz), C.POINTER(sz)]),
        "sfg_rotcache_build_jobs_dev": (i, [vp, vp, i, i, i, i, i, i, vp]),
        "sfg_rotcache_scatter_dev": (i, [vp, vp, i, i, i, i, i, i, vp]),
        "sfg_rotcache_build_rows_dev": (i, [vp, vp, i, i, i, i, i, i, vp]),
        "sfg_matmul_resident_range_rc_dev": (i, [vp, vp, i, i, vp, C.c_uint, i, i, vp]),
        "sfg_matmul_accumulate_rc_dev": (i, [vp, vp, i, i, vp, C.c_uint, i, i, i, i, i, vp]),
        "sfg_beaver_elem_dev": (i, [vp, i, i, u64p, vp, vp, vp, vp, vp, sz]),
        "sfg_ss_mask_dev": (i, [vp, i, u64p, u64p, vp, vp, vp, vp, sz]),
        "sfg_ss_hub_share_dev": (i, [vp, i, u64p, vp, vp, vp, sz]),
        "sfg_beaver_elem": (i, [vp, i, i, u64p, u64p, u64p, u64p, u64p, u64p, sz]),
        "sfg_beaver_matmul": (i, [vp, i, i, u64p, u64p, u64p, u64p, u64p, u64p, i, i, i]),
        "sfg_sketch": (i, [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int8), i, C.POINTER(d), u64p, u64p]),
        "sfg_fill_uniform_ct_dev": (i, [vp, vp, i, i, u64]),
        "sfg_fill_geno_dev": (i, [vp, vp, sz, sz, u64]),
        "sfg_fill_geno_window_dev": (i, [vp, vp, sz, sz, sz, sz, sz, u64]),
        "sfg_fill_rotkeys_synthetic": (i, [vp, C.POINTER(i), i, u64]),
        "sfg_mgpu_unique_id": (i, [vp]),
        "sfg_mgpu_create": (i, [C.POINTER(vp), C.POINTER(i), i, i, i, i, u64p, u64p, d]),
        "sfg_mgpu_create_rank": (i, [C.POINTER(vp), i, i, i, vp, i, i, i, u64p, u64p, d]),
        "sfg_mgpu_destroy": (None, [vp]),
        "sfg_mgpu_last_error": (C.c_char_p, [vp]),
        "sfg_mgpu_world": (i, [vp]),
        "sfg_mgpu_nlocal": (i, [vp]),
        "sfg_mgpu_rank": (i, [vp, i]),
        "sfg_mgpu_ctx": (vp, [vp, i]),
        "sfg_mgpu_transport": (C.c_char_p, [vp]),
        "sfg_mgpu_synchronize": (i, [vp]),
        "sfg_mgpu_load_rotkey": (i, [vp, u64, u64p, i]),
        "sfg_mgpu_load_relinkey": (i, [vp, u64p, i]),
        "sfg_mgpu_fill_rotkeys_synthetic": (i, [vp, C.POINTER(i), i, u64]),
        "sfg_mgpu_shard": (i, [i, sz, i, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "sfg_mgpu_geno_upload": (i, [vp, vp, sz, sz, sz, C.POINTER(vp)]),
        "sfg_mgpu_geno_adopt": (i, [vp, sz, sz, C.POINTER(vp), C.POINTER(vp)]),
        "sfg_mgpu_geno_create": (i, [vp, sz, sz, C.POINTER(vp)]),
        "sfg_mgpu_geno_write_rows": (i, [vp, vp, sz, sz, vp, sz]),
        "sfg_mgpu_geno_compare_rows": (i, [vp, vp, C.c_uint, sz, sz, vp, sz, u64p]),
        "sfg_mgpu_comm_info": (i, [vp, i, C.POINTER(i), C.POINTER(i)]),
        "sfg_mgpu_preflight": (i, [vp, sz]),
        "sfg_mgpu_geno_synthetic": (i, [vp, sz, sz, u64, i, C.POINTER(vp)]),
        "sfg_mgpu_geno_free": (None, [vp, vp]),
        "sfg_mgpu_geno_shard": (vp, [vp, i]),
        "sfg_mgpu_geno_dims": (i, [vp, C.POINTER(sz), C.POINTER(sz)]),
        "sfg_mgpu_geno_blocks": (i, [vp, i, C.POINTER(sz), C.POINTER(sz)]),
        "sfg_mgpu_geno_set_plaintext_cache": (i, [vp, vp, sz]),
        "sfg_mgpu_matmul_dev": (i, [vp, C.POINTER(vp), i, i, i, vp, C.c_uint, C.POINTER(vp)]),
        "sfg_mgpu_matmul": (i, [vp, u64p, i, i, i, vp, C.c_uint, u64p]),
        "sfg_mgpu_inject_failure_for_test": (i, [vp, i, i]),
        "sfg_mgpu_assoc_stream_bed": (i, [vp, C.c_char_p, sz, sz, vp, vp, sz, u64p, i, i, i, C.c_uint, u64p, sz, C.POINTER(sz), vp, vp]),
        "sfg_mgpu_assoc_stream_pgen": (i, [vp, C.c_char_p, vp, vp, sz, sz, u64p, i, i, i, C.c_uint, u64p, sz, C.POINTER(sz), vp, vp]),
        "sfg_ctx_clear_phases": (i, [vp]),
        "sfg_last_phase_ms": (d, [vp, C.c_char_p]),
        "sfg_last_phase_launches": (i, [vp, C.c_char_p]),
        "sfg_last_phase_bytes": (d, [vp, C.c_char_p]),
    }
    S.update(_ring_sig())
    for name, (res, args) in S.items():
        fn = getattr(L, name)         # AttributeError here = the library does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    return list(S.keys())


EXPORTS = []


def lib():
    global _lib, EXPORTS
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SfgError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
        _lib = C.CDLL(LIB_PATH)
        EXPORTS = _sig(_lib)
    return _lib


def p64(a):
    assert a.dtype == np.uint64 and a.flags.c_contiguous
    return a.ctypes.data_as(u64p)


class Context:
    """sfg_ctx wrapper. moduli = q list + p list; psi=None derives lattigo's root."""

    def __init__(self, q, p, scale=2.0 ** 34, logN=14, device=0, psi=None, config=None):
        L = lib()
        self.q, self.p = list(q), list(p)
        self.nq, self.np_ = len(q), len(p)
        self.N, self.slots = 1 << logN, (1 << logN) // 2
        mods = np.array(self.q + self.p, dtype=np.uint64)
        h = C.c_void_p()
        ps = None if psi is None else p64(np.array(psi, dtype=np.uint64))
        if config is None:
            rc = L.sfg_ctx_create(C.byref(h), device, logN, self.nq, self.np_, p64(mods), ps, float(scale))
        else:                                               # config: SfgConfig (include/sfgwas_hip.h: sfg_config)
            rc = L.sfg_ctx_create_ex(C.byref(h), device, logN, self.nq, self.np_, p64(mods), ps, float(scale), C.byref(config))
        if rc:
            raise SfgError("sfg_ctx_create: " + L.sfg_last_error(None).decode())
        self.h = h
        self.beta = (self.nq + self.np_ - 1) // self.np_

    def close(self):
        if getattr(self, "h", None):
            lib().sfg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what):
        if rc:
            raise SfgError(f"{what}: {lib().sfg_last_error(self.h).decode()}")

    # ---- memory
    def malloc(self, nbytes):
        p = C.c_void_p()
        self.check(lib().sfg_malloc(self.h, C.byref(p), nbytes), "sfg_malloc")
        return p

    def free(self, p):
        self.check(lib().sfg_free(self.h, p), "sfg_free")

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        self.check(lib().sfg_memcpy_h2d(self.h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
        return p

    def to_host(self, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self.check(lib().sfg_memcpy_d2h(self.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes), "d2h")
        return out

    def sync(self):
        self.check(lib().sfg_ctx_synchronize(self.h), "sync")

    # ---- ring substrate
    def ntt_rows(self, rows, mod_idx, inverse=False):
        """rows: [nrows][N] uint64 host array; returns transformed copy (round-trips through HBM)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = rows.shape[0]
        mi = (C.c_int * n)(*[int(x) for x in mod_idx])
        d = self.to_device(rows)
        fn = lib().sfg_intt_rows if inverse else lib().sfg_ntt_rows
        self.check(fn(self.h, d, n, mi), "ntt_rows")
        out = self.to_host(d, rows.shape, np.uint64)
        self.free(d)
        return out

    def load_rotkey(self, galois, key, montgomery=False):
        key = np.ascontiguousarray(key, dtype=np.uint64)
        self.check(lib().sfg_ctx_load_rotkey(self.h, int(galois), p64(key), int(montgomery)), "load_rotkey")

    def export_rotkey(self, galois):
        key = np.zeros((self.beta, 2, self.nq + self.np_, self.N), dtype=np.uint64)
        self.check(lib().sfg_ctx_export_rotkey(self.h, int(galois), p64(key)), "export_rotkey")
        return key

    # ---- collective bootstrap, local work
    def load_secret_key(self, sk_rows, montgomery=False):
        sk_rows = np.ascontiguousarray(sk_rows, dtype=np.uint64)
        assert sk_rows.shape == (self.nq, self.N)
        self.check(lib().sfg_ctx_load_secret_key(self.h, p64(sk_rows), int(montgomery)), "load_secret_key")

    def refresh_gen_shares(self, cts, level, crs, mask_limbs, e0, e1, scales=None):
        """cts [nct][2][level+1][N], crs [nct][nq][N], mask_limbs [nct][N][W] uint64, e0/e1 [nct][N] int32 -> (h0 [nct][level+1][N], h1 [nct][nq][N]);
        scales = (ciphertext scale, target scale) selects the target-scale form"""
        nct, W = cts.shape[0], mask_limbs.shape[-1]
        d = [self.to_device(np.ascontiguousarray(a)) for a in (cts, crs, mask_limbs, e0.astype(np.int32), e1.astype(np.int32))]
        h0, h1 = self.malloc(nct * (level + 1) * self.N * 8), self.malloc(nct * self.nq * self.N * 8)
        if scales is None:
            self.check(lib().sfg_refresh_gen_shares_dev(self.h, d[0], nct, level, d[1], d[2], W, d[3], d[4], h0, h1), "refresh_gen_shares")
        else:
            self.check(lib().sfg_refresh_gen_shares_scaled_dev(self.h, d[0], nct, level, float(scales[0]), float(scales[1]), d[1], d[2], W, d[3], d[4], h0, h1),
                       "refresh_gen_shares_scaled")
        out = self.to_host(h0, (nct, level + 1, self.N), np.uint64), self.to_host(h1, (nct, self.nq, self.N), np.uint64)
        for p_ in d + [h0, h1]:
            self.free(p_)
        return out

    def ckks_to_ss_share(self, cts, level, mask_limbs, e0):
        nct, W = cts.shape[0], mask_limbs.shape[-1]
        d = [self.to_device(np.ascontiguousarray(a)) for a in (cts, mask_limbs, e0.astype(np.int32))]
        h0, mk = self.malloc(nct * (level + 1) * self.N * 8), self.malloc(nct * (level + 1) * self.N * 8)
        self.check(lib().sfg_ckks_to_ss_share_dev(self.h, d[0], nct, level, d[1], W, d[2], h0, mk), "ckks_to_ss_share")
        out = self.to_host(h0, (nct, level + 1, self.N), np.uint64), self.to_host(mk, (nct, level + 1, self.N), np.uint64)
        for p_ in d + [h0, mk]:
            self.free(p_)
        return out

    def rvec_encode(self, modulus, shares, level, scale, frac_bits):
        """sfg_rvec_encode_dev: shares uint64 [nct][n_elem][limbs] -> plaintext rows uint64 [nct][level+1][N]"""
        nct, n_elem, limbs = shares.shape
        d_in, o = self.to_device(np.ascontiguousarray(shares, dtype=np.uint64)), self.malloc(nct * (level + 1) * self.N * 8)
        try:
            self.check(lib().sfg_rvec_encode_dev(self.h, limbs, p64(modulus), d_in, n_elem, nct, level, float(scale), frac_bits, o), "rvec_encode")
            return self.to_host(o, (nct, level + 1, self.N), np.uint64)
        finally:
            self.free(d_in)
            self.free(o)

    def rvec_decode(self, modulus, pts, level, scale, frac_bits, n_elem):
        """sfg_rvec_decode_dev: plaintext rows uint64 [nct][>= level+1][N] (the row blocks one pts.shape[1] * N apart) -> field elements uint64 [nct][n_elem][limbs]"""
        nct, limbs = pts.shape[0], len(modulus)
        d_in, o = self.to_device(np.ascontiguousarray(pts, dtype=np.uint64)), self.malloc(nct * n_elem * limbs * 8)
        try:
            self.check(lib().sfg_rvec_decode_dev(self.h, limbs, p64(modulus), d_in, pts.shape[1] * self.N, nct, level, float(scale), frac_bits, n_elem, o), "rvec_decode")
            return self.to_host(o, (nct, n_elem, limbs), np.uint64)
        finally:
            self.free(d_in)
            self.free(o)

    def ckks_to_ss_finish(self, modulus, cts, level, scale, frac_bits, h0agg, mask_ntt, is_hub, n_elem):
        """sfg_ckks_to_ss_finish_dev: the additive share [nct][n_elem][limbs] of this party after the aggregation (cts, h0agg: None off the hub)"""
        nct, limbs = mask_ntt.shape[0], len(modulus)
        d = [None if a is None else self.to_device(np.ascontiguousarray(a, dtype=np.uint64)) for a in (cts, h0agg, mask_ntt)]
        o = self.malloc(nct * n_elem * limbs * 8)
        try:
            self.check(lib().sfg_ckks_to_ss_finish_dev(self.h, limbs, p64(modulus), d[0], nct, level, float(scale), frac_bits, d[1], d[2], 1 if is_hub else 0, n_elem, o),
                       "ckks_to_ss_finish")
            return self.to_host(o, (nct, n_elem, limbs), np.uint64)
        finally:
            for p_ in d + [o]:
                if p_ is not None:
                    self.free(p_)

    def refresh_finish(self, cts, level, h0agg, h1agg, crs, scales=None):
        nct = cts.shape[0]
        d = [self.to_device(np.ascontiguousarray(a)) for a in (cts, h0agg, h1agg, crs)]
        o = self.malloc(nct * 2 * self.nq * self.N * 8)
        if scales is None:
            self.check(lib().sfg_refresh_finish_dev(self.h, d[0], nct, level, d[1], d[2], d[3], o), "refresh_finish")
        else:
            self.check(lib().sfg_refresh_finish_scaled_dev(self.h, d[0], nct, level, float(scales[0]), float(scales[1]), d[1], d[2], d[3], o), "refresh_finish_scaled")
        out = self.to_host(o, (nct, 2, self.nq, self.N), np.uint64)
        for p_ in d + [o]:
            self.free(p_)
        return out

    def fork(self):
        """a second caller on the same tables and keys (sfg_ctx_fork): own queues, scratch and timers"""
        h = C.c_void_p()
        self.check(lib().sfg_ctx_fork(self.h, C.byref(h)), "sfg_ctx_fork")
        child = Context.__new__(Context)
        child.__dict__.update({k: v for k, v in self.__dict__.items()})
        child.h = h
        return child

    def encoder_near_ties(self, reset=False):
        n = C.c_ulonglong()
        self.check(lib().sfg_ctx_encoder_near_ties(self.h, C.byref(n), int(reset)), "encoder_near_ties")
        return n.value

    def galois(self, k):
        return lib().sfg_galois_for_rotation(self.h, k)

    def phase_ms(self, name):
        return lib().sfg_last_phase_ms(self.h, name.encode())


def _ctx_mac(self, rot, pt, L, out_init=None):
    """rot: [K][R][L][N], pt: [K][Ncols][L][N] -> out [Ncols][R][L][N] (host arrays, staged through HBM)."""
    rot = np.ascontiguousarray(rot, dtype=np.uint64)
    pt = np.ascontiguousarray(pt, dtype=np.uint64)
    K, R = rot.shape[0], rot.shape[1]
    Ncols = pt.shape[1]
    assert rot.shape[2] == L and pt.shape[2] == L and pt.shape[0] == K
    d_rot, d_pt = self.to_device(rot), self.to_device(pt)
    if out_init is not None:
        d_out = self.to_device(np.ascontiguousarray(out_init, dtype=np.uint64))
    else:
        d_out = self.malloc(Ncols * R * L * self.N * 8)
    self.check(lib().sfg_mac_dev(self.h, d_rot, d_pt, d_out, K, R, Ncols, L, int(out_init is not None)), "sfg_mac_dev")
    out = self.to_host(d_out, (Ncols, R, L, self.N), np.uint64)
    for p in (d_rot, d_pt, d_out):
        self.free(p)
    return out


Context.mac = _ctx_mac


def _ctx_mac_i8(self, rot, pt_half, L, K=None, out_init=None, pt_form=0):
    """sfg_mac_i8_dev (test hook): the default int8 matrix-core MAC.  rot [P][R][L][N], pt_half [P][Ncols][L][N/2]; with K > P the P k-slices are
    repeated cyclically ON THE DEVICE (k-slice k = slice k mod P) so that long contractions cost one small upload.  Returns out [Ncols][R][L][N]."""
    rot = np.ascontiguousarray(rot, dtype=np.uint64)
    pt_half = np.ascontiguousarray(pt_half, dtype=np.uint64)
    P, R = rot.shape[0], rot.shape[1]
    Ncols = pt_half.shape[1]
    K = P if K is None else K
    assert rot.shape[2] == L and pt_half.shape[2] == L and pt_half.shape[0] == P and pt_half.shape[3] == self.N // 2 and K >= P
    bufs = []
    for arr in (rot, pt_half):
        sl = arr.nbytes // P                                    # bytes per k-slice
        d = self.malloc(sl * K)
        self.check(lib().sfg_memcpy_h2d(self.h, d, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
        filled = P
        while filled < K:
            n = min(filled, K - filled)
            self.check(lib().sfg_memcpy_d2d(self.h, C.c_void_p(d.value + filled * sl), d, n * sl), "d2d")
            filled += n
        bufs.append(d)
    if out_init is not None:
        d_out = self.to_device(np.ascontiguousarray(out_init, dtype=np.uint64))
    else:
        d_out = self.malloc(Ncols * R * L * self.N * 8)
    try:
        self.check(lib().sfg_mac_i8_dev(self.h, bufs[0], bufs[1], d_out, K, R, Ncols, L, int(out_init is not None), pt_form), "sfg_mac_i8_dev")
        out = self.to_host(d_out, (Ncols, R, L, self.N), np.uint64)
    finally:
        for p_ in bufs + [d_out]:
            self.free(p_)
    return out


Context.mac_i8 = _ctx_mac_i8


I8T_GUARD = 4096


def _ctx_i8_move_for_test(self, panel, layout, pt_k, pt_n, K, Ncols, L, mode, a0=0, a1=0, a2=0, no_mover=False, pc=None, sentinel=0xA5):
    """sfg_i8_move_for_test (test hook): the int8 MAC's plaintext transposition through the product's own launches.  panel: the digit-plane panel as host bytes
    (tests/i8tile_ref.py places one); mode 0: the pass, 1: a0 = first, a1 = count, a2 = mover workgroups alone, 2: a0 = predicted NTT launches, a1 = mover
    workgroups, a2 = launches made of 8 plaintexts each, pc [a2 * 8][N/2] doubles.  Returns a dict: on (False: the ride declined and nothing was launched),
    leftover, n5, n6, per, small / big (the tile buffers with their guard bands, uint8; big is None without a six-digit modulus), panel2 (mode 2), panel_after
    (the caller's panel read back)."""
    panel = np.ascontiguousarray(panel, dtype=np.uint8)
    H = self.N // 2
    nch, njt = (K + 63) // 64, (Ncols + 15) // 16
    small_q = [q < (1 << 36) for q in self.q[:L]]
    n_small, n_big = sum(small_q), L - sum(small_q)
    planes = 5 * n_small + 6 * n_big
    small = np.zeros(max(n_small, 1) * H * njt * nch * 5 * 1024 + I8T_GUARD, dtype=np.uint8)
    big = np.zeros(H * njt * nch * 6 * 1024 + I8T_GUARD, dtype=np.uint8) if n_big else None
    panel2 = np.zeros(planes * 64 * 91 * 128, dtype=np.uint8) if mode == 2 else None
    pcp = None
    if mode == 2:
        pc = np.ascontiguousarray(pc, dtype=np.float64)
        assert pc.size >= a2 * 8 * H
        pcp = pc.ctypes.data_as(C.c_void_p)
    info = (C.c_int * 8)()
    d_panel = self.to_device(panel)
    try:
        self.check(lib().sfg_i8_move_for_test(self.h, d_panel, panel.nbytes, layout, pt_k, pt_n, K, Ncols, L, mode, a0, a1, a2, int(no_mover), pcp, sentinel,
                                              small.ctypes.data_as(C.c_void_p), small.nbytes,
                                              None if big is None else big.ctypes.data_as(C.c_void_p), 0 if big is None else big.nbytes,
                                              None if panel2 is None else panel2.ctypes.data_as(C.c_void_p), 0 if panel2 is None else panel2.nbytes, info),
                   "sfg_i8_move_for_test")
        after = self.to_host(d_panel, panel.shape, np.uint8)
    finally:
        self.free(d_panel)
    return dict(on=bool(info[0]), leftover=info[1], n5=info[2], n6=info[3], per=info[4], n_small=info[5], l_small0=info[6], l_big=info[7],
                small=small, big=big, panel2=panel2, panel_after=after)


Context.i8_move_for_test = _ctx_i8_move_for_test


def _ctx_encode_diags(self, block, shift0, nshift, L, transposed=False):
    """block: [r][c] int8 host array (<= slots x slots) -> pt [nshift][L][N] uint64."""
    block = np.ascontiguousarray(block, dtype=np.int8)
    r, c = block.shape
    if transposed:
        r, c = c, r
    d_blk = self.to_device(block)
    d_pt = self.malloc(nshift * L * self.N * 8)
    self.check(lib().sfg_encode_diags_dev(self.h, d_blk, block.shape[1], r, c, int(transposed), shift0, nshift, L, d_pt), "sfg_encode_diags_dev")
    out = self.to_host(d_pt, (nshift, L, self.N), np.uint64)
    self.free(d_blk)
    self.free(d_pt)
    return out


Context.encode_diags = _ctx_encode_diags


def _ctx_rotate_right(self, cts, level, nrots):
    """cts: [nct][2][level+1][N] host array; nrots: list of right-rotation amounts."""
    cts = np.ascontiguousarray(cts, dtype=np.uint64)
    nct = cts.shape[0]
    d_in = self.to_device(cts)
    d_out = self.malloc(cts.nbytes)
    arr = (C.c_int * nct)(*[int(x) for x in nrots])
    self.check(lib().sfg_rotate_right_dev(self.h, d_in, d_out, nct, level, arr), "sfg_rotate_right_dev")
    out = self.to_host(d_out, cts.shape, np.uint64)
    self.free(d_in)
    self.free(d_out)
    return out


Context.rotate_right = _ctx_rotate_right


def _ctx_matmul_stream(self, A, in_level, max_level, geno, flags=0, want_sums=False):
    """MatMult4Stream through the C-ABI with host buffers.
    A: [s][nbr][2][in_level+1][N] uint64, geno: [nrow][ncol] int8 -> (out [s][m_ct][2][max_level][N], sum, sqsum)"""
    A = np.ascontiguousarray(A, dtype=np.uint64)
    geno = np.ascontiguousarray(geno, dtype=np.int8)
    s = A.shape[0]
    nrow, ncol = geno.shape
    lrow, lcol = (ncol, nrow) if flags & SFG_TRANSPOSE else (nrow, ncol)
    nbr, m_ct = (lrow - 1) // self.slots + 1, (lcol - 1) // self.slots + 1
    assert A.shape[1] == nbr, (A.shape, nbr)
    out = np.zeros((s, m_ct, 2, max_level, self.N), dtype=np.uint64)
    sm = np.zeros(ncol) if want_sums else None
    sq = np.zeros(ncol) if want_sums else None
    dp = C.POINTER(C.c_double)
    self.check(lib().sfg_matmul_stream(self.h, p64(A), s, in_level, max_level, geno.ctypes.data_as(C.c_void_p), nrow, ncol, ncol, flags,
                                       p64(out), sm.ctypes.data_as(dp) if want_sums else None, sq.ctypes.data_as(dp) if want_sums else None),
               "sfg_matmul_stream")
    return out, sm, sq


Context.matmul_stream = _ctx_matmul_stream


def random_rotkey(ctx_or_ring_moduli, beta, N, seed):
    """uniform random key words [beta][2][nmod][N] — enough for GPU-vs-oracle parity (which does not need a valid key)"""
    rnd = np.random.default_rng(seed)
    mods = ctx_or_ring_moduli
    k = np.zeros((beta, 2, len(mods), N), dtype=np.uint64)
    for m, q in enumerate(mods):
        k[:, :, m, :] = rnd.integers(0, q, (beta, 2, N), dtype=np.uint64)
    return k


def _ctx_evalop(self, name, level, *arrays, out_level=None, extra=()):
    """run one of the batched evaluator ops (host arrays in, host array out): test plumbing"""
    devs = [self.to_device(np.ascontiguousarray(a, dtype=np.uint64)) for a in arrays]
    nct = arrays[0].shape[0]
    ol_ = level if out_level is None else out_level
    out = self.malloc(nct * 2 * (ol_ + 1) * self.N * 8)
    fn = getattr(lib(), name)
    if name in ("sfg_ct_mul_plain_dev", "sfg_ct_add_plain_dev"):
        self.check(fn(self.h, devs[0], devs[1], extra[0], out, nct, level), name)
    elif name in ("sfg_ct_mul_scalar_dev", "sfg_ct_add_scalar_dev"):
        self.check(fn(self.h, devs[0], p64(np.ascontiguousarray(extra[0], dtype=np.uint64)), out, nct, level), name)
    elif name == "sfg_ct_rescale_dev":
        self.check(fn(self.h, devs[0], out, nct, level), name)
    else:
        self.check(fn(self.h, devs[0], devs[1], out, nct, level), name)
    res = self.to_host(out, (nct, 2, ol_ + 1, self.N), np.uint64)
    for d_ in devs + [out]:
        self.free(d_)
    return res


def _ctx_innersum(self, cts, level):
    cts = np.ascontiguousarray(cts, dtype=np.uint64)
    d_in = self.to_device(cts)
    out = self.malloc(2 * (level + 1) * self.N * 8)
    self.check(lib().sfg_ct_innersum_dev(self.h, d_in, cts.shape[0], level, out), "innersum")
    res = self.to_host(out, (2, level + 1, self.N), np.uint64)
    self.free(d_in); self.free(out)
    return res


def _ctx_load_relinkey(self, key, montgomery=False):
    key = np.ascontiguousarray(key, dtype=np.uint64)
    self.check(lib().sfg_ctx_load_relinkey(self.h, p64(key), int(montgomery)), "load_relinkey")


Context.evalop = _ctx_evalop
Context.innersum = _ctx_innersum
Context.load_relinkey = _ctx_load_relinkey


def _ctx_geno_to_host(self, g):
    nr, nc = C.c_size_t(), C.c_size_t()
    lib().sfg_geno_dims(g, C.byref(nr), C.byref(nc))
    out = np.empty((nr.value, nc.value), dtype=np.int8)
    self.check(lib().sfg_geno_download(self.h, g, out.ctypes.data_as(C.c_void_p)), "geno_download")
    return out


def _ctx_geno_from_bed(self, bed, num_sample, num_snp, row_filter=None, col_filter=None):
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    rf = None if row_filter is None else np.ascontiguousarray(row_filter, dtype=np.uint8)
    cf = None if col_filter is None else np.ascontiguousarray(col_filter, dtype=np.uint8)
    g = C.c_void_p()
    self.check(lib().sfg_geno_from_bed(self.h, bed.ctypes.data_as(C.c_void_p), bed.size, num_sample, num_snp,
                                       None if rf is None else rf.ctypes.data_as(C.c_void_p),
                                       None if cf is None else cf.ctypes.data_as(C.c_void_p), C.byref(g)), "geno_from_bed")
    return g


def _ctx_geno_from_pgen(self, img, v0=0, v1=0, row_filter=None, col_filter=None):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    rf = None if row_filter is None else np.ascontiguousarray(row_filter, dtype=np.uint8)
    cf = None if col_filter is None else np.ascontiguousarray(col_filter, dtype=np.uint8)
    g = C.c_void_p()
    self.check(lib().sfg_geno_from_pgen(self.h, img.ctypes.data_as(C.c_void_p), img.size, v0, v1,
                                        None if rf is None else rf.ctypes.data_as(C.c_void_p),
                                        None if cf is None else cf.ctypes.data_as(C.c_void_p), C.byref(g)), "geno_from_pgen")
    return g


def _ctx_pgen_geno_counts(self, img, row_filter=None):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    ns, nv = C.c_size_t(), C.c_size_t()
    self.check(lib().sfg_pgen_dims(self.h, img.ctypes.data_as(C.c_void_p), img.size, C.byref(ns), C.byref(nv)), "pgen_dims")
    rf = None if row_filter is None else np.ascontiguousarray(row_filter, dtype=np.uint8)
    out = np.empty((6, nv.value), dtype=np.uint32)
    self.check(lib().sfg_pgen_geno_counts(self.h, img.ctypes.data_as(C.c_void_p), img.size, None if rf is None else rf.ctypes.data_as(C.c_void_p),
                                          out.ctypes.data_as(C.c_void_p)), "pgen_geno_counts")
    return out


Context.geno_to_host = _ctx_geno_to_host
Context.geno_from_bed = _ctx_geno_from_bed
Context.geno_from_pgen = _ctx_geno_from_pgen
Context.pgen_geno_counts = _ctx_pgen_geno_counts


def _ctx_encode_vectors(self, values, level):
    values = np.ascontiguousarray(values, dtype=np.float64)
    nvec = values.shape[0]
    out = self.malloc(nvec * (level + 1) * self.N * 8)
    self.check(lib().sfg_encode_vectors_dev(self.h, values.ctypes.data_as(C.POINTER(C.c_double)), nvec, level, out), "encode_vectors")
    res = self.to_host(out, (nvec, level + 1, self.N), np.uint64)
    self.free(out)
    return res


Context.encode_vectors = _ctx_encode_vectors


# ---- public-key encryption on the device (encrypt.hip)
def _ctx_load_public_key(self, pk_rows, montgomery=False):
    """pk_rows [2][nq+np][N] uint64, NTT domain (cryptoParams.Pk.Value)"""
    pk_rows = np.ascontiguousarray(pk_rows, dtype=np.uint64)
    assert pk_rows.shape == (2, self.nq + self.np_, self.N)
    self.check(lib().sfg_ctx_load_public_key(self.h, p64(pk_rows), int(montgomery)), "load_public_key")


def _ctx_has_public_key(self):
    return bool(lib().sfg_ctx_has_public_key(self.h))


def _ctx_seed_encryptor(self, key32):
    """key32: 32 bytes from the caller's CSPRNG; resets the encryption index (shared with every fork) to 0"""
    key32 = bytes(key32)
    if len(key32) != 32:
        raise ValueError("the encryptor key is 32 bytes")
    self.check(lib().sfg_ctx_seed_encryptor(self.h, key32), "seed_encryptor")


def _ctx_encryptor_next_index(self):
    n = C.c_uint64()
    self.check(lib().sfg_ctx_encryptor_next_index(self.h, C.byref(n)), "encryptor_next_index")
    return n.value


def _ctx_encrypt_explicit(self, pt, level, u, e0, e1):
    """the deterministic core: pt None or [nct][level+1][N] uint64, u int8 [nct][N], e0/e1 int32 [nct][N] -> host [nct][2][level+1][N]"""
    u, e0, e1 = (np.ascontiguousarray(u, dtype=np.int8), np.ascontiguousarray(e0, dtype=np.int32), np.ascontiguousarray(e1, dtype=np.int32))
    nct = u.shape[0]
    assert u.shape == e0.shape == e1.shape == (nct, self.N)
    d = [DevArray.from_host(self, a) for a in (u, e0, e1)]
    dpt = None
    if pt is not None:
        pt = np.ascontiguousarray(pt, dtype=np.uint64)
        assert pt.shape == (nct, level + 1, self.N)
        dpt = DevArray.from_host(self, pt)
    out = DevArray(self, (nct, 2, level + 1, self.N))
    try:
        self.check(lib().sfg_encrypt_explicit_dev(self.h, None if dpt is None else dpt.p, nct, level, d[0].p, d[1].p, d[2].p, out.p), "encrypt_explicit")
        return out.host()
    finally:
        for a in d + [out] + ([dpt] if dpt is not None else []):
            a.free()


def _ctx_add_fresh_zero(self, ct_dev, level):
    """ct_dev: DevArray [...][2][level+1][N]; every ciphertext += a fresh encryption of zero, in place"""
    nct = int(np.prod(ct_dev.shape[:-3])) if len(ct_dev.shape) > 3 else 1
    assert ct_dev.shape[-3:] == (2, level + 1, self.N)
    self.check(lib().sfg_ct_add_fresh_zero_dev(self.h, ct_dev.p, nct, level), "add_fresh_zero")
    return ct_dev


def _ctx_encrypt_vectors(self, values, level):
    """values [nct][slots] float64 -> DevArray [nct][2][level+1][N] (EncryptFloatVector)"""
    values = np.ascontiguousarray(values, dtype=np.float64)
    nct = values.shape[0]
    out = DevArray(self, (max(nct, 1), 2, level + 1, self.N))
    rc = lib().sfg_encrypt_vectors_dev(self.h, values.ctypes.data_as(C.POINTER(C.c_double)), nct, level, out.p)
    if rc:
        out.free()
    self.check(rc, "encrypt_vectors")
    return out


def _ctx_encrypt_transcript(self, first_index, nct):
    """test hook: (u int8, e0 int32, e1 int32), each [nct][N], of the given encryption indices; the counter does not move"""
    d = [DevArray(self, (max(nct, 1), self.N), t) for t in (np.int8, np.int32, np.int32)]
    try:
        self.check(lib().sfg_encrypt_transcript_for_test(self.h, int(first_index), nct, d[0].p, d[1].p, d[2].p), "encrypt_transcript")
        return tuple(a.host() for a in d)
    finally:
        for a in d:
            a.free()


Context.load_public_key = _ctx_load_public_key
Context.has_public_key = _ctx_has_public_key
Context.seed_encryptor = _ctx_seed_encryptor
Context.encryptor_next_index = _ctx_encryptor_next_index
Context.encrypt_explicit = _ctx_encrypt_explicit
Context.add_fresh_zero = _ctx_add_fresh_zero
Context.encrypt_vectors = _ctx_encrypt_vectors
Context.encrypt_transcript = _ctx_encrypt_transcript


# ---- collective decryption and decoding on the device (decrypt.hip)
def _dev_ptr(self, a, dtype, shape=None):
    """(pointer, DevArray to free or None): a DevArray is used in place, a host array is uploaded"""
    if isinstance(a, DevArray):
        return a.p, None
    a = np.ascontiguousarray(a, dtype=dtype)
    assert shape is None or a.shape == shape, (a.shape, shape)
    d = DevArray.from_host(self, a)
    return d.p, d


def _ctx_pcks_gen_share(self, cts, level, e0, e1=None):
    """cts [nct][2][level+1][N] (DevArray or host), e0 / e1 int32 [nct][N] -> host (h0, h1) [nct][level+1][N]; e1 None: h1 is not computed (None)"""
    nct = int(cts.shape[0])
    keep = []
    try:
        pc, t = _dev_ptr(self, cts, np.uint64, (nct, 2, level + 1, self.N)); keep.append(t)
        p0, t = _dev_ptr(self, e0, np.int32, (nct, self.N)); keep.append(t)
        p1 = None
        if e1 is not None:
            p1, t = _dev_ptr(self, e1, np.int32, (nct, self.N)); keep.append(t)
        h0 = DevArray(self, (nct, level + 1, self.N)); keep.append(h0)
        h1 = None
        if e1 is not None:
            h1 = DevArray(self, (nct, level + 1, self.N)); keep.append(h1)
        self.check(lib().sfg_pcks_gen_share_dev(self.h, pc, nct, level, p0, p1, h0.p, None if h1 is None else h1.p), "pcks_gen_share")
        return h0.host(), (None if h1 is None else h1.host())
    finally:
        for a in keep:
            if a is not None:
                a.free()


def _ctx_pcks_finish(self, cts, level, h0agg, scale=None, want_imag=False):
    """scale None: the plaintext rows [nct][level+1][N] (host); else the fused finish + decode: real parts [nct][slots] (and the imaginary parts)"""
    nct = int(cts.shape[0])
    keep = []
    try:
        pc, t = _dev_ptr(self, cts, np.uint64, (nct, 2, level + 1, self.N)); keep.append(t)
        ph, t = _dev_ptr(self, h0agg, np.uint64, (nct, level + 1, self.N)); keep.append(t)
        if scale is None:
            pt = DevArray(self, (nct, level + 1, self.N)); keep.append(pt)
            self.check(lib().sfg_pcks_finish_dev(self.h, pc, nct, level, ph, pt.p), "pcks_finish")
            return pt.host()
        re = np.empty((nct, self.slots)); im = np.empty((nct, self.slots)) if want_imag else None
        self.check(lib().sfg_pcks_finish_decode(self.h, pc, nct, level, float(scale), ph, re.ctypes.data_as(C.c_void_p),
                                                None if im is None else im.ctypes.data_as(C.c_void_p)), "pcks_finish_decode")
        return (re, im) if want_imag else re
    finally:
        for a in keep:
            if a is not None:
                a.free()


def _ctx_decode_vectors(self, pt, level, scale, want_imag=False, stride=None):
    """pt: DevArray or host rows; [nct][level+1][N] plaintexts, or (stride = 2 (level+1) N) ciphertexts whose polynomial 0 is read in place"""
    nct = int(pt.shape[0])
    p, t = _dev_ptr(self, pt, np.uint64)
    try:
        re = np.empty((nct, self.slots)); im = np.empty((nct, self.slots)) if want_imag else None
        self.check(lib().sfg_decode_vectors(self.h, p, (level + 1) * self.N if stride is None else int(stride), nct, level, float(scale),
                                            re.ctypes.data_as(C.c_void_p), None if im is None else im.ctypes.data_as(C.c_void_p)), "decode_vectors")
        return (re, im) if want_imag else re
    finally:
        if t is not None:
            t.free()


def _ctx_decode_coeffs(self, pt, level, scale, stride=None):
    nct = int(pt.shape[0])
    p, t = _dev_ptr(self, pt, np.uint64)
    try:
        out = np.empty((nct, self.N))
        self.check(lib().sfg_decode_coeffs(self.h, p, (level + 1) * self.N if stride is None else int(stride), nct, level, float(scale),
                                           out.ctypes.data_as(C.c_void_p)), "decode_coeffs")
        return out
    finally:
        if t is not None:
            t.free()


def _ctx_decrypt_vectors(self, cts, level, scale, want_imag=False):
    """cts [nct][2][level+1][N] (DevArray or host) under the loaded secret key -> real parts [nct][slots] (and the imaginary parts)"""
    nct = int(np.prod(cts.shape[:-3]))
    p, t = _dev_ptr(self, cts, np.uint64)
    try:
        re = np.empty((nct, self.slots)); im = np.empty((nct, self.slots)) if want_imag else None
        self.check(lib().sfg_decrypt_vectors(self.h, p, nct, level, float(scale), re.ctypes.data_as(C.c_void_p),
                                             None if im is None else im.ctypes.data_as(C.c_void_p)), "decrypt_vectors")
        return (re, im) if want_imag else re
    finally:
        if t is not None:
            t.free()


Context.pcks_gen_share = _ctx_pcks_gen_share
Context.pcks_finish = _ctx_pcks_finish
Context.decode_vectors = _ctx_decode_vectors
Context.decode_coeffs = _ctx_decode_coeffs
Context.decrypt_vectors = _ctx_decrypt_vectors


# ---- resident products (device-level plumbing for the tests and bench.py)
class DevArray:
    """a device buffer with a numpy-like shape (uint64 words unless dtype says otherwise); freed with .free()"""

    def __init__(self, ctx, shape, dtype=np.uint64):
        self.ctx, self.shape, self.dtype = ctx, tuple(int(x) for x in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.p = ctx.malloc(max(self.nbytes, 8))

    @classmethod
    def from_host(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        d = cls(ctx, arr.shape, arr.dtype)
        ctx.check(lib().sfg_memcpy_h2d(ctx.h, d.p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
        return d

    def host(self):
        return self.ctx.to_host(self.p, self.shape, self.dtype)

    def host_slice(self, index):
        """download self[index] for a leading-axis integer index (or tuple of leading indices)"""
        index = index if isinstance(index, tuple) else (index,)
        sub = self.shape[len(index):]
        off = 0
        for k, i in enumerate(index):
            off += int(i) * int(np.prod(self.shape[k + 1:]))
        out = np.empty(sub, dtype=self.dtype)
        src = C.c_void_p(self.p.value + off * self.dtype.itemsize)
        self.ctx.check(lib().sfg_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), src, out.nbytes), "d2h")
        return out

    def free(self):
        if self.p is not None:
            self.ctx.free(self.p)
            self.p = None


def _ctx_geno_upload(self, geno):
    geno = np.ascontiguousarray(geno, dtype=np.int8)
    g = C.c_void_p()
    self.check(lib().sfg_geno_upload(self.h, geno.ctypes.data_as(C.c_void_p), geno.shape[0], geno.shape[1], geno.shape[1], C.byref(g)), "geno_upload")
    return g


def _ctx_geno_free(self, g):
    lib().sfg_geno_free(self.h, g)


def _ctx_geno_create(self, nrow, ncol):
    g = C.c_void_p()
    self.check(lib().sfg_geno_create(self.h, nrow, ncol, C.byref(g)), "geno_create")
    return g


def _ctx_geno_write_rows(self, g, row0, rows, ld=None):
    """rows: int8 [nrows][>= ncol] (a C-contiguous chunk of whole rows; ld = its row stride)"""
    rows = np.ascontiguousarray(rows, dtype=np.int8)
    self.check(lib().sfg_geno_write_rows(self.h, g, row0, rows.shape[0], rows.ctypes.data_as(C.c_void_p), ld or rows.shape[1]), "geno_write_rows")


def _ctx_geno_compare_rows(self, g, flags, row0, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int8)
    nd = np.zeros(1, dtype=np.uint64)
    self.check(lib().sfg_geno_compare_rows(self.h, g, flags, row0, rows.shape[0], rows.ctypes.data_as(C.c_void_p), rows.shape[1], p64(nd)), "geno_compare_rows")
    return int(nd[0])


def _ctx_fill_uniform_cts(self, nct, level, seed):
    d = DevArray(self, (nct, 2, level + 1, self.N))
    self.check(lib().sfg_fill_uniform_ct_dev(self.h, d.p, nct, level, seed), "fill_uniform_ct")
    return d


def _ctx_fill_geno(self, nrow, ncol, seed):
    d = DevArray(self, (nrow, ncol), np.int8)
    self.check(lib().sfg_fill_geno_dev(self.h, d.p, nrow, ncol, seed), "fill_geno")
    g = C.c_void_p()
    self.check(lib().sfg_geno_from_device(self.h, d.p, nrow, ncol, ncol, C.byref(g)), "geno_from_device")
    return d, g


def _ctx_matmul_resident(self, A_dev, s, in_level, max_level, g, flags=0, blk=None):
    """A_dev: DevArray [s][nbr][2][in_level+1][N]; returns DevArray out [s][m_out][2][max_level][N]"""
    nr, nc = C.c_size_t(), C.c_size_t()
    lib().sfg_geno_dims(g, C.byref(nr), C.byref(nc))
    lcol = nr.value if flags & SFG_TRANSPOSE else nc.value
    m_ct = (lcol - 1) // self.slots + 1
    if blk is None:
        out = DevArray(self, (s, m_ct, 2, max_level, self.N))
        self.check(lib().sfg_matmul_resident_dev(self.h, A_dev.p, s, in_level, max_level, g, flags, out.p), "matmul_resident")
    else:
        m_out = m_ct if flags & SFG_TRANSPOSE else blk[1] - blk[0]
        out = DevArray(self, (s, m_out, 2, max_level, self.N))
        self.check(lib().sfg_matmul_resident_range_dev(self.h, A_dev.p, s, in_level, max_level, g, flags, blk[0], blk[1], out.p), "matmul_resident_range")
    return out


def _ctx_matmul_accumulate(self, A_dev, s, in_level, max_level, g, flags, b0, b1, j0, j1, acc=None):
    d = 91
    accumulate = acc is not None
    if acc is None:
        acc = DevArray(self, (j1 - j0, d, s, 2, max_level, self.N))
    self.check(lib().sfg_matmul_accumulate_dev(self.h, A_dev.p, s, in_level, max_level, g, flags, b0, b1, j0, j1, int(accumulate), acc.p), "matmul_accumulate")
    return acc


def _ctx_matmul_finalize(self, acc, s, max_level, ncolb, g0, g1, out=None):
    accumulate = out is not None
    if out is None:
        out = DevArray(self, (s, ncolb, 2, max_level, self.N))
    self.check(lib().sfg_matmul_finalize_dev(self.h, acc.p, s, max_level, ncolb, g0, g1, int(accumulate), out.p), "matmul_finalize")
    return out


# ---- the baby-step rotation cache as an object (sfg_rotcache_*, the *_rc_dev products): fp64 operand rows in caller-held DevArrays of float64
def _ctx_rotcache_layout(self, s, max_level):
    """(job_doubles, tail_doubles): doubles of one job's 91 rotations [91][2][rowf], of the zero tail [3][s][2][rowf]"""
    jw, tw = C.c_size_t(), C.c_size_t()
    self.check(lib().sfg_rotcache_layout(self.h, s, max_level, C.byref(jw), C.byref(tw)), "rotcache_layout")
    return jw.value, tw.value


def _f64_at(d, at):
    return C.c_void_p(d.p.value + int(at) * 8) if d is not None else None


def _rc_call(self, what, fn, out, made, *args):
    rc = fn(*args)
    if rc and made:
        out.free()
    self.check(rc, what)
    return out


def _ctx_rotcache_build_jobs(self, A_dev, s, in_level, max_level, nbr, job0, job1, staged=None, at=0):
    """A_dev: DevArray [s][nbr][2][in_level+1][N].  Jobs [job0, job1) (job = block row * s + i) land job-major, [job - job0][91][2][rowf], from double `at`
    of `staged` (a float64 DevArray; None: one of exactly that size is made).  Returns staged."""
    made = staged is None
    if made:
        staged = DevArray(self, ((job1 - job0) * self.rotcache_layout(s, max_level)[0],), np.float64)
    return _rc_call(self, "rotcache_build_jobs", lib().sfg_rotcache_build_jobs_dev, staged, made,
                    self.h, A_dev.p, s, in_level, max_level, nbr, job0, job1, _f64_at(staged, at))


def _ctx_rotcache_scatter(self, staged, s, max_level, job0, job1, row0, nrows, cache=None, at=0):
    """staged (from double `at` on): jobs [job0, job1) job-major -> cache [nrows][91][s][2][rowf] of block rows [row0, row0 + nrows) + the zero tail.  Returns cache."""
    made = cache is None
    if made:
        jw, tw = self.rotcache_layout(s, max_level)
        cache = DevArray(self, (nrows * s * jw + tw,), np.float64)
    return _rc_call(self, "rotcache_scatter", lib().sfg_rotcache_scatter_dev, cache, made,
                    self.h, _f64_at(staged, at), s, max_level, job0, job1, row0, nrows, cache.p)


def _ctx_rotcache_build_rows(self, A_dev, s, in_level, max_level, nbr, b0, b1, cache=None):
    """cache [b1 - b0][91][s][2][rowf] of block rows [b0, b1) of A_dev + the zero tail, built in place.  Returns cache."""
    made = cache is None
    if made:
        jw, tw = self.rotcache_layout(s, max_level)
        cache = DevArray(self, ((b1 - b0) * s * jw + tw,), np.float64)
    return _rc_call(self, "rotcache_build_rows", lib().sfg_rotcache_build_rows_dev, cache, made,
                    self.h, A_dev.p, s, in_level, max_level, nbr, b0, b1, cache.p)


def _ctx_rotcache_invalidate(self):
    self.check(lib().sfg_rotcache_invalidate(self.h), "rotcache_invalidate")


def _ctx_matmul_resident_range_rc(self, cache, s, max_level, g, flags, blk0, blk1, out=None):
    """the product of matmul_resident(blk=(blk0, blk1)) on a prebuilt cache of the operand block rows it contracts over; cache None passes a null pointer"""
    nr, nc = C.c_size_t(), C.c_size_t()
    lib().sfg_geno_dims(g, C.byref(nr), C.byref(nc))
    m_out = (nr.value - 1) // self.slots + 1 if flags & SFG_TRANSPOSE else blk1 - blk0
    made = out is None
    if made:
        out = DevArray(self, (s, m_out, 2, max_level, self.N))
    return _rc_call(self, "matmul_resident_range_rc", lib().sfg_matmul_resident_range_rc_dev, out, made,
                    self.h, cache.p if cache is not None else None, s, max_level, g, flags, blk0, blk1, out.p)


def _ctx_matmul_accumulate_rc(self, cache, s, max_level, g, flags, b0, b1, j0, j1, acc=None):
    """matmul_accumulate on a prebuilt cache of block rows [b0, b1); acc given: accumulated onto"""
    accumulate = acc is not None
    if acc is None:
        acc = DevArray(self, (j1 - j0, 91, s, 2, max_level, self.N))
    return _rc_call(self, "matmul_accumulate_rc", lib().sfg_matmul_accumulate_rc_dev, acc, not accumulate,
                    self.h, cache.p if cache is not None else None, s, max_level, g, flags, b0, b1, j0, j1, int(accumulate), acc.p)


Context.rotcache_layout = _ctx_rotcache_layout
Context.rotcache_build_jobs = _ctx_rotcache_build_jobs
Context.rotcache_scatter = _ctx_rotcache_scatter
Context.rotcache_build_rows = _ctx_rotcache_build_rows
Context.rotcache_invalidate = _ctx_rotcache_invalidate
Context.matmul_resident_range_rc = _ctx_matmul_resident_range_rc
Context.matmul_accumulate_rc = _ctx_matmul_accumulate_rc


def _filter_arg(f, n, what):
    """a row / column filter or cohort mask as the uint8 array the library reads (None stays None)"""
    if f is None:
        return None, None
    f = np.ascontiguousarray(np.asarray(f) != 0, dtype=np.uint8)
    if f.shape != (n,):
        raise ValueError(f"{what}: expected {n} entries, got {f.shape}")
    return f, f.ctypes.data_as(C.c_void_p)


def _qc_scan(check, fn, h, g, nrow, ncol, row_filter, col_filter, row_ctrl, cols, rows):
    rf, prf = _filter_arg(row_filter, nrow, "row_filter")
    cf, pcf = _filter_arg(col_filter, ncol, "col_filter")
    rc, prc = _filter_arg(row_ctrl, nrow, "row_ctrl")
    cc = np.empty((2, 4, ncol), dtype=np.uint32) if cols else None
    rm = np.empty(nrow, dtype=np.uint32) if rows else None
    rh = np.empty(nrow, dtype=np.uint32) if rows else None
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    check(fn(h, g, prf, pcf, prc, ptr(cc), ptr(rm), ptr(rh)), "geno_qc_scan")
    return cc, rm, rh


def _ctx_geno_qc_scan(self, g, row_filter=None, col_filter=None, row_ctrl=None, cols=True, rows=True):
    """one pass over a resident matrix (sfg_geno_qc_scan): (col_counts [2][4][ncol], row_miss [nrow], row_het [nrow]) as uint32; cols / rows = False leaves that
    output out (None is returned in its place)"""
    nr, nc = C.c_size_t(), C.c_size_t()
    lib().sfg_geno_dims(g, C.byref(nr), C.byref(nc))
    return _qc_scan(self.check, lib().sfg_geno_qc_scan, self.h, g, nr.value, nc.value, row_filter, col_filter, row_ctrl, cols, rows)


def _ctx_geno_filter(self, g, row_filter=None, col_filter=None):
    """the kept rows / columns of a resident matrix as a new resident handle of the same layout (sfg_geno_filter)"""
    nr, nc = C.c_size_t(), C.c_size_t()
    lib().sfg_geno_dims(g, C.byref(nr), C.byref(nc))
    rf, prf = _filter_arg(row_filter, nr.value, "row_filter")
    cf, pcf = _filter_arg(col_filter, nc.value, "col_filter")
    out = C.c_void_p()
    self.check(lib().sfg_geno_filter(self.h, g, prf, pcf, C.byref(out)), "geno_filter")
    return out


def _sketch(check, fn, h, g, nrow, ncol, bucket, sgn, kp, sketch, sums):
    """sfg_sketch / sfg_mgpu_sketch: (sketch [kp][ncol] fp64, xsum [ncol], x2sum [ncol] uint64); sketch / sums = False leaves that output out (None in its place)"""
    bucket, sgn = np.ascontiguousarray(bucket, dtype=np.int32), np.ascontiguousarray(sgn, dtype=np.int8)
    if bucket.shape != (nrow,) or sgn.shape != (nrow,):
        raise ValueError(f"sketch: expected {nrow} buckets and signs")
    sk = np.empty((kp, ncol), dtype=np.float64) if sketch else None
    xs = np.empty(ncol, dtype=np.uint64) if sums else None
    x2 = np.empty(ncol, dtype=np.uint64) if sums else None
    check(fn(h, g, bucket.ctypes.data_as(C.POINTER(C.c_int32)), sgn.ctypes.data_as(C.POINTER(C.c_int8)), kp,
             None if sk is None else sk.ctypes.data_as(C.POINTER(C.c_double)), None if xs is None else p64(xs), None if x2 is None else p64(x2)), "sketch")
    return sk, xs, x2


def _colsums(check, fn, h, g, ncol, sums, sqsums):
    """sfg_geno_colsums / sfg_mgpu_geno_colsums: (sum [ncol], sqsum [ncol]) as fp64 after missing -> 0"""
    a = np.empty(ncol, dtype=np.float64) if sums else None
    b = np.empty(ncol, dtype=np.float64) if sqsums else None
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    check(fn(h, g, ptr(a), ptr(b)), "geno_colsums")
    return a, b


def _ctx_sketch(self, g, bucket, sgn, kp, sketch=True, sums=True):
    nr, nc = C.c_size_t(), C.c_size_t()
    lib().sfg_geno_dims(g, C.byref(nr), C.byref(nc))
    return _sketch(self.check, lib().sfg_sketch, self.h, g, nr.value, nc.value, bucket, sgn, kp, sketch, sums)


def _ctx_geno_colsums(self, g, sums=True, sqsums=True):
    nr, nc = C.c_size_t(), C.c_size_t()
    lib().sfg_geno_dims(g, C.byref(nr), C.byref(nc))
    return _colsums(self.check, lib().sfg_geno_colsums, self.h, g, nc.value, sums, sqsums)


def geno_layout(g):
    """(device address, row stride in bytes, packed) of a resident handle (sfg_geno_layout)"""
    dev, ld, pk = C.c_void_p(), C.c_size_t(), C.c_int()
    if lib().sfg_geno_layout(g, C.byref(dev), C.byref(ld), C.byref(pk)):
        raise SfgError("geno_layout: null matrix")
    return dev.value, ld.value, bool(pk.value)


Context.sketch = _ctx_sketch
Context.geno_colsums = _ctx_geno_colsums
Context.geno_qc_scan = _ctx_geno_qc_scan
Context.geno_filter = _ctx_geno_filter
Context.geno_upload = _ctx_geno_upload
Context.geno_free = _ctx_geno_free
Context.geno_create = _ctx_geno_create
Context.geno_write_rows = _ctx_geno_write_rows
Context.geno_compare_rows = _ctx_geno_compare_rows
Context.fill_uniform_cts = _ctx_fill_uniform_cts
Context.fill_geno = _ctx_fill_geno
Context.matmul_resident = _ctx_matmul_resident
Context.matmul_accumulate = _ctx_matmul_accumulate
Context.matmul_finalize = _ctx_matmul_finalize


# ---- the multi-GPU engine (sfg_mgpu_*, mgpu.hip); plumbing for the tests and bench.py
class MultiGpu:
    """sfg_mgpu wrapper.  devices = [0, 1, ...] makes a single-process engine (one rank per entry; a repeated device selects the in-process `direct` transport);
    rank / world / uid join a multi-process world (one rank per process)."""

    def __init__(self, q, p, devices=None, scale=2.0 ** 34, logN=14, rank=None, world=None, uid=None, device=0, config=None):
        L = lib()
        self.q, self.p = list(q), list(p)
        self.nq, self.np_ = len(q), len(p)
        self.N, self.slots = 1 << logN, (1 << logN) // 2
        mods = np.array(self.q + self.p, dtype=np.uint64)
        h = C.c_void_p()
        cfgp = None if config is None else C.byref(config)
        if uid is None:
            devs = (C.c_int * len(devices))(*devices)
            rc = L.sfg_mgpu_create_ex(C.byref(h), devs, len(devices), logN, self.nq, self.np_, p64(mods), None, float(scale), cfgp)
        else:
            buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
            rc = L.sfg_mgpu_create_rank_ex(C.byref(h), device, rank, world, buf, logN, self.nq, self.np_, p64(mods), None, float(scale), cfgp)
        if rc:
            raise SfgError("sfg_mgpu_create: " + L.sfg_mgpu_last_error(None).decode())
        self.h = h
        self.world, self.nlocal = L.sfg_mgpu_world(h), L.sfg_mgpu_nlocal(h)
        self.transport = L.sfg_mgpu_transport(h).decode()
        self.ctx = []
        for i in range(self.nlocal):                        # borrowed contexts (owned by the engine): for device buffers and phase timers
            c = Context.__new__(Context)
            c.__dict__.update(q=self.q, p=self.p, nq=self.nq, np_=self.np_, N=self.N, slots=self.slots, beta=(self.nq + self.np_ - 1) // self.np_)
            c.h = C.c_void_p(L.sfg_mgpu_ctx(h, i))
            c.close = lambda: None
            self.ctx.append(c)
        self.ranks = [L.sfg_mgpu_rank(h, i) for i in range(self.nlocal)]

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        if lib().sfg_mgpu_unique_id(buf):
            raise SfgError("sfg_mgpu_unique_id: " + lib().sfg_mgpu_last_error(None).decode())
        return bytes(buf)

    def check(self, rc, what):
        if rc:
            raise SfgError(f"{what}: {lib().sfg_mgpu_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            for c in self.ctx:
                c.h = None
            lib().sfg_mgpu_destroy(self.h)
            self.h = None

    def sync(self):
        self.check(lib().sfg_mgpu_synchronize(self.h), "sfg_mgpu_synchronize")

    def fill_rotkeys_synthetic(self, rots_left, seed):
        arr = (C.c_int * len(rots_left))(*rots_left)
        self.check(lib().sfg_mgpu_fill_rotkeys_synthetic(self.h, arr, len(rots_left), seed), "sfg_mgpu_fill_rotkeys_synthetic")

    def load_rotkey(self, galois, key, montgomery=False):
        key = np.ascontiguousarray(key, dtype=np.uint64)
        self.check(lib().sfg_mgpu_load_rotkey(self.h, int(galois), p64(key), int(montgomery)), "sfg_mgpu_load_rotkey")

    def geno_upload(self, geno):
        geno = np.ascontiguousarray(geno, dtype=np.int8)
        g = C.c_void_p()
        self.check(lib().sfg_mgpu_geno_upload(self.h, geno.ctypes.data_as(C.c_void_p), geno.shape[0], geno.shape[1], geno.shape[1], C.byref(g)), "sfg_mgpu_geno_upload")
        return g

    def geno_create(self, nrow, ncol):
        g = C.c_void_p()
        self.check(lib().sfg_mgpu_geno_create(self.h, nrow, ncol, C.byref(g)), "sfg_mgpu_geno_create")
        return g

    def geno_write_rows(self, g, row0, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int8)
        self.check(lib().sfg_mgpu_geno_write_rows(self.h, g, row0, rows.shape[0], rows.ctypes.data_as(C.c_void_p), rows.shape[1]), "sfg_mgpu_geno_write_rows")

    def geno_compare_rows(self, g, flags, row0, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int8)
        nd = np.zeros(1, dtype=np.uint64)
        self.check(lib().sfg_mgpu_geno_compare_rows(self.h, g, flags, row0, rows.shape[0], rows.ctypes.data_as(C.c_void_p), rows.shape[1], p64(nd)), "sfg_mgpu_geno_compare_rows")
        return int(nd[0])

    def preflight(self, count_per_rank=4096):
        self.check(lib().sfg_mgpu_preflight(self.h, count_per_rank), "sfg_mgpu_preflight")

    def comm_info(self, local=0):
        n, r = C.c_int(), C.c_int()
        self.check(lib().sfg_mgpu_comm_info(self.h, local, C.byref(n), C.byref(r)), "sfg_mgpu_comm_info")
        return n.value, r.value

    def geno_synthetic(self, nrow, ncol, seed, packed=False):
        g = C.c_void_p()
        self.check(lib().sfg_mgpu_geno_synthetic(self.h, nrow, ncol, seed, int(packed), C.byref(g)), "sfg_mgpu_geno_synthetic")
        return g

    def geno_free(self, g):
        lib().sfg_mgpu_geno_free(self.h, g)

    def geno_qc_scan(self, g, row_filter=None, col_filter=None, row_ctrl=None, cols=True, rows=True):
        """Context.geno_qc_scan on the sharded matrix (sfg_mgpu_geno_qc_scan): filters and outputs span the whole matrix; the row counts are those of this
        process's ranks"""
        nr, nc = C.c_size_t(), C.c_size_t()
        lib().sfg_mgpu_geno_dims(g, C.byref(nr), C.byref(nc))
        return _qc_scan(self.check, lib().sfg_mgpu_geno_qc_scan, self.h, g, nr.value, nc.value, row_filter, col_filter, row_ctrl, cols, rows)

    def geno_dims(self, g):
        nr, nc = C.c_size_t(), C.c_size_t()
        lib().sfg_mgpu_geno_dims(g, C.byref(nr), C.byref(nc))
        return nr.value, nc.value

    def geno_shard(self, g, local):
        """the borrowed handle of local rank `local`'s window on self.ctx[local] (None: the rank owns no block)"""
        h = lib().sfg_mgpu_geno_shard(g, local)
        return C.c_void_p(h) if h else None

    def geno_filter(self, g, row_filter=None, col_filter=None):
        """the kept rows / columns of a sharded matrix as a new sharded matrix over the kept columns (sfg_mgpu_geno_filter: re-sharding, single process only)"""
        nr, nc = (0, 0) if g is None else self.geno_dims(g)
        rf, prf = _filter_arg(row_filter, nr, "row_filter")
        cf, pcf = _filter_arg(col_filter, nc, "col_filter")
        out = C.c_void_p()
        self.check(lib().sfg_mgpu_geno_filter(self.h, g, prf, pcf, C.byref(out)), "sfg_mgpu_geno_filter")
        return out

    def sketch(self, g, bucket, sgn, kp, sketch=True, sums=True):
        """Context.sketch on the sharded matrix (sfg_mgpu_sketch): outputs in the global column layout"""
        nr, nc = self.geno_dims(g)
        return _sketch(self.check, lib().sfg_mgpu_sketch, self.h, g, nr, nc, bucket, sgn, kp, sketch, sums)

    def geno_colsums(self, g, sums=True, sqsums=True):
        """Context.geno_colsums on the sharded matrix (sfg_mgpu_geno_colsums): outputs in the global column layout"""
        return _colsums(self.check, lib().sfg_mgpu_geno_colsums, self.h, g, self.geno_dims(g)[1], sums, sqsums)

    def geno_blocks(self, g, local):
        b0, b1 = C.c_size_t(), C.c_size_t()
        lib().sfg_mgpu_geno_blocks(g, local, C.byref(b0), C.byref(b1))
        return b0.value, b1.value

    def matmul_dev(self, A, s, in_level, max_level, g, flags, out):
        """A / out: lists of DevArray, one per local rank"""
        n = self.nlocal
        pa = (C.c_void_p * n)(*[a.p for a in A])
        po = (C.c_void_p * n)(*[o.p for o in out])
        self.check(lib().sfg_mgpu_matmul_dev(self.h, pa, s, in_level, max_level, g, flags, po), "sfg_mgpu_matmul_dev")

    def inject_failure_for_test(self, local, phase):
        """test hook (SFG_ENABLE_TEST_HOOKS=1 before the engine was made): local rank `local` fails once in the next exchanging Q'X^T call; phase 0 = I/O pass, 1 = prepare"""
        self.check(lib().sfg_mgpu_inject_failure_for_test(self.h, local, phase), "sfg_mgpu_inject_failure_for_test")

    def matmul(self, A_host, s, in_level, max_level, g, flags=0):
        """host form: A_host [s][nbr or m_ct][2][in_level+1][N] -> out [s][m_ct or nbr][2][max_level][N]"""
        A_host = np.ascontiguousarray(A_host, dtype=np.uint64)
        nr, nc = C.c_size_t(), C.c_size_t()
        lib().sfg_mgpu_geno_dims(g, C.byref(nr), C.byref(nc))
        ncols = ((nr.value if flags & SFG_TRANSPOSE else nc.value) - 1) // self.slots + 1
        out = np.zeros((s, ncols, 2, max_level, self.N), dtype=np.uint64)
        self.check(lib().sfg_mgpu_matmul(self.h, p64(A_host), s, in_level, max_level, g, flags, p64(out)), "sfg_mgpu_matmul")
        return out


# ---- collective key generation on the device (keygen.hip).  Every polynomial argument is a DevArray (used in place) or a host array (uploaded); results are
# DevArrays the caller frees.  nmod = nq + np rows per polynomial.
def _kg_call(self, what, fn, ins, outs):
    """ins: [(array, dtype, shape)] -> device pointers; outs: [shape] -> fresh DevArrays; fn(*in pointers, *out pointers) -> rc"""
    keep, res = [], []
    try:
        ptrs = []
        for a, dt, shp in ins:
            ptr, tmp = _dev_ptr(self, a, dt, None if isinstance(a, DevArray) else shp); keep.append(tmp); ptrs.append(ptr)
        res = [DevArray(self, s) for s in outs]
        rc = fn(*ptrs, *[o.p for o in res])
        if rc:
            for o in res:
                o.free()
        self.check(rc, what)
        return res
    finally:
        for a in keep:
            if a is not None:
                a.free()


def _galois_arr(galois):
    g = np.ascontiguousarray(galois, dtype=np.uint64)
    return g, (p64(g) if g.size else None)


def _ctx_load_secret_key_qp(self, sk_rows, montgomery=False):
    sk_rows = np.ascontiguousarray(sk_rows, dtype=np.uint64)
    assert sk_rows.shape == (self.nq + self.np_, self.N)
    self.check(lib().sfg_ctx_load_secret_key_qp(self.h, p64(sk_rows), int(montgomery)), "load_secret_key_qp")


def _ctx_ckg_gen_share(self, crp, e=None):
    """crp [nmod][N]; e int32 [N] (the explicit core) or None (sampled: returns (share, first index))"""
    nm, L = self.nq + self.np_, lib()
    if e is not None:
        return _kg_call(self, "ckg_gen_share", lambda c, ee, o: L.sfg_ckg_gen_share_dev(self.h, c, ee, o), [(crp, np.uint64, (nm, self.N)), (e, np.int32, (self.N,))], [(nm, self.N)])[0]
    first = C.c_uint64()
    out = _kg_call(self, "ckg_gen_share_sampled", lambda c, o: L.sfg_ckg_gen_share_sampled_dev(self.h, c, o, C.byref(first)), [(crp, np.uint64, (nm, self.N))], [(nm, self.N)])[0]
    return out, first.value


def _ctx_rtg_gen_shares(self, galois, crp, e=None):
    """galois: nkeys Galois elements; crp [nkeys][beta][nmod][N]; e int32 [nkeys][beta][N] or None (sampled: returns (shares, first index))"""
    nm, L = self.nq + self.np_, lib()
    g, gp = _galois_arr(galois); nk = int(g.size)
    shp = (max(nk, 1), self.beta, nm, self.N)
    if e is not None:
        return _kg_call(self, "rtg_gen_shares", lambda c, ee, o: L.sfg_rtg_gen_shares_dev(self.h, gp, nk, c, ee, o),
                        [(crp, np.uint64, shp), (e, np.int32, (max(nk, 1), self.beta, self.N))], [shp])[0]
    first = C.c_uint64()
    out = _kg_call(self, "rtg_gen_shares_sampled", lambda c, o: L.sfg_rtg_gen_shares_sampled_dev(self.h, gp, nk, c, o, C.byref(first)), [(crp, np.uint64, shp)], [shp])[0]
    return out, first.value


def _ctx_rkg_round1(self, crp, u=None, e0=None, e1=None):
    """crp [beta][nmod][N]; u int8 [N], e0, e1 int32 [beta][N] -> (h0, h1); all None: sampled, returns (h0, h1, first index, u index)"""
    nm, L = self.nq + self.np_, lib()
    shp = (self.beta, nm, self.N)
    if u is not None:
        return tuple(_kg_call(self, "rkg_round1", lambda c, uu, a, b, h0, h1: L.sfg_rkg_round1_dev(self.h, c, uu, a, b, h0, h1),
                              [(crp, np.uint64, shp), (u, np.int8, (self.N,)), (e0, np.int32, (self.beta, self.N)), (e1, np.int32, (self.beta, self.N))], [shp, shp]))
    first, ui = C.c_uint64(), C.c_uint64()
    h0, h1 = _kg_call(self, "rkg_round1_sampled", lambda c, a, b: L.sfg_rkg_round1_sampled_dev(self.h, c, a, b, C.byref(first), C.byref(ui)), [(crp, np.uint64, shp)], [shp, shp])
    return h0, h1, first.value, ui.value


def _ctx_rkg_round2(self, h0agg, h1agg, u=None, e2=None, e3=None, u_index=None):
    """H0agg, H1agg [beta][nmod][N]; explicit (u, e2, e3) -> share; or u_index (from round 1) -> (share, first index)"""
    nm, L = self.nq + self.np_, lib()
    shp = (self.beta, nm, self.N)
    if u is not None:
        return _kg_call(self, "rkg_round2", lambda a, b, uu, x, y, o: L.sfg_rkg_round2_dev(self.h, a, b, uu, x, y, o),
                        [(h0agg, np.uint64, shp), (h1agg, np.uint64, shp), (u, np.int8, (self.N,)), (e2, np.int32, (self.beta, self.N)), (e3, np.int32, (self.beta, self.N))], [shp])[0]
    first = C.c_uint64()
    out = _kg_call(self, "rkg_round2_sampled", lambda a, b, o: L.sfg_rkg_round2_sampled_dev(self.h, a, b, int(u_index), o, C.byref(first)),
                   [(h0agg, np.uint64, shp), (h1agg, np.uint64, shp)], [shp])[0]
    return out, first.value


def _ctx_install_public_key(self, agg, crp):
    nm = self.nq + self.np_
    _kg_call(self, "install_public_key", lambda a, c: lib().sfg_ctx_install_public_key_dev(self.h, a, c), [(agg, np.uint64, (nm, self.N)), (crp, np.uint64, (nm, self.N))], [])


def _ctx_install_rotkeys(self, galois, agg, crp):
    nm = self.nq + self.np_
    g, gp = _galois_arr(galois); nk = int(g.size)
    shp = (max(nk, 1), self.beta, nm, self.N)
    _kg_call(self, "install_rotkeys", lambda a, c: lib().sfg_ctx_install_rotkeys_dev(self.h, gp, nk, a, c), [(agg, np.uint64, shp), (crp, np.uint64, shp)], [])


def _ctx_install_relinkey(self, round2agg, h1agg):
    shp = (self.beta, self.nq + self.np_, self.N)
    _kg_call(self, "install_relinkey", lambda a, c: lib().sfg_ctx_install_relinkey_dev(self.h, a, c), [(round2agg, np.uint64, shp), (h1agg, np.uint64, shp)], [])


def _ctx_crp_fill(self, key32, first_row, mod_idx, out=None):
    """rows first_row .. first_row + len(mod_idx) - 1 of the common reference stream under the 32-byte seed -> DevArray [nrows][N] (or into `out`)"""
    key32 = bytes(key32)
    if len(key32) != 32:
        raise ValueError("the common reference seed is 32 bytes")
    n = len(mod_idx)
    mi = (C.c_int * max(n, 1))(*[int(x) for x in mod_idx])
    dst = out if out is not None else DevArray(self, (max(n, 1), self.N))
    rc = lib().sfg_crp_fill_dev(self.h, key32, int(first_row), n, mi, dst.p)
    if rc and out is None:
        dst.free()
    self.check(rc, "crp_fill")
    return dst


Context.load_secret_key_qp = _ctx_load_secret_key_qp
Context.ckg_gen_share = _ctx_ckg_gen_share
Context.rtg_gen_shares = _ctx_rtg_gen_shares
Context.rkg_round1 = _ctx_rkg_round1
Context.rkg_round2 = _ctx_rkg_round2
Context.install_public_key = _ctx_install_public_key
Context.install_rotkeys = _ctx_install_rotkeys
Context.install_relinkey = _ctx_install_relinkey
Context.crp_fill = _ctx_crp_fill


class Ring:
    """sfg_ring wrapper: the general ring (logN 12..16, prime moduli below 2^61).  Shaped like Context: host arrays in, host arrays out for the tests; the *_dev
    entry points take the pointers of malloc / to_device for callers that keep ciphertexts resident."""

    def __init__(self, logN, q, p, device=0, psi=None):
        L = lib()
        self.logN, self.q, self.p = logN, list(q), list(p)
        self.nq, self.np_ = len(q), len(p)
        self.moduli = self.q + self.p
        self.N, self.slots = 1 << logN, (1 << logN) // 2
        mods = np.array(self.moduli, dtype=np.uint64)
        h = C.c_void_p()
        ps = None if psi is None else p64(np.array(psi, dtype=np.uint64))
        if L.sfg_ring_create(C.byref(h), device, logN, self.nq, self.np_, p64(mods) if len(mods) else None, ps):
            raise SfgError("sfg_ring_create: " + L.sfg_ring_last_error(None).decode())
        self.h = h
        self.beta = (self.nq + self.np_ - 1) // self.np_

    def close(self):
        if getattr(self, "h", None):
            lib().sfg_ring_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what):
        if rc:
            raise SfgError(f"{what}: {lib().sfg_ring_last_error(self.h).decode()}")

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.check(lib().sfg_ring_malloc(self.h, C.byref(p), max(int(nbytes), 8)), "sfg_ring_malloc")
        return p

    def free(self, p):
        self.check(lib().sfg_ring_free(self.h, p), "sfg_ring_free")

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        self.check(lib().sfg_ring_memcpy_h2d(self.h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "sfg_ring_memcpy_h2d")
        return p

    def to_host(self, p, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        self.check(lib().sfg_ring_memcpy_d2h(self.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes), "sfg_ring_memcpy_d2h")
        return out

    def sync(self):
        self.check(lib().sfg_ring_synchronize(self.h), "sfg_ring_synchronize")

    def galois(self, k_left):
        return lib().sfg_ring_galois_for_rotation(self.h, int(k_left))

    def ntt_rows(self, rows, mod_idx, inverse=False):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = rows.shape[0]
        mi = (C.c_int * n)(*[int(x) for x in mod_idx])
        d = self.to_device(rows)
        name = "sfg_ring_intt_rows" if inverse else "sfg_ring_ntt_rows"
        try:
            self.check(getattr(lib(), name)(self.h, d, n, mi), name)
            return self.to_host(d, rows.shape)
        finally:
            self.free(d)

    def load_rotkey(self, galois, key, montgomery=False):
        key = np.ascontiguousarray(key, dtype=np.uint64)
        self.check(lib().sfg_ring_load_rotkey(self.h, int(galois), p64(key), int(montgomery)), "sfg_ring_load_rotkey")

    def has_rotkey(self, galois):
        return bool(lib().sfg_ring_has_rotkey(self.h, int(galois)))

    def load_relinkey(self, key, montgomery=False):
        key = np.ascontiguousarray(key, dtype=np.uint64)
        self.check(lib().sfg_ring_load_relinkey(self.h, p64(key), int(montgomery)), "sfg_ring_load_relinkey")

    def _run(self, name, ins, out_shape, call):
        """upload the host arrays `ins`, allocate the output, run call(device inputs, device output), download"""
        devs = [self.to_device(np.ascontiguousarray(a, dtype=np.uint64)) for a in ins]
        out = self.malloc(int(np.prod(out_shape)) * 8)
        try:
            self.check(call(devs, out), name)
            return self.to_host(out, out_shape)
        finally:
            for d_ in devs + [out]:
                self.free(d_)

    def rotate_right(self, cts, level, nrots):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        arr = (C.c_int * cts.shape[0])(*[int(x) for x in nrots])
        return self._run("sfg_ring_rotate_right_dev", [cts], cts.shape,
                         lambda d, o: lib().sfg_ring_rotate_right_dev(self.h, d[0], o, cts.shape[0], level, arr))

    def apply_galois(self, cts, level, galois):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        return self._run("sfg_ring_ct_galois_dev", [cts], cts.shape,
                         lambda d, o: lib().sfg_ring_ct_galois_dev(self.h, d[0], o, cts.shape[0], level, int(galois)))

    def _binary(self, name, a, b, level):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return self._run(name, [a, b], a.shape, lambda d, o: getattr(lib(), name)(self.h, d[0], d[1], o, a.shape[0], level))

    def add(self, a, b, level):
        return self._binary("sfg_ring_ct_add_dev", a, b, level)

    def sub(self, a, b, level):
        return self._binary("sfg_ring_ct_sub_dev", a, b, level)

    def mulrelin(self, a, b, level):
        return self._binary("sfg_ring_ct_mulrelin_dev", a, b, level)

    def drop_level(self, cts, level_in, level_out):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        return self._run("sfg_ring_ct_drop_level_dev", [cts], (cts.shape[0], 2, max(level_out, 0) + 1, self.N),
                         lambda d, o: lib().sfg_ring_ct_drop_level_dev(self.h, d[0], o, cts.shape[0], level_in, level_out))

    def _scalar(self, name, cts, scalars, level):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        sc = np.ascontiguousarray(scalars, dtype=np.uint64)
        return self._run(name, [cts], cts.shape, lambda d, o: getattr(lib(), name)(self.h, d[0], p64(sc), o, cts.shape[0], level))

    def mul_scalar(self, cts, scalars, level):
        return self._scalar("sfg_ring_ct_mul_scalar_dev", cts, scalars, level)

    def add_scalar(self, cts, scalars, level):
        return self._scalar("sfg_ring_ct_add_scalar_dev", cts, scalars, level)

    def mul_scalar_add(self, cts, scalars, acc, level):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        sc = np.ascontiguousarray(scalars, dtype=np.uint64)
        d_ct, d_acc = self.to_device(cts), self.to_device(np.ascontiguousarray(acc, dtype=np.uint64))
        try:
            self.check(lib().sfg_ring_ct_mul_scalar_add_dev(self.h, d_ct, p64(sc), d_acc, cts.shape[0], level), "sfg_ring_ct_mul_scalar_add_dev")
            return self.to_host(d_acc, cts.shape)
        finally:
            self.free(d_ct)
            self.free(d_acc)

    def _plain(self, name, cts, pt, level):
        """pt: [level+1][N] (one plaintext for all) or [nct][level+1][N]"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        pt = np.ascontiguousarray(pt, dtype=np.uint64)
        stride = 0 if pt.ndim == 2 else pt.shape[1] * pt.shape[2]
        return self._run(name, [cts, pt], cts.shape, lambda d, o: getattr(lib(), name)(self.h, d[0], d[1], stride, o, cts.shape[0], level))

    def add_plain(self, cts, pt, level):
        return self._plain("sfg_ring_ct_add_plain_dev", cts, pt, level)

    def mul_plain(self, cts, pt, level):
        return self._plain("sfg_ring_ct_mul_plain_dev", cts, pt, level)

    def rescale(self, cts, level):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        return self._run("sfg_ring_ct_rescale_dev", [cts], (cts.shape[0], 2, max(level, 1), self.N),
                         lambda d, o: lib().sfg_ring_ct_rescale_dev(self.h, d[0], o, cts.shape[0], level))

    def innersum(self, cts, level):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        return self._run("sfg_ring_ct_innersum_dev", [cts], (2, level + 1, self.N),
                         lambda d, o: lib().sfg_ring_ct_innersum_dev(self.h, d[0], cts.shape[0], level, o))

    # ---- the two ends (gring_io.hip): keys, sampler, encryption, the collective decryption's local halves
    def load_public_key(self, pk, montgomery=False):
        pk = np.ascontiguousarray(pk, dtype=np.uint64)
        assert pk.shape == (2, len(self.moduli), self.N)
        self.check(lib().sfg_ring_load_public_key(self.h, p64(pk), int(montgomery)), "sfg_ring_load_public_key")

    def has_public_key(self):
        return bool(lib().sfg_ring_has_public_key(self.h))

    def load_secret_key(self, sk, montgomery=False):
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        assert sk.shape == (self.nq, self.N)
        self.check(lib().sfg_ring_load_secret_key(self.h, p64(sk), int(montgomery)), "sfg_ring_load_secret_key")

    def seed_encryptor(self, key32):
        key32 = bytes(key32)
        assert len(key32) == 32
        self.check(lib().sfg_ring_seed_encryptor(self.h, key32), "sfg_ring_seed_encryptor")

    def encryptor_next_index(self):
        v = C.c_uint64()
        self.check(lib().sfg_ring_encryptor_next_index(self.h, C.byref(v)), "sfg_ring_encryptor_next_index")
        return v.value

    def _run_mixed(self, name, ins, out_shapes, call):
        """_run for inputs of any dtype (None stays a null pointer) and several uint64 outputs (a None shape stays a null pointer)"""
        devs = [None if a is None else self.to_device(np.ascontiguousarray(a)) for a in ins]
        outs = [None if s is None else self.malloc(int(np.prod(s)) * 8) for s in out_shapes]
        try:
            self.check(call(devs, outs), name)
            return [None if s is None else self.to_host(o, s) for o, s in zip(outs, out_shapes)]
        finally:
            for d_ in devs + outs:
                if d_ is not None:
                    self.free(d_)

    def encrypt_explicit(self, pt, level, u, e0, e1):
        """pt None or [nct][level+1][N]; u int8, e0, e1 int32 [nct][N] -> [nct][2][level+1][N]"""
        u, e0, e1 = np.ascontiguousarray(u, dtype=np.int8), np.ascontiguousarray(e0, dtype=np.int32), np.ascontiguousarray(e1, dtype=np.int32)
        nct = u.shape[0]
        pt = None if pt is None else np.ascontiguousarray(pt, dtype=np.uint64)
        return self._run_mixed("sfg_ring_encrypt_explicit_dev", [pt, u, e0, e1], [(nct, 2, level + 1, self.N)],
                               lambda d, o: lib().sfg_ring_encrypt_explicit_dev(self.h, d[0], nct, level, d[1], d[2], d[3], o[0]))[0]

    def add_fresh_zero(self, cts, level):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        d = self.to_device(cts)
        try:
            self.check(lib().sfg_ring_ct_add_fresh_zero_dev(self.h, d, cts.shape[0], level), "sfg_ring_ct_add_fresh_zero_dev")
            return self.to_host(d, cts.shape)
        finally:
            self.free(d)

    def encrypt_transcript(self, first_index, nct):
        """test hook -> (u int8, e0 int32, e1 int32), each [nct][N]"""
        n = max(nct, 1) * self.N
        du, d0, d1 = self.malloc(n), self.malloc(4 * n), self.malloc(4 * n)
        try:
            self.check(lib().sfg_ring_encrypt_transcript_for_test(self.h, int(first_index), nct, du, d0, d1), "sfg_ring_encrypt_transcript_for_test")
            return (self.to_host(du, (nct, self.N), np.int8), self.to_host(d0, (nct, self.N), np.int32), self.to_host(d1, (nct, self.N), np.int32))
        finally:
            for d_ in (du, d0, d1):
                self.free(d_)

    def pcks_gen_share(self, cts, level, e0, e1=None):
        """-> (h0, h1) [nct][level+1][N]; e1 None: h1 is not computed (None)"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        nct = cts.shape[0]
        e0 = np.ascontiguousarray(e0, dtype=np.int32)
        e1 = None if e1 is None else np.ascontiguousarray(e1, dtype=np.int32)
        row = (nct, level + 1, self.N)
        return tuple(self._run_mixed("sfg_ring_pcks_gen_share_dev", [cts, e0, e1], [row, None if e1 is None else row],
                                     lambda d, o: lib().sfg_ring_pcks_gen_share_dev(self.h, d[0], nct, level, d[1], d[2], o[0], o[1])))

    def pcks_finish(self, cts, level, h0agg):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        nct = cts.shape[0]
        return self._run_mixed("sfg_ring_pcks_finish_dev", [cts, np.ascontiguousarray(h0agg, dtype=np.uint64)], [(nct, level + 1, self.N)],
                               lambda d, o: lib().sfg_ring_pcks_finish_dev(self.h, d[0], nct, level, d[1], o[0]))[0]

    # ---- collective bootstrap, local halves (gring_refresh.hip)
    def refresh_gen_shares(self, cts, level, crs, mask_limbs, e0, e1, scales=None):
        """cts [nct][2][level+1][N], crs [nct][nq][N], mask_limbs [nct][N][W] uint64 two's complement, e0 / e1 [nct][N] int32 -> (h0 [nct][level+1][N], h1 [nct][nq][N]);
        scales = (ciphertext scale, target scale) selects the target-scale form"""
        cts, crs = np.ascontiguousarray(cts, dtype=np.uint64), np.ascontiguousarray(crs, dtype=np.uint64)
        mask_limbs = np.ascontiguousarray(mask_limbs, dtype=np.uint64)
        nct, W = cts.shape[0], mask_limbs.shape[-1]
        ins = [cts, crs, mask_limbs, np.ascontiguousarray(e0, dtype=np.int32), np.ascontiguousarray(e1, dtype=np.int32)]
        shapes = [(nct, level + 1, self.N), (nct, self.nq, self.N)]
        if scales is None:
            return tuple(self._run_mixed("sfg_ring_refresh_gen_shares_dev", ins, shapes,
                                         lambda d, o: lib().sfg_ring_refresh_gen_shares_dev(self.h, d[0], nct, level, d[1], d[2], W, d[3], d[4], o[0], o[1])))
        return tuple(self._run_mixed("sfg_ring_refresh_gen_shares_scaled_dev", ins, shapes,
                                     lambda d, o: lib().sfg_ring_refresh_gen_shares_scaled_dev(self.h, d[0], nct, level, float(scales[0]), float(scales[1]), d[1], d[2], W,
                                                                                               d[3], d[4], o[0], o[1])))

    def refresh_finish(self, cts, level, h0agg, h1agg, crs, scales=None):
        """cts [nct][2][level+1][N], h0agg [nct][level+1][N], h1agg, crs [nct][nq][N] -> [nct][2][nq][N] at level nq - 1"""
        ins = [np.ascontiguousarray(a, dtype=np.uint64) for a in (cts, h0agg, h1agg, crs)]
        nct = ins[0].shape[0]
        shapes = [(nct, 2, self.nq, self.N)]
        if scales is None:
            return self._run_mixed("sfg_ring_refresh_finish_dev", ins, shapes,
                                   lambda d, o: lib().sfg_ring_refresh_finish_dev(self.h, d[0], nct, level, d[1], d[2], d[3], o[0]))[0]
        return self._run_mixed("sfg_ring_refresh_finish_scaled_dev", ins, shapes,
                               lambda d, o: lib().sfg_ring_refresh_finish_scaled_dev(self.h, d[0], nct, level, float(scales[0]), float(scales[1]), d[1], d[2], d[3], o[0]))[0]

    def decode_coeffs(self, pt, level, scale, poly0_of_cts=False):
        """pt [nct][level+1][N] NTT-domain rows -> float64 [nct][N]: centred coefficient / scale.  poly0_of_cts: pt is [nct][2][level+1][N], polynomial 0 read in place"""
        pt = np.ascontiguousarray(pt, dtype=np.uint64)
        nct, rows = pt.shape[0], (level + 1) * self.N
        stride = 2 * rows if poly0_of_cts else rows
        out = np.empty((nct, self.N), dtype=np.float64)
        d = self.to_device(pt)
        try:
            self.check(lib().sfg_ring_decode_coeffs(self.h, d, stride, nct, level, float(scale), out.ctypes.data_as(C.POINTER(C.c_double))), "sfg_ring_decode_coeffs")
            return out
        finally:
            self.free(d)

    def _values_call(self, name, values, level, scale, out_shape):
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.ndim == 2 and values.shape[1] == self.slots
        out = self.malloc(int(np.prod(out_shape)) * 8)
        try:
            self.check(getattr(lib(), name)(self.h, values.ctypes.data_as(C.POINTER(C.c_double)), values.shape[0], level, float(scale), out), name)
            return self.to_host(out, out_shape)
        finally:
            self.free(out)

    def encode_vectors(self, values, level, scale):
        """values [nvec][slots] real -> NTT-domain plaintext rows [nvec][level+1][N]"""
        return self._values_call("sfg_ring_encode_vectors_dev", values, level, scale, (len(values), level + 1, self.N))

    def encrypt_vectors(self, values, level, scale):
        """values [nct][slots] real -> ciphertexts [nct][2][level+1][N] (EncryptFloatVector)"""
        return self._values_call("sfg_ring_encrypt_vectors_dev", values, level, scale, (len(values), 2, level + 1, self.N))

    def decode_vectors(self, pt, level, scale, want_imag=False, poly0_of_cts=False, on_device=False):
        """pt [nct][level+1][N] -> real parts [nct][slots] (and the imaginary parts); on_device: through sfg_ring_decode_vectors_dev and a download"""
        pt = np.ascontiguousarray(pt, dtype=np.uint64)
        nct, rows = pt.shape[0], (level + 1) * self.N
        stride = 2 * rows if poly0_of_cts else rows
        re, im = np.empty((nct, self.slots)), (np.empty((nct, self.slots)) if want_imag else None)
        pd_ = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
        d = self.to_device(pt)
        try:
            if on_device:
                dre, dim_ = self.malloc(re.nbytes), (self.malloc(re.nbytes) if want_imag else None)
                try:
                    self.check(lib().sfg_ring_decode_vectors_dev(self.h, d, stride, nct, level, float(scale), dre, dim_), "sfg_ring_decode_vectors_dev")
                    re = self.to_host(dre, re.shape, np.float64)
                    im = self.to_host(dim_, re.shape, np.float64) if want_imag else None
                finally:
                    self.free(dre)
                    if dim_ is not None:
                        self.free(dim_)
            else:
                self.check(lib().sfg_ring_decode_vectors(self.h, d, stride, nct, level, float(scale), pd_(re), pd_(im)), "sfg_ring_decode_vectors")
        finally:
            self.free(d)
        return (re, im) if want_imag else re

    def decrypt_vectors(self, cts, level, scale, want_imag=False):
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        nct = cts.shape[0]
        re, im = np.empty((nct, self.slots)), (np.empty((nct, self.slots)) if want_imag else None)
        d = self.to_device(cts)
        try:
            self.check(lib().sfg_ring_decrypt_vectors(self.h, d, nct, level, float(scale), re.ctypes.data_as(C.POINTER(C.c_double)),
                                                      None if im is None else im.ctypes.data_as(C.POINTER(C.c_double))), "sfg_ring_decrypt_vectors")
        finally:
            self.free(d)
        return (re, im) if want_imag else re

    # ---- collective key generation (gring_keygen.hip).  A polynomial argument is a host array (uploaded for the call) or a device pointer of malloc / to_device
    # (used in place).  Results come back as host arrays, or stay on the device (`keep`: the pointers, for the caller to free); `out` supplies the result buffers.
    def _kg(self, name, ins, out_shapes, call, keep=False, out=None):
        own_in = [not isinstance(a, C.c_void_p) and a is not None for a, _ in ins]
        devs = [self.to_device(np.ascontiguousarray(a, dtype=dt)) if o else a for (a, dt), o in zip(ins, own_in)]
        outs = list(out) if out is not None else [self.malloc(int(np.prod(s)) * 8) for s in out_shapes]
        ok = False
        try:
            self.check(call(devs, outs), name)
            ok = True
            return outs if keep or out is not None else [self.to_host(o, s) for o, s in zip(outs, out_shapes)]
        finally:
            for d_, o in zip(devs, own_in):
                if o:
                    self.free(d_)
            if out is None and not (keep and ok):
                for o in outs:
                    self.free(o)

    def load_secret_key_qp(self, sk, montgomery=False):
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        assert sk.shape == (len(self.moduli), self.N)
        self.check(lib().sfg_ring_load_secret_key_qp(self.h, p64(sk), int(montgomery)), "sfg_ring_load_secret_key_qp")

    def ckg_gen_share(self, crp, e=None, sampled=False, keep=False, out=None):
        """crp [nmod][N]; e int32 [N] -> share [nmod][N]; sampled: -> (share, first index)"""
        shp, L = [(len(self.moduli), self.N)], lib()
        if not sampled:
            return self._kg("sfg_ring_ckg_gen_share_dev", [(crp, np.uint64), (e, np.int32)], shp, lambda d, o: L.sfg_ring_ckg_gen_share_dev(self.h, d[0], d[1], o[0]), keep, out)[0]
        first = C.c_uint64()
        r = self._kg("sfg_ring_ckg_gen_share_sampled_dev", [(crp, np.uint64)], shp, lambda d, o: L.sfg_ring_ckg_gen_share_sampled_dev(self.h, d[0], o[0], C.byref(first)), keep, out)
        return r[0], first.value

    def rtg_gen_shares(self, galois, crp, e=None, sampled=False, keep=False, out=None):
        """galois: nkeys elements; crp [nkeys][beta][nmod][N]; e int32 [nkeys][beta][N] -> shares like crp; sampled: -> (shares, first index)"""
        g, gp = _galois_arr(galois); nk, L = int(g.size), lib()
        shp = [(max(nk, 1), self.beta, len(self.moduli), self.N)]
        if not sampled:
            return self._kg("sfg_ring_rtg_gen_shares_dev", [(crp, np.uint64), (e, np.int32)], shp, lambda d, o: L.sfg_ring_rtg_gen_shares_dev(self.h, gp, nk, d[0], d[1], o[0]), keep, out)[0]
        first = C.c_uint64()
        r = self._kg("sfg_ring_rtg_gen_shares_sampled_dev", [(crp, np.uint64)], shp, lambda d, o: L.sfg_ring_rtg_gen_shares_sampled_dev(self.h, gp, nk, d[0], o[0], C.byref(first)), keep, out)
        return r[0], first.value

    def rkg_round1(self, crp, u=None, e0=None, e1=None, sampled=False, keep=False, out=None):
        """crp [beta][nmod][N]; u int8 [N], e0, e1 int32 [beta][N] -> (h0, h1); sampled: -> (h0, h1, first index, u index)"""
        shp, L = [(self.beta, len(self.moduli), self.N)] * 2, lib()
        if not sampled:
            return tuple(self._kg("sfg_ring_rkg_round1_dev", [(crp, np.uint64), (u, np.int8), (e0, np.int32), (e1, np.int32)], shp,
                                  lambda d, o: L.sfg_ring_rkg_round1_dev(self.h, d[0], d[1], d[2], d[3], o[0], o[1]), keep, out))
        first, ui = C.c_uint64(), C.c_uint64()
        h0, h1 = self._kg("sfg_ring_rkg_round1_sampled_dev", [(crp, np.uint64)], shp, lambda d, o: L.sfg_ring_rkg_round1_sampled_dev(self.h, d[0], o[0], o[1], C.byref(first), C.byref(ui)), keep, out)
        return h0, h1, first.value, ui.value

    def rkg_round2(self, h0agg, h1agg, u=None, e2=None, e3=None, u_index=None, sampled=False, keep=False, out=None):
        """H0agg, H1agg [beta][nmod][N]; (u, e2, e3) -> share; sampled with u_index (from round 1): -> (share, first index)"""
        shp, L = [(self.beta, len(self.moduli), self.N)], lib()
        if not sampled:
            return self._kg("sfg_ring_rkg_round2_dev", [(h0agg, np.uint64), (h1agg, np.uint64), (u, np.int8), (e2, np.int32), (e3, np.int32)], shp,
                            lambda d, o: L.sfg_ring_rkg_round2_dev(self.h, d[0], d[1], d[2], d[3], d[4], o[0]), keep, out)[0]
        first = C.c_uint64()
        r = self._kg("sfg_ring_rkg_round2_sampled_dev", [(h0agg, np.uint64), (h1agg, np.uint64)], shp,
                     lambda d, o: L.sfg_ring_rkg_round2_sampled_dev(self.h, d[0], d[1], int(u_index), o[0], C.byref(first)), keep, out)
        return r[0], first.value

    def install_public_key(self, agg, crp):
        self._kg("sfg_ring_install_public_key_dev", [(agg, np.uint64), (crp, np.uint64)], [], lambda d, o: lib().sfg_ring_install_public_key_dev(self.h, d[0], d[1]))

    def install_rotkeys(self, galois, agg, crp):
        g, gp = _galois_arr(galois)
        self._kg("sfg_ring_install_rotkeys_dev", [(agg, np.uint64), (crp, np.uint64)], [], lambda d, o: lib().sfg_ring_install_rotkeys_dev(self.h, gp, int(g.size), d[0], d[1]))

    def install_relinkey(self, round2agg, h1agg):
        self._kg("sfg_ring_install_relinkey_dev", [(round2agg, np.uint64), (h1agg, np.uint64)], [], lambda d, o: lib().sfg_ring_install_relinkey_dev(self.h, d[0], d[1]))

    def export_rotkey(self, galois):
        """-> [beta][2][nmod][N]: exactly (agg, crp); galois 1 = the relinearisation key"""
        out = np.empty((self.beta, 2, len(self.moduli), self.N), dtype=np.uint64)
        self.check(lib().sfg_ring_export_rotkey(self.h, int(galois), p64(out)), "sfg_ring_export_rotkey")
        return out

    def crp_fill(self, key32, first_row, mod_idx, keep=False, out=None):
        """rows first_row .. first_row + len(mod_idx) - 1 of the common reference stream under the 32-byte seed -> [nrows][N]"""
        key32 = bytes(key32)
        if len(key32) != 32:
            raise ValueError("the common reference seed is 32 bytes")
        n = len(mod_idx)
        mi = (C.c_int * max(n, 1))(*[int(x) for x in mod_idx])
        return self._kg("sfg_ring_crp_fill_dev", [], [(max(n, 1), self.N)], lambda d, o: lib().sfg_ring_crp_fill_dev(self.h, key32, int(first_row), n, mi, o[0]), keep, out)[0]

    # ---- the matrix products (gring_matmul.hip)
    def mm_shape(self, geno_shape, flags=0):
        """-> (nbr, m_ct, d) of the operand: the matrix, or its transpose with SFG_TRANSPOSE"""
        import math
        nrow, ncol = geno_shape
        rows, cols = (ncol, nrow) if flags & SFG_TRANSPOSE else (nrow, ncol)
        d = math.isqrt(self.slots - 1) + 1
        return (rows - 1) // self.slots + 1, (cols - 1) // self.slots + 1, d

    def _mm_operands(self, A, in_level, geno, flags):
        A = np.ascontiguousarray(A, dtype=np.uint64)
        geno = np.ascontiguousarray(geno, dtype=np.int8)
        nbr, m_ct, d = self.mm_shape(geno.shape, flags)
        if A.ndim != 5 or A.shape[1:] != (nbr, 2, in_level + 1, self.N):
            raise ValueError(f"A must be [s][{nbr}][2][{in_level + 1}][{self.N}], got {A.shape}")
        return A, geno, nbr, m_ct, d

    def matmul(self, A, in_level, max_level, geno, scale, flags=0):
        """MatMult4Stream: A [s][nbr][2][in_level+1][N] x geno int8 [nrow][ncol] -> [s][m_ct][2][max_level][N]"""
        A, geno, nbr, m_ct, d = self._mm_operands(A, in_level, geno, flags)
        s = A.shape[0]
        g = self.to_device(geno)
        try:
            return self._run("sfg_ring_matmul_dev", [A], (s, m_ct, 2, max_level, self.N),
                             lambda dv, o: lib().sfg_ring_matmul_dev(self.h, dv[0], s, in_level, max_level, g, geno.shape[0], geno.shape[1], geno.shape[1], flags, float(scale), o))
        finally:
            self.free(g)

    def matmul_accumulate(self, A, in_level, max_level, geno, scale, flags=0, b0=0, b1=None):
        """-> (acc [m_ct][d][s][2][max_level][N] canonical, giant_active uint8 [d]) over operand block rows [b0, b1)"""
        A, geno, nbr, m_ct, d = self._mm_operands(A, in_level, geno, flags)
        s = A.shape[0]
        b1 = nbr if b1 is None else b1
        active = np.zeros(d, dtype=np.uint8)
        g = self.to_device(geno)
        try:
            acc = self._run("sfg_ring_matmul_accumulate_dev", [A], (m_ct, d, s, 2, max_level, self.N),
                            lambda dv, o: lib().sfg_ring_matmul_accumulate_dev(self.h, dv[0], s, in_level, max_level, g, geno.shape[0], geno.shape[1], geno.shape[1], flags,
                                                                               float(scale), int(b0), int(b1), o, active.ctypes.data_as(C.POINTER(C.c_uint8))))
        finally:
            self.free(g)
        return acc, active

    def matmul_finalize(self, acc, giant_active, max_level, g0=0, g1=None, into=None):
        """acc [m_ct][d][s][2][max_level][N] -> out [s][m_ct][2][max_level][N]: the giants of [g0, g1) that giant_active marks (None: all), added to `into` when given"""
        acc = np.ascontiguousarray(acc, dtype=np.uint64)
        m_ct, d, s = acc.shape[:3]
        g1 = d if g1 is None else g1
        ga = None if giant_active is None else np.ascontiguousarray(giant_active, dtype=np.uint8)
        gp = None if ga is None else ga.ctypes.data_as(C.POINTER(C.c_uint8))
        shape = (s, m_ct, 2, max_level, self.N)
        devs = [self.to_device(acc)]
        out = self.to_device(np.ascontiguousarray(into, dtype=np.uint64)) if into is not None else self.malloc(int(np.prod(shape)) * 8)
        try:
            self.check(lib().sfg_ring_matmul_finalize_dev(self.h, devs[0], gp, s, max_level, m_ct, int(g0), int(g1), int(into is not None), out), "sfg_ring_matmul_finalize_dev")
            return self.to_host(out, shape)
        finally:
            for d_ in devs + [out]:
                self.free(d_)

    def set_ws_budget_for_test(self, nbytes):
        """test hook (SFG_ENABLE_TEST_HOOKS=1 before the ring was made): the byte budget that sizes the chunks of the evaluator's workspaces"""
        self.check(lib().sfg_ring_set_ws_budget_for_test(self.h, int(nbytes)), "sfg_ring_set_ws_budget_for_test")

    def encoder_resolved(self, reset=False):
        """diagonal coefficients the products re-derived exactly (inside the encoder's band of a rounding tie) since the last reset"""
        n = C.c_ulonglong(0)
        self.check(lib().sfg_ring_encoder_resolved(self.h, C.byref(n), int(bool(reset))), "sfg_ring_encoder_resolved")
        return int(n.value)

    def set_tie_band_for_test(self, log2_floor):
        """test hook (SFG_ENABLE_TEST_HOOKS=1 before the ring was made): the floor 2^log2_floor of the band of the products' diagonals"""
        self.check(lib().sfg_ring_set_tie_band_for_test(self.h, int(log2_floor)), "sfg_ring_set_tie_band_for_test")
