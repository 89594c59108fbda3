/*
 * sfgwas_hip.h — C-ABI of libsfgwas_hip.so: the MI355X (gfx950) implementation of SF-GWAS's
 * per-party local linear-algebra hot path.
 *
 * The reference (hhcho/sfgwas, 100 % Go) has no FFI/plugin seam; the seam is cut at Go function level
 * (SURVEY.md §8b).  Each entry point below names the reference interface it replaces (file:line under
 * the reference tree); INTEGRATION.md shows the cgo stub a maintainer would add on the Go side.
 *
 * Conventions
 *  - plain pointers and sizes only; every function returns 0 on success, non-zero on error, and
 *    sfg_last_error(ctx) describes the failure (the reference panics on this path — matmult.go:361,
 *    filestream.go:60 — so the Go shim turns non-zero into panic()).
 *  - Ring: N = 2^logN (logN = 14 for the PN14QP438 preset used by the reference, gwas.go:169),
 *    nq ciphertext primes q_0..q_{nq-1} followed by np special primes; all < 2^47 and == 1 mod 2N
 *    (PN12..PN14 presets of gwas.go:164-177 in prime size; the 55-bit primes of PN15 / PN16 and logN != 14 are not supported).
 *  - Polynomial rows are N uint64 canonical residues in lattigo's NTT order
 *    (row[i] = p(psi^(2*bitrev(i)+1))); a ciphertext at level l is [2][l+1][N]
 *    (= ct.Value()[k].Coeffs[m][:] flattened, crypto.go:32-60).
 *  - "_dev" pointers are device (HBM) addresses on the context's GPU; "_host" are host pointers.
 *  - Threading: one host thread drives a context at a time - the exclusivity rule of the Go evaluator
 *    pool (crypto.go:311-316).  Concurrent callers (assoc.go:360-408 runs assoc_num_blocks_parallel MatMult4Stream
 *    calls at once) each take a fork (sfg_ctx_fork): forks share the immutable ring tables and key material of their
 *    parent and own their HIP queues, scratch, staging ring, timers and error string.  The library keeps no
 *    process-global state and reads the environment only inside sfg_ctx_create.
 */
#ifndef SFGWAS_HIP_H
#define SFGWAS_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfg_ctx sfg_ctx;
typedef struct sfg_geno sfg_geno;

/* ---- context: created after CollectiveInit (gwas.go:212), from cryptoParams.Params + ring tables ----
 * replaces: ring.NewRing(N, Qi) at matmult.go:328,345,403 and the evaluator/encoder pools (crypto.go:89-135).
 * psi[m]: the primitive 2N-th root lattigo uses for modulus m (ring.Ring.PsiMont un-Montgomery'd); NULL =>
 * derived from the smallest primitive root exactly as lattigo derives it. */
int sfg_ctx_create(sfg_ctx **out, int device, int logN, int nq, int np,
                   const uint64_t *moduli, const uint64_t *psi, double scale);
/* The configuration a deployment legitimately tunes - the counterpart of the reference's TOML keys (gwas/gwas.go:40-117 `Config`; SURVEY section 5: "GPU knobs = new
 * optional TOML keys; defaults must reproduce reference behaviour").  Zero in a field = the library's default.  None of these changes a result word.  The same fields can
 * be given by an operator through the environment (read once, at creation; it overrides this struct): SFG_MM_GROUP, SFG_MM_ACC_BUDGET_MB, SFG_ASSOC_ROTCACHE_MB,
 * SFG_KSW_BUDGET_MB, SFG_ENC_BATCH, SFG_UPLOAD_BLOCKING, SFG_MGPU_TRANSPORT, SFG_MGPU_CACHE_GB, SFG_RCCL_LIB.  Kernel A/B and diagnostic switches are NOT part of this
 * library: they exist in the experimenters' build only (`make -C sfgwas_amd/csrc ab`). */
typedef struct sfg_config {
    uint32_t struct_size;            /* sizeof(sfg_config) of the caller's header (sfg_config_default sets it): lets the struct grow */
    int mm_group;                    /* block rows of the matrix multiplied per MAC launch; 0 = 8, or 10 .. 24 when their operands fit the free HBM */
    size_t acc_budget_bytes;         /* accumulators of the block columns of one pass; 0 = 24 GiB */
    size_t assoc_rotcache_bytes;     /* largest call-wide baby-step rotation cache of an association scan; 0 = 160 GiB; SIZE_MAX = none (rebuilt per batch, as the reference does) */
    size_t ksw_budget_bytes;         /* key-switch scratch per job chunk; 0 = 4 GiB */
    int enc_batch;                   /* diagonals per encode FFT / plaintext-NTT launch pair, 64 .. 8192; 0 = 2048 */
    int upload_blocking;             /* != 0: blocking pointer-table uploads (needed under rocprofv3 --pmc) */
    const char *mgpu_transport;      /* sfg_mgpu_create*_ex: NULL / "rccl" (default) or "direct" (one process only: ranks read their peers' buffers) */
    size_t mgpu_cache_bytes;         /* sfg_mgpu_create*_ex: a rank's own Q'X^T rotation cache up to this size -> per-column pipelined exchange; 0 = 72 GiB; SIZE_MAX = never */
    const char *rccl_lib;            /* sfg_mgpu_create*_ex: library name to dlopen instead of librccl.so.1 */
} sfg_config;
void sfg_config_default(sfg_config *c);
int sfg_ctx_create_ex(sfg_ctx **out, int device, int logN, int nq, int np,
                      const uint64_t *moduli, const uint64_t *psi, double scale, const sfg_config *config /* NULL = defaults */);
/* a second caller on the same keys: replaces checking a private evaluator out of the pool (crypto.go:287-316,
 * ckks.NewEvaluator per goroutine at matmult.go:1110,1200,1371).  Load keys before forks run concurrently. */
int sfg_ctx_fork(sfg_ctx *parent, sfg_ctx **out);
void sfg_ctx_destroy(sfg_ctx *ctx);
const char *sfg_last_error(const sfg_ctx *ctx);     /* ctx may be NULL: error of a failed sfg_ctx_create */
int sfg_ctx_synchronize(sfg_ctx *ctx);
/* returns every scratch buffer the context has grown (plaintext panels, rotation operands, digit streams, accumulators) to the device, after its queues
 * have drained; the next call re-grows what it needs.  For callers that change to a very different product shape beside a large resident matrix.
 * (No reference counterpart: Go's garbage collector plays this role for the accCache / rotCache slices of matmult.go:1065-1129.) */
int sfg_ctx_release_scratch(sfg_ctx *ctx);
/* bytes the context currently keeps in scratch buffers whose name starts with `prefix` ("" = all of them; "assoc.rot8" / "assoc.rotf" = an association scan's
 * rotation cache as int8 tiles / fp64 rows, "mm." = the product's panels, operands and accumulators, "mi8." = the int8 MAC's streams).  Introspection for tests
 * and memory planning; sfg_malloc returns these buffers to the device by itself when a caller's allocation would otherwise fail between library calls. */
int sfg_ctx_scratch_bytes(const sfg_ctx *ctx, const char *prefix, size_t *bytes);
/* sfg_ctx_synchronize waits for every queue of the context (main, own, auxiliary key-switch queue).  It - like sfg_memcpy_d2h and the host-pointer product
 * entry points - FAILS while an encoder coefficient within 2^-50 of a rounding tie is outstanding (see sfg_ctx_encoder_near_ties): results whose
 * bit-exactness with the reference's 256-bit encoder cannot be proven do not leave the device silently. */
/* run all subsequent work of this context on the given hipStream_t, so that a caller can order other work (RCCL collectives, torch ops) against the
 * library.  The handle must be an explicit stream: NULL is HIP's default stream and is refused.  sfg_ctx_use_own_stream returns to the context's own
 * (non-blocking) queue. */
int sfg_ctx_set_stream(sfg_ctx *ctx, void *hip_stream);
int sfg_ctx_use_own_stream(sfg_ctx *ctx);

/* rotation key of one Galois element (cryptoParams.RotKs, crypto.go:50; generated at mhe.go:73, crypto.go:232-275).
 * key_host: [beta][2][nq+np][N], beta = ceil(nq/np), NTT domain; montgomery_form != 0 if the words are in
 * lattigo's Montgomery representation (they are in lattigo's SwitchingKey) */
int sfg_ctx_load_rotkey(sfg_ctx *ctx, uint64_t galois_el, const uint64_t *key_host, int montgomery_form);
int sfg_ctx_has_rotkey(const sfg_ctx *ctx, uint64_t galois_el);
/* copy a loaded key back to the host in normal (non-Montgomery) form, [beta][2][nq+np][N]: lets a CPU checker (bench.py's parity
 * gate) or a CPU-only party work with exactly the key material resident on the device */
int sfg_ctx_export_rotkey(sfg_ctx *ctx, uint64_t galois_el, uint64_t *key_host);
uint64_t sfg_galois_for_rotation(const sfg_ctx *ctx, int k_left);

/* ---- device memory (so ciphertexts / genotypes stay resident across calls) ---- */
int sfg_malloc(sfg_ctx *ctx, void **dev_ptr, size_t bytes);
int sfg_free(sfg_ctx *ctx, void *dev_ptr);
int sfg_memcpy_h2d(sfg_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int sfg_memcpy_d2h(sfg_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int sfg_memcpy_d2d(sfg_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);      /* stream-ordered */

/* ---- ring substrate (lattigo ring.NTT / ring.InvNTT behind crypto/basics.go) ----
 * rows: nrows device rows of N words; mod_idx[r] selects the modulus (0..nq+np-1) of row r (host array) */
int sfg_ntt_rows(sfg_ctx *ctx, uint64_t *rows_dev, int nrows, const int *mod_idx_host);
int sfg_intt_rows(sfg_ctx *ctx, uint64_t *rows_dev, int nrows, const int *mod_idx_host);

/* ---- A1/A2/A4: the lazy MAC (matmult.go:247-399) as a batched modular GEMM ----
 * For every coefficient c < N and modulus l < L:
 *    out[n][r][l][c] (+)= sum_{k<K} rot[k][r][l][c] * pt[k][n][l][c]   mod q_l
 * rot: [K][R][L][N] rotated-ciphertext rows (R = 2*s: (i, poly)), pt: [K][Ncols][L][N] NTT-domain plaintexts
 * (canonical, NOT Montgomery form), out: [Ncols][R][L][N].  accumulate != 0 adds onto out.
 * Net effect of MulCoeffsAndAdd128 + ReduceAndAddUint128 + MForm + eval.Reduce: the canonical sum. */
int sfg_mac_dev(sfg_ctx *ctx, const uint64_t *rot_dev, const uint64_t *pt_dev, uint64_t *out_dev,
                int K, int R, int Ncols, int L, int accumulate);

/* Test hook (refused unless SFG_ENABLE_TEST_HOOKS=1 was set before sfg_ctx_create): the SAME sum through the kernels a product multiplies with by default -
 * the int8 matrix-core MAC of mac_i8.hip (five signed base-256 digits for moduli < 2^36, six for moduli < 2^47; transposition kernels, ring / cache kernel by
 * column count, Horner recombination, untile), reached exactly as sfg_matmul_* reaches it.  Those kernels serve the mirror-symmetric plaintexts a real slot
 * vector encodes to (P[N-1-x] = P[x]) from half rows: pt_half_dev is [K][Ncols][L][N/2] canonical words, the result is
 *    out[n][r][l][x] (+)= sum_k rot[k][r][l][x] * pt_half[k][n][l][min(x, N-1-x)]   mod q_l.
 * pt_form 0: the plaintext rows are first written as the digit planes the product's plaintext NTT emits (k_i8_pack_pt_digits); 1: as panel words - packed
 * limbs / plain words - the DiagCache product's form (k_i8_pack_pt).  Ncols <= 96, K < 21846.  Replaces nothing in the reference: it exists so that
 * matmult.go:247-324's arithmetic can be checked against the default kernels directly (tests/test_gpu_mac.py). */
int sfg_mac_i8_dev(sfg_ctx *ctx, const uint64_t *rot_dev, const uint64_t *pt_half_dev, uint64_t *out_dev,
                   int K, int R, int Ncols, int L, int accumulate, int pt_form);

/* Test hook (refused unless SFG_ENABLE_TEST_HOOKS=1 was set before sfg_ctx_create): the int8 MAC's plaintext transposition by itself, through the launches a
 * product makes (i8_ride_prepare, launch_i8_pack_pt_digits, launch_move_alone, launch_ntt_plain_half with mover workgroups, i8_ride_finish; mac_i8.hip).
 * panel_dev: the caller's digit-plane panel of K rows x Ncols columns x the first L moduli, panel_bytes long, in layout 0 (rows of N/2 words, planes first;
 * pt_k / pt_n = words between consecutive k / columns), 1 (compact: a plaintext's planes back to back; same strides) or 2 (K-major
 * [column][plane][128-byte block][k < K][128 B]; strides ignored).  The mover addresses rows up to the end of the last 64-row chunk, so the panel must reach
 * that far (layout 2: (64 ceil(K/64) - K) * 128 bytes past its last plane); the hook refuses a shorter one.  It fills the tile buffers and 4096 guard bytes behind
 * each with `sentinel`, then transposes by
 *   mode 0  the pass (k_i8_pack_pt_digits) over every item;
 *   mode 1  one launch of a2 mover workgroups alone over items [a0, a0 + a1);
 *   mode 2  the ride: i8_ride_prepare for a0 predicted NTT launches and a1 mover workgroups (a multiple of 8), then a2 <= 11 plaintext-NTT launches of 8
 *           plaintexts each (coefficients pc_host [a2 * 8][N/2] doubles, digit-plane K-major form, into a scratch second panel of one 91-row column that was
 *           filled with `sentinel`), each carrying the slice launch_encode_rows would give it, then i8_ride_finish.  no_mover != 0: the same NTT launches and
 *           nothing else.
 * and copies back tiles_small_host (n_small * (N/2) * ceil(Ncols/16) * ceil(K/64) * 5 * 1024 bytes + 4096; *_cap = the buffer's size), tiles_big_host (the same
 * with 6 for the one modulus above 2^36, if any) and, in mode 2, panel2_host (planes * 64 * 91 * 128 bytes).  info[8]: [0] 1 if the ride was prepared - 0 means
 * it declined (no 35-bit modulus, a six-digit modulus above the int8 range, offsets beyond 32 bits) and NOTHING was launched or written; [1] items the leftover
 * launch of i8_ride_finish took; [2], [3] five- and six-digit items; [4] items per NTT launch; [5] 35-bit moduli, [6] the first of them, [7] the big one or -1. */
int sfg_i8_move_for_test(sfg_ctx *ctx, const uint64_t *panel_dev, size_t panel_bytes, int layout, size_t pt_k, size_t pt_n, int K, int Ncols, int L,
                         int mode, int a0, int a1, int a2, int no_mover, const double *pc_host, int sentinel,
                         uint8_t *tiles_small_host, size_t small_cap, uint8_t *tiles_big_host, size_t big_cap, uint8_t *panel2_host, size_t panel2_cap, int *info);

/* ---- A6/A7: diagonal extraction + CKKS encode (matmult.go:636-731, EncodeNTT) ----
 * Encodes the generalized diagonals `shift` in [shift0, shift0+nshift) of one <= slots x slots int8 block
 * (block rows r, cols c, row stride ld; transposed != 0 reads the block transposed), each right-rotated by
 * d*(shift/d), into NTT-domain plaintexts for moduli 0..L-1: pt_dev[nshift][L][N] canonical residues.
 * Genotype values must already be cleaned (missing -> 0; squared if requested). */
int sfg_encode_diags_dev(sfg_ctx *ctx, const int8_t *block_dev, size_t ld, int r, int c, int transposed,
                         int shift0, int nshift, int L, uint64_t *pt_dev);
/* coefficient-domain result of the encoder for arbitrary real slot vectors (host convenience used by
 * Mask/MaskTrunc-style callers, basics.go:110-172): values_host[nvec][slots] -> coeffs_host[nvec][N] int64.
 * Domain (both real-slot entry points): finite slot values with |Delta w_c| < 2^53 for every coefficient - there every coefficient is the exactly
 * rounded integer (half away from zero).  A NaN / inf value, or a coefficient of magnitude 2^53 or more, fails the call (the message names the
 * cause) and leaves the output undefined; nothing is returned as words. */
int sfg_encode_coeffs_host(sfg_ctx *ctx, const double *values_host, int nvec, int64_t *coeffs_host);
/* Rounding audit of the encoder.  The reference rounds Delta * sigma^-1(v) computed with 256-bit big floats (NewEncoderBig(params, 256),
 * matmult.go:1019,1421); the device computes the same reals in double-double (better than 2^-58 absolute here).  The two can only round a
 * coefficient differently when its exact value lies within that distance of a tie; every coefficient within 2^-40 of a tie is counted
 * per context.  count == 0 after a call proves that call's plaintexts are the reference's, bit for bit; a non-zero count (expected
 * about once per 2 * 10^11 coefficients) is informational - the pipeline's own error is ~2^-59.  A coefficient within 2^-50 of a tie (about once per
 * 10^15) is NOT tolerated: every synchronising entry point fails until the counters are reset, and the affected products must be re-derived with a
 * big-float encoder on the host. */
int sfg_ctx_encoder_near_ties(sfg_ctx *ctx, unsigned long long *count, int reset);
/* Round 4: a genotype-diagonal coefficient inside the 2^-50 band is RE-DERIVED on the device before it can fail anything: p_j = (Delta/n) sum_t v_t cos(2 pi 5^t j / 2N)
 * is summed exactly - small integers times 100-bit fixed-point cosines, integer accumulation - so only the cosine table's error (< 2^-68 of a unit) is left, and a sum
 * farther than 2^-62 from the tie proves its rounding and replaces the double-double value (sfg_ctx_encoder_resolved counts them).  What stays unproven - closer than
 * 2^-62 (about once per 10^18 coefficients), a second such coefficient among the 16 - 20 one lane rounds, real-valued slot rows (sfg_encode_vectors_dev) - fails as
 * described.  Cost: 1.4 % of the encode FFT (the re-derivation is a non-inlined serial loop at the kernel's end; same-box A/B in profiles/r04_fft_resolver_ab.txt). */
int sfg_ctx_encoder_resolved(sfg_ctx *ctx, unsigned long long *count);
/* the coefficients within 2^-50 of a tie seen since the last reset that could NOT be proven (the condition that makes the synchronising entry points fail) */
int sfg_ctx_encoder_unprovable(sfg_ctx *ctx, unsigned long long *count);
/* With a plaintext coefficient cache on (sfg_geno_set_plaintext_cache) a cached row was audited when it was FILLED: "count == 0" then proves the plaintexts
 * of the calls since the cache was enabled.  When the 2^-50 condition is reported (a failing synchronising call) or reset, every cache the context owns
 * forgets its rows, so the recovery never keeps serving a row that was filled while the condition was outstanding. */
/* test hook for the failure path above: marks n coefficients as too close to a tie.  Refused unless the process set SFG_ENABLE_TEST_HOOKS=1 before
 * sfg_ctx_create (a production caller cannot wedge a context with it by accident). */
int sfg_ctx_encoder_inject_unsafe_for_test(sfg_ctx *ctx, unsigned long long n);
/* crypto.EncodeFloatVector (crypto.go:398-420; behind Mask / MaskTrunc / MaskWithScaling, basics.go:110-172, and
 * CPMult operands): nvec real slot vectors [nvec][slots] (host) -> NTT-domain plaintexts pt_dev[nvec][level+1][N]
 * at the context's default scale. The reference encodes at MaxLevel; a product at a lower level reads the first rows.
 * Same domain as sfg_encode_coeffs_host; out of it (or for a NaN / inf value) the call fails. */
int sfg_encode_vectors_dev(sfg_ctx *ctx, const double *values_host, int nvec, int level, uint64_t *pt_dev);

/* ---- C1/A8: rotations (crypto/basics.go:201-224 -> ckks.Evaluator.RotateNew) ----
 * batch of nct ciphertexts at `level`, each [2][level+1][N]; ct j is rotated RIGHT by nrot_host[j]
 * (RotateRightWithEvaluator semantics: nrot mod slots, 0 = copy). in/out may not alias. */
int sfg_rotate_right_dev(sfg_ctx *ctx, const uint64_t *ct_in_dev, uint64_t *ct_out_dev, int nct, int level,
                         const int *nrot_host);
/* eval.ConjugateNew behind crypto.ComplexConjugate / CReal (basics.go:826-846): the automorphism X -> X^galois_el with the switching key loaded
 * under that element by sfg_ctx_load_rotkey (lattigo's conjugation key: galois element 2N-1).  Batch of nct ciphertexts; in/out may not alias. */
int sfg_ct_galois_dev(sfg_ctx *ctx, const uint64_t *ct_in_dev, uint64_t *ct_out_dev, int nct, int level, uint64_t galois_el);
/* C4: element-wise ciphertext add (eval.Add, basics.go:174, matmult.go:1225,1494): out = a + b */
int sfg_ct_add_dev(sfg_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int nct, int level);
/* C4: eval.Sub (crypto.CSub, basics.go:575-590): out = a - b */
int sfg_ct_sub_dev(sfg_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int nct, int level);

/* C6: crypto.DropLevel -> eval.DropLevelNew (basics.go:806-824; FlattenLevels :514-531 drops a matrix to its minimum level):
 * in [nct][2][level_in+1][N] -> out [nct][2][level_out+1][N].  level_out == level_in copies (CopyNew); level_out > level_in fails. */
int sfg_ct_drop_level_dev(sfg_ctx *ctx, const uint64_t *in_dev, uint64_t *out_dev, int nct, int level_in, int level_out);

/* C4: eval.MultByConst / AddConst / AddNew(ct, plaintext) behind crypto.CMultConst, CMultConstRescale, AddConst, CAddConst,
 * AddPlain, CPAdd (basics.go:183-199, 472-497, 533-551, 592-611). scalars_host[level+1]: one canonical residue per modulus
 * (lattigo scaleUpExact(constant, scale, q_m); the host side owns that rule and the scale bookkeeping). out may alias ct. */
int sfg_ct_mul_scalar_dev(sfg_ctx *ctx, const uint64_t *ct_dev, const uint64_t *scalars_host, uint64_t *out_dev, int nct, int level);
/* eval.MultByConstAndAdd (pca.go:264; qrfact.go:195,280): acc += ct * scalars[m], both polynomials, acc and ct at the same level.  The scale
 * matching lattigo performs first (MultByConst of the receiver by floor(scale ratio), SetScale) is host-side: crypto::MultByConstAndAddDev. */
int sfg_ct_mul_scalar_add_dev(sfg_ctx *ctx, const uint64_t *ct_dev, const uint64_t *scalars_host, uint64_t *acc_dev, int nct, int level);
int sfg_ct_add_scalar_dev(sfg_ctx *ctx, const uint64_t *ct_dev, const uint64_t *scalars_host, uint64_t *out_dev, int nct, int level);
int sfg_ct_add_plain_dev(sfg_ctx *ctx, const uint64_t *ct_dev, const uint64_t *pt_dev, size_t pt_stride, uint64_t *out_dev,
                         int nct, int level);

/* ---- C3: ciphertext products (crypto.CMult / CPMult / Mask, basics.go:110-172, 386-470) ----
 * The relinearisation key (cryptoParams.Rlk, crypto.go:47) has the same layout as a rotation key:
 * [beta][2][nq+np][N], montgomery != 0 if in lattigo's stored Montgomery form. */
int sfg_ctx_load_relinkey(sfg_ctx *ctx, const uint64_t *key_host, int montgomery);
/* eval.MulRelinNew(a, b): degree-2 tensor product + relinearisation, batch of nct pairs; level unchanged, scale = product.
 * No rescale (call sfg_ct_rescale_dev, as CMult does at basics.go:394). out may alias neither input. */
int sfg_ct_mulrelin_dev(sfg_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int nct, int level);
/* eval.MulRelinNew(plaintext, ct): both polynomials times an NTT-domain plaintext [level+1][N]; ct j uses
 * pt_dev + j*pt_stride words (pt_stride 0 = one plaintext for all, e.g. a Mask). out may alias ct. */
int sfg_ct_mul_plain_dev(sfg_ctx *ctx, const uint64_t *ct_dev, const uint64_t *pt_dev, size_t pt_stride, uint64_t *out_dev,
                         int nct, int level);
/* one step of eval.Rescale = ring.DivRoundByLastModulusNTT on both polynomials: in [nct][2][level+1][N] ->
 * out [nct][2][level][N] (level-1); the caller divides the scale by q_level. Fails at level 0 like lattigo. */
int sfg_ct_rescale_dev(sfg_ctx *ctx, const uint64_t *in_dev, uint64_t *out_dev, int nct, int level);
/* C2: crypto.InnerSumAll (basics.go:278-292): sum of the nct ciphertexts and of all their slots, in every slot of the one
 * output ciphertext. Needs the rotation keys for left rotations by 1,2,4,..,slots/2. */
int sfg_ct_innersum_dev(sfg_ctx *ctx, const uint64_t *in_dev, int nct, int level, uint64_t *out_dev);

/* ---- F1 + A11: genotype matrix residency (replaces GenoFileStream reads + the DiagCache of
 * MatMult4StreamPreprocess, matmult.go:914-1041; filestream.go:284-494).
 * geno: nrow x ncol int8 row-major (row stride ld), -1 = missing.  The handle keeps ONE int8 copy in HBM
 * that serves both X (transpose = 0) and X^T (transpose = 1) products. */
int sfg_geno_upload(sfg_ctx *ctx, const int8_t *geno_host, size_t nrow, size_t ncol, size_t ld, sfg_geno **out);
int sfg_geno_from_device(sfg_ctx *ctx, const int8_t *geno_dev, size_t nrow, size_t ncol, size_t ld, sfg_geno **out);
void sfg_geno_free(sfg_ctx *ctx, sfg_geno *g);
/* Row-streamed registration.  The reference never holds its matrix: MatMult4StreamPreprocess (gwas/matmult.go:914-1041) pulls ONE ROW at a time out of
 * GenoFileStream.NextRow (gwas/filestream.go:414-426).  sfg_geno_create makes the resident nrow x ncol matrix (contents undefined until written),
 * sfg_geno_write_rows copies rows [row0, row0 + nrows) from a host chunk (row stride ld; the call returns when the chunk may be refilled), so a caller needs a
 * staging buffer of a few thousand rows and nothing that scales with nrow * ncol.  sfg_geno_compare_rows compares a chunk of the rows of the matrix arriving now
 * with the RESIDENT matrix `g` viewed with `flags` (0, or SFG_TRANSPOSE: the rows of its transpose) on the device, entry by entry, and ADDS the number of
 * differing entries to *ndiff: that is how the second registration of pca.go:112-113 (X, then X^T from its own file) is recognised as a view of the first
 * without X^T being held anywhere - exactly, not by a hash.  sfg_pinned_alloc / _free: page-locked host memory for the staging buffer (optional). */
int sfg_geno_create(sfg_ctx *ctx, size_t nrow, size_t ncol, sfg_geno **out);
int sfg_geno_write_rows(sfg_ctx *ctx, sfg_geno *g, size_t row0, size_t nrows, const int8_t *rows_host, size_t ld);
int sfg_geno_compare_rows(sfg_ctx *ctx, const sfg_geno *g, unsigned flags, size_t row0, size_t nrows, const int8_t *rows_host, size_t ld, uint64_t *ndiff);
int sfg_pinned_alloc(sfg_ctx *ctx, void **host_ptr, size_t bytes);
int sfg_pinned_free(sfg_ctx *ctx, void *host_ptr);
/* Plaintext coefficient cache of a resident matrix - the device-memory counterpart of the reference's on-disk DiagCache (MatMult4StreamPreprocess,
 * gwas/matmult.go:1228-1334, read back per iteration at :1386-1400).  After this call the products over `g` keep, per 8192 x 8192 block (and per SFG_SQUARE
 * flavour), the encoder's rounded coefficient rows (512 MB) until max_bytes are held; a later product over a cached block - in EITHER orientation: the
 * diagonals of the transposed block are slot rotations of the cached ones, i.e. automorphism images of the cached plaintexts - skips the skew and the FFT and
 * produces the same words.  max_bytes = 0 drops the cache.  The matrix must not change while cached; only `ctx` may multiply with `g` meanwhile.
 * sfg_geno_plaintext_cache_stats: blocks held, bytes held, block encodes served from the cache, blocks filled (any pointer may be NULL). */
int sfg_geno_set_plaintext_cache(sfg_ctx *ctx, const sfg_geno *g, size_t max_bytes);
int sfg_geno_plaintext_cache_stats(sfg_ctx *ctx, const sfg_geno *g, size_t *blocks, size_t *bytes, size_t *hits, size_t *fills);
/* Input pipeline on the device (replaces the per-batch shell-outs of assoc.go:389 to the Python converters under scripts/):
 * scripts/plinkBedToBinary.py + filterMatrix.py: `bed_host` is a whole SNP-major PLINK .bed image (3 magic bytes +
 * ceil(num_sample/4) bytes per SNP; codes 00->2, 01->-1, 10->1, 11->0); rows (samples) / columns (SNPs) whose filter
 * byte is zero are dropped (nullptr = keep all). Result: resident sample-major int8 matrix. Fails on a size mismatch
 * (the script's assert) or wrong magic. */
int sfg_geno_from_bed(sfg_ctx *ctx, const uint8_t *bed_host, size_t bed_bytes, size_t num_sample, size_t num_snp,
                      const uint8_t *row_filter, const uint8_t *col_filter, sfg_geno **out);
/* PLINK 2 .pgen hard calls (the reference's shipped example data, config 1): replaces gwas/utilities.go:141 FilterMatrixFilePgen ->
 * scripts/filterMatrixPgen.sh:12-18 (plink2 --pfile --keep --extract --indiv-sort none --make-bed, then plinkBedToBinary.py) for variants [v0, v1)
 * of one file (v1 = 0: all).  pgen_host: the whole .pgen image (storage mode 0x10 or 0x02; hard calls only).  row_filter: one byte per sample of the
 * .psam (the --keep list as a mask), col_filter: one byte per variant of [v0, v1) (the --extract list), zero = drop, NULL = keep all.
 * Result: resident sample-major int8 (ALT allele count, missing = -1), i.e. the bytes of the temporary file GenoFileStream would read. */
int sfg_pgen_dims(sfg_ctx *ctx, const uint8_t *pgen_host, size_t pgen_bytes, size_t *num_sample, size_t *num_variant);
int sfg_geno_from_pgen(sfg_ctx *ctx, const uint8_t *pgen_host, size_t pgen_bytes, size_t v0, size_t v1,
                       const uint8_t *row_filter, const uint8_t *col_filter, sfg_geno **out);
/* scripts/preprocessing/computeGenoCounts.py (plink2 --keep --geno-counts, columns 5-10; the file behind geno_count_file, read at
 * gwas/qualcontrol.go:595): counts_host[6][num_variant] uint32 = HOM_REF_CT, HET_REF_ALT_CTS, TWO_ALT_GENO_CTS, HAP_REF_CT, HAP_ALT_CTS, MISSING_CT */
int sfg_pgen_geno_counts(sfg_ctx *ctx, const uint8_t *pgen_host, size_t pgen_bytes, const uint8_t *row_filter, uint32_t *counts_host);
/* 2-bit packed residency (c4 is 25 GB instead of 100 GB; c5 fits 8 GPUs): codes 0, 1, 2 = the genotype, 3 = missing, 4 columns per byte.
 * Every product entry point takes a packed handle (blocks are expanded on the fly, ~1 % of a block's time); results are bit-identical.  Fails if a
 * value above 2 is present (the int8 layout stays available for such matrices).  Free the int8 handle afterwards to release its memory. */
int sfg_geno_pack(sfg_ctx *ctx, const sfg_geno *g, sfg_geno **out);
int sfg_geno_unpack(sfg_ctx *ctx, const sfg_geno *g, sfg_geno **out);
int sfg_geno_dims(const sfg_geno *g, size_t *nrow, size_t *ncol);
/* how a handle lies in device memory: *dev = its first byte, *ld = the row stride in BYTES (int8: >= ncol; packed: 4 columns per byte, a multiple of 4),
 * *packed = 1 for 2-bit codes (any pointer may be NULL).  For INSPECTION and interoperability only - a test that reads the padding of a row, a caller that hands
 * the matrix to a kernel of its own: the memory stays the library's (or, for sfg_geno_from_device, the caller's, as before), it is read-only to the caller, the
 * pointer dies with the handle, and no library call takes such a pointer back as a matrix (sfg_geno_from_device wants memory the caller owns). */
int sfg_geno_layout(const sfg_geno *g, const void **dev, size_t *ld, int *packed);
/* host [nrow][ncol] copy of a resident matrix (interoperability with CPU-only parties, tests) */
int sfg_geno_download(sfg_ctx *ctx, const sfg_geno *g, int8_t *host);
/* scripts/transposeMatrix.py as a materialised copy (the products themselves use SFG_TRANSPOSE on the one copy) */
int sfg_geno_transpose(sfg_ctx *ctx, const sfg_geno *g, sfg_geno **out);
/* scripts/mergeMatrices.py: column-wise concatenation of k resident matrices with equal row counts */
int sfg_geno_concat_cols(sfg_ctx *ctx, const sfg_geno *const *parts, int k, sfg_geno **out);
/* P2: per-column sum / sum of squares after missing->0 (matmult.go:1292-1300); either may be NULL */
int sfg_geno_colsums(sfg_ctx *ctx, const sfg_geno *g, double *sum_host, double *sqsum_host);
/* ---- quality control on the resident matrix (qcscan.hip): the three local passes of gwas/qualcontrol.go in ONE pass over the matrix bytes ----
 * replaces the genotype loops of SNPMissFilter (qualcontrol.go:339-378), IndividualMissAndHetFilters (qualcontrol.go:36-81) and SNPMAFAndHWEFilters
 * (qualcontrol.go:416-463); their secure comparisons stay in Go.  Only entries (i, j) with row_filter[i] != 0 and col_filter[j] != 0 are looked at (a NULL
 * filter keeps all); row_ctrl[i] != 0 marks the control cohort (the reference's pheno < 1), NULL = no controls.  Outputs, any of which may be NULL (not all):
 *   col_counts_host [2][4][ncol] uint32: [c][k][j] = kept rows of cohort c (0: all kept rows, 1: the kept controls) whose entry in column j is k = 0, 1, 2
 *                                        or (k = 3) missing: any negative int8 / packed code 3
 *   row_miss_host / row_het_host [nrow]: missing entries / entries equal to 1 of row i over the kept columns
 * indexed by ORIGINAL position; a dropped row or column has zeros.  Per cohort the reference's xCount = 2 (n0 + n1 + n2), xSum = n1 + 2 n2,
 * genoObservedCtrl[k] = n_k of cohort 1, and SNPMissFilter's count is n0 + n1 + n2 of cohort 0.  An int8 value above 2 at a kept position fails the call (the
 * message names how many; the reference would panic at genoObservedCtrl[snp]); at a dropped position it is not looked at.  A packed handle is scanned in place.
 * The matrix is read once whichever outputs are asked for; temporaries are O(nrow + ncol) ("qc." scratch).  Synchronising.  g == NULL or no output: an error that
 * launches nothing. */
int sfg_geno_qc_scan(sfg_ctx *ctx, const sfg_geno *g, const uint8_t *row_filter, const uint8_t *col_filter, const uint8_t *row_ctrl,
                     uint32_t *col_counts_host, uint32_t *row_miss_host, uint32_t *row_het_host);
/* the filtered matrix as a new owned resident handle: replaces FilterMatrixFile (gwas/utilities.go:154 -> scripts/filterMatrix.py) and the lazy row / column
 * filters of the GenoFileStreams (gwas/gwas.go:545 GeneratePCAInput reads through them) for a matrix that is already in HBM.  Kept rows and columns in order;
 * int8 in -> int8 out, packed in -> packed out (codes re-packed across the dropped columns, padding codes 0, no int8 intermediate).  Both filters NULL: a copy.
 * Filters that keep nothing: an error that allocates nothing. */
int sfg_geno_filter(sfg_ctx *ctx, const sfg_geno *g, const uint8_t *row_filter, const uint8_t *col_filter, sfg_geno **out);

/* ---- A9/A10: the full product (MatMult4Stream matmult.go:1238-1505, MatMult4StreamCompute :1043-1236) ----
 * A: s x nbr ciphertexts [s][nbr][2][in_level+1][N] (nbr = ceil(rows/slots) of the operand orientation);
 * out: s x m_ct ciphertexts [s][m_ct][2][max_level][N] at level max_level-1, scale = A.scale * Params.Scale().
 * The result is the deterministic sum over giant steps; the reference adds it onto a fresh encryption of zero
 * (CZeroMat, matmult.go:1174,1443): sfg_ct_add_fresh_zero_dev does that on the device when a public key is loaded, else the Go shim keeps doing it.
 * flags: SFG_SQUARE squares genotypes after missing->0 (matmult.go:1301-1303); SFG_TRANSPOSE multiplies by X^T. */
#define SFG_SQUARE 1u
#define SFG_TRANSPOSE 2u
#define SFG_STREAM_DIRECT 4u      /* sfg_assoc_stream_bed only: read the file with O_DIRECT (4096-byte aligned ranges, no page cache) */
int sfg_matmul_resident_dev(sfg_ctx *ctx, const uint64_t *A_dev, int s, int in_level, int max_level,
                            const sfg_geno *g, unsigned flags, uint64_t *out_dev);
/* MatMult4StreamCompute on the reference's OWN on-disk cache (matmult.go:1043-1236 reading the DiagCache files that
 * MatMult4StreamPreprocess of a CPU party wrote, filestream.go:19-282): files <prefix>_<bi>.bin for bi < nbr hold NTT + Montgomery-form
 * plaintexts as big-endian words; they are streamed, converted on the device and multiplied without re-encoding.  out: s x vectorLen
 * ciphertexts, as sfg_matmul_resident_dev.  Fails like the reference when a file is missing (os.Open panics, filestream.go:59-61).
 * Header fields are validated against the ring and the file size before anything is allocated.  Records are expected in the order
 * MatMult4StreamPreprocess writes them (increasing shift, matmult.go:1001-1035): the records of one giant step then form ONE MAC launch; any
 * other order still gives the right sums, at one upload + launch per change of giant step. */
int sfg_matmul_from_cache(sfg_ctx *ctx, const uint64_t *A_dev, int s, int in_level, int max_level, const char *cache_prefix, int nbr, uint64_t *out_dev);
/* MatMult4StreamPreprocess with its on-disk result (gwas/matmult.go:914-1041): writes <prefix>_<bi>.bin for every block row of the (optionally transposed)
 * resident matrix in the reference's DiagCacheStream format (filestream.go:144-231: 6 x u64 LE header, 2 d table bytes, per active shift u64 LE length,
 * u32 LE shift, per block column u8 isEmpty + (max_level + 1) x N words, NTT + Montgomery form, big-endian) from diagonals encoded ON THE DEVICE - for
 * interoperability with CPU-only parties and for sfg_matmul_from_cache.  Existing files are kept, as the reference keeps them (:928-931); records are in
 * increasing shift (the reference's worker pool delivers them in nearly that order; every reader takes them in any order).  96 bytes per genotype:
 * a 10 000 x 100 000 matrix makes 96 GB - the resident int8 matrix is the default for a reason.  *files_written (optional): files created by this call. */
int sfg_diagcache_write(sfg_ctx *ctx, const sfg_geno *g, unsigned flags, int max_level, const char *cache_prefix, int *files_written);
/* header of <prefix>_<block_row>.bin: {vectorLen (= block columns), level, scale (f64 bits), n, numModuli, rowSize} */
int sfg_diagcache_header(sfg_ctx *ctx, const char *cache_prefix, int block_row, uint64_t hdr[6]);
/* host-pointer form, one call = MatMult4Stream(cps, A, gfs, maxLevel, computeSquaredSum, square, nproc) */
int sfg_matmul_stream(sfg_ctx *ctx, const uint64_t *A_host, int s, int in_level, int max_level,
                      const int8_t *geno_host, size_t nrow, size_t ncol, size_t ld, unsigned flags,
                      uint64_t *out_host, double *sum_host, double *sqsum_host);
/* ---- f-3: the association scan's batches streamed from storage (gwas/assoc.go:340-420, GenoBlockMult; BASELINE config 5) ----
 * Replaces, per batch of `batch_snps` KEPT SNPs: FilterMatrixFilePgen (plink2 and the Python converters under scripts/ writing an int8 temp file), NewGenoFileStream,
 * MatMult4Stream(cps, mat, X, 5, false, square, nproc) and the final crypto.ConcatCipherMatrix.  `bed_path` is a SNP-major PLINK .bed of
 * num_sample x num_snp (a .pgen is converted once with plink2 --make-bed); row_filter / col_filter: one byte per sample / SNP, zero = drop, NULL = keep
 * all.  A batch is one contiguous byte range of the file: read by a reader thread into pinned memory while the GPU multiplies the previous batch,
 * moved to HBM as packed 2-bit codes, decoded / filtered / transposed on the device.  A_dev: [s][ceil(kept_samples / slots)] ciphertexts;
 * out_dev: [s][out_ct_capacity][2][max_level][N]; *out_ct = sum over batches of ceil(kept / slots).  sum_host / sqsum_host (optional):
 * [*out_ct * slots] column sums in the reference's padded layout (dosageSum[outShift + c], assoc.go:404-405).  flags: SFG_SQUARE, SFG_STREAM_DIRECT.
 * The baby-step rotation cache of `A` (rotCache[i][baby], matmult.go:1373-1377 - a function of A alone, rebuilt by the reference in every MatMult4Stream
 * call) is built ONCE per call and shared by all batches when it fits (SFG_ASSOC_ROTCACHE_MB, 0 = per batch): as the int8 MAC's rot tiles where every
 * modulus multiplies on the matrix core (1.3 GB per block row for s <= 15), else as fp64 operand rows (1.86 GB per block row at s = 13).
 * The cache and the call's staging buffers (two pinned file slots of one batch each, the decoded batches) stay in the context's scratch pools for the next
 * call of the scan (sfg_ctx_scratch_bytes(ctx, "assoc.", ..); sfg_ctx_release_scratch returns them).
 * A Go shim that keeps calling per batch gets the same saving from sfg_rotcache_build_rows_dev + sfg_matmul_resident_range_rc_dev. */
int sfg_assoc_stream_bed(sfg_ctx *ctx, const char *bed_path, size_t num_sample, size_t num_snp, const uint8_t *row_filter, const uint8_t *col_filter,
                         size_t batch_snps, const uint64_t *A_dev, int s, int in_level, int max_level, unsigned flags,
                         uint64_t *out_dev, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host);
/* the same scan over one chromosome's .pgen image - BASELINE config 1's path (assoc.go:371-416 with isPgen): per batch of `batch_snps` kept variants
 * FilterMatrixFilePgen (plink2 + plinkBedToBinary.py) + MatMult4Stream, decoded natively on the device (sfg_geno_from_pgen).  row_filter: one byte per
 * sample (the --keep list), col_filter: one byte per variant of the file (snpFilt).  Layout of out_dev / sum_host / sqsum_host as above. */
int sfg_assoc_pgen(sfg_ctx *ctx, const uint8_t *pgen_host, size_t pgen_bytes, const uint8_t *row_filter, const uint8_t *col_filter, size_t batch_snps,
                   const uint64_t *A_dev, int s, int in_level, int max_level, unsigned flags,
                   uint64_t *out_dev, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host);
/* ... and straight from the .pgen on disk (config 5: 10 M SNPs per party, the file does not fit host memory as one image): the header tables are read once,
 * every batch is the contiguous byte range of its variant records (plus the LD base its first records may need), read ahead by a reader thread into pinned
 * memory (SFG_STREAM_DIRECT: O_DIRECT) while the GPU works on the previous batch.  Sample and variant counts come from the file's header. */
int sfg_assoc_stream_pgen(sfg_ctx *ctx, const char *pgen_path, const uint8_t *row_filter, const uint8_t *col_filter, size_t batch_snps,
                          const uint64_t *A_dev, int s, int in_level, int max_level, unsigned flags,
                          uint64_t *out_dev, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host);
/* sharding hooks for one-process-per-GPU runs: restrict a resident product to block columns
 * [j0, j1) of the output (X: SNP-column blocks) or block rows [b0, b1) of the contraction (X^T) */
int sfg_matmul_resident_range_dev(sfg_ctx *ctx, const uint64_t *A_dev, int s, int in_level, int max_level,
                                  const sfg_geno *g, unsigned flags, int blk0, int blk1, uint64_t *out_dev);
/* two-phase form of the same product, for contraction-sharded (X^T) multi-GPU runs.  Key switching is not
 * bit-linear, so partial sums must be combined BEFORE the giant-step rotations to stay bit-exact with the reference:
 *   accumulate: acc[(j-j0)][giant < 91][i < s][2][max_level][N] (+)= sum over operand block rows [b0,b1) and baby steps
 *   (ranks then reduce-scatter / all-reduce acc as uint64 and call sfg_reduce_rows_dev)
 *   finalize:   out[i][j][2][max_level][N] (+)= sum_{giant in [g0,g1)} RotateRight(acc[j][giant][i], -giant*91)
 *               (matmult.go:1443-1502); out has ncolb block columns */
int sfg_matmul_accumulate_dev(sfg_ctx *ctx, const uint64_t *A_dev, int s, int in_level, int max_level,
                              const sfg_geno *g, unsigned flags, int b0, int b1, int j0, int j1,
                              int accumulate, uint64_t *acc_dev);
int sfg_matmul_finalize_dev(sfg_ctx *ctx, const uint64_t *acc_dev, int s, int max_level, int ncolb,
                            int g0, int g1, int accumulate, uint64_t *out_dev);
/* finalize for a rank of a giant-sharded run: acc_dev is [ncolb][acc_giants][s][2][max_level][N] and slot g of a block column holds
 * giant step giant_base + g (what a reduce-scatter over the giant axis leaves on each rank); slots [g0, g1) are aligned, giant steps
 * >= 91 ignored */
int sfg_matmul_finalize_slots_dev(sfg_ctx *ctx, const uint64_t *acc_dev, int s, int max_level, int ncolb, int acc_giants, int giant_base,
                                  int g0, int g1, int accumulate, uint64_t *out_dev);
/* ---- the baby-step rotation cache as an object (SURVEY.md §8e "builds the full rotation cache (or the rotation cache is built once and
 * broadcast)"): rotCache[i][baby] = RotateRightWithEvaluator(A[i][bi], -baby) of matmult.go:1083-1119,1373-1377 in the MAC's fp64 operand layout
 *     cache[bi - row0][baby < 91][i < s][poly < 2][rowf doubles]   followed by tail_doubles zeros,   job_doubles = 91 * 2 * rowf.
 * Every rank of the output-sharded product Q*X multiplies by the cache of ALL operand block rows; rank r key-switches only the inputs
 * (bi, i) of its job range (job = bi*s + i: the decomposition of an input is shared by its 91 rotations) into job-major staging
 *     staged[job - job0][baby][poly][rowf],
 * the ranks all-gather the staging buffers and scatter them into the cache layout.  All 91 baby steps are rotated (rotations the reference's
 * active-baby table would skip meet zero plaintexts only), so every baby rotation key must be loaded (crypto.go:252-263 generates them all).
 * The MAC keeps a transposed copy of the operand it last multiplied with, keyed by the cache pointer, its shape and strides, and a PER-CONTEXT generation
 * count that sfg_rotcache_scatter_dev / sfg_rotcache_build_rows_dev advance on the context they run on.  A cache buffer written by any other route - a
 * collective straight into the layout, a device copy of a saved cache, a build on ANOTHER (forked) context - must be announced to the multiplying context
 * with sfg_rotcache_invalidate before its next *_rc_dev product, or that product may read the stale copy. */
int sfg_rotcache_invalidate(sfg_ctx *ctx);
int sfg_rotcache_layout(sfg_ctx *ctx, int s, int max_level, size_t *job_doubles, size_t *tail_doubles);
int sfg_rotcache_build_jobs_dev(sfg_ctx *ctx, const uint64_t *A_dev, int s, int in_level, int max_level, int nbr, int job0, int job1, double *staged_dev);
/* staged jobs [job0, job1) -> cache rows [row0, row0 + nrows); also zeroes the tail */
int sfg_rotcache_scatter_dev(sfg_ctx *ctx, const double *staged_dev, int s, int max_level, int job0, int job1, int row0, int nrows, double *cache_dev);
/* the cache of block rows [b0, b1) written in place (a rank's own rows of the contraction-sharded product Q'*X^T) */
int sfg_rotcache_build_rows_dev(sfg_ctx *ctx, const uint64_t *A_dev, int s, int in_level, int max_level, int nbr, int b0, int b1, double *cache_dev);
/* sfg_matmul_resident_range_dev / sfg_matmul_accumulate_dev on a prebuilt cache that covers exactly the operand block rows the call contracts
 * over (X: all of them; X^T: [blk0, blk1) resp. [b0, b1)); inputs are taken to be at level max_level (the cache holds max_level moduli) */
int sfg_matmul_resident_range_rc_dev(sfg_ctx *ctx, const double *cache_dev, int s, int max_level, const sfg_geno *g, unsigned flags,
                                     int blk0, int blk1, uint64_t *out_dev);
int sfg_matmul_accumulate_rc_dev(sfg_ctx *ctx, const double *cache_dev, int s, int max_level, const sfg_geno *g, unsigned flags,
                                 int b0, int b1, int j0, int j1, int accumulate, uint64_t *acc_dev);
/* after an integer all-reduce(sum) of partial outputs across ranks: canonical reduction mod q_l of [rows][L][N] */
int sfg_reduce_rows_dev(sfg_ctx *ctx, uint64_t *rows_dev, size_t nrows_of_L, int L);

/* ---- one party's products on the G GPUs of a node (mgpu.hip) ----
 * The reference runs one OS process per party (run_example.sh:1-12) and calls MatMult4StreamCompute twice per power iteration (gwas/pca.go:344,352) and
 * MatMult4Stream once per SNP batch (gwas/assoc.go:360-408).  sfg_mgpu_create gives such a process all of a node's GPUs: one context per device, one host thread per
 * device inside every call, RCCL (resolved with dlopen at the first use) for the one exchange step of Q' * X^T.  Launchers that start one process per GPU
 * (bench.py under torch.distributed.run) join the same engine with sfg_mgpu_create_rank and a 128-byte id made by sfg_mgpu_unique_id on rank 0 and carried to
 * the other ranks by the caller's own channel (the Go network layer, a TCP store).
 * Partitioning: X (n_ind x m_snp) by blocks of 8192 SNP columns, rank r owns blocks [nblk r / world, nblk (r + 1) / world) (sfg_mgpu_shard).
 *   Q * X     every rank multiplies its own output block columns; no data-path collective.
 *   Q' * X^T  contraction over the rank's blocks; per output block column the canonical uint64 accumulators are REDUCE-SCATTERED over the giant-step axis
 *             (padded to world * ceil(91 / world) slots) on a second queue while the next column is multiplied; every rank reduces mod q and aligns its own giant
 *             steps (key switching is not bit-linear: partial sums must be combined BEFORE the rotations of matmult.go:1474-1494), the aligned partial
 *             outputs are ALL-REDUCED and reduced mod q.  Identical words for every world size (tests/test_gpu_mgpu.py, bench.py's digests).
 * SFG_MGPU_TRANSPORT=direct (single process only; forced when `devices` repeats a device, which RCCL refuses): a rank sums its slice straight from its peers'
 * buffers with a kernel (peer access); SFG_MGPU_FORCE_COLLECTIVES=1 runs the exchange even at world size 1; SFG_MGPU_CACHE_GB (72) bounds a rank's own
 * rotation cache for the pipelined form.  A failing rank fails the call (sfg_mgpu_last_error names it). */
typedef struct sfg_mgpu sfg_mgpu;
typedef struct sfg_mgeno sfg_mgeno;
#define SFG_MGPU_ID_BYTES 128
int sfg_mgpu_unique_id(uint8_t *id128);
/* context arguments as sfg_ctx_create; devices[n]: HIP device indices, world size = n, local rank i = rank i */
int sfg_mgpu_create(sfg_mgpu **out, const int *devices, int n, int logN, int nq, int np, const uint64_t *moduli, const uint64_t *psi, double scale);
int sfg_mgpu_create_rank(sfg_mgpu **out, int device, int rank, int world, const uint8_t *id128, int logN, int nq, int np, const uint64_t *moduli,
                         const uint64_t *psi, double scale);
/* the same with a configuration (sfg_config above; NULL = defaults): every rank's context takes it, the engine takes mgpu_transport / mgpu_cache_bytes / rccl_lib */
int sfg_mgpu_create_ex(sfg_mgpu **out, const int *devices, int n, int logN, int nq, int np, const uint64_t *moduli, const uint64_t *psi, double scale,
                       const sfg_config *config);
int sfg_mgpu_create_rank_ex(sfg_mgpu **out, int device, int rank, int world, const uint8_t *id128, int logN, int nq, int np, const uint64_t *moduli,
                            const uint64_t *psi, double scale, const sfg_config *config);
void sfg_mgpu_destroy(sfg_mgpu *mg);
const char *sfg_mgpu_last_error(const sfg_mgpu *mg);      /* mg may be NULL: error of a failed create */
int sfg_mgpu_world(const sfg_mgpu *mg);
int sfg_mgpu_nlocal(const sfg_mgpu *mg);                  /* ranks driven by this process (n, or 1) */
int sfg_mgpu_rank(const sfg_mgpu *mg, int local);
sfg_ctx *sfg_mgpu_ctx(sfg_mgpu *mg, int local);           /* the context of a local rank: device buffers (sfg_malloc), evaluator ops, phase timers */
const char *sfg_mgpu_transport(const sfg_mgpu *mg);       /* "none" (world 1), "rccl", "direct" */
int sfg_mgpu_synchronize(sfg_mgpu *mg);
/* What the RCCL communicator of local rank `local` itself reports (ncclCommCount / ncclCommUserRank); 0 / 0 when the engine holds none (world 1, direct transport).
 * A record of a multi-GPU run can state "RCCL saw N ranks" from this instead of trusting the launcher's environment. */
int sfg_mgpu_comm_info(sfg_mgpu *mg, int local, int *nranks, int *rank);
/* Pre-flight of the exchange paths, for the first contact with a node (the exchanges stand behind gwas/pca.go:344,352): a reduce-scatter and an all-reduce of
 * a known uint64 pattern (count_per_rank words per rank slice) through the very functions the products use, on the collectives' queue of every rank, checked on the
 * host.  Every exchanging call - this one, sfg_mgpu_matmul* with SFG_TRANSPOSE - has an AGREEMENT POINT after its allocations and before its first collective: a rank
 * that failed so far fails the call on every rank instead of leaving the others waiting in a collective; a rank that fails after it aborts its communicator
 * (ncclCommAbort), which releases the peers, and the engine then refuses further exchanges. */
int sfg_mgpu_preflight(sfg_mgpu *mg, size_t count_per_rank);
/* key material to every local device: cryptoParams.RotKs / Rlk as sfg_ctx_load_rotkey / _relinkey */
int sfg_mgpu_load_rotkey(sfg_mgpu *mg, uint64_t galois_el, const uint64_t *key_host, int montgomery_form);
int sfg_mgpu_load_relinkey(sfg_mgpu *mg, const uint64_t *key_host, int montgomery_form);
int sfg_mgpu_fill_rotkeys_synthetic(sfg_mgpu *mg, const int *rot_left, int nrot, uint64_t seed);
/* SNP-block shard of `rank`: block columns [*blk0, *blk1), columns [*col0, *col1) (any pointer may be NULL) */
int sfg_mgpu_shard(int world, size_t ncol, int rank, size_t *blk0, size_t *blk1, size_t *col0, size_t *col1);
/* MatMult4StreamPreprocess on G GPUs (matmult.go:914-1041): the party's whole row-major int8 matrix (row stride ld); every local rank keeps its column window
 * resident.  _adopt: per-rank windows the caller made on the ranks' contexts (sfg_geno_from_bed / _from_pgen / _from_device; NULL for an empty window), ownership
 * passes.  _synthetic: the window of ONE global synthetic matrix (sfg_fill_geno_window_dev), optionally 2-bit packed - bench.py and the tests. */
int sfg_mgpu_geno_upload(sfg_mgpu *mg, const int8_t *geno_host, size_t nrow, size_t ncol, size_t ld, sfg_mgeno **out);
int sfg_mgpu_geno_adopt(sfg_mgpu *mg, size_t nrow, size_t ncol, sfg_geno *const *shards, sfg_mgeno **out);
int sfg_mgpu_geno_synthetic(sfg_mgpu *mg, size_t nrow, size_t ncol, uint64_t seed, int packed, sfg_mgeno **out);
void sfg_mgpu_geno_free(sfg_mgpu *mg, sfg_mgeno *g);
const sfg_geno *sfg_mgpu_geno_shard(const sfg_mgeno *g, int local);
int sfg_mgpu_geno_dims(const sfg_mgeno *g, size_t *nrow, size_t *ncol);
int sfg_mgpu_geno_blocks(const sfg_mgeno *g, int local, size_t *blk0, size_t *blk1);
int sfg_mgpu_geno_set_plaintext_cache(sfg_mgpu *mg, const sfg_mgeno *g, size_t max_bytes_per_rank);
/* sfg_geno_qc_scan on the sharded matrix (gwas/qualcontrol.go:36-81, 339-378, 416-463): filters and outputs span the WHOLE matrix; every local rank scans its
 * column window, column counts land at the window's columns, the row counts of the local ranks are summed on the host.  No collective: in a one-process-per-GPU
 * world the column counts outside this process's windows are zero and the row counts are the PARTIAL sums of this process's ranks - the caller adds them across
 * processes.  (The sharded counterpart of sfg_geno_filter is sfg_mgpu_geno_filter below: it re-shards, because a rank's filtered window is no longer a whole
 * number of 8192-column blocks, which is what sfg_mgeno windows are.  It exists inside one process only; in a one-process-per-GPU world filter before sharding.) */
int sfg_mgpu_geno_qc_scan(sfg_mgpu *mg, const sfg_mgeno *g, const uint8_t *row_filter, const uint8_t *col_filter, const uint8_t *row_ctrl,
                          uint32_t *col_counts_host, uint32_t *row_miss_host, uint32_t *row_het_host);
/* sfg_geno_filter on the sharded matrix, re-sharding (reshard.hip): what lies between quality control and the PCA in the reference - GeneratePCAInput
 * (gwas/gwas.go:545) reads through the row and column filters, FilterMatrixFile (gwas/utilities.go:154) materialises the filtered matrix.  The filters span the
 * WHOLE matrix (one byte per row, one per global column; zero drops, NULL keeps all; kept rows and columns stay in order).  *out is a new owned sfg_mgeno of
 * kept_rows x kept_cols whose windows are those of sfg_mgpu_shard(world, kept_cols, rank): every rank gathers its new window straight out of the old windows of
 * the ranks that hold its columns (plain loads between ranks that share a device, peer access between devices - enabled here on first use; devices that cannot
 * reach each other fail the call before anything is allocated and are named).  int8 in -> int8 out, with the row stride of a shard rounded up to a multiple of
 * 16 bytes and zero padding bytes (sfg_geno_layout tells; every product and scan takes a row stride); packed in -> packed out, codes re-packed across dropped
 * columns and old rank boundaries, padding codes 0, no int8 intermediate.  Temporaries are the index tables, O(kept_rows + window columns) per rank ("qc."
 * scratch).  The source is not changed and no collective is used; the call returns after every rank's queue has drained, so the source may be freed at once.  The
 * result has no plaintext cache.  Both filters NULL: a copy with the same windows.  Filters that keep nothing, a NULL g or out, a dimension of 2^32 or more: an
 * error that allocates and launches nothing.  If a rank fails, every new buffer is freed, *out is NULL and sfg_mgpu_last_error names the rank.  In a world of one
 * rank per process a peer's memory is not addressable: the call is refused, and the matrix is filtered before it is sharded (sfg_geno_filter, or the filters of
 * sfg_geno_from_bed / _from_pgen on each rank's window). */
int sfg_mgpu_geno_filter(sfg_mgpu *mg, const sfg_mgeno *g, const uint8_t *row_filter, const uint8_t *col_filter, sfg_mgeno **out);
/* sfg_sketch (gwas/pca.go:152-162) on the sharded matrix (SURVEY 8e "SNP-sharded, independent"): every local rank sketches its own window with the same per-row
 * bucket_host / sgn_host; sketch_host [kp][ncol] and xsum_host / x2sum_host [ncol] are in the GLOBAL column layout, any of them may be NULL.  No collective: in a
 * one-process-per-GPU world the entries outside this process's windows are zero.  A packed matrix is refused as by sfg_sketch, before anything is launched. */
int sfg_mgpu_sketch(sfg_mgpu *mg, const sfg_mgeno *g, const int32_t *bucket_host, const int8_t *sgn_host, int kp,
                    double *sketch_host, uint64_t *xsum_host, uint64_t *x2sum_host);
/* sfg_geno_colsums (gwas/matmult.go:1292-1300) on the sharded matrix: sum_host / sqsum_host [ncol] in the global column layout, either may be NULL; entries
 * outside this process's windows are zero. */
int sfg_mgpu_geno_colsums(sfg_mgpu *mg, const sfg_mgeno *g, double *sum_host, double *sqsum_host);
/* The row-streamed forms of sfg_geno_create / _write_rows / _compare_rows on the sharded matrix (MatMult4StreamPreprocess, gwas/matmult.go:914-1041, reads one row
 * at a time: gwas/filestream.go:414-426): a chunk of whole-matrix rows is scattered to the ranks' column windows; a chunk of the rows of the TRANSPOSE is compared by
 * the ranks whose windows hold those columns.  *ndiff accumulates over the local ranks. */
int sfg_mgpu_geno_create(sfg_mgpu *mg, size_t nrow, size_t ncol, sfg_mgeno **out);
int sfg_mgpu_geno_write_rows(sfg_mgpu *mg, sfg_mgeno *g, size_t row0, size_t nrows, const int8_t *rows_host, size_t ld);
int sfg_mgpu_geno_compare_rows(sfg_mgpu *mg, const sfg_mgeno *g, unsigned flags, size_t row0, size_t nrows, const int8_t *rows_host, size_t ld, uint64_t *ndiff);
/* MatMult4StreamCompute (matmult.go:1043-1236) on the sharded matrix.  Device-pointer form, A_dev[i] / out_dev[i] on local rank i's device:
 *   flags = 0 or SFG_SQUARE  (Q * X):    A_dev[i] = the whole input grid [s][ceil(nrow / 8192)] (replicated);  out_dev[i] = [s][blk1 - blk0], the rank's block columns
 *   | SFG_TRANSPOSE          (Q' * X^T): A_dev[i] = [s][blk1 - blk0], the inputs of the rank's SNP blocks;    out_dev[i] = the whole [s][ceil(nrow / 8192)], on every rank
 * ciphertext layouts as sfg_matmul_resident_dev; stream-ordered on each rank's queue (sfg_mgpu_synchronize waits).
 * Host-pointer form (the Go shim's): Q * X takes A_host [s][nbr] and fills out_host [s][m_ct] (in a multi-process world: the block columns of this process's
 * ranks only); Q' * X^T takes A_host [s][m_ct] (all SNP blocks, each rank uploads its own) and fills out_host [s][nbr] completely in every process. */
int sfg_mgpu_matmul_dev(sfg_mgpu *mg, const uint64_t *const *A_dev, int s, int in_level, int max_level, const sfg_mgeno *g, unsigned flags,
                        uint64_t *const *out_dev);
int sfg_mgpu_matmul(sfg_mgpu *mg, const uint64_t *A_host, int s, int in_level, int max_level, const sfg_mgeno *g, unsigned flags, uint64_t *out_host);
/* test hook: local rank `local` fails ONCE in the next exchanging Q' * X^T call (phase 0: the host form's I/O pass, 1: before the agreement point); refused unless SFG_ENABLE_TEST_HOOKS=1 was set before sfg_mgpu_create */
int sfg_mgpu_inject_failure_for_test(sfg_mgpu *mg, int local, int phase);
/* GenoBlockMult's batch loop (gwas/assoc.go:340-420) on G GPUs: the reference hands the SNP batches of a chromosome file to assoc_num_blocks_parallel workers
 * (:360-408); here batch k goes to rank k % world.  Every rank streams its batches from the file (sfg_assoc_stream_bed / _pgen: reader thread, pinned slots, decode on
 * the device), multiplies them against its own call-wide rotation cache of `mat` and its output ciphertexts land at their positions of
 * out_host [s][out_ct_capacity][2][max_level][N] (a multi-process world: the positions of this process's ranks only).  A_host: mat, [s][ceil(kept samples / 8192)]
 * ciphertexts at in_level.  sum_host / sqsum_host, flags, *out_ct as in the single-GPU calls.  No collective. */
int sfg_mgpu_assoc_stream_bed(sfg_mgpu *mg, const char *bed_path, size_t num_sample, size_t num_snp, const uint8_t *row_filter, const uint8_t *col_filter,
                              size_t batch_snps, const uint64_t *A_host, int s, int in_level, int max_level, unsigned flags,
                              uint64_t *out_host, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host);
int sfg_mgpu_assoc_stream_pgen(sfg_mgpu *mg, const char *pgen_path, const uint8_t *row_filter, const uint8_t *col_filter, size_t kept_samples,
                               size_t batch_snps, const uint64_t *A_host, int s, int in_level, int max_level, unsigned flags,
                               uint64_t *out_host, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host);

/* ---- f-1: collective bootstrap, LOCAL work (mpc/mhe.go:222-348: CollectiveBootstrap / CollectiveBootstrapMat) ----
 * Per ciphertext the reference calls lattigo's dckks.RefreshProtocol: GenShares (mhe.go:251,315), aggregates the shares over the network
 * (AggregateRefreshShare*, stays in Go), then Decrypt / Recode / Recrypt (mhe.go:256-258,329-331).  PARITY UNPINNED: restated from the published
 * lattigo v2.1.0 dckks/refresh.go for ciphertext scale == target scale (the fork's target-scale argument is not in the reference tree).
 * Randomness stays with the caller: mask_dev [nct][N][mask_limbs] two's-complement 64-bit limbs (ring.RandInt(bound) recentred, one big
 * integer per coefficient), e0/e1 [nct][N] Gaussian error coefficients, crs [nct][nq][N] the common reference polynomials (NTT domain). */
/* cryptoParams.Sk.Value (crypto.go:44): secret-key shard, rows [nq][N] in the NTT domain; montgomery_form != 0 for lattigo's stored form */
int sfg_ctx_load_secret_key(sfg_ctx *ctx, const uint64_t *sk_host, int montgomery_form);
/* RefreshProtocol.GenShares on nct ciphertexts [nct][2][level+1][N]:
 *   h0 [nct][level+1][N] = NTT(mask + e0) + sk (.) c1        (refSharesDecrypt)
 *   h1 [nct][nq][N]      = -(NTT(mask + e1) + sk (.) crs)     (refSharesRecrypt, at MaxLevel) */
int sfg_refresh_gen_shares_dev(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, const uint64_t *crs_dev, const uint64_t *mask_dev, int mask_limbs,
                               const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
/* RefreshProtocol.Decrypt + Recode + Recrypt with the AGGREGATED shares: out [nct][2][nq][N] at MaxLevel = nq-1:
 *   c0' = NTT( centred( CRT( INTT(c0 + h0agg) ) ) mod every q_j ) + h1agg,   c1' = crs */
int sfg_refresh_finish_dev(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, const uint64_t *h0agg_dev, const uint64_t *h1agg_dev,
                           const uint64_t *crs_dev, uint64_t *out_dev);

/* The target-scale form, which is what the reference calls: mhe.go:251,315 GenShares(sk, levelStart, nParties, ct, parameters.Scale(), crp, ...) and
 * mhe.go:257,330 Recode(ct, parameters.Scale()), on products whose scale is A.scale * Params.Scale() (matmult.go:44,92 -> :1045).  PARITY UNPINNED:
 * restated from the published lattigo v2.2.0 dckks/refresh.go (the nearest upstream with the targetScale argument):
 *   GenShares: recrypt share from Quo(mask * Int(target_scale), Int(ct_scale)) (big.Int.Quo, truncated towards zero); decrypt share from the mask itself
 *   Recode:    x <- Quo(x * Int(target_scale), Int(ct_scale)) on the centred big integer, before the re-reduction into all nq moduli
 * The caller sets the refreshed ciphertext's scale to target_scale.  mask_limbs <= 8 here. */
int sfg_refresh_gen_shares_scaled_dev(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, double ct_scale, double target_scale, const uint64_t *crs_dev,
                                      const uint64_t *mask_dev, int mask_limbs, const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
int sfg_refresh_finish_scaled_dev(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, double ct_scale, double target_scale, const uint64_t *h0agg_dev,
                                  const uint64_t *h1agg_dev, const uint64_t *crs_dev, uint64_t *out_dev);

/* f-4: ring work of MPC.CMatToSS (mpc/ss.go:146-281): the masked decryption share of each ciphertext and NTT(mask), which sfg_ckks_to_ss_finish_dev
 * (below) turns into the additive share after the aggregation (ss.go:239-279).
 *   h0 [nct][level+1][N] = NTT(mask) + sk (.) c1 + NTT(e0)   (ss.go:222-236)      mask_ntt [nct][level+1][N] = NTT(mask)   (ctMask, ss.go:226) */
int sfg_ckks_to_ss_share_dev(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, const uint64_t *mask_dev, int mask_limbs, const int32_t *e0_dev,
                             uint64_t *h0_dev, uint64_t *mask_ntt_dev);

/* f-4: the share algebra of MPC.SSToCMat (mpc/ss.go:84-110; EncodeRVecNew, :125, is sfg_rvec_encode_dev below, the encryption sfg_encrypt_explicit_dev).
 * Field elements as in the Beaver products.  rand_dev: the ring.RandInt(bound) draws of the caller (< bound), bound_host = Modulus / (4 (nParty - 1)):
 *   mask = rand >= bound / 2 ? rand - bound : rand  (mod p, :90-99);   rm_masked = rm - mask (:101-102, what RevealSymMat then opens)
 * and, on the hub party after the reveal, share = revealed + mask (:104-106). */
int sfg_ss_mask_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *bound_host, const uint64_t *rm_dev, const uint64_t *rand_dev,
                    uint64_t *rm_masked_dev, uint64_t *mask_dev, size_t n);
int sfg_ss_hub_share_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *revealed_dev, const uint64_t *mask_dev, uint64_t *share_dev, size_t n);

/* ---- f-4: secret shares to CKKS plaintexts and back on the device (rvec.hip) ----
 * PARITY UNPINNED against the lattigo fork's encoder.EncodeRVecNew / DecodeRVec, whose source is not published: what they compute is fixed by their call sites and
 * by linearity, stated here exactly and pinned against that statement (tests/rvec_ref.py, tests/test_gpu_rvec.py; derivations: DESIGN.md section 12).
 * N = 2^14, n = N/2 slots, zeta = exp(2 pi i / 2N), slot order and the 5^t rotation group of sfg_encode_vectors_dev / sfg_decode_vectors.  A field element is
 * `limbs` (2 or 4) little-endian 64-bit words holding a canonical residue in [0, p) of the odd modulus p = modulus_host, plain (not Montgomery), as sfg_ss_mask_dev
 * takes and returns it; centre(x) = x for x <= (p - 1)/2, else x - p.  scale: a finite double >= 1 taken as the exact rational it is; 0 <= frac_bits = f <= 62;
 * round() is to nearest.
 *   encode:  s_t = centre(x_t) for t < n_elem, 0 beyond;  w_c = (1/n) sum_t s_t zeta^(-5^t c);  p_c = round(scale 2^-f Re w_c),  p_{c+n} = round(scale 2^-f Im w_c);
 *            pt = the NTT-domain rows [level+1][N] of p mod q_0..q_level, canonical words (what sfg_encrypt_explicit_dev takes as pt_dev)
 *   decode:  p_c = the centred CRT integer of the INTT of the rows (lattigo's Cmp(QHalf) rule, as sfg_decode_vectors);  v_t = sum_c (p_c + i p_{c+n}) zeta^(5^t c);
 *            r_t = round(2^f / scale Re v_t) mod p in [0, p), t < n_elem
 * Accuracy contract, both directions: the transform is W-word fixed point (no floating point between the input words and the output words); before the final
 * rounding the device value is within 2^-32 of the exact real value, in units of the output.  Every output is therefore the exact nearest integer, except where
 * the exact value lies within 2^-32 of a rounding tie: there either neighbour may come out (exact ties round away from zero).
 * Refused, with an error string and nothing launched: limbs not 2 or 4, an even modulus, n_elem outside 1..8192, a bad level, a scale that is not finite or below 1,
 * frac_bits outside 0..62, a (scale, frac_bits) pair that needs more than 8 words of precision, and for the encoder a level too small for the field:
 *   bitlen(p) - 1 - f + ceil(log2 scale) + 1 < bitlen(Q_level) - 1   must hold   (PN14QP438, f = 30, scale 2^34: limbs 2 from level 3, limbs 4 from level 7).
 * Stream-ordered, not synchronising.  Scratch from the context's pool, per ciphertext of a chunk of at most 64: 2 W 65,536 bytes + (level + 1) 131,072 bytes, W <= 8
 * the word count of the call (sfgwas_amd/csrc/rvec_host.hpp: 3 / 5 for the encoder at limbs 2 / 4, 2..7 for the decoder at levels 0..9, with f = 30, scale 2^34). */
/* encoder.EncodeRVecNew (mpc/ss.go:125): share_dev [nct][n_elem][limbs] -> pt_dev [nct][level+1][N] */
int sfg_rvec_encode_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *share_dev, int n_elem, int nct, int level, double scale, int frac_bits,
                        uint64_t *pt_dev);
/* encoder.DecodeRVec (mpc/ss.go:260,264): plaintext rows pt_stride words apart (>= (level+1) * N: polynomial 0 of a resident ciphertext can be read in place)
 * -> out_dev [nct][n_elem][limbs] */
int sfg_rvec_decode_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale, int frac_bits,
                        int n_elem, uint64_t *out_dev);
/* mpc/ss.go:239-279 in one call, after the aggregation of the sfg_ckks_to_ss_share_dev shares: on the hub (is_hub != 0; ct_dev [nct][2][level+1][N], h0agg_dev
 * [nct][level+1][N]) out = decode(c0 + h0agg) - decode(mask_ntt) mod p, on every other party out = -decode(mask_ntt) mod p (ct_dev and h0agg_dev not read).
 * Every output word equals sfg_pcks_finish_dev, two sfg_rvec_decode_dev calls and the field subtraction.  out_dev [nct][n_elem][limbs]; additionally 2 * nct *
 * n_elem * limbs * 8 bytes of scratch. */
int sfg_ckks_to_ss_finish_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *ct_dev, int nct, int level, double scale, int frac_bits,
                              const uint64_t *h0agg_dev, const uint64_t *mask_ntt_dev, int is_hub, int n_elem, uint64_t *out_dev);

/* ---- C6 on the device: public-key encryption (crypto.CZeros / CZeroMat, basics.go:367-384; EncryptFloatVector / EncryptFloatMatrixRow, crypto.go:340-388;
 * both end in lattigo's pkEncryptor.EncryptNew) ----
 * PARITY UNPINNED: restated from the published lattigo v2.1 ckks/encryptor.go (the form that samples in R_QP and divides by P); with fresh randomness bit parity
 * with the Go binary cannot exist.  What IS pinned (tests/test_gpu_encrypt.py): every word against a big-integer statement of the arithmetic below, the sampler
 * against an independent Python ChaCha20 + table inversion, and decryption within the derived worst-case noise bound. */
/* cryptoParams.Pk.Value (crypto.go:45, what crypto.go:355 NewEncryptorFromPk takes): [2][nq+np][N] words in the NTT domain; montgomery_form != 0 for lattigo's
 * stored form.  Kept with the rotation keys: every fork sees it, it is freed with the root.  Every encrypting call without it fails and launches nothing. */
int sfg_ctx_load_public_key(sfg_ctx *ctx, const uint64_t *pk_host, int montgomery_form);
int sfg_ctx_has_public_key(const sfg_ctx *ctx);
/* The deterministic core of EncryptNew (lattigo ckks/encryptor.go encrypt(), the ModDown branch); randomness stays with the caller: u int8 [nct][N] in {-1, 0, 1},
 * e0, e1 int32 [nct][N], pt_dev NULL (zero) or [nct][level+1][N] NTT-domain plaintext rows, out_dev [nct][2][level+1][N] canonical words.
 * For every modulus m of Q_0..Q_level and of P:  t_i = pk_i (.) NTT(u) + NTT(e_i);  c_i = ModDown_P(t_i), the key switch's (float-corrected basis extension);
 * c_0 += pt.  Row j of the result depends on modulus j and the P rows only: level l gives rows 0..l of the MaxLevel encryption of the same u, e0, e1. */
int sfg_encrypt_explicit_dev(sfg_ctx *ctx, const uint64_t *pt_dev, int nct, int level, const int8_t *u_dev, const int32_t *e0_dev, const int32_t *e1_dev,
                             uint64_t *out_dev);
/* The sampler's key (replaces the PRNG lattigo's NewEncryptorFromPk draws from crypto/rand, crypto.go:355): 32 bytes from the caller's CSPRNG.  There is no default and
 * nothing is derived from time or addresses: unseeded, the sampling calls fail.  ChaCha20 (RFC 8439) with nonce = (64-bit encryption index, 32-bit polynomial id);
 * the index is ONE atomic counter shared by the root and its forks, a call takes nct consecutive indices, seeding resets it to 0.  A key must never be seeded twice
 * (after a restart: a fresh key).  Wiped from host and device memory with the root context; never part of an error string.  Setup-time call: not concurrent with
 * encrypting calls of other forks. */
int sfg_ctx_seed_encryptor(sfg_ctx *ctx, const uint8_t *key32);
int sfg_ctx_encryptor_next_index(const sfg_ctx *ctx, uint64_t *next_index);
/* crypto.CZeroMat + eval.Add (matmult.go:1174,1225,1443,1494; integration/go/gwas/matmult_hip.go finish()): ct += Enc(0) in place on [nct][2][level+1][N], each
 * with fresh samples (nct indices).  Bit-identical to sfg_encrypt_explicit_dev on those samples, added. */
int sfg_ct_add_fresh_zero_dev(sfg_ctx *ctx, uint64_t *ct_dev, int nct, int level);
/* crypto.EncryptFloatVector (crypto.go:340-362) / one row of EncryptFloatMatrixRow (crypto.go:364-388): sfg_encode_vectors_dev's plaintext rows (same argument
 * conventions, same bits), encrypted: values_host [nct][slots] -> out_dev [nct][2][level+1][N]. */
int sfg_encrypt_vectors_dev(sfg_ctx *ctx, const double *values_host, int nct, int level, uint64_t *out_dev);
/* test hook (replaces nothing in the reference): the samples u, e0, e1 ([nct][N] int8 / int32 / int32) of encryption indices first_index .. first_index + nct - 1
 * under the seeded key, without advancing the counter.  Refused unless the process set SFG_ENABLE_TEST_HOOKS=1 before sfg_ctx_create. */
int sfg_encrypt_transcript_for_test(sfg_ctx *ctx, uint64_t first_index, int nct, int8_t *u_dev, int32_t *e0_dev, int32_t *e1_dev);

/* ---- the way back out: collective decryption and decoding on the device (decrypt.hip) ----
 * PARITY UNPINNED: the collective key switch is restated from the published lattigo v2.1 dckks/public_keyswitch.go (PCKSProtocol.GenShare / KeySwitch), the branch
 * that samples in R_QP and divides by P; with the reference's all-zero public key (mpc/mhe.go:107-220) the ternary sample multiplies zero and drops out.  Neither bit
 * parity with the Go binary nor the CPU cost these calls replace (lattigo's decoder) can be established without a Go toolchain.  What IS pinned
 * (tests/test_gpu_decrypt.py): every share word against the big-integer statement, every decoded coefficient bit for bit, every slot against an exact decoder. */
/* mpc/mhe.go:107-220 CollectiveDecrypt / CollectiveDecryptVec / CollectiveDecryptMat, the local half before the aggregation: PCKSProtocol.GenShare(skShard, zeroPk,
 * ct, share) on nct ciphertexts [nct][2][level+1][N]:
 *   h0 [nct][level+1][N] = ModDown_P(NTT_QP(e0)) + sk (.) c1,     h1 [nct][level+1][N] = ModDown_P(NTT_QP(e1))
 * ModDown_P(NTT_QP(e)) is sfg_encrypt_explicit_dev's for u = 0 and no plaintext (the same code path).  Randomness stays with the caller: e0, e1 int32 [nct][N]
 * (the reference draws them with sigma 6.36, bound 38: NewPCKSProtocol(parameters, 6.36)).  h1_dev may be NULL (then e1_dev is not read): the reference discards
 * polynomial 1 after KeySwitch.  Fails without a loaded secret-key shard.  The aggregation over the network stays in Go (mpc/aggregate.go). */
int sfg_pcks_gen_share_dev(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
/* the local half after the aggregation: PCKSProtocol.KeySwitch followed by .Plaintext(): pt [nct][level+1][N] = c0 + h0agg, NTT domain.  The scale is the
 * ciphertext's; the caller carries it. */
int sfg_pcks_finish_dev(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, const uint64_t *h0agg_dev, uint64_t *pt_dev);
/* crypto.DecodeFloatVector (crypto/crypto.go:525-536 -> encoder.Decode; gwas/assoc.go:491,496,587, gwas/utilities.go:385-389): the inverse of sfg_encode_vectors_dev.
 * pt_dev: NTT-domain plaintext rows [level+1][N] per plaintext, pt_stride words apart (>= (level+1) * N: polynomial 0 of resident ciphertexts can be read in place);
 * scale: any finite double >= 1 (not a power of two after a rescale).  re_host [nct][slots]: the real parts in lattigo's slot order; im_host NULL (the common case,
 * ConvertVectorComplexToFloat64 keeps the real parts only: one transform) or [nct][slots] (a second transform).  The real parts are the same bits either way.
 * All on the device: INTT, CRT to the centred integer p_c in (-Q/2, Q/2] with lattigo's Cmp(QHalf) rule, p_c / scale in double-double, the forward embedding
 * v_t = sum_c (p_c + i p_{c+n}) / scale * zeta^(5^t c) in double-double, rounded to double once.  Accuracy contract: every returned double d_t satisfies
 *   |d_t - v_t| <= B max_t |v_t|,   B = 2^-53 + 2^-82    (derivation: decrypt.hip)
 * for levels 0..11 (level + 1 <= 12 moduli).  Synchronising; like sfg_memcpy_d2h it fails - before anything is launched - while an encoder coefficient within
 * 2^-50 of a rounding tie is outstanding.  nct == 0 returns 0; a bad level, scale or count is an error that launches nothing. */
int sfg_decode_vectors(sfg_ctx *ctx, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale, double *re_host, double *im_host);
/* the same with the doubles left in HBM (re_dev [nct][slots], im_dev NULL or [nct][slots]): stream-ordered, not synchronising */
int sfg_decode_vectors_dev(sfg_ctx *ctx, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale, double *re_dev, double *im_dev);
/* the counterpart of sfg_encode_coeffs_host: INTT, CRT and the division only; coeffs_host [nct][N] doubles, each p_c / scale rounded to nearest (half to even) from a
 * double-double value that is exact for |p_c| < 2^106 and otherwise within 2^-100 relative (correctly rounded unless the quotient lies that close to a rounding boundary). */
int sfg_decode_coeffs(sfg_ctx *ctx, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale, double *coeffs_host);
/* gwas/gwas.go:385-386 (CollectiveDecryptVec, then DecodeFloatVector) after the aggregation, in one call: sfg_pcks_finish_dev + sfg_decode_vectors, same doubles,
 * no plaintext rows returned to the caller */
int sfg_pcks_finish_decode(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, double scale, const uint64_t *h0agg_dev, double *re_host, double *im_host);
/* crypto.DecryptFloatVector (crypto/crypto.go:489-510; DecryptFloat / DecryptMultipleFloat / DecryptFloatMatrix, :446-523) with the loaded key as the WHOLE secret
 * key: c0 + sk (.) c1, then sfg_decode_vectors.  Fails without a loaded secret key. */
int sfg_decrypt_vectors(sfg_ctx *ctx, const uint64_t *ct_dev, int nct, int level, double scale, double *re_host, double *im_host);

/* ---- collective key generation on the device: the local halves of mpc.CollectiveInit (mpc/mhe.go:24-81; keygen.hip) ----
 * PARITY UNPINNED: restated from the published lattigo v2.1 dckks / drlwe (CKGProtocol.GenShare, RTGProtocol.GenShare, RKGProtocol.GenShareRoundOne / RoundTwo);
 * with fresh randomness bit parity with the Go binary cannot exist.  What IS pinned (tests/test_gpu_keygen.py): every share word against the Python-integer statement
 * tests/keygen_ref.py, the sampled forms against the explicit cores, and keys made here carrying a ciphertext through a rotation and a relinearisation within the
 * noise bound DESIGN.md derives.  The aggregation over the network stays in Go (mpc/aggregate.go:121-240); drawing the secret key stays with the caller.
 * All polynomials are rows [nmod = nq + np][N], NTT domain, canonical words, in device memory.  beta = ceil(nq / np) digits; g_i at modulus m is P mod q_m when
 * m < nq && m / np == i, else 0 (the convention the library's key switch consumes); a rotation key for Galois element g switches from phi_{g^-1}(s). */
/* cryptoParams.Sk.Value over Q and P: sk_host [nq+np][N], NTT domain; montgomery_form != 0 for lattigo's stored form.  Also provides the Q rows that
 * sfg_ctx_load_secret_key provides, stored identically.  Wiped from device memory with the root context.  Every key-generation call below fails, launching
 * nothing, without it. */
int sfg_ctx_load_secret_key_qp(sfg_ctx *ctx, const uint64_t *sk_host, int montgomery_form);
/* CKGProtocol.GenShare (CollectivePubKeyGen, mhe.go:83-105): share [nmod][N] = -crp (.) sk + NTT(e); crp [nmod][N], e int32 [N] */
int sfg_ckg_gen_share_dev(sfg_ctx *ctx, const uint64_t *crp_dev, const int32_t *e_dev, uint64_t *share_dev);
/* RTGProtocol.GenShare for nkeys Galois elements at once (CollectiveRotKeyGen, mhe.go:381-476): shares [nkeys][beta][nmod][N],
 *   h_{k,i} = -crp_{k,i} (.) phi_{g_k^-1}(sk) + NTT(e_{k,i}) + g_i sk;   crp [nkeys][beta][nmod][N], e int32 [nkeys][beta][N].
 * nkeys is the caller's batching knob: the only scratch is 32 KiB of automorphism index per key.  An even Galois element or nkeys < 0 is an error that launches
 * nothing; nkeys == 0 returns 0. */
int sfg_rtg_gen_shares_dev(sfg_ctx *ctx, const uint64_t *galois_host, int nkeys, const uint64_t *crp_dev, const int32_t *e_dev, uint64_t *shares_dev);
/* RKGProtocol.GenShareRoundOne (CollectiveRelinKeyGen, mhe.go:478-502): u int8 [N] the party's ephemeral ternary secret, e0, e1 int32 [beta][N], crp, h0, h1 [beta][nmod][N]:
 *   h0_i = -NTT(u) (.) crp_i + g_i sk + NTT(e0_i),     h1_i = sk (.) crp_i + NTT(e1_i) */
int sfg_rkg_round1_dev(sfg_ctx *ctx, const uint64_t *crp_dev, const int8_t *u_dev, const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
/* RKGProtocol.GenShareRoundTwo on the aggregated round-one shares:  out_i = sk (.) H0agg_i + NTT(e2_i) + (NTT(u) - sk) (.) H1agg_i + NTT(e3_i) */
int sfg_rkg_round2_dev(sfg_ctx *ctx, const uint64_t *h0agg_dev, const uint64_t *h1agg_dev, const int8_t *u_dev, const int32_t *e2_dev, const int32_t *e3_dev, uint64_t *out_dev);
/* The sampled forms: the same shares with the errors (and the ephemeral u) drawn in the same kernel from the encryptor's keyed stream (sfg_ctx_seed_encryptor; the
 * byte-to-sample map of sfg_encrypt_* unchanged), no host randomness.  Each polynomial pair takes one encryption index from the counter the root and its forks share:
 *   public key share: 1 index, e = its polynomial id 1;   rotation shares: nkeys * beta indices, (k, i) takes first + k beta + i, e = id 1;
 *   round 1: beta + 1 indices, digit i takes first + i (e0, e1 = ids 1, 2), u = id 0 of index first + beta, returned in *u_index;
 *   round 2: beta indices, digit i takes first + i (e2, e3 = ids 1, 2); u is redrawn from u_index, never stored.
 * *first_index (may be NULL) states the first index taken: sfg_encrypt_transcript_for_test reproduces every sample from it.  Each call is bit-identical to its
 * explicit core on those samples.  Unseeded, they fail and launch nothing. */
int sfg_ckg_gen_share_sampled_dev(sfg_ctx *ctx, const uint64_t *crp_dev, uint64_t *share_dev, uint64_t *first_index);
int sfg_rtg_gen_shares_sampled_dev(sfg_ctx *ctx, const uint64_t *galois_host, int nkeys, const uint64_t *crp_dev, uint64_t *shares_dev, uint64_t *first_index);
int sfg_rkg_round1_sampled_dev(sfg_ctx *ctx, const uint64_t *crp_dev, uint64_t *h0_dev, uint64_t *h1_dev, uint64_t *first_index, uint64_t *u_index);
int sfg_rkg_round2_sampled_dev(sfg_ctx *ctx, const uint64_t *h0agg_dev, const uint64_t *h1agg_dev, uint64_t u_index, uint64_t *out_dev, uint64_t *first_index);
/* Installation of the aggregated keys straight from device memory (no host copy; the words are kept as sfg_ctx_load_* keeps non-Montgomery input):
 *   public key = (agg, crp);   rotation key k = (agg_{k,i}, crp_{k,i}) under galois_host[k];   relinearisation key = (round2agg_i, H1agg_i).
 * Setup-time calls like the loads; forks see the installed keys as they see loaded ones; sfg_ctx_export_rotkey returns exactly (agg, crp). */
int sfg_ctx_install_public_key_dev(sfg_ctx *ctx, const uint64_t *agg_dev, const uint64_t *crp_dev);
int sfg_ctx_install_rotkeys_dev(sfg_ctx *ctx, const uint64_t *galois_host, int nkeys, const uint64_t *agg_dev, const uint64_t *crp_dev);
int sfg_ctx_install_relinkey_dev(sfg_ctx *ctx, const uint64_t *round2agg_dev, const uint64_t *h1agg_dev);
/* The common reference polynomials from a 32-byte seed all parties share (replaces ring.UniformSampler over the fork's frand, mhe.go:49-59, whose bytes cannot be
 * reproduced here: a CPU-only party must implement this map).  Row r of the call is global row first_row + r at modulus mod_idx_host[r]; coefficient j comes from
 * the ChaCha20 block (RFC 8439) under key32 with block counter j and nonce (64-bit global row number, 32-bit try counter t = 0): its sixteen words form eight
 * 64-bit candidates (word 2k low, 2k + 1 high), each masked to bitlen(q) bits; the coefficient is the first candidate < q, and if none is, the same with t + 1.
 * out_dev [nrows][N].  The key is not retained by the context. */
int sfg_crp_fill_dev(sfg_ctx *ctx, const uint8_t *key32_host, uint64_t first_row, size_t nrows, const int *mod_idx_host, uint64_t *out_dev);

/* ---- B1-B3: Beaver local products (mpc/beavermult.go:94-147) over a prime field of `limbs` 64-bit LE limbs ---- */
int sfg_beaver_elem_dev(sfg_ctx *ctx, int pid, int limbs, const uint64_t *modulus_host,
                        const uint64_t *ar_dev, const uint64_t *am_dev, const uint64_t *br_dev, const uint64_t *bm_dev,
                        uint64_t *out_dev, size_t n);
int sfg_beaver_elem(sfg_ctx *ctx, int pid, int limbs, const uint64_t *modulus_host,
                    const uint64_t *ar_host, const uint64_t *am_host, const uint64_t *br_host, const uint64_t *bm_host,
                    uint64_t *out_host, size_t n);
int sfg_beaver_matmul(sfg_ctx *ctx, int pid, int limbs, const uint64_t *modulus_host,
                      const uint64_t *ar_host, const uint64_t *am_host, const uint64_t *br_host, const uint64_t *bm_host,
                      uint64_t *out_host, int m, int k, int n);

/* ---- P1: count-sketch + moments (gwas/pca.go:152-162) ----
 * sketch[kp][ncol] fp64 (exact integers), xsum/x2sum[ncol] uint64 */
int sfg_sketch(sfg_ctx *ctx, const sfg_geno *g, const int32_t *bucket_host, const int8_t *sgn_host, int kp,
               double *sketch_host, uint64_t *xsum_host, uint64_t *x2sum_host);

/* ---- synthetic data generators used by bench.py / tests (counter-mode splitmix64) ---- */
int sfg_fill_uniform_ct_dev(sfg_ctx *ctx, uint64_t *ct_dev, int nct, int level, uint64_t seed);
int sfg_fill_geno_dev(sfg_ctx *ctx, int8_t *geno_dev, size_t nrow, size_t ncol, uint64_t seed);
/* the column window [col0, col0+ncol) of the same global nrow x ncol_global matrix (row stride ld): SNP-sharded ranks hold
 * exactly the bytes the single-GPU run holds in that window, so outputs are comparable across world sizes */
int sfg_fill_geno_window_dev(sfg_ctx *ctx, int8_t *geno_dev, size_t nrow, size_t ncol, size_t ld, size_t col0, size_t ncol_global, uint64_t seed);
int sfg_fill_rotkeys_synthetic(sfg_ctx *ctx, const int *rot_left, int nrot, uint64_t seed);

/* last kernel timing hooks for bench.py: milliseconds spent (HIP events on the ctx stream) in the named phase
 * of the most recent matmul call: "encode" (diagonal FFT + plaintext NTT), "mac", "mac_small"/"mac_big" (the two k_mac instances), "rotate", "skew" ; returns <0 if unknown */
int sfg_ctx_clear_phases(sfg_ctx *ctx);
double sfg_last_phase_ms(const sfg_ctx *ctx, const char *phase);
int sfg_last_phase_launches(const sfg_ctx *ctx, const char *phase);
/* algorithmic bytes (operands read once + results written once, as laid out in HBM) credited to the phase's launches */
double sfg_last_phase_bytes(const sfg_ctx *ctx, const char *phase);

/* ---- the general ring: evaluator operations at the other CKKS presets (gwas/gwas.go:164-177: PN12QP109 .. PN16QP1761) ----
 * sfg_ctx is built for PN14QP438 alone (N = 16384, moduli below 2^47 held exactly in fp64).  sfg_ring serves 12 <= logN <= 16 and any prime modulus
 * q < 2^61 with q == 1 mod 2N (lattigo's own bound) in integer arithmetic; nq >= 1, np >= 1, nq + np <= 48.  It covers the ring arithmetic of
 * crypto/basics.go on device-resident ciphertexts - every word equal to lattigo's canonical residue - and, further down, public-key encryption and the collective decryption's
 * local halves, the encoder and the decoder, collective key generation, the collective bootstrap's local halves and, last in this header, the two matrix products.  Layouts are those of the sfg_ctx twin of each call: ciphertext [nct][2][level+1][N], key [beta][2][nq+np][N] in the NTT
 * domain with beta = ceil(nq/np), montgomery_form != 0 for lattigo's stored representation.  PN14QP438's own parameters are accepted as well.
 * Every call returns 0, or 1 with the cause in sfg_ring_last_error; all device work is ordered on the ring's own non-blocking stream.
 * psi NULL: derived as lattigo's ring.NewRing derives it; otherwise psi[m] must be a primitive 2N-th root of unity modulo moduli[m]. */
typedef struct sfg_ring sfg_ring;
/* ckks.NewParametersFromLiteral + ckks.NewEvaluator (crypto.go:60-110) for a preset other than PN14QP438 */
int sfg_ring_create(sfg_ring **out, int device, int logN, int nq, int np, const uint64_t *moduli, const uint64_t *psi);
void sfg_ring_destroy(sfg_ring *ring);
const char *sfg_ring_last_error(const sfg_ring *ring);     /* ring may be NULL: error of a failed sfg_ring_create */
int sfg_ring_synchronize(sfg_ring *ring);
/* device memory of the ring's device (twins: sfg_malloc, sfg_free, sfg_memcpy_h2d, sfg_memcpy_d2h) */
int sfg_ring_malloc(sfg_ring *ring, void **dev_ptr, size_t bytes);
int sfg_ring_free(sfg_ring *ring, void *dev_ptr);
int sfg_ring_memcpy_h2d(sfg_ring *ring, void *dst_dev, const void *src_host, size_t bytes);
int sfg_ring_memcpy_d2h(sfg_ring *ring, void *dst_host, const void *src_dev, size_t bytes);
/* lattigo ring.NTT / ring.InvNTT behind crypto/basics.go (twins: sfg_ntt_rows, sfg_intt_rows): nrows device rows of N canonical words, natural order in,
 * bit-reversed out; mod_idx_host[r] in 0..nq+np-1 */
int sfg_ring_ntt_rows(sfg_ring *ring, uint64_t *rows_dev, int nrows, const int *mod_idx_host);
int sfg_ring_intt_rows(sfg_ring *ring, uint64_t *rows_dev, int nrows, const int *mod_idx_host);
/* cryptoParams.RotKs (crypto.go:50; generated at mhe.go:73, crypto.go:232-275) and cryptoParams.Rlk (crypto.go:47) (twins: sfg_ctx_load_rotkey,
 * sfg_ctx_has_rotkey, sfg_ctx_load_relinkey, sfg_galois_for_rotation) */
int sfg_ring_load_rotkey(sfg_ring *ring, uint64_t galois_el, const uint64_t *key_host, int montgomery_form);
int sfg_ring_has_rotkey(const sfg_ring *ring, uint64_t galois_el);
int sfg_ring_load_relinkey(sfg_ring *ring, const uint64_t *key_host, int montgomery_form);
uint64_t sfg_ring_galois_for_rotation(const sfg_ring *ring, int k_left);
/* crypto.RotateRight / RotateRightWithEvaluator (basics.go:201-224 -> eval.RotateNew): ct j rotated RIGHT by nrot_host[j] mod slots, 0 = copy; in/out may not alias */
int sfg_ring_rotate_right_dev(sfg_ring *ring, const uint64_t *ct_in_dev, uint64_t *ct_out_dev, int nct, int level, const int *nrot_host);
/* eval.ConjugateNew behind crypto.ComplexConjugate / CReal (basics.go:826-846) and any automorphism X -> X^galois_el whose key is loaded; in/out may not alias */
int sfg_ring_ct_galois_dev(sfg_ring *ring, const uint64_t *ct_in_dev, uint64_t *ct_out_dev, int nct, int level, uint64_t galois_el);
/* eval.Add (basics.go:174, matmult.go:1225,1494) and eval.Sub (crypto.CSub, basics.go:575-590) */
int sfg_ring_ct_add_dev(sfg_ring *ring, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int nct, int level);
int sfg_ring_ct_sub_dev(sfg_ring *ring, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int nct, int level);
/* crypto.DropLevel -> eval.DropLevelNew (basics.go:806-824; FlattenLevels :514-531); level_out == level_in copies, level_out > level_in fails; in/out may not alias */
int sfg_ring_ct_drop_level_dev(sfg_ring *ring, const uint64_t *in_dev, uint64_t *out_dev, int nct, int level_in, int level_out);
/* eval.MultByConst / MultByConstAndAdd / AddConst / AddNew(ct, plaintext) behind crypto.CMultConst, CMultConstRescale, AddConst, CAddConst, AddPlain, CPAdd
 * (basics.go:183-199, 472-497, 533-551, 592-611; pca.go:264; qrfact.go:195,280).  scalars_host[level+1]: one canonical residue per modulus (the host side owns
 * lattigo's scaleUpExact and the scale bookkeeping, as for the twins).  out may alias ct. */
int sfg_ring_ct_mul_scalar_dev(sfg_ring *ring, const uint64_t *ct_dev, const uint64_t *scalars_host, uint64_t *out_dev, int nct, int level);
int sfg_ring_ct_mul_scalar_add_dev(sfg_ring *ring, const uint64_t *ct_dev, const uint64_t *scalars_host, uint64_t *acc_dev, int nct, int level);
int sfg_ring_ct_add_scalar_dev(sfg_ring *ring, const uint64_t *ct_dev, const uint64_t *scalars_host, uint64_t *out_dev, int nct, int level);
int sfg_ring_ct_add_plain_dev(sfg_ring *ring, const uint64_t *ct_dev, const uint64_t *pt_dev, size_t pt_stride, uint64_t *out_dev, int nct, int level);
/* eval.MulRelinNew(plaintext, ct) behind crypto.CPMult / Mask (basics.go:110-172): ct j uses pt_dev + j*pt_stride words (0 = one plaintext for all); out may alias ct */
int sfg_ring_ct_mul_plain_dev(sfg_ring *ring, const uint64_t *ct_dev, const uint64_t *pt_dev, size_t pt_stride, uint64_t *out_dev, int nct, int level);
/* eval.MulRelinNew(a, b) behind crypto.CMult (basics.go:386-470): tensor product + relinearisation, no rescale; out may alias neither input */
int sfg_ring_ct_mulrelin_dev(sfg_ring *ring, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, int nct, int level);
/* one step of eval.Rescale (basics.go:123,394) = ring.DivRoundByLastModulusNTT: in [nct][2][level+1][N] -> out [nct][2][level][N]; fails at level 0; in/out may not alias */
int sfg_ring_ct_rescale_dev(sfg_ring *ring, const uint64_t *in_dev, uint64_t *out_dev, int nct, int level);
/* crypto.InnerSumAll (basics.go:278-292): needs the keys of the left rotations by 1, 2, 4, .., slots/2; in/out may not alias */
int sfg_ring_ct_innersum_dev(sfg_ring *ring, const uint64_t *in_dev, int nct, int level, uint64_t *out_dev);

/* ---- the general ring's two ends (gring_io.hip): encode, encrypt, decrypt and decode at every ring sfg_ring_create accepts ----
 * The twins of the sfg_ctx calls of "C6 on the device" and "the way back out" above, same layouts: the encryption in the ring's integer words, the two embeddings in
 * double-double; PARITY UNPINNED in the same sense.  The ring carries no scale: every encoding and decoding call is given one.  Every refusal returns 1 with the cause
 * in sfg_ring_last_error and launches nothing (the encoder's rounding and domain refusals come after its own launches and before anything is written to the caller's
 * buffer); a count of 0 returns 0. */
/* cryptoParams.Pk.Value (crypto.go:45, what crypto.go:355 NewEncryptorFromPk takes): [2][nq+np][N] NTT-domain words; montgomery_form != 0 for lattigo's stored form */
int sfg_ring_load_public_key(sfg_ring *ring, const uint64_t *pk_host, int montgomery_form);
int sfg_ring_has_public_key(const sfg_ring *ring);
/* cryptoParams.Sk.Value (crypto.go:44): secret key or key shard, rows [nq][N] in the NTT domain.  Wiped from device memory in sfg_ring_destroy. */
int sfg_ring_load_secret_key(sfg_ring *ring, const uint64_t *sk_host, int montgomery_form);
/* the sampler's key (replaces the PRNG lattigo's NewEncryptorFromPk draws from crypto/rand, crypto.go:355), as sfg_ctx_seed_encryptor: 32 bytes from the caller's
 * CSPRNG, no default, ONE atomic 64-bit encryption index per ring, a call takes nct consecutive indices, seeding resets it to 0.  Wiped from host and device memory
 * in sfg_ring_destroy; never part of an error string.  The map from stream bytes to samples is sfg_ctx's with the coefficient's high part ranging over N/512 instead
 * of 32: at N = 16384 the two samplers give the same polynomials for the same key and index. */
int sfg_ring_seed_encryptor(sfg_ring *ring, const uint8_t *key32);
int sfg_ring_encryptor_next_index(sfg_ring *ring, uint64_t *next_index);      /* fails on a NULL next_index */
/* the deterministic core of pkEncryptor.EncryptNew (lattigo ckks/encryptor.go encrypt(), the ModDown branch; crypto.go:340-388), as sfg_encrypt_explicit_dev:
 * u int8 [nct][N], e0, e1 int32 [nct][N], pt_dev NULL (zero) or [nct][level+1][N], out_dev [nct][2][level+1][N].  For every modulus m of Q_0..Q_level and of P:
 * t_i = pk_i (.) NTT(u) + NTT(e_i);  c_i = ModDown_P(t_i) with the key switch's float-corrected extension (np = 1: a raw copy);  c_0 += pt. */
int sfg_ring_encrypt_explicit_dev(sfg_ring *ring, const uint64_t *pt_dev, int nct, int level, const int8_t *u_dev, const int32_t *e0_dev, const int32_t *e1_dev,
                                  uint64_t *out_dev);
/* crypto.CZeroMat + eval.Add (matmult.go:1174,1225,1443,1494): ct += Enc(0) in place with fresh samples (nct indices); bit-identical to the explicit form, added.
 * On zeroed words it gives crypto.CZeros (basics.go:367-384); on (pt, 0) it gives encryptor.EncryptNew(pt) (crypto.go:355-361): c_0 += pt is the core's last step.
 * The workspace is reserved before the indices are taken: a call that fails spends none. */
int sfg_ring_ct_add_fresh_zero_dev(sfg_ring *ring, uint64_t *ct_dev, int nct, int level);
/* test hook (replaces nothing in the reference): the samples u, e0, e1 ([nct][N] int8 / int32 / int32) of encryption indices first_index .. first_index + nct - 1
 * under the seeded key, without advancing the counter.  Refused unless the process set SFG_ENABLE_TEST_HOOKS=1 before sfg_ring_create. */
int sfg_ring_encrypt_transcript_for_test(sfg_ring *ring, uint64_t first_index, int nct, int8_t *u_dev, int32_t *e0_dev, int32_t *e1_dev);
/* mpc/mhe.go:107-220 CollectiveDecrypt*, the local half before the aggregation (PCKSProtocol.GenShare with the reference's zero public key), as sfg_pcks_gen_share_dev:
 *   h0 [nct][level+1][N] = ModDown_P(NTT_QP(e0)) + sk (.) c1,     h1 [nct][level+1][N] = ModDown_P(NTT_QP(e1))
 * through the encryption core with u = 0 and no plaintext (the same code path).  e0, e1 int32 [nct][N] from the caller; h1_dev may be NULL (then e1_dev is not read). */
int sfg_ring_pcks_gen_share_dev(sfg_ring *ring, const uint64_t *ct_dev, int nct, int level, const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
/* the local half after the aggregation (PCKSProtocol.KeySwitch, then .Plaintext()), as sfg_pcks_finish_dev: pt [nct][level+1][N] = c0 + h0agg, NTT domain */
int sfg_ring_pcks_finish_dev(sfg_ring *ring, const uint64_t *ct_dev, int nct, int level, const uint64_t *h0agg_dev, uint64_t *pt_dev);
/* the first half of crypto.DecodeFloatVector (crypto/crypto.go:525-536 -> encoder.Decode: InvNTT, the big-integer CRT with lattigo's Cmp(QHalf) centring, the division
 * by the scale), as sfg_decode_coeffs: pt_dev NTT-domain plaintext rows [level+1][N] per plaintext, pt_stride words apart (>= (level+1) * N: polynomial 0 of resident
 * ciphertexts can be read in place); scale any finite double >= 1; coeffs_host [nct][N]: the centred integer coefficient in (-Q/2, Q/2] divided by the scale, correctly
 * rounded to double unless the exact quotient lies within 2^-96 relative of a rounding boundary (derived for up to 48 mixed-radix digits in gring_io_arith.hpp);
 * a magnitude beyond 2^960 gives an infinity.  The call synchronises.  The embedding that turns coefficients into slot values stays with the caller. */
int sfg_ring_decode_coeffs(sfg_ring *ring, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale, double *coeffs_host);
/* ckks encoder.Encode behind crypto.EncryptFloatVector / EncodeFloatVector (crypto.go:340-362, 394-420), as sfg_encode_vectors_dev: values_host [nvec][N/2] real
 * doubles -> pt_dev [nvec][level+1][N], NTT domain.  scale: a finite double >= 1 (the ring carries none).  p_c = round(scale Re w_c), p_(c+n) = round(scale Im w_c),
 * w_c = (1/n) sum_t v_t zeta^(-5^t c), half away from zero, each reduced modulo every q_i in integer arithmetic.  The embedding runs in double-double; a coefficient
 * whose value lies within B_enc = max(2^-50, 2^-93 (sum |p_c| + n)) of a rounding tie is unproven (derivation: gring_io_arith.hpp): the call
 * then fails, says how many, and hands out no plaintext.  NaN, inf and |p| >= 2^62 fail before anything is written.  Every coefficient handed out is the exactly
 * rounded integer.  The call synchronises. */
int sfg_ring_encode_vectors_dev(sfg_ring *ring, const double *values_host, int nvec, int level, double scale, uint64_t *pt_dev);
/* crypto.EncryptFloatVector (crypto.go:340-362) / one row of EncryptFloatMatrixRow (:364-388), as sfg_encrypt_vectors_dev: sfg_ring_encode_vectors_dev's rows (its
 * refusals first, before an index is spent), encrypted with samples drawn on the device (nct indices): out_dev [nct][2][level+1][N].  Bit-identical to
 * sfg_ring_encrypt_explicit_dev on the transcript's samples and the encoder's rows. */
int sfg_ring_encrypt_vectors_dev(sfg_ring *ring, const double *values_host, int nct, int level, double scale, uint64_t *out_dev);
/* crypto.DecodeFloatVector (crypto.go:525-536 -> encoder.Decode), as sfg_decode_vectors: sfg_ring_decode_coeffs' quotients kept as double-double pairs, then the
 * forward embedding v_t = sum_c w_c zeta^(5^t c) in double-double, each part rounded to double once.  re_host [nct][N/2] in lattigo's slot order; im_host may be NULL
 * (the real parts are the same bits either way).  |d_t - v_t| <= B max_t |v_t| with B = 2^-53 + 2^-86 (derived in gring_io_arith.hpp).  pt_stride as above. */
int sfg_ring_decode_vectors(sfg_ring *ring, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale, double *re_host, double *im_host);
/* the same with the slot values left on the device (re_dev, im_dev [nct][N/2] doubles; im_dev may be NULL); ordered on the ring's stream, does not synchronise */
int sfg_ring_decode_vectors_dev(sfg_ring *ring, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale, double *re_dev, double *im_dev);
/* crypto.DecryptFloatVector (crypto.go:489-510), as sfg_decrypt_vectors: pt = c0 + sk (.) c1 under the loaded (whole) secret key, then sfg_ring_decode_vectors */
int sfg_ring_decrypt_vectors(sfg_ring *ring, const uint64_t *ct_dev, int nct, int level, double scale, double *re_host, double *im_host);

/* ---- the general ring's collective key generation (gring_keygen.hip): the local halves of mpc.CollectiveInit (mpc/mhe.go:24-81) at every ring sfg_ring_create accepts ----
 * The twins of the sfg_ckg_* / sfg_rtg_* / sfg_rkg_* / sfg_ctx_install_*_dev / sfg_crp_fill_dev block above, call for call: the same layouts (rows [nmod = nq + np][N],
 * NTT domain, canonical words, device memory; shares [nkeys][beta][nmod][N]; errors int32 [..][N]; u int8 [N]), the same key convention (beta = ceil(nq / np); g_i at
 * modulus m is P mod q_m when m < nq && m / np == i, else 0; a rotation key for Galois element g switches from phi_{g^-1}(s)) and the same three equations.
 * PARITY UNPINNED, as there: restated from the published lattigo v2.1 dckks / drlwe; with fresh randomness bit parity with the Go binary cannot exist.  What IS pinned
 * (tests/test_gpu_ring_keygen.py): every share word against the Python-integer statement tests/keygen_ref.py, the PN14 parameters against the specialised context, the
 * sampled forms against the explicit cores on the sampler's transcript, and keys made here carrying a ciphertext through a rotation and a relinearisation.
 * Each call returns 1 with the cause in sfg_ring_last_error and launches nothing: without a QP secret key, with an unseeded encryptor (sampled forms), on a null
 * argument, nkeys < 0, an even Galois element or one >= 2N, a modulus index out of range, an export of an element that has no key.  nkeys == 0 and nrows == 0 return 0. */
/* cryptoParams.Sk.Value over Q and P (crypto.go:44), as sfg_ctx_load_secret_key_qp: sk_host [nq+np][N], NTT domain.  Also provides what sfg_ring_load_secret_key
 * provides.  Wiped from device memory in sfg_ring_destroy. */
int sfg_ring_load_secret_key_qp(sfg_ring *ring, const uint64_t *sk_host, int montgomery_form);
/* CKGProtocol.GenShare (CollectivePubKeyGen, mhe.go:83-105), as sfg_ckg_gen_share_dev: share = -crp (.) sk + NTT(e) */
int sfg_ring_ckg_gen_share_dev(sfg_ring *ring, const uint64_t *crp_dev, const int32_t *e_dev, uint64_t *share_dev);
/* RTGProtocol.GenShare for nkeys Galois elements at once (CollectiveRotKeyGen, mhe.go:381-476), as sfg_rtg_gen_shares_dev:
 *   h_{k,i} = -crp_{k,i} (.) phi_{g_k^-1}(sk) + NTT(e_{k,i}) + g_i sk.  Any nkeys: the call runs in chunks of at most 1024 keys (gring_keygen_plan.hpp). */
int sfg_ring_rtg_gen_shares_dev(sfg_ring *ring, const uint64_t *galois_host, int nkeys, const uint64_t *crp_dev, const int32_t *e_dev, uint64_t *shares_dev);
/* RKGProtocol.GenShareRoundOne (CollectiveRelinKeyGen, mhe.go:478-502), as sfg_rkg_round1_dev: h0_i = -NTT(u) (.) crp_i + g_i sk + NTT(e0_i), h1_i = sk (.) crp_i + NTT(e1_i) */
int sfg_ring_rkg_round1_dev(sfg_ring *ring, const uint64_t *crp_dev, const int8_t *u_dev, const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
/* RKGProtocol.GenShareRoundTwo (mhe.go:478-502), as sfg_rkg_round2_dev: out_i = sk (.) H0agg_i + NTT(e2_i) + (NTT(u) - sk) (.) H1agg_i + NTT(e3_i) */
int sfg_ring_rkg_round2_dev(sfg_ring *ring, const uint64_t *h0agg_dev, const uint64_t *h1agg_dev, const int8_t *u_dev, const int32_t *e2_dev, const int32_t *e3_dev, uint64_t *out_dev);
/* The sampled forms (the CKG / RTG / RKG protocols' own ring.GaussianSampler and TernarySampler reads, mhe.go:83-105, 381-502), as sfg_*_sampled_dev: errors and u from the
 * ring's encryptor stream (sfg_ring_seed_encryptor; the one counter of sfg_ring_encryptor_next_index).  Public key share: 1 index, e = polynomial id 1; rotation
 * shares: nkeys * beta indices, (k, i) at first + k beta + i, e = id 1; round 1: beta + 1 indices (e0, e1 = ids 1, 2), u = id 0 of index first + beta, returned in
 * *u_index (required); round 2: beta indices (e2, e3 = ids 1, 2), u redrawn from u_index and never stored.  *first_index (may be NULL) states the first index taken:
 * sfg_ring_encrypt_transcript_for_test reproduces every sample from it.  Bit-identical to the explicit core on those samples.  The workspace is reserved before an
 * index is taken: a call that fails spends none. */
int sfg_ring_ckg_gen_share_sampled_dev(sfg_ring *ring, const uint64_t *crp_dev, uint64_t *share_dev, uint64_t *first_index);
int sfg_ring_rtg_gen_shares_sampled_dev(sfg_ring *ring, const uint64_t *galois_host, int nkeys, const uint64_t *crp_dev, uint64_t *shares_dev, uint64_t *first_index);
int sfg_ring_rkg_round1_sampled_dev(sfg_ring *ring, const uint64_t *crp_dev, uint64_t *h0_dev, uint64_t *h1_dev, uint64_t *first_index, uint64_t *u_index);
int sfg_ring_rkg_round2_sampled_dev(sfg_ring *ring, const uint64_t *h0agg_dev, const uint64_t *h1agg_dev, uint64_t u_index, uint64_t *out_dev, uint64_t *first_index);
/* Installation of the aggregated keys from device memory (replaces the evaluation-key assembly after the aggregation, mhe.go:60-81), as sfg_ctx_install_*_dev: device
 * to device, no host copy of key words, the words kept as given.  public key = (agg, crp); rotation key k = (agg_{k,i}, crp_{k,i}) under galois_host[k], with its
 * automorphism index; relinearisation key = (round2agg_i, H1agg_i).  As in sfg_ring_load_rotkey a new element's key enters the ring only when it is complete. */
int sfg_ring_install_public_key_dev(sfg_ring *ring, const uint64_t *agg_dev, const uint64_t *crp_dev);
int sfg_ring_install_rotkeys_dev(sfg_ring *ring, const uint64_t *galois_host, int nkeys, const uint64_t *agg_dev, const uint64_t *crp_dev);
int sfg_ring_install_relinkey_dev(sfg_ring *ring, const uint64_t *round2agg_dev, const uint64_t *h1agg_dev);
/* the stored key of a Galois element (what a party would send on, mhe.go:60-81), as sfg_ctx_export_rotkey: exactly (agg, crp) as key_host [beta][2][nmod][N];
 * galois_el 1 = the relinearisation key */
int sfg_ring_export_rotkey(sfg_ring *ring, uint64_t galois_el, uint64_t *key_host);
/* The common reference polynomials (replaces ring.UniformSampler over the fork's frand, mhe.go:49-59), sfg_crp_fill_dev's exact map at any N and any modulus below
 * 2^61 (bitlen(q) up to 61): on PN14's parameters it gives the same words.  out_dev [nrows][N]; row r is global row first_row + r at modulus mod_idx_host[r].  The
 * seed is not retained by the ring. */
int sfg_ring_crp_fill_dev(sfg_ring *ring, const uint8_t *key32_host, uint64_t first_row, size_t nrows, const int *mod_idx_host, uint64_t *out_dev);

/* ---- the general ring's collective bootstrap, local halves (gring_refresh.hip): mpc.BootstrapMatAll / CollectiveBootstrapMat / CollectiveBootstrapVec
 * (mpc/mhe.go:222-376) at every ring sfg_ring_create accepts ----
 * The twins of the four sfg_refresh_* calls above, call for call, with the ring's N and nq: ct [nct][2][level+1][N]; crs, h1, h1agg [nct][nq][N]; h0, h0agg
 * [nct][level+1][N]; mask [nct][N][mask_limbs] two's-complement 64-bit limbs, 1 <= mask_limbs <= 48; e0, e1 [nct][N] int32; out [nct][2][nq][N] at level nq - 1.
 * All rows NTT domain, canonical, device memory.  The secret key is the one sfg_ring_load_secret_key holds.  Randomness (mask, errors, crs) is an input and the
 * aggregation of the shares stays in Go, as for PN14.  Any nct: a call runs in chunks of at most 1024 ciphertexts (gring_refresh_plan.hpp).
 * PARITY UNPINNED, as there: dckks.RefreshProtocol lives in the absent lattigo fork; restated from the published lattigo v2.1.0 / v2.2.0 dckks/refresh.go as
 * orc_refresh_gen_shares / orc_refresh_finish and their _scaled forms state it (oracle/sfgwas_oracle.c).  What IS pinned (tests/test_gpu_ring_refresh.py): every
 * word of h0, h1 and out against Python integers (tests/ring_refresh_ref.py), and PN14's parameters against the specialised context word for word.
 * The device big integer has 48 limbs (3072 bits).  The target-scale forms require bits(Q_level) + 54 + max(sh, 0) <= 3070, and the share form
 * 64 mask_limbs + 54 + max(sh, 0) <= 3072 as well, sh = the exponent of Int(target scale) minus that of Int(ct scale): every ring fits at the reference's pairs.
 * Each call returns 1 with the cause in sfg_ring_last_error and launches nothing: without a secret key (the share forms), on a null pointer, a level out of range,
 * nct < 0, mask_limbs outside 1..48, a scale that is not finite, below 1 or above 2^400, a product that does not fit.  nct == 0 returns 0. */
/* RefreshProtocol.GenShares (mhe.go:251,315), as sfg_refresh_gen_shares_dev: h0 = NTT_level(mask + e0) + sk (.) c1; h1 = -(NTT(mask + e1) + sk (.) crs) over all nq moduli */
int sfg_ring_refresh_gen_shares_dev(sfg_ring *ring, const uint64_t *ct_dev, int nct, int level, const uint64_t *crs_dev, const uint64_t *mask_dev, int mask_limbs,
                                    const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
/* RefreshProtocol.Decrypt, Recode, Recrypt (mhe.go:256-258,329-331), as sfg_refresh_finish_dev: x = INTT_level(c0 + h0agg) as a big integer, negative when
 * x >= floor(Q_level / 2), reduced into all nq moduli; c0' = NTT(x) + h1agg, c1' = crs */
int sfg_ring_refresh_finish_dev(sfg_ring *ring, const uint64_t *ct_dev, int nct, int level, const uint64_t *h0agg_dev, const uint64_t *h1agg_dev, const uint64_t *crs_dev,
                                uint64_t *out_dev);
/* The target-scale forms the reference calls (mhe.go:251,315 GenShares(..., parameters.Scale(), ...); mhe.go:256-258,329-331 Recode(ct, parameters.Scale())), as
 * sfg_refresh_gen_shares_scaled_dev / sfg_refresh_finish_scaled_dev: h1 from Quo(mask Int(target), Int(ct scale)); x <- Quo(x Int(target), Int(ct scale)) before
 * the re-reduction; Quo truncates towards zero.  ct_scale == target_scale takes the unscaled path. */
int sfg_ring_refresh_gen_shares_scaled_dev(sfg_ring *ring, const uint64_t *ct_dev, int nct, int level, double ct_scale, double target_scale, const uint64_t *crs_dev,
                                           const uint64_t *mask_dev, int mask_limbs, const int32_t *e0_dev, const int32_t *e1_dev, uint64_t *h0_dev, uint64_t *h1_dev);
int sfg_ring_refresh_finish_scaled_dev(sfg_ring *ring, const uint64_t *ct_dev, int nct, int level, double ct_scale, double target_scale, const uint64_t *h0agg_dev,
                                       const uint64_t *h1agg_dev, const uint64_t *crs_dev, uint64_t *out_dev);

/* ---- the general ring's matrix products (gring_matmul.hip): gwas/matmult.go MatMult4Stream at every ring sfg_ring_create accepts ----
 * The twins of sfg_matmul_stream / sfg_matmul_accumulate_dev / sfg_matmul_finalize_dev above with slots = N/2 and d = ceil(sqrt(slots)), in the ring's integer
 * arithmetic; the layouts are those of orc_matmult_accumulate / orc_matmult_finalize (oracle/sfgwas_oracle.c), so words compare directly:
 *   A    [s][nbr][2][in_level+1][N], nbr = ceil(rows / slots) of the OPERAND (the matrix, or its transpose with SFG_TRANSPOSE)
 *   acc  [m_ct][d][s][2][L][N] canonical residues, L = max_level, m_ct = ceil(columns of the operand / slots); zero where a giant step never became active
 *   out  [s][m_ct][2][L][N] at level L - 1
 * geno_dev: int8 [nrow][ld] in device memory of sfg_ring_malloc, ld >= ncol (sfg_geno belongs to sfg_ctx and is not used here).  Missing (negative) genotypes count
 * as 0; SFG_SQUARE squares after that with the int8 wrap-around of matmult.go:1301-1303; SFG_TRANSPOSE multiplies by the transpose of the same bytes, no copy made.
 * The level drops to min(in_level, max_level) (matmult.go:1256-1259); the diagonal of shift giant d + baby is rotated right by d giant and encoded at `scale` (a
 * finite double >= 1; the ring carries none) over the first L moduli by sfg_ring_encode_vectors_dev's encoder, from device memory: no diagonal crosses the host.
 * A coefficient inside that encoder's proven band of a rounding tie is re-derived exactly on the device (gring_tie.hpp: the slot values read again from the matrix
 * bytes, a fixed-point cosine table of 191 fractional bits kept by the ring, integer sums; no host synchronisation is added) and counted by
 * sfg_ring_encoder_resolved.  Only a coefficient whose exact value is itself within the table's error of a tie (S 2^-191, S = scale sum |v_t| / n; an exact tie
 * included), one past the 512 flagged coefficients a batch of diagonals may hold, or one outside |p| < 2^62 fails the call with the encoder's message before `out`
 * is written.
 * The MAC sums rot (.) pt in 128 bits with no Montgomery form: REDC(rot MForm(pt)) = rot pt mod q, so the canonical words are the reference's.  The reference's u128
 * sum silently wraps once terms (q - 1)^2 >= 2^128 (64 terms at 61-bit moduli; d alone is 182 at logN 16); the MAC folds its sum to a word below q every
 * floor((2^128 - q) / (q - 1)^2) terms, so the DEFINED result is the exact sum modulo q.  That equals the reference wherever the reference does not wrap, which is
 * at every lattigo preset (55-bit words allow 2^18 terms).
 * Each refusal returns 1 with the cause in sfg_ring_last_error, launches nothing and writes nothing: s, nrow or ncol not positive; ld < ncol; a level out of range,
 * max_level < 1 or min(in_level, max_level) + 1 < max_level; a bad block-row or giant range; a scale that is not finite or below 1; out, acc or the matrix
 * overlapping A; an unknown flag bit; a missing rotation key, named by its left rotation, looked for over every baby and giant the call needs before its first
 * launch. */
/* gwas/matmult.go:1238-1505 MatMult4Stream (block products at :1280-1439, giant-step alignment and aggregation at :1443-1502): the accumulate over all block rows
 * followed by the finalize over all giants; the accumulator lives in the ring's workspace, in chunks of ciphertexts under the products' byte budget (32 GiB; every
 * chunk encodes the diagonals again) */
int sfg_ring_matmul_dev(sfg_ring *ring, const uint64_t *A_dev, int s, int in_level, int max_level, const int8_t *geno_dev, size_t nrow, size_t ncol, size_t ld,
                        unsigned flags, double scale, uint64_t *out_dev);
/* matmult.go:1280-1439 and the reduction of :343-366 (ModularReduceV2) for operand block rows [b0, b1): rotation cache, diagonals, encode, lazy MAC, canonical
 * residues.  giant_active_host [d] (may be NULL) is set where a giant step became active.  Partial accumulators of disjoint ranges add up modulo q to the whole's. */
int sfg_ring_matmul_accumulate_dev(sfg_ring *ring, const uint64_t *A_dev, int s, int in_level, int max_level, const int8_t *geno_dev, size_t nrow, size_t ncol, size_t ld,
                                   unsigned flags, double scale, int b0, int b1, uint64_t *acc_dev, uint8_t *giant_active_host);
/* matmult.go:1443-1502: RotateRight(acc of giant g, -g d) at level L - 1 for the active giants g > 0 of [g0, g1) (giant_active_host NULL: all) and eval.Add; out is
 * overwritten unless `accumulate` */
int sfg_ring_matmul_finalize_dev(sfg_ring *ring, const uint64_t *acc_dev, const uint8_t *giant_active_host, int s, int max_level, int m_ct, int g0, int g1,
                                 int accumulate, uint64_t *out_dev);
/* test hook (replaces nothing in the reference): the byte budget that sizes the chunks of the ring's evaluator workspaces (key switch, rescale: 768 MiB; the products: 32 GiB), so
 * that a small shape runs in several chunks.  Refused unless the process set SFG_ENABLE_TEST_HOOKS=1 before sfg_ring_create. */
int sfg_ring_set_ws_budget_for_test(sfg_ring *ring, size_t bytes);
/* diagonal coefficients the products re-derived exactly since the last reset (every re-derivation counts: a product in several chunks of ciphertexts encodes its
 * diagonals once per chunk and once more in its checking pass).  Host arithmetic; the count is complete when the product has returned. */
int sfg_ring_encoder_resolved(sfg_ring *ring, unsigned long long *count, int reset);
/* test hook (replaces nothing in the reference): the floor 2^log2_floor (-50 .. -2; the library's is 2^-50) of the band inside which a coefficient of the PRODUCTS'
 * diagonals goes to the exact re-derivation, so that ordinary data exercises it.  sfg_ring_encode_vectors_dev and sfg_ring_encrypt_vectors_dev keep their band.
 * Refused unless the process set SFG_ENABLE_TEST_HOOKS=1 before sfg_ring_create. */
int sfg_ring_set_tie_band_for_test(sfg_ring *ring, int log2_floor);

#ifdef __cplusplus
}
#endif
#endif
