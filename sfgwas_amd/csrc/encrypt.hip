// encrypt.hip — public-key encryption on the device: crypto.CZeros / CZeroMat (crypto/basics.go:367-384) and crypto.EncryptFloatVector /
// EncryptFloatMatrixRow (crypto.go:340-388) -> lattigo ckks pkEncryptor.EncryptNew.  PARITY UNPINNED: restated from the published lattigo v2.1
// (ckks/encryptor.go, the "not fast" form: sample in R_QP, ModDown by P); with fresh randomness bit parity with the Go binary cannot exist anyway.
//
// Per ciphertext at level l (nl = l + 1 moduli of Q, np special primes, nt = nl + np targets), from a ternary u and two Gaussian e0, e1:
//   1. for every target m:  t0_m = pk0_m (.) NTT_m(u) + NTT_m(e0),  t1_m = pk1_m (.) NTT_m(u) + NTT_m(e1)          (k_enc_fwd)
//      ONE workgroup per ciphertext keeps the three small polynomials in registers (24 dwords a thread: bytes) and walks the targets; the u64 rows of
//      u, e0, e1 never exist, and with the sampler on neither do the small polynomials: they come out of the ChaCha20 stream in the same kernel.
//      (NTT(e0), NTT(e1) wait in the rows of T that t0, t1 then take; NTT(u) lives in registers only.)
//   2. INTT of the 2 np special-prime rows                                                                        (k_ntt_inv, ntt.hip)
//   3. for every Q row: basis extension P -> q_m of the coefficient column in registers (the key switch's float-corrected one, ksw.hpp), its NTT,
//      and (t_m - ext) * P^-1 + {plaintext | ciphertext already there} as that transform's epilogue             (k_enc_tail)
// The arithmetic of 3 is rotate.hip's k_moddown_extend + k_ksw_finish word for word, so the result is what lattigo's ModDownNTTPQ gives.
// Row j <= l of the result depends on modulus j and the P rows only: encrypting at level l gives rows 0..l of the MaxLevel encryption.
//
// The sampler (DESIGN.md "Encryption on the device" states the byte map; tests/encrypt_ref.py restates it): ChaCha20 (RFC 8439) under the key of
// sfg_ctx_seed_encryptor, nonce = (64-bit encryption index, 32-bit polynomial id 0 = u, 1 = e0, 2 = e1), block counter inside a polynomial.
// The stream, the byte-to-sample map and the Gaussian table live in sampler.hpp, which keygen.hip shares; the table's twenty thresholds, as DESIGN.md lists them:
//   0x0fe49b6827cb0a22 0x2e2d1c3d2d673909 0x485d35a4168455fb 0x5ceb732fcf500f03 0x6b909790cec541bc 0x750918a85086780a 0x7a98381b8b05d44b
//   0x7d8e6d674ccde58a 0x7efd1569779956ed 0x7f9e04eac7bbada7 0x7fde228ae318bb83 0x7ff551b87c6c82e1 0x7ffcedaa42aca3e8 0x7fff31ef2eb41935
//   0x7fffced272bc4241 0x7ffff5523bb74b16 0x7ffffde5526b5ceb 0x7fffffa10a4c8db3 0x7ffffff2720cd7c6 0x8000000000000000
#include "common.hpp"
#include "kernels.hpp"
#include "ntt_core.hpp"
#include "ksw.hpp"
#include "sampler.hpp"      // the keyed stream and the byte-to-sample map

// ---------------------------------------------------------------- 1. sampling + first transforms
struct EncSrc { const int8_t *u; const int32_t *e0, *e1; const unsigned *key; u64 index0; };     // key != nullptr: the sampler; else the caller's polynomials [nct][N]
// grid nct, 512 threads.  T: [nct][2][nt][N], rows Q_0..level then P (canonical, NTT domain).  pk: [2][nmod][N].
template <bool SAMPLE>
__global__ void __launch_bounds__(512) k_enc_fwd(EncSrc src, const u64 *pk, u64 *T, int nl, int np, int nq, int nmod, const double *tw_all, const double2 *pack_all, const ModConst *modc) {
    extern __shared__ double lds[];
    const int N = SFG_N, tid = threadIdx.x, nt = nl + np;
    const size_t ct = blockIdx.x;
    unsigned su[8], s0[8], s1[8];
    const int8_t *up = nullptr; const int32_t *e0p = nullptr, *e1p = nullptr;
    if constexpr (SAMPLE) {
        unsigned key[8];
#pragma unroll
        for (int i = 0; i < 8; i++) key[i] = src.key[i];
        enc_sample_thread(key, src.index0 + ct, tid, su, s0, s1);
    } else { up = src.u ? src.u + ct * N : nullptr; e0p = src.e0 + ct * N; e1p = src.e1 + ct * N; }
    const int b = tid >> 4, c = tid & 15;
    for (int t = 0; t < nt; t++) {
        const int m = t < nl ? t : nq + (t - nl);
        const double *tw = tw_all + (size_t)m * N;
        const double2 *pack = pack_all + (size_t)m * (N / 2);
        const double q = modc[m].q, qinv = modc[m].qinv;
        double v[32];
        // NTT_m(e0), NTT_m(e1): the signed coefficients go in as they are (|x| < q, the bound the lazy stages take canonical input at).  The canonical transforms wait
        // in the rows of T that the results will take - each thread reads back only the words it wrote itself - so that no transform is held in registers across the next
        // (32 more doubles a thread would spill: 512-thread workgroups have 256 registers a lane)
#pragma unroll 1
        for (int p = 0; p < 2; p++) {
            if constexpr (SAMPLE) {
#pragma unroll
                for (int a = 0; a < 32; a++) v[a] = p ? byte_of(s1, a) : byte_of(s0, a);
            } else {
                const int32_t *ep = p ? e1p : e0p;
#pragma unroll
                for (int a = 0; a < 32; a++) v[a] = (double)ep[a * 512 + tid];
            }
            ntt_fwd_phases(v, lds, tw, pack, q, qinv, tid);
            u64 *out = T + ((ct * 2 + p) * (size_t)nt + t) * N;
#pragma unroll
            for (int a = 0; a < 32; a++) out[a * 512 + tid] = f64_to_u64(canon(lds[a * LDS_ROW + c * 33 + b], q, qinv));
            __syncthreads();                                       // the image has been read
        }
        // NTT_m(u), and as its epilogue t_p = pk_p (.) u^ + e_p^
        if (!SAMPLE && !pk) continue;                              // (uniform) the zero public key of a collective key switch (decrypt.hip): u drops out, t_p = e_p^ as written
#pragma unroll
        for (int a = 0; a < 32; a++) v[a] = SAMPLE ? byte_of(su, a) : (double)up[a * 512 + tid];
        ntt_fwd_phases(v, lds, tw, pack, q, qinv, tid);
#pragma unroll
        for (int a = 0; a < 32; a++) v[a] = canon(lds[a * LDS_ROW + c * 33 + b], q, qinv);
#pragma unroll 1
        for (int p = 0; p < 2; p++) {
            const u64 *pkr = pk + ((size_t)p * nmod + m) * N;
            u64 *out = T + ((ct * 2 + p) * (size_t)nt + t) * N;
#pragma unroll
            for (int a = 0; a < 32; a++) {
                const double r = mulmod2(u64_to_f64(pkr[a * 512 + tid]), v[a], q, qinv) + u64_to_f64(out[a * 512 + tid]);
                out[a * 512 + tid] = f64_to_u64(canon(r, q, qinv));
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- 3. ModDown tail
// grid nct * 2 * nl, 512 threads: row (ct, p, t).  T as above with its P rows in the COEFFICIENT domain.  MODE 0: out = result (+ pt on polynomial 0 when pt != nullptr);
// MODE 1: out += result (in place on a resident ciphertext).  out: [nct][2][nl][N]; pt: [nct][nl][N].
template <int MODE>
__global__ void __launch_bounds__(512) k_enc_tail(const u64 *T, const u64 *pt, u64 *out_, const KswConst *kcp, const double *tw_all, const double2 *pack_all, const ModConst *modc) {
    extern __shared__ double lds[];
    const KswConst &kc = *kcp;
    const int N = SFG_N, tid = threadIdx.x, nl = kc.nl, nt = kc.nt;
    const size_t row = blockIdx.x; const int t = (int)(row % nl), p = (int)((row / nl) & 1); const size_t ct = row / (2 * (size_t)nl);
    const ExtConst &e = kc.pq;
    const double *tw = tw_all + (size_t)t * N;
    const double2 *pack = pack_all + (size_t)t * (N / 2);
    const double q = modc[t].q, qinv = modc[t].qinv;
    const u64 *Tp = T + ((ct * 2 + p) * (size_t)nt + nl) * N;
    double v[32];
#pragma unroll
    for (int a = 0; a < 32; a++) {
        const int x = a * 512 + tid;
        double xs[KSW_MAXA], y[KSW_MAXA], vv = 0.0;
#pragma unroll
        for (int m = 0; m < KSW_MAXA; m++) xs[m] = m < e.a ? u64_to_f64(Tp[(size_t)m * N + x]) : 0.0;
        if (e.a == 1) v[a] = canon(xs[0], q, qinv);
        else { ext_prepare(e, modc, xs, y, vv); v[a] = ext_target(e, t, q, qinv, y, vv); }
    }
    ntt_fwd_phases(v, lds, tw, pack, q, qinv, tid);
    const double pinv = kc.pinv[t], pinv_q = kc.pinv_q[t];
    const u64 *Tq = T + ((ct * 2 + p) * (size_t)nt + t) * N;
    u64 *out = out_ + ((ct * 2 + p) * (size_t)nl + t) * N;
    const u64 *add = MODE == 1 ? out : (p == 0 && pt) ? pt + (ct * (size_t)nl + t) * N : nullptr;
    const int b = tid >> 4, c = tid & 15;
#pragma unroll
    for (int a = 0; a < 32; a++) {
        const int x = a * 512 + tid;
        const double ext = canon(lds[a * LDS_ROW + c * 33 + b], q, qinv);
        double r = mulmod_lazy(u64_to_f64(Tq[x]) - ext, pinv, pinv_q, q);
        if (add) r += u64_to_f64(add[x]);
        out[x] = f64_to_u64(canon(r, q, qinv));
    }
}

// the samples themselves (test hook; also what DESIGN.md's byte map is checked against): grid nct, 512 threads
__global__ void __launch_bounds__(512) k_enc_transcript(const unsigned *keyp, u64 index0, int8_t *u, int32_t *e0, int32_t *e1) {
    const int N = SFG_N, tid = threadIdx.x; const size_t ct = blockIdx.x;
    unsigned key[8], su[8], s0[8], s1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = keyp[i];
    enc_sample_thread(key, index0 + ct, tid, su, s0, s1);
#pragma unroll
    for (int a = 0; a < 32; a++) {
        u[ct * N + a * 512 + tid] = (int8_t)(int)byte_of(su, a);
        e0[ct * N + a * 512 + tid] = (int)byte_of(s0, a);
        e1[ct * N + a * 512 + tid] = (int)byte_of(s1, a);
    }
}

int encrypt_set_attrs(sfg_ctx *ctx) {
    if (sfg_raise_lds({(const void *)k_enc_fwd<false>, (const void *)k_enc_fwd<true>, (const void *)k_enc_tail<0>, (const void *)k_enc_tail<1>}, LDS_DOUBLES * 8) != hipSuccess)
        SFG_FAIL(ctx, "cannot raise dynamic LDS limit for the encryption kernels");
    return 0;
}
static void wipe(volatile void *p, size_t n) { volatile unsigned char *b = (volatile unsigned char *)p; for (size_t i = 0; i < n; i++) b[i] = 0; }
void sfg_encrypt_destroy(SfgShared *sh) {
    wipe(sh->enc_key, sizeof sh->enc_key);
    if (sh->enc_key_dev) { (void)hipMemset(sh->enc_key_dev, 0, 32); (void)hipDeviceSynchronize(); (void)hipFree(sh->enc_key_dev); sh->enc_key_dev = nullptr; }
    sh->enc_seeded = false;
    (void)hipFree(sh->pk_dev); sh->pk_dev = nullptr;
}

// ---------------------------------------------------------------- host side
// the three steps for nct ciphertexts, in the chunks of enc_core_plan (batch_plan.hpp: the T rows of a chunk fit its budget).  mode 0: out = Enc(pt) (pt nullable: zero); mode 1: out += Enc(0)
static int encrypt_run(sfg_ctx *ctx, const EncSrc &src0, const u64 *pk, const u64 *pt, int nct, int level, int mode, u64 *out) {
    const int N = SFG_N, nl = level + 1, np = ctx->np, nt = nl + np;
    const KswConst *kcd, *kc;
    SFG_TRY(get_ksw(ctx, level, &kcd, &kc));
    ApiScope scope(ctx);
    const BatchPlan plan = enc_core_plan(nct, nl, np, (size_t)N);
    void *Tp = nullptr;
    SFG_TRY(sfg_scratch(ctx, "encrypt.T", plan.bytes, &Tp));
    u64 *T = (u64 *)Tp;
    const ModPattern pp = mod_pattern_run(ctx->nq, np);
    RowMap rm; rm.rpg = np; rm.gstride_in = (size_t)nt * N; rm.gstride_out = (size_t)nt * N;
    PhaseTimer timer(ctx, "encrypt");
    int launches = 0;
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct);
        EncSrc src = src0;
        if (src.key) src.index0 += (u64)c0;
        else { if (src.u) src.u += (size_t)c0 * N; src.e0 += (size_t)c0 * N; src.e1 += (size_t)c0 * N; }
        sfg_by_sampled(src.key != nullptr, [&](auto sampled) {
            hipLaunchKernelGGL(k_enc_fwd<decltype(sampled)::value>, dim3(nb), dim3(512), LDS_DOUBLES * 8, ctx->stream, src, pk, T, nl, np, ctx->nq, ctx->nmod, ctx->tw_fwd, ctx->pack_fwd, ctx->modc);
        });
        SFG_HIP(ctx, hipGetLastError());
        SFG_TRY(launch_ntt_inv_map(ctx, T + (size_t)nl * N, T + (size_t)nl * N, (size_t)nb * 2 * np, pp, rm));
        u64 *o = out + (size_t)c0 * 2 * nl * N;
        const u64 *ptc = pt ? pt + (size_t)c0 * nl * N : nullptr;
        if (mode == 1) hipLaunchKernelGGL(k_enc_tail<1>, dim3((unsigned)((size_t)nb * 2 * nl)), dim3(512), LDS_DOUBLES * 8, ctx->stream, (const u64 *)T, (const u64 *)nullptr, o, (const KswConst *)kcd, ctx->tw_fwd, ctx->pack_fwd, ctx->modc);
        else hipLaunchKernelGGL(k_enc_tail<0>, dim3((unsigned)((size_t)nb * 2 * nl)), dim3(512), LDS_DOUBLES * 8, ctx->stream, (const u64 *)T, ptc, o, (const KswConst *)kcd, ctx->tw_fwd, ctx->pack_fwd, ctx->modc);
        SFG_HIP(ctx, hipGetLastError());
        launches += 3;
    }
    timer.stop(launches);
    return 0;
}

static int enc_check_common(sfg_ctx *ctx, const char *what, int nct, int level) {
    if (!ctx->sh->pk_dev) SFG_FAIL(ctx, "%s: no public key loaded (sfg_ctx_load_public_key)", what);
    SFG_TRY(check_level_count(ctx, what, nct, level, 0, 1));
    if (ctx->np < 1 || ctx->np > KSW_MAXA) SFG_FAIL(ctx, "%s: needs 1..%d special primes", what, KSW_MAXA);
    return 0;
}
// takes nct consecutive encryption indices from the ONE counter the root and its forks share
int enc_take_indices(sfg_ctx *ctx, const char *what, int nct, u64 *first) {
    SfgShared *sh = ctx->sh;
    if (!sh->enc_seeded) SFG_FAIL(ctx, "%s: the encryptor has no key (sfg_ctx_seed_encryptor); there is no default", what);
    u64 cur = __atomic_load_n(&sh->enc_next, __ATOMIC_ACQUIRE);
    for (;;) {
        if (cur > ~0ULL - (u64)nct) SFG_FAIL(ctx, "%s: the encryption index space of this key is used up (re-seed)", what);
        if (__atomic_compare_exchange_n(&sh->enc_next, &cur, cur + (u64)nct, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) break;
    }
    *first = cur;
    return 0;
}

// cryptoParams.Pk.Value (crypto.go:45): [2][nq+np][N], NTT domain
extern "C" int sfg_ctx_load_public_key(sfg_ctx *ctx, const uint64_t *pk_host, int mont) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!pk_host) SFG_FAIL(ctx, "load_public_key: NULL key");
    const size_t rows = (size_t)2 * ctx->nmod, words = rows * SFG_N;
    if (!ctx->sh->pk_dev) SFG_HIP(ctx, hipMalloc(&ctx->sh->pk_dev, words * 8));
    SFG_HIP(ctx, hipMemcpyAsync(ctx->sh->pk_dev, pk_host, words * 8, hipMemcpyHostToDevice, ctx->stream));
    if (mont) SFG_TRY(sfg_rows_from_montgomery(ctx, ctx->sh->pk_dev, rows, ctx->nmod));
    SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
extern "C" int sfg_ctx_has_public_key(const sfg_ctx *ctx) { return ctx->sh->pk_dev ? 1 : 0; }

extern "C" int sfg_ctx_seed_encryptor(sfg_ctx *ctx, const uint8_t *key32) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!key32) SFG_FAIL(ctx, "seed_encryptor: NULL key");
    SfgShared *sh = ctx->sh;
    SFG_TRY(sfg_sync_all(ctx));                                   // (launches of this context that still read the previous key)
    if (!sh->enc_key_dev) SFG_HIP(ctx, hipMalloc(&sh->enc_key_dev, 32));
    for (int i = 0; i < 8; i++) sh->enc_key[i] = (uint32_t)key32[4 * i] | (uint32_t)key32[4 * i + 1] << 8 | (uint32_t)key32[4 * i + 2] << 16 | (uint32_t)key32[4 * i + 3] << 24;
    SFG_HIP(ctx, hipMemcpy(sh->enc_key_dev, sh->enc_key, 32, hipMemcpyHostToDevice));
    __atomic_store_n(&sh->enc_next, 0ULL, __ATOMIC_RELEASE);
    sh->enc_seeded = true;
    return 0;
}
extern "C" int sfg_ctx_encryptor_next_index(const sfg_ctx *ctx, uint64_t *next) {
    if (next) *next = __atomic_load_n(&ctx->sh->enc_next, __ATOMIC_ACQUIRE);
    return 0;
}

// decrypt.hip: (ModDown_P(NTT_QP(e0)), ModDown_P(NTT_QP(e1))) for nct pairs of error polynomials, out [nct][2][level+1][N] - sfg_encrypt_explicit_dev for the zero public
// key (u multiplies zero and drops out) and no plaintext: the same three launches, the same ModDown
int encrypt_errors_moddown(sfg_ctx *ctx, const int32_t *e0, const int32_t *e1, int nct, int level, u64 *out) {
    if (ctx->np < 1 || ctx->np > KSW_MAXA) SFG_FAIL(ctx, "pcks_gen_share: needs 1..%d special primes", KSW_MAXA);
    EncSrc src{nullptr, e0, e1, nullptr, 0};
    return encrypt_run(ctx, src, nullptr, nullptr, nct, level, 0, out);
}
extern "C" int sfg_encrypt_explicit_dev(sfg_ctx *ctx, const uint64_t *pt, int nct, int level, const int8_t *u, const int32_t *e0, const int32_t *e1, uint64_t *out) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(enc_check_common(ctx, "encrypt_explicit", nct, level));
    if (!u || !e0 || !e1 || !out) SFG_FAIL(ctx, "encrypt_explicit: NULL polynomial or output");
    EncSrc src{u, e0, e1, nullptr, 0};
    return encrypt_run(ctx, src, ctx->sh->pk_dev, (const u64 *)pt, nct, level, 0, (u64 *)out);
}
extern "C" int sfg_ct_add_fresh_zero_dev(sfg_ctx *ctx, uint64_t *ct, int nct, int level) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(enc_check_common(ctx, "add_fresh_zero", nct, level));
    if (!ct) SFG_FAIL(ctx, "add_fresh_zero: NULL ciphertexts");
    u64 first; SFG_TRY(enc_take_indices(ctx, "add_fresh_zero", nct, &first));
    EncSrc src{nullptr, nullptr, nullptr, ctx->sh->enc_key_dev, first};
    return encrypt_run(ctx, src, ctx->sh->pk_dev, nullptr, nct, level, 1, (u64 *)ct);
}
extern "C" int sfg_encrypt_vectors_dev(sfg_ctx *ctx, const double *values_host, int nct, int level, uint64_t *out) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(enc_check_common(ctx, "encrypt_vectors", nct, level));
    if (!values_host || !out) SFG_FAIL(ctx, "encrypt_vectors: NULL values or output");
    if (!ctx->sh->enc_seeded) SFG_FAIL(ctx, "encrypt_vectors: the encryptor has no key (sfg_ctx_seed_encryptor); there is no default");
    ApiScope scope(ctx);
    void *ptp = nullptr;
    SFG_TRY(sfg_scratch(ctx, "encrypt.pt", (size_t)nct * (level + 1) * SFG_N * 8, &ptp));
    SFG_TRY(sfg_encode_vectors_dev(ctx, values_host, nct, level, (uint64_t *)ptp));      // the encoder's own rows (and its domain / rounding checks), before an index is spent
    u64 first; SFG_TRY(enc_take_indices(ctx, "encrypt_vectors", nct, &first));
    EncSrc src{nullptr, nullptr, nullptr, ctx->sh->enc_key_dev, first};
    return encrypt_run(ctx, src, ctx->sh->pk_dev, (const u64 *)ptp, nct, level, 0, (u64 *)out);
}
extern "C" int sfg_encrypt_transcript_for_test(sfg_ctx *ctx, uint64_t first_index, int nct, int8_t *u, int32_t *e0, int32_t *e1) {
    if (!ctx->test_hooks) SFG_FAIL(ctx, "sfg_encrypt_transcript_for_test: test hook, enabled only in a process that set the test switch before creating the context");
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->sh->enc_seeded) SFG_FAIL(ctx, "encrypt_transcript: the encryptor has no key (sfg_ctx_seed_encryptor); there is no default");
    if (nct <= 0 || !u || !e0 || !e1) SFG_FAIL(ctx, "encrypt_transcript: count %d must be positive and the outputs given", nct);
    if (first_index > ~0ULL - (u64)nct) SFG_FAIL(ctx, "encrypt_transcript: indices beyond 2^64");
    hipLaunchKernelGGL(k_enc_transcript, dim3(nct), dim3(512), 0, ctx->stream, (const unsigned *)ctx->sh->enc_key_dev, (u64)first_index, u, e0, e1);
    SFG_HIP(ctx, hipGetLastError());
    return 0;
}
