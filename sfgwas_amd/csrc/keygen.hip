// keygen.hip — the local halves of the collective key generation on the device: mpc.CollectiveInit (mpc/mhe.go:24-81) -> CollectivePubKeyGen (:83-105),
// CollectiveRelinKeyGen (:478-502), CollectiveRotKeyGen (:381-476) -> lattigo dckks / drlwe CKGProtocol.GenShare, RKGProtocol.GenShareRoundOne / RoundTwo,
// RTGProtocol.GenShare.  PARITY UNPINNED: restated from the published lattigo v2.1; with fresh randomness and a common reference polynomial the Go binary
// draws from a fork-only PRNG, bit parity with it cannot exist.  What is pinned (tests/test_gpu_keygen.py): every share word against the Python-integer
// statement tests/keygen_ref.py, the sampled forms against the explicit cores on the sampler's transcript, and keys made here carrying a ciphertext through a
// rotation and a relinearisation within the derived noise bound.  The aggregation over the network stays in Go (mpc/aggregate.go:121-240).
//
// All polynomials are rows [nmod = nq + np][N] in the NTT domain, canonical words.  Key convention = the key switch's (rotate.hip; orc_gen_rotkey / orc_gen_rlk):
// digit i = (b_i, a_i), g_i at modulus m = P mod q_m when m < nq && m / np == i, else 0; a rotation key for Galois element g switches from phi_{g^-1}(s).
//   public key share        h       = -crp (.) sk + NTT(e)
//   rotation key share      h_{k,i} = -crp_{k,i} (.) phi_{g_k^-1}(sk) + NTT(e_{k,i}) + g_i sk
//   relin. key, round 1     h0_i    = -NTT(u) (.) crp_i + g_i sk + NTT(e0_i),      h1_i = sk (.) crp_i + NTT(e1_i)
//   relin. key, round 2     out_i   = sk (.) H0agg_i + NTT(e2_i) + (NTT(u) - sk) (.) H1agg_i + NTT(e3_i)
// ONE 512-thread workgroup per share polynomial (key, digit) keeps the small polynomial(s) in registers - drawn from the encryptor's ChaCha20 stream in the same
// kernel (sampler.hpp) or loaded once - and walks the nmod modulus targets with ntt_core.hpp; the epilogue of each target's transform forms the row from crp, sk
// (gathered through the NTT-domain automorphism index of g^-1) and the g_i sk term.  u64 rows of e or u never exist in HBM.  The share kernel (public and rotation
// keys: all but 2 beta polynomials of a key set) writes each row once; the two relinearisation rounds carry two transforms per row (u and an error) and park the first
// in the row the result then takes, as k_enc_fwd does (each thread reads back only the words it wrote itself).
// Scratch per key: the 32 KiB automorphism index; nothing else beyond the caller's outputs.
//
// The common reference polynomials (sfg_crp_fill_dev) replace ring.UniformSampler over the fork's frand (mhe.go:49-59); the map is stated at k_crp_fill and in DESIGN.md.
// Drawing the secret key itself stays with the caller (out of scope here): sfg_ctx_load_secret_key_qp takes its NTT rows.
#include "common.hpp"
#include "kernels.hpp"
#include "ntt_core.hpp"
#include "ksw.hpp"
#include "sampler.hpp"

struct KgConst { double pmod[SFG_MAXMOD]; int nq, np, nmod, beta; };        // pmod[m] = P mod q_m (m < nq)
// g_i at modulus m, as a canonical double (0: no term)
__device__ __forceinline__ double kg_gterm(const KgConst &kc, int digit, int m) { return (digit >= 0 && m < kc.nq && m / kc.np == digit) ? kc.pmod[m] : 0.0; }

// ---------------------------------------------------------------- public / rotation key shares
struct KgShareSrc { const int32_t *e; const unsigned *key; u64 index0; };      // key != nullptr: e = polynomial id 1 of encryption index0 + block; else the caller's e [npoly][N]
// grid npoly = nkeys * beta, 512 threads.  crp, out: [npoly][nmod][N]; sk: [nmod][N]; idx: nullptr (identity: the public key) or [nkeys][N], the NTT-domain
// automorphism index of g_k^-1.  gterm: the rotation keys' g_i sk (digit = block % beta); the public key has none.
template <bool SAMPLE>
__global__ void __launch_bounds__(512) k_kg_share(KgShareSrc src, KgConst kc, const u64 *sk, const u64 *crp, const uint16_t *idx, int gterm, u64 *out_,
                                                  const double *tw_all, const double2 *pack_all, const ModConst *modc) {
    extern __shared__ double lds[];
    const int N = SFG_N, tid = threadIdx.x, nmod = kc.nmod;
    const size_t blk = blockIdx.x;
    const int digit = gterm ? (int)(blk % kc.beta) : -1;
    const uint16_t *ix = idx ? idx + (blk / kc.beta) * N : nullptr;
    unsigned sb[8]; int ev[32];
    if constexpr (SAMPLE) {
        unsigned key[8];
#pragma unroll
        for (int i = 0; i < 8; i++) key[i] = src.key[i];
        enc_sample_e_thread(key, src.index0 + blk, 1u, tid, sb);
    } else {
        const int32_t *ep = src.e + blk * N;
#pragma unroll
        for (int a = 0; a < 32; a++) ev[a] = ep[a * 512 + tid];
    }
    const int b = tid >> 4, c = tid & 15;
    for (int m = 0; m < nmod; m++) {
        const double *tw = tw_all + (size_t)m * N;
        const double2 *pack = pack_all + (size_t)m * (N / 2);
        const double q = modc[m].q, qinv = modc[m].qinv, pg = kg_gterm(kc, digit, m);
        double v[32];
#pragma unroll
        for (int a = 0; a < 32; a++) { if constexpr (SAMPLE) v[a] = byte_of(sb, a); else v[a] = (double)ev[a]; }
        ntt_fwd_phases(v, lds, tw, pack, q, qinv, tid);
        const u64 *skr = sk + (size_t)m * N, *cr = crp + (blk * nmod + m) * N;
        u64 *out = out_ + (blk * nmod + m) * N;
#pragma unroll 4
        for (int a = 0; a < 32; a++) {
            const int x = a * 512 + tid;
            const double sp = u64_to_f64(skr[ix ? (int)ix[x] : x]);
            double r = canon(lds[a * LDS_ROW + c * 33 + b], q, qinv) - mulmod2(u64_to_f64(cr[x]), sp, q, qinv);
            if (pg != 0.0) r += mulmod2(pg, u64_to_f64(skr[x]), q, qinv);
            out[x] = f64_to_u64(canon(r, q, qinv));
        }
        __syncthreads();                                           // the image has been read
    }
}

// ---------------------------------------------------------------- relinearisation key shares
struct KgRkgSrc { const int8_t *u; const int32_t *ea, *eb; const unsigned *key; u64 index0, u_index; };   // key != nullptr: digit i draws (ea, eb) = ids 1, 2 of index0 + i, u = id 0 of u_index
// grid beta, 512 threads.  ROUND 1: A = crp [beta][nmod][N], out0 = h0, out1 = h1 (ea, eb = e0, e1).  ROUND 2: A = H0agg, B = H1agg, out0 = out (ea, eb = e2, e3).
template <int ROUND, bool SAMPLE>
__global__ void __launch_bounds__(512) k_kg_rkg(KgRkgSrc src, KgConst kc, const u64 *sk, const u64 *A, const u64 *B, u64 *out0_, u64 *out1_,
                                                const double *tw_all, const double2 *pack_all, const ModConst *modc) {
    extern __shared__ double lds[];
    const int N = SFG_N, tid = threadIdx.x, nmod = kc.nmod;
    const size_t blk = blockIdx.x;
    unsigned su[8], sa[8], sbb[8];
    const int32_t *eap = nullptr, *ebp = nullptr;
    if constexpr (SAMPLE) {
        unsigned key[8];
#pragma unroll
        for (int i = 0; i < 8; i++) key[i] = src.key[i];
        enc_sample_u_thread(key, src.u_index, tid, su);
        enc_sample_e_thread(key, src.index0 + blk, 1u, tid, sa);
        enc_sample_e_thread(key, src.index0 + blk, 2u, tid, sbb);
    } else {
        eap = src.ea + blk * N; ebp = src.eb + blk * N;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            unsigned w = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) w |= ((unsigned)(int)src.u[(4 * d + k) * 512 + tid] & 0xFFu) << (8 * k);
            su[d] = w;
        }
    }
    const int b = tid >> 4, c = tid & 15;
    for (int m = 0; m < nmod; m++) {
        const double *tw = tw_all + (size_t)m * N;
        const double2 *pack = pack_all + (size_t)m * (N / 2);
        const double q = modc[m].q, qinv = modc[m].qinv, pg = ROUND == 1 ? kg_gterm(kc, (int)blk, m) : 0.0; (void)pg;
        const u64 *skr = sk + (size_t)m * N, *Ar = A + (blk * nmod + m) * N;
        u64 *out0 = out0_ + (blk * nmod + m) * N;
        u64 *out1 = ROUND == 1 ? out1_ + (blk * nmod + m) * N : nullptr;
        const u64 *Br = ROUND == 2 ? B + (blk * nmod + m) * N : nullptr;
        // one transform per step (not unrolled: three inlined transforms would not fit the registers), the row formed in its epilogue:
        //   round 1   step 0: h1 = sk (.) crp + NTT(e1), written once;  step 1: NTT(e0) + g_i sk parked in h0's row;  step 2: h0 -= NTT(u) (.) crp
        //   round 2   step 1: NTT(e2 + e3) + sk (.) (H0agg - H1agg) parked in the result's row;  step 2: += NTT(u) (.) H1agg
#pragma unroll 1
        for (int step = ROUND == 1 ? 0 : 1; step < 3; step++) {
            double v[32];
            if constexpr (SAMPLE) {
#pragma unroll
                for (int a = 0; a < 32; a++) {
                    const double xa = byte_of(sa, a), xb = byte_of(sbb, a), xu = byte_of(su, a);
                    v[a] = step == 2 ? xu : ROUND == 2 ? xa + xb : step == 0 ? xb : xa;
                }
            } else {
#pragma unroll
                for (int a = 0; a < 32; a++) {
                    if (step == 2) v[a] = byte_of(su, a);
                    else if (ROUND == 2) v[a] = (double)eap[a * 512 + tid] + (double)ebp[a * 512 + tid];
                    else v[a] = (double)(step == 0 ? ebp : eap)[a * 512 + tid];
                }
            }
            ntt_fwd_phases(v, lds, tw, pack, q, qinv, tid);
#pragma unroll 4
            for (int a = 0; a < 32; a++) {
                const int x = a * 512 + tid;
                const double h = canon(lds[a * LDS_ROW + c * 33 + b], q, qinv), s = u64_to_f64(skr[x]), av = u64_to_f64(Ar[x]);
                double r;
                if constexpr (ROUND == 1) {
                    if (step == 0) r = h + mulmod2(s, av, q, qinv);
                    else if (step == 1) r = pg != 0.0 ? h + mulmod2(pg, s, q, qinv) : h;
                    else r = u64_to_f64(out0[x]) - mulmod2(h, av, q, qinv);
                    (step == 0 ? out1 : out0)[x] = f64_to_u64(canon(r, q, qinv));
                } else {
                    const double bv = u64_to_f64(Br[x]);
                    if (step == 1) r = h + mulmod2(s, canon(av - bv, q, qinv), q, qinv);
                    else r = u64_to_f64(out0[x]) + mulmod2(h, bv, q, qinv);
                    out0[x] = f64_to_u64(canon(r, q, qinv));
                }
            }
            __syncthreads();                                       // the image has been read
        }
    }
}

// ---------------------------------------------------------------- common reference polynomials
// Row r (global number first_row + blockIdx.y) at modulus q, coefficient j: ChaCha20 block (RFC 8439) under key32 with block counter j and nonce
// (r low word, r high word, try t); its sixteen words form eight 64-bit candidates w[2k] | w[2k+1] << 32, each masked to bitlen(q) bits; the coefficient is the
// first candidate < q, and when none is, the same with t + 1 (t starts at 0).  Every candidate is accepted with probability > 1/2, a try fails with < 2^-8.
struct CrpKey { unsigned k[8]; };
__global__ void __launch_bounds__(256) k_crp_fill(CrpKey key, u64 first_row, const int *mod_idx, const ModConst *modc, u64 *out) {
    const size_t row = blockIdx.y; const int j = blockIdx.x * 256 + threadIdx.x;
    const u64 q = modc[mod_idx[row]].qi, mask = ~0ULL >> __builtin_clzll(q), r = first_row + row;
    unsigned kk[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) kk[i] = key.k[i];
    u64 val = 0; bool found = false;
    for (unsigned t = 0; !found; t++) {
        chacha20_block(kk, (unsigned)j, (unsigned)r, (unsigned)(r >> 32), t, w);
#pragma unroll
        for (int k = 7; k >= 0; k--) { const u64 cand = (((u64)w[2 * k + 1] << 32) | w[2 * k]) & mask; if (cand < q) { val = cand; found = true; } }
    }
    out[row * SFG_N + j] = val;
}

int keygen_set_attrs(sfg_ctx *ctx) {
    if (sfg_raise_lds({(const void *)k_kg_share<false>, (const void *)k_kg_share<true>, (const void *)k_kg_rkg<1, false>, (const void *)k_kg_rkg<1, true>,
                       (const void *)k_kg_rkg<2, false>, (const void *)k_kg_rkg<2, true>}, LDS_DOUBLES * 8) != hipSuccess)
        SFG_FAIL(ctx, "cannot raise dynamic LDS limit for the key-generation kernels");
    return 0;
}
void sfg_keygen_destroy(SfgShared *sh) {
    if (!sh->skqp_dev) return;
    (void)hipMemset(sh->skqp_dev, 0, (size_t)sh->nmod * SFG_N * 8);
    if (sh->sk_dev) (void)hipMemset(sh->sk_dev, 0, (size_t)sh->nq * SFG_N * 8);       // its Q rows (freed by the caller, ctx.hip)
    (void)hipDeviceSynchronize();
    (void)hipFree(sh->skqp_dev); sh->skqp_dev = nullptr;
}

// ---------------------------------------------------------------- host side
static void kg_const(const sfg_ctx *ctx, KgConst &kc) {
    memset(&kc, 0, sizeof kc);
    kc.nq = ctx->nq; kc.np = ctx->np; kc.nmod = ctx->nmod; kc.beta = ctx->beta;
    for (int m = 0; m < ctx->nq; m++) {
        u64 q = ctx->q[m], pg = 1;
        for (int p = 0; p < ctx->np; p++) pg = h_mulmod(pg, ctx->q[ctx->nq + p] % q, q);
        kc.pmod[m] = (double)pg;
    }
}
// lattigo ring.PermuteNTTIndex (as sfg_ctx_load_rotkey builds it): out[i] = in[index[i]] is phi_g in the NTT domain
static void kg_index_table(u64 g, uint16_t *idx) {
    const u64 mask = 2ULL * SFG_N - 1;
    for (int i = 0; i < SFG_N; i++) { u64 t1 = 2ULL * h_brev((uint32_t)i, SFG_LOGN) + 1; u64 t2 = ((g * t1 & mask) - 1) >> 1; idx[i] = (uint16_t)h_brev((uint32_t)t2, SFG_LOGN); }
}
static u64 kg_galois_inverse(u64 g) {           // g odd: Newton's iteration doubles the correct low bits (3 -> 6 -> 12 -> 24 >= 15)
    const u64 mask = 2ULL * SFG_N - 1; u64 x = g;
    for (int i = 0; i < 4; i++) x = (x * (2 - g * x)) & mask;
    return x & mask;
}
static int kg_check_sk(sfg_ctx *ctx, const char *what) {
    if (!ctx->sh->skqp_dev) SFG_FAIL(ctx, "%s: no secret key over QP loaded (sfg_ctx_load_secret_key_qp)", what);
    return 0;
}
static int kg_check_seeded(sfg_ctx *ctx, const char *what) {
    if (!ctx->sh->enc_seeded) SFG_FAIL(ctx, "%s: the encryptor has no key (sfg_ctx_seed_encryptor); there is no default", what);
    return 0;
}
static int kg_check_galois(sfg_ctx *ctx, const char *what, const uint64_t *galois, int nkeys) {
    if (nkeys < 0) SFG_FAIL(ctx, "%s: negative key count %d", what, nkeys);
    if (nkeys > 0 && !galois) SFG_FAIL(ctx, "%s: NULL Galois elements", what);
    for (int k = 0; k < nkeys; k++)
        if (!(galois[k] & 1) || galois[k] >= 2ULL * SFG_N) SFG_FAIL(ctx, "%s: Galois element %llu is not an odd number below 2N", what, (unsigned long long)galois[k]);
    return 0;
}

// cryptoParams.Sk.Value over Q and P: [nq+np][N], NTT domain
extern "C" int sfg_ctx_load_secret_key_qp(sfg_ctx *ctx, const uint64_t *sk_host, int mont) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!sk_host) SFG_FAIL(ctx, "load_secret_key_qp: NULL key");
    SfgShared *sh = ctx->sh;
    const size_t words = (size_t)ctx->nmod * SFG_N, qwords = (size_t)ctx->nq * SFG_N;
    if (!sh->skqp_dev) SFG_HIP(ctx, hipMalloc(&sh->skqp_dev, words * 8));
    if (!sh->sk_dev) SFG_HIP(ctx, hipMalloc(&sh->sk_dev, qwords * 8));
    SFG_HIP(ctx, hipMemcpyAsync(sh->skqp_dev, sk_host, words * 8, hipMemcpyHostToDevice, ctx->stream));
    if (mont) SFG_TRY(sfg_rows_from_montgomery(ctx, sh->skqp_dev, (size_t)ctx->nmod, ctx->nmod));
    SFG_HIP(ctx, hipMemcpyAsync(sh->sk_dev, sh->skqp_dev, qwords * 8, hipMemcpyDeviceToDevice, ctx->stream));      // the rows sfg_ctx_load_secret_key keeps
    SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// shares of npoly = nkeys * beta polynomials (the public key: one, no automorphism, no g term)
static int kg_run_shares(sfg_ctx *ctx, const KgShareSrc &src, const uint64_t *galois, int nkeys, bool pubkey, const u64 *crp, u64 *out) {
    KgConst kc; kg_const(ctx, kc);
    ApiScope scope(ctx);
    const uint16_t *idx_dev = nullptr;
    if (!pubkey) {
        std::vector<uint16_t> idx((size_t)nkeys * SFG_N);
        for (int k = 0; k < nkeys; k++) kg_index_table(kg_galois_inverse(galois[k]), idx.data() + (size_t)k * SFG_N);
        void *p = nullptr;
        SFG_TRY(sfg_scratch(ctx, "keygen.idx", idx.size() * sizeof(uint16_t), &p));
        SFG_TRY(sfg_upload_small(ctx, p, idx.data(), idx.size() * sizeof(uint16_t)));
        idx_dev = (const uint16_t *)p;
    }
    const unsigned npoly = pubkey ? 1u : (unsigned)nkeys * (unsigned)ctx->beta;
    PhaseTimer timer(ctx, "keygen");
    sfg_by_sampled(src.key != nullptr, [&](auto sampled) {
        hipLaunchKernelGGL(k_kg_share<decltype(sampled)::value>, dim3(npoly), dim3(512), LDS_DOUBLES * 8, ctx->stream, src, kc, (const u64 *)ctx->sh->skqp_dev, crp, idx_dev, pubkey ? 0 : 1, out, ctx->tw_fwd, ctx->pack_fwd, ctx->modc);
    });
    SFG_HIP(ctx, hipGetLastError());
    timer.stop(1, (double)npoly * ctx->nmod * SFG_N * 8 * 2);
    return 0;
}

// The four share entry points, each in its explicit form (the caller's small polynomials) and its sampled form (none given: they come from the encryptor's
// stream, `nidx` consecutive encryption indices are taken and the first is reported through first_index, nullable).  kg_sample is the sampled form's step.
static int kg_sample(sfg_ctx *ctx, const char *what, int nidx, const unsigned **key, u64 *index0, uint64_t *first_index) {
    SFG_TRY(enc_take_indices(ctx, what, nidx, index0));           // (refuses an unseeded encryptor)
    if (first_index) *first_index = *index0;
    *key = ctx->sh->enc_key_dev;
    return 0;
}
static int kg_ckg(sfg_ctx *ctx, const char *what, bool sampled, const uint64_t *crp, const int32_t *e, uint64_t *share, uint64_t *first_index) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(kg_check_sk(ctx, what));
    if (!crp || (!sampled && !e) || !share) SFG_FAIL(ctx, "%s: NULL polynomial or output", what);
    KgShareSrc src{e, nullptr, 0};
    if (sampled) SFG_TRY(kg_sample(ctx, what, 1, &src.key, &src.index0, first_index));
    return kg_run_shares(ctx, src, nullptr, 1, true, (const u64 *)crp, (u64 *)share);
}
static int kg_rtg(sfg_ctx *ctx, const char *what, bool sampled, const uint64_t *galois_host, int nkeys, const uint64_t *crp, const int32_t *e, uint64_t *shares, uint64_t *first_index) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(kg_check_sk(ctx, what));
    SFG_TRY(kg_check_galois(ctx, what, galois_host, nkeys));
    if (sampled) SFG_TRY(kg_check_seeded(ctx, what));             // (before the empty call returns)
    if (!nkeys) return 0;
    if (!crp || (!sampled && !e) || !shares) SFG_FAIL(ctx, "%s: NULL polynomial or output", what);
    KgShareSrc src{e, nullptr, 0};
    if (sampled) {
        if ((long long)nkeys * ctx->beta > 0x7FFFFFFFLL) SFG_FAIL(ctx, "%s: too many keys in one call", what);
        SFG_TRY(kg_sample(ctx, what, nkeys * ctx->beta, &src.key, &src.index0, first_index));
    }
    return kg_run_shares(ctx, src, galois_host, nkeys, false, (const u64 *)crp, (u64 *)shares);
}

template <int ROUND>
static int kg_run_rkg(sfg_ctx *ctx, const KgRkgSrc &src, const u64 *A, const u64 *B, u64 *out0, u64 *out1) {
    KgConst kc; kg_const(ctx, kc);
    PhaseTimer timer(ctx, "keygen");
    sfg_by_sampled(src.key != nullptr, [&](auto sampled) {
        hipLaunchKernelGGL((k_kg_rkg<ROUND, decltype(sampled)::value>), dim3(ctx->beta), dim3(512), LDS_DOUBLES * 8, ctx->stream, src, kc, (const u64 *)ctx->sh->skqp_dev, A, B, out0, out1, ctx->tw_fwd, ctx->pack_fwd, ctx->modc);
    });
    SFG_HIP(ctx, hipGetLastError());
    timer.stop(1);
    return 0;
}
// round 1 takes beta + 1 indices (the last is u's, reported through u_index: round 2 needs it); round 2 takes beta and reads u at u_index
static int kg_rkg1(sfg_ctx *ctx, const char *what, bool sampled, const uint64_t *crp, const int8_t *u, const int32_t *e0, const int32_t *e1, uint64_t *h0, uint64_t *h1,
                   uint64_t *first_index, uint64_t *u_index) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(kg_check_sk(ctx, what));
    if (!crp || !h0 || !h1 || (sampled ? !u_index : (!u || !e0 || !e1))) SFG_FAIL(ctx, "%s: NULL polynomial or output%s", what, sampled ? " or u_index (round 2 needs it)" : "");
    KgRkgSrc src{u, e0, e1, nullptr, 0, 0};
    if (sampled) {
        SFG_TRY(kg_sample(ctx, what, ctx->beta + 1, &src.key, &src.index0, first_index));
        *u_index = src.u_index = src.index0 + (u64)ctx->beta;
    }
    return kg_run_rkg<1>(ctx, src, (const u64 *)crp, nullptr, (u64 *)h0, (u64 *)h1);
}
static int kg_rkg2(sfg_ctx *ctx, const char *what, bool sampled, const uint64_t *h0agg, const uint64_t *h1agg, const int8_t *u, const int32_t *e2, const int32_t *e3,
                   uint64_t u_index, uint64_t *out, uint64_t *first_index) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(kg_check_sk(ctx, what));
    if (!h0agg || !h1agg || !out || (!sampled && (!u || !e2 || !e3))) SFG_FAIL(ctx, "%s: NULL polynomial or output", what);
    KgRkgSrc src{u, e2, e3, nullptr, 0, (u64)u_index};
    if (sampled) SFG_TRY(kg_sample(ctx, what, ctx->beta, &src.key, &src.index0, first_index));
    return kg_run_rkg<2>(ctx, src, (const u64 *)h0agg, (const u64 *)h1agg, (u64 *)out, nullptr);
}
extern "C" int sfg_ckg_gen_share_dev(sfg_ctx *ctx, const uint64_t *crp, const int32_t *e, uint64_t *share) { return kg_ckg(ctx, "ckg_gen_share", false, crp, e, share, nullptr); }
extern "C" int sfg_ckg_gen_share_sampled_dev(sfg_ctx *ctx, const uint64_t *crp, uint64_t *share, uint64_t *first_index) { return kg_ckg(ctx, "ckg_gen_share_sampled", true, crp, nullptr, share, first_index); }
extern "C" int sfg_rtg_gen_shares_dev(sfg_ctx *ctx, const uint64_t *galois_host, int nkeys, const uint64_t *crp, const int32_t *e, uint64_t *shares) { return kg_rtg(ctx, "rtg_gen_shares", false, galois_host, nkeys, crp, e, shares, nullptr); }
extern "C" int sfg_rtg_gen_shares_sampled_dev(sfg_ctx *ctx, const uint64_t *galois_host, int nkeys, const uint64_t *crp, uint64_t *shares, uint64_t *first_index) { return kg_rtg(ctx, "rtg_gen_shares_sampled", true, galois_host, nkeys, crp, nullptr, shares, first_index); }
extern "C" int sfg_rkg_round1_dev(sfg_ctx *ctx, const uint64_t *crp, const int8_t *u, const int32_t *e0, const int32_t *e1, uint64_t *h0, uint64_t *h1) { return kg_rkg1(ctx, "rkg_round1", false, crp, u, e0, e1, h0, h1, nullptr, nullptr); }
extern "C" int sfg_rkg_round1_sampled_dev(sfg_ctx *ctx, const uint64_t *crp, uint64_t *h0, uint64_t *h1, uint64_t *first_index, uint64_t *u_index) { return kg_rkg1(ctx, "rkg_round1_sampled", true, crp, nullptr, nullptr, nullptr, h0, h1, first_index, u_index); }
extern "C" int sfg_rkg_round2_dev(sfg_ctx *ctx, const uint64_t *h0agg, const uint64_t *h1agg, const int8_t *u, const int32_t *e2, const int32_t *e3, uint64_t *out) { return kg_rkg2(ctx, "rkg_round2", false, h0agg, h1agg, u, e2, e3, 0, out, nullptr); }
extern "C" int sfg_rkg_round2_sampled_dev(sfg_ctx *ctx, const uint64_t *h0agg, const uint64_t *h1agg, uint64_t u_index, uint64_t *out, uint64_t *first_index) { return kg_rkg2(ctx, "rkg_round2_sampled", true, h0agg, h1agg, nullptr, nullptr, nullptr, u_index, out, first_index); }

// ---------------------------------------------------------------- installation from device memory
// key storage [beta][2][nmod][N] (sfg_ctx_load_rotkey's, normal form: the words are kept as they are) from b = agg [beta][nmod][N], a = crp [beta][nmod][N]
static int kg_install_key(sfg_ctx *ctx, u64 g, const u64 *b, const u64 *a) {
    const int N = SFG_N; const size_t row = (size_t)ctx->nmod * N * 8, words = (size_t)ctx->beta * 2 * ctx->nmod * N;
    RotKey rk;
    DevMem key_new, index_new;                                  // a new key's storage: owned here until the key is installed
    auto it = ctx->rotkeys().find(g);
    if (it != ctx->rotkeys().end()) rk = it->second;
    else {
        SFG_HIP(ctx, hipMalloc(&key_new.h, words * 8)); SFG_HIP(ctx, hipMalloc(&index_new.h, N * sizeof(uint16_t)));
        rk.key_dev = (decltype(rk.key_dev))key_new.h; rk.index_dev = (decltype(rk.index_dev))index_new.h;
    }
    for (int i = 0; i < ctx->beta; i++) {
        SFG_HIP(ctx, hipMemcpyAsync((char *)rk.key_dev + (size_t)(2 * i) * row, (const char *)b + (size_t)i * row, row, hipMemcpyDeviceToDevice, ctx->stream));
        SFG_HIP(ctx, hipMemcpyAsync((char *)rk.key_dev + (size_t)(2 * i + 1) * row, (const char *)a + (size_t)i * row, row, hipMemcpyDeviceToDevice, ctx->stream));
    }
    std::vector<uint16_t> idx(N); kg_index_table(g, idx.data());
    SFG_TRY(sfg_upload_small(ctx, rk.index_dev, idx.data(), N * sizeof(uint16_t)));
    ctx->rotkeys()[g] = rk;
    (void)key_new.release(); (void)index_new.release();
    return 0;
}
extern "C" int sfg_ctx_install_public_key_dev(sfg_ctx *ctx, const uint64_t *agg, const uint64_t *crp) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!agg || !crp) SFG_FAIL(ctx, "install_public_key: NULL polynomial");
    const size_t row = (size_t)ctx->nmod * SFG_N * 8;
    if (!ctx->sh->pk_dev) SFG_HIP(ctx, hipMalloc(&ctx->sh->pk_dev, 2 * row));
    SFG_HIP(ctx, hipMemcpyAsync(ctx->sh->pk_dev, agg, row, hipMemcpyDeviceToDevice, ctx->stream));
    SFG_HIP(ctx, hipMemcpyAsync((char *)ctx->sh->pk_dev + row, crp, row, hipMemcpyDeviceToDevice, ctx->stream));
    SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
extern "C" int sfg_ctx_install_rotkeys_dev(sfg_ctx *ctx, const uint64_t *galois_host, int nkeys, const uint64_t *agg, const uint64_t *crp) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(kg_check_galois(ctx, "install_rotkeys", galois_host, nkeys));
    if (!nkeys) return 0;
    if (!agg || !crp) SFG_FAIL(ctx, "install_rotkeys: NULL polynomial");
    const size_t per = (size_t)ctx->beta * ctx->nmod * SFG_N;
    for (int k = 0; k < nkeys; k++) SFG_TRY(kg_install_key(ctx, galois_host[k], (const u64 *)agg + k * per, (const u64 *)crp + k * per));
    SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
extern "C" int sfg_ctx_install_relinkey_dev(sfg_ctx *ctx, const uint64_t *round2agg, const uint64_t *h1agg) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!round2agg || !h1agg) SFG_FAIL(ctx, "install_relinkey: NULL polynomial");
    SFG_TRY(kg_install_key(ctx, 1, (const u64 *)round2agg, (const u64 *)h1agg));        // stored under Galois element 1, as sfg_ctx_load_relinkey stores it
    SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int sfg_crp_fill_dev(sfg_ctx *ctx, const uint8_t *key32, uint64_t first_row, size_t nrows, const int *mod_idx_host, uint64_t *out) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!key32 || (nrows && (!mod_idx_host || !out))) SFG_FAIL(ctx, "crp_fill: NULL key, modulus indices or output");
    if (first_row > ~0ULL - nrows) SFG_FAIL(ctx, "crp_fill: row numbers beyond 2^64");
    if (nrows > 0x7FFFFFFFu) SFG_FAIL(ctx, "crp_fill: more than 2^31 - 1 rows in one call");        // (256 TiB of output: the plan counts in int)
    for (size_t r = 0; r < nrows; r++) if (mod_idx_host[r] < 0 || mod_idx_host[r] >= ctx->nmod) SFG_FAIL(ctx, "crp_fill: modulus index %d of row %zu out of range", mod_idx_host[r], r);
    if (!nrows) return 0;
    ApiScope scope(ctx);
    void *mp = nullptr;
    SFG_TRY(sfg_scratch(ctx, "keygen.crp_mod", nrows * sizeof(int), &mp));
    SFG_TRY(sfg_upload_small(ctx, mp, mod_idx_host, nrows * sizeof(int)));
    CrpKey key;                                     // passed by value: the context keeps no copy of the seed
    for (int i = 0; i < 8; i++) key.k[i] = (uint32_t)key32[4 * i] | (uint32_t)key32[4 * i + 1] << 8 | (uint32_t)key32[4 * i + 2] << 16 | (uint32_t)key32[4 * i + 3] << 24;
    PhaseTimer timer(ctx, "crp_fill");
    const BatchPlan plan = grid_rows_plan((int)nrows);  // (the grid's second dimension)
    for (int c = 0; c < plan.nchunks; c++) {
        const size_t r0 = (size_t)plan.first(c), nr = (size_t)plan.count(c, (int)nrows);
        hipLaunchKernelGGL(k_crp_fill, dim3(SFG_N / 256, (unsigned)nr), dim3(256), 0, ctx->stream, key, (u64)first_row + r0, (const int *)mp + r0, ctx->modc, (u64 *)out + r0 * SFG_N);
        SFG_HIP(ctx, hipGetLastError());
    }
    timer.stop(1, (double)nrows * SFG_N * 8);
    return 0;
}
