// gring_io.hip - the general ring's way in and out on the device: the encoder (real slot vectors -> plaintext rows), public and secret key, the keyed sampler at any
// N, public-key encryption (explicit and sampled), the local halves of the collective decryption, secret-key decryption and the decoder (plaintext rows -> slot
// values).  The twins of encode.hip, encrypt.hip and decrypt.hip (DESIGN.md sections 9 and 10) for every ring sfg_ring_create accepts: the encryption in the ring's
// integer arithmetic, the two embeddings in double-double through one two-launch transform over LDS tiles (further down).  Per-element arithmetic, the sampler's map
// and every derived bound: gring_io_arith.hpp.  Workspace and chunks: gring_io_plan.hpp.  DESIGN.md section 14.
//
// The core, per ciphertext at level l (nl = l + 1 moduli of Q, np of P), from a ternary u and two small e0, e1:
//   1. k_gri_lift    the samples (drawn from the stream in this kernel, or the caller's) lifted modulo every target: rows U (u) and T (e0, e1)
//   2. the ring's forward transform of U and T (gring.hip)
//   3. k_gri_mac     t_i = pk_i (.) NTT(u) + NTT(e_i)                      (skipped with U when u drops out: the collective key switch's zero public key)
//   4. ModDown_P of t_i as the key switch does it: inverse transform of the P rows, the float-corrected extension P -> Q (gr_extend on the ring's own table), its
//      forward transform
//   5. k_gri_finish  c_i = (t_i - ext) P^-1; then + plaintext on c_0 | + the ciphertext already there | + sk (.) c_1 on polynomial 0 (the share)
// All launches go on the ring's stream.  Every word written is canonical.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gring_dev.hpp"
#include "gring_io_arith.hpp"
#include "gring_io_plan.hpp"
#include "ddfft.hpp"          // host only: the double-double Taylor series the transform's tables are built with (dd_sincos_small)
#include "gring_sampler.hpp"  // gri_sample8 (shared with gring_keygen.hip) over sampler.hpp: chacha20_block, gauss_from_bits and the Gaussian table, not forked

// ---------------------------------------------------------------- sampling and lifting
struct GriSrc { const int8_t *u; const int32_t *e0, *e1; const unsigned *key; u64 index0; };     // key != nullptr: the sampler; else the caller's polynomials [nct][N] (u nullable: zero)

// grid (N / 8 / 256, 1, chunk).  U: UQ [chunk][nl][N], UP [chunk][np][N] (both null when u drops out); T: TQ [chunk][npoly][nl][N], TP [chunk][npoly][np][N].
// j = 512 (8 g + k) + t < 4096 (g + 1) <= N since g < N / 4096 by the grid.
template <bool SAMPLE>
__global__ __launch_bounds__(GR_T) void k_gri_lift(GriSrc src, u64 *UQ, u64 *UP, u64 *TQ, u64 *TP, const GrMod *modc, int npoly, int nl, int np, int nq, int N) {
    const int id = blockIdx.x * GR_T + threadIdx.x, t = id & (gio::kSampT - 1), g = id >> 9;
    const size_t ct = blockIdx.z;
    const bool has_u = UQ != nullptr;
    int su[8], s0[8], s1[8];
#pragma unroll
    for (int k = 0; k < 8; k++) su[k] = s0[k] = s1[k] = 0;
    if (SAMPLE) {
        unsigned key[8];
#pragma unroll
        for (int i = 0; i < 8; i++) key[i] = src.key[i];
        gri_sample8(key, src.index0 + ct, t, g, has_u, npoly, su, s0, s1);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const size_t j = ct * N + (size_t)gio::kSampT * (8 * g + k) + t;
            if (has_u && src.u) su[k] = src.u[j];
            s0[k] = src.e0[j];
            if (npoly == 2) s1[k] = src.e1[j];
        }
    }
    for (int tg = 0; tg < nl + np; tg++) {
        const bool isq = tg < nl;
        const u64 q = modc[isq ? tg : nq + tg - nl].q;
        u64 *U = !has_u ? nullptr : isq ? UQ + (ct * nl + tg) * N : UP + (ct * np + (tg - nl)) * N;
        u64 *T0 = isq ? TQ + (ct * npoly * nl + tg) * N : TP + (ct * npoly * np + (tg - nl)) * N;
        u64 *T1 = T0 + (size_t)(isq ? nl : np) * N;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int j = gio::kSampT * (8 * g + k) + t;
            if (has_u) U[j] = gio::lift(su[k], q);
            T0[j] = gio::lift(s0[k], q);
            if (npoly == 2) T1[j] = gio::lift(s1[k], q);
        }
    }
}
// the samples themselves (test hook): grid (N / 8 / 256, 1, nct)
__global__ __launch_bounds__(GR_T) void k_gri_transcript(const unsigned *keyp, u64 index0, int8_t *u, int32_t *e0, int32_t *e1, int N) {
    const int id = blockIdx.x * GR_T + threadIdx.x, t = id & (gio::kSampT - 1), g = id >> 9;
    const size_t ct = blockIdx.z;
    unsigned key[8]; int su[8], s0[8], s1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = keyp[i];
    gri_sample8(key, index0 + ct, t, g, true, 2, su, s0, s1);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const size_t j = ct * N + (size_t)gio::kSampT * (8 * g + k) + t;
        u[j] = (int8_t)su[k]; e0[j] = s0[k]; e1[j] = s1[k];
    }
}

// ---------------------------------------------------------------- element-wise kernels; x < N by the grid: N is a multiple of 256
// t_p = pk_p (.) u^ + e_p^ at every target: grid (N / 256, nl + np, chunk * npoly).  pk [2][nmod][N].
__global__ __launch_bounds__(GR_T) void k_gri_mac(const u64 *pk, const u64 *UQ, const u64 *UP, u64 *TQ, u64 *TP, const GrMod *modc, int npoly, int nl, int np, int nq, int nmod, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, tg = blockIdx.y, p = blockIdx.z % npoly; const size_t z = blockIdx.z, ct = z / npoly;
    const bool isq = tg < nl; const int mod = isq ? tg : nq + tg - nl; const GrMod mc = modc[mod];
    const u64 u = isq ? UQ[(ct * nl + tg) * N + x] : UP[(ct * np + (tg - nl)) * N + x];
    u64 *T = isq ? TQ + (z * nl + tg) * N + x : TP + (z * np + (tg - nl)) * N + x;
    *T = gr::addmod(gr::mulmod(pk[((size_t)p * nmod + mod) * N + x], u, mc.q, mc.uhi, mc.ulo), *T, mc.q);
}
// ModDown's last step and what follows it: d = (t - ext) P^-1, grid (N / 256, nl, chunk * npoly)
//   GRI_OUT    out0 [chunk][2][nl][N] = d (+ aux = plaintext rows [chunk][nl][N] on polynomial 0 when aux != nullptr)
//   GRI_ADD    out0 [chunk][2][nl][N] += d
//   GRI_SHARE  out0 [chunk][nl][N] = d_0 + sk (.) c1 with c1 read from aux = ciphertexts [chunk][2][nl][N];  out1 [chunk][nl][N] = d_1 (npoly == 2 only)
enum { GRI_OUT, GRI_ADD, GRI_SHARE };
template <int MODE>
__global__ __launch_bounds__(GR_T) void k_gri_finish(const u64 *TQ, const u64 *ext, const u64 *pinv, const u64 *aux, const u64 *sk, u64 *out0, u64 *out1, const GrMod *modc, int npoly, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, t = blockIdx.y, p = blockIdx.z % npoly; const size_t z = blockIdx.z, ct = z / npoly;
    const GrMod mc = modc[t];
    const size_t w = (z * nl + t) * N + x, row = (ct * nl + t) * N + x, o = ((ct * 2 + p) * nl + t) * N + x;
    u64 d = gr::shoup(gr::submod(TQ[w], ext[w], mc.q), pinv[2 * t], pinv[2 * t + 1], mc.q);
    if (MODE == GRI_OUT) { if (p == 0 && aux) d = gr::addmod(d, aux[row], mc.q); out0[o] = d; }
    else if (MODE == GRI_ADD) out0[o] = gr::addmod(out0[o], d, mc.q);
    else if (p == 0) out0[row] = gr::addmod(d, gr::mulmod(sk[(size_t)t * N + x], aux[((ct * 2 + 1) * nl + t) * N + x], mc.q, mc.uhi, mc.ulo), mc.q);
    else out1[row] = d;
}
// pt = c0 + h0agg: grid (N / 256, nl, chunk)
__global__ __launch_bounds__(GR_T) void k_gri_add_c0(const u64 *ct, const u64 *h, u64 *pt, const GrMod *modc, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, t = blockIdx.y; const size_t c = blockIdx.z, row = (c * nl + t) * N + x;
    pt[row] = gr::addmod(ct[(c * 2 * nl + t) * N + x], h[row], modc[t].q);
}

// ---------------------------------------------------------------- host side
// pt [nb][nl][N] = c0 + h for nb <= kGrLaunchCap ciphertexts: one launch (the collective decryption's finish, the front of the collective bootstrap's)
int gri_add_c0(sfg_ring *r, const u64 *ct, const u64 *h, u64 *pt, int nb, int level) {
    const int nl = level + 1, N = r->N;
    hipLaunchKernelGGL(k_gri_add_c0, dim3(N / GR_T, nl, (unsigned)nb), dim3(GR_T), 0, r->stream, ct, h, pt, r->modc, nl, N);
    GR_HIP(r, hipGetLastError());
    return 0;
}
// the workspace of a call, reserved before the call spends an encryption index: a failed allocation leaves the counter where it was
static int gri_reserve(sfg_ring *r, int npoly, int nct, int level, bool with_u, GriPlan &plan) {
    plan = gri_plan(nct, level + 1, r->np, npoly, with_u, (size_t)r->N, r->io.ws_budget);
    return gr_reserve(r, r->io.ws, plan.reserve());
}
// the core for nct ciphertexts, in the chunks of the plan gri_reserve made.  pk null: u drops out.  mode GRI_OUT (aux = plaintext rows or null), GRI_ADD, GRI_SHARE (aux = ciphertexts)
static int gri_core(sfg_ring *r, const GriPlan &plan, const GriSrc &src0, const u64 *pk, int npoly, int nct, int level, int mode, const u64 *aux, u64 *out0, u64 *out1) {
    const int nl = level + 1, np = r->np, N = r->N;
    const bool with_u = pk != nullptr;
    const GriCoreLayout lay = gri_core_layout(nl, np, npoly, with_u, (size_t)N, (size_t)plan.chunk);
    u64 *ws = (u64 *)r->io.ws.p;
    u64 *UQ = with_u ? ws + lay.UQ : nullptr, *UP = with_u ? ws + lay.UP : nullptr;
    u64 *TQ = ws + lay.TQ, *TP = ws + lay.TP, *Y2 = ws + lay.Y2, *ext = ws + lay.ext;
    uint32_t *V2 = (uint32_t *)(ws + lay.V2);
    const unsigned gx = N / GR_T, gs = N / 8 / GR_T;
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct); const size_t n = nb, z = n * npoly;
        GriSrc src = src0;
        if (src.key) src.index0 += (u64)c0;
        else { if (src.u) src.u += (size_t)c0 * N; src.e0 += (size_t)c0 * N; if (src.e1) src.e1 += (size_t)c0 * N; }
        if (src.key) hipLaunchKernelGGL(k_gri_lift<true>, dim3(gs, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, src, UQ, UP, TQ, TP, r->modc, npoly, nl, np, r->nq, N);
        else hipLaunchKernelGGL(k_gri_lift<false>, dim3(gs, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, src, UQ, UP, TQ, TP, r->modc, npoly, nl, np, r->nq, N);
        GR_HIP(r, hipGetLastError());
        if (with_u) {
            GR_TRY(gr_transform(r, UQ, n * nl, gr_map(nl, nl, 0, 0), false));
            GR_TRY(gr_transform(r, UP, n * np, gr_map(np, np, r->nq, 0), false));
        }
        GR_TRY(gr_transform(r, TQ, z * nl, gr_map(nl, nl, 0, 0), false));
        GR_TRY(gr_transform(r, TP, z * np, gr_map(np, np, r->nq, 0), false));
        if (with_u) hipLaunchKernelGGL(k_gri_mac, dim3(gx, nl + np, (unsigned)z), dim3(GR_T), 0, r->stream, pk, (const u64 *)UQ, (const u64 *)UP, TQ, TP, r->modc, npoly, nl, np, r->nq, r->nmod, N);
        GR_TRY(gr_transform(r, TP, z * np, gr_map(np, np, r->nq, 0), true));
        GR_TRY(gr_extend(r, r->down.e, TP, Y2, V2, ext, nl, z));
        GR_TRY(gr_transform(r, ext, z * nl, gr_map(nl, nl, 0, 0), false));
        const dim3 gf(gx, nl, (unsigned)z);
        if (mode == GRI_OUT) hipLaunchKernelGGL(k_gri_finish<GRI_OUT>, gf, dim3(GR_T), 0, r->stream, (const u64 *)TQ, (const u64 *)ext, (const u64 *)r->pinv, aux ? aux + (size_t)c0 * nl * N : nullptr,
                                                (const u64 *)nullptr, out0 + (size_t)c0 * 2 * nl * N, (u64 *)nullptr, r->modc, npoly, nl, N);
        else if (mode == GRI_ADD) hipLaunchKernelGGL(k_gri_finish<GRI_ADD>, gf, dim3(GR_T), 0, r->stream, (const u64 *)TQ, (const u64 *)ext, (const u64 *)r->pinv, (const u64 *)nullptr,
                                                     (const u64 *)nullptr, out0 + (size_t)c0 * 2 * nl * N, (u64 *)nullptr, r->modc, npoly, nl, N);
        else hipLaunchKernelGGL(k_gri_finish<GRI_SHARE>, gf, dim3(GR_T), 0, r->stream, (const u64 *)TQ, (const u64 *)ext, (const u64 *)r->pinv, aux + (size_t)c0 * 2 * nl * N,
                                r->io.sk, out0 + (size_t)c0 * nl * N, out1 ? out1 + (size_t)c0 * nl * N : nullptr, r->modc, npoly, nl, N);
        GR_HIP(r, hipGetLastError());
    }
    return 0;
}

// takes nct consecutive encryption indices from the ring's one counter
int gri_take_indices(sfg_ring *r, const char *what, int nct, u64 *first) {
    GrIo &io = r->io;
    if (!io.enc_seeded) GR_FAIL(r, "%s: the encryptor has no key (sfg_ring_seed_encryptor); there is no default", what);
    unsigned long long cur = __atomic_load_n(&io.enc_next, __ATOMIC_ACQUIRE);
    for (;;) {
        if (cur > ~0ULL - (u64)nct) GR_FAIL(r, "%s: the encryption index space of this key is used up (re-seed)", what);
        if (__atomic_compare_exchange_n(&io.enc_next, &cur, cur + (u64)nct, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) break;
    }
    *first = cur;
    return 0;
}
#define GRI_ENTRY(what)                                                          \
    GR_HIP(r, hipSetDevice(r->device));                                         \
    GR_TRY(gr_check_level(r, what, nct, level));                                \
    if (nct == 0) return 0;

// ---------------------------------------------------------------- C-ABI: keys and sampler
extern "C" int sfg_ring_load_public_key(sfg_ring *r, const uint64_t *pk_host, int mont) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!pk_host) GR_FAIL(r, "sfg_ring_load_public_key: null key");
    const size_t rows = (size_t)2 * r->nmod, words = rows * r->N;
    GR_HIP(r, hipStreamSynchronize(r->stream));                                // launches that still read the previous key
    if (!r->io.pk) GR_HIP(r, r->io.pk.alloc(words * 8));
    GR_HIP(r, hipMemcpyAsync(r->io.pk, pk_host, words * 8, hipMemcpyHostToDevice, r->stream));
    if (mont) GR_TRY(gr_rows_from_mont(r, r->io.pk, rows));
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}
extern "C" int sfg_ring_has_public_key(const sfg_ring *r) { return r->io.pk ? 1 : 0; }
extern "C" int sfg_ring_load_secret_key(sfg_ring *r, const uint64_t *sk_host, int mont) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!sk_host) GR_FAIL(r, "sfg_ring_load_secret_key: null key");
    const size_t rows = (size_t)r->nq, words = rows * r->N;
    GR_HIP(r, hipStreamSynchronize(r->stream));
    if (!r->io.sk) GR_HIP(r, r->io.sk.alloc(words * 8));
    GR_HIP(r, hipMemcpyAsync(r->io.sk, sk_host, words * 8, hipMemcpyHostToDevice, r->stream));
    if (mont) GR_TRY(gr_rows_from_mont(r, r->io.sk, rows));                    // rows 0..nq-1 of one group of nmod: row m is modulus m
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}
extern "C" int sfg_ring_seed_encryptor(sfg_ring *r, const uint8_t *key32) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!key32) GR_FAIL(r, "sfg_ring_seed_encryptor: null key");
    GrIo &io = r->io;
    GR_HIP(r, hipStreamSynchronize(r->stream));                                // launches that still read the previous key
    if (!io.enc_key_dev) GR_HIP(r, io.enc_key_dev.alloc(32));
    for (int i = 0; i < 8; i++) io.enc_key[i] = (uint32_t)key32[4 * i] | (uint32_t)key32[4 * i + 1] << 8 | (uint32_t)key32[4 * i + 2] << 16 | (uint32_t)key32[4 * i + 3] << 24;
    GR_HIP(r, hipMemcpy(io.enc_key_dev, io.enc_key, 32, hipMemcpyHostToDevice));
    __atomic_store_n(&io.enc_next, 0ULL, __ATOMIC_RELEASE);
    io.enc_seeded = true;
    return 0;
}
extern "C" int sfg_ring_encryptor_next_index(sfg_ring *r, uint64_t *next) {
    if (!next) GR_FAIL(r, "sfg_ring_encryptor_next_index: null result pointer");
    *next = __atomic_load_n(&r->io.enc_next, __ATOMIC_ACQUIRE);
    return 0;
}

// ---------------------------------------------------------------- C-ABI: encryption
extern "C" int sfg_ring_encrypt_explicit_dev(sfg_ring *r, const uint64_t *pt, int nct, int level, const int8_t *u, const int32_t *e0, const int32_t *e1, uint64_t *out) {
    GRI_ENTRY("sfg_ring_encrypt_explicit_dev")
    if (!r->io.pk) GR_FAIL(r, "sfg_ring_encrypt_explicit_dev: no public key loaded (sfg_ring_load_public_key)");
    if (!u || !e0 || !e1 || !out) GR_FAIL(r, "sfg_ring_encrypt_explicit_dev: null polynomial or output");
    GriSrc src{u, e0, e1, nullptr, 0};
    GriPlan plan; GR_TRY(gri_reserve(r, 2, nct, level, true, plan));
    return gri_core(r, plan, src, r->io.pk, 2, nct, level, GRI_OUT, (const u64 *)pt, (u64 *)out, nullptr);
}
extern "C" int sfg_ring_ct_add_fresh_zero_dev(sfg_ring *r, uint64_t *ct, int nct, int level) {
    GRI_ENTRY("sfg_ring_ct_add_fresh_zero_dev")
    if (!r->io.pk) GR_FAIL(r, "sfg_ring_ct_add_fresh_zero_dev: no public key loaded (sfg_ring_load_public_key)");
    if (!ct) GR_FAIL(r, "sfg_ring_ct_add_fresh_zero_dev: null ciphertexts");
    GriPlan plan; GR_TRY(gri_reserve(r, 2, nct, level, true, plan));          // before an index is taken: a failed allocation leaves the counter where it was
    u64 first; GR_TRY(gri_take_indices(r, "sfg_ring_ct_add_fresh_zero_dev", nct, &first));
    GriSrc src{nullptr, nullptr, nullptr, r->io.enc_key_dev, first};
    return gri_core(r, plan, src, r->io.pk, 2, nct, level, GRI_ADD, nullptr, (u64 *)ct, nullptr);
}
extern "C" int sfg_ring_encrypt_transcript_for_test(sfg_ring *r, uint64_t first_index, int nct, int8_t *u, int32_t *e0, int32_t *e1) {
    if (!r->test_hooks) GR_FAIL(r, "sfg_ring_encrypt_transcript_for_test: test hook, enabled only in a process that set the test switch before creating the ring");
    GR_HIP(r, hipSetDevice(r->device));
    if (!r->io.enc_seeded) GR_FAIL(r, "sfg_ring_encrypt_transcript_for_test: the encryptor has no key (sfg_ring_seed_encryptor); there is no default");
    if (nct < 0) GR_FAIL(r, "sfg_ring_encrypt_transcript_for_test: negative ciphertext count %d", nct);
    if (nct == 0) return 0;
    if (!u || !e0 || !e1) GR_FAIL(r, "sfg_ring_encrypt_transcript_for_test: null output");
    if (first_index > ~0ULL - (u64)nct) GR_FAIL(r, "sfg_ring_encrypt_transcript_for_test: indices beyond 2^64");
    gr_split((size_t)nct, kGrLaunchCap, [&](size_t c0, size_t nb) {
        hipLaunchKernelGGL(k_gri_transcript, dim3(r->N / 8 / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, (const unsigned *)r->io.enc_key_dev, (u64)first_index + c0,
                           u + c0 * r->N, e0 + c0 * r->N, e1 + c0 * r->N, r->N);
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- C-ABI: collective decryption, local halves
extern "C" int sfg_ring_pcks_gen_share_dev(sfg_ring *r, const uint64_t *ct, int nct, int level, const int32_t *e0, const int32_t *e1, uint64_t *h0, uint64_t *h1) {
    GRI_ENTRY("sfg_ring_pcks_gen_share_dev")
    if (!r->io.sk) GR_FAIL(r, "sfg_ring_pcks_gen_share_dev: no secret-key shard loaded (sfg_ring_load_secret_key)");
    if (!ct || !e0 || !h0 || (h1 && !e1)) GR_FAIL(r, "sfg_ring_pcks_gen_share_dev: null ciphertexts, errors or output");
    GriSrc src{nullptr, e0, h1 ? e1 : nullptr, nullptr, 0};
    GriPlan plan; GR_TRY(gri_reserve(r, h1 ? 2 : 1, nct, level, false, plan));
    return gri_core(r, plan, src, nullptr, h1 ? 2 : 1, nct, level, GRI_SHARE, (const u64 *)ct, (u64 *)h0, (u64 *)h1);
}
extern "C" int sfg_ring_pcks_finish_dev(sfg_ring *r, const uint64_t *ct, int nct, int level, const uint64_t *h0agg, uint64_t *pt) {
    GRI_ENTRY("sfg_ring_pcks_finish_dev")
    if (!ct || !h0agg || !pt) GR_FAIL(r, "sfg_ring_pcks_finish_dev: null ciphertexts, shares or output");
    const int nl = level + 1, N = r->N;
    return gr_split((size_t)nct, kGrLaunchCap, [&](size_t c0, size_t nb) {
        return gri_add_c0(r, (const u64 *)ct + c0 * 2 * nl * N, (const u64 *)h0agg + c0 * nl * N, (u64 *)pt + c0 * nl * N, (int)nb, level);
    });
}

// ---------------------------------------------------------------- the decoder's coefficients (sfg_ring_decode_coeffs)
// INTT of the rows; mixed-radix digits, one launch per digit, the digits taking the place of the residues row by row (rows of digits in the workspace, no per-thread
// array: level + 1 may be 47); then one thread per coefficient walks its column of digits three times (gio::decode_digits).
// tables of a level (GriDecTab, gring_dev.hpp): qmod [nl][nl] (q_j mod q_i, j < i), winv [nl][2] (W_i^-1 mod q_i and its Shoup quotient), half [nl] (the digits of floor(Q / 2))
// digit i of every coefficient: grid (N / 256, 1, chunk); X [chunk][nl][N], rows 0 .. i-1 digits already, row i the residue
__global__ __launch_bounds__(GR_T) void k_gri_garner(u64 *X, GriDecTab t, const GrMod *modc, int i, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x; u64 *col = X + (size_t)blockIdx.z * nl * N + x;
    const GrMod mc = modc[i];
    u64 acc = 0;
    for (int j = i - 1; j >= 0; j--) acc = gio::garner_acc(acc, col[(size_t)j * N], t.qmod[i * nl + j], mc.q, mc.uhi, mc.ulo);
    col[(size_t)i * N] = gio::garner_digit(col[(size_t)i * N], acc, t.winv[2 * i], t.winv[2 * i + 1], mc.q);
}
// grid (N / 256, 1, chunk): out [chunk][N]
__global__ __launch_bounds__(GR_T) void k_gri_decode_fin(u64 *X, double *out, GriDecTab t, const GrMod *modc, int nl, int N, double scale) {
    const int x = blockIdx.x * GR_T + threadIdx.x; u64 *col = X + (size_t)blockIdx.z * nl * N + x;
    out[(size_t)blockIdx.z * N + x] = gio::decode_digits(nl, [&](int i) { return col[(size_t)i * N]; }, [&](int i, u64 v) { col[(size_t)i * N] = v; },
                                                         [&](int i) { return modc[i].q; }, [&](int i) { return t.half[i]; }, scale);
}

int gri_dec_tab(sfg_ring *r, int level, GriDecTab *out) {
    const int nl = level + 1;
    auto it = r->io.dec_tabs.find(level);
    if (it == r->io.dec_tabs.end()) {
        std::vector<u64> h((size_t)nl * nl + 3 * nl, 0);
        u64 *qmod = h.data(), *winv = qmod + (size_t)nl * nl, *half = winv + 2 * nl;
        for (int i = 0; i < nl; i++) {
            const u64 qi = r->q[i]; u64 W = 1 % qi;
            for (int j = 0; j < i; j++) { qmod[i * nl + j] = r->q[j] % qi; W = hm_mul(W, r->q[j] % qi, qi); }
            winv[2 * i] = hm_inv(W, qi); winv[2 * i + 1] = hm_shoup(winv[2 * i], qi);
        }
        // floor(Q / 2) = (Q - 1) / 2 and Q - 1 has the digits q_i - 1: halve from the top, the remainder of digit i + 1 entering digit i as q_i
        u64 rem = 0;
        for (int i = nl - 1; i >= 0; i--) { const u128 cur = (u128)rem * r->q[i] + (r->q[i] - 1); half[i] = (u64)(cur >> 1); rem = (u64)(cur & 1); }
        GrBuf<u64> d; GR_TRY(gr_table(r, d, h.data(), h.size() * 8));
        it = r->io.dec_tabs.emplace(level, std::move(d)).first;
    }
    const u64 *d = it->second;
    out->qmod = d; out->winv = d + (size_t)nl * nl; out->half = out->winv + 2 * nl;
    return 0;
}
// the checks every decoding entry point shares
static int gri_decode_checks(sfg_ring *r, const char *what, const void *src, const void *out, size_t stride, int level, double scale) {
    if (!src || !out) GR_FAIL(r, "%s: null plaintexts or output", what);
    if (!(scale >= 1.0) || !std::isfinite(scale)) GR_FAIL(r, "%s: scale %g must be finite and at least 1", what, scale);
    const size_t rowsw = (size_t)(level + 1) * r->N;
    if (stride < rowsw) GR_FAIL(r, "%s: pt_stride %zu is below the (level + 1) * N = %zu words of a plaintext", what, stride, rowsw);
    return 0;
}
// NTT-domain residue rows X [nb][nl][N] -> their mixed-radix digits in place (nl == 1: the inverse transform alone, no Garner launch)
int gri_digits_inplace(sfg_ring *r, u64 *X, int nb, int level, const GriDecTab &tab) {
    const int nl = level + 1, N = r->N;
    GR_TRY(gr_transform(r, X, (size_t)nb * nl, gr_map(nl, nl, 0, 0), true));
    for (int i = 1; i < nl; i++) hipLaunchKernelGGL(k_gri_garner, dim3(N / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, X, tab, r->modc, i, nl, N);
    GR_HIP(r, hipGetLastError());
    return 0;
}
// residues of nb plaintexts (stride words apart) -> their mixed-radix digits in X [nb][nl][N]
static int gri_digits(sfg_ring *r, const u64 *src, size_t stride, int nb, int level, u64 *X, const GriDecTab &tab) {
    const int nl = level + 1, N = r->N; const size_t rowsw = (size_t)nl * N;
    GR_HIP(r, hipMemcpy2DAsync(X, rowsw * 8, src, stride * 8, rowsw * 8, nb, hipMemcpyDeviceToDevice, r->stream));
    return gri_digits_inplace(r, X, nb, level, tab);
}
extern "C" int sfg_ring_decode_coeffs(sfg_ring *r, const uint64_t *pt, size_t pt_stride, int nct, int level, double scale, double *coeffs_host) {
    GRI_ENTRY("sfg_ring_decode_coeffs")
    GR_TRY(gri_decode_checks(r, "sfg_ring_decode_coeffs", pt, coeffs_host, pt_stride, level, scale));
    const int nl = level + 1, N = r->N;
    GriDecTab tab; GR_TRY(gri_dec_tab(r, level, &tab));
    const GriPlan plan = gri_decode_plan(nct, nl, (size_t)N, r->io.ws_budget);
    GR_TRY(gr_reserve(r, r->io.ws, plan.reserve()));
    const GriDecodeLayout lay = gri_decode_layout(nl, (size_t)N, (size_t)plan.chunk);
    u64 *X = (u64 *)r->io.ws.p + lay.X; double *out = (double *)r->io.ws.p + lay.out;
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct);
        GR_TRY(gri_digits(r, (const u64 *)pt + (size_t)c0 * pt_stride, pt_stride, nb, level, X, tab));
        hipLaunchKernelGGL(k_gri_decode_fin, dim3(N / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, X, out, tab, r->modc, nl, N, scale);
        GR_HIP(r, hipGetLastError());
        GR_HIP(r, hipMemcpyAsync(coeffs_host + (size_t)c0 * N, out, (size_t)nb * N * 8, hipMemcpyDeviceToHost, r->stream));
        GR_HIP(r, hipStreamSynchronize(r->stream));
    }
    return 0;
}

// ---------------------------------------------------------------- the double-double transform between slots and coefficients
// The forward DFT of n = N / 2 complex points (kernel exp(-2 pi i m c / n)), natural order in, bit-reversed out, decimation in frequency, for every logN through one
// code path: like the ring's integer transform (gring_plan.hpp) the log2 n = a + b radix-2 stages are split over two launches, the `a` stages of distance >= 2^b on a
// tile of all 2^a rows of 1024 / 2^a adjacent columns, the `b` stages of distance < 2^b on 1024 contiguous points.  A point is 32 bytes ({re.hi, re.lo, im.hi, im.lo});
// a tile of 1024 points is 32 KiB of LDS in four planes of doubles (consecutive lanes, consecutive banks); 256 threads, two butterflies a thread and stage, all in
// registers.  a = floor(log2 n / 2): 11 = 5 + 6 ... 15 = 7 + 8, so a row segment of the columns pass is at least 8 points = 256 contiguous bytes.
// The encoder feeds it u_m = v_t at m = (5^t - 1) / 4 and reads w_c = zeta^-c X_c / n at the bit-reversed place; the decoder feeds conj(w_c) zeta^-c and reads the
// conjugate at the place of m_t: bit reversal, twist and slot permutation are addressing, and one transform serves both directions.
// Index bounds: a tile index is < 1024 by construction; the columns pass reads (r << b) + c0 + c with r < 2^a, c0 + c < 2^b; twiddle indices are < n / 2 (see the loops).
constexpr int GDD_TILE = 1024;
__device__ __forceinline__ gio::cdd gdd_of(double4 v) { gio::cdd r; r.re.hi = v.x; r.re.lo = v.y; r.im.hi = v.z; r.im.lo = v.w; return r; }
__device__ __forceinline__ double4 gdd_to(gio::cdd v) { return make_double4(v.re.hi, v.re.lo, v.im.hi, v.im.lo); }
__device__ __forceinline__ gio::cdd gdd_lds(const double (*t)[GDD_TILE], int i) { gio::cdd r; r.re.hi = t[0][i]; r.re.lo = t[1][i]; r.im.hi = t[2][i]; r.im.lo = t[3][i]; return r; }
__device__ __forceinline__ void gdd_sts(double (*t)[GDD_TILE], int i, gio::cdd v) { t[0][i] = v.re.hi; t[1][i] = v.re.lo; t[2][i] = v.im.hi; t[3][i] = v.im.lo; }
// grid (n / 1024, nvec)
__global__ __launch_bounds__(GR_T) void k_gdd_cols(double4 *A, const double4 *W, int logn, int a, int b) {
    __shared__ double tile[4][GDD_TILE];
    double4 *base = A + ((size_t)blockIdx.y << logn);
    const int lg = 10 - a, G = 1 << lg, c0 = blockIdx.x * G;
    for (int e = threadIdx.x; e < GDD_TILE; e += GR_T) gdd_sts(tile, e, gdd_of(base[((size_t)(e >> lg) << b) + c0 + (e & (G - 1))]));
    __syncthreads();
    for (int s = 0; s < a; s++) {
        const int lh = a - 1 - s, h = 1 << lh;
        for (int k = threadIdx.x; k < GDD_TILE / 2; k += GR_T) {
            const int c = k & (G - 1), p = k >> lg, i = p >> lh, r = (i << (lh + 1)) + (p & (h - 1));
            const int tw = (((r & (h - 1)) << b) + c0 + c) << (a - 1 - lh);          // < 2^lh 2^b 2^(a-1-lh) = n / 2
            gio::cdd X = gdd_lds(tile, (r << lg) + c), Y = gdd_lds(tile, ((r + h) << lg) + c);
            gio::bfly_dif(X, Y, gdd_of(W[tw]));
            gdd_sts(tile, (r << lg) + c, X); gdd_sts(tile, ((r + h) << lg) + c, Y);
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < GDD_TILE; e += GR_T) base[((size_t)(e >> lg) << b) + c0 + (e & (G - 1))] = gdd_to(gdd_lds(tile, e));
}
__global__ __launch_bounds__(GR_T) void k_gdd_contig(double4 *A, const double4 *W, int logn, int a, int b) {
    __shared__ double tile[4][GDD_TILE];
    double4 *base = A + ((size_t)blockIdx.y << logn) + (size_t)blockIdx.x * GDD_TILE;
    for (int e = threadIdx.x; e < GDD_TILE; e += GR_T) gdd_sts(tile, e, gdd_of(base[e]));
    __syncthreads();
    for (int s = 0; s < b; s++) {
        const int lt = b - 1 - s, t = 1 << lt;
        for (int k = threadIdx.x; k < GDD_TILE / 2; k += GR_T) {
            const int ch = k >> (b - 1), bb = k & ((1 << (b - 1)) - 1), i = bb >> lt, j = (ch << b) + (i << (lt + 1)) + (bb & (t - 1));
            const int tw = (bb & (t - 1)) << (logn - 1 - lt);                        // < 2^lt 2^(logn-1-lt) = n / 2
            gio::cdd X = gdd_lds(tile, j), Y = gdd_lds(tile, j + t);
            gio::bfly_dif(X, Y, gdd_of(W[tw]));
            gdd_sts(tile, j, X); gdd_sts(tile, j + t, Y);
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < GDD_TILE; e += GR_T) base[e] = gdd_to(gdd_lds(tile, e));
}
// encoder in: A[vec][m_t] = v_t.  grid (n / 256, 1, nvec)
__global__ __launch_bounds__(GR_T) void k_gdd_enc_load(const double *vals, double4 *A, const uint32_t *slot_m, int n) {
    const int t = blockIdx.x * GR_T + threadIdx.x; const size_t o = (size_t)blockIdx.z * n;
    A[o + slot_m[t]] = make_double4(vals[o + t], 0.0, 0.0, 0.0);
}
// encoder out: y = (scale / n) zeta^-c X_c; p_c = round(Re y), p_(c+n) = round(Im y), half away from zero, with the band test; p reduced modulo every q_i into
// R [nvec][nl][N] (coefficient domain).  flags[0] counts unproven coefficients, flags[1] those outside the domain.  grid (n / 256, 1, nvec)
// ties (null for the real-slot-vector entry points: a coefficient in the band is refused there): the products' list of a batch (GriTies, gring_dev.hpp).  A coefficient
// in the band is appended as (vector, coefficient index) for the resolver to re-derive and does not count as unproven - unless the list is full.
__device__ __forceinline__ void gdd_flag(unsigned *flags, unsigned *ties, unsigned vec, unsigned coeff) {
    if (ties) {
        const unsigned k = atomicAdd(&ties[GriTies::kCount], 1u);
        if (k < (unsigned)GriTies::kCap) { ties[GriTies::kEntries + 2 * k] = vec; ties[GriTies::kEntries + 2 * k + 1] = coeff; return; }
    }
    atomicAdd(&flags[0], 1u);
}
__global__ __launch_bounds__(GR_T) void k_gdd_enc_post(const double4 *A, const double4 *Z, u64 *R, unsigned *flags, unsigned *ties, const double *band, const GrMod *modc, double mul, int logn,
                                                       int nl) {
    const int c = blockIdx.x * GR_T + threadIdx.x, n = 1 << logn, N = 2 * n; const size_t vec = blockIdx.z;
    const gio::cdd y = gio::cdd_mul(gdd_of(A[vec * n + (__brev((unsigned)c) >> (32 - logn))]), gdd_of(Z[c]));
    long long pr, pi;
    const int sr = gio::round_half_away(gio::dd_mul_d(y.re, mul), band[vec], pr), si = gio::round_half_away(gio::dd_mul_d(y.im, mul), band[vec], pi);
    if (sr == 1) gdd_flag(flags, ties, (unsigned)vec, (unsigned)c); if (si == 1) gdd_flag(flags, ties, (unsigned)vec, (unsigned)(c + n));
    if (sr == 2) atomicAdd(&flags[1], 1u); if (si == 2) atomicAdd(&flags[1], 1u);
    for (int i = 0; i < nl; i++) {
        const GrMod mc = modc[i]; u64 *row = R + (vec * nl + i) * N;
        row[c] = gio::reduce_i62(pr, mc.q, mc.uhi, mc.ulo); row[c + n] = gio::reduce_i62(pi, mc.q, mc.uhi, mc.ulo);
    }
}
// decoder: the signed quotient of every coefficient as a pair.  grid (N / 256, 1, chunk); Wd [chunk][N] {hi, lo}
__global__ __launch_bounds__(GR_T) void k_gri_decode_fin_dd(u64 *X, double2 *Wd, GriDecTab t, const GrMod *modc, int nl, int N, double scale) {
    const int x = blockIdx.x * GR_T + threadIdx.x; u64 *col = X + (size_t)blockIdx.z * nl * N + x;
    const gio::dd r = gio::decode_digits_dd(nl, [&](int i) { return col[(size_t)i * N]; }, [&](int i, u64 v) { col[(size_t)i * N] = v; },
                                            [&](int i) { return modc[i].q; }, [&](int i) { return t.half[i]; }, scale);
    Wd[(size_t)blockIdx.z * N + x] = make_double2(r.hi, r.lo);
}
// decoder in: A[vec][c] = conj(w_c) zeta^-c, w_c = Wd[c] + i Wd[c + n].  grid (n / 256, 1, nvec)
__global__ __launch_bounds__(GR_T) void k_gdd_dec_load(const double2 *Wd, const double4 *Z, double4 *A, int n) {
    const int c = blockIdx.x * GR_T + threadIdx.x; const size_t vec = blockIdx.z;
    const double2 re = Wd[vec * 2 * n + c], im = Wd[vec * 2 * n + n + c];
    gio::cdd w; w.re.hi = re.x; w.re.lo = re.y; w.im.hi = -im.x; w.im.lo = -im.y;
    A[vec * n + c] = gdd_to(gio::cdd_mul(w, gdd_of(Z[c])));
}
// decoder out: v_t = conj(X at m_t), each part rounded to double once (the high part of a normalised pair is the pair rounded).  im may be null.  grid (n / 256, 1, nvec)
__global__ __launch_bounds__(GR_T) void k_gdd_dec_post(const double4 *A, const uint32_t *slot_pos, double *re, double *im, int n) {
    const int t = blockIdx.x * GR_T + threadIdx.x; const size_t o = (size_t)blockIdx.z * n;
    const double4 X = A[o + slot_pos[t]];
    re[o + t] = X.x + X.y;
    if (im) im[o + t] = -(X.z + X.w);
}
// pt = c0 + sk (.) c1 (secret-key decryption): grid (N / 256, nl, nct)
__global__ __launch_bounds__(GR_T) void k_gri_decrypt(const u64 *ct, const u64 *sk, u64 *pt, const GrMod *modc, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, t = blockIdx.y; const size_t c = blockIdx.z; const GrMod mc = modc[t];
    pt[(c * nl + t) * N + x] = gr::addmod(ct[(c * 2 * nl + t) * N + x], gr::mulmod(sk[(size_t)t * N + x], ct[((c * 2 + 1) * nl + t) * N + x], mc.q, mc.uhi, mc.ulo), mc.q);
}

// exp(-i pi num / den), 0 <= num < den, den a power of two >= 4: the angle reduced to an octant (pi r, r = r_num / den exact in double, 0 <= r <= 1/4), the Taylor series
// of ddfft.hpp in double-double there; exact at the multiples of pi / 2
static void gdd_expm(long long num, long long den, double *out4) {
    const ::dd pi = dd_make(3.141592653589793116e+00, 1.224646799147353207e-16);
    bool negc = false, swap = false; long long r = num;
    if (2 * r > den) { r = den - r; negc = true; }
    if (4 * r > den) { r = den / 2 - r; swap = true; }
    ::dd s, c; dd_sincos_small(::dd_mul_d(pi, (double)r / (double)den), s, c);
    if (swap) { const ::dd t = s; s = c; c = t; }
    if (negc) c = dd_neg(c);
    out4[0] = c.hi; out4[1] = c.lo; out4[2] = -s.hi; out4[3] = -s.lo;
}
int gri_dd_tab(sfg_ring *r, GriDdTab *out) {
    const int N = r->N, n = N / 2;
    if (!r->io.dd_tab) {
        const size_t bW = (size_t)(n / 2) * 32, bZ = (size_t)n * 32, bS = (size_t)n * 4;
        std::vector<unsigned char> h(bW + bZ + 2 * bS);
        double *W = (double *)h.data(), *Z = (double *)(h.data() + bW); uint32_t *sm = (uint32_t *)(h.data() + bW + bZ), *sp = sm + n;
        for (int k = 0; k < n / 2; k++) gdd_expm(2LL * k, n, W + 4 * k);
        for (int c = 0; c < n; c++) gdd_expm(c, N, Z + 4 * c);
        const int logn = r->logN - 1; u64 g = 1;
        for (int t = 0; t < n; t++) {
            const uint32_t m = (uint32_t)(((g - 1) / 4) % (u64)n); uint32_t rev = 0;
            for (int i = 0; i < logn; i++) rev |= ((m >> i) & 1u) << (logn - 1 - i);
            sm[t] = m; sp[t] = rev; g = g * 5 % (2ULL * N);
        }
        GrBuf<void> d; GR_TRY(gr_table(r, d, h.data(), h.size()));
        r->io.dd_tab = std::move(d);
    }
    const unsigned char *d = (const unsigned char *)r->io.dd_tab.p;
    out->W = (const double4 *)d; out->Z = (const double4 *)(d + (size_t)(n / 2) * 32);
    out->slot_m = (const uint32_t *)(d + (size_t)(n / 2) * 32 + (size_t)n * 32); out->slot_pos = out->slot_m + n;
    return 0;
}
static int gdd_transform(sfg_ring *r, double4 *A, int nvec, const GriDdTab &t) {
    const int logn = r->logN - 1, a = logn / 2, b = logn - a, n = 1 << logn;
    const dim3 grid(n / GDD_TILE, (unsigned)nvec);
    hipLaunchKernelGGL(k_gdd_cols, grid, dim3(GR_T), 0, r->stream, A, t.W, logn, a, b);
    hipLaunchKernelGGL(k_gdd_contig, grid, dim3(GR_T), 0, r->stream, A, t.W, logn, a, b);
    GR_HIP(r, hipGetLastError());
    return 0;
}

int gri_encode_dft(sfg_ring *r, double4 *A, int nb, const GriDdTab &tab, const double *band_dev, unsigned *flags, unsigned *ties, u64 *R, int nl, double scale) {
    const int n = r->N / 2, logn = r->logN - 1;
    GR_TRY(gdd_transform(r, A, nb, tab));
    hipLaunchKernelGGL(k_gdd_enc_post, dim3(n / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, (const double4 *)A, tab.Z, R, flags, ties, band_dev, r->modc, scale / n, logn, nl);
    GR_HIP(r, hipGetLastError());
    return 0;
}
int gri_encode_refuse(sfg_ring *r, const char *what, const unsigned *f, double scale) {
    if (f[1]) GR_FAIL(r, "%s: %u coefficients are outside the domain |p| < 2^62 (scale %g)", what, f[1], scale);
    if (f[0]) GR_FAIL(r, "%s: %u coefficients lie within the proven band of a rounding tie: no plaintext is handed out", what, f[0]);
    return 0;
}
// real slot vectors -> NTT-domain plaintext rows dst [nvec][level+1][N] (device).  Nothing is written to dst unless every coefficient of every vector is proven.
static int gri_encode(sfg_ring *r, const char *what, const double *values, int nvec, int level, double scale, u64 *dst) {
    const int nl = level + 1, N = r->N, n = N / 2;
    if (!(scale >= 1.0) || !std::isfinite(scale)) GR_FAIL(r, "%s: scale %g must be finite and at least 1", what, scale);
    std::vector<double> band(nvec);
    for (int v = 0; v < nvec; v++) {
        double s1 = 0.0;
        for (int t = 0; t < n; t++) { const double x = values[(size_t)v * n + t]; if (!std::isfinite(x)) GR_FAIL(r, "%s: value %d of vector %d is not finite", what, t, v); s1 += std::fabs(x); }
        band[v] = gio::enc_band(s1 * (scale / n) * (1.0 + 0x1p-40));           // S with its own rounding covered (n + 1 roundings of 2^-53 each)
    }
    GriDdTab tab; GR_TRY(gri_dd_tab(r, &tab));
    const GriPlan plan = gri_encode_plan(nvec, nl, (size_t)N, r->io.ws_budget);
    GR_TRY(gr_reserve(r, r->io.ws, plan.reserve()));
    const GriEncodeLayout lay = gri_encode_layout(nl, (size_t)N, (size_t)plan.chunk);
    u64 *ws = (u64 *)r->io.ws.p;
    double4 *A = (double4 *)(ws + lay.A); double *vals = (double *)(ws + lay.vals); u64 *R = ws + lay.R;
    double *bandd = (double *)(ws + lay.band); unsigned *flags = (unsigned *)(ws + lay.flags);
    for (int pass = plan.nchunks > 1 ? 0 : 1; pass < 2; pass++)                  // several chunks: a checking pass over all of them first, then the writing pass
        for (int c = 0; c < plan.nchunks; c++) {
            const int c0 = plan.first(c), nb = plan.count(c, nvec);
            GR_HIP(r, hipMemcpyAsync(vals, values + (size_t)c0 * n, (size_t)nb * n * 8, hipMemcpyHostToDevice, r->stream));
            GR_HIP(r, hipMemcpyAsync(bandd, band.data() + c0, (size_t)nb * 8, hipMemcpyHostToDevice, r->stream));
            GR_HIP(r, hipMemsetAsync(flags, 0, 8, r->stream));
            GR_HIP(r, hipMemsetAsync(A, 0, (size_t)nb * n * 32, r->stream));
            hipLaunchKernelGGL(k_gdd_enc_load, dim3(n / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, (const double *)vals, A, tab.slot_m, n);
            GR_HIP(r, hipGetLastError());
            GR_TRY(gri_encode_dft(r, A, nb, tab, bandd, flags, nullptr, R, nl, scale));
            unsigned f[2];
            GR_HIP(r, hipMemcpyAsync(f, flags, 8, hipMemcpyDeviceToHost, r->stream));
            GR_HIP(r, hipStreamSynchronize(r->stream));
            GR_TRY(gri_encode_refuse(r, what, f, scale));
            if (pass == 0) continue;
            GR_TRY(gr_transform(r, R, (size_t)nb * nl, gr_map(nl, nl, 0, 0), false));
            GR_HIP(r, hipMemcpyAsync(dst + (size_t)c0 * nl * N, R, (size_t)nb * nl * N * 8, hipMemcpyDeviceToDevice, r->stream));
        }
    return 0;
}
// plaintext rows (stride words apart) -> slot values; re / im on the device when dev_out, else on the host (the call then synchronises).  im may be null.
static int gri_decode_vectors(sfg_ring *r, const u64 *src, size_t stride, int nct, int level, double scale, double *re, double *im, bool dev_out) {
    const int nl = level + 1, N = r->N, n = N / 2;
    GriDecTab dtab; GR_TRY(gri_dec_tab(r, level, &dtab));
    GriDdTab tab; GR_TRY(gri_dd_tab(r, &tab));
    const GriPlan plan = gri_vectors_plan(nct, nl, (size_t)N, r->io.ws_budget);
    GR_TRY(gr_reserve(r, r->io.ws, plan.reserve()));
    const GriVectorsLayout lay = gri_vectors_layout(nl, (size_t)N, (size_t)plan.chunk);
    u64 *ws = (u64 *)r->io.ws.p;
    double4 *A = (double4 *)(ws + lay.A); double2 *Wd = (double2 *)(ws + lay.Wd); u64 *X = ws + lay.X; double *ore = (double *)(ws + lay.re), *oim = (double *)(ws + lay.im);
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct);
        GR_TRY(gri_digits(r, src + (size_t)c0 * stride, stride, nb, level, X, dtab));
        hipLaunchKernelGGL(k_gri_decode_fin_dd, dim3(N / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, X, Wd, dtab, r->modc, nl, N, scale);
        hipLaunchKernelGGL(k_gdd_dec_load, dim3(n / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, (const double2 *)Wd, tab.Z, A, n);
        GR_TRY(gdd_transform(r, A, nb, tab));
        double *dre = dev_out ? re + (size_t)c0 * n : ore, *dim_ = !im ? nullptr : dev_out ? im + (size_t)c0 * n : oim;
        hipLaunchKernelGGL(k_gdd_dec_post, dim3(n / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, (const double4 *)A, tab.slot_pos, dre, dim_, n);
        GR_HIP(r, hipGetLastError());
        if (!dev_out) {
            GR_HIP(r, hipMemcpyAsync(re + (size_t)c0 * n, ore, (size_t)nb * n * 8, hipMemcpyDeviceToHost, r->stream));
            if (im) GR_HIP(r, hipMemcpyAsync(im + (size_t)c0 * n, oim, (size_t)nb * n * 8, hipMemcpyDeviceToHost, r->stream));
            GR_HIP(r, hipStreamSynchronize(r->stream));
        }
    }
    return 0;
}

extern "C" int sfg_ring_encode_vectors_dev(sfg_ring *r, const double *values_host, int nvec, int level, double scale, uint64_t *pt) {
    const int nct = nvec;
    GRI_ENTRY("sfg_ring_encode_vectors_dev")
    if (!values_host || !pt) GR_FAIL(r, "sfg_ring_encode_vectors_dev: null values or output");
    return gri_encode(r, "sfg_ring_encode_vectors_dev", values_host, nvec, level, scale, (u64 *)pt);
}
extern "C" int sfg_ring_encrypt_vectors_dev(sfg_ring *r, const double *values_host, int nct, int level, double scale, uint64_t *out) {
    GRI_ENTRY("sfg_ring_encrypt_vectors_dev")
    if (!r->io.pk) GR_FAIL(r, "sfg_ring_encrypt_vectors_dev: no public key loaded (sfg_ring_load_public_key)");
    if (!values_host || !out) GR_FAIL(r, "sfg_ring_encrypt_vectors_dev: null values or output");
    if (!r->io.enc_seeded) GR_FAIL(r, "sfg_ring_encrypt_vectors_dev: the encryptor has no key (sfg_ring_seed_encryptor); there is no default");
    GR_TRY(gr_reserve(r, r->io.pt, (size_t)nct * (level + 1) * r->N * 8));
    GR_TRY(gri_encode(r, "sfg_ring_encrypt_vectors_dev", values_host, nct, level, scale, r->io.pt));      // the encoder's rows and its refusals, before an index is spent
    GriPlan plan; GR_TRY(gri_reserve(r, 2, nct, level, true, plan));
    u64 first; GR_TRY(gri_take_indices(r, "sfg_ring_encrypt_vectors_dev", nct, &first));
    GriSrc src{nullptr, nullptr, nullptr, r->io.enc_key_dev, first};
    return gri_core(r, plan, src, r->io.pk, 2, nct, level, GRI_OUT, r->io.pt, (u64 *)out, nullptr);
}
extern "C" int sfg_ring_decode_vectors(sfg_ring *r, const uint64_t *pt, size_t pt_stride, int nct, int level, double scale, double *re_host, double *im_host) {
    GRI_ENTRY("sfg_ring_decode_vectors")
    GR_TRY(gri_decode_checks(r, "sfg_ring_decode_vectors", pt, re_host, pt_stride, level, scale));
    return gri_decode_vectors(r, (const u64 *)pt, pt_stride, nct, level, scale, re_host, im_host, false);
}
extern "C" int sfg_ring_decode_vectors_dev(sfg_ring *r, const uint64_t *pt, size_t pt_stride, int nct, int level, double scale, double *re_dev, double *im_dev) {
    GRI_ENTRY("sfg_ring_decode_vectors_dev")
    GR_TRY(gri_decode_checks(r, "sfg_ring_decode_vectors_dev", pt, re_dev, pt_stride, level, scale));
    return gri_decode_vectors(r, (const u64 *)pt, pt_stride, nct, level, scale, re_dev, im_dev, true);
}
extern "C" int sfg_ring_decrypt_vectors(sfg_ring *r, const uint64_t *ct, int nct, int level, double scale, double *re_host, double *im_host) {
    GRI_ENTRY("sfg_ring_decrypt_vectors")
    if (!r->io.sk) GR_FAIL(r, "sfg_ring_decrypt_vectors: no secret key loaded (sfg_ring_load_secret_key)");
    const int nl = level + 1, N = r->N; const size_t rowsw = (size_t)nl * N;
    GR_TRY(gri_decode_checks(r, "sfg_ring_decrypt_vectors", ct, re_host, rowsw, level, scale));
    GR_TRY(gr_reserve(r, r->io.pt, (size_t)nct * rowsw * 8));
    gr_split((size_t)nct, kGrLaunchCap, [&](size_t c0, size_t nb) {
        hipLaunchKernelGGL(k_gri_decrypt, dim3(N / GR_T, nl, (unsigned)nb), dim3(GR_T), 0, r->stream, (const u64 *)ct + c0 * 2 * rowsw, r->io.sk, r->io.pt + c0 * rowsw, r->modc, nl, N);
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return gri_decode_vectors(r, r->io.pt, rowsw, nct, level, scale, re_host, im_host, false);
}
