// gring_keygen.hip - the general ring's collective key generation on the device: the local halves of mpc.CollectiveInit (mpc/mhe.go:24-81) at every ring
// sfg_ring_create accepts.  The twin of keygen.hip in the ring's integer arithmetic: the same three equations, the same key convention
// (digit i = (b_i, a_i); g_i at modulus m = P mod q_m when m < nq && m / np == i; a rotation key for g switches from phi_{g^-1}(s)), the same sampled forms and
// index accounting, the same map from a seed to the common reference polynomials, the same installation from device memory.  PARITY UNPINNED as there.
// Per-element epilogues and their bounds: gring_keygen_arith.hpp.  Chunks and bytes to reserve: gring_keygen_plan.hpp.  DESIGN.md section 16.
//
// A share row is made IN THE CALLER'S OUTPUT BUFFER, no u64 workspace for the shares:
//   1. k_grk_lift     the error polynomial (drawn from the encryptor's stream in this kernel through gri_sample8, or the caller's) lifted modulo all nmod moduli
//                     into the share's own rows
//   2. the ring's forward columns pass over those rows (gring.hip: k_gr_cols<false> as it is, through gr_transform_cols_fwd)
//   3. k_grk_contig   the forward contiguous pass with the share's arithmetic as its epilogue: the row is formed in registers from the tile, crp (coalesced) and sk
//                     (gathered through the NTT-domain index of g^-1; a row of sk is at most 512 KiB and stays in L2) and written once
// The stage loop of k_grk_contig RESTATES k_gr_contig<false>'s ten lines (gring.hip) rather than sharing them through a __device__ function: the four transform
// kernels stay untouched.  The relinearisation rounds transform NTT(u) once per call into a wiping workspace and read it from there.
// All launches go on the ring's stream.  Every word written is canonical.
#include <cstdio>
#include <cstring>
#include <vector>
#include "gring_dev.hpp"
#include "gring_sampler.hpp"
#include "gring_keygen_arith.hpp"
#include "gring_keygen_plan.hpp"

static_assert(kGrkLaunchRows == kGrLaunchCap, "gring_keygen_plan.hpp restates the transform's launch cap");

// ---------------------------------------------------------------- sampling and lifting
struct GrkSrc { const int32_t *ea, *eb; const unsigned *key; u64 index0; };     // key != nullptr: polynomial z draws ids 1, 2 of index0 + z; else the caller's [npoly][N]
// grid (N / 8 / 256, 1, npoly).  d0 [npoly][nmod][N] = lift(ea) (sum: lift(ea) + lift(eb)); d1 (nullable) [npoly][nmod][N] = lift(eb).
// j = 512 (8 g + k) + t < 4096 (g + 1) <= N since g < N / 4096 by the grid.
template <bool SAMPLE>
__global__ __launch_bounds__(GR_T) void k_grk_lift(GrkSrc src, u64 *d0, u64 *d1, int sum, const GrMod *modc, int nmod, int N) {
    const int id = blockIdx.x * GR_T + threadIdx.x, t = id & (gio::kSampT - 1), g = id >> 9;
    const size_t z = blockIdx.z;
    const bool two = d1 != nullptr || sum;
    int su[8], s0[8], s1[8];
#pragma unroll
    for (int k = 0; k < 8; k++) su[k] = s0[k] = s1[k] = 0;
    if (SAMPLE) {
        unsigned key[8];
#pragma unroll
        for (int i = 0; i < 8; i++) key[i] = src.key[i];
        gri_sample8(key, src.index0 + z, t, g, false, two ? 2 : 1, su, s0, s1);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const size_t j = z * N + (size_t)gio::kSampT * (8 * g + k) + t;
            s0[k] = src.ea[j];
            if (two) s1[k] = src.eb[j];
        }
    }
    for (int m = 0; m < nmod; m++) {
        const u64 q = modc[m].q;
        u64 *D0 = d0 + (z * nmod + m) * N, *D1 = d1 ? d1 + (z * nmod + m) * N : nullptr;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int j = gio::kSampT * (8 * g + k) + t;
            D0[j] = sum ? gkg::lift_sum(s0[k], s1[k], q) : gio::lift(s0[k], q);
            if (D1) D1[j] = gio::lift(s1[k], q);
        }
    }
}
// the ephemeral u of a relinearisation round (polynomial id 0 of u_index, or the caller's int8 [N]) lifted into U [nmod][N]: grid (N / 8 / 256)
template <bool SAMPLE>
__global__ __launch_bounds__(GR_T) void k_grk_lift_u(const int8_t *u, const unsigned *keyp, u64 u_index, u64 *U, const GrMod *modc, int nmod, int N) {
    const int id = blockIdx.x * GR_T + threadIdx.x, t = id & (gio::kSampT - 1), g = id >> 9;
    int su[8], s0[8], s1[8];
#pragma unroll
    for (int k = 0; k < 8; k++) su[k] = s0[k] = s1[k] = 0;
    if (SAMPLE) {
        unsigned key[8];
#pragma unroll
        for (int i = 0; i < 8; i++) key[i] = keyp[i];
        gri_sample8(key, u_index, t, g, true, 0, su, s0, s1);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) su[k] = u[gio::kSampT * (8 * g + k) + t];
    }
    for (int m = 0; m < nmod; m++) {
        const u64 q = modc[m].q;
#pragma unroll
        for (int k = 0; k < 8; k++) U[(size_t)m * N + gio::kSampT * (8 * g + k) + t] = gio::lift(su[k], q);
    }
}

// ---------------------------------------------------------------- the automorphism index on the device
// gkg::index_entry (gring_keygen_arith.hpp): the table sfg_ring_load_rotkey builds on the host, entry by entry.  Every entry is below N.
// grid (N / 256, nkeys): idx [nkeys][N], key k under gal[k]
__global__ __launch_bounds__(GR_T) void k_grk_index(const u64 *gal, uint32_t *idx, int logN) {
    const int i = blockIdx.x * GR_T + threadIdx.x;
    idx[((size_t)blockIdx.y << logN) + i] = gkg::index_entry(gal[blockIdx.y], i, logN);
}

// ---------------------------------------------------------------- the hot kernel: forward contiguous pass + the share's epilogue
// rows [npoly][nmod][N] (polynomial = row / nmod, modulus = row % nmod; key = polynomial / beta, digit = polynomial % beta), after the columns pass.
//   GRK_SHARE  row = NTT(e) - A (.) B[index] (+ g_i sk)      A [npoly][nmod][N] = crp; B [nmod][N] = sk (shares; idx [nkeys][N] or null) or NTT(u) (round 1's h0)
//   GRK_H1     row = NTT(e) + sk (.) A                        A = crp
//   GRK_R2     row = NTT(e2 + e3) + sk (.) A + (B - sk) (.) A2   A = H0agg, A2 = H1agg, B = NTT(u)
// pmod [nmod][2]: P mod q_m and its Shoup quotient (rows of P: unused).
enum { GRK_SHARE, GRK_H1, GRK_R2 };
struct GrkEpi { const u64 *A, *A2, *B, *sk, *pmod; const uint32_t *idx; int gterm, beta, nq, np, nmod; };
// grid (N / 4096, rows <= kGrkLaunchRows).  tile index < 4096 by construction; global index x = blockIdx.x * 4096 + e < N; idx entries < N (gkg::index_entry).
template <int MODE>
__global__ __launch_bounds__(GR_T) void k_grk_contig(u64 *rows, GrkEpi ep, const GrMod *modc, const u64 *tw, int logN, int a, int b) {
    __shared__ u64 tile[GrNttPlan::kTileWords];
    const size_t row = blockIdx.y, poly = row / (size_t)ep.nmod;
    const int mod = (int)(row % (size_t)ep.nmod), N = 1 << logN;
    const GrMod mc = modc[mod];
    const u64 q = mc.q;
    const u64 *w = tw + (size_t)mod * 4 * N, *wsh = w + N;
    const int x0 = blockIdx.x * GrNttPlan::kTileWords;
    u64 *base = rows + row * (size_t)N + x0;
    const int chunk0 = blockIdx.x << (12 - b);
    for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T) tile[e] = base[e];
    __syncthreads();
    // k_gr_contig<false>'s stage loop, restated: distance t = 2^(b-1) .. 1; twiddle (2^(b-1) / t) (2^a + chunk) + (group index inside the chunk) < N
    for (int s = 0; s < b; s++) {
        const int lt = b - 1 - s, t = 1 << lt, lm = b - 1 - lt;
        for (int k = threadIdx.x; k < GrNttPlan::kTileWords / 2; k += GR_T) {
            const int ch = k >> (b - 1), bb = k & ((1 << (b - 1)) - 1), i = bb >> lt, j = (ch << b) + (i << (lt + 1)) + (bb & (t - 1));
            const int ti = (((1 << a) + chunk0 + ch) << lm) + i;
            u64 X = tile[j], Y = tile[j + t];
            gr::bfly_fwd(X, Y, w[ti], wsh[ti], q);
            tile[j] = X; tile[j + t] = Y;
        }
        __syncthreads();
    }
    const u64 *A = ep.A + row * (size_t)N + x0, *sk = ep.sk + (size_t)mod * N;
    if (MODE == GRK_SHARE) {
        const u64 *B = ep.B + (size_t)mod * N;
        const uint32_t *ix = ep.idx ? ep.idx + (poly / (size_t)ep.beta) * N : nullptr;
        const bool with_g = ep.gterm && gkg::g_applies((int)(poly % (size_t)ep.beta), mod, ep.nq, ep.np);      // uniform over the workgroup
        const u64 pg = with_g ? ep.pmod[2 * mod] : 0, pg_sh = with_g ? ep.pmod[2 * mod + 1] : 0;
        for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T) {
            const int x = x0 + e;
            base[e] = gkg::share(gr::canon4(tile[e], q), A[e], B[ix ? (int)ix[x] : x], with_g ? sk[x] : 0, with_g, pg, pg_sh, q, mc.uhi, mc.ulo);
        }
    } else if (MODE == GRK_H1) {
        for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T) base[e] = gkg::round1_h1(gr::canon4(tile[e], q), A[e], sk[x0 + e], q, mc.uhi, mc.ulo);
    } else {
        const u64 *A2 = ep.A2 + row * (size_t)N + x0, *U = ep.B + (size_t)mod * N;
        for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T)
            base[e] = gkg::round2(gr::canon4(tile[e], q), A[e], A2[e], sk[x0 + e], U[x0 + e], q, mc.uhi, mc.ulo);
    }
}

// ---------------------------------------------------------------- installation: the key storage from device memory
// key [beta][2][nmod][N] (sfg_ring_load_rotkey's; the words kept as given) from b = agg [beta][nmod][N], a = crp [beta][nmod][N]; idx (nullable) [N]: the index of g.
// grid (N / 256, beta * nmod); x < N by the grid
__global__ __launch_bounds__(GR_T) void k_grk_install(const u64 *b, const u64 *a, u64 *key, uint32_t *idx, u64 g, int nmod, int logN) {
    const int x = blockIdx.x * GR_T + threadIdx.x, N = 1 << logN; const size_t row = blockIdx.y, i = row / (size_t)nmod, m = row % (size_t)nmod;
    key[((i * 2 + 0) * nmod + m) * N + x] = b[row * N + x];
    key[((i * 2 + 1) * nmod + m) * N + x] = a[row * N + x];
    if (idx && row == 0) idx[x] = gkg::index_entry(g, x, logN);
}

// ---------------------------------------------------------------- common reference polynomials
// keygen.hip's map (k_crp_fill) at any N and any modulus below 2^61: row r (global number first_row + blockIdx.y) at modulus q, coefficient j:
// ChaCha20 block under the seed with block counter j and nonce (r low word, r high word, try t); the first of its eight masked 64-bit candidates below q, else the
// same with t + 1.  One thread per coefficient; the seed is a kernel argument and is not retained.  grid (N / 256, nrows <= kGrkLaunchRows)
struct GrkSeed { unsigned k[8]; };
__global__ __launch_bounds__(GR_T) void k_grk_crp(GrkSeed key, u64 first_row, const int *mod_idx, const GrMod *modc, u64 *out, int N) {
    const size_t row = blockIdx.y; const int j = blockIdx.x * GR_T + threadIdx.x;
    const u64 q = modc[mod_idx[row]].q, mask = gkg::crp_mask(q), r = first_row + row;
    unsigned kk[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) kk[i] = key.k[i];
    u64 val = 0; bool found = false;
    for (unsigned t = 0; !found; t++) {
        chacha20_block(kk, (unsigned)j, (unsigned)r, (unsigned)(r >> 32), t, w);
        found = gkg::crp_pick(w, q, mask, val);
    }
    out[row * N + j] = val;
}

// ---------------------------------------------------------------- host side
static int grk_check_sk(sfg_ring *r, const char *what) {
    if (!r->kg.skqp) GR_FAIL(r, "%s: no secret key over QP loaded (sfg_ring_load_secret_key_qp)", what);
    return 0;
}
static int grk_check_seeded(sfg_ring *r, const char *what) {
    if (!r->io.enc_seeded) GR_FAIL(r, "%s: the encryptor has no key (sfg_ring_seed_encryptor); there is no default", what);
    return 0;
}
static int grk_check_galois(sfg_ring *r, const char *what, const uint64_t *galois, int nkeys) {
    if (nkeys < 0) GR_FAIL(r, "%s: negative key count %d", what, nkeys);
    if (nkeys > 0 && !galois) GR_FAIL(r, "%s: null Galois elements", what);
    for (int k = 0; k < nkeys; k++)
        if (!(galois[k] & 1) || galois[k] >= 2ULL * r->N) GR_FAIL(r, "%s: galois element %llu is not an odd number below 2N", what, (unsigned long long)galois[k]);
    return 0;
}
static GrkEpi grk_epi(const sfg_ring *r, const u64 *A, const u64 *A2, const u64 *B, const uint32_t *idx, int gterm, int beta) {
    return GrkEpi{A, A2, B, r->kg.skqp, r->kg.pmod, idx, gterm, beta, r->nq, r->np, r->nmod};
}
static GrRowMap grk_map(const sfg_ring *r) { return gr_map(r->nmod, r->nmod, 0, 0); }      // row % nmod is the row's modulus
template <int MODE> static int grk_contig(sfg_ring *r, u64 *rows, size_t nrows, const GrkEpi &ep) {
    const GrNttPlan &p = r->plan;
    hipLaunchKernelGGL(k_grk_contig<MODE>, dim3((unsigned)p.tiles_per_row, (unsigned)nrows), dim3(GR_T), 0, r->stream, rows, ep, r->modc, r->tw, p.logN, p.a, p.b);
    GR_HIP(r, hipGetLastError());
    return 0;
}
static int grk_lift(sfg_ring *r, const GrkSrc &src, u64 *d0, u64 *d1, int sum, size_t npoly) {
    const dim3 grid(r->N / 8 / GR_T, 1, (unsigned)npoly);
    if (src.key) hipLaunchKernelGGL(k_grk_lift<true>, grid, dim3(GR_T), 0, r->stream, src, d0, d1, sum, r->modc, r->nmod, r->N);
    else hipLaunchKernelGGL(k_grk_lift<false>, grid, dim3(GR_T), 0, r->stream, src, d0, d1, sum, r->modc, r->nmod, r->N);
    GR_HIP(r, hipGetLastError());
    return 0;
}
// NTT(u) at all nmod moduli in the wiping workspace (reserved by the caller from the plan)
static int grk_make_u(sfg_ring *r, const int8_t *u, bool sampled, u64 u_index) {
    const dim3 grid(r->N / 8 / GR_T);
    if (sampled) hipLaunchKernelGGL(k_grk_lift_u<true>, grid, dim3(GR_T), 0, r->stream, u, (const unsigned *)r->io.enc_key_dev, u_index, (u64 *)r->kg.u, r->modc, r->nmod, r->N);
    else hipLaunchKernelGGL(k_grk_lift_u<false>, grid, dim3(GR_T), 0, r->stream, u, (const unsigned *)nullptr, (u64)0, (u64 *)r->kg.u, r->modc, r->nmod, r->N);
    GR_HIP(r, hipGetLastError());
    return gr_transform(r, r->kg.u, (size_t)r->nmod, grk_map(r), false);
}

// shares of nkeys keys of `per` polynomials each (the public key: one key of one polynomial, no automorphism, no g term) in the chunks of the plan
static int grk_run_shares(sfg_ring *r, const GrkPlan &plan, const GrkSrc &src0, const uint64_t *galois, size_t nkeys, bool pubkey, const u64 *crp, u64 *out) {
    const size_t N = r->N, per = pubkey ? 1 : (size_t)r->beta, nmod = r->nmod;
    uint32_t *idx = pubkey ? nullptr : (uint32_t *)r->kg.index.p;
    u64 *gal_dev = pubkey ? nullptr : (u64 *)((unsigned char *)r->kg.index.p + plan.galois_at);
    std::vector<u64> ginv;
    for (size_t c = 0; c < plan.nchunks; c++) {
        const size_t k0 = plan.first(c), nk = plan.count(c, nkeys), p0 = k0 * per, npoly = nk * per, nrows = npoly * nmod;
        if (!pubkey) {
            ginv.resize(nk);
            for (size_t k = 0; k < nk; k++) ginv[k] = gkg::share_galois(galois[k0 + k], r->logN);
            GR_TRY(gr_upload(r, gal_dev, ginv.data(), nk * 8));
            hipLaunchKernelGGL(k_grk_index, dim3((unsigned)(N / GR_T), (unsigned)nk), dim3(GR_T), 0, r->stream, (const u64 *)gal_dev, idx, r->logN);
            GR_HIP(r, hipGetLastError());
        }
        GrkSrc src = src0;
        if (src.key) src.index0 += p0; else src.ea += p0 * N;
        u64 *rows = out + p0 * nmod * N;
        GR_TRY(grk_lift(r, src, rows, nullptr, 0, npoly));
        GR_TRY(gr_transform_cols_fwd(r, rows, nrows, grk_map(r)));
        GR_TRY(grk_contig<GRK_SHARE>(r, rows, nrows, grk_epi(r, crp + p0 * nmod * N, nullptr, r->kg.skqp, idx, pubkey ? 0 : 1, (int)per)));
    }
    return 0;
}

// The four share entry points, each in its explicit form (the caller's small polynomials) and its sampled form (none given: they come from the encryptor's stream; the
// workspace is reserved first, then the indices are taken, the first reported through first_index, nullable).
static int grk_ckg(sfg_ring *r, const char *what, bool sampled, const uint64_t *crp, const int32_t *e, uint64_t *share, uint64_t *first_index) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(grk_check_sk(r, what));
    if (sampled) GR_TRY(grk_check_seeded(r, what));
    if (!crp || (!sampled && !e) || !share) GR_FAIL(r, "%s: null polynomial or output", what);
    GrkPlan plan = grk_plan(1, 1, r->nmod, (size_t)r->N, false);
    GrkSrc src{e, nullptr, nullptr, 0};
    if (sampled) {
        GR_TRY(gri_take_indices(r, what, 1, &src.index0));
        if (first_index) *first_index = src.index0;
        src.key = r->io.enc_key_dev;
    }
    return grk_run_shares(r, plan, src, nullptr, 1, true, (const u64 *)crp, (u64 *)share);
}
static int grk_rtg(sfg_ring *r, const char *what, bool sampled, const uint64_t *galois, int nkeys, const uint64_t *crp, const int32_t *e, uint64_t *shares, uint64_t *first_index) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(grk_check_sk(r, what));
    GR_TRY(grk_check_galois(r, what, galois, nkeys));
    if (sampled) GR_TRY(grk_check_seeded(r, what));               // (before the empty call returns)
    if (!nkeys) return 0;
    if (!crp || (!sampled && !e) || !shares) GR_FAIL(r, "%s: null polynomial or output", what);
    if (sampled && (long long)nkeys * r->beta > 0x7FFFFFFFLL) GR_FAIL(r, "%s: too many keys in one call", what);
    const GrkPlan plan = grk_plan((size_t)nkeys, r->beta, r->nmod, (size_t)r->N, false);
    GR_TRY(gr_reserve(r, r->kg.index, plan.index_bytes));          // before an index is taken: a failed allocation leaves the counter where it was
    GrkSrc src{e, nullptr, nullptr, 0};
    if (sampled) {
        GR_TRY(gri_take_indices(r, what, nkeys * r->beta, &src.index0));
        if (first_index) *first_index = src.index0;
        src.key = r->io.enc_key_dev;
    }
    return grk_run_shares(r, plan, src, galois, (size_t)nkeys, false, (const u64 *)crp, (u64 *)shares);
}
// round 1 takes beta + 1 indices (the last is u's, reported through u_index: round 2 needs it); round 2 takes beta and reads u at u_index
static int grk_rkg1(sfg_ring *r, const char *what, bool sampled, const uint64_t *crp, const int8_t *u, const int32_t *e0, const int32_t *e1, uint64_t *h0, uint64_t *h1,
                    uint64_t *first_index, uint64_t *u_index) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(grk_check_sk(r, what));
    if (sampled) GR_TRY(grk_check_seeded(r, what));
    if (!crp || !h0 || !h1 || (sampled ? !u_index : (!u || !e0 || !e1))) GR_FAIL(r, "%s: null polynomial or output%s", what, sampled ? " or u_index (round 2 needs it)" : "");
    const size_t beta = r->beta, nrows = beta * r->nmod;
    const GrkPlan plan = grk_plan(0, r->beta, r->nmod, (size_t)r->N, true);
    GR_TRY(gr_reserve(r, r->kg.u, plan.u_bytes));
    GrkSrc src{e0, e1, nullptr, 0}; u64 ui = 0;
    if (sampled) {
        GR_TRY(gri_take_indices(r, what, r->beta + 1, &src.index0));
        if (first_index) *first_index = src.index0;
        *u_index = ui = src.index0 + beta;
        src.key = r->io.enc_key_dev;
    }
    GR_TRY(grk_make_u(r, u, sampled, ui));
    GR_TRY(grk_lift(r, src, (u64 *)h0, (u64 *)h1, 0, beta));
    GR_TRY(gr_transform_cols_fwd(r, (u64 *)h0, nrows, grk_map(r)));
    GR_TRY(gr_transform_cols_fwd(r, (u64 *)h1, nrows, grk_map(r)));
    GR_TRY(grk_contig<GRK_SHARE>(r, (u64 *)h0, nrows, grk_epi(r, (const u64 *)crp, nullptr, r->kg.u, nullptr, 1, r->beta)));
    return grk_contig<GRK_H1>(r, (u64 *)h1, nrows, grk_epi(r, (const u64 *)crp, nullptr, nullptr, nullptr, 0, r->beta));
}
static int grk_rkg2(sfg_ring *r, const char *what, bool sampled, const uint64_t *h0agg, const uint64_t *h1agg, const int8_t *u, const int32_t *e2, const int32_t *e3,
                    uint64_t u_index, uint64_t *out, uint64_t *first_index) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(grk_check_sk(r, what));
    if (sampled) GR_TRY(grk_check_seeded(r, what));
    if (!h0agg || !h1agg || !out || (!sampled && (!u || !e2 || !e3))) GR_FAIL(r, "%s: null polynomial or output", what);
    const size_t beta = r->beta, nrows = beta * r->nmod;
    const GrkPlan plan = grk_plan(0, r->beta, r->nmod, (size_t)r->N, true);
    GR_TRY(gr_reserve(r, r->kg.u, plan.u_bytes));
    GrkSrc src{e2, e3, nullptr, 0};
    if (sampled) {
        GR_TRY(gri_take_indices(r, what, r->beta, &src.index0));
        if (first_index) *first_index = src.index0;
        src.key = r->io.enc_key_dev;
    }
    GR_TRY(grk_make_u(r, u, sampled, (u64)u_index));
    GR_TRY(grk_lift(r, src, (u64 *)out, nullptr, 1, beta));        // e2 + e3 as one polynomial
    GR_TRY(gr_transform_cols_fwd(r, (u64 *)out, nrows, grk_map(r)));
    return grk_contig<GRK_R2>(r, (u64 *)out, nrows, grk_epi(r, (const u64 *)h0agg, (const u64 *)h1agg, r->kg.u, nullptr, 0, r->beta));
}

// ---------------------------------------------------------------- C-ABI
extern "C" int sfg_ring_load_secret_key_qp(sfg_ring *r, const uint64_t *sk_host, int mont) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!sk_host) GR_FAIL(r, "sfg_ring_load_secret_key_qp: null key");
    const size_t words = (size_t)r->nmod * r->N, qwords = (size_t)r->nq * r->N;
    GR_HIP(r, hipStreamSynchronize(r->stream));                                // launches that still read the previous key
    if (!r->kg.pmod) {
        std::vector<u64> pm((size_t)2 * r->nmod, 0);
        for (int m = 0; m < r->nq; m++) { const u64 q = r->q[m]; u64 P = 1; for (int p = 0; p < r->np; p++) P = hm_mul(P, r->q[r->nq + p] % q, q); pm[2 * m] = P; pm[2 * m + 1] = hm_shoup(P, q); }
        GrBuf<u64> t; GR_TRY(gr_table(r, t, pm.data(), pm.size() * 8));
        r->kg.pmod = std::move(t);
    }
    if (!r->kg.skqp) GR_HIP(r, r->kg.skqp.alloc(words * 8));
    if (!r->io.sk) GR_HIP(r, r->io.sk.alloc(qwords * 8));
    GR_HIP(r, hipMemcpyAsync(r->kg.skqp, sk_host, words * 8, hipMemcpyHostToDevice, r->stream));
    if (mont) GR_TRY(gr_rows_from_mont(r, r->kg.skqp, (size_t)r->nmod));        // one group of nmod rows: row m is modulus m
    GR_HIP(r, hipMemcpyAsync(r->io.sk, r->kg.skqp, qwords * 8, hipMemcpyDeviceToDevice, r->stream));      // the rows sfg_ring_load_secret_key keeps
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}
extern "C" int sfg_ring_ckg_gen_share_dev(sfg_ring *r, const uint64_t *crp, const int32_t *e, uint64_t *share) { return grk_ckg(r, "sfg_ring_ckg_gen_share_dev", false, crp, e, share, nullptr); }
extern "C" int sfg_ring_ckg_gen_share_sampled_dev(sfg_ring *r, const uint64_t *crp, uint64_t *share, uint64_t *first_index) { return grk_ckg(r, "sfg_ring_ckg_gen_share_sampled_dev", true, crp, nullptr, share, first_index); }
extern "C" int sfg_ring_rtg_gen_shares_dev(sfg_ring *r, const uint64_t *galois_host, int nkeys, const uint64_t *crp, const int32_t *e, uint64_t *shares) {
    return grk_rtg(r, "sfg_ring_rtg_gen_shares_dev", false, galois_host, nkeys, crp, e, shares, nullptr);
}
extern "C" int sfg_ring_rtg_gen_shares_sampled_dev(sfg_ring *r, const uint64_t *galois_host, int nkeys, const uint64_t *crp, uint64_t *shares, uint64_t *first_index) {
    return grk_rtg(r, "sfg_ring_rtg_gen_shares_sampled_dev", true, galois_host, nkeys, crp, nullptr, shares, first_index);
}
extern "C" int sfg_ring_rkg_round1_dev(sfg_ring *r, const uint64_t *crp, const int8_t *u, const int32_t *e0, const int32_t *e1, uint64_t *h0, uint64_t *h1) {
    return grk_rkg1(r, "sfg_ring_rkg_round1_dev", false, crp, u, e0, e1, h0, h1, nullptr, nullptr);
}
extern "C" int sfg_ring_rkg_round1_sampled_dev(sfg_ring *r, const uint64_t *crp, uint64_t *h0, uint64_t *h1, uint64_t *first_index, uint64_t *u_index) {
    return grk_rkg1(r, "sfg_ring_rkg_round1_sampled_dev", true, crp, nullptr, nullptr, nullptr, h0, h1, first_index, u_index);
}
extern "C" int sfg_ring_rkg_round2_dev(sfg_ring *r, const uint64_t *h0agg, const uint64_t *h1agg, const int8_t *u, const int32_t *e2, const int32_t *e3, uint64_t *out) {
    return grk_rkg2(r, "sfg_ring_rkg_round2_dev", false, h0agg, h1agg, u, e2, e3, 0, out, nullptr);
}
extern "C" int sfg_ring_rkg_round2_sampled_dev(sfg_ring *r, const uint64_t *h0agg, const uint64_t *h1agg, uint64_t u_index, uint64_t *out, uint64_t *first_index) {
    return grk_rkg2(r, "sfg_ring_rkg_round2_sampled_dev", true, h0agg, h1agg, nullptr, nullptr, nullptr, u_index, out, first_index);
}

// one key's storage filled from (b, a) on the ring's stream; a new key's storage is the caller's until the key is complete
static int grk_fill_key(sfg_ring *r, GrKey &k, bool with_idx, u64 g, const u64 *b, const u64 *a) {
    const size_t words = (size_t)r->beta * 2 * r->nmod * r->N;
    if (!k.key) GR_HIP(r, k.key.alloc(words * 8));
    if (with_idx && !k.idx) GR_HIP(r, k.idx.alloc((size_t)r->N * 4));
    hipLaunchKernelGGL(k_grk_install, dim3(r->N / GR_T, (unsigned)(r->beta * r->nmod)), dim3(GR_T), 0, r->stream, b, a, (u64 *)k.key, with_idx ? (uint32_t *)k.idx : nullptr, g, r->nmod, r->logN);
    GR_HIP(r, hipGetLastError());
    return 0;
}
extern "C" int sfg_ring_install_public_key_dev(sfg_ring *r, const uint64_t *agg, const uint64_t *crp) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!agg || !crp) GR_FAIL(r, "sfg_ring_install_public_key_dev: null polynomial");
    const size_t row = (size_t)r->nmod * r->N * 8;
    GR_HIP(r, hipStreamSynchronize(r->stream));                                // launches that still read the previous key
    if (!r->io.pk) GR_HIP(r, r->io.pk.alloc(2 * row));
    GR_HIP(r, hipMemcpyAsync(r->io.pk, agg, row, hipMemcpyDeviceToDevice, r->stream));
    GR_HIP(r, hipMemcpyAsync((char *)r->io.pk.p + row, crp, row, hipMemcpyDeviceToDevice, r->stream));
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}
extern "C" int sfg_ring_install_rotkeys_dev(sfg_ring *r, const uint64_t *galois_host, int nkeys, const uint64_t *agg, const uint64_t *crp) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(grk_check_galois(r, "sfg_ring_install_rotkeys_dev", galois_host, nkeys));
    if (!nkeys) return 0;
    if (!agg || !crp) GR_FAIL(r, "sfg_ring_install_rotkeys_dev: null polynomial");
    const size_t per = (size_t)r->beta * r->nmod * r->N;
    for (int k = 0; k < nkeys; k++) {
        const u64 g = galois_host[k];
        GrKey fresh; const auto it = r->rotkeys.find(g);                        // a new element's key enters the map only when it is complete
        GrKey &key = it != r->rotkeys.end() ? it->second : fresh;
        GR_TRY(grk_fill_key(r, key, true, g, (const u64 *)agg + k * per, (const u64 *)crp + k * per));
        if (it == r->rotkeys.end()) r->rotkeys.emplace(g, std::move(fresh));
    }
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}
extern "C" int sfg_ring_install_relinkey_dev(sfg_ring *r, const uint64_t *round2agg, const uint64_t *h1agg) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!round2agg || !h1agg) GR_FAIL(r, "sfg_ring_install_relinkey_dev: null polynomial");
    GR_TRY(grk_fill_key(r, r->rlk, false, 1, (const u64 *)round2agg, (const u64 *)h1agg));
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}
extern "C" int sfg_ring_export_rotkey(sfg_ring *r, uint64_t g, uint64_t *key_host) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!key_host) GR_FAIL(r, "sfg_ring_export_rotkey: null output");
    const GrKey *k = nullptr;
    if (g == 1) { if (r->rlk.key) k = &r->rlk; }
    else { const auto it = r->rotkeys.find(g); if (it != r->rotkeys.end()) k = &it->second; }
    if (!k) GR_FAIL(r, "sfg_ring_export_rotkey: no key for galois element %llu", (unsigned long long)g);
    GR_HIP(r, hipMemcpyAsync(key_host, k->key, (size_t)r->beta * 2 * r->nmod * r->N * 8, hipMemcpyDeviceToHost, r->stream));
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}

extern "C" int sfg_ring_crp_fill_dev(sfg_ring *r, const uint8_t *key32, uint64_t first_row, size_t nrows, const int *mod_idx_host, uint64_t *out) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!key32 || (nrows && (!mod_idx_host || !out))) GR_FAIL(r, "sfg_ring_crp_fill_dev: null key, modulus indices or output");
    if (first_row > ~0ULL - nrows) GR_FAIL(r, "sfg_ring_crp_fill_dev: row numbers beyond 2^64");
    if (nrows > 0x7FFFFFFFu) GR_FAIL(r, "sfg_ring_crp_fill_dev: more than 2^31 - 1 rows in one call");
    for (size_t i = 0; i < nrows; i++)
        if (mod_idx_host[i] < 0 || mod_idx_host[i] >= r->nmod) GR_FAIL(r, "sfg_ring_crp_fill_dev: modulus index %d of row %zu out of range 0..%d", mod_idx_host[i], i, r->nmod - 1);
    if (!nrows) return 0;
    GR_TRY(gr_reserve(r, r->modidx, nrows * sizeof(int)));
    GR_TRY(gr_upload(r, r->modidx, mod_idx_host, nrows * sizeof(int)));
    GrkSeed key;                                    // passed by value: the ring keeps no copy of the seed
    for (int i = 0; i < 8; i++) key.k[i] = (uint32_t)key32[4 * i] | (uint32_t)key32[4 * i + 1] << 8 | (uint32_t)key32[4 * i + 2] << 16 | (uint32_t)key32[4 * i + 3] << 24;
    gr_split(nrows, kGrkLaunchRows, [&](size_t r0, size_t n) {
        hipLaunchKernelGGL(k_grk_crp, dim3(r->N / GR_T, (unsigned)n), dim3(GR_T), 0, r->stream, key, (u64)first_row + r0, (const int *)r->modidx + r0, r->modc, (u64 *)out + r0 * r->N, r->N);
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return 0;
}
