// gring_refresh.hip - the general ring's local halves of the collective bootstrap: the twins of refresh.hip's four sfg_refresh_* calls for every ring
// sfg_ring_create accepts (logN 12..16, up to 47 moduli of Q below 2^61).  mpc/mhe.go:222-376 (BootstrapMatAll, CollectiveBootstrapMat, CollectiveBootstrapVec)
// calls, per ciphertext, lattigo's dckks.RefreshProtocol: GenShares, then - after the aggregation of the shares, which stays in Go - Decrypt, Recode, Recrypt.
//
// PARITY UNPINNED, exactly as for PN14 (refresh.hip): RefreshProtocol lives in the absent fork; the semantics are lattigo v2.1.0 / v2.2.0
// dckks/refresh.go as the CPU checker under oracle/ restates them (orc_refresh_gen_shares, orc_refresh_finish and their _scaled forms).  Randomness (mask, e0,
// e1, crs) is an input: the Go side keeps drawing it.
//
//   GenShares:  h0 = NTT_level(mask + e0) + sk (.) c1        h1 = -( NTT(mask' + e1) + sk (.) crs ) over all nq moduli
//               mask' = mask, or Quo(mask Int(target), Int(ct scale)) in the target-scale form
//   finish:     x = INTT_level(c0 + sum h0) as a big integer, negative when x >= floor(Q_level / 2); the target-scale form applies Quo here; x reduced into all nq
//               moduli; c0' = NTT(x) + sum h1, c1' = crs
//
// Where the integers live.  A mask arrives coefficient-major ([N][W] limbs); Q_level reaches 2867 bits.  One workgroup is one wave of 64 lanes and owns 64
// adjacent coefficients: their 64 W limbs are one contiguous stretch, read from HBM once, coalesced, and transposed into LDS planes [limb][lane] (8 n 64 bytes, at
// most 24 KiB at n = 48 limbs; lane l reads bank pair l of every plane: conflict-free).  From there one lane owns one coefficient: it forms every residue row of its
// coefficient by Horner over the planes (rows written 512 contiguous bytes a wave) and, in the target-scale form, rescales in place.  n is what the call's integers
// occupy (grf::limbs_for), not the capacity: a PN14-sized ring runs over at most 7 limbs.  No kernel holds limbs or digits in a per-thread array.
// The unscaled recode needs no limbs: rows below the level are c0 + h0 + h1 themselves (x and x - Q agree there, and NTT(INTT(.)) is the identity on canonical
// rows), rows above it are a Horner over the mixed-radix digit rows modulo q_j, minus Q_level mod q_j for a negative x; the sign is decided once per coefficient.
// Per-coefficient arithmetic and every bound: gring_refresh_arith.hpp.  Workspace and chunks: gring_refresh_plan.hpp.  DESIGN.md section 17.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "gring_dev.hpp"
#include "gring_refresh_arith.hpp"
#include "gring_refresh_plan.hpp"

constexpr int GRF_L = 64;                                  // coefficients of a workgroup of the multi-word kernels: one wave, a coefficient a lane
static_assert(grf::kBigLimbs * GRF_L * 8 <= 32 * 1024, "the limb planes of a wave stay within 32 KiB of LDS");

// ---------------------------------------------------------------- share generation
// R0 [chunk][nl][N] = (mask + e0) mod q_j, R1 [chunk][nq][N] = (mask' + e1) mod q_j, coefficient domain.  grid (N / 64, 1, chunk), 64 threads, 8 n 64 bytes of LDS.
// Bounds: x0 + 64 <= N by the grid (N is a multiple of 64), so the tile's 64 W words lie inside the ciphertext's mask; an LDS index is li * 64 + co with li < W <= n.
template <bool SCALED>
__global__ __launch_bounds__(GRF_L) void k_grf_mask_rows(const u64 *mask, int W, int n, const int32_t *e0, const int32_t *e1, u64 *R0, u64 *R1, grf::Ratio sr,
                                                         const GrMod *modc, int nl, int nq, int N) {
    extern __shared__ u64 grf_planes[];
    u64 *a = grf_planes;
    const int lane = threadIdx.x, x0 = blockIdx.x * GRF_L, x = x0 + lane; const size_t c = blockIdx.z;
    const u64 *src = mask + (c * N + x0) * (size_t)W;
    for (int k = lane; k < GRF_L * W; k += GRF_L) { const int co = k / W, li = k - co * W; a[li * GRF_L + co] = src[k]; }
    for (int i = W; i < n; i++) a[i * GRF_L + lane] = 0;
    __syncthreads();
    auto L = [&](int i) { return a[i * GRF_L + lane]; };
    auto S = [&](int i, u64 v) { a[i * GRF_L + lane] = v; };
    const bool neg = grf::to_magnitude(W, L, S);
    const int32_t v0 = e0[c * N + x], v1 = e1[c * N + x];
    for (int j = 0; j < (SCALED ? nl : nq); j++) {
        const GrMod mc = modc[j];
        const u64 m = grf::signed_residue(grf::limbs_mod(W, L, mc.q, mc.uhi, mc.ulo), neg, mc.q);
        if (j < nl) R0[(c * nl + j) * N + x] = grf::add_small(m, v0, mc.q);
        if (!SCALED) R1[(c * nq + j) * N + x] = grf::add_small(m, v1, mc.q);
    }
    if (SCALED) {
        grf::rescale(n, L, S, sr);
        for (int j = 0; j < nq; j++) {
            const GrMod mc = modc[j];
            R1[(c * nq + j) * N + x] = grf::add_small(grf::signed_residue(grf::limbs_mod(n, L, mc.q, mc.uhi, mc.ulo), neg, mc.q), v1, mc.q);
        }
    }
}
// h [chunk][nm][N] = rows + sk (.) xr, negated when NEG; xr: row (ct, j) at ct * x_stride + j * N.  grid (N / 256, nm, chunk); x < N by the grid
template <bool NEG>
__global__ __launch_bounds__(GR_T) void k_grf_share(const u64 *rows, const u64 *sk, const u64 *xr, size_t x_stride, u64 *h, const GrMod *modc, int nm, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, j = blockIdx.y; const size_t c = blockIdx.z, w = (c * nm + j) * N + x; const GrMod mc = modc[j];
    const u64 v = gr::addmod(rows[w], gr::mulmod(sk[(size_t)j * N + x], xr[c * x_stride + (size_t)j * N + x], mc.q, mc.uhi, mc.ulo), mc.q);
    h[w] = NEG ? (v ? mc.q - v : 0) : v;
}

// ---------------------------------------------------------------- the finish
// tables of a level: qm [nq - nl][nl] (q_i mod q_j for the new moduli j), Qmod [nq - nl] (Q_level mod q_j), Q [kBigLimbs] (Q_level, zero above its top limb)
struct GrfTab { const u64 *qm, *Qmod, *Q; };
// the sign of every coefficient, once: grid (N / 256, 1, chunk); X [chunk][nl][N] digits, sgn [chunk][N] bytes
__global__ __launch_bounds__(GR_T) void k_grf_sign(const u64 *X, unsigned char *sgn, const u64 *half, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x; const u64 *col = X + (size_t)blockIdx.z * nl * N + x;
    sgn[(size_t)blockIdx.z * N + x] = grf::is_negative(nl, [&](int i) { return col[(size_t)i * N]; }, [&](int i) { return half[i]; }) ? 1 : 0;
}
// the rows of x at the moduli above the level: grid (N / 256, nq - nl, chunk); Y [chunk][nq - nl][N]
__global__ __launch_bounds__(GR_T) void k_grf_new_rows(const u64 *X, const unsigned char *sgn, u64 *Y, GrfTab t, const GrMod *modc, int nl, int nq, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, jj = blockIdx.y, ny = nq - nl; const size_t c = blockIdx.z; const u64 *col = X + c * nl * N + x;
    const GrMod mc = modc[nl + jj]; const u64 *qm = t.qm + (size_t)jj * nl;
    const u64 v = grf::digits_mod(nl, [&](int i) { return col[(size_t)i * N]; }, [&](int i) { return qm[i]; }, mc.q, mc.uhi, mc.ulo);
    Y[(c * ny + jj) * N + x] = grf::recode_new(v, sgn[c * N + x] != 0, t.Qmod[jj], mc.q);
}
// the target-scale recode: digits -> limbs in LDS planes, sign, Q - x, the rescale, every one of the nq rows.  grid (N / 64, 1, chunk), 64 threads, 8 n 64 bytes of
// LDS; Y [chunk][nq][N].  Every LDS index is i * 64 + lane with i < n.
__global__ __launch_bounds__(GRF_L) void k_grf_recode_scaled(const u64 *X, u64 *Y, GrfTab t, const u64 *half, grf::Ratio sr, const GrMod *modc, int n, int nl, int nq, int N) {
    extern __shared__ u64 grf_planes[];
    u64 *a = grf_planes;
    const int lane = threadIdx.x, x = blockIdx.x * GRF_L + lane; const size_t c = blockIdx.z; const u64 *col = X + c * nl * N + x;
    auto L = [&](int i) { return a[i * GRF_L + lane]; };
    auto S = [&](int i, u64 v) { a[i * GRF_L + lane] = v; };
    auto D = [&](int i) { return col[(size_t)i * N]; };
    grf::digits_to_limbs(nl, D, [&](int i) { return modc[i].q; }, n, L, S);
    const bool neg = grf::is_negative(nl, D, [&](int i) { return half[i]; });
    if (neg) grf::rsub(n, L, [&](int i) { return t.Q[i]; }, S);
    grf::rescale(n, L, S, sr);
    for (int j = 0; j < nq; j++) {
        const GrMod mc = modc[j];
        Y[(c * nq + j) * N + x] = grf::signed_residue(grf::limbs_mod(n, L, mc.q, mc.uhi, mc.ulo), neg, mc.q);
    }
}
// Recrypt: c0' = NTT(x) + h1agg, c1' = crs.  Row j of NTT(x) is c0 + h0agg itself for j < first_new, else row j - first_new of Y [chunk][nq - first_new][N].
// grid (N / 256, nq, chunk); out [chunk][2][nq][N]
__global__ __launch_bounds__(GR_T) void k_grf_recrypt(const u64 *ct, const u64 *h0, const u64 *Y, const u64 *h1, const u64 *crs, u64 *out, const GrMod *modc, int first_new,
                                                      int nl, int nq, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, j = blockIdx.y; const size_t c = blockIdx.z, s = (c * nq + j) * N + x, o = (c * 2 * nq + j) * N + x; const u64 q = modc[j].q;
    const u64 v = j < first_new ? gr::addmod(ct[(c * 2 * nl + j) * N + x], h0[(c * nl + j) * N + x], q) : Y[(c * (nq - first_new) + (j - first_new)) * N + x];
    out[o] = gr::addmod(v, h1[s], q);
    out[o + (size_t)nq * N] = crs[s];
}

// ---------------------------------------------------------------- host side
// Q_level in kBigLimbs limbs (it fits: at most 47 moduli below 2^61); returns its bit length
static int grf_q_limbs(const sfg_ring *r, int level, u64 *Q) {
    memset(Q, 0, sizeof(u64) * grf::kBigLimbs); Q[0] = 1;
    for (int i = 0; i <= level; i++) (void)grf::mul_add(grf::kBigLimbs, [&](int k) { return Q[k]; }, [&](int k, u64 v) { Q[k] = v; }, r->q[i], 0);
    for (int k = grf::kBigLimbs - 1; k >= 0; k--) if (Q[k]) return 64 * k + 64 - __builtin_clzll(Q[k]);
    return 0;
}
static int grf_tab(sfg_ring *r, int level, GrfTab *out) {
    const int nl = level + 1, ny = r->nq - nl;
    auto it = r->rf_tabs.find(level);
    if (it == r->rf_tabs.end()) {
        std::vector<u64> h((size_t)ny * nl + ny + grf::kBigLimbs, 0);
        u64 *qm = h.data(), *Qmod = qm + (size_t)ny * nl, *Q = Qmod + ny;
        for (int jj = 0; jj < ny; jj++) {
            const u64 qj = r->q[nl + jj]; u64 m = 1 % qj;
            for (int i = 0; i < nl; i++) { qm[(size_t)jj * nl + i] = r->q[i] % qj; m = hm_mul(m, r->q[i] % qj, qj); }
            Qmod[jj] = m;
        }
        (void)grf_q_limbs(r, level, Q);
        GrBuf<u64> d; GR_TRY(gr_table(r, d, h.data(), h.size() * 8));
        it = r->rf_tabs.emplace(level, std::move(d)).first;
    }
    const u64 *d = it->second;
    out->qm = d; out->Qmod = d + (size_t)ny * nl; out->Q = out->Qmod + ny;
    return 0;
}
// the scale pair of a target-scale call: *scaled = false when the two scales are equal (Quo(v x, x) = v: the unscaled kernels, as PN14 takes them)
static int grf_ratio(sfg_ring *r, const char *what, int level, double ct_scale, double target_scale, grf::Ratio &sr, int &q_bits, bool *scaled) {
    if (!grf::scale_ok(ct_scale) || !grf::scale_ok(target_scale))
        GR_FAIL(r, "%s: scales %g, %g must be finite, at least 1 and at most 2^400", what, ct_scale, target_scale);
    *scaled = ct_scale != target_scale;
    if (!*scaled) return 0;
    sr = grf::scale_ratio(ct_scale, target_scale);
    u64 Q[grf::kBigLimbs]; q_bits = grf_q_limbs(r, level, Q);
    if (!grf::fits_q(q_bits, sr.sh))
        GR_FAIL(r, "%s: Q_level (%d bits) times the target scale over the ciphertext scale (shift %d) does not fit %d bits", what, q_bits, sr.sh, grf::kBigBits);
    return 0;
}

static int grf_gen_shares(sfg_ring *r, const char *what, const u64 *ct, int nct, int level, const u64 *crs, const u64 *mask, int W, const int32_t *e0, const int32_t *e1,
                          u64 *h0, u64 *h1, const double *scales) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(gr_check_level(r, what, nct, level));
    if (!r->io.sk) GR_FAIL(r, "%s: no secret-key shard loaded (sfg_ring_load_secret_key)", what);
    if (W < 1 || W > grf::kBigLimbs) GR_FAIL(r, "%s: mask limb count %d out of range 1..%d", what, W, grf::kBigLimbs);
    grf::Ratio sr{1, 1, 0}; bool scaled = false; int q_bits = 0;
    if (scales) {
        GR_TRY(grf_ratio(r, what, level, scales[0], scales[1], sr, q_bits, &scaled));
        // the kernel multiplies the W-limb magnitude by the target's mantissa and shifts it inside the capacity: a mask wider than Q_level must fit as well
        if (scaled && !grf::fits_mask(W, sr.sh)) GR_FAIL(r, "%s: a %d-limb mask times the target scale (shift %d) does not fit %d bits", what, W, sr.sh, grf::kBigBits);
    }
    if (nct == 0) return 0;
    if (!ct || !crs || !mask || !e0 || !e1 || !h0 || !h1) GR_FAIL(r, "%s: null ciphertexts, reference polynomials, masks, errors or output", what);
    const int nl = level + 1, nq = r->nq, N = r->N;
    const int n = scaled ? grf::limbs_for(64 * W, sr.sh) : W;                       // <= kBigLimbs by fits_mask
    const GrfPlan plan = grf_shares_plan((size_t)nct, nl, nq, (size_t)N, r->io.ws_budget);
    GR_TRY(gr_reserve(r, r->io.ws, plan.reserve()));
    const GrfSharesLayout lay = grf_shares_layout(nl, nq, (size_t)N, plan.chunk);
    u64 *R0 = (u64 *)r->io.ws.p + lay.R0, *R1 = (u64 *)r->io.ws.p + lay.R1;
    const size_t lds = (size_t)n * GRF_L * 8; const unsigned gx = N / GR_T;
    for (size_t c = 0; c < plan.nchunks; c++) {
        const size_t c0 = plan.first(c), nb = plan.count(c, (size_t)nct);
        const dim3 gm(N / GRF_L, 1, (unsigned)nb);
        if (scaled) hipLaunchKernelGGL(k_grf_mask_rows<true>, gm, dim3(GRF_L), lds, r->stream, mask + c0 * N * W, W, n, e0 + c0 * N, e1 + c0 * N, R0, R1, sr, r->modc, nl, nq, N);
        else hipLaunchKernelGGL(k_grf_mask_rows<false>, gm, dim3(GRF_L), lds, r->stream, mask + c0 * N * W, W, n, e0 + c0 * N, e1 + c0 * N, R0, R1, sr, r->modc, nl, nq, N);
        GR_HIP(r, hipGetLastError());
        GR_TRY(gr_transform(r, R0, nb * nl, gr_map(nl, nl, 0, 0), false));
        GR_TRY(gr_transform(r, R1, nb * nq, gr_map(nq, nq, 0, 0), false));
        hipLaunchKernelGGL(k_grf_share<false>, dim3(gx, nl, (unsigned)nb), dim3(GR_T), 0, r->stream, (const u64 *)R0, r->io.sk, ct + c0 * 2 * nl * N + (size_t)nl * N, (size_t)2 * nl * N,
                           h0 + c0 * nl * N, r->modc, nl, N);
        hipLaunchKernelGGL(k_grf_share<true>, dim3(gx, nq, (unsigned)nb), dim3(GR_T), 0, r->stream, (const u64 *)R1, r->io.sk, crs + c0 * nq * N, (size_t)nq * N,
                           h1 + c0 * nq * N, r->modc, nq, N);
        GR_HIP(r, hipGetLastError());
    }
    return 0;
}
static int grf_finish(sfg_ring *r, const char *what, const u64 *ct, int nct, int level, const u64 *h0agg, const u64 *h1agg, const u64 *crs, u64 *out, const double *scales) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(gr_check_level(r, what, nct, level));
    grf::Ratio sr{1, 1, 0}; bool scaled = false; int q_bits = 0;
    if (scales) GR_TRY(grf_ratio(r, what, level, scales[0], scales[1], sr, q_bits, &scaled));
    if (nct == 0) return 0;
    if (!ct || !h0agg || !h1agg || !crs || !out) GR_FAIL(r, "%s: null ciphertexts, shares, reference polynomials or output", what);
    const int nl = level + 1, nq = r->nq, N = r->N, ny = grf_new_rows(nl, nq, scaled), first_new = nq - ny;
    const int n = scaled ? grf::limbs_for(q_bits, sr.sh) : 0;                        // <= kBigLimbs by fits_q, and at least the limbs of Q_level
    const GrfPlan plan = grf_finish_plan((size_t)nct, nl, nq, scaled, (size_t)N, r->io.ws_budget);
    GriDecTab dtab{}; GrfTab tab{};
    if (ny) {                                                                        // ny == 0: the unscaled form at the top level has no new modulus and needs no digit
        GR_TRY(gri_dec_tab(r, level, &dtab));
        GR_TRY(grf_tab(r, level, &tab));
        GR_TRY(gr_reserve(r, r->io.ws, plan.reserve()));
    }
    const GrfFinishLayout lay = grf_finish_layout(nl, nq, scaled, (size_t)N, plan.chunk);
    u64 *X = (u64 *)r->io.ws.p + lay.X, *Y = (u64 *)r->io.ws.p + lay.Y; unsigned char *sgn = (unsigned char *)((u64 *)r->io.ws.p + lay.S);
    const unsigned gx = N / GR_T;
    for (size_t c = 0; c < plan.nchunks; c++) {
        const size_t c0 = plan.first(c), nb = plan.count(c, (size_t)nct);
        const u64 *ctc = ct + c0 * 2 * nl * N, *h0c = h0agg + c0 * nl * N;
        if (ny) {
            GR_TRY(gri_add_c0(r, ctc, h0c, X, (int)nb, level));                      // Decrypt: c0 + sum h0 ...
            GR_TRY(gri_digits_inplace(r, X, (int)nb, level, dtab));                  // ... to the coefficient domain and on to mixed-radix digits (nl == 1: no Garner launch)
            if (scaled) hipLaunchKernelGGL(k_grf_recode_scaled, dim3(N / GRF_L, 1, (unsigned)nb), dim3(GRF_L), (size_t)n * GRF_L * 8, r->stream, (const u64 *)X, Y, tab, dtab.half, sr,
                                           r->modc, n, nl, nq, N);
            else {
                hipLaunchKernelGGL(k_grf_sign, dim3(gx, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, (const u64 *)X, sgn, dtab.half, nl, N);
                hipLaunchKernelGGL(k_grf_new_rows, dim3(gx, ny, (unsigned)nb), dim3(GR_T), 0, r->stream, (const u64 *)X, (const unsigned char *)sgn, Y, tab, r->modc, nl, nq, N);
            }
            GR_HIP(r, hipGetLastError());
            GR_TRY(gr_transform(r, Y, nb * ny, gr_map(ny, ny, first_new, 0), false));
        }
        hipLaunchKernelGGL(k_grf_recrypt, dim3(gx, nq, (unsigned)nb), dim3(GR_T), 0, r->stream, ctc, h0c, (const u64 *)Y, h1agg + c0 * nq * N, crs + c0 * nq * N, out + c0 * 2 * nq * N,
                           r->modc, first_new, nl, nq, N);
        GR_HIP(r, hipGetLastError());
    }
    return 0;
}

// ---------------------------------------------------------------- C-ABI
extern "C" int sfg_ring_refresh_gen_shares_dev(sfg_ring *r, const uint64_t *ct, int nct, int level, const uint64_t *crs, const uint64_t *mask, int mask_limbs, const int32_t *e0,
                                               const int32_t *e1, uint64_t *h0, uint64_t *h1) {
    return grf_gen_shares(r, "sfg_ring_refresh_gen_shares_dev", (const u64 *)ct, nct, level, (const u64 *)crs, (const u64 *)mask, mask_limbs, e0, e1, (u64 *)h0, (u64 *)h1, nullptr);
}
extern "C" int sfg_ring_refresh_gen_shares_scaled_dev(sfg_ring *r, const uint64_t *ct, int nct, int level, double ct_scale, double target_scale, const uint64_t *crs,
                                                      const uint64_t *mask, int mask_limbs, const int32_t *e0, const int32_t *e1, uint64_t *h0, uint64_t *h1) {
    const double s[2] = {ct_scale, target_scale};
    return grf_gen_shares(r, "sfg_ring_refresh_gen_shares_scaled_dev", (const u64 *)ct, nct, level, (const u64 *)crs, (const u64 *)mask, mask_limbs, e0, e1, (u64 *)h0, (u64 *)h1, s);
}
extern "C" int sfg_ring_refresh_finish_dev(sfg_ring *r, const uint64_t *ct, int nct, int level, const uint64_t *h0agg, const uint64_t *h1agg, const uint64_t *crs, uint64_t *out) {
    return grf_finish(r, "sfg_ring_refresh_finish_dev", (const u64 *)ct, nct, level, (const u64 *)h0agg, (const u64 *)h1agg, (const u64 *)crs, (u64 *)out, nullptr);
}
extern "C" int sfg_ring_refresh_finish_scaled_dev(sfg_ring *r, const uint64_t *ct, int nct, int level, double ct_scale, double target_scale, const uint64_t *h0agg,
                                                  const uint64_t *h1agg, const uint64_t *crs, uint64_t *out) {
    const double s[2] = {ct_scale, target_scale};
    return grf_finish(r, "sfg_ring_refresh_finish_scaled_dev", (const u64 *)ct, nct, level, (const u64 *)h0agg, (const u64 *)h1agg, (const u64 *)crs, (u64 *)out, s);
}
