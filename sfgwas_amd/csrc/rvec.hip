// rvec.hip — secret shares to CKKS plaintexts and back: the ring-vector encoder and decoder that MPC.SSToCMat and MPC.CMatToSS call on the lattigo fork
// (encoder.EncodeRVecNew, mpc/ss.go:125; encoder.DecodeRVec, ss.go:260,264).
//
// PARITY UNPINNED against the fork's EncodeRVecNew / DecodeRVec: the fork's source is not published.  What the two functions compute is fixed by their call sites
// and by linearity; it is stated here exactly and pinned against that statement (tests/rvec_ref.py, tests/test_gpu_rvec.py).
//
// N = 2^14, n = N/2 slots, zeta = exp(2 pi i / 2N), slot t <-> 5^t = 4 m_t + 1 (mod 2N).  A field element is `limbs` (2 or 4) little-endian 64-bit words, a canonical
// residue of the odd modulus p, plain; centre(x) = x for x <= (p - 1)/2, else x - p.  scale = mant 2^exp is a finite double >= 1 taken exactly, f = frac_bits.
//   encode:  s_t = centre(x_t) (0 for t >= n_elem),  w_c = (1/n) sum_t s_t zeta^(-5^t c),  p_c = round(scale 2^-f Re w_c),  p_{c+n} = round(scale 2^-f Im w_c),
//            out = NTT rows of p mod q_0..q_level
//   decode:  p_c = centred CRT integer of the INTT of the rows (lattigo's Cmp(QHalf) rule, recode.hpp),  v_t = sum_c (p_c + i p_{c+n}) zeta^(5^t c),
//            r_t = round(2^f / scale Re v_t) mod p
// With 5^t = 4 m + 1 both sums are length-n DFTs (kernel omega^(-/+ m c), omega = zeta^4) behind a twist by zeta^(-/+ c):
//   encode:  u_{m_t} = s_t,  X = DFT-(u),  w_c = zeta^-c X_c / n            decode:  a_c = (p_c + i p_{c+n}) zeta^c,  V = DFT+(a),  v_t = V_{m_t}
//
// The numbers are far too wide for floating point (shares are uniform in a 128- or 256-bit field, the decoded value must be right to one unit modulo p), so the
// transform is FIXED POINT: a real number is a two's-complement integer of W 64-bit words with g fractional bits, W and g chosen per call by rvec_host.hpp from
// the field, the level, the scale and f.  No floating point touches a value between the input words and the output words (the Garner digits of the decoder are
// exact integers held in doubles, as everywhere in this library).
//   * a product by a twiddle is sign-magnitude: the full 2W-word product of the magnitudes, shifted down by the twiddle's 64 W - 2 fractional bits, truncated once;
//   * twiddles zeta^j, j < N, live in ONE table per root context at 9 words (574 fractional bits), built by k_rvec_table from the 14 committed base roots
//     exp(i pi / 2^k) (rvec_roots.hpp) by at most 13 truncating products along the bits of j; a kernel at width W reads the top W words of an entry;
//   * the 13 radix-2 stages run as two passes through HBM over sets of 256 points that are closed under the stages of the pass: pass 0 = stages 1..7 on 256
//     consecutive points (two 128-point sub-transforms), pass 1 = stages 8..13 on 64 x 4 points (rows 128 apart, 4 consecutive columns).  The bit reversal is the
//     pre-pass's store address, the twist is inside the pre-pass (decode) or the post-pass (encode), the slot permutation is the pre-pass's (encode) or the
//     post-pass's (decode) address: no pass of its own for any of them;
//   * HBM and LDS images are limb-planar, [re, im][word][point]: the loads of one word by a wave are consecutive.
// Scratch, from the context's pool and per ciphertext of a chunk (rvec_batch_plan, batch_plan.hpp): 2 W 65,536 B ("rvec.fft") + (level + 1) 131,072 B ("rvec.coef").
//
// Error, in units of 2^-g (derivation: DESIGN.md 12).  A complex product truncates two real products per component: below 2 units per component, 2 sqrt 2 in modulus.
// Point errors add through the butterflies with unit gain, so an output collects the truncations of every product of its tree, the twist's included: fewer than
// 2^14 products, below 2^15.5 units.  A twiddle is off by less than 2^-(64W-3) per component; the operands of stage s have modulus at most 2^s A (A the largest
// input modulus, 2^13 A 2^g < 2^(64W-1)) and an output collects 2^(13-s) of them: below 12 units per stage, 2^7.2 in all.  Together below 2^16 units.
// g = 48 + (log2 of the output units per transform unit, when positive), so the value that is finally rounded is within 2^-32 of the exact one in units of the
// output; the final scaling and rounding are exact integer arithmetic on that value (rvec_fx.hpp: the arithmetic and the per-element work of every kernel, host and
// device, which tests/host/host_rvec_test.cpp runs over whole transforms on the CPU).
#include "common.hpp"
#include "kernels.hpp"
#include "recode.hpp"
#include "rvec_fx.hpp"

constexpr int RV_N = SFG_N, RV_n = SFG_SLOTS, RV_TWN = SFG_N;       // table entries: zeta^j, j < N
struct RvecTables { u64 *tw = nullptr; uint16_t *slot_m = nullptr; };     // tw [2][9][N] (re, im planes, word planes); slot_m[t] = (5^t - 1)/4 mod n

// the top W words of table entry j (the value at 64 W - 2 fractional bits, rounded down); conj: the conjugate
template <int W> __device__ __forceinline__ void tw_load(const u64 *tw, int j, bool conj, u64 (&tr)[W], u64 (&ti)[W]) {
#pragma unroll
    for (int k = 0; k < W; k++) {
        tr[k] = tw[(size_t)(RVEC_TW_LIMBS - W + k) * RV_TWN + j];
        ti[k] = tw[(size_t)(RVEC_TW_LIMBS + RVEC_TW_LIMBS - W + k) * RV_TWN + j];
    }
    if (conj) fx_negate<W>(ti);
}
__device__ __forceinline__ int brev13(int x) { return (int)(__brev((unsigned)x) >> 19); }

// ---------------------------------------------------------------- the table zeta^j, j < N, from the base roots: one entry per thread.  grid N / 64
__global__ void __launch_bounds__(64) k_rvec_table(const u64 *roots, u64 *tw) {
    constexpr int T = RVEC_TW_LIMBS;
    const int j = blockIdx.x * 64 + threadIdx.x;
    u64 ar[T], ai[T];
    rvec_table_entry(roots, j, ar, ai);
#pragma unroll
    for (int k = 0; k < T; k++) { tw[(size_t)k * RV_TWN + j] = ar[k]; tw[(size_t)(T + k) * RV_TWN + j] = ai[k]; }
}

// ---------------------------------------------------------------- one pass of the transform: 256 points per workgroup, in place
// buf [nct][2][W][n].  PASS 0: points b*256 + l, stages with half 1..64;  PASS 1: points (l >> 2) * 128 + b * 4 + (l & 3), stages with half 128..4096 (local half
// 4..128).  Input in bit-reversed order, output in natural order; twiddle of the butterfly at position k of a stage with half H: zeta^(+/- k N / H).  grid (32, nct)
template <int W, int PASS>
__global__ void __launch_bounds__(128) k_rvec_fft(u64 *buf, const u64 *tw, int conj) {
    __shared__ u64 s[2 * W * 256];
    const int tid = threadIdx.x, b = blockIdx.x;
    u64 *base = buf + (size_t)blockIdx.y * (2 * W * RV_n);
    auto gidx = [&](int l) { return PASS == 0 ? b * 256 + l : ((l >> 2) * 128 + b * 4 + (l & 3)); };
#pragma unroll
    for (int pw = 0; pw < 2 * W; pw++) {
        s[pw * 256 + tid] = base[(size_t)pw * RV_n + gidx(tid)];
        s[pw * 256 + tid + 128] = base[(size_t)pw * RV_n + gidx(tid + 128)];
    }
    __syncthreads();
    for (int hl = (PASS == 0 ? 1 : 4); hl <= (PASS == 0 ? 64 : 128); hl <<= 1) {
        const int i0 = ((tid & ~(hl - 1)) << 1) | (tid & (hl - 1)), i1 = i0 + hl;
        const int H = PASS == 0 ? hl : hl * 32;
        const int j = (gidx(i0) & (H - 1)) * (RV_TWN / H);
        u64 tr[W], ti[W], ar[W], ai[W], br[W], bi[W];
        tw_load<W>(tw, j, conj != 0, tr, ti);
#pragma unroll
        for (int k = 0; k < W; k++) { ar[k] = s[k * 256 + i0]; ai[k] = s[(W + k) * 256 + i0]; br[k] = s[k * 256 + i1]; bi[k] = s[(W + k) * 256 + i1]; }
        rvec_butterfly<W>(ar, ai, br, bi, tr, ti);
#pragma unroll
        for (int k = 0; k < W; k++) { s[k * 256 + i0] = ar[k]; s[(W + k) * 256 + i0] = ai[k]; s[k * 256 + i1] = br[k]; s[(W + k) * 256 + i1] = bi[k]; }
        __syncthreads();
    }
#pragma unroll
    for (int pw = 0; pw < 2 * W; pw++) {
        base[(size_t)pw * RV_n + gidx(tid)] = s[pw * 256 + tid];
        base[(size_t)pw * RV_n + gidx(tid + 128)] = s[pw * 256 + tid + 128];
    }
}

// ---------------------------------------------------------------- encode, pre-pass: centre mod p, place the binary point, scatter to the transform's input order
// share [nct][n_elem][limbs] -> buf [nct][2][W][n]: slot t goes to point brev13(m_t); slots >= n_elem and every imaginary part are zero.  grid (n / 256, nct)
template <int W>
__global__ void __launch_bounds__(256) k_rvec_enc_pre(const u64 *share, RvecField f, int n_elem, int g, const uint16_t *slot_m, u64 *buf) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    u64 x[4] = {0, 0, 0, 0}, v[W];
    if (t < n_elem) {
        const u64 *src = share + ((size_t)blockIdx.y * n_elem + t) * f.limbs;
        for (int i = 0; i < f.limbs; i++) x[i] = src[i];
    }
    rvec_centre_place<W>(x, f, g, v);
    u64 *base = buf + (size_t)blockIdx.y * (2 * W * RV_n);
    const int pos = brev13(slot_m[t]);
#pragma unroll
    for (int k = 0; k < W; k++) { base[(size_t)k * RV_n + pos] = v[k]; base[(size_t)(W + k) * RV_n + pos] = 0; }
}

// ---------------------------------------------------------------- encode, post-pass: twist by zeta^-c, times mant 2^-shift, round, reduce mod q_0..q_level
// buf -> coef [nct][nl][N] canonical coefficient words (c and c + n from one thread).  grid (n / 256, nct)
template <int W>
__global__ void __launch_bounds__(256) k_rvec_enc_post(const u64 *buf, const u64 *tw, u64 mant, int shift, int nl, const ModConst *modc, u64 *coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const u64 *base = buf + (size_t)blockIdx.y * (2 * W * RV_n);
    u64 xr[W], xi[W], tr[W], ti[W], yr[W], yi[W];
#pragma unroll
    for (int k = 0; k < W; k++) { xr[k] = base[(size_t)k * RV_n + c]; xi[k] = base[(size_t)(W + k) * RV_n + c]; }
    tw_load<W>(tw, c, true, tr, ti);
    fx_cmul<W>(xr, xi, tr, ti, yr, yi);
    u64 rd[2][W + 1];
    const bool neg0 = rvec_scale_round<W>(yr, mant, shift, rd[0]), neg1 = rvec_scale_round<W>(yi, mant, shift, rd[1]);
    for (int i = 0; i < nl; i++) {
        const u64 q = modc[i].qi;
        u64 *row = coef + ((size_t)blockIdx.y * nl + i) * RV_N;
        row[c] = rvec_mod_q<W + 1>(rd[0], neg0, q);
        row[c + RV_n] = rvec_mod_q<W + 1>(rd[1], neg1, q);
    }
}

// ---------------------------------------------------------------- decode, pre-pass: centred CRT integer, binary point, twist by zeta^c, bit-reversed store
// xin [nct][nl][N] coefficient-domain residues -> buf.  grid (n / 256, nct)
template <int W>
__global__ void __launch_bounds__(256) k_rvec_dec_pre(const u64 *xin, RecodeConst rc, const ModConst *modc, const u64 *tw, int g, u64 *buf) {
    const int c = blockIdx.x * 256 + threadIdx.x, nl = rc.nl;
    u64 p[2][W];
    for (int part = 0; part < 2; part++) {
        double v[RF_MAXL], r[RF_MAXL];
        for (int i = 0; i < nl; i++) r[i] = u64_to_f64(xin[((size_t)blockIdx.y * nl + i) * RV_N + c + part * RV_n]);
        garner_digits(r, v, nl, rc, modc);
        const bool neg = garner_negative(v, nl, rc);
        if (neg) {          // Q - x in the digits: complement plus one with the carry walked up (decrypt.hip k_dec_coeffs)
            double carry = 1.0;
            for (int i = 0; i < nl; i++) {
                const double q = modc[i].q, m = (q - 1.0 - v[i]) + carry;
                carry = m == q ? 1.0 : 0.0;
                v[i] = m == q ? 0.0 : m;
            }
        }
        u64 dg[RF_MAXL], qs[RF_MAXL];
        for (int i = 0; i < nl; i++) { dg[i] = f64_to_u64(v[i]); qs[i] = modc[i].qi; }
        rvec_from_digits<W>(dg, qs, nl, neg, g, p[part]);
    }
    u64 tr[W], ti[W], yr[W], yi[W];
    tw_load<W>(tw, c, false, tr, ti);
    fx_cmul<W>(p[0], p[1], tr, ti, yr, yi);
    u64 *base = buf + (size_t)blockIdx.y * (2 * W * RV_n);
    const int pos = brev13(c);
#pragma unroll
    for (int k = 0; k < W; k++) { base[(size_t)k * RV_n + pos] = yr[k]; base[(size_t)(W + k) * RV_n + pos] = yi[k]; }
}

// ---------------------------------------------------------------- decode, post-pass: r_t = round(2^f / scale Re V_{m_t}) mod p.  out [nct][n_elem][limbs].  grid (n / 256, nct)
template <int W>
__global__ void __launch_bounds__(256) k_rvec_dec_post(const u64 *buf, const uint16_t *slot_m, int n_elem, u64 mant, int shift, RvecField f, u64 *out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_elem) return;
    const u64 *base = buf + (size_t)blockIdx.y * (2 * W * RV_n);
    const int m = slot_m[t];
    u64 y[W], r[4];
#pragma unroll
    for (int k = 0; k < W; k++) y[k] = base[(size_t)k * RV_n + m];
    rvec_div_mod_p<W>(y, mant, shift, f, r);
    u64 *dst = out + ((size_t)blockIdx.y * n_elem + t) * f.limbs;
    for (int i = 0; i < f.limbs; i++) dst[i] = r[i];
}

// out = (a ? a : 0) - b mod p over cnt field elements
__global__ void __launch_bounds__(256) k_rvec_field_sub(const u64 *a, const u64 *b, u64 *out, RvecField f, size_t cnt) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    u64 x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0}, d[4];
    for (int i = 0; i < f.limbs; i++) { if (a) x[i] = a[e * f.limbs + i]; y[i] = b[e * f.limbs + i]; }
    rvec_field_sub(x, y, f, d);
    for (int i = 0; i < f.limbs; i++) out[e * f.limbs + i] = d[i];
}

// ---------------------------------------------------------------- host side
int sfg_rvec_init(sfg_ctx *ctx) {
    RvecTables *rt = new RvecTables();
    ctx->sh->rvec_tables = rt;
    constexpr int T = RVEC_TW_LIMBS;
    std::vector<u64> roots((size_t)14 * 2 * T);
    rvec_host_roots(roots.data());
    std::vector<uint16_t> sm(RV_n);
    u64 g = 1;
    for (int t = 0; t < RV_n; t++) { sm[t] = (uint16_t)(((g - 1) / 4) % RV_n); g = (g * 5) % (2ULL * RV_N); }
    DevMem roots_dev;                                           // the base roots: needed until the table is built
    SFG_HIP(ctx, hipMalloc(&rt->tw, (size_t)2 * T * RV_TWN * 8));
    SFG_HIP(ctx, hipMalloc(&rt->slot_m, RV_n * sizeof(uint16_t)));
    SFG_HIP(ctx, hipMalloc(&roots_dev.h, roots.size() * 8));
    SFG_HIP(ctx, hipMemcpy(roots_dev.h, roots.data(), roots.size() * 8, hipMemcpyHostToDevice));
    SFG_HIP(ctx, hipMemcpy(rt->slot_m, sm.data(), RV_n * sizeof(uint16_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rvec_table, dim3(RV_TWN / 64), dim3(64), 0, 0, (const u64 *)roots_dev.h, rt->tw);
    SFG_HIP(ctx, hipGetLastError());
    SFG_HIP(ctx, hipDeviceSynchronize());
    return 0;
}
void sfg_rvec_destroy(SfgShared *sh) {
    RvecTables *rt = (RvecTables *)sh->rvec_tables;
    if (!rt) return;
    (void)hipFree(rt->tw); (void)hipFree(rt->slot_m);
    delete rt; sh->rvec_tables = nullptr;
}

#define RVEC_BY_W(W_, ...) do { switch (W_) { case 2: { constexpr int W = 2; __VA_ARGS__; } break; case 3: { constexpr int W = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int W = 4; __VA_ARGS__; } break; case 5: { constexpr int W = 5; __VA_ARGS__; } break; case 6: { constexpr int W = 6; __VA_ARGS__; } break; \
    case 7: { constexpr int W = 7; __VA_ARGS__; } break; case 8: { constexpr int W = 8; __VA_ARGS__; } break; default: SFG_FAIL(ctx, "rvec: no kernel for %d words", W_); } } while (0)

template <int W> static void rvec_fft_launch(sfg_ctx *ctx, u64 *buf, const u64 *tw, int nb, int conj) {
    hipLaunchKernelGGL((k_rvec_fft<W, 0>), dim3(32, nb), dim3(128), 0, ctx->stream, buf, tw, conj);
    hipLaunchKernelGGL((k_rvec_fft<W, 1>), dim3(32, nb), dim3(128), 0, ctx->stream, buf, tw, conj);
}

// encoder.EncodeRVecNew (mpc/ss.go:125)
extern "C" int sfg_rvec_encode_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *share_dev, int n_elem, int nct, int level, double scale,
                                   int frac_bits, uint64_t *pt_dev) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    RvecPlan pl;
    if (const char *e = rvec_plan_encode(limbs, modulus_host, (const uint64_t *)ctx->q, ctx->nq, n_elem, level, scale, frac_bits, pl)) SFG_FAIL(ctx, "rvec_encode: %s", e);
    SFG_TRY(check_level_count(ctx, "rvec_encode", nct, level, 0));
    if (!nct) return 0;
    if (!share_dev || !pt_dev) SFG_FAIL(ctx, "rvec_encode: NULL shares or output");
    ApiScope scope(ctx);
    const RvecTables *rt = (const RvecTables *)ctx->sh->rvec_tables;
    RvecField f; rvec_field(limbs, modulus_host, f);
    const int nl = level + 1;
    const RvecWords rw = rvec_words(pl.W, nl, (size_t)RV_N);
    const BatchPlan plan = rvec_batch_plan(nct, rw);
    void *bp = nullptr, *cp = nullptr;
    SFG_TRY(sfg_scratch(ctx, "rvec.fft", plan.bytes_of(rw.fft), &bp));
    SFG_TRY(sfg_scratch(ctx, "rvec.coef", plan.bytes_of(rw.coef), &cp));
    u64 *buf = (u64 *)bp, *coef = (u64 *)cp;
    const ModPattern p0 = mod_pattern_run(0, nl);
    PhaseTimer timer(ctx, "rvec_encode");
    int launches = 0;
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct);
        const u64 *src = (const u64 *)share_dev + (size_t)c0 * n_elem * limbs;
        RVEC_BY_W(pl.W, {
            hipLaunchKernelGGL(k_rvec_enc_pre<W>, dim3(RV_n / 256, nb), dim3(256), 0, ctx->stream, src, f, n_elem, pl.g, (const uint16_t *)rt->slot_m, buf);
            rvec_fft_launch<W>(ctx, buf, rt->tw, nb, 1);
            hipLaunchKernelGGL(k_rvec_enc_post<W>, dim3(RV_n / 256, nb), dim3(256), 0, ctx->stream, (const u64 *)buf, (const u64 *)rt->tw, (u64)pl.sc.mant, pl.shift, nl,
                               (const ModConst *)ctx->modc, coef);
        });
        SFG_HIP(ctx, hipGetLastError());
        SFG_TRY(launch_ntt_fwd(ctx, coef, (u64 *)pt_dev + (size_t)c0 * nl * RV_N, (size_t)nb * nl, p0));
        launches += 5;
    }
    timer.stop(launches);
    return 0;
}

// the decryption front end (decrypt.hip: INTT of the rows, or of c0 + h0agg) and the decoder, for nct plaintexts, in the chunks of rvec_batch_plan
static int rvec_decode_run(sfg_ctx *ctx, const char *what, const DecSrc &src, const RvecPlan &pl, const RvecField &f, int nct, int level, int n_elem, u64 *out) {
    ApiScope scope(ctx);
    const RvecTables *rt = (const RvecTables *)ctx->sh->rvec_tables;
    const int nl = level + 1;
    SFG_TRY(check_level_count(ctx, what, nct, level, RF_MAXL));
    const RvecWords rw = rvec_words(pl.W, nl, (size_t)RV_N);
    const BatchPlan plan = rvec_batch_plan(nct, rw);
    void *bp = nullptr, *cp = nullptr;
    SFG_TRY(sfg_scratch(ctx, "rvec.fft", plan.bytes_of(rw.fft), &bp));
    SFG_TRY(sfg_scratch(ctx, "rvec.coef", plan.bytes_of(rw.coef), &cp));
    u64 *buf = (u64 *)bp, *x = (u64 *)cp;
    RecodeConst rc; recode_constants(ctx, level, rc);
    PhaseTimer timer(ctx, "rvec_decode");
    int launches = 0;
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct);
        SFG_TRY(launch_dec_front(ctx, src, c0, nb, nl, x, &launches));
        RVEC_BY_W(pl.W, {
            hipLaunchKernelGGL(k_rvec_dec_pre<W>, dim3(RV_n / 256, nb), dim3(256), 0, ctx->stream, (const u64 *)x, rc, (const ModConst *)ctx->modc, (const u64 *)rt->tw, pl.g, buf);
            rvec_fft_launch<W>(ctx, buf, rt->tw, nb, 0);
            hipLaunchKernelGGL(k_rvec_dec_post<W>, dim3(RV_n / 256, nb), dim3(256), 0, ctx->stream, (const u64 *)buf, (const uint16_t *)rt->slot_m, n_elem, (u64)pl.sc.mant, pl.shift, f,
                               out + (size_t)c0 * n_elem * f.limbs);
        });
        SFG_HIP(ctx, hipGetLastError());
        launches += 5;
    }
    timer.stop(launches);
    return 0;
}

// encoder.DecodeRVec (mpc/ss.go:260,264)
extern "C" int sfg_rvec_decode_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *pt_dev, size_t pt_stride, int nct, int level, double scale,
                                   int frac_bits, int n_elem, uint64_t *out_dev) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    RvecPlan pl;
    if (const char *e = rvec_plan_decode(limbs, modulus_host, (const uint64_t *)ctx->q, ctx->nq, n_elem, level, scale, frac_bits, pl)) SFG_FAIL(ctx, "rvec_decode: %s", e);
    SFG_TRY(check_level_count(ctx, "rvec_decode", nct, level, 0));
    if (pt_stride < (size_t)(level + 1) * RV_N) SFG_FAIL(ctx, "rvec_decode: plaintext stride %zu below (level + 1) * N", pt_stride);
    if (!nct) return 0;
    if (!pt_dev || !out_dev) SFG_FAIL(ctx, "rvec_decode: NULL plaintexts or output");
    RvecField f; rvec_field(limbs, modulus_host, f);
    return rvec_decode_run(ctx, "rvec_decode", DecSrc::rows((const u64 *)pt_dev, pt_stride), pl, f, nct, level, n_elem, (u64 *)out_dev);
}

// mpc/ss.go:239-279: KeySwitch + Plaintext() on the hub, DecodeRVec of the result and of NTT(mask), the field subtraction
extern "C" int sfg_ckks_to_ss_finish_dev(sfg_ctx *ctx, int limbs, const uint64_t *modulus_host, const uint64_t *ct_dev, int nct, int level, double scale, int frac_bits,
                                         const uint64_t *h0agg_dev, const uint64_t *mask_ntt_dev, int is_hub, int n_elem, uint64_t *out_dev) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    RvecPlan pl;
    if (const char *e = rvec_plan_decode(limbs, modulus_host, (const uint64_t *)ctx->q, ctx->nq, n_elem, level, scale, frac_bits, pl)) SFG_FAIL(ctx, "ckks_to_ss_finish: %s", e);
    SFG_TRY(check_level_count(ctx, "ckks_to_ss_finish", nct, level, 0));
    if (!nct) return 0;
    if (!mask_ntt_dev || !out_dev || (is_hub && (!ct_dev || !h0agg_dev))) SFG_FAIL(ctx, "ckks_to_ss_finish: NULL ciphertexts, shares, masks or output");
    ApiScope scope(ctx);
    RvecField f; rvec_field(limbs, modulus_host, f);
    const size_t cnt = (size_t)nct * n_elem;
    void *ap = nullptr, *mp = nullptr;
    SFG_TRY(sfg_scratch(ctx, "rvec.mask", cnt * limbs * 8, &mp));
    SFG_TRY(rvec_decode_run(ctx, "ckks_to_ss_finish", DecSrc::rows((const u64 *)mask_ntt_dev, (size_t)(level + 1) * RV_N), pl, f, nct, level, n_elem, (u64 *)mp));
    if (is_hub) {
        SFG_TRY(sfg_scratch(ctx, "rvec.hub", cnt * limbs * 8, &ap));
        SFG_TRY(rvec_decode_run(ctx, "ckks_to_ss_finish", DecSrc::finish((const u64 *)ct_dev, (const u64 *)h0agg_dev), pl, f, nct, level, n_elem, (u64 *)ap));
    }
    hipLaunchKernelGGL(k_rvec_field_sub, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, (const u64 *)ap, (const u64 *)mp, (u64 *)out_dev, f, cnt);
    SFG_HIP(ctx, hipGetLastError());
    return 0;
}
