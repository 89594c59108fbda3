// decrypt.hip — the way back out of the device: collective decryption (mpc/mhe.go:107-220 CollectiveDecrypt / CollectiveDecryptVec / CollectiveDecryptMat ->
// lattigo dckks.PCKSProtocol.GenShare / KeySwitch with the all-zero public key), single-key decryption (crypto/crypto.go:446-510 DecryptFloat*) and decoding
// (crypto.DecodeFloatVector, crypto/crypto.go:525-536 -> lattigo encoder.Decode).
//
// PARITY UNPINNED: PCKS is restated from the published lattigo v2.1 dckks/public_keyswitch.go, the branch that samples in R_QP and divides by P:
//   GenShare:  h0 = ModDown_P(u pk0 + e0) + sk (.) c1,  h1 = ModDown_P(u pk1 + e1)      with pk = 0 the ternary u multiplies zero and drops out
//   KeySwitch: c0' = c0 + sum h0,  c1' = sum h1;  the callers keep ciphertextSwitched.Plaintext() = c0' only
// ModDown_P(NTT_QP(e)) is the encryption core's (encrypt.hip, encrypt_errors_moddown: the same three launches with the public-key product skipped), sk (.) c1 + row
// and the row additions are the collective bootstrap's kernels (refresh.hip).  Neither bit parity with the Go binary nor the CPU cost this replaces can be established
// without a Go toolchain; what is pinned is the arithmetic (tests/test_gpu_decrypt.py).
//
// The decoder, per plaintext at level l (nl = l + 1 moduli):
//   1. INTT of the nl rows                                                                                         (k_ntt_inv, ntt.hip)
//   2. per coefficient: Garner mixed-radix digits, lattigo's Cmp(QHalf) centring rule (recode.hpp: the bootstrap's Recode states the same), the digits of the
//      MAGNITUDE |p_c| (for a negative value the digit-wise complement plus one: no cancellation ever happens in floating point), Horner over the digits in
//      double-double, one double-double division by the scale                                                      (k_dec_coeffs)
//   3. v_t = sum_c w_c zeta^(5^t c),  w_c = (p_c + i p_{c+n}) / scale,  n = N/2, zeta = exp(2 pi i / 2N): with 5^t = 4 m + 1 this is the length-n DFT (kernel
//      omega^(+mc), omega = exp(2 pi i / n)) of a_c = w_c zeta^c, read out at m = (5^t - 1)/4.                        (k_fft_decode)
// Which form of 3 was built: the REAL-ONLY transform, run once for the real parts and a second time (input -i w) when the imaginary parts are wanted as well.
// 8192 complex double-double points are 256 KiB and do not fit a workgroup's LDS; but Re v depends only on the Hermitian part g_c = (a_c + conj a_{n-c}) / 2 of
// the twisted input, and the transform of a Hermitian sequence is a length-n/2 complex transform behind one packing pass - the encoder's layout (encode.hip)
// backwards:  z_j = r_2j + i r_2j+1 = sum_{c < n/2} G_c Omega^(jc),  G_c = (g_c + g_{c+h}) + i omega^c (g_c - g_{c+h}),  h = n/2, Omega = omega^2.
// With a_{n-c} = i conj(zeta^c) w_{n-c}, a_{c+h} = eps zeta^c w_{c+h}, a_{h-c} = eps conj(zeta^c) w_{h-c} (eps = exp(i pi / 4)) everything factors through zeta^c:
//   U_c = w_c - i conj(w_{n-c})  (U_0 = 2 Re w_0),   V_c = eps w_{c+h} + conj(eps w_{h-c}),   G_c = (zeta^c / 2) ((U + V) + i omega^c (U - V)).
// The transform itself is the encoder's: x = conj(G) through the same four radix-8 passes and twiddle tables (dif_radix8, ddfft.hpp), z = conj(Z); the results are
// rounded to double ONCE, at the end, and leave through LDS in slot order.  ConvertVectorComplexToFloat64 keeps the real parts only, so the common call costs one
// transform of half the length; the complex call costs two.
//
// Error (the contract the header states): every intermediate of pass s that feeds one output is a sum over a disjoint subset of the inputs with unit-modulus
// weights, so the magnitudes that feed an output sum to at most 2 S, S = sum_c |w_c| (the packing adds four inputs with weight 1/2 each into two points).  Each of
// the K < 64 double-double operations on a path is off by at most 2^-96 of its operands' magnitudes (the lazy sums of dif_radix8 included), the errors reach the
// output with unit gain: |d_t - v_t| <= 2^-53 |v_t| + 64 * 2 * 2^-96 S.  By Parseval max_t |v_t| >= sqrt(sum |w_c|^2) >= S / sqrt(n), so with sqrt(n) < 2^6.5
//   |d_t - v_t| <= (2^-53 + 2^-82) max_t |v_t|.
#include "common.hpp"
#include "kernels.hpp"
#include "ddfft.hpp"
#include "recode.hpp"

__device__ __forceinline__ dd dd_add_d(dd a, double b) { dd s = dd_two_sum(a.hi, b); s.lo += a.lo; return dd_quick(s.hi, s.lo); }
__device__ __forceinline__ dd dd_div_d(dd a, double b) {            // (b finite, >= 1) the remainder of the first quotient is exact
    const double q1 = a.hi / b, r = __builtin_fma(-q1, b, a.hi);
    return dd_quick(q1, (r + a.lo) / b);
}

// ---------------------------------------------------------------- 2. centred big integer / scale, one coefficient per thread
// xin: [nvec][nl][N] coefficient-domain residues.  wdd (nullable): [nvec][N] {hi, lo};  coef (nullable): [nvec][N] the same rounded to double.  grid (N/256, nvec)
__global__ void __launch_bounds__(256) k_dec_coeffs(const u64 *xin, RecodeConst rc, double scale, double2 *wdd, double *coef, const ModConst *modc) {
    const int N = SFG_N, x = blockIdx.x * 256 + threadIdx.x; const size_t c = blockIdx.y;
    const int nl = rc.nl;
    double v[RF_MAXL], r[RF_MAXL];
    for (int i = 0; i < nl; i++) r[i] = u64_to_f64(xin[(c * nl + i) * (size_t)N + x]);
    garner_digits(r, v, nl, rc, modc);
    const bool neg = garner_negative(v, nl, rc);
    if (neg) {          // Q - x: every digit complemented (that is Q - 1 - x), plus one with the carry walked up - exact in the digits
        double carry = 1.0;
        for (int i = 0; i < nl; i++) {
            const double q = modc[i].q, m = (q - 1.0 - v[i]) + carry;
            carry = m == q ? 1.0 : 0.0;
            v[i] = m == q ? 0.0 : m;
        }
    }
    dd acc = dd_make(v[nl - 1], 0.0);                                          // |p| = v0 + q0 (v1 + q1 (v2 + ...)): non-negative terms only
    for (int i = nl - 2; i >= 0; i--) acc = dd_add_d(dd_mul_d(acc, modc[i].q), v[i]);
    dd w = dd_div_d(acc, scale);
    if (neg) w = dd_neg(w);
    const size_t o = c * (size_t)N + x;
    if (wdd) wdd[o] = make_double2(w.hi, w.lo);
    if (coef) coef[o] = w.hi + w.lo;
}

// ---------------------------------------------------------------- 3. the forward embedding, real parts (blockIdx.y = 0) or imaginary parts (1)
constexpr size_t DEC_LDS_BYTES = (size_t)2 * ENC_H * 8;        // 65,536 B: the exchange image (high parts, then low parts), at the end the n output doubles
// grid (nvec, 1 or 2), 512 threads
__global__ void __launch_bounds__(512) k_fft_decode(const double2 *wdd, const double4 *tb, const double4 *dec, const uint16_t *tinv, double *re_out, double *im_out) {
    extern __shared__ double lds[];
    double *RE = lds, *IM = lds + ENC_H;
    const int n = SFG_SLOTS, h = ENC_H, tid = threadIdx.x;
    const int part = blockIdx.y;
    const double2 *w = wdd + (size_t)blockIdx.x * SFG_N;
    double *out = (part ? im_out : re_out) + (size_t)blockIdx.x * n;
    // w_c, or -i w_c for the imaginary parts (Im v = Re of the transform of -i w)
    auto W = [&](int c, dd &re, dd &im) {
        const double2 a = w[c], b = w[c + n];
        if (!part) { re = dd_make(a.x, a.y); im = dd_make(b.x, b.y); }
        else { re = dd_make(b.x, b.y); im = dd_make(-a.x, -a.y); }
    };
    dd xr[8], xi[8], yr[8], yi[8];
    const dd rs = dd_make(7.071067811865475727e-01, -4.833646656726456726e-17);      // 1/sqrt(2) in double-double
    // ---- packing: x_m = conj(G_m), m = a*512 + tid
#pragma unroll
    for (int a = 0; a < 8; a++) {
        const int c = a * 512 + tid;
        dd Ur, Ui, Vr, Vi;
        {
            dd pr, pi; W(c, pr, pi);
            if (c == 0) { Ur = dd_make(2.0 * pr.hi, 2.0 * pr.lo); Ui = dd_make(0.0, 0.0); }
            else { dd qr, qi; W(n - c, qr, qi); Ur = dd_sub(pr, qi); Ui = dd_sub(pi, qr); }      // -i conj(x + iy) = -y - ix
        }
        {   // eps (x + iy) = ((x - y) + i (x + y)) / sqrt 2
            dd ar, ai, br, bi; W(c + h, ar, ai); W(h - c, br, bi);
            Vr = dd_mul(dd_add(dd_sub(ar, ai), dd_sub(br, bi)), rs);
            Vi = dd_mul(dd_sub(dd_add(ar, ai), dd_add(br, bi)), rs);
        }
        const dd Sr = dd_add(Ur, Vr), Si = dd_add(Ui, Vi), Dr = dd_sub(Ur, Vr), Di = dd_sub(Ui, Vi);
        const double4 wo = dec[h + c], zc = dec[c];
        const dd wor = dd_make(wo.x, wo.y), woi = dd_make(wo.z, wo.w), zr = dd_make(zc.x, zc.y), zi = dd_make(zc.z, zc.w);
        const dd Tr = dd_dot2(Dr, wor, Di, woi, -1.0), Ti = dd_dot2(Dr, woi, Di, wor, 1.0);
        const dd Rr = dd_sub(Sr, Ti), Ri = dd_add(Si, Tr);                                      // S + i T
        xr[a] = dd_dot2(Rr, zr, Ri, zi, -1.0);
        xi[a] = dd_neg(dd_dot2(Rr, zi, Ri, zr, 1.0));
        __builtin_amdgcn_sched_barrier(0);          // one point at a time: the 64 loads of a thread hoisted in front of the arithmetic do not fit the register file
    }
    // ---- the encoder's four passes (encode.hip k_fft_encode): src[k] goes to image index widx(k), dst[k] comes from index ridx(k); the high parts of all 4096 points
    // move through the image, then the low parts.  WAVE: every index a wave writes or reads lies in its own 512-point region, so wave-level ordering is enough.
    auto exchange = [&](dd (&sr)[8], dd (&si)[8], dd (&dr)[8], dd (&di)[8], auto widx, auto ridx, auto wave, bool entry_barrier) {
        constexpr bool WAVE = decltype(wave)::value;
        auto sync = [&]() { if (WAVE) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); else __syncthreads(); };
        if (entry_barrier) __syncthreads(); else sync();
#pragma unroll
        for (int k = 0; k < 8; k++) { const int p = padj(widx(k)); RE[p] = sr[k].hi; IM[p] = si[k].hi; }
        sync();
#pragma unroll
        for (int k = 0; k < 8; k++) { const int p = padj(ridx(k)); dr[k].hi = RE[p]; di[k].hi = IM[p]; }
        sync();
#pragma unroll
        for (int k = 0; k < 8; k++) { const int p = padj(widx(k)); RE[p] = sr[k].lo; IM[p] = si[k].lo; }
        sync();
#pragma unroll
        for (int k = 0; k < 8; k++) { const int p = padj(ridx(k)); dr[k].lo = RE[p]; di[k].lo = IM[p]; }
    };
    const std::false_type wg_wide; const std::true_type wave_local;
    dif_radix8<512, false>(xr, xi, tb + ENC_TB_P512, tid);
    {
        const int cd = tid & 63, ar = tid >> 6;
        exchange(xr, xi, yr, yi, [&](int a) { return a * 512 + tid; }, [&](int b) { return ar * 512 + b * 64 + cd; }, wg_wide, true);
        dif_radix8<64, false>(yr, yi, tb + ENC_TB_P64, cd);
        const int d = tid & 7, ab = tid >> 3;
        exchange(yr, yi, xr, xi, [&](int b) { return ar * 512 + b * 64 + cd; }, [&](int c) { return ab * 64 + c * 8 + d; }, wave_local, true);
        dif_radix8<8, false>(xr, xi, tb + ENC_TB_P8, d);
        exchange(xr, xi, yr, yi, [&](int c) { return ab * 64 + c * 8 + d; }, [&](int d4) { return tid * 8 + d4; }, wave_local, false);
        dif_radix8<1, false>(yr, yi, tb, 0);
    }
    // ---- position tid*8 + d4 holds Z_j, j = brev12(position); z_j = conj(Z_j) = r_2j + i r_2j+1 and r_m is the slot tinv[m].  Rounded to double here, once.
    __syncthreads();
    const int jb = (int)(__brev((unsigned)tid) >> 23);
#pragma unroll
    for (int d4 = 0; d4 < 8; d4++) {
        const int j = (int)((__brev((unsigned)d4) >> 29) << 9) | jb;
        const unsigned tt = reinterpret_cast<const unsigned *>(tinv)[j];                        // tinv[2j] | tinv[2j + 1] << 16
        lds[tt & 0xFFFFu] = yr[d4].hi + yr[d4].lo;
        lds[tt >> 16] = -(yi[d4].hi + yi[d4].lo);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) out[k * 512 + tid] = lds[k * 512 + tid];
}

int decrypt_set_attrs(sfg_ctx *ctx) {
    SFG_HIP(ctx, sfg_raise_lds({(const void *)k_fft_decode}, DEC_LDS_BYTES));
    return 0;
}

// ---------------------------------------------------------------- host side
int check_level_count(sfg_ctx *ctx, const char *what, int nct, int level, int maxl, int min_count) {
    if (level < 0 || level >= ctx->nq) SFG_FAIL(ctx, "%s: level %d out of range", what, level);
    if (maxl && level + 1 > maxl) SFG_FAIL(ctx, "%s: more than %d moduli at the input level", what, maxl);
    if (nct < 0) SFG_FAIL(ctx, "%s: negative ciphertext count", what);
    if (nct < min_count) SFG_FAIL(ctx, "%s: ciphertext count %d must be positive", what, nct);
    return 0;
}
static int dec_check_scale(sfg_ctx *ctx, const char *what, double scale) {
    if (!(scale >= 1.0) || !std::isfinite(scale)) SFG_FAIL(ctx, "%s: scale %g must be finite and at least 1", what, scale);
    return 0;
}

// GenShare(skShard, zeroPk, ct, share) for nct ciphertexts [nct][2][level+1][N]
extern "C" int sfg_pcks_gen_share_dev(sfg_ctx *ctx, const uint64_t *ct, int nct, int level, const int32_t *e0, const int32_t *e1, uint64_t *h0, uint64_t *h1) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(check_level_count(ctx, "pcks_gen_share", nct, level, RF_MAXL));
    if (!ctx->sh->sk_dev) SFG_FAIL(ctx, "pcks_gen_share: no secret-key shard loaded (sfg_ctx_load_secret_key)");
    if (!nct) return 0;
    if (!ct || !e0 || !h0 || (h1 && !e1)) SFG_FAIL(ctx, "pcks_gen_share: NULL ciphertexts, errors or output");
    ApiScope scope(ctx);
    const int N = SFG_N, nl = level + 1;
    const size_t ctw = pcks_share_words(nl, (size_t)N), roww = (size_t)nl * N;
    const BatchPlan plan = pcks_share_plan(nct, nl, (size_t)N);
    void *tp = nullptr;
    SFG_TRY(sfg_scratch(ctx, "decrypt.share", plan.bytes, &tp));
    u64 *T = (u64 *)tp;
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct);
        const int32_t *e0c = e0 + (size_t)c0 * N, *e1c = h1 ? e1 + (size_t)c0 * N : e0c;         // (h1 not wanted: polynomial 1 of T is not read)
        SFG_TRY(encrypt_errors_moddown(ctx, e0c, e1c, nb, level, T));
        SFG_TRY(launch_share(ctx, T, ctw, (const u64 *)ct + (size_t)c0 * ctw + roww, ctw, (u64 *)h0 + (size_t)c0 * roww, nl, nb));
        if (h1) SFG_HIP(ctx, hipMemcpy2DAsync(h1 + (size_t)c0 * roww, roww * 8, T + roww, ctw * 8, roww * 8, nb, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return 0;
}

// KeySwitch + .Plaintext(): pt = c0 + h0agg
extern "C" int sfg_pcks_finish_dev(sfg_ctx *ctx, const uint64_t *ct, int nct, int level, const uint64_t *h0agg, uint64_t *pt) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(check_level_count(ctx, "pcks_finish", nct, level, RF_MAXL));
    if (!nct) return 0;
    if (!ct || !h0agg || !pt) SFG_FAIL(ctx, "pcks_finish: NULL ciphertexts, shares or output");
    const int N = SFG_N, nl = level + 1;
    const BatchPlan plan = grid_rows_plan(nct);
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nct);
        SFG_TRY(launch_add_rows(ctx, (const u64 *)ct + (size_t)c0 * 2 * nl * N, (size_t)2 * nl * N, (const u64 *)h0agg + (size_t)c0 * nl * N, (size_t)nl * N,
                                (u64 *)pt + (size_t)c0 * nl * N, (size_t)nl * N, nl, nb));
    }
    return 0;
}

// the decryption front end (kernels.hpp): the one place that turns a source into coefficient rows, for the decoder here, the ring-vector decoder (rvec.hip) and
// the collective bootstrap's finish (refresh.hip)
int launch_dec_front(sfg_ctx *ctx, const DecSrc &s, int first, int nb, int nl, u64 *x, int *launches) {
    const size_t ctw = (size_t)2 * nl * SFG_N, roww = (size_t)nl * SFG_N;
    const ModPattern p0 = mod_pattern_run(0, nl);
    if (s.kind == DecSrc::ROWS) {
        RowMap rm; rm.rpg = nl; rm.gstride_in = s.stride; rm.gstride_out = roww;
        return launch_ntt_inv_map(ctx, s.src + (size_t)first * s.stride, x, (size_t)nb * nl, p0, rm);
    }
    const u64 *ct = s.src + (size_t)first * ctw;
    if (s.kind == DecSrc::FINISH) SFG_TRY(launch_add_rows(ctx, ct, ctw, s.h0agg + (size_t)first * roww, roww, x, roww, nl, nb));
    else SFG_TRY(launch_share(ctx, ct, ctw, ct + roww, ctw, x, nl, nb));                       // c0 + sk (.) c1
    if (launches) ++*launches;
    return launch_ntt_inv(ctx, x, x, (size_t)nb * nl, p0);
}

// the three stages for nvec plaintexts, in the chunks of decode_plan (batch_plan.hpp).  src: plaintext rows or ciphertexts [nvec][2][nl][N]; outputs on the host
// (host_out: the call synchronises) or on the device; coeffs != nullptr: stages 1 and 2 only.
static int decode_run(sfg_ctx *ctx, const char *what, const DecSrc &src, int nvec, int level, double scale, double *re, double *im, double *coeffs, bool host_out) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    SFG_TRY(check_level_count(ctx, what, nvec, level, RF_MAXL));
    SFG_TRY(dec_check_scale(ctx, what, scale));
    if (src.kind == DecSrc::DECRYPT && !ctx->sh->sk_dev) SFG_FAIL(ctx, "%s: no secret key loaded (sfg_ctx_load_secret_key)", what);
    const int N = SFG_N, n = SFG_SLOTS, nl = level + 1;
    if (src.kind == DecSrc::ROWS && src.stride < (size_t)nl * N) SFG_FAIL(ctx, "%s: plaintext stride %zu below (level + 1) * N", what, src.stride);
    if (host_out) {       // results leave the device here: refused, with nothing launched, while an unprovable encoder rounding is outstanding
        SFG_TRY(sfg_sync_all(ctx));
        SFG_TRY(sfg_encoder_check(ctx));
    }
    if (!nvec) return 0;
    if (!src.src || (!coeffs && !re) || (src.kind == DecSrc::FINISH && !src.h0agg)) SFG_FAIL(ctx, "%s: NULL input or output", what);
    ApiScope scope(ctx);
    EncTables *et = (EncTables *)ctx->enc_tables();
    const int parts = im ? 2 : 1;
    const DecodeWords dw = decode_words(nl, (size_t)N, coeffs != nullptr, host_out, parts);
    const BatchPlan plan = decode_plan(nvec, dw);
    void *xp = nullptr, *wp = nullptr, *op = nullptr;
    SFG_TRY(sfg_scratch(ctx, "decrypt.x", plan.bytes_of(dw.x), &xp));
    if (dw.w) SFG_TRY(sfg_scratch(ctx, "decrypt.w", plan.bytes_of(dw.w), &wp));
    if (dw.out) SFG_TRY(sfg_scratch(ctx, "decrypt.out", plan.bytes_of(dw.out), &op));
    u64 *x = (u64 *)xp; double2 *wdd = (double2 *)wp; double *ob = (double *)op;
    RecodeConst rc; recode_constants(ctx, level, rc);
    PhaseTimer timer(ctx, "decode");
    int launches = 0;
    for (int c = 0; c < plan.nchunks; c++) {
        const int c0 = plan.first(c), nb = plan.count(c, nvec);
        SFG_TRY(launch_dec_front(ctx, src, c0, nb, nl, x, &launches));
        double *cdst = coeffs ? (host_out ? ob : coeffs + (size_t)c0 * N) : nullptr;
        hipLaunchKernelGGL(k_dec_coeffs, dim3(N / 256, nb), dim3(256), 0, ctx->stream, (const u64 *)x, rc, scale, coeffs ? (double2 *)nullptr : wdd, cdst, ctx->modc);
        SFG_HIP(ctx, hipGetLastError());
        launches += 2;
        if (coeffs) {
            if (host_out) {
                SFG_HIP(ctx, hipMemcpyAsync(coeffs + (size_t)c0 * N, ob, (size_t)nb * N * 8, hipMemcpyDeviceToHost, ctx->stream));
                if (c + 1 < plan.nchunks) SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the staging buffer is reused by the next chunk)
            }
            continue;
        }
        double *rdst = host_out ? ob : re + (size_t)c0 * n, *idst = !im ? nullptr : host_out ? ob + (size_t)plan.chunk * n : im + (size_t)c0 * n;
        hipLaunchKernelGGL(k_fft_decode, dim3(nb, parts), dim3(512), DEC_LDS_BYTES, ctx->stream, (const double2 *)wdd, (const double4 *)et->tb, (const double4 *)et->dec,
                           (const uint16_t *)et->tinv, rdst, idst);
        SFG_HIP(ctx, hipGetLastError());
        launches++;
        if (host_out) {
            SFG_HIP(ctx, hipMemcpyAsync(re + (size_t)c0 * n, rdst, (size_t)nb * n * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (im) SFG_HIP(ctx, hipMemcpyAsync(im + (size_t)c0 * n, idst, (size_t)nb * n * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (c + 1 < plan.nchunks) SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the staging buffer is reused by the next chunk)
        }
    }
    timer.stop(launches);
    if (host_out) SFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int sfg_decode_vectors(sfg_ctx *ctx, const uint64_t *pt, size_t pt_stride, int nct, int level, double scale, double *re_host, double *im_host) {
    return decode_run(ctx, "decode_vectors", DecSrc::rows((const u64 *)pt, pt_stride), nct, level, scale, re_host, im_host, nullptr, true);
}
extern "C" int sfg_decode_vectors_dev(sfg_ctx *ctx, const uint64_t *pt, size_t pt_stride, int nct, int level, double scale, double *re_dev, double *im_dev) {
    return decode_run(ctx, "decode_vectors_dev", DecSrc::rows((const u64 *)pt, pt_stride), nct, level, scale, re_dev, im_dev, nullptr, false);
}
extern "C" int sfg_decode_coeffs(sfg_ctx *ctx, const uint64_t *pt, size_t pt_stride, int nct, int level, double scale, double *coeffs_host) {
    if (nct > 0 && !coeffs_host) SFG_FAIL(ctx, "decode_coeffs: NULL output");
    static double none;       // (nct == 0: the argument checks still run; nothing is written)
    return decode_run(ctx, "decode_coeffs", DecSrc::rows((const u64 *)pt, pt_stride), nct, level, scale, nullptr, nullptr, coeffs_host ? coeffs_host : &none, true);
}
extern "C" int sfg_pcks_finish_decode(sfg_ctx *ctx, const uint64_t *ct, int nct, int level, double scale, const uint64_t *h0agg, double *re_host, double *im_host) {
    return decode_run(ctx, "pcks_finish_decode", DecSrc::finish((const u64 *)ct, (const u64 *)h0agg), nct, level, scale, re_host, im_host, nullptr, true);
}
extern "C" int sfg_decrypt_vectors(sfg_ctx *ctx, const uint64_t *ct, int nct, int level, double scale, double *re_host, double *im_host) {
    return decode_run(ctx, "decrypt_vectors", DecSrc::decrypt((const u64 *)ct), nct, level, scale, re_host, im_host, nullptr, true);
}
