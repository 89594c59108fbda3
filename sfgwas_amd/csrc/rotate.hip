// rotate.hip — ciphertext slot rotations: crypto.RotateRightWithEvaluator / RotateRight
// (crypto/basics.go:201-224) -> lattigo ckks.Evaluator.RotateNew = hybrid key switch of c1 with the Galois key,
// add to c0, NTT-domain automorphism of both polynomials.  Used for the baby-step rotation cache
// (gwas/matmult.go:1114,1375) and the giant-step alignment (:1207,1476).
//
// Batched over ciphertexts (each may use a different key).  Per ciphertext at level l (nl = l+1 moduli,
// alpha = np special primes per digit, beta = ceil(nl/alpha) digits, nt = nl + np targets):
//   1. c2 = INTT(c1), without the last stage and 1/N                              nl rows  (k_ntt_inv_split)
//   2. digit i -> last inverse stage and 1/N on the pairs it loads, exact (float-corrected) basis extension to every target outside the digit (k_ksw_extend)
//      (inside the digit the original NTT rows are reused), then NTT of the extended rows         beta*nt rows
//   3. special-prime targets only: acc_{0,1}[t] = sum_i ext[i][t] * key[i][{0,1}][t]              (k_ksw_inner_p)
//   4. ModDown: INTT of those 2 np rows (split, finished by the reader), basis extension P -> Q, NTT   (k_moddown_extend)
//   5. at the gathered position src = index[x]: acc_{0,1}[t] of the Q targets as in 3, then
//      out0 = perm(c0 + (acc0 - ext0) / P), out1 = perm((acc1 - ext1) / P)                        (k_ksw_finish, k_ksw_finish_sum)
// The float correction v = uint64(sum float64(y_m)/float64(q_m)) is lattigo's (ring.Decomposer /
// FastBasisExtender); the oracle mirrors it, so results agree bit for bit.
// Which kernel computes what (profiles/ksw_fused_ab.txt, profiles/ksw_inner_finish_ab.txt): the extension kernels of 2 and 4 apply the forward transform's first
// stage to the rows they write, so the split transform reads half a row per workgroup and starts at stage 2, and the inverse transform's last stage to the rows
// they read, so the split inverse transform stays inside half a row; a job written as MAC operand rows produces nothing of the moduli the MAC does not read; jobs
// whose results are summed (the giant-step alignment) are summed in step 5 (k_ksw_finish_sum); no Q row of the inner product is stored - the finish forms it from
// the rows it gathers anyway; consecutive jobs under one key and table (a tile, ksw_plan.hpp) share each load of a key word in 3 and 5.  Every output word is the
// canonical word it was.
// The host side: a front-end resolves its rotations into a list of jobs (KswJobs; resolve_rotation: one rule for index, Galois element and key) and describes the
// batch (KswBatch); ksw_plan.hpp decides, as pure functions tested on a CPU, how many inputs share a decomposition and how many jobs a chunk, where the regions of
// the workspace lie, and which jobs fall into which input group, chunk and tile; launch_keyswitch_jobs executes that plan: reserve, upload, launch.
#include "common.hpp"
#include "kernels.hpp"
#include "ksw.hpp"
#include "ksw_plan.hpp"
#include <memory>

// Jobs per tile (ksw_plan.hpp) of k_ksw_inner_p and k_ksw_finish: a key word is loaded once for that many jobs.  Measured at 1, 3 and 5 (profiles/ksw_inner_finish_ab.txt):
// 3 is the fastest for both.  The summed finish takes no tiles: with s = 15 outputs per block column, tiles of 3 or 5 segments leave it too few workgroups.
constexpr int KSW_T = 3;


static void fill_ext(const sfg_ctx *ctx, ExtConst &e, const std::vector<int> &src) {
    memset(&e, 0, sizeof e);
    e.a = (int)src.size();
    for (int m = 0; m < e.a; m++) e.src[m] = src[m];
    for (int m = 0; m < e.a; m++) {
        u64 qm = ctx->q[src[m]], h = 1;
        for (int k = 0; k < e.a; k++) if (k != m) h = h_mulmod(h, ctx->q[src[k]] % qm, qm);
        u64 hi = h_invmod(h, qm);
        e.qhat_inv[m] = (double)hi; e.qhat_inv_q[m] = (double)hi / (double)qm;
    }
    for (int t = 0; t < ctx->nmod; t++) {
        u64 qt = ctx->q[t], D = 1 % qt;
        for (int m = 0; m < e.a; m++) {
            u64 ht = 1 % qt;
            for (int k = 0; k < e.a; k++) if (k != m) ht = h_mulmod(ht, ctx->q[src[k]] % qt, qt);
            e.qhat_t[t][m] = (double)ht; e.qhat_t_q[t][m] = (double)ht / (double)qt;
            D = h_mulmod(D, ctx->q[src[m]] % qt, qt);
        }
        e.D_t[t] = (double)D; e.D_t_q[t] = (double)D / (double)qt;
    }
}


// The constants are built once per level and kept, host and device copy together, in the context (freed by sfg_ctx_destroy); an unsupported shape is refused on
// every call and caches nothing.
int get_ksw(sfg_ctx *ctx, int level, const KswConst **dev, const KswConst **host) {
    const int nl = level + 1, alpha = ctx->np, nt = nl + ctx->np, beta = (nl + alpha - 1) / alpha;
    if (alpha > KSW_MAXA || beta > KSW_MAXDIG) SFG_FAIL(ctx, "key-switch shape unsupported (alpha > 4 or beta > 8)");
    if (beta * nt > SFG_MAXPATTERN) SFG_FAIL(ctx, "key-switch shape unsupported (beta * (level + 1 + np) = %d rows exceed the modulus pattern table)", beta * nt);
    auto it = ctx->ksw_cache.find(level);
    if (it != ctx->ksw_cache.end()) { *dev = it->second->dev; *host = &it->second->host; return 0; }
    std::unique_ptr<KswLevel> rec(new KswLevel);
    KswConst &kc = rec->host; memset(&kc, 0, sizeof kc);
    kc.level = level; kc.nl = nl; kc.np = ctx->np; kc.alpha = alpha; kc.nt = nt; kc.beta = beta;
    for (int t = 0; t < kc.nt; t++) { kc.tmod[t] = t < kc.nl ? t : ctx->nq + (t - kc.nl); kc.digit_of[t] = t < kc.nl ? t / kc.alpha : -1; }
    for (int i = 0; i < kc.beta; i++) {
        std::vector<int> src;
        for (int m = i * kc.alpha; m < (i + 1) * kc.alpha && m < kc.nl; m++) src.push_back(m);
        fill_ext(ctx, kc.dig[i], src);
    }
    std::vector<int> ps; for (int p = 0; p < kc.np; p++) ps.push_back(ctx->nq + p);
    fill_ext(ctx, kc.pq, ps);
    for (int t = 0; t < kc.nl; t++) {
        u64 qt = ctx->q[t], P = 1;
        for (int p = 0; p < kc.np; p++) P = h_mulmod(P, ctx->q[ctx->nq + p] % qt, qt);
        u64 pi = h_invmod(P, qt);
        kc.pinv[t] = (double)pi; kc.pinv_q[t] = (double)pi / (double)qt;
    }
    SFG_HIP(ctx, hipMalloc(&rec->dev, sizeof(KswConst)));
    if (hipError_t e = hipMemcpy(rec->dev, &kc, sizeof(KswConst), hipMemcpyHostToDevice)) { (void)hipFree(rec->dev); SFG_HIP(ctx, e); }
    *dev = rec->dev; *host = &rec->host;
    ctx->ksw_cache[level] = rec.release();
    return 0;
}


// the last inverse stage and 1/N on the pair (u, v) at x and x + N/2 of a row of modulus mc, w = entry 1 of its inverse table (fp64mod.hpp inv_last_pair)
__device__ __forceinline__ void inv_last_of(const ModConst &mc, double w, double &u, double &v) {
    const double wn = canon(mulmod_lazy(w, mc.ninv, mc.ninv_q, mc.q), mc.q, mc.qinv);
    inv_last_pair(u, v, mc.ninv, mc.ninv_q, wn, wn * mc.qinv, mc.q, mc.qinv, u, v);
}
// grid (N/512, beta, B). c2: [B][nl][N] c1 out of the split inverse transform; ext: [B][beta][nt][N].  A thread extends positions x and x + N/2, so that it can
// apply the forward transform's first stage to the rows it writes (PRE1, fp64mod.hpp fwd_stage1_pair): the element-wise kernels wait for memory and have fp64
// issue slots to spare, the transforms do not.  c2 lacks the inverse transform's last stage and 1/N (ntt.hip k_ntt_inv_split): the pair a thread loads is exactly
// a pair of that stage, finished here (inv_last_of) for the same reason.
// The body is k_moddown_extend's, line for line, and stays written out in both: moved into shared __forceinline__ helpers, the compiler schedules it differently
// (other instruction text, other instruction counts), and these two kernels are pinned to the instruction.
template <bool PRE1>
__global__ void __launch_bounds__(256) k_ksw_extend(const u64 *c2, u64 *ext, const KswConst *kcp, const ModConst *modc, const double *tw_fwd, const double *tw_inv) {
    const KswConst &kc = *kcp;
    const int N = SFG_N, n = N / 2, x = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y; const size_t b = blockIdx.z;
    const ExtConst &e = kc.dig[i];
    const u64 *c2b = c2 + b * (size_t)kc.nl * N;
    u64 *eb = ext + (b * kc.beta + i) * (size_t)kc.nt * N;
    double xs[2][KSW_MAXA], y[2][KSW_MAXA], v[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int m = 0; m < KSW_MAXA; m++) xs[h][m] = m < e.a ? u64_to_f64(c2b[(size_t)e.src[m] * N + h * n + x]) : 0.0;
#pragma unroll
    for (int m = 0; m < KSW_MAXA; m++) if (m < e.a) inv_last_of(modc[e.src[m]], tw_inv[(size_t)e.src[m] * N + 1], xs[0][m], xs[1][m]);
    if (e.a > 1) { ext_prepare(e, modc, xs[0], y[0], v[0]); ext_prepare(e, modc, xs[1], y[1], v[1]); }
    for (int t = 0; t < kc.nt; t++) {
        const int tg = kc.tmod[t];
        if (kc.digit_of[t] == i) continue;                                            // in-digit: the original NTT row, which the finish reads where it lies
        const double q = modc[tg].q, qinv = modc[tg].qinv;
        double o0, o1;
        if (e.a == 1) { o0 = canon(xs[0][0], q, qinv); o1 = canon(xs[1][0], q, qinv); }      // single-prime digit: raw copy mod q_t
        else { o0 = ext_target(e, tg, q, qinv, y[0], v[0]); o1 = ext_target(e, tg, q, qinv, y[1], v[1]); }
        if (PRE1) { const double W = tw_fwd[(size_t)tg * N + 1]; fwd_stage1_pair(o0, o1, W, W * qinv, q, qinv, o0, o1); }
        eb[(size_t)t * N + x] = f64_to_u64(o0); eb[(size_t)t * N + n + x] = f64_to_u64(o1);
    }
}

// grid (N/512, np, tiles). acc: [B][2][np][N], the special-prime targets only (the ModDown's input): the Q targets of the inner product are formed where they
// are consumed, in the finish.  Two coefficients per thread: 16-byte loads and stores.  A tile is up to T consecutive jobs under one key (ksw_plan.hpp): a key word
// is loaded once and applied to the tile's T extended inputs.
template <int T>
__global__ void __launch_bounds__(256) k_ksw_inner_p(const u64 *ext, const u64 *const *keys, const int *inidx, const KswTile *tiles, u64 *acc, const KswConst *kcp,
                                                    const ModConst *modc, int nmod) {
    const KswConst &kc = *kcp;
    const int N = SFG_N, x = 2 * (blockIdx.x * 256 + threadIdx.x), m = blockIdx.y, t = kc.nl + m;
    const KswTile tl = tiles[blockIdx.z];
    const int tg = kc.tmod[t];
    const double q = modc[tg].q, qinv = modc[tg].qinv;
    const u64 *key = keys[tl.start];
    const u64 *eb[T];
#pragma unroll
    for (int j = 0; j < T; j++) eb[j] = ext + ((size_t)inidx[tl.start + (j < tl.count ? j : 0)] * kc.beta * (size_t)kc.nt + t) * N + x;
    double a[T][4];
#pragma unroll
    for (int j = 0; j < T; j++) a[j][0] = a[j][1] = a[j][2] = a[j][3] = 0.0;
    for (int i = 0; i < kc.beta; i++) {
        const ulonglong2 k0 = *reinterpret_cast<const ulonglong2 *>(key + (((size_t)i * 2 + 0) * nmod + tg) * N + x);
        const ulonglong2 k1 = *reinterpret_cast<const ulonglong2 *>(key + (((size_t)i * 2 + 1) * nmod + tg) * N + x);
        const double k0x = u64_to_f64(k0.x), k0y = u64_to_f64(k0.y), k1x = u64_to_f64(k1.x), k1y = u64_to_f64(k1.y);
#pragma unroll
        for (int j = 0; j < T; j++) {           // no branch on the tile's length: a short tile's spare slots repeat its first job (loads that hit), only the stores are guarded
            const ulonglong2 ev = *reinterpret_cast<const ulonglong2 *>(eb[j] + (size_t)i * kc.nt * N);
            const double ex = u64_to_f64(ev.x), ey = u64_to_f64(ev.y);
            a[j][0] += mulmod2(ex, k0x, q, qinv); a[j][1] += mulmod2(ey, k0y, q, qinv);
            a[j][2] += mulmod2(ex, k1x, q, qinv); a[j][3] += mulmod2(ey, k1y, q, qinv);
        }
    }
#pragma unroll
    for (int j = 0; j < T; j++) {
        if (j < tl.count) {
            u64 *o = acc + ((size_t)(tl.start + j) * 2 * kc.np + m) * N + x;
            *reinterpret_cast<ulonglong2 *>(o) = make_ulonglong2(f64_to_u64(canon(a[j][0], q, qinv)), f64_to_u64(canon(a[j][1], q, qinv)));
            *reinterpret_cast<ulonglong2 *>(o + (size_t)kc.np * N) = make_ulonglong2(f64_to_u64(canon(a[j][2], q, qinv)), f64_to_u64(canon(a[j][3], q, qinv)));
        }
    }
}

// grid (N/512, 2, B): the rows of acc [B][2][np][N] (out of the split inverse transform) -> ext2 [B][2][nl][N] coefficient domain, rows t < nq_out (the others
// nobody reads).  Positions x and x + N/2 in one thread, the last inverse stage on the pairs read and PRE1 on the pairs written as in k_ksw_extend.
template <bool PRE1>
__global__ void __launch_bounds__(256) k_moddown_extend(const u64 *acc, u64 *ext2, const KswConst *kcp, const ModConst *modc, const double *tw_fwd, const double *tw_inv, int nq_out) {
    const KswConst &kc = *kcp;
    const int N = SFG_N, n = N / 2, x = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y; const size_t b = blockIdx.z;
    const ExtConst &e = kc.pq;
    const u64 *ap = acc + (b * 2 + p) * (size_t)kc.np * N;
    double xs[2][KSW_MAXA], y[2][KSW_MAXA], v[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int m = 0; m < KSW_MAXA; m++) xs[h][m] = m < e.a ? u64_to_f64(ap[(size_t)m * N + h * n + x]) : 0.0;
#pragma unroll
    for (int m = 0; m < KSW_MAXA; m++) if (m < e.a) inv_last_of(modc[e.src[m]], tw_inv[(size_t)e.src[m] * N + 1], xs[0][m], xs[1][m]);
    if (e.a > 1) { ext_prepare(e, modc, xs[0], y[0], v[0]); ext_prepare(e, modc, xs[1], y[1], v[1]); }
    for (int t = 0; t < nq_out; t++) {
        const double q = modc[t].q, qinv = modc[t].qinv;
        double o0, o1;
        if (e.a == 1) { o0 = canon(xs[0][0], q, qinv); o1 = canon(xs[1][0], q, qinv); }
        else { o0 = ext_target(e, t, q, qinv, y[0], v[0]); o1 = ext_target(e, t, q, qinv, y[1], v[1]); }
        if (PRE1) { const double W = tw_fwd[(size_t)t * N + 1]; fwd_stage1_pair(o0, o1, W, W * qinv, q, qinv, o0, o1); }
        u64 *row = ext2 + ((b * 2 + p) * (size_t)kc.nl + t) * N;
        row[x] = f64_to_u64(o0); row[n + x] = f64_to_u64(o1);
    }
}

// Optional output form of a key-switch job: instead of a u64 ciphertext, the fp64 operand rows the MAC reads (mac_dma.hip k_rot_to_f64: one centred double per
// word for a small modulus, a signed {lo, hi} pair for the 46-bit one; only the first L moduli, which are all the MAC accumulates over).  The baby-step
// rotation cache is written in this form directly: no u64 copy of it exists, and the rows of modulus L are never produced.
struct F64Form { int on, L, centre; size_t rowf; int plane_of[SFG_MAXMOD], big[SFG_MAXMOD]; };
__device__ __forceinline__ void store_rot_f64(double *row, const F64Form &ff, int t, int x, double v, double q) {     // v canonical in [0, q)
    const int N = SFG_N;
    double *o = row + (size_t)ff.plane_of[t] * N;
    if (ff.big[t]) {
        const double wc = v > __builtin_floor(q * 0.5) ? v - q : v;                         // centred; q odd: floor(q/2) = (q-1)/2 = q >> 1
        const double hi = __builtin_floor((wc + 4194304.0) * 0x1p-23), lo = wc - hi * 8388608.0;
        o[2 * x] = lo; o[2 * x + 1] = hi;
    } else o[x] = (ff.centre && v > __builtin_floor(q * 0.5)) ? v - q : v;
}
// The inner product of one Q target at one gathered position, for the (up to T) jobs that share the key word: a[j][p] += ext_j[i][t][src] * key[i][p][t][src] over the
// digits i, the row of digit i at a target inside digit i being the input's own NTT row (polynomial 1 of ct_in): read there, never copied.  bi[j]: the job's
// decomposed input.  Sums of beta <= 8 lazy products, |a| < 8 q < 2^51.
template <int T>
__device__ __forceinline__ void ksw_inner_q(const u64 *ext, const u64 *ct_in, const u64 *key, const KswConst &kc, int nmod, int t, int src, const size_t (&bi)[T],
                                           double q, double qinv, double (&a)[T][2]) {
    const int N = SFG_N;
#pragma unroll
    for (int j = 0; j < T; j++) a[j][0] = a[j][1] = 0.0;
    for (int i = 0; i < kc.beta; i++) {
        const double k0 = u64_to_f64(key[(((size_t)i * 2 + 0) * nmod + t) * N + src]), k1 = u64_to_f64(key[(((size_t)i * 2 + 1) * nmod + t) * N + src]);
        const bool own = kc.digit_of[t] == i;
#pragma unroll
        for (int j = 0; j < T; j++) {           // no branch on the tile's length: the spare slots of a short tile repeat its first job (bi[j] = bi[0]: loads that hit)
            const double e = u64_to_f64(own ? ct_in[(bi[j] * 2 * (size_t)kc.nl + kc.nl + t) * N + src] : ext[((bi[j] * kc.beta + i) * (size_t)kc.nt + t) * N + src]);
            a[j][0] += mulmod2(e, k0, q, qinv); a[j][1] += mulmod2(e, k1, q, qinv);
        }
    }
}
// grid (N/256, nq_out, tiles): out = perm(c0 + (acc0 - ext0)/P), perm((acc1 - ext1)/P); out[x] = in[index[x]], with acc_p[t] = sum_i ext[i][t] * key[i][p][t] formed
// here at the gathered position (no Q row of the inner product crosses memory).  A tile: up to T consecutive jobs with one key and one table (ksw_plan.hpp).
// An aligned run of 256 positions maps into an aligned run of 256 sources (the low bits of x are the high bits of the evaluation point's exponent, which the
// automorphism keeps): the gathers of a workgroup stay inside 2 KiB of each row.  Only their speed rests on that.
// add1 (nullable): [nin][nl][N] rows added to polynomial 1 (relinearisation: the degree-1 term of the tensor product)
template <int T>
__global__ void __launch_bounds__(256) k_ksw_finish(const u64 *ext, const u64 *ct_in, const u64 *const *keys, const int *inidx, const u64 *ext2, const uint16_t *const *index,
                                                   u64 *const *ct_out, const KswTile *tiles, const KswConst *kcp, const ModConst *modc, int nmod, const u64 *add1, F64Form ff) {
    const KswConst &kc = *kcp;
    const int N = SFG_N, x = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (ff.on && t >= ff.L) return;
    const KswTile tl = tiles[blockIdx.z];
    const double q = modc[t].q, qinv = modc[t].qinv, pinv = kc.pinv[t], pinv_q = kc.pinv_q[t];
    const int src = index[tl.start][x];
    size_t bi[T];
#pragma unroll
    for (int j = 0; j < T; j++) bi[j] = (size_t)inidx[tl.start + (j < tl.count ? j : 0)];
    double a[T][2];
    ksw_inner_q<T>(ext, ct_in, keys[tl.start], kc, nmod, t, src, bi, q, qinv, a);
#pragma unroll
    for (int j = 0; j < T; j++) {
        if (j < tl.count) {
            const size_t b = (size_t)(tl.start + j);
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const double e = u64_to_f64(ext2[((b * 2 + p) * (size_t)kc.nl + t) * N + src]);
                double r = mulmod_lazy(pred(a[j][p], q, qinv) - e, pinv, pinv_q, q);
                if (p == 0) r += u64_to_f64(ct_in[(bi[j] * 2 * (size_t)kc.nl + t) * N + src]);
                else if (add1) r += u64_to_f64(add1[(bi[j] * (size_t)kc.nl + t) * N + src]);
                const double v = canon(r, q, qinv);
                if (ff.on) store_rot_f64(reinterpret_cast<double *>(ct_out[b]) + (size_t)p * ff.rowf, ff, t, x, v, q);
                else ct_out[b][((size_t)p * kc.nl + t) * N + x] = f64_to_u64(v);
            }
        }
    }
}

// The finish of jobs whose results are SUMMED (the giant-step alignment, KswSum): grid (N/256, nl, segments), one thread per output word of both polynomials.
// A segment is one output and the jobs of this chunk that add into it (jobs[start .. start + count), chunk-local numbers): each job with its own automorphism
// table, key, extended rows and c0; the Q-row inner product of each is formed here as in k_ksw_finish.  The canonical results are added as exact integers (reduced
// every 8 jobs: below 11 q < 2^51), an unrotated member (plain) joins as a plain read, and the sum is reduced once: the canonical word the separate rotations,
// summed afterwards, give.  No tiles here: the jobs that share a key go to DIFFERENT outputs, and walking 3 or 5 outputs in step left the grid too few
// workgroups (0.249 / 0.208 s per step against 0.187 s, profiles/ksw_inner_finish_ab.txt).
struct KswSeg { const u64 *plain; u64 *out; int start, count, accumulate, pad; };
__global__ void __launch_bounds__(256) k_ksw_finish_sum(const u64 *ext, const u64 *ct_in, const u64 *const *keys, const int *inidx, const u64 *ext2, const uint16_t *const *index,
                                                       const KswSeg *segs, const int *jobs, const KswConst *kcp, const ModConst *modc, int nmod) {
    const KswConst &kc = *kcp;
    const int N = SFG_N, x = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    const KswSeg sg = segs[blockIdx.z];
    const double q = modc[t].q, qinv = modc[t].qinv, pinv = kc.pinv[t], pinv_q = kc.pinv_q[t];
    const size_t w0 = (size_t)t * N + x, w1 = ((size_t)kc.nl + t) * N + x;
    double s0 = 0.0, s1 = 0.0;
    if (sg.accumulate) { s0 = u64_to_f64(sg.out[w0]); s1 = u64_to_f64(sg.out[w1]); }
    if (sg.plain) { s0 += u64_to_f64(sg.plain[w0]); s1 += u64_to_f64(sg.plain[w1]); }
    for (int k = 0; k < sg.count; k++) {
        const size_t b = (size_t)jobs[sg.start + k];
        const size_t bi[1] = {(size_t)inidx[b]};
        const int src = index[b][x];
        double a[1][2];
        ksw_inner_q<1>(ext, ct_in, keys[b], kc, nmod, t, src, bi, q, qinv, a);
        const double e0 = u64_to_f64(ext2[((b * 2 + 0) * (size_t)kc.nl + t) * N + src]), e1 = u64_to_f64(ext2[((b * 2 + 1) * (size_t)kc.nl + t) * N + src]);
        const double c0 = u64_to_f64(ct_in[(bi[0] * 2 * (size_t)kc.nl + t) * N + src]);
        s0 += canon(mulmod_lazy(pred(a[0][0], q, qinv) - e0, pinv, pinv_q, q) + c0, q, qinv);
        s1 += canon(mulmod_lazy(pred(a[0][1], q, qinv) - e1, pinv, pinv_q, q), q, qinv);
        if ((k & 7) == 7) { s0 = pred(s0, q, qinv); s1 = pred(s1, q, qinv); }
    }
    sg.out[w0] = f64_to_u64(canon(s0, q, qinv)); sg.out[w1] = f64_to_u64(canon(s1, q, qinv));
}

__global__ void __launch_bounds__(256) k_ct_add(const u64 *a, const u64 *b, u64 *out, int nl, const ModConst *modc, size_t total_rows) {
    const int N = SFG_N; const size_t row = blockIdx.x / (N / 256); const int m = (int)(row % nl);
    const u64 q = modc[m].qi;
    const size_t off = row * N + (blockIdx.x % (N / 256)) * 256 + threadIdx.x;
    u64 v = a[off] + b[off]; out[off] = v >= q ? v - q : v;
}

// Key-switch a batch of jobs.  `in` holds nin ciphertext-shaped inputs [nin][2][nl][N] whose polynomial 1 is switched;
// job k reads input job_in[k], uses key keyp[k] and automorphism table idxp[k], and writes
//   out0 = perm(in.p0 + d0), out1 = perm(d1 [+ add1[in]])            to outp[k].
// Decomposition (steps 1-2) is done once per INPUT and shared by all its jobs ("hoisting"): the per-key work is
// only the inner product, ModDown and the automorphism.  Same arithmetic, same bits.
// With a KswSum the jobs' results are not stored one by one (outp is not read): job k adds into output group[k] < nout (KswJobs), and output i becomes
//   [its old content, when accumulate] + [plain[i], an unrotated ciphertext, when not null] + sum of its jobs     at out + i * out_stride,
// every word reduced once (k_ksw_finish_sum).  An input group or job chunk may hold any part of an output's jobs: the first part writes, the others add.
struct KswSum { int nout; std::vector<const u64 *> plain; u64 *out; size_t out_stride; int accumulate; };
// The jobs of a batch: job k reads input job_in[k] with key keyp[k] and table idxp[k]; it writes outp[k], or adds into output group[k] of the batch's KswSum.
struct KswJobs {
    std::vector<int> job_in; std::vector<const u64 *> keyp; std::vector<const uint16_t *> idxp; std::vector<u64 *> outp; std::vector<int> group;
    void add(int in, const RotKey &key, u64 *out, int grp = 0) { job_in.push_back(in); keyp.push_back(key.key_dev); idxp.push_back(key.index_dev); outp.push_back(out); group.push_back(grp); }
    // job j = input j under one key, written to out + j * stride words
    KswJobs(int nct, const RotKey &key, u64 *out, size_t stride) { for (int j = 0; j < nct; j++) add(j, key, out + (size_t)j * stride); }
    KswJobs() {}
};
// What the jobs work on: the inputs and their level, rows added to polynomial 1 (add1, nullable), the output form (ff, nullable: u64 ciphertexts), the sum (nullable)
struct KswBatch { const u64 *in; int nin, level; const u64 *add1 = nullptr; const F64Form *ff = nullptr; const KswSum *sum = nullptr; };
static_assert(sizeof(KswSeg) == KSW_SEG_BYTES && sizeof(void *) == KSW_PTR_BYTES, "ksw_plan.hpp lays the tables out for these sizes");

static int launch_keyswitch_jobs(sfg_ctx *ctx, const KswBatch &bt, const KswJobs &jb) {
    const int N = SFG_N, level = bt.level, nl = level + 1, nin = bt.nin;
    const u64 *in = bt.in, *add1 = bt.add1; const KswSum *sum = bt.sum;
    F64Form ff; memset(&ff, 0, sizeof ff); if (bt.ff) ff = *bt.ff;
    const KswConst *kcd, *kcp;
    SFG_TRY(get_ksw(ctx, level, &kcd, &kcp));
    const KswConst &kc = *kcp;
    const size_t ctw = (size_t)2 * nl * N;
    const int nr = (int)jb.job_in.size(), nout = sum ? sum->nout : 0;
    if (sum && (ff.on || add1 || (int)sum->plain.size() != nout)) SFG_FAIL(ctx, "key switch: internal: malformed sum groups");
    if (!nr && !nout) return 0;
    const int nq_out = ff.on ? ff.L : nl;                       // moduli of the result that the finish stores: the rows of the others are not produced
    const bool pre1 = !ctx->cfg.ntt_fwd_full;                   // the extension kernels apply the forward transform's first stage (the split transform starts at stage 2)
    // inputs are processed in groups whose decomposition fits the budget (SFG_KSW_BUDGET_MB, 4 GiB by default), jobs of a group in chunks whose acc / ext2 fit it:
    // the sizes, the workspace layout and the groups are ksw_plan.hpp's
    const KswSizes sz = ksw_plan_sizes(nl, kc.np, kc.nt, kc.beta, nin, nr, nout, ctx->cfg.ksw_budget, (size_t)N);
    std::vector<KswGroup> groups;
    ksw_plan_groups(jb.job_in.data(), jb.keyp.data(), jb.idxp.data(), nr, nin, sz.in_grp, sz.chunk, KSW_T, groups);
    SFG_TRY(sfg_ws_reserve(ctx, sz.at.bytes));
    u64 *const w = (u64 *)ctx->ws; char *const wb = (char *)ctx->ws;
    u64 *c2 = w + sz.at.c2, *ext = w + sz.at.ext, *acc = w + sz.at.acc, *ext2 = w + sz.at.ext2, *extT = w + sz.at.extT, *ext2T = w + sz.at.ext2T;
    const u64 **keys_all = (const u64 **)(wb + sz.at.keys); const uint16_t **idx_all = (const uint16_t **)(wb + sz.at.idx); u64 **out_all = (u64 **)(wb + sz.at.out);
    KswSeg *segs_d = (KswSeg *)(wb + sz.at.segs); int *inidx_all = (int *)(wb + sz.at.inidx), *segjobs_d = (int *)(wb + sz.at.segjobs);
    KswTile *tiles_all = (KswTile *)(wb + sz.at.tiles);
    std::vector<char> seen(nout, 0);                            // outputs of a sum that have been written by an earlier chunk
    std::vector<KswSegPlan> plan; std::vector<KswSeg> segs; std::vector<int> segjobs, grp;
    // the summed finish of the chunk's jobs [c0, c0 + nb) of the group's list (nb == 0: the outputs no job has touched); segments: ksw_plan.hpp
    auto finish_sum = [&](const std::vector<int> &jobs, size_t c0, int nb, const u64 *bin, const u64 **keys_d, const int *inidx_d, const uint16_t **idx_d) -> int {
        grp.resize(nb);
        for (int k = 0; k < nb; k++) grp[k] = jb.group[jobs[c0 + k]];
        ksw_plan_segments(grp.data(), nb, nout, seen, plan, segjobs);
        if (plan.empty()) return 0;
        segs.clear();
        for (const KswSegPlan &sp : plan) {
            KswSeg sg; sg.plain = sp.first ? sum->plain[sp.out] : nullptr; sg.out = sum->out + (size_t)sp.out * sum->out_stride;
            sg.start = sp.start; sg.count = sp.count; sg.accumulate = (sum->accumulate || !sp.first) ? 1 : 0; sg.pad = 0;
            segs.push_back(sg);
        }
        SFG_TRY(sfg_upload_small(ctx, segs_d, segs.data(), segs.size() * sizeof(KswSeg)));
        SFG_TRY(sfg_upload_small(ctx, segjobs_d, segjobs.data(), (size_t)nb * sizeof(int)));
        hipLaunchKernelGGL(k_ksw_finish_sum, dim3(N / 256, nl, (unsigned)segs.size()), dim3(256), 0, ctx->stream, extT, bin, keys_d, inidx_d, ext2T, idx_d,
                           segs_d, segjobs_d, kcd, ctx->modc, ctx->nmod);
        SFG_HIP(ctx, hipGetLastError());
        return 0;
    };
    ModPattern pq; pq.period = nl; for (int m = 0; m < nl; m++) pq.m[m] = m < nq_out ? (int8_t)m : (int8_t)-2;
    const ModPattern pin = mod_pattern_run(0, nl);
    ModPattern pext; pext.period = kc.beta * kc.nt;
    for (int i = 0; i < kc.beta; i++) for (int t = 0; t < kc.nt; t++)           // in-digit rows and the targets the finish does not store: nobody reads them
        pext.m[i * kc.nt + t] = (kc.digit_of[t] == i || (t >= nq_out && t < nl)) ? (int8_t)-2 : (int8_t)kc.tmod[t];
    const ModPattern pp = mod_pattern_run(ctx->nq, kc.np);
    RowMap rm_dense; rm_dense.rpg = 1; rm_dense.gstride_in = N; rm_dense.gstride_out = N;
    for (const KswGroup &g : groups) {
        const int i0 = g.i0, ni = g.ni;
        const std::vector<int> &jobs = g.jobs;
        const u64 *bin = in + (size_t)i0 * ctw;
        // 1. c2 = INTT(c1) for every input of the group, without the last stage and 1/N
        RowMap rm1; rm1.rpg = nl; rm1.gstride_in = ctw; rm1.gstride_out = (size_t)nl * N;
        SFG_TRY(launch_ntt_inv_split(ctx, bin + (size_t)nl * N, c2, (size_t)ni * nl, pin, rm1));
        // 2. digit extension + NTT (in-digit rows are skipped by the pattern)
        if (pre1) hipLaunchKernelGGL(k_ksw_extend<true>, dim3(N / 512, kc.beta, ni), dim3(256), 0, ctx->stream, c2, ext, kcd, ctx->modc, ctx->tw_fwd, ctx->tw_inv);
        else hipLaunchKernelGGL(k_ksw_extend<false>, dim3(N / 512, kc.beta, ni), dim3(256), 0, ctx->stream, c2, ext, kcd, ctx->modc, ctx->tw_fwd, ctx->tw_inv);
        SFG_HIP(ctx, hipGetLastError());
        SFG_TRY(launch_ntt_fwd_staged(ctx, ext, extT, (size_t)ni * kc.beta * kc.nt, pext, pre1));
        // pointer tables and tiles of the whole group (group-local job numbers; a chunk's tiles: chunk-local): staged in the pinned ring, stream-ordered (no host
        // wait on the launch path)
        {
            const size_t nj = jobs.size();
            std::vector<const u64 *> kp(nj); std::vector<const uint16_t *> ip(nj); std::vector<u64 *> op(nj); std::vector<int> ii(nj);
            for (size_t k = 0; k < nj; k++) { int j = jobs[k]; kp[k] = jb.keyp[j]; ip[k] = jb.idxp[j]; op[k] = sum ? nullptr : jb.outp[j]; ii[k] = jb.job_in[j] - i0; }
            SFG_TRY(sfg_upload_small(ctx, keys_all, kp.data(), nj * sizeof(void *)));
            SFG_TRY(sfg_upload_small(ctx, idx_all, ip.data(), nj * sizeof(void *)));
            if (!sum) SFG_TRY(sfg_upload_small(ctx, out_all, op.data(), nj * sizeof(void *)));
            SFG_TRY(sfg_upload_small(ctx, inidx_all, ii.data(), nj * sizeof(int)));
            SFG_TRY(sfg_upload_small(ctx, tiles_all, g.tiles.data(), g.tiles.size() * sizeof(KswTile)));
        }
        for (const KswChunk &c : g.chunks) {
            const int nb = c.nb;
            const u64 **keys_d = keys_all + c.c0; const uint16_t **idx_d = idx_all + c.c0; u64 **out_d = out_all + c.c0; int *inidx_d = inidx_all + c.c0;
            const KswTile *tiles_d = tiles_all + c.tile0; const unsigned ntiles = (unsigned)c.ntiles;
            // 3. inner product with the key, special-prime targets only
            hipLaunchKernelGGL(k_ksw_inner_p<KSW_T>, dim3(N / 512, kc.np, ntiles), dim3(256), 0, ctx->stream, extT, keys_d, inidx_d, tiles_d, acc, kcd, ctx->modc, ctx->nmod);
            SFG_HIP(ctx, hipGetLastError());
            // 4. ModDown: INTT of the special rows in place (split: finished by the extension), extend to Q, NTT
            SFG_TRY(launch_ntt_inv_split(ctx, acc, acc, (size_t)nb * 2 * kc.np, pp, rm_dense));
            if (pre1) hipLaunchKernelGGL(k_moddown_extend<true>, dim3(N / 512, 2, nb), dim3(256), 0, ctx->stream, acc, ext2, kcd, ctx->modc, ctx->tw_fwd, ctx->tw_inv, nq_out);
            else hipLaunchKernelGGL(k_moddown_extend<false>, dim3(N / 512, 2, nb), dim3(256), 0, ctx->stream, acc, ext2, kcd, ctx->modc, ctx->tw_fwd, ctx->tw_inv, nq_out);
            SFG_HIP(ctx, hipGetLastError());
            SFG_TRY(launch_ntt_fwd_staged(ctx, ext2, ext2T, (size_t)nb * 2 * nl, pq, pre1));
            // 5. inner product of the Q targets + finish + automorphism
            if (sum) { SFG_TRY(finish_sum(jobs, (size_t)c.c0, nb, bin, keys_d, inidx_d, idx_d)); continue; }
            hipLaunchKernelGGL(k_ksw_finish<KSW_T>, dim3(N / 256, nq_out, ntiles), dim3(256), 0, ctx->stream, extT, bin, keys_d, inidx_d, ext2T, idx_d, out_d, tiles_d, kcd,
                               ctx->modc, ctx->nmod, add1 ? add1 + (size_t)i0 * nl * N : nullptr, ff);
            SFG_HIP(ctx, hipGetLastError());
        }
    }
    if (sum) SFG_TRY(finish_sum(std::vector<int>(), 0, 0, in, keys_all, inidx_all, idx_all));          // outputs without a job
    return 0;
}
// What the rotation front-ends share: job j rotates input src = in_index[j] (nullptr: j) right by nrot = nrot_host[j] mod SFG_SLOTS in [0, SFG_SLOTS); key: the
// switching key of that rotation (basics.go:205: RotateNew(ct, slots - nrot)), nullptr for nrot == 0, which each front-end treats in its own way.
struct RotJob { int nrot, src; const RotKey *key; };
static int resolve_rotation(sfg_ctx *ctx, const int *nrot_host, const int *in_index, int j, int nin, RotJob &r) {
    r.nrot = nrot_host[j] % SFG_SLOTS; if (r.nrot < 0) r.nrot += SFG_SLOTS;
    r.src = in_index ? in_index[j] : j; r.key = nullptr;
    if (r.src < 0 || r.src >= nin) SFG_FAIL(ctx, "rotate: input index out of range");
    if (r.nrot == 0) return 0;
    u64 g = sfg_galois_for_rotation(ctx, SFG_SLOTS - r.nrot);
    auto it = ctx->rotkeys().find(g);
    if (it == ctx->rotkeys().end()) SFG_FAIL(ctx, "rotate: no rotation key loaded for right-rotation by %d (galois element %llu)", r.nrot, g);
    r.key = &it->second;
    return 0;
}
// the run of unrotated jobs from job j (input src) on whose (source, slot) pairs are consecutive: one copy or conversion serves them all
static int unrotated_run(const int *nrot_host, const int *in_index, int j, int nct, int src, int nin) {
    int run = 1;
    while (j + run < nct && (nrot_host[j + run] % SFG_SLOTS) == 0 && (in_index ? in_index[j + run] : j + run) == src + run && src + run < nin) run++;
    return run;
}
// Rotate a batch.  `in` holds nin ciphertexts [nin][2][nl][N]; output j = RotateRight(in[in_index[j]], nrot[j])
// (RotateRightWithEvaluator semantics) written to out + j*ct words.  in_index == nullptr means identity (nin == nct).
int launch_rotate_right_indexed(sfg_ctx *ctx, const u64 *in, int nin, u64 *out, int nct, int level, const int *nrot_host, const int *in_index) {
    if (level < 0 || level >= ctx->nq) SFG_FAIL(ctx, "rotate: level out of range");
    const size_t ctw = (size_t)2 * (level + 1) * SFG_N;
    KswBatch bt{in, nin, level}; KswJobs jb; RotJob r;
    for (int j = 0; j < nct; j++) {
        SFG_TRY(resolve_rotation(ctx, nrot_host, in_index, j, nin, r));
        if (r.key) { jb.add(r.src, *r.key, out + j * ctw); continue; }
        const int run = unrotated_run(nrot_host, in_index, j, nct, r.src, nin);      // not rotated: copied
        SFG_HIP(ctx, hipMemcpyAsync(out + j * ctw, in + (size_t)r.src * ctw, (size_t)run * ctw * 8, hipMemcpyDeviceToDevice, ctx->stream));
        j += run - 1;
    }
    return launch_keyswitch_jobs(ctx, bt, jb);
}
// The same batch SUMMED where it is produced: out + i * out_stride (+)= sum over the jobs j with group[j] == i of RotateRight(in[in_index[j]], nrot[j]), i < nout.
// A job that does not rotate joins its sum as a plain read (one per output).  No rotated ciphertext is stored.  `out` must not overlap `in`.
int launch_rotate_right_sum(sfg_ctx *ctx, const u64 *in, int nin, int nct, int level, const int *nrot_host, const int *in_index, const int *group, int nout,
                            u64 *out, size_t out_stride, int accumulate) {
    if (level < 0 || level >= ctx->nq) SFG_FAIL(ctx, "rotate: level out of range");
    const size_t ctw = (size_t)2 * (level + 1) * SFG_N;
    KswSum sum; sum.nout = nout; sum.plain.assign(nout, nullptr); sum.out = out; sum.out_stride = out_stride; sum.accumulate = accumulate;
    KswBatch bt{in, nin, level}; bt.sum = &sum; KswJobs jb; RotJob r;
    for (int j = 0; j < nct; j++) {
        if (group[j] < 0 || group[j] >= nout) SFG_FAIL(ctx, "rotate: sum group out of range");
        SFG_TRY(resolve_rotation(ctx, nrot_host, in_index, j, nin, r));
        if (r.key) { jb.add(r.src, *r.key, nullptr, group[j]); continue; }
        if (sum.plain[group[j]]) SFG_FAIL(ctx, "rotate: more than one unrotated member in a sum group");
        sum.plain[group[j]] = in + (size_t)r.src * ctw;                                // not rotated: the sum's plain member
    }
    return launch_keyswitch_jobs(ctx, bt, jb);
}
// The same batch written as the MAC's fp64 operand rows: job j lands at outf + j * 2 * rowf (row pair of polynomials 0, 1), rowf = nplanes * N doubles.
// Jobs that do not rotate (nrot == 0) are converted from their input.
// out_slot (nullable): job j lands at outf + out_slot[j] * 2 * rowf instead of outf + j * 2 * rowf (sharded rotation-cache builds write job-major staging).
int launch_rotate_right_indexed_f64(sfg_ctx *ctx, const u64 *in, int nin, double *outf, int nct, int level, const int *nrot_host, const int *in_index, int L,
                                    const size_t *out_slot) {
    const int N = SFG_N, nl = level + 1;
    ctx->i8_gen++;                  // fp64 rot operand rows are (re)written: the int8 MAC's transposed copy of whatever buffer this is goes stale
    if (level < 0 || level >= ctx->nq || L > nl) SFG_FAIL(ctx, "rotate: level out of range");
    const size_t ctw = (size_t)2 * nl * N;
    std::vector<int> plane_of, is_big; const int nplanes = mac_dma_planes(ctx, L, plane_of, is_big);
    if (nplanes < 0) return 1;
    F64Form ff; memset(&ff, 0, sizeof ff);
    ff.on = 1; ff.L = L; ff.centre = mac_dma_packed_mask(ctx, L) != 0; ff.rowf = (size_t)nplanes * N;
    for (int l = 0; l < L; l++) { ff.plane_of[l] = plane_of[l]; ff.big[l] = is_big[l]; }
    KswBatch bt{in, nin, level}; bt.ff = &ff; KswJobs jb; RotJob r;
    for (int j = 0; j < nct; j++) {
        SFG_TRY(resolve_rotation(ctx, nrot_host, in_index, j, nin, r));
        double *dst = outf + (out_slot ? out_slot[j] : (size_t)j) * 2 * ff.rowf;
        if (r.key) { jb.add(r.src, *r.key, reinterpret_cast<u64 *>(dst)); continue; }
        const int run = out_slot ? 1 : unrotated_run(nrot_host, in_index, j, nct, r.src, nin);      // not rotated: converted from the input
        SFG_TRY(launch_rot_to_f64(ctx, in + (size_t)r.src * ctw, (size_t)2 * run, nl, L, dst));
        j += run - 1;
    }
    return launch_keyswitch_jobs(ctx, bt, jb);
}
// relinearisation: out[i] = (tmp[i].p0 + d0, mid[i] + d1) with (d0, d1) = key switch of tmp[i].p1 under the key stored at Galois element 1
int launch_relinearize(sfg_ctx *ctx, const u64 *tmp, int nct, int level, const u64 *mid, u64 *out) {
    auto it = ctx->rotkeys().find(1);
    if (it == ctx->rotkeys().end()) SFG_FAIL(ctx, "relinearize: no relinearisation key loaded");
    KswBatch bt{tmp, nct, level}; bt.add1 = mid;
    return launch_keyswitch_jobs(ctx, bt, KswJobs(nct, it->second, out, (size_t)2 * (level + 1) * SFG_N));
}
int launch_rotate_right(sfg_ctx *ctx, const u64 *in, u64 *out, int nct, int level, const int *nrot_host) {
    return launch_rotate_right_indexed(ctx, in, nct, out, nct, level, nrot_host, nullptr);
}

extern "C" int sfg_rotate_right_dev(sfg_ctx *ctx, const uint64_t *in, uint64_t *out, int nct, int level, const int *nrot_host) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (in == out) SFG_FAIL(ctx, "rotate: in and out must not alias");
    PhaseTimer t(ctx, "rotate");
    int rc = launch_rotate_right(ctx, (const u64 *)in, (u64 *)out, nct, level, nrot_host);
    t.stop(1);
    return rc;
}

// eval.ConjugateNew (crypto.ComplexConjugate / CReal, basics.go:826-846) and any other automorphism X -> X^g whose switching key was loaded under g
// (lattigo: g = 2N-1 conjugates the slots)
extern "C" int sfg_ct_galois_dev(sfg_ctx *ctx, const uint64_t *in, uint64_t *out, int nct, int level, uint64_t galois_el) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (in == out) SFG_FAIL(ctx, "galois: in and out must not alias");
    if (level < 0 || level >= ctx->nq) SFG_FAIL(ctx, "galois: level out of range");
    auto it = ctx->rotkeys().find(galois_el);
    if (it == ctx->rotkeys().end() || galois_el == 1) SFG_FAIL(ctx, "galois: no switching key loaded for galois element %llu", (unsigned long long)galois_el);
    PhaseTimer t(ctx, "rotate");
    int rc = launch_keyswitch_jobs(ctx, KswBatch{(const u64 *)in, nct, level}, KswJobs(nct, it->second, (u64 *)out, (size_t)2 * (level + 1) * SFG_N));
    t.stop(1);
    return rc;
}

int launch_ct_add(sfg_ctx *ctx, const u64 *a, const u64 *b, u64 *out, size_t nct, int level) {
    const int nl = level + 1; const size_t rows = nct * 2 * nl;
    if (!rows) return 0;
    hipLaunchKernelGGL(k_ct_add, dim3((unsigned)(rows * (SFG_N / 256))), dim3(256), 0, ctx->stream, a, b, out, nl, ctx->modc, rows);
    SFG_HIP(ctx, hipGetLastError());
    return 0;
}
extern "C" int sfg_ct_add_dev(sfg_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, int nct, int level) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (level < 0 || level >= ctx->nq) SFG_FAIL(ctx, "evaluator op: level %d out of range", level);
    if (nct < 0) SFG_FAIL(ctx, "evaluator op: negative ciphertext count");
    return launch_ct_add(ctx, (const u64 *)a, (const u64 *)b, (u64 *)out, (size_t)nct, level);
}
