// gring.hip - the general ring: evaluator operations for logN 12..16 and any NTT-friendly modulus below 2^61, in integer arithmetic.
// A second path beside the PN14QP438 context (whose kernels are specialised for N = 16384 and residues held exactly in fp64): nothing here is shared with it
// but the C-ABI's layouts.  Arithmetic and bounds: gring_arith.hpp.  Stage split, digits, launch caps, workspace layouts and chunks: gring_plan.hpp.  DESIGN.md section 13.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "gring_dev.hpp"      // the device-side tables, the owners, struct sfg_ring and the error macros, shared with gring_io.hip

// ---------------------------------------------------------------- the transform: two launches, logN = a + b (gring_plan.hpp)
// Twiddle tables tw[mod][4][N]: psi^brev forward, its Shoup quotients, psi^-brev inverse, its Shoup quotients - lattigo's and the oracle's order
// (natural in, bit-reversed out).  A workgroup holds 4096 words (32 KiB) in LDS; stage loops are runtime loops over LDS, no per-thread arrays.
// Bounds: forward words stay in [0, 4q), inverse words in [0, 2q) (gring_arith.hpp); the last pass of each direction stores canonical words.
// tile index < 4096 by construction; global index < N: the columns pass reads (r << b) + c0 + c with r < 2^a, c0 + c < 2^b; the contiguous pass reads
// blockIdx.x * 4096 + e with blockIdx.x < N / 4096.
template <bool INV>
__global__ __launch_bounds__(GR_T) void k_gr_cols(u64 *rows, size_t row0, GrRowMap map, const GrMod *modc, const u64 *tw, int logN, int a, int b) {
    __shared__ u64 tile[GrNttPlan::kTileWords];
    const size_t row = row0 + blockIdx.y;
    const int mod = gr_row_mod(map, row), N = 1 << logN;
    const GrMod mc = modc[mod];
    const u64 q = mc.q;
    const u64 *w = tw + ((size_t)mod * 4 + (INV ? 2 : 0)) * N, *wsh = w + N;
    u64 *base = rows + row * (size_t)N;
    const int lg = 12 - a, G = 1 << lg, c0 = blockIdx.x * G;                // G adjacent columns: G * 8 >= 128 contiguous bytes per row segment
    for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T) tile[e] = base[((size_t)(e >> lg) << b) + c0 + (e & (G - 1))];
    __syncthreads();
    // row distance h: forward 2^(a-1) .. 1, inverse 1 .. 2^(a-1); the butterflies of distance h use twiddle 2^(a-1) / h + (group index)
    for (int s = 0; s < a; s++) {
        const int lh = INV ? s : a - 1 - s, h = 1 << lh, tw0 = 1 << (a - 1 - lh);
        for (int k = threadIdx.x; k < GrNttPlan::kTileWords / 2; k += GR_T) {
            const int c = k & (G - 1), p = k >> lg, i = p >> lh, r = (i << (lh + 1)) + (p & (h - 1));
            u64 X = tile[(r << lg) + c], Y = tile[((r + h) << lg) + c];
            if (INV) gr::bfly_inv(X, Y, w[tw0 + i], wsh[tw0 + i], q); else gr::bfly_fwd(X, Y, w[tw0 + i], wsh[tw0 + i], q);
            tile[(r << lg) + c] = X; tile[((r + h) << lg) + c] = Y;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T) {
        u64 v = tile[e];
        if (INV) v = gr::shoup(v, mc.ninv, mc.ninv_sh, q);                 // last pass of the inverse: times N^-1, canonical
        base[((size_t)(e >> lg) << b) + c0 + (e & (G - 1))] = v;
    }
}
template <bool INV>
__global__ __launch_bounds__(GR_T) void k_gr_contig(u64 *rows, size_t row0, GrRowMap map, const GrMod *modc, const u64 *tw, int logN, int a, int b) {
    __shared__ u64 tile[GrNttPlan::kTileWords];
    const size_t row = row0 + blockIdx.y;
    const int mod = gr_row_mod(map, row), N = 1 << logN;
    const u64 q = modc[mod].q;
    const u64 *w = tw + ((size_t)mod * 4 + (INV ? 2 : 0)) * N, *wsh = w + N;
    u64 *base = rows + row * (size_t)N + (size_t)blockIdx.x * GrNttPlan::kTileWords;
    const int chunk0 = blockIdx.x << (12 - b);                              // index of this tile's first sub-transform of 2^b words in the row
    for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T) tile[e] = base[e];
    __syncthreads();
    // distance t: forward 2^(b-1) .. 1, inverse 1 .. 2^(b-1); twiddle (2^(b-1) / t) (2^a + chunk) + (group index inside the chunk)
    for (int s = 0; s < b; s++) {
        const int lt = INV ? s : b - 1 - s, t = 1 << lt, lm = b - 1 - lt;
        for (int k = threadIdx.x; k < GrNttPlan::kTileWords / 2; k += GR_T) {
            const int ch = k >> (b - 1), bb = k & ((1 << (b - 1)) - 1), i = bb >> lt, j = (ch << b) + (i << (lt + 1)) + (bb & (t - 1));
            const int ti = (((1 << a) + chunk0 + ch) << lm) + i;            // < 2^(a + b) = N
            u64 X = tile[j], Y = tile[j + t];
            if (INV) gr::bfly_inv(X, Y, w[ti], wsh[ti], q); else gr::bfly_fwd(X, Y, w[ti], wsh[ti], q);
            tile[j] = X; tile[j + t] = Y;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < GrNttPlan::kTileWords; e += GR_T) base[e] = INV ? tile[e] : gr::canon4(tile[e], q);   // last pass of the forward transform: canonical
}

// ---------------------------------------------------------------- basis extension (three element-wise kernels; x < N guarded by the grid: N is a multiple of 256)
// y_m = x_m (D / q_m)^-1 mod q_m, canonical
__global__ __launch_bounds__(GR_T) void k_gr_ext_y(const u64 *src, u64 *Y, GrExt e, const GrMod *modc, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, r = blockIdx.y; const size_t o = ((size_t)blockIdx.z * e.nsrc + r) * N + x;
    Y[o] = gr::shoup(src[o], e.inv[2 * r], e.inv[2 * r + 1], modc[e.src_mod[r]].q);
}
// v = uint64(sum_m (double)y_m / (double)q_m), summed in modulus order; a single-modulus digit is a raw copy: v = 0
__global__ __launch_bounds__(GR_T) void k_gr_ext_v(const u64 *Y, uint32_t *V, GrExt e, const GrMod *modc, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, i = blockIdx.y, st = i * e.alpha, len = min(e.alpha, e.nsrc - st);
    double vf = 0.0;
    for (int m = 0; m < len; m++) vf = gr::ext_accumulate(vf, Y[((size_t)blockIdx.z * e.nsrc + st + m) * N + x], modc[e.src_mod[st + m]].q);
    V[((size_t)blockIdx.z * e.ndig + i) * N + x] = len == 1 ? 0u : (uint32_t)gr::ext_truncate(vf);
}
// out[poly][digit][target] = sum_m y_m (D / q_m) - v D mod qt; a target that is one of the digit's own moduli gets the source row itself
__global__ __launch_bounds__(GR_T) void k_gr_ext_out(const u64 *src, const u64 *Y, const uint32_t *V, u64 *out, GrExt e, const GrMod *modc, int ntgt, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, i = blockIdx.y / ntgt, t = blockIdx.y % ntgt, st = i * e.alpha, len = min(e.alpha, e.nsrc - st);
    const size_t po = (size_t)blockIdx.z * e.nsrc * N, oo = (((size_t)blockIdx.z * e.ndig + i) * ntgt + t) * N + x;
    const int own = e.tgt_src[i * e.tgt_cap + t];
    if (own >= 0) { out[oo] = src[po + (size_t)own * N + x]; return; }       // uniform over the workgroup
    const GrMod mc = modc[e.tgt_mod[t]];
    const u64 *tab = e.tgt_tab + ((size_t)i * e.tgt_cap + t) * (1 + e.alpha);
    u128 S = 0;                                                             // len <= 47 terms below 2^61 * 2^61: S < 2^128
    for (int m = 0; m < len; m++) S += (u128)Y[po + (size_t)(st + m) * N + x] * tab[1 + m];
    out[oo] = gr::ext_finish(S, V[((size_t)blockIdx.z * e.ndig + i) * N + x], tab[0], mc.q, mc.uhi, mc.ulo);
}

// ---------------------------------------------------------------- key switch
__global__ __launch_bounds__(GR_T) void k_gr_gather_c1(const u64 *in, u64 *c2, const GrJob *jobs, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y; const size_t ct = (size_t)jobs[blockIdx.z].ct;
    c2[((size_t)blockIdx.z * nl + m) * N + x] = in[((ct * 2 + 1) * nl + m) * N + x];
}
// out0 = a0 b0, out1 = a0 b1 + a1 b0 (two products below 2^122 summed in 128 bits, one reduction), c2 = a1 b1
__global__ __launch_bounds__(GR_T) void k_gr_tensor(const u64 *a, const u64 *b, u64 *out, u64 *c2, const GrMod *modc, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y; const GrMod mc = modc[m];
    const size_t o0 = (((size_t)blockIdx.z * 2) * nl + m) * N + x, o1 = o0 + (size_t)nl * N;
    const u64 a0 = a[o0], a1 = a[o1], b0 = b[o0], b1 = b[o1];
    out[o0] = gr::mulmod(a0, b0, mc.q, mc.uhi, mc.ulo);
    u128 S = (u128)a0 * b1 + (u128)a1 * b0;
    out[o1] = gr::barrett128((u64)(S >> 64), (u64)S, mc.q, mc.uhi, mc.ulo);
    c2[((size_t)blockIdx.z * nl + m) * N + x] = gr::mulmod(a1, b1, mc.q, mc.uhi, mc.ulo);
}
// acc[p][t] = sum over the beta digits of ext[digit][t] * key[digit][p][mod(t)]: the sum stays unreduced in 128 bits (beta <= 48 terms below 2^122) and reduces once
__global__ __launch_bounds__(GR_T) void k_gr_keyip(const u64 *ext, const GrJob *jobs, u64 *accQ, u64 *accP, const GrMod *modc, int beta, int nl, int nq, int np, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, t = blockIdx.y, nt = nl + np, mod = t < nl ? t : nq + (t - nl), nmod = nq + np;
    const GrMod mc = modc[mod]; const u64 *key = jobs[blockIdx.z].key;
    u128 S0 = 0, S1 = 0;
    for (int i = 0; i < beta; i++) {
        const u64 e = ext[(((size_t)blockIdx.z * beta + i) * nt + t) * N + x];
        S0 += (u128)e * key[(((size_t)i * 2 + 0) * nmod + mod) * N + x];
        S1 += (u128)e * key[(((size_t)i * 2 + 1) * nmod + mod) * N + x];
    }
    const u64 r0 = gr::barrett128((u64)(S0 >> 64), (u64)S0, mc.q, mc.uhi, mc.ulo), r1 = gr::barrett128((u64)(S1 >> 64), (u64)S1, mc.q, mc.uhi, mc.ulo);
    if (t < nl) { accQ[(((size_t)blockIdx.z * 2 + 0) * nl + t) * N + x] = r0; accQ[(((size_t)blockIdx.z * 2 + 1) * nl + t) * N + x] = r1; }
    else { accP[(((size_t)blockIdx.z * 2 + 0) * np + (t - nl)) * N + x] = r0; accP[(((size_t)blockIdx.z * 2 + 1) * np + (t - nl)) * N + x] = r1; }
}
// ModDown's last step and what follows it: d = (accQ - ext) P^-1; plus `add` (the rotation's c0, the product's tensor terms) where add_mask has the polynomial's
// bit; read through the job's automorphism index (out[x] = d[index[x]]) when it has one
__global__ __launch_bounds__(GR_T) void k_gr_ks_finish(const u64 *accQ, const u64 *ext2, const GrJob *jobs, const u64 *pinv, const u64 *add, int add_mask, u64 *out,
                                                       const GrMod *modc, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, t = blockIdx.y, p = blockIdx.z & 1; const size_t job = blockIdx.z >> 1;
    const GrJob jb = jobs[job]; const u64 q = modc[t].q;
    const int xs = jb.idx ? (int)jb.idx[x] : x;                              // index table entries < N (built on the host from brev of values < N)
    const size_t w = ((size_t)blockIdx.z * nl + t) * N + xs, o = (((size_t)jb.ct * 2 + p) * nl + t) * N;
    u64 d = gr::shoup(gr::submod(accQ[w], ext2[w], q), pinv[2 * t], pinv[2 * t + 1], q);
    if ((add_mask >> p) & 1) d = gr::addmod(d, add[o + xs], q);
    out[o + x] = d;
}

// ---------------------------------------------------------------- rescale (ring.DivRoundByLastModulusNTT)
__global__ __launch_bounds__(GR_T) void k_gr_copy_last(const u64 *in, u64 *T, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x; T[(size_t)blockIdx.z * N + x] = in[((size_t)blockIdx.z * nl + nl - 1) * N + x];
}
// tab[m] = {hneg = q_m - (half mod q_m), qL^-1 mod q_m, its Shoup quotient}
__global__ __launch_bounds__(GR_T) void k_gr_rescale_prep(const u64 *T, u64 *tmp, const u64 *tab, const GrMod *modc, int level, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y; const GrMod mc = modc[m]; const u64 qL = modc[level].q;
    u64 v = gr::addmod(T[(size_t)blockIdx.z * N + x], (qL - 1) >> 1, qL);
    tmp[((size_t)blockIdx.z * level + m) * N + x] = gr::addmod(gr::barrett128(0, v, mc.q, mc.uhi, mc.ulo), tab[3 * m] == mc.q ? 0 : tab[3 * m], mc.q);
}
__global__ __launch_bounds__(GR_T) void k_gr_rescale_fin(const u64 *in, const u64 *tmp, u64 *out, const u64 *tab, const GrMod *modc, int level, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y; const u64 q = modc[m].q;
    const u64 d = gr::submod(in[((size_t)blockIdx.z * (level + 1) + m) * N + x], tmp[((size_t)blockIdx.z * level + m) * N + x], q);
    out[((size_t)blockIdx.z * level + m) * N + x] = gr::shoup(d, tab[3 * m + 1], tab[3 * m + 2], q);
}

// ---------------------------------------------------------------- element-wise operations; grid (N / 256, level_out + 1, nct * 2)
enum GrOp { GR_ADD, GR_SUB, GR_DROP, GR_MULS, GR_MULSADD, GR_ADDS, GR_ADDP, GR_MULP };
template <int OP>
__global__ __launch_bounds__(GR_T) void k_gr_ew(const u64 *a, const u64 *b, u64 *out, GrScalars sc, size_t pt_stride, const GrMod *modc, int nl_in, int nl_out, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y, p = blockIdx.z & 1; const size_t ct = blockIdx.z >> 1;
    const GrMod mc = modc[m];
    const size_t i = ((size_t)blockIdx.z * nl_in + m) * N + x, o = ((size_t)blockIdx.z * nl_out + m) * N + x, pi = ct * pt_stride + (size_t)m * N + x;
    u64 v;
    if (OP == GR_ADD) v = gr::addmod(a[i], b[i], mc.q);
    else if (OP == GR_SUB) v = gr::submod(a[i], b[i], mc.q);
    else if (OP == GR_DROP) v = a[i];
    else if (OP == GR_MULS) v = gr::mulmod(a[i], sc.s[m], mc.q, mc.uhi, mc.ulo);
    else if (OP == GR_MULSADD) v = gr::addmod(out[o], gr::mulmod(a[i], sc.s[m], mc.q, mc.uhi, mc.ulo), mc.q);
    else if (OP == GR_ADDS) v = p ? a[i] : gr::addmod(a[i], sc.s[m], mc.q);
    else if (OP == GR_ADDP) v = p ? a[i] : gr::addmod(a[i], b[pi], mc.q);
    else v = gr::mulmod(a[i], b[pi], mc.q, mc.uhi, mc.ulo);
    out[o] = v;
}
// lattigo ring.InvMForm: x 2^-64 mod q on key rows [.][nmod][N]
__global__ __launch_bounds__(GR_T) void k_gr_from_mont(u64 *rows, const GrMod *modc, int nmod, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x; const GrMod mc = modc[blockIdx.y % nmod];
    u64 *p = rows + (size_t)blockIdx.y * N + x; *p = gr::shoup(*p, mc.r64inv, mc.r64inv_sh, mc.q);
}

// ---------------------------------------------------------------- host side
static thread_local std::string g_ring_create_error;

static bool hm_is_prime(u64 n) {            // Miller-Rabin, deterministic below 2^64 with the first twelve primes as bases
    if (n < 2) return false;
    for (u64 p : {2ULL, 3ULL, 5ULL, 7ULL, 11ULL, 13ULL, 17ULL, 19ULL, 23ULL, 29ULL, 31ULL, 37ULL}) { if (n % p == 0) return n == p; }
    u64 d = n - 1; int s = 0; while (!(d & 1)) { d >>= 1; s++; }
    for (u64 a : {2ULL, 3ULL, 5ULL, 7ULL, 11ULL, 13ULL, 17ULL, 19ULL, 23ULL, 29ULL, 31ULL, 37ULL}) {
        u64 x = hm_pow(a, d, n); if (x == 1 || x == n - 1) continue;
        bool comp = true; for (int i = 1; i < s && comp; i++) { x = hm_mul(x, x, n); if (x == n - 1) comp = false; }
        if (comp) return false;
    }
    return true;
}
// smallest primitive root g of the prime q, psi = g^((q-1)/2N): how lattigo's ring.NewRing derives its 2N-th root
static u64 hm_derive_psi(u64 q, int logN) {
    u64 phi = q - 1, n = phi; std::vector<u64> fac;
    for (u64 p = 2; p * p <= n; p += (p == 2 ? 1 : 2)) if (n % p == 0) { fac.push_back(p); while (n % p == 0) n /= p; }
    if (n > 1) fac.push_back(n);
    for (u64 g = 2;; g++) {
        bool ok = true;
        for (u64 f : fac) if (hm_pow(g, phi / f, q) == 1) { ok = false; break; }
        if (ok) return hm_pow(g, phi >> (logN + 1), q);
    }
}

// stream-ordered upload of a small host table through the pinned ring (the host array may die at return)
int gr_upload(sfg_ring *r, void *dst, const void *src, size_t bytes) {
    if (!bytes) return 0;
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (need > r->pin_bytes) { GR_HIP(r, hipStreamSynchronize(r->stream)); GR_HIP(r, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return 0; }
    if (r->pin_head + need > r->pin_bytes) { GR_HIP(r, hipStreamSynchronize(r->stream)); r->pin_head = 0; }
    unsigned char *slot = (unsigned char *)r->pin.h + r->pin_head; r->pin_head += need;
    memcpy(slot, src, bytes);
    GR_HIP(r, hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, r->stream));
    return 0;
}
int gr_reserve(sfg_ring *r, GrMem &buf, size_t bytes) {
    if (bytes <= buf.bytes) return 0;
    GR_HIP(r, hipStreamSynchronize(r->stream));
    if (buf.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); GR_FAIL(r, "out of device memory: %zu bytes of workspace", bytes); }
    return 0;
}
int gr_table(sfg_ring *r, GrMem &dst, const void *host, size_t bytes) {
    GR_HIP(r, dst.alloc(bytes));
    GR_HIP(r, hipMemcpy(dst.p, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

static int gr_build_ext(sfg_ring *r, GrExtOwner &o, const std::vector<int> &src, int alpha, const std::vector<int> &tgt) {
    const int nsrc = (int)src.size(), ntgt = (int)tgt.size(), ndig = gr_digits(nsrc - 1, alpha).beta;
    std::vector<u64> inv((size_t)nsrc * 2), tab((size_t)ndig * ntgt * (1 + alpha), 0);
    std::vector<int> tsrc((size_t)ndig * ntgt, -1);
    for (int i = 0; i < ndig; i++) {
        const int st = i * alpha, len = std::min(alpha, nsrc - st);
        for (int m = 0; m < len; m++) {
            const u64 qm = r->q[src[st + m]]; u64 h = 1;
            for (int k = 0; k < len; k++) if (k != m) h = hm_mul(h, r->q[src[st + k]] % qm, qm);
            const u64 hi = hm_inv(h, qm);
            inv[2 * (st + m)] = hi; inv[2 * (st + m) + 1] = hm_shoup(hi, qm);
        }
        for (int t = 0; t < ntgt; t++) {
            const u64 qt = r->q[tgt[t]]; u64 *row = tab.data() + ((size_t)i * ntgt + t) * (1 + alpha);
            u64 D = 1 % qt;
            for (int m = 0; m < len; m++) {
                D = hm_mul(D, r->q[src[st + m]] % qt, qt);
                u64 ht = 1 % qt;
                for (int k = 0; k < len; k++) if (k != m) ht = hm_mul(ht, r->q[src[st + k]] % qt, qt);
                row[1 + m] = ht;
                if (src[st + m] == tgt[t]) tsrc[(size_t)i * ntgt + t] = st + m;
            }
            row[0] = D;
        }
    }
    const size_t b_src = (size_t)nsrc * 4, b_inv = inv.size() * 8, b_tm = (size_t)ntgt * 4, b_ts = tsrc.size() * 4, b_tab = tab.size() * 8;
    auto up8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    const size_t o_inv = 0, o_tab = o_inv + b_inv, o_src = o_tab + b_tab, o_tm = o_src + up8(b_src), o_ts = o_tm + up8(b_tm), total = o_ts + up8(b_ts);
    std::vector<unsigned char> host(total, 0);
    memcpy(host.data() + o_inv, inv.data(), b_inv); memcpy(host.data() + o_tab, tab.data(), b_tab); memcpy(host.data() + o_src, src.data(), b_src);
    memcpy(host.data() + o_tm, tgt.data(), b_tm); memcpy(host.data() + o_ts, tsrc.data(), b_ts);
    GR_TRY(gr_table(r, o.buf, host.data(), total));
    unsigned char *d = (unsigned char *)o.buf.p;
    o.e.nsrc = nsrc; o.e.ndig = ndig; o.e.alpha = alpha; o.e.tgt_cap = ntgt;
    o.e.inv = (const u64 *)(d + o_inv); o.e.tgt_tab = (const u64 *)(d + o_tab); o.e.src_mod = (const int *)(d + o_src);
    o.e.tgt_mod = (const int *)(d + o_tm); o.e.tgt_src = (const int *)(d + o_ts);
    return 0;
}
// the tables of one level, built at its first use: the digits' extension to Q_level + P and the rescale's constants
static int gr_level(sfg_ring *r, int level, GrLevel **out) {
    auto it = r->levels.find(level);
    if (it == r->levels.end()) {
        GrLevel L; const int nl = level + 1;
        std::vector<int> src(nl), tgt(nl + r->np);
        for (int m = 0; m < nl; m++) src[m] = tgt[m] = m;
        for (int p = 0; p < r->np; p++) tgt[nl + p] = r->nq + p;
        GR_TRY(gr_build_ext(r, L.up, src, r->np, tgt));
        std::vector<u64> tab((size_t)3 * std::max(level, 1), 0);
        const u64 qL = r->q[level], half = (qL - 1) >> 1;
        for (int m = 0; m < level; m++) { const u64 q = r->q[m], li = hm_inv(qL % q, q); tab[3 * m] = q - half % q; tab[3 * m + 1] = li; tab[3 * m + 2] = hm_shoup(li, q); }
        GR_TRY(gr_table(r, L.rescale_tab, tab.data(), tab.size() * 8));
        it = r->levels.emplace(level, std::move(L)).first;                   // complete: a failure above let the local tables go
    }
    *out = &it->second;
    return 0;
}

int gr_transform(sfg_ring *r, u64 *rows, size_t nrows, GrRowMap map, bool inv) {
    const GrNttPlan &p = r->plan;
    gr_split(nrows, kGrLaunchCap, [&](size_t row0, size_t n) {
        dim3 grid((unsigned)p.tiles_per_row, (unsigned)n);
        if (!inv) {
            hipLaunchKernelGGL(k_gr_cols<false>, grid, dim3(GR_T), 0, r->stream, rows, row0, map, r->modc, r->tw, p.logN, p.a, p.b);
            hipLaunchKernelGGL(k_gr_contig<false>, grid, dim3(GR_T), 0, r->stream, rows, row0, map, r->modc, r->tw, p.logN, p.a, p.b);
        } else {
            hipLaunchKernelGGL(k_gr_contig<true>, grid, dim3(GR_T), 0, r->stream, rows, row0, map, r->modc, r->tw, p.logN, p.a, p.b);
            hipLaunchKernelGGL(k_gr_cols<true>, grid, dim3(GR_T), 0, r->stream, rows, row0, map, r->modc, r->tw, p.logN, p.a, p.b);
        }
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return 0;
}
int gr_transform_cols_fwd(sfg_ring *r, u64 *rows, size_t nrows, GrRowMap map) {
    const GrNttPlan &p = r->plan;
    gr_split(nrows, kGrLaunchCap, [&](size_t row0, size_t n) {
        hipLaunchKernelGGL(k_gr_cols<false>, dim3((unsigned)p.tiles_per_row, (unsigned)n), dim3(GR_T), 0, r->stream, rows, row0, map, r->modc, r->tw, p.logN, p.a, p.b);
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return 0;
}
GrRowMap gr_map(int period, int split, int base0, int base1) { GrRowMap m; m.table = nullptr; m.period = period; m.split = split; m.base0 = base0; m.base1 = base1; return m; }

// basis extension of npoly polynomials: src [npoly][nsrc][N] (coefficient domain) -> out [npoly][ndig][ntgt][N] (coefficient domain)
int gr_extend(sfg_ring *r, const GrExt &e, const u64 *src, u64 *Y, uint32_t *V, u64 *out, int ntgt, size_t npoly) {
    const unsigned gx = r->N / GR_T;
    hipLaunchKernelGGL(k_gr_ext_y, dim3(gx, e.nsrc, (unsigned)npoly), dim3(GR_T), 0, r->stream, src, Y, e, r->modc, r->N);
    hipLaunchKernelGGL(k_gr_ext_v, dim3(gx, e.ndig, (unsigned)npoly), dim3(GR_T), 0, r->stream, Y, V, e, r->modc, r->N);
    hipLaunchKernelGGL(k_gr_ext_out, dim3(gx, e.ndig * ntgt, (unsigned)npoly), dim3(GR_T), 0, r->stream, src, Y, V, out, e, r->modc, ntgt, r->N);
    GR_HIP(r, hipGetLastError());
    return 0;
}

// workspace of one chunk of key switches (GrKsWs, gring_dev.hpp): the regions of gr_ks_layout (gring_plan.hpp) in the ring's workspace
GrKsWs gr_ks_ws(void *ws, const GrKsLayout &l) {
    u64 *p = (u64 *)ws;
    return GrKsWs{p + l.c2, p + l.Y, p + l.ext, p + l.accQ, p + l.accP, p + l.Y2, p + l.ext2, (uint32_t *)(p + l.V), (uint32_t *)(p + l.V2), (GrJob *)(p + l.jobs)};
}
// lattigo switchKeysInPlace on J jobs whose c2 rows (NTT domain) are in w.c2 and whose job list is uploaded: out[ct][p] = d_p (+ add[ct][p] where add_mask says so),
// read through the job's automorphism index
int gr_keyswitch(sfg_ring *r, int level, size_t J, const GrKsWs &w, const u64 *add, int add_mask, u64 *out) {
    const int nl = level + 1, np = r->np, nt = nl + np, N = r->N; const unsigned gx = N / GR_T;
    GrLevel *L; GR_TRY(gr_level(r, level, &L));
    const int beta = L->up.e.ndig;
    GR_TRY(gr_transform(r, w.c2, J * nl, gr_map(nl, nl, 0, 0), true));
    GR_TRY(gr_extend(r, L->up.e, w.c2, w.Y, w.V, w.ext, nt, J));
    GR_TRY(gr_transform(r, w.ext, J * beta * nt, gr_map(nt, nl, 0, r->nq), false));      // a digit's own moduli transform back to the input's rows: NTT(INTT(x)) = x on canonical words
    hipLaunchKernelGGL(k_gr_keyip, dim3(gx, nt, (unsigned)J), dim3(GR_T), 0, r->stream, w.ext, w.jobs, w.accQ, w.accP, r->modc, beta, nl, r->nq, np, N);
    GR_TRY(gr_transform(r, w.accP, J * 2 * np, gr_map(np, np, r->nq, 0), true));
    GR_TRY(gr_extend(r, r->down.e, w.accP, w.Y2, w.V2, w.ext2, nl, J * 2));
    GR_TRY(gr_transform(r, w.ext2, J * 2 * nl, gr_map(nl, nl, 0, 0), false));
    hipLaunchKernelGGL(k_gr_ks_finish, dim3(gx, nl, (unsigned)(J * 2)), dim3(GR_T), 0, r->stream, w.accQ, w.ext2, w.jobs, r->pinv, add, add_mask, out, r->modc, nl, N);
    GR_HIP(r, hipGetLastError());
    return 0;
}
bool gr_overlap(const void *a, size_t na, const void *b, size_t nb) { const char *x = (const char *)a, *y = (const char *)b; return x < y + nb && y < x + na; }
int gr_check_level(sfg_ring *r, const char *what, int nct, int level) {
    if (nct < 0) GR_FAIL(r, "%s: negative ciphertext count %d", what, nct);
    if (level < 0 || level >= r->nq) GR_FAIL(r, "%s: level %d out of range 0..%d", what, level, r->nq - 1);
    return 0;
}
u64 gr_galois(const sfg_ring *r, int k) { const u64 M = 2ULL * r->N; int n = r->N / 2; k %= n; if (k < 0) k += n; u64 g = 1; for (int i = 0; i < k; i++) g = (g * 5) % M; return g; }

// automorphisms of a batch: ct j under galois[j] (0 = copy)
static int gr_apply_galois(sfg_ring *r, const char *what, const u64 *in, u64 *out, int nct, int level, const std::vector<u64> &gal) {
    const int nl = level + 1, N = r->N; const size_t ctw = (size_t)2 * nl * N;
    std::vector<GrJob> jobs;
    for (int j = 0; j < nct; j++) {
        if (gal[j] == 0) continue;
        auto it = r->rotkeys.find(gal[j]);
        if (it == r->rotkeys.end()) GR_FAIL(r, "%s: no key loaded for galois element %llu", what, (unsigned long long)gal[j]);
        jobs.push_back(GrJob{it->second.key, it->second.idx, j});
    }
    for (int j = 0; j < nct; j++) if (gal[j] == 0) GR_HIP(r, hipMemcpyAsync(out + j * ctw, in + j * ctw, ctw * 8, hipMemcpyDeviceToDevice, r->stream));
    return gr_ks_batch(r, level, jobs, in, 1, out, [&](size_t, size_t n, const GrKsWs &w) {
        hipLaunchKernelGGL(k_gr_gather_c1, dim3(N / GR_T, nl, (unsigned)n), dim3(GR_T), 0, r->stream, in, w.c2, w.jobs, nl, N);
    });
}

template <int OP>
static int gr_ew(sfg_ring *r, const u64 *a, const u64 *b, u64 *out, const GrScalars &sc, size_t pt_stride, int nct, int nl_in, int nl_out) {
    gr_split((size_t)nct, kGrEwCap, [&](size_t c0, size_t n) {
        const size_t oi = c0 * 2 * nl_in * r->N, oo = c0 * 2 * nl_out * r->N;
        const bool pt = OP == GR_ADDP || OP == GR_MULP;
        hipLaunchKernelGGL(k_gr_ew<OP>, dim3(r->N / GR_T, nl_out, (unsigned)n * 2), dim3(GR_T), 0, r->stream, a + oi, b ? (pt ? b + c0 * pt_stride : b + oi) : nullptr,
                           out + oo, sc, pt_stride, r->modc, nl_in, nl_out, r->N);
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return 0;
}
static int gr_scalars(sfg_ring *r, const char *what, const uint64_t *s, int level, GrScalars &sc) {
    if (!s) GR_FAIL(r, "%s: null scalars", what);
    for (int m = 0; m <= level; m++) { if (s[m] >= r->q[m]) GR_FAIL(r, "%s: scalar %d is not a canonical residue", what, m); sc.s[m] = s[m]; }
    return 0;
}

// ---------------------------------------------------------------- C-ABI
extern "C" void sfg_ring_destroy(sfg_ring *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    volatile uint32_t *k = r->io.enc_key; for (int i = 0; i < 8; i++) k[i] = 0;      // the host copy of the ChaCha20 key; the device's secrets are wiped by their owners
    delete r;
}
extern "C" int sfg_ring_create(sfg_ring **out, int device, int logN, int nq, int np, const uint64_t *moduli, const uint64_t *psi) {
    if (!out) { g_ring_create_error = "null result pointer"; return 1; }
    *out = nullptr;
    const GrNttPlan plan = gr_ntt_plan(logN);
    if (!plan.ok) { g_ring_create_error = "logN must be 12..16"; return 1; }
    if (nq < 1 || np < 1 || nq + np > gr::kMaxMod) { g_ring_create_error = "bad modulus counts: nq >= 1, np >= 1, nq + np <= 48"; return 1; }
    if (!moduli) { g_ring_create_error = "null moduli"; return 1; }
    const int N = 1 << logN, nmod = nq + np;
    std::vector<u64> ps(nmod);
    for (int m = 0; m < nmod; m++) {
        const u64 q = moduli[m]; char b[160];
        if (q >= gr::kMaxModulus || q < 3 || (q - 1) % (2ULL * N)) { snprintf(b, sizeof b, "modulus %d must be < 2^61 and == 1 mod 2N", m); g_ring_create_error = b; return 1; }
        if (!hm_is_prime(q)) { snprintf(b, sizeof b, "modulus %d is not prime", m); g_ring_create_error = b; return 1; }
        for (int k = 0; k < m; k++) if (moduli[k] == q) { snprintf(b, sizeof b, "modulus %d repeats modulus %d", m, k); g_ring_create_error = b; return 1; }
        ps[m] = psi ? psi[m] : hm_derive_psi(q, logN);
        if (ps[m] >= q || hm_pow(ps[m], N, q) != q - 1) { g_ring_create_error = "psi is not a primitive 2N-th root of unity"; return 1; }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); g_ring_create_error = "no HIP device: libsfgwas_hip has no CPU fallback"; return 1; }
    if (device < 0 || device >= ndev) { g_ring_create_error = "bad device index"; return 1; }
    sfg_ring *r = new sfg_ring();
    r->device = device; r->logN = logN; r->N = N; r->nq = nq; r->np = np; r->nmod = nmod; r->beta = gr_digits(nq - 1, np).beta; r->plan = plan;
    if (const char *e = getenv("SFG_ENABLE_TEST_HOOKS")) r->test_hooks = atoi(e) == 1;
    auto fail = [&](const char *m) { std::string msg = m; sfg_ring_destroy(r); g_ring_create_error = msg; return 1; };
    if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
    if (hipStreamCreateWithFlags(&r->stream.h, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    r->pin_bytes = 1u << 20;
    if (hipHostMalloc(&r->pin.h, r->pin_bytes, hipHostMallocDefault) != hipSuccess) return fail("hipHostMalloc failed");
    std::vector<GrMod> mc(nmod); std::vector<u64> tw((size_t)nmod * 4 * N);
    for (int m = 0; m < nmod; m++) {
        const u64 q = moduli[m]; r->q[m] = q; r->psi[m] = ps[m];
        const u128 u = ~(u128)0 / q;                                        // floor((2^128 - 1) / q) = floor(2^128 / q): q is odd
        const u64 ninv = hm_inv((u64)N, q), r64 = hm_inv((u64)((((u128)1) << 64) % q), q);
        mc[m] = GrMod{q, (u64)(u >> 64), (u64)u, ninv, hm_shoup(ninv, q), r64, hm_shoup(r64, q)};
        u64 *t = tw.data() + (size_t)m * 4 * N; const u64 psi_inv = hm_inv(ps[m], q); u64 p = 1, pi = 1;
        for (int k = 0; k < N; k++) {
            const uint32_t b = hm_brev((uint32_t)k, logN);
            t[b] = p; t[N + b] = hm_shoup(p, q); t[2 * N + b] = pi; t[3 * N + b] = hm_shoup(pi, q);
            p = hm_mul(p, ps[m], q); pi = hm_mul(pi, psi_inv, q);
        }
    }
    std::vector<u64> pinv((size_t)2 * nq);
    for (int t = 0; t < nq; t++) { const u64 q = r->q[t]; u64 P = 1; for (int p = 0; p < np; p++) P = hm_mul(P, r->q[nq + p] % q, q); P = hm_inv(P, q); pinv[2 * t] = P; pinv[2 * t + 1] = hm_shoup(P, q); }
    if (r->modc.alloc(mc.size() * sizeof(GrMod)) != hipSuccess || r->tw.alloc(tw.size() * 8) != hipSuccess || r->pinv.alloc(pinv.size() * 8) != hipSuccess) return fail("hipMalloc of tables failed");
    if (hipMemcpy(r->modc, mc.data(), mc.size() * sizeof(GrMod), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(r->tw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(r->pinv, pinv.data(), pinv.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return fail("table upload failed");
    std::vector<int> src(np), tgt(nq);
    for (int p = 0; p < np; p++) src[p] = nq + p;
    for (int t = 0; t < nq; t++) tgt[t] = t;
    if (gr_build_ext(r, r->down, src, np, tgt)) { std::string e = r->err; return fail(e.c_str()); }
    *out = r;
    return 0;
}
extern "C" const char *sfg_ring_last_error(const sfg_ring *r) { return r ? r->err.c_str() : g_ring_create_error.c_str(); }
extern "C" int sfg_ring_synchronize(sfg_ring *r) { GR_HIP(r, hipSetDevice(r->device)); GR_HIP(r, hipStreamSynchronize(r->stream)); return 0; }
extern "C" int sfg_ring_malloc(sfg_ring *r, void **p, size_t bytes) { GR_HIP(r, hipSetDevice(r->device)); GR_HIP(r, hipMalloc(p, bytes)); return 0; }
extern "C" int sfg_ring_free(sfg_ring *r, void *p) { GR_HIP(r, hipSetDevice(r->device)); GR_HIP(r, hipStreamSynchronize(r->stream)); GR_HIP(r, hipFree(p)); return 0; }
extern "C" int sfg_ring_memcpy_h2d(sfg_ring *r, void *d, const void *s, size_t n) {
    GR_HIP(r, hipSetDevice(r->device)); GR_HIP(r, hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, r->stream)); GR_HIP(r, hipStreamSynchronize(r->stream)); return 0;
}
extern "C" int sfg_ring_memcpy_d2h(sfg_ring *r, void *d, const void *s, size_t n) {
    GR_HIP(r, hipSetDevice(r->device)); GR_HIP(r, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, r->stream)); GR_HIP(r, hipStreamSynchronize(r->stream)); return 0;
}

static int gr_rows(sfg_ring *r, const char *what, uint64_t *rows, int nrows, const int *mod_idx, bool inv) {
    GR_HIP(r, hipSetDevice(r->device));
    if (nrows < 0) GR_FAIL(r, "%s: negative row count %d", what, nrows);
    if (nrows == 0) return 0;
    if (!rows || !mod_idx) GR_FAIL(r, "%s: null argument", what);
    for (int i = 0; i < nrows; i++) if (mod_idx[i] < 0 || mod_idx[i] >= r->nmod) GR_FAIL(r, "%s: modulus index %d of row %d out of range 0..%d", what, mod_idx[i], i, r->nmod - 1);
    GR_TRY(gr_reserve(r, r->modidx, (size_t)nrows * sizeof(int)));
    GR_TRY(gr_upload(r, r->modidx, mod_idx, (size_t)nrows * sizeof(int)));
    GrRowMap map = gr_map(1, 1, 0, 0); map.table = r->modidx;
    return gr_transform(r, (u64 *)rows, (size_t)nrows, map, inv);
}
extern "C" int sfg_ring_ntt_rows(sfg_ring *r, uint64_t *rows, int nrows, const int *mod_idx) { return gr_rows(r, "sfg_ring_ntt_rows", rows, nrows, mod_idx, false); }
extern "C" int sfg_ring_intt_rows(sfg_ring *r, uint64_t *rows, int nrows, const int *mod_idx) { return gr_rows(r, "sfg_ring_intt_rows", rows, nrows, mod_idx, true); }

int gr_rows_from_mont(sfg_ring *r, u64 *rows, size_t nrows) {
    gr_split(nrows, gr_from_mont_cap(r->nmod), [&](size_t r0, size_t n) {
        hipLaunchKernelGGL(k_gr_from_mont, dim3(r->N / GR_T, (unsigned)n), dim3(GR_T), 0, r->stream, rows + r0 * r->N, r->modc, r->nmod, r->N);
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return 0;
}
static int gr_load_key(sfg_ring *r, GrKey &k, const uint64_t *key_host, int mont) {
    const size_t words = (size_t)r->beta * 2 * r->nmod * r->N;
    if (!k.key) GR_HIP(r, k.key.alloc(words * 8));
    GR_HIP(r, hipMemcpyAsync(k.key, key_host, words * 8, hipMemcpyHostToDevice, r->stream));
    if (mont) hipLaunchKernelGGL(k_gr_from_mont, dim3(r->N / GR_T, (unsigned)(r->beta * 2 * r->nmod)), dim3(GR_T), 0, r->stream, k.key, r->modc, r->nmod, r->N);
    GR_HIP(r, hipStreamSynchronize(r->stream));
    return 0;
}
extern "C" int sfg_ring_load_rotkey(sfg_ring *r, uint64_t g, const uint64_t *key_host, int mont) {
    GR_HIP(r, hipSetDevice(r->device));
    const int N = r->N;
    if (!key_host) GR_FAIL(r, "sfg_ring_load_rotkey: null key");
    if (!(g & 1) || g >= 2ULL * N) GR_FAIL(r, "sfg_ring_load_rotkey: galois element %llu is not an odd number below 2N", (unsigned long long)g);
    GrKey fresh; const auto it = r->rotkeys.find(g);                        // a new element's key enters the map only when it is complete
    GrKey &k = it != r->rotkeys.end() ? it->second : fresh;
    GR_TRY(gr_load_key(r, k, key_host, mont));
    if (!k.idx) GR_HIP(r, k.idx.alloc((size_t)N * 4));
    std::vector<uint32_t> idx(N); const u64 mask = 2ULL * N - 1;             // lattigo ring.PermuteNTTIndex: out[i] = in[index[i]]
    for (int i = 0; i < N; i++) { u64 t1 = 2ULL * hm_brev((uint32_t)i, r->logN) + 1, t2 = ((g * t1 & mask) - 1) >> 1; idx[i] = hm_brev((uint32_t)t2, r->logN); }
    GR_HIP(r, hipMemcpy(k.idx, idx.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    if (it == r->rotkeys.end()) r->rotkeys.emplace(g, std::move(fresh));
    return 0;
}
extern "C" int sfg_ring_has_rotkey(const sfg_ring *r, uint64_t g) { return r->rotkeys.count(g) ? 1 : 0; }
extern "C" int sfg_ring_load_relinkey(sfg_ring *r, const uint64_t *key_host, int mont) {
    GR_HIP(r, hipSetDevice(r->device));
    if (!key_host) GR_FAIL(r, "sfg_ring_load_relinkey: null key");
    return gr_load_key(r, r->rlk, key_host, mont);
}
extern "C" uint64_t sfg_ring_galois_for_rotation(const sfg_ring *r, int k_left) { return gr_galois(r, k_left); }

extern "C" int sfg_ring_rotate_right_dev(sfg_ring *r, const uint64_t *in, uint64_t *out, int nct, int level, const int *nrot_host) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(gr_check_level(r, "sfg_ring_rotate_right_dev", nct, level));
    if (nct == 0) return 0;
    if (!in || !out || !nrot_host) GR_FAIL(r, "sfg_ring_rotate_right_dev: null argument");
    const size_t bytes = (size_t)nct * 2 * (level + 1) * r->N * 8;
    if (gr_overlap(in, bytes, out, bytes)) GR_FAIL(r, "sfg_ring_rotate_right_dev: in and out may not alias");
    std::vector<u64> gal(nct); const int n = r->N / 2;
    for (int j = 0; j < nct; j++) { int k = nrot_host[j] % n; if (k < 0) k += n; gal[j] = k ? gr_galois(r, n - k) : 0; }
    return gr_apply_galois(r, "sfg_ring_rotate_right_dev", (const u64 *)in, (u64 *)out, nct, level, gal);
}
extern "C" int sfg_ring_ct_galois_dev(sfg_ring *r, const uint64_t *in, uint64_t *out, int nct, int level, uint64_t g) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(gr_check_level(r, "sfg_ring_ct_galois_dev", nct, level));
    if (nct == 0) return 0;
    if (!in || !out) GR_FAIL(r, "sfg_ring_ct_galois_dev: null argument");
    const size_t bytes = (size_t)nct * 2 * (level + 1) * r->N * 8;
    if (gr_overlap(in, bytes, out, bytes)) GR_FAIL(r, "sfg_ring_ct_galois_dev: in and out may not alias");
    if (!(g & 1) || g >= 2ULL * r->N) GR_FAIL(r, "sfg_ring_ct_galois_dev: galois element %llu is not an odd number below 2N", (unsigned long long)g);
    return gr_apply_galois(r, "sfg_ring_ct_galois_dev", (const u64 *)in, (u64 *)out, nct, level, std::vector<u64>(nct, g));
}

#define GR_EW_ENTRY(what, cond_null)                                            \
    GR_HIP(r, hipSetDevice(r->device));                                         \
    GR_TRY(gr_check_level(r, what, nct, level));                                \
    if (nct == 0) return 0;                                                     \
    if (cond_null) GR_FAIL(r, what ": null argument");
extern "C" int sfg_ring_ct_add_dev(sfg_ring *r, const uint64_t *a, const uint64_t *b, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_add_dev", !a || !b || !out)
    return gr_ew<GR_ADD>(r, (const u64 *)a, (const u64 *)b, (u64 *)out, GrScalars(), 0, nct, level + 1, level + 1);
}
extern "C" int sfg_ring_ct_sub_dev(sfg_ring *r, const uint64_t *a, const uint64_t *b, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_sub_dev", !a || !b || !out)
    return gr_ew<GR_SUB>(r, (const u64 *)a, (const u64 *)b, (u64 *)out, GrScalars(), 0, nct, level + 1, level + 1);
}
extern "C" int sfg_ring_ct_drop_level_dev(sfg_ring *r, const uint64_t *in, uint64_t *out, int nct, int level_in, int level_out) {
    const int level = level_in;
    GR_EW_ENTRY("sfg_ring_ct_drop_level_dev", !in || !out)
    if (level_out < 0 || level_out > level_in) GR_FAIL(r, "sfg_ring_ct_drop_level_dev: level_out %d out of range 0..%d", level_out, level_in);
    if (gr_overlap(in, (size_t)nct * 2 * (level_in + 1) * r->N * 8, out, (size_t)nct * 2 * (level_out + 1) * r->N * 8)) GR_FAIL(r, "sfg_ring_ct_drop_level_dev: in and out may not alias");
    return gr_ew<GR_DROP>(r, (const u64 *)in, nullptr, (u64 *)out, GrScalars(), 0, nct, level_in + 1, level_out + 1);
}
extern "C" int sfg_ring_ct_mul_scalar_dev(sfg_ring *r, const uint64_t *ct, const uint64_t *scalars_host, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_mul_scalar_dev", !ct || !out)
    GrScalars sc; GR_TRY(gr_scalars(r, "sfg_ring_ct_mul_scalar_dev", scalars_host, level, sc));
    return gr_ew<GR_MULS>(r, (const u64 *)ct, nullptr, (u64 *)out, sc, 0, nct, level + 1, level + 1);
}
extern "C" int sfg_ring_ct_mul_scalar_add_dev(sfg_ring *r, const uint64_t *ct, const uint64_t *scalars_host, uint64_t *acc, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_mul_scalar_add_dev", !ct || !acc)
    GrScalars sc; GR_TRY(gr_scalars(r, "sfg_ring_ct_mul_scalar_add_dev", scalars_host, level, sc));
    return gr_ew<GR_MULSADD>(r, (const u64 *)ct, nullptr, (u64 *)acc, sc, 0, nct, level + 1, level + 1);
}
extern "C" int sfg_ring_ct_add_scalar_dev(sfg_ring *r, const uint64_t *ct, const uint64_t *scalars_host, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_add_scalar_dev", !ct || !out)
    GrScalars sc; GR_TRY(gr_scalars(r, "sfg_ring_ct_add_scalar_dev", scalars_host, level, sc));
    return gr_ew<GR_ADDS>(r, (const u64 *)ct, nullptr, (u64 *)out, sc, 0, nct, level + 1, level + 1);
}
extern "C" int sfg_ring_ct_add_plain_dev(sfg_ring *r, const uint64_t *ct, const uint64_t *pt, size_t pt_stride, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_add_plain_dev", !ct || !pt || !out)
    return gr_ew<GR_ADDP>(r, (const u64 *)ct, (const u64 *)pt, (u64 *)out, GrScalars(), pt_stride, nct, level + 1, level + 1);
}
extern "C" int sfg_ring_ct_mul_plain_dev(sfg_ring *r, const uint64_t *ct, const uint64_t *pt, size_t pt_stride, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_mul_plain_dev", !ct || !pt || !out)
    return gr_ew<GR_MULP>(r, (const u64 *)ct, (const u64 *)pt, (u64 *)out, GrScalars(), pt_stride, nct, level + 1, level + 1);
}

extern "C" int sfg_ring_ct_mulrelin_dev(sfg_ring *r, const uint64_t *a, const uint64_t *b, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_mulrelin_dev", !a || !b || !out)
    const int nl = level + 1, N = r->N; const size_t ctw = (size_t)2 * nl * N, bytes = (size_t)nct * ctw * 8;
    if (gr_overlap(a, bytes, out, bytes) || gr_overlap(b, bytes, out, bytes)) GR_FAIL(r, "sfg_ring_ct_mulrelin_dev: out may alias neither input");
    if (!r->rlk.key) GR_FAIL(r, "sfg_ring_ct_mulrelin_dev: no relinearisation key loaded");
    std::vector<GrJob> jobs(nct);
    for (int j = 0; j < nct; j++) jobs[j] = GrJob{r->rlk.key, nullptr, j};
    return gr_ks_batch(r, level, jobs, (const u64 *)out, 3, (u64 *)out, [&](size_t j0, size_t n, const GrKsWs &w) {
        hipLaunchKernelGGL(k_gr_tensor, dim3(N / GR_T, nl, (unsigned)n), dim3(GR_T), 0, r->stream, (const u64 *)a + j0 * ctw, (const u64 *)b + j0 * ctw, (u64 *)out + j0 * ctw, w.c2, r->modc, nl, N);
    });
}
extern "C" int sfg_ring_ct_rescale_dev(sfg_ring *r, const uint64_t *in, uint64_t *out, int nct, int level) {
    GR_EW_ENTRY("sfg_ring_ct_rescale_dev", !in || !out)
    if (level == 0) GR_FAIL(r, "sfg_ring_ct_rescale_dev: cannot rescale at level 0");
    const int nl = level + 1, N = r->N;
    if (gr_overlap(in, (size_t)nct * 2 * nl * N * 8, out, (size_t)nct * 2 * level * N * 8)) GR_FAIL(r, "sfg_ring_ct_rescale_dev: in and out may not alias");
    GrLevel *L; GR_TRY(gr_level(r, level, &L));
    const GrChunks plan = gr_rescale_plan((size_t)nct, level, (size_t)N, r->ws_budget);
    GR_TRY(gr_reserve(r, r->ws, plan.bytes));
    const GrRescaleLayout lay = gr_rescale_layout(level, (size_t)N, plan.chunk);
    u64 *T = (u64 *)r->ws.p + lay.T, *tmp = (u64 *)r->ws.p + lay.tmp;
    for (size_t c = 0; c < plan.nchunks; c++) {
        const size_t j0 = plan.first(c), n = plan.count(c, (size_t)nct); const u64 *src = (const u64 *)in + j0 * 2 * nl * N; const unsigned gx = N / GR_T;
        hipLaunchKernelGGL(k_gr_copy_last, dim3(gx, 1, (unsigned)n * 2), dim3(GR_T), 0, r->stream, src, T, nl, N);
        GR_TRY(gr_transform(r, T, n * 2, gr_map(1, 1, level, 0), true));
        hipLaunchKernelGGL(k_gr_rescale_prep, dim3(gx, level, (unsigned)n * 2), dim3(GR_T), 0, r->stream, T, tmp, L->rescale_tab, r->modc, level, N);
        GR_TRY(gr_transform(r, tmp, n * 2 * level, gr_map(level, level, 0, 0), false));
        hipLaunchKernelGGL(k_gr_rescale_fin, dim3(gx, level, (unsigned)n * 2), dim3(GR_T), 0, r->stream, src, tmp, (u64 *)out + j0 * 2 * level * N, L->rescale_tab, r->modc, level, N);
    }
    GR_HIP(r, hipGetLastError());
    return 0;
}
extern "C" int sfg_ring_ct_innersum_dev(sfg_ring *r, const uint64_t *in, int nct, int level, uint64_t *out) {
    GR_HIP(r, hipSetDevice(r->device));
    GR_TRY(gr_check_level(r, "sfg_ring_ct_innersum_dev", nct, level));
    if (nct < 1) GR_FAIL(r, "sfg_ring_ct_innersum_dev: needs at least one ciphertext");
    if (!in || !out) GR_FAIL(r, "sfg_ring_ct_innersum_dev: null argument");
    const int nl = level + 1, N = r->N; const size_t ctw = (size_t)2 * nl * N;
    if (gr_overlap(in, (size_t)nct * ctw * 8, out, ctw * 8)) GR_FAIL(r, "sfg_ring_ct_innersum_dev: in and out may not alias");
    for (int rot = 1; rot < N / 2; rot *= 2) if (!r->rotkeys.count(gr_galois(r, rot))) GR_FAIL(r, "sfg_ring_ct_innersum_dev: no key loaded for the left rotation by %d", rot);
    GR_TRY(gr_reserve(r, r->small, ctw * 8));
    u64 *rt = r->small;
    GR_HIP(r, hipMemcpyAsync(out, in, ctw * 8, hipMemcpyDeviceToDevice, r->stream));
    for (int i = 1; i < nct; i++) GR_TRY(gr_ew<GR_ADD>(r, (const u64 *)in + i * ctw, (const u64 *)out, (u64 *)out, GrScalars(), 0, 1, nl, nl));
    for (int rot = 1; rot < N / 2; rot *= 2) {
        GR_TRY(gr_apply_galois(r, "sfg_ring_ct_innersum_dev", (const u64 *)out, rt, 1, level, std::vector<u64>(1, gr_galois(r, rot))));
        GR_TRY(gr_ew<GR_ADD>(r, rt, (const u64 *)out, (u64 *)out, GrScalars(), 0, 1, nl, nl));
    }
    return 0;
}
