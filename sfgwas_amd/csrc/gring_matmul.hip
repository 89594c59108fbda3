// gring_matmul.hip - the general ring's matrix products: the encrypted-row-vector x int8-genotype block product of gwas/matmult.go (MatMult4Stream) for every ring
// sfg_ring_create accepts, in the ring's integer arithmetic.  The twin of matmul.hip (the PN14QP438 context) with nothing shared but the C-ABI's layouts.
// Shift tables, the fold's bound, launch caps, workspace layout and chunks: gring_matmul_plan.hpp.  DESIGN.md section 18.
//
// Per chunk of ciphertexts and operand block row (the oracle's orc_matmult_accumulate, loop for loop):
//   1. the rotation cache: RotateRight(A, -baby) at the dropped level for every active baby, one batch of key switches (gr_ks_batch); the key switch hands out the
//      permuted d_p, k_gr_mm_add_c0 adds the permuted c0 (the automorphism is additive, so the words are those of rotating c0 + d_0)
//   2. per active giant, in batches of diagonals: k_gr_mm_diag (the diagonals straight into the encoder's DFT input, their sum of magnitudes beside them),
//      k_gr_mm_band, the encoder's shared device half (gri_encode_dft), k_gr_mm_tie (the coefficients the encoder could not prove rounded, re-derived exactly from
//      the matrix bytes: gring_tie.hpp), the ring's forward transform of the plaintext rows
//   3. k_gr_mm_mac: the batch's products summed in 128-bit registers, reduced, added into the canonical accumulator rows
// and the finalize (orc_matmult_finalize): giant g > 0 rotated by -g d at level L - 1 through the same batch, the giants of one output summed by k_gr_mm_fin.
// All launches go on the ring's stream.  Every word written is canonical.
//
// The MAC's sum and the reference's: lattigo sums REDC-form products lazily in a u128 and reduces once; REDC(rot * MForm(pt)) = rot * pt mod q, so the canonical
// words are the same and no Montgomery form appears here.  The reference's u128 silently wraps once terms (q - 1)^2 >= 2^128; the MAC folds its sum to a word
// below q every fold_terms(q) terms instead, so its result is the exact sum modulo q.  That equals the reference wherever the reference does not wrap, which is at
// every lattigo preset (55-bit words allow 2^18 terms); at 61-bit words (64 terms) the reference's own result is the defect.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "gring_dev.hpp"
#include "gring_io_arith.hpp"
#include "gring_matmul_plan.hpp"
#include "gring_tie.hpp"

struct MmVec { int shift, bj, slot, pad; };                                 // one diagonal of a batch: its shift, its block column, its baby's slot of the rotation cache
struct MmJob { u64 src; const uint32_t *idx; long long ct; };               // one rotation: word offset of its source ciphertext, its index table, its slot
static_assert(sizeof(MmVec) == 16 && sizeof(MmJob) == 24, "gring_matmul_plan.hpp sizes the tables");

// ---------------------------------------------------------------- kernels; x < N and t < n by the grids: N / 2 is a multiple of 256
// Diagonal `shift` of operand block (bi, bj), rotated right by rotg = d giant: slot t holds diag[jp], jp = t - rotg mod n, and diag[jp] = X[(shift + jp) mod n][jp]
// (matmult.go:636-672), zero outside the block.  The operand is the resident matrix (element (I, J) at I ld + J) or its transpose (at J ld + I): I < R and J < C
// bound the address in both.  Missing (negative) -> 0, then the optional square with the int8 wrap-around.  One function for the extraction and for the resolver,
// which reads the slot again (the encoder's DFT input was transformed in place).
struct MmOperand { const int8_t *geno; size_t ld, R, C; int transpose, square, bi, rotg; };
__device__ __forceinline__ int gr_mm_slot(const MmOperand &o, const MmVec &v, int t, int n) {
    int jp = t - o.rotg; if (jp < 0) jp += n;
    int i = v.shift + jp; if (i >= n) i -= n;
    const size_t I = (size_t)o.bi * n + i, J = (size_t)v.bj * n + jp;
    int x = 0;
    if (I < o.R && J < o.C) x = o.geno[o.transpose ? J * o.ld + I : I * o.ld + J];
    if (x < 0) x = 0;
    if (o.square) x = (int8_t)(x * x);
    return x;
}
// The value goes to the encoder's DFT input position m_t (a permutation of 0 .. n-1: every point of the vector is written); sums[vec] += |v|, an integer below
// 2^7 n.   grid (n / 256, 1, nvec)
__global__ __launch_bounds__(GR_T) void k_gr_mm_diag(MmOperand o, const MmVec *vecs, double4 *A, const uint32_t *slot_m, unsigned *sums, int n) {
    const int t = blockIdx.x * GR_T + threadIdx.x; const size_t vec = blockIdx.z;
    const int x = gr_mm_slot(o, vecs[vec], t, n);
    A[vec * n + slot_m[t]] = make_double4((double)x, 0.0, 0.0, 0.0);
    unsigned a = (unsigned)(x < 0 ? -x : x);
    for (int off = 32; off; off >>= 1) a += __shfl_down(a, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sums[vec], a);
}
// the band of a vector from its exact sum of magnitudes, as gri_encode forms it on the host; `floor` is gio::kEncBandFloor unless the test hook widened it.  The
// batch's list of flagged coefficients starts empty.
__global__ __launch_bounds__(GR_T) void k_gr_mm_band(const unsigned *sums, double *band, double mul, double floor, int nvec, unsigned *ties) {
    const int v = blockIdx.x * GR_T + threadIdx.x;
    if (v == 0) ties[GriTies::kCount] = 0;
    if (v < nvec) { const double b = gio::enc_band((double)sums[v] * mul * (1.0 + 0x1p-40)); band[v] = b > floor ? b : floor; }
}
// The resolver: workgroup k re-derives entry k of the batch's list (gring_tie.hpp has the arithmetic and its bounds); workgroups beyond the count leave at once.
// The threads stride over the n slots: the slot's value from the matrix, the angle pi (5^t j mod 2N) / N with 5^t = 4 m_t + 1 folded to the table, the term added
// into a 256-bit signed sum in registers.  The sums meet as eight columns of 32-bit limbs (a wave's by shuffles, the four waves' through LDS); thread 0 carries them
// into four words (modulo 2^256: the true sum is far below 2^255) and decides: proven -> the rounded value modulo every q_i into the coefficient-domain rows
// R [nvec][nl][N] in place of the encoder's, ties[kResolved] += 1; otherwise flags[0] += 1 (unproven) or flags[1] += 1 (outside |p| < 2^62).
// An entry's vector is < nvec and its coefficient < N: k_gdd_enc_post wrote both from its own grid.   grid (GriTies::kCap)
__global__ __launch_bounds__(GR_T) void k_gr_mm_tie(MmOperand o, const MmVec *vecs, const uint32_t *slot_m, const unsigned *sums, const u64 *ctab, unsigned *ties, u64 *R, unsigned *flags,
                                                    const GrMod *modc, u64 scale_m, int scale_e, int logn, int nl) {
    __shared__ u64 part[GR_T / 64][8];
    const unsigned count = ties[GriTies::kCount];
    if (blockIdx.x >= (count < (unsigned)GriTies::kCap ? count : (unsigned)GriTies::kCap)) return;       // uniform
    const unsigned vec = ties[GriTies::kEntries + 2 * blockIdx.x], j = ties[GriTies::kEntries + 2 * blockIdx.x + 1];
    const int n = 1 << logn; const unsigned N = 2u * n;
    const MmVec v = vecs[vec];
    gtie::Acc acc; acc.zero();
    for (int t = threadIdx.x; t < n; t += GR_T) {
        const int x = gr_mm_slot(o, v, t, n);
        if (!x) continue;
        bool neg; const unsigned k = gtie::fold(((4u * slot_m[t] + 1u) * j) & (2u * N - 1u), N, neg);     // k <= N / 2: inside the table's N / 2 + 1 entries
        const u64 *c = ctab + (size_t)k * gtie::kWords;
        const u64 cw[3] = {c[0], c[1], c[2]};
        acc.addmul(cw, x, neg);
    }
    u64 col[8];
#pragma unroll
    for (int i = 0; i < 4; i++) { col[2 * i] = acc.w[i] & 0xFFFFFFFFu; col[2 * i + 1] = acc.w[i] >> 32; }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        for (int off = 32; off; off >>= 1) col[i] += __shfl_down(col[i], off);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][i] = col[i];
    }
    __syncthreads();
    if (threadIdx.x) return;
    u64 X[4], carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u64 lo = carry, hi;
#pragma unroll
        for (int w = 0; w < GR_T / 64; w++) lo += part[w][2 * i];                                         // 256 limbs and a carry: below 2^41
        hi = lo >> 32;
#pragma unroll
        for (int w = 0; w < GR_T / 64; w++) hi += part[w][2 * i + 1];
        X[i] = (lo & 0xFFFFFFFFu) | (hi << 32); carry = hi >> 32;
    }
    long long p;
    const int st = gtie::decide(X, scale_m, scale_e, logn, (u64)sums[vec], p);
    if (st) { atomicAdd(&flags[st - 1], 1u); return; }
    for (int i = 0; i < nl; i++) { const GrMod mc = modc[i]; R[((size_t)vec * nl + i) * N + j] = gio::reduce_i62(p, mc.q, mc.uhi, mc.ulo); }
    atomicAdd(&ties[GriTies::kResolved], 1u);
}
static_assert((int)GriTies::kCap == gtie::kCap, "one capacity");
// slot 0 of the cache: the ciphertext itself at the dropped level.  grid (N / 256, nl, sc * 2)
__global__ __launch_bounds__(GR_T) void k_gr_mm_drop(const u64 *A, u64 *rot, int nbr, int bi, int d, int nl_in, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y, p = blockIdx.z & 1; const size_t i = blockIdx.z >> 1;
    rot[(((i * d) * 2 + p) * nl + m) * N + x] = A[(((i * nbr + bi) * 2 + p) * nl_in + m) * N + x];
}
// the key switch's input: c1 of every job's source.  grid (N / 256, nl, jobs of the chunk)
__global__ __launch_bounds__(GR_T) void k_gr_mm_gather_c1(const u64 *in, const MmJob *jobs, u64 *c2, int nl_in, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y;
    c2[((size_t)blockIdx.z * nl + m) * N + x] = in[jobs[blockIdx.z].src + ((size_t)nl_in + m) * N + x];
}
// polynomial 0 of every job's slot += the source's c0 read through the job's automorphism index.  grid (N / 256, nl, jobs)
__global__ __launch_bounds__(GR_T) void k_gr_mm_add_c0(const u64 *in, const MmJob *jobs, u64 *out, const GrMod *modc, int nl, int N) {
    const int x = blockIdx.x * GR_T + threadIdx.x, m = blockIdx.y; const MmJob jb = jobs[blockIdx.z];
    u64 *o = out + (((size_t)jb.ct * 2) * nl + m) * N + x;
    *o = gr::addmod(*o, in[jb.src + (size_t)m * N + jb.idx[x]], modc[m].q);           // index table entries < N
}
// The MAC.  A thread owns coefficient x of modulus row l of one block column and a tile of ST ciphertexts of the giant step; its 2 ST sums are 128-bit registers.
// It walks the batch's diagonals of its block column (first[bj] .. first[bj + 1]), reads each plaintext word once and each rotated word once, folds every `fold`
// terms (uniform over the workgroup: one modulus), and adds the reduced sums into the canonical accumulator rows.
//   rot [sc][d][2][nl][N]   pt [nvec][L][N]   acc [m_ct][d][acc_s][2][L][N] at ciphertext acc_i0 + i.   grid (N / 256, L, block columns x tiles)
struct MmMacArgs { int sc, d, nl, L, N, giant, bj0, ntiles, acc_s, acc_i0; };
template <int ST>
__global__ __launch_bounds__(GR_T) void k_gr_mm_mac(const u64 *rot, const u64 *pt, const MmVec *vecs, const int *first, u64 *acc, const GrMod *modc, const unsigned *fold_tab, MmMacArgs a) {
    const int x = blockIdx.x * GR_T + threadIdx.x, l = blockIdx.y, bj = a.bj0 + blockIdx.z / a.ntiles, i0 = (blockIdx.z % a.ntiles) * ST;
    const int v0 = first[bj], v1 = first[bj + 1];
    if (v0 == v1) return;                                                   // uniform: the block column has no diagonal in this batch
    const GrMod mc = modc[l]; const unsigned fold = fold_tab[l];
    const int ni = min(ST, a.sc - i0);
    MmSum S[ST][2];
    unsigned terms = 0;
    const size_t N = a.N, polyw = (size_t)a.nl * N, ctw = 2 * polyw;
    for (int v = v0; v < v1; v++) {
        if (terms == fold) {
#pragma unroll
            for (int k = 0; k < ST; k++) { S[k][0].fold(mc.q, mc.uhi, mc.ulo); S[k][1].fold(mc.q, mc.uhi, mc.ulo); }
            terms = 0;
        }
        const u64 p = pt[((size_t)v * a.L + l) * N + x];
        const u64 *r0 = rot + ((size_t)i0 * a.d + vecs[v].slot) * ctw + (size_t)l * N + x;
#pragma unroll
        for (int k = 0; k < ST; k++) if (k < ni) { S[k][0].mac(r0[(size_t)k * a.d * ctw], p); S[k][1].mac(r0[(size_t)k * a.d * ctw + polyw], p); }
        terms++;
    }
#pragma unroll
    for (int k = 0; k < ST; k++) if (k < ni) {
        u64 *o = acc + (((((size_t)bj * a.d + a.giant) * a.acc_s + a.acc_i0 + i0 + k) * 2) * a.L + l) * N + x;
        o[0] = gr::addmod(o[0], S[k][0].word(mc.q, mc.uhi, mc.ulo), mc.q);
        o[(size_t)a.L * N] = gr::addmod(o[(size_t)a.L * N], S[k][1].word(mc.q, mc.uhi, mc.ulo), mc.q);
    }
}
// the finalize's sum of one block column: out[i][bj] (+)= acc of giant 0 + the rotated accumulators T of the giants glist[0 .. ng).  grid (N / 256, L, sc * 2)
//   acc [m_ct][d][acc_s][2][L][N]   T [sc][d][2][L][N]   out [.][m_ct][2][L][N] at ciphertext i0 + i
struct MmFinArgs { int d, L, N, m_ct, bj, ng, with0, accumulate, acc_s, i0; };
__global__ __launch_bounds__(GR_T) void k_gr_mm_fin(const u64 *acc, const u64 *T, const int *glist, u64 *out, const GrMod *modc, MmFinArgs a) {
    const int x = blockIdx.x * GR_T + threadIdx.x, l = blockIdx.y, p = blockIdx.z & 1; const size_t i = blockIdx.z >> 1, N = a.N;
    const u64 q = modc[l].q; const size_t row = ((size_t)p * a.L + l) * N + x;
    u64 *o = out + (((size_t)a.i0 + i) * a.m_ct + a.bj) * 2 * a.L * N + row;
    u64 v = a.accumulate ? *o : 0;
    if (a.with0) v = gr::addmod(v, acc[(((size_t)a.bj * a.d) * a.acc_s + a.i0 + i) * 2 * a.L * N + row], q);
    for (int k = 0; k < a.ng; k++) v = gr::addmod(v, T[(i * a.d + glist[k]) * 2 * a.L * N + row], q);
    *o = v;
}

// ---------------------------------------------------------------- host side
struct MmShape {
    int s, in_level, max_level, lev, nl_in, nl, L, d, slots, N, nbr, m_ct;
    size_t R, C, ld; bool tr, sq; const int8_t *geno; double scale;
};
struct MmWs { u64 *rot, *acc, *pt; double4 *dft; MmVec *vecs; int *first, *glist; MmJob *jobs; unsigned *sums, *flags; double *band; };
static MmWs mm_ws(void *ws, const MmLayout &l) {
    u64 *p = (u64 *)ws;
    return MmWs{p + l.rot, p + l.acc, p + l.pt, (double4 *)(p + l.dft), (MmVec *)(p + l.vecs), (int *)(p + l.first), (int *)(p + l.glist), (MmJob *)(p + l.jobs),
                (unsigned *)(p + l.sums), (unsigned *)(p + l.flags), (double *)(p + l.band)};
}
// the fold bound of every modulus row, on the device (built at first use)
static int mm_fold_tab(sfg_ring *r, const unsigned **out) {
    if (!r->mm_fold) {
        std::vector<u64> h((r->nq + 1) / 2, 0); unsigned *f = (unsigned *)h.data();
        for (int m = 0; m < r->nq; m++) f[m] = (unsigned)mm_fold_terms(r->q[m]);
        GrBuf<u64> d; GR_TRY(gr_table(r, d, h.data(), h.size() * 8));
        r->mm_fold = std::move(d);
    }
    *out = (const unsigned *)r->mm_fold.p;
    return 0;
}
// the resolver's cosine table and its list, on the device (built at first use)
static int mm_tie_tab(sfg_ring *r) {
    if (!r->tie_tab) {
        const std::vector<u64> h = gtie::build_table(r->logN);
        GrBuf<unsigned> l; GR_HIP(r, l.alloc(GriTies::kWords * sizeof(unsigned)));
        GR_HIP(r, hipMemsetAsync(l.p, 0, GriTies::kWords * sizeof(unsigned), r->stream));
        GrBuf<u64> d; GR_TRY(gr_table(r, d, h.data(), h.size() * 8));
        r->tie_list = std::move(l); r->tie_tab = std::move(d);
    }
    return 0;
}
// rotations of a list of jobs (slot = job.ct, source = job.src words into `in`, whose ciphertexts have nl_in rows a polynomial) at `level`, into slots of
// 2 (level + 1) N words at `out`: one batch of key switches, then the permuted c0
static int mm_rotate(sfg_ring *r, const MmWs &w, const std::vector<GrJob> &jobs, const std::vector<MmJob> &mj, const u64 *in, int nl_in, int level, u64 *out) {
    if (jobs.empty()) return 0;
    const int nl = level + 1, N = r->N;
    GR_TRY(gr_upload(r, w.jobs, mj.data(), mj.size() * sizeof(MmJob)));
    GR_TRY(gr_ks_batch(r, level, jobs, nullptr, 0, out, [&](size_t j0, size_t n, const GrKsWs &k) {
        hipLaunchKernelGGL(k_gr_mm_gather_c1, dim3(N / GR_T, nl, (unsigned)n), dim3(GR_T), 0, r->stream, in, (const MmJob *)w.jobs + j0, k.c2, nl_in, nl, N);
    }));
    gr_split(jobs.size(), kGrLaunchCap, [&](size_t j0, size_t n) {
        hipLaunchKernelGGL(k_gr_mm_add_c0, dim3(N / GR_T, nl, (unsigned)n), dim3(GR_T), 0, r->stream, in, (const MmJob *)w.jobs + j0, out, r->modc, nl, N);
        return 0;
    });
    GR_HIP(r, hipGetLastError());
    return 0;
}
static int mm_key(sfg_ring *r, const char *what, int k_left, const GrKey **out) {
    auto it = r->rotkeys.find(gr_galois(r, k_left));
    if (it == r->rotkeys.end()) GR_FAIL(r, "%s: no key loaded for the left rotation by %d", what, k_left);
    if (out) *out = &it->second;
    return 0;
}
template <int ST>
static void mm_launch_mac(sfg_ring *r, const MmShape &sh, const MmWs &w, u64 *acc, const unsigned *fold, int sc, int giant, int acc_s, int acc_i0) {
    const int ntiles = (sc + ST - 1) / ST; const size_t per = kMmMacZCap / (size_t)ntiles;
    gr_split((size_t)sh.m_ct, per ? per : 1, [&](size_t bj0, size_t nbj) {
        const MmMacArgs a{sc, sh.d, sh.nl, sh.L, sh.N, giant, (int)bj0, ntiles, acc_s, acc_i0};
        hipLaunchKernelGGL(k_gr_mm_mac<ST>, dim3(sh.N / GR_T, sh.L, (unsigned)(nbj * ntiles)), dim3(GR_T), 0, r->stream, (const u64 *)w.rot, (const u64 *)w.pt, (const MmVec *)w.vecs,
                           (const int *)w.first, acc, r->modc, fold, a);
        return 0;
    });
}
// the accumulate of one chunk of sc ciphertexts (Ac: their block rows [sc][nbr][2][nl_in][N]) over block rows [b0, b1) into acc [m_ct][d][acc_s][2][L][N] at acc_i0
static int mm_accumulate_chunk(sfg_ring *r, const char *what, const MmShape &sh, const MmPlan &plan, const MmWs &w, const u64 *Ac, int sc, int b0, int b1, u64 *acc, int acc_s, int acc_i0) {
    const int N = sh.N, n = sh.slots, d = sh.d;
    GriDdTab tab; GR_TRY(gri_dd_tab(r, &tab));
    const unsigned *fold; GR_TRY(mm_fold_tab(r, &fold));
    GR_TRY(mm_tie_tab(r));
    u64 scale_m; int scale_e; gtie::split_scale(sh.scale, scale_m, scale_e);
    const double band_floor = std::ldexp(1.0, r->tie_band_log2);
    const size_t ctw_in = (size_t)2 * sh.nl_in * N;
    for (int bi = b0; bi < b1; bi++) {
        const MmShifts t = mm_shifts(sh.R, sh.C, n, bi);
        if (t.baby[0]) hipLaunchKernelGGL(k_gr_mm_drop, dim3(N / GR_T, sh.nl, (unsigned)sc * 2), dim3(GR_T), 0, r->stream, Ac, w.rot, sh.nbr, bi, d, sh.nl_in, sh.nl, N);
        std::vector<GrJob> jobs; std::vector<MmJob> mj;
        for (int i = 0; i < sc; i++) for (int b = 1; b < d; b++) if (t.baby[b]) {
            const GrKey *k; GR_TRY(mm_key(r, what, b, &k));
            jobs.push_back(GrJob{k->key, k->idx, (long long)i * d + b});
            mj.push_back(MmJob{((size_t)i * sh.nbr + bi) * ctw_in, k->idx, (long long)i * d + b});
        }
        GR_TRY(mm_rotate(r, w, jobs, mj, Ac, sh.nl_in, sh.lev, w.rot));
        for (int g = 0; g < d; g++) {
            if (!t.giant[g]) continue;
            std::vector<MmVec> vecs;                                            // a giant's existing diagonals, block column by block column
            for (int bj = 0; bj < sh.m_ct; bj++) {
                const int nc = mm_block_len(sh.C, n, bj);
                for (int b = 0; b < d; b++) { const int shift = g * d + b; if (shift < n && t.shift[shift] && mm_diag_exists(t.nr, nc, n, shift)) vecs.push_back(MmVec{shift, bj, b, 0}); }
            }
            for (size_t bt = 0; bt < plan.nbatches(vecs.size()); bt++) {
                const size_t f0 = plan.bfirst(bt), nb = plan.bcount(bt, vecs.size());
                std::vector<int> first(sh.m_ct + 1); size_t v = 0;
                for (int bj = 0; bj <= sh.m_ct; bj++) { while (v < nb && vecs[f0 + v].bj < bj) v++; first[bj] = (int)v; }
                GR_TRY(gr_upload(r, w.vecs, vecs.data() + f0, nb * sizeof(MmVec)));
                GR_TRY(gr_upload(r, w.first, first.data(), first.size() * sizeof(int)));
                GR_HIP(r, hipMemsetAsync(w.sums, 0, nb * 4, r->stream));
                const MmOperand op{sh.geno, sh.ld, sh.R, sh.C, (int)sh.tr, (int)sh.sq, bi, g * d};
                hipLaunchKernelGGL(k_gr_mm_diag, dim3(n / GR_T, 1, (unsigned)nb), dim3(GR_T), 0, r->stream, op, (const MmVec *)w.vecs, w.dft, tab.slot_m, w.sums, n);
                hipLaunchKernelGGL(k_gr_mm_band, dim3((unsigned)((nb + GR_T - 1) / GR_T)), dim3(GR_T), 0, r->stream, (const unsigned *)w.sums, w.band, sh.scale / n, band_floor, (int)nb,
                                   (unsigned *)r->tie_list);
                GR_HIP(r, hipGetLastError());
                GR_TRY(gri_encode_dft(r, w.dft, (int)nb, tab, w.band, w.flags, r->tie_list, w.pt, sh.L, sh.scale));
                hipLaunchKernelGGL(k_gr_mm_tie, dim3(GriTies::kCap), dim3(GR_T), 0, r->stream, op, (const MmVec *)w.vecs, tab.slot_m, (const unsigned *)w.sums, (const u64 *)r->tie_tab,
                                   (unsigned *)r->tie_list, w.pt, w.flags, r->modc, scale_m, scale_e, r->logN - 1, sh.L);
                GR_TRY(gr_transform(r, w.pt, nb * sh.L, gr_map(sh.L, sh.L, 0, 0), false));
                if (sc == 1) mm_launch_mac<1>(r, sh, w, acc, fold, sc, g, acc_s, acc_i0);
                else if (sc == 2) mm_launch_mac<2>(r, sh, w, acc, fold, sc, g, acc_s, acc_i0);
                else mm_launch_mac<kMmTile>(r, sh, w, acc, fold, sc, g, acc_s, acc_i0);
                GR_HIP(r, hipGetLastError());
            }
        }
    }
    return 0;
}
// the finalize of sc ciphertexts i0 .. of acc [m_ct][d][acc_s][2][L][N] into out [.][m_ct][2][L][N]: giants [g0, g1) that `active` marks (null: all)
static int mm_finalize_chunk(sfg_ring *r, const char *what, const MmWs &w, int L, int d, int m_ct, int sc, int i0, const u64 *acc, int acc_s, const uint8_t *active, int g0, int g1,
                             int accumulate, u64 *out) {
    const int N = r->N; const size_t outw = (size_t)2 * L * N;
    std::vector<int> gl; bool with0 = false;
    for (int g = g0; g < g1; g++) { if (active && !active[g]) continue; if (g == 0) with0 = true; else gl.push_back(g); }
    GR_TRY(gr_upload(r, w.glist, gl.data(), gl.size() * sizeof(int)));
    for (int bj = 0; bj < m_ct; bj++) {
        std::vector<GrJob> jobs; std::vector<MmJob> mj;
        for (int i = 0; i < sc; i++) for (int g : gl) {
            const GrKey *k; GR_TRY(mm_key(r, what, g * d, &k));
            jobs.push_back(GrJob{k->key, k->idx, (long long)i * d + g});
            mj.push_back(MmJob{(((size_t)bj * d + g) * acc_s + i0 + i) * outw, k->idx, (long long)i * d + g});
        }
        GR_TRY(mm_rotate(r, w, jobs, mj, acc, L, L - 1, w.rot));
        const MmFinArgs a{d, L, N, m_ct, bj, (int)gl.size(), (int)with0, accumulate, acc_s, i0};
        hipLaunchKernelGGL(k_gr_mm_fin, dim3(N / GR_T, L, (unsigned)sc * 2), dim3(GR_T), 0, r->stream, acc, (const u64 *)w.rot, (const int *)w.glist, out, r->modc, a);
        GR_HIP(r, hipGetLastError());
    }
    return 0;
}
// a call starts with no refusal and no re-derivation counted
static int mm_clear_flags(sfg_ring *r, const MmWs &w) {
    GR_TRY(mm_tie_tab(r));
    GR_HIP(r, hipMemsetAsync(w.flags, 0, 8, r->stream));
    GR_HIP(r, hipMemsetAsync((unsigned *)r->tie_list + GriTies::kResolved, 0, 4, r->stream));
    return 0;
}
// the encoder's flags of a whole call, read once, with the resolver's count of re-derived coefficients (taken and cleared)
static int mm_read_flags(sfg_ring *r, const char *what, const MmWs &w, double scale) {
    unsigned f[2], resolved = 0;
    GR_HIP(r, hipMemcpyAsync(f, w.flags, 8, hipMemcpyDeviceToHost, r->stream));
    GR_HIP(r, hipMemcpyAsync(&resolved, (unsigned *)r->tie_list + GriTies::kResolved, 4, hipMemcpyDeviceToHost, r->stream));
    GR_HIP(r, hipMemsetAsync((unsigned *)r->tie_list + GriTies::kResolved, 0, 4, r->stream));
    GR_HIP(r, hipStreamSynchronize(r->stream));
    r->tie_resolved += resolved;
    return gri_encode_refuse(r, what, f, scale);
}

// the refusals the three entry points share; fills the shape
static int mm_check(sfg_ring *r, const char *what, const void *A, int s, int in_level, int max_level, const int8_t *geno, size_t nrow, size_t ncol, size_t ld, unsigned flags,
                    double scale, MmShape &sh) {
    if (!A || !geno) GR_FAIL(r, "%s: null ciphertexts or matrix", what);
    if (s < 1) GR_FAIL(r, "%s: s = %d must be positive", what, s);
    if (nrow < 1 || ncol < 1) GR_FAIL(r, "%s: the matrix needs at least one row and one column (%zu x %zu)", what, nrow, ncol);
    if (ld < ncol) GR_FAIL(r, "%s: ld %zu is below ncol %zu", what, ld, ncol);
    if (flags & ~(SFG_SQUARE | SFG_TRANSPOSE)) GR_FAIL(r, "%s: unknown flag bits 0x%x", what, flags & ~(SFG_SQUARE | SFG_TRANSPOSE));
    if (in_level < 0 || in_level >= r->nq) GR_FAIL(r, "%s: in_level %d out of range 0..%d", what, in_level, r->nq - 1);
    if (max_level < 1) GR_FAIL(r, "%s: max_level %d must be at least 1", what, max_level);
    if (max_level > r->nq) GR_FAIL(r, "%s: max_level %d out of range 1..%d", what, max_level, r->nq);
    const int lev = std::min(in_level, max_level);
    if (lev + 1 < max_level) GR_FAIL(r, "%s: in_level %d leaves %d moduli, the product at max_level %d needs %d", what, in_level, lev + 1, max_level, max_level);
    if (!(scale >= 1.0) || !std::isfinite(scale)) GR_FAIL(r, "%s: scale %g must be finite and at least 1", what, scale);
    sh.s = s; sh.in_level = in_level; sh.max_level = max_level; sh.lev = lev; sh.nl_in = in_level + 1; sh.nl = lev + 1; sh.L = max_level;
    sh.N = r->N; sh.slots = r->N / 2; sh.d = mm_d(sh.slots);
    sh.tr = flags & SFG_TRANSPOSE; sh.sq = flags & SFG_SQUARE; sh.R = sh.tr ? ncol : nrow; sh.C = sh.tr ? nrow : ncol; sh.ld = ld; sh.geno = geno; sh.scale = scale;
    sh.nbr = mm_blocks(sh.R, sh.slots); sh.m_ct = mm_blocks(sh.C, sh.slots);
    if (gr_overlap(A, (size_t)s * sh.nbr * 2 * sh.nl_in * sh.N * 8, geno, (nrow - 1) * ld + ncol)) GR_FAIL(r, "%s: the matrix overlaps A", what);
    return 0;
}
static size_t mm_budget(const sfg_ring *r) { return r->mm_budget ? r->mm_budget : kMmBudgetBytes; }
static int mm_check_keys(sfg_ring *r, const char *what, const MmShape &sh, int b0, int b1, bool babies, bool giants) {
    for (int k : mm_rotations(sh.R, sh.C, sh.slots, b0, b1, babies, giants)) GR_TRY(mm_key(r, what, k, nullptr));
    return 0;
}

/* test hook */
extern "C" int sfg_ring_set_ws_budget_for_test(sfg_ring *r, size_t bytes) {
    if (!r->test_hooks) GR_FAIL(r, "sfg_ring_set_ws_budget_for_test: test hook, enabled only in a process that set the test switch before creating the ring");
    if (!bytes) GR_FAIL(r, "sfg_ring_set_ws_budget_for_test: the budget must be positive");
    r->ws_budget = bytes; r->mm_budget = bytes;
    return 0;
}

/* test hook */
extern "C" int sfg_ring_set_tie_band_for_test(sfg_ring *r, int log2_floor) {
    if (!r->test_hooks) GR_FAIL(r, "sfg_ring_set_tie_band_for_test: test hook, enabled only in a process that set the test switch before creating the ring");
    if (log2_floor < -50 || log2_floor > -2) GR_FAIL(r, "sfg_ring_set_tie_band_for_test: the floor 2^%d is outside 2^-50 .. 2^-2", log2_floor);
    r->tie_band_log2 = log2_floor;
    return 0;
}
extern "C" int sfg_ring_encoder_resolved(sfg_ring *r, unsigned long long *count, int reset) {
    if (!count) GR_FAIL(r, "sfg_ring_encoder_resolved: null result pointer");
    *count = r->tie_resolved;
    if (reset) r->tie_resolved = 0;
    return 0;
}

extern "C" int sfg_ring_matmul_accumulate_dev(sfg_ring *r, const uint64_t *A, int s, int in_level, int max_level, const int8_t *geno, size_t nrow, size_t ncol, size_t ld, unsigned flags,
                                              double scale, int b0, int b1, uint64_t *acc, uint8_t *giant_active_host) {
    const char *what = "sfg_ring_matmul_accumulate_dev";
    GR_HIP(r, hipSetDevice(r->device));
    MmShape sh; GR_TRY(mm_check(r, what, A, s, in_level, max_level, geno, nrow, ncol, ld, flags, scale, sh));
    if (!acc) GR_FAIL(r, "%s: null accumulator", what);
    if (b0 < 0 || b1 > sh.nbr || b0 > b1) GR_FAIL(r, "%s: block rows [%d, %d) out of range 0..%d", what, b0, b1, sh.nbr);
    const size_t accw = (size_t)sh.m_ct * sh.d * s * 2 * sh.L * sh.N;
    if (gr_overlap(A, (size_t)s * sh.nbr * 2 * sh.nl_in * sh.N * 8, acc, accw * 8)) GR_FAIL(r, "%s: acc overlaps A", what);
    GR_TRY(mm_check_keys(r, what, sh, b0, b1, true, false));
    const MmPlan plan = mm_plan((size_t)s, sh.d, sh.nl, sh.L, sh.m_ct, (size_t)sh.N, false, mm_budget(r));
    GR_TRY(gr_reserve(r, r->mm_ws, plan.bytes));
    const MmWs w = mm_ws(r->mm_ws.p, mm_layout(sh.d, sh.nl, sh.L, sh.m_ct, (size_t)sh.N, plan.sc, plan.vc, false));
    GR_HIP(r, hipMemsetAsync(acc, 0, accw * 8, r->stream));
    GR_TRY(mm_clear_flags(r, w));
    for (size_t c = 0; c < plan.nsc; c++) {
        const size_t i0 = plan.first(c), sc = plan.count(c, (size_t)s);
        GR_TRY(mm_accumulate_chunk(r, what, sh, plan, w, (const u64 *)A + i0 * sh.nbr * 2 * sh.nl_in * sh.N, (int)sc, b0, b1, (u64 *)acc, s, (int)i0));
    }
    GR_TRY(mm_read_flags(r, what, w, scale));
    if (giant_active_host) {
        memset(giant_active_host, 0, sh.d);
        for (int bi = b0; bi < b1; bi++) { const MmShifts t = mm_shifts(sh.R, sh.C, sh.slots, bi); for (int g = 0; g < sh.d; g++) giant_active_host[g] |= t.giant[g]; }
    }
    return 0;
}
extern "C" int sfg_ring_matmul_finalize_dev(sfg_ring *r, const uint64_t *acc, const uint8_t *giant_active_host, int s, int max_level, int m_ct, int g0, int g1, int accumulate,
                                            uint64_t *out) {
    const char *what = "sfg_ring_matmul_finalize_dev";
    GR_HIP(r, hipSetDevice(r->device));
    if (!acc || !out) GR_FAIL(r, "%s: null accumulator or output", what);
    if (s < 1 || m_ct < 1) GR_FAIL(r, "%s: s = %d and m_ct = %d must be positive", what, s, m_ct);
    if (max_level < 1 || max_level > r->nq) GR_FAIL(r, "%s: max_level %d out of range 1..%d", what, max_level, r->nq);
    const int N = r->N, L = max_level, d = mm_d(N / 2);
    if (g0 < 0 || g1 > d || g0 > g1) GR_FAIL(r, "%s: giants [%d, %d) out of range 0..%d", what, g0, g1, d);
    const size_t accw = (size_t)m_ct * d * s * 2 * L * N, outw = (size_t)s * m_ct * 2 * L * N;
    if (gr_overlap(acc, accw * 8, out, outw * 8)) GR_FAIL(r, "%s: out overlaps acc", what);
    for (int g = std::max(g0, 1); g < g1; g++) if (!giant_active_host || giant_active_host[g]) GR_TRY(mm_key(r, what, g * d, nullptr));
    const MmPlan plan = mm_plan((size_t)s, d, L, L, m_ct, (size_t)N, false, mm_budget(r));
    GR_TRY(gr_reserve(r, r->mm_ws, plan.bytes));
    const MmWs w = mm_ws(r->mm_ws.p, mm_layout(d, L, L, m_ct, (size_t)N, plan.sc, plan.vc, false));
    for (size_t c = 0; c < plan.nsc; c++)
        GR_TRY(mm_finalize_chunk(r, what, w, L, d, m_ct, (int)plan.count(c, (size_t)s), (int)plan.first(c), (const u64 *)acc, s, giant_active_host, g0, g1, accumulate, (u64 *)out));
    return 0;
}
extern "C" int sfg_ring_matmul_dev(sfg_ring *r, const uint64_t *A, int s, int in_level, int max_level, const int8_t *geno, size_t nrow, size_t ncol, size_t ld, unsigned flags,
                                   double scale, uint64_t *out) {
    const char *what = "sfg_ring_matmul_dev";
    GR_HIP(r, hipSetDevice(r->device));
    MmShape sh; GR_TRY(mm_check(r, what, A, s, in_level, max_level, geno, nrow, ncol, ld, flags, scale, sh));
    if (!out) GR_FAIL(r, "%s: null output", what);
    const size_t outw = (size_t)sh.m_ct * 2 * sh.L * sh.N;
    if (gr_overlap(A, (size_t)s * sh.nbr * 2 * sh.nl_in * sh.N * 8, out, (size_t)s * outw * 8)) GR_FAIL(r, "%s: out overlaps A", what);
    GR_TRY(mm_check_keys(r, what, sh, 0, sh.nbr, true, true));
    const MmPlan plan = mm_plan((size_t)s, sh.d, sh.nl, sh.L, sh.m_ct, (size_t)sh.N, true, mm_budget(r));
    GR_TRY(gr_reserve(r, r->mm_ws, plan.bytes));
    const MmWs w = mm_ws(r->mm_ws.p, mm_layout(sh.d, sh.nl, sh.L, sh.m_ct, (size_t)sh.N, plan.sc, plan.vc, true));
    std::vector<uint8_t> active(sh.d, 0);
    for (int bi = 0; bi < sh.nbr; bi++) { const MmShifts t = mm_shifts(sh.R, sh.C, sh.slots, bi); for (int g = 0; g < sh.d; g++) active[g] |= t.giant[g]; }
    GR_TRY(mm_clear_flags(r, w));
    // the encoder's refusals come before `out` is written: with several chunks a checking pass over the first chunk's accumulate comes first
    for (int pass = plan.nsc > 1 ? 0 : 1; pass < 2; pass++)
        for (size_t c = 0; c < plan.nsc; c++) {
            const size_t i0 = plan.first(c), sc = plan.count(c, (size_t)s);
            GR_HIP(r, hipMemsetAsync(w.acc, 0, (size_t)sh.m_ct * sh.d * sc * 2 * sh.L * sh.N * 8, r->stream));
            GR_TRY(mm_accumulate_chunk(r, what, sh, plan, w, (const u64 *)A + i0 * sh.nbr * 2 * sh.nl_in * sh.N, (int)sc, 0, sh.nbr, w.acc, (int)sc, 0));
            GR_TRY(mm_read_flags(r, what, w, scale));
            if (pass == 0) break;                                               // the diagonals do not depend on the ciphertexts: one chunk has met them all
            GR_TRY(mm_finalize_chunk(r, what, w, sh.L, sh.d, sh.m_ct, (int)sc, 0, w.acc, (int)sc, active.data(), 0, sh.d, 0, (u64 *)out + i0 * outw));
        }
    return 0;
}
