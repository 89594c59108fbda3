// mac_dma.hip — the fp64 operand form of the rotation cache and the entry of the fp64 MAC (launch_mac_dma: the DPP-broadcast kernel, mac_bc.hip), with the
// plaintext packing and modulus planes both fp64 kernels share.  The round-1 LDS-DMA kernel this file was named after is ab/mac_dma_tiles.hip (A/B build).
#include "common.hpp"
#include "kernels.hpp"
#include <algorithm>

// rotation cache -> fp64 operand form.  in: [nct][2][nl][N] u64 ciphertext rows; out row (ct, poly) holds the
// planes of moduli 0..L-1: a "big" modulus (>= 2^36) takes 2N doubles {low 23 bits, high bits} interleaved per
// coefficient, a small one N doubles.
// centre != 0: small-modulus words are stored as the centred representative in (-q/2, q/2] (packed-limb panels)
__global__ void __launch_bounds__(256) k_rot_to_f64(const u64 *in, double *out, int nl, int L, size_t out_row_stride, const int *plane_of, const int *is_big,
                                                    int centre, const ModConst *modc) {
    const int N = SFG_N; const size_t rowl = blockIdx.x / (N / 256);         // over [ct*2][L]
    const size_t ctp = rowl / L; const int l = (int)(rowl % L);
    const size_t x = (blockIdx.x % (N / 256)) * 256 + threadIdx.x;
    const u64 w = in[(ctp * nl + l) * N + x];
    double *o = out + ctp * out_row_stride + (size_t)plane_of[l] * N;
    if (is_big[l]) {            // centred, then a SIGNED 23-bit split: |lo| <= 2^22, |hi| <= (q / 2 >> 23) + 1 - the Karatsuba middle term (lo + hi)(p_lo + p_hi) halves
        const u64 q = modc[l].qi;
        const long long wc = w > (q >> 1) ? (long long)w - (long long)q : (long long)w;
        const long long lo = ((wc + 4194304) & 0x7FFFFF) - 4194304, hi = (wc - lo) >> 23;
        o[2 * x] = (double)lo; o[2 * x + 1] = (double)hi;
    }
    else {
        const u64 q = modc[l].qi;
        o[x] = (centre && w > (q >> 1)) ? -u64_to_f64(q - w) : u64_to_f64(w);
    }
}
// plain canonical words -> packed-limb words for the small-modulus rows of a plaintext array [nrows = (k, n, l)][words]
__global__ void __launch_bounds__(256) k_pack_pt(const u64 *in, u64 *out, size_t words_per_row, int L, unsigned packed_mask) {
    const size_t row = blockIdx.y, x = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= words_per_row) return;
    const u64 w = in[row * words_per_row + x];
    out[row * words_per_row + x] = ((packed_mask >> (row % L)) & 1u) ? pack_limbs(w) : w;
}

// bit l set: the plaintext rows of modulus l use the packed-limb format (small moduli with the default broadcast kernel; not with the A/B build's plain panel / dma / reg kernels)
unsigned mac_dma_packed_mask(sfg_ctx *ctx, int L) {
    if (ctx->cfg.mac_plain_pt || ctx->cfg.mac_reg || !ctx->cfg.mac_bc) return 0u;       // the packed format is the broadcast kernel's
    return ModSplit(ctx->q, L).packed_mask_all;
}

// 46/47-bit moduli: rot words are centred and split into signed halves (k_rot_to_f64: |lo| <= 2^22, |hi| <= (q >> 24) + 1), plaintext words into
// unsigned halves (p_lo < 2^23, p_hi <= q >> 23).  The largest product of a k-step is the Karatsuba middle term.
double mac_big_maxterm(u64 q) { return (4194304.0 + (double)((q >> 24) + 1)) * (8388608.0 + (double)((q >> 23) + 1)); }
int mac_dma_planes(sfg_ctx *ctx, int L, std::vector<int> &plane_of, std::vector<int> &is_big) {
    const ModSplit m(ctx->q, L);
    if (m.too_big) { ctx->err = "sfg_mac: modulus >= 2^47 unsupported by the fp64 limb schedule"; return -1; }
    plane_of.assign(m.plane_of, m.plane_of + L); is_big.assign(m.is_big, m.is_big + L);
    return m.fp64_planes;
}

// convert nrows polynomial rows [nrows][nl_rot][N] (ciphertexts are two consecutive rows) to the fp64 operand form rotf[nrows][nplanes*N]
int launch_rot_to_f64(sfg_ctx *ctx, const u64 *rot, size_t nrows, int nl_rot, int L, double *rotf) {
    ctx->i8_gen++;                  // (as launch_rotate_right_indexed_f64)
    const int centre = mac_dma_packed_mask(ctx, L) != 0;
    const int N = SFG_N;
    std::vector<int> plane_of, is_big; const int nplanes = mac_dma_planes(ctx, L, plane_of, is_big);
    if (nplanes < 0) return 1;
    // plane tables live in the context scratch pool (one small blocking upload per call would drain the stream)
    int *d_tab = nullptr; char name[32]; snprintf(name, sizeof name, "mac.planes.%d", L);
    const bool fresh = ctx->pool.find(name) == ctx->pool.end();
    SFG_TRY(sfg_scratch(ctx, name, 2 * L * sizeof(int), (void **)&d_tab));
    if (fresh) {
        SFG_HIP(ctx, hipMemcpy(d_tab, plane_of.data(), L * sizeof(int), hipMemcpyHostToDevice));
        SFG_HIP(ctx, hipMemcpy(d_tab + L, is_big.data(), L * sizeof(int), hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_rot_to_f64, dim3((unsigned)(nrows * L * (N / 256))), dim3(256), 0, ctx->stream, rot, rotf, nl_rot, L, (size_t)nplanes * N, d_tab, d_tab + L, centre, ctx->modc);
    SFG_HIP(ctx, hipGetLastError());
    return 0;
}

int launch_pack_pt(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, size_t words_per_row, int L, unsigned packed_mask) {
    if (!nrows) return 0;
    if (nrows > 65535u * 1024u) SFG_FAIL(ctx, "pack_pt: too many rows");
    for (size_t r0 = 0; r0 < nrows; r0 += 65535u - 65535u % (unsigned)L) {          // grid.y bands that start on a multiple of L
        const size_t nr = std::min<size_t>(nrows - r0, 65535u - 65535u % (unsigned)L);
        hipLaunchKernelGGL(k_pack_pt, dim3((unsigned)((words_per_row + 255) / 256), (unsigned)nr), dim3(256), 0, ctx->stream, in + r0 * words_per_row, out + r0 * words_per_row,
                           words_per_row, L, packed_mask);
        SFG_HIP(ctx, hipGetLastError());
    }
    return 0;
}

// rotf: fp64 rotation cache with row stride nplanes*N doubles; rows_per_k = rows (ct, poly) between consecutive k.
// st.pt_packed: the small-modulus plaintext rows hold packed-limb words and rotf is centred (broadcast kernel only).
// Contract: when K % 4 != 0 the buffer must extend over the k-slices K .. 4*ceil(K/4)-1 and hold finite doubles there
// (they are multiplied by zero plaintexts).
int launch_mac_dma(sfg_ctx *ctx, const double *rotf, size_t rows_per_k, const u64 *pt, u64 *out, int K, int R, int Ncols, int L, int accumulate,
                   const MacStrides &st) {
    if (ctx->cfg.mac_bc && (st.pt_packed || mac_dma_packed_mask(ctx, L) == 0) && !ctx->cfg.mac_plain_pt)      // default: the DPP-broadcast kernel (mac_bc.hip)
        return launch_mac_bc(ctx, rotf, rows_per_k, pt, out, K, R, Ncols, L, accumulate, st);
#ifdef SFG_AB
    return ab_launch_mac_dma_tiles(ctx, rotf, rows_per_k, pt, out, K, R, Ncols, L, accumulate, st);
#endif
    SFG_FAIL(ctx, "the LDS-DMA baseline MAC kernel exists in the A/B build only (make ab)");
}

// (A/B build: SFG_MAC_IMPL=reg selects the register-staged kernel of ab/mac_reg.hip)
bool mac_use_dma(const sfg_ctx *ctx) { return !ctx->cfg.mac_reg; }

extern "C" int sfg_mac_dev(sfg_ctx *ctx, const uint64_t *rot, const uint64_t *pt, uint64_t *out, int K, int R, int Ncols, int L, int accumulate) {
    SFG_HIP(ctx, hipSetDevice(ctx->device));
    if (L < 1 || L > ctx->nq) SFG_FAIL(ctx, "sfg_mac: L out of range");
    if (K < 1 || R < 1 || Ncols < 1) SFG_FAIL(ctx, "sfg_mac: K, R and Ncols must be positive (got %d, %d, %d)", K, R, Ncols);
    PhaseTimer t(ctx, "mac");
#ifdef SFG_AB
    if (!mac_use_dma(ctx)) { const int r = launch_mac(ctx, (const u64 *)rot, (const u64 *)pt, (u64 *)out, K, R, Ncols, L, accumulate); t.stop(1); return r; }    // ab/mac_reg.hip
#endif
    int rc;
    {
        std::vector<int> plane_of, is_big; const int nplanes = mac_dma_planes(ctx, L, plane_of, is_big);
        if (nplanes < 0) return 1;
        double *rotf = nullptr;
        const size_t rows = (size_t)K * R;                       // rot is [K][R][L][N]
        const size_t pad_rows = (size_t)((4 - K % 4) % 4) * R;       // k-slices read (against zero plaintexts) by the ragged last chunk
        SFG_HIP(ctx, hipMalloc(&rotf, (rows + pad_rows) * (size_t)nplanes * SFG_N * 8));
        if (pad_rows) SFG_HIP(ctx, hipMemsetAsync(rotf + rows * (size_t)nplanes * SFG_N, 0, pad_rows * (size_t)nplanes * SFG_N * 8, ctx->stream));
        rc = launch_rot_to_f64(ctx, (const u64 *)rot, rows, L, L, rotf);
        MacStrides st;
        st.rot_k = (size_t)R * L * SFG_N; st.rot_r = (size_t)L * SFG_N;
        st.pt_k = (size_t)Ncols * L * SFG_N; st.pt_n = (size_t)L * SFG_N;
        st.out_n = (size_t)R * L * SFG_N; st.out_r = (size_t)L * SFG_N;
        // default build: the small-modulus plaintext rows go through the packed-limb format the product path uses (A/B build, plain panel: as given)
        const unsigned pmask = mac_dma_packed_mask(ctx, L);
        u64 *ptp = nullptr;
        if (!rc && pmask) {
            const size_t prows = (size_t)K * Ncols * L;
            if (hipMalloc(&ptp, prows * SFG_N * 8) != hipSuccess) { rc = 1; ctx->err = "sfg_mac: out of device memory"; }
            if (!rc) rc = launch_pack_pt(ctx, (const u64 *)pt, ptp, prows, SFG_N, L, pmask);
            st.pt_packed = true;
        }
        if (!rc) rc = launch_mac_dma(ctx, rotf, (size_t)R, pmask ? ptp : (const u64 *)pt, (u64 *)out, K, R, Ncols, L, accumulate, st);
        (void)hipStreamSynchronize(ctx->stream); (void)hipFree(rotf); (void)hipFree(ptp);
    }
    t.stop(1);
    return rc;
}
