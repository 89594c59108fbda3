// ab/mac_i8_lds.hip — the int8 MAC with LDS-staged rot tiles (round 3, SFG_MAC_I8_ROT=lds, A/B build only): measured slower than the cache-shared k_mac_i8 and
// the product's ring form k_mac_i8_ring (mac_i8.hip), whose launch contract - I8Args, tile layouts, results in tile order - it shares.
#include "../common.hpp"
#include "../kernels.hpp"
#include "../i8_move.hpp"

// ---- the same with the rot tiles of the pair staged through LDS (six column waves: the product's 91 columns).  Through the cache alone the six waves fetched
// them 2.8 x (PMC); here the workgroup loads the 20 KiB of a chunk once - the next chunk's pieces travel in registers beside the current chunk's MFMAs - and every
// wave reads its 20 operand tiles from the 2 x 20 KiB image.
__global__ void __launch_bounds__(384, 1) k_mac_i8_lds(I8Args a, const ModConst *modc) {
    __shared__ uint4 As[2][2 * 2 * I8_ND * 64];
    const int N = SFG_N, H = N / 2, tid = threadIdx.x;
    const int lane = tid & 63, jt = tid >> 6;
    const int c = blockIdx.x % H, m = blockIdx.x / H;
    const double q = modc[a.l0 + m].q, qinv = modc[a.l0 + m].qinv;
    v4i acc[4][9];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int s = 0; s < 9; s++) acc[t][s] = (v4i){0, 0, 0, 0};
    const uint4 *Bp = reinterpret_cast<const uint4 *>(a.B) + ((((size_t)m * H + c) * a.njt + jt) * a.nch) * I8_ND * 64 + lane;
    const uint4 *A0 = reinterpret_cast<const uint4 *>(a.A) + (((size_t)m * N + c) * a.nch) * 2 * I8_ND * 64;
    const uint4 *A1 = reinterpret_cast<const uint4 *>(a.A) + (((size_t)m * N + (N - 1 - c)) * a.nch) * 2 * I8_ND * 64;
    constexpr int HALF = 2 * I8_ND * 64;               // uint4 per coefficient and chunk (10 KiB)
    // piece i < 2 HALF of chunk ch: coefficient half i / HALF, offset i % HALF; thread tid takes pieces tid, tid + 384, ...
    auto src = [&](int ch, int i) { return (i < HALF ? A0 : A1) + (size_t)ch * HALF + (i < HALF ? i : i - HALF); };
    uint4 stage[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const int i = tid + 384 * u; if (i < 2 * HALF) As[0][i] = *src(0, i); }
    __syncthreads();
#pragma unroll 1
    for (int ch = 0; ch < a.nch; ch++) {
        const bool more = ch + 1 < a.nch;
        if (more) {
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = tid + 384 * u; if (i < 2 * HALF) stage[u] = *src(ch + 1, i); }
        }
        v4i b[I8_ND];
#pragma unroll
        for (int d = 0; d < I8_ND; d++) { const uint4 w = Bp[(size_t)(ch * I8_ND + d) * 64]; b[d] = (v4i){(int)w.x, (int)w.y, (int)w.z, (int)w.w}; }
        const uint4 *Ac = As[ch & 1];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int x = 0; x < I8_ND; x++) {
                const uint4 w = Ac[(t * I8_ND + x) * 64 + lane];
                const v4i av = (v4i){(int)w.x, (int)w.y, (int)w.z, (int)w.w};
#pragma unroll
                for (int d = 0; d < I8_ND; d++) acc[t][x + d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b[d], acc[t][x + d], 0, 0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = tid + 384 * u; if (i < 2 * HALF) As[(ch + 1) & 1][i] = stage[u]; }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        u64 *o = a.T + ((((((size_t)m * H + c) * 2 + (t >> 1)) * a.njt + jt) * 2 + (t & 1)) * 64 + lane) * 4;
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = (u64)i8_horner(acc[t], e, q, qinv, false);       // (five digits: q < 2^39)
    }
}
void ab_launch_mac_i8_lds(hipStream_t q, const I8Args &a, const ModConst *modc, int nl) {
    hipLaunchKernelGGL(k_mac_i8_lds, dim3((unsigned)(nl * (SFG_N / 2))), dim3(384), 0, q, a, modc);
}
