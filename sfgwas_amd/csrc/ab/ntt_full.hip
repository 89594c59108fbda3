// ab/ntt_full.hip — the full-image form of the plaintext NTT (round 1; SFG_NTT_HALF_IMPL=full, A/B build only).  The product's form is k_ntt_half3 (ntt.hip):
// every exchange through a half image, three workgroups per CU instead of two.
#include "../common.hpp"
#include "../kernels.hpp"
#include "../ntt_core.hpp"

constexpr int HLDS_DOUBLES = 16 * LDS_ROW;   // 67,584 B
__global__ void __launch_bounds__(256) k_ntt_half(const double *pc_all, u64 *out_, size_t nplain, int L, PanelMap pm, const double *tw_all, const double2 *pack_all, const ModConst *modc) {
    extern __shared__ double lds[];
    const int N = SFG_N, n = N / 2, tid = threadIdx.x;
    size_t row; int m;
    if (!plain_block(nplain, L, row, m)) return;
    const double *tw = tw_all + (size_t)m * N;
    const double2 *pack = pack_all + (size_t)m * (N / 2);
    const double q = modc[m].q, qinv = modc[m].qinv;
    const double *pc = pc_all + (row / L) * (size_t)n;
    const double W = tw[1], Wq = W * qinv;
    double v[32];
    // ---- phase A: two (b,c) columns per thread, 16 values of a each; stages t = 4096, 2048, 1024, 512
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int pp = tid + 256 * h;
        double w[16];
#pragma unroll
        for (int a = 0; a < 16; a++) {
            const int j = a * 512 + pp;
            const double lo = pc[j];
            const double hi = j == 0 ? 0.0 : pc[n - j];          // p_{n+j} = -p_{n-j}
            w[a] = lo - mulmod_lazy(hi, W, Wq, q);
        }
        ct_stage<16, 8>(w, q, qinv, [&](int g) { return tw[2 + g]; });
        ct_stage<16, 4>(w, q, qinv, [&](int g) { return tw[4 + g]; });
        ct_stage<16, 2>(w, q, qinv, [&](int g) { return tw[8 + g]; });
        ct_stage<16, 1>(w, q, qinv, [&](int g) { return tw[16 + g]; });
#pragma unroll
        for (int a = 0; a < 16; a++) lds[a * LDS_ROW + pp] = w[a];
    }
    __syncthreads();
    // ---- phase B: thread (a, c), 32 values of b; stages t = 256 .. 16
    {
        const int a = tid >> 4, c = tid & 15;
#pragma unroll
        for (int b = 0; b < 32; b++) v[b] = lds[a * LDS_ROW + b * 16 + c];
        ct_stage<32, 16>(v, q, qinv, [&](int g) { return tw[32 + a + g]; });
        ct_stage<32, 8>(v, q, qinv, [&](int g) { return tw[64 + a * 2 + g]; });
        ct_stage<32, 4>(v, q, qinv, [&](int g) { return tw[128 + a * 4 + g]; });
        ct_stage<32, 2>(v, q, qinv, [&](int g) { return tw[256 + a * 8 + g]; });
        ct_stage<32, 1>(v, q, qinv, [&](int g) { return tw[512 + a * 16 + g]; });
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 32; b++) lds[a * LDS_ROW + c * 33 + b] = v[b];
    }
    __syncthreads();
    // ---- phase C: two (a, b) groups per thread, 16 values of c; stages t = 8 .. 1 with the packed twiddles
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int p = tid + 256 * h, a = p >> 5, b = p & 31;
        double w[16];
#pragma unroll
        for (int c = 0; c < 16; c++) w[c] = lds[a * LDS_ROW + c * 33 + b];
        double tl[16];
        {
            const double2 *pk = pack + (size_t)(p >> 6) * 512 + (p & 63);
#pragma unroll
            for (int i = 0; i < 8; i++) { const double2 e = pk[i * 64]; tl[2 * i] = e.x; tl[2 * i + 1] = e.y; }
        }
        ct_stage<16, 8>(w, q, qinv, [&](int g) { return tl[0 + g]; });
        ct_stage<16, 4>(w, q, qinv, [&](int g) { return tl[1 + g]; });
        ct_stage<16, 2>(w, q, qinv, [&](int g) { return tl[3 + g]; });
        ct_stage<16, 1>(w, q, qinv, [&](int g) { return tl[7 + g]; });
#pragma unroll
        for (int c = 0; c < 16; c++) v[h * 16 + c] = w[c];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int p = tid + 256 * h, a = p >> 5, b = p & 31;
#pragma unroll
        for (int c = 0; c < 16; c++) lds[a * LDS_ROW + c * 33 + b] = v[h * 16 + c];
    }
    __syncthreads();
    // destination plaintext slot inside a (possibly multi-block-row) panel: see PanelMap
    const size_t plain = row / L; const int shift = pm.shift0 + (int)plain;
    const size_t dst = pm.G ? ((size_t)(shift / SFG_D) * pm.G + pm.g) * SFG_D + (size_t)(shift % SFG_D) : plain;
    u64 *out = out_ + (dst * L + m) * (size_t)n;
    const bool packed = (pm.packed_mask >> m) & 1u;
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const int j = k * 256 + tid, a = j >> 9, x = j & 511, b = x >> 4, c = x & 15;
        const u64 w = f64_to_u64(canon(lds[a * LDS_ROW + c * 33 + b], q, qinv));
        out[j] = packed ? pack_limbs(w) : w;
    }
}

int ab_ntt_set_attrs(sfg_ctx *ctx) {
    SFG_HIP(ctx, hipFuncSetAttribute((const void *)k_ntt_half, hipFuncAttributeMaxDynamicSharedMemorySize, HLDS_DOUBLES * 8));
    return 0;
}
int ab_launch_ntt_half_full(sfg_ctx *ctx, const double *pc, u64 *out_half, size_t nplain, int L, const PanelMap &pm) {
    hipLaunchKernelGGL(k_ntt_half, dim3((unsigned)((nplain + 7) / 8 * 8 * L)), dim3(256), HLDS_DOUBLES * 8, ctx->stream, pc, out_half, nplain, L, pm, ctx->tw_fwd, ctx->pack_fwd, ctx->modc);
    return 0;
}
