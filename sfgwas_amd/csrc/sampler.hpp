// sampler.hpp — the keyed ChaCha20 stream and its byte-to-sample map (DESIGN.md "Encryption on the device"), shared by the encryptor (encrypt.hip) and the
// collective key generation (keygen.hip), which draws its error polynomials and its ephemeral secret from the same stream and the same index counter.
#pragma once
#include "common.hpp"

// ---------------------------------------------------------------- the keyed stream
__device__ __forceinline__ unsigned rotl32(unsigned x, int n) { return __builtin_rotateleft32(x, n); }
#define SFG_QR(a, b, c, d) do { a += b; d ^= a; d = rotl32(d, 16); c += d; b ^= c; b = rotl32(b, 12); a += b; d ^= a; d = rotl32(d, 8); c += d; b ^= c; b = rotl32(b, 7); } while (0)
// one ChaCha20 block (RFC 8439 2.3): key words k[8], 32-bit block counter, nonce words n0, n1, n2 -> 16 output words
__device__ __forceinline__ void chacha20_block(const unsigned (&k)[8], unsigned counter, unsigned n0, unsigned n1, unsigned n2, unsigned (&o)[16]) {
    const unsigned s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], counter, n0, n1, n2};
    unsigned x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#pragma unroll 1
    for (int r = 0; r < 10; r++) {
        SFG_QR(x[0], x[4], x[8], x[12]); SFG_QR(x[1], x[5], x[9], x[13]); SFG_QR(x[2], x[6], x[10], x[14]); SFG_QR(x[3], x[7], x[11], x[15]);
        SFG_QR(x[0], x[5], x[10], x[15]); SFG_QR(x[1], x[6], x[11], x[12]); SFG_QR(x[2], x[7], x[8], x[13]); SFG_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) o[i] = x[i] + s[i];
}
// Rounded Gaussian, sigma = 3.2, cut at 19: cumulative distribution of the MAGNITUDE as 63-bit thresholds, C[k] = round(2^63 (p_0 + 2 p_1 + .. + 2 p_k)),
// p_k = (Phi((k + 1/2) / sigma) - Phi((k - 1/2) / sigma)) / Z renormalised over |k| <= 19 (a drawn -0 is 0: magnitude 0 carries p_0 whatever the sign bit).
// Derived with mpmath at 400 bits (tests/test_encrypt_ref.py recomputes every entry); C[19] = 2^63 exactly.
static __constant__ u64 ENC_GAUSS_CUM[20] = {
    0x0fe49b6827cb0a22ULL, 0x2e2d1c3d2d673909ULL, 0x485d35a4168455fbULL, 0x5ceb732fcf500f03ULL, 0x6b909790cec541bcULL,
    0x750918a85086780aULL, 0x7a98381b8b05d44bULL, 0x7d8e6d674ccde58aULL, 0x7efd1569779956edULL, 0x7f9e04eac7bbada7ULL,
    0x7fde228ae318bb83ULL, 0x7ff551b87c6c82e1ULL, 0x7ffcedaa42aca3e8ULL, 0x7fff31ef2eb41935ULL, 0x7fffced272bc4241ULL,
    0x7ffff5523bb74b16ULL, 0x7ffffde5526b5cebULL, 0x7fffffa10a4c8db3ULL, 0x7ffffff2720cd7c6ULL, 0x8000000000000000ULL};
// 64 stream bits -> one sample: bit 0 the sign, bits 1..63 against all 20 thresholds (no early exit: every coefficient costs the same)
__device__ __forceinline__ int gauss_from_bits(unsigned lo, unsigned hi) {
    const u64 r = ((u64)hi << 32) | lo, x = r >> 1;
    int mag = 0;
#pragma unroll
    for (int k = 0; k < 20; k++) mag += x >= ENC_GAUSS_CUM[k] ? 1 : 0;
    return (r & 1) ? -mag : mag;
}
// The samples of thread `tid` (of 512) for encryption `index`: its 32 coefficients j = a * 512 + tid of u, e0, e1, one signed byte each, coefficient a in
// byte a & 3 of dword a >> 2.
//   u  (polynomial 0, blocks 0..63):   block tid >> 3, the 64 bits r = w[2 (tid & 7)] | w[2 (tid & 7) + 1] << 32; bits 2a, 2a + 1 = (b0, b1): b0 ? (b1 ? -1 : +1) : 0
//   e  (polynomial 1 / 2, blocks 0..2047): block tid + 512 (a >> 3), r = w[2 (a & 7)] | w[2 (a & 7) + 1] << 32 -> gauss_from_bits
__device__ __forceinline__ void enc_sample_thread(const unsigned (&key)[8], u64 index, int tid, unsigned (&su)[8], unsigned (&s0)[8], unsigned (&s1)[8]) {
    const unsigned n0 = (unsigned)index, n1 = (unsigned)(index >> 32);
    unsigned w[16];
    chacha20_block(key, (unsigned)(tid >> 3), n0, n1, 0u, w);
    {
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) if ((tid & 7) == i) { lo = w[2 * i]; hi = w[2 * i + 1]; }
        const u64 r = ((u64)hi << 32) | lo;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int a = 4 * d + b; const unsigned two = (unsigned)(r >> (2 * a)) & 3u;
                const unsigned byte = (two & 1u) ? ((two & 2u) ? 0xFFu : 1u) : 0u;
                v |= byte << (8 * b);
            }
            su[d] = v;
        }
    }
#pragma unroll 1
    for (int pol = 0; pol < 2; pol++) {
        unsigned acc[8];
#pragma unroll
        for (int blk = 0; blk < 4; blk++) {
            chacha20_block(key, (unsigned)(tid + 512 * blk), n0, n1, (unsigned)(1 + pol), w);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                unsigned v = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) { const int k = 4 * h + b; v |= ((unsigned)gauss_from_bits(w[2 * k], w[2 * k + 1]) & 0xFFu) << (8 * b); }
                acc[2 * blk + h] = v;
            }
        }
#pragma unroll
        for (int d = 0; d < 8; d++) { if (pol == 0) s0[d] = acc[d]; else s1[d] = acc[d]; }
    }
}
__device__ __forceinline__ double byte_of(const unsigned (&s)[8], int a) { return (double)(int)(int8_t)(s[a >> 2] >> (8 * (a & 3))); }
// one Gaussian polynomial alone (polynomial id `pol` = 1 or 2 of encryption `index`): the same bytes, the same map as enc_sample_thread's e0 / e1 (keygen.hip)
__device__ __forceinline__ void enc_sample_e_thread(const unsigned (&key)[8], u64 index, unsigned pol, int tid, unsigned (&s)[8]) {
    const unsigned n0 = (unsigned)index, n1 = (unsigned)(index >> 32);
    unsigned w[16];
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
        chacha20_block(key, (unsigned)(tid + 512 * blk), n0, n1, pol, w);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) { const int k = 4 * h + b; v |= ((unsigned)gauss_from_bits(w[2 * k], w[2 * k + 1]) & 0xFFu) << (8 * b); }
            s[2 * blk + h] = v;
        }
    }
}
// the ternary polynomial alone (polynomial id 0 of encryption `index`): enc_sample_thread's u
__device__ __forceinline__ void enc_sample_u_thread(const unsigned (&key)[8], u64 index, int tid, unsigned (&su)[8]) {
    unsigned w[16];
    chacha20_block(key, (unsigned)(tid >> 3), (unsigned)index, (unsigned)(index >> 32), 0u, w);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) if ((tid & 7) == i) { lo = w[2 * i]; hi = w[2 * i + 1]; }
    const u64 r = ((u64)hi << 32) | lo;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        unsigned v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int a = 4 * d + b; const unsigned two = (unsigned)(r >> (2 * a)) & 3u;
            const unsigned byte = (two & 1u) ? ((two & 2u) ? 0xFFu : 1u) : 0u;
            v |= byte << (8 * b);
        }
        su[d] = v;
    }
}
