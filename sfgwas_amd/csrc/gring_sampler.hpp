// gring_sampler.hpp - the general ring's keyed sampler on the device: the one draw of a thread's eight coefficients of u and of up to two Gaussian polynomials
// from the ChaCha20 stream, shared by gring_io.hip (encryption, the transcript hook) and gring_keygen.hip (the key-generation shares) so that neither restates
// the map (gring_io_arith.hpp) nor the byte-to-sample tables (sampler.hpp).  Included by .hip files only, after gring_dev.hpp.
#pragma once
#include "gring_io_arith.hpp"
#include "sampler.hpp"        // chacha20_block, gauss_from_bits and the Gaussian table: shared with encrypt.hip and keygen.hip, not forked

// words idx, idx + 1 of a block without a dynamically indexed register array (idx even, < 16)
__device__ __forceinline__ u64 gri_pick(const unsigned (&w)[16], int idx) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) if (idx == 2 * i) { lo = w[2 * i]; hi = w[2 * i + 1]; }
    return ((u64)hi << 32) | lo;
}
// Thread (t, g), t < 512, g < N / 4096, owns the 8 coefficients j = 512 (8 g + k) + t, k < 8: one block of each Gaussian polynomial serves exactly these 8 (word pair
// k), and one block of u holds their 8 bit pairs.  Three ChaCha20 blocks a thread.
__device__ __forceinline__ void gri_sample8(const unsigned (&key)[8], u64 index, int t, int g, bool want_u, int npoly, int (&su)[8], int (&s0)[8], int (&s1)[8]) {
    const unsigned n0 = (unsigned)index, n1 = (unsigned)(index >> 32);
    unsigned w[16];
    if (want_u) {
        chacha20_block(key, gio::samp_u_block(t, 8 * g), n0, n1, 0u, w);
        const u64 r = gri_pick(w, gio::samp_u_word(t));
#pragma unroll
        for (int k = 0; k < 8; k++) su[k] = gio::samp_ternary(r, gio::samp_u_shift(8 * g + k));
    }
#pragma unroll 1
    for (int pol = 0; pol < npoly; pol++) {
        chacha20_block(key, gio::samp_e_block(t, 8 * g), n0, n1, (unsigned)(1 + pol), w);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const u64 r = gri_pick(w, gio::samp_e_word(8 * g + k));
            const int v = gauss_from_bits((unsigned)r, (unsigned)(r >> 32));
            if (pol == 0) s0[k] = v; else s1[k] = v;
        }
    }
}
