// gring_dev.hpp - what the general ring's translation units share (gring.hip: the ring, its transform, its evaluator; gring_io.hip: keys, sampler, encryption,
// collective decryption): the device-side tables, struct sfg_ring, the error macros and the host helpers gring.hip defines.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <map>
#include <string>
#include "../../include/sfgwas_hip.h"
#include "gring_arith.hpp"
#include "gring_plan.hpp"

using gr::u64;
using gr::u128;

// ---------------------------------------------------------------- device-side tables
struct GrMod { u64 q, uhi, ulo, ninv, ninv_sh, r64inv, r64inv_sh; };        // per modulus: q, floor(2^128 / q), N^-1 and 2^-64 with their Shoup quotients
// which modulus a row of a batch belongs to: an explicit table, or t = row % period, t < split ? t + base0 : t - split + base1
struct GrRowMap { const int *table; int period, split, base0, base1; };
__device__ __forceinline__ int gr_row_mod(const GrRowMap &m, size_t row) {
    if (m.table) return m.table[row];
    int t = (int)(row % (size_t)m.period);
    return t < m.split ? t + m.base0 : t - m.split + m.base1;
}
// one basis-extension configuration (lattigo modUpExact): sources in digits of alpha moduli, a list of target moduli
struct GrExt {
    int nsrc, ndig, alpha, tgt_cap;
    const int *src_mod;       // [nsrc]
    const u64 *inv;           // [nsrc][2]   (D / q_m)^-1 mod q_m of the source's digit, and its Shoup quotient
    const int *tgt_mod;       // [tgt_cap]
    const int *tgt_src;       // [ndig][tgt_cap]   source row when the target is one of the digit's own moduli, else -1
    const u64 *tgt_tab;       // [ndig][tgt_cap][1 + alpha]   D mod qt, then (D / q_m) mod qt
};
struct GrJob { const u64 *key; const uint32_t *idx; long long ct; };     // one key switch of a batch: its key, its automorphism index (or null), its ciphertext
struct GrScalars { u64 s[gr::kMaxMod]; };

constexpr int GR_T = 256;

// ---------------------------------------------------------------- host side
struct GrKey { u64 *key = nullptr; uint32_t *idx = nullptr; };
struct GrExtOwner { GrExt e{}; void *buf = nullptr; };
struct GrLevel { GrExtOwner up; u64 *rescale_tab = nullptr; };
// keys and sampler of gring_io.hip: the public key [2][nmod][N], the secret key [nq][N] (both NTT domain, canonical), the ChaCha20 key and the encryption index
struct GrIo {
    u64 *pk = nullptr, *sk = nullptr;
    uint32_t enc_key[8] = {}; uint32_t *enc_key_dev = nullptr; bool enc_seeded = false;
    unsigned long long enc_next = 0;                   // ONE atomic counter per ring
    void *ws = nullptr; size_t ws_bytes = 0;           // grow-only workspace of the encryption core and of the decoder
    std::map<int, void *> dec_tabs;                    // the decoder's tables of a level (mixed-radix constants, the digits of floor(Q / 2)), built at its first use
    void *dd_tab = nullptr;                            // the double-double transform's tables (twiddles, twist, slot permutation), built at first use
    void *pt = nullptr; size_t pt_bytes = 0;           // grow-only plaintext rows between the encoder and the encryption core, and between decryption and the decoder
    size_t ws_budget = 512ull << 20;
};
struct sfg_ring {
    int device = 0, logN = 0, N = 0, nq = 0, np = 0, nmod = 0, beta = 0;
    u64 q[gr::kMaxMod] = {}, psi[gr::kMaxMod] = {};
    GrNttPlan plan;
    hipStream_t stream = nullptr;
    GrMod *modc = nullptr; u64 *tw = nullptr; u64 *pinv = nullptr;
    GrExtOwner down;                                   // ModDown: P -> Q
    std::map<int, GrLevel> levels;
    std::map<u64, GrKey> rotkeys; GrKey rlk;
    void *ws = nullptr; size_t ws_bytes = 0;           // grow-only workspace of the key switch and the rescale
    int *modidx = nullptr; size_t modidx_cap = 0;      // sfg_ring_ntt_rows' modulus table
    unsigned char *pin = nullptr; size_t pin_bytes = 0, pin_head = 0;       // pinned staging of small uploads
    void *small = nullptr; size_t small_bytes = 0;     // the inner sum's rotated ciphertext
    size_t ws_budget = 768ull << 20;
    bool test_hooks = false;                           // SFG_ENABLE_TEST_HOOKS=1 when the ring was made: the *_for_test entry points may be called
    GrIo io;
    std::string err;
};
#define GR_FAIL(r, ...) do { char _b[512]; snprintf(_b, sizeof _b, __VA_ARGS__); (r)->err = _b; return 1; } while (0)
#define GR_HIP(r, call) do { hipError_t _e = (call); if (_e != hipSuccess) { char _b[512]; \
    snprintf(_b, sizeof _b, "HIP call failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); (r)->err = _b; return 1; } } while (0)
#define GR_TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// gring.hip
int gr_upload(sfg_ring *r, void *dst, const void *src, size_t bytes);
int gr_reserve(sfg_ring *r, void **buf, size_t *have, size_t bytes);
int gr_transform(sfg_ring *r, u64 *rows, size_t nrows, GrRowMap map, bool inv);
GrRowMap gr_map(int period, int split, int base0, int base1);
int gr_extend(sfg_ring *r, const GrExt &e, const u64 *src, u64 *Y, uint32_t *V, u64 *out, int ntgt, size_t npoly);
int gr_check_level(sfg_ring *r, const char *what, int nct, int level);
int gr_rows_from_mont(sfg_ring *r, u64 *rows, size_t nrows);      // lattigo ring.InvMForm on key rows [.][nmod][N], enqueued on the ring's stream
// gring_io.hip: wipes and frees the keys and the sampler (sfg_ring_destroy)
void gr_io_destroy(sfg_ring *r);
