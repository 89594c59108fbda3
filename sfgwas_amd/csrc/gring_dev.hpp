// gring_dev.hpp - what the general ring's translation units share (gring.hip: the ring, its transform, its evaluator; gring_io.hip: keys, sampler, encryption,
// collective decryption; gring_matmul.hip: the matrix products, which batch their rotations through gr_ks_batch and share the encoder's device half): the device-side tables, the owners of what a ring holds, struct sfg_ring, the error macros, the host modular helpers and the host
// functions gring.hip defines.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>
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
static_assert(sizeof(GrJob) == kGrJobBytes, "gring_plan.hpp sizes the key switch's job list");
struct GrScalars { u64 s[gr::kMaxMod]; };

constexpr int GR_T = 256;

// ---------------------------------------------------------------- owners (move-only; the ring's device must be current when one lets go)
// one device allocation; a wiping one is zeroed, and the device synchronised, before it is freed
struct GrMem {
    void *p = nullptr; size_t bytes = 0; bool wipe = false;
    GrMem() {}
    GrMem(GrMem &&o) : p(o.p), bytes(o.bytes), wipe(o.wipe) { o.p = nullptr; o.bytes = 0; }
    GrMem &operator=(GrMem &&o) { if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    GrMem(const GrMem &) = delete; GrMem &operator=(const GrMem &) = delete;
    ~GrMem() { reset(); }
    void reset() {
        if (!p) return;
        if (wipe) { (void)hipMemset(p, 0, bytes); (void)hipDeviceSynchronize(); }
        (void)hipFree(p); p = nullptr; bytes = 0;
    }
    hipError_t alloc(size_t n) { reset(); const hipError_t e = hipMalloc(&p, n); if (e == hipSuccess) bytes = n; else p = nullptr; return e; }
};
template <class T> struct GrBuf : GrMem { operator T *() const { return (T *)p; } };
template <class T> struct GrSecret : GrBuf<T> { GrSecret() { this->wipe = true; } };
template <class T, hipError_t (*Free)(T)> struct GrHandle {             // the stream, the pinned staging buffer
    T h = T();
    GrHandle() {}
    GrHandle(const GrHandle &) = delete; GrHandle &operator=(const GrHandle &) = delete;
    ~GrHandle() { if (h) (void)Free(h); }
    operator T() const { return h; }
};

// ---------------------------------------------------------------- host side
struct GrKey { GrBuf<u64> key; GrBuf<uint32_t> idx; };
struct GrExtOwner { GrExt e{}; GrBuf<void> buf; };
struct GrLevel { GrExtOwner up; GrBuf<u64> rescale_tab; };
// keys and sampler of gring_io.hip: the public key [2][nmod][N], the secret key [nq][N] (both NTT domain, canonical), the ChaCha20 key and the encryption index
struct GrIo {
    GrBuf<u64> pk; GrSecret<u64> sk;
    uint32_t enc_key[8] = {}; GrSecret<uint32_t> enc_key_dev; bool enc_seeded = false;
    unsigned long long enc_next = 0;                   // ONE atomic counter per ring
    GrSecret<void> ws;                                 // grow-only workspace of the encryption core, the encoder and the decoders: lifted samples
    std::map<int, GrBuf<u64>> dec_tabs;                // the decoder's tables of a level (mixed-radix constants, the digits of floor(Q / 2)), built at its first use
    GrBuf<void> dd_tab;                                // the double-double transform's tables (twiddles, twist, slot permutation), built at first use
    GrSecret<u64> pt;                                  // grow-only plaintext rows between the encoder and the encryption core, and between decryption and the decoder
    size_t ws_budget = 512ull << 20;
};
// key generation (gring_keygen.hip): the secret key over Q and P [nmod][N] (NTT domain, canonical), P mod q_m with its Shoup quotient [nmod][2] (the rows of P zero), the index
// tables of a chunk of rotation keys, and NTT(u) of a relinearisation round
struct GrKeygen {
    GrSecret<u64> skqp; GrBuf<u64> pmod;
    GrBuf<void> index;                                 // grow-only
    GrSecret<u64> u;                                   // grow-only, wiping
};
struct sfg_ring {
    int device = 0, logN = 0, N = 0, nq = 0, np = 0, nmod = 0, beta = 0;
    u64 q[gr::kMaxMod] = {}, psi[gr::kMaxMod] = {};
    GrNttPlan plan;
    GrHandle<hipStream_t, hipStreamDestroy> stream;    // declared before every allocation: destroyed after them
    GrHandle<void *, hipHostFree> pin; size_t pin_bytes = 0, pin_head = 0;  // pinned staging of small uploads
    GrBuf<GrMod> modc; GrBuf<u64> tw, pinv;
    GrExtOwner down;                                   // ModDown: P -> Q
    std::map<int, GrLevel> levels;
    std::map<u64, GrKey> rotkeys; GrKey rlk;
    GrBuf<void> ws;                                    // grow-only workspace of the key switch and the rescale
    GrBuf<int> modidx;                                 // sfg_ring_ntt_rows' modulus table
    GrBuf<u64> small;                                  // the inner sum's rotated ciphertext
    GrBuf<u64> mm_fold;                                // gring_matmul.hip: the fold bound of every modulus row (32-bit), built at first use
    GrBuf<void> mm_ws;                                 // grow-only workspace of the matrix products (gring_matmul.hip), apart from ws: the key switches they batch use that one
    size_t ws_budget = 768ull << 20;
    size_t mm_budget = 0;                              // the products' workspace budget; 0 = kMmBudgetBytes (gring_matmul_plan.hpp)
    GrBuf<u64> tie_tab;                                // gring_matmul.hip: the fixed-point cosine table of the tie resolver (gring_tie.hpp), built at first use
    GrBuf<unsigned> tie_list;                          // the resolver's list of one batch (GriTies), allocated with the table
    unsigned long long tie_resolved = 0;               // coefficients re-derived since the last reset (sfg_ring_encoder_resolved)
    int tie_band_log2 = -50;                           // the floor of the band of the products' diagonals (sfg_ring_set_tie_band_for_test)
    bool test_hooks = false;                           // SFG_ENABLE_TEST_HOOKS=1 when the ring was made: the *_for_test entry points may be called
    GrIo io;
    GrKeygen kg;
    std::map<int, GrBuf<u64>> rf_tabs;                 // gring_refresh.hip: the recode's tables of a level, built at its first use
    std::string err;
};
#define GR_FAIL(r, ...) do { char _b[512]; snprintf(_b, sizeof _b, __VA_ARGS__); (r)->err = _b; return 1; } while (0)
#define GR_HIP(r, call) do { hipError_t _e = (call); if (_e != hipSuccess) { char _b[512]; \
    snprintf(_b, sizeof _b, "HIP call failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); (r)->err = _b; return 1; } } while (0)
#define GR_TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// host modular helpers of both translation units
static inline u64 hm_mul(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }
static inline u64 hm_pow(u64 a, u64 e, u64 q) { u64 r = 1 % q; a %= q; while (e) { if (e & 1) r = hm_mul(r, a, q); a = hm_mul(a, a, q); e >>= 1; } return r; }
static inline u64 hm_inv(u64 a, u64 q) { return hm_pow(a, q - 2, q); }
static inline u64 hm_shoup(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
static inline uint32_t hm_brev(uint32_t x, int bits) { uint32_t r = 0; for (int i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }

// gring.hip
int gr_upload(sfg_ring *r, void *dst, const void *src, size_t bytes);
int gr_reserve(sfg_ring *r, GrMem &buf, size_t bytes);             // grow-only: a buffer too small is let go (a wiping one wiped) and allocated anew
int gr_table(sfg_ring *r, GrMem &dst, const void *host, size_t bytes);   // a table allocated and filled; the caller moves it into the ring when it is complete
int gr_transform(sfg_ring *r, u64 *rows, size_t nrows, GrRowMap map, bool inv);
int gr_transform_cols_fwd(sfg_ring *r, u64 *rows, size_t nrows, GrRowMap map);   // the forward transform's first launch alone (the caller runs its own contiguous pass)
GrRowMap gr_map(int period, int split, int base0, int base1);
int gr_extend(sfg_ring *r, const GrExt &e, const u64 *src, u64 *Y, uint32_t *V, u64 *out, int ntgt, size_t npoly);
int gr_check_level(sfg_ring *r, const char *what, int nct, int level);
bool gr_overlap(const void *a, size_t na, const void *b, size_t nb);
u64 gr_galois(const sfg_ring *r, int k_left);
// workspace of one chunk of key switches: the regions of gr_ks_layout (gring_plan.hpp) in the ring's workspace
struct GrKsWs { u64 *c2, *Y, *ext, *accQ, *accP, *Y2, *ext2; uint32_t *V, *V2; GrJob *jobs; };
GrKsWs gr_ks_ws(void *ws, const GrKsLayout &l);
// lattigo switchKeysInPlace on J jobs whose c2 rows (NTT domain) are in w.c2 and whose job list is uploaded
int gr_keyswitch(sfg_ring *r, int level, size_t J, const GrKsWs &w, const u64 *add, int add_mask, u64 *out);
// a batch of key switches in the chunks of gr_ks_plan: per chunk the job list is uploaded, front(first job, jobs, workspace) launches what fills the chunk's c2
// rows (a job's ciphertext index is absolute, its workspace rows are the chunk's), and the key switch runs
template <class Front>
static int gr_ks_batch(sfg_ring *r, int level, const std::vector<GrJob> &jobs, const u64 *add, int add_mask, u64 *out, Front front) {
    const GrChunks plan = gr_ks_plan(jobs.size(), level, r->np, (size_t)r->N, r->ws_budget);
    GR_TRY(gr_reserve(r, r->ws, plan.bytes));
    const GrKsWs w = gr_ks_ws(r->ws.p, gr_ks_layout(level, r->np, (size_t)r->N, plan.chunk));
    for (size_t c = 0; c < plan.nchunks; c++) {
        const size_t j0 = plan.first(c), n = plan.count(c, jobs.size());
        GR_TRY(gr_upload(r, w.jobs, jobs.data() + j0, n * sizeof(GrJob)));
        front(j0, n, w);
        GR_TRY(gr_keyswitch(r, level, n, w, add, add_mask, out));
    }
    return 0;
}
int gr_rows_from_mont(sfg_ring *r, u64 *rows, size_t nrows);      // lattigo ring.InvMForm on key rows [.][nmod][N], enqueued on the ring's stream
// gring_io.hip
struct GriDecTab { const u64 *qmod, *winv, *half; };               // the decoder's tables of a level
int gri_dec_tab(sfg_ring *r, int level, GriDecTab *out);           // built at the level's first use, kept by the ring
int gri_add_c0(sfg_ring *r, const u64 *ct, const u64 *h, u64 *pt, int nb, int level);          // pt [nb][nl][N] = c0 + h, one launch
int gri_digits_inplace(sfg_ring *r, u64 *X, int nb, int level, const GriDecTab &tab);          // NTT-domain rows -> mixed-radix digits in place
int gri_take_indices(sfg_ring *r, const char *what, int nct, u64 *first);       // nct consecutive encryption indices from the ring's one counter; refuses an unseeded encryptor
// the encoder's device half, shared by gri_encode (host vectors) and the products' diagonals (gring_matmul.hip)
struct GriDdTab { const double4 *W, *Z; const uint32_t *slot_m, *slot_pos; };      // W [n/2] exp(-2 pi i k / n); Z [n] zeta^-c = exp(-pi i c / N); m_t; brev(m_t)
int gri_dd_tab(sfg_ring *r, GriDdTab *out);                        // built at first use, kept by the ring
// The products' list of the coefficients of one batch of diagonals that fell inside the band (32-bit words in device memory, kept by the ring): the count of the
// batch (reset by k_gr_mm_band; it may pass the capacity, entries past it were counted unproven), the coefficients re-derived since the flags were last read, then
// kCap pairs (vector of the batch, coefficient index < N).
struct GriTies { enum { kCount = 0, kResolved = 1, kEntries = 2, kCap = 512, kWords = kEntries + 2 * kCap }; };
// A [nb][n] (v_t at m_t, zero elsewhere) -> the transform, the rounding with the band test band[vec] and the residues modulo the first nl moduli, coefficient domain, in
// R [nb][nl][N].  flags[0] += unproven coefficients, flags[1] += coefficients outside |p| < 2^62: the caller zeroes and reads them.  ties (nullable): see GriTies; with
// it a coefficient inside the band goes to the list, not to flags[0].
int gri_encode_dft(sfg_ring *r, double4 *A, int nb, const GriDdTab &tab, const double *band_dev, unsigned *flags, unsigned *ties, u64 *R, int nl, double scale);
int gri_encode_refuse(sfg_ring *r, const char *what, const unsigned *f, double scale);           // the encoder's two refusals from the flags read back (0 = none)
