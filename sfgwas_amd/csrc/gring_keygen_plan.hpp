// gring_keygen_plan.hpp - host-only planning of the general ring's key generation (gring_keygen.hip): how many keys one chunk of a share call holds, the chunks
// of a call and the bytes to reserve.  A share row is made in the caller's output buffer, so the only workspaces are the automorphism index tables of a chunk's
// keys (4 N bytes a key, with the key's inverse Galois element beside it) and, for the relinearisation rounds, the nmod rows of NTT(u).  The executors take
// every count and pointer from here.
// Standard library only and on its own (like gring_io_plan.hpp): tests/host/host_gring_keygen_test.cpp holds it on the CPU.
#pragma once
#include <cstddef>

constexpr size_t kGrkMaxKeys = 1024;                   // keys of one chunk at most
constexpr size_t kGrkLaunchRows = 32768;               // rows of one transform launch (gring_plan.hpp: kGrLaunchCap, asserted equal in gring_keygen.hip)
constexpr size_t kGrkGridLimit = 65536;                // every grid dimension of a chunk stays below it
constexpr size_t kGrkIndexBudget = 256ull << 20;       // bytes of index tables one chunk may hold

// keys of one chunk: the least of the cap, what keeps the chunk's beta * nmod rows a key within one transform launch and its grid dimensions (rows in grid.y,
// polynomials in grid.z) below 65536, and what the index-table budget holds; at least 1
inline size_t grk_keys_per_chunk(int beta, int nmod, size_t N, size_t index_budget) {
    const size_t rows = (size_t)beta * nmod;
    size_t k = kGrkMaxKeys;
    const size_t by_launch = kGrkLaunchRows / rows, by_grid = (kGrkGridLimit - 1) / rows, by_budget = index_budget / (4 * N);
    if (by_launch < k) k = by_launch;
    if (by_grid < k) k = by_grid;
    if (by_budget < k) k = by_budget;
    return k < 1 ? 1 : k;
}
struct GrkPlan {
    size_t chunk = 0, nchunks = 0;
    size_t index_bytes = 0;                            // to reserve: chunk tables of N 32-bit entries, then chunk 64-bit inverse Galois elements
    size_t galois_at = 0;                              // byte offset of those elements in the index workspace
    size_t u_bytes = 0;                                // to reserve in the wiping workspace: NTT(u) at all nmod moduli (the relinearisation rounds; else 0)
    size_t first(size_t c) const { return c * chunk; }
    size_t count(size_t c, size_t n) const { const size_t left = n - c * chunk; return left < chunk ? left : chunk; }
};
// nkeys keys with an index table each (the rotation keys); with_u: the call also holds NTT(u)
inline GrkPlan grk_plan(size_t nkeys, int beta, int nmod, size_t N, bool with_u, size_t index_budget = kGrkIndexBudget) {
    GrkPlan p;
    p.u_bytes = with_u ? (size_t)nmod * N * 8 : 0;
    if (nkeys == 0) return p;
    const size_t k = grk_keys_per_chunk(beta, nmod, N, index_budget);
    p.chunk = nkeys < k ? nkeys : k;
    p.nchunks = (nkeys + p.chunk - 1) / p.chunk;
    p.galois_at = p.chunk * 4 * N;
    p.index_bytes = p.galois_at + p.chunk * 8;
    return p;
}
