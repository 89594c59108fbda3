// kernels.hpp — internal launch interface between the translation units of libsfgwas_hip.
#pragma once
#include "common.hpp"
#include "mm_plan.hpp"            // the product's launch plan; the byte models mac_i8_stream_bytes / mac_i8_tile_bytes / mac_i8_rot_tile_bytes
#include "assoc_plan.hpp"         // the association scan's batch plan, filter maps, diag_bool, the active-baby tables
#include "batch_plan.hpp"         // the one chunk rule and the per-family figures of the fixed-ring protocol ends

// row r of a batch uses modulus m[r % period] (ciphertext rows, plaintext rows, key-switch rows are all periodic)
// m < 0 marks a row the kernel must leave untouched
constexpr int SFG_MAXPATTERN = 128;   // >= KSW_MAXDIG * SFG_MAXMOD
struct ModPattern { int period; int8_t m[SFG_MAXPATTERN]; };
// the pattern of `count` consecutive moduli from `first`: row r uses modulus first + r % count
inline ModPattern mod_pattern_run(int first, int count) { ModPattern p; p.period = count; for (int j = 0; j < count; j++) p.m[j] = (int8_t)(first + j); return p; }
// row r of a launch lives at base + (r / rpg) * gstride + (r % rpg) * N  (strides in words)
struct RowMap { int rpg; size_t gstride_in, gstride_out; };
// where the plaintext of diagonal `shift` (= shift0 + index in the batch) of block row g lands inside a panel that holds G
// block rows: slot ((shift / 91) * G + g) * 91 + shift % 91, i.e. [giant][g][baby] so that k = g*91 + baby is contiguous.
// G == 0: dense (slot = index in the batch)
struct PanelMap { int G, g, shift0; unsigned packed_mask = 0; int K = 0; };   // packed_mask: the panel's flag word - bit l: rows of modulus l are written as packed-limb words (mac_dma.hip); PT_DIGITS, PT_DIGITS_BIG, PT_COMPACT, PT_KMAJOR (consts.hpp); K: rows per column of a K-major panel

// ntt.hip
int launch_ntt_fwd(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, const ModPattern &pat);
int launch_ntt_inv(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, const ModPattern &pat);
int launch_ntt_plain(sfg_ctx *ctx, const double *pc, u64 *out, size_t nplain, int L);
struct MoveJob;                                   // i8_move.hpp: mover workgroups of the previous MAC launch's plaintext transposition riding in front of the NTT's
// The riding transposition (round 6): the plaintext panel of MAC launch k - 1 goes into the int8 MAC's tiles INSIDE the plaintext-NTT launches of launch k's encode
// (k_ntt_half3_move: `nblocks` mover workgroups first in every grid, one to a CU beside three NTT workgroups).  matmul.hip fills one per delayed MAC launch;
// launch_encode_rows deals its items out evenly over the NTT launches it makes and i8_ride_finish moves whatever is left.
struct PtRide;
int launch_ntt_plain_half(sfg_ctx *ctx, const double *pc, u64 *out_half, size_t nplain, int L, PanelMap pm, const uint32_t *perm = nullptr, const MoveJob *mv = nullptr);
int launch_expand_half(sfg_ctx *ctx, const u64 *half, u64 *full, size_t nrows);
int launch_ntt_fwd_map(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, const ModPattern &pat, const RowMap &rm);
int launch_ntt_inv_map(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, const ModPattern &pat, const RowMap &rm);
// dense forward NTT, out of place; staged: the rows arrive through the transform's first stage (fp64mod.hpp fwd_stage1_pair), each half-row workgroup reads only its half
int launch_ntt_fwd_staged(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, const ModPattern &pat, bool staged);
// inverse NTT WITHOUT its last stage and without 1/N, as two half-row workgroups per row; in place or not.  The reader of the rows finishes them (fp64mod.hpp inv_last_pair)
int launch_ntt_inv_split(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, const ModPattern &pat, const RowMap &rm);
// the MAC launches
struct MacStrides { size_t rot_k, rot_r, pt_k, pt_n, out_n, out_r; bool pt_half = false; bool pt_packed = false; bool pt_digits = false; bool i8 = false; bool i8_big = false; bool pt_digits_big = false;
                    const int8_t *B_small = nullptr, *B_big = nullptr;
                    int pt_layout = 0, pt_L = 0;  // 1: digit-plane panel rows packed - a plaintext is its pt_L moduli's 5 / 6 planes of N/2 bytes back to back (208 KiB at PN14QP438, L = 5) instead of L rows of N/2 words (320 KiB), PanelMap bit 29; 2: K-major, bits 29 + 28 (mac_i8.hip i8_panel_rows)
                    int B_mode = 0;       // B_* given (the riding transposition's tile buffers) and B_mode 1: already transposed (riding mover): no pass; 2: the pass runs into these buffers
                    const int8_t *A_small = nullptr, *A_big = nullptr; };   // A_*: the transposed rot tiles of this launch are given (I8RotPre): no copy to look up or make   // i8: small moduli on the int8 MAC (mac_i8.hip); pt_digits: their panel rows hold five digit planes   // in words; pt_half: pt rows hold N/2 words (mirror-symmetric plaintexts)
int launch_mac_i8_small(sfg_ctx *ctx, const double *rotf, size_t rotf_k_stride, size_t rotf_r_stride, int plane0, const u64 *pt, u64 *out, int K, int R, int r0, int Ncols,
                        int l0, int nl, int accumulate, const MacStrides &st);       // mac_i8.hip
int launch_mac_i8_big(sfg_ctx *ctx, const double *rotf, size_t rotf_k_stride, size_t rotf_r_stride, int plane0, const u64 *pt, u64 *out, int K, int R, int r0, int Ncols,
                      int l0, int accumulate, const MacStrides &st);
// encode.hip
int launch_skew(sfg_ctx *ctx, const int8_t *blk, size_t ld, int r, int c, int transposed, int square, int8_t *D);
// pcache (nullable): the block's slot of the plaintext coefficient cache, [8192 shifts][N/2] doubles.  mode 1: the FFT writes its rows there (and the NTT reads them);
// 2: the rows are there already (no FFT; D unused); 3: they are there in the block's other orientation (no FFT; NTT through the permutation table)
struct PcCache { double *slot = nullptr; int mode = 0; const uint32_t *perm = nullptr; };
int launch_encode_rows(sfg_ctx *ctx, const int8_t *D, int shift0, int nshift, int L, u64 *pt, bool half_rows = false, int G = 0, int g = 0, unsigned packed_mask = 0, const PcCache *pcache = nullptr,
                       PtRide *ride = nullptr);
int encode_rows_launches(const sfg_ctx *ctx, int nshift);          // NTT launches launch_encode_rows makes for nshift diagonals (panel form)
// mac_i8.hip: the riding transposition of one delayed MAC launch (panel of K = ng * 91 k-rows x 91 columns -> tile buffers mi8.Bs / mi8.Bb); ride.on stays false where the
// moduli are not one run of 35-bit ones plus at most one 46-bit one
int i8_ride_prepare(sfg_ctx *ctx, const u64 *panel, int K, int Ncols, size_t pt_k, size_t pt_n, int layout, int L, int launches, PtRide &ride);
int i8_ride_finish(sfg_ctx *ctx, PtRide &ride);                     // items no NTT launch took: a launch of mover workgroups alone on the current stream
int i8_ride_tiles(sfg_ctx *ctx, int K, int L, int8_t **Bs, int8_t **Bb);          // the two tile buffers (a launch that transposes by the pass uses them as well: B_mode 2)
struct I8Args;                                                      // i8_move.hpp
void launch_i8_pack_pt_digits(hipStream_t q, const I8Args &a, unsigned items, bool big);      // the transposition pass of digit-plane panel rows
void launch_move_alone(hipStream_t q, const MoveJob &j);           // the same by mover workgroups alone on queue q
// refresh.hip: h = rows + sk (.) xr (negated if neg) and out = a + b over [nct][nl][N] rows taken from strided sources (the loaded secret-key shard)
int launch_share(sfg_ctx *ctx, const u64 *rows, size_t rows_ct_stride, const u64 *xr, size_t x_ct_stride, u64 *h, int nl, int nct, int neg = 0);
int launch_add_rows(sfg_ctx *ctx, const u64 *a, size_t a_ct_stride, const u64 *b, size_t b_ct_stride, u64 *out, size_t out_ct_stride, int nl, int nct);
// decrypt.hip: the decryption front end - x [nb][nl][N] = the coefficient rows of plaintexts first .. first + nb - 1 of the source: NTT rows `stride` words apart,
// c0 + h0agg, or c0 + sk (.) c1 of ciphertexts [..][2][nl][N].  *launches (nullable) grows by the launches made beyond the inverse NTT
struct DecSrc {
    enum Kind { ROWS, FINISH, DECRYPT } kind; const u64 *src; size_t stride; const u64 *h0agg;
    static DecSrc rows(const u64 *pt, size_t stride) { return DecSrc{ROWS, pt, stride, nullptr}; }
    static DecSrc finish(const u64 *ct, const u64 *h0agg) { return DecSrc{FINISH, ct, 0, h0agg}; }
    static DecSrc decrypt(const u64 *ct) { return DecSrc{DECRYPT, ct, 0, nullptr}; }
};
int launch_dec_front(sfg_ctx *ctx, const DecSrc &s, int first, int nb, int nl, u64 *x, int *launches = nullptr);
// decrypt.hip: the level and the count of a protocol entry point.  what: the caller's prefix; maxl: the module's modulus cap at the input level (RF_MAXL; 0: none);
// min_count: 0, or 1 where an empty call is refused
int check_level_count(sfg_ctx *ctx, const char *what, int nct, int level, int maxl, int min_count = 0);
// encrypt.hip: the deterministic encryption core for the zero public key: out [nct][2][level+1][N] = (ModDown_P(NTT_QP(e0)), ModDown_P(NTT_QP(e1)))
int encrypt_errors_moddown(sfg_ctx *ctx, const int32_t *e0, const int32_t *e1, int nct, int level, u64 *out);
// genoio.hip: dense int8 copy [nr][ld_out] of the stored sub-block (r0.., c0..) of a 2-bit packed matrix (c0 a multiple of 4)
int launch_geno_unpack(sfg_ctx *ctx, const sfg_geno *g, size_t r0, size_t c0, size_t nr, size_t nc, int8_t *out, size_t ld_out);
// rotate.hip
int launch_rotate_right(sfg_ctx *ctx, const u64 *in, u64 *out, int nct, int level, const int *nrot_host);
int launch_rotate_right_indexed(sfg_ctx *ctx, const u64 *in, int nin, u64 *out, int nct, int level, const int *nrot_host, const int *in_index);
int launch_rotate_right_indexed_f64(sfg_ctx *ctx, const u64 *in, int nin, double *outf, int nct, int level, const int *nrot_host, const int *in_index, int L,
                                    const size_t *out_slot = nullptr);
int launch_rotate_right_sum(sfg_ctx *ctx, const u64 *in, int nin, int nct, int level, const int *nrot_host, const int *in_index, const int *group, int nout,
                            u64 *out, size_t out_stride, int accumulate);
int launch_relinearize(sfg_ctx *ctx, const u64 *tmp, int nct, int level, const u64 *mid, u64 *out);
int launch_ct_add(sfg_ctx *ctx, const u64 *a, const u64 *b, u64 *out, size_t nct, int level);
// mac_dma.hip
int mac_dma_planes(sfg_ctx *ctx, int L, std::vector<int> &plane_of, std::vector<int> &is_big);
double mac_big_maxterm(u64 q);
int launch_rot_to_f64(sfg_ctx *ctx, const u64 *rot, size_t nrows, int nl_rot, int L, double *rotf);
int launch_mac_dma(sfg_ctx *ctx, const double *rotf, size_t rows_per_k, const u64 *pt, u64 *out, int K, int R, int Ncols, int L, int accumulate, const MacStrides &st);
int launch_pack_pt(sfg_ctx *ctx, const u64 *in, u64 *out, size_t nrows, size_t words_per_row, int L, unsigned packed_mask);
unsigned mac_dma_packed_mask(sfg_ctx *ctx, int L);
bool mac_use_dma(const sfg_ctx *ctx);
// mac_bc.hip (same contract as launch_mac_dma; small-modulus plaintext rows packed)
int launch_mac_bc(sfg_ctx *ctx, const double *rotf, size_t rows_per_k, const u64 *pt, u64 *out, int K, int R, int Ncols, int L, int accumulate, const MacStrides &st);
// matmul.hip: the baby-step rotation cache of block rows [b0, b1) in the MAC layout; tabs = per-row active-baby flags (null: all 91)
int rotcache_build_rows_tab(sfg_ctx *ctx, const u64 *A, int s, int in_level, int max_level, int nbr, int b0, int b1, const std::vector<std::vector<uint8_t>> *tabs, double *cache);
// stream.hip: the call-wide rotation cache of an association scan (nullptr in *out = not applicable; caller hipFree()s)
int assoc_build_rotcache(sfg_ctx *ctx, const u64 *A_dev, int s, int in_level, int max_level, size_t nr, const std::vector<size_t> &widths, double **out);
// A caller's baby-step rotation cache held ONLY as the int8 MAC's transposed rot tiles (round 4): one pair of buffers (35-bit moduli / 46-bit modulus) per MAC group of
// G block rows.  The association scan multiplies one block column per batch against the cache of all its block rows: the fp64 operand form (1.86 GB per block row at
// s = 13, 115 GB at 500 000 samples) is then only the source of the tiles - built group by group in a scratch buffer and dropped - and the scan's MAC runs on the matrix core.
struct I8RotPre { int G = 0, nbr = 0, s = 0, L = 0; std::vector<int8_t *> As, Ab; };
int i8_rotpre_build(sfg_ctx *ctx, const u64 *A_dev, int s, int in_level, int max_level, int nbr, const std::vector<std::vector<uint8_t>> *tabs, size_t budget_bytes, const char *prefix, I8RotPre &pre);   // pre.G == 0 afterwards: not taken (fp64 path)
void i8_rotpre_free(I8RotPre &pre);
struct I8RotPreScope { I8RotPre pre; ~I8RotPreScope() { i8_rotpre_free(pre); } };
// The rotation operand of a product: where the baby-step rotations of the operand's block rows come from (mm_plan.hpp RotSrc).  A view: the holder keeps the
// ciphertexts, the cache rows or the tiles alive.
struct RotOperand {
    RotSrc src = RotSrc::own;
    const u64 *A = nullptr;               // own: the ciphertexts [s][nbr][2][in_level + 1][N], key-switched by the call group by group
    int in_level = -1;                    // own: their level.  A cache: the level its source ciphertexts had (sizes the call's operand scratch), -1: the product's max_level
    const double *rows = nullptr;         // f64_cache: cache[block row - b0][baby < 91][i < s][poly < 2][rowf] (+ 3 zero k-slices) of exactly the block rows the call contracts over
    const I8RotPre *tiles = nullptr;      // i8_tiles: of ALL operand block rows of the (possibly transposed) matrix
    static RotOperand own(const u64 *A, int in_level) { RotOperand r; r.A = A; r.in_level = in_level; return r; }
    static RotOperand f64_cache(const double *rows, int in_level = -1) { RotOperand r; r.src = RotSrc::f64_cache; r.rows = rows; r.in_level = in_level; return r; }
    static RotOperand i8_tiles(const I8RotPre *pre) { RotOperand r; r.src = RotSrc::i8_tiles; r.tiles = pre; return r; }
    int level_in(int max_level) const { return in_level < 0 ? max_level : in_level; }
    int validate(sfg_ctx *ctx, int s, int L, int nbr, int b0, int b1) const;    // matmul.hip: can it multiply block rows [b0, b1) of nbr at s rows and L moduli on this context?
};
// matmul.hip: a product call but for its rotation operand.  Accumulate phase: operand block rows [b0, b1) x block columns [j0, j1) into
// acc [(j - j0)][giant < 91][i < s][2][L][N] (zero-initialised unless accumulate != 0); acc_col_words: words between consecutive block columns' accumulators
// (0: dense, 91 giants).  Whole product: SNP blocks [blk0, blk1) of the STORED matrix - output columns for X, contraction rows for X^T - into out
struct MmArgs { const sfg_geno *g; unsigned flags; int s, max_level, b0, b1, j0, j1, accumulate; uint64_t *acc; size_t acc_col_words; };
struct MmRangeArgs { const sfg_geno *g; unsigned flags; int s, max_level, blk0, blk1; uint64_t *out; };
int matmul_accumulate(sfg_ctx *ctx, const RotOperand &rot, const MmArgs &a);
int matmul_resident_range(sfg_ctx *ctx, const RotOperand &rot, const MmRangeArgs &a);
int launch_i8_pack_rot_to(sfg_ctx *ctx, const double *rotf, size_t rotf_k_stride, size_t rotf_r_stride, int plane0, int K, int R, int l0, int nl, bool big, int8_t *A_out);      // mac_i8.hip
// the rotation cache of an association scan in whichever form the context multiplies with: the operand every batch multiplies and, where that is int8 tiles, their
// storage (op then points at pre: not to be copied once built; fp64 rows are the context's scratch entry "assoc.rotf")
struct AssocRot { RotOperand op; I8RotPre pre; };
int assoc_build_rot(sfg_ctx *ctx, const u64 *A_dev, int s, int in_level, int max_level, size_t nr, const std::vector<size_t> &widths, AssocRot &out);
void assoc_free_rot(AssocRot &r);
struct AssocRotScope { AssocRot r; ~AssocRotScope() { assoc_free_rot(r); } };
int assoc_product(sfg_ctx *ctx, const AssocRot &r, int s, int max_level, const sfg_geno *g, unsigned flags, int nct, uint64_t *out);
int assoc_batch_tail(sfg_ctx *ctx, const u64 *tmp, const sfg_geno *g, int s, size_t nct, size_t ctw, uint64_t *out_dev, size_t out_ct_capacity, size_t out_shift,
                     double *sum_host, double *sqsum_host);      // stream.hip: rows of tmp copied into place, padded sums zeroed, column sums

// genoio.hip: decode + filter + transpose of a packed SNP range in HBM on queue st; a byte filter as a device map (NULL filter: no map, *kept = n)
int launch_bed_decode(sfg_ctx *ctx, hipStream_t st, const uint8_t *dbed, size_t bps, size_t num_sample, size_t num_snp, const int32_t *rmap, const int32_t *cmap,
                      int8_t *out, size_t ld);
int launch_bed_decode_lut(sfg_ctx *ctx, hipStream_t st, const uint8_t *dbed, size_t bps, size_t num_sample, size_t num_snp, const int32_t *rmap, const int32_t *cmap,
                          int8_t *out, size_t ld, unsigned lut);
int upload_filter_map(sfg_ctx *ctx, const uint8_t *filt, size_t n, DevMem &map, size_t *kept);

// stream.hip: the streamed association scan restricted to the batches k % nparts == part (fmt 0 = .bed, 1 = .pgen); see its definition
int assoc_stream_part(sfg_ctx *ctx, int fmt, const char *path, size_t num_sample, size_t num_snp, const uint8_t *row_filter, const uint8_t *col_filter,
                      size_t batch_snps, const uint64_t *A_dev, int s, int in_level, int max_level, unsigned flags,
                      uint64_t *out_dev, size_t out_ct_capacity, size_t *out_ct, double *sum_host, double *sqsum_host,
                      int part, int nparts, std::vector<std::pair<size_t, size_t>> *ranges);
