// ab/ab.hpp — entry points of the A/B build's sources (csrc/ab/*.hip, make ab): the superseded kernels that tests hold the product's words against, and the
// switches that select them.  Included by common.hpp under SFG_AB only; each product call site is one guarded line.
#pragma once
struct MacStrides; struct PanelMap; struct I8Args;
void ab_read_config(SfgConfig &c);                                              // config.hip: the switches of SfgConfig's A/B block
const char *ab_mgpu_solo(int n_local, bool multi_process, bool &solo, int &world, int &rank0);    // mgpu_solo.hip: SFG_MGPU_SOLO=r/w (error message or nullptr)
int ab_set_attrs(sfg_ctx *ctx);                                                // config.hip: the dynamic-LDS limits of the A/B kernels (context creation)
int ab_mac_dma_set_attrs(sfg_ctx *ctx);                                        // mac_dma_tiles.hip: the round-1 LDS-DMA MAC, SFG_MAC_IMPL=dma
int ab_launch_mac_dma_tiles(sfg_ctx *ctx, const double *rotf, size_t rows_per_k, const u64 *pt, u64 *out, int K, int R, int Ncols, int L, int accumulate, const MacStrides &st);
int ab_ntt_set_attrs(sfg_ctx *ctx);                                            // ntt_full.hip: the full-image plaintext NTT, SFG_NTT_HALF_IMPL=full
int ab_launch_ntt_half_full(sfg_ctx *ctx, const double *pc, u64 *out_half, size_t nplain, int L, const PanelMap &pm);
int launch_mac(sfg_ctx *ctx, const u64 *rot, const u64 *pt, u64 *out, int K, int R, int Ncols, int L, int accumulate);     // mac_reg.hip: SFG_MAC_IMPL=reg
int launch_mac_strided(sfg_ctx *ctx, const u64 *rot, const u64 *pt, u64 *out, int K, int R, int Ncols, int L, int accumulate, const MacStrides &st);
void ab_launch_mac_i8_lds(hipStream_t q, const I8Args &a, const ModConst *modc, int nl);          // mac_i8_lds.hip: SFG_MAC_I8_ROT=lds
