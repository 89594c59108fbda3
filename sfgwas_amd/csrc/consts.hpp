// consts.hpp — the constants the host-only planner (mm_plan.hpp) shares with the device code (common.hpp).  Standard library only.
#pragma once
#include <cstddef>

constexpr int SFG_LOGN = 14;
constexpr int SFG_N = 1 << SFG_LOGN;      // ring degree (PN14QP438, gwas.go:169)
constexpr int SFG_SLOTS = SFG_N / 2;
constexpr int SFG_D = 91;                 // ceil(sqrt(8192)), matmult.go:1047
constexpr int SFG_MAXMOD = 16;
// HBM that must stay free beside the transposed copies of ALL groups of a caller's rotation cache (association scan) for the int8 MAC to take that call
constexpr size_t SFG_I8_KEEP_RESERVE = 80ULL << 30;
// the largest fp64 rotation cache a product of several accumulator passes builds for itself (mm_range_plan)
constexpr size_t SFG_MM_WHOLE_CACHE_CAP = 48ULL << 30;

// The flag word of a plaintext panel (PanelMap::packed_mask, the last argument of launch_encode_rows).  Bit l < 16: the rows of modulus l are written as
// packed-limb words (mac_dma.hip).  The named bits:
constexpr unsigned PT_DIGITS = 1u << 31;       // the packed rows leave as five digit planes instead (int8 MAC, mac_i8.hip)
constexpr unsigned PT_DIGITS_BIG = 1u << 30;   // the 46-bit modulus too (six planes)
constexpr unsigned PT_COMPACT = 1u << 29;      // compact rows: every modulus in planes, a plaintext's planes back to back
// (with PT_COMPACT) K-MAJOR panel - [column][plane][128-byte coefficient block][k < K][128 B]: the k rows of a column's coefficient block are adjacent, so a transposition
// unit reads 16 runs of 2 KiB instead of 256 runs of 128 B (PanelMap::K = rows per column; G == 0: plaintext p of the launch is column p / K, row p % K)
constexpr unsigned PT_KMAJOR = 1u << 28;
