// reshard.hpp — one rank's share of sfg_mgpu_geno_filter (reshard.hip): its new column window, gathered from the old windows of the ranks that hold its columns.
#pragma once
#include "common.hpp"

constexpr int RESHARD_MAX_SEGS = 64;       // local ranks of an engine at most (mgpu_create_common)
// One old shard a new window draws on.  The filter is monotone, so segment j serves the output columns [out0[j], out0[j + 1]) of the window and only shards that
// serve at least one column are listed: out0 is strictly increasing and out0[0] = 0.
struct ReshardSeg {
    const uint8_t *base;                   // the old shard's first byte (on this device, on a peer, or on a device several ranks share)
    size_t ld;                             // its row stride in bytes
    unsigned gcol0;                        // the global column of its first stored column
    unsigned out0;                         // the first output column of this window it serves
};
struct ReshardSegs { ReshardSeg s[RESHARD_MAX_SEGS]; int n; };      // passed to the kernels by value, like PeerPtrs (mgpu.hip)

// cols_host [wcols]: the global source column of every output column of the window; rows_host [nr]: the kept rows.  Both are copied before the call returns.
// *out: a new owned handle of nr x wcols on ctx's device - int8 with a row stride of ceil(wcols / 16) * 16 bytes, or packed with ceil(wcols / 16) dwords a row -
// padding zero.  Synchronising.  The caller answers for the table: every column lies inside the shard of its segment.
int sfg_reshard_window(sfg_ctx *ctx, const ReshardSegs &segs, const unsigned *cols_host, size_t wcols, const unsigned *rows_host, size_t nr, bool packed, sfg_geno **out);
