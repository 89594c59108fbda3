// ab/config.hip — the A/B build's experiment switches (make ab, -DSFG_AB).  Defaults = the measured configuration; results are identical words.
#include "../common.hpp"

void ab_read_config(SfgConfig &c) {
    auto env = [](const char *n) { return getenv(n); };
    if (const char *e = env("SFG_MAC_IMPL")) { c.mac_reg = !strcmp(e, "reg"); c.mac_bc = strcmp(e, "dma") != 0 && !c.mac_reg; c.mac_i8 = !strcmp(e, "i8"); }      // bc | dma | reg | i8
    if (const char *e = env("SFG_MAC_I8_BIG")) c.mac_i8_big = atoi(e) != 0;
    if (const char *e = env("SFG_MAC_I8_ROT")) { c.mac_i8_nolds = strcmp(e, "lds") != 0; c.mac_i8_ring = !strcmp(e, "ring"); }      // ring (default) | cache | lds
    if (env("SFG_MAC_I8_WG")) c.mac_i8_ring = false;
    if (const char *e = env("SFG_MAC_I8_WAVES")) c.mac_i8_waves = atoi(e) == 6 ? 6 : 12;
    if (const char *e = env("SFG_MAC_I8_WG")) c.mac_i8_wg1 = atoi(e) == 1;
    if (const char *e = env("SFG_MAC_WC")) c.mac_wc = atoi(e) == 2 ? 2 : 1;
    if (const char *e = env("SFG_MM_OVERLAP")) c.no_overlap = atoi(e) == 0;
    if (env("SFG_MM_NO_OVERLAP")) c.no_overlap = true;
    if (const char *e = env("SFG_NTT_HALF_IMPL")) c.ntt_half_full = !strcmp(e, "full");
    if (const char *e = env("SFG_NTT_FWD_IMPL")) c.ntt_fwd_full = !strcmp(e, "full");
    if (const char *e = env("SFG_MAC_PT")) c.mac_plain_pt = !strcmp(e, "plain");
    if (const char *e = env("SFG_PT_RIDE")) { c.pt_ride = atoi(e); if (c.pt_ride < 0) c.pt_ride = 0; c.pt_ride = c.pt_ride / 8 * 8; }
    if (const char *e = env("SFG_PT_COMPACT")) c.pt_compact = atoi(e) != 0;
    if (const char *e = env("SFG_PT_KMAJOR")) c.pt_kmajor = atoi(e) != 0;
    if (const char *e = env("SFG_PT_RIDE_DEPTH")) { c.i8_mover_depth_ride = atoi(e); if (c.i8_mover_depth_ride < 1 || c.i8_mover_depth_ride > 3) c.i8_mover_depth_ride = 1; }
    if (const char *e = env("SFG_PT_RIDE_NT")) c.i8_mover_nt_ride = atoi(e) != 0;
    if (env("SFG_ASSOC_TRACE")) c.assoc_trace = true;
}
int ab_set_attrs(sfg_ctx *ctx) { return ab_mac_dma_set_attrs(ctx) || ab_ntt_set_attrs(ctx); }
