// ab/mgpu_solo.hip — the solo-rank timing mode of the multi-GPU engine (A/B build only, make ab).
#include "../common.hpp"

// SFG_MGPU_SOLO=r/w: this process computes the share of rank r of a w-rank world on one GPU, every exchange replaced by a local copy of the rank's own slice (the
// outputs are not a product): per-rank phase times of world sizes a one-GPU box cannot run (bench.py).  Unset: nothing changes.  Returns an error message or nullptr.
const char *ab_mgpu_solo(int n_local, bool multi_process, bool &solo, int &world, int &rank0) {
    const char *e = getenv("SFG_MGPU_SOLO");
    if (!e) return nullptr;
    int r = 0, w = 0;
    if (sscanf(e, "%d/%d", &r, &w) != 2 || w < 1 || r < 0 || r >= w || n_local != 1 || multi_process) return "SFG_MGPU_SOLO=r/w needs one local device and a single process";
    solo = true; world = w; rank0 = r;
    return nullptr;
}
