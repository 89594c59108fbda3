// ksw_plan.hpp — the host arithmetic of the key switch's job batching (rotate.hip launch_keyswitch_jobs) as pure functions: which jobs of a chunk share one read of
// their switching key (tiles), and which jobs of a chunk add into which output of a summed finish (segments).  Standard library only, so that all of it runs on a CPU (tests/host/host_ksw_plan_test.cpp).
#pragma once
#include <cstddef>
#include <vector>

// tile = `count` <= T consecutive items starting at `start`, all with the same key and the same automorphism table: a thread loads a key word once for all of them.
// Chunk-local job numbers (k_ksw_inner_p, k_ksw_finish).
struct KswTile { int start, count; };

// Jobs 0 .. nb of a chunk, job k with key key[k] and table tab[k]: the maximal runs of consecutive jobs with equal key AND equal table, each cut into pieces of at
// most T.  Any job list is covered exactly once and in order; a list without repeats gets nb tiles of one job.
template <class K, class I>
inline void ksw_job_tiles(const K *key, const I *tab, int nb, int T, std::vector<KswTile> &tiles) {
    tiles.clear();
    if (T < 1) T = 1;
    for (int k = 0; k < nb;) {
        int n = 1;
        while (k + n < nb && n < T && key[k + n] == key[k] && tab[k + n] == tab[k]) n++;
        tiles.push_back(KswTile{k, n});
        k += n;
    }
}

// A summed finish (KswSum): job k of the chunk adds into output group[k] < nout.  One segment per output that has a job in this chunk, in output order; the jobs of
// segment i are segjobs[start .. start + count) in chunk order.  `first`: no earlier chunk has written the output (the segment then takes the plain member and obeys
// the caller's accumulate flag; a later one adds to what is there).  nb == 0 is the closing call: a segment without jobs for every output that no chunk has touched.
// seen[] (nout flags, all 0 before the first chunk) carries that knowledge from call to call.
struct KswSegPlan { int out, start, count, first; };
inline void ksw_plan_segments(const int *group, int nb, int nout, std::vector<char> &seen, std::vector<KswSegPlan> &segs, std::vector<int> &segjobs) {
    std::vector<int> cnt((size_t)nout, 0), at((size_t)nout, 0);
    for (int k = 0; k < nb; k++) cnt[(size_t)group[k]]++;
    segs.clear(); segjobs.assign((size_t)nb, 0);
    for (int i = 0, start = 0; i < nout; i++) {
        if (nb ? !cnt[(size_t)i] : (bool)seen[(size_t)i]) continue;
        segs.push_back(KswSegPlan{i, start, cnt[(size_t)i], seen[(size_t)i] ? 0 : 1});
        at[(size_t)i] = start; start += cnt[(size_t)i]; seen[(size_t)i] = 1;
    }
    for (int k = 0; k < nb; k++) segjobs[(size_t)at[(size_t)group[k]]++] = k;
}
