// ksw_plan.hpp — the host arithmetic of the key switch's job batching (rotate.hip launch_keyswitch_jobs) as pure functions: how many inputs share a decomposition
// and how many jobs a chunk, from the scratch budget, and where the thirteen regions of the workspace lie (ksw_plan_sizes); which jobs belong to which input group,
// chunk and tile (ksw_plan_groups); which jobs of a chunk share one read of their switching key (tiles, ksw_job_tiles), and which jobs of a chunk add into which
// output of a summed finish (segments, ksw_plan_segments).  Standard library only, so that all of it runs on a CPU (tests/host/host_ksw_plan_test.cpp).
#pragma once
#include <cstddef>
#include <utility>
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

// ---- sizes and workspace layout
// Six row regions of N words each row, then seven small tables.  Offsets from the workspace's start: the row regions in u64 WORDS, the tables in BYTES.
//   c2 [in_grp][nl]  ext [ext_rows]  acc [acc_rows]  ext2 [ext2_rows]  extT [ext_rows]  ext2T [ext2_rows]       (extT / ext2T: the forward transforms run out of place)
//   keys, idx, out: a pointer per job of the batch; segs: a KswSeg per output of a sum; inidx, segjobs: an int per job; tiles: a KswTile per job (a tile holds >= 1 job)
constexpr size_t KSW_PTR_BYTES = 8, KSW_SEG_BYTES = 32, KSW_TABLE_SPARE = 256;
struct KswLayout { size_t c2, ext, acc, ext2, extT, ext2T, keys, idx, out, segs, inidx, segjobs, tiles, bytes; };
struct KswSizes { int in_grp, chunk; size_t ext_rows, ext2_rows, acc_rows; KswLayout at; };

// Level shape (nl moduli, np special primes, nt = nl + np targets, beta digits), nin inputs, nr jobs, nout outputs of a sum (0: none), `budget` bytes of decomposition
// resp. accumulator scratch, N words per row.  Inputs are processed in groups of in_grp whose decomposition fits the budget, the jobs of a group in chunks of `chunk`
// whose acc / ext2 rows fit it; each at least 1 and then at most nin resp. nr (so no input gives in_grp 0 and no job chunk 0: a sum that only closes its outputs).
inline KswSizes ksw_plan_sizes(int nl, int np, int nt, int beta, int nin, int nr, int nout, size_t budget, size_t N) {
    // acc holds the 2 np special-prime rows of a job only; the chunk is still cut as when it held all 2 nt rows: the job list is cut where it was
    const size_t in_rows = (size_t)nl + (size_t)beta * nt, job_rows = 2 * (size_t)nt + 2 * (size_t)nl;
    auto fit = [&](size_t rows, int most) { size_t n = budget / (rows * N * 8); if (n < 1) n = 1; if (n > (size_t)most) n = (size_t)most; return (int)n; };
    KswSizes s;
    s.in_grp = fit(in_rows, nin); s.chunk = fit(job_rows, nr);
    s.ext_rows = (size_t)s.in_grp * beta * nt; s.ext2_rows = (size_t)s.chunk * 2 * nl; s.acc_rows = (size_t)s.chunk * 2 * np;
    KswLayout &a = s.at;
    a.c2 = 0; a.ext = a.c2 + (size_t)s.in_grp * nl * N; a.acc = a.ext + s.ext_rows * N; a.ext2 = a.acc + s.acc_rows * N;
    a.extT = a.ext2 + s.ext2_rows * N; a.ext2T = a.extT + s.ext_rows * N;
    a.keys = (a.ext2T + s.ext2_rows * N) * 8; a.idx = a.keys + (size_t)nr * KSW_PTR_BYTES; a.out = a.idx + (size_t)nr * KSW_PTR_BYTES;
    a.segs = a.out + (size_t)nr * KSW_PTR_BYTES; a.inidx = a.segs + (size_t)nout * KSW_SEG_BYTES; a.segjobs = a.inidx + (size_t)nr * sizeof(int);
    a.tiles = a.segjobs + (size_t)nr * sizeof(int);
    a.bytes = a.tiles + (size_t)nr * sizeof(KswTile) + KSW_TABLE_SPARE;
    return s;
}

// ---- jobs -> input groups, chunks, tiles
// Job k of the batch reads input job_in[k] < nin with key key[k] and table tab[k].  One KswGroup per run of in_grp inputs [i0, i0 + ni) that has a job, in input
// order: its jobs (batch numbers) in list order - a job's GROUP-LOCAL number, its place in `jobs`, indexes the pointer tables - cut into chunks of at most `chunk`,
// chunk c = group-local jobs [c0, c0 + nb) with the tiles tiles[tile0 .. tile0 + ntiles) of CHUNK-LOCAL job numbers (ksw_job_tiles per chunk: no tile crosses a chunk).
// A group has at most as many tiles as jobs, which is the room the layout gives them.
struct KswChunk { int c0, nb, tile0, ntiles; };
struct KswGroup { int i0, ni; std::vector<int> jobs; std::vector<KswChunk> chunks; std::vector<KswTile> tiles; };
template <class K, class I>
inline void ksw_plan_groups(const int *job_in, const K *key, const I *tab, int nr, int nin, int in_grp, int chunk, int T, std::vector<KswGroup> &groups) {
    groups.clear();
    if (in_grp < 1 || chunk < 1) return;
    std::vector<K> gk; std::vector<I> gt; std::vector<KswTile> tl;
    for (int i0 = 0; i0 < nin; i0 += in_grp) {
        KswGroup g; g.i0 = i0; g.ni = nin - i0 < in_grp ? nin - i0 : in_grp;
        for (int k = 0; k < nr; k++) if (job_in[k] >= i0 && job_in[k] < i0 + g.ni) g.jobs.push_back(k);
        if (g.jobs.empty()) continue;
        const int nj = (int)g.jobs.size();
        gk.resize((size_t)nj); gt.resize((size_t)nj);
        for (int k = 0; k < nj; k++) { gk[(size_t)k] = key[g.jobs[(size_t)k]]; gt[(size_t)k] = tab[g.jobs[(size_t)k]]; }
        for (int c0 = 0; c0 < nj; c0 += chunk) {
            const int nb = nj - c0 < chunk ? nj - c0 : chunk;
            ksw_job_tiles(gk.data() + c0, gt.data() + c0, nb, T, tl);
            g.chunks.push_back(KswChunk{c0, nb, (int)g.tiles.size(), (int)tl.size()});
            g.tiles.insert(g.tiles.end(), tl.begin(), tl.end());
        }
        groups.push_back(std::move(g));
    }
}
