// The host C++ of the ring-vector encoder / decoder on the CPU (no HIP, no device): sfgwas_amd/csrc/rvec_host.hpp (root constants brought to the table's fixed point,
// limb-count selection, refusal arithmetic) and sfgwas_amd/csrc/rvec_fx.hpp (the W-word arithmetic and the per-element work of every kernel of rvec.hip), driven
// over a whole 8192-point transform in the kernels' order.  tests/test_rvec_ref.py builds this with -fsanitize=address,undefined and holds its words against
// tests/rvec_ref.py.
//   host_rvec_test <command file> <output file>
// command file, whitespace separated:
//   plan (enc|dec) limbs f n_elem scale level nq q_0.. p_0..p_{limbs-1}       -> "ok W g shift" or "refused <message>"
//   roots                                                                     -> "k cos sin" (hex, 574 fractional bits), k = 1..15
//   table cnt j_1..j_cnt                                                      -> "j re im" (signed hex, 574 fractional bits)
//   encode limbs f n_elem scale level nq q_0.. p_0.. x_0..x_{n_elem-1} (hex)  -> "ok W g shift", then N signed hex coefficients, then (level+1) rows of N residues
//   decode limbs f n_elem scale level nq q_0.. p_0.. c_0..c_{N-1} (signed hex)-> "ok W g shift", then n_elem hex residues
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sfgwas_amd/csrc/rvec_fx.hpp"

static const int N = 1 << 14, n = N / 2;

static std::string hex_of(const rv_u64 *w, int nw) {          // unsigned, no leading zeros
    std::string s;
    char b[20];
    bool lead = true;
    for (int i = nw - 1; i >= 0; i--) {
        if (lead && !w[i] && i) continue;
        snprintf(b, sizeof b, lead ? "%llx" : "%016llx", w[i]);
        s += b; lead = false;
    }
    return s;
}
template <int W> static std::string shex_of(const rv_u64 (&w)[W]) {
    rv_u64 t[W];
    for (int i = 0; i < W; i++) t[i] = w[i];
    const bool neg = fx_isneg<W>(t);
    if (neg) fx_negate<W>(t);
    return (neg ? "-" : "") + hex_of(t, W);
}
// hex (optionally signed) -> nw words; false when it does not fit
static bool parse_hex(const std::string &tok, rv_u64 *w, int nw, bool *neg) {
    size_t i0 = 0;
    *neg = false;
    if (!tok.empty() && tok[0] == '-') { *neg = true; i0 = 1; }
    for (int i = 0; i < nw; i++) w[i] = 0;
    const size_t nd = tok.size() - i0;
    if (!nd || nd > (size_t)nw * 16) return false;
    for (size_t d = 0; d < nd; d++) {
        const char ch = tok[tok.size() - 1 - d];
        int v;
        if (ch >= '0' && ch <= '9') v = ch - '0'; else if (ch >= 'a' && ch <= 'f') v = ch - 'a' + 10; else if (ch >= 'A' && ch <= 'F') v = ch - 'A' + 10; else return false;
        w[d / 16] |= (rv_u64)v << (4 * (d % 16));
    }
    return true;
}

struct Table {
    std::vector<rv_u64> w;                                     // [N][2][9]
    Table() : w((size_t)N * 2 * RVEC_TW_LIMBS) {
        std::vector<rv_u64> roots(14 * 2 * RVEC_TW_LIMBS);
        rvec_host_roots(roots.data());
        for (int j = 0; j < N; j++) {
            rv_u64 ar[RVEC_TW_LIMBS], ai[RVEC_TW_LIMBS];
            rvec_table_entry(roots.data(), j, ar, ai);
            for (int k = 0; k < RVEC_TW_LIMBS; k++) { w[((size_t)j * 2) * RVEC_TW_LIMBS + k] = ar[k]; w[((size_t)j * 2 + 1) * RVEC_TW_LIMBS + k] = ai[k]; }
        }
    }
    template <int W> void load(int j, bool conj, rv_u64 (&tr)[W], rv_u64 (&ti)[W]) const {       // rvec.hip tw_load
        for (int k = 0; k < W; k++) {
            tr[k] = w[((size_t)j * 2) * RVEC_TW_LIMBS + RVEC_TW_LIMBS - W + k];
            ti[k] = w[((size_t)j * 2 + 1) * RVEC_TW_LIMBS + RVEC_TW_LIMBS - W + k];
        }
        if (conj) fx_negate<W>(ti);
    }
};
static int brev13(int x) { int r = 0; for (int i = 0; i < 13; i++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }
static std::vector<int> slot_map() {
    std::vector<int> sm(n);
    rv_u64 g = 1;
    for (int t = 0; t < n; t++) { sm[t] = (int)(((g - 1) / 4) % n); g = (g * 5) % (2ULL * N); }
    return sm;
}

template <int W> struct Pt { rv_u64 re[W], im[W]; };
// the 13 stages in the kernels' order (the two passes of k_rvec_fft differ in which workgroup holds a point, not in the arithmetic)
template <int W> static void fft(std::vector<Pt<W>> &x, const Table &tb, bool conj) {
    for (int H = 1; H < n; H <<= 1)
        for (int i = 0; i < n; i++) {
            if (i & H) continue;
            rv_u64 tr[W], ti[W];
            tb.load<W>((i & (H - 1)) * (N / H), conj, tr, ti);
            rvec_butterfly<W>(x[i].re, x[i].im, x[i + H].re, x[i + H].im, tr, ti);
        }
}

struct Case { int limbs, f, n_elem, level, nq; double scale; std::vector<uint64_t> q, p; };
static bool read_case(std::istream &in, Case &c) {
    std::string sc;
    if (!(in >> c.limbs >> c.f >> c.n_elem >> sc >> c.level >> c.nq)) return false;
    c.scale = strtod(sc.c_str(), nullptr);
    if (c.nq < 1 || c.nq > 16) return false;
    c.q.resize(c.nq);
    for (auto &v : c.q) if (!(in >> v)) return false;
    const int np = c.limbs > 0 && c.limbs <= 8 ? c.limbs : 1;
    c.p.assign(np < 4 ? 4 : np, 0);
    for (int i = 0; i < np; i++) if (!(in >> c.p[i])) return false;
    return true;
}

template <int W> static int run_encode(std::istream &in, std::ostream &out, const Case &c, const RvecPlan &pl) {
    Table tb;
    const std::vector<int> sm = slot_map();
    RvecField f; rvec_field(c.limbs, c.p.data(), f);
    std::vector<Pt<W>> x(n);
    for (int t = 0; t < n; t++) {
        rv_u64 e[4] = {0, 0, 0, 0};
        if (t < c.n_elem) { std::string tok; bool neg; if (!(in >> tok) || !parse_hex(tok, e, 4, &neg) || neg) return 2; }
        Pt<W> &pt = x[brev13(sm[t])];
        rvec_centre_place<W>(e, f, pl.g, pt.re);
        for (int k = 0; k < W; k++) pt.im[k] = 0;
    }
    fft<W>(x, tb, true);
    const int nl = c.level + 1;
    std::vector<std::string> coef(N);
    std::vector<std::vector<rv_u64>> rows(nl, std::vector<rv_u64>(N));
    for (int cc = 0; cc < n; cc++) {
        rv_u64 tr[W], ti[W], yr[W], yi[W], rd[2][W + 1];
        tb.load<W>(cc, true, tr, ti);
        fx_cmul<W>(x[cc].re, x[cc].im, tr, ti, yr, yi);
        const bool neg0 = rvec_scale_round<W>(yr, pl.sc.mant, pl.shift, rd[0]), neg1 = rvec_scale_round<W>(yi, pl.sc.mant, pl.shift, rd[1]);
        coef[cc] = (neg0 ? "-" : "") + hex_of(rd[0], W + 1);
        coef[cc + n] = (neg1 ? "-" : "") + hex_of(rd[1], W + 1);
        for (int i = 0; i < nl; i++) { rows[i][cc] = rvec_mod_q<W + 1>(rd[0], neg0, c.q[i]); rows[i][cc + n] = rvec_mod_q<W + 1>(rd[1], neg1, c.q[i]); }
    }
    for (int i = 0; i < N; i++) out << coef[i] << "\n";
    for (int i = 0; i < nl; i++) for (int k = 0; k < N; k++) out << rows[i][k] << "\n";
    return 0;
}
template <int W> static int run_decode(std::istream &in, std::ostream &out, const Case &c, const RvecPlan &pl) {
    Table tb;
    const std::vector<int> sm = slot_map();
    RvecField f; rvec_field(c.limbs, c.p.data(), f);
    std::vector<Pt<W>> p(N), x(n);
    for (int i = 0; i < N; i++) {          // the kernel composes the integer from its mixed-radix digits over the chain: derive them here, then run its Horner
        std::string tok; bool neg; rv_u64 mag[W];
        if (!(in >> tok) || !parse_hex(tok, mag, W, &neg)) return 2;
        // mixed-radix digits of |c| by repeated short division (host only), then the kernel's Horner
        std::vector<rv_u64> dg(c.level + 1);
        rv_u64 cur[W];
        for (int k = 0; k < W; k++) cur[k] = mag[k];
        for (int d = 0; d <= c.level; d++) {
            rv_u128 rem = 0;
            for (int k = W - 1; k >= 0; k--) { const rv_u128 v = (rem << 64) | cur[k]; cur[k] = (rv_u64)(v / c.q[d]); rem = v % c.q[d]; }
            dg[d] = (rv_u64)rem;
        }
        rvec_from_digits<W>(dg.data(), (const rv_u64 *)c.q.data(), c.level + 1, neg, pl.g, p[i].re);
    }
    for (int cc = 0; cc < n; cc++) {
        rv_u64 tr[W], ti[W];
        tb.load<W>(cc, false, tr, ti);
        Pt<W> &pt = x[brev13(cc)];
        fx_cmul<W>(p[cc].re, p[cc + n].re, tr, ti, pt.re, pt.im);
    }
    fft<W>(x, tb, false);
    for (int t = 0; t < c.n_elem; t++) {
        rv_u64 r[4];
        rvec_div_mod_p<W>(x[sm[t]].re, pl.sc.mant, pl.shift, f, r);
        out << hex_of(r, 4) << "\n";
    }
    return 0;
}

#define BY_W(W_, ...) switch (W_) { case 2: { constexpr int W = 2; __VA_ARGS__; } break; case 3: { constexpr int W = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int W = 4; __VA_ARGS__; } break; case 5: { constexpr int W = 5; __VA_ARGS__; } break; case 6: { constexpr int W = 6; __VA_ARGS__; } break; \
    case 7: { constexpr int W = 7; __VA_ARGS__; } break; case 8: { constexpr int W = 8; __VA_ARGS__; } break; default: return 3; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_rvec_test <command file> <output file>\n"); return 1; }
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    std::string cmd;
    if (!(in >> cmd)) return 1;
    if (cmd == "roots") {
        for (int k = 1; k <= RVEC_NROOTS; k++) {
            uint64_t c[RVEC_TW_LIMBS], s[RVEC_TW_LIMBS];
            rvec_root_words(k, c, s);
            out << k << " " << hex_of((const rv_u64 *)c, RVEC_TW_LIMBS) << " " << hex_of((const rv_u64 *)s, RVEC_TW_LIMBS) << "\n";
        }
        return 0;
    }
    if (cmd == "table") {
        Table tb;
        int cnt = 0;
        in >> cnt;
        for (int i = 0; i < cnt; i++) {
            int j;
            if (!(in >> j) || j < 0 || j >= N) return 2;
            rv_u64 tr[RVEC_TW_LIMBS], ti[RVEC_TW_LIMBS];
            tb.load<RVEC_TW_LIMBS>(j, false, tr, ti);
            out << j << " " << shex_of<RVEC_TW_LIMBS>(tr) << " " << shex_of<RVEC_TW_LIMBS>(ti) << "\n";
        }
        return 0;
    }
    std::string dir;
    if (cmd == "plan") in >> dir; else dir = cmd == "encode" ? "enc" : "dec";
    Case c;
    if (!read_case(in, c)) return 2;
    RvecPlan pl;
    const char *e = dir == "enc" ? rvec_plan_encode(c.limbs, c.p.data(), c.q.data(), c.nq, c.n_elem, c.level, c.scale, c.f, pl)
                                 : rvec_plan_decode(c.limbs, c.p.data(), c.q.data(), c.nq, c.n_elem, c.level, c.scale, c.f, pl);
    if (e) { out << "refused " << e << "\n"; return 0; }
    out << "ok " << pl.W << " " << pl.g << " " << pl.shift << "\n";
    if (cmd == "plan") return 0;
    if (cmd == "encode") { BY_W(pl.W, return run_encode<W>(in, out, c, pl)) }
    if (cmd == "decode") { BY_W(pl.W, return run_decode<W>(in, out, c, pl)) }
    return 1;
}
