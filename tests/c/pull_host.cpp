// pull_host.cpp -- the host side of emdee_md_set_pull, alone: the functions of csrc/pull.hpp (plain C++ there) and the table builder
// of csrc/topology.hpp.  Reads one case from stdin and prints lines of numbers ("%.17g"), or "REFUSED <code> <message>" for a table
// the builder refuses.  tests/test_pull_host.py compiles this with the host compiler under ASan and UBSan and compares with
// tests/helpers/pull_ref.py.
//   words                                                                 -> "<PULL_WORDS> <PULL_GROUP_WORDS> <PULL_MAX_GROUPS> <PULL_MAX_COORDS>"
//   term <n> {kind geometry mask k nx ny nz xi0 Dx Dy Dz} x n             -> "xi f U Fb (3) T (6)" per entry
//   work <n> {f rate dt} x n                                              -> the work word after each entry, from 0
//   advance <xi0> <rate> <dt> <n>                                         -> xi0 after n steps
//   group <nc> {a b U Fb (3) T (6)} x nc <g> <M>                           -> the group's ten words
//   table <n> {group} x n <n_groups> <nc> {a b kind geometry mask} x nc {k r0 rate nx ny nz} x nc <nv> {vsite ids} x nv
//                                     -> "table <n_grouped> <n_chunks>", "ids ...", "group_of ...", "chunks first count group ...",
//                                        then "a b kind geometry mask k rate nx ny nz r0" per coordinate
//   vsites <lim> <n> {site a b c} x n {w_b w_c} x n <np> {pulled ids} x np   -> "sites <n>"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/pull.hpp"
#include "../../emdee.jl_amd/csrc/topology.hpp"

namespace emdee {
static char g_error[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_error; }
}  // namespace emdee

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "pull_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

static void term(int64_t n) {
    for (int64_t e = 0; e < n; e++) {
        PullCoord c{};
        c.a = 0; c.b = 1;
        c.kind = (int)integer(); c.geometry = (int)integer(); c.mask = (int)integer();
        c.k = number(); c.rate = 0.0;
        for (auto &v : c.n) v = number();
        const double xi0 = number();
        double D[3];
        for (auto &v : D) v = number();
        PullResult r;
        pull_term(c, xi0, D, r);
        printf("%.17g %.17g %.17g", r.xi, r.f, r.U);
        for (double v : r.Fb) printf(" %.17g", v);
        for (double v : r.T) printf(" %.17g", v);
        printf("\n");
    }
}

static void group() {
    const int nc = (int)integer();
    std::vector<PullResult> res((size_t)nc);
    for (auto &r : res) {
        r = PullResult{};
        r.a = (int)integer(); r.b = (int)integer(); r.U = number();
        for (auto &v : r.Fb) v = number();
        for (auto &v : r.T) v = number();
    }
    const int g = (int)integer();
    const double M = number();
    double out[PULL_GROUP_WORDS];
    pull_group_words(res.data(), nc, g, M, out);
    for (double v : out) printf("%.17g ", v);
    printf("\n");
}

static void table() {
    const int64_t n = integer();
    std::vector<int64_t> grp((size_t)n);
    for (auto &g : grp) g = integer();
    const int64_t n_groups = integer(), nc = integer();
    const size_t rows = nc > 0 && nc <= 64 ? (size_t)nc : 0;    // (a count out of range: the builder refuses before it reads a row)
    std::vector<int32_t> ci(5 * rows);
    for (auto &v : ci) v = (int32_t)integer();
    std::vector<double> cd(6 * rows);
    for (auto &v : cd) v = number();
    std::vector<int32_t> vs((size_t)integer());
    for (auto &g : vs) g = (int32_t)integer();
    const topo::PullRows t = topo::pull_table(grp, n_groups, ci, cd, nc, vs.empty() ? nullptr : &vs);
    printf("table %d %zu\nids", t.lay.n_grouped, t.lay.chunks.size());
    for (int v : t.ids) printf(" %d", v);
    printf("\ngroup_of");
    for (int v : t.group_of) printf(" %d", v);
    printf("\nchunks");
    for (const MsdChunk &c : t.lay.chunks) printf(" %d %d %d", c.first, c.count, c.group);
    printf("\n");
    for (int c = 0; c < t.n_coords; c++) {
        const PullCoord &p = t.coord[c];
        printf("%d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", p.a, p.b, p.kind, p.geometry, p.mask, p.k, p.rate, p.n[0], p.n[1], p.n[2],
               t.r0[c]);
    }
}

static void vsites() {
    const int64_t lim = integer(), n = integer();
    std::vector<int32_t> raw((size_t)4 * n);
    for (auto &g : raw) g = (int32_t)integer();
    std::vector<double> w((size_t)2 * n);
    for (auto &v : w) v = number();
    std::vector<int32_t> pulled((size_t)integer());
    for (auto &g : pulled) g = (int32_t)integer();
    const std::vector<int32_t> out = topo::checked_vsites(raw, w, lim, nullptr, nullptr, nullptr, &pulled);
    printf("sites %zu\n", out.size() / 4);
}

int main() {
    const std::string what = token();
    try {
        if (what == "words") {
            printf("%d %d %d %d\n", PULL_WORDS, PULL_GROUP_WORDS, PULL_MAX_GROUPS, PULL_MAX_COORDS);
        } else if (what == "term") {
            term(integer());
        } else if (what == "work") {
            const int64_t n = integer();
            double w = 0.0;
            for (int64_t e = 0; e < n; e++) {
                const double f = number(), rate = number(), dt = number();
                w = pull_work(w, f, rate, dt);
                printf("%.17g\n", w);
            }
        } else if (what == "advance") {
            double xi0 = number();
            const double rate = number(), dt = number();
            const int64_t n = integer();
            for (int64_t s = 0; s < n; s++) xi0 = pull_advance(xi0, rate, dt);
            printf("%.17g\n", xi0);
        } else if (what == "group") {
            group();
        } else if (what == "table") {
            table();
        } else if (what == "vsites") {
            vsites();
        } else {
            fprintf(stderr, "pull_host: unknown case %s\n", what.c_str());
            return 2;
        }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
