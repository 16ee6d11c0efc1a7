// vsite_host.cpp -- the host side of emdee_md_set_vsites, alone: the two functions of csrc/vsite.hpp (plain C++ there) and the
// table builders of csrc/topology.hpp.  Reads one case from stdin and prints lines of numbers ("%.17g"), or "REFUSED <code>
// <message>" for a table a builder refuses.  tests/test_vsite_host.py compiles this with the host compiler under ASan and UBSan
// and compares with tests/helpers/vsite_ref.py.
//   place <len (3)> <per (3)> <n_atoms> x (3 n_atoms) <n> {site a b c} x n {w_b w_c} x n    -> "x (3)" per entry
//   spread <n_atoms> f (3 n_atoms) <n> {site a b c} x n {w_b w_c} x n                       -> "f (3)" per atom, after spreading
//   table <lim> <n> {site a b c} x n {w_b w_c} x n <nr> {rigid ids} x nr <nh> {hbonds ids} x nh
//                                              -> "table <n> ids ...", a message, "weights ...", "parents ...", "start ...", "entries (site weight) ..."
//   rigid <lim> <n> {apex a b} x n {d_leg d_base} x n <nv> {vsite ids} x nv                 -> "table <n>"
//   hbonds <lim> <n> {c s1 s2 s3} x n {d1 d2 d3} x n <nv> {vsite ids} x nv                  -> "table <n>"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/topology.hpp"
#include "../../emdee.jl_amd/csrc/vsite.hpp"

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
    if (!(std::cin >> t)) { fprintf(stderr, "vsite_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

struct Table {
    std::vector<int32_t> atoms;
    std::vector<double> weights;
};
// the entries of a case, through the builder (as Topology::set_vsites does)
static Table read_table(int64_t lim) {
    const int64_t n = integer();
    std::vector<int64_t> raw((size_t)4 * n);
    for (auto &g : raw) g = integer();
    std::vector<double> w((size_t)2 * n);
    for (auto &g : w) g = number();
    Table t;
    t.atoms = topo::checked_vsites(raw, w, lim);
    t.weights = topo::vsite_weights(t.atoms, w);
    return t;
}

static void place() {
    double len[3];
    int per[3];
    for (auto &v : len) v = number();
    for (auto &v : per) v = (int)integer();
    const int64_t n_atoms = integer();
    std::vector<double> x((size_t)3 * n_atoms);
    for (auto &v : x) v = number();
    const Table t = read_table(n_atoms);
    for (size_t s = 0; s < t.atoms.size() / 4; s++) {
        const int32_t a = t.atoms[4 * s + 1], b = t.atoms[4 * s + 2], c = t.atoms[4 * s + 3];
        double xa[3], d[3], e[3], out[3];
        for (int k = 0; k < 3; k++) {
            xa[k] = x[(size_t)3 * a + k];
            d[k] = vsite_image(x[(size_t)3 * b + k] - xa[k], len[k], per[k]);
            e[k] = c >= 0 ? vsite_image(x[(size_t)3 * c + k] - xa[k], len[k], per[k]) : 0.0;
        }
        vsite_place(xa, d, e, t.weights[2 * s], t.weights[2 * s + 1], out);
        printf("%.17g %.17g %.17g\n", out[0], out[1], out[2]);
    }
}

static void spread() {
    const int64_t n_atoms = integer();
    std::vector<double> f((size_t)3 * n_atoms);
    for (auto &v : f) v = number();
    const Table t = read_table(n_atoms);
    const topo::VsiteParents par = topo::build_vsite_parents(t.atoms, t.weights);
    std::vector<double> out(f);
    // one pass per distinct parent, as the kernel's threads; then the sites' forces are cleared
    for (size_t q = 0; q < par.parent.size(); q++) {
        const int32_t p = par.parent[q];
        double fp[3] = {f[(size_t)3 * p], f[(size_t)3 * p + 1], f[(size_t)3 * p + 2]};
        vsite_spread_parent(par.site.data(), par.weight.data(), par.start[q], par.start[q + 1], [&](int s, double (&fs)[3]) {
            for (int k = 0; k < 3; k++) fs[k] = f[(size_t)3 * t.atoms[(size_t)4 * s] + k];
        }, fp);
        for (int k = 0; k < 3; k++) out[(size_t)3 * p + k] = fp[k];
    }
    for (size_t s = 0; s < t.atoms.size() / 4; s++)
        for (int k = 0; k < 3; k++) out[(size_t)3 * t.atoms[4 * s] + k] = 0.0;
    for (int64_t i = 0; i < n_atoms; i++) printf("%.17g %.17g %.17g\n", out[(size_t)3 * i], out[(size_t)3 * i + 1], out[(size_t)3 * i + 2]);
}

static std::vector<int32_t> ids() {
    std::vector<int32_t> v((size_t)integer());
    for (auto &g : v) g = (int32_t)integer();
    return v;
}

static void table() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> raw((size_t)4 * n);
    for (auto &g : raw) g = integer();
    std::vector<double> w((size_t)2 * n);
    for (auto &g : w) g = number();
    const std::vector<int32_t> rigid = ids(), hb = ids();
    const std::vector<int32_t> h = topo::checked_vsites(raw, w, lim, rigid.empty() ? nullptr : &rigid, hb.empty() ? nullptr : &hb);
    printf("table %lld ids", (long long)(h.size() / 4));
    for (int32_t g : h) printf(" %d", g);
    printf("\n%s\n", topo::vsite_message(h, 0, "message").c_str());
    const std::vector<double> ww = topo::vsite_weights(h, w);
    printf("weights");
    for (double v : ww) printf(" %.17g", v);
    const topo::VsiteParents par = topo::build_vsite_parents(h, ww);
    printf("\nparents");
    for (int32_t g : par.parent) printf(" %d", g);
    printf("\nstart");
    for (int32_t g : par.start) printf(" %d", g);
    printf("\nentries");
    for (size_t e = 0; e < par.site.size(); e++) printf(" %d %.17g", par.site[e], par.weight[e]);
    printf("\n");
}

static void rigid() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> raw((size_t)3 * n);
    for (auto &g : raw) g = integer();
    std::vector<double> geom((size_t)2 * n);
    for (auto &g : geom) g = number();
    const std::vector<int32_t> vs = ids();
    const std::vector<int32_t> h = topo::checked_rigid3(raw, geom, lim, nullptr, vs.empty() ? nullptr : &vs);
    printf("table %lld\n", (long long)(h.size() / 3));
}

static void hbonds() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> raw((size_t)4 * n);
    for (auto &g : raw) g = integer();
    std::vector<double> dist((size_t)3 * n);
    for (auto &g : dist) g = number();
    const std::vector<int32_t> vs = ids();
    const std::vector<int32_t> h = topo::checked_hbonds(raw, dist, lim, nullptr, vs.empty() ? nullptr : &vs);
    printf("table %lld\n", (long long)(h.size() / 4));
}

int main() {
    const std::string what = token();
    try {
        if (what == "place") place();
        else if (what == "spread") spread();
        else if (what == "table") table();
        else if (what == "rigid") rigid();
        else if (what == "hbonds") hbonds();
        else { fprintf(stderr, "vsite_host: unknown case %s\n", what.c_str()); return 2; }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
