// restraint_host.cpp -- the host side of emdee_md_set_restraints, alone: the two functions of csrc/restraint.hpp (plain C++ there) and
// the table builder of csrc/topology.hpp.  Reads one case from stdin and prints lines of numbers ("%.17g"), or "REFUSED <code>
// <message>" for a table the builder refuses.  tests/test_restraint_host.py compiles this with the host compiler under ASan and UBSan
// and compares with tests/helpers/restraint_ref.py.
//   words                                                        -> "<RESTRAINT_WORDS>"
//   term <float|double> <n> {d (3) k (3) r0} x n                 -> "U f (3) T (6)" per entry
//   scale <n> {ref lo mu} x n                                    -> "ref'" per entry
//   table <lim> <n> {id} x n <nref: 0 or n> {ref (3)} x nref {k (3)} x n <nflat: 0 or n> {r0} x nflat <nv> {vsite ids} x nv
//                                                                -> "table <n>", then "id ref (3) k (3) r0" per entry (ref: 0 if none)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/restraint.hpp"
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
    if (!(std::cin >> t)) { fprintf(stderr, "restraint_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

template <typename real>
static void term(int64_t n) {
    for (int64_t e = 0; e < n; e++) {
        double d[3], k[3];
        for (auto &v : d) v = number();
        for (auto &v : k) v = number();
        const double r0 = number();
        real f[3], T[6];
        const double U = restraint_term<real>(d, k, r0, f, T);
        printf("%.17g", U);
        for (real v : f) printf(" %.17g", (double)v);
        for (real v : T) printf(" %.17g", (double)v);
        printf("\n");
    }
}

static void table() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> ids((size_t)n);
    for (auto &g : ids) g = integer();
    std::vector<double> ref((size_t)(3 * integer()));
    for (auto &v : ref) v = number();
    std::vector<double> k((size_t)3 * n);
    for (auto &v : k) v = number();
    std::vector<double> flat((size_t)integer());
    for (auto &v : flat) v = number();
    std::vector<int32_t> vs((size_t)integer());
    for (auto &g : vs) g = (int32_t)integer();
    const topo::RestraintRows t = topo::restraint_table(ids, ref, k, flat, lim, vs.empty() ? nullptr : &vs);
    printf("table %zu\n", t.atoms.size());
    for (size_t e = 0; e < t.atoms.size(); e++) {
        printf("%d", t.atoms[e]);
        for (int a = 0; a < 3; a++) printf(" %.17g", t.ref.empty() ? 0.0 : t.ref[3 * e + a]);
        for (int a = 0; a < 3; a++) printf(" %.17g", t.k[3 * e + a]);
        printf(" %.17g\n", t.flat[e]);
    }
}

int main() {
    const std::string what = token();
    try {
        if (what == "words") {
            printf("%d\n", RESTRAINT_WORDS);
        } else if (what == "term") {
            const std::string real = token();
            const int64_t n = integer();
            if (real == "float") term<float>(n); else term<double>(n);
        } else if (what == "scale") {
            const int64_t n = integer();
            for (int64_t e = 0; e < n; e++) {
                const double ref = number(), lo = number(), mu = number();
                printf("%.17g\n", restraint_scale_ref(ref, lo, mu));
            }
        } else if (what == "table") {
            table();
        } else {
            fprintf(stderr, "restraint_host: unknown case %s\n", what.c_str());
            return 2;
        }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
