// pme_host.cpp -- the host side of smooth particle-mesh Ewald (csrc/topology.hpp check_pme, pme_bspline, pme_moduli, pme_fold,
// pme_twiddles, pme_fixed_shift), alone: reads one case from stdin and prints what they build, or "REFUSED <code> <message>"
// for a case they refuse.  tests/test_pme_host.py compiles this with the host compiler under ASan and UBSan and compares with
// tests/helpers/pme_ref.py.
//   check <alpha> <rc> <has_grid> <gx> <gy> <gz> <order>               "ok" or the refusal
//   moduli <K> <order>                                                 per index "b <m> <|b(m)|^2>"
//   fold <K>                                                           per index "n <m> <folded>"
//   twiddles <K>                                                       per index "t <j> <re> <im>"
//   spline <t> <order>                                                 per point "w <j> <M(t + j)> <M'(t + j)>"
//   shift <sum |q|>                                                    "shift <s>"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

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
    if (!(std::cin >> t)) { fprintf(stderr, "pme_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

static void check() {
    const double alpha = number(), rc = number();
    const bool has = integer() != 0;
    const int32_t grid[3] = {(int32_t)integer(), (int32_t)integer(), (int32_t)integer()};
    const int32_t order = (int32_t)integer();
    topo::check_pme(alpha, has ? grid : nullptr, order, rc);
    printf("ok\n");
}

int main() {
    const std::string what = token();
    try {
        if (what == "check") check();
        else if (what == "moduli") {
            const int K = (int)integer(), p = (int)integer();
            const std::vector<double> b = topo::pme_moduli(K, p);
            for (size_t m = 0; m < b.size(); m++) printf("b %zu %.17g\n", m, b[m]);
        } else if (what == "fold") {
            const int K = (int)integer();
            for (int m = 0; m < K; m++) printf("n %d %d\n", m, topo::pme_fold(m, K));
        } else if (what == "twiddles") {
            const int K = (int)integer();
            const std::vector<double> t = topo::pme_twiddles(K);
            for (int j = 0; j < K / 2; j++) printf("t %d %.17g %.17g\n", j, t[2 * (size_t)j], t[2 * (size_t)j + 1]);
        } else if (what == "spline") {
            const double t = number();
            const int p = (int)integer();
            double w[8], dw[8];
            topo::pme_bspline(t, p, w, dw);
            for (int j = 0; j < p; j++) printf("w %d %.17g %.17g\n", j, w[j], dw[j]);
        } else if (what == "shift") {
            printf("shift %d\n", topo::pme_fixed_shift(number()));
        } else { fprintf(stderr, "pme_host: unknown case %s\n", what.c_str()); return 2; }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
