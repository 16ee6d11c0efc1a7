// settle_host.cpp -- the host side of emdee_md_set_rigid3, alone: the two functions of csrc/settle.hpp (plain C++ there) and the
// table builder of csrc/topology.hpp.  Reads one case from stdin and prints lines of numbers ("%.17g"), or "REFUSED <code>
// <message>" for a table the builder refuses.  tests/test_settle_host.py compiles this with the host compiler under ASan and
// UBSan and compares with tests/helpers/settle_ref.py.
//   positions <n> then per molecule: m_apex m_leg d_leg d_base x0 (9) x1 (9)   -> "<ok> x1 (9)" per molecule
//   velocities <n> then per molecule: m_apex m_leg x (9) v (9)                   -> "v (9)" per molecule
//   table <lim> <n> {apex a b} x n {d_leg d_base} x n                            -> "table <n> ids ..."
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/settle.hpp"
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
    if (!(std::cin >> t)) { fprintf(stderr, "settle_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")
static void nine(double (&x)[3][3]) {
    for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) x[k][d] = number();
}
static void print_nine(const double (&x)[3][3]) {
    for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) printf(" %.17g", x[k][d]);
    printf("\n");
}

static void positions() {
    const int64_t n = integer();
    for (int64_t m = 0; m < n; m++) {
        const double m_apex = number(), m_leg = number(), d_leg = number(), d_base = number();
        double x0[3][3], x1[3][3];
        nine(x0);
        nine(x1);
        const bool ok = settle_positions(x0, x1, m_apex, m_leg, d_leg, d_base);
        printf("%d", ok ? 1 : 0);
        print_nine(x1);
    }
}

static void velocities() {
    const int64_t n = integer();
    for (int64_t m = 0; m < n; m++) {
        const double m_apex = number(), m_leg = number();
        double x[3][3], v[3][3];
        nine(x);
        nine(v);
        settle_velocities(x, v, m_apex, m_leg);
        printf("v");
        print_nine(v);
    }
}

static void table() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> raw((size_t)3 * n);
    for (auto &g : raw) g = integer();
    std::vector<double> geom((size_t)2 * n);
    for (auto &g : geom) g = number();
    const std::vector<int32_t> h = topo::checked_rigid3(raw, geom, lim);
    printf("table %lld ids", (long long)(h.size() / 3));
    for (int32_t g : h) printf(" %d", g);
    printf("\n%s\n", topo::rigid3_message(h, 0, "message").c_str());
}

int main() {
    const std::string what = token();
    try {
        if (what == "positions") positions();
        else if (what == "velocities") velocities();
        else if (what == "table") table();
        else { fprintf(stderr, "settle_host: unknown case %s\n", what.c_str()); return 2; }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
