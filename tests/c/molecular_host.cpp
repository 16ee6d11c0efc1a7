// molecular_host.cpp -- the host side of emdee_md_molecular_pressure_tensor and emdee_md_set_molecular_scaling, alone: the two
// per-molecule functions of csrc/settle.hpp (plain C++ there) and the membership builder of csrc/topology.hpp.  Reads one case
// from stdin and prints lines of numbers ("%.17g").  tests/test_molecular_host.py compiles this with the host compiler under ASan
// and UBSan and compares with tests/helpers/molecular_ref.py.
//   sums <n> then per molecule: m_apex m_leg y (9) v (9) f (9)                   -> "s" and the twelve terms per molecule
//   scale <n> mu (3) lo (3) velocity_scale then per molecule: m_apex m_leg y (9) v (9)   -> "c shift (3) dv (3)" per molecule
//   members <lim> <n> {apex a b} x n                                             -> "members" and lim bytes
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
    if (!(std::cin >> t)) { fprintf(stderr, "molecular_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }
static void nine(double (&x)[3][3]) {
    for (int k = 0; k < 3; k++)
        for (int d = 0; d < 3; d++) x[k][d] = number();
}

static void sums() {
    const int64_t n = integer();
    for (int64_t m = 0; m < n; m++) {
        const double m_apex = number(), m_leg = number();
        double y[3][3], v[3][3], f[3][3], out[12];
        nine(y);
        nine(v);
        nine(f);
        molecule_sums(y, v, f, m_apex, m_leg, out);
        printf("s");
        for (double t : out) printf(" %.17g", t);
        printf("\n");
    }
}

static void scale() {
    const int64_t n = integer();
    double mu[3], lo[3];
    for (double &t : mu) t = number();
    for (double &t : lo) t = number();
    const double vscale = number();
    for (int64_t m = 0; m < n; m++) {
        const double m_apex = number(), m_leg = number();
        double y[3][3], v[3][3], shift[3], dv[3];
        nine(y);
        nine(v);
        molecule_scale(y, v, m_apex, m_leg, mu, lo, vscale, shift, dv);
        printf("c %.17g %.17g %.17g %.17g %.17g %.17g\n", shift[0], shift[1], shift[2], dv[0], dv[1], dv[2]);
    }
}

static void members() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> raw((size_t)3 * n);
    for (auto &g : raw) g = integer();
    const std::vector<double> geom((size_t)2 * n, 1.0);
    const std::vector<uint8_t> member = topo::rigid3_members(topo::checked_rigid3(raw, geom, lim), lim);
    printf("members");
    for (uint8_t b : member) printf(" %d", (int)b);
    printf("\n");
}

int main() {
    const std::string what = token();
    try {
        if (what == "sums") sums();
        else if (what == "scale") scale();
        else if (what == "members") members();
        else { fprintf(stderr, "molecular_host: unknown case %s\n", what.c_str()); return 2; }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
