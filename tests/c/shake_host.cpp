// shake_host.cpp -- the host side of emdee_md_set_hbonds, alone: the two functions of csrc/shake.hpp (plain C++ there) and the
// table builder of csrc/topology.hpp.  Reads one case from stdin and prints lines of numbers ("%.17g"), or "REFUSED <code>
// <message>" for a table the builder refuses.  tests/test_shake_host.py compiles this with the host compiler under ASan and
// UBSan and compares with tests/helpers/shake_ref.py.
//   positions <n> then per cluster: nsat m (4) d (3) x0 (12) x1 (12)   -> "<ok> <newton steps> x1 (12)" per cluster
//   velocities <n> then per cluster: nsat m (4) x (12) v (12)          -> "v (12)" per cluster
//   table <lim> <n> {c s1 s2 s3} x n {d1 d2 d3} x n <nr> {rigid ids} x nr   -> "table <n> ids ..." and a message
//   rigid <lim> <n> {apex a b} x n {d_leg d_base} x n <nh> {hbonds ids} x nh -> "table <n>"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/shake.hpp"
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
    if (!(std::cin >> t)) { fprintf(stderr, "shake_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")
static void twelve(double (&x)[4][3]) {
    for (int k = 0; k < 4; k++)
        for (int d = 0; d < 3; d++) x[k][d] = number();
}
static void print_twelve(const double (&x)[4][3]) {
    for (int k = 0; k < 4; k++)
        for (int d = 0; d < 3; d++) printf(" %.17g", x[k][d]);
    printf("\n");
}
static void inverse_masses(double (&w)[4]) {
    for (int k = 0; k < 4; k++) w[k] = 1.0 / number();
}

static void positions() {
    const int64_t n = integer();
    for (int64_t m = 0; m < n; m++) {
        const int nsat = (int)integer();
        double w[4], d[3], x0[4][3], x1[4][3];
        inverse_masses(w);
        for (int k = 0; k < 3; k++) d[k] = number();
        twelve(x0);
        twelve(x1);
        int steps = -1;
        const bool ok = shake_positions(x0, x1, w, d, nsat, &steps);
        printf("%d %d", ok ? 1 : 0, steps);
        print_twelve(x1);
    }
}

static void velocities() {
    const int64_t n = integer();
    for (int64_t m = 0; m < n; m++) {
        const int nsat = (int)integer();
        double w[4], x[4][3], v[4][3];
        inverse_masses(w);
        twelve(x);
        twelve(v);
        shake_velocities(x, v, w, nsat);
        printf("v");
        print_twelve(v);
    }
}

static void table() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> raw((size_t)4 * n);
    for (auto &g : raw) g = integer();
    std::vector<double> dist((size_t)3 * n);
    for (auto &g : dist) g = number();
    std::vector<int32_t> rigid((size_t)integer());
    for (auto &g : rigid) g = (int32_t)integer();
    const std::vector<int32_t> h = topo::checked_hbonds(raw, dist, lim, rigid.empty() ? nullptr : &rigid);
    printf("table %lld ids", (long long)(h.size() / 4));
    for (int32_t g : h) printf(" %d", g);
    printf("\n%s\n", topo::hbonds_message(h, 0, "message").c_str());
    printf("dist");
    for (double d : topo::hbonds_distances(h, dist)) printf(" %.17g", d);
    printf("\n");
}

static void rigid() {
    const int64_t lim = integer(), n = integer();
    std::vector<int64_t> raw((size_t)3 * n);
    for (auto &g : raw) g = integer();
    std::vector<double> geom((size_t)2 * n);
    for (auto &g : geom) g = number();
    std::vector<int32_t> hb((size_t)integer());
    for (auto &g : hb) g = (int32_t)integer();
    const std::vector<int32_t> h = topo::checked_rigid3(raw, geom, lim, hb.empty() ? nullptr : &hb);
    printf("table %lld\n", (long long)(h.size() / 3));
}

int main() {
    const std::string what = token();
    try {
        if (what == "positions") positions();
        else if (what == "velocities") velocities();
        else if (what == "table") table();
        else if (what == "rigid") rigid();
        else { fprintf(stderr, "shake_host: unknown case %s\n", what.c_str()); return 2; }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
