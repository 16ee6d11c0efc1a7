// ewald_host.cpp -- the host side of the Ewald sum (csrc/topology.hpp check_ewald, ewald_vectors, ewald_table, lost_pair_message),
// alone: reads one case from stdin and prints what they build, or "REFUSED <code> <message>" for a case they refuse.
// tests/test_ewald_host.py compiles this with the host compiler under ASan and UBSan and compares with tests/helpers/ewald_ref.py.
//   check <alpha> <rc> <has_kmax> <kx> <ky> <kz>                       "ok" or the refusal
//   table <alpha> <Lx> <Ly> <Lz> <kx> <ky> <kz>                        "count <m>", then per vector "k <nx> <ny> <nz> <a> <b> <kx> <ky> <kz>"
//   lost <n> {i j} x n <n14> {i j} x n14 <entry>                       the message for that entry of the struck CSR
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
    if (!(std::cin >> t)) { fprintf(stderr, "ewald_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

static void check() {
    const double alpha = number(), rc = number();
    const bool has = integer() != 0;
    const int32_t kmax[3] = {(int32_t)integer(), (int32_t)integer(), (int32_t)integer()};
    topo::check_ewald(alpha, has ? kmax : nullptr, rc);
    printf("ok\n");
}

static void table() {
    const double alpha = number();
    const double len[3] = {number(), number(), number()};
    const int32_t kmax[3] = {(int32_t)integer(), (int32_t)integer(), (int32_t)integer()};
    const std::vector<int32_t> n = topo::ewald_vectors(kmax);
    const std::vector<topo::EwaldK> t = topo::ewald_table(n, len, alpha);
    printf("count %zu\n", t.size());
    for (const topo::EwaldK &e : t)
        printf("k %d %d %d %.17g %.17g %.17g %.17g %.17g\n", e.nx, e.ny, e.nz, e.a, e.b, e.kx, e.ky, e.kz);
}

static std::vector<int32_t> pairs() {
    std::vector<int32_t> v(2 * (size_t)integer());
    for (auto &x : v) x = (int32_t)integer();
    return v;
}
static void lost() {
    const std::vector<int32_t> excl = pairs(), p14 = pairs();
    printf("lost %s\n", topo::lost_pair_message(excl, p14, integer()).c_str());
}

int main() {
    const std::string what = token();
    try {
        if (what == "check") check();
        else if (what == "table") table();
        else if (what == "lost") lost();
        else { fprintf(stderr, "ewald_host: unknown case %s\n", what.c_str()); return 2; }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
