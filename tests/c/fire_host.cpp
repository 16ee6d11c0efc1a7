// fire_host.cpp -- the host side of emdee_md_minimize, alone: the two update rules of csrc/minimize.hpp (plain C++ there).  Reads
// one case from stdin and prints lines of numbers ("%.17g").  tests/test_fire_host.py compiles this with the host compiler under
// ASan and UBSan and compares with tests/helpers/fire_ref.py.
//   cap <n> then per row: dt vmax amax max_step                 -> "t" per row
//   update <dt_start> <dt_max> <n> then P x n                   -> "<mix> dt alpha n_pos" per P
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../emdee.jl_amd/csrc/minimize.hpp"

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "fire_host: input ends early\n"); exit(2); }
    return t;
}
static long long integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

static void cap() {
    const long long n = integer();
    for (long long k = 0; k < n; k++) {
        const double dt = number(), vmax = number(), amax = number(), max_step = number();
        printf("%.17g\n", fire_cap(dt, vmax, amax, max_step));
    }
}

static void update() {
    const double dt_start = number(), dt_max = number();
    const long long n = integer();
    FireState s = fire_start(dt_start, dt_max);
    for (long long k = 0; k < n; k++) {
        const bool mix = fire_update(s, number());
        printf("%d %.17g %.17g %d\n", mix ? 1 : 0, s.dt, s.alpha, s.n_pos);
    }
}

int main() {
    const std::string what = token();
    if (what == "cap") cap();
    else if (what == "update") update();
    else { fprintf(stderr, "fire_host: unknown case %s\n", what.c_str()); return 2; }
    return 0;
}
