// gk_host.cpp -- the parts of the Green-Kubo observables with no HIP in them, alone: csrc/gk.hpp (plain C++ there).
// Reads one case from stdin and prints lines of numbers.  tests/test_gk_host.py compiles this with the host compiler under ASan and
// UBSan and compares with numpy and a brute-force enumeration of its own.
//   words                                                     -> "GK_WORDS GK_STRESS_WORDS GK_HEAT_WORDS GK_MAX_LAGS"
//   stress <n> then 12 doubles x n (W then K)                 -> per case the six stress words ("%.17g")
//   ring <n_lags> <s_end>                                     -> per s = 0 .. s_end: "slot live", then the slot of s - l for l < live
//   count <n_lags> <samples>                                  -> the n_lags counts
//   heat <float|double> <n> then 11 numbers x n (inv_mass, e, w x 6, v x 3) -> per case the three addends ("%.17g")
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../emdee.jl_amd/csrc/gk.hpp"

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "gk_host: input ends early\n"); exit(2); }
    return t;
}
static long long integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }

static void stress() {
    const long long n = integer();
    for (long long k = 0; k < n; k++) {
        double t[GK_BOX_SUMS], out[GK_STRESS_WORDS];
        for (double &v : t) v = number();
        gk_stress_words(t, out);
        for (double v : out) printf("%.17g ", v);
        printf("\n");
    }
}

static void ring() {
    const int n_lags = (int)integer();
    const long long s_end = integer();
    for (long long s = 0; s <= s_end; s++) {
        const int live = gk_live_lags(s, n_lags);
        printf("%d %d", gk_slot(s, n_lags), live);
        for (int l = 0; l < live; l++) printf(" %d", gk_slot(s - l, n_lags));
        printf("\n");
    }
}

static void count() {
    const int n_lags = (int)integer();
    const long long samples = integer();
    for (int l = 0; l < n_lags; l++) printf("%lld ", gk_count(samples, l));
    printf("\n");
}

template <typename real>
static void heat() {
    const long long n = integer();
    for (long long k = 0; k < n; k++) {
        const real inv_mass = (real)number(), e = (real)number();
        real w[6], v[3];
        for (real &x : w) x = (real)number();
        for (real &x : v) x = (real)number();
        double out[GK_HEAT_WORDS];
        gk_heat_term<real>(inv_mass, e, w, v, out);
        for (double x : out) printf("%.17g ", x);
        printf("\n");
    }
}

int main() {
    const std::string what = token();
    if (what == "words") printf("%d %d %d %d\n", GK_WORDS, GK_STRESS_WORDS, GK_HEAT_WORDS, GK_MAX_LAGS);
    else if (what == "stress") stress();
    else if (what == "ring") ring();
    else if (what == "count") count();
    else if (what == "heat") {
        const std::string real = token();
        if (real == "float") heat<float>();
        else if (real == "double") heat<double>();
        else { fprintf(stderr, "gk_host: unknown precision %s\n", real.c_str()); return 2; }
    } else { fprintf(stderr, "gk_host: unknown case %s\n", what.c_str()); return 2; }
    return 0;
}
