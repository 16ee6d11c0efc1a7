// alchemical_coulomb_host.cpp -- the host side of emdee_md_set_alchemical_coulomb, alone: the Coulomb pair function, its foreign
// variant and the parameter checks of csrc/alchemical.hpp (plain C++ there).  Reads one case from stdin and prints lines of numbers
// ("%.17g"), or "REFUSED <code> <message>" for parameters the checks refuse.  tests/test_alchemical_coulomb_host.py compiles this with
// the host compiler under ASan and UBSan and compares with tests/helpers/alchemical_coulomb_ref.py.
//   words                                                            -> "<ALCH_COULOMB_WORDS> <ALCH_WORDS> <ALCH_MAX_FOREIGN>"
//   pair <f|d> <k_rf> <c_rf> <n> {r2 qq lambda_q beta} x n           -> "E W dEdl wr2" per entry, in the real type asked for
//   foreign <f|d> <k_rf> <c_rf> <r2> <qq> <beta> <K> {lambda_q} x K  -> "E" per lambda_q
//   params <lambda_q> <beta> <nf> <null: 0|1> {foreign_q} x nf <table_nf>  -> "ok"
//   lambda <lambda_q>                                                -> "ok" (the check of emdee_md_set_lambda_coulomb)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/alchemical.hpp"

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
    if (!(std::cin >> t)) { fprintf(stderr, "alchemical_coulomb_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

template <typename real>
static void pairs(double k, double c, int64_t n) {
    const AlchRf<real> rf{(real)k, (real)c};
    for (int64_t e = 0; e < n; e++) {
        const real r2 = (real)number(), qq = (real)number(), lambda_q = (real)number(), beta = (real)number();
        real E, W, dEdl, wr2;
        alch_coulomb_pair(r2, qq, rf, lambda_q, beta, E, W, dEdl, wr2);
        printf("%.17g %.17g %.17g %.17g\n", (double)E, (double)W, (double)dEdl, (double)wr2);
    }
}

template <typename real>
static void foreign(double k, double c) {
    const AlchRf<real> rf{(real)k, (real)c};
    const real r2 = (real)number(), qq = (real)number(), beta = (real)number();
    const int64_t K = integer();
    std::vector<real> lam((size_t)K), E((size_t)K);
    for (auto &v : lam) v = (real)number();
    alch_coulomb_pair_foreign(r2, qq, rf, beta, lam.data(), (int)K, E.data());
    for (real v : E) printf("%.17g\n", (double)v);
}

int main() {
    const std::string what = token();
    try {
        if (what == "words") {
            printf("%d %d %d\n", ALCH_COULOMB_WORDS, ALCH_WORDS, ALCH_MAX_FOREIGN);
        } else if (what == "pair" || what == "foreign") {
            const std::string real = token();
            const double k = number(), c = number();
            if (what == "pair") {
                const int64_t n = integer();
                if (real == "f") pairs<float>(k, c, n); else pairs<double>(k, c, n);
            } else {
                if (real == "f") foreign<float>(k, c); else foreign<double>(k, c);
            }
        } else if (what == "params") {
            const double lambda_q = number(), beta = number();
            const int64_t nf = integer(), null = integer();
            std::vector<double> f((size_t)(nf > 0 && nf <= 64 && !null ? nf : 0));
            for (auto &v : f) v = number();
            const int64_t table_nf = integer();
            alch_coulomb_check_params(lambda_q, beta, f.empty() ? nullptr : f.data(), nf, table_nf);
            printf("ok\n");
        } else if (what == "lambda") {
            alch_check_lambda_q("set_lambda_coulomb", number());
            printf("ok\n");
        } else {
            fprintf(stderr, "alchemical_coulomb_host: unknown case %s\n", what.c_str());
            return 2;
        }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
