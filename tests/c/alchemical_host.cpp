// alchemical_host.cpp -- the host side of emdee_md_set_alchemical, alone: the pair function, its foreign-lambda variant, the words of
// a read and the table checks of csrc/alchemical.hpp (plain C++ there).  Reads one case from stdin and prints lines of numbers
// ("%.17g"), or "REFUSED <code> <message>" for a table the checks refuse.  tests/test_alchemical_host.py compiles this with the host
// compiler under ASan and UBSan and compares with tests/helpers/alchemical_ref.py.
//   words                                                               -> "<ALCH_WORDS> <ALCH_MAX_FOREIGN>"
//   pair <f|d> <rc> <rs> <n> {r2 sigma2 e4 lambda alpha} x n            -> "E W dEdl wr2" per entry, in the real type asked for
//   foreign <f|d> <rc> <rs> <r2> <sigma2> <e4> <alpha> <K> {lambda} x K -> "E" per lambda
//   params <lambda> <alpha> <nf> {foreign} x nf <log_every> <log_capacity>  -> "ok"
//   flags <n> {flag} x n                                                -> "flagged <k> ids ..."
//   charged <nf> {ids} x nf <nq> {q} x nq                               -> the first flagged atom with a charge, or -1
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
    if (!(std::cin >> t)) { fprintf(stderr, "alchemical_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

// the constants as make_model (csrc/lj_pair.hpp) forms them: each field rounded to the real type first
template <typename real>
static AlchModel<real> model(double rc, double rs) {
    const real rs2 = (real)(rs * rs), idl2 = (real)(1.0 / (rc * rc - rs * rs));
    return AlchModel<real>{idl2, rs2 * idl2, (real)60 * idl2};
}

template <typename real>
static void pairs(double rc, double rs, int64_t n) {
    const AlchModel<real> m = model<real>(rc, rs);
    for (int64_t e = 0; e < n; e++) {
        const real r2 = (real)number(), sigma2 = (real)number(), e4 = (real)number(), lambda = (real)number(), alpha = (real)number();
        real E, W, dEdl, wr2;
        alch_pair(r2, m, sigma2, e4, lambda, alpha, E, W, dEdl, wr2);
        printf("%.17g %.17g %.17g %.17g\n", (double)E, (double)W, (double)dEdl, (double)wr2);
    }
}

template <typename real>
static void foreign(double rc, double rs) {
    const AlchModel<real> m = model<real>(rc, rs);
    const real r2 = (real)number(), sigma2 = (real)number(), e4 = (real)number(), alpha = (real)number();
    const int64_t K = integer();
    std::vector<real> lam((size_t)K), E((size_t)K);
    for (auto &v : lam) v = (real)number();
    alch_pair_foreign(r2, m, sigma2, e4, alpha, lam.data(), (int)K, E.data());
    for (real v : E) printf("%.17g\n", (double)v);
}

int main() {
    const std::string what = token();
    try {
        if (what == "words") {
            printf("%d %d\n", ALCH_WORDS, ALCH_MAX_FOREIGN);
        } else if (what == "pair" || what == "foreign") {
            const std::string real = token();
            const double rc = number(), rs = number();
            if (what == "pair") {
                const int64_t n = integer();
                if (real == "f") pairs<float>(rc, rs, n); else pairs<double>(rc, rs, n);
            } else {
                if (real == "f") foreign<float>(rc, rs); else foreign<double>(rc, rs);
            }
        } else if (what == "params") {
            const double lambda = number(), alpha = number();
            const int64_t nf = integer();
            std::vector<double> f((size_t)(nf > 0 && nf <= 64 ? nf : 0));   // (a count out of range: refused before an entry is read)
            for (auto &v : f) v = number();
            const int64_t every = integer(), capacity = integer();
            alch_check_params(lambda, alpha, f.empty() ? nullptr : f.data(), nf, every, capacity);
            printf("ok\n");
        } else if (what == "flags") {
            std::vector<int64_t> flag((size_t)integer());
            for (auto &v : flag) v = integer();
            const std::vector<int32_t> ids = alch_check_flags(flag);
            printf("flagged %zu ids", ids.size());
            for (int32_t i : ids) printf(" %d", i);
            printf("\n");
        } else if (what == "charged") {
            std::vector<int32_t> ids((size_t)integer());
            for (auto &v : ids) v = (int32_t)integer();
            std::vector<double> q((size_t)integer());
            for (auto &v : q) v = number();
            printf("%lld\n", (long long)alch_first_charged(ids, q));
        } else {
            fprintf(stderr, "alchemical_host: unknown case %s\n", what.c_str());
            return 2;
        }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
