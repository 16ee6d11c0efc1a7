// topology_host.cpp -- the host builders of csrc/topology.hpp, alone: reads one case from stdin, prints the tables they build
// as lines of "<name> <values ...>", or "REFUSED <code> <message>" for a case they refuse.  tests/test_topology_host.py
// compiles this with the host compiler under ASan and UBSan and compares with its own restatement of the layout.
//   pairs <lim> <n> {i j} x n <n14> {i j} x n14                 exclusions, then 1-4 pairs
//   bonded <lim> then per kind 1, 2, 3: <n> {ids} x n {params} x n, then term numbers for the lost-partner message
//   charges <n> <want> <K> <eps_rf> <coulomb14scale> {q} x n
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
    if (!(std::cin >> t)) { fprintf(stderr, "topology_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")
static std::vector<int64_t> integers(size_t n) {
    std::vector<int64_t> v(n);
    for (auto &x : v) x = integer();
    return v;
}
static std::vector<double> numbers(size_t n) {
    std::vector<double> v(n);
    for (auto &x : v) x = number();
    return v;
}
template <typename V>
static void line(const char *name, const V &v) {
    printf("%s", name);
    for (auto x : v) printf(" %lld", (long long)x);
    printf("\n");
}

static void pairs() {
    const int64_t lim = integer();
    const std::vector<int64_t> e = integers(2 * (size_t)integer());
    const std::vector<int64_t> p = integers(2 * (size_t)integer());
    const std::vector<int32_t> excl = topo::checked_pairs("set_exclusions", e, lim);
    const std::vector<int32_t> p14 = topo::checked_pairs("set_pairs14", p, lim);
    const topo::PairCsrs t = topo::build_pairs(excl, p14);
    printf("rows %d\nn14 %zu\nhas_excl %d\nhas_14 %d\n", t.rows, t.n14, (int)t.has_excl, (int)t.has_14);
    line("xs", t.xs); line("xi", t.xi); line("ps", t.ps); line("pi", t.pi);
}

static void bonded() {
    const int64_t lim = integer();
    std::vector<int32_t> atoms[topo::KINDS];
    std::vector<double> prm[topo::KINDS];
    for (int kind = 1; kind < topo::KINDS; kind++) {         // one kind at a time, each checked against the ones before it
        const size_t n = (size_t)integer();
        const std::vector<int64_t> raw = integers(n * topo::kind_atoms(kind));
        const std::vector<double> q = numbers(n * topo::kind_params(kind));
        atoms[kind] = topo::checked_terms(kind, raw, q, lim, atoms);
        prm[kind] = q;
    }
    const std::vector<int32_t> *at[topo::KINDS] = {nullptr, &atoms[1], &atoms[2], &atoms[3]};
    const std::vector<double> *pr[topo::KINDS] = {nullptr, &prm[1], &prm[2], &prm[3]};
    const topo::BondedRows t = topo::build_bonded(at, pr);
    printf("rows %d\nnb %zu\n", t.rows, t.nb);
    line("ps", t.ps); line("pi", t.pi); line("ts", t.ts); line("tid", t.tid);
    printf("terms");
    for (const topo::TermEntry &e : t.terms) printf(" %d %d %d %d", e.code, e.loc[0], e.loc[1], e.loc[2]);
    printf("\npd");
    for (double x : t.pd) printf(" %.17g", x);
    printf("\npf");
    for (float x : t.pf) printf(" %.9g", x);
    printf("\n");
    int64_t total = 0;
    for (int kind = 1; kind < topo::KINDS; kind++) total += (int64_t)atoms[kind].size() / topo::kind_atoms(kind);
    for (int64_t id = 0; id < total; id++) {
        int kind;
        int64_t index;
        topo::bonded_term_of(atoms, id, kind, index);
        printf("term_of %lld %d %lld\n", (long long)id, kind, (long long)index);
    }
    std::string t2;
    while (std::cin >> t2) printf("lost %s\n", topo::lost_partner_message(atoms, strtoll(t2.c_str(), nullptr, 10)).c_str());
}

static void charges() {
    const int64_t n = integer(), want = integer();
    const double K = number(), eps = number(), s14 = number();
    std::vector<double> q = numbers((size_t)n);
    topo::check_coulomb(n, want, K, eps, s14);
    topo::scale_charges(q, K);
    printf("q");
    for (double x : q) printf(" %.17g", x);
    printf("\n");
}

int main() {
    const std::string what = token();
    try {
        if (what == "pairs") pairs();
        else if (what == "bonded") bonded();
        else if (what == "charges") charges();
        else { fprintf(stderr, "topology_host: unknown case %s\n", what.c_str()); return 2; }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
