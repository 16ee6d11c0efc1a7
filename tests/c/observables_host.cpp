// observables_host.cpp -- the part of csrc/observables.hpp with no HIP in it, alone: the gate the entries of the three observables
// pass a table and the engine's facts through.  Reads one case from stdin and prints "OK", or "REFUSED <code> <message>" for a
// case the gate refuses.  tests/test_observables_host.py compiles this with the host compiler under ASan and UBSan and holds the
// messages against the ones recorded from the library (tests/golden/observable_refusal_texts.json).
//   present <kind> <verb> <present>
//   fit <kind> <table: n_atoms serial len x 3> <engine: lent has_ghosts sorted id_gaps n_owned n_ghost serial len x 3>
//   whole_box <fn> <engine: as above>
//   groups <kind> <n_groups> <n> {group} x n
// kind: 0 rdf, 1 msd, 2 gk
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/observables.hpp"

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
    if (!(std::cin >> t)) { fprintf(stderr, "observables_host: input ends early\n"); exit(2); }
    return t;
}
static long long integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }
static ObsKind kind() {
    const long long k = integer();
    if (k < 0 || k > 2) { fprintf(stderr, "observables_host: unknown kind\n"); exit(2); }
    return (ObsKind)k;
}
static ObsEngine engine() {
    ObsEngine e{};
    e.lent = integer() != 0; e.has_ghosts = integer() != 0; e.sorted = integer() != 0; e.id_gaps = integer() != 0;
    e.n_owned = (int)integer(); e.n_ghost = (int)integer(); e.state_serial = (uint64_t)integer();
    for (double &l : e.len) l = number();
    return e;
}

static void run(const std::string &what) {
    if (what == "present") {
        const ObsKind k = kind();
        const std::string verb = token();
        ObsTable t;
        t.present = integer() != 0;
        obs_require_present(k, verb.c_str(), t);
    } else if (what == "fit") {
        const ObsKind k = kind();
        ObsTable t;
        t.present = true; t.n_atoms = (int)integer(); t.serial = (uint64_t)integer();
        for (double &l : t.len) l = number();
        obs_require_fit(k, t, engine());
    } else if (what == "whole_box") {
        const std::string fn = token();
        obs_require_whole_box(fn.c_str(), engine());
    } else if (what == "groups") {
        const ObsKind k = kind();
        const int n_groups = (int)integer();
        std::vector<int32_t> g((size_t)integer());
        for (int32_t &x : g) x = (int32_t)integer();
        obs_check_groups(k, g.data(), (int)g.size(), n_groups);
    } else {
        fprintf(stderr, "observables_host: unknown case %s\n", what.c_str());
        exit(2);
    }
}

int main() {
    try {
        run(token());
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", (int)f.code, get_error());
        return 0;
    }
    printf("OK\n");
    return 0;
}
