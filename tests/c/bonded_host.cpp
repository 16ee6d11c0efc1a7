// bonded_host.cpp -- the formula of the bonded terms, alone: bonded_term of csrc/bonded.hpp (plain C++ there, the function
// k_bonded calls on the device) instantiated for float and for double.  Reads one batch from stdin and prints one line per term.
// tests/test_bonded_terms_host.py compiles this with the host compiler under ASan and UBSan and compares with
// tests/helpers/bonded_ref.py in a wider format.
//   <float|double> <n> then per term: kind u (12: four atoms, the unused ones ignored) p0 p1 p2
//       -> "U F (12)" per term, "%.17g" (a float prints exactly)
// The numbers go in as decimal text read as double and, for float, rounded once to float: the test sends values that are
// floats already.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../emdee.jl_amd/csrc/bonded.hpp"

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "bonded_host: input ends early\n"); exit(2); }
    return t;
}
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan", "inf" and denormals)

template <typename real>
static void batch(long n) {
    for (long t = 0; t < n; t++) {
        const int kind = (int)strtol(token().c_str(), nullptr, 10);
        if (kind < 1 || kind > 3) { fprintf(stderr, "bonded_host: kind %d\n", kind); exit(2); }
        real u[4][3], F[4][3];
        for (int a = 0; a < 4; a++)
            for (int c = 0; c < 3; c++) { u[a][c] = (real)number(); F[a][c] = (real)-77; }
        const real p0 = (real)number(), p1 = (real)number(), p2 = (real)number();
        const real U = emdee::bonded_term<real>(kind, u, p0, p1, p2, F);
        printf("%.17g", (double)U);
        for (int a = 0; a < 4; a++)
            for (int c = 0; c < 3; c++) printf(" %.17g", (double)F[a][c]);
        printf("\n");
    }
}

int main() {
    std::ios::sync_with_stdio(false);
    const std::string type = token();
    const long n = strtol(token().c_str(), nullptr, 10);
    if (type == "float") batch<float>(n);
    else if (type == "double") batch<double>(n);
    else { fprintf(stderr, "bonded_host: unknown type %s\n", type.c_str()); return 2; }
    return 0;
}
