// thermostat_host.cpp -- the scalar rules of the global thermostats, alone: csrc/thermostat.hpp (plain C++ there).  Reads one case
// from stdin and prints lines of numbers ("%.17g").  tests/test_thermostat_host.py compiles this with the host compiler under ASan
// and UBSan and compares with tests/helpers/thermostat_ref.py.
//   alpha2 <n> then per row: K n_dof c R1 S (Kbar = n_dof / 2: kT = 1)   -> "alpha2" per row
//   draws <seed> <first> <n> <n_dof>                                     -> "R1 S" per step first .. first + n - 1
//   moments <seed> <n> <n_dof>                                           -> "mean(R1) var(R1) mean(S) var(S)" over steps 1 .. n
//   chain <K> <n_dof> <kT> <tau> <Delta> <M> then xi x M, vxi x M        -> "alpha E_th", then xi x M, then vxi x M
//   ensemble <seed> <n_osc> <steps> <dt> <kT> <tau>                      -> "K" after every step
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/thermostat.hpp"

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "thermostat_host: input ends early\n"); exit(2); }
    return t;
}
static long long integer() { return strtoll(token().c_str(), nullptr, 10); }
static unsigned long long counter() { return strtoull(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }   // (takes "nan" and "inf")

static void alpha2() {
    const long long n = integer();
    for (long long k = 0; k < n; k++) {
        const double K = number(), n_dof = number(), c = number(), R1 = number(), S = number();
        printf("%.17g\n", vrescale_alpha2(K, n_dof, c, 0.5 * n_dof, R1, S));
    }
}

static void draws() {
    const unsigned long long seed = counter(), first = counter();
    const long long n = integer(), n_dof = integer();
    for (long long k = 0; k < n; k++) {
        double r[2];
        th_draws(seed, first + (unsigned long long)k, n_dof, r);
        printf("%.17g %.17g\n", r[0], r[1]);
    }
}

static void moments() {
    const unsigned long long seed = counter();
    const long long n = integer(), n_dof = integer();
    std::vector<double> a((size_t)n), b((size_t)n);
    double ma = 0.0, mb = 0.0, va = 0.0, vb = 0.0;
    for (long long k = 0; k < n; k++) {
        double r[2];
        th_draws(seed, (unsigned long long)(k + 1), n_dof, r);
        a[(size_t)k] = r[0]; b[(size_t)k] = r[1];
        ma += r[0]; mb += r[1];
    }
    ma /= (double)n; mb /= (double)n;
    for (long long k = 0; k < n; k++) { va += (a[(size_t)k] - ma) * (a[(size_t)k] - ma); vb += (b[(size_t)k] - mb) * (b[(size_t)k] - mb); }
    printf("%.17g %.17g %.17g %.17g\n", ma, va / (double)(n - 1), mb, vb / (double)(n - 1));
}

static void chain() {
    const double K = number(), n_dof = number(), kT = number(), tau = number(), Delta = number();
    const long long M = integer();
    if (M < 1 || M > TH_CHAIN_MAX) { fprintf(stderr, "thermostat_host: chain length %lld\n", M); exit(2); }
    double xi[TH_CHAIN_MAX] = {0}, vxi[TH_CHAIN_MAX] = {0};
    for (long long k = 0; k < M; k++) xi[k] = number();
    for (long long k = 0; k < M; k++) vxi[k] = number();
    const double alpha = nhc_step(K, n_dof, kT, tau, Delta, (int)M, xi, vxi);
    printf("%.17g %.17g\n", alpha, nhc_energy(n_dof, kT, tau, (int)M, xi, vxi));
    for (long long k = 0; k < M; k++) printf("%.17g%c", xi[k], k + 1 < M ? ' ' : '\n');
    for (long long k = 0; k < M; k++) printf("%.17g%c", vxi[k], k + 1 < M ? ' ' : '\n');
}

// n_osc uncoupled unit-mass oscillators in one dimension with frequencies spread over [1, 2], velocity Verlet, a v-rescale event
// after every step through thermostat_update (n_dof = n_osc: nothing is conserved but the energy)
static void ensemble() {
    const unsigned long long seed = counter();
    const long long n_osc = integer(), steps = integer();
    const double dt = number(), kT = number(), tau = number();
    std::vector<double> x((size_t)n_osc), v((size_t)n_osc), w2((size_t)n_osc);
    for (long long i = 0; i < n_osc; i++) {
        const double w = 1.0 + (double)i / (double)n_osc;
        w2[(size_t)i] = w * w;
        x[(size_t)i] = 0.0;
        v[(size_t)i] = (i % 2 ? -1.0 : 1.0) * sqrt(kT);
    }
    double words[TH_WORDS] = {0};
    ThermostatParams p{};
    p.kind = TH_VRESCALE; p.chain = 0; p.kT = kT; p.tau = tau; p.Delta = dt; p.n_dof = (double)n_osc; p.seed = seed;
    for (long long s = 1; s <= steps; s++) {
        double K = 0.0;
        for (long long i = 0; i < n_osc; i++) {
            const size_t k = (size_t)i;
            v[k] -= 0.5 * dt * w2[k] * x[k];
            x[k] += dt * v[k];
            v[k] -= 0.5 * dt * w2[k] * x[k];
            K += 0.5 * v[k] * v[k];
        }
        p.step = (unsigned long long)s;
        const double alpha = thermostat_update(p, K, words);
        for (long long i = 0; i < n_osc; i++) v[(size_t)i] *= alpha;
        printf("%.17g\n", alpha * alpha * K);
    }
}

int main() {
    const std::string what = token();
    if (what == "alpha2") alpha2();
    else if (what == "draws") draws();
    else if (what == "moments") moments();
    else if (what == "chain") chain();
    else if (what == "ensemble") ensemble();
    else { fprintf(stderr, "thermostat_host: unknown case %s\n", what.c_str()); return 2; }
    return 0;
}
