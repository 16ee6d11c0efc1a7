// thermostat.hpp -- global thermostats (emdee_md_set_thermostat): stochastic velocity rescaling (Bussi, Donadio & Parrinello,
// J. Chem. Phys. 126, 014101 (2007)) and a Nose-Hoover chain (Martyna, Tuckerman, Tobias & Klein, Mol. Phys. 87, 1117 (1996)).
// Both reduce the kinetic energy K, update a few scalars and multiply every velocity by one factor alpha.  The scalar rules at the
// top are plain C++ on doubles, as the tops of settle.hpp, shake.hpp and minimize.hpp are: a stand-alone host program tests them
// with the host compiler (tests/c/thermostat_host.cpp); the kernels below them need HIP.  DESIGN.md 4f has the algorithm;
// MdImpl::thermostat_event (impl.hpp) queues the three kernels of an event.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int TH_OFF = 0, TH_VRESCALE = 1, TH_NOSE_HOOVER = 2;
constexpr int TH_CHAIN_MAX = 8;
// the state words of emdee_md_thermostat_state
constexpr int TH_NDOF = 0, TH_K = 1, TH_ALPHA = 2, TH_ETH = 3, TH_XI = 4, TH_VXI = 12, TH_WORDS = 20;
constexpr int TH_GAMMA_ATTEMPTS = 64;

// ---- the counter generator: the integer arithmetic of the Langevin noise (kernels.hpp lgv_mix, lgv_normals) on (seed, step, id)
EMDEE_HD unsigned long long th_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// one N(0,1) number (component 0 of lgv_normals) and one uniform number in (0, 1] that does not share a counter with it
EMDEE_HD void th_normal_uniform(unsigned long long seed, unsigned long long step, long long id, double *normal, double *uniform) {
    const unsigned long long base = th_mix(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)id);
    const unsigned long long s2 = th_mix(base ^ (0xD1B54A32D192ED03ull * (step + 1)));
    const unsigned long long r0 = th_mix(s2 + 0x9E3779B97F4A7C15ull), r1 = th_mix(s2 + 0x9E3779B97F4A7C15ull * 2ull),
                             r2 = th_mix(s2 + 0x9E3779B97F4A7C15ull * 3ull);
    const double two53 = 1.0 / 9007199254740992.0, twopi = 6.283185307179586476925286766559;
    const double u1 = (double)((r0 >> 11) + 1) * two53, v2 = (double)(r1 >> 11) * two53;
    *normal = sqrt(-2.0 * log(u1)) * cos(twopi * v2);
    *uniform = (double)((r2 >> 11) + 1) * two53;
}
// Gamma(a), a > 0, by Marsaglia & Tsang (ACM Trans. Math. Softw. 26, 363 (2000)): attempt j takes its normal and its uniform from
// id = -3 - j.  The loop is capped; acceptance is above 95 % per attempt, so the cap is not reached in practice, and on
// exhaustion the mean is returned.  a < 1: Gamma(a + 1) U^(1/a), U from id = -2 (whose normal is R1).
EMDEE_HD double th_gamma(unsigned long long seed, unsigned long long step, double a) {
    double boost = 1.0;
    if (a < 1.0) {
        double x, u;
        th_normal_uniform(seed, step, -2, &x, &u);
        boost = pow(u, 1.0 / a);
        a += 1.0;
    }
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (int j = 0; j < TH_GAMMA_ATTEMPTS; j++) {
        double x, u;
        th_normal_uniform(seed, step, -3 - (long long)j, &x, &u);
        const double t = 1.0 + c * x;
        if (t <= 0.0) continue;
        const double v = t * t * t;
        if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) return boost * d * v;
    }
    return boost * a;
}
// the two draws of a v-rescale event: out[0] = R1, N(0,1); out[1] = S, chi-squared with n_dof - 1 degrees of freedom
EMDEE_HD void th_draws(unsigned long long seed, unsigned long long step, long long n_dof, double out[2]) {
    double u;
    th_normal_uniform(seed, step, -2, &out[0], &u);
    out[1] = n_dof > 1 ? 2.0 * th_gamma(seed, step, 0.5 * (double)(n_dof - 1)) : 0.0;
}

// ---- stochastic velocity rescaling: alpha^2 for the kinetic energy K, c = exp(-Delta / tau), the target Kbar = n_dof kT / 2
EMDEE_HD double vrescale_alpha2(double K, double n_dof, double c, double Kbar, double R1, double S) {
    if (!(K > 0.0)) return 1.0;
    const double q = (1.0 - c) * Kbar / (n_dof * K);
    const double a2 = c + q * (S + R1 * R1) + 2.0 * R1 * sqrt(c * q);
    return a2 > 0.0 ? a2 : 0.0;
}

// ---- Nose-Hoover chain: xi[0..M), vxi[0..M) in place over Delta for the kinetic energy K; returns alpha.
// Q_1 = n_dof kT tau^2, Q_k = kT tau^2.  One pass of the MTK factorisation advances the chain and the scale by Delta / 2 (the
// kicks of its two sweeps are Delta / 4 each, its scale and drift Delta / 2); two passes make the Delta of an event, each with
// the kinetic energy the pass before it left.  Every pass is a palindrome of maps that each invert with -Delta, so nhc_step(Delta)
// followed by nhc_step(-Delta) restores the state to rounding.
EMDEE_HD void nhc_kick(double *vxi, int k, int M, double K, double n_dof, double kT, double Q1, double Qk, double Delta) {
    const double e = k + 1 < M ? exp(-0.125 * Delta * vxi[k + 1]) : 1.0;
    const double G = k == 0 ? (2.0 * K - n_dof * kT) / Q1 : ((k == 1 ? Q1 : Qk) * vxi[k - 1] * vxi[k - 1] - kT) / Qk;
    vxi[k] = (vxi[k] * e + 0.25 * Delta * G) * e;
}
EMDEE_HD double nhc_step(double K, double n_dof, double kT, double tau, double Delta, int M, double *xi, double *vxi) {
    const double Q1 = n_dof * kT * tau * tau, Qk = kT * tau * tau;
    double alpha = 1.0;
    for (int pass = 0; pass < 2; pass++) {
        for (int k = M - 1; k >= 0; k--) nhc_kick(vxi, k, M, K, n_dof, kT, Q1, Qk, Delta);
        const double s = exp(-0.5 * Delta * vxi[0]);
        alpha *= s;
        K *= s * s;
        for (int k = 0; k < M; k++) xi[k] += 0.5 * Delta * vxi[k];
        for (int k = 0; k < M; k++) nhc_kick(vxi, k, M, K, n_dof, kT, Q1, Qk, Delta);
    }
    return alpha;
}
EMDEE_HD double nhc_energy(double n_dof, double kT, double tau, int M, const double *xi, const double *vxi) {
    const double Q1 = n_dof * kT * tau * tau, Qk = kT * tau * tau;
    double e = 0.0;
    for (int k = 0; k < M; k++) e += 0.5 * (k == 0 ? Q1 : Qk) * vxi[k] * vxi[k] + (k == 0 ? n_dof : 1.0) * kT * xi[k];
    return e;
}

// what an event needs besides K
struct ThermostatParams {
    int kind, chain;
    double kT, tau, Delta, n_dof;
    unsigned long long seed, step;                           // step: the count the event completes, numbered from first_step
};
// one event on the state words: K as the event sees it; words 0..19 are updated, alpha is returned
EMDEE_HD double thermostat_update(const ThermostatParams &p, double K, double *w) {
    double alpha = 1.0;
    if (p.kind == TH_VRESCALE) {
        double r[2];
        th_draws(p.seed, p.step, (long long)p.n_dof, r);
        const double a2 = vrescale_alpha2(K, p.n_dof, exp(-p.Delta / p.tau), 0.5 * p.n_dof * p.kT, r[0], r[1]);
        alpha = sqrt(a2);
        w[TH_ETH] -= (a2 - 1.0) * K;
    } else if (p.kind == TH_NOSE_HOOVER) {
        alpha = nhc_step(K, p.n_dof, p.kT, p.tau, p.Delta, p.chain, w + TH_XI, w + TH_VXI);
        w[TH_ETH] = nhc_energy(p.n_dof, p.kT, p.tau, p.chain, w + TH_XI, w + TH_VXI);
    }
    w[TH_NDOF] = p.n_dof;
    w[TH_K] = K;
    w[TH_ALPHA] = alpha;
    return alpha;
}

}  // namespace emdee

#if defined(__HIPCC__)

#include "reduce.hpp"

namespace emdee {

// The term of an event's K (reduce.hpp), over the owned slots, fp64 in both precisions: the sum of m v^2 / 2 (k_thermostat_update
// completes it)
template <typename real>
struct KineticSums {
    static constexpr int SUMS = 1, MAXES = 0;
    int n_owned;
    size_t pitch;
    const int *perm;
    const real *vel, *inv_mass;
    __device__ __forceinline__ void operator()(int p, double *s) const {
        if (perm[p] >= n_owned) return;
        const real im = inv_mass ? inv_mass[p] : (real)1;
        const double m = im != (real)0 ? 1.0 / (double)im : 0.0;   // (a massless atom, a virtual site: exactly 0)
        const double vx = (double)vel[p], vy = (double)vel[pitch + p], vz = (double)vel[2 * pitch + p];
        s[0] += 0.5 * m * (vx * vx + vy * vy + vz * vz);
    }
};

// one block: K as k_reduce_final would leave it, then thread 0 runs the scalar update on the state words w[0..19]
static __global__ __launch_bounds__(RED_BLOCK) void k_thermostat_update(int nblocks, const double *__restrict__ partial,
                                                                        ThermostatParams p, double *__restrict__ w) {
    __shared__ double sh[RED_BLOCK / WAVE];
    const double K = final_word(nblocks, partial, 1, 0, false, sh);
    if (threadIdx.x == 0) thermostat_update(p, K, w);
}

// v <- alpha v on every owned slot, alpha from the state words; fp64 product in both precisions
template <typename real>
__global__ __launch_bounds__(256) void k_scale_velocities(int n, int n_owned, size_t pitch, const int *__restrict__ perm,
                                                          real *__restrict__ vel, const double *__restrict__ w) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    const double alpha = w[TH_ALPHA];
    vel[p] = (real)((double)vel[p] * alpha);
    vel[pitch + p] = (real)((double)vel[pitch + p] * alpha);
    vel[2 * pitch + p] = (real)((double)vel[2 * pitch + p] * alpha);
}

// emdee_md_thermostat_draws: th_draws in one thread
static __global__ void k_thermostat_draws(unsigned long long seed, unsigned long long step, long long n_dof, double *__restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) th_draws(seed, step, n_dof, out);
}

}  // namespace emdee
#endif
