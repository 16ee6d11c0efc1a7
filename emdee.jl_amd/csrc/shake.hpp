// shake.hpp -- bonds to hydrogen held at fixed lengths (emdee_md_set_hbonds): star clusters of a centre and one, two or three
// satellites (X-H, XH2, XH3), every satellite at a fixed distance from the centre, no constraint between satellites.  The
// position stage is SHAKE in matrix form (M-SHAKE: Kraeutler, van Gunsteren & Huenenberger, J. Comput. Chem. 22, 501 (2001)):
// Newton's method on the n coupled equations, the n x n system solved directly; the velocity stage is RATTLE (Andersen, J.
// Comput. Phys. 52, 24 (1983)): one symmetric linear solve.  The two functions at the top are plain C++ on fixed-size arrays of
// doubles, as the top of settle.hpp is: a stand-alone host program tests them with the host compiler (tests/c/shake_host.cpp);
// the group policy below them (Star: how settle.hpp's constraint kernels take a cluster) needs HIP.
// Sites: 0 = the centre, 1..3 = the satellites; w: the inverse masses; n: how many satellites are in use (1..3).  Both functions
// are written for three satellites with compile-time loops: a slot k >= n becomes an identity row with a zero right-hand side,
// a zero bond vector and w = 0, so nothing is indexed at run time (a run-time index put a struct in scratch once).
#pragma once

#include "settle.hpp"

namespace emdee {

// The position stage stops when every | |r_k|^2 - d_k^2 | <= SHAKE_TOL d_k^2, or fails after SHAKE_MAX_ITER Newton steps.
// |r|^2 - d^2 is a difference of two numbers near d^2, each rounded at eps d^2 / 2, and |r|^2 a sum of three such products: its
// floor in fp64 is a few eps d^2 (eps = 2.2e-16).  4e-15 is 18 eps: above the floor, so that a converged cluster never spends
// iterations on rounding noise, and a relative distance error of 2e-15, 500 times below the 1e-12 the tests ask for.  Newton
// from lambda = 0 converges quadratically: displacements of 10 % of d take at most 5 steps (tests/test_shake_host.py prints the
// worst count it sees); 32 is reached only where no solution is near.
constexpr double SHAKE_TOL = 4e-15;
constexpr int SHAKE_MAX_ITER = 32;

namespace shake_detail {
// s = A^-1 r for a general 3 x 3 matrix (cofactors, as settle_detail::solve3; A is not symmetric here).  False when the
// determinant is zero or not finite.
EMDEE_HD bool solve3g(const double (&a)[3][3], const double (&r)[3], double (&s)[3]) {
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double c10 = a[0][2] * a[2][1] - a[0][1] * a[2][2], c11 = a[0][0] * a[2][2] - a[0][2] * a[2][0], c12 = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    const double c20 = a[0][1] * a[1][2] - a[0][2] * a[1][1], c21 = a[0][2] * a[1][0] - a[0][0] * a[1][2], c22 = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
    if (!(fabs(det) > 0.0) || !(fabs(det) < INFINITY)) return false;
    const double idet = 1.0 / det;
    s[0] = (c00 * r[0] + c10 * r[1] + c20 * r[2]) * idet;
    s[1] = (c01 * r[0] + c11 * r[1] + c21 * r[2]) * idet;
    s[2] = (c02 * r[0] + c12 * r[1] + c22 * r[2]) * idet;
    return true;
}
}  // namespace shake_detail

// x0: the sites where they satisfy the constraints (before the step); x1: where the unconstrained step put them.  Both are
// unwrapped and in one frame, whichever.  With e_k = x0_c - x0_k and r_k = x1_c - x1_k, x1 becomes x1_c + w_c sum_j lambda_j e_j
// and x1_k - w_k lambda_k e_k, lambda the solution of g_k = |r_k + w_c sum_j lambda_j e_j + w_k lambda_k e_k|^2 - d_k^2 = 0 that
// Newton's method reaches from lambda = 0 (Jacobian J_kj = 2 r'_k . (w_c e_j + delta_kj w_k e_k)).  Returns false, with x1
// untouched, when SHAKE_MAX_ITER steps do not reach SHAKE_TOL, when the Jacobian is singular or when anything is not finite: the
// sites have moved too far for the bonds of x0 to bring them back (SETTLE's negative radicand).  iterations: the Newton steps
// taken, if asked for.
EMDEE_HD bool shake_positions(const double (&x0)[4][3], double (&x1)[4][3], const double (&w)[4], const double (&dist)[3], int n,
                              int *iterations = nullptr) {
    double e[3][3], r[3][3], wk[3], d2[3];
    for (int k = 0; k < 3; k++) {
        const bool on = k < n;
        for (int c = 0; c < 3; c++) {
            e[k][c] = on ? x0[0][c] - x0[k + 1][c] : 0.0;
            r[k][c] = on ? x1[0][c] - x1[k + 1][c] : 0.0;
        }
        wk[k] = on ? w[k + 1] : 0.0;
        d2[k] = on ? dist[k] * dist[k] : 1.0;
    }
    const double wc = w[0];
    double lam[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
    bool done = false;
    int it = 0;
    for (;; it++) {
        double rp[3][3], g[3];
        for (int c = 0; c < 3; c++) s[c] = wc * (lam[0] * e[0][c] + lam[1] * e[1][c] + lam[2] * e[2][c]);
        done = true;
        for (int k = 0; k < 3; k++) {
            for (int c = 0; c < 3; c++) rp[k][c] = r[k][c] + s[c] + wk[k] * lam[k] * e[k][c];
            g[k] = k < n ? rp[k][0] * rp[k][0] + rp[k][1] * rp[k][1] + rp[k][2] * rp[k][2] - d2[k] : 0.0;
            done = done && fabs(g[k]) <= SHAKE_TOL * d2[k];   // (false for a NaN)
        }
        if (done || it == SHAKE_MAX_ITER) break;
        double J[3][3], rhs[3], dl[3];
        for (int k = 0; k < 3; k++) {
            for (int j = 0; j < 3; j++) {
                const double own = k == j ? wk[k] : 0.0;
                J[k][j] = k < n ? 2.0 * (wc + own) * (rp[k][0] * e[j][0] + rp[k][1] * e[j][1] + rp[k][2] * e[j][2]) : (k == j ? 1.0 : 0.0);
            }
            rhs[k] = -g[k];
        }
        if (!shake_detail::solve3g(J, rhs, dl)) return false;
        for (int k = 0; k < 3; k++) lam[k] += dl[k];
    }
    if (iterations) *iterations = it;
    if (!done) return false;
    for (int c = 0; c < 3; c++) {
        x1[0][c] += s[c];
        for (int k = 0; k < 3; k++)
            if (k < n) x1[k + 1][c] -= wk[k] * lam[k] * e[k][c];
    }
    return true;
}

// x: the sites (unwrapped, one frame); v: their velocities.  v becomes v_c + w_c sum_j mu_j r_j and v_k - w_k mu_k r_k, r_k = x_c -
// x_k, with the mu that leave no relative velocity along any bond: sum_j A_kj mu_j = -(v_c - v_k) . r_k, A_kj = w_c r_k . r_j +
// delta_kj w_k r_k . r_k, symmetric.  The solve is applied twice, as settle_velocities applies its own.
EMDEE_HD void shake_velocities(const double (&x)[4][3], double (&v)[4][3], const double (&w)[4], int n) {
    double r[3][3], wk[3];
    for (int k = 0; k < 3; k++) {
        const bool on = k < n;
        for (int c = 0; c < 3; c++) r[k][c] = on ? x[0][c] - x[k + 1][c] : 0.0;
        wk[k] = on ? w[k + 1] : 0.0;
    }
    const double wc = w[0];
    double a[3][3];
    for (int k = 0; k < 3; k++)
        for (int j = k; j < 3; j++) {
            const double dot = r[k][0] * r[j][0] + r[k][1] * r[j][1] + r[k][2] * r[j][2];
            a[k][j] = k < n ? (k == j ? (wc + wk[k]) * dot : wc * dot) : (k == j ? 1.0 : 0.0);
        }
    for (int pass = 0; pass < 2; pass++) {
        double rhs[3], mu[3];
        for (int k = 0; k < 3; k++) {
            rhs[k] = 0.0;
            if (k < n)
                for (int c = 0; c < 3; c++) rhs[k] -= (v[0][c] - v[k + 1][c]) * r[k][c];
        }
        settle_detail::solve3(a[0][0], a[0][1], a[0][2], a[1][1], a[1][2], a[2][2], rhs, mu);
        for (int c = 0; c < 3; c++) {
            v[0][c] += wc * (mu[0] * r[0][c] + mu[1] * r[1][c] + mu[2] * r[2][c]);
            for (int k = 0; k < 3; k++)
                if (k < n) v[k + 1][c] -= wk[k] * mu[k] * r[k][c];
        }
    }
}

}  // namespace emdee

#if defined(__HIPCC__)

namespace emdee {

// the star cluster as a group policy of settle.hpp's constraint kernels: atoms = {centre, s1, s2, s3} caller ids per cluster with
// -1 in the unused trailing slots, geom = the three distances; M-SHAKE and RATTLE take the inverse masses of the four sites
struct Star {
    static constexpr int SITES = 4, GEOM = 3;
    // the slots of cluster m's atoms (an unused site gets the centre's slot: never written, read for nothing) and the satellites in use
    template <typename real>
    static __device__ __forceinline__ int slots(const ConstraintArgs<real> &a, int m, int (&p)[4]) {
        const int4 id = *reinterpret_cast<const int4 *>(a.atoms + 4 * (size_t)m);
        p[0] = a.inv_perm[id.x];
        p[1] = a.inv_perm[id.y];
        p[2] = id.z >= 0 ? a.inv_perm[id.z] : p[0];
        p[3] = id.w >= 0 ? a.inv_perm[id.w] : p[0];
        return 1 + (id.z >= 0 ? 1 : 0) + (id.w >= 0 ? 1 : 0);
    }
    template <typename real>
    static __device__ __forceinline__ void inverse_masses(const ConstraintArgs<real> &a, const int (&p)[4], double (&w)[4]) {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = a.inv_mass ? (double)a.inv_mass[p[k]] : 1.0;
    }
    template <typename real>
    static __device__ __forceinline__ bool positions(const ConstraintArgs<real> &a, int m, const int (&p)[4], int n, const double (&x0)[4][3],
                                                     double (&x1)[4][3]) {
        double w[4], dist[3];
        inverse_masses(a, p, w);
#pragma unroll
        for (int k = 0; k < 3; k++) dist[k] = a.geom[3 * (size_t)m + k];
        return shake_positions(x0, x1, w, dist, n);
    }
    template <typename real>
    static __device__ __forceinline__ void velocities(const ConstraintArgs<real> &a, const int (&p)[4], int n, const double (&x)[4][3],
                                                      double (&v)[4][3]) {
        double w[4];
        inverse_masses(a, p, w);
        shake_velocities(x, v, w, n);
    }
    // *word = a cluster + 1 with a distance more than 1e-3 (relative) off its table entry (the highest such cluster): a wrong
    // topology, not rounding
    template <typename real>
    static __device__ __forceinline__ void check(const ConstraintArgs<real> &a, int m, const int (&)[4], int n, const double (&x)[4][3],
                                                 int *__restrict__ word) {
        bool off = false;
#pragma unroll
        for (int k = 1; k < 4; k++) {
            if (k > n) continue;
            const double d = a.geom[3 * (size_t)m + k - 1];
            const double l = sqrt(x[k][0] * x[k][0] + x[k][1] * x[k][1] + x[k][2] * x[k][2]);
            off = off || !(fabs(l - d) <= 1e-3 * d);
        }
        if (off) atomicMax(word, m + 1);
    }
};

}  // namespace emdee
#endif
