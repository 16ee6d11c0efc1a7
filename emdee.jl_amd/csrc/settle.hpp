// settle.hpp -- rigid three-site molecules (emdee_md_set_rigid3): the closed-form position stage (SETTLE: Miyamoto & Kollman,
// J. Comput. Chem. 13, 952 (1992)) and the velocity stage (RATTLE for a triangle: one 3 x 3 linear solve), the group policy
// (Triangle) that hands them to the constraint kernels, and those kernels, written here once for every kind of group (shake.hpp
// adds the Star).  The two functions at the top are plain C++ on fixed-size arrays of doubles: a stand-alone host program tests
// them with the host compiler (tests/c/settle_host.cpp); the kernels below them need HIP.
// Sites: 0 = apex, 1 and 2 = the legs a and b, |0 - 1| = |0 - 2| = d_leg, |1 - 2| = d_base; the legs have one mass.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

// x0: the three sites where they satisfy the constraints (before the step); x1: where the unconstrained step put them.  Both are
// unwrapped (differences between sites are the molecule's own, no box lengths in them) and in one frame, whichever.  x1 becomes
// the solution of the SHAKE equations -- x1 + sum over the three bonds of lambda_k (x0_i - x0_j) / m_i with the three distances
// restored -- in closed form.  The corrections lie in the plane of x0, leave the centre of mass where it is and exert no torque
// about the plane's normal; that fixes the three angles of the paper: phi and psi from the heights above the plane, theta from
// the torque balance.  Returns false, with x1 untouched, when a radicand is negative (or a length is zero or not a number): the
// sites have moved too far for a rigid triangle to reach them this way.
EMDEE_HD bool settle_positions(const double (&x0)[3][3], double (&x1)[3][3], double m_apex, double m_leg, double d_leg, double d_base) {
    const double mt = m_apex + 2.0 * m_leg;
    // the canonical triangle about its centre of mass: apex at (0, ra), legs at (-+rc, -rb)
    const double rc = 0.5 * d_base;
    const double h2 = d_leg * d_leg - rc * rc;
    if (!(h2 > 0.0) || !(mt > 0.0)) return false;
    const double h = sqrt(h2), ra = 2.0 * m_leg * h / mt, rb = h - ra;
    // b0, c0: the legs of x0 from its apex; a1, b1, c1: the sites of x1 from x1's centre of mass
    double b0[3], c0[3], com[3], a1[3], b1[3], c1[3];
    for (int d = 0; d < 3; d++) {
        b0[d] = x0[1][d] - x0[0][d]; c0[d] = x0[2][d] - x0[0][d];
        // (the centre of mass relative to x1's apex: differences of near numbers, not an average of far ones)
        const double pb = x1[1][d] - x1[0][d], pc = x1[2][d] - x1[0][d];
        com[d] = m_leg * (pb + pc) / mt;
        a1[d] = -com[d]; b1[d] = pb - com[d]; c1[d] = pc - com[d];
    }
    // the frame: Z normal to the plane of x0, X = a1 x Z, Y = Z x X
    double ez[3] = {b0[1] * c0[2] - b0[2] * c0[1], b0[2] * c0[0] - b0[0] * c0[2], b0[0] * c0[1] - b0[1] * c0[0]};
    double ex[3] = {a1[1] * ez[2] - a1[2] * ez[1], a1[2] * ez[0] - a1[0] * ez[2], a1[0] * ez[1] - a1[1] * ez[0]};
    double ey[3] = {ez[1] * ex[2] - ez[2] * ex[1], ez[2] * ex[0] - ez[0] * ex[2], ez[0] * ex[1] - ez[1] * ex[0]};
    const double lx2 = ex[0] * ex[0] + ex[1] * ex[1] + ex[2] * ex[2], ly2 = ey[0] * ey[0] + ey[1] * ey[1] + ey[2] * ey[2],
                 lz2 = ez[0] * ez[0] + ez[1] * ez[1] + ez[2] * ez[2];
    if (!(lx2 > 0.0) || !(ly2 > 0.0) || !(lz2 > 0.0) || !(lx2 < INFINITY) || !(ly2 < INFINITY)) return false;
    const double ix = 1.0 / sqrt(lx2), iy = 1.0 / sqrt(ly2), iz = 1.0 / sqrt(lz2);
    for (int d = 0; d < 3; d++) { ex[d] *= ix; ey[d] *= iy; ez[d] *= iz; }
    const double xb0 = ex[0] * b0[0] + ex[1] * b0[1] + ex[2] * b0[2], yb0 = ey[0] * b0[0] + ey[1] * b0[1] + ey[2] * b0[2];
    const double xc0 = ex[0] * c0[0] + ex[1] * c0[1] + ex[2] * c0[2], yc0 = ey[0] * c0[0] + ey[1] * c0[1] + ey[2] * c0[2];
    const double za1 = ez[0] * a1[0] + ez[1] * a1[1] + ez[2] * a1[2];
    const double xb1 = ex[0] * b1[0] + ex[1] * b1[1] + ex[2] * b1[2], yb1 = ey[0] * b1[0] + ey[1] * b1[1] + ey[2] * b1[2],
                 zb1 = ez[0] * b1[0] + ez[1] * b1[1] + ez[2] * b1[2];
    const double xc1 = ex[0] * c1[0] + ex[1] * c1[1] + ex[2] * c1[2], yc1 = ey[0] * c1[0] + ey[1] * c1[1] + ey[2] * c1[2],
                 zc1 = ez[0] * c1[0] + ez[1] * c1[1] + ez[2] * c1[2];
    // phi, psi: the tilt that gives the canonical triangle the heights of x1 above the plane
    const double sinphi = za1 / ra, cosphi2 = 1.0 - sinphi * sinphi;
    if (!(cosphi2 > 0.0)) return false;
    const double cosphi = sqrt(cosphi2);
    const double sinpsi = (zb1 - zc1) / (2.0 * rc * cosphi), cospsi2 = 1.0 - sinpsi * sinpsi;
    if (!(cospsi2 > 0.0)) return false;
    const double cospsi = sqrt(cospsi2);
    const double ya2 = ra * cosphi, xb2 = -rc * cospsi, yb2 = -rb * cosphi - rc * sinpsi * sinphi, yc2 = -rb * cosphi + rc * sinpsi * sinphi;
    // theta: the rotation about Z at which the corrections exert no torque
    const double alpha = xb2 * (xb0 - xc0) + yb0 * yb2 + yc0 * yc2;
    const double beta = xb2 * (yc0 - yb0) + xb0 * yb2 + xc0 * yc2;
    const double gamma = xb0 * yb1 - xb1 * yb0 + xc0 * yc1 - xc1 * yc0;
    const double a2b2 = alpha * alpha + beta * beta, rad = a2b2 - gamma * gamma;
    if (!(a2b2 > 0.0) || !(rad >= 0.0)) return false;
    const double sintheta = (alpha * gamma - beta * sqrt(rad)) / a2b2, costheta2 = 1.0 - sintheta * sintheta;
    if (!(costheta2 > 0.0)) return false;
    const double costheta = sqrt(costheta2);
    const double xa3 = -ya2 * sintheta, ya3 = ya2 * costheta;
    const double xb3 = xb2 * costheta - yb2 * sintheta, yb3 = xb2 * sintheta + yb2 * costheta;
    const double xc3 = -xb2 * costheta - yc2 * sintheta, yc3 = -xb2 * sintheta + yc2 * costheta;
    // back to the caller's frame: x1's apex + centre of mass + the site
    for (int d = 0; d < 3; d++) {
        const double o = x1[0][d] + com[d];
        x1[0][d] = o + (ex[d] * xa3 + ey[d] * ya3 + ez[d] * za1);
        x1[1][d] = o + (ex[d] * xb3 + ey[d] * yb3 + ez[d] * zb1);
        x1[2][d] = o + (ex[d] * xc3 + ey[d] * yc3 + ez[d] * zc1);
    }
    return true;
}

namespace settle_detail {
// s = A^-1 r for the symmetric 3 x 3 matrix {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}} (cofactors)
EMDEE_HD void solve3(double a00, double a01, double a02, double a11, double a12, double a22, const double (&r)[3], double (&s)[3]) {
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double idet = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
    s[0] = (c00 * r[0] + c01 * r[1] + c02 * r[2]) * idet;
    s[1] = (c01 * r[0] + c11 * r[1] + c12 * r[2]) * idet;
    s[2] = (c02 * r[0] + c12 * r[1] + c22 * r[2]) * idet;
}
}  // namespace settle_detail

// x: the three sites (unwrapped, one frame); v: their velocities.  v becomes v_i + sum over the bonds of lambda_k (x_i - x_j) / m_i
// with the lambdas that leave no relative velocity along any of the three bonds: three linear equations in three unknowns, solved
// directly.  The solve is applied a second time to what rounding left of the residuals (a fixed second pass, not an iteration to
// a tolerance): the velocities then satisfy the conditions to a few ulp whatever the mass ratio.
EMDEE_HD void settle_velocities(const double (&x)[3][3], double (&v)[3][3], double m_apex, double m_leg) {
    const double wa = 1.0 / m_apex, wl = 1.0 / m_leg;
    double e01[3], e02[3], e12[3];
    for (int d = 0; d < 3; d++) { e01[d] = x[0][d] - x[1][d]; e02[d] = x[0][d] - x[2][d]; e12[d] = x[1][d] - x[2][d]; }
    const double d0101 = e01[0] * e01[0] + e01[1] * e01[1] + e01[2] * e01[2], d0202 = e02[0] * e02[0] + e02[1] * e02[1] + e02[2] * e02[2],
                 d1212 = e12[0] * e12[0] + e12[1] * e12[1] + e12[2] * e12[2], d0102 = e01[0] * e02[0] + e01[1] * e02[1] + e01[2] * e02[2],
                 d0112 = e01[0] * e12[0] + e01[1] * e12[1] + e01[2] * e12[2], d0212 = e02[0] * e12[0] + e02[1] * e12[1] + e02[2] * e12[2];
    // unknowns (l01, l02, l12); rows: the bonds 0-1, 0-2, 1-2
    const double a00 = (wa + wl) * d0101, a01 = wa * d0102, a02 = -wl * d0112, a11 = (wa + wl) * d0202, a12 = wl * d0212, a22 = 2.0 * wl * d1212;
    for (int pass = 0; pass < 2; pass++) {
        double r[3] = {0.0, 0.0, 0.0}, l[3];
        for (int d = 0; d < 3; d++) {
            r[0] -= (v[0][d] - v[1][d]) * e01[d]; r[1] -= (v[0][d] - v[2][d]) * e02[d]; r[2] -= (v[1][d] - v[2][d]) * e12[d];
        }
        settle_detail::solve3(a00, a01, a02, a11, a12, a22, r, l);
        for (int d = 0; d < 3; d++) {
            v[0][d] += wa * (l[0] * e01[d] + l[1] * e02[d]);
            v[1][d] += wl * (l[2] * e12[d] - l[0] * e01[d]);
            v[2][d] -= wl * (l[1] * e02[d] + l[2] * e12[d]);
        }
    }
}

// ---- molecular pressure and centre-of-mass scaling (emdee_md_molecular_pressure_tensor, emdee_md_set_molecular_scaling) ------
// y: the three sites, unwrapped and in one frame, whichever; v: their velocities; f: the force-field forces on them (no constraint
// forces).  out[0..5] = sum_k 1/2 (d_k^a f_k^b + d_k^b f_k^a) with d_k = y_k - Y, out[6..11] = sum_k m_k v_k^a v_k^b - M V^a V^b,
// both in the order (xx, yy, zz, xy, xz, yz): what the molecule's atoms add to the atomic sums W and K beyond what its centre of
// mass carries.  Y and V are formed from differences to the apex (as settle_positions forms its centre of mass), and the kinetic
// term as sum_k m_k u_k^a u_k^b with u_k = v_k - V, which is the same number without the cancellation.
EMDEE_HD void molecule_sums(const double (&y)[3][3], const double (&v)[3][3], const double (&f)[3][3], double m_apex, double m_leg,
                            double (&out)[12]) {
    const double mt = m_apex + 2.0 * m_leg, m[3] = {m_apex, m_leg, m_leg};
    double d[3][3], u[3][3];
    for (int c = 0; c < 3; c++) {
        const double yb = y[1][c] - y[0][c], yc = y[2][c] - y[0][c], vb = v[1][c] - v[0][c], vc = v[2][c] - v[0][c];
        const double com = m_leg * (yb + yc) / mt, vcm = m_leg * (vb + vc) / mt;
        d[0][c] = -com; d[1][c] = yb - com; d[2][c] = yc - com;
        u[0][c] = -vcm; u[1][c] = vb - vcm; u[2][c] = vc - vcm;
    }
    const int ca[6] = {0, 1, 2, 0, 0, 1}, cb[6] = {0, 1, 2, 1, 2, 2};
    for (int q = 0; q < 6; q++) {
        const int a = ca[q], b = cb[q];
        double w = 0.0, k = 0.0;
        for (int s = 0; s < 3; s++) {
            w += 0.5 * (d[s][a] * f[s][b] + d[s][b] * f[s][a]);
            k += m[s] * u[s][a] * u[s][b];
        }
        out[q] = w; out[6 + q] = k;
    }
}

// The molecular scale of one molecule: y as above but in the frame of the box (lo is subtracted from its centre of mass), shift =
// (mu - 1) (Y - lo), what every site of the molecule moves by (a site whose record is another periodic image of y_k adds (mu - 1)
// times that whole number of box lengths itself), dv = (velocity_scale - 1) V, what every site's velocity gains: the centre of
// mass scales, its momentum scales, geometry and rotation are untouched.
EMDEE_HD void molecule_scale(const double (&y)[3][3], const double (&v)[3][3], double m_apex, double m_leg, const double (&mu)[3],
                             const double (&lo)[3], double velocity_scale, double (&shift)[3], double (&dv)[3]) {
    const double mt = m_apex + 2.0 * m_leg;
    for (int c = 0; c < 3; c++) {
        const double Y = y[0][c] + m_leg * ((y[1][c] - y[0][c]) + (y[2][c] - y[0][c])) / mt;
        const double V = v[0][c] + m_leg * ((v[1][c] - v[0][c]) + (v[2][c] - v[0][c])) / mt;
        shift[c] = (mu[c] - 1.0) * (Y - lo[c]);
        dv[c] = (velocity_scale - 1.0) * V;
    }
}

}  // namespace emdee

#if defined(__HIPCC__)
#include "kernels.hpp"

namespace emdee {

// the box as the constraint stages see it: fp64 lengths, whatever the engine's precision
struct SettleBox {
    double len[3];
    int per[3];
};
// A constraint table (Topology, topology_dev.hpp) and where the atoms are: n groups, atoms = the caller ids of every group's
// sites, geom = its distances, both as the group policy lays them out (Triangle below, Star in shake.hpp); an atom's slot comes
// from inv_perm, so nothing here depends on the sort and a re-sort between two stages is harmless.
template <typename real>
struct ConstraintArgs {
    int n;
    const int *atoms;
    const double *geom;
    const int *inv_perm;
    Rec<real> *rec;
    real *vel;
    const real *inv_mass;                                    // per slot, or NULL: every mass is 1
    size_t pitch;
    RelGrid rel;                                             // fp32: cell-relative records (their cells' origins are added in double)
    SettleBox box;
};

namespace settle_detail {
// the position a record stands for, in double: fp32 cell-relative records get their cell's origin (no box lengths: a record is
// continuous between two sorts, wrapped or not)
template <typename real>
__device__ __forceinline__ void site(const ConstraintArgs<real> &a, int p, double (&x)[3]) {
    const Rec<real> r = a.rec[p];
    x[0] = (double)r.x; x[1] = (double)r.y; x[2] = (double)r.z;
    if (sizeof(real) == 4 && a.rel.on) {
        double ox, oy, oz;
        a.rel.origin(a.rel.cell[p], ox, oy, oz);
        x[0] += ox; x[1] += oy; x[2] += oz;
    }
}
__device__ __forceinline__ double image(double d, double len, int periodic) { return periodic ? d - len * rint(d / len) : d; }
// the sites of a group as site 0 at the origin and the minimum images of the others from it
template <int S>
__device__ __forceinline__ void unwrap(const SettleBox &b, const double (&s)[S][3], double (&x)[S][3]) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
        x[0][d] = 0.0;
#pragma unroll
        for (int k = 1; k < S; k++) x[k][d] = image(s[k][d] - s[0][d], b.len[d], b.per[d]);
    }
}
template <typename real>
__device__ __forceinline__ void masses(const ConstraintArgs<real> &a, int p_apex, int p_leg, double &m_apex, double &m_leg) {
    m_apex = a.inv_mass ? 1.0 / (double)a.inv_mass[p_apex] : 1.0;
    m_leg = a.inv_mass ? 1.0 / (double)a.inv_mass[p_leg] : 1.0;
}
}  // namespace settle_detail

// ---- the constraint kernels: one thread per group, fp64 on unwrapped differences in both precisions, no atomics on the state.
// Written once for every kind of group; a group policy G carries what differs between kinds:
//   SITES, GEOM             sites per group (x0 holds 3 * SITES doubles per group) and doubles of geom per group
//   slots(a, m, p)          the slots of group m's sites; returns n, the last site in use (a site k > n reads site 0's slot and
//                           is never written)
//   positions(a, m, p, n, x0, x1), velocities(a, p, n, x, v)
//                           the plain-C++ solvers above (and in shake.hpp) with the masses and the geometry as each takes them
//   check(a, m, p, n, x, words)
//                           the test of a table entry against the loaded sites x (unwrapped about site 0)
// Every loop over sites is a compile-time loop over SITES and no array is indexed at run time.

// the rigid triangle: atoms = {apex, a, b}, geom = {d_leg, d_base}; SETTLE and RATTLE take the masses of the apex and of a leg
struct Triangle {
    static constexpr int SITES = 3, GEOM = 2;
    template <typename real>
    static __device__ __forceinline__ int slots(const ConstraintArgs<real> &a, int m, int (&p)[3]) {
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = a.inv_perm[a.atoms[3 * (size_t)m + k]];
        return 2;
    }
    template <typename real>
    static __device__ __forceinline__ bool positions(const ConstraintArgs<real> &a, int m, const int (&p)[3], int, const double (&x0)[3][3],
                                                     double (&x1)[3][3]) {
        double m_apex, m_leg;
        settle_detail::masses(a, p[0], p[1], m_apex, m_leg);
        return settle_positions(x0, x1, m_apex, m_leg, a.geom[2 * (size_t)m], a.geom[2 * (size_t)m + 1]);
    }
    template <typename real>
    static __device__ __forceinline__ void velocities(const ConstraintArgs<real> &a, const int (&p)[3], int, const double (&x)[3][3],
                                                      double (&v)[3][3]) {
        double m_apex, m_leg;
        settle_detail::masses(a, p[0], p[1], m_apex, m_leg);
        settle_velocities(x, v, m_apex, m_leg);
    }
    // words[0] = a molecule + 1 whose legs have different masses, words[1] = a molecule + 1 with a distance more than 1e-3
    // (relative) off its table entry; the highest such molecule each
    template <typename real>
    static __device__ __forceinline__ void check(const ConstraintArgs<real> &a, int m, const int (&p)[3], int, const double (&x)[3][3],
                                                 int *__restrict__ words) {
        if (a.inv_mass && a.inv_mass[p[1]] != a.inv_mass[p[2]]) atomicMax(words, m + 1);
        const double d_leg = a.geom[2 * (size_t)m], d_base = a.geom[2 * (size_t)m + 1];
        const double l1 = sqrt(x[1][0] * x[1][0] + x[1][1] * x[1][1] + x[1][2] * x[1][2]);
        const double l2 = sqrt(x[2][0] * x[2][0] + x[2][1] * x[2][1] + x[2][2] * x[2][2]);
        const double bx = x[1][0] - x[2][0], by = x[1][1] - x[2][1], bz = x[1][2] - x[2][2];
        const double l3 = sqrt(bx * bx + by * by + bz * bz);
        if (!(fabs(l1 - d_leg) <= 1e-3 * d_leg) || !(fabs(l2 - d_leg) <= 1e-3 * d_leg) || !(fabs(l3 - d_base) <= 1e-3 * d_base))
            atomicMax(words + 1, m + 1);
    }
};

// stage (a): the positions the groups have before the step, 3 * SITES doubles per group in table order (an unused site: site 0's)
template <typename real, class G>
__global__ __launch_bounds__(256) void k_constraint_gather(ConstraintArgs<real> a, double *__restrict__ x0) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n) return;
    int p[G::SITES];
    G::slots(a, m, p);
#pragma unroll
    for (int k = 0; k < G::SITES; k++) {
        double x[3];
        settle_detail::site(a, p[k], x);
#pragma unroll
        for (int d = 0; d < 3; d++) x0[3 * G::SITES * (size_t)m + 3 * k + d] = x[d];
    }
}

// stage (c): the records of the unconstrained step -> the group with its distances restored; v += (x_constrained -
// x_unconstrained) / dt; the group's atoms tested against the rebuild threshold again (k_kick_drift's test, on the corrected
// record).  A group without a solution stays as it is and its number + 1 goes to *err.
template <typename real, class G>
__global__ __launch_bounds__(256) void k_constraint_positions(ConstraintArgs<real> a, const double *__restrict__ x0, double inv_dt,
                                                              const real *__restrict__ xb, real thr2, int *__restrict__ flag,
                                                              int *__restrict__ err) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n) return;
    int p[G::SITES];
    const int n = G::slots(a, m, p);
    double s0[G::SITES][3], xa[G::SITES][3], xn[G::SITES][3], xs[G::SITES][3];
#pragma unroll
    for (int k = 0; k < G::SITES; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) s0[k][d] = x0[3 * G::SITES * (size_t)m + 3 * k + d];
    settle_detail::unwrap(a.box, s0, xa);
    // the unconstrained sites: x0 (unwrapped) + what each record moved since stage (a) (no sort in between: the same frame)
#pragma unroll
    for (int k = 0; k < G::SITES; k++) {
        double now[3];
        settle_detail::site(a, p[k], now);
#pragma unroll
        for (int d = 0; d < 3; d++) xs[k][d] = xn[k][d] = xa[k][d] + (now[d] - s0[k][d]);
    }
    if (!G::positions(a, m, p, n, xa, xs)) {
        atomicMax(err, m + 1);                               // (the failure path only; which group is named does not depend on the schedule)
        return;
    }
    bool far = false;
#pragma unroll
    for (int k = 0; k < G::SITES; k++) {
        if (k > n) continue;
        const double dx = xs[k][0] - xn[k][0], dy = xs[k][1] - xn[k][1], dz = xs[k][2] - xn[k][2];
        Rec<real> r = a.rec[p[k]];
        r.x = (real)((double)r.x + dx); r.y = (real)((double)r.y + dy); r.z = (real)((double)r.z + dz);
        a.rec[p[k]] = r;
        a.vel[p[k]] = (real)((double)a.vel[p[k]] + dx * inv_dt);
        a.vel[a.pitch + p[k]] = (real)((double)a.vel[a.pitch + p[k]] + dy * inv_dt);
        a.vel[2 * a.pitch + p[k]] = (real)((double)a.vel[2 * a.pitch + p[k]] + dz * inv_dt);
        const real ux = r.x - xb[p[k]], uy = r.y - xb[a.pitch + p[k]], uz = r.z - xb[2 * a.pitch + p[k]];
        far = far || ux * ux + uy * uy + uz * uz > thr2;
    }
    if (far) *flag = 1;
}

// stage (e): no relative velocity along any of the group's bonds
template <typename real, class G>
__global__ __launch_bounds__(256) void k_constraint_velocities(ConstraintArgs<real> a) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n) return;
    int p[G::SITES];
    const int n = G::slots(a, m, p);
    double s[G::SITES][3], x[G::SITES][3], v[G::SITES][3];
#pragma unroll
    for (int k = 0; k < G::SITES; k++) {
        settle_detail::site(a, p[k], s[k]);
#pragma unroll
        for (int d = 0; d < 3; d++) v[k][d] = (double)a.vel[d * a.pitch + p[k]];
    }
    settle_detail::unwrap(a.box, s, x);
    G::velocities(a, p, n, x, v);
#pragma unroll
    for (int k = 0; k < G::SITES; k++) {
        if (k > n) continue;
#pragma unroll
        for (int d = 0; d < 3; d++) a.vel[d * a.pitch + p[k]] = (real)v[k][d];
    }
}

// the check of a table against a loaded state: the policy's words, each the highest group + 1 that fails its test
template <typename real, class G>
__global__ __launch_bounds__(256) void k_constraint_check(ConstraintArgs<real> a, int *__restrict__ words) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n) return;
    int p[G::SITES];
    const int n = G::slots(a, m, p);
    double s[G::SITES][3], x[G::SITES][3];
#pragma unroll
    for (int k = 0; k < G::SITES; k++) settle_detail::site(a, p[k], s[k]);
    settle_detail::unwrap(a.box, s, x);
    G::check(a, m, p, n, x, words);
}

// ---- molecular pressure and centre-of-mass scaling: the two kernels (timed under emdee_md_kernel_time index 10) ----------------
// The sites of molecule m as the molecular definitions take them: s = the records in double (site()), y = the apex record and the
// minimum images of the legs from it, v the velocities; p the slots.
template <typename real>
__device__ __forceinline__ void molecule_load(const ConstraintArgs<real> &a, int m, int (&p)[3], double (&s)[3][3], double (&y)[3][3],
                                              double (&v)[3][3], double &m_apex, double &m_leg) {
    double x[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p[k] = a.inv_perm[a.atoms[3 * (size_t)m + k]];
        settle_detail::site(a, p[k], s[k]);
#pragma unroll
        for (int d = 0; d < 3; d++) v[k][d] = (double)a.vel[d * a.pitch + p[k]];
    }
    settle_detail::unwrap(a.box, s, x);
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) y[k][d] = s[0][d] + x[k][d];
    settle_detail::masses(a, p[0], p[1], m_apex, m_leg);
}

// The term of the molecular sums (reduce.hpp), over the molecules of the table: [0..11] = the sum of molecule_sums.  frc: the engine's
// force planes (the force-field forces of the last force pass).
template <typename real>
struct MoleculeSums {
    static constexpr int SUMS = TENSOR_SUMS, MAXES = 0;
    ConstraintArgs<real> a;
    const real *frc;
    __device__ __forceinline__ void operator()(int m, double *sum) const {
        int p[3];
        double s[3][3], y[3][3], v[3][3], f[3][3], m_apex, m_leg, t[TENSOR_SUMS];
        molecule_load(a, m, p, s, y, v, m_apex, m_leg);
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int d = 0; d < 3; d++) f[k][d] = (double)frc[d * a.pitch + p[k]];
        molecule_sums(y, v, f, m_apex, m_leg, t);
        for (int q = 0; q < TENSOR_SUMS; q++) sum[q] += t[q];
    }
};

// The molecular scale, one thread per molecule: every site's record moves by (mu - 1) (C_k - lo), C_k = Y + (r_k - y_k) the image
// of the centre of mass that goes with the record (r_k - y_k: whole box lengths, so the stored image counts stay valid); the
// shift is added to the record in its own frame in double and rounded once, as k_constraint_positions adds its corrections.
// scale_vel: v_k += (velocity_scale - 1) V; 0 leaves the velocity planes untouched, bit for bit.  k_cell_state_scale, given the
// membership bytes, leaves these atoms alone.
template <typename real>
__global__ __launch_bounds__(256) void k_molecule_scale(ConstraintArgs<real> a, ScaleBox sb, double velocity_scale, int scale_vel) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n) return;
    int p[3];
    double s[3][3], y[3][3], v[3][3], m_apex, m_leg, shift[3], dv[3];
    molecule_load(a, m, p, s, y, v, m_apex, m_leg);
    molecule_scale(y, v, m_apex, m_leg, sb.mu, sb.lo, velocity_scale, shift, dv);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        Rec<real> r = a.rec[p[k]];
        r.x = (real)((double)r.x + (shift[0] + (sb.mu[0] - 1.0) * (s[k][0] - y[k][0])));
        r.y = (real)((double)r.y + (shift[1] + (sb.mu[1] - 1.0) * (s[k][1] - y[k][1])));
        r.z = (real)((double)r.z + (shift[2] + (sb.mu[2] - 1.0) * (s[k][2] - y[k][2])));
        a.rec[p[k]] = r;
        if (scale_vel) {
#pragma unroll
            for (int d = 0; d < 3; d++) a.vel[d * a.pitch + p[k]] = (real)(v[k][d] + dv[d]);
        }
    }
}

}  // namespace emdee
#endif
