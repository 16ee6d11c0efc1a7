// bonded.hpp -- the formula of one bonded term (emdee_*_set_bonded): a harmonic bond, a harmonic angle or a periodic torsion
// at unwrapped positions, its energy and the force on each of its atoms.  Plain C++ on fixed-size arrays, templated on the real
// type, as the tops of settle.hpp and shake.hpp are: no HIP types, so that a stand-alone host program runs the very expressions
// the device runs (tests/c/bonded_host.cpp, for float and double); k_bonded (kernels.hpp) is the one caller on the device.
//
// Singular geometries (include/emdee_hip.h, "bonded terms").  The direction of a term's force is undefined
// where a norm it divides by is zero: a bond of length 0, an angle with |a x b| = 0 (straight or folded), a torsion with
// |b1 x b2| = 0, |b2 x b3| = 0 or b2 = 0.  There the term gives zero force on all its atoms and a finite energy.  Each guarded
// denominator (r; |a x b|; |m|^2, |n|^2, |b2|^2) selects: at or above `tiny` the quotient is the one it always was, below it
// the numerator is zero (for the angle: its force constant), and zero over max(den, tiny) is zero.  The guard max(den, tiny)
// alone is not enough: at den = 0 the quotient overflows as soon as |x| / tiny leaves the format (|x| above 34 in float, above
// 1.8e8 in double), and infinity times the zero cross product is NaN.  The selects sit on scalars in front of the divisions and
// nowhere else on purpose: the fp32 build packs and fuses the multiply-adds around them, and a select on the finished forces
// or on a denominator regroups them, which moves the last bit of every fp32 trajectory.  As written the arithmetic of a term
// with every denominator at or above tiny is bit for bit what it was before there was a contract, in either precision.
// What is left out: an angle's quotient also divides by |a|^2 (|b|^2); with |a x b| = 0 *and* an arm shorter than 1e-4 (float;
// 1e-11 in double) of the length unit, |a|^2 tiny underflows to zero and 0 / 0 is NaN.  Two atoms of an angle that close are
// not a geometry the contract covers.
#pragma once

#include <algorithm>
#include <cmath>

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#define EMDEE_UNROLL _Pragma("unroll")
#else
#define EMDEE_HD inline
#define EMDEE_UNROLL
#endif

namespace emdee {

template <typename real>
EMDEE_HD void cross3(const real a[3], const real b[3], real c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
template <typename real>
EMDEE_HD real dot3(const real a[3], const real b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// below this a guarded denominator counts as zero
template <typename real>
EMDEE_HD real bonded_tiny() { return sizeof(real) == 8 ? (real)1e-300 : (real)1e-37; }

// U and the forces F[0 .. nat) of one term at unwrapped positions u[0 .. nat) (kind: 1 bond, 2 angle, 3 torsion)
template <typename real>
EMDEE_HD real bonded_term(int kind, const real u[4][3], real p0, real p1, real p2, real F[4][3]) {
#if !defined(__HIPCC__)
    using std::atan2;                                        // (the device has these overloads in the global namespace)
    using std::cos;
    using std::max;
    using std::sin;
    using std::sqrt;
#endif
    const real tiny = bonded_tiny<real>();
    real U;
    if (kind == 1) {
        real d[3];
        EMDEE_UNROLL
        for (int c = 0; c < 3; c++) d[c] = u[1][c] - u[0][c];
        const real r = sqrt(dot3(d, d));
        const real g = (r >= tiny ? p0 * (r - p1) : (real)0) / max(r, tiny);   // coincident atoms: no force, U = k/2 r0^2
        EMDEE_UNROLL
        for (int c = 0; c < 3; c++) { F[1][c] = -g * d[c]; F[0][c] = g * d[c]; F[2][c] = 0; F[3][c] = 0; }
        U = (real)0.5 * p0 * (r - p1) * (r - p1);
    } else if (kind == 2) {
        real a[3], b[3], cr[3], ac[3], bc[3];
        EMDEE_UNROLL
        for (int c = 0; c < 3; c++) { a[c] = u[0][c] - u[1][c]; b[c] = u[2][c] - u[1][c]; }
        cross3(a, b, cr);
        const real cn = sqrt(dot3(cr, cr));
        const real th = atan2(cn, dot3(a, b));               // finite at 0 and pi (no acos of a clamped cosine needed)
        const bool ok = cn >= tiny;                           // straight or folded: theta is 0 or pi, no force
        const real dU = (ok ? p0 : (real)0) * (th - p1);
        cross3(a, cr, ac);
        cross3(b, cr, bc);
        const real gi = -dU / (dot3(a, a) * max(cn, tiny)), gk = dU / (dot3(b, b) * max(cn, tiny));
        EMDEE_UNROLL
        for (int c = 0; c < 3; c++) {
            F[0][c] = gi * ac[c]; F[2][c] = gk * bc[c]; F[1][c] = -F[0][c] - F[2][c]; F[3][c] = 0;
        }
        U = (real)0.5 * p0 * (th - p1) * (th - p1);
    } else {
        real b1[3], b2[3], b3[3], m[3], n[3];
        EMDEE_UNROLL
        for (int c = 0; c < 3; c++) { b1[c] = u[1][c] - u[0][c]; b2[c] = u[2][c] - u[1][c]; b3[c] = u[3][c] - u[2][c]; }
        cross3(b1, b2, m);
        cross3(b2, b3, n);
        const real b22 = dot3(b2, b2), b2n = sqrt(b22);
        const real phi = atan2(b2n * dot3(b1, n), dot3(m, n));   // IUPAC: trans = pi
        const real arg = p1 * phi - p2;
        const real dU = -p0 * p1 * sin(arg);
        // a collinear bond pair on either side (or b2 = 0): phi is undefined, no force on any atom, U finite (atan2 of zeros)
        const bool ok = dot3(m, m) >= tiny && dot3(n, n) >= tiny && b22 >= tiny;
        const real ci = (ok ? dU * b2n : (real)0) / max(dot3(m, m), tiny), cl = (ok ? -dU * b2n : (real)0) / max(dot3(n, n), tiny);   // F_i = ci m, F_l = cl n
        const real s1 = dot3(b1, b2) / max(b22, tiny), s3 = dot3(b3, b2) / max(b22, tiny);
        EMDEE_UNROLL
        for (int c = 0; c < 3; c++) {
            F[0][c] = ci * m[c];
            F[3][c] = cl * n[c];
            F[1][c] = -((real)1 + s1) * F[0][c] + s3 * F[3][c];
            F[2][c] = -F[0][c] - F[3][c] - F[1][c];
        }
        U = p0 * ((real)1 + cos(arg));
    }
    return U;
}

}  // namespace emdee
