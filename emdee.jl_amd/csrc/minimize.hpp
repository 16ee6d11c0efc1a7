// minimize.hpp -- energy minimisation on the device (emdee_md_minimize): FIRE (Bitzek, Koskinen, Gaehler, Moseler & Gumbsch,
// Phys. Rev. Lett. 97, 170201 (2006)) around the closed velocity-Verlet step of MdImpl::closed_step, with the engine's masses and
// whatever constraint tables are in force.  The two update rules at the top are plain C++ on doubles, as the tops of settle.hpp
// and shake.hpp are: a stand-alone host program tests them with the host compiler (tests/c/fire_host.cpp); the kernels below them
// need HIP.  DESIGN.md 4d has the algorithm; MdImpl::minimize (impl.hpp) drives it.
#pragma once

#include "settle.hpp"

namespace emdee {

// the paper's constants
constexpr int FIRE_N_MIN = 5;
constexpr double FIRE_F_INC = 1.1, FIRE_F_DEC = 0.5, FIRE_ALPHA0 = 0.1, FIRE_F_ALPHA = 0.99;

// the host scalars of one call
struct FireState {
    double dt, alpha, dt_max;
    int n_pos;
};
EMDEE_HD FireState fire_start(double dt_start, double dt_max) { return FireState{dt_start, FIRE_ALPHA0, dt_max, 0}; }

// The step cap: the largest t <= dt with t vmax + t^2 amax / 2 <= max_step, so that no atom's unconstrained drift t v + t^2 w F / 2
// exceeds max_step.  vmax, amax >= 0, max_step > 0.  The root is taken in the form that does not cancel and that holds for amax = 0
// (max_step / vmax) and for vmax = 0 (sqrt(2 max_step / amax)) alike.
EMDEE_HD double fire_cap(double dt, double vmax, double amax, double max_step) {
    if (dt * vmax + 0.5 * dt * dt * amax <= max_step) return dt;
    const double t = 2.0 * max_step / (vmax + sqrt(vmax * vmax + 2.0 * amax * max_step));
    return t < dt ? t : dt;
}

// Step 6 on the scalars, P = sum G . v of the iteration just completed.  True: the velocities are to be mixed (with the alpha the
// state held BEFORE the call); false: they are to be zeroed.
EMDEE_HD bool fire_update(FireState &s, double P) {
    if (P > 0.0) {
        if (++s.n_pos > FIRE_N_MIN) {
            const double dt = FIRE_F_INC * s.dt;
            s.dt = dt < s.dt_max ? dt : s.dt_max;
            s.alpha *= FIRE_F_ALPHA;
        }
        return true;
    }
    s.dt *= FIRE_F_DEC;
    s.alpha = FIRE_ALPHA0;
    s.n_pos = 0;
    return false;
}

}  // namespace emdee

#if defined(__HIPCC__)

namespace emdee {

// what one reduction brings back: sum G . v, sum v . v, sum G . G, then the largest |G_i|^2, |v_i|^2 and |w_i F_i|^2
constexpr int FIRE_SUMS = 3, FIRE_MAXIMA = 3, FIRE_WORDS = FIRE_SUMS + FIRE_MAXIMA;

// mode 0: a = w F on every owned slot (the plane the velocity stages project, ConstraintArgs::vel); mode 1, after the projection:
// a -> G = a / w where the projection changed a component, F itself where it did not (every atom outside the tables); 0 for an
// atom with w = 0 (a virtual site, whose force has gone to its parents).
template <typename real>
__global__ __launch_bounds__(256) void k_fire_weight(int n, int n_owned, size_t pitch, const int *__restrict__ perm,
                                                     const real *__restrict__ frc, const real *__restrict__ inv_mass,
                                                     real *__restrict__ a, int mode) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    const real w = inv_mass ? inv_mass[p] : (real)1;
    const real fx = frc[p], fy = frc[pitch + p], fz = frc[2 * pitch + p];
    const real ax = w * fx, ay = w * fy, az = w * fz;
    if (mode == 0) {
        a[p] = ax; a[pitch + p] = ay; a[2 * pitch + p] = az;
        return;
    }
    if (w == (real)0) {                                      // (a massless atom, a virtual site: G = 0, no 0 / 0)
        a[p] = (real)0; a[pitch + p] = (real)0; a[2 * pitch + p] = (real)0;
        return;
    }
    const real bx = a[p], by = a[pitch + p], bz = a[2 * pitch + p];
    a[p] = bx == ax ? fx : bx / w;
    a[pitch + p] = by == ay ? fy : by / w;
    a[2 * pitch + p] = bz == az ? fz : bz / w;
}

// The term of FIRE's six words (reduce.hpp), over the owned slots, fp64 in both precisions.  g: the G planes, or frc itself on an
// engine without a table.
template <typename real>
struct FireSums {
    static constexpr int SUMS = FIRE_SUMS, MAXES = FIRE_MAXIMA;
    int n_owned;
    size_t pitch;
    const int *perm;
    const real *g, *frc, *vel, *inv_mass;
    __device__ __forceinline__ void operator()(int p, double *acc) const {
        if (perm[p] >= n_owned) return;
        const double w = inv_mass ? (double)inv_mass[p] : 1.0;
        const double gx = (double)g[p], gy = (double)g[pitch + p], gz = (double)g[2 * pitch + p];
        const double vx = (double)vel[p], vy = (double)vel[pitch + p], vz = (double)vel[2 * pitch + p];
        const double fx = (double)frc[p], fy = (double)frc[pitch + p], fz = (double)frc[2 * pitch + p];
        const double gi = gx * gx + gy * gy + gz * gz, vi = vx * vx + vy * vy + vz * vz, ai = w * w * (fx * fx + fy * fy + fz * fz);
        acc[0] += gx * vx + gy * vy + gz * vz;
        acc[1] += vi;
        acc[2] += gi;
        acc[3] = fmax(acc[3], gi); acc[4] = fmax(acc[4], vi); acc[5] = fmax(acc[5], ai);
    }
};

// the mixing of step 6: v <- c_v v + c_g G, with c_v = 1 - alpha and c_g = alpha sqrt(vv / gg) from the host
template <typename real>
__global__ __launch_bounds__(256) void k_fire_mix(int n, int n_owned, size_t pitch, const int *__restrict__ perm, real *__restrict__ vel,
                                                  const real *__restrict__ g, real c_v, real c_g) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    vel[p] = c_v * vel[p] + c_g * g[p];
    vel[pitch + p] = c_v * vel[pitch + p] + c_g * g[pitch + p];
    vel[2 * pitch + p] = c_v * vel[2 * pitch + p] + c_g * g[2 * pitch + p];
}

}  // namespace emdee
#endif
