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

// the largest of a wavefront's values, valid in lane 63: wave_sum_to_lane63's exchange with max in place of +.  A lane without a
// source reads 0, which no value >= 0 minds.
__device__ __forceinline__ double wave_max_to_lane63(double v) {
    v = fmax(v, dpp_mov<DPP_ROW_SHR1, 0xf, 0xf>(v));
    v = fmax(v, dpp_mov<DPP_ROW_SHR2, 0xf, 0xf>(v));
    v = fmax(v, dpp_mov<DPP_ROW_SHR4, 0xf, 0xf>(v));
    v = fmax(v, dpp_mov<DPP_ROW_SHR8, 0xf, 0xf>(v));
    v = fmax(v, dpp_mov<DPP_ROW_BCAST15, 0xa, 0xf>(v));
    v = fmax(v, dpp_mov<DPP_ROW_BCAST31, 0xc, 0xf>(v));
    return v;
}
__device__ __forceinline__ double block_max(double v, double *sh) {
    v = wave_max_to_lane63(v);
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if (lane == WAVE - 1) sh[wv] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int w = 0; w < RED_BLOCK / WAVE; w++) t = fmax(t, sh[w]);
    __syncthreads();
    return t;   // valid in thread 0
}

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

// partial[b][0..5] over the owned slots of block b's stride, k_tensor_partials' shape: fp64 in both precisions, fixed order, no
// atomics (k_fire_final completes them).  g: the G planes, or frc itself on an engine without a table.
template <typename real>
__global__ __launch_bounds__(RED_BLOCK) void k_fire_partials(int n, int n_owned, size_t pitch, const int *__restrict__ perm,
                                                             const real *__restrict__ g, const real *__restrict__ frc,
                                                             const real *__restrict__ vel, const real *__restrict__ inv_mass,
                                                             double *__restrict__ partial) {
    __shared__ double sh[RED_BLOCK / WAVE];
    double P = 0.0, vv = 0.0, gg = 0.0, g2 = 0.0, v2 = 0.0, a2 = 0.0;
    for (int p = blockIdx.x * RED_BLOCK + threadIdx.x; p < n; p += gridDim.x * RED_BLOCK) {
        if (perm[p] >= n_owned) continue;
        const double w = inv_mass ? (double)inv_mass[p] : 1.0;
        const double gx = (double)g[p], gy = (double)g[pitch + p], gz = (double)g[2 * pitch + p];
        const double vx = (double)vel[p], vy = (double)vel[pitch + p], vz = (double)vel[2 * pitch + p];
        const double fx = (double)frc[p], fy = (double)frc[pitch + p], fz = (double)frc[2 * pitch + p];
        const double gi = gx * gx + gy * gy + gz * gz, vi = vx * vx + vy * vy + vz * vz, ai = w * w * (fx * fx + fy * fy + fz * fz);
        P += gx * vx + gy * vy + gz * vz;
        vv += vi;
        gg += gi;
        g2 = fmax(g2, gi); v2 = fmax(v2, vi); a2 = fmax(a2, ai);
    }
    double t;
    t = block_sum(P, sh); if (threadIdx.x == 0) partial[FIRE_WORDS * blockIdx.x] = t;
    t = block_sum(vv, sh); if (threadIdx.x == 0) partial[FIRE_WORDS * blockIdx.x + 1] = t;
    t = block_sum(gg, sh); if (threadIdx.x == 0) partial[FIRE_WORDS * blockIdx.x + 2] = t;
    t = block_max(g2, sh); if (threadIdx.x == 0) partial[FIRE_WORDS * blockIdx.x + 3] = t;
    t = block_max(v2, sh); if (threadIdx.x == 0) partial[FIRE_WORDS * blockIdx.x + 4] = t;
    t = block_max(a2, sh); if (threadIdx.x == 0) partial[FIRE_WORDS * blockIdx.x + 5] = t;
}

// out[0..5] = the three sums and the three maxima over the blocks' partials (k_final_sums' shape); out[6] = *energy, the potential
// energy k_final_sum3 has just left, so that one copy brings everything back
static __global__ __launch_bounds__(RED_BLOCK) void k_fire_final(int nblocks, const double *__restrict__ partial,
                                                                 const double *__restrict__ energy, double *__restrict__ out) {
    __shared__ double sh[RED_BLOCK / WAVE];
    for (int q = 0; q < FIRE_WORDS; q++) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += RED_BLOCK) {
            const double t = partial[(size_t)FIRE_WORDS * b + q];
            s = q < FIRE_SUMS ? s + t : fmax(s, t);
        }
        const double t = q < FIRE_SUMS ? block_sum(s, sh) : block_max(s, sh);
        if (threadIdx.x == 0) out[q] = t;
    }
    if (threadIdx.x == 0) out[FIRE_WORDS] = *energy;
}

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
