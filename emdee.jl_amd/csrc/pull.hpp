// pull.hpp -- centre-of-mass pulling between atom groups (emdee_md_set_pull): a harmonic (umbrella) or constant bias along the distance
// or the projection between the centres of mass of two groups.  One more post term behind a force pass (NbSystem::add_pull, next to
// add_restraints), three launches: (1) one workgroup per chunk of the table order (group_layout.hpp) sums m x, m y, m z and m of its
// atoms' unwrapped fp64 coordinates (restraint_unwrapped) into partial[chunk][4]; (2) one block sums the partials per group in a fixed
// order, forms every coordinate's xi, f, U, D and work, writes the read-back words and the log entry, and folds the coordinates into
// ten words per group (the acceleration, the energy share, six tensor shares, each per unit mass); (3) one thread per table entry adds
// m_i times its group's words to the planes the pass's mask asks for.  No atomics, no order that depends on the CU count: the same
// bits in every run.  No minimum image anywhere.
// The parts with no HIP in them -- the term of one coordinate, the work rule, a group's ten words -- are plain C++ at the top, as the
// top of restraint.hpp is: a stand-alone host program tests them with the host compiler (tests/c/pull_host.cpp); the kernels below
// them need HIP.  DESIGN.md 4k has the algorithm; MdImpl::set_pull (impl.hpp) installs a table.
#pragma once

#include <cmath>

#include "group_layout.hpp"

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int PULL_MAX_GROUPS = MSD_MAX_GROUPS, PULL_MAX_COORDS = 8;
constexpr int PULL_WORDS = 8;                                // (EMDEE_PULL_WORDS) xi, xi0, f, U, work, Dx, Dy, Dz
constexpr int PULL_GROUP_WORDS = 10;                         // A[3], the energy share, six tensor shares: all per unit mass
constexpr int PULL_UMBRELLA = 1, PULL_CONSTANT_FORCE = 2;    // (EMDEE_PULL_UMBRELLA, EMDEE_PULL_CONSTANT_FORCE)
constexpr int PULL_DISTANCE = 1, PULL_DIRECTION = 2;         // (EMDEE_PULL_DISTANCE, EMDEE_PULL_DIRECTION)

// one coordinate as the kernels take it, by value.  k: the spring constant (umbrella) or the force F (constant force); n: the unit
// vector of the direction geometry; mask: bit a keeps axis a in the distance geometry
struct PullCoord {
    int a, b, kind, geometry, mask;
    double k, rate, n[3];
};
// what one coordinate gives at D = R_b - R_a: the read-back words and the force on group b with its tensor
struct PullResult {
    int a, b;
    double xi, f, U, D[3], Fb[3], T[6];
};

// ---- the term of one coordinate
// distance: xi = |m o D|, dxi/dD = m o D / xi; at xi = 0 the force is zero and U finite (bonded.hpp's convention): no division happens.
// direction: xi = n . D, signed, dxi/dD = n.  umbrella: U = 1/2 k (xi - xi0)^2; constant force: U = -F xi.  f = -dU/dxi, F_b = f dxi/dD
// is the force on group b, -F_b the force on group a, T the symmetrised D (x) F_b in the order (xx, yy, zz, xy, xz, yz).
EMDEE_HD void pull_term(const PullCoord &c, double xi0, const double D[3], PullResult &r) {
    double g[3];                                             // dxi/dD
    double xi;
    if (c.geometry == PULL_DIRECTION) {
        xi = c.n[0] * D[0] + c.n[1] * D[1] + c.n[2] * D[2];
        for (int a = 0; a < 3; a++) g[a] = c.n[a];
    } else {
        double md[3], s = 0.0;
        for (int a = 0; a < 3; a++) {
            md[a] = ((c.mask >> a) & 1) ? D[a] : 0.0;
            s += md[a] * md[a];
        }
        xi = sqrt(s);
        const double inv = xi > 0.0 ? 1.0 / xi : 0.0;
        for (int a = 0; a < 3; a++) g[a] = md[a] * inv;
    }
    double f, U;
    if (c.kind == PULL_CONSTANT_FORCE) {
        f = c.k;
        U = -c.k * xi;
    } else {
        const double d = xi - xi0;
        f = -c.k * d;
        U = 0.5 * c.k * d * d;
    }
    r.a = c.a; r.b = c.b;
    r.xi = xi; r.f = f; r.U = U;
    for (int a = 0; a < 3; a++) { r.D[a] = D[a]; r.Fb[a] = f * g[a]; }
    r.T[0] = D[0] * r.Fb[0]; r.T[1] = D[1] * r.Fb[1]; r.T[2] = D[2] * r.Fb[2];
    r.T[3] = 0.5 * (D[0] * r.Fb[1] + D[1] * r.Fb[0]);
    r.T[4] = 0.5 * (D[0] * r.Fb[2] + D[2] * r.Fb[0]);
    r.T[5] = 0.5 * (D[1] * r.Fb[2] + D[2] * r.Fb[1]);
}

// ---- the moving reference and the work
// xi0 after one more completed step of length dt: one fp64 addition per step, on the host, so that the sequence does not depend on
// how the steps are dealt to calls
inline double pull_advance(double xi0, double rate, double dt) { return xi0 + rate * dt; }
// the work done on the system by the moving reference, by the RECTANGLE RULE: at the force pass that closes a step, after xi0 has
// advanced, work += f rate dt with f at the new xi and xi0 (dU/dxi0 = -f for the umbrella)
EMDEE_HD double pull_work(double work, double f, double rate, double dt) { return work + f * rate * dt; }

// ---- a group's ten words from the coordinates that name it, in coordinate order, per unit mass of the group: atom i of the group
// gets m_i times them.  A = sum (+-F_b) / M; the energy share sum 1/2 U / M; the tensor shares sum 1/2 T / M -- so that the box sums hold
// exactly U_c and sym(D_c (x) F_b,c).  A group of mass 0 gets nothing.
EMDEE_HD void pull_group_words(const PullResult *res, int n_coords, int g, double M, double out[PULL_GROUP_WORDS]) {
    for (int w = 0; w < PULL_GROUP_WORDS; w++) out[w] = 0.0;
    for (int c = 0; c < n_coords; c++) {
        const bool is_a = res[c].a == g, is_b = res[c].b == g;
        if (!is_a && !is_b) continue;
        const double sign = is_b ? 1.0 : -1.0;
        for (int a = 0; a < 3; a++) out[a] += sign * res[c].Fb[a];
        out[3] += 0.5 * res[c].U;
        for (int q = 0; q < 6; q++) out[4 + q] += 0.5 * res[c].T[q];
    }
    const double inv = M > 0.0 ? 1.0 / M : 0.0;
    for (int w = 0; w < PULL_GROUP_WORDS; w++) out[w] *= inv;
}

}  // namespace emdee

#if defined(__HIPCC__)
#include "kernels.hpp"
#include "restraint.hpp"

namespace emdee {

static_assert(MSD_BLOCK == RED_BLOCK, "k_pull_partials reduces a chunk with block_sum");

// What the finishing block needs of the table, by value: the host owns xi0.  closing: this pass closes a step of length dt (the work
// word advances); log_slot >= 0: the pass's xi and f go to that entry of the log.
struct ComPullArgs {
    int n_groups, n_coords, closing, log_slot;
    int chunk_of_group[PULL_MAX_GROUPS + 1];
    double dt;
    double xi0[PULL_MAX_COORDS];
    PullCoord coord[PULL_MAX_COORDS];
};

// the mass of the atom in slot p: 1 / inv_mass, 1 where the engine has no masses; a massless atom (the builder refuses the sites of the
// site table) weighs nothing
template <typename real>
__device__ __forceinline__ double pull_mass(const real *__restrict__ inv_mass, int p) {
    if (!inv_mass) return 1.0;
    const double w = (double)inv_mass[p];
    return w > 0.0 ? 1.0 / w : 0.0;
}

// (1) One workgroup per chunk: a.atoms is the table order (one caller id per entry).  A thread takes entries first + t, first + t + 256,
// ... of its chunk; the four words go through block_sum into partial[chunk][0..3].
template <typename real>
__global__ __launch_bounds__(MSD_BLOCK) void k_pull_partials(RestraintArgs<real> a, const real *__restrict__ inv_mass,
                                                             const MsdChunk *__restrict__ chunks, double *__restrict__ partial) {
    __shared__ double sh[RED_BLOCK / WAVE];
    const MsdChunk ch = chunks[blockIdx.x];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < MSD_PER_THREAD; k++) {
        const int e = threadIdx.x + k * MSD_BLOCK;
        if (e >= ch.count || ch.first + e >= a.n) continue;
        const int p = restraint_slot(a, ch.first + e);
        if (p < 0) continue;
        double x[3];
        restraint_unwrapped(a, p, x);
        const double m = pull_mass(inv_mass, p);
        s[0] += m * x[0]; s[1] += m * x[1]; s[2] += m * x[2]; s[3] += m;
    }
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const double t = block_sum(s[w], sh);
        if (threadIdx.x == 0) partial[4 * (size_t)blockIdx.x + w] = t;
    }
}

// (2) One block.  Per group the chunk partials in a fixed order (final_word, reduce.hpp) give M and R; one thread per coordinate forms
// the term, advances the work word and writes coords_out[c][0..7] (and the log entry); one thread per group folds the coordinates into
// group_words[g][0..9].  coords_out keeps the work word between passes: the host zeroes it at the set.  The arrays that are indexed at
// run time live in LDS; the argument struct is read with compile-time indices only.
static __global__ __launch_bounds__(RED_BLOCK) void k_pull_finish(ComPullArgs a, const double *__restrict__ partial, double *__restrict__ coords_out,
                                                                  double *__restrict__ groups_out, double *__restrict__ group_words,
                                                                  double *__restrict__ log) {
    __shared__ double sh[RED_BLOCK / WAVE];
    __shared__ double R[PULL_MAX_GROUPS][4];
    __shared__ PullResult res[PULL_MAX_COORDS];
    const int t = threadIdx.x;
#pragma unroll
    for (int g = 0; g < PULL_MAX_GROUPS; g++) {
        if (g >= a.n_groups) continue;                       // (uniform: every thread takes the same branch, the barriers inside are safe)
        const int c0 = a.chunk_of_group[g], c1 = a.chunk_of_group[g + 1];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const double tot = final_word(c1 - c0, partial + 4 * (size_t)c0, 4, w, false, sh);
            if (t == 0) R[g][w] = tot;
        }
    }
    __syncthreads();
    if (t < a.n_groups) {
        const double M = R[t][3], inv = M > 0.0 ? 1.0 / M : 0.0;
        for (int d = 0; d < 3; d++) R[t][d] *= inv;
        for (int w = 0; w < 4; w++) groups_out[4 * t + w] = R[t][w];
    }
    __syncthreads();
    if (t < a.n_coords) {
        PullCoord pc = a.coord[0];
        double xi0 = a.xi0[0];
#pragma unroll
        for (int c = 1; c < PULL_MAX_COORDS; c++)
            if (t == c) { pc = a.coord[c]; xi0 = a.xi0[c]; }
        double D[3];
        for (int d = 0; d < 3; d++) D[d] = R[pc.b][d] - R[pc.a][d];
        PullResult r;
        pull_term(pc, xi0, D, r);
        double *out = coords_out + PULL_WORDS * t;
        double work = out[4];
        if (a.closing && pc.kind == PULL_UMBRELLA) work = pull_work(work, r.f, pc.rate, a.dt);
        out[0] = r.xi; out[1] = xi0; out[2] = r.f; out[3] = r.U; out[4] = work;
        out[5] = D[0]; out[6] = D[1]; out[7] = D[2];
        if (a.log_slot >= 0) {
            double *l = log + 2 * ((size_t)a.log_slot * a.n_coords + t);
            l[0] = r.xi; l[1] = r.f;
        }
        res[t] = r;
    }
    __syncthreads();
    if (t < a.n_groups) {
        double gw[PULL_GROUP_WORDS];
        pull_group_words(res, a.n_coords, t, R[t][3], gw);
        for (int w = 0; w < PULL_GROUP_WORDS; w++) group_words[PULL_GROUP_WORDS * t + w] = gw[w];
    }
}

// (3) One thread per table entry: m_i times its group's words into the planes the mask asks for (TENSOR: the tensor pass, six planes
// of vt).  Each atom is in one group: plain read-modify-writes.
template <typename real, bool TENSOR>
__global__ __launch_bounds__(256) void k_pull_apply(RestraintArgs<real> a, const real *__restrict__ inv_mass, const int *__restrict__ group_of,
                                                    const double *__restrict__ group_words, int bitmask, real *__restrict__ frc,
                                                    real *__restrict__ en, real *__restrict__ vir, real *__restrict__ vt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n) return;
    const int p = restraint_slot(a, e);
    if (p < 0) return;
    const int g = group_of[e];
    if (g < 0 || g >= PULL_MAX_GROUPS) return;
    const double m = pull_mass(inv_mass, p);
    const double *gw = group_words + PULL_GROUP_WORDS * g;
    if (bitmask & EMDEE_FORCES) {
        frc[p] += (real)(m * gw[0]); frc[a.pitch + p] += (real)(m * gw[1]); frc[2 * a.pitch + p] += (real)(m * gw[2]);
    }
    if (bitmask & EMDEE_ENERGIES) en[p] += (real)(m * gw[3]);
    if (bitmask & EMDEE_VIRIALS) vir[p] += (real)(m * (gw[4] + gw[5] + gw[6]));
    if (TENSOR)
        for (int c = 0; c < 6; c++) vt[c * a.pitch + p] += (real)(m * gw[4 + c]);
}

}  // namespace emdee
#endif
