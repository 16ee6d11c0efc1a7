// gk.hpp -- Green-Kubo observables on the device (emdee_md_set_gk, emdee_md_gk_sample): per sample nine fp64 words -- the five
// independent traceless components of the stress S = K + W, its trace / 3, and the heat flux J -- a ring of them in HBM, and a
// correlator that adds A_w(s) A_w(s - l) to the lag sums with nothing read back.  The stress words come from the twelve box sums of
// the pressure entries (TensorSums, kernels.hpp, through reduce.hpp), the heat flux from one more reduction of that shape over the
// tensor pass's per-atom energies and tensors and the velocities.  The parts with no HIP in them -- the six stress words, an atom's
// three heat addends, the ring slot and the lag counts -- are plain C++ at the top, as the top of msd.hpp is: a stand-alone host
// program tests them with the host compiler (tests/c/gk_host.cpp); the kernels below them need HIP.  DESIGN.md 4i has the algorithm;
// MdImpl::gk_sample (impl.hpp) queues a sample.
#pragma once

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int GK_WORDS = 9, GK_STRESS_WORDS = 6, GK_HEAT_WORDS = 3;
constexpr int GK_STRESS = 1, GK_HEAT = 2;                    // (EMDEE_GK_STRESS, EMDEE_GK_HEAT)
constexpr int GK_MAX_LAGS = 65536;
constexpr int GK_BOX_SUMS = 12;                              // (TENSOR_SUMS: W then K, each xx, yy, zz, xy, xz, yz)

// ---- the stress words
// t[0..5] = W, t[6..11] = K, (xx, yy, zz, xy, xz, yz): S_ab = K_ab + W_ab, then xy, xz, yz, (xx - yy) / 2, (yy - zz) / 2 and the
// trace / 3.  No product that could contract with a sum: the same bits from every compiler.
EMDEE_HD void gk_stress_words(const double t[GK_BOX_SUMS], double out[GK_STRESS_WORDS]) {
    const double sxx = t[6] + t[0], syy = t[7] + t[1], szz = t[8] + t[2];
    out[0] = t[9] + t[3];
    out[1] = t[10] + t[4];
    out[2] = t[11] + t[5];
    out[3] = 0.5 * (sxx - syy);
    out[4] = 0.5 * (syy - szz);
    out[5] = (sxx + syy + szz) / 3.0;
}

// ---- the heat flux
// an atom's three addends of J = sum (k + e) v + sum W . v from its records -- inverse mass, energy and tensor (xx, yy, zz, xy, xz, yz)
// of the tensor pass, velocity -- in the engine's precision; the arithmetic is fp64.  k = m v^2 / 2, exactly 0 for a massless atom.
template <typename real>
EMDEE_HD void gk_heat_term(real inv_mass, real e, const real w[6], const real v[3], double out[GK_HEAT_WORDS]) {
    const double vx = (double)v[0], vy = (double)v[1], vz = (double)v[2];
    const double k = inv_mass != (real)0 ? 0.5 * (vx * vx + vy * vy + vz * vz) / (double)inv_mass : 0.0;
    const double h = k + (double)e;
    out[0] = h * vx + ((double)w[0] * vx + (double)w[3] * vy + (double)w[4] * vz);
    out[1] = h * vy + ((double)w[3] * vx + (double)w[1] * vy + (double)w[5] * vz);
    out[2] = h * vz + ((double)w[4] * vx + (double)w[5] * vy + (double)w[2] * vz);
}

// ---- the ring and the lags
// Samples are numbered s = 0, 1, ...; every sample is an origin.  Sample s lives in ring slot s % n_lags and is correlated with
// the samples s - l, l = 0 ... min(s, n_lags - 1): those are still in the ring, sample s - n_lags is the one s has just replaced.
EMDEE_HD int gk_slot(long long s, int n_lags) { return (int)(s % n_lags); }
EMDEE_HD int gk_live_lags(long long s, int n_lags) { return (int)(s < n_lags - 1 ? s + 1 : n_lags); }
// the number of products behind lag l after `samples` samples
EMDEE_HD long long gk_count(long long samples, int lag) { return samples > lag ? samples - lag : 0; }

}  // namespace emdee

#if defined(__HIPCC__)

#include "kernels.hpp"

namespace emdee {

// The term of the heat flux (reduce.hpp), over the owned slots, fp64 in both precisions: the three heat addends.  en, vt: the per-atom
// energies and tensors of the last tensor pass; vel: the velocities EnergySums takes, no pending kick.
template <typename real>
struct HeatSums {
    static constexpr int SUMS = GK_HEAT_WORDS, MAXES = 0;
    int n_owned;
    size_t pitch;
    const int *perm;
    const real *en, *vt, *vel, *inv_mass;
    __device__ __forceinline__ void operator()(int p, double *s) const {
        if (perm[p] >= n_owned) return;
        real w[6], v[3];
#pragma unroll
        for (int c = 0; c < 6; c++) w[c] = vt[c * pitch + p];
#pragma unroll
        for (int d = 0; d < 3; d++) v[d] = vel[d * pitch + p];
        double term[GK_HEAT_WORDS];
        gk_heat_term<real>(inv_mass ? inv_mass[p] : (real)1, en[p], w, v, term);
#pragma unroll
        for (int d = 0; d < GK_HEAT_WORDS; d++) s[d] += term[d];
    }
};

// what a sample needs of the table: the mask, the ring, the sample's number; acc = sums (n_lags x 9), then totals (9), then last (9)
struct GkArgs {
    int what, n_lags, molecular;
    long long s;
    double *ring, *acc;
    EMDEE_HD double *sums() const { return acc; }
    EMDEE_HD double *totals() const { return acc + (size_t)n_lags * GK_WORDS; }
    EMDEE_HD double *last() const { return acc + (size_t)n_lags * GK_WORDS + GK_WORDS; }
};

// One thread: the nine words of sample a.s to its ring slot and to `last`, and added to the totals.  box: the twelve sums of the
// pressure entry, or (a.molecular) twenty-four, the atomic sums and what the rigid molecules carry about their centres, subtracted
// here in the order of NbSystem::molecular_tensor_sums; heat: the three sums of J.  NULL: the words of that bit stay exactly 0.
static __global__ void k_gk_push(GkArgs a, const double *__restrict__ box, const double *__restrict__ heat) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double A[GK_WORDS];
#pragma unroll
    for (int w = 0; w < GK_WORDS; w++) A[w] = 0.0;
    if (box) {
        double t[GK_BOX_SUMS];
#pragma unroll
        for (int q = 0; q < GK_BOX_SUMS; q++) t[q] = a.molecular ? box[q] - box[GK_BOX_SUMS + q] : box[q];
        gk_stress_words(t, A);
    }
    if (heat)
#pragma unroll
        for (int d = 0; d < GK_HEAT_WORDS; d++) A[GK_STRESS_WORDS + d] = heat[d];
    double *slot = a.ring + (size_t)gk_slot(a.s, a.n_lags) * GK_WORDS, *totals = a.totals(), *last = a.last();
#pragma unroll
    for (int w = 0; w < GK_WORDS; w++) {
        slot[w] = A[w];
        last[w] = A[w];
        totals[w] += A[w];
    }
}

// One thread per lag l <= min(s, n_lags - 1): sums[l][w] += A_w(s) A_w(s - l).  A thread owns its nine sums and the samples follow
// one another on the stream: plain loads and stores, no atomics.
constexpr int GK_BLOCK = 256;
static __global__ __launch_bounds__(GK_BLOCK) void k_gk_correlate(GkArgs a) {
    const int l = blockIdx.x * GK_BLOCK + threadIdx.x;
    if (l >= gk_live_lags(a.s, a.n_lags)) return;
    const double *now = a.ring + (size_t)gk_slot(a.s, a.n_lags) * GK_WORDS;
    const double *then = a.ring + (size_t)gk_slot(a.s - l, a.n_lags) * GK_WORDS;
    double *dst = a.sums() + (size_t)l * GK_WORDS;
#pragma unroll
    for (int w = 0; w < GK_WORDS; w++) dst[w] += now[w] * then[w];
}

}  // namespace emdee
#endif
