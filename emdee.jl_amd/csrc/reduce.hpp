// reduce.hpp -- the one deterministic two-stage fp64 reduction behind every box sum (mixed precision: fp32 per-atom values, fp64
// totals).  Stage 1, k_reduce_partials<Term>: a grid-stride loop in which a thread adds its elements' terms into its own words, then
// block_sum (block_max) per word into partial[block][word].  Stage 2, final_word: one block, a strided loop over the blocks' partials,
// then block_sum (block_max) again.  No atomics; the number of blocks is a function of n alone (red_blocks), so the order of summation
// is, and a total is the same bits on every run.  A Term is a small struct of pointers and scalars -- EnergySums and TensorSums
// (kernels.hpp), MoleculeSums (settle.hpp), MoleculeAtomSums (molecule.hpp), RestraintSums (restraint.hpp), FireSums (minimize.hpp), KineticSums (thermostat.hpp),
// HeatSums (gk.hpp) -- with
//     static constexpr int SUMS, MAXES;                      // its words: SUMS sums first, then MAXES maxima of values >= 0
//     __device__ void operator()(int i, double *acc) const;  // element i's terms into acc[0 .. SUMS + MAXES)
// NbSystem::queue (nbsys.hpp) launches the two stages and owns the scratch.  The block counts are plain C++ at the top; the device
// code below them needs HIP.
#pragma once

namespace emdee {

constexpr int RED_BLOCK = 256;
constexpr int RED_MAX_BLOCKS = 1024;
constexpr int RED_MAX_WORDS = 12;                            // the widest term (the tensor sums)

// the blocks of stage 1 over n elements
inline int red_blocks(long long n) {
    const long long nb = (n + RED_BLOCK - 1) / RED_BLOCK;
    return (int)(nb < RED_MAX_BLOCKS ? nb : RED_MAX_BLOCKS);
}

}  // namespace emdee

#if defined(__HIPCC__)

#include "wave_ops.hpp"

namespace emdee {

__device__ __forceinline__ double block_sum(double v, double *sh) {
    v = wave_sum_to_lane63(v);
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if (lane == WAVE - 1) sh[wv] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int w = 0; w < RED_BLOCK / WAVE; w++) t += sh[w];
    __syncthreads();
    return t;   // valid in thread 0
}

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

// stage 1: partial[b][0 .. WORDS) over the elements of block b's stride.  The body, for k_reduce_partials and for a stage-1 kernel that
// a family keeps under its own name (molecule.hpp k_molecule_partials); sh: RED_BLOCK / WAVE doubles of LDS
template <class Term>
__device__ __forceinline__ void reduce_partials(int n, const Term &term, double *__restrict__ partial, double *sh) {
    constexpr int WORDS = Term::SUMS + Term::MAXES;
    static_assert(WORDS >= 1 && WORDS <= RED_MAX_WORDS, "the scratch of the reductions is sized for RED_MAX_WORDS words");
    double acc[WORDS];
    for (int q = 0; q < WORDS; q++) acc[q] = 0.0;
    for (int i = blockIdx.x * RED_BLOCK + threadIdx.x; i < n; i += gridDim.x * RED_BLOCK) term(i, acc);
    for (int q = 0; q < WORDS; q++) {
        const double t = q < Term::SUMS ? block_sum(acc[q], sh) : block_max(acc[q], sh);
        if (threadIdx.x == 0) partial[WORDS * blockIdx.x + q] = t;
    }
}
template <class Term>
__global__ __launch_bounds__(RED_BLOCK) void k_reduce_partials(int n, Term term, double *__restrict__ partial) {
    __shared__ double sh[RED_BLOCK / WAVE];
    reduce_partials(n, term, partial, sh);
}

// stage 2, one block: word q of `words` over the blocks' partials, valid in thread 0
__device__ __forceinline__ double final_word(int nblocks, const double *__restrict__ partial, int words, int q, bool is_max, double *sh) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += RED_BLOCK) {
        const double t = partial[(size_t)words * b + q];
        s = is_max ? fmax(s, t) : s + t;
    }
    return is_max ? block_max(s, sh) : block_sum(s, sh);
}
// out[0 .. sums) = the sums, out[sums .. sums + maxes) = the maxima
static __global__ __launch_bounds__(RED_BLOCK) void k_reduce_final(int nblocks, int sums, int maxes, const double *__restrict__ partial,
                                                                   double *__restrict__ out) {
    __shared__ double sh[RED_BLOCK / WAVE];
    for (int q = 0; q < sums + maxes; q++) {
        const double t = final_word(nblocks, partial, sums + maxes, q, q >= sums, sh);
        if (threadIdx.x == 0) out[q] = t;
    }
}

}  // namespace emdee
#endif
