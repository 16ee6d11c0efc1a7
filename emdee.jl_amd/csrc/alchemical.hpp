// alchemical.hpp -- soft-core alchemical decoupling of one group of atoms, the "solute" (emdee_md_set_alchemical): the Lennard-Jones
// coupling between a flagged and an unflagged atom is turned off along lambda through the soft core of Beutler et al. 1994 with
// lambda-power 1 and r-power 6 (GROMACS sc-power = 1, sc-r-power = 6),
//     u = (r^2 / sigma_ij^2)^3,  D = alpha (1 - lambda) + u,  U(r; lambda) = lambda 4 eps_ij (D^-2 - D^-1) g(r),
// g the model's switch, the cutoff the caller's test as in lj_pair.hpp.  Flagged-flagged and unflagged-unflagged pairs stay in the
// ordinary rows at full strength: decoupling, not annihilation.
// Right after every list build a row pass strikes the cross entries from the rows of the owned atoms and records their cell-order
// slots in a compact CSR of the build (count, one exclusive scan, fill: memory O(struck entries)), with the list of the atoms that own
// at least one, solute owners first.  Behind every force pass one launch runs over that list, owner-computes as k_pairs14: one wavefront
// per solute owner (hundreds of entries, lanes over entries, summed in a fixed order with wave_ops.hpp), one thread per environment
// owner (a handful of entries); half of a pair's E and W to the owner, plain read-modify-writes to the planes, and the owner's half of
// U, dU/dlambda, W and the pair count as fp64 partials that reduce.hpp sums.  No atomics: the same bits in every run.
// The parts with no HIP in them -- the pair function, its foreign-lambda variant, the words of a read, the table checks -- are plain
// C++ at the top, as the top of pull.hpp is: a stand-alone host program tests them with the host compiler
// (tests/c/alchemical_host.cpp); the kernels below them need HIP.  DESIGN.md 4l has the algorithm; MdImpl::set_alchemical (impl.hpp)
// installs a table.
// The Coulomb stage (emdee_md_set_alchemical_coulomb) puts the soft-core charge term of a reaction-field engine on
// the same entries: alch_coulomb_pair beside alch_pair, the COUL instances of the two kernels, sums, words and a log of its own.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "error.hpp"

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int ALCH_WORDS = 5;                                // (EMDEE_ALCH_WORDS) lambda, U_alch, dU/dlambda, the cross virial, the cross pairs inside rc
constexpr int ALCH_MAX_FOREIGN = 16;                         // (EMDEE_ALCH_MAX_FOREIGN)
constexpr int ALCH_SUMS = 4;                                 // the words an owner writes: its half of U, dU/dlambda, W and of the pair count
constexpr int ALCH_COULOMB_WORDS = 4;                        // (EMDEE_ALCH_COULOMB_WORDS) lambda_q, U_q, dU/dlambda_q, the cross Coulomb virial
constexpr int ALCH_COULOMB_SUMS = 3;                         // the Coulomb words an owner writes: its half of U_q, dU/dlambda_q and W_q

// what the pair function needs of the model (lj_pair.hpp LJModel): x = r2 idl2 - x0, -r g' = c60 x^2 (1 - x)^2 r2
template <typename real>
struct AlchModel {
    real idl2, x0, c60;
};

// the reference's clamp of the switch variable (lj_pair.hpp switch_clamp): 0 < x < 1 -> x; x <= 0 -> 0; x == 1 -> 0.5; x > 1 -> 0
template <typename real>
EMDEE_HD real alch_clamp(real x) {
    x = x > (real)0 ? x : (real)0;
    if (x >= (real)1) x = (x == (real)1) ? (real)0.5 : (real)0;
    return x;
}

// ---- the pair function.  sigma2 = sigma_ij^2 and e4 = 4 eps_ij as lj_interaction forms them.  Returns
//   E       = lambda e4 (D^-2 - D^-1) g
//   W       = -r dE/dr = 6 u lambda e4 (2 D^-3 - D^-2) g + (E / g) (-r g')
//   dEdl    = e4 g [(D^-2 - D^-1) + lambda alpha (2 D^-3 - D^-2)]
//   wr2     = W / r^2, formed without a division by r^2 (u / r^2 = r^4 / sigma^6): the factor of the force d wr2, finite at r = 0
// At lambda = 1 D = u exactly and the term is lj_interaction_pair up to rounding; at lambda = 0 E, W and wr2 are exactly 0 (dEdl is
// not); at r = 0 with lambda < 1 and alpha > 0 everything is finite and W = 0; alpha = 0 is lambda times the plain pair.
template <typename real>
EMDEE_HD void alch_pair(real r2, const AlchModel<real> &m, real sigma2, real e4, real lambda, real alpha, real &E_out, real &W_out,
                        real &dEdl_out, real &wr2_out) {
    const real is2 = (real)1 / sigma2;
    const real t = r2 * is2, t2 = t * t;
    const real u = t2 * t;                                   // (r / sigma)^6
    const real D = alpha * ((real)1 - lambda) + u;
    const real iD = (real)1 / D;
    const real a = e4 * iD, b = a * iD;                      // 4 eps D^-1, 4 eps D^-2
    const real El = b - a;                                   // 4 eps (D^-2 - D^-1)
    const real Wl = ((real)2 * b - a) * iD;                  // 4 eps (2 D^-3 - D^-2)
    const real x = alch_clamp(r2 * m.idl2 - m.x0);
    const real v = (real)1 - x, v2 = v * v;
    const real g = (v2 * v) * ((real)1 + x * ((real)3 + (real)6 * x));
    const real mg2 = m.c60 * ((x * x) * v2);                 // -r g' / r^2
    const real core = (real)6 * Wl * g;
    dEdl_out = g * (El + lambda * alpha * Wl);
    if (lambda > (real)0) {
        E_out = lambda * (El * g);
        W_out = lambda * (u * core + El * (mg2 * r2));
        wr2_out = lambda * ((t2 * is2) * core + El * mg2);
    } else {                                                 // exactly 0, whatever D is
        E_out = (real)0; W_out = (real)0; wr2_out = (real)0;
    }
}
// E at K foreign lambda values (BAR, MBAR): K calls of the function above, bit for bit
template <typename real>
EMDEE_HD void alch_pair_foreign(real r2, const AlchModel<real> &m, real sigma2, real e4, real alpha, const real *lambdas, int K, real *E_out) {
    for (int k = 0; k < K; k++) {
        real W, dEdl, wr2;
        alch_pair(r2, m, sigma2, e4, lambdas[k], alpha, E_out[k], W, dEdl, wr2);
    }
}

// ---- the Coulomb stage (emdee_md_set_alchemical_coulomb): the charge term of the same cross pairs on a reaction-field engine, the
// soft core of Steinbrecher, Joung & Case 2011 (AMBER) on the reaction field of emdee_md_set_coulomb.  qq = K q_i q_j; k and c the
// reaction field's constants (lj_pair.hpp Charges: k = (eps_rf - 1) / ((2 eps_rf + 1) rc^3), c = 1/rc + k rc^2); beta a squared length:
//     rho2 = r2 + beta (1 - lambda_q),  phi = 1/rho + k rho2 - c,  wl = 1/rho^3 - 2 k
//   E       = lambda_q qq phi
//   wr2     = lambda_q qq wl          the factor of the force d wr2: finite at r = 0, where the force is 0
//   W       = wr2 r2                  = -r dE/dr
//   dEdl    = qq (phi + lambda_q (beta / 2) wl)
// One inverse square root, no sixth root.  At lambda_q = 0 E, W and wr2 are exactly 0 (dEdl is not); at beta (1 - lambda_q) = 0
// rho2 == r2 bit for bit and the term is lambda_q times the reaction-field pair; at r = 0 with beta (1 - lambda_q) > 0 everything is
// finite.  The cutoff is the caller's strict test: with beta (1 - lambda_q) > 0 E(rc) is not 0 (phi vanishes at rho = rc, not at
// r = rc), the jump GROMACS's soft-core reaction field has as well.
template <typename real>
struct AlchRf {
    real k, c;
};
template <typename real>
EMDEE_HD void alch_coulomb_pair(real r2, real qq, const AlchRf<real> &rf, real lambda_q, real beta, real &E_out, real &W_out, real &dEdl_out,
                                real &wr2_out) {
    const real rho2 = r2 + beta * ((real)1 - lambda_q);
    const real ir = (real)1 / std::sqrt(rho2);
    const real phi = ir + (rf.k * rho2 - rf.c);
    const real wl = (ir * ir) * ir - (real)2 * rf.k;
    dEdl_out = qq * (phi + lambda_q * ((real)0.5 * beta) * wl);
    if (lambda_q > (real)0) {
        E_out = lambda_q * (qq * phi);
        wr2_out = lambda_q * (qq * wl);
        W_out = wr2_out * r2;
    } else {                                                 // exactly 0, whatever rho is
        E_out = (real)0; W_out = (real)0; wr2_out = (real)0;
    }
}
// E at K foreign lambda_q values: K calls of the function above, bit for bit
template <typename real>
EMDEE_HD void alch_coulomb_pair_foreign(real r2, real qq, const AlchRf<real> &rf, real beta, const real *lambdas_q, int K, real *E_out) {
    for (int k = 0; k < K; k++) {
        real W, dEdl, wr2;
        alch_coulomb_pair(r2, qq, rf, lambdas_q[k], beta, E_out[k], W, dEdl, wr2);
    }
}

// ---- the table checks (emdee_md_set_alchemical): every refusal names the offending value
inline void alch_check_lambda(const char *what, double lambda) {
    EMDEE_REQUIRE(lambda >= 0.0 && lambda <= 1.0, EMDEE_ERR_INVALID, "%s: lambda = %g is outside [0, 1]", what, lambda);
}
// lambda and every foreign lambda in [0, 1]; alpha >= 0 and finite; n_foreign in 0 ... 16; the log as the pull's: a log (capacity > 0)
// needs log_every >= 1, neither is negative, and capacity entries of 2 + n_foreign words stay below 2^30 words
inline void alch_check_params(double lambda, double alpha, const double *foreign, int64_t n_foreign, int64_t log_every, int64_t log_capacity) {
    alch_check_lambda("set_alchemical", lambda);
    EMDEE_REQUIRE(std::isfinite(alpha) && alpha >= 0.0, EMDEE_ERR_INVALID, "set_alchemical: alpha = %g must be finite and >= 0", alpha);
    EMDEE_REQUIRE(n_foreign >= 0 && n_foreign <= ALCH_MAX_FOREIGN, EMDEE_ERR_INVALID, "set_alchemical: n_foreign = %lld is outside 0...%d",
                  (long long)n_foreign, ALCH_MAX_FOREIGN);
    EMDEE_REQUIRE(n_foreign == 0 || foreign, EMDEE_ERR_INVALID, "set_alchemical: NULL array of foreign lambdas with n_foreign = %lld",
                  (long long)n_foreign);
    for (int64_t k = 0; k < n_foreign; k++)
        EMDEE_REQUIRE(foreign[k] >= 0.0 && foreign[k] <= 1.0, EMDEE_ERR_INVALID, "set_alchemical: foreign lambda %lld = %g is outside [0, 1]",
                      (long long)k, foreign[k]);
    EMDEE_REQUIRE(log_capacity >= 0 && log_every >= 0 && (log_capacity == 0 || log_every >= 1), EMDEE_ERR_INVALID, "set_alchemical: log_every = "
                  "%lld and log_capacity = %lld: a log (capacity > 0) needs log_every >= 1, and neither is negative", (long long)log_every,
                  (long long)log_capacity);
    EMDEE_REQUIRE(log_capacity * (2 + n_foreign) <= INT32_MAX / 2, EMDEE_ERR_INVALID, "set_alchemical: log_capacity = %lld with %lld foreign "
                  "lambdas is more than 2^30 words", (long long)log_capacity, (long long)n_foreign);
}
// the checks of the Coulomb stage (emdee_md_set_alchemical_coulomb): lambda_q and every foreign lambda_q in [0, 1]; beta >= 0 and
// finite; as many foreign lambda_q as the table has foreign lambdas (the k-th foreign state is the pair of the two)
inline void alch_check_lambda_q(const char *what, double lambda_q) {
    EMDEE_REQUIRE(lambda_q >= 0.0 && lambda_q <= 1.0, EMDEE_ERR_INVALID, "%s: lambda_q = %g is outside [0, 1]", what, lambda_q);
}
inline void alch_coulomb_check_params(double lambda_q, double beta, const double *foreign_q, int64_t n_foreign, int64_t table_n_foreign) {
    alch_check_lambda_q("set_alchemical_coulomb", lambda_q);
    EMDEE_REQUIRE(std::isfinite(beta) && beta >= 0.0, EMDEE_ERR_INVALID, "set_alchemical_coulomb: beta = %g must be finite and >= 0", beta);
    EMDEE_REQUIRE(n_foreign == table_n_foreign, EMDEE_ERR_INVALID, "set_alchemical_coulomb: n_foreign = %lld, the alchemical table has %lld "
                  "foreign lambdas (the k-th foreign state is the pair of the two)", (long long)n_foreign, (long long)table_n_foreign);
    EMDEE_REQUIRE(n_foreign == 0 || foreign_q, EMDEE_ERR_INVALID, "set_alchemical_coulomb: NULL array of foreign lambda_q with n_foreign = %lld",
                  (long long)n_foreign);
    for (int64_t k = 0; k < n_foreign; k++)
        EMDEE_REQUIRE(foreign_q[k] >= 0.0 && foreign_q[k] <= 1.0, EMDEE_ERR_INVALID, "set_alchemical_coulomb: foreign lambda_q %lld = %g is outside "
                      "[0, 1]", (long long)k, foreign_q[k]);
}
// the flag array as a caller gave it: every entry 0 or 1, at least one 1.  Returns the flagged ids, ascending.
template <typename T>
std::vector<int32_t> alch_check_flags(const std::vector<T> &flag) {
    EMDEE_REQUIRE((int64_t)flag.size() <= INT32_MAX, EMDEE_ERR_INVALID, "set_alchemical: %lld atoms (at most 2^31 - 1)", (long long)flag.size());
    std::vector<int32_t> ids;
    for (size_t i = 0; i < flag.size(); i++) {
        EMDEE_REQUIRE(flag[i] == 0 || flag[i] == 1, EMDEE_ERR_INVALID, "set_alchemical: atom %lld has flag %lld (0: environment, 1: solute)",
                      (long long)i, (long long)flag[i]);
        if (flag[i] == 1) ids.push_back((int32_t)i);
    }
    EMDEE_REQUIRE(!ids.empty(), EMDEE_ERR_INVALID, "set_alchemical: no atom is flagged (the solute holds at least one atom; flag = NULL clears "
                  "the table)");
    return ids;
}
// a charged engine: the first flagged atom that carries a charge, or -1 (refused without the Coulomb stage, and with it under Ewald
// or PME: scale the solute's charges to zero with emdee_md_set_coulomb first)
inline int64_t alch_first_charged(const std::vector<int32_t> &flagged, const std::vector<double> &charge) {
    for (int32_t i : flagged)
        if (i >= 0 && (size_t)i < charge.size() && charge[(size_t)i] != 0.0) return i;
    return -1;
}

}  // namespace emdee

#if defined(__HIPCC__)
#include "kernels.hpp"
#include "reduce.hpp"

namespace emdee {

// ---- the row pass, right after a build (and after the exclusion filter: an entry that the exclusion or 1-4 tables struck is gone
// already and is never recorded).  flag: the caller's array, one int per caller id; an atom's own flag is flag[perm[slot]].
// at(e): the row's e-th entry (a reference); slot(entry): its cell-order slot, as kernels.hpp strike_row.
template <class At, class Slot>
__device__ __forceinline__ int alch_count_row(const int *__restrict__ flag, const int *__restrict__ perm, int p, int m, At at, Slot slot) {
    const int fi = flag[perm[p]];
    int c = 0;
    for (int e = 0; e < m; e++) c += flag[perm[slot(at(e))]] != fi ? 1 : 0;
    return c;
}
// the row compacted in place, the struck entries' slots to xs[0 .. count) in row order; returns the new length
template <class At, class Slot>
__device__ __forceinline__ int alch_strike_row(const int *__restrict__ flag, const int *__restrict__ perm, int p, int m, At at, Slot slot,
                                               int *__restrict__ xs) {
    const int fi = flag[perm[p]];
    int w = 0, c = 0;
    for (int e = 0; e < m; e++) {
        const auto ent = at(e);
        const int q = slot(ent);
        if (flag[perm[q]] != fi) { xs[c++] = q; continue; }
        if (w != e) at(w) = ent;
        w++;
    }
    return w;
}

// The scan array of the pass, 3 n + 4 ints: [0, n) the struck entries of every slot, [n, 2n) 1 for a solute owner, [2n, 3n) 1 for an
// environment owner, [3n] 0; after the exclusive scan the starts of the CSR and the ranks in the two owner lists, and k_alch_totals
// leaves the three totals in [3n + 1, 3n + 4) for the one read-back.
__device__ __forceinline__ void alch_put_count(int *__restrict__ scan, int n, int p, int c, int flagged) {
    scan[p] = c;
    scan[n + p] = (c > 0 && flagged) ? 1 : 0;
    scan[2 * (size_t)n + p] = (c > 0 && !flagged) ? 1 : 0;
}
static __global__ void k_alch_totals(int *__restrict__ scan, int n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        scan[3 * (size_t)n + 1] = scan[n];
        scan[3 * (size_t)n + 2] = scan[2 * (size_t)n] - scan[n];
        scan[3 * (size_t)n + 3] = scan[3 * (size_t)n] - scan[2 * (size_t)n];
    }
}
// One owner of struck entries: its cell-order slot, where its entries start in the CSR, and how many.  Solute owners first
// (owners[0 .. n_sol)), then the environment's, each list in cell order.
struct AlchOwner {
    int p, start, count;
};
__device__ __forceinline__ void alch_put_owner(const int *__restrict__ scan, int n, int p, int c, int flagged, AlchOwner *__restrict__ owners) {
    if (c == 0) return;
    const int n_sol = scan[2 * (size_t)n] - scan[n];
    const int rank = flagged ? scan[n + p] - scan[n] : n_sol + scan[2 * (size_t)n + p] - scan[2 * (size_t)n];
    owners[rank] = AlchOwner{p, scan[p], c};
}

// the direct (int32, cell-order slot) list
static __global__ void k_alch_count_rows(int n, int n_owned, const int *__restrict__ perm, const int *__restrict__ nbr, int stride,
                                         const int *__restrict__ cnt, const int *__restrict__ flag, int *__restrict__ scan) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int c = 0;
    const bool own = perm[p] < n_owned;
    if (own) {
        const int *row = nbr + (size_t)p * stride;
        c = alch_count_row(flag, perm, p, min(cnt[p], stride), [&](int e) { return row[e]; }, [](int q) { return q; });
    }
    alch_put_count(scan, n, p, c, own ? flag[perm[p]] : 0);
}
static __global__ void k_alch_strike_rows(int n, int n_owned, const int *__restrict__ perm, int *__restrict__ nbr, int stride,
                                          int *__restrict__ cnt, const int *__restrict__ flag, const int *__restrict__ scan,
                                          int *__restrict__ xs, AlchOwner *__restrict__ owners) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    const int c = scan[p + 1] - scan[p];                     // (scan[n] is the total: the CSR's end)
    if (c == 0) return;
    int *row = nbr + (size_t)p * stride;
    cnt[p] = alch_strike_row(flag, perm, p, min(cnt[p], stride), [&](int e) -> int & { return row[e]; }, [](int q) { return q; },
                             xs + scan[p]);
    alch_put_owner(scan, n, p, c, flag[perm[p]], owners);
}

// ---- the force kernel.  lambda and alpha are host scalars: emdee_md_set_lambda changes an argument, nothing on the device.
template <typename real>
struct AlchArgs {
    int n_sol, n_env;                                        // owners[0 .. n_sol): one wavefront each; then n_env: one thread each
    const AlchOwner *owners;
    const int *xs;
    size_t pitch;
    real lambda, alpha;
    AlchModel<real> sw;
    real rc2;
};
constexpr int ALCH_BLOCK = 256;
// the blocks of a launch: the solute owners' (ALCH_BLOCK / WAVE wavefronts each), then the environment owners'
EMDEE_HD int alch_sol_blocks(int n_sol) { return (n_sol + ALCH_BLOCK / WAVE - 1) / (ALCH_BLOCK / WAVE); }
EMDEE_HD int alch_env_blocks(int n_env) { return (n_env + ALCH_BLOCK - 1) / ALCH_BLOCK; }

// The Coulomb stage (emdee_md_set_alchemical_coulomb) of the same launch, the COUL instances: q the plane of sqrt(K) q per cell-order
// slot that the charged force kernels read (lj_pair.hpp Charges), so that qq is one product; lambda_q and beta host scalars as lambda.
template <typename real>
struct AlchCoulomb {
    const real *q;
    real lambda_q, beta;
    AlchRf<real> rf;
};
// what one lane or thread gathers over its entries (eq, wq, dlq: the Coulomb stage's U_q, W_q and dU/dlambda_q, kept apart from the
// Lennard-Jones words of a read; unused, and gone, in the instances without the stage)
template <typename real, bool TENSOR>
struct AlchAcc {
    real fx = 0, fy = 0, fz = 0, e = 0, w = 0, dl = 0, np = 0;
    real tv[6] = {0, 0, 0, 0, 0, 0};
    real eq = 0, wq = 0, dlq = 0;
};
template <typename real, bool TENSOR, bool COUL>
__device__ __forceinline__ void alch_entry(const AlchArgs<real> &a, const AlchCoulomb<real> &cq, const AtomView<real> &atoms,
                                           const GridP<real> &g, real xi, real yi, real zi, real hs_i, real te_i, real q_i, int q,
                                           AlchAcc<real, TENSOR> &s) {
    real xj, yj, zj, hs_j, te_j;
    load_atom(atoms, q, xj, yj, zj, hs_j, te_j);
    const real dx = min_image(xi - xj, g.plen[0], g.pinv[0]);
    const real dy = min_image(yi - yj, g.plen[1], g.pinv[1]);
    const real dz = min_image(zi - zj, g.plen[2], g.pinv[2]);
    const real r2 = dx * dx + dy * dy + dz * dz;
    if (!(r2 < a.rc2)) return;                               // CUTOFF semantics, as the list kernels
    const real sigma = hs_i + hs_j;
    real E, W, dEdl, wr2;
    alch_pair(r2, a.sw, sigma * sigma, te_i * te_j, a.lambda, a.alpha, E, W, dEdl, wr2);
    s.e += E; s.w += W; s.dl += dEdl; s.np += (real)1;
    if (COUL) {                                              // (wr2_lj + wr2_q) d: at lambda_q = 0 wr2_q is exactly 0, the force the uncharged one
        real Eq, Wq, dEdlq, wr2q;
        alch_coulomb_pair(r2, q_i * cq.q[q], cq.rf, cq.lambda_q, cq.beta, Eq, Wq, dEdlq, wr2q);
        s.eq += Eq; s.wq += Wq; s.dlq += dEdlq;
        wr2 += wr2q;
    }
    s.fx += wr2 * dx; s.fy += wr2 * dy; s.fz += wr2 * dz;
    if (TENSOR) {
        const real hx = wr2 * dx, hy = wr2 * dy, hz = wr2 * dz;
        s.tv[0] += hx * dx; s.tv[1] += hy * dy; s.tv[2] += hz * dz;
        s.tv[3] += hx * dy; s.tv[4] += hx * dz; s.tv[5] += hy * dz;
    }
}
// Owner o's sums into the planes under the mask, and its half of U, dU/dlambda, W and the pair count into part[o][0..4); COUL: U_q and
// W_q go to the planes with the Lennard-Jones words, and the owner's half of U_q, dU/dlambda_q and W_q to part_q[o][0..3)
template <typename real, bool TENSOR, bool COUL>
__device__ __forceinline__ void alch_write(const AlchArgs<real> &a, int o, int p, const AlchAcc<real, TENSOR> &s, int bitmask,
                                           real *__restrict__ frc, real *__restrict__ en, real *__restrict__ vir, real *__restrict__ vt,
                                           double *__restrict__ part, double *__restrict__ part_q) {
    const real h = (real)0.5;
    if (bitmask & EMDEE_FORCES) { frc[p] += s.fx; frc[a.pitch + p] += s.fy; frc[2 * a.pitch + p] += s.fz; }
    if (bitmask & EMDEE_ENERGIES) en[p] += h * (COUL ? s.e + s.eq : s.e);
    if (bitmask & EMDEE_VIRIALS) vir[p] += h * (COUL ? s.w + s.wq : s.w);
    if (TENSOR)
        for (int c = 0; c < 6; c++) vt[c * a.pitch + p] += h * s.tv[c];
    double *out = part + (size_t)ALCH_SUMS * o;
    out[0] = 0.5 * (double)s.e; out[1] = 0.5 * (double)s.dl; out[2] = 0.5 * (double)s.w; out[3] = 0.5 * (double)s.np;
    if (COUL) {
        double *oq = part_q + (size_t)ALCH_COULOMB_SUMS * o;
        oq[0] = 0.5 * (double)s.eq; oq[1] = 0.5 * (double)s.dlq; oq[2] = 0.5 * (double)s.wq;
    }
}
// (TENSOR: the tensor pass's instance; the force and the observable passes keep the instance without the six sums, as k_pairs14.
// COUL: the Coulomb stage on a charged engine; the instances without it never touch cq or part_q)
template <typename real, bool TENSOR, bool COUL>
__global__ __launch_bounds__(ALCH_BLOCK) void k_alchemical(AlchArgs<real> a, AlchCoulomb<real> cq, AtomView<real> atoms, GridP<real> g,
                                                            int bitmask, real *__restrict__ frc, real *__restrict__ en,
                                                            real *__restrict__ vir, real *__restrict__ vt, double *__restrict__ part,
                                                            double *__restrict__ part_q) {
    const int sol_blocks = alch_sol_blocks(a.n_sol);
    AlchAcc<real, TENSOR> s;
    if ((int)blockIdx.x < sol_blocks) {                      // one wavefront per solute owner, lanes over its entries
        const int o = blockIdx.x * (ALCH_BLOCK / WAVE) + threadIdx.x / WAVE;
        if (o >= a.n_sol) return;                            // (a whole wavefront leaves)
        const AlchOwner ow = a.owners[o];
        real xi, yi, zi, hs_i, te_i;
        load_atom(atoms, ow.p, xi, yi, zi, hs_i, te_i);
        const real q_i = COUL ? cq.q[ow.p] : (real)0;
        const int lane = threadIdx.x & (WAVE - 1);
        for (int k = lane; k < ow.count; k += WAVE)
            alch_entry<real, TENSOR, COUL>(a, cq, atoms, g, xi, yi, zi, hs_i, te_i, q_i, a.xs[ow.start + k], s);
        s.fx = wave_sum_to_lane63(s.fx); s.fy = wave_sum_to_lane63(s.fy); s.fz = wave_sum_to_lane63(s.fz);
        s.e = wave_sum_to_lane63(s.e); s.w = wave_sum_to_lane63(s.w); s.dl = wave_sum_to_lane63(s.dl); s.np = wave_sum_to_lane63(s.np);
        if (TENSOR)
            for (int c = 0; c < 6; c++) s.tv[c] = wave_sum_to_lane63(s.tv[c]);
        if (COUL) { s.eq = wave_sum_to_lane63(s.eq); s.wq = wave_sum_to_lane63(s.wq); s.dlq = wave_sum_to_lane63(s.dlq); }
        if (lane == WAVE - 1) alch_write<real, TENSOR, COUL>(a, o, ow.p, s, bitmask, frc, en, vir, vt, part, part_q);
        return;
    }
    const int o = a.n_sol + ((int)blockIdx.x - sol_blocks) * ALCH_BLOCK + threadIdx.x;   // one thread per environment owner
    if (o >= a.n_sol + a.n_env) return;
    const AlchOwner ow = a.owners[o];
    real xi, yi, zi, hs_i, te_i;
    load_atom(atoms, ow.p, xi, yi, zi, hs_i, te_i);
    const real q_i = COUL ? cq.q[ow.p] : (real)0;
    for (int k = 0; k < ow.count; k++) alch_entry<real, TENSOR, COUL>(a, cq, atoms, g, xi, yi, zi, hs_i, te_i, q_i, a.xs[ow.start + k], s);
    alch_write<real, TENSOR, COUL>(a, o, ow.p, s, bitmask, frc, en, vir, vt, part, part_q);
}
// The energies-only instance: U_alch at K foreign lambdas at the current positions.  Every cross pair has exactly one solute atom,
// and every solute atom is owned: the solute owners' wavefronts alone see each pair once, so the whole E goes to part[o][0 .. K).
// COUL: a second set of accumulators, U_q at the K foreign lambda_q, to part_q[o][0 .. K).
template <typename real>
struct AlchForeign {
    int K;
    real lambda[ALCH_MAX_FOREIGN];
    real lambda_q[ALCH_MAX_FOREIGN];
};
template <typename real, bool COUL>
__global__ __launch_bounds__(ALCH_BLOCK) void k_alchemical_foreign(AlchArgs<real> a, AlchCoulomb<real> cq, AtomView<real> atoms, GridP<real> g,
                                                                    AlchForeign<real> f, double *__restrict__ part,
                                                                    double *__restrict__ part_q) {
    const int o = blockIdx.x * (ALCH_BLOCK / WAVE) + threadIdx.x / WAVE;
    if (o >= a.n_sol) return;
    const AlchOwner ow = a.owners[o];
    real xi, yi, zi, hs_i, te_i;
    load_atom(atoms, ow.p, xi, yi, zi, hs_i, te_i);
    const real q_i = COUL ? cq.q[ow.p] : (real)0;
    const int lane = threadIdx.x & (WAVE - 1);
    real e[ALCH_MAX_FOREIGN], eq[ALCH_MAX_FOREIGN];
#pragma unroll
    for (int k = 0; k < ALCH_MAX_FOREIGN; k++) { e[k] = 0; eq[k] = 0; }
    for (int c = lane; c < ow.count; c += WAVE) {
        real xj, yj, zj, hs_j, te_j;
        const int q = a.xs[ow.start + c];
        load_atom(atoms, q, xj, yj, zj, hs_j, te_j);
        const real dx = min_image(xi - xj, g.plen[0], g.pinv[0]);
        const real dy = min_image(yi - yj, g.plen[1], g.pinv[1]);
        const real dz = min_image(zi - zj, g.plen[2], g.pinv[2]);
        const real r2 = dx * dx + dy * dy + dz * dz;
        if (!(r2 < a.rc2)) continue;
        const real sigma = hs_i + hs_j;
        const real qq = COUL ? q_i * cq.q[q] : (real)0;
#pragma unroll
        for (int k = 0; k < ALCH_MAX_FOREIGN; k++) {
            if (k >= f.K) continue;
            real E, W, dEdl, wr2;
            alch_pair(r2, a.sw, sigma * sigma, te_i * te_j, f.lambda[k], a.alpha, E, W, dEdl, wr2);
            e[k] += E;
            if (COUL) {
                alch_coulomb_pair(r2, qq, cq.rf, f.lambda_q[k], cq.beta, E, W, dEdl, wr2);
                eq[k] += E;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < ALCH_MAX_FOREIGN; k++) {
        const real t = wave_sum_to_lane63(e[k]);
        if (lane == WAVE - 1) part[(size_t)ALCH_MAX_FOREIGN * o + k] = (double)t;
        if (COUL) {
            const real tq = wave_sum_to_lane63(eq[k]);
            if (lane == WAVE - 1) part_q[(size_t)ALCH_MAX_FOREIGN * o + k] = (double)tq;
        }
    }
}

// ---- the sums (reduce.hpp Terms over the owners' partials): the order depends on the owner lists alone, which depend on the state alone
struct AlchSums {
    static constexpr int SUMS = ALCH_SUMS, MAXES = 0;
    const double *part;
    __device__ void operator()(int o, double *acc) const {
        for (int w = 0; w < ALCH_SUMS; w++) acc[w] += part[(size_t)ALCH_SUMS * o + w];
    }
};
struct AlchForeignSums {
    static constexpr int SUMS = 8, MAXES = 0;                // (RED_MAX_WORDS is 12: sixteen foreign energies go in two halves)
    const double *part;
    int first;
    __device__ void operator()(int o, double *acc) const {
        for (int w = 0; w < 8; w++) acc[w] += part[(size_t)ALCH_MAX_FOREIGN * o + first + w];
    }
};
// the Coulomb stage's sums, in slots of their own: every owner's half of U_q, dU/dlambda_q and W_q; the solute owners' U_q at the
// foreign lambda_q
struct AlchCoulombSums {
    static constexpr int SUMS = ALCH_COULOMB_SUMS, MAXES = 0;
    const double *part;
    __device__ void operator()(int o, double *acc) const {
        for (int w = 0; w < ALCH_COULOMB_SUMS; w++) acc[w] += part[(size_t)ALCH_COULOMB_SUMS * o + w];
    }
};
struct AlchCoulombForeignSums {
    static constexpr int SUMS = 8, MAXES = 0;
    const double *part;
    int first;
    __device__ void operator()(int o, double *acc) const {
        for (int w = 0; w < 8; w++) acc[w] += part[(size_t)ALCH_MAX_FOREIGN * o + first + w];
    }
};
// stage 1 of both sums under the family's own name (reduce_partials is the body, as molecule.hpp k_molecule_partials); stage 2 is
// k_reduce_final
template <class Term>
__global__ __launch_bounds__(RED_BLOCK) void k_alch_partials(int n, Term term, double *__restrict__ partial) {
    __shared__ double sh[RED_BLOCK / WAVE];
    reduce_partials(n, term, partial, sh);
}
// What the closing launch of a pass leaves in the table's words: out[0 .. ALCH_WORDS) from the four totals; log_slot >= 0: the
// entry {dU/dlambda, U_alch, K foreign energies} of the on-device log (the foreign totals were queued before it).
static __global__ void k_alch_finish(double lambda, const double *__restrict__ tot, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = lambda; out[1] = tot[0]; out[2] = tot[1]; out[3] = tot[2]; out[4] = tot[3];
}
// the Coulomb stage's words: out[0 .. ALCH_COULOMB_WORDS) from the three totals
static __global__ void k_alch_coulomb_finish(double lambda_q, const double *__restrict__ tot, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = lambda_q; out[1] = tot[0]; out[2] = tot[1]; out[3] = tot[2];
}
static __global__ void k_alch_zero_words(double lambda, double *__restrict__ out, int n) {
    const int t = threadIdx.x;
    if (t < n) out[t] = t == 0 ? lambda : 0.0;
}
static __global__ void k_alch_log(const double *__restrict__ out, int K, double *__restrict__ entry) {
    const int t = threadIdx.x;
    if (t == 0) entry[0] = out[2];
    if (t == 1) entry[1] = out[1];
    if (t >= 2 && t < 2 + K) entry[t] = out[ALCH_WORDS + t - 2];
}
// the second log's entry {dU/dlambda_q, U_q, K foreign U_q}, at the same pass as the first log's
static __global__ void k_alch_coulomb_log(const double *__restrict__ out, int K, double *__restrict__ entry) {
    const int t = threadIdx.x;
    if (t == 0) entry[0] = out[2];
    if (t == 1) entry[1] = out[1];
    if (t >= 2 && t < 2 + K) entry[t] = out[ALCH_COULOMB_WORDS + t - 2];
}

}  // namespace emdee
#endif
