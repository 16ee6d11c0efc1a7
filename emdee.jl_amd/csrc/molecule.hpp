// molecule.hpp -- whole molecules of any size (emdee_md_set_molecules): the molecular sums and the molecular scale over a per-atom
// molecule table, for engines whose constraint groups are not all three-site molecules (an hbonds table) and for flexible molecules.
// The molecular pressure is exact for any partition of the atoms into groups as long as every constraint lies inside one group
// (DESIGN.md 4c-2), so the unit here is whatever the caller names a molecule.  Three kernels, ordered by the stream:
//   (1) k_molecule_centres   per molecule M, the unwrapped position of its first atom, Y - x_first and V: one thread per small molecule
//                            (<= MOL_SMALL atoms, sorted by size so that the lanes of a wavefront run the same trip count), one
//                            wavefront per large one (a strided loop, then wave_sum_to_lane63);
//   (2) MoleculeAtomSums     a Term of reduce.hpp over the table's entries (the molecular sums; stage 1 is k_molecule_partials), or
//       k_molecule_shift     one thread per entry (the molecular scale).
// No atomics on the state; the order of every sum is a function of the table alone, never of the CU count: the same bits in every run.
// Centres of mass are formed in fp64 from UNWRAPPED coordinates (restraint_unwrapped: the record plus the image counts), every
// difference relative to the molecule's first atom: a molecule may be larger than half a box, and the caller loads it whole.
// The parts with no HIP in them -- one atom's share of a centre, the centre, one entry's twelve words, one entry's shift -- are plain
// C++ at the top, as the top of pull.hpp is: a stand-alone host program tests them with the host compiler
// (tests/c/molecule_host.cpp); the kernels below them need HIP.  topology.hpp builds the table (topo::molecule_table).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int MOL_SMALL = 8;                                 // molecules of up to this many atoms take one thread each
constexpr int MOL_ACC = 7;                                   // the words of a centre while it is summed: M, m (x - x_first), m (v - v_first)
constexpr int MOL_CENTRE = 10;                               // a finished centre: M, x_first (3), Y - x_first (3), V (3)

// ---- a centre of mass
// one atom's share: x, v its unwrapped position and velocity, x1, v1 those of the molecule's first atom.  A massless atom (a
// virtual site) adds exactly 0.
EMDEE_HD void molecule_centre_add(double m, const double x[3], const double v[3], const double x1[3], const double v1[3], double acc[MOL_ACC]) {
    acc[0] += m;
    for (int c = 0; c < 3; c++) {
        acc[1 + c] += m * (x[c] - x1[c]);
        acc[4 + c] += m * (v[c] - v1[c]);
    }
}
// acc -> the centre.  A molecule of mass 0 (refused at the set) gets Y = x_first and V = v_first: no division happens.
EMDEE_HD void molecule_centre_finish(const double acc[MOL_ACC], const double x1[3], const double v1[3], double out[MOL_CENTRE]) {
    const double inv = acc[0] > 0.0 ? 1.0 / acc[0] : 0.0;
    out[0] = acc[0];
    for (int c = 0; c < 3; c++) {
        out[1 + c] = x1[c];
        out[4 + c] = acc[1 + c] * inv;
        out[7 + c] = v1[c] + acc[4 + c] * inv;
    }
}

// ---- one entry's share of the molecular sums: out[0..5] += 1/2 (d^a f^b + d^b f^a), out[6..11] += m u^a u^b in the order (xx, yy,
// zz, xy, xz, yz), with d = (x - x_first) - (Y - x_first) and u = v - V: settle.hpp molecule_sums' cancellation-free form, one atom
// at a time.  Summed over a molecule's atoms they are sum_k sym(d_k (x) f_k) and sum_k m_k v_k (x) v_k - M V (x) V.
EMDEE_HD void molecule_entry_sums(double m, const double x[3], const double v[3], const double f[3], const double centre[MOL_CENTRE],
                                  double out[12]) {
    double d[3], u[3];
    for (int c = 0; c < 3; c++) {
        d[c] = (x[c] - centre[1 + c]) - centre[4 + c];
        u[c] = v[c] - centre[7 + c];
    }
    const int ca[6] = {0, 1, 2, 0, 0, 1}, cb[6] = {0, 1, 2, 1, 2, 2};
    for (int q = 0; q < 6; q++) {
        const int a = ca[q], b = cb[q];
        out[q] += 0.5 * (d[a] * f[b] + d[b] * f[a]);
        out[6 + q] += m * u[a] * u[b];
    }
}

// ---- one entry's share of the molecular scale: the record whose image counts are k (kl = k len, the box lengths it stands away
// from its unwrapped position) moves by shift = (mu - 1) (Y - k len - lo), the image of the centre that goes with the record, so that
// the stored counts stay valid on the scaled box: r' + k (mu len) = (r + k len) + (mu - 1) (Y - lo).  dv = (velocity_scale - 1) V.
// A factor of exactly 1 gives a shift of exactly 0.
EMDEE_HD void molecule_entry_shift(const double centre[MOL_CENTRE], const double kl[3], const double mu[3], const double lo[3],
                                   double velocity_scale, double shift[3], double dv[3]) {
    for (int c = 0; c < 3; c++) {
        shift[c] = (mu[c] - 1.0) * (((centre[1 + c] - kl[c]) + centre[4 + c]) - lo[c]);
        dv[c] = (velocity_scale - 1.0) * centre[7 + c];
    }
}

}  // namespace emdee

#if defined(__HIPCC__)
#include "kernels.hpp"
#include "pull.hpp"
#include "reduce.hpp"

namespace emdee {

// The table (Topology::molecules) and where the atoms are.  start, atoms: the CSR of the molecules of two atoms and more in table
// order (small ones first), caller ids ascending within a molecule; entry_mol: the molecule of every entry; centres: MOL_CENTRE
// doubles per molecule, written by (1) and read by (2).  r: the state as the restraint kernels see it (r.atoms = atoms, r.n = the
// entries); rec: the same records, to be written.
template <typename real>
struct MoleculeArgs {
    int n_mol, n_small;
    const int *start, *entry_mol;
    double *centres;
    RestraintArgs<real> r;
    Rec<real> *rec;
    real *vel;
    const real *inv_mass;
};

// position, velocity and mass of entry e (slot p)
template <typename real>
__device__ __forceinline__ void molecule_atom(const MoleculeArgs<real> &a, int p, double x[3], double v[3], double &m) {
    restraint_unwrapped(a.r, p, x);
    for (int c = 0; c < 3; c++) v[c] = (double)a.vel[c * a.r.pitch + p];
    m = pull_mass(a.inv_mass, p);
}

// (1) The centres.  Blocks [0, small_blocks): one thread per small molecule, a loop over its atoms in table order.  The blocks
// behind them: one wavefront per large molecule; lane l takes entries first + l, first + l + 64, ..., the seven words go through the
// fixed-order DPP reduction and lane 63 writes.  Every lane of a wavefront that reduces is active (a wavefront without a molecule
// leaves as a whole).
template <typename real>
__global__ __launch_bounds__(256) void k_molecule_centres(MoleculeArgs<real> a, int small_blocks) {
    const bool large = (int)blockIdx.x >= small_blocks;
    const int mol = large ? a.n_small + ((int)blockIdx.x - small_blocks) * (256 / WAVE) + (int)threadIdx.x / WAVE
                          : (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (mol >= (large ? a.n_mol : a.n_small)) return;
    const int first = a.start[mol], end = a.start[mol + 1];
    const int p1 = restraint_slot(a.r, first);
    if (p1 < 0) return;                                      // (an id or a slot outside the state: the host refuses such a table)
    double x1[3], v1[3], m1, acc[MOL_ACC];
    molecule_atom(a, p1, x1, v1, m1);
    for (int w = 0; w < MOL_ACC; w++) acc[w] = 0.0;
    const int lane = large ? (int)threadIdx.x & (WAVE - 1) : 0, stride = large ? WAVE : 1;
    for (int e = first + lane; e < end; e += stride) {
        const int p = restraint_slot(a.r, e);
        if (p < 0) continue;
        double x[3], v[3], m;
        molecule_atom(a, p, x, v, m);
        molecule_centre_add(m, x, v, x1, v1, acc);
    }
    if (large) {
#pragma unroll
        for (int w = 0; w < MOL_ACC; w++) acc[w] = wave_sum_to_lane63(acc[w]);
        if (lane != WAVE - 1) return;
    }
    double out[MOL_CENTRE];
    molecule_centre_finish(acc, x1, v1, out);
    for (int w = 0; w < MOL_CENTRE; w++) a.centres[MOL_CENTRE * (size_t)mol + w] = out[w];
}

// (2) The term of the molecular sums (reduce.hpp), over the entries of the table: [0..11] = the sum of molecule_entry_sums.  frc: the
// engine's force planes (the force-field forces of the last force pass; a virtual site's are 0 after spreading).
template <typename real>
struct MoleculeAtomSums {
    static constexpr int SUMS = TENSOR_SUMS, MAXES = 0;
    MoleculeArgs<real> a;
    const real *frc;
    __device__ __forceinline__ void operator()(int e, double *sum) const {
        const int p = restraint_slot(a.r, e);
        if (p < 0) return;
        double x[3], v[3], f[3], m;
        molecule_atom(a, p, x, v, m);
        for (int c = 0; c < 3; c++) f[c] = (double)frc[c * a.r.pitch + p];
        molecule_entry_sums(m, x, v, f, a.centres + MOL_CENTRE * (size_t)a.entry_mol[e], sum);
    }
};

// ... and its stage 1 under the family's own name (stage 2 is k_reduce_final): the same blocks, the same order, the same partials as
// k_reduce_partials<MoleculeAtomSums> would write
template <typename real>
__global__ __launch_bounds__(RED_BLOCK) void k_molecule_partials(int n, MoleculeAtomSums<real> term, double *__restrict__ partial) {
    __shared__ double sh[RED_BLOCK / WAVE];
    reduce_partials(n, term, partial, sh);
}

// (2) The molecular scale, one thread per entry: the shift is added to the record in its own frame in double and rounded once, as
// k_constraint_positions adds its corrections.  scale_vel: v += (velocity_scale - 1) V; 0 leaves the velocity planes untouched, bit
// for bit.  k_cell_state_scale, given the membership bytes, passes these atoms over.
template <typename real>
__global__ __launch_bounds__(256) void k_molecule_shift(MoleculeArgs<real> a, ScaleBox sb, double velocity_scale, int scale_vel) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.r.n) return;
    const int p = restraint_slot(a.r, e);
    if (p < 0) return;
    int kx, ky, kz;
    img_unpack(a.r.img[p], kx, ky, kz);
    const double kl[3] = {(double)kx * a.r.len[0], (double)ky * a.r.len[1], (double)kz * a.r.len[2]};
    double shift[3], dv[3];
    molecule_entry_shift(a.centres + MOL_CENTRE * (size_t)a.entry_mol[e], kl, sb.mu, sb.lo, velocity_scale, shift, dv);
    Rec<real> r = a.rec[p];
    r.x = (real)((double)r.x + shift[0]); r.y = (real)((double)r.y + shift[1]); r.z = (real)((double)r.z + shift[2]);
    a.rec[p] = r;
    if (scale_vel) {
#pragma unroll
        for (int c = 0; c < 3; c++) a.vel[c * a.r.pitch + p] = (real)((double)a.vel[c * a.r.pitch + p] + dv[c]);
    }
}

// ---- the check of a table against a loaded state (emdee_md_set_molecules, and again at emdee_md_set_state), behind (1).
// words[0] = a molecule + 1 whose total mass is 0 (the highest such molecule).
static __global__ __launch_bounds__(256) void k_molecule_check_mass(int n_mol, const double *__restrict__ centres, int *__restrict__ words) {
    const int mol = blockIdx.x * blockDim.x + threadIdx.x;
    if (mol >= n_mol) return;
    if (!(centres[MOL_CENTRE * (size_t)mol] > 0.0)) atomicMax(words, mol + 1);
}
// words[1] = a molecule + 1 that is not loaded whole: one thread per group of a constraint table in force (groups: `sites` caller
// ids per group, -1 in unused trailing slots; geom: `ngeom` doubles per group -- sites = 3: {d_leg, d_base} of a triangle, sites =
// 4: the three centre-satellite distances of a star); the UNWRAPPED distance of two constrained sites is off its table entry by more
// than 1e-3 (relative), where the minimum image the constraint kernels take is not.  mol_of: the molecule of every caller id.
template <typename real>
__global__ __launch_bounds__(256) void k_molecule_check_whole(RestraintArgs<real> r, int n_groups, int sites, const int *__restrict__ groups,
                                                              const double *__restrict__ geom, const int *__restrict__ mol_of,
                                                              int *__restrict__ words) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const int id0 = groups[(size_t)sites * g];
    if (id0 < 0 || id0 >= r.n_owned) return;
    double x0[3], xp[3] = {0.0, 0.0, 0.0};                   // the first site, the site before this one
    restraint_unwrapped(r, r.inv_perm[id0], x0);
    bool off = false;
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const int id = k < sites ? groups[(size_t)sites * g + k] : -1;
        if (id < 0 || id >= r.n_owned) continue;             // (unused slots are the trailing ones)
        double x[3];
        restraint_unwrapped(r, r.inv_perm[id], x);
        const double d = sites == 3 ? geom[2 * (size_t)g] : geom[3 * (size_t)g + k - 1];
        const double dx = x[0] - x0[0], dy = x[1] - x0[1], dz = x[2] - x0[2];
        off = off || !(fabs(sqrt(dx * dx + dy * dy + dz * dz) - d) <= 1e-3 * d);
        if (sites == 3 && k == 2) {                          // the base of a triangle
            const double b = geom[2 * (size_t)g + 1];
            const double bx = x[0] - xp[0], by = x[1] - xp[1], bz = x[2] - xp[2];
            off = off || !(fabs(sqrt(bx * bx + by * by + bz * bz) - b) <= 1e-3 * b);
        }
        xp[0] = x[0]; xp[1] = x[1]; xp[2] = x[2];
    }
    if (off && mol_of[id0] >= 0) atomicMax(words + 1, mol_of[id0] + 1);
}

}  // namespace emdee
#endif
