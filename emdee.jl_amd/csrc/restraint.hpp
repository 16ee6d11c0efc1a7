// restraint.hpp -- position restraints (emdee_md_set_restraints): an external field that ties named atoms to reference points, harmonic
// per axis or flat-bottomed, with references that follow the box.  One more post term behind a force pass (NbSystem::add_restraints,
// next to add_pairs14, add_bonded, add_ewald): one thread per table entry finds its atom through inv_perm, forms d = x_unwrapped - ref
// in fp64 from the record, the image count and, for Float32, the cell origin (k_unsort's expression, as k_msd_gather), and adds the
// atom's whole term to the planes the pass's mask asks for.  Each atom is named once: plain read-modify-writes, no atomics, the same
// bits in every run.  No minimum image anywhere: an atom that walks through a box face or is re-sorted sees a continuous force.
// The parts with no HIP in them -- the term of one atom and the scaling of a reference -- are plain C++ at the top, as the top of gk.hpp
// is: a stand-alone host program tests them with the host compiler (tests/c/restraint_host.cpp); the kernels below them need HIP.
// DESIGN.md 4j has the algorithm; MdImpl::set_restraints (impl.hpp) installs a table.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int RESTRAINT_WORDS = 8;                           // (EMDEE_RESTRAINT_WORDS)

// ---- the term of one atom
// d: x_unwrapped - ref; k: the spring constants per axis (each >= 0); r0 >= 0: the flat-bottom radius.  Returns U; f: the force on the
// atom; T: the symmetrised d (x) f in the order (xx, yy, zz, xy, xz, yz), so that T[0] + T[1] + T[2] = d . f.  The arithmetic is fp64
// whatever `real` is; f and T are rounded once, to the precision of the planes they are added to.
//   r0 = 0: U = 1/2 sum_a k_a d_a^2, f_a = -k_a d_a.
//   r0 > 0: the non-zero constants are one value k (the builder refuses anything else); rho is the norm of d over the axes with
//           k_a > 0 (a sphere, a cylinder or a slab); U = 1/2 k max(0, rho - r0)^2, f along the masked d, exactly 0 inside the well:
//           no division happens when rho <= r0.
template <typename real>
EMDEE_HD double restraint_term(const double d[3], const double k[3], double r0, real f[3], real T[6]) {
    double g[3] = {0.0, 0.0, 0.0}, U = 0.0;                  // g: the force in fp64
    if (!(r0 > 0.0)) {
        for (int a = 0; a < 3; a++) {
            g[a] = -k[a] * d[a];
            U += 0.5 * k[a] * d[a] * d[a];
        }
    } else {
        double rho2 = 0.0, kk = 0.0;
        for (int a = 0; a < 3; a++)
            if (k[a] > 0.0) { rho2 += d[a] * d[a]; kk = k[a]; }
        const double rho = sqrt(rho2);
        if (rho > r0) {
            const double s = rho - r0, c = -kk * s / rho;
            for (int a = 0; a < 3; a++) g[a] = k[a] > 0.0 ? c * d[a] : 0.0;
            U = 0.5 * kk * s * s;
        }
    }
    for (int a = 0; a < 3; a++) f[a] = (real)g[a];
    T[0] = (real)(d[0] * g[0]); T[1] = (real)(d[1] * g[1]); T[2] = (real)(d[2] * g[2]);
    T[3] = (real)(0.5 * (d[0] * g[1] + d[1] * g[0]));
    T[4] = (real)(0.5 * (d[0] * g[2] + d[2] * g[0]));
    T[5] = (real)(0.5 * (d[1] * g[2] + d[2] * g[1]));
    return U;
}

// ---- the references follow the box (emdee_md_scale_box, every barostat event): ref <- lo + mu (ref - lo) per axis.  An atom scaled
// the same way keeps d -> mu d.  A factor of exactly 1 leaves the reference its bits, as it leaves the atom's coordinate
// (kernels.hpp k_cell_state_scale).
EMDEE_HD double restraint_scale_ref(double ref, double lo, double mu) { return mu == 1.0 ? ref : lo + mu * (ref - lo); }

}  // namespace emdee

#if defined(__HIPCC__)
#include "kernels.hpp"

namespace emdee {

// The table (Topology::restraints) and where the atoms are.  atoms: one caller id per entry; ref, k: three doubles per entry; flat: one.
template <typename real>
struct RestraintArgs {
    int n, n_owned, n_total;
    const int *atoms;
    const double *ref, *k, *flat;
    const int *inv_perm, *img;
    const Rec<real> *rec;
    RelGrid rel;
    double len[3];
    size_t pitch;
};

// the slot of entry e's atom, or -1 (an id or a slot outside the state: the host refuses such a table before any launch)
template <typename real>
__device__ __forceinline__ int restraint_slot(const RestraintArgs<real> &a, int e) {
    const int id = a.atoms[e];
    if (id < 0 || id >= a.n_owned) return -1;
    const int p = a.inv_perm[id];
    return (p >= 0 && p < a.n_total) ? p : -1;
}
// the unwrapped coordinates of slot p, in fp64: k_unsort's expression (a Float32 engine adds its cell origin and the box lengths in
// double, as k_msd_gather does; an fp64 engine's are bit for bit what emdee_md_get_state returns)
template <typename real>
__device__ __forceinline__ void restraint_unwrapped(const RestraintArgs<real> &a, int p, double x[3]) {
    const Rec<real> r = a.rec[p];
    int kx, ky, kz;
    img_unpack(a.img[p], kx, ky, kz);
    x[0] = (double)r.x; x[1] = (double)r.y; x[2] = (double)r.z;
    if (sizeof(real) == 4 && a.rel.on) {
        double ox, oy, oz;
        a.rel.origin(a.rel.cell[p], ox, oy, oz);
        x[0] += ox; x[1] += oy; x[2] += oz;
    }
    x[0] += (double)kx * a.len[0]; x[1] += (double)ky * a.len[1]; x[2] += (double)kz * a.len[2];
}
// d, k and r0 of entry e whose atom sits in slot p
template <typename real>
__device__ __forceinline__ void restraint_entry(const RestraintArgs<real> &a, int e, int p, double d[3], double k[3], double &r0) {
    double x[3];
    restraint_unwrapped(a, p, x);
    for (int c = 0; c < 3; c++) { d[c] = x[c] - a.ref[3 * (size_t)e + c]; k[c] = a.k[3 * (size_t)e + c]; }
    r0 = a.flat[e];
}

// One thread per table entry: the atom's whole term into the planes the mask asks for (TENSOR: the tensor pass, six planes of vt).
template <typename real, bool TENSOR>
__global__ __launch_bounds__(256) void k_restraints(RestraintArgs<real> a, int bitmask, real *__restrict__ frc, real *__restrict__ en,
                                                    real *__restrict__ vir, real *__restrict__ vt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n) return;
    const int p = restraint_slot(a, e);
    if (p < 0) return;
    double d[3], k[3], r0;
    restraint_entry(a, e, p, d, k, r0);
    real f[3], T[6];
    const double U = restraint_term<real>(d, k, r0, f, T);
    if (bitmask & EMDEE_FORCES) { frc[p] += f[0]; frc[a.pitch + p] += f[1]; frc[2 * a.pitch + p] += f[2]; }
    if (bitmask & EMDEE_ENERGIES) en[p] += (real)U;
    if (bitmask & EMDEE_VIRIALS) vir[p] += T[0] + T[1] + T[2];
    if (TENSOR)
        for (int c = 0; c < 6; c++) vt[c * a.pitch + p] += T[c];
}

// ref of every entry <- its atom's current unwrapped coordinates (emdee_md_set_restraints with ref NULL: d = 0 exactly, in both precisions)
template <typename real>
__global__ __launch_bounds__(256) void k_restraint_capture(RestraintArgs<real> a, double *__restrict__ ref) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n) return;
    const int p = restraint_slot(a, e);
    if (p < 0) return;
    double x[3];
    restraint_unwrapped(a, p, x);
    for (int c = 0; c < 3; c++) ref[3 * (size_t)e + c] = x[c];
}

// One thread per entry: the references follow the box.
static __global__ __launch_bounds__(256) void k_restraint_scale(int n, double *__restrict__ ref, ScaleBox s) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    for (int c = 0; c < 3; c++) ref[3 * (size_t)e + c] = restraint_scale_ref(ref[3 * (size_t)e + c], s.lo[c], s.mu[c]);
}

// The term of emdee_md_restraint_sums (reduce.hpp), over the entries of the table, fp64 in both precisions: [0] = sum U, [1..6] = sum of
// the tensors, [7] = the largest |d| (all three axes).
template <typename real>
struct RestraintSums {
    static constexpr int SUMS = 7, MAXES = 1;
    static_assert(SUMS + MAXES == RESTRAINT_WORDS, "emdee_md_restraint_sums returns RESTRAINT_WORDS words");
    RestraintArgs<real> a;
    __device__ __forceinline__ void operator()(int e, double *s) const {
        const int p = restraint_slot(a, e);
        if (p < 0) return;
        double d[3], k[3], r0, f[3], T[6];
        restraint_entry(a, e, p, d, k, r0);
        s[0] += restraint_term<double>(d, k, r0, f, T);
        for (int c = 0; c < 6; c++) s[1 + c] += T[c];
        s[7] = fmax(s[7], sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
    }
};

}  // namespace emdee
#endif
