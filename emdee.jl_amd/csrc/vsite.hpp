// vsite.hpp -- virtual interaction sites (emdee_md_set_vsites): massless particles that carry interactions and sit at a fixed
// linear combination of two or three atoms with mass, the fourth site of the TIP4P family and of OPC.  Placement and force
// spreading are the two functions at the top, plain C++ on doubles as the tops of settle.hpp and shake.hpp are: a stand-alone host
// program tests them with the host compiler (tests/c/vsite_host.cpp); the kernels below them need HIP.
//   x_s = x_a + w_b mi(x_b - x_a) + w_c mi(x_c - x_a)            (mi: the minimum image; GROMACS' site types 2 and 3)
//   f_a += (1 - w_b - w_c) f_s,  f_b += w_b f_s,  f_c += w_c f_s,  then f_s = 0
// Placement is linear in the parents, so spreading is its exact transpose: sum_k x_k (x) (w_k f_s) = x_s (x) f_s on unwrapped
// coordinates, and the box sums of energies, virials and tensors need nothing.  Out-of-plane sites (TIP5P's lone pairs: a cross
// product of the two legs) are not linear in this sense and are a follow-up.
#pragma once

#include "settle.hpp"

namespace emdee {

// d = x_b - x_a and e = x_c - x_a as minimum images (a two-parent site: w_c = 0 and e = 0), x_a in whichever frame: the site in
// that frame
EMDEE_HD void vsite_place(const double (&xa)[3], const double (&d)[3], const double (&e)[3], double w_b, double w_c, double (&x)[3]) {
    for (int c = 0; c < 3; c++) x[c] = xa[c] + (w_b * d[c] + w_c * e[c]);
}
// the minimum image of a difference along one axis (settle_detail::image on the host as well)
EMDEE_HD double vsite_image(double d, double len, int periodic) { return periodic ? d - len * rint(d / len) : d; }

// One parent's share: f += sum over the parent's entries [first, last) of weight[e] * (the force on site[e]), in entry order -- the
// order of the table, so the sum does not depend on a schedule.  site_force(s, fs): the force on table entry s.
template <class SiteForce>
EMDEE_HD void vsite_spread_parent(const int *site, const double *weight, int first, int last, SiteForce &&site_force, double (&f)[3]) {
    for (int e = first; e < last; e++) {
        double fs[3];
        site_force(site[e], fs);
        for (int c = 0; c < 3; c++) f[c] += weight[e] * fs[c];
    }
}

}  // namespace emdee

#if defined(__HIPCC__)

namespace emdee {

// The site table (Topology::vsites, topology.hpp VsiteParents) and where the atoms are.  atoms: {site, a, b, c} caller ids per
// entry, c = -1 for a two-parent site; weights: {w_b, w_c}, w_c = 0 where c = -1.  The parent list: parent[q] the caller id of the
// q-th distinct parent, its entries [pstart[q], pstart[q + 1]) of (esite, eweight) in table order.  Slots come from inv_perm, as
// in the constraint kernels: nothing depends on the sort.
template <typename real>
struct VsiteArgs {
    int n, n_parents;
    const int *atoms;
    const double *weights;
    const int *parent, *pstart, *esite;
    const double *eweight;
    ConstraintArgs<real> c;                                  // inv_perm, rec, vel, inv_mass, pitch, rel, box (n, atoms, geom unused)
};

// words[0] = a site + 1 that has a mass, words[1] = a site + 1 one of whose parents has none; the highest such entry each
template <typename real>
__global__ __launch_bounds__(256) void k_vsite_check(VsiteArgs<real> a, int *__restrict__ words) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n) return;
    const real *w = a.c.inv_mass;
    if (w[a.c.inv_perm[a.atoms[4 * (size_t)s]]] != (real)0) atomicMax(words, s + 1);
    bool massless = false;
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const int g = a.atoms[4 * (size_t)s + k];
        if (g >= 0 && w[a.c.inv_perm[g]] == (real)0) massless = true;
    }
    if (massless) atomicMax(words + 1, s + 1);
}

// Placement, one thread per site: the parents' records in double (settle_detail::site), the minimum images of b and c from a, the
// site; the site's record moves by the minimum image of (new - old), added in double in the record's own frame and rounded once
// (as k_constraint_positions adds its corrections), so the record stays continuous and its image count valid.  The site is
// tested against the rebuild threshold (k_kick_drift's test, on the new record).  zero_vel: the site's velocity becomes 0.
template <typename real>
__global__ __launch_bounds__(256) void k_vsite_place(VsiteArgs<real> a, const real *__restrict__ xb, real thr2, int *__restrict__ flag,
                                                     int zero_vel) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n) return;
    const int gc = a.atoms[4 * (size_t)s + 3];
    const int ps = a.c.inv_perm[a.atoms[4 * (size_t)s]], pa = a.c.inv_perm[a.atoms[4 * (size_t)s + 1]],
              pb = a.c.inv_perm[a.atoms[4 * (size_t)s + 2]], pc = gc >= 0 ? a.c.inv_perm[gc] : pa;
    double xs[3], xa[3], xbb[3], xc[3], d[3], e[3], x[3];
    settle_detail::site(a.c, ps, xs);
    settle_detail::site(a.c, pa, xa);
    settle_detail::site(a.c, pb, xbb);
    settle_detail::site(a.c, pc, xc);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d[k] = vsite_image(xbb[k] - xa[k], a.c.box.len[k], a.c.box.per[k]);
        e[k] = gc >= 0 ? vsite_image(xc[k] - xa[k], a.c.box.len[k], a.c.box.per[k]) : 0.0;
    }
    vsite_place(xa, d, e, a.weights[2 * (size_t)s], a.weights[2 * (size_t)s + 1], x);
    Rec<real> r = a.c.rec[ps];
    r.x = (real)((double)r.x + vsite_image(x[0] - xs[0], a.c.box.len[0], a.c.box.per[0]));
    r.y = (real)((double)r.y + vsite_image(x[1] - xs[1], a.c.box.len[1], a.c.box.per[1]));
    r.z = (real)((double)r.z + vsite_image(x[2] - xs[2], a.c.box.len[2], a.c.box.per[2]));
    a.c.rec[ps] = r;
    if (zero_vel) { a.c.vel[ps] = (real)0; a.c.vel[a.c.pitch + ps] = (real)0; a.c.vel[2 * a.c.pitch + ps] = (real)0; }
    const real ux = r.x - xb[ps], uy = r.y - xb[a.c.pitch + ps], uz = r.z - xb[2 * a.c.pitch + ps];
    if (ux * ux + uy * uy + uz * uz > thr2) *flag = 1;
}

// Spreading, one thread per distinct parent: its force plus its entries' shares in table order, summed in fp64 and rounded once.
// No thread writes what another reads (parents are never sites); k_vsite_clear zeroes the sites' forces afterwards.
template <typename real>
__global__ __launch_bounds__(256) void k_vsite_spread(VsiteArgs<real> a, real *__restrict__ frc) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n_parents) return;
    const int p = a.c.inv_perm[a.parent[q]];
    const size_t pitch = a.c.pitch;
    double f[3] = {(double)frc[p], (double)frc[pitch + p], (double)frc[2 * pitch + p]};
    vsite_spread_parent(a.esite, a.eweight, a.pstart[q], a.pstart[q + 1], [&](int s, double (&fs)[3]) {
        const int ps = a.c.inv_perm[a.atoms[4 * (size_t)s]];
        fs[0] = (double)frc[ps]; fs[1] = (double)frc[pitch + ps]; fs[2] = (double)frc[2 * pitch + ps];
    }, f);
    frc[p] = (real)f[0]; frc[pitch + p] = (real)f[1]; frc[2 * pitch + p] = (real)f[2];
}
template <typename real>
__global__ __launch_bounds__(256) void k_vsite_clear(VsiteArgs<real> a, real *__restrict__ frc) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n) return;
    const int ps = a.c.inv_perm[a.atoms[4 * (size_t)s]];
    frc[ps] = (real)0; frc[a.c.pitch + ps] = (real)0; frc[2 * a.c.pitch + ps] = (real)0;
}

}  // namespace emdee
#endif
