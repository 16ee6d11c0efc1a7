// rdf.hpp -- radial distribution functions on the device (emdee_md_set_rdf, emdee_md_rdf_sample): a pair histogram of the current
// positions, one per unordered pair of atom groups.  A sample bins the grouped atoms on a grid of its own, made from the positions as
// they are now (it never looks at the neighbour list, whose age it therefore does not depend on), and runs a cell-tiled pair loop
// through LDS whose sums are integers: the result is exact and the same whatever the order of the atoms.  The parts with no HIP in
// them -- the slot map, the bin rule, the planner of the grid and its stencil, the normalisation -- are plain C++ at the top, as the
// tops of settle.hpp, shake.hpp and thermostat.hpp are: a stand-alone host program tests them with the host compiler
// (tests/c/rdf_host.cpp); the kernels below them need HIP.  DESIGN.md 4g has the algorithm; MdImpl::rdf_sample (impl.hpp) queues a sample.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int RDF_MAX_GROUPS = 8;
constexpr int RDF_MAX_COUNTERS = 8192;                       // n_pairs n_bins: a workgroup's private histogram is at most 32 KB of LDS
constexpr int RDF_ND_MAX = 3;
// A pair is looked at when r^2 <= r_max^2 (1 + 2^-40) and kept when its bin is below n_bins: the bin rule alone decides, as it does
// in (r * inv_dr).astype(int) of numpy, also for a pair whose r rounds to r_max.  The cells are wider than r_max / nd by 2^-30, which
// covers that margin and the rounding of the cell coordinates.
constexpr double RDF_R2_MARGIN = 1.0 + 0x1p-40, RDF_SIDE_MARGIN = 1.0 + 0x1p-30;

// the histogram of the unordered group pair {a, b}: slots 0 ... n_groups (n_groups + 1) / 2 - 1, row by row of the upper triangle
EMDEE_HD int rdf_pair_slot(int a, int b, int n_groups) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo * n_groups - lo * (lo - 1) / 2 + (hi - lo);
}
EMDEE_HD int rdf_n_pairs(int n_groups) { return n_groups * (n_groups + 1) / 2; }

// the bin of a pair at squared distance r2, or -1 when it lies beyond the last bin; inv_dr = n_bins / r_max, formed once in double
EMDEE_HD int rdf_bin(double r2, double inv_dr, int n_bins) {
    const double t = sqrt(r2) * inv_dr;
    if (!(t < (double)n_bins)) return -1;
    return (int)t;
}

// ---- the grid of a sample and its stencil
// M[d] cells of side >= r_max / nd (RDF_SIDE_MARGIN) along axis d.  From a home cell the stencil visits the 2 nd + 1 cells
// c - nd ... c + nd (periodically) of an axis, all distinct as long as the axis has at least 2 nd + 1 cells.  On a shorter axis
// the offsets would wrap onto cells already visited and count pairs twice: wrap[d] is set, and every cell of that axis is visited
// exactly once instead.
struct RdfPlan {
    int M[3], nd, wrap[3];
};
EMDEE_HD long long rdf_plan_cells(const RdfPlan &p) { return (long long)p.M[0] * p.M[1] * p.M[2]; }
// how many cells of axis d a home cell visits, and the k-th of them seen from cell coordinate c
EMDEE_HD int rdf_axis_count(int M, int nd, int wrap) { return wrap ? M : 2 * nd + 1; }
EMDEE_HD int rdf_axis_cell(int M, int nd, int wrap, int c, int k) { return wrap ? k : (c - nd + k + M) % M; }
// The cells of the x axis are neighbours in memory, so the pair kernel does not walk x cell by cell: the cells a home cell at
// coordinate cx visits along x are one run [xa0, xa1] of coordinates, or two, [xa0, xa1] and [xb0, xb1], where the stencil passes
// the box face.  Returns the number of runs (the second run is left empty, [0, -1], when there is one).  The same cells as
// rdf_axis_cell gives for k = 0 ... rdf_axis_count - 1.
EMDEE_HD int rdf_row_runs(int M, int nd, int wrap, int cx, int &xa0, int &xa1, int &xb0, int &xb1) {
    xb0 = 0; xb1 = -1;
    if (wrap) { xa0 = 0; xa1 = M - 1; return 1; }
    if (cx - nd < 0) { xa0 = 0; xa1 = cx + nd; xb0 = cx - nd + M; xb1 = M - 1; return 2; }
    if (cx + nd >= M) { xa0 = 0; xa1 = cx + nd - M; xb0 = cx - nd; xb1 = M - 1; return 2; }
    xa0 = cx - nd; xa1 = cx + nd;
    return 1;
}
// the cell coordinate of x on a periodic axis [lo, lo + len) of M cells; any periodic image of x gives the same cell
EMDEE_HD int rdf_axis_cell_of(double x, double lo, double len, int M) {
    double s = (x - lo) / len;
    s -= floor(s);
    const int v = (int)(s * (double)M);
    return v < 0 ? 0 : (v < M ? v : M - 1);
}
// The planner: nd is the largest of 1 ... RDF_ND_MAX that leaves a mean of eight atoms to a cell (finer cells look at fewer pairs
// beyond r_max: 27 cells of side r_max hold 6.4 times the sphere, 125 of side r_max / 2 hold 3.7 times); a sparse box never gets
// more than about four cells per atom (wider cells stay valid).
inline RdfPlan rdf_plan(const double len[3], double r_max, long long n_atoms) {
    RdfPlan best{};
    for (int nd = 1; nd <= RDF_ND_MAX; nd++) {
        RdfPlan p{};
        p.nd = nd;
        const double side = r_max * RDF_SIDE_MARGIN / (double)nd;
        for (int d = 0; d < 3; d++) {
            const double m = floor(len[d] / side);
            p.M[d] = m < 1.0 ? 1 : (m > 1024.0 ? 1024 : (int)m);
        }
        if (nd > 1 && (double)n_atoms < 8.0 * (double)rdf_plan_cells(p)) break;
        best = p;
    }
    const long long most = 4 * (n_atoms > 16 ? n_atoms : 16) + 64;
    while (rdf_plan_cells(best) > most) {
        int big = 0;
        for (int d = 1; d < 3; d++)
            if (best.M[d] > best.M[big]) big = d;
        if (best.M[big] <= 1) break;
        best.M[big] = (best.M[big] + 1) / 2;
    }
    for (int d = 0; d < 3; d++) best.wrap[d] = best.M[d] < 2 * best.nd + 1 ? 1 : 0;
    return best;
}

// ---- g(r) and the running coordination numbers from the accumulators of emdee_md_rdf_read
// g_ab(bin) = counts / (P_ab shell(bin) inv_volume_sum), shell(bin) = 4 pi / 3 (r_{bin+1}^3 - r_bin^3), r_k = r_max k / n_bins,
// P_ab = N_a N_b (a != b) or N_a (N_a - 1) / 2; coordination(bin) = cumulative counts x (2 if a == b else 1) / (N_a frames): the
// atoms of group b within r_{bin+1} of an atom of group a, a <= b.  Pairs left out as intramolecular are not taken out of P.  A slot
// without pairs or without frames gives zeros.
inline void rdf_normalise(const long long *counts, int n_groups, int n_bins, double r_max, const long long *sizes, long long frames,
                          double inv_volume_sum, double *g, double *coordination) {
    const double four_thirds_pi = 4.0 * 3.14159265358979323846 / 3.0;
    for (int a = 0; a < n_groups; a++)
        for (int b = a; b < n_groups; b++) {
            const int s = rdf_pair_slot(a, b, n_groups);
            const double P = a == b ? 0.5 * (double)sizes[a] * (double)(sizes[a] - 1) : (double)sizes[a] * (double)sizes[b];
            const double per_a = (double)sizes[a] * (double)frames;
            long long sum = 0;
            for (int k = 0; k < n_bins; k++) {
                const double r0 = r_max * (double)k / (double)n_bins, r1 = r_max * (double)(k + 1) / (double)n_bins;
                const double ideal = P * four_thirds_pi * (r1 * r1 * r1 - r0 * r0 * r0) * inv_volume_sum;
                const long long c = counts[(size_t)s * n_bins + k];
                sum += c;
                g[(size_t)s * n_bins + k] = ideal > 0.0 ? (double)c / ideal : 0.0;
                coordination[(size_t)s * n_bins + k] = per_a > 0.0 ? (a == b ? 2.0 : 1.0) * (double)sum / per_a : 0.0;
            }
        }
}

}  // namespace emdee

#if defined(__HIPCC__)

#include "kernels.hpp"

namespace emdee {

// one grouped atom in the sample's own cell order: the position in fp64 in both precisions, its group and its molecule (-1: none)
struct alignas(32) RdfAtom {
    double x, y, z;
    int group, mol;
};
// what the kernels need of the box and the plan (every member is read with a constant index: the struct stays in registers)
struct RdfGrid {
    double lo[3], len[3], inv_len[3];
    int M[3], nd, wrap[3];
};

// the position of slot p as doubles: the record itself, or (Float32 engines with cell-relative records) the record plus the origin
// of its cell, the sum RecPos forms, kept in fp64
template <typename real>
__device__ __forceinline__ void rdf_position(const Rec<real> *__restrict__ rec, const RelGrid &rel, int p, double &x, double &y, double &z) {
    const Rec<real> q = rec[p];
    x = (double)q.x; y = (double)q.y; z = (double)q.z;
    if (sizeof(real) == 4 && rel.on) {
        double ox, oy, oz;
        rel.origin(rel.cell[p], ox, oy, oz);
        x += ox; y += oy; z += oz;
    }
}

// Counting sort, pass 1: the cell of every grouped owned atom (-1 for the others) and the cells' populations; one integer atomic per
// run of equal cells in a wavefront (the engine's order is nearly the sample's), as k_cell_assign has it.
template <typename real>
__global__ __launch_bounds__(256) void k_rdf_count(int n, int n_owned, const Rec<real> *__restrict__ rec, RelGrid rel,
                                                   const int *__restrict__ perm, const int *__restrict__ group, RdfGrid g,
                                                   int *__restrict__ cell_of, int *__restrict__ count) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    int c = -1;
    if (p < n) {
        const int id = perm[p];
        const int grp = (id >= 0 && id < n_owned) ? (group ? group[id] : 0) : -1;
        if (grp >= 0) {
            double x, y, z;
            rdf_position(rec, rel, p, x, y, z);
            c = rdf_axis_cell_of(x, g.lo[0], g.len[0], g.M[0]) +
                g.M[0] * (rdf_axis_cell_of(y, g.lo[1], g.len[1], g.M[1]) + g.M[1] * rdf_axis_cell_of(z, g.lo[2], g.len[2], g.M[2]));
        }
        cell_of[p] = c;
    }
    int first, len;
    wave_run(c, first, len);
    if (c >= 0 && lane_id() == first) atomicAdd(&count[c], len);
}

// pass 2: the compact array in cell order (start[] is the scanned count[]).  The order inside a cell is the order of arrival: the
// histogram is a sum of integers and does not depend on it.
template <typename real>
__global__ __launch_bounds__(256) void k_rdf_fill(int n, const Rec<real> *__restrict__ rec, RelGrid rel, const int *__restrict__ perm,
                                                  const int *__restrict__ group, const int *__restrict__ mol,
                                                  const int *__restrict__ cell_of, const int *__restrict__ start,
                                                  int *__restrict__ fill, RdfAtom *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = p < n ? cell_of[p] : -1;
    int first, len;
    wave_run(c, first, len);
    int base = 0;
    if (c >= 0 && lane_id() == first) base = start[c] + atomicAdd(&fill[c], len);
    base = __shfl(base, first);
    if (c < 0) return;
    const int id = perm[p];
    RdfAtom a;
    rdf_position(rec, rel, p, a.x, a.y, a.z);
    a.group = group ? group[id] : 0;
    a.mol = mol ? mol[id] : -1;
    out[base + (lane_id() - first)] = a;
}


// The pair loop.  A workgroup takes a contiguous block of home cells, one after the other.  The atoms of a home cell sit in
// registers, up to RDF_BLOCK at a time: nh of them on the low bits of the thread index, the other bits deal the staged atoms among
// the threads of one home atom.  The cells of a stencil row along x are neighbours in memory, so a row is one range of the compact
// array (two where it passes the box face): the stencil is a list of at most RDF_MAX_SEGS ranges.  A pair is counted from the atom
// with the lower index of the compact array only -- every unordered pair exactly once --, so every range is cut off below the home
// atoms, which leaves about half the stencil.  The ranges are laid end to end and staged through LDS RDF_BLOCK atoms at a time,
// whatever range they come from: at liquid densities the half stencil of a cell is one or a few stagings, not one per row.  The
// distance is the minimum image in fp64; r^2 is tested before the square root.
// The workgroup's histogram lives in LDS as u32 counters filled by LDS integer atomics; the non-zero ones are added to the global
// u64 histogram by integer atomics.  One staging tests at most RDF_BLOCK x RDF_BLOCK = 65536 pairs, and the histogram is flushed
// after RDF_FLUSH_STEPS = 65535 of them at the latest: no counter ever holds more than 65535 x 65536 < 2^32.
constexpr int RDF_BLOCK = 256, RDF_FLUSH_STEPS = 65535;
constexpr int RDF_MAX_SEGS = 2 * (2 * RDF_ND_MAX + 1) * (2 * RDF_ND_MAX + 1);   // (a wrapped axis has fewer cells than 2 nd + 1)

__device__ __forceinline__ void rdf_flush(unsigned int *hist, int n_counters, unsigned long long *__restrict__ counts) {
    __syncthreads();
    for (int k = threadIdx.x; k < n_counters; k += RDF_BLOCK) {
        const unsigned int v = hist[k];
        if (v != 0u) {
            atomicAdd(&counts[k], (unsigned long long)v);
            hist[k] = 0u;
        }
    }
    __syncthreads();
}

static __global__ __launch_bounds__(RDF_BLOCK) void k_rdf_pairs(RdfGrid g, int ncell, const int *__restrict__ start,
                                                                const RdfAtom *__restrict__ atoms, double r2_cut, double inv_dr,
                                                                int n_bins, int n_groups, int n_counters,
                                                                unsigned long long *__restrict__ counts) {
    extern __shared__ unsigned int rdf_hist[];
    __shared__ double sx[RDF_BLOCK], sy[RDF_BLOCK], sz[RDF_BLOCK];
    __shared__ int sg[RDF_BLOCK], sm[RDF_BLOCK], sslot[RDF_BLOCK];
    __shared__ int seg_s0[RDF_MAX_SEGS], seg_len[RDF_MAX_SEGS], seg_off[RDF_MAX_SEGS + 1];
    const int t = threadIdx.x;
    for (int k = t; k < n_counters; k += RDF_BLOCK) rdf_hist[k] = 0u;
    __syncthreads();
    int steps = 0;
    const int Mx = g.M[0], My = g.M[1], Mz = g.M[2], nd = g.nd;
    const int ny = rdf_axis_count(My, nd, g.wrap[1]), nz = rdf_axis_count(Mz, nd, g.wrap[2]);
    const int c_begin = (int)((long long)blockIdx.x * ncell / gridDim.x), c_end = (int)((long long)(blockIdx.x + 1) * ncell / gridDim.x);
    for (int c = c_begin; c < c_end; c++) {
        const int h_begin = start[c], h_end = start[c + 1];
        if (h_begin == h_end) continue;
        const int cx = c % Mx, cy = (c / Mx) % My, cz = c / (Mx * My);
        // the cells of a row along x: one run [xa0, xa1], or a second one [xb0, xb1] where the stencil passes the box face
        int xa0, xa1, xb0, xb1;
        const int nseg = rdf_row_runs(Mx, nd, g.wrap[0], cx, xa0, xa1, xb0, xb1);
        const int nsegs = ny * nz * nseg;                    // <= RDF_MAX_SEGS
        for (int h0 = h_begin; h0 < h_end; h0 += RDF_BLOCK) {
            const int nh = min(RDF_BLOCK, h_end - h0);
            int sh = 0;
            while ((1 << sh) < nh) sh++;
            const int i = t & ((1 << sh) - 1), jl = t >> sh, JL = RDF_BLOCK >> sh;
            const bool home = i < nh;
            RdfAtom me{};
            if (home) me = atoms[h0 + i];
            const int my_slot = h0 + i;
            // the ranges of the stencil above the first home atom, then where each begins in the queue they form
            if (t < nsegs) {
                const int r = t / nseg, q = t - r * nseg, kz = r / ny, ky = r - kz * ny;
                const int row = (rdf_axis_cell(Mz, nd, g.wrap[2], cz, kz) * My + rdf_axis_cell(My, nd, g.wrap[1], cy, ky)) * Mx;
                const int s0 = max(start[row + (q ? xb0 : xa0)], h0 + 1), s1 = start[row + (q ? xb1 : xa1) + 1];
                seg_s0[t] = s0;
                seg_len[t] = max(s1 - s0, 0);
            }
            __syncthreads();
            if (t <= nsegs) {
                int o = 0;
                for (int k = 0; k < t; k++) o += seg_len[k];
                seg_off[t] = o;
            }
            __syncthreads();
            const int total = seg_off[nsegs];
            for (int base = 0; base < total; base += RDF_BLOCK) {
                if (steps == RDF_FLUSH_STEPS) { rdf_flush(rdf_hist, n_counters, counts); steps = 0; }
                steps++;
                const int v = base + t;
                if (v < total) {
                    int lo = 0, hi = nsegs;                  // seg_off[lo] <= v < seg_off[hi]
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (seg_off[mid] <= v) lo = mid; else hi = mid;
                    }
                    const int slot = seg_s0[lo] + (v - seg_off[lo]);
                    const RdfAtom a = atoms[slot];
                    sx[t] = a.x; sy[t] = a.y; sz[t] = a.z; sg[t] = a.group; sm[t] = a.mol; sslot[t] = slot;
                }
                __syncthreads();
                if (home) {
                    const int nj = min(RDF_BLOCK, total - base);
                    for (int j = jl; j < nj; j += JL) {
                        if (sslot[j] <= my_slot) continue;
                        if (me.mol >= 0 && me.mol == sm[j]) continue;
                        double dx = sx[j] - me.x, dy = sy[j] - me.y, dz = sz[j] - me.z;
                        dx -= g.len[0] * rint(dx * g.inv_len[0]);
                        dy -= g.len[1] * rint(dy * g.inv_len[1]);
                        dz -= g.len[2] * rint(dz * g.inv_len[2]);
                        const double r2 = dx * dx + dy * dy + dz * dz;
                        if (!(r2 <= r2_cut)) continue;
                        const int bin = rdf_bin(r2, inv_dr, n_bins);
                        if (bin < 0) continue;
                        atomicAdd(&rdf_hist[rdf_pair_slot(me.group, sg[j], n_groups) * n_bins + bin], 1u);
                    }
                }
                __syncthreads();
            }
        }
    }
    rdf_flush(rdf_hist, n_counters, counts);
}

}  // namespace emdee
#endif
