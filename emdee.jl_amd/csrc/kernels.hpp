// kernels.hpp -- device kernels of the O(N) nonbonded path, templated on the real type.
//
// Data layout in HBM (cell order = atoms sorted by cell id, ascending caller id inside a cell):
//   rec[p]      one aligned record per atom: fp64 {x,y,z, half_sigma, twice_sqrt_eps} = 32 B
//               (a neighbour gather is exactly one record: position AND LJAtom parameters);
//               fp32 {x,y,z, half_sigma} = 16 B plus te[p] (4 B)
//   vel/frc     structure-of-arrays, 3 planes of `pitch` reals: every streaming pass is a
//               unit-stride 4/8-B-per-lane access
//   nbr         row-major ELL: row p holds the neighbours of atom p at nbr[p*stride .. +cnt[p])
//               so a wavefront reads its atom's indices as 256-B coalesced segments
//   perm/inv    cell-order slot -> caller id and back
//
// Reference lines restated here: cell id convention src/cells.jl:82-85,180-181; minimum image
// src/nonbonded.jl:40; f_ij = W/r2 * r_ij and the half split of E and W src/nonbonded.jl:136-145;
// the pair function is lj_pair.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "bonded.hpp"
#include "common.hpp"
#include "lj_pair.hpp"
#include "reduce.hpp"
#include "wave_ops.hpp"

namespace emdee {

// ------------------------------------------------------------------------------------ records
template <typename real>
struct Rec;
template <>
struct alignas(32) Rec<double> {
    double x, y, z;
    float hs, te;
};
template <>
struct alignas(16) Rec<float> {
    float x, y, z, hs;
};

// Cell-relative records (round 5; fp32 integrators): a record holds the atom's position RELATIVE TO THE ORIGIN OF ITS CELL
// as of the last sort, so that the drift x += dt v of a step rounds at the ulp of a cell-sized number (2.4e-7 sigma) and
// not at the ulp of the box (1.5e-5 sigma at 10^7 atoms, 3.1e-5 at 10^8 -- against ~5e-3 sigma moved per step: the noise
// that random-walked the fp32 runs' energy).  Between sorts an atom may wander a little out of its cell: the relative
// coordinate simply leaves [0, cell width).  on = 0: records are absolute (every fp64 state, operator handles, domains).
struct RelGrid {
    double lo[3], cw[3];      // box origin, cell widths
    int M[3];
    int on;
    const int *cell;          // cell of every slot (NbSystem::cell_sorted as of the sort the records belong to)
    // Cell origins sit on ONE fixed-point grid of the box, REL_FX = 2^19 points per length unit (what fp32 resolves at the far end
    // of a brick's tile): a tile coordinate is then (round(record x 2^19) + an INTEGER per tile cell) / 2^19, exact in fp32, and
    // two atoms have the same separation in whichever brick's tile they meet -- F_ij = -F_ji to the bit (brick.hpp rel_tile).
    __host__ __device__ __forceinline__ double origin_q(int d, int c) const { return rint((lo[d] + (double)c * cw[d]) * 524288.0); }   // in grid points
    // c / m and c % m for 0 <= c < 2^24 (a box of 10^8 atoms has 5.6e6 cells): one fp32 multiply and a correction by one instead of
    // the ~35 instructions of an integer division by a run-time divisor -- twice per atom in every pass that reads relative records
    __device__ static __forceinline__ int divmod(int c, int m, int &rem) {
        int q = (int)((float)c * __builtin_amdgcn_rcpf((float)m));       // (v_rcp_f32: 1 ulp, the correction below absorbs it)
        rem = c - q * m;
        while (rem < 0) { q--; rem += m; }                   // (the estimate is off by at most one: c < 2^24, two roundings of 6e-8)
        while (rem >= m) { q++; rem -= m; }
        return q;
    }
    __device__ __forceinline__ void origin(int c, double &ox, double &oy, double &oz) const {
        int cx, cy, cz;
        if (c < (1 << 24)) {
            const int t = divmod(c, M[0], cx);
            cz = divmod(t, M[1], cy);
        } else {
            cx = c % M[0]; cy = (c / M[0]) % M[1]; cz = c / (M[0] * M[1]);
        }
        ox = origin_q(0, cx) * (1.0 / 524288.0); oy = origin_q(1, cy) * (1.0 / 524288.0); oz = origin_q(2, cz) * (1.0 / 524288.0);
    }
};
constexpr float REL_FX = 524288.f, REL_IFX = 1.f / 524288.f;

// read-only view of the cell-ordered atoms
template <typename real>
struct AtomView {
    const Rec<real> *rec;
    const float *te;   // fp32 only (fp64 keeps te inside the record)
    RelGrid rel;       // fp32 only: cell-relative records (load_atom returns absolute coordinates, rounded to fp32)
};

__device__ __forceinline__ void load_atom(const AtomView<double> &a, int p, double &x, double &y, double &z, double &hs,
                                          double &te) {
    Rec<double> r = a.rec[p];   // 2 x global_load_dwordx4
    x = r.x; y = r.y; z = r.z; hs = (double)r.hs; te = (double)r.te;
}
__device__ __forceinline__ void load_atom(const AtomView<float> &a, int p, float &x, float &y, float &z, float &hs,
                                          float &te) {
    Rec<float> r = a.rec[p];    // 1 x global_load_dwordx4
    x = r.x; y = r.y; z = r.z; hs = r.hs; te = a.te[p];
    if (a.rel.on) {             // (the kernels that come through here are not the integrator's hot ones)
        double ox, oy, oz;
        a.rel.origin(a.rel.cell[p], ox, oy, oz);
        x = (float)((double)x + ox); y = (float)((double)y + oy); z = (float)((double)z + oz);
    }
}

// ------------------------------------------------------------------------------------ grid
template <typename real>
struct GridP {
    real lo[3], len[3];      // box
    real plen[3], pinv[3];   // minimum image d -= plen * rint(d * pinv); both 0 on non-periodic dims
    int per[3];
    int M[3];                // cells per dimension
    int nd;                  // stencil half-width in cells (cell side >= rlist / nd)
    int one_based;           // Cells API: ids are 1-based (src/cells.jl:181)
};

// 0-based voxel of coordinate p along dimension d: floor(M (s - floor s)), s = (p - lo)/len.
// True division, not a reciprocal multiply: the Cells API must agree bit-for-bit with the
// reference arithmetic s = r / L (src/cells.jl:79-84,180).
template <typename real>
__device__ __forceinline__ int voxel(real p, real lo, real len, int M, int periodic) {
    real s = (p - lo) / len;
    real t = periodic ? s - floor(s) : s;
    int v = (int)floor((real)M * t);
    return min(max(v, 0), M - 1);
}

template <typename real>
__device__ __forceinline__ int cell_id(const GridP<real> &g, real x, real y, real z) {
    int vx = voxel(x, g.lo[0], g.len[0], g.M[0], g.per[0]);
    int vy = voxel(y, g.lo[1], g.len[1], g.M[1], g.per[1]);
    int vz = voxel(z, g.lo[2], g.len[2], g.M[2], g.per[2]);
    return vx + g.M[0] * (vy + g.M[1] * vz);
}

template <typename real>
__device__ __forceinline__ real min_image(real d, real plen, real pinv) {
    return d - plen * rint(d * pinv);   // v_rndne: ties-to-even like Julia round (Q8)
}

// position sources: caller order (3xN interleaved) or cell-ordered records
template <typename real>
struct UserPos {
    const real *p;
    __device__ __forceinline__ void get(int i, real &x, real &y, real &z) const {
        x = p[3 * (size_t)i]; y = p[3 * (size_t)i + 1]; z = p[3 * (size_t)i + 2];
    }
};
template <typename real>
struct RecPos {
    const Rec<real> *r;
    RelGrid rel;
    __device__ __forceinline__ void get(int i, real &x, real &y, real &z) const {
        Rec<real> q = r[i];
        x = q.x; y = q.y; z = q.z;
        if (sizeof(real) == 4 && rel.on) {
            double ox, oy, oz;
            rel.origin(rel.cell[i], ox, oy, oz);
            x = (real)((double)q.x + ox); y = (real)((double)q.y + oy); z = (real)((double)q.z + oz);
        }
    }
};

// ------------------------------------------------------------------------------------ x sub-bins (untyped boxes)
// Inside a cell the atoms are ordered by the quarter of the cell (along x) they sit in: the sort digit is cell * S + sub-bin,
// exactly as a typed box uses cell * 2 + species.  The tile rows of the neighbour build are runs of three cells along x, so
// an atom in sub-bin s needs only the sub-bins >= s + K of the cell on its left and <= s - K of the cell on its right
// (K = 0 when the cell is as wide as r_list): 9 of the 12 quarters of a row instead of all -- the build tests a quarter
// fewer candidates (brick.hpp).  The sub-bin comes from the SAME product M t the cell does (voxel above), so an atom of
// sub-bin s of cell v has M t in [v + s / S, v + (s + 1) / S) exactly.
template <typename real, class Src>
struct XSubBin {
    Src src;
    real lo, len;
    int M, per, S;
    __device__ __forceinline__ int of(int i) const {
        real x, y, z;
        src.get(i, x, y, z);
        const real s = (x - lo) / len;
        const real t = per ? s - floor(s) : s;
        const real f = (real)M * t;
        const int v = (int)floor(f);
        if (v < 0) return 0;                       // (clamped into the first / last cell by voxel())
        if (v > M - 1) return S - 1;
        const int sb = (int)((f - (real)v) * (real)S);
        return min(max(sb, 0), S - 1);
    }
};

// ------------------------------------------------------------------------------------ species ("typed" boxes)
// A box with 2 distinct LJAtom values is sorted by (cell, species): inside a cell the atoms of species 0 come first.
// The LDS tiles of the brick kernels are then staged species-major, neighbour rows come out as one segment per neighbour
// species, and the pair loop needs no per-pair parameter mixing (brick.hpp, NT).  The table holds the distinct LJAtom
// bit patterns in ascending order (the host sorts what k_species_collect found: the numbering must not depend on a race).
constexpr int MAX_SPECIES = 4;
struct SpeciesTable {
    int n;                                  // 1: untyped (every kernel behaves as before)
    unsigned long long key[MAX_SPECIES];    // half_sigma bits | twice_sqrt_eps bits << 32
};
__host__ __device__ __forceinline__ unsigned long long species_key(float hs, float te) {
    unsigned a, b;
#if defined(__HIP_DEVICE_COMPILE__)
    a = __float_as_uint(hs); b = __float_as_uint(te);
#else
    memcpy(&a, &hs, 4); memcpy(&b, &te, 4);
#endif
    return (unsigned long long)a | ((unsigned long long)b << 32);
}
__device__ __forceinline__ int species_of(const SpeciesTable &t, unsigned long long k) {
    int s = 0;
#pragma unroll
    for (int q = 1; q < MAX_SPECIES; q++) s = (q < t.n && t.key[q] == k) ? q : s;
    return s;
}
// species of item i of a position source (caller order: from the LJAtom array; cell order: from the records)
struct NoSpecies {
    __device__ __forceinline__ int of(int) const { return 0; }
};
struct UserSpecies {
    SpeciesTable t;
    const emdee_lj_atom *atoms;
    __device__ __forceinline__ int of(int i) const { return species_of(t, species_key(atoms[i].half_sigma, atoms[i].twice_sqrt_eps)); }
};
template <typename real>
struct RecSpecies;
template <>
struct RecSpecies<double> {
    SpeciesTable t;
    const Rec<double> *rec;
    const float *te;
    __device__ __forceinline__ int of(int i) const { return species_of(t, species_key(rec[i].hs, rec[i].te)); }
};
template <>
struct RecSpecies<float> {
    SpeciesTable t;
    const Rec<float> *rec;
    const float *te;
    __device__ __forceinline__ int of(int i) const { return species_of(t, species_key(rec[i].hs, te[i])); }
};
// two-species boxes whose build takes x sub-bins (typed.hpp): digit = species * S + quarter
template <class Spc, class Sub>
struct SpeciesSub {
    Spc spc;
    Sub sub;
    __device__ __forceinline__ int of(int i) const { return spc.of(i) * sub.S + sub.of(i); }
};
// distinct LJAtom values of a box, at most MAX_SPECIES: tab[0..3] = keys in order of arrival (EMPTY = all ones),
// tab[4] != 0 if there are more.  Almost every thread finds its key with device-scope loads; the atomics are for the
// first few arrivals.
// (Round 4: ONE look-up per distinct key of a wavefront, by the first lane that holds it -- every thread looking at the hot words
// itself was 10^7 device-scope loads of four addresses: 2-6 ms at every load of a 10^7-atom state, more than its whole sort.)
static __global__ void k_species_collect(int n, const emdee_lj_atom *__restrict__ atoms, unsigned long long *__restrict__ tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long EMPTY = ~0ull;
    unsigned long long mine = EMPTY;
    bool pending = i < n;
    if (pending) mine = species_key(atoms[i].half_sigma, atoms[i].twice_sqrt_eps);
    const int lane = lane_id();
    for (int round = 0; round <= MAX_SPECIES; round++) {       // at most MAX_SPECIES + 1 distinct keys matter: one more is "too many"
        const unsigned long long left = __ballot(pending);
        if (left == 0) return;
        const int leader = __ffsll((long long)left) - 1;
        const unsigned lo = __shfl((unsigned)mine, leader), hi = __shfl((unsigned)(mine >> 32), leader);
        const unsigned long long key = (unsigned long long)lo | ((unsigned long long)hi << 32);
        if (pending && mine == key) {
            pending = false;
            if (lane == leader) {
                bool found = false;
                for (int q = 0; q < MAX_SPECIES && !found; q++) {
                    unsigned long long cur = __hip_atomic_load(&tab[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == EMPTY) cur = atomicCAS(&tab[q], EMPTY, key);
                    found = cur == EMPTY || cur == key;
                }
                if (!found) tab[MAX_SPECIES] = 1;
            }
        }
    }
    if (__ballot(pending) != 0 && lane == 0) tab[MAX_SPECIES] = 1;   // a wavefront with more distinct keys than the table holds
}
// ------------------------------------------------------------------------------------ binning
// Runs of equal keys among the 64 lanes of a wavefront (adjacent lanes only).  When the input is already
// nearly cell-ordered -- every MD rebuild -- a wavefront spans ~4 cells, so one atomic per RUN instead of one
// per atom cuts the integer atomics ~16x.  Returns the first lane and the length of this lane's run.
__device__ __forceinline__ void wave_run(int key, int &first, int &len) {
    const int lane = lane_id();
    const int prev = __shfl_up(key, 1);
    const unsigned long long leaders = __ballot(lane == 0 || key != prev);
    const unsigned long long upto = leaders & (~0ull >> (63 - lane));          // leaders at or below me
    first = 63 - __clzll(upto);
    const unsigned long long after = (first == 63) ? 0ull : (leaders & (~0ull << (first + 1)));
    len = (after ? (__ffsll((long long)after) - 1) : 64) - first;
}

// Radix-count pass of the counting sort: one digit = the cell id.
// (typed boxes: the digit is cell * nt + species, so that a cell's atoms come out grouped by species)
// (keep, optional: one byte per item -- an item whose byte is 0 is not part of the new state: a decomposed domain re-sorts
// its own records with the leavers and the old ghosts struck out and the arrivals appended, NbSystem::resort_edit)
template <typename real, class Src, class Spc = NoSpecies>
__global__ void k_cell_assign(int n, Src src, GridP<real> g, int *__restrict__ cell_of, int *__restrict__ count, Spc spc = Spc(),
                              int nt = 1, const unsigned char *__restrict__ keep = nullptr) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int c = -1;                                   // lanes past the end form their own run and add nothing
    if (i < n) {
        if (keep == nullptr || keep[i] != 0) {
            real x, y, z;
            src.get(i, x, y, z);
            c = cell_id(g, x, y, z) * nt + spc.of(i);
            cell_of[i] = c + g.one_based;
        } else {
            cell_of[i] = -1;
        }
    }
    int first, len;
    wave_run(c, first, len);
    if (c >= 0 && lane_id() == first) atomicAdd(&count[c], len);
}

// Scatter ids into their cell's range (arrival order inside a cell is arbitrary here)...
static __global__ void k_cell_scatter(int n, const int *__restrict__ cell_of, int one_based, const int *__restrict__ start,
                               int *__restrict__ fill, int *__restrict__ tmp) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = (i < n) ? cell_of[i] - one_based : -1;
    int first, len;
    wave_run(c, first, len);
    int base = 0;
    if (c >= 0 && lane_id() == first) base = start[c] + atomicAdd(&fill[c], len);
    base = __shfl(base, first);
    if (c >= 0) tmp[base + (lane_id() - first)] = i;
}

// The same for the engine's rebuilds, with each id's sort key (caller id) stored next to it: the ranking pass below then
// reads its cell-mates' keys from consecutive addresses instead of one dependent gather per cell-mate (cells of side
// >= r_list hold ~18 atoms: 0.22 -> 0.1 ms per rebuild at 10^7 atoms).
// (tag, optional: 64-bit ids that travel with the atoms -- decomposed domains order a cell's atoms by the low word of the
// GLOBAL id, which makes the cell order independent of the local numbering, i.e. of the history of migrations)
static __global__ void k_cell_scatter_keyed(int n, const int *__restrict__ cell_of, const int *__restrict__ start,
                                            int *__restrict__ fill, const int *__restrict__ key, int2 *__restrict__ tmp,
                                            const long long *__restrict__ tag = nullptr) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = (i < n) ? cell_of[i] : -1;
    int first, len;
    wave_run(c, first, len);
    int base = 0;
    if (c >= 0 && lane_id() == first) base = start[c] + atomicAdd(&fill[c], len);
    base = __shfl(base, first);
    if (c >= 0) tmp[base + (lane_id() - first)] = make_int2(i, tag ? (int)tag[i] : (key ? key[i] : i));
}
// (n_dev, optional: the number of items that were scattered, as a device word -- a re-sort with struck-out items launches over
// the upper bound; equal keys -- only the low words of two 64-bit tags can collide -- are ranked by the item index)
// (ties: keys that are caller ids or slots of the previous order are unique and the loop reads the keys alone, as in rounds 1-4
// -- 0.06 ms per rebuild at 10^7 atoms against 0.095 with the tie-break)
static __global__ void k_cell_rankfix_keyed(int n, const int *__restrict__ cell_of, const int *__restrict__ start,
                                            const int2 *__restrict__ tmp, int *__restrict__ order,
                                            const int *__restrict__ n_dev = nullptr, int ties = 1) {
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (q >= n) return;
    const int2 me = tmp[q];
    const int c = cell_of[me.x];
    const int s = start[c], e = start[c + 1];
    int rank = 0;
    if (ties) {
        for (int r = s; r < e; r++) {
            const int2 o = tmp[r];
            rank += (o.y < me.y || (o.y == me.y && o.x < me.x)) ? 1 : 0;
        }
    } else {
        for (int r = s; r < e; r++) rank += (tmp[r].y < me.y) ? 1 : 0;
    }
    order[s + rank] = me.x;
}

// ...then make it deterministic: inside each cell order by key (caller id), by counting smaller
// keys among the cell-mates (cells hold O(10) atoms).  order[q] = source index of slot q.
static __global__ void k_cell_rankfix(int n, const int *__restrict__ cell_of, int one_based, const int *__restrict__ start,
                               const int *__restrict__ tmp, const int *__restrict__ key, int *__restrict__ order) {
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    int i = tmp[q];
    int c = cell_of[i] - one_based;
    int s = start[c], e = start[c + 1];
    int ki = key ? key[i] : i;
    int rank = 0;
    for (int r = s; r < e; r++) {
        int j = tmp[r];
        int kj = key ? key[j] : j;
        rank += (kj < ki) ? 1 : 0;
    }
    order[s + rank] = i;
}

// ------------------------------------------------------------------------------------ scan
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

// exclusive scan of one tile per block, tile totals to sums[]
static __global__ void k_scan_tiles(const int *__restrict__ in, int *__restrict__ out, size_t n, int *__restrict__ sums) {
    __shared__ int wave_tot[SCAN_THREADS / WAVE];
    size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    int tsum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        tsum += v[k];
    }
    // inclusive scan of tsum over the wave via DPP-free shuffles (ints, cheap), then across waves
    int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    int inc = tsum;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == WAVE - 1) wave_tot[wv] = inc;
    __syncthreads();
    int wave_off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / WAVE; w++) {
        if (w < wv) wave_off += wave_tot[w];
        total += wave_tot[w];
    }
    int run = wave_off + inc - tsum;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0 && sums) sums[blockIdx.x] = total;
}

static __global__ void k_scan_add(int *__restrict__ out, size_t n, const int *__restrict__ offs) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += offs[i / SCAN_TILE];
}

// One workgroup scans up to a few ten thousand values in place (4096 per trip: coalesced 16-byte loads, a block scan, a
// carry): the count arrays of the decomposition's partitions, for which three launches of the tiled scan were three launch
// latencies behind a blocking read-back.
constexpr int SCAN_BLOCK_MAX = 65536;
static __global__ __launch_bounds__(1024) void k_scan_block(int *__restrict__ data, int n) {
    __shared__ int wtot[1024 / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    int carry = 0;
    for (int base = 0; base < n; base += 4096) {
        const int i0 = base + (int)threadIdx.x * 4;
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (i0 + k < n) ? data[i0 + k] : 0;
        const int s = v[0] + v[1] + v[2] + v[3];
        int inc = s;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int t = __shfl_up(inc, off);
            if (lane >= off) inc += t;
        }
        if (lane == WAVE - 1) wtot[wv] = inc;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 1024 / WAVE; w++) {
            if (w < wv) woff += wtot[w];
            tot += wtot[w];
        }
        int run = carry + woff + inc - s;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) data[i0 + k] = run;
            run += v[k];
        }
        carry += tot;
        __syncthreads();
    }
}

// in-place exclusive scan of int32 data[0..n) (n may exceed one tile: recursive tile sums)
struct Scanner {
    DevBuf<int> scratch;
    void run(int *data, size_t n, hipStream_t s) {
        if (n == 0) return;
        if (n <= (size_t)SCAN_BLOCK_MAX) {
            hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(1024), 0, s, data, (int)n);
            return;
        }
        size_t total = 0;
        for (size_t m = n; m > 1;) {
            m = (m + SCAN_TILE - 1) / SCAN_TILE;
            total += m;
            if (m == 1) break;
        }
        scratch.ensure(total + 1);
        level(data, n, scratch.ptr, s);
    }

  private:
    void level(int *data, size_t n, int *sums, hipStream_t s) {
        size_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
        hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)tiles), dim3(SCAN_THREADS), 0, s, data, data, n,
                           tiles > 1 ? sums : nullptr);
        if (tiles > 1) {
            level(sums, tiles, sums + tiles, s);
            hipLaunchKernelGGL(k_scan_add, dim3(blocks_for(n, 256)), dim3(256), 0, s, data, n, sums);
        }
    }
};

// Several small zero-fills in ONE launch (a hipMemsetAsync whose size is not a multiple of 16 bytes is two fill kernels,
// and every launch behind a blocking read-back is a launch latency on the critical path of a rebuild)
struct ZeroRanges {
    int *ptr[6];
    unsigned n[6];
};
static __global__ void k_zero_ranges(ZeroRanges z) {
    int *p = z.ptr[blockIdx.y];
    const unsigned n = z.n[blockIdx.y];
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0;
}
struct Zeros {
    ZeroRanges z{};
    int count = 0;
    unsigned most = 0;
    Zeros &add(int *p, size_t n) {
        if (n == 0) return *this;
        z.ptr[count] = p; z.n[count] = (unsigned)n; count++;
        most = n > most ? (unsigned)n : most;
        return *this;
    }
    void run(hipStream_t s) {
        if (count == 0) return;
        const unsigned bx = most <= 256 ? 1u : (most + 1023u) / 1024u;
        hipLaunchKernelGGL(k_zero_ranges, dim3(bx > 512u ? 512u : bx, count), dim3(256), 0, s, z);
    }
};

// ------------------------------------------------------------------------------------ gathers
template <typename real>
__device__ __forceinline__ void store_rec(Rec<real> *rec, float *te, int p, real x, real y, real z, float hs, float tev);
template <>
__device__ __forceinline__ void store_rec<double>(Rec<double> *rec, float *, int p, double x, double y, double z,
                                                  float hs, float tev) {
    Rec<double> r;
    r.x = x; r.y = y; r.z = z; r.hs = hs; r.te = tev;
    rec[p] = r;
}
template <>
__device__ __forceinline__ void store_rec<float>(Rec<float> *rec, float *te, int p, float x, float y, float z, float hs,
                                                 float tev) {
    Rec<float> r;
    r.x = x; r.y = y; r.z = z; r.hs = hs;
    rec[p] = r;
    te[p] = tev;
}
__device__ __forceinline__ void rec_params(const Rec<double> *rec, const float *, int p, float &hs, float &tev) {
    hs = rec[p].hs; tev = rec[p].te;
}
__device__ __forceinline__ void rec_params(const Rec<float> *rec, const float *te, int p, float &hs, float &tev) {
    hs = rec[p].hs; tev = te[p];
}

// Cell-ordered records hold the image of each atom INSIDE the primary box along periodic
// dimensions (the LDS-tiled kernels add explicit +-L shifts and never apply a minimum image);
// the number of box lengths removed is kept per atom so caller-order copies return the
// caller's unwrapped coordinates.  Packed 3 x 10 bits, biased by 512: a count lies in [-512, 511] (img_bound).
constexpr int IMG_BIAS = 512;
__device__ __forceinline__ int img_pack(int kx, int ky, int kz) {
    return (kx + IMG_BIAS) | ((ky + IMG_BIAS) << 10) | ((kz + IMG_BIAS) << 20);
}
// A count that has left the field must not carry into its neighbours': it is clamped (that atom's unwrapped image is lost, every
// other atom's stays right) and, where the engine hands positions back (fault != NULL), reported: the first atom to find
// fault[0] clear leaves its id + 1 there, the axis in fault[1] and the count in fault[2].  The word stays raised until the host
// clears it (NbSystem::image_fault), so a later rebuild does not overwrite the report.
__device__ __forceinline__ void img_bound(int &kx, int &ky, int &kz, int atom, int *__restrict__ fault) {
    if ((((unsigned)kx + IMG_BIAS) | ((unsigned)ky + IMG_BIAS) | ((unsigned)kz + IMG_BIAS)) < 2u * IMG_BIAS) return;
    const bool bx = kx < -IMG_BIAS || kx >= IMG_BIAS, by = ky < -IMG_BIAS || ky >= IMG_BIAS;
    if (fault && atomicCAS(fault, 0, atom + 1) == 0) { fault[1] = bx ? 0 : by ? 1 : 2; fault[2] = bx ? kx : by ? ky : kz; }
    kx = min(max(kx, -IMG_BIAS), IMG_BIAS - 1); ky = min(max(ky, -IMG_BIAS), IMG_BIAS - 1); kz = min(max(kz, -IMG_BIAS), IMG_BIAS - 1);
}
__device__ __forceinline__ void img_unpack(int v, int &kx, int &ky, int &kz) {
    kx = (v & 1023) - IMG_BIAS; ky = ((v >> 10) & 1023) - IMG_BIAS; kz = ((v >> 20) & 1023) - IMG_BIAS;
}
template <typename real>
__device__ __forceinline__ int wrap_into_box(real &p, real lo, real len, int periodic) {
    if (!periodic) return 0;
    const real k = floor((p - lo) / len);
    p -= k * len;
    return (int)k;
}

// cell-relative records: the periodic image of a coordinate (already relative to a cell origin) that lies next to that cell;
// returns the box lengths removed
__device__ __forceinline__ int rel_nearest_image(double &r, double len, int periodic) {
    if (!periodic) return 0;
    const double s = rint(r / len);
    r -= s * len;
    return (int)s;
}

// Build the cell-ordered state from caller-order arrays.  order[p] = caller id of slot p.
template <typename real>
__global__ void k_gather_user(int n, int n_owned, size_t pitch, GridP<real> g, const int *__restrict__ order,
                              const int *__restrict__ cell_of, const real *__restrict__ pos,
                              const emdee_lj_atom *__restrict__ atoms, const real *__restrict__ vel,
                              const real *__restrict__ inv_mass, Rec<real> *__restrict__ rec, float *__restrict__ te,
                              real *__restrict__ xb, real *__restrict__ v_out, real *__restrict__ im_out,
                              int *__restrict__ perm, int *__restrict__ inv_perm, int *__restrict__ cell_sorted,
                              int *__restrict__ img, int nt = 1, const long long *__restrict__ tag_in = nullptr,
                              long long *__restrict__ tag_out = nullptr, int ncell = 0, int *__restrict__ cstart = nullptr,
                              const int *__restrict__ tstart = nullptr, RelGrid rel_out = RelGrid{},
                              int *__restrict__ img_fault = nullptr) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    // (typed boxes and x sub-bins: the first slot of every CELL from the per-(cell, digit) starts -- rides here instead of
    // being a launch of its own)
    if (cstart) for (int c = p; c <= ncell; c += gridDim.x * blockDim.x) cstart[c] = tstart[(size_t)c * nt];
    if (p >= n) return;
    int i = order[p];
    if (tag_out) tag_out[p] = tag_in[i];
    real x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
    const int kx = wrap_into_box(x, g.lo[0], g.len[0], g.per[0]);
    const int ky = wrap_into_box(y, g.lo[1], g.len[1], g.per[1]);
    const int kz = wrap_into_box(z, g.lo[2], g.len[2], g.per[2]);
    int jx = kx, jy = ky, jz = kz;
    emdee_lj_atom a = atoms[i];
    if (sizeof(real) == 4 && rel_out.on) {                   // cell-relative records (RelGrid)
        double ox, oy, oz;
        rel_out.origin(cell_of[i] / nt, ox, oy, oz);
        double rx = (double)x - ox, ry = (double)y - oy, rz = (double)z - oz;
        jx += rel_nearest_image(rx, (double)g.len[0], g.per[0]);
        jy += rel_nearest_image(ry, (double)g.len[1], g.per[1]);
        jz += rel_nearest_image(rz, (double)g.len[2], g.per[2]);
        x = (real)rx; y = (real)ry; z = (real)rz;
    }
    img_bound(jx, jy, jz, i, img_fault);
    img[p] = img_pack(jx, jy, jz);
    store_rec<real>(rec, te, p, x, y, z, a.half_sigma, a.twice_sqrt_eps);
    xb[p] = x; xb[pitch + p] = y; xb[2 * pitch + p] = z;
    bool owned = i < n_owned;
    if (v_out) {
        for (int d = 0; d < 3; d++) v_out[d * pitch + p] = (owned && vel) ? vel[3 * (size_t)i + d] : (real)0;
    }
    if (im_out) im_out[p] = (owned && inv_mass) ? inv_mass[i] : (real)1;
    perm[p] = i;
    inv_perm[i] = p;
    cell_sorted[p] = cell_of[i] / nt;
}

// Re-sort an already cell-ordered state (MD rebuild). order[p] = OLD slot of new slot p.
// EDIT (NbSystem::resort_edit, a decomposed domain's rebuild in its own order): the old slots are the ids from now on
// (perm[p] = o: atoms that stay keep no other name, arrivals and new ghosts sit behind the old state), the image counts
// start afresh (the positions were wrapped by the ownership pass; an atom that changes owner takes no count along), only
// the *n_dev items that were kept exist, and their number goes out with the words of the rebuild's one read-back.
template <typename real, bool EDIT = false>
__global__ void k_gather_sorted(int n, size_t pitch, GridP<real> g, const int *__restrict__ order,
                                const int *__restrict__ cell_of, const Rec<real> *__restrict__ rec_in,
                                const float *__restrict__ te_in, const real *__restrict__ v_in,
                                const real *__restrict__ im_in, const int *__restrict__ perm_in,
                                const int *__restrict__ img_in, Rec<real> *__restrict__ rec, float *__restrict__ te,
                                real *__restrict__ xb, real *__restrict__ v_out, real *__restrict__ im_out,
                                int *__restrict__ perm, int *__restrict__ inv_perm, int *__restrict__ cell_sorted,
                                int *__restrict__ img, int nt = 1, const long long *__restrict__ tag_in = nullptr,
                                long long *__restrict__ tag_out = nullptr, const int *__restrict__ n_dev = nullptr,
                                int *__restrict__ n_out = nullptr, int ncell = 0, int *__restrict__ cstart = nullptr,
                                const int *__restrict__ tstart = nullptr, RelGrid rel_in = RelGrid{}, RelGrid rel_out = RelGrid{},
                                int *__restrict__ img_fault = nullptr) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (cstart) for (int c = p; c <= ncell; c += gridDim.x * blockDim.x) cstart[c] = tstart[(size_t)c * nt];
    if (EDIT) {
        n = min(n, *n_dev);
        if (p == 0 && n_out) *n_out = *n_dev;
    }
    if (p >= n) return;
    int o = order[p];
    Rec<real> r = rec_in[o];
    float hs, tev;
    rec_params(rec_in, te_in, o, hs, tev);
    int kx = 0, ky = 0, kz = 0;
    if (!EDIT) img_unpack(img_in[o], kx, ky, kz);
    if (sizeof(real) == 4 && (rel_in.on || rel_out.on)) {
        // cell-relative records: the absolute position in double, wrapped, then relative to the NEW cell (the cell the
        // binning pass found from the same position rounded to fp32: should the rounding have crossed a cell boundary, the
        // relative coordinate is a hair outside [0, width) -- as after any step)
        double ax = (double)r.x, ay = (double)r.y, az = (double)r.z, ox, oy, oz;
        if (rel_in.on) { rel_in.origin(rel_in.cell[o], ox, oy, oz); ax += ox; ay += oy; az += oz; }
        kx += wrap_into_box(ax, (double)g.lo[0], (double)g.len[0], g.per[0]);
        ky += wrap_into_box(ay, (double)g.lo[1], (double)g.len[1], g.per[1]);
        kz += wrap_into_box(az, (double)g.lo[2], (double)g.len[2], g.per[2]);
        if (rel_out.on) {
            rel_out.origin(cell_of[o] / nt, ox, oy, oz); ax -= ox; ay -= oy; az -= oz;
            // At a periodic face the binning (position rounded to fp32) and the wrap above (double) may pick different images of
            // the same atom -- fp32(L - 1e-6) is L, i.e. cell 0, while the double stays below L: take the image next to the cell
            // the atom was binned into (found on the GPU: an atom at z = 0 came out a whole box away from its cell, with an empty row)
            kx += rel_nearest_image(ax, (double)g.len[0], g.per[0]);
            ky += rel_nearest_image(ay, (double)g.len[1], g.per[1]);
            kz += rel_nearest_image(az, (double)g.len[2], g.per[2]);
        }
        r.x = (real)ax; r.y = (real)ay; r.z = (real)az;
    } else {
        kx += wrap_into_box(r.x, g.lo[0], g.len[0], g.per[0]);
        ky += wrap_into_box(r.y, g.lo[1], g.len[1], g.per[1]);
        kz += wrap_into_box(r.z, g.lo[2], g.len[2], g.per[2]);
    }
    int i = EDIT ? o : perm_in[o];
    img_bound(kx, ky, kz, i, img_fault);
    img[p] = img_pack(kx, ky, kz);
    store_rec<real>(rec, te, p, r.x, r.y, r.z, hs, tev);
    xb[p] = r.x; xb[pitch + p] = r.y; xb[2 * pitch + p] = r.z;
    if (v_out) {
        for (int d = 0; d < 3; d++) v_out[d * pitch + p] = v_in[d * pitch + o];
    }
    if (im_out) im_out[p] = im_in[o];
    if (tag_out) tag_out[p] = tag_in[o];
    perm[p] = i;
    inv_perm[i] = p;
    cell_sorted[p] = cell_of[o] / nt;
}

// Operator path, one pass per call: same list, new caller positions -> refresh the records in place, each atom in the
// periodic image nearest to where it was at build time (the caller may have wrapped or shifted it); raise flags[1] if an atom
// has moved more than sqrt(thr2) since the build (the caller then rebuilds and this refresh is discarded) and flags[5] if the
// LJAtom array is not one value repeated (which selects between the single-species and the general kernels).
template <typename real>
__global__ void k_refresh_check(int n, size_t pitch, GridP<real> g, const int *__restrict__ perm, const real *__restrict__ pos,
                                const emdee_lj_atom *__restrict__ atoms, const real *__restrict__ xb, Rec<real> *__restrict__ rec,
                                float *__restrict__ te, real thr2, int *__restrict__ flags, int typed = 0) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int i = perm[p];
    const emdee_lj_atom a = atoms[i], first = atoms[0];
    if (typed) {   // a typed box is SORTED by species: an atom whose LJAtom was edited invalidates the order and the list
        float hs0, te0;
        rec_params(rec, te, p, hs0, te0);
        if (__float_as_int(a.half_sigma) != __float_as_int(hs0) || __float_as_int(a.twice_sqrt_eps) != __float_as_int(te0)) flags[1] = 1;
    }
    const real bx = xb[p], by = xb[pitch + p], bz = xb[2 * pitch + p];
    const real dx = min_image(pos[3 * (size_t)i] - bx, g.plen[0], g.pinv[0]);
    const real dy = min_image(pos[3 * (size_t)i + 1] - by, g.plen[1], g.pinv[1]);
    const real dz = min_image(pos[3 * (size_t)i + 2] - bz, g.plen[2], g.pinv[2]);
    store_rec<real>(rec, te, p, bx + dx, by + dy, bz + dz, a.half_sigma, a.twice_sqrt_eps);
    if (dx * dx + dy * dy + dz * dz > thr2) flags[1] = 1;
    if (__float_as_int(a.half_sigma) != __float_as_int(first.half_sigma) ||
        __float_as_int(a.twice_sqrt_eps) != __float_as_int(first.twice_sqrt_eps))
        flags[5] = 1;
    // the first LJAtom itself rides along (flags[14], [15]): the host needs it for the single-species constants, and one
    // posted read-back of the words is cheaper than two copies and a synchronisation
    if (p == 0) { flags[14] = __float_as_int(first.half_sigma); flags[15] = __float_as_int(first.twice_sqrt_eps); }
}

// ------------------------------------------------------------------------------------ neighbour build
// One wavefront per atom (cell order).  The stencil is walked as rows of cells along x: in cell
// order a row segment is ONE contiguous slot range, so the 64 lanes read 64 consecutive records
// (coalesced), test the minimum-image distance, and compact the survivors with ballot + mbcnt.
constexpr int NBR_BLOCK = 256;

template <typename real>
__global__ __launch_bounds__(NBR_BLOCK) void k_nbr_build(int n, int n_owned, AtomView<real> atoms,
                                                          const int *__restrict__ perm,
                                                          const int *__restrict__ cell_sorted,
                                                          const int *__restrict__ start, GridP<real> g, real rlist2,
                                                          int *__restrict__ nbr, int stride, int *__restrict__ cnt,
                                                          int *__restrict__ overflow) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int p = __builtin_amdgcn_readfirstlane(blockIdx.x * (NBR_BLOCK / WAVE) + threadIdx.x / WAVE);
    if (p >= n) return;
    if (perm[p] >= n_owned) {   // ghosts act on owned atoms but own no row
        if (lane == 0) cnt[p] = 0;
        return;
    }
    real xi, yi, zi, hs_unused, te_unused;
    load_atom(atoms, p, xi, yi, zi, hs_unused, te_unused);
    const int c = cell_sorted[p];
    const int Mx = g.M[0], My = g.M[1], Mz = g.M[2], nd = g.nd;
    const int cx = c % Mx, cy = (c / Mx) % My, cz = c / (Mx * My);
    int *row = nbr + (size_t)p * stride;
    int count = 0;

    const int span = 2 * nd + 1;
    const int nz = g.per[2] ? min(span, Mz) : span;
    const int ny = g.per[1] ? min(span, My) : span;
    for (int kz = 0; kz < nz; kz++) {
        int zz = cz - nd + kz;
        if (g.per[2]) zz = ((zz % Mz) + Mz) % Mz;
        else if (zz < 0 || zz >= Mz) continue;
        for (int ky = 0; ky < ny; ky++) {
            int yy = cy - nd + ky;
            if (g.per[1]) yy = ((yy % My) + My) % My;
            else if (yy < 0 || yy >= My) continue;
            const int base = (zz * My + yy) * Mx;
            // x range of this row as one or two contiguous cell segments
            int xa0, xb0, xa1 = 0, xb1 = -1;
            int xa = cx - nd, xb = cx + nd;
            if (g.per[0]) {
                if (Mx <= span) { xa0 = 0; xb0 = Mx - 1; }
                else if (xa < 0) { xa0 = xa + Mx; xb0 = Mx - 1; xa1 = 0; xb1 = xb; }
                else if (xb >= Mx) { xa0 = xa; xb0 = Mx - 1; xa1 = 0; xb1 = xb - Mx; }
                else { xa0 = xa; xb0 = xb; }
            } else {
                xa0 = max(xa, 0); xb0 = min(xb, Mx - 1);
            }
            for (int seg = 0; seg < 2; seg++) {
                const int a = seg ? xa1 : xa0, b = seg ? xb1 : xb0;
                if (b < a) continue;
                const int s = start[base + a], e = start[base + b + 1];
                for (int q0 = s; q0 < e; q0 += WAVE) {
                    const int q = q0 + lane;
                    bool pass = false;
                    if (q < e && q != p) {
                        real xj, yj, zj, hs_j, te_j;
                        load_atom(atoms, q, xj, yj, zj, hs_j, te_j);
                        real dx = min_image(xi - xj, g.plen[0], g.pinv[0]);
                        real dy = min_image(yi - yj, g.plen[1], g.pinv[1]);
                        real dz = min_image(zi - zj, g.plen[2], g.pinv[2]);
                        pass = dx * dx + dy * dy + dz * dz < rlist2;
                    }
                    const unsigned long long mask = __ballot(pass);
                    if (pass) {
                        const int k = count + prefix_popc(mask);
                        if (k < stride) row[k] = q;
                    }
                    count += __popcll(mask);
                }
            }
        }
    }
    if (lane == 0) {
        cnt[p] = min(count, stride);
        if (count > stride) atomicMax(overflow, count);   // rare: host grows the stride and rebuilds
    }
}

// ------------------------------------------------------------------------------------ force kernel
// lj_force_nbr: one wavefront per atom.  Each block owns FORCE_ATOMS consecutive atoms (cell
// order), each of its 4 waves walks FORCE_ATOMS/4 of them: the 64 lanes read 64 neighbour
// indices per 256-B segment, gather one record each, evaluate the pair function, and the
// per-lane partial sums are combined with DPP row shifts/broadcasts.  Results are staged in
// LDS and stored once per block as unit-stride segments of the SoA force planes: no atomics,
// no pre-zeroing (the reference zero-fills and atomically accumulates, src/nonbonded.jl:88-104,
// 112-114).  Block ids are remapped so that each XCD (private L2) owns one contiguous span of
// atoms: neighbouring atoms gather the same records.
constexpr int FORCE_BLOCK = 256;
constexpr int FORCE_ATOMS = 64;

// (the body of k_lj_force_nbr and of its charged twin k_lj_force_nbr_q: CHG adds the reaction-field terms, lj_pair.hpp rf_pair)
template <typename real, int BITMASK, bool CHG, bool EWD = false>
__device__ __forceinline__ void lj_force_nbr_body(int n, int n_owned, int nblocks_per_xcd, const AtomView<real> &atoms,
                                                  const int *__restrict__ perm, const int *__restrict__ nbr, int stride,
                                                  const int *__restrict__ cnt, const GridP<real> &g, const LJModel<real> &model,
                                                  size_t pitch, real *__restrict__ frc, real *__restrict__ en,
                                                  real *__restrict__ vir, const int *__restrict__ guard, real *__restrict__ vt,
                                                  const Charges<real> &ch) {
    constexpr int NOUT = (BITMASK & EMDEE_TENSOR) ? 11 : 5;   // f, e, w (+ the six tensor components)
    __shared__ real s_out[NOUT][FORCE_ATOMS];
    if (guard != nullptr && *guard != 0) return;   // a step queued behind a rebuild request (emdee_dd_step): leave no trace
    const int lane = threadIdx.x & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    // XCD-aware remap: hardware deals consecutive block ids round-robin over the 8 XCDs
    const int lb = (blockIdx.x % NXCD) * nblocks_per_xcd + blockIdx.x / NXCD;
    const int first = lb * FORCE_ATOMS;
    if (first >= n) return;
    constexpr int PER_WAVE = FORCE_ATOMS / (FORCE_BLOCK / WAVE);

    for (int a = 0; a < PER_WAVE; a++) {
        const int slot = wv * PER_WAVE + a;
        const int p = first + slot;
        if (p >= n) break;
        real fx = 0, fy = 0, fz = 0, e = 0, w = 0;
        real tv[6] = {0, 0, 0, 0, 0, 0};   // (tensor pass only: xx, yy, zz, xy, xz, yz)
        if (perm[p] < n_owned) {
            real xi, yi, zi, hs_i, te_i;
            load_atom(atoms, p, xi, yi, zi, hs_i, te_i);
            const real q_i = CHG ? ch.q[p] : (real)0;
            const int m = cnt[p];
            const int *row = nbr + (size_t)p * stride;
            for (int k = lane; k < m; k += WAVE) {
                const int j = row[k];
                real xj, yj, zj, hs_j, te_j;
                load_atom(atoms, j, xj, yj, zj, hs_j, te_j);
                const real dx = min_image(xi - xj, g.plen[0], g.pinv[0]);
                const real dy = min_image(yi - yj, g.plen[1], g.pinv[1]);
                const real dz = min_image(zi - zj, g.plen[2], g.pinv[2]);
                const real r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < model.rc2) {   // strict test (Q2): listed-but-outside pairs cost nothing more
                    const real inv_r2 = fast_rcp(r2);
                    real E, W;
                    lj_interaction(r2, inv_r2, model, hs_i, te_i, hs_j, te_j, E, W);
                    if (CHG) {
                        real Ec, Wc;
                        if (EWD) ewald_pair(r2, q_i * ch.q[j], ch, Ec, Wc);
                        else rf_pair(r2, q_i * ch.q[j], ch, Ec, Wc);
                        E += Ec; W += Wc;
                    }
                    if (BITMASK & EMDEE_FORCES) {
                        const real wr2 = W * inv_r2;   // src/nonbonded.jl:139
                        fx += wr2 * dx; fy += wr2 * dy; fz += wr2 * dz;
                    }
                    if (BITMASK & EMDEE_ENERGIES) e += E;
                    if (BITMASK & EMDEE_VIRIALS) w += W;
                    if (BITMASK & EMDEE_TENSOR) {   // W / r2 d^a d^b
                        const real wr2 = W * inv_r2, hx = wr2 * dx, hy = wr2 * dy, hz = wr2 * dz;
                        tv[0] += hx * dx; tv[1] += hy * dy; tv[2] += hz * dz;
                        tv[3] += hx * dy; tv[4] += hx * dz; tv[5] += hy * dz;
                    }
                }
            }
            if (BITMASK & EMDEE_FORCES) {
                fx = wave_sum_to_lane63(fx); fy = wave_sum_to_lane63(fy); fz = wave_sum_to_lane63(fz);
            }
            if (BITMASK & EMDEE_ENERGIES) e = wave_sum_to_lane63(e);
            if (BITMASK & EMDEE_VIRIALS) w = wave_sum_to_lane63(w);
            if (BITMASK & EMDEE_TENSOR)
                for (int c = 0; c < 6; c++) tv[c] = wave_sum_to_lane63(tv[c]);
        }
        if (lane == WAVE - 1) {
            s_out[0][slot] = fx; s_out[1][slot] = fy; s_out[2][slot] = fz;
            s_out[3][slot] = (real)0.5 * e;   // half of each pair term per atom, src/nonbonded.jl:142-145
            s_out[4][slot] = (real)0.5 * w;
            if (BITMASK & EMDEE_TENSOR)
                for (int c = 0; c < 6; c++) s_out[(NOUT - 6) + c][slot] = (real)0.5 * tv[c];
        }
    }
    __syncthreads();
    const int t = threadIdx.x, col = t & (FORCE_ATOMS - 1), plane = t / FORCE_ATOMS;   // 4 planes of 64 threads
    if (first + col < n) {
        if ((BITMASK & EMDEE_FORCES) && plane < 3) frc[plane * pitch + first + col] = s_out[plane][col];
        if (plane == 3) {
            if (BITMASK & EMDEE_ENERGIES) en[first + col] = s_out[3][col];
            if (BITMASK & EMDEE_VIRIALS) vir[first + col] = s_out[4][col];
        }
        if (BITMASK & EMDEE_TENSOR)
            for (int c = plane; c < 6; c += FORCE_BLOCK / FORCE_ATOMS) vt[c * pitch + first + col] = s_out[(NOUT - 6) + c][col];
    }
}
template <typename real, int BITMASK>
__global__ __launch_bounds__(FORCE_BLOCK) void k_lj_force_nbr(int n, int n_owned, int nblocks_per_xcd,
                                                              AtomView<real> atoms, const int *__restrict__ perm,
                                                              const int *__restrict__ nbr, int stride,
                                                              const int *__restrict__ cnt, GridP<real> g,
                                                              LJModel<real> model, size_t pitch,
                                                              real *__restrict__ frc, real *__restrict__ en,
                                                              real *__restrict__ vir, const int *__restrict__ guard = nullptr,
                                                              real *__restrict__ vt = nullptr) {
    lj_force_nbr_body<real, BITMASK, false>(n, n_owned, nblocks_per_xcd, atoms, perm, nbr, stride, cnt, g, model, pitch, frc, en,
                                            vir, guard, vt, Charges<real>{});
}
// a charged engine's direct kernel: the same body with the reaction-field terms (its own name, so that the uncharged instances
// keep their signatures and code); BITMASK | EMDEE_EWALD: the Ewald real-space terms in their place
template <typename real, int BITMASK>
__global__ __launch_bounds__(FORCE_BLOCK) void k_lj_force_nbr_q(int n, int n_owned, int nblocks_per_xcd,
                                                                AtomView<real> atoms, const int *__restrict__ perm,
                                                                const int *__restrict__ nbr, int stride,
                                                                const int *__restrict__ cnt, GridP<real> g,
                                                                LJModel<real> model, size_t pitch,
                                                                real *__restrict__ frc, real *__restrict__ en,
                                                                real *__restrict__ vir, const int *__restrict__ guard,
                                                                real *__restrict__ vt, Charges<real> ch) {
    lj_force_nbr_body<real, BITMASK & ~EMDEE_EWALD, true, (BITMASK & EMDEE_EWALD) != 0>(n, n_owned, nblocks_per_xcd, atoms, perm, nbr, stride,
                                                                                        cnt, g, model, pitch, frc, en, vir, guard, vt, ch);
}

// ------------------------------------------------------------------------------------ integrator
// verlet_kick_drift: v += c f / m ; x += dt v, one pass (c = dt/2 for a lone half kick, dt when
// the closing half kick of the previous step is fused in), plus the rebuild trigger:
// |x - x_build|^2 > (skin/2)^2 raises *flag.
// noise != NULL: Langevin O step between the kick and the drift, v = c1 v + noise (k_langevin_noise).
template <typename real>
__global__ void k_kick_drift(int n, int n_owned, size_t pitch, const int *__restrict__ perm, Rec<real> *__restrict__ rec,
                             real *__restrict__ vel, const real *__restrict__ frc, const real *__restrict__ inv_mass,
                             real c, real dt, const real *__restrict__ xb, real thr2, int *__restrict__ flag,
                             const real *__restrict__ noise, real c1, const int *__restrict__ guard = nullptr) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (guard != nullptr && *guard != 0) {   // queued behind a rebuild request: do nothing and pass the request on
        if (p == 0) *flag = 1;
        return;
    }
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    Rec<real> r = rec[p];
    const real cm = inv_mass ? c * inv_mass[p] : c;
    real vx = vel[p] + cm * frc[p];
    real vy = vel[pitch + p] + cm * frc[pitch + p];
    real vz = vel[2 * pitch + p] + cm * frc[2 * pitch + p];
    if (noise) {
        vx = c1 * vx + noise[p]; vy = c1 * vy + noise[pitch + p]; vz = c1 * vz + noise[2 * pitch + p];
    }
    vel[p] = vx; vel[pitch + p] = vy; vel[2 * pitch + p] = vz;
    r.x += dt * vx; r.y += dt * vy; r.z += dt * vz;
    rec[p] = r;
    const real dx = r.x - xb[p], dy = r.y - xb[pitch + p], dz = r.z - xb[2 * pitch + p];
    if (dx * dx + dy * dy + dz * dz > thr2) *flag = 1;
}

// ---- Langevin thermostat (build-defined; the reference has neither integrator nor thermostat) ----------
// Three N(0,1) numbers per (seed, step, atom id): splitmix64-finalised counters + Box-Muller, so the noise of
// an atom does not depend on where the sort put it or on which rank owns it.  Same integer arithmetic as
// oracle/emdee_oracle.c orc_langevin_normals.
__device__ __forceinline__ unsigned long long lgv_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__device__ __forceinline__ void lgv_normals(unsigned long long seed, unsigned long long step, unsigned long long id,
                                            double out[3]) {
    const unsigned long long base = lgv_mix(seed + 0x9E3779B97F4A7C15ull * id);
    const unsigned long long s2 = lgv_mix(base ^ (0xD1B54A32D192ED03ull * (step + 1)));
    unsigned long long r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = lgv_mix(s2 + 0x9E3779B97F4A7C15ull * (unsigned long long)(j + 1));
    const double two53 = 1.0 / 9007199254740992.0, twopi = 6.283185307179586476925286766559;
    const double u1 = (double)((r[0] >> 11) + 1) * two53, v2 = (double)(r[1] >> 11) * two53;
    const double u3 = (double)((r[2] >> 11) + 1) * two53, v4 = (double)(r[3] >> 11) * two53;
    const double a = sqrt(-2.0 * log(u1)), b = sqrt(-2.0 * log(u3));
    double sn, cs;
    sincos(twopi * v2, &sn, &cs);
    out[0] = a * cs;
    out[1] = a * sn;
    out[2] = b * cos(twopi * v4);
}
// noise[p] = c2 sqrt(T / m_p) xi(seed, step, id_p) in cell order, one thread per atom (the fused step kernel's
// owner lanes only pick the three numbers up: the transcendental work stays out of the pair kernel)
template <typename real>
__global__ void k_langevin_noise(int n, int n_owned, size_t pitch, const int *__restrict__ perm,
                                 const long long *__restrict__ ids, const real *__restrict__ inv_mass,
                                 unsigned long long seed, unsigned long long step, double c2, double temperature,
                                 real *__restrict__ noise, const long long *__restrict__ tag = nullptr) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = perm[p];
    if (i >= n_owned) return;
    double xi[3];
    // (tag: the ids that travel with the atoms in cell order -- decomposed domains; ids: a caller-order array)
    lgv_normals(seed, step, (unsigned long long)(tag ? tag[p] : (ids ? ids[i] : (long long)i)), xi);
    const double amp = c2 * sqrt(temperature * (inv_mass ? (double)inv_mass[p] : 1.0));
    noise[p] = (real)(amp * xi[0]); noise[pitch + p] = (real)(amp * xi[1]); noise[2 * pitch + p] = (real)(amp * xi[2]);
}
template <typename real>
__global__ void k_langevin_normals_test(int n, unsigned long long seed, unsigned long long step, const long long *ids,
                                        double *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double xi[3];
    lgv_normals(seed, step, (unsigned long long)ids[i], xi);
    out[3 * i] = xi[0]; out[3 * i + 1] = xi[1]; out[3 * i + 2] = xi[2];
}

// verlet_kick: v += c f / m
template <typename real>
__global__ void k_kick(int n, int n_owned, size_t pitch, const int *__restrict__ perm, real *__restrict__ vel,
                       const real *__restrict__ frc, const real *__restrict__ inv_mass, real c) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    const real cm = inv_mass ? c * inv_mass[p] : c;
    vel[p] += cm * frc[p];
    vel[pitch + p] += cm * frc[pitch + p];
    vel[2 * pitch + p] += cm * frc[2 * pitch + p];
}

// ---- pressure coupling (emdee_md_scale_box; build-defined: the reference has no barostat) -----------------------------------
// The cell-ordered state rescaled where it lives, one thread per slot: x_d <- lo_d + mu_d (x_d - lo_d) on the record, v <- s v on
// the velocity planes (scale_vel = 0: the planes are not touched, bit for bit).  The arithmetic is fp64 in both precisions.
// Cell-relative records (fp32 integrators, RelGrid) go through the ABSOLUTE position: origin of the record's cell + record,
// scaled, and stored relative to the SAME origin again -- the cells of the old grid, which is what the re-sort that follows
// reads them with (NbSystem::resort: rel_in); the offset leaves [0, cell width) by (mu - 1) x, as after a long drift, and the
// re-sort brings it back.  Scaling the offset itself would move every atom towards its own cell's corner.
// Wrapped records stay consistent with the image counts: lo + mu (x + k len - lo) = [lo + mu (x - lo)] + k (mu len).
// member (with perm): one byte per caller id, non-zero for the atoms of rigid molecules, which the molecular scale moves by their
// centres of mass (settle.hpp k_molecule_scale) and this kernel leaves alone; NULL: every slot is scaled.
struct ScaleBox {
    double lo[3], mu[3];
};
template <typename real>
__global__ void k_cell_state_scale(int n, size_t pitch, Rec<real> *__restrict__ rec, real *__restrict__ vel, ScaleBox s,
                                   real vscale, int scale_vel, RelGrid rel, const unsigned char *__restrict__ member = nullptr,
                                   const int *__restrict__ perm = nullptr) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (member != nullptr && member[perm[p]]) return;
    Rec<real> r = rec[p];
    double ox = 0.0, oy = 0.0, oz = 0.0;
    if (sizeof(real) == 4 && rel.on) rel.origin(rel.cell[p], ox, oy, oz);
    // (a factor of exactly 1 -- an axis the barostat does not couple -- leaves the coordinate its bits: lo + (x - lo) rounds twice)
    if (s.mu[0] != 1.0) r.x = (real)(s.lo[0] + s.mu[0] * ((double)r.x + ox - s.lo[0]) - ox);
    if (s.mu[1] != 1.0) r.y = (real)(s.lo[1] + s.mu[1] * ((double)r.y + oy - s.lo[1]) - oy);
    if (s.mu[2] != 1.0) r.z = (real)(s.lo[2] + s.mu[2] * ((double)r.z + oz - s.lo[2]) - oz);
    rec[p] = r;
    if (scale_vel) {
        vel[p] *= vscale; vel[pitch + p] *= vscale; vel[2 * pitch + p] *= vscale;
    }
}

// ------------------------------------------------------------------------------------ caller-order copies
// One thread per cell-order slot p, written to the atom's id i = perm[p] -- or, when the ids have gaps (a decomposed domain
// that re-sorted its own records: NbSystem::resort_edit), to the rank of that id among the ids in use, cmap[i]: owned atoms
// first, then the ghosts, as every caller of these copies expects.  raw: the record's own coordinates, without the box
// lengths the sorts removed (the ownership pass of a decomposition wraps them anyway).
template <typename real>
__global__ void k_unsort(int n_owned, int n_total, size_t pitch, GridP<real> g, const int *__restrict__ img,
                         const int *__restrict__ perm, const int *__restrict__ cmap,
                         const Rec<real> *__restrict__ rec, const float *__restrict__ te, const real *__restrict__ vel,
                         const real *__restrict__ frc,
                         const real *__restrict__ en, const real *__restrict__ vir, const long long *__restrict__ tag,
                         real *__restrict__ pos_out,
                         real *__restrict__ vel_out, real *__restrict__ frc_out, real *__restrict__ en_out,
                         real *__restrict__ vir_out, emdee_lj_atom *__restrict__ atoms_out, long long *__restrict__ tag_out,
                         int raw, RelGrid rel = RelGrid{}) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_total) return;
    const int id = perm[p];
    const int i = cmap ? cmap[id] : id;
    if (pos_out) {
        Rec<real> r = rec[p];
        int kx = 0, ky = 0, kz = 0;
        if (!raw) img_unpack(img[p], kx, ky, kz);   // back to the caller's (unwrapped) image
        if (sizeof(real) == 4 && rel.on) {          // cell-relative records: origin + record + images, in double, rounded once
            double ox, oy, oz;
            rel.origin(rel.cell[p], ox, oy, oz);
            pos_out[3 * (size_t)i] = (real)((double)r.x + ox + (double)kx * (double)g.len[0]);
            pos_out[3 * (size_t)i + 1] = (real)((double)r.y + oy + (double)ky * (double)g.len[1]);
            pos_out[3 * (size_t)i + 2] = (real)((double)r.z + oz + (double)kz * (double)g.len[2]);
        } else {
            pos_out[3 * (size_t)i] = r.x + (real)kx * g.len[0];
            pos_out[3 * (size_t)i + 1] = r.y + (real)ky * g.len[1];
            pos_out[3 * (size_t)i + 2] = r.z + (real)kz * g.len[2];
        }
    }
    if (atoms_out) {
        emdee_lj_atom a;
        rec_params(rec, te, p, a.half_sigma, a.twice_sqrt_eps);
        atoms_out[i] = a;
    }
    if (tag_out) tag_out[i] = tag[p];
    if (id >= n_owned) return;
    if (vel_out) for (int d = 0; d < 3; d++) vel_out[3 * (size_t)i + d] = vel[d * pitch + p];
    if (frc_out) for (int d = 0; d < 3; d++) frc_out[3 * (size_t)i + d] = frc[d * pitch + p];
    if (en_out) en_out[i] = en[p];
    if (vir_out) vir_out[i] = vir[p];
}

// ids in use -> their ranks (cmap): live[id] = 1 for every id some slot carries, then an exclusive scan of live[]
static __global__ void k_mark_live(int n, const int *__restrict__ perm, int *__restrict__ live) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) live[perm[p]] = 1;
}

// sets *flag if any LJAtom differs (bitwise) from the first one
static __global__ void k_atoms_differ(int n, const emdee_lj_atom *__restrict__ atoms, int *__restrict__ flag) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const emdee_lj_atom a = atoms[i], b = atoms[0];
    if (__float_as_int(a.half_sigma) != __float_as_int(b.half_sigma) ||
        __float_as_int(a.twice_sqrt_eps) != __float_as_int(b.twice_sqrt_eps))
        *flag = 1;
}

// fused decomposed step: ghost records (not owned, never integrated here) follow the buffer swap
template <typename real>
__global__ void k_copy_ghost_records(int n, int n_owned, const int *__restrict__ perm, const Rec<real> *__restrict__ src,
                                     Rec<real> *__restrict__ dst) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && perm[p] >= n_owned) dst[p] = src[p];
}

// halo exchange helpers: gather positions (+ periodic shift) of listed caller ids;
// scatter received positions into ghost records
template <typename real>
struct ShiftTable {
    real s[27][3];
};

template <typename real>
__global__ void k_pack_positions(int n, const int *__restrict__ ids, const int *__restrict__ codes, int n_shifts,
                                 const int *__restrict__ inv_perm, const Rec<real> *__restrict__ rec,
                                 ShiftTable<real> tab, real *__restrict__ buf) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Rec<real> r = rec[inv_perm[ids[k]]];
    int c = codes ? codes[k] : 0;
    c = min(max(c, 0), n_shifts - 1);
    buf[3 * (size_t)k] = r.x + tab.s[c][0]; buf[3 * (size_t)k + 1] = r.y + tab.s[c][1]; buf[3 * (size_t)k + 2] = r.z + tab.s[c][2];
}

template <typename real>
__global__ void k_unpack_ghosts(int n, int first_id, const int *__restrict__ inv_perm, const real *__restrict__ buf,
                                Rec<real> *__restrict__ rec) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int p = inv_perm[first_id + k];
    Rec<real> r = rec[p];
    r.x = buf[3 * (size_t)k]; r.y = buf[3 * (size_t)k + 1]; r.z = buf[3 * (size_t)k + 2];
    rec[p] = r;
}

// neighbour rows of the direct (int32, cell-order slot) list as caller ids
static __global__ void k_export_rows(int n, int n_owned, const int *__restrict__ perm, const int *__restrict__ nbr, int stride,
                                     const int *__restrict__ cnt, int *__restrict__ counts, int *__restrict__ out, int capacity,
                                     const int *__restrict__ cmap = nullptr) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    const int i = cmap ? cmap[perm[p]] : perm[p];
    const int m = cnt[p];
    counts[i] = m;
    for (int e = 0; e < m && e < capacity; e++) {
        const int j = perm[nbr[(size_t)p * stride + e]];
        out[(size_t)i * capacity + e] = cmap ? cmap[j] : j;
    }
}

// ------------------------------------------------------------------------------------ exclusions and 1-4 pairs
// (the hooks of src/modelling.jl:197-200.  The reference parses lj14scale and nothing consumes it --
// its hot path sums every pair, src/nonbonded.jl:129-150 -- so these are build-defined: pairs named by the caller are struck
// from the neighbour rows right after every build (the pair loop gets no mask), and the 1-4 pairs among them are
// evaluated on their own, scaled.)  Both tables are symmetric CSR lists over ids (PairKeys), partners ascending.
// position of j in idx[lo, hi), or -1
__device__ __forceinline__ int csr_find(const int *__restrict__ idx, int lo, int hi, long long j) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int v = idx[mid];
        if (v == j) return mid;
        if (v < j) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// How a row filter and k_pairs14 name an atom: by its tag (the global id that travels with it) when the engine carries tags
// -- a decomposed engine (dd.hpp), owned atoms and ghosts alike -- else by its caller index (perm).  n_tab: ids 0 .. n_tab - 1
// have rows (an id beyond names no pair).  With a 1-4 table (s14 != NULL) the filter also records, for every 1-4 partner of an
// owned atom, the cell-order slot of the entry it strikes, in the table's order: s14[k] for idx14[k], -1 when the partner is
// not in the row (beyond the list radius at the build, so beyond rc until the next one).  k_pairs14 sums those slots.
// An Ewald engine (sx != NULL) has the slot of EVERY struck entry recorded the same way, in the order of the struck CSR
// (ex_idx): k_ewald_struck takes the reciprocal sum's share of those pairs back.  Other engines pass NULL and record nothing.
struct PairKeys {
    const long long *tag;
    int n_tab;
    const int *start14, *idx14;
    int *s14;
    int *sx;
};
__device__ __forceinline__ long long pair_key(const PairKeys &k, const int *__restrict__ perm, int slot) {
    return k.tag ? k.tag[slot] : (long long)perm[slot];
}

// Bonded terms (emdee_*_set_bonded; topology_dev.hpp Topology): a CSR per atom key, keyed as PairKeys.  Row gi lists the atom's
// bonded partners (pidx[pstart[gi] .. pstart[gi + 1]), ascending) and its terms (terms[tstart[gi] .. tstart[gi + 1])): x = kind
// | role << 2 (role: the atom's position in the term), y, z, w = the other atoms of the term, in term order, as positions in
// the atom's partner list.  The row filter records each partner's cell-order slot in slots[] (-1: not in the row at the build).
struct BondedKeys {
    int n_tab;
    const int *pstart, *pidx;
    int *slots;                                              // NULL: no bonded table
    const int *tstart;
    const int4 *terms;
    const int *tid;                                          // per term entry: the term's number over all kinds (error reports)
};

// The loop both row filters share (k_filter_rows, brick.hpp k_brick_filter): owned atom p's row of m entries without its struck
// entries (ex_start / ex_idx: exclusions and 1-4 pairs together), compacted in place, the 1-4 and bonded partners' slots recorded.
// at(e): the row's e-th entry (a reference); slot(entry): its cell-order slot.  Returns the new length, or -1 if p has nothing
// struck (its row is left as it is).
template <class At, class Slot>
__device__ __forceinline__ int strike_row(const PairKeys &keys, const BondedKeys &bk, const int *__restrict__ perm,
                                          const int *__restrict__ ex_start, const int *__restrict__ ex_idx, int p, int m, At at,
                                          Slot slot) {
    const long long gi = pair_key(keys, perm, p);
    const bool ex = gi >= 0 && gi < keys.n_tab && ex_start[gi] < ex_start[gi + 1];
    const bool bd = bk.slots != nullptr && gi >= 0 && gi < bk.n_tab && bk.pstart[gi] < bk.pstart[gi + 1];
    if (!ex && !bd) return -1;
    const int lo = ex ? ex_start[gi] : 0, hi = ex ? ex_start[gi + 1] : 0;
    const int lo14 = (ex && keys.s14) ? keys.start14[gi] : 0, hi14 = (ex && keys.s14) ? keys.start14[gi + 1] : 0;
    for (int k = lo14; k < hi14; k++) keys.s14[k] = -1;
    if (keys.sx)
        for (int k = lo; k < hi; k++) keys.sx[k] = -1;
    const int lob = bd ? bk.pstart[gi] : 0, hib = bd ? bk.pstart[gi + 1] : 0;
    for (int k = lob; k < hib; k++) bk.slots[k] = -1;
    int w = 0;
    for (int e = 0; e < m; e++) {
        const auto ent = at(e);
        const int q = slot(ent);
        const long long gj = pair_key(keys, perm, q);
        if (lob < hib) {
            const int k = csr_find(bk.pidx, lob, hib, gj);
            if (k >= 0) bk.slots[k] = q;
        }
        const int kx = csr_find(ex_idx, lo, hi, min(gj, (long long)keys.n_tab));
        if (kx < 0) {
            if (w != e) at(w) = ent;
            w++;
        } else {
            if (keys.sx) keys.sx[kx] = q;
            if (lo14 < hi14) {
                const int k = csr_find(keys.idx14, lo14, hi14, gj);
                if (k >= 0) keys.s14[k] = q;
            }
        }
    }
    return ex ? w : -1;
}

// rows of the direct (int32, cell-order slot) list without their excluded entries
static __global__ void k_filter_rows(int n, int n_owned, const int *__restrict__ perm, int *__restrict__ nbr, int stride,
                                     int *__restrict__ cnt, const int *__restrict__ ex_start, const int *__restrict__ ex_idx,
                                     PairKeys keys, BondedKeys bk) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    int *row = nbr + (size_t)p * stride;
    const int w = strike_row(keys, bk, perm, ex_start, ex_idx, p, min(cnt[p], stride), [&](int e) -> int & { return row[e]; },
                             [](int q) { return q; });
    if (w >= 0) cnt[p] = w;
}

// 1-4 pairs: owner-computes over the slots the row filter recorded at the last build (k_filter_rows / k_brick_filter) -- no
// atomics, the table's order of summation, half of a pair's E and W to the owner.  The partner may be an owned atom or a ghost
// image (the records hold its shifted coordinates).  The scaled pair terms are ADDED to what the list kernels have left -- in
// the cell-ordered arrays, or in the caller's arrays when the operator path had its results written there (user_*: caller
// order).  A pair missing from the rows is beyond rc + skin at the build, so beyond rc while the list is valid.
// (TENSOR: the tensor pass's instance; the force and observable passes keep the instance without the six sums)
// (CHG: the body of k_pairs14_q, a charged engine's: the pair's reaction-field terms scaled by ch.scale14 on top)
// (EWD: an Ewald engine's: the pair's Coulomb part is ch.scale14 qq / r with NO cutoff test -- k_ewald_struck adds the
// correction every struck pair gets -- and the LJ part keeps its cutoff test)
template <typename real, bool TENSOR, bool CHG, bool EWD = false>
__device__ __forceinline__ void pairs14_body(int n, int n_owned, size_t pitch, const AtomView<real> &atoms, const int *__restrict__ perm,
                                             const PairKeys &keys, const GridP<real> &g, const LJModel<real> &model, real scale,
                                             int bitmask, real *__restrict__ frc, real *__restrict__ en, real *__restrict__ vir,
                                             real *__restrict__ user_f, real *__restrict__ user_e, real *__restrict__ user_w,
                                             real *__restrict__ vt, real *__restrict__ user_vt, const Charges<real> &ch) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = perm[p];
    if (i >= n_owned) return;
    const long long gi = pair_key(keys, perm, p);
    if (gi < 0 || gi >= keys.n_tab) return;
    const int lo = keys.start14[gi], hi = keys.start14[gi + 1];
    if (lo == hi) return;
    real xi, yi, zi, hs_i, te_i;
    load_atom(atoms, p, xi, yi, zi, hs_i, te_i);
    real fx = 0, fy = 0, fz = 0, e = 0, w = 0;
    real tv[6] = {0, 0, 0, 0, 0, 0};                           // (tensor pass: the scaled terms of the tensor, as of w)
    const real q_i = CHG ? ch.q[p] : (real)0;
    real cfx = 0, cfy = 0, cfz = 0, ce = 0, cw = 0;            // (charged: the reaction-field terms, scaled by ch.scale14)
    real ctv[6] = {0, 0, 0, 0, 0, 0};
    for (int k = lo; k < hi; k++) {
        const int q = keys.s14[k];
        if (q < 0) continue;
        real xj, yj, zj, hs_j, te_j;
        load_atom(atoms, q, xj, yj, zj, hs_j, te_j);
        const real dx = min_image(xi - xj, g.plen[0], g.pinv[0]);
        const real dy = min_image(yi - yj, g.plen[1], g.pinv[1]);
        const real dz = min_image(zi - zj, g.plen[2], g.pinv[2]);
        const real r2 = dx * dx + dy * dy + dz * dz;
        if (EWD) {                                             // bare Coulomb, whatever the distance
            const real inv_r2 = (real)1 / r2;
            const real Wc = q_i * ch.q[q] * sqrt(inv_r2), cr2 = Wc * inv_r2;
            cfx += cr2 * dx; cfy += cr2 * dy; cfz += cr2 * dz;
            ce += Wc; cw += Wc;
            if (TENSOR) {
                const real hx = cr2 * dx, hy = cr2 * dy, hz = cr2 * dz;
                ctv[0] += hx * dx; ctv[1] += hy * dy; ctv[2] += hz * dz;
                ctv[3] += hx * dy; ctv[4] += hx * dz; ctv[5] += hy * dz;
            }
        }
        if (r2 < model.rc2) {                                  // CUTOFF semantics, as the list kernels
            const real inv_r2 = (real)1 / r2;
            real E, W;
            lj_interaction(r2, inv_r2, model, hs_i, te_i, hs_j, te_j, E, W);
            const real wr2 = W * inv_r2;                      // src/nonbonded.jl:139
            fx += wr2 * dx; fy += wr2 * dy; fz += wr2 * dz;
            e += E; w += W;
            if (TENSOR) {
                const real hx = wr2 * dx, hy = wr2 * dy, hz = wr2 * dz;
                tv[0] += hx * dx; tv[1] += hy * dy; tv[2] += hz * dz;
                tv[3] += hx * dy; tv[4] += hx * dz; tv[5] += hy * dz;
            }
            if (CHG && !EWD) {
                real Ec, Wc;
                rf_pair(r2, q_i * ch.q[q], ch, Ec, Wc);
                const real cr2 = Wc * inv_r2;
                cfx += cr2 * dx; cfy += cr2 * dy; cfz += cr2 * dz;
                ce += Ec; cw += Wc;
                if (TENSOR) {
                    const real hx = cr2 * dx, hy = cr2 * dy, hz = cr2 * dz;
                    ctv[0] += hx * dx; ctv[1] += hy * dy; ctv[2] += hz * dz;
                    ctv[3] += hx * dy; ctv[4] += hx * dz; ctv[5] += hy * dz;
                }
            }
        }
    }
    fx *= scale; fy *= scale; fz *= scale;
    e *= (real)0.5 * scale; w *= (real)0.5 * scale;           // src/nonbonded.jl:142-145: half of a pair's E and W to either atom
    for (int c = 0; c < 6; c++) tv[c] *= (real)0.5 * scale;
    if (CHG) {
        const real sc = ch.scale14, hc = (real)0.5 * ch.scale14;
        fx += sc * cfx; fy += sc * cfy; fz += sc * cfz;
        e += hc * ce; w += hc * cw;
        for (int c = 0; c < 6; c++) tv[c] += hc * ctv[c];
    }
    if (user_f != nullptr || user_e != nullptr || user_w != nullptr || (TENSOR && user_vt != nullptr)) {
        if ((bitmask & EMDEE_FORCES) && user_f) { user_f[3 * (size_t)i] += fx; user_f[3 * (size_t)i + 1] += fy; user_f[3 * (size_t)i + 2] += fz; }
        if ((bitmask & EMDEE_ENERGIES) && user_e) user_e[i] += e;
        if ((bitmask & EMDEE_VIRIALS) && user_w) user_w[i] += w;
        if (TENSOR && user_vt)
            for (int c = 0; c < 6; c++) user_vt[6 * (size_t)i + c] += tv[c];
    } else {
        if (bitmask & EMDEE_FORCES) { frc[p] += fx; frc[pitch + p] += fy; frc[2 * pitch + p] += fz; }
        if (bitmask & EMDEE_ENERGIES) en[p] += e;
        if (bitmask & EMDEE_VIRIALS) vir[p] += w;
        if (TENSOR)
            for (int c = 0; c < 6; c++) vt[c * pitch + p] += tv[c];
    }
}
template <typename real, bool TENSOR = false>
__global__ void k_pairs14(int n, int n_owned, size_t pitch, AtomView<real> atoms, const int *__restrict__ perm, PairKeys keys,
                          GridP<real> g, LJModel<real> model, real scale, int bitmask, real *__restrict__ frc, real *__restrict__ en,
                          real *__restrict__ vir, real *__restrict__ user_f, real *__restrict__ user_e, real *__restrict__ user_w,
                          real *__restrict__ vt = nullptr, real *__restrict__ user_vt = nullptr) {
    pairs14_body<real, TENSOR, false>(n, n_owned, pitch, atoms, perm, keys, g, model, scale, bitmask, frc, en, vir, user_f, user_e,
                                      user_w, vt, user_vt, Charges<real>{});
}
// a charged engine's 1-4 kernel (its own name: the uncharged instances keep their signatures and code)
template <typename real, bool TENSOR, bool EWD = false>
__global__ void k_pairs14_q(int n, int n_owned, size_t pitch, AtomView<real> atoms, const int *__restrict__ perm, PairKeys keys,
                            GridP<real> g, LJModel<real> model, real scale, int bitmask, real *__restrict__ frc, real *__restrict__ en,
                            real *__restrict__ vir, real *__restrict__ user_f, real *__restrict__ user_e, real *__restrict__ user_w,
                            real *__restrict__ vt, real *__restrict__ user_vt, Charges<real> ch) {
    pairs14_body<real, TENSOR, true, EWD>(n, n_owned, pitch, atoms, perm, keys, g, model, scale, bitmask, frc, en, vir, user_f, user_e,
                                          user_w, vt, user_vt, ch);
}

// Ewald engines: the correction of every pair struck from the rows (exclusions and 1-4 pairs; lj_pair.hpp ewald_struck_pair).
// Owner-computes over the slots the row filter recorded for the struck CSR (PairKeys::sx) -- no atomics, the table's order of
// summation, half of a pair's E and W to the owner, added to the cell-ordered arrays.  Minimum image, no cutoff test.  A
// partner missing from the rows (farther than rc + skin at the build) leaves the pair out and writes its entry's number + 1 to
// *err (read by the host: NbSystem::check_ewald).
template <typename real, bool TENSOR>
__global__ void k_ewald_struck(int n, int n_owned, size_t pitch, AtomView<real> atoms, const int *__restrict__ perm, PairKeys keys,
                               const int *__restrict__ ex_start, GridP<real> g, int bitmask, real *__restrict__ frc,
                               real *__restrict__ en, real *__restrict__ vir, real *__restrict__ vt, Charges<real> ch,
                               int *__restrict__ err) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (perm[p] >= n_owned) return;
    const long long gi = pair_key(keys, perm, p);
    if (gi < 0 || gi >= keys.n_tab) return;
    const int lo = ex_start[gi], hi = ex_start[gi + 1];
    if (lo == hi) return;
    real xi, yi, zi, hs_i, te_i;
    load_atom(atoms, p, xi, yi, zi, hs_i, te_i);
    const real q_i = ch.q[p];
    real fx = 0, fy = 0, fz = 0, e = 0, w = 0;
    real tv[6] = {0, 0, 0, 0, 0, 0};
    for (int k = lo; k < hi; k++) {
        const int q = keys.sx[k];
        if (q < 0 || q >= n) { *err = k + 1; continue; }
        real xj, yj, zj, hs_j, te_j;
        load_atom(atoms, q, xj, yj, zj, hs_j, te_j);
        const real dx = min_image(xi - xj, g.plen[0], g.pinv[0]);
        const real dy = min_image(yi - yj, g.plen[1], g.pinv[1]);
        const real dz = min_image(zi - zj, g.plen[2], g.pinv[2]);
        const real r2 = dx * dx + dy * dy + dz * dz;
        real E, W;
        ewald_struck_pair(r2, q_i * ch.q[q], ch, E, W);
        const real wr2 = W / r2;
        fx += wr2 * dx; fy += wr2 * dy; fz += wr2 * dz;
        e += E; w += W;
        if (TENSOR) {
            const real hx = wr2 * dx, hy = wr2 * dy, hz = wr2 * dz;
            tv[0] += hx * dx; tv[1] += hy * dy; tv[2] += hz * dz;
            tv[3] += hx * dy; tv[4] += hx * dz; tv[5] += hy * dz;
        }
    }
    if (bitmask & EMDEE_FORCES) { frc[p] += fx; frc[pitch + p] += fy; frc[2 * pitch + p] += fz; }
    if (bitmask & EMDEE_ENERGIES) en[p] += (real)0.5 * e;
    if (bitmask & EMDEE_VIRIALS) vir[p] += (real)0.5 * w;
    if (TENSOR)
        for (int c = 0; c < 6; c++) vt[c * pitch + p] += (real)0.5 * tv[c];
}

// The charge plane of a charged engine: sqrt(K) q of the atom in every cell-order slot, looked up by the key it carries (tag or
// caller id, as PairKeys) in the table of n_tab keys.  A key outside the table leaves 0 in the slot and raises *err (the host
// refuses to step: NbSystem::check_charges).
template <typename real>
__global__ void k_fill_charges(int n, const int *__restrict__ perm, const long long *__restrict__ tag, const double *__restrict__ tab,
                               long long n_tab, real *__restrict__ q, int *__restrict__ err) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long key = tag ? tag[p] : (long long)perm[p];
    const bool ok = key >= 0 && key < n_tab;
    q[p] = ok ? (real)tab[key] : (real)0;
    if (!ok) *err = 1;
}

// Bonded terms: owner-computes over the slots the row filter recorded at the last build -- no atomics, the row's order of
// summation.  Each owned atom evaluates every term it belongs to in full (chained minimum images along the term's bonds: the
// term is unwrapped) and keeps its own force and a 1/2, 1/3, 1/4 share of the term's U, of W = sum_a x_a . F_a and of the
// symmetrised tensor sum_a x_a (x) F_a.  A partner missing from the rows (farther than rc + skin at the build) leaves the term
// out and writes its number + 1 to *err (read by the host: NbSystem::check_bonded).
// prm: 3 values per term entry -- bond {k, r0, 0}, angle {k, theta0, 0}, torsion {k, n, phase}.
// The formula of one term -- bonded_term: U and the forces at unwrapped positions, zero force at singular geometries -- is
// plain C++ in bonded.hpp, where a host program tests it.
template <typename real, bool TENSOR = false>
__global__ __launch_bounds__(256) void k_bonded(int n, int n_owned, size_t pitch, AtomView<real> atoms, const int *__restrict__ perm, PairKeys keys,
                         BondedKeys bk, const real *__restrict__ prm, GridP<real> g, int bitmask, real *__restrict__ frc,
                         real *__restrict__ en, real *__restrict__ vir, real *__restrict__ vt, int *__restrict__ err) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = perm[p];
    if (i >= n_owned) return;
    const long long gi = pair_key(keys, perm, p);
    if (gi < 0 || gi >= bk.n_tab) return;
    const int lo = bk.tstart[gi], hi = bk.tstart[gi + 1];
    if (lo == hi) return;
    const int base = bk.pstart[gi];
    real fx = 0, fy = 0, fz = 0, e = 0, w = 0;
    real tv[6] = {0, 0, 0, 0, 0, 0};
    for (int t = lo; t < hi; t++) {
        const int4 d = bk.terms[t];
        const int kind = d.x & 3, role = d.x >> 2, nat = kind + 1;
        // the term's atoms in term order: this atom at `role`, the others from the recorded slots
        int s[4];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int k = a < role ? a : a - 1;              // position among the other atoms
            const int loc = k == 0 ? d.y : (k == 1 ? d.z : d.w);
            const int q = (a < nat && a != role) ? bk.slots[base + loc] : p;
            ok = ok && q >= 0;
            s[a] = q;
        }
        if (!ok) { *err = bk.tid[t] + 1; continue; }
        real u[4][3], F[4][3];                                // u: unwrapped positions relative to the term's first atom
        real px, py, pz;
        {
            real hs, te;
            load_atom(atoms, s[0], px, py, pz, hs, te);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) u[0][c] = 0;
#pragma unroll
        for (int a = 1; a < 4; a++) {
            real x, y, z, hs, te;
            load_atom(atoms, s[a], x, y, z, hs, te);
            u[a][0] = u[a - 1][0] + min_image(x - px, g.plen[0], g.pinv[0]);
            u[a][1] = u[a - 1][1] + min_image(y - py, g.plen[1], g.pinv[1]);
            u[a][2] = u[a - 1][2] + min_image(z - pz, g.plen[2], g.pinv[2]);
            px = x; py = y; pz = z;
        }
        const real U = bonded_term<real>(kind, u, prm[3 * (size_t)t], prm[3 * (size_t)t + 1], prm[3 * (size_t)t + 2], F);
        real T[6] = {0, 0, 0, 0, 0, 0};                       // sum_a u_a (x) F_a, symmetrised
#pragma unroll
        for (int a = 0; a < 4; a++) {
            T[0] += u[a][0] * F[a][0]; T[1] += u[a][1] * F[a][1]; T[2] += u[a][2] * F[a][2];
            T[3] += (real)0.5 * (u[a][0] * F[a][1] + u[a][1] * F[a][0]);
            T[4] += (real)0.5 * (u[a][0] * F[a][2] + u[a][2] * F[a][0]);
            T[5] += (real)0.5 * (u[a][1] * F[a][2] + u[a][2] * F[a][1]);
        }
        const real share = (real)1 / (real)nat;
        fx += role == 0 ? F[0][0] : role == 1 ? F[1][0] : role == 2 ? F[2][0] : F[3][0];
        fy += role == 0 ? F[0][1] : role == 1 ? F[1][1] : role == 2 ? F[2][1] : F[3][1];
        fz += role == 0 ? F[0][2] : role == 1 ? F[1][2] : role == 2 ? F[2][2] : F[3][2];
        e += share * U;
        w += share * (T[0] + T[1] + T[2]);
        if (TENSOR)
            for (int c = 0; c < 6; c++) tv[c] += share * T[c];
    }
    if (bitmask & EMDEE_FORCES) { frc[p] += fx; frc[pitch + p] += fy; frc[2 * pitch + p] += fz; }
    if (bitmask & EMDEE_ENERGIES) en[p] += e;
    if (bitmask & EMDEE_VIRIALS) vir[p] += w;
    if (TENSOR)
        for (int c = 0; c < 6; c++) vt[c * pitch + p] += tv[c];
}

// ------------------------------------------------------------------------------------ reductions
// The two-stage fp64 sums are reduce.hpp's; here the terms of the energy and the tensor entries.
// [0] = sum e, [1] = kinetic energy (with optional pending half kick c f/m), [2] = sum w
template <typename real>
struct EnergySums {
    static constexpr int SUMS = 3, MAXES = 0;
    int n_owned;
    size_t pitch;
    const int *perm;
    const real *en, *vir, *vel, *frc, *inv_mass;
    real c;
    __device__ __forceinline__ void operator()(int p, double *acc) const {
        if (perm[p] >= n_owned) return;
        if (en) acc[0] += (double)en[p];
        if (vir) acc[2] += (double)vir[p];
        if (vel) {
            const real im = inv_mass ? inv_mass[p] : (real)1;
            double k2 = 0.0;
            for (int d = 0; d < 3; d++) {
                double v = (double)vel[d * pitch + p] + (double)(c * im) * (double)frc[d * pitch + p];
                k2 += v * v;
            }
            acc[1] += im != (real)0 ? 0.5 * k2 / (double)im : 0.0;   // (a massless atom, a virtual site: exactly 0)
        }
    }
};

// Pressure tensor sums: [0..5] = sum of the owned atoms' virial tensors W_i, [6..11] = kinetic tensor sum m_i v_i^a v_i^b (with the
// velocities EnergySums takes for its kinetic energy, no pending kick), both in the order (xx, yy, zz, xy, xz, yz)
constexpr int TENSOR_SUMS = 12;
template <typename real>
struct TensorSums {
    static constexpr int SUMS = TENSOR_SUMS, MAXES = 0;
    int n_owned;
    size_t pitch;
    const int *perm;
    const real *vt, *vel, *inv_mass;
    __device__ __forceinline__ void operator()(int p, double *s) const {
        if (perm[p] >= n_owned) return;
        for (int c = 0; c < 6; c++) s[c] += (double)vt[c * pitch + p];
        if (vel) {
            const real im = inv_mass ? inv_mass[p] : (real)1;
            const double m = im != (real)0 ? 1.0 / (double)im : 0.0;   // (a massless atom, a virtual site: exactly 0)
            const double vx = (double)vel[p], vy = (double)vel[pitch + p], vz = (double)vel[2 * pitch + p];
            s[6] += m * vx * vx; s[7] += m * vy * vy; s[8] += m * vz * vz;
            s[9] += m * vx * vy; s[10] += m * vx * vz; s[11] += m * vy * vz;
        }
    }
};

// per-atom tensors in caller order, owned atoms only: out[6 i + c] = vt[c][p] (i: k_unsort's caller index)
template <typename real>
__global__ void k_unsort_tensor(int n_owned, int n_total, size_t pitch, const int *__restrict__ perm, const int *__restrict__ cmap,
                                const real *__restrict__ vt, real *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_total) return;
    const int id = perm[p];
    const int i = cmap ? cmap[id] : id;
    if (i >= n_owned) return;
    for (int c = 0; c < 6; c++) out[6 * (size_t)i + c] = vt[c * pitch + p];
}

// list statistics: out[0] = entries, out[1] = max row, out[2] = entries with r2 < rc2
template <typename real>
__global__ __launch_bounds__(RED_BLOCK) void k_list_stats(int n, AtomView<real> atoms, const int *__restrict__ nbr,
                                                          int stride, const int *__restrict__ cnt, GridP<real> g,
                                                          real rc2, int count_pairs,
                                                          unsigned long long *__restrict__ out) {
    unsigned long long entries = 0, inside = 0;
    int mx = 0;
    for (int p = blockIdx.x * RED_BLOCK + threadIdx.x; p < n; p += gridDim.x * RED_BLOCK) {
        int m = cnt[p];
        entries += (unsigned long long)m;
        mx = max(mx, m);
        if (count_pairs) {
            real xi, yi, zi, h, t;
            load_atom(atoms, p, xi, yi, zi, h, t);
            for (int k = 0; k < m; k++) {
                real xj, yj, zj;
                load_atom(atoms, nbr[(size_t)p * stride + k], xj, yj, zj, h, t);
                real dx = min_image(xi - xj, g.plen[0], g.pinv[0]);
                real dy = min_image(yi - yj, g.plen[1], g.pinv[1]);
                real dz = min_image(zi - zj, g.plen[2], g.pinv[2]);
                inside += (dx * dx + dy * dy + dz * dz < rc2) ? 1ull : 0ull;
            }
        }
    }
    atomicAdd(&out[0], entries);   // one integer atomic per thread of a <=1024-block grid: exact, order-free
    atomicMax(&out[1], (unsigned long long)mx);
    atomicAdd(&out[2], inside);
}

}  // namespace emdee
