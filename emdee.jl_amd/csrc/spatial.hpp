// spatial.hpp -- spatial profiles on the device (emdee_md_set_spatial, emdee_md_spatial_sample): per sample every grouped atom is put
// into a bin -- a planar slab normal to one axis, or a spherical shell around a centre -- and ten fp64 words per (group, bin) take its
// mass and charge, its momentum and kinetic terms, and its energy and virial tensor of the tensor pass.  The table order is msd.hpp's
// (group-major, ascending caller id, chunks of 1024 entries of one group, group_layout.hpp): a rebuild of the neighbour list re-sorts
// the engine's records and changes no bit of a sum.  Three launches: (1) the gather, one thread per slot, writes the bin and the
// masked addends as fp64 planes in table order; (2) one workgroup per chunk sorts bin * 1024 + local index in LDS (unique keys: the
// bitonic network is deterministic), the head of every run of equal bins sums that run in index order and leaves (bin, length,
// words) at its sorted position; (3) one thread per (group, bin) walks its group's chunks in chunk order, finds its run in each by
// binary search and adds the total to the sums and the counts with plain stores.  No floating-point atomics, no integer ones either.
// The parts with no HIP in them -- the bin rules, an atom's ten addends, the run sums of a chunk and the finish -- are plain C++ at
// the top, as the top of msd.hpp is: a stand-alone host program tests them with the host compiler (tests/c/spatial_host.cpp); the
// kernels below them need HIP.  DESIGN.md 4i-2 has the algorithm; MdImpl::spatial_sample (impl.hpp) queues a sample.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "group_layout.hpp"

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int SPATIAL_WORDS = 10;                            // (EMDEE_SPATIAL_WORDS)
constexpr int SPATIAL_MAX_BINS = 4096, SPATIAL_MAX_GROUPS = MSD_MAX_GROUPS;
constexpr int SPATIAL_DENSITY = 1, SPATIAL_KINETIC = 2, SPATIAL_STRESS = 4, SPATIAL_ALL = 7;
constexpr int SPATIAL_X = 0, SPATIAL_Y = 1, SPATIAL_Z = 2, SPATIAL_RADIAL = 3;
constexpr int SPATIAL_CHUNK = MSD_CHUNK;
constexpr int SPATIAL_SHIFT = 10;                            // a sort key is bin << SPATIAL_SHIFT | local index
static_assert(SPATIAL_CHUNK == 1 << SPATIAL_SHIFT, "a sort key holds the local index in its low bits");
constexpr int SPATIAL_OUT = SPATIAL_MAX_BINS;                // the bin of an atom outside the range, in a sort key
constexpr int SPATIAL_PAD = SPATIAL_MAX_BINS + 1;            // ... of an entry beyond the chunk's count

// ---- the words of a mask, compacted: DENSITY 0-1, KINETIC 2-6, STRESS 7-9
EMDEE_HD constexpr int spatial_n_words(int what) {
    return ((what & SPATIAL_DENSITY) ? 2 : 0) + ((what & SPATIAL_KINETIC) ? 5 : 0) + ((what & SPATIAL_STRESS) ? 3 : 0);
}
// the word behind compact index j < spatial_n_words(what)
EMDEE_HD constexpr int spatial_word_of(int what, int j) {
    if (what & SPATIAL_DENSITY) {
        if (j < 2) return j;
        j -= 2;
    }
    if (what & SPATIAL_KINETIC) {
        if (j < 5) return 2 + j;
        j -= 5;
    }
    return 7 + j;
}

// ---- the geometry of one sample, by value: formed on the host, in double, from the box of that sample
struct SpatialGeom {
    int geometry, n_bins, periodic;                          // periodic: the planar axis is
    double lo, inv_width;                                    // planar: lo_d (or r0) and n_bins / len_d (or n_bins / (r1 - r0))
    double cx, cy, cz;                                       // radial: the fixed centre
    double len[3], inv_len[3];                               // radial: the box lengths and 1 / them; 0 on an open axis (no image)
    double r_max, inv_dr;                                    // radial: n_bins / r_max
};

// ---- the bin rules: the same integer from the same doubles on the host and on the device.  Every difference and every product is
// a rounding of its own -- no fused multiply-add -- then floor (sqrt and a truncation in the radial rule).
// A product that no compiler fuses with the sum it feeds: on the device the instruction itself (the library is built with
// -ffp-contract=fast, which passes over the pragma), on the host the pragma (clang) or a target without fused multiply-add.
EMDEE_HD double spatial_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double r = a * b;
    return r;
#endif
}
// planar: floor((x - lo) * inv_width), wrapped into 0 ... n_bins - 1 on a periodic axis; -1 outside [0, n_bins) on an open one
EMDEE_HD int spatial_bin_planar(double x, double lo, double inv_width, int n_bins, int periodic) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = x - lo;
    const double s = spatial_mul(d, inv_width);
    const double f = floor(s);
    if (!(f > -9.0e15 && f < 9.0e15)) return -1;              // (not a number, or beyond what a 64-bit integer wraps exactly)
    if (periodic) {
        const long long i = (long long)f;
        long long k = i % n_bins;
        if (k < 0) k += n_bins;
        return (int)k;
    }
    return (f >= 0.0 && f < (double)n_bins) ? (int)f : -1;
}
// one minimum-image difference: x - c, less the nearest whole number of box lengths on a periodic axis (inv_len != 0)
EMDEE_HD double spatial_image(double x, double c, double len, double inv_len) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double d = x - c;
    if (inv_len != 0.0) {
        const double q = spatial_mul(d, inv_len);
        const double n = rint(q);
        const double s = spatial_mul(n, len);
        d = d - s;
    }
    return d;
}
// radial: d = the minimum-image vector from the centre, r = |d|; the shell (int)(r * inv_dr), -1 for r >= r_max
EMDEE_HD int spatial_bin_radial(const double d[3], double r_max, double inv_dr, int n_bins, double &r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p0 = spatial_mul(d[0], d[0]), p1 = spatial_mul(d[1], d[1]), p2 = spatial_mul(d[2], d[2]);
    const double s01 = p0 + p1;
    const double r2 = s01 + p2;
    r = sqrt(r2);
    if (!(r < r_max)) return -1;
    const double s = spatial_mul(r, inv_dr);
    const int k = (int)s;
    return k < n_bins ? k : -1;
}

// ---- an atom's ten addends.  m: its mass (0 for a massless atom), q: its charge, v: its velocity, e and w: its energy and tensor
// (xx, yy, zz, xy, xz, yz) of the tensor pass, n: the unit normal; no_normal: the atom sits on the centre of the radial geometry,
// where words 6 and 9 take a third of words 5 and 8.  A bit of `what` that is off leaves its words 0.
EMDEE_HD void spatial_addends(int what, double m, double q, const double v[3], double e, const double w[6], const double n[3],
                              bool no_normal, double out[SPATIAL_WORDS]) {
    for (int k = 0; k < SPATIAL_WORDS; k++) out[k] = 0.0;
    if (what & SPATIAL_DENSITY) {
        out[0] = m;
        out[1] = q;
    }
    if (what & SPATIAL_KINETIC) {
        out[2] = m * v[0]; out[3] = m * v[1]; out[4] = m * v[2];
        out[5] = m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double vn = v[0] * n[0] + v[1] * n[1] + v[2] * n[2];
        out[6] = no_normal ? out[5] / 3.0 : m * (vn * vn);
    }
    if (what & SPATIAL_STRESS) {
        out[7] = e;
        out[8] = w[0] + w[1] + w[2];
        const double nn = n[0] * n[0] * w[0] + n[1] * n[1] * w[1] + n[2] * n[2] * w[2] +
                          2.0 * (n[0] * n[1] * w[3] + n[0] * n[2] * w[4] + n[1] * n[2] * w[5]);
        out[9] = no_normal ? out[8] / 3.0 : nn;
    }
}

// ---- the runs of a chunk and the finish.  sorted: the chunk's SPATIAL_CHUNK keys, ascending.
EMDEE_HD int spatial_key(int bin, int count, int i) {
    const int b = i >= count ? SPATIAL_PAD : (bin < 0 ? SPATIAL_OUT : bin);
    return (b << SPATIAL_SHIFT) | i;
}
// position i heads a run: the bin of its key differs from the one before it
EMDEE_HD bool spatial_is_head(const int *sorted, int i) {
    return i == 0 || (sorted[i] >> SPATIAL_SHIFT) != (sorted[i - 1] >> SPATIAL_SHIFT);
}
// the run that starts at sorted position i: its length, and its NW words summed in index order from planes (word j of local
// entry e at planes[j * pitch + e]); an outside run has a length only
template <int NW>
EMDEE_HD int spatial_run_sum(const int *sorted, int i, const double *planes, size_t pitch, double acc[NW > 0 ? NW : 1]) {
    const int b = sorted[i] >> SPATIAL_SHIFT;
    for (int j = 0; j < NW; j++) acc[j] = 0.0;
    int n = 0;
    for (int at = i; at < SPATIAL_CHUNK && (sorted[at] >> SPATIAL_SHIFT) == b; at++, n++) {
        if (b >= SPATIAL_OUT) continue;
        const int e = sorted[at] & (SPATIAL_CHUNK - 1);
        for (int j = 0; j < NW; j++) acc[j] += planes[j * pitch + e];
    }
    return n;
}
// where the run of `bin` starts among a chunk's sorted bins (ascending), or -1
EMDEE_HD int spatial_find_run(const int *sbin, int bin) {
    int lo = 0, hi = SPATIAL_CHUNK;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sbin[mid] < bin) lo = mid + 1; else hi = mid;
    }
    return (lo < SPATIAL_CHUNK && sbin[lo] == bin) ? lo : -1;
}
// the total of `bin` over chunks c0 ... c1 - 1, in chunk order: NW words and the count
template <int NW>
EMDEE_HD long long spatial_bin_total(int c0, int c1, int bin, const int *sbin, const int *runn, const double *runw, double tot[NW > 0 ? NW : 1]) {
    for (int j = 0; j < NW; j++) tot[j] = 0.0;
    long long cnt = 0;
    for (int c = c0; c < c1; c++) {
        const int i = spatial_find_run(sbin + (size_t)c * SPATIAL_CHUNK, bin);
        if (i < 0) continue;
        const size_t at = (size_t)c * SPATIAL_CHUNK + i;
        cnt += runn[at];
        for (int j = 0; j < NW; j++) tot[j] += runw[at * NW + j];
    }
    return cnt;
}

// ---- the host's mirror of launches (2) and (3), for the stand-alone test: bins and planes in table order (plane j of entry e at
// planes[j * n_grouped + e]), the table's chunks; adds into sums[(g n_bins + k) NW + j], counts[g n_bins + k] and outside[g]
template <int NW>
inline void spatial_reduce_host(const MsdLayout &lay, int n_groups, int n_bins, const int *bin, const double *planes, double *sums,
                                long long *counts, long long *outside) {
    const size_t nc = lay.chunks.size(), ng = (size_t)lay.n_grouped;
    std::vector<int> sbin(nc * SPATIAL_CHUNK), runn(nc * SPATIAL_CHUNK, 0), key(SPATIAL_CHUNK);
    std::vector<double> runw(nc * SPATIAL_CHUNK * (NW > 0 ? NW : 1), 0.0);
    for (size_t c = 0; c < nc; c++) {
        const MsdChunk ch = lay.chunks[c];
        for (int i = 0; i < SPATIAL_CHUNK; i++) key[(size_t)i] = spatial_key(i < ch.count ? bin[ch.first + i] : 0, ch.count, i);
        std::sort(key.begin(), key.end());
        for (int i = 0; i < SPATIAL_CHUNK; i++) {
            const size_t at = c * SPATIAL_CHUNK + i;
            sbin[at] = key[(size_t)i] >> SPATIAL_SHIFT;
            if (!spatial_is_head(key.data(), i) || sbin[at] >= SPATIAL_PAD) continue;
            double acc[NW > 0 ? NW : 1];
            runn[at] = spatial_run_sum<NW>(key.data(), i, planes + ch.first, ng, acc);
            for (int j = 0; j < NW; j++) runw[at * NW + j] = acc[j];
        }
    }
    for (int g = 0; g < n_groups; g++)
        for (int k = 0; k <= n_bins; k++) {
            double tot[NW > 0 ? NW : 1];
            const long long cnt = spatial_bin_total<NW>(lay.chunk_of_group[g], lay.chunk_of_group[g + 1], k < n_bins ? k : SPATIAL_OUT,
                                                        sbin.data(), runn.data(), runw.data(), tot);
            if (k == n_bins) { outside[g] += cnt; continue; }
            counts[(size_t)g * n_bins + k] += cnt;
            for (int j = 0; j < NW; j++) sums[((size_t)g * n_bins + k) * NW + j] += tot[j];
        }
}

}  // namespace emdee

#if defined(__HIPCC__)

#include "kernels.hpp"
#include "pull.hpp"

namespace emdee {

constexpr int SPATIAL_BLOCK = 256, SPATIAL_PER_THREAD = SPATIAL_CHUNK / SPATIAL_BLOCK;

// what the gather reads of the engine: the records and their images (k_msd_gather's unwrapped coordinates), the velocities, the
// inverse masses (NULL: every mass 1), the energies and tensors of the tensor pass, the caller's charges by caller id (NULL: no
// charges)
template <typename real>
struct SpatialSrc {
    int n, n_owned;
    GridP<real> g;
    const int *img, *perm;
    const Rec<real> *rec;
    RelGrid rel;
    const real *vel, *inv_mass, *en, *vt;
    size_t pitch;
    const double *q_raw;
    long long q_n;
};

// (1) One thread per slot p of the engine's order: the unwrapped coordinates by k_msd_gather's expression, the bin to key[e], the
// masked addends to planes[j][e], e = pos_of[id] the entry of the table order.  centre_dev: the centre of mass of the centre group,
// formed by the two launches ahead of this one (NULL: the fixed centre of the geometry).
template <typename real, int MASK>
__global__ __launch_bounds__(256) void k_spatial_gather(SpatialSrc<real> a, SpatialGeom sg, const double *__restrict__ centre_dev,
                                                        const int *__restrict__ pos_of, int n_grouped, int *__restrict__ key,
                                                        double *__restrict__ planes) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const int id = a.perm[p];
    if (id < 0 || id >= a.n_owned) return;
    const int e = pos_of[id];
    if (e < 0 || e >= n_grouped) return;
    const Rec<real> r = a.rec[p];
    int kx, ky, kz;
    img_unpack(a.img[p], kx, ky, kz);
    double x, y, z;
    if (sizeof(real) == 4) {
        x = (double)r.x; y = (double)r.y; z = (double)r.z;
        if (a.rel.on) {
            double ox, oy, oz;
            a.rel.origin(a.rel.cell[p], ox, oy, oz);
            x += ox; y += oy; z += oz;
        }
        x += (double)kx * (double)a.g.len[0];
        y += (double)ky * (double)a.g.len[1];
        z += (double)kz * (double)a.g.len[2];
    } else {
        x = r.x + (real)kx * a.g.len[0];
        y = r.y + (real)ky * a.g.len[1];
        z = r.z + (real)kz * a.g.len[2];
    }
    double n[3] = {0.0, 0.0, 0.0};
    bool no_normal = false;
    int bin;
    if (sg.geometry == SPATIAL_RADIAL) {
        const double cx = centre_dev ? centre_dev[0] : sg.cx, cy = centre_dev ? centre_dev[1] : sg.cy, cz = centre_dev ? centre_dev[2] : sg.cz;
        double d[3], rr;
        d[0] = spatial_image(x, cx, sg.len[0], sg.inv_len[0]);
        d[1] = spatial_image(y, cy, sg.len[1], sg.inv_len[1]);
        d[2] = spatial_image(z, cz, sg.len[2], sg.inv_len[2]);
        bin = spatial_bin_radial(d, sg.r_max, sg.inv_dr, sg.n_bins, rr);
        no_normal = !(rr > 0.0);
        if (!no_normal) { n[0] = d[0] / rr; n[1] = d[1] / rr; n[2] = d[2] / rr; }
    } else {
        const double c = sg.geometry == SPATIAL_X ? x : (sg.geometry == SPATIAL_Y ? y : z);
        bin = spatial_bin_planar(c, sg.lo, sg.inv_width, sg.n_bins, sg.periodic);
        n[0] = sg.geometry == SPATIAL_X ? 1.0 : 0.0; n[1] = sg.geometry == SPATIAL_Y ? 1.0 : 0.0; n[2] = sg.geometry == SPATIAL_Z ? 1.0 : 0.0;
    }
    key[e] = bin;
    if (bin < 0) return;                                     // (an atom outside the range adds to `outside` and nothing else)
    double m = 0.0, q = 0.0, v[3] = {0.0, 0.0, 0.0}, en = 0.0, w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (MASK & (SPATIAL_DENSITY | SPATIAL_KINETIC)) {
        const real im = a.inv_mass ? a.inv_mass[p] : (real)1;
        m = im != (real)0 ? 1.0 / (double)im : 0.0;          // (a massless atom, a virtual site: exactly 0)
    }
    if ((MASK & SPATIAL_DENSITY) && a.q_raw && id < a.q_n) q = a.q_raw[id];
    if ((MASK & SPATIAL_KINETIC) && a.vel) {
        v[0] = (double)a.vel[p]; v[1] = (double)a.vel[a.pitch + p]; v[2] = (double)a.vel[2 * a.pitch + p];
    }
    if (MASK & SPATIAL_STRESS) {
        en = (double)a.en[p];
#pragma unroll
        for (int c = 0; c < 6; c++) w[c] = (double)a.vt[c * a.pitch + p];
    }
    double out[SPATIAL_WORDS];
    spatial_addends(MASK, m, q, v, en, w, n, no_normal, out);
    constexpr int NW = spatial_n_words(MASK);
#pragma unroll
    for (int j = 0; j < NW; j++) planes[(size_t)j * n_grouped + e] = out[spatial_word_of(MASK, j)];
}

// The centre of mass of the centre group, in an order a host can repeat bit for bit from emdee_md_get_state's coordinates.  One
// workgroup per chunk of the group: the products m x, m y, m z -- each a rounding of its own (spatial_mul) -- and m of the chunk's
// entries, zeros beyond its count, go through a halving tree in LDS (s[i] += s[i + h], h = 512 ... 1) into partial[chunk][0..3].
// atoms: one caller id per entry of the table order.
template <typename real>
__global__ __launch_bounds__(SPATIAL_BLOCK) void k_spatial_centre_partials(RestraintArgs<real> a, const real *__restrict__ inv_mass,
                                                                           const MsdChunk *__restrict__ chunks, double *__restrict__ partial) {
    __shared__ double s[SPATIAL_CHUNK];
    const MsdChunk ch = chunks[blockIdx.x];
    const int t = threadIdx.x;
    double x[SPATIAL_PER_THREAD][3], m[SPATIAL_PER_THREAD];
#pragma unroll
    for (int k = 0; k < SPATIAL_PER_THREAD; k++) {
        const int e = t + k * SPATIAL_BLOCK;
        x[k][0] = x[k][1] = x[k][2] = m[k] = 0.0;
        if (e >= ch.count || ch.first + e >= a.n) continue;
        const int p = restraint_slot(a, ch.first + e);
        if (p < 0) continue;
        restraint_unwrapped(a, p, x[k]);
        m[k] = pull_mass(inv_mass, p);
    }
#pragma unroll
    for (int w = 0; w < 4; w++) {
#pragma unroll
        for (int k = 0; k < SPATIAL_PER_THREAD; k++) s[t + k * SPATIAL_BLOCK] = w < 3 ? spatial_mul(m[k], x[k][w]) : m[k];
        __syncthreads();
        for (int h = SPATIAL_CHUNK / 2; h >= 1; h >>= 1) {
            for (int i = t; i < h; i += SPATIAL_BLOCK) s[i] = s[i] + s[i + h];
            __syncthreads();
        }
        if (t == 0) partial[4 * (size_t)blockIdx.x + w] = s[0];
        __syncthreads();
    }
}
// ... then one thread adds the chunks' partials in chunk order: out[0..2] = R = (sum m x) / M, out[3] = M
static __global__ void k_spatial_centre(int n_chunks, const double *__restrict__ partial, double *__restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < n_chunks; c++)
#pragma unroll
        for (int w = 0; w < 4; w++) tot[w] = tot[w] + partial[4 * (size_t)c + w];
#pragma unroll
    for (int d = 0; d < 3; d++) out[d] = tot[3] > 0.0 ? tot[d] / tot[3] : 0.0;
    out[3] = tot[3];
}

// (2) One workgroup per chunk.  The chunk's keys -- bin << 10 | local index, unique -- are sorted in LDS by a bitonic network (55
// rounds of 512 compare-exchanges, two per thread); every position writes its bin to sbin[chunk][position], and the thread at the
// head of a run of equal bins sums the run in index order (spatial_run_sum) and writes its length and words to that position.
template <int MASK>
__global__ __launch_bounds__(SPATIAL_BLOCK) void k_spatial_accumulate(const MsdChunk *__restrict__ chunks, const int *__restrict__ key,
                                                                      const double *__restrict__ planes, size_t n_grouped,
                                                                      int *__restrict__ sbin, int *__restrict__ runn, double *__restrict__ runw) {
    __shared__ int s[SPATIAL_CHUNK];
    constexpr int NW = spatial_n_words(MASK);
    const MsdChunk ch = chunks[blockIdx.x];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < SPATIAL_PER_THREAD; k++) {
        const int i = t + k * SPATIAL_BLOCK;
        s[i] = spatial_key(i < ch.count ? key[ch.first + i] : 0, ch.count, i);
    }
    __syncthreads();
    for (int size = 2; size <= SPATIAL_CHUNK; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
            for (int k = 0; k < SPATIAL_CHUNK / 2 / SPATIAL_BLOCK; k++) {
                const int j = t + k * SPATIAL_BLOCK;
                const int i = ((j & ~(stride - 1)) << 1) | (j & (stride - 1)), o = i + stride;
                const int a = s[i], b = s[o];
                const bool up = (i & size) == 0;
                if ((a > b) == up) { s[i] = b; s[o] = a; }
            }
            __syncthreads();
        }
    const size_t base = (size_t)blockIdx.x * SPATIAL_CHUNK;
#pragma unroll
    for (int k = 0; k < SPATIAL_PER_THREAD; k++) {
        const int i = t + k * SPATIAL_BLOCK;
        const int b = s[i] >> SPATIAL_SHIFT;
        sbin[base + i] = b;
        if (b >= SPATIAL_PAD || !spatial_is_head(s, i)) continue;
        double acc[NW];
        runn[base + i] = spatial_run_sum<NW>(s, i, planes + ch.first, n_grouped, acc);
#pragma unroll
        for (int j = 0; j < NW; j++) runw[(base + i) * NW + j] = acc[j];
    }
}

// (3) One thread per (group blockIdx.y, bin k); thread k == n_bins takes the atoms outside the range.  The group's chunks in chunk
// order (spatial_bin_total), then plain read-modify-writes: a thread owns its words, and the samples follow one another on the stream.
template <int MASK>
__global__ __launch_bounds__(SPATIAL_BLOCK) void k_spatial_finish(int n_bins, const int *__restrict__ chunk_of_group, const int *__restrict__ sbin,
                                                                  const int *__restrict__ runn, const double *__restrict__ runw,
                                                                  double *__restrict__ sums, unsigned long long *__restrict__ counts,
                                                                  unsigned long long *__restrict__ outside) {
    constexpr int NW = spatial_n_words(MASK);
    const int k = blockIdx.x * SPATIAL_BLOCK + threadIdx.x, g = blockIdx.y;
    if (k > n_bins) return;
    double tot[NW];
    const long long cnt = spatial_bin_total<NW>(chunk_of_group[g], chunk_of_group[g + 1], k < n_bins ? k : SPATIAL_OUT, sbin, runn, runw, tot);
    if (k == n_bins) {
        outside[g] += (unsigned long long)cnt;
        return;
    }
    const size_t at = (size_t)g * n_bins + k;
    counts[at] += (unsigned long long)cnt;
#pragma unroll
    for (int j = 0; j < NW; j++) sums[at * SPATIAL_WORDS + spatial_word_of(MASK, j)] += tot[j];
}

}  // namespace emdee
#endif
