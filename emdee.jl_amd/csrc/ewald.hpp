// ewald.hpp -- the reciprocal-space part of the Ewald sum (emdee_md_set_ewald): a direct O(N K) sum over the wave vectors of
// topology.hpp ewald_vectors, exact to the chosen truncation.  All of it in fp64 whatever the engine's precision: a phase k.r
// reaches hundreds of radians, and the positions are converted when they are loaded.
//   1. k_ewald_phases: per atom and axis exp(i 2 pi n (x - lo) / L) for n = 0 .. kmax, by complex recurrence from one sincospi,
//      into planes in cell order (plane off[d] + n, pitch slots each).
//   2. k_ewald_sfac: S(k) = sum_j q_j exp(i k.r_j).  A workgroup takes a block of wave vectors and a chunk of atoms; a wavefront
//      keeps EW_KPW consecutive wave vectors in registers, its lanes walk the chunk's atoms, and one wave64 reduction per wave
//      vector (wave_ops.hpp) closes the chunk.  The partials [chunk][k] go to memory and k_ewald_sfac_sum adds them in chunk
//      order: no floating-point atomics, the same bits from run to run.
//   3. k_ewald_atoms: lanes are atoms, the loop runs over wave vectors whose coefficients and S(k) are wave-uniform reads; the
//      product of the x and y phase factors stays in registers while (n_x, n_y) stays the same (the list is sorted by them), the
//      z factor is one coalesced read.  The wave vectors are dealt to blockIdx.y in contiguous ranges so that a small box still
//      fills the device; k_ewald_add sums the ranges in order and adds the result, the self term and the neutralising
//      background to the cell-ordered arrays.  The forces-only instance computes the three force sums alone.
// The sums run over the half space of wave vectors; -k contributes the same to every one of them, hence the factors 2.
// The particle-mesh version (emdee_md_set_pme, pme.hpp) replaces kernels 1 to 3 behind EwaldRecip::run and hands k_ewald_add one
// range of the same layout.
#pragma once

#include "kernels.hpp"
#include "pme.hpp"
#include "topology.hpp"
#include "wave_ops.hpp"

namespace emdee {

constexpr int EW_BLOCK = 256;
constexpr int EW_KPW = 16;                                   // wave vectors a wavefront keeps in registers
constexpr int EW_KB = EW_KPW * (EW_BLOCK / WAVE);            // ... and a workgroup covers
constexpr int EW_CHUNK = 1024;                               // atoms per chunk of the structure-factor partials (at least)
constexpr int EW_MAX_SPLIT = 64;                             // ranges of wave vectors of the per-atom pass (at most)

struct EwaldAxes {
    double lo[3], inv[3];                                    // box origin, 1 / side
    int kmax[3], off[3];                                     // off[d]: the first phase plane of axis d
};

template <typename real>
__global__ void k_ewald_phases(int n, size_t pitch, AtomView<real> atoms, EwaldAxes ax, double2 *__restrict__ ph) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    real x, y, z, hs, te;
    load_atom(atoms, p, x, y, z, hs, te);
    const double r[3] = {(double)x, (double)y, (double)z};
#pragma unroll
    for (int d = 0; d < 3; d++) {
        double s1, c1;
        sincospi(2.0 * (r[d] - ax.lo[d]) * ax.inv[d], &s1, &c1);
        double c = 1.0, s = 0.0;
        for (int m = 0; m <= ax.kmax[d]; m++) {
            ph[(size_t)(ax.off[d] + m) * pitch + p] = make_double2(c, s);
            const double cn = c * c1 - s * s1;
            s = c * s1 + s * c1;
            c = cn;
        }
    }
}

// the phase factor of plane `plane0 + |m|` for atom p, conjugated for m < 0
__device__ __forceinline__ double2 ewald_phase(const double2 *__restrict__ ph, size_t pitch, int plane0, int m, int p) {
    double2 e = ph[(size_t)(plane0 + (m < 0 ? -m : m)) * pitch + p];
    if (m < 0) e.y = -e.y;
    return e;
}

template <typename real>
__global__ __launch_bounds__(EW_BLOCK) void k_ewald_sfac(int n, size_t pitch, int nk, int chunk_len, const topo::EwaldK *__restrict__ kt,
                                                         const double2 *__restrict__ ph, int offy, int offz,
                                                         const real *__restrict__ q, double2 *__restrict__ partial) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int k0 = blockIdx.x * EW_KB + wv * EW_KPW;
    if (k0 >= nk) return;                                    // (the whole wavefront; the kernel has no barrier)
    const int first = blockIdx.y * chunk_len, last = min(n, first + chunk_len);
    double re[EW_KPW], im[EW_KPW];
#pragma unroll
    for (int i = 0; i < EW_KPW; i++) re[i] = im[i] = 0.0;
    for (int base = first; base < last; base += WAVE) {
        const bool live = base + lane < last;
        const int p = live ? base + lane : first;
        const double qi = live ? (double)q[p] : 0.0;
        int pnx = -1, pny = 0;
        double cr = 0.0, ci = 0.0;                           // q_j exp(i (k_x x + k_y y))
#pragma unroll
        for (int i = 0; i < EW_KPW; i++) {
            if (k0 + i < nk) {
                const int nx = __builtin_amdgcn_readfirstlane(kt[k0 + i].nx), ny = __builtin_amdgcn_readfirstlane(kt[k0 + i].ny),
                          nz = __builtin_amdgcn_readfirstlane(kt[k0 + i].nz);
                if (nx != pnx || ny != pny) {
                    const double2 ex = ewald_phase(ph, pitch, 0, nx, p), ey = ewald_phase(ph, pitch, offy, ny, p);
                    cr = qi * (ex.x * ey.x - ex.y * ey.y);
                    ci = qi * (ex.x * ey.y + ex.y * ey.x);
                    pnx = nx; pny = ny;
                }
                const double2 ez = ewald_phase(ph, pitch, offz, nz, p);
                re[i] += cr * ez.x - ci * ez.y;
                im[i] += cr * ez.y + ci * ez.x;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < EW_KPW; i++) {
        const double r = wave_sum_to_lane63(re[i]), m = wave_sum_to_lane63(im[i]);
        if (lane == WAVE - 1 && k0 + i < nk) partial[(size_t)blockIdx.y * nk + k0 + i] = make_double2(r, m);
    }
}

static __global__ void k_ewald_sfac_sum(int nk, int nchunk, const double2 *__restrict__ partial, double2 *__restrict__ S) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nk) return;
    double r = 0.0, m = 0.0;
    for (int c = 0; c < nchunk; c++) {
        const double2 v = partial[(size_t)c * nk + k];
        r += v.x; m += v.y;
    }
    S[k] = make_double2(r, m);
}

// part: [range][component][slot] -- 3 force sums, and with ALL the energy sum and the six tensor sums (xx, yy, zz, xy, xz, yz)
template <bool ALL>
__global__ __launch_bounds__(EW_BLOCK) void k_ewald_atoms(int n, size_t pitch, int nk, int klen, const topo::EwaldK *__restrict__ kt,
                                                          const double2 *__restrict__ S, const double2 *__restrict__ ph, int offy,
                                                          int offz, double *__restrict__ part) {
    constexpr int NV = ALL ? 10 : 3;
    const int t = blockIdx.x * EW_BLOCK + threadIdx.x;
    const bool live = t < n;
    const int p = live ? t : 0;
    const int kbeg = blockIdx.y * klen, kend = min(nk, kbeg + klen);
    double fx = 0.0, fy = 0.0, fz = 0.0, se = 0.0;
    double tv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int pnx = -1, pny = 0;
    double cr = 0.0, ci = 0.0;
    for (int k = kbeg; k < kend; k++) {
        const topo::EwaldK kv = kt[k];                       // (wave-uniform address: scalar loads)
        const double2 s = S[k];
        const int nx = __builtin_amdgcn_readfirstlane(kv.nx), ny = __builtin_amdgcn_readfirstlane(kv.ny);
        if (nx != pnx || ny != pny) {
            const double2 ex = ewald_phase(ph, pitch, 0, nx, p), ey = ewald_phase(ph, pitch, offy, ny, p);
            cr = ex.x * ey.x - ex.y * ey.y;
            ci = ex.x * ey.y + ex.y * ey.x;
            pnx = nx; pny = ny;
        }
        const double2 ez = ewald_phase(ph, pitch, offz, kv.nz, p);
        const double c = cr * ez.x - ci * ez.y, sn = cr * ez.y + ci * ez.x;   // cos and sin of k.r_i
        const double t1 = kv.a * (sn * s.x - c * s.y);
        fx += t1 * kv.kx; fy += t1 * kv.ky; fz += t1 * kv.kz;
        if (ALL) {
            const double t2 = kv.a * (c * s.x + sn * s.y);
            se += t2;
            const double u = t2 * kv.b, ux = u * kv.kx, uy = u * kv.ky;
            tv[0] += ux * kv.kx; tv[1] += uy * kv.ky; tv[2] += u * kv.kz * kv.kz;
            tv[3] += ux * kv.ky; tv[4] += ux * kv.kz; tv[5] += uy * kv.kz;
        }
    }
    if (!live) return;
    double *out = part + (size_t)blockIdx.y * NV * pitch + p;
    out[0] = fx; out[pitch] = fy; out[2 * pitch] = fz;
    if (ALL) {
        out[3 * pitch] = se;
        for (int c = 0; c < 6; c++) out[(size_t)(4 + c) * pitch] = tv[c];
    }
}

// The ranges' sums in range order, times the atom's charge, plus the self term -K (alpha / sqrt(pi)) q_i^2 and the atom's share
// e_bg = E_n / N of the neutralising background (energy; xx, yy and zz of the tensor), ADDED to the cell-ordered arrays.
template <typename real, bool ALL>
__global__ void k_ewald_add(int n, size_t pitch, int nsplit, const double *__restrict__ part, const real *__restrict__ q, double self_c,
                            double e_bg, int bitmask, real *__restrict__ frc, real *__restrict__ en, real *__restrict__ vir,
                            real *__restrict__ vt) {
    constexpr int NV = ALL ? 10 : 3;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double v[NV];
#pragma unroll
    for (int c = 0; c < NV; c++) v[c] = 0.0;
    for (int r = 0; r < nsplit; r++)
#pragma unroll
        for (int c = 0; c < NV; c++) v[c] += part[((size_t)r * NV + c) * pitch + p];
    const double qi = (double)q[p];
    if (bitmask & EMDEE_FORCES) {
        frc[p] += (real)(2.0 * qi * v[0]); frc[pitch + p] += (real)(2.0 * qi * v[1]); frc[2 * pitch + p] += (real)(2.0 * qi * v[2]);
    }
    if (ALL) {
        const double se = qi * v[3];
        const double w[6] = {se - qi * v[4] + e_bg, se - qi * v[5] + e_bg, se - qi * v[6] + e_bg, -qi * v[7], -qi * v[8], -qi * v[9]};
        if (bitmask & EMDEE_ENERGIES) en[p] += (real)(se - self_c * qi * qi + e_bg);
        if (bitmask & EMDEE_VIRIALS) vir[p] += (real)(w[0] + w[1] + w[2]);
        if (bitmask & EMDEE_TENSOR)
            for (int c = 0; c < 6; c++) vt[c * pitch + p] += (real)w[c];
    }
}

// The reciprocal-space pass of one engine: its setting, its wave vectors and its device buffers.
template <typename real>
struct EwaldRecip {
    double alpha = 0.0;                                      // 0: off
    int32_t kmax[3] = {0, 0, 0};
    std::vector<int32_t> nvec;                               // topo::ewald_vectors(kmax)
    std::vector<topo::EwaldK> table;                         // ... and their coefficients for the box of table_len
    double table_len[3] = {-1.0, -1.0, -1.0}, table_alpha = 0.0;
    DevBuf<topo::EwaldK> ktab;
    DevBuf<double2> ph, S, partial;
    DevBuf<double> part;
    PmeRecip<real> pme;                                      // on: the mesh takes the place of the direct sum (emdee_md_set_pme)

    bool on() const { return alpha > 0.0; }
    void set(double a, const int32_t k[3]) {
        alpha = a;
        pme.clear();
        for (int d = 0; d < 3; d++) kmax[d] = k[d];
        nvec = topo::ewald_vectors(kmax);
        table_len[0] = -1.0;
    }
    void set_pme(double a, const int32_t grid[3], int32_t order) {
        alpha = a;
        pme.set(grid, order);
    }
    void clear() { alpha = 0.0; pme.clear(); }

    // adds the reciprocal-space terms of the n atoms (all owned) to the outputs `bitmask` names; q: sqrt(K) q per slot, q_sum
    // their sum, q_abs the sum of their magnitudes
    void run(hipStream_t s, int n, size_t pitch, const AtomView<real> &atoms, const double lo[3], const double len[3], const real *q,
             double q_sum, double q_abs, int bitmask, real *frc, real *en, real *vir, real *vt) {
        if (!on() || n == 0) return;
        const bool all = bitmask != EMDEE_FORCES;
        if (pme.on()) {
            part.ensure((size_t)(all ? 10 : 3) * pitch);
            pme.run(s, n, pitch, atoms, lo, len, alpha, q, q_abs, all, part.ptr);
            add(s, n, pitch, 1, len, q, q_sum, bitmask, frc, en, vir, vt);
            return;
        }
        const int nk = (int)(nvec.size() / 3);
        if (table_len[0] != len[0] || table_len[1] != len[1] || table_len[2] != len[2] || table_alpha != alpha) {
            EMDEE_HIP_CHECK(hipStreamSynchronize(s));        // (nothing in flight reads the table it replaces)
            table = topo::ewald_table(nvec, len, alpha);
            ktab.ensure(table.size() + 1);
            EMDEE_HIP_CHECK(hipMemcpyAsync(ktab.ptr, table.data(), table.size() * sizeof(topo::EwaldK), hipMemcpyHostToDevice, s));
            EMDEE_HIP_CHECK(hipStreamSynchronize(s));
            for (int d = 0; d < 3; d++) table_len[d] = len[d];
            table_alpha = alpha;
        }
        EwaldAxes ax{};
        int planes = 0;
        for (int d = 0; d < 3; d++) {
            ax.lo[d] = lo[d]; ax.inv[d] = 1.0 / len[d]; ax.kmax[d] = kmax[d]; ax.off[d] = planes;
            planes += kmax[d] + 1;
        }
        ph.ensure((size_t)planes * pitch);
        hipLaunchKernelGGL((k_ewald_phases<real>), dim3(blocks_for(n, 256)), dim3(256), 0, s, n, pitch, atoms, ax, ph.ptr);
        // chunks of atoms: EW_CHUNK each, longer where the partials would outgrow 2^25 entries (512 MiB)
        int chunk_len = EW_CHUNK;
        while ((size_t)((n + chunk_len - 1) / chunk_len) * nk > ((size_t)1 << 25)) chunk_len *= 2;
        const int nchunk = (n + chunk_len - 1) / chunk_len;
        partial.ensure((size_t)nchunk * nk);
        S.ensure((size_t)nk + 1);
        hipLaunchKernelGGL((k_ewald_sfac<real>), dim3(blocks_for(nk, EW_KB), nchunk), dim3(EW_BLOCK), 0, s, n, pitch, nk, chunk_len,
                           ktab.ptr, ph.ptr, ax.off[1], ax.off[2], q, partial.ptr);
        hipLaunchKernelGGL(k_ewald_sfac_sum, dim3(blocks_for(nk, 256)), dim3(256), 0, s, nk, nchunk, partial.ptr, S.ptr);
        // ranges of wave vectors: enough workgroups to fill the device, at least 256 wave vectors each
        const int ablocks = (int)blocks_for(n, EW_BLOCK);
        int nsplit = std::min(std::min(EW_MAX_SPLIT, (1024 + ablocks - 1) / ablocks), std::max(1, nk / 256));
        const int klen = (nk + nsplit - 1) / nsplit;
        nsplit = (nk + klen - 1) / klen;
        part.ensure((size_t)nsplit * (all ? 10 : 3) * pitch);
        with_bool(all, [&](auto a) {
            hipLaunchKernelGGL((k_ewald_atoms<decltype(a)::value>), dim3(ablocks, nsplit), dim3(EW_BLOCK), 0, s, n, pitch, nk, klen, ktab.ptr, S.ptr,
                               ph.ptr, ax.off[1], ax.off[2], part.ptr);
        });
        add(s, n, pitch, nsplit, len, q, q_sum, bitmask, frc, en, vir, vt);
    }

  private:
    // the tail the mesh and the direct sum share: the partials of nsplit ranges of wave vectors (the mesh: one), the self term
    // and the background, added to the outputs
    void add(hipStream_t s, int n, size_t pitch, int nsplit, const double len[3], const real *q, double q_sum, int bitmask, real *frc,
             real *en, real *vir, real *vt) {
        const double self_c = alpha / std::sqrt(M_PI);
        const double V = len[0] * len[1] * len[2], e_bg = -M_PI * q_sum * q_sum / (2.0 * V * alpha * alpha) / (double)n;
        with_bool(bitmask != EMDEE_FORCES, [&](auto all) {
            hipLaunchKernelGGL((k_ewald_add<real, decltype(all)::value>), dim3(blocks_for(n, 256)), dim3(256), 0, s, n, pitch, nsplit, part.ptr, q,
                               self_c, e_bg, bitmask, frc, en, vir, vt);
        });
    }
};

}  // namespace emdee
