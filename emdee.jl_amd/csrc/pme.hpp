// pme.hpp -- the mesh form of the reciprocal-space part of the Ewald sum (emdee_md_set_pme): smooth particle-mesh Ewald, Essmann
// et al., J. Chem. Phys. 103, 8577 (1995), on an orthorhombic box.  It takes the place of the direct sum's kernels 1 to 3 of
// ewald.hpp (EwaldRecip::run: no phase table is built) and ends in the same k_ewald_add.  All of it in fp64 whatever the
// engine's precision.
// Mesh K = grid, point (m_x, m_y, m_z) at index (m_x K_y + m_y) K_z + m_z; scaled coordinate u_d = K_d (x_d - lo_d) / L_d,
// f = floor(u), t = u - f: the atom touches the p points m_d = (f_d - j) mod K_d, j = 0 .. p - 1, with weight M_p(t + j).
//   1. k_pme_spread: one wavefront per atom, lanes are stencil points (order 4: 4 x 4 x 4 = one wave64; order 6: 216 points in
//      four rounds).  Q is summed in 64-bit FIXED POINT with integer atomic adds: integer addition is associative, so the
//      mesh has the same bits whatever order the adds arrive in -- no floating-point atomics.  The scale 2^shift comes from
//      the host (topology.hpp pme_fixed_shift: no mesh point can overflow).  The rate of 64-bit integer atomics on this chip
//      has not been measured by anybody here; profiles/pme_cost.py times the pass as a whole.  k_pme_convert turns the
//      integers into the complex mesh.
//   2. k_pme_fft: one axis of the 3-D complex transform.  A workgroup holds FFT_TILE points = FFT_TILE / K whole lines in LDS
//      (line pitch K + 1 elements, so that the strided fill of the x and y passes does not land on one bank), Stockham
//      radix-2 with the operands staged in registers between two barriers, twiddles from the host table.  The x and y passes
//      take lines that are neighbours in memory, so a wavefront's global access is runs of lines x 16 bytes (at least 128).
//      The inverse conjugates the twiddles and is unnormalised.
//   3. k_pme_spectrum: W = A(k) |b(m)|^2 (x 2 k_a k_b (1 / k^2 + 1 / 4 alpha^2) for a tensor component) F Q, from the kept
//      spectrum into the work mesh, which the inverse transform turns into phi (or phi'_ab) in place.
//   4. k_pme_gather: the stencil mapping of the spreading; per atom sum_m theta phi (and sum_m grad theta phi), lanes first
//      in round order, then one wave64 reduction (wave_ops.hpp): a fixed order.  It writes the `part` layout of ewald.hpp with
//      one range, scaled so that k_ewald_add adds charge, self term and background exactly as it does for the direct sum:
//      v[0..2] = -1/2 sum grad theta phi, v[3] = 1/2 sum theta phi, v[4 + c] = 1/2 sum theta phi'_c with
//      phi'_ab = F^-1[A |b|^2 2 k_a k_b (1 / k^2 + 1 / 4 alpha^2) F Q]  (phi_ab of the header = delta_ab phi - phi'_ab).
// Two complex meshes: the spectrum, and the work mesh, which is the fixed-point mesh first.
#pragma once

#include "kernels.hpp"
#include "topology.hpp"
#include "wave_ops.hpp"

namespace emdee {

constexpr int PME_BLOCK = 256;
constexpr int FFT_TILE_LOG2 = 11, FFT_TILE = 1 << FFT_TILE_LOG2;    // points of a workgroup's LDS tile
constexpr int FFT_MAXLINES = FFT_TILE / 8;                   // ... of the shortest axis

struct PmeMesh {
    double lo[3], inv[3];                                    // box origin, 1 / side
    int K[3];
};

// One axis of an atom's stencil: f = floor(u) and, for the points f - j, j = 0 .. P - 1, w_j = M_P(u - f + j) and d_j, its
// derivative by the POSITION.  Named scalars, not arrays: a lane picks its own j with selects, and nothing goes to scratch.
struct PmeAxis {
    double w0, w1, w2, w3, w4, w5, d0, d1, d2, d3, d4, d5;
    int f;
};
// order N - 1 -> N of topology.hpp pme_bspline: a_j = ((t + j) a_j + (N - t - j) a_{j-1}) / (N - 1), descending j
template <int N>
__device__ __forceinline__ void pme_raise(double t, PmeAxis &a) {
    constexpr double r = 1.0 / (double)(N - 1);
    if (N > 5) a.w5 = ((t + 5.0) * a.w5 + ((double)N - t - 5.0) * a.w4) * r;
    if (N > 4) a.w4 = ((t + 4.0) * a.w4 + ((double)N - t - 4.0) * a.w3) * r;
    if (N > 3) a.w3 = ((t + 3.0) * a.w3 + ((double)N - t - 3.0) * a.w2) * r;
    a.w2 = ((t + 2.0) * a.w2 + ((double)N - t - 2.0) * a.w1) * r;
    a.w1 = ((t + 1.0) * a.w1 + ((double)N - t - 1.0) * a.w0) * r;
    a.w0 = t * a.w0 * r;
}
template <int P>
__device__ __forceinline__ PmeAxis pme_axis(double x, double lo, double inv, int K) {
    static_assert(P == 4 || P == 6, "orders 4 and 6");
    PmeAxis a;
    const double u = (x - lo) * inv * (double)K, fl = floor(u), t = u - fl;
    a.f = (int)fl;
    a.w0 = t; a.w1 = 1.0 - t; a.w2 = a.w3 = a.w4 = a.w5 = 0.0;
    pme_raise<3>(t, a);
    if (P == 6) { pme_raise<4>(t, a); pme_raise<5>(t, a); }
    const double c = (double)K * inv;                        // M_P'(x) = M_{P-1}(x) - M_{P-1}(x - 1), and du/dx
    a.d0 = c * a.w0; a.d1 = c * (a.w1 - a.w0); a.d2 = c * (a.w2 - a.w1); a.d3 = c * (a.w3 - a.w2); a.d4 = c * (a.w4 - a.w3);
    a.d5 = c * (a.w5 - a.w4);
    pme_raise<P>(t, a);
    return a;
}
__device__ __forceinline__ double pme_pick(int j, double v0, double v1, double v2, double v3, double v4, double v5) {
    double v = v0;
    v = j == 1 ? v1 : v; v = j == 2 ? v2 : v; v = j == 3 ? v3 : v; v = j == 4 ? v4 : v; v = j == 5 ? v5 : v;
    return v;
}
__device__ __forceinline__ double pme_w(const PmeAxis &a, int j) { return pme_pick(j, a.w0, a.w1, a.w2, a.w3, a.w4, a.w5); }
__device__ __forceinline__ double pme_d(const PmeAxis &a, int j) { return pme_pick(j, a.d0, a.d1, a.d2, a.d3, a.d4, a.d5); }
// the stencil point s (0 .. P^3 - 1): its mesh index, its weight theta_x theta_y theta_z and, with GRAD, the gradient of the weight
template <int P, bool GRAD>
__device__ __forceinline__ size_t pme_point(int s, const PmeMesh &g, const PmeAxis &ax, const PmeAxis &ay, const PmeAxis &az, double &th,
                                            double &gx, double &gy, double &gz) {
    const int jx = s / (P * P), jy = (s / P) % P, jz = s % P;
    const int mx = (ax.f - jx) & (g.K[0] - 1), my = (ay.f - jy) & (g.K[1] - 1), mz = (az.f - jz) & (g.K[2] - 1);
    const double wx = pme_w(ax, jx), wy = pme_w(ay, jy), wz = pme_w(az, jz);
    th = wx * wy * wz;
    if (GRAD) {
        gx = pme_d(ax, jx) * wy * wz;
        gy = wx * pme_d(ay, jy) * wz;
        gz = wx * wy * pme_d(az, jz);
    }
    return ((size_t)mx * g.K[1] + my) * g.K[2] + mz;
}

template <typename real, int P>
__global__ __launch_bounds__(PME_BLOCK) void k_pme_spread(int n, AtomView<real> atoms, PmeMesh g, const real *__restrict__ q, double scale,
                                                          unsigned long long *__restrict__ Qi) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int p = blockIdx.x * (PME_BLOCK / WAVE) + threadIdx.x / WAVE;
    if (p >= n) return;                                      // (the whole wavefront; the kernel has no barrier)
    const double qs = (double)q[p] * scale;
    if (qs == 0.0) return;
    real x, y, z, hs, te;
    load_atom(atoms, p, x, y, z, hs, te);
    const PmeAxis ax = pme_axis<P>((double)x, g.lo[0], g.inv[0], g.K[0]), ay = pme_axis<P>((double)y, g.lo[1], g.inv[1], g.K[1]),
                     az = pme_axis<P>((double)z, g.lo[2], g.inv[2], g.K[2]);
#pragma unroll
    for (int s = lane; s < P * P * P; s += WAVE) {
        double th, gx, gy, gz;
        const size_t m = pme_point<P, false>(s, g, ax, ay, az, th, gx, gy, gz);
        atomicAdd(Qi + m, (unsigned long long)__double2ll_rn(qs * th));
    }
}

static __global__ void k_pme_convert(size_t total, const long long *__restrict__ Qi, double inv_scale, double2 *__restrict__ S) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    S[i] = make_double2((double)Qi[i] * inv_scale, 0.0);
}

// One axis of the transform, in place.  K points per line at stride `stride`; line l starts at (l / inner) * outer + l % inner,
// inner a power of two (z: inner 1, outer K_z; y: inner K_z, outer K_y K_z; x: inner K_y K_z, outer 0).  tw: exp(-2 pi i j / K), j < K / 2.
template <bool INVERSE, bool CONTIGUOUS>
__global__ __launch_bounds__(PME_BLOCK) void k_pme_fft(int K, int log2K, size_t nlines, size_t stride, int inner_log2, size_t outer,
                                                       const double2 *__restrict__ tw, double2 *__restrict__ mesh) {
    __shared__ double2 tile[FFT_TILE + FFT_MAXLINES];
    const int lines = FFT_TILE >> log2K, pitch = K + 1, lines_log2 = FFT_TILE_LOG2 - log2K;
    const size_t first = (size_t)blockIdx.x * lines;
    const int live = (int)min((size_t)lines, nlines - first);
    const int t = threadIdx.x;
    for (int i = t; i < FFT_TILE; i += PME_BLOCK) {
        const int ln = CONTIGUOUS ? (i >> log2K) : (i & (lines - 1));
        const int pos = CONTIGUOUS ? (i & (K - 1)) : (i >> lines_log2);
        if (ln < live) {
            const size_t l = first + ln;
            tile[ln * pitch + pos] = mesh[(l >> inner_log2) * outer + (l & (((size_t)1 << inner_log2) - 1)) + (size_t)pos * stride];
        }
    }
    __syncthreads();
    const int half = K >> 1;
    constexpr int PER = FFT_TILE / 2 / PME_BLOCK;            // butterflies per thread and stage
    for (int ns = 1, shift = log2K - 1; ns < K; ns <<= 1, shift--) {
        double2 a[PER], b[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int bf = t + i * PME_BLOCK;
            const int ln = bf >> (log2K - 1), j = bf & (half - 1);
            a[i] = tile[ln * pitch + j];
            const double2 x = tile[ln * pitch + j + half];
            double2 w = tw[(j & (ns - 1)) << shift];         // exp(-2 pi i k / (2 ns)), k = j mod ns
            if (INVERSE) w.y = -w.y;
            b[i] = make_double2(x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int bf = t + i * PME_BLOCK;
            const int ln = bf >> (log2K - 1), j = bf & (half - 1);
            const int k = j & (ns - 1), j0 = ((j - k) << 1) + k;
            tile[ln * pitch + j0] = make_double2(a[i].x + b[i].x, a[i].y + b[i].y);
            tile[ln * pitch + j0 + ns] = make_double2(a[i].x - b[i].x, a[i].y - b[i].y);
        }
        __syncthreads();
    }
    for (int i = t; i < FFT_TILE; i += PME_BLOCK) {
        const int ln = CONTIGUOUS ? (i >> log2K) : (i & (lines - 1));
        const int pos = CONTIGUOUS ? (i & (K - 1)) : (i >> lines_log2);
        if (ln < live) {
            const size_t l = first + ln;
            mesh[(l >> inner_log2) * outer + (l & (((size_t)1 << inner_log2) - 1)) + (size_t)pos * stride] = tile[ln * pitch + pos];
        }
    }
}

// comp < 0: W = A |b|^2 S; comp = 0 .. 5 (xx, yy, zz, xy, xz, yz): W = A |b|^2 2 k_a k_b (1 / k^2 + 1 / 4 alpha^2) S.  W(0) = 0.
// bmod: the three modulus tables one after the other (K_x, K_y, K_z entries).
static __global__ void k_pme_spectrum(PmeMesh g, double alpha, int comp, const double *__restrict__ bmod, const double2 *__restrict__ S,
                                      double2 *__restrict__ W) {
    const size_t total = (size_t)g.K[0] * g.K[1] * g.K[2];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int mz = (int)(i % g.K[2]), my = (int)((i / g.K[2]) % g.K[1]), mx = (int)(i / ((size_t)g.K[2] * g.K[1]));
    double factor = 0.0;
    if (i != 0) {
        const int m[3] = {mx, my, mz};
        double k[3];
#pragma unroll
        for (int d = 0; d < 3; d++) k[d] = 2.0 * M_PI * (double)(m[d] <= g.K[d] / 2 ? m[d] : m[d] - g.K[d]) * g.inv[d];
        const double k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2], q4 = 1.0 / (4.0 * alpha * alpha);
        factor = (4.0 * M_PI * g.inv[0] * g.inv[1] * g.inv[2]) * exp(-k2 * q4) / k2 * bmod[mx] * bmod[g.K[0] + my] * bmod[g.K[0] + g.K[1] + mz];
        if (comp >= 0) {
            const int a = comp < 3 ? comp : (comp == 5 ? 1 : 0), b = comp < 3 ? comp : (comp == 3 ? 1 : 2);
            const double ka = a == 0 ? k[0] : (a == 1 ? k[1] : k[2]), kb = b == 0 ? k[0] : (b == 1 ? k[1] : k[2]);
            factor *= 2.0 * ka * kb * (1.0 / k2 + q4);
        }
    }
    const double2 s = S[i];
    W[i] = make_double2(s.x * factor, s.y * factor);
}

// FIELD: phi is the convolved mesh: rows 0 .. 2 of `part` get -1/2 sum grad theta phi and, with ENERGY, row 3 gets
// 1/2 sum theta phi.  Otherwise phi is phi'_c and row `row` gets 1/2 sum theta phi.  (part: [row][slot], pitch slots a row.)
template <typename real, int P, bool FIELD, bool ENERGY>
__global__ __launch_bounds__(PME_BLOCK) void k_pme_gather(int n, size_t pitch, AtomView<real> atoms, PmeMesh g, const double2 *__restrict__ phi,
                                                          int row, double *__restrict__ part) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int p = blockIdx.x * (PME_BLOCK / WAVE) + threadIdx.x / WAVE;
    if (p >= n) return;                                      // (the whole wavefront; the kernel has no barrier)
    real x, y, z, hs, te;
    load_atom(atoms, p, x, y, z, hs, te);
    const PmeAxis ax = pme_axis<P>((double)x, g.lo[0], g.inv[0], g.K[0]), ay = pme_axis<P>((double)y, g.lo[1], g.inv[1], g.K[1]),
                     az = pme_axis<P>((double)z, g.lo[2], g.inv[2], g.K[2]);
    double se = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
#pragma unroll
    for (int s = lane; s < P * P * P; s += WAVE) {
        double th, gx, gy, gz;
        const double v = phi[pme_point<P, FIELD>(s, g, ax, ay, az, th, gx, gy, gz)].x;
        se += th * v;
        if (FIELD) { fx += gx * v; fy += gy * v; fz += gz * v; }
    }
    if (FIELD) {
        fx = wave_sum_to_lane63(fx); fy = wave_sum_to_lane63(fy); fz = wave_sum_to_lane63(fz);
        if (ENERGY) se = wave_sum_to_lane63(se);
        if (lane == WAVE - 1) {
            part[p] = -0.5 * fx; part[pitch + p] = -0.5 * fy; part[2 * pitch + p] = -0.5 * fz;
            if (ENERGY) part[3 * pitch + p] = 0.5 * se;
        }
    } else {
        se = wave_sum_to_lane63(se);
        if (lane == WAVE - 1) part[(size_t)row * pitch + p] = 0.5 * se;
    }
}

// The mesh pass of one engine: its setting, its tables and its device buffers (a member of EwaldRecip).
template <typename real>
struct PmeRecip {
    int32_t grid[3] = {0, 0, 0}, order = 0;                  // order 0: off
    DevBuf<double> bmod;                                     // |b_x|^2, |b_y|^2, |b_z|^2
    DevBuf<double2> tw;                                      // the twiddles of the three axes, 128 entries apart
    DevBuf<double2> spec, work;
    bool tables_current = false;

    bool on() const { return order != 0; }
    void set(const int32_t g[3], int32_t p) {
        for (int d = 0; d < 3; d++) grid[d] = g[d];
        order = p;
        tables_current = false;
    }
    void clear() { order = 0; }

    void upload(hipStream_t s) {
        std::vector<double> b, t((size_t)3 * 256, 0.0);
        for (int d = 0; d < 3; d++) {
            const std::vector<double> m = topo::pme_moduli(grid[d], order), w = topo::pme_twiddles(grid[d]);
            b.insert(b.end(), m.begin(), m.end());
            std::copy(w.begin(), w.end(), t.begin() + (size_t)d * 256);
        }
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));            // (nothing in flight reads the tables they replace)
        bmod.ensure(b.size());
        tw.ensure((size_t)3 * 128);
        EMDEE_HIP_CHECK(hipMemcpyAsync(bmod.ptr, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice, s));
        EMDEE_HIP_CHECK(hipMemcpyAsync(tw.ptr, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, s));
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        tables_current = true;
    }

    template <bool INVERSE>
    void fft(hipStream_t s, double2 *mesh) {
        const size_t Kx = grid[0], Ky = grid[1], Kz = grid[2], total = Kx * Ky * Kz;
        const size_t stride[3] = {Ky * Kz, Kz, 1}, outer[3] = {0, Ky * Kz, Kz};
        for (int d = 2; d >= 0; d--) {
            const int K = grid[d];
            int lg = 0, il = 0;
            while ((1 << lg) < K) lg++;
            while (((size_t)1 << il) < stride[d]) il++;       // (inner = the stride of the axis)
            const size_t nlines = total / K, lines = FFT_TILE / K;
            const dim3 blocks((unsigned)((nlines + lines - 1) / lines));
            with_bool(d == 2, [&](auto contiguous) {
                hipLaunchKernelGGL((k_pme_fft<INVERSE, decltype(contiguous)::value>), blocks, dim3(PME_BLOCK), 0, s, K, lg, nlines, stride[d], il,
                                   outer[d], tw.ptr + (size_t)d * 128, mesh);
            });
        }
    }

    template <int P>
    void run_order(hipStream_t s, int n, size_t pitch, const AtomView<real> &atoms, const PmeMesh &g, double alpha, const real *q,
                   int shift, bool all, double *part) {
        const size_t total = (size_t)grid[0] * grid[1] * grid[2];
        const unsigned ablocks = blocks_for(n, PME_BLOCK / WAVE), mblocks = blocks_for(total, 256);
        EMDEE_HIP_CHECK(hipMemsetAsync(work.ptr, 0, total * sizeof(long long), s));
        hipLaunchKernelGGL((k_pme_spread<real, P>), dim3(ablocks), dim3(PME_BLOCK), 0, s, n, atoms, g, q, std::ldexp(1.0, shift),
                           reinterpret_cast<unsigned long long *>(work.ptr));
        hipLaunchKernelGGL(k_pme_convert, dim3(mblocks), dim3(256), 0, s, total, reinterpret_cast<const long long *>(work.ptr),
                           std::ldexp(1.0, -shift), spec.ptr);
        fft<false>(s, spec.ptr);
        hipLaunchKernelGGL(k_pme_spectrum, dim3(mblocks), dim3(256), 0, s, g, alpha, -1, bmod.ptr, spec.ptr, work.ptr);
        fft<true>(s, work.ptr);
        if (!all) {
            hipLaunchKernelGGL((k_pme_gather<real, P, true, false>), dim3(ablocks), dim3(PME_BLOCK), 0, s, n, pitch, atoms, g, work.ptr, 0, part);
            return;
        }
        hipLaunchKernelGGL((k_pme_gather<real, P, true, true>), dim3(ablocks), dim3(PME_BLOCK), 0, s, n, pitch, atoms, g, work.ptr, 0, part);
        // One component at a time against the kept spectrum, so that two meshes are enough.  Each of the seven gathers works out
        // the atom's splines again: deliberate, the observable pass runs once per sample and a transform costs far more.
        for (int c = 0; c < 6; c++) {
            hipLaunchKernelGGL(k_pme_spectrum, dim3(mblocks), dim3(256), 0, s, g, alpha, c, bmod.ptr, spec.ptr, work.ptr);
            fft<true>(s, work.ptr);
            hipLaunchKernelGGL((k_pme_gather<real, P, false, false>), dim3(ablocks), dim3(PME_BLOCK), 0, s, n, pitch, atoms, g, work.ptr, 4 + c,
                               part);
        }
    }

    // fills rows 0 .. 2 (all: 0 .. 9) of part for the n atoms; q_abs: sum of |q| over them
    void run(hipStream_t s, int n, size_t pitch, const AtomView<real> &atoms, const double lo[3], const double len[3], double alpha,
             const real *q, double q_abs, bool all, double *part) {
        if (!tables_current) upload(s);
        PmeMesh g{};
        for (int d = 0; d < 3; d++) { g.lo[d] = lo[d]; g.inv[d] = 1.0 / len[d]; g.K[d] = grid[d]; }
        const size_t total = (size_t)grid[0] * grid[1] * grid[2];
        spec.ensure(total);
        work.ensure(total);
        const int shift = topo::pme_fixed_shift(q_abs);
        if (order == 4) run_order<4>(s, n, pitch, atoms, g, alpha, q, shift, all, part);
        else run_order<6>(s, n, pitch, atoms, g, alpha, q, shift, all, part);
    }
};

}  // namespace emdee
