"""numpy fp64 restatement of smooth particle-mesh Ewald as include/emdee_hip.h emdee_md_set_pme states it (Essmann et al., J. Chem.
Phys. 103, 8577, 1995), the yardstick of the PME engines.  Independent of the library's code: the B-splines by the Cox-de Boor
recursion as a function of x, the transforms by numpy.fft, the mesh by numpy.add.at.
  mesh K = grid, u = K (x - lo) / L, Q(m) = sum_j q_j prod_d M_p(u_jd - m_d) over periodic images,
  |b_d(m)|^2 = 1 / |sum_{k=0}^{p-2} M_p(k + 1) exp(2 pi i m k / K_d)|^2, k = 2 pi fold(m) / L with fold to (-K/2, K/2],
  A = (4 pi / V) exp(-k^2 / 4 a^2) / k^2, C = A |b_x|^2 |b_y|^2 |b_z|^2 (0 at m = 0),
  phi = F^-1[C F Q] (unnormalised), F_i = -K q_i sum_m grad theta phi, e_i = (K/2) q_i sum_m theta phi,
  W_i^ab = (K/2) q_i sum_m theta F^-1[C (delta_ab - 2 k_a k_b (1/k^2 + 1/(4 a^2))) F Q].
reciprocal(...) returns (f, e, w, t) of these alone; pme(...) adds ewald_ref.real_space, the self term and the background, as
ewald_ref.ewald does.  Tensors are (n, 6): xx, yy, zz, xy, xz, yz."""
import numpy as np

from . import ewald_ref as er
from .coulomb_ref import box_lengths

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def bspline(x, n):
    """M_n(x), the cardinal B-spline of order n (support [0, n]), by the Cox-de Boor recursion"""
    x = np.asarray(x, dtype=np.float64)
    if n == 1:
        return np.where((x >= 0.0) & (x < 1.0), 1.0, 0.0)
    return (x * bspline(x, n - 1) + (n - x) * bspline(x - 1.0, n - 1)) / (n - 1)


def dbspline(x, n):
    return bspline(x, n - 1) - bspline(np.asarray(x, dtype=np.float64) - 1.0, n - 1)


def fold(K):
    """the integers of the wave vectors of mesh indices 0 .. K - 1, in (-K/2, K/2]"""
    m = np.arange(K)
    return np.where(m <= K // 2, m, m - K)


def moduli(K, p):
    """|b(m)|^2, m = 0 .. K - 1"""
    k = np.arange(p - 1)
    s = (bspline(k + 1.0, p)[None, :] * np.exp(2j * np.pi * np.outer(np.arange(K), k) / K)).sum(axis=1)
    return 1.0 / np.abs(s) ** 2


def fixed_shift(sum_abs_q):
    """the exponent of the fixed-point scale of the charge mesh: with sum |q| < 2^e, 61 - e"""
    if sum_abs_q == 0.0:
        return 0
    return 61 - int(np.frexp(sum_abs_q)[1])


def _stencil(pos, lo, L, grid, p):
    """per atom and axis the p mesh indices it touches (n, 3, p), their weights and the derivatives of the weights by position"""
    grid = np.asarray(grid, dtype=np.int64)
    u = (np.asarray(pos, dtype=np.float64) - lo) / L * grid
    f = np.floor(u)
    j = np.arange(p)
    x = (u - f)[:, :, None] + j                                          # u - m for m = f - j
    m = np.mod(f.astype(np.int64)[:, :, None] - j, grid[None, :, None])
    return m, bspline(x, p), dbspline(x, p) * (grid / L)[None, :, None]


def charge_mesh(pos, L, q, grid, p, lo=(0.0, 0.0, 0.0)):
    L = box_lengths(L)
    m, w, _ = _stencil(pos, np.asarray(lo, dtype=np.float64), L, grid, p)
    Q = np.zeros(tuple(grid))
    th = w[:, 0, :, None, None] * w[:, 1, None, :, None] * w[:, 2, None, None, :]
    np.add.at(Q, (m[:, 0, :, None, None], m[:, 1, None, :, None], m[:, 2, None, None, :]), np.asarray(q)[:, None, None, None] * th)
    return Q


def _kernel(L, alpha, grid, p):
    """(C (Kx, Ky, Kz), k (3, Kx, Ky, Kz), k^2) of the box"""
    L = box_lengths(L)
    kx, ky, kz = np.meshgrid(*[2.0 * np.pi * fold(grid[d]) / L[d] for d in range(3)], indexing="ij")
    k2 = kx * kx + ky * ky + kz * kz
    k2[0, 0, 0] = 1.0
    bx, by, bz = (moduli(grid[d], p) for d in range(3))
    C = (4.0 * np.pi / np.prod(L)) * np.exp(-k2 / (4.0 * alpha * alpha)) / k2 * bx[:, None, None] * by[None, :, None] * bz[None, None, :]
    C[0, 0, 0] = 0.0
    return C, np.stack([kx, ky, kz]), k2


def reciprocal_energy(pos, L, q, K, alpha, grid, p, lo=(0.0, 0.0, 0.0)):
    """E = (K/2) sum_{m != 0} A |b|^2 |F Q|^2"""
    C, _, _ = _kernel(L, alpha, grid, p)
    FQ = np.fft.fftn(charge_mesh(pos, L, q, grid, p, lo))
    return 0.5 * K * (C * np.abs(FQ) ** 2).sum()


def reciprocal(pos, L, q, K, alpha, grid, p, lo=(0.0, 0.0, 0.0)):
    """(f, e, w, t) of the mesh sum alone (no self term, no background)"""
    L = box_lengths(L)
    q = np.asarray(q, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64)
    total = int(np.prod(grid))
    m, w, dw = _stencil(pos, lo, L, grid, p)
    ix = (m[:, 0, :, None, None], m[:, 1, None, :, None], m[:, 2, None, None, :])
    th = w[:, 0, :, None, None] * w[:, 1, None, :, None] * w[:, 2, None, None, :]
    C, k, k2 = _kernel(L, alpha, grid, p)
    FQ = np.fft.fftn(charge_mesh(pos, L, q, grid, p, lo))

    def back(spectrum):                                                  # the unnormalised inverse
        return np.fft.ifftn(spectrum).real * total

    phi = back(C * FQ)[ix]                                               # (n, p, p, p)
    e = 0.5 * K * q * (th * phi).sum(axis=(1, 2, 3))
    grad = [dw[:, 0, :, None, None] * w[:, 1, None, :, None] * w[:, 2, None, None, :],
            w[:, 0, :, None, None] * dw[:, 1, None, :, None] * w[:, 2, None, None, :],
            w[:, 0, :, None, None] * w[:, 1, None, :, None] * dw[:, 2, None, None, :]]
    f = -K * q[:, None] * np.stack([(g * phi).sum(axis=(1, 2, 3)) for g in grad], axis=1)
    t = np.zeros((q.shape[0], 6))
    b = 2.0 * (1.0 / k2 + 1.0 / (4.0 * alpha * alpha))
    for c, (a1, a2) in enumerate(PAIRS):
        factor = (1.0 if a1 == a2 else 0.0) - k[a1] * k[a2] * b
        t[:, c] = 0.5 * K * q * (th * back(C * factor * FQ)[ix]).sum(axis=(1, 2, 3))
    return f, e, t[:, :3].sum(axis=1), t


def pme(pos, L, q, K, alpha, grid, p, rc, excl=None, p14=None, s14=1.0, lo=(0.0, 0.0, 0.0)):
    """(f, e, w, t): every Coulomb term of a PME engine"""
    q = np.asarray(q, dtype=np.float64)
    n = q.shape[0]
    f, e, w, t = (a + b for a, b in zip(er.real_space(pos, L, q, K, alpha, rc, excl, p14, s14), reciprocal(pos, L, q, K, alpha, grid, p, lo)))
    e_bg = -np.pi * K * q.sum() ** 2 / (2.0 * np.prod(box_lengths(L)) * alpha * alpha) / n
    e = e - K * alpha / np.sqrt(np.pi) * q * q + e_bg
    t = t.copy()
    t[:, :3] += e_bg
    return f, e, w + 3.0 * e_bg, t


def energy(pos, L, q, K, alpha, grid, p, rc):
    return pme(pos, L, q, K, alpha, grid, p, rc)[1].sum()
