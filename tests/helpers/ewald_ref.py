"""numpy/scipy fp64 restatement of the Ewald sum of include/emdee_hip.h emdee_md_set_ewald, the yardstick of the Ewald engines.
With qq = K q_i q_j, V the volume, Q = sum q_i, N atoms, in a periodic orthorhombic box L = (Lx, Ly, Lz) (one number: a cube):
  real space, pairs with r^2 < rc^2 that are not struck:   U = qq erfc(a r)/r,  W = qq (erfc(a r)/r + (2a/sqrt(pi)) exp(-a^2 r^2))
  struck pair (excluded or 1-4; minimum image, no cutoff):  U = -qq erf(a r)/r,  W = -qq (erf(a r)/r - (2a/sqrt(pi)) exp(-a^2 r^2))
  1-4 pair, on top of that:                                 U = W = s14 qq / r
  reciprocal space, k = 2 pi n / L, |n_d| <= kmax[d], n != 0, A = (4 pi / V) exp(-k^2 / 4a^2) / k^2, S = sum_j q_j exp(i k.r_j):
      F_i = K q_i sum_k A k (sin(k.r_i) Re S - cos(k.r_i) Im S),   e_i = (K/2) q_i sum_k A (cos(k.r_i) Re S + sin(k.r_i) Im S),
      W_i^ab = (K/2) q_i sum_k A (cos Re S + sin Im S) (delta_ab - 2 k_a k_b (1/k^2 + 1/(4a^2)))
  self term -K (a/sqrt(pi)) q_i^2 in e_i;  background E_n = -pi K Q^2 / (2 V a^2): E_n/N in e_i and in xx, yy, zz of the tensor.
Pair terms go half to either atom; F_i = (W / r^2) d, d = r_i - r_j.  Tensors are (n, 6): xx, yy, zz, xy, xz, yz.
The reciprocal sum runs over the half space of n (n_x > 0, or n_x = 0 and n_y > 0, or n_x = n_y = 0 and n_z > 0) with a factor 2."""
import numpy as np
from scipy.special import erf, erfc

from .coulomb_ref import box_lengths, pairs_within

TWO_OVER_SQRT_PI = 2.0 / np.sqrt(np.pi)


def kmax3(kmax):
    k = np.broadcast_to(np.asarray(kmax, dtype=np.int64), (3,))
    return int(k[0]), int(k[1]), int(k[2])


def half_vectors(kmax):
    """the integer wave vectors of the half space, (m, 3), in ascending (n_x, n_y, n_z) order"""
    kx, ky, kz = kmax3(kmax)
    x, y, z = np.meshgrid(np.arange(0, kx + 1), np.arange(-ky, ky + 1), np.arange(-kz, kz + 1), indexing="ij")
    n = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    keep = (n[:, 0] > 0) | ((n[:, 0] == 0) & (n[:, 1] > 0)) | ((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] > 0))
    return n[keep]


def coefficients(n, L, alpha):
    """(k (m, 3), A(k) (m,)) of the integer vectors n in the box L"""
    L = box_lengths(L)
    k = 2.0 * np.pi * np.asarray(n, dtype=np.float64) / L
    k2 = (k * k).sum(axis=1)
    return k, (4.0 * np.pi / np.prod(L)) * np.exp(-k2 / (4.0 * alpha * alpha)) / k2


def _tensor6(a, b):
    return np.stack([a[:, 0] * b[:, 0], a[:, 1] * b[:, 1], a[:, 2] * b[:, 2], a[:, 0] * b[:, 1], a[:, 0] * b[:, 2], a[:, 1] * b[:, 2]], axis=1)


def reciprocal(pos, L, q, K, alpha, kmax, chunk=2048):
    """(f, e, w, t) of the reciprocal-space sum alone (no self term, no background)"""
    pos = np.asarray(pos, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = pos.shape[0]
    kall, Aall = coefficients(half_vectors(kmax), L, alpha)
    f, e, t = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 6))
    for a in range(0, kall.shape[0], chunk):
        k, A = kall[a:a + chunk], 2.0 * Aall[a:a + chunk]               # (the factor 2 of the half space)
        ph = pos @ k.T                                                 # (n, m)
        c, s = np.cos(ph), np.sin(ph)
        re, im = q @ c, q @ s
        f += K * q[:, None] * ((s * re - c * im) * A) @ k
        g = 0.5 * K * q[:, None] * (c * re + s * im) * A               # (n, m): the atom's share of E(k)
        e += g.sum(axis=1)
        k2 = (k * k).sum(axis=1)
        b = 2.0 * (1.0 / k2 + 1.0 / (4.0 * alpha * alpha))
        t -= g @ (_tensor6(k, k) * b[:, None])
        t[:, :3] += g.sum(axis=1)[:, None]
    return f, e, t[:, :3].sum(axis=1), t


def _pair_sum(pos, L, pairs, terms):
    """pair terms (U, W) = terms(r, i, j) of the listed pairs, shared as the library shares them"""
    n = pos.shape[0]
    f, e, w, t = np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros((n, 6))
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.shape[0] == 0:
        return f, e, w, t
    i, j = pairs[:, 0], pairs[:, 1]
    L = box_lengths(L)
    d = pos[i] - pos[j]
    d -= L * np.rint(d / L)
    r2 = (d * d).sum(axis=1)
    U, W = terms(np.sqrt(r2), i, j)
    fv = (W / r2)[:, None] * d
    tv = 0.5 * _tensor6(fv, d)
    for a, sgn in ((i, 1.0), (j, -1.0)):
        np.add.at(f, a, sgn * fv)
        np.add.at(e, a, 0.5 * U)
        np.add.at(w, a, 0.5 * W)
        np.add.at(t, a, tv)
    return f, e, w, t


def _table(tab):
    return np.zeros((0, 2), dtype=np.int64) if tab is None or len(tab) == 0 else np.asarray(tab, dtype=np.int64).reshape(-1, 2)


def real_space(pos, L, q, K, alpha, rc, excl=None, p14=None, s14=1.0):
    """(f, e, w, t) of the erfc pairs inside rc that are not struck, the corrections of the struck pairs and the 1-4 Coulomb terms"""
    pos = np.asarray(pos, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = pos.shape[0]
    excl, p14 = _table(excl), _table(p14)
    struck = np.concatenate([excl, p14])
    pairs = pairs_within(pos, L, rc)
    if struck.shape[0]:
        code = np.minimum(struck[:, 0], struck[:, 1]) * n + np.maximum(struck[:, 0], struck[:, 1])
        struck = np.unique(code)
        pairs = pairs[~np.isin(pairs[:, 0] * n + pairs[:, 1], struck)]
        struck = np.stack([struck // n, struck % n], axis=1)

    def screened(r, i, j):
        qq = K * q[i] * q[j]
        u = qq * erfc(alpha * r) / r
        return u, u + qq * TWO_OVER_SQRT_PI * alpha * np.exp(-(alpha * r) ** 2)

    def correction(r, i, j):
        qq = K * q[i] * q[j]
        u = -qq * erf(alpha * r) / r
        return u, u + qq * TWO_OVER_SQRT_PI * alpha * np.exp(-(alpha * r) ** 2)

    def bare14(r, i, j):
        u = s14 * K * q[i] * q[j] / r
        return u, u

    out = _pair_sum(pos, L, pairs, screened)
    for tab, fn in ((struck, correction), (p14, bare14)):
        out = tuple(a + b for a, b in zip(out, _pair_sum(pos, L, tab, fn)))
    return out


def ewald(pos, L, q, K, alpha, kmax, rc, excl=None, p14=None, s14=1.0):
    """(f, e, w, t): every Coulomb term of an Ewald engine"""
    q = np.asarray(q, dtype=np.float64)
    n = q.shape[0]
    f, e, w, t = (a + b for a, b in zip(real_space(pos, L, q, K, alpha, rc, excl, p14, s14), reciprocal(pos, L, q, K, alpha, kmax)))
    e_bg = -np.pi * K * q.sum() ** 2 / (2.0 * np.prod(box_lengths(L)) * alpha * alpha) / n
    e = e - K * alpha / np.sqrt(np.pi) * q * q + e_bg
    t = t.copy()
    t[:, :3] += e_bg
    return f, e, w + 3.0 * e_bg, t


def energy(pos, L, q, K, alpha, kmax, rc, excl=None, p14=None, s14=1.0):
    return ewald(pos, L, q, K, alpha, kmax, rc, excl, p14, s14)[1].sum()


def kmax_estimate(alpha, L, rc):
    """Per axis the smallest n with exp(-(pi n / (alpha L))^2) <= erfc(alpha rc): the reciprocal sum is cut where its Gaussian
    factor exp(-k^2 / 4 alpha^2) has fallen to the relative size of the real-space terms left out at rc (the exponential
    factors of the Kolafa-Perram error estimates; their prefactors are of order one at these parameters)."""
    L = box_lengths(L)
    return tuple(int(v) for v in np.ceil(alpha * L / np.pi * np.sqrt(-np.log(erfc(alpha * rc)))))


def rock_salt(cells=8):
    """cells^3 ions on a unit grid, charges +-1 alternating: (pos, L, q); its energy per ion is -M K / 2, M the Madelung constant"""
    g = np.arange(cells)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    pos = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float64)
    return pos, float(cells), np.where((x + y + z).ravel() % 2 == 0, 1.0, -1.0)


MADELUNG_NACL = 1.7475645946331822


def random_charges(n=300, L=(7.0, 8.0, 9.5), seed=5, min_sep=0.0, total=0.0):
    """n random positions in the box L (no two closer than min_sep: rejection, in order) and random charges with sum `total`"""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    pos = np.zeros((0, 3))
    while pos.shape[0] < n:
        x = rng.uniform(0.0, 1.0, 3) * L
        if pos.shape[0] and min_sep > 0.0:
            d = pos - x
            d -= L * np.rint(d / L)
            if (d * d).sum(axis=1).min() < min_sep * min_sep:
                continue
        pos = np.vstack([pos, x])
    q = rng.uniform(-1.0, 1.0, n)
    return pos, L, q - q.mean() + total / n
