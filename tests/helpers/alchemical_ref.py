"""numpy yardstick of the soft-core alchemical decoupling (include/emdee_hip.h: emdee_md_set_alchemical), written from the formulas
of the contract, not from the library's header.  It never calls the library.  Everything is float64 unless a dtype is asked for.

    u = (r^2 / sigma^2)^3,  D = alpha (1 - lambda) + u
    U    = lambda e4 (D^-2 - D^-1) g
    W    = -r dU/dr = 6 u lambda e4 (2 D^-3 - D^-2) g + (U / g) (-r g')
    dUdl = e4 g [(D^-2 - D^-1) + lambda alpha (2 D^-3 - D^-2)]

with g = 1 + x^3 (15 x - 6 x^2 - 10), x = (r^2 - rs^2) / (rc^2 - rs^2) clamped as the reference clamps it, -r g' = 60 x^2 (1 - x)^2 r^2
/ (rc^2 - rs^2), and e4 = 4 eps_ij.  The pair functions are LITERAL (no cutoff test); system() applies r^2 < rc^2 as every pair loop."""
import numpy as np

COMPONENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # xx, yy, zz, xy, xz, yz


def switch(r2, rc, rs):
    """g and -r g' (the reference's clamp: 0 < x < 1 -> x; x <= 0 -> 0; x == 1 -> 0.5; x > 1 -> 0)"""
    r2 = np.asarray(r2, dtype=np.float64)
    idl2 = 1.0 / (rc * rc - rs * rs)
    x = r2 * idl2 - rs * rs * idl2
    x = np.where(x > 0.0, x, 0.0)
    x = np.where(x >= 1.0, np.where(x == 1.0, 0.5, 0.0), x)
    g = 1.0 + x ** 3 * (15.0 * x - 6.0 * x * x - 10.0)
    mgr = 60.0 * x * x * (1.0 - x) ** 2 * idl2 * r2
    return g, mgr


def plain_pair(r2, rc, rs, sigma2, e4):
    """(E, W) of the model's own pair function"""
    r2 = np.asarray(r2, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s6 = (sigma2 / r2) ** 3
        E = e4 * (s6 * s6 - s6)
        W = 6.0 * e4 * (2.0 * s6 * s6 - s6)
        g, mgr = switch(r2, rc, rs)
        return E * g, W * g + E * mgr


def literal_pair(r2, rc, rs, sigma2, e4, dtype):
    """lj_interaction_pair operation by operation in `dtype` (csrc/lj_pair.hpp: the comparison at lambda = 1 is to a few ulp of this)"""
    t = dtype
    r2, sigma2, e4 = t(r2), t(sigma2), t(e4)
    rc2, rs2 = t(rc * rc), t(rs * rs)
    idl2 = t(1.0 / (rc * rc - rs * rs))
    x0 = t(rs2 * idl2)
    c60 = t(t(60) * idl2)
    s2 = t(sigma2 * t(t(1) / r2))
    s6 = t(t(s2 * s2) * s2)
    e4s6 = t(e4 * s6)
    tt = t(e4s6 * s6)
    E = t(tt - e4s6)
    W = t(t(6) * t(E + tt))
    x = t(t(r2 * idl2) - x0)
    x = x if x > 0 else t(0)
    if x >= 1:
        x = t(0.5) if x == 1 else t(0)
    u = t(t(1) - x)
    u2 = t(u * u)
    g = t(t(u2 * u) * t(t(1) + t(x * t(t(3) + t(t(6) * x)))))
    mgr = t(t(c60 * t(t(x * x) * u2)) * r2)
    return float(t(E * g)), float(t(t(W * g) + t(E * mgr)))


def pair(r2, rc, rs, sigma2, e4, lam, alpha):
    """(U, W, dUdl, W / r^2) of one cross pair, vectorised; W / r^2 is formed without dividing by r^2 (u / r^2 = r^4 / sigma^6)"""
    r2 = np.asarray(r2, dtype=np.float64)
    u = (r2 / sigma2) ** 3
    D = alpha * (1.0 - lam) + u
    with np.errstate(divide="ignore", invalid="ignore"):
        El = e4 * (D ** -2 - D ** -1)
        Wl = e4 * (2.0 * D ** -3 - D ** -2)
    g, mgr = switch(r2, rc, rs)
    mg2 = np.where(r2 > 0.0, mgr / np.where(r2 > 0.0, r2, 1.0), 0.0)   # -r g' / r^2 = 60 x^2 (1 - x)^2 idl2, 0 below the switch
    U = lam * El * g
    W = 6.0 * u * lam * Wl * g + lam * El * mgr
    wr2 = 6.0 * (r2 * r2 / sigma2 ** 3) * lam * Wl * g + lam * El * mg2
    dUdl = g * (El + lam * alpha * Wl)
    if np.ndim(lam) == 0 and lam == 0.0:
        U, W, wr2 = np.zeros_like(U), np.zeros_like(W), np.zeros_like(wr2)
    return U, W, dUdl, wr2


def system(pos, lengths, rc, rs, hs, te, flag=None, lam=1.0, alpha=0.0, excl=None, block=256):
    """Every pair term of the box by the O(N^2) sum, owner by owner (half of a pair's E and W to either atom): forces (N, 3), energies,
    virials (N,), tensors (N, 6), and -- with flag -- the alchemical words of the cross pairs: U, dUdl, W, pairs (inside rc).  Cross
    pairs (one flagged, one unflagged atom) take the soft core at (lam, alpha), every other pair the plain function.  excl: (n, 2)
    pairs left out altogether."""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    hs = np.asarray(hs, np.float32).astype(np.float64)
    te = np.asarray(te, np.float32).astype(np.float64)
    flag = np.zeros(N, dtype=np.int64) if flag is None else np.asarray(flag, dtype=np.int64)
    L = np.asarray(lengths, dtype=np.float64)
    skip = np.zeros((0, 2), dtype=np.int64) if excl is None else np.asarray(excl, dtype=np.int64).reshape(-1, 2)
    f, e, w, t = np.zeros((N, 3)), np.zeros(N), np.zeros(N), np.zeros((N, 6))
    out = dict(U=0.0, dUdl=0.0, W=0.0, pairs=0)
    sizes = np.zeros(3)
    for lo in range(0, N, block):
        I = np.arange(lo, min(N, lo + block))
        d = pos[I, None, :] - pos[None, :, :]
        d -= L * np.rint(d / L)
        r2 = np.einsum("ijk,ijk->ij", d, d)
        keep = r2 < rc * rc
        keep[np.arange(len(I)), I] = False
        for a, b in skip:
            for p, q in ((a, b), (b, a)):
                if lo <= p < lo + len(I):
                    keep[p - lo, q] = False
        sigma2 = (hs[I, None] + hs[None, :]) ** 2
        e4 = te[I, None] * te[None, :]
        cross = flag[I, None] != flag[None, :]
        r2s = np.where(keep, r2, 1.0)
        Ep, Wp = plain_pair(r2s, rc, rs, sigma2, e4)
        Ea, Wa, dl, wr2a = pair(r2s, rc, rs, sigma2, e4, lam, alpha)
        # (a coincident cross pair: r2 = 0 is inside the cutoff and finite under the soft core)
        zero = keep & (r2 == 0.0) & cross
        if zero.any():
            Ez, Wz, dz, wz = pair(np.zeros(1), rc, rs, sigma2[zero], e4[zero], lam, alpha)
            Ea[zero], Wa[zero], dl[zero], wr2a[zero] = Ez, Wz, dz, wz
        E = np.where(keep, np.where(cross, Ea, Ep), 0.0)
        W = np.where(keep, np.where(cross, Wa, Wp), 0.0)
        wr2 = np.where(keep, np.where(cross, wr2a, Wp / r2s), 0.0)
        f[I] = np.einsum("ij,ijk->ik", wr2, d)
        e[I] = 0.5 * E.sum(axis=1)
        w[I] = 0.5 * W.sum(axis=1)
        for c, (a, b) in enumerate(COMPONENTS):
            t[I, c] = 0.5 * (wr2 * d[:, :, a] * d[:, :, b]).sum(axis=1)
        kc = keep & cross
        out["U"] += 0.5 * Ea[kc].sum()
        out["dUdl"] += 0.5 * dl[kc].sum()
        out["W"] += 0.5 * Wa[kc].sum()
        out["pairs"] += int(kc.sum())
        sizes += 0.5 * np.array([np.abs(Ea[kc]).sum(), np.abs(dl[kc]).sum(), np.abs(Wa[kc]).sum()])
    out["pairs"] //= 2
    out.update(forces=f, energies=e, virials=w, tensors=t, sizes=sizes)   # sizes: the sums of |U|, |dUdl|, |W| over the cross pairs
    return out


def cross_pairs(pos, lengths, rc, hs, te, flag):
    """(r2, sigma2, e4) of every cross pair inside rc, each once"""
    pos = np.asarray(pos, dtype=np.float64)
    hs = np.asarray(hs, np.float32).astype(np.float64)
    te = np.asarray(te, np.float32).astype(np.float64)
    flag = np.asarray(flag)
    L = np.asarray(lengths, dtype=np.float64)
    sol, env = np.where(flag == 1)[0], np.where(flag == 0)[0]
    d = pos[sol, None, :] - pos[None, env, :]
    d -= L * np.rint(d / L)
    r2 = np.einsum("ijk,ijk->ij", d, d)
    i, j = np.nonzero(r2 < rc * rc)
    return r2[i, j], (hs[sol[i]] + hs[env[j]]) ** 2, te[sol[i]] * te[env[j]]
