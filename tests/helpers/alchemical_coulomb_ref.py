"""The numpy yardstick of the Coulomb stage of the alchemical table (include/emdee_hip.h: emdee_md_set_alchemical_coulomb), written
from the formulas of the contract, in float64:
    rho2 = r2 + beta (1 - lambda_q),  phi = 1/rho + k_rf rho2 - c_rf,  wl = 1/rho^3 - 2 k_rf
    U_q = lambda_q qq phi,  wr2_q = lambda_q qq wl,  W_q = wr2_q r2,  dU/dlambda_q = qq (phi + lambda_q (beta / 2) wl)
and the sums over the cross pairs of a box (one flagged, one unflagged atom, r^2 < rc^2, minimum image)."""
import numpy as np


def rf_constants(rc, eps_rf):
    """k_rf and c_rf of emdee_md_set_coulomb: k = (eps - 1) / ((2 eps + 1) rc^3) (1 / (2 rc^3) at eps = inf), c = 1/rc + k rc^2"""
    k = 0.5 / rc ** 3 if np.isinf(eps_rf) else (eps_rf - 1.0) / ((2.0 * eps_rf + 1.0) * rc ** 3)
    return k, 1.0 / rc + k * rc * rc


def pair(r2, qq, k_rf, c_rf, lam_q, beta):
    """(U_q, W_q, dU/dlambda_q, wr2_q) of the literal formulas; no cutoff (the caller's test)"""
    r2, qq, lam_q, beta = (np.asarray(v, dtype=np.float64) for v in (r2, qq, lam_q, beta))
    rho2 = r2 + beta * (1.0 - lam_q)
    with np.errstate(divide="ignore", invalid="ignore"):
        ir = 1.0 / np.sqrt(rho2)
        phi = ir + k_rf * rho2 - c_rf
        wl = ir ** 3 - 2.0 * k_rf
        U = lam_q * qq * phi
        wr2 = lam_q * qq * wl
        dl = qq * (phi + lam_q * 0.5 * beta * wl)
    return U, wr2 * r2, dl, wr2


def size(r2, qq, k_rf, c_rf, lam_q, beta):
    """the term's size before cancellation: |qq| (1/rho + k_rf rho2 + c_rf)"""
    rho2 = np.asarray(r2, dtype=np.float64) + beta * (1.0 - np.asarray(lam_q, dtype=np.float64))
    return np.abs(qq) * (1.0 / np.sqrt(rho2) + k_rf * rho2 + c_rf)


def plain_rf(r2, qq, k_rf, c_rf):
    """the model's own reaction-field pair: U = qq (1/r + k r^2 - c), W = qq (1/r - 2 k r^2)"""
    r2 = np.asarray(r2, dtype=np.float64)
    ir = 1.0 / np.sqrt(r2)
    return qq * (ir + k_rf * r2 - c_rf), qq * (ir - 2.0 * k_rf * r2)


def cross_pairs(pos, box, flag, rc):
    """(i, j, d) of every pair of one flagged (i) and one unflagged (j) atom with |d|^2 < rc^2, d = x_i - x_j at the minimum image"""
    pos = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    sol = np.flatnonzero(np.asarray(flag) == 1)
    env = np.flatnonzero(np.asarray(flag) == 0)
    d = pos[sol][:, None, :] - pos[env][None, :, :]
    d -= box * np.round(d / box)
    r2 = (d * d).sum(axis=2)
    a, b = np.nonzero(r2 < rc * rc)
    return sol[a], env[b], d[a, b]


def system(pos, box, flag, q, K, rc, eps_rf, lam_q, beta):
    """Every Coulomb pair term of a reaction-field box by the O(N^2) sum: a cross pair (one flagged, one unflagged atom) takes the
    soft core at (lam_q, beta), every other pair the plain reaction-field pair, which is the same formula at (1, 0).  Returns
    forces (n, 3), energies, virials (n,; half of a pair's to each atom), tensors (n, 6: xx, yy, zz, xy, xz, yz; half to each atom)
    and the words of the cross pairs: U, dUdl, W, pairs, and sizes, the sums of |U_q|, |dU/dlambda_q| and |W_q| over them.  A
    coincident cross pair (r = 0) is inside the cutoff and finite for beta (1 - lam_q) > 0."""
    pos = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    q = np.asarray(q, dtype=np.float64)
    flag = np.asarray(flag)
    n = len(pos)
    k_rf, c_rf = rf_constants(rc, eps_rf)
    i, j = np.triu_indices(n, 1)
    d = pos[i] - pos[j]
    d -= box * np.round(d / box)
    r2 = (d * d).sum(axis=1)
    keep = r2 < rc * rc
    i, j, d, r2 = i[keep], j[keep], d[keep], r2[keep]
    cross = flag[i] != flag[j]
    qq = K * q[i] * q[j]
    U, W, dl, wr2 = pair(r2, qq, k_rf, c_rf, np.where(cross, lam_q, 1.0), np.where(cross, beta, 0.0))
    f, e, w, t = np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros((n, 6))
    fd = wr2[:, None] * d
    np.add.at(f, i, fd)
    np.add.at(f, j, -fd)
    tv = 0.5 * np.stack([fd[:, 0] * d[:, 0], fd[:, 1] * d[:, 1], fd[:, 2] * d[:, 2], fd[:, 0] * d[:, 1], fd[:, 0] * d[:, 2],
                         fd[:, 1] * d[:, 2]], axis=1)
    for a in (i, j):
        np.add.at(e, a, 0.5 * U)
        np.add.at(w, a, 0.5 * W)
        np.add.at(t, a, tv)
    # the words of the cross pairs: dU/dlambda_q at the stage's own (lam_q, beta)
    Uc, Wc, dlc, _ = pair(r2[cross], qq[cross], k_rf, c_rf, lam_q, beta)
    return dict(forces=f, energies=e, virials=w, tensors=t, U=float(Uc.sum()), dUdl=float(dlc.sum()), W=float(Wc.sum()),
                pairs=int(cross.sum()), sizes=np.array([np.abs(Uc).sum(), np.abs(dlc).sum(), np.abs(Wc).sum()]))


def cross_words(pos, box, flag, q, K, rc, eps_rf, lam_q, beta):
    """(U_q, dU/dlambda_q, W_q, the sum of |U_q|) over the cross pairs alone"""
    i, j, d = cross_pairs(pos, box, flag, rc)
    k_rf, c_rf = rf_constants(rc, eps_rf)
    q = np.asarray(q, dtype=np.float64)
    U, W, dl, _ = pair((d * d).sum(axis=1), K * q[i] * q[j], k_rf, c_rf, lam_q, beta)
    return float(U.sum()), float(dl.sum()), float(W.sum()), float(np.abs(U).sum())
