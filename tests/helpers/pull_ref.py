"""numpy yardstick of the centre-of-mass pull (include/emdee_hip.h: emdee_md_set_pull).  It never calls the library: it works on the
unwrapped positions emdee_md_get_state returns, the masses and the group array, in float64 throughout.  A coordinate is a dict with
a, b, kind (1 umbrella, 2 constant force), geometry (1 distance, 2 direction), mask (bits 1..7), k (or F), r0, rate, n (3,)."""
import numpy as np

UMBRELLA, CONSTANT_FORCE, DISTANCE, DIRECTION = 1, 2, 1, 2
ORDER = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))           # xx, yy, zz, xy, xz, yz


def unit(n):
    n = np.asarray(n, dtype=np.float64)
    return n / np.sqrt((n * n).sum())


def term(c, xi0, D):
    """xi, f, U, F_b (3,), T (6,) of one coordinate at D = R_b - R_a"""
    D = np.asarray(D, dtype=np.float64)
    if c["geometry"] == DIRECTION:
        g = unit(c["n"])
        xi = float(g @ D)
    else:
        m = np.array([(c["mask"] >> a) & 1 for a in range(3)], dtype=np.float64)
        md = m * D
        xi = float(np.sqrt((md * md).sum()))
        g = md / xi if xi > 0.0 else np.zeros(3)
    if c["kind"] == CONSTANT_FORCE:
        f, U = c["k"], -c["k"] * xi
    else:
        f, U = -c["k"] * (xi - xi0), 0.5 * c["k"] * (xi - xi0) ** 2
    Fb = f * g
    T = np.array([0.5 * (D[i] * Fb[j] + D[j] * Fb[i]) for i, j in ORDER])
    return xi, f, U, Fb, T


def centres(x, m, group, n_groups):
    """R (n_groups, 3) and M (n_groups,)"""
    R, M = np.zeros((n_groups, 3)), np.zeros(n_groups)
    for g in range(n_groups):
        sel = group == g
        M[g] = m[sel].sum()
        R[g] = (m[sel, None] * x[sel]).sum(axis=0) / M[g]
    return R, M


def evaluate(x, m, group, coords, xi0, n_groups):
    """The pull part of every per-atom plane and the read-back words.  Returns a dict: forces (n, 3), energies (n,), virials (n,),
    tensors (n, 6), words (n_coords, 8) = xi, xi0, f, U, 0 (work: not a function of the state), D; centres, masses; U (n_coords,),
    W (n_coords, 6) = sym(D (x) F_b)."""
    x, m, group = np.asarray(x, dtype=np.float64), np.asarray(m, dtype=np.float64), np.asarray(group)
    n = x.shape[0]
    R, M = centres(x, m, group, n_groups)
    A, E, Tg = np.zeros((n_groups, 3)), np.zeros(n_groups), np.zeros((n_groups, 6))
    words, Us, Ws = np.zeros((len(coords), 8)), np.zeros(len(coords)), np.zeros((len(coords), 6))
    for k, c in enumerate(coords):
        D = R[c["b"]] - R[c["a"]]
        xi, f, U, Fb, T = term(c, xi0[k], D)
        words[k] = [xi, xi0[k], f, U, 0.0, D[0], D[1], D[2]]
        Us[k], Ws[k] = U, T
        for g, sign in ((c["a"], -1.0), (c["b"], 1.0)):
            A[g] += sign * Fb / M[g]
            E[g] += 0.5 * U / M[g]
            Tg[g] += 0.5 * T / M[g]
    out = dict(forces=np.zeros((n, 3)), energies=np.zeros(n), virials=np.zeros(n), tensors=np.zeros((n, 6)), words=words, centres=R,
               masses=M, U=Us, W=Ws)
    sel = group >= 0
    g = group[sel]
    out["forces"][sel] = m[sel, None] * A[g]
    out["energies"][sel] = m[sel] * E[g]
    out["tensors"][sel] = m[sel, None] * Tg[g]
    out["virials"] = out["tensors"][:, :3].sum(axis=1)
    return out


def advance(xi0, rate, dt, n):
    """the host's sequence: n times xi0 <- xi0 + rate dt, one fp64 addition per step"""
    xi0, step = np.float64(xi0), np.float64(rate) * np.float64(dt)
    for _ in range(n):
        xi0 = xi0 + step
    return float(xi0)


def work_rule(f, rate, dt):
    """the rectangle rule: work after each step, work_s = work_(s-1) + f_s rate dt with f_s at the pass that closes step s"""
    w, out = 0.0, []
    for fs in f:
        w = w + fs * rate * dt
        out.append(w)
    return np.array(out)


def verlet(x, v, m, group, coords, n_groups, dt, nsteps):
    """velocity Verlet under the pull alone; xi0 advances by rate dt per completed step before the step's closing force evaluation.
    Returns x, v, xi0 (n_coords,), work (n_coords,), the f of every closing pass (nsteps, n_coords) and the amplitudes of the motion:
    the largest |x - x(0)| and the largest |v| over the run."""
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    x_start, amp_x, amp_v = x.copy(), 0.0, np.abs(v).max()
    xi0 = np.array([c["r0"] for c in coords], dtype=np.float64)
    work, fs = np.zeros(len(coords)), np.zeros((nsteps, len(coords)))
    F = evaluate(x, m, group, coords, xi0, n_groups)["forces"]
    for s in range(nsteps):
        v += 0.5 * dt * F / m[:, None]
        x += dt * v
        for k, c in enumerate(coords):
            xi0[k] = xi0[k] + c["rate"] * dt
        ev = evaluate(x, m, group, coords, xi0, n_groups)
        F = ev["forces"]
        v += 0.5 * dt * F / m[:, None]
        for k, c in enumerate(coords):
            fs[s, k] = ev["words"][k, 2]
            if c["kind"] == UMBRELLA:
                work[k] = work[k] + fs[s, k] * c["rate"] * dt
        amp_x, amp_v = max(amp_x, np.abs(x - x_start).max()), max(amp_v, np.abs(v).max())
    return x, v, xi0, work, fs, (amp_x, amp_v)
