"""numpy fp64 yardstick of rigid three-site molecules (include/emdee_hip.h: emdee_md_set_rigid3).  It does not use the SETTLE
formulas: the position stage is iterative SHAKE (one bond at a time, corrections along the bonds of x0, mass weighted) run to
a relative constraint residual of 1e-15, the velocity stage iterative RATTLE, and constrained_verlet puts them around a force
callback in the step of the header.  SETTLE is the closed-form solution of exactly those SHAKE equations, so the library must
agree with this file to rounding.  Plain numpy; it never calls the library.

mol: (n, 3) ids {apex, a, b}; geom: (n, 2) {d_leg, d_base}; mass: (N,).  Positions are unwrapped: the three sites of a
molecule differ by the molecule's own vectors, no box lengths (unwrap() makes them so).

Run as a program (python -m tests.helpers.settle_ref) it prints the energy drift of the reference on the box of
tests/test_gpu_settle.py, the constant REFERENCE_DRIFT of that file."""
import numpy as np

BONDS = ((0, 1, 0), (0, 2, 0), (1, 2, 1))               # (site, site, column of geom)


def unwrap(pos, mol, lengths, periodic=(1, 1, 1)):
    """pos with the legs of every molecule moved to their minimum image from the apex (taken on the periodic axes only)"""
    x = np.array(pos, dtype=np.float64)
    ln = np.asarray(lengths, dtype=np.float64) * np.asarray(periodic, dtype=bool)
    for k in (1, 2):
        d = x[mol[:, k]] - x[mol[:, 0]]
        x[mol[:, k]] = x[mol[:, 0]] + d - ln * np.rint(d / np.where(ln > 0.0, ln, 1.0))
    return x


def distances(x, mol):
    """(n, 3): |apex - a|, |apex - b|, |a - b|"""
    return np.stack([np.linalg.norm(x[mol[:, i]] - x[mol[:, j]], axis=1) for i, j, _ in BONDS], axis=1)


def residual(x, mol, geom):
    """largest relative deviation of a distance from its constraint"""
    want = np.stack([geom[:, c] for _, _, c in BONDS], axis=1)
    return np.abs(distances(x, mol) / want - 1.0).max()


def _local(x, mol, origin):
    return np.stack([x[mol[:, k]] - origin for k in range(3)], axis=1)           # (n, 3 sites, 3)


def shake(x0, x1, mol, geom, mass, tol=1e-15, max_iter=2000):
    """x1 + sum_k lambda_k (x0_i - x0_j) / m_i with the three distances restored, by sweeps over the bonds.  Works on
    coordinates relative to each molecule's x0 apex (an exact shift), where a residual of 1e-15 can be resolved."""
    mol = np.asarray(mol, dtype=np.int64)
    origin = x0[mol[:, 0]]
    y0, y = _local(x0, mol, origin), _local(x1, mol, origin)
    w = 1.0 / np.asarray(mass, dtype=np.float64)[mol]                            # (n, 3)
    best, since = np.inf, 0
    for sweep in range(max_iter):
        worst = 0.0
        for i, j, c in BONDS:
            d2 = geom[:, c] ** 2
            s, r0 = y[:, i] - y[:, j], y0[:, i] - y0[:, j]
            diff = d2 - np.einsum("ij,ij->i", s, s)
            worst = max(worst, np.abs(diff / d2).max())
            g = diff / (2.0 * (w[:, i] + w[:, j]) * np.einsum("ij,ij->i", s, r0))
            y[:, i] += (g * w[:, i])[:, None] * r0
            y[:, j] -= (g * w[:, j])[:, None] * r0
        if worst <= 2.0 * tol:                                                   # (|s|^2 / d^2 - 1 = 2 (|s| / d - 1))
            break
        since = 0 if worst < best else since + 1
        best = min(best, worst)
        assert since < 50, "SHAKE stalls at a residual of %.3e" % (0.5 * best)
    else:
        raise AssertionError("SHAKE did not converge: residual %.3e" % (0.5 * worst))
    out = np.array(x1, dtype=np.float64)
    for k in range(3):
        out[mol[:, k]] = y[:, k] + origin
    return out


def rattle(x, v, mol, mass, tol=1e-16, max_iter=5000):
    """v + sum_k mu_k (x_i - x_j) / m_i with no relative velocity along any of the three bonds, by sweeps over the bonds; stops
    when every |(v_i - v_j) . (x_i - x_j)| is within tol |v| d (|v|: the molecule's largest speed) or no longer shrinks"""
    mol = np.asarray(mol, dtype=np.int64)
    y = _local(x, mol, x[mol[:, 0]])
    u = np.stack([v[mol[:, k]] for k in range(3)], axis=1)
    w = 1.0 / np.asarray(mass, dtype=np.float64)[mol]
    speed = np.linalg.norm(u, axis=2).max(axis=1) + 1e-300
    best, since = np.inf, 0
    for sweep in range(max_iter):
        worst = 0.0
        for i, j, _ in BONDS:
            r, dv = y[:, i] - y[:, j], u[:, i] - u[:, j]
            rv, rr = np.einsum("ij,ij->i", r, dv), np.einsum("ij,ij->i", r, r)
            worst = max(worst, (np.abs(rv) / (np.sqrt(rr) * speed)).max())
            g = -rv / ((w[:, i] + w[:, j]) * rr)
            u[:, i] += (g * w[:, i])[:, None] * r
            u[:, j] -= (g * w[:, j])[:, None] * r
        if worst <= tol:
            break
        since = 0 if worst < best else since + 1
        best = min(best, worst)
        if since >= 20:
            assert best <= 1e-15, "RATTLE stalls at a residual of %.3e" % best
            break
    else:
        raise AssertionError("RATTLE did not converge: residual %.3e" % worst)
    out = np.array(v, dtype=np.float64)
    for k in range(3):
        out[mol[:, k]] = u[:, k]
    return out


def bond_velocities(x, v, mol):
    """(n, 3): |(v_i - v_j) . (x_i - x_j)| / (|v| d) per bond, |v| the molecule's largest speed"""
    speed = np.stack([np.linalg.norm(v[mol[:, k]], axis=1) for k in range(3)], axis=1).max(axis=1) + 1e-300
    out = []
    for i, j, _ in BONDS:
        r, dv = x[mol[:, i]] - x[mol[:, j]], v[mol[:, i]] - v[mol[:, j]]
        out.append(np.abs(np.einsum("ij,ij->i", r, dv)) / (np.linalg.norm(r, axis=1) * speed))
    return np.stack(out, axis=1)


def constrained_verlet(pos, vel, force, nsteps, dt, mol, geom, mass, langevin=None, observe=None):
    """The step of emdee_md_set_rigid3 around force(x, k) -> (N, 3): k = 0 for the starting positions, k = s for those after
    the position stage of step s (from 1).  pos unwrapped and on the constraints, vel without bond components.  langevin =
    (gamma, temperature, normals) as ortho_ref.verlet.  observe(s, x, v): called after every step.  Returns (x, v)."""
    x, v = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    im = (1.0 / mass)[:, None]
    f = force(x, 0)
    for s in range(1, nsteps + 1):
        x0 = x.copy()
        v += 0.5 * dt * im * f
        if langevin is not None:
            gamma, temperature, normals = langevin
            c1 = np.exp(-gamma * dt)
            v = c1 * v + np.sqrt(1.0 - c1 * c1) * np.sqrt(temperature * im) * normals(s - 1)
        x += dt * v
        xc = shake(x0, x, mol, geom, mass)
        v += (xc - x) / dt
        x = xc
        f = force(x, s)
        v += 0.5 * dt * im * f
        v = rattle(x, v, mol, mass)
        if observe is not None:
            observe(s, x, v)
    return x, v


# ---------------------------------------------------------------- the box the GPU tests share
N_MOL, LENGTHS, LO = 150, np.array([7.0, 7.5, 8.2]), np.array([-1.0, 0.5, 2.0])
RC, RS, SKIN, DT = 2.5, 2.0, 0.4, 0.002
MASSES, D_LEG, D_BASE = (16.0, 1.0, 1.0), 0.32, 0.50
HALF_SIGMA, TWICE_SQRT_EPS = (0.5, 0.2, 0.2), (2.0, 1.0, 1.0)
CHARGES = (-0.8, 0.4, 0.4)
_CACHE = {}


def triangle(d_leg, d_base):
    """the three sites in a plane, apex at the origin"""
    h = np.sqrt(d_leg ** 2 - 0.25 * d_base ** 2)
    return np.array([[0.0, 0.0, 0.0], [-0.5 * d_base, -h, 0.0], [0.5 * d_base, -h, 0.0]])


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    a, b, c, d = q.T
    return np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], axis=1),
                     np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], axis=1),
                     np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], axis=1)], axis=1)


def water_box(seed=11, temperature=1.0, n_mol=N_MOL, lengths=LENGTHS, lo=LO):
    """150 three-site molecules: centres on a jittered 5 x 5 x 6 lattice, random orientations, every atom wrapped into the box
    on its own (molecules straddle box faces and cell faces), velocities drawn at `temperature` and projected by rattle().
    dict(pos (wrapped), unwrapped, vel, mol, geom, mass, atoms, excl, charges); computed once per process."""
    key = (seed, temperature, n_mol, tuple(lengths), tuple(lo))
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        lengths, lo = np.asarray(lengths, dtype=np.float64), np.asarray(lo, dtype=np.float64)
        side = int(np.ceil(n_mol ** (1.0 / 3.0)))
        grid = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side + 1)], dtype=np.float64)[:n_mol]
        shape = np.array([side, side, side + 1], dtype=np.float64)
        centres = lo + (grid + 0.5 + 0.2 * (rng.random((n_mol, 3)) - 0.5)) / shape * lengths
        sites = np.einsum("nij,kj->nki", random_rotations(rng, n_mol), triangle(D_LEG, D_BASE))
        x = (centres[:, None, :] + sites).reshape(-1, 3)
        mol = np.arange(3 * n_mol, dtype=np.int64).reshape(-1, 3)
        geom = np.tile([D_LEG, D_BASE], (n_mol, 1))
        mass = np.tile(MASSES, n_mol)
        v = rng.normal(size=x.shape) * np.sqrt(temperature / mass)[:, None]
        v -= (mass[:, None] * v).sum(axis=0) / mass.sum()
        v = rattle(x, v, mol, mass)
        atoms = np.zeros(3 * n_mol, dtype=np.dtype([("half_sigma", np.float32), ("twice_sqrt_eps", np.float32)]))
        atoms["half_sigma"], atoms["twice_sqrt_eps"] = np.tile(HALF_SIGMA, n_mol), np.tile(TWICE_SQRT_EPS, n_mol)
        excl = np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]])
        _CACHE[key] = dict(pos=lo + np.mod(x - lo, lengths), unwrapped=x, vel=v, mol=mol, geom=geom, mass=mass, atoms=atoms, excl=excl,
                           charges=np.tile(CHARGES, n_mol))
    return {k: np.array(v) for k, v in _CACHE[key].items()}


def reference_drift(nsteps=400, every=20):
    """max |E(t) - E(0)| of constrained_verlet on water_box() with the all-pairs forces of ortho_ref, sampled every `every` steps"""
    from . import ortho_ref as oref
    B = water_box()
    total = lambda x: oref.total(x, LO, LENGTHS, [1, 1, 1], RC, RS, B["atoms"], excl=B["excl"])
    energy = lambda x, v: total(x)["e"].sum() + 0.5 * (B["mass"][:, None] * v * v).sum()
    e0, seen = energy(B["unwrapped"], B["vel"]), []

    def observe(s, x, v):
        if s % every == 0:
            seen.append(abs(energy(x, v) - e0))
    constrained_verlet(B["unwrapped"], B["vel"], lambda x, k: total(x)["f"], nsteps, DT, B["mol"], B["geom"], B["mass"], observe=observe)
    return max(seen), e0


if __name__ == "__main__":
    drift, e0 = reference_drift()
    print("reference: max |E(t) - E(0)| over 400 steps of dt = %g, sampled every 20: %.6e (E(0) = %.6f)" % (DT, drift, e0))
