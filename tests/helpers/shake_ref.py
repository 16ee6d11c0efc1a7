"""numpy fp64 yardstick of bonds held at fixed lengths (include/emdee_hip.h: emdee_md_set_hbonds, and emdee_md_set_rigid3 beside
it).  It does not use the Newton / matrix form of csrc/shake.hpp: the position stage is Gauss-Seidel SHAKE over a list of pairs
(one bond at a time, corrections along the bonds of x0, mass weighted) run to a relative constraint residual of 1e-15 (2e-15
where the sweeps stall at the rounding of the coordinates), the
velocity stage Gauss-Seidel RATTLE, and constrained_verlet puts them around a force callback in the order of stages (a) to (e)
of the header.  The library solves exactly those SHAKE equations, so it must agree with this file to rounding.  A rigid
three-site molecule is three pairs of the same list (settle_ref.BONDS), so one list holds clusters and waters together.
Plain numpy; it never calls the library.

pairs: (P, 3) float64 rows {i, j, d}; clusters: (n, 4) ids {centre, s1, s2, s3}, -1 in unused trailing slots; dist: (n, 3).
Positions are unwrapped: the atoms of a constrained group differ by the group's own vectors, no box lengths.

Run as a program (python -m tests.helpers.shake_ref) it prints the energy drift of the reference on mixed_box()."""
import numpy as np

from . import settle_ref as sr


def cluster_pairs(clusters, dist):
    """(P, 3) rows {centre, satellite, d} of the slots in use"""
    clusters, dist = np.asarray(clusters, dtype=np.int64).reshape(-1, 4), np.asarray(dist, dtype=np.float64).reshape(-1, 3)
    rows = [(c[0], c[1 + k], d[k]) for c, d in zip(clusters, dist) for k in range(3) if c[1 + k] >= 0]
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def triangle_pairs(mol, geom):
    """(3 n, 3) rows of the three bonds of rigid three-site molecules"""
    rows = [(m[i], m[j], g[c]) for m, g in zip(np.asarray(mol, dtype=np.int64), np.asarray(geom, dtype=np.float64)) for i, j, c in sr.BONDS]
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _plan(pairs, n_atoms):
    """(i, j, d) as arrays, the colours (lists of pair indices in which no atom appears twice: one vectorised Gauss-Seidel
    update each, in a fixed order) and root[atom]: the lowest id of the atom's constrained group"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 3)
    i, j, d = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64), pairs[:, 2]
    used, colours, root = {}, [], np.arange(n_atoms)

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    for k in range(len(i)):
        taken = used.setdefault(int(i[k]), set()) | used.setdefault(int(j[k]), set())
        c = next(c for c in range(len(taken) + 1) if c not in taken)
        used[int(i[k])].add(c); used[int(j[k])].add(c)
        if c == len(colours):
            colours.append([])
        colours[c].append(k)
        a, b = find(int(i[k])), find(int(j[k]))
        root[max(a, b)] = min(a, b)
    root = np.array([find(a) for a in range(n_atoms)])
    return i, j, d, [np.array(c, dtype=np.int64) for c in colours], root


def residual(x, pairs):
    """largest relative deviation of a distance from its constraint"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 3)
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    return np.abs(np.linalg.norm(x[i] - x[j], axis=1) / pairs[:, 2] - 1.0).max()


def shake(x0, x1, pairs, mass, tol=1e-15, max_iter=5000):
    """x1 + sum_k lambda_k (x0_i - x0_j) / m_i with every distance restored, by sweeps over the pairs.  Works on coordinates
    relative to x0 of each group's lowest atom (an exact shift), where a residual of 1e-15 can be resolved."""
    i, j, d, colours, root = _plan(pairs, len(x0))
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    origin = x0[root]
    y0, y = x0 - origin, x1 - origin
    w = 1.0 / np.asarray(mass, dtype=np.float64)
    best, kept, since = np.inf, y, 0
    for sweep in range(max_iter):
        for c in colours:
            a, b, d2 = i[c], j[c], d[c] ** 2
            s, r0 = y[a] - y[b], y0[a] - y0[b]
            g = (d2 - np.einsum("ij,ij->i", s, s)) / (2.0 * (w[a] + w[b]) * np.einsum("ij,ij->i", s, r0))
            y[a] += (g * w[a])[:, None] * r0
            y[b] -= (g * w[b])[:, None] * r0
        s = y[i] - y[j]
        worst = np.abs(np.einsum("ij,ij->i", s, s) / d ** 2 - 1.0).max()         # (|s|^2 / d^2 - 1 = 2 (|s| / d - 1))
        since = 0 if worst < best else since + 1
        if worst < best:
            best, kept = worst, y.copy()
        if best <= 2.0 * tol:
            break
        if since >= 50:
            # four atoms that share a centre disturb one another at the rounding of their coordinates (ulp(d) / d per update):
            # a sweep then hovers between 1e-15 and 2e-15 without settling; the best sweep is the answer
            assert best <= 4.0 * tol, "SHAKE stalls at a residual of %.3e" % (0.5 * best)
            break
    else:
        raise AssertionError("SHAKE did not converge: residual %.3e" % (0.5 * worst))
    y = kept
    return y + origin


def rattle(x, v, pairs, mass, tol=1e-16, max_iter=5000):
    """v + sum_k mu_k (x_i - x_j) / m_i with no relative velocity along any pair, by sweeps over the pairs; stops when every
    |(v_i - v_j) . (x_i - x_j)| is within tol |v| d (|v|: the larger speed of the two going in) or no longer shrinks"""
    i, j, d, colours, root = _plan(pairs, len(x))
    x = np.asarray(x, dtype=np.float64)
    y = x - x[root]
    u = np.array(v, dtype=np.float64)
    w = 1.0 / np.asarray(mass, dtype=np.float64)
    speed = np.linalg.norm(u, axis=1)
    speed = np.maximum(speed[i], speed[j]) + 1e-300
    best, since = np.inf, 0
    for sweep in range(max_iter):
        worst = 0.0
        for c in colours:
            a, b = i[c], j[c]
            r, dv = y[a] - y[b], u[a] - u[b]
            rv, rr = np.einsum("ij,ij->i", r, dv), np.einsum("ij,ij->i", r, r)
            worst = max(worst, (np.abs(rv) / (np.sqrt(rr) * speed[c])).max())
            g = -rv / ((w[a] + w[b]) * rr)
            u[a] += (g * w[a])[:, None] * r
            u[b] -= (g * w[b])[:, None] * r
        if worst <= tol:
            break
        since = 0 if worst < best else since + 1
        best = min(best, worst)
        if since >= 20:
            assert best <= 1e-15, "RATTLE stalls at a residual of %.3e" % best
            break
    else:
        raise AssertionError("RATTLE did not converge: residual %.3e" % worst)
    return u


def bond_velocities(x, v, pairs):
    """(P,): |(v_i - v_j) . (x_i - x_j)| / (|v| d) per pair, |v| the larger speed of the two"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 3)
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    speed = np.linalg.norm(v, axis=1)
    r, dv = x[i] - x[j], v[i] - v[j]
    return np.abs(np.einsum("ij,ij->i", r, dv)) / (np.linalg.norm(r, axis=1) * (np.maximum(speed[i], speed[j]) + 1e-300))


def unwrap(pos, pairs, lengths, periodic=(1, 1, 1)):
    """pos with the second atom of every pair moved to its minimum image (on the periodic axes only) from the first, pairs taken
    in order (a star's centre comes first in each of its pairs; a triangle's third bond then changes nothing)"""
    x, ln = np.array(pos, dtype=np.float64), np.asarray(lengths, dtype=np.float64) * np.asarray(periodic, dtype=bool)
    div = np.where(ln > 0.0, ln, 1.0)
    for a, b, _ in np.asarray(pairs, dtype=np.float64).reshape(-1, 3):
        a, b = int(a), int(b)
        d = x[b] - x[a]
        x[b] = x[a] + d - ln * np.rint(d / div)
    return x


def constrained_verlet(pos, vel, force, nsteps, dt, pairs, mass, langevin=None, observe=None):
    """settle_ref.constrained_verlet over a list of pairs: (a) x0 is remembered, (b) half kick [, Langevin O step] and drift, (c)
    SHAKE and v += (x_constrained - x_unconstrained) / dt, (d) force(x, s) and half kick, (e) RATTLE.  force(x, k) -> (N, 3): k = 0
    for the starting positions.  pos unwrapped and on the constraints, vel without bond components.  Returns (x, v)."""
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
        xc = shake(x0, x, pairs, mass)
        v += (xc - x) / dt
        x = xc
        f = force(x, s)
        v += 0.5 * dt * im * f
        v = rattle(x, v, pairs, mass)
        if observe is not None:
            observe(s, x, v)
    return x, v


# ---------------------------------------------------------------- the box the GPU tests share
N_CLUSTERS, N_WATER, N_FREE = 300, 60, 100
LENGTHS, LO = np.array([9.0, 9.6, 10.5]), np.array([-1.0, 0.5, 2.0])
RC, RS, SKIN, DT = sr.RC, sr.RS, sr.SKIN, sr.DT                 # every side >= 2 (rc + skin) = 5.8
MASS_SETS = ((12.0, 1.008), (14.0, 1.008), (1.0, 19.0))         # (centre, satellite); the last inverted
D_RANGE = (0.28, 0.40)
FREE_MASS = 10.0
TETRAHEDRON = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0]]) / np.sqrt(3.0)
_CACHE = {}


def mixed_box(seed=23, temperature=1.0):
    """300 star clusters (100 each of 2, 3 and 4 atoms, the mass sets in turn, distances drawn from D_RANGE per bond, satellites
    along the corners of a randomly turned tetrahedron), 60 rigid waters of settle_ref's geometry and masses, 100 free atoms:
    1180 atoms, the 460 centres on a jittered 8 x 8 x 8 lattice in shuffled order, every atom wrapped into the box on its own
    (groups straddle box faces and cell faces), velocities drawn at `temperature` and projected by rattle().  Atom order:
    clusters (centre, satellites), waters (apex, a, b), free atoms.
    dict(pos (wrapped), unwrapped, vel, mass, atoms, charges, clusters, dist, mol, geom, excl, pairs_h, pairs_w, pairs);
    computed once per process."""
    key = (seed, temperature)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        n_sites = N_CLUSTERS + N_WATER + N_FREE
        grid = np.array([(i, j, k) for i in range(8) for j in range(8) for k in range(8)], dtype=np.float64)
        grid = grid[rng.permutation(len(grid))[:n_sites]]
        centres = LO + (grid + 0.5 + 0.2 * (rng.random((n_sites, 3)) - 0.5)) / 8.0 * LENGTHS
        x, mass, hs, eps, q, clusters, dist, excl = [], [], [], [], [], [], [], []
        rot = sr.random_rotations(rng, N_CLUSTERS + N_WATER)
        for c in range(N_CLUSTERS):
            nsat, (mc, ms) = 1 + c % 3, MASS_SETS[(c // 3) % 3]
            d = rng.uniform(*D_RANGE, size=3)
            first = len(x)
            x.append(centres[c]); mass.append(mc); hs.append(0.5); eps.append(2.0); q.append(-0.3 * nsat)
            for k in range(nsat):
                x.append(centres[c] + d[k] * rot[c] @ TETRAHEDRON[k]); mass.append(ms); hs.append(0.2); eps.append(1.0); q.append(0.3)
            ids = list(range(first, first + 1 + nsat))
            clusters.append(ids + [-1] * (3 - nsat)); dist.append([d[k] if k < nsat else 0.0 for k in range(3)])
            excl += [(a, b) for a in ids for b in ids if a < b]
        mol = []
        for m in range(N_WATER):
            first = len(x)
            for k, site in enumerate(sr.triangle(sr.D_LEG, sr.D_BASE)):
                x.append(centres[N_CLUSTERS + m] + rot[N_CLUSTERS + m] @ site)
                mass.append(sr.MASSES[k]); hs.append(sr.HALF_SIGMA[k]); eps.append(sr.TWICE_SQRT_EPS[k]); q.append(sr.CHARGES[k])
            mol.append([first, first + 1, first + 2])
            excl += [(first, first + 1), (first, first + 2), (first + 1, first + 2)]
        for a in range(N_FREE):
            x.append(centres[N_CLUSTERS + N_WATER + a]); mass.append(FREE_MASS); hs.append(0.5); eps.append(2.0); q.append(0.0)
        x, mass = np.array(x), np.array(mass)
        clusters, dist, mol = np.array(clusters, dtype=np.int64), np.array(dist), np.array(mol, dtype=np.int64)
        geom = np.tile([sr.D_LEG, sr.D_BASE], (N_WATER, 1))
        pairs_h, pairs_w = cluster_pairs(clusters, dist), triangle_pairs(mol, geom)
        pairs = np.concatenate([pairs_h, pairs_w])
        v = rng.normal(size=x.shape) * np.sqrt(temperature / mass)[:, None]
        v -= (mass[:, None] * v).sum(axis=0) / mass.sum()
        v = rattle(x, v, pairs, mass)
        atoms = np.zeros(len(x), dtype=np.dtype([("half_sigma", np.float32), ("twice_sqrt_eps", np.float32)]))
        atoms["half_sigma"], atoms["twice_sqrt_eps"] = hs, eps
        _CACHE[key] = dict(pos=LO + np.mod(x - LO, LENGTHS), unwrapped=x, vel=v, mass=mass, atoms=atoms, charges=np.array(q),
                           clusters=clusters, dist=dist, mol=mol, geom=geom, excl=np.array(excl, dtype=np.int64), pairs_h=pairs_h,
                           pairs_w=pairs_w, pairs=pairs)
    return {k: np.array(v) for k, v in _CACHE[key].items()}


def reference_drift(nsteps=400, every=20):
    """max |E(t) - E(0)| of constrained_verlet on mixed_box() with the all-pairs forces of ortho_ref, sampled every `every` steps"""
    from . import ortho_ref as oref
    B = mixed_box()
    total = lambda x: oref.total(x, LO, LENGTHS, [1, 1, 1], RC, RS, B["atoms"], excl=B["excl"])
    energy = lambda x, v: total(x)["e"].sum() + 0.5 * (B["mass"][:, None] * v * v).sum()
    e0, seen = energy(B["unwrapped"], B["vel"]), []

    def observe(s, x, v):
        if s % every == 0:
            seen.append(abs(energy(x, v) - e0))
    constrained_verlet(B["unwrapped"], B["vel"], lambda x, k: total(x)["f"], nsteps, DT, B["pairs"], B["mass"], observe=observe)
    return max(seen), e0


if __name__ == "__main__":
    drift, e0 = reference_drift()
    print("reference: max |E(t) - E(0)| over 400 steps of dt = %g, sampled every 20: %.6e (E(0) = %.6f)" % (DT, drift, e0))
