"""numpy fp64 yardstick of virtual interaction sites (include/emdee_hip.h: emdee_md_set_vsites): placement, force spreading, the
four-site water box the GPU tests share, and the step of settle_ref.constrained_verlet around a force callback that places the
sites, asks for the forces on all atoms and spreads them.  Plain numpy; it never calls the library (the GPU tests hand it a
callback that does).

atoms: (n, 4) ids {site, a, b, c}, c = -1 for a two-parent site; weights: (n, 2) {w_b, w_c} (w_c ignored where c = -1).

Run as a program (python -m tests.helpers.vsite_ref) it prints the energy drift of the reference on the box of
tests/test_gpu_vsites.py, the constant REFERENCE_DRIFT of that file."""
import numpy as np

from . import settle_ref as sr

W_SITE = 0.13                                            # w_b = w_c of the shared box
_CACHE = {}


def _image(d, lengths, periodic):
    ln, per = np.asarray(lengths, dtype=np.float64), np.asarray(periodic, dtype=bool)
    return np.where(per, d - ln * np.rint(d / ln), d)


def parent_weights(atoms, weights):
    """(n, 3): the weights of a, b and c -- 1 - w_b - w_c, w_b, w_c, with w_c = 0 where c = -1"""
    atoms, w = np.asarray(atoms, dtype=np.int64).reshape(-1, 4), np.array(weights, dtype=np.float64).reshape(-1, 2)
    w[atoms[:, 3] < 0, 1] = 0.0
    return np.stack([1.0 - w[:, 0] - w[:, 1], w[:, 0], w[:, 1]], axis=1)


def place(x, atoms, weights, lengths, periodic=(1, 1, 1)):
    """(n, 3): x_a + w_b mi(x_b - x_a) + w_c mi(x_c - x_a), the sites in the frame of their a"""
    x, atoms = np.asarray(x, dtype=np.float64), np.asarray(atoms, dtype=np.int64).reshape(-1, 4)
    w = parent_weights(atoms, weights)
    c = np.where(atoms[:, 3] >= 0, atoms[:, 3], atoms[:, 1])
    xa = x[atoms[:, 1]]
    return xa + (w[:, 1:2] * _image(x[atoms[:, 2]] - xa, lengths, periodic) + w[:, 2:3] * _image(x[c] - xa, lengths, periodic))


def spread(f, atoms, weights):
    """f with every site's force handed to its parents (entry by entry, in table order) and the sites' forces zeroed"""
    f, atoms = np.asarray(f, dtype=np.float64), np.asarray(atoms, dtype=np.int64).reshape(-1, 4)
    w, out = parent_weights(atoms, weights), np.array(f, dtype=np.float64)
    for s in range(atoms.shape[0]):
        for k in range(3):
            if atoms[s, 1 + k] >= 0:
                out[atoms[s, 1 + k]] += w[s, k] * f[atoms[s, 0]]
    out[atoms[:, 0]] = 0.0
    return out


def parent_list(atoms, weights):
    """the distinct parents ascending, start (CSR), and per parent its (entry, weight) pairs in table order"""
    atoms, w = np.asarray(atoms, dtype=np.int64).reshape(-1, 4), parent_weights(atoms, weights)
    parents = sorted(set(int(g) for g in atoms[:, 1:].ravel() if g >= 0))
    rows = {p: [] for p in parents}
    for s in range(atoms.shape[0]):
        for k in range(3):
            if atoms[s, 1 + k] >= 0:
                rows[int(atoms[s, 1 + k])].append((s, w[s, k]))
    start = np.concatenate([[0], np.cumsum([len(rows[p]) for p in parents])]).astype(int)
    return parents, start.tolist(), [e for p in parents for e in rows[p]]


# ---------------------------------------------------------------- the box the GPU tests share
def four_site_box():
    """settle_ref.water_box() with a fourth site per molecule (ids 450 .. 599, after the 450 atoms of the waters): massless
    (mass inf, inv_mass 0), epsilon = 0, the apex charge moved to it, on the bisector at w_b = w_c = 0.13; exclusions over all six
    pairs of a molecule.  The sites of pos / unwrapped are placed; vel of the sites is 0.  dict of settle_ref.water_box's keys
    plus inv_mass, vs_atoms, vs_weights, sites, real (ids of the atoms with mass)."""
    if "box" not in _CACHE:
        B = sr.water_box()
        n = B["mol"].shape[0]
        sites = np.arange(3 * n, 4 * n, dtype=np.int64)
        vs_atoms = np.concatenate([sites[:, None], B["mol"]], axis=1)
        vs_weights = np.full((n, 2), W_SITE)
        xs = place(B["unwrapped"], vs_atoms, vs_weights, sr.LENGTHS)
        unwrapped = np.concatenate([B["unwrapped"], xs])
        atoms = np.concatenate([B["atoms"], np.zeros(n, dtype=B["atoms"].dtype)])
        atoms["half_sigma"][3 * n:] = 0.1
        charges = np.concatenate([B["charges"], B["charges"][B["mol"][:, 0]]])
        charges[B["mol"][:, 0]] = 0.0
        four = np.concatenate([B["mol"], sites[:, None]], axis=1)
        excl = np.concatenate([four[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
        mass = np.concatenate([B["mass"], np.full(n, np.inf)])
        _CACHE["box"] = dict(pos=sr.LO + np.mod(unwrapped - sr.LO, sr.LENGTHS), unwrapped=unwrapped, vel=np.concatenate([B["vel"], np.zeros((n, 3))]),
                             mol=B["mol"], geom=B["geom"], mass=mass, inv_mass=1.0 / mass, atoms=atoms, excl=excl, charges=charges,
                             vs_atoms=vs_atoms, vs_weights=vs_weights, sites=sites, real=np.arange(3 * n))
    return {k: np.array(v) for k, v in _CACHE["box"].items()}


def constrained_verlet(pos, vel, raw_force, nsteps, dt, B, langevin=None, observe=None):
    """settle_ref.constrained_verlet for a box with sites: before every force evaluation the sites of x are placed (in x itself,
    so the trajectory carries them), raw_force(x, k) -> (N, 3) gives the forces on all atoms, sites included, and they are spread.
    The sites have mass inf: kick, drift and noise leave them alone."""
    def force(x, k):
        x[B["sites"]] = place(x, B["vs_atoms"], B["vs_weights"], sr.LENGTHS)
        return spread(raw_force(x, k), B["vs_atoms"], B["vs_weights"])
    return sr.constrained_verlet(pos, vel, force, nsteps, dt, B["mol"], B["geom"], B["mass"], langevin=langevin, observe=observe)


def kinetic(B, v):
    return 0.5 * (B["mass"][B["real"], None] * v[B["real"]] ** 2).sum()


def reference_drift(nsteps=400, every=20):
    """max |E(t) - E(0)| of constrained_verlet on four_site_box() with the all-pairs Lennard-Jones and reaction-field forces of
    ortho_ref (coulomb_k = 1, eps_rf = inf), sampled every `every` steps"""
    from . import ortho_ref as oref
    B = four_site_box()
    total = lambda x: oref.total(x, sr.LO, sr.LENGTHS, [1, 1, 1], sr.RC, sr.RS, B["atoms"], excl=B["excl"], charges=B["charges"], coulomb_k=1.0)
    energy = lambda x, v: total(x)["e"].sum() + kinetic(B, v)
    e0, seen = energy(B["unwrapped"], B["vel"]), []

    def observe(s, x, v):
        if s % every == 0:
            seen.append(abs(energy(x, v) - e0))
    constrained_verlet(B["unwrapped"], B["vel"], lambda x, k: total(x)["f"], nsteps, sr.DT, B, observe=observe)
    return max(seen), e0


if __name__ == "__main__":
    drift, e0 = reference_drift()
    print("reference: max |E(t) - E(0)| over 400 steps of dt = %g, sampled every 20: %.6e (E(0) = %.6f)" % (sr.DT, drift, e0))
