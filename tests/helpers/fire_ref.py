"""numpy fp64 yardstick of energy minimisation (include/emdee_hip.h: emdee_md_minimize): classic FIRE (Bitzek et
al., Phys. Rev. Lett. 97, 170201 (2006)) around the closed velocity-Verlet step, with masses and constraints.  Forces come from
a callback (lj() wraps ortho_ref.total), constraints from shake_ref.shake / rattle over a list of pairs (triangle_pairs /
cluster_pairs), and the constrained force G is rattle() applied to w F.  Plain numpy; it never calls the library.

One iteration, with the host scalars dt, alpha, n_pos and v_max (the bound on the largest speed now):
  1. t = fire_cap(dt, v_max, max |w_i F_i|, max_step)
  2. x0 = x ; v += t/2 w F ; x += t v ; x <- shake(x0, x), v += (x_constrained - x) / t ; F, E = force(x) ; v += t/2 w F ;
     v <- rattle(x, v)
  3. G = rattle(x, w F) / w on the atoms of the pairs, F elsewhere
  4. P = sum G . v, vv = sum v . v, gg = sum G . G, g_max = max |G_i|
  5. g_max <= f_tol: stop, converged
  6. P > 0: v <- (1 - alpha) v + alpha sqrt(vv / gg) G, v <- rattle(x, v), v_max <- (1 - alpha) max |v_i| + alpha sqrt(vv / gg)
     g_max (no speed exceeds it), and if ++n_pos > N_MIN: dt <- min(F_INC dt, dt_max), alpha <- F_ALPHA alpha;
     else: v <- 0, v_max <- 0, dt <- F_DEC dt, alpha <- ALPHA0, n_pos <- 0
Iteration 0 is steps 3 to 5 at the entry positions with v = 0.  Positions are unwrapped (a group's atoms differ by the group's
own vectors) and stay so."""
import numpy as np

from . import ortho_ref as oref
from . import shake_ref as hr

N_MIN, F_INC, F_DEC, ALPHA0, F_ALPHA = 5, 1.1, 0.5, 0.1, 0.99
# shake_ref.rattle sweeps until the bond-relative velocities are within tol |v| d.  Its default, 1e-16, is below what the sweeps
# reach on w F, whose components along a bond nearly cancel between the two ends (on clashing molecules they stall near 5e-15); 2e-14 is
# above that floor and orders below anything the tests ask of G.
RATTLE_TOL = 2e-14


def fire_cap(dt, vmax, amax, max_step):
    """the largest t <= dt with t vmax + t^2 amax / 2 <= max_step"""
    if dt * vmax + 0.5 * dt * dt * amax <= max_step:
        return dt
    t = 2.0 * max_step / (vmax + np.sqrt(vmax * vmax + 2.0 * amax * max_step))
    return t if t < dt else dt


class State:
    def __init__(self, dt_start, dt_max):
        self.dt, self.alpha, self.dt_max, self.n_pos = float(dt_start), ALPHA0, float(dt_max), 0


def fire_update(s, P):
    """step 6 on the scalars; True: mix (with the alpha held before the call), False: zero"""
    if P > 0.0:
        s.n_pos += 1
        if s.n_pos > N_MIN:
            s.dt = min(F_INC * s.dt, s.dt_max)
            s.alpha *= F_ALPHA
        return True
    s.dt *= F_DEC
    s.alpha = ALPHA0
    s.n_pos = 0
    return False


def constrained_force(x, f, pairs, mass):
    """G: f with the components along the constraints removed (rattle on w f); f itself on atoms outside the pairs"""
    if pairs is None or len(pairs) == 0:
        return f
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 3)
    g = np.array(f, dtype=np.float64)
    a = hr.rattle(x, f / mass[:, None], pairs, mass, tol=RATTLE_TOL) * mass[:, None]
    members = np.unique(pairs[:, :2].astype(np.int64))
    g[members] = a[members]
    return g


def lj(lo, lengths, periodic, rc, rs, atoms, **kw):
    """force(x) -> (F (N, 3), potential energy) from ortho_ref.total (all pairs; kw: terms, excl, p14, charges, ...)"""
    def force(x):
        out = oref.total(x, lo, lengths, periodic, rc, rs, atoms, **kw)
        return out["f"], out["e"].sum()
    return force


def minimize(pos, force, mass, max_iter, f_tol, dt_start, dt_max, max_step, pairs=None, keep=False):
    """dict(x, converged, iterations, energy0, energy, g_max, dt, forces, records, moved): records[k] = (t, dt, alpha, n_pos, P,
    energy, g_max) of iteration k (dt, alpha, n_pos after its update; t = 0 for iteration 0); moved = the largest distance of an
    atom from its entry position seen at any iteration; keep: xs = the positions after every iteration (from 0) as well"""
    x = np.array(pos, dtype=np.float64)
    start = x.copy()
    mass = np.asarray(mass, dtype=np.float64)
    w = (1.0 / mass)[:, None]
    constrained = pairs is not None and len(pairs) > 0
    s = State(dt_start, dt_max)
    v = np.zeros_like(x)
    f, e = force(x)
    energy0 = e
    records, xs, iterations, converged, vmax, t, moved = [], [], 0, False, 0.0, 0.0, 0.0
    while True:
        G = constrained_force(x, f, pairs, mass)
        P, vv, gg = (G * v).sum(), (v * v).sum(), (G * G).sum()
        g_max = np.sqrt((G * G).sum(axis=1).max())
        converged = bool(g_max <= f_tol)
        if not converged and iterations > 0:
            alpha = s.alpha
            if fire_update(s, P):
                c_g = alpha * np.sqrt(vv / gg)
                speed = np.sqrt((v * v).sum(axis=1).max())
                v = (1.0 - alpha) * v + c_g * G
                if constrained:
                    v = hr.rattle(x, v, pairs, mass, tol=RATTLE_TOL)
                vmax = (1.0 - alpha) * speed + c_g * g_max
            else:
                v = np.zeros_like(x)
                vmax = 0.0
        records.append((t, s.dt, s.alpha, s.n_pos, P, e, g_max))
        if keep:
            xs.append(x.copy())
        if converged or iterations >= max_iter:
            break
        amax = np.sqrt(((w * f) ** 2).sum(axis=1).max())
        t = fire_cap(s.dt, vmax, amax, max_step)
        x0 = x.copy()
        v = v + 0.5 * t * w * f
        x = x + t * v
        if constrained:
            xc = hr.shake(x0, x, pairs, mass)
            v = v + (xc - x) / t
            x = xc
        f, e = force(x)
        v = v + 0.5 * t * w * f
        if constrained:
            v = hr.rattle(x, v, pairs, mass, tol=RATTLE_TOL)
        iterations += 1
        moved = max(moved, np.sqrt(((x - start) ** 2).sum(axis=1).max()))
    return dict(x=x, converged=converged, iterations=iterations, energy0=energy0, energy=e, g_max=g_max, dt=s.dt, forces=f, records=records,
                moved=moved, xs=xs)


# ---------------------------------------------------------------- the boxes the GPU tests share
# Reduced Lennard-Jones units, orthorhombic boxes with unequal sides at lo != 0, every side >= 2 (rc + skin).
LO = np.array([-1.0, 0.5, 2.0])
PARAMS = dict(dt_start=0.002, dt_max=0.02, max_step=0.1)
_CACHE = {}


def _lj_atoms(n):
    atoms = np.zeros(n, dtype=np.dtype([("half_sigma", np.float32), ("twice_sqrt_eps", np.float32)]))
    atoms["half_sigma"], atoms["twice_sqrt_eps"] = 0.5, 2.0
    return atoms


def _fcc(cells, a, rng, jitter):
    base = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.5, 0.0, 0.5], [0.0, 0.5, 0.5]])
    x = np.array([(np.array([i, j, k]) + c) * a for i in range(cells[0]) for j in range(cells[1]) for k in range(cells[2]) for c in base])
    u = rng.normal(size=x.shape)
    u *= (jitter * rng.random((len(x), 1))) / np.linalg.norm(u, axis=1, keepdims=True)
    return x + LO + 0.25 * a + u, a * np.array(cells, dtype=np.float64)


def fcc_box(seed=31):
    """108 atoms on 4 x 3 x 3 fcc cells of sides (1.60, 1.64, 1.68), each displaced by up to 0.05 sigma, masses in [1, 4];
    rc = 1.6, rs = 1.3, skin = 0.3.  dict(pos, lengths, mass, atoms, rc, rs, skin)"""
    if ("fcc", seed) not in _CACHE:
        rng = np.random.default_rng(seed)
        x, lengths = _fcc((4, 3, 3), np.array([1.60, 1.64, 1.68]), rng, 0.05)
        _CACHE[("fcc", seed)] = dict(pos=x, lengths=lengths, mass=rng.uniform(1.0, 4.0, len(x)), atoms=_lj_atoms(len(x)), rc=1.6, rs=1.3, skin=0.3)
    return {k: np.array(v) for k, v in _CACHE[("fcc", seed)].items()}


def overlap_box(seed=32):
    """256 atoms: 4 x 4 x 4 fcc cells of sides (1.70, 1.72, 1.68) (density 0.81) displaced by up to 0.3 sigma, then atom 0 moved
    onto the line to its nearest neighbour, 0.6 sigma from it; masses 1; rc = 2.5, rs = 2.0, skin = 0.3.  Adds `partner`."""
    if ("overlap", seed) not in _CACHE:
        rng = np.random.default_rng(seed)
        x, lengths = _fcc((4, 4, 4), np.array([1.70, 1.72, 1.68]), rng, 0.3)
        d = x[1:] - x[0]
        d -= lengths * np.rint(d / lengths)
        j = int(np.argmin(np.linalg.norm(d, axis=1)))
        x[0] = x[1 + j] - d[j] - 0.6 * (-d[j]) / np.linalg.norm(d[j]) + d[j]          # x[0] = x_j - 0.6 (unit vector from 0 to j)
        _CACHE[("overlap", seed)] = dict(pos=x, lengths=lengths, mass=np.ones(len(x)), atoms=_lj_atoms(len(x)), rc=2.5, rs=2.0, skin=0.3,
                                         partner=np.array(1 + j))
    return {k: np.array(v) for k, v in _CACHE[("overlap", seed)].items()}


def dilute_box(seed=33):
    """80 atoms placed at random, none within 0.8 sigma of another, in a box of sides (6.0, 6.4, 6.9): density 0.30; masses 1;
    rc = 2.5, rs = 2.0, skin = 0.3"""
    if ("dilute", seed) not in _CACHE:
        rng = np.random.default_rng(seed)
        lengths, x = np.array([6.0, 6.4, 6.9]), []
        while len(x) < 80:
            c = LO + rng.random(3) * lengths
            if x:
                d = np.array(x) - c
                d -= lengths * np.rint(d / lengths)
                if np.linalg.norm(d, axis=1).min() < 0.8:
                    continue
            x.append(c)
        _CACHE[("dilute", seed)] = dict(pos=np.array(x), lengths=lengths, mass=np.ones(80), atoms=_lj_atoms(80), rc=2.5, rs=2.0, skin=0.3)
    return {k: np.array(v) for k, v in _CACHE[("dilute", seed)].items()}


def clashing_water_box(seed=34):
    """settle_ref.water_box() with every molecule moved by up to 0.25 and turned at random about its apex: neighbours clash, the
    geometry is intact.  settle_ref's dict with pos (wrapped) and unwrapped replaced."""
    from . import settle_ref as sr
    if ("water", seed) not in _CACHE:
        B = sr.water_box()
        rng = np.random.default_rng(seed)
        n = len(B["mol"])
        shift = rng.normal(size=(n, 3))
        shift *= (0.25 * rng.random((n, 1))) / np.linalg.norm(shift, axis=1, keepdims=True)
        sites = np.einsum("nij,kj->nki", sr.random_rotations(rng, n), sr.triangle(sr.D_LEG, sr.D_BASE))
        x = ((B["unwrapped"][B["mol"][:, 0]] + shift)[:, None, :] + sites).reshape(-1, 3)
        B["unwrapped"], B["pos"] = x, sr.LO + np.mod(x - sr.LO, sr.LENGTHS)
        _CACHE[("water", seed)] = B
    return {k: np.array(v) for k, v in _CACHE[("water", seed)].items()}


def closest_pair(x, lengths, skip=None):
    """the smallest minimum-image distance between two atoms (skip: (P, 2) pairs left out)"""
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    d -= lengths * np.rint(d / lengths)
    r = np.linalg.norm(d, axis=2)
    r[np.diag_indices(len(x))] = np.inf
    if skip is not None and len(skip):
        s = np.asarray(skip, dtype=np.int64).reshape(-1, 2)
        r[s[:, 0], s[:, 1]] = r[s[:, 1], s[:, 0]] = np.inf
    return r.min()
