"""Host yardstick of the integrators on orthorhombic boxes with per-axis geometry (emdee_md_create: lo[3], len[3],
periodic[3]; emdee_dd_create: len[3]).  Plain numpy fp64; it never calls the library.

Pair terms (include/emdee_hip.h, oracle/: switched Lennard-Jones, CUTOFF semantics, Lorentz-Berthelot mixing carried by the
LJAtom fields half_sigma and twice_sqrt_eps):

    sigma = hs_i + hs_j,  4 eps = te_i te_j,  s6 = (sigma^2 / r^2)^3
    E0 = 4 eps s6 (s6 - 1),  W0 = -r dE0/dr = 24 eps s6 (2 s6 - 1)
    x = (r^2 - rs^2) / (rc^2 - rs^2) clamped to [0, 1],  g = 1 + x^3 (15 x - 6 x^2 - 10)
    E = E0 g,  W = W0 g + E0 60 x^2 (1 - x)^2 r^2 / (rc^2 - rs^2)           for r^2 < rc^2, else nothing

(tests/helpers/virial_tensor_ref.py: pair_energy_virial), plus, with charges, the reaction field of
tests/helpers/coulomb_ref.py.  F_i = (W / r^2) d with d = r_i - r_j the minimum image on the PERIODIC axes, each with its own
length; half of E, W and (W / r^2) d (x) d to either atom; tensor order (xx, yy, zz, xy, xz, yz).  Excluded pairs contribute
nothing; 1-4 pairs lj14scale (coulomb14scale) times their terms.  Pairs come from virial_tensor_ref.pairs_in_range: all of
them, or -- sampled mode -- the whole rows of a few atoms.

`lo` does not enter a pair term (only differences do); it is taken so that callers pass the box they gave the engine, and
open axes are checked against it: an atom outside the walls of an open axis is a mistake in the test."""
import numpy as np

from . import bonded_ref as br
from . import coulomb_ref as cr
from . import virial_tensor_ref as vt

OPEN = 1e300       # the length that stands for an open axis in bonded_ref / coulomb_ref: rint(d / OPEN) = 0


def lj_fields(atoms):
    a = np.asarray(atoms)
    return a["half_sigma"].astype(np.float32), a["twice_sqrt_eps"].astype(np.float32)


def effective_lengths(lengths, periodic):
    """per-axis lengths for the minimum image of bonded_ref and coulomb_ref: the box length on a periodic axis, OPEN otherwise"""
    return np.where(np.asarray(periodic, dtype=bool), np.asarray(lengths, dtype=np.float64), OPEN)


def check_inside(pos, lo, lengths, periodic):
    for a in range(3):
        if not periodic[a]:
            assert (pos[:, a] > lo[a]).all() and (pos[:, a] < lo[a] + lengths[a]).all(), "atoms beyond the walls of open axis %d" % a


def cycle(v, k):
    """the per-axis quantity v (last dimension 3) with its axes cycled k times: new axis a is old axis (a + k) % 3"""
    v = np.asarray(v)
    return v[..., [(a + k) % 3 for a in range(3)]]


def cycle_tensor(t, k):
    """(N, 6) tensors (xx, yy, zz, xy, xz, yz) under the same cycling"""
    p = [(a + k) % 3 for a in range(3)]
    full = np.empty(t.shape[:-1] + (3, 3))
    for c, (a, b) in enumerate(vt.COMPONENTS):
        full[..., a, b] = full[..., b, a] = t[..., c]
    return np.stack([full[..., p[a], p[b]] for a, b in vt.COMPONENTS], axis=-1)


def _scales(i, j, N, excl, p14, s14):
    """per-pair factor: 0 for excluded pairs, s14 for 1-4 pairs, 1 otherwise"""
    scale = np.ones(i.shape[0])
    key = vt._pair_key(i, j, N)
    if excl is not None and len(excl):
        e = np.asarray(excl, dtype=np.int64).reshape(-1, 2)
        scale[np.isin(key, vt._pair_key(e[:, 0], e[:, 1], N))] = 0.0
    if p14 is not None and len(p14):
        p = np.asarray(p14, dtype=np.int64).reshape(-1, 2)
        scale[np.isin(key, vt._pair_key(p[:, 0], p[:, 1], N))] = s14
    return scale


def nonbonded(pos, lo, lengths, periodic, rc, rs, atoms, excl=None, p14=None, lj14scale=1.0, rows=None,
              charges=None, coulomb_k=1.0, eps_rf=np.inf, coulomb14scale=1.0, lj=True, oracle=None):
    """dict(f (N, 3), e (N,), w (N,), t (N, 6)) of the pair terms.  rows: sampled mode -- only these atoms' entries are
    filled (whole: every partner of theirs is visited), the others stay zero.  charges: adds the reaction field; lj=False
    leaves the Lennard-Jones part out (the Coulomb part alone).  oracle: on a cubic periodic box the candidate pairs come from
    the oracle's cell list in place of the N^2 table (virial_tensor_ref.pairs_in_range); the terms are summed here all the same."""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    check_inside(pos, lo, lengths, periodic)
    i, j, d = vt.pairs_in_range(pos, lengths, periodic, rc, oracle=oracle, rows=rows, margin=0.0)
    r2 = np.einsum("ij,ij->i", d, d)
    E, W = np.zeros(r2.shape[0]), np.zeros(r2.shape[0])
    if lj:
        hs, te = lj_fields(atoms)
        E0, W0 = vt.pair_energy_virial(r2, rc, rs, hs[i], te[i], hs[j], te[j])
        s = _scales(i, j, N, excl, p14, lj14scale)
        E, W = E + s * E0, W + s * W0
    if charges is not None:
        q = np.asarray(charges, dtype=np.float64)
        U, Wc = cr.pair_energy_virial(np.sqrt(r2), coulomb_k * q[i] * q[j], rc, eps_rf)
        s = _scales(i, j, N, excl, p14, coulomb14scale)
        E, W = E + s * U, W + s * Wc
    fv = (W / r2)[:, None] * d
    tv = 0.5 * np.stack([fv[:, a] * d[:, b] for a, b in vt.COMPONENTS], axis=1)
    f, e, w, t = np.zeros((N, 3)), np.zeros(N), np.zeros(N), np.zeros((N, 6))
    ends = ((i, 1.0),) if rows is not None else ((i, 1.0), (j, -1.0))
    for a, sign in ends:
        for c in range(3):
            f[:, c] += sign * np.bincount(a, fv[:, c], minlength=N)
        e += np.bincount(a, 0.5 * E, minlength=N)
        w += np.bincount(a, 0.5 * W, minlength=N)
        for c in range(6):
            t[:, c] += np.bincount(a, tv[:, c], minlength=N)
    return dict(f=f, e=e, w=w, t=t)


def bonded(pos, lengths, periodic, terms):
    """bonded_ref.bonded with per-axis lengths (chained minimum image on the periodic axes only) as the same dict"""
    f, e, w, t = br.bonded(pos, effective_lengths(lengths, periodic), terms)
    return dict(f=f, e=e, w=w, t=t)


def total(pos, lo, lengths, periodic, rc, rs, atoms, terms=None, **kw):
    """pair terms plus bonded terms"""
    out = nonbonded(pos, lo, lengths, periodic, rc, rs, atoms, **kw)
    if terms:
        b = bonded(pos, lengths, periodic, terms)
        out = {k: out[k] + b[k] for k in out}
    return out


def energy(pos, lo, lengths, periodic, rc, rs, atoms, terms=None, **kw):
    return total(pos, lo, lengths, periodic, rc, rs, atoms, terms, **kw)["e"].sum()


def verlet(pos, vel, force, nsteps, dt, inv_mass=None, langevin=None):
    """Velocity Verlet, v += (dt / 2m) f ; x += dt v ; f = force(x) ; v += (dt / 2m) f, positions left unwrapped
    (tests/test_gpu_bonded.py: _numpy_verlet, with masses).  langevin = (gamma, temperature, normals): between the first
    kick and the drift of step k (from 0), v = c1 v + c2 sqrt(T / m) normals(k), c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2)
    (include/emdee_hip.h: emdee_md_set_langevin); normals(k) is the (N, 3) array of the step's N(0, 1) numbers."""
    x, v = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    im = 1.0 if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)[:, None]
    f = force(x)
    for k in range(nsteps):
        v += 0.5 * dt * im * f
        if langevin is not None:
            gamma, temperature, normals = langevin
            c1 = np.exp(-gamma * dt)
            v = c1 * v + np.sqrt(1.0 - c1 * c1) * np.sqrt(temperature * im) * normals(k)
        x += dt * v
        f = force(x)
        v += 0.5 * dt * im * f
    return x, v


def wrapped(pos, lo, lengths, periodic):
    """positions folded into [lo, lo + len) on the periodic axes (the yardstick's pair terms do not need it: open axes must
    stay inside their walls along a trajectory, and check_inside sees the folded positions the same)"""
    pos = np.array(pos, dtype=np.float64)
    for a in range(3):
        if periodic[a]:
            pos[:, a] = lo[a] + np.mod(pos[:, a] - lo[a], lengths[a])
    return pos


def image_difference(a, b, lengths, periodic):
    """a - b up to whole box lengths on the periodic axes"""
    return vt._minimum_image(np.array(a, dtype=np.float64) - b, lengths, periodic)


def neighbour_rows(pos, lengths, periodic, rlist, rows=None):
    """the set r < rlist of every atom (or of the sampled rows) as sorted index arrays: what emdee_md_nbr_list must hold"""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    i, j, _ = vt.pairs_in_range(pos, lengths, periodic, rlist, rows=rows, margin=0.0)
    if rows is None:
        i, j = np.concatenate([i, j]), np.concatenate([j, i])
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    cut = np.searchsorted(i, np.arange(N + 1))
    which = range(N) if rows is None else rows
    return {int(r): j[cut[r]:cut[r + 1]] for r in which}


def nearest_to_radius(pos, lengths, periodic, r, rows=None):
    """min over pairs of |d^2 - r^2| / r^2: how far the configuration stays from a pair that an fp32 distance test at r
    could decide either way"""
    _, _, d = vt.pairs_in_range(np.asarray(pos, dtype=np.float64), lengths, periodic, r, rows=rows, margin=0.05 * r)
    r2 = np.einsum("ij,ij->i", d, d)
    return np.abs(r2 - r * r).min() / (r * r)
