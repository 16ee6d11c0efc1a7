"""numpy fp64 yardstick of the molecular pressure and the molecular scale over whole molecules of any size (include/emdee_hip.h:
emdee_md_set_molecules): molecular_ref.py with the (n, 3) table of triangles replaced by one molecule id per atom.  Plain numpy;
it never calls the library and was written from the header's formulas, not from csrc/molecule.hpp.

ids: (N,) integers >= -1; equal ids >= 0 form one molecule, -1 is a molecule of one.  Positions are UNWRAPPED and every molecule is
whole as the caller means it: no box length is added or taken anywhere in this file.

    M = sum_k m_k,  Y = sum_k m_k x_k / M,  V = sum_k m_k v_k / M,  d_k = x_k - Y          (k over ALL atoms of a molecule)
    W_mol^ab = W^ab - sum_mol sum_k 1/2 (d_k^a f_k^b + d_k^b f_k^a)
    K_mol^ab = K^ab - sum_mol (sum_k m_k v_k^a v_k^b - M V^a V^b)          order (xx, yy, zz, xy, xz, yz)
    scale: every atom of a molecule moves by (mu - 1) (Y - lo), its velocity gains (velocity_scale - 1) V; molecules of one and
           the box scale as barostat_ref.scale does
"""
import numpy as np

from . import barostat_ref as bref
from . import molecular_ref as mr
from . import shake_ref as hr

COMPONENTS = mr.COMPONENTS


def labels(ids):
    """(mol, n_mol, first): a dense molecule number per atom in order of first appearance (an atom at -1 gets a number of its own),
    their count, and the first (lowest) atom of every molecule"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    assert (ids >= -1).all()
    key = np.where(ids >= 0, ids, ids.max(initial=0) + 1 + np.arange(len(ids)))
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                                    # molecules by first atom
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return rank[inverse.reshape(-1)], len(first), first[order]


def centres(x, v, ids, mass):
    """(Y, V, M, d, u, mol): per molecule the centre of mass, its velocity and the mass; per atom d = x - Y and u = v - V; the
    molecule number of every atom.  Y and V are formed from differences to the molecule's first atom, so that d does not lose
    digits to a far origin."""
    x, v, m = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    mol, n_mol, first = labels(ids)
    M = np.bincount(mol, m, minlength=n_mol)
    rel, relv = x - x[first][mol], v - v[first][mol]
    c = np.stack([np.bincount(mol, m * rel[:, a], minlength=n_mol) for a in range(3)], axis=1) / M[:, None]
    cv = np.stack([np.bincount(mol, m * relv[:, a], minlength=n_mol) for a in range(3)], axis=1) / M[:, None]
    return x[first] + c, v[first] + cv, M, rel - c[mol], relv - cv[mol], mol


def corrections(x, v, f, ids, mass):
    """(cw, ck), six numbers each: what the atomic sums W and K hold beyond the molecular ones"""
    _, _, _, d, u, _ = centres(x, v, ids, mass)
    f, m = np.asarray(f, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    cw = np.array([0.5 * (d[:, a] * f[:, b] + d[:, b] * f[:, a]).sum() for a, b in COMPONENTS])
    ck = np.array([(m * u[:, a] * u[:, b]).sum() for a, b in COMPONENTS])          # (= sum m v v - M V V, without the cancellation)
    return cw, ck


def molecular_sums(x, v, f, tensors, ids, mass):
    """(W_mol, K_mol) from unwrapped positions, velocities, force-field forces and the per-atom virial tensors (N, 6) -- or their
    six sums -- of ortho_ref.total"""
    t = np.asarray(tensors, dtype=np.float64)
    W = t.sum(axis=0) if t.ndim == 2 else t
    cw, ck = corrections(x, v, f, ids, mass)
    return W - cw, mr.kinetic_sums(v, mass) - ck


def scale(x, v, lo, lengths, mu, ids, mass, velocity_scale=1.0):
    """(positions, velocities, lengths) after the molecular scale"""
    lo, mu = np.asarray(lo, dtype=np.float64), np.broadcast_to(np.asarray(mu, dtype=np.float64), (3,))
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    xs, ln = bref.scale(x, lo, lengths, mu)                                    # molecules of one, and the box
    vs = velocity_scale * v
    Y, V, _, _, _, mol = centres(x, v, ids, mass)
    many = (np.bincount(mol)[mol] > 1)
    xs[many] = (x + (mu - 1.0) * (Y - lo)[mol])[many]
    vs[many] = (v + (velocity_scale - 1.0) * V[mol])[many]
    return xs, vs, ln


def coupled_constrained_verlet(pos, vel, force, atomic_virial, nsteps, dt, pairs, ids, mass, lo, lengths, kind, p_ref, beta, tau_p,
                               every, coupling=bref.ISOTROPIC, temperature=None, xi=None, first_step=0, langevin=None, observe=None):
    """molecular_ref.coupled_constrained_verlet with the triangles replaced by shake_ref's list of constraint pairs (Gauss-Seidel
    SHAKE and RATTLE) and the molecules by an id array: a coupling event after stage (e) of every step that brings the count (from
    first_step) to a multiple of `every` -- P_mol from that step's forces and velocities, mu (and the velocity scale) from
    barostat_ref, the molecular scale.  The callbacks are molecular_ref's: force(x, lengths, k), atomic_virial(x, lengths, s),
    xi(count), observe(s, x, v, lengths).  Returns (x, v, lengths, events), events = [(s, P diagonal, mu, velocity scale)]."""
    x, v = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    im = (1.0 / mass)[:, None]
    ln = np.array(lengths, dtype=np.float64)
    f = force(x, ln, 0)
    count, events = int(first_step), []
    for s in range(1, nsteps + 1):
        x0 = x.copy()
        v += 0.5 * dt * im * f
        if langevin is not None:
            gamma, temp, normals = langevin
            c1 = np.exp(-gamma * dt)
            v = c1 * v + np.sqrt(1.0 - c1 * c1) * np.sqrt(temp * im) * normals(s - 1)
        x += dt * v
        xc = hr.shake(x0, x, pairs, mass)
        v += (xc - x) / dt
        x = xc
        f = force(x, ln, s)
        v += 0.5 * dt * im * f
        v = hr.rattle(x, v, pairs, mass)
        count += 1
        if count % every == 0:
            Wm, Km = molecular_sums(x, v, f, atomic_virial(x, ln, s), ids, mass)
            P = mr.pressure_diagonal(Wm, Km, ln)
            if kind == bref.BERENDSEN:
                mu, vs = bref.berendsen_mu(P, p_ref, beta, tau_p, every * dt, coupling), 1.0
            else:
                assert coupling == bref.ISOTROPIC
                mu, vs = bref.crescale_mu(P, np.ravel(p_ref)[0], np.ravel(beta)[0], tau_p, every * dt, temperature, float(np.prod(ln)),
                                          xi(count))
            x, v, ln = scale(x, v, lo, ln, mu, ids, mass, vs)
            f = force(x, ln, -s)
            events.append((s, P, mu, vs))
        if observe is not None:
            observe(s, x, v, ln)
    return x, v, ln, events


def strained_terms(B, factor=0.97):
    """the bonds of molecule_box() with r0 shortened by `factor`: they pull at the loaded geometry (a smooth change of U alone)"""
    return [(1, B["bonds"], B["bond_params"] * np.array([1.0, factor]))]


# ---------------------------------------------------------------- the box the tests share
SIZES = (1, 2, 3, 4, 8, 9, 63, 64, 65, 129)                      # atoms: the class boundary (8 | 9), the wavefront loop's edges, two trips
# whole box lengths these molecules are loaded away by.  Every coordinate stays below 32: coupled_constrained_verlet forms
# v += (x_constrained - x_unconstrained) / dt from absolute coordinates, so its own velocities carry ulp(|x|) / dt per step (3.6e-15 /
# 0.002 below 32, twice that above), which is what a comparison at 1e-11 of the rms velocity over 20 steps can afford
FAR = {9: (-3, 2, -2), 129: (2, -2, 1), 65: (0, 0, -1)}
BOND_K = 60.0
_CACHE = {}


def molecule_box(seed=23):
    """shake_ref.mixed_box (1180 atoms: 300 clusters, 60 waters, 100 free atoms; sides (9.0, 9.6, 10.5)) with every constraint group
    made whole (shake_ref.unwrap) and the atoms dealt to molecules: one of each size in SIZES, built from groups that neighbour one
    another on the lattice of the box (Morton order of the cells of the groups' first atoms: compact blocks) and topped up with free atoms; every other cluster
    and water is a molecule of its own, every other free atom is at -1.  The ids are neither dense nor ordered.  The molecules of
    FAR are loaded whole box lengths away (the 9-atom one three lengths out along x, two along y and z), the others where unwrap left them:
    groups stick out of the box faces.  Inside the molecules of 8 atoms and more harmonic bonds tie consecutive cluster centres, r0 =
    the starting distance (no force at the start), each shorter than half the shortest side minus rc.
    mixed_box's dict with pos = unwrapped = the loaded positions, and ids (N,), members {size: atom ids}, bonds (n, 2), bond_params
    (n, 2) {k, r0}, terms (ortho_ref.total's list); computed once per process."""
    if seed not in _CACHE:
        B = hr.mixed_box(seed)
        x = hr.unwrap(B["pos"], B["pairs"], hr.LENGTHS)
        N = x.shape[0]
        groups = [[int(a) for a in c if a >= 0] for c in B["clusters"]] + [[int(a) for a in m] for m in B["mol"]]
        n_held = sum(len(g) for g in groups)
        free = list(range(n_held, N))

        def cell(a):
            """the Morton number of the atom's lattice cell: a run of consecutive groups is a compact block of the 8 x 8 x 8 lattice"""
            i, j, k = np.floor((B["pos"][a] - hr.LO) / hr.LENGTHS * 8.0).astype(int)
            return sum((((i >> b) & 1) << (3 * b + 2)) | (((j >> b) & 1) << (3 * b + 1)) | (((k >> b) & 1) << (3 * b)) for b in range(3))
        order = sorted(range(len(groups)), key=lambda g: cell(groups[g][0]))
        free.sort(key=cell)
        ids = np.full(N, -1, dtype=np.int64)
        members, heads, used, label = {}, {}, set(), 1000
        cursor = 0
        for size in sorted(SIZES, reverse=True):
            atoms, heads[size] = [], []
            if size == 1:
                atoms = [free.pop()]
            else:
                while cursor < len(order) and len(atoms) + len(groups[order[cursor]]) <= size and (size > 4 or not atoms):
                    if size <= 4 and len(groups[order[cursor]]) != size:
                        cursor += 1
                        continue
                    if order[cursor] < len(B["clusters"]):
                        heads[size].append(groups[order[cursor]][0])       # (cluster centres, in lattice order)
                    atoms += groups[order[cursor]]; used.add(order[cursor]); cursor += 1
                while len(atoms) < size:
                    atoms.append(free.pop(0))
            label -= 7                                                         # (descending, with gaps: neither dense nor ordered)
            ids[atoms] = label
            members[size] = np.array(sorted(atoms))
        for g in range(len(groups)):
            if g not in used:
                label += 5000
                ids[groups[g]] = label
        for size, shift in FAR.items():
            x[members[size]] += np.array(shift) * hr.LENGTHS
        assert np.abs(x).max() < 32.0 and np.abs(x[members[9]] - B["pos"][members[9]]).max() > 2.9 * hr.LENGTHS.min()
        bonds = []
        for size in SIZES:
            if size >= 8:
                c = heads[size]
                bonds += [(a, b) for a, b in zip(c[:-1], c[1:]) if np.linalg.norm(x[a] - x[b]) < 2.0][:12]
        bonds = np.array(bonds, dtype=np.int64)
        r0 = np.linalg.norm(x[bonds[:, 0]] - x[bonds[:, 1]], axis=1)
        assert len(bonds) >= 8 and (r0 < 0.5 * hr.LENGTHS.min() - hr.RC).all()
        params = np.stack([np.full(len(bonds), BOND_K), r0], axis=1)
        B.update(pos=x, unwrapped=x.copy(), ids=ids, members=members, bonds=bonds, bond_params=params, terms=[(1, bonds, params)])
        for c in B["clusters"]:                                               # every constraint group inside one molecule
            assert len({ids[a] for a in c if a >= 0}) == 1 and ids[c[0]] >= 0
        for m in B["mol"]:
            assert len({ids[a] for a in m}) == 1 and ids[m[0]] >= 0
        assert sorted(len(v) for v in members.values()) == sorted(SIZES)
        assert all((ids == ids[members[s][0]]).sum() == s for s in SIZES)
        _CACHE[seed] = B
    return {k: (dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else np.array(v)) for k, v in _CACHE[seed].items()}
