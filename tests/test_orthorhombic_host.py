"""Host tests of the per-axis yardstick tests/helpers/ortho_ref.py, which the GPU tests of tests/test_gpu_orthorhombic.py are
held against: it equals the pinned oracle and the golden vectors on cubes, it is covariant under a cycling of the axes, and
its forces are minus the gradient of its own energy on a box with three different sides and an origin off zero."""
import numpy as np
import pytest

from .helpers import bonded_ref as br
from .helpers import coulomb_ref as cr
from .helpers import ortho_ref as oref
from .helpers import virial_tensor_ref as vt

ZERO = [0.0, 0.0, 0.0]
PER = [1, 1, 1]


def _cube_cases(oracle, syn, lj_sample, golden):
    g = golden["lj_sample_expected"]
    yield ("lj_sample", lj_sample.astype(np.float64), 10.0, (3.0, 2.5), oracle.lj_atoms(1.0, 1.0, 800),
           (g["forces_cutoff"], g["energies_cutoff"], g["virials_cutoff"]))
    g = golden["fcc864_expected"]
    pos, L = syn.fcc_positions(6)
    yield "fcc864", pos, L, (2.5, 2.0), oracle.lj_atoms(1.0, 1.0, 864), (g["forces"], g["energies"], g["virials"])
    g = golden["mix500_expected"]
    pos, L = syn.fcc_positions(5)
    eps, sigma = syn.mixture_parameters(syn.mixture_types(500))
    yield "mix500", pos, L, (3.5, 3.0), oracle.lj_atoms(eps, sigma), (g["forces"], g["energies"], None)


def test_yardstick_equals_the_oracle_and_the_golden_vectors_on_cubes(oracle, emdee_synthetic, lj_sample, golden):
    for name, pos, L, (rc, rs), atoms, gold in _cube_cases(oracle, emdee_synthetic, lj_sample, golden):
        out = oref.nonbonded(pos, ZERO, [L] * 3, PER, rc, rs, atoms)
        f0, e0, w0 = oracle.nonbonded_cells(pos, L, oracle.model(rc, rs), atoms)
        for got, want in ((out["f"], f0), (out["e"], e0), (out["w"], w0)) + tuple(zip((out["f"], out["e"], out["w"]), gold)):
            if want is not None:
                np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10, err_msg=name)
        # the tensor: virial_tensor_ref's, and its trace the virial
        t0, _ = vt.per_atom_tensor(pos, [L] * 3, PER, rc, rs, *oref.lj_fields(atoms))
        np.testing.assert_allclose(out["t"], t0, rtol=1e-10, atol=1e-10, err_msg=name)
        np.testing.assert_allclose(vt.trace(out["t"]), out["w"], rtol=1e-10, atol=1e-10, err_msg=name)
        # sampled mode: the same rows
        rows = np.array([0, 7, pos.shape[0] - 1])
        some = oref.nonbonded(pos, ZERO, [L] * 3, PER, rc, rs, atoms, rows=rows)
        for k in "fewt":
            np.testing.assert_allclose(some[k][rows], out[k][rows], rtol=1e-10, atol=1e-12, err_msg=name + " sampled " + k)
        want_rows = oracle.neighbor_list(pos, L, rc + 0.3)
        got_rows = oref.neighbour_rows(pos, [L] * 3, PER, rc + 0.3)
        off, nb = want_rows
        for i in range(pos.shape[0]):
            assert np.array_equal(got_rows[i], np.sort(nb[off[i]:off[i + 1]])), (name, i)


def _ortho_system(oracle, rng, n=160):
    """A dense random box [5, 6, 7] with lo != 0: atoms at least 0.85 apart, two species, charges, three molecules' worth of
    exclusions and 1-4 pairs, positions left wherever the draw put them around the box (pairs straddle every face)."""
    lo, lengths = np.array([-1.3, 0.4, 2.1]), np.array([5.0, 6.0, 7.0])
    pos = []
    while len(pos) < n:
        p = lo + rng.random(3) * lengths
        if all(np.linalg.norm(vt._minimum_image((p - q)[None, :].copy(), lengths, PER)) > 0.85 for q in pos):
            pos.append(p)
    pos = np.array(pos)
    k = np.arange(n) % 2
    atoms = oracle.lj_atoms(np.array([1.0, 0.5])[k], np.array([1.0, 0.88])[k])
    q = 0.4 * np.where(np.arange(n) % 3 == 0, 1.0, -0.5)
    mol = np.arange(12).reshape(-1, 4)
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]]])
    return pos, lo, lengths, atoms, q, excl, mol[:, [0, 3]]


def test_yardstick_is_covariant_under_a_cycling_of_the_axes(oracle):
    rng = np.random.default_rng(5)
    pos, lo, lengths, atoms, q, excl, p14 = _ortho_system(oracle, rng)
    vel = rng.normal(size=pos.shape)
    terms = [(br.BOND, [[20, 21]], [[100.0, 1.0]]), (br.ANGLE, [[22, 23, 24]], [[30.0, 1.5]]), (br.TORSION, [[25, 26, 27, 28]], [[1.5, 2.0, 0.3]])]
    kw = dict(excl=excl, p14=p14, lj14scale=0.5, charges=q, coulomb_k=1.3, eps_rf=7.0, coulomb14scale=0.8)
    for periodic in ([1, 1, 1], [1, 0, 1]):
        p = oref.wrapped(pos, lo, lengths, [1, 1, 1]) if not all(periodic) else pos
        base = oref.total(p, lo, lengths, periodic, 2.4, 2.0, atoms, terms, **kw)
        force = lambda x, per=periodic, l=lengths, o=lo: oref.total(x, o, l, per, 2.4, 2.0, atoms, terms, **kw)["f"]
        x5, v5 = oref.verlet(p, vel, force, 5, 0.002)
        for k in (1, 2):
            cp, cl, clo, cper = oref.cycle(p, k), oref.cycle(lengths, k), oref.cycle(lo, k), list(oref.cycle(periodic, k))
            out = oref.total(cp, clo, cl, cper, 2.4, 2.0, atoms, terms, **kw)
            np.testing.assert_allclose(out["f"], oref.cycle(base["f"], k), rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(out["t"], oref.cycle_tensor(base["t"], k), rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(out["e"], base["e"], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(out["w"], base["w"], rtol=1e-12, atol=1e-11)
            cforce = lambda x: oref.total(x, clo, cl, cper, 2.4, 2.0, atoms, terms, **kw)["f"]
            cx, cv = oref.verlet(cp, oref.cycle(vel, k), cforce, 5, 0.002)
            np.testing.assert_allclose(cx, oref.cycle(x5, k), rtol=0, atol=1e-11)
            np.testing.assert_allclose(cv, oref.cycle(v5, k), rtol=0, atol=1e-10)
        # and the box is not one on which a swap would go unseen: two lengths exchanged change the answer
        swapped = oref.total(p, lo, lengths[[0, 2, 1]], [periodic[0], periodic[2], periodic[1]], 2.4, 2.0, atoms, terms, **kw) \
            if all(periodic) else None
        if swapped is not None:
            assert np.abs(swapped["f"] - base["f"]).max() > 1e-2 * np.abs(base["f"]).max()


def test_yardstick_forces_are_minus_the_gradient_of_its_energy(oracle):
    rng = np.random.default_rng(9)
    pos, lo, lengths, atoms, q, excl, p14 = _ortho_system(oracle, rng, n=90)
    # unwrap some atoms by whole box lengths, a different multiple per axis: nothing may change
    far = pos + np.array([2.0, -1.0, 3.0]) * lengths * (np.arange(pos.shape[0]) % 2)[:, None]
    rc, rs = 2.4, 2.0                                           # below half of the shortest side
    kw = dict(excl=excl, p14=p14, lj14scale=0.5, charges=q, coulomb_k=1.3, eps_rf=7.0, coulomb14scale=0.8)
    out = oref.nonbonded(pos, lo, lengths, PER, rc, rs, atoms, **kw)
    again = oref.nonbonded(far, lo, lengths, PER, rc, rs, atoms, **kw)
    for k in "fewt":
        np.testing.assert_allclose(again[k], out[k], rtol=1e-10, atol=1e-10)
    # pairs straddle each of the three faces
    i, j, d = vt.pairs_in_range(oref.wrapped(pos, lo, lengths, PER), lengths, PER, rc, margin=0.0)
    w = oref.wrapped(pos, lo, lengths, PER)
    for a in range(3):
        assert (np.abs((w[i] - w[j])[:, a]) > lengths[a] / 2).sum() > 10
    # no pair so close to rc that the +-h displacements carry it across: the reaction-field energy is continuous there, the force is not
    assert oref.nearest_to_radius(pos, lengths, PER, rc) > 1e-4
    h = 1e-5
    E = lambda x: oref.energy(x, lo, lengths, PER, rc, rs, atoms, **kw)
    for g in rng.choice(pos.shape[0], 12, replace=False):
        for c in range(3):
            xp, xm = pos.copy(), pos.copy()
            xp[g, c] += h; xm[g, c] -= h
            fd = -(E(xp) - E(xm)) / (2 * h)
            assert abs(out["f"][g, c] - fd) <= 1e-7 * np.abs(out["f"]).max(), (g, c)
    # the Coulomb part alone is coulomb_ref's with the per-axis lengths
    fc, ec, wc, tc = cr.coulomb(pos, lengths, q, 1.3, rc, 7.0, excl=excl, p14=p14, s14=0.8)
    mine = oref.nonbonded(pos, lo, lengths, PER, rc, rs, atoms, lj=False, **kw)
    for got, want in zip((mine["f"], mine["e"], mine["w"], mine["t"]), (fc, ec, wc, tc)):
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)
    with pytest.raises(AssertionError):
        cr.box_lengths([1.0, 2.0])
