"""CPU tests of the numpy yardstick of whole-molecule pressure and scaling (tests/helpers/molecule_ref.py; include/emdee_hip.h:
emdee_md_set_molecules), with the yardsticks alone: on molecule_ref.molecule_box() -- molecules of 1 to 129 atoms, some loaded whole
box lengths away -- tr W_mol = -dU/dmu under the reference's own scale with the all-pairs sums of ortho_ref.total plus the harmonic
bonds; with every atom its own molecule the sums are the atomic ones; on triangles alone the file is molecular_ref.py; the scale
keeps every intramolecular distance and multiplies the centres' distances to lo by mu."""
import numpy as np

from .helpers import molecular_ref as mr
from .helpers import molecule_ref as gr
from .helpers import ortho_ref as oref
from .helpers import settle_ref as sr
from .helpers import shake_ref as hr
from .test_molecular_ref_host import FD_BOUND, H

MU = np.array([1.013, 0.991, 1.004])


def _total(B, x, lengths, terms):
    return oref.total(oref.wrapped(x, hr.LO, lengths, [1, 1, 1]), hr.LO, lengths, [1, 1, 1], hr.RC, hr.RS, B["atoms"], terms=terms, excl=B["excl"])


def test_trace_of_the_molecular_virial_is_the_volume_derivative_under_the_molecular_scale():
    B = gr.molecule_box()
    x0 = B["unwrapped"]
    # (the bonds carry no force at the loaded geometry: shorten their r0, so that the bonded part of the identity is tested too)
    terms = gr.strained_terms(B)
    out = _total(B, x0, hr.LENGTHS, terms)
    Wm, _ = gr.molecular_sums(x0, B["vel"], out["f"], out["t"], B["ids"], B["mass"])
    U = []
    for mu in (1.0 + H, 1.0 - H):
        x, _, ln = gr.scale(x0, B["vel"], hr.LO, hr.LENGTHS, mu, B["ids"], B["mass"])
        U.append(_total(B, x, ln, terms)["e"].sum())
    fd = -(U[0] - U[1]) / (2.0 * H)
    gap = abs(fd - Wm[:3].sum()) / abs(Wm[:3].sum())
    W = out["t"].sum(axis=0)
    print("tr W_mol = %.4f (tr W = %.4f), -dU/dmu = %.4f: relative difference %.3e (bound %.2e)" % (Wm[:3].sum(), W[:3].sum(), fd, gap, FD_BOUND))
    assert gap <= FD_BOUND
    assert abs(W[:3].sum() - Wm[:3].sum()) > 1e-3 * abs(Wm[:3].sum())          # (the two formulations differ: neither passes for the other)
    bonded = oref.bonded(oref.wrapped(x0, hr.LO, hr.LENGTHS, [1, 1, 1]), hr.LENGTHS, [1, 1, 1], terms)
    assert np.abs(bonded["f"]).max() > 0.1                                     # (the bonds take part)


def test_with_every_atom_its_own_molecule_the_sums_are_the_atomic_ones():
    B = gr.molecule_box()
    rng = np.random.default_rng(3)
    N = B["pos"].shape[0]
    f, t = rng.normal(size=(N, 3)), rng.normal(size=(N, 6))
    for ids in (np.full(N, -1), np.arange(N)[::-1] * 3, np.where(np.arange(N) % 2, -1, np.arange(N))):
        Wm, Km = gr.molecular_sums(B["unwrapped"], B["vel"], f, t, ids, B["mass"])
        assert np.array_equal(Wm, t.sum(axis=0)) and np.array_equal(Km, mr.kinetic_sums(B["vel"], B["mass"]))
        x, v, ln = gr.scale(B["unwrapped"], B["vel"], hr.LO, hr.LENGTHS, MU, ids, B["mass"], 0.5)
        assert np.array_equal(x, hr.LO + MU * (B["unwrapped"] - hr.LO)) and np.array_equal(v, 0.5 * B["vel"]) and np.array_equal(ln, MU * hr.LENGTHS)


def test_on_triangles_alone_it_is_the_rigid_yardstick():
    B = sr.water_box()
    mol = B["mol"][:120]
    ids = np.full(B["pos"].shape[0], -1)
    ids[mol] = (7 * np.arange(len(mol))[::-1])[:, None]                        # (neither dense nor ordered)
    out = oref.total(B["pos"], sr.LO, sr.LENGTHS, [1, 1, 1], sr.RC, sr.RS, B["atoms"], excl=B["excl"])
    want = np.concatenate(mr.molecular_sums(B["unwrapped"], B["vel"], out["f"], out["t"], mol, B["mass"]))
    got = np.concatenate(gr.molecular_sums(B["unwrapped"], B["vel"], out["f"], out["t"], ids, B["mass"]))
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-13 * scale
    Y, V, M, d, u, which = gr.centres(B["unwrapped"], B["vel"], ids, B["mass"])
    Yr, Vr, Mr, dr = mr.centres(B["unwrapped"], B["vel"], mol, B["mass"])
    m_of = which[mol[:, 0]]
    assert np.abs(Y[m_of] - Yr).max() <= 1e-14 * np.abs(Yr).max() and np.abs(V[m_of] - Vr).max() <= 1e-14 and np.array_equal(M[m_of], Mr)
    assert np.abs(d[mol] - dr).max() <= 1e-14
    a, b = gr.scale(B["unwrapped"], B["vel"], sr.LO, sr.LENGTHS, MU, ids, B["mass"], 0.5), mr.scale(B["unwrapped"], B["vel"], sr.LO, sr.LENGTHS, MU,
                                                                                                  mol, B["mass"], 0.5)
    assert np.abs(a[0] - b[0]).max() <= 1e-14 * np.abs(b[0]).max() and np.abs(a[1] - b[1]).max() <= 1e-14 and np.array_equal(a[2], b[2])


def test_scale_keeps_every_intramolecular_distance():
    B = gr.molecule_box()
    x0, ids = B["unwrapped"], B["ids"]
    x, v, ln = gr.scale(x0, B["vel"], hr.LO, hr.LENGTHS, MU, ids, B["mass"], 0.5)
    worst = 0.0
    for size, atoms in B["members"].items():                                 # every pair of every molecule of the size classes
        d0 = np.linalg.norm(x0[atoms][:, None] - x0[atoms][None], axis=2)
        d1 = np.linalg.norm(x[atoms][:, None] - x[atoms][None], axis=2)
        # (the shift is one number per molecule; each new coordinate is rounded once)
        worst = max(worst, (np.abs(d1 - d0) / np.where(d0 > 0.0, d0, 1.0)).max())
    i, j = B["pairs"][:, 0].astype(int), B["pairs"][:, 1].astype(int)
    res = np.abs(np.linalg.norm(x[i] - x[j], axis=1) - np.linalg.norm(x0[i] - x0[j], axis=1)) / B["pairs"][:, 2]
    print("largest change of an intramolecular distance %.3e (relative), of a constrained distance %.3e" % (worst, res.max()))
    assert worst <= 1e-14 and res.max() <= 1e-14


def test_scale_multiplies_the_centres_distances_to_lo_by_mu():
    B = gr.molecule_box()
    x0, ids = B["unwrapped"], B["ids"]
    x, v, ln = gr.scale(x0, B["vel"], hr.LO, hr.LENGTHS, MU, ids, B["mass"], 0.5)
    Y0, V0, M, _, u0, mol = gr.centres(x0, B["vel"], ids, B["mass"])
    Y1, V1, _, _, u1, _ = gr.centres(x, v, ids, B["mass"])
    assert np.abs((Y1 - hr.LO) - MU * (Y0 - hr.LO)).max() <= 1e-14 * np.abs(Y0 - hr.LO).max()
    many = np.bincount(mol)[mol] > 1
    assert np.abs(V1 - 0.5 * V0).max() <= 1e-14 and np.abs(u1 - u0)[many].max() <= 1e-14      # (momentum scales, internal motion stays)
    assert np.array_equal(ln, MU * hr.LENGTHS)


def test_ingest_molecules_are_the_connected_components_of_the_bond_graph(emdee):
    """ingest.molecules against the yardstick's labels: two waters, a five-atom chain given out of order, two atoms without a bond"""
    bonds = [(0, 1), (0, 2), (9, 7), (3, 4), (3, 5), (7, 6), (10, 9), (8, 10)]
    ids = emdee.ingest.molecules(13, bonds)
    assert ids.dtype == np.int32 and list(ids) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, -1, -1]
    mol, n_mol, first = gr.labels(ids)
    assert n_mol == 5 and list(first) == [0, 3, 6, 11, 12]
    assert list(emdee.ingest.molecules(3, [])) == [-1, -1, -1] and emdee.ingest.molecules(0, []).shape == (0,)
    try:
        emdee.ingest.molecules(3, [(0, 3)])
    except ValueError as err:
        assert "outside" in str(err)
    else:
        raise AssertionError("a bond to an atom outside the state was accepted")
