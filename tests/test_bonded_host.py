"""Host tests of the bonded terms: the numpy restatement (tests/helpers/bonded_ref.py) against finite differences of its own
energy, and the force-field ingest (BondedTable, ResidueTemplates, topology) on the committed fixture."""
import os
from collections import deque

import numpy as np
import pytest

from .conftest import GOLDEN
from .helpers import bonded_ref as br

XML = os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml")


def _random_terms(rng, L, n_terms=6):
    """terms whose atoms straddle the periodic boundary (placed near a corner, then wrapped)"""
    x, terms = [], []
    for kind, params in ((br.BOND, (300.0, 0.9)), (br.ANGLE, (50.0, 1.9)), (br.TORSION, (2.0, 3.0, 0.4))):
        for _ in range(n_terms):
            base = len(x)
            p = L - 0.3 + np.cumsum(rng.normal(scale=0.6, size=(br.ATOMS[kind], 3)), axis=0)
            x.extend(np.mod(p, L))
            terms.append((kind, [np.arange(base, base + br.ATOMS[kind])], [params]))
    return np.array(x), terms


def test_reference_forces_are_minus_the_gradient_of_its_energy():
    rng = np.random.default_rng(3)
    L = np.array([5.0, 6.0, 7.0])
    x, terms = _random_terms(rng, L)
    assert (np.abs(np.diff(x, axis=0)) > L / 2).any()           # the terms cross the boundary
    f, e, w, t = br.bonded(x, L, terms)
    h = 1e-6
    for term in terms:
        idx = term[1][0]
        got = br.bonded(x, L, [term])[0][idx]
        fd = np.zeros_like(got)
        for a, g in enumerate(idx):
            for c in range(3):
                xp, xm = x.copy(), x.copy()
                xp[g, c] += h; xm[g, c] -= h
                fd[a, c] = -(br.total_energy(xp, L, [term]) - br.total_energy(xm, L, [term])) / (2 * h)
        assert np.abs(got - fd).max() <= 1e-7 * np.abs(got).max()
    assert e.sum() == pytest.approx(br.total_energy(x, L, terms), rel=1e-12)
    # no net force, no net torque (about the unwrapped positions), symmetric tensor whose trace is w
    for term in terms:
        idx = term[1][0]
        ft = br.bonded(x, L, [term])[0][idx]
        u = br.unwrapped(x, idx, L)
        assert np.abs(ft.sum(axis=0)).max() <= 1e-10 * np.abs(ft).max()
        assert np.abs(np.cross(u, ft).sum(axis=0)).max() <= 1e-9 * np.abs(ft).max() * np.abs(u).max()
        T = u.T @ ft
        assert np.abs(T - T.T).max() <= 1e-9 * np.abs(T).max()
    assert np.abs(t[:, :3].sum(axis=1) - w).max() <= 1e-12 * np.abs(w).max()


def test_reference_is_finite_at_straight_angles_and_collinear_torsions():
    L = np.array([10.0, 10.0, 10.0])
    x = np.array([[1.0, 1, 1], [2.0, 1, 1], [3.0, 1, 1], [4.0, 1, 1]])
    for kind, p in ((br.ANGLE, (50.0, 1.9)), (br.TORSION, (2.0, 3.0, 0.4))):
        f, e, w, t = br.bonded(x, L, [(kind, [np.arange(br.ATOMS[kind])], [p])])
        assert np.isfinite(f).all() and np.isfinite(e).all() and np.isfinite(t).all()


@pytest.fixture(scope="module")
def ingest(emdee):
    return emdee.ingest


def test_bonded_table_of_the_fixture(ingest):
    t = ingest.BondedTable(XML)
    assert (len(t.bonds), len(t.angles), len(t.propers)) == (4, 5, 2)
    assert t.bond("HW", "OW") == t.bond("OW", "HW") == [(443153.375, 0.101199999)]
    assert t.angle("HW", "OW", "HW") == [(317.565613, 1.97641087)]
    assert t.angle("ha", "ca", "ca") == t.angle("ca", "ca", "ha")   # forward or reversed
    assert t.proper("ha", "ca", "ca", "os") == [(15.1669998, 2.0, 3.14159274)]   # "" wildcards
    assert t.proper("ca", "ca", "os", "ca") == [(3.76559997, 2.0, 3.14159274)]
    assert t.proper("ca", "os", "os", "ca") is None


def _distance3_pairs(n, bonds):
    nb = [[] for _ in range(n)]
    for i, j in bonds:
        nb[i].append(j); nb[j].append(i)
    count = 0
    for s in range(n):
        dist, todo = {s: 0}, deque([s])
        while todo:
            a = todo.popleft()
            for b in nb[a]:
                if b not in dist:
                    dist[b] = dist[a] + 1
                    todo.append(b)
        count += sum(1 for t, d in dist.items() if t > s and d == 3)
    return count


def test_topology_of_dibenzo_p_dioxin_and_water(ingest):
    t, r = ingest.BondedTable(XML), ingest.ResidueTemplates(XML)
    types, bonds = r.build(["aaa"])
    top = ingest.topology(types, bonds, t)
    assert len(top["bonds"]) == 24 and len(top["angles"]) == 38 and len(top["torsions"]) == 56
    for key, n in (("bond_params", 24), ("angle_params", 38), ("torsion_params", 56)):
        assert top[key].shape[0] == n and np.isfinite(top[key]).all()
    assert len(top["pairs14"]) == _distance3_pairs(len(types), bonds)
    assert len({tuple(p) for p in top["pairs14"]}) == len(top["pairs14"])
    types, bonds = r.build(["HOH"])
    top = ingest.topology(types, bonds, t)
    assert (len(top["bonds"]), len(top["angles"]), len(top["torsions"]), len(top["exclusions"])) == (2, 1, 0, 3)
    # two molecules: ids of the second are offset, nothing joins them
    types, bonds = r.build(["HOH", "aaa"])
    top = ingest.topology(types, bonds, t, length_unit=0.1)
    assert len(top["bonds"]) == 26 and top["bond_params"][0][1] == pytest.approx(1.01199999)


def test_topology_raises_on_a_term_without_parameters(ingest):
    t = ingest.BondedTable(XML)
    with pytest.raises(KeyError):
        ingest.topology(["os", "os"], [[0, 1]], t)


def test_water_box_geometry(emdee):
    w = emdee.synthetic.water_box(4)
    x, L = w["positions"], w["L"]
    u = np.array([br.unwrapped(x, b, L) for b in w["bonds"]])
    assert np.allclose(np.linalg.norm(u[:, 1] - u[:, 0], axis=1), w["bond_params"][:, 1])
    a = np.array([br.unwrapped(x, q, L) for q in w["angles"]])
    v1, v2 = a[:, 0] - a[:, 1], a[:, 2] - a[:, 1]
    th = np.arccos(np.einsum("ij,ij->i", v1, v2) / np.linalg.norm(v1, axis=1) / np.linalg.norm(v2, axis=1))
    assert np.allclose(th, w["angle_params"][:, 1])
    assert w["inv_mass"].shape == (x.shape[0],) and (w["inv_mass"] > 0).all()
