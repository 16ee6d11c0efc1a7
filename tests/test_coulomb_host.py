"""Host tests of the reaction-field Coulomb terms: the numpy yardstick (tests/helpers/coulomb_ref.py) against its own energy,
its limits and identities, and the charges that force-field ingest and synthetic.water_box hand to emdee_*_set_coulomb."""
import os

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import coulomb_ref as cr

XML = os.path.join(ROOT, "tests", "golden", "dibenzo-p-dioxin-in-water.xml")


def _cluster(n=40, L=3.0, seed=3):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, L, (n, 3))
    q = rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 0.8, n)
    return pos, q, L


@pytest.mark.parametrize("eps_rf", [1.0, 4.0, 78.5, np.inf])
def test_forces_are_the_central_difference_of_the_energy(eps_rf):
    pos, q, L = _cluster()
    K, rc = 1.7, 1.1
    excl, p14 = np.array([[0, 1], [2, 3]]), np.array([[4, 5], [6, 7]])
    f = cr.coulomb(pos, L, q, K, rc, eps_rf, excl, p14, 0.5)[0]
    h = 1e-6
    for a in (0, 4, 9, 17):
        for d in range(3):
            p, m = pos.copy(), pos.copy()
            p[a, d] += h
            m[a, d] -= h
            num = -(cr.energy(p, L, q, K, rc, eps_rf, excl, p14, 0.5) - cr.energy(m, L, q, K, rc, eps_rf, excl, p14, 0.5)) / (2 * h)
            assert num == pytest.approx(f[a, d], rel=1e-6, abs=1e-7)


def test_tensor_trace_is_the_virial_and_forces_sum_to_zero():
    pos, q, L = _cluster(seed=5)
    f, e, w, t = cr.coulomb(pos, L, q, 2.0, 1.2, 10.0, np.array([[0, 1]]), np.array([[2, 3]]), 0.8333)
    assert np.allclose(t[:, :3].sum(axis=1), w, rtol=1e-12, atol=1e-12)
    assert np.abs(f.sum(axis=0)).max() < 1e-10 * np.abs(f).max()


def test_reaction_field_limits():
    rc = 0.9
    k1, c1 = cr.rf_constants(rc, 1.0)
    assert k1 == 0.0 and c1 == pytest.approx(1.0 / rc)
    kinf, cinf = cr.rf_constants(rc, np.inf)
    assert kinf == pytest.approx(0.5 / rc ** 3) and cinf == pytest.approx(1.5 / rc)
    assert cr.rf_constants(rc, 1e12)[0] == pytest.approx(kinf, rel=1e-9)
    for eps in (1.0, 2.0, 78.5, np.inf):
        U, W = cr.pair_energy_virial(rc, 1.3, rc, eps)
        assert U == pytest.approx(0.0, abs=1e-14)
        # the force at rc: zero at eps = inf, else K q q 3 / ((2 eps + 1) rc^2)
        jump = 0.0 if np.isinf(eps) else 1.3 * 3.0 / ((2 * eps + 1) * rc * rc)
        assert W / rc == pytest.approx(jump, abs=1e-12)


def test_the_fixture_water_charges_and_neutral_molecules(emdee):
    E = emdee
    t = E.ingest.ResidueTemplates(XML)
    hoh = t.residues["HOH"]
    assert dict(zip(hoh["names"], hoh["charges"])) == {"Ow": -0.84, "Hw1": 0.42, "Hw2": 0.42}
    q = t.charges(["HOH"] * 5)
    types, _ = t.build(["HOH"] * 5)
    assert len(q) == len(types) == 15
    assert np.abs(q.reshape(-1, 3).sum(axis=1)).max() < 1e-12
    # build() keeps its two results
    assert len(t.build(["HOH"])) == 2
    assert E.ingest.NonbondedTable(XML).coulomb14scale == pytest.approx(0.833333)


def test_water_box_carries_charges_in_atom_order(emdee):
    E = emdee
    w = E.synthetic.water_box(3)
    q = w["charges"]
    assert q.shape == (81,) and q.dtype == np.float64
    assert np.array_equal(q, np.array([{"OW": -0.84, "HW": 0.42}[t] for t in w["types"]]))
    assert np.abs(q.reshape(-1, 3).sum(axis=1)).max() < 1e-12
    assert E.COULOMB_K_KJ_NM == pytest.approx(138.935457644)
