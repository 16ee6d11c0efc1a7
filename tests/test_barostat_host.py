"""CPU checks of the pressure-coupling yardstick (tests/helpers/barostat_ref.py): the scale factors of include/emdee_hip.h
(emdee_md_set_barostat) and the scale itself (emdee_md_scale_box), which the GPU tests of tests/test_gpu_barostat.py hold the
engine to."""
import numpy as np
import pytest

from .helpers import barostat_ref as bref

P = np.array([1.3, -0.4, 2.2])


@pytest.mark.parametrize("coupling", [bref.ISOTROPIC, bref.SEMIISOTROPIC, bref.ANISOTROPIC])
def test_reference_pressure_gives_no_scaling(coupling):
    target = bref.coupled_pressure(P, coupling)                      # per axis; entries 0 (and 2, or all) are the ones read
    assert np.array_equal(bref.berendsen_mu(P, target, [0.03, 0.02, 0.05], 0.7, 0.02, coupling), np.ones(3))
    if coupling == bref.ISOTROPIC:
        mu, vs = bref.crescale_mu(P, target[0], 0.03, 0.7, 0.02, 1.0, 1000.0, 0.0)
        assert np.array_equal(mu, np.ones(3)) and vs == 1.0


def test_the_factors_follow_the_formulas():
    Dt, tau, beta, pref = 0.02, 0.5, np.array([0.03, 0.02, 0.05]), np.array([4.0, 5.0, 6.0])
    c = Dt / (3.0 * tau)
    assert bref.berendsen_mu(P, pref, beta, tau, Dt, bref.ISOTROPIC) == pytest.approx([1.0 - c * 0.03 * (4.0 - P.mean())] * 3, rel=1e-15)
    want = [1.0 - c * 0.03 * (4.0 - 0.45), 1.0 - c * 0.03 * (4.0 - 0.45), 1.0 - c * 0.05 * (6.0 - 2.2)]
    assert bref.berendsen_mu(P, pref, beta, tau, Dt, bref.SEMIISOTROPIC) == pytest.approx(want, rel=1e-15)
    assert bref.berendsen_mu(P, pref, beta, tau, Dt, bref.ANISOTROPIC) == pytest.approx(1.0 - c * beta * (pref - P), rel=1e-15)
    mu, vs = bref.crescale_mu(P, 4.0, 0.03, tau, Dt, 1.2, 800.0, -0.7)
    de = -(0.03 / tau) * (4.0 - P.mean()) * Dt + np.sqrt(2.0 * 1.2 * 0.03 * Dt / (800.0 * tau)) * -0.7
    assert mu == pytest.approx([np.exp(de / 3.0)] * 3, rel=1e-15) and vs == pytest.approx(np.exp(-de / 3.0), rel=1e-15)


def test_semi_isotropic_shares_one_factor_between_x_and_y():
    mu = bref.berendsen_mu(P, [4.0, 99.0, 6.0], [0.03, 99.0, 0.05], 0.5, 0.02, bref.SEMIISOTROPIC)
    assert mu[0] == mu[1] and mu[2] != mu[0]


def test_crescale_without_noise_is_berendsen_to_first_order():
    """mu = exp(-x) against 1 - x with x = (Dt / (3 tau_p)) beta (P_ref - P): the difference is x^2 / 2 to leading order, so it
    falls by four when Dt / tau_p halves."""
    gaps = []
    for Dt in (0.04, 0.02, 0.01):
        b = bref.berendsen_mu(P, [9.0] * 3, [0.05] * 3, 1.0, Dt, bref.ISOTROPIC)
        c, _ = bref.crescale_mu(P, 9.0, 0.05, 1.0, Dt, 1.0, 1000.0, 0.0)
        x = 1.0 - b[0]
        assert abs((c[0] - b[0]) - 0.5 * x * x) <= x ** 3
        gaps.append(c[0] - b[0])
    assert gaps[0] / gaps[1] == pytest.approx(4.0, rel=1e-2) and gaps[1] / gaps[2] == pytest.approx(4.0, rel=1e-2)


def test_the_scale_maps_the_box_onto_the_scaled_box():
    lo, ln, mu = np.array([-3.7, 1.9, 11.3]), np.array([10.0, 12.0, 9.0]), np.array([1.10, 1.00, 0.95])
    rng = np.random.default_rng(3)
    x = lo + ln * rng.random((1000, 3))
    x[0], x[1] = lo, lo + ln * (1.0 - 2.0 ** -50)
    y, ln2 = bref.scale(x, lo, ln, mu)
    assert np.array_equal(ln2, mu * ln) and np.array_equal(y[0], lo)
    assert (y >= lo).all() and (y < lo + ln2).all()
    assert np.abs((y - lo) / ln2 - (x - lo) / ln).max() < 1e-15     # fractional coordinates are kept
    # an image k box lengths away lands k NEW box lengths away
    z, _ = bref.scale(x + np.array([2.0, -1.0, 3.0]) * ln, lo, ln, mu)
    assert np.abs(z - (y + np.array([2.0, -1.0, 3.0]) * ln2)).max() < 1e-13


def test_coupled_verlet_with_zero_compressibility_is_plain_verlet(emdee_synthetic):
    from .helpers import ortho_ref as oref
    S = bref.fluid864(emdee_synthetic)
    tot = bref.field(S["atoms"])
    x, v, ln, ev = bref.coupled_verlet(S["pos"], S["vel"], np.zeros(3), [S["L"]] * 3, tot, 4, bref.DT, bref.BERENDSEN, [5.0] * 3,
                                       [0.0] * 3, 1.0, 2)
    xr, vr = oref.verlet(S["pos"], S["vel"], lambda q: tot(q, [S["L"]] * 3)["f"], 4, bref.DT)
    assert len(ev) == 2 and [e[0] for e in ev] == [2, 4] and np.array_equal(ln, [S["L"]] * 3)
    assert np.abs(x - xr).max() < 1e-13 and np.abs(v - vr).max() < 1e-13
    # the pressure the events saw is the scalar one: (2 KE + sum w) / (3 V)
    out = tot(xr, ln)
    assert ev[-1][1].mean() == pytest.approx((np.sum(vr * vr) + out["w"].sum()) / (3.0 * np.prod(ln)), rel=1e-12)
