"""CPU test of the identity the molecular pressure rests on (include/emdee_hip.h: emdee_md_molecular_pressure_tensor), with the
numpy yardsticks alone: on settle_ref.water_box() with the all-pairs sums of ortho_ref.total, tr W_mol = -dU/dmu at mu = 1 under
the molecular scale of tests/helpers/molecular_ref.py (every molecule translated with its centre of mass, the box scaled)."""
import numpy as np

from .helpers import molecular_ref as mr
from .helpers import ortho_ref as oref
from .helpers import settle_ref as sr

H = 1e-4
# |central difference at h = 1e-4 - tr W_mol| / |tr W_mol|, measured on the CPU, 2026-10-18: 4.4e-7 (4.4e-5 at h = 1e-3, 4.4e-9 at
# 1e-5: the h^2 truncation of the difference, nothing else); the bound is four times that
FD_MEASURED = 4.4e-7
FD_BOUND = 4.0 * FD_MEASURED


def _total(B, x, lengths):
    return oref.total(oref.wrapped(x, sr.LO, lengths, [1, 1, 1]), sr.LO, lengths, [1, 1, 1], sr.RC, sr.RS, B["atoms"], excl=B["excl"])


def test_trace_of_the_molecular_virial_is_the_volume_derivative_under_the_molecular_scale():
    B = sr.water_box()
    out = _total(B, B["unwrapped"], sr.LENGTHS)
    Wm, Km = mr.molecular_sums(B["unwrapped"], B["vel"], out["f"], out["t"], B["mol"], B["mass"])
    U = []
    for mu in (1.0 + H, 1.0 - H):
        x, _, ln = mr.scale(B["unwrapped"], B["vel"], sr.LO, sr.LENGTHS, mu, B["mol"], B["mass"])
        assert sr.residual(x, B["mol"], B["geom"]) <= 1e-14                     # (rigid geometry survives the scale)
        U.append(_total(B, x, ln)["e"].sum())
    fd = -(U[0] - U[1]) / (2.0 * H)
    gap = abs(fd - Wm[:3].sum()) / abs(Wm[:3].sum())
    print("tr W_mol = %.4f, -dU/dmu = %.4f: relative difference %.3e (bound %.2e)" % (Wm[:3].sum(), fd, gap, FD_BOUND))
    assert gap <= FD_BOUND
    # the two formulations are far apart on this box: no test can take one for the other
    W, K = out["t"].sum(axis=0), mr.kinetic_sums(B["vel"], B["mass"])
    V = float(np.prod(sr.LENGTHS))
    P_mol, P_atom = (Wm[:3].sum() + Km[:3].sum()) / (3.0 * V), (W[:3].sum() + K[:3].sum()) / (3.0 * V)
    print("P_mol = %.4f, P_atom = %.4f; tr K_mol = %.1f, tr K = %.1f" % (P_mol, P_atom, Km[:3].sum(), K[:3].sum()))
    assert abs(Wm[:3].sum() - (-1997.94)) <= 0.01 and abs(W[:3].sum() - (-1958.77)) <= 0.01
    assert abs(P_mol - (-1.2076)) <= 1e-4 and abs(P_atom - (-0.8291)) <= 1e-4
    # the atomic scale does not have tr W_mol as its derivative
    Ua = [_total(B, sr.LO + mu * (B["unwrapped"] - sr.LO), mu * sr.LENGTHS)["e"].sum() for mu in (1.0 + H, 1.0 - H)]
    fda = -(Ua[0] - Ua[1]) / (2.0 * H)
    assert abs(fda - W[:3].sum()) <= FD_BOUND * abs(W[:3].sum()) and abs(fda - Wm[:3].sum()) > 1e-3 * abs(Wm[:3].sum())


def test_scale_translates_molecules_and_scales_single_atoms_and_momenta():
    B = sr.water_box()
    mol, mass = B["mol"][:120], B["mass"]
    mu = np.array([1.013, 0.991, 1.004])
    x, v, ln = mr.scale(B["unwrapped"], B["vel"], sr.LO, sr.LENGTHS, mu, mol, mass, 0.5)
    assert np.array_equal(ln, mu * sr.LENGTHS)
    single = np.arange(360, 450)
    assert np.array_equal(x[single], sr.LO + mu * (B["unwrapped"][single] - sr.LO)) and np.array_equal(v[single], 0.5 * B["vel"][single])
    Y0, V0, _, d0 = mr.centres(B["unwrapped"], B["vel"], mol, mass)
    Y1, V1, _, d1 = mr.centres(x, v, mol, mass)
    assert np.abs(Y1 - (sr.LO + mu * (Y0 - sr.LO))).max() <= 1e-14 * np.abs(Y0).max()
    assert np.abs(d1 - d0).max() <= 1e-15 and np.abs(V1 - 0.5 * V0).max() <= 1e-15
    rel0, rel1 = B["vel"][mol] - V0[:, None], v[mol] - V1[:, None]
    assert np.abs(rel1 - rel0).max() <= 1e-15
    # without a table the sums are the atomic ones
    f, t = np.ones((450, 3)), np.ones((450, 6))
    Wm, Km = mr.molecular_sums(B["unwrapped"], B["vel"], f, t, np.zeros((0, 3), dtype=np.int64), mass)
    assert np.array_equal(Wm, t.sum(axis=0)) and np.array_equal(Km, mr.kinetic_sums(B["vel"], mass))
