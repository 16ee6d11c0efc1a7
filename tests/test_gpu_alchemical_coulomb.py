"""GPU tests of the Coulomb stage of the alchemical table (include/emdee_hip.h: emdee_md_set_alchemical_coulomb,
emdee_md_set_lambda_coulomb, emdee_md_alchemical_coulomb_read, emdee_md_alchemical_coulomb_log_read): on a reaction-field engine the
launch behind every force pass forms the soft-core charge term of the cross pairs beside the Lennard-Jones one.  The yardsticks are
the numpy restatements tests/helpers/alchemical_ref.py (Lennard-Jones) and tests/helpers/alchemical_coulomb_ref.py (every Coulomb
pair of the box, the cross pairs through the soft core), O(N^2) sums over the positions emdee_md_get_state returns.

The box: 864 Lennard-Jones atoms at rho* = 0.8, rc = 2.5 sigma, jittered off the fcc lattice; eight flagged atoms half a box length
apart (no two are neighbours), one of them just above the lower x face and flying at it; every atom charged +-0.4, the box neutral,
the solute's net charge +3.2; eps_rf = inf and one case at 78.  Solute owners (the wavefront path) and environment owners (the thread
path) coexist and a rebuild moves slots.  Tolerances are those of tests/test_gpu_alchemical.py: max error over max entry within 1e-9
(fp64) or 1e-4 (fp32), a read within that of the sum of its terms' sizes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import alchemical_coulomb_ref as qr
from .helpers import alchemical_ref as ar
from .helpers import settle_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
TOL = {np.float64: 1e-9, np.float32: 1e-4}
DT = 0.005
RC, RS, SKIN, ALPHA = 2.5, 2.0, 0.3, 0.5
KC = 1.0                                                   # the Coulomb constant
CASES = [("brick", np.float64, True), ("direct", np.float64, True), ("brick", np.float32, True), ("brick", np.float32, False)]


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _refused(E, code, call, *args, **kw):
    with pytest.raises(E.EmDeeError) as err:
        call(*args, **kw)
    assert err.value.code == code, str(err.value)
    return str(err.value)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _outputs(md):
    """forces, energies, virials, per-atom tensors, the twelve box sums"""
    st = md.state(positions=False, velocities=False, energies=True, virials=True)
    return [_np(st["forces"]), _np(st["energies"]), _np(st["virials"]), _np(md.virial_tensor()), np.array(md.tensor_sums())]


def _xv(md):
    st = md.state(forces=False)
    return _np(st["positions"]), _np(st["velocities"])


def _err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _image(d, L):
    return d - L * np.rint(d / L)


# ---------------------------------------------------------------- the box
_BOX = {}


def _fluid(E):
    if not _BOX:
        pos, L = E.synthetic.fcc_positions(6)
        N = pos.shape[0]
        assert N == 864
        pos = pos.astype(np.float32).astype(np.float64)
        rng = np.random.default_rng(211)
        mass = rng.uniform(1.0, 3.0, N)
        low = np.where((pos[:, 0] > 0.02) & (pos[:, 0] < 0.2))[0]
        flyer = int(low[0])
        flag = np.zeros(N, dtype=np.int32)
        for off in [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]:
            d = _image(pos - (pos[flyer] + 0.5 * L * np.array(off)), L)
            flag[int(np.argmin((d * d).sum(axis=1)))] = 1
        sol = np.where(flag == 1)[0]
        assert len(sol) == 8 and flag[flyer] == 1
        dd = _image(pos[sol][:, None, :] - pos[sol][None, :, :], L)
        assert np.sqrt((dd * dd).sum(axis=2))[~np.eye(8, dtype=bool)].min() > RC + SKIN + 0.7
        q = np.full(N, -0.4)
        q[sol] = 0.4
        env = np.where(flag == 0)[0]
        q[rng.permutation(env)[:424]] = 0.4                            # 8 + 424 positive, 432 negative
        assert abs(q.sum()) < 1e-12 and abs(q[sol].sum() - 3.2) < 1e-12 and (np.abs(q) == 0.4).all()
        vel = E.synthetic.velocities(N) / np.sqrt(mass)[:, None]
        vel[flyer, 0] = -3.0
        atoms = E.lennard_jones_atoms(np.where(flag == 1, 0.7, 1.0), np.where(flag == 1, 1.2, 1.0))
        _BOX.update(pos=pos, L=L, vel=vel, mass=mass, flag=flag, flyer=flyer, atoms=atoms, q=q, sol=sol)
    return _BOX


def _md(E, dev, B, dtype=np.float64, masses=True, pos=None, vel=None):
    im = E.cu((1.0 / B["mass"]).astype(dtype), dev) if masses else None
    pos = B["pos"] if pos is None else pos
    vel = B["vel"] if vel is None else vel
    return E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), float(B["L"]),
                            E.LennardJonesModel(RC, RS), E.cu(B["atoms"], dev), skin=SKIN, inv_mass=im, lo=[0.0, 0.0, 0.0],
                            lengths=[float(B["L"])] * 3, periodic=[1, 1, 1])


def _engine(E, dev, B, dtype=np.float64, masses=True, lam=None, lam_q=None, beta=0.3, eps_rf=np.inf, q=None, foreign=(), foreign_q=(),
            pos=None, vel=None, **kw):
    """a charged engine; lam: with the table; lam_q: with the stage"""
    md = _md(E, dev, B, dtype=dtype, masses=masses, pos=pos, vel=vel)
    md.set_coulomb_(B["q"] if q is None else q, KC, eps_rf=eps_rf)
    if lam is not None:
        md.set_alchemical_(B["flag"], lam=lam, alpha=ALPHA, foreign=foreign, **kw)
    if lam_q is not None:
        md.set_alchemical_coulomb_(lam_q, beta, foreign_q=foreign_q)
    return md


def _reference(B, x, lam, lam_q, beta, eps_rf=np.inf, alpha=ALPHA):
    lj = ar.system(x, [B["L"]] * 3, RC, RS, B["atoms"]["half_sigma"], B["atoms"]["twice_sqrt_eps"], B["flag"], lam, alpha)
    cq = qr.system(x, [B["L"]] * 3, B["flag"], B["q"], KC, RC, eps_rf, lam_q, beta)
    return lj, cq


def _check(md, B, lam, lam_q, beta, dtype, what, eps_rf=np.inf, mass=None, alpha=ALPHA):
    """Every output against numpy at the engine's own positions: the rule of tests/test_gpu_alchemical.py _check_planes with the
    Coulomb addends in the size of every plane, the five Lennard-Jones words as there, and the four Coulomb words within the
    tolerance of the sums of their terms' sizes."""
    tol = TOL[dtype]
    out = _outputs(md)
    x, v = _xv(md)
    lj, cq = _reference(B, x, lam, lam_q, beta, eps_rf, alpha)
    want = [lj[k] + cq[k] for k in ("forces", "energies", "virials", "tensors")]
    for name, got, w in zip(("forces", "energies", "virials", "tensors"), out[:4], want):
        err = _err(got, w)
        print("%s, (%.2f, %.2f, %.2f), %s: max error / max entry = %.3e (bound %.0e)" % (what, lam, lam_q, beta, name, err, tol))
        assert np.isfinite(got).all() and err <= tol, (what, name)
    total = out[0].sum(axis=0)
    assert np.abs(want[0].sum(axis=0)).max() <= 1e-11 * np.abs(want[0]).max()
    assert np.abs(total).max() <= tol * np.abs(want[0]).max()
    # the box sums: emdee_md_pressure_tensor (W from the tensors, K from the velocities) and emdee_md_energies
    m = B["mass"] if mass is None else mass
    K = np.array([(m * v[:, a] * v[:, b]).sum() for a, b in ar.COMPONENTS])
    wsum = want[3].sum(axis=0)
    assert np.abs(out[4][:6] - wsum).max() <= 10 * tol * np.abs(wsum).max()
    assert np.abs(out[4][6:] - K).max() <= 10 * tol * np.abs(K).max()
    ep, ek, wt = md.totals()
    assert abs(ep - want[1].sum()) <= 10 * tol * np.abs(want[1]).sum() and abs(wt - want[2].sum()) <= 10 * tol * np.abs(want[2]).sum()
    assert abs(ek - 0.5 * K[:3].sum()) <= 10 * tol * 0.5 * K[:3].sum()
    # the five Lennard-Jones words: unchanged in layout and meaning
    read = md.alchemical()
    assert read["lam"] == lam and read["pairs"] == lj["pairs"] == cq["pairs"] and lj["pairs"] > 300, (read["pairs"], lj["pairs"])
    for key, r, size in (("U", lj["U"], lj["sizes"][0]), ("dUdl", lj["dUdl"], lj["sizes"][1]), ("virial", lj["W"], lj["sizes"][2])):
        assert abs(read[key] - r) <= tol * size, (what, key, read[key], r)
    # the four Coulomb words
    rq = md.alchemical_coulomb()
    assert rq["lam_q"] == lam_q
    for key, r, size in (("U", cq["U"], cq["sizes"][0]), ("dUdl", cq["dUdl"], cq["sizes"][1]), ("virial", cq["W"], cq["sizes"][2])):
        print("%s, read Coulomb %s: %.9g against %.9g (size %.3g)" % (what, key, rq[key], r, size))
        assert abs(rq[key] - r) <= tol * size, (what, key, rq[key], r)
    if lam_q == 0.0:
        assert rq["U"] == 0.0 and rq["virial"] == 0.0 and rq["dUdl"] != 0.0
    return out


# ---------------------------------------------------------------- 1. planes and words against numpy
@pytest.mark.parametrize("path,dtype,masses", CASES)
def test_planes_and_words_at_the_load_after_a_rebuild_and_a_face_match_numpy(emdee, dev, monkeypatch, path, dtype, masses):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    B = _fluid(E)
    what = "%s/%s%s" % (path, dtype.__name__, "" if masses else "/no masses")
    mass = B["mass"] if masses else np.ones(len(B["mass"]))
    md = _engine(E, dev, B, dtype=dtype, masses=masses, lam=0.6, lam_q=0.35, beta=0.3)
    settings = ((0.6, 0.35, 0.3), (1.0, 0.5, 0.0))

    def both(where):
        for lam, lam_q, beta in settings:
            md.set_lambda_(lam)
            md.set_alchemical_coulomb_(lam_q, beta)
            _check(md, B, lam, lam_q, beta, dtype, what + where, mass=mass)
    both(" at the load")
    builds, image0 = md.nbr_stats()["builds"], np.floor(B["pos"] / B["L"])
    md.set_lambda_(0.6)
    md.set_alchemical_coulomb_(0.35, 0.3)
    md.step_(40, DT)
    x, _ = _xv(md)
    crossed = (np.floor(x / B["L"]) != image0).any(axis=1) & (B["flag"] == 1)
    assert crossed.any() and md.nbr_stats()["builds"] > builds, (crossed.sum(), md.nbr_stats())
    assert np.isfinite(x).all() and np.abs(x - B["pos"]).max() < 2.0
    both(" after 40 steps")
    md.close()


def test_planes_and_words_on_a_finite_reaction_field_dielectric(emdee, dev):
    E = emdee
    B = _fluid(E)
    md = _engine(E, dev, B, lam=0.6, lam_q=0.35, beta=0.3, eps_rf=78.0)
    _check(md, B, 0.6, 0.35, 0.3, np.float64, "eps_rf 78", eps_rf=78.0)
    md.step_(10, DT)
    _check(md, B, 0.6, 0.35, 0.3, np.float64, "eps_rf 78 after 10 steps", eps_rf=78.0)
    md.close()


# ---------------------------------------------------------------- 2., 3. against the engine itself
@pytest.mark.parametrize("path,dtype,masses", CASES[:3])
def test_both_lambdas_at_one_are_the_charged_engine_without_a_table_for_any_beta(emdee, dev, monkeypatch, path, dtype, masses):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    B = _fluid(E)
    tol = TOL[dtype]
    plain = _engine(E, dev, B, dtype=dtype)
    want = _outputs(plain)
    plain.close()
    md = _engine(E, dev, B, dtype=dtype, lam=1.0, lam_q=1.0, beta=0.0)
    for beta in (0.0, 0.3, 2.0):
        md.set_alchemical_coulomb_(1.0, beta)
        for name, a, b in zip(("forces", "energies", "virials", "tensors", "sums"), _outputs(md), want):
            err = _err(a, b)
            print("%s/%s beta %.1f against no table, %s: %.3e (bound %.0e)" % (path, dtype.__name__, beta, name, err, tol))
            assert err <= tol, (name, beta)
    md.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lambda_q_zero_is_numerically_the_twin_whose_solute_charges_were_zeroed(emdee, dev, dtype):
    E = emdee
    B = _fluid(E)
    q0 = B["q"].copy()
    q0[B["flag"] == 1] = 0.0
    md = _engine(E, dev, B, dtype=dtype, lam=0.6, lam_q=0.0, beta=0.3)
    twin = _engine(E, dev, B, dtype=dtype, lam=0.6, q=q0)             # (never sets the stage)
    for where in ("at the load", "after 5 steps"):
        for name, a, b in zip(("forces", "energies", "virials", "tensors", "sums"), _outputs(md), _outputs(twin)):
            assert np.array_equal(a, b), (where, name, np.abs(a - b).max())
        for a, b in zip(_xv(md), _xv(twin)):
            assert np.array_equal(a, b), where
        rq = md.alchemical_coulomb()
        assert rq["U"] == 0.0 and rq["virial"] == 0.0 and rq["dUdl"] != 0.0 and np.isfinite(rq["dUdl"])
        md.step_(5, DT)
        twin.step_(5, DT)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 4. dU/dlambda_q as a difference
def test_dUdlambda_q_is_the_centred_difference_of_U_q_through_set_lambda_coulomb(emdee, dev):
    """The rule of test_dUdlambda_is_the_centred_difference_of_U_alch_through_set_lambda: at fixed positions
    (U_q(lambda_q + h) - U_q(lambda_q - h)) / 2h errs by h^2 / 6 |U_q'''| -- from the fp64 yardstick's sum over the cross pairs by a
    five-point stencil of step 2 h, doubled for the stencil's own error -- plus the rounding of the two reads, 1e-9 (the tolerance of
    a read) of the size of U_q before cancellation, over 2 h.  The Lennard-Jones words do not depend on lambda_q: the same bits."""
    E = emdee
    B = _fluid(E)
    beta = 0.3
    md = _engine(E, dev, B, lam=0.6, lam_q=0.5, beta=beta)
    x, _ = _xv(md)
    words = lambda lq: qr.cross_words(x, [B["L"]] * 3, B["flag"], B["q"], KC, RC, np.inf, lq, beta)
    U = lambda lq: words(lq)[0]
    lj0 = md.alchemical()
    h = 2.0 ** -7
    for lam_q in (0.2, 0.5, 0.8):
        md.set_lambda_coulomb_(lam_q)
        here = md.alchemical_coulomb()
        lj = md.alchemical()
        assert all(lj[k] == lj0[k] for k in ("lam", "U", "dUdl", "virial", "pairs")), (lam_q, lj, lj0)
        md.set_lambda_coulomb_(lam_q + h)
        up = md.alchemical_coulomb()["U"]
        md.set_lambda_coulomb_(lam_q - h)
        dn = md.alchemical_coulomb()["U"]
        k = 2 * h
        third = max(abs(U(c + 2 * k) - 2 * U(c + k) + 2 * U(c - k) - U(c - 2 * k)) / (2 * k ** 3) for c in (lam_q - k, lam_q, lam_q + k))
        size = words(lam_q + h)[3]
        bound = 2.0 * h * h / 6.0 * third + 2 * TOL[np.float64] * size / (2 * h)
        slope = (up - dn) / (2 * h)
        print("lambda_q %.2f: dU/dlambda_q read %.9g, centred difference %.9g, bound %.3e" % (lam_q, here["dUdl"], slope, bound))
        assert here["lam_q"] == lam_q and abs(slope - here["dUdl"]) <= bound
    md.close()


# ---------------------------------------------------------------- 5. foreign energies
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_foreign_energies_of_both_reads_are_the_reads_of_twins_at_those_states(emdee, dev, dtype):
    E = emdee
    B = _fluid(E)
    foreign, foreign_q = [0.0, 0.4, 1.0], [0.0, 0.7, 1.0]
    md = _engine(E, dev, B, dtype=dtype, lam=0.6, lam_q=0.35, beta=0.3, foreign=foreign, foreign_q=foreign_q)
    twin = _engine(E, dev, B, dtype=dtype, lam=0.6, lam_q=0.35, beta=0.3)
    got, got_q = md.alchemical()["foreign"], md.alchemical_coulomb()["foreign"]
    assert got.shape == (3,) and got_q.shape == (3,)
    x, _ = _xv(md)
    r2, s2, e4 = ar.cross_pairs(x, [B["L"]] * 3, RC, B["atoms"]["half_sigma"], B["atoms"]["twice_sqrt_eps"], B["flag"])
    for k, (lam, lam_q) in enumerate(zip(foreign, foreign_q)):
        twin.set_lambda_(lam)
        twin.set_lambda_coulomb_(lam_q)
        want, want_q = twin.alchemical()["U"], twin.alchemical_coulomb()["U"]
        size = float(np.abs(ar.pair(r2, RC, RS, s2, e4, lam, ALPHA)[0]).sum())
        size_q = qr.cross_words(x, [B["L"]] * 3, B["flag"], B["q"], KC, RC, np.inf, lam_q, 0.3)[3]
        print("foreign state %d: U %.9g / %.9g, U_q %.9g / %.9g" % (k, got[k], want, got_q[k], want_q))
        assert abs(got[k] - want) <= TOL[dtype] * max(size, 1e-300), (k, got[k], want)
        assert abs(got_q[k] - want_q) <= TOL[dtype] * max(size_q, 1e-300), (k, got_q[k], want_q)
    assert got[0] == 0.0 and got_q[0] == 0.0 and abs(got_q[2]) > 0.1
    md.close()
    twin.close()


# ---------------------------------------------------------------- 6. overlap
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_flagged_atom_exactly_on_an_unflagged_atom_of_opposite_charge(emdee, dev, dtype):
    """an input the term is defined on: rho2 = beta (1 - lambda_q) > 0 at r = 0, the coincident pair exerts no force"""
    E = emdee
    B = _fluid(E)
    pos = B["pos"].copy()
    s = int(B["sol"][3])
    free = np.where((B["flag"] == 0) & (B["q"] < 0.0))[0]
    d = _image(pos[free] - pos[s], B["L"])
    on = int(free[np.argmax((d * d).sum(axis=1))])                    # (from far away: its old neighbours lose it, no new overlap but this one)
    pos[on] = pos[s]
    assert (pos[on] == pos[s]).all() and B["q"][on] * B["q"][s] < 0.0
    md = _md(E, dev, B, dtype=dtype, pos=pos, vel=np.zeros_like(pos))
    md.set_alchemical_(B["flag"], lam=0.5, alpha=0.5)
    md.set_coulomb_(B["q"], KC)
    md.set_alchemical_coulomb_(0.5, 0.3)
    _check(md, B, 0.5, 0.5, 0.3, dtype, "overlap/%s" % dtype.__name__, alpha=0.5)
    md.step_(5, 0.001)
    x, v = _xv(md)
    assert np.isfinite(x).all() and np.isfinite(v).all() and all(np.isfinite(a).all() for a in _outputs(md))
    rq = md.alchemical_coulomb()
    assert all(np.isfinite(rq[k]) for k in ("U", "dUdl", "virial"))
    md.close()


# ---------------------------------------------------------------- 7. reproducibility
def _bits(md):
    r, rq = md.alchemical(), md.alchemical_coulomb()
    log, logq = md.alchemical_log(), md.alchemical_coulomb_log()
    reads = np.array([r["lam"], r["U"], r["dUdl"], r["virial"], float(r["pairs"]), rq["lam_q"], rq["U"], rq["dUdl"], rq["virial"]]).tobytes()
    reads += r["foreign"].tobytes() + rq["foreign"].tobytes()
    logs = b"".join(l[k].tobytes() for l in (log, logq) for k in ("dUdl", "U", "foreign"))
    return reads, logs, (log["count"], log["dropped"], logq["count"], logq["dropped"])


def test_dealing_of_steps_fresh_engines_and_a_cleared_stage(emdee, dev):
    E = emdee
    B = _fluid(E)
    foreign, foreign_q = [0.0, 0.4, 1.0], [0.0, 0.7, 1.0]
    ends = []
    for deal in ((40,), (5,) * 8, (1,) * 40, (40,)):                   # (the last: a second fresh engine)
        md = _engine(E, dev, B, lam=0.6, lam_q=0.35, beta=0.3, foreign=foreign, foreign_q=foreign_q, log_every=4, log_capacity=16)
        for n in deal:
            md.step_(n, DT)
        ends.append((md.state(),) + _bits(md))
        md.close()
    assert ends[0][3] == (10, 0, 10, 0)
    for other in ends[1:]:
        for key in ("positions", "velocities", "forces"):
            assert torch.equal(ends[0][0][key], other[0][key]), key
        assert ends[0][1] == other[1] and ends[0][2] == other[2] and ends[0][3] == other[3]
    # the stage set and cleared: the table-only engine's bits, and its refusal of the charged solute
    md, twin = _engine(E, dev, B, lam=0.6, lam_q=0.35, beta=0.3), _engine(E, dev, B, lam=0.6)
    md.set_alchemical_coulomb_(None)
    for name, a, b in zip(("forces", "energies", "virials", "tensors", "sums"), _outputs(md), _outputs(twin)):
        assert np.array_equal(a, b), name
    assert _bits_lj(md) == _bits_lj(twin)
    for eng in (md, twin):
        text = _refused(E, ERR_STATE, eng.step_, 1, DT)
        assert "atom %d " % B["sol"][0] in text and "emdee_md_set_coulomb" in text and "Lennard-Jones coupling only" in text
    with pytest.raises(RuntimeError):
        md.alchemical_coulomb()
    md.close()
    twin.close()


def _bits_lj(md):
    r = md.alchemical()
    return np.array([r["lam"], r["U"], r["dUdl"], r["virial"], float(r["pairs"])]).tobytes()


# ---------------------------------------------------------------- 8. the logs
@pytest.mark.parametrize("samples", [4, 7])
def test_entries_of_both_logs_are_the_reads_of_a_twin(emdee, dev, samples):
    """capacity 5: fewer samples than it, and more"""
    E = emdee
    B = _fluid(E)
    every, cap = 3, 5
    foreign, foreign_q = [0.0, 0.4, 1.0], [0.0, 0.7, 1.0]
    kw = dict(lam=0.6, lam_q=0.35, beta=0.3, foreign=foreign, foreign_q=foreign_q)
    md = _engine(E, dev, B, log_every=every, log_capacity=cap, **kw)
    twin = _engine(E, dev, B, **kw)
    md.step_(every * samples + 2, DT)                                 # (two steps past the last sample: they add none)
    rows, rows_q = [], []
    for _ in range(samples):
        twin.step_(every, DT)
        r, rq = twin.alchemical(), twin.alchemical_coulomb()
        rows.append([r["dUdl"], r["U"]] + list(r["foreign"]))
        rows_q.append([rq["dUdl"], rq["U"]] + list(rq["foreign"]))
    kept = min(samples, cap)
    for log, want in ((md.alchemical_log(), rows), (md.alchemical_coulomb_log(), rows_q)):
        assert (log["count"], log["dropped"]) == (kept, samples - kept)
        got = np.concatenate([log["dUdl"][:, None], log["U"][:, None], log["foreign"]], axis=1)
        assert got.shape == (kept, 2 + len(foreign)) and np.array_equal(got, np.array(want)[:kept])
    assert np.abs(np.array(rows_q)[:, :2]).min() > 0.0 and twin.alchemical_coulomb_log()["count"] == 0
    # setting the stage again restarts the table's step count and both logs
    md.set_alchemical_coulomb_(0.35, 0.3, foreign_q=foreign_q)
    assert md.alchemical_log()["count"] == 0 and md.alchemical_coulomb_log()["count"] == 0 and md.alchemical_log()["dropped"] == 0
    md.step_(every, DT)
    assert md.alchemical_log()["count"] == 1 and md.alchemical_coulomb_log()["count"] == 1
    md.close()
    twin.close()


# ---------------------------------------------------------------- 9. rigid water
def test_a_flagged_rigid_water_keeps_its_charges_under_c_rescale_with_molecular_scaling(emdee, dev):
    E = emdee
    lengths, lo = np.array([6.0, 6.2, 6.6]), np.array([-1.0, 0.5, 2.0])
    B = sr.water_box(n_mol=64, lengths=lengths, lo=lo)
    N = B["pos"].shape[0]
    assert N == 192
    flag = np.zeros(N, dtype=np.int32)
    flag[B["mol"][3]] = 1                                              # a whole molecule: its internal pairs are excluded, not cross
    md = E.VelocityVerlet(E.cu(B["pos"], dev), E.cu(B["vel"], dev), float(lengths[0]), E.LennardJonesModel(sr.RC, sr.RS),
                          E.cu(B["atoms"], dev), skin=sr.SKIN, inv_mass=E.cu(1.0 / B["mass"], dev), lo=list(lo), lengths=list(lengths),
                          periodic=[1, 1, 1])
    md.set_exclusions_(B["excl"])
    md.set_rigid3_(B["mol"], B["geom"])
    md.set_coulomb_(B["charges"], KC, eps_rf=78.0)
    md.set_molecular_scaling_()
    md.set_alchemical_(flag, lam=0.8, alpha=ALPHA)
    md.set_alchemical_coulomb_(0.6, 0.05)
    md.set_barostat_("c-rescale", p_ref=1.0, compressibility=0.05, tau_p=0.5, every=5, temperature=1.0, seed=7)
    md.step_(10, sr.DT)                                               # two events
    box = np.array(md.box()[1])
    assert not np.array_equal(box, lengths)
    x, v = _xv(md)
    assert np.isfinite(x).all() and np.isfinite(v).all()
    rq = md.alchemical_coulomb()
    i, j, d = qr.cross_pairs(x, box, flag, sr.RC)
    k_rf, c_rf = qr.rf_constants(sr.RC, 78.0)
    U, W, dl, _ = qr.pair((d * d).sum(axis=1), KC * B["charges"][i] * B["charges"][j], k_rf, c_rf, 0.6, 0.05)
    print("rigid water: %d cross pairs, W_q %.9g against %.9g, U_q %.9g against %.9g" % (len(i), rq["virial"], W.sum(), rq["U"], U.sum()))
    assert len(i) > 100 and md.alchemical()["pairs"] == len(i)
    assert abs(rq["virial"] - W.sum()) <= 1e-9 * np.abs(W).sum()
    assert abs(rq["U"] - U.sum()) <= 1e-9 * np.abs(U).sum() and abs(rq["dUdl"] - dl.sum()) <= 1e-9 * np.abs(dl).sum()
    # the trace of the atomic virial moves by the cross Coulomb virial when the stage goes from lambda_q = 0 to its value
    on = np.array(md.tensor_sums())
    md.set_lambda_coulomb_(0.0)
    off = np.array(md.tensor_sums())
    assert abs((on[:3] - off[:3]).sum() - rq["virial"]) <= 1e-9 * np.abs(on[:3]).sum()
    assert np.isfinite(np.array(md.molecular_tensor_sums())).all()
    md.close()


# ---------------------------------------------------------------- 10. refusals
def test_every_refusal_leaves_the_previous_stage_in_force(emdee, dev):
    import ctypes as C
    E = emdee
    B = _fluid(E)
    foreign, foreign_q = [0.0, 0.4, 1.0], [0.0, 0.7, 1.0]
    md = _engine(E, dev, B, lam=0.6, lam_q=0.35, beta=0.3, foreign=foreign, foreign_q=foreign_q, log_every=2, log_capacity=4)
    bits = _bits(md)
    raw = lambda lq, beta, f, nf: E._lib.call("emdee_md_set_alchemical_coulomb", md._handle, 1, lq, beta,
                                              None if f is None else f.ctypes.data_as(C.c_void_p), nf)
    three = np.array(foreign_q)
    cases = [
        ("lambda_q above", lambda: md.set_alchemical_coulomb_(1.01, 0.3, foreign_q=foreign_q), "lambda_q = 1.01"),
        ("lambda_q below", lambda: md.set_alchemical_coulomb_(-0.2, 0.3, foreign_q=foreign_q), "lambda_q = -0.2"),
        ("lambda_q nan", lambda: md.set_alchemical_coulomb_(np.nan, 0.3, foreign_q=foreign_q), "lambda_q = nan"),
        ("a foreign lambda_q outside", lambda: md.set_alchemical_coulomb_(0.5, 0.3, foreign_q=[0.5, 1.5, 0.2]), "foreign lambda_q 1 = 1.5"),
        ("a foreign lambda_q nan", lambda: md.set_alchemical_coulomb_(0.5, 0.3, foreign_q=[0.5, 0.5, np.nan]), "foreign lambda_q 2 = nan"),
        ("beta < 0", lambda: md.set_alchemical_coulomb_(0.5, -0.1, foreign_q=foreign_q), "beta = -0.1"),
        ("beta nan", lambda: md.set_alchemical_coulomb_(0.5, np.nan, foreign_q=foreign_q), "beta = nan"),
        ("beta inf", lambda: md.set_alchemical_coulomb_(0.5, np.inf, foreign_q=foreign_q), "beta = inf"),
        ("another n_foreign", lambda: md.set_alchemical_coulomb_(0.5, 0.3, foreign_q=[0.5, 0.6]), "n_foreign = 2"),
        ("no foreign_q", lambda: md.set_alchemical_coulomb_(0.5, 0.3), "n_foreign = 0"),
        ("NULL foreign_q", lambda: raw(0.5, 0.3, None, 3), "NULL"),
    ]
    for name, call, word in cases:
        text = _refused(E, ERR_INVALID, call)
        assert "set_alchemical_coulomb" in text and word in text, (name, text)
        assert _bits(md) == bits, name
    raw(0.35, 0.3, three, 3)                                          # (the raw call with an array sets the stage: the logs restart)
    bits = _bits(md)
    for lam_q in (-0.5, 1.5, np.nan):
        text = _refused(E, ERR_INVALID, md.set_lambda_coulomb_, lam_q)
        assert "set_lambda_coulomb" in text and "lambda_q = " in text and _bits(md) == bits
    md.step_(4, DT)                                                   # the stage in force still steps and logs
    assert md.alchemical_coulomb_log()["count"] == 2 and md.alchemical_coulomb()["lam_q"] == 0.35
    # Ewald and PME with a charged flagged atom: refused at the set with the sum on ...
    for method, setter, on, off in (("Ewald summation", "emdee_md_set_ewald", lambda: md.set_ewald_(1.2, 6), lambda: md.set_ewald_(0.0, 6)),
                                    ("particle-mesh Ewald", "emdee_md_set_pme", lambda: md.set_pme_(1.2, (32, 32, 32), 4),
                                     lambda: md.set_pme_(0.0, (32, 32, 32), 4))):
        # ... the stage set first, the sum after it: the readiness check of step and minimize refuses
        on()
        for call, args in ((md.step_, (1, DT)), (md.minimize_, (3, 1.0))):
            text = _refused(E, ERR_STATE, call, *args)
            assert "atom %d " % B["sol"][0] in text and "emdee_md_set_alchemical_coulomb" in text and setter in text and method in text, text
        # ... the sum on, the stage set after it: refused at the set, the previous stage in force
        text = _refused(E, ERR_STATE, md.set_alchemical_coulomb_, 0.5, 0.1, foreign_q=foreign_q)
        assert "atom %d " % B["sol"][0] in text and "emdee_md_set_alchemical_coulomb" in text and setter in text, text
        off()
        assert md.alchemical_coulomb()["lam_q"] == 0.35
        md.step_(1, DT)
    # with zero solute charges PME keeps working, the stage on
    q0 = B["q"].copy()
    q0[B["flag"] == 1] = 0.0
    q0[B["flag"] == 0] -= q0.sum() / (B["flag"] == 0).sum()
    md.set_coulomb_(q0, KC)
    md.set_pme_(1.2, (32, 32, 32), 4)
    md.step_(2, DT)
    rq = md.alchemical_coulomb()
    assert rq["U"] == 0.0 and rq["dUdl"] == 0.0 and rq["virial"] == 0.0
    md.set_pme_(0.0, (32, 32, 32), 4)
    # clearing the charges leaves the stage set but inert: the words read 0, the engine steps
    md.set_coulomb_(None, KC)
    rq = md.alchemical_coulomb()
    assert rq["lam_q"] == 0.35 and rq["U"] == 0.0 and rq["dUdl"] == 0.0 and rq["virial"] == 0.0 and (rq["foreign"] == 0.0).all()
    md.step_(2, DT)
    assert np.isfinite(md.alchemical()["U"])
    # ... and no charges at the set: refused
    md.set_alchemical_coulomb_(None)
    text = _refused(E, ERR_STATE, md.set_alchemical_coulomb_, 0.5, 0.3, foreign_q=foreign_q)
    assert "emdee_md_set_coulomb" in text and "set_alchemical_coulomb" in text
    # a new table (set or clear) clears the stage; without a table the set and the reads refuse
    md.set_coulomb_(B["q"], KC)
    md.set_alchemical_coulomb_(0.5, 0.3, foreign_q=foreign_q)
    md.set_alchemical_(B["flag"], lam=0.6, alpha=ALPHA)
    out = np.zeros(32)
    for name, args in (("emdee_md_alchemical_coulomb_read", (out.ctypes.data_as(C.c_void_p),)), ("emdee_md_set_lambda_coulomb", (0.5,)),
                       ("emdee_md_alchemical_coulomb_log_read", (None, None, None))):
        with pytest.raises(E.EmDeeError) as err:
            E._lib.call(name, md._handle, *args)
        assert err.value.code == ERR_STATE and "emdee_md_set_alchemical_coulomb" in str(err.value), name
    md.set_alchemical_(None)
    text = _refused(E, ERR_STATE, md.set_alchemical_coulomb_, 0.5, 0.3)
    assert "emdee_md_set_alchemical" in text and "no alchemical table" in text
    md.set_alchemical_coulomb_(None)                                  # (enable = 0: nothing is looked at)
    md.step_(1, DT)
    md.close()


def test_the_stage_with_ghosts_and_on_a_lent_engine(emdee, dev):
    from .test_gpu_dd_pairs import _build
    E = emdee
    B = _fluid(E)
    N = B["pos"].shape[0]
    md = _engine(E, dev, B, lam=0.6)
    # the last 64 atoms loaded as ghosts: the table stays (for another count), the stage is refused
    md.set_state_(E.cu(B["pos"], dev), E.cu(B["vel"][:N - 64], dev), E.cu(B["atoms"], dev), inv_mass=E.cu(1.0 / B["mass"][:N - 64], dev), n_ghost=64)
    text = _refused(E, ERR_STATE, md.set_alchemical_coulomb_, 0.5, 0.3)
    assert "ghosts" in text and "set_alchemical_coulomb" in text
    md.close()
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)
    pos = pos[np.argsort(gid)]
    n = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((n, 3)), E.lennard_jones_atoms(1.0, 1.0, n), float(lengths[0]))
    eng = dd.engine(0)
    text = _refused(E, ERR_STATE, eng.set_alchemical_coulomb_, 0.5, 0.3)
    assert "emdee_dd_engine" in text and "set_alchemical_coulomb" in text
    dd.step_(2, DT)
    dd.close()


# ---------------------------------------------------------------- 11. the example
def test_the_example_runs_at_its_small_size(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "charged_solvation.py"), "--molecules", "64", "--melt", "100",
                        "--windows", "3", "--equil", "20", "--steps", "60", "--every", "10"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-1600:]
    rows = [line.split() for line in r.stdout.splitlines() if line and not line.startswith("#")]
    # three Coulomb windows, three Lennard-Jones windows, the two integrals, then the foreign-energy differences of both stages
    assert len(rows) == 3 + 3 + 2 + 2 * 2 and all(int(row[4]) == 6 for row in rows[:6]), r.stdout[-1200:]
    assert all(np.isfinite(float(t)) for row in rows for t in row[1:])
    assert rows[0][0] == "coulomb" and rows[3][0] == "lj" and float(rows[2][1]) == 0.0 and float(rows[5][1]) == 0.0
