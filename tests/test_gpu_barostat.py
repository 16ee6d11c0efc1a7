"""GPU tests of pressure coupling (include/emdee_hip.h: emdee_md_get_box, emdee_md_scale_box, emdee_md_set_barostat) against
the numpy yardstick of tests/helpers/barostat_ref.py, on the tiled and the direct kernels.

The base box is the 864-atom fluid of the bonded and orthorhombic tests after a short melt on the host (barostat_ref.fluid864):
L = 10.26 sigma at rc + skin = 2.8 is three cells per side, the smallest box in which a scale can change a cell count (3 -> 4
along x at mu = 1.10) while another axis stays and a third shrinks.  Tolerances are the project's: fp64 per-atom outputs of two
engines on the same positions 1e-12 of the largest component, against the numpy sums 1e-9, fp32 outputs 1e-4
(tests/test_gpu_orthorhombic.py: TOL), fp64 trajectories against the numpy integrator 1e-8 in position and velocity."""
import ctypes as C

import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import bonded_ref as br
from .helpers import ortho_ref as oref
from .test_gpu_bonded import _outputs
from .test_gpu_dd_pairs import _build

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
RC, RS, SKIN, DT = bref.RC, bref.RS, bref.SKIN, bref.DT
X64 = 1e-8                                              # tests/test_gpu_bonded.py: test_trajectory_matches_a_numpy_velocity_verlet
F32 = 1e-4                                              # tests/test_gpu_orthorhombic.py: TOL[np.float32]
PATHS = ["tiled", "direct"]


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _path(monkeypatch, path):
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")


def _engine(E, dev, pos, vel, lengths, atoms, dtype=np.float64, lo=(0.0, 0.0, 0.0), rc=RC, rs=RS, skin=SKIN, inv_mass=None):
    im = None if inv_mass is None else E.cu(np.asarray(inv_mass).astype(dtype), dev)
    lengths = [float(v) for v in np.broadcast_to(lengths, 3)]
    return E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), lengths[0],
                            E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=skin, inv_mass=im, lo=list(lo), lengths=lengths,
                            periodic=[1, 1, 1])


def _fluid(E, dev, dtype=np.float64):
    S = bref.fluid864(E.synthetic)
    if dtype == np.float32:
        S["pos"], S["vel"] = S["pos"].astype(np.float32).astype(np.float64), S["vel"].astype(np.float32).astype(np.float64)
    return S, _engine(E, dev, S["pos"], S["vel"], S["L"], S["atoms"], dtype)


def _xv(md):
    st = md.state(forces=False)
    return st["positions"].cpu().numpy(), st["velocities"].cpu().numpy()


def _close_outputs(got, want, tol, what):
    for name, g, w in zip(("forces", "energies", "virials", "tensors", "tensor sums"), got, want):
        scale, err = np.abs(w).max(), np.abs(g - w).max()
        print("%s %s: max err %.3e of max %.3e (tol %.0e)" % (what, name, err, scale, tol))
        assert err <= tol * scale, (what, name, err, scale)


def _image_gap(x, xr, lengths):
    d = np.asarray(x, dtype=np.float64) - xr
    return np.abs(d - lengths * np.rint(d / lengths)).max()


# ---------------------------------------------------------------- 1. the scale primitive
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("path", PATHS)
def test_scale_box_changes_the_cell_count_and_matches_a_fresh_engine(emdee, dev, monkeypatch, path, dtype):
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev, dtype)
    L, mu = S["L"], np.array([1.10, 1.00, 0.95])
    assert int(L // (RC + SKIN)) == 3 and int(1.10 * L // (RC + SKIN)) == 4 and int(0.95 * L // (RC + SKIN)) == 3
    assert md.box() == ([0.0] * 3, [L] * 3)
    x0, v0 = _xv(md)
    builds = md.nbr_stats()["builds"]
    md.scale_box_(mu)
    lo, ln = md.box()
    assert lo == [0.0] * 3 and ln == [m * L for m in mu] and md.lengths == ln          # exactly mu x len
    assert md.nbr_stats()["builds"] == builds + 1
    x1, v1 = _xv(md)
    assert np.array_equal(v1, v0)                                                       # velocity_scale = 1: bit for bit
    want_x = mu * x0.astype(np.float64)
    if dtype == np.float64:
        assert np.abs(x1 - want_x).max() <= 1e-14 * np.abs(want_x).max()
    else:   # the records are rounded once more: one fp32 ulp of the largest coordinate (2^-20 below 16, as a relative bound 2^-23)
        assert np.abs(x1 - want_x).max() <= 2.0 ** -22 * np.abs(want_x).max()
    got = _outputs(md) + [md.pressure_tensor()["pressure"]]
    fresh = _engine(E, dev, x1, v1, ln, S["atoms"], dtype)
    want = _outputs(fresh) + [fresh.pressure_tensor()["pressure"]]
    if dtype == np.float64:
        _close_outputs(got[:5], want[:5], 1e-12, "scaled engine against a fresh one")
        assert np.abs(got[5] - want[5]).max() <= 1e-12 * np.abs(want[5]).max()
        ref = oref.total(x1, np.zeros(3), np.array(ln), [1, 1, 1], RC, RS, S["atoms"])
        _close_outputs(got[:4], [ref["f"], ref["e"], ref["w"], ref["t"]], 1e-9, "scaled engine against the numpy sums")
        Pref = bref.pressure_diagonal(v1, ref["t"], ln)
        assert np.abs(np.diag(got[5]) - Pref).max() <= 1e-9 * np.abs(Pref).max()
    else:
        _close_outputs(got[:5], want[:5], F32, "scaled fp32 engine against a fresh one")
        assert np.abs(got[5] - want[5]).max() <= F32 * np.abs(want[5]).max()
    # the engine steps on from there as the fresh one does
    md.step_(3, DT)
    fresh.step_(3, DT)
    xa, xb = _xv(md)[0], _xv(fresh)[0]
    assert _image_gap(xa, xb.astype(np.float64), np.array(ln)) <= (1e-12 if dtype == np.float64 else 1e-4)
    md.close()
    fresh.close()


# ---------------------------------------------------------------- 2. the velocity scale
@pytest.mark.parametrize("path", PATHS)
def test_velocity_scale_halves_the_velocities_and_leaves_the_rest(emdee, dev, monkeypatch, path):
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    x0, v0 = _xv(md)
    f0 = md.state()["forces"].cpu().numpy()
    ke0 = md.totals()[1]
    md.scale_box_((1.0, 1.0, 1.0), 0.5)
    x1, v1 = _xv(md)
    assert np.array_equal(v1, 0.5 * v0)
    assert md.totals()[1] == pytest.approx(0.25 * ke0, rel=1e-14)
    assert md.box()[1] == [S["L"]] * 3
    assert np.abs(x1 - x0).max() <= 1e-14 * np.abs(x0).max()
    f1 = md.state()["forces"].cpu().numpy()
    assert np.abs(f1 - f0).max() <= 1e-14 * np.abs(f0).max()
    md.close()


# ---------------------------------------------------------------- 3. refusals
def test_a_refused_scale_leaves_the_engine_as_it_was(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    _, twin = _fluid(E, dev)
    x0, v0 = _xv(md)
    builds = md.nbr_stats()["builds"]
    assert 0.5 * S["L"] < 2 * (RC + SKIN)
    bad = [((0.5, 1.0, 1.0), 1.0), ((1.0, np.nan, 1.0), 1.0), ((1.0, 1.0, 0.0), 1.0), ((-1.0, 1.0, 1.0), 1.0), ((np.inf, 1.0, 1.0), 1.0),
           ((1.0, 1.0, 1.0), 0.0), ((1.0, 1.0, 1.0), -2.0), ((1.0, 1.0, 1.0), np.nan), ((1.0, 1.0, 1.0), np.inf)]
    for mu, vs in bad:
        with pytest.raises(E.EmDeeError) as err:
            md.scale_box_(mu, vs)
        assert err.value.code == ERR_INVALID, (mu, vs)
    x1, v1 = _xv(md)
    assert md.box()[1] == [S["L"]] * 3 and md.nbr_stats()["builds"] == builds
    assert np.array_equal(x1, x0) and np.array_equal(v1, v0)
    md.step_(5, DT)
    twin.step_(5, DT)
    for a, b in zip(_xv(md), _xv(twin)):
        assert np.array_equal(a, b)
    md.close()
    twin.close()


def test_invalid_barostat_settings_are_refused_and_the_previous_one_stays(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    _, twin = _fluid(E, dev)
    good = dict(p_ref=5.0, compressibility=0.0, tau_p=1.0, every=2)
    md.set_barostat_(E.BAROSTAT_BERENDSEN, **good)
    twin.set_barostat_(E.BAROSTAT_BERENDSEN, **good)
    B, Cr = E.BAROSTAT_BERENDSEN, E.BAROSTAT_CRESCALE
    bad = [dict(kind=7), dict(kind=-1), dict(coupling=3), dict(coupling=-1), dict(every=0), dict(every=-3), dict(tau_p=0.0),
           dict(tau_p=-1.0), dict(tau_p=np.nan), dict(tau_p=np.inf), dict(p_ref=np.nan), dict(p_ref=(1.0, np.inf, 1.0)),
           dict(compressibility=-0.1), dict(compressibility=(0.1, 0.1, np.nan)), dict(compressibility=np.inf),
           dict(kind=Cr, temperature=0.0), dict(kind=Cr, temperature=-1.0), dict(kind=Cr, temperature=None),
           dict(kind=Cr, temperature=np.nan), dict(kind=Cr, temperature=1.0, coupling="semiisotropic"),
           dict(kind=Cr, temperature=1.0, coupling="anisotropic")]
    for over in bad:
        kw = dict(kind=B, p_ref=1e3, compressibility=0.5, tau_p=0.1, every=1, coupling="isotropic", temperature=1.0)
        kw.update(over)
        with pytest.raises(E.EmDeeError) as err:
            md.set_barostat_(**kw)
        assert err.value.code == ERR_INVALID, over
    # NULL arrays, through the C ABI
    three = (C.c_double * 3)(1.0, 1.0, 1.0)
    for p, b in ((None, three), (three, None)):
        with pytest.raises(E.EmDeeError) as err:
            E._lib.call("emdee_md_set_barostat", md._handle, B, 0, p, b, 1.0, 1, 0.0, 0, 0)
        assert err.value.code == ERR_INVALID
    # the setting of before (compressibility 0, every 2) is the one in force: the run is the twin's, bit for bit
    md.step_(4, DT)
    twin.step_(4, DT)
    for a, b in zip(_xv(md), _xv(twin)):
        assert np.array_equal(a, b)
    assert md.box() == twin.box()
    # off: the other arguments are not looked at
    E._lib.call("emdee_md_set_barostat", md._handle, E.BAROSTAT_OFF, 99, None, None, np.nan, -1, -1.0, 0, 0)
    md.close()
    twin.close()


def test_lent_and_unloaded_engines_refuse_both_calls(emdee, dev):
    E = emdee
    S = bref.fluid864(E.synthetic)
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (a decomposition needs two bricks of 2.8 + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    eng = dd.engine(0)
    with pytest.raises(E.EmDeeError) as err:
        eng.scale_box_((1.01, 1.0, 1.0))
    assert err.value.code == ERR_STATE
    with pytest.raises(E.EmDeeError) as err:
        eng.set_barostat_(E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)
    assert err.value.code == ERR_STATE
    dd.step_(2, DT)                                                                      # the decomposition is unharmed
    dd.close()
    # before emdee_md_set_state, through the C ABI
    ctx = E.context_for(dev)
    h = C.c_void_p()
    three = lambda *v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", ctx.handle, three(0, 0, 0), three(S["L"], S["L"], S["L"]), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(E.LennardJonesModel(RC, RS)), SKIN, 8, C.byref(h))
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_scale_box", h, three(1.0, 1.0, 1.0), 1.0)
    assert err.value.code == ERR_STATE
    lo, ln = three(9, 9, 9), three(9, 9, 9)
    E._lib.call("emdee_md_get_box", h, lo, ln)
    assert list(lo) == [0.0] * 3 and list(ln) == [S["L"]] * 3
    E._lib.call("emdee_md_destroy", h)
    # an engine with ghosts
    g = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"][:-4], dev), S["L"], E.LennardJonesModel(RC, RS), E.cu(S["atoms"], dev),
                         skin=SKIN, n_ghost=4)
    with pytest.raises(E.EmDeeError) as err:
        g.scale_box_((1.01, 1.0, 1.0))
    assert err.value.code == ERR_STATE
    with pytest.raises(E.EmDeeError) as err:
        g.set_barostat_(E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)
    assert err.value.code == ERR_STATE
    g.close()


def test_a_scale_refused_at_an_event_comes_back_from_step_as_a_state_error(emdee, dev):
    """A huge compressibility asks the first event for mu far below what the box can take: the step call returns
    EMDEE_ERR_STATE, the state is the completed step's (the uncoupled twin's, to rounding) and the box is untouched."""
    E = emdee
    S, md = _fluid(E, dev)
    _, twin = _fluid(E, dev)
    md.set_barostat_(E.BAROSTAT_BERENDSEN, 100.0, 50.0, 1.0, 3)
    with pytest.raises(E.EmDeeError) as err:
        md.step_(10, DT)
    assert err.value.code == ERR_STATE and "coupling" in str(err.value)
    assert md.box()[1] == [S["L"]] * 3
    twin.step_(3, DT)
    for a, b in zip(_xv(md), _xv(twin)):
        assert np.abs(a - b).max() <= 1e-12
    md.set_barostat_(None)
    md.step_(2, DT)                                                                      # still able to step
    md.close()
    twin.close()


# ---------------------------------------------------------------- 4. trajectories under Berendsen coupling
COUPLINGS = {"isotropic": bref.ISOTROPIC, "semiisotropic": bref.SEMIISOTROPIC, "anisotropic": bref.ANISOTROPIC}


@pytest.mark.parametrize("coupling", list(COUPLINGS))
@pytest.mark.parametrize("path", PATHS)
def test_berendsen_trajectory_matches_the_numpy_integrator(emdee, dev, monkeypatch, path, coupling):
    E = emdee
    _path(monkeypatch, path)
    R = bref.berendsen_case(E.synthetic, COUPLINGS[coupling])
    mus = np.array([e[2] for e in R["events"]])
    assert len(R["events"]) == 8 and (np.abs(mus - 1.0) >= 1e-3).all() and (np.abs(mus - 1.0) <= 1e-2).all()
    assert (R["lengths"] < 0.99 * bref.fluid864(E.synthetic)["L"]).all() and (R["lengths"] // (RC + SKIN) == 3).all()
    if coupling == "semiisotropic":
        assert R["lengths"][0] == R["lengths"][1] != R["lengths"][2]
    if coupling == "anisotropic":
        assert len(set(R["lengths"])) == 3
    S, md = _fluid(E, dev)
    builds = md.nbr_stats()["builds"]
    md.set_barostat_(E.BAROSTAT_BERENDSEN, R["p_ref"], R["beta"], R["tau_p"], R["every"], coupling=coupling)
    md.step_(40, DT)
    ln = np.array(md.box()[1])
    x, v = _xv(md)
    gap_l, gap_x, gap_v = np.abs(ln / R["lengths"] - 1.0).max(), _image_gap(x, R["x"], ln), np.abs(v - R["v"]).max()
    print("%s %s: box %.2e, positions %.2e, velocities %.2e" % (path, coupling, gap_l, gap_x, gap_v))
    assert gap_l <= 1e-10
    assert gap_x < X64 and gap_v < X64
    assert md.nbr_stats()["builds"] >= builds + 8                                        # every event rebuilds
    assert md.observables()["density"] == pytest.approx(864 / np.prod(R["lengths"]), rel=1e-9)   # (the binding follows the box)
    md.close()


# ---------------------------------------------------------------- 5. batching
@pytest.mark.parametrize("rebuild_every", [0, 4])
@pytest.mark.parametrize("path", PATHS)
def test_the_states_do_not_depend_on_how_the_steps_are_dealt_to_calls(emdee, dev, monkeypatch, path, rebuild_every):
    E = emdee
    _path(monkeypatch, path)
    R = bref.berendsen_case(E.synthetic, bref.ISOTROPIC)
    out = []
    for calls, n in ((1, 40), (8, 5), (40, 1)):
        S, md = _fluid(E, dev)
        md.set_barostat_(E.BAROSTAT_BERENDSEN, R["p_ref"], R["beta"], R["tau_p"], R["every"])
        for _ in range(calls):
            md.step_(n, DT, rebuild_every)
        out.append(_xv(md) + (np.array(md.box()[1]),))
        md.close()
    assert (out[0][2] < 0.99 * S["L"]).all()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------- 6. stochastic cell rescaling
@pytest.mark.parametrize("path", PATHS)
def test_crescale_matches_the_numpy_integrator_and_is_reproducible(emdee, dev, monkeypatch, path):
    E = emdee
    _path(monkeypatch, path)
    R = bref.berendsen_case(E.synthetic, bref.ISOTROPIC)                                 # (its p_ref, compressibility and tau_p)
    seed, T = 12345, 1.0

    def run(sd):
        S, md = _fluid(E, dev)
        md.set_barostat_(E.BAROSTAT_CRESCALE, R["p_ref"][0], R["beta"][0], R["tau_p"], R["every"], temperature=T, seed=sd)
        md.step_(40, DT)
        return S, md

    S, md = run(seed)
    xi = lambda s: float(md.langevin_normals(seed, s, torch.tensor([-1]))[0, 0])
    x, v, ln, ev = bref.coupled_verlet(S["pos"], S["vel"], np.zeros(3), [S["L"]] * 3, bref.field(S["atoms"]), 40, DT, bref.CRESCALE,
                                       R["p_ref"][0], R["beta"][0], R["tau_p"], R["every"], temperature=T, xi=xi)
    noise = np.array([np.sqrt(2.0 * T * R["beta"][0] * R["every"] * DT / (np.prod(ln) * R["tau_p"])) * xi(e[0]) / 3.0 for e in ev])
    assert np.abs(noise).max() > 1e-4                                                    # the noise moves the box far beyond the bounds below
    got_l = np.array(md.box()[1])
    gx, gv = _xv(md)
    gap_l, gap_x, gap_v = np.abs(got_l / ln - 1.0).max(), _image_gap(gx, x, got_l), np.abs(gv - v).max()
    print("%s c-rescale: box %.2e, positions %.2e, velocities %.2e" % (path, gap_l, gap_x, gap_v))
    assert gap_l <= 1e-10 and gap_x < X64
    assert gap_v < X64                                                                   # (the 1 / mu factor: ~2e-3 of |v| ~ 3 per event)
    _, again = run(seed)
    assert again.box() == md.box()
    for a, b in zip(_xv(again), (gx, gv)):
        assert np.array_equal(a, b)
    _, other = run(seed + 1)
    assert other.box()[1] != md.box()[1]
    for m in (md, again, other):
        m.close()


# ---------------------------------------------------------------- 7. molecules
def _water_engine(E, dev, w, pos, vel, lengths, rc, rs, skin):
    md = _engine(E, dev, pos, vel, lengths, w["atoms"], rc=rc, rs=rs, skin=skin, inv_mass=w["inv_mass"])
    md.set_exclusions_(w["exclusions"])
    md.set_bonded_(br.BOND, w["bonds"], w["bond_params"])
    md.set_bonded_(br.ANGLE, w["angles"], w["angle_params"])
    md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
    return md


@pytest.mark.parametrize("path", PATHS)
def test_water_keeps_its_tables_through_a_scale_and_steps_under_coupling(emdee, dev, monkeypatch, path):
    E = emdee
    _path(monkeypatch, path)
    rc, rs, skin, n = 0.9, 0.8, 0.1, 7
    w = E.synthetic.water_box(n)
    L, N = w["L"], w["positions"].shape[0]
    assert L >= 2 * (rc + skin) > E.synthetic.water_box(n - 1)["L"] and 0.98 * L >= 2 * (rc + skin)
    pos = np.mod(w["positions"] + np.random.default_rng(7).uniform(-0.005, 0.005, (N, 3)), L)
    m = 1.0 / w["inv_mass"]
    vel = np.random.default_rng(11).standard_normal((N, 3)) * np.sqrt(2.0 / m)[:, None]
    vel -= (m[:, None] * vel).sum(axis=0) / m.sum()
    md = _water_engine(E, dev, w, pos, vel, L, rc, rs, skin)
    md.scale_box_((0.98, 1.01, 1.0))
    ln = md.box()[1]
    assert ln == [0.98 * L, 1.01 * L, 1.0 * L]
    x1, v1 = _xv(md)
    fresh = _water_engine(E, dev, w, x1, v1, ln, rc, rs, skin)
    _close_outputs(_outputs(md), _outputs(fresh), 1e-12, "scaled water against a fresh engine")
    fresh.close()
    md.set_barostat_(E.BAROSTAT_BERENDSEN, 0.06, 7.5e-4, 0.5, 2)                         # 1 bar, water's 4.5e-5 / bar, in kJ / mol / nm^3
    md.step_(10, 0.0004)
    assert md.box()[1] != ln and np.isfinite(md.totals()).all()
    md.close()


# ---------------------------------------------------------------- 8. off is off
@pytest.mark.parametrize("path", PATHS)
def test_zero_compressibility_leaves_the_box_and_the_trajectory(emdee, dev, monkeypatch, path):
    """mu = 1 at every event: the box is unchanged and the positions are those of an uncoupled run to rounding -- not bit for
    bit, since a coupled run closes the half kick of every step and rebuilds at every event."""
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    _, plain = _fluid(E, dev)
    builds = md.nbr_stats()["builds"]
    md.set_barostat_("berendsen", 5.0, 0.0, 1.0, 5, coupling="anisotropic")
    md.step_(40, DT)
    plain.step_(40, DT)
    assert md.box()[1] == [S["L"]] * 3 and md.nbr_stats()["builds"] >= builds + 8
    gap = _image_gap(_xv(md)[0], _xv(plain)[0], np.array([S["L"]] * 3))
    print("%s off: positions %.2e" % (path, gap))
    assert gap <= 1e-12
    md.close()
    plain.close()
