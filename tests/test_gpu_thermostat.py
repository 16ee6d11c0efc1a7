"""GPU tests of the global thermostats (include/emdee_hip.h: emdee_md_set_thermostat; csrc/thermostat.hpp) against the numpy
yardstick of tests/helpers/thermostat_ref.py, on the tiled and the direct kernels wherever the barostat tests use both.

The base box is barostat_ref.fluid864 (864 atoms, n_dof = 3 N - 3 = 2589, T* = 0.76 after its melt); the engines with tables are
the water, solute and four-site boxes of the settle, hbonds and vsites tests.  v-rescale's draws are redrawn through
thermostat_draws, as the barostat tests redraw through langevin_normals.  Tolerances are the project's: fp64 trajectories against
the numpy integrator 1e-8 in position and velocity over 40 steps (test_gpu_barostat.X64), the box 1e-10."""
import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import settle_ref as sr
from .helpers import shake_ref as hr
from .helpers import thermostat_ref as tr
from .helpers import vsite_ref as vr
from .test_gpu_barostat import DT, PATHS, X64, _fluid, _image_gap, _path, _xv
from .test_gpu_dd_pairs import _build
from .test_gpu_hbonds import _constraints_hold as _bonds_hold
from .test_gpu_hbonds import _engine as _solute_engine
from .test_gpu_settle import _constraints_hold, _refused
from .test_gpu_settle import _engine as _water_engine
from .test_gpu_vsites import _engine as _tip4p_engine
from .test_gpu_vsites import _sites_on_parents

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
N_DOF = 3 * 864 - 3
KT = 1.0
# v-rescale on the fluid: tau of half a step, so that every event redraws most of K (alpha - 1 of order sqrt(1 / n_dof) = 2e-2)
# and no event of the two reference runs below leaves |alpha - 1| under 1e-3; the seed was chosen on the CPU for that
TAU_V, SEED = 0.002, 40
# Nose-Hoover on the fluid: a period of a dozen steps
TAU_NH, CHAIN = 0.05, 3


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _state_gap(md, R, lengths):
    x, v = _xv(md)
    return _image_gap(x, R["x"], np.asarray(lengths, dtype=np.float64)), np.abs(v - R["v"]).max()


def _vrescale_reference(E, md, every, seed=None, baro=None):
    seed = SEED if seed is None else seed
    make = lambda: tr.Thermostat(tr.VRESCALE, KT, TAU_V, every, N_DOF, draws=lambda s: md.thermostat_draws(seed, s, N_DOF))
    return tr.fluid_case(E.synthetic, ("v-rescale", every, seed, baro is not None), make, baro=baro)


# ---------------------------------------------------------------- 1. v-rescale against numpy
@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("path", PATHS)
def test_vrescale_trajectory_matches_the_numpy_integrator(emdee, dev, monkeypatch, path, every):
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, KT, TAU_V, every=every, seed=SEED)
    R = _vrescale_reference(E, md, every)
    alphas = np.array([e[2] for e in R["thermo"].events])
    print("every %d: |alpha - 1| of the reference in [%.2e, %.2e]" % (every, np.abs(alphas - 1.0).min(), np.abs(alphas - 1.0).max()))
    assert len(alphas) == 40 // every and (np.abs(alphas - 1.0) >= 1e-3).all()
    md.step_(40, DT)
    gap_x, gap_v = _state_gap(md, R, [S["L"]] * 3)
    st = md.thermostat_state()
    e_ref = R["thermo"].energy
    print("%s every %d: positions %.2e, velocities %.2e, E_th %.9f against %.9f" % (path, every, gap_x, gap_v, st["energy"], e_ref))
    assert gap_x < X64 and gap_v < X64
    assert abs(st["energy"] - e_ref) <= 1e-9 * abs(e_ref)
    assert st["n_dof"] == N_DOF and abs(st["alpha"] - alphas[-1]) <= 1e-9 and st["xi"] == [0.0] * 8 and st["v_xi"] == [0.0] * 8
    md.close()


# ---------------------------------------------------------------- 2. Nose-Hoover against numpy
@pytest.mark.parametrize("path", PATHS)
def test_nose_hoover_trajectory_and_conserved_quantity_match_the_numpy_integrator(emdee, dev, monkeypatch, path):
    """U + K + E_th of the device run, read after every step (40 calls of one step are the sequence of one call of 40), stays
    within the spread the numpy run shows, plus the 1e-9 of its size by which fp64 box sums of the two may differ"""
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    md.set_thermostat_(E.THERMOSTAT_NOSE_HOOVER, KT, TAU_NH, chain=CHAIN)
    R = tr.fluid_case(E.synthetic, ("nose-hoover",), lambda: tr.Thermostat(tr.NOSE_HOOVER, KT, TAU_NH, 1, N_DOF, chain=CHAIN))
    alphas = np.array([e[2] for e in R["thermo"].events])
    assert np.abs(alphas - 1.0).max() >= 1e-3
    ep, ek, _ = md.totals()
    conserved = [ep + ek + md.thermostat_state()["energy"]]
    for _ in range(40):
        md.step_(1, DT)
        ep, ek, _ = md.totals()
        conserved.append(ep + ek + md.thermostat_state()["energy"])
    conserved = np.array(conserved)
    gap_x, gap_v = _state_gap(md, R, [S["L"]] * 3)
    spread, want = np.abs(conserved - conserved[0]).max(), np.abs(R["conserved"] - R["conserved"][0]).max()
    print("%s: positions %.2e, velocities %.2e; U + K + E_th = %.6f, spread %.3e (numpy %.3e); E_th %.6f"
          % (path, gap_x, gap_v, conserved[0], spread, want, md.thermostat_state()["energy"]))
    assert gap_x < X64 and gap_v < X64
    assert abs(conserved[0] - R["conserved"][0]) <= 1e-9 * abs(conserved[0])
    assert spread <= want + 1e-9 * abs(conserved[0])
    assert abs(md.thermostat_state()["energy"]) > 20.0 * want                # (E_th moved far more than the sum did)
    st, th = md.thermostat_state(), R["thermo"]
    assert np.abs(np.array(st["xi"][:CHAIN]) - th.xi).max() <= 1e-9 and np.abs(np.array(st["v_xi"][:CHAIN]) - th.vxi).max() <= 1e-9
    assert st["xi"][CHAIN:] == [0.0] * (8 - CHAIN) and st["v_xi"][CHAIN:] == [0.0] * (8 - CHAIN)
    md.close()


# ---------------------------------------------------------------- 3. dealing the steps to calls
def _switch_on(E, md, kind, seed):
    if kind == "nose-hoover":
        md.set_thermostat_(E.THERMOSTAT_NOSE_HOOVER, KT, TAU_NH, every=2, chain=CHAIN)
        return
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, KT, TAU_V, every=2 if kind == "v-rescale" else 1, seed=seed)
    if kind == "v-rescale+c-rescale":
        B = bref.berendsen_case(E.synthetic, bref.ISOTROPIC)
        md.set_barostat_(E.BAROSTAT_CRESCALE, B["p_ref"][0], B["beta"][0], B["tau_p"], B["every"], temperature=KT, seed=seed)


@pytest.mark.parametrize("kind", ["v-rescale", "nose-hoover", "v-rescale+c-rescale"])
@pytest.mark.parametrize("rebuild_every", [0, 4])
@pytest.mark.parametrize("path", PATHS)
def test_the_states_do_not_depend_on_how_the_steps_are_dealt_to_calls(emdee, dev, monkeypatch, path, rebuild_every, kind):
    E = emdee
    _path(monkeypatch, path)
    out = []
    for calls, n, seed in ((1, 40, 5), (8, 5, 5), (40, 1, 5), (1, 40, 5), (1, 40, 6)):
        S, md = _fluid(E, dev)
        _switch_on(E, md, kind, seed)
        for _ in range(calls):
            md.step_(n, DT, rebuild_every)
        st = md.thermostat_state()
        out.append(_xv(md) + (np.array(md.box()[1]), np.array([st["kinetic"], st["alpha"], st["energy"]] + st["xi"] + st["v_xi"])))
        md.close()
    for other in out[1:4]:                                                   # the three deals, and the same seed twice
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    if kind != "nose-hoover":                                                # another seed differs
        assert not np.array_equal(out[0][1], out[4][1]) and out[0][3][1] != out[4][3][1]


# ---------------------------------------------------------------- 4. restart
@pytest.mark.parametrize("kind", ["v-rescale", "nose-hoover"])
def test_a_restart_from_the_state_words_continues_bit_for_bit(emdee, dev, kind):
    E = emdee
    S, straight = _fluid(E, dev)
    _switch_on(E, straight, kind, 9)
    straight.step_(40, DT)
    _, md = _fluid(E, dev)
    _switch_on(E, md, kind, 9)
    md.step_(20, DT)
    words = md.thermostat_state()
    assert words["energy"] != 0.0 and words["alpha"] != 0.0
    if kind == "nose-hoover":
        md.set_thermostat_(E.THERMOSTAT_NOSE_HOOVER, KT, TAU_NH, every=2, chain=CHAIN, first_step=20)
    else:
        md.set_thermostat_(E.THERMOSTAT_VRESCALE, KT, TAU_V, every=2, seed=9, first_step=20)
    zeroed = md.thermostat_state()
    assert zeroed["energy"] == 0.0 and zeroed["alpha"] == 0.0 and zeroed["v_xi"] == [0.0] * 8
    md.set_thermostat_state_(words)
    back = md.thermostat_state()
    assert back["energy"] == words["energy"] and back["xi"] == words["xi"] and back["v_xi"] == words["v_xi"]
    md.step_(20, DT)
    for a, b in zip(_xv(md), _xv(straight)):
        assert np.array_equal(a, b)
    assert md.thermostat_state() == straight.thermostat_state()
    for m in (straight, md):
        m.close()


# ---------------------------------------------------------------- 5. twin engines, one step, every engine kind
def _pme_solute(E, dev, B, dtype=np.float64):
    md = _solute_engine(E, dev, B, dtype, hbonds=False)
    md.set_coulomb_(B["charges"], 1.0)
    md.set_hbonds_(B["clusters"], B["dist"])
    md.set_rigid3_(B["mol"], B["geom"])
    md.set_pme_(1.2, 16, 4)
    return md


def _twin_case(E, dev, kind):
    """(make engine, inv_mass or None, dt, the example's hand formula for n_dof, checks(md, what), dtype)"""
    if kind in ("lj", "fp32"):
        dtype = np.float32 if kind == "fp32" else np.float64
        return (lambda: _fluid(E, dev, dtype)[1]), None, DT, 3 * 864 - 3, (lambda md, what: None), dtype
    if kind == "rigid water":
        B = sr.water_box()
        return (lambda: _water_engine(E, dev, B)), 1.0 / B["mass"], sr.DT, 6 * len(B["mol"]) - 3, \
            (lambda md, what: _constraints_hold(md, B, np.float64, what)), np.float64
    if kind in ("hbonds solute", "charged pme"):
        B = hr.mixed_box()
        n = 3 * len(B["mass"]) - 3 * len(B["mol"]) - int((np.asarray(B["clusters"])[:, 1:] >= 0).sum()) - 3
        make = (lambda: _solute_engine(E, dev, B, rigid=True)) if kind == "hbonds solute" else (lambda: _pme_solute(E, dev, B))
        return make, 1.0 / B["mass"], hr.DT, n, (lambda md, what: _bonds_hold(md, B, B["pairs"], np.float64, what)), np.float64
    B = vr.four_site_box()

    def checks(md, what):
        _constraints_hold(md, B, np.float64, what)
        _sites_on_parents(md, B, np.float64, what)
    return (lambda: _tip4p_engine(E, dev, B)), B["inv_mass"], sr.DT, 6 * len(B["mol"]) - 3, checks, np.float64


@pytest.mark.parametrize("thermostat", ["v-rescale", "nose-hoover"])
@pytest.mark.parametrize("kind", ["lj", "rigid water", "hbonds solute", "tip4p sites", "charged pme", "fp32"])
def test_a_thermostatted_step_is_the_twins_step_with_scaled_velocities(emdee, dev, kind, thermostat):
    E = emdee
    make, inv_mass, dt, n_dof, checks, dtype = _twin_case(E, dev, kind)
    plain, md = make(), make()
    kT = 1.2 * 2.0 * tr.kinetic(_xv(plain)[1], inv_mass) / n_dof             # a target a fifth above where the state is
    # v-rescale: tau of half a step (alpha^2 about c + (1 - c) 1.2); Nose-Hoover: four steps, which its factorisation resolves
    tau, seed = (0.5 * dt if thermostat == "v-rescale" else 4.0 * dt), 31
    if thermostat == "v-rescale":
        md.set_thermostat_(E.THERMOSTAT_VRESCALE, kT, tau, seed=seed)
    else:
        md.set_thermostat_(E.THERMOSTAT_NOSE_HOOVER, kT, tau, chain=CHAIN)
    plain.step_(1, dt)
    md.step_(1, dt)
    st = md.thermostat_state()
    assert st["n_dof"] == n_dof                                              # the library's own count is the example's hand formula
    (xp, vp), (xt, vt) = _xv(plain), _xv(md)
    vp, vt = np.asarray(vp, dtype=np.float64), np.asarray(vt, dtype=np.float64)
    assert np.array_equal(xt, xp)
    K = tr.kinetic(vp, inv_mass)
    if thermostat == "v-rescale":
        R1, S = md.thermostat_draws(seed, 1, n_dof)
        want = float(np.sqrt(tr.alpha2(K, n_dof, np.exp(-dt / tau), 0.5 * n_dof * kT, R1, S)))
    else:
        want = tr.nhc_step(K, n_dof, kT, tau, dt, CHAIN, [0.0] * CHAIN, [0.0] * CHAIN)[0]
    alpha = st["alpha"]
    print("%s, %s: alpha %.12f (numpy %.12f), K %.9g (numpy %.9g)" % (kind, thermostat, alpha, want, st["kinetic"], K))
    assert abs(alpha - 1.0) >= 1e-3
    assert abs(st["kinetic"] - K) <= 1e-12 * K and abs(alpha - want) <= 1e-12 * want
    rounding = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    assert (np.abs(vt - alpha * vp) <= rounding * np.abs(alpha * vp)).all()
    checks(md, "%s, %s" % (kind, thermostat))
    md.step_(3, dt)                                                          # and it steps on, tables in place
    checks(md, "%s, %s, three steps on" % (kind, thermostat))
    plain.close()
    md.close()


# ---------------------------------------------------------------- 6. v-rescale with C-rescale against numpy
@pytest.mark.parametrize("path", PATHS)
def test_vrescale_with_crescale_matches_the_numpy_integrator(emdee, dev, monkeypatch, path):
    E = emdee
    _path(monkeypatch, path)
    B = bref.berendsen_case(E.synthetic, bref.ISOTROPIC)                                 # (its p_ref, compressibility and tau_p)
    seed = 12345
    S, md = _fluid(E, dev)
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, KT, TAU_V, seed=seed)
    md.set_barostat_(E.BAROSTAT_CRESCALE, B["p_ref"][0], B["beta"][0], B["tau_p"], B["every"], temperature=KT, seed=seed)
    baro = dict(p_ref=B["p_ref"][0], beta=B["beta"][0], tau_p=B["tau_p"], every=B["every"], temperature=KT,
                xi=lambda s: float(md.langevin_normals(seed, s, torch.tensor([-1]))[0, 0]))
    R = _vrescale_reference(E, md, 1, seed=seed, baro=baro)
    md.step_(40, DT)
    ln = np.array(md.box()[1])
    gap_l = np.abs(ln / R["lengths"] - 1.0).max()
    gap_x, gap_v = _state_gap(md, R, ln)
    print("%s v-rescale + c-rescale: box %.2e, positions %.2e, velocities %.2e" % (path, gap_l, gap_x, gap_v))
    assert np.abs(R["lengths"] / S["L"] - 1.0).max() > 1e-3
    assert gap_l <= 1e-10 and gap_x < X64 and gap_v < X64
    assert abs(md.thermostat_state()["energy"] - R["thermo"].energy) <= 1e-9 * abs(R["thermo"].energy)
    md.close()


# ---------------------------------------------------------------- 7. launch counts and the return to the fused loop
@pytest.mark.parametrize("path", PATHS)
def test_three_launches_per_event_and_off_is_the_fused_loop_again(emdee, dev, monkeypatch, path):
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    _, never = _fluid(E, dev)
    md.profile_(True)
    # switched on and off again before the first step: no trace in the 40 steps that follow, and they are fused steps
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, KT, TAU_V, every=5, seed=3)
    md.set_thermostat_(E.THERMOSTAT_OFF)
    md.step_(40, DT)
    never.step_(40, DT)
    for a, b in zip(_xv(md), _xv(never)):
        assert np.array_equal(a, b)
    assert md.kernel_time("thermostat") == (0.0, 0)
    fused = md.kernel_time("lj_force_nbr_fused_step")[1]
    assert (fused > 0) == (path == "tiled")
    md.set_thermostat_(E.THERMOSTAT_NOSE_HOOVER, KT, TAU_NH, every=5)
    md.step_(20, DT)
    ms, launches = md.kernel_time("thermostat")
    assert launches == 3 * 4 and ms > 0.0
    assert md.kernel_time("lj_force_nbr_fused_step")[1] == fused             # (closed steps: no fused launch)
    md.set_thermostat_(None)
    md.step_(10, DT)
    assert md.kernel_time("thermostat")[1] == 12
    if path == "tiled":
        assert md.kernel_time("lj_force_nbr_fused_step")[1] > fused
    md.close()
    never.close()


# ---------------------------------------------------------------- 8. refusals
def test_invalid_settings_are_refused_and_the_previous_one_stays(emdee, dev):
    E = emdee
    V, NH = E.THERMOSTAT_VRESCALE, E.THERMOSTAT_NOSE_HOOVER
    S, md = _fluid(E, dev)
    _, twin = _fluid(E, dev)
    good = dict(kind=V, temperature=KT, tau_t=TAU_V, every=2, seed=4)
    md.set_thermostat_(**good)
    twin.set_thermostat_(**good)
    bad = [dict(kind=3), dict(kind=-1), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=np.nan), dict(temperature=np.inf),
           dict(tau_t=0.0), dict(tau_t=-0.1), dict(tau_t=np.nan), dict(tau_t=np.inf), dict(every=0), dict(every=-2), dict(n_dof=-1),
           dict(kind=NH, chain=0), dict(kind=NH, chain=9), dict(kind=NH, chain=-3)]
    for over in bad:
        kw = dict(kind=V, temperature=2.0, tau_t=0.5, every=1, n_dof=0, chain=3, seed=1)
        kw.update(over)
        text = _refused(E, ERR_INVALID, md.set_thermostat_, **kw)
        assert "set_thermostat" in text, (over, text)
    md.set_thermostat_(V, 2.0, 0.5, chain=99)                                # (the chain length is not looked at for v-rescale) ...
    md.set_thermostat_(**good)                                               # ... and the good setting again, from its first step
    # NULL arrays, through the C ABI
    for name in ("emdee_md_thermostat_state", "emdee_md_set_thermostat_state"):
        with pytest.raises(E.EmDeeError) as err:
            E._lib.call(name, md._handle, None)
        assert err.value.code == ERR_INVALID and "thermostat_state" in str(err.value)
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_thermostat_draws", md._handle, 1, 1, 10, None)
    assert err.value.code == ERR_INVALID and "thermostat_draws" in str(err.value)
    # Langevin and a global thermostat exclude each other, whichever comes second
    assert "set_langevin" in _refused(E, ERR_STATE, md.set_langevin_, 1.0, 1.0)
    md.set_langevin_(0.0, 1.0)                                               # (gamma = 0 is no thermostat)
    _, lgv = _fluid(E, dev)
    lgv.set_langevin_(1.0, 1.0, seed=2)
    assert "set_thermostat" in _refused(E, ERR_STATE, lgv.set_thermostat_, V, KT, TAU_V)
    lgv.set_thermostat_(E.THERMOSTAT_OFF)
    lgv.step_(2, DT)
    lgv.close()
    # the setting of before is the one in force: the run is the twin's, bit for bit
    md.step_(6, DT)
    twin.step_(6, DT)
    for a, b in zip(_xv(md), _xv(twin)):
        assert np.array_equal(a, b)
    assert md.thermostat_state() == twin.thermostat_state() and md.thermostat_state()["alpha"] != 0.0
    # minimisation leaves the thermostat out and its words alone
    words = md.thermostat_state()
    md.minimize_(5, 1e-3)
    assert md.thermostat_state() == words
    md.step_(2, DT)
    # off: the other arguments are not looked at
    E._lib.call("emdee_md_set_thermostat", md._handle, E.THERMOSTAT_OFF, np.nan, -1.0, 0, -5, 99, 0, 0)
    md.close()
    twin.close()


def test_too_few_degrees_of_freedom_are_refused_at_step_time(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, KT, TAU_V, n_dof=2)            # (taken as given ...)
    text = _refused(E, ERR_STATE, md.step_, 1, DT)                           # ... and too few at step time
    assert "set_thermostat" in text and "degrees" in text
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, KT, TAU_V, n_dof=2000)
    md.step_(2, DT)
    assert md.thermostat_state()["n_dof"] == 2000
    md.close()


def test_lent_engines_and_engines_with_ghosts_refuse_the_setters(emdee, dev):
    E = emdee
    S = bref.fluid864(E.synthetic)
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (a decomposition needs two bricks of 2.8 + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    eng = dd.engine(0)
    assert "set_thermostat" in _refused(E, ERR_STATE, eng.set_thermostat_, E.THERMOSTAT_VRESCALE, KT, TAU_V)
    state = dict(energy=0.0, xi=[0.0] * 8, v_xi=[0.0] * 8)
    assert "set_thermostat_state" in _refused(E, ERR_STATE, eng.set_thermostat_state_, state)
    dd.step_(2, DT)                                                                      # the decomposition is unharmed
    dd.close()
    g = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"][:-4], dev), S["L"], E.LennardJonesModel(bref.RC, bref.RS), E.cu(S["atoms"], dev),
                         skin=bref.SKIN, n_ghost=4)
    assert "set_thermostat" in _refused(E, ERR_STATE, g.set_thermostat_, E.THERMOSTAT_NOSE_HOOVER, KT, TAU_NH)
    assert "set_thermostat_state" in _refused(E, ERR_STATE, g.set_thermostat_state_, state)
    g.close()
