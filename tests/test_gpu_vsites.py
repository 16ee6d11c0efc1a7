"""GPU tests of virtual interaction sites (include/emdee_hip.h: emdee_md_set_vsites; csrc/vsite.hpp) against the numpy yardstick of
tests/helpers/vsite_ref.py: four-site rigid water.

The box is settle_ref.water_box() -- 150 molecules of masses (16, 1, 1) in a box of sides (7.0, 7.5, 8.2) at lo = (-1.0, 0.5, 2.0),
every atom wrapped on its own -- with a fourth, massless site per molecule (ids 450 .. 599) on the bisector at w_b = w_c = 0.13,
epsilon = 0, carrying the apex charge; exclusions over all six pairs of a molecule; 600 atoms.  Unless a test says otherwise the
engine is charged (reaction field, coulomb_k = 1): without charges a site with epsilon = 0 feels nothing.

The reference (vsite_ref.constrained_verlet) places the sites, takes the forces on all 600 atoms from an engine WITHOUT a site
table loaded with those positions, and spreads them on the host.

Bounds.  Placement: 8 eps(real) of the largest box side (fp64 arithmetic on a handful of terms of that size, rounded once into
the record and once on the way out).  Spread forces: 8 eps(real) of the largest force in the molecule (one short sum).
Trajectories: the 1e-11 L_max and 1e-11 v_rms of tests/test_gpu_settle.py.  Energy drift: twice the reference's, as there."""
import numpy as np
import pytest

from .helpers import settle_ref as sr
from .helpers import vsite_ref as vr
from .test_gpu_dd_pairs import _build
from .test_gpu_settle import DT, EPS32, ERR_INVALID, ERR_STATE, _constraints_hold, _forces, _refused, _xv
from .test_molecular_ref_host import FD_BOUND, H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS64 = float(np.finfo(np.float64).eps)
EPS = {np.float64: EPS64, np.float32: EPS32}
L_MAX = float(sr.LENGTHS.max())
X_TOL, V_TOL = 1e-11, 1e-11                             # tests/test_gpu_settle.py: _against_reference
# the Berendsen setting of tests/test_gpu_molecular.py (isotropic entries)
P_REF, BETA, TAU_P, EVERY = 19.0, 0.02, 1.0, 5
MU = np.array([1.013, 0.991, 1.004])
# max |E(t) - E(0)| of the numpy reference (vsite_ref.constrained_verlet with the all-pairs Lennard-Jones and reaction-field
# forces of tests/helpers/ortho_ref.py) from the same start over 400 steps, sampled every 20; E(0) = -220.190396.  Measured on
# the CPU, 2026-10-20:
#   python -m tests.helpers.vsite_ref
REFERENCE_DRIFT = 1.223856e-03


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _engine(E, dev, B, dtype=np.float64, sites=True, rigid=True, charged=True, excl=True, masses=True, pos=None, vel=None, lengths=None, atoms=None):
    pos, vel = B["pos"] if pos is None else pos, B["vel"] if vel is None else vel
    lengths = [float(t) for t in (sr.LENGTHS if lengths is None else lengths)]
    md = E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), lengths[0],
                          E.LennardJonesModel(sr.RC, sr.RS), E.cu(B["atoms"] if atoms is None else atoms, dev), skin=sr.SKIN,
                          inv_mass=E.cu(B["inv_mass"].astype(dtype), dev) if masses else None, lo=list(sr.LO), lengths=lengths, periodic=[1, 1, 1])
    if excl:
        md.set_exclusions_(B["excl"])
    if charged:
        md.set_coulomb_(B["charges"], 1.0)
    if rigid:
        md.set_rigid3_(B["mol"], B["geom"])
    if sites:
        md.set_vsites_(B["vs_atoms"], B["vs_weights"])
    return md


def _load(E, dev, md, B, pos, vel, dtype=np.float64, n=None):
    n = len(pos) if n is None else n
    md.set_state_(E.cu(np.asarray(pos[:n]).astype(dtype), dev), E.cu(np.asarray(vel[:n]).astype(dtype), dev), E.cu(B["atoms"][:n], dev),
                  E.cu(B["inv_mass"][:n].astype(dtype), dev))


def _gap(x, want, lengths=sr.LENGTHS):
    d = np.asarray(x, dtype=np.float64) - want
    return np.abs(d - lengths * np.rint(d / lengths)).max()


def _sites_on_parents(md, B, dtype, what, lengths=sr.LENGTHS, atoms=None, weights=None):
    """the engine's sites against numpy's placement from the engine's own parents, modulo the box"""
    atoms, weights = B["vs_atoms"] if atoms is None else atoms, B["vs_weights"] if weights is None else weights
    x, v = _xv(md)
    gap = _gap(x[atoms[:, 0]], vr.place(x, atoms, weights, lengths), lengths)
    bound = 8.0 * EPS[dtype] * float(np.max(lengths))
    print("%s: sites against their parents %.3e (bound %.3e)" % (what, gap, bound))
    assert gap <= bound, (what, gap)
    assert (v[atoms[:, 0]] == 0.0).all()
    return x


def _twin_forces(E, dev, twin, B, x, dtype=np.float64):
    """the forces on all atoms, sites included, of an engine without a site table loaded with x"""
    _load(E, dev, twin, B, x, np.zeros_like(x), dtype)
    return _forces(twin)


def _spread_bound(B, raw, dtype):
    """(N, 1): 8 eps(real) max |f| over the four atoms of each atom's molecule"""
    four = np.concatenate([B["mol"], B["sites"][:, None]], axis=1)
    big = np.abs(raw[four]).max(axis=(1, 2))
    out = np.zeros(raw.shape[0])
    for k in range(4):
        out[four[:, k]] = big
    return 8.0 * EPS[dtype] * out[:, None]


def _check_spread_forces(E, dev, md, twin, B, dtype, what):
    x = md.state(velocities=False, forces=False)["positions"].cpu().numpy()
    f = _forces(md)
    raw = _twin_forces(E, dev, twin, B, x, dtype)
    want = vr.spread(raw, B["vs_atoms"], B["vs_weights"])
    assert (f[B["sites"]] == 0.0).all()
    err = np.abs(f - want)
    bound = _spread_bound(B, raw, dtype)
    assert (np.abs(want - raw)[B["real"]] > 100.0 * bound[B["real"]]).any()  # (the sites carried forces: leaving the spreading out would show)
    print("%s: largest |f - spread(f_twin)| / (8 eps max |f| of the molecule) = %.3f" % (what, (err / bound).max()))
    assert (err <= bound).all(), what
    return raw


# ---------------------------------------------------------------- 1. placement
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_placement_at_the_set_call_and_after_set_state(emdee, dev, dtype):
    E = emdee
    B = vr.four_site_box()
    rng = np.random.default_rng(29)
    n = len(B["pos"])

    def scattered():
        """every atom in an image of its own, up to +-3 box lengths; the sites 0.3 off where they belong, with velocities"""
        pos = B["unwrapped"] + rng.integers(-3, 4, (n, 3)) * sr.LENGTHS
        pos = pos.astype(dtype).astype(np.float64)
        pos[B["sites"]] = (vr.place(pos, B["vs_atoms"], B["vs_weights"], sr.LENGTHS) + rng.uniform(-0.3, 0.3, (150, 3))).astype(dtype)
        vel = B["vel"].copy()
        vel[B["sites"]] = rng.normal(size=(150, 3))
        return pos, vel
    pos, vel = scattered()
    md = _engine(E, dev, B, dtype, pos=pos, vel=vel)
    for what in ("set call", "set_state"):
        x = _sites_on_parents(md, B, dtype, "%s, %s" % (np.dtype(dtype).name, what))
        real = B["real"]
        # (no parent moved: the positions come back in the caller's image, wrapped and unwrapped with a rounding each)
        assert np.abs(x[real] - pos[real]).max() <= 4.0 * EPS[dtype] * np.abs(pos).max()
        assert np.abs(x[B["sites"]] - vr.place(pos, B["vs_atoms"], B["vs_weights"], sr.LENGTHS)).max() < 0.5    # (the image nearest to where it was loaded)
        pos, vel = scattered()
        _load(E, dev, md, B, pos, vel, dtype)
    md.step_(2, DT)
    md.close()


# ---------------------------------------------------------------- 2. forces after the set call
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_forces_and_sums_after_the_set_call(emdee, dev, dtype):
    E = emdee
    B = vr.four_site_box()
    md = _engine(E, dev, B, dtype)
    twin = _engine(E, dev, B, dtype, sites=False, rigid=False)
    _check_spread_forces(E, dev, md, twin, B, dtype, "%s, after the set call" % np.dtype(dtype).name)
    ep, ek, w = md.totals()
    assert np.isfinite([ep, ek, w]).all()
    tp, _, tw = twin.totals()
    assert (ep, w) == (tp, tw)                                               # (the box sums are the force field's, untouched: bit for bit)
    _, v = _xv(md)
    want = vr.kinetic(B, v)
    assert abs(ek - want) <= 1e-12 * want                                    # (the sites count as exactly 0, no 0 / 0)
    # a second query, and a pass that writes the force planes again, spread once each
    md.forces_(E.FORCES)
    f0 = _forces(md)
    md.forces_(E.FORCES)
    assert np.array_equal(_forces(md), f0)
    assert np.isfinite(md.tensor_sums()).all() and np.array_equal(_forces(md), f0)      # (the tensor pass leaves the planes alone)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 3. trajectories
def test_one_step_and_twenty_steps_match_the_reference(emdee, dev):
    E = emdee
    B = vr.four_site_box()
    md = _engine(E, dev, B)
    twin = _engine(E, dev, B, sites=False, rigid=False)
    offset = B["pos"] - B["unwrapped"]
    seen = {}

    def observe(s, x, v):
        md.step_(1, DT, 3)
        if s in (1, 20):
            gx, gv = _xv(md)
            seen[s] = (np.abs(gx - (x + offset)).max(), np.abs(gv - v).max(), np.sqrt((v[B["real"]] ** 2).sum(axis=1).mean()))
    vr.constrained_verlet(B["unwrapped"], B["vel"], lambda x, k: _twin_forces(E, dev, twin, B, x), 20, DT, B, observe=observe)
    for s in (1, 20):
        ex, ev, vrms = seen[s]
        print("step %d: max |dx| = %.3e (box side %.1f), max |dv| = %.3e (rms velocity %.3f)" % (s, ex, L_MAX, ev, vrms))
        assert ex <= X_TOL * L_MAX and ev <= V_TOL * vrms, (s, ex, ev)
    assert md.nbr_stats()["builds"] >= 1 + 20 // 3
    _sites_on_parents(md, B, np.float64, "after 20 steps")
    md.close()
    twin.close()


@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_geometry_and_sites_hold_over_300_steps_with_automatic_rebuilds(emdee, dev, dtype, langevin):
    B = vr.four_site_box()
    md = _engine(emdee, dev, B, dtype)
    if langevin:
        md.set_langevin_(1.0, 1.0, seed=7)
    before = md.nbr_stats()["builds"]
    md.step_(300, DT)
    assert md.nbr_stats()["builds"] > before
    what = "%s, %s" % (np.dtype(dtype).name, "Langevin" if langevin else "NVE")
    _constraints_hold(md, B, dtype, what, records=dtype == np.float32)
    _sites_on_parents(md, B, dtype, what)
    md.close()


# ---------------------------------------------------------------- 4. energy conservation
def test_energy_is_conserved_as_well_as_by_the_reference(emdee, dev):
    B = vr.four_site_box()
    md = _engine(emdee, dev, B)
    ep, ek, _ = md.totals()
    e0, worst = ep + ek, 0.0
    for _ in range(20):
        md.step_(20, DT)
        ep, ek, _ = md.totals()
        worst = max(worst, abs(ep + ek - e0))
    print("engine: E(0) = %.6f, max |E(t) - E(0)| over 400 steps = %.6e; reference %.6e" % (e0, worst, REFERENCE_DRIFT))
    assert abs(e0 - (-220.190396)) <= 1e-5                                   # (the same start as the reference's)
    assert worst <= 2.0 * REFERENCE_DRIFT                                    # (the factor: another summation order over 400 chaotic steps)
    md.close()


# ---------------------------------------------------------------- 5. dealing and reproducibility
@pytest.mark.parametrize("rebuild_every", [0, 7])
def test_dealing_of_steps_to_calls_and_reruns_are_bit_identical(emdee, dev, rebuild_every):
    B = vr.four_site_box()
    out = []
    for deal in ((40,), (5,) * 8, (1,) * 40, (40,)):
        md = _engine(emdee, dev, B)
        md.profile_(True)
        for n in deal:
            md.step_(n, DT, rebuild_every)
        out.append(_xv(md) + (_forces(md),))
        ms, launches = md.kernel_time("vsites")
        assert launches == 2 * 40 and ms > 0.0                               # (place and spread of every step; emdee_md_kernel_time index 13)
        assert md.kernel_time(13) == (ms, launches)
        md.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------- 6. minimisation
def test_minimize_converges_with_sites_on_their_parents(emdee, dev):
    """Whole molecules displaced by a random vector of 10 % of the lattice spacing (7.0 / 5).  Converged means here: the largest
    constrained force has fallen to a tenth of what it was at the start (f_tol is set from the start's own g_max)."""
    E = emdee
    B = vr.four_site_box()
    rng = np.random.default_rng(31)
    shift = rng.normal(size=(150, 3))
    shift *= 0.1 * (7.0 / 5.0) / np.linalg.norm(shift, axis=1, keepdims=True)
    pos = B["unwrapped"].copy()
    for col in range(3):
        pos[B["mol"][:, col]] += shift
    pos[B["sites"]] += shift
    runs = []
    for _ in range(2):
        md = _engine(E, dev, B, pos=pos, vel=np.zeros_like(pos))
        start = md.minimize_(0, 0.0)
        assert np.isfinite(start.g_max) and start.g_max > 0.0
        res = md.minimize_(500, 0.1 * start.g_max, dt_start=0.001, dt_max=0.01, max_step=0.05)
        print(start, res)
        assert res.converged and np.isfinite(res.g_max) and res.g_max <= 0.1 * start.g_max
        assert np.isfinite(res.energy) and res.energy < res.energy0
        _constraints_hold(md, B, np.float64, "minimised")
        _sites_on_parents(md, B, np.float64, "minimised")
        assert (_forces(md)[B["sites"]] == 0.0).all()
        runs.append(_xv(md) + (_forces(md), res.energy, res.g_max, res.iterations))
        md.step_(5, DT)
        md.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 7. charged engines
def test_charged_engine_reaction_field_then_ewald_then_pme(emdee, dev):
    E = emdee
    B = vr.four_site_box()
    md = _engine(E, dev, B)
    twin = _engine(E, dev, B, sites=False, rigid=False)
    # (no step in between: the positions stay the in-box ones both engines were loaded with, so the twin sees the same numbers)
    _check_spread_forces(E, dev, md, twin, B, np.float64, "reaction field")
    for what, switch in (("Ewald", lambda e: e.set_ewald_(1.2, 6)), ("PME", lambda e: e.set_pme_(1.2, 16, 4))):
        switch(md)
        switch(twin)
        _check_spread_forces(E, dev, md, twin, B, np.float64, what)
        _sites_on_parents(md, B, np.float64, what)
    md.step_(5, DT)                                                          # (the engine steps on under the mesh)
    _sites_on_parents(md, B, np.float64, "PME, five steps on")
    _constraints_hold(md, B, np.float64, "reaction field, Ewald, PME")
    md.close()
    twin.close()


# ---------------------------------------------------------------- 8. pressure
def test_atomic_scale_keeps_two_parent_sites_of_free_atoms_on_their_parents(emdee, dev):
    B = vr.four_site_box()
    atoms = np.concatenate([B["vs_atoms"][:, :3], np.full((150, 1), -1)], axis=1)       # {site, apex, a}: on the apex-leg line
    weights = np.tile([0.3, np.nan], (150, 1))
    md = _engine(emdee, dev, B, rigid=False, sites=False)
    md.set_vsites_(atoms, weights)
    assert np.isfinite(md.tensor_sums()).all()
    _sites_on_parents(md, B, np.float64, "two-parent sites", atoms=atoms, weights=weights)
    x0, _ = _xv(md)
    md.scale_box_(MU)
    ln = np.array(md.box()[1])
    assert np.array_equal(ln, MU * sr.LENGTHS)
    x1 = _sites_on_parents(md, B, np.float64, "two-parent sites, scaled atom by atom", lengths=ln, atoms=atoms, weights=weights)
    real = B["real"]
    assert _gap(x1[real], sr.LO + MU * (x0[real] - sr.LO), ln) <= X_TOL * L_MAX
    assert (_forces(md)[atoms[:, 0]] == 0.0).all()
    md.step_(3, DT)
    _sites_on_parents(md, B, np.float64, "two-parent sites, three steps on", lengths=ln, atoms=atoms, weights=weights)
    md.close()


def test_trace_of_the_molecular_virial_is_the_volume_derivative_with_sites(emdee, dev):
    B = vr.four_site_box()
    md = _engine(emdee, dev, B)
    md.set_molecular_scaling_()
    assert np.isfinite(md.tensor_sums()).all()
    trace = sum(md.molecular_tensor_sums()[:3])
    md.scale_box_(1.0 + H)
    up = md.totals()[0]
    md.scale_box_((1.0 - H) / (1.0 + H))                                     # (molecular scales compose: this is mu = 1 - h of the start)
    ln = np.array(md.box()[1])
    assert np.abs(ln / sr.LENGTHS - (1.0 - H)).max() <= 1e-15
    down = md.totals()[0]
    fd = -(up - down) / (2.0 * H)
    gap = abs(fd - trace) / abs(trace)
    print("tr W_mol = %.4f, -dU/dmu through scale_box_ and totals() = %.4f: relative difference %.3e (bound %.2e)" % (trace, fd, gap, FD_BOUND))
    assert gap <= FD_BOUND
    x, _ = _xv(md)
    assert sr.residual(sr.unwrap(x, B["mol"], ln), B["mol"], B["geom"]) <= 1e-12       # (tests/test_gpu_molecular.py: the scale primitive)
    _sites_on_parents(md, B, np.float64, "scaled by molecular centres", lengths=ln)
    md.close()


def test_molecular_scale_moves_a_site_rigidly_with_its_water(emdee, dev):
    B = vr.four_site_box()
    md = _engine(emdee, dev, B)
    md.set_molecular_scaling_()
    x0, _ = _xv(md)
    md.scale_box_(MU)
    ln = np.array(md.box()[1])
    x1 = _sites_on_parents(md, B, np.float64, "molecular scale", lengths=ln)
    # site - apex is the same vector before and after (modulo the boxes)
    d0 = x0[B["sites"]] - x0[B["mol"][:, 0]]
    d1 = x1[B["sites"]] - x1[B["mol"][:, 0]]
    d0, d1 = d0 - sr.LENGTHS * np.rint(d0 / sr.LENGTHS), d1 - ln * np.rint(d1 / ln)
    assert np.abs(d1 - d0).max() <= X_TOL * L_MAX
    assert sr.residual(sr.unwrap(x1, B["mol"], ln), B["mol"], B["geom"]) <= 1e-12
    md.close()


def test_a_berendsen_run_does_not_depend_on_the_dealing(emdee, dev):
    E = emdee
    B = vr.four_site_box()
    out = []
    for deal in ((40,), (5,) * 8, (1,) * 40):
        md = _engine(E, dev, B)
        md.set_molecular_scaling_()
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY)
        for n in deal:
            md.step_(n, DT)
        out.append(_xv(md) + (np.array(md.box()[1]),))
        _sites_on_parents(md, B, np.float64, "Berendsen, dealt %s" % (deal[:1],), lengths=out[-1][2])
        md.close()
    assert not np.array_equal(out[0][2], sr.LENGTHS)                         # (the box did change)
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------- 9. refusals and state rules
def test_invalid_tables_are_refused_and_the_previous_table_still_steps(emdee, dev):
    E = emdee
    B = vr.four_site_box()
    md = _engine(E, dev, B)
    atoms, weights = B["vs_atoms"], B["vs_weights"]

    def changed(arr, s, k, value):
        out = arr.astype(np.float64 if arr is weights else np.int64).copy()
        out[s, k] = value
        return out
    one = torch.zeros(4, dtype=torch.int32, device=dev)
    cases = {
        "NULL atoms": lambda: E._lib.call("emdee_md_set_vsites", md._handle, None, None, 1),
        "NULL weights": lambda: E._lib.call("emdee_md_set_vsites", md._handle, one.data_ptr(), None, 1),
        "negative count": lambda: E._lib.call("emdee_md_set_vsites", md._handle, one.data_ptr(), one.data_ptr(), -1),
        "id too high": lambda: md.set_vsites_(changed(atoms, 3, 2, 600), weights),
        "negative site": lambda: md.set_vsites_(changed(atoms, 3, 0, -1), weights),
        "negative a": lambda: md.set_vsites_(changed(atoms, 3, 1, -1), weights),
        "negative b": lambda: md.set_vsites_(changed(atoms, 3, 2, -1), weights),
        "c below -1": lambda: md.set_vsites_(changed(atoms, 3, 3, -2), weights),
        "twice within": lambda: md.set_vsites_(changed(atoms, 4, 3, atoms[4, 1]), weights),
        "a site in two entries": lambda: md.set_vsites_(changed(atoms, 4, 0, atoms[9, 0]), weights),
        "a site that is a parent": lambda: md.set_vsites_(changed(atoms, 4, 3, atoms[9, 0]), weights),
        "a site of the rigid table": lambda: md.set_vsites_(changed(atoms, 4, 0, B["mol"][77, 1])[[4]], weights[[4]]),
        "nan weight": lambda: md.set_vsites_(atoms, changed(weights, 2, 0, np.nan)),
        "infinite weight": lambda: md.set_vsites_(atoms, changed(weights, 2, 1, np.inf)),
        # the mirror refusals: a constraint table that names a site
        "rigid molecule with a site": lambda: md.set_rigid3_(np.concatenate([B["mol"][:149], [[447, 448, 599]]]), B["geom"]),
        "hbonds cluster with a site": lambda: md.set_hbonds_([[599, 1, -1, -1]], [[0.3, 0.0, 0.0]]),
    }
    for name, call in cases.items():
        _refused(E, ERR_INVALID, call)
        md.step_(1, DT)
    _constraints_hold(md, B, np.float64, "after %d refusals" % len(cases))
    _sites_on_parents(md, B, np.float64, "after %d refusals" % len(cases))   # (the table set at the start is the one in force)
    md.close()


def test_the_device_check_names_the_site(emdee, dev):
    E = emdee
    B = vr.four_site_box()
    md = _engine(E, dev, B, rigid=False, sites=False)
    good = B["vs_atoms"][:5]
    md.set_vsites_(good, B["vs_weights"][:5])
    massive = good.copy()
    massive[3, 0] = B["mol"][100, 1]                                         # (a hydrogen as the site)
    text = _refused(E, ERR_STATE, md.set_vsites_, massive, B["vs_weights"][:5])
    assert "site 3 " in text and "has a mass" in text
    md.step_(1, DT)
    orphan = good.copy()
    orphan[2, 2] = B["sites"][140]                                           # (a massless atom, not a site of this table, as a parent)
    text = _refused(E, ERR_STATE, md.set_vsites_, orphan, B["vs_weights"][:5])
    assert "site 2 " in text and "massless" in text
    md.step_(1, DT)
    _sites_on_parents(md, B, np.float64, "after two device refusals", atoms=good, weights=B["vs_weights"][:5])
    md.close()
    bare = _engine(E, dev, B, rigid=False, sites=False, charged=False, masses=False)
    text = _refused(E, ERR_STATE, bare.set_vsites_, B["vs_atoms"], B["vs_weights"])
    assert "site 0 " in text and "without masses" in text
    bare.step_(1, DT)
    bare.close()


def test_an_engine_lent_by_a_decomposition_refuses_the_call(emdee, dev):
    E = emdee
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (two bricks of rc + skin + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    text = _refused(E, ERR_STATE, dd.engine(0).set_vsites_, [[0, 1, 2, -1]], [[0.5, 0.0]])
    assert "emdee_dd_engine" in text
    dd.step_(2, 0.005)                                                                   # the decomposition is unharmed
    dd.close()


def test_set_state_with_another_count_refuses_until_the_table_is_set_again_or_cleared(emdee, dev):
    # without exclusions and charges (they would refuse the smaller state themselves) and without LJ forces: the rules of the table alone
    E = emdee
    B = vr.four_site_box()
    ghostly = B["atoms"].copy()
    ghostly["twice_sqrt_eps"] = 0.0
    B["atoms"] = ghostly
    md = _engine(E, dev, B, excl=False, charged=False, rigid=False)
    md.profile_(True)
    md.step_(2, DT)
    assert md.kernel_time("vsites")[1] == 2 * 2
    _load(E, dev, md, B, B["pos"], B["vel"], n=599)                          # another count
    _refused(E, ERR_STATE, md.step_, 1, DT)
    text = _refused(E, ERR_STATE, md.minimize_, 1, 0.0)
    assert "emdee_md_set_vsites" in text
    _refused(E, ERR_STATE, md.scale_box_, 1.001)
    md.set_vsites_(B["vs_atoms"][:149], B["vs_weights"][:149])               # set again for this count
    md.step_(2, DT)
    _load(E, dev, md, B, B["pos"], B["vel"])                                 # 600 again: the table is for 599
    _refused(E, ERR_STATE, md.step_, 1, DT)
    md.set_vsites_(None, None)                                               # cleared: steps again, and books nothing
    md.profile_(True)
    md.step_(2, DT)
    assert md.kernel_time("vsites") == (0.0, 0)
    # a state of the same count that does not fit (a site loaded with a mass): set_state says so, the engine refuses to step
    md.set_vsites_(B["vs_atoms"], B["vs_weights"])
    heavy = B["inv_mass"].copy()
    heavy[B["sites"][12]] = 1.0
    text = _refused(E, ERR_STATE, md.set_state_, E.cu(B["pos"], dev), E.cu(B["vel"], dev), E.cu(ghostly, dev), E.cu(heavy, dev))
    assert "site 12 " in text
    _refused(E, ERR_STATE, md.step_, 1, DT)
    _load(E, dev, md, B, B["pos"], B["vel"])
    md.step_(1, DT)
    md.close()


def test_an_engine_without_a_table_books_no_site_launches_and_steps_as_before(emdee, dev):
    B = vr.four_site_box()
    out = []
    for cleared in (False, True):
        md = _engine(emdee, dev, B, sites=cleared)
        if cleared:
            md.set_vsites_(None, None)
            _load(emdee, dev, md, B, B["pos"], B["vel"])                      # (the state the twin has: the set call had zeroed nothing here, but placed)
        md.profile_(True)
        md.step_(10, DT)
        assert md.kernel_time("vsites") == (0.0, 0)
        out.append(_xv(md))
        md.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
