"""GPU tests of energy minimisation (include/emdee_hip.h: emdee_md_minimize; csrc/minimize.hpp) against the numpy
yardstick of tests/helpers/fire_ref.py: FIRE around the closed step, forces from ortho_ref (all pairs), constraints from
shake_ref's Gauss-Seidel SHAKE and RATTLE, G from rattle on w F.

Every box has a few hundred atoms (the two-table box of shake_ref 1180), orthorhombic with unequal sides at lo != 0.  The
iteration counts the tests cap at three times were taken from fire_ref on the CPU (tests/test_fire_host.py repeats the cheap
one): 334 iterations to g_max <= 1e-8 on fcc_box(), 37 to g_max <= 17 on clashing_water_box(), 47 to g_max <= 8 on
shake_ref.mixed_box() (dt_start = 0.001, dt_max = 0.01, max_step = 0.05 for the last two).

Tolerances of the parity test: fire_ref run on fcc_box() with the atoms in forward and in reversed order (another order of every
sum, the same mathematics) differs over 25 iterations by at most 2.8e-17 in a position and 2.3e-13 in the energy; the test
measures both again and allows 100 x each."""
import ctypes as C

import numpy as np
import pytest

from .helpers import fire_ref as fr
from .helpers import ortho_ref as oref
from .helpers import settle_ref as sr
from .helpers import shake_ref as hr
from .test_gpu_hbonds import _constraints_hold as _pairs_hold
from .test_gpu_hbonds import _engine as _mixed_engine
from .test_gpu_settle import _constraints_hold as _waters_hold
from .test_gpu_settle import _engine as _water_engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
P3 = [1, 1, 1]
EPS = float(np.finfo(np.float64).eps)
TOL = {np.float64: 1e-6, np.float32: 1e-4}             # (test_gpu_orthorhombic.py: energies against the all-pairs yardstick)
FCC_ITERS, WATER_ITERS, MIXED_ITERS = 334, 37, 47      # fire_ref's counts (module docstring)
WATER_FTOL, MIXED_FTOL = 17.0, 8.0
TIGHT = dict(dt_start=0.001, dt_max=0.01, max_step=0.05)
# 10 x the largest |F_fp32 - F_fp64| over the atoms of fcc_box() at the fp64 minimum (measured once on the device; the test
# measures it again and holds the constant to it within a factor of two)
F32_FTOL = 4.76e-4


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _engine(E, dev, B, dtype=np.float64, pos=None):
    pos = B["pos"] if pos is None else pos
    n = len(pos)
    return E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.zeros((n, 3), dtype=dtype), dev), float(B["lengths"][0]),
                            E.LennardJonesModel(float(B["rc"]), float(B["rs"])), E.cu(B["atoms"], dev), skin=float(B["skin"]),
                            inv_mass=E.cu((1.0 / B["mass"]).astype(dtype), dev), lo=list(fr.LO), lengths=list(B["lengths"]), periodic=P3)


def _reload(E, dev, md, B, dtype=np.float64):
    n = len(B["pos"])
    md.set_state_(E.cu(B["pos"].astype(dtype), dev), E.cu(np.zeros((n, 3), dtype=dtype), dev), E.cu(B["atoms"], dev),
                  E.cu((1.0 / B["mass"]).astype(dtype), dev))


def _get(md, what="positions"):
    st = md.state(positions=what == "positions", velocities=what == "velocities", forces=what == "forces")
    return st[what].cpu().numpy().astype(np.float64)


def _force(B, **kw):
    return fr.lj(fr.LO, B["lengths"], P3, float(B["rc"]), float(B["rs"]), B["atoms"], **kw)


def _refused(E, code, call, *args, **kw):
    with pytest.raises(E.EmDeeError) as err:
        call(*args, **kw)
    assert err.value.code == code, str(err.value)
    return str(err.value)


def _bytes(md):
    st = md.state()
    return tuple(st[k].cpu().numpy().tobytes() for k in ("positions", "velocities", "forces"))


def _projected_gmax(x, f, pairs, mass, lengths):
    """max |G_i| from the numpy projection of forces f at positions x (unwrapped over the pairs), and how much the same
    projection with the pairs in reversed order differs from it"""
    u = hr.unwrap(x, pairs, lengths)
    g = np.sqrt((fr.constrained_force(u, f, pairs, mass) ** 2).sum(axis=1).max())
    back = np.sqrt((fr.constrained_force(u, f, pairs[::-1], mass) ** 2).sum(axis=1).max())
    return g, abs(g - back)


# ---------------------------------------------------------------- 1. parity with the reference
_PARITY = {}


def _parity_reference():
    if not _PARITY:
        B = fr.fcc_box()
        fwd = fr.minimize(B["pos"], _force(B), B["mass"], 25, 0.0, keep=True, **fr.PARAMS)
        R = {k: v[::-1] for k, v in B.items() if k in ("pos", "mass", "atoms")}
        rev = fr.minimize(R["pos"], fr.lj(fr.LO, B["lengths"], P3, float(B["rc"]), float(B["rs"]), R["atoms"]), R["mass"], 25, 0.0, keep=True,
                          **fr.PARAMS)
        dx = max(np.abs(a - b[::-1]).max() for a, b in zip(fwd["xs"], rev["xs"]))
        de = max(abs(a[5] - b[5]) for a, b in zip(fwd["records"], rev["records"]))
        print("fire_ref, forward against reversed atom order over 25 iterations: max |dx| = %.3e, max |dE| = %.3e" % (dx, de))
        _PARITY.update(B=B, ref=fwd, dx=dx, de=de)
    return _PARITY


def test_parity_iterations_and_energies(emdee, dev):
    """(converged, iterations) and the energy of every iteration, through calls with max_iter = 0 .. 25 from the same state"""
    Q = _parity_reference()
    B, ref = Q["B"], Q["ref"]
    md = _engine(emdee, dev, B)
    worst = 0.0
    for k in range(26):
        _reload(emdee, dev, md, B)
        res = md.minimize_(k, 0.0, **fr.PARAMS)
        assert (res.converged, res.iterations) == (False, k)
        assert res.energy0 == pytest.approx(ref["energy0"], abs=100.0 * Q["de"])
        worst = max(worst, abs(res.energy - ref["records"][k][5]))
    print("energies of 26 calls against fire_ref: max |dE| = %.3e (allowed %.3e)" % (worst, 100.0 * Q["de"]))
    assert worst <= 100.0 * Q["de"]
    assert res.dt == ref["dt"]
    md.close()


def test_parity_positions(emdee, dev):
    """the positions after every iteration (calls with max_iter = 1 .. 25 from the same state) against fire_ref.
    Measured on the device: see DESIGN.md 4d."""
    Q = _parity_reference()
    B, ref = Q["B"], Q["ref"]
    md = _engine(emdee, dev, B)
    worst = 0.0
    for k in range(1, 26):
        _reload(emdee, dev, md, B)
        md.minimize_(k, 0.0, **fr.PARAMS)
        worst = max(worst, np.abs(_get(md) - ref["xs"][k]).max())
    print("positions of 25 calls against fire_ref: max |dx| = %.3e (allowed %.3e)" % (worst, 100.0 * Q["dx"]))
    assert worst <= 100.0 * Q["dx"]
    md.close()


# ---------------------------------------------------------------- 2. convergence
def test_convergence_to_1e_minus_8(emdee, dev):
    B = fr.fcc_box()
    md = _engine(emdee, dev, B)
    res = md.minimize_(3 * FCC_ITERS, 1e-8, **fr.PARAMS)
    print(res)
    assert res.converged and res.iterations <= 3 * FCC_ITERS and res.g_max <= 1e-8
    f, x = _get(md, "forces"), _get(md)
    assert res.g_max == pytest.approx(np.sqrt((f * f).sum(axis=1).max()), rel=8.0 * EPS)     # (the same planes, another order of the three squares)
    assert (_get(md, "velocities") == 0.0).all()
    want = oref.energy(x, fr.LO, B["lengths"], P3, float(B["rc"]), float(B["rs"]), B["atoms"])
    assert res.energy == pytest.approx(want, rel=TOL[np.float64]) and res.energy < res.energy0
    assert md.totals()[0] == pytest.approx(res.energy, rel=1e-12)                           # (emdee_md_energies adds the virials: a pass of its own)
    md.close()


# ---------------------------------------------------------------- 3. an overlapping start and the step cap
def test_overlap_start_and_the_step_cap(emdee, dev):
    B = fr.overlap_box()
    L = B["lengths"]
    P = dict(dt_start=0.005, dt_max=0.02, max_step=0.1)
    assert fr.closest_pair(B["pos"], L) == pytest.approx(0.6, abs=1e-12)
    # without the cap the first iteration throws the overlapping atoms further than max_step
    free = _engine(emdee, dev, B)
    before = _get(free)
    free.minimize_(1, 0.0, dt_start=0.005, dt_max=0.02, max_step=1e9)
    assert np.sqrt((oref.image_difference(_get(free), before, L, P3) ** 2).sum(axis=1).max()) > 0.1
    free.close()
    md = _engine(emdee, dev, B)
    margin = 8.0 * EPS * 0.1 + 4.0 * float(np.spacing(np.abs(before).max() + L.max()))       # (t^2 a / 2 in rounded arithmetic; two rounded positions)
    e0 = None
    for call in range(10):
        res = md.minimize_(1, 0.0, **P)
        e0 = res.energy0 if e0 is None else e0
        after = _get(md)
        moved = np.sqrt((oref.image_difference(after, before, L, P3) ** 2).sum(axis=1).max())
        print("call %d: largest displacement %.17g, energy %.6f" % (call, moved, res.energy))
        assert moved <= 0.1 + margin
        before = after
    res = md.minimize_(200, 0.0, **P)
    x = _get(md)
    assert np.isfinite(x).all() and np.isfinite(_get(md, "forces")).all() and np.isfinite([res.energy, res.g_max]).all()
    assert res.energy < e0 and res.iterations == 200
    assert fr.closest_pair(x, L) > 0.85
    md.close()


# ---------------------------------------------------------------- 4. rebuilds
def test_rebuilds_on_a_dilute_start(emdee, dev):
    B = fr.dilute_box()
    ref = fr.minimize(B["pos"], _force(B), B["mass"], 100, 0.0, **fr.PARAMS)
    assert ref["moved"] > float(B["skin"])                                                  # (1.02 against a skin of 0.3)
    md = _engine(emdee, dev, B)
    builds = md.nbr_stats()["builds"]
    res = md.minimize_(100, 0.0, **fr.PARAMS)
    print(res)
    assert res.rebuilds >= 1 and md.nbr_stats()["builds"] == builds + res.rebuilds
    want = oref.energy(_get(md), fr.LO, B["lengths"], P3, float(B["rc"]), float(B["rs"]), B["atoms"])
    assert res.energy == pytest.approx(want, rel=TOL[np.float64]) and res.energy < res.energy0
    md.close()


# ---------------------------------------------------------------- 5. rigid water, 6. both tables
def _constrained_case(md, res, pairs, mass, lengths):
    x, f = _get(md), _get(md, "forces")
    g, spread = _projected_gmax(x, f, pairs, mass, lengths)
    margin = 100.0 * max(spread, EPS * g)                   # (as in the parity test: 100 x what another order of the same sums changes, not below one rounding of g)
    print("g_max reported %.15g, numpy projection %.15g, allowed difference %.3e" % (res.g_max, g, margin))
    assert abs(res.g_max - g) <= margin
    assert res.energy < res.energy0
    assert (_get(md, "velocities") == 0.0).all()


def test_rigid_water_from_a_clashing_start(emdee, dev):
    B = fr.clashing_water_box()
    assert fr.closest_pair(B["unwrapped"], sr.LENGTHS, B["excl"]) < 0.4                    # (neighbours clash: the oxygens' sigma is 1)
    md = _water_engine(emdee, dev, B, vel=np.zeros_like(B["pos"]))
    res = md.minimize_(3 * WATER_ITERS, WATER_FTOL, **TIGHT)
    print(res)
    assert res.converged and res.g_max <= WATER_FTOL
    _waters_hold(md, B, np.float64, "minimised water")
    _constrained_case(md, res, hr.triangle_pairs(B["mol"], B["geom"]), B["mass"], sr.LENGTHS)
    md.step_(50, sr.DT)
    _waters_hold(md, B, np.float64, "50 steps after the minimisation")
    md.close()


def test_both_tables(emdee, dev):
    B = hr.mixed_box()
    md = _mixed_engine(emdee, dev, B, rigid=True, vel=np.zeros_like(B["pos"]))
    res = md.minimize_(3 * MIXED_ITERS, MIXED_FTOL, **TIGHT)
    print(res)
    assert res.converged and res.g_max <= MIXED_FTOL
    _pairs_hold(md, B, B["pairs"], np.float64, "minimised clusters and waters")
    _constrained_case(md, res, B["pairs"], B["mass"], hr.LENGTHS)
    md.step_(50, hr.DT)
    _pairs_hold(md, B, B["pairs"], np.float64, "50 steps after the minimisation")
    md.close()


# ---------------------------------------------------------------- 7. fp32 engines
def test_fp32_engine_holds_the_constraints_and_follows_the_fp64_energy(emdee, dev):
    B = hr.mixed_box()
    out = {}
    for dtype in (np.float64, np.float32):
        md = _mixed_engine(emdee, dev, B, dtype, rigid=True, vel=np.zeros_like(B["pos"]))
        out[dtype] = md.minimize_(MIXED_ITERS, 0.0, **TIGHT)
        if dtype == np.float32:
            _pairs_hold(md, B, B["pairs"], np.float32, "fp32, minimised", records=True)
        md.close()
    print(out[np.float64], out[np.float32])
    assert out[np.float32].energy == pytest.approx(out[np.float64].energy, rel=TOL[np.float32])
    assert out[np.float32].energy0 == pytest.approx(out[np.float64].energy0, rel=TOL[np.float32])


def test_fp32_engine_converges_to_its_force_noise(emdee, dev):
    B = fr.fcc_box()
    md = _engine(emdee, dev, B)
    assert md.minimize_(3 * FCC_ITERS, 1e-8, **fr.PARAMS).converged
    x, f64 = _get(md), _get(md, "forces")
    md.close()
    md = _engine(emdee, dev, B, np.float32, pos=x)
    noise = np.sqrt(((_get(md, "forces") - f64) ** 2).sum(axis=1).max())
    md.close()
    print("largest |F_fp32 - F_fp64| at the fp64 minimum: %.3e (F32_FTOL = %.3e)" % (noise, F32_FTOL))
    assert 0.5 * F32_FTOL <= 10.0 * noise <= 2.0 * F32_FTOL
    md = _engine(emdee, dev, B, np.float32)
    res = md.minimize_(3 * FCC_ITERS, F32_FTOL, **fr.PARAMS)
    print(res)
    assert res.converged and res.g_max <= F32_FTOL
    md.close()


# ---------------------------------------------------------------- 8. the charged path
def test_charged_flexible_water_with_the_reaction_field(emdee, dev):
    E = emdee
    from .helpers import bonded_ref as br
    w = E.synthetic.water_box(5)
    N, L = w["positions"].shape[0], w["L"]
    pos = np.mod(w["positions"] + np.random.default_rng(7).uniform(-0.005, 0.005, (N, 3)), L)
    terms = [(br.BOND, w["bonds"], w["bond_params"]), (br.ANGLE, w["angles"], w["angle_params"])]
    rc, rs = 0.6, 0.5
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(np.zeros((N, 3)), dev), L, E.LennardJonesModel(rc, rs), E.cu(w["atoms"], dev), skin=0.1,
                          inv_mass=E.cu(w["inv_mass"].astype(np.float64), dev))
    md.set_exclusions_(w["exclusions"])
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
    res = md.minimize_(60, 0.0, dt_start=0.0002, dt_max=0.002, max_step=0.01)
    print(res)
    assert res.iterations == 60 and res.energy < res.energy0
    want = oref.energy(_get(md), [0.0] * 3, [L] * 3, P3, rc, rs, w["atoms"], terms, excl=w["exclusions"], charges=w["charges"],
                       coulomb_k=E.COULOMB_K_KJ_NM, eps_rf=np.inf)
    assert res.energy == pytest.approx(want, rel=TOL[np.float64])
    md.close()


# ---------------------------------------------------------------- 9. reproducibility and bookkeeping
def test_reproducibility_and_bookkeeping(emdee, dev):
    B = fr.clashing_water_box()
    out = []
    for _ in range(2):
        md = _water_engine(emdee, dev, B, vel=np.zeros_like(B["pos"]))
        md.profile_(True)
        res = md.minimize_(30, 0.0, **TIGHT)
        ms, launches = md.kernel_time("minimize")
        assert launches > 0 and ms > 0.0
        assert md.kernel_time("settle")[1] >= 3 * res.iterations                           # (stages (a), (c), (e) of every step; (e) again behind a mixing)
        assert md.kernel_time("molecular") == (0.0, 0) and md.kernel_time("hbonds") == (0.0, 0)
        assert md.kernel_time(12) == (ms, launches)
        assert (_get(md, "velocities") == 0.0).all()
        out.append((_bytes(md), (res.iterations, res.converged, res.rebuilds, res.energy0, res.energy, res.g_max, res.dt)))
        md.step_(5, sr.DT)                                                                  # (no set_state in between)
        _waters_hold(md, B, np.float64, "5 steps after the minimisation")
        md.close()
    assert out[0] == out[1]


def test_thermostat_is_left_out_and_comes_back(emdee, dev):
    B = fr.fcc_box()
    a, b = _engine(emdee, dev, B), _engine(emdee, dev, B)
    b.set_langevin_(1.0, 1.0, seed=3)
    ra, rb = a.minimize_(20, 0.0, **fr.PARAMS), b.minimize_(20, 0.0, **fr.PARAMS)
    assert _bytes(a) == _bytes(b) and ra.energy == rb.energy
    a.step_(3, 0.002)
    b.step_(3, 0.002)
    assert _bytes(a) != _bytes(b)                                                           # (b's thermostat is on again)
    a.close()
    b.close()


# ---------------------------------------------------------------- 10. refusals
def test_refusals_leave_the_state_as_it_is(emdee, dev):
    E = emdee
    B = fr.clashing_water_box()
    md = _water_engine(E, dev, B)
    before = _bytes(md)
    nan, inf = float("nan"), float("inf")
    for args in ((-1, 1.0, 0.001, 0.01, 0.05), (5, 1.0, 0.02, 0.01, 0.05), (5, 1.0, 0.001, 0.01, 0.0), (5, 1.0, 0.001, 0.01, -0.1),
                 (5, nan, 0.001, 0.01, 0.05), (5, -1.0, 0.001, 0.01, 0.05), (5, 1.0, 0.0, 0.01, 0.05), (5, 1.0, 0.001, inf, 0.05),
                 (5, 1.0, 0.001, 0.01, nan), (5, inf, 0.001, 0.01, 0.05)):
        text = _refused(E, ERR_INVALID, md.minimize_, *args)
        assert "md_minimize" in text
        assert _bytes(md) == before
    md.close()
    # a stale table: a state of another atom count under the table in force (no exclusions: they would refuse the state themselves)
    md = _water_engine(E, dev, B, excl=False)
    n = len(B["pos"]) - 3
    md.set_state_(E.cu(B["pos"][:n], dev), E.cu(B["vel"][:n], dev), E.cu(B["atoms"][:n], dev), E.cu(1.0 / B["mass"][:n], dev))
    before = _bytes(md)
    assert "rigid molecules" in _refused(E, ERR_STATE, md.minimize_, 5, 1.0, **TIGHT)
    assert _bytes(md) == before
    md.close()
    # out == NULL is accepted
    md = _water_engine(E, dev, B)
    E._lib.call("emdee_md_minimize", md._handle, 3, 0.0, 0.001, 0.01, 0.05, None)
    _waters_hold(md, B, np.float64, "after a call without a result")
    md.close()
    # no state loaded
    h = C.c_void_p()
    ctx = E.device.context_for(dev)
    E._lib.call("emdee_md_create", ctx.handle, (C.c_double * 3)(*fr.LO), (C.c_double * 3)(*sr.LENGTHS), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(E.LennardJonesModel(sr.RC, sr.RS)), float(sr.SKIN), 8, C.byref(h))
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_minimize", h, 3, 0.0, 0.001, 0.01, 0.05, None)
    assert err.value.code == ERR_STATE and "no state loaded" in str(err.value)
    E._lib.call("emdee_md_destroy", h)


def test_an_engine_lent_by_a_decomposition_refuses_the_call(emdee, dev):
    from .test_gpu_dd_pairs import _build
    E = emdee
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    view = dd.engine(0)
    before = _bytes(view)
    text = _refused(E, ERR_STATE, view.minimize_, 5, 1.0)
    assert "emdee_dd_engine" in text and _bytes(view) == before
    dd.step_(2, 0.005)                                                                   # the decomposition is unharmed
    dd.close()
