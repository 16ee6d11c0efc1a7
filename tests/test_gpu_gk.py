"""GPU tests of the Green-Kubo observables (include/emdee_hip.h: emdee_md_set_gk; csrc/gk.hpp).

The stress words of a sample are compared bit for bit with the words numpy forms (tests/helpers/gk_ref.py: stress_words) from the
twelve sums emdee_md_pressure_tensor (or, with rigid molecules, emdee_md_molecular_pressure_tensor) returns for the same state: the
sample queues the same kernels and does the same arithmetic on the device.  The heat flux is compared with gk_ref on the positions
and velocities of md.state(): fields from tests/helpers/ortho_ref.py, relative to the sum of the absolute addends, 1e-12 for an
fp64 engine and 1e-5 for a Float32 one -- the figures tests/test_gpu_virial_tensor.py holds the virial sums to against the same numpy
field.  The lag sums and the totals are compared with numpy's brute-force enumeration over the recorded samples within
2 n 2^-53 sum |addends| (gk_ref.bound)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import barostat_ref as bref
from .helpers import gk_ref as gr
from .helpers import ortho_ref as oref
from .helpers import settle_ref as sr
from . import test_gpu_orthorhombic as ortho
from .test_gpu_barostat import DT, _engine, _fluid
from .test_gpu_dd_pairs import _build
from .test_gpu_hbonds import _engine as _hbonds_engine
from .test_gpu_settle import _engine as _water_engine
from .test_gpu_settle import _refused
from .helpers import shake_ref as hr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
HEAT_REL = {np.float64: 1e-12, np.float32: 1e-5}
# launches under emdee_md_kernel_time index 17 per sample (include/emdee_hip.h)
LAUNCHES = {"stress": 4, "stress, rigid": 5, "heat": 4, "both": 6}


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _frame(md):
    st = md.state(forces=False)
    return st["positions"].cpu().numpy().astype(np.float64), st["velocities"].cpu().numpy().astype(np.float64)


def _heat_reference(md, lo, lengths, periodic, rc, rs, atoms, inv_mass=None, **kw):
    x, v = _frame(md)
    out = oref.nonbonded(x, lo, np.asarray(lengths, dtype=np.float64), periodic, rc, rs, atoms, **kw)
    return gr.heat_flux_fields(v, out["e"], out["t"], inv_mass)


def _check_sample(md, what, dtype, heat_ref, sums=None):
    """the sample just taken: words 0-5 bit for bit from the engine's own twelve sums, words 6-8 against the numpy heat flux"""
    last = md.green_kubo()["last"]
    want = gr.stress_words(md.tensor_sums() if sums is None else sums)
    assert last[:6].tobytes() == want.tobytes(), (what, last[:6], want)
    J, A = heat_ref()
    gap = np.abs(last[6:] - J)
    print("%s: J = %r, |dev - ref| / sum |addends| = %r (bound %.0e)" % (what, last[6:], gap / A, HEAT_REL[dtype]))
    assert (gap <= HEAT_REL[dtype] * A).all(), (what, gap, A)
    assert (np.abs(J) > 100 * HEAT_REL[dtype] * A).any()     # (not a sum that vanishes by symmetry)
    return last


def _check_sums(out, lasts, n_lags, what):
    ref = gr.correlate(lasts, n_lags)
    b_sums, b_totals = gr.bound(ref)
    assert out["samples"] == len(lasts) and np.array_equal(out["counts"], ref["counts"])
    gap, gap_t = np.abs(out["sums"] - ref["sums"]), np.abs(out["totals"] - ref["totals"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print("%s: largest |dev - ref| / bound: sums %.3f, totals %.3f" % (what, np.nanmax(gap / b_sums), np.nanmax(gap_t / b_totals)))
    assert (gap <= b_sums).all(), (what, np.argwhere(gap > b_sums)[:5])
    assert (gap_t <= b_totals).all(), what
    assert (out["sums"][0] > 0.0).all()                      # (lag 0: sums of squares of nine words none of which is zero)


# ---------------------------------------------------------------- 1, 2. the fluid, both precisions
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fluid_every_sample_and_every_sum_while_the_ring_wraps(emdee, dev, dtype):
    """864 atoms, three cells a side, NVE; both bits, n_lags = 5, 13 samples three steps apart: the ring wraps twice and the
    neighbour list is rebuilt under it"""
    E = emdee
    S, md = _fluid(E, dev, dtype)
    L3 = [S["L"]] * 3
    md.set_green_kubo_(5)
    builds = md.nbr_stats()["builds"]
    zero = md.green_kubo()
    assert (zero["last"] == 0.0).all() and zero["samples"] == 0 and np.isnan(zero["stress_acf"]).all()
    lasts = []
    for k in range(13):
        if k:
            md.step_(3, DT)
        md.gk_sample_()
        lasts.append(_check_sample(md, "fluid %s, sample %d" % (np.dtype(dtype).name, k), dtype,
                                   lambda: _heat_reference(md, np.zeros(3), L3, [1, 1, 1], bref.RC, bref.RS, S["atoms"])))
    grew = md.nbr_stats()["builds"] - builds
    print("%d builds between the first and the last sample" % grew)
    assert grew >= 1
    out = md.green_kubo(dt_sample=3 * DT, temperature=1.4)
    assert list(out["counts"]) == [13, 12, 11, 10, 9] and list(out["lags"]) == list(range(5))
    assert out["last"].tobytes() == lasts[-1].tobytes()
    _check_sums(out, lasts, 5, "fluid %s" % np.dtype(dtype).name)
    # the derived curves are the words over the counts
    mean = out["sums"] / out["counts"][:, None]
    assert np.allclose(out["stress_acf"], mean[:, :5].mean(axis=1), rtol=1e-15)
    assert np.allclose(out["heat_acf"], mean[:, 6:].mean(axis=1), rtol=1e-15)
    assert np.allclose(out["pressure_acf"], mean[:, 5] - (out["totals"][5] / 13.0) ** 2, rtol=1e-12)
    V = S["L"] ** 3
    assert out["eta"][0] == 0.0 and np.isclose(out["eta"][1], 0.5 * (out["stress_acf"][0] + out["stress_acf"][1]) * 3 * DT / (V * 1.4), rtol=1e-14)
    assert np.isclose(out["lambda_"][-1], (0.5 * (out["heat_acf"][1:] + out["heat_acf"][:-1]) * 3 * DT).sum() / (V * 1.4 ** 2), rtol=1e-12)
    md.close()


# ---------------------------------------------------------------- 3. an orthorhombic box with lo != 0
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_orthorhombic_box_with_an_offset_origin(emdee, dev, dtype):
    E = emdee
    S = ortho._system(E.synthetic, ortho.SMALL, dtype, seed=ortho.SEEDS["single"], lo=True)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    md = ortho._engine(E, S, atoms, dev)
    md.step_(7, DT)
    md.set_green_kubo_(3)
    md.gk_sample_()
    last = _check_sample(md, "orthorhombic %s" % np.dtype(dtype).name, dtype,
                         lambda: _heat_reference(md, S["lo"], S["lengths"], S["periodic"], S["rc"], S["rs"], atoms))
    out = md.green_kubo()
    assert out["samples"] == 1 and list(out["counts"]) == [1, 0, 0]
    assert np.array_equal(out["sums"][0], last * last) and (out["sums"][1:] == 0.0).all() and np.array_equal(out["totals"], last)
    assert np.isnan(out["stress_acf"][1:]).all() and out["stress_acf"][0] > 0.0
    md.close()


# ---------------------------------------------------------------- 4. reaction-field charges
def test_charged_fluid_with_the_reaction_field(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    q = 0.6 * (1.0 - 2.0 * (np.arange(864) % 2))
    kw = dict(charges=q, coulomb_k=1.5, eps_rf=78.0)
    md.set_coulomb_(q, 1.5, 78.0)
    md.step_(5, DT)
    md.set_green_kubo_(2)
    md.gk_sample_()
    L3 = [S["L"]] * 3
    _check_sample(md, "reaction field", np.float64, lambda: _heat_reference(md, np.zeros(3), L3, [1, 1, 1], bref.RC, bref.RS, S["atoms"], **kw))
    # the Coulomb part is a visible share of J: the reference without charges is far outside the bound
    J0, A0 = _heat_reference(md, np.zeros(3), L3, [1, 1, 1], bref.RC, bref.RS, S["atoms"])
    assert (np.abs(md.green_kubo()["last"][6:] - J0) > 1e-6 * A0).all()
    md.close()


# ---------------------------------------------------------------- 5. rigid water: the molecular stress
def test_rigid_water_takes_the_molecular_stress_and_refuses_the_heat_flux(emdee, dev):
    E = emdee
    B = sr.water_box()
    md = _water_engine(E, dev, B)
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, 1.0, 0.1, every=2, seed=3)
    for heat, stress in ((True, True), (True, False)):
        text = _refused(E, ERR_STATE, md.set_green_kubo_, 4, stress=stress, heat=heat)
        assert "emdee_md_set_rigid3" in text and "EMDEE_GK_HEAT" in text
    md.step_(4, sr.DT)                                       # the engine still steps
    md.set_green_kubo_(4, heat=False)
    md.profile_(True)
    lasts = []
    for k in range(3):
        md.step_(4, sr.DT)
        md.gk_sample_()
        last = md.green_kubo()["last"]
        mol, atomic = md.molecular_tensor_sums(), md.tensor_sums()
        assert last[:6].tobytes() == gr.stress_words(mol).tobytes()
        assert last[:6].tobytes() != gr.stress_words(atomic).tobytes() and (last[6:] == 0.0).all()
        lasts.append(last)
    assert md.kernel_time("green_kubo")[1] == 3 * LAUNCHES["stress, rigid"]
    md.profile_(False)
    _check_sums_stress_only(md.green_kubo(), lasts, 4, "water")
    md.close()


def _check_sums_stress_only(out, lasts, n_lags, what):
    ref = gr.correlate(lasts, n_lags)
    b_sums, b_totals = gr.bound(ref)
    assert out["samples"] == len(lasts) and np.array_equal(out["counts"], ref["counts"])
    assert (np.abs(out["sums"] - ref["sums"]) <= b_sums).all() and (np.abs(out["totals"] - ref["totals"]) <= b_totals).all(), what
    assert (out["sums"][..., 6:] == 0.0).all() and (out["totals"][6:] == 0.0).all() and (out["sums"][0, :6] > 0.0).all()


# ---------------------------------------------------------------- 6. sampling leaves the run alone
def _bits(md):
    st = md.state()
    return [st[k].cpu().numpy().tobytes() for k in ("positions", "velocities", "forces")]


def test_sampling_does_not_change_the_run(emdee, dev):
    E = emdee
    S, a = _fluid(E, dev)
    _, b = _fluid(E, dev)
    b.set_green_kubo_(6)
    b.gk_sample_()
    for _ in range(20):
        a.step_(2, DT)
        b.step_(2, DT)
        b.gk_sample_()
    assert _bits(a) == _bits(b) and a.nbr_stats() == b.nbr_stats()
    assert a.totals() == b.totals()
    assert b.green_kubo()["samples"] == 21
    a.close()
    b.close()


# ---------------------------------------------------------------- 7. reproducibility, reading twice, reset
def test_sums_are_bitwise_reproducible_and_reset_starts_again(emdee, dev):
    E = emdee
    runs = []
    for _ in range(2):
        S, md = _fluid(E, dev)
        md.set_green_kubo_(4)

        def run():
            for k in range(7):
                md.gk_sample_()
                md.step_(3, DT)
            first, again = md.green_kubo(), md.green_kubo()
            assert first["sums"].tobytes() == again["sums"].tobytes() and first["totals"].tobytes() == again["totals"].tobytes()
            assert first["samples"] == 7 and (first["sums"][0] > 0).all()
            return first
        runs.append(run())
        md.gk_reset_()
        zero = md.green_kubo()
        assert (zero["sums"] == 0.0).all() and (zero["totals"] == 0.0).all() and (zero["last"] == 0.0).all() and zero["samples"] == 0
        assert np.isnan(zero["stress_acf"]).all() and np.isnan(zero["heat_acf"]).all() and np.isnan(zero["pressure_acf"]).all()
        # the same state again: a rerun after the reset reproduces the first run's bits
        md.set_state_(E.cu(S["pos"], dev), E.cu(S["vel"], dev), E.cu(S["atoms"], dev))
        md.gk_reset_()
        runs.append(run())
        md.close()
    for k in (1, 2, 3):
        assert runs[0]["sums"].tobytes() == runs[k]["sums"].tobytes() and runs[0]["totals"].tobytes() == runs[k]["totals"].tobytes()
        assert runs[0]["last"].tobytes() == runs[k]["last"].tobytes()


# ---------------------------------------------------------------- 8. masks
def test_masks_keep_the_other_words_at_exactly_zero(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    md.profile_(True)
    md.set_green_kubo_(3, heat=False)
    for k in range(4):
        md.gk_sample_()
        md.step_(3, DT)
    out = md.green_kubo()
    assert (out["sums"][..., 6:] == 0.0).all() and (out["totals"][6:] == 0.0).all() and (out["last"][6:] == 0.0).all()
    assert (out["sums"][0, :6] > 0.0).all() and out["samples"] == 4
    assert md.kernel_time("green_kubo")[1] == 4 * LAUNCHES["stress"]
    md.profile_(True)                                        # (resets the timers)
    md.set_green_kubo_(3, stress=False)
    for k in range(4):
        md.gk_sample_()
        md.step_(3, DT)
    out = md.green_kubo()
    assert (out["sums"][..., :6] == 0.0).all() and (out["totals"][:6] == 0.0).all() and (out["last"][:6] == 0.0).all()
    assert (out["sums"][0, 6:] > 0.0).all() and out["samples"] == 4
    assert md.kernel_time("green_kubo")[1] == 4 * LAUNCHES["heat"]
    md.profile_(False)
    md.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_table_and_the_sums_in_force(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    for call in (md.gk_sample_, md.gk_reset_):
        assert "no table" in _refused(E, ERR_STATE, call)
    assert "no table" in _refused(E, ERR_STATE, E._lib.call, "emdee_md_gk_read", md._handle, None, None, None, None)
    md.set_green_kubo_(4)
    md.gk_sample_()
    md.step_(3, DT)
    md.gk_sample_()
    before = md.green_kubo()

    def intact(samples=2):
        now = md.green_kubo()
        return now["sums"].tobytes() == before["sums"].tobytes() and now["totals"].tobytes() == before["totals"].tobytes() and now["samples"] == samples

    raw = lambda what, n_lags: E._lib.call("emdee_md_set_gk", md._handle, what, n_lags)
    assert "EMDEE_GK_STRESS | EMDEE_GK_HEAT" in _refused(E, ERR_INVALID, raw, 0, 4)
    assert "EMDEE_GK_STRESS | EMDEE_GK_HEAT" in _refused(E, ERR_INVALID, raw, 4, 4)
    assert "n_lags = -1" in _refused(E, ERR_INVALID, raw, 3, -1)
    assert "n_lags = 65537" in _refused(E, ERR_INVALID, raw, 3, 65537)
    assert intact()
    # every table that is not a pair term of the neighbour rows: the heat flux is refused at set and at sample, with its setter
    # named; the stress alone is accepted (and dropped again); once the table is cleared the table in force samples on
    bond = ([[0, 1]], [[10.0, 1.1]])
    attach = {
        "emdee_md_set_exclusions": (lambda: md.set_exclusions_([[0, 1]]), lambda: md.set_exclusions_(None)),
        "emdee_md_set_pairs14": (lambda: md.set_pairs14_([[0, 1]], 0.5), lambda: md.set_pairs14_(None, 1.0)),
        "emdee_md_set_bonded": (lambda: md.set_bonded_(E.HARMONIC_BOND, *bond), lambda: md.set_bonded_(E.HARMONIC_BOND, [], [])),
    }
    samples = 2
    for setter, (on, off) in attach.items():
        on()
        assert setter in _refused(E, ERR_STATE, md.gk_sample_) and intact(samples)
        text = _refused(E, ERR_STATE, md.set_green_kubo_, 4)
        assert setter in text and "EMDEE_GK_HEAT" in text and intact(samples)
        off()
        md.gk_sample_()
        samples += 1
        assert md.green_kubo()["samples"] == samples
        before = md.green_kubo()
    # Ewald and PME (a charged engine; the reaction field itself is accepted)
    md.set_coulomb_(0.3 * (1.0 - 2.0 * (np.arange(864) % 2)), 1.0)
    md.gk_sample_()
    samples += 1
    before = md.green_kubo()
    md.set_ewald_(1.0, 4)
    assert "emdee_md_set_ewald" in _refused(E, ERR_STATE, md.gk_sample_) and intact(samples)
    assert "emdee_md_set_ewald" in _refused(E, ERR_STATE, md.set_green_kubo_, 4) and intact(samples)
    md.set_pme_(1.0, 16, 4)
    assert "emdee_md_set_pme" in _refused(E, ERR_STATE, md.gk_sample_) and intact(samples)
    assert "emdee_md_set_pme" in _refused(E, ERR_STATE, md.set_green_kubo_, 4, stress=False) and intact(samples)
    md.set_pme_(0.0)
    md.set_coulomb_(None, 1.0)
    md.gk_sample_()
    samples += 1
    before = md.green_kubo()
    # a rescaled box: refused until a reset
    md.scale_box_(0.999)
    assert "emdee_md_gk_reset" in _refused(E, ERR_STATE, md.gk_sample_) and intact(samples)
    md.gk_reset_()
    md.gk_sample_()
    assert md.green_kubo()["samples"] == 1
    # a new state of the same size: refused until a reset
    md.set_state_(E.cu(S["pos"] * 0.999, dev), E.cu(S["vel"], dev), E.cu(S["atoms"], dev))
    after = md.green_kubo()
    assert "emdee_md_set_state" in _refused(E, ERR_STATE, md.gk_sample_)
    assert md.green_kubo()["sums"].tobytes() == after["sums"].tobytes() and md.green_kubo()["samples"] == 1
    md.gk_reset_()
    md.gk_sample_()
    assert list(md.green_kubo()["counts"]) == [1, 0, 0, 0]
    # another atom count: refused until the table is set again
    md.set_state_(E.cu(S["pos"][:-3] * 0.999, dev), E.cu(S["vel"][:-3], dev), E.cu(S["atoms"][:-3], dev))
    assert "861" in _refused(E, ERR_STATE, md.gk_sample_)
    md.gk_reset_()
    assert "861" in _refused(E, ERR_STATE, md.gk_sample_)
    md.set_green_kubo_(4)
    md.gk_sample_()
    assert md.green_kubo()["samples"] == 1
    md.set_green_kubo_(0)                                    # cleared
    assert "no table" in _refused(E, ERR_STATE, md.gk_sample_)
    with pytest.raises(ValueError):
        md.green_kubo()
    md.close()


def test_hbonds_and_virtual_sites_are_refused(emdee, dev):
    """an hbonds table refuses every mask, at set and -- attached later -- at sample; virtual sites refuse the heat flux"""
    E = emdee
    B = hr.mixed_box()
    md = _hbonds_engine(E, dev, B, hbonds=False)
    md.set_green_kubo_(3, heat=False)
    md.gk_sample_()
    md.set_hbonds_(B["clusters"], B["dist"])
    assert "emdee_md_set_hbonds" in _refused(E, ERR_STATE, md.gk_sample_)
    for stress, heat in ((True, False), (False, True), (True, True)):
        assert "emdee_md_set_hbonds" in _refused(E, ERR_STATE, md.set_green_kubo_, 3, stress=stress, heat=heat)
    assert md.green_kubo()["samples"] == 1
    md.set_hbonds_(None, None)
    md.gk_sample_()                                          # the table in force samples on
    assert md.green_kubo()["samples"] == 2
    md.close()
    from .helpers import vsite_ref as vr
    from .test_gpu_vsites import _engine as _site_engine
    V = vr.four_site_box()
    md = _site_engine(E, dev, V)
    text = _refused(E, ERR_STATE, md.set_green_kubo_, 3)
    assert "emdee_md_set_vsites" in text and "emdee_md_set_rigid3" in text and "emdee_md_set_exclusions" in text
    md.set_green_kubo_(3, heat=False)                        # the molecular stress of the four-site water
    md.gk_sample_()
    assert md.green_kubo()["last"][:6].tobytes() == gr.stress_words(md.molecular_tensor_sums()).tobytes()
    md.close()


def test_lent_unloaded_and_ghost_engines_refuse_a_table(emdee, dev):
    E = emdee
    S = bref.fluid864(E.synthetic)
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (a decomposition needs two bricks of 2.8 + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    assert "lent" in _refused(E, ERR_STATE, dd.engine(0).set_green_kubo_, 4)
    dd.step_(2, DT)                                                                      # the decomposition is unharmed
    dd.close()
    model = E.LennardJonesModel(bref.RC, bref.RS)
    g = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"][:-4], dev), S["L"], model, E.cu(S["atoms"], dev), skin=bref.SKIN, n_ghost=4)
    assert "ghosts" in _refused(E, ERR_STATE, g.set_green_kubo_, 4)
    g.close()
    # before emdee_md_set_state, through the C ABI
    ctx = E.context_for(dev)
    h = C.c_void_p()
    three = lambda *v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", ctx.handle, three(0, 0, 0), three(S["L"], S["L"], S["L"]), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(model), bref.SKIN, 8, C.byref(h))
    assert "no state loaded" in _refused(E, ERR_STATE, E._lib.call, "emdee_md_set_gk", h, 3, 4)
    E._lib.call("emdee_md_set_gk", h, 3, 0)                 # clearing nothing is fine
    E._lib.call("emdee_md_destroy", h)


# ---------------------------------------------------------------- 10. the timer
def test_kernel_time_counts_the_launches_a_sample_adds(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    md.set_green_kubo_(4)
    assert md.kernel_time("green_kubo") == (0.0, 0)
    md.profile_(True)
    assert md.kernel_time("green_kubo") == (0.0, 0)
    for _ in range(5):
        md.gk_sample_()
        md.step_(2, DT)
    ms, launches = md.kernel_time("green_kubo")
    assert launches == 5 * LAUNCHES["both"] and ms > 0.0 and md.kernel_time(17) == (ms, launches)
    md.profile_(False)
    md.close()


# ---------------------------------------------------------------- 11. the example
def test_example_prints_positive_running_viscosity_and_conductivity(emdee):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lj_viscosity.py"), "--cells", "6", "--melt", "400", "--steps", "1200",
                        "--every", "4", "--lags", "30"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = np.array([[float(t) for t in line.split()] for line in r.stdout.splitlines() if line and line[0].isdigit()])
    final = {line.split("=")[0].strip(): float(line.split("=")[1]) for line in r.stdout.splitlines() if line.startswith(("eta ", "lambda "))}
    print(r.stdout.splitlines()[0], r.stdout.splitlines()[1], final)
    assert rows.shape == (30, 5) and np.isfinite(rows).all()
    assert (rows[1:, 3] > 0.0).all() and (rows[1:, 4] > 0.0).all()                       # the running eta and lambda
    assert set(final) == {"eta", "lambda"} and all(np.isfinite(v) and v > 0.0 for v in final.values())
