"""GPU tests of the mean-squared displacement and the velocity autocorrelation (include/emdee_hip.h: emdee_md_set_msd; csrc/msd.hpp).
The reference is always tests/helpers/msd_ref.py, plain numpy over the positions and velocities md.state() returned at every sample,
with its own enumeration of the pairs of frames.

The tolerances are derived, not measured (msd_ref.bound64 / bound32).  An fp64 engine's snapshot is bit for bit what state()
returns, so only the order of summation and the contraction of multiply-adds differ: per word |dev - ref| <= 2^-50 (N_g + origins +
8) A, A the sum of the absolute addends, twice that for the squared drift.  A Float32 engine takes unrounded doubles where state()
rounds to fp32: with X the largest |unwrapped coordinate| and delta = 2 x 2^-24 X, w0-2 may differ by sum (2 |d_i| delta + delta^2)
more, w3-5 by 2 |S1| N_g delta + N_g^2 delta^2 per origin, w6 by nothing more; that this bound cannot hide a failure is asserted:
it stays below 1e-3 of w0 + w1 + w2 at every lag >= 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import barostat_ref as bref
from .helpers import msd_ref as mr
from .helpers import settle_ref as sr
from . import test_gpu_orthorhombic as ortho
from .test_gpu_barostat import DT, PATHS, _engine, _fluid, _path
from .test_gpu_dd_pairs import _build
from .test_gpu_settle import _engine as _water_engine
from .test_gpu_settle import _refused

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
MSD_CHUNK = 1024                                           # csrc/msd.hpp (tests/test_msd_host.py reads it from the header's program)


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _frame(md):
    st = md.state(forces=False)
    return st["positions"].cpu().numpy().astype(np.float64), st["velocities"].cpu().numpy().astype(np.float64)


def _sampled(md, n_samples, steps, dt=DT):
    """n_samples samples, `steps` steps apart, the first one of the state as it is; the frames the reference works on"""
    xs, vs = [], []
    for k in range(n_samples):
        if k:
            md.step_(steps, dt)
        x, v = _frame(md)
        xs.append(x)
        vs.append(v)
        md.msd_sample_()
    return xs, vs


def _check(out, ref, what, x_max=None):
    """every word, lag and origins entry against the reference, within the derived bound (x_max: a Float32 engine)"""
    bound = mr.bound64(ref) if x_max is None else mr.bound32(ref, x_max)
    gap = np.abs(out["sums"] - ref["sums"])
    for w in range(mr.WORDS):
        worst = np.argmax(gap[..., w])
        l, g = np.unravel_index(worst, gap.shape[:2])
        print("%s: word %d: largest gap at lag %d group %d: |dev - ref| %.3e, bound %.3e, word %.6e"
              % (what, w, l, g, gap[l, g, w], bound[l, g, w], ref["sums"][l, g, w]))
    assert np.array_equal(out["origins"], ref["origins"]), what
    assert out["group_sizes"] == [int(s) for s in ref["sizes"]], what
    assert (gap <= bound).all(), (what, np.argwhere(gap > bound)[:5])
    if x_max is not None:
        total = ref["sums"][1:, :, 0:3].sum(axis=2)
        live = (ref["origins"][1:, None] * ref["sizes"][None, :]) > 0
        assert (bound[1:][live] < 1e-3 * total[live][:, None]).all(), (what, (bound[1:] / np.maximum(total[..., None], 1e-300)).max())
    return bound


# ---------------------------------------------------------------- 1. ring reuse across rebuilds
@pytest.mark.parametrize("path", PATHS)
def test_fluid_every_word_while_the_ring_is_reused_across_rebuilds(emdee, dev, monkeypatch, path):
    """n_lags = 6 with an origin every 2 samples: three ring slots; 13 samples, 5 steps apart, write each slot at least twice while
    the list is rebuilt under the snapshots and atoms leave the box"""
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    L = S["L"]
    md.set_msd_(6, origin_every=2)
    builds = md.nbr_stats()["builds"]
    xs, vs = _sampled(md, 13, 5)
    outside = ((xs[-1] < 0.0) | (xs[-1] >= L)).any(axis=1).sum()
    grew = md.nbr_stats()["builds"] - builds
    print("fluid, %s: %d atoms outside the box at the last sample, %d builds between the first and the last" % (path, outside, grew))
    assert outside >= 50 and grew >= 2
    ref = mr.correlate(xs, vs, 6, 2)
    assert list(ref["origins"]) == [7, 6, 6, 5, 5, 4]
    out = md.msd()
    assert out["samples"] == 13 and list(out["lags"]) == list(range(6))
    _check(out, ref, "fluid, " + path)
    # the derived curves are the words over origins N_g
    count = ref["origins"][:, None] * 864.0
    assert np.allclose(out["msd"][..., 3], out["sums"][..., 0:3].sum(axis=2) / count, rtol=1e-15)
    assert np.allclose(out["msd"][..., 0:3], out["sums"][..., 0:3] / count[..., None], rtol=1e-15)
    assert np.allclose(out["vacf"], out["sums"][..., 6] / count, rtol=1e-15)
    assert (out["msd"][0] == 0.0).all() and (np.diff(out["msd"][:, 0, 3]) > 0).all()
    md.close()


# ---------------------------------------------------------------- 2. chunk edges and table order
def test_groups_interleaved_by_id_at_the_chunk_edges(emdee, dev):
    """4000 atoms: a group over three chunks with a part-filled last one, a group of exactly one chunk, a group of one atom, the
    rest left out; the members of every group are scattered over the ids"""
    E = emdee
    pos, L = E.synthetic.fcc_positions(10)
    n = pos.shape[0]
    assert n == 4000
    sizes = [2 * MSD_CHUNK + 100, MSD_CHUNK, 1]
    order = np.random.default_rng(9).permutation(n)
    groups = np.full(n, -1, dtype=np.int64)
    at = 0
    for g, s in enumerate(sizes):
        groups[order[at:at + s]] = g
        at += s
    md = _engine(E, dev, pos, E.synthetic.velocities(n, temperature=1.4), L, bref.lj_atoms(n))
    md.set_msd_(4, origin_every=1, groups=groups)
    xs, vs = _sampled(md, 6, 5)
    ref = mr.correlate(xs, vs, 4, 1, groups, 3)
    assert list(ref["sizes"]) == sizes and list(ref["origins"]) == [6, 5, 4, 3]
    _check(md.msd(), ref, "chunk edges")
    md.close()


# ---------------------------------------------------------------- 3. whole box lengths and drift
def test_drifting_fluid_crosses_whole_box_lengths(emdee, dev):
    E = emdee
    S = bref.fluid864(E.synthetic)
    L = S["L"]
    md = _engine(E, dev, S["pos"], S["vel"] + np.array([4.0, -3.0, 2.0]), L, S["atoms"])
    md.set_msd_(11, origin_every=5)
    xs, vs = _sampled(md, 11, 100)
    image = np.floor(xs[-1][:, 0] / L) - np.floor(xs[0][:, 0] / L)
    print("drift: x images changed by %d to %d" % (image.min(), image.max()))
    assert image.min() >= 1 and image.max() >= 2
    ref = mr.correlate(xs, vs, 11, 5)
    assert list(ref["origins"]) == [3, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1]
    out = md.msd()
    bound = _check(out, ref, "drift")
    # the drift is most of the displacement: 16 sigma along x in 10 samples against a diffusive 1 sigma or so
    assert (ref["sums"][10, 0, 3:6].sum() / 864.0 > 0.9 * ref["sums"][10, 0, 0:3].sum())
    want = mr.drift_free(ref["sums"], ref["origins"], ref["sizes"])
    count = ref["origins"][:, None] * 864.0
    tol = (bound[..., 0:3].sum(axis=2) + bound[..., 3:6].sum(axis=2) / 864.0) / count
    tol += 8 * 2.0 ** -53 * (ref["sums"][..., 0:3].sum(axis=2) + ref["sums"][..., 3:6].sum(axis=2) / 864.0) / count      # (the host's own roundings)
    gap = np.abs(out["msd_drift_free"] - want)
    print("drift-free MSD: largest gap %.3e, bound there %.3e, value %.6e" % (gap.max(), tol.ravel()[gap.argmax()], want.ravel()[gap.argmax()]))
    assert (gap <= tol).all()
    assert 0.0 < want[10, 0] < 0.1 * out["msd"][10, 0, 3]
    md.close()


# ---------------------------------------------------------------- 4. an orthorhombic box with lo != 0; Float32
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_orthorhombic_box_with_an_offset_origin(emdee, dev, dtype):
    E = emdee
    S = ortho._system(E.synthetic, ortho.SMALL, dtype, seed=ortho.SEEDS["single"], lo=True)
    md = ortho._engine(E, S, E.lennard_jones_atoms(S["eps"], S["sigma"]), dev)
    # fp64: two groups, every other atom (those were loaded whole box lengths away).  Float32: the whole box as one group, whose
    # total momentum is zero by construction -- the Float32 bound of the squared drift, 2 |S1| N_g delta, is 2 sqrt(N_g) delta / |d|
    # of the MSD for a group that drifts like a random half of the atoms, and could not stay below the 1e-3 asserted of it
    groups, n_groups = (np.arange(S["N"]) % 2, 2) if dtype == np.float64 else (None, 1)
    md.set_msd_(4, origin_every=2, groups=groups)
    xs, vs = _sampled(md, 7, 20)
    ref = mr.correlate(xs, vs, 4, 2, groups, n_groups)
    x_max = None if dtype == np.float64 else max(np.abs(x).max() for x in xs)
    assert max(np.abs(x).max() for x in xs) > 2.0 * S["lengths"].max()
    _check(md.msd(), ref, "orthorhombic, %s" % np.dtype(dtype).name, x_max)
    md.close()


def test_float32_fluid_is_within_the_rounding_of_state(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev, np.float32)
    md.set_msd_(6, origin_every=2)
    xs, vs = _sampled(md, 13, 5)
    ref = mr.correlate(xs, vs, 6, 2)
    _check(md.msd(), ref, "fluid, Float32", max(np.abs(x).max() for x in xs))
    md.close()


# ---------------------------------------------------------------- 5. rigid water under v-rescale
def test_rigid_water_under_vrescale_by_species(emdee, dev):
    E = emdee
    B = sr.water_box()
    n = len(B["mass"])
    groups = (np.arange(n) % 3 != 0).astype(np.int64)       # group 0: O, group 1: H
    md = _water_engine(E, dev, B)
    md.set_thermostat_(E.THERMOSTAT_VRESCALE, 1.0, 0.1, every=2, seed=3)
    md.set_msd_(4, origin_every=2, groups=groups)
    xs, vs = _sampled(md, 6, 5, sr.DT)
    ref = mr.correlate(xs, vs, 4, 2, groups, 2)
    assert list(ref["sizes"]) == [n // 3, 2 * n // 3]
    out = md.msd()
    _check(out, ref, "water")
    assert (out["msd"][1:, 1, 3] > out["msd"][1:, 0, 3]).all()             # the hydrogens turn about the oxygens as well
    md.close()


# ---------------------------------------------------------------- 6. sampling leaves the run alone
def _bits(md):
    st = md.state()
    return [st[k].cpu().numpy().tobytes() for k in ("positions", "velocities", "forces")]


def test_sampling_does_not_change_the_run(emdee, dev):
    E = emdee
    S, a = _fluid(E, dev)
    _, b = _fluid(E, dev)
    b.set_msd_(6, origin_every=2)
    b.msd_sample_()
    for _ in range(12):
        a.step_(5, DT)
        b.step_(5, DT)
        b.msd_sample_()
    assert _bits(a) == _bits(b) and a.nbr_stats() == b.nbr_stats()
    assert b.msd()["samples"] == 13
    a.close()
    b.close()


# ---------------------------------------------------------------- 7. reproducibility, reading twice, reset
def test_sums_are_bitwise_reproducible_and_reset_starts_again(emdee, dev):
    E = emdee
    runs = []
    for _ in range(2):
        S, md = _fluid(E, dev)
        groups = np.arange(864) % 3 - 1                     # a third left out, two groups
        md.set_msd_(5, origin_every=2, groups=groups)
        for k in range(7):
            md.msd_sample_()
            md.step_(5, DT)
        first, again = md.msd(), md.msd()
        assert first["sums"].tobytes() == again["sums"].tobytes() and np.array_equal(first["origins"], again["origins"])
        assert first["samples"] == 7 and (first["sums"][1:, :, 0:3] > 0).all()
        runs.append(first)
        md.msd_reset_()
        zero = md.msd()
        assert (zero["sums"] == 0.0).all() and zero["samples"] == 0 and (zero["origins"] == 0).all()
        assert np.isnan(zero["msd"]).all() and np.isnan(zero["vacf"]).all() and np.isnan(zero["msd_drift_free"]).all()
        x, v = _frame(md)
        md.msd_sample_()                                     # an origin again: lag 0, sum v . v
        one = md.msd()
        assert list(one["origins"]) == [1, 0, 0, 0, 0] and one["samples"] == 1
        ref = mr.correlate([x], [v], 5, 2, groups, 2)
        assert (np.abs(one["sums"] - ref["sums"]) <= mr.bound64(ref)).all() and (one["sums"][0, :, 6] > 0).all()
        runs.append(one)
        md.close()
    assert runs[0]["sums"].tobytes() == runs[2]["sums"].tobytes() and runs[1]["sums"].tobytes() == runs[3]["sums"].tobytes()


# ---------------------------------------------------------------- 8. masks
def test_masks_keep_the_other_words_at_exactly_zero(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    md.set_msd_(3, vacf=False)
    xs, vs = _sampled(md, 4, 5)
    out = md.msd()
    assert (out["sums"][..., 6] == 0.0).all() and (out["sums"][1:, :, 0:3] > 0).all()
    _check(out, mr.correlate(xs, vs, 3, 1, vacf=False), "MSD only")
    md.set_msd_(3, msd=False)
    xs, vs = _sampled(md, 4, 5)
    out = md.msd()
    assert (out["sums"][..., 0:6] == 0.0).all()
    ref = mr.correlate(xs, vs, 3, 1, msd=False)
    _check(out, ref, "VACF only")
    vv = sum((v * v).sum() for v in vs)
    assert abs(out["sums"][0, 0, 6] - vv) <= mr.bound64(ref)[0, 0, 6]
    md.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_table_and_the_sums_in_force(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    for call in (md.msd_sample_, md.msd_reset_):
        assert "no table" in _refused(E, ERR_STATE, call)
    assert "no table" in _refused(E, ERR_STATE, E._lib.call, "emdee_md_msd_read", md._handle, None, None, None, None)
    md.set_msd_(4, origin_every=2)
    md.msd_sample_()
    md.step_(5, DT)
    md.msd_sample_()
    before = md.msd()
    g2 = np.arange(864) % 2

    def intact():
        now = md.msd()
        return now["sums"].tobytes() == before["sums"].tobytes() and now["samples"] == 2 and np.array_equal(now["origins"], before["origins"])

    def raw(what, n_groups, groups, n_lags, every):
        t = None if groups is None else torch.as_tensor(groups).to(device=dev, dtype=torch.int32).contiguous()
        E._lib.call("emdee_md_set_msd", md._handle, what, n_groups, None if t is None else C.c_void_p(t.data_ptr()), n_lags, every)

    assert "EMDEE_MSD | EMDEE_VACF" in _refused(E, ERR_INVALID, raw, 0, 1, None, 4, 1)
    assert "EMDEE_MSD | EMDEE_VACF" in _refused(E, ERR_INVALID, raw, 4, 1, None, 4, 1)
    assert "n_groups = 0" in _refused(E, ERR_INVALID, raw, 3, 0, None, 4, 1)
    assert "n_groups = 9" in _refused(E, ERR_INVALID, raw, 3, 9, np.arange(864) % 9, 4, 1)
    bad = g2.copy()
    bad[123] = 2
    assert "atom 123" in _refused(E, ERR_INVALID, raw, 3, 2, bad, 4, 1)
    bad[123], bad[7] = 0, -2
    assert "atom 7" in _refused(E, ERR_INVALID, raw, 3, 2, bad, 4, 1)
    assert "groups is NULL" in _refused(E, ERR_INVALID, raw, 3, 2, None, 4, 1)
    assert "n_lags = -1" in _refused(E, ERR_INVALID, raw, 3, 1, None, -1, 1)
    assert "n_lags = 4097" in _refused(E, ERR_INVALID, raw, 3, 1, None, 4097, 64)
    assert "origin_every = 0" in _refused(E, ERR_INVALID, raw, 3, 1, None, 4, 0)
    assert "65 origins" in _refused(E, ERR_INVALID, raw, 3, 1, None, 65, 1)
    assert intact()
    # a rescaled box: refused until a reset
    md.scale_box_(0.999)
    assert "emdee_md_msd_reset" in _refused(E, ERR_STATE, md.msd_sample_) and intact()
    md.msd_reset_()
    md.msd_sample_()
    assert md.msd()["samples"] == 1
    # a new state of the same size: refused until a reset
    md.set_state_(E.cu(S["pos"], dev), E.cu(S["vel"], dev), E.cu(S["atoms"], dev))
    after = md.msd()
    assert "emdee_md_set_state" in _refused(E, ERR_STATE, md.msd_sample_)
    assert md.msd()["sums"].tobytes() == after["sums"].tobytes() and md.msd()["samples"] == 1
    md.msd_reset_()
    md.msd_sample_()
    assert list(md.msd()["origins"]) == [1, 0, 0, 0]
    # another atom count: refused until the table is set again
    md.set_state_(E.cu(S["pos"][:-3], dev), E.cu(S["vel"][:-3], dev), E.cu(S["atoms"][:-3], dev))
    assert "861" in _refused(E, ERR_STATE, md.msd_sample_)
    md.msd_reset_()
    assert "861" in _refused(E, ERR_STATE, md.msd_sample_)
    md.set_msd_(4, origin_every=2)
    md.msd_sample_()
    assert md.msd()["group_sizes"] == [861]
    md.set_msd_(0)                                           # cleared
    assert "no table" in _refused(E, ERR_STATE, md.msd_sample_)
    md.close()


def test_lent_unloaded_and_ghost_engines_refuse_a_table(emdee, dev):
    E = emdee
    S = bref.fluid864(E.synthetic)
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (a decomposition needs two bricks of 2.8 + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    assert "lent" in _refused(E, ERR_STATE, dd.engine(0).set_msd_, 4)
    dd.step_(2, DT)                                                                      # the decomposition is unharmed
    dd.close()
    model = E.LennardJonesModel(bref.RC, bref.RS)
    g = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"][:-4], dev), S["L"], model, E.cu(S["atoms"], dev), skin=bref.SKIN, n_ghost=4)
    assert "ghosts" in _refused(E, ERR_STATE, g.set_msd_, 4)
    g.close()
    # before emdee_md_set_state, through the C ABI
    ctx = E.context_for(dev)
    h = C.c_void_p()
    three = lambda *v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", ctx.handle, three(0, 0, 0), three(S["L"], S["L"], S["L"]), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(model), bref.SKIN, 8, C.byref(h))
    assert "no state loaded" in _refused(E, ERR_STATE, E._lib.call, "emdee_md_set_msd", h, 3, 1, None, 4, 1)
    E._lib.call("emdee_md_destroy", h)
    # an open axis is fine: its image count is 0
    o = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"], dev), S["L"], model, E.cu(S["atoms"], dev), skin=bref.SKIN,
                         lo=[-3.0] * 3, lengths=[S["L"] + 6.0] * 3, periodic=[1, 1, 0])
    o.set_msd_(2)
    xs, vs = _sampled(o, 3, 5)
    _check(o.msd(), mr.correlate(xs, vs, 2, 1), "open z")
    o.close()


# ---------------------------------------------------------------- 10. the timer
def test_kernel_time_counts_three_launches_a_sample(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    md.set_msd_(4, origin_every=2)
    assert md.kernel_time("msd") == (0.0, 0)
    md.profile_(True)
    for _ in range(5):
        md.msd_sample_()
        md.step_(2, DT)
    ms, launches = md.kernel_time("msd")
    assert launches == 15 and ms > 0.0 and md.kernel_time(16) == (ms, launches)
    md.profile_(False)
    md.close()


# ---------------------------------------------------------------- 11. the example
def test_example_prints_two_positive_diffusion_coefficients(emdee):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lj_diffusion.py"), "--cells", "6", "--melt", "300", "--steps", "600"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = {line.split("=")[0].strip(): float(line.split("=")[1]) for line in r.stdout.splitlines() if line.startswith("D ")}
    print(r.stdout.splitlines()[0], d)
    assert set(d) == {"D Einstein", "D Green-Kubo"}
    assert all(np.isfinite(v) and v > 0.0 for v in d.values())
