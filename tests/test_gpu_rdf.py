"""GPU tests of the radial distribution functions (include/emdee_hip.h: emdee_md_set_rdf; csrc/rdf.hpp).  The reference is always
tests/helpers/rdf_ref.py, a numpy brute force over all pairs, on the positions md.state() returns.

fp64 engines must give the reference's counts exactly.  The reference also counts the pairs within delta = 1e-10 r_max of a bin edge
-- the only pairs whose bin the last places of a position could change -- and every exact case first asserts that it finds none:
the boxes, seeds and bin widths below were chosen on the CPU for that.  (The one exception is named where it is made: the two
coincident atoms of the orthorhombic case sit on edge 0 by construction, and a pair at r = 0 has no bin below to fall into; the
case asserts that edge 0 holds exactly that pair.)  Float32 engines histogram their records in fp64 while
state() returns them rounded to fp32, so there delta = 4 sqrt(3) 2^-24 max(|lo| + len), two atoms' rounding of state(), and with e_k
the reference's pairs within delta of edge k: |dev - ref| <= e_b + e_(b+1) per bin, the totals differ by at most e_(n_bins), and
the sum of e is asserted to be at most 1e-3 of the pairs counted."""
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import barostat_ref as bref
from .helpers import rdf_ref as rr
from .helpers import settle_ref as sr
from .test_gpu_barostat import DT, PATHS, _engine, _fluid, _path
from .test_gpu_dd_pairs import _build
from .test_gpu_settle import _engine as _water_engine
from .test_gpu_settle import _refused

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
# steps of the fluid under rebuild_every = 1000 after which some atom is more than SKIN from where it was loaded: the numpy
# integrator (ortho_ref.verlet on barostat_ref.fluid864) has 81 atoms beyond 0.3, the farthest at 0.46, after 40 steps
STALE_STEPS = 40


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _positions(md):
    return md.state(velocities=False, forces=False)["positions"].cpu().numpy().astype(np.float64)


def _reference(md, lengths, r_max, n_bins, delta, **kw):
    return rr.histogram(_positions(md), lengths, r_max, n_bins, delta=delta, **kw)


def _exact(md, lengths, r_max, n_bins, what, coincident=0, **kw):
    """one sample of a fresh table against the reference: no edge pairs, equal counts.  coincident: the pairs of atoms the case
    put at one point on purpose; they sit on edge 0, r = 0, which has no bin below it to fall into, and nothing else may"""
    want, edge = _reference(md, lengths, r_max, n_bins, 1e-10 * r_max, **kw)
    assert edge[0] == coincident and edge[1:].sum() == 0, (what, edge.nonzero())
    md.rdf_sample_()
    out = md.rdf()
    print("%s: %d pairs in %d histograms, %d differ" % (what, want.sum(), len(want), (out["counts"] != want).sum()))
    assert out["counts"].dtype == np.int64 and np.array_equal(out["counts"], want), what
    assert out["frames"] == 1
    return out, want


def _within_rounding(md, lengths, lo, r_max, n_bins, what, **kw):
    """a Float32 engine: the bounds of the module docstring"""
    lengths = np.asarray(lengths, dtype=np.float64)
    delta = 4.0 * np.sqrt(3.0) * 2.0 ** -24 * float(np.max(np.abs(lo) + lengths))
    want, edge = _reference(md, lengths, r_max, n_bins, delta, **kw)
    assert edge.sum() <= 1e-3 * want.sum(), (what, edge.sum(), want.sum())
    md.rdf_sample_()
    got = md.rdf()["counts"]
    assert got.shape == want.shape == (1, n_bins)                          # (one histogram: the edge pairs are its own)
    gap = np.abs(got[0] - want[0])
    print("%s: %d pairs, %d edge pairs (delta %.2e), %d bins differ by %d at the most, totals %d and %d"
          % (what, want.sum(), edge.sum(), delta, (gap > 0).sum(), gap.max(), got.sum(), want.sum()))
    assert (gap <= edge[:-1] + edge[1:]).all(), what
    assert abs(int(got.sum()) - int(want.sum())) <= edge[-1], what


# ---------------------------------------------------------------- exactness
@pytest.mark.parametrize("path", PATHS)
def test_fluid_counts_are_exact_up_to_half_the_box(emdee, dev, monkeypatch, path):
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    L = S["L"]
    md.set_rdf_(0.5 * L, 100)
    out, want = _exact(md, [L] * 3, 0.5 * L, 100, "fluid, " + path)
    assert out["pairs"] == [(0, 0)] and out["group_sizes"] == [864] and want.sum() > 150000
    assert out["inv_volume_sum"] == 1.0 / (L * L * L)
    md.close()


@pytest.mark.parametrize("path", PATHS)
def test_fluid_counts_are_exact_where_no_axis_of_the_grid_wraps(emdee, dev, monkeypatch, path):
    """r_max = 1.5: the sample's grid is 6 x 6 x 6 cells with nd = 1 (tests/test_rdf_host.py pins the plan), so the kernel takes a
    row along x as the run cx - 1 ... cx + 1 in the interior and as two runs at either box face -- the path of every large box"""
    E = emdee
    _path(monkeypatch, path)
    S, md = _fluid(E, dev)
    L, r_max = S["L"], rr.NOWRAP_FLUID_R_MAX
    md.step_(10, DT)
    md.set_rdf_(r_max, 30)
    out, want = _exact(md, [L] * 3, r_max, 30, "fluid up to 1.5, " + path)
    assert want.sum() > 3000
    groups, molecules = _three_groups(864)
    md.set_rdf_(r_max, 30, groups, molecules, n_groups=3)
    _exact(md, [L] * 3, r_max, 30, "fluid up to 1.5, three groups, " + path, groups=groups, molecules=molecules, n_groups=3)
    md.close()


def test_counts_are_exact_where_x_does_not_wrap_at_two_cells_per_r_max(emdee, dev):
    """864 atoms in 12.6 x 10.1 x 10.1 up to r_max = 5: the grid is 5 x 4 x 4 cells with nd = 2 (pinned in tests/test_rdf_host.py):
    y and z wrap, x does not, and with five cells every home cell's row along x passes a box face or touches it"""
    E = emdee
    pos = rr.nowrap_box()
    atoms = bref.lj_atoms(rr.NOWRAP_N)
    atoms["twice_sqrt_eps"] = 0.0                                          # (no forces: any placement loads)
    md = _engine(E, dev, pos, np.zeros_like(pos), np.array(rr.NOWRAP_LENGTHS), atoms)
    md.set_rdf_(rr.NOWRAP_R_MAX, 50)
    out, want = _exact(md, rr.NOWRAP_LENGTHS, rr.NOWRAP_R_MAX, 50, "x unwrapped at nd = 2")
    assert want.sum() > 100000
    md.close()


def _three_groups(n):
    groups = np.zeros(n, dtype=np.int64)
    groups[::7] = -1                                                       # left out
    groups[5] = 2                                                          # a group of one; group 1 stays empty
    return groups, np.arange(n) // 3


def test_three_groups_an_empty_one_a_single_atom_and_molecules(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    L = S["L"]
    groups, molecules = _three_groups(864)
    md.set_rdf_(0.5 * L, 100, groups, molecules, n_groups=3)
    out, want = _exact(md, [L] * 3, 0.5 * L, 100, "three groups", groups=groups, molecules=molecules, n_groups=3)
    assert out["pairs"] == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert out["group_sizes"] == [int((groups == 0).sum()), 0, 1]
    counts = out["counts"]
    for a, b in ((0, 1), (1, 1), (1, 2), (2, 2)):
        assert counts[rr.pair_slot(a, b, 3)].sum() == 0                     # the empty group, and a single atom with itself
    assert counts[rr.pair_slot(0, 0, 3)].sum() > 100000 and counts[rr.pair_slot(0, 2, 3)].sum() > 100
    # the molecules took pairs out: without them the same groups count more
    md.set_rdf_(0.5 * L, 100, groups, None, n_groups=3)
    more, _ = _exact(md, [L] * 3, 0.5 * L, 100, "three groups, no molecules", groups=groups, n_groups=3)
    assert more["counts"].sum() > counts.sum()
    md.close()


# an orthorhombic box with lo != 0; r_max is half its shortest side.  |x| of an atom loaded up to three box lengths out along x or
# y (one along z) stays below 2 max(|lo| + len) = 32, which is what the Float32 delta allows a rounded coordinate
ORTHO_LO, ORTHO_LEN = np.array([0.5, -1.0, 2.0]), np.array([5.7, 7.0, 14.0])


def _ortho_case(E, dtype):
    rng = np.random.default_rng(20261)
    n = 500
    pos = ORTHO_LO + rng.uniform(0.0, 1.0, (n, 3)) * ORTHO_LEN
    pos[17] = pos[3]                                                       # two coincident atoms: r = 0, bin 0
    far = rng.choice(np.arange(20, n), 60, replace=False)
    pos[far] += rng.integers(-3, 4, (60, 3)) * np.array([1, 1, 0]) * ORTHO_LEN + rng.integers(-1, 2, (60, 3)) * np.array([0, 0, 1]) * ORTHO_LEN
    atoms = bref.lj_atoms(n)
    atoms["twice_sqrt_eps"] = 0.0                                          # (no forces: any placement loads)
    if dtype == np.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    return pos, atoms


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_orthorhombic_box_with_coincident_atoms_and_far_images(emdee, dev, dtype):
    E = emdee
    pos, atoms = _ortho_case(E, dtype)
    md = _engine(E, dev, pos, np.zeros_like(pos), ORTHO_LEN, atoms, dtype, lo=ORTHO_LO)
    r_max = 0.5 * float(ORTHO_LEN.min())
    assert np.abs(pos - ORTHO_LO - 0.5 * ORTHO_LEN).max() > 2.5 * ORTHO_LEN.min()
    md.set_rdf_(r_max, 60)
    if dtype == np.float64:
        out, want = _exact(md, ORTHO_LEN, r_max, 60, "orthorhombic", coincident=1)
        assert out["counts"][0, 0] >= 1 and want.sum() > 15000
    else:
        _within_rounding(md, ORTHO_LEN, ORTHO_LO, r_max, 60, "orthorhombic, Float32")
    md.close()


def test_fewer_atoms_than_a_wavefront_in_a_box_the_stencil_wraps_around(emdee, dev):
    E = emdee
    r_max = 2.85                                                           # (the engine's own minimum image needs 2 (rc + skin) = 5.6)
    lengths = np.array([2.0, 2.1, 2.2]) * r_max
    rng = np.random.default_rng(37)
    pos = rng.uniform(0.0, 1.0, (37, 3)) * lengths
    atoms = bref.lj_atoms(37)
    atoms["twice_sqrt_eps"] = 0.0
    md = _engine(E, dev, pos, np.zeros_like(pos), lengths, atoms)
    md.set_rdf_(r_max, 50)
    out, want = _exact(md, lengths, r_max, 50, "37 atoms")
    assert 100 < want.sum() < 37 * 36 // 2
    md.close()


def test_sample_is_exact_under_a_stale_list(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    L = S["L"]
    md.step_(STALE_STEPS, DT, rebuild_every=1000)
    moved = _positions(md) - S["pos"]
    moved -= L * np.rint(moved / L)
    far = np.sqrt((moved * moved).sum(axis=1))
    print("after %d steps without a rebuild: %d atoms beyond the skin, the farthest %.3f" % (STALE_STEPS, (far > bref.SKIN).sum(), far.max()))
    assert far.max() > bref.SKIN
    builds = md.nbr_stats()["builds"]
    md.set_rdf_(0.5 * L, 100)
    _exact(md, [L] * 3, 0.5 * L, 100, "stale list")
    assert md.nbr_stats()["builds"] == builds
    md.close()


def test_float32_fluid_counts_are_within_the_rounding_of_the_positions(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev, np.float32)
    L = S["L"]
    md.step_(10, DT)                                                       # (records that have left their cells' origins)
    md.set_rdf_(0.5 * L, 100)
    _within_rounding(md, [L] * 3, np.zeros(3), 0.5 * L, 100, "fluid, Float32")
    md.close()


# ---------------------------------------------------------------- sampling leaves the run alone
def _bits(md):
    st = md.state()
    return [st[k].cpu().numpy().tobytes() for k in ("positions", "velocities", "forces")]


def test_sampling_does_not_change_the_fused_loop(emdee, dev):
    E = emdee
    S, a = _fluid(E, dev)
    _, b = _fluid(E, dev)
    L = S["L"]
    b.set_rdf_(0.5 * L, 100)
    for _ in range(4):
        a.step_(10, DT)
        b.step_(10, DT)
        b.rdf_sample_()
    assert _bits(a) == _bits(b) and a.nbr_stats() == b.nbr_stats()
    assert b.rdf()["frames"] == 4
    a.close()
    b.close()


def test_sampling_does_not_change_rigid_water_under_vrescale_and_sums_the_frames(emdee, dev):
    E = emdee
    B = sr.water_box()
    n = len(B["mass"])
    groups, molecules = np.arange(n) % 3 != 0, np.arange(n) // 3            # group 0: O, group 1: H
    r_max, n_bins = 0.5 * float(sr.LENGTHS.min()), 70                     # bins of 0.05
    engines = []
    for _ in range(2):
        md = _water_engine(E, dev, B)
        md.set_thermostat_(E.THERMOSTAT_VRESCALE, 1.0, 0.1, every=2, seed=3)
        engines.append(md)
    a, b = engines
    b.set_rdf_(r_max, n_bins, groups.astype(np.int64), molecules)
    want = np.zeros((3, n_bins), dtype=np.int64)
    for _ in range(4):
        a.step_(10, sr.DT)
        b.step_(10, sr.DT)
        frame, edge = _reference(b, sr.LENGTHS, r_max, n_bins, 1e-10 * r_max, groups=groups.astype(np.int64), molecules=molecules)
        assert edge.sum() == 0
        want += frame
        b.rdf_sample_()
    assert _bits(a) == _bits(b) and a.nbr_stats() == b.nbr_stats()
    out = b.rdf()
    assert out["frames"] == 4 and out["group_sizes"] == [n // 3, 2 * n // 3] and np.array_equal(out["counts"], want)
    # no intramolecular pair.  In this box's reduced units the O-H bond is 0.32 (bin 6) -- the 0.1 nm of water, so that "below
    # 0.12 nm" is below 0.384 here: the bins up to 0.40.  The last frame counted with the bonds has every one of the 300 bonds in
    # that range, all in bin 6; the four frames of the engine have nothing there at all (O and H of different molecules stay
    # beyond sigma_OH = 0.7), neither in the counts nor in g
    oh = rr.pair_slot(0, 1, 2)
    low = out["edges"][1:] <= 0.40 + 1e-12
    assert low.sum() == 8 and low[6]
    with_bonds, _ = _reference(b, sr.LENGTHS, r_max, n_bins, 0.0, groups=groups.astype(np.int64))
    assert with_bonds[oh][low].sum() == with_bonds[oh][6] == 2 * n // 3
    assert out["counts"][oh][low].sum() == 0 and (out["g"][oh][low] == 0.0).all()
    a.close()
    b.close()


# ---------------------------------------------------------------- accumulation and reproducibility
def test_accumulation_reset_reproducibility_and_normalisation(emdee, dev):
    E = emdee
    runs = []
    for _ in range(2):
        S, md = _fluid(E, dev)
        L = S["L"]
        groups = (np.arange(864) % 4 == 0).astype(np.int64)
        md.set_rdf_(0.5 * L, 64, groups)
        assert md.kernel_time("rdf") == (0.0, 0)
        first = None
        md.profile_(True)
        for k in range(3):
            md.rdf_sample_()
            if first is None:
                first = md.rdf()["counts"].copy()
            md.step_(5, DT)
        ms, launches = md.kernel_time("rdf")
        assert launches > 0 and launches % 3 == 0 and ms > 0.0 and md.kernel_time(15) == (ms, launches)
        md.profile_(False)
        out = md.rdf()
        runs.append(out)
        assert out["frames"] == 3 and out["inv_volume_sum"] == pytest.approx(3.0 / L ** 3, rel=1e-15)
        assert (out["counts"] >= first).all() and out["counts"].sum() > 2 * first.sum()
        g, cn = rr.normalise(out["counts"], 2, 0.5 * L, out["group_sizes"], out["frames"], out["inv_volume_sum"])
        assert np.allclose(out["g"], g, rtol=1e-13, atol=0.0) and np.allclose(out["coordination"], cn, rtol=1e-13, atol=0.0)
        assert np.allclose(out["edges"], 0.5 * L * np.arange(65) / 64, rtol=1e-15) and np.allclose(out["r"], 0.5 * (out["edges"][1:] + out["edges"][:-1]))
        # a liquid beyond three sigma: g swings by less than 0.15 about 1, and 1.9 sigma of bins hold two of its periods
        assert abs(out["g"][0][40:].mean() - 1.0) < 0.1
        md.rdf_reset_()
        zero = md.rdf()
        assert zero["counts"].sum() == 0 and zero["frames"] == 0 and zero["inv_volume_sum"] == 0.0 and (zero["g"] == 0.0).all()
        md.rdf_sample_()
        again = md.rdf()
        assert again["frames"] == 1 and again["counts"].sum() > 0
        runs.append(again)
        md.close()
    assert np.array_equal(runs[0]["counts"], runs[2]["counts"]) and np.array_equal(runs[1]["counts"], runs[3]["counts"])


def test_inverse_volume_sum_follows_the_box_under_c_rescale(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    md.set_barostat_(E.BAROSTAT_CRESCALE, 1.0, 0.05, 0.5, 5, temperature=1.0, seed=5)      # (an event, with its noise, every 5 steps)
    md.set_rdf_(4.0, 40)
    want, volumes = 0.0, []
    for _ in range(4):
        md.step_(5, DT)
        md.rdf_sample_()
        ln = md.box()[1]
        volumes.append(ln[0] * ln[1] * ln[2])
        want += 1.0 / volumes[-1]
    out = md.rdf()
    assert len(set(volumes)) == 4 and out["frames"] == 4
    assert abs(out["inv_volume_sum"] - want) <= 1e-15 * want
    md.close()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_table_in_force(emdee, dev):
    E = emdee
    S, md = _fluid(E, dev)
    L = S["L"]
    assert "no table" in _refused(E, ERR_STATE, md.rdf_sample_)
    md.set_rdf_(0.5 * L, 100)
    md.rdf_sample_()
    before = md.rdf()["counts"].copy()
    assert "half the shortest" in _refused(E, ERR_INVALID, md.set_rdf_, 0.5 * L * 1.0001, 100)
    assert "counters" in _refused(E, ERR_INVALID, md.set_rdf_, 0.5 * L, 2731, np.arange(864) % 2, n_groups=2)      # 3 x 2731 = 8193
    bad = np.zeros(864, dtype=np.int64)
    bad[123] = 3
    assert "atom 123" in _refused(E, ERR_INVALID, md.set_rdf_, 0.5 * L, 10, bad, n_groups=3)
    assert "n_groups = 9" in _refused(E, ERR_INVALID, md.set_rdf_, 0.5 * L, 10, np.arange(864) % 9)
    low = np.zeros(864, dtype=np.int64)
    low[7] = -2
    assert "atom 7" in _refused(E, ERR_INVALID, md.set_rdf_, 0.5 * L, 10, None, low)
    # the table set before still samples, and exactly
    assert np.array_equal(md.rdf()["counts"], before)
    md.rdf_sample_()
    assert np.array_equal(md.rdf()["counts"], 2 * before)
    # a box shrunk below 2 r_max: refused with the counts as they were, accepted again after a smaller table
    md.scale_box_(0.99)
    assert "shrunk" in _refused(E, ERR_STATE, md.rdf_sample_)
    assert np.array_equal(md.rdf()["counts"], 2 * before) and md.rdf()["frames"] == 2
    md.set_rdf_(0.49 * L, 100)
    _exact(md, [0.99 * L] * 3, 0.49 * L, 100, "after the scale")
    # another atom count
    md.set_state_(E.cu(S["pos"][:-3], dev), E.cu(S["vel"][:-3], dev), E.cu(S["atoms"][:-3], dev))
    assert "861" in _refused(E, ERR_STATE, md.rdf_sample_)
    md.set_rdf_(0.49 * L, 100)
    _exact(md, [0.99 * L] * 3, 0.49 * L, 100, "after the new state")
    md.set_rdf_(1.0, 0)                                                    # cleared
    assert "no table" in _refused(E, ERR_STATE, md.rdf_sample_)
    md.close()


def test_lent_engines_engines_with_ghosts_and_open_boxes_refuse_a_table(emdee, dev):
    E = emdee
    S = bref.fluid864(E.synthetic)
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (a decomposition needs two bricks of 2.8 + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    assert "lent" in _refused(E, ERR_STATE, dd.engine(0).set_rdf_, 2.5, 50)
    dd.step_(2, DT)                                                                      # the decomposition is unharmed
    dd.close()
    model = E.LennardJonesModel(bref.RC, bref.RS)
    g = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"][:-4], dev), S["L"], model, E.cu(S["atoms"], dev), skin=bref.SKIN, n_ghost=4)
    assert "ghosts" in _refused(E, ERR_STATE, g.set_rdf_, 2.5, 50)
    g.close()
    o = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"], dev), S["L"], model, E.cu(S["atoms"], dev), skin=bref.SKIN,
                         lo=[0.0] * 3, lengths=[S["L"]] * 3, periodic=[1, 1, 0])
    assert "open axis" in _refused(E, ERR_STATE, o.set_rdf_, 2.5, 50)
    o.close()


# ---------------------------------------------------------------- the example
def test_example_prints_the_g_of_the_frames_it_sampled(emdee, tmp_path):
    dump = str(tmp_path / "frames.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lj_rdf.py"), "--cells", "6", "--steps", "100", "--dump", dump],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = np.array([[float(t) for t in line.split()] for line in r.stdout.splitlines() if line and line[0].isdigit()])
    d = np.load(dump)
    frames, L, r_max, n_bins = d["frames"], float(d["L"]), float(d["r_max"]), int(d["n_bins"])
    assert len(frames) == 5 and rows.shape == (n_bins, 3)
    counts = sum(rr.histogram(x, [L] * 3, r_max, n_bins)[0] for x in frames)
    g, cn = rr.normalise(counts, 1, r_max, [frames.shape[1]], len(frames), len(frames) / L ** 3)
    # (printed with six decimals)
    assert np.abs(rows[:, 1] - g[0]).max() <= 1e-6 and np.abs(rows[:, 2] - cn[0]).max() <= 1e-6
    assert g[0].max() > 2.0 and (g[0][:int(0.8 / (r_max / n_bins))] == 0.0).all()      # a liquid's first peak, nothing inside the core
