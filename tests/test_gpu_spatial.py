"""GPU tests of the spatial profiles (include/emdee_hip.h: emdee_md_set_spatial).

The reference is always tests/helpers/spatial_ref.py on the engine's own md.state() (positions, velocities, energies) and
md.virial_tensor(), with the caller's masses and charges.  What is left between the two is the order of summation and the few
roundings in forming an addend (the device may contract a product into a sum, the radial normal adds a square root and a division),
so every fp64 word must satisfy |dev - ref| <= 2 (n_k + 16) 2^-53 A_k, n_k the bin's atom count and A_k the sum of the absolute
elementary products behind the word (spatial_ref.bound: gk_ref.bound widened by the addend roundings; derived, not tuned).  fp64
engines bin bit for bit the coordinates state() returns: the counts are the reference's exactly, and each such case first asserts
on the reference alone that no grouped atom lies within 1e-10 bin widths of an edge.  Float32 engines bin unrounded records while
state() returns fp32: with delta = 4 2^-24 max(|lo| + len) and e_k the reference's atoms within delta of edge k, counts may differ
by e_k + e_{k+1} per bin, sum e <= 1e-3 of the grouped atoms; their words are compared on loaded configurations with e = 0 only."""
import ctypes as C

import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import open_cases as oc
from .helpers import settle_ref as sr
from .helpers import shake_ref as hr
from .helpers import spatial_ref as sp
from .test_gpu_barostat import DT, _engine
from .test_gpu_dd_pairs import _build
from .test_gpu_hbonds import _engine as _hbonds_engine
from .test_gpu_open_axes_stages import _slab_engine, _stage_engine
from .test_gpu_orthorhombic import _dress
from .test_gpu_orthorhombic import _engine as _ortho_engine
from .test_gpu_settle import _engine as _water_engine
from .test_gpu_settle import _refused

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
EDGE = 1e-10                                            # bin widths: how far from an edge every grouped atom of an fp64 case stays


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _geom(md, geometry, n_bins, range=None, centre=None):
    lo, ln = md.box()
    if geometry == sp.RADIAL:
        return sp.radial(n_bins, range[1], centre, ln, md_periodic(md))
    if range is None:
        return sp.planar(geometry, n_bins, lo[geometry], ln[geometry])
    return sp.planar(geometry, n_bins, None, range=range)


def md_periodic(md):
    return tuple(md.periodic)


def _reference(md, masses, charges, groups, n_groups, geom, what=7, delta=None):
    """spatial_ref.profile on the engine's own state (read AFTER the sample: the planes the sample read are still current)"""
    stress = bool(what & sp.STRESS)
    st = md.state(forces=False, energies=stress)
    tens = _np(md.virial_tensor()) if stress else None
    en = _np(st["energies"]) if stress else None
    delta = EDGE * geom["width"] if delta is None else delta
    return sp.profile(_np(st["positions"]), _np(st["velocities"]), masses, charges, en, tens, groups, n_groups, geom, what=what, delta=delta)


def _add(a, b):
    return {k: (a[k] + b[k] if k in ("counts", "words", "outside", "absum", "near") else b[k]) for k in b}


def _check(out, ref, what, exact=True, words=True):
    """counts, outside and the ten words of md.spatial() against the (accumulated) reference; returns the largest ratio to the bound"""
    counts, sums = out["counts"], out["sums"]
    if exact:
        assert ref["near"].sum() == 0, ("a grouped atom within the edge band", what, ref["near"].nonzero())
        assert np.array_equal(counts, ref["counts"]), what
        assert out["outside"] == ref["outside"].tolist(), what
    else:
        e = ref["near"]
        assert e.sum() <= 1e-3 * (ref["counts"].sum() + ref["outside"].sum()) + 0.5, (what, e.sum())
        # (with one group: an atom within delta of an edge may sit on either side of it)
        assert (np.abs(counts - ref["counts"]).sum(axis=0) <= e[:-1] + e[1:]).all(), what
    if not words:
        return 0.0
    bound = sp.bound(ref["counts"], ref["absum"])
    err = np.abs(sums - ref["words"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("%s: largest |dev - ref| / bound = %.3f" % (what, ratio.max()))
    assert (err <= bound).all(), (what, np.argwhere(err > bound)[:5], ratio.max())
    return float(ratio.max())


# ---------------------------------------------------------------- 1. the 864-atom fluid, axis z
def _fluid_groups(n):
    g = np.arange(n) % 3 - 1                                # -1, 0, 1: two groups and ungrouped atoms
    return g


def _fluid_engine(E, dev, dtype):
    S = bref.fluid864(E.synthetic)
    pos, vel = S["pos"], S["vel"]
    if dtype == np.float32:
        pos, vel = pos.astype(np.float32).astype(np.float64), vel.astype(np.float32).astype(np.float64)
    n = pos.shape[0]
    inv_mass = np.where(np.arange(n) % 2 == 0, 1.0, 0.25)   # masses 1 and 4, exact in both precisions
    md = _engine(E, dev, pos, vel, S["L"], S["atoms"], dtype, inv_mass=inv_mass)
    return S, md, 1.0 / inv_mass


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_bins", [7, 64])
def test_fluid_profiles_along_z_match_the_reference(emdee, dev, dtype, n_bins):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, dtype)
    groups = _fluid_groups(len(masses))
    f64 = dtype == np.float64
    delta = None if f64 else 4.0 * 2.0 ** -24 * S["L"]
    md.set_spatial_("z", n_bins, groups=groups, n_groups=2)
    md.spatial_sample_()
    geom = _geom(md, sp.Z, n_bins)
    ref = _reference(md, masses, None, groups, 2, geom, delta=delta)
    if not f64:
        assert ref["near"].sum() == 0                       # the loaded configuration: e = 0, the words are compared
    out = md.spatial()
    _check(out, ref, "fluid %s %d bins, at the load" % (dtype.__name__, n_bins), exact=True)
    assert out["frames"] == 1 and out["group_sizes"] == [288, 288]
    v_bin = S["L"] ** 3 / n_bins
    assert out["inv_bin_volume_sum"] == 1.0 / (S["L"] * S["L"] * (S["L"] / n_bins))
    assert abs(out["bin_volume"][0] - v_bin) <= 1e-14 * v_bin
    # a few steps later, with a rebuild of the list in between: the second frame adds to the first
    md.step_(5, DT)
    md.rebuild_()
    md.spatial_sample_()
    ref2 = _add(ref, _reference(md, masses, None, groups, 2, geom, delta=delta))
    out = md.spatial()
    _check(out, ref2, "fluid %s %d bins, two frames" % (dtype.__name__, n_bins), exact=f64, words=f64)
    assert out["frames"] == 2 and out["inv_bin_volume_sum"] == 2.0 * (1.0 / (S["L"] * S["L"] * (S["L"] / n_bins)))
    assert out["counts"].sum() == 2 * 576 and out["outside"] == [0, 0]


@pytest.mark.parametrize("what", [sp.DENSITY, sp.KINETIC, sp.STRESS])
def test_a_single_bit_leaves_the_other_words_exactly_zero(emdee, dev, what):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    groups = _fluid_groups(len(masses))
    md.set_spatial_("z", 7, groups=groups, n_groups=2, density=bool(what & 1), kinetic=bool(what & 2), stress=bool(what & 4))
    md.spatial_sample_()
    ref = _reference(md, masses, None, groups, 2, _geom(md, sp.Z, 7), what=what)
    out = md.spatial()
    _check(out, ref, "mask %d" % what)
    mine = {1: [0, 1], 2: [2, 3, 4, 5, 6], 4: [7, 8, 9]}[what]
    others = [w for w in range(10) if w not in mine]
    assert (out["sums"][..., others] == 0.0).all() and not np.signbit(out["sums"][..., others]).any()
    first, last = mine[0], (mine[-1] if what != sp.DENSITY else mine[0])     # (no charges here: word 1 is 0 as well)
    assert np.abs(out["sums"][..., first]).sum() > 0.0 and np.abs(out["sums"][..., last]).sum() > 0.0


# ---------------------------------------------------------------- 2. chunk seams
def _fcc7(E, dev):
    pos, L = E.synthetic.fcc_positions(7)
    rng = np.random.default_rng(71)
    pos = np.mod(pos + rng.uniform(-0.08, 0.08, pos.shape), L)
    vel = E.synthetic.velocities(pos.shape[0], temperature=1.0)
    return pos, L, _engine(E, dev, pos, vel, L, bref.lj_atoms(pos.shape[0]))


@pytest.mark.parametrize("n_bins", [1, 4096])
@pytest.mark.parametrize("eight", [False, True])
def test_chunk_seams_one_and_eight_groups(emdee, dev, n_bins, eight):
    E = emdee
    pos, L, md = _fcc7(E, dev)
    n = pos.shape[0]
    assert n == 1372                                        # two chunks, the second part-filled
    if eight:
        groups = np.arange(n) % 6                           # groups 0 ... 5 dealt round; 6 stays empty; 7 holds one atom
        groups[1000] = 7
        n_groups = 8
    else:
        groups, n_groups = None, 1
    md.set_spatial_("x", n_bins, groups=groups, n_groups=n_groups)
    md.spatial_sample_()
    ref = _reference(md, np.ones(n), None, groups, n_groups, _geom(md, sp.X, n_bins))
    out = md.spatial()
    _check(out, ref, "seams %d bins, %d groups" % (n_bins, n_groups))
    if eight:
        assert out["group_sizes"][6:] == [0, 1] and out["counts"][6].sum() == 0 and out["counts"][7].sum() == 1
    assert out["counts"].sum() == n


# ---------------------------------------------------------------- 3. the identity with the box sums
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_bins_add_up_to_the_box_sums(emdee, dev, axis):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    n = len(masses)
    md.set_spatial_("xyz"[axis], 7)
    md.spatial_sample_()
    ref = _reference(md, masses, None, None, 1, _geom(md, axis, 7))
    out = md.spatial()
    _check(out, ref, "identity, axis %d" % axis)
    total = out["sums"].sum(axis=(0, 1))
    bound = 2.0 * (n + 16.0) * 2.0 ** -53 * ref["absum"].sum(axis=(0, 1))
    pt = md.pressure_tensor()
    potential, kinetic, _ = md.totals()
    want = {0: masses.sum(), 5: np.trace(pt["kinetic"]), 6: pt["kinetic"][axis, axis], 7: potential, 8: np.trace(pt["virial"]),
            9: pt["virial"][axis, axis]}
    for w, value in want.items():
        assert abs(total[w] - value) <= bound[w] + 4.0 * 2.0 ** -53 * abs(value), (w, total[w], value, bound[w])
    assert abs(0.5 * total[5] - kinetic) <= bound[5]


# ---------------------------------------------------------------- 4. charged and bonded engines; 5. open axes
def test_a_charged_water_slab_along_its_open_and_a_periodic_axis(emdee, dev):
    """open_cases.stage_box("water", "slab") without constraints, with charges and exclusions: word 1 is not zero; along the open
    axis the range is narrower than the atoms' extent and two atoms are placed beyond the faces"""
    E = emdee
    B = oc.stage_box("water", "slab")
    pos = np.array(B["pos"], dtype=np.float64)
    lo, ln = np.array(B["lo"]), np.array(B["lengths"])
    assert tuple(B["periodic"]) == (1, 1, 0)
    zs = np.argsort(pos[:, 2])
    pos[zs[0], 2], pos[zs[-1], 2] = lo[2] - 0.37, lo[2] + ln[2] + 0.41      # beyond both faces of the open axis
    md = _stage_engine(E, dev, B, rigid=False, charged=True, pos=pos)
    masses, charges = 1.0 / np.asarray(B["inv_mass"]), np.asarray(B["charges"], dtype=np.float64)
    n = len(masses)
    groups = (np.arange(n) % 3 == 0).astype(int)            # the apexes and the others
    z = np.sort(pos[:, 2])
    rng_z = (float(z[n // 10]) + 0.0123, float(z[-n // 10]) - 0.0321)          # narrower than the atoms' extent
    md.set_spatial_("z", 11, groups=groups, n_groups=2, range=rng_z)
    md.spatial_sample_()
    ref = _reference(md, masses, charges, groups, 2, _geom(md, sp.Z, 11, range=rng_z))
    out = md.spatial()
    _check(out, ref, "water slab, open axis")
    assert sum(out["outside"]) >= n // 5 and sum(out["outside"]) + out["counts"].sum() == n
    assert np.abs(out["sums"][..., 1]).max() > 0.1 and out["inv_bin_volume_sum"] == 1.0 / (ln[0] * ln[1] * ((rng_z[1] - rng_z[0]) / 11))
    md.set_spatial_("x", 9, groups=groups, n_groups=2)
    md.spatial_sample_()
    ref = _reference(md, masses, charges, groups, 2, _geom(md, sp.X, 9))
    out = md.spatial()
    _check(out, ref, "water slab, periodic axis")
    assert out["outside"] == [0, 0] and out["counts"].sum() == n


def test_a_bonded_charged_slab_with_exclusions(emdee, dev):
    E = emdee
    S = oc.chain_system(E, np.float64)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    md = _ortho_engine(E, S, atoms, dev)
    _dress(md, S)
    n = S["pos"].shape[0]
    masses = np.ones(n) if S["inv_mass"] is None else 1.0 / np.asarray(S["inv_mass"])
    for axis, n_bins, rng in ((sp.Y, 5, None), (sp.Z, 6, (float(S["lo"][2]) + 0.4, float(S["lo"][2] + S["lengths"][2]) - 0.3))):
        md.set_spatial_(axis, n_bins, range=rng)
        md.spatial_sample_()
        ref = _reference(md, masses, S["q"], None, 1, _geom(md, axis, n_bins, range=rng))
        _check(md.spatial(), ref, "chains, axis %d" % axis)


def test_the_lj_slab_along_its_open_axis_with_atoms_beyond_both_faces(emdee, dev):
    E = emdee
    S = oc.lj_slab(E.synthetic)
    S = dict(S)
    pos = np.array(S["pos"], dtype=np.float64)
    lo, ln = np.array(S["lo"]), np.array(S["lengths"])
    zs = np.argsort(pos[:, 2])
    pos[zs[:2], 2] = lo[2] - np.array([0.21, 0.55])
    pos[zs[-2:], 2] = lo[2] + ln[2] + np.array([0.17, 0.62])
    S["pos"] = pos
    md = _slab_engine(E, dev, S, bref.lj_atoms(S["N"]))
    rng_z = (float(lo[2]) + 0.61, float(lo[2] + ln[2]) - 0.77)
    md.set_spatial_("z", 13, range=rng_z)
    md.spatial_sample_()
    ref = _reference(md, np.ones(S["N"]), None, None, 1, _geom(md, sp.Z, 13, range=rng_z))
    out = md.spatial()
    _check(out, ref, "lj slab, open axis")
    assert out["outside"][0] >= 4 and out["outside"][0] + out["counts"].sum() == S["N"]


# ---------------------------------------------------------------- 6. radial
def _droplet(E, dev):
    S = oc.pair_system(E.synthetic, "droplet", np.float64)
    md = _ortho_engine(E, S, bref.lj_atoms(S["N"]), dev)
    return S, md


def test_droplet_shells_around_a_fixed_centre_with_an_atom_on_it(emdee, dev):
    E = emdee
    S = oc.pair_system(E.synthetic, "droplet", np.float64)
    centre = np.array(S["lo"]) + 0.5 * np.array(S["lengths"]) + np.array([0.11, -0.07, 0.05])
    i = int(np.argmin(np.linalg.norm(S["pos"] - centre, axis=1)))
    centre = np.array(S["pos"][i], dtype=np.float64)        # an atom exactly on the centre: r = 0
    md = _ortho_engine(E, S, bref.lj_atoms(S["N"]), dev)
    r_max = 0.45 * float(np.min(S["lengths"]))
    md.set_spatial_("radial", 9, range=r_max, centre=centre)
    md.spatial_sample_()
    geom = _geom(md, sp.RADIAL, 9, range=(0.0, r_max), centre=centre)
    ref = _reference(md, np.ones(S["N"]), None, None, 1, geom)
    out = md.spatial()
    _check(out, ref, "droplet, fixed centre")
    assert out["counts"][0, 0] >= 1 and out["outside"][0] > 0 and out["inv_bin_volume_sum"] == 0.0
    assert abs(out["bin_volume"].sum() - 4.0 * np.pi / 3.0 * r_max ** 3) <= 1e-13 * r_max ** 3


def _centre_of_mass(md, ids, masses):
    """the centre the device forms, in its order (include/emdee_hip.h): per chunk of 1024 entries of the group, ascending id, a
    halving tree over m x, m y, m z and m -- zeros beyond the count --, the chunks in order, then R = (sum m x) / M; from the unwrapped
    coordinates state() returns.  numpy's elementwise products and sums round once each, as the kernel's do."""
    x = _np(md.state(forces=False)["positions"])[ids]
    m = masses[ids]
    tot = np.zeros(4)
    for at in range(0, len(ids), 1024):
        v = np.zeros((1024, 4))
        cnt = min(1024, len(ids) - at)
        v[:cnt, :3] = m[at:at + cnt, None] * x[at:at + cnt]
        v[:cnt, 3] = m[at:at + cnt]
        h = 512
        while h >= 1:
            v = v[:h] + v[h:2 * h]
            h //= 2
        tot = tot + v[0]
    return tot[:3] / tot[3]


def _stable_under_a_shift(md, masses, groups, n_groups, n_bins, r_max, centre, ref):
    """on the reference: moving the centre by 1e-12 r_max along any axis changes no bin"""
    for d in range(3):
        for sign in (-1.0, 1.0):
            c = np.array(centre)
            c[d] += sign * 1e-12 * r_max
            other = _reference(md, masses, None, groups, n_groups, _geom(md, sp.RADIAL, n_bins, range=(0.0, r_max), centre=c), what=3)
            assert np.array_equal(other["bins"], ref["bins"]), (d, sign)


def test_droplet_shells_around_the_centre_of_mass_of_a_group(emdee, dev):
    E = emdee
    S, md = _droplet(E, dev)
    n = S["N"]
    masses = np.ones(n)
    groups = (np.arange(n) % 4 == 0).astype(int)            # group 1: the centre group, a quarter of the droplet
    r_max = 0.4 * float(np.min(S["lengths"]))
    md.set_spatial_("radial", 8, groups=groups, n_groups=2, range=r_max, centre_group=1)
    md.spatial_sample_()
    centre = _centre_of_mass(md, np.nonzero(groups == 1)[0], masses)
    ref = _reference(md, masses, None, groups, 2, _geom(md, sp.RADIAL, 8, range=(0.0, r_max), centre=centre))
    _stable_under_a_shift(md, masses, groups, 2, 8, r_max, centre, ref)
    _check(md.spatial(), ref, "droplet, centre group")


def test_a_centre_group_that_straddles_a_face_of_a_periodic_box(emdee, dev):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    L = S["L"]
    md.step_(40, DT)                                        # atoms cross the faces: their image counts are not all 0
    x = _np(md.state(forces=False)["positions"])
    near = np.nonzero((np.mod(x[:, 0], L) < 1.6) | (np.mod(x[:, 0], L) > L - 1.6))[0]
    groups = np.zeros(len(masses), dtype=int)
    groups[near] = 1
    wrapped = np.mod(x[near, 0], L)
    assert (wrapped < 1.6).sum() > 20 and (wrapped > L - 1.6).sum() > 20       # on both sides of the face
    md.set_spatial_("radial", 6, groups=groups, n_groups=2, range=0.45 * L, centre_group=1, stress=False)
    md.spatial_sample_()
    centre = _centre_of_mass(md, near, masses)              # from the unwrapped coordinates state() returns
    ref = _reference(md, masses, None, groups, 2, _geom(md, sp.RADIAL, 6, range=(0.0, 0.45 * L), centre=centre), what=3)
    _stable_under_a_shift(md, masses, groups, 2, 6, 0.45 * L, centre, ref)
    _check(md.spatial(), ref, "periodic box, centre group across a face")


# ---------------------------------------------------------------- 7. barostat
def test_fractional_bins_follow_the_box_under_berendsen(emdee, dev):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    md.set_barostat_(E.BAROSTAT_BERENDSEN, 5.0, 0.02, 1.0, 4)
    md.set_spatial_("z", 7, stress=False)
    inv, ref = 0.0, None
    boxes = []
    for _ in range(3):
        md.step_(4, DT)                                     # one coupling event per call
        md.spatial_sample_()
        lo, ln = md.box()
        boxes.append(ln[2])
        inv += 1.0 / (ln[0] * ln[1] * (ln[2] / 7))
        r = _reference(md, masses, None, None, 1, _geom(md, sp.Z, 7), what=3)
        ref = r if ref is None else _add(ref, r)
    assert len(set(boxes)) == 3                             # the box moved at every event
    out = md.spatial()
    _check(out, ref, "berendsen")
    assert out["inv_bin_volume_sum"] == inv and out["frames"] == 3


# ---------------------------------------------------------------- 8. reproducibility
def _raw(md):
    out = md.spatial()
    return out["counts"].tobytes(), out["sums"].tobytes()


def test_two_engines_given_the_same_calls_agree_in_every_bit(emdee, dev):
    E = emdee
    raws = []
    for _ in range(2):
        S, md, masses = _fluid_engine(E, dev, np.float64)
        md.set_spatial_("y", 64, groups=_fluid_groups(len(masses)), n_groups=2)
        for _ in range(3):
            md.step_(3, DT)
            md.spatial_sample_()
        raws.append(_raw(md))
    assert raws[0] == raws[1]


@pytest.mark.parametrize("stress", [False, True])
def test_an_engine_that_samples_stays_bit_for_bit_the_one_that_does_not(emdee, dev, stress):
    E = emdee
    states = []
    for sampling in (True, False):
        S, md, masses = _fluid_engine(E, dev, np.float64)
        if sampling:
            md.set_spatial_("z", 16, density=not stress, kinetic=not stress, stress=stress)
        for _ in range(4):
            md.step_(3, DT)
            if sampling:
                md.spatial_sample_()
        st = md.state()
        states.append(b"".join(st[k].cpu().numpy().tobytes() for k in ("positions", "velocities", "forces")))
    assert states[0] == states[1]


def test_a_rebuild_between_two_samples_changes_no_bit(emdee, dev):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    md.step_(7, DT)
    # (density and kinetic words: the per-atom energies and tensors are the engine's to re-evaluate after a rebuild, in the order of
    # its new rows -- they are the sample's input, not its sums)
    md.set_spatial_("x", 64, groups=_fluid_groups(len(masses)), n_groups=2, stress=False)
    md.spatial_sample_()
    first = md.spatial()
    md.rebuild_()
    md.spatial_sample_()
    both = md.spatial()
    assert np.array_equal(both["counts"], 2 * first["counts"])
    assert (2.0 * first["sums"]).tobytes() == both["sums"].tobytes()        # the sum of two equal doubles is exact
    md.spatial_reset_()
    out = md.spatial()
    assert out["frames"] == 0 and out["counts"].sum() == 0 and not out["sums"].any() and out["inv_bin_volume_sum"] == 0.0


def test_a_rebuild_between_two_stress_samples_keeps_the_counts_and_the_bound(emdee, dev):
    """with EMDEE_SPATIAL_STRESS the engine re-evaluates the per-atom energies and tensors after a rebuild, in the order of its new
    rows: the sample's inputs move in the last bit, so the two frames are held to the exact counts and to the word bound"""
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    md.step_(7, DT)
    groups = _fluid_groups(len(masses))
    md.set_spatial_("x", 64, groups=groups, n_groups=2)
    md.spatial_sample_()
    geom = _geom(md, sp.X, 64)
    ref = _reference(md, masses, None, groups, 2, geom)
    first = md.spatial()
    _check(first, ref, "stress, before the rebuild")
    md.rebuild_()
    md.spatial_sample_()
    both = md.spatial()
    assert np.array_equal(both["counts"], 2 * first["counts"])
    assert (2.0 * first["sums"][..., :7]).tobytes() == both["sums"][..., :7].tobytes()   # the density and kinetic words: every bit
    _check(both, _add(ref, _reference(md, masses, None, groups, 2, geom)), "stress, two frames across a rebuild")


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_previous_table_and_its_sums(emdee, dev):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    L = S["L"]
    md.set_spatial_("z", 7)
    md.spatial_sample_()
    before = _raw(md)
    bad = [(dict(geometry=4, n_bins=4), "geometry = 4"),
           (dict(geometry="z", n_bins=4, density=False, kinetic=False, stress=False), "non-empty mask"),
           (dict(geometry="z", n_bins=4097), "n_bins = 4097"),
           (dict(geometry="z", n_bins=-1), "n_bins = -1"),
           (dict(geometry="z", n_bins=4, n_groups=9), "n_groups = 9"),
           (dict(geometry="z", n_bins=4, n_groups=0), "n_groups = 0"),
           (dict(geometry="z", n_bins=4, n_groups=2), "groups is NULL"),
           (dict(geometry="z", n_bins=4, groups=np.full(864, 3), n_groups=2), "the group 3 of atom 0"),
           (dict(geometry="z", n_bins=4, range=(0.0, 1.0)), "is periodic"),
           (dict(geometry="radial", n_bins=4, centre=[0, 0, 0]), "needs range"),
           (dict(geometry="radial", n_bins=4, range=(1.0, 2.0), centre=[0, 0, 0]), "{0, r_max}"),
           (dict(geometry="radial", n_bins=4, range=float("inf"), centre=[0, 0, 0]), "{0, r_max}"),
           (dict(geometry="radial", n_bins=4, range=0.51 * L, centre=[0, 0, 0]), "half the shortest periodic side"),
           (dict(geometry="radial", n_bins=4, range=2.0), "needs a centre"),
           (dict(geometry="radial", n_bins=4, range=2.0, centre=[0.0, float("nan"), 0.0]), "not finite"),
           (dict(geometry="radial", n_bins=4, range=2.0, centre_group=1), "centre_group = 1"),
           (dict(geometry="radial", n_bins=4, range=2.0, centre_group=-2), "centre_group = -2")]
    for kw, text in bad:
        assert text in _refused(E, ERR_INVALID, md.set_spatial_, **kw), kw
        assert _raw(md) == before and md.spatial()["frames"] == 1
    md.spatial_sample_()                                    # the table in force still samples
    assert md.spatial()["frames"] == 2
    md.set_spatial_("z", 0)                                 # n_bins = 0 clears the table
    md._spatial = ("z", 7, 1, None)
    assert "no table is set" in _refused(E, ERR_STATE, md.spatial_sample_)
    assert "no table is set" in _refused(E, ERR_STATE, md.spatial)
    assert "no table is set" in _refused(E, ERR_STATE, md.spatial_reset_)


def test_open_axis_ranges_and_a_massless_centre_group_are_refused(emdee, dev):
    E = emdee
    S = oc.lj_slab(E.synthetic)
    inv_mass = np.ones(S["N"])
    inv_mass[:3] = 0.0
    md = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"], dev), float(S["lengths"][0]), E.LennardJonesModel(S["rc"], S["rs"]),
                          E.cu(bref.lj_atoms(S["N"]), dev), skin=S["skin"], inv_mass=E.cu(inv_mass, dev), lo=list(S["lo"]),
                          lengths=list(S["lengths"]), periodic=list(S["periodic"]))
    assert "is open" in _refused(E, ERR_INVALID, md.set_spatial_, "z", 4)
    assert "r0 < r1" in _refused(E, ERR_INVALID, md.set_spatial_, "z", 4, range=(1.0, 1.0))
    assert "r0 < r1" in _refused(E, ERR_INVALID, md.set_spatial_, "z", 4, range=(0.0, float("nan")))
    groups = np.zeros(S["N"], dtype=int)
    groups[:3] = 1                                          # three massless atoms
    assert "total mass 0" in _refused(E, ERR_INVALID, md.set_spatial_, "radial", 4, groups=groups, n_groups=2, range=2.0, centre_group=1)
    # only the periodic sides bound r_max: half of x or y, whatever the open z is
    half = 0.5 * float(min(S["lengths"][0], S["lengths"][1]))
    assert "periodic side" in _refused(E, ERR_INVALID, md.set_spatial_, "radial", 4, range=1.01 * half, centre=[0, 0, 0])
    md.set_spatial_("radial", 4, groups=groups, n_groups=2, range=0.99 * half, centre_group=0)
    md.spatial_sample_()
    out = md.spatial()
    assert out["sums"][1, :, 0].sum() == 0.0 and out["counts"].sum() + sum(out["outside"]) == S["N"]     # massless atoms are binned, with mass 0


def test_state_refusals(emdee, dev):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    md.set_spatial_("z", 7)
    md.spatial_sample_()
    # a state of another atom count: the sample is refused, the table stays
    keep = 800
    md.set_state_(E.cu(S["pos"][:keep], dev), E.cu(S["vel"][:keep], dev), E.cu(S["atoms"][:keep], dev))
    assert "the table was set for 864 atoms" in _refused(E, ERR_STATE, md.spatial_sample_)
    assert md.spatial()["frames"] == 1
    # a radial table whose r_max a shrunken box no longer holds
    S, md, masses = _fluid_engine(E, dev, np.float64)
    md.set_spatial_("radial", 4, range=0.499 * S["L"], centre=[1.0, 2.0, 3.0], stress=False)
    md.spatial_sample_()
    md.scale_box_([0.99, 1.0, 1.0])
    assert "the box has shrunk" in _refused(E, ERR_STATE, md.spatial_sample_)
    assert md.spatial()["frames"] == 1


def test_lent_unloaded_and_ghost_engines_refuse_a_table(emdee, dev):
    """the shared whole-box refusals, on the pattern of test_gpu_msd: each with a distinctive part of its text"""
    E = emdee
    S = bref.fluid864(E.synthetic)
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (a decomposition needs two bricks of 2.8 + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    assert "lent" in _refused(E, ERR_STATE, dd.engine(0).set_spatial_, "z", 4)
    dd.step_(2, DT)                                                                      # the decomposition is unharmed
    dd.close()
    model = E.LennardJonesModel(bref.RC, bref.RS)
    g = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"][:-4], dev), S["L"], model, E.cu(S["atoms"], dev), skin=bref.SKIN, n_ghost=4)
    assert "ghosts" in _refused(E, ERR_STATE, g.set_spatial_, "z", 4)
    assert "ghosts" in _refused(E, ERR_STATE, g.set_spatial_, "radial", 4, range=2.0, centre=[1.0, 1.0, 1.0], stress=False)
    g.close()
    # before emdee_md_set_state, through the C ABI
    ctx = E.context_for(dev)
    h = C.c_void_p()
    three = lambda *v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", ctx.handle, three(0, 0, 0), three(S["L"], S["L"], S["L"]), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(model), bref.SKIN, 8, C.byref(h))
    assert "no state loaded" in _refused(E, ERR_STATE, E._lib.call, "emdee_md_set_spatial", h, 2, 7, 4, 1, None, None, None, -1)
    assert "no table is set" in _refused(E, ERR_STATE, E._lib.call, "emdee_md_spatial_sample", h)
    E._lib.call("emdee_md_destroy", h)


def _constrained_case(md, masses, what_fn, setter):
    E_state = ERR_STATE
    text = what_fn(E_state, md.set_spatial_, "z", 5)
    assert "EMDEE_SPATIAL_STRESS" in text and setter in text
    text = what_fn(E_state, md.set_spatial_, "z", 5, density=False, kinetic=False)
    assert setter in text
    md.set_spatial_("z", 5, stress=False)                   # DENSITY | KINETIC are accepted
    md.spatial_sample_()
    ref = _reference(md, masses, None, None, 1, _geom(md, sp.Z, 5), what=3)
    _check(md.spatial(), ref, "density and kinetic beside %s" % setter)


def test_stress_is_refused_beside_constraints_and_the_rest_is_accepted(emdee, dev):
    E = emdee
    refused = lambda code, call, *a, **kw: _refused(E, code, call, *a, **kw)
    B = sr.water_box()
    md = _water_engine(E, dev, B)
    _constrained_case(md, np.asarray(B["mass"], dtype=np.float64), refused, "emdee_md_set_rigid3")
    H = hr.mixed_box()
    md = _hbonds_engine(E, dev, H)
    _constrained_case(md, np.asarray(H["mass"], dtype=np.float64), refused, "emdee_md_set_hbonds")
    # a table attached after the set: the sample re-checks
    S, md, masses = _fluid_engine(E, dev, np.float64)
    md.set_spatial_("z", 5)
    md.spatial_sample_()
    d = S["pos"] - S["pos"][0]
    d -= S["L"] * np.rint(d / S["L"])
    r = np.linalg.norm(d, axis=1)
    r[0] = np.inf
    j = int(np.argmin(r))                                   # a bond from atom 0 to its nearest neighbour, at its loaded length
    md.set_hbonds_([[0, j, -1, -1]], [[float(r[j]), 0.0, 0.0]])
    assert "emdee_md_set_hbonds" in _refused(E, ERR_STATE, md.spatial_sample_)
    assert md.spatial()["frames"] == 1


# ---------------------------------------------------------------- 10. kernel time
def test_kernel_time_counts_the_launches_the_header_documents(emdee, dev):
    E = emdee
    S, md, masses = _fluid_engine(E, dev, np.float64)
    groups = _fluid_groups(len(masses))
    md.state(energies=True)                                 # the forces are current before the timers start
    cases = [(dict(geometry="z", n_bins=7, stress=False, kinetic=False), 3), (dict(geometry="z", n_bins=7), 3),
             (dict(geometry="x", n_bins=7, density=False, stress=False), 3),
             (dict(geometry="radial", n_bins=7, range=3.0, centre=[1, 1, 1]), 3),
             (dict(geometry="radial", n_bins=7, range=3.0, groups=groups, n_groups=2, centre_group=0), 5),
             (dict(geometry="radial", n_bins=7, range=3.0, groups=groups, n_groups=2, centre_group=1, stress=False, kinetic=False), 5)]
    for kw, launches in cases:
        md.set_spatial_(**kw)
        md.profile_(True)
        md.spatial_sample_()
        md.spatial_sample_()
        ms, k = md.kernel_time("spatial")
        assert k == 2 * launches and ms > 0.0, (kw, k)
        assert md.kernel_time(21)[1] == k
        if not kw.get("stress", True):                      # a sample without STRESS runs no pass of the engine
            for other in (0, 15, 16, 17):
                assert md.kernel_time(other)[1] == 0, (kw, other)
        md.profile_(False)
