"""GPU tests of every stage behind the pair loop on a SLAB (periodic x and y, z open, lo != 0) and on a DROPLET (all three
axes open): the constraint stages (csrc/settle.hpp image(), SettleBox::per), virtual sites (csrc/vsite.hpp vsite_image()), the
bonded terms and reaction-field charges, position restraints, and the box scale on open axes (include/emdee_hip.h and DESIGN.md,
"Open axes").  Every other GPU module creates its engines of these stages with periodic = (1, 1, 1).

Boxes: tests/helpers/open_cases.py -- settle_ref.water_box, shake_ref.mixed_box and vsite_ref.four_site_box (geometry, counts
and parameters unchanged) re-boxed, "tall" molecules whose sites are more than half the open length apart, and chains along the
open axis of a one-cell-thick slab.  Each test asserts on the CPU, before it touches the device, that the yardstick with the open
axes taken as periodic differs from the right one by at least 100 x the tolerance in use (tests/test_open_axes_host.py pins the
same without a GPU).  Each compares with the numpy reference of its stage; the force field is ortho_ref.total(..., periodic).

Tolerances are those of the periodic counterpart of each test, named where used."""
import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import molecular_ref as mr
from .helpers import open_cases as oc
from .helpers import ortho_ref as oref
from .helpers import restraint_ref as rr
from .helpers import settle_ref as sr
from .helpers import shake_ref as hr
from .helpers import vsite_ref as vr
from .test_gpu_bonded import _outputs
from .test_gpu_orthorhombic import DT as DT_LJ
from .test_gpu_orthorhombic import TOL, X32, X64, _dress, _engine, _part_bound
from .test_gpu_settle import EPS32, _forces, _xv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT = sr.DT
EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: EPS32}
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
KINDS = pytest.mark.parametrize("kind", list(oc.KINDS))
PART = {np.float64: 1e-9, np.float32: 1e-4}             # a post term alone: tests/test_gpu_restraints.py TOL, test_gpu_orthorhombic.PART


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _stage_engine(E, dev, B, dtype=np.float64, rigid=True, hbonds=False, sites=False, charged=False, pos=None, vel=None, lengths=None):
    pos, vel = B["pos"] if pos is None else pos, B["vel"] if vel is None else vel
    lengths = [float(t) for t in (B["lengths"] if lengths is None else lengths)]
    md = E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), lengths[0],
                          E.LennardJonesModel(sr.RC, sr.RS), E.cu(B["atoms"], dev), skin=sr.SKIN, inv_mass=E.cu(B["inv_mass"].astype(dtype), dev),
                          lo=[float(t) for t in B["lo"]], lengths=lengths, periodic=list(B["periodic"]))
    md.set_exclusions_(B["excl"])
    if charged:
        md.set_coulomb_(B["charges"], 1.0)
    if hbonds:
        md.set_hbonds_(B["clusters"], B["dist"])
    if rigid and len(B["mol"]):
        md.set_rigid3_(B["mol"], B["geom"])
    if sites:
        md.set_vsites_(B["vs_atoms"], B["vs_weights"])
    return md


def _force_field_matches(md, right, dtype, what):
    """the engine's forces at the load against ortho_ref.total (test_gpu_orthorhombic.TOL: 1e-6 / 1e-4 of the largest entry)"""
    f = _forces(md)
    err, scale = np.abs(f - right["f"]).max(), np.abs(right["f"]).max()
    print("%s: forces at the load within %.3e of max %.3e (tol %.0e)" % (what, err, scale, TOL[dtype]))
    assert err <= TOL[dtype] * scale, (what, err)


def _against_reference(md, B, checkpoints, rebuild_every, what):
    """test_gpu_settle._against_reference / test_gpu_hbonds._against_reference on the box's own sides: the engine, one step per
    call, against shake_ref.constrained_verlet fed the engine's own forces; 1e-11 of the largest side and of the rms velocity"""
    seen, offset = {}, B["pos"] - B["unwrapped"]

    def force(x, k):
        if k > 0:
            md.step_(1, DT, rebuild_every)
        return _forces(md)

    def observe(s, x, v):
        if s in checkpoints:
            gx, gv = _xv(md)
            seen[s] = (np.abs(gx - (x + offset)).max(), np.abs(gv - v).max(), np.sqrt((v * v).sum(axis=1).mean()))
    hr.constrained_verlet(B["unwrapped"], B["vel"], force, max(checkpoints), DT, B["pairs"], B["mass"], observe=observe)
    for s in checkpoints:
        ex, ev, vrms = seen[s]
        print("%s, step %d: max |dx| = %.3e (box side %.1f), max |dv| = %.3e (rms velocity %.3f)" % (what, s, ex, B["lengths"].max(), ev, vrms))
        assert ex <= 1e-11 * B["lengths"].max() and ev <= 1e-11 * vrms, (what, s, ex, ev)


def _constraints_hold(md, B, dtype, what):
    """test_gpu_hbonds._constraints_hold with the box's periodic flags: 1e-12 in fp64; in fp32 8 ulp_fp32(largest coordinate) / d
    for a distance d and 8 eps_fp32 for the bond-relative velocities, read from the records (pack_positions with a zero shift: a
    Float32 engine with masses keeps absolute records, which the geometry stage itself used)"""
    x, v = _xv(md)
    pairs = B["pairs"]
    i, j, d = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64), pairs[:, 2]
    if dtype == np.float64:
        tol_x, tol_v = np.full(len(d), 1e-12), np.full(len(d), 1e-12)
    else:
        ulp = float(np.spacing(np.float32(np.abs(x).max())))
        tol_x, tol_v = 8.0 * ulp / d, np.full(len(d), 8.0 * EPS32)
        ids = torch.arange(x.shape[0], dtype=torch.int32, device=md.device)
        x = md.pack_positions(ids, [0.0, 0.0, 0.0]).cpu().numpy().astype(np.float64)
    u = hr.unwrap(x, pairs, B["lengths"], B["periodic"])
    res = np.abs(np.linalg.norm(u[i] - u[j], axis=1) / d - 1.0)
    left = hr.bond_velocities(u, v, pairs)
    print("%s: largest relative distance error %.3e (%.2f of its bound), largest bond-relative velocity / (|v| d) %.3e (%.2f of its bound)"
          % (what, res.max(), (res / tol_x).max(), left.max(), (left / tol_v).max()))
    assert (res <= tol_x).all() and (left <= tol_v).all(), (what, res.max(), left.max())


# ---------------------------------------------------------------- 1. rigid water, tall molecules, hbonds clusters
@DTYPES
@KINDS
@pytest.mark.parametrize("name", ["water", "tall", "mixed"])
def test_constraint_stages_on_open_axes(emdee, dev, name, kind, dtype):
    """SETTLE / RATTLE (and SHAKE stars in "mixed") where image() must leave the open axes alone.  fp64: positions and
    velocities after 1 and 20 steps with rebuilds against the reference; both precisions: the constraints after 40 more steps
    with automatic rebuilds."""
    B = oc.stage_box(name, kind)
    right = oc.assert_stage_conditions(B, TOL[dtype])
    if name == "tall":
        assert (oc.tall_spans(B) > 0.5).all()            # image() along z would fold a leg of every molecule
    md = _stage_engine(emdee, dev, B, dtype, hbonds=(name == "mixed"))
    what = "%s %s %s" % (name, kind, np.dtype(dtype).name)
    _force_field_matches(md, right, dtype, what)
    if dtype == np.float64:
        _against_reference(md, B, (1, 20), 3, what)
        assert md.nbr_stats()["builds"] >= 1 + 20 // 3
    before = md.nbr_stats()["builds"]
    md.step_(40, DT)
    assert name == "tall" or md.nbr_stats()["builds"] > before
    _constraints_hold(md, B, dtype, what)
    md.close()


# ---------------------------------------------------------------- 2. virtual sites
def _gap(x, want, B):
    return np.abs(oref.image_difference(x, want, B["lengths"], B["periodic"])).max()


def _sites_on_parents(md, B, dtype, what):
    """test_gpu_vsites._sites_on_parents with the box's periodic flags: 8 eps(real) of the largest box side"""
    x, v = _xv(md)
    want = vr.place(x, B["vs_atoms"], B["vs_weights"], B["lengths"], B["periodic"])
    gap, bound = _gap(x[B["sites"]], want, B), 8.0 * EPS[dtype] * float(B["lengths"].max())
    print("%s: sites against their parents %.3e (bound %.3e)" % (what, gap, bound))
    assert gap <= bound, (what, gap)
    assert (v[B["sites"]] == 0.0).all()
    return x


def _spread_matches(E, dev, md, twin, B, dtype, what):
    """test_gpu_vsites._check_spread_forces: the engine's forces are vsite_ref.spread of the forces of a twin without a site table
    loaded with the engine's positions; 8 eps(real) of the largest force in the molecule"""
    x = md.state(velocities=False, forces=False)["positions"].cpu().numpy()
    twin.set_state_(E.cu(x.astype(dtype), dev), E.cu(np.zeros_like(x).astype(dtype), dev), E.cu(B["atoms"], dev), E.cu(B["inv_mass"].astype(dtype), dev))
    raw, f = _forces(twin), _forces(md)
    want = vr.spread(raw, B["vs_atoms"], B["vs_weights"])
    four = np.concatenate([B["mol"], B["sites"][:, None]], axis=1)
    big, per_atom = np.abs(raw[four]).max(axis=(1, 2)), np.zeros(raw.shape[0])
    for k in range(4):
        per_atom[four[:, k]] = big
    bound = 8.0 * EPS[dtype] * per_atom[:, None]
    assert (f[B["sites"]] == 0.0).all()
    assert (np.abs(want - raw)[B["real"]] > 100.0 * bound[B["real"]]).any()          # (the sites carried forces)
    err = np.abs(f - want)
    print("%s: largest |f - spread(f_twin)| / (8 eps max |f| of the molecule) = %.3f" % (what, (err / bound).max()))
    assert (err <= bound).all(), what
    return x, f


@DTYPES
@KINDS
@pytest.mark.parametrize("name", ["water4", "tall4"])
def test_virtual_sites_on_open_axes(emdee, dev, name, kind, dtype):
    """Placement against vsite_ref.place(..., periodic), spreading against vsite_ref.spread, and the spread forces against
    ortho_ref (reaction field), at the load and after 10 steps with a rebuild."""
    E = emdee
    B = oc.stage_box(name, kind)
    oc.assert_stage_conditions(B, TOL[dtype], charged=True)
    what = "%s %s %s" % (name, kind, np.dtype(dtype).name)
    if name == "tall4":
        folded = vr.place(B["unwrapped"], B["vs_atoms"], B["vs_weights"], B["lengths"], (1, 1, 1))
        assert np.abs(folded - B["unwrapped"][B["sites"]]).max() >= 100 * 8.0 * EPS[dtype] * B["lengths"].max()
    # the sites are loaded 0.2 off where they belong: the set call places them
    pos = B["pos"].copy()
    pos[B["sites"]] += 0.2
    md = _stage_engine(E, dev, B, dtype, sites=True, charged=True, pos=pos)
    twin = _stage_engine(E, dev, B, dtype, sites=False, charged=True, rigid=False)
    for stage in ("at the load", "after 10 steps"):
        x = _sites_on_parents(md, B, dtype, "%s, %s" % (what, stage))
        x, f = _spread_matches(E, dev, md, twin, B, dtype, "%s, %s" % (what, stage))
        u = hr.unwrap(x.astype(np.float64), B["pairs"], B["lengths"], B["periodic"])
        u[B["sites"]] = vr.place(u, B["vs_atoms"], B["vs_weights"], B["lengths"], B["periodic"])
        ref = vr.spread(oc.stage_total(B, u, charged=True)["f"], B["vs_atoms"], B["vs_weights"])
        assert np.abs(f - ref).max() <= TOL[dtype] * np.abs(ref).max(), (what, stage)
        if stage == "at the load":
            md.step_(10, DT, 4)
    _constraints_hold(md, B, dtype, what)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 3. chains along the open axis
@DTYPES
def test_chains_along_the_open_axis_parts_and_whole(emdee, dev, dtype):
    """test_gpu_orthorhombic.test_chains_cross_every_face_parts_and_whole on open_cases.chain_system: the bonded part and the
    Coulomb part alone (_part_bound), the whole (TOL), then open_cases.CHAIN_STEPS steps against ortho_ref.verlet (X64 / X32)."""
    E = emdee
    S = oc.chain_system(E, dtype)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    bonded, coul, whole = parts = oc.chain_parts(S, atoms)
    oc.assert_chain_conditions(S, atoms, parts, TOL[dtype])
    md = _engine(E, S, atoms, dev)
    bare = _outputs(md)
    _dress(md, S, charged=False)
    with_b = _outputs(md)
    _dress(md, S, bonded=False)
    full = _outputs(md)
    for g, p, key in zip(with_b[:4], bare[:4], "fewt"):
        assert np.abs((g - p) - bonded[key]).max() <= _part_bound(dtype, bonded[key], g), ("bonded", key)
    for g, p, key in zip(full[:4], with_b[:4], "fewt"):
        assert np.abs((g - p) - coul[key]).max() <= _part_bound(dtype, coul[key], g), ("coulomb", key)
    for g, key in zip(full[:4], "fewt"):
        assert np.abs(g - whole[key]).max() <= TOL[dtype] * np.abs(whole[key]).max(), ("whole", key)
    xr, vr_ = oc.chain_trajectory(S, atoms, oc.CHAIN_STEPS)
    md.step_(oc.CHAIN_STEPS, DT_LJ)
    x, v = _xv(md)
    assert md.nbr_stats()["builds"] >= 2
    dx = np.abs(oref.image_difference(x, xr, S["lengths"], S["periodic"])).max()
    print("chains %s: %d builds, max |dx| %.3e, max |dv| %.3e" % (np.dtype(dtype).name, md.nbr_stats()["builds"], dx, np.abs(v - vr_).max()))
    lim = X64 if dtype == np.float64 else X32
    assert dx < lim and np.abs(v - vr_).max() < 10 * lim
    assert np.abs(x[:, 2] - xr[:, 2]).max() < lim        # the open axis: no whole box length taken out
    md.close()


# ---------------------------------------------------------------- 4. restraints
def _restraint_part(md, ids, k, ref, flat):
    without = _outputs(md)
    md.set_restraints_(ids, k, ref=ref, flat=flat)
    return [a - b for a, b in zip(_outputs(md)[:4], without[:4])]


@DTYPES
@pytest.mark.parametrize("name", ["open-z", "droplet"])
def test_restraints_on_open_axes(emdee, dev, name, dtype):
    """open-z: a slab pinned along its open axis, k = (0, 0, kz).  droplet: every atom held by one flat-bottomed sphere about the
    droplet's centre, the atoms beyond the faces (open_cases' outsiders) outside the well.  Planes and restraint_sums against
    restraint_ref (tests/test_gpu_restraints.py: 1e-9 / 1e-4 of the largest entry), ref = NULL, and the references after
    scale_box_ against restraint_ref.scale_ref (4 x 2^-53, as test_harmonic_virial_scale_box_and_references).
    (After the scale the cells are up to 1.03 times wider and the guaranteed distance of a Float32 engine, 32 - 6 w, shorter: the
    outsiders placed at 0.999 of it then lie a little beyond the new one, where the contract promises nothing.  What is compared
    after the scale -- the references and the table's own sums, fp64 arithmetic on single atoms -- does not depend on it.)"""
    E = emdee
    S = oc.pair_system(E.synthetic, name, dtype)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    right = oc.want(S, atoms)
    oc.assert_pair_conditions(S, atoms, right, TOL[dtype])
    N, tol = S["N"], PART[dtype]
    fmax = np.abs(right["f"]).max()
    rng = np.random.default_rng(5)
    outsiders = np.concatenate(list(S["outsiders"].values()))
    if name == "open-z":
        ids = np.unique(np.concatenate([rng.permutation(N)[:N // 3], outsiders]))
        k = np.zeros((len(ids), 3))
        k[:, 2] = rng.uniform(0.5, 1.5, len(ids)) * fmax / 0.15
        ref = S["pos"][ids] + rng.uniform(-0.15, 0.15, (len(ids), 3))
        flat = np.zeros(len(ids))
        # the outsiders of the upper face are pinned to references 0.6 len_z below them, inside the slab: a minimum image taken
        # along z would turn that displacement round (softer springs, so that their forces stay of the order of the pair forces)
        far = np.isin(ids, S["outsiders"][(2, 1)])
        ref[far, 2] = S["pos"][ids[far], 2] - 0.6 * S["lengths"][2]
        k[far, 2] = fmax / (0.6 * S["lengths"][2])
    else:
        ids = rng.permutation(N)
        centre = S["lo"] + 0.5 * S["lengths"]
        rho = np.linalg.norm(S["pos"][ids] - centre, axis=1)
        r0 = float(np.median(rho))
        k = np.full((N, 3), fmax / 0.5)
        ref, flat = np.tile(centre, (N, 1)), np.full(N, r0)
        out_of_box = np.isin(ids, outsiders)
        assert (rho[out_of_box] > r0).all() and (rho[~out_of_box] > r0).any() and (rho < r0).any()
    # the restraint reference with d folded by the minimum image along the open axes differs by at least 100 x tol
    folded = ref.copy()
    for a in range(3):
        if not S["periodic"][a]:
            folded[:, a] += S["lengths"][a] * np.rint((S["pos"][ids, a] - ref[:, a]) / S["lengths"][a])
    good, bad = rr.planes(N, ids, S["pos"], ref, k, flat), rr.planes(N, ids, S["pos"], folded, k, flat)
    assert np.abs(bad[0] - good[0]).max() >= 100 * tol * np.abs(good[0]).max()
    md = _engine(E, S, atoms, dev)
    got = _restraint_part(md, ids, k, ref, flat)
    x = md.state(velocities=False, forces=False)["positions"].cpu().numpy().astype(np.float64)
    want = rr.planes(N, ids, x, ref, k, flat)
    assert 0.05 * fmax <= np.abs(want[0]).max()
    for what, g, w in zip(("forces", "energies", "virials", "tensors"), got, want):
        err = np.abs(g - w).max() / np.abs(w).max()
        print("%s %s %s: max error / max entry = %.3e (bound %.0e)" % (name, np.dtype(dtype).name, what, err, tol))
        assert err <= tol, what
    if name == "open-z":
        assert (got[0][:, :2] == 0.0).all()                                            # k = (0, 0, kz): no force along x or y
    sums, want_sums = md.restraint_sums(), rr.sums(ids, x, ref, k, flat)
    assert np.abs(sums[:7] - want_sums[:7]).max() <= tol * np.abs(want_sums[:7]).max() and abs(sums[7] - want_sums[7]) <= tol * want_sums[7]
    # the box scale carries the references along on open axes too
    mu = np.array([1.02, 0.99, 1.03])
    md.scale_box_(mu)
    refs, want_refs = md.restraint_refs().cpu().numpy().astype(np.float64), rr.scale_ref(ref, S["lo"], mu)
    assert np.abs(refs - want_refs).max() <= 4 * 2.0 ** -53 * np.abs(want_refs).max()
    x = md.state(velocities=False, forces=False)["positions"].cpu().numpy().astype(np.float64)
    sums, want_sums = md.restraint_sums(), rr.sums(ids, x, want_refs, k, flat)
    assert np.abs(sums - want_sums).max() <= tol * np.abs(want_sums).max()
    # ref = NULL: the references are the current positions, on open axes the atoms beyond the faces where they are
    md.set_restraints_(ids, 40.0)
    assert md.restraint_sums().tolist() == [0.0] * 8
    refs = md.restraint_refs().cpu().numpy().astype(np.float64)
    open_ = [d for d in range(3) if not S["periodic"][d]]
    assert np.abs(refs - x[ids])[:, open_].max() <= (0.0 if dtype == np.float64 else 2.0 ** -18)   # (one fp32 ulp below 64)
    # periodic axes: the unwrapped coordinate is record + count x length, formed once for the reference and once by get_state --
    # fp64: a rounding each, 4 eps of the largest coordinate (tests/test_gpu_vsites.py: positions handed back); fp32: get_state
    # rounds to the engine's type, one fp32 ulp of the largest coordinate (tests/test_gpu_restraints.py: test_planes_at_the_load)
    big = np.abs(x).max()
    assert np.abs(refs - x[ids]).max() <= (4.0 * EPS[np.float64] * big if dtype == np.float64 else float(np.spacing(np.float32(big))))
    md.close()


# ---------------------------------------------------------------- 5. the box scale on open axes
MU = np.array([1.02, 0.99, 1.03])


@DTYPES
@pytest.mark.parametrize("name", ["open-z", "droplet"])
def test_scale_box_with_atoms_beyond_open_faces_equals_a_fresh_engine(emdee, dev, name, dtype):
    """test_gpu_barostat.test_scale_box_changes_the_cell_count_and_matches_a_fresh_engine on the pair cases of open_cases, three
    different factors: x -> lo + mu (x - lo) on open axes as on periodic ones (1e-14 relative in fp64, 2^-22 in fp32), the open
    lengths scaled, and the outputs those of a fresh engine on the scaled state (1e-12 / 1e-4) and of ortho_ref (1e-9).  Then the
    dealing of the steps to calls: step(40) against 8 x step(5) after the same scale, bit for bit, on engines that carry a
    restraint table (ref = NULL, so no force at the start) -- a table makes emdee_md_step take closed steps, the only kind for
    which the library promises that the dealing is immaterial; the merged kicks of a bare Lennard-Jones engine promise it on no
    box ("Open axes").
    Float32: after the scale the cells are up to 1.03 times wider, so the guaranteed distance 32 - 6 w is shorter and the
    outsiders placed at 0.999 of the old one lie a little beyond the new: for them the scaled fp32 comparisons run where the
    contract says "unspecified".  They are held to the counterpart's 1e-4 all the same and meet it."""
    E = emdee
    S = oc.pair_system(E.synthetic, name, dtype)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    oc.assert_pair_conditions(S, atoms, oc.want(S, atoms), TOL[dtype])
    md = _engine(E, S, atoms, dev)
    x0, v0 = _xv(md)
    md.scale_box_(MU)
    lo, ln = md.box()
    assert lo == list(S["lo"]) and ln == [m * l for m, l in zip(MU, S["lengths"])]
    x1, v1 = _xv(md)
    assert np.array_equal(v1, v0)
    want_x, _ = bref.scale(x0, S["lo"], S["lengths"], MU)
    rel = 1e-14 if dtype == np.float64 else 2.0 ** -22
    assert np.abs(x1 - want_x).max() <= rel * np.abs(want_x).max()
    for face in oc.faces(S):                                                       # the outsiders are still outsiders
        S1 = dict(S, lengths=np.array(ln))
        assert oc.beyond(S1, x1, *face)[S["outsiders"][face]].all()
    got = _outputs(md)
    S1 = dict(S, pos=x1, lengths=np.array(ln))
    fresh = _engine(E, S1, atoms, dev)
    want = _outputs(fresh)
    tol = 1e-12 if dtype == np.float64 else 1e-4
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= tol * np.abs(w).max()
    if dtype == np.float64:
        ref = oc.want(S1, atoms)
        for g, key in zip(got[:4], "fewt"):
            assert np.abs(g - ref[key]).max() <= 1e-9 * np.abs(ref[key]).max(), key
    md.step_(3, DT_LJ)
    fresh.step_(3, DT_LJ)
    gap = _gap(_xv(md)[0], _xv(fresh)[0].astype(np.float64), S1)
    assert gap <= (1e-12 if dtype == np.float64 else 1e-4)
    md.close()
    fresh.close()
    whole, dealt = _engine(E, S, atoms, dev), _engine(E, S, atoms, dev)
    for eng in (whole, dealt):
        eng.set_restraints_(np.arange(0, S["N"], 3), 40.0)
        eng.scale_box_(MU)
    whole.step_(40, DT_LJ)
    for _ in range(8):
        dealt.step_(5, DT_LJ)
    assert whole.nbr_stats()["builds"] >= 3
    for a, b in zip(_xv(dealt), _xv(whole)):
        assert np.array_equal(a, b)
    whole.close()
    dealt.close()


@KINDS
@pytest.mark.parametrize("name", ["water", "tall"])
def test_molecular_scale_on_open_axes(emdee, dev, name, kind):
    """Rigid molecules with molecular scaling: scale_box_ moves every site by (mu - 1) (Y - lo) of its molecule's centre of mass,
    on open axes too (molecular_ref.scale; test_gpu_molecular's X_TOL = 1e-11 of the largest side), the constraints hold
    afterwards, and the outputs are those of a fresh engine on the scaled state (1e-12)."""
    E = emdee
    B = oc.stage_box(name, kind)
    oc.assert_stage_conditions(B, TOL[np.float64])
    md = _stage_engine(E, dev, B)
    md.set_molecular_scaling_(True)
    x0, v0 = _xv(md)
    u0 = hr.unwrap(x0, B["pairs"], B["lengths"], B["periodic"])
    md.scale_box_(MU, 0.5)
    ln = np.array(md.box()[1])
    assert np.array_equal(ln, MU * B["lengths"])
    x1, v1 = _xv(md)
    xs, vs, _ = mr.scale(u0, v0, B["lo"], B["lengths"], MU, B["mol"], B["mass"], 0.5)
    B1 = dict(B, lengths=ln)
    assert _gap(x1, xs, B1) <= 1e-11 * ln.max() and np.abs(v1 - vs).max() <= 1e-11 * np.abs(vs).max()    # test_gpu_molecular: X_TOL, V_TOL
    if name == "tall":                                                            # a site moved by image() along z would be off by len_z
        assert np.abs(x1[:, 2] - xs[:, 2]).max() <= 1e-11 * ln.max()
    _constraints_hold(md, B1, np.float64, "%s %s after the molecular scale" % (name, kind))
    fresh = _stage_engine(E, dev, B, pos=x1, vel=v1, lengths=ln)
    for g, w in zip(_outputs(md), _outputs(fresh)):
        assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max()
    md.close()
    fresh.close()
    # The dealing of the steps to calls changes no bit of a scaled engine's run: one call of 40 against eight of 5.  (An engine
    # with a table steps in closed steps, which is what makes the dealing immaterial; the merged kicks of a bare Lennard-Jones
    # engine promise it for no box.)
    whole, dealt = _stage_engine(E, dev, B), _stage_engine(E, dev, B)
    for eng in (whole, dealt):
        eng.set_molecular_scaling_(True)
        eng.scale_box_(MU, 0.5)
    whole.step_(40, DT)
    for _ in range(8):
        dealt.step_(5, DT)
    for a, b in zip(_xv(dealt), _xv(whole)):
        assert np.array_equal(a, b)
    whole.close()
    dealt.close()


# ---------------------------------------------------------------- 6. pressure coupling on a slab
def _slab_engine(E, dev, S, atoms):
    return E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"], dev), float(S["lengths"][0]), E.LennardJonesModel(S["rc"], S["rs"]),
                            E.cu(atoms, dev), skin=S["skin"], lo=list(S["lo"]), lengths=list(S["lengths"]), periodic=list(S["periodic"]))


def _set_coupling(E, md, R, kind, seed=None):
    if kind == "crescale":
        md.set_barostat_(E.BAROSTAT_CRESCALE, R["p_ref"][0], R["beta"][0], R["tau_p"], R["every"], temperature=1.0, seed=seed)
    else:
        md.set_barostat_(E.BAROSTAT_BERENDSEN, R["p_ref"], R["beta"], R["tau_p"], R["every"],
                         coupling="semiisotropic" if kind == "semi-z0" else "anisotropic")


@pytest.mark.parametrize("kind", ["semi-z0", "aniso", "crescale"])
def test_coupling_on_a_slab_matches_the_numpy_integrator(emdee, dev, kind):
    """test_gpu_barostat.test_berendsen_trajectory_matches_the_numpy_integrator / test_crescale_... on open_cases.lj_slab with
    barostat_ref.field(..., periodic=(1, 1, 0)): the volume in P is the product of all three lengths, the open one included; box
    1e-10, positions and velocities X64 = 1e-8.  semi-z0: compressibility_z = 0 leaves len_z its bits.  That every z COORDINATE
    keeps its bits at such an event cannot be read off a run in which the atoms move, and X64 would not see an ulp: it is pinned
    by test_a_factor_of_one_leaves_the_open_axis_its_bits below, through scale_box_ -- the function every event calls -- and this
    run shows that the event's mu_z is exactly 1 (len_z keeps its bits; the reference's factors are asserted to be 1.0).  The
    dealing of the steps to calls (one of 40, eight of 5) changes no bit."""
    E = emdee
    seed = 12345
    S = oc.lj_slab(E.synthetic)
    atoms = bref.lj_atoms(S["N"])
    # the conditions on the box, before the device is touched (C-rescale's own reference needs the engine's random numbers: the
    # box, the force field and the starting pressure it shares with the Berendsen cases are checked on one of those first)
    oc.assert_coupling_conditions(oc.coupling_case(E.synthetic, "aniso" if kind == "crescale" else kind), TOL[np.float64])
    md = _slab_engine(E, dev, S, atoms)
    xi = (lambda s: float(md.langevin_normals(seed, s, torch.tensor([-1]))[0, 0])) if kind == "crescale" else None
    R = oc.coupling_case(E.synthetic, kind, xi=xi)
    mus = oc.assert_coupling_conditions(R, TOL[np.float64])
    assert (np.abs(mus - 1.0)[:, :2] >= 1e-4).all() and (np.abs(mus - 1.0) <= 1e-2).all()
    if kind == "semi-z0":
        assert (mus[:, 2] == 1.0).all() and (mus[:, 0] == mus[:, 1]).all()
    if kind == "aniso":
        assert (np.abs(mus[:, 2] - 1.0) >= 1e-4).all()                               # the open length is scaled
    builds = md.nbr_stats()["builds"]
    _set_coupling(E, md, R, kind, seed)
    md.step_(oc.COUPLING_STEPS, DT_LJ)
    ln = np.array(md.box()[1])
    x, v = _xv(md)
    gap_l, gap_x, gap_v = np.abs(ln / R["lengths"] - 1.0).max(), _gap(x, R["x"], dict(S, lengths=ln)), np.abs(v - R["v"]).max()
    print("%s: box %.2e, positions %.2e, velocities %.2e" % (kind, gap_l, gap_x, gap_v))
    assert gap_l <= 1e-10 and gap_x < X64 and gap_v < X64
    assert np.abs(x[:, 2] - R["x"][:, 2]).max() < X64                                # the open axis, no image taken out
    assert md.nbr_stats()["builds"] >= builds + oc.COUPLING_STEPS // oc.COUPLING_EVERY
    if kind == "semi-z0":
        assert ln[2] == S["lengths"][2] and md.box()[0] == list(S["lo"])
    dealt = _slab_engine(E, dev, S, atoms)
    _set_coupling(E, dealt, R, kind, seed)
    for _ in range(8):
        dealt.step_(5, DT_LJ)
    assert dealt.box() == md.box()
    for a, b in zip(_xv(dealt), (x, v)):
        assert np.array_equal(a, b)
    md.close()
    dealt.close()


@DTYPES
def test_a_factor_of_one_leaves_the_open_axis_its_bits(emdee, dev, dtype):
    """scale_box_((mu_x, mu_y, 1)) -- what a coupling event with compressibility_z = 0 does -- on a slab with atoms beyond its open
    faces: len_z, every z coordinate and every restraint reference's z keep their bits, x and y are scaled.  (Found by this test:
    lo + 1 x (z - lo) rounds twice, and in fp64 moved a third of the coordinates by an ulp per event.)"""
    E = emdee
    S = oc.pair_system(E.synthetic, "open-z", dtype)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    md = _engine(E, S, atoms, dev)
    ids = np.arange(0, S["N"], 5)
    ref = S["pos"][ids] + 0.1
    md.set_restraints_(ids, 40.0, ref=ref)
    x0, _ = _xv(md)
    md.scale_box_((1.02, 0.99, 1.0))
    x1, _ = _xv(md)
    assert md.box()[1][2] == S["lengths"][2]
    assert np.array_equal(x1[:, 2], x0[:, 2])
    assert np.abs(x1[:, :2] - x0[:, :2]).max() > 1e-3
    refs = md.restraint_refs().cpu().numpy()
    assert np.array_equal(refs[:, 2], ref[:, 2]) and np.abs(refs[:, :2] - ref[:, :2]).max() > 1e-3     # the references as the atoms
    md.close()


# ---------------------------------------------------------------- 7. molecular sums
@KINDS
def test_molecular_sums_of_rigid_water_on_open_axes(emdee, dev, kind):
    """test_gpu_molecular._check_sums on the re-boxed water: molecular_tensor_sums against molecular_ref fed the engine's own state
    (SUMS = 1e-12) and against the all-pairs sums of ortho_ref (test_gpu_virial_tensor.TOL), before and after 25 steps."""
    from .test_gpu_molecular import SUMS, TENSOR_TOL
    B = oc.stage_box("water", kind)
    oc.assert_stage_conditions(B, TOL[np.float64])
    md = _stage_engine(emdee, dev, B)
    for stage in ("start", "after 25 steps"):
        x, v = _xv(md)
        u = hr.unwrap(x, B["pairs"], B["lengths"], B["periodic"])
        f, atomic, got = _forces(md), np.array(md.tensor_sums()), np.array(md.molecular_tensor_sums())
        cw, ck = mr.corrections(u, v, f, B["mol"], B["mass"])
        scale, err = np.abs(atomic).max(), np.abs(got - (atomic - np.concatenate([cw, ck]))).max()
        print("%s %s: max |sums - reference| = %.3e of %.3e" % (kind, stage, err, scale))
        assert err <= SUMS * scale
        assert abs(got[:3].sum() - atomic[:3].sum()) > 1e-3 * abs(atomic[:3].sum())
        ref = oc.stage_total(B, u)
        Wm, Km = mr.molecular_sums(u, v, ref["f"], ref["t"], B["mol"], B["mass"])
        assert np.abs(got - np.concatenate([Wm, Km])).max() <= TENSOR_TOL[np.float64] * scale
        wrong = oc.stage_total(B, u, periodic=(1, 1, 1))
        Ww, _ = mr.molecular_sums(u, v, wrong["f"], wrong["t"], B["mol"], B["mass"])
        assert np.abs(Ww - Wm).max() >= 100 * TENSOR_TOL[np.float64] * scale
        if stage == "start":
            md.step_(25, DT, 3)
    md.close()


# ---------------------------------------------------------------- 8. minimise
def test_minimize_a_clashing_droplet(emdee, dev):
    """test_gpu_minimize.test_rigid_water_from_a_clashing_start on fire_ref.clashing_water_box re-boxed as a droplet: converged
    within three times fire_ref's own iteration count (tests/test_open_axes_host.py counts them on the CPU), the constraints
    hold, the reported g_max is numpy's projection of the engine's forces, and the energy is ortho_ref's on open axes (TOL)."""
    from .helpers import fire_ref as fr
    from .test_gpu_minimize import EPS as EPS_M
    from .test_gpu_minimize import TIGHT, WATER_FTOL
    B = oc.clashing_droplet()
    assert fr.closest_pair(B["unwrapped"], 1e9 * np.ones(3), B["excl"]) < 0.4
    right = oc.assert_stage_conditions(B, TOL[np.float64], energy=True)
    md = _stage_engine(emdee, dev, B, vel=np.zeros_like(B["pos"]))
    res = md.minimize_(3 * oc.DROPLET_ITERS, WATER_FTOL, **TIGHT)
    print(res)
    assert res.converged and res.g_max <= WATER_FTOL
    assert res.energy0 == pytest.approx(right["e"].sum(), rel=TOL[np.float64])
    _constraints_hold(md, B, np.float64, "minimised droplet")
    x, f = _xv(md)[0], _forces(md)
    u = hr.unwrap(x, B["pairs"], B["lengths"], B["periodic"])
    g = np.sqrt((fr.constrained_force(u, f, B["pairs"], B["mass"]) ** 2).sum(axis=1).max())
    back = np.sqrt((fr.constrained_force(u, f, B["pairs"][::-1], B["mass"]) ** 2).sum(axis=1).max())
    assert abs(res.g_max - g) <= 100.0 * max(abs(g - back), EPS_M * g)               # test_gpu_minimize._constrained_case
    assert res.energy < res.energy0
    assert res.energy == pytest.approx(oc.stage_total(B, u)["e"].sum(), rel=TOL[np.float64])
    md.step_(50, DT)
    _constraints_hold(md, B, np.float64, "50 steps after the minimisation")
    md.close()


# ---------------------------------------------------------------- 9. thermostats
@pytest.mark.parametrize("thermostat", ["v-rescale", "nose-hoover"])
def test_thermostatted_rigid_water_on_a_slab(emdee, dev, thermostat):
    """Ten steps of rigid water on the slab under a global thermostat, one step per call, against shake_ref.constrained_verlet fed
    the engine's own forces with thermostat_ref's event after every step (the 1e-11 bounds of _against_reference); n_dof is the
    library's own count, 6 per molecule less 3; alpha and E_th as test_gpu_thermostat holds them (1e-9)."""
    from .helpers import thermostat_ref as tr
    E = emdee
    B = oc.stage_box("water", "slab")
    oc.assert_stage_conditions(B, TOL[np.float64])
    md = _stage_engine(E, dev, B)
    n_dof = 6 * len(B["mol"]) - 3
    kT = 1.2 * 2.0 * tr.kinetic(B["vel"], B["inv_mass"]) / n_dof
    seed, chain, nsteps = 31, 3, 10
    if thermostat == "v-rescale":
        md.set_thermostat_(E.THERMOSTAT_VRESCALE, kT, 0.5 * DT, seed=seed)
        th = tr.Thermostat(tr.VRESCALE, kT, 0.5 * DT, 1, n_dof, draws=lambda s: md.thermostat_draws(seed, s, n_dof))
    else:
        md.set_thermostat_(E.THERMOSTAT_NOSE_HOOVER, kT, 4.0 * DT, chain=chain)
        th = tr.Thermostat(tr.NOSE_HOOVER, kT, 4.0 * DT, 1, n_dof, chain=chain)
    seen, offset = {}, B["pos"] - B["unwrapped"]

    def force(x, k):
        if k > 0:
            md.step_(1, DT, 3)
        return _forces(md)

    def observe(s, x, v):
        th.step += 1
        v *= th.event(tr.kinetic(v, B["inv_mass"]), DT)          # in place: constrained_verlet goes on with the scaled velocities
        gx, gv = _xv(md)
        seen[s] = (np.abs(gx - (x + offset)).max(), np.abs(gv - v).max(), np.sqrt((v * v).sum(axis=1).mean()))
    hr.constrained_verlet(B["unwrapped"], B["vel"], force, nsteps, DT, B["pairs"], B["mass"], observe=observe)
    st = md.thermostat_state()
    assert st["n_dof"] == n_dof
    alphas = np.array([e[2] for e in th.events])
    assert len(alphas) == nsteps and np.abs(alphas - 1.0).max() >= 1e-3
    for s, (ex, ev, vrms) in seen.items():
        assert ex <= 1e-11 * B["lengths"].max() and ev <= 1e-11 * vrms, (s, ex, ev)
    assert abs(st["alpha"] - alphas[-1]) <= 1e-9 and abs(st["energy"] - th.energy) <= 1e-9 * abs(th.energy)
    _constraints_hold(md, B, np.float64, "slab water, %s" % thermostat)
    md.close()


# ---------------------------------------------------------------- 10. the pull
def _pull_part(md, group, coords, n_groups):
    from .test_gpu_pull import _clear, _set
    _clear(md)
    without = _outputs(md)
    _set(md, group, coords, n_groups=n_groups)
    return [a - b for a, b in zip(_outputs(md)[:4], without[:4])]


@DTYPES
def test_pull_between_a_slab_and_a_group_beyond_its_open_face(emdee, dev, dtype):
    """Two groups separated along the open axis of open_cases' "open-z": atoms of the lower half of the slab, and the outsiders of
    the upper face with a few atoms next to it, whose centre of mass lies beyond the face.  A distance and a direction
    coordinate; planes and pull_read against pull_ref.evaluate on the positions get_state returns (tests/test_gpu_pull.py: 1e-9 /
    1e-4 of the largest entry), at the load and after 20 steps."""
    from .helpers import pull_ref as pr
    from .test_gpu_pull import DIR, DIST, U, _coord
    E = emdee
    S = oc.pair_system(E.synthetic, "open-z", dtype)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    right = oc.want(S, atoms)
    oc.assert_pair_conditions(S, atoms, right, TOL[dtype])
    N, tol = S["N"], PART[dtype]
    up, mid = S["lo"][2] + S["lengths"][2], S["lo"][2] + 0.5 * S["lengths"][2]
    group = np.full(N, -1)
    group[np.nonzero(S["pos"][:, 2] < mid)[0][::7]] = 0
    group[S["outsiders"][(2, 1)]] = 1
    group[np.nonzero((S["pos"][:, 2] > up - 1.0) & (S["pos"][:, 2] < up))[0][:4]] = 1
    mass = np.ones(N)
    R, _ = pr.centres(S["pos"], mass, group, 2)
    assert R[1][2] > up and S["lo"][2] < R[0][2] < mid                               # one centre of mass beyond the face
    fmax = np.abs(right["f"]).max()
    n = np.array([0.2, -0.3, 1.0])
    coords = [_coord(0, 1, U, DIST, fmax / 0.4 * 8, r0=np.linalg.norm(R[1] - R[0]) + 0.4, rate=0.5),
              _coord(0, 1, U, DIR, fmax / 0.3 * 8, r0=float(pr.unit(n) @ (R[1] - R[0])) - 0.3, n=n)]
    # taken as periodic, z would be folded into the box: the centre of group 1 and both coordinates move by far more than tol
    folded = oref.wrapped(S["pos"], S["lo"], S["lengths"], [1, 1, 1])
    ref0 = pr.evaluate(S["pos"], mass, group, coords, [c["r0"] for c in coords], 2)
    bad = pr.evaluate(folded, mass, group, coords, [c["r0"] for c in coords], 2)
    assert np.abs(bad["forces"] - ref0["forces"]).max() >= 100 * tol * np.abs(ref0["forces"]).max()
    md = _engine(E, S, atoms, dev)
    for stage in ("at the load", "after 20 steps"):
        got = _pull_part(md, group, coords, 2) if stage == "at the load" else None
        if got is None:
            with_p = _outputs(md)
            read = md.pull()
            xi0 = read["xi0"]
            from .test_gpu_pull import _clear, _set
            _clear(md)
            got = [a - b for a, b in zip(with_p[:4], _outputs(md)[:4])]
        else:
            read = md.pull()
            xi0 = read["xi0"]
        x = md.state(velocities=False, forces=False)["positions"].cpu().numpy().astype(np.float64)
        ref = pr.evaluate(x, mass, group, coords, xi0, 2)
        for what, g, key in zip(("forces", "energies", "virials", "tensors"), got, ("forces", "energies", "virials", "tensors")):
            err = np.abs(g - ref[key]).max() / np.abs(ref[key]).max()
            print("pull %s %s, %s: max error / max entry = %.3e (bound %.0e)" % (np.dtype(dtype).name, stage, what, err, tol))
            assert err <= tol, (stage, what)
        for q, key in enumerate(("xi", "xi0", "f", "U")):
            assert np.abs(read[key] - ref["words"][:, q]).max() <= tol * np.abs(ref["words"][:, q]).max(), key
        assert np.abs(read["D"] - ref["words"][:, 5:8]).max() <= tol * np.abs(ref["words"][:, 5:8]).max()
        assert np.abs(read["centres"] - ref["centres"]).max() <= tol * np.abs(ref["centres"]).max()
        assert read["centres"][1][2] > S["lo"][2] + S["lengths"][2]
        assert 0.1 * fmax <= np.abs(ref["forces"]).max() <= 10.0 * fmax
        if stage == "at the load":
            md.step_(20, DT_LJ)
            assert md.nbr_stats()["builds"] >= 2
    md.close()


@DTYPES
def test_two_atoms_across_an_open_face_follow_the_numpy_velocity_verlet(emdee, dev, dtype):
    """test_gpu_pull.test_two_atoms_follow_the_numpy_velocity_verlet with the pair lying along the open z of a slab at lo != 0, the
    second atom 2.5 beyond the upper face: the umbrella is their only force; TOL of the amplitudes over 200 steps."""
    from .helpers import pull_ref as pr
    from .test_gpu_pull import DIST, U, _coord, _set
    E = emdee
    lo, L = np.array([-3.7, 1.9, 11.3]), np.array([12.0, 12.0, 6.0])
    axis = pr.unit([0.2, -0.1, 1.0])
    pos = np.array([lo + [1.5, 1.0, 4.5], lo + [1.5, 1.0, 4.5] + 4.0 * axis])
    assert pos[1, 2] > lo[2] + L[2] + 2.0 and 4.0 * axis[2] > 0.5 * L[2]             # beyond the face, and more than half of len_z apart
    vel = np.array([[0.05, -0.02, 0.03], [-0.01, 0.04, 0.02]])
    mass, group = np.array([1.0, 3.0]), np.array([0, 1])
    coords = [_coord(0, 1, U, DIST, 20.0, r0=3.7, rate=0.35)]
    md = E.VelocityVerlet(E.cu(pos.astype(dtype), dev), E.cu(vel.astype(dtype), dev), float(L[0]), E.LennardJonesModel(2.5, 2.0),
                          E.cu(E.lennard_jones_atoms(1.0, 1.0, 2), dev), skin=0.3, inv_mass=E.cu((1.0 / mass).astype(dtype), dev), lo=list(lo),
                          lengths=list(L), periodic=[1, 1, 0])
    _set(md, group, coords)
    md.step_(200, DT_LJ)
    p, w = pos.astype(dtype).astype(np.float64), vel.astype(dtype).astype(np.float64)
    x, v, xi0, work, fs, (amp_x, amp_v) = pr.verlet(p, w, mass, group, coords, 2, DT_LJ, 200)
    gx, gv = _xv(md)
    ex, ev = np.abs(gx - x).max(), np.abs(gv - v).max()
    print("%s: max |dx| = %.3e (amplitude %.3f), max |dv| = %.3e (amplitude %.3f)" % (np.dtype(dtype).name, ex, amp_x, ev, amp_v))
    assert amp_x > 0.1 and ex <= PART[dtype] * amp_x and ev <= PART[dtype] * amp_v
    read = md.pull()
    assert read["xi0"][0] == pr.advance(3.7, 0.35, DT_LJ, 200) == xi0[0]
    assert abs(read["work"][0] - work[0]) <= PART[dtype] * np.abs(pr.work_rule(fs[:, 0], 0.35, DT_LJ)).max()
    md.close()
