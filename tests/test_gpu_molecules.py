"""GPU tests of whole-molecule pressure and scaling (include/emdee_hip.h: emdee_md_set_molecules; csrc/molecule.hpp) against the
numpy yardstick of tests/helpers/molecule_ref.py: constant pressure for an engine with hbonds clusters, rigid waters and bonds.

One box for most of them (molecule_ref.molecule_box): shake_ref.mixed_box -- 1180 atoms, 300 star clusters, 60 rigid waters, 100
free atoms, sides (9.0, 9.6, 10.5) -- with every constraint group whole, dealt to molecules of 1, 2, 3, 4, 8, 9, 63, 64, 65 and 129
atoms (the small / large class boundary of the table, the edges of the wavefront loop, two trips) plus one molecule per remaining
cluster and water; 1096 entries, five blocks of the reduction.  Three molecules are loaded whole box lengths away, groups stick
out of the faces, harmonic bonds tie cluster centres inside the large molecules.

Bounds are those of the files that own them: SUMS, X_TOL, V_TOL, FRESH and the Berendsen setting of tests/test_gpu_molecular.py, the
all-pairs TOL of tests/test_gpu_virial_tensor.py, H and FD_BOUND of tests/test_molecular_ref_host.py, the constraint bounds of
tests/test_gpu_hbonds.py.  Where a Float32 engine has no bound there, the bound is worked out next to its assertion."""
import ctypes as C

import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import molecular_ref as mr
from .helpers import molecule_ref as gr
from .helpers import ortho_ref as oref
from .helpers import settle_ref as sr
from .helpers import shake_ref as hr
from .test_gpu_dd_pairs import _build
from .test_gpu_hbonds import DT, ERR_INVALID, ERR_STATE, _constraints_hold, _forces, _refused, _xv
from .test_gpu_molecular import BETA, EVERY, FRESH, MU, P_REF, SUMS, TAU_P, V_TOL, X_TOL
from .test_gpu_molecular import _engine as _water_engine
from .test_gpu_virial_tensor import TOL as TENSOR_TOL
from .test_molecular_ref_host import FD_BOUND, H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NSTEPS = 20                                             # tests/test_gpu_molecular.py: the Berendsen trajectories
VSCALE = 0.97


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _engine(E, dev, B, dtype=np.float64, pos=None, vel=None, lengths=None, ids="box", switch=True, hbonds=True, rigid=True, terms=None,
            mass=None, excl=True, atoms=None):
    """the molecule box (or another state on another box) with exclusions, bonds, both constraint tables, the molecule table and the
    switch; ids None: no molecule table; excl False: neither exclusions nor bonds (a state of another atom count can be loaded)"""
    mass = B["mass"] if mass is None else mass
    with np.errstate(divide="ignore"):
        im = E.cu((1.0 / mass).astype(dtype), dev)
    lengths = [float(t) for t in (hr.LENGTHS if lengths is None else lengths)]
    md = E.VelocityVerlet(E.cu(np.asarray(B["pos"] if pos is None else pos).astype(dtype), dev),
                          E.cu(np.asarray(B["vel"] if vel is None else vel).astype(dtype), dev), lengths[0], E.LennardJonesModel(hr.RC, hr.RS),
                          E.cu(B["atoms"] if atoms is None else atoms, dev), skin=hr.SKIN, inv_mass=im, lo=list(hr.LO), lengths=lengths, periodic=[1, 1, 1])
    if excl:
        md.set_exclusions_(B["excl"])
        _, bonds, params = (B["terms"] if terms is None else terms)[0]
        md.set_bonded_(E.HARMONIC_BOND, bonds, params)
    if hbonds:
        md.set_hbonds_(B["clusters"], B["dist"])
    if rigid:
        md.set_rigid3_(B["mol"], B["geom"])
    if ids is not None:
        md.set_molecules_(B["ids"] if isinstance(ids, str) else ids)
    if switch:
        md.set_molecular_scaling_()
    return md


def _unwrapped(md, lengths):
    """the unwrapped coordinates as the molecular kernels form them.  fp64: what get_state returns, bit for bit.  fp32 (absolute
    records: the state has masses): the record, as pack_positions returns it, plus the image counts times the engine's fp32 box
    length, added in double -- get_state's own sum is rounded to fp32 once more."""
    x, v = _xv(md)
    if md.dtype == torch.float64:
        return x, v
    ids = torch.arange(x.shape[0], dtype=torch.int32, device=md.device)
    rec = md.pack_positions(ids, [0.0, 0.0, 0.0]).cpu().numpy().astype(np.float64)
    l32 = np.asarray(lengths, dtype=np.float32).astype(np.float64)
    return rec + np.rint((x - rec) / l32) * l32, v


def _masses(B, dtype):
    """the masses as the engine holds them: 1 / inv_mass, with inv_mass rounded to the engine's precision"""
    return 1.0 / (1.0 / B["mass"]).astype(dtype).astype(np.float64)


def _all_pairs(B, u, lengths, terms=None):
    return oref.total(oref.wrapped(u, hr.LO, lengths, [1, 1, 1]), hr.LO, np.asarray(lengths), [1, 1, 1], hr.RC, hr.RS, B["atoms"],
                      terms=B["terms"] if terms is None else terms, excl=B["excl"])


def _check_sums(md, B, ids, lengths, dtype, what, allpairs=True):
    u, v = _unwrapped(md, lengths)
    f = _forces(md)
    atomic = np.array(md.tensor_sums())
    got = np.array(md.molecular_tensor_sums())
    mass = _masses(B, dtype)
    cw, ck = gr.corrections(u, v, f, ids, mass)
    want = atomic - np.concatenate([cw, ck])
    scale, err = np.abs(atomic).max(), np.abs(got - want).max()
    print("%s: max |sums - reference| = %.3e, largest component %.3e (bound %.0e relative); tr W_mol = %.4f, tr W = %.4f"
          % (what, err, scale, SUMS, got[:3].sum(), atomic[:3].sum()))
    assert err <= SUMS * scale, (what, err, scale)
    assert abs(got[:3].sum() - atomic[:3].sum()) > 1e-3 * abs(atomic[:3].sum())   # (the two formulations differ)
    if allpairs:
        ref = _all_pairs(B, u, lengths)
        Wm, Km = gr.molecular_sums(u, v, ref["f"], ref["t"], ids, mass)
        err = np.abs(got - np.concatenate([Wm, Km])).max()
        print("%s: against the all-pairs sums %.3e (bound %.0e relative)" % (what, err, TENSOR_TOL[dtype]))
        assert err <= TENSOR_TOL[dtype] * scale
    return got


# ---------------------------------------------------------------- 1. the molecular sums (and 8.: Float32)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_molecular_sums_over_molecules_of_every_size_class(emdee, dev, dtype):
    B = gr.molecule_box()
    md = _engine(emdee, dev, B, dtype, terms=gr.strained_terms(B))
    B["terms"] = gr.strained_terms(B)                                        # (bonds that pull: exclusions and bonds are in force)
    md.profile_(True)
    name = np.dtype(dtype).name
    _check_sums(md, B, B["ids"], hr.LENGTHS, dtype, name + ", start")
    assert md.kernel_time("molecular")[1] == 2                               # (index 10: the centres, then the entries' pass)
    md.step_(10, DT, 3)                                                      # (slots are permuted, atoms cross faces)
    _check_sums(md, B, B["ids"], hr.LENGTHS, dtype, name + ", after 10 steps", allpairs=False)
    md.close()


# ---------------------------------------------------------------- 2. the virial theorem on the device
def test_trace_of_the_molecular_virial_is_the_engines_own_volume_derivative(emdee, dev):
    """What catches a wrong image of Y or a wrong d_k: U at mu = 1 +- h from the engine's own scale_box_ and energies, on fresh
    engines, against -tr W_mol of a third."""
    B = gr.molecule_box()
    terms = gr.strained_terms(B)
    md = _engine(emdee, dev, B, terms=terms)
    trace = sum(md.molecular_tensor_sums()[:3])
    atomic = sum(md.tensor_sums()[:3])
    md.close()
    U = []
    for mu in (1.0 + H, 1.0 - H):
        md = _engine(emdee, dev, B, terms=terms)
        md.scale_box_(mu)
        assert np.abs(np.array(md.box()[1]) / hr.LENGTHS - mu).max() <= 1e-15
        U.append(md.totals()[0])
        md.close()
    fd = -(U[0] - U[1]) / (2.0 * H)
    gap = abs(fd - trace) / abs(trace)
    print("tr W_mol = %.4f (tr W = %.4f), -dU/dmu through scale_box_ and totals() = %.4f: relative difference %.3e (bound %.2e)"
          % (trace, atomic, fd, gap, FD_BOUND))
    assert gap <= FD_BOUND
    assert abs(fd - atomic) > 100.0 * FD_BOUND * abs(trace)                  # (the atomic virial is not this derivative)


# ---------------------------------------------------------------- 3. the scale (and 8.: Float32)
def _intramolecular(B, x):
    return [np.linalg.norm(x[a][:, None] - x[a][None], axis=2) for a in B["members"].values()]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_molecular_scale_translates_whole_molecules(emdee, dev, dtype):
    E = emdee
    B = gr.molecule_box()
    f32 = dtype == np.float32
    name = np.dtype(dtype).name
    md = _engine(E, dev, B, dtype)
    md.profile_(True)
    x0, v0 = _xv(md)
    u0, _ = _unwrapped(md, hr.LENGTHS)
    builds = md.nbr_stats()["builds"]
    md.scale_box_(MU, VSCALE)
    assert md.kernel_time("molecular")[1] == 2                               # (the centres, the shift)
    ln = np.array(md.box()[1])
    assert np.array_equal(ln, MU * hr.LENGTHS) and md.box()[0] == list(hr.LO) and md.nbr_stats()["builds"] > builds
    x1, v1 = _xv(md)
    xr, vr, lr = gr.scale(u0, v0, hr.LO, hr.LENGTHS, MU, B["ids"], _masses(B, dtype), VSCALE)
    ex, ev, vrms = np.abs(x1 - xr).max(), np.abs(v1 - vr).max(), np.sqrt((v0 * v0).sum(axis=1).mean())
    ulp_x, ulp_v = float(np.spacing(np.float32(np.abs(x1).max()))), float(np.spacing(np.float32(np.abs(v1).max())))
    # fp32: tests/test_gpu_molecular.py's count for positions -- the record rounded once, get_state once more, and the image counts
    # times an fp32 box length -- 2 ulp_fp32 of the largest coordinate; a velocity is rounded once when it is stored: 1 ulp_fp32
    bx, bv = (2.0 * ulp_x, ulp_v) if f32 else (X_TOL * hr.LENGTHS.max(), V_TOL * vrms)
    print("%s: max |dx| = %.3e (bound %.3e), max |dv| = %.3e (bound %.3e)" % (name, ex, bx, ev, bv))
    assert ex <= bx and ev <= bv
    # (positions read through get_state, each off by up to half an ulp_fp32 of the largest coordinate -- the far molecules': the
    # `relative` allowance of tests/test_gpu_hbonds.py; the records themselves cannot be unwrapped with the lengths of that file here)
    _constraints_hold(md, B, B["pairs"], dtype, name + ", scaled", relative=f32)
    # every distance inside every molecule of the size classes, the 129-atom one and the ones loaded boxes away included: two
    # coordinates, each rounded when it was stored and when it was read, before and after -- 4 ulp of the largest coordinate
    ulp = ulp_x if f32 else float(np.spacing(np.abs(x1).max()))
    worst = max(np.abs(a - b).max() for a, b in zip(_intramolecular(B, x0), _intramolecular(B, x1)))
    print("%s: largest change of an intramolecular distance %.3e (bound %.3e)" % (name, worst, 4.0 * ulp))
    assert worst <= 4.0 * ulp
    assert np.abs(x1 - x0).max() > 0.02                                      # (something moved)
    fresh = _engine(E, dev, B, dtype, pos=x1, vel=v1, lengths=ln)
    f, ff = _forces(md), _forces(fresh)
    print("%s: forces against a fresh engine %.3e of %.3e" % (name, np.abs(f - ff).max(), np.abs(ff).max()))
    assert np.abs(f - ff).max() <= FRESH[dtype] * np.abs(ff).max()
    fresh.close()
    raw = md.state(forces=False)["velocities"].cpu().numpy()
    md.scale_box_(1.0 / MU)                                                  # velocity_scale = 1: the planes bit for bit
    assert np.array_equal(md.state(forces=False)["velocities"].cpu().numpy(), raw)
    md.step_(3, DT)
    _constraints_hold(md, B, B["pairs"], dtype, name + ", scaled there and back, 3 steps", relative=f32)
    md.close()


# ---------------------------------------------------------------- 4. NPT trajectories
def _coupled_against_reference(E, dev, B, kind, coupling, what, crescale=None):
    """tests/test_gpu_molecular.py's comparison for this box: the engine, one step per call, against
    molecule_ref.coupled_constrained_verlet fed the engine's forces."""
    md = _engine(E, dev, B)
    if kind == bref.BERENDSEN:
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY, coupling="anisotropic")
    else:
        md.set_barostat_(E.BAROSTAT_CRESCALE, P_REF[0], BETA[0], TAU_P, EVERY, temperature=crescale[0], seed=crescale[1])
    held, boxes, seen = {}, {0: np.array(md.box()[1])}, {}

    def force(x, ln, k):
        if k <= 0:
            return _forces(md)
        if k % EVERY == 0:
            # the step of an event: the engine's forces and atomic virial BEFORE the event are gone once the call returns, so a
            # second engine -- the same tables, no coupling -- takes the same step from the engine's own state first
            gx, gv = _xv(md)
            twin = _engine(E, dev, B, pos=gx, vel=gv, lengths=md.box()[1], ids=None, switch=False)
            twin.step_(1, DT)
            held[k] = np.array(twin.tensor_sums()[:6])
            f = _forces(twin)
            twin.close()
        md.step_(1, DT)
        boxes[k] = np.array(md.box()[1])
        return f if k % EVERY == 0 else _forces(md)

    def observe(s, x, v, ln):
        assert ln.min() > 2.0 * (hr.RC + hr.SKIN)                            # (the reference's box stays legal: 5.8)
        gx, gv = _xv(md)
        seen[s] = (np.abs(gx - x).max(), np.abs(gv - v).max(), np.sqrt((v * v).sum(axis=1).mean()), np.abs(boxes[s] - ln).max())

    xi = None if crescale is None else (lambda count: float(md.langevin_normals(crescale[1], count, torch.tensor([-1]))[0, 0]))
    x, v, ln, events = gr.coupled_constrained_verlet(B["unwrapped"], B["vel"], force, lambda x, ln, s: held[s], NSTEPS, DT, B["pairs"], B["ids"],
                                                     B["mass"], hr.LO, hr.LENGTHS, kind, P_REF, BETA, TAU_P, EVERY, coupling,
                                                     temperature=None if crescale is None else crescale[0], xi=xi, observe=observe)
    assert len(events) == NSTEPS // EVERY
    for s, P, mu, vs in events:
        got = boxes[s] / boxes[s - 1]
        print("%s, event at step %d: P_mol = %s, mu = %s, engine's mu off by %.3e" % (what, s, P, mu, np.abs(got - mu).max()))
        assert (np.abs(mu - 1.0) > 1e-6).all() and np.abs(got - mu).max() <= X_TOL
    for s in sorted(seen):
        ex, ev, vrms, el = seen[s]
        if s in (1, EVERY, NSTEPS):
            print("%s, step %d: max |dx| = %.3e, max |dv| = %.3e (rms velocity %.3f), box %.3e" % (what, s, ex, ev, vrms, el))
        assert ex <= X_TOL * hr.LENGTHS.max() and ev <= V_TOL * vrms and el <= X_TOL * hr.LENGTHS.max(), (what, s, ex, ev, el)
    _constraints_hold(md, B, B["pairs"], np.float64, what)
    return md


def test_berendsen_trajectory_with_clusters_waters_and_molecules_matches_the_reference(emdee, dev):
    md = _coupled_against_reference(emdee, dev, gr.molecule_box(), bref.BERENDSEN, bref.ANISOTROPIC, "Berendsen anisotropic")
    assert len(set(np.round(np.array(md.box()[1]) / hr.LENGTHS, 9))) == 3
    md.close()


def test_crescale_trajectory_matches_the_reference(emdee, dev):
    md = _coupled_against_reference(emdee, dev, gr.molecule_box(), bref.CRESCALE, bref.ISOTROPIC, "C-rescale", crescale=(1.0, 12345))
    md.close()


@pytest.mark.parametrize("coupling", ["isotropic", "semiisotropic"])
def test_the_other_berendsen_couplings_are_accepted_and_keep_the_constraints(emdee, dev, coupling):
    B = gr.molecule_box()
    md = _engine(emdee, dev, B)
    md.set_barostat_(emdee.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY, coupling=coupling)
    md.step_(2 * EVERY, DT)
    r = np.array(md.box()[1]) / hr.LENGTHS
    assert (np.abs(r - 1.0) > 1e-6).all() and abs(r[0] - r[1]) <= 4e-15 and ((abs(r[0] - r[2]) <= 4e-15) == (coupling == "isotropic"))
    _constraints_hold(md, B, B["pairs"], np.float64, "Berendsen " + coupling)
    md.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_states_of_a_coupled_engine_do_not_depend_on_the_dealing(emdee, dev, dtype):
    E = emdee
    B = gr.molecule_box()
    out = []
    for deal in ((40,), (5,) * 8, (1,) * 40, (40,)):
        md = _engine(E, dev, B, dtype)
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY, coupling="anisotropic")
        md.profile_(True)
        for n in deal:
            md.step_(n, DT)
        assert md.kernel_time("molecular")[1] == 4 * (40 // EVERY)           # (centres + sums, centres + shift per event)
        st = md.state(forces=False)
        out.append((st["positions"].cpu().numpy(), st["velocities"].cpu().numpy(), np.array(md.box()[1])))
        if deal == (40,) and len(out) == 1:
            _constraints_hold(md, B, B["pairs"], dtype, "%s, 40 coupled steps" % np.dtype(dtype).name, relative=dtype == np.float32)
        md.close()
    assert (out[0][2] != hr.LENGTHS).all()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    if dtype == np.float32:
        # 8.: the Float32 run against the Float64 run's box.  A factor is 1 - c (p_ref - P) with c (p_ref - P) about 1e-3 per event
        # (tests/test_gpu_molecular.py's setting); the fp32 engine's P rests on forces good to FRESH[float32] = 1e-4 relative, so a
        # factor is good to about 1e-7 and eight of them to 1e-6 of a side
        md = _engine(E, dev, B, np.float64)
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY, coupling="anisotropic")
        md.step_(40, DT)
        gap = np.abs(out[0][2] / np.array(md.box()[1]) - 1.0).max()
        print("float32 box against float64 box after 8 events: %.3e (bound 1e-6)" % gap)
        assert gap <= 1e-6
        md.close()


# ---------------------------------------------------------------- 5. both paths on water
def test_the_general_path_agrees_with_the_triangle_path_on_water(emdee, dev):
    """A rigid-only box and a table that names exactly the waters.  The two paths are NOT bitwise equal: the Triangle path sums per
    molecule and then over molecules, the general path over entries, and the centres are formed in another order."""
    B = sr.water_box()
    ids = np.full(B["pos"].shape[0], -1)
    ids[B["mol"]] = np.arange(len(B["mol"]))[:, None]
    pos = sr.unwrap(B["pos"], B["mol"], sr.LENGTHS)                          # (loaded whole)
    out = []
    for table in (False, True):
        md = _water_engine(emdee, dev, dict(B, pos=pos))
        md.set_molecular_scaling_()
        if table:
            md.set_molecules_(ids)
        md.profile_(True)
        sums = np.array(md.molecular_tensor_sums())
        assert md.kernel_time("molecular")[1] == (2 if table else 1)         # (which path ran)
        md.scale_box_(MU, VSCALE)
        out.append((sums,) + _xv(md))
        md.close()
    (s0, x0, v0), (s1, x1, v1) = out
    scale, vrms = np.abs(np.array(s0)).max(), np.sqrt((v0 * v0).sum(axis=1).mean())
    print("general against Triangle: sums %.3e of %.3e, positions %.3e, velocities %.3e" % (np.abs(s1 - s0).max(), scale, np.abs(x1 - x0).max(),
                                                                                              np.abs(v1 - v0).max()))
    assert np.abs(s1 - s0).max() <= SUMS * scale
    assert np.abs(x1 - x0).max() <= X_TOL * sr.LENGTHS.max() and np.abs(v1 - v0).max() <= V_TOL * vrms


# ---------------------------------------------------------------- 6. nothing changes without a table
def test_a_table_set_and_cleared_leaves_the_rigid_path_bit_for_bit_and_launch_for_launch(emdee, dev):
    E = emdee
    B = sr.water_box()
    pos = sr.unwrap(B["pos"], B["mol"], sr.LENGTHS)
    ids = np.full(pos.shape[0], -1)
    ids[B["mol"]] = np.arange(len(B["mol"]))[:, None]
    out = []
    for touched in (True, False):
        md = _water_engine(E, dev, dict(B, pos=pos))
        md.profile_(True)
        md.set_molecular_scaling_()
        if touched:
            md.set_molecules_(ids)
            md.set_molecules_(None)
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY, coupling="anisotropic")
        md.step_(NSTEPS, DT)
        out.append(_xv(md) + (np.array(md.box()[1]), md.kernel_time("molecular")[1]))
        md.close()
    assert out[0][3] == out[1][3] == 2 * (NSTEPS // EVERY)                   # (tests/test_gpu_molecular.py: one sum and one scale per event)
    for a, b in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(a, b)


def test_with_every_atom_at_minus_one_the_entries_are_the_atomic_ones_bit_for_bit(emdee, dev):
    B = gr.molecule_box()
    out = []
    for table in (True, False):
        md = _engine(emdee, dev, B, ids=np.full(B["pos"].shape[0], -1) if table else None, switch=table, hbonds=False, rigid=False)
        assert md.molecular_tensor_sums() == md.tensor_sums()
        md.scale_box_(MU, VSCALE)
        st = md.state()
        out.append([st[k].cpu().numpy() for k in ("positions", "velocities", "forces")] + [np.array(md.box()[1])])
        md.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 7. refusals and lifecycle
def _call_set(E, md, ptr, n):
    return E._lib.call("emdee_md_set_molecules", md._handle, ptr, n)


def test_refusals_name_the_molecule_the_group_and_the_atoms(emdee, dev):
    E = emdee
    B = gr.molecule_box()
    N = B["pos"].shape[0]
    md = _engine(E, dev, B, ids=None, switch=False)
    good = torch.as_tensor(B["ids"], dtype=torch.int32, device=dev)
    # the count and the pointer
    text = _refused(E, ERR_INVALID, _call_set, E, md, C.c_void_p(good.data_ptr()), N - 1)
    assert str(N - 1) in text and str(N) in text
    _refused(E, ERR_INVALID, _call_set, E, md, None, N)
    _refused(E, ERR_INVALID, _call_set, E, md, C.c_void_p(good.data_ptr()), -1)
    # an id below -1
    bad = B["ids"].copy(); bad[17] = -2
    text = _refused(E, ERR_INVALID, md.set_molecules_, bad)
    assert "atom 17" in text and "-2" in text
    # a cluster split, a water split, a cluster left at -1: the group, its atoms and the molecules are named
    c = B["clusters"][5]
    bad = B["ids"].copy(); bad[c[1]] = 999999
    text = _refused(E, ERR_INVALID, md.set_molecules_, bad)
    assert "hbonds cluster 5" in text and "atom %d" % c[1] in text and "999999" in text and "emdee_md_set_hbonds" in text
    w = B["mol"][7]
    bad = B["ids"].copy(); bad[w[2]] = 999999
    text = _refused(E, ERR_INVALID, md.set_molecules_, bad)
    assert "rigid molecule 7" in text and "%d %d %d" % tuple(w) in text and "emdee_md_set_rigid3" in text
    bad = B["ids"].copy(); bad[[a for a in c if a >= 0]] = -1
    text = _refused(E, ERR_INVALID, md.set_molecules_, bad)
    assert "hbonds cluster 5" in text and "-1" in text
    # an hbonds engine without a table, and with a table but the switch off, keeps its three refusals, texts included
    for with_table in (False, True):
        if with_table:
            md.set_molecules_(B["ids"])
        for call, args in ((md.scale_box_, (1.001,)), (md.set_barostat_, (E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)), (md.molecular_tensor_sums, ())):
            text = _refused(E, ERR_STATE, call, *args)
            assert "hbonds table" in text and "three-site molecules" in text
    # the switch on: all lifted; then clearing the table or the switch under a barostat is refused, and both stay
    md.set_molecular_scaling_()
    md.molecular_tensor_sums()
    md.scale_box_(1.001)
    md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY, coupling="anisotropic")
    text = _refused(E, ERR_STATE, md.set_molecules_, None)
    assert "emdee_md_set_hbonds" in text and "coupling" in text
    text = _refused(E, ERR_STATE, md.set_molecular_scaling_, False)
    assert "rigid molecules" in text and "coupling" in text                 # (the rule and the text of the rigid table, which this engine holds too)
    md.set_hbonds_(B["clusters"], B["dist"])                                 # (accepted while a barostat is on)
    before = md.box()[1]
    md.step_(EVERY, DT)
    assert md.box()[1] != before
    md.set_barostat_(None)
    # the mirror refusals: a constraint table that the molecule table in force splits, or leaves at -1
    j = next(k for k in range(6, len(B["clusters"])) if B["ids"][B["clusters"][k, 0]] != B["ids"][c[0]])   # (a cluster of another molecule)
    clusters = B["clusters"].copy()
    clusters[5, 1] = B["clusters"][j, 0]
    clusters = np.delete(clusters, j, axis=0)
    text = _refused(E, ERR_INVALID, md.set_hbonds_, clusters, np.delete(B["dist"], j, axis=0))
    assert "hbonds cluster 5" in text and "molecule table" in text and "atom %d" % B["clusters"][j, 0] in text
    free = np.flatnonzero(B["ids"] == -1)[:3]
    md.set_rigid3_(None, None)
    text = _refused(E, ERR_INVALID, md.set_rigid3_, np.concatenate([B["mol"], free[None]]), np.concatenate([B["geom"], B["geom"][:1]]))
    assert "rigid molecule %d" % len(B["mol"]) in text and "atom %d" % free[0] in text and "-1" in text
    md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY)         # (hbonds clusters alone: the same rule, its own text)
    text = _refused(E, ERR_STATE, md.set_molecular_scaling_, False)
    assert "hbonds table" in text and "coupling" in text and "emdee_md_set_hbonds" in text
    md.set_barostat_(None)
    md.set_rigid3_(B["mol"], B["geom"])
    # after all refusals the engine still steps and its constraints hold
    md.step_(3, DT)
    _constraints_hold(md, B, B["pairs"], np.float64, "after the refusals")
    md.close()


def _wrapped_atom_by_atom(B):
    """The common mistake: every atom folded into the box on its own.  shake_ref.mixed_box()["pos"] is such a state, but its lattice
    keeps every group clear of the box faces (checked here: loaded as it is, it IS whole), so the state is moved by half a lattice
    spacing first; then groups do straddle faces."""
    W = hr.mixed_box()
    i, j, d = B["pairs"][:, 0].astype(int), B["pairs"][:, 1].astype(int), B["pairs"][:, 2]
    broken = lambda x: int((np.abs(np.linalg.norm(x[i] - x[j], axis=1) - d) > 1e-3 * d).sum())
    assert broken(W["pos"]) == 0
    x = hr.LO + np.mod(W["unwrapped"] + 0.5 * hr.LENGTHS / 8.0 - hr.LO, hr.LENGTHS)
    assert broken(x) >= 10
    return x


def test_a_state_wrapped_atom_by_atom_and_a_massless_molecule_are_refused(emdee, dev):
    E = emdee
    B = gr.molecule_box()
    wrapped = _wrapped_atom_by_atom(B)
    whole = _engine(E, dev, B, pos=hr.mixed_box()["pos"])                    # (mixed_box as it is: no group across a box face, accepted)
    whole.close()
    md = _engine(E, dev, B, pos=wrapped, ids=None, switch=False)
    text = _refused(E, ERR_STATE, md.set_molecules_, B["ids"])
    assert "not loaded whole" in text and "molecule" in text and "atoms" in text
    md.set_molecular_scaling_()
    _refused(E, ERR_STATE, md.scale_box_, 1.001)                             # (no table came into force)
    md.step_(2, DT)
    md.close()
    free = np.flatnonzero(B["ids"] == -1)[:2]
    mass = B["mass"].copy(); mass[free] = np.inf                              # (inv_mass = 0)
    ids = B["ids"].copy(); ids[free] = 424242
    md = _engine(E, dev, B, ids=None, switch=False, mass=mass)
    text = _refused(E, ERR_STATE, md.set_molecules_, ids)
    assert "molecule 424242" in text and "%d %d" % tuple(free) in text and "mass is 0" in text
    md.set_molecules_(B["ids"])                                              # (the same atoms as molecules of one: fine)
    md.close()


def test_the_table_survives_a_state_of_the_same_count_and_goes_stale_after_another(emdee, dev):
    E = emdee
    B = gr.molecule_box()
    N = B["pos"].shape[0]
    ghostly = B["atoms"].copy()
    ghostly["twice_sqrt_eps"] = 0.0                                          # (tests/test_gpu_molecular.py: the rules of the table alone)
    md = _engine(E, dev, B, hbonds=False, rigid=False, excl=False, atoms=ghostly)
    before = np.array(md.molecular_tensor_sums())
    state = lambda n, pos, at=ghostly: (E.cu(pos[:n], dev), E.cu(B["vel"][:n], dev), E.cu(at[:n], dev), E.cu(1.0 / B["mass"][:n], dev))
    md.set_state_(*state(N, B["pos"]))
    assert np.abs(np.array(md.molecular_tensor_sums()) - before).max() <= SUMS * np.abs(before).max()
    assert np.abs(before - np.array(md.tensor_sums())).max() > 1e-3 * np.abs(before).max()      # (the table is in use)
    md.set_state_(*state(N - 3, B["pos"]))
    for call, args in ((md.step_, (1, DT)), (md.scale_box_, (1.001,)), (md.molecular_tensor_sums, ())):
        text = _refused(E, ERR_STATE, call, *args)
        assert "emdee_md_set_molecules" in text and str(N) in text and str(N - 3) in text
    md.set_molecules_(None)
    md.step_(2, DT)
    md.close()
    # a state of the same count that is not whole: refused at the set_state, and the engine waits for a table that fits
    full = _engine(E, dev, B)
    wrapped = _wrapped_atom_by_atom(B)
    text = _refused(E, ERR_STATE, full.set_state_, *state(N, wrapped, B["atoms"]))
    assert "not loaded whole" in text
    _refused(E, ERR_STATE, full.step_, 1, DT)
    full.set_state_(*state(N, B["pos"], B["atoms"]))
    full.step_(2, DT)
    _constraints_hold(full, B, B["pairs"], np.float64, "after a state that did not fit")
    full.close()


def test_no_state_and_a_lent_engine_refuse(emdee, dev):
    E = emdee
    ctx = E.context_for(dev)
    h = C.c_void_p()
    three = lambda *v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", ctx.handle, three(*hr.LO), three(*hr.LENGTHS), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(E.LennardJonesModel(hr.RC, hr.RS)), hr.SKIN, 8, C.byref(h))
    ids = torch.zeros(4, dtype=torch.int32, device=dev)
    _refused(E, ERR_STATE, E._lib.call, "emdee_md_set_molecules", h, C.c_void_p(ids.data_ptr()), 4)
    E._lib.call("emdee_md_destroy", h)
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)
    pos = pos[np.argsort(gid)]
    n = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((n, 3)), E.lennard_jones_atoms(1.0, 1.0, n), float(lengths[0]))
    eng = dd.engine(0)
    text = _refused(E, ERR_STATE, eng.set_molecules_, np.zeros(eng.n_owned, dtype=np.int32))
    assert "emdee_dd_engine" in text
    dd.step_(2, 0.005)
    dd.close()
