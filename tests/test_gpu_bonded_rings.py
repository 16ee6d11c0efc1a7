"""GPU tests of the bonded terms on real topologies and at singular geometries (include/emdee_hip.h, "bonded terms"): the
fused-ring solute of the force-field fixture in flexible water, small rings, branches, improper-style torsions and several terms
on one quadruple, and the exactly and nearly singular geometries of tests/test_bonded_terms_host.py on the device.  The
yardstick is tests/helpers/bonded_ref.py.  In boxes of atoms with epsilon = 0 the outputs are the bonded terms alone, and each
atom is compared at its own scale under the rounding model of tests/helpers/ring_cases.py, with the C measured on the host."""
import os

import numpy as np
import pytest

from .conftest import GOLDEN
from .helpers import bonded_ref as br
from .helpers import ring_cases as rc
from .test_gpu_bonded import _check_bonded_part, _chains, _box, _md, _numpy_verlet, _outputs, _reference
from .test_gpu_dd_pairs import _compare, _gather, _lj14scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

XML = os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml")
RC_NM, RS_NM, SKIN_NM = 0.8, 0.7, 0.1
DTYPES = {"f64": torch.float64, "f32": torch.float32}
CHAIN_ENTRIES = 6                                                # the most term entries an atom of test_gpu_bonded's chains owns


@pytest.fixture(scope="module")
def solutes(emdee):
    return {pucker: rc.solute_box(emdee, XML, pucker=pucker) for pucker in (False, True)}


def _held(md):
    """the positions the engine holds (an fp32 engine keeps them on its own grid), as float64"""
    return md.state(velocities=False, forces=False)["positions"].cpu().numpy().astype(np.float64)


def _check_lj_off(md, L, terms, dtype, label):
    """every per-atom output of a box without pair forces against bonded_ref at the engine's positions, each atom within the
    rounding model's bound for its own terms; -> the outputs"""
    x = _held(md)
    f, e, w, t, tsum = _outputs(md)
    assert all(np.isfinite(a).all() for a in (f, e, w, t, tsum))
    fb, eb, wb, tb = br.bonded(x, L, terms)
    bf, bw = rc.box_bounds(x, L, terms, rc.unit_roundoff(np.float32 if dtype == torch.float32 else np.float64))
    err = np.linalg.norm(f - fb, axis=1)
    live = bf > 0
    print("%s: worst |dF| / bound %.3f, |dE| / bound %.3f, |dW| / bound %.3f, |dT| / bound %.3f over %d atoms" % (
        label, (err[live] / bf[live]).max(), (np.abs(e - eb)[live] / bw[live]).max(), (np.abs(w - wb)[live] / bw[live]).max(),
        (np.abs(t - tb).max(axis=1)[live] / bw[live]).max(), live.sum()))
    assert (err <= bf).all(), np.flatnonzero(err > bf)
    assert (np.abs(e - eb) <= bw).all() and (np.abs(w - wb) <= bw).all() and (np.abs(t - tb).max(axis=1) <= bw).all()
    assert (np.abs(t[:, :3].sum(axis=1) - w) <= bw).all()                                    # trace = virial
    assert np.abs(tsum - tb.sum(axis=0)).max() <= bw.sum()
    return f, e, w, t


# ------------------------------------------------------------------------------------ the fixture's solute in flexible water
@pytest.mark.parametrize("pucker", [False, True], ids=["flat", "puckered"])
@pytest.mark.parametrize("path,dtype", [("brick", "f64"), ("direct", "f64"), ("brick", "f32")])
def test_solute_in_flexible_water_matches_the_reference(emdee, solutes, monkeypatch, path, dtype, pucker):
    E, S, dtype = emdee, solutes[pucker], DTYPES[dtype]
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    pos, L, terms = S["positions"], S["L"], S["terms"]
    N = pos.shape[0]
    assert [len(a) for _, a, _ in terms] == [24 + 2 * S["n_water"], 38 + S["n_water"], 56] and S["n_water"] > 200
    assert rc.entries_per_atom(N, terms).max() > CHAIN_ENTRIES
    sol = pos[:S["n_solute"]]
    assert all((np.abs(sol[:, d, None] - sol[None, :, d]) > L / 2).any() for d in range(3))   # wrapped across all three faces
    if not pucker:                                                                            # every torsion exactly at 0 or pi
        phi = np.array([br.dihedral(br.unwrapped(pos, idx, L)) for idx in terms[2][1]])
        assert np.minimum(np.abs(phi), np.abs(np.abs(phi) - np.pi)).max() < 1e-12
    md = _md(E, pos, np.zeros((N, 3)), S["atoms"], L, dtype=dtype, excl=S["exclusions"], p14=S["pairs14"], s14=S["lj14scale"],
             inv_mass=S["inv_mass"], rc=RC_NM, rs=RS_NM, skin=SKIN_NM)
    without = _outputs(md)
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    with_b = _outputs(md)
    ref = br.bonded(_held(md), L, terms)
    _check_bonded_part(with_b, without, ref, 1e-9 if dtype == torch.float64 else 1e-4)
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    part = [a - b for a, b in zip(with_b[:4], without[:4])]
    assert np.abs(part[3][:, :3].sum(axis=1) - part[2]).max() <= tol * np.abs(ref[2]).max()  # per-atom tensors: trace = virial
    md.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_solute_without_pair_forces_each_atom_at_its_own_scale(emdee, solutes, dtype):
    E, S, dtype = emdee, solutes[True], DTYPES[dtype]
    pos, L, terms = S["positions"], S["L"], S["terms"]
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(np.zeros(N), np.full(N, 0.3))
    md = _md(E, pos, np.zeros((N, 3)), atoms, L, dtype=dtype, excl=S["exclusions"], terms=terms, inv_mass=S["inv_mass"],
             rc=RC_NM, rs=RS_NM, skin=SKIN_NM)
    _check_lj_off(md, L, terms, dtype, "solute, LJ off")
    md.close()


# ------------------------------------------------------------------------------------ small rings and branches
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_small_rings_branches_and_impropers(emdee, dtype):
    E, dtype = emdee, DTYPES[dtype]
    B = rc.ring_box()
    pos, L, terms = B["positions"], B["L"], B["terms"]
    N = pos.shape[0]
    assert len(B["first"]) >= 36 and set(B["names"]) == {"ring3", "ring4", "ring5", "ring6", "star", "improper", "chain3"}
    # molecules across the box faces and across the cell faces
    ends = np.append(B["first"], N)
    wrapped = [np.ptp(pos[a:b], axis=0).max() > L / 2 for a, b in zip(ends[:-1], ends[1:])]
    cells = [len({tuple(c) for c in np.floor(pos[a:b] / (L / 3)).astype(int)}) > 1 for a, b in zip(ends[:-1], ends[1:])]
    assert sum(wrapped) >= 8 and sum(cells) >= 20
    tors = terms[2][1]
    quad = {}
    for row in tors.tolist():
        quad[tuple(row)] = quad.get(tuple(row), 0) + 1
    assert 2 in quad.values() and 3 in quad.values()                                          # two and three terms on one quadruple
    assert rc.entries_per_atom(N, terms).max() > CHAIN_ENTRIES
    md = _md(E, pos, np.zeros((N, 3)), E.lennard_jones_atoms(np.zeros(N), np.ones(N)), L, dtype=dtype, excl=B["exclusions"], terms=terms)
    _check_lj_off(md, L, terms, dtype, "rings")
    md.close()


# ------------------------------------------------------------------------------------ singular geometries on the device
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_singular_and_nearly_singular_terms_on_the_device(emdee, dtype):
    E, dtype = emdee, DTYPES[dtype]
    ndt = np.float32 if dtype == torch.float32 else np.float64
    B = rc.singular_box(ndt)
    pos, L, terms = B["positions"], B["L"], B["terms"]
    N = pos.shape[0]
    md = _md(E, pos, np.zeros((N, 3)), E.lennard_jones_atoms(np.zeros(N), np.ones(N)), L, dtype=dtype, excl=B["exclusions"], terms=terms)
    x = _held(md)
    # the engine holds the exact cases exactly (representable coordinates): still singular where it evaluates them
    assert np.array_equal(x[B["exact_atoms"]], pos[B["exact_atoms"]])
    f, e, w, t = _check_lj_off(md, L, terms, dtype, "singular")
    assert np.array_equal(f[B["exact_atoms"]], np.zeros((len(B["exact_atoms"]), 3)))        # zero force by contract
    assert np.array_equal(w[B["exact_atoms"]], np.zeros(len(B["exact_atoms"])))
    # how near the singular geometries the box came where the engine evaluated it
    sn = rc.internal(br.ANGLE, np.pad(x[terms[1][1]], ((0, 0), (0, 1), (0, 0))))[1]
    t_int = rc.internal(br.TORSION, x[terms[2][1]])
    print("smallest nonzero sin(theta): angles %.2e, torsions %.2e" % (sn[sn > 0].min(), min(t_int[1][t_int[1] > 0].min(),
                                                                                                t_int[2][t_int[2] > 0].min())))
    assert sn[sn > 0].min() < (1e-5 if dtype == torch.float32 else 1e-12)
    md.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_straight_angle_leaves_every_other_atom_alone(emdee, dtype):
    """The chain box of test_gpu_bonded with three more atoms on a line along x and one angle term over them (k = 50,
    theta0 = 1.9): their own forces and every other atom's are bit for bit those of the box without that term."""
    E, dtype = emdee, DTYPES[dtype]
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N0 = pos.shape[0]
    terms, excl, p14 = _chains(N0)
    pos = np.concatenate([pos, [[0.25, 0.5, 0.5], [1.25, 0.5, 0.5], [2.0, 0.5, 0.5]]])
    N = N0 + 3
    atoms = E.lennard_jones_atoms(np.append(eps, np.zeros(3)), np.append(sigma, np.ones(3)))
    md = _md(E, pos, np.zeros((N, 3)), atoms, L, dtype=dtype, excl=excl, p14=p14, s14=_lj14scale(E), terms=terms)
    base = _outputs(md)
    angles = np.concatenate([terms[1][1], [[N0, N0 + 1, N0 + 2]]])
    md.set_bonded_(br.ANGLE, angles, np.concatenate([terms[1][2], [[50.0, 1.9]]]))
    got = _outputs(md)
    assert all(np.isfinite(a).all() for a in got)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3])
    ndt = np.float32 if dtype == torch.float32 else np.float64
    want = float(ndt(0.5) * ndt(50.0) * (ndt(np.pi) - ndt(1.9)) * (ndt(np.pi) - ndt(1.9))) / 3.0
    de = got[1] - base[1]
    assert np.array_equal(de[:N0], np.zeros(N0)) and np.abs(de[N0:] - want).max() <= 8 * rc.unit_roundoff(ndt) * want
    md.close()


# ------------------------------------------------------------------------------------ the use case: minimise and step from a lattice start
def _lattice_start(E):
    """the chain box with one chain drawn straight along x (an exactly straight angle pair and a collinear torsion, spacing 0.875
    against an r0 of 0.8 for its bonds: it contracts and swings back, never longer than 2.625 from end to end, inside rc + skin), its atoms without pair forces and at rest: it stays on its line, singular at every step"""
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N = pos.shape[0]
    terms, excl, p14 = _chains(N)
    chain = terms[2][1][0]
    pos, vel, eps = pos.copy(), vel.copy(), eps.copy()
    pos[chain] = np.array([0.5, 0.25, 0.25]) + np.outer(np.arange(4), [0.875, 0.0, 0.0])
    vel[chain] = 0.0
    eps[chain] = 0.0
    bp = terms[0][2].copy()
    bp[(terms[0][1][:, 0] >= chain[0]) & (terms[0][1][:, 1] <= chain[3])] = (200.0, 0.8)
    terms = [(br.BOND, terms[0][1], bp), (br.ANGLE, terms[1][1], np.tile((50.0, 1.9), (len(terms[1][1]), 1))), terms[2]]
    return pos, vel, E.lennard_jones_atoms(eps, sigma), L, terms, excl, p14, chain


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_minimise_and_step_from_a_start_with_straight_chains(emdee, oracle, dtype):
    E, dtype = emdee, DTYPES[dtype]
    pos, vel, atoms, L, terms, excl, p14, chain = _lattice_start(E)
    s14 = _lj14scale(E)
    md = _md(E, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14, terms=terms)
    res = md.minimize_(5, 0.0, dt_start=0.001, dt_max=0.005, max_step=0.05)
    st = md.state()
    assert np.isfinite([res.energy0, res.energy, res.g_max]).all() and res.iterations == 5
    assert all(np.isfinite(st[k].cpu().numpy()).all() for k in ("positions", "velocities", "forces"))
    x = st["positions"].cpu().numpy()
    assert np.array_equal(x[chain][:, 1:], pos[chain][:, 1:])                                 # still on its line
    md.close()
    md = _md(E, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14, terms=terms)
    md.step_(50, 0.005)
    st = md.state()
    x, v = st["positions"].cpu().numpy().astype(np.float64), st["velocities"].cpu().numpy()
    assert np.isfinite(x).all() and np.isfinite(v).all() and np.isfinite(md.totals()).all()
    assert np.array_equal(x[chain][:, 1:], pos[chain][:, 1:]) and np.abs(x[chain][:, 0] - pos[chain][:, 0]).max() > 1e-3
    if dtype == torch.float64:
        xr, _ = _numpy_verlet(oracle, pos, vel, L, atoms, excl, p14, s14, terms, 50, 0.005)
        d = x - xr
        assert np.abs(d - L * np.rint(d / L)).max() < 1e-8
    md.close()


# ------------------------------------------------------------------------------------ trajectory of the solute box
def test_solute_trajectory_matches_a_numpy_velocity_verlet(emdee, oracle, solutes):
    E, S = emdee, solutes[True]
    pos, L, terms, excl, p14, s14 = S["positions"], S["L"], S["terms"], S["exclusions"], S["pairs14"], S["lj14scale"]
    N = pos.shape[0]
    dt, nsteps = 2e-5, 50                                                                     # ps: the start has solvent packed on the solute
    md = _md(E, pos, np.zeros((N, 3)), S["atoms"], L, excl=excl, p14=p14, s14=s14, terms=terms, inv_mass=S["inv_mass"],
             rc=RC_NM, rs=RS_NM, skin=SKIN_NM)
    md.step_(nsteps, dt)
    x = md.state()["positions"].cpu().numpy()
    im = S["inv_mass"][:, None]
    force = lambda y: _reference(oracle, y, L, S["atoms"], excl, p14, s14, terms, rc=RC_NM, rs=RS_NM)[0][0]
    xr, v = pos.copy(), np.zeros((N, 3))
    f = force(xr)
    for _ in range(nsteps):
        v += 0.5 * dt * im * f
        xr += dt * v
        f = force(xr)
        v += 0.5 * dt * im * f
    d = x - xr
    print("largest displacement %.3e nm, largest |dx| %.3e" % (np.abs(xr - pos).max(), np.abs(d - L * np.rint(d / L)).max()))
    assert np.abs(xr - pos).max() > 1e-5
    assert np.abs(d - L * np.rint(d / L)).max() < 1e-8
    md.close()


# ------------------------------------------------------------------------------------ decomposed, in-process, eight domains
def _decomposed(E, world, pos, vel, atoms, L, dtype, excl, p14, s14, terms):
    """tests/test_gpu_dd_pairs.py's _build with the cutoffs of the nm boxes and the bonded tables set before the load"""
    dev = torch.device("cuda", 0)
    N = pos.shape[0]
    dd = E.DomainDecomposition([L] * 3, E.domain.rank_grid(world), E.LennardJonesModel(RC_NM, RS_NM), skin=SKIN_NM, dtype=dtype, device=dev)
    ndt = np.float64 if dtype == torch.float64 else np.float32
    for r in range(world):
        mine = np.arange(r, N, world)
        dd.set_atoms_(r, E.cu(pos[mine].astype(ndt), dev), E.cu(vel[mine].astype(ndt), dev), E.cu(atoms[mine], dev),
                      torch.from_numpy(mine.astype(np.int64)).to(dev))
    dd.set_exclusions_(excl)
    dd.set_pairs14_(p14, s14)
    for kind, a, p in terms:
        dd.set_bonded_(kind, a, p)
    dd.load_()
    return dd


@pytest.fixture(scope="module")
def corner_solute(emdee):
    """the puckered solute on the box corner, where the eight domains of a 2 x 2 x 2 grid meet; the waters nearer than 0.25 nm
    left out (unit masses in a decomposed run: the start of the other tests would throw the solvent across the box), and
    three more atoms without pair forces on a line along x through the cut at L / 2, for the case with a straight angle"""
    S = rc.solute_box(emdee, XML, pucker=True, tight=0.25)
    L = S["L"]
    N = S["positions"].shape[0]
    line = np.array([[0.5 * L - 0.11, 0.25, 0.5], [0.5 * L, 0.25, 0.5], [0.5 * L + 0.11, 0.25, 0.5]])
    ids = np.arange(N, N + 3)
    S["straight"] = dict(positions=np.concatenate([S["positions"], line]),
                         atoms=np.concatenate([S["atoms"], emdee.lennard_jones_atoms(np.zeros(3), np.full(3, 0.3))]),
                         bonds=(np.concatenate([S["terms"][0][1], [ids[:2], ids[1:]]]), np.concatenate([S["terms"][0][2], [[2e5, 0.1]] * 2])),
                         angles=(np.concatenate([S["terms"][1][1], [ids]]), np.concatenate([S["terms"][1][2], [[500.0, 2.09]]])),
                         exclusions=np.concatenate([S["exclusions"], [ids[:2], ids[1:], ids[[0, 2]]]]), ids=ids)
    return S


@pytest.mark.parametrize("case,dtype", [("solute", "f64"), ("solute", "f32"), ("straight", "f64")])
def test_decomposed_solute_matches_the_undivided_run(emdee, corner_solute, case, dtype):
    E, S, dtype = emdee, corner_solute, DTYPES[dtype]
    world, dt = 8, 2e-5
    L, terms, excl, atoms, pos = S["L"], S["terms"], S["exclusions"], S["atoms"], S["positions"]
    if case == "straight":
        X = S["straight"]
        pos, atoms, excl = X["positions"], X["atoms"], X["exclusions"]
        terms = [(br.BOND,) + X["bonds"], (br.ANGLE,) + X["angles"], terms[2]]
        a, b = pos[X["ids"][0]] - pos[X["ids"][1]], pos[X["ids"][2]] - pos[X["ids"][1]]
        assert not np.cross(a, b).any()                                                       # exactly straight
    N = pos.shape[0]
    vel = np.zeros((N, 3))
    dd = _decomposed(E, world, pos, vel, atoms, L, dtype, excl, S["pairs14"], S["lj14scale"], terms)
    md = _md(E, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=S["pairs14"], s14=S["lj14scale"], terms=terms, rc=RC_NM, rs=RS_NM,
             skin=SKIN_NM)
    _, _, f, owner = _gather(dd, world, N)
    assert len(set(owner[:S["n_solute"]].tolist())) >= 4                                       # the solute's atoms live in several domains
    tors = terms[2][1]
    assert (owner[tors] != owner[tors[:, :1]]).any(axis=1).sum() >= 10                        # and its terms span them
    if case == "straight":
        assert len(set(owner[S["straight"]["ids"]].tolist())) == 2
    fm = md.state()["forces"].cpu().numpy().astype(np.float64)
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    assert np.isfinite(f).all() and np.abs(f - fm).max() <= tol * np.abs(fm).max()
    dd.step_(29, dt)
    dd.step_(31, dt)
    md.step_(60, dt)
    if dtype == torch.float32:
        _compare(dd, md, world, N, L, tol_x=2e-4, tol_v=2e-3, tol_e=1e-4)
    else:
        _compare(dd, md, world, N, L)
    if case == "straight":
        x = _gather(dd, world, N)[0][S["straight"]["ids"]]
        assert np.array_equal(x[:, 1:], pos[S["straight"]["ids"]][:, 1:]) and np.abs(x[:, 0] - pos[S["straight"]["ids"]][:, 0]).max() > 1e-7
    dd.close()
    md.close()


# ------------------------------------------------------------------------------------ chained minimum images
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_term_longer_than_half_the_box_is_chained_along_its_bonds(emdee, dtype):
    E, dtype = emdee, DTYPES[dtype]
    B = rc.long_chain_box()
    pos, L, terms = B["positions"], B["L"], B["terms"]
    N = pos.shape[0]
    tors = terms[2][1]
    u = np.array([br.unwrapped(pos, idx, L) for idx in tors])
    along = np.linalg.norm(u[:, 3] - u[:, 0], axis=1)
    d = pos[tors[:, 3]] - pos[tors[:, 0]]
    nearest = np.linalg.norm(d - L * np.rint(d / L), axis=1)
    assert (along > L / 2).all() and (nearest < 2.8).all() and (nearest < along - 0.5).all()  # the ends meet through the boundary
    pair = pos[tors][:, :, None, :] - pos[tors][:, None, :, :]
    assert np.linalg.norm(pair - L * np.rint(pair / L), axis=3).max() < 2.8                   # every partner is in its owner's rows
    md = _md(E, pos, np.zeros((N, 3)), E.lennard_jones_atoms(np.zeros(N), np.ones(N)), L, dtype=dtype, excl=B["exclusions"], terms=terms)
    _check_lj_off(md, L, terms, dtype, "long chains")
    md.close()
