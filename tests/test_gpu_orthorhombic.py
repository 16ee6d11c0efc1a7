"""GPU tests of every kernel family on orthorhombic boxes whose three sides AND three cell counts differ (emdee_md_create:
lo[3], len[3], periodic[3]; emdee_dd_create: len[3]).  On a cube M[0] == M[1] == M[2] and len[0] == len[1] == len[2], so a
kernel that reads one axis's quantity where it means another's passes every cubic test bit for bit.  The yardstick is
tests/helpers/ortho_ref.py (numpy fp64, pinned to the oracle on cubes by tests/test_orthorhombic_host.py).

Every case asserts, on the CPU and before the GPU is touched, that
  * no pair lies within 1e-5 (relative, in r^2) of the cutoff, nor within 1e-5 (in r) of rc + skin where the neighbour set is
    compared: the strict tests r^2 < rc^2 then have one answer in fp32 as in fp64, and no pair is left out of a comparison;
  * the yardstick evaluated with two box lengths exchanged differs from the right answer by more than 100 x the tolerance
    in use: an axis mix-up cannot hide inside it;
and, from the EMDEE_DEBUG_PLAN line, that the brick grid is the one of three different cell counts.  What that line can
prove: it prints the brick counts nb[d] = ceil(M[d] / shape[d]), not M itself (emdee_md_nbr_stats carries no geometry
either), so M = (3, 4, 5) and (4, 4, 5) print the same 1 x 2 x 3.  The cell counts are therefore pinned from two sides: the
test computes M = floor(len / (rc + skin)) as configure_grid does and asserts it literally, and the engine's brick counts
must be the ones of that M on all three cyclings, where the brick shape (4, 2, 2) meets each count in turn -- (3, 4, 5) gives
1 x 2 x 3, 1 x 3 x 2 and 2 x 2 x 2, which no single cubic or two-equal M reproduces.  The direct path prints no plan line:
there the cyclings and the exchanged-lengths condition carry the check.  Decomposed runs take their geometry from
emdee_dd_describe.

Trajectories also run on the two cyclic permutations of the axes (positions, velocities, lo, lengths, periodic): the three
runs, un-permuted, must match the yardstick and so one another.

Tolerances are the project's: fp64 per-atom quantities 1e-6 max|want|, an isolated bonded or Coulomb part 1e-9, fp32 1e-4,
fp64 trajectories against the numpy integrator 1e-8 in position.  The one bound that is this module's own is the fp32
trajectory against the fp64 yardstick, X32 below."""
import functools
import math

import numpy as np
import pytest

from .helpers import ortho_ref as oref
from .test_gpu_bonded import _chains, _outputs
from .test_gpu_dd_pairs import _compare, _gather, _lj14scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RC, RS, SKIN, DT = 2.5, 2.0, 0.3, 0.005
TOL = {np.float64: 1e-6, np.float32: 1e-4}
PART = {np.float64: 1e-9, np.float32: 1e-4}
X64 = 1e-8
# fp32 positions after n steps against the fp64 yardstick.  Coordinates stay below 64, where one fp32 ulp is 2^-18 = 3.8e-6;
# each step rounds the position once (<= 1 ulp with the wrap) and the force error 1e-4 max|F| adds dt^2 / 2 x 1e-4 x ~50 =
# 6e-8, negligible.  Errors grow by exp(lambda t) with lambda ~ 4 for a Lennard-Jones liquid at T* ~ 2, t = 60 x 0.005:
# a factor 3.3.  Summed without cancellation: 60 x 3.8e-6 x 3.3 = 7.5e-4, taken as 1e-3 (the decomposed fp32 runs of
# tests/test_gpu_dd_pairs.py are held to 2e-3 against the undivided engine over the same 60 steps).  Measured on an MI355X:
# 4.6e-6 to 1.6e-5 over the cases of this module (largest: the direct path with lo != 0, and the chains), the thin box 5.2e-6
# after 40 steps; velocities 5e-5 to 2.2e-4 against their bound of 1e-2.  A margin of 60.
X32 = 1e-3
BAND = 1e-5
OFFSETS = np.array([-3.7, 1.9, 11.3])                  # lo != 0: three different offsets, one negative
UNWRAP = np.array([1.0, -1.0, 2.0])                    # whole box lengths added to every other atom, per axis
BRICK = {0: (4, 2, 2), 7: (4, 2, 2), 8: (4, 2, 2), 9: (2, 2, 2)}


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


# ---------------------------------------------------------------- systems
def _cell_counts(lengths, rlist):
    return [int(math.floor(l / rlist)) for l in lengths]


def _system(syn, cells, dtype, seed=None, lo=False, periodic=(1, 1, 1), species=1, rc=RC, rs=RS, skin=SKIN, pad=2.5,
            hot=1.4, unwrap=True, shift=0.0, jitter=None):
    """A jittered fcc block of cells = (nx, ny, nz) unit cells in global-id order.  Open axes get `pad` of room on either
    side of the lattice, so that no atom reaches a wall during a run.  species: 1, 2 (the synthetic mixture) or 3 (as the
    species3 family of tests/test_gpu_virial_tensor.py).  shift (in unit cells): moves the lattice and wraps it, so that the
    four-atom molecules of _chains cross each face."""
    kw = {} if seed is None else dict(seed=seed)
    if jitter is not None:
        kw["jitter"] = jitter
    pos, gid, lengths = syn.fcc_block(cells, (0, 0, 0), cells, **kw)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    lengths = np.array(lengths, dtype=np.float64)
    a = lengths[0] / cells[0]
    periodic = [int(p) for p in periodic]
    if shift:
        pos = np.mod(pos + shift * a, lengths)
    for d in range(3):
        if not periodic[d]:
            pos[:, d] += pad + 0.25 * a
            lengths[d] += 2.0 * pad
    box_lo = OFFSETS.copy() if lo else np.zeros(3)
    pos = pos + box_lo
    if unwrap:
        pos = pos + (np.arange(N) % 2)[:, None] * UNWRAP * lengths * np.array(periodic)
    vel = syn.raw_normals(np.arange(N), N)
    vel -= vel.mean(axis=0)
    vel *= hot * np.sqrt((3 * N - 3) / np.sum(vel * vel))
    if species == 1:
        eps, sigma = np.ones(N), np.ones(N)
    elif species == 2:
        eps, sigma = syn.mixture_parameters(syn.mixture_types(N))
    else:
        k = np.arange(N) % 3
        eps, sigma = np.array([1.0, 0.8, 0.6])[k], np.array([1.0, 0.95, 0.9])[k]
    if dtype == np.float32:
        pos, vel = pos.astype(np.float32).astype(np.float64), vel.astype(np.float32).astype(np.float64)
    return dict(pos=pos, vel=vel, lo=box_lo, lengths=lengths, periodic=periodic, eps=eps, sigma=sigma, rc=rc, rs=rs, skin=skin,
                N=N, M=_cell_counts(lengths, rc + skin), dtype=dtype, excl=None, p14=None, s14=1.0, c14=1.0, terms=None, q=None,
                coulomb=None, inv_mass=None, langevin=None)


def _pair_kw(S):
    kw = dict(excl=S["excl"], p14=S["p14"], lj14scale=S["s14"])
    if S["q"] is not None:
        kw.update(charges=S["q"], coulomb_k=S["coulomb"][0], eps_rf=S["coulomb"][1], coulomb14scale=S["c14"])
    return kw


def _want(S, atoms, pos=None, lengths=None, **over):
    kw = _pair_kw(S)
    kw.update(over)
    return oref.total(S["pos"] if pos is None else pos, S["lo"], S["lengths"] if lengths is None else lengths, S["periodic"],
                      S["rc"], S["rs"], atoms, S["terms"], **kw)


def _assert_decisive(S, atoms, want, tol, nbr=False):
    """The CPU-side conditions of the module's docstring, on the (rounded) positions the engine will be given and on their
    cycled copies."""
    M = S["M"]
    assert len(set(M)) == 3, "the three cell counts must differ: %r" % (M,)
    assert not all(m % b == 0 for m, b in zip(M, BRICK[0])), "some last brick must be ragged: %r" % (M,)
    for k in range(3):
        p, l, per = oref.cycle(S["pos"], k), oref.cycle(S["lengths"], k), list(oref.cycle(S["periodic"], k))
        near = oref.nearest_to_radius(p, l, per, S["rc"])
        assert near > BAND, "a pair within %.1e of the cutoff" % near
        if nbr:
            near = oref.nearest_to_radius(p, l, per, S["rc"] + S["skin"])
            assert near > 2 * BAND, "a pair within %.1e of rc + skin" % near
    for a, b in ((0, 1), (0, 2), (1, 2)):
        if not (S["periodic"][a] or S["periodic"][b]):
            continue
        sw = S["lengths"].copy()
        sw[[a, b]] = sw[[b, a]]
        # (the walls of an open axis moved far out: the exchange must show in the minimum image, not trip the wall check)
        wrong = oref.nonbonded(S["pos"], S["lo"] - 1e3, sw + 2e3 * (1 - np.array(S["periodic"])), S["periodic"], S["rc"], S["rs"],
                               atoms, **_pair_kw(S))
        for key in ("f", "t"):
            assert np.abs(wrong[key] - want[key]).max() >= 100 * tol * np.abs(want[key]).max(), (a, b, key)


def _part_bound(dtype, part, whole):
    """An isolated part is the difference of two outputs of the same engine.  fp64: 1e-9 of the part's largest entry.  fp32:
    1e-4 of it, plus what the subtraction itself cannot resolve -- either output is a sum of ~55 pair terms rounded to fp32
    at every addition, 2 sqrt(55) ~ 16 roundings of 2^-24 of the WHOLE output's size (where the part is a thousandth of the
    whole, as the Coulomb share of the virials of the chains, this term is the larger one)."""
    b = PART[dtype] * np.abs(part).max()
    return b if dtype == np.float64 else b + 16 * 2.0 ** -24 * np.abs(whole).max()


def _plan_bricks(err):
    lines = [l for l in err.splitlines() if l.startswith("emdee plan: bricks")]
    assert lines, "the brick path must be in use: " + err[-400:]
    return tuple(int(v) for v in lines[-1].split("bricks ")[1].split(",")[0].split(" x ")), lines[-1]


def _expected_bricks(M, variant=0):
    return tuple(-(-m // b) for m, b in zip(M, BRICK[variant]))


def _engine(E, S, atoms, dev, k=0):
    """the integrator on the system with its axes cycled k times"""
    dt = S["dtype"]
    cyc = lambda v: np.ascontiguousarray(oref.cycle(v, k))
    im = None if S["inv_mass"] is None else E.cu(S["inv_mass"].astype(dt), dev)
    md = E.VelocityVerlet(E.cu(cyc(S["pos"]).astype(dt), dev), E.cu(cyc(S["vel"]).astype(dt), dev), float(cyc(S["lengths"])[0]),
                          E.LennardJonesModel(S["rc"], S["rs"]), E.cu(atoms, dev), skin=S["skin"], inv_mass=im,
                          lo=list(cyc(S["lo"])), lengths=list(cyc(S["lengths"])), periodic=list(cyc(S["periodic"])))
    if S["excl"] is not None:
        md.set_exclusions_(S["excl"])
    if S["p14"] is not None:
        md.set_pairs14_(S["p14"], S["s14"])
    return md


def _dress(md, S, bonded=True, charged=True):
    if bonded:
        for kind, a, p in S["terms"] or []:
            md.set_bonded_(kind, a, p)
    if charged and S["q"] is not None:
        md.set_coulomb_(S["q"], S["coulomb"][0], S["coulomb"][1], S["c14"])
    if S["langevin"] is not None:
        md.set_langevin_(*S["langevin"])


def _uncycled(out, k):
    """test_gpu_bonded._outputs of a run on cycled axes, back in the caller's axes"""
    f, e, w, t, ts = out
    back = (3 - k) % 3
    return [oref.cycle(f, back), e, w, oref.cycle_tensor(t, back), oref.cycle_tensor(ts[None, :], back)[0]]


def _check_load(got, want, tol, what):
    for name, g, key in (("f", got[0], "f"), ("e", got[1], "e"), ("w", got[2], "w"), ("tensor", got[3], "t")):
        scale = np.abs(want[key]).max()
        err = np.abs(g - want[key]).max()
        print("%s %s: max err %.3e of max %.3e (tol %.0e)" % (what, name, err, scale, tol))
        assert err <= tol * scale, (what, name, err, scale)
    # the box sums: every atom's share to tol of its own size
    assert np.abs(got[4] - want["t"].sum(axis=0)).max() <= tol * np.abs(want["t"]).sum(axis=0).max(), what


def _rows(md):
    counts, nb = md.neighbor_lists()
    counts, nb = counts.cpu().numpy(), nb.cpu().numpy()
    return [np.sort(nb[i, :counts[i]]) for i in range(counts.shape[0])]        # (no unique: a pair listed twice shows)


def _check_rows(got, want, what):
    for i, row in want.items():
        assert np.array_equal(got[i], row), "%s: row %d differs (%d listed, %d wanted)" % (what, i, len(got[i]), len(row))


_TRAJ = {}


def _yard_trajectory(key, S, atoms, nsteps, k=0, normals=None):
    """the numpy integrator on the system cycled k times, un-cycled; cached per case (brick and direct runs share it)"""
    key = (key, S["dtype"], nsteps, k)
    if key not in _TRAJ:
        cyc = lambda v: oref.cycle(v, k)
        lo, lengths, periodic = cyc(S["lo"]), cyc(S["lengths"]), list(cyc(S["periodic"]))
        force = lambda x: oref.total(x, lo, lengths, periodic, S["rc"], S["rs"], atoms, S["terms"], **_pair_kw(S))["f"]
        lv = None if S["langevin"] is None else (S["langevin"][0], S["langevin"][1], normals)
        x, v = oref.verlet(cyc(S["pos"]), cyc(S["vel"]), force, nsteps, DT, S["inv_mass"], lv)
        back = (3 - k) % 3
        _TRAJ[key] = (oref.cycle(x, back), oref.cycle(v, back))
    return _TRAJ[key]


def _run_case(E, dev, capfd, monkeypatch, key, S, nsteps=60, path="brick", min_builds=3, rows=False, normals=None, cycles=(0, 1, 2),
              require=None, forbid=None):
    """load + trajectory of one system on its three axis cyclings, against the yardstick and against one another"""
    dtype = S["dtype"]
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    want = _want(S, atoms)
    _assert_decisive(S, atoms, want, TOL[dtype], nbr=rows)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    finals = []
    for k in cycles:
        capfd.readouterr()
        md = _engine(E, S, atoms, dev, k)
        _dress(md, S)
        got = _uncycled(_outputs(md), k)
        err = capfd.readouterr().err
        Mk = list(oref.cycle(S["M"], k))
        assert require is None or require in err, err[-600:]
        assert forbid is None or forbid not in err, err[-600:]
        if path == "direct":
            assert "emdee plan: bricks" not in err, err[-400:]
        else:
            bricks, line = _plan_bricks(err)
            print("cycle %d M %r: %s" % (k, Mk, line))
            assert bricks == _expected_bricks(Mk), (bricks, Mk, line)
        _check_load(got, want, TOL[dtype], "%s cycle %d" % (key, k))
        ep, _, vir = md.totals()
        assert ep == pytest.approx(want["e"].sum(), rel=TOL[dtype]) and vir == pytest.approx(want["w"].sum(), rel=TOL[dtype], abs=TOL[dtype] * np.abs(want["w"]).sum())
        st0 = md.nbr_stats()
        if rows:
            nbr = oref.neighbour_rows(S["pos"], S["lengths"], S["periodic"], S["rc"] + S["skin"])
            assert st0["listed"] == sum(len(r) for r in nbr.values())
            _check_rows(_rows(md), nbr, "%s cycle %d at the load" % (key, k))
        if nsteps:
            md.step_(nsteps, DT)
            st = md.state()
            back = (3 - k) % 3
            x = oref.cycle(st["positions"].cpu().numpy().astype(np.float64), back)
            v = oref.cycle(st["velocities"].cpu().numpy().astype(np.float64), back)
            builds = md.nbr_stats()["builds"]
            assert builds >= min_builds, builds                    # the load and at least two automatic rebuilds
            xr, vr = _yard_trajectory(key, S, atoms, nsteps, k if S["langevin"] is not None else 0, normals)
            dx = np.abs(oref.image_difference(x, xr, S["lengths"], S["periodic"])).max()
            print("%s cycle %d: %d builds, max |dx| %.3e, max |dv| %.3e" % (key, k, builds, dx, np.abs(v - vr).max()))
            assert dx < (X64 if dtype == np.float64 else X32)
            assert np.abs(v - vr).max() < 10 * (X64 if dtype == np.float64 else X32)
            finals.append((x, v, md.totals()))
        md.close()
    if S["langevin"] is None:
        for x, v, tot in finals[1:]:
            lim = 2 * (X64 if dtype == np.float64 else X32)
            assert np.abs(oref.image_difference(x, finals[0][0], S["lengths"], S["periodic"])).max() < lim
            assert tot[0] == pytest.approx(finals[0][2][0], rel=1e-9 if dtype == np.float64 else 1e-4)
            assert tot[1] == pytest.approx(finals[0][2][1], rel=1e-9 if dtype == np.float64 else 1e-4)


# ---------------------------------------------------------------- a, b, c, h: small boxes, N^2 yardstick
#   cells (5, 7, 9) at rc + skin = 2.8: sides (8.55, 11.97, 15.39), M = (3, 4, 5), bricks 1 x 2 x 3 of shape 4 x 2 x 2 with
#   ragged last bricks in x (3 of 4 cells) and z (1 of 2); the cyclings give M = (4, 5, 3) and (5, 3, 4).
SMALL = (5, 7, 9)
# per case, the fcc_block jitter seed whose box (fp64, fp32-rounded, and their cyclings) keeps clear of the bands; found on the
# CPU with the yardstick alone, and asserted again by every test before it touches the GPU
SEEDS = {"single": 0x5EED, "open1": 0x5EED, "open0": 0x5EEE, "thin": 0x5EF0, "chains": 0x5EED, "dd": 0x5F01, "typed": 0x5EF3,
         "large": 0x5EED, "long": 0x5EED}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lo", [False, True])
@pytest.mark.parametrize("path", ["brick", "direct"])
def test_single_species_load_and_trajectory(emdee, dev, capfd, monkeypatch, path, lo, dtype):
    S = _system(emdee.synthetic, SMALL, dtype, seed=SEEDS["single"], lo=lo)
    assert S["M"] == [3, 4, 5]
    _run_case(emdee, dev, capfd, monkeypatch, ("single", lo), S, path=path, rows=(path == "brick"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_three_species_load_and_trajectory(emdee, dev, capfd, monkeypatch, dtype):
    S = _system(emdee.synthetic, SMALL, dtype, seed=SEEDS["single"], lo=True, species=3)
    _run_case(emdee, dev, capfd, monkeypatch, "species3", S, require="emdee plan: bricks", forbid="two species")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("periodic,cells", [((1, 0, 1), (5, 7, 9)), ((0, 1, 1), (7, 5, 9))])
def test_mixed_periodicity_load_and_trajectory(emdee, dev, capfd, monkeypatch, periodic, cells, dtype):
    """One open axis, x or y (z open is tests/test_gpu_virial_tensor.py's): the lattice sits 2.5 + a / 4 inside the walls, and
    the yardstick checks at every step that no atom reaches them."""
    S = _system(emdee.synthetic, cells, dtype, seed=SEEDS["open%d" % periodic.index(0)], lo=(periodic[0] == 0), periodic=periodic)
    assert sorted(S["M"]) == [3, 5, 6], S["M"]
    _run_case(emdee, dev, capfd, monkeypatch, ("open", periodic), S)


# ---------------------------------------------------------------- g: the thin box
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_thin_box_with_two_cells_across(emdee, dev, capfd, monkeypatch, dtype):
    """cells (4, 7, 11): sides (6.84, 11.97, 18.81), the shortest just above 2 (rc + skin) = 5.6, M = (2, 4, 6): the +1 and
    the -1 neighbour cell of the thin axis are the same cell.  The cyclings put the thin axis on y and on z.  No pair may be
    listed twice and none missed."""
    S = _system(emdee.synthetic, (4, 7, 11), dtype, seed=SEEDS["thin"], lo=True)
    assert S["M"] == [2, 4, 6]
    _run_case(emdee, dev, capfd, monkeypatch, "thin", S, nsteps=40, min_builds=2, rows=True)


# ---------------------------------------------------------------- f: x sub-bins on and off, the set after rebuilds
@pytest.mark.parametrize("subbins", [True, False])
def test_neighbour_rows_after_rebuilds_with_and_without_x_sub_bins(emdee, dev, capfd, monkeypatch, subbins):
    E = emdee
    S = _system(E.synthetic, SMALL, np.float64, seed=SEEDS["single"], lo=True)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    if not subbins:
        monkeypatch.setenv("EMDEE_NO_SUBBINS", "1")
    for k in range(3):
        capfd.readouterr()
        md = _engine(E, S, atoms, dev, k)
        md.step_(30, DT)
        assert md.nbr_stats()["builds"] >= 3
        md.rebuild_()                                              # the list of the CURRENT positions
        plan = [l for l in capfd.readouterr().err.splitlines() if l.startswith("emdee plan: bricks")][-1]
        assert ("x sub-bins 4 " if subbins else "x sub-bins 1 ") in plan, plan
        cyc = lambda v: oref.cycle(v, k)
        x = md.state()["positions"].cpu().numpy()
        lengths, periodic = cyc(S["lengths"]), list(cyc(S["periodic"]))
        assert oref.nearest_to_radius(x, lengths, periodic, S["rc"] + S["skin"]) > 1e-12       # fp64: the set has one answer
        _check_rows(_rows(md), oref.neighbour_rows(x, lengths, periodic, S["rc"] + S["skin"]), "cycle %d" % k)
        md.close()


# ---------------------------------------------------------------- e: the 1024-thread variant (long rows, charged tile)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_long_rows_take_the_1024_thread_variant_on_a_non_cubic_box(emdee, dev, capfd, monkeypatch, dtype):
    """As test_long_rows_take_the_charged_instances_of_the_1024_thread_variant (tests/test_gpu_coulomb.py), on cells
    (8, 10, 12): M = (4, 5, 6).  Neighbour set, the Coulomb part alone and the whole, at eps_rf = 6 where the force jumps at rc.
    Among 3840 atoms with the project's jitter of 0.1 some pair always falls in the fp32 band around rc = 3 (about five are
    expected), whatever the seed.  So the inputs are chosen instead: a jitter of 0.06 moves every pair distance by less than
    0.06 sqrt(3) = 0.104 from an fcc shell (2.962, 3.199, 3.420 at this density), and rc = 3.08, rc + skin = 3.31 lie in the
    middle of the gaps between the shells, 0.11 from either: no pair is near either radius, in fp32 as in fp64.  (Not less
    jitter: on a nearly perfect lattice the forces cancel to a fraction of one pair's, and a tolerance relative to the largest
    force then measures the rounding of the cancellation.)"""
    E = emdee
    S = _system(E.synthetic, (8, 10, 12), dtype, seed=SEEDS["long"], lo=True, rc=3.08, rs=2.5, skin=0.23, jitter=0.06)
    assert S["M"] == [4, 5, 6]
    S["q"], S["coulomb"] = 0.5 * np.where(np.arange(S["N"]) % 2 == 0, 1.0, -1.0), (1.0, 6.0)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    want = _want(S, atoms)
    part = oref.nonbonded(S["pos"], S["lo"], S["lengths"], S["periodic"], S["rc"], S["rs"], atoms, lj=False, **_pair_kw(S))
    _assert_decisive(S, atoms, want, TOL[dtype], nbr=True)
    nbr = oref.neighbour_rows(S["pos"], S["lengths"], S["periodic"], S["rc"] + S["skin"])
    for k in range(3):
        md = _engine(E, S, atoms, dev, k)
        plain = _uncycled(_outputs(md), k)
        monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
        capfd.readouterr()
        _dress(md, S)
        err = capfd.readouterr().err
        monkeypatch.delenv("EMDEE_DEBUG_PLAN")
        plans = [l for l in err.splitlines() if l.startswith("emdee plan: charged engine")]
        assert plans and "brick kernels, variant 8" in plans[-1], err[-600:]
        assert _plan_bricks(err)[0] == _expected_bricks(list(oref.cycle(S["M"], k)), 8), err[-600:]
        charged = _uncycled(_outputs(md), k)
        for g, p, key in zip(charged[:4], plain[:4], "fewt"):
            assert np.abs((g - p) - part[key]).max() <= _part_bound(dtype, part[key], g), (k, key)
        _check_load(charged, want, TOL[dtype], "long rows cycle %d" % k)
        _check_rows(_rows(md), nbr, "long rows cycle %d" % k)
        md.close()


# ---------------------------------------------------------------- e: the 32-bit-field and the ballot builds
COL_RC, COL_RS, COL_SKIN = 3.5, 3.0, 0.4
GB = 8                                         # lanes per atom in the build (nbsys.hpp BrickVariant: GB)


def _column_box(lattice, spacing, sd, seed):
    """As test_neighbour_set_of_the_ballot_build (tests/test_gpu_parity2.py) on sides (5.05, 6.05, 7.05) (rc + skin): a dilute
    gas, a jittered lattice 2.1 apart, and THREE dense columns, one along each axis, each a lattice x lattice grid per layer
    with layers `spacing` apart, in cross-section cells that keep the columns a whole cell apart.  The build's tile rows run
    along x; with a column along every axis, each cycling of the axes has one lying along its rows."""
    rng = np.random.default_rng(seed)
    rl = COL_RC + COL_SKIN
    lengths = np.array([5.05, 6.05, 7.05]) * rl
    M = _cell_counts(lengths, rl)
    assert M == [5, 6, 7]
    cw = lengths / np.array(M)
    where = {0: {1: 1, 2: 1}, 1: {0: 3, 2: 3}, 2: {0: 1, 1: 4}}       # column along d: the cell index on the two other axes
    width = (lattice - 1) * spacing
    assert width + 0.5 < cw.min()
    cols, boxes = [], []
    for d, cells in where.items():
        axes = [None] * 3
        axes[d] = np.arange(int(lengths[d] / spacing)) * spacing
        lo_hi = {}
        for a, c in cells.items():
            axes[a] = np.arange(lattice) * spacing + c * cw[a] + 0.25
            lo_hi[a] = (c * cw[a] + 0.25 - 0.7, c * cw[a] + 0.25 + width + 0.7)
        g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        cols.append(g + rng.normal(0.0, sd, size=g.shape))
        boxes.append(lo_hi)
    m = np.round(lengths / 2.1).astype(int)
    gas = np.stack(np.meshgrid(*[np.arange(k) * (l / k) for k, l in zip(m, lengths)], indexing="ij"), axis=-1).reshape(-1, 3)
    gas = gas + rng.normal(0.0, 0.2, size=gas.shape)
    for lo_hi in boxes:                                                 # keep the gas out of the columns' reach
        inside = np.ones(gas.shape[0], dtype=bool)
        for a, (lo, hi) in lo_hi.items():
            inside &= (gas[:, a] > lo) & (gas[:, a] < hi)
        gas = gas[~inside]
    pos = np.concatenate(cols + [gas]) + OFFSETS
    N = pos.shape[0]
    return dict(pos=pos, vel=np.zeros((N, 3)), lo=OFFSETS.copy(), lengths=lengths, periodic=[1, 1, 1], eps=np.ones(N), sigma=np.ones(N),
                rc=COL_RC, rs=COL_RS, skin=COL_SKIN, N=N, M=M, dtype=np.float64, excl=None, p14=None, s14=1.0, c14=1.0, terms=None,
                q=None, coulomb=None, inv_mass=None, langevin=None)


@pytest.mark.parametrize("build,lattice,spacing,sd", [("ballot", 5, 0.72, 0.04), ("field32", 3, 0.6, 0.03)])
def test_crowded_tile_rows_take_the_32_bit_field_and_the_ballot_builds(emdee, dev, capfd, monkeypatch, build, lattice, spacing, sd):
    """The build is chosen from the most atoms in three consecutive cells of a tile row, with headroom span + span / 16 + 2
    (nbsys.hpp plan_sizes): up to 16 GB the two-phase build with 16-bit hit fields, up to 32 GB the same with one 32-bit field
    per row, beyond that the ballot build.  The plan line prints the span; the test restates the selection on it.  ballot:
    columns of 5 x 5 atoms per layer, 0.72 apart (about 137 per cell, 410 per span); field32: 3 x 3, 0.6 apart (59 per cell,
    177 per span).  M = (5, 6, 7) and its cyclings.  Neighbour set and forces at the load, in fp64 as the cubic test: a column
    atom has some 70 partners per unit of distance around rc + skin, so among the 2,000 column atoms several pairs lie in the
    fp32 band whatever the seed, and the fp32 set has no single answer."""
    E = emdee
    S = _column_box(lattice, spacing, sd, 41)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    want = _want(S, atoms)
    nbr = oref.neighbour_rows(S["pos"], S["lengths"], S["periodic"], S["rc"] + S["skin"])
    assert min(oref.nearest_to_radius(S["pos"], S["lengths"], S["periodic"], r) for r in (S["rc"], S["rc"] + S["skin"])) > 1e-10
    for a, b in ((0, 1), (0, 2), (1, 2)):
        sw = S["lengths"].copy()
        sw[[a, b]] = sw[[b, a]]
        wrong = _want(S, atoms, lengths=sw)
        assert np.abs(wrong["f"] - want["f"]).max() >= 100 * TOL[np.float64] * np.abs(want["f"]).max(), (a, b)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    for k in range(3):
        capfd.readouterr()
        md = _engine(E, S, atoms, dev, k)
        got = _uncycled(_outputs(md), k)
        err = capfd.readouterr().err
        bricks, line = _plan_bricks(err)
        print("cycle %d: %s" % (k, line))
        assert bricks == _expected_bricks(list(oref.cycle(S["M"], k))), line
        span = int(line.split("max 3-cell span ")[1].split(",")[0])
        planned = span + span // 16 + 2
        if build == "ballot":
            assert planned > 32 * GB, line
        else:
            assert 16 * GB < planned <= 32 * GB, line
        _check_load(got, want, TOL[np.float64], "%s cycle %d" % (build, k))
        rows = _rows(md)
        assert md.nbr_stats()["listed"] == sum(len(r) for r in nbr.values())
        _check_rows(rows, nbr, "%s cycle %d" % (build, k))
        md.close()


# ---------------------------------------------------------------- i: chains
def _chain_system(E, dtype, langevin=False):
    S = _system(E.synthetic, SMALL, dtype, seed=SEEDS["chains"], lo=True, species=2, hot=1.0, shift=0.75)
    N = S["N"]
    S["terms"], S["excl"], S["p14"] = _chains(N)
    S["s14"], S["c14"] = _lj14scale(E), 0.8333
    S["q"], S["coulomb"] = np.tile([0.6, -0.3, -0.5, 0.2], N // 4), (1.0, 5.0)
    S["inv_mass"] = 1.0 / (1.0 + 0.5 * (np.arange(N) % 3))
    if langevin:
        S["langevin"] = (2.0, 0.7, 0x5EED)
    return S


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_chains_cross_every_face_parts_and_whole(emdee, dev, capfd, monkeypatch, dtype):
    """Exclusions, 1-4 pairs, bonds, angles, torsions, charges and masses on M = (3, 4, 5), the molecules shifted by 0.75 of a
    unit cell so that some cross each of the three faces: the bonded part and the Coulomb part alone (1e-9), then the whole,
    then a trajectory on the three cyclings."""
    E = emdee
    S = _chain_system(E, dtype)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    w = oref.wrapped(S["pos"], S["lo"], S["lengths"], S["periodic"])
    span = np.abs(w.reshape(-1, 4, 1, 3) - w.reshape(-1, 1, 4, 3)).max(axis=(1, 2))
    for a in range(3):
        assert (span[:, a] > S["lengths"][a] / 2).any(), "no molecule crosses face %d" % a
    bonded = oref.bonded(S["pos"], S["lengths"], S["periodic"], S["terms"])
    coul = oref.nonbonded(S["pos"], S["lo"], S["lengths"], S["periodic"], S["rc"], S["rs"], atoms, lj=False, **_pair_kw(S))
    swapped = oref.bonded(S["pos"], S["lengths"][[0, 2, 1]], S["periodic"], S["terms"])
    assert np.abs(swapped["f"] - bonded["f"]).max() >= 100 * TOL[dtype] * np.abs(bonded["f"]).max()
    for k in range(3):
        md = _engine(E, S, atoms, dev, k)
        bare = _uncycled(_outputs(md), k)
        _dress(md, S, charged=False)
        with_b = _uncycled(_outputs(md), k)
        _dress(md, S, bonded=False)
        whole = _uncycled(_outputs(md), k)
        for g, p, key in zip(with_b[:4], bare[:4], "fewt"):
            assert np.abs((g - p) - bonded[key]).max() <= _part_bound(dtype, bonded[key], g), ("bonded", k, key)
        for g, p, key in zip(whole[:4], with_b[:4], "fewt"):
            assert np.abs((g - p) - coul[key]).max() <= _part_bound(dtype, coul[key], g), ("coulomb", k, key)
        md.close()
    _run_case(E, dev, capfd, monkeypatch, "chains", S, nsteps=50, min_builds=2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_chains_under_langevin(emdee, oracle, dev, capfd, monkeypatch, dtype):
    """The thermostat's noise is a function of (seed, step, atom id, component): it does not cycle with the axes, so each
    cycled run has a yardstick trajectory of its own.  The numbers come from the oracle's generator (orc_langevin_normals, C on
    the host): the counter-based generator is part of the interface (include/emdee_hip.h), so the yardstick shares its
    definition with the library by design, not its code; tests/test_oracle.py holds it to an independent restatement."""
    E = emdee
    S = _chain_system(E, dtype, langevin=True)
    seed = S["langevin"][2]
    normals = lambda step: np.array([oracle.langevin_normals(seed, step, i) for i in range(S["N"])])
    _run_case(E, dev, capfd, monkeypatch, "chains-langevin", S, nsteps=30, min_builds=2, normals=normals)


# ---------------------------------------------------------------- d and the large single-species box: sampled rows
def _sampled_case(E, dev, capfd, monkeypatch, S, want_line, nsteps, variant_from_plan=False):
    dtype = S["dtype"]
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    N = S["N"]
    rows = np.unique(np.concatenate([np.arange(0, N, N // 61), [N - 1]]))
    kw = dict(rows=rows)
    want = _want(S, atoms, **kw)
    assert len(set(S["M"])) == 3 and not all(m % b == 0 for m, b in zip(S["M"], BRICK[0])), S["M"]
    assert oref.nearest_to_radius(S["pos"], S["lengths"], S["periodic"], S["rc"], rows=rows) > BAND
    assert oref.nearest_to_radius(S["pos"], S["lengths"], S["periodic"], S["rc"] + S["skin"], rows=rows) > 2 * BAND
    for a, b in ((0, 1), (0, 2), (1, 2)):
        sw = S["lengths"].copy()
        sw[[a, b]] = sw[[b, a]]
        wrong = _want(S, atoms, lengths=sw, **kw)
        # (only the sampled atoms next to a face see the exchange: the largest difference is what counts)
        assert np.abs(wrong["f"] - want["f"]).max() >= 100 * TOL[dtype] * np.abs(want["f"]).max(), (a, b)
    nbr = oref.neighbour_rows(S["pos"], S["lengths"], S["periodic"], S["rc"] + S["skin"], rows=rows)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    finals = []
    for k in range(3):
        capfd.readouterr()
        md = _engine(E, S, atoms, dev, k)
        got = _uncycled(_outputs(md), k)
        err = capfd.readouterr().err
        assert want_line in err, err[-600:]
        variant = 0
        if variant_from_plan:
            on = [l for l in err.splitlines() if "typed kernels on" in l][-1]
            variant = int(on.split("variant ")[1].split(":")[0])
        bricks, line = _plan_bricks(err)
        print("cycle %d: %s" % (k, line))
        assert bricks == _expected_bricks(list(oref.cycle(S["M"], k)), variant), (bricks, variant, S["M"], k)
        for g, key in zip(got[:4], "fewt"):
            assert np.abs(g[rows] - want[key][rows]).max() <= TOL[dtype] * np.abs(want[key][rows]).max(), (k, key)
        got_rows = _rows(md)
        _check_rows(got_rows, nbr, "cycle %d" % k)
        md.step_(nsteps, DT)
        st = md.state()
        back = (3 - k) % 3
        finals.append((oref.cycle(st["positions"].cpu().numpy().astype(np.float64), back),
                       oref.cycle(st["velocities"].cpu().numpy().astype(np.float64), back), md.totals(), md.nbr_stats()["builds"]))
        md.close()
    assert finals[0][3] >= 2
    lim = 2 * (X64 if dtype == np.float64 else X32)
    for x, v, tot, _ in finals[1:]:
        dx = np.abs(oref.image_difference(x, finals[0][0], S["lengths"], S["periodic"])).max()
        print("cycled runs: max |dx| %.3e" % dx)
        assert dx < lim and np.abs(v - finals[0][1]).max() < 10 * lim
        assert tot[0] == pytest.approx(finals[0][2][0], rel=1e-9 if dtype == np.float64 else 1e-4)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_species_typed_kernels_long_cutoff_non_cubic(emdee, dev, capfd, monkeypatch, dtype):
    """As test_two_species_boxes_take_the_typed_kernels at rc = 3.5 (tests/test_gpu_parity2.py), cells (18, 29, 38): 79,344
    atoms, cell sides just above rc + skin = 3.8 on every axis, M = (8, 13, 17).  Sampled rows against the yardstick, the
    neighbour set of the sampled rows whole, and 20 steps on the three cyclings compared in full with one another."""
    S = _system(emdee.synthetic, (18, 29, 38), dtype, seed=SEEDS["typed"], lo=True, species=2, rc=3.5, rs=3.0)
    assert S["M"] == [8, 13, 17]
    _sampled_case(emdee, dev, capfd, monkeypatch, S, "typed kernels on", 20, variant_from_plan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hundred_thousand_atoms_single_species_non_cubic(emdee, dev, capfd, monkeypatch, dtype):
    """cells (20, 27, 45): 97,200 atoms, M = (12, 16, 27), bricks 3 x 8 x 14 with a ragged last brick in z."""
    S = _system(emdee.synthetic, (20, 27, 45), dtype, seed=SEEDS["large"], lo=False)
    assert S["M"] == [12, 16, 27]
    _sampled_case(emdee, dev, capfd, monkeypatch, S, "emdee plan: bricks", 20)


# ---------------------------------------------------------------- j: decomposed runs on a non-cubic GLOBAL box
DD_CELLS = (8, 10, 13)               # sides (13.68, 17.10, 22.23), M = (4, 6, 7) undivided; 4160 atoms


def _build_dd(E, dev, S, atoms, grid, load=True):
    """DomainDecomposition(lengths, grid) with per-axis lengths and an explicit grid; scattered initial slices"""
    dt = S["dtype"]
    world = grid[0] * grid[1] * grid[2]
    dd = E.DomainDecomposition(list(S["lengths"]), grid, E.LennardJonesModel(S["rc"], S["rs"]), skin=S["skin"], dtype=_tdt(dt), device=dev)
    for r in range(world):
        mine = np.arange(r, S["N"], world)
        dd.set_atoms_(r, E.cu(S["pos"][mine].astype(dt), dev), E.cu(S["vel"][mine].astype(dt), dev), E.cu(atoms[mine], dev),
                      torch.from_numpy(mine.astype(np.int64)).to(dev))
    if S["excl"] is not None:
        dd.set_exclusions_(S["excl"])
    if S["p14"] is not None:
        dd.set_pairs14_(S["p14"], S["s14"])
    for kind, a, p in S["terms"] or []:
        dd.set_bonded_(kind, a, p)
    if S["q"] is not None:
        dd.set_coulomb_(S["q"], S["coulomb"][0], S["coulomb"][1], S["c14"])
    if load:
        dd.load_()
    return dd


@functools.lru_cache(maxsize=None)
def _dd_want(E, dtype_name, chains):
    dtype = np.float64 if dtype_name == "float64" else np.float32
    S = _system(E.synthetic, DD_CELLS, dtype, seed=SEEDS["dd"], species=2, hot=1.0, shift=0.75 if chains else 0.0)
    if chains:
        S["terms"], S["excl"], S["p14"] = _chains(S["N"])
        S["s14"], S["c14"] = _lj14scale(E), 0.8333
        S["q"], S["coulomb"] = np.tile([0.6, -0.3, -0.5, 0.2], S["N"] // 4), (1.0, 5.0)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    want = _want(S, atoms)
    _assert_decisive(S, atoms, want, TOL[dtype])
    return S, atoms, want


@pytest.mark.parametrize("grid,variant", [((2, 1, 1), "f64"), ((1, 2, 1), "f64"), ((1, 1, 2), "f64"), ((2, 2, 2), "f64"), ((3, 2, 1), "f64"),
                                          ((1, 3, 2), "f64"), ((1, 3, 2), "chains"), ((3, 2, 1), "every5"), ((2, 2, 2), "f32")])
def test_decomposed_runs_on_a_non_cubic_global_box(emdee, dev, grid, variant):
    E = emdee
    dtype = np.float32 if variant == "f32" else np.float64
    S, atoms, want = _dd_want(E, np.dtype(dtype).name, variant == "chains")
    assert S["M"] == [4, 6, 7]
    N, world = S["N"], grid[0] * grid[1] * grid[2]
    # the domains' sides differ on every axis, and so do the periodic shifts of the ghost messages
    geo = E.dd.describe(list(S["lengths"]), grid, S["rc"] + S["skin"], 0)
    assert len(set(np.round(geo["local_len"], 9))) == 3, geo["local_len"]
    shifts = np.abs(np.array(geo["dir_shift"]))
    for a in range(3):
        assert set(np.unique(shifts[:, a])) <= {0.0, S["lengths"][a]}
    dd = _build_dd(E, dev, S, atoms, grid)
    md = _engine(E, S, atoms, dev)
    _dress(md, S)
    x, _, f, owner = _gather(dd, world, N)
    tol = TOL[dtype]
    assert np.abs(f - want["f"]).max() <= tol * np.abs(want["f"]).max()
    ep, _, vir = dd.totals()
    assert ep == pytest.approx(want["e"].sum(), rel=tol) and vir == pytest.approx(want["w"].sum(), rel=tol, abs=tol * np.abs(want["w"]).sum())
    a, b = np.array(dd.tensor_sums()), np.array(md.tensor_sums())
    rel = 1e-12 if dtype == np.float64 else 1e-5
    assert np.abs(a[:6] - b[:6]).max() <= rel * np.abs(b[:6]).max() and np.abs(a[6:] - b[6:]).max() <= rel * np.abs(b[6:]).max()
    assert np.abs(a[:6] - want["t"].sum(axis=0)).max() <= tol * np.abs(want["t"]).sum(axis=0).max()
    every = 5 if variant == "every5" else 0
    dd.step_(29, DT, every)
    dd.step_(31, DT, every)
    md.step_(60, DT, every)
    if dtype == np.float32:
        _compare(dd, md, world, N, S["lengths"], tol_x=2e-4, tol_v=2e-3, tol_e=1e-4)
    else:
        _compare(dd, md, world, N, S["lengths"])
    assert dd.stats()["rebuilds"] >= 3 and dd.stats()["migrated"] > 0
    dd.close()
    md.close()


# ---------------------------------------------------------------- k: two RCCL ranks on one GPU
@pytest.mark.parametrize("grid", [(1, 2, 1), (1, 1, 2)])
def test_two_rccl_ranks_on_a_non_cubic_box_match_the_undivided_run(emdee, dev, tmp_path, grid):
    """tests/helpers/ortho_rank.py: the chain box of the decomposed cases ((8, 10, 13) cells, charges, bonded terms) over two
    processes, the cut across y or across z, each child a fresh process under its own time limit."""
    import os
    import subprocess
    import sys

    from .conftest import ROOT
    E = emdee
    script = os.path.join(ROOT, "tests", "helpers", "ortho_rank.py")
    env0 = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1", NCCL_NET_GDR_LEVEL="0")
    kids = []
    try:
        for r in range(2):
            env = dict(env0, NCCL_HOSTID="emdee-ortho-rank-%d" % r)
            cmd = ["timeout", "-k", "10", "240", sys.executable, script, "--rank", str(r), "--out", str(tmp_path),
                   "--grid", ",".join(str(g) for g in grid)]
            k = subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                 start_new_session=True)
            kids.append(k)
            if r == 0:
                uid = k.stdout.readline().strip()
                assert uid.startswith("ID "), uid + k.stderr.read()[-800:]
            else:
                k.stdin.write(uid + "\n")
                k.stdin.flush()
        outs = [k.communicate(timeout=260) for k in kids]
    finally:
        for k in kids:
            if k.poll() is None:
                k.kill()
    for k, (out, err) in zip(kids, outs):
        assert k.returncode == 0, err[-800:]
    S, atoms, _ = _dd_want(E, "float64", True)
    N = S["N"]
    x, v, owner = np.zeros((N, 3)), np.zeros((N, 3)), np.full(N, -1)
    for r in range(2):
        d = np.load(os.path.join(tmp_path, "rank%d.npz" % r))
        assert (owner[d["gid"]] == -1).all()
        owner[d["gid"]] = r
        x[d["gid"]], v[d["gid"]] = d["x"], d["v"]
    assert (owner >= 0).all()
    tors = S["terms"][2][1]
    assert (owner[tors] != owner[tors[:, :1]]).any()                 # some terms span the two ranks
    md = _engine(E, S, atoms, dev)
    _dress(md, S)
    md.step_(60, DT)
    st = md.state()
    dx = oref.image_difference(x, st["positions"].cpu().numpy(), S["lengths"], S["periodic"])
    assert np.abs(dx).max() < 1e-9                                   # _compare's defaults
    assert np.abs(v - st["velocities"].cpu().numpy()).max() < 1e-8
    want = md.totals()
    for out, _ in outs:
        got = [float(t) for t in out.split("TOTALS")[1].split()[:3]]
        for a, b in zip(got, want):
            assert a == pytest.approx(b, rel=1e-9, abs=1e-9 * abs(want[0]))
    md.close()
