"""GPU tests of the centre-of-mass pull (include/emdee_hip.h: emdee_md_set_pull, emdee_md_pull_read, emdee_md_pull_log_read): a bias
between the centres of mass of atom groups behind every force pass, three launches, no atomics.  The yardstick is the numpy
restatement tests/helpers/pull_ref.py on the unwrapped positions emdee_md_get_state returns; it never calls the library.

Tolerances are those of a post term (tests/test_gpu_bonded.py, tests/test_gpu_restraints.py): the pull part -- the difference of an
engine's outputs with and without the table -- within 1e-9 (fp64) or 1e-4 (fp32) of the largest reference value; k is chosen so that
the pull forces are of the order of the pair forces.  Every box is the smallest on which the kernels can still go wrong."""
import ctypes as C

import numpy as np
import pytest

from .helpers import mask_cases as mc
from .helpers import pull_ref as pr
from .helpers import settle_ref as sr
from .test_gpu_dd_pairs import _build
from .test_gpu_masks import _engine as _mask_engine
from .test_gpu_masks import _stale_planes
from .test_gpu_molecular import _constraints_hold_on
from .test_gpu_settle import _engine as _water_engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
TOL = {np.float64: 1e-9, np.float32: 1e-4}
DT = 0.005
U, CF, DIST, DIR = pr.UMBRELLA, pr.CONSTANT_FORCE, pr.DISTANCE, pr.DIRECTION


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _refused(E, code, call, *args, **kw):
    with pytest.raises(E.EmDeeError) as err:
        call(*args, **kw)
    assert err.value.code == code, str(err.value)
    return str(err.value)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _md(E, dev, pos, vel, atoms, lengths, dtype=np.float64, rc=2.5, rs=2.0, skin=0.3, inv_mass=None):
    im = None if inv_mass is None else E.cu(np.asarray(inv_mass).astype(dtype), dev)
    lengths = [float(v) for v in lengths]
    return E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), lengths[0],
                            E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=skin, inv_mass=im, lo=[0.0, 0.0, 0.0],
                            lengths=lengths, periodic=[1, 1, 1])


def _outputs(md):
    """forces, energies, virials, per-atom tensors, the twelve box sums"""
    st = md.state(positions=False, velocities=False, energies=True, virials=True)
    return [_np(st["forces"]), _np(st["energies"]), _np(st["virials"]), _np(md.virial_tensor()), np.array(md.tensor_sums())]


def _positions(md):
    return _np(md.state(velocities=False, forces=False)["positions"])


def _coord(a, b, kind, geometry, k, r0=0.0, rate=0.0, mask=7, n=(0.0, 0.0, 0.0)):
    return dict(a=a, b=b, kind=kind, geometry=geometry, mask=mask if geometry == DIST else 0, k=k, r0=r0, rate=rate,
                n=np.asarray(n, dtype=np.float64))


def _raw(coords):
    ci = np.array([[c["a"], c["b"], c["kind"], c["geometry"], c["mask"]] for c in coords], dtype=np.int32)
    cd = np.array([[c["k"], c["r0"], c["rate"]] + list(c["n"]) for c in coords], dtype=np.float64)
    return ci, cd


def _set(md, group, coords, n_groups=None, **kw):
    ci, cd = _raw(coords)
    md.set_pull_(group, ci, cd, n_groups=n_groups, **kw)


def _clear(md):
    md.set_pull_(None, None)


def _read_bits(md):
    p = md.pull()
    return b"".join(np.ascontiguousarray(p[k]).tobytes() for k in ("xi", "xi0", "f", "U", "work", "D", "centres", "masses"))


# ---------------------------------------------------------------- 1. planes
_BOX = {}
SIZES = (1, 2, 1024, 1025, 257)                                # the chunk boundary and one past it


def _fluid(E):
    """synthetic.fcc_positions(9): 2916 atoms (Float32-rounded once, so that both precisions see the same atoms), unequal masses,
    five groups of SIZES dealt at random (the rest -1), and the grouped atoms nearest above the lower x face flying at it"""
    if not _BOX:
        pos, L = E.synthetic.fcc_positions(9)
        N = pos.shape[0]
        assert N == 2916
        pos = pos.astype(np.float32).astype(np.float64)
        rng = np.random.default_rng(83)
        mass = rng.uniform(1.0, 4.0, N)
        order = rng.permutation(N)
        group, at = np.full(N, -1), 0
        for g, s in enumerate(SIZES):
            group[order[at:at + s]] = g
            at += s
        vel = E.synthetic.velocities(N) / np.sqrt(mass)[:, None]
        flyers = np.where((group >= 0) & (pos[:, 0] > 0.02) & (pos[:, 0] < 0.2))[0][:6]
        assert len(flyers) == 6
        vel[flyers, 0] = -3.0
        _BOX.update(pos=pos, L=L, vel=vel, mass=mass, group=group, flyers=flyers, atoms=E.lennard_jones_atoms(1.0, 1.0, N))
    return _BOX


def _fluid_coords(B, k=60.0):
    """four coordinates: two share group 1; a direction coordinate with a skew n; a single-axis mask; a constant force.  The
    references sit 0.3 - 0.5 from the loaded xi, so that k |xi - xi0| is of the order of the pair forces (tens)."""
    R, _ = pr.centres(B["pos"], B["mass"], B["group"], 5)
    n = np.array([1.0, -2.0, 0.5])
    d01 = np.linalg.norm(R[1] - R[0])
    return [_coord(0, 1, U, DIST, k, r0=d01 + 0.4, rate=0.5),
            _coord(1, 2, U, DIR, k, r0=float(pr.unit(n) @ (R[2] - R[1])) - 0.3, n=n),
            _coord(3, 2, U, DIST, 40.0 * k, r0=abs(R[2][1] - R[3][1]) + 0.5, mask=2),
            _coord(4, 0, CF, DIST, -25.0)]


def _check_planes(md, B, coords, dtype, what, without=None):
    """the pull part of every output against numpy at the engine's own positions; returns the outputs with the table"""
    tol = TOL[dtype]
    with_p = _outputs(md)
    x, read = _positions(md), md.pull()
    ref = pr.evaluate(x, B["mass"], B["group"], coords, read["xi0"], 5)
    if without is None:
        _clear(md)
        without = _outputs(md)
    for name, got, want in zip(("forces", "energies", "virials", "tensors"), [a - b for a, b in zip(with_p[:4], without[:4])],
                               (ref["forces"], ref["energies"], ref["virials"], ref["tensors"])):
        err = np.abs(got - want).max() / np.abs(want).max()
        print("%s, %s: max error / max entry = %.3e (bound %.0e)" % (what, name, err, tol))
        assert err <= tol, (what, name)
    # the sum of the pull forces is zero to that tolerance
    total = (with_p[0] - without[0]).sum(axis=0)
    print("%s: sum of the pull forces %s (largest %.3f)" % (what, total, np.abs(ref["forces"]).max()))
    assert np.abs(total).max() <= tol * np.abs(ref["forces"]).max()
    assert np.abs(ref["forces"].sum(axis=0)).max() <= 1e-12 * np.abs(ref["forces"]).max()
    # atoms outside every group keep their bits
    out = B["group"] < 0
    for a, b in zip(with_p[:4], without[:4]):
        assert np.array_equal(a[out], b[out])
    # the twelve box sums: W moves by sum_c sym(D (x) F_b), K not at all; the energy by sum_c U_c
    wsum = ref["W"].sum(axis=0)
    assert np.abs((with_p[4][:6] - without[4][:6]) - wsum).max() <= tol * np.abs(wsum).max() * 10      # (tests/test_gpu_bonded.py's form)
    assert np.array_equal(with_p[4][6:], without[4][6:])
    assert abs((with_p[1].sum() - without[1].sum()) - ref["U"].sum()) <= tol * 10 * np.abs(ref["U"]).sum()
    # pull_read: the words of every coordinate and the centres
    for q, key in enumerate(("xi", "xi0", "f", "U")):
        assert np.abs(read[key] - ref["words"][:, q]).max() <= tol * np.abs(ref["words"][:, q]).max(), key
    assert np.abs(read["D"] - ref["words"][:, 5:8]).max() <= tol * np.abs(ref["words"][:, 5:8]).max()
    assert np.abs(read["centres"] - ref["centres"]).max() <= tol * np.abs(ref["centres"]).max()
    assert np.abs(read["masses"] - ref["masses"]).max() <= tol * ref["masses"].max()
    return with_p, ref


@pytest.mark.parametrize("path,dtype", [("brick", np.float64), ("direct", np.float64), ("brick", np.float32)])
def test_planes_at_the_load_and_after_a_rebuild_and_a_face_match_numpy(emdee, dev, monkeypatch, path, dtype):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    B = _fluid(E)
    coords = _fluid_coords(B)
    mk = lambda: _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, dtype=dtype, inv_mass=1.0 / B["mass"])
    md, twin = mk(), mk()
    without = _outputs(md)
    _set(md, B["group"], coords, log_every=10, log_capacity=8)
    what = "%s/%s" % (path, dtype.__name__)
    _, ref = _check_planes(md, B, coords, dtype, what + " at the load", without=without)
    # (a Float32 engine works on the inverse masses rounded to fp32: within its tolerance)
    pair = np.abs(without[0]).max()
    print("%s: largest pull force %.2f, largest pair force %.2f" % (what, np.abs(ref["forces"]).max(), pair))
    builds, image0 = md.nbr_stats()["builds"], np.floor(B["pos"] / B["L"])
    md.step_(40, DT)
    x = _positions(md)
    crossed = (np.floor(x / B["L"]) != image0).any(axis=1) & (B["group"] >= 0)
    assert crossed.any() and md.nbr_stats()["builds"] > builds, (crossed.sum(), md.nbr_stats())
    assert np.abs(x - B["pos"]).max() < 2.0                            # (unwrapped: nobody jumped a box length)
    read = md.pull()
    assert read["xi0"][0] == pr.advance(coords[0]["r0"], coords[0]["rate"], DT, 40) and read["work"][0] != 0.0
    assert (read["work"][1:] == 0.0).all()                              # (rate 0, and a constant force keeps no work)
    _, ref = _check_planes(md, B, coords, dtype, what + " after 40 steps")
    fpair = np.abs(_np(md.state()["forces"])).max()
    assert 0.1 * fpair <= np.abs(ref["forces"]).max() <= 10.0 * fpair  # of the order of the pair forces
    # the twin that never had a table went elsewhere: the bias acts
    twin.step_(40, DT)
    assert np.abs(_positions(twin) - x).max() > 1e-3
    md.close()
    twin.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family,post", [("uniform", "none"), ("species3", "tables"), ("typed", "none"), ("direct", "none"), ("uniform", "bonded")])
def test_a_plane_the_mask_leaves_out_keeps_its_bits(emdee, oracle, dev, capfd, monkeypatch, family, post, dtype):
    """every mask with a table in force (an engine without masses: m = 1): the planes asked for hold the whole force field plus the
    pull term (once), the force plane keeps its bits under a mask without FORCES and under the tensor pass, and the three launches
    run once per pass"""
    E = emdee
    box = mc.family_box(E, family, dtype)
    md, _ = _mask_engine(E, dev, box, dtype, monkeypatch, capfd, post)
    N = box["pos"].shape[0]
    base = mc.reference(oracle, box, post)
    fmax = np.abs(base[0]).max()
    rng = np.random.default_rng(89)
    group = np.full(N, -1)
    order = rng.permutation(N)
    group[order[:1]], group[order[1:N // 3]], group[order[N // 3:N // 2]] = 0, 1, 2
    R, _ = pr.centres(box["pos"], np.ones(N), group, 3)
    k = fmax / 0.4
    coords = [_coord(0, 1, U, DIST, k, r0=np.linalg.norm(R[1] - R[0]) + 0.4), _coord(2, 1, CF, DIR, 0.5 * fmax, n=(0.3, 0.4, -1.0)),
              _coord(0, 2, U, DIST, k, r0=abs(R[2][2] - R[0][2]) - 0.3, mask=4)]
    _set(md, group, coords)
    P = pr.evaluate(box["pos"], np.ones(N), group, coords, [c["r0"] for c in coords], 3)
    want = [base[0] + P["forces"], base[1] + P["energies"], base[2] + P["virials"]]
    tol = 1e-6 if dtype == np.float64 else 1e-4                      # (the whole force field against its fp64 reference)
    md.profile_(True)
    for m in range(1, 8):
        what = "%s/%s mask %d" % (family, post, m)
        _stale_planes(md)
        md.forces_(1)
        f1 = md.state(positions=False, velocities=False)["forces"]
        before = md.kernel_time("pull")[1]
        md.forces_(m)
        assert md.kernel_time("pull")[1] == before + 1, what
        fm = md.state(positions=False, velocities=False)["forces"]
        if m & 1:
            assert np.abs(_np(fm) - want[0]).max() <= tol * np.abs(want[0]).max(), what
        else:
            assert torch.equal(fm, f1), what + ": the force plane was rewritten"
        st = md.state(positions=False, velocities=False, forces=False, energies=True, virials=True)
        assert np.abs(_np(st["energies"]) - want[1]).max() <= tol * np.abs(want[1]).max(), what
        assert np.abs(_np(st["virials"]) - want[2]).max() <= tol * np.abs(want[2]).max(), what
        f2 = md.state(positions=False, velocities=False)["forces"]
        vt = _np(md.virial_tensor())                                  # the tensor pass: forces left alone, trace = virial
        assert torch.equal(md.state(positions=False, velocities=False)["forces"], f2), what + ": the tensor pass wrote forces"
        assert np.abs(vt[:, :3].sum(axis=1) - want[2]).max() <= tol * np.abs(want[2]).max(), what
    md.close()


# ---------------------------------------------------------------- 2. dynamics
def _pair(E, rate):
    """two atoms of masses 1 and 3, 4.0 apart along a skew axis in a 12 sigma box (rc + skin = 2.8, the nearest image 8.0): the
    umbrella is their only force; small velocities across and along the axis"""
    axis = pr.unit([1.0, 2.0, -1.5])
    pos = np.array([[1.5, 1.0, 3.0], [1.5, 1.0, 3.0] + 4.0 * axis])
    vel = np.array([[0.05, -0.02, 0.03], [-0.01, 0.04, 0.02]])
    mass = np.array([1.0, 3.0])
    coords = [_coord(0, 1, U, DIST, 20.0, r0=3.7, rate=rate)]
    return dict(pos=pos, vel=vel, mass=mass, group=np.array([0, 1]), coords=coords, L=12.0, atoms=E.lennard_jones_atoms(1.0, 1.0, 2))


def _pair_engine(E, dev, B, dtype=np.float64, **kw):
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, dtype=dtype, inv_mass=1.0 / B["mass"])
    _set(md, B["group"], B["coords"], **kw)
    return md


@pytest.mark.parametrize("rate", [0.0, 0.35])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_atoms_follow_the_numpy_velocity_verlet(emdee, dev, dtype, rate):
    E = emdee
    B = _pair(E, rate)
    md = _pair_engine(E, dev, B, dtype)
    md.step_(200, DT)
    pos = B["pos"].astype(dtype).astype(np.float64)
    vel = B["vel"].astype(dtype).astype(np.float64)
    x, v, xi0, work, fs, (amp_x, amp_v) = pr.verlet(pos, vel, B["mass"], B["group"], B["coords"], 2, DT, 200)
    st = md.state()
    gx, gv = _np(st["positions"]), _np(st["velocities"])
    # (the amplitudes: the largest displacement from the start and the largest speed over numpy's run; xi starts 0.3 off xi0)
    ex, ev = np.abs(gx - x).max(), np.abs(gv - v).max()
    print("%s rate %.2f, 200 steps: max |dx| = %.3e (amplitude %.3f), max |dv| = %.3e (amplitude %.3f), bound %.0e of them"
          % (dtype.__name__, rate, ex, amp_x, ev, amp_v, TOL[dtype]))
    assert amp_x > 0.1
    assert ex <= TOL[dtype] * amp_x and ev <= TOL[dtype] * amp_v
    read = md.pull()
    assert read["xi0"][0] == pr.advance(3.7, rate, DT, 200) == xi0[0]          # the host's sequence, bit for bit
    print("work %.12g (numpy %.12g)" % (read["work"][0], work[0]))
    if rate == 0.0:
        assert read["work"][0] == 0.0
    else:
        assert abs(work[0]) > 1e-3 and abs(read["work"][0] - work[0]) <= TOL[dtype] * np.abs(pr.work_rule(fs[:, 0], rate, DT)).max()
    md.close()


# ---------------------------------------------------------------- 3. reproducibility
def _small(E):
    """the 864-atom fcc box with three groups and two coordinates, one of them moving"""
    pos, L = E.synthetic.fcc_positions(6)
    N = pos.shape[0]
    rng = np.random.default_rng(97)
    mass = rng.uniform(1.0, 3.0, N)
    group = np.full(N, -1)
    order = rng.permutation(N)
    group[order[:3]], group[order[3:300]], group[order[300:301]] = 0, 1, 2
    R, _ = pr.centres(pos, mass, group, 3)
    coords = [_coord(0, 1, U, DIST, 80.0, r0=np.linalg.norm(R[1] - R[0]) + 0.3, rate=0.4),
              _coord(2, 1, U, DIR, 50.0, r0=float(pr.unit([0.0, 1.0, 1.0]) @ (R[1] - R[2])) - 0.2, rate=-0.3, n=(0.0, 1.0, 1.0))]
    return dict(pos=pos, vel=E.synthetic.velocities(N) / np.sqrt(mass)[:, None], mass=mass, group=group, coords=coords, L=L,
                atoms=E.lennard_jones_atoms(1.0, 1.0, N))


def _small_engine(E, dev, B, table=True, **kw):
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, inv_mass=1.0 / B["mass"])
    if table:
        _set(md, B["group"], B["coords"], **kw)
    return md


def test_dealing_of_steps_fresh_engines_and_a_cleared_table(emdee, dev):
    E = emdee
    B = _small(E)
    ends = []
    for deal in ((40,), (5,) * 8, (1,) * 40, (40,)):                   # (the last: a second fresh engine)
        md = _small_engine(E, dev, B, log_every=4, log_capacity=16)
        for n in deal:
            md.step_(n, DT)
        log = md.pull_log()
        ends.append((md.state(), _read_bits(md), log["xi"].tobytes() + log["f"].tobytes(), (log["count"], log["dropped"])))
        md.close()
    assert ends[0][3] == (10, 0) and np.frombuffer(ends[0][2]).size == 40
    for other in ends[1:]:
        for key in ("positions", "velocities", "forces"):
            assert torch.equal(ends[0][0][key], other[0][key]), key
        assert ends[0][1] == other[1] and ends[0][2] == other[2] and ends[0][3] == other[3]
    # a table set and cleared: the twin that never had one, bit for bit and launch for launch
    md, twin = _small_engine(E, dev, B), _small_engine(E, dev, B, table=False)
    _clear(md)
    for eng in (md, twin):
        eng.profile_(True)
        eng.step_(40, DT)
    a, b = md.state(), twin.state()
    for key in ("positions", "velocities", "forces"):
        assert torch.equal(a[key], b[key]), key
    assert twin.kernel_time("pull") == (0.0, 0) and md.kernel_time("pull") == (0.0, 0)
    for name in ("lj_force_nbr", "verlet_kick_drift", "verlet_kick", "lj_force_nbr_fused_step", "rebuild"):
        assert md.kernel_time(name)[1] == twin.kernel_time(name)[1], name
    # with a table: the three launches, timed as one entry, behind every force pass
    _set(md, B["group"], B["coords"])
    md.profile_(True)
    md.step_(7, DT)
    ms, launches = md.kernel_time("pull")
    assert launches == md.kernel_time("lj_force_nbr")[1] == 7 and ms > 0.0 and md.kernel_time(19) == (ms, launches)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 4. composition
def _two_waters(B):
    """two molecules of the water box that were loaded whole (no atom wrapped away from its molecule), well apart"""
    whole = np.where(np.abs(B["pos"] - B["unwrapped"]).reshape(-1, 3, 3).max(axis=(1, 2)) == 0.0)[0]
    a = whole[0]
    com = lambda m: (B["mass"][B["mol"][m], None] * B["pos"][B["mol"][m]]).sum(axis=0) / B["mass"][B["mol"][m]].sum()
    far = [m for m in whole[1:] if 2.0 < np.linalg.norm(com(m) - com(a)) < 3.5]
    assert far
    return int(a), int(far[0])


def test_rigid_water_under_c_rescale_with_molecular_scaling(emdee, dev):
    E = emdee
    B = sr.water_box()
    ma, mb = _two_waters(B)
    N = B["pos"].shape[0]
    group = np.full(N, -1)
    group[B["mol"][ma]], group[B["mol"][mb]] = 0, 1
    md = _water_engine(E, dev, B)
    md.set_molecular_scaling_()
    without = np.array(md.molecular_tensor_sums())
    x0 = _positions(md)
    R, _ = pr.centres(x0, B["mass"], group, 2)
    r0 = np.linalg.norm(R[1] - R[0]) - 0.5
    coords = [_coord(0, 1, U, DIST, 200.0, r0=r0)]
    _set(md, group, coords)
    with_p = np.array(md.molecular_tensor_sums())
    ref = pr.evaluate(x0, B["mass"], group, coords, [r0], 2)
    got, want = with_p[:6] - without[:6], ref["W"][0]
    print("W_mol with - without = %s\n   sym(D (x) F_b)     = %s" % (got, want))
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    assert np.array_equal(with_p[6:], without[6:])
    md.set_barostat_("c-rescale", p_ref=1.0, compressibility=0.05, tau_p=0.5, every=5, temperature=1.0, seed=7)
    box0 = np.array(md.box()[1])
    md.step_(20, sr.DT)                                              # four events
    box1 = np.array(md.box()[1])
    assert not np.array_equal(box0, box1)
    _constraints_hold_on(md, B, box1, "rigid water pulled under C-rescale")
    read = md.pull()
    assert read["xi0"][0] == r0                                      # xi0 does not scale with the box
    x = _positions(md)
    ref = pr.evaluate(x, B["mass"], group, coords, [r0], 2)
    assert abs(read["xi"][0] - ref["words"][0, 0]) <= 1e-9 * ref["words"][0, 0]
    md.close()


def test_minimize_moves_the_coordinate_towards_its_reference(emdee, dev):
    E = emdee
    B = sr.water_box()
    ma, mb = _two_waters(B)
    group = np.full(B["pos"].shape[0], -1)
    group[B["mol"][ma]], group[B["mol"][mb]] = 0, 1
    md = _water_engine(E, dev, B)
    R, _ = pr.centres(_positions(md), B["mass"], group, 2)
    r0 = np.linalg.norm(R[1] - R[0]) - 0.5
    _set(md, group, [_coord(0, 1, U, DIST, 500.0, r0=r0, rate=0.25)])
    before = md.pull()
    md.minimize_(150, 1e-3, dt_start=0.0005, dt_max=0.005, max_step=0.05)
    after = md.pull()
    print("|xi - r0|: %.4f before, %.4f after the minimisation" % (abs(before["xi"][0] - r0), abs(after["xi"][0] - r0)))
    assert abs(after["xi"][0] - r0) < abs(before["xi"][0] - r0)
    assert after["xi0"][0] == r0 and after["work"][0] == 0.0         # (the minimiser completes no step: the reference stays)
    _constraints_hold_on(md, B, np.array(md.box()[1]), "rigid water minimised under a pull")
    md.close()


# ---------------------------------------------------------------- 5. the log
@pytest.mark.parametrize("samples", [4, 5, 8])
def test_log_entries_are_the_reads_of_a_twin(emdee, dev, samples):
    """capacity 5: capacity - 1, capacity and capacity + 3 samples"""
    E = emdee
    B = _small(E)
    every, cap = 3, 5
    md, twin = _small_engine(E, dev, B, log_every=every, log_capacity=cap), _small_engine(E, dev, B)
    md.step_(every * samples + 2, DT)                                 # (two steps past the last sample: they add none)
    xi, f = [], []
    for _ in range(samples):
        twin.step_(every, DT)
        read = twin.pull()
        xi.append(read["xi"]); f.append(read["f"])
    log = md.pull_log()
    kept = min(samples, cap)
    assert (log["count"], log["dropped"]) == (kept, samples - kept)
    assert log["xi"].shape == (kept, 2) and np.array_equal(log["xi"], np.array(xi)[:kept]) and np.array_equal(log["f"], np.array(f)[:kept])
    assert twin.pull_log()["count"] == 0 and twin.pull_log()["xi"].shape == (0, 2)     # (no log asked for)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 6. refusals
def test_every_refusal_leaves_the_previous_table_in_force(emdee, dev):
    E = emdee
    B = _small(E)
    N = B["pos"].shape[0]
    md = _small_engine(E, dev, B)
    bits, state = _read_bits(md), md.state()
    g, ci, cd = B["group"], *_raw(B["coords"])

    def grp(i, v):
        out = g.copy(); out[i] = v
        return out

    def ints(row, col, v):
        out = ci.copy(); out[row, col] = v
        return out

    def dbl(row, col, v):
        out = cd.copy(); out[row, col] = v
        return out
    gdev = torch.as_tensor(g, dtype=torch.int32, device=dev)
    raw = lambda group, a, b, n, le=0, lc=0: E._lib.call(
        "emdee_md_set_pull", md._handle, None if group is None else C.c_void_p(group.data_ptr()), 3,
        None if a is None else a.ctypes.data_as(C.c_void_p), None if b is None else b.ctypes.data_as(C.c_void_p), n, le, lc)
    cases = [
        ("group id too high", ERR_INVALID, lambda: md.set_pull_(grp(5, 3), ci, cd, n_groups=3), "atom 5"),
        ("group id too low", ERR_INVALID, lambda: md.set_pull_(grp(7, -2), ci, cd, n_groups=3), "atom 7"),
        ("n_groups 0", ERR_INVALID, lambda: md.set_pull_(g, ci, cd, n_groups=0), "n_groups = 0"),
        ("n_groups 9", ERR_INVALID, lambda: md.set_pull_(g, ci, cd, n_groups=9), "n_groups = 9"),
        ("n_coords 9", ERR_INVALID, lambda: md.set_pull_(g, np.tile(ci[0], (9, 1)), np.tile(cd[0], (9, 1)), n_groups=3), "n_coords = 9"),
        ("n_coords -1", ERR_INVALID, lambda: raw(gdev, ci, cd, -1), "n_coords = -1"),
        ("an empty group", ERR_INVALID, lambda: md.set_pull_(grp(np.where(g == 2)[0], -1), ci, cd, n_groups=3), "group 2 is empty"),
        ("a = b", ERR_INVALID, lambda: md.set_pull_(g, ints(0, 1, 0), cd, n_groups=3), "coordinate 0"),
        ("a group outside the table", ERR_INVALID, lambda: md.set_pull_(g, ints(1, 0, 3), cd, n_groups=3), "coordinate 1"),
        ("unknown kind", ERR_INVALID, lambda: md.set_pull_(g, ints(0, 2, 0), cd, n_groups=3), "kind 0"),
        ("unknown geometry", ERR_INVALID, lambda: md.set_pull_(g, ints(1, 3, 3), cd, n_groups=3), "geometry 3"),
        ("mask 0", ERR_INVALID, lambda: md.set_pull_(g, ints(0, 4, 0), cd, n_groups=3), "mask 0"),
        ("zero vector", ERR_INVALID, lambda: md.set_pull_(g, ci, dbl(1, slice(3, 6), 0.0), n_groups=3), "direction (0, 0, 0)"),
        ("k nan", ERR_INVALID, lambda: md.set_pull_(g, ci, dbl(0, 0, np.nan), n_groups=3), "nan"),
        ("r0 inf", ERR_INVALID, lambda: md.set_pull_(g, ci, dbl(1, 1, np.inf), n_groups=3), "inf"),
        ("rate nan", ERR_INVALID, lambda: md.set_pull_(g, ci, dbl(1, 2, np.nan), n_groups=3), "rate"),
        ("vector inf", ERR_INVALID, lambda: md.set_pull_(g, ci, dbl(1, 4, np.inf), n_groups=3), "direction"),
        ("k < 0", ERR_INVALID, lambda: md.set_pull_(g, ci, dbl(0, 0, -1.0), n_groups=3), "k = -1"),
        ("rate with a constant force", ERR_INVALID, lambda: md.set_pull_(g, ints(0, 2, CF), cd, n_groups=3), "rate = 0.4"),
        ("NULL group", ERR_INVALID, lambda: raw(None, ci, cd, 2), "NULL"),
        ("NULL coords", ERR_INVALID, lambda: raw(gdev, None, cd, 2), "NULL"),
        ("a log without log_every", ERR_INVALID, lambda: raw(gdev, ci, cd, 2, 0, 4), "log_every = 0"),
        ("negative capacity", ERR_INVALID, lambda: raw(gdev, ci, cd, 2, 1, -1), "log_capacity = -1"),
    ]
    for name, code, call, word in cases:
        text = _refused(E, code, call)
        assert "set_pull" in text and word in text, (name, text)
        assert _read_bits(md) == bits, name
        assert all(torch.equal(a, b) for a, b in zip(md.state().values(), state.values()) if a is not None), name
    md.step_(3, DT)                                                   # the table in force still steps
    assert md.pull()["xi0"][0] == pr.advance(B["coords"][0]["r0"], 0.4, DT, 3)
    md.close()


def test_calls_before_a_state_with_ghosts_and_on_a_lent_engine(emdee, dev):
    E = emdee
    B = _small(E)
    ci, cd = _raw(B["coords"])
    gdev = torch.as_tensor(B["group"], dtype=torch.int32, device=dev)
    md = _small_engine(E, dev, B, table=False)
    h = C.c_void_p()
    three = lambda v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", md._ctx.handle, three([0.0] * 3), three([B["L"]] * 3), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(E.LennardJonesModel(2.5, 2.0)), 0.3, E._lib.F64, C.byref(h))
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_set_pull", h, C.c_void_p(gdev.data_ptr()), 3, ci.ctypes.data_as(C.c_void_p), cd.ctypes.data_as(C.c_void_p), 2, 0, 0)
    assert err.value.code == ERR_STATE and "emdee_md_set_state" in str(err.value) and "set_pull" in str(err.value)
    out = np.zeros(16)
    with pytest.raises(E.EmDeeError) as err:                          # a read without a table
        E._lib.call("emdee_md_pull_read", h, out.ctypes.data_as(C.c_void_p), None)
    assert err.value.code == ERR_STATE and "set_pull" in str(err.value)
    E._lib.call("emdee_md_destroy", h)
    md.close()
    # ghosts: the last 64 atoms of the box loaded as ghosts
    N = B["pos"].shape[0]
    ghosts = E.VelocityVerlet(E.cu(B["pos"], dev), E.cu(B["vel"][:N - 64], dev), B["L"], E.LennardJonesModel(2.5, 2.0), E.cu(B["atoms"], dev),
                              n_ghost=64)
    text = _refused(E, ERR_STATE, ghosts.set_pull_, B["group"][:N - 64], ci, cd, n_groups=3)
    assert "ghosts" in text and "set_pull" in text
    ghosts.close()
    # an engine lent by a decomposition
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)
    pos = pos[np.argsort(gid)]
    n = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((n, 3)), E.lennard_jones_atoms(1.0, 1.0, n), float(lengths[0]))
    eng = dd.engine(0)
    text = _refused(E, ERR_STATE, eng.set_pull_, np.arange(eng.n_owned) % 2, ci[:1], cd[:1], n_groups=2)
    assert "emdee_dd_engine" in text and "set_pull" in text
    dd.step_(2, DT)
    dd.close()


def test_set_state_keeps_the_table_for_the_same_count_and_refuses_for_another(emdee, dev):
    E = emdee
    B = _small(E)
    N = B["pos"].shape[0]
    md = _small_engine(E, dev, B)
    load = lambda n, pos: md.set_state_(E.cu(pos[:n], dev), E.cu(B["vel"][:n], dev), E.cu(B["atoms"][:n], dev),
                                        inv_mass=E.cu(1.0 / B["mass"][:n], dev))
    md.step_(2, DT)
    xi0 = md.pull()["xi0"]
    load(N, B["pos"] + 0.01)                                          # the same count: kept, xi0 as it stood
    read = md.pull()
    assert np.array_equal(read["xi0"], xi0)
    ref = pr.evaluate(B["pos"] + 0.01, B["mass"], B["group"], B["coords"], xi0, 3)
    assert np.abs(read["f"] - ref["words"][:, 2]).max() <= 1e-9 * np.abs(ref["words"][:, 2]).max()
    md.step_(2, DT)
    load(N - 64, B["pos"])                                            # another count: refused until set again or cleared
    for call, args in ((md.step_, (1, DT)), (md.minimize_, (5, 1.0)), (md.pull, ()), (md.scale_box_, (1.01,)), (md.totals, ())):
        text = _refused(E, ERR_STATE, call, *args)
        assert "emdee_md_set_pull" in text, text
    _refused(E, ERR_STATE, md.state)                                  # (forces that were never evaluated)
    _clear(md)
    md.step_(2, DT)
    md.close()


def test_virtual_sites_and_the_heat_flux(emdee, dev):
    E = emdee
    B = _small(E)
    N = B["pos"].shape[0]
    im = 1.0 / B["mass"]
    in1 = np.where(B["group"] == 1)[0]
    free = np.where(B["group"] < 0)[0]
    site_in, site_out = int(in1[0]), int(free[0])
    im[[site_in, site_out]] = 0.0                                     # two massless sites
    parents = [int(t) for t in in1[1:4]]
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, inv_mass=im)
    ci, cd = _raw(B["coords"])
    md.set_vsites_([[site_in, parents[0], parents[1], -1]], [[0.5, 0.0]])
    text = _refused(E, ERR_STATE, md.set_pull_, B["group"], ci, cd, n_groups=3)
    assert "atom %d" % site_in in text and "group 1" in text and "emdee_md_set_vsites" in text and "set_pull" in text
    md.set_vsites_([[site_out, parents[0], parents[1], parents[2]]], [[0.3, 0.3]])
    md.set_pull_(B["group"], ci, cd, n_groups=3)                       # parents may be grouped
    bits = _read_bits(md)
    # the mirror case: a site in a group of the table in force
    text = _refused(E, ERR_INVALID, md.set_vsites_, [[site_in, parents[0], parents[1], -1]], [[0.5, 0.0]])
    assert "atom %d" % site_in in text and "emdee_md_set_pull" in text
    assert _read_bits(md) == bits
    md.step_(2, DT)
    md.close()
    # the Green-Kubo heat flux: refused at set and at sample, naming the setter; the stress is not
    md = _small_engine(E, dev, B, table=False)
    md.set_green_kubo_(8, stress=True, heat=True)
    md.gk_sample_()
    _set(md, B["group"], B["coords"])
    text = _refused(E, ERR_STATE, md.gk_sample_)
    assert "emdee_md_set_pull" in text and "EMDEE_GK_HEAT" in text
    text = _refused(E, ERR_STATE, md.set_green_kubo_, 8, True, True)
    assert "emdee_md_set_pull" in text
    md.set_green_kubo_(8, stress=True, heat=False)
    md.gk_sample_()
    md.close()


# ---------------------------------------------------------------- 7. the example
def test_the_example_runs_at_its_small_size(tmp_path):
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lj_pmf.py"), "--cells", "5", "--melt", "100", "--windows", "3",
                        "--equil", "20", "--steps", "100", "--every", "10"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-1600:]
    rows = [line.split() for line in r.stdout.splitlines() if not line.startswith("#")]
    assert len(rows) == 6 and all(int(row[3]) == 10 for row in rows[:3]), r.stdout[-800:]
    assert all(abs(float(row[1]) - float(row[0])) < 0.5 for row in rows[:3])      # (every window holds the pair near its r0)
