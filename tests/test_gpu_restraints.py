"""GPU tests of the position restraints (include/emdee_hip.h: emdee_md_set_restraints, emdee_md_restraint_sums,
emdee_md_get_restraint_refs): an external field behind every force pass, one thread per table entry, references that follow the
box.  The yardstick is the numpy restatement tests/helpers/restraint_ref.py on the unwrapped positions emdee_md_get_state returns.

Tolerances are those of a post term (tests/test_gpu_bonded.py): the restraint part -- the difference of an engine's outputs with
and without the table -- within 1e-9 (fp64) or 1e-4 (fp32) of the largest reference value; the spring constants are chosen so that
the restraint forces are of the order of the pair forces.  Every box is the smallest on which the kernel can still go wrong."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import GOLDEN, ROOT
from .helpers import image_cases as ic
from .helpers import mask_cases as mc
from .helpers import restraint_ref as rr
from .helpers import settle_ref as sr
from .test_gpu_dd_pairs import _build
from .test_gpu_masks import _engine as _mask_engine
from .test_gpu_masks import _stale_planes
from .test_gpu_settle import _engine as _water_engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
TOL = {np.float64: 1e-9, np.float32: 1e-4}
DT = 0.005
XML = os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml")


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


def _md(E, dev, pos, vel, atoms, lengths, lo=(0.0, 0.0, 0.0), dtype=np.float64, rc=2.5, rs=2.0, skin=0.3, inv_mass=None):
    im = None if inv_mass is None else E.cu(np.asarray(inv_mass).astype(dtype), dev)
    lengths = [float(v) for v in lengths]
    return E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), lengths[0],
                            E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=skin, inv_mass=im, lo=[float(v) for v in lo],
                            lengths=lengths, periodic=[1, 1, 1])


def _outputs(md):
    """forces, energies, virials, per-atom tensors, the twelve box sums"""
    st = md.state(positions=False, velocities=False, energies=True, virials=True)
    return [_np(st["forces"]), _np(st["energies"]), _np(st["virials"]), _np(md.virial_tensor()), np.array(md.tensor_sums())]


def _positions(md):
    return _np(md.state(velocities=False, forces=False)["positions"])


def _bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


_FCC = {}


def _fcc(E, golden):
    """the 864-atom fcc box of the golden set (Float32-rounded once, so that both precisions see the same atoms), and the size of
    its pair forces"""
    if not _FCC:
        pos, L = E.synthetic.fcc_positions(6)
        g = golden["fcc864_expected"]
        assert pos.shape[0] == 864 and float(g["L"]) == L and pos.sum() == float(g["pos_checksum"])
        _FCC.update(pos=pos.astype(np.float32).astype(np.float64), L=L, vel=E.synthetic.velocities(864),
                    atoms=E.lennard_jones_atoms(1.0, 1.0, 864), fmax=float(np.abs(g["forces"]).max()))
    return _FCC


def _table(n, N, fmax, pos, mixed, seed=5):
    """n entries on N atoms, unsorted ids; references the positions plus an offset of up to 0.15 per axis; constants near
    fmax / 0.15, so that the restraint forces are of the order of the pair forces.  mixed: harmonic entries with 1, 2 and 3 axes and
    independent constants, and flat-bottomed spheres, cylinders and slabs, about a third of them inside their well."""
    rng = np.random.default_rng(seed + n)
    ids = rng.permutation(N)[:n] if n < N else rng.permutation(N)
    off = rng.uniform(-0.15, 0.15, (n, 3))
    off[np.abs(off) < 0.02] = 0.02
    k = rng.uniform(0.5, 1.5, (n, 3)) * fmax / 0.15
    flat = np.zeros(n)
    if mixed:
        masks = np.array([(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)], dtype=np.float64)
        m = masks[rng.integers(0, len(masks), n)]
        k *= m
        fb = rng.random(n) < 0.5
        k[fb] = (k[fb].max(axis=1))[:, None] * m[fb]                 # one constant on the masked axes
        rho = np.sqrt((off * off * m).sum(axis=1))
        flat[fb] = rho[fb] * rng.choice([0.5, 0.5, 1.4], int(fb.sum()))   # outside, outside, inside
        assert (flat[fb] > rho[fb]).any() and (flat[fb] < rho[fb]).any()
    return ids, pos[ids] + off, k, flat


# ---------------------------------------------------------------- 1. planes at the load
@pytest.mark.parametrize("n", [1, 257, 864])
@pytest.mark.parametrize("path,dtype", [("brick", np.float64), ("direct", np.float64), ("brick", np.float32)])
def test_planes_at_the_load_match_numpy(emdee, golden, dev, monkeypatch, path, dtype, n):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    B = _fcc(E, golden)
    N, tol = 864, TOL[dtype]
    ids, ref, k, flat = _table(n, N, B["fmax"], B["pos"], mixed=(n == 257))
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, dtype=dtype)
    twin = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, dtype=dtype)
    without = _outputs(md)
    _outputs(twin)
    assert md.restraint_sums().tolist() == [0.0] * 8 and md.restraint_refs().shape == (0, 3)
    for eng in (md, twin):
        eng.set_restraints_(ids, k, ref=ref, flat=flat)
    with_r = _outputs(md)
    x = _positions(md)
    # (a Float32 engine hands back record + cell origin rounded to fp32 again: an ulp of the box side off what it was given)
    assert np.abs(x - B["pos"]).max() <= (0.0 if dtype == np.float64 else float(np.spacing(np.float32(B["L"]))))
    F, U, W, T = rr.planes(N, ids, x, ref, k, flat)
    scale_f = np.abs(F).max()
    assert 0.1 * B["fmax"] <= scale_f <= 10.0 * B["fmax"]             # of the order of the pair forces
    for name, got, want in zip(("forces", "energies", "virials", "tensors"), [a - b for a, b in zip(with_r[:4], without[:4])], (F, U, W, T)):
        err = np.abs(got - want).max() / np.abs(want).max()
        print("%s/%s n = %d, %s: max error / max entry = %.3e (bound %.0e)" % (path, dtype.__name__, n, name, err, tol))
        assert err <= tol, name
    # atoms outside the table keep their bits
    out = np.setdiff1d(np.arange(N), ids)
    for a, b in zip(with_r[:4], without[:4]):
        assert np.array_equal(a[out], b[out])
    # the twelve box sums: W moves by the sum of the tensors, K not at all
    tsum = T.sum(axis=0)
    assert np.abs((with_r[4][:6] - without[4][:6]) - tsum).max() <= tol * np.abs(tsum).max() * 10      # (tests/test_gpu_bonded.py's form)
    assert np.array_equal(with_r[4][6:], without[4][6:])
    ep, _, vir = md.totals()
    assert abs((ep - without[1].sum()) - U.sum()) <= tol * 10 * abs(U.sum())
    assert abs((vir - without[2].sum()) - W.sum()) <= tol * 10 * np.abs(W).sum()
    # the table's own sums, and their bits on a second engine
    got, want = md.restraint_sums(), rr.sums(ids, x, ref, k, flat)
    print("restraint_sums: %s\n         numpy: %s" % (got, want))
    assert np.abs(got[:7] - want[:7]).max() <= tol * np.abs(want[:7]).max() and abs(got[7] - want[7]) <= tol * want[7]
    assert _bits(got) == _bits(twin.restraint_sums())
    assert all(np.array_equal(a, b) for a, b in zip(_outputs(twin), with_r))
    assert np.array_equal(_np(md.restraint_refs()), ref)
    md.close()
    twin.close()


def test_null_references_are_the_current_positions(emdee, golden, dev):
    """ref = None: d = 0 exactly in both precisions (the references are the fp64 unwrapped coordinates the kernels form), so the
    table changes no force, and after steps the sums are those of the displacement from the start"""
    E = emdee
    B = _fcc(E, golden)
    for dtype in (np.float64, np.float32):
        md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, dtype=dtype)
        f0 = md.state()["forces"]
        ids = np.arange(0, 864, 3)
        md.set_restraints_(ids, 40.0)
        assert torch.equal(md.state()["forces"], f0) and md.restraint_sums().tolist() == [0.0] * 8
        refs = _np(md.restraint_refs())
        assert np.abs(refs - B["pos"][ids]).max() <= (0.0 if dtype == np.float64 else 1e-6)
        md.step_(10, DT)
        got, want = md.restraint_sums(), rr.sums(ids, _positions(md), refs, np.full((len(ids), 3), 40.0))
        # (numpy sees the positions get_state rounds to the engine's type: for Float32 an ulp of the box side, 1e-6, on displacements
        # of a few hundredths after ten steps, twice that on U -- ten times the bound of the planes)
        assert got[0] > 0.0 and np.abs(got - want).max() <= TOL[dtype] * 10 * np.abs(want).max()
        md.close()


# ---------------------------------------------------------------- 2. faces and images
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restraint_force_is_continuous_across_faces_images_and_rebuilds(emdee, dev, dtype):
    """Unequal sides at lo != 0, atoms loaded up to three box lengths outside, references on the far side of the upper x face from
    their atoms, which fly at it: some cross it, the list is rebuilt, and the restraint part of the forces is still numpy's on the
    unwrapped positions get_state returns."""
    E = emdee
    box = ic.settle_lj_box(E)
    lo, L = np.array(box["lo"]), np.array(box["lengths"])
    N = box["pos"].shape[0]
    rng = np.random.default_rng(17)
    shift = rng.integers(-3, 4, (N, 3))
    pos = (box["pos"] + shift * L).astype(np.float32).astype(np.float64)
    vel = box["vel"].copy()
    wrapped = lo + np.mod(pos - lo, L)
    hi = lo[0] + L[0]
    near = np.where(hi - wrapped[:, 0] < 0.3)[0]
    assert len(near) >= 8
    vel[near, 0] = 3.0
    others = rng.permutation(np.setdiff1d(np.arange(N), near))[:40]
    ids = np.concatenate([near, others])
    ref = pos[ids] + rng.uniform(-0.1, 0.1, (len(ids), 3))
    ref[:len(near), 0] = pos[near, 0] + 0.8                       # beyond the face
    assert (lo[0] + np.mod(ref[:len(near), 0] - lo[0], L[0]) < wrapped[near, 0]).all()   # (its wrapped image lies at the other end)
    k = np.full((len(ids), 3), 30.0)
    flat = np.where(np.arange(len(ids)) % 3 == 0, 0.05, 0.0)
    md = _md(E, dev, pos, vel, box["atoms"], L, lo=lo, dtype=dtype, rc=box["rc"], rs=box["rs"], skin=box["skin"])
    assert np.abs(_positions(md) - pos).max() <= (0.0 if dtype == np.float64 else float(np.spacing(np.float32(np.abs(pos).max()))))
    md.set_restraints_(ids, k, ref=ref, flat=flat)
    builds = md.nbr_stats()["builds"]
    md.step_(40, DT)
    x = _positions(md)
    crossed = (x[near, 0] - shift[near, 0] * L[0]) >= hi
    assert crossed.any() and md.nbr_stats()["builds"] > builds, (crossed, md.nbr_stats())
    assert np.abs(np.rint((x - pos) / L)).max() == 0                 # (unwrapped: nobody jumped a box length)
    f_with = _np(md.state()["forces"])
    md.set_restraints_(None, 0.0)
    f_without = _np(md.state()["forces"])
    want = rr.planes(N, ids, x, ref, k, flat)[0]
    err = np.abs((f_with - f_without) - want).max() / np.abs(want).max()
    print("%s: %d of %d atoms crossed the face; restraint forces: max error / max entry = %.3e" % (dtype.__name__, crossed.sum(), len(near), err))
    assert err <= TOL[dtype]
    md.close()


# ---------------------------------------------------------------- 3. the integrator
def _lattice(E, seed=23):
    """64 atoms on a 4 x 4 x 4 lattice of spacing 2.0 with rc + skin = 1.5: no pair force acts while the amplitudes stay below
    0.25; unequal masses, harmonic restraints, small displacements and velocities"""
    rng = np.random.default_rng(seed)
    g = (np.arange(4) + 0.5) * 2.0
    ref = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    mass = rng.uniform(1.0, 4.0, 64)
    k = rng.uniform(20.0, 60.0, (64, 3))
    pos = ref + rng.uniform(-0.05, 0.05, (64, 3))
    vel = rng.uniform(-0.2, 0.2, (64, 3))
    amp = np.sqrt((pos - ref) ** 2 + vel ** 2 * mass[:, None] / k)
    assert amp.max() < 0.1
    return dict(ref=ref, mass=mass, k=k, pos=pos, vel=vel, L=8.0, atoms=E.lennard_jones_atoms(1.0, 1.0, 64), ids=rng.permutation(64))


def _lattice_engine(E, dev, B, table=True, pos=None):
    md = _md(E, dev, B["pos"] if pos is None else pos, B["vel"], B["atoms"], [B["L"]] * 3, rc=1.2, rs=1.0, skin=0.3, inv_mass=1.0 / B["mass"])
    if table:
        md.set_restraints_(B["ids"], B["k"][B["ids"]], ref=B["ref"][B["ids"]])
    return md


def test_trajectory_is_the_numpy_velocity_verlet_of_uncoupled_oscillators(emdee, dev):
    """The bound is the one tests/test_gpu_settle.py holds its numpy integrator to (_against_reference): 1e-11 of the box side for
    the positions, 1e-11 of the rms velocity for the velocities."""
    E = emdee
    B = _lattice(E)
    md = _lattice_engine(E, dev, B)
    md.step_(200, DT)
    x, v = B["pos"].copy(), B["vel"].copy()
    w = 1.0 / B["mass"][:, None]
    f = -B["k"] * (x - B["ref"])
    for _ in range(200):
        v += 0.5 * DT * f * w
        x += DT * v
        f = -B["k"] * (x - B["ref"])
        v += 0.5 * DT * f * w
    st = md.state()
    gx, gv, gf = _np(st["positions"]), _np(st["velocities"]), _np(st["forces"])
    vrms = np.sqrt((v * v).sum(axis=1).mean())
    ex, ev = np.abs(gx - x).max(), np.abs(gv - v).max()
    print("200 steps: max |dx| = %.3e (bound %.1e), max |dv| = %.3e (bound %.1e)" % (ex, 1e-11 * B["L"], ev, 1e-11 * vrms))
    assert ex <= 1e-11 * B["L"] and ev <= 1e-11 * vrms
    assert np.abs(gf - f).max() <= 1e-9 * np.abs(f).max()
    assert np.abs(x - B["pos"]).max() > 0.02                          # (it moved)
    md.close()


def test_dealing_of_steps_and_a_cleared_table(emdee, dev):
    E = emdee
    B = _lattice(E)
    ends = []
    for deal in ((40,), (5,) * 8, (1,) * 40):
        md = _lattice_engine(E, dev, B)
        for n in deal:
            md.step_(n, DT)
        ends.append(md.state())
        md.close()
    for other in ends[1:]:
        for key in ("positions", "velocities", "forces"):
            assert torch.equal(ends[0][key], other[key]), key
    # a cleared table: the twin that never had one, bit for bit and launch for launch
    md, twin = _lattice_engine(E, dev, B), _lattice_engine(E, dev, B, table=False)
    md.set_restraints_(None, 0.0)
    for eng in (md, twin):
        eng.profile_(True)
        eng.step_(40, DT)
    a, b = md.state(), twin.state()
    for key in ("positions", "velocities", "forces"):
        assert torch.equal(a[key], b[key]), key
    assert twin.kernel_time("restraints") == (0.0, 0) and md.kernel_time("restraints") == (0.0, 0)
    for name in ("lj_force_nbr", "verlet_kick_drift", "verlet_kick", "lj_force_nbr_fused_step", "rebuild"):
        assert md.kernel_time(name)[1] == twin.kernel_time(name)[1], name
    # with a table: one launch behind every force pass
    md.set_restraints_(B["ids"], B["k"][B["ids"]], ref=B["ref"][B["ids"]])
    md.profile_(True)
    md.step_(7, DT)
    ms, launches = md.kernel_time("restraints")
    assert launches == md.kernel_time("lj_force_nbr")[1] == 7 and ms > 0.0 and md.kernel_time(18) == (ms, launches)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 4. masks
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family,post", [(f, "none") for f in mc.FAMILIES] + [("uniform", "bonded"), ("species3", "tables")])
def test_a_plane_the_mask_leaves_out_keeps_its_bits(emdee, oracle, dev, capfd, monkeypatch, family, post, dtype):
    """every mask on every kernel family with a table in force: the planes asked for hold the whole force field plus the restraint
    term (once), the force plane keeps its bits under a mask without FORCES and under the tensor pass, and the restraint launch runs
    once per pass"""
    E = emdee
    box = mc.family_box(E, family, dtype)
    md, _ = _mask_engine(E, dev, box, dtype, monkeypatch, capfd, post)
    N = box["pos"].shape[0]
    base = mc.reference(oracle, box, post)
    fmax = np.abs(base[0]).max()
    ids, ref, k, flat = _table(min(N, 300), N, fmax, box["pos"], mixed=True)
    md.set_restraints_(ids, k, ref=ref, flat=flat)
    R = rr.planes(N, ids, box["pos"], ref, k, flat)
    want = [base[0] + R[0], base[1] + R[1], base[2] + R[2]]
    tol = 1e-6 if dtype == np.float64 else 1e-4                      # (the whole force field against its fp64 reference)
    md.profile_(True)
    for m in range(1, 8):
        what = "%s/%s mask %d" % (family, post, m)
        _stale_planes(md)
        md.forces_(1)
        f1 = md.state(positions=False, velocities=False)["forces"]
        before = md.kernel_time("restraints")[1]
        md.forces_(m)
        assert md.kernel_time("restraints")[1] == before + 1, what
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


# ---------------------------------------------------------------- 5. pressure and the box
def test_harmonic_virial_scale_box_and_references(emdee, golden, dev):
    E = emdee
    B = _fcc(E, golden)
    L = B["L"]
    ids, ref, k, _ = _table(864, 864, B["fmax"], B["pos"], mixed=False)
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [L] * 3, lo=(0.5, -1.0, 2.0))     # (the box origin is not the coordinate origin)
    lo = np.array([0.5, -1.0, 2.0])
    md.set_restraints_(ids, k, ref=ref)
    s = md.restraint_sums()
    # harmonic: d . f = -2 U entry by entry
    assert abs(s[1] + s[2] + s[3] + 2.0 * s[0]) <= 1e-13 * abs(s[0]) * 4
    mu = np.array([1.013, 0.991, 1.004])
    md.scale_box_(mu)
    x = _positions(md)
    refs = _np(md.restraint_refs())
    want_refs = rr.scale_ref(ref, lo, mu)
    assert np.abs(refs - want_refs).max() <= 4 * 2.0 ** -53 * np.abs(want_refs).max()
    want = rr.sums(ids, x, want_refs, k)
    got = md.restraint_sums()
    print("after scale_box: U = %.12g (numpy %.12g)" % (got[0], want[0]))
    assert abs(got[0] - want[0]) <= 1e-12 * want[0] and np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
    # d -> mu d: U(mu) from the unscaled d
    d0 = B["pos"][ids] - ref
    assert abs(got[0] - 0.5 * (k * (mu * d0) ** 2).sum()) <= 1e-9 * got[0]
    md.close()


def test_molecular_virial_holds_the_restraint_force(emdee, dev):
    """Rigid water with the oxygens restrained under molecular scaling: tr (W_mol with the table - W_mol without) =
    -dU_restr/dmu.  The derivative is a centred difference of restraint_sums()[0] over scale_box(1 +- h), h = 2^-10, on engines
    loaded from one state; an oxygen moves by (mu - 1)(Y - lo) and its reference to lo + mu (ref - lo), so d is linear and U
    quadratic in mu: the difference quotient is exact, and the bound is rounding -- 2^-53 of U per evaluation and sum, a few
    hundred terms, divided by 2h: 64 x 2^-53 U / 2h -- plus the project's bound on the molecular sums (tests/test_gpu_molecular.py
    SUMS = 1e-12 of the largest sum) for the two reads that are subtracted."""
    E = emdee
    B = sr.water_box()
    h = 2.0 ** -10
    ox = B["mol"][:, 0]
    rng = np.random.default_rng(31)
    off = rng.uniform(-0.1, 0.1, (len(ox), 3))
    k = rng.uniform(20.0, 60.0, (len(ox), 3))
    engines = [_water_engine(E, dev, B) for _ in range(3)]
    for md in engines:
        md.set_molecular_scaling_()
    base, up, down = engines
    without = np.array(base.molecular_tensor_sums())
    x0 = _positions(base)
    for md in engines:
        md.set_restraints_(ox, k, ref=x0[ox] + off)
    with_r = np.array(base.molecular_tensor_sums())
    trace = (with_r[:3] - without[:3]).sum()
    up.scale_box_(1.0 + h)
    down.scale_box_(1.0 - h)
    u0, u_up, u_down = base.restraint_sums()[0], up.restraint_sums()[0], down.restraint_sums()[0]
    fd = -(u_up - u_down) / (2.0 * h)
    bound = 64 * 2.0 ** -53 * max(u_up, u_down) / (2.0 * h) + 2e-12 * np.abs(without).max()
    print("tr (W_mol with - without) = %.12g, -dU_restr/dmu = %.12g: difference %.3e (bound %.3e, h = 2^-10, U = %.6g)"
          % (trace, fd, abs(trace - fd), bound, u0))
    assert u0 > 0.0 and abs(trace) > 1e-3 * u0
    assert abs(trace - fd) <= bound
    for md in engines:
        md.close()


@pytest.mark.parametrize("kind", ["berendsen", "c-rescale"])
def test_coupled_runs_do_not_depend_on_the_dealing_and_the_references_follow(emdee, golden, dev, kind):
    E = emdee
    B = _fcc(E, golden)
    L = B["L"]
    ids, ref, k, _ = _table(257, 864, B["fmax"], B["pos"], mixed=False)
    ends = []
    for deal in ((20,), (5,) * 4, (1,) * 20, (7, 13)):
        md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [L] * 3)
        md.set_restraints_(ids, k, ref=ref)
        md.set_barostat_(kind, p_ref=2.0, compressibility=0.05, tau_p=0.5, every=5, temperature=1.0, seed=11)
        lengths, done = [np.array(md.box()[1])], 0
        for n in deal:
            md.step_(n, DT)
            done += n
            if done % 5 == 0 and deal != (7, 13):
                lengths.append(np.array(md.box()[1]))
        st = md.state()
        ends.append((st, _np(md.restraint_refs()), md.restraint_sums(), lengths, np.array(md.box()[1])))
        md.close()
    for st, refs, sums, _, box in ends[1:]:
        for key in ("positions", "velocities", "forces"):
            assert torch.equal(ends[0][0][key], st[key]), key
        assert np.array_equal(refs, ends[0][1]) and _bits(sums) == _bits(ends[0][2]) and np.array_equal(box, ends[0][4])
    # the factors of the four events, replayed: lo = 0, so ref <- mu ref
    lengths = ends[1][3]
    assert len(lengths) == 5 and not np.array_equal(lengths[0], lengths[-1])
    want = ref.copy()
    for a, b in zip(lengths[:-1], lengths[1:]):
        want = rr.scale_ref(want, np.zeros(3), b / a)
    # (b / a is the event's factor to one rounding, the product another: three roundings per event)
    assert np.abs(ends[0][1] - want).max() <= 4 * 3 * 2.0 ** -53 * np.abs(want).max()


# ---------------------------------------------------------------- 6. minimise
def test_minimize_ends_within_f_tol_over_k_of_the_references(emdee, dev):
    E = emdee
    B = _lattice(E)
    rng = np.random.default_rng(37)
    md = _lattice_engine(E, dev, B, pos=B["ref"] + rng.uniform(-0.2, 0.2, (64, 3)))
    f_tol = 1e-6
    res = md.minimize_(5000, f_tol, dt_start=0.01, dt_max=0.1, max_step=0.1)
    x = _positions(md)
    gap = np.abs(x - B["ref"]) * B["k"]
    print("minimised in %d iterations: largest k |x - ref| = %.3e (f_tol %.0e), restraint energy %.3e" % (res.iterations, gap.max(), f_tol, md.restraint_sums()[0]))
    assert res.converged
    assert (np.sqrt((gap * gap).sum(axis=1)) <= f_tol * (1.0 + 1e-9)).all()
    assert (np.abs(x - B["ref"]) <= f_tol / B["k"] * (1.0 + 1e-9)).all()
    md.close()


def _solute_engine(E, dev, cells=6):
    """the box of examples/minimize_solute.py: the fixture's solute drawn flat in a lattice of water, rigid waters, the solute's
    C-H bonds fixed, the harmonic terms the two tables replace taken out -> engine, dict(types, table, mol, geom, clusters, dist, n_solute, L)"""
    from .helpers import ring_cases as rc
    ing = E.ingest
    box = rc.solute_box(E, XML, cells=cells, corner=False)
    table, templates, nonbonded = ing.BondedTable(XML), ing.ResidueTemplates(XML), ing.NonbondedTable(XML)
    sequence = ["aaa"] + ["HOH"] * box["n_water"]
    types, bonds = templates.build(sequence)
    mol, geom, drop_b, drop_a = ing.rigid_triatomics(types, bonds, table, with_dropped=True)
    clusters, dist, drop_h = ing.hydrogen_clusters(types, bonds, table, skip=mol, with_dropped=True)

    def without(rows, params, drop):
        gone = {tuple(r) for r in np.asarray(drop).tolist()}
        sel = np.array([tuple(r) not in gone for r in rows.tolist()], dtype=bool)
        return rows[sel], params[sel]
    terms = {kind: (a, p) for kind, a, p in box["terms"]}
    N = len(types)
    md = _md(E, dev, box["positions"], np.zeros((N, 3)), box["atoms"], [box["L"]] * 3, rc=0.8, rs=0.7, skin=0.1, inv_mass=box["inv_mass"])
    md.set_exclusions_(box["exclusions"])
    md.set_pairs14_(box["pairs14"], box["lj14scale"])
    md.set_bonded_(E.HARMONIC_BOND, *without(*terms[1], np.concatenate([drop_b, drop_h])))
    md.set_bonded_(E.HARMONIC_ANGLE, *without(*terms[2], drop_a))
    md.set_bonded_(E.PERIODIC_TORSION, *terms[3])
    md.set_coulomb_(templates.charges(sequence), E.COULOMB_K_KJ_NM, eps_rf=78.0, coulomb14scale=nonbonded.coulomb14scale)
    md.set_rigid3_(mol, geom)
    md.set_hbonds_(clusters, dist)
    return md, dict(types=types, table=table, mol=mol, geom=geom, clusters=clusters, dist=dist, n_solute=box["n_solute"], L=box["L"],
                    pos=box["positions"])


def test_minimize_with_the_solutes_heavy_atoms_restrained(emdee, dev):
    E = emdee
    rms, worst = {}, {}
    for restrained in (False, True):
        md, S = _solute_engine(E, dev)
        heavy = E.ingest.heavy_atoms(S["types"], S["table"], skip=S["mol"])
        assert len(heavy) == 14 and heavy.max() < S["n_solute"]
        if restrained:
            md.set_restraints_(heavy, 1000.0)                           # kJ/mol/nm^2, the usual constant
        md.minimize_(300, 200.0, dt_start=0.0002, dt_max=0.002, max_step=0.01)
        x = _positions(md)
        d = x[heavy] - S["pos"][heavy]
        rms[restrained] = np.sqrt((d * d).sum(axis=1).mean())
        dev_ = 0.0
        for i, j, want in ([(S["mol"][:, 0], S["mol"][:, 1], S["geom"][:, 0]), (S["mol"][:, 0], S["mol"][:, 2], S["geom"][:, 0]),
                            (S["mol"][:, 1], S["mol"][:, 2], S["geom"][:, 1])]
                           + [(S["clusters"][S["clusters"][:, c] >= 0, 0], S["clusters"][S["clusters"][:, c] >= 0, c],
                               S["dist"][S["clusters"][:, c] >= 0, c - 1]) for c in (1, 2, 3)]):
            if len(i):
                r = x[i] - x[j]
                r -= S["L"] * np.rint(r / S["L"])
                dev_ = max(dev_, np.abs(np.linalg.norm(r, axis=1) / want - 1.0).max())
        worst[restrained] = dev_
        if restrained:
            s = md.restraint_sums()
            assert s[0] > 0.0 and abs(s[7] - np.sqrt((d * d).sum(axis=1)).max()) <= 1e-9
        md.close()
    print("rms displacement of the solute's heavy atoms: %.4f nm free, %.4f nm restrained; constraint deviations %.1e, %.1e"
          % (rms[False], rms[True], worst[False], worst[True]))
    assert rms[True] < rms[False]
    assert worst[True] < 1e-10 and worst[False] < 1e-10              # (examples/minimize_solute.py's bound)


# ---------------------------------------------------------------- 7. refusals and lifetimes
def test_every_refusal_leaves_the_previous_table_in_force(emdee, golden, dev):
    E = emdee
    B = _fcc(E, golden)
    N = 864
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3)
    ids, ref, k, flat = _table(40, N, B["fmax"], B["pos"], mixed=True)
    md.set_restraints_(ids, k, ref=ref, flat=flat)
    bits, state = _bits(md.restraint_sums()), md.state()
    i3 = torch.tensor([5, 6, 7], dtype=torch.int32, device=dev)
    k3 = torch.full((3, 3), 2.0, dtype=torch.float64, device=dev)
    handle = md._handle

    def raw(atoms, ref_, k_, flat_, n):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        E._lib.call("emdee_md_set_restraints", handle, p(atoms), p(ref_), p(k_), p(flat_), n)
    bad = lambda row, col, v: [[v if (r, c) == (row, col) else 2.0 for c in range(3)] for r in range(3)]
    cases = [
        ("NULL atoms", ERR_INVALID, lambda: raw(None, None, k3, None, 3), "NULL"),
        ("NULL k", ERR_INVALID, lambda: raw(i3, None, None, None, 3), "NULL"),
        ("n < 0", ERR_INVALID, lambda: raw(i3, None, k3, None, -1), "negative"),
        ("id outside", ERR_INVALID, lambda: md.set_restraints_([5, N, 7], 2.0), "entry 1"),
        ("id negative", ERR_INVALID, lambda: md.set_restraints_([-1, 6, 7], 2.0), "entry 0"),
        ("named twice", ERR_INVALID, lambda: md.set_restraints_([5, 6, 5], 2.0), "atom 5"),
        ("k negative", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], bad(1, 2, -1.0)), "entry 1"),
        ("k nan", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], bad(2, 0, float("nan"))), "entry 2"),
        ("k inf", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], bad(0, 0, float("inf"))), "entry 0"),
        ("r0 negative", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], 2.0, flat=[0.0, -1.0, 0.0]), "entry 1"),
        ("r0 nan", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], 2.0, flat=[0.0, 0.0, float("nan")]), "entry 2"),
        ("ref inf", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], 2.0, ref=bad(1, 1, float("inf"))), "entry 1"),
        ("ref nan", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], 2.0, ref=bad(2, 1, float("nan"))), "entry 2"),
        ("flat, unequal", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], [[2.0, 3.0, 0.0]] * 3, flat=[0.0, 0.5, 0.0]), "unequal"),
        ("flat, no constant", ERR_INVALID, lambda: md.set_restraints_([5, 6, 7], [[2.0] * 3, [2.0] * 3, [0.0] * 3], flat=[0.0, 0.0, 0.5]), "no non-zero"),
    ]
    for name, code, call, word in cases:
        text = _refused(E, code, call)
        assert word in text, (name, text)
        assert _bits(md.restraint_sums()) == bits, name
        assert all(torch.equal(a, b) for a, b in zip(md.state().values(), state.values()) if a is not None), name
    md.step_(3, DT)                                                   # the table still steps
    assert md.restraint_sums()[0] > 0.0
    md.close()


def test_calls_before_a_state_with_ghosts_and_on_a_lent_engine(emdee, golden, dev):
    E = emdee
    B = _fcc(E, golden)
    # before emdee_md_set_state
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3)
    h = C.c_void_p()
    three = lambda v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", md._ctx.handle, three([0.0] * 3), three([B["L"]] * 3), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(E.LennardJonesModel(2.5, 2.0)), 0.3, E._lib.F64, C.byref(h))
    i3 = torch.tensor([5, 6, 7], dtype=torch.int32, device=dev)
    k3 = torch.full((3, 3), 2.0, dtype=torch.float64, device=dev)
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_set_restraints", h, C.c_void_p(i3.data_ptr()), None, C.c_void_p(k3.data_ptr()), None, 3)
    assert err.value.code == ERR_STATE and "emdee_md_set_state" in str(err.value)
    out = np.zeros(8)
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_restraint_sums", h, out.ctypes.data_as(C.c_void_p))
    assert err.value.code == ERR_STATE
    E._lib.call("emdee_md_destroy", h)
    md.close()
    # ghosts: the last 64 atoms of the box loaded as ghosts
    ghosts = E.VelocityVerlet(E.cu(B["pos"], dev), E.cu(B["vel"][:800], dev), B["L"], E.LennardJonesModel(2.5, 2.0), E.cu(B["atoms"], dev),
                              n_ghost=64)
    text = _refused(E, ERR_STATE, ghosts.set_restraints_, [5, 6, 7], 2.0)
    assert "ghosts" in text
    ghosts.close()
    # an engine lent by a decomposition
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)
    pos = pos[np.argsort(gid)]
    n = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((n, 3)), E.lennard_jones_atoms(1.0, 1.0, n), float(lengths[0]))
    text = _refused(E, ERR_STATE, dd.engine(0).set_restraints_, [0, 1, 2], 2.0)
    assert "emdee_dd_engine" in text
    dd.step_(2, DT)
    dd.close()


def test_set_state_keeps_the_table_for_the_same_count_and_refuses_for_another(emdee, golden, dev):
    E = emdee
    B = _fcc(E, golden)
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3)
    ids, ref, k, flat = _table(40, 800, B["fmax"], B["pos"], mixed=True)
    md.set_restraints_(ids, k, ref=ref, flat=flat)
    load = lambda n, pos: md.set_state_(E.cu(pos[:n], dev), E.cu(B["vel"][:n], dev), E.cu(B["atoms"][:n], dev))
    moved = B["pos"] + 0.01
    load(864, moved)
    assert np.array_equal(_np(md.restraint_refs()), ref)              # kept
    want = rr.sums(ids, moved, ref, k, flat)
    assert np.abs(md.restraint_sums() - want).max() <= 1e-9 * np.abs(want).max()
    md.step_(2, DT)
    # another count: step, minimise and the reads refuse until the table is set again or cleared
    load(800, B["pos"])
    for call, args in ((md.step_, (1, DT)), (md.minimize_, (5, 1.0)), (md.restraint_sums, ()), (md.restraint_refs, ()),
                       (md.scale_box_, (1.01,)), (md.totals, ())):
        text = _refused(E, ERR_STATE, call, *args)
        assert "emdee_md_set_restraints" in text, text
    _refused(E, ERR_STATE, md.state)                                  # (forces that were never evaluated)
    assert np.array_equal(_positions(md), B["pos"][:800])             # (positions alone are the state's)
    md.set_restraints_(ids, k, ref=ref, flat=flat)                    # set again: for 800 atoms now
    md.step_(2, DT)
    load(864, B["pos"])
    _refused(E, ERR_STATE, md.step_, 1, DT)
    md.set_restraints_(None, 0.0)                                     # or cleared
    md.step_(2, DT)
    assert md.restraint_sums().tolist() == [0.0] * 8
    md.close()


def test_virtual_sites_and_the_heat_flux(emdee, golden, dev):
    E = emdee
    B = _fcc(E, golden)
    im = np.ones(864)
    im[[100, 200]] = 0.0                                              # two massless sites
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3, inv_mass=im)
    sites = [[100, 101, 102, -1], [200, 201, 202, 203]]
    weights = [[0.5, 0.0], [0.3, 0.3]]
    md.set_vsites_(sites, weights)
    text = _refused(E, ERR_STATE, md.set_restraints_, [5, 200, 7], 2.0)
    assert "atom 200" in text and "entry 1" in text and "emdee_md_set_vsites" in text
    md.set_restraints_([5, 201, 7], 2.0)                              # a parent may be restrained
    bits = _bits(md.restraint_sums())
    # the mirror case: a site the restraint table names
    md.set_vsites_(None, None)
    md.set_restraints_([5, 100, 7], 2.0)
    text = _refused(E, ERR_INVALID, md.set_vsites_, sites, weights)
    assert "atom 100" in text and "emdee_md_set_restraints" in text
    md.set_restraints_([5, 201, 7], 2.0)
    md.set_vsites_(sites, weights)                                    # ... and without it the same table is taken
    assert _bits(md.restraint_sums()) == bits
    md.close()
    # the Green-Kubo heat flux: refused at set and at sample, naming the setter; the stress is not
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], [B["L"]] * 3)
    md.set_green_kubo_(8, stress=True, heat=True)
    md.gk_sample_()
    md.set_restraints_([5, 6, 7], 2.0, ref=B["pos"][[5, 6, 7]] + 0.1)
    text = _refused(E, ERR_STATE, md.gk_sample_)
    assert "emdee_md_set_restraints" in text and "EMDEE_GK_HEAT" in text
    text = _refused(E, ERR_STATE, md.set_green_kubo_, 8, True, True)
    assert "emdee_md_set_restraints" in text
    md.set_green_kubo_(8, stress=True, heat=False)
    md.gk_sample_()
    md.close()


# ---------------------------------------------------------------- 8. the example
def test_the_example_runs_at_its_small_size(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "restrained_solute.py"), "6", "100"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-1600:]
    assert "restraint energy" in r.stdout and "released" in r.stdout, r.stdout[-800:]
