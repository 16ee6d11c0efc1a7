"""GPU tests of the soft-core alchemical decoupling (include/emdee_hip.h: emdee_md_set_alchemical, emdee_md_set_lambda,
emdee_md_alchemical_read, emdee_md_alchemical_log_read): the cross entries leave the neighbour rows after every build and one launch
behind every force pass evaluates them through the soft core, owner-computes, no atomics.  The yardstick is the numpy restatement
tests/helpers/alchemical_ref.py, an O(N^2) sum over the positions emdee_md_get_state returns; it never calls the library.

Tolerances are those of tests/test_gpu_pull.py: max error over max entry within 1e-9 (fp64) or 1e-4 (fp32).  Every box is the
2916-atom fcc box of that file, or smaller."""
import ctypes as C

import numpy as np
import pytest

from .helpers import alchemical_ref as ar
from .helpers import coulomb_ref as cr
from .helpers import pme_ref as pm
from .helpers import settle_ref as sr
from .test_gpu_dd_pairs import _build
from .test_gpu_molecular import _constraints_hold_on
from .test_gpu_settle import _engine as _water_engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
TOL = {np.float64: 1e-9, np.float32: 1e-4}
DT = 0.005
RC, RS, SKIN, ALPHA = 2.5, 2.0, 0.3, 0.5
FOREIGN = [0.0, 0.3, 0.6, 0.85, 1.0]


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


def _md(E, dev, pos, vel, atoms, L, dtype=np.float64, inv_mass=None):
    im = None if inv_mass is None else E.cu(np.asarray(inv_mass).astype(dtype), dev)
    return E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), float(L),
                            E.LennardJonesModel(RC, RS), E.cu(atoms, dev), skin=SKIN, inv_mass=im, lo=[0.0, 0.0, 0.0],
                            lengths=[float(L)] * 3, periodic=[1, 1, 1])


def _outputs(md):
    """forces, energies, virials, per-atom tensors, the twelve box sums"""
    st = md.state(positions=False, velocities=False, energies=True, virials=True)
    return [_np(st["forces"]), _np(st["energies"]), _np(st["virials"]), _np(md.virial_tensor()), np.array(md.tensor_sums())]


def _xv(md):
    st = md.state(forces=False)
    return _np(st["positions"]), _np(st["velocities"])


def _err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


# ---------------------------------------------------------------- the box
_BOX = {}


def _fluid(E):
    """synthetic.fcc_positions(9): 2916 atoms (Float32-rounded once, so that both precisions see the same atoms), unequal masses.
    The solute is 9 flagged atoms with sigma = 1.2 and eps = 0.7 against 1 and 1: the atom nearest the middle of the box with its 7
    nearest neighbours (flagged-flagged pairs exist), and one more atom just above the lower x face, flying at it."""
    if not _BOX:
        pos, L = E.synthetic.fcc_positions(9)
        N = pos.shape[0]
        assert N == 2916
        pos = pos.astype(np.float32).astype(np.float64)
        rng = np.random.default_rng(101)
        mass = rng.uniform(1.0, 4.0, N)
        c = int(np.argmin(((pos - 0.5 * L) ** 2).sum(axis=1)))
        near = np.argsort(((pos - pos[c]) ** 2).sum(axis=1))[:8]
        low = np.where((pos[:, 0] > 0.02) & (pos[:, 0] < 0.2))[0]
        flyer = int(low[0])
        flag = np.zeros(N, dtype=np.int32)
        flag[near], flag[flyer] = 1, 1
        assert flag.sum() == 9
        vel = E.synthetic.velocities(N) / np.sqrt(mass)[:, None]
        vel[flyer, 0] = -3.0
        atoms = E.lennard_jones_atoms(np.where(flag == 1, 0.7, 1.0), np.where(flag == 1, 1.2, 1.0))
        _BOX.update(pos=pos, L=L, vel=vel, mass=mass, flag=flag, flyer=flyer, atoms=atoms, cluster=near)
    return _BOX


def _engine(E, dev, B, dtype=np.float64, lam=None, masses=True, **kw):
    md = _md(E, dev, B["pos"], B["vel"], B["atoms"], B["L"], dtype=dtype, inv_mass=1.0 / B["mass"] if masses else None)
    if lam is not None:
        md.set_alchemical_(B["flag"], lam=lam, alpha=ALPHA, **kw)
    return md


def _reference(B, x, lam, flag=None, excl=None):
    return ar.system(x, [B["L"]] * 3, RC, RS, B["atoms"]["half_sigma"], B["atoms"]["twice_sqrt_eps"], B["flag"] if flag is None else flag,
                     lam, ALPHA, excl=excl)


def _check_planes(md, B, lam, dtype, what, extra=None, excl=None, mass=None):
    """every output against numpy at the engine's own positions (extra: (f, e, w, t) of terms the yardstick lacks: Coulomb)"""
    tol = TOL[dtype]
    out = _outputs(md)
    x, v = _xv(md)
    ref = _reference(B, x, lam, excl=excl)
    want = [ref["forces"], ref["energies"], ref["virials"], ref["tensors"]]
    if extra is not None:
        want = [a + b for a, b in zip(want, extra(x))]
    for name, got, w in zip(("forces", "energies", "virials", "tensors"), out[:4], want):
        err = _err(got, w)
        print("%s, lambda %.2f, %s: max error / max entry = %.3e (bound %.0e)" % (what, lam, name, err, tol))
        assert err <= tol, (what, lam, name)
    # the forces sum to zero within the tolerance (to the yardstick's own sum where a mesh is in play: it does not conserve momentum)
    total = out[0].sum(axis=0)
    print("%s, lambda %.2f: sum of the forces %s (largest %.3f)" % (what, lam, total, np.abs(want[0]).max()))
    assert np.abs(ref["forces"].sum(axis=0)).max() <= 1e-12 * np.abs(ref["forces"]).max()
    assert np.abs(total - (want[0].sum(axis=0) if extra is not None else 0.0)).max() <= tol * np.abs(want[0]).max()
    # the twelve box sums: W from the tensors, K from the velocities
    m = B["mass"] if mass is None else mass
    K = np.array([(m * v[:, a] * v[:, b]).sum() for a, b in ar.COMPONENTS])
    wsum = want[3].sum(axis=0)
    assert np.abs(out[4][:6] - wsum).max() <= 10 * tol * np.abs(wsum).max()       # (tests/test_gpu_bonded.py's form)
    assert np.abs(out[4][6:] - K).max() <= 10 * tol * np.abs(K).max()
    # the read: U_alch, dU/dlambda and the cross virial within the tolerance of their sizes, the pair count exactly
    read = md.alchemical()
    assert read["lam"] == lam and read["pairs"] == ref["pairs"] and ref["pairs"] > 300, (read["pairs"], ref["pairs"])
    size = dict(U=ref["sizes"][0], dUdl=ref["sizes"][1], virial=ref["sizes"][2])
    for key, r in (("U", ref["U"]), ("dUdl", ref["dUdl"]), ("virial", ref["W"])):
        print("%s, lambda %.2f, read %s: %.9g against %.9g" % (what, lam, key, read[key], r))
        assert abs(read[key] - r) <= tol * size[key], (what, lam, key)
    if lam == 0.0:
        assert read["U"] == 0.0 and read["virial"] == 0.0
    return out, ref


CASES = [("brick", np.float64, True), ("direct", np.float64, True), ("brick", np.float32, True), ("brick", np.float32, False)]


# ---------------------------------------------------------------- 1. planes against numpy
@pytest.mark.parametrize("path,dtype,masses", CASES)
def test_planes_at_the_load_and_after_a_rebuild_and_a_face_match_numpy(emdee, dev, monkeypatch, path, dtype, masses):
    """(the fourth case: a Float32 engine without masses keeps cell-relative records)"""
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    B = _fluid(E)
    md = _engine(E, dev, B, dtype=dtype, lam=1.0, masses=masses, foreign=FOREIGN)
    what = "%s/%s%s" % (path, dtype.__name__, "" if masses else "/no masses")
    mass = B["mass"] if masses else np.ones(len(B["mass"]))
    for lam in (1.0, 0.6, 0.0):
        md.set_lambda_(lam)
        _check_planes(md, B, lam, dtype, what + " at the load", mass=mass)
    builds, image0 = md.nbr_stats()["builds"], np.floor(B["pos"] / B["L"])
    md.set_lambda_(0.6)
    md.step_(40, DT)
    x, _ = _xv(md)
    crossed = (np.floor(x / B["L"]) != image0).any(axis=1) & (B["flag"] == 1)
    assert crossed.any() and md.nbr_stats()["builds"] > builds, (crossed.sum(), md.nbr_stats())
    assert np.isfinite(x).all() and np.abs(x - B["pos"]).max() < 2.0
    for lam in (0.6, 1.0, 0.0):
        md.set_lambda_(lam)
        _check_planes(md, B, lam, dtype, what + " after 40 steps", mass=mass)
    md.close()


# ---------------------------------------------------------------- 2. against the engine itself
@pytest.mark.parametrize("path,dtype,masses", CASES[:3])
def test_lambda_one_is_the_engine_without_a_table_and_lambda_zero_the_engine_without_the_solute(emdee, dev, monkeypatch, path, dtype, masses):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    B = _fluid(E)
    tol = TOL[dtype]
    md, plain = _engine(E, dev, B, dtype=dtype, lam=1.0), _engine(E, dev, B, dtype=dtype)
    for name, a, b in zip(("forces", "energies", "virials", "tensors", "sums"), _outputs(md), _outputs(plain)):
        err = _err(a, b)
        print("%s/%s lambda 1 against no table, %s: %.3e (bound %.0e; not bit for bit: the summation is split)" % (path, dtype.__name__, name, err, tol))
        assert err <= tol, name
    plain.close()
    env = B["flag"] == 0
    without = _md(E, dev, B["pos"][env], B["vel"][env], B["atoms"][env], B["L"], dtype=dtype, inv_mass=1.0 / B["mass"][env])
    md.set_lambda_(0.0)
    for name, a, b in zip(("forces", "energies", "virials", "tensors"), _outputs(md)[:4], _outputs(without)[:4]):
        err = _err(a[env], b)
        print("%s/%s lambda 0 against the box without the solute, %s: %.3e (bound %.0e)" % (path, dtype.__name__, name, err, tol))
        assert err <= tol, name
    without.close()
    md.close()


def test_dUdlambda_is_the_centred_difference_of_U_alch_through_set_lambda(emdee, dev):
    """At fixed positions (U(lambda + h) - U(lambda - h)) / 2h errs by h^2 / 6 |U'''| -- from the fp64 yardstick's sum over the cross
    pairs by a five-point stencil of step 2 h, doubled for the stencil's own error, as on the host -- plus the rounding of the two
    reads, 1e-9 (the tolerance of a read) of the size of U before cancellation, over 2 h."""
    E = emdee
    B = _fluid(E)
    md = _engine(E, dev, B, lam=0.5)
    x, _ = _xv(md)
    r2, s2, e4 = ar.cross_pairs(x, [B["L"]] * 3, RC, B["atoms"]["half_sigma"], B["atoms"]["twice_sqrt_eps"], B["flag"])
    U = lambda lam: float(ar.pair(r2, RC, RS, s2, e4, lam, ALPHA)[0].sum())
    h = 2.0 ** -7
    for lam in (0.2, 0.5, 0.8):
        md.set_lambda_(lam)
        here = md.alchemical()
        md.set_lambda_(lam + h)
        up = md.alchemical()["U"]
        md.set_lambda_(lam - h)
        dn = md.alchemical()["U"]
        k = 2 * h
        third = max(abs(U(c + 2 * k) - 2 * U(c + k) + 2 * U(c - k) - U(c - 2 * k)) / (2 * k ** 3) for c in (lam - k, lam, lam + k))
        size = float(np.abs(ar.pair(r2, RC, RS, s2, e4, lam + h, ALPHA)[0]).sum())
        bound = 2.0 * h * h / 6.0 * third + 2 * TOL[np.float64] * size / (2 * h)
        slope = (up - dn) / (2 * h)
        print("lambda %.2f: dU/dlambda read %.9g, centred difference %.9g, bound %.3e" % (lam, here["dUdl"], slope, bound))
        assert abs(slope - here["dUdl"]) <= bound
    md.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_foreign_energies_are_the_reads_of_a_twin_at_those_lambdas(emdee, dev, dtype):
    E = emdee
    B = _fluid(E)
    foreign = [k / 15.0 for k in range(16)]                          # sixteen: both halves of the sums
    md, twin = _engine(E, dev, B, dtype=dtype, lam=0.4, foreign=foreign), _engine(E, dev, B, dtype=dtype, lam=0.4)
    got = md.alchemical()["foreign"]
    assert got.shape == (16,)
    x, _ = _xv(md)
    r2, s2, e4 = ar.cross_pairs(x, [B["L"]] * 3, RC, B["atoms"]["half_sigma"], B["atoms"]["twice_sqrt_eps"], B["flag"])
    for k, lam in enumerate(foreign):
        twin.set_lambda_(lam)
        want = twin.alchemical()["U"]
        size = float(np.abs(ar.pair(r2, RC, RS, s2, e4, lam, ALPHA)[0]).sum())
        assert abs(got[k] - want) <= TOL[dtype] * max(size, 1e-300), (k, got[k], want)
    assert got[0] == 0.0 and abs(got[15]) > 1.0
    md.close()
    twin.close()


# ---------------------------------------------------------------- 3. overlap
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_overlapping_atoms_stay_finite_under_the_soft_core(emdee, dev, dtype):
    """one unflagged atom exactly on a flagged one, another 1e-3 sigma from a flagged one (the flyer, far from the first: the two
    unflagged atoms must not overlap each other, their pair is the plain one); nothing is asked of an engine without a table here"""
    E = emdee
    B = _fluid(E)
    pos = B["pos"].copy()
    s, s2 = int(B["cluster"][0]), int(B["flyer"])
    free = np.where(B["flag"] == 0)[0]
    far = free[np.argsort(-((pos[free] - pos[s]) ** 2).sum(axis=1))[:2]]
    on, close = int(far[0]), int(far[1])
    pos[on] = pos[s]
    pos[close] = pos[s2] + np.array([1e-3, 0.0, 0.0])
    pos = pos.astype(np.float32).astype(np.float64)
    assert (pos[on] == pos[s]).all() and 0.0 < pos[close][0] - pos[s2][0] < 2e-3
    # (loaded with lambda = 0.5 from the start: set_state evaluates the plain force field of the overlap first, whose NaNs a force
    # pass overwrites)
    md = _md(E, dev, pos, np.zeros_like(pos), B["atoms"], B["L"], dtype=dtype, inv_mass=1.0 / B["mass"])
    md.set_alchemical_(B["flag"], lam=0.5, alpha=ALPHA, foreign=FOREIGN)
    out = _outputs(md)
    for name, a in zip(("forces", "energies", "virials", "tensors", "sums"), out):
        assert np.isfinite(a).all(), name
    read = md.alchemical()
    assert all(np.isfinite(read[k]) for k in ("U", "dUdl", "virial")) and np.isfinite(read["foreign"][:4]).all()
    # the coincident pair contributes no force: the forces match numpy, whose coincident pair has d = 0
    ref = ar.system(pos, [B["L"]] * 3, RC, RS, B["atoms"]["half_sigma"], B["atoms"]["twice_sqrt_eps"], B["flag"], 0.5, ALPHA)
    assert np.isfinite(ref["forces"]).all()
    assert _err(out[0], ref["forces"]) <= TOL[dtype]
    md.minimize_(50, 1e-3, dt_start=0.0005, dt_max=0.005, max_step=0.05)
    md.step_(20, 0.001)
    x, v = _xv(md)
    assert np.isfinite(x).all() and np.isfinite(v).all() and all(np.isfinite(a).all() for a in _outputs(md))
    md.close()


# ---------------------------------------------------------------- 4. reproducibility
def _small(E):
    """the 864-atom fcc box with a solute of three neighbouring atoms"""
    pos, L = E.synthetic.fcc_positions(6)
    N = pos.shape[0]
    rng = np.random.default_rng(103)
    mass = rng.uniform(1.0, 3.0, N)
    c = int(np.argmin(((pos - 0.5 * L) ** 2).sum(axis=1)))
    flag = np.zeros(N, dtype=np.int32)
    flag[np.argsort(((pos - pos[c]) ** 2).sum(axis=1))[:3]] = 1
    atoms = E.lennard_jones_atoms(np.where(flag == 1, 0.7, 1.0), np.where(flag == 1, 1.2, 1.0))
    return dict(pos=pos, vel=E.synthetic.velocities(N) / np.sqrt(mass)[:, None], mass=mass, flag=flag, L=L, atoms=atoms)


def _read_bits(md):
    r = md.alchemical()
    return np.array([r["lam"], r["U"], r["dUdl"], r["virial"], float(r["pairs"])]).tobytes() + r["foreign"].tobytes()


def test_dealing_of_steps_fresh_engines_and_a_cleared_table(emdee, dev):
    E = emdee
    B = _small(E)
    ends = []
    for deal in ((40,), (5,) * 8, (1,) * 40, (40,)):                   # (the last: a second fresh engine)
        md = _engine(E, dev, B, lam=0.9, foreign=FOREIGN, log_every=4, log_capacity=32)
        for lam in (0.9, 0.55, 0.2):                                   # lambda moves between the calls, on a fixed schedule
            md.set_lambda_(lam)
            for n in deal:
                md.step_(n, DT)
        log = md.alchemical_log()
        ends.append((md.state(), _read_bits(md), log["dUdl"].tobytes() + log["U"].tobytes() + log["foreign"].tobytes(),
                     (log["count"], log["dropped"])))
        md.close()
    assert ends[0][3] == (30, 0)
    for other in ends[1:]:
        for key in ("positions", "velocities", "forces"):
            assert torch.equal(ends[0][0][key], other[0][key]), key
        assert ends[0][1] == other[1] and ends[0][2] == other[2] and ends[0][3] == other[3]
    # a table set and cleared: the twin that never had one, bit for bit and launch for launch
    md, twin = _engine(E, dev, B, lam=0.5), _engine(E, dev, B)
    md.set_alchemical_(None)
    for eng in (md, twin):
        eng.profile_(True)
        eng.step_(40, DT)
    a, b = md.state(), twin.state()
    for key in ("positions", "velocities", "forces"):
        assert torch.equal(a[key], b[key]), key
    assert twin.kernel_time("alchemical") == (0.0, 0) and md.kernel_time("alchemical") == (0.0, 0)
    for name in ("lj_force_nbr", "verlet_kick_drift", "verlet_kick", "lj_force_nbr_fused_step", "rebuild"):
        assert md.kernel_time(name)[1] == twin.kernel_time(name)[1], name
    # with a table: timed as one entry, behind every force pass and at every rebuild
    md.set_alchemical_(B["flag"], lam=0.5, alpha=ALPHA)
    md.profile_(True)
    md.step_(7, DT, rebuild_every=100)
    ms, launches = md.kernel_time("alchemical")
    assert launches == md.kernel_time("lj_force_nbr")[1] == 7 and ms > 0.0 and md.kernel_time(20) == (ms, launches)
    md.close()
    twin.close()


@pytest.mark.parametrize("samples", [4, 7])
def test_log_entries_are_the_reads_of_a_twin(emdee, dev, samples):
    """capacity 5: fewer samples than it, and more"""
    E = emdee
    B = _small(E)
    every, cap = 3, 5
    md = _engine(E, dev, B, lam=0.45, foreign=FOREIGN, log_every=every, log_capacity=cap)
    twin = _engine(E, dev, B, lam=0.45, foreign=FOREIGN)
    md.step_(every * samples + 2, DT)                                 # (two steps past the last sample: they add none)
    rows = []
    for _ in range(samples):
        twin.step_(every, DT)
        r = twin.alchemical()
        rows.append([r["dUdl"], r["U"]] + list(r["foreign"]))
    log = md.alchemical_log()
    kept = min(samples, cap)
    assert (log["count"], log["dropped"]) == (kept, samples - kept)
    got = np.concatenate([log["dUdl"][:, None], log["U"][:, None], log["foreign"]], axis=1)
    assert got.shape == (kept, 2 + len(FOREIGN)) and np.array_equal(got, np.array(rows)[:kept])
    assert twin.alchemical_log()["count"] == 0
    md.close()
    twin.close()


# ---------------------------------------------------------------- 5. composition
def test_an_excluded_cross_pair_stays_excluded(emdee, dev):
    E = emdee
    B = _fluid(E)
    x = B["pos"]
    s = int(B["cluster"][0])
    d = x - x[s]
    d -= B["L"] * np.rint(d / B["L"])
    order = np.argsort((d * d).sum(axis=1))
    env = [int(i) for i in order if B["flag"][i] == 0][:2]
    sol = [int(i) for i in order[1:] if B["flag"][i] == 1][:1]
    excl = np.array([[s, env[0]], [env[1], s], [s, sol[0]], [env[0], env[1]]])     # two cross pairs, a solute pair, an environment pair
    md = _engine(E, dev, B)
    md.set_exclusions_(excl)
    md.set_alchemical_(B["flag"], lam=0.6, alpha=ALPHA)
    _, ref = _check_planes(md, B, 0.6, np.float64, "exclusions", excl=excl)
    whole = _reference(B, x, 0.6)
    assert whole["pairs"] == ref["pairs"] + 2                           # (the two excluded cross pairs are inside rc and are not counted)
    md.step_(10, DT)
    _check_planes(md, B, 0.6, np.float64, "exclusions after 10 steps", excl=excl)
    md.close()


@pytest.mark.parametrize("method", ["reaction field", "pme"])
def test_a_charged_engine_whose_solute_carries_no_charge(emdee, dev, method):
    E = emdee
    B = _fluid(E)
    N = len(B["flag"])
    rng = np.random.default_rng(107)
    q = rng.choice([-0.4, 0.4], N)
    q[B["flag"] == 1] = 0.0
    q -= q.sum() / (B["flag"] == 0).sum() * (B["flag"] == 0)          # neutral, the solute still at zero
    assert abs(q.sum()) < 1e-12 and (q[B["flag"] == 1] == 0.0).all()
    md = _engine(E, dev, B)
    md.set_coulomb_(q, 1.0)
    L3 = np.array([B["L"]] * 3)
    if method == "pme":
        alpha, grid, order = 1.2, (32, 32, 32), 4
        md.set_pme_(alpha, grid, order)
        extra = lambda x: pm.pme(x, L3, q, 1.0, alpha, grid, order, RC)
    else:
        extra = lambda x: cr.coulomb(x, L3, q, 1.0, RC, np.inf)
    md.set_alchemical_(B["flag"], lam=0.6, alpha=ALPHA)
    _check_planes(md, B, 0.6, np.float64, method, extra=extra)
    md.step_(5, DT)
    _check_planes(md, B, 0.6, np.float64, method + " after 5 steps", extra=extra)
    # a charge on a flagged atom: the readiness check refuses the step, naming the first such atom
    bad = q.copy()
    first = int(np.where(B["flag"] == 1)[0][2])
    bad[first] = 0.25
    bad[np.where(B["flag"] == 1)[0][5]] = -0.25
    md.set_coulomb_(bad, 1.0)
    if method == "pme":
        md.set_pme_(1.2, (32, 32, 32), 4)
    for call, args in ((md.step_, (1, DT)), (md.minimize_, (3, 1.0))):
        text = _refused(E, ERR_STATE, call, *args)
        assert "atom %d " % first in text and "emdee_md_set_alchemical" in text and "emdee_md_set_coulomb" in text, text
    md.set_coulomb_(q, 1.0)
    md.step_(1, DT)
    md.close()


def test_rigid_water_with_a_flagged_site_under_c_rescale_with_molecular_scaling(emdee, dev):
    E = emdee
    B = sr.water_box()
    N = B["pos"].shape[0]
    flag = np.zeros(N, dtype=np.int32)
    flag[int(B["mol"][3][0])] = 1                                      # one site of one rigid molecule (its own partners are excluded)
    md = _water_engine(E, dev, B)
    md.set_molecular_scaling_()
    md.set_alchemical_(flag, lam=0.0, alpha=ALPHA)
    off = np.array(md.tensor_sums())
    md.set_lambda_(0.5)
    on = np.array(md.tensor_sums())
    read = md.alchemical()
    moved = (on[:3] - off[:3]).sum()
    print("trace of W moves by %.9g, the cross virial is %.9g (%d cross pairs)" % (moved, read["virial"], read["pairs"]))
    assert read["pairs"] > 10 and abs(moved - read["virial"]) <= 1e-9 * np.abs(on[:3]).sum()
    assert np.array_equal(on[6:], off[6:])
    assert np.isfinite(np.array(md.molecular_tensor_sums())).all()
    md.set_barostat_("c-rescale", p_ref=1.0, compressibility=0.05, tau_p=0.5, every=5, temperature=1.0, seed=7)
    box0 = np.array(md.box()[1])
    md.step_(20, sr.DT)                                              # four events
    box1 = np.array(md.box()[1])
    assert not np.array_equal(box0, box1)
    _constraints_hold_on(md, B, box1, "rigid water with a flagged site under C-rescale")
    x, v = _xv(md)
    assert np.isfinite(x).all() and np.isfinite(v).all() and np.isfinite(md.alchemical()["dUdl"])
    md.close()


# ---------------------------------------------------------------- 6. refusals
def test_every_refusal_leaves_the_previous_table_in_force(emdee, dev):
    E = emdee
    B = _small(E)
    N = B["pos"].shape[0]
    md = _engine(E, dev, B, lam=0.7, foreign=FOREIGN, log_every=2, log_capacity=4)
    bits, state = _read_bits(md), md.state()

    def flags(i, v):
        out = B["flag"].copy(); out[i] = v
        return out
    fdev = torch.as_tensor(B["flag"], dtype=torch.int32, device=dev)
    raw = lambda lam, alpha, f, nf, le=0, lc=0: E._lib.call(
        "emdee_md_set_alchemical", md._handle, C.c_void_p(fdev.data_ptr()), lam, alpha, None if f is None else f.ctypes.data_as(C.c_void_p), nf, le, lc)
    two = np.array([0.2, 0.4])
    cases = [
        ("a flag of 2", lambda: md.set_alchemical_(flags(5, 2), lam=0.5), "atom 5"),
        ("a flag of -1", lambda: md.set_alchemical_(flags(7, -1), lam=0.5), "atom 7"),
        ("no flagged atom", lambda: md.set_alchemical_(np.zeros(N, dtype=np.int32), lam=0.5), "no atom is flagged"),
        ("lambda above", lambda: md.set_alchemical_(B["flag"], lam=1.01), "lambda = 1.01"),
        ("lambda below", lambda: md.set_alchemical_(B["flag"], lam=-0.2), "lambda = -0.2"),
        ("lambda nan", lambda: md.set_alchemical_(B["flag"], lam=np.nan), "lambda = nan"),
        ("a foreign lambda outside", lambda: md.set_alchemical_(B["flag"], lam=0.5, foreign=[0.5, 1.5]), "foreign lambda 1 = 1.5"),
        ("alpha < 0", lambda: md.set_alchemical_(B["flag"], lam=0.5, alpha=-0.1), "alpha = -0.1"),
        ("alpha nan", lambda: md.set_alchemical_(B["flag"], lam=0.5, alpha=np.nan), "alpha = nan"),
        ("17 foreign values", lambda: md.set_alchemical_(B["flag"], lam=0.5, foreign=[0.5] * 17), "n_foreign = 17"),
        ("NULL foreign", lambda: raw(0.5, 0.5, None, 2), "NULL"),
        ("a log without log_every", lambda: raw(0.5, 0.5, two, 2, 0, 4), "log_every = 0"),
        ("negative capacity", lambda: raw(0.5, 0.5, two, 2, 1, -1), "log_capacity = -1"),
    ]
    for name, call, word in cases:
        text = _refused(E, ERR_INVALID, call)
        assert "set_alchemical" in text and word in text, (name, text)
        assert _read_bits(md) == bits, name
        assert all(torch.equal(a, b) for a, b in zip(md.state().values(), state.values()) if a is not None), name
    for lam in (-0.5, 1.5, np.nan):
        text = _refused(E, ERR_INVALID, md.set_lambda_, lam)
        assert "set_lambda" in text and _read_bits(md) == bits
    md.step_(4, DT)                                                   # the table in force still steps and logs
    assert md.alchemical_log()["count"] == 2 and md.alchemical()["lam"] == 0.7
    # the Green-Kubo heat flux: refused at set and at sample, naming the setter; the stress is not
    text = _refused(E, ERR_STATE, md.set_green_kubo_, 8, True, True)
    assert "emdee_md_set_alchemical" in text and "EMDEE_GK_HEAT" in text
    md.set_green_kubo_(8, stress=True, heat=False)
    md.gk_sample_()
    md.close()
    md = _engine(E, dev, B)
    md.set_green_kubo_(8, stress=True, heat=True)
    md.gk_sample_()
    md.set_alchemical_(B["flag"], lam=0.5)
    text = _refused(E, ERR_STATE, md.gk_sample_)
    assert "emdee_md_set_alchemical" in text and "EMDEE_GK_HEAT" in text
    md.close()


def test_calls_before_a_state_with_ghosts_and_on_a_lent_engine(emdee, dev):
    E = emdee
    B = _small(E)
    fdev = torch.as_tensor(B["flag"], dtype=torch.int32, device=dev)
    md = _engine(E, dev, B)
    h = C.c_void_p()
    three = lambda v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", md._ctx.handle, three([0.0] * 3), three([B["L"]] * 3), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(E.LennardJonesModel(RC, RS)), SKIN, E._lib.F64, C.byref(h))
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_set_alchemical", h, C.c_void_p(fdev.data_ptr()), 0.5, 0.5, None, 0, 0, 0)
    assert err.value.code == ERR_STATE and "emdee_md_set_state" in str(err.value) and "set_alchemical" in str(err.value)
    out = np.zeros(32)
    for name, args in (("emdee_md_alchemical_read", (out.ctypes.data_as(C.c_void_p),)), ("emdee_md_set_lambda", (0.5,)),
                       ("emdee_md_alchemical_log_read", (None, None, None))):
        with pytest.raises(E.EmDeeError) as err:                      # without a table
            E._lib.call(name, h, *args)
        assert err.value.code == ERR_STATE and "emdee_md_set_alchemical" in str(err.value), name
    E._lib.call("emdee_md_destroy", h)
    _refused(E, ERR_STATE, md.set_lambda_, 0.5)
    with pytest.raises(RuntimeError):
        md.alchemical()
    md.close()
    # ghosts: the last 64 atoms of the box loaded as ghosts
    N = B["pos"].shape[0]
    ghosts = E.VelocityVerlet(E.cu(B["pos"], dev), E.cu(B["vel"][:N - 64], dev), B["L"], E.LennardJonesModel(RC, RS), E.cu(B["atoms"], dev),
                              n_ghost=64)
    text = _refused(E, ERR_STATE, ghosts.set_alchemical_, B["flag"][:N - 64], lam=0.5)
    assert "ghosts" in text and "set_alchemical" in text
    ghosts.close()
    # an engine lent by a decomposition
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)
    pos = pos[np.argsort(gid)]
    n = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((n, 3)), E.lennard_jones_atoms(1.0, 1.0, n), float(lengths[0]))
    eng = dd.engine(0)
    text = _refused(E, ERR_STATE, eng.set_alchemical_, np.arange(eng.n_owned) % 2, lam=0.5)
    assert "emdee_dd_engine" in text and "set_alchemical" in text
    dd.step_(2, DT)
    dd.close()


def test_set_state_keeps_the_table_for_the_same_count_and_refuses_for_another(emdee, dev):
    E = emdee
    B = _small(E)
    N = B["pos"].shape[0]
    md = _engine(E, dev, B, lam=0.6)
    load = lambda n, pos: md.set_state_(E.cu(pos[:n], dev), E.cu(B["vel"][:n], dev), E.cu(B["atoms"][:n], dev),
                                        inv_mass=E.cu(1.0 / B["mass"][:n], dev))
    md.step_(2, DT)
    load(N, B["pos"] + 0.01)                                          # the same count: kept
    read = md.alchemical()
    ref = ar.system(B["pos"] + 0.01, [B["L"]] * 3, RC, RS, B["atoms"]["half_sigma"], B["atoms"]["twice_sqrt_eps"], B["flag"], 0.6, ALPHA)
    assert read["pairs"] == ref["pairs"] and abs(read["dUdl"] - ref["dUdl"]) <= 1e-9 * ref["sizes"][1]
    md.step_(2, DT)
    load(N - 64, B["pos"])                                            # another count: refused until set again or cleared
    for call, args in ((md.step_, (1, DT)), (md.minimize_, (5, 1.0)), (md.alchemical, ()), (md.scale_box_, (1.01,)), (md.totals, ())):
        text = _refused(E, ERR_STATE, call, *args)
        assert "emdee_md_set_alchemical" in text, text
    _refused(E, ERR_STATE, md.state)                                  # (forces that were never evaluated)
    md.set_alchemical_(None)
    md.step_(2, DT)
    md.close()


# ---------------------------------------------------------------- 7. the example
def test_the_example_runs_at_its_small_size(tmp_path):
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lj_solvation.py"), "--cells", "5", "--melt", "100", "--windows", "3",
                        "--equil", "20", "--steps", "100", "--every", "10"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-1600:]
    rows = [line.split() for line in r.stdout.splitlines() if not line.startswith("#")]
    assert len(rows) == 3 + 1 + 2 and all(int(row[3]) == 10 for row in rows[:3]), r.stdout[-800:]
    assert all(np.isfinite(float(t)) for row in rows for t in row)
    assert float(rows[2][2]) == 0.0                                   # (the last window is lambda = 0: U_alch is exactly 0)
