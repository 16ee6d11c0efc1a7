"""GPU tests of the per-atom virial tensor and the pressure tensor (emdee_compute_virial_tensor, emdee_md_virial_tensor,
emdee_md_pressure_tensor, emdee_dd_pressure_tensor) against the host yardstick of tests/helpers/virial_tensor_ref.py, on
every kernel family the planner selects: the single-species plane kernel, the general-species kernel, the two-species typed
kernel, the direct path, a non-cubic box with a non-periodic axis, molecular tables, decomposed runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import GOLDEN, ROOT, read_xyz
from .helpers import virial_tensor_ref as vt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
TOL = {np.float64: 1e-10, np.float32: 1e-4}
DT = 0.005


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _fields(atoms):
    a = np.asarray(atoms)
    return a["half_sigma"].astype(np.float32), a["twice_sqrt_eps"].astype(np.float32)


def _close(got, want, dtype, what):
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    assert err <= TOL[dtype] * scale, "%s: max |dW| = %.3e of max |W| = %.3e" % (what, err, scale)


def _jittered_fcc(E, cells, seed=7, amp=0.25):
    pos, L = E.synthetic.fcc_positions(cells)
    return pos + amp * (np.random.default_rng(seed).random(pos.shape) - 0.5), L


# ---------------------------------------------------------------- operator
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("box", ["lj_sample", "fcc864"])
def test_operator_tensor_matches_the_yardstick_and_traces_to_the_virials(emdee, oracle, dev, box, dtype):
    E = emdee
    if box == "lj_sample":
        x = read_xyz(os.path.join(GOLDEN, "lj_sample.xyz")).astype(np.float32)
        L, rc, rs = 10.0, 3.0, 2.5
    else:
        x, L = E.synthetic.fcc_positions(6)
        rc, rs = 2.5, 2.0
    x = x.astype(dtype)
    N = x.shape[0]
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    hs, te = _fields(atoms)
    want, _ = vt.per_atom_tensor(x.astype(np.float64), [L] * 3, [1, 1, 1], rc, rs, hs, te, oracle=oracle)
    tdt = _tdt(dtype)
    tiles = E.nonbonded_computation_tiles(N)
    model = E.LennardJonesModel(rc, rs)
    xd, ad = E.cu(x, dev), E.cu(atoms, dev)
    t = torch.full((N, 6), float("nan"), dtype=tdt, device=dev)
    E.compute_virial_tensor_(t, xd, L, tiles, model, ad)
    w = torch.zeros(N, dtype=tdt, device=dev)
    E.compute_nonbonded_(None, None, w, xd, L, tiles, model, ad, E.VIRIALS)
    t, w = t.cpu().numpy(), w.cpu().numpy()
    _close(t, want, dtype, box)
    tr = t[:, 0].astype(np.float64) + t[:, 1] + t[:, 2]
    assert np.abs(tr - w).max() <= (1e-13 if dtype == np.float64 else 1e-5) * np.abs(w).max()


# ---------------------------------------------------------------- the integrator, every kernel family
FAMILIES = ["uniform", "species3", "typed", "direct", "orthorhombic"]


def _family_box(E, family):
    """positions, lengths, periodic, atoms, model (rc, rs), environment, the debug-plan text expected / refused"""
    if family == "typed":
        pos, L = E.synthetic.fcc_positions(29)          # (cell side just above rc + skin: the tiles fit the typed planes, tests/test_gpu_parity2.py)
        eps, sigma = E.synthetic.mixture_parameters(E.synthetic.mixture_types(pos.shape[0]))
        return pos, [L] * 3, [1, 1, 1], E.lennard_jones_atoms(eps, sigma), (3.5, 3.0), {}, "typed kernels on", None
    pos, L = _jittered_fcc(E, 10)
    N = pos.shape[0]
    if family == "species3":
        k = np.arange(N) % 3
        atoms = E.lennard_jones_atoms(np.array([1.0, 0.8, 0.6])[k], np.array([1.0, 0.95, 0.9])[k])
        return pos, [L] * 3, [1, 1, 1], atoms, (2.5, 2.0), {}, "emdee plan: bricks", "two species"
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    if family == "uniform":
        return pos, [L] * 3, [1, 1, 1], atoms, (2.5, 2.0), {}, "emdee plan: bricks", "two species"
    if family == "direct":
        return pos, [L] * 3, [1, 1, 1], atoms, (2.5, 2.0), {"EMDEE_PATH": "direct"}, None, "emdee plan: bricks"
    # orthorhombic, z not periodic: stretch y and z so that every component differs, and so do the three cell counts
    # (sides 17.1, 20.5, 24.8 at rc + skin = 2.8: 6, 7 and 8 cells); keep z inside the walls
    lengths = [L, 1.2 * L, 1.45 * L]
    pos = pos * np.array([1.0, 1.2, 1.45]) + np.array([0.0, 0.0, 0.0])
    pos[:, 2] = np.clip(pos[:, 2], 0.05, lengths[2] - 0.05)
    return pos, lengths, [1, 1, 0], atoms, (2.5, 2.0), {}, "emdee plan: bricks", None


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", FAMILIES)
def test_integrator_tensor_on_every_kernel_family(emdee, oracle, dev, capfd, monkeypatch, family, dtype):
    E = emdee
    pos, lengths, periodic, atoms, (rc, rs), env, want_line, no_line = _family_box(E, family)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    N = pos.shape[0]
    x = pos.astype(dtype)
    vel = E.synthetic.velocities(N).astype(dtype)
    capfd.readouterr()
    md = E.VelocityVerlet(E.cu(x, dev), E.cu(vel, dev), lengths[0], E.LennardJonesModel(rc, rs), E.cu(atoms, dev),
                          lo=[0.0, 0.0, 0.0], lengths=lengths, periodic=periodic)
    t = md.virial_tensor().cpu().numpy()
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    if want_line is not None:
        assert want_line in err, err[-600:]
    if no_line is not None:
        assert no_line not in err, err[-600:]
    hs, te = _fields(atoms)
    want, _ = vt.per_atom_tensor(x.astype(np.float64), lengths, periodic, rc, rs, hs, te,
                                 oracle=oracle if periodic == [1, 1, 1] else None)
    _close(t, want, dtype, family)
    if family == "orthorhombic":
        # the three diagonal components differ box-wide: swapped components would show
        diag = want[:, :3].sum(axis=0)
        assert np.abs(t[:, :3].sum(axis=0) - diag).max() <= 1e-3 * np.abs(diag).min()
    md.close()


# ---------------------------------------------------------------- molecular tables
def _molecules(N):
    mol = np.arange(N).reshape(-1, 4)
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]], mol[:, [0, 2]], mol[:, [1, 3]]])
    return excl, mol[:, [0, 3]]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_integrator_tensor_with_exclusions_and_14_pairs(emdee, oracle, dev, dtype):
    E = emdee
    pos, L = E.synthetic.fcc_positions(8)
    N = pos.shape[0]
    eps, sigma = E.synthetic.mixture_parameters(E.synthetic.mixture_types(N))
    atoms = E.lennard_jones_atoms(eps, sigma)
    excl, p14 = _molecules(N)
    s14 = 0.5
    x = pos.astype(dtype)
    md = E.VelocityVerlet(E.cu(x, dev), E.cu(E.synthetic.velocities(N).astype(dtype), dev), L, E.LennardJonesModel(2.5, 2.0), E.cu(atoms, dev))
    md.set_exclusions_(excl)
    md.set_pairs14_(p14, s14)
    t = md.virial_tensor().cpu().numpy()
    hs, te = _fields(atoms)
    want, _ = vt.per_atom_tensor(x.astype(np.float64), [L] * 3, [1, 1, 1], 2.5, 2.0, hs, te, excl=excl, p14=p14, lj14scale=s14, oracle=oracle)
    _close(t, want, dtype, "molecular")
    # the operator with the same tables
    tiles = E.nonbonded_computation_tiles(N)
    tiles.set_exclusions_(excl)
    tiles.set_pairs14_(p14, s14)
    to = torch.zeros((N, 6), dtype=_tdt(dtype), device=dev)
    E.compute_virial_tensor_(to, E.cu(x, dev), L, tiles, E.LennardJonesModel(2.5, 2.0), E.cu(atoms, dev))
    _close(to.cpu().numpy(), want, dtype, "molecular operator")


# ---------------------------------------------------------------- box totals
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pressure_tensor_totals_match_the_scalar_observables(emdee, dev, dtype):
    E = emdee
    pos, L = _jittered_fcc(E, 8)
    N = pos.shape[0]
    eps, sigma = E.synthetic.mixture_parameters(E.synthetic.mixture_types(N))
    inv_mass = (1.0 / (1.0 + 0.5 * E.synthetic.mixture_types(N))).astype(dtype)
    md = E.VelocityVerlet(E.cu(pos.astype(dtype), dev), E.cu(E.synthetic.velocities(N).astype(dtype), dev), L,
                          E.LennardJonesModel(2.5, 2.0), E.cu(E.lennard_jones_atoms(eps, sigma), dev), inv_mass=E.cu(inv_mass, dev))
    md.step_(20, DT)
    per_atom = md.virial_tensor().cpu().numpy().astype(np.float64)
    s = md.tensor_sums()
    ep, ek, vir = md.totals()
    rel = 1e-12 if dtype == np.float64 else 1e-5
    W, K = np.array(s[:6]), np.array(s[6:])
    assert np.abs(W - per_atom.sum(axis=0)).max() <= rel * np.abs(W).max() * (1 if dtype == np.float64 else 10)
    assert W[:3].sum() == pytest.approx(vir, rel=1e-12 if dtype == np.float64 else 1e-5)
    assert K[:3].sum() == pytest.approx(2.0 * ek, rel=1e-12)
    v = md.state()["velocities"].cpu().numpy().astype(np.float64)
    m = 1.0 / inv_mass.astype(np.float64)
    Kh = np.array([np.sum(m * v[:, a] * v[:, b]) for a, b in vt.COMPONENTS])
    assert np.abs(K - Kh).max() <= 1e-12 * np.abs(Kh).max()
    P = md.pressure_tensor()
    obs = md.observables()
    assert np.trace(P["pressure"]) / 3.0 == pytest.approx(obs["pressure"], rel=1e-12 if dtype == np.float64 else 1e-6)
    assert np.array_equal(P["virial"], vt.matrix(W)) and np.array_equal(P["kinetic"], vt.matrix(K))


# ---------------------------------------------------------------- no side effects, reproducible
def test_tensor_queries_leave_the_trajectory_bit_for_bit(emdee, dev):
    E = emdee
    pos, L = _jittered_fcc(E, 8)
    N = pos.shape[0]
    vel = E.synthetic.velocities(N)
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)

    def run(query):
        md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(2.5, 2.0), E.cu(atoms, dev))
        seen = []
        for _ in range(10):
            md.step_(10, DT)
            if query:
                seen.append((md.virial_tensor().cpu().numpy(), md.tensor_sums(), md.virial_tensor().cpu().numpy()))
        st = md.state()
        out = {k: st[k].cpu().numpy() for k in ("positions", "velocities", "forces")}
        md.close()
        return out, seen

    plain, _ = run(False)
    a, ta = run(True)
    b, tb = run(True)
    for k in plain:
        assert np.array_equal(plain[k], a[k]), k
        assert np.array_equal(a[k], b[k]), k
    for (t1, s1, t1again), (t2, s2, _) in zip(ta, tb):
        assert np.array_equal(t1, t2) and s1 == s2
        assert np.array_equal(t1, t1again)                # a second query between steps reads the same tensors


# ---------------------------------------------------------------- decomposed runs
def _dd_box(E, cells=8):
    pos, gid, lengths = E.synthetic.fcc_block((cells,) * 3, (0, 0, 0), (cells,) * 3)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    vel = E.synthetic.raw_normals(np.arange(N), N)
    vel -= vel.mean(axis=0)
    eps, sigma = E.synthetic.mixture_parameters(E.synthetic.mixture_types(N))
    return pos, vel, E.lennard_jones_atoms(eps, sigma), float(lengths[0])


def _rel_max(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("world", [1, 2, 8])
def test_decomposed_pressure_tensor_matches_the_undivided_engine(emdee, dev, world, tables):
    E = emdee
    pos, vel, atoms, L = _dd_box(E)
    N = pos.shape[0]
    excl, p14 = _molecules(N) if tables else (None, None)
    model = E.LennardJonesModel(2.5, 2.0)
    dd = E.DomainDecomposition([L] * 3, E.domain.rank_grid(world), model, skin=0.3, dtype=torch.float64, device=dev)
    for r in range(world):
        mine = np.arange(r, N, world)
        dd.set_atoms_(r, E.cu(pos[mine], dev), E.cu(vel[mine], dev), E.cu(atoms[mine], dev), torch.from_numpy(mine.astype(np.int64)).to(dev))
    if tables:
        dd.set_exclusions_(excl)
        dd.set_pairs14_(p14, 0.5)
    dd.load_()
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, model, E.cu(atoms, dev))
    if tables:
        md.set_exclusions_(excl)
        md.set_pairs14_(p14, 0.5)
    a, b = np.array(dd.tensor_sums()), np.array(md.tensor_sums())
    assert _rel_max(a[:6], b[:6]) <= 1e-12 and _rel_max(a[6:], b[6:]) <= 1e-12
    P = dd.pressure_tensor()
    assert np.trace(P["pressure"]) / 3.0 == pytest.approx(dd.observables()["pressure"], rel=1e-12)
    dd.step_(60, DT, 0)
    md.step_(60, DT, 0)
    a, b = np.array(dd.tensor_sums()), np.array(md.tensor_sums())
    assert _rel_max(a[:6], b[:6]) <= 1e-8 and _rel_max(a[6:], b[6:]) <= 1e-8
    assert np.array_equal(np.array(dd.tensor_sums()), a)     # a repeated query: the same sums
    dd.close()
    md.close()


def test_two_rccl_ranks_all_reduce_the_twelve_sums(emdee):
    """Two processes, one communicator rank each, on the one device (RCCL's TCP transport, as tests/test_gpu_dd.py runs its
    ranks): the all-reduced twelve sums of each rank equal the in-process two-domain run's."""
    script = os.path.join(ROOT, "tests", "helpers", "tensor_rank.py")
    env0 = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1", NCCL_NET_GDR_LEVEL="0")
    kids = []
    try:
        for r in range(2):
            env = dict(env0, NCCL_HOSTID="emdee-tensor-rank-%d" % r)
            k = subprocess.Popen([sys.executable, script, "--rank", str(r)], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True, start_new_session=True)
            kids.append(k)
            if r == 0:
                uid = k.stdout.readline().strip()
                assert uid.startswith("ID "), uid
            else:
                k.stdin.write(uid + "\n")
                k.stdin.flush()
        outs = [k.communicate(timeout=240) for k in kids]
    finally:
        for k in kids:
            if k.poll() is None:
                k.kill()
    ref = subprocess.run([sys.executable, script, "--in-process"], capture_output=True, text=True, timeout=240)
    assert ref.returncode == 0, ref.stderr[-800:]
    want = [float(v) for v in ref.stdout.split("SUMS")[1].split()]
    for k, (out, err) in zip(kids, outs):
        assert k.returncode == 0, err[-800:]
        got = [float(v) for v in out.split("SUMS")[1].split()]
        assert _rel_max(got[:12], want[:12]) <= 1e-12 and _rel_max(got[12:], want[12:]) <= 1e-9


# ---------------------------------------------------------------- refusals
def test_tensor_calls_refuse_missing_state_and_null_outputs(emdee, dev):
    import ctypes as C
    E = emdee
    lib = E._lib
    ctx = E.context_for(dev)
    h = C.c_void_p()
    lib.call("emdee_md_create", ctx.handle, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(8, 8, 8), (C.c_int32 * 3)(1, 1, 1),
             lib.model_c(E.LennardJonesModel(2.5, 2.0)), 0.3, 8, C.byref(h))
    buf = torch.zeros((4, 6), dtype=torch.float64, device=dev)
    out = (C.c_double * 12)()
    try:
        with pytest.raises(E.EmDeeError) as ei:
            lib.call("emdee_md_virial_tensor", h, C.c_void_p(buf.data_ptr()))
        assert ei.value.code == ERR_STATE
        with pytest.raises(E.EmDeeError) as ei:
            lib.call("emdee_md_pressure_tensor", h, out)
        assert ei.value.code == ERR_STATE
    finally:
        lib.call("emdee_md_destroy", h)
    pos, L = _jittered_fcc(E, 4)
    N = pos.shape[0]
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N), dev), L, E.LennardJonesModel(2.5, 2.0),
                          E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev))
    for name, args in (("emdee_md_virial_tensor", (None,)), ("emdee_md_pressure_tensor", (None,))):
        with pytest.raises(E.EmDeeError) as ei:
            lib.call(name, md._handle, *args)
        assert ei.value.code == ERR_INVALID
    for mask in (8, 14, 15):
        with pytest.raises(E.EmDeeError) as ei:
            md.forces_(mask)
        assert ei.value.code == ERR_INVALID
    tiles = E.nonbonded_computation_tiles(N)
    x, a = E.cu(pos, dev), E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev)
    with pytest.raises(E.EmDeeError) as ei:
        lib.call("emdee_compute_virial_tensor", ctx.handle, None, C.c_void_p(x.data_ptr()), L, tiles._get(ctx, 8),
                 lib.model_c(E.LennardJonesModel(2.5, 2.0)), C.c_void_p(a.data_ptr()), 8)
    assert ei.value.code == ERR_INVALID
    dd = E.DomainDecomposition([L] * 3, (1, 1, 1), E.LennardJonesModel(2.5, 2.0), dtype=torch.float64, device=dev)
    with pytest.raises(E.EmDeeError) as ei:
        dd.pressure_tensor()
    assert ei.value.code == ERR_STATE
    with pytest.raises(E.EmDeeError) as ei:
        lib.call("emdee_dd_pressure_tensor", dd._handle, None)
    assert ei.value.code == ERR_INVALID
    dd.close()
    md.close()
