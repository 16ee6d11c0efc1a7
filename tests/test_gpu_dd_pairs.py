"""GPU tests of exclusions and scaled 1-4 pairs in decomposed runs (emdee_dd_set_exclusions / emdee_dd_set_pairs14): tables
over GLOBAL ids, rows filtered by the tags that travel with the atoms, 1-4 partners found by the row filter -- owned atoms or
ghost images -- and the split step of a domain with a 1-4 table.  The oracle has no exclusions: the yardsticks are its full sum
minus the named pairs' terms minus (1 - lj14scale) times the 1-4 terms, and the undivided integrator with the same tables
(which tests/test_gpu_parity2.py validates against that sum)."""
import os

import numpy as np
import pytest

from .conftest import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RC, RS, SKIN, DT = 2.5, 2.0, 0.3, 0.005
NCELL = 8
LANGEVIN = (2.0, 0.7, 0x5EED)
ERR_INVALID, ERR_STATE = -1, -6


def _global_box(syn, uniform=False, ncell=NCELL):
    """The fcc box of tests/test_gpu_dd.py, atoms in global-id order."""
    pos, gid, lengths = syn.fcc_block((ncell,) * 3, (0, 0, 0), (ncell,) * 3)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    vel = syn.raw_normals(np.arange(N), N)
    vel -= vel.mean(axis=0)
    vel *= np.sqrt((3 * N - 3) / np.sum(vel * vel))
    eps, sigma = syn.mixture_parameters(syn.mixture_types(N))
    if uniform:
        eps, sigma = np.ones(N), np.ones(N)
    return pos, vel, eps, sigma, float(lengths[0])


def _molecules(N):
    """'Molecules' of the four atoms of each fcc unit cell (global id = 4 cell + b): 1-2 and 1-3 pairs excluded, 1-4 scaled."""
    mol = np.arange(N).reshape(-1, 4)
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]], mol[:, [0, 2]], mol[:, [1, 3]]])
    return excl, mol[:, [0, 3]]


def _lj14scale(E):
    s14 = E.ingest.NonbondedTable(os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml")).lj14scale
    assert 0.0 < s14 < 1.0
    return s14


def _pair_terms(oracle, x, L, om, atoms, pairs):
    """(f, e, w) contributions of the named pairs alone (as in tests/test_gpu_parity2.py): the oracle's pair function at the
    minimum-image distance, f = W / r^2 r_ij and half of E and W to either atom."""
    f, e, w = np.zeros_like(x), np.zeros(x.shape[0]), np.zeros(x.shape[0])
    for i, j in pairs:
        d = x[i] - x[j]
        d -= L * np.rint(d / L)
        r2 = float(d @ d)
        E, W = oracle.interaction(r2, om, atoms[i], atoms[j], mode=oracle.CUTOFF)
        f[i] += W / r2 * d; f[j] -= W / r2 * d
        e[i] += 0.5 * E; e[j] += 0.5 * E
        w[i] += 0.5 * W; w[j] += 0.5 * W
    return f, e, w


def _build(E, world, pos, vel, atoms, L, dtype=torch.float64, excl=None, p14=None, s14=1.0, load=True):
    dev = torch.device("cuda", 0)
    N = pos.shape[0]
    dd = E.DomainDecomposition([L] * 3, E.domain.rank_grid(world), E.LennardJonesModel(RC, RS), skin=SKIN, dtype=dtype, device=dev)
    ndt = np.float64 if dtype == torch.float64 else np.float32
    for r in range(world):
        mine = np.arange(r, N, world)               # scattered initial slices: the load hands each atom to its brick
        dd.set_atoms_(r, E.cu(pos[mine].astype(ndt), dev), E.cu(vel[mine].astype(ndt), dev), E.cu(atoms[mine], dev),
                      torch.from_numpy(mine.astype(np.int64)).to(dev))
    if excl is not None:
        dd.set_exclusions_(excl)
    if p14 is not None:
        dd.set_pairs14_(p14, s14)
    if load:
        dd.load_()
    return dd


def _undivided(E, pos, vel, atoms, L, dtype=torch.float64, excl=None, p14=None, s14=1.0):
    dev = torch.device("cuda", 0)
    ndt = np.float64 if dtype == torch.float64 else np.float32
    md = E.VelocityVerlet(E.cu(pos.astype(ndt), dev), E.cu(vel.astype(ndt), dev), L, E.LennardJonesModel(RC, RS), E.cu(atoms, dev),
                          skin=SKIN)
    if excl is not None:
        md.set_exclusions_(excl)
    if p14 is not None:
        md.set_pairs14_(p14, s14)
    return md


def _gather(dd, world, N):
    gids, x, v, f = np.zeros(N, dtype=int), np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3))
    owner = np.full(N, -1)
    for r in range(world):
        gid, xr, vr, fr = (t.cpu().numpy() for t in dd.state(r))
        assert (owner[gid] == -1).all()
        owner[gid] = r
        x[gid], v[gid], f[gid] = xr, vr, fr
    assert (owner >= 0).all(), "every atom is owned by exactly one domain"
    return x, v, f, owner


def _compare(dd, md, world, N, L, tol_x=1e-9, tol_v=1e-8, tol_e=1e-9):
    x, v, _, _ = _gather(dd, world, N)
    st = md.state()
    xr, vr = st["positions"].cpu().numpy().astype(np.float64), st["velocities"].cpu().numpy().astype(np.float64)
    dx = x - xr
    assert np.abs(dx - L * np.rint(dx / L)).max() < tol_x
    assert np.abs(v - vr).max() < tol_v
    got, want = dd.totals(), md.totals()
    for a, b in zip(got, want):
        assert a == pytest.approx(b, rel=tol_e, abs=tol_e * abs(want[0]))


@pytest.mark.parametrize("world,rebuild_every", [(1, 0), (2, 0), (4, 0), (8, 0), (2, 6), (8, 5)])
def test_molecular_box_in_domains_matches_the_oracle_and_the_undivided_run(emdee, oracle, world, rebuild_every):
    E = emdee
    pos, vel, eps, sigma, L = _global_box(E.synthetic)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    excl, p14 = _molecules(N)
    s14 = _lj14scale(E)
    dd = _build(E, world, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14)

    # at the load: forces and energies against the oracle's full sum minus the named pairs' terms
    om = oracle.model(RC, RS)
    f0, e0, w0 = oracle.nonbonded_cells(np.mod(pos, L), L, om, atoms)
    fx, ex, wx = _pair_terms(oracle, pos, L, om, atoms, excl)
    f4, e4, w4 = _pair_terms(oracle, pos, L, om, atoms, p14)
    want_f, want_e, want_w = f0 - fx - (1.0 - s14) * f4, e0 - ex - (1.0 - s14) * e4, w0 - wx - (1.0 - s14) * w4
    assert np.abs(f4).max() > 1e-3 * np.abs(f0).max()              # the 1-4 pairs are inside the cutoff: they matter
    x, _, f, owner = _gather(dd, world, N)
    assert np.abs(f - want_f).max() <= 1e-6 * np.abs(want_f).max()
    ep, _, vir = dd.totals()
    assert ep == pytest.approx(want_e.sum(), rel=1e-6) and vir == pytest.approx(want_w.sum(), rel=1e-6)
    if world > 1:
        # named pairs across a cut: one atom owned here, its partner within the cutoff and owned by another domain (a ghost here)
        named = np.concatenate([excl, p14])
        d = pos[named[:, 0]] - pos[named[:, 1]]
        d -= L * np.rint(d / L)
        across = (owner[named[:, 0]] != owner[named[:, 1]]) & (np.einsum("ij,ij->i", d, d) < RC * RC)
        assert across.sum() > 0
        assert (owner[p14[:, 0]] != owner[p14[:, 1]]).any()

    md = _undivided(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14)
    nsteps = 60
    dd.step_(29, DT, rebuild_every)                  # two calls: the closing half kick and the re-opening must chain
    dd.step_(nsteps - 29, DT, rebuild_every)
    md.step_(nsteps, DT)
    _compare(dd, md, world, N, L)
    st = dd.stats()
    assert st["rebuilds"] >= 3                       # the load and at least two in the run
    if world > 1:
        assert st["migrated"] > 0
    dd.close()


def test_exclusions_only_keep_the_fused_step(emdee):
    E = emdee
    world = 8
    pos, vel, eps, sigma, L = _global_box(E.synthetic)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    excl, _ = _molecules(N)
    dd = _build(E, world, pos, vel, atoms, L, excl=excl)
    eng = [dd.engine(r) for r in range(world)]
    for e in eng:
        e.profile_(True)
    md = _undivided(E, pos, vel, atoms, L, excl=excl)
    dd.step_(60, DT)
    md.step_(60, DT)
    _compare(dd, md, world, N, L)
    assert dd.stats()["rebuilds"] >= 3
    fused = sum(e.kernel_time("fused_step_interior")[1] + e.kernel_time("fused_step_boundary")[1] for e in eng)
    assert fused >= 50 * world // 2, fused
    assert sum(e.kernel_time("verlet_kick_drift")[1] for e in eng) <= 2 * world * dd.stats()["rebuilds"]
    dd.close()


@pytest.mark.parametrize("variant", ["f32", "direct", "uniform", "langevin"])
def test_decomposed_pairs_variants(emdee, monkeypatch, variant):
    E = emdee
    if variant == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    world = 8 if variant != "direct" else 4
    dtype = torch.float32 if variant == "f32" else torch.float64
    pos, vel, eps, sigma, L = _global_box(E.synthetic, uniform=variant == "uniform")
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    excl, p14 = _molecules(N)
    s14 = _lj14scale(E)
    dd = _build(E, world, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14)
    md = _undivided(E, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14)
    if variant == "langevin":
        dd.set_langevin_(*LANGEVIN)                  # noise keyed by global id = the undivided run's caller index
        md.set_langevin_(*LANGEVIN)
    dd.step_(60, DT)
    md.step_(60, DT)
    if dtype == torch.float32:
        _compare(dd, md, world, N, L, tol_x=2e-3, tol_v=2e-2, tol_e=2e-4)
    else:
        _compare(dd, md, world, N, L)
    assert dd.stats()["rebuilds"] >= 3
    dd.close()


def test_tables_set_between_steps(emdee):
    """A table set after the load rebuilds every domain: on return the forces follow it, and the run goes on as the undivided
    integrator given the same tables at the same point."""
    E = emdee
    world = 4
    pos, vel, eps, sigma, L = _global_box(E.synthetic)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    excl, p14 = _molecules(N)
    s14 = _lj14scale(E)
    dd = _build(E, world, pos, vel, atoms, L)
    md = _undivided(E, pos, vel, atoms, L)
    dd.step_(20, DT)
    md.step_(20, DT)
    dd.set_exclusions_(excl)
    dd.set_pairs14_(p14, s14)
    md.set_exclusions_(excl)
    md.set_pairs14_(p14, s14)
    _, _, f, _ = _gather(dd, world, N)
    fr = md.state()["forces"].cpu().numpy()
    assert np.abs(f - fr).max() <= 1e-9 * np.abs(fr).max()
    dd.step_(30, DT)
    md.step_(30, DT)
    _compare(dd, md, world, N, L)
    dd.close()


def test_cleared_tables_cost_nothing(emdee):
    """Tables set and cleared again before the load: the run is the one that never had tables, bit for bit."""
    E = emdee
    world = 8
    pos, vel, eps, sigma, L = _global_box(E.synthetic)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    excl, p14 = _molecules(N)
    a = _build(E, world, pos, vel, atoms, L, excl=excl, p14=p14, s14=0.5, load=False)
    a.set_exclusions_(None)
    a.set_pairs14_(None, 1.0)
    a.load_()
    b = _build(E, world, pos, vel, atoms, L)
    a.step_(30, DT)
    b.step_(30, DT)
    for ga, gb in zip(_gather(a, world, N), _gather(b, world, N)):
        assert np.array_equal(ga, gb)
    assert a.totals() == b.totals()
    a.close(); b.close()


def test_refusals(emdee):
    E = emdee
    world = 4
    pos, vel, eps, sigma, L = _global_box(E.synthetic)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    excl, p14 = _molecules(N)
    a = _build(E, world, pos, vel, atoms, L, excl=excl, p14=p14, s14=0.5)
    b = _build(E, world, pos, vel, atoms, L, excl=excl, p14=p14, s14=0.5)
    # invalid pairs: nothing changes -- the previous tables keep working
    for bad in ([[3, 3]], [[-1, 5]], [[0, 1 << 31]]):
        with pytest.raises(E.EmDeeError) as err:
            a.set_exclusions_(np.concatenate([excl[:7], np.array(bad)]))
        assert err.value.code == ERR_INVALID
        with pytest.raises(E.EmDeeError) as err:
            a.set_pairs14_(np.array(bad), 0.5)
        assert err.value.code == ERR_INVALID
    a.step_(30, DT)
    b.step_(30, DT)
    for ga, gb in zip(_gather(a, world, N), _gather(b, world, N)):
        assert np.array_equal(ga, gb)
    # a domain's integrator has no tables of its own: its pairs are the decomposition's, keyed by global id
    eng = a.engine(0)
    with pytest.raises(E.EmDeeError) as err:
        eng.set_exclusions_(excl[:4])
    assert err.value.code == ERR_STATE and "emdee_dd_set" in str(err.value)
    with pytest.raises(E.EmDeeError) as err:
        eng.set_pairs14_(p14[:4], 0.5)
    assert err.value.code == ERR_STATE
    # a pair naming a gid no domain holds is legal and contributes nothing
    a.set_exclusions_(np.concatenate([excl, np.array([[N + 5, N + 9], [2, N + 100]])]))
    b.set_exclusions_(excl)
    a.step_(10, DT)
    b.step_(10, DT)
    for ga, gb in zip(_gather(a, world, N), _gather(b, world, N)):
        assert np.array_equal(ga, gb)
    a.close(); b.close()
