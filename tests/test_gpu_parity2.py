"""GPU parity, second file (round 2): things the first suite pinned only indirectly.

  * the neighbour SET, read back through emdee_nbr_list / emdee_md_nbr_list and compared with the oracle's list
    entry for entry (index work is bit-exact, not just equal in count);
  * position/parameter ingest feeding the HIP path: XYZ fixture + the NonbondedForce table of
    the reference's own force-field fixture (src/modelling.jl:71-73,197-200) -> compute_nonbonded_ vs the oracle;
  * the fp32 configuration (BASELINE configs[3]) at the size it is quoted on: 10^7 atoms, conserved quantities.
"""
import ctypes
import os

import numpy as np
import pytest

from .conftest import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev(emdee):
    assert emdee.gpu_available(), "GPU tests need a MI355X"
    return torch.device("cuda", 0)


def _rows(counts, nb):
    counts, nb = counts.cpu().numpy(), nb.cpu().numpy()
    return [np.sort(nb[i, :counts[i]]) for i in range(counts.shape[0])]


def _oracle_rows(oracle, x, L, rlist):
    off, nb = oracle.neighbor_list(x, L, rlist)
    return [np.sort(nb[off[i]:off[i + 1]]) for i in range(x.shape[0])]


@pytest.mark.parametrize("case", ["lj_sample_800", "fcc_32k", "mixture_random"])
def test_neighbour_set_is_the_oracles_set(emdee, oracle, dev, lj_sample, case):
    """Every row of the device list holds exactly the oracle's neighbours (r < rc + skin, minimum image)."""
    E = emdee
    rng = np.random.default_rng(7)
    if case == "lj_sample_800":
        x, L, rc, rs = lj_sample.astype(np.float64), 10.0, 3.0, 2.5
        atoms = E.lennard_jones_atoms(1.0, 1.0, x.shape[0])
    elif case == "fcc_32k":
        x, L = E.synthetic.fcc_positions(20)
        rc, rs = 2.5, 2.0
        atoms = E.lennard_jones_atoms(1.0, 1.0, x.shape[0])
    else:
        N, L, rc, rs = 6000, 19.0, 3.5, 3.0                       # random gas + lattice remnants: ragged rows, two species
        x = rng.uniform(0.0, L, size=(N, 3))
        keep = np.ones(N, dtype=bool)
        eps, sigma = E.synthetic.mixture_parameters(E.synthetic.mixture_types(N))
        atoms = E.lennard_jones_atoms(eps, sigma)
        x = x[keep]
    N = x.shape[0]
    skin = 0.3
    tiles = E.nonbonded_computation_tiles(N)
    f = torch.zeros((N, 3), dtype=torch.float64, device=dev)
    E.compute_nonbonded_(f, None, None, E.cu(x, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(E.FORCES))
    got = _rows(*tiles.neighbor_lists())
    want = _oracle_rows(oracle, x, L, rc + skin)
    assert sum(len(r) for r in got) == sum(len(r) for r in want) == tiles.stats()["listed"]
    for i in range(N):
        assert np.array_equal(got[i], want[i]), "row %d differs" % i


@pytest.mark.parametrize("case", ["cell_equals_rlist", "wide_cells", "fp32_melt"])
def test_neighbour_set_with_x_sub_bins(emdee, oracle, dev, case, monkeypatch, capfd):
    """Untyped boxes are sorted by (cell, quarter of the cell along x) and the build skips the quarters of the left and right
    cells that lie beyond r_list (kernels.hpp XSubBin, brick.hpp): the set must not change -- when the cell is exactly r_list
    wide (K = -1: one quarter more on either side), when the cells are much wider than r_list (sparse box, K = 2), and in
    fp32, where the fp32 distance test IS the definition of the set (against the same build without sub-bins)."""
    E = emdee
    rng = np.random.default_rng(11)
    rc, rs, skin = 2.5, 2.0, 0.3
    dtype, want_k = np.float64, None
    if case == "cell_equals_rlist":
        L, N, want_k = 8 * 2.8, 9000, -1
        x = rng.uniform(0.0, L, size=(N, 3))
    elif case == "wide_cells":
        L, N, want_k = 40.0, 500, 2
        x = rng.uniform(0.0, L, size=(N, 3))
    else:
        x, L = E.synthetic.fcc_positions(16)
        x = x + rng.normal(0.0, 0.12, size=x.shape)
        dtype, want_k = np.float32, 0
    N = x.shape[0]
    x = x.astype(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    lists = {}
    for name, env in (("sub", {}), ("plain", {"EMDEE_NO_SUBBINS": "1"})):
        monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tiles = E.nonbonded_computation_tiles(N, skin=skin)
        f = torch.zeros((N, 3), dtype=tdt, device=dev)
        E.compute_nonbonded_(f, None, None, E.cu(x, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(E.FORCES))
        lists[name] = (_rows(*tiles.neighbor_lists()), f.cpu().numpy())
        err = capfd.readouterr().err
        for k in env:
            monkeypatch.delenv(k)
        plans = [l for l in err.splitlines() if l.startswith("emdee plan")]
        assert plans, "the tiled path must be in use"
        if name == "sub":
            assert ("x sub-bins 4 K %d" % want_k) in plans[-1], plans[-1]
        else:
            assert "x sub-bins 1 " in plans[-1], plans[-1]
    got, plain = lists["sub"][0], lists["plain"][0]
    assert sum(len(r) for r in got) > 0
    for i in range(N):
        assert np.array_equal(got[i], plain[i]), "row %d differs from the build without sub-bins" % i
    if dtype == np.float64:
        want = _oracle_rows(oracle, x.astype(np.float64), L, rc + skin)
        for i in range(N):
            assert np.array_equal(got[i], want[i]), "row %d differs from the oracle" % i
    # same set, other order inside a cell: the forces agree to rounding
    fa, fb = lists["sub"][1], lists["plain"][1]
    assert np.abs(fa - fb).max() <= (1e-10 if dtype == np.float64 else 2e-3) * max(1.0, np.abs(fb).max())



def test_neighbour_set_of_the_ballot_build(emdee, oracle, dev, monkeypatch, capfd):
    """A tile row too crowded for the two-phase builds -- more than 32 GB atoms in three consecutive cells, GB = 8 lanes per atom
    in the build -- takes the ballot build (k_brick_build ALG 1): a dilute gas with one dense column of cells along x.  Its rows
    are the oracle's, entry for entry, and its forces the oracle's."""
    E = emdee
    rng = np.random.default_rng(41)
    rc, rs, skin = 3.5, 3.0, 0.4
    L = 6.05 * (rc + skin)                                             # 6 cells of 3.93 per side
    cw = L / 6
    a = 0.72                                                           # column: a 5 x 5 lattice per layer, layers a apart
    g = np.arange(5) * a + 2 * cw + 0.25
    layers = np.arange(int(L / a)) * a
    col = np.array([(x, y, z) for x in layers for y in g for z in g]) + rng.normal(0.0, 0.04, size=(len(layers) * 25, 3))
    m = np.arange(11) * (L / 11)                                       # the gas: a jittered lattice 2.1 apart
    gas = np.array([(x, y, z) for x in m for y in m for z in m]) + rng.normal(0.0, 0.2, size=(11 ** 3, 3))
    lo, hi = 2 * cw - 0.6, 2 * cw + 0.25 + 4 * a + 0.6                  # keep the gas out of the column's reach
    gas = gas[~(np.all((gas[:, 1:] > lo) & (gas[:, 1:] < hi), axis=1))]
    x = np.concatenate([col, gas])
    N = x.shape[0]
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    tiles = E.nonbonded_computation_tiles(N, skin=skin)
    f = torch.zeros((N, 3), dtype=torch.float64, device=dev)
    E.compute_nonbonded_(f, None, None, E.cu(x, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(E.FORCES))
    got = _rows(*tiles.neighbor_lists())
    plans = [l for l in capfd.readouterr().err.splitlines() if l.startswith("emdee plan")]
    assert plans, "the tiled path must be in use"
    span = int(plans[-1].split("max 3-cell span ")[1].split(",")[0])
    assert span > 32 * 8, plans[-1]
    want = _oracle_rows(oracle, x, L, rc + skin)
    assert sum(len(r) for r in got) == sum(len(r) for r in want) == tiles.stats()["listed"]
    for i in range(N):
        assert np.array_equal(got[i], want[i]), "row %d differs from the oracle" % i
    f0, _, _ = oracle.nonbonded_cells(x, L, oracle.model(rc, rs), atoms)
    assert np.abs(f.cpu().numpy() - f0).max() <= 1e-9 * np.abs(f0).max()


def test_posted_read_backs_and_copies_give_the_same_run(emdee, dev, monkeypatch):
    """The small blocking read-backs (rebuild requests of a batch of queued steps, the build's overflow words) are posted by a
    kernel into pinned host memory while the host spins on a stamp; EMDEE_READBACK=copy takes hipMemcpyAsync +
    hipStreamSynchronize instead.  Same decisions, same states, same number of rebuilds."""
    E = emdee
    x0, L = E.synthetic.fcc_positions(8)
    N = x0.shape[0]
    v0 = E.synthetic.velocities(N) * 1.4
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    out = {}
    for name, env in (("posted", {}), ("copy", {"EMDEE_READBACK": "copy"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx_dev = torch.device("cuda", 0)
        md = E.VelocityVerlet(E.cu(x0, ctx_dev), E.cu(v0, ctx_dev), L, E.LennardJonesModel(2.5, 2.0), E.cu(atoms, ctx_dev), skin=0.3)
        md.step_(60, 0.005)
        st = md.state()
        out[name] = (st["positions"].cpu().numpy(), st["velocities"].cpu().numpy(), md.nbr_stats()["builds"])
        for k in env:
            monkeypatch.delenv(k)
    assert np.array_equal(out["posted"][0], out["copy"][0]) and np.array_equal(out["posted"][1], out["copy"][1])
    assert out["posted"][2] == out["copy"][2] >= 5


def test_neighbour_set_of_the_integrator_after_rebuilds(emdee, oracle, dev):
    """emdee_md_nbr_list after displacement-triggered rebuilds: the list is the oracle's list of the positions it was
    built from (read back at the same moment)."""
    E = emdee
    x0, L = E.synthetic.fcc_positions(10)
    N = x0.shape[0]
    v0 = E.synthetic.velocities(N) * 1.3
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    md = E.VelocityVerlet(E.cu(x0, dev), E.cu(v0, dev), L, E.LennardJonesModel(2.5, 2.0), E.cu(atoms, dev), skin=0.3)
    md.step_(30, 0.005)
    assert md.nbr_stats()["builds"] >= 3
    md.rebuild_()                                                  # list of the CURRENT positions
    x = md.state()["positions"].cpu().numpy()
    got = _rows(*md.neighbor_lists())
    want = _oracle_rows(oracle, x, L, 2.8)
    for i in range(N):
        assert np.array_equal(got[i], want[i]), "row %d differs" % i


def test_ingest_feeds_the_hip_path(emdee, oracle, dev):
    """read_xyz(lj_sample.xyz) + NonbondedTable(dibenzo-p-dioxin-in-water.xml).lj_atoms -> compute_nonbonded_ with five
    species (one of them with eps = 0) vs the oracle given the same LJAtom array (src/modelling.jl:71-73,197-200)."""
    E = emdee
    names, pos = E.ingest.read_xyz(os.path.join(GOLDEN, "lj_sample.xyz"))
    table = E.ingest.NonbondedTable(os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml"))
    kinds = sorted(table.types)
    types = [kinds[i % len(kinds)] for i in range(len(names))]
    atoms = table.lj_atoms(types, length_unit=0.35)              # nm -> box units with sigma(OW) ~ 0.9
    assert atoms.dtype == E.LJAtom and (atoms["twice_sqrt_eps"] == 0.0).any() and len(set(atoms["half_sigma"])) >= 4
    N, L = pos.shape[0], 10.0
    x = pos.astype(np.float32).astype(np.float64)
    f0, e0, w0 = oracle.nonbonded_cells(x, L, oracle.model(3.0, 2.5), atoms)
    f = torch.zeros((N, 3), dtype=torch.float64, device=dev)
    e = torch.zeros(N, dtype=torch.float64, device=dev)
    w = torch.zeros(N, dtype=torch.float64, device=dev)
    E.compute_nonbonded_(f, e, w, E.cu(x, dev), L, E.nonbonded_computation_tiles(N), E.LennardJonesModel(3.0, 2.5),
                         E.cu(atoms, dev), E.Val(7))
    for got, want in ((f, f0), (e, e0), (w, w0)):
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(f0).max() > 1.0                                  # a non-trivial configuration


def test_fp32_reference_bound_per_quantity(emdee, oracle, dev, lj_sample):
    """The reference's `< 1e-4` absolute (test/runtests.jl:39-41) is between two fp32 implementations of the SAME
    arithmetic on lj_sample.xyz: scaled positions s = x / L, r_ij = L (ds - round(ds)).  Against the fp32 oracle
    (operation order of src/nonbonded.jl:122-155) every Float32 entry point holds it on forces, energies and virials:
    the all-pairs kernels (tile operator, naive double loop) and the O(N) list path, whose Float32 operator calls stage
    their LDS tiles as scaled positions read from the caller's array and take the minimum image per pair
    (BrickArgs::refmath) -- round 2 resolved images by adding +-L to wrapped fp32 coordinates and missed the bound by 6x
    (profiles/r02/fp32_error_probe.txt; now profiles/r03/fp32_error_probe.txt: 6.9e-5 / 2.4e-6 / 3.8e-5)."""
    E = emdee
    N = 800
    x = lj_sample
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    model = E.LennardJonesModel(3.0, 2.5)
    xd, ad = E.cu(x, dev), E.cu(atoms, dev)
    for mode, om, em in (("literal", oracle.LITERAL, E.LITERAL), ("cutoff", oracle.CUTOFF, E.CUTOFF)):
        f0, e0, w0 = oracle.naive(x, 10.0, oracle.model(3.0, 2.5, np.float32), atoms, om)
        for which in ("tiles", "naive", "nbr"):
            if which == "nbr" and mode == "literal":
                continue
            f = torch.zeros((N, 3), dtype=torch.float32, device=dev)
            e = torch.zeros(N, dtype=torch.float32, device=dev)
            w = torch.zeros(N, dtype=torch.float32, device=dev)
            if which == "tiles":
                E.compute_nonbonded_(f, e, w, xd, 10.0, E.nonbonded_computation_tiles(N, all_pairs=True, mode=em), model, ad, 7)
            elif which == "naive":
                E.naively_compute_nonbonded_(f, e, w, xd, 10.0, model, ad, mode=em)
            else:
                E.compute_nonbonded_(f, e, w, xd, 10.0, E.nonbonded_computation_tiles(N), model, ad, 7)
            df = np.abs(f.cpu().numpy() - f0).max()
            de = np.abs(e.cpu().numpy() - e0).max()
            dw = np.abs(w.cpu().numpy() - w0).max()
            assert de < 1e-4 and df < 1e-4 and dw < 1e-4, (mode, which, df, de, dw)      # the reference's bound, absolute


def test_ten_million_atoms_fp32_properties(emdee, dev):
    """BASELINE configs[3] at the size it is quoted on (fp32 storage and pair math, fp64 reductions).  Stored coordinates
    reach 232 sigma (ulp 1.5e-5); the force kernels work on brick-relative tile coordinates (one rounding at the ulp of a
    brick-sized number), so the in-cutoff pair count must be that of the fp64 engine on the SAME (fp32-representable)
    positions up to the pairs within rounding of the cutoff sphere, and the dynamics must conserve what it conserves."""
    E = emdee
    syn = E.synthetic
    pos, L = syn.fcc_positions(136)
    N = pos.shape[0]
    vel = syn.velocities(N)
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    model = E.LennardJonesModel(2.5, 2.0)
    x32 = pos.astype(np.float32)
    md64 = E.VelocityVerlet(E.cu(x32.astype(np.float64), dev), E.cu(vel.astype(np.float32).astype(np.float64), dev), float(np.float32(L)), model,
                            E.cu(atoms, dev), skin=0.3)
    pairs64 = md64.count_pairs()
    ep64, ek64, _ = md64.totals()
    # the SAME start in fp64, 400 steps: what the integrator itself does to the total energy (dt^2 truncation: -6e-6 after 40
    # steps of the melting lattice, -1e-6 after 400) -- the trace the fp32 run is to follow
    md64.step_(40, 0.005)
    a40 = sum(md64.totals()[:2])
    md64.step_(360, 0.005)
    a400 = sum(md64.totals()[:2])
    err64 = ((a40 - (ep64 + ek64)) / abs(ep64 + ek64), (a400 - (ep64 + ek64)) / abs(ep64 + ek64))
    md64.close()
    del md64
    torch.cuda.empty_cache()
    md = E.VelocityVerlet(E.cu(x32, dev), E.cu(vel.astype(np.float32), dev), L, model, E.cu(atoms, dev), skin=0.3)
    del pos, vel, x32
    ep0, ek0, _ = md.totals()
    pairs0 = md.count_pairs()
    # a pair flips only if r^2 is within the fp32 rounding of rc^2: |r^2 - rc^2| < ~1e-6 rc^2 holds for ~1e-6 * 3/2 of the pairs
    # (measured: 270,349,415 against 270,349,425 -- ten pairs)
    assert abs(pairs0 - pairs64) <= 1e-6 * pairs64, (pairs0, pairs64)
    assert abs(pairs0 / (0.5 * N) - 53.7) < 0.5                          # 53.7 on the jittered lattice (52.36 for a uniform fluid)
    assert ep0 == pytest.approx(ep64, rel=2e-6)                          # per-pair fp32 terms, fp64 sums
    md.step_(40, 0.005)
    ep1, ek1, _ = md.totals()
    e0, e1 = ep0 + ek0, ep1 + ek1
    assert abs(e1 - e0) < 5e-5 * abs(e0)                                   # NVE drift over 40 steps in fp32 (measured: -6e-6)
    md.step_(360, 0.005)
    ep2, ek2, _ = md.totals()
    e2 = ep2 + ek2
    print("fp32 10^7: pairs %d vs fp64 %d; E0 %.9g E40 %.9g E400 %.9g (rel %.2e, %.2e; the fp64 run: %.2e, %.2e)"
          % (pairs0, pairs64, e0, e1, e2, (e1 - e0) / abs(e0), (e2 - e0) / abs(e0), err64[0], err64[1]))
    assert abs(e2 - e0) < 5e-5 * abs(e0)                                   # ... and over 400 steps, ~55 rebuilds
    # Cell-relative records (round 5): the drift x += dt v rounds at the ulp of a cell-sized number, and the fp32 run's energy
    # error IS the fp64 run's (-5.99e-6 / -1.04e-6 both: same-box measurement, profiles/r05/fp32_drift.txt); with absolute fp32
    # records (EMDEE_F32_ABS=1, rounds 1-4) the 400-step figure was off by 2.2e-7 (-8.25e-7).
    assert abs((e1 - e0) / abs(e0) - err64[0]) < 5e-8 and abs((e2 - e0) / abs(e0) - err64[1]) < 5e-8
    st = md.state(positions=False, forces=False)
    p = st["velocities"].double().sum(dim=0).abs().max().item()
    assert p < 2e-5 * (N * 3.0) ** 0.5                                     # total momentum stays at rounding level (fixed-point tile
                                                                           # coordinates: F_ij = -F_ji to the bit; measured 2e-3, absolute records 0.8)
    assert md.nbr_stats()["builds"] >= 30 and md.nbr_stats()["max_count"] <= md.nbr_stats()["capacity"]
    assert abs(md.count_pairs() / (0.5 * N) - 52.36) < 2.0
    assert 2.0 * ek2 / (3 * N - 3) > 0.5                                   # the lattice is melting, not exploding


def test_same_box_with_very_different_density_profiles(emdee, oracle, dev):
    """Three configurations of the same box through one operator handle: uniform, a third of the atoms crowded into one
    corner (twice the density the first list was sized for: LDS tile capacity, row stride and build variant all have
    to be re-planned), then dilute again.  Neighbour set and forces must be the oracle's each time."""
    E = emdee
    rng = np.random.default_rng(11)
    N, L, rc, rs, skin = 24000, 36.0, 2.5, 2.0, 0.3
    model = E.LennardJonesModel(rc, rs)
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    tiles = E.nonbonded_computation_tiles(N)

    def jittered_grid(n, lo, hi):                                  # n points on a jittered cubic grid inside [lo, hi)^3: no overlaps
        m = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
        h = (hi - lo) / m
        return lo + (g + 0.5) * h + rng.uniform(-0.15, 0.15, size=(n, 3)) * h

    uniform = jittered_grid(N, 0.0, L)
    crowded = uniform.copy()
    crowded[:N // 3] = jittered_grid(N // 3, 0.0, 16.0)            # ~2 atoms per sigma^3 in the corner, spacing 0.8 sigma
    crowded[N // 3:] = jittered_grid(N - N // 3, 0.0, L)           # (overlaps between the two sets are possible: forces just get large)
    # keep every pair apart: drop the second set's atoms that fall inside the crowded corner
    inside = np.all(crowded[N // 3:] < 16.5, axis=1)
    crowded[N // 3:][inside] = rng.uniform(17.0, L - 0.5, size=(int(inside.sum()), 3))
    dilute = jittered_grid(N, 0.0, L)
    for k, x in enumerate((uniform, crowded, dilute)):
        f = torch.zeros((N, 3), dtype=torch.float64, device=dev)
        E.compute_nonbonded_(f, None, None, E.cu(x, dev), L, tiles, model, E.cu(atoms, dev), E.Val(E.FORCES))
        got = _rows(*tiles.neighbor_lists())
        want = _oracle_rows(oracle, x, L, rc + skin)
        for i in range(N):
            assert np.array_equal(got[i], want[i]), "configuration %d, row %d differs" % (k, i)
        fo, _, _ = oracle.nonbonded_cells(x.astype(np.float64), L, oracle.model(rc, rs), atoms)
        scale = np.abs(fo).max()
        assert np.abs(f.cpu().numpy() - fo).max() <= 1e-9 * scale
    assert tiles.stats()["builds"] >= 3


@pytest.mark.parametrize("rc,rs,cells", [(2.5, 2.0, 23), (3.5, 3.0, 29)])    # (cell side just above rc + skin, as in the 10^7-atom boxes: the tiles fit the typed planes)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_species_boxes_take_the_typed_kernels(emdee, oracle, dev, capfd, monkeypatch, rc, rs, cells, dtype):
    """Two distinct LJAtom values: the box is sorted by (cell, species), tiles are staged species-major, rows are built as one
    segment per neighbour species and the pair loop runs per segment with the pair constants in registers (csrc/typed.hpp;
    rc = 2.5: 512-thread workgroups, rc = 3.5: 1024).  Same per-pair arithmetic as the general-species kernels
    (EMDEE_NO_TYPED=1), which serve as the second witness next to the oracle: operator outputs, the neighbour SET, counted
    pairs and a trajectory."""
    E = emdee
    syn = E.synthetic
    pos, L = syn.fcc_positions(cells)
    N = pos.shape[0]
    pos = pos + 0.25 * (np.random.default_rng(7).random(pos.shape) - 0.5)
    types = syn.mixture_types(N)
    eps, sigma = syn.mixture_parameters(types)
    atoms = E.lennard_jones_atoms(eps, sigma)
    model = E.LennardJonesModel(rc, rs)
    x = pos.astype(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    out = {}
    for typed in (True, False):
        if typed:
            monkeypatch.delenv("EMDEE_NO_TYPED", raising=False)
            monkeypatch.setenv("EMDEE_F32_FAST", "1")          # (Float32 operator calls otherwise run the reference arithmetic on the general-species kernels)
        else:
            monkeypatch.setenv("EMDEE_NO_TYPED", "1")
        monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
        monkeypatch.setenv("EMDEE_TYPED_ALL", "1")             # short rows too (by default only the long-row boxes, where they win)
        capfd.readouterr()
        tiles = E.nonbonded_computation_tiles(N)
        f = torch.zeros((N, 3), dtype=tdt, device=dev)
        e = torch.zeros(N, dtype=tdt, device=dev)
        w = torch.zeros(N, dtype=tdt, device=dev)
        E.compute_nonbonded_(f, e, w, E.cu(x, dev), L, tiles, model, E.cu(atoms, dev), 7)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert ("typed kernels on" in err) == typed, err[-400:]
        f1 = torch.zeros((N, 3), dtype=tdt, device=dev)
        E.compute_nonbonded_(f1, None, None, E.cu(x, dev), L, tiles, model, E.cu(atoms, dev), 1)     # the forces-only kernel
        out[typed] = dict(f=f.cpu().numpy(), e=e.cpu().numpy(), w=w.cpu().numpy(), f1=f1.cpu().numpy(), rows=_rows(*tiles.neighbor_lists()),
                          pairs=tiles.count_pairs(), stats=tiles.stats())
        vel = syn.velocities(N)
        md = E.VelocityVerlet(E.cu(x, dev), E.cu(vel.astype(dtype), dev), L, model, E.cu(atoms, dev))
        md.step_(12, 0.004)
        out[typed]["x12"] = md.state()["positions"].cpu().numpy()
        out[typed]["md_pairs"] = md.count_pairs()
        md.close()
    monkeypatch.delenv("EMDEE_DEBUG_PLAN", raising=False)
    a, b = out[True], out[False]
    tol = 1e-12 if dtype == np.float64 else 2e-5
    for k in ("f", "e", "w", "f1"):
        assert np.abs(a[k] - b[k]).max() <= tol * np.abs(b[k]).max(), k
    assert np.abs(a["f1"] - a["f"]).max() <= tol * np.abs(a["f"]).max()
    # Float32 records are relative to their cell and tile coordinates relative to the tile's first cell: at rc = 3.5 the typed
    # kernels work on 2 x 2 x 2-cell bricks and the general-species ones on 4 x 2 x 2, so a pair within one rounding of r_c or
    # of r_list may fall on different sides in the two (Float64, and Float32 on equal bricks: identical)
    slack = 4 if (dtype == np.float32 and rc == 3.5) else 0
    assert abs(a["pairs"] - b["pairs"]) <= slack and abs(a["md_pairs"] - b["md_pairs"]) <= slack
    assert abs(a["stats"]["listed"] - b["stats"]["listed"]) <= slack and abs(a["stats"]["max_count"] - b["stats"]["max_count"]) <= (1 if slack else 0)
    differing = 0
    for i in range(N):
        if not np.array_equal(a["rows"][i], b["rows"][i]):
            differing += 1
            assert differing <= 2 * slack, "row %d: typed and general-species builds disagree" % i
            assert len(np.setxor1d(a["rows"][i], b["rows"][i])) <= 2
    dx = a["x12"] - b["x12"]
    assert np.abs(dx - L * np.rint(dx / L)).max() < (1e-10 if dtype == np.float64 else 2e-4)
    if dtype == np.float64:
        # the A/B baselines of round 5 stay honest: the (cell, species) sort without x quarters, and -- long rows -- the 4 x 2 x 2
        # bricks in 1024-thread workgroups, give the same rows and the same forces
        monkeypatch.delenv("EMDEE_NO_TYPED", raising=False)
        monkeypatch.setenv("EMDEE_TYPED_SUBBINS", "0")
        monkeypatch.setenv("EMDEE_TYPED_BRICKS", "7")
        monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
        capfd.readouterr()
        tiles = E.nonbonded_computation_tiles(N)
        f = torch.zeros((N, 3), dtype=tdt, device=dev)
        E.compute_nonbonded_(f, None, None, E.cu(x, dev), L, tiles, model, E.cu(atoms, dev), 1)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        assert "typed kernels on" in err and "variant 9" not in err, err[-400:]
        rows7 = _rows(*tiles.neighbor_lists())
        for i in range(N):
            assert np.array_equal(rows7[i], a["rows"][i]), "row %d: the baseline typed build disagrees" % i
        assert np.abs(f.cpu().numpy() - a["f"]).max() <= tol * np.abs(a["f"]).max()
        for k in ("EMDEE_TYPED_SUBBINS", "EMDEE_TYPED_BRICKS", "EMDEE_DEBUG_PLAN"):
            monkeypatch.delenv(k, raising=False)
    if dtype == np.float64:
        f0, e0, w0 = oracle.nonbonded_cells(pos, L, oracle.model(rc, rs), atoms)
        assert np.abs(a["f"] - f0).max() <= 1e-9 * np.abs(f0).max()
        assert np.abs(a["e"] - e0).max() <= 1e-9 * np.abs(e0).max() and np.abs(a["w"] - w0).max() <= 1e-9 * np.abs(w0).max()
        want = _oracle_rows(oracle, pos, L, rc + 0.3)
        for i in range(N):
            assert np.array_equal(a["rows"][i], want[i]), "row %d differs from the oracle's" % i


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("species", ["uniform", "five_species"])
def test_operator_calls_that_outrun_their_list(emdee, oracle, dev, monkeypatch, dtype, species):
    """compute_nonbonded_ on a kept handle, tiled box with x sub-bins (32,000 atoms): a call whose positions have moved past
    skin / 2 re-sorts from the records its own refresh pass has just written (round 4, csrc/impl.hpp NbrImpl::compute) -- against
    EMDEE_OPERATOR_RELOAD=1, which loads afresh from the caller's arrays as rounds 1-3 did.  Several such calls, with the LJAtom
    array edited in between (a uniform box that gets a new sigma; a five-species box whose species are dealt again): the
    same builds counter, the same neighbour rows, forces against the fp64 oracle, in both forms."""
    E = emdee
    rng = np.random.default_rng(41)
    rc, rs, skin = 2.5, 2.0, 0.3
    ndt = np.float64 if dtype == "f64" else np.float32
    tdt = torch.float64 if dtype == "f64" else torch.float32
    x0, L = E.synthetic.fcc_positions(20)
    N = x0.shape[0]
    x0 = x0 + rng.normal(0.0, 0.05, size=x0.shape)

    def make_atoms(seed, sigma_uniform):
        if species == "uniform":
            return np.full(N, 1.0), np.full(N, sigma_uniform)
        r = np.random.default_rng(seed)
        kind = r.integers(0, 5, N)
        return np.array([1.0, 0.8, 1.2, 0.5, 0.9])[kind], np.array([1.0, 0.95, 1.03, 0.9, 0.97])[kind]

    # (move amplitude, new LJAtom array or None)
    script = [(0.0, None), (0.05, None), (0.4, None), (0.3, (7, 1.04)), (0.02, None), (0.35, (9, 0.98)), (0.3, None)]
    runs = {}
    for form in ("resort", "reload"):
        if form == "reload":
            monkeypatch.setenv("EMDEE_OPERATOR_RELOAD", "1")
        x = x0.copy()
        eps, sigma = make_atoms(3, 1.0)
        tiles = E.nonbonded_computation_tiles(N, skin=skin)
        builds, out = [], []
        for call, (amp, edit) in enumerate(script):
            # a smooth displacement field (one long wave per call, another direction each time): atoms move past skin / 2
            # together with their neighbours, so the fluid stays a fluid (random kicks of 0.4 sigma would push pairs to r = 0.6)
            kv = np.roll(np.array([1.0, 2.0, 0.0]), call) * 2.0 * np.pi / L
            pol = np.roll(np.array([0.0, 0.6, 0.8]), call)
            x = x + amp * np.sin(x0 @ kv + 0.7 * call)[:, None] * pol[None, :]
            if edit is not None:
                eps, sigma = make_atoms(*edit)
            atoms = E.lennard_jones_atoms(eps, sigma)
            xs = x.astype(ndt)
            f = torch.zeros((N, 3), dtype=tdt, device=dev)
            e = torch.zeros(N, dtype=tdt, device=dev)
            E.compute_nonbonded_(f, e, None, E.cu(xs, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(E.FORCES | E.ENERGIES))
            builds.append(tiles.stats()["builds"])
            out.append((f.cpu().numpy().astype(np.float64), e.cpu().numpy().astype(np.float64), _rows(*tiles.neighbor_lists()), xs.astype(np.float64), atoms))
        runs[form] = (builds, out)
    monkeypatch.delenv("EMDEE_OPERATOR_RELOAD")
    assert runs["resort"][0] == runs["reload"][0] == [1, 1, 2, 3, 3, 4, 5], runs["resort"][0]
    om = oracle.model(rc, rs)
    for k in range(len(script)):
        fa, ea, ra, xs, atoms = runs["resort"][1][k]
        fb, eb, rb, _, _ = runs["reload"][1][k]
        f0, e0, _ = oracle.nonbonded_cells(xs, L, om, atoms)
        scale = np.abs(f0).max()
        tol = 1e-9 if dtype == "f64" else 2e-4
        assert np.abs(fa - f0).max() <= tol * scale and np.abs(fb - f0).max() <= tol * scale, (k, np.abs(fa - f0).max() / scale)
        assert np.abs(ea - e0).max() <= tol * np.abs(e0).max() and np.abs(eb - e0).max() <= tol * np.abs(e0).max()
        assert np.abs(fa - fb).max() <= (1e-12 if dtype == "f64" else 1e-4) * scale
        differing = sum(0 if np.array_equal(a, b) else 1 for a, b in zip(ra, rb))
        assert differing <= (0 if dtype == "f64" else 4), "call %d: %d rows differ between the re-sort and the reload" % (k, differing)
        if dtype == "f64" and builds_changed(runs["resort"][0], k):
            want = _oracle_rows(oracle, xs, L, rc + skin)
            for i in range(N):
                assert np.array_equal(ra[i], want[i]), "call %d row %d differs from the oracle" % (k, i)


def builds_changed(builds, k):
    return k == 0 or builds[k] != builds[k - 1]



def _pair_terms(oracle, x, L, om, atoms, pairs):
    """(f, e, w) contributions of the named pairs alone: the oracle's pair function (oracle.interaction = interaction() of
    src/lennard_jones.jl:25-42, CUTOFF mode) at the minimum-image distance (src/nonbonded.jl:40), f = W / r^2 r_ij and half
    of E and W to either atom (src/nonbonded.jl:136-145)."""
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


@pytest.mark.parametrize("path", ["tiled", "direct"])
def test_exclusions_and_scaled_14_pairs(emdee, oracle, dev, lj_sample, monkeypatch, path):
    """SURVEY.md 8(f) item 2, the hooks of src/modelling.jl:197-200 (lj14scale is parsed by the reference and consumed by
    nothing): a molecular-like box cut out of the reference's own fixture -- consecutive atoms of lj_sample.xyz chained into
    4-atom "molecules" (1-2 and 1-3 neighbours excluded, 1-4 pairs scaled by the lj14scale of the reference's force-field
    fixture) -- through compute_nonbonded_ and through the integrator, against the oracle's sum over ALL pairs minus the
    excluded pairs' terms plus the scaled 1-4 terms.  A 4,000-atom periodic copy takes the tiled kernels (rows filtered after
    the build, the pair loop has no mask), EMDEE_PATH=direct the global-gather ones."""
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    table = E.ingest.NonbondedTable(os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml"))
    s14 = table.lj14scale
    assert 0.0 < s14 < 1.0
    # 5 periodic images of the 800-atom fixture side by side along x: a box of 50 x 10 x 10 would break cubic periodicity, so
    # instead the fixture itself (L = 10, rc = 3: tiled kernels need L >= 2 (rc + skin), i.e. three cells: 10 / 3.3) is used as is
    x = lj_sample.astype(np.float64)
    N, L = x.shape[0], 10.0
    rc, rs = 3.0, 2.5
    kind = np.arange(N) % 4
    eps = np.array([1.0, 0.8, 1.1, 0.9])[kind]
    sigma = np.array([1.0, 0.9, 1.05, 0.95])[kind]
    atoms = E.lennard_jones_atoms(eps, sigma)
    mol = np.arange(N).reshape(-1, 4)
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]], mol[:, [0, 2]], mol[:, [1, 3]]])
    p14 = mol[:, [0, 3]]
    om = oracle.model(rc, rs)
    f0, e0, w0 = oracle.nonbonded_cells(x, L, om, atoms)
    fx, ex, wx = _pair_terms(oracle, x, L, om, atoms, excl)
    f4, e4, w4 = _pair_terms(oracle, x, L, om, atoms, p14)
    want = (f0 - fx - (1.0 - s14) * f4, e0 - ex - (1.0 - s14) * e4, w0 - wx - (1.0 - s14) * w4)
    assert np.abs(fx).max() > 1e-3 * np.abs(f0).max()                     # the named pairs are inside the cutoff: they matter

    tiles = E.nonbonded_computation_tiles(N, skin=0.3)
    tiles.set_exclusions_(excl)
    tiles.set_pairs14_(p14, s14)
    f, e, w = (torch.zeros(s, dtype=torch.float64, device=dev) for s in ((N, 3), (N,), (N,)))
    E.compute_nonbonded_(f, e, w, E.cu(x, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(7))
    for got, ref in zip((f, e, w), want):
        assert np.abs(got.cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
    # the rows no longer hold the named pairs (either direction), and nothing else went missing
    rows = _rows(*tiles.neighbor_lists())
    full = _oracle_rows(oracle, x, L, rc + 0.3)
    named = {(int(a), int(b)) for a, b in np.concatenate([excl, p14])} | {(int(b), int(a)) for a, b in np.concatenate([excl, p14])}
    for i in range(N):
        assert np.array_equal(rows[i], np.array([j for j in full[i] if (i, int(j)) not in named], dtype=rows[i].dtype)), i
    # a second call after a move past skin / 2 (the re-sort filters again), and clearing the tables gives the plain sum back
    x2 = x + 0.25 * np.sin(x[:, [1, 2, 0]])
    E.compute_nonbonded_(f, e, w, E.cu(x2, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(7))
    g0 = oracle.nonbonded_cells(x2, L, om, atoms)
    gx, g4 = _pair_terms(oracle, x2, L, om, atoms, excl), _pair_terms(oracle, x2, L, om, atoms, p14)
    for got, a, b, c in zip((f, e, w), g0, gx, g4):
        ref = a - b - (1.0 - s14) * c
        assert np.abs(got.cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
    tiles.set_exclusions_(None)
    tiles.set_pairs14_(None, 1.0)
    E.compute_nonbonded_(f, e, w, E.cu(x2, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(7))
    assert np.abs(f.cpu().numpy() - g0[0]).max() <= 1e-9 * np.abs(g0[0]).max()

    # the integrator: 1-4 pairs make it step with the split kernels; 20 steps against the oracle's trajectory of the same
    # modified potential are out of the oracle's reach (it has no exclusions), so: forces at the start, and energy conservation
    v0 = 0.3 * E.synthetic.velocities(N)
    md = E.VelocityVerlet(E.cu(x, dev), E.cu(v0, dev), L, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=0.3)
    md.set_exclusions_(excl)
    md.set_pairs14_(p14, s14)
    st = md.state(energies=True, virials=True)
    assert np.abs(st["forces"].cpu().numpy() - want[0]).max() <= 1e-6 * np.abs(want[0]).max()
    assert np.abs(st["energies"].cpu().numpy() - want[1]).max() <= 1e-6 * np.abs(want[1]).max()
    ep0, ek0, _ = md.totals()
    md.step_(80, 0.001)
    ep1, ek1, _ = md.totals()
    assert md.nbr_stats()["builds"] >= 2
    # (the fixture is not an equilibrium of the modified potential: excluded neighbours fall into each other and the box
    # heats up several-fold in these steps -- what must hold is the total, to the integrator's dt^2)
    assert abs((ep1 + ek1) - (ep0 + ek0)) <= 2e-5 * abs(ep0), ((ep0, ek0), (ep1, ek1))
    half = E.VelocityVerlet(E.cu(x, dev), E.cu(v0, dev), L, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=0.3)
    half.set_exclusions_(excl)
    half.set_pairs14_(p14, s14)
    half.step_(40, 0.002)
    eph, ekh, _ = half.totals()
    assert abs((eph + ekh) - (ep0 + ek0)) > 2.5 * abs((ep1 + ek1) - (ep0 + ek0))          # ... and it shrinks with dt^2


@pytest.mark.parametrize("path", ["tiled", "direct"])
def test_invalid_pair_tables_leave_the_previous_ones_in_force(emdee, dev, lj_sample, monkeypatch, path):
    """The undivided counterpart of test_gpu_dd_pairs.py::test_refusals: every emdee_md_set_* / emdee_nbr_set_* is all or
    nothing.  A pair of one atom, a negative index or an index equal to N in either table returns EMDEE_ERR_INVALID, and the
    engine then steps / computes bit for bit like a twin that never saw the bad calls; a call that clears only one table
    afterwards succeeds (the bad pairs were not kept)."""
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    x = lj_sample.astype(np.float64)
    N, L, rc, rs = x.shape[0], 10.0, 3.0, 2.5
    atoms = E.lennard_jones_atoms(np.array([1.0, 0.8, 1.1, 0.9])[np.arange(N) % 4], np.array([1.0, 0.9, 1.05, 0.95])[np.arange(N) % 4])
    mol = np.arange(N).reshape(-1, 4)
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]], mol[:, [0, 2]], mol[:, [1, 3]]])
    p14, s14 = mol[:, [0, 3]], 0.5
    bads = ([[3, 3]], [[-1, 5]], [[0, N]])
    ERR_INVALID = -1

    def dev_pairs(p):
        return torch.as_tensor(np.asarray(p)).to(device=dev, dtype=torch.int32).contiguous()

    # emdee_md
    v0 = 0.3 * E.synthetic.velocities(N)
    a, b = (E.VelocityVerlet(E.cu(x, dev), E.cu(v0, dev), L, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=0.3) for _ in range(2))
    for md in (a, b):
        md.set_exclusions_(excl)
        md.set_pairs14_(p14, s14)
    for bad in bads:
        with pytest.raises(E.EmDeeError) as err:
            a.set_exclusions_(np.concatenate([excl[:7], np.array(bad)]))
        assert err.value.code == ERR_INVALID
        with pytest.raises(E.EmDeeError) as err:
            a.set_pairs14_(np.array(bad), s14)
        assert err.value.code == ERR_INVALID

    def same(ma, mb):
        sa, sb = ma.state(energies=True, virials=True), mb.state(energies=True, virials=True)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k

    for md in (a, b):
        md.step_(30, 0.001)
    same(a, b)
    for md in (a, b):
        md.set_pairs14_(None, 1.0)                                   # clears the 1-4 table only
        md.step_(10, 0.001)
    same(a, b)
    a.close(); b.close()

    # emdee_nbr (the C calls on the handle: the Python wrapper re-sends both tables it holds at every call)
    ta, tb = (E.nonbonded_computation_tiles(N, skin=0.3) for _ in range(2))
    outs = []
    for tiles in (ta, tb):
        tiles.set_exclusions_(excl)
        tiles.set_pairs14_(p14, s14)
        out = tuple(torch.zeros(s, dtype=torch.float64, device=dev) for s in ((N, 3), (N,), (N,)))
        E.compute_nonbonded_(*out, E.cu(x, dev), L, tiles, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), E.Val(7))
        outs.append(out)
    h = ta._handle
    for bad in bads:
        for name, t, extra in (("emdee_nbr_set_exclusions", dev_pairs(np.concatenate([excl[:7], bad])), ()),
                               ("emdee_nbr_set_pairs14", dev_pairs(bad), (s14,))):
            with pytest.raises(E.EmDeeError) as err:
                E._lib.call(name, h, ctypes.c_void_p(t.data_ptr()), int(t.shape[0]), *extra)
            assert err.value.code == ERR_INVALID
    x2 = x + 0.25 * np.sin(x[:, [1, 2, 0]])                           # past skin / 2: the rows are built and filtered again
    for step in ("same positions", "moved", "1-4 cleared"):
        if step == "1-4 cleared":
            for tiles in (ta, tb):
                E._lib.call("emdee_nbr_set_pairs14", tiles._handle, None, 0, 1.0)
        for tiles, out in zip((ta, tb), outs):
            E.compute_nonbonded_(*out, E.cu(x if step == "same positions" else x2, dev), L, tiles, E.LennardJonesModel(rc, rs),
                                 E.cu(atoms, dev), E.Val(7))
        for qa, qb in zip(*outs):
            assert torch.equal(qa, qb), step
    ta.close(); tb.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exclusions_on_a_single_species_box(emdee, oracle, dev, dtype):
    """The kernel class of the headline box -- one LJAtom value: coordinate-plane tiles, list entries stored as byte offsets into
    the planes -- with an exclusion table: a 32,000-atom jittered lattice (tiled kernels, x sub-bins), every atom's lattice
    neighbour pairs 2k / 2k + 1 excluded.  Operator outputs and the integrator's forces against the oracle's full sum minus
    the named pairs; Float32 through the integrator's brick-relative tiles (EMDEE_F32_FAST) so that the filtered rows are
    the ones the fp32 MD kernels walk.  The rows hold every listed neighbour but the named ones."""
    E = emdee
    x0, L = E.synthetic.fcc_positions(20)
    N = x0.shape[0]
    rc, rs = 2.5, 2.0
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    ndt = np.float64 if dtype == "f64" else np.float32
    tdt = torch.float64 if dtype == "f64" else torch.float32
    x = x0.astype(ndt)
    x64 = x.astype(np.float64)
    excl = np.arange(N).reshape(-1, 2)                                   # consecutive atoms of an fcc cell: first neighbours
    om = oracle.model(rc, rs)
    f0, e0, w0 = oracle.nonbonded_cells(x64, L, om, atoms)
    fx, ex, wx = _pair_terms(oracle, x64, L, om, atoms, excl)
    assert np.abs(fx).max() > 1e-2 * np.abs(f0).max()
    want_f, want_e = f0 - fx, e0 - ex
    tol = 1e-6 if dtype == "f64" else 2e-4
    md = E.VelocityVerlet(E.cu(x, dev), E.cu(np.zeros_like(x), dev), L, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=0.3)
    md.set_exclusions_(excl)
    st = md.state(energies=True)
    assert np.abs(st["forces"].cpu().numpy() - want_f).max() <= tol * np.abs(want_f).max()
    assert np.abs(st["energies"].cpu().numpy() - want_e).max() <= tol * np.abs(want_e).max()
    rows = _rows(*md.neighbor_lists())
    full = _oracle_rows(oracle, x64, L, rc + 0.3)
    partner = np.arange(N) ^ 1
    bad = 0
    for i in range(N):
        expect = full[i][full[i] != partner[i]]
        if not np.array_equal(rows[i], expect):
            bad += 1
            # (Float32: a pair within one rounding of r_list may be listed or not; the named pair must be gone either way)
            assert dtype == "f32" and partner[i] not in rows[i] and len(np.setxor1d(rows[i], expect)) <= 2, i
    assert bad <= (0 if dtype == "f64" else 16)
    # a few steps with rebuilds: the re-sorted state is filtered again (the pair would otherwise come back into the rows)
    md2 = E.VelocityVerlet(E.cu(x, dev), E.cu((0.8 * E.synthetic.velocities(N)).astype(ndt), dev), L, E.LennardJonesModel(rc, rs), E.cu(atoms, dev), skin=0.3)
    md2.set_exclusions_(excl)
    md2.step_(40, 0.004)
    assert md2.nbr_stats()["builds"] >= 3
    rows2 = _rows(*md2.neighbor_lists())
    assert all(partner[i] not in rows2[i] for i in range(0, N, 7))
    md.close(); md2.close()


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("family", ["uniform", "species3", "long_rows", "typed", "typed_all", "direct", "long_rows_charged"])
def test_plan_lines_match_the_recorded_ones(emdee, dev, capfd, monkeypatch, family, bits):
    """The `emdee plan:` lines of the family boxes of tests/helpers/mask_cases.py, and of the charged long-row box under the
    reaction field and under Ewald summation, are byte for byte the ones recorded in tests/golden/plan_lines.json before the
    planner became a function (tests/test_plan_host.py feeds the same file to choose_plan on the host)."""
    import json

    from .helpers import plan_cases as pc
    with open(os.path.join(GOLDEN, "plan_lines.json")) as fh:
        want = {(c["case"], c["bits"], c["event"]): c for c in json.load(fh)}
    box, events = pc.run(emdee, dev, family, bits, lambda: capfd.readouterr().err, monkeypatch.setenv)
    assert events
    for event, stride, lines in events:
        rec = want[(family, bits, event)]
        assert pc.facts(box, family, bits, event, stride) == rec["facts"]
        assert lines == rec["lines"], (family, bits, event)
