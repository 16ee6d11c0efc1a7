"""GPU tests of positions in far periodic images and of the bound on the per-atom image counts.

The interface takes positions anywhere (emdee_md_set_state, the operator path, emdee_dd_set_atoms) and emdee_md_get_state answers
in the caller's image.  Elsewhere in the suite the furthest an atom sits outside its box is two box lengths.

1. Exact boxes (tests/helpers/image_cases.py: every length of a family box scaled so that the side is a power of two, every
   coordinate on the grid side 2^-13).  Adding up to 500 box lengths to a coordinate is then exact in Float32 as in Float64, and
   so are the wrap, the binning and the scaled differences of the operator path: the engine must build the SAME records from
   shifted and from unshifted input, and every output must agree bit for bit -- at the load, after 12 steps with at least two
   displacement-triggered rebuilds, through the operator path (tiled and direct, a second call with a third of the atoms in yet
   another image included), the all-pairs kernels, the Cells API (index = 1 + vx + M vy + M^2 vz with v = floor(M (s - floor s))
   evaluated by numpy in the engine's type) and decomposed engines.  Positions come back as the unshifted engine's plus k len:
   exactly at the load; after steps both engines round the same exact sum record + count x len once, at different magnitudes, so
   they agree to half a unit in the last place of the shifted one where the records are absolute and the unshifted atom sits
   inside the box, to one unit of the larger otherwise (the only bound of this section, and it is the number format's).
2. General boxes in Float64, far images against the existing yardsticks at the existing bounds: the orthorhombic family box
   with lo != 0, the charged boxes under Ewald and PME (with and without the chain tables), the rigid water box with every ATOM
   of a molecule in an image of its own.  At the load and after a step.
3. Faces (image_cases.with_face_atoms): per axis an atom exactly on lo, on lo + len, on every cell face and on the neighbours of
   those numbers in the engine's type.  Rows, outputs and positions at the load and behind a rebuild, the same atoms as their
   other images, a run in which they cross their faces both ways, the operator path and 2 x 2 x 2 domains.  Rows are compared
   up to the band about rc + skin (every pair inside it less the band listed, none beyond it plus the band); no pair of an atom
   on a face lies in the band, so for those rows that is equality.  The two-species box of 97556 atoms is sheared first and checked on sampled rows; it has no crossing run.
4. The bound on the counts (include/emdee_hip.h, emdee_md_set_state): a load 600 box lengths out is refused with
   EMDEE_ERR_INVALID naming atom, axis and count, on the absolute and on the cell-relative records, and a valid load follows; an
   atom that flies 0.75 box lengths per step returns x0 + 400 dt v exactly after 400 steps, the call that takes its count past
   the field returns EMDEE_ERR_STATE, the engine then refuses to step, and the other atom's position is exact throughout.

The CPU-side conditions (coordinates on the grid, shifted sums exact in Float32, the free-flight rebuild count) are plain asserts
of the helpers and run before any device work."""
import numpy as np
import pytest

from .helpers import image_cases as ic
from .helpers import mask_cases as mc
from .helpers import ortho_ref as oref
from .test_gpu_bonded import _outputs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTYPES = [np.float64, np.float32]
DRAWS = ["uniform", "extremes"]
ERR_INVALID, ERR_STATE = -1, -6


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _box(E, name, dtype):
    box = ic.ortho_box(E) if name == "ortho" else ic.dyadic_box(E, name, dtype)
    ic.assert_dyadic(box)
    return box


def _engine(E, dev, box, pos, dtype, post="none", charges=None, vel=None):
    md = E.VelocityVerlet(E.cu(pos.astype(dtype), dev), E.cu((box["vel"] if vel is None else vel).astype(dtype), dev), box["lengths"][0],
                          E.LennardJonesModel(box["rc"], box["rs"]), E.cu(box["atoms"], dev), skin=box["skin"], lo=box["lo"],
                          lengths=box["lengths"], periodic=box["periodic"])
    excl, p14, terms = mc.tables(pos.shape[0], post)
    if excl is not None:
        md.set_exclusions_(excl)
        md.set_pairs14_(p14, mc.S14)
    for kind, a, p in terms or []:
        md.set_bonded_(kind, a, p)
    if charges is not None:
        md.set_coulomb_(charges, 1.0, np.inf, mc.C14)
    if box.get("excl") is not None:
        md.set_exclusions_(box["excl"])
    return md


def _rows(md):
    counts, nb = md.neighbor_lists()
    counts, nb = counts.cpu().numpy(), nb.cpu().numpy().astype(np.int64)
    nb[np.arange(nb.shape[1])[None, :] >= counts[:, None]] = np.iinfo(np.int64).max        # (behind the row's end)
    return counts, np.sort(nb, axis=1)


def _same_rows(a, b, what):
    """the rows as sets: the same counts and, sorted, the same ids (a pair listed twice would show in the count)"""
    assert np.array_equal(a[0], b[0]), "%s: row lengths differ" % what
    w = min(a[1].shape[1], b[1].shape[1])
    assert np.array_equal(a[1][:, :w], b[1][:, :w]), "%s: rows differ" % what


def _same_bits(a, b, what):
    for name, x, y in zip(("forces", "energies", "virials", "tensors", "tensor sums"), a, b):
        assert np.array_equal(x, y), "%s: %s differ, max %.3e" % (what, name, np.abs(x - y).max())


def _positions(md):
    return md.state(velocities=False, forces=False)["positions"].cpu().numpy()


# ---------------------------------------------------------------- 1. exact boxes, the integrator
MD_CASES = [(f, "none", False) for f in mc.FAMILIES + ["ortho"]] + [("species3", "bonded", True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,post,charged", MD_CASES)
def test_whole_box_shifts_leave_every_bit_of_the_integrator(emdee, dev, capfd, monkeypatch, family, post, charged, dtype):
    """(species3 / bonded / charged: the chain tables of mask_cases with their reaction-field charges -- every atom of a chain in
    an image of its own, so the chained minimum image of the bonded terms and the 1-4 look-up see the shift.)"""
    E = emdee
    box = _box(E, family, dtype)
    N = box["pos"].shape[0]
    ic.assert_rebuilds_twice(box)
    shifts = {draw: ic.image_counts(N, draw) for draw in DRAWS}
    inputs = {draw: ic.shifted(box, k) for draw, k in shifts.items()}
    assert np.abs(shifts["uniform"]).max() == ic.KMAX and (shifts["uniform"] < 0).any()
    q = np.tile(mc.CHAIN_CHARGES, N // 4) if charged else None
    for k, v in box["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    base = _engine(E, dev, box, box["pos"], dtype, post, q)
    torch.cuda.synchronize()
    box["plan"](capfd.readouterr().err)                    # (the chain tables and charges leave the family's plan text as it is)
    L = np.asarray(box["lengths"])
    out0, rows0, x0, tot0 = _outputs(base), _rows(base), _positions(base), base.totals()
    assert np.array_equal(x0.astype(np.float64), box["pos"]), "the unshifted engine hands back other positions than it was given"
    base.step_(ic.STEPS, ic.DT)
    assert base.nbr_stats()["builds"] >= 3, "the run must rebuild at least twice"
    out1, rows1, x1, tot1 = _outputs(base), _rows(base), _positions(base), base.totals()
    v1 = base.state(positions=False, forces=False)["velocities"].cpu().numpy()
    base.close()
    for draw in DRAWS:
        what = "%s/%s %s" % (family, post, draw)
        md = _engine(E, dev, box, inputs[draw], dtype, post, q)
        _same_bits(_outputs(md), out0, what + " at the load")
        assert md.totals() == tot0, what
        assert np.array_equal(_positions(md).astype(np.float64), inputs[draw]), what + ": positions at the load"
        _same_rows(_rows(md), rows0, what + " at the load")
        md.step_(ic.STEPS, ic.DT)
        _same_bits(_outputs(md), out1, what + " after the steps")
        assert md.totals() == tot1, what
        assert np.array_equal(md.state(positions=False, forces=False)["velocities"].cpu().numpy(), v1), what + ": velocities"
        _same_rows(_rows(md), rows1, what + " after the steps")
        x = _positions(md)
        want = x1.astype(np.longdouble) + shifts[draw] * L.astype(np.longdouble)     # (exact: 53 + 9 bits in 64)
        # Absolute records (Float64; Float32 on the direct kernels): the shifted engine rounds record + count x len once, half a
        # unit in its last place; the unshifted engine's position IS the record where its count is 0 (inside the box) and carries
        # half a unit of its own otherwise.  Cell-relative Float32 records (the brick kernels): both engines round origin +
        # record + count x len, one unit of the larger together.
        sp = lambda a: np.spacing(np.abs(a).astype(dtype)).astype(np.float64)
        if dtype == np.float64 or family == "direct":
            lo = np.asarray(box["lo"])
            inside = (x1 >= lo) & (x1 < lo + L)
            bound = 0.5 * sp(x) + np.where(inside, 0.0, 0.5 * sp(x1))
        else:
            bound = sp(np.maximum(np.abs(x), np.abs(x1)))
        worst = float((np.abs(x.astype(np.longdouble) - want) / bound).max())
        print("%s: positions after the steps within %.2f of the rounding bound of the unshifted engine's plus k len" % (what, worst))
        assert worst <= 1.0, what
        md.close()


# ---------------------------------------------------------------- 1. exact boxes, the operator path
def _operator(E, dev, box, tiles, pos, dtype, tensor=True):
    N = pos.shape[0]
    tdt = _tdt(dtype)
    xd, ad = E.cu(pos.astype(dtype), dev), E.cu(box["atoms"], dev)
    model = E.LennardJonesModel(box["rc"], box["rs"])
    f, e, w = torch.zeros((N, 3), dtype=tdt, device=dev), torch.zeros(N, dtype=tdt, device=dev), torch.zeros(N, dtype=tdt, device=dev)
    E.compute_nonbonded_(f, e, w, xd, box["lengths"][0], tiles, model, ad, E.Val(7))
    out = [f, e, w]
    if tensor:
        t = torch.zeros((N, 6), dtype=tdt, device=dev)
        E.compute_virial_tensor_(t, xd, box["lengths"][0], tiles, model, ad)
        out.append(t)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_whole_box_shifts_leave_every_bit_of_the_operator_path(emdee, dev, capfd, monkeypatch, family, dtype):
    E = emdee
    box = _box(E, family, dtype)
    N = box["pos"].shape[0]
    for k, v in box["env"].items():
        monkeypatch.setenv(k, v)
    if family.startswith("typed") and dtype == np.float32:
        monkeypatch.setenv("EMDEE_F32_FAST", "1")            # (as tests/test_gpu_masks.py: the typed kernels carry the fast arithmetic)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    tiles = E.nonbonded_computation_tiles(N, skin=box["skin"])
    want = _operator(E, dev, box, tiles, box["pos"], dtype)
    torch.cuda.synchronize()
    box["plan"](capfd.readouterr().err)
    tiles.close()
    names = ("forces", "energies", "virials", "tensors")
    for draw in DRAWS:
        k = ic.image_counts(N, draw)
        tiles = E.nonbonded_computation_tiles(N, skin=box["skin"])
        got = _operator(E, dev, box, tiles, ic.shifted(box, k), dtype)
        for name, a, b in zip(names, got, want):
            assert np.array_equal(a, b), "%s %s: %s of the first call differ, max %.3e" % (family, draw, name, np.abs(a - b).max())
        builds = tiles.stats()["builds"]
        # a third of the atoms in yet another image, nothing else changed: the list is kept and the bits stay
        k2 = k.copy()
        k2[::3] = ic.image_counts(N, draw, seed=0x2B7F)[::3]
        assert (k2 != k).any()
        got = _operator(E, dev, box, tiles, ic.shifted(box, k2), dtype)
        for name, a, b in zip(names, got, want):
            assert np.array_equal(a, b), "%s %s: %s of the second call differ, max %.3e" % (family, draw, name, np.abs(a - b).max())
        assert tiles.stats()["builds"] == builds, "%s %s: atoms moved by whole box lengths made the list rebuild" % (family, draw)
        tiles.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["cutoff", "literal"])
@pytest.mark.parametrize("kernel", ["tiles", "naive"])
def test_whole_box_shifts_leave_every_bit_of_the_all_pairs_kernels(emdee, oracle, dev, kernel, mode, dtype):
    """CUTOFF: every output bit for bit.  LITERAL: energies and virials bit for bit, the forces not -- found by this test, first
    run: max |dF| 4.4e-5 of 52.  Nothing rounds (s = r / L, the differences, s - rint(s) and L times it are exact on these
    boxes); on the 2^-13 grid some pairs sit EXACTLY half a box apart along an axis, rint breaks that tie to the even integer
    (allpairs.hpp pair_terms, the reference's round), and which of the two equally near images that is depends on the parity
    of the shift.  r^2, E and W are the same for both; the force component along that axis changes sign.  CUTOFF drops such
    pairs (half a box is beyond rc), LITERAL sums them.  Either answer is a minimum image, so the forces of each run are held
    to the oracle's statement of the same arithmetic on the same input, at the bound tests/test_gpu_masks.py uses for the
    all-pairs family (1e-6 / 1e-4 of the largest entry)."""
    E = emdee
    box = _box(E, "uniform", dtype)
    N, L = box["pos"].shape[0], box["lengths"][0]
    tdt = _tdt(dtype)
    model, ad = E.LennardJonesModel(box["rc"], box["rs"]), E.cu(box["atoms"], dev)
    md = E.LITERAL if mode == "literal" else E.CUTOFF
    s = box["pos"][:, 0] / L
    assert (np.abs(s[:, None] - s[None, :]) == 0.5).any(), "the box has pairs exactly half a side apart (the tie of the docstring)"
    assert 0.5 * L > box["rc"]

    def run(pos):
        xd = E.cu(pos.astype(dtype), dev)
        f, e, w = torch.zeros((N, 3), dtype=tdt, device=dev), torch.zeros(N, dtype=tdt, device=dev), torch.zeros(N, dtype=tdt, device=dev)
        if kernel == "naive":
            E.naively_compute_nonbonded_(f, e, w, xd, L, model, ad, mode=md)
        else:
            E.compute_nonbonded_(f, e, w, xd, L, E.nonbonded_computation_tiles(N, all_pairs=True, mode=md), model, ad, E.Val(7))
        return [o.cpu().numpy() for o in (f, e, w)]

    def against_the_oracle(f, pos, what):
        f0 = oracle.naive(pos.astype(dtype), L, oracle.model(box["rc"], box["rs"], dtype), box["atoms"], oracle.LITERAL)[0]
        err = np.abs(f.astype(np.float64) - f0).max() / np.abs(f0).max()
        print("%s: forces against the oracle %.3e" % (what, err))
        assert err <= (1e-6 if dtype == np.float64 else 1e-4), what

    want = run(box["pos"])
    assert np.abs(want[0]).max() > 0
    if mode == "literal":
        against_the_oracle(want[0], box["pos"], "%s unshifted" % kernel)
    for draw in DRAWS:
        pos = ic.shifted(box, ic.image_counts(N, draw))
        got = run(pos)
        for name, a, b in zip(("forces", "energies", "virials"), got, want):
            if mode == "literal" and name == "forces":
                against_the_oracle(a, pos, "%s %s" % (kernel, draw))
            else:
                assert np.array_equal(a, b), "%s %s %s: %s differ, max %.3e" % (kernel, mode, draw, name, np.abs(a - b).max())


# ---------------------------------------------------------------- 1. exact boxes, the Cells API
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("draw", ["none"] + DRAWS)
def test_cells_index_follows_the_rule_of_the_header_in_far_images(emdee, dev, draw, dtype):
    E = emdee
    box = _box(E, "uniform", dtype)
    N = box["pos"].shape[0]
    pos = box["pos"] if draw == "none" else ic.shifted(box, ic.image_counts(N, draw))
    L = box["lengths"][0]
    cells = E.Cells(E.cu(pos.astype(dtype), dev), L, box["rc"], ndiv=2)
    M = cells.M
    s = pos.astype(dtype) / dtype(L)
    v = np.floor(dtype(M) * (s - np.floor(s))).astype(np.int64)
    assert s.dtype == dtype and (v >= 0).all() and (v < M).all()
    want = 1 + v[:, 0] + M * v[:, 1] + M * M * v[:, 2]
    assert np.array_equal(cells.index.cpu().numpy().astype(np.int64), want)
    assert np.array_equal(cells.population.cpu().numpy(), np.bincount(want - 1, minlength=M ** 3))
    cells.close()


# ---------------------------------------------------------------- 1. exact boxes, decomposed engines
def _decomposed(E, dev, box, pos, world, dtype):
    N = pos.shape[0]
    dd = E.DomainDecomposition(box["lengths"], E.domain.rank_grid(world), E.LennardJonesModel(box["rc"], box["rs"]), skin=box["skin"],
                               dtype=_tdt(dtype), device=dev)
    for r in range(world):
        mine = np.arange(r, N, world)
        dd.set_atoms_(r, E.cu(pos[mine].astype(dtype), dev), E.cu(box["vel"][mine].astype(dtype), dev), E.cu(box["atoms"][mine], dev),
                      torch.from_numpy(mine.astype(np.int64)).to(dev))
    dd.load_()
    return dd


def _gathered(dd, world, N, dtype):
    x, v, f = np.zeros((N, 3), dtype=dtype), np.zeros((N, 3), dtype=dtype), np.zeros((N, 3), dtype=dtype)
    owner = np.full(N, -1)
    for r in range(world):
        gid, xr, vr, fr = (t.cpu().numpy() for t in dd.state(r))
        assert dd.counts(r)["n_owned"] == gid.shape[0]
        assert (owner[gid] == -1).all(), "an atom is owned twice"
        owner[gid] = r
        x[gid], v[gid], f[gid] = xr, vr, fr
    assert (owner >= 0).all(), "an atom is owned by no domain"
    return x, v, f, owner


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("world", [2, 8])
def test_whole_box_shifts_leave_every_bit_of_a_decomposed_run(emdee, dev, world, dtype):
    E = emdee
    box = _box(E, "species3", dtype)
    N = box["pos"].shape[0]
    assert tuple(E.domain.rank_grid(world)) == ((2, 1, 1) if world == 2 else (2, 2, 2))
    base = _decomposed(E, dev, box, box["pos"], world, dtype)
    a0 = _gathered(base, world, N, dtype)
    assert np.array_equal(a0[0].astype(np.float64), box["pos"]), "a decomposed engine hands back wrapped positions"
    base.step_(ic.STEPS, ic.DT)
    a1 = _gathered(base, world, N, dtype)
    base.close()
    for draw in DRAWS:
        dd = _decomposed(E, dev, box, ic.shifted(box, ic.image_counts(N, draw)), world, dtype)
        for name, got, want in zip(("positions", "velocities", "forces", "owners"), _gathered(dd, world, N, dtype), a0):
            assert np.array_equal(got, want), "%d domains %s: %s at the load" % (world, draw, name)
        dd.step_(ic.STEPS, ic.DT)
        for name, got, want in zip(("positions", "velocities", "forces", "owners"), _gathered(dd, world, N, dtype), a1):
            assert np.array_equal(got, want), "%d domains %s: %s after the steps" % (world, draw, name)
        dd.close()


# ---------------------------------------------------------------- 2. general boxes, Float64: far images against the yardstick
X64 = 1e-8                                                  # positions after a step (tests/test_gpu_orthorhombic.py)
OFFSETS = np.array([-3.7, 1.9, 11.3])                      # lo of the orthorhombic family box here (that module's offsets)
TOL64, TOL64_CHARGED = 1e-6, 1e-9                          # tests/test_gpu_masks.py: TOL and TOL_CHARGED at Float64


def _far(pos, lo, lengths, periodic, seed):
    """every atom in an image of its own on the periodic axes, up to 500 box lengths out"""
    k = ic.image_counts(pos.shape[0], "uniform", seed=seed) * np.asarray(periodic)
    return pos + np.asarray(lo) + k * np.asarray(lengths), k


def _close(got, want, tol, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max()
    print("%s: max error / max entry = %.3e (bound %.0e)" % (what, err, tol))
    assert err <= tol, what


def _fewv(md):
    st = md.state(positions=False, energies=True, virials=True)
    return [st[k].cpu().numpy().astype(np.float64) for k in ("forces", "energies", "virials", "velocities")]


def _far_case(md, x_in, lo, box, ref0, ref1, tol, what, rows=None):
    """The load against ref0 = (f, e, w) of the wrapped positions, positions handed back in the caller's image, then one step:
    x1 = x0 + dt v0 + dt^2 / 2 f0 from the reference's forces, and the engine's forces there against ref1(x1) (rows: on these
    atoms only -- the sampled mode of the yardstick, whole rows)."""
    L, per = np.asarray(box["lengths"]), box["periodic"]
    f, e, w, v = _fewv(md)
    for name, g, r in zip(("forces", "energies", "virials"), (f, e, w), ref0):
        _close(g, r, tol, "%s at the load: %s" % (what, name))
    x = _positions(md).astype(np.float64)
    # (a coordinate 500 sides out carries 500 len 2^-53 of rounding from the wrap and as much from the way back)
    assert np.abs(x - x_in).max() <= 2 * ic.KMAX * L.max() * 2.0 ** -53, what + ": positions at the load are not the caller's"
    v0 = box["vel"]
    x1 = x_in + ic.DT * v0 + 0.5 * ic.DT ** 2 * ref0[0]
    md.step_(1, ic.DT)
    x = _positions(md).astype(np.float64)
    assert np.abs(np.rint((x - x1) / L) * np.asarray(per)).max() == 0, what + ": an atom came back in another image after the step"
    dx = np.abs(oref.image_difference(x, x1, L, per)).max()
    f, e, w, v = _fewv(md)
    r1 = ref1(oref.wrapped(x1, lo, L, per) - np.asarray(lo))
    sel = slice(None) if rows is None else rows
    dv = np.abs(v - (v0 + 0.5 * ic.DT * (ref0[0] + r1[0])))[sel].max()
    print("%s after one step: max |dx| %.3e, max |dv| %.3e" % (what, dx, dv))
    assert dx < X64 and dv < 10 * X64, what
    for name, g, r in zip(("forces", "energies", "virials"), (f, e, w), r1):
        _close(g[sel], r[sel], tol, "%s after one step: %s" % (what, name))


def test_far_images_on_the_orthorhombic_family_box(emdee, oracle, dev, capfd, monkeypatch):
    """sides 17.1, 20.5, 24.8 with z open, lo = (-3.7, 1.9, 11.3); x and y in far images"""
    E = emdee
    src = mc.family_box(E, "orthorhombic", np.float64)
    box = dict(src, lo=list(OFFSETS), skin=0.3)
    x_in, k = _far(src["pos"], OFFSETS, box["lengths"], box["periodic"], 0x3C01)
    assert (k[:, 2] == 0).all() and np.abs(k[:, :2]).max() == ic.KMAX
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    md = _engine(E, dev, box, x_in, np.float64)
    torch.cuda.synchronize()
    box["plan"](capfd.readouterr().err)
    rows = np.arange(0, x_in.shape[0], 16)                 # (the N^2 table of this box takes seconds: the load's is the cached one)
    ref1 = lambda p: [oref.total(p, (0.0, 0.0, 0.0), box["lengths"], box["periodic"], box["rc"], box["rs"], box["atoms"], rows=rows)[q]
                      for q in "few"]
    _far_case(md, x_in, OFFSETS, box, mc.reference(oracle, src), ref1, TOL64, "orthorhombic", rows=rows)
    md.close()


@pytest.mark.parametrize("chains", [False, True])
@pytest.mark.parametrize("method", ["ewald", "pme"])
def test_far_images_under_ewald_and_pme(emdee, oracle, dev, method, chains):
    """the 300-charge box of three sides and the 256-atom chain box (exclusions, 1-4 pairs, bonded terms: every atom of a chain
    in an image of its own): pme_axis, the struck-pair corrections and the chained minimum images on far inputs"""
    from .helpers import ewald_ref as er
    from .helpers import pme_ref as pr
    E = emdee
    box = mc.ewald_box(E, chains)
    N = box["pos"].shape[0]
    box.update(vel=E.synthetic.velocities(N), lo=[0.0, 0.0, 0.0])
    x_in, k = _far(box["pos"], box["lo"], box["lengths"], box["periodic"], 0x3C02)
    md = _engine(E, dev, box, x_in, np.float64, box["post"])
    md.set_coulomb_(box["q"], 1.0, 5.0, mc.C14)
    if method == "ewald":
        md.set_ewald_(box["alpha"], box["kmax"])
    else:
        md.set_pme_(box["alpha"], box["grid"], 4)
    excl, p14, terms = mc.tables(N, box["post"])
    L = np.array(box["lengths"])

    def ref1(p):
        t = oref.total(p, (0.0, 0.0, 0.0), box["lengths"], box["periodic"], box["rc"], box["rs"], box["atoms"], terms, excl=excl, p14=p14,
                       lj14scale=mc.S14)
        if method == "ewald":
            c = er.ewald(p, L, box["q"], 1.0, box["alpha"], box["kmax"], box["rc"], excl=excl, p14=p14, s14=mc.C14)
        else:
            c = pr.pme(p, L, box["q"], 1.0, box["alpha"], box["grid"], 4, box["rc"], excl=excl, p14=p14, s14=mc.C14)
        return [t[q] + c[i] for i, q in enumerate("few")]

    _far_case(md, x_in, box["lo"], box, mc.ewald_reference(oracle, box, method), ref1, TOL64_CHARGED, "%s %s" % (method, box["key"]))
    md.close()


def test_far_images_of_every_atom_of_a_rigid_molecule(emdee, dev):
    """the water box of tests/test_gpu_settle.py with every ATOM of a molecule in a far image of its own: the constraint stages'
    minimum images; one step and twenty against constrained_verlet, at that module's bound"""
    from .helpers import settle_ref as sr
    from .test_gpu_settle import _against_reference
    from .test_gpu_settle import _engine as water_engine
    B = sr.water_box()
    k = ic.image_counts(B["pos"].shape[0], "uniform", seed=0x3C03)
    far = B["pos"] + k * sr.LENGTHS
    md = water_engine(emdee, dev, dict(B, pos=far))
    _against_reference(md, B["unwrapped"], B["vel"], far - B["unwrapped"], B, (1, 20), 3, "rigid water in far images")
    md.close()


# ---------------------------------------------------------------- 3. faces
TOL = {np.float64: 1e-6, np.float32: 1e-4}                 # tests/test_gpu_masks.py, tests/test_gpu_orthorhombic.py
X32 = 1e-3                                                  # tests/test_gpu_orthorhombic.py: Float32 positions after a run
FACE_BOXES = ["uniform", "species3", "typed", "direct", "ortho", "settle_lj"]
BIG = 2500                                                  # atoms beyond which the yardstick works on sampled rows
_FACE, _ROWS, _RUN = {}, {}, {}


def _sampled(fb, faces):
    """None (every atom) on the small boxes; else the snapped atoms and some 250 others: the yardstick's sampled mode, whole rows"""
    N = fb["pos"].shape[0]
    if N <= BIG:
        return None
    return np.unique(np.concatenate([[f[0] for f in faces], np.arange(0, N, max(1, N // 120))]))


def _face_case(E, oracle, name, dtype):
    """(box with atoms on its faces, faces, yardstick of the whole force field, neighbour rows at rc + skin); the CPU-side
    conditions are asserted here, before any device work.  name + "@0": the box moved to lo = 0 first (a decomposition's box
    starts there), the face set built on the moved box.  The two-species box (97556 atoms): sampled rows throughout."""
    key = (name, dtype)
    if key not in _FACE:
        base = name.split("@")[0]
        box = ic.settle_lj_box(E) if base == "settle_lj" else _box(E, base, dtype)
        if base == "typed":
            box = ic.sheared_box(box, 0.6)               # (so that atoms lie within 0.15 sigma of every cell face)
        if name.endswith("@0"):
            box = dict(box, pos=box["pos"] - np.asarray(box["lo"]), lo=[0.0, 0.0, 0.0], key=box["key"] + "@0")
        fb, faces = ic.with_face_atoms(box, dtype)
        ic.assert_face_conditions(fb, faces, box["scale"], excl=box.get("excl"))
        rows = _sampled(fb, faces) if base == "typed" else None
        fb["rows"] = rows
        _FACE[key] = (fb, faces, _yardstick(oracle, fb, fb["pos"], rows), _yard_rows(fb, fb["pos"], rows))
    return _FACE[key]


def _yardstick(oracle, box, pos, rows=None):
    L = box["lengths"]
    w = oref.wrapped(pos, box["lo"], L, box["periodic"])
    cubic = list(box["lo"]) == [0.0] * 3 and L[0] == L[1] == L[2]
    return oref.total(w, box["lo"], L, box["periodic"], box["rc"], box["rs"], box["atoms"], excl=box.get("excl"), rows=rows,
                      oracle=oracle if (cubic and rows is None) else None)


def _yard_rows(box, pos, rows=None):
    """directed pair keys i N + j (must, may, rows): every (non-excluded) pair closer than rc + skin less the band 2 BAND
    (relative, in r^2), and every pair closer than rc + skin plus the band; of every atom, or of the sampled rows.  For an atom
    on a face the two are the same set (image_cases.with_face_atoms); the families on the jittered fcc box share their
    positions and so their pairs."""
    from .helpers import virial_tensor_ref as vt
    w = oref.wrapped(pos, box["lo"], box["lengths"], box["periodic"])
    key = (w.tobytes(), box["rc"] + box["skin"], None if rows is None else rows.tobytes())
    if key not in _ROWS:
        N = w.shape[0]
        i, j, d = vt.pairs_in_range(w, box["lengths"], box["periodic"], box["rc"] + box["skin"], rows=rows, margin=0.01)
        r2 = np.einsum("ij,ij->i", d, d)
        if box.get("excl") is not None:
            e = np.asarray(box["excl"])
            r2[np.isin(vt._pair_key(i, j, N), vt._pair_key(e[:, 0], e[:, 1], N))] = np.inf
        if rows is None:
            i, j, r2 = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([r2, r2])
        keys = i.astype(np.int64) * N + j
        rl2 = (box["rc"] + box["skin"]) ** 2
        _ROWS[key] = (keys[r2 < rl2 * (1 - 2 * ic.BAND)], keys[r2 < rl2 * (1 + 2 * ic.BAND)], rows)
    return _ROWS[key]


def _check_rows(md, want, what):
    """every pair of `must` is in its row, once; nothing outside `may` is; no row is empty that the yardstick fills"""
    must, may, sample = want
    counts, rows = _rows(md)
    N = counts.shape[0]
    ii, jj = np.repeat(np.arange(N), counts), rows[rows < N]
    assert jj.shape == ii.shape
    if sample is not None:
        keep = np.isin(ii, sample)
        ii, jj = ii[keep], jj[keep]
    got = ii.astype(np.int64) * N + jj
    assert len(np.unique(got)) == len(got), "%s: a pair is listed twice in a row" % what
    missing = must[~np.isin(must, got)]
    assert len(missing) == 0, "%s: %d pairs inside rc + skin are not listed, first (%d, %d)" % (what, len(missing), missing[0] // N, missing[0] % N)
    assert np.isin(got, may).all(), "%s: a pair beyond rc + skin is listed" % what
    filled = np.bincount(must // N, minlength=N) > 0
    assert (counts[filled] > 0).all(), "%s: a row is empty that the yardstick fills" % what


def _check_outputs(got, want, tol, what, rows=None):
    """rows: the sampled atoms only (the yardstick filled no other row; the box sums then have no yardstick)"""
    sel = slice(None) if rows is None else rows
    for name, g, key in (("forces", got[0], "f"), ("energies", got[1], "e"), ("virials", got[2], "w"), ("tensors", got[3], "t")):
        _close(g[sel], want[key][sel], tol, "%s: %s" % (what, name))
    if rows is None:
        assert np.abs(got[4] - want["t"].sum(axis=0)).max() <= tol * np.abs(want["t"]).sum(axis=0).max(), what


def _same_place(x, x_in, dtype, what, box):
    """positions handed back against the ones given.  Float64 records are the wrapped coordinate itself: one rounding of record +
    count x len, one unit in the last place of the coordinate.  A Float32 engine may keep its records relative to the atom's
    cell (kernels.hpp RelGrid), rounded at the size of a cell, not of the coordinate: one unit in the last place of the larger."""
    size = np.abs(x_in)
    if dtype == np.float32:
        size = np.maximum(size, np.asarray(box["lengths"]) / np.asarray(ic.cells_per_side(box)))
    ulp = np.spacing(size.astype(dtype)).astype(np.float64)
    assert (np.abs(x.astype(np.float64) - x_in) <= ulp).all(), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FACE_BOXES)
def test_atoms_on_box_faces_and_cell_faces_at_the_load_and_through_a_rebuild(emdee, oracle, dev, capfd, monkeypatch, name, dtype):
    """Per axis one atom exactly on lo, on lo + len, on every cell face, and on the neighbours of each of those numbers in the
    engine's type.  The rows, every output, and the positions handed back -- at the load (k_gather_user) and again behind an
    emdee_md_rebuild with the atoms still there (k_gather_sorted: the binning of the rounded position against the wrap in
    double, the case of that kernel's comment on the Float32 cell-relative records).  Then the same atoms given as their
    other images: bit for bit where the other image is a number of the engine's type, else against the yardstick.

    The (8, 16, 32) box is exact and still not bit for bit (found by this test: forces differ by 7e-15 / 4e-6 of 150).  Its lo is
    not 0 and its cell faces lo + c len / M are not on the 2^-13 grid: voxel() forms (p - lo) / len, and p - lo rounds
    differently for p and for p + len, so an atom within a unit in the last place of a cell face may be binned on either side
    of it.  The record is the same number in both engines; the cell, hence the order of the sums, is not.  That box is
    therefore held to the yardstick and to the rows as sets, as the non-dyadic box is; on the cubic boxes (lo = 0, len a power
    of two) the quotient is exact and the bits agree."""
    E = emdee
    fb, faces, want, rows = _face_case(E, oracle, name, dtype)
    dyadic = name != "settle_lj"
    bitwise = dyadic and name != "ortho"
    sample = fb["rows"]
    for k, v in fb["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    md = _engine(E, dev, fb, fb["pos"], dtype)
    torch.cuda.synchronize()
    fb["plan"](capfd.readouterr().err)
    for stage in ("at the load", "behind a rebuild"):
        what = "%s %s" % (name, stage)
        _check_outputs(_outputs(md), want, TOL[dtype], what, sample)
        _check_rows(md, rows, what)
        _same_place(_positions(md), fb["pos"], dtype, what, fb)
        md.rebuild_()
    out, listed = _outputs(md), _rows(md)
    md.close()
    pos2, n = ic.other_images(fb, faces, dtype, exact=dyadic)
    assert n >= (6 if dyadic else len(faces)), n
    assert np.abs(oref.image_difference(pos2, fb["pos"], fb["lengths"], fb["periodic"])).max() <= (0 if dyadic else np.spacing(dtype(16.0)))
    md = _engine(E, dev, fb, pos2, dtype)
    if bitwise:
        _same_bits(_outputs(md), out, name + ": the other images")
        _same_rows(_rows(md), listed, name + ": the other images")
    else:
        _check_outputs(_outputs(md), _yardstick(oracle, fb, pos2, sample), TOL[dtype], name + ": the other images", sample)
        _check_rows(md, rows, name + ": the other images")
    _same_place(_positions(md), pos2, dtype, name + ": the other images", fb)
    md.close()


def _yard_run(oracle, fb, faces, dt, dtype, distance):
    """(crossing velocities, x, v of the yardstick after 20 steps), once per box and precision: the families on the jittered fcc
    box with one species share it.  Cubic boxes take their candidate pairs from the oracle's cell list."""
    vel = ic.crossing_velocities(fb, faces, dt, dtype, distance=distance)
    key = (fb["pos"].tobytes(), np.asarray(fb["atoms"]).tobytes(), vel.tobytes(), dt)
    if key not in _RUN:
        lo, L, per = np.asarray(fb["lo"]), np.asarray(fb["lengths"]), fb["periodic"]
        cubic = list(fb["lo"]) == [0.0] * 3 and L[0] == L[1] == L[2]
        force = lambda x: oref.total(oref.wrapped(x, lo, L, per), lo, L, per, fb["rc"], fb["rs"], fb["atoms"], excl=fb.get("excl"),
                                     oracle=oracle if cubic else None)["f"]
        xr, vr = oref.verlet(fb["pos"], vel, force, 20, dt)
        ic.assert_crossed(fb, faces, xr)
        _RUN[key] = (vel, xr, vr)
    return _RUN[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["uniform", "species3", "direct", "ortho", "settle_lj"])
def test_face_atoms_cross_their_faces_both_ways_within_a_run(emdee, oracle, dev, capfd, monkeypatch, name, dtype):
    """20 steps; the atom just below a face flies up through it, the one just above down, the one on it up (0.3 sigma in the
    run on the dense family boxes, where a neighbour at 0.8 sigma pushes an atom back by 0.1 sigma; 0.1 sigma on the 320-atom box).  CPU-side, from the yardstick's trajectory: every face is crossed each way.  The trajectory against oref.verlet at the
    bounds of tests/test_gpu_orthorhombic.py's _run_case; then, behind a rebuild, every pair closer than rc + skin less the band
    is listed, none beyond it plus the band (4000 atoms: on sampled rows), and the outputs match the yardstick at the engine's
    own positions.  The 320-atom box also runs on its axes cycled, as _run_case does.  The two-species box of 97556 atoms has
    no run: twenty-one evaluations of its yardstick take a minute and more."""
    E = emdee
    fb, faces, _, _ = _face_case(E, oracle, name, dtype)
    dt = 0.002                                              # (tests/test_gpu_settle.py's step: the push of a close neighbour stays below the crossing)
    vel, xr, vr = _yard_run(oracle, fb, faces, dt, dtype, 0.1 if name == "settle_lj" else 0.3)
    L, per = np.asarray(fb["lengths"]), fb["periodic"]
    for k, v in fb["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    bound = X64 if dtype == np.float64 else X32
    finals = []
    for k in ((0, 1, 2) if name == "settle_lj" else (0,)):  # the axes cycled k times
        cyc = lambda a: np.ascontiguousarray(oref.cycle(a, k))
        cb = dict(fb, lo=list(cyc(fb["lo"])), lengths=list(cyc(fb["lengths"])), periodic=list(cyc(fb["periodic"])))
        capfd.readouterr()
        md = _engine(E, dev, cb, cyc(fb["pos"]), dtype, vel=cyc(vel))
        torch.cuda.synchronize()
        fb["plan"](capfd.readouterr().err)
        md.step_(20, dt)
        st = md.state()
        x, v = (oref.cycle(st[q].cpu().numpy().astype(np.float64), (3 - k) % 3) for q in ("positions", "velocities"))
        dx = np.abs(oref.image_difference(x, xr, L, per)).max()
        assert np.abs(np.rint((x - xr) / L)).max() == 0, "an atom came back in another image"
        print("%s cycle %d: max |dx| %.3e, max |dv| %.3e, %d builds" % (name, k, dx, np.abs(v - vr).max(), md.nbr_stats()["builds"]))
        assert dx < bound and np.abs(v - vr).max() < 10 * bound
        finals.append(x)
        if k == 0:
            md.rebuild_()
            sample = _sampled(fb, faces)
            _check_outputs(_outputs(md), _yardstick(oracle, fb, x, sample), TOL[dtype], name + " after the run", sample)
            _check_rows(md, _yard_rows(fb, x, sample), name + " behind the last rebuild")
        md.close()
    for x in finals[1:]:
        assert np.abs(oref.image_difference(x, finals[0], L, per)).max() < 2 * bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["uniform", "species3", "typed", "direct"])
def test_face_atoms_through_the_operator_path(emdee, oracle, dev, capfd, monkeypatch, name, dtype):
    """the face sets of the cubic boxes through emdee_compute_nonbonded and emdee_compute_virial_tensor (tiled, two species, and
    direct under EMDEE_PATH), and again as their other images with the list kept (k_refresh_check).  The operator takes one box
    length and lo = 0 (the reference's only geometry): the (8, 16, 32) box and the non-dyadic box cannot go through it."""
    E = emdee
    fb, faces, want, _ = _face_case(E, oracle, name, dtype)
    N = fb["pos"].shape[0]
    for k, v in fb["env"].items():
        monkeypatch.setenv(k, v)
    if name == "typed" and dtype == np.float32:
        monkeypatch.setenv("EMDEE_F32_FAST", "1")            # (as tests/test_gpu_masks.py)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    tiles = E.nonbonded_computation_tiles(N, skin=fb["skin"])
    got = _operator(E, dev, fb, tiles, fb["pos"], dtype)
    torch.cuda.synchronize()
    fb["plan"](capfd.readouterr().err)
    sel = slice(None) if fb["rows"] is None else fb["rows"]
    for nm, g, key in zip(("forces", "energies", "virials", "tensors"), got, "fewt"):
        _close(g[sel], want[key][sel], TOL[dtype], "%s operator: %s" % (name, nm))
    builds = tiles.stats()["builds"]
    pos2, n = ic.other_images(fb, faces, dtype, exact=True)
    assert n >= 6
    again = _operator(E, dev, fb, tiles, pos2, dtype)
    for nm, g, key in zip(("forces", "energies", "virials", "tensors"), again, "fewt"):         # (the same atoms: the same yardstick)
        _close(g[sel], want[key][sel], TOL[dtype], "%s operator, other images: %s" % (name, nm))
    assert tiles.stats()["builds"] == builds, "atoms given as their other images made the list rebuild"
    tiles.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["uniform", "species3", "typed", "ortho@0", "settle_lj@0"])
def test_face_atoms_in_eight_domains(emdee, oracle, dev, name, dtype):
    """2 x 2 x 2 domains: with an even number of cells per side (all but the two-species box, 13, and x of the (8, 16, 32) box, 3)
    the brick faces at len / 2 are cell faces and carry atoms.  A decomposition's box starts at 0: the (8, 16, 32) box and the non-dyadic box are moved there
    and their face sets built anew.  The yardstick's forces, every atom owned exactly once, positions handed back wrapped."""
    E = emdee
    fb, faces, want, _ = _face_case(E, oracle, name, dtype)
    N = fb["pos"].shape[0]
    dd = _decomposed(E, dev, fb, fb["pos"], 8, dtype)
    x, v, f, owner = _gathered(dd, 8, N, dtype)
    assert sum(dd.counts(r)["n_owned"] for r in range(8)) == N
    sel = slice(None) if fb["rows"] is None else fb["rows"]
    _close(f[sel], want["f"][sel], TOL[dtype], name + " in eight domains: forces")
    assert np.abs(oref.image_difference(x, fb["pos"], fb["lengths"], fb["periodic"])).max() <= np.spacing(dtype(max(fb["lengths"])))
    dd.close()


# ---------------------------------------------------------------- 4. the bound on the image counts
def _refused(call, code, *words):
    with pytest.raises(RuntimeError) as info:
        call()
    assert getattr(info.value, "code", None) == code, info.value
    for w in words:
        assert w in str(info.value), (w, str(info.value))


@pytest.mark.parametrize("records", ["absolute", "cell_relative"])
def test_a_load_beyond_the_count_field_is_refused_and_a_valid_one_follows(emdee, dev, records):
    """absolute: the Float64 engine; cell_relative: the Float32 engine on the brick kernels (csrc/nbsys.hpp rel_wanted)"""
    E = emdee
    dtype = np.float64 if records == "absolute" else np.float32
    box = _box(E, "uniform", dtype)
    N, L = box["pos"].shape[0], box["lengths"][0]
    md = _engine(E, dev, box, box["pos"], dtype)
    want = _outputs(md)
    xd = lambda p: E.cu(p.astype(dtype), dev)
    vd, ad = E.cu(box["vel"].astype(dtype), dev), E.cu(box["atoms"], dev)
    atom = 1234
    for axis in range(3):
        for count in (600, -600):
            pos = box["pos"].copy()
            pos[atom, axis] += count * L
            assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos)
            _refused(lambda: md.set_state_(xd(pos), vd, ad), ERR_INVALID, "atom %d " % atom, "axis %d" % axis, "%d box lengths" % count)
            _refused(lambda: md.step_(1, ic.DT), ERR_STATE)            # (no state, as before the first load)
            _refused(lambda: md.state(), ERR_STATE)
    # ... and the field's own ends are accepted where the header promises it
    k = np.zeros((N, 3), dtype=np.int64)
    k[atom] = (500, -500, 500)
    md.set_state_(xd(ic.shifted(box, k)), vd, ad)
    _same_bits(_outputs(md), want, "the valid load behind the refusals")
    assert np.array_equal(_positions(md).astype(np.float64), ic.shifted(box, k))
    md.step_(2, ic.DT)
    md.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_ballistic_atom_is_exact_up_to_the_bound_and_then_reported(emdee, dev, dtype):
    """Two atoms further apart than rc + skin in a box of side 16: atom 1 flies 0.75 box lengths per step along one axis (every
    factor dyadic: x0 + n dt v is exact in either precision), rebuild_every = 1.  Its count reaches 300 after 400 steps and
    passes 511 in step 682; atom 0 drifts slowly and stays exact throughout."""
    E = emdee
    L, dt = 16.0, 0.0625
    for axis in range(3):
        pos = np.array([[1.0, 1.0, 1.0], [9.0, 9.0, 9.0]])
        vel = np.zeros((2, 3))
        vel[1, axis] = (0.75 * L if axis != 1 else -0.75 * L) / dt
        vel[0, (axis + 1) % 3] = 2.0 ** -6
        md = E.VelocityVerlet(E.cu(pos.astype(dtype), dev), E.cu(vel.astype(dtype), dev), L, E.LennardJonesModel(2.5, 2.0),
                              E.cu(E.lennard_jones_atoms(1.0, 1.0, 2), dev), skin=0.3)
        md.step_(400, dt, 1)
        want = pos + 400 * dt * vel
        assert abs(want[1, axis]) > 290 * L
        assert np.array_equal(_positions(md).astype(np.float64), want), "after 400 steps"
        done = 400
        with pytest.raises(RuntimeError) as info:
            while done < 800:
                md.step_(50, dt, 1)
                done += 50
                assert np.array_equal(_positions(md).astype(np.float64), pos + done * dt * vel), "after %d steps" % done
        assert getattr(info.value, "code", None) == ERR_STATE and "atom 1 " in str(info.value), info.value
        assert "axis %d" % axis in str(info.value), info.value
        assert done == 650, "the count passes the field between steps 650 and 700, not after %d" % done
        _refused(lambda: md.step_(1, dt, 1), ERR_STATE)
        x = _positions(md).astype(np.float64)
        steps = (x[0, (axis + 1) % 3] - 1.0) / (dt * 2.0 ** -6)
        assert steps == np.rint(steps) and 650 < steps <= 700, steps
        assert np.array_equal(x[0], pos[0] + steps * dt * vel[0]), "the other atom's position"
        # a new state lifts the refusal
        md.set_state_(E.cu(pos.astype(dtype), dev), E.cu(vel.astype(dtype), dev), E.cu(E.lennard_jones_atoms(1.0, 1.0, 2), dev))
        md.step_(4, dt, 1)
        assert np.array_equal(_positions(md).astype(np.float64), pos + 4 * dt * vel)
        md.close()
