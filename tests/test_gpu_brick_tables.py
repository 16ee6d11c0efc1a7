"""GPU test of the brick tables (csrc/brick.hpp: BrickTables, brick_setup, k_brick_tables, k_brick_export with NT = 1 and
NT = 2): the rows emdee_md_nbr_list exports are the brute-force set r < rc + skin of every owned atom, on boxes whose cell
counts end in a partial brick along every dimension.

Cases: species count (one, two) x brick shape x engine (undivided periodic, two domains in one process).  Bricks of
2 x 2 x 2 cells exist for two-species boxes with long rows only (plan.hpp choose_plan: variant 9 where the one-species plan
would take variant 8), so "one species, 2 x 2 x 2" is no path of the library and has no case; 4 x 2 x 2 with two species
needs EMDEE_TYPED_ALL.  The EMDEE_DEBUG_PLAN lines say which kernels ran.

Float64: the set has one answer (no pair within 1e-9 of rc + skin, asserted here on the CPU) and every row must equal it.
Undivided engines report caller ids, compared as arrays.  A domain reports its own numbering (owned atoms, then ghosts, whose
global ids it does not hand out): there a row is the set when its entries are distinct, all inside rc + skin of the atom, and
as many as the undivided box holds -- the argument of test_gpu_dd.py::_row_sample_check, here for every owned atom.
Float32 (undivided engines): the rule test_gpu_parity2.py::test_two_species_boxes_take_the_typed_kernels applies to typed
rows against a second build, with the brute-force set of the rounded positions as the second witness: at most 2 x 4 rows
differ, none by more than two entries.

Related: test_gpu_dd.py::test_dd_neighbour_rows_are_complete counts the listed entries of cubic boxes in 2, 3 and 8
domains; test_gpu_orthorhombic.py checks one-species rows on orthorhombic boxes with ragged last bricks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SKIN = 0.3
SIDE = 1.013                 # cell side in units of rc + skin: just above it
# cells: cell counts of the box -- 9 x 5 x 5 undivided (4 x 2 x 2 and 2 x 2 x 2 bricks both end ragged along every axis), 10 x 5 x 5
# cut in two along x (5 own cells + a ghost layer on either side = 7 per domain).  fcc: lattice cells of the jittered fcc the box
# is filled with, stretched to the box (rho* = 0.71 .. 0.75): at rc = 3.5 a 4 x 2 x 2 tile then outgrows half a CU's LDS, which
# is what sends a two-species box to the 2 x 2 x 2 bricks, and a 2 x 2 x 2 tile still fits their planes.
CASES = {
    "one-4x2x2": dict(rc=2.5, rs=2.0, fcc={9: 15, 10: 16, 5: 8}, species=1, env={}, variant=0, bricks="3 x 3 x 3"),
    "two-4x2x2": dict(rc=2.5, rs=2.0, fcc={9: 15, 10: 16, 5: 8}, species=2, env={"EMDEE_TYPED_ALL": "1"}, variant=0, bricks="3 x 3 x 3"),
    "two-2x2x2": dict(rc=3.5, rs=3.0, fcc={9: 19, 10: 21, 5: 11}, species=2, env={}, variant=9, bricks="5 x 3 x 3"),
}
_BOX = {}


def _brute_rows(pos, lengths, rlist):
    """rows of the set r < rlist in the periodic box (sorted ids), and the smallest | r - rlist | over all pairs"""
    N = pos.shape[0]
    rows, gap = [], np.inf
    for a in range(0, N, 256):
        d = pos[a:a + 256, None, :] - pos[None, :, :]
        d -= lengths * np.rint(d / lengths)
        r = np.sqrt(np.einsum("ijk,ijk->ij", d, d))
        r[np.arange(r.shape[0]), a + np.arange(r.shape[0])] = np.inf
        gap = min(gap, np.abs(r - rlist).min())
        rows.extend(np.nonzero(row < rlist)[0] for row in r)
    return rows, gap


def _box(E, key, dtype, cells=(9, 5, 5)):
    """positions (as the engine's precision holds them), box, atoms and the brute-force rows: once per case, precision and box"""
    if (key, dtype, cells) not in _BOX:
        c = CASES[key]
        syn = E.synthetic
        rlist = c["rc"] + SKIN
        lengths = np.array(cells, dtype=np.float64) * SIDE * rlist
        fcc = tuple(c["fcc"][m] for m in cells)
        pos, gid, lat = syn.fcc_block(fcc, (0, 0, 0), fcc)
        pos = pos[np.argsort(gid)] * (lengths / np.asarray(lat, dtype=np.float64))
        pos = pos + 0.25 * (np.random.default_rng(11).random(pos.shape) - 0.5)
        pos = (pos - lengths * np.floor(pos / lengths)).astype(dtype)
        N = pos.shape[0]
        eps, sigma = (np.ones(N), np.ones(N)) if c["species"] == 1 else syn.mixture_parameters(syn.mixture_types(N))
        rows, gap = _brute_rows(pos.astype(np.float64), lengths, rlist)
        print("%s %s %s: %d atoms, nearest pair to rc + skin %.2e" % (key, np.dtype(dtype).name, cells, N, gap))
        if dtype == np.float64:
            assert gap > 1e-9, "a pair within %.1e of rc + skin: the Float64 set must have one answer" % gap
        _BOX[(key, dtype, cells)] = dict(pos=pos, lengths=lengths, atoms=E.lennard_jones_atoms(eps, sigma), vel=syn.velocities(N), rows=rows, N=N)
    return _BOX[(key, dtype, cells)]


def _check_plan(err, c, undivided):
    """the planner prints one `bricks` line per variant it sizes, the chosen one last, and one `two species` line per typed
    candidate: every engine (one, or one per domain) must have ended on the case's variant and kernels"""
    lines = [l.rstrip() for l in err.splitlines() if l.startswith("emdee plan:")]
    engines = 1 if undivided else 2
    bricks = [l for l in lines if l.startswith("emdee plan: bricks")]
    typed = [l for l in lines if "two species" in l]
    if undivided:
        assert bricks and bricks[-1].endswith("variant %d" % c["variant"]) and ("bricks %s," % c["bricks"]) in bricks[-1], lines
    else:
        assert sum(l.endswith("variant %d" % c["variant"]) for l in bricks) >= engines, lines
    if c["species"] == 2:
        mine = [l for l in typed if ("variant %d:" % c["variant"]) in l]
        assert len(mine) >= engines and all(l.endswith("typed kernels on") for l in mine), lines
    else:
        assert not typed, lines


def _setenv(monkeypatch, c):
    for k in ("EMDEE_TYPED_ALL", "EMDEE_NO_TYPED", "EMDEE_TYPED_BRICKS", "EMDEE_TYPED_SUBBINS", "EMDEE_NO_SUBBINS", "EMDEE_PATH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("key", list(CASES))
def test_exported_rows_are_the_brute_force_set(emdee, capfd, monkeypatch, key, dtype):
    E, c, dev = emdee, CASES[key], torch.device("cuda", 0)
    B = _box(E, key, dtype)
    _setenv(monkeypatch, c)
    capfd.readouterr()
    md = E.VelocityVerlet(E.cu(B["pos"], dev), E.cu(B["vel"].astype(dtype), dev), float(B["lengths"][0]), E.LennardJonesModel(c["rc"], c["rs"]),
                          E.cu(B["atoms"], dev), skin=SKIN, lengths=list(B["lengths"]), periodic=[1, 1, 1])
    counts, nb = md.neighbor_lists()
    torch.cuda.synchronize()
    _check_plan(capfd.readouterr().err, c, True)
    counts, nb = counts.cpu().numpy(), nb.cpu().numpy()
    md.close()
    assert counts.shape[0] == B["N"]
    differing = 0
    for i in range(B["N"]):
        got = np.sort(nb[i, :counts[i]])                                   # (no unique: an entry listed twice shows)
        if np.array_equal(got, B["rows"][i]):
            continue
        assert dtype == np.float32, "row %d differs from the brute-force set (%d listed, %d wanted)" % (i, len(got), len(B["rows"][i]))
        differing += 1
        assert differing <= 2 * 4, "row %d: more than 8 rows differ from the brute-force set" % i
        assert len(np.setxor1d(got, B["rows"][i])) <= 2, "row %d differs by more than two entries" % i


@pytest.mark.parametrize("key", list(CASES))
def test_rows_of_two_domains_are_the_brute_force_set(emdee, capfd, monkeypatch, key):
    E, c, dev = emdee, CASES[key], torch.device("cuda", 0)
    B = _box(E, key, np.float64, (10, 5, 5))
    _setenv(monkeypatch, c)
    capfd.readouterr()
    world, N, lengths, rlist = 2, B["N"], B["lengths"], c["rc"] + SKIN
    dd = E.DomainDecomposition(list(lengths), E.domain.rank_grid(world), E.LennardJonesModel(c["rc"], c["rs"]), skin=SKIN, dtype=torch.float64, device=dev)
    for r in range(world):
        mine = np.arange(r, N, world)
        dd.set_atoms_(r, E.cu(B["pos"][mine], dev), E.cu(B["vel"][mine], dev), E.cu(B["atoms"][mine], dev), torch.from_numpy(mine.astype(np.int64)).to(dev))
    dd.load_()
    torch.cuda.synchronize()
    _check_plan(capfd.readouterr().err, c, False)
    want = np.array([len(r) for r in B["rows"]])
    Lt = torch.from_numpy(lengths).to(dev)
    owned = 0
    for r in range(world):
        eng = dd.engine(r)
        gid = dd.state(r)[0].cpu().numpy()
        assert dd.counts(r)["n_ghost"] > 0
        x = eng.state(velocities=False, forces=False)["positions"]        # owned atoms first, then the ghosts
        counts, nb = eng.neighbor_lists()
        assert counts.shape[0] == gid.shape[0]
        assert np.array_equal(counts.cpu().numpy(), want[gid]), "domain %d: %d rows differ in length from the brute-force set" % (
            r, int((counts.cpu().numpy() != want[gid]).sum()))
        cl, rows = counts.long(), nb.long()
        valid = torch.arange(rows.shape[1], device=dev)[None, :] < cl[:, None]
        d = x[rows.clamp(min=0)] - x[:gid.shape[0], None, :]
        d = d - Lt * torch.round(d / Lt)                                    # (a ghost is reported in the image it is used in)
        assert bool(((d * d).sum(dim=2)[valid] < rlist * rlist).all()), "domain %d: an entry outside rc + skin" % r
        srt = torch.where(valid, rows, torch.full_like(rows, -1)).sort(dim=1).values
        assert not bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()), "domain %d: an entry listed twice" % r
        owned += gid.shape[0]
    assert owned == N
    dd.close()
