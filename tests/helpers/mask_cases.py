"""Boxes and fp64 host references of tests/test_gpu_masks.py: one box per kernel family the planner selects, with the tables and
charges the test puts on it, and the reference of the whole force field on it -- computed once per (box, tables, charges) and
kept for the module's life.  The builders are those of the other GPU modules (tests/test_gpu_virial_tensor.py _family_box,
tests/test_gpu_bonded.py _chains -- whose exclusions and 1-4 pairs are _molecules' -- and tests/test_gpu_dd_pairs.py
_global_box); the references are ortho_ref (pair terms,
reaction field and bonded terms), ewald_ref, pme_ref, and the oracle where the box is too large for numpy's pair table.

Positions are rounded to Float32 once, so that both precisions of a family (and their one reference) see the same box."""
import numpy as np

from . import ewald_ref as er
from . import ortho_ref as orf
from . import pme_ref as pr

# (typed_all: the two-species kernels on the default brick variant, EMDEE_TYPED_ALL=1 -- the one place where a typed launch is
# instantiated for the masks 2 .. 6 themselves; the short-row box of tests/test_gpu_parity2.py)
FAMILIES = ["uniform", "species3", "long_rows", "typed", "typed_all", "direct"]
S14, C14 = 0.5, 0.8333                                     # LJ and Coulomb factors of the 1-4 pairs
LONG_ROWS = {np.float64: (3.0, 2.5), np.float32: (3.2, 2.7)}   # (rc, rs) of tests/test_gpu_coulomb.py's long-row cases
CHAIN_CHARGES = [0.6, -0.3, -0.5, 0.2]                     # per chain of four: neutral molecules


def _f32(pos):
    return np.asarray(pos, dtype=np.float64).astype(np.float32).astype(np.float64)


def family_box(E, family, dtype=np.float64):
    """dict(key, pos, vel, lengths, periodic, atoms, rc, rs, env, plan): plan(err) asserts from the EMDEE_DEBUG_PLAN text that
    the family's kernels are the ones in use."""
    from ..test_gpu_dd_pairs import _global_box
    from ..test_gpu_virial_tensor import _family_box

    def last_bricks_line(err):
        lines = [l for l in err.splitlines() if l.startswith("emdee plan: bricks")]
        assert lines, "the brick kernels must be in use: " + err[-600:]
        assert "direct kernels" not in err, err[-600:]
        return lines[-1]

    if family == "long_rows":
        pos, _, eps, sigma, L = _global_box(E.synthetic, uniform=True, ncell=10)
        rc, rs = LONG_ROWS[dtype]
        box = dict(key="long_rows%d" % (64 if dtype == np.float64 else 32), lengths=[L] * 3, periodic=[1, 1, 1],
                   atoms=E.lennard_jones_atoms(eps, sigma), rc=rc, rs=rs, env={})

        def plan(err):
            line = last_bricks_line(err)
            assert line.rstrip().endswith("variant 8"), line
            assert "two species" not in err
    elif family == "typed_all":
        pos, L = E.synthetic.fcc_positions(23)
        pos = pos + 0.25 * (np.random.default_rng(7).random(pos.shape) - 0.5)
        eps, sigma = E.synthetic.mixture_parameters(E.synthetic.mixture_types(pos.shape[0]))
        box = dict(key="typed_all", lengths=[L] * 3, periodic=[1, 1, 1], atoms=E.lennard_jones_atoms(eps, sigma), rc=2.5, rs=2.0,
                   env={"EMDEE_TYPED_ALL": "1"})

        def plan(err):
            on = [l for l in err.splitlines() if "typed kernels on" in l]
            assert on and "two species, variant 0:" in on[-1], err[-600:]
            assert "typed kernels off" not in err, err[-600:]
    else:
        pos, lengths, periodic, atoms, (rc, rs), env, want, forbid = _family_box(E, family)
        box = dict(key="uniform" if family == "direct" else family, lengths=list(lengths), periodic=list(periodic), atoms=atoms,
                   rc=rc, rs=rs, env=env)

        def plan(err):
            if want is not None:
                assert want in err, err[-600:]
            if forbid is not None:
                assert forbid not in err, err[-600:]
            if family in ("uniform", "species3", "orthorhombic"):
                assert last_bricks_line(err).rstrip().endswith("variant 0"), err[-600:]
            if family == "typed":
                assert "typed kernels off" not in err, err[-600:]
    box["pos"] = _f32(pos)
    if family == "orthorhombic":
        assert (box["pos"][:, 2] > 0).all() and (box["pos"][:, 2] < box["lengths"][2]).all()
    box["vel"] = E.synthetic.velocities(pos.shape[0])
    box["plan"] = plan
    return box


def tables(N, post):
    """post: "none", "tables" (exclusions + scaled 1-4 pairs of the four-atom molecules) or "bonded" (those + the chains'
    bonds, angles and torsions) -> (excl, p14, terms)"""
    from ..test_gpu_bonded import _chains
    if post == "none":
        return None, None, None
    terms, excl, p14 = _chains(N)
    return excl, p14, (terms if post == "bonded" else None)


_REF = {}


def reference(oracle, box, post="none", charges=None, eps_rf=np.inf):
    """(f, e, w) of the whole force field on the box in fp64: switched LJ less the excluded pairs, 1-4 pairs S14 times, the
    bonded terms, and with charges the reaction field (K = 1, 1-4 pairs C14 times).  The caller gets the cached arrays: do not
    write to them."""
    key = (box["key"], post, None if charges is None else (charges.tobytes(), float(eps_rf)))
    if key not in _REF:
        pos, L = box["pos"], box["lengths"]
        excl, p14, terms = tables(pos.shape[0], post)
        if box["key"].startswith("typed"):
            assert post == "none" and charges is None
            _REF[key] = oracle.nonbonded_cells(np.mod(pos, L[0]), L[0], oracle.model(box["rc"], box["rs"]), box["atoms"])
        else:
            cubic = box["periodic"] == [1, 1, 1] and L[0] == L[1] == L[2]
            t = orf.total(pos, (0.0, 0.0, 0.0), L, box["periodic"], box["rc"], box["rs"], box["atoms"], terms, excl=excl, p14=p14,
                          lj14scale=S14, charges=charges, coulomb_k=1.0, eps_rf=eps_rf, coulomb14scale=C14,
                          oracle=oracle if cubic else None)
            _REF[key] = (t["f"], t["e"], t["w"])
    return _REF[key]


def ewald_box(E, chains):
    """the charged boxes of tests/test_gpu_ewald.py and tests/test_gpu_pme.py: 300 random charges with LJ in a box of three
    different sides, or (chains) the 256-atom chain box with its exclusions, 1-4 pairs and bonded terms.
    -> dict(key, pos, lengths, atoms, rc, rs, skin, q, post, alpha, kmax, grid)"""
    from ..test_gpu_bonded import _box
    from ..test_gpu_ewald import ALPHA, KMAX, RC_BOX, RS_BOX, SKIN_BOX, _lj_box
    from ..test_gpu_pme import GRID
    if chains:
        pos, _, eps, sigma, L = _box(E, ncell=4)
        return dict(key="chains256", pos=_f32(pos), lengths=[L] * 3, periodic=[1, 1, 1], atoms=E.lennard_jones_atoms(eps, sigma), rc=2.5,
                    rs=2.0, skin=0.3, q=np.tile(CHAIN_CHARGES, pos.shape[0] // 4), post="bonded", alpha=1.4, kmax=9, grid=(16, 8, 32))
    pos, L, q, eps, sigma = _lj_box()
    return dict(key="charges300", pos=_f32(pos), lengths=[float(v) for v in L], periodic=[1, 1, 1], atoms=E.lennard_jones_atoms(eps, sigma),
                rc=RC_BOX, rs=RS_BOX, skin=SKIN_BOX, q=q, post="none", alpha=ALPHA, kmax=KMAX, grid=GRID)


def ewald_reference(oracle, box, method):
    """(f, e, w): the uncharged reference of the box plus ewald_ref's (method "ewald") or pme_ref's (method "pme", order 4) sum"""
    key = (box["key"], method)
    if key not in _REF:
        lj = reference(oracle, box, box["post"])
        excl, p14, _ = tables(box["pos"].shape[0], box["post"])
        L = np.array(box["lengths"])
        if method == "ewald":
            c = er.ewald(box["pos"], L, box["q"], 1.0, box["alpha"], box["kmax"], box["rc"], excl=excl, p14=p14, s14=C14)
        else:
            c = pr.pme(box["pos"], L, box["q"], 1.0, box["alpha"], box["grid"], 4, box["rc"], excl=excl, p14=p14, s14=C14)
        _REF[key] = tuple(a + b for a, b in zip(lj, c[:3]))
    return _REF[key]
