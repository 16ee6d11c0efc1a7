"""Boxes with open axes whose atoms lie BEYOND the open faces (include/emdee_hip.h, "Open axes"), for
tests/test_open_axes_host.py (the conditions, on the CPU) and tests/test_gpu_open_axes.py (the device).  Plain numpy on top of
test_gpu_orthorhombic._system; the yardstick is tests/helpers/ortho_ref.py, which works on unwrapped coordinates and takes
`periodic`.

ortho_ref.check_inside calls an atom beyond the walls of an open axis a mistake in the test.  Here it is the point of the test:
the yardstick is therefore given walls moved far out on the open axes (as test_gpu_orthorhombic._assert_decisive does for its
exchanged lengths) -- no pair term reads the length of an open axis.

The pair cases (CASES):
    open-x    periodic (0, 1, 1), cells (6, 7, 9): x is the bricks' long axis and the axis of the sub-bins
    open-z    periodic (1, 1, 0), cells (7, 5, 9)
    droplet   periodic (0, 0, 0), cells (5, 6, 7)
all at lo = test_gpu_orthorhombic.OFFSETS != 0, with unequal sides and cell counts.  The lattice starts PAD + a / 4 inside each
open wall, so that its outermost layers cross the wall during a hot run, and per open face eight atoms are moved out at the
load: two lattice neighbours each (they stay about 1.2 apart, an outsider-outsider pair) to 0.3, to one cell width, to two
cell widths and to the guaranteed distance of the contract; the two at 0.3 are within rc of the atoms left inside."""
import numpy as np

from . import ortho_ref as oref
from ..test_gpu_orthorhombic import BAND, DT, OFFSETS, SEEDS, TOL, _pair_kw, _system  # noqa: F401  (re-exported)

PAD = -0.3                 # the lattice's outermost layer sits PAD + a / 4 = 0.13 (+- the jitter of 0.05) from an open wall
HOT = 1.4                  # test_gpu_orthorhombic's own velocity scale (its X32 is derived for it): atoms leave through every open face
NSTEPS = 40
FAR = 1e3                  # how far the yardstick's walls are moved out on open axes
CASES = {"open-x": dict(periodic=(0, 1, 1), cells=(6, 7, 9)),
         "open-z": dict(periodic=(1, 1, 0), cells=(7, 5, 9)),
         "droplet": dict(periodic=(0, 0, 0), cells=(5, 6, 7))}
# per case, the fcc_block jitter seed whose box (fp64 and fp32-rounded) keeps every pair clear of the bands around rc and
# rc + skin (test_gpu_orthorhombic.BAND); found on the CPU by find_seed() below and asserted by tests/test_open_axes_host.py and
# again by every GPU test before it touches the device
OPEN_SEEDS = {"open-x": 0x6002, "open-z": 0x6000, "droplet": 0x6001}


def cell_widths(S):
    return np.asarray(S["lengths"]) / np.asarray(S["M"])


def guaranteed_distance(S):
    """How far beyond an open face the contract holds (DESIGN.md "Open axes"): 12 widest cell widths in fp64 (the build's fp32
    pre-test margin is 4 x the rounding bound of coordinates below cmax >= 4 cell widths: it covers coordinates up to 4 cmax),
    32 - 6 widest cell widths in fp32 (a tile coordinate, at most 6 cell widths inside the bricks plus the distance, must stay
    below 2^24 grid points of 2^-19 for rel_tile to be exact)."""
    cw = cell_widths(S).max()
    return 12.0 * cw if S["dtype"] == np.float64 else 32.0 - 6.0 * cw


def far_walls(S):
    """(lo, lengths) for the yardstick: the walls of the open axes moved FAR out"""
    open_ = 1 - np.array(S["periodic"])
    return S["lo"] - FAR * open_, S["lengths"] + 2 * FAR * open_


def faces(S):
    return [(d, side) for d in range(3) if not S["periodic"][d] for side in (0, 1)]


def beyond(S, pos, d, side):
    """mask of the atoms beyond face `side` (0: lower, 1: upper) of open axis d"""
    return pos[:, d] < S["lo"][d] if side == 0 else pos[:, d] >= S["lo"][d] + S["lengths"][d]


def _round(S, pos):
    return pos.astype(np.float32).astype(np.float64) if S["dtype"] == np.float32 else pos


def pair_system(syn, name, dtype, seed=None):
    """the case `name` with its outsiders placed; S["outsiders"][(d, side)] = their ids, two per distance in the order of `dist`"""
    case = CASES[name]
    S = _system(syn, case["cells"], dtype, seed=OPEN_SEEDS[name] if seed is None else seed, lo=True, periodic=case["periodic"],
                pad=PAD, hot=HOT)
    pos, lo, hi = S["pos"].copy(), S["lo"], S["lo"] + S["lengths"]
    S["outsiders"], taken = {}, np.zeros(S["N"], dtype=bool)
    for d, side in faces(S):
        wall, sign = (lo[d], -1.0) if side == 0 else (hi[d], 1.0)
        dist = [0.3, cell_widths(S)[d], 2.0 * cell_widths(S)[d], 0.999 * guaranteed_distance(S)]
        depth = sign * (wall - pos[:, d])                       # how far inside the wall an atom is
        ids = []
        for k, want in enumerate(dist):
            # the free atom nearest the wall and its nearest free neighbour of the same lattice layer: both move out by the same
            # amount, the first to `want` exactly, the second to at most 0.1 (twice the jitter) less
            free = np.nonzero(~taken & (depth > 0))[0]
            i = free[np.argmin(depth[free])]
            taken[i] = True
            free = free[(free != i) & (depth[free] < depth[i] + 0.25)]
            j = free[np.argmin(np.linalg.norm(pos[free] - pos[i], axis=1))]
            taken[j] = True
            pos[[i, j], d] += sign * (want + depth[i])
            ids += [int(i), int(j)]
        S["outsiders"][(d, side)] = np.array(ids)
    S["pos"] = _round(S, pos)
    return S


def want(S, atoms, pos=None, periodic=None):
    """ortho_ref.total on the far walls; periodic: override (the wrong reference that treats open axes as periodic)"""
    lo, lengths = far_walls(S)
    if periodic is not None:
        lo, lengths = S["lo"], S["lengths"]
        return _total_unchecked(S, atoms, S["pos"] if pos is None else pos, lengths, periodic)
    return oref.total(S["pos"] if pos is None else pos, lo, lengths, S["periodic"], S["rc"], S["rs"], atoms, S["terms"], **_pair_kw(S))


def _total_unchecked(S, atoms, pos, lengths, periodic):
    # every axis periodic: check_inside has nothing to check, and the minimum image is taken along the open axes too
    return oref.total(pos, S["lo"], lengths, periodic, S["rc"], S["rs"], atoms, S["terms"], **_pair_kw(S))


def neighbour_rows(S, pos=None):
    return oref.neighbour_rows(S["pos"] if pos is None else pos, S["lengths"], S["periodic"], S["rc"] + S["skin"])


def assert_pair_conditions(S, atoms, right, tol):
    """The conditions of the issue, on the CPU: the outsiders are where the docstring says, every open face has an
    outsider-outsider and an outsider-insider pair within rc, no pair lies in a rounding band, and the reference that takes the
    open axes as periodic differs from the right one by at least 100 x tol."""
    pos, rc = S["pos"], S["rc"]
    assert len(set(S["M"])) == 3 and np.all(S["lo"] != 0), (S["M"], S["lo"])
    out_any = np.zeros(S["N"], dtype=bool)
    for d, side in faces(S):
        out_any |= beyond(S, pos, d, side)
    for d, side in faces(S):
        ids = S["outsiders"][(d, side)]
        out = beyond(S, pos, d, side)
        assert out[ids].all() and out.sum() >= 8, (d, side, out.sum())
        wall = S["lo"][d] + side * S["lengths"][d]
        gone = np.abs(pos[ids, d] - wall)
        cw, g = cell_widths(S)[d], guaranteed_distance(S)
        assert abs(gone[0] - 0.3) < 1e-3 and abs(gone[2] - cw) < 1e-3 and abs(gone[4] - 2 * cw) < 1e-3, gone
        assert 0.98 * g < gone[6:].min() and gone[6:].max() <= g, (gone, g)
        dd = np.linalg.norm(pos[ids][:, None, :] - pos[None, :, :], axis=2)     # (8, N) plain distances: pairs through a periodic face are not needed here
        near = dd < rc
        near[np.arange(8), ids] = False
        assert (near & out[None, :]).any(), "no outsider-outsider pair within rc at face %r" % ((d, side),)
        assert (near & ~out_any[None, :]).any(), "no outsider-insider pair within rc at face %r" % ((d, side),)
        for k in (0, 2, 4, 6):                                                  # each distance has its own outsider-outsider pair
            assert dd[k, ids[k + 1]] < rc, (d, side, k, dd[k, ids[k + 1]])
    near = oref.nearest_to_radius(pos, S["lengths"], S["periodic"], rc)
    assert near > BAND, "a pair within %.1e of the cutoff" % near
    near = oref.nearest_to_radius(pos, S["lengths"], S["periodic"], rc + S["skin"])
    assert near > 2 * BAND, "a pair within %.1e of rc + skin" % near
    wrong = want(S, atoms, periodic=[1, 1, 1])
    for key in ("f", "t"):
        diff = np.abs(wrong[key] - right[key]).max()
        assert diff >= 100 * tol * np.abs(right[key]).max(), (key, diff)


_TRAJ = {}


def trajectory(name, S, atoms, nsteps=NSTEPS):
    """ortho_ref.verlet on the case (cached per case and precision), and per open face the number of atoms that were inside it
    at the load and are beyond it at the end"""
    key = (name, S["dtype"], nsteps)
    if key not in _TRAJ:
        force = lambda x: want(S, atoms, pos=x)["f"]
        x, v = oref.verlet(S["pos"], S["vel"], force, nsteps, DT, S["inv_mass"])
        crossed = {f: int((beyond(S, x, *f) & ~beyond(S, S["pos"], *f)).sum()) for f in faces(S)}
        _TRAJ[key] = (x, v, crossed)
    return _TRAJ[key]


def find_seed(syn, name, first=0x6000, tries=4000):
    """the first seed from `first` whose fp64 and fp32 boxes both keep clear of the bands (python -m tests.helpers.open_cases)"""
    for seed in range(first, first + tries):
        ok = True
        for dtype in (np.float64, np.float32):
            S = pair_system(syn, name, dtype, seed=seed)
            ok = ok and oref.nearest_to_radius(S["pos"], S["lengths"], S["periodic"], S["rc"]) > BAND
            ok = ok and oref.nearest_to_radius(S["pos"], S["lengths"], S["periodic"], S["rc"] + S["skin"]) > 2 * BAND
            if not ok:
                break
        if ok:
            return seed
    raise AssertionError("no seed among %d" % tries)


if __name__ == "__main__":
    import importlib.util
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("syn", os.path.join(here, "..", "..", "emdee.jl_amd", "synthetic.py"))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    for name in CASES:
        print(name, hex(find_seed(syn, name)))


# ---------------------------------------------------------------- the stages behind the pair loop: slab and droplet boxes
# The molecular boxes of the other GPU modules (settle_ref.water_box, shake_ref.mixed_box, vsite_ref.four_site_box: geometry,
# counts and parameters unchanged) re-boxed as a SLAB -- periodic x and y, z open with VAC[0] of vacuum below and VAC[1] above
# the box the helper made, so lo != 0 and the two vacua differ -- and as a DROPLET, all three axes open with the same vacua.
# The vacua sum to less than rc: taken as periodic, the open axes would let the two surfaces see each other, which is what
# the wrong reference of assert_stage_conditions shows.  Molecules are whole along open axes and wrapped atom by atom along
# periodic ones.
from . import settle_ref as sr  # noqa: E402
from . import shake_ref as hr  # noqa: E402
from . import vsite_ref as vr  # noqa: E402

VAC = (0.3, 0.5)
VAC_MIXED = (0.05, 0.15)
KINDS = {"slab": (1, 1, 0), "droplet": (0, 0, 0)}
TALL_LEG, TALL_BASE, TALL_Z = 1.7, 0.5, 3.0              # legs >= 1.6 in an open length just above rc + skin = 2.9
_STAGE = {}


def _rebox(B, lo, lengths, kind, vac_axes=(0, 1, 2), vac=None):
    """B (a helper's box dict with `unwrapped`) in the slab or droplet made from the box (lo, lengths)"""
    periodic = np.array(KINDS[kind])
    grow = np.array([0.0 if periodic[d] or d not in vac_axes else 1.0 for d in range(3)])
    B, vac = dict(B), VAC if vac is None else vac
    B["lo"], B["lengths"], B["periodic"] = lo - vac[0] * grow, lengths + (vac[0] + vac[1]) * grow, [int(p) for p in periodic]
    x = np.array(B["unwrapped"])
    for d in range(3):
        if periodic[d]:
            x[:, d] = B["lo"][d] + np.mod(x[:, d] - B["lo"][d], B["lengths"][d])
    B["pos"] = x
    B["kind"] = kind
    return B


def _four_sites(B):
    """vsite_ref.four_site_box's construction on any box of three-site molecules: a massless bisector site per molecule at
    w_b = w_c = vsite_ref.W_SITE carrying the apex charge, epsilon = 0, all six pairs of a molecule excluded"""
    n, n3 = B["mol"].shape[0], len(B["unwrapped"])
    sites = np.arange(n3, n3 + n, dtype=np.int64)
    vs_atoms = np.concatenate([sites[:, None], B["mol"]], axis=1)
    vs_weights = np.full((n, 2), vr.W_SITE)
    xs = vr.place(B["unwrapped"], vs_atoms, vs_weights, np.ones(3), (0, 0, 0))          # (unwrapped: no image anywhere)
    atoms = np.concatenate([B["atoms"], np.zeros(n, dtype=B["atoms"].dtype)])
    atoms["half_sigma"][n3:] = 0.1
    charges = np.concatenate([B["charges"], B["charges"][B["mol"][:, 0]]])
    charges[B["mol"][:, 0]] = 0.0
    four = np.concatenate([B["mol"], sites[:, None]], axis=1)
    excl = np.concatenate([four[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    if "excl_more" in B:
        excl = np.concatenate([excl, B["excl_more"]])
    mass = np.concatenate([B["mass"], np.full(n, np.inf)])
    out = dict(B)
    out.update(unwrapped=np.concatenate([B["unwrapped"], xs]), vel=np.concatenate([B["vel"], np.zeros((n, 3))]), mass=mass,
               inv_mass=1.0 / mass, atoms=atoms, excl=excl, charges=charges, vs_atoms=vs_atoms, vs_weights=vs_weights, sites=sites,
               real=np.arange(n3))
    return out


def tall_molecules(seed=31, temperature=1.0, nx=7, ny=8, spacing=1.3):
    """56 triangles of legs TALL_LEG standing along z in a box TALL_Z thick: apex 0.35 (+- 0.05) above the lower face, the two
    legs about 1.68 higher, tilted by up to 0.1 rad and turned about z at random, on a 7 x 8 lattice 1.3 apart jittered by
    +- 0.15 (enough disorder that an atom's force is of the size of its largest pair term, not what a lattice leaves of it).  The apex and a leg are more than half of
    TALL_Z apart along z: the minimum image taken along z would fold the leg to the other side of the apex.  Masses, Lennard-
    Jones parameters and charges are settle_ref's."""
    rng = np.random.default_rng(seed)
    n = nx * ny
    lengths, lo = np.array([nx * spacing, ny * spacing, TALL_Z]), np.array(sr.LO)
    h = np.sqrt(TALL_LEG ** 2 - 0.25 * TALL_BASE ** 2)
    up = np.array([[0.0, 0.0, 0.0], [-0.5 * TALL_BASE, 0.0, h], [0.5 * TALL_BASE, 0.0, h]])
    ij = np.array([(i, j) for i in range(nx) for j in range(ny)], dtype=np.float64)
    centres = np.concatenate([(ij + 0.5) * spacing + 0.3 * (rng.random((n, 2)) - 0.5), 0.35 + 0.1 * (rng.random((n, 1)) - 0.5)], axis=1) + lo
    phi, tx, ty = rng.uniform(0, 2 * np.pi, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n)
    c, s, o, z = np.cos, np.sin, np.ones(n), np.zeros(n)
    rz = np.stack([np.stack([c(phi), -s(phi), z], 1), np.stack([s(phi), c(phi), z], 1), np.stack([z, z, o], 1)], 1)
    rx = np.stack([np.stack([o, z, z], 1), np.stack([z, c(tx), -s(tx)], 1), np.stack([z, s(tx), c(tx)], 1)], 1)
    ry = np.stack([np.stack([c(ty), z, s(ty)], 1), np.stack([z, o, z], 1), np.stack([-s(ty), z, c(ty)], 1)], 1)
    sites = np.einsum("nij,kj->nki", rx @ ry @ rz, up)
    x = (centres[:, None, :] + sites).reshape(-1, 3)
    mol = np.arange(3 * n, dtype=np.int64).reshape(-1, 3)
    geom = np.tile([TALL_LEG, TALL_BASE], (n, 1))
    mass = np.tile(sr.MASSES, n)
    v = rng.normal(size=x.shape) * np.sqrt(temperature / mass)[:, None]
    v -= (mass[:, None] * v).sum(axis=0) / mass.sum()
    v = sr.rattle(x, v, mol, mass)
    atoms = np.zeros(3 * n, dtype=np.dtype([("half_sigma", np.float32), ("twice_sqrt_eps", np.float32)]))
    atoms["half_sigma"], atoms["twice_sqrt_eps"] = np.tile(sr.HALF_SIGMA, n), np.tile(sr.TWICE_SQRT_EPS, n)
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]])
    return dict(unwrapped=x, vel=v, mol=mol, geom=geom, mass=mass, atoms=atoms, excl=excl, charges=np.tile(sr.CHARGES, n)), lo, lengths


def stage_box(name, kind):
    """name: "water" (settle_ref.water_box), "tall" (tall_molecules), "mixed" (shake_ref.mixed_box), or "water4" / "tall4" (the
    first two with a virtual site per molecule); kind: "slab" or "droplet".  dict of the helper's keys plus lo, lengths,
    periodic, pos (wrapped on the periodic axes only), pairs (shake_ref's constraint list of every group), inv_mass.  Cached."""
    key = (name, kind)
    if key not in _STAGE:
        base = name.rstrip("4")
        if base == "water":
            B, lo, lengths = sr.water_box(), sr.LO, sr.LENGTHS
        elif base == "tall":
            B, lo, lengths = tall_molecules()
        else:
            B, lo, lengths = hr.mixed_box(), hr.LO, hr.LENGTHS
        if base != "mixed":
            B["pairs"] = hr.triangle_pairs(B["mol"], B["geom"])
        if name.endswith("4"):
            B = _four_sites(B)
        B.setdefault("inv_mass", 1.0 / B["mass"])
        # (the tall box keeps its thickness: its z is the open length just above rc + skin)
        # (the mixed box's centres already keep 0.5 from its faces, and its largest force is a few hundred: narrower vacua keep
        # the two surfaces close enough for the wrong reference to differ by 100 x the fp32 tolerance of that force)
        _STAGE[key] = _rebox(B, lo, lengths, kind, vac_axes=(0, 1) if base == "tall" else (0, 1, 2), vac=VAC_MIXED if base == "mixed" else VAC)
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in _STAGE[key].items()}


def stage_total(B, x=None, periodic=None, charged=False, **kw):
    """ortho_ref.total on the box's atoms at rc, rs of settle_ref (walls moved out); periodic: override, the wrong reference"""
    x = B["unwrapped"] if x is None else x
    open_ = 1 - np.array(B["periodic"])
    lo, lengths, per = B["lo"] - FAR * open_, B["lengths"] + 2 * FAR * open_, B["periodic"]
    if periodic is not None:
        lo, lengths, per = B["lo"], B["lengths"], list(periodic)
    if charged:
        kw.update(charges=B["charges"], coulomb_k=1.0)
    return oref.total(x, lo, lengths, per, sr.RC, sr.RS, B["atoms"], kw.pop("terms", None), excl=B["excl"], **kw)


def assert_stage_conditions(B, tol, charged=False, energy=False):
    """every atom inside the walls of the open axes (the molecular boxes start there), the cell grid one the engine accepts, and
    the force field with the open axes taken as periodic at least 100 x tol away from the right one -- in the forces, or
    (energy: the minimiser's test, whose clashing start has forces of 1e4) in the total energy, the quantity that test compares"""
    for d in range(3):
        assert B["periodic"][d] or ((B["pos"][:, d] > B["lo"][d]).all() and (B["pos"][:, d] < B["lo"][d] + B["lengths"][d]).all()), d
        assert B["lengths"][d] >= (2.0 if B["periodic"][d] else 1.0) * (sr.RC + sr.SKIN), (d, B["lengths"][d])
    assert np.all(B["lo"] != 0.0)
    right, wrong = stage_total(B, charged=charged), stage_total(B, periodic=(1, 1, 1), charged=charged)
    if energy:
        assert abs(wrong["e"].sum() - right["e"].sum()) >= 100 * tol * abs(right["e"].sum())
        return right
    diff = np.abs(wrong["f"] - right["f"]).max()
    assert diff >= 100 * tol * np.abs(right["f"]).max(), diff
    return right


def tall_spans(B):
    """per molecule, the largest |dz| between two of its sites over the open length"""
    z = B["unwrapped"][B["mol"], 2]
    return (z.max(axis=1) - z.min(axis=1)) / B["lengths"][2]


# ---------------------------------------------------------------- chains along the open axis of a one-cell-thick slab
CHAIN_CELLS, CHAIN_LIFT = (7, 5, 2), 0.5
CHAIN_SEED = 0x6100             # clear of the bands around rc and rc + skin in fp64 and fp32 (found on the CPU, asserted by the tests)
CHAIN_STEPS = 20


def chain_system(E, dtype, seed=None):
    """test_gpu_orthorhombic._chain_system's ingredients (test_gpu_bonded._chains, _lj14scale, the same charges, masses and
    reaction field) on a slab of CHAIN_CELLS fcc cells, periodic (1, 1, 0), whose open length 2 a + 2 PAD = 2.82 is one cell of
    rc + skin.  The atoms are renumbered so that a chain is {A, B, C, D} = a basis atom of the lower and of the upper cell of a
    column, then the basis atom of the same height of the two cells: the bonds A-B and C-D run along z and are a = 1.71 long,
    more than half the open length -- the minimum image taken along z would turn them round.  The lattice is lifted by
    CHAIN_LIFT: the even chains (basis atoms 0 and 1, at heights 0 and a) stay inside the walls, the odd ones (basis atoms 3
    and 2, at a / 2 and 3 a / 2) have their B and D beyond the upper face."""
    from ..test_gpu_bonded import _chains
    from ..test_gpu_dd_pairs import _lj14scale
    S = _system(E.synthetic, CHAIN_CELLS, dtype, seed=CHAIN_SEED if seed is None else seed, lo=True, periodic=(1, 1, 0), species=2,
                hot=1.0, pad=PAD)
    nx, ny, nz = CHAIN_CELLS
    order = []
    for cy in range(ny):
        for cx in range(nx):
            g0, g1 = 4 * (cx + nx * cy), 4 * (cx + nx * (cy + ny))
            order += [g0, g1, g0 + 1, g1 + 1, g0 + 3, g1 + 3, g0 + 2, g1 + 2]
    order = np.array(order)
    assert np.array_equal(np.sort(order), np.arange(S["N"]))
    for key in ("pos", "vel", "eps", "sigma"):
        S[key] = S[key][order]
    S["pos"][:, 2] += CHAIN_LIFT
    S["pos"] = _round(S, S["pos"])
    N = S["N"]
    S["terms"], S["excl"], S["p14"] = _chains(N)
    S["s14"], S["c14"] = _lj14scale(E), 0.8333
    S["q"], S["coulomb"] = np.tile([0.6, -0.3, -0.5, 0.2], N // 4), (1.0, 5.0)
    S["inv_mass"] = 1.0 / (1.0 + 0.5 * (np.arange(N) % 3))
    return S


def chain_parts(S, atoms, periodic=None):
    """(bonded, coulomb, whole) of ortho_ref; periodic: override (the wrong references)"""
    lo, lengths = far_walls(S)
    per = S["periodic"]
    if periodic is not None:
        lo, lengths, per = S["lo"], S["lengths"], list(periodic)
    kw = _pair_kw(S)
    bonded = oref.bonded(S["pos"], lengths, per, S["terms"])
    coul = oref.nonbonded(S["pos"], lo, lengths, per, S["rc"], S["rs"], atoms, lj=False, **kw)
    whole = oref.total(S["pos"], lo, lengths, per, S["rc"], S["rs"], atoms, S["terms"], **kw)
    return bonded, coul, whole


def assert_chain_conditions(S, atoms, parts, tol):
    up = S["lo"][2] + S["lengths"][2]
    z = S["pos"][:, 2].reshape(-1, 4)
    assert S["M"][2] == 1 and (z > S["lo"][2]).all() and (z[0::2] < up).all()
    assert (z[1::2, [1, 3]] > up).all() and (z[1::2, [0, 2]] < up).all()                     # B and D of the odd chains: beyond the face
    assert (np.abs(z[:, 1] - z[:, 0]) > 0.5 * S["lengths"][2]).all() and (np.abs(z[:, 3] - z[:, 2]) > 0.5 * S["lengths"][2]).all()
    assert oref.nearest_to_radius(S["pos"], S["lengths"], S["periodic"], S["rc"]) > BAND
    wrong = chain_parts(S, atoms, periodic=(1, 1, 1))
    for name, r, w in zip(("bonded", "coulomb", "whole"), parts, wrong):
        diff = np.abs(w["f"] - r["f"]).max()
        assert diff >= 100 * tol * np.abs(r["f"]).max(), (name, diff)


def chain_trajectory(S, atoms, nsteps):
    key = ("chains", S["dtype"], nsteps)
    if key not in _TRAJ:
        lo, lengths = far_walls(S)
        force = lambda x: oref.total(x, lo, lengths, S["periodic"], S["rc"], S["rs"], atoms, S["terms"], **_pair_kw(S))["f"]
        _TRAJ[key] = oref.verlet(S["pos"], S["vel"], force, nsteps, DT, S["inv_mass"])
    return _TRAJ[key]


# ---------------------------------------------------------------- pressure coupling on a slab
SLAB_CELLS, SLAB_PAD, SLAB_SEED = (6, 6, 4), 0.6, 0x5EED
COUPLING_STEPS, COUPLING_EVERY = 40, 5


def lj_slab(syn):
    """A Lennard-Jones slab for the coupling tests: 6 x 6 x 4 fcc cells (576 atoms), periodic (1, 1, 0), 0.6 + a / 4 of vacuum on
    either side along z (less than rc in all: the wrong reference sees the slab's other surface), lo != 0, fp64.  The atoms stay
    inside the walls over the run (barostat_ref.field checks it at every force evaluation)."""
    S = _system(syn, SLAB_CELLS, np.float64, seed=SLAB_SEED, lo=True, periodic=(1, 1, 0), pad=SLAB_PAD, hot=1.0, unwrap=False)
    return S


def coupling_case(syn, kind, xi=None):
    """barostat_ref.coupled_verlet on lj_slab with field(..., periodic=(1, 1, 0)): kind "semi-z0" (Berendsen semi-isotropic,
    compressibility_z = 0), "aniso" (Berendsen anisotropic) or "crescale" (needs xi(s)).  p_ref and the compressibilities are
    barostat_ref.berendsen_case's: 20 (12, 28) above the starting pressure, about 0.02, tau_p = 1.  Cached."""
    from . import barostat_ref as bref
    key = ("coupling", kind)
    if key not in _TRAJ:
        S = lj_slab(syn)
        atoms = bref.lj_atoms(S["N"])
        tot = bref.field(atoms, lo=S["lo"], periodic=S["periodic"], rc=S["rc"], rs=S["rs"])
        P0 = bref.pressure_diagonal(S["vel"], tot(S["pos"], S["lengths"])["t"], S["lengths"]).mean()
        p_ref, beta, tau_p = np.round(P0) + np.array([20.0, 12.0, 28.0]), np.array([0.02, 0.025, 0.015]), 1.0
        if kind == "semi-z0":
            beta[2] = 0.0
            args = (bref.BERENDSEN, p_ref, beta, tau_p, COUPLING_EVERY, bref.SEMIISOTROPIC)
            kw = {}
        elif kind == "aniso":
            args, kw = (bref.BERENDSEN, p_ref, beta, tau_p, COUPLING_EVERY, bref.ANISOTROPIC), {}
        else:
            args, kw = (bref.CRESCALE, p_ref[0], beta[0], tau_p, COUPLING_EVERY, bref.ISOTROPIC), dict(temperature=1.0, xi=xi)
        x, v, ln, ev = bref.coupled_verlet(S["pos"], S["vel"], S["lo"], S["lengths"], tot, COUPLING_STEPS, DT, *args, **kw)
        wrong = bref.field(atoms, lo=S["lo"], periodic=(1, 1, 1), rc=S["rc"], rs=S["rs"])(S["pos"], S["lengths"])
        _TRAJ[key] = dict(S=S, atoms=atoms, x=x, v=v, lengths=ln, events=ev, p_ref=p_ref, beta=beta, tau_p=tau_p, every=COUPLING_EVERY,
                          right=tot(S["pos"], S["lengths"]), wrong=wrong)
    return _TRAJ[key]


def assert_coupling_conditions(R, tol):
    """the wrong reference differs in the forces and in the pressure the coupling reads; every event moves the box by 1e-4 .. 1e-2"""
    from . import barostat_ref as bref
    S = R["S"]
    assert np.abs(R["wrong"]["f"] - R["right"]["f"]).max() >= 100 * tol * np.abs(R["right"]["f"]).max()
    Pr, Pw = (bref.pressure_diagonal(S["vel"], R[k]["t"], S["lengths"]) for k in ("right", "wrong"))
    assert np.abs(Pw - Pr).max() >= 100 * tol * np.abs(Pr).max()
    mus = np.array([e[2] for e in R["events"]])
    assert len(mus) == COUPLING_STEPS // COUPLING_EVERY
    return mus


# ---------------------------------------------------------------- a clashing droplet for the minimiser
# fire_ref.minimize on clashing_droplet() (tests/test_gpu_minimize.TIGHT, f_tol = WATER_FTOL = 17) converges in this many
# iterations; counted on the CPU by tests/test_open_axes_host.py
DROPLET_ITERS = 39


def clashing_droplet():
    """fire_ref.clashing_water_box() (molecules moved and turned until neighbours clash) re-boxed as a droplet"""
    from . import fire_ref as fr
    if "clash" not in _STAGE:
        B = fr.clashing_water_box()
        B["pairs"] = hr.triangle_pairs(B["mol"], B["geom"])
        B["inv_mass"] = 1.0 / B["mass"]
        _STAGE["clash"] = _rebox(B, sr.LO, sr.LENGTHS, "droplet")
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in _STAGE["clash"].items()}
