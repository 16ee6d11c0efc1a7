"""Boxes of tests/test_gpu_images.py: dyadic copies of the family boxes of mask_cases, on which a shift by whole box lengths is
exact in Float32, the hand-made (8, 16, 32) box, the image counts the tests shift atoms by, and the face sets.  numpy only.

A dyadic box: every length of the family box (positions, side, sigma, rc, rs, skin, velocities) times the one factor that makes
the side a power of two -- cells per side, atoms per cell and row lengths stay, so the planner's choice stays -- and every
coordinate rounded to a multiple of side 2^-13.  A coordinate is then q (n + 8192 k) with q = side 2^-13, 0 <= n < 8192 and
|k| <= 500: 23 bits, exact in Float32, and so are (p - lo) / len, its floor, p - k len and the differences of two such
coordinates."""
import math

import numpy as np

from . import mask_cases as mc
from . import ortho_ref as oref

GRID_BITS = 13
KMAX = 500
DT = 0.005
STEPS = 12
DRIFT = 0.045          # of sigma per step, the fastest atom: 12 steps carry it 0.54 sigma, the rebuild threshold skin / 2 = 0.15


def snap(pos, lo, lengths):
    """every coordinate on the grid lo + n len 2^-13, 0 <= n < 8192"""
    lo, lengths = np.asarray(lo, dtype=np.float64), np.asarray(lengths, dtype=np.float64)
    q = lengths * 2.0 ** -GRID_BITS
    n = np.mod(np.rint((np.asarray(pos, dtype=np.float64) - lo) / q), 2 ** GRID_BITS)
    return lo + n * q


def _fast_velocities(vel, sigma_unit):
    """the box's velocities rescaled so that the fastest atom drifts DRIFT sigma per step of DT"""
    vmax = np.sqrt((vel * vel).sum(axis=1)).max()
    return vel * (DRIFT * sigma_unit / DT / vmax)


def assert_rebuilds_twice(box):
    """CPU-side condition of the 12-step runs: in free flight the fastest atom passes skin / 2 at least three times"""
    vmax = np.sqrt((box["vel"] * box["vel"]).sum(axis=1)).max()
    assert STEPS * DT * vmax >= 3.0 * 0.5 * box["skin"], (vmax, box["skin"])


_BOX = {}


def dyadic_box(E, family, dtype):
    """the family box of mask_cases scaled and rounded as the module's docstring says; lo = 0; plan(err) is the family's"""
    key = (family, dtype if family == "long_rows" else None)
    if key not in _BOX:
        src = mc.family_box(E, family, dtype)
        L = src["lengths"][0]
        assert src["lengths"] == [L] * 3 and src["periodic"] == [1, 1, 1]
        side = 2.0 ** round(math.log2(L))
        s = side / L
        atoms = src["atoms"].copy()
        atoms["half_sigma"] = (atoms["half_sigma"].astype(np.float64) * s).astype(np.float32)
        box = dict(key="dyadic_" + src["key"], lo=[0.0] * 3, lengths=[side] * 3, periodic=[1, 1, 1], atoms=atoms, rc=src["rc"] * s,
                   rs=src["rs"] * s, skin=0.3 * s, env=src["env"], plan=src["plan"], scale=s)
        box["pos"] = snap(src["pos"] * s, box["lo"], box["lengths"])
        box["vel"] = _fast_velocities(src["vel"], s).astype(np.float32).astype(np.float64)
        # (the rounding moves an atom by at most side 2^-14 per axis: no pair comes closer than the lattice's jitter allows)
        _BOX[key] = box
    return dict(_BOX[key])


ORTHO_SIGMA = 0.9


def ortho_box(E, m=0):
    """sides (8, 16, 32) 2^m at lo = (-1.0, 0.5, 2.0) 2^m: 4 x 8 x 16 fcc cells of side 2 (2048 atoms), three species about
    sigma = 0.9, so that rc + skin = 2.52 gives 3, 6 and 12 cells per side"""
    key = ("ortho", m)
    if key not in _BOX:
        u = 2.0 ** m
        # (jitter 0.5 of the layer spacing 1: no cell face is further than 0.09 from where the atoms of a layer lie)
        pos, gid, lengths = E.synthetic.fcc_block((4, 8, 16), (0, 0, 0), (4, 8, 16), rho=0.5, jitter=0.5)
        assert np.allclose(lengths, (8.0, 16.0, 32.0))
        pos = pos[np.argsort(gid)]
        N = pos.shape[0]
        lo, lengths = np.array([-1.0, 0.5, 2.0]) * u, np.array([8.0, 16.0, 32.0]) * u
        k = np.arange(N) % 3
        eps, sigma = np.array([1.0, 0.8, 0.6])[k], ORTHO_SIGMA * u * np.array([1.0, 0.95, 0.9])[k]
        rc, rs, skin = 2.5 * ORTHO_SIGMA * u, 2.0 * ORTHO_SIGMA * u, 0.3 * ORTHO_SIGMA * u
        assert [int(math.floor(l / (rc + skin))) for l in lengths] == [3, 6, 12]

        def plan(err):
            lines = [l for l in err.splitlines() if l.startswith("emdee plan: bricks")]
            assert lines and "direct kernels" not in err and "two species" not in err, err[-600:]

        box = dict(key="dyadic_ortho%d" % m, lo=list(lo), lengths=list(lengths), periodic=[1, 1, 1], atoms=E.lennard_jones_atoms(eps, sigma),
                   rc=rc, rs=rs, skin=skin, env={}, plan=plan, scale=ORTHO_SIGMA * u)
        box["pos"] = snap(pos * u + lo, lo, lengths)
        box["vel"] = _fast_velocities(E.synthetic.velocities(N), ORTHO_SIGMA * u).astype(np.float32).astype(np.float64)
        _BOX[key] = box
    return dict(_BOX[key])


def image_counts(N, draw, seed=0x1A6E):
    """(N, 3) integer box lengths per atom and axis: draw "uniform" from -500 .. 500, draw "extremes" from {-500, 0, 500}"""
    rng = np.random.default_rng(seed + (0 if draw == "uniform" else 1))
    if draw == "uniform":
        return rng.integers(-KMAX, KMAX + 1, size=(N, 3))
    return KMAX * rng.integers(-1, 2, size=(N, 3))


def shifted(box, k):
    """the box's positions plus k box lengths; asserts that the sum is exact in Float32 (and so in Float64)"""
    x = box["pos"] + k * np.asarray(box["lengths"])
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x), "a shifted coordinate is not a Float32 number"
    assert np.array_equal(oref.wrapped(x, box["lo"], box["lengths"], box["periodic"]), box["pos"]), "the shift is not whole box lengths"
    return x


def assert_dyadic(box):
    """the CPU-side conditions of an exact box: power-of-two sides, coordinates on the 2^-13 grid inside [lo, lo + len)"""
    lo, lengths = np.asarray(box["lo"]), np.asarray(box["lengths"])
    assert all(math.frexp(l)[0] == 0.5 for l in lengths), lengths
    n = (box["pos"] - lo) / (lengths * 2.0 ** -GRID_BITS)
    assert np.array_equal(n, np.rint(n)) and (n >= 0).all() and (n < 2 ** GRID_BITS).all()
    assert np.array_equal(box["pos"].astype(np.float32).astype(np.float64), box["pos"])


# ---------------------------------------------------------------- faces
BAND = 1e-5            # tests/test_gpu_orthorhombic.py: no pair within BAND (relative, r^2) of rc, 2 BAND of rc + skin


def cells_per_side(box):
    """configure_grid's count: floor(len / (rc + skin))"""
    return [int(math.floor(l / (box["rc"] + box["skin"]))) for l in box["lengths"]]


def face_targets(box, dtype):
    """[(axis, c, side, value)]: per axis the planes lo + c len / M, c = 0 .. M (c = M: lo + len), rounded to the engine's type,
    and the neighbours of each in that type (side -1, +1)"""
    out = []
    for d, (lo, L, M) in enumerate(zip(box["lo"], box["lengths"], cells_per_side(box))):
        for c in range(M + 1):
            v = dtype(lo + c * L / M)
            out += [(d, c, 0, float(v)), (d, c, -1, float(np.nextafter(v, dtype(-np.inf)))), (d, c, 1, float(np.nextafter(v, dtype(np.inf))))]
    return out


def _row_is_clear(pos, a, box, hs, struck):
    """atom a keeps 0.8 sigma_ij from every (non-excluded) atom and its pairs keep clear of the bands about rc and rc + skin"""
    L = np.asarray(box["lengths"])
    d = pos - pos[a]
    d -= L * np.rint(d / L)
    r2 = np.einsum("ij,ij->i", d, d)
    r2[a] = np.inf
    near = r2 < (0.8 * (hs + hs[a])) ** 2
    near[list(struck.get(a, ()))] = False
    if near.any():
        return False
    for r, band in ((box["rc"], BAND), (box["rc"] + box["skin"], 2 * BAND)):
        if (np.abs(r2 - r * r) <= 2 * band * r * r).any():
            return False
    return True


def with_face_atoms(box, dtype):
    """the box (its positions rounded to the engine's type) with, per target of face_targets, an atom moved onto it along that
    axis: the nearest atom not yet used whose pairs the move leaves further apart than 0.8 sigma_ij and clear of the bands about
    rc and rc + skin (twice the bands assert_face_conditions then asserts) -> (box, faces = [(atom, axis, c, side)])"""
    pos = box["pos"].astype(dtype).astype(np.float64)
    L = np.asarray(box["lengths"])
    hs = np.asarray(box["atoms"])["half_sigma"].astype(np.float64)
    struck = {}
    for i, j in ([] if box.get("excl") is None else np.asarray(box["excl"])):
        struck.setdefault(int(i), set()).add(int(j))
        struck.setdefault(int(j), set()).add(int(i))
    used, faces = set(), []
    for d, c, side, value in face_targets(box, dtype):
        gap = pos[:, d] - value
        gap = np.abs(gap - L[d] * np.rint(gap / L[d]))
        for a in np.argsort(gap, kind="stable")[:64]:
            a = int(a)
            if a in used:
                continue
            old = pos[a, d]
            pos[a, d] = value
            if _row_is_clear(pos, a, box, hs, struck):
                break
            pos[a, d] = old
        else:
            raise AssertionError("no atom fits the face %r" % ((d, c, side),))
        used.add(a)
        faces.append((a, d, c, side))
    assert np.array_equal(pos.astype(dtype).astype(np.float64), pos)
    return dict(box, pos=pos, base=box["pos"], key=box["key"] + "_faces%d" % np.dtype(dtype).itemsize), faces


def assert_face_conditions(box, faces, sigma, excl=None, sample=8):
    """CPU-side, before any device work: every snapped atom moved less than 0.15 sigma; no (non-excluded) pair of a snapped or
    sampled atom closer than 0.8 sigma_ij; no such pair within BAND of rc or 2 BAND of rc + skin.  (Boxes of up to 2500 atoms:
    every pair.  Larger: the rows of the snapped atoms, the only pairs the snapping changed, and of every `sample`-th atom.)"""
    from . import virial_tensor_ref as vt
    pos, L, per = box["pos"], np.asarray(box["lengths"]), box["periodic"]
    moved = oref.image_difference(pos, box["base"], L, per)
    assert np.abs(moved).max() < 0.15 * sigma, np.abs(moved).max()
    N = pos.shape[0]
    rows = None if N <= 2500 else np.unique(np.concatenate([[f[0] for f in faces], np.arange(0, N, max(sample, N // 120))]))
    w = oref.wrapped(pos, box["lo"], L, per)
    hs = np.asarray(box["atoms"])["half_sigma"].astype(np.float64)
    i, j, dvec = vt.pairs_in_range(w, L, per, 1.1 * sigma, rows=rows, margin=0.0)
    keep = np.ones(i.shape[0], dtype=bool)
    if excl is not None:
        keep = ~np.isin(vt._pair_key(i, j, N), vt._pair_key(np.asarray(excl)[:, 0], np.asarray(excl)[:, 1], N))
    r = np.sqrt(np.einsum("ij,ij->i", dvec, dvec))[keep]
    assert (r > 0.8 * (hs[i] + hs[j])[keep]).all(), (r / (hs[i] + hs[j])[keep]).min()
    # (the bands: on the pairs the snapping changed.  A box of 4000 atoms at this density has some nine pairs within 2 BAND of
    # rc + skin among its other pairs, whichever seed: the tests compare those rows up to the band)
    snapped = np.array(sorted(f[0] for f in faces))
    assert oref.nearest_to_radius(w, L, per, box["rc"], rows=snapped) > BAND
    assert oref.nearest_to_radius(w, L, per, box["rc"] + box["skin"], rows=snapped) > 2 * BAND


def other_images(box, faces, dtype, exact):
    """every face atom given as another image of itself: the atoms on lo and lo + len exchanged, the rest one side up or down
    (towards the box).  exact: only where the sum is a number of the engine's type (dyadic boxes: the two engines then see
    the same atoms bit for bit); else rounded to it.  -> (positions, how many atoms moved)"""
    pos = box["pos"].copy()
    n = 0
    for a, d, c, side in faces:
        lo, L = box["lo"][d], box["lengths"][d]
        for step in ((-L, L) if pos[a, d] >= lo + 0.5 * L else (L, -L)):
            new = pos[a, d] + step
            if (float(dtype(new)) == new and new - step == pos[a, d]) or not exact:
                pos[a, d] = float(dtype(new))
                n += 1
                break
    return pos, n


def settle_lj_box(E):
    """the non-dyadic box of tests/test_gpu_settle.py -- sides (7.0, 7.5, 8.2) at lo = (-1.0, 0.5, 2.0), rc = 2.5, skin = 0.4, two
    cells per side -- filled with plain Lennard-Jones atoms (sigma = 1): 4 x 4 x 5 fcc cells stretched to the sides, 320 atoms.
    (That module's own atoms are water molecules on a lattice whose planes keep 0.2 and more from the faces along x, where
    lo and lo + len / 2 lie half a lattice spacing out of phase: no atom of it can be moved onto both planes by less than
    0.15 sigma.  The layers of this lattice lie on all three planes of every axis.)"""
    from . import settle_ref as sr
    if "settle_lj" not in _BOX:
        lo, L = np.asarray(sr.LO, dtype=np.float64), np.asarray(sr.LENGTHS, dtype=np.float64)
        pos, gid, lengths = E.synthetic.fcc_block((4, 4, 5), (0, 0, 0), (4, 4, 5))
        pos = pos[np.argsort(gid)] * (L / np.asarray(lengths))
        N = pos.shape[0]

        def plan(err):
            pass

        _BOX["settle_lj"] = dict(key="settle_lj", pos=lo + np.mod(pos, L), vel=E.synthetic.velocities(N), lo=list(lo), lengths=list(L),
                                 periodic=[1, 1, 1], atoms=E.lennard_jones_atoms(1.0, 1.0, N), rc=sr.RC, rs=sr.RS, skin=sr.SKIN, env={},
                                 plan=plan, scale=1.0)
    return dict(_BOX["settle_lj"])


def crossing_velocities(box, faces, dt, dtype, steps=20, distance=0.1):
    """the box's velocities with every face atom sent through its face: `distance` sigma in `steps` steps along the face's axis,
    the atom just above the face downwards, the atom just below it and the one on it upwards"""
    vel = box["vel"].copy()
    for a, d, c, side in faces:
        vel[a, d] = (-1.0 if side > 0 else 1.0) * distance * box["scale"] / (steps * dt)
    return vel.astype(dtype).astype(np.float64)


def assert_crossed(box, faces, x_end):
    """CPU-side condition on the yardstick's unwrapped trajectory: each face atom ends 0.02 sigma or more beyond its face, on the
    side it was sent to -- every face is crossed upwards (twice) and downwards (once)"""
    for a, d, c, side in faces:
        moved = x_end[a, d] - box["pos"][a, d]
        assert (moved < -0.02 * box["scale"]) if side > 0 else (moved > 0.02 * box["scale"]), (a, d, c, side, moved)


def sheared_box(box, amplitude):
    """a dyadic cubic box with a smooth shear wave on it, x += A sin(2 pi y / L), y += A sin(2 pi z / L), z += A sin(2 pi x / L),
    and every atom put back on the grid.  The two-species box is an fcc lattice of 58 layers per side with little jitter under 13
    cells: most cell faces lie further than 0.15 sigma from every atom, up to half a layer spacing (0.55).  Under the wave the
    layers of each axis take every offset up to A somewhere along every plane, while neighbours move together: with A = 0.6 the
    strain is 2 pi A / L = 0.06, and no pair comes closer than the lattice allows less 6 %."""
    L = box["lengths"][0]
    p = box["pos"]
    w = amplitude * np.sin(2.0 * np.pi * p[:, [1, 2, 0]] / L)
    return dict(box, pos=snap(p + w, box["lo"], box["lengths"]), key=box["key"] + "_sheared")
