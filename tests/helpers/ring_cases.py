"""Cases for the bonded terms off the beaten track (tests/test_bonded_terms_host.py, tests/test_gpu_bonded_rings.py): geometries
built from their internal coordinates in a random frame, exactly and nearly singular ones, a reference of the formulas that works
in any numpy float format, the rounding model that bounds a term's error, and the topologies the GPU tests run -- rings,
branches, improper-style torsions and the fused-ring solute of the force-field fixture.

The rounding model.  u is the unit round-off of the format under test (2^-24, 2^-53).  A term's vectors carry a relative error
of a few u; the cross product of two vectors at an angle theta loses 1 / sin(theta) of that (its components are differences of
nearly equal products), and so does the direction of the force, which is built from it.  An angle's force on an end atom has
magnitude M = |k (theta - theta0)| / |arm|, so its error is bounded by C u M / sin(theta); theta itself comes out of atan2 with an
absolute error of a few u, which costs C u k / |arm| more -- the larger part where theta is at theta0 and M goes to zero.  A
torsion's force on an end atom has magnitude |dU/dphi| / (|b1| sin(theta_1)); phi inherits the 1 / sin(theta_1) of the cross
product and dU/dphi = -k n sin(n phi - phase) can vanish while its slope in phi is k n^2, so the error is stated against
k n^2 / (|b1| sin(theta_1)), as C u / min(sin(theta_1), sin(theta_3)) of that.  The inner atoms take the sums of the ends' bounds
weighted by the lever arms.  A bond's force k (r - r0) loses u r in the difference: C u (|F| + k r).  C is measured in
tests/test_bonded_terms_host.py (DESIGN.md has the figures)."""
import numpy as np

from . import bonded_ref as br

U32, U64 = 2.0 ** -24, 2.0 ** -53
# 4 x the worst err sin(theta) / (u M) of the host sweep, rounded up to a power of two (test_bonded_terms_host.py asserts the tie)
C_BOUND = 16.0


def unit_roundoff(dtype):
    return U32 if np.dtype(dtype) == np.float32 else U64


# ------------------------------------------------------------------------------------ geometries
def frames(rng, n):
    """n random orthonormal frames (n, 3, 3): rows e1, e2, e3"""
    q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    return np.swapaxes(q, 1, 2)


def angle_geometry(theta, la, lb, R, origin=None):
    """(n, 4, 3): atoms 0, 1 (the vertex), 2 of an angle theta with arms la, lb in the frames R; the fourth row is zero"""
    theta, la, lb = (np.asarray(t, dtype=np.float64) for t in (theta, la, lb))
    n = R.shape[0]
    u = np.zeros((n, 4, 3))
    o = np.zeros((n, 3)) if origin is None else origin
    u[:, 1] = o
    u[:, 0] = o + la[:, None] * R[:, 0]
    u[:, 2] = o + lb[:, None] * (np.cos(theta)[:, None] * R[:, 0] + np.sin(theta)[:, None] * R[:, 1])
    return u


def torsion_geometry(th1, th3, phi, l1, l2, l3, R, origin=None):
    """(n, 4, 3): a torsion with the IUPAC dihedral phi, theta_1 the angle between b1 = x1 - x0 and b2 = x2 - x1, theta_3 the one
    between b2 and b3 = x3 - x2, bond lengths l1, l2, l3, in the frames R (b2 along e3)"""
    th1, th3, phi, l1, l2, l3 = (np.asarray(t, dtype=np.float64)[:, None] for t in (th1, th3, phi, l1, l2, l3))
    e1, e2, e3 = R[:, 0], R[:, 1], R[:, 2]
    n = R.shape[0]
    o = np.zeros((n, 3)) if origin is None else origin
    b1 = l1 * (np.sin(th1) * e1 + np.cos(th1) * e3)
    w = phi - np.pi                                          # m = b1 x b2 points along -e2: phi = w + pi
    b3 = l3 * (np.sin(th3) * (np.cos(w) * e1 + np.sin(w) * e2) + np.cos(th3) * e3)
    u = np.zeros((n, 4, 3))
    u[:, 1] = o
    u[:, 0] = o - b1
    u[:, 2] = o + l2 * e3
    u[:, 3] = u[:, 2] + b3
    return u


# ------------------------------------------------------------------------------------ the reference, in any float format
def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _safe(d):
    return np.where(d > 0, d, 1)


def reference(kind, u, p, dtype=np.float64):
    """bonded_ref.term_forces over a batch: u (n, 4, 3), p (n, 3) -> U (n,), F (n, 4, 3), every operation in dtype.  A term at a
    singular geometry (a zero denominator) has zero force."""
    u, p = np.asarray(u).astype(dtype), np.asarray(p).astype(dtype)
    F = np.zeros(u.shape, dtype=dtype)
    if kind == br.BOND:
        d = u[:, 1] - u[:, 0]
        r = _norm(d)
        g = np.where(r > 0, p[:, 0] * (r - p[:, 1]) / _safe(r), 0)
        F[:, 0], F[:, 1] = g[:, None] * d, -g[:, None] * d
        return p[:, 0] * (r - p[:, 1]) ** 2 / 2, F
    if kind == br.ANGLE:
        a, b = u[:, 0] - u[:, 1], u[:, 2] - u[:, 1]
        c = np.cross(a, b)
        cn = _norm(c)
        th = np.arctan2(cn, _dot(a, b))
        dU = p[:, 0] * (th - p[:, 1])
        ok = cn > 0
        F[:, 0] = np.where(ok, -dU / _safe(_dot(a, a) * cn), 0)[:, None] * np.cross(a, c)
        F[:, 2] = np.where(ok, dU / _safe(_dot(b, b) * cn), 0)[:, None] * np.cross(b, c)
        F[:, 1] = -F[:, 0] - F[:, 2]
        return p[:, 0] * (th - p[:, 1]) ** 2 / 2, F
    b1, b2, b3 = u[:, 1] - u[:, 0], u[:, 2] - u[:, 1], u[:, 3] - u[:, 2]
    m, n = np.cross(b1, b2), np.cross(b2, b3)
    b2n = _norm(b2)
    phi = np.arctan2(b2n * _dot(b1, n), _dot(m, n))
    arg = p[:, 1] * phi - p[:, 2]
    dU = -p[:, 0] * p[:, 1] * np.sin(arg)
    mm, nn, b22 = _dot(m, m), _dot(n, n), _dot(b2, b2)
    ok = (mm > 0) & (nn > 0) & (b22 > 0)
    z = np.zeros_like(dU)
    gi = np.where(ok, -b2n / _safe(mm), z)[:, None] * m
    gl = np.where(ok, b2n / _safe(nn), z)[:, None] * n
    s1, s3 = np.where(ok, _dot(b1, b2) / _safe(b22), z), np.where(ok, _dot(b3, b2) / _safe(b22), z)
    gj = -(1 + s1)[:, None] * gi + s3[:, None] * gl
    gk = -gi - gl - gj
    F[:, 0], F[:, 1], F[:, 2], F[:, 3] = (-dU[:, None] * g for g in (gi, gj, gk, gl))
    return p[:, 0] * (1 + np.cos(arg)), F


def internal(kind, u, dtype=np.float64):
    """the internal coordinates the bounds need, in dtype: bond -> r; angle -> theta, sin(theta), |a|, |b|; torsion -> phi,
    sin(theta_1), sin(theta_3), |b1|, |b2|, |b3|"""
    u = np.asarray(u).astype(dtype)
    if kind == br.BOND:
        return (_norm(u[:, 1] - u[:, 0]),)
    if kind == br.ANGLE:
        a, b = u[:, 0] - u[:, 1], u[:, 2] - u[:, 1]
        cn, la, lb = _norm(np.cross(a, b)), _norm(a), _norm(b)
        return np.arctan2(cn, _dot(a, b)), cn / (la * lb), la, lb
    b1, b2, b3 = u[:, 1] - u[:, 0], u[:, 2] - u[:, 1], u[:, 3] - u[:, 2]
    m, n = np.cross(b1, b2), np.cross(b2, b3)
    l1, l2, l3 = _norm(b1), _norm(b2), _norm(b3)
    return np.arctan2(l2 * _dot(b1, n), _dot(m, n)), _norm(m) / (l1 * l2), _norm(n) / (l2 * l3), l1, l2, l3


def error_scales(kind, u, p, absolute=True):
    """(n, 4): per atom of each term, the magnitude S such that the rounding model bounds the error of its force by C u S (the
    module's docstring).  absolute=False leaves out an angle's C u k / |arm| part: the purely relative bound, for angles far
    from theta0."""
    u, p = np.asarray(u, dtype=np.float64), np.asarray(p, dtype=np.float64)
    S = np.zeros(u.shape[:2])
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == br.BOND:
            r, = internal(kind, u)
            S[:, 0] = S[:, 1] = np.abs(p[:, 0] * (r - p[:, 1])) + p[:, 0] * r
        elif kind == br.ANGLE:
            th, sn, la, lb = internal(kind, u)
            dU = np.abs(p[:, 0] * (th - p[:, 1]))
            extra = p[:, 0] if absolute else 0.0
            S[:, 0], S[:, 2] = (dU / sn + extra) / la, (dU / sn + extra) / lb
            S[:, 1] = S[:, 0] + S[:, 2]
        else:
            _, s1, s3, l1, l2, l3 = internal(kind, u)
            top = np.abs(p[:, 0]) * p[:, 1] ** 2
            smin = np.minimum(s1, s3)                            # (phi, and with it dU/dphi on both ends, loses the smaller sine)
            S[:, 0], S[:, 3] = top / (l1 * s1 * smin), top / (l3 * s3 * smin)
            S[:, 1] = S[:, 2] = (1 + l1 / l2) * S[:, 0] + (1 + l3 / l2) * S[:, 3]
    return S


# ------------------------------------------------------------------------------------ per-atom bounds for a whole box
def box_bounds(x, L, terms, eps_u, C=None):
    """Per-atom bounds on the errors of a box's bonded outputs under the rounding model: (forces (N,), energies / virials /
    tensor components (N,)).  x: the positions the engine holds (N, 3), float64.  A term whose chained minimum images wrap
    around the box takes its vectors from differences of coordinates of size L, rounded at u L: its u is scaled by
    1 + L / (its shortest bond vector)."""
    C = C_BOUND if C is None else C
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    Lv = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    bf, bw = np.zeros(N), np.zeros(N)
    for kind, atoms, params in terms:
        nat = br.ATOMS[kind]
        atoms = np.asarray(atoms).reshape(-1, nat)
        n = len(atoms)
        p = np.zeros((n, 3))
        pp = np.asarray(params, dtype=np.float64).reshape(n, -1)
        p[:, :pp.shape[1]] = pp
        u = np.zeros((n, 4, 3))
        raw = np.zeros((n, nat - 1, 3))
        for a in range(1, nat):
            raw[:, a - 1] = x[atoms[:, a]] - x[atoms[:, a - 1]]
            u[:, a] = u[:, a - 1] + raw[:, a - 1] - Lv * np.round(raw[:, a - 1] / Lv)
        steps = np.linalg.norm(np.diff(u[:, :nat], axis=1), axis=2)
        wrapped = (np.abs(raw) > 0.5 * Lv).any(axis=(1, 2))
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = 1.0 + wrapped * Lv.max() / steps.min(axis=1)
        S = error_scales(kind, u, p)[:, :nat]
        S = np.where(np.isfinite(S), S, 0.0)                     # (an exactly singular term: zero force by contract, no rounding)
        scale = np.where(np.isfinite(scale), scale, 1.0)
        U = np.abs(reference(kind, u, p)[0])
        W = (np.linalg.norm(u[:, :nat], axis=2) * S).sum(axis=1)
        for a in range(nat):
            np.add.at(bf, atoms[:, a], C * eps_u * scale * S[:, a])
            np.add.at(bw, atoms[:, a], C * eps_u * scale * (U + 2.0 * W) / nat)
    return bf, bw


def entries_per_atom(N, terms):
    """how many term entries each atom owns (k_bonded's loop count)"""
    count = np.zeros(N, dtype=int)
    for kind, atoms, _ in terms:
        np.add.at(count, np.asarray(atoms).ravel(), 1)
    return count


# ------------------------------------------------------------------------------------ small rings and branches (sigma units)
BOND_P, ANGLE_P = (200.0, 0.95), (40.0, 1.9)
TORSION_SETS = ((1.5, 1.0, 0.0), (0.6, 3.0, np.pi), (0.9, 2.0, 0.4), (0.4, 5.0, -2.0), (0.7, 4.0, 0.0), (0.3, 6.0, np.pi))


def graph_terms(n, bonds):
    """every angle (i, j, k: j bonded to both, i < k) and every torsion path (i, j, k, l along three bonds, four different
    atoms, each path once) of a bond graph"""
    nb = [[] for _ in range(n)]
    for i, j in bonds:
        nb[i].append(j)
        nb[j].append(i)
    angles = [(i, j, k) for j in range(n) for i in nb[j] for k in nb[j] if i < k]
    tors = [(i, j, k, l) for j, k in [tuple(b) for b in bonds] + [tuple(b[::-1]) for b in bonds] if j < k
            for i in nb[j] if i != k for l in nb[k] if l != j and l != i]
    return np.array(angles).reshape(-1, 3), np.array(tors).reshape(-1, 4)


def _polygon(n, pucker):
    R = 1.0 / (2.0 * np.sin(np.pi / n))
    t = 2.0 * np.pi * np.arange(n) / n
    return np.stack([R * np.cos(t), R * np.sin(t), pucker * (-1.0) ** np.arange(n)], axis=1)


def molecules():
    """name -> (positions (n, 3), bonds, angles, torsions (m, 4), torsion parameters (m, 3)).  Rings of 3 (with a tail atom, so
    that it has torsions), 4 (every torsion's end atoms are bonded to each other), 5 and 6 atoms with all their angles and
    torsions; a centre with four neighbours, one of them carrying a tail: its six angles and the torsions through it; an
    improper-style torsion, the centre first, whose chain 1-2, 2-3 has no bonds; a chain with three torsion terms on its one
    quadruple."""
    rng = np.random.default_rng(21)
    out = {}

    def add(name, pos, bonds, tors=None, repeat=1):
        pos = np.asarray(pos, dtype=np.float64) + rng.uniform(-0.06, 0.06, (len(pos), 3))
        angles, paths = graph_terms(len(pos), bonds)
        tors = paths if tors is None else np.asarray(tors)
        tors = np.concatenate([tors] * repeat)
        tp = np.array([TORSION_SETS[t % len(TORSION_SETS)] for t in range(len(tors))]).reshape(-1, 3)
        out[name] = (pos, np.asarray(bonds), angles, tors, tp)

    ring = lambda n: [(i, (i + 1) % n) for i in range(n)]
    out_of_ring = np.array([[1.45, 0.0, 0.3]])
    add("ring3", np.concatenate([_polygon(3, 0.0), out_of_ring]), ring(3) + [(0, 3)])
    add("ring4", _polygon(4, 0.12), ring(4))
    add("ring5", _polygon(5, 0.1), ring(5))
    add("ring6", _polygon(6, 0.15), ring(6), repeat=2)
    tet = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]) / np.sqrt(3.0)
    add("star", np.concatenate([[(0, 0, 0)], tet, [tet[3] + (0.2, -0.9, 0.3)]]), [(0, 1), (0, 2), (0, 3), (0, 4), (4, 5)])
    tri = [(np.cos(t), np.sin(t), 0.25) for t in (0.0, 2.1, 4.2)]
    add("improper", [(0, 0, 0)] + tri, [(0, 1), (0, 2), (0, 3)], tors=[(0, 1, 2, 3), (0, 2, 3, 1)])
    add("chain3", [(0, 0, 0), (0.9, 0.3, 0), (1.3, 1.1, 0.2), (2.1, 1.3, 0.9)], [(0, 1), (1, 2), (2, 3)], repeat=3)
    return out


def assemble(placed, L):
    """placed: list of (unwrapped positions (n, 3), bonds, angles, torsions, torsion parameters) -> wrapped positions (N, 3), the
    three term tables with BOND_P / ANGLE_P, every intramolecular pair (the exclusions), the first atom of each molecule"""
    pos, B, A, T, TP, X, first = [], [], [], [], [], [], []
    at = 0
    for x, bonds, angles, tors, tp in placed:
        n = len(x)
        first.append(at)
        pos.append(x)
        B.append(np.asarray(bonds).reshape(-1, 2) + at)
        A.append(np.asarray(angles).reshape(-1, 3) + at)
        T.append(np.asarray(tors).reshape(-1, 4) + at)
        TP.append(np.asarray(tp, dtype=np.float64).reshape(-1, 3))
        X.append(np.array([(i, j) for i in range(n) for j in range(i + 1, n)]).reshape(-1, 2) + at)
        at += n
    B, A, T, TP, X = (np.concatenate(t) for t in (B, A, T, TP, X))
    terms = [(br.BOND, B, np.tile(BOND_P, (len(B), 1))), (br.ANGLE, A, np.tile(ANGLE_P, (len(A), 1))), (br.TORSION, T, TP)]
    return np.mod(np.concatenate(pos), L), terms, X, np.array(first)


def ring_box(copies=6, cells=3, cell=3.0, seed=22):
    """copies of every molecule of molecules(), each in a random orientation, on the sites of a grid that puts them across the
    box faces and the faces of the cells (cells per side, each of `cell`): sites at multiples of L / 4 starting at 0."""
    rng = np.random.default_rng(seed)
    L = cells * cell
    lib = molecules()
    sites = np.stack(np.meshgrid(*[np.arange(4) * L / 4] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    assert copies * len(lib) <= len(sites)
    sites = sites[rng.permutation(len(sites))]
    placed, names = [], []
    for c in range(copies):
        for name, (x, bonds, angles, tors, tp) in lib.items():
            R = frames(rng, 1)[0]
            site = sites[len(placed)] + rng.uniform(-0.2, 0.2, 3)
            placed.append(((x - x.mean(axis=0)) @ R + site, bonds, angles, tors, tp))
            names.append(name)
    pos, terms, excl, first = assemble(placed, L)
    return dict(positions=pos, L=L, terms=terms, exclusions=excl, first=first, names=names)


# ------------------------------------------------------------------------------------ singular molecules on the device
def singular_box(dtype, frames_per_point=4, seed=23):
    """Three- and four-atom molecules in one box of side 24 (sigma units), one per site of a grid of spacing 3, none across a
    face: the exactly singular cases (atoms along an axis on representable coordinates: straight angles with theta0 = 1.9 and
    pi, a folded one, torsions collinear on either side and on both, a coincident bond with r0 > 0 and r0 = 0), then the
    near-singular sweep: theta = pi - 10^-j and 10^-j for angles (theta0 = 1.9 and pi) and for a torsion's theta_1 and theta_3.
    Returns positions, L, terms, exclusions (every intramolecular pair) and the atoms of the exactly singular terms.  The
    angle terms carry their own theta0 and k."""
    rng = np.random.default_rng(seed)
    j_max = 7 if np.dtype(dtype) == np.float32 else 14
    mols = []                                                    # (positions, kind, params)
    for theta0 in (1.9, np.pi):
        for k in (50.0, 1e4):
            mols.append(([(-1, 0, 0), (0, 0, 0), (0.5, 0, 0)], br.ANGLE, (k, theta0, 0.0), True))
    mols.append(([(0, 1, 0), (0, 0, 0), (0, 0.5, 0)], br.ANGLE, (500.0, 1.9, 0.0), True))                     # folded
    mols.append(([(0, 0, -1), (0, 0, 0), (0, 0, 1), (0.5, 0.5, 1.25)], br.TORSION, (40.0, 1.0, 0.0), True))  # b1 || b2
    mols.append(([(0, 1, 0), (0, 0, 0), (1, 0, 0), (1.75, 0, 0)], br.TORSION, (1e4, 3.0, 0.4), True))         # b2 || b3
    mols.append(([(-0.75, 0, 0), (0, 0, 0), (0.75, 0, 0), (1.5, 0, 0)], br.TORSION, (1e6, 2.0, np.pi), True))  # both
    mols.append(([(0.25, 0.5, 0), (0.25, 0.5, 0)], br.BOND, (1e4, 0.75, 0.0), True))
    mols.append(([(0.5, 0.25, 0), (0.5, 0.25, 0)], br.BOND, (1e4, 0.0, 0.0), True))
    n_exact = len(mols)
    near = np.concatenate([np.pi - 10.0 ** -np.arange(1, j_max + 1), 10.0 ** -np.arange(1, j_max + 1)])
    for th in np.repeat(near, frames_per_point):
        R = frames(rng, 1)
        la, lb, lc = rng.uniform(0.4, 0.85, 3)                  # (a stretched torsion stays inside rc + skin = 2.8)
        for theta0 in (1.9, np.pi):
            mols.append((angle_geometry([th], [la], [lb], R)[0, :3], br.ANGLE, (rng.uniform(10, 500), theta0, 0.0), False))
        other, phi = rng.uniform(0.6, 2.5), rng.uniform(-np.pi, np.pi)
        tp = (rng.uniform(1, 40), float(rng.integers(1, 4)), rng.uniform(-3, 3))
        mols.append((torsion_geometry([th], [other], [phi], [la], [lb], [lc], R)[0], br.TORSION, tp, False))
        mols.append((torsion_geometry([other], [th], [phi], [la], [lb], [lc], R)[0], br.TORSION, tp, False))
    side = 8
    assert len(mols) <= side ** 3
    L = 3.0 * side
    pos, tabs, excl, exact_atoms, at = [], {1: ([], []), 2: ([], []), 3: ([], [])}, [], [], 0
    for s, (x, kind, p, exact) in enumerate(mols):
        x = np.asarray(x, dtype=np.float64)
        site = 3.0 * np.array([s // (side * side), (s // side) % side, s % side]) + 1.5
        if not exact:
            x = x - 0.5 * (x.max(axis=0) + x.min(axis=0))
        assert np.abs(x).max() <= 2.0 or exact
        pos.append(x + site)
        n = len(x)
        tabs[kind][0].append(np.arange(at, at + n))
        tabs[kind][1].append(p)
        excl += [(at + i, at + j) for i in range(n) for j in range(i + 1, n)]
        if exact:
            exact_atoms += list(range(at, at + n))
        at += n
    terms = [(kind, np.array(tabs[kind][0]), np.array(tabs[kind][1])[:, :3 if kind == br.TORSION else 2]) for kind in (1, 2, 3)]
    pos = np.concatenate(pos)
    assert pos.min() > 0 and pos.max() < L
    return dict(positions=pos, L=L, terms=terms, exclusions=np.array(excl), exact_atoms=np.array(exact_atoms), n_exact=n_exact)


# ------------------------------------------------------------------------------------ the fixture's solute in flexible water
def solute_box(E, xml, cells=6, pucker=False, tight=0.16, corner=True):
    """Dibenzo-p-dioxin in flexible water as examples/minimize_solute.py builds it (the solute flat from ideal hexagons in a
    lattice of water, the waters within `tight` of it left out), with the full topology of ingest.topology and no constraint
    tables.  pucker: a fixed out-of-plane pattern of 0.01 - 0.03 nm on the solute, so that no term sits at its minimum.
    corner: the box translated so that the centre of the middle ring lies on the box corner (the solute wraps across all three
    faces; its plane is tilted out of the xy plane first, or one face would cut no bond).  nm, kJ/mol, atomic mass units."""
    ing = E.ingest
    table, templates, nonbonded = ing.BondedTable(xml), ing.ResidueTemplates(xml), ing.NonbondedTable(xml)
    s, r_ch = table.bond("ca", "ca")[0][1], table.bond("ca", "ha")[0][1]
    h = 0.5 * np.sqrt(3.0) * s
    ring = {"C5": (-h, 0.5 * s), "C4": (-h, -0.5 * s), "O1": (0.0, s), "O2": (0.0, -s), "C7": (h, 0.5 * s), "C12": (h, -0.5 * s),
            "C3": (-2 * h, -s), "C2": (-3 * h, -0.5 * s), "C1": (-3 * h, 0.5 * s), "C6": (-2 * h, s),
            "C8": (2 * h, s), "C9": (3 * h, 0.5 * s), "C10": (3 * h, -0.5 * s), "C11": (2 * h, -s)}
    for name, carbon in (("H1", "C1"), ("H2", "C2"), ("H3", "C3"), ("H4", "C6"), ("H5", "C8"), ("H6", "C9"), ("H7", "C10"), ("H8", "C11")):
        c = np.array(ring[carbon])
        out = c - np.array([-2 * h if c[0] < 0 else 2 * h, 0.0])
        ring[name] = tuple(c + r_ch * out / np.linalg.norm(out))
    names = templates.residues["aaa"]["names"]
    solute = np.array([[ring[n][0], ring[n][1], 0.0] for n in names])
    if pucker:
        k = np.arange(len(names))
        solute[:, 2] = (0.01 + 0.02 * ((7 * k) % 5) / 4.0) * (-1.0) ** k
    tilt = np.linalg.qr(np.array([[1.0, 0.3, 0.2], [-0.2, 1.0, 0.4], [0.1, -0.3, 1.0]]))[0]
    solute = solute @ tilt.T
    w = E.synthetic.water_box(cells)
    L = w["L"]
    solute = solute + 0.5 * L
    water = w["positions"].reshape(-1, 3, 3)
    ow = templates.residues["HOH"]["types"].index("OW")
    d = water[:, ow, None, :] - solute[None, :, :]
    d -= L * np.rint(d / L)
    water = water[np.linalg.norm(d, axis=2).min(axis=1) >= tight]
    sequence = ["aaa"] + ["HOH"] * len(water)
    types, bonds = templates.build(sequence)
    pos = np.concatenate([solute, water.reshape(-1, 3)])
    if corner:
        pos = pos - 0.5 * L
    pos = np.mod(pos, L)
    top = ing.topology(types, bonds, table)
    terms = [(br.BOND, top["bonds"], top["bond_params"]), (br.ANGLE, top["angles"], top["angle_params"]),
             (br.TORSION, top["torsions"], top["torsion_params"])]
    mass = np.array([table.masses[t] for t in types])
    return dict(positions=pos, L=L, terms=terms, exclusions=top["exclusions"], pairs14=top["pairs14"], lj14scale=nonbonded.lj14scale,
                atoms=nonbonded.lj_atoms(types), inv_mass=1.0 / mass, n_solute=len(solute), n_water=len(water))


def long_chain_box(copies=8, seed=24):
    """Four-atom chains longer than half the box, in the smallest box the engine takes for rc + skin = 2.8 (two cells: L = 5.9):
    bonds of 1.25, angles near 165 degrees, so that the ends are 3.6 apart along the bonds and 2.3 apart through the periodic
    boundary.  Every partner is inside rc + skin of its owner (the ends through their nearer image), and the term's geometry
    is the one chained along its bonds, not the minimum images against its first atom.  Filled up with a lattice of free atoms."""
    rng = np.random.default_rng(seed)
    L = 5.9
    placed = []
    for c in range(copies):
        th = rng.uniform(0.2, 0.32, 2)                           # bond-vector angles: 162 - 168 degrees between the bonds
        # along a box axis, a little off it: only there is the other image of the far end the nearer one
        R = np.linalg.qr(np.roll(np.eye(3), c % 3, axis=0) + rng.uniform(-0.05, 0.05, (3, 3)))[0][None]
        x = torsion_geometry([th[0]], [th[1]], [rng.uniform(-np.pi, np.pi)], [1.25], [1.25], [1.25], R)[0]
        bonds = [(0, 1), (1, 2), (2, 3)]
        angles, tors = graph_terms(4, bonds)
        placed.append((x + rng.uniform(0, L, 3), bonds, angles, tors, [TORSION_SETS[c % len(TORSION_SETS)]]))
    pos, terms, excl, first = assemble(placed, L)
    g = (np.arange(5) + 0.5) * L / 5
    free = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return dict(positions=np.concatenate([pos, free]), L=L, terms=terms, exclusions=excl, n_chain=len(pos))
