"""CPU tests of the bonded terms' formula (include/emdee_hip.h, "bonded terms"): bonded_term of emdee.jl_amd/csrc/bonded.hpp, the
function k_bonded calls on the device, through the stand-alone program tests/c/bonded_host.cpp, built with the host compiler under
ASan and UBSan and instantiated for float and double.  The references are wider than the code under test: for float,
tests/helpers/bonded_ref.py's formulas in float64 at the float32-rounded positions and parameters; for double, the same formulas
in the x87 extended format (np.longdouble).  Generic geometries and closed forms, the approach to the singular geometries under
the rounding model of tests/helpers/ring_cases.py, and the singular geometries themselves, where the contract is zero force and
a finite energy whatever k is."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import bonded_ref as br
from .helpers import ring_cases as rc

# the reference for double needs a format wider than double: fail loudly where long double is double
assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format on this platform"

TYPES = {"float": (np.float32, np.float64, rc.U32, 7), "double": (np.float64, np.longdouble, rc.U64, 14)}   # (real, reference, u, j_max)
TINY = {"float": 1e-37, "double": 1e-300}
FRAMES = 1000


@pytest.fixture(scope="session")
def bonded_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bonded_host") / "bonded_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "bonded_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(name, kind, u, p):
        """kind: one kind or one per term; u (n, 4, 3) and p (n, 3) in the real type of `name` -> U (n,), F (n, 4, 3) in float64
        (exact: every float and double prints and reads back as itself)"""
        real = TYPES[name][0]
        u, p = np.asarray(u), np.asarray(p)
        assert u.dtype == real and p.dtype == real and u.shape[1:] == (4, 3) and p.shape == (u.shape[0], 3)
        n = u.shape[0]
        rows = np.concatenate([u.reshape(n, 12), p], axis=1).astype(np.float64)
        kinds = np.broadcast_to(kind, (n,))
        text = "%s %d\n" % (name, n) + "\n".join("%d " % k + " ".join(map(repr, row)) for k, row in zip(kinds, rows.tolist())) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]          # (a sanitizer report goes to stderr and aborts)
        out = np.array([line.split() for line in r.stdout.splitlines()], dtype=np.float64).reshape(n, 13)
        return out[:, 0], out[:, 1:].reshape(n, 4, 3)
    return run


def _errors(bonded_host, name, kind, u, p):
    """run the program on u, p rounded to the real type; -> (U, F, reference U, reference F, |F - F_ref| per atom (n, 4), the
    rounded u and p as float64)"""
    real, wide, _, _ = TYPES[name]
    ur, pr = np.asarray(u).astype(real), np.asarray(p).astype(real)
    U, F = bonded_host(name, kind, ur, pr)
    Ur, Fr = rc.reference(kind, ur, pr, wide)
    err = np.sqrt((((F.astype(wide) - Fr) ** 2).sum(axis=2)).astype(np.float64))
    return U, F, Ur.astype(np.float64), Fr.astype(np.float64), err, ur.astype(np.float64), pr.astype(np.float64)


def _balance(u, F):
    """|sum F| and |sum u x F| per term against sum |F| and sum |u - u_1| |F| (torques about the second atom)"""
    d = u - u[:, 1:2]
    f = np.linalg.norm(F, axis=2)
    net = np.linalg.norm(F.sum(axis=1), axis=1) / np.maximum(f.sum(axis=1), 1e-300)
    lever = (np.linalg.norm(d, axis=2) * f).sum(axis=1)
    torque = np.linalg.norm(np.cross(d, F).sum(axis=1), axis=1) / np.maximum(lever, 1e-300)
    return net.max(), torque.max()


def test_the_batched_reference_is_bonded_ref():
    rng = np.random.default_rng(11)
    n = 200
    R = rc.frames(rng, n)
    cases = [(br.BOND, rc.angle_geometry(rng.uniform(0.3, 2.8, n), rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n), R),
              np.stack([rng.uniform(1, 300, n), rng.uniform(0.5, 1.5, n), np.zeros(n)], axis=1)),
             (br.ANGLE, rc.angle_geometry(rng.uniform(0.01, 3.13, n), rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n), R),
              np.stack([rng.uniform(1, 300, n), rng.uniform(0, np.pi, n), np.zeros(n)], axis=1)),
             (br.TORSION, rc.torsion_geometry(rng.uniform(0.1, 3.0, n), rng.uniform(0.1, 3.0, n), rng.uniform(-np.pi, np.pi, n),
                                              *rng.uniform(0.5, 1.5, (3, n)), R),
              np.stack([rng.uniform(1, 40, n), rng.integers(1, 7, n).astype(float), rng.uniform(-3, 3, n)], axis=1))]
    for kind, u, p in cases:
        U, F = rc.reference(kind, u, p)
        for t in range(n):
            Ut, Ft = br.term_forces(kind, u[t, :br.ATOMS[kind]], p[t])
            assert U[t] == pytest.approx(Ut, rel=1e-13, abs=1e-13)
            assert np.abs(F[t, :br.ATOMS[kind]] - Ft).max() <= 1e-12 * max(np.abs(Ft).max(), 1.0)
            assert not F[t, br.ATOMS[kind]:].any()
    # the constructions give the internal coordinates they are asked for
    th = rng.uniform(0.01, 3.13, n)
    assert np.abs(rc.internal(br.ANGLE, rc.angle_geometry(th, np.ones(n), 2 * np.ones(n), R))[0] - th).max() < 1e-13
    phi, t1, t3 = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.2, 2.9, n), rng.uniform(0.2, 2.9, n)
    got = rc.internal(br.TORSION, rc.torsion_geometry(t1, t3, phi, np.ones(n), 2 * np.ones(n), 0.5 * np.ones(n), R))
    assert np.abs(np.angle(np.exp(1j * (got[0] - phi)))).max() < 1e-12
    assert np.abs(got[1] - np.sin(t1)).max() < 1e-13 and np.abs(got[2] - np.sin(t3)).max() < 1e-13


@pytest.mark.parametrize("name", ["float", "double"])
def test_generic_terms_match_the_wider_reference_and_the_closed_forms(bonded_host, name):
    """Random bonds, angles and torsions (n = 1 .. 6, phases 0, pi, 0.4, -2.0), all angles between 0.3 and pi - 0.3: the rounding
    model at its generic end, 1 / sin(theta) <= 3.4.  Closed forms on the reference, to its own rounding; the program's net force
    and torque vanish to rounding."""
    _, _, eps, _ = TYPES[name]
    rng = np.random.default_rng(12)
    n = 2400
    R = rc.frames(rng, n)
    o = rng.uniform(-3, 3, (n, 3))
    la, lb, lc = rng.uniform(0.1, 1.5, (3, n))
    # bonds
    u = rc.angle_geometry(np.full(n, 1.0), la, lb, R, o)
    p = np.stack([rng.uniform(1, 1000, n), rng.uniform(0.1, 1.5, n), np.zeros(n)], axis=1)
    U, F, Ur, Fr, err, ur, pr = _errors(bonded_host, name, br.BOND, u, p)
    S = rc.error_scales(br.BOND, ur, pr)
    print("%s bonds: worst err / (u S) = %.2f" % (name, (err[:, :2] / (eps * S[:, :2])).max()))
    assert (err <= rc.C_BOUND * eps * S).all() and not F[:, 2:].any()
    assert np.abs(U - Ur).max() <= rc.C_BOUND * eps * np.abs(pr[:, 0] * (la + pr[:, 1]) ** 2).max()
    net, torque = _balance(ur - o[:, None, :], F)
    assert net == 0.0 and torque <= 4 * eps                                 # (F_1 = -F_0 exactly, both along the bond)
    # angles: |F_0| = |k (theta - theta0)| / |a|, |F_2| = ... / |b|
    theta = rng.uniform(0.3, np.pi - 0.3, n)
    u = rc.angle_geometry(theta, la, lb, R, o)
    p = np.stack([rng.uniform(1, 1000, n), rng.uniform(0, np.pi, n), np.zeros(n)], axis=1)
    U, F, Ur, Fr, err, ur, pr = _errors(bonded_host, name, br.ANGLE, u, p)
    th, sn, a, b = rc.internal(br.ANGLE, ur)
    M = np.abs(pr[:, 0] * (th - pr[:, 1]))
    assert np.abs(np.linalg.norm(Fr[:, 0], axis=1) - M / a).max() <= 1e-9 * (pr[:, 0] / a).max()
    assert np.abs(np.linalg.norm(Fr[:, 2], axis=1) - M / b).max() <= 1e-9 * (pr[:, 0] / b).max()
    S = rc.error_scales(br.ANGLE, ur, pr)
    print("%s angles: worst err / (u S) = %.2f" % (name, (err[:, :3] / (eps * S[:, :3])).max()))
    assert (err <= rc.C_BOUND * eps * S).all() and not F[:, 3].any()
    assert np.abs(U - Ur).max() <= rc.C_BOUND * eps * (pr[:, 0] * np.pi ** 2).max()
    net, torque = _balance(ur - o[:, None, :], F)
    assert net <= 4 * eps and torque <= rc.C_BOUND * eps / sn.min()
    # torsions: |F_0| = |dU/dphi| / (|b1| sin theta_1), |F_3| = |dU/dphi| / (|b3| sin theta_3)
    t1, t3, phi = rng.uniform(0.3, np.pi - 0.3, n), rng.uniform(0.3, np.pi - 0.3, n), rng.uniform(-np.pi, np.pi, n)
    mult = (1 + np.arange(n) % 6).astype(float)
    phase = np.array([0.0, np.pi, 0.4, -2.0])[(np.arange(n) // 6) % 4]
    u = rc.torsion_geometry(t1, t3, phi, la, lb, lc, R, o)
    p = np.stack([rng.uniform(1, 40, n), mult, phase], axis=1)
    U, F, Ur, Fr, err, ur, pr = _errors(bonded_host, name, br.TORSION, u, p)
    ph, s1, s3, l1, l2, l3 = rc.internal(br.TORSION, ur)
    dU = np.abs(pr[:, 0] * pr[:, 1] * np.sin(pr[:, 1] * ph - pr[:, 2]))
    assert np.abs(np.linalg.norm(Fr[:, 0], axis=1) - dU / (l1 * s1)).max() <= 1e-9 * (pr[:, 0] * pr[:, 1] / (l1 * s1)).max()
    assert np.abs(np.linalg.norm(Fr[:, 3], axis=1) - dU / (l3 * s3)).max() <= 1e-9 * (pr[:, 0] * pr[:, 1] / (l3 * s3)).max()
    S = rc.error_scales(br.TORSION, ur, pr)
    print("%s torsions: worst err / (u S) = %.2f" % (name, (err / (eps * S)).max()))
    assert (err <= rc.C_BOUND * eps * S).all()
    assert np.abs(U - Ur).max() <= rc.C_BOUND * eps * (pr[:, 0] * pr[:, 1] / np.minimum(s1, s3)).max()
    net, torque = _balance(ur - o[:, None, :], F)
    assert net <= 8 * eps and torque <= rc.C_BOUND * eps / min(s1.min(), s3.min())


@pytest.mark.parametrize("name", ["float", "double"])
def test_planar_and_perpendicular_torsions(bonded_host, name):
    """phi exactly 0 (cis), exactly pi (trans) and +-pi / 2 on representable coordinates, n = 1 .. 6 and the four phases: at cis
    and trans with phase 0 or pi the force is a rounding of zero against k n; the energies tell the branches of atan2 apart."""
    real, _, eps, _ = TYPES[name]
    ends = {0.0: (1, 0, 1), np.pi: (-1, 0, 1), 0.5 * np.pi: (0, 1, 1), -0.5 * np.pi: (0, -1, 1)}
    rows, params, want_phi = [], [], []
    for phi, end in ends.items():
        for mult in range(1, 7):
            for phase in (0.0, np.pi, 0.4, -2.0):
                rows.append([(1, 0, 0), (0, 0, 0), (0, 0, 1), end])
                params.append((3.0, mult, phase))
                want_phi.append(phi)
    u, p, want_phi = 0.5 * np.array(rows, dtype=np.float64), np.array(params), np.array(want_phi)
    U, F, Ur, Fr, err, ur, pr = _errors(bonded_host, name, br.TORSION, u, p)
    assert np.abs(np.angle(np.exp(1j * (rc.internal(br.TORSION, ur)[0] - want_phi)))).max() < 1e-15
    want_U = pr[:, 0] * (1 + np.cos(pr[:, 1] * want_phi - pr[:, 2]))
    assert np.abs(U - want_U).max() <= 16 * eps * 3.0 * 6 and np.abs(Ur - want_U).max() <= 1e-14 * 18
    S = rc.error_scales(br.TORSION, ur, pr)
    assert (err <= rc.C_BOUND * eps * S).all()
    flat = np.isin(want_phi, (0.0, np.pi)) & np.isin(p[:, 2], (0.0, np.pi))
    assert (np.abs(F[flat]).max(axis=(1, 2)) <= rc.C_BOUND * eps * S[flat].max(axis=1)).all()
    assert np.abs(F[~flat]).max() > 1.0


def _sweep_angles(j_max):
    d = 10.0 ** -np.arange(1, j_max + 1)
    return np.concatenate([np.pi - d, d])


@pytest.mark.parametrize("name", ["float", "double"])
def test_near_singular_angles_stay_inside_the_rounding_model(bonded_host, name):
    """theta = pi - 10^-j and 10^-j against theta0 = 1.9 (the purely relative bound C u / sin(theta) of |k (theta - theta0)| / |arm|)
    and theta0 = pi (where the force goes to zero with pi - theta: the bound with its absolute part, C u k / |arm|), 1000 frames
    and arm pairs per point.  sin(theta) is the one of the rounded positions."""
    _, _, eps, j_max = TYPES[name]
    rng = np.random.default_rng(13)
    theta = np.repeat(_sweep_angles(j_max), FRAMES)
    n = theta.size
    u = rc.angle_geometry(theta, rng.uniform(0.1, 1.5, n), rng.uniform(0.1, 1.5, n), rc.frames(rng, n), rng.uniform(-1, 1, (n, 3)))
    worst = 0.0
    for theta0, absolute in ((1.9, False), (np.pi, True)):
        p = np.stack([rng.uniform(1, 1000, n), np.full(n, theta0), np.zeros(n)], axis=1)
        U, F, Ur, Fr, err, ur, pr = _errors(bonded_host, name, br.ANGLE, u, p)
        assert np.isfinite(F).all() and np.isfinite(U).all()
        S = rc.error_scales(br.ANGLE, ur, pr, absolute=absolute)
        live = np.isfinite(S[:, 0])                                        # (rounding may put a float case exactly on the line)
        assert live.mean() > 0.99
        ratio = err[live, :3] / (eps * S[live, :3])
        per_point = ratio.max(axis=1)[: live.size // FRAMES * FRAMES] if live.all() else None
        print("%s theta0 = %.2f: worst err / (u S) = %.2f%s" % (name, theta0, ratio.max(), "" if per_point is None else
              "; per point " + " ".join("%.1f" % t for t in per_point.reshape(-1, FRAMES).max(axis=1))))
        worst = max(worst, ratio.max())
        assert np.abs(U - Ur)[live].max() <= rc.C_BOUND * eps * (pr[:, 0] * np.pi ** 2).max()
    assert worst <= rc.C_BOUND / 4                                         # (C is 4 x the host's worst, rounded up to a power of two)


@pytest.mark.parametrize("name", ["float", "double"])
def test_near_singular_torsions_stay_inside_the_rounding_model(bonded_host, name):
    """The same sweep for a torsion's theta_1 and theta_3, the other one generic: the error of every force against
    C u / min(sin) of k n^2 / (|b| sin)."""
    _, _, eps, j_max = TYPES[name]
    rng = np.random.default_rng(14)
    near = np.repeat(_sweep_angles(j_max), FRAMES)
    n = near.size
    worst = 0.0
    for side in (1, 3):
        other = rng.uniform(0.5, np.pi - 0.5, n)
        t1, t3 = (near, other) if side == 1 else (other, near)
        u = rc.torsion_geometry(t1, t3, rng.uniform(-np.pi, np.pi, n), *rng.uniform(0.1, 1.5, (3, n)), rc.frames(rng, n),
                                rng.uniform(-1, 1, (n, 3)))
        p = np.stack([rng.uniform(1, 40, n), rng.integers(1, 4, n).astype(float), rng.uniform(-3, 3, n)], axis=1)
        U, F, Ur, Fr, err, ur, pr = _errors(bonded_host, name, br.TORSION, u, p)
        assert np.isfinite(F).all() and np.isfinite(U).all()
        S = rc.error_scales(br.TORSION, ur, pr)
        live = np.isfinite(S[:, 0]) & np.isfinite(S[:, 3])
        assert live.mean() > 0.99
        ratio = err[live] / (eps * S[live])
        print("%s theta_%d: worst err / (u S) = %.2f" % (name, side, ratio.max()))
        worst = max(worst, ratio.max())
    assert worst <= rc.C_BOUND / 4


K_VALUES = (1.0, 34.0, 40.0, 50.0, 500.0, 1e4, 1e6)


def _singular_cases():
    """(kind, atoms on the x axis, (p1, p2), what the energy is as a function of k or None for 'finite')"""
    X = lambda *x: [(t, 0.0, 0.0) for t in x] + [(0.0, 0.0, 0.0)] * (4 - len(x))
    cases = []
    for theta0 in (1.9, np.pi):
        cases.append((br.ANGLE, X(-1.0, 0.0, 1.0), (theta0, 0.0), ("straight", theta0)))
        cases.append((br.ANGLE, X(-0.125, 0.0, 0.25), (theta0, 0.0), ("straight", theta0)))
        cases.append((br.ANGLE, X(1.0, 0.0, 0.5), (theta0, 0.0), ("folded", theta0)))
    cases.append((br.ANGLE, X(-0.001, 0.0, 0.002), (1.9, 0.0), ("straight", 1.9)))           # short arms (the header's limit is 1e-4)
    Y = lambda *x: [tuple(t) for t in x]
    cases.append((br.TORSION, Y((-1, 0, 0), (0, 0, 0), (1, 0, 0), (1.5, 1, 0)), (1.0, 0.0), None))       # b1 || b2
    cases.append((br.TORSION, Y((0, 1, 0), (0, 0, 0), (1, 0, 0), (2, 0, 0)), (3.0, 0.4), None))          # b2 || b3
    cases.append((br.TORSION, Y((-1, 0, 0), (0, 0, 0), (1, 0, 0), (2, 0, 0)), (2.0, np.pi), None))       # both
    cases.append((br.TORSION, Y((2, 0, 0), (0, 0, 0), (1, 0, 0), (0.5, 0, 0)), (1.0, -2.0), None))       # both, folded back
    cases.append((br.TORSION, Y((0, 1, 0), (0.5, 0, 0), (0.5, 0, 0), (1, 0, 1)), (1.0, 0.0), None))      # b2 = 0
    cases.append((br.BOND, Y((0.25, -1, 3), (0.25, -1, 3), (0, 0, 0), (0, 0, 0)), (0.75, 0.0), ("bond", 0.75)))
    cases.append((br.BOND, Y((0.25, -1, 3), (0.25, -1, 3), (0, 0, 0), (0, 0, 0)), (0.0, 0.0), ("bond", 0.0)))
    return cases


@pytest.mark.parametrize("name", ["float", "double"])
def test_exactly_singular_geometries_give_zero_force_and_the_contracts_energy(bonded_host, name):
    """Atoms on a coordinate axis with representable coordinates, k from 1 to 1e6: every force is exactly zero; an angle's energy
    is k/2 (theta - theta0)^2 with theta = 0 or pi, a bond's k/2 r0^2, a torsion's finite.  (Guarded by x / max(den, 1e-37) alone,
    the float angles with theta0 = 1.9 come out NaN from k = 34 on -- |dU| / tiny leaves the format at |dU| = 34 -- and so do the
    torsions with k n |sin(n phi - phase)| above that; in double that guard gives a torsion collinear on one side a force.)"""
    real, _, eps, _ = TYPES[name]
    for kind, atoms, (p1, p2), energy in _singular_cases():
        u = np.tile(np.array(atoms, dtype=np.float64), (len(K_VALUES), 1, 1))
        p = np.array([(k, p1, p2) for k in K_VALUES])
        U, F = bonded_host(name, kind, u.astype(real), p.astype(real))
        assert np.array_equal(F, np.zeros_like(F)), (kind, atoms, p1, F)
        assert np.isfinite(U).all(), (kind, atoms, U)
        pr = p.astype(real).astype(np.float64)
        if energy is None:
            assert (U >= 0).all() and (U <= 2 * pr[:, 0] * (1 + 4 * eps)).all()
        elif energy[0] == "bond":
            assert np.abs(U - 0.5 * pr[:, 0] * pr[:, 1] ** 2).max() <= 4 * eps * (0.5 * pr[:, 0] * pr[:, 1] ** 2).max()
        else:
            theta = float(real(np.pi)) if energy[0] == "straight" else 0.0        # (atan2(0, -x) is pi rounded to the format)
            want = 0.5 * pr[:, 0] * (theta - pr[:, 1]) ** 2
            assert (np.abs(U - want) <= 8 * eps * want).all(), (atoms, p1, U, want)


@pytest.mark.parametrize("name", ["float", "double"])
def test_denominators_below_tiny_give_finite_bounded_forces(bonded_host, name):
    """Geometries a hair off the singular ones, down through the denormal range: what the formula divides by is anywhere between
    0 and `tiny` (or underflows to 0 on the way).  Every force component is finite; an angle's and a bond's force is at most
    (1 + C u) times its analytic magnitude.  Then offsets above that range, where the quotients are taken: a bond and an angle
    stay finite (a norm that survives the underflow of its square is at least the square root of the least denormal: the
    quotient stays far inside the format), a torsion wherever k n |b2| / |m|^2 itself stays inside the format -- the header
    says so."""
    real, wide, eps, _ = TYPES[name]
    tiny, top = TINY[name], float(np.finfo(real).max)
    least = float(np.finfo(real).smallest_subnormal)
    below = [least, 3 * least, 1e3 * least] + [tiny * 10.0 ** -e for e in (6, 4, 2, 1)] + [tiny * 0.99]
    above = [tiny * 10.0 ** e for e in (0, 1, 3, 6, 9, 12, 15, 18)] + [np.sqrt(tiny) * 10.0 ** e for e in (-2, -1, 0, 1, 3)]
    bonds, angles, torsions = [], [], []                                     # (u, p, the bound on |F| per atom or None)
    for k in K_VALUES:
        for off in below + above:
            small = off < tiny
            grow = 1 + rc.C_BOUND * eps
            # bond: two atoms `off` apart
            bonds.append(([(0, 0, 0), (0, off, 0), (0, 0, 0), (0, 0, 0)], (k, 0.75, 0.0), grow * k * 0.75 if small else None))
            # angle: a straight one with the third atom `off` to the side, and a folded one
            for x2 in (1.0, -0.5):
                M = grow * k * max(np.pi - 1.9, 1.9) / abs(x2)
                angles.append(([(-1.0, 0, 0), (0, 0, 0), (x2, off, 0), (0, 0, 0)], (k, 1.9, 0.0), M if small else None))
            # torsion: b1 and b2 (then b2 and b3) `off` from collinear: m . m (n . n) is off^2, so the square roots of the
            # offsets put that product itself anywhere below tiny
            for off2 in (off, np.sqrt(off)):
                if off2 ** 2 < tiny or 2 * k / off2 ** 2 < 1e-3 * top:
                    torsions.append(([(-1.0, off2, 0), (0, 0, 0), (1, 0, 0), (1.5, 0, 1)], (k, 1.0, 0.4), None))
                    torsions.append(([(-0.5, 0, 1), (0, 0, 0), (1, 0, 0), (2, off2, 0)], (k, 1.0, 0.4), None))
    for kind, cases in ((br.BOND, bonds), (br.ANGLE, angles), (br.TORSION, torsions)):
        u, p = np.array([c[0] for c in cases], dtype=np.float64), np.array([c[1] for c in cases])
        U, F = bonded_host(name, kind, u.astype(real), p.astype(real))
        assert np.isfinite(F).all() and np.isfinite(U).all(), (kind, u[~np.isfinite(F).all(axis=(1, 2))], p[~np.isfinite(F).all(axis=(1, 2))])
        for t, (_, _, bound) in enumerate(cases):
            if bound is not None:
                assert np.linalg.norm(F[t], axis=1).max() <= 2 * bound if kind == br.ANGLE else np.linalg.norm(F[t], axis=1).max() <= bound
