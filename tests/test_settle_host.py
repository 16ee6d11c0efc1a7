"""CPU tests of rigid three-site molecules (include/emdee_hip.h: emdee_md_set_rigid3): the closed-form position and velocity stages
of emdee.jl_amd/csrc/settle.hpp and the table builder of csrc/topology.hpp through the stand-alone program tests/c/settle_host.cpp,
built with the host compiler under ASan and UBSan, against the iterative SHAKE / RATTLE of tests/helpers/settle_ref.py (which
does not use the SETTLE formulas); and ingest.rigid_triatomics on the committed force-field fixture."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import GOLDEN, ROOT
from .helpers import settle_ref as sr

ERR_INVALID = -1
XML = os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml")
N = 200
MASS_SETS, GEOMETRIES = ((16.0, 1.0, 1.0), (12.0, 3.0, 3.0)), ((0.32, 0.50), (1.0, 1.6))


@pytest.fixture(scope="session")
def settle_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("settle_host") / "settle_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "settle_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _num(v):
    return [repr(float(t)) for t in np.ravel(v)]


@pytest.fixture(scope="session")
def molecules():
    """200 random molecules over the two mass sets and the two geometries, the apex of x0 at the origin (the functions take
    unwrapped difference vectors, and the kernels pass them so): x0 on the constraints,
    x1 = x0 + a displacement of up to 10 % of d_leg per atom, random velocities"""
    rng = np.random.default_rng(5)
    pick_m, pick_g = rng.integers(0, 2, N), rng.integers(0, 2, N)
    pick_m[:4], pick_g[:4] = (0, 0, 1, 1), (0, 1, 0, 1)                          # (every combination at least once)
    masses = np.array([MASS_SETS[k] for k in pick_m])
    geom = np.array([GEOMETRIES[k] for k in pick_g])
    rot = sr.random_rotations(rng, N)
    sites = np.stack([np.einsum("ij,kj->ki", rot[m], sr.triangle(*geom[m])) for m in range(N)])
    x0 = sites                                                                   # (apex at the origin: the frame the kernels use)
    step = rng.normal(size=(N, 3, 3))
    step *= (rng.uniform(0.0, 0.1, (N, 3, 1)) * geom[:, :1, None]) / np.linalg.norm(step, axis=2, keepdims=True)
    mol = np.arange(3 * N).reshape(-1, 3)
    return dict(x0=x0.reshape(-1, 3), x1=(x0 + step).reshape(-1, 3), v=rng.normal(size=(3 * N, 3)), mol=mol, geom=geom,
                masses=masses, mass=masses.reshape(-1))


def _run_positions(settle_host, M, x0, x1):
    case = ["positions", N]
    for m in range(N):
        case += _num([M["masses"][m, 0], M["masses"][m, 1], M["geom"][m, 0], M["geom"][m, 1]]) + _num(x0[3 * m:3 * m + 3]) + _num(x1[3 * m:3 * m + 3])
    rows = [line.split() for line in settle_host(case).splitlines()]
    assert len(rows) == N
    return np.array([int(r[0]) for r in rows]), np.array([[float(t) for t in r[1:]] for r in rows]).reshape(-1, 3)


@pytest.fixture(scope="session")
def settled(settle_host, molecules):
    ok, x = _run_positions(settle_host, molecules, molecules["x0"], molecules["x1"])
    assert ok.all()
    return x


def test_positions_agree_with_iterative_shake(molecules, settled):
    M = molecules
    want = sr.shake(M["x0"], M["x1"], M["mol"], M["geom"], M["mass"])
    assert sr.residual(want, M["mol"], M["geom"]) <= 2e-15                       # (the reference is converged)
    err = np.linalg.norm(settled - want, axis=1).reshape(-1, 3).max(axis=1) / M["geom"][:, 0]
    print("largest |x - x_shake| / d_leg = %.3e" % err.max())
    assert err.max() <= 1e-10


def test_distances_are_exact_and_the_centre_of_mass_stays(molecules, settled):
    M = molecules
    res = sr.residual(settled, M["mol"], M["geom"])
    print("largest relative distance error %.3e" % res)
    assert res <= 1e-14
    # sum m dx = 0 to 1e-14 m |dx|, with m the molecule's mass and |dx| its largest correction.  (The corrections are differences
    # of positions that are rounded at eps |x|, |x| up to d_leg: against sum_i m_i |dx_i|, a few times smaller, the same figure is
    # 1.06e-14 here, and 8e-14 for the converged iterative SHAKE of the reference -- the floor of the format, printed below.)
    dx = (settled - M["x1"]).reshape(-1, 3, 3)
    moved = np.linalg.norm((M["masses"][:, :, None] * dx).sum(axis=1), axis=1)
    scale = M["masses"].sum(axis=1) * np.linalg.norm(dx, axis=2).max(axis=1)
    print("largest |sum m dx| / (m max |dx|) = %.3e; / sum m_i |dx_i| = %.3e"
          % ((moved / scale).max(), (moved / (M["masses"] * np.linalg.norm(dx, axis=2)).sum(axis=1)).max()))
    assert (moved <= 1e-14 * scale).all()


def test_velocity_stage_removes_the_bond_components_and_agrees_with_iterative_rattle(settle_host, molecules, settled):
    M = molecules
    case = ["velocities", N]
    for m in range(N):
        case += _num(M["masses"][m, :2]) + _num(settled[3 * m:3 * m + 3]) + _num(M["v"][3 * m:3 * m + 3])
    rows = [line.split() for line in settle_host(case).splitlines()]
    assert len(rows) == N and all(r[0] == "v" for r in rows)
    got = np.array([[float(t) for t in r[1:]] for r in rows]).reshape(-1, 3)
    speed = np.linalg.norm(M["v"], axis=1).reshape(-1, 3).max(axis=1)            # |v|: the molecule's largest speed going in
    after = np.linalg.norm(got, axis=1).reshape(-1, 3).max(axis=1)
    left = sr.bond_velocities(settled, got, M["mol"]) * (after / speed)[:, None]  # -> relative to the speed going in
    print("largest |(v_i - v_j) . (x_i - x_j)| / (|v| d) = %.3e" % left.max())
    assert left.max() <= 1e-14
    want = sr.rattle(settled, M["v"], M["mol"], M["mass"])
    err = np.linalg.norm(got - want, axis=1).reshape(-1, 3).max(axis=1) / speed
    print("largest |v - v_rattle| / |v| = %.3e" % err.max())
    assert err.max() <= 1e-12
    # the corrections carry no momentum
    dp = (M["mass"][:, None] * (got - M["v"])).reshape(-1, 3, 3).sum(axis=1)
    assert np.abs(dp).max() <= 1e-13 * (M["masses"].max() * speed.max())


def test_a_move_too_far_is_reported_not_solved(settle_host, molecules):
    M = molecules
    x1 = M["x1"].copy()
    for m, site in ((0, 1), (1, 0), (2, 2), (3, 1)):                             # (one of every mass set and geometry)
        x1[3 * m + site] += 3.0 * M["geom"][m, 0] * np.array([0.6, -0.48, 0.64])
    ok, x = _run_positions(settle_host, M, M["x0"], x1)
    assert not ok[:4].any() and ok[4:].all()
    assert np.isfinite(x).all()
    assert np.array_equal(x[:12], x1[:12])                                       # (left as it is)
    # a flat triangle (x0 without a plane) and a NaN: refused, no NaN made up, no sanitizer report
    case = ["positions", 2, 16.0, 1.0, 0.32, 0.5] + ["0.0"] * 9 + _num(M["x1"][:3])
    case += [16.0, 1.0, 0.32, 0.5] + _num(M["x0"][:3]) + ["nan"] + _num(M["x1"][:3])[1:]
    rows = [line.split() for line in settle_host(case).splitlines()]
    assert [r[0] for r in rows] == ["0", "0"]


def _table(settle_host, lim, ids, geom):
    ids, geom = np.asarray(ids).reshape(-1, 3), np.asarray(geom, dtype=np.float64).reshape(-1, 2)
    return settle_host(["table", lim, ids.shape[0]] + [int(t) for t in ids.ravel()] + _num(geom))


def test_table_builder_refusals_and_a_table_that_passes(settle_host):
    good_ids, good_geom = [[3, 4, 5], [0, 1, 2], [8, 7, 6]], [[0.32, 0.5], [1.0, 1.6], [1.0, 1.999]]
    out = _table(settle_host, 9, good_ids, good_geom).splitlines()
    assert out[0] == "table 3 ids 3 4 5 0 1 2 8 7 6"
    assert out[1] == "rigid molecule 0 (atoms 3 4 5): message"
    assert _table(settle_host, 9, [], []).splitlines()[0] == "table 0 ids"
    refused = {
        "id out of range (high)": ([[3, 4, 9]], [[0.32, 0.5]], "outside"),
        "id out of range (negative)": ([[-1, 4, 5]], [[0.32, 0.5]], "outside"),
        "twice within a molecule": ([[3, 4, 3]], [[0.32, 0.5]], "twice"),
        "twice across molecules": ([[3, 4, 5], [0, 1, 4]], [[0.32, 0.5]] * 2, "twice"),
        "zero distance": ([[3, 4, 5]], [[0.0, 0.5]], "finite"),
        "negative distance": ([[3, 4, 5]], [[0.32, -0.5]], "finite"),
        "nan distance": ([[3, 4, 5]], [[float("nan"), 0.5]], "finite"),
        "infinite distance": ([[3, 4, 5]], [[float("inf"), 0.5]], "finite"),
        "no triangle": ([[3, 4, 5]], [[0.25, 0.5]], "no triangle"),
        "no triangle (beyond)": ([[3, 4, 5]], [[0.2, 0.5]], "no triangle"),
    }
    for name, (ids, geom, word) in refused.items():
        out = _table(settle_host, 9, ids, geom)
        assert out.startswith("REFUSED %d " % ERR_INVALID) and word in out, (name, out)


def test_rigid_triatomics_finds_the_waters_of_the_fixture(emdee):
    ingest = emdee.ingest
    t, r = ingest.BondedTable(XML), ingest.ResidueTemplates(XML)
    types, bonds = r.build(["HOH", "aaa", "HOH"])
    n_dioxin = len(r.residues["aaa"]["types"])
    atoms, geom, drop_b, drop_a = ingest.rigid_triatomics(types, bonds, t, with_dropped=True)
    # template order is Hw1, Ow, Hw2: the centre is the second atom of each water and comes first
    assert atoms.tolist() == [[1, 0, 2], [n_dioxin + 4, n_dioxin + 3, n_dioxin + 5]]
    (_, r0), = t.bond("OW", "HW")
    (_, theta0), = t.angle("HW", "OW", "HW")
    assert r0 == 0.101199999 and theta0 == 1.97641087                           # (the file's entries)
    assert np.array_equal(geom, np.tile([r0, 2.0 * r0 * np.sin(0.5 * theta0)], (2, 1)))
    assert drop_b.tolist() == [[0, 1], [1, 2], [n_dioxin + 3, n_dioxin + 4], [n_dioxin + 4, n_dioxin + 5]]
    assert drop_a.tolist() == [[0, 1, 2], [n_dioxin + 3, n_dioxin + 4, n_dioxin + 5]]
    top = ingest.topology(types, bonds, t)
    assert all(b in top["bonds"].tolist() for b in drop_b.tolist()) and all(a in top["angles"].tolist() for a in drop_a.tolist())
    two = ingest.rigid_triatomics(types, bonds, t)
    assert len(two) == 2 and np.array_equal(two[0], atoms) and np.array_equal(two[1], geom)
    # Angstrom positions: lengths / 0.1
    assert np.allclose(ingest.rigid_triatomics(types, bonds, t, length_unit=0.1)[1], geom / 0.1, rtol=1e-15)
    # a three-atom chain whose ends differ in type, and a centre with a third neighbour, are not rigid triatomics
    assert ingest.rigid_triatomics(["HW", "OW", "OW"], [(0, 1), (1, 2)], t)[0].shape == (0, 3)
    assert ingest.rigid_triatomics(["HW", "OW", "HW", "HW"], [(0, 1), (1, 2), (1, 3)], t)[0].shape == (0, 3)
