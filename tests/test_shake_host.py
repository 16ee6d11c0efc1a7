"""CPU tests of bonds to hydrogen at fixed lengths (include/emdee_hip.h: emdee_md_set_hbonds): the Newton / matrix position stage
and the velocity stage of emdee.jl_amd/csrc/shake.hpp and the table builder of csrc/topology.hpp through the stand-alone program
tests/c/shake_host.cpp, built with the host compiler under ASan and UBSan, against the Gauss-Seidel SHAKE / RATTLE of
tests/helpers/shake_ref.py (which does not use the Newton form); and ingest.hydrogen_clusters on the committed force-field
fixture."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import GOLDEN, ROOT
from .helpers import shake_ref as hr

ERR_INVALID = -1
XML = os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml")
N = 300


@pytest.fixture(scope="session")
def shake_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shake_host") / "shake_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "shake_host.cpp"), "-o", exe]
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
def clusters():
    """300 random clusters over n = 1, 2, 3 satellites and the three mass sets of shake_ref (every combination at least once),
    the centre of x0 at the origin (the functions take unwrapped difference vectors, and the kernels pass them so), satellites
    in random directions at distances drawn from shake_ref.D_RANGE: x0 on the constraints, x1 = x0 + a displacement of up to
    10 % of d (the cluster's shortest) per atom, random velocities.  Four sites per cluster, the unused ones zero."""
    rng = np.random.default_rng(5)
    nsat = 1 + np.arange(N) % 3
    pick = (np.arange(N) // 3) % 3
    masses = np.ones((N, 4))
    dist = np.zeros((N, 3))
    x0 = np.zeros((N, 4, 3))
    for m in range(N):
        mc, ms = hr.MASS_SETS[pick[m]]
        masses[m, 0], masses[m, 1:1 + nsat[m]] = mc, ms
        dist[m, :nsat[m]] = rng.uniform(*hr.D_RANGE, size=nsat[m])
        u = rng.normal(size=(nsat[m], 3))
        x0[m, 1:1 + nsat[m]] = dist[m, :nsat[m], None] * u / np.linalg.norm(u, axis=1, keepdims=True)
    used = np.arange(4)[None, :] <= nsat[:, None]                                # (N, 4)
    dmin = np.where(dist > 0, dist, np.inf).min(axis=1)
    step = rng.normal(size=(N, 4, 3))
    step *= (rng.uniform(0.0, 0.1, (N, 4, 1)) * dmin[:, None, None]) / np.linalg.norm(step, axis=2, keepdims=True)
    step *= used[:, :, None]
    v = rng.normal(size=(N, 4, 3)) * used[:, :, None]
    ids = np.where(used, np.arange(4 * N).reshape(N, 4), -1)
    return dict(nsat=nsat, masses=masses, mass=masses.reshape(-1), dist=dist, dmin=dmin, used=used, x0=x0.reshape(-1, 3),
                x1=(x0 + step).reshape(-1, 3), v=v.reshape(-1, 3), pairs=hr.cluster_pairs(ids, dist))


def _run_positions(shake_host, C, x0, x1, rows=None):
    rows = range(N) if rows is None else rows
    case = ["positions", len(rows)]
    for m in rows:
        case += [int(C["nsat"][m])] + _num(C["masses"][m]) + _num(C["dist"][m]) + _num(x0[4 * m:4 * m + 4]) + _num(x1[4 * m:4 * m + 4])
    out = [line.split() for line in shake_host(case).splitlines()]
    assert len(out) == len(rows)
    return (np.array([int(r[0]) for r in out]), np.array([int(r[1]) for r in out]),
            np.array([[float(t) for t in r[2:]] for r in out]).reshape(-1, 3))


@pytest.fixture(scope="session")
def shaken(shake_host, clusters):
    ok, steps, x = _run_positions(shake_host, clusters, clusters["x0"], clusters["x1"])
    assert ok.all()
    print("Newton steps: at most %d (mean %.2f) over %d clusters" % (steps.max(), steps.mean(), N))
    assert steps.max() <= 8                                                      # (quadratic convergence; the cap is 32)
    return x


def test_positions_agree_with_gauss_seidel_shake(clusters, shaken):
    C = clusters
    want = hr.shake(C["x0"], C["x1"], C["pairs"], C["mass"])
    assert hr.residual(want, C["pairs"]) <= 2e-15                                # (the reference is converged)
    err = np.linalg.norm(shaken - want, axis=1).reshape(-1, 4).max(axis=1) / C["dmin"]
    print("largest |x - x_shake| / d = %.3e" % err.max())
    assert err.max() <= 1e-12
    assert np.array_equal(shaken.reshape(-1, 4, 3)[~C["used"]], np.zeros(((~C["used"]).sum(), 3)))      # (unused sites untouched)


def test_distances_are_restored_and_the_centre_of_mass_stays(clusters, shaken):
    C = clusters
    res = hr.residual(shaken, C["pairs"])
    print("largest relative distance error %.3e" % res)
    assert res <= 1e-12
    # sum m dx = 0 to 1e-14 m |dx|, m the cluster's mass and |dx| its largest correction: the bound of test_settle_host -- plus
    # what that bound leaves out there because a triangle's corrections are never small: dx is read off stored coordinates, each
    # rounded once at eps |x_k| / 2 per component whatever the size of the correction, which carries up to eps sum_k m_k |x_k|.
    # A cluster of two whose displacement happens to lie across its bond is corrected by 1e-4 d, and a satellite of mass 19 sits
    # at |x| = d from the origin: there the second term is the larger one (3 clusters of the 300 exceed the first alone, by up
    # to 5.2; against the sum the worst figure is 0.34).
    eps = float(np.finfo(np.float64).eps)
    dx = (shaken - C["x1"]).reshape(-1, 4, 3)
    m = C["masses"] * C["used"]
    moved = np.linalg.norm((m[:, :, None] * dx).sum(axis=1), axis=1)
    scale = m.sum(axis=1) * np.linalg.norm(dx, axis=2).max(axis=1)
    floor = eps * (m * np.linalg.norm(shaken.reshape(-1, 4, 3), axis=2)).sum(axis=1)
    print("largest |sum m dx| / (m max |dx|) = %.3e; / (1e-14 m max |dx| + eps sum m |x|) = %.3e"
          % ((moved / scale).max(), (moved / (1e-14 * scale + floor)).max()))
    assert (moved <= 1e-14 * scale + floor).all()


def test_velocity_stage_removes_the_bond_components_and_agrees_with_gauss_seidel_rattle(shake_host, clusters, shaken):
    C = clusters
    case = ["velocities", N]
    for m in range(N):
        case += [int(C["nsat"][m])] + _num(C["masses"][m]) + _num(shaken[4 * m:4 * m + 4]) + _num(C["v"][4 * m:4 * m + 4])
    rows = [line.split() for line in shake_host(case).splitlines()]
    assert len(rows) == N and all(r[0] == "v" for r in rows)
    got = np.array([[float(t) for t in r[1:]] for r in rows]).reshape(-1, 3)
    speed = np.linalg.norm(C["v"], axis=1).reshape(-1, 4).max(axis=1)            # |v|: the cluster's largest speed going in
    i, j = C["pairs"][:, 0].astype(int), C["pairs"][:, 1].astype(int)
    r, dv = shaken[i] - shaken[j], got[i] - got[j]
    left = np.abs(np.einsum("ij,ij->i", r, dv)) / (np.linalg.norm(r, axis=1) * speed[i // 4])
    print("largest |(v_c - v_k) . (x_c - x_k)| / (|v| d) = %.3e" % left.max())
    assert left.max() <= 1e-14
    want = hr.rattle(shaken, C["v"], C["pairs"], C["mass"])
    err = np.linalg.norm(got - want, axis=1).reshape(-1, 4).max(axis=1) / speed
    print("largest |v - v_rattle| / |v| = %.3e" % err.max())
    assert err.max() <= 1e-12
    # the corrections carry no momentum, and the unused sites are untouched
    dp = (C["mass"][:, None] * (got - C["v"])).reshape(-1, 4, 3).sum(axis=1)
    assert np.abs(dp).max() <= 1e-13 * (C["masses"].max() * speed.max())
    assert np.array_equal(got.reshape(-1, 4, 3)[~C["used"]], np.zeros(((~C["used"]).sum(), 3)))


def test_a_satellite_without_a_solution_is_reported_not_solved(shake_host, clusters):
    # A satellite displaced perpendicular to its bond by 1.5 d: its own correction runs along the bond of x0 and cannot bring it
    # within d.  With further satellites the centre also moves along their bonds, by at most 2 d w_c / (w_c + w_k) each while
    # their own distances hold: 0.16 d for the heavy centres (12 and 14 against 1.008), far from the 0.5 d needed, so no lambda
    # exists for n = 1, 2, 3 there; for the inverted masses (1 against 19) that figure is 1.9 d and a solution may exist, so of
    # that set only n = 1 is taken (no other bond to move along).
    C = clusters
    x1 = C["x0"].copy()
    rows = list(range(7))                                                        # (n = 1, 2, 3 of two mass sets; n = 1 of the inverted one)
    for m in rows:
        bond = C["x0"][4 * m + 1] - C["x0"][4 * m]
        perp = np.cross(bond, [0.3, -0.5, 0.8])
        x1[4 * m + 1] += 1.5 * C["dist"][m, 0] * perp / np.linalg.norm(perp)
    ok, steps, x = _run_positions(shake_host, C, C["x0"], x1, rows + [9, 10])
    assert not ok[:7].any() and ok[7:].all()
    assert np.isfinite(x).all()
    assert np.array_equal(x[:28], x1[:28])                                       # (left as it is)
    # a bond of length zero in x0 (a singular Jacobian) and a NaN: refused, no NaN made up, no sanitizer report
    case = ["positions", 2, 1, 12.0, 1.008, 1.0, 1.0, 0.3, 0.0, 0.0] + ["0.0"] * 12 + _num(C["x1"][:4])
    case += [1, 12.0, 1.008, 1.0, 1.0, 0.3, 0.0, 0.0] + _num(C["x0"][:4]) + ["nan"] + _num(C["x1"][:4])[1:]
    out = [line.split() for line in shake_host(case).splitlines()]
    assert [r[0] for r in out] == ["0", "0"]
    assert out[0][2:] == [t for t in ("%.17g" % float(s) for s in _num(C["x1"][:4]))]


def _table(shake_host, lim, ids, dist, rigid=()):
    ids, dist = np.asarray(ids).reshape(-1, 4), np.asarray(dist, dtype=np.float64).reshape(-1, 3)
    return shake_host(["table", lim, ids.shape[0]] + [int(t) for t in ids.ravel()] + _num(dist) + [len(rigid)] + [int(t) for t in rigid])


def test_table_builder_refusals_and_a_table_that_passes(shake_host):
    good_ids, good_dist = [[3, 4, -1, -1], [0, 1, 2, -1], [8, 7, 6, 5]], [[0.3, np.nan, -1.0], [0.3, 0.31, 0.0], [0.3, 0.31, 0.32]]
    out = _table(shake_host, 12, good_ids, good_dist, rigid=[9, 10, 11]).splitlines()
    assert out[0] == "table 3 ids 3 4 -1 -1 0 1 2 -1 8 7 6 5"
    assert out[1] == "hbonds cluster 0 (atoms 3 4): message"
    assert [float(t) for t in out[2].split()[1:]] == [0.3, 0.0, 0.0, 0.3, 0.31, 0.0, 0.3, 0.31, 0.32]    # (unused slots: ignored, stored as 0)
    assert _table(shake_host, 9, [], []).splitlines()[0] == "table 0 ids"
    d = [[0.3, 0.3, 0.3]]
    refused = {
        "id out of range (high)": ([[3, 4, 9, -1]], d, (), "outside"),
        "centre out of range (negative)": ([[-1, 4, 5, -1]], d, (), "outside"),
        "id out of range (below -1)": ([[3, 4, -2, -1]], d, (), "outside"),
        "empty cluster": ([[3, -1, -1, -1]], d, (), "empty"),
        "an id after a -1": ([[3, 4, -1, 5]], d, (), "after a -1"),
        "twice within a cluster": ([[3, 4, 3, -1]], d, (), "twice"),
        "twice across clusters": ([[3, 4, 5, -1], [0, 1, 4, -1]], d * 2, (), "twice"),
        "named by the rigid table": ([[3, 4, 5, -1]], d, (6, 5, 7), "rigid table"),
        "zero distance": ([[3, 4, 5, -1]], [[0.3, 0.0, 0.3]], (), "finite"),
        "negative distance": ([[3, 4, 5, -1]], [[-0.3, 0.3, 0.3]], (), "finite"),
        "nan distance": ([[3, 4, 5, 6]], [[0.3, 0.3, float("nan")]], (), "finite"),
        "infinite distance": ([[3, 4, 5, -1]], [[0.3, float("inf"), 0.3]], (), "finite"),
    }
    for name, (ids, dist, rigid, word) in refused.items():
        out = _table(shake_host, 9, ids, dist, rigid)
        assert out.startswith("REFUSED %d " % ERR_INVALID) and word in out, (name, out)
    # the mirror check of the rigid builder against an hbonds table in force
    rigid = lambda hb: shake_host(["rigid", 9, 1, 0, 1, 2, 0.32, 0.5, len(hb)] + list(hb))
    assert rigid([3, 4, -1, -1]).startswith("table 1")
    out = rigid([3, 2, -1, -1])
    assert out.startswith("REFUSED %d " % ERR_INVALID) and "hbonds table" in out, out


def test_hydrogen_clusters_finds_the_bonds_to_hydrogen_of_the_fixture(emdee):
    ingest = emdee.ingest
    t, r = ingest.BondedTable(XML), ingest.ResidueTemplates(XML)
    assert t.elements["ha"] == "H" and t.elements["HW"] == "H" and t.elements["ca"] == "C"
    types, bonds = r.build(["HOH", "aaa", "HOH"])
    waters = ingest.rigid_triatomics(types, bonds, t)[0]
    atoms, dist, drop = ingest.hydrogen_clusters(types, bonds, t, skip=waters.ravel(), with_dropped=True)
    assert atoms.shape == (8, 4) and (atoms[:, 2:] == -1).all()                  # eight clusters of two for the solute, none for the waters
    assert all(types[c] == "ca" and types[h] == "ha" for c, h in atoms[:, :2])
    assert not set(atoms[:, :2].ravel().tolist()) & set(waters.ravel().tolist())
    (_, r0), = t.bond("ca", "ha")
    assert r0 == 0.108599998                                                     # (the file's entry: 0.1086 as the file rounds it)
    assert np.array_equal(dist, np.tile([r0, 0.0, 0.0], (8, 1)))
    assert drop.tolist() == sorted([min(c, h), max(c, h)] for c, h in atoms[:, :2].tolist())
    assert all(b in ingest.topology(types, bonds, t)["bonds"].tolist() for b in drop.tolist())
    two = ingest.hydrogen_clusters(types, bonds, t, skip=waters.ravel())
    assert len(two) == 2 and np.array_equal(two[0], atoms)
    assert np.array_equal(ingest.hydrogen_clusters(types, bonds, t, length_unit=0.1, skip=waters.ravel())[1][:, 0], np.full(8, r0 / 0.1))
    # without the skip the waters are clusters of three atoms (O with two H)
    assert ingest.hydrogen_clusters(types, bonds, t)[0].shape == (10, 4)
    # XH2, XH3, the refusals
    a, d = ingest.hydrogen_clusters(["ca", "ha", "ha", "ha", "ca", "ha"], [(0, 1), (0, 3), (2, 0), (0, 4), (4, 5)], t)
    assert a.tolist() == [[0, 1, 2, 3], [4, 5, -1, -1]] and d[0].tolist() == [r0] * 3
    with pytest.raises(KeyError):
        ingest.hydrogen_clusters(["os", "ha"], [(0, 1)], t)                      # no os-ha bond entry
    with pytest.raises(ValueError):
        ingest.hydrogen_clusters(["ca", "ha", "ca"], [(0, 1), (1, 2)], t)        # a hydrogen bonded to two atoms
    with pytest.raises(ValueError):
        ingest.hydrogen_clusters(["ca", "ha", "ha", "ha", "ha"], [(0, 1), (0, 2), (0, 3), (0, 4)], t)
