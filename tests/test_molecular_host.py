"""CPU tests of the molecular pressure and the molecular scale (include/emdee_hip.h: emdee_md_molecular_pressure_tensor,
emdee_md_set_molecular_scaling): the two per-molecule functions of emdee.jl_amd/csrc/settle.hpp and the membership builder of
csrc/topology.hpp through the stand-alone program tests/c/molecular_host.cpp, built with the host compiler under ASan and UBSan
as tests/test_settle_host.py builds its program, against tests/helpers/molecular_ref.py on that file's 200 random molecules (both
mass sets, both geometries).  Bound: the 1e-12 relative of the fp64 SETTLE host tests."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import molecular_ref as mr
from .test_settle_host import N, _num, molecules  # noqa: F401  (the fixture of the 200 molecules)

TOL = 1e-12


@pytest.fixture(scope="session")
def molecular_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("molecular_host") / "molecular_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "molecular_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


@pytest.fixture(scope="session")
def sites(molecules):
    """the molecules of test_settle_host moved to random places in a box of side 8 at lo = (-1, 0.5, 2), with forces"""
    rng = np.random.default_rng(17)
    x = molecules["x0"] + np.repeat(np.array([-1.0, 0.5, 2.0]) + 8.0 * rng.random((N, 3)), 3, axis=0)
    return dict(x=x, v=molecules["v"], f=30.0 * rng.normal(size=(3 * N, 3)))


def test_the_twelve_terms_of_every_molecule_agree_with_the_reference(molecular_host, molecules, sites):
    M, S = molecules, sites
    case = ["sums", N]
    for m in range(N):
        case += _num(M["masses"][m, :2]) + _num(S["x"][3 * m:3 * m + 3]) + _num(S["v"][3 * m:3 * m + 3]) + _num(S["f"][3 * m:3 * m + 3])
    rows = [line.split() for line in molecular_host(case).splitlines()]
    assert len(rows) == N and all(r[0] == "s" and len(r) == 13 for r in rows)
    got = np.array([[float(t) for t in r[1:]] for r in rows])
    want = np.array([np.concatenate(mr.corrections(S["x"], S["v"], S["f"], M["mol"][m:m + 1], M["mass"])) for m in range(N)])
    for name, cols in (("virial", slice(0, 6)), ("kinetic", slice(6, 12))):
        scale = np.abs(want[:, cols]).max(axis=1)
        err = (np.abs(got[:, cols] - want[:, cols]).max(axis=1) / scale).max()
        print("%s terms: largest error relative to the molecule's largest component %.3e" % (name, err))
        assert err <= TOL
    # summed over the table they are what the atomic sums hold beyond the molecular ones
    cw, ck = mr.corrections(S["x"], S["v"], S["f"], M["mol"], M["mass"])
    total = got.sum(axis=0)
    assert np.abs(total[:6] - cw).max() <= TOL * np.abs(want[:, :6]).max() * np.sqrt(N)
    assert np.abs(total[6:] - ck).max() <= TOL * np.abs(want[:, 6:]).max() * np.sqrt(N)


@pytest.mark.parametrize("vscale", [1.0, 0.5])
def test_shifts_and_velocity_increments_agree_with_the_reference(molecular_host, molecules, sites, vscale):
    M, S = molecules, sites
    mu, lo, lengths = np.array([1.013, 0.991, 1.004]), np.array([-1.0, 0.5, 2.0]), np.array([8.0, 8.0, 8.0])
    case = ["scale", N] + _num(mu) + _num(lo) + _num(vscale)
    for m in range(N):
        case += _num(M["masses"][m, :2]) + _num(S["x"][3 * m:3 * m + 3]) + _num(S["v"][3 * m:3 * m + 3])
    rows = [line.split() for line in molecular_host(case).splitlines()]
    assert len(rows) == N and all(r[0] == "c" and len(r) == 7 for r in rows)
    got = np.array([[float(t) for t in r[1:]] for r in rows])
    x, v, _ = mr.scale(S["x"], S["v"], lo, lengths, mu, M["mol"], M["mass"], vscale)
    dx, dv = (x - S["x"]).reshape(N, 3, 3), (v - S["v"]).reshape(N, 3, 3)
    assert np.abs(dx - dx[:, :1]).max() <= 1e-14 and np.abs(dv - dv[:, :1]).max() <= 1e-15     # (the reference translates molecules)
    # the shift against |mu - 1| (|Y - lo|), the velocity increment against |velocity_scale - 1| |V|: 1e-12 of either; the
    # reference's own x' - x carries the rounding of x ~ 10, so its shift is known to 1e-15 absolute only
    Y, V, _, _ = mr.centres(S["x"], S["v"], M["mol"], M["mass"])
    want = (mu - 1.0) * (Y - lo)
    assert np.abs(got[:, :3] - want).max() <= TOL * np.abs(want).max()
    assert np.abs(got[:, :3] - dx[:, 0]).max() <= 4e-15
    if vscale == 1.0:
        assert np.array_equal(got[:, 3:], np.zeros((N, 3)))
    else:
        assert np.abs(got[:, 3:] - (vscale - 1.0) * V).max() <= TOL * np.abs(V).max()
        assert np.abs(got[:, 3:] - dv[:, 0]).max() <= 4e-15


def test_membership_bytes_mark_the_atoms_of_the_table_and_no_others(molecular_host):
    out = molecular_host(["members", 11, 2, 3, 4, 5, 9, 0, 7]).split()
    assert out == ["members"] + [str(int(i in (3, 4, 5, 9, 0, 7))) for i in range(11)]
    assert molecular_host(["members", 4, 0]).split() == ["members", "0", "0", "0", "0"]
    assert molecular_host(["members", 3, 1, 0, 1, 3]).startswith("REFUSED -1 ")               # (the builder checks the table first)
