"""CPU tests of the Ewald sum: the numpy/scipy reference tests/helpers/ewald_ref.py against known results (the Madelung constant
of rock salt, the independence of the sum of its splitting parameter), and the host side of emdee_md_set_ewald
(emdee.jl_amd/csrc/topology.hpp: the argument checks, the wave vectors, A(k)) through the stand-alone program
tests/c/ewald_host.cpp, built with the host compiler under ASan and UBSan, against that reference."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import ewald_ref as er

ERR_INVALID = -1


def test_reference_gives_the_madelung_constant_of_rock_salt():
    pos, L, q = er.rock_salt(8)
    f, e, w, t = er.ewald(pos, L, q, 1.0, 1.5, 18, 3.0)
    madelung = -2.0 * e.sum() / pos.shape[0]
    print("Madelung error", madelung - er.MADELUNG_NACL)
    assert abs(madelung - er.MADELUNG_NACL) < 1e-8
    assert np.abs(f).max() < 1e-10                                     # every ion sits on a centre of symmetry


def test_reference_does_not_depend_on_alpha():
    pos, L, q = er.random_charges()
    assert abs(q.sum()) < 1e-12
    a = er.ewald(pos, L, q, 1.0, 1.5, 22, 3.3)
    b = er.ewald(pos, L, q, 1.0, 1.7, 25, 3.3)
    de = abs(a[1].sum() - b[1].sum()) / abs(a[1].sum())
    df = np.abs(a[0] - b[0]).max() / np.abs(a[0]).max()
    print("energy", de, "forces", df)
    assert de <= 1e-10 and df <= 1e-10


def test_reference_virial_is_the_trace_of_its_tensor_and_the_volume_derivative_of_its_energy():
    pos, L, q = er.random_charges(n=60, L=(5.0, 5.5, 6.0), seed=2, total=1.5)
    args = (1.0, 1.6, 14, 2.4)
    f, e, w, t = er.ewald(pos, L, q, *args)
    assert np.abs(t[:, :3].sum(axis=1) - w).max() <= 1e-12 * np.abs(w).max()
    # -dE/dmu at mu = 1, all sides scaled alike, by a central difference: truncation h^2 |E'''| / 6 ~ 1e-8 relative at h = 1e-4
    h = 1e-4
    dE = (er.energy(pos * (1 + h), L * (1 + h), q, *args) - er.energy(pos * (1 - h), L * (1 - h), q, *args)) / (2 * h)
    assert abs(w.sum() + dE) <= 1e-6 * abs(w.sum())


@pytest.fixture(scope="session")
def ewald_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ewald_host") / "ewald_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "ewald_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


@pytest.mark.parametrize("alpha,L,kmax", [(1.5, (7.0, 8.0, 9.5), (3, 2, 4)), (3.9, (2.5, 2.5, 2.5), (1, 1, 1)), (0.8, (11.0, 6.0, 30.0), (2, 5, 1))])
def test_host_vectors_and_coefficients_match_the_reference(ewald_host, alpha, L, kmax):
    lines = ewald_host(["table", alpha, *L, *kmax]).splitlines()
    n = er.half_vectors(kmax)
    assert lines[0] == "count %d" % n.shape[0]
    assert n.shape[0] == ((2 * kmax[0] + 1) * (2 * kmax[1] + 1) * (2 * kmax[2] + 1) - 1) // 2
    got = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[1:]])
    assert np.array_equal(got[:, :3].astype(np.int64), n)               # the same vectors in the same order
    assert not (n[:, None, :] == -n[None, :, :]).all(axis=2).any()      # a half space: no vector with its opposite
    k, A = er.coefficients(n, L, alpha)
    assert np.abs(got[:, 3] - A).max() <= 1e-14 * A.max()
    assert np.abs(got[:, 5:8] - k).max() <= 1e-14 * np.abs(k).max()
    b = 2.0 * (1.0 / (k * k).sum(axis=1) + 1.0 / (4 * alpha * alpha))
    assert np.abs(got[:, 4] - b).max() <= 1e-14 * b.max()


@pytest.mark.parametrize("case,text", [
    (["check", -1.0, 3.0, 1, 4, 4, 4], "alpha must be finite"),
    (["check", "nan", 3.0, 1, 4, 4, 4], "alpha must be finite"),
    (["check", "inf", 3.0, 1, 4, 4, 4], "alpha must be finite"),
    (["check", 1.5, 3.0, 0, 4, 4, 4], "kmax is NULL"),
    (["check", 1.5, 3.0, 1, 0, 4, 4], "kmax[0] = 0 outside [1, 64]"),
    (["check", 1.5, 3.0, 1, 4, 65, 4], "kmax[1] = 65 outside [1, 64]"),
    (["check", 1.5, 3.0, 1, 4, 4, -3], "kmax[2] = -3 outside [1, 64]"),
    (["check", 0.3, 3.0, 1, 4, 4, 4], "alpha rc = 0.9 < 1"),
])
def test_host_checks_refuse_invalid_arguments(ewald_host, case, text):
    word, code, message = ewald_host(case).rstrip("\n").split(" ", 2)
    assert word == "REFUSED" and int(code) == ERR_INVALID
    assert text in message


def test_host_checks_accept_the_limits_and_name_a_lost_pair(ewald_host):
    assert ewald_host(["check", 1.0 / 3.0 + 1e-12, 3.0, 1, 1, 64, 1]) == "ok\n"
    # struck CSR of exclusions (0,1), (1,2) and the 1-4 pair (0,3): rows 0: [1, 3], 1: [0, 2], 2: [1], 3: [0]
    for entry, pair in ((0, "(0, 1)"), (1, "(0, 3)"), (3, "(1, 2)"), (5, "(3, 0)")):
        out = ewald_host(["lost", 2, 0, 1, 1, 2, 1, 0, 3, entry])
        assert out.startswith("lost Ewald: the excluded or 1-4 pair " + pair + " is farther apart than rc + skin"), out
