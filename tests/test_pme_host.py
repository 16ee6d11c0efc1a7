"""CPU tests of smooth particle-mesh Ewald: the numpy reference tests/helpers/pme_ref.py against the direct Ewald reference
(tests/helpers/ewald_ref.py) and against its own energy, and the host side of emdee_md_set_pme (emdee.jl_amd/csrc/topology.hpp: the
argument checks, the spline moduli, the index folding, the twiddles, the fixed-point scale) through the stand-alone program
tests/c/pme_host.cpp, built with the host compiler under ASan and UBSan, against that reference."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import ewald_ref as er
from .helpers import pme_ref as pr

ERR_INVALID = -1
ALPHA, KMAX, RC = 1.5, (20, 22, 26), 3.3
# rms force error of pme_ref against ewald_ref relative to the rms force, on er.random_charges(), as measured on the CPU
#  at (order, grid) = (4, 32^3), (6, 32^3), (6, 64^3)
MEASURED = {(4, 32): 9.01e-4, (6, 32): 5.77e-5, (6, 64): 7.72e-7}


def test_reference_converges_on_the_direct_sum_along_order_and_grid():
    pos, L, q = er.random_charges()
    want = er.ewald(pos, L, q, 1.0, ALPHA, KMAX, RC)[0]
    rms = np.sqrt((want ** 2).mean())
    errs = []
    for p, g in ((4, 32), (6, 32), (6, 64)):
        got = pr.pme(pos, L, q, 1.0, ALPHA, (g, g, g), p, RC)[0]
        errs.append(np.sqrt(((got - want) ** 2).mean()) / rms)
        print("order %d grid %d^3: rms force error / rms force = %.4e (measured %.3e)" % (p, g, errs[-1], MEASURED[(p, g)]))
    assert errs[0] > errs[1] > errs[2]
    for e, key in zip(errs, ((4, 32), (6, 32), (6, 64))):
        assert e <= 2.0 * MEASURED[key]                                # (the margin: BLAS and FFT libraries of another machine)


def test_reference_forces_are_the_gradient_and_its_energy_is_the_spectral_sum():
    pos, L, q = er.random_charges(n=40, L=(5.0, 5.5, 6.0), seed=3)
    grid, p = (8, 16, 32), 4
    f, e, w, t = pr.reciprocal(pos, L, q, 1.0, 1.6, grid, p)
    E = pr.reciprocal_energy(pos, L, q, 1.0, 1.6, grid, p)
    assert abs(e.sum() - E) <= 1e-12 * abs(E)
    d = 1e-5
    for i, a in ((0, 0), (17, 1), (39, 2)):
        hi, lo = pos.copy(), pos.copy()
        hi[i, a] += d
        lo[i, a] -= d
        num = -(pr.reciprocal_energy(hi, L, q, 1.0, 1.6, grid, p) - pr.reciprocal_energy(lo, L, q, 1.0, 1.6, grid, p)) / (2 * d)
        assert abs(f[i, a] - num) <= 1e-7 * np.abs(f).max()


def test_reference_tensor_sums_to_the_volume_derivative_of_its_energy():
    # -dE/dmu at mu = 1, all sides scaled alike and the mesh kept, by a central difference over mu = 1 +- h.  The exact Coulomb
    # energy scales as E / mu, so E''' = -6 E and the truncation error of the difference is h^2 |E|; the mesh energy differs from
    # the exact one by a relative 4e-5 at order 6 on 32^3 (the energy error behind MEASURED), and the third derivative of that
    # difference -- factors (k^2 / 4 alpha^2)^3 of a few hundred on the modes that carry it -- stays under a hundredth of |E|.
    # 1e-9 |E|: the rounding of two sums of 300 fp64 terms divided by 2 h (tests/test_gpu_ewald.py, test 3).
    pos, L, q = er.random_charges(total=15.0)
    grid, p, h = (32, 32, 32), 6, 1e-4
    f, e, w, t = pr.pme(pos, L, q, 1.0, ALPHA, grid, p, RC)
    assert np.abs(t[:, :3].sum(axis=1) - w).max() <= 1e-12 * np.abs(w).max()
    dE = (pr.energy(pos * (1 + h), L * (1 + h), q, 1.0, ALPHA, grid, p, RC) - pr.energy(pos * (1 - h), L * (1 - h), q, 1.0, ALPHA, grid, p, RC)) / (2 * h)
    print("sum of the tensor's trace %.12g, -dE/dmu %.12g, difference %.3e, bound %.3e" % (t[:, :3].sum(), -dE, abs(t[:, :3].sum() + dE), (h * h + 1e-9) * abs(e.sum())))
    assert abs(t[:, :3].sum() + dE) <= (h * h + 1e-9) * abs(e.sum())


@pytest.fixture(scope="session")
def pme_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pme_host") / "pme_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "pme_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _column(out, col):
    return np.array([float(ln.split()[col]) for ln in out.splitlines()])


@pytest.mark.parametrize("K", [8, 16, 64, 256])
@pytest.mark.parametrize("p", [4, 6])
def test_host_moduli_match_the_reference(pme_host, K, p):
    got = _column(pme_host(["moduli", K, p]), 2)
    want = pr.moduli(K, p)
    assert got.shape == (K,) and got[0] == pytest.approx(1.0, abs=1e-14)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.isfinite(got).all() and got[K // 2] == got.max()          # an even order: no zero of the sum at the Nyquist index


@pytest.mark.parametrize("K", [8, 32, 256])
def test_host_folding_and_twiddles_match_the_reference(pme_host, K):
    got = _column(pme_host(["fold", K]), 2).astype(np.int64)
    assert np.array_equal(got, pr.fold(K))
    assert got.min() == -K // 2 + 1 and got.max() == K // 2             # (-K/2, K/2]
    out = pme_host(["twiddles", K])
    tw = _column(out, 2) + 1j * _column(out, 3)
    want = np.exp(-2j * np.pi * np.arange(K // 2) / K)
    # (numpy's own argument 2 pi j / K, up to pi, carries two roundings: pi * 2.2e-16, and an ulp each in cos and sin)
    assert tw.shape == (K // 2,) and np.abs(tw - want).max() <= 1e-15
    assert tw[0] == 1.0 and tw[K // 4] == -1j                           # exact on the axes
    j = np.arange(1, K // 4)
    assert np.array_equal(tw[K // 2 - j], -tw[j].conj())                # ... and mirrored exactly about them


@pytest.mark.parametrize("p", [4, 6])
def test_host_splines_match_the_cox_de_boor_recursion(pme_host, p):
    for t in (0.0, 0.25, 0.5, 0.999999, 1e-300):
        out = pme_host(["spline", repr(t), p])
        w, dw = _column(out, 2), _column(out, 3)
        j = np.arange(p)
        assert np.abs(w - pr.bspline(t + j, p)).max() <= 1e-15
        assert np.abs(dw - pr.dbspline(t + j, p)).max() <= 1e-15
        assert abs(w.sum() - 1.0) <= 1e-15 and abs(dw.sum()) <= 1e-15   # a partition of unity


def test_host_fixed_point_scale_leaves_no_room_for_an_overflow(pme_host):
    for total in (0.0, 1e-30, 0.3, 1.0, 150.0, 2.0 ** 20, 2.0 ** 20 - 1e-9, 1e30):
        shift = int(pme_host(["shift", repr(total)]).split()[1])
        assert shift == pr.fixed_shift(total), total
        if total > 0.0:
            # every contribution |q_i| w 2^shift rounded to the nearest integer, all on one mesh point: sum |q| 2^shift + N / 2
            assert total * 2.0 ** shift < 2.0 ** 61 and total * 2.0 ** shift >= 2.0 ** 60
    for bad in ("nan", "inf", -1.0):
        word, code, _ = pme_host(["shift", bad]).split(" ", 2)
        assert word == "REFUSED" and int(code) == ERR_INVALID


@pytest.mark.parametrize("case,text", [
    (["check", -1.0, 3.0, 1, 32, 32, 32, 4], "alpha must be finite"),
    (["check", "nan", 3.0, 1, 32, 32, 32, 4], "alpha must be finite"),
    (["check", "inf", 3.0, 1, 32, 32, 32, 4], "alpha must be finite"),
    (["check", 0.3, 3.0, 1, 32, 32, 32, 4], "alpha rc = 0.9 < 1"),
    (["check", 1.5, 3.0, 0, 32, 32, 32, 4], "grid is NULL"),
    (["check", 1.5, 3.0, 1, 4, 32, 32, 4], "grid[0] = 4 is not a power of two in [8, 256]"),
    (["check", 1.5, 3.0, 1, 32, 512, 32, 4], "grid[1] = 512 is not a power of two in [8, 256]"),
    (["check", 1.5, 3.0, 1, 32, 32, 48, 4], "grid[2] = 48 is not a power of two in [8, 256]"),
    (["check", 1.5, 3.0, 1, 32, 32, -16, 4], "grid[2] = -16 is not a power of two in [8, 256]"),
    (["check", 1.5, 3.0, 1, 32, 32, 0, 4], "grid[2] = 0 is not a power of two in [8, 256]"),
    (["check", 1.5, 3.0, 1, 32, 32, 32, 5], "order = 5 is neither 4 nor 6"),
    (["check", 1.5, 3.0, 1, 32, 32, 32, 8], "order = 8 is neither 4 nor 6"),
    (["check", 1.5, 3.0, 1, 32, 32, 32, 0], "order = 0 is neither 4 nor 6"),
])
def test_host_checks_refuse_invalid_arguments(pme_host, case, text):
    word, code, message = pme_host(case).rstrip("\n").split(" ", 2)
    assert word == "REFUSED" and int(code) == ERR_INVALID
    assert text in message


def test_host_checks_accept_the_limits(pme_host):
    assert pme_host(["check", 1.0 / 3.0 + 1e-12, 3.0, 1, 8, 256, 64, 4]) == "ok\n"
    assert pme_host(["check", 1.5, 3.0, 1, 256, 8, 16, 6]) == "ok\n"
