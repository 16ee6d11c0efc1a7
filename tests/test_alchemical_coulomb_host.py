"""CPU tests of the parts of the Coulomb stage of the alchemical table with no HIP in them (include/emdee_hip.h:
emdee_md_set_alchemical_coulomb): the pair function, its foreign variant and the parameter checks of emdee.jl_amd/csrc/alchemical.hpp,
through the stand-alone program tests/c/alchemical_coulomb_host.cpp, built with the host compiler under ASan and UBSan, against the
numpy yardstick tests/helpers/alchemical_coulomb_ref.py, which is written from the formulas of the contract."""
import os
import re
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import alchemical_coulomb_ref as cr

EPS = {"d": 2.0 ** -53, "f": 2.0 ** -24}
ERR_INVALID = -1
RC = 2.5
EPS_RF = (1.0, 78.0, np.inf)
K_ULP = 16                                                 # (the constant of tests/test_alchemical_host.py; no switch is involved)


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("alchemical_coulomb_host") / "alchemical_coulomb_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "alchemical_coulomb_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _num(v):
    return [repr(float(t)) for t in np.asarray(v, dtype=np.float64).ravel()]


def _held(v, real):
    """operands and constants as the program holds them"""
    v = np.asarray(v, dtype=np.float64)
    return v.astype(np.float32).astype(np.float64) if real == "f" else v


def _rf(eps_rf, real):
    k, c = cr.rf_constants(RC, eps_rf)
    return float(_held(k, real)), float(_held(c, real)), k, c


def _pairs(host, real, k, c, cases):
    """cases: rows of (r2, qq, lambda_q, beta) -> (n, 4) of E, W, dEdl, wr2"""
    cases = np.asarray(cases, dtype=np.float64).reshape(-1, 4)
    out = host(["pair", real] + _num([k, c]) + [len(cases)] + _num(cases))
    return np.array([[float(t) for t in line.split()] for line in out.splitlines()])


def _grid(seed, n, lam_q=None, beta=None, lo=0.05, hi=1.2):
    """n random cross pairs: r in [lo, hi) rc, qq in +-(0.05 ... 2), lambda_q in 0.05 ... 0.95, beta in 0 ... 1"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(lo, hi, n) * RC
    qq = rng.uniform(0.05, 2.0, n) * rng.choice([-1.0, 1.0], n)
    lam_q = rng.uniform(0.05, 0.95, n) if lam_q is None else np.full(n, lam_q)
    beta = rng.uniform(0.0, 1.0, n) if beta is None else np.full(n, beta)
    return np.stack([r * r, qq, lam_q, beta], axis=1)


def _size_dl(r2, qq, k, c, lam_q, beta):
    """dU/dlambda_q = qq (phi + lambda_q (beta / 2) wl) has one addend more than U: its size before cancellation is the term's,
    |qq| (1/rho + k rho2 + c), plus |qq| lambda_q (beta / 2) (1/rho^3 + 2 k)"""
    rho2 = r2 + beta * (1.0 - lam_q)
    return cr.size(r2, qq, k, c, lam_q, beta) + np.abs(qq) * lam_q * 0.5 * beta * (rho2 ** -1.5 + 2.0 * k)


def test_constants_and_prototypes_are_the_headers(host):
    assert host(["words"]).split() == ["4", "5", "16"]
    text = open(os.path.join(ROOT, "include", "emdee_hip.h")).read()
    for name, value in (("EMDEE_ALCH_COULOMB_WORDS", 4), ("EMDEE_ALCH_WORDS", 5), ("EMDEE_ALCH_MAX_FOREIGN", 16)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), text), name
    for name in ("emdee_md_set_alchemical_coulomb", "emdee_md_set_lambda_coulomb", "emdee_md_alchemical_coulomb_read",
                 "emdee_md_alchemical_coulomb_log_read"):
        assert re.search(r"int32_t %s\(" % name, text), name
    for follow_up in ("a Coulomb soft core under Ewald or PME", "more than one group", "annihilation", "decomposed runs",
                      "a per-pair soft-core length", "GROMACS's"):
        assert follow_up in text, follow_up
    # the ctypes table of the Python binding names the four entries too
    lib = open(os.path.join(ROOT, "emdee.jl_amd", "_lib.py")).read()
    for name in ("emdee_md_set_alchemical_coulomb", "emdee_md_set_lambda_coulomb", "emdee_md_alchemical_coulomb_read",
                 "emdee_md_alchemical_coulomb_log_read"):
        assert '"%s"' % name in lib, name


@pytest.mark.parametrize("eps_rf", EPS_RF)
@pytest.mark.parametrize("real", ["d", "f"])
def test_every_output_is_the_numpy_formula_inside_at_and_beyond_the_cutoff(host, real, eps_rf):
    """r in [0.05, 1.2] rc, r^2 = rc^2 exactly and beyond it (the cutoff is the caller's test: the function goes on).  Bound: 16 eps
    of the term's size before cancellation, |qq| (1/rho + k_rf rho2 + c_rf); dU/dlambda_q has the soft core's addend on top
    (_size_dl).  A count of the roundings: 1/rho carries 1.5 eps, k rho2 2 eps, the two sums, qq and lambda_q half an eps each of
    partial results no larger than the size -- under 6 eps in all."""
    k, c, _, _ = _rf(eps_rf, real)
    cases = np.concatenate([_grid(3, 300), _grid(5, 60, lo=1.0, hi=1.2), [[RC * RC, -0.7, 0.4, 0.3], [RC * RC, 0.7, 1.0, 0.3],
                                                                         [RC * RC, 0.7, 0.5, 0.0]]])
    got = _pairs(host, real, k, c, cases)
    C = _held(cases, real)
    U, W, dl, wr2 = cr.pair(C[:, 0], C[:, 1], k, c, C[:, 2], C[:, 3])
    s = cr.size(C[:, 0], C[:, 1], k, c, C[:, 2], C[:, 3])
    tol = K_ULP * EPS[real]
    assert (np.abs(got[:, 0] - U) <= tol * s).all()
    assert (np.abs(got[:, 1] - W) <= tol * s).all()
    assert (np.abs(got[:, 3] * C[:, 0] - W) <= tol * s).all()
    assert (np.abs(got[:, 2] - dl) <= tol * _size_dl(C[:, 0], C[:, 1], k, c, C[:, 2], C[:, 3])).all()
    assert (C[:, 0] >= RC * RC).sum() >= 40 and (C[:, 0] < 0.01 * RC * RC).sum() >= 5


def _third(fun, s, k):
    """|f'''| near s from the five-point stencil of step k, on the fp64 yardstick: the largest of the estimates at s - k, s, s + k"""
    est = [abs(fun(c + 2 * k) - 2 * fun(c + k) + 2 * fun(c - k) - fun(c - 2 * k)) / (2 * k ** 3) for c in (s - k, s, s + k)]
    return max(est)


@pytest.mark.parametrize("eps_rf", EPS_RF)
def test_W_is_the_centred_difference_of_the_energy_in_ln_r(host, eps_rf):
    """With s = ln r, dU/ds = r dU/dr = -W.  The centred difference of step h errs by h^2 / 6 |U'''(s)| -- its size taken from the
    fp64 yardstick by a five-point stencil of step 8 h, doubled for the stencil's own error -- plus the rounding of the two energies,
    16 x 2^-53 of their size before cancellation, over 2 h; h is a power of two (the rule of tests/test_alchemical_host.py)."""
    h = 2.0 ** -13
    k, c, _, _ = _rf(eps_rf, "d")
    cases = _grid(7, 200)
    got = _pairs(host, "d", k, c, cases)
    up, dn = cases.copy(), cases.copy()
    up[:, 0] *= np.exp(2 * h)
    dn[:, 0] *= np.exp(-2 * h)
    Up, Um = _pairs(host, "d", k, c, up)[:, 0], _pairs(host, "d", k, c, dn)[:, 0]
    for q, (r2, qq, lam_q, beta) in enumerate(cases):
        fun = lambda s: float(cr.pair(r2 * np.exp(2 * s), qq, k, c, lam_q, beta)[0])
        trunc = 2.0 * h * h / 6.0 * _third(fun, 0.0, 8 * h)
        rounding = K_ULP * EPS["d"] * cr.size(r2, qq, k, c, lam_q, beta) / (2 * h)
        slope = (Up[q] - Um[q]) / (2 * h)
        assert abs(slope + got[q, 1]) <= trunc + rounding, (q, slope, got[q, 1], trunc, rounding)


@pytest.mark.parametrize("eps_rf", EPS_RF)
def test_dUdlambda_q_is_the_centred_difference_of_the_energy_in_lambda_q(host, eps_rf):
    """the same rule along lambda_q (lambda_q +- h stays inside (0, 1)); U_q is smooth in lambda_q for rho2 > 0"""
    h = 2.0 ** -13
    k, c, _, _ = _rf(eps_rf, "d")
    cases = _grid(9, 200)
    got = _pairs(host, "d", k, c, cases)
    up, dn = cases.copy(), cases.copy()
    up[:, 2] += h
    dn[:, 2] -= h
    Up, Um = _pairs(host, "d", k, c, up)[:, 0], _pairs(host, "d", k, c, dn)[:, 0]
    for q, (r2, qq, lam_q, beta) in enumerate(cases):
        fun = lambda t: float(cr.pair(r2, qq, k, c, lam_q + t, beta)[0])
        trunc = 2.0 * h * h / 6.0 * _third(fun, 0.0, 8 * h)
        rounding = K_ULP * EPS["d"] * cr.size(r2, qq, k, c, lam_q + h, beta) / (2 * h)
        slope = (Up[q] - Um[q]) / (2 * h)
        assert abs(slope - got[q, 2]) <= trunc + rounding, (q, slope, got[q, 2], trunc, rounding)


@pytest.mark.parametrize("real", ["d", "f"])
def test_lambda_q_zero_is_exactly_zero_and_dUdlambda_q_is_not(host, real):
    k, c, _, _ = _rf(78.0, real)
    cases = np.concatenate([_grid(11, 60, lam_q=0.0), [[0.0, 0.9, 0.0, 0.5], [1e-30, -0.9, 0.0, 0.5], [RC * RC, 0.9, 0.0, 0.3],
                                                       [9.0, 0.9, 0.0, 0.3]]])
    got = _pairs(host, real, k, c, cases)
    assert (got[:, 0] == 0.0).all() and (got[:, 1] == 0.0).all() and (got[:, 3] == 0.0).all()
    C = _held(cases[:60], real)
    _, _, dl, _ = cr.pair(C[:, 0], C[:, 1], k, c, 0.0, C[:, 3])
    s = cr.size(C[:, 0], C[:, 1], k, c, 0.0, C[:, 3])
    assert (np.abs(got[:60, 2] - dl) <= K_ULP * EPS[real] * s).all() and np.abs(dl).min() > 0.0 and (got[:60, 2] != 0.0).all()


@pytest.mark.parametrize("eps_rf", EPS_RF)
@pytest.mark.parametrize("real", ["d", "f"])
def test_beta_zero_is_lambda_q_times_the_plain_reaction_field_pair(host, real, eps_rf):
    """rho2 = r2 + 0 (1 - lambda_q) == r2 bit for bit; dU/dlambda_q of a linear scaling is the plain energy.  Also beta > 0 at
    lambda_q = 1, where beta (1 - lambda_q) is 0 again."""
    k, c, _, _ = _rf(eps_rf, real)
    cases = np.concatenate([_grid(13, 200, beta=0.0), _grid(15, 50, lam_q=1.0)])
    got = _pairs(host, real, k, c, cases)
    C = _held(cases, real)
    E, W = cr.plain_rf(C[:, 0], C[:, 1], k, c)
    s = cr.size(C[:, 0], C[:, 1], k, c, 1.0, 0.0)
    tol = K_ULP * EPS[real]
    assert (np.abs(got[:, 0] - C[:, 2] * E) <= tol * s).all()
    assert (np.abs(got[:, 1] - C[:, 2] * W) <= tol * s).all()
    assert (np.abs(got[:200, 2] - E[:200]) <= tol * s[:200]).all()


@pytest.mark.parametrize("real", ["d", "f"])
def test_overlap_is_finite_and_exerts_no_force(host, real):
    """r^2 in {0, 1e-30} with beta (1 - lambda_q) > 0.  Everything is finite; W_q = wr2 r^2 is 0 or of the order 1e-30; the force is
    wr2 d, |d| = r: 0 at r = 0.  The contract's check is wr2 r <= 1e-40, as the Lennard-Jones test writes it (signed): it holds at
    r = 0 for either sign of qq and at r^2 = 1e-30 for opposite charges (qq < 0, wl > 0: the pair attracts).  Unlike the
    Lennard-Jones soft core, whose wr2 goes as r^4, wr2_q tends to lambda_q qq (1/rho^3 - 2 k) at r = 0, so for like charges at
    r^2 = 1e-30 the force is |wr2| r ~ 1e-15 |qq| / rho^3, linear in r: that case is bounded by this size, not by 1e-40."""
    k, c, _, _ = _rf(np.inf, real)
    cases = [[r2, qq, lam_q, 0.3] for r2 in (0.0, 1e-30) for qq in (-0.16, 0.16) for lam_q in (0.1, 0.5, 0.9)]
    got = _pairs(host, real, k, c, cases)
    assert np.isfinite(got).all()
    C = _held(cases, real)
    U, W, dl, wr2 = cr.pair(C[:, 0], C[:, 1], k, c, C[:, 2], C[:, 3])
    s = cr.size(C[:, 0], C[:, 1], k, c, C[:, 2], C[:, 3])
    assert (np.abs(got[:, 0] - U) <= K_ULP * EPS[real] * s).all()
    assert (np.abs(got[:, 2] - dl) <= K_ULP * EPS[real] * _size_dl(C[:, 0], C[:, 1], k, c, C[:, 2], C[:, 3])).all()
    for q, (r2, qq, lam_q, beta) in enumerate(C):
        r = np.sqrt(r2)
        if r2 == 0.0:
            assert got[q, 1] == 0.0 and abs(got[q, 3]) * r <= 1e-40
        if qq < 0.0:
            assert got[q, 3] * r <= 1e-40
        rho3 = (r2 + beta * (1.0 - lam_q)) ** 1.5
        assert abs(got[q, 3]) * r <= 1.001 * lam_q * abs(qq) * (1.0 / rho3 + 2.0 * k) * r
        assert abs(got[q, 1]) <= 1.001 * lam_q * abs(qq) * (1.0 / rho3 + 2.0 * k) * r2


@pytest.mark.parametrize("real", ["d", "f"])
def test_foreign_variant_is_K_single_calls_bit_for_bit(host, real):
    k, c, _, _ = _rf(78.0, real)
    lams = [0.0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 1.0, 0.33, 0.66, 0.99]
    for r2, qq, beta in ((1.3, -0.16, 0.3), (4.9, 0.16, 0.25), (0.0, -0.64, 0.5), (6.25, 0.3, 0.1), (6.1, 1.0, 0.0)):
        out = host(["foreign", real] + _num([k, c, r2, qq, beta]) + [len(lams)] + _num(lams)).split()
        single = host(["pair", real] + _num([k, c]) + [len(lams)] + _num([[r2, qq, lam, beta] for lam in lams])).splitlines()
        assert out == [line.split()[0] for line in single]


def _params(host, lam_q=0.5, beta=0.3, foreign_q=(0.0, 1.0), nf=None, table_nf=None, null=False):
    nf = len(foreign_q) if nf is None else nf
    table_nf = nf if table_nf is None else table_nf
    return host(["params"] + _num([lam_q, beta]) + [nf, int(null)] + (_num(foreign_q) if 0 < nf <= 64 and not null else []) + [table_nf])


def test_every_parameter_check_refuses_with_its_code_and_names_the_value(host):
    assert _params(host).split() == ["ok"]
    assert _params(host, lam_q=0.0, beta=0.0, foreign_q=()).split() == ["ok"]
    assert _params(host, foreign_q=(), null=True).split() == ["ok"]                    # (NULL is allowed with n_foreign = 0)
    assert _params(host, lam_q=1.0, foreign_q=[k / 15.0 for k in range(16)]).split() == ["ok"]
    cases = {
        "lambda_q below": (dict(lam_q=-0.01), ["lambda_q = -0.01", "[0, 1]"]),
        "lambda_q above": (dict(lam_q=1.5), ["lambda_q = 1.5", "[0, 1]"]),
        "lambda_q nan": (dict(lam_q=np.nan), ["lambda_q = nan"]),
        "foreign above": (dict(foreign_q=(0.2, 1.25)), ["foreign lambda_q 1 = 1.25", "[0, 1]"]),
        "foreign below": (dict(foreign_q=(-0.5, 0.25)), ["foreign lambda_q 0 = -0.5", "[0, 1]"]),
        "foreign nan": (dict(foreign_q=(np.nan,)), ["foreign lambda_q 0 = nan"]),
        "beta negative": (dict(beta=-0.5), ["beta = -0.5"]),
        "beta nan": (dict(beta=np.nan), ["beta = nan"]),
        "beta inf": (dict(beta=np.inf), ["beta = inf"]),
        "fewer than the table": (dict(foreign_q=(0.5,), table_nf=3), ["n_foreign = 1", "has 3"]),
        "more than the table": (dict(foreign_q=(0.5, 0.6), table_nf=0), ["n_foreign = 2", "has 0"]),
        "a NULL array": (dict(foreign_q=(0.5, 0.6), null=True), ["NULL", "n_foreign = 2"]),
    }
    for name, (change, words) in cases.items():
        out = _params(host, **change)
        assert out.startswith("REFUSED %d set_alchemical_coulomb: " % ERR_INVALID), (name, out)
        for w in words:
            assert w in out, (name, w, out)
    assert host(["lambda", 0.25]).split() == ["ok"]
    for bad in (-0.125, 1.125, np.nan):
        out = host(["lambda", repr(float(bad))])
        assert out.startswith("REFUSED %d set_lambda_coulomb: lambda_q = %g" % (ERR_INVALID, bad)), out
