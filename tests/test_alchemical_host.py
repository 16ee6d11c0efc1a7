"""CPU tests of the parts of the soft-core alchemical decoupling with no HIP in them (include/emdee_hip.h: emdee_md_set_alchemical):
the pair function, its foreign-lambda variant, the words of a read and the table checks of emdee.jl_amd/csrc/alchemical.hpp, through
the stand-alone program tests/c/alchemical_host.cpp, built with the host compiler under ASan and UBSan, against the numpy yardstick
tests/helpers/alchemical_ref.py, which is written from the formulas of the contract."""
import os
import re
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import alchemical_ref as ar

EPS = {"d": 2.0 ** -53, "f": 2.0 ** -24}
ERR_INVALID = -1
RC, RS = 2.5, 2.0


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("alchemical_host") / "alchemical_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "alchemical_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _num(v):
    return [repr(float(t)) for t in np.asarray(v, dtype=np.float64).ravel()]


def _pairs(host, real, cases, rc=RC, rs=RS):
    """cases: rows of (r2, sigma2, e4, lambda, alpha) -> (n, 4) of E, W, dEdl, wr2"""
    cases = np.asarray(cases, dtype=np.float64).reshape(-1, 5)
    out = host(["pair", real] + _num([rc, rs]) + [len(cases)] + _num(cases))
    return np.array([[float(t) for t in line.split()] for line in out.splitlines()])


def _rounded(cases, real):
    """the operands as the program holds them"""
    cases = np.asarray(cases, dtype=np.float64).reshape(-1, 5)
    return cases.astype(np.float32).astype(np.float64) if real == "f" else cases


def _size(r2, sigma2, e4, lam, alpha):
    """the sizes of U, of W and of dUdl before any cancellation (g <= 1, -r g' <= 60/16 r^2 / (rc^2 - rs^2))"""
    u = (r2 / sigma2) ** 3
    D = alpha * (1.0 - lam) + u
    mgr = 3.75 * r2 / (RC * RC - RS * RS)
    sE = e4 * (D ** -2 + D ** -1)
    sWl = e4 * (2.0 * D ** -3 + D ** -2)
    return lam * sE, lam * (6.0 * u * sWl + sE * mgr), sE + lam * alpha * sWl


def _grid(seed, n, lam=None, alpha=None, lo=0.8, hi=2.45):
    """n random cross pairs: r in [lo, hi) sigma-free units, sigma in 0.9...1.3, 4 eps in 2...5"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(lo, hi, n)
    sigma = rng.uniform(0.9, 1.3, n)
    e4 = rng.uniform(2.0, 5.0, n)
    lam = rng.uniform(0.05, 0.95, n) if lam is None else np.full(n, lam)
    alpha = rng.uniform(0.0, 1.0, n) if alpha is None else np.full(n, alpha)
    return np.stack([r * r, sigma * sigma, e4, lam, alpha], axis=1)


def test_constants_are_the_headers(host):
    assert host(["words"]).split() == ["5", "16"]
    text = open(os.path.join(ROOT, "include", "emdee_hip.h")).read()
    for name, value in (("EMDEE_ALCH_WORDS", 5), ("EMDEE_ALCH_MAX_FOREIGN", 16)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), text), name
    for name in ("emdee_md_set_alchemical", "emdee_md_set_lambda", "emdee_md_alchemical_read", "emdee_md_alchemical_log_read"):
        assert re.search(r"int32_t %s\(" % name, text), name
    for follow_up in ("a Coulomb soft core", "more than one group, each with its own lambda", "annihilation", "decomposed runs",
                      "DECOUPLING, NOT ANNIHILATION"):
        assert follow_up in text, follow_up


@pytest.mark.parametrize("real", ["d", "f"])
def test_lambda_one_is_the_models_own_pair_function_for_any_alpha(host, real):
    """D = alpha 0 + u = u exactly, so the term is 4 eps (s^-12 - s^-6) g with s^-6 = 1 / u in place of (sigma^2 / r^2)^3: a handful of
    roundings of the size of the terms before their cancellation.  Bound: 16 x eps of that size against lj_interaction_pair restated
    operation by operation in the same precision."""
    dtype = np.float64 if real == "d" else np.float32
    cases = _grid(11, 200, lam=1.0)
    got = _pairs(host, real, cases)
    C = _rounded(cases, real)
    for q, (r2, s2, e4, lam, alpha) in enumerate(C):
        E, W = ar.literal_pair(r2, RC, RS, s2, e4, dtype)
        sE, sW, _ = _size(r2, s2, e4, 1.0, 0.0)
        assert abs(got[q, 0] - E) <= 16 * EPS[real] * sE, (q, got[q, 0], E)
        assert abs(got[q, 1] - W) <= 16 * EPS[real] * sW, (q, got[q, 1], W)
        assert abs(got[q, 3] * r2 - W) <= 16 * EPS[real] * sW, (q, got[q, 3] * r2, W)


@pytest.mark.parametrize("real", ["d", "f"])
def test_lambda_zero_is_exactly_zero(host, real):
    cases = _grid(13, 60, lam=0.0)
    cases = np.concatenate([cases, [[0.0, 1.44, 2.8, 0.0, 0.5], [0.0, 1.44, 2.8, 0.0, 0.0], [1e-30, 1.0, 4.0, 0.0, 0.5], [RC * RC, 1.0, 4.0, 0.0, 0.3],
                                    [9.0, 1.0, 4.0, 0.0, 0.3]]])
    got = _pairs(host, real, cases)
    assert (got[:, 0] == 0.0).all() and (got[:, 1] == 0.0).all() and (got[:, 3] == 0.0).all()
    # dU/dlambda is not zero there: 4 eps g (D^-2 - D^-1) with D = alpha + u
    C = _rounded(cases[:60], real)
    _, _, dl, _ = ar.pair(C[:, 0], RC, RS, C[:, 1], C[:, 2], 0.0, C[:, 4])
    _, _, sD = _size(C[:, 0], C[:, 1], C[:, 2], 0.0, C[:, 4])
    assert (np.abs(got[:60, 2] - dl) <= 16 * EPS[real] * sD).all() and np.abs(dl).max() > 0.0


@pytest.mark.parametrize("real", ["d", "f"])
def test_alpha_zero_is_lambda_times_the_plain_pair(host, real):
    cases = _grid(17, 200, alpha=0.0)
    got = _pairs(host, real, cases)
    C = _rounded(cases, real)
    E, W = ar.plain_pair(C[:, 0], RC, RS, C[:, 1], C[:, 2])
    sE, sW, _ = _size(C[:, 0], C[:, 1], C[:, 2], C[:, 3], 0.0)
    assert (np.abs(got[:, 0] - C[:, 3] * E) <= 16 * EPS[real] * sE).all()
    assert (np.abs(got[:, 1] - C[:, 3] * W) <= 16 * EPS[real] * sW).all()
    assert (np.abs(got[:, 2] - E) <= 16 * EPS[real] * sE / C[:, 3]).all()      # (dU/dlambda of a linear scaling is the plain energy)


@pytest.mark.parametrize("real", ["d", "f"])
def test_every_output_is_the_numpy_formula_below_in_and_beyond_the_switch(host, real):
    """the whole range: the core, the switch region (2.0 < r < 2.5), r^2 = rc^2 exactly (x == 1 -> 0.5, the reference's quirk) and
    beyond the cutoff, where the literal function goes on unswitched (the cutoff is the caller's test)"""
    cases = np.concatenate([_grid(19, 150), _grid(23, 150, lo=2.0, hi=2.5), _grid(29, 40, lo=2.5, hi=3.2),
                            [[RC * RC, 1.21, 3.0, 0.6, 0.5], [RS * RS, 1.21, 3.0, 0.6, 0.5]]])
    got = _pairs(host, real, cases)
    C = _rounded(cases, real)
    U, W, dl, wr2 = ar.pair(C[:, 0], RC, RS, C[:, 1], C[:, 2], C[:, 3], C[:, 4])
    sE, sW, sD = _size(C[:, 0], C[:, 1], C[:, 2], C[:, 3], C[:, 4])
    # (the switch variable x carries eps32 / eps64 of r^2 / (rc^2 - rs^2) ~ 3: g and g' move by tens of eps inside the switch)
    k = 64 * EPS[real]
    exact = np.ones(len(C), dtype=bool)
    if real == "f":
        # (fp32 rounds rc^2 idl2 - x0 to a neighbour of 1: the x == 1 quirk is a property of the fp64 operands only)
        exact[-2] = False
    assert (np.abs(got[:, 0] - U) <= k * sE)[exact].all()
    assert (np.abs(got[:, 1] - W) <= k * sW)[exact].all()
    assert (np.abs(got[:, 2] - dl) <= k * sD)[exact].all()
    assert (np.abs(got[:, 3] * C[:, 0] - W) <= k * sW)[exact].all()
    inside = (C[:, 0] > RS * RS) & (C[:, 0] < RC * RC)
    assert inside.sum() >= 150 and (C[:, 0] >= RC * RC).sum() >= 40


def _third(fun, s, k):
    """|f'''| near s from the five-point stencil of step k, on the fp64 yardstick: the largest of the estimates at s - k, s, s + k"""
    est = [abs(fun(c + 2 * k) - 2 * fun(c + k) + 2 * fun(c - k) - fun(c - 2 * k)) / (2 * k ** 3) for c in (s - k, s, s + k)]
    return max(est)


def test_W_is_the_centred_difference_of_the_energy_in_ln_r(host):
    """With s = ln r, dU/ds = r dU/dr = -W.  The centred difference of step h errs by h^2 / 6 |U'''(s)| -- the third derivative's size
    is taken from the fp64 yardstick by a five-point stencil of step 8 h, doubled for the stencil's own error -- plus the rounding of
    the two energies, 64 x 2^-53 of their size before cancellation, over 2 h; h is a power of two.  Points within the stencil's reach
    of the two seams of the switch, where U''' jumps, are left to the test above."""
    h = 2.0 ** -13
    cases = np.concatenate([_grid(31, 120, lo=0.8, hi=1.95), _grid(37, 80, lo=2.06, hi=2.44), _grid(41, 20, lo=0.3, hi=0.8)])
    got = _pairs(host, "d", cases)
    up, dn = cases.copy(), cases.copy()
    up[:, 0] *= np.exp(2 * h)
    dn[:, 0] *= np.exp(-2 * h)
    Up, Um = _pairs(host, "d", up)[:, 0], _pairs(host, "d", dn)[:, 0]
    for q, (r2, s2, e4, lam, alpha) in enumerate(cases):
        fun = lambda s: float(ar.pair(r2 * np.exp(2 * s), RC, RS, s2, e4, lam, alpha)[0])
        trunc = 2.0 * h * h / 6.0 * _third(fun, 0.0, 8 * h)
        rounding = 64 * EPS["d"] * _size(r2, s2, e4, lam, alpha)[0] / (2 * h)
        slope = (Up[q] - Um[q]) / (2 * h)
        assert abs(slope + got[q, 1]) <= trunc + rounding, (q, slope, got[q, 1], trunc, rounding)
        # ... and the force factor is W / r^2
        assert abs(got[q, 3] * r2 - got[q, 1]) <= 16 * EPS["d"] * _size(r2, s2, e4, lam, alpha)[1]


def test_dUdlambda_is_the_centred_difference_of_the_energy_in_lambda(host):
    """the same rule along lambda (lambda +- h stays inside (0, 1)); U is smooth in lambda for alpha (1 - lambda) + u > 0"""
    h = 2.0 ** -13
    cases = np.concatenate([_grid(43, 150), _grid(47, 50, lo=0.2, hi=0.8, alpha=0.5)])
    got = _pairs(host, "d", cases)
    up, dn = cases.copy(), cases.copy()
    up[:, 3] += h
    dn[:, 3] -= h
    Up, Um = _pairs(host, "d", up)[:, 0], _pairs(host, "d", dn)[:, 0]
    for q, (r2, s2, e4, lam, alpha) in enumerate(cases):
        fun = lambda t: float(ar.pair(r2, RC, RS, s2, e4, lam + t, alpha)[0])
        trunc = 2.0 * h * h / 6.0 * _third(fun, 0.0, 8 * h)
        rounding = 64 * EPS["d"] * _size(r2, s2, e4, lam + h, alpha)[0] / (2 * h)
        slope = (Up[q] - Um[q]) / (2 * h)
        assert abs(slope - got[q, 2]) <= trunc + rounding, (q, slope, got[q, 2], trunc, rounding)


@pytest.mark.parametrize("real", ["d", "f"])
def test_overlap_is_finite_with_no_virial_and_no_force(host, real):
    cases = [[r2, 1.44, 2.8, lam, 0.5] for r2 in (0.0, 1e-30) for lam in (0.1, 0.5, 0.9)]
    got = _pairs(host, real, cases)
    assert np.isfinite(got).all()
    for q, (r2, s2, e4, lam, alpha) in enumerate(cases):
        D = alpha * (1.0 - lam)
        want = lam * e4 * (D ** -2 - D ** -1)
        assert abs(got[q, 0] - want) <= 16 * EPS[real] * lam * e4 * (D ** -2 + D ** -1)
        # W = 6 u lambda 4 eps (2 D^-3 - D^-2): u = (r^2 / sigma^2)^3 is 0 at r = 0 and 1e-90 / sigma^6 at r^2 = 1e-30 (0 in Float32)
        u = (r2 / s2) ** 3
        assert abs(got[q, 1]) <= 6.0 * u * lam * e4 * 3.0 * D ** -3
        if r2 == 0.0 or real == "f":
            assert got[q, 1] == 0.0
        assert got[q, 3] * np.sqrt(r2) <= 1e-40                      # the force d W / r^2 at |d| = r


@pytest.mark.parametrize("real", ["d", "f"])
def test_foreign_variant_is_K_single_calls_bit_for_bit(host, real):
    lams = [0.0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 1.0, 0.33, 0.66, 0.99]
    for r2, s2, e4, alpha in ((1.3, 1.21, 3.3, 0.5), (4.9, 1.0, 4.0, 0.25), (0.0, 1.44, 2.8, 0.5), (6.1, 1.0, 4.0, 0.0)):
        out = host(["foreign", real] + _num([RC, RS, r2, s2, e4, alpha]) + [len(lams)] + _num(lams)).split()
        single = host(["pair", real] + _num([RC, RS]) + [len(lams)] + _num([[r2, s2, e4, lam, alpha] for lam in lams])).splitlines()
        assert out == [line.split()[0] for line in single]


def _params(host, lam=0.5, alpha=0.5, foreign=(0.0, 1.0), every=1, capacity=4, nf=None):
    nf = len(foreign) if nf is None else nf
    return host(["params"] + _num([lam, alpha]) + [nf] + (_num(foreign) if 0 < nf <= 64 else []) + [every, capacity])


def test_every_table_check_refuses_with_its_code_and_names_the_value(host):
    assert _params(host).split() == ["ok"]
    assert _params(host, lam=0.0, alpha=0.0, foreign=(), every=0, capacity=0).split() == ["ok"]
    assert _params(host, lam=1.0, foreign=[k / 15.0 for k in range(16)]).split() == ["ok"]
    cases = {
        "lambda below": (dict(lam=-0.01), ["lambda = -0.01", "[0, 1]"]),
        "lambda above": (dict(lam=1.5), ["lambda = 1.5", "[0, 1]"]),
        "lambda nan": (dict(lam=np.nan), ["lambda = nan"]),
        "foreign above": (dict(foreign=(0.2, 1.25)), ["foreign lambda 1 = 1.25", "[0, 1]"]),
        "foreign nan": (dict(foreign=(np.nan,)), ["foreign lambda 0 = nan"]),
        "alpha negative": (dict(alpha=-0.5), ["alpha = -0.5"]),
        "alpha nan": (dict(alpha=np.nan), ["alpha = nan"]),
        "alpha inf": (dict(alpha=np.inf), ["alpha = inf"]),
        "17 foreign": (dict(foreign=[0.5] * 17), ["n_foreign = 17", "0...16"]),
        "negative count": (dict(nf=-1), ["n_foreign = -1"]),
        "negative every": (dict(every=-1), ["log_every = -1"]),
        "negative capacity": (dict(capacity=-3), ["log_capacity = -3"]),
        "a log without a cadence": (dict(every=0, capacity=8), ["log_every = 0", "log_capacity = 8"]),
        "a log too large": (dict(capacity=2 ** 30), ["2^30 words"]),
    }
    for name, (change, words) in cases.items():
        out = _params(host, **change)
        assert out.startswith("REFUSED %d set_alchemical: " % ERR_INVALID), (name, out)
        for w in words:
            assert w in out, (name, w, out)


def test_flags_are_zero_or_one_with_at_least_one_set(host):
    flag = np.zeros(300, dtype=np.int64)
    flag[[7, 150, 299]] = 1
    assert host(["flags", len(flag)] + list(flag)).split() == ["flagged", "3", "ids", "7", "150", "299"]
    for bad, words in ((2, ["atom 41", "flag 2"]), (-1, ["atom 41", "flag -1"])):
        f = flag.copy()
        f[41] = bad
        out = host(["flags", len(f)] + list(f))
        assert out.startswith("REFUSED %d set_alchemical: " % ERR_INVALID), out
        for w in words:
            assert w in out
    out = host(["flags", 300] + [0] * 300)
    assert out.startswith("REFUSED %d set_alchemical: " % ERR_INVALID) and "no atom is flagged" in out
    # the readiness check of a charged engine: the first flagged atom that carries a charge
    q = np.zeros(300)
    assert host(["charged", 3, 7, 150, 299, 300] + _num(q)).split() == ["-1"]
    q[[3, 150, 299]] = [0.4, -0.2, 0.1]
    assert host(["charged", 3, 7, 150, 299, 300] + _num(q)).split() == ["150"]
