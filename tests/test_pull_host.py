"""CPU tests of the parts of the centre-of-mass pull with no HIP in them (include/emdee_hip.h: emdee_md_set_pull): the term of one
coordinate, the work rule and a group's ten words of emdee.jl_amd/csrc/pull.hpp, and the table builder of
emdee.jl_amd/csrc/topology.hpp with the mirror refusal of the site table, through the stand-alone program tests/c/pull_host.cpp, built
with the host compiler under ASan and UBSan, against the numpy yardstick tests/helpers/pull_ref.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import pull_ref as pr

EPS = 2.0 ** -53
ERR_INVALID, ERR_STATE = -1, -6
MASKS = [1, 2, 3, 4, 5, 6, 7]


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pull_host") / "pull_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "pull_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _num(v):
    return [repr(float(t)) for t in np.asarray(v, dtype=np.float64).ravel()]


def _rows(text):
    return np.array([[float(t) for t in line.split()] for line in text.splitlines()])


def _term(host, cases):
    """cases: a list of (coordinate dict, xi0, D) -> xi, f, U (n,), Fb (n, 3), T (n, 6)"""
    flat = []
    for c, xi0, D in cases:
        flat += [c["kind"], c["geometry"], c["mask"]] + _num([c["k"]]) + _num(c["n"]) + _num([xi0]) + _num(D)
    out = _rows(host(["term", len(cases)] + flat))
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3:6], out[:, 6:12]


def _coord(kind, geometry, mask=7, k=1.0, n=(0.0, 0.0, 0.0), r0=0.0, rate=0.0, a=0, b=1):
    return dict(a=a, b=b, kind=kind, geometry=geometry, mask=mask, k=k, n=np.asarray(n, dtype=np.float64), r0=r0, rate=rate)


def _cases():
    """both geometries x both kinds, all seven masks; the direction vectors are unit vectors, as the builder leaves them.  |xi| >= 0.5
    throughout, so the finite differences below stay away from the cusp of the distance at xi = 0."""
    rng = np.random.default_rng(61)
    cases = []
    for kind in (pr.UMBRELLA, pr.CONSTANT_FORCE):
        for mask in MASKS:
            m = np.array([(mask >> a) & 1 for a in range(3)], dtype=np.float64)
            for _ in range(12):
                D = rng.normal(0.0, 2.0, 3)
                D += np.sign(D) * 0.5 * m                           # every kept axis at least 0.5 from 0
                k = rng.uniform(0.5, 300.0) * (1.0 if kind == pr.UMBRELLA else rng.choice([-1.0, 1.0]))
                cases.append((_coord(kind, pr.DISTANCE, mask, k), rng.uniform(0.0, 4.0), D))
        for _ in range(40):
            n = pr.unit(rng.normal(0.0, 1.0, 3))
            D = rng.normal(0.0, 2.0, 3)
            D += n * np.sign(n @ D) * 0.5
            k = rng.uniform(0.5, 300.0) * (1.0 if kind == pr.UMBRELLA else rng.choice([-1.0, 1.0]))
            cases.append((_coord(kind, pr.DIRECTION, 0, k, n), rng.uniform(-4.0, 4.0), D))
    return cases


def _scale(c, xi0, xi, h=0.0):
    """the size of U before any cancellation"""
    if c["kind"] == pr.CONSTANT_FORCE:
        return abs(c["k"]) * (abs(xi) + h)
    return c["k"] * (abs(xi) + abs(xi0) + h) ** 2


def test_constants_are_the_headers(host):
    assert host(["words"]).split() == ["8", "10", "8", "8"]
    text = open(os.path.join(ROOT, "include", "emdee_hip.h")).read()
    for name, value in (("EMDEE_PULL_WORDS", 8), ("EMDEE_PULL_UMBRELLA", 1), ("EMDEE_PULL_CONSTANT_FORCE", 2), ("EMDEE_PULL_DISTANCE", 1),
                        ("EMDEE_PULL_DIRECTION", 2)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), text), name
    for name in ("emdee_md_set_pull", "emdee_md_pull_read", "emdee_md_pull_log_read"):
        assert re.search(r"int32_t %s\(" % name, text), name
    for follow_up in ("fixed point in space", "angle and dihedral", "flat-bottomed biases", "decomposed engines", "RECTANGLE RULE",
                      "DO NOT SCALE WITH THE BOX"):
        assert follow_up in text, follow_up


def test_term_is_the_numpy_formula(host):
    """Same formulas on both sides, fp64: what may differ is the order of a three-term sum, contraction, the square root and the
    division -- a handful of roundings of the size of the terms.  Bound: 8 x 2^-53 of the size before cancellation."""
    cases = _cases()
    xi, f, U, Fb, T = _term(host, cases)
    for q, (c, xi0, D) in enumerate(cases):
        rxi, rf, rU, rFb, rT = pr.term(c, xi0, D)
        dn, fs = np.abs(D).sum(), abs(c["k"]) * (1.0 if c["kind"] == pr.CONSTANT_FORCE else abs(rxi) + abs(xi0))
        assert abs(xi[q] - rxi) <= 8 * EPS * dn
        assert abs(f[q] - rf) <= 16 * EPS * fs
        assert abs(U[q] - rU) <= 16 * EPS * _scale(c, xi0, rxi)
        assert (np.abs(Fb[q] - rFb) <= 16 * EPS * fs).all()
        assert (np.abs(T[q] - rT) <= 24 * EPS * fs * dn).all()
        # the tensor's trace is D . F_b
        assert abs(T[q, :3].sum() - D @ Fb[q]) <= 8 * EPS * (np.abs(D) * np.abs(Fb[q])).sum()
        # a masked axis carries no force
        if c["geometry"] == pr.DISTANCE:
            for a in range(3):
                if not (c["mask"] >> a) & 1:
                    assert Fb[q, a] == 0.0


def test_f_is_the_centred_difference_of_the_energy_along_xi(host):
    """Stepping D by +-h along dxi/dD (a unit vector in both geometries) moves xi by +-h.  U is quadratic or linear in xi, so
    (U(+h) - U(-h)) / 2h = dU/dxi = -f up to the rounding of the operands: 2^-53 of the size of U per evaluation, a few of them,
    and of xi itself (whose error k |xi - xi0| multiplies), all divided by 2h; h is a power of two."""
    cases = _cases()
    xi, f, U, Fb, _ = _term(host, cases)
    h = 2.0 ** -10
    plus, minus = [], []
    for q, (c, xi0, D) in enumerate(cases):
        g = Fb[q] / f[q] if f[q] != 0.0 else None
        if g is None:
            g = pr.unit(c["n"]) if c["geometry"] == pr.DIRECTION else np.zeros(3)
        plus.append((c, xi0, D + h * g)); minus.append((c, xi0, D - h * g))
    _, _, Up, _, _ = _term(host, plus)
    _, _, Um, _, _ = _term(host, minus)
    for q, (c, xi0, D) in enumerate(cases):
        slope = (Up[q] - Um[q]) / (2.0 * h)
        bound = 64 * EPS * _scale(c, xi0, xi[q], h) / (2.0 * h)
        assert abs(slope + f[q]) <= bound, (q, slope, f[q], bound)


def test_force_on_b_is_the_centred_difference_in_D(host):
    """-dU/dD_a = F_b,a.  The direction geometry is linear or quadratic in D: rounding only.  The distance geometry is
    1/2 k (|m o D| - xi0)^2 or -F |m o D|, whose third derivatives are at most 3 k xi0 / xi^2 and 3 |F| / xi^2 (restraint_host's bound for
    the same function): truncation h^2 / 6 of that, rounded up to h^2 k xi0 / xi^2 (|F| for k xi0)."""
    cases = _cases()
    xi, f, U, Fb, _ = _term(host, cases)
    h = 2.0 ** -17
    for a in range(3):
        e = np.zeros(3); e[a] = 1.0
        _, _, Up, _, _ = _term(host, [(c, xi0, D + h * e) for c, xi0, D in cases])
        _, _, Um, _, _ = _term(host, [(c, xi0, D - h * e) for c, xi0, D in cases])
        for q, (c, xi0, D) in enumerate(cases):
            slope = -(Up[q] - Um[q]) / (2.0 * h)
            rounding = 64 * EPS * _scale(c, xi0, xi[q], h) / (2.0 * h)
            trunc = 0.0
            if c["geometry"] == pr.DISTANCE:
                trunc = h * h * (abs(c["k"]) if c["kind"] == pr.CONSTANT_FORCE else c["k"] * abs(xi0)) / xi[q] ** 2
            assert abs(slope - Fb[q, a]) <= rounding + trunc, (q, a, slope, Fb[q, a], rounding, trunc)


def test_zero_distance_gives_zero_force_and_a_finite_energy(host):
    cases = []
    for kind in (pr.UMBRELLA, pr.CONSTANT_FORCE):
        for mask in MASKS:
            m = np.array([(mask >> a) & 1 for a in range(3)], dtype=np.float64)
            D = (1.0 - m) * np.array([1.5, -2.5, 0.75])              # zero on every kept axis
            cases.append((_coord(kind, pr.DISTANCE, mask, 40.0), 1.25, D))
    xi, f, U, Fb, T = _term(host, cases)
    assert (xi == 0.0).all() and (Fb == 0.0).all() and (T == 0.0).all()
    assert np.isfinite(U).all() and np.isfinite(f).all()
    for q, (c, xi0, _) in enumerate(cases):
        assert U[q] == (0.5 * 40.0 * 1.25 * 1.25 if c["kind"] == pr.UMBRELLA else 0.0)


def test_work_is_the_rectangle_rule(host):
    """work_s = work_(s-1) + f_s rate dt: the same three operations in numpy; they may differ by the contraction of the product into
    the sum, 2^-53 of the running size per step"""
    rng = np.random.default_rng(67)
    f = rng.normal(0.0, 50.0, 300)
    rate, dt = 0.37, 0.004
    got = _rows(host(["work", len(f)] + [t for fs in f for t in _num([fs, rate, dt])]))[:, 0]
    want = pr.work_rule(f, rate, dt)
    size = np.cumsum(np.abs(f) * rate * dt)
    assert (np.abs(got - want) <= 2 * EPS * np.arange(1, len(f) + 1) * size).all()
    assert np.abs(want).max() > 0.0


def test_reference_advances_by_one_addition_per_step(host):
    for xi0, rate, dt, n in ((1.5, 0.25, 0.004, 1000), (0.3, -0.1, 0.0025, 777), (2.0, 0.0, 0.005, 10)):
        got = float(host(["advance"] + _num([xi0, rate, dt]) + [n]).split()[0])
        assert got == pr.advance(xi0, rate, dt, n)


def test_group_words_fold_the_coordinates_that_name_the_group(host):
    rng = np.random.default_rng(71)
    pairs = [(0, 1), (1, 2), (3, 1), (2, 0)]
    U, Fb, T = rng.normal(0.0, 5.0, 4), rng.normal(0.0, 9.0, (4, 3)), rng.normal(0.0, 7.0, (4, 6))
    flat = []
    for q, (a, b) in enumerate(pairs):
        flat += [a, b] + _num([U[q]]) + _num(Fb[q]) + _num(T[q])
    for g, M in ((0, 3.5), (1, 1024.25), (2, 0.125), (3, 7.0), (4, 2.0)):
        got = _rows(host(["group", 4] + flat + [g] + _num([M])))[0]
        want = np.zeros(10)
        for q, (a, b) in enumerate(pairs):
            if g in (a, b):
                want[:3] += (1.0 if g == b else -1.0) * Fb[q]
                want[3] += 0.5 * U[q]
                want[4:] += 0.5 * T[q]
        size = np.zeros(10)
        size[:3], size[3], size[4:] = np.abs(Fb).sum(axis=0), np.abs(U).sum(), np.abs(T).sum(axis=0)
        assert (np.abs(got - want / M) <= 8 * EPS * size / M).all()
    # the two ends of a coordinate get opposite forces and equal shares: per unit mass times M they cancel
    one = [0, 1] + _num([U[0]]) + _num(Fb[0]) + _num(T[0])
    wa = _rows(host(["group", 1] + one + [0] + _num([2.0])))[0] * 2.0
    wb = _rows(host(["group", 1] + one + [1] + _num([8.0])))[0] * 8.0
    assert np.array_equal(wa[:3], -wb[:3]) and np.array_equal(wa[3:], wb[3:])
    assert wa[3] + wb[3] == U[0] and np.array_equal(wa[4:] + wb[4:], T[0])


# ---------------------------------------------------------------- the builder
def _table(host, group, n_groups, ci, cd, vsites=()):
    ci, cd = np.asarray(ci, dtype=np.int64).reshape(-1, 5), np.asarray(cd, dtype=np.float64).reshape(-1, 6)
    return _table_raw(host, group, n_groups, len(ci), ci, cd, vsites)


def _table_raw(host, group, n_groups, nc, ci, cd, vsites=()):
    case = ["table", len(group)] + [int(g) for g in group] + [n_groups, nc]
    if 0 < nc <= 64:
        case += [int(t) for t in np.asarray(ci).ravel()] + _num(cd)
    case += [len(vsites)] + [int(v) for v in vsites]
    return host(case)


GOOD_I = [[0, 1, 1, 1, 7], [2, 1, 1, 2, 0], [0, 2, 2, 1, 4]]
GOOD_D = [[50.0, 1.5, 0.1, 0, 0, 0], [20.0, -0.5, 0.0, 1.0, 2.0, -2.0], [3.0, 0.0, 0.0, 0, 0, 0]]


def _good_group():
    g = np.full(2100, -1)
    g[5] = 0
    g[10:1035] = 1                                              # 1025 atoms: a full chunk and one more
    g[[7, 2050]] = 2
    return g


def test_a_good_table_is_group_major_with_chunks_of_one_group(host):
    g = _good_group()
    lines = _table(host, g, 3, GOOD_I, GOOD_D).splitlines()
    assert lines[0] == "table 1028 4"
    ids = [int(t) for t in lines[1].split()[1:]]
    assert ids == [5] + list(range(10, 1035)) + [7, 2050]
    assert [int(t) for t in lines[2].split()[1:]] == [0] + [1] * 1025 + [2, 2]
    assert [int(t) for t in lines[3].split()[1:]] == [0, 1, 0, 1, 1024, 1, 1025, 1, 1, 1026, 2, 2]
    rows = _rows("\n".join(lines[4:]))
    assert np.array_equal(rows[:, :5], GOOD_I)
    assert np.array_equal(rows[:, 5], [50.0, 20.0, 3.0]) and np.array_equal(rows[:, 6], [0.1, 0.0, 0.0])
    assert np.array_equal(rows[:, 10], [1.5, -0.5, 0.0])
    assert np.abs(rows[1, 7:10] - np.array([1.0, 2.0, -2.0]) / 3.0).max() <= 2 * EPS      # normalised by the builder
    assert (rows[0, 7:10] == 0.0).all()
    # a parent of a site may be grouped; the site itself is in no group here
    assert _table(host, g, 3, GOOD_I, GOOD_D, vsites=[6, 5, 7, -1]).startswith("table 1028 4")


def test_every_refusal_names_the_entry_and_the_value(host):
    g = _good_group()

    def ci(row, col, value):
        out = np.array(GOOD_I)
        out[row, col] = value
        return out

    def cd(row, col, value):
        out = np.array(GOOD_D, dtype=np.float64)
        out[row, col] = value
        return out
    bad_group = g.copy(); bad_group[100] = 3
    low_group = g.copy(); low_group[3] = -2
    empty = g.copy(); empty[5] = -1
    cases = {
        "group id too high": (dict(group=bad_group), ERR_INVALID, ["atom 100", "group 3", "outside -1...2"]),
        "group id too low": (dict(group=low_group), ERR_INVALID, ["atom 3", "group -2", "outside -1...2"]),
        "n_groups 0": (dict(n_groups=0), ERR_INVALID, ["n_groups = 0", "1...8"]),
        "n_groups 9": (dict(n_groups=9), ERR_INVALID, ["n_groups = 9", "1...8"]),
        "n_coords 0": (dict(nc=0), ERR_INVALID, ["n_coords = 0", "1...8"]),
        "n_coords 9": (dict(nc=9, ci=np.tile(GOOD_I[0], (9, 1)), cd=np.tile(GOOD_D[0], (9, 1))), ERR_INVALID, ["n_coords = 9", "1...8"]),
        "empty group": (dict(group=empty), ERR_INVALID, ["group 0", "empty"]),
        "a = b": (dict(ci=ci(1, 0, 1)), ERR_INVALID, ["coordinate 1", "group 1 twice"]),
        "group outside the table": (dict(ci=ci(2, 1, 3)), ERR_INVALID, ["coordinate 2", "groups 0 and 3", "outside 0...2"]),
        "group negative": (dict(ci=ci(0, 0, -1)), ERR_INVALID, ["coordinate 0", "groups -1 and 1"]),
        "unknown kind": (dict(ci=ci(0, 2, 3)), ERR_INVALID, ["coordinate 0", "kind 3"]),
        "unknown geometry": (dict(ci=ci(2, 3, 0)), ERR_INVALID, ["coordinate 2", "geometry 0"]),
        "mask 0": (dict(ci=ci(0, 4, 0)), ERR_INVALID, ["coordinate 0", "mask 0", "1...7"]),
        "mask 8": (dict(ci=ci(2, 4, 8)), ERR_INVALID, ["coordinate 2", "mask 8", "1...7"]),
        "zero vector": (dict(cd=cd(1, slice(3, 6), 0.0)), ERR_INVALID, ["coordinate 1", "direction (0, 0, 0)", "zero"]),
        "nan vector": (dict(cd=cd(1, 4, np.nan)), ERR_INVALID, ["coordinate 1", "direction", "nan"]),
        "inf vector": (dict(cd=cd(1, 5, np.inf)), ERR_INVALID, ["coordinate 1", "direction", "inf"]),
        "k nan": (dict(cd=cd(0, 0, np.nan)), ERR_INVALID, ["coordinate 0", "k (or F)", "nan"]),
        "r0 inf": (dict(cd=cd(1, 1, np.inf)), ERR_INVALID, ["coordinate 1", "r0", "inf"]),
        "rate nan": (dict(cd=cd(0, 2, np.nan)), ERR_INVALID, ["coordinate 0", "rate", "nan"]),
        "k negative": (dict(cd=cd(0, 0, -2.5)), ERR_INVALID, ["coordinate 0", "k = -2.5"]),
        "rate with a constant force": (dict(cd=cd(2, 2, 0.25)), ERR_INVALID, ["coordinate 2", "constant force", "rate = 0.25"]),
        "a virtual site in a group": (dict(vsites=[3, 5, 7, -1, 12, 5, 7, 2050]), ERR_STATE,
                                      ["atom 12", "group 1", "virtual site", "emdee_md_set_vsites"]),
    }
    for name, (change, code, words) in cases.items():
        kw = dict(group=g, n_groups=3, nc=3, ci=np.array(GOOD_I), cd=np.array(GOOD_D, dtype=np.float64), vsites=())
        kw.update(change)
        out = _table_raw(host, kw["group"], kw["n_groups"], kw["nc"], kw["ci"], kw["cd"], kw["vsites"])
        assert out.startswith("REFUSED %d set_pull: " % code), (name, out)
        for w in words:
            assert w in out, (name, w, out)
    # a negative force is a force; a constant force along a direction is fine
    along = cd(2, slice(3, 6), [0.0, 0.0, -4.0])
    along[2, 0] = -3.0
    assert _table(host, g, 3, ci(2, 3, 2), along).startswith("table 1028")


def test_the_site_table_refuses_a_site_in_a_pull_group(host):
    """the mirror: emdee_md_set_vsites with a pull table in force"""
    sites, weights = [6, 5, 7, -1, 12, 5, 7, 2050], [0.5, 0.0, 0.3, 0.3]
    pulled = [5] + list(range(10, 1035)) + [7, 2050]
    out = host(["vsites", 2100, 2] + sites + _num(weights) + [len(pulled)] + pulled)
    assert out.startswith("REFUSED %d set_vsites: " % ERR_INVALID), out
    for w in ("atom 12", "entry 1", "pull table", "emdee_md_set_pull"):
        assert w in out, (w, out)
    # parents in a group are fine, and so is a site outside every group
    assert host(["vsites", 2100, 1] + sites[:4] + _num(weights[:2]) + [len(pulled)] + pulled).split() == ["sites", "1"]
