"""CPU tests of the parts of the position restraints with no HIP in them (include/emdee_hip.h: emdee_md_set_restraints): the term of
one atom and the scaling of a reference of emdee.jl_amd/csrc/restraint.hpp and the table builder of emdee.jl_amd/csrc/topology.hpp,
through the stand-alone program tests/c/restraint_host.cpp, built with the host compiler under ASan and UBSan, against the numpy
yardstick tests/helpers/restraint_ref.py; ingest.heavy_atoms on the committed force-field file; and the kernels' resource usage from
`make report`."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import GOLDEN, ROOT
from .helpers import restraint_ref as rr

EPS = 2.0 ** -53
ERR_INVALID, ERR_STATE = -1, -6


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("restraint_host") / "restraint_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "restraint_host.cpp"), "-o", exe]
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


def _term(host, real, d, k, r0):
    n = len(d)
    rec = np.concatenate([d, k, np.asarray(r0).reshape(n, 1)], axis=1)
    out = _rows(host(["term", real, n] + _num(rec)))
    return out[:, 0], out[:, 1:4], out[:, 4:10]


def _cases():
    """harmonic entries with 1, 2 and 3 non-zero axes, d = 0, k = 0; flat-bottomed spheres, cylinders and slabs inside, on and
    outside r0.  Returns d, k, r0 and the index ranges by name."""
    rng = np.random.default_rng(41)
    d, k, r0, where = [], [], [], {}

    def add(name, dd, kk, rr0):
        where[name] = (len(d), len(d) + len(dd))
        d.extend(dd); k.extend(kk); r0.extend(rr0)
    masks = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
    for m in masks:                                             # harmonic: independent constants per axis
        dd = rng.normal(0.0, 1.0, (20, 3)) * 10.0 ** rng.integers(-3, 2, (20, 1))
        add("harmonic%d%d%d" % m, dd, rng.uniform(0.5, 500.0, (20, 3)) * np.array(m), np.zeros(20))
    add("d=0", np.zeros((3, 3)), rng.uniform(1.0, 10.0, (3, 3)), np.zeros(3))
    add("k=0", rng.normal(0.0, 1.0, (3, 3)), np.zeros((3, 3)), np.zeros(3))
    for m in masks:                                             # flat-bottomed: one constant on the masked axes
        u = rng.normal(0.0, 1.0, (30, 3))
        u /= np.sqrt((u * u * np.array(m)).sum(axis=1))[:, None]    # masked norm 1
        rad = rng.uniform(0.2, 2.0, 30)
        rho = rad * np.concatenate([rng.uniform(0.05, 0.95, 10), np.ones(10), rng.uniform(1.05, 4.0, 10)])
        kk = rng.uniform(0.5, 500.0, (30, 1)) * np.array(m, dtype=np.float64)
        add("flat%d%d%d" % m, u * rho[:, None], kk, rad)
    add("flat d=0", np.zeros((2, 3)), np.full((2, 3), 7.0), np.array([0.5, 0.5]))
    return np.array(d), np.array(k), np.array(r0), where


def test_constants_are_the_headers(host):
    assert host(["words"]).split() == ["8"]
    text = open(os.path.join(ROOT, "include", "emdee_hip.h")).read()
    assert re.search(r"#define EMDEE_RESTRAINT_WORDS\s+8\b", text)
    for name in ("emdee_md_set_restraints", "emdee_md_restraint_sums", "emdee_md_get_restraint_refs"):
        assert re.search(r"int32_t %s\(" % name, text), name


@pytest.mark.parametrize("real", ["double", "float"])
def test_term_is_the_numpy_formula(host, real):
    """The arithmetic is fp64 for both instances; f and T are rounded once to `real`.  numpy follows the same formulas; what may
    differ is the order of a three-term sum, contraction of a product into a sum, and the square root and the division of the
    flat-bottomed branch: a handful of roundings of the size of the terms.  Bound: 8 x 2^-53 of the sum of the absolute terms
    (the bound tests/test_gk_host.py derives for seven products and a sum), plus for `float` half an ulp of fp32 for the one rounding
    of the outputs.  Near the rim rho - r0 cancels: its own error is 2^-53 of rho, so f and T, proportional to it, move by k 2^-52 rho
    (times |d| for T); the scale below holds that term."""
    d, k, r0, where = _cases()
    U, f, T = _term(host, real, d, k, r0)
    Ur, fr, Tr = rr.terms(d, k, r0)
    kd = (k * np.abs(d)).sum(axis=1)                            # the size of a force before any cancellation
    dn = np.abs(d).sum(axis=1)
    ulp = 2.0 ** -24 if real == "float" else 0.0
    tol = 8 * EPS
    gap_u = np.abs(U - Ur)
    gap_f = np.abs(f - fr)
    gap_t = np.abs(T - Tr)
    print("%s: largest |U - numpy| / (k d d) = %.2e, |f - numpy| / (k d) = %.2e, |T - numpy| / (k d d) = %.2e (bound %.2e + %.2e)"
          % (real, (gap_u / np.maximum(kd * dn, 1e-300)).max(), (gap_f / np.maximum(kd, 1e-300)[:, None]).max(),
             (gap_t / np.maximum(kd * dn, 1e-300)[:, None]).max(), tol, ulp))
    assert (gap_u <= tol * kd * dn).all()
    assert (gap_f <= tol * kd[:, None] + ulp * np.abs(fr)).all()
    assert (gap_t <= tol * (kd * dn)[:, None] + ulp * np.abs(Tr)).all()
    # exact zeros: d = 0, k = 0, inside and on the rim of a well (no division there)
    for name in ("d=0", "k=0", "flat d=0"):
        lo, hi = where[name]
        assert (U[lo:hi] == 0.0).all() and (f[lo:hi] == 0.0).all() and (T[lo:hi] == 0.0).all(), name
    for name in where:
        if name.startswith("flat") and name != "flat d=0":
            lo = where[name][0]
            assert (U[lo:lo + 10] == 0.0).all() and (f[lo:lo + 10] == 0.0).all() and (T[lo:lo + 10] == 0.0).all(), name   # inside
            assert (f[lo + 20:lo + 30] != 0.0).any(axis=1).all() and (U[lo + 20:lo + 30] > 0.0).all(), name               # outside
            # on the rim (rho = r0 up to the rounding of the construction): nothing, or the first ulps of the ramp
            # (rho = r0 to the six roundings of its construction here and its evaluation there)
            rim_f = np.abs(f[lo + 10:lo + 20]).max(axis=1)
            assert (rim_f <= 16 * EPS * kd[lo + 10:lo + 20] + 1e-300).all(), name
    # the force never has a component on an axis whose constant is 0
    assert (f[k == 0.0] == 0.0).all()
    # trace T = d . f, in the outputs' own precision
    dot = (d * f).sum(axis=1)
    assert (np.abs(T[:, :3].sum(axis=1) - dot) <= (8 * EPS + 4 * ulp) * kd * dn).all()


def test_force_is_the_centred_difference_of_the_energy(host):
    """Harmonic terms are quadratic in d: (U(d + h) - U(d - h)) / 2h = -f exactly, up to the rounding of the operands -- U carries
    2^-53 of k (|d| + h)^2 / 2 per evaluation (three roundings each: square, product, sum), and the difference is divided by 2h.
    Flat-bottomed terms are quadratic in rho only along the radial direction; off it the curvature k (1 - r0 / rho) enters at h^2,
    so the step is small, h = 1e-5 of max(|d|, 1), the points keep |rho - r0| >= 0.01 >> h (the kink is not straddled), and the
    bound adds the truncation k h^2 / rho to the rounding term."""
    d, k, r0, where = _cases()
    keep = np.ones(len(d), dtype=bool)
    for name, (lo, hi) in where.items():
        if name.startswith("flat") and name != "flat d=0":
            keep[lo + 10:lo + 20] = False                       # on the rim: the kink
    keep[where["flat d=0"][0]:where["flat d=0"][1]] = True
    d, k, r0 = d[keep], k[keep], r0[keep]
    _, f, _ = _term(host, "double", d, k, r0)
    size = np.sqrt((d * d).sum(axis=1))
    rho = np.sqrt((d * d * (k > 0.0)).sum(axis=1))             # the norm over the axes with a constant
    h = np.where(r0 > 0.0, 1e-5, 2.0 ** -3) * np.maximum(size, 1.0)
    h = 2.0 ** np.round(np.log2(h))                             # a power of two: d +- h and the division by 2h round nothing away
    kmax = k.max(axis=1)
    for a in range(3):
        e = np.zeros(3); e[a] = 1.0
        Up, _, _ = _term(host, "double", d + h[:, None] * e, k, r0)
        Um, _, _ = _term(host, "double", d - h[:, None] * e, k, r0)
        slope = (Up - Um) / (2.0 * h)
        rounding = 16 * EPS * kmax * (size + h) ** 2 / (2.0 * h)
        # (the third derivatives of k (rho - r0)^2 / 2 are at most 3 k r0 / rho^2 < 3 k / rho outside the well: h^2 / 6 of that)
        truncation = np.where(r0 > 0.0, kmax * h * h / np.maximum(rho, 1e-300), 0.0)
        gap = np.abs(slope + f[:, a])
        print("axis %d: largest |dU/dd + f| / bound = %.3f" % (a, (gap / np.maximum(rounding + truncation, 1e-300)).max()))
        assert (gap <= rounding + truncation).all()


def test_scaled_reference_keeps_d_proportional(host):
    """ref' = lo + mu (ref - lo); an atom scaled the same way, x' = lo + mu (x - lo), keeps d' = x' - ref' = mu d: four roundings
    of numbers of the size of mu |x - lo| and mu |ref - lo|"""
    rng = np.random.default_rng(43)
    n = 200
    ref, x = rng.uniform(-30.0, 30.0, n), rng.uniform(-30.0, 30.0, n)
    lo, mu = rng.uniform(-5.0, 5.0, n), rng.uniform(0.8, 1.25, n)
    got = _rows(host(["scale", n] + _num(np.stack([ref, lo, mu], axis=1))))[:, 0]
    want = rr.scale_ref(ref, lo, mu)
    assert (np.abs(got - want) <= 2 * EPS * (np.abs(lo) + mu * np.abs(ref - lo))).all()
    xs = lo + mu * (x - lo)
    size = np.abs(lo) + mu * (np.abs(x - lo) + np.abs(ref - lo))
    assert (np.abs((xs - got) - mu * (x - ref)) <= 6 * EPS * size).all()
    # mu = 1 moves nothing but the rounding of lo + (ref - lo)
    same = _rows(host(["scale", n] + _num(np.stack([ref, lo, np.ones(n)], axis=1))))[:, 0]
    assert (np.abs(same - ref) <= 2 * EPS * (np.abs(lo) + np.abs(ref - lo))).all()


# ---------------------------------------------------------------- the builder
def _table(host, lim, ids, k, ref=None, flat=None, vsites=()):
    n = len(ids)
    case = ["table", lim, n] + [int(i) for i in ids]
    case += [0] if ref is None else [n] + _num(ref)
    case += _num(k)
    case += [0] if flat is None else [n] + _num(flat)
    case += [len(vsites)] + [int(v) for v in vsites]
    return host(case)


def test_a_good_table_comes_back_in_caller_order(host):
    ids = [7, 2, 9, 0, 4]
    rng = np.random.default_rng(47)
    ref, k = rng.uniform(-20.0, 20.0, (5, 3)), rng.uniform(0.0, 9.0, (5, 3))
    k[1] = [0.0, 3.0, 3.0]; k[3] = [5.0, 0.0, 0.0]
    flat = np.array([0.0, 0.4, 0.0, 1.5, 0.0])
    lines = _table(host, 10, ids, k, ref, flat, vsites=[5, 0, 2, 9, 6, 7, 9, -1]).splitlines()   # (sites 5 and 6; 0, 2, 9, 7 are parents)
    assert lines[0] == "table 5"
    got = _rows("\n".join(lines[1:]))
    assert np.array_equal(got[:, 0], ids) and np.array_equal(got[:, 1:4], ref) and np.array_equal(got[:, 4:7], k)
    assert np.array_equal(got[:, 7], flat)
    # no references (the engine fills them), no radii (all zero)
    lines = _table(host, 10, ids, k).splitlines()
    got = _rows("\n".join(lines[1:]))
    assert lines[0] == "table 5" and np.array_equal(got[:, 0], ids) and (got[:, 7] == 0.0).all()
    assert _table(host, 10, [], np.zeros((0, 3))).splitlines() == ["table 0"]


def test_every_refusal_names_the_entry(host):
    ids = [7, 2, 9, 0]
    k = np.full((4, 3), 2.0)
    ref = np.zeros((4, 3))

    def with_(arr, row, col, value):
        out = np.array(arr, dtype=np.float64)
        if col is None:
            out[row] = value
        else:
            out[row, col] = value
        return out
    cases = {
        "id too high": (dict(ids=[7, 2, 10, 0]), ERR_INVALID, ["entry 2", "id 10", "outside [0, 10)"]),
        "id negative": (dict(ids=[7, -1, 9, 0]), ERR_INVALID, ["entry 1", "id -1", "outside"]),
        "named twice": (dict(ids=[7, 2, 9, 7]), ERR_INVALID, ["atom 7", "twice", "entries 0 and 3"]),
        "k negative": (dict(k=with_(k, 2, 1, -1.0)), ERR_INVALID, ["entry 2", "atom 9", "spring constant", "axis 1"]),
        "k nan": (dict(k=with_(k, 1, 0, np.nan)), ERR_INVALID, ["entry 1", "atom 2", "spring constant", "axis 0"]),
        "k inf": (dict(k=with_(k, 3, 2, np.inf)), ERR_INVALID, ["entry 3", "atom 0", "spring constant", "axis 2"]),
        "r0 negative": (dict(flat=[0.0, -0.1, 0.0, 0.0]), ERR_INVALID, ["entry 1", "atom 2", "radius"]),
        "r0 nan": (dict(flat=[0.0, 0.0, np.nan, 0.0]), ERR_INVALID, ["entry 2", "atom 9", "radius"]),
        "r0 inf": (dict(flat=[np.inf, 0.0, 0.0, 0.0]), ERR_INVALID, ["entry 0", "atom 7", "radius"]),
        "ref nan": (dict(ref=with_(ref, 3, 0, np.nan)), ERR_INVALID, ["entry 3", "atom 0", "reference", "axis 0"]),
        "ref inf": (dict(ref=with_(ref, 0, 2, -np.inf)), ERR_INVALID, ["entry 0", "atom 7", "reference", "axis 2"]),
        "flat, unequal": (dict(k=with_(k, 1, None, [2.0, 3.0, 0.0]), flat=[0.0, 0.5, 0.0, 0.0]), ERR_INVALID,
                          ["entry 1", "atom 2", "unequal"]),
        "flat, no constant": (dict(k=with_(k, 2, None, [0.0, 0.0, 0.0]), flat=[0.0, 0.0, 0.5, 0.0]), ERR_INVALID,
                              ["entry 2", "atom 9", "no non-zero"]),
        "a virtual site": (dict(vsites=[9, 1, 3, -1]), ERR_STATE, ["atom 9", "entry 2", "virtual site", "emdee_md_set_vsites"]),
    }
    for name, (change, code, words) in cases.items():
        kw = dict(ids=ids, k=k, ref=ref, flat=None, vsites=())
        kw.update(change)
        out = _table(host, 10, kw["ids"], kw["k"], kw["ref"], kw["flat"], kw["vsites"])
        assert out.startswith("REFUSED %d set_restraints: " % code), (name, out)
        for w in words:
            assert w in out, (name, w, out)
    # a parent of a site may be restrained, and unequal constants without a flat bottom are the per-axis harmonic term
    assert _table(host, 10, ids, with_(k, 1, None, [2.0, 3.0, 0.0]), ref, None, vsites=[5, 7, 2, 9]).startswith("table 4")


# ---------------------------------------------------------------- the selection
def test_heavy_atoms_on_the_fixture(emdee):
    ing = emdee.ingest
    xml = os.path.join(GOLDEN, "dibenzo-p-dioxin-in-water.xml")
    table, templates = ing.BondedTable(xml), ing.ResidueTemplates(xml)
    types, bonds = templates.build(["HOH", "aaa", "HOH", "HOH"])
    mol, _ = ing.rigid_triatomics(types, bonds, table)
    assert len(mol) == 3
    heavy = ing.heavy_atoms(types, table, skip=mol)
    names = templates.residues["aaa"]["names"]
    want = [3 + i for i, nm in enumerate(names) if not nm.startswith("H")]
    assert heavy.dtype == np.int64 and heavy.tolist() == want and len(want) == 14          # twelve carbons, two oxygens
    assert all(table.elements[types[i]] in ("C", "O") for i in heavy)
    # without skip the water oxygens come too; hydrogens never
    every = ing.heavy_atoms(types, table)
    assert every.tolist() == sorted(want + [int(m[0]) for m in mol])
    assert ing.heavy_atoms(types, table, skip=np.arange(len(types))).tolist() == []


# ---------------------------------------------------------------- the kernels
def test_restraint_kernels_are_in_the_report_and_use_no_scratch_memory():
    """`make report` (hipcc -Rpass-analysis=kernel-resource-usage on both kernel translation units, cross-compiled: no GPU needed):
    the kernels of the restraints are there in both precisions -- the sums as reduce.hpp's two stages over RestraintSums -- and keep
    nothing in scratch"""
    src = os.path.join(ROOT, "emdee.jl_amd", "csrc")
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-s", "-C", src, "report"], timeout=1500)
    seen = {}
    for name in ("resource_usage_f64.txt", "resource_usage_f32.txt"):
        text = open(os.path.join(src, name)).read()
        for b in re.split(r"remark: Function Name: ", text)[1:]:
            fn = b.split(" ", 1)[0].strip()
            if "k_restraint" not in fn and "RestraintSums" not in fn and "k_reduce_final" not in fn:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
            assert m is not None, fn
            assert int(m.group(1)) == 0, "%s keeps %s bytes per lane in scratch memory" % (fn, m.group(1))
            seen.setdefault(name, set()).add(fn)
    for name, real in (("resource_usage_f64.txt", "Id"), ("resource_usage_f32.txt", "If")):
        fns = seen.get(name, set())
        for kernel in ("k_restraints" + real + "Lb0", "k_restraints" + real + "Lb1", "k_restraint_capture" + real,
                       "k_reduce_partialsINS_13RestraintSums" + real, "k_restraint_scale", "k_reduce_final"):
            assert any(kernel in f for f in fns), (name, kernel, sorted(fns))
