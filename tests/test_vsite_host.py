"""CPU tests of virtual interaction sites (include/emdee_hip.h: emdee_md_set_vsites): placement and per-parent force spreading of
emdee.jl_amd/csrc/vsite.hpp and the table builders of csrc/topology.hpp through the stand-alone program tests/c/vsite_host.cpp,
built with the host compiler under ASan and UBSan, against the numpy of tests/helpers/vsite_ref.py; and ingest.bisector_sites.

Bounds.  Every output is one short fp64 sum of products (a site: x_a plus two products; a parent: its force plus one product per
entry, here at most a dozen), so it carries a few roundings of its largest term: 8 eps of the sum of the terms' magnitudes."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import vsite_ref as vr

ERR_INVALID = -1
EPS = float(np.finfo(np.float64).eps)
N_ATOMS, N = 260, 200
LENGTHS = np.array([7.0, 7.5, 8.2])


@pytest.fixture(scope="session")
def vsite_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vsite_host") / "vsite_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "vsite_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _num(v):
    return [repr(float(t)) for t in np.ravel(v)]


def _ints(v):
    return [int(t) for t in np.ravel(v)]


@pytest.fixture(scope="session")
def entries():
    """200 random entries over 260 atoms: ids 0 .. 199 are the sites, 200 .. 259 the 60 parents (so every parent is shared by about
    ten sites); every third entry has two parents (its w_c is NaN: ignored); weights uniform in [-0.5, 1.5], outside [0, 1]
    for about half of them; positions anywhere within +-3 box lengths, forces of order 1 to 100."""
    rng = np.random.default_rng(17)
    atoms = np.empty((N, 4), dtype=np.int64)
    atoms[:, 0] = rng.permutation(N)
    for s in range(N):
        atoms[s, 1:] = 200 + rng.choice(60, 3, replace=False)
    atoms[::3, 3] = -1
    weights = rng.uniform(-0.5, 1.5, (N, 2))
    weights[::3, 1] = np.nan
    x = sr_lo() + rng.uniform(-3.0, 4.0, (N_ATOMS, 3)) * LENGTHS
    f = rng.normal(size=(N_ATOMS, 3)) * rng.choice([1.0, 10.0, 100.0], (N_ATOMS, 1))
    assert ((weights[:, 0] < 0) | (weights[:, 0] > 1)).sum() > 50
    return dict(atoms=atoms, weights=weights, x=x, f=f)


def sr_lo():
    return np.array([-1.0, 0.5, 2.0])


def _table_args(E):
    return [N] + _ints(E["atoms"]) + _num(E["weights"])


def _rows(out, n):
    rows = np.array([[float(t) for t in line.split()] for line in out.splitlines()])
    assert rows.shape == (n, 3), out[:200]
    return rows


@pytest.fixture(scope="session")
def spread_host(vsite_host, entries):
    E = entries
    return _rows(vsite_host(["spread", N_ATOMS] + _num(E["f"]) + _table_args(E)), N_ATOMS)


def test_placement_matches_numpy(vsite_host, entries):
    E = entries
    got = _rows(vsite_host(["place"] + _num(LENGTHS) + [1, 1, 1, N_ATOMS] + _num(E["x"]) + _table_args(E)), N)
    want = vr.place(E["x"], E["atoms"], E["weights"], LENGTHS)
    w = vr.parent_weights(E["atoms"], E["weights"])
    scale = np.abs(E["x"][E["atoms"][:, 1]]) + (np.abs(w[:, 1:2]) + np.abs(w[:, 2:3])) * 0.5 * LENGTHS
    err = np.abs(got - want) / scale
    print("placement: largest |x - x_numpy| / (|x_a| + (|w_b| + |w_c|) L / 2) = %.3e (bound %.3e)" % (err.max(), 8 * EPS))
    assert err.max() <= 8 * EPS
    # a site lies within (|w_b| + |w_c|) L sqrt(3) / 2 of its a: the minimum image was taken (parents are up to 7 L apart as loaded)
    far = np.linalg.norm(got - E["x"][E["atoms"][:, 1]], axis=1)
    assert (far <= (np.abs(w[:, 1]) + np.abs(w[:, 2])) * 0.5 * np.linalg.norm(LENGTHS) * (1 + 1e-12)).all()
    # an open axis takes no image
    open_x = _rows(vsite_host(["place"] + _num(LENGTHS) + [0, 1, 1, N_ATOMS] + _num(E["x"]) + _table_args(E)), N)
    assert np.abs(open_x - vr.place(E["x"], E["atoms"], E["weights"], LENGTHS, (0, 1, 1))).max() <= 8 * EPS * np.abs(E["x"]).max() * 4


def _term_scale(E):
    """(N_ATOMS, 3): |f_p| + sum over the parent's entries of |w| |f_site|: the magnitude of the terms of each output"""
    w = vr.parent_weights(E["atoms"], E["weights"])
    scale = np.abs(E["f"]).copy()
    for s in range(N):
        for k in range(3):
            if E["atoms"][s, 1 + k] >= 0:
                scale[E["atoms"][s, 1 + k]] += abs(w[s, k]) * np.abs(E["f"][E["atoms"][s, 0]])
    return scale


def test_spreading_matches_numpy_and_clears_the_sites(entries, spread_host):
    E = entries
    want = vr.spread(E["f"], E["atoms"], E["weights"])
    err = np.abs(spread_host - want) / _term_scale(E)
    print("spreading: largest |f - f_numpy| / sum |terms| = %.3e (bound %.3e)" % (err.max(), 8 * EPS))
    assert err.max() <= 8 * EPS
    assert (spread_host[E["atoms"][:, 0]] == 0.0).all()
    assert np.isfinite(spread_host).all()                                        # (the NaN w_c of the two-parent entries was never read)


def test_spreading_conserves_total_force_and_torque(entries, spread_host):
    """Torque about the origin, with the parents unwrapped about each site's a and the site placed by numpy: sum_k x_k x (w_k f) =
    x_s x f holds per entry on unwrapped coordinates, so the test moves every site's force to a private copy of its parents."""
    E = entries
    total_before, total_after = E["f"].sum(axis=0), spread_host.sum(axis=0)
    bound = 8 * EPS * _term_scale(E).sum(axis=0)
    print("total force: before - after = %s (bound %s)" % (np.abs(total_before - total_after), bound))
    assert (np.abs(total_before - total_after) <= bound).all()
    # torque: what each entry's spreading adds, on that entry's own unwrapped frame
    w = vr.parent_weights(E["atoms"], E["weights"])
    xs = vr.place(E["x"], E["atoms"], E["weights"], LENGTHS)
    worst = 0.0
    for s in range(N):
        a = E["atoms"][s]
        fs = E["f"][a[0]]
        xa = E["x"][a[1]]
        parents = [xa] + [xa + vr._image(E["x"][g] - xa, LENGTHS, (1, 1, 1)) for g in a[2:] if g >= 0]
        torque = sum(np.cross(xp, w[s, k] * fs) for k, xp in enumerate(parents))
        scale = sum(np.abs(xp).max() * abs(w[s, k]) for k, xp in enumerate(parents)) * np.abs(fs).max()
        worst = max(worst, np.abs(torque - np.cross(xs[s], fs)).max() / scale)
    print("torque: largest |sum x_k x (w_k f) - x_s x f| / sum |x_k| |w_k| |f| = %.3e (bound %.3e)" % (worst, 16 * EPS))
    assert worst <= 16 * EPS


def test_spreading_is_the_chain_rule_of_a_potential_of_the_site_positions(vsite_host, entries):
    """U = sum_s 1/2 k_s |x_s - c_s|^2 with x_s the placed sites: f_site = -k_s (x_s - c_s), and -dU/dx_p of a parent is the sum
    of w f_site over its entries -- what spreading gives a parent whose own force is 0."""
    E = entries
    rng = np.random.default_rng(23)
    k, c = rng.uniform(0.5, 2.0, N), rng.normal(size=(N, 3))
    xs = vr.place(E["x"], E["atoms"], E["weights"], LENGTHS)
    f = np.zeros((N_ATOMS, 3))
    f[E["atoms"][:, 0]] = -k[:, None] * (xs - c)
    got = _rows(vsite_host(["spread", N_ATOMS] + _num(f) + _table_args(E)), N_ATOMS)
    # the analytic gradient, parent by parent: dx_s / dx_p is w times the identity (the minimum image is locally a shift)
    w = vr.parent_weights(E["atoms"], E["weights"])
    want, scale = np.zeros((N_ATOMS, 3)), np.zeros((N_ATOMS, 3))
    for s in range(N):
        for q in range(3):
            g = E["atoms"][s, 1 + q]
            if g >= 0:
                want[g] += w[s, q] * f[E["atoms"][s, 0]]
                scale[g] += abs(w[s, q]) * np.abs(f[E["atoms"][s, 0]])
    parents = np.unique(E["atoms"][:, 1:][E["atoms"][:, 1:] >= 0])
    err = np.abs(got[parents] - want[parents]) / scale[parents].max(axis=1, keepdims=True)
    print("chain rule: largest |f_parent + dU/dx_parent| / largest term = %.3e (bound %.3e)" % (err.max(), 16 * EPS))
    assert err.max() <= 16 * EPS                                                 # (a dozen terms: a few ulp of the largest)
    # ... and a central difference of U itself agrees to the difference's own error (U is quadratic: exact up to rounding)
    def U(x):
        return 0.5 * (k * ((vr.place(x, E["atoms"], E["weights"], LENGTHS) - c) ** 2).sum(axis=1)).sum()
    h = 1e-4
    for g in parents[:5]:
        for d in range(3):
            xp, xm = E["x"].copy(), E["x"].copy()
            xp[g, d] += h
            xm[g, d] -= h
            fd = -(U(xp) - U(xm)) / (2 * h)
            assert abs(fd - got[g, d]) <= 1e-7 * max(1.0, abs(got[g, d])) + 1e-9 * abs(U(E["x"])) / h


def _table(vsite_host, lim, atoms, weights, rigid=(), hbonds=()):
    atoms, weights = np.asarray(atoms).reshape(-1, 4), np.asarray(weights, dtype=np.float64).reshape(-1, 2)
    return vsite_host(["table", lim, atoms.shape[0]] + _ints(atoms) + _num(weights) + [len(rigid)] + _ints(rigid) + [len(hbonds)] + _ints(hbonds))


GOOD = ([[9, 0, 1, 2], [10, 3, 1, -1], [11, 0, 4, 5]], [[0.13, 0.13], [1.5, float("nan")], [-0.2, 0.4]])


def test_a_table_that_passes_and_the_order_of_the_parent_list(vsite_host):
    out = _table(vsite_host, 12, *GOOD, rigid=[0, 1, 2], hbonds=[3, 4, -1, -1]).splitlines()   # (parents may be constrained)
    assert out[0] == "table 3 ids 9 0 1 2 10 3 1 -1 11 0 4 5"
    assert out[1] == "virtual site 0 (atoms 9 0 1 2): message"
    assert [float(t) for t in out[2].split()[1:]] == [0.13, 0.13, 1.5, 0.0, -0.2, 0.4]       # (the ignored w_c became 0)
    parents, start, ent = vr.parent_list(*GOOD)
    assert out[3] == "parents " + " ".join(str(p) for p in parents) == "parents 0 1 2 3 4 5"
    assert out[4] == "start " + " ".join(str(s) for s in start) == "start 0 2 4 5 6 7 8"
    got = out[5].split()[1:]
    assert [int(t) for t in got[0::2]] == [e[0] for e in ent] == [0, 2, 0, 1, 0, 1, 2, 2]   # (per parent: its entries in table order)
    assert np.allclose([float(t) for t in got[1::2]], [e[1] for e in ent], rtol=0, atol=2 * EPS)
    assert [float(t) for t in got[1::2]][:2] == [1.0 - 0.13 - 0.13, 1.0 - (-0.2) - 0.4]
    assert _table(vsite_host, 12, [], []).splitlines()[0] == "table 0 ids"


def test_every_refusal_of_the_builder(vsite_host):
    ids, w = GOOD

    def changed(s, k, value):
        out = [list(r) for r in ids]
        out[s][k] = value
        return out
    refused = {
        "id too high": (changed(0, 2, 12), w, {}, "outside"),
        "site too high": (changed(0, 0, 12), w, {}, "outside"),
        "negative site": (changed(0, 0, -1), w, {}, "outside"),
        "negative a": (changed(0, 1, -1), w, {}, "outside"),
        "negative b": (changed(1, 2, -1), w, {}, "outside"),
        "c below -1": (changed(0, 3, -2), w, {}, "outside"),
        "twice within an entry (parents)": (changed(0, 3, 0), w, {}, "twice"),
        "twice within an entry (site)": (changed(0, 2, 9), w, {}, "twice"),
        "a site in two entries": (changed(1, 0, 9), w, {}, "two entries"),
        "a site that is a parent": (changed(2, 2, 10), w, {}, "is a parent"),
        "a site of the rigid table": (ids, w, dict(rigid=[6, 9, 7]), "rigid table"),
        "a site of the hbonds table": (ids, w, dict(hbonds=[6, 10, -1, -1]), "hbonds table"),
        "nan w_b": (ids, [[float("nan"), 0.1]] + w[1:], {}, "finite"),
        "infinite w_c of a three-parent site": (ids, [[0.1, float("inf")]] + w[1:], {}, "finite"),
        "infinite w_b of a two-parent site": (ids, [w[0], [float("inf"), 0.0], w[2]], {}, "finite"),
    }
    for name, (a, ww, kw, word) in refused.items():
        out = _table(vsite_host, 12, a, ww, **kw)
        assert out.startswith("REFUSED %d " % ERR_INVALID) and word in out, (name, out)


def test_the_two_constraint_builders_refuse_an_atom_that_is_a_site(vsite_host):
    vs = [9, 0, 1, 2, 10, 3, 1, -1]
    ok = vsite_host(["rigid", 12, 1, 0, 1, 2, 0.32, 0.5, len(vs)] + vs)
    assert ok.splitlines()[0] == "table 1"                                       # (parents may be rigid)
    out = vsite_host(["rigid", 12, 1, 0, 9, 2, 0.32, 0.5, len(vs)] + vs)
    assert out.startswith("REFUSED %d " % ERR_INVALID) and "virtual site" in out and "atom 9 " in out, out
    assert vsite_host(["rigid", 12, 1, 0, 9, 2, 0.32, 0.5, 0]).splitlines()[0] == "table 1"      # (no site table in force)
    ok = vsite_host(["hbonds", 12, 1, 3, 1, -1, -1, 0.3, 0.0, 0.0, len(vs)] + vs)
    assert ok.splitlines()[0] == "table 1"
    out = vsite_host(["hbonds", 12, 1, 3, 10, -1, -1, 0.3, 0.0, 0.0, len(vs)] + vs)
    assert out.startswith("REFUSED %d " % ERR_INVALID) and "virtual site" in out and "atom 10 " in out, out


def test_bisector_sites_gives_the_weights_of_the_tip4p_family(emdee):
    ingest = emdee.ingest
    # TIP4P/2005: r_OH = 0.9572, HOH = 104.52 degrees, d_OM = 0.1546 (Angstrom)
    d_leg, theta, d_om = 0.9572, np.deg2rad(104.52), 0.1546
    d_base = 2.0 * d_leg * np.sin(0.5 * theta)
    atoms, weights = ingest.bisector_sites([3, 7], [[0, 1, 2], [4, 5, 6]], d_leg, d_base, d_om)
    assert atoms.dtype == np.int32 and atoms.tolist() == [[3, 0, 1, 2], [7, 4, 5, 6]]
    assert weights.shape == (2, 2) and np.array_equal(weights[:, 0], weights[:, 1])
    assert weights[0, 0] == pytest.approx(d_om / (2.0 * d_leg * np.cos(0.5 * theta)), rel=1e-14)
    assert 0.1319 < weights[0, 0] < 0.1320                                       # (the a = b that TIP4P/2005 topologies print)
    # the placed site lies d_om from the apex, on the bisector
    x = np.array([[0.0, 0.0, 0.0], [d_leg * np.sin(0.5 * theta), d_leg * np.cos(0.5 * theta), 0.0],
                  [-d_leg * np.sin(0.5 * theta), d_leg * np.cos(0.5 * theta), 0.0], [0.0, 0.0, 0.0]])
    site = vr.place(x, atoms[:1], weights[:1], [50.0] * 3)[0]
    assert np.abs(site - [0.0, d_om, 0.0]).max() <= 4 * EPS
    with pytest.raises(ValueError):
        ingest.bisector_sites([3], [[0, 1, 2]], 0.25, 0.5, 0.1)
    with pytest.raises(ValueError):
        ingest.bisector_sites([3, 4], [[0, 1, 2]], 0.32, 0.5, 0.1)
