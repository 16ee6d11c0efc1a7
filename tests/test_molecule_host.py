"""CPU tests of the parts of whole-molecule pressure and scaling with no HIP in them (include/emdee_hip.h: emdee_md_set_molecules): the
centre of mass, the entry's share of the molecular sums and the entry's shift of emdee.jl_amd/csrc/molecule.hpp, and the table builder
of emdee.jl_amd/csrc/topology.hpp with its refusals and the mirror refusals of the constraint setters, through the stand-alone program
tests/c/molecule_host.cpp, built with the host compiler under ASan and UBSan, against the numpy yardstick
tests/helpers/molecule_ref.py and, on a triangle, against settle.hpp's own molecule_sums and molecule_scale."""
import os
import re
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import molecule_ref as gr
from .helpers import shake_ref as hr

ERR_INVALID = -1
REL = 1e-13
MU, LO, VSCALE = np.array([1.013, 0.991, 1.004]), hr.LO, 0.97


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("molecule_host") / "molecule_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "molecule_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _num(v):
    return [repr(float(t)) for t in np.asarray(v, dtype=np.float64).ravel()]


def _table(host, ids, lim=None, rigid=(), hbonds=()):
    ids, rigid, hbonds = list(ids), np.asarray(rigid, dtype=np.int64).reshape(-1, 3), np.asarray(hbonds, dtype=np.int64).reshape(-1, 4)
    out = host(["table", len(ids)] + ids + [len(ids) if lim is None else lim, len(rigid)] + list(rigid.ravel()) + [len(hbonds)] + list(hbonds.ravel()))
    if out.startswith("REFUSED"):
        return out
    lines = out.splitlines()
    t = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in lines[1:]}
    t["n_mol"], t["n_small"] = (int(v) for v in lines[0].split()[1:])
    return t


def _refused(out, *words):
    assert out.startswith("REFUSED %d " % ERR_INVALID), out
    for w in words:
        assert w in out, (w, out)
    return out


def test_constants_and_the_header(host):
    assert host(["words"]).split() == ["8", "7", "10"]
    text = open(os.path.join(ROOT, "include", "emdee_hip.h")).read()
    assert re.search(r"int32_t emdee_md_set_molecules\(emdee_md \*md, const int32_t \*molecule_dev, int32_t n\);", text)
    for phrase in ("THE CALLER LOADS EVERY MOLECULE WHOLE", "not loaded whole", "a molecule of one"):
        assert phrase in text, phrase


# ---------------------------------------------------------------- the table
def test_ids_are_compacted_in_order_of_first_appearance_and_the_table_is_ordered_by_size_class(host):
    """ids neither dense nor ordered; molecules of sizes 1 (an id >= 0 of its own and a -1), 2, 3, 8, 9 and 12, interleaved"""
    sizes = {50: 9, 7: 2, 900: 12, 3: 8, 41: 3, 8: 2, 600: 1, 13: 3}
    order = [50, 7, 900, 3, 41, 8, 600, 13]                                  # first appearance
    ids = []
    left = dict(sizes)
    while any(left.values()):                                                # round robin: the molecules interleave
        for k in order:
            if left[k]:
                ids.append(k); left[k] -= 1
        ids.append(-1)
    t = _table(host, ids)
    n = len(ids)
    atoms_of = {k: [a for a in range(n) if ids[a] == k] for k in order}
    # compaction: every atom has a number, numbers follow the first atom
    first_seen = []
    for a in range(n):
        c = t["compact"][a]
        if c not in first_seen:
            first_seen.append(c)
    assert first_seen == list(range(len(first_seen))) and len(first_seen) == len(order) + ids.count(-1)
    assert all(len({t["compact"][a] for a in atoms_of[k]}) == 1 for k in order)
    # the table: singletons dropped; small by size then first atom, then large by first atom
    want = [7, 8, 41, 13, 3, 50, 900]
    assert t["n_mol"] == 7 and t["n_small"] == 5 and t["label"] == want
    assert t["start"] == list(np.cumsum([0] + [sizes[k] for k in want]))
    assert t["atoms"] == [a for k in want for a in atoms_of[k]]              # caller ids ascending within a molecule
    assert t["entry_mol"] == [m for m, k in enumerate(want) for _ in range(sizes[k])]
    assert [t["mol_of"][a] for a in range(n)] == [want.index(ids[a]) if ids[a] in want else -1 for a in range(n)]
    assert t["member"] == [1 if ids[a] in want else 0 for a in range(n)]
    # the order depends on the table alone: the same ids under other names
    rename = {k: 10 * q for q, k in enumerate(order)}
    t2 = _table(host, [rename.get(k, -1) for k in ids])
    assert all(t2[k] == t[k] for k in ("start", "atoms", "entry_mol", "mol_of", "compact", "member"))
    # all at -1: an empty table
    t0 = _table(host, [-1] * 5)
    assert t0["n_mol"] == 0 and t0["start"] == [0] and t0["atoms"] == [] and t0["member"] == [0] * 5


def test_every_invalid_table_is_refused_with_names(host):
    _refused(_table(host, [0, 0, 1], lim=4), "3 ids", "4 atoms")
    _refused(_table(host, [0, 0, -2, 1]), "atom 2", "-2")
    rigid, hbonds = [[0, 1, 2], [3, 4, 5]], [[6, 7, 8, -1], [9, 10, -1, -1]]
    good = [5, 5, 5, 9, 9, 9, 4, 4, 4, 4, 4, -1]
    assert _table(host, good, rigid=rigid, hbonds=hbonds)["n_mol"] == 3
    bad = list(good); bad[4] = 5
    _refused(_table(host, bad, rigid=rigid, hbonds=hbonds), "rigid molecule 1", "atoms 3 4 5", "atom 3 is in molecule 9", "atom 4 in molecule 5",
             "emdee_md_set_rigid3")
    bad = list(good); bad[10] = 77
    _refused(_table(host, bad, rigid=rigid, hbonds=hbonds), "hbonds cluster 1", "atoms 9 10", "atom 10 in molecule 77", "emdee_md_set_hbonds")
    bad = list(good); bad[6] = bad[7] = bad[8] = -1
    _refused(_table(host, bad, rigid=rigid, hbonds=hbonds), "hbonds cluster 0", "atoms 6 7 8", "atom 6 in no molecule", "-1")
    bad = list(good); bad[2] = -1
    _refused(_table(host, bad, rigid=rigid, hbonds=hbonds), "rigid molecule 0", "atom 2 in no molecule")


def test_the_constraint_setters_refuse_what_the_table_in_force_splits(host):
    mol = [5, 5, 5, 9, 9, 9, 4, 4, -1, -1]
    assert host(["mirror", "rigid", len(mol)] + mol + [2, 0, 1, 2, 3, 4, 5]).strip() == "ok"
    assert host(["mirror", "hbonds", len(mol)] + mol + [2, 6, 7, -1, -1, 3, 4, 5, -1]).strip() == "ok"
    _refused(host(["mirror", "rigid", len(mol)] + mol + [2, 0, 1, 2, 3, 4, 6]), "set_rigid3", "rigid molecule 1", "atoms 3 4 6", "atom 6 in molecule 4",
             "molecule table", "emdee_md_set_molecules")
    _refused(host(["mirror", "hbonds", len(mol)] + mol + [1, 7, 8, -1, -1]), "set_hbonds", "hbonds cluster 0", "atoms 7 8", "atom 8 in no molecule")
    _refused(host(["mirror", "hbonds", len(mol)] + mol + [1, 8, 9, -1, -1]), "hbonds cluster 0", "atom 8 in no molecule")
    text = host(["message", 6, 3, 3, -1, 12, 12, 12, 1])
    assert "molecule 12" in text and "atoms 3 4 5" in text and "mass is 0" in text


# ---------------------------------------------------------------- the arithmetic
def _system(host, ids, mass, r, k, v, f, lengths):
    n = len(ids)
    rows = []
    for a in range(n):
        rows += _num([mass[a]]) + _num(r[a]) + _num(k[a]) + _num(v[a]) + _num(f[a])
    out = host(["system", n] + [int(i) for i in ids] + rows + _num(lengths) + _num(MU) + _num(LO) + _num([VSCALE])).splitlines()
    n_mol = int(out[0].split()[1])
    cen = np.array([[float(t) for t in l.split()] for l in out[1:1 + n_mol]]).reshape(n_mol, 10)
    sums = np.array([float(t) for t in out[2 + n_mol].split()])
    ent = np.array([[float(t) for t in l.split()] for l in out[4 + n_mol:]])
    return cen, sums, ent[:, 0].astype(int), ent[:, 1:4], ent[:, 4:7]


def _against_reference(host, ids, mass, r, k, v, f, lengths, what):
    x = r + k * lengths
    cen, sums, atoms, shift, dv = _system(host, ids, mass, r, k, v, f, lengths)
    Y, V, M, d, u, mol = gr.centres(x, v, ids, mass)
    many = np.flatnonzero(np.bincount(mol)[mol] > 1)
    assert sorted(atoms) == list(many)
    # one molecule of the table per multi-atom molecule of the reference: matched through an atom
    _, start = np.unique(np.cumsum(np.r_[0, np.diff(mol[atoms]) != 0]), return_index=True)
    assert len(start) == len(cen)
    which = mol[atoms[start]]
    scale_x, scale_v = np.abs(x).max(), np.abs(v).max()
    assert np.array_equal(cen[:, 0], M[which])
    assert np.abs(cen[:, 1:4] + cen[:, 4:7] - Y[which]).max() <= REL * scale_x and np.abs(cen[:, 7:10] - V[which]).max() <= REL * scale_v
    cw, ck = gr.corrections(x, v, f, ids, mass)
    want = np.concatenate([cw, ck])
    print("%s: centres off by %.3e, sums by %.3e of %.3e" % (what, np.abs(cen[:, 1:4] + cen[:, 4:7] - Y[which]).max(), np.abs(sums - want).max(),
                                                             np.abs(want).max()))
    assert np.abs(sums - want).max() <= REL * np.abs(want).max()
    xs, vs, _ = gr.scale(x, v, LO, lengths, MU, ids, mass, VSCALE)
    # the record's shift: r' = r + shift must be the reference's new unwrapped position minus k (mu L)
    got = r[atoms] + shift + k[atoms] * (MU * lengths)
    assert np.abs(got - xs[atoms]).max() <= REL * scale_x
    assert np.abs(v[atoms] + dv - vs[atoms]).max() <= REL * scale_v
    return shift


def _quantised(a):
    """multiples of 2^-20: r + k L (L a multiple of 2^-20 as well) and every difference of two such numbers below 2^32 is exact"""
    return np.round(np.asarray(a) * 2.0 ** 20) / 2.0 ** 20


def test_centres_sums_and_shifts_match_the_reference_on_the_molecule_box(host):
    B = gr.molecule_box()
    lengths = hr.LENGTHS
    k = np.floor((B["pos"] - LO) / lengths)
    r = B["pos"] - k * lengths                                               # (the engine's wrapped record and its image counts)
    rng = np.random.default_rng(11)
    f = rng.normal(size=r.shape) * 30.0
    assert np.abs(k).max() >= 3                                              # (molecules several box lengths out)
    _against_reference(host, B["ids"], B["mass"], r, k, B["vel"], f, lengths, "molecule box")


def test_atoms_five_hundred_box_lengths_out(host):
    """One molecule of 70 atoms and three small ones, 500 box lengths out on two axes, with members in different images.  The
    coordinates and lengths are multiples of 2^-20, so that the yardstick's unwrapped positions are exact and 1e-13 is a bound on the
    code alone."""
    rng = np.random.default_rng(12)
    lengths = _quantised([9.0, 9.6, 10.5])
    n = 80
    ids = np.array([3] * 70 + [8, 8, 8] + [1, 1] + [-1] * 5)
    base = _quantised(rng.uniform(0.0, 1.0, size=(n, 3)) * 6.0)
    k = np.tile([500.0, -500.0, 0.0], (n, 1)) + rng.integers(-1, 2, size=(n, 3))
    x = LO + base + k * lengths
    kk = np.floor((x - LO) / lengths)
    r = x - kk * lengths
    assert np.array_equal(r + kk * lengths, x) and np.abs(kk).max() >= 500
    mass = rng.uniform(1.0, 16.0, size=n)
    mass[5] = 0.0                                                            # a massless member (a virtual site) adds nothing
    v, f = rng.normal(size=(n, 3)), rng.normal(size=(n, 3)) * 30.0
    shift = _against_reference(host, ids, mass, r, kk, v, f, lengths, "500 box lengths out")
    # a factor of exactly 1 along an axis would leave the record its bits: the shift is (mu - 1) times a finite number
    assert np.isfinite(shift).all()


def test_on_a_triangle_the_functions_are_settle_hpps_own(host):
    rng = np.random.default_rng(13)
    for _ in range(20):
        y = rng.normal(size=(3, 3)) * 0.3 + rng.uniform(-8.0, 8.0, 3)
        v, f = rng.normal(size=(3, 3)), rng.normal(size=(3, 3)) * 40.0
        m_apex, m_leg = rng.uniform(8.0, 20.0), rng.uniform(0.5, 3.0)
        out = host(["triangle"] + _num(y) + _num(v) + _num(f) + _num([m_apex, m_leg]) + _num(MU) + _num(LO) + _num([VSCALE])).splitlines()
        a, b = (np.array([float(t) for t in l.split()]) for l in out)
        assert np.abs(a[:6] - b[:6]).max() <= REL * np.abs(a[:6]).max() and np.abs(a[6:12] - b[6:12]).max() <= REL * np.abs(a[6:12]).max()
        assert np.abs(a[12:15] - b[12:15]).max() <= REL * np.abs(y).max() and np.abs(a[15:] - b[15:]).max() <= REL * np.abs(v).max()
