"""CPU test of the host builders of the topology tables (emdee.jl_amd/csrc/topology.hpp) through the stand-alone program
tests/c/topology_host.cpp, built with the host compiler under ASan and UBSan.  The expected tables are restated here from the
documented layout with sets and sorted lists; nothing is recorded output of the builders.

Layout.  A pair table is a CSR over ids 0 .. rows - 1 (rows = max id + 1): start[rows + 1], and behind it each id's partners,
ascending and without duplicates, every pair listed from both sides.  The struck rows hold the exclusions and the 1-4 pairs
together, the 1-4 rows the 1-4 pairs alone.  The bonded tables give every atom the row of its partners (the other atoms of its
terms, ascending, unique) and a row of term entries in (kind, term, role) order: code = kind | role << 2, loc[c] = where the c-th
other atom of the term (in term order) sits in the owner's partner row, tid = the term's number over all kinds in kind order,
and three parameters per entry, zero padded, in fp64 and rounded to fp32."""
import math
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT

ERR_INVALID = -1
KIND_ATOMS = {1: 2, 2: 3, 3: 4}
KIND_PARAMS = {1: 2, 2: 2, 3: 3}
NAMES = {1: "bond", 2: "angle", 3: "torsion"}


@pytest.fixture(scope="session")
def topology_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("topology_host") / "topology_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "topology_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _fields(out):
    """"name v v v" lines -> {name: [tokens]} ('lost' and 'term_of' lines collect into lists)."""
    got = {"lost": [], "term_of": []}
    for ln in out.splitlines():
        name, _, rest = ln.partition(" ")
        if name == "lost":
            got["lost"].append(rest)
        elif name == "term_of":
            got["term_of"].append([int(t) for t in rest.split()])
        else:
            got[name] = rest.split()
    return got


def _ints(got, name):
    return [int(t) for t in got[name]]


def _refusal(out):
    word, code, message = out.rstrip("\n").split(" ", 2)
    assert word == "REFUSED", out
    return int(code), message


def _flat(pairs):
    return [len(pairs)] + [g for p in pairs for g in p]


def _csr(pairs, rows):
    """Symmetric rows as sets -> (start, idx)."""
    sets = [set() for _ in range(rows)]
    for i, j in pairs:
        sets[i].add(j)
        sets[j].add(i)
    start, idx = [0], []
    for s in sets:
        idx += sorted(s)
        start.append(len(idx))
    return start, idx


def _pair_case(run, excl, p14, lim=8):
    got = _fields(run(["pairs", lim] + _flat(excl) + _flat(p14)))
    rows = max([g + 1 for p in excl + p14 for g in p], default=0)
    assert _ints(got, "rows") == [rows]
    xs, xi = _csr(excl + p14, rows)
    ps, pi = _csr(p14, rows)
    assert (_ints(got, "xs"), _ints(got, "xi")) == (xs, xi)
    assert (_ints(got, "ps"), _ints(got, "pi")) == (ps, pi)
    assert _ints(got, "n14") == [len(pi)]
    assert (_ints(got, "has_excl"), _ints(got, "has_14")) == ([int(bool(xi))], [int(bool(pi))])
    return got


def test_pair_tables_are_symmetric_sorted_and_duplicate_free(topology_host):
    p14 = [(0, 3), (5, 2)]
    got = _pair_case(topology_host, [(0, 1), (1, 0), (0, 1), (2, 5), (7, 3)], p14)
    assert _ints(got, "rows") == [8] and _ints(got, "n14") == [4]
    # spelled out once: the symmetric union without duplicates, and the 1-4 pairs alone
    assert _ints(got, "xs") == [0, 2, 3, 4, 6, 6, 7, 7, 8] and _ints(got, "xi") == [1, 3, 0, 5, 0, 7, 2, 3]
    assert _ints(got, "ps") == [0, 1, 1, 2, 3, 3, 4, 4, 4] and _ints(got, "pi") == [3, 5, 0, 2]
    # 1-4 pairs without exclusions: they are all that is struck
    got = _pair_case(topology_host, [], p14)
    assert (got["xs"], got["xi"]) == (got["ps"], got["pi"]) and _ints(got, "rows") == [6]
    # nothing at all: no rows, a single start entry
    got = _pair_case(topology_host, [], [])
    assert _ints(got, "rows") == [0] and _ints(got, "xs") == [0] and _ints(got, "ps") == [0]
    assert _ints(got, "has_excl") == [0] and _ints(got, "has_14") == [0] and got["xi"] == [] and got["pi"] == []


# bonds: a 3-ring and a tail; two torsions over the same four atoms; atom 5 in no term (lim = 6)
TERMS = {1: ([(0, 1), (1, 2), (2, 0), (2, 3)], [(100.1, 1.1), (200.2, 1.2), (300.3, 0.0), (400.4, 1.4)]),
         2: ([(0, 1, 2), (1, 2, 3)], [(50.5, 0.0), (60.6, math.pi)]),
         3: ([(0, 1, 2, 3), (3, 2, 1, 0), (1, 2, 3, 4)], [(1.1, 1.0, 0.3), (2.2, 3.0, -0.7), (3.3, 2.0, 3.1)])}


def _bonded_case(terms, lim=6, lost=()):
    case = ["bonded", lim]
    for kind in (1, 2, 3):
        ids, prm = terms.get(kind, ([], []))
        case += [len(ids)] + [g for t in ids for g in t] + [repr(float(q)) for p in prm for q in p]
    return case + list(lost)


def test_bonded_tables_on_a_ring_and_on_terms_that_share_atoms(topology_host):
    got = _fields(topology_host(_bonded_case(TERMS)))
    rows = 5                                                 # ids 0 .. 4 are named; atom 5 has no row at all
    partners = [set() for _ in range(rows)]
    for kind, (ids, _) in TERMS.items():
        for t in ids:
            for g in t:
                partners[g] |= set(t) - {g}
    prow = [sorted(s) for s in partners]
    ps = [0] + list(np.cumsum([len(r) for r in prow]))
    assert _ints(got, "rows") == [rows] and _ints(got, "nb") == [ps[-1]]
    assert _ints(got, "ps") == ps and _ints(got, "pi") == [g for r in prow for g in r]
    assert prow[2] == [0, 1, 3, 4] and prow[0] == [1, 2, 3]  # (the ring closes: 0 and 2 are partners through bond (2, 0))
    # entries per owner in (kind, term, role) order
    entries = [[] for _ in range(rows)]
    number = 0
    for kind in (1, 2, 3):
        for t, p in zip(*TERMS[kind]):
            for role, g in enumerate(t):
                loc = [prow[g].index(o) for a, o in enumerate(t) if a != role]
                entries[g].append((kind | role << 2, loc + [0] * (3 - len(loc)), number, list(p) + [0.0] * (3 - len(p))))
            number += 1
    flat = [e for row in entries for e in row]
    assert _ints(got, "ts") == [0] + list(np.cumsum([len(r) for r in entries]))
    assert _ints(got, "terms") == [v for code, loc, _, _ in flat for v in [code] + loc]
    assert _ints(got, "tid") == [n for _, _, n, _ in flat]
    pd = np.array([q for _, _, _, p in flat for q in p])
    assert [float(t) for t in got["pd"]] == list(pd)                              # (%.17g round-trips a double)
    assert [np.float32(t) for t in got["pf"]] == list(pd.astype(np.float32))      # (%.9g round-trips a float)
    assert len(flat) == 2 * 4 + 3 * 2 + 4 * 3
    # bonded_term_of inverts the numbering
    want = [[n, kind, k] for n, (kind, k) in enumerate((kind, k) for kind in (1, 2, 3) for k in range(len(TERMS[kind][0])))]
    assert got["term_of"] == want and len(want) == number


def test_an_atom_beyond_the_last_named_id_and_empty_tables(topology_host):
    got = _fields(topology_host(_bonded_case({1: ([(1, 3)], [(1.0, 1.0)])})))
    assert _ints(got, "rows") == [4] and _ints(got, "ps") == [0, 0, 1, 1, 2] and _ints(got, "pi") == [3, 1]   # rows 0 and 2 are empty
    assert _ints(got, "ts") == [0, 0, 1, 1, 2] and _ints(got, "terms") == [1, 0, 0, 0, 1 | 1 << 2, 0, 0, 0]
    got = _fields(topology_host(_bonded_case({})))
    assert _ints(got, "rows") == [0] and _ints(got, "ps") == [0] and _ints(got, "ts") == [0] and got["terms"] == [] and got["pd"] == []


PAIR_TEXT = "%s: pair %d = (%d, %d) is not a pair of two different ids in [0, 8)"
BOND2 = ([(0, 1), (1, 2)], [(1.0, 1.0), (1.0, 1.0)])
REFUSALS = [
    (["pairs", 8] + _flat([(0, 1), (3, 3)]) + _flat([]), PAIR_TEXT % ("set_exclusions", 1, 3, 3)),
    (["pairs", 8] + _flat([]) + _flat([(1, 8)]), PAIR_TEXT % ("set_pairs14", 0, 1, 8)),
    (["pairs", 8] + _flat([(-1, 2)]) + _flat([]), PAIR_TEXT % ("set_exclusions", 0, -1, 2)),
    (_bonded_case({1: ([(0, 1), (2, 2)], BOND2[1])}), "set_bonded: bond 1 names atom 2 twice"),
    (_bonded_case({1: BOND2, 2: ([(0, 1, 6)], [(1.0, 1.0)])}), "set_bonded: angle 0 names id 6, outside [0, 6)"),
    (_bonded_case({1: (BOND2[0], [(1.0, 1.0), (1.0, -1.0)])}), "set_bonded: bond 1 has r0 < 0"),
    (_bonded_case({2: ([(0, 1, 2)], [(1.0, 4.0)])}), "set_bonded: angle 0 has theta0 outside [0, pi]"),
    (_bonded_case({3: ([(0, 1, 2, 3)], [(1.0, 1.5, 0.0)])}), "set_bonded: torsion 0 has a periodicity that is not an integer >= 1"),
    (_bonded_case({3: ([(0, 1, 2, 3)], [(1.0, 0.0, 0.0)])}), "set_bonded: torsion 0 has a periodicity that is not an integer >= 1"),
    (_bonded_case({1: (BOND2[0], [(1.0, 1.0), (float("nan"), 1.0)])}), "set_bonded: bond 1 has a non-finite parameter"),
    (["charges", 3, 3, 1.0, "inf", 1.0, 0.5, "nan", 0.25], "set_coulomb: charge 1 is not finite"),
    (["charges", 3, 3, 0.0, "inf", 1.0, 0.5, 0.5, 0.25], "set_coulomb: the Coulomb constant must be finite and > 0"),
    (["charges", 3, 3, 1.0, 0.5, 1.0, 0.5, 0.5, 0.25], "set_coulomb: the reaction-field dielectric must be >= 1 (+inf allowed)"),
]


@pytest.mark.parametrize("case,message", REFUSALS, ids=[m.split(" (")[0][:60] for _, m in REFUSALS])
def test_invalid_tables_are_refused_with_the_message_of_the_set_calls(topology_host, case, message):
    assert _refusal(topology_host(case)) == (ERR_INVALID, message)


def test_charges_are_scaled_by_the_root_of_the_coulomb_constant(topology_host):
    q = [0.5, -0.25, 0.1]
    got = _fields(topology_host(["charges", 3, -1, 2.0, 78.5, 0.5] + [repr(x) for x in q]))
    assert [float(t) for t in got["q"]] == [x * math.sqrt(2.0) for x in q]


def test_the_lost_partner_message_names_the_term_and_its_atoms(topology_host):
    tail = ": a partner is farther than rc + skin from its owner at a neighbour-list build, so the term cannot be evaluated; " \
           "replace the tables or the state"
    got = _fields(topology_host(_bonded_case(TERMS, lost=[2, 5, 7])))
    assert got["lost"] == ["bonded bond 2 (atoms 2 0)" + tail, "bonded angle 1 (atoms 1 2 3)" + tail,
                           "bonded torsion 1 (atoms 3 2 1 0)" + tail]
