"""CPU tests of the parts of the radial distribution functions with no HIP in them (include/emdee_hip.h: emdee_md_set_rdf): the slot
map, the bin rule, the planner of the sample's grid and stencil and the normalisation of emdee.jl_amd/csrc/rdf.hpp through the
stand-alone program tests/c/rdf_host.cpp, built with the host compiler under ASan and UBSan, against tests/helpers/rdf_ref.py; and
the kernels' resource usage from `make report`."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import barostat_ref as bref
from .helpers import rdf_ref as rr


@pytest.fixture(scope="session")
def rdf_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rdf_host") / "rdf_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "rdf_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _rows(text, kind=int):
    return [[kind(t) for t in line.split()] for line in text.splitlines()]


# ---------------------------------------------------------------- slots and bins
@pytest.mark.parametrize("n_groups", range(1, 9))
def test_slot_map_is_a_bijection_onto_the_pairs(rdf_host, n_groups):
    table = _rows(rdf_host(["slots", n_groups]))
    upper = [table[a][b] for a in range(n_groups) for b in range(a, n_groups)]
    assert upper == list(range(rr.n_pairs(n_groups)))                      # row by row of the upper triangle, nothing left out
    for a, b in itertools.product(range(n_groups), repeat=2):
        assert table[a][b] == table[b][a] == rr.pair_slot(a, b, n_groups)


@pytest.mark.parametrize("r_max,n_bins", [(5.13, 100), (1.0, 7), (2.5, 8192), (0.3, 1)])
def test_bin_rule_is_numpys_at_edges_at_zero_and_below_r_max(rdf_host, r_max, n_bins):
    inv_dr = n_bins / r_max
    edges = r_max * np.arange(n_bins + 1) / n_bins
    pick = np.unique(np.concatenate([np.arange(min(n_bins + 1, 40)), np.arange(max(n_bins - 40, 0), n_bins + 1)]))
    r = np.concatenate([edges[pick], np.nextafter(edges[pick], 0.0), np.nextafter(edges[pick], np.inf),
                        [0.0, np.nextafter(r_max, 0.0), r_max, 1.5 * r_max], np.random.default_rng(3).uniform(0.0, 1.2 * r_max, 200)])
    r2 = r * r
    got = np.array(_rows(rdf_host(["bins", repr(r_max), n_bins, len(r2)] + [repr(float(t)) for t in r2])))[:, 0]
    want = (np.sqrt(r2) * inv_dr).astype(np.int64)
    want[want >= n_bins] = -1
    assert np.array_equal(got, want)
    assert got[len(r) - 204] == 0 and got[len(r) - 201] == -1             # r = 0 lands in bin 0, 1.5 r_max nowhere
    assert (got == n_bins - 1).any() and (got == -1).any()


# ---------------------------------------------------------------- the planner
BOXES = [(2.0, 2.0, 2.0), (2.0, 2.1, 2.2), (2.0, 3.0, 5.0), (4.0, 4.9, 5.1), (6.99, 7.0, 7.01), (3.0, 11.0, 40.0), (40.0, 2.0, 9.5),
         (12.3, 7.7, 5.05)]
ATOMS = [37, 864, 200000]


def _plan(rdf_host, sides, r_max, n):
    M = _rows(rdf_host(["plan"] + [repr(s * r_max) for s in sides] + [repr(r_max), n]))[0]
    return M[:3], M[3], M[4:]


@pytest.mark.parametrize("n", ATOMS)
@pytest.mark.parametrize("sides", BOXES)
def test_planner_cells_are_wide_enough_and_every_cell_in_reach_is_visited_once(rdf_host, sides, n):
    r_max = 1.37
    M, nd, wrap = _plan(rdf_host, sides, r_max, n)
    L = [s * r_max for s in sides]
    assert 1 <= nd <= 3 and all(m >= 1 for m in M)
    assert all(L[d] / M[d] >= r_max / nd for d in range(3))
    assert wrap == [1 if M[d] < 2 * nd + 1 else 0 for d in range(3)]
    visits = _rows(rdf_host(["visits"] + [repr(t) for t in L] + [repr(r_max), n]))
    ncell = M[0] * M[1] * M[2]
    assert len(visits) == ncell
    # within reach along an axis: the nearest faces of the two cells are closer than r_max in some periodic image
    reach = []
    for d in range(3):
        w = L[d] / M[d]
        k = np.arange(M[d])
        gap = np.abs(k[:, None] - k[None, :])
        gap = np.minimum(gap, M[d] - gap)
        reach.append((np.maximum(gap - 1, 0) * w) < r_max)
    for c, seen in enumerate(visits):
        assert len(seen) == len(set(seen)), "cell %d visits a cell twice" % c
        cx, cy, cz = c % M[0], (c // M[0]) % M[1], c // (M[0] * M[1])
        need = {x + M[0] * (y + M[1] * z) for z in np.nonzero(reach[2][cz])[0] for y in np.nonzero(reach[1][cy])[0]
                for x in np.nonzero(reach[0][cx])[0]}
        assert need <= set(seen), "cell %d misses %s" % (c, sorted(need - set(seen))[:5])
    # the relation is symmetric, which is what lets a pair be counted from the atom of the lower cell alone
    sets = [set(s) for s in visits]
    assert all(c in sets[c2] for c, s in enumerate(sets) for c2 in s)


def test_planner_takes_finer_cells_only_where_they_stay_populated(rdf_host):
    r_max = 2.5
    assert _plan(rdf_host, (8.0, 8.0, 8.0), r_max, 100)[1] == 1            # 0.2 atoms per cell of side r_max: no finer
    assert _plan(rdf_host, (8.0, 8.0, 8.0), r_max, 6400)[1] == 1           # 12.5 per cell of side r_max, 1.6 at half the side
    assert _plan(rdf_host, (8.0, 8.0, 8.0), r_max * 2, 51200)[1] == 2      # 100 per cell of side r_max: nd = 2 leaves 12.5
    M, nd, wrap = _plan(rdf_host, (40.0, 40.0, 40.0), r_max, 30)           # a sparse box: about four cells per atom at the most
    assert M[0] * M[1] * M[2] <= 4 * 30 + 64 and nd == 1


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_row_runs_are_the_cells_of_the_axis(rdf_host, nd):
    """the pair kernel walks x by runs of cells, not by rdf_axis_cell: for every axis length and home coordinate the runs hold
    exactly the cells rdf_axis_cell names, each once, as ascending in-range runs; an axis that does not wrap has one run of
    2 nd + 1 cells in its interior and two runs at either face"""
    for M in range(1, 4 * nd + 4):
        wrap = 1 if M < 2 * nd + 1 else 0
        rows = _rows(rdf_host(["runs", M, nd, wrap]))
        assert len(rows) == M
        for cx, row in enumerate(rows):
            nseg, xa0, xa1, xb0, xb1 = row[:5]
            cells = row[5:]
            runs = list(range(xa0, xa1 + 1)) + (list(range(xb0, xb1 + 1)) if nseg == 2 else [])
            assert 0 <= xa0 <= xa1 < M and (nseg == 1 or xa1 < xb0 <= xb1 < M), (M, cx, row)
            assert sorted(runs) == sorted(cells) and len(set(runs)) == len(runs), (M, cx, row)
            if wrap:
                assert nseg == 1 and runs == list(range(M))
            else:
                assert len(runs) == 2 * nd + 1
                assert nseg == (2 if (cx < nd or cx + nd >= M) else 1), (M, cx, row)
                if nseg == 1:
                    assert (xa0, xa1) == (cx - nd, cx + nd)
                elif cx < nd:
                    assert (xa0, xa1, xb0, xb1) == (0, cx + nd, cx - nd + M, M - 1)
                else:
                    assert (xa0, xa1, xb0, xb1) == (0, cx + nd - M, cx - nd, M - 1)


def test_planner_leaves_x_unwrapped_on_the_two_boxes_kept_for_that(rdf_host, emdee_synthetic):
    L = bref.fluid864(emdee_synthetic)["L"]
    assert _plan(rdf_host, (L / rr.NOWRAP_FLUID_R_MAX,) * 3, rr.NOWRAP_FLUID_R_MAX, 864) == ([6, 6, 6], 1, [0, 0, 0])
    sides = tuple(s / rr.NOWRAP_R_MAX for s in rr.NOWRAP_LENGTHS)
    assert _plan(rdf_host, sides, rr.NOWRAP_R_MAX, rr.NOWRAP_N) == ([5, 4, 4], 2, [0, 1, 1])


def test_host_pair_loop_reproduces_the_brute_force_where_x_does_not_wrap(rdf_host, emdee_synthetic):
    """the loop walks x by rdf_row_runs, as the kernel does: interior runs and both kinds of face runs, at nd = 1 and nd = 2"""
    S = bref.fluid864(emdee_synthetic)
    n = 864
    for pos, L, r_max, n_bins in ((S["pos"], [S["L"]] * 3, rr.NOWRAP_FLUID_R_MAX, 30), (rr.nowrap_box(), rr.NOWRAP_LENGTHS, rr.NOWRAP_R_MAX, 50)):
        want, edge = rr.histogram(pos, L, r_max, n_bins, delta=1e-10 * r_max)
        assert edge.sum() == 0
        got = _host_pairs(rdf_host, pos, L, r_max, n_bins, np.zeros(n, int), -np.ones(n, int), 1)
        assert np.array_equal(got, want) and want.sum() > 3000


# ---------------------------------------------------------------- the pair loop the planner drives
def _host_pairs(rdf_host, pos, L, r_max, n_bins, groups, molecules, n_groups):
    case = ["pairs"] + [repr(float(t)) for t in L] + [repr(r_max), n_bins, n_groups, len(pos)]
    for p, g, m in zip(pos, groups, molecules):
        case += [repr(float(t)) for t in p] + [int(g), int(m)]
    return np.array(_rows(rdf_host(case)), dtype=np.int64)


@pytest.mark.parametrize("sides", [(2.0, 2.0, 2.0), (2.0, 2.1, 2.2), (2.0, 5.3, 7.1)])
def test_host_pair_loop_reproduces_the_brute_force_where_the_stencil_wraps(rdf_host, sides):
    rng = np.random.default_rng(37)
    r_max, n_bins, n = 1.5, 20, 37
    L = np.array(sides) * r_max
    pos = rng.uniform(0.0, 1.0, (n, 3)) * L
    groups = rng.integers(-1, 3, n)
    molecules = np.arange(n) // 3
    want, edge = rr.histogram(pos, L, r_max, n_bins, groups, molecules, 3, delta=1e-10 * r_max)
    assert edge.sum() == 0
    got = _host_pairs(rdf_host, pos, L, r_max, n_bins, groups, molecules, 3)
    # (the widest box holds 666 pairs x (4 pi / 3) / 75 within r_max, 9 / 16 of them grouped: about twenty)
    assert np.array_equal(got, want) and want.sum() > 10
    # one group, no molecules: every pair within r_max, once
    want1, _ = rr.histogram(pos, L, r_max, n_bins)
    got1 = _host_pairs(rdf_host, pos, L, r_max, n_bins, np.zeros(n, int), -np.ones(n, int), 1)
    assert np.array_equal(got1, want1) and want1.sum() > want.sum()


# ---------------------------------------------------------------- normalisation
def test_normalise_is_the_numpy_formula(rdf_host):
    rng = np.random.default_rng(11)
    n_groups, n_bins, r_max, frames, ivs = 3, 25, 1.3, 7, 7 / 33.3
    sizes = [100, 1, 0]
    counts = rng.integers(0, 5000, (rr.n_pairs(n_groups), n_bins))
    out = np.array(_rows(rdf_host(["normalise", n_groups, n_bins, repr(r_max), frames, repr(ivs)] + sizes + list(counts.ravel())), float))
    g, cn = out[:len(counts)], out[len(counts):]
    wg, wc = rr.normalise(counts, n_groups, r_max, sizes, frames, ivs)
    assert np.allclose(g, wg, rtol=1e-13, atol=0.0) and np.allclose(cn, wc, rtol=1e-13, atol=0.0)
    assert (g[rr.pair_slot(0, 0, 3)] > 0).all() and (g[rr.pair_slot(0, 1, 3)] > 0).all()
    assert (g[rr.pair_slot(1, 1, 3)] == 0).all() and (g[rr.pair_slot(2, 2, 3)] == 0).all()      # P = 0: no pairs to speak of
    assert (cn[rr.pair_slot(0, 2, 3)] > 0).all() and (cn[rr.pair_slot(2, 2, 3)] == 0).all()
    # an ideal gas: counts = P shell / V per frame gives g = 1, and the coordination number of the last bin is N_b (4 pi / 3) r_max^3 / V
    V, N = 1000.0, 5000
    edges = r_max * np.arange(n_bins + 1) / n_bins
    ideal = np.rint(1e6 * 0.5 * N * (N - 1) * 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3) / V).astype(np.int64)
    out = np.array(_rows(rdf_host(["normalise", 1, n_bins, repr(r_max), 1000000, repr(1e6 / V), N] + list(ideal)), float))
    assert np.abs(out[0] - 1.0).max() < 1e-6
    assert out[1][-1] == pytest.approx((N - 1) * 4.0 * np.pi / 3.0 * r_max ** 3 / V, rel=1e-6)


# ---------------------------------------------------------------- the kernels
def test_rdf_kernels_are_in_the_report_and_use_no_scratch_memory():
    """`make report` (hipcc -Rpass-analysis=kernel-resource-usage on both kernel translation units, cross-compiled: no GPU needed):
    the three kernels of a sample are there, in both precisions where they depend on the record type, and keep nothing in scratch"""
    src = os.path.join(ROOT, "emdee.jl_amd", "csrc")
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-s", "-C", src, "report"], timeout=1500)
    seen = {}
    for name in ("resource_usage_f64.txt", "resource_usage_f32.txt"):
        text = open(os.path.join(src, name)).read()
        for b in re.split(r"remark: Function Name: ", text)[1:]:
            fn = b.split(" ", 1)[0].strip()
            if "k_rdf" not in fn:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
            assert m is not None, fn
            assert int(m.group(1)) == 0, "%s keeps %s bytes per lane in scratch memory" % (fn, m.group(1))
            seen.setdefault(name, set()).add(fn)
    for name, real in (("resource_usage_f64.txt", "Id"), ("resource_usage_f32.txt", "If")):
        fns = seen.get(name, set())
        assert any("k_rdf_count" + real in f for f in fns), (name, sorted(fns))
        assert any("k_rdf_fill" + real in f for f in fns), (name, sorted(fns))
        assert any("k_rdf_pairs" in f for f in fns), (name, sorted(fns))
