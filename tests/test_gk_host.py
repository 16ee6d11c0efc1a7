"""CPU tests of the parts of the Green-Kubo observables with no HIP in them (include/emdee_hip.h: emdee_md_set_gk): the six stress
words, the ring slot and the lag counts, an atom's three heat addends of emdee.jl_amd/csrc/gk.hpp through the stand-alone program
tests/c/gk_host.cpp, built with the host compiler under ASan and UBSan, against numpy and a brute-force enumeration written here;
and the kernels' resource usage from `make report`."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import gk_ref as gr


@pytest.fixture(scope="session")
def gk_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gk_host") / "gk_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "gk_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _rows(text, kind=int):
    return [[kind(t) for t in line.split()] for line in text.splitlines()]


def test_constants_are_the_headers(gk_host):
    assert _rows(gk_host(["words"]))[0] == [9, 6, 3, 65536]
    text = open(os.path.join(ROOT, "include", "emdee_hip.h")).read()
    for name, value in (("EMDEE_GK_STRESS", 1), ("EMDEE_GK_HEAT", 2), ("EMDEE_GK_WORDS", 9)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), text), name


# ---------------------------------------------------------------- the stress words
def test_stress_words_are_the_numpy_formulas_exactly(gk_host):
    """S = K + W, then sums, differences, a halving and a division by three: no product that a compiler could contract with a sum,
    so the words are bit for bit numpy's, whatever the sizes of the twelve sums"""
    rng = np.random.default_rng(23)
    n = 300
    t = rng.normal(0.0, 1.0, (n, 12)) * 10.0 ** rng.integers(-3, 6, (n, 1))
    t[0] = 0.0
    t[1, :6] = -t[1, 6:]                                     # S = 0 exactly
    got = np.array(_rows(gk_host(["stress", n] + [repr(float(v)) for v in t.ravel()]), float))
    want = np.array([gr.stress_words(row) for row in t])
    assert np.array_equal(got, want)
    assert (got[0] == 0.0).all() and (got[1] == 0.0).all()
    # the five traceless words do not see a pressure added to the diagonal, the sixth is that pressure
    p = t[2].copy()
    p[[6, 7, 8]] += 1024.0
    shifted = np.array(_rows(gk_host(["stress", 1] + [repr(float(v)) for v in p]), float))[0]
    assert np.allclose(shifted[:5], got[2][:5], rtol=0, atol=1e-9 * np.abs(t[2]).max()) and abs(shifted[5] - got[2][5] - 1024.0) < 1e-9


# ---------------------------------------------------------------- the ring and the lags
@pytest.mark.parametrize("n_lags", [1, 5, 64])
def test_ring_slots_and_lag_counts_are_the_brute_force_enumeration(gk_host, n_lags):
    """0 ... 200 samples: for n_lags = 64 the ring wraps three times, for 5 forty times.  A ring slot holds the sample written to
    it last; at sample s the slots read for lags 0 ... live - 1 must still hold s, s - 1, ..., and every pair of samples at most
    n_lags - 1 apart must be visited exactly once"""
    s_end = 200
    rows = _rows(gk_host(["ring", n_lags, s_end]))
    assert len(rows) == s_end + 1
    held, pairs = {}, set()
    for s, row in enumerate(rows):
        slot, live, then = row[0], row[1], row[2:]
        assert slot == s % n_lags and 0 <= slot < n_lags
        assert live == min(s, n_lags - 1) + 1 == len(then)
        held[slot] = s                                       # (the push comes before the correlator)
        for l, sl in enumerate(then):
            assert 0 <= sl < n_lags and held.get(sl) == s - l, (s, l, sl)
            pairs.add((s - l, s))
    assert pairs == {(so, s) for s in range(s_end + 1) for so in range(s + 1) if s - so < n_lags}
    # the counts are a function of the number of samples alone, and they are what the enumeration visited
    for samples in (0, 1, n_lags - 1, n_lags, n_lags + 1, 2 * n_lags + 3, s_end + 1):
        counts = _rows(gk_host(["count", n_lags, samples]))[0]
        want = [sum(1 for (so, s) in pairs if s - so == l and s < samples) for l in range(n_lags)]
        assert counts == want == [max(0, samples - l) for l in range(n_lags)]


# ---------------------------------------------------------------- the heat addends
@pytest.mark.parametrize("real", ["double", "float"])
def test_heat_addends_are_the_numpy_formula(gk_host, real):
    """(k + e) v_a + sum_b W_ab v_b per atom, fp64 arithmetic on records of the engine's precision.  numpy follows the same order
    of operations; what may differ is contraction: each of the seven products behind an addend (three of v^2, one (k + e) v_a, three
    W v) can lose its own rounding to a fused multiply-add, 2^-53 of its size each, and one rounding of the last sum moves with
    them: 8 x 2^-53 of the sum of the absolute terms"""
    rng = np.random.default_rng(29)
    n = 400
    kind = np.float32 if real == "float" else np.float64
    rec = rng.normal(0.0, 1.0, (n, 11)) * 10.0 ** rng.integers(-2, 3, (n, 1))
    rec[:, 0] = np.abs(rec[:, 0]) + 0.1                      # inverse masses
    rec[::7, 0] = 0.0                                        # massless atoms
    rec = rec.astype(kind).astype(np.float64)                # (exactly representable in the engine's records)
    got = np.array(_rows(gk_host(["heat", real, n] + [repr(float(v)) for v in rec.ravel()]), float))
    im, e, w, v = rec[:, 0], rec[:, 1], rec[:, 2:8], rec[:, 8:11]
    a = gr.heat_addends(v, e, w, im)
    want, size = a.sum(axis=2), np.abs(a).sum(axis=2)
    gap = np.abs(got - want)
    print("%s records: largest |addend - numpy| / sum |terms| = %.3e (bound %.3e)" % (real, (gap / size).max(), 8 * 2.0 ** -53))
    assert (gap <= 8 * 2.0 ** -53 * size).all()
    # a massless atom has k exactly 0: its addends are e v + W . v alone
    zero = gr.heat_addends(v[::7], e[::7], w[::7], np.ones(len(v[::7])))
    zero[:, :, 0] = e[::7, None] * v[::7]
    assert (np.abs(got[::7] - zero.sum(axis=2)) <= 8 * 2.0 ** -53 * np.abs(zero).sum(axis=2)).all()
    only_k = rec[:1].copy()
    only_k[0, 0], only_k[0, 1:8] = 0.0, 0.0                  # no mass, no energy, no tensor: exactly nothing
    assert (np.array(_rows(gk_host(["heat", real, 1] + [repr(float(t)) for t in only_k.ravel()]), float)) == 0.0).all()


# ---------------------------------------------------------------- the kernels
def test_gk_kernels_are_in_the_report_and_use_no_scratch_memory():
    """`make report` (hipcc -Rpass-analysis=kernel-resource-usage on both kernel translation units, cross-compiled: no GPU needed):
    the kernels of a sample are there, the heat reduction (reduce.hpp's two stages over HeatSums) in both precisions, and keep
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
            if "k_gk" not in fn and "HeatSums" not in fn and "k_reduce_final" not in fn:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
            assert m is not None, fn
            assert int(m.group(1)) == 0, "%s keeps %s bytes per lane in scratch memory" % (fn, m.group(1))
            seen.setdefault(name, set()).add(fn)
    for name, real in (("resource_usage_f64.txt", "Id"), ("resource_usage_f32.txt", "If")):
        fns = seen.get(name, set())
        assert any("k_reduce_partialsINS_8HeatSums" + real in f for f in fns), (name, sorted(fns))
        assert any("k_reduce_final" in f for f in fns), (name, sorted(fns))
        assert any("k_gk_push" in f for f in fns), (name, sorted(fns))
        assert any("k_gk_correlate" in f for f in fns), (name, sorted(fns))
