"""CPU tests of the parts of the displacement and velocity correlations with no HIP in them (include/emdee_hip.h: emdee_md_set_msd):
the table order and its chunks, the schedule of origins, an atom's addends and a group's words of emdee.jl_amd/csrc/msd.hpp through
the stand-alone program tests/c/msd_host.cpp, built with the host compiler under ASan and UBSan, against numpy and a brute-force
enumeration written here; and the kernels' resource usage from `make report`."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import ROOT


@pytest.fixture(scope="session")
def msd_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msd_host") / "msd_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "msd_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _rows(text, kind=int):
    return [[kind(t) for t in line.split()] for line in text.splitlines()]


@pytest.fixture(scope="session")
def chunk(msd_host):
    c, words = _rows(msd_host(["chunk"]))[0]
    assert words == 7
    return c


# ---------------------------------------------------------------- the table order and its chunks
def _layout(msd_host, groups, n_groups, n=None):
    if groups is None:
        rows = _rows(msd_host(["layout", n_groups, n, 0]))
    else:
        rows = _rows(msd_host(["layout", n_groups, len(groups), 1] + [int(g) for g in groups]))
    (n_grouped, n_chunks), sizes, cog, pos_of = rows[0], rows[1], rows[2], rows[3]
    chunks = rows[4:]
    assert len(chunks) == n_chunks
    return n_grouped, sizes, cog, np.array(pos_of, dtype=np.int64), chunks


def _check_layout(groups, n_groups, n_grouped, sizes, cog, pos_of, chunks, chunk):
    groups = np.asarray(groups)
    want_sizes = [int((groups == g).sum()) for g in range(n_groups)] + [0] * (8 - n_groups)
    assert sizes == want_sizes and n_grouped == sum(want_sizes)
    # a bijection from the grouped ids onto 0 ... n_grouped - 1; the others are absent
    assert (pos_of[groups < 0] == -1).all()
    assert sorted(pos_of[groups >= 0].tolist()) == list(range(n_grouped))
    # group-major, ascending id inside a group: the entries in order are the ids sorted by (group, id)
    ids = np.nonzero(groups >= 0)[0]
    order = ids[np.lexsort((ids, groups[ids]))]
    assert np.array_equal(pos_of[order], np.arange(n_grouped))
    # chunks tile every group exactly, in order; none mixes groups or exceeds the chunk; chunk_of_group brackets each group's
    first = np.concatenate([[0], np.cumsum(want_sizes)])
    at = 0
    for g in range(n_groups):
        mine = chunks[cog[g]:cog[g + 1]]
        assert all(c[2] == g for c in mine)
        assert len(mine) == -(-want_sizes[g] // chunk)
        e = int(first[g])
        for f, count, _ in mine:
            assert f == e and 1 <= count <= chunk
            e += count
        assert e == first[g + 1]
        assert all(c[1] == chunk for c in mine[:-1])         # only the last chunk of a group is part-filled
        at += len(mine)
    assert at == len(chunks) and all(c == len(chunks) for c in cog[n_groups:])


def test_layout_at_the_chunk_edges(msd_host, chunk):
    sizes = [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
    rng = np.random.default_rng(5)
    groups = np.concatenate([np.full(s, g) for g, s in enumerate(sizes)] + [np.full(300, -1)])
    rng.shuffle(groups)
    out = _layout(msd_host, groups, len(sizes))
    _check_layout(groups, len(sizes), *out, chunk)
    assert out[0] == sum(sizes) and len(out[4]) == 0 + 1 + 1 + 1 + 2 + 4


def test_layout_with_all_atoms_ungrouped_but_one(msd_host, chunk):
    groups = np.full(2 * chunk + 3, -1)
    groups[chunk + 1] = 2
    out = _layout(msd_host, groups, 3)
    _check_layout(groups, 3, *out, chunk)
    assert out[0] == 1 and out[4] == [[0, 1, 2]] and out[3][chunk + 1] == 0


def test_layout_with_eight_groups_interleaved_by_id(msd_host, chunk):
    groups = np.arange(8 * chunk + 24) % 8
    out = _layout(msd_host, groups, 8)
    _check_layout(groups, 8, *out, chunk)
    assert out[1] == [chunk + 3] * 8 and len(out[4]) == 16


def test_layout_without_a_group_array_is_the_identity(msd_host, chunk):
    n = chunk + 7
    n_grouped, sizes, cog, pos_of, chunks = _layout(msd_host, None, 1, n)
    assert n_grouped == n and sizes[0] == n and np.array_equal(pos_of, np.arange(n))
    assert chunks == [[0, chunk, 0], [chunk, 7, 0]] and cog[:2] == [0, 2]
    assert _layout(msd_host, None, 1, 0)[0] == 0             # no atoms: no entries, no chunks


# ---------------------------------------------------------------- the schedule
@pytest.mark.parametrize("n_lags,every", [(1, 1), (6, 2), (7, 3), (64, 1), (4096, 64)])
def test_schedule_is_the_brute_force_enumeration(msd_host, n_lags, every):
    s_end = 3 * n_lags
    rows = _rows(msd_host(["schedule", n_lags, every, s_end]))
    assert len(rows) == s_end + 1
    n_origins = -(-n_lags // every)
    held = {}                                                # ring slot -> the sample it holds
    seen = set()
    for s, row in enumerate(rows):
        is_origin, slot, n_live = row[:3]
        live = list(zip(row[3::2], row[4::2]))
        assert len(live) == n_live <= n_origins
        assert is_origin == (1 if s % every == 0 else 0)
        if is_origin:
            assert slot == (s // every) % n_origins
            # the slot is free: what it held is out of reach of this and every later sample
            assert slot not in held or s - held[slot] >= n_lags
            held[slot] = s
        else:
            assert slot == -1
        want = [(so, s - so) for so in range(0, s + 1, every) if s - so < n_lags]
        got = []
        for sl, lag in live:
            so = s - lag
            assert 0 <= lag < n_lags and so >= 0 and so % every == 0
            assert sl == (so // every) % n_origins and held.get(sl) == so      # the slot still holds that origin
            got.append((so, lag))
        assert sorted(got) == sorted(want) and len(set(got)) == len(got)
        assert (0 in [lag for _, lag in live]) == bool(is_origin)              # lag 0 exactly at origin samples
        seen.update((so, s) for so, _ in got)
    # every pair (s_o, s) within reach appears exactly once over the run
    assert seen == {(so, s) for s in range(s_end + 1) for so in range(0, s + 1, every) if s - so < n_lags}


# ---------------------------------------------------------------- the addends and the words
def test_term_and_finish_are_the_numpy_formulas(msd_host):
    rng = np.random.default_rng(17)
    n = 200
    c, o = rng.normal(0.0, 30.0, (n, 6)), rng.normal(0.0, 30.0, (n, 6))
    got = np.array(_rows(msd_host(["term", n] + [repr(float(t)) for t in np.concatenate([c, o], axis=1).ravel()]), float))
    d = c[:, :3] - o[:, :3]
    assert np.array_equal(got[:, 0:3], d * d) and np.array_equal(got[:, 3:6], d)
    vv = c[:, 3:] * o[:, 3:]
    # (the dot product may be contracted: three products of at most 2^-53 relative error each, two sums)
    assert (np.abs(got[:, 6] - vv.sum(axis=1)) <= 4 * 2.0 ** -53 * np.abs(vv).sum(axis=1)).all()
    tot = rng.normal(0.0, 1e3, (n, 7))
    got = np.array(_rows(msd_host(["finish", n] + [repr(float(t)) for t in tot.ravel()]), float))
    want = tot.copy()
    want[:, 3:6] = tot[:, 3:6] ** 2
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- the kernels
def test_msd_kernels_are_in_the_report_and_use_no_scratch_memory():
    """`make report` (hipcc -Rpass-analysis=kernel-resource-usage on both kernel translation units, cross-compiled: no GPU needed):
    the three kernels of a sample are there, the gather in both precisions, the accumulate in its three masks, and keep nothing in
    scratch"""
    src = os.path.join(ROOT, "emdee.jl_amd", "csrc")
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-s", "-C", src, "report"], timeout=1500)
    seen = {}
    for name in ("resource_usage_f64.txt", "resource_usage_f32.txt"):
        text = open(os.path.join(src, name)).read()
        for b in re.split(r"remark: Function Name: ", text)[1:]:
            fn = b.split(" ", 1)[0].strip()
            if "k_msd" not in fn:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
            assert m is not None, fn
            assert int(m.group(1)) == 0, "%s keeps %s bytes per lane in scratch memory" % (fn, m.group(1))
            seen.setdefault(name, set()).add(fn)
    for name, real in (("resource_usage_f64.txt", "Id"), ("resource_usage_f32.txt", "If")):
        fns = seen.get(name, set())
        assert any("k_msd_gather" + real in f for f in fns), (name, sorted(fns))
        assert sum("k_msd_accumulate" in f for f in fns) == 3, (name, sorted(fns))
        assert any("k_msd_finish" in f for f in fns), (name, sorted(fns))
