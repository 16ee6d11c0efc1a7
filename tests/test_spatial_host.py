"""CPU tests of the parts of the spatial profiles with no HIP in them (include/emdee_hip.h: emdee_md_set_spatial): the bin rules, the
table order and its chunks, an atom's addends, and the run reduction and finish of emdee.jl_amd/csrc/spatial.hpp through the
stand-alone program tests/c/spatial_host.cpp, built with the host compiler under ASan and UBSan, against numpy
(tests/helpers/spatial_ref.py) and a brute-force enumeration written here; the normalisation of verlet.spatial_profiles on a
hand-made record; and the kernels' resource usage from `make report`."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import spatial_ref as sp


@pytest.fixture(scope="session")
def spatial_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spatial_host") / "spatial_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "spatial_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _rows(text, kind=int):
    return [[kind(t) for t in line.split()] for line in text.splitlines()]


def _f(v):
    return [float(t).hex() for t in np.asarray(v, dtype=np.float64).ravel()]


@pytest.fixture(scope="session")
def chunk(spatial_host):
    c, words, max_bins = _rows(spatial_host(["consts"]))[0]
    assert (c, words, max_bins) == (1024, sp.WORDS, 4096)
    return c


# ---------------------------------------------------------------- the bin rules
def _planar(spatial_host, x, geom):
    out = spatial_host(["planar", len(x), float(geom["lo"]).hex(), float(geom["inv_width"]).hex(), geom["n_bins"], int(geom["periodic"])] + _f(x))
    return np.array(_rows(out)).ravel()


@pytest.mark.parametrize("lo,length,n_bins", [(0.0, 9.7, 7), (-3.25, 11.3, 64), (2.5, 7.1, 4096), (0.0, 1.0, 1)])
def test_periodic_planar_bins_are_numpys_two_rounding_formula(spatial_host, lo, length, n_bins):
    rng = np.random.default_rng(11)
    geom = sp.planar(2, n_bins, lo, length)
    edges = lo + length * np.arange(n_bins + 1) / n_bins
    x = np.concatenate([lo + length * rng.random(4000), edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                        lo + length * (rng.random(500) + 500.0), lo + length * (rng.random(500) - 500.0), edges + 500.0 * length,
                        edges - 500.0 * length])
    got = _planar(spatial_host, x, geom)
    want, _ = sp.bins_planar(x, geom)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < n_bins
    inner = lo + length * (np.arange(n_bins) + 0.5) / n_bins     # a coordinate well inside bin k lands in bin k, 500 boxes out too
    assert np.array_equal(_planar(spatial_host, inner, geom), np.arange(n_bins))
    if n_bins < 4096:                                            # (500 boxes out the bin centres of 4096 bins keep 2^-53 * 500 * 4096 of a bin)
        assert np.array_equal(_planar(spatial_host, inner + 500.0 * length, geom), np.arange(n_bins))


@pytest.mark.parametrize("r0,r1,n_bins", [(-2.0, 5.5, 7), (1.25, 9.0, 64), (-4.0, -1.0, 4096)])
def test_open_planar_bins_drop_what_lies_outside_the_range(spatial_host, r0, r1, n_bins):
    rng = np.random.default_rng(12)
    geom = sp.planar(0, n_bins, None, range=(r0, r1))
    edges = r0 + (r1 - r0) * np.arange(n_bins + 1) / n_bins
    x = np.concatenate([r0 + (r1 - r0) * rng.random(4000), edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                        r0 - 10.0 * rng.random(300), r1 + 10.0 * rng.random(300), [np.nan, np.inf, -np.inf, 1e300, -1e300]])
    got = _planar(spatial_host, x, geom)
    want, _ = sp.bins_planar(np.where(np.isfinite(x), x, r0 - 1.0), geom)
    assert np.array_equal(got, want)
    assert (got[x < r0] == -1).all() and (got[x >= r1] == -1).all() and (got[~np.isfinite(x)] == -1).all()
    assert got[4000] == 0 and got[4000 + n_bins] == -1           # r0 itself is inside, r1 itself is not


def _radial(spatial_host, pos, geom):
    out = spatial_host(["radial", len(pos)] + _f(geom["centre"]) + _f(geom["len"]) + [float(geom["r_max"]).hex(), geom["n_bins"]] + _f(pos))
    rows = [line.split() for line in out.splitlines()]
    return np.array([int(r[0]) for r in rows]), np.array([float.fromhex(r[1]) for r in rows]), np.array([[float.fromhex(t) for t in r[2:5]] for r in rows])


@pytest.mark.parametrize("periodic", [(1, 1, 1), (0, 0, 0), (1, 1, 0)])
def test_radial_bins_are_numpys_formula_with_the_centre_and_r_max_themselves(spatial_host, periodic):
    rng = np.random.default_rng(13)
    lengths, centre, r_max, n_bins = [9.0, 10.5, 12.0], [0.4, 9.9, -3.0], 4.25, 17
    geom = sp.radial(n_bins, r_max, centre, lengths, periodic)
    pos = rng.uniform(-15.0, 25.0, (3000, 3))
    radii = r_max * np.arange(n_bins + 1) / n_bins
    on_x = np.array(centre)[None, :] + np.stack([radii, 0 * radii, 0 * radii], axis=1)      # every edge, r_max itself included
    pos = np.concatenate([pos, [centre], on_x, on_x + np.array([lengths[0], 0.0, 0.0]) * periodic[0]])
    got, r, d = _radial(spatial_host, pos, geom)
    want, want_r, want_d, _ = sp.bins_radial(pos, geom)
    assert np.array_equal(got, want) and np.array_equal(r, want_r) and np.array_equal(d, want_d)
    assert got[3000] == 0 and r[3000] == 0.0                     # the centre itself: shell 0, r = 0
    assert got[3001 + n_bins] == -1                              # r_max itself is dropped
    assert (got[r >= r_max] == -1).all() and (got[r < r_max] >= 0).all()


# ---------------------------------------------------------------- the table order and its chunks
def _layout(spatial_host, groups, n_groups, n=None):
    if groups is None:
        rows = _rows(spatial_host(["layout", n_groups, n, 0]))
    else:
        rows = _rows(spatial_host(["layout", n_groups, len(groups), 1] + [int(g) for g in groups]))
    return rows[0], rows[1], rows[2], np.array(rows[3], dtype=np.int64), rows[4:]


def _brute_layout(groups, n_groups, chunk):
    """the table order by enumeration: (entries: caller ids in table order, chunks: (first, count, group))"""
    entries, chunks = [], []
    for g in range(n_groups):
        ids = [i for i, gi in enumerate(groups) if gi == g]
        for at in range(0, len(ids), chunk):
            chunks.append((len(entries) + at, min(chunk, len(ids) - at), g))
        entries += ids
    return entries, chunks


@pytest.mark.parametrize("sizes", [[2049], [1, 1023, 1024, 1025, 2049, 0, 0, 7], [0, 5], [1024, 0, 1]])
def test_layout_is_the_brute_force_enumeration(spatial_host, chunk, sizes):
    rng = np.random.default_rng(5)
    groups = np.concatenate([np.full(s, g) for g, s in enumerate(sizes)] + [np.full(100, -1)]).astype(int)
    rng.shuffle(groups)
    (n_grouped, n_chunks), got_sizes, cog, pos_of, chunks = _layout(spatial_host, groups, len(sizes))
    entries, want_chunks = _brute_layout(groups.tolist(), len(sizes), chunk)
    assert n_grouped == len(entries) and got_sizes[:len(sizes)] == sizes
    assert [tuple(c) for c in chunks] == want_chunks and n_chunks == len(want_chunks)
    assert np.array_equal(pos_of[entries], np.arange(len(entries))) and (pos_of[groups < 0] == -1).all()
    for g in range(len(sizes)):
        assert [c[2] for c in chunks[cog[g]:cog[g + 1]]] == [g] * (-(-sizes[g] // chunk))
    if len(sizes) == 1:                                          # one group without a group array: the identity
        none = _layout(spatial_host, None, 1, sizes[0])
        assert np.array_equal(none[3], np.arange(sizes[0])) and len(none[4]) == -(-sizes[0] // chunk)


def test_compact_words_of_every_mask(spatial_host):
    blocks = {1: [0, 1], 2: [2, 3, 4, 5, 6], 4: [7, 8, 9]}
    for mask in range(1, 8):
        assert _rows(spatial_host(["words", mask]))[0] == [w for bit in (1, 2, 4) if mask & bit for w in blocks[bit]]


# ---------------------------------------------------------------- the addends
@pytest.mark.parametrize("what", [1, 2, 4, 7])
def test_addends_are_the_numpy_formulas_and_masked_words_stay_zero(spatial_host, what):
    rng = np.random.default_rng(19)
    n = 120
    m, q, v, e, w = rng.uniform(0.5, 3.0, n), rng.normal(0, 1, n), rng.normal(0, 2, (n, 3)), rng.normal(0, 5, n), rng.normal(0, 9, (n, 6))
    m[:5] = 0.0
    nrm = rng.normal(0, 1, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[5:15] = [0.0, 0.0, 1.0]
    none = np.zeros(n, dtype=int)
    none[15:25] = 1
    case = np.concatenate([m[:, None], q[:, None], v, e[:, None], w, nrm], axis=1)
    tokens = []
    for k in range(n):
        tokens += [repr(float(t)) for t in case[k]] + [int(none[k])]
    got = np.array(_rows(spatial_host(["addends", what, n] + tokens), float))
    # numpy's words through the reference: one atom per bin of a planar geometry along a made-up axis is not needed -- the formulas
    full = np.zeros((n, 10))
    absum = np.zeros((n, 10))
    full[:, 0], full[:, 1] = m, q
    full[:, 2:5] = m[:, None] * v
    full[:, 5] = m * (v * v).sum(axis=1)
    vn = (v * nrm).sum(axis=1)
    full[:, 6] = np.where(none == 1, full[:, 5] / 3.0, m * vn * vn)
    full[:, 7], full[:, 8] = e, w[:, :3].sum(axis=1)
    nn = (nrm[:, 0] ** 2 * w[:, 0] + nrm[:, 1] ** 2 * w[:, 1] + nrm[:, 2] ** 2 * w[:, 2]
          + 2.0 * (nrm[:, 0] * nrm[:, 1] * w[:, 3] + nrm[:, 0] * nrm[:, 2] * w[:, 4] + nrm[:, 1] * nrm[:, 2] * w[:, 5]))
    full[:, 9] = np.where(none == 1, full[:, 8] / 3.0, nn)
    absum[:, 5] = np.abs(full[:, 5])
    absum[:, 6] = m * np.abs(v * nrm).sum(axis=1) ** 2 + absum[:, 5]
    absum[:, 8] = np.abs(w[:, :3]).sum(axis=1)
    absum[:, 9] = np.abs(w).sum(axis=1) * 2.0
    keep = np.array([bool(what & (1 if k < 2 else 2 if k < 7 else 4)) for k in range(10)])
    assert (got[:, ~keep] == 0.0).all() and not np.signbit(got[:, ~keep]).any()
    exact = [0, 1, 2, 3, 4, 7]                                    # one product or none: the same bits
    assert np.array_equal(got[:, [k for k in exact if keep[k]]], full[:, [k for k in exact if keep[k]]])
    for k in (5, 6, 8, 9):                                        # sums of products: a few roundings apart
        if keep[k]:
            assert (np.abs(got[:, k] - full[:, k]) <= 16 * 2.0 ** -53 * absum[:, k]).all(), k
    if what & 2:
        assert (got[:5, 2:7] == 0.0).all()                       # a massless atom adds exactly 0
        planar = slice(5, 15)
        assert np.array_equal(got[planar, 6], m[planar] * (v[planar, 2] * v[planar, 2]))     # n = e_z: m v_z^2
    if what & 4:
        assert np.array_equal(got[5:15, 9], w[5:15, 2])          # n = e_z: W_zz, bit for bit


# ---------------------------------------------------------------- the run reduction and the finish
def _brute_reduce(groups, n_groups, n_bins, bins, words, chunk):
    """a straightforward loop in table order: chunk by chunk, entry by entry, each bin's addends in that order from 0.0; then the
    chunks' totals in chunk order from 0.0, added to the (zero) sums"""
    nw = words.shape[1]
    entries, chunks = _brute_layout(groups, n_groups, chunk)
    counts = np.zeros((n_groups, n_bins), dtype=np.int64)
    outside = np.zeros(n_groups, dtype=np.int64)
    sums = [[[0.0] * nw for _ in range(n_bins)] for _ in range(n_groups)]
    total = {}
    for first, count, g in chunks:
        part = {}
        for e in range(first, first + count):
            i = entries[e]
            b = int(bins[i])
            if b < 0:
                outside[g] += 1
                continue
            counts[g, b] += 1
            acc = part.setdefault(b, [0.0] * nw)
            for j in range(nw):
                acc[j] = acc[j] + float(words[i, j])
        for b, acc in part.items():
            tot = total.setdefault((g, b), [0.0] * nw)
            for j in range(nw):
                tot[j] = tot[j] + acc[j]
    for (g, b), tot in total.items():
        for j in range(nw):
            sums[g][b][j] = sums[g][b][j] + tot[j]
    return counts, outside, np.array(sums, dtype=np.float64).reshape(n_groups, n_bins, nw)


@pytest.mark.parametrize("sizes,n_bins,nw", [([1372], 1, 10), ([1372], 4096, 10), ([1372], 7, 3), ([1, 1023, 1024, 1025, 2049, 0, 3, 40], 13, 2),
                                             ([2049, 0], 64, 10)])
def test_run_reduction_and_finish_are_the_loop_in_table_order_bit_for_bit(spatial_host, chunk, sizes, n_bins, nw):
    rng = np.random.default_rng(23 + n_bins)
    groups = np.concatenate([np.full(s, g) for g, s in enumerate(sizes)] + [np.full(50, -1)]).astype(int)
    rng.shuffle(groups)
    n = len(groups)
    bins = rng.integers(-1, n_bins, n)
    words = rng.normal(0.0, 1.0, (n, nw)) * 10.0 ** rng.integers(-3, 4, (n, nw))
    tokens = []
    for i in range(n):
        tokens += [int(bins[i])] + [float(t).hex() for t in words[i]]
    out = spatial_host(["reduce", nw, len(sizes), n_bins, n, 1] + [int(g) for g in groups] + tokens).splitlines()
    counts = np.array([int(t) for t in out[0].split()]).reshape(len(sizes), n_bins)
    outside = np.array([int(t) for t in out[1].split()])
    sums = np.array([[float.fromhex(t) for t in line.split()] for line in out[2:]]).reshape(len(sizes), n_bins, nw)
    want_counts, want_outside, want_sums = _brute_reduce(groups.tolist(), len(sizes), n_bins, bins, words, chunk)
    assert np.array_equal(counts, want_counts) and np.array_equal(outside, want_outside)
    assert counts.sum() + outside.sum() == sum(sizes)
    assert np.array_equal(sums.view(np.uint64), want_sums.view(np.uint64))
    # and it is the reference's sum within the bound of the tests on the device
    ref = np.zeros((len(sizes), n_bins, nw))
    ref_abs = np.zeros((len(sizes), n_bins, nw))
    ok = (groups >= 0) & (bins >= 0)
    np.add.at(ref, (groups[ok], bins[ok]), words[ok])
    np.add.at(ref_abs, (groups[ok], bins[ok]), np.abs(words[ok]))
    assert (np.abs(sums - ref) <= sp.bound(counts, ref_abs)).all()


# ---------------------------------------------------------------- the reference itself, and the normalisation
def test_reference_profile_on_a_hand_made_configuration(spatial_host):
    pos = np.array([[0.5, 0.5, 0.25], [0.5, 0.5, 1.75], [0.5, 0.5, 2.25], [0.5, 0.5, -0.25], [0.1, 0.1, 1.0 + 1e-13]])
    vel = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    masses, charges = np.array([2.0, 1.0, 1.0, 0.0, 1.0]), np.array([1.0, -1.0, 0.5, 0.0, 0.0])
    tensors = np.tile(np.array([1.0, 2.0, 3.0, 0.1, 0.2, 0.3]), (5, 1))
    out = sp.profile(pos, vel, masses, charges, np.arange(5.0), tensors, [0, 0, 1, 0, -1], 2, sp.planar(2, 2, 0.0, 2.0), delta=1e-12)
    assert out["counts"].tolist() == [[1, 2], [1, 0]] and out["outside"].tolist() == [0, 0]     # -0.25 and 2.25 wrap
    assert np.array_equal(_planar(spatial_host, pos[:, 2], sp.planar(2, 2, 0.0, 2.0)), out["bins"])     # the library's rule, same bins
    assert out["words"][0, 0].tolist() == [2.0, 1.0, 2.0, 0.0, 4.0, 10.0, 8.0, 0.0, 6.0, 3.0]
    assert out["words"][0, 1, 0] == 1.0 and out["words"][0, 1, 5] == 1.0 and out["words"][0, 1, 7] == 1.0 + 3.0
    assert out["near"].tolist() == [0, 0, 0]                     # the ungrouped atom next to edge 1 does not count
    out = sp.profile(pos, vel, masses, charges, None, None, None, 1, sp.planar(2, 2, None, range=(0.0, 2.0)), what=3, delta=1e-12)
    assert out["counts"].tolist() == [[1, 2]] and out["outside"].tolist() == [2] and out["near"].tolist() == [0, 1, 0]
    assert (out["words"][..., 7:] == 0.0).all()
    rad = sp.radial(2, 1.0, [0.5, 0.5, 0.25], [2.0, 2.0, 2.0], (1, 1, 1))
    out = sp.profile(pos, vel, masses, None, np.arange(5.0), tensors, None, 1, rad)
    assert np.array_equal(_radial(spatial_host, pos, rad)[0], out["bins"])
    assert out["counts"].tolist() == [[2, 3]] and out["outside"].tolist() == [0]     # the centre itself, and (0.5, 0.5, 2.25) by its image
    assert out["words"][0, 0, 6] == 10.0 / 3.0 + 1.0 / 3.0 and out["words"][0, 0, 9] == 6.0 / 3.0 + 6.0 / 3.0


def test_normalisation_of_a_hand_made_record(emdee):
    V = emdee.verlet
    counts = np.array([[4, 0], [2, 2]])
    sums = np.zeros((2, 2, 10))
    sums[0, 0] = [8.0, 2.0, 4.0, 0.0, -8.0, 48.0, 16.0, -6.0, -30.0, -4.0]
    sums[1, 1] = [2.0, 0.0, 0.0, 0.0, 0.0, 6.0, 2.0, 1.0, 3.0, 1.0]
    # two frames of a box with cross-section 4 and bins 0.5 wide: V_bin = 2, inv_bin_volume_sum = 2 / 2
    out = V.spatial_profiles(V.SPATIAL_Z, [0.0, 0.5, 1.0], counts, sums, [0, 1], [5, 4], 2, 1.0)
    assert out["bin_volume"].tolist() == [2.0, 2.0] and out["centres"].tolist() == [0.25, 0.75] and out["frames"] == 2
    assert out["number_density"].tolist() == [[1.0, 0.0], [0.5, 0.5]]
    assert out["mass_density"][0, 0] == 2.0 and out["charge_density"][0, 0] == 0.5 and out["energy_density"][0, 0] == -1.5
    assert out["velocity"][0, 0].tolist() == [0.5, 0.0, -1.0] and np.isnan(out["velocity"][0, 1]).all()
    assert out["kinetic_energy"][0, 0] == 6.0 and out["kinetic_normal"][0, 0] == 2.0 and out["kinetic_tangential"][0, 0] == 2.0
    assert np.isnan(out["kinetic_energy"][0, 1])
    assert out["p_normal"][0, 0] == (16.0 - 4.0) / 4.0 and out["p_tangential"][0, 0] == ((48.0 - 16.0) + (-30.0 + 4.0)) / 8.0
    assert out["gamma_sum"].tolist() == [(3.0 - 0.75) * 0.5, ((2.0 + 1.0) / 4.0 - (4.0 + 2.0) / 8.0) * 0.5]
    assert out["outside"] == [0, 1] and out["group_sizes"] == [5, 4]
    rad = V.spatial_profiles(V.SPATIAL_RADIAL, [0.0, 1.0, 2.0], counts, sums, [0, 0], [4, 4], 1, 0.0)
    assert np.allclose(rad["bin_volume"], [4.0 * np.pi / 3.0, 4.0 * np.pi / 3.0 * 7.0], rtol=1e-15) and "gamma_sum" not in rad
    assert rad["number_density"][0, 0] == 4.0 / (4.0 * np.pi / 3.0)


# ---------------------------------------------------------------- the kernels
def test_spatial_kernels_are_in_the_report_and_use_no_scratch_memory():
    """`make report` (hipcc -Rpass-analysis=kernel-resource-usage on both kernel translation units, cross-compiled: no GPU needed):
    the kernels of a sample are there -- the gather in both precisions and its seven masks, the accumulate and the finish in seven, the
    centre -- and keep nothing in scratch"""
    src = os.path.join(ROOT, "emdee.jl_amd", "csrc")
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-s", "-C", src, "report"], timeout=1500)
    for name, real in (("resource_usage_f64.txt", "Id"), ("resource_usage_f32.txt", "If")):
        text = open(os.path.join(src, name)).read()
        fns = set()
        for b in re.split(r"remark: Function Name: ", text)[1:]:
            fn = b.split(" ", 1)[0].strip()
            if "k_spatial" not in fn:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
            assert m is not None, fn
            assert int(m.group(1)) == 0, "%s keeps %s bytes per lane in scratch memory" % (fn, m.group(1))
            fns.add(fn)
        assert sum("k_spatial_gather" + real in f for f in fns) == 7, (name, sorted(fns))
        assert sum("k_spatial_accumulate" in f for f in fns) == 7, (name, sorted(fns))
        assert sum("k_spatial_finish" in f for f in fns) == 7, (name, sorted(fns))
        assert any("k_spatial_centre" in f for f in fns), (name, sorted(fns))
