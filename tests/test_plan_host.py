"""CPU tests of the planner (emdee.jl_amd/csrc/plan.hpp: choose_plan, plan_sizes, plan_kept, plan_holds, after_build and the LDS
sizes of the brick and typed kernels) through the stand-alone program tests/c/plan_host.cpp, built with the host compiler under
ASan and UBSan.  The sizes are compared with a restatement of the formulas in Python; the contract the kernels rely on is swept
over the flags and over populations on both sides of every threshold; the cliffs are worked by hand from the formulas; and the
`emdee plan:` lines the GPU printed before the planner became a function (tests/golden/plan_lines.json) are reproduced from
the facts and maxima of each case."""
import json
import os
import subprocess

import numpy as np
import pytest

from .conftest import GOLDEN, ROOT

LDS_LIMIT = 160 * 1024
SOA_SLOTS = 2048
EPL = 8
# brick variants (plan.hpp BrickVariant): brick shape, workgroup size, lanes per atom in the force kernels (G) and in the build (GB)
VARIANTS = {0: ((4, 2, 2), 512, 4, 8), 7: ((4, 2, 2), 1024, 4, 8), 8: ((4, 2, 2), 1024, 8, 8), 9: ((2, 2, 2), 512, 4, 8)}
NO_BRICK_PATH, NO_ATOMS, TILE_TOO_LARGE, BUILD_TOO_LARGE = 1, 2, 3, 4


@pytest.fixture(scope="session")
def plan_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_host") / "plan_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "plan_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(text, binary=False):
        r = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=300)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]      # (a sanitizer report goes to stderr and aborts)
        return r.stdout if binary else r.stdout.decode()
    return run


# ---------------------------------------------------------------- the formulas, restated from the comments of brick.hpp / typed.hpp
def _a16(x):
    return (x + 15) & ~15


def _cells(v):
    (bx, by, bz), threads, _, _ = VARIANTS[v]
    return (bx + 2) * (by + 2) * (bz + 2), bx * by * bz, threads // 64        # tile cells, own cells, wavefronts


def tables_bytes(v, own_cap):
    """off[NTC+4] | gbeg[NTC] | shift[NTC] | own[NOC+4] | wtot[waves, even] | oinfo: two ints per own atom"""
    ntc, noc, nw = _cells(v)
    return _a16(((ntc + 4) + ntc + ntc + (noc + 4) + ((nw + 1) & ~1) + 2 * own_cap) * 4)


def typed_tables_bytes(v, own_cap):
    """the same per (species, cell), two species; the shift per tile cell; oinfo and the row lengths: three ints per own atom"""
    ntc, noc, nw = _cells(v)
    return _a16(((2 * ntc + 4) + 2 * ntc + ntc + (2 * noc + 4) + ((nw + 1) & ~1) + 3 * own_cap) * 4)


def force_bytes(rb, v, tile_cap, own_cap, charged=False):
    """the HBM records (fp64 32 B; fp32 16 B + a plane of te), a plane of charges on a charged engine, the tables"""
    tile = tile_cap * (32 if rb == 8 else 16) + (_a16(tile_cap * 4) if rb == 4 else 0)
    return tile + (_a16(tile_cap * rb) if charged else 0) + tables_bytes(v, own_cap)


def soa_bytes(rb, v, own_cap):
    """three coordinate planes of SOA_SLOTS records (fp64: one record more), the tables"""
    return _a16(3 * (SOA_SLOTS + (1 if rb == 8 else 0)) * rb) + tables_bytes(v, own_cap)


def build_bytes(v, tile_cap, own_cap, stride, nsub):
    """float4 tile, the tables, one row buffer of `stride` uint16 per lane group, nine packed candidate rows per own cell and
    sub-bin and one set for the ghosts"""
    _, noc, _ = _cells(v)
    _, threads, _, gb = VARIANTS[v]
    return tile_cap * 16 + tables_bytes(v, own_cap) + (threads // gb) * stride * 2 + _a16((noc * nsub + 1) * 9 * 4)


def typed_slots(v):
    _, noc, _ = _cells(v)
    return 4608 if VARIANTS[v][1] >= 1024 else (3104 if noc == 8 else SOA_SLOTS)


def typed_force_bytes(rb, v, own_cap):
    """three planes of typed_slots records (fp64: one more), the typed tables, the four pair-constant records"""
    return _a16(3 * (typed_slots(v) + (1 if rb == 8 else 0)) * rb) + typed_tables_bytes(v, own_cap) + 256


def typed_build_bytes(v, tile_cap, own_cap, stride):
    """as build_bytes with the typed tables, a row buffer of ONE segment (half the stride, whole blocks of the force kernels'
    rows) and candidate rows per (own cell, x quarter, species)"""
    _, noc, _ = _cells(v)
    _, threads, g, gb = VARIANTS[v]
    seg = -(-(stride // 2) // (EPL * g)) * (EPL * g)
    return tile_cap * 16 + typed_tables_bytes(v, own_cap) + (threads // gb) * seg * 2 + _a16((noc * 4 + 1) * 9 * 2 * 4)


def min_stride(v):
    """the prefetched blocks of 8 G entries and the one after them"""
    _, threads, g, _ = VARIANTS[v]
    blocks = 1 if EPL * g >= 128 else (5 if g == 4 and threads >= 1024 else 2)
    return (blocks + 1) * EPL * g


def typed_min_stride(v):
    _, noc, _ = _cells(v)
    _, threads, g, _ = VARIANTS[v]
    blocks = 1 if EPL * g >= 128 else (4 if g == 4 and (threads >= 1024 or noc == 8) else 2)
    return (blocks + 1) * EPL * g


def headroom(x):
    return (x + x // 32 + 8 + 15) // 16 * 16


def test_lds_sizes_match_the_restated_formulas(plan_host):
    cases = [(rb, v, tc, oc, st, ns) for rb in (4, 8) for v in VARIANTS for tc in (64, 1000, 2048, 3104, 4608, 6208)
             for oc in (64, 352, 1056) for st in (96, 192, 288, 512) for ns in (1, 4)]
    out = plan_host("".join("sizes %d %d %d %d %d %d\n" % c for c in cases)).splitlines()
    assert len(out) == len(cases)
    for (rb, v, tc, oc, st, ns), line in zip(cases, out):
        got = [int(t) for t in line.split()]
        want = [force_bytes(rb, v, tc, oc), force_bytes(rb, v, tc, oc, True), soa_bytes(rb, v, oc), build_bytes(v, tc, oc, st, ns),
                typed_force_bytes(rb, v, oc), typed_build_bytes(v, tc, oc, st), typed_slots(v), min_stride(v), typed_min_stride(v),
                EPL * VARIANTS[v][2], VARIANTS[v][3], VARIANTS[v][1]]
        assert got == want, (rb, v, tc, oc, st, ns)


# ---------------------------------------------------------------- facts and plans
BASE = dict(real_bytes=8, M=[13, 13, 13], per=[1, 1, 1], len=[50.7, 50.7, 50.7], rlist=3.8, n=100000, n_plan=100000, nt=1, nsub=4,
            uniform=True, charged=False, ewald=False, filters_rows=False, brick_path=True, in_edit=False, stride=0, typed_stride=False,
            field16_blocked=False, typed_blocked=False, typed_all=False, typed_bricks7=False)
PLAN_FIELDS = ["active", "typed", "reason", "variant", "tile_cap", "own_cap", "row_block", "stride", "typed_stride", "build_alg",
               "span3_limit", "idx_shift", "lds_force", "lds_build", "holds", "nb0", "nb1", "nb2", "n", "asked4", "asked2"]


def _facts(f, debug=True):
    t = [f["real_bytes"], *f["M"], *f["per"], *[repr(float(x)) for x in f["len"]], repr(float(f["rlist"])), f["n"], f["n_plan"], f["nt"], f["nsub"]]
    t += [int(f[k]) for k in ("uniform", "charged", "ewald", "filters_rows", "brick_path", "in_edit")] + [f["stride"]]
    t += [int(f[k]) for k in ("typed_stride", "field16_blocked", "typed_blocked", "typed_all", "typed_bricks7")] + [int(debug)]
    return " ".join(str(x) for x in t)


def _pops(m4=(0, 0, 0), m2=(0, 0, 0), s4=0, s2=0):
    return " ".join(str(x) for x in [*m4, *m2, s4, s2])


def _parse(out):
    """[(plan dict, lines, block_typed or None)] of the program's answers to plan / after commands"""
    res, cur = [], None
    for l in out.splitlines():
        if l.startswith("plan "):
            cur = [dict(zip(PLAN_FIELDS, (int(t) for t in l.split()[1:len(PLAN_FIELDS) + 1]))), [], None]
        elif l.startswith("| "):
            cur[1].append(l[2:])
        elif l.startswith("block_typed"):
            cur[2] = int(l.split()[1])
        elif l == ".":
            res.append(tuple(cur))
    return res


def _plans(plan_host, cases):
    """cases: [(facts dict, populations string)]"""
    res = _parse(plan_host("".join("plan %s %s\n" % (_facts(f), p) for f, p in cases)))
    assert len(res) == len(cases)
    return res


def _with(**kw):
    f = dict(BASE)
    f.update(kw)
    return f


# ---------------------------------------------------------------- the contract with the kernels
TILES = [1, 63, 1900, 2047, 2048, 2400, 2560, 3103, 3300, 4000, 4607, 5200, 8300, 70000]
OWN_DIVISORS = [1, 6, 100000]                                 # most own atoms = the whole tile, a sixth of it, one atom
SPANS = [1, 119, 120, 239, 240, 600]
STRIDES = [0, 200, 512]
REC = ["rb", "nt", "uniform", "charged", "ewald", "filters", "f16", "tblocked", "tall", "b7", "tile", "own", "span", "stride_in", "mt", "mo",
       "tspan", "active", "typed", "reason", "variant", "tile_cap", "own_cap", "row_block", "stride", "build_alg", "span3_limit", "idx_shift",
       "lds_force", "lds_build", "holds", "typed_stride"]


@pytest.fixture(scope="module")
def sweep(plan_host):
    lists = "\n".join(" ".join(str(t) for t in l) for l in (TILES, OWN_DIVISORS, SPANS, STRIDES))
    raw = np.frombuffer(plan_host("sweep\n" + lists + "\n", binary=True), dtype=np.int32).reshape(-1, len(REC))
    per_flags = len(TILES) * len(OWN_DIVISORS) * len(SPANS) * len(STRIDES)
    # precision x nt x {uniform, filters, f16, tblocked, tall, b7} x {uncharged, reaction field, Ewald}, + the two inactive modes
    assert raw.shape[0] == per_flags * (2 * 3 * 2 ** 6 * 3 + 2 + 2)
    return {k: raw[:, i] for i, k in enumerate(REC)}


def _per_variant(s, fn):
    out = np.zeros(s["variant"].shape, dtype=np.int64)
    for v in VARIANTS:
        m = s["variant"] == v
        out[m] = fn(v, m)
    return out


def test_every_active_plan_keeps_the_contract_with_the_kernels(sweep):
    """Precision, nt in {1, 2, 3}, uniform, charged / Ewald, row filters, both block bits, EMDEE_TYPED_ALL, EMDEE_TYPED_BRICKS=7, the
    largest tile from 1 to past the point where nothing fits (70000: past the 16-bit slots too), the most own atoms from 1 to the
    tile, spans from 1 to 600 on both sides of 16 GB and 32 GB with and without the headroom, strides from 0 to 512: every
    combination.  (The bricks of 2 x 2 x 2 cells see two thirds of the tile and half of the own atoms, a species half of a span.)"""
    s = sweep
    a = s["active"] == 1
    assert a.sum() > 100000 and (~a).sum() > 100000
    gb = 8
    for name, ok in {
        "tile_cap holds the largest tile and the sentinel": s["tile_cap"] >= s["mt"] + 1,
        "own_cap holds the most own atoms": s["own_cap"] >= s["mo"],
        "tile slots fit 16 bits": s["tile_cap"] < 65536,
        "plan_holds for the maxima it was made from": s["holds"] == 1,
        "force kernel fits LDS": s["lds_force"] <= LDS_LIMIT,
        "build kernel fits LDS": s["lds_build"] <= LDS_LIMIT,
        "stride is whole lane-major blocks": s["stride"] % s["row_block"] == 0,
        "row_block is 8 G": s["row_block"] == _per_variant(s, lambda v, m: EPL * VARIANTS[v][2]),
        "stride holds the prefetched blocks": s["stride"] >= _per_variant(s, lambda v, m: min_stride(v)),
        "typed stride holds the typed prefetch and a block of padding": (s["typed"] == 0) | (s["stride"] >= _per_variant(s, lambda v, m: typed_min_stride(v)) + s["row_block"]),
        "typed_stride is set by typed plans alone": s["typed_stride"] == s["typed"],
        "plane offsets: the tile fits the coordinate planes": (s["idx_shift"] == 0) | (s["tile_cap"] <= np.where(s["typed"] == 1, _per_variant(s, lambda v, m: typed_slots(v)), SOA_SLOTS)),
        "the shift is that of the precision": (s["idx_shift"] == 0) | (s["idx_shift"] == np.where(s["rb"] == 8, 3, 2)),
        "single-species planes on variant 0 of uncharged uniform boxes alone": (s["idx_shift"] == 0) | (s["typed"] == 1) | ((s["variant"] == 0) & (s["uniform"] == 1) & (s["charged"] == 0)),
        "16-bit hit fields hold the widest span": (s["build_alg"] != 3) | (s["span"] <= 16 * gb),
        "32-bit hit fields hold the widest span": (s["build_alg"] != 5) | (s["span"] <= 32 * gb),
        "build_alg is 1, 3 or 5": np.isin(s["build_alg"], [1, 3, 5]),
        "a blocked 16-bit field is never taken": (s["f16"] == 0) | (s["build_alg"] != 3),
        "Ewald plans stay on variant 0": (s["ewald"] == 0) | (s["variant"] == 0),
        "charged plans take variant 0 or 8": (s["charged"] == 0) | np.isin(s["variant"], [0, 8]),
        "typed plans take variant 0, 7 or 9": (s["typed"] == 0) | np.isin(s["variant"], [0, 7, 9]),
        "variants 7 and 9 are typed plans": np.isin(s["variant"], [0, 8]) | (s["typed"] == 1),
        "typed plans: two species, no charges, no row filters, not blocked": (s["typed"] == 0) | ((s["nt"] == 2) & (s["charged"] == 0) & (s["filters"] == 0) & (s["tblocked"] == 0)),
        "the species' span fits the typed build's 16-bit fields": (s["typed"] == 0) | (s["tspan"] <= 16 * gb),
        "variant 9 leaves room for two workgroups per CU": (s["variant"] != 9) | ((s["lds_force"] <= LDS_LIMIT // 2 - 128) & (s["lds_build"] <= LDS_LIMIT // 2 - 128)),
        "lds_force is the force kernel's": s["lds_force"] == np.where(
            s["typed"] == 1, _per_variant(s, lambda v, m: np.where(s["rb"][m] == 8, typed_force_bytes(8, v, s["own_cap"][m]), typed_force_bytes(4, v, s["own_cap"][m]))),
            _per_variant(s, lambda v, m: np.where(s["rb"][m] == 8, force_bytes(8, v, s["tile_cap"][m], s["own_cap"][m]), force_bytes(4, v, s["tile_cap"][m], s["own_cap"][m]))
                         + np.where(s["charged"][m] == 1, (s["tile_cap"][m] * s["rb"][m] + 15) & ~15, 0))),
        "lds_build is the build kernel's": s["lds_build"] == np.where(
            s["typed"] == 1, _per_variant(s, lambda v, m: typed_build_bytes(v, s["tile_cap"][m], s["own_cap"][m], s["stride"][m])),
            _per_variant(s, lambda v, m: build_bytes(v, s["tile_cap"][m], s["own_cap"][m], s["stride"][m], np.where(s["nt"][m] == 1, 4, 1)))),
    }.items():
        bad = a & ~ok
        assert not bad.any(), "%s: %d plans, first %s" % (name, bad.sum(), {k: int(s[k][bad][0]) for k in REC})
    for v in VARIANTS:
        assert (a & (s["variant"] == v)).sum() > 0, "no plan of variant %d in the sweep" % v
    assert (a & (s["typed"] == 1)).sum() > 0 and (a & (s["idx_shift"] != 0) & (s["typed"] == 0)).sum() > 0
    for alg in (1, 3, 5):
        assert (a & (s["build_alg"] == alg)).sum() > 0


def test_every_inactive_plan_names_the_condition_that_failed(sweep):
    s = sweep
    ina = s["active"] == 0
    assert np.isin(s["reason"][ina], [NO_BRICK_PATH, NO_ATOMS, TILE_TOO_LARGE, BUILD_TOO_LARGE]).all() and (s["reason"][~ina] == 0).all()
    for reason in (NO_BRICK_PATH, NO_ATOMS, TILE_TOO_LARGE, BUILD_TOO_LARGE):
        assert (ina & (s["reason"] == reason)).sum() > 0, "no inactive plan with reason %d in the sweep" % reason
    # the named condition is the one that failed: with the capacities before any headroom is given back (the most the plan
    # can have asked for) the variant-0 force tile, or the largest build -- variant 8's, 128 row buffers -- is over the limit
    top = np.maximum(64, (s["tile"] + 1 + (s["tile"] + 1) // 32 + 8 + 15) // 16 * 16)
    top = np.where(s["tile"] + 1 <= SOA_SLOTS, np.minimum(top, SOA_SLOTS), top)
    own_cap = np.maximum(64, (s["own"] + s["own"] // 32 + 8 + 15) // 16 * 16)
    charge = np.where(s["charged"] == 1, (top * s["rb"] + 15) & ~15, 0)
    force = np.where(s["rb"] == 8, force_bytes(8, 0, top, own_cap), force_bytes(4, 0, top, own_cap)) + charge
    m = ina & (s["reason"] == TILE_TOO_LARGE)
    assert ((force[m] > LDS_LIMIT) | (top[m] >= 65536)).all()
    m = ina & (s["reason"] == BUILD_TOO_LARGE)
    stride = np.maximum((s["stride_in"] + 63) // 64 * 64, min_stride(8))
    assert (build_bytes(8, top, own_cap, stride, np.where(s["nt"] == 1, 4, 1))[m] > LDS_LIMIT).all()
    # ... and nothing else of an inactive plan is set
    for k in ("typed", "tile_cap", "own_cap", "idx_shift", "lds_force", "lds_build", "typed_stride"):
        assert (s[k][ina] == 0).all(), k


# ---------------------------------------------------------------- the cliffs
def _sized_tile_cap(rb, v, max_tile, max_own, stride, nsub, charged):
    """plan_sizes, restated: headroom of 1/32 + 8 rounded to 16 records, clamped to the coordinate planes where the tile fits them,
    then given back 16 records at a time while the build (weight 16) and force kernels hold fewer workgroups per CU of
    USABLE = 150000 bytes than they would at the exact size"""
    tile_cap = max(64, headroom(max_tile + 1))
    if max_tile + 1 <= SOA_SLOTS:
        tile_cap = min(tile_cap, SOA_SLOTS)
    own_cap = max(64, headroom(max_own))
    exact, st = max(64, (max_tile + 1 + 15) // 16 * 16), stride if stride > 0 else 128
    per_cu = lambda tc: 150000 // build_bytes(v, tc, own_cap, st, nsub) * 16 + 150000 // force_bytes(rb, v, tc, own_cap, charged)
    top = tile_cap
    while tile_cap > exact and per_cu(tile_cap) < per_cu(exact):
        tile_cap -= 16
    return tile_cap, own_cap, exact, top, per_cu


def test_the_tile_of_2048_records_is_the_last_with_plane_offsets(plan_host):
    """A uniform fp64 box.  max_tile = 2047: 2048 records with the sentinel; the headroom asks for (2048 + 64 + 8 + 15) / 16 * 16 =
    2128, the clamp to SOA_SLOTS = 2048 applies because 2048 <= 2048: tile_cap 2048, entries are plane offsets (shift 3).
    max_tile = 2048: 2049 records do not fit the planes, no clamp; tile_cap is between (2049 + 15) / 16 * 16 = 2064 and 2128 and
    the entries are tile slots."""
    (lo, _, _), (hi, _, _) = _plans(plan_host, [(_with(), _pops((2047, 300, 60))), (_with(), _pops((2048, 300, 60)))])
    assert lo["active"] and lo["variant"] == 0 and lo["tile_cap"] == 2048 and lo["idx_shift"] == 3
    assert hi["active"] and hi["variant"] == 0 and 2064 <= hi["tile_cap"] <= 2128 and hi["idx_shift"] == 0
    # fp32: the same tile, shift 2
    (lo32, _, _), = _plans(plan_host, [(_with(real_bytes=4), _pops((2047, 300, 60)))])
    assert lo32["tile_cap"] == 2048 and lo32["idx_shift"] == 2


def test_half_a_cu_of_lds_moves_uncharged_boxes_to_1024_threads_and_leaves_ewald_boxes(plan_host):
    """fp64, 300 own atoms: own_cap = (300 + 9 + 8 + 15) / 16 * 16 = 320, the tables of variant 0 are (320 + 2 * 320) * 4 = 3840 B
    (96 tile cells, 16 own cells, 8 wavefronts: 100 + 96 + 96 + 20 + 8 = 320 ints), a tile is 32 B per record: the force kernel
    passes LDS_LIMIT / 2 = 81920 B from tile_cap = 2448 on (32 * 2448 + 3840 = 82176; 2432 gives 81664).  The first line of every
    plan is the sizing of variant 0: the plan takes variant 8 exactly where that line's capacities pass half the limit.  The
    Ewald box (a charge plane of 8 B per record more: over the half from tile_cap = 1952 on) stays on variant 0 throughout."""
    assert force_bytes(8, 0, 2448, 320) == 82176 and force_bytes(8, 0, 2432, 320) == 81664
    tiles = list(range(1700, 2700, 3))
    plain = _plans(plan_host, [(_with(uniform=False), _pops((t, 300, 60))) for t in tiles])
    ewald = _plans(plan_host, [(_with(uniform=False, charged=True, ewald=True), _pops((t, 300, 60))) for t in tiles])
    moved = []
    for t, (p, lines, _) in zip(tiles, plain):
        first = lines[0]
        assert first.endswith("variant 0"), first
        tc, oc = int(first.split("tile_cap ")[1].split()[0]), int(first.split("own_cap ")[1].split()[0])
        assert oc == 320
        over = force_bytes(8, 0, tc, oc) > LDS_LIMIT // 2
        assert over == (tc >= 2448)
        assert p["active"] and p["variant"] == (8 if over else 0), (t, lines)
        moved.append(over)
    first_over = moved.index(True)
    assert 0 < first_over and all(moved[first_over:]) and not any(moved[:first_over])
    n_over = 0
    for t, (p, lines, _) in zip(tiles, ewald):
        assert p["active"] and p["variant"] == 0 and len([l for l in lines if l.startswith("emdee plan: bricks")]) == 1, (t, lines)
        n_over += p["lds_force"] > LDS_LIMIT // 2
    assert n_over > 0


def test_the_span_of_a_tile_row_picks_the_hit_fields(plan_host):
    """The build is picked from the widest three-cell span WITH its headroom, span + span / 16 + 2, against 16 GB = 128 and
    32 GB = 256 (GB = 8 lanes per atom in every variant): a measured span of 119 plans for 119 + 7 + 2 = 128 and keeps the 16-bit
    fields (ALG 3); 120 plans for 129 and takes the 32-bit fields (ALG 5); 239 plans for 239 + 14 + 2 = 255 and keeps them; 240
    plans for 257 and takes the ballot build (ALG 1), which has no limit.  (No span plans for exactly 256.  A MEASURED span of
    128 or 256 is therefore already on the far side: 128 + 8 + 2 = 138, 256 + 16 + 2 = 274.)  A blocked 16-bit field goes
    straight to the 32-bit ones."""
    spans = [119, 120, 128, 239, 240, 256]
    res = _plans(plan_host, [(_with(), _pops((1800, 300, sp))) for sp in spans])
    assert [p["build_alg"] for p, _, _ in res] == [3, 5, 5, 5, 1, 1]
    assert [p["span3_limit"] for p, _, _ in res] == [128, 256, 256, 256, 1 << 30, 1 << 30]
    res = _plans(plan_host, [(_with(field16_blocked=True), _pops((1800, 300, sp))) for sp in spans])
    assert [p["build_alg"] for p, _, _ in res] == [5, 5, 5, 5, 1, 1]


def test_headroom_is_given_back_only_for_a_workgroup_per_cu(plan_host):
    """tile_cap is never below the exact size ((max_tile + 1 + 15) / 16 * 16), and below the full headroom only as far as the
    USABLE rule asks: the first size, going down, at which the kernels hold as many workgroups per CU as at the exact size."""
    cases = [(rb, charged, stride, t) for rb in (4, 8) for charged in (False, True) for stride in (0, 96, 200) for t in range(1, 6000, 7)]
    res = _plans(plan_host, [(_with(real_bytes=rb, uniform=False, charged=charged, stride=stride), _pops((t, max(1, t // 6), 60)))
                             for rb, charged, stride, t in cases])
    lowered = 0
    for (rb, charged, stride, t), (_, lines, _) in zip(cases, res):
        first = lines[0]                                          # (the sizing of variant 0, whatever the plan goes on to)
        tc = int(first.split("tile_cap ")[1].split()[0])
        want, own_cap, exact, top, per_cu = _sized_tile_cap(rb, 0, t, max(1, t // 6), stride, 4, charged)
        assert tc == want and exact <= tc <= top, (rb, charged, stride, t, first)
        if tc < top:
            lowered += 1
            assert per_cu(tc + 16) < per_cu(exact) and (tc == exact or per_cu(tc) >= per_cu(exact))
    assert lowered > 0


# ---------------------------------------------------------------- kept plans, after_build
def test_a_plan_is_kept_for_the_same_grid_flags_and_about_as_many_atoms(plan_host):
    pops = _pops((1800, 300, 60))
    a = _with(n=80000, n_plan=80000)
    others = {
        "same": (a, 1), "Mx": (_with(n=80000, M=[12, 13, 13]), 0), "My": (_with(n=80000, M=[13, 14, 13]), 0), "Mz": (_with(n=80000, M=[13, 13, 12]), 0),
        "uniform": (_with(n=80000, uniform=False), 0), "charged": (_with(n=80000, charged=True), 0), "nt": (_with(n=80000, nt=2), 0),
        # the window: plan.n <= n + n / 8 and n <= plan.n + plan.n / 8 (integer divisions)
        "n up, inside": (_with(n=90000), 1), "n up, outside": (_with(n=90001), 0),
        "n down, inside": (_with(n=71112), 1), "n down, outside": (_with(n=71111), 0),
        "no atoms": (_with(n=0), 0), "direct path": (_with(n=80000, brick_path=False), 0),
        # inside an in-place edit n is an upper bound: the count before the edit decides
        "edit, n_plan inside": (_with(n=200000, n_plan=80000, in_edit=True), 1),
        "edit, n_plan outside": (_with(n=80000, n_plan=95000, in_edit=True), 0),
    }
    out = plan_host("".join("kept %s %s %s\n" % (_facts(a), pops, _facts(b)) for b, _ in others.values())).split()
    got = [int(t) for t in out[1::2]]
    assert got == [w for _, w in others.values()], dict(zip(others, got))
    assert 80000 <= 71112 + 71112 // 8 and 80000 > 71111 + 71111 // 8 and 90000 <= 80000 + 80000 // 8
    # a plan made inside an edit remembers the count before the edit
    (p, _, _), = _plans(plan_host, [(_with(n=200000, n_plan=80000, in_edit=True), pops)])
    assert p["n"] == 80000
    # an inactive plan is never kept
    out = plan_host("kept %s %s %s\n" % (_facts(_with(brick_path=False)), pops, _facts(_with(brick_path=False))))
    assert out.split() == ["kept", "0"]


def test_after_build_grows_the_stride_blocks_the_typed_kernels_and_gives_way_to_the_direct_ones(plan_host, golden_cases):
    def after(key, needed):
        c = golden_cases[key]
        return _parse(plan_host("after %s %s %d\n" % (_facts(c["facts"]), _case_pops(c), needed)))[0]
    # rows of 100 under a stride of 96: (100 + 12 + 15) / 16 * 16 = 112, whole blocks of 32: 128; 64 row buffers grow by 32 uint16
    p, _, block = after(("uniform", 64, "load"), 100)
    assert p["active"] and p["stride"] == 128 and p["lds_build"] == 49200 + 64 * 32 * 2 and block == 0
    # the typed plan of variant 9 at rows of 2000: (2000 + 250 + 15) / 16 * 16 = 2256 -> 2272; 64 segments of 1152 entries do not fit
    p, _, block = after(("typed", 64, "load"), 2000)
    assert p["active"] and p["typed"] and p["stride"] == 2272 and p["lds_build"] > LDS_LIMIT and block == 1
    # the fp32 long-row box (build at 160592 B of 163840) at rows of 300: 352 -> 384, 128 row buffers grow by 192 uint16
    p, _, block = after(("long_rows", 32, "load"), 300)
    assert not p["active"] and p["reason"] == BUILD_TOO_LARGE and p["stride"] == 384 and block == 0
    # an engine on the direct kernels: an eighth more, rounded to 16
    p, _, block = after(("direct", 64, "load"), 100)
    assert not p["active"] and p["stride"] == 112 and block == 0


# ---------------------------------------------------------------- the lines recorded before the planner became a function
@pytest.fixture(scope="module")
def golden_cases():
    with open(os.path.join(GOLDEN, "plan_lines.json")) as fh:
        return {(c["case"], c["bits"], c["event"]): c for c in json.load(fh)}


def _case_pops(c):
    return _pops(c["maxima"].get("4x2x2", (0, 0, 0)), c["maxima"].get("2x2x2", (0, 0, 0)), c["typed_span"].get("4x2x2", 0), c["typed_span"].get("2x2x2", 0))


def test_the_recorded_plan_lines_are_reproduced_from_their_facts(plan_host, golden_cases):
    assert len(golden_cases) == 16
    keys = list(golden_cases)
    res = _plans(plan_host, [(golden_cases[k]["facts"], _case_pops(golden_cases[k])) for k in keys])
    for k, (p, lines, _) in zip(keys, res):
        assert lines == golden_cases[k]["lines"], k
        assert p["active"] == (k[0] != "direct")
        # every sizing asks the measure for its shape's maxima (the engine's measure reads a shape back once per plan)
        assert p["asked4"] == len([l for l in lines if l.startswith("emdee plan: bricks") and not l.endswith("variant 9")])
    want = {"uniform": 0, "species3": 0, "long_rows": 8, "typed": 9, "typed_all": 0, "long_rows_charged": None}
    for k, (p, _, _) in zip(keys, res):
        if want.get(k[0]) is not None:
            assert p["variant"] == want[k[0]], k


def test_a_plan_does_not_depend_on_what_was_planned_before(plan_host, golden_cases):
    """every recorded case alone, and in one process after each of two unrelated ones (a typed plan, a direct engine)"""
    keys = list(golden_cases)
    one = lambda k, debug=True: "plan %s %s\n" % (_facts(golden_cases[k]["facts"], debug), _case_pops(golden_cases[k]))
    alone = [plan_host(one(k)) for k in keys]
    for before in (("typed", 64, "load"), ("direct", 32, "load"), ("long_rows_charged", 32, "ewald")):
        out = plan_host("".join(one(before) + one(k) for k in keys))
        chunks = [c + ".\n" for c in out.split(".\n") if c]
        assert len(chunks) == 2 * len(keys)
        assert chunks[1::2] == alone
    # without EMDEE_DEBUG_PLAN: the same plan, no text
    for k, a in zip(keys, alone):
        quiet = plan_host(one(k, debug=False))
        assert quiet.splitlines()[0] == a.splitlines()[0] and quiet.splitlines()[1:] == ["."]
