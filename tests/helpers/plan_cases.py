"""The boxes whose `emdee plan:` lines tests/golden/plan_lines.json records, and how a plan event is read from the debug text.

A case is one engine on a family box of mask_cases (both precisions); a plan event is one run of the planner on it: the load, and
for the charged long-row box the replans of set_coulomb_ (reaction field) and set_ewald_.  run() yields, per event, the row stride
the list had before it and the lines the planner printed.  facts() restates what the engine hands the planner for the event
(nbsys.hpp configure_grid, build_list's first stride), and maxima() reads the populations back out of the lines themselves, so
that the host test can feed both to choose_plan without a GPU."""
import math
import re

import numpy as np

from . import mask_cases as mc

SKIN = 0.3
EWALD_ALPHA, EWALD_KMAX = 1.0, 4


def _dtype(bits):
    return np.float64 if bits == 64 else np.float32


def first_stride(n, lengths, rlist):
    """build_list's first guess of the row stride (nbsys.hpp)"""
    expect = (4.0 / 3.0) * math.pi * rlist ** 3 * n / (lengths[0] * lengths[1] * lengths[2]) if n > 0 else 0.0
    return int((expect * 1.15 + 8.0) / 16.0 + 1.0) * 16


def cell_grid(n, lengths, rlist):
    """configure_grid (nbsys.hpp)"""
    M = [min(max(1, int(math.floor(l / rlist))), 1024) for l in lengths]
    while M[0] * M[1] * M[2] > 4 * max(n, 16) + 64:
        big = max(range(3), key=lambda d: (M[d], -d))
        if M[big] <= 1:
            break
        M[big] = (M[big] + 1) // 2
    return M


def run(E, dev, family, bits, read_err, setenv):
    """(box, [(event name, stride before, lines)]) -- read_err() returns (and clears) what the library wrote to stderr since the last
    call; setenv(name, value) sets the box's environment and EMDEE_DEBUG_PLAN for the engine"""
    import torch
    dtype = _dtype(bits)
    charged = family == "long_rows_charged"
    box = mc.family_box(E, "long_rows" if charged else family, dtype)
    n = box["pos"].shape[0]
    rlist = math.sqrt(box["rc"] * box["rc"]) + SKIN
    plans = lambda: [l for l in read_err().splitlines() if l.startswith("emdee plan")]
    for k, v in box["env"].items():
        setenv(k, v)
    setenv("EMDEE_DEBUG_PLAN", "1")
    read_err()
    md = E.VelocityVerlet(E.cu(box["pos"].astype(dtype), dev), E.cu(box["vel"].astype(dtype), dev), box["lengths"][0],
                          E.LennardJonesModel(box["rc"], box["rs"]), E.cu(box["atoms"], dev), skin=SKIN, lo=[0.0, 0.0, 0.0],
                          lengths=box["lengths"], periodic=box["periodic"])
    torch.cuda.synchronize()
    events = [("load", first_stride(n, box["lengths"], rlist), plans())]
    if charged:
        q = 0.5 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        events = []                                            # (the load is the long_rows case's)
        stride = md.nbr_stats()["capacity"]
        md.set_coulomb_(q, 1.0, 6.0 if bits == 64 else np.inf)
        torch.cuda.synchronize()
        events.append(("reaction_field", stride, plans()))
        stride = md.nbr_stats()["capacity"]
        md.set_ewald_(EWALD_ALPHA, EWALD_KMAX)
        torch.cuda.synchronize()
        events.append(("ewald", stride, plans()))
    md.close()
    return box, events


def facts(box, family, bits, event, stride):
    """the planner's input for the event, as plan_host reads it"""
    n = box["pos"].shape[0]
    rlist = math.sqrt(box["rc"] * box["rc"]) + SKIN
    kinds = len(np.unique(np.asarray(box["atoms"])))
    nt = 2 if kinds == 2 else 1
    brick = box["env"].get("EMDEE_PATH") != "direct"
    return dict(real_bytes=bits // 8, M=cell_grid(n, box["lengths"], rlist), per=list(box["periodic"]), len=list(box["lengths"]),
                rlist=rlist, n=n, n_plan=n, nt=nt, nsub=4 if (nt == 1 and brick) else 1, uniform=kinds == 1,
                charged=event != "load", ewald=event == "ewald", filters_rows=False, brick_path=brick, in_edit=False, stride=stride,
                typed_stride=False, field16_blocked=False, typed_blocked=False, typed_all="EMDEE_TYPED_ALL" in box["env"],
                typed_bricks7=False)


_BRICKS = re.compile(r"emdee plan: bricks .* \(max (\d+)\), own_cap \d+ \(max (\d+)\), max 3-cell span (\d+), .* variant (\d+)$")
_TYPED = re.compile(r"emdee plan: two species, variant (\d+): .* longest 3-cell span of one species (\d+),")


def shape_of(variant):
    return "2x2x2" if variant == 9 else "4x2x2"


def maxima(lines):
    """({shape: [largest tile, most own atoms, widest span]}, {shape: widest span of one species}) as the lines print them"""
    pops, spans = {}, {}
    for l in lines:
        m = _BRICKS.match(l.rstrip())
        if m:
            pops[shape_of(int(m.group(4)))] = [int(m.group(k)) for k in (1, 2, 3)]
        m = _TYPED.match(l.rstrip())
        if m:
            spans[shape_of(int(m.group(1)))] = int(m.group(2))
    return pops, spans
