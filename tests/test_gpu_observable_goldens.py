"""GPU test of the raw words emdee_md_rdf_read, emdee_md_msd_read and emdee_md_gk_read return, bit for bit against words recorded from
the library as it was while each observable kept its table in two places (tests/golden/observable_words.json; doubles as hex
strings).  Exact comparison is what the sums allow: tests/test_gpu_rdf.py, test_gpu_msd.py and test_gpu_gk.py hold them to
run-to-run bit equality, and a change that moves no kernel and no launch moves no bit.

One engine per precision on the 256-atom fcc Lennard-Jones fluid of tests/test_gpu_observable_refusals.py, the three tables in
force together, a sample every 5 steps:
  rdf: two groups with a third of the atoms at -1, molecules of three atoms, 16 bins; the first 3 samples are its frames;
  msd: EMDEE_MSD | EMDEE_VACF, the same groups, 5 lags, an origin every 2 samples -- three ring slots, 7 samples, so that every
       slot is written at least twice;
  gk:  EMDEE_GK_STRESS | EMDEE_GK_HEAT, 4 lags, 7 samples: the ring wraps.
Then each table in force is replaced by a larger one (24 bins, 6 lags, 5 lags), sampled twice and read again: the install of a
table over a live one.

Recording (with EMDEE_HIP_LIB naming the library to record from):
    python -m tests.test_gpu_observable_goldens [out.json]"""
import json
import os
import sys

import numpy as np
import pytest

from .test_gpu_barostat import DT, _engine
from .test_gpu_observable_refusals import N, _box

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observable_words.json")
DTYPES = {"Float32": np.float32, "Float64": np.float64}
R_MAX, EVERY = 3.0, 5


def _hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def _ints(a):
    return [int(v) for v in np.asarray(a).ravel()]


def _read(md):
    r, m, g = md.rdf(), md.msd(), md.green_kubo()
    return {
        "rdf": dict(counts=_ints(r["counts"]), group_sizes=_ints(r["group_sizes"]), frames=r["frames"], inv_volume_sum=_hex(r["inv_volume_sum"])),
        "msd": dict(sums=_hex(m["sums"]), origins=_ints(m["origins"]), group_sizes=_ints(m["group_sizes"]), samples=m["samples"]),
        "gk": dict(sums=_hex(g["sums"]), totals=_hex(g["totals"]), last=_hex(g["last"]), samples=g["samples"]),
    }


def words(E, dev, dtype):
    """{"first": the three tables after 7 samples (3 frames), "replaced": the larger tables set over them, after 2}"""
    S = _box(E)
    if dtype == np.float32:
        S["pos"], S["vel"] = S["pos"].astype(np.float32).astype(np.float64), S["vel"].astype(np.float32).astype(np.float64)
    md = _engine(E, dev, S["pos"], S["vel"], S["L"], S["atoms"], dtype)
    groups, molecules = np.arange(N) % 3 - 1, np.arange(N) // 3
    md.set_rdf_(R_MAX, 16, groups, molecules, n_groups=2)
    md.set_msd_(5, origin_every=2, groups=groups, n_groups=2)
    md.set_green_kubo_(4)
    for k in range(7):
        if k < 3:
            md.rdf_sample_()
        md.msd_sample_()
        md.gk_sample_()
        md.step_(EVERY, DT)
    out = {"first": _read(md)}
    md.set_rdf_(R_MAX, 24, groups, molecules, n_groups=2)
    md.set_msd_(6, origin_every=2, groups=groups, n_groups=2)
    md.set_green_kubo_(5)
    for k in range(2):
        md.rdf_sample_()
        md.msd_sample_()
        md.gk_sample_()
        md.step_(EVERY, DT)
    out["replaced"] = _read(md)
    md.close()
    return out


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_both_precisions_and_live_sums(recorded):
    assert sorted(recorded) == sorted(DTYPES)
    for name in DTYPES:
        for stage, frames, samples in (("first", 3, 7), ("replaced", 2, 2)):
            r = recorded[name][stage]
            assert r["rdf"]["frames"] == frames and r["msd"]["samples"] == samples and r["gk"]["samples"] == samples
            assert sum(r["rdf"]["counts"]) > 1000 and r["rdf"]["group_sizes"][:2] == [(N + 1) // 3, N // 3]
            assert any(float.fromhex(v) > 0.0 for v in r["msd"]["sums"]) and any(float.fromhex(v) != 0.0 for v in r["gk"]["sums"])


@pytest.mark.parametrize("name", list(DTYPES))
def test_words_are_the_recorded_ones_bit_for_bit(emdee, dev, recorded, name):
    got, want = words(emdee, dev, DTYPES[name]), recorded[name]
    for stage in ("first", "replaced"):
        for kind in ("rdf", "msd", "gk"):
            for field, w in want[stage][kind].items():
                g = got[stage][kind][field]
                differ = sum(1 for a, b in zip(g, w) if a != b) if isinstance(w, list) else int(g != w)
                print("%s, %s, %s.%s: %d of %d words differ" % (name, stage, kind, field, differ, len(w) if isinstance(w, list) else 1))
    assert got == want


if __name__ == "__main__":
    from __graft_entry__ import load_package
    E, device = load_package(), torch.device("cuda", 0)
    recorded_now = {name: words(E, device, dtype) for name, dtype in DTYPES.items()}
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as fh:
        json.dump(recorded_now, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded %s from %s" % (", ".join(recorded_now), E._lib.LIB_PATH))
