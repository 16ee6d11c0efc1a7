"""CPU test of the gate the entries of the three observables pass a table and the engine's facts through (the part of
emdee.jl_amd/csrc/observables.hpp with no HIP in it), through the stand-alone program tests/c/observables_host.cpp, built with the host
compiler under ASan and UBSan.  Every message is held against the entry of tests/golden/observable_refusal_texts.json that
tests/test_gpu_observable_refusals.py holds the library to: texts recorded on the GPU from the library as it was while each
observable formed its refusals on its own."""
import json
import os
import subprocess

import pytest

from .conftest import ROOT

KINDS = {"rdf": 0, "msd": 1, "gk": 2}
N, L = 256, 6.84                                          # the atoms and the side of the box the texts were recorded on


@pytest.fixture(scope="session")
def gate(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("observables_host") / "observables_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "observables_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        out = r.stdout.rstrip("\n")
        if out == "OK":
            return None
        word, code, message = out.split(" ", 2)
        assert word == "REFUSED"
        return [int(code), "libemdee_hip status %d: %s" % (int(code), message)]
    return run


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "observable_refusal_texts.json")) as fh:
        return json.load(fh)


def _engine(n_owned=N, serial=1, lengths=(L, L, L), lent=0, has_ghosts=0, is_sorted=1, id_gaps=0, n_ghost=0):
    return [lent, has_ghosts, is_sorted, id_gaps, n_owned, n_ghost, serial] + [repr(float(v)) for v in lengths]


def _table(n_atoms=N, serial=1, lengths=(L, L, L)):
    return [n_atoms, serial] + [repr(float(v)) for v in lengths]


@pytest.mark.parametrize("kind", list(KINDS))
def test_no_table_refuses_sample_read_and_reset_with_the_recorded_texts(gate, recorded, kind):
    for verb, key in (("sample", "sample"), ("reset", "reset"), ("read", "read_null")):
        assert gate("present", KINDS[kind], verb, 0) == recorded["%s/no_table/%s" % (kind, key)] == recorded["%s/cleared/%s" % (kind, key)]
        assert gate("present", KINDS[kind], verb, 1) is None


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_fitting_table_passes_and_another_atom_count_is_the_recorded_refusal(gate, recorded, kind):
    k = KINDS[kind]
    assert gate("fit", k, *_table(), *_engine()) is None
    want = recorded["%s/sample/atom_count" % kind]
    assert "set for 256 atoms, the state holds 253" in want[1]
    assert gate("fit", k, *_table(), *_engine(n_owned=N - 3)) == want
    # ... which comes before the state and the box: a reset pins both again and the table still does not fit
    assert gate("fit", k, *_table(), *_engine(n_owned=N - 3, serial=2, lengths=(L, L, 0.999 * L))) == want
    assert recorded["%s/sample/atom_count_after_reset" % kind] == want
    # an engine that is not what the table was set on holds no state of that count either
    for facts in (dict(is_sorted=0), dict(id_gaps=1), dict(n_ghost=4)):
        assert gate("fit", k, *_table(), *_engine(**facts)) == [want[0], want[1].replace("holds 253", "holds 256")]


@pytest.mark.parametrize("kind", ["msd", "gk"])
def test_a_replaced_state_and_a_rescaled_box_are_the_recorded_refusals(gate, recorded, kind):
    k = KINDS[kind]
    replaced, rescaled = recorded["%s/sample/state_replaced" % kind], recorded["%s/sample/box_rescaled" % kind]
    assert gate("fit", k, *_table(serial=1), *_engine(serial=2)) == replaced
    for axis in range(3):
        lengths = [L, L, L]
        lengths[axis] *= 0.999
        assert gate("fit", k, *_table(), *_engine(lengths=lengths)) == rescaled
    assert gate("fit", k, *_table(serial=1), *_engine(serial=2, lengths=(0.999 * L, L, L))) == replaced      # the state first
    assert replaced != rescaled and replaced[0] == rescaled[0] == -6


def test_a_frame_of_the_rdf_pins_neither_the_state_nor_the_box(gate):
    assert gate("fit", KINDS["rdf"], *_table(serial=1), *_engine(serial=5, lengths=(0.9 * L, L, 1.1 * L))) is None


@pytest.mark.parametrize("kind", list(KINDS))
def test_engines_that_do_not_see_the_whole_box_are_the_recorded_refusals(gate, recorded, kind):
    fn = "set_" + kind
    assert gate("whole_box", fn, *_engine()) is None
    assert gate("whole_box", fn, *_engine(lent=1, has_ghosts=1, n_ghost=4, is_sorted=0)) == recorded["engines/lent/" + kind]
    assert gate("whole_box", fn, *_engine(has_ghosts=1, is_sorted=0)) == recorded["engines/ghosts/" + kind]
    assert gate("whole_box", fn, *_engine(n_ghost=4)) == recorded["engines/ghosts/" + kind]
    assert gate("whole_box", fn, *_engine(is_sorted=0)) == recorded["engines/no_state/" + kind]
    assert gate("whole_box", fn, *_engine(id_gaps=1)) == recorded["engines/no_state/" + kind]


@pytest.mark.parametrize("kind", ["rdf", "msd"])
def test_group_entries_out_of_range_are_the_recorded_refusals(gate, recorded, kind):
    good = [i % 2 for i in range(N)]
    assert gate("groups", KINDS[kind], 2, N, *good) is None
    assert gate("groups", KINDS[kind], 2, N, *[-1] * N) is None and gate("groups", KINDS[kind], 1, 0) is None
    for name, at in (("first", 0), ("middle", 123), ("last", N - 1)):
        for which, value in (("high", 2), ("low", -2)):
            bad = list(good)
            bad[at] = value
            assert gate("groups", KINDS[kind], 2, N, *bad) == recorded["%s/set/group_%s_%s" % (kind, which, name)]
