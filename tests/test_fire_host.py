"""CPU tests of the update rules of energy minimisation (include/emdee_hip.h: emdee_md_minimize): fire_cap and fire_update of
emdee.jl_amd/csrc/minimize.hpp through the stand-alone program tests/c/fire_host.cpp, built with the host compiler under ASan and
UBSan, against the closed-form root and against tests/helpers/fire_ref.py; and that reference itself on a small box (it
converges, and a reversed atom order changes nothing but rounding)."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import fire_ref as fr

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="session")
def fire_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fire_host") / "fire_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "fire_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _cap(fire_host, rows):
    case = ["cap", len(rows)]
    for row in rows:
        case += [repr(float(t)) for t in row]
    out = [float(t) for t in fire_host(case).split()]
    assert len(out) == len(rows)
    return np.array(out)


def test_fire_cap_is_the_closed_form_root(fire_host):
    """capped rows: t is the positive root of amax t^2 / 2 + vmax t - max_step = 0.  Written as (-v + sqrt(v^2 + 2 a s)) / a the
    root loses digits by cancellation: its relative error is about eps (v + sqrt(...)) / (a t) = 2 eps s / (a t^2), which the
    bound below carries per row (with a factor 8 for the roundings of the other operations)."""
    rng = np.random.default_rng(3)
    rows = np.column_stack([10.0 ** rng.uniform(-3.0, 0.3, 200), rng.uniform(0.1, 5.0, 200), rng.uniform(0.1, 50.0, 200), rng.uniform(0.01, 0.2, 200)])
    dt, v, a, s = rows.T
    got = _cap(fire_host, rows)
    root = (-v + np.sqrt(v * v + 2.0 * a * s)) / a
    capped = dt * v + 0.5 * dt * dt * a > s
    assert capped.sum() >= 50 and (~capped).sum() >= 20
    bound = 8.0 * EPS * (1.0 + 2.0 * s / (a * root * root))
    assert (np.abs(got[capped] / root[capped] - 1.0) <= bound[capped]).all()
    assert (got[~capped] == dt[~capped]).all()
    assert (got <= dt).all()
    # (and the python reference is the same function)
    assert np.array_equal(got, np.array([fr.fire_cap(*row) for row in rows]))


def test_fire_cap_at_zero_speed_zero_acceleration_and_uncapped(fire_host):
    rows = np.array([[1.0, 0.0, 400.0, 0.1],        # v = 0: t = sqrt(2 s / a)
                     [1.0, 25.0, 0.0, 0.1],         # a = 0: t = s / v
                     [0.01, 0.0, 0.0, 0.1],         # both zero: nothing to cap
                     [0.01, 1.0, 10.0, 0.1],        # uncapped: 0.01 + 0.0005 <= 0.1
                     [2.0, 0.0, 1e12, 0.1],         # an overlap: a huge acceleration
                     [2.0, 1e-9, 1e12, 0.1],
                     [2.0, 1e6, 1e-9, 0.1]])
    got = _cap(fire_host, rows)
    dt, v, a, s = rows.T
    want = np.array([np.sqrt(2.0 * 0.1 / 400.0), 0.1 / 25.0, 0.01, 0.01, np.sqrt(2.0 * 0.1 / 1e12), np.nan, np.nan])
    assert got[2] == 0.01 and got[3] == 0.01
    for k in (0, 1, 4):
        assert abs(got[k] / want[k] - 1.0) <= 4.0 * EPS, (k, got[k], want[k])
    # every capped row lands on the bound: t v + t^2 a / 2 = s to rounding, never meaningfully beyond it
    drift = got * v + 0.5 * got * got * a
    for k in (0, 1, 4, 5, 6):
        assert abs(drift[k] / s[k] - 1.0) <= 8.0 * EPS, (k, drift[k])
    assert np.array_equal(got, np.array([fr.fire_cap(*row) for row in rows]))


def test_fire_update_reproduces_the_reference_sequence(fire_host):
    """a recorded sign sequence of P: six positives (n_pos crosses N_min at the sixth), growth until dt_max is hit and held, a
    reset, a second climb cut short, two resets in a row, a zero (P <= 0 resets) and a last climb"""
    signs = [+1] * 20 + [-1] + [+1] * 7 + [-1, -1, 0] + [+1] * 9
    rng = np.random.default_rng(4)
    P = [s * float(rng.uniform(0.1, 3.0)) for s in signs]
    dt_start, dt_max = 0.002, 0.0065
    out = [line.split() for line in fire_host(["update", repr(dt_start), repr(dt_max), len(P)] + [repr(p) for p in P]).splitlines()]
    assert len(out) == len(P)
    ref, hit_max, crossed = fr.State(dt_start, dt_max), False, False
    for k, p in enumerate(P):
        before = ref.dt
        mix = fr.fire_update(ref, p)
        got = (int(out[k][0]), float(out[k][1]), float(out[k][2]), int(out[k][3]))
        assert got == (int(mix), ref.dt, ref.alpha, ref.n_pos), (k, got, (mix, ref.dt, ref.alpha, ref.n_pos))
        crossed = crossed or (ref.n_pos == fr.N_MIN + 1 and ref.dt > before)
        hit_max = hit_max or (ref.dt == dt_max and before == dt_max and mix)
    assert crossed and hit_max
    # the first five positives leave dt and alpha alone
    assert all(float(out[k][1]) == dt_start and float(out[k][2]) == fr.ALPHA0 for k in range(5))
    assert float(out[5][1]) == fr.F_INC * dt_start and float(out[5][2]) == fr.F_ALPHA * fr.ALPHA0
    assert float(out[20][1]) == fr.F_DEC * dt_max and float(out[20][2]) == fr.ALPHA0 and int(out[20][3]) == 0
    assert int(out[30][0]) == 0 and int(out[30][3]) == 0                      # (P = 0 resets)


def test_reference_converges_and_does_not_depend_on_the_atom_order():
    """fire_ref on a perturbed 2 x 2 x 2 fcc box (32 atoms, all pairs): the energy falls, g_max reaches 1e-6, and the atoms in
    reversed order take the same path up to the rounding of the sums"""
    rng = np.random.default_rng(8)
    a = 2.0 ** (2.0 / 3.0)
    cell = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    x = np.array([(np.array([i, j, k]) + c) * a for i in range(2) for j in range(2) for k in range(2) for c in cell])
    lengths, lo = np.array([2 * a, 2 * a, 2 * a]), np.array([-0.5, 0.25, 1.0])
    x = x + lo + 0.05 * (rng.random(x.shape) - 0.5)
    mass = rng.uniform(1.0, 4.0, len(x))
    atoms = np.zeros(len(x), dtype=np.dtype([("half_sigma", np.float32), ("twice_sqrt_eps", np.float32)]))
    atoms["half_sigma"], atoms["twice_sqrt_eps"] = 0.5, 2.0
    force = fr.lj(lo, lengths, [1, 1, 1], 1.5, 1.2, atoms)
    out = fr.minimize(x, force, mass, 400, 1e-6, 0.002, 0.02, 0.1)
    assert out["converged"] and out["g_max"] <= 1e-6 and out["energy"] < out["energy0"]
    assert out["iterations"] == len(out["records"]) - 1
    back = fr.minimize(x[::-1], fr.lj(lo, lengths, [1, 1, 1], 1.5, 1.2, atoms[::-1]), mass[::-1], 400, 1e-6, 0.002, 0.02, 0.1)
    assert back["iterations"] == out["iterations"]
    assert np.abs(back["x"][::-1] - out["x"]).max() <= 1e-9


def test_reference_iteration_count_on_the_parity_box():
    """the count tests/test_gpu_minimize.py caps at three times: fire_ref reaches g_max <= 1e-8 on fcc_box() in 334 iterations"""
    B = fr.fcc_box()
    force = fr.lj(fr.LO, B["lengths"], [1, 1, 1], float(B["rc"]), float(B["rs"]), B["atoms"])
    out = fr.minimize(B["pos"], force, B["mass"], 1000, 1e-8, **fr.PARAMS)
    assert out["converged"] and out["iterations"] == 334
    assert (B["lengths"] >= 2.0 * (B["rc"] + B["skin"])).all() and len(set(B["lengths"])) == 3
