"""GPU test of the box sums behind emdee_md_energies and emdee_md_pressure_tensor (csrc/reduce.hpp: k_reduce_partials over EnergySums
and TensorSums, k_reduce_final) against fp64 numpy sums of the per-atom values the engine itself returns.

A single-species Lennard-Jones box at n = 1, 255, 256, 257 -- one block of 256 threads less one, full, and a second block of one
thread -- and 275,684 = 4 x 41^3, past the 256 x 1024 = 262,144 slots one pass of the grid covers, so the stride loop runs twice.

The bound.  The per-atom energies, virials and tensors convert to fp64 exactly, so a sum of n of them, in whatever order, differs
from the exact sum by at most (n - 1) 2^-53 sum |terms|; the reference is math.fsum, the exact sum rounded once, which takes less
than one more 2^-53 sum |terms|: |got - want| <= n 2^-53 sum |terms| per word.  A kinetic term is a product of three or four fp64
factors formed on the device and again in numpy, each of which may lose a rounding or keep one to contraction, as the heat addends
of tests/test_gk_host.py do: the same bound with a factor 8."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -53
SIZES = [1, 255, 256, 257, 275684]


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


_BOXES = {}


def _box(syn, n):
    """n atoms of a jittered fcc box (4 cells a side for the small ones, 41 for 275,684): one short of it, all of it, or one more in
    the middle of the first cell; n = 1: the first atom alone.  Velocities at T* = 1.2, masses in [1, 4]."""
    if n not in _BOXES:
        cells = 41 if n > 257 else 4
        pos, L = syn.fcc_positions(cells)
        full = len(pos)
        if n > full:
            a = L / cells
            pos = np.concatenate([pos, np.full((n - full, 3), 0.5 * a)])
        pos = pos[:n]
        rng = np.random.default_rng(n)
        _BOXES[n] = dict(pos=pos, vel=syn.velocities(max(n, 2), 1.2)[:n], L=L, mass=rng.uniform(1.0, 4.0, n))
    return _BOXES[n]


def _engine(E, dev, B, dtype, inv_mass):
    n = len(B["pos"])
    im = None if inv_mass is None else E.cu(np.asarray(inv_mass).astype(dtype), dev)
    return E.VelocityVerlet(E.cu(B["pos"].astype(dtype), dev), E.cu(B["vel"].astype(dtype), dev), B["L"], E.LennardJonesModel(2.5, 2.0),
                            E.cu(E.lennard_jones_atoms(1.0, 1.0, n), dev), inv_mass=im)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _word(what, got, terms, factor=1):
    """one word against the exact sum of its terms (n, ...): the last axis of `terms` holds the addends of one atom"""
    terms = terms.reshape(len(terms), -1)
    want, size = math.fsum(terms.ravel()), math.fsum(np.abs(terms).ravel())
    bound = factor * len(terms) * U * size
    print("%-28s got %r want %r |got - want| %.3e bound %.3e" % (what, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound, (what, got, want, bound)


def _check(E, dev, B, dtype, inv_mass, what):
    md = _engine(E, dev, B, dtype, inv_mass)
    n = len(B["pos"])
    ep, ek, w = md.totals()
    st = md.state(positions=False, forces=False, energies=True, virials=True)
    sums = md.tensor_sums()
    vt, v = _np(md.virial_tensor()), _np(st["velocities"])
    md.close()
    # the masses as the engine holds them: 1 / inv_mass of its precision, exactly 0 for an atom without mass
    im = np.ones(n) if inv_mass is None else np.asarray(inv_mass).astype(dtype).astype(np.float64)
    m = np.where(im != 0.0, 1.0 / np.where(im != 0.0, im, 1.0), 0.0)
    tag = "%s n=%d %s: " % (what, n, np.dtype(dtype).name)
    _word(tag + "potential energy", ep, _np(st["energies"]))
    _word(tag + "virial", w, _np(st["virials"]))
    _word(tag + "kinetic energy", ek, 0.5 * m[:, None] * v * v, factor=8)
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    for c, (a, b) in enumerate(pairs):
        _word(tag + "W[%d]" % c, sums[c], vt[:, c])
        _word(tag + "K[%d]" % c, sums[6 + c], m * v[:, a] * v[:, b], factor=8)
    if inv_mass is not None and (im == 0.0).any():
        assert (v[im == 0.0] == 0.0).all()
    assert ek > 0.0 and sums[6] > 0.0
    if n > 1:
        assert ep != 0.0 and w != 0.0 and all(s != 0.0 for s in sums[:6])   # (sums of something)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", SIZES)
def test_totals_and_tensor_sums_are_the_sums_of_the_per_atom_values(emdee, dev, dtype, n):
    B = _box(emdee.synthetic, n)
    _check(emdee, dev, B, dtype, 1.0 / B["mass"], "masses")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_without_a_mass_array(emdee, dev, dtype):
    """no inv_mass: every mass is 1"""
    _check(emdee, dev, _box(emdee.synthetic, 257), dtype, None, "unit masses")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_atoms_without_mass_add_exactly_nothing_to_the_kinetic_words(emdee, dev, dtype):
    """five atoms with inv_mass = 0 at zero velocity, one of them the last slot's"""
    B = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in _box(emdee.synthetic, 256).items()}
    im = 1.0 / B["mass"]
    idx = [0, 63, 64, 200, 255]
    im[idx] = 0.0
    B["vel"][idx] = 0.0
    _check(emdee, dev, B, dtype, im, "massless")
