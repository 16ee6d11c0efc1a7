"""Host tests of the per-atom virial tensor's yardstick (tests/helpers/virial_tensor_ref.py) and of the Python bindings'
argument checks (emdee_compute_virial_tensor, emdee_md_virial_tensor): no GPU needed."""
import os

import numpy as np
import pytest

from .conftest import GOLDEN, read_xyz
from .helpers import virial_tensor_ref as vt

torch = pytest.importorskip("torch")


def _atoms(eps, sigma, N):
    eps, sigma = np.broadcast_to(eps, (N,)), np.broadcast_to(sigma, (N,))
    return (0.5 * sigma).astype(np.float32), (2.0 * np.sqrt(eps)).astype(np.float32)


def _boxes(emdee_synthetic, golden):
    syn = emdee_synthetic
    x = read_xyz(os.path.join(GOLDEN, "lj_sample.xyz")).astype(np.float32).astype(np.float64)
    yield "lj_sample", x, 10.0, 3.0, 2.5, _atoms(1.0, 1.0, x.shape[0]), golden["lj_sample_expected"]["virials_cutoff"]
    p, L = syn.fcc_positions(6)
    g = golden["fcc864_expected"]
    assert float(g["L"]) == L
    yield "fcc864", p, L, 2.5, 2.0, _atoms(1.0, 1.0, p.shape[0]), g["virials"]
    p, L = syn.fcc_positions(5)
    g = golden["mix500_expected"]
    eps, sigma = syn.mixture_parameters(g["types"])
    yield "mix500", p, L, 3.5, 3.0, _atoms(eps, sigma, p.shape[0]), g["virials"]


def test_trace_of_the_yardstick_is_the_pinned_per_atom_virial(oracle, emdee_synthetic, golden):
    for name, x, L, rc, rs, (hs, te), want in _boxes(emdee_synthetic, golden):
        t, w = vt.per_atom_tensor(x, [L] * 3, [1, 1, 1], rc, rs, hs, te, oracle=oracle)
        scale = np.abs(want).max()
        assert np.abs(vt.trace(t) - want).max() <= 1e-12 * scale, name
        assert np.abs(w - want).max() <= 1e-12 * scale, name
        # the off-diagonal part is not zero (the tensor carries more than the trace), and the brute-force pairs agree
        assert np.abs(t[:, 3:]).max() > 1e-3 * np.abs(t[:, :3]).max(), name
        if x.shape[0] <= 900:
            tb, _ = vt.per_atom_tensor(x, [L] * 3, [1, 1, 1], rc, rs, hs, te, oracle=None)
            assert np.abs(tb - t).max() <= 1e-13 * np.abs(t).max(), name


def test_numpy_pair_function_matches_the_oracle(oracle):
    rng = np.random.default_rng(11)
    for rc, rs in ((2.5, 2.0), (3.5, 3.0), (3.0, 2.5)):
        om = oracle.model(rc, rs)
        r2 = rng.uniform(0.6, (rc + 0.2) ** 2, 400)
        r2[:4] = [rs * rs, rc * rc, np.nextafter(rc * rc, 0.0), 0.5 * (rs * rs + rc * rc)]
        hs = rng.uniform(0.4, 0.6, (400, 2)).astype(np.float32)
        te = rng.uniform(1.0, 2.4, (400, 2)).astype(np.float32)
        E, W = vt.pair_energy_virial(r2, rc, rs, hs[:, 0], te[:, 0], hs[:, 1], te[:, 1])
        for k in range(r2.shape[0]):
            e0, w0 = oracle.interaction(r2[k], om, (hs[k, 0], te[k, 0]), (hs[k, 1], te[k, 1]), mode=oracle.CUTOFF)
            assert E[k] == pytest.approx(e0, rel=1e-13, abs=1e-13)
            assert W[k] == pytest.approx(w0, rel=1e-13, abs=1e-13)


def test_exclusions_and_scaled_14_pairs_in_the_yardstick(oracle, emdee_synthetic):
    """Excluded pairs contribute nothing; 1-4 pairs contribute lj14scale times their term -- checked against the
    tensor of the named pairs alone."""
    p, L = emdee_synthetic.fcc_positions(4)
    N = p.shape[0]
    hs, te = _atoms(1.0, 1.0, N)
    mol = np.arange(N).reshape(-1, 4)
    excl, p14 = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]]]), mol[:, [0, 3]]
    full, _ = vt.per_atom_tensor(p, [L] * 3, [1, 1, 1], 2.5, 2.0, hs, te, oracle=oracle)
    got, _ = vt.per_atom_tensor(p, [L] * 3, [1, 1, 1], 2.5, 2.0, hs, te, excl=excl, p14=p14, lj14scale=0.5, oracle=oracle)
    named = np.zeros_like(full)
    for pairs, s in ((excl, 1.0), (p14, 0.5)):
        for i, j in pairs:
            d = p[i] - p[j]
            d -= L * np.rint(d / L)
            r2 = float(d @ d)
            _, W = oracle.interaction(r2, oracle.model(2.5, 2.0), (hs[i], te[i]), (hs[j], te[j]), mode=oracle.CUTOFF)
            h = np.array([0.5 * s * W / r2 * d[a] * d[b] for a, b in vt.COMPONENTS])
            named[i] += h; named[j] += h
    assert np.abs(named).max() > 1e-3 * np.abs(full).max()
    assert np.abs(got - (full - named)).max() <= 1e-12 * np.abs(full).max()


def test_non_periodic_axis_takes_no_image(emdee_synthetic):
    """A pair across a non-periodic face is far apart; across a periodic face it is close."""
    x = np.array([[0.2, 5.0, 5.0], [9.6, 5.0, 5.0], [5.0, 5.0, 0.2], [5.0, 5.0, 11.6]])
    hs, te = _atoms(1.0, 1.0, 4)
    t, _ = vt.per_atom_tensor(x, [9.8, 10.0, 12.0], [1, 1, 0], 2.5, 2.0, hs, te)
    assert t[0, 0] != 0.0 and t[1, 0] == t[0, 0] and np.all(t[0, 1:] == 0.0)     # the x pair, through the periodic face
    assert np.all(t[2:] == 0.0)                                                   # the z pair stays 11.4 apart


def _package():
    from __graft_entry__ import load_package
    try:
        return load_package()
    except OSError as e:                                  # (the library is built by __graft_entry__.build())
        pytest.skip("libemdee_hip.so not built: %s" % e)


def test_bindings_reject_bad_tensor_arguments_before_any_device_call():
    E = _package()
    N = 8
    x = torch.zeros((N, 3), dtype=torch.float64)
    atoms = torch.zeros((N, 2), dtype=torch.float32)
    tiles = E.nonbonded_computation_tiles(N)
    model = E.LennardJonesModel(2.5, 2.0)
    with pytest.raises(ValueError, match="all-pairs"):
        E.compute_virial_tensor_(torch.zeros((N, 6), dtype=torch.float64), x, 4.0, E.nonbonded_computation_tiles(N, all_pairs=True), model, atoms)
    with pytest.raises(ValueError, match="shape"):
        E.compute_virial_tensor_(torch.zeros((N, 3), dtype=torch.float64), x, 4.0, tiles, model, atoms)
    with pytest.raises(ValueError, match="shape"):
        E.compute_virial_tensor_(torch.zeros((6, N), dtype=torch.float64), x, 4.0, tiles, model, atoms)
    with pytest.raises(TypeError, match="dtype"):
        E.compute_virial_tensor_(torch.zeros((N, 6), dtype=torch.float32), x, 4.0, tiles, model, atoms)
    with pytest.raises(ValueError, match="tiles were built"):
        E.compute_virial_tensor_(torch.zeros((N + 1, 6), dtype=torch.float64), torch.zeros((N + 1, 3), dtype=torch.float64), 4.0,
                                 tiles, model, torch.zeros((N + 1, 2), dtype=torch.float32))
    with pytest.raises(TypeError, match="GPU"):
        E.compute_virial_tensor_(torch.zeros((N, 6), dtype=torch.float64), x, 4.0, tiles, model, atoms)
    assert tiles._handle is None                          # nothing reached the library
    # the integrator's binding checks its output the same way (an object with no engine behind it: a call would fail)
    md = E.VelocityVerlet.__new__(E.VelocityVerlet)
    md.n_owned, md.dtype, md._handle = N, torch.float64, None
    with pytest.raises(ValueError, match="shape"):
        md.virial_tensor(out=torch.zeros((N, 3), dtype=torch.float64))
    with pytest.raises(TypeError, match="dtype"):
        md.virial_tensor(out=torch.zeros((N, 6), dtype=torch.float32))


def test_pressure_tensor_dict_is_symmetric_and_traces_to_the_scalar_pressure():
    E = _package()
    from importlib import import_module
    verlet = import_module(E.__name__ + ".verlet")
    sums = [1.0, 2.0, 3.0, 0.1, 0.2, 0.3, 4.0, 5.0, 6.0, 0.4, 0.5, 0.6]
    d = verlet.pressure_tensor_dict(sums, 10.0)
    assert np.array_equal(d["virial"], d["virial"].T) and np.array_equal(d["kinetic"], d["kinetic"].T)
    assert d["virial"][0, 1] == 0.1 and d["virial"][0, 2] == 0.2 and d["virial"][1, 2] == 0.3
    assert np.trace(d["pressure"]) / 3 == pytest.approx((2.0 * 7.5 + 6.0) / 30.0, rel=1e-15)
