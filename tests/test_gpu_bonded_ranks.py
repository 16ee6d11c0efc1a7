"""GPU tests of the bonded terms beyond tests/test_gpu_bonded.py: the per-atom virial tensors and the twelve sums of
emdee_md_pressure_tensor at the load against the host yardsticks (the LJ tensor of tests/helpers/virial_tensor_ref.py plus the
bonded tensor of tests/helpers/bonded_ref.py), and a decomposition over two RCCL ranks: the same trajectory as the undivided
run, and a lost partner refused on both ranks, by the set call and by the next step, without either rank waiting for the other."""
import os

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import bonded_ref as br
from .helpers import virial_tensor_ref as vt
from .helpers.two_ranks import run_two_ranks
from .test_gpu_bonded import DT, RC, RS, _box, _chains, _md, _reference
from .test_gpu_dd_pairs import _lj14scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_STATE = -6


def _fields(atoms):
    a = np.asarray(atoms)
    return a["half_sigma"].astype(np.float32), a["twice_sqrt_eps"].astype(np.float32)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_chain_tensors_at_the_load_match_the_yardsticks(emdee, oracle, dtype):
    E = emdee
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14 = _lj14scale(E)
    if dtype == torch.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    md = _md(E, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14, terms=terms)
    t = md.virial_tensor().cpu().numpy().astype(np.float64)
    sums = np.array(md.tensor_sums())
    hs, te = _fields(atoms)
    t_lj, _ = vt.per_atom_tensor(pos, [L] * 3, [1, 1, 1], RC, RS, hs, te, excl=excl, p14=p14, lj14scale=s14, oracle=oracle)
    _, _, _, t_b = br.bonded(pos, L, terms)
    want = t_lj + t_b
    tol = 1e-6 if dtype == torch.float64 else 1e-4
    assert np.abs(t - want).max() <= tol * np.abs(want).max()
    # the box sums: the engine's own per-atom tensors summed, and the yardstick's
    f64 = dtype == torch.float64
    assert np.abs(sums[:6] - t.sum(axis=0)).max() <= (1e-12 if f64 else 1e-4) * np.abs(sums[:6]).max()
    assert np.abs(sums[:6] - want.sum(axis=0)).max() <= (1e-9 if f64 else 1e-3) * np.abs(want.sum(axis=0)).max()
    # the kinetic half: sum m v (x) v of the velocities the engine holds (m = 1)
    v = md.state()["velocities"].cpu().numpy().astype(np.float64)
    K = np.array([np.sum(v[:, a] * v[:, b]) for a, b in vt.COMPONENTS])
    assert np.abs(sums[6:] - K).max() <= 1e-9 * np.abs(K).max()
    # the trace of the box sum is the scalar virial of the same state
    (_, _, want_w), _ = _reference(oracle, pos, L, atoms, excl, p14, s14, terms)
    assert sums[:3].sum() == pytest.approx(want_w.sum(), rel=tol)
    md.close()


def test_two_rccl_ranks_match_the_undivided_run_and_refuse_together(emdee, tmp_path):
    E = emdee
    script = os.path.join(ROOT, "tests", "helpers", "bonded_rank.py")
    kids, outs = run_two_ranks(script, tmp_path, "emdee-bonded-rank-")
    for k, (out, err) in zip(kids, outs):
        assert k.returncode == 0, err[-800:]
        assert "REFUSED %d %d" % (ERR_STATE, ERR_STATE) in out, out + err[-800:]

    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    x, v, owner = np.zeros((N, 3)), np.zeros((N, 3)), np.full(N, -1)
    for r in range(2):
        d = np.load(os.path.join(tmp_path, "rank%d.npz" % r))
        assert (owner[d["gid"]] == -1).all()
        owner[d["gid"]] = r
        x[d["gid"]], v[d["gid"]] = d["x"], d["v"]
    assert (owner >= 0).all()
    terms, excl, p14 = _chains(N)
    tors = terms[2][1]
    assert (owner[tors] != owner[tors[:, :1]]).any()                 # some terms span the two ranks
    md = _md(E, pos, vel, E.lennard_jones_atoms(eps, sigma), L, excl=excl, p14=p14, s14=_lj14scale(E), terms=terms)
    md.step_(60, DT)
    st = md.state()
    dx = x - st["positions"].cpu().numpy()
    assert np.abs(dx - L * np.rint(dx / L)).max() < 1e-9
    assert np.abs(v - st["velocities"].cpu().numpy()).max() < 1e-8
    want = md.totals()
    for out, _ in outs:
        got = [float(t) for t in out.split("TOTALS")[1].split()[:3]]
        for a, b in zip(got, want):
            assert a == pytest.approx(b, rel=1e-9, abs=1e-9 * abs(want[0]))
    md.close()
