"""GPU test of the reaction-field Coulomb terms across processes: a decomposition over two RCCL ranks on one device
(tests/helpers/coulomb_rank.py) with the per-process charge table of every rank.  The same trajectory as the undivided run, and
a charge table that misses the gid one rank holds refused on both ranks, by the set call and by the next step, without either
rank waiting for the other."""
import os

import numpy as np
import pytest

from .conftest import ROOT
from .helpers.coulomb_rank import CHARGES
from .helpers.two_ranks import run_two_ranks
from .test_gpu_bonded import DT, _box, _chains, _md
from .test_gpu_dd_pairs import _lj14scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_STATE = -6


def test_two_rccl_ranks_with_charges_match_the_undivided_run_and_refuse_an_unknown_gid_together(emdee, tmp_path):
    E = emdee
    script = os.path.join(ROOT, "tests", "helpers", "coulomb_rank.py")
    kids, outs = run_two_ranks(script, tmp_path, "emdee-coulomb-rank-")
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
    md.set_coulomb_(CHARGES(N), 1.0, 5.0, 0.8333)
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
