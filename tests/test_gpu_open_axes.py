"""GPU tests of the pair path on boxes with open axes whose atoms lie BEYOND the open faces, at the load and after steps
(include/emdee_hip.h and DESIGN.md, "Open axes").  The other GPU modules keep every atom inside the walls of an open axis; an
atom beyond one takes its own route: voxel() clamps it into the edge cell, wrap_into_box() returns no image count, an fp32
cell-relative record leaves [0, width) for good, and the brick build's fp32 pre-test sees a brick-relative coordinate above
the cmax its margin was derived for.

Systems and their CPU-side conditions: tests/helpers/open_cases.py (pinned without a GPU by tests/test_open_axes_host.py and
asserted again here before the device is touched).  Yardstick: tests/helpers/ortho_ref.py.  Tolerances are those of
tests/test_gpu_orthorhombic.py, named where used: TOL (fp64 1e-6, fp32 1e-4 of the largest entry), X64 / X32 for trajectories
against the numpy integrator, and one fp32 ulp below 64 (2^-18, the figure X32 is derived from) for positions handed back."""
import numpy as np
import pytest

from .helpers import open_cases as oc
from .helpers import ortho_ref as oref
from .test_gpu_bonded import _outputs
from .test_gpu_orthorhombic import DT, TOL, X32, X64, _check_load, _check_rows, _engine, _plan_bricks, _rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ULP64 = 2.0 ** -18                  # one fp32 ulp of a coordinate below 64 (test_gpu_orthorhombic: the comment above X32)


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _prepared(E, name, dtype):
    S = oc.pair_system(E.synthetic, name, dtype)
    atoms = E.lennard_jones_atoms(S["eps"], S["sigma"])
    right = oc.want(S, atoms)
    oc.assert_pair_conditions(S, atoms, right, TOL[dtype])
    return S, atoms, right


def _positions_come_back(md, S, what):
    """emdee_md_get_state hands an atom beyond an open face back where it is: no image count, no clamp into the box"""
    x = md.state(velocities=False, forces=False)["positions"].cpu().numpy().astype(np.float64)
    for d in range(3):
        if S["periodic"][d]:
            continue
        err = np.abs(x[:, d] - S["pos"][:, d]).max()
        print("%s: open axis %d comes back within %.3e" % (what, d, err))
        if S["dtype"] == np.float64:
            assert np.array_equal(x[:, d], S["pos"][:, d]), (what, d, err)
        else:
            assert np.abs(S["pos"]).max() < 64.0 and err <= ULP64, (what, d, err)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("path", ["brick", "direct"])
@pytest.mark.parametrize("name", list(oc.CASES))
def test_load_with_atoms_beyond_open_faces(emdee, dev, capfd, monkeypatch, name, path, dtype):
    """Forces, energies, virials and tensors against ortho_ref (TOL), the neighbour rows against the brute-force set on the
    brick path, and the positions handed back."""
    E = emdee
    S, atoms, right = _prepared(E, name, dtype)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    capfd.readouterr()
    md = _engine(E, S, atoms, dev)
    got = _outputs(md)
    err = capfd.readouterr().err
    if path == "direct":
        assert "emdee plan: bricks" not in err, err[-400:]
    else:
        print(_plan_bricks(err)[1])
    _check_load(got, right, TOL[dtype], "%s %s" % (name, path))
    ep, _, vir = md.totals()
    assert ep == pytest.approx(right["e"].sum(), rel=TOL[dtype])
    assert vir == pytest.approx(right["w"].sum(), rel=TOL[dtype], abs=TOL[dtype] * np.abs(right["w"]).sum())
    if path == "brick":
        nbr = oc.neighbour_rows(S)
        assert md.nbr_stats()["listed"] == sum(len(r) for r in nbr.values())
        _check_rows(_rows(md), nbr, "%s at the load" % name)
    _positions_come_back(md, S, "%s %s" % (name, path))
    md.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("path", ["brick", "direct"])
@pytest.mark.parametrize("name", list(oc.CASES))
def test_trajectory_with_atoms_leaving_through_open_faces(emdee, dev, monkeypatch, name, path, dtype):
    """open_cases.NSTEPS steps against ortho_ref.verlet as test_gpu_orthorhombic._run_case compares them (X64 / X32 in
    position, ten times that in velocity), with at least two rebuilds after the load; the yardstick's run counts the atoms that
    leave through each open face."""
    E = emdee
    S, atoms, right = _prepared(E, name, dtype)
    xr, vr, crossed = oc.trajectory(name, S, atoms)
    for face in oc.faces(S):
        assert crossed[face] >= 1, "no atom leaves through face %r" % (face,)
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    md = _engine(E, S, atoms, dev)
    md.step_(oc.NSTEPS, DT)
    st = md.state()
    x, v = st["positions"].cpu().numpy().astype(np.float64), st["velocities"].cpu().numpy().astype(np.float64)
    builds = md.nbr_stats()["builds"]
    assert builds >= 3, builds                                       # the load and at least two automatic rebuilds
    dx = np.abs(oref.image_difference(x, xr, S["lengths"], S["periodic"])).max()
    print("%s %s: %d builds, max |dx| %.3e, max |dv| %.3e, crossings %r" % (name, path, builds, dx, np.abs(v - vr).max(), crossed))
    lim = X64 if dtype == np.float64 else X32
    assert dx < lim and np.abs(v - vr).max() < 10 * lim
    for d in range(3):                                               # open axes: no whole box length may have been taken out
        if not S["periodic"][d]:
            assert np.abs(x[:, d] - xr[:, d]).max() < lim, d
    if path == "brick" and dtype == np.float64:                      # the list of the CURRENT positions, outsiders of the run included
        md.rebuild_()
        x = md.state()["positions"].cpu().numpy()
        assert oref.nearest_to_radius(x, S["lengths"], S["periodic"], S["rc"] + S["skin"]) > 1e-12
        _check_rows(_rows(md), oc.neighbour_rows(S, x), "%s after %d steps" % (name, oc.NSTEPS))
    md.close()
