"""The CPU-side conditions of the open-axes GPU tests (tests/test_gpu_open_axes.py, tests/test_gpu_open_axes_stages.py; systems
in tests/helpers/open_cases.py), checked without a GPU: a case whose conditions fail proves nothing on the device, so each is
pinned here and asserted again by the GPU test before it touches the device.

  * per open face at least eight atoms lie beyond it at the load, at 0.3, one and two cell widths and the guaranteed distance
    of the contract (include/emdee_hip.h, "Open axes"), with an outsider-outsider and an outsider-insider pair within rc;
  * no pair lies within test_gpu_orthorhombic.BAND of rc (twice that of rc + skin);
  * the yardstick evaluated with the open axes taken as periodic differs from the right one by at least 100 x the tolerance
    in use (the factor of test_chains_cross_every_face_parts_and_whole);
  * in the yardstick's trajectory atoms leave through every open face."""
import numpy as np
import pytest
import torch  # noqa: F401  (open_cases builds on the systems of the GPU modules, which skip at import where torch is missing: these
#                            conditions must fail loudly there, not skip with them)

from .helpers import open_cases as oc

TOL = oc.TOL                                             # tests/test_gpu_orthorhombic.py: fp64 1e-6, fp32 1e-4

DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(oc.CASES))
def test_pair_cases_keep_their_conditions(emdee, name, dtype):
    S = oc.pair_system(emdee.synthetic, name, dtype)
    atoms = emdee.lennard_jones_atoms(S["eps"], S["sigma"])
    assert 200 <= S["N"] <= 1600
    oc.assert_pair_conditions(S, atoms, oc.want(S, atoms), TOL[dtype])
    # the guaranteed distance is the one derived in DESIGN.md, restated: 12 cell widths (fp64), 32 - 6 cell widths (fp32)
    cw = (S["lengths"] / np.floor(S["lengths"] / (S["rc"] + S["skin"]))).max()
    assert oc.guaranteed_distance(S) == (12.0 * cw if dtype == np.float64 else 32.0 - 6.0 * cw)
    assert oc.guaranteed_distance(S) > 2.0 * cw


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(oc.CASES))
def test_atoms_leave_through_every_open_face_in_the_yardsticks_run(emdee, name, dtype):
    S = oc.pair_system(emdee.synthetic, name, dtype)
    atoms = emdee.lennard_jones_atoms(S["eps"], S["sigma"])
    _, _, crossed = oc.trajectory(name, S, atoms)
    assert sorted(crossed) == oc.faces(S) and len(crossed) == 2 * (3 - sum(S["periodic"]))
    for face, n in crossed.items():
        assert n >= 1, "no atom leaves through face %r" % (face,)


def test_moving_the_walls_out_does_not_change_the_yardstick(emdee):
    """what open_cases.want relies on: no pair term reads the length or the origin of an open axis"""
    from .helpers import ortho_ref as oref
    S = oc._system(emdee.synthetic, (5, 7, 9), np.float64, seed=oc.SEEDS["open1"], lo=True, periodic=(1, 0, 1))
    atoms = emdee.lennard_jones_atoms(S["eps"], S["sigma"])
    near = oref.total(S["pos"], S["lo"], S["lengths"], S["periodic"], S["rc"], S["rs"], atoms)
    far = oc.want(S, atoms)
    for key in "fewt":
        assert np.array_equal(near[key], far[key]), key


# ---------------------------------------------------------------- the stage boxes of tests/test_gpu_open_axes_stages.py
@pytest.mark.parametrize("kind", list(oc.KINDS))
@pytest.mark.parametrize("name", ["water", "tall", "mixed", "water4", "tall4"])
def test_stage_boxes_keep_their_conditions(name, kind):
    B = oc.stage_box(name, kind)
    assert len(B["pos"]) <= 1180 and len(B["mol"]) <= 150
    for dtype in DTYPES:
        oc.assert_stage_conditions(B, TOL[dtype], charged=name.endswith("4"))
    assert B["periodic"] == list(oc.KINDS[kind]) and np.all(B["lo"] != 0.0)
    # the molecules are whole along the open axes and on their constraints; on the periodic axes every atom is wrapped on its own
    u = oc.hr.unwrap(B["pos"], B["pairs"], B["lengths"], B["periodic"])
    i, j, d = B["pairs"][:, 0].astype(int), B["pairs"][:, 1].astype(int), B["pairs"][:, 2]
    assert np.abs(np.linalg.norm(u[i] - u[j], axis=1) / d - 1.0).max() <= 1e-12
    for a in range(3):
        if not B["periodic"][a]:
            assert np.array_equal(B["pos"][:, a], B["unwrapped"][:, a])
    if name.startswith("tall"):
        # two sites of every molecule more than half the open length apart: the minimum image along z would fold them
        assert B["lengths"][2] == oc.TALL_Z and oc.sr.RC + oc.sr.SKIN < oc.TALL_Z < 1.1 * (oc.sr.RC + oc.sr.SKIN)
        assert (oc.tall_spans(B) > 0.5).all() and B["geom"][:, 0].min() >= 1.6
        folded = oc.hr.unwrap(B["pos"], B["pairs"], B["lengths"], (1, 1, 1))
        assert np.abs(folded - u).max() > 0.9 * oc.TALL_Z
    if name == "tall4":
        folded = oc.vr.place(B["unwrapped"], B["vs_atoms"], B["vs_weights"], B["lengths"], (1, 1, 1))
        assert np.abs(folded - B["unwrapped"][B["sites"]]).max() > 0.1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_chain_slab_keeps_its_conditions(emdee, dtype):
    S = oc.chain_system(emdee, dtype)
    atoms = emdee.lennard_jones_atoms(S["eps"], S["sigma"])
    oc.assert_chain_conditions(S, atoms, oc.chain_parts(S, atoms), TOL[dtype])
    x, _ = oc.chain_trajectory(S, atoms, oc.CHAIN_STEPS)
    assert np.abs(x - S["pos"]).max() > 0.5 * S["skin"]                 # far enough for a rebuild


@pytest.mark.parametrize("kind", ["semi-z0", "aniso"])
def test_slab_coupling_references_keep_their_conditions(emdee, kind):
    R = oc.coupling_case(emdee.synthetic, kind)
    mus = oc.assert_coupling_conditions(R, TOL[np.float64])
    assert (np.abs(mus - 1.0)[:, :2] >= 1e-4).all() and (np.abs(mus - 1.0) <= 1e-2).all()
    assert (mus[:, 2] == 1.0).all() if kind == "semi-z0" else (np.abs(mus[:, 2] - 1.0) >= 1e-4).all()
    assert (R["lengths"][:2] >= 2.0 * (R["S"]["rc"] + R["S"]["skin"])).all()


def test_the_reference_minimiser_converges_on_the_clashing_droplet_in_the_recorded_count():
    from .helpers import fire_ref as fr
    from .test_gpu_minimize import TIGHT, WATER_FTOL
    B = oc.clashing_droplet()
    oc.assert_stage_conditions(B, TOL[np.float64], energy=True)

    def force(x):
        out = oc.stage_total(B, x)
        return out["f"], out["e"].sum()
    ref = fr.minimize(B["unwrapped"], force, B["mass"], 200, WATER_FTOL, pairs=B["pairs"], **TIGHT)
    assert ref["converged"] and ref["iterations"] == oc.DROPLET_ITERS and ref["energy"] < ref["energy0"]
