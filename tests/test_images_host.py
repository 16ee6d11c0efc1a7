"""The CPU-side conditions of tests/test_gpu_images.py, without a GPU: the dyadic boxes are what tests/helpers/image_cases.py says
(power-of-two sides, coordinates on the 2^-13 grid), every shifted input is a Float32 number, the 12-step runs rebuild at least
twice in free flight, the face sets keep their distance and band conditions, and the yardstick's trajectory carries every face
atom through its face in the direction the GPU test relies on."""
import numpy as np
import pytest

from .helpers import image_cases as ic
from .helpers import mask_cases as mc
from .helpers import ortho_ref as oref

DTYPES = [np.float64, np.float32]


def _box(E, name, dtype):
    if name == "settle_lj":
        return ic.settle_lj_box(E)
    return ic.ortho_box(E) if name == "ortho" else ic.dyadic_box(E, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", mc.FAMILIES + ["ortho"])
def test_dyadic_boxes_take_whole_box_shifts_exactly(emdee, family, dtype):
    box = _box(emdee, family, dtype)
    ic.assert_dyadic(box)
    ic.assert_rebuilds_twice(box)
    N = box["pos"].shape[0]
    for draw in ("uniform", "extremes"):
        k = ic.image_counts(N, draw)
        assert np.abs(k).max() == ic.KMAX and (k < 0).any() and (k > 0).any()
        x = ic.shifted(box, k)                                        # (asserts exactness in Float32)
        assert np.array_equal(x - k * np.asarray(box["lengths"]), box["pos"])
    if family == "ortho":
        assert ic.cells_per_side(box) == [3, 6, 12] and box["lo"] == [-1.0, 0.5, 2.0]
    else:
        src = mc.family_box(emdee, family, dtype)                     # the planner's facts stay: cells per side
        assert ic.cells_per_side(box)[0] == int(src["lengths"][0] // (src["rc"] + 0.3))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["uniform", "species3", "typed", "direct", "ortho", "settle_lj"])
def test_face_sets_keep_their_conditions(emdee, name, dtype):
    box = _box(emdee, name, dtype)
    if name == "typed":
        box = ic.sheared_box(box, 0.6)
        ic.assert_dyadic(box)
    fb, faces = ic.with_face_atoms(box, dtype)
    M = ic.cells_per_side(box)
    assert len(faces) == 3 * sum(m + 1 for m in M) and len({f[0] for f in faces}) == len(faces)
    for (a, d, c, side), (_, _, _, value) in zip(faces, ic.face_targets(box, dtype)):
        assert fb["pos"][a, d] == value
    ic.assert_face_conditions(fb, faces, box["scale"])
    pos2, n = ic.other_images(fb, faces, dtype, exact=name != "settle_lj")
    assert n >= (6 if name != "settle_lj" else len(faces))
    if name == "settle_lj" and dtype == np.float32:
        # the case of k_gather_sorted's comment: values just below lo + len round to lo + len itself
        hi = [box["lo"][d] + box["lengths"][d] for d in range(3)]
        assert sum(fb["pos"][a, d] == float(np.float32(hi[d])) for a, d, c, side in faces) >= 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_face_atoms_cross_their_faces_in_the_yardsticks_run(emdee, dtype):
    fb, faces = ic.with_face_atoms(ic.settle_lj_box(emdee), dtype)
    vel = ic.crossing_velocities(fb, faces, 0.002, dtype)
    lo, L, per = np.asarray(fb["lo"]), np.asarray(fb["lengths"]), fb["periodic"]
    force = lambda x: oref.total(oref.wrapped(x, lo, L, per), lo, L, per, fb["rc"], fb["rs"], fb["atoms"])["f"]
    xr, _ = oref.verlet(fb["pos"], vel, force, 20, 0.002)
    ic.assert_crossed(fb, faces, xr)
