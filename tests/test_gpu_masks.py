"""GPU tests of the output mask (FORCES | ENERGIES | VIRIALS) on every kernel family and on every term behind a force pass.

A launch request carries the mask (csrc/nbsys.hpp Pass); the default brick variant and the direct kernels have an instance per
mask, the 1024-thread variant and the two-species typed kernels run their all-outputs instance for the masks 2 .. 6, and the
terms behind the pass (1-4 pairs, bonded terms, struck Ewald pairs, the reciprocal sum) switch on the mask at run time.  What is
pinned here, per family (tests/helpers/mask_cases.py: the plan text says which kernels a case runs) and in both precisions:

  1. the operator writes the selected caller arrays and no other, NULL ones included;
  2. emdee_md_forces(mask) on an uncharged engine writes the selected planes -- post terms included -- and leaves the force
     plane alone otherwise; emdee_md_get_state hands out the planes a pass with both ENERGIES and VIRIALS wrote and
     re-evaluates after any other; emdee_md_step re-evaluates a force plane the last pass left stale;
  3. a charged engine (reaction field, Ewald, PME) evaluates all three outputs for every mask but FORCES;
  4. the interior + boundary halves of a pass leave the bits of the whole pass, post terms added once;
  5. the tensor pass leaves the forces alone next to any mask.

References: the fp64 host yardsticks of tests/helpers (ortho_ref, ewald_ref, pme_ref) and the oracle, once per box.
Tolerances, relative to the largest entry of the reference: fp64 REL64 = 1e-6 of tests/test_gpu_parity.py for the uncharged
sections and 1e-9, the Ewald module's, for the charged ones; fp32 1e-4, what the Float32 operator and the Float32 engines are
held to elsewhere (a row of a few hundred pair terms, each good to 2^-24 relative, with the fast reciprocal of the pair loop)."""
import numpy as np
import pytest

from .helpers import mask_cases as mc
from .test_gpu_parity import REL64, rel_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT = 0.005
DTYPES = [np.float64, np.float32]
TOL = {np.float64: REL64, np.float32: 1e-4}
TOL_CHARGED = {np.float64: 1e-9, np.float32: 1e-4}
SENTINEL = 7.0
F = 1                                                          # EMDEE_FORCES


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _close(got, want, tol, what):
    err = rel_err(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
    print("%s: max error / max entry = %.3e (bound %.0e)" % (what, err, tol))
    assert err <= tol, what


def _engine(E, dev, box, dtype, monkeypatch, capfd, post="none", charges=None, eps_rf=np.inf, skin=0.3, check_plan=True):
    """the integrator on the box with the tables of `post` (and charges), its plan asserted from the debug text"""
    for k, v in box["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    md = E.VelocityVerlet(E.cu(box["pos"].astype(dtype), dev), E.cu(box["vel"].astype(dtype), dev), box["lengths"][0],
                          E.LennardJonesModel(box["rc"], box["rs"]), E.cu(box["atoms"], dev), skin=skin, lo=[0.0, 0.0, 0.0],
                          lengths=box["lengths"], periodic=box["periodic"])
    excl, p14, terms = mc.tables(box["pos"].shape[0], post)
    if excl is not None:
        md.set_exclusions_(excl)
        md.set_pairs14_(p14, mc.S14)
    for kind, a, p in terms or []:
        md.set_bonded_(kind, a, p)
    if charges is not None:
        md.set_coulomb_(charges, 1.0, eps_rf, mc.C14)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    if check_plan:
        box["plan"](err)
    return md, err


def _forces(md):
    """the force plane as it is: a forces-only read never re-evaluates"""
    return md.state(positions=False, velocities=False)["forces"]


def _energies_virials(md):
    st = md.state(positions=False, velocities=False, forces=False, energies=True, virials=True)
    return st["energies"], st["virials"]


def _passes(md):
    return md.kernel_time("lj_force_nbr")[1]


def _stale_planes(*engines):
    """Every plane of the engines made wrong for the positions they end at: a drift of DT v (no kick), an all-outputs pass there,
    and the drift back.  The atoms return to where they were to rounding (the velocities are untouched, so engines that go
    through this together stay bit-identical), and the planes hold the values of positions 0.01 away: a pass that then skips a
    plane it was asked for misses the reference by percents, not by rounding."""
    for md in engines:
        md.kick_drift_(DT, 0.0)
        md.forces_(7)
        md.kick_drift_(-DT, 0.0)


# ---------------------------------------------------------------- 1. the operator
def _call_operator(E, dev, tiles, outputs, xd, L, model, ad, mask):
    """emdee_compute_nonbonded / emdee_compute_nonbonded_tiles with the three output pointers as given (compute_nonbonded_ itself
    passes NULL for every output the mask leaves out)"""
    import ctypes as C
    lib, ctx = E._lib, E.context_for(dev)
    prec = 8 if xd.dtype == torch.float64 else 4
    N = xd.shape[0]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    head = [ctx.handle] + [ptr(t) for t in outputs] + [ptr(xd), float(L)]
    if isinstance(tiles, E.AllPairsTiles):
        lib.call("emdee_compute_nonbonded_tiles", *head, N, lib.model_c(model), ptr(ad), int(mask), tiles.mode, prec)
    else:
        lib.call("emdee_compute_nonbonded", *head, tiles._get(ctx, prec), lib.model_c(model), ptr(ad), int(mask), prec)


def _operator_masks(E, dev, tiles, box, dtype, ref, masks, what):
    N = box["pos"].shape[0]
    tdt = _tdt(dtype)
    xd, ad = E.cu(box["pos"].astype(dtype), dev), E.cu(box["atoms"], dev)
    model = E.LennardJonesModel(box["rc"], box["rs"])
    for with_null in (False, True):
        for mask in masks:
            out = [torch.full((N, 3), SENTINEL, dtype=tdt, device=dev), torch.full((N,), SENTINEL, dtype=tdt, device=dev),
                   torch.full((N,), SENTINEL, dtype=tdt, device=dev)]
            args = [t if (mask >> k) & 1 or not with_null else None for k, t in enumerate(out)]
            _call_operator(E, dev, tiles, args, xd, box["lengths"][0], model, ad, mask)
            for k, name in enumerate(("forces", "energies", "virials")):
                tag = "%s mask %d%s: %s" % (what, mask, " (NULL for the rest)" if with_null else "", name)
                if (mask >> k) & 1:
                    _close(out[k], ref[k], TOL[dtype], tag)
                else:
                    assert (out[k] == SENTINEL).all().item(), tag + " was written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", mc.FAMILIES + ["all_pairs"])
def test_operator_writes_the_selected_outputs_only(emdee, oracle, dev, capfd, monkeypatch, family, dtype):
    E = emdee
    box = mc.family_box(E, "uniform" if family == "all_pairs" else family, dtype)
    N = box["pos"].shape[0]
    for k, v in box["env"].items():
        monkeypatch.setenv(k, v)
    if family.startswith("typed") and dtype == np.float32:
        # (Float32 operator calls otherwise run the reference's Float32 arithmetic, which the general-species kernels carry)
        monkeypatch.setenv("EMDEE_F32_FAST", "1")
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    if family == "all_pairs":
        tiles = E.nonbonded_computation_tiles(N, all_pairs=True, mode=E.CUTOFF)
    else:
        tiles = E.nonbonded_computation_tiles(N)
    _operator_masks(E, dev, tiles, box, dtype, mc.reference(oracle, box), range(1, 8), family)
    torch.cuda.synchronize()
    if family != "all_pairs":
        box["plan"](capfd.readouterr().err)
    if family.startswith("typed") or family == "all_pairs":           # (tables take a two-species box off the typed kernels; all pairs have none)
        if family != "all_pairs":
            tiles.close()
        return
    excl, p14, _ = mc.tables(N, "tables")
    tiles.set_exclusions_(excl)
    tiles.set_pairs14_(p14, mc.S14)
    _operator_masks(E, dev, tiles, box, dtype, mc.reference(oracle, box, "tables"), (2, 4, 6), family + " with tables")
    tiles.close()


# ---------------------------------------------------------------- 2. the uncharged engine
def _posts(family):
    return ["none"] if family.startswith("typed") else ["none", "tables", "bonded"]


CASES_2 = [(f, p) for f in mc.FAMILIES for p in _posts(f)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,post", CASES_2)
def test_engine_pass_writes_the_selected_planes_and_get_state_knows_which(emdee, oracle, dev, capfd, monkeypatch, family, post, dtype):
    E = emdee
    box = mc.family_box(E, family, dtype)
    md, _ = _engine(E, dev, box, dtype, monkeypatch, capfd, post)
    ref = mc.reference(oracle, box, post)
    tol = TOL[dtype]
    md.profile_(True)
    for m in range(1, 8):
        what = "%s/%s mask %d" % (family, post, m)
        # (a) the force plane
        _stale_planes(md)
        md.forces_(F)
        f1 = _forces(md)
        md.forces_(m)
        fm = _forces(md)
        if m & F:
            _close(fm, ref[0], tol, what + ": forces")
        else:
            assert torch.equal(fm, f1), what + ": the force plane was rewritten"
        # (b) energies and virials; the pass's own planes where it wrote both
        before = _passes(md)
        e, w = _energies_virials(md)
        after = _passes(md)
        _close(e, ref[1], tol, what + ": energies")
        _close(w, ref[2], tol, what + ": virials")
        assert after - before == (0 if m in (6, 7) else 1), "%s: %d passes behind get_state" % (what, after - before)
        _close(_forces(md), ref[0], tol, what + ": forces behind get_state")   # (f1, the pass's, or the re-evaluation's)
    md.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,post", CASES_2)
def test_step_re_evaluates_a_force_plane_the_last_pass_left_stale(emdee, dev, capfd, monkeypatch, family, post, dtype):
    """forces(1), kick + drift, forces(m) without FORCES, step(3): the state of a twin that called forces(1) there, bit for bit.
    (No emdee_md_kick between forces(m) and the steps: the kick reads the force plane as it is, and under the header's rule that
    plane is the one from before the drift -- a caller who kicks there has asked for stale forces.  emdee_md_step must not.)"""
    E = emdee
    box = mc.family_box(E, family, dtype)
    md, _ = _engine(E, dev, box, dtype, monkeypatch, capfd, post)
    twin, _ = _engine(E, dev, box, dtype, monkeypatch, capfd, post)
    for m in (2, 4, 6):
        for eng, mask in ((md, m), (twin, F)):
            eng.forces_(F)
            eng.kick_drift_(DT, 0.5)
            eng.forces_(mask)
            eng.step_(3, DT)
        a, b = md.state(), twin.state()
        for k in ("positions", "velocities", "forces"):
            assert torch.equal(a[k], b[k]), "%s/%s mask %d: %s differ from the twin's" % (family, post, m, k)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 3. charged engines
def _alternating(N, q=0.5):
    return q * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)


def _charged_masks(md, twin, ref, tol, what):
    """md runs forces(m); the twin, bit-identical before every pass, the all-outputs pass (the force-only pass for m = 1)"""
    for m in range(1, 8):
        _stale_planes(md, twin)
        md.forces_(m)
        twin.forces_(F if m == F else 7)
        got = (_forces(md),) + _energies_virials(md)                   # (forces first: the read of e and w may re-evaluate)
        want = (_forces(twin),) + (_energies_virials(twin) if m != F else ())
        for g, r, name in zip(got, ref, ("forces", "energies", "virials")):
            _close(g, r, tol, "%s mask %d: %s" % (what, m, name))
        for g, a, name in zip(got, want, ("forces", "energies", "virials")):
            assert torch.equal(g, a), "%s mask %d: %s are not those of the %s pass" % (what, m, name, "force-only" if m == F else "all-outputs")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chains", [False, True])
@pytest.mark.parametrize("family", ["species3", "long_rows"])
def test_reaction_field_engine_evaluates_all_three_outputs(emdee, oracle, dev, capfd, monkeypatch, family, chains, dtype):
    E = emdee
    box = mc.family_box(E, family, dtype)
    N = box["pos"].shape[0]
    q = np.tile(mc.CHAIN_CHARGES, N // 4) if chains else _alternating(N)
    post = "bonded" if chains else "none"
    # (Float32: a pair within rounding of rc may fall on either side of it; at eps_rf = inf the force is continuous there)
    eps_rf = 6.0 if dtype == np.float64 else np.inf
    md, err = _engine(E, dev, box, dtype, monkeypatch, capfd, post, charges=q, eps_rf=eps_rf)
    twin, _ = _engine(E, dev, box, dtype, monkeypatch, capfd, post, charges=q, eps_rf=eps_rf)
    plans = [l for l in err.splitlines() if l.startswith("emdee plan: charged engine")]
    assert plans and ("brick kernels, variant %d" % (8 if family == "long_rows" else 0)) in plans[-1], plans
    _charged_masks(md, twin, mc.reference(oracle, box, post, q, eps_rf), TOL_CHARGED[dtype], "%s %s" % (family, post))
    md.close()
    twin.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chains", [False, True])
@pytest.mark.parametrize("method", ["ewald", "pme"])
def test_ewald_engine_evaluates_all_three_outputs(emdee, oracle, dev, capfd, monkeypatch, method, chains, dtype):
    """(The chain tables go on the chain box of the Ewald and PME chain tests, with its alpha, kmax and grid: consecutive atoms of
    the 300-charge box are not neighbours, and a struck pair beyond the list radius is refused.)"""
    E = emdee
    box = mc.ewald_box(E, chains)
    box.update(vel=E.synthetic.velocities(box["pos"].shape[0]), env={}, plan=None)
    engines = []
    for _ in range(2):
        md, _ = _engine(E, dev, box, dtype, monkeypatch, capfd, box["post"], charges=box["q"], eps_rf=5.0, skin=box["skin"], check_plan=False)
        capfd.readouterr()
        if method == "ewald":
            md.set_ewald_(box["alpha"], box["kmax"])
        else:
            md.set_pme_(box["alpha"], box["grid"], 4)
        plans = [l for l in capfd.readouterr().err.splitlines() if l.startswith("emdee plan: charged engine")]
        assert plans and "brick kernels, variant 0" in plans[-1], plans
        engines.append(md)
    _charged_masks(engines[0], engines[1], mc.ewald_reference(oracle, box, method), TOL_CHARGED[dtype], "%s %s" % (method, box["key"]))
    for md in engines:
        md.close()


# ---------------------------------------------------------------- 4. the two halves of a pass
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,post", [("uniform", "none"), ("species3", "tables"), ("orthorhombic", "none")])
def test_interior_and_boundary_halves_leave_the_bits_of_the_whole_pass(emdee, dev, capfd, monkeypatch, family, post, dtype):
    E = emdee
    box = mc.family_box(E, family, dtype)
    whole, _ = _engine(E, dev, box, dtype, monkeypatch, capfd, post)
    halves, _ = _engine(E, dev, box, dtype, monkeypatch, capfd, post)

    def planes(md, m):
        out = {}
        if m & F:
            out["forces"] = _forces(md)
        if m & 6 == 6:
            out["energies"], out["virials"] = _energies_virials(md)    # (both current: no re-evaluation)
        return out

    for m in (1, 6, 7):
        for md in (whole, halves):
            md.forces_(7)
        old = planes(whole, 7)
        for md in (whole, halves):
            md.kick_drift_(DT, 0.5)                                    # new positions: stale planes would show
        whole.forces_(m, 0)
        halves.forces_(m, 1)
        halves.forces_(m, 2)
        a, b = planes(whole, m), planes(halves, m)
        for k in a:
            assert not torch.equal(a[k], old[k]), "%s mask %d: %s did not change with the positions" % (family, m, k)
            assert torch.equal(a[k], b[k]), "%s mask %d: %s of the two halves differ from the whole pass's" % (family, m, k)
        for md in (whole, halves):
            md.forces_(F)                                              # (the next round kicks with current forces on both)
    whole.close()
    halves.close()


# ---------------------------------------------------------------- 5. the tensor pass next to masks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["uniform", "typed"])
def test_tensor_pass_leaves_the_forces_alone_next_to_any_mask(emdee, oracle, dev, capfd, monkeypatch, family, dtype):
    E = emdee
    box = mc.family_box(E, family, dtype)
    md, _ = _engine(E, dev, box, dtype, monkeypatch, capfd)
    ref = mc.reference(oracle, box)
    tol = TOL[dtype]
    md.profile_(True)
    for m in (1, 6):
        _stale_planes(md)
        md.forces_(F)
        md.forces_(m)
        before = _forces(md)
        n0 = _passes(md)
        t = md.virial_tensor()
        assert _passes(md) - n0 == 1, "mask %d: the tensor pass did not run" % m
        assert torch.equal(_forces(md), before), "mask %d: the tensor pass touched the forces" % m
        _close(before, ref[0], tol, "mask %d: forces" % m)
        n0 = _passes(md)
        e, w = _energies_virials(md)
        assert _passes(md) == n0, "mask %d: get_state re-evaluated behind a tensor pass" % m
        _close(e, ref[1], tol, "mask %d: energies" % m)
        _close(w, ref[2], tol, "mask %d: virials" % m)
        _close(t[:, 0] + t[:, 1] + t[:, 2], ref[2], tol, "mask %d: trace of the tensors" % m)
    md.close()
