"""GPU test of every refusal of the twelve observable entries (include/emdee_hip.h: emdee_md_set_rdf / _rdf_sample / _rdf_read /
_rdf_reset, the same four of emdee_md_set_msd and of emdee_md_set_gk): status code and full message, against texts recorded from
the library as it was while each observable formed its refusals on its own (tests/golden/observable_refusal_texts.json).  The
situations are the ones tests/test_gpu_rdf.py, test_gpu_msd.py and test_gpu_gk.py provoke and check by substring; after every
refused set and sample the table in force is read and must be the one it was, sums and counters unchanged.

The box is the smallest fcc Lennard-Jones fluid the engine takes: 4 x 4 x 4 jittered cells, 256 atoms at the density of the other
tests' 864-atom fluid, side 6.84 >= 2 (rc + skin) = 5.6.  Float64: the texts do not depend on the engine's precision.

Recording (with EMDEE_HIP_LIB naming the library to record from):
    python -m tests.test_gpu_observable_refusals [out.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import shake_ref as hr
from .helpers import vsite_ref as vr
from .test_gpu_barostat import DT, _engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observable_refusal_texts.json")
CELLS, N = 4, 256
FIRST, MIDDLE, LAST = 0, 123, N - 1


def _box(E):
    pos, L = E.synthetic.fcc_positions(CELLS)
    return dict(pos=pos, vel=E.synthetic.velocities(N, temperature=1.4), L=float(L), atoms=bref.lj_atoms(N))


def _load(E, dev, md, S, n=N, scale=1.0):
    md.set_state_(E.cu(S["pos"][:n] * scale, dev), E.cu(S["vel"][:n], dev), E.cu(S["atoms"][:n], dev))


class Log:
    """the refusals of one group of situations, by key"""

    def __init__(self, E, group):
        self.E, self.group, self.out = E, group, {}

    def refused(self, key, code, call, *args, **kw):
        with pytest.raises(self.E.EmDeeError) as err:
            call(*args, **kw)
        key = "%s/%s" % (self.group, key)
        assert key not in self.out, key
        self.out[key] = [err.value.code, str(err.value)]
        print("%s: %s" % (key, self.out[key]))
        assert err.value.code == code, key


def _i32(dev, v):
    return None if v is None else torch.as_tensor(v).to(device=dev, dtype=torch.int32).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bad_at(good, where, value):
    bad = good.copy()
    bad[where] = value
    return bad


# ---------------------------------------------------------------- the radial distribution functions
def rdf_refusals(E, dev):
    log, S = Log(E, "rdf"), _box(E)
    L = S["L"]
    md = _engine(E, dev, S["pos"], S["vel"], L, S["atoms"])
    h = md._handle
    log.refused("no_table/sample", ERR_STATE, md.rdf_sample_)
    log.refused("no_table/reset", ERR_STATE, md.rdf_reset_)
    log.refused("no_table/read_null", ERR_STATE, E._lib.call, "emdee_md_rdf_read", h, None, None, None, None)
    md.set_rdf_(0.5 * L, 32)
    md.rdf_sample_()
    E._lib.call("emdee_md_rdf_read", h, None, None, None, None)          # every output NULL: nothing to refuse
    before = md.rdf()

    def intact(frames=1, times=1):
        now = md.rdf()
        return (np.array_equal(now["counts"], times * before["counts"]) and now["frames"] == frames and
                now["group_sizes"] == before["group_sizes"] and now["inv_volume_sum"] == frames * before["inv_volume_sum"])

    def raw(r_max, n_bins, n_groups, groups, molecules):
        g, m = _i32(dev, groups), _i32(dev, molecules)
        E._lib.call("emdee_md_set_rdf", h, float(r_max), n_bins, n_groups, _ptr(g), _ptr(m))

    two = np.arange(N) % 2
    for key, args in (("n_groups_0", (0.5 * L, 10, 0, None, None)), ("n_groups_9", (0.5 * L, 10, 9, np.arange(N) % 9, None)),
                      ("n_bins_negative", (0.5 * L, -1, 1, None, None)), ("counters", (0.5 * L, 2731, 2, two, None)),
                      ("r_max_nan", (float("nan"), 10, 1, None, None)), ("r_max_inf", (float("inf"), 10, 1, None, None)),
                      ("r_max_0", (0.0, 10, 1, None, None)), ("r_max_negative", (-1.0, 10, 1, None, None)),
                      ("r_max_above_half", (0.5 * L * 1.0001, 10, 1, None, None)), ("groups_null", (0.5 * L, 10, 2, None, None))):
        log.refused("set/" + key, ERR_INVALID, raw, *args)
        assert intact(), key
    for name, at in (("first", FIRST), ("middle", MIDDLE), ("last", LAST)):
        log.refused("set/group_high_" + name, ERR_INVALID, raw, 0.5 * L, 10, 2, _bad_at(two, at, 2), None)
        log.refused("set/group_low_" + name, ERR_INVALID, raw, 0.5 * L, 10, 2, _bad_at(two, at, -2), None)
        log.refused("set/molecule_low_" + name, ERR_INVALID, raw, 0.5 * L, 10, 1, None, _bad_at(np.arange(N) // 3, at, -2))
        log.refused("set/molecule_low_grouped_" + name, ERR_INVALID, raw, 0.5 * L, 10, 2, two, _bad_at(np.arange(N) // 3, at, -5))
        assert intact(), name
    md.rdf_sample_()                                                     # the table set before still samples
    assert intact(2, 2)
    md.scale_box_(0.99)
    log.refused("sample/box_shrunk", ERR_STATE, md.rdf_sample_)
    assert intact(2, 2)
    md.set_rdf_(0.49 * L, 32)
    md.rdf_sample_()
    before = md.rdf()
    _load(E, dev, md, S, N - 3, 0.99)
    log.refused("sample/atom_count", ERR_STATE, md.rdf_sample_)
    assert intact()
    md.rdf_reset_()                                                      # (a reset does not make the table fit)
    log.refused("sample/atom_count_after_reset", ERR_STATE, md.rdf_sample_)
    md.set_rdf_(0.49 * L, 32)
    md.rdf_sample_()
    assert md.rdf()["group_sizes"] == [N - 3] and md.rdf()["frames"] == 1
    md.set_rdf_(1.0, 0)
    log.refused("cleared/sample", ERR_STATE, md.rdf_sample_)
    log.refused("cleared/reset", ERR_STATE, md.rdf_reset_)
    log.refused("cleared/read_null", ERR_STATE, E._lib.call, "emdee_md_rdf_read", h, None, None, None, None)
    md.close()
    return log.out


# ---------------------------------------------------------------- the displacement and velocity correlations
def msd_refusals(E, dev):
    log, S = Log(E, "msd"), _box(E)
    md = _engine(E, dev, S["pos"], S["vel"], S["L"], S["atoms"])
    h = md._handle
    log.refused("no_table/sample", ERR_STATE, md.msd_sample_)
    log.refused("no_table/reset", ERR_STATE, md.msd_reset_)
    log.refused("no_table/read_null", ERR_STATE, E._lib.call, "emdee_md_msd_read", h, None, None, None, None)
    md.set_msd_(4, origin_every=2)
    md.msd_sample_()
    md.step_(5, DT)
    md.msd_sample_()
    E._lib.call("emdee_md_msd_read", h, None, None, None, None)
    before = md.msd()

    def intact(of=None):
        now, of = md.msd(), before if of is None else of
        return (now["sums"].tobytes() == of["sums"].tobytes() and now["samples"] == of["samples"] and
                np.array_equal(now["origins"], of["origins"]) and now["group_sizes"] == of["group_sizes"])

    def raw(what, n_groups, groups, n_lags, every):
        g = _i32(dev, groups)
        E._lib.call("emdee_md_set_msd", h, what, n_groups, _ptr(g), n_lags, every)

    two = np.arange(N) % 2
    for key, args in (("what_0", (0, 1, None, 4, 1)), ("what_4", (4, 1, None, 4, 1)), ("n_groups_0", (3, 0, None, 4, 1)),
                      ("n_groups_9", (3, 9, np.arange(N) % 9, 4, 1)), ("groups_null", (3, 2, None, 4, 1)),
                      ("n_lags_negative", (3, 1, None, -1, 1)), ("n_lags_4097", (3, 1, None, 4097, 64)),
                      ("origin_every_0", (3, 1, None, 4, 0)), ("origins_65", (3, 1, None, 65, 1))):
        log.refused("set/" + key, ERR_INVALID, raw, *args)
        assert intact(), key
    for name, at in (("first", FIRST), ("middle", MIDDLE), ("last", LAST)):
        log.refused("set/group_high_" + name, ERR_INVALID, raw, 3, 2, _bad_at(two, at, 2), 4, 1)
        log.refused("set/group_low_" + name, ERR_INVALID, raw, 3, 2, _bad_at(two, at, -2), 4, 1)
        assert intact(), name
    md.scale_box_(0.999)
    log.refused("sample/box_rescaled", ERR_STATE, md.msd_sample_)
    assert intact()
    md.msd_reset_()
    md.msd_sample_()
    assert md.msd()["samples"] == 1
    _load(E, dev, md, S, N, 0.999)
    after = md.msd()
    log.refused("sample/state_replaced", ERR_STATE, md.msd_sample_)
    assert intact(after)
    md.msd_reset_()
    md.msd_sample_()
    assert list(md.msd()["origins"]) == [1, 0, 0, 0]
    after = md.msd()
    _load(E, dev, md, S, N - 3, 0.999)
    log.refused("sample/atom_count", ERR_STATE, md.msd_sample_)
    assert intact(after)
    md.msd_reset_()
    log.refused("sample/atom_count_after_reset", ERR_STATE, md.msd_sample_)
    md.set_msd_(4, origin_every=2)
    md.msd_sample_()
    assert md.msd()["group_sizes"] == [N - 3]
    md.set_msd_(0)
    log.refused("cleared/sample", ERR_STATE, md.msd_sample_)
    log.refused("cleared/reset", ERR_STATE, md.msd_reset_)
    log.refused("cleared/read_null", ERR_STATE, E._lib.call, "emdee_md_msd_read", h, None, None, None, None)
    md.close()
    return log.out


# ---------------------------------------------------------------- the Green-Kubo observables
def gk_refusals(E, dev):
    log, S = Log(E, "gk"), _box(E)
    md = _engine(E, dev, S["pos"], S["vel"], S["L"], S["atoms"])
    h = md._handle
    log.refused("no_table/sample", ERR_STATE, md.gk_sample_)
    log.refused("no_table/reset", ERR_STATE, md.gk_reset_)
    log.refused("no_table/read_null", ERR_STATE, E._lib.call, "emdee_md_gk_read", h, None, None, None, None)
    md.set_green_kubo_(4)
    md.gk_sample_()
    md.step_(3, DT)
    md.gk_sample_()
    E._lib.call("emdee_md_gk_read", h, None, None, None, None)
    before = md.green_kubo()

    def intact(of=None):
        now, of = md.green_kubo(), before if of is None else of
        return (now["sums"].tobytes() == of["sums"].tobytes() and now["totals"].tobytes() == of["totals"].tobytes() and
                now["last"].tobytes() == of["last"].tobytes() and now["samples"] == of["samples"])

    raw = lambda what, n_lags: E._lib.call("emdee_md_set_gk", h, what, n_lags)
    for key, args in (("what_0", (0, 4)), ("what_4", (4, 4)), ("n_lags_negative", (3, -1)), ("n_lags_65537", (3, 65537)),
                      ("what_0_and_n_lags_negative", (0, -1))):
        log.refused("set/" + key, ERR_INVALID, raw, *args)
        assert intact(), key
    # every table that is not a pair term of the neighbour rows: the heat flux is refused at set and at sample
    bond = ([[0, 1]], [[10.0, 1.1]])
    attach = {
        "exclusions": (lambda: md.set_exclusions_([[0, 1]]), lambda: md.set_exclusions_(None)),
        "pairs14": (lambda: md.set_pairs14_([[0, 1]], 0.5), lambda: md.set_pairs14_(None, 1.0)),
        "bonded": (lambda: md.set_bonded_(E.HARMONIC_BOND, *bond), lambda: md.set_bonded_(E.HARMONIC_BOND, [], [])),
    }
    for name, (on, off) in attach.items():
        on()
        log.refused("sample/in_the_way_" + name, ERR_STATE, md.gk_sample_)
        log.refused("set/in_the_way_" + name, ERR_STATE, md.set_green_kubo_, 4)
        assert intact(), name
        off()
    md.set_exclusions_([[0, 1]])
    md.set_pairs14_([[2, 3]], 0.5)
    log.refused("sample/in_the_way_two_tables", ERR_STATE, md.gk_sample_)
    assert intact()
    md.set_exclusions_(None)
    md.set_pairs14_(None, 1.0)
    md.set_coulomb_(0.3 * (1.0 - 2.0 * (np.arange(N) % 2)), 1.0)
    md.set_ewald_(1.0, 4)
    log.refused("sample/in_the_way_ewald", ERR_STATE, md.gk_sample_)
    log.refused("set/in_the_way_ewald", ERR_STATE, md.set_green_kubo_, 4)
    md.set_pme_(1.0, 16, 4)
    log.refused("sample/in_the_way_pme", ERR_STATE, md.gk_sample_)
    log.refused("set/in_the_way_pme", ERR_STATE, md.set_green_kubo_, 4, stress=False)
    assert intact()
    md.set_pme_(0.0)
    md.set_coulomb_(None, 1.0)
    md.gk_sample_()                                                      # the table in force samples on
    assert md.green_kubo()["samples"] == 3
    before = md.green_kubo()
    md.scale_box_(0.999)
    log.refused("sample/box_rescaled", ERR_STATE, md.gk_sample_)
    assert intact()
    md.gk_reset_()
    md.gk_sample_()
    assert md.green_kubo()["samples"] == 1
    _load(E, dev, md, S, N, 0.999)
    after = md.green_kubo()
    log.refused("sample/state_replaced", ERR_STATE, md.gk_sample_)
    assert intact(after)
    md.gk_reset_()
    md.gk_sample_()
    assert list(md.green_kubo()["counts"]) == [1, 0, 0, 0]
    after = md.green_kubo()
    _load(E, dev, md, S, N - 3, 0.999)
    log.refused("sample/atom_count", ERR_STATE, md.gk_sample_)
    assert intact(after)
    md.gk_reset_()
    log.refused("sample/atom_count_after_reset", ERR_STATE, md.gk_sample_)
    # charges set for another atom count: the table fits the state, the charges do not
    _load(E, dev, md, S, N, 0.999)
    md.set_coulomb_(0.3 * (1.0 - 2.0 * (np.arange(N) % 2)), 1.0)
    _load(E, dev, md, S, N - 3, 0.999)
    md.set_green_kubo_(4)
    after = md.green_kubo()
    log.refused("sample/stale_charges", ERR_STATE, md.gk_sample_)
    assert intact(after)
    md.set_coulomb_(None, 1.0)
    md.gk_sample_()
    assert md.green_kubo()["samples"] == 1
    md.set_green_kubo_(0)
    log.refused("cleared/sample", ERR_STATE, md.gk_sample_)
    log.refused("cleared/reset", ERR_STATE, md.gk_reset_)
    log.refused("cleared/read_null", ERR_STATE, E._lib.call, "emdee_md_gk_read", h, None, None, None, None)
    md.close()
    return log.out


def gk_tables_refusals(E, dev):
    """an hbonds table refuses every mask, at set and -- attached later -- at sample; rigid four-site water refuses the heat flux
    with every table it holds named"""
    from .test_gpu_hbonds import _engine as _hbonds_engine
    from .test_gpu_vsites import _engine as _site_engine
    log = Log(E, "gk_tables")
    B = hr.mixed_box()
    md = _hbonds_engine(E, dev, B, hbonds=False)
    md.set_green_kubo_(3, heat=False)
    md.gk_sample_()
    after = md.green_kubo()
    md.set_hbonds_(B["clusters"], B["dist"])
    log.refused("sample/hbonds", ERR_STATE, md.gk_sample_)
    for name, stress, heat in (("stress", True, False), ("heat", False, True), ("both", True, True)):
        log.refused("set/hbonds_" + name, ERR_STATE, md.set_green_kubo_, 3, stress=stress, heat=heat)
    now = md.green_kubo()
    assert now["sums"].tobytes() == after["sums"].tobytes() and now["samples"] == 1
    md.set_hbonds_(None, None)
    md.gk_sample_()
    assert md.green_kubo()["samples"] == 2
    md.close()
    md = _site_engine(E, dev, vr.four_site_box())
    log.refused("set/four_site_water", ERR_STATE, md.set_green_kubo_, 3)
    md.set_green_kubo_(3, heat=False)
    md.gk_sample_()
    assert md.green_kubo()["samples"] == 1
    md.close()
    return log.out


# ---------------------------------------------------------------- engines that take no table
def engine_refusals(E, dev):
    from .test_gpu_dd_pairs import _build
    log, S = Log(E, "engines"), _box(E)
    L, model = S["L"], E.LennardJonesModel(bref.RC, bref.RS)
    setters = {"rdf": lambda md: md.set_rdf_(2.5, 50), "msd": lambda md: md.set_msd_(4), "gk": lambda md: md.set_green_kubo_(4)}
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (a decomposition needs two bricks of 2.8 + halo)
    pos = pos[np.argsort(gid)]
    n = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((n, 3)), E.lennard_jones_atoms(1.0, 1.0, n), float(lengths[0]))
    for kind, set_ in setters.items():
        log.refused("lent/" + kind, ERR_STATE, set_, dd.engine(0))
    dd.step_(2, DT)                                                                      # the decomposition is unharmed
    dd.close()
    g = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"][:-4], dev), L, model, E.cu(S["atoms"], dev), skin=bref.SKIN, n_ghost=4)
    for kind, set_ in setters.items():
        log.refused("ghosts/" + kind, ERR_STATE, set_, g)
    g.close()
    # before emdee_md_set_state, through the C ABI
    ctx, h = E.context_for(dev), C.c_void_p()
    three = lambda *v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", ctx.handle, three(0, 0, 0), three(L, L, L), (C.c_int32 * 3)(1, 1, 1), E._lib.model_c(model), bref.SKIN, 8,
                C.byref(h))
    log.refused("no_state/rdf", ERR_STATE, E._lib.call, "emdee_md_set_rdf", h, 2.5, 50, 1, None, None)
    log.refused("no_state/msd", ERR_STATE, E._lib.call, "emdee_md_set_msd", h, 3, 1, None, 4, 1)
    log.refused("no_state/gk", ERR_STATE, E._lib.call, "emdee_md_set_gk", h, 3, 4)
    # which refusal wins where two hold: the engine before the arguments (rdf, msd), the mask and the lags before the engine (gk)
    log.refused("no_state/rdf_n_groups_0", ERR_STATE, E._lib.call, "emdee_md_set_rdf", h, 2.5, 50, 0, None, None)
    log.refused("no_state/msd_what_0", ERR_STATE, E._lib.call, "emdee_md_set_msd", h, 0, 1, None, 4, 1)
    log.refused("no_state/gk_what_0", ERR_INVALID, E._lib.call, "emdee_md_set_gk", h, 0, 4)
    log.refused("no_state/gk_n_lags_negative", ERR_INVALID, E._lib.call, "emdee_md_set_gk", h, 3, -1)
    E._lib.call("emdee_md_set_rdf", h, 2.5, 0, 1, None, None)                            # clearing nothing is fine
    E._lib.call("emdee_md_set_msd", h, 3, 1, None, 0, 1)
    E._lib.call("emdee_md_set_gk", h, 3, 0)
    E._lib.call("emdee_md_destroy", h)
    o = E.VelocityVerlet(E.cu(S["pos"], dev), E.cu(S["vel"], dev), L, model, E.cu(S["atoms"], dev), skin=bref.SKIN, lo=[0.0] * 3,
                         lengths=[L] * 3, periodic=[1, 1, 0])
    log.refused("open_axis/rdf", ERR_STATE, o.set_rdf_, 2.5, 50)
    o.set_msd_(2)                                                                        # an open axis is fine for the other two
    o.set_green_kubo_(2)
    o.close()
    return log.out


GROUPS = {"rdf": rdf_refusals, "msd": msd_refusals, "gk": gk_refusals, "gk_tables": gk_tables_refusals, "engines": engine_refusals}


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_the_groups_and_nothing_else(recorded):
    assert {k.split("/", 1)[0] for k in recorded} == set(GROUPS)


@pytest.mark.parametrize("group", list(GROUPS))
def test_refusals_are_the_recorded_ones_and_leave_the_table_in_force(emdee, dev, recorded, group):
    got = GROUPS[group](emdee, dev)
    want = {k: v for k, v in recorded.items() if k.split("/", 1)[0] == group}
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key


if __name__ == "__main__":
    from __graft_entry__ import load_package
    E, device = load_package(), torch.device("cuda", 0)
    texts = {}
    for fn in GROUPS.values():
        texts.update(fn(E, device))
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as fh:
        json.dump(texts, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded %d refusals from %s" % (len(texts), E._lib.LIB_PATH))
