"""GPU test of the refusals an attached table draws from the entries that consult it (include/emdee_hip.h: emdee_md_set_rigid3,
emdee_md_set_hbonds, emdee_md_set_vsites): status code and full message, against texts recorded from the library as it was
before MdImpl::require_ready and require_fitting took over the forming of them (tests/golden/refusal_texts.json).

Per table and entry: the refusal after set_state with another atom count; the refusal of set_state with the same count and a
state that does not fit the table, and of the entry after it; and the recovery -- the table set again, one step.

The boxes are the smallest the engine takes: 8 three-site waters of settle_ref's geometry (24 atoms; as rigid molecules, or as
hbonds clusters of an apex and two satellites) or the same with a fourth, massless site each (32 atoms, the sites after the
waters) in a cube of side 6.0 -- 2 (rc + skin) = 5.8 is the least a periodic side may be.  Float64, no Lennard-Jones forces
(twice_sqrt_eps = 0), no exclusions and no charges (they would refuse the smaller state themselves): the rules of the table
alone.

Recording (with EMDEE_HIP_LIB naming the library to record from):
    python -m tests.test_gpu_refusal_texts [out.json]"""
import json
import os
import sys

import numpy as np
import pytest

from .helpers import settle_ref as sr
from .helpers import vsite_ref as vr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_STATE = -6
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_texts.json")
N_MOL, SIDE, DT = 8, 6.0, sr.DT
LENGTHS, LO = np.full(3, SIDE), np.zeros(3)
ENTRIES = {
    "emdee_md_step": lambda md: md.step_(1, DT),
    "emdee_md_minimize": lambda md: md.minimize_(1, 0.0),
    "emdee_md_scale_box": lambda md: md.scale_box_(1.001),
    "emdee_md_molecular_pressure_tensor": lambda md: md.molecular_tensor_sums(),
}
CASES = ([("rigid3", e) for e in ENTRIES] + [("hbonds", e) for e in ("emdee_md_step", "emdee_md_minimize")] +
         [("vsites", e) for e in ("emdee_md_step", "emdee_md_minimize", "emdee_md_scale_box")])
BENT = 3                                                 # the molecule, cluster or site of the state that does not fit


def _box(table):
    """dict(pos, unwrapped, vel, atoms, inv_mass, mol, rows, params): the table of the first m molecules is rows[:m], params[:m]"""
    W = sr.water_box(n_mol=N_MOL, lengths=LENGTHS, lo=LO)
    atoms = W["atoms"].copy()
    atoms["twice_sqrt_eps"] = 0.0
    B = dict(pos=W["pos"], unwrapped=W["unwrapped"], vel=W["vel"], atoms=atoms, inv_mass=1.0 / W["mass"], mol=W["mol"])
    if table == "rigid3":
        B.update(rows=W["mol"], params=W["geom"])
    elif table == "hbonds":
        B.update(rows=np.concatenate([W["mol"], np.full((N_MOL, 1), -1)], axis=1), params=np.tile([sr.D_LEG, sr.D_LEG, 0.0], (N_MOL, 1)))
    else:
        sites = np.arange(3 * N_MOL, 4 * N_MOL)
        rows, weights = np.concatenate([sites[:, None], W["mol"]], axis=1), np.full((N_MOL, 2), vr.W_SITE)
        xs = vr.place(W["unwrapped"], rows, weights, LENGTHS)
        site_atoms = np.zeros(N_MOL, dtype=atoms.dtype)
        site_atoms["half_sigma"] = 0.1
        B.update(pos=np.concatenate([W["pos"], LO + np.mod(xs - LO, LENGTHS)]), vel=np.concatenate([W["vel"], np.zeros((N_MOL, 3))]),
                 atoms=np.concatenate([atoms, site_atoms]), inv_mass=np.concatenate([B["inv_mass"], np.zeros(N_MOL)]), rows=rows, params=weights)
    return B


def _set_table(md, table, B, m):
    {"rigid3": md.set_rigid3_, "hbonds": md.set_hbonds_, "vsites": md.set_vsites_}[table](B["rows"][:m], B["params"][:m])


def _load(E, dev, md, B, n, pos=None, inv_mass=None):
    pos, inv_mass = B["pos"] if pos is None else pos, B["inv_mass"] if inv_mass is None else inv_mass
    md.set_state_(E.cu(pos[:n], dev), E.cu(B["vel"][:n], dev), E.cu(B["atoms"][:n], dev), E.cu(inv_mass[:n], dev))


def _refusal(E, call, *args):
    with pytest.raises(E.EmDeeError) as err:
        call(*args)
    return [err.value.code, str(err.value)]


def refusals(E, dev, table, entry):
    """{"other_count", "set_state", "unfit"}: [code, text] of the entry's refusal after a set_state with another atom count, of
    the set_state with a state that does not fit, and of the entry after it.  Steps once after every recovery."""
    B = _box(table)
    n = len(B["pos"])
    fewer = n - 1 if table == "vsites" else n - 3            # one site or one molecule less: a table of N_MOL - 1 rows fits it
    md = E.VelocityVerlet(E.cu(B["pos"], dev), E.cu(B["vel"], dev), SIDE, E.LennardJonesModel(sr.RC, sr.RS), E.cu(B["atoms"], dev), skin=sr.SKIN,
                          inv_mass=E.cu(B["inv_mass"], dev), lo=list(LO), lengths=list(LENGTHS), periodic=[1, 1, 1])
    if (table, entry) == ("rigid3", "emdee_md_scale_box"):
        md.set_molecular_scaling_()                          # (without it scale_box refuses the rigid table itself, fitting or not)
    _set_table(md, table, B, N_MOL)
    md.step_(1, DT)
    out = {}
    _load(E, dev, md, B, fewer)
    out["other_count"] = _refusal(E, ENTRIES[entry], md)
    _set_table(md, table, B, N_MOL - 1)                      # set again for this count: steps
    md.step_(1, DT)
    _load(E, dev, md, B, n)
    _set_table(md, table, B, N_MOL)
    md.step_(1, DT)
    pos, inv_mass = B["pos"].copy(), B["inv_mass"].copy()
    if table == "vsites":
        inv_mass[B["rows"][BENT, 0]] = 1.0                   # (a site loaded with a mass)
    else:
        apex, leg = B["mol"][BENT, 0], B["mol"][BENT, 1]
        pos[leg] += 0.03 * (B["unwrapped"][leg] - B["unwrapped"][apex])      # (3 % farther out: thirty times the check's bound)
    out["set_state"] = _refusal(E, _load, E, dev, md, B, n, pos, inv_mass)
    out["unfit"] = _refusal(E, ENTRIES[entry], md)
    _load(E, dev, md, B, n)                                  # a state that fits: checked again, steps
    md.step_(1, DT)
    md.close()
    return out


def _key(table, entry):
    return "%s/%s" % (table, entry)


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_the_cases_and_nothing_else(recorded):
    assert sorted(recorded) == sorted(_key(t, e) for t, e in CASES)


@pytest.mark.parametrize("table,entry", CASES, ids=[_key(t, e) for t, e in CASES])
def test_refusals_are_the_recorded_ones_and_the_table_set_again_steps(emdee, dev, recorded, table, entry):
    got, want = refusals(emdee, dev, table, entry), recorded[_key(table, entry)]
    for which in ("other_count", "set_state", "unfit"):
        print("%s, %s: %s" % (_key(table, entry), which, got[which]))
    for which in ("other_count", "set_state", "unfit"):
        assert got[which][0] == ERR_STATE and got[which] == want[which], which


if __name__ == "__main__":
    from __graft_entry__ import load_package
    E, device = load_package(), torch.device("cuda", 0)
    texts = {_key(t, e): refusals(E, device, t, e) for t, e in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as fh:
        json.dump(texts, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded %d cases from %s" % (len(texts), E._lib.LIB_PATH))
