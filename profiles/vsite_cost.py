"""Device time of placement and force spreading of virtual sites (emdee_md_set_vsites; csrc/vsite.hpp) beside the force pass.

Two boxes of four-site rigid water, the molecule of tests/helpers/vsite_ref.py (masses 16, 1, 1, d_leg 0.32, d_base 0.50, a
massless site on the bisector at w_b = w_c = 0.13 that carries the apex charge; reaction field, rc = 2.5, skin = 0.4, dt = 0.002,
NVE): the 600-atom box of tests/test_gpu_vsites.py, and 10^5 molecules (4 x 10^5 atoms) on the lattice of profiles/hbonds_cost.py.
Every step launches one placement and the two spreading kernels (emdee_md_kernel_time index 13) beside the three SETTLE stages
(index 9) and one force pass (index 0).

Numbers for the record, not gates.

    python3 profiles/vsite_cost.py [--steps 200] [--warmup 50] [--groups 100000]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from profiles.hbonds_cost import DT, groups  # noqa: E402
from tests.helpers import settle_ref as sr  # noqa: E402
from tests.helpers import vsite_ref as vr  # noqa: E402

E = load_package()


def four_site(pos, vel, L, mass, atoms, mol):
    """the three-site groups of hbonds_cost.groups with a site per molecule appended (vsite_ref.four_site_box's recipe)"""
    n = len(mol)
    sites = 3 * n + np.arange(n)
    vs_atoms, vs_weights = np.concatenate([sites[:, None], mol], axis=1), np.full((n, 2), vr.W_SITE)
    ln = np.array([L] * 3) if np.isscalar(L) else np.asarray(L)
    xs = vr.place(pos, vs_atoms, vs_weights, ln)
    site_atoms = np.zeros(n, dtype=atoms.dtype)
    site_atoms["half_sigma"] = 0.1
    charges = np.concatenate([np.tile(sr.CHARGES, n), np.full(n, sr.CHARGES[0])])
    charges[mol[:, 0]] = 0.0
    four = np.concatenate([mol, sites[:, None]], axis=1)
    excl = np.concatenate([four[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    return dict(pos=np.concatenate([pos, xs]), vel=np.concatenate([vel, np.zeros((n, 3))]), inv_mass=np.concatenate([1.0 / mass, np.zeros(n)]),
                atoms=np.concatenate([atoms, site_atoms]), charges=charges, excl=excl, mol=mol, vs_atoms=vs_atoms, vs_weights=vs_weights)


def measure(dev, a, what, B, lo, lengths, dtype):
    md = E.VelocityVerlet(E.cu(B["pos"].astype(dtype), dev), E.cu(B["vel"].astype(dtype), dev), float(lengths[0]), E.LennardJonesModel(sr.RC, sr.RS),
                          E.cu(B["atoms"], dev), skin=sr.SKIN, inv_mass=E.cu(B["inv_mass"].astype(dtype), dev), lo=list(lo), lengths=list(lengths),
                          periodic=[1, 1, 1])
    md.set_exclusions_(B["excl"])
    md.set_coulomb_(B["charges"], 1.0)
    md.set_rigid3_(B["mol"], np.tile([sr.D_LEG, sr.D_BASE], (len(B["mol"]), 1)))
    md.set_vsites_(B["vs_atoms"], B["vs_weights"])
    md.step_(a.warmup, DT)
    md.profile_(True)
    md.step_(a.steps, DT)
    ms, n = md.kernel_time("vsites")
    settle_ms, _ = md.kernel_time("settle")
    force_ms, force_n = md.kernel_time("lj_force_nbr")
    print("%s, %s: place + spread %.4f ms/step device (%d timed stages); SETTLE stages %.4f ms/step; force pass %.4f ms/step (%d launches); "
          "sites / force pass %.3f" % (np.dtype(dtype).name, what, ms / a.steps, n, settle_ms / a.steps, force_ms / a.steps, force_n, ms / force_ms), flush=True)
    md.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--groups", type=int, default=100000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    small = vr.four_site_box()
    big = four_site(*groups(a.groups, np.random.default_rng(2026)))
    side = int(np.ceil(a.groups ** (1.0 / 3.0))) * 1.25
    for dtype in (np.float64, np.float32):
        measure(dev, a, "150 molecules (600 atoms)", small, sr.LO, sr.LENGTHS, dtype)
        measure(dev, a, "%d molecules (%d atoms)" % (a.groups, 4 * a.groups), big, [0.0, 0.0, 0.0], [side] * 3, dtype)


if __name__ == "__main__":
    main()
