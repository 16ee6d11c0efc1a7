"""Device time of the hbonds constraint stages (emdee_md_set_hbonds; csrc/shake.hpp) and the energy drift they leave.

Cost: 10^5 three-atom groups (3 x 10^5 atoms: a centre of mass 16 and two satellites of mass 1 at 0.32, the geometry of
tests/helpers/settle_ref.py, on a 47^3 lattice of spacing 1.25 with the first 10^5 sites filled; rc = 2.5, skin = 0.4, dt =
0.002, NVE), in fp64 and fp32, once as 10^5 clusters of three (emdee_md_kernel_time index 11) and once as 10^5 rigid molecules
(index 9), each against the force pass of the same run (index 0).  Every step of either run launches three constraint kernels
and one plain force pass.

Drift: max |E(t) - E(0)| over 400 steps of the box of tests/test_gpu_hbonds.py (clusters and waters in force), sampled every
20, beside the figure of the numpy yardstick from the same start (python -m tests.helpers.shake_ref, a minute on a CPU;
--reference computes it here).

Numbers for the record, not gates.

    python3 profiles/hbonds_cost.py [--steps 200] [--warmup 50] [--groups 100000] [--reference]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tests.helpers import settle_ref as sr  # noqa: E402
from tests.helpers import shake_ref as hr  # noqa: E402

E = load_package()
SPACING, DT = 1.25, 0.002


def groups(n, rng):
    side = int(np.ceil(n ** (1.0 / 3.0)))
    L = side * SPACING
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    centres = (grid + 0.5 + 0.2 * (rng.random((n, 3)) - 0.5)) * SPACING
    sites = np.einsum("nij,kj->nki", sr.random_rotations(rng, n), sr.triangle(sr.D_LEG, sr.D_BASE))
    x = (centres[:, None, :] + sites).reshape(-1, 3)
    mass = np.tile(sr.MASSES, n)
    vel = rng.normal(size=x.shape) / np.sqrt(mass)[:, None]
    atoms = np.zeros(3 * n, dtype=E.LJAtom)
    atoms["half_sigma"], atoms["twice_sqrt_eps"] = np.tile(sr.HALF_SIGMA, n), np.tile(sr.TWICE_SQRT_EPS, n)
    return np.mod(x, L), vel, L, mass, atoms, np.arange(3 * n).reshape(-1, 3)


def cost(dev, a):
    pos, vel, L, mass, atoms, mol = groups(a.groups, np.random.default_rng(2026))
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]])
    for dtype in (np.float64, np.float32):
        for kind in ("hbonds", "settle"):
            md = E.VelocityVerlet(E.cu(pos.astype(dtype), dev), E.cu(vel.astype(dtype), dev), L, E.LennardJonesModel(sr.RC, sr.RS),
                                  E.cu(atoms, dev), skin=sr.SKIN, inv_mass=E.cu((1.0 / mass).astype(dtype), dev))
            md.set_exclusions_(excl)
            if kind == "hbonds":
                md.set_hbonds_(np.concatenate([mol, np.full((len(mol), 1), -1)], axis=1), np.tile([sr.D_LEG, sr.D_LEG, 0.0], (len(mol), 1)))
            else:
                md.set_rigid3_(mol, np.tile([sr.D_LEG, sr.D_BASE], (len(mol), 1)))
            md.step_(a.warmup, DT)
            md.profile_(True)
            md.step_(a.steps, DT)
            ms, n = md.kernel_time(kind)
            force_ms, force_n = md.kernel_time("lj_force_nbr")
            print("%s, %d %s: constraint stages %.4f ms/step device (%d launches); force pass %.4f ms/step (%d launches); ratio %.3f"
                  % (np.dtype(dtype).name, a.groups, "clusters of three" if kind == "hbonds" else "rigid molecules", ms / a.steps, n,
                     force_ms / a.steps, force_n, ms / force_ms), flush=True)
            md.close()


def drift(dev, a):
    B = hr.mixed_box()
    md = E.VelocityVerlet(E.cu(B["pos"], dev), E.cu(B["vel"], dev), float(hr.LENGTHS[0]), E.LennardJonesModel(hr.RC, hr.RS),
                          E.cu(B["atoms"], dev), skin=hr.SKIN, inv_mass=E.cu(1.0 / B["mass"], dev), lo=list(hr.LO),
                          lengths=list(hr.LENGTHS), periodic=[1, 1, 1])
    md.set_exclusions_(B["excl"])
    md.set_hbonds_(B["clusters"], B["dist"])
    md.set_rigid3_(B["mol"], B["geom"])
    ep, ek, _ = md.totals()
    e0, worst = ep + ek, 0.0
    for _ in range(20):
        md.step_(20, hr.DT)
        ep, ek, _ = md.totals()
        worst = max(worst, abs(ep + ek - e0))
    md.close()
    print("engine: E(0) = %.6f, max |E(t) - E(0)| over 400 steps of dt = %g, sampled every 20: %.6e" % (e0, hr.DT, worst), flush=True)
    if a.reference:
        ref, e0 = hr.reference_drift()
        print("yardstick: E(0) = %.6f, max |E(t) - E(0)| = %.6e" % (e0, ref), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--groups", type=int, default=100000)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    drift(dev, a)
    cost(dev, a)


if __name__ == "__main__":
    main()
