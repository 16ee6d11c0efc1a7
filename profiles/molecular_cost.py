"""Device time of the molecular sums and the molecular scale at the size of examples/rigid_water.py (12^3 = 1728 rigid three-site
molecules, 5184 atoms, fp64, masses, reaction field, Langevin): emdee_md_kernel_time index 10 (the molecule pass of the molecular
sums once and k_molecule_scale once per coupling event) per event, against index 9 (the three constraint stages) per step and the wall time
of one rigid step without coupling -- the step of the commit before molecular scaling, whose loop and kernels are unchanged.
A number for the record, not a gate.

    python3 profiles/molecular_cost.py [--steps 400] [--warmup 100] [--every 10]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()
R_OH, D_HH, KB, T, DT = 0.1, 2.0 * 0.1 * np.sin(0.5 * np.deg2rad(109.47)), 0.0083144626, 300.0, 0.002
BAR = 0.0602214076


def water(cells, rng):
    n = cells ** 3
    L = (n / 33.4) ** (1.0 / 3.0)
    h = np.sqrt(R_OH ** 2 - 0.25 * D_HH ** 2)
    site = np.array([[0.0, 0.0, 0.0], [-0.5 * D_HH, -h, 0.0], [0.5 * D_HH, -h, 0.0]])
    grid = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = np.mod(((grid + 0.5) * (L / cells))[:, None, :] + site, L).reshape(-1, 3)
    mass = np.tile([15.9994, 1.008, 1.008], n)
    vel = rng.normal(size=(3 * n, 3)) * np.sqrt(KB * T / mass)[:, None]
    atoms = E.lennard_jones_atoms(np.tile([0.650194, 0.0, 0.0], n), np.tile([0.316557, 0.1, 0.1], n))
    return pos, vel, L, mass, atoms, np.arange(3 * n).reshape(-1, 3)


def engine(dev, cells):
    pos, vel, L, mass, atoms, mol = water(cells, np.random.default_rng(2026))
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(0.9, 0.8), E.cu(atoms, dev), skin=0.1,
                          inv_mass=E.cu(1.0 / mass, dev))
    md.set_exclusions_(np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]]))
    md.set_coulomb_(np.tile([-0.8476, 0.4238, 0.4238], mol.shape[0]), E.COULOMB_K_KJ_NM, eps_rf=78.0)
    md.set_rigid3_(mol, np.tile([R_OH, D_HH], (mol.shape[0], 1)))
    md.set_langevin_(gamma=5.0, temperature=KB * T, seed=2026)
    return md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--cells", type=int, default=12)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for coupled in (False, True, False, True):
        md = engine(dev, a.cells)
        if coupled:
            md.set_molecular_scaling_()
            md.set_barostat_("c-rescale", BAR, 4.5e-5 / BAR, 1.0, a.every, temperature=KB * T, seed=2027)
        md.step_(a.warmup, DT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        md.step_(a.steps, DT)
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0) / a.steps
        md.profile_(True)
        md.step_(a.steps, DT)
        settle_ms, settle_n = md.kernel_time("settle")
        mol_ms, mol_n = md.kernel_time("molecular")
        events = a.steps // a.every if coupled else 0
        print("%s: %.4f ms/step wall; constraint stages %.4f ms/step device (%d launches); molecular sums + scale %s"
              % ("coupled every %d" % a.every if coupled else "uncoupled", wall, settle_ms / a.steps, settle_n,
                 "%.4f ms/event device (%d launches, %d events)" % (mol_ms / max(events, 1), mol_n, events) if coupled else "none"))
        md.close()


if __name__ == "__main__":
    main()
