"""Device time of one molecular-sums call and one molecular scale over a molecule table (emdee_md_set_molecules) at 10^6 atoms: 70^3 =
343,000 rigid three-site waters (1,029,000 atoms, fp64, masses, reaction field), emdee_md_kernel_time index 10 per call, against the
plain force pass of the same run (index 0).  Three tables:

  triangle   no molecule table: the Triangle kernels over the rigid table (one launch per call);
  general    a table that names exactly the waters: k_molecule_centres + the entries' pass or k_molecule_shift (two launches per call);
  mixed      the same with eight runs of 3334 waters merged into eight molecules of 10,002 atoms (one wavefront each in the centres).

A number for the record, not a gate: nothing routes water away from the Triangle path unless a table is set.

    python3 profiles/molecule_cost.py [--cells 70] [--reps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()
R_OH, D_HH, KB, T = 0.1, 2.0 * 0.1 * np.sin(0.5 * np.deg2rad(109.47)), 0.0083144626, 300.0
BIG, N_BIG = 3334, 8


def water(cells, rng):
    """whole molecules: the sites are not wrapped into the box one by one"""
    n = cells ** 3
    L = (n / 33.4) ** (1.0 / 3.0)
    h = np.sqrt(R_OH ** 2 - 0.25 * D_HH ** 2)
    site = np.array([[0.0, 0.0, 0.0], [-0.5 * D_HH, -h, 0.0], [0.5 * D_HH, -h, 0.0]])
    grid = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = (((grid + 0.5) * (L / cells))[:, None, :] + site).reshape(-1, 3)
    mass = np.tile([15.9994, 1.008, 1.008], n)
    vel = rng.normal(size=(3 * n, 3)) * np.sqrt(KB * T / mass)[:, None]
    atoms = E.lennard_jones_atoms(np.tile([0.650194, 0.0, 0.0], n), np.tile([0.316557, 0.1, 0.1], n))
    return pos, vel, L, mass, atoms, np.arange(3 * n).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=70)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pos, vel, L, mass, atoms, mol = water(a.cells, np.random.default_rng(2026))
    n_mol = mol.shape[0]
    ids = np.repeat(np.arange(n_mol, dtype=np.int32), 3)
    mixed = ids.copy()
    for b in range(min(N_BIG, n_mol // BIG)):
        mixed[3 * b * BIG:3 * (b + 1) * BIG] = n_mol + b
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(0.9, 0.8), E.cu(atoms, dev), skin=0.1,
                          inv_mass=E.cu(1.0 / mass, dev))
    md.set_exclusions_(np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]]))
    md.set_coulomb_(np.tile([-0.8476, 0.4238, 0.4238], n_mol), E.COULOMB_K_KJ_NM, eps_rf=78.0)
    md.set_rigid3_(mol, np.tile([R_OH, D_HH], (n_mol, 1)))
    md.set_molecular_scaling_()
    print("%d atoms in %d waters, box %.3f nm" % (pos.shape[0], n_mol, L))
    for name, table in (("triangle", None), ("general", ids), ("mixed", mixed), ("triangle", None), ("general", ids)):
        md.set_molecules_(table)
        md.molecular_tensor_sums()                                           # (warm: the first launch of a kernel loads it)
        md.scale_box_(1.0)
        md.profile_(True)
        for _ in range(a.reps):
            md.molecular_tensor_sums()
        sums_ms, sums_n = md.kernel_time("molecular")
        md.profile_(True)
        for r in range(a.reps):
            md.scale_box_(1.00001 if r % 2 == 0 else 1.0 / 1.00001)          # (each scale rebuilds and ends with a plain force pass)
        scale_ms, scale_n = md.kernel_time("molecular")
        force_ms, force_n = md.kernel_time("lj_force_nbr")
        print("%-9s molecular sums %.4f ms per call (%d launches), molecular scale %.4f ms per call (%d launches); plain force pass %.4f ms"
              % (name, sums_ms / a.reps, sums_n // a.reps, scale_ms / a.reps, scale_n // a.reps, force_ms / max(force_n, 1)))
        md.profile_(False)
    md.close()


if __name__ == "__main__":
    main()
