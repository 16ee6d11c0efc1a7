#!/usr/bin/env python3
"""Both stages of a solvation free energy of a charged solute on one MI355X, by thermodynamic integration: one rigid SPC/E water
molecule in SPC/E water on the reaction field (eps_rf = 78), under stochastic velocity rescaling at 300 K with a time step of 2 fs.
The molecule is flagged as the solute (emdee_md_set_alchemical).  First the Coulomb stage (emdee_md_set_alchemical_coulomb) takes
lambda_q from 1 to 0 at lambda = 1: the charge term of every solute-solvent pair goes through the soft core
U_q = lambda_q qq (1/rho + k_rf rho^2 - c_rf), rho^2 = r^2 + beta (1 - lambda_q), while the molecule's own pairs keep their charges.
Then the Lennard-Jones stage takes lambda from 1 to 0 at lambda_q = 0.  In every window the two on-device logs take dU/dlambda (or
dU_q/dlambda_q), the energies and the energies at the two neighbouring windows every few steps; no position leaves the device.
Per window the mean derivative is printed, then the two trapezoid sums -- their sum is the free energy of coupling the molecule, the
negative of water's excess chemical potential up to the finite-size and cutoff corrections -- and, per pair of neighbouring windows,
the mean foreign-energy differences in both directions, which is what a BAR estimate of the same differences takes.

    python examples/charged_solvation.py [--molecules 512] [--melt 2000] [--windows 11] [--equil 500] [--steps 4000] [--every 10]
                                         [--alpha 0.5] [--beta 0.12]

--molecules 64 is the small size: the cutoff shrinks with the box (rc = min(0.9 nm, L / 2 - skin)).  Units: nm, ps, atomic mass
units, kJ/mol, elementary charges; beta in nm^2.  Needs the built library (python -c "import __graft_entry__ as g; g.build()") and a
gfx950 device."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--molecules", type=int, default=512)
ap.add_argument("--melt", type=int, default=2000)
ap.add_argument("--windows", type=int, default=11)
ap.add_argument("--equil", type=int, default=500)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--beta", type=float, default=0.12)
args = ap.parse_args()

E = load_package()
dev = torch.device("cuda", 0)

# SPC/E: r(OH) = 0.1 nm, tetrahedral angle, q = -0.8476 / +0.4238, LJ on the oxygen only
R_OH, THETA = 0.1, np.deg2rad(109.47)
D_HH = 2.0 * R_OH * np.sin(0.5 * THETA)
SIGMA_O, EPS_O = 0.316557, 0.650194
MASS = np.array([15.9994, 1.008, 1.008])
KB = 0.0083144626                                                # kJ/mol/K
T, DT, SKIN = 300.0, 0.002, 0.1

rng = np.random.default_rng(2026)
n_mol = args.molecules
L = (n_mol / 33.4) ** (1.0 / 3.0)                                # 33.4 molecules per nm^3: 0.997 g/cm^3
RC = min(0.9, 0.5 * L - SKIN - 1e-3)
if RC < 0.45:
    sys.exit("the box side %.2f nm leaves a cutoff of %.2f nm: use more molecules" % (L, RC))
cells = int(np.ceil(n_mol ** (1.0 / 3.0) - 1e-9))
h = np.sqrt(R_OH ** 2 - 0.25 * D_HH ** 2)
site = np.array([[0.0, 0.0, 0.0], [-0.5 * D_HH, -h, 0.0], [0.5 * D_HH, -h, 0.0]])
quat = rng.normal(size=(n_mol, 4))
quat /= np.linalg.norm(quat, axis=1)[:, None]
a, b, c, d = quat.T                                              # random orientations from unit quaternions
rot = np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], axis=1),
                np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], axis=1),
                np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], axis=1)], axis=1)
grid = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n_mol]
centres = (grid + 0.5) * (L / cells)
pos = np.mod((centres[:, None, :] + np.einsum("nij,kj->nki", rot, site)).reshape(-1, 3), L)

N = 3 * n_mol
mass = np.tile(MASS, n_mol)
vel = rng.normal(size=(N, 3)) * np.sqrt(KB * T / mass)[:, None]  # set_rigid3_ removes the components along the bonds
atoms = E.lennard_jones_atoms(np.tile([EPS_O, 0.0, 0.0], n_mol), np.tile([SIGMA_O, 0.1, 0.1], n_mol))
mol = np.arange(N).reshape(-1, 3)                                # {O, H, H} per molecule: the apex first
solute = int(np.argmin(((centres - 0.5 * L) ** 2).sum(axis=1)))  # the molecule nearest the middle of the box
flag = np.zeros(N, dtype=np.int32)
flag[mol[solute]] = 1

md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(RC, RC - 0.1), E.cu(atoms, dev), skin=SKIN,
                      inv_mass=E.cu(1.0 / mass, dev))
md.set_exclusions_(np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]]))
md.set_coulomb_(np.tile([-0.8476, 0.4238, 0.4238], n_mol), E.COULOMB_K_KJ_NM, eps_rf=78.0)
md.set_rigid3_(mol, np.tile([R_OH, D_HH], (n_mol, 1)))
# the lattice start has molecules at random orientations next to each other: relax it before the first 2 fs step
md.minimize_(500, 500.0, dt_start=0.0002, dt_max=0.002, max_step=0.01)
md.set_state_(md.state(velocities=False, forces=False)["positions"], E.cu(vel, dev), E.cu(atoms, dev), E.cu(1.0 / mass, dev))
md.set_thermostat_("v-rescale", temperature=KB * T, tau_t=0.1, seed=2026)
md.step_(args.melt, DT)
ek = md.totals()[1]
print("# %d rigid SPC/E molecules, box %.3f nm, rc %.3f nm, molecule %d flagged, %d steps of equilibration: T = %.1f K"
      % (n_mol, L, RC, solute, args.melt, 2.0 * ek / (6 * n_mol * KB)))

sched = np.linspace(1.0, 0.0, args.windows)                      # from the coupled molecule down: every window starts equilibrated nearby
capacity = args.steps // args.every


def window(lam, lam_q, foreign, foreign_q):
    """equilibrate at (lam, lam_q), then sample: the table is set again with its log, which clears the stage, so the stage follows it"""
    md.set_alchemical_(flag, lam=lam, alpha=args.alpha)
    md.set_alchemical_coulomb_(lam_q, args.beta)
    md.step_(args.equil, DT)
    md.set_alchemical_(flag, lam=lam, alpha=args.alpha, foreign=foreign, log_every=args.every, log_capacity=capacity)
    md.set_alchemical_coulomb_(lam_q, args.beta, foreign_q=foreign_q)
    md.step_(args.steps, DT)
    lj, cq = md.alchemical_log(), md.alchemical_coulomb_log()    # two reads per window
    assert lj["dropped"] == 0 and cq["count"] == lj["count"]
    # the energy of a foreign state less the energy here: both logs' entries are taken at the same passes
    diff = (lj["foreign"] + cq["foreign"]) - (lj["U"] + cq["U"])[:, None]
    return lj, cq, diff.mean(axis=0)


def stage(name, states, which):
    means, up, down = [], [], []
    for w, x in enumerate(sched):
        near = [float(sched[max(w - 1, 0)]), float(sched[min(w + 1, len(sched) - 1)])]
        lam, lam_q, foreign, foreign_q = states(float(x), near)
        lj, cq, diff = window(lam, lam_q, foreign, foreign_q)
        log = cq if which == "q" else lj
        means.append(log["dUdl"].mean())
        up.append(diff[0])                                       # towards the previous window of the schedule
        down.append(diff[1])                                     # towards the next
        print("%s %.4f %.6f %.6f %d" % (name, x, means[-1], log["U"].mean(), log["count"]))
    order = np.argsort(sched)
    xs, ys = sched[order], np.array(means)[order]
    return float(np.sum(0.5 * (ys[1:] + ys[:-1]) * np.diff(xs))), up, down


print("# stage  lambda_q or lambda  <dU/dlambda>  <U>  samples   (kJ/mol)")
ti_q, up_q, down_q = stage("coulomb", lambda x, near: (1.0, x, [1.0, 1.0], near), "q")
ti_lj, up_lj, down_lj = stage("lj", lambda x, near: (x, 0.0, near, [0.0, 0.0]), "lj")
print("# A(1) - A(0) of either stage by the trapezoid rule over its mean derivative; their sum couples the whole molecule")
print("ti_coulomb %.6f" % ti_q)
print("ti_lj %.6f" % ti_lj)
print("# stage  x -> x'  <U(x') - U(x)>_x  <U(x) - U(x')>_x'   (what a BAR estimate takes)")
for name, up, down in (("bar_coulomb", up_q, down_q), ("bar_lj", up_lj, down_lj)):
    for w in range(len(sched) - 1):
        print("%s %.4f %.4f %.6f %.6f" % (name, sched[w], sched[w + 1], down[w], up[w + 1]))
md.close()
