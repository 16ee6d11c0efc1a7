#!/usr/bin/env python3
"""A small box of rigid three-site water on one MI355X: SPC/E geometry and charges, reaction-field electrostatics, the Langevin
thermostat at 300 K and a time step of 2 fs, which the rigid molecules (emdee_md_set_rigid3: SETTLE + RATTLE) make possible.
The lattice start is relaxed by emdee_md_minimize first.  Prints the largest bond-length deviation and the temperature as it runs.  An NPT leg follows: stochastic cell rescaling
(C-rescale) at 1 bar with the Langevin thermostat, coupled to the molecular pressure and scaling the box by molecular centres of
mass (emdee_md_set_molecular_scaling), which keeps the molecules rigid; it prints the box side and P_mol as well.

    python examples/rigid_water.py [cells] [steps] [npt_steps]   # cells^3 molecules (default 12: 1728), steps (default 2000),
                                                                 # npt_steps (default 1000; 0 leaves the NPT leg out)

Units: nm, ps, atomic mass units, kJ/mol, elementary charges.  Needs the built library
(python -c "import __graft_entry__ as g; g.build()") and a gfx950 device."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()
dev = torch.device("cuda", 0)
cells = int(sys.argv[1]) if len(sys.argv) > 1 else 12
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
npt_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 1000

# SPC/E: r(OH) = 0.1 nm, tetrahedral angle, q = -0.8476 / +0.4238, LJ on the oxygen only
R_OH, THETA = 0.1, np.deg2rad(109.47)
D_HH = 2.0 * R_OH * np.sin(0.5 * THETA)
SIGMA_O, EPS_O = 0.316557, 0.650194
MASS = np.array([15.9994, 1.008, 1.008])
KB = 0.0083144626                                                # kJ/mol/K
T, DT, RC = 300.0, 0.002, 0.9
BAR = 0.0602214076                                               # 1 bar in kJ/mol/nm^3
P_REF, BETA, TAU_P, EVERY = 1.0 * BAR, 4.5e-5 / BAR, 1.0, 10     # water's compressibility 4.5e-5 / bar; tau_p in ps

rng = np.random.default_rng(2026)
n_mol = cells ** 3
L = (n_mol / 33.4) ** (1.0 / 3.0)                                # 33.4 molecules per nm^3: 0.997 g/cm^3
if L < 2.0 * (RC + 0.1):
    sys.exit("the box side %.2f nm is below 2 (rc + skin) = %.2f nm: use more cells" % (L, 2.0 * (RC + 0.1)))
h = np.sqrt(R_OH ** 2 - 0.25 * D_HH ** 2)
site = np.array([[0.0, 0.0, 0.0], [-0.5 * D_HH, -h, 0.0], [0.5 * D_HH, -h, 0.0]])
q = rng.normal(size=(n_mol, 4))
q /= np.linalg.norm(q, axis=1)[:, None]
a, b, c, d = q.T                                                 # random orientations from unit quaternions
rot = np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], axis=1),
                np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], axis=1),
                np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], axis=1)], axis=1)
grid = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
centres = (grid + 0.5) * (L / cells)
pos = np.mod((centres[:, None, :] + np.einsum("nij,kj->nki", rot, site)).reshape(-1, 3), L)

N = 3 * n_mol
mass = np.tile(MASS, n_mol)
vel = rng.normal(size=(N, 3)) * np.sqrt(KB * T / mass)[:, None]  # set_rigid3_ removes the components along the bonds
atoms = E.lennard_jones_atoms(np.tile([EPS_O, 0.0, 0.0], n_mol), np.tile([SIGMA_O, 0.1, 0.1], n_mol))
mol = np.arange(N).reshape(-1, 3)                                # {O, H, H} per molecule: the apex first

md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(RC, 0.8), E.cu(atoms, dev), skin=0.1,
                      inv_mass=E.cu(1.0 / mass, dev))
md.set_exclusions_(np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]]))
md.set_coulomb_(np.tile([-0.8476, 0.4238, 0.4238], n_mol), E.COULOMB_K_KJ_NM, eps_rf=78.0)
md.set_rigid3_(mol, np.tile([R_OH, D_HH], (n_mol, 1)))
md.set_langevin_(gamma=5.0, temperature=KB * T, seed=2026)       # 1/ps
# the lattice start has molecules at random orientations next to each other: relax it before the first 2 fs step
# (emdee_md_minimize: FIRE around the constrained step; it leaves the velocities at zero, so they are loaded again)
res = md.minimize_(500, 500.0, dt_start=0.0002, dt_max=0.002, max_step=0.01)
print("minimised: %d iterations, converged = %s, E_pot %.1f -> %.1f kJ/mol, largest constrained force %.1f kJ/mol/nm"
      % (res.iterations, res.converged, res.energy0, res.energy, res.g_max))
md.set_state_(md.state(velocities=False, forces=False)["positions"], E.cu(vel, dev), E.cu(atoms, dev), E.cu(1.0 / mass, dev))


def report(step, npt=False):
    x = md.state(velocities=False, forces=False)["positions"].cpu().numpy()
    side = np.array(md.box()[1])
    dev_max = 0.0
    for i, j, want in ((0, 1, R_OH), (0, 2, R_OH), (1, 2, D_HH)):
        r = x[mol[:, i]] - x[mol[:, j]]
        r -= side * np.rint(r / side)
        dev_max = max(dev_max, np.abs(np.linalg.norm(r, axis=1) / want - 1.0).max())
    ep, ek, _ = md.totals()
    # 6 degrees of freedom per rigid molecule
    line = ("step %6d  t = %7.3f ps  T = %6.1f K  E_pot = %10.1f kJ/mol  largest bond-length deviation %.2e"
            % (step, step * DT, 2.0 * ek / (6 * n_mol * KB), ep, dev_max))
    if npt:
        p_mol = np.trace(md.molecular_pressure_tensor()["pressure"]) / 3.0
        line += "  box %.4f nm  P_mol = %8.1f bar  density %.1f / nm^3" % (side[0], p_mol / BAR, n_mol / np.prod(side))
    print(line)
    return dev_max


print("%d rigid SPC/E molecules, box %.3f nm, dt = %g fs, reaction field (eps_rf = 78), Langevin at %g K" % (n_mol, L, 1e3 * DT, T))
report(0)
done = 0
while done < steps:
    n = min(200, steps - done)
    md.step_(n, DT)
    done += n
    report(done)

if npt_steps > 0:
    md.set_molecular_scaling_()                                  # lets the engine with the rigid table take a barostat
    md.set_barostat_("c-rescale", P_REF, BETA, TAU_P, EVERY, temperature=KB * T, seed=2027)
    print("NPT: C-rescale at %g bar every %d steps (tau_p = %g ps), coupled to the molecular pressure" % (P_REF / BAR, EVERY, TAU_P))
    worst, done = report(steps, npt=True), 0
    while done < npt_steps:
        n = min(200, npt_steps - done)
        md.step_(n, DT)
        done += n
        worst = max(worst, report(steps + done, npt=True))
    assert worst < 1e-10, "the molecules lost their geometry under the molecular scale"
md.close()
