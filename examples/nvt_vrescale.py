#!/usr/bin/env python3
"""Rigid SPC/E water on one MI355X under a global thermostat: stochastic velocity rescaling (emdee_md_set_thermostat, kind
v-rescale) at 300 K and a time step of 2 fs, with the library's own count of the degrees of freedom (n_dof = 0: 6 per rigid
molecule minus 3), then the same thermostat together with stochastic cell rescaling (C-rescale) at 1 bar on the molecular
pressure.  Unlike the Langevin thermostat of examples/rigid_water.py this one multiplies all velocities by one factor per
event and leaves the dynamics of the atoms alone.  Prints T and, for the NVT leg, U + K + E_th: the thermostat books the energy
it moves in E_th, so the sum is conserved to the integrator's error.

    python examples/nvt_vrescale.py [cells] [steps] [npt_steps]   # cells^3 molecules (default 12: 1728), steps (default 2000),
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
TAU_T, EVERY_T = 0.1, 10                                         # ps; an event every 10 steps
BAR = 0.0602214076                                               # 1 bar in kJ/mol/nm^3
P_REF, BETA, TAU_P, EVERY_P = 1.0 * BAR, 4.5e-5 / BAR, 1.0, 10   # water's compressibility 4.5e-5 / bar; tau_p in ps

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
vel -= (mass[:, None] * vel).sum(axis=0) / mass.sum()            # no momentum of the box: the 3 the count takes off
atoms = E.lennard_jones_atoms(np.tile([EPS_O, 0.0, 0.0], n_mol), np.tile([SIGMA_O, 0.1, 0.1], n_mol))
mol = np.arange(N).reshape(-1, 3)                                # {O, H, H} per molecule: the apex first

md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(RC, 0.8), E.cu(atoms, dev), skin=0.1,
                      inv_mass=E.cu(1.0 / mass, dev))
md.set_exclusions_(np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]]))
md.set_coulomb_(np.tile([-0.8476, 0.4238, 0.4238], n_mol), E.COULOMB_K_KJ_NM, eps_rf=78.0)
md.set_rigid3_(mol, np.tile([R_OH, D_HH], (n_mol, 1)))
# the lattice start has molecules at random orientations next to each other: relax it before the first 2 fs step
# (emdee_md_minimize leaves the velocities at zero, so they are loaded again)
res = md.minimize_(500, 500.0, dt_start=0.0002, dt_max=0.002, max_step=0.01)
print("minimised: %d iterations, converged = %s, E_pot %.1f -> %.1f kJ/mol" % (res.iterations, res.converged, res.energy0, res.energy))
md.set_state_(md.state(velocities=False, forces=False)["positions"], E.cu(vel, dev), E.cu(atoms, dev), E.cu(1.0 / mass, dev))
md.set_thermostat_("v-rescale", KB * T, TAU_T, every=EVERY_T, seed=2026)      # n_dof = 0: the library counts


def report(step, npt=False):
    ep, ek, _ = md.totals()
    th = md.thermostat_state()
    line = "step %6d  t = %7.3f ps  T = %6.1f K  E_pot = %10.1f kJ/mol" % (step, step * DT, 2.0 * ek / (th["n_dof"] * KB), ep)
    if npt:
        side = md.box()[1]
        p_mol = np.trace(md.molecular_pressure_tensor()["pressure"]) / 3.0
        line += "  box %.4f nm  P_mol = %8.1f bar" % (side[0], p_mol / BAR)
    else:
        line += "  U + K + E_th = %12.3f kJ/mol" % (ep + ek + th["energy"])
    print(line)


print("%d rigid SPC/E molecules, box %.3f nm, dt = %g fs, reaction field (eps_rf = 78), v-rescale at %g K (tau_t = %g ps), "
      "n_dof = %d = 6 x %d - 3" % (n_mol, L, 1e3 * DT, T, TAU_T, md.thermostat_state()["n_dof"], n_mol))
assert md.thermostat_state()["n_dof"] == 6 * n_mol - 3
report(0)
done = 0
while done < steps:
    n = min(200, steps - done)
    md.step_(n, DT)
    done += n
    report(done)

if npt_steps > 0:
    md.set_molecular_scaling_()                                  # lets the engine with the rigid table take a barostat
    md.set_barostat_("c-rescale", P_REF, BETA, TAU_P, EVERY_P, temperature=KB * T, seed=2027)
    print("NPT: v-rescale with C-rescale at %g bar every %d steps (tau_p = %g ps), coupled to the molecular pressure"
          % (P_REF / BAR, EVERY_P, TAU_P))
    report(steps, npt=True)
    done = 0
    while done < npt_steps:
        n = min(200, npt_steps - done)
        md.step_(n, DT)
        done += n
        report(steps + done, npt=True)
md.close()
