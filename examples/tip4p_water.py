#!/usr/bin/env python3
"""TIP4P/2005 water (Abascal & Vega, J. Chem. Phys. 123, 234505 (2005)) with the negative charge on a massless fourth site
(emdee_md_set_vsites): rigid molecules (emdee_md_set_rigid3) on a lattice in random orientations are minimised
(emdee_md_minimize), run at 2 fs under the Langevin thermostat with reaction-field electrostatics, then with particle-mesh Ewald,
then at constant pressure under stochastic cell rescaling on the molecular pressure (emdee_md_set_molecular_scaling).

    python examples/tip4p_water.py [cells] [steps]     # cells^3 molecules (default 6: 216), steps per stage (default 500)

Atoms are ordered O, H, H per molecule, then the M sites.  Units: nm, ps, atomic mass units, kJ/mol, elementary charges, so
pressures are kJ/mol/nm^3 (1 bar = 0.0602214 of them).  Needs the built library
(python -c "import __graft_entry__ as g; g.build()") and a gfx950 device."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

E = load_package()
dev = torch.device("cuda", 0)
cells = int(sys.argv[1]) if len(sys.argv) > 1 else 6
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 500
KB, T, DT, RC, RS, SKIN, SPACING = 0.0083144626, 300.0, 0.002, 0.8, 0.7, 0.1, 0.3107
BAR = 0.0602214
# the model: geometry, the distance of M from O along the bisector, charges, and the one Lennard-Jones centre (on O)
R_OH, THETA, D_OM, Q_H, SIGMA_O, EPS_O = 0.09572, np.deg2rad(104.52), 0.01546, 0.5564, 0.31589, 0.7749
M_O, M_H = 15.9994, 1.008

n = cells ** 3
L = cells * SPACING
if L < 2.0 * (RC + SKIN):
    sys.exit("the box side %.2f nm is below 2 (rc + skin) = %.2f nm: use more cells" % (L, 2.0 * (RC + SKIN)))
rng = np.random.default_rng(2026)
g = (np.arange(cells) + 0.5) * SPACING
centres = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
local = np.array([[0.0, 0.0, 0.0], [R_OH * np.cos(THETA / 2), R_OH * np.sin(THETA / 2), 0.0], [R_OH * np.cos(THETA / 2), -R_OH * np.sin(THETA / 2), 0.0]])
rot = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
real = (centres[:, None, :] + np.einsum("nij,kj->nki", rot, local)).reshape(-1, 3)

mol = np.arange(3 * n).reshape(-1, 3)                            # {O, H, H}
sites = 3 * n + np.arange(n)
d_base = 2.0 * R_OH * np.sin(THETA / 2)
geom = np.tile([R_OH, d_base], (n, 1))
vs_atoms, vs_weights = E.ingest.bisector_sites(sites, mol, R_OH, d_base, D_OM)
N = 4 * n
o, h1, h2 = (real[mol[:, k]] for k in range(3))
# (the set call places the sites itself; loading them near their place keeps the first neighbour list small)
pos = np.concatenate([real, o + vs_weights[:, :1] * (h1 - o) + vs_weights[:, 1:] * (h2 - o)])
inv_mass = np.concatenate([np.tile([1.0 / M_O, 1.0 / M_H, 1.0 / M_H], n), np.zeros(n)])       # a site is loaded with inv_mass = 0
charges = np.concatenate([np.tile([0.0, Q_H, Q_H], n), np.full(n, -2.0 * Q_H)])
atoms = E.lennard_jones_atoms(np.concatenate([np.tile([EPS_O, 0.0, 0.0], n), np.zeros(n)]), np.full(N, SIGMA_O))
four = np.concatenate([mol, sites[:, None]], axis=1)
excl = np.concatenate([four[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])

md = E.VelocityVerlet(E.cu(np.mod(pos, L), dev), E.cu(np.zeros((N, 3)), dev), L, E.LennardJonesModel(RC, RS), E.cu(atoms, dev), skin=SKIN,
                      inv_mass=E.cu(inv_mass, dev))
md.set_exclusions_(excl)
md.set_coulomb_(charges, E.COULOMB_K_KJ_NM, eps_rf=78.0)
md.set_rigid3_(mol, geom)
md.set_vsites_(vs_atoms, vs_weights)
md.set_molecular_scaling_()


def deviations(x, lengths):
    """largest relative error of a rigid distance, and the largest distance of a site from where its parents put it (nm)"""
    ln = np.asarray(lengths)
    mi = lambda d: d - ln * np.rint(d / ln)
    worst = 0.0
    for i, j, want in ((0, 1, R_OH), (0, 2, R_OH), (1, 2, d_base)):
        worst = max(worst, np.abs(np.linalg.norm(mi(x[mol[:, i]] - x[mol[:, j]]), axis=1) / want - 1.0).max())
    o = x[mol[:, 0]]
    m = o + vs_weights[:, :1] * mi(x[mol[:, 1]] - o) + vs_weights[:, 1:] * mi(x[mol[:, 2]] - o)
    return worst, np.abs(mi(x[sites] - m)).max()


print("%d TIP4P/2005 molecules (%d atoms, %d of them sites), box %.3f nm, w_b = w_c = %.6f" % (n, N, n, L, vs_weights[0, 0]))
res = md.minimize_(2000, 100.0, dt_start=0.0002, dt_max=0.002, max_step=0.01)
x = md.state(velocities=False, forces=False)["positions"].cpu().numpy()
print("minimised: %d iterations, converged = %s; E_pot %.1f -> %.1f kJ/mol; largest constrained force %.1f kJ/mol/nm; "
      "rigid distances off by %.1e, sites off by %.1e nm" % ((res.iterations, res.converged, res.energy0, res.energy, res.g_max) + deviations(x, [L] * 3)))

# ---- 2 fs steps (the minimiser left the velocities at zero: draw them for the atoms with mass; the sites' stay 0)
vel = np.zeros((N, 3))
vel[:3 * n] = rng.normal(size=(3 * n, 3)) * np.sqrt(KB * T * inv_mass[:3 * n])[:, None]
md.set_state_(E.cu(x, dev), E.cu(vel, dev), E.cu(atoms, dev), E.cu(inv_mass, dev))
md.set_langevin_(gamma=5.0, temperature=KB * T, seed=2026)
dof = 6 * n - 3                                                  # rigid bodies; the sites have no degrees of freedom


def run(stage):
    done = 0
    while done < steps:
        k = min(100, steps - done)
        md.step_(k, DT)
        done += k
        ep, ek, _ = md.totals()
        lengths = md.box()[1]
        p = np.trace(md.molecular_pressure_tensor()["pressure"]) / 3.0
        x = md.state(velocities=False, forces=False)["positions"].cpu().numpy()
        rigid, site = deviations(x, lengths)
        print("%-14s step %5d  T = %6.1f K  E_pot = %10.1f kJ/mol  P_mol = %8.1f bar  box %.4f nm  rigid %.1e  sites %.1e nm"
              % (stage, done, 2.0 * ek / (dof * KB), ep, p / BAR, lengths[0], rigid, site))
        assert np.isfinite(ep) and rigid < 1e-10 and site < 1e-12


run("reaction field")
md.set_pme_(3.5, 16 if cells <= 8 else 32, 4)                    # alpha rc = 2.8; the real-space terms keep the cutoff
run("PME")
md.set_barostat_("c-rescale", p_ref=1.0 * BAR, compressibility=4.5e-5 / BAR, tau_p=1.0, every=10, temperature=KB * T, seed=2026)
run("PME, C-rescale")
md.close()
