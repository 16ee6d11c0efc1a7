#!/usr/bin/env python3
"""The shear viscosity and the thermal conductivity of the Lennard-Jones fluid near its triple point (T* = 0.722, rho* = 0.8442) on
one MI355X by the Green-Kubo relations: an fcc lattice at that density is melted under the Langevin thermostat, cooled to T*, then
run on under stochastic velocity rescaling while emdee_md_gk_sample takes the box stress and the heat flux every few steps and
correlates them with the earlier samples kept on the device.  Neither a pressure tensor nor a per-atom virial leaves the device: the
lag sums are read once, at the end.

    eta = V / (kT) int <P_ab(0) P_ab(t)> dt,  averaged over the five independent traceless components of the stress
    lambda = 1 / (V kT^2) int <J_a(0) J_a(t)> dt,  averaged over the three axes

(the sums hold S = P V and J, both extensive, hence 1 / (V kT) and 1 / (V kT^2) in front of them).  The running integrals are
printed; a plateau needs 10^5 - 10^6 samples, a short run is noise around it.

    python examples/lj_viscosity.py [--cells 8] [--melt 3000] [--steps 20000] [--every 4] [--lags 250]

cells^3 fcc cells hold 4 cells^3 atoms; a sample every --every steps, lags up to --lags samples.  Reduced units.  Needs the built
library (python -c "import __graft_entry__ as g; g.build()") and a gfx950 device."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=8)
ap.add_argument("--melt", type=int, default=3000)
ap.add_argument("--steps", type=int, default=20000)
ap.add_argument("--every", type=int, default=4)
ap.add_argument("--lags", type=int, default=250)
args = ap.parse_args()

E = load_package()
dev = torch.device("cuda", 0)
DT, T, RHO = 0.004, 0.722, 0.8442
pos, L = E.synthetic.fcc_positions(args.cells, rho=RHO)
N = pos.shape[0]
md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N, temperature=2.0), dev), L, E.LennardJonesModel(2.5, 2.0),
                      E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
md.set_langevin_(2.0, 2.0, seed=2026)                        # (well above melting first: the lattice must go)
md.step_(args.melt // 2, DT)
md.set_langevin_(2.0, T, seed=2027)
md.step_(args.melt - args.melt // 2, DT)
md.set_langevin_(0.0, T)
md.set_thermostat_("v-rescale", T, 1.0, seed=2026)
print("# %d atoms, box %.4f sigma (rho* = %.4f), melted for %d steps: T* = %.3f" % (N, L, N / L ** 3, args.melt, md.observables()["temperature"]))

n_samples = args.steps // args.every
n_lags = max(2, min(args.lags, n_samples // 2))
md.set_green_kubo_(n_lags)
md.gk_sample_()
for _ in range(n_samples):
    md.step_(args.every, DT)
    md.gk_sample_()                                          # queued behind the steps; nothing comes back
out = md.green_kubo(dt_sample=args.every * DT, temperature=T)
t = out["lags"] * args.every * DT
print("# %d samples, %d lags of %.3f, %d to %d products per lag; T* = %.3f; <p> = %.4f"
      % (out["samples"], n_lags, args.every * DT, out["counts"].min(), out["counts"].max(), md.observables()["temperature"],
         out["totals"][5] / out["samples"] / L ** 3))
print("# t  stress_acf  heat_acf  eta(t)  lambda(t)")
for row in zip(t, out["stress_acf"], out["heat_acf"], out["eta"], out["lambda_"]):
    print("%.6f %.6e %.6e %.6f %.6f" % row)
print("eta = %.6f" % out["eta"][-1])
print("lambda = %.6f" % out["lambda_"][-1])
md.close()
