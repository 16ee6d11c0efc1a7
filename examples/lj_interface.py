#!/usr/bin/env python3
"""The liquid-vapour interface of the Lennard-Jones fluid on one MI355X: a slab of fcc cells at rho* = 0.8 in a periodic box three
times as long along z is held at T* under stochastic velocity rescaling while emdee_md_spatial_sample adds the current state to
on-device profiles along z every few steps.  No position, velocity or per-atom tensor leaves the device: the profiles are read
once, at the end.  Printed: rho(z), P_N - P_T, and the surface tension gamma = gamma_sum / 2 (the slab has two interfaces); beside
it the box value L_z / 2 (P_zz - (P_xx + P_yy) / 2) from pressure_tensor() of the last frame alone.

    python examples/lj_interface.py [--cells 8] [--temperature 0.8] [--equilibrate 4000] [--steps 4000] [--every 10] [--bins 120]

The slab is cells x cells x cells fcc cells (4 cells^3 atoms), the box cells x cells x 3 cells.  The profiles bin the per-atom
split of the tensor pass (half of every pair term to each partner), not the Irving-Kirkwood contour: their integral across an
interface is the same.  It only prints: with the cutoff at 2.5 sigma and no tail correction gamma is well below the full
potential's.  Reduced units.  Needs the built library (python -c "import __graft_entry__ as g; g.build()") and a gfx950 device."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=8)
ap.add_argument("--temperature", type=float, default=0.8)
ap.add_argument("--equilibrate", type=int, default=4000)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--bins", type=int, default=120)
args = ap.parse_args()

E = load_package()
dev = torch.device("cuda", 0)
DT = 0.004
pos, L = E.synthetic.fcc_positions(args.cells)
N = pos.shape[0]
lengths = [L, L, 3.0 * L]
pos = pos + np.array([0.0, 0.0, L])                         # the slab in the middle third of the box
md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N, temperature=args.temperature), dev), L, E.LennardJonesModel(2.5, 2.0),
                      E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3, lengths=lengths, periodic=[1, 1, 1])
md.set_thermostat_("v-rescale", temperature=args.temperature, tau_t=0.5, seed=2026)
md.step_(args.equilibrate, DT)
print("# %d atoms, box %.4f x %.4f x %.4f sigma, equilibrated for %d steps: T* = %.3f"
      % (N, lengths[0], lengths[1], lengths[2], args.equilibrate, md.observables()["temperature"]))

md.set_spatial_("z", args.bins)
for _ in range(args.steps // args.every):
    md.step_(args.every, DT)
    md.spatial_sample_()                                     # queued behind the steps; nothing comes back
out = md.spatial()
p = md.pressure_tensor()["pressure"]
print("# %d frames; T* = %.3f" % (out["frames"], md.observables()["temperature"]))
print("# z  rho(z)  P_N - P_T  kinetic energy per atom")
for z, rho, pn, pt, k in zip(out["centres"], out["number_density"][0], out["p_normal"][0], out["p_tangential"][0], out["kinetic_energy"][0]):
    print("%.6f %.6f %.6f %.6f" % (z, rho, pn - pt, k))
print("# gamma = gamma_sum / 2 = %.6f  (the profiles, %d frames)" % (0.5 * out["gamma_sum"][0], out["frames"]))
print("# L_z / 2 (P_zz - (P_xx + P_yy) / 2) = %.6f  (pressure_tensor() of the last frame)" % (0.5 * lengths[2] * (p[2, 2] - 0.5 * (p[0, 0] + p[1, 1]))))
md.close()
