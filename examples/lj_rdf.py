#!/usr/bin/env python3
"""The radial distribution function of the Lennard-Jones fluid on one MI355X: an fcc lattice at rho* = 0.8 is melted under the
Langevin thermostat at T* = 1, then run on in NVE while emdee_md_rdf_sample adds the current positions to an on-device pair
histogram every 20 steps.  No position leaves the device: the histogram is read once, at the end, and g(r) and the running
coordination number are printed.

    python examples/lj_rdf.py [--cells 10] [--melt 2000] [--steps 2000] [--every 20] [--bins 100] [--r-max R] [--dump FILE]

cells^3 fcc cells hold 4 cells^3 atoms; r_max defaults to half the box side, at most 5 sigma.  --dump writes the sampled frames
(positions in caller order) to an .npz file, for a comparison with a host loop over all pairs.  Reduced units.  Needs the built
library (python -c "import __graft_entry__ as g; g.build()") and a gfx950 device."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=10)
ap.add_argument("--melt", type=int, default=2000)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--every", type=int, default=20)
ap.add_argument("--bins", type=int, default=100)
ap.add_argument("--r-max", type=float, default=None)
ap.add_argument("--dump", default=None)
args = ap.parse_args()

E = load_package()
dev = torch.device("cuda", 0)
DT = 0.004
pos, L = E.synthetic.fcc_positions(args.cells)
N = pos.shape[0]
r_max = min(0.5 * L, 5.0) if args.r_max is None else args.r_max
md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N, temperature=1.0), dev), L, E.LennardJonesModel(2.5, 2.0),
                      E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
md.set_langevin_(2.0, 1.0, seed=2026)
md.step_(args.melt, DT)
md.set_langevin_(0.0, 1.0)
print("# %d atoms, box %.4f sigma, melted for %d steps: T* = %.3f" % (N, L, args.melt, md.observables()["temperature"]))

md.set_rdf_(r_max, args.bins)
frames = []
for _ in range(args.steps // args.every):
    md.step_(args.every, DT)
    md.rdf_sample_()                                         # queued behind the steps; nothing comes back
    if args.dump:
        frames.append(md.state(velocities=False, forces=False)["positions"].cpu().numpy())
out = md.rdf()
print("# %d frames, %d pairs counted up to r_max = %.4f; T* = %.3f" % (out["frames"], out["counts"].sum(), r_max, md.observables()["temperature"]))
print("# r  g(r)  coordination")
for r, g, c in zip(out["r"], out["g"][0], out["coordination"][0]):
    print("%.6f %.6f %.6f" % (r, g, c))
if args.dump:
    np.savez(args.dump, frames=np.array(frames), L=L, r_max=r_max, n_bins=args.bins)
md.close()
