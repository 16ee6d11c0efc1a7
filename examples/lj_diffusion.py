#!/usr/bin/env python3
"""The self-diffusion coefficient of the Lennard-Jones fluid on one MI355X, two ways: an fcc lattice at rho* = 0.8 is melted under
the Langevin thermostat at T* = 1, then run on under stochastic velocity rescaling while emdee_md_msd_sample correlates the current
positions and velocities with the time origins kept on the device.  No position leaves the device: the sums are read once, at the
end.  D from the Einstein relation is the slope of the drift-free mean-squared displacement over the second half of the lags,
divided by 6; D from the Green-Kubo relation is the trapezoid integral of the velocity autocorrelation function, divided by 3.

    python examples/lj_diffusion.py [--cells 10] [--melt 2000] [--steps 4000] [--every 5] [--lags 200] [--origin-every 10]

cells^3 fcc cells hold 4 cells^3 atoms; a sample every --every steps, lags up to --lags samples, every --origin-every-th sample a
time origin (at most 64 origins within the lags).  Reduced units.  Needs the built library
(python -c "import __graft_entry__ as g; g.build()") and a gfx950 device."""
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
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--every", type=int, default=5)
ap.add_argument("--lags", type=int, default=200)
ap.add_argument("--origin-every", type=int, default=10)
args = ap.parse_args()

E = load_package()
dev = torch.device("cuda", 0)
DT = 0.004
pos, L = E.synthetic.fcc_positions(args.cells)
N = pos.shape[0]
md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N, temperature=1.0), dev), L, E.LennardJonesModel(2.5, 2.0),
                      E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
md.set_langevin_(2.0, 1.0, seed=2026)
md.step_(args.melt, DT)
md.set_langevin_(0.0, 1.0)
md.set_thermostat_("v-rescale", 1.0, 1.0, seed=2026)
print("# %d atoms, box %.4f sigma, melted for %d steps: T* = %.3f" % (N, L, args.melt, md.observables()["temperature"]))

n_samples = args.steps // args.every
n_lags = max(2, min(args.lags, n_samples // 2))
md.set_msd_(n_lags, origin_every=args.origin_every)
md.msd_sample_()
for _ in range(n_samples):
    md.step_(args.every, DT)
    md.msd_sample_()                                         # queued behind the steps; nothing comes back
out = md.msd()
t = out["lags"] * args.every * DT
msd, vacf = out["msd_drift_free"][:, 0], out["vacf"][:, 0]
half = n_lags // 2
slope = np.polyfit(t[half:], msd[half:], 1)[0]
integral = float(np.sum(0.5 * (vacf[1:] + vacf[:-1]) * np.diff(t)))
print("# %d samples, %d lags of %.3f, %d to %d origins per lag; T* = %.3f"
      % (out["samples"], n_lags, args.every * DT, out["origins"].min(), out["origins"].max(), md.observables()["temperature"]))
print("# t  msd_drift_free  vacf")
for a, b, c in zip(t, msd, vacf):
    print("%.6f %.6f %.6f" % (a, b, c))
print("D Einstein = %.6f" % (slope / 6.0))
print("D Green-Kubo = %.6f" % (integral / 3.0))
md.close()
