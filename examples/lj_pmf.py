#!/usr/bin/env python3
"""The potential of mean force between two tagged atoms of the Lennard-Jones fluid on one MI355X, by umbrella sampling: an fcc
lattice at rho* = 0.8 is melted under the Langevin thermostat at T* = 1; two neighbouring atoms are tagged as groups 0 and 1 and
emdee_md_set_pull holds their distance near r0 with U = 1/2 k (xi - r0)^2 in a handful of windows.  In every window the on-device
log takes (xi, f) every few steps; no position leaves the device.  Per window the mean distance and the mean bias force are
printed.  In equilibrium the bias force balances the slope of the free energy A(xi) of the distance, dA/dxi = <f>, so the trapezoid
sum of <f> over the mean distances is A, and w(xi) = A(xi) + 2 T ln xi (the Jacobian of a distance) the potential of mean force.

    python examples/lj_pmf.py [--cells 8] [--melt 2000] [--windows 8] [--equil 500] [--steps 4000] [--every 10] [--k 200]

cells^3 fcc cells hold 4 cells^3 atoms.  Reduced units.  Needs the built library (python -c "import __graft_entry__ as g;
g.build()") and a gfx950 device."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=8)
ap.add_argument("--melt", type=int, default=2000)
ap.add_argument("--windows", type=int, default=8)
ap.add_argument("--equil", type=int, default=500)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--k", type=float, default=200.0)
args = ap.parse_args()

E = load_package()
dev = torch.device("cuda", 0)
DT, T = 0.004, 1.0
pos, L = E.synthetic.fcc_positions(args.cells)
N = pos.shape[0]
# the atom nearest the middle of the box and its nearest neighbour: both groups are single atoms, loaded whole by construction
a = int(np.argmin(((pos - 0.5 * L) ** 2).sum(axis=1)))
d = np.sqrt(((pos - pos[a]) ** 2).sum(axis=1))
d[a] = np.inf
b = int(np.argmin(d))
group = np.full(N, -1, dtype=np.int32)
group[a], group[b] = 0, 1
md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N, temperature=T), dev), L, E.LennardJonesModel(2.5, 2.0),
                      E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
md.set_langevin_(2.0, T, seed=2026)
window = lambda r0, **log: md.set_pull_(group, [dict(a=0, b=1, kind="umbrella", geometry="distance", k=args.k, r0=r0)], **log)
window(float(d[b]))                                          # (the pair stays together while the lattice melts)
md.step_(args.melt, DT)
print("# %d atoms, box %.4f sigma, atoms %d and %d tagged, melted for %d steps: T* = %.3f" % (N, L, a, b, args.melt, md.observables()["temperature"]))

print("# r0  <xi>  <f>  samples")
centres, means = [], []
for r0 in np.linspace(1.0, 2.2, args.windows):
    window(float(r0))
    md.step_(args.equil, DT)
    window(float(r0), log_every=args.every, log_capacity=args.steps // args.every)
    md.step_(args.steps, DT)
    log = md.pull_log()                                      # one read per window: (count, 1) arrays of xi and f
    assert log["dropped"] == 0
    centres.append(log["xi"].mean()); means.append(log["f"].mean())
    print("%.4f %.6f %.6f %d" % (r0, centres[-1], means[-1], log["count"]))
xi, f = np.array(centres), np.array(means)
A = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(xi))])
w = A + 2.0 * T * np.log(xi)
print("# xi  w(xi) - w(last)   (the trapezoid sum of <f>, plus 2 T ln xi)")
for r, v in zip(xi, w - w[-1]):
    print("%.6f %.6f" % (r, v))
md.close()
