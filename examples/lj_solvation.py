#!/usr/bin/env python3
"""The Lennard-Jones stage of a solvation free energy on one MI355X, by thermodynamic integration: an fcc lattice at rho* = 0.8 is
melted under stochastic velocity rescaling at T* = 1; one atom is tagged as the solute and emdee_md_set_alchemical decouples it from
the rest of the fluid along lambda through the soft core U = lambda 4 eps (D^-2 - D^-1), D = alpha (1 - lambda) + (r / sigma)^6.  In
every window the on-device log takes dU/dlambda, U_alch and U_alch at the two neighbouring lambdas every few steps; no position leaves
the device.  Per window the mean dU/dlambda is printed, then the trapezoid sum over the schedule -- the free energy of coupling the
atom, A(1) - A(0), the excess chemical potential of the fluid at this state point -- and, per pair of neighbouring windows, the mean foreign-energy differences
<U(lambda') - U(lambda)> in both directions, which is what a BAR estimate of the same difference takes.

    python examples/lj_solvation.py [--cells 8] [--melt 2000] [--windows 11] [--equil 500] [--steps 4000] [--every 10] [--alpha 0.5]

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
ap.add_argument("--windows", type=int, default=11)
ap.add_argument("--equil", type=int, default=500)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--alpha", type=float, default=0.5)
args = ap.parse_args()

E = load_package()
dev = torch.device("cuda", 0)
DT, T = 0.004, 1.0
pos, L = E.synthetic.fcc_positions(args.cells)
N = pos.shape[0]
flag = np.zeros(N, dtype=np.int32)
flag[int(np.argmin(((pos - 0.5 * L) ** 2).sum(axis=1)))] = 1       # the solute: the atom nearest the middle of the box
md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N, temperature=T), dev), L, E.LennardJonesModel(2.5, 2.0),
                      E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
md.set_thermostat_("v-rescale", temperature=T, tau_t=0.1, seed=2026)
md.step_(args.melt, DT)
print("# %d atoms, box %.4f sigma, atom %d tagged, melted for %d steps: T* = %.3f" % (N, L, int(flag.argmax()), args.melt,
                                                                                    md.observables()["temperature"]))

lams = np.linspace(1.0, 0.0, args.windows)                         # from the coupled atom down: every window starts equilibrated nearby
print("# lambda  <dU/dlambda>  <U_alch>  samples")
means, up, down = [], [], []
for w, lam in enumerate(lams):
    near = [float(lams[max(w - 1, 0)]), float(lams[min(w + 1, len(lams) - 1)])]
    md.set_alchemical_(flag, lam=float(lam), alpha=args.alpha)
    md.step_(args.equil, DT)
    md.set_alchemical_(flag, lam=float(lam), alpha=args.alpha, foreign=near, log_every=args.every, log_capacity=args.steps // args.every)
    md.step_(args.steps, DT)
    log = md.alchemical_log()                                      # one read per window
    assert log["dropped"] == 0
    means.append(log["dUdl"].mean())
    up.append((log["foreign"][:, 0] - log["U"]).mean())           # towards the previous window of the schedule
    down.append((log["foreign"][:, 1] - log["U"]).mean())         # towards the next
    print("%.4f %.6f %.6f %d" % (lam, means[-1], log["U"].mean(), log["count"]))
order = np.argsort(lams)
x, y = lams[order], np.array(means)[order]
print("# A(1) - A(0) by the trapezoid rule over <dU/dlambda>")
print("%.6f" % float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x))))
print("# lambda -> lambda'  <U(lambda') - U(lambda)>_lambda  <U(lambda) - U(lambda')>_lambda'   (what a BAR estimate takes)")
for w in range(len(lams) - 1):
    print("%.4f %.4f %.6f %.6f" % (lams[w], lams[w + 1], down[w], up[w + 1]))
md.close()
