"""Cost of the Coulomb stage of the alchemical table (emdee_md_set_alchemical_coulomb), undivided fp64: the box of
profiles/alchemical_cost.py -- 63^3 fcc cells (1,000,188 atoms, rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a
short run -- with every atom charged +-0.2 on the reaction field (eps_rf = inf).  Three solutes -- 1 atom, 22 atoms and 1024 atoms,
each a compact blob around the middle of the box -- at lambda = 0.5, alpha = 0.5.  With profiling on (HIP events around every launch),
over `--steps` single steps without a rebuild (rebuild_every far away), emdee_md_kernel_time index 20 per force pass:

    stage off     the launches of the table alone: the force kernel's instance without the stage, the two stages of the sums, the
                  words.  (The solute's charges are zeroed for this run, as an engine without the stage asks; the launches do not
                  depend on the charges.)  Run on the parent commit with --no-stage-api, this is the parent's number.
    stage on      lambda_q = 0.5, beta = 0.3: the Coulomb instance, and the stage's own sums and words on top
    stage at 0    lambda_q = 0: the planes from the instance without the stage and a second launch for dU/dlambda_q

Index 0 over the same steps is the charged force pass the launches stand next to.  No target: numbers for the record.

    python3 profiles/alchemical_coulomb_cost.py [--cells 63] [--steps 20] [--no-stage-api]"""
import argparse
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=63)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--no-stage-api", action="store_true", help="the stage-off rows alone (a build without the stage)")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()
DT = 0.005


def main():
    dev = torch.device("cuda", 0)
    pos, L = E.synthetic.fcc_positions(args.cells)
    N = pos.shape[0]
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N), dev), L, E.LennardJonesModel(2.5, 2.0),
                          E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
    md.step_(50, DT)                                        # (off the lattice)
    nearest = np.argsort(((pos - 0.5 * L) ** 2).sum(axis=1))
    q = np.where(np.arange(N) % 2 == 0, 0.2, -0.2)
    q[-1] -= q.sum()

    def timed(index):
        """device ms per single step under timer `index`, and its timed entries"""
        md.profile_(True)                                   # (resets the timers)
        for _ in range(args.steps):
            md.step_(1, DT, 1 << 30)
        ms, n = md.kernel_time(index)
        md.profile_(False)
        return ms / args.steps, n

    for size in (1, 22, 1024):
        flag = np.zeros(N, dtype=np.int32)
        flag[nearest[:size]] = 1
        q0 = q.copy()
        q0[flag == 1] = 0.0
        md.set_coulomb_(q0, 1.0)
        md.set_alchemical_(flag, lam=0.5, alpha=0.5)
        md.step_(2, DT)                                     # (buffers)
        pairs = md.alchemical()["pairs"]
        off_ms, n_off = timed("alchemical")
        force_ms, _ = timed(0)
        line = ("%8d atoms, solute of %4d (%7d cross pairs inside rc): stage off %8.4f ms a force pass (%d timed entries over %d steps); "
                "charged force pass %8.4f ms" % (N, size, pairs, off_ms, n_off, args.steps, force_ms))
        if not args.no_stage_api:
            md.set_coulomb_(q, 1.0)
            md.set_alchemical_(flag, lam=0.5, alpha=0.5)
            md.set_alchemical_coulomb_(0.5, 0.3)
            md.step_(2, DT)
            on_ms, n_on = timed("alchemical")
            md.set_lambda_coulomb_(0.0)
            md.step_(2, DT)
            zero_ms, n_zero = timed("alchemical")
            line += (";  stage on %8.4f ms (%d entries), at lambda_q = 0 %8.4f ms (%d entries);  on / off %.3f, added / force pass %.3f"
                     % (on_ms, n_on, zero_ms, n_zero, on_ms / off_ms, (on_ms - off_ms) / force_ms))
        print(line, flush=True)
    md.close()


if __name__ == "__main__":
    main()
