"""Cost of the soft-core alchemical decoupling (emdee_md_set_alchemical), undivided fp64: an fcc box of 63^3 cells (1,000,188 atoms,
rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a short run.  Three solutes -- 1 atom, 22 atoms (a small
molecule's worth) and 1024 atoms, each a compact blob around the middle of the box -- at lambda = 0.5, alpha = 0.5.  With profiling on
(HIP events around every launch), over `--steps` single steps:

    the launches behind a force pass     emdee_md_kernel_time index 20 over steps without a rebuild (rebuild_every far away): the
                                         force kernel over the owners of struck entries, the two stages of the sums, the words
    the row pass per rebuild             index 20 over steps that rebuild every time (rebuild_every = 1), minus the above: count,
                                         scan, the read-back's launch, fill
    one plain force pass and rebuild     indices 0 and 2 over the same steps of the same engine with the table cleared

The row pass visits every row twice (count and fill) whatever the solute's size: its cost is that of two exclusion filters plus a
scan over 3 N integers.  The launches behind a force pass scale with the struck entries.  No target: numbers for the record.

    python3 profiles/alchemical_cost.py [--cells 63] [--steps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=63)
ap.add_argument("--steps", type=int, default=20)
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

    def timed(index, rebuild_every):
        """device ms per single step under timer `index`, and its timed entries"""
        md.profile_(True)                                   # (resets the timers)
        for _ in range(args.steps):
            md.step_(1, DT, rebuild_every)
        ms, n = md.kernel_time(index)
        md.profile_(False)
        return ms / args.steps, n

    rows = []
    for size in (1, 22, 1024):
        flag = np.zeros(N, dtype=np.int32)
        flag[nearest[:size]] = 1
        md.set_alchemical_(flag, lam=0.5, alpha=0.5)
        md.step_(2, DT)                                     # (buffers)
        pairs = md.alchemical()["pairs"]
        force_ms, n_force = timed("alchemical", 1 << 30)
        both_ms, n_both = timed("alchemical", 1)
        rows.append((size, pairs, force_ms, n_force, both_ms - force_ms, n_both))
    md.set_alchemical_(None)
    md.step_(2, DT)
    plain_ms, _ = timed(0, 1)
    rebuild_ms, _ = timed(2, 1)
    for size, pairs, force_ms, n_force, row_ms, n_both in rows:
        print("%8d atoms, solute of %4d (%7d cross pairs inside rc): launches behind a force pass %8.4f ms (%d timed entries over %d "
              "steps);  row pass %8.4f ms a rebuild (%d entries);  plain force pass %8.4f ms, plain rebuild %8.4f ms;  added / force "
              "pass %.3f, row pass / rebuild %.3f" % (N, size, pairs, force_ms, n_force, args.steps, row_ms, n_both, plain_ms, rebuild_ms,
                                                      force_ms / plain_ms, row_ms / rebuild_ms), flush=True)
    md.close()


if __name__ == "__main__":
    main()
