"""Cost of the centre-of-mass pull (emdee_md_set_pull) behind a force pass, undivided fp64: an fcc box of 63^3 cells (1,000,188 atoms,
rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a short run.  Two tables: two solutes of 500 atoms each with one
umbrella between them (the usual use), and every atom in one of eight groups with eight coordinates (the ceiling: every atom is
gathered in the partial sums and written by the apply launch).  With profiling on (HIP events around every launch), over `--steps`
single steps:

    the three launches the table adds    emdee_md_kernel_time index 19: partial sums, finish, apply -- once per force pass
    one plain force pass, the yardstick  index 0 over single steps of the same engine with the table cleared

The algorithmic bytes of the added launches per grouped atom at fp64: the partial sums read an id, a slot, a record (32), an image
word and an inverse mass (52 bytes); the apply launch reads an id, a slot, a group and an inverse mass and reads and writes three
force words (68 bytes); the finish block is scalar work.  No target: a number for the record.

    python3 profiles/pull_cost.py [--cells 63] [--steps 20]"""
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

    def timed(index):
        """device ms per single step under timer `index`, and its launches"""
        md.profile_(True)                                   # (resets the timers)
        for _ in range(args.steps):
            md.step_(1, DT)
        ms, n = md.kernel_time(index)
        md.profile_(False)
        return ms / args.steps, n

    two = np.full(N, -1, dtype=np.int32)
    two[:500], two[N // 2:N // 2 + 500] = 0, 1
    umbrella = [dict(a=0, b=1, kind="umbrella", geometry="distance", k=10.0, r0=0.4 * L, rate=0.01)]
    every = (np.arange(N) % 8).astype(np.int32)
    eight = [dict(a=c, b=(c + 1) % 8, kind="umbrella", geometry="direction", k=10.0, r0=0.0, n=(1.0, 1.0, 0.0)) for c in range(8)]
    rows = []
    for name, group, coords in (("two groups of 500, one coordinate", two, umbrella), ("every atom, eight groups, eight coordinates", every, eight)):
        md.set_pull_(group, coords, log_every=1, log_capacity=args.steps)
        grouped = int((group >= 0).sum())
        md.step_(2, DT)                                     # (buffers)
        ms, n = timed("pull")
        rows.append((name, grouped, ms, n))
    md.set_pull_(None, None)
    md.step_(2, DT)
    step_ms, _ = timed(0)
    for name, grouped, ms, n in rows:
        nbytes = grouped * (52 + 68)
        print("%8d atoms, %s: added launches %8.4f ms a force pass (%d timed entries over %d steps; %.2f MB algorithmic, %.0f GB/s);  "
              "plain force pass %8.4f ms;  added / force pass %.3f"
              % (N, name, ms, n, args.steps, nbytes / 1e6, nbytes / ms / 1e6, step_ms, ms / step_ms), flush=True)
    md.close()


if __name__ == "__main__":
    main()
