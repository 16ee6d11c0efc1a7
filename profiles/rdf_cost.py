"""Cost of a sample of the radial distribution functions (emdee_md_rdf_sample), undivided fp64: an fcc box of 63^3 cells (1,000,188
atoms, rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a short run, four tables on the same engine:

    r_max 2.5 / 5.0 sigma, 100 bins; one histogram (every atom in one group) or three (two groups, atoms dealt alternately)

Each table is sampled `--samples` times with profiling on: the device time of a sample is emdee_md_kernel_time index 15 over the
samples (count, scan, fill, pair loop).  Next to it the plain force pass of the same engine (index 0, the same number of passes).
--root DIR loads the package from another checkout of the project (the parent commit, built): a checkout without the sampler
prints its force pass alone, which is the parent's force pass on the same box.  No target: a number for the record.

    python3 profiles/rdf_cost.py [--cells 63] [--samples 10] [--root DIR]"""
import argparse
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=63)
ap.add_argument("--samples", type=int, default=10)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()


def main():
    dev = torch.device("cuda", 0)
    pos, L = E.synthetic.fcc_positions(args.cells)
    N = pos.shape[0]
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N), dev), L, E.LennardJonesModel(2.5, 2.0),
                          E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
    md.step_(50, 0.005)                                     # (off the lattice)
    md.profile_(True)
    for _ in range(args.samples):
        md.forces_(E.FORCES)
    ms, n = md.kernel_time("lj_force_nbr")
    print("%8d atoms  force pass                         %8.3f ms  (%d launches in %d passes)" % (N, ms / args.samples, n, args.samples), flush=True)
    if not hasattr(md, "set_rdf_"):
        md.close()
        return
    for r_max in (2.5, 5.0):
        for groups in (None, np.arange(N) % 2):
            md.set_rdf_(r_max, 100, groups)
            md.rdf_sample_()                                # (buffers)
            md.rdf_reset_()
            md.profile_(True)                               # (resets the timers)
            for _ in range(args.samples):
                md.rdf_sample_()
            ms, n = md.kernel_time("rdf")
            out = md.rdf()
            print("%8d atoms  sample r_max %.1f, %d histogram%s  %8.3f ms  (%d launches in %d samples; %.4g pairs per frame; g at r_max %.4f)"
                  % (N, r_max, len(out["pairs"]), " " if len(out["pairs"]) == 1 else "s", ms / args.samples, n, args.samples,
                     out["counts"].sum() / out["frames"], out["g"][0][-1]), flush=True)
    md.close()


if __name__ == "__main__":
    main()
