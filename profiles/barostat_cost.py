"""Cost of pressure coupling on the headline-sized box, undivided fp64: ms/step of a 1,000,188-atom fcc box (63^3 cells,
rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) with coupling off (the fused step kernel with merged kicks and
run-ahead) and with Berendsen coupling every 10 steps (every step closes its half kick: kick + drift, force pass, kick; every
event adds the box sums, the scale pass, a re-plan and a rebuild), the two forms alternating on the same build.  The
compressibility is small enough that the box moves by 1e-4 per event at most: the populations, and so the cost of a step,
stay those of the uncoupled run.

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 profiles/barostat_cost.py`
and read the k_brick / k_kick_drift / k_kick / k_cell_state_scale rows of the stats file.

    python3 profiles/barostat_cost.py [--steps 200] [--warmup 40] [--cells 63] [--every 10]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()


def box(ncell):
    pos, gid, lengths = E.synthetic.fcc_block((ncell,) * 3, (0, 0, 0), (ncell,) * 3)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    vel = E.synthetic.raw_normals(np.arange(N), N)
    vel -= vel.mean(axis=0)
    vel *= np.sqrt(0.8 * (3 * N - 3) / np.sum(vel * vel))
    return pos, vel, float(lengths[0]), E.lennard_jones_atoms(1.0, 1.0, N)


def run(pos, vel, L, atoms, coupled, steps, warmup, every, dev, dt=0.005):
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(2.5, 2.0), E.cu(atoms, dev), skin=0.3)
    if coupled:
        md.set_barostat_(E.BAROSTAT_BERENDSEN, md.observables()["pressure"], 1e-3, tau_p=1.0, every=every)
    md.step_(warmup, dt)
    torch.cuda.synchronize()
    b0 = md.nbr_stats()["builds"]
    t0 = time.perf_counter()
    md.step_(steps, dt)
    md.totals()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    builds = md.nbr_stats()["builds"] - b0
    side = md.box()[1][0]
    md.close()
    return ms, builds, side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--cells", type=int, default=63)
    ap.add_argument("--every", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pos, vel, L, atoms = box(args.cells)
    for coupled in (False, True, False, True):
        ms, builds, side = run(pos, vel, L, atoms, coupled, args.steps, args.warmup, args.every, dev)
        print("%7d atoms  %-22s %.3f ms/step  (%d rebuilds in %d steps, side %.6f -> %.6f)" % (
            pos.shape[0], "berendsen every %d" % args.every if coupled else "coupling off", ms, builds, args.steps, L, side), flush=True)


if __name__ == "__main__":
    main()
