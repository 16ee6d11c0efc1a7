"""Cost of a global thermostat on the benchmark box, undivided fp64: steps/s of bench.py's fcc box (136^3 cells: 10,061,824 atoms,
rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005, T* = 1) on four loops, alternating on the same build:

    fused        no thermostat: the fused step kernel with merged kicks and run-ahead
    closed       the closed loop with no event in the run (v-rescale with `every` beyond the run): every step closes its half
                 kick -- kick + drift, force pass, kick -- and reads the rebuild word
    v-rescale/1  the closed loop with an event after every step (three launches: K, the scalar update, v <- alpha v)
    v-rescale/10 the closed loop with an event after every tenth step

The target is T* = 1 with tau_t = 1: the lattice start settles near T* = 0.56 on its own, the thermostatted runs are near 0.69
by the end of the 130 steps, and the rebuild count moves by one.  After the timed steps ten more run with profiling on, for the
device time of the events' own launches (emdee_md_kernel_time index 14).  No target: what leaving the fused loop costs a
thermostatted run is a number for the record; if it is large, keeping the fused loop between events is the follow-up.

    python3 profiles/thermostat_cost.py [--steps 100] [--warmup 20] [--cells 136]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()
LOOPS = (("fused", None), ("closed", 10 ** 9), ("v-rescale/1", 1), ("v-rescale/10", 10))


def run(pos, vel, L, atoms, every, steps, warmup, dev, dt=0.005):
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(vel, dev), L, E.LennardJonesModel(2.5, 2.0), E.cu(atoms, dev), skin=0.3)
    if every is not None:
        md.set_thermostat_(E.THERMOSTAT_VRESCALE, 1.0, 1.0, every=every, seed=1)
    md.step_(warmup, dt)
    md.totals()
    torch.cuda.synchronize()
    b0 = md.nbr_stats()["builds"]
    t0 = time.perf_counter()
    md.step_(steps, dt)
    md.needs_rebuild()                                      # (blocking: one word behind everything the call queued)
    sec = time.perf_counter() - t0
    builds = md.nbr_stats()["builds"] - b0
    md.profile_(True)                                       # (the events' own device time, from ten more steps)
    md.step_(10, dt)
    th_ms, th_n = md.kernel_time("thermostat")
    temperature = md.observables()["temperature"]
    md.close()
    return steps / sec, builds, th_ms, th_n, temperature


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cells", type=int, default=136)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pos, L = E.synthetic.fcc_positions(args.cells)
    N = pos.shape[0]
    vel = E.synthetic.velocities(N)
    atoms = E.lennard_jones_atoms(1.0, 1.0, N)
    for name, every in LOOPS + LOOPS:
        sps, builds, th_ms, th_n, temperature = run(pos, vel, L, atoms, every, args.steps, args.warmup, dev)
        print("%8d atoms  %-13s %8.1f steps/s  %.3f ms/step  (%d rebuilds in %d steps; in 10 more steps the thermostat's %d launches take %.3f ms; T* = %.4f)"
              % (N, name, sps, 1e3 / sps, builds, args.steps, th_n, th_ms, temperature), flush=True)


if __name__ == "__main__":
    main()
