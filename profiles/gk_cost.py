"""Cost of a sample of the Green-Kubo observables (emdee_md_gk_sample), undivided fp64, EMDEE_GK_STRESS | EMDEE_GK_HEAT: an fcc box
of 63^3 cells (1,000,188 atoms, rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a short run, n_lags = 1000 with
the ring full.  Between two samples the engine takes one step, so that every sample triggers its tensor pass, as in a run.  With
profiling on (HIP events around every launch), over `--samples` samples:

    the launches a sample adds           emdee_md_kernel_time index 17: the box sums (2), the heat sums (2), push, correlate
    the tensor pass it triggers          the tensor pass of the same box, timed alone: index 0 over emdee_md_pressure_tensor calls,
                                         each behind one step, whose own force pass (the line below) is subtracted
    one plain force pass, the yardstick  index 0 over single steps: the one force pass each of them ends with

The algorithmic bytes of the added launches: the box sums read a permutation entry, six tensor words, three velocities and an
inverse mass per atom (4 + 10 x 8 = 84 bytes at fp64; the engine keeps masses only when it was given them), the heat sums the same
and the energy (92); the rest is scalar work.  No target: a number for the record.

    python3 profiles/gk_cost.py [--cells 63] [--samples 20] [--lags 1000]"""
import argparse
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=63)
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--lags", type=int, default=1000)
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
    md.set_green_kubo_(args.lags)
    for _ in range(args.lags + 2):                          # (buffers; the ring full: every sample meets n_lags earlier ones)
        md.gk_sample_()

    def timed(index, each):
        """device ms per call of `each` under timer `index`, one step between two calls"""
        md.profile_(True)                                   # (resets the timers)
        for _ in range(args.samples):
            md.step_(1, DT)
            each()
        ms, n = md.kernel_time(index)
        md.profile_(False)
        return ms / args.samples, n

    gk_ms, gk_n = timed("green_kubo", md.gk_sample_)
    # index 0 counts every force-kernel launch: the step's own pass, and the tensor pass behind it
    both_ms, _ = timed(0, md.tensor_sums)
    step_ms, _ = timed(0, lambda: None)
    tensor_ms = both_ms - step_ms
    assert md.green_kubo()["samples"] == args.lags + 2 + args.samples
    nbytes = N * (84 + 92)
    print("%8d atoms, n_lags %d, %d samples: added launches %8.4f ms a sample (%d launches, %d a sample; %.1f MB algorithmic, %.0f GB/s);  "
          "tensor pass %8.4f ms;  plain force pass %8.4f ms;  added / tensor pass %.3f, added / force pass %.3f"
          % (N, args.lags, args.samples, gk_ms, gk_n, gk_n // args.samples, nbytes / 1e6, nbytes / gk_ms / 1e6, tensor_ms, step_ms,
             gk_ms / tensor_ms, gk_ms / step_ms), flush=True)
    md.close()


if __name__ == "__main__":
    main()
