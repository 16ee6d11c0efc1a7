"""Cost of a sample of the displacement and velocity correlations (emdee_md_msd_sample), undivided fp64, EMDEE_MSD | EMDEE_VACF: an
fcc box of 63^3 cells (1,000,188 atoms, rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a short run, every atom
in one group, two tables on the same engine:

    1 live origin  (n_lags = 1, origin_every = 1: every sample is an origin and meets itself alone)
    16 live origins (n_lags = 16, origin_every = 1, measured once the ring is full)

Each table is sampled `--samples` times with profiling on: the device time of a sample is emdee_md_kernel_time index 16 over the
samples (gather, accumulate, finish; HIP events around every launch).  Next to it the algorithmic bytes of a sample -- the gather
reads a record, an image word, a permutation entry, a table entry and three velocities per atom (68 bytes) and writes 48; the
accumulate reads (1 + live) snapshots of 48 bytes per atom -- and the yardstick: the device time of one device-to-device copy
(hipMemcpyAsync) of a buffer of that many bytes in the same run, which moves twice that traffic (every byte read and written).
No target: a number for the record.

    python3 profiles/msd_cost.py [--cells 63] [--samples 20]"""
import argparse
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=63)
ap.add_argument("--samples", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()


def copy_ms(nbytes, rounds):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.zero_()
    dst.copy_(src)                                          # (touched once)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(rounds):
        start.record()
        dst.copy_(src)
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return times[len(times) // 2]


def main():
    dev = torch.device("cuda", 0)
    pos, L = E.synthetic.fcc_positions(args.cells)
    N = pos.shape[0]
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N), dev), L, E.LennardJonesModel(2.5, 2.0),
                          E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
    md.step_(50, 0.005)                                     # (off the lattice)
    for live, n_lags in ((1, 1), (16, 16)):
        md.set_msd_(n_lags, origin_every=1)
        for _ in range(n_lags + 2):                         # (buffers; the ring full)
            md.msd_sample_()
        md.profile_(True)                                   # (resets the timers)
        for _ in range(args.samples):
            md.msd_sample_()
        ms, n = md.kernel_time("msd")
        md.profile_(False)
        out = md.msd()
        assert out["origins"][n_lags - 1] >= args.samples
        per = ms / args.samples
        nbytes = N * (68 + 48) + (1 + live) * 48 * N
        yard = copy_ms(nbytes, args.samples)
        print("%8d atoms  %2d live origin%s  %8.4f ms a sample (%d launches in %d samples)  %7.1f MB algorithmic, %6.0f GB/s;  a copy of "
              "%.1f MB: %8.4f ms (%6.0f GB/s read + written);  sample / copy %.2f"
              % (N, live, " " if live == 1 else "s", per, n, args.samples, nbytes / 1e6, nbytes / per / 1e6, nbytes / 1e6, yard,
                 2.0 * nbytes / yard / 1e6, per / yard), flush=True)
    md.close()


if __name__ == "__main__":
    main()
