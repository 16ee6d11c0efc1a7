"""Cost of a sample of the spatial profiles (emdee_md_spatial_sample), undivided fp64: an fcc box of 63^3 cells (1,000,188 atoms,
rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a short run, planar bins along z, eight tables on the same engine:

    EMDEE_SPATIAL_DENSITY alone, and all three bits;  64 and 4096 bins;  one group, and eight groups (atoms dealt round by id)

Each table is sampled `--samples` times with profiling on: the device time of a sample is emdee_md_kernel_time index 21 over the
samples (gather, accumulate, finish; HIP events around every launch; the tensor pass of a STRESS sample is index 0's and is not in
it -- the state does not move between the samples, so it runs once).  Next to it one plain force pass of the same run (index 0), the
algorithmic bytes of the gather -- per atom a record (32), an image word, a permutation entry and a table entry (12), and per mask bit
the planes it reads: the inverse mass (8; DENSITY or KINETIC), three velocities (24; KINETIC), the energy and six tensor words (56;
STRESS); written: the bin (4) and 8 bytes per word of the mask (2, 5, 3) -- and the yardstick: the device time of one
device-to-device copy (hipMemcpyAsync) of a buffer of that many bytes in the same run, which moves twice that traffic (every byte
read and written).  No target: a number for the record.

    python3 profiles/spatial_cost.py [--cells 63] [--samples 20]"""
import argparse
import os
import sys

import numpy as np
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


def gather_bytes(n, density, kinetic, stress):
    read = 32 + 12 + (8 if density or kinetic else 0) + (24 if kinetic else 0) + (56 if stress else 0)
    words = (2 if density else 0) + (5 if kinetic else 0) + (3 if stress else 0)
    return n * (read + 4 + 8 * words)


def main():
    dev = torch.device("cuda", 0)
    pos, L = E.synthetic.fcc_positions(args.cells)
    N = pos.shape[0]
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(E.synthetic.velocities(N), dev), L, E.LennardJonesModel(2.5, 2.0),
                          E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), skin=0.3)
    md.step_(50, 0.005)                                     # (off the lattice)
    md.profile_(True)
    for _ in range(args.samples):
        md.forces_(1)
    force_ms, k = md.kernel_time(0)
    force_ms /= max(k, 1)
    md.profile_(False)
    print("%d atoms; one plain force pass: %.4f ms" % (N, force_ms), flush=True)
    eight = np.arange(N) % 8
    for all_bits in (False, True):
        for n_bins in (64, 4096):
            for groups, n_groups in ((None, 1), (eight, 8)):
                md.set_spatial_("z", n_bins, groups=groups, n_groups=n_groups, kinetic=all_bits, stress=all_bits)
                for _ in range(2):                          # (buffers; the tensor pass of a STRESS table)
                    md.spatial_sample_()
                md.profile_(True)                           # (resets the timers)
                for _ in range(args.samples):
                    md.spatial_sample_()
                ms, n = md.kernel_time("spatial")
                md.profile_(False)
                out = md.spatial()
                assert out["frames"] == args.samples + 2 and out["counts"].sum() == N * out["frames"]
                per = ms / args.samples
                nbytes = gather_bytes(N, True, all_bits, all_bits)
                yard = copy_ms(nbytes, args.samples)
                print("%-22s %4d bins  %d group%s  %8.4f ms a sample (%d launches in %d samples; %.2f of a force pass)  gather %6.1f MB "
                      "algorithmic;  a copy of that: %8.4f ms (%6.0f GB/s read + written);  sample / copy %.2f"
                      % ("DENSITY|KINETIC|STRESS" if all_bits else "DENSITY", n_bins, n_groups, " " if n_groups == 1 else "s", per, n,
                         args.samples, per / force_ms, nbytes / 1e6, yard, 2.0 * nbytes / yard / 1e6, per / yard), flush=True)
    md.close()


if __name__ == "__main__":
    main()
