"""Cost of the launch the position restraints add to a force pass (emdee_md_set_restraints), undivided fp64: an fcc box of 63^3 cells
(1,000,188 atoms, rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) after a short run, harmonic tables of 1 % of the atoms
(every hundredth id: a scattered solute) and of all atoms, in the caller's order.  With profiling on (HIP events around every
launch), over `--steps` single steps:

    the added launch per force pass      emdee_md_kernel_time index 18 (k_restraints, one thread per table entry)
    one plain force pass, the yardstick  index 0 over single steps of the same engine before any table is set
    a device-to-device copy              hipMemcpyAsync of a buffer of the launch's algorithmic bytes in the same run, which moves
                                         twice that traffic (every byte read and written)

The algorithmic bytes of the launch under the FORCES mask: per entry an id (4), three references, three constants and a radius
(56), the slot from inv_perm (4), the record (32 at fp64), the image word (4), and three force words read and written (48): 148
bytes.  The table is read in order; the slot, the record, the image word and the force planes are reached through inv_perm, which
after a sort by cells scatters the caller's order over the planes.  No target: numbers for the record.

    python3 profiles/restraint_cost.py [--cells 63] [--steps 20]"""
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
BYTES_PER_ENTRY = 4 + 56 + 4 + 32 + 4 + 48


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
    md.step_(50, DT)                                        # (off the lattice)

    def timed(index):
        """device ms per force pass under timer `index` over single steps (each ends with one force pass)"""
        md.profile_(True)                                   # (resets the timers)
        for _ in range(args.steps):
            md.step_(1, DT)
        ms, n = md.kernel_time(index)
        passes = md.kernel_time(0)[1]
        md.profile_(False)
        return ms / max(passes, 1), n, passes

    plain_ms, _, _ = timed(0)
    for name, ids in (("1 % of the atoms", np.arange(0, N, 100)), ("all atoms", np.arange(N))):
        md.set_restraints_(ids, 5.0)                        # (the current positions: the atoms stay where the fluid has them)
        md.step_(2, DT)
        ms, n, passes = timed("restraints")
        with_ms, _, _ = timed(0)                            # (index 0 spans the pass and the terms behind it)
        nbytes = len(ids) * BYTES_PER_ENTRY
        yard = copy_ms(nbytes, args.steps)
        print("%8d atoms, table of %s (%d entries): added launch %8.4f ms a force pass (%d launches in %d passes; %.1f MB algorithmic, "
              "%.0f GB/s);  plain force pass %8.4f ms (with the table %8.4f ms);  a copy of %.1f MB: %8.4f ms (%.0f GB/s read + written);  "
              "added / force pass %.3f, added / copy %.2f"
              % (N, name, len(ids), ms, n, passes, nbytes / 1e6, nbytes / ms / 1e6, plain_ms, with_ms, nbytes / 1e6, yard,
                 2.0 * nbytes / yard / 1e6, ms / plain_ms, ms / yard), flush=True)
        md.set_restraints_(None, 0.0)
    md.close()


if __name__ == "__main__":
    main()
