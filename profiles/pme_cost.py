"""Cost of the reciprocal-space pass of the Ewald sum, direct sum against particle mesh, on the boxes of profiles/ewald_cost.py
(undivided, fp64), through emdee_md_kernel_time:

  rf      ms per force pass of the engine under the reaction field (index 0), for scale
  direct  ms per reciprocal pass of the direct sum (index 8; kmax by the rule of ewald_cost.py, at most 64)
  pme     ms per reciprocal pass of the mesh (index 8): order 4, per axis the smallest power of two K in [8, 256] with a spacing
          L / K of at most 1 / (3 alpha) -- the spacing at which tests/test_pme_host.py measures an rms force error of 9e-4 of the
          rms force at order 4 (alpha 1.5, 32^3 points on a 7 x 8 x 9.5 box).  The direct sum is cut at erfc(alpha rc), far below
          that: the two columns are what each method costs at its customary setting, not at equal accuracy.

These are passes of emdee_md_forces with EMDEE_FORCES: the forces-only mesh pass, one forward and one inverse transform.

    python3 profiles/pme_cost.py [--passes 20] [--water 8,16,24] [--salt 8,16,24,32,46]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ewald_cost import E, kmax_estimate, salt, water  # noqa: E402


def mesh(alpha, L):
    """the smallest power of two in [8, 256] with L / K <= 1 / (3 alpha)"""
    K = 8
    while K < 256 and L / K > 1.0 / (3.0 * alpha):
        K *= 2
    return K


def run(box, mode, passes, dev):
    n = box["pos"].shape[0]
    md = E.VelocityVerlet(E.cu(box["pos"], dev), E.cu(np.zeros((n, 3)), dev), box["L"], E.LennardJonesModel(box["rc"], box["rs"]),
                          E.cu(box["atoms"], dev), skin=box["skin"])
    if box["excl"] is not None:
        md.set_exclusions_(box["excl"])
    for kind, a, p in box["terms"]:
        md.set_bonded_(kind, a, p)
    md.set_coulomb_(box["q"], box["K"], float("inf"))
    if mode == "direct":
        md.set_ewald_(box["alpha"], kmax_estimate(box["alpha"], box["L"], box["rc"]))
    elif mode == "pme":
        md.set_pme_(box["alpha"], mesh(box["alpha"], box["L"]), 4)
    md.forces_()
    torch.cuda.synchronize()
    md.profile_(True)
    for _ in range(passes):
        md.forces_()
    force_ms, force_n = md.kernel_time("lj_force_nbr")
    recip_ms, recip_n = md.kernel_time("ewald_reciprocal")
    md.close()
    return force_ms / max(force_n, 1), recip_ms / max(recip_n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--water", default="8,16,24")
    ap.add_argument("--salt", default="8,16,24,32,46")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for make, sizes in ((water, args.water), (salt, args.salt)):
        for size in [int(s) for s in sizes.split(",") if s]:
            box = make(size)
            rf, _ = run(box, "rf", args.passes, dev)
            _, direct = run(box, "direct", args.passes, dev)
            _, pme = run(box, "pme", args.passes, dev)
            print("%-6s %8d atoms  L %7.3f  kmax %2d  mesh %3d^3  reaction-field force pass %8.3f ms  reciprocal pass: direct %9.3f ms, PME %8.3f ms"
                  % (box["name"], box["pos"].shape[0], box["L"], kmax_estimate(box["alpha"], box["L"], box["rc"]),
                     mesh(box["alpha"], box["L"]), rf, direct, pme), flush=True)


if __name__ == "__main__":
    main()
