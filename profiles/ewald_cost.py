"""Cost of the Ewald sum against the reaction field on the same engine, undivided fp64, through emdee_md_kernel_time:

  force   ms per force pass (index 0: pair loop, 1-4 / bonded / struck-pair terms and, on an Ewald engine, the reciprocal pass)
  recip   ms per reciprocal pass alone (index 8: phase table, structure factors, per-atom pass)

on the water box (synthetic.water_box(n): exclusions, bonds, angles; rc 0.9, rs 0.8, skin 0.1, alpha rc = 3.5, kmax from the
leading factor of the truncation error, as tests/helpers/ewald_ref.py kmax_estimate) and on rock salt (unit grid, charges +-1,
no LJ, rc 3, alpha 1.5, kmax by the same rule) at growing sizes: the direct reciprocal sum is O(N K) with K growing as the
volume, the pair pass O(N), so there is a box above which the reciprocal pass costs more than the pair pass.

    python3 profiles/ewald_cost.py [--passes 20] [--water 8,16,24] [--salt 8,16,24,32,46]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()


def kmax_estimate(alpha, L, rc):
    """the smallest n with exp(-(pi n / (alpha L))^2) <= erfc(alpha rc)"""
    return max(1, min(64, int(math.ceil(alpha * L / math.pi * math.sqrt(-math.log(math.erfc(alpha * rc)))))))


def water(n):
    w = E.synthetic.water_box(n)
    terms = [(E.HARMONIC_BOND, w["bonds"], w["bond_params"]), (E.HARMONIC_ANGLE, w["angles"], w["angle_params"])]
    return dict(name="water", pos=w["positions"], L=w["L"], atoms=w["atoms"], excl=w["exclusions"], terms=terms, q=w["charges"],
                K=E.COULOMB_K_KJ_NM, rc=0.9, rs=0.8, skin=0.1, alpha=3.5 / 0.9)


def salt(cells):
    g = np.arange(cells)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    pos = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float64)
    q = np.where((x + y + z).ravel() % 2 == 0, 1.0, -1.0)
    return dict(name="salt", pos=pos, L=float(cells), atoms=E.lennard_jones_atoms(0.0, 1.0, pos.shape[0]), excl=None, terms=[], q=q,
                K=1.0, rc=3.0, rs=2.5, skin=0.3, alpha=1.5)


def run(box, ewald, passes, dev):
    n = box["pos"].shape[0]
    md = E.VelocityVerlet(E.cu(box["pos"], dev), E.cu(np.zeros((n, 3)), dev), box["L"], E.LennardJonesModel(box["rc"], box["rs"]),
                          E.cu(box["atoms"], dev), skin=box["skin"])
    if box["excl"] is not None:
        md.set_exclusions_(box["excl"])
    for kind, a, p in box["terms"]:
        md.set_bonded_(kind, a, p)
    md.set_coulomb_(box["q"], box["K"], float("inf"))
    kmax = kmax_estimate(box["alpha"], box["L"], box["rc"])
    if ewald:
        md.set_ewald_(box["alpha"], kmax)
    md.forces_()
    torch.cuda.synchronize()
    md.profile_(True)
    for _ in range(passes):
        md.forces_()
    force_ms, force_n = md.kernel_time("lj_force_nbr")
    recip_ms, recip_n = md.kernel_time("ewald_reciprocal")
    md.close()
    return force_ms / max(force_n, 1), recip_ms / max(recip_n, 1), kmax


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
            rf, _, _ = run(box, False, args.passes, dev)
            ew, recip, kmax = run(box, True, args.passes, dev)
            print("%-6s %8d atoms  L %7.3f  kmax %2d  force pass: reaction field %8.3f ms, Ewald %8.3f ms, of which reciprocal %8.3f ms"
                  % (box["name"], box["pos"].shape[0], box["L"], kmax, rf, ew, recip), flush=True)


if __name__ == "__main__":
    main()
