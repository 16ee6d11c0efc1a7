"""Device time of what emdee_md_minimize adds to the stages of its steps (csrc/minimize.hpp: the constrained force, the reduction,
the mixing; emdee_md_kernel_time index 12) against the force pass of the same call (index 0), and the wall time of an iteration,
which holds the two read-backs per iteration as well.

The box of profiles/hbonds_cost.py: 10^5 rigid three-site molecules (3 x 10^5 atoms) on a 47^3 lattice of spacing 1.25, rc =
2.5, skin = 0.4, in fp64 and fp32, with the rigid table and without any.

Numbers for the record, not gates.

    python3 profiles/minimize_cost.py [--iterations 100] [--groups 100000]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles.hbonds_cost import E, groups  # noqa: E402
from tests.helpers import settle_ref as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--groups", type=int, default=100000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pos, vel, L, mass, atoms, mol = groups(a.groups, np.random.default_rng(2026))
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [0, 2]], mol[:, [1, 2]]])
    for dtype in (np.float64, np.float32):
        for rigid in (True, False):
            md = E.VelocityVerlet(E.cu(pos.astype(dtype), dev), E.cu(vel.astype(dtype), dev), L, E.LennardJonesModel(sr.RC, sr.RS),
                                  E.cu(atoms, dev), skin=sr.SKIN, inv_mass=E.cu((1.0 / mass).astype(dtype), dev))
            md.set_exclusions_(excl)
            if rigid:
                md.set_rigid3_(mol, np.tile([sr.D_LEG, sr.D_BASE], (len(mol), 1)))
            md.minimize_(10, 0.0, dt_start=0.001, dt_max=0.01, max_step=0.05)              # (warm-up)
            md.profile_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = md.minimize_(a.iterations, 0.0, dt_start=0.001, dt_max=0.01, max_step=0.05)
            wall = time.perf_counter() - t0
            ms, _ = md.kernel_time("minimize")
            force_ms, force_n = md.kernel_time("lj_force_nbr")
            settle_ms, _ = md.kernel_time("settle")
            print("%s, %d molecules, %s: minimiser's own kernels %.4f ms/iteration device; force pass %.4f ms (%d launches); ratio %.3f; "
                  "constraint stages %.4f ms/iteration; wall %.4f ms/iteration; %d rebuilds; energy %.1f -> %.1f"
                  % (np.dtype(dtype).name, a.groups, "rigid table" if rigid else "no table", ms / res.iterations, force_ms / force_n, force_n,
                     ms / res.iterations / (force_ms / force_n), settle_ms / res.iterations, 1e3 * wall / res.iterations, res.rebuilds,
                     res.energy0, res.energy), flush=True)
            md.close()


if __name__ == "__main__":
    main()
