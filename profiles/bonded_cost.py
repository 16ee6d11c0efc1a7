"""Cost of the bonded terms, undivided fp64: ms/step of the 1,000,188-atom chain box (fcc 63^3 cells, each cell's four atoms a
chain with bonds 0-1, 1-2, 2-3, angles 0-1-2, 1-2-3 and a two-term torsion 0-1-2-3; 1-2 / 1-3 excluded, 1-4 scaled by 0.5; sigma
units, rc 2.5, rs 2.0, skin 0.3) and of a water box of similar size (synthetic.water_box(69): 985,527 atoms, nm and kJ/mol, real
masses, rc 0.9, rs 0.8, skin 0.1, dt 0.5 fs), each run with its exclusions and 1-4 pairs only, then with the bonded terms too.
For the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python3 profiles/bonded_cost.py` and read the
k_bonded rows of the stats file.

    python3 profiles/bonded_cost.py [--steps 100] [--warmup 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()


def chain_box(ncell=63):
    pos, gid, lengths = E.synthetic.fcc_block((ncell,) * 3, (0, 0, 0), (ncell,) * 3)
    pos = pos[np.argsort(gid)]
    L = float(lengths[0])
    pos = np.mod(pos + 0.75 * L / ncell, L)
    N = pos.shape[0]
    vel = E.synthetic.raw_normals(np.arange(N), N)
    vel -= vel.mean(axis=0)
    vel *= np.sqrt(0.8 * (3 * N - 3) / np.sum(vel * vel))
    mol = np.arange(N).reshape(-1, 4)
    terms = [(E.HARMONIC_BOND, np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]]]), (200.0, 0.95)),
             (E.HARMONIC_ANGLE, np.concatenate([mol[:, [0, 1, 2]], mol[:, [1, 2, 3]]]), (40.0, 1.2)),
             (E.PERIODIC_TORSION, np.concatenate([mol, mol]),
              np.concatenate([np.tile((1.5, 1.0, 0.0), (len(mol), 1)), np.tile((0.6, 3.0, np.pi), (len(mol), 1))]))]
    terms = [(k, a, np.array(np.broadcast_to(np.atleast_2d(p), (len(a), np.atleast_2d(p).shape[1])))) for k, a, p in terms]
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]], mol[:, [0, 2]], mol[:, [1, 3]]])
    return dict(name="chains", pos=pos, vel=vel, L=L, atoms=E.lennard_jones_atoms(1.0, 1.0, N), inv_mass=None, excl=excl,
                p14=mol[:, [0, 3]], terms=terms, rc=2.5, rs=2.0, skin=0.3, dt=0.005)


def water(n=69):
    w = E.synthetic.water_box(n)
    N = w["positions"].shape[0]
    rng = np.random.default_rng(11)
    vel = rng.normal(size=(N, 3)) * np.sqrt(2.494 * w["inv_mass"])[:, None]   # ~300 K in kJ/mol, nm/ps
    terms = [(E.HARMONIC_BOND, w["bonds"], w["bond_params"]), (E.HARMONIC_ANGLE, w["angles"], w["angle_params"])]
    return dict(name="water", pos=w["positions"], vel=vel, L=w["L"], atoms=w["atoms"], inv_mass=w["inv_mass"], excl=w["exclusions"],
                p14=None, terms=terms, rc=0.9, rs=0.8, skin=0.1, dt=0.0005)


def run(box, bonded, steps, warmup, dev):
    md = E.VelocityVerlet(E.cu(box["pos"], dev), E.cu(box["vel"], dev), box["L"], E.LennardJonesModel(box["rc"], box["rs"]),
                          E.cu(box["atoms"], dev), skin=box["skin"],
                          inv_mass=None if box["inv_mass"] is None else E.cu(box["inv_mass"], dev))
    md.set_exclusions_(box["excl"])
    if box["p14"] is not None:
        md.set_pairs14_(box["p14"], 0.5)
    if bonded:
        for kind, a, p in box["terms"]:
            md.set_bonded_(kind, a, p)
    md.step_(warmup, box["dt"])
    torch.cuda.synchronize()
    b0 = md.nbr_stats()["builds"]
    t0 = time.perf_counter()
    md.step_(steps, box["dt"])
    md.totals()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    builds = md.nbr_stats()["builds"] - b0
    md.close()
    return ms, builds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for box in (chain_box(), water()):
        for bonded in (False, True, False, True):
            ms, builds = run(box, bonded, args.steps, args.warmup, dev)
            print("%-6s %7d atoms  %-22s %.3f ms/step  (%d rebuilds in %d steps)" % (
                box["name"], box["pos"].shape[0], "exclusions + 1-4 + bonded" if bonded else "exclusions + 1-4", ms, builds,
                args.steps), flush=True)


if __name__ == "__main__":
    main()
