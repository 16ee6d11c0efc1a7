"""Cost and accuracy of the reaction-field Coulomb terms, undivided fp64:

  rsq    the relative error of the fp64 1/r of the charged kernels (lj_pair.hpp fast_rsq: v_rsq_f64 seed + one Newton step),
         read off the per-atom virials of isolated charged dimers at eps_rf = 1, where W = K q_i q_j / r exactly and the LJ
         terms vanish (epsilon 0): 200,000 dimers at r uniform in [0.2, rc), relative error of 2 w_i against K q q / r in fp64
  water  ms/step of the 985,527-atom water box of profiles/bonded_cost.py (synthetic.water_box(69): exclusions, bonds, angles;
         nm, kJ/mol, real masses, rc 0.9, rs 0.8, skin 0.1, dt 0.5 fs) without and with the HOH charges (K = COULOMB_K_KJ_NM,
         eps_rf = inf), the two forms alternating
  sigma  ms/step of a 1,000,188-atom fcc box (63^3 cells, rho* = 0.8, one LJ type, rc 2.5, rs 2.0, skin 0.3, dt 0.005) without
         charges (the single-species plane kernel, fused step) and with alternating +-0.5 charges (K = 1, eps_rf = inf: the
         charged general-species kernel, split step), alternating

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 profiles/coulomb_cost.py`
and read the k_brick / k_lj_force_nbr(_q) / k_pairs14(_q) rows of the stats file.

    python3 profiles/coulomb_cost.py [--steps 100] [--warmup 20] [--only rsq,water,sigma]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

E = load_package()


def rsq_error(dev, n=200_000, rc=2.5, seed=3):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3)))
    spacing = 2.0 * (rc + 0.3) + rc
    sites = np.stack(np.meshgrid(*(np.arange(side),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n] * spacing + 1.0
    r = rng.uniform(0.2, rc, n)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    L = side * spacing
    pos = np.empty((2 * n, 3))
    pos[0::2], pos[1::2] = sites, sites + r[:, None] * u
    pos = np.mod(pos, L)
    q = np.empty(2 * n)
    q[0::2], q[1::2] = 1.0, -1.0
    atoms = E.lennard_jones_atoms(np.zeros(2 * n), np.ones(2 * n))
    md = E.VelocityVerlet(E.cu(pos, dev), E.cu(np.zeros((2 * n, 3)), dev), L, E.LennardJonesModel(rc, 0.8 * rc), E.cu(atoms, dev),
                          skin=0.3)
    md.set_coulomb_(q, 1.0, 1.0)                                        # eps_rf = 1: k_rf = 0, W = K q q / r
    w = md.state(positions=False, velocities=False, forces=False, virials=True)["virials"].cpu().numpy()
    md.close()
    d = pos[0::2] - pos[1::2]
    d -= L * np.rint(d / L)
    exact = -1.0 / np.sqrt((d * d).sum(axis=1))                        # K q_i q_j / r with q_i q_j = -1
    rel = np.abs(np.concatenate([2 * w[0::2], 2 * w[1::2]]) / np.concatenate([exact, exact]) - 1.0)
    return rel.max(), np.sqrt(np.mean(rel * rel))


def water(n=69):
    w = E.synthetic.water_box(n)
    N = w["positions"].shape[0]
    vel = np.random.default_rng(11).normal(size=(N, 3)) * np.sqrt(2.494 * w["inv_mass"])[:, None]
    terms = [(E.HARMONIC_BOND, w["bonds"], w["bond_params"]), (E.HARMONIC_ANGLE, w["angles"], w["angle_params"])]
    return dict(name="water", pos=w["positions"], vel=vel, L=w["L"], atoms=w["atoms"], inv_mass=w["inv_mass"], excl=w["exclusions"],
                terms=terms, q=w["charges"], K=E.COULOMB_K_KJ_NM, rc=0.9, rs=0.8, skin=0.1, dt=0.0005)


def sigma_box(ncell=63):
    pos, gid, lengths = E.synthetic.fcc_block((ncell,) * 3, (0, 0, 0), (ncell,) * 3)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    vel = E.synthetic.raw_normals(np.arange(N), N)
    vel -= vel.mean(axis=0)
    vel *= np.sqrt(0.8 * (3 * N - 3) / np.sum(vel * vel))
    q = 0.5 * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    return dict(name="sigma", pos=pos, vel=vel, L=float(lengths[0]), atoms=E.lennard_jones_atoms(1.0, 1.0, N), inv_mass=None,
                excl=None, terms=[], q=q, K=1.0, rc=2.5, rs=2.0, skin=0.3, dt=0.005)


def run(box, charged, steps, warmup, dev):
    md = E.VelocityVerlet(E.cu(box["pos"], dev), E.cu(box["vel"], dev), box["L"], E.LennardJonesModel(box["rc"], box["rs"]),
                          E.cu(box["atoms"], dev), skin=box["skin"],
                          inv_mass=None if box["inv_mass"] is None else E.cu(box["inv_mass"], dev))
    if box["excl"] is not None:
        md.set_exclusions_(box["excl"])
    for kind, a, p in box["terms"]:
        md.set_bonded_(kind, a, p)
    if charged:
        md.set_coulomb_(box["q"], box["K"], float("inf"))
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
    ap.add_argument("--only", default="rsq,water,sigma")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    if "rsq" in only:
        mx, rms = rsq_error(dev)
        print("rsq    fp64 1/r relative error over 400,000 pair terms: max %.3g, rms %.3g" % (mx, rms), flush=True)
    for name, make in (("water", water), ("sigma", sigma_box)):
        if name not in only:
            continue
        box = make()
        for charged in (False, True, False, True):
            ms, builds = run(box, charged, args.steps, args.warmup, dev)
            print("%-6s %7d atoms  %-10s %.3f ms/step  (%d rebuilds in %d steps)" % (
                name, box["pos"].shape[0], "charged" if charged else "uncharged", ms, builds, args.steps), flush=True)


if __name__ == "__main__":
    main()
