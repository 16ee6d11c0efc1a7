"""One rank of a two-rank decomposition over RCCL on one device with charges (tests/test_gpu_coulomb_ranks.py).  Rank 0 prints
`ID <hex>` (the communicator id), the other rank reads that line on stdin.

The charged chain box of tests/test_gpu_coulomb.py (exclusions, 1-4 pairs, bonded terms, charges 0.6 / -0.3 / -0.5 / 0.2 per
chain, eps_rf = 5, coulomb14scale 0.8333) is loaded, stepped 60 times in two calls, and each rank writes its owned atoms (gid,
positions, velocities) to <out>/rank<r>.npz and prints `TOTALS <potential> <kinetic> <virial>`.  Then a charge table one id
short replaces the charges: the set call and a following step must both fail on every rank, although only the rank that owns
the last gid holds an atom outside the table; the rank prints `REFUSED <code of the set call> <code of the step>`.  Exit 0."""
import argparse
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def CHARGES(N):
    import numpy as np
    return np.tile([0.6, -0.3, -0.5, 0.2], N // 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    limit = threading.Timer(200.0, lambda: os._exit(3))   # a rank whose peer has gone must not wait for ever
    limit.daemon = True
    limit.start()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    from tests.test_gpu_bonded import DT, RC, RS, SKIN, _box, _chains, _lj14scale
    E = load_package()
    dev = torch.device("cuda", 0)
    if args.rank == 0:
        uid = E.DomainDecomposition.unique_id()
        print("ID " + uid.hex(), flush=True)
    else:
        uid = bytes.fromhex(sys.stdin.readline().split()[1])
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    dd = E.DomainDecomposition([L] * 3, E.domain.rank_grid(2), E.LennardJonesModel(RC, RS), skin=SKIN, device=dev, rank=args.rank,
                               unique_id=uid)
    mine = np.arange(args.rank, N, 2)                 # scattered initial slices: the load hands each atom to its domain
    dd.set_atoms_(0, E.cu(pos[mine], dev), E.cu(vel[mine], dev), E.cu(atoms[mine], dev), torch.from_numpy(mine.astype(np.int64)).to(dev))
    dd.set_exclusions_(excl)
    dd.set_pairs14_(p14, _lj14scale(E))
    for kind, a, p in terms:
        dd.set_bonded_(kind, a, p)
    dd.set_coulomb_(CHARGES(N), 1.0, 5.0, 0.8333)
    dd.load_()
    dd.step_(29, DT)
    dd.step_(31, DT)
    gid, x, v, _ = (t.cpu().numpy() for t in dd.state(0))
    np.savez(os.path.join(args.out, "rank%d.npz" % args.rank), gid=gid, x=x, v=v)
    print("TOTALS " + " ".join("%.17g" % t for t in dd.totals()), flush=True)
    codes = []
    for call in (lambda: dd.set_coulomb_(CHARGES(N)[:-1], 1.0, 5.0, 0.8333), lambda: dd.step_(1, DT)):
        try:
            call()
            codes.append(0)
        except E.EmDeeError as err:
            codes.append(err.code)
    print("REFUSED %d %d" % tuple(codes), flush=True)
    torch.cuda.synchronize(dev)
    dd.close()


if __name__ == "__main__":
    main()
