"""One rank of a two-rank decomposition over RCCL on one device on a NON-CUBIC global box
(tests/test_gpu_orthorhombic.py).  Rank 0 prints `ID <hex>` (the communicator id), the other rank reads that line on stdin.

The chain box of the decomposed cases of that module -- (8, 10, 13) fcc cells, sides (13.68, 17.10, 22.23), exclusions, 1-4
pairs, bonded terms, charges -- is loaded on the grid given by --grid, stepped 60 times in two calls, and each rank writes its
owned atoms (gid, positions, velocities) to <out>/rank<r>.npz and prints `TOTALS <potential> <kinetic> <virial>`.  Exit 0."""
import argparse
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--out", required=True)
    ap.add_argument("--grid", default="1,2,1")
    args = ap.parse_args()
    limit = threading.Timer(200.0, lambda: os._exit(3))   # a rank whose peer has gone must not wait for ever
    limit.daemon = True
    limit.start()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    from tests.test_gpu_orthorhombic import DT, _dd_want
    E = load_package()
    dev = torch.device("cuda", 0)
    grid = tuple(int(g) for g in args.grid.split(","))
    assert grid[0] * grid[1] * grid[2] == 2
    if args.rank == 0:
        uid = E.DomainDecomposition.unique_id()
        print("ID " + uid.hex(), flush=True)
    else:
        uid = bytes.fromhex(sys.stdin.readline().split()[1])
    S, atoms, _ = _dd_want(E, "float64", True)
    N = S["N"]
    dd = E.DomainDecomposition(list(S["lengths"]), grid, E.LennardJonesModel(S["rc"], S["rs"]), skin=S["skin"], device=dev,
                               rank=args.rank, unique_id=uid)
    mine = np.arange(args.rank, N, 2)                 # scattered initial slices: the load hands each atom to its domain
    dd.set_atoms_(0, E.cu(S["pos"][mine], dev), E.cu(S["vel"][mine], dev), E.cu(atoms[mine], dev),
                  torch.from_numpy(mine.astype(np.int64)).to(dev))
    dd.set_exclusions_(S["excl"])
    dd.set_pairs14_(S["p14"], S["s14"])
    for kind, a, p in S["terms"]:
        dd.set_bonded_(kind, a, p)
    dd.set_coulomb_(S["q"], S["coulomb"][0], S["coulomb"][1], S["c14"])
    dd.load_()
    dd.step_(29, DT)
    dd.step_(31, DT)
    gid, x, v, _ = (t.cpu().numpy() for t in dd.state(0))
    np.savez(os.path.join(args.out, "rank%d.npz" % args.rank), gid=gid, x=x, v=v)
    print("TOTALS " + " ".join("%.17g" % t for t in dd.totals()), flush=True)
    torch.cuda.synchronize(dev)
    dd.close()


if __name__ == "__main__":
    main()
