"""One rank of a two-rank decomposition over RCCL on one device (tests/test_gpu_virial_tensor.py), or with --in-process both
domains in this process.  Rank 0 prints `ID <hex>` (the communicator id), the other rank reads that line on stdin.  Every
process ends with `SUMS <12 all-reduced sums at the load> <12 after 30 steps>` and exit code 0."""
import argparse
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--in-process", action="store_true")
    ap.add_argument("--cells", type=int, default=16)
    args = ap.parse_args()
    limit = threading.Timer(200.0, lambda: os._exit(3))   # a rank whose peer has gone must not wait for ever
    limit.daemon = True
    limit.start()
    sys.path.insert(0, ROOT)
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    dev = torch.device("cuda", 0)
    if args.in_process:
        uid = None
    elif args.rank == 0:
        uid = pkg.DomainDecomposition.unique_id()
        print("ID " + uid.hex(), flush=True)
    else:
        line = sys.stdin.readline().split()
        uid = bytes.fromhex(line[1])
    dd = pkg.DomainDecomposition.synthetic(args.cells, 2, None if args.in_process else args.rank, dev, pkg.LennardJonesModel(2.5, 2.0),
                                           pkg=pkg, unique_id=uid, raw_velocities=True)
    s0 = dd.tensor_sums()
    dd.step_(30, 0.005, 0)
    s1 = dd.tensor_sums()
    torch.cuda.synchronize(dev)
    print("SUMS " + " ".join("%.17g" % v for v in s0 + s1), flush=True)
    dd.close()


if __name__ == "__main__":
    main()
