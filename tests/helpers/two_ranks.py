"""Launcher of the two-rank GPU tests: two processes of one rank script (bonded_rank.py, coulomb_rank.py) on one device, joined
by RCCL.  Rank 0 prints the unique id ("ID ..."), which rank 1 reads from its standard input."""
import os
import subprocess
import sys


def run_two_ranks(script, out_dir, hostid):
    """Runs `script --rank r --out out_dir` for r = 0, 1 with NCCL_HOSTID = hostid + r; returns the two processes and their
    (stdout, stderr).  Whatever still runs when this returns or raises is killed."""
    env0 = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1", NCCL_NET_GDR_LEVEL="0")
    kids = []
    try:
        for r in range(2):
            env = dict(env0, NCCL_HOSTID="%s%d" % (hostid, r))
            k = subprocess.Popen([sys.executable, script, "--rank", str(r), "--out", str(out_dir)], env=env, stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
            kids.append(k)
            if r == 0:
                uid = k.stdout.readline().strip()
                assert uid.startswith("ID "), uid
            else:
                k.stdin.write(uid + "\n")
                k.stdin.flush()
        outs = [k.communicate(timeout=240) for k in kids]
    finally:
        for k in kids:
            if k.poll() is None:
                k.kill()
    return kids, outs
