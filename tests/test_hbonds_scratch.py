"""CPU check of the constraint kernels (csrc/settle.hpp, instantiated for the Triangle policy there and the Star policy of
csrc/shake.hpp) in the shape of test_abi_and_host's scratch-memory test: after `make report` (hipcc
-Rpass-analysis=kernel-resource-usage on both kernel translation units, cross-compiled: no GPU needed) no instance of the four
kernels, in either policy, in either resource file keeps bytes in scratch memory.  The kernels loop over a group's sites at
compile time and the solvers are written for three satellites with compile-time loops, so that no array is indexed at run time;
an index that did would put the site arrays in scratch."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from .conftest import ROOT

SRC = os.path.join(ROOT, "emdee.jl_amd", "csrc")
REPORTS = [os.path.join(SRC, name) for name in ("resource_usage_f64.txt", "resource_usage_f32.txt")]


def _reports_are_current():
    sources = glob.glob(os.path.join(SRC, "*.hpp")) + glob.glob(os.path.join(SRC, "*.hip")) + [os.path.join(SRC, "Makefile")]
    newest = max(os.path.getmtime(p) for p in sources)
    return all(os.path.exists(p) and os.path.getmtime(p) >= newest for p in REPORTS)


def test_no_hbonds_kernel_uses_scratch_memory():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    if not _reports_are_current():                                           # (the other scratch test may have written them just now)
        subprocess.check_call(["make", "-s", "-C", SRC, "report"], timeout=1500)
    stages = ("k_constraint_gather", "k_constraint_positions", "k_constraint_velocities", "k_constraint_check")
    want = {(stage, policy) for stage in stages for policy in ("Triangle", "Star")}
    for path in REPORTS:
        seen = set()
        for b in re.split(r"remark: Function Name: ", open(path).read())[1:]:
            fn = b.split(" ", 1)[0]
            if "k_constraint_" not in fn:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
            assert m is not None, fn
            assert int(m.group(1)) == 0, "%s keeps %s bytes per lane in scratch memory" % (fn, m.group(1))
            here = {(stage, policy) for stage, policy in want if stage in fn and policy in fn}
            assert len(here) == 1, fn                                            # (every instance is one stage in one policy)
            seen |= here
        assert seen == want, (os.path.basename(path), sorted(want - seen))
