"""CPU test of the shared two-stage reduction (csrc/reduce.hpp): every box sum is an instance of k_reduce_partials over its term,
completed by k_reduce_final or, for the thermostat's K, by k_thermostat_update, and none of them keeps anything in scratch memory --
a term struct passed by value that the compiler spills is the regression this guards against."""
import os
import re
import shutil
import subprocess

import pytest

from .conftest import ROOT

TERMS = ("EnergySums", "TensorSums", "MoleculeSums", "RestraintSums", "FireSums", "KineticSums", "HeatSums")


def test_every_sum_is_in_the_report_and_uses_no_scratch_memory():
    """`make report` (hipcc -Rpass-analysis=kernel-resource-usage on both kernel translation units, cross-compiled: no GPU needed)"""
    src = os.path.join(ROOT, "emdee.jl_amd", "csrc")
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-s", "-C", src, "report"], timeout=1500)
    for name, real in (("resource_usage_f64.txt", "Id"), ("resource_usage_f32.txt", "If")):
        text = open(os.path.join(src, name)).read()
        scratch = {}
        for b in re.split(r"remark: Function Name: ", text)[1:]:
            fn = b.split(" ", 1)[0].strip()
            if "k_reduce_" not in fn and "k_thermostat_update" not in fn:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
            assert m is not None, fn
            scratch[fn] = int(m.group(1))
        wanted = ["k_reduce_partialsINS_%d%s%sE" % (len(t), t, real) for t in TERMS] + ["k_reduce_final", "k_thermostat_update"]
        for kernel in wanted:
            found = [f for f in scratch if kernel in f]
            assert len(found) == 1, (name, kernel, sorted(scratch))
            assert scratch[found[0]] == 0, "%s keeps %d bytes per lane in scratch memory" % (found[0], scratch[found[0]])
        assert len(scratch) == len(wanted), (name, sorted(scratch))   # (a term nobody listed here)
