"""The laboratory of rounds 1-5 -- measured alternatives that lost (the transposed build, the 4-lane build, near/far rows and
the far-class skip, the two-phase build with per-lane candidate loops, tuning brick shapes) and the ablation switches that
measured them -- has been retired from the tree; DESIGN.md ("Product and laboratory") keeps the measurements.  The library
REFUSES those switches with a message (a run that believes it measures a variant must not silently measure the default).

The library reads the environment when an engine is created, so every case runs in a child process."""
import os
import subprocess
import sys
import textwrap

import pytest

from .conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REMOVED = ["EMDEE_TBUILD", "EMDEE_BUILD4", "EMDEE_BUILD_ALG", "EMDEE_BUILD_NEARFAR", "EMDEE_FAR_SKIP", "EMDEE_DEBUG_RC2_SCALE",
           "EMDEE_NO_BRICK_TABLES", "EMDEE_NO_PREMUL", "EMDEE_BRICK_VARIANT", "EMDEE_STRIDE"]

SMALL = textwrap.dedent("""
    import sys
    import numpy as np, torch
    sys.path.insert(0, %r)
    import __graft_entry__ as g
    E = g.load_package()
    dev = torch.device("cuda", 0)
    x, L = E.synthetic.fcc_positions(8)
    N = x.shape[0]
    try:
        tiles = E.nonbonded_computation_tiles(N, skin=0.3)
        f = torch.zeros((N, 3), dtype=torch.float64, device=dev)
        E.compute_nonbonded_(f, None, None, E.cu(x, dev), L, tiles, E.LennardJonesModel(2.5, 2.0), E.cu(E.lennard_jones_atoms(1.0, 1.0, N), dev), E.Val(E.FORCES))
        print("RAN", float(f.abs().max()))
    except E.EmDeeError as err:
        print("REFUSED code=%%d %%s" %% (err.code, err))
""") % ROOT


@pytest.mark.parametrize("switch", REMOVED)
def test_the_product_library_refuses_experiment_switches(switch):
    env = dict(os.environ)
    env.pop("EMDEE_HIP_LIB", None)
    env[switch] = "1"
    r = subprocess.run([sys.executable, "-c", SMALL], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-600:]
    line = [l for l in r.stdout.splitlines() if l.startswith(("RAN", "REFUSED"))][-1]
    assert line.startswith("REFUSED") and switch in line and "experiment switch" in line and "EXPERIMENTS=1" in line, line
    assert "retired" in line, line
    assert "DESIGN.md" in line and "Product and laboratory" in line, line

