#!/usr/bin/env python3
"""Dibenzo-p-dioxin in water at constant pressure: the box of examples/restrained_solute.py -- the solute of the committed force-field
file (tests/golden/dibenzo-p-dioxin-in-water.xml) in a lattice of water, the waters rigid (emdee_md_set_rigid3), the solute's C-H
bonds fixed (emdee_md_set_hbonds), the solute's heavy atoms restrained (emdee_md_set_restraints) -- with the molecule table
(emdee_md_set_molecules, built in one line by ingest.molecules from the bond list) that lets such an engine take a barostat: the
pressure is the molecular one over WHOLE molecules, the scale translates the solute and every water with their centres of mass.
Four stages, the density and P_mol printed along the way:

  1. emdee_md_minimize with the heavy atoms restrained to where they are;
  2. 2 fs Langevin steps at 300 K, restrained, at constant volume;
  3. NPT: the same with C-rescale at 1 bar coupled to the molecular pressure (the restraint references follow the box);
  4. the release (the restraint table cleared) and the same number of NPT steps: the box finds its density.

    python examples/npt_solute.py [cells] [steps]   # cells^3 lattice sites of water (default 6: 216), steps per stage (default 500)

Every molecule is loaded WHOLE (no atom is wrapped into the box on its own): the centres of mass are formed from the unwrapped
coordinates.  Units: nm, ps, atomic mass units, kJ/mol, elementary charges.  Needs the built library
(python -c "import __graft_entry__ as g; g.build()") and a gfx950 device."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

E = load_package()
ing = E.ingest
dev = torch.device("cuda", 0)
cells = int(sys.argv[1]) if len(sys.argv) > 1 else 6
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 500
XML = os.path.join(ROOT, "tests", "golden", "dibenzo-p-dioxin-in-water.xml")
KB, T, DT, RC, RS, SKIN = 0.0083144626, 300.0, 0.002, 0.8, 0.7, 0.1
K_RESTRAINT = 1000.0                                             # kJ/mol/nm^2 on every axis of every heavy atom of the solute
TIGHT = 0.16                                                     # nm: a water whose oxygen is nearer to a solute atom is left out
BAR = 0.0602214076                                               # 1 bar in kJ/mol/nm^3
P_REF, BETA, TAU_P, EVERY = 1.0 * BAR, 4.5e-5 / BAR, 1.0, 10     # water's compressibility 4.5e-5 / bar; tau_p in ps

table, templates, nonbonded = ing.BondedTable(XML), ing.ResidueTemplates(XML), ing.NonbondedTable(XML)

# ---- the solute, flat: three fused hexagons of side s (ring A, the dioxin ring, ring B), hydrogens pointing away from their ring
s, r_ch = table.bond("ca", "ca")[0][1], table.bond("ca", "ha")[0][1]
h = 0.5 * np.sqrt(3.0) * s
ring = {"C5": (-h, 0.5 * s), "C4": (-h, -0.5 * s), "O1": (0.0, s), "O2": (0.0, -s), "C7": (h, 0.5 * s), "C12": (h, -0.5 * s),
        "C3": (-2 * h, -s), "C2": (-3 * h, -0.5 * s), "C1": (-3 * h, 0.5 * s), "C6": (-2 * h, s),
        "C8": (2 * h, s), "C9": (3 * h, 0.5 * s), "C10": (3 * h, -0.5 * s), "C11": (2 * h, -s)}
for name, carbon in (("H1", "C1"), ("H2", "C2"), ("H3", "C3"), ("H4", "C6"), ("H5", "C8"), ("H6", "C9"), ("H7", "C10"), ("H8", "C11")):
    c = np.array(ring[carbon])
    out = c - np.array([-2 * h if c[0] < 0 else 2 * h, 0.0])     # from the centre of the carbon's ring
    ring[name] = tuple(c + r_ch * out / np.linalg.norm(out))
names = templates.residues["aaa"]["names"]
solute = np.array([[ring[n][0], ring[n][1], 0.0] for n in names])

# ---- water on a lattice, the molecules that overlap the solute most left out
w = E.synthetic.water_box(cells)
L = w["L"]
if L < 2.0 * (RC + SKIN):
    sys.exit("the box side %.2f nm is below 2 (rc + skin) = %.2f nm: use more cells" % (L, 2.0 * (RC + SKIN)))
solute += 0.5 * L
water = w["positions"].reshape(-1, 3, 3)
ow = templates.residues["HOH"]["types"].index("OW")
rel = water - water[:, ow:ow + 1, :]                             # the lattice builder wraps atom by atom: make every water whole again
water = water[:, ow:ow + 1, :] + rel - L * np.rint(rel / L)
d = water[:, ow, None, :] - solute[None, :, :]
d -= L * np.rint(d / L)
keep = np.linalg.norm(d, axis=2).min(axis=1) >= TIGHT
water = water[keep]
n_water = len(water)
sequence = ["aaa"] + ["HOH"] * n_water
types, bonds = templates.build(sequence)
pos = np.concatenate([solute, water.reshape(-1, 3)])              # whole molecules: nothing is wrapped atom by atom
N = len(types)
mass = np.array([table.masses[t] for t in types])
charges = templates.charges(sequence)
atoms = nonbonded.lj_atoms(types)

# ---- topology: the harmonic terms the two constraint tables replace are taken out
top = ing.topology(types, bonds, table)
mol, geom, drop_b, drop_a = ing.rigid_triatomics(types, bonds, table, with_dropped=True)
clusters, dist, drop_h = ing.hydrogen_clusters(types, bonds, table, skip=mol, with_dropped=True)


def without(rows, params, drop):
    gone = {tuple(r) for r in np.asarray(drop).tolist()}
    sel = np.array([tuple(r) not in gone for r in rows.tolist()], dtype=bool)
    return rows[sel], params[sel]


bond_ids, bond_params = without(top["bonds"], top["bond_params"], np.concatenate([drop_b, drop_h]))
angle_ids, angle_params = without(top["angles"], top["angle_params"], drop_a)

md = E.VelocityVerlet(E.cu(pos, dev), E.cu(np.zeros((N, 3)), dev), L, E.LennardJonesModel(RC, RS), E.cu(atoms, dev), skin=SKIN,
                      inv_mass=E.cu(1.0 / mass, dev))
md.set_exclusions_(top["exclusions"])
md.set_pairs14_(top["pairs14"], nonbonded.lj14scale)
md.set_bonded_(E.HARMONIC_BOND, bond_ids, bond_params)
md.set_bonded_(E.HARMONIC_ANGLE, angle_ids, angle_params)
md.set_bonded_(E.PERIODIC_TORSION, top["torsions"], top["torsion_params"])
md.set_coulomb_(charges, E.COULOMB_K_KJ_NM, eps_rf=78.0, coulomb14scale=nonbonded.coulomb14scale)
md.set_rigid3_(mol, geom)
md.set_hbonds_(clusters, dist)
molecule = ing.molecules(N, bonds)                               # the solute is one molecule, every water another
md.set_molecules_(molecule)
md.set_molecular_scaling_()                                      # the three pressure entries take whole molecules from the table


def side():
    return np.array(md.box()[1])


def closest_contact(x):
    """the shortest distance between a solute atom and a water atom"""
    d = x[len(solute):, None, :] - x[None, :len(solute), :]
    d -= side() * np.rint(d / side())
    return np.linalg.norm(d, axis=2).min()


def worst_constraint(x):
    worst = 0.0
    for i, j, want in ([(mol[:, 0], mol[:, 1], geom[:, 0]), (mol[:, 0], mol[:, 2], geom[:, 0]), (mol[:, 1], mol[:, 2], geom[:, 1])]
                       + [(clusters[clusters[:, k] >= 0, 0], clusters[clusters[:, k] >= 0, k], dist[clusters[:, k] >= 0, k - 1]) for k in (1, 2, 3)]):
        if len(i):
            r = x[i] - x[j]
            r -= side() * np.rint(r / side())
            worst = max(worst, np.abs(np.linalg.norm(r, axis=1) / want - 1.0).max())
    return worst



heavy = ing.heavy_atoms(types, table, skip=mol)                  # the twelve carbons and two oxygens of the solute
start = None


def report(stage):
    """the restraint energy and the RMS distance of the solute's heavy atoms from where they started"""
    x = md.state(velocities=False, forces=False)["positions"].cpu().numpy()
    d = x[heavy] - start
    sums = md.restraint_sums()
    p_mol = np.trace(md.molecular_pressure_tensor()["pressure"]) / 3.0
    print("%-26s box %.4f nm  density %.3f g/cm^3  P_mol %9.1f bar  restraint energy %8.3f kJ/mol  solute RMS %.4f nm  constraints %.1e"
          % (stage, side()[0], mass.sum() / np.prod(side()) * 1.66053907e-3, p_mol / BAR, sums[0], np.sqrt((d * d).sum(axis=1).mean()),
             worst_constraint(x)))
    assert np.isfinite(sums[0]) and worst_constraint(x) < 1e-10
    return x


print("%d solute atoms (%d heavy) and %d rigid waters in %d molecules, box %.3f nm; closest solute-water contact %.3f nm"
      % (len(solute), len(heavy), n_water, molecule.max() + 1, L, closest_contact(pos)))
start = md.state(velocities=False, forces=False)["positions"].cpu().numpy()[heavy]

# ---- 1. minimise with the heavy atoms restrained to where they are (ref = None: the current positions)
md.set_restraints_(heavy, K_RESTRAINT)
res = md.minimize_(2000, 200.0, dt_start=0.0002, dt_max=0.002, max_step=0.01)
x = report("minimised (%d iterations):" % res.iterations)
print("    E_pot %.1f -> %.1f kJ/mol, closest contact %.3f nm" % (res.energy0, res.energy, closest_contact(x)))

# ---- 2. 2 fs Langevin steps with the restraints on (the references are kept across set_state: the atom count is the same)
rng = np.random.default_rng(2026)
vel = rng.normal(size=(N, 3)) * np.sqrt(KB * T / mass)[:, None]
md.set_state_(E.cu(x, dev), E.cu(vel, dev), E.cu(atoms, dev), E.cu(1.0 / mass, dev))
md.set_langevin_(gamma=5.0, temperature=KB * T, seed=2026)
dof = 3 * N - 3 * len(mol) - int((clusters[:, 1:] >= 0).sum()) - 3
done = 0
while done < steps:
    n = min(100, steps - done)
    md.step_(n, DT)
    done += n
    report("NVT, restrained, %5d:" % done)

# ---- 3. NPT with the restraints on: C-rescale on the molecular pressure; an hbonds engine takes it because the molecule table is in force
md.set_barostat_("c-rescale", P_REF, BETA, TAU_P, EVERY, temperature=KB * T, seed=2027)
print("NPT: C-rescale at %g bar every %d steps (tau_p = %g ps), coupled to the molecular pressure over whole molecules" % (P_REF / BAR, EVERY, TAU_P))
done = 0
while done < steps:
    n = min(100, steps - done)
    md.step_(n, DT)
    done += n
    report("NPT, restrained, %5d:" % done)

# ---- 4. the release (the restraint sums of an empty table are zero)
md.set_restraints_(None, 0.0)
done = 0
while done < steps:
    n = min(100, steps - done)
    md.step_(n, DT)
    done += n
    ep, ek, _ = md.totals()
    report("NPT, released, %5d:" % done)
    print("    T = %6.1f K  E_pot = %10.1f kJ/mol" % (2.0 * ek / (dof * KB), ep))
    assert np.isfinite(ep)
md.close()
