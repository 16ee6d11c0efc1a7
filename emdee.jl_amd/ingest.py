"""Inputs and outputs either side of the hot path: an XYZ reader/writer
(stands in for the Chemfiles read of test/runtests.jl:20-23), the Lennard-Jones part of an OpenMM-style
force-field file (the `NonbondedForce` table the reference parses at src/modelling.jl:71-73,197-200)
turned into LJAtom arrays, its bonded terms (`HarmonicBondForce`, `HarmonicAngleForce`, `PeriodicTorsionForce` propers,
src/modelling.jl:46-69) and residue templates turned into the tables of emdee_*_set_bonded, exclusions and 1-4 pairs, and a
checkpoint of (positions, velocities, step).  Host-side, numpy only."""
from collections import deque
import xml.etree.ElementTree as ET

import numpy as np

from .lennard_jones import lennard_jones_atoms


def read_xyz(path):
    """(names, positions (N, 3) float64) of the first frame of an XYZ file."""
    with open(path) as fh:
        n = int(fh.readline())
        fh.readline()
        names, pos = [], np.empty((n, 3), dtype=np.float64)
        for i in range(n):
            t = fh.readline().split()
            names.append(t[0])
            pos[i] = [float(t[1]), float(t[2]), float(t[3])]
    return names, pos


def write_xyz(path, names, positions, comment=""):
    positions = np.asarray(positions, dtype=np.float64)
    with open(path, "w") as fh:
        fh.write("%d\n%s\n" % (positions.shape[0], comment))
        for name, p in zip(names, positions):
            fh.write("%s %.12E %.12E %.12E\n" % (name, p[0], p[1], p[2]))


class NonbondedTable:
    """`<NonbondedForce lj14scale= coulomb14scale=><Atom type= sigma= epsilon= [charge=]/>...` -- the
    columns of the reference's NONBONDED frame (src/modelling.jl:71-73) and the two 1-4 scaling factors
    (:198-200, default 1.0).  sigma in nm and epsilon in kJ/mol as OpenMM writes them."""

    def __init__(self, xml_file):
        root = ET.parse(xml_file).getroot()
        nb = root.find("NonbondedForce")
        if nb is None:
            raise ValueError("no NonbondedForce element in %s" % xml_file)
        self.lj14scale = float(nb.attrib.get("lj14scale", 1.0))
        self.coulomb14scale = float(nb.attrib.get("coulomb14scale", 1.0))
        self.types = {}
        for atom in nb.findall("Atom"):
            self.types[atom.attrib["type"]] = dict(sigma=float(atom.attrib["sigma"]), epsilon=float(atom.attrib["epsilon"]),
                                                   charge=float(atom.attrib.get("charge", 0.0)))

    def lj_atoms(self, atom_types, length_unit=1.0, energy_unit=1.0):
        """LJAtom array for a sequence of type names; sigma / length_unit and epsilon / energy_unit convert to
        the caller's units (e.g. length_unit = 0.1 for Angstrom positions with nm force-field sigmas)."""
        sigma = np.array([self.types[t]["sigma"] for t in atom_types], dtype=np.float64) / length_unit
        eps = np.array([self.types[t]["epsilon"] for t in atom_types], dtype=np.float64) / energy_unit
        return lennard_jones_atoms(eps, sigma)


class BondedTable:
    """Bonded parameters by atom type: `<HarmonicBondForce><Bond type1= type2= length= k=/>`, `<HarmonicAngleForce><Angle
    type1..3= angle= k=/>` and `<PeriodicTorsionForce><Proper type1..4= periodicity1..N= phase1..N= k1..N=/>` (impropers are
    not read).  A pattern names types (`typeN`) or classes (`classN`, the class of each type from `<AtomTypes>`); "" is a
    wildcard; a pattern matches forward or reversed.  Of the patterns that match, the one with the fewest wildcards wins, and
    among those the first in the file (OpenMM's preference of a specific match over a wildcard one).  Units as OpenMM writes
    them: nm, kJ/mol, radians."""

    def __init__(self, xml_file):
        root = ET.parse(xml_file).getroot()
        self.classes = {t.attrib["name"]: t.attrib.get("class", t.attrib["name"]) for t in root.iter("Type")}
        self.masses = {t.attrib["name"]: float(t.attrib["mass"]) for t in root.iter("Type") if "mass" in t.attrib}
        self.elements = {t.attrib["name"]: t.attrib["element"] for t in root.iter("Type") if "element" in t.attrib}
        self.bonds, self.angles, self.propers = [], [], []
        for kind, tag, n, out in (("HarmonicBondForce", "Bond", 2, self.bonds), ("HarmonicAngleForce", "Angle", 3, self.angles),
                                  ("PeriodicTorsionForce", "Proper", 4, self.propers)):
            for force in root.findall(kind):
                for el in force.findall(tag):
                    a = el.attrib
                    by = "class" if ("class1" in a and "type1" not in a) else "type"
                    pattern = tuple(a.get("%s%d" % (by, k + 1), "") for k in range(n))
                    if tag == "Bond":
                        params = [(float(a["k"]), float(a["length"]))]
                    elif tag == "Angle":
                        params = [(float(a["k"]), float(a["angle"]))]
                    else:
                        params, m = [], 1
                        while "k%d" % m in a:
                            params.append((float(a["k%d" % m]), float(a["periodicity%d" % m]), float(a["phase%d" % m])))
                            m += 1
                    out.append((by, pattern, params))

    def _find(self, table, atom_types):
        best, fewest = None, None
        for by, pattern, params in table:
            names = atom_types if by == "type" else tuple(self.classes.get(t, t) for t in atom_types)
            if any(all(p == "" or p == t for p, t in zip(pattern, seq)) for seq in (names, names[::-1])):
                wild = pattern.count("")
                if fewest is None or wild < fewest:
                    best, fewest = params, wild
        return best

    def bond(self, t1, t2):
        return self._find(self.bonds, (t1, t2))

    def angle(self, t1, t2, t3):
        return self._find(self.angles, (t1, t2, t3))

    def proper(self, t1, t2, t3, t4):
        return self._find(self.propers, (t1, t2, t3, t4))


class ResidueTemplates:
    """`<Residues><Residue name=><Atom name= type= [charge=]/>...<Bond atomName1= atomName2=/>...` of a force-field file
    (a template atom without a charge has charge 0)."""

    def __init__(self, xml_file):
        root = ET.parse(xml_file).getroot()
        self.residues = {}
        for res in root.iter("Residue"):
            names = [a.attrib["name"] for a in res.findall("Atom")]
            index = {nm: k for k, nm in enumerate(names)}
            types = [a.attrib["type"] for a in res.findall("Atom")]
            charges = [float(a.attrib.get("charge", 0.0)) for a in res.findall("Atom")]
            bonds = [(index[b.attrib["atomName1"]], index[b.attrib["atomName2"]]) for b in res.findall("Bond")]
            self.residues[res.attrib["name"]] = dict(names=names, types=types, bonds=bonds, charges=charges)

    def build(self, sequence):
        """(types, bonds (n, 2) int64) of a sequence of residue names, the atoms of each residue in template order"""
        types, bonds = [], []
        for name in sequence:
            r = self.residues[name]
            bonds += [(len(types) + i, len(types) + j) for i, j in r["bonds"]]
            types += r["types"]
        return types, np.array(bonds, dtype=np.int64).reshape(-1, 2)

    def charges(self, sequence):
        """charges (elementary charges, float64) of a sequence of residue names, in the atom order of build(sequence)"""
        return np.array([q for name in sequence for q in self.residues[name]["charges"]], dtype=np.float64)


def topology(types, bonds, table, length_unit=1.0, energy_unit=1.0):
    """Bonded terms, exclusions and 1-4 pairs of atoms of the given types joined by the given bonds (emdee_*_set_bonded,
    _set_exclusions, _set_pairs14):
      bonds, angles, torsions: (n, 2 | 3 | 4) ids, every i-j-k and i-j-k-l path of distinct atoms once; a torsion with several
        periodicities appears once per term;
      bond_params {k, r0}, angle_params {k, theta0}, torsion_params {k, n, phase}: parameters in the caller's units (lengths
        / length_unit, energies / energy_unit, as NonbondedTable.lj_atoms);
      exclusions: the 1-2 and 1-3 pairs; pairs14: the pairs at bond distance exactly 3, each once.
    Raises KeyError for a term the table has no parameters for."""
    n = len(types)
    nb = [set() for _ in range(n)]
    for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2):
        nb[i].add(int(j)); nb[j].add(int(i))
    nb = [sorted(s) for s in nb]
    bl = sorted({(min(i, j), max(i, j)) for i in range(n) for j in nb[i]})
    angles = [(i, j, k) for j in range(n) for i in nb[j] for k in nb[j] if i < k]
    tors = [(i, j, k, l) for j in range(n) for k in nb[j] if j < k for i in nb[j] if i != k for l in nb[k] if l != j and l != i]

    def need(params, what, ids):
        if params is None:
            raise KeyError("no %s parameters for atoms %s (types %s)" % (what, ids, tuple(types[a] for a in ids)))
        return params

    kb, kt = energy_unit / length_unit ** 2, energy_unit
    bp = [(k / kb, r0 / length_unit) for i, j in bl for k, r0 in need(table.bond(types[i], types[j]), "bond", (i, j))]
    ap = [(k / kt, th) for i, j, k_ in angles for k, th in need(table.angle(types[i], types[j], types[k_]), "angle", (i, j, k_))]
    ta, tp = [], []
    for q in tors:
        for k, per, ph in need(table.proper(*(types[a] for a in q)), "proper torsion", q):
            ta.append(q); tp.append((k / kt, per, ph))
    # bond distances up to 3 from every atom (ring atoms reached by two paths count once, at their shortest distance)
    excl, p14 = set(), set()
    for s in range(n):
        dist = {s: 0}
        todo = deque([s])
        while todo:
            a = todo.popleft()
            if dist[a] == 3:
                continue
            for b in nb[a]:
                if b not in dist:
                    dist[b] = dist[a] + 1
                    todo.append(b)
        for t, d in dist.items():
            if t > s and d in (1, 2):
                excl.add((s, t))
            elif t > s and d == 3:
                p14.add((s, t))
    arr = lambda v, m, dt=np.int64: np.array(sorted(v) if isinstance(v, set) else v, dtype=dt).reshape(-1, m)
    return dict(bonds=arr(bl, 2), bond_params=arr(bp, 2, np.float64), angles=arr(angles, 3), angle_params=arr(ap, 2, np.float64),
                torsions=arr(ta, 4), torsion_params=arr(tp, 3, np.float64), exclusions=arr(excl, 2), pairs14=arr(p14, 2))


def rigid_triatomics(types, bonds, table, length_unit=1.0, with_dropped=False):
    """The rigid three-site molecules (emdee_md_set_rigid3) among the molecules of a bond graph: those of exactly three atoms in
    which a centre is bonded to two atoms of one type that are bonded to nothing else (water, H-O-H).  Returns (atoms, geom):
      atoms (n, 3) int64 {centre, a, b}, centre first, a < b; geom (n, 2) float64 {d_leg, d_base} with d_leg the bond's r0 and
        d_base = 2 r0 sin(theta0 / 2) from the angle entry, lengths / length_unit;
    with_dropped: (atoms, geom, drop_bonds, drop_angles), the last two the (m, 2) and (m, 3) ids of the bonds and angles the
    constraints replace, written as topology() writes them (i < j; i < k around the centre), for a caller who takes them out of
    the harmonic tables.
    Raises KeyError for a molecule the table has no bond or angle parameters for."""
    n = len(types)
    nb = [set() for _ in range(n)]
    for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2):
        nb[i].add(int(j)); nb[j].add(int(i))
    atoms, geom, drop_b, drop_a = [], [], [], []
    for c in range(n):
        if len(nb[c]) != 2:
            continue
        a, b = sorted(nb[c])
        if nb[a] != {c} or nb[b] != {c} or types[a] != types[b]:
            continue
        bond, angle = table.bond(types[c], types[a]), table.angle(types[a], types[c], types[b])
        if bond is None or angle is None:
            raise KeyError("no bond or angle parameters for the three-site molecule %s (types %s)"
                           % ((c, a, b), tuple(types[t] for t in (c, a, b))))
        r0, th = bond[0][1] / length_unit, angle[0][1]
        atoms.append((c, a, b)); geom.append((r0, 2.0 * r0 * np.sin(0.5 * th)))
        drop_b += [(min(c, a), max(c, a)), (min(c, b), max(c, b))]
        drop_a.append((a, c, b))
    arr = lambda v, m, dt=np.int64: np.array(v, dtype=dt).reshape(-1, m)
    out = (arr(atoms, 3), arr(geom, 2, np.float64))
    return out + (arr(drop_b, 2), arr(drop_a, 3)) if with_dropped else out


def heavy_atoms(types, table, skip=()):
    """The ids (ascending, int64) of the atoms that are not hydrogen and not in `skip`: the usual selection of a position-restraint
    table (emdee_md_set_restraints), with the waters found by rigid_triatomics passed as skip (any nesting of ids).  An atom is a
    hydrogen by the element of its type in the force-field file (`table`: a BondedTable), or, where the file names none, by a
    mass below 1.5."""
    skipped = set(int(i) for i in np.asarray(skip, dtype=np.int64).reshape(-1))

    def hydrogen(t):
        if t in table.elements:
            return table.elements[t].strip().upper() == "H"
        return t in table.masses and table.masses[t] < 1.5
    return np.array([i for i, t in enumerate(types) if i not in skipped and not hydrogen(t)], dtype=np.int64)


def bisector_sites(sites, molecules, d_leg, d_base, d_om):
    """The site table (emdee_md_set_vsites) of a fourth site on the bisector of rigid three-site molecules, at d_om from the apex
    towards the legs: sites (n,) the ids of the massless sites, molecules (n, 3) ids {apex, a, b} (rigid_triatomics' first result),
    d_leg, d_base the molecules' distances (scalars or (n,)).  With h = sqrt(d_leg^2 - d_base^2 / 4) the height of the triangle,
    the site apex + w (a - apex) + w (b - apex) lies 2 w h from the apex: w_b = w_c = d_om / (2 h).
    Returns (atoms (n, 4) int32 {site, apex, a, b}, weights (n, 2) float64)."""
    mol = np.asarray(molecules, dtype=np.int64).reshape(-1, 3)
    site = np.asarray(sites, dtype=np.int64).reshape(-1)
    if site.shape[0] != mol.shape[0]:
        raise ValueError("bisector_sites: %d sites but %d molecules" % (site.shape[0], mol.shape[0]))
    d_leg, d_base, d_om = (np.broadcast_to(np.asarray(v, dtype=np.float64), site.shape) for v in (d_leg, d_base, d_om))
    h2 = d_leg ** 2 - 0.25 * d_base ** 2
    if (h2 <= 0.0).any():
        raise ValueError("bisector_sites: d_base >= 2 d_leg is no triangle")
    w = d_om / (2.0 * np.sqrt(h2))
    return np.concatenate([site[:, None], mol], axis=1).astype(np.int32), np.stack([w, w], axis=1)


def hydrogen_clusters(types, bonds, table, length_unit=1.0, skip=(), with_dropped=False):
    """The star clusters of bonds to hydrogen (emdee_md_set_hbonds) of a bond graph: every non-hydrogen atom together with the
    one, two or three hydrogens bonded to it.  Hydrogen is decided by the `element` attribute of the atom's type
    (table.elements).  skip: atom ids to leave out, centres and hydrogens alike (those of rigid_triatomics, which stay with
    emdee_md_set_rigid3).  Returns (atoms, dist):
      atoms (n, 4) int64 {centre, h1, h2, h3}, hydrogens ascending, -1 in the unused trailing slots; dist (n, 3) float64, the
        r0 of each bond's entry / length_unit, 0 in the unused slots;
    with_dropped: (atoms, dist, drop_bonds), the last the (m, 2) ids (i < j) of the bonds the constraints replace, as topology()
    writes them.
    Raises KeyError for a bond the table has no entry for, ValueError for a hydrogen bonded to two atoms or to another hydrogen,
    or a centre with more than three hydrogens."""
    n = len(types)
    skip = {int(a) for a in np.asarray(skip, dtype=np.int64).ravel()}
    nb = [set() for _ in range(n)]
    for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2):
        nb[i].add(int(j)); nb[j].add(int(i))
    is_h = [table.elements.get(t) == "H" for t in types]
    for h in range(n):
        if is_h[h] and h not in skip and nb[h]:
            if len(nb[h]) != 1:
                raise ValueError("hydrogen %d (type %s) is bonded to %d atoms" % (h, types[h], len(nb[h])))
            if is_h[next(iter(nb[h]))]:
                raise ValueError("hydrogen %d (type %s) is bonded to another hydrogen" % (h, types[h]))
    atoms, dist, drop = [], [], []
    for c in range(n):
        if is_h[c] or c in skip:
            continue
        hs = sorted(h for h in nb[c] if is_h[h] and h not in skip)
        if not hs:
            continue
        if len(hs) > 3:
            raise ValueError("atom %d (type %s) is bonded to %d hydrogens (a cluster holds at most three)" % (c, types[c], len(hs)))
        row = []
        for h in hs:
            bond = table.bond(types[c], types[h])
            if bond is None:
                raise KeyError("no bond parameters for atoms %s (types %s)" % ((c, h), (types[c], types[h])))
            row.append(bond[0][1] / length_unit)
            drop.append((min(c, h), max(c, h)))
        atoms.append([c] + hs + [-1] * (3 - len(hs)))
        dist.append(row + [0.0] * (3 - len(hs)))
    arr = lambda v, m, dt=np.int64: np.array(v, dtype=dt).reshape(-1, m)
    out = (arr(atoms, 4), arr(dist, 3, np.float64))
    return out + (arr(sorted(drop), 2),) if with_dropped else out


def molecules(n_atoms, bonds):
    """The molecule table (emdee_md_set_molecules) of a bond graph: the connected components of `bonds` ((m, 2) ids, the full
    list, constrained bonds included) as an (n_atoms,) int32 array, one id per atom.  Ids are dense and in order of first
    appearance by atom id; an atom without a bond is a molecule of one and gets -1.  Union-find with path halving, plain Python."""
    n_atoms = int(n_atoms)
    root = list(range(n_atoms))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2):
        i, j = int(i), int(j)
        if not (0 <= i < n_atoms and 0 <= j < n_atoms):
            raise ValueError("molecules: bond (%d, %d) names an atom outside [0, %d)" % (i, j, n_atoms))
        a, b = find(i), find(j)
        if a != b:
            root[max(a, b)] = min(a, b)
    roots = [find(a) for a in range(n_atoms)]
    size = np.bincount(np.array(roots, dtype=np.int64), minlength=n_atoms) if n_atoms else np.zeros(0, dtype=np.int64)
    ids, out = {}, np.full(n_atoms, -1, dtype=np.int32)
    for a, r in enumerate(roots):
        if size[r] >= 2:
            out[a] = ids.setdefault(r, len(ids))
    return out


def save_checkpoint(path, positions, velocities, step, box_length):
    """(x, v, step, L) as a compressed npz; accepts GPU tensors or numpy arrays."""
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    np.savez_compressed(path, positions=to_np(positions), velocities=to_np(velocities), step=int(step), L=float(box_length))


def load_checkpoint(path):
    d = np.load(path)
    return d["positions"], d["velocities"], int(d["step"]), float(d["L"])
