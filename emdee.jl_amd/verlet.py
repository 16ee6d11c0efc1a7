"""Velocity-Verlet on the device.  Build-defined: the reference has no integrator (SURVEY.md 8a
row a16); the API follows EmDee's operator style (constructor + `!` mutators spelled `_`)."""
import ctypes as C

import torch

from . import _lib
from .device import check_array, context_for, precision_of
from .nonbonded import ENERGIES, FORCES, VIRIALS, check_tensor_out, tensor_matrix

HARMONIC_BOND, HARMONIC_ANGLE, PERIODIC_TORSION = 1, 2, 3
_BONDED_SHAPE = {HARMONIC_BOND: (2, 2), HARMONIC_ANGLE: (3, 2), PERIODIC_TORSION: (4, 3)}

# Coulomb's constant 1 / (4 pi eps0) in kJ mol^-1 nm e^-2 (CODATA 2018 e, eps0 and N_A): the K of set_coulomb_ in the units of
# the force-field files the library ingests
COULOMB_K_KJ_NM = 138.935457644

# pressure coupling (include/emdee_hip.h: emdee_md_set_barostat)
BAROSTAT_OFF, BAROSTAT_BERENDSEN, BAROSTAT_CRESCALE = 0, 1, 2
COUPLE_ISOTROPIC, COUPLE_SEMIISOTROPIC, COUPLE_ANISOTROPIC = 0, 1, 2
_COUPLINGS = {"isotropic": COUPLE_ISOTROPIC, "semiisotropic": COUPLE_SEMIISOTROPIC, "anisotropic": COUPLE_ANISOTROPIC}
_BAROSTATS = {"off": BAROSTAT_OFF, "berendsen": BAROSTAT_BERENDSEN, "c-rescale": BAROSTAT_CRESCALE, "crescale": BAROSTAT_CRESCALE}

# global thermostats (include/emdee_hip.h: emdee_md_set_thermostat)
THERMOSTAT_OFF, THERMOSTAT_VRESCALE, THERMOSTAT_NOSE_HOOVER = 0, 1, 2
THERMOSTAT_WORDS, THERMOSTAT_CHAIN_MAX = 20, 8
_THERMOSTATS = {"off": THERMOSTAT_OFF, "v-rescale": THERMOSTAT_VRESCALE, "vrescale": THERMOSTAT_VRESCALE,
                "nose-hoover": THERMOSTAT_NOSE_HOOVER, "nosehoover": THERMOSTAT_NOSE_HOOVER}

# mean-squared displacement and velocity autocorrelation (include/emdee_hip.h: emdee_md_set_msd)
MSD, VACF, MSD_WORDS = 1, 2, 7
# Green-Kubo observables (include/emdee_hip.h: emdee_md_set_gk)
GK_STRESS, GK_HEAT, GK_WORDS = 1, 2, 9
# spatial profiles (include/emdee_hip.h: emdee_md_set_spatial)
SPATIAL_X, SPATIAL_Y, SPATIAL_Z, SPATIAL_RADIAL = 0, 1, 2, 3
SPATIAL_DENSITY, SPATIAL_KINETIC, SPATIAL_STRESS, SPATIAL_WORDS = 1, 2, 4, 10
_SPATIAL_GEOMETRIES = {"x": SPATIAL_X, "y": SPATIAL_Y, "z": SPATIAL_Z, "radial": SPATIAL_RADIAL}
RESTRAINT_WORDS = 8                                        # (EMDEE_RESTRAINT_WORDS)
# the centre-of-mass pull (include/emdee_hip.h: emdee_md_set_pull)
PULL_WORDS, PULL_UMBRELLA, PULL_CONSTANT_FORCE, PULL_DISTANCE, PULL_DIRECTION = 8, 1, 2, 1, 2
_PULL_KINDS = {"umbrella": PULL_UMBRELLA, "constant-force": PULL_CONSTANT_FORCE, "constant_force": PULL_CONSTANT_FORCE}
_PULL_GEOMETRIES = {"distance": PULL_DISTANCE, "direction": PULL_DIRECTION}
ALCH_WORDS, ALCH_MAX_FOREIGN = 5, 16                       # (EMDEE_ALCH_WORDS, EMDEE_ALCH_MAX_FOREIGN: emdee_md_set_alchemical)
ALCH_COULOMB_WORDS = 4                                     # (EMDEE_ALCH_COULOMB_WORDS: emdee_md_set_alchemical_coulomb)


def _three(v):
    """a scalar or three numbers as three floats"""
    try:
        out = [float(t) for t in v]
    except TypeError:
        out = [float(v)] * 3
    if len(out) != 3:
        raise ValueError("expected a scalar or three numbers, got %d" % len(out))
    return out


def charge_array(charges, device):
    """charges as a contiguous float64 device vector (None: empty)."""
    return torch.as_tensor(charges if charges is not None else [], dtype=torch.float64).reshape(-1).to(device=device).contiguous()


def bonded_arrays(kind, atoms, params, device, id_dtype):
    """(atoms, params) of one bonded kind as contiguous device tensors (ids of id_dtype, parameters float64).  An unknown kind
    keeps 2 ids and 2 parameters per term, so that the library is the one to refuse it."""
    na, npar = _BONDED_SHAPE.get(int(kind), (2, 2))
    a = torch.as_tensor(atoms if atoms is not None else []).reshape(-1, na).to(device=device, dtype=id_dtype).contiguous()
    p = torch.as_tensor(params if params is not None else [], dtype=torch.float64).reshape(-1, npar).to(device=device).contiguous()
    if a.shape[0] != p.shape[0]:
        raise ValueError("set_bonded_: %d terms but %d parameter rows" % (a.shape[0], p.shape[0]))
    return a, p


KERNELS = {"lj_force_nbr": 0, "verlet_kick_drift": 1, "rebuild": 2, "verlet_kick": 3, "lj_force_nbr_fused_step": 4,
           # decomposed steps: the fused launches over interior bricks (or all bricks, in-order form), over boundary bricks, and the
           # halo (pack -> exchange -> unpack) on the stream it runs on
           "fused_step_interior": 5, "fused_step_boundary": 6, "halo": 7,
           # the reciprocal-space pass of an Ewald engine (set_ewald_, set_pme_); "lj_force_nbr" contains it as well
           "ewald_reciprocal": 8,
           # the constraint stages of an engine with rigid molecules (set_rigid3_)
           "settle": 9,
           # the molecular sums and the molecular scale of an engine with rigid molecules (set_molecular_scaling_) or a molecule
           # table (set_molecules_: the centres, then the entries' pass or the shift)
           "molecular": 10,
           # the constraint stages of an engine with an hbonds table (set_hbonds_)
           "hbonds": 11,
           # what minimize_ adds to the stages of its steps: the constrained force, the reduction, the mixing
           "minimize": 12,
           # placement and force spreading of an engine with virtual sites (set_vsites_)
           "vsites": 13,
           # the three launches of every event of a global thermostat (set_thermostat_)
           "thermostat": 14,
           # the four stages of every sample of the radial distribution functions (rdf_sample_)
           "rdf": 15,
           # the three launches of every sample of the displacement and velocity correlations (msd_sample_)
           "msd": 16,
           # the launches every sample of the Green-Kubo observables adds to the tensor pass (gk_sample_): 4 per mask bit alone
           # (5 for the stress of an engine with rigid molecules), 6 with both
           "green_kubo": 17,
           # the launch the position restraints add to every force pass, and the scaling of their references (set_restraints_)
           "restraints": 18,
           # the three launches the centre-of-mass pull adds to every force pass (set_pull_): partial sums, finish, apply
           "pull": 19,
           # the row pass of the alchemical table at every rebuild and its launches behind every force pass (set_alchemical_)
           "alchemical": 20,
           # the launches of every sample of the spatial profiles (spatial_sample_): gather, accumulate, finish, and two more ahead
           # of them with a centre group
           "spatial": 21}


def spatial_profiles(geometry, edges, counts, sums, outside, group_sizes, frames, inv_bin_volume_sum):
    """What follows from the words of emdee_md_spatial_read, as a dict.  edges: the n_bins + 1 bin edges (positions along the axis,
    or radii); counts (n_groups, n_bins), sums (n_groups, n_bins, 10).  bin_volume: planar frames / inv_bin_volume_sum (the harmonic
    mean over the frames' boxes), radial the shells' 4 pi / 3 (r_{k+1}^3 - r_k^3).  Densities and pressures are per frame and per
    bin volume; velocity = sum m v / sum m; kinetic_energy = sum m v^2 / 2 per atom, kinetic_normal the share of the normal
    component, kinetic_tangential that of ONE tangential component (no Boltzmann constant is applied: a temperature is twice a
    component's share, over k_B); p_normal = (w6 + w9) / V, p_tangential = ((w5 - w6) + (w8 - w9)) / (2 V).  Planar geometries
    add gamma_sum = sum_k (P_N - P_T)_k times the bin width: the sum over every interface crossed.  NaN where nothing was counted."""
    import numpy as np
    edges = np.asarray(edges, dtype=np.float64)
    counts, sums = np.asarray(counts, dtype=np.int64), np.asarray(sums, dtype=np.float64)
    frames = int(frames)
    if int(geometry) == SPATIAL_RADIAL:
        volume = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    else:
        volume = np.full(edges.shape[0] - 1, frames / inv_bin_volume_sum if inv_bin_volume_sum > 0.0 else np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        per = 1.0 / (frames * volume)[None, :] if frames > 0 else np.full((1, volume.shape[0]), np.nan)
        n = counts.astype(np.float64)
        velocity = np.where(sums[..., 0:1] != 0.0, sums[..., 2:5] / sums[..., 0:1], np.nan)
        kinetic = np.where(n > 0, 0.5 * sums[..., 5] / n, np.nan)
        kinetic_n = np.where(n > 0, 0.5 * sums[..., 6] / n, np.nan)
        kinetic_t = np.where(n > 0, 0.25 * (sums[..., 5] - sums[..., 6]) / n, np.nan)
        p_n = (sums[..., 6] + sums[..., 9]) * per
        p_t = 0.5 * ((sums[..., 5] - sums[..., 6]) + (sums[..., 8] - sums[..., 9])) * per
    out = dict(edges=edges, centres=0.5 * (edges[1:] + edges[:-1]), bin_volume=volume, counts=counts, sums=sums,
               outside=[int(t) for t in outside], group_sizes=[int(t) for t in group_sizes], frames=frames,
               inv_bin_volume_sum=float(inv_bin_volume_sum), number_density=n * per, mass_density=sums[..., 0] * per,
               charge_density=sums[..., 1] * per, velocity=velocity, kinetic_energy=kinetic, kinetic_normal=kinetic_n,
               kinetic_tangential=kinetic_t, energy_density=sums[..., 7] * per, p_normal=p_n, p_tangential=p_t)
    if int(geometry) != SPATIAL_RADIAL:
        out["gamma_sum"] = ((p_n - p_t) * (edges[1:] - edges[:-1])[None, :]).sum(axis=1)
    return out


class MinimizeResult:
    """emdee_minimize_result as attributes: iterations, converged (bool), rebuilds, energy0, energy, g_max, dt"""

    def __init__(self, c):
        self.iterations, self.converged, self.rebuilds = int(c.iterations), bool(c.converged), int(c.rebuilds)
        self.energy0, self.energy, self.g_max, self.dt = float(c.energy0), float(c.energy), float(c.g_max), float(c.dt)

    def __repr__(self):
        return ("MinimizeResult(iterations=%d, converged=%s, rebuilds=%d, energy0=%r, energy=%r, g_max=%r, dt=%r)"
                % (self.iterations, self.converged, self.rebuilds, self.energy0, self.energy, self.g_max, self.dt))


class VelocityVerlet:
    """v += (dt/2m) f ; x += dt v ; f = F(x) ; v += (dt/2m) f, with the state kept in cell order in
    HBM between steps.  positions (n_owned + n_ghost, 3), velocities (n_owned, 3), atoms
    (n_owned + n_ghost, 2) float32 [LJAtom], inv_mass (n_owned,) or None (m = 1).

    Single-GPU, reference-shaped box: VelocityVerlet(x, v, L, model, atoms).
    Domain-decomposed: pass lo/lengths/periodic and n_ghost, and drive kick_drift_/forces_/kick_."""

    _coupled = False                                       # set_barostat_ has switched pressure coupling on

    def __init__(self, positions, velocities, L, model, atoms, skin=0.3, inv_mass=None, lo=None, lengths=None,
                 periodic=None, n_ghost=0):
        n_total = positions.shape[0]
        n_owned = n_total - int(n_ghost)
        dev, dt = positions.device, positions.dtype
        self.n_owned, self.n_ghost, self.device, self.dtype = n_owned, int(n_ghost), dev, dt
        self.model = model
        self._ctx = context_for(dev)
        lo = [0.0, 0.0, 0.0] if lo is None else [float(v) for v in lo]
        lengths = [float(L)] * 3 if lengths is None else [float(v) for v in lengths]
        periodic = [1, 1, 1] if periodic is None else [int(bool(v)) for v in periodic]
        self.lo, self.lengths, self.periodic = lo, lengths, periodic
        h = C.c_void_p()
        _lib.call("emdee_md_create", self._ctx.handle, (C.c_double * 3)(*lo), (C.c_double * 3)(*lengths),
                  (C.c_int32 * 3)(*periodic), _lib.model_c(model), float(skin), precision_of(positions), C.byref(h))
        self._handle = h
        self.set_state_(positions, velocities, atoms, inv_mass, n_ghost)

    def set_state_(self, positions, velocities, atoms, inv_mass=None, n_ghost=0):
        n_total = positions.shape[0]
        n_owned = n_total - int(n_ghost)
        check_array(positions, "positions", n_total, 3, self.dtype, self.device)
        check_array(velocities, "velocities", n_owned, 3, self.dtype, self.device)
        check_array(atoms, "atoms", n_total, 2, torch.float32, self.device)
        if inv_mass is not None:
            check_array(inv_mass, "inv_mass", n_owned, None, self.dtype, self.device)
        self.n_owned, self.n_ghost = n_owned, int(n_ghost)
        self._langevin_ids = None                      # the library forgets the id array with the old state
        _lib.call("emdee_md_set_state", self._handle, n_owned, int(n_ghost), C.c_void_p(positions.data_ptr()),
                  C.c_void_p(velocities.data_ptr()), C.c_void_p(atoms.data_ptr()),
                  C.c_void_p(inv_mass.data_ptr()) if inv_mass is not None else None)

    # -- whole steps (single domain)
    def step_(self, nsteps, dt, rebuild_every=0):
        try:
            _lib.call("emdee_md_step", self._handle, int(nsteps), float(dt), int(rebuild_every))
        finally:
            if self._coupled:
                self.box()                                  # (the coupling events of the call have changed the lengths)

    def minimize_(self, max_iter, f_tol, dt_start=0.001, dt_max=0.01, max_step=0.1):
        """Energy minimisation by FIRE around the constrained step (include/emdee_hip.h emdee_md_minimize): at most max_iter
        iterations, until no atom's constrained force exceeds f_tol.  dt_start, dt_max: FIRE's first and largest time step;
        max_step: the farthest an atom may drift in one iteration.  OVERWRITES the velocities with zeros.  Returns a
        MinimizeResult."""
        res = _lib.MinimizeResultC()
        _lib.call("emdee_md_minimize", self._handle, int(max_iter), float(f_tol), float(dt_start), float(dt_max), float(max_step),
                  C.byref(res))
        return MinimizeResult(res)

    # -- split step (domain-decomposed driver: kick_drift_ -> halo exchange -> forces_ -> kick_)
    def kick_drift_(self, dt, kick=0.5):
        """v += kick dt f/m ; x += dt v.  kick = 1.0 fuses the previous step's closing half kick."""
        _lib.call("emdee_md_kick_drift", self._handle, float(dt), float(kick))

    def forces_(self, bitmask=FORCES, phase=0):
        """phase 0: all; 1: interior bricks (no ghost in their tile); 2: boundary bricks."""
        _lib.call("emdee_md_forces", self._handle, int(bitmask), int(phase))

    def kick_(self, dt):
        _lib.call("emdee_md_kick", self._handle, float(dt))

    def fused_step_(self, dt, kick=1.0, phase=0):
        """One inner step as one kernel (force + kick + drift, positions ping-ponged).  Returns False, having
        done nothing, when the LDS-tiled kernels are not in use for this box."""
        ok = C.c_int32(0)
        _lib.call("emdee_md_fused_step", self._handle, float(dt), float(kick), int(phase), C.byref(ok))
        return bool(ok.value)

    def needs_rebuild(self):
        f = C.c_int32()
        _lib.call("emdee_md_needs_rebuild", self._handle, C.byref(f))
        return bool(f.value)

    def rebuild_(self):
        _lib.call("emdee_md_rebuild", self._handle)

    def pack_positions(self, ids, shifts, codes=None, out=None):
        """Positions of caller-order ids (int32 GPU tensor) plus shifts[codes[k]] (flat list of 3-vectors;
        codes None: every atom uses shifts[0:3]) -> (n, 3) buffer for the halo exchange."""
        n = ids.shape[0]
        if out is None:
            out = torch.empty((n, 3), dtype=self.dtype, device=self.device)
        flat = [float(s) for s in shifts]
        _lib.call("emdee_md_pack_positions", self._handle, C.c_void_p(ids.data_ptr()),
                  C.c_void_p(codes.data_ptr()) if codes is not None else None, n,
                  (C.c_double * len(flat))(*flat), len(flat) // 3, C.c_void_p(out.data_ptr()))
        return out

    def unpack_ghosts_(self, buf, first):
        _lib.call("emdee_md_unpack_ghosts", self._handle, C.c_void_p(buf.data_ptr()), int(first), buf.shape[0])

    # -- state back in caller order
    def state(self, positions=True, velocities=True, forces=True, energies=False, virials=False):
        n, nt = self.n_owned, self.n_owned + self.n_ghost
        mk = lambda rows, cols: torch.empty((rows, cols) if cols else (rows,), dtype=self.dtype, device=self.device)
        out = dict(positions=mk(nt, 3) if positions else None, velocities=mk(n, 3) if velocities else None,
                   forces=mk(n, 3) if forces else None, energies=mk(n, 0) if energies else None,
                   virials=mk(n, 0) if virials else None)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.call("emdee_md_get_state", self._handle, p(out["positions"]), p(out["velocities"]), p(out["forces"]),
                  p(out["energies"]), p(out["virials"]))
        return out

    def totals(self):
        """(potential energy, kinetic energy, virial sum) over owned atoms; fp64 reduction (blocking)."""
        out = (C.c_double * 3)()
        _lib.call("emdee_md_energies", self._handle, out)
        return out[0], out[1], out[2]

    def observables(self, volume=None, n_atoms=None):
        """Instantaneous thermodynamic state from the on-device reductions, reduced units:
        T = 2 KE / (3 N - 3) (centre-of-mass momentum removed), P = (2 KE + sum W) / (3 V) -- the per-atom virials
        w_i already hold half of every pair's -r dE/dr, so sum W is the pair virial.  Decomposed runs pass the
        global volume / atom count and sum the totals over ranks first (DecomposedVerlet.observables)."""
        ep, ek, vir = self.totals()
        n = self.n_owned if n_atoms is None else n_atoms
        v = self.lengths[0] * self.lengths[1] * self.lengths[2] if volume is None else volume
        return dict(potential=ep, kinetic=ek, virial=vir, temperature=2.0 * ek / max(3 * n - 3, 1),
                    pressure=(2.0 * ek + vir) / (3.0 * v), density=n / v)

    def virial_tensor(self, out=None):
        """Per-atom virial tensors of the owned atoms, (n_owned, 6) in caller order, columns (xx, yy, zz, xy, xz, yz)
        (compute_virial_tensor_'s convention).  One extra pass over the list if they are not current; the forces and the
        trajectory are left as they are."""
        if out is None:
            out = torch.empty((self.n_owned, 6), dtype=self.dtype, device=self.device)
        check_tensor_out(out, self.n_owned, self.dtype)
        _lib.call("emdee_md_virial_tensor", self._handle, C.c_void_p(out.data_ptr()))
        return out

    def tensor_sums(self):
        """The twelve fp64 sums of emdee_md_pressure_tensor: sum of W_i (6), kinetic tensor sum m v v (6) (blocking)."""
        out = (C.c_double * 12)()
        _lib.call("emdee_md_pressure_tensor", self._handle, out)
        return list(out)

    def pressure_tensor(self, volume=None):
        """dict(virial=W, kinetic=K, pressure=(K + W) / V) as 3 x 3 numpy arrays: W the sum of the per-atom virial tensors,
        K = sum m v (x) v over owned atoms, so that trace(pressure) / 3 is observables()["pressure"]."""
        v = self.lengths[0] * self.lengths[1] * self.lengths[2] if volume is None else volume
        return pressure_tensor_dict(self.tensor_sums(), v)

    def molecular_tensor_sums(self):
        """The twelve fp64 sums of emdee_md_molecular_pressure_tensor: W_mol (6), K_mol (6) -- tensor_sums() minus what the atoms
        of the rigid molecules (set_rigid3_), or of the molecules of set_molecules_ with set_molecular_scaling_ on, carry about
        their centres of mass; without a table, tensor_sums() itself (blocking)."""
        out = (C.c_double * 12)()
        _lib.call("emdee_md_molecular_pressure_tensor", self._handle, out)
        return list(out)

    def molecular_pressure_tensor(self, volume=None):
        """pressure_tensor() from the molecular sums: dict(virial=W_mol, kinetic=K_mol, pressure=(K_mol + W_mol) / V), the
        pressure an engine with rigid molecules couples to under set_molecular_scaling_."""
        v = self.lengths[0] * self.lengths[1] * self.lengths[2] if volume is None else volume
        return pressure_tensor_dict(self.molecular_tensor_sums(), v)

    def nbr_stats(self):
        b, l, m, c = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        _lib.call("emdee_md_nbr_stats", self._handle, C.byref(b), C.byref(l), C.byref(m), C.byref(c))
        return dict(builds=b.value, listed=l.value, max_count=m.value, capacity=c.value)

    def count_pairs(self):
        n = C.c_int64()
        _lib.call("emdee_md_count_pairs", self._handle, C.byref(n))
        return n.value

    def neighbor_lists(self):
        """The current list as caller ids: (counts (n_owned,), neighbors (n_owned, capacity)) int32, list order."""
        cap = max(self.nbr_stats()["capacity"], 1)
        counts = torch.zeros(self.n_owned, dtype=torch.int32, device=self.device)
        nb = torch.full((self.n_owned, cap), -1, dtype=torch.int32, device=self.device)
        _lib.call("emdee_md_nbr_list", self._handle, C.c_void_p(counts.data_ptr()), C.c_void_p(nb.data_ptr()), cap)
        return counts, nb

    def profile_(self, enable=True):
        _lib.call("emdee_md_profile", self._handle, int(bool(enable)))

    def kernel_time(self, kernel):
        """(total device ms, launches) of a kernel since profile_(True): HIP events on the stream."""
        ms, k = C.c_double(), C.c_int64()
        _lib.call("emdee_md_kernel_time", self._handle, KERNELS[kernel] if isinstance(kernel, str) else int(kernel),
                  C.byref(ms), C.byref(k))
        return ms.value, k.value

    # -- Langevin thermostat
    def set_langevin_(self, gamma, temperature, seed=0, first_step=0):
        """gamma > 0: every later step does v = c1 v + c2 sqrt(T/m) xi between its kick and its drift
        (include/emdee_hip.h: emdee_md_set_langevin); gamma <= 0 switches the thermostat off."""
        _lib.call("emdee_md_set_langevin", self._handle, float(gamma), float(temperature), int(seed) & (2 ** 64 - 1),
                  int(first_step))

    def set_langevin_ids_(self, ids):
        """int64 ids (device, caller order, owned atoms) keying the noise; None = the caller index.  Must be set
        again after every set_state_."""
        if ids is not None:
            check_array(ids, "ids", self.n_owned, None, torch.int64, self.device)
        self._langevin_ids = ids
        _lib.call("emdee_md_set_langevin_ids", self._handle, C.c_void_p(ids.data_ptr()) if ids is not None else None)

    def langevin_normals(self, seed, step, ids):
        """The thermostat's generator on its own: (len(ids), 3) float64 tensor of N(0,1) numbers."""
        ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty((ids.shape[0], 3), dtype=torch.float64, device=self.device)
        _lib.call("emdee_md_langevin_normals", self._handle, int(seed) & (2 ** 64 - 1), int(step),
                  C.c_void_p(ids.data_ptr()), int(ids.shape[0]), C.c_void_p(out.data_ptr()))
        return out

    # -- pressure coupling (include/emdee_hip.h: emdee_md_get_box, emdee_md_scale_box, emdee_md_set_barostat; undivided boxes)
    def box(self):
        """(lo, lengths) of the engine's box as two lists; also refreshes self.lengths, the volume observables() and
        pressure_tensor() divide by."""
        lo, ln = (C.c_double * 3)(), (C.c_double * 3)()
        _lib.call("emdee_md_get_box", self._handle, lo, ln)
        self.lo, self.lengths = list(lo), list(ln)
        return list(lo), list(ln)

    def scale_box_(self, mu, velocity_scale=1.0):
        """x <- lo + mu (x - lo) per axis, lengths <- mu lengths, v <- velocity_scale v; then re-bin, re-plan, rebuild and a
        force pass on the new box.  mu: a scalar or three factors.  All or nothing (EmDeeError code -1, nothing changed, for a
        factor that is not finite and > 0 or a periodic length that would fall below 2 (rc + skin))."""
        try:
            _lib.call("emdee_md_scale_box", self._handle, (C.c_double * 3)(*_three(mu)), float(velocity_scale))
        finally:
            self.box()

    def set_barostat_(self, kind, p_ref=0.0, compressibility=0.0, tau_p=1.0, every=1, coupling="isotropic", temperature=None,
                      seed=0, first_step=0):
        """Pressure coupling in every later step_: kind BAROSTAT_BERENDSEN / BAROSTAT_CRESCALE (or "berendsen" / "c-rescale"),
        BAROSTAT_OFF (or None, "off") switches it off.  p_ref and compressibility: a scalar or three entries (isotropic reads
        entry 0, semi-isotropic 0 for x, y and 2 for z); every: steps between events; coupling: "isotropic", "semiisotropic",
        "anisotropic" or a COUPLE_* constant; temperature (energy units), seed, first_step: C-rescale's noise."""
        if kind is None:
            kind = BAROSTAT_OFF
        k = _BAROSTATS[kind.lower()] if isinstance(kind, str) else int(kind)
        c = _COUPLINGS[coupling.lower().replace("-", "").replace("_", "")] if isinstance(coupling, str) else int(coupling)
        _lib.call("emdee_md_set_barostat", self._handle, k, c, (C.c_double * 3)(*_three(p_ref)),
                  (C.c_double * 3)(*_three(compressibility)), float(tau_p), int(every),
                  0.0 if temperature is None else float(temperature), int(seed) & (2 ** 64 - 1), int(first_step))
        self._coupled = k != BAROSTAT_OFF

    # -- global thermostats (include/emdee_hip.h: emdee_md_set_thermostat; undivided boxes)
    def set_thermostat_(self, kind, temperature=1.0, tau_t=1.0, every=1, n_dof=0, chain=3, seed=0, first_step=0):
        """A global thermostat in every later step_: kind THERMOSTAT_VRESCALE / THERMOSTAT_NOSE_HOOVER (or "v-rescale" /
        "nose-hoover"), THERMOSTAT_OFF (or None, "off") switches it off.  temperature: kT in energy units; tau_t: the relaxation
        time; every: steps between events; n_dof: the degrees of freedom, 0 for the library's own count from the tables in force;
        chain: the length of the Nose-Hoover chain (1...8); seed, first_step: v-rescale's noise and the numbering of the steps."""
        if kind is None:
            kind = THERMOSTAT_OFF
        k = _THERMOSTATS[kind.lower().replace("_", "-")] if isinstance(kind, str) else int(kind)
        _lib.call("emdee_md_set_thermostat", self._handle, k, float(temperature), float(tau_t), int(every), int(n_dof), int(chain),
                  int(seed) & (2 ** 64 - 1), int(first_step))

    def thermostat_state(self):
        """The thermostat's state words as a dict (blocking): n_dof in use, kinetic (K as the last event saw it, before its
        scaling), alpha (that event's factor), energy (E_th: U + K + E_th is the conserved quantity), xi and v_xi (8 each; unused
        chain slots are 0)."""
        w = (C.c_double * THERMOSTAT_WORDS)()
        _lib.call("emdee_md_thermostat_state", self._handle, w)
        w = list(w)
        return dict(n_dof=int(w[0]), kinetic=w[1], alpha=w[2], energy=w[3], xi=w[4:12], v_xi=w[12:20])

    def set_thermostat_state_(self, state):
        """Writes energy, xi and v_xi of a dict from thermostat_state() (the words a restart carries over; the others are the
        library's).  A restart: set_thermostat_(..., first_step=steps done), then this."""
        xi, v_xi = [float(t) for t in state["xi"]], [float(t) for t in state["v_xi"]]
        if len(xi) != THERMOSTAT_CHAIN_MAX or len(v_xi) != THERMOSTAT_CHAIN_MAX:
            raise ValueError("set_thermostat_state_: xi and v_xi take %d numbers each" % THERMOSTAT_CHAIN_MAX)
        w = [0.0, 0.0, 0.0, float(state["energy"])] + xi + v_xi
        _lib.call("emdee_md_set_thermostat_state", self._handle, (C.c_double * THERMOSTAT_WORDS)(*w))

    def thermostat_draws(self, seed, step, n_dof):
        """v-rescale's generator on its own: (R1, S) of the event that completes step `step` -- R1 ~ N(0,1), S chi-squared with
        n_dof - 1 degrees of freedom (blocking)."""
        out = (C.c_double * 2)()
        _lib.call("emdee_md_thermostat_draws", self._handle, int(seed) & (2 ** 64 - 1), int(step), int(n_dof), out)
        return out[0], out[1]

    def _per_atom_i32(self, fn, n_groups, **arrays):
        """The per-atom integer arrays of a set_rdf_ / set_msd_ call (name=values or name=None, `groups` first) as int32 device
        tensors of n_owned entries each, and n_groups (None: what groups implies -- its largest entry + 1, at least 1)."""
        out = [None if v is None else torch.as_tensor(v).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous() for v in arrays.values()]
        for name, t in zip(arrays, out):
            if t is not None and t.shape[0] != self.n_owned:
                raise ValueError("%s: %s holds %d entries, the state %d owned atoms" % (fn, name, t.shape[0], self.n_owned))
        g = out[0]
        if n_groups is None:
            n_groups = 1 if g is None or g.numel() == 0 else max(int(g.max().item()) + 1, 1)
        return out, int(n_groups)

    # -- radial distribution functions (include/emdee_hip.h: emdee_md_set_rdf; undivided periodic boxes)
    _rdf = None                                            # (r_max, n_bins, n_groups) of the table in force

    def set_rdf_(self, r_max, n_bins, groups=None, molecules=None, n_groups=None):
        """The table of the pair histograms rdf_sample_() fills: n_bins bins up to r_max (at most half the shortest box side).
        groups: None (every atom in one group) or one integer per owned atom, -1 to leave the atom out; there is one histogram
        per unordered pair of groups (n_groups: how many groups there are, 1...8; None: the largest entry of groups + 1).
        molecules: None, or one integer per owned atom; pairs with equal entries >= 0 are skipped.  n_bins = 0 clears the
        table.  Zeroes the accumulators."""
        (g, m), n_groups = self._per_atom_i32("set_rdf_", n_groups, groups=groups, molecules=molecules)
        _lib.call("emdee_md_set_rdf", self._handle, float(r_max), int(n_bins), n_groups,
                  C.c_void_p(g.data_ptr()) if g is not None else None, C.c_void_p(m.data_ptr()) if m is not None else None)
        self._rdf = (float(r_max), int(n_bins), n_groups) if int(n_bins) != 0 else None

    def rdf_sample_(self):
        """Adds the current positions to the histograms as one frame: queued on the stream, nothing read back, the run untouched."""
        _lib.call("emdee_md_rdf_sample", self._handle)

    def rdf_reset_(self):
        """Zeroes the counts, the frame count and the sum of 1 / V."""
        _lib.call("emdee_md_rdf_reset", self._handle)

    def rdf(self):
        """The accumulated histograms and what follows from them, as a dict (blocking): r (bin centres), edges, pairs (the
        (a, b) of every histogram, a <= b, in slot order), counts ((n_pairs, n_bins) int64 numpy), group_sizes, frames,
        inv_volume_sum, g ((n_pairs, n_bins): counts / (P_ab shell inv_volume_sum), P_ab = N_a N_b or N_a (N_a - 1) / 2; pairs
        skipped as intramolecular stay in P_ab) and coordination (the running number of b around a: cumulative counts, times 2
        for a == b, over N_a frames)."""
        import numpy as np
        if self._rdf is None:
            raise ValueError("rdf: no table is set (set_rdf_)")
        r_max, n_bins, n_groups = self._rdf
        pairs = [(a, b) for a in range(n_groups) for b in range(a, n_groups)]
        counts = np.zeros((len(pairs), n_bins), dtype=np.int64)
        sizes, frames, ivs = (C.c_int64 * 8)(), C.c_int64(), C.c_double()
        _lib.call("emdee_md_rdf_read", self._handle, counts.ctypes.data_as(C.c_void_p), sizes, C.byref(frames), C.byref(ivs))
        sizes = [int(s) for s in sizes][:n_groups]
        edges = r_max * np.arange(n_bins + 1, dtype=np.float64) / n_bins
        shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
        g, coordination = np.zeros(counts.shape), np.zeros(counts.shape)
        for s, (a, b) in enumerate(pairs):
            P = 0.5 * sizes[a] * (sizes[a] - 1) if a == b else float(sizes[a]) * sizes[b]
            ideal = P * shell * ivs.value
            if P > 0 and ivs.value > 0.0:
                g[s] = counts[s] / ideal
            if sizes[a] > 0 and frames.value > 0:
                coordination[s] = (2.0 if a == b else 1.0) * np.cumsum(counts[s]) / (float(sizes[a]) * frames.value)
        return dict(r=0.5 * (edges[1:] + edges[:-1]), edges=edges, pairs=pairs, counts=counts, group_sizes=sizes,
                    frames=int(frames.value), inv_volume_sum=float(ivs.value), g=g, coordination=coordination)

    # -- mean-squared displacement and velocity autocorrelation (include/emdee_hip.h: emdee_md_set_msd; undivided boxes)
    _msd = None                                            # (n_lags, n_groups) of the table in force

    def set_msd_(self, n_lags, origin_every=1, groups=None, n_groups=None, msd=True, vacf=True):
        """The table msd_sample_() fills: lags 0 ... n_lags - 1 (in samples), every origin_every-th sample an origin (at most 64
        origins within n_lags).  groups: None (every atom in one group) or one integer per owned atom, -1 to leave the atom out
        (n_groups: how many groups there are, 1...8; None: the largest entry of groups + 1).  msd / vacf: which of the two to
        keep (positions and velocities are stored only for the one that needs them).  n_lags = 0 clears the table.  Zeroes the
        sums and restarts the sample counter."""
        (g,), n_groups = self._per_atom_i32("set_msd_", n_groups, groups=groups)
        what = (MSD if msd else 0) | (VACF if vacf else 0)
        _lib.call("emdee_md_set_msd", self._handle, what, n_groups, C.c_void_p(g.data_ptr()) if g is not None else None,
                  int(n_lags), int(origin_every))
        self._msd = (int(n_lags), n_groups) if int(n_lags) != 0 else None

    def msd_sample_(self):
        """Takes the current state as the next sample: an origin when its number is a multiple of origin_every, and correlated
        with every origin within n_lags.  Queued on the stream, nothing read back, the run untouched."""
        _lib.call("emdee_md_msd_sample", self._handle)

    def msd_reset_(self):
        """Zeroes the sums, restarts the sample counter at 0 and takes the current box and state as the ones the origins belong to."""
        _lib.call("emdee_md_msd_reset", self._handle)

    def msd(self):
        """The accumulated sums and what follows from them, as a dict (blocking): lags (0 ... n_lags - 1, in samples), origins
        (per lag: how many origins have contributed), group_sizes, samples, sums ((n_lags, n_groups, 7) float64 numpy: the raw
        words of emdee_md_msd_read), msd ((n_lags, n_groups, 4): per axis and total, sums / (origins N_g)), msd_drift_free
        ((n_lags, n_groups): the total with the group's mean displacement taken out, per origin) and vacf ((n_lags, n_groups):
        <v(s) . v(0)> per atom).  NaN where origins N_g == 0."""
        import numpy as np
        if self._msd is None:
            raise ValueError("msd: no table is set (set_msd_)")
        n_lags, n_groups = self._msd
        sums = np.zeros((n_lags, n_groups, MSD_WORDS), dtype=np.float64)
        origins = np.zeros(n_lags, dtype=np.int64)
        sizes, samples = (C.c_int64 * 8)(), C.c_int64()
        _lib.call("emdee_md_msd_read", self._handle, sums.ctypes.data_as(C.c_void_p), origins.ctypes.data_as(C.c_void_p), sizes, C.byref(samples))
        sizes = np.array([int(s) for s in sizes][:n_groups], dtype=np.int64)
        count = origins[:, None].astype(np.float64) * sizes[None, :].astype(np.float64)
        ng = sizes[None, :].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            per_axis = np.where(count[..., None] > 0, sums[..., 0:3] / count[..., None], np.nan)
            total = np.where(count > 0, sums[..., 0:3].sum(axis=2) / count, np.nan)
            drift_free = np.where(count > 0, (sums[..., 0:3].sum(axis=2) - sums[..., 3:6].sum(axis=2) / ng) / count, np.nan)
            vacf = np.where(count > 0, sums[..., 6] / count, np.nan)
        return dict(lags=np.arange(n_lags), origins=origins, group_sizes=[int(s) for s in sizes], samples=int(samples.value), sums=sums,
                    msd=np.concatenate([per_axis, total[..., None]], axis=2), msd_drift_free=drift_free, vacf=vacf)

    # -- spatial profiles along an axis and around a centre (include/emdee_hip.h: emdee_md_set_spatial; undivided engines)
    _spatial = None                                        # (geometry, n_bins, n_groups, range) of the table in force

    def set_spatial_(self, geometry, n_bins, groups=None, n_groups=None, range=None, centre=None, centre_group=-1, density=True,
                     kinetic=True, stress=True):
        """The table spatial_sample_() fills.  geometry: "x", "y", "z" (planar slabs normal to that axis; range=None on a periodic
        axis, whose bins are fractions of the box, range=(r0, r1) on an open one) or "radial" (shells up to r_max: range=(0, r_max)
        or range=r_max; the centre is `centre`, or with centre_group >= 0 the centre of mass of that group, formed on the device
        at every sample).  groups / n_groups as set_msd_ takes them.  density / kinetic / stress: which words to keep (see
        spatial()).  n_bins = 0 clears the table.  Zeroes the sums."""
        geometry = _SPATIAL_GEOMETRIES[geometry] if isinstance(geometry, str) else int(geometry)
        (g,), n_groups = self._per_atom_i32("set_spatial_", n_groups, groups=groups)
        what = (SPATIAL_DENSITY if density else 0) | (SPATIAL_KINETIC if kinetic else 0) | (SPATIAL_STRESS if stress else 0)
        if range is not None:
            try:
                range = (float(range[0]), float(range[1]))
            except TypeError:
                range = (0.0, float(range))
        rng = (C.c_double * 2)(*range) if range is not None else None
        ctr = (C.c_double * 3)(*_three(centre)) if centre is not None else None
        _lib.call("emdee_md_set_spatial", self._handle, geometry, what, int(n_bins), n_groups,
                  C.c_void_p(g.data_ptr()) if g is not None else None, rng, ctr, int(centre_group))
        self._spatial = (geometry, int(n_bins), n_groups, range) if int(n_bins) != 0 else None

    def spatial_sample_(self):
        """Adds the current state to the profiles as one frame: queued on the stream, nothing read back, the run untouched (with
        stress the tensor pass is evaluated first if it is not current)."""
        _lib.call("emdee_md_spatial_sample", self._handle)

    def spatial_reset_(self):
        """Zeroes the counts, the sums, outside, the frame count and the sum of 1 / V_bin."""
        _lib.call("emdee_md_spatial_reset", self._handle)

    def spatial(self):
        """The accumulated profiles and what follows from them (spatial_profiles), as a dict (blocking): edges (of the current box
        on a periodic axis), centres, bin_volume, counts ((n_groups, n_bins) int64), sums ((n_groups, n_bins, 10): the raw words of
        emdee_md_spatial_read), outside, group_sizes, frames, inv_bin_volume_sum, number_density, mass_density, charge_density,
        velocity, kinetic_energy, kinetic_normal, kinetic_tangential, energy_density, p_normal, p_tangential and, planar,
        gamma_sum."""
        import numpy as np
        if self._spatial is None:
            raise ValueError("spatial: no table is set (set_spatial_)")
        geometry, n_bins, n_groups, rng = self._spatial
        counts = np.zeros((n_groups, n_bins), dtype=np.int64)
        sums = np.zeros((n_groups, n_bins, SPATIAL_WORDS), dtype=np.float64)
        outside, sizes, frames, ivs = (C.c_int64 * 8)(), (C.c_int64 * 8)(), C.c_int64(), C.c_double()
        _lib.call("emdee_md_spatial_read", self._handle, counts.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p), outside,
                  sizes, C.byref(frames), C.byref(ivs))
        if rng is None:
            lo, ln = self.box()
            rng = (float(lo[geometry]), float(lo[geometry]) + float(ln[geometry]))
        edges = rng[0] + (rng[1] - rng[0]) * np.arange(n_bins + 1, dtype=np.float64) / n_bins
        return spatial_profiles(geometry, edges, counts, sums, list(outside)[:n_groups], list(sizes)[:n_groups], frames.value, ivs.value)

    # -- Green-Kubo observables: stress and heat-flux autocorrelations (include/emdee_hip.h: emdee_md_set_gk; undivided engines)
    _gk = None                                             # n_lags of the table in force

    def set_green_kubo_(self, n_lags, stress=True, heat=True):
        """The table gk_sample_() fills: lags 0 ... n_lags - 1 (in samples, at most 65536), every sample an origin.  stress:
        words 0-4, the five independent traceless components of S = K + W (the molecular stress with set_rigid3_ in force), and
        word 5, trace(S) / 3 = p V; heat: words 6-8, the heat flux J = sum (k + e) v + sum W . v, for engines whose forces are
        all pair terms of the neighbour rows (Lennard-Jones, reaction-field charges).  n_lags = 0 clears the table.  Zeroes the
        sums and restarts the sample counter."""
        what = (GK_STRESS if stress else 0) | (GK_HEAT if heat else 0)
        _lib.call("emdee_md_set_gk", self._handle, what, int(n_lags))
        self._gk = int(n_lags) if int(n_lags) != 0 else None

    def gk_sample_(self):
        """Takes the current state as the next sample: its nine words go to the ring and are correlated with every sample
        within n_lags.  Queued on the stream, nothing read back, the run untouched."""
        _lib.call("emdee_md_gk_sample", self._handle)

    def gk_reset_(self):
        """Zeroes the sums, the totals and the ring, restarts the sample counter at 0 and takes the current box and state as
        the ones the run belongs to."""
        _lib.call("emdee_md_gk_reset", self._handle)

    def green_kubo(self, dt_sample=None, temperature=None):
        """The accumulated sums and what follows from them, as a dict (blocking): lags (0 ... n_lags - 1, in samples), counts
        (per lag: the products behind it, max(0, samples - lag)), sums ((n_lags, 9) float64 numpy: the raw words of
        emdee_md_gk_read), totals (9), last (9: the most recent sample), samples; stress_acf (the mean of words 0-4 over
        counts: <P_ab(0) P_ab(t)> V^2 averaged over the five independent traceless components), pressure_acf (word 5 over
        counts minus (totals[5] / samples)^2: the fluctuation of p V; the mean is taken over all samples and not over the
        counts[l] pairs of lag l, so the estimate is biased by end effects of relative order l / samples), heat_acf (the mean
        of words 6-8 over counts).  NaN where counts == 0.  With dt_sample (the time between two samples) and temperature (kT,
        in energy units) both given, the trapezoid running integrals eta = int stress_acf / (V kT) and
        lambda_ = int heat_acf / (V kT^2), V the current box."""
        import numpy as np
        if self._gk is None:
            raise ValueError("green_kubo: no table is set (set_green_kubo_)")
        n_lags = self._gk
        sums = np.zeros((n_lags, GK_WORDS), dtype=np.float64)
        totals, last, samples = np.zeros(GK_WORDS), np.zeros(GK_WORDS), C.c_int64()
        _lib.call("emdee_md_gk_read", self._handle, sums.ctypes.data_as(C.c_void_p), totals.ctypes.data_as(C.c_void_p),
                  last.ctypes.data_as(C.c_void_p), C.byref(samples))
        n = int(samples.value)
        lags = np.arange(n_lags)
        counts = np.maximum(n - lags, 0).astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(counts[:, None] > 0, sums / counts[:, None].astype(np.float64), np.nan)
            stress_acf = mean[:, 0:5].mean(axis=1)
            pressure_acf = mean[:, 5] - (totals[5] / n) ** 2 if n > 0 else np.full(n_lags, np.nan)
            heat_acf = mean[:, 6:9].mean(axis=1)
        out = dict(lags=lags, counts=counts, sums=sums, totals=totals, last=last, samples=n, stress_acf=stress_acf,
                   pressure_acf=pressure_acf, heat_acf=heat_acf)
        if dt_sample is not None and temperature is not None:
            _, ln = self.box()
            volume, kt = ln[0] * ln[1] * ln[2], float(temperature)

            def running(acf):
                steps = 0.5 * (acf[1:] + acf[:-1]) * float(dt_sample)
                return np.concatenate([[0.0], np.cumsum(steps)])
            out["eta"] = running(stress_acf) / (volume * kt)
            out["lambda_"] = running(heat_acf) / (volume * kt * kt)
        return out

    def set_molecular_scaling_(self, on=True):
        """Molecular scaling (include/emdee_hip.h emdee_md_set_molecular_scaling): with it on, an engine with rigid molecules
        (set_rigid3_) accepts scale_box_ and set_barostat_ -- molecules are translated with their centres of mass, and the
        coupling takes the molecular pressure.  Changes nothing for an engine without a table."""
        _lib.call("emdee_md_set_molecular_scaling", self._handle, int(on))

    def set_molecules_(self, molecule):
        """The molecule table (include/emdee_hip.h emdee_md_set_molecules): one int32 id per atom in caller order, equal ids >= 0
        form one molecule, -1 is a molecule of one (ingest.molecules builds the array from a bond list).  With
        set_molecular_scaling_ on, molecular_tensor_sums, scale_box_ and the barostats take whole molecules from it, and an engine
        with set_hbonds_ in force can be pressure-coupled.  Load every molecule whole.  None clears the table."""
        if molecule is None:
            _lib.call("emdee_md_set_molecules", self._handle, None, 0)
            return
        m = torch.as_tensor(molecule).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        _lib.call("emdee_md_set_molecules", self._handle, C.c_void_p(m.data_ptr()) if m.numel() else None, int(m.shape[0]))

    # -- exclusions and 1-4 pairs (include/emdee_hip.h; set after the state is loaded, undivided boxes)
    def set_exclusions_(self, pairs):
        t = torch.as_tensor(pairs if pairs is not None else []).reshape(-1, 2).to(device=self.device, dtype=torch.int32).contiguous()
        _lib.call("emdee_md_set_exclusions", self._handle, C.c_void_p(t.data_ptr()) if t.numel() else None, int(t.shape[0]))

    def set_pairs14_(self, pairs, lj14scale):
        t = torch.as_tensor(pairs if pairs is not None else []).reshape(-1, 2).to(device=self.device, dtype=torch.int32).contiguous()
        _lib.call("emdee_md_set_pairs14", self._handle, C.c_void_p(t.data_ptr()) if t.numel() else None, int(t.shape[0]), float(lj14scale))

    def set_bonded_(self, kind, atoms, params):
        """Bonded terms of one kind (HARMONIC_BOND, HARMONIC_ANGLE, PERIODIC_TORSION; include/emdee_hip.h emdee_md_set_bonded):
        atoms (n, 2 | 3 | 4) caller ids, params (n, 2 | 2 | 3).  Replaces that kind's table; an empty one clears it."""
        a, p = bonded_arrays(kind, atoms, params, self.device, torch.int32)
        _lib.call("emdee_md_set_bonded", self._handle, int(kind), C.c_void_p(a.data_ptr()) if a.numel() else None,
                  C.c_void_p(p.data_ptr()) if p.numel() else None, int(a.shape[0]))

    def set_coulomb_(self, charges, coulomb_k, eps_rf=float("inf"), coulomb14scale=1.0):
        """Reaction-field Coulomb forces (include/emdee_hip.h emdee_md_set_coulomb): charges (n,) in caller order, n the atom
        count; coulomb_k in the caller's units (COULOMB_K_KJ_NM for nm / kJ mol^-1 / e); eps_rf >= 1 (inf: the conducting
        boundary); coulomb14scale scales the 1-4 pairs of set_pairs14_.  Empty or None clears them."""
        q = charge_array(charges, self.device)
        _lib.call("emdee_md_set_coulomb", self._handle, C.c_void_p(q.data_ptr()) if q.numel() else None, int(q.shape[0]),
                  float(coulomb_k), float(eps_rf), float(coulomb14scale))

    def set_ewald_(self, alpha, kmax=None):
        """Ewald summation for a charged engine (include/emdee_hip.h emdee_md_set_ewald): alpha > 0, the splitting parameter (an
        inverse length), switches the Coulomb terms from the reaction field to the Ewald sum over the integer wave vectors
        |n_d| <= kmax[d] (one int for all three axes, or three); alpha = 0 switches back to the reaction field."""
        if kmax is None:
            arr = None
        else:
            k = [int(v) for v in kmax] if hasattr(kmax, "__len__") else [int(kmax)] * 3
            if len(k) != 3:
                raise ValueError("set_ewald_: kmax is one integer or three")
            arr = (C.c_int32 * 3)(*k)
        _lib.call("emdee_md_set_ewald", self._handle, float(alpha), arr)

    def set_pme_(self, alpha, grid=None, order=4):
        """Smooth particle-mesh Ewald for a charged engine (include/emdee_hip.h emdee_md_set_pme): alpha > 0 switches the
        reciprocal-space terms of the Ewald sum to a mesh of grid[d] points per axis (one int for all three axes, or three; powers
        of two in [8, 256]) with cardinal B-splines of the given order (4 or 6); the real-space terms are those of set_ewald_.
        alpha = 0 switches back to the reaction field.  Whichever of set_ewald_ and set_pme_ came last with alpha > 0 is in force."""
        if grid is None:
            arr = None
        else:
            g = [int(v) for v in grid] if hasattr(grid, "__len__") else [int(grid)] * 3
            if len(g) != 3:
                raise ValueError("set_pme_: grid is one integer or three")
            arr = (C.c_int32 * 3)(*g)
        _lib.call("emdee_md_set_pme", self._handle, float(alpha), arr, int(order))

    def set_rigid3_(self, atoms, geom):
        """Rigid three-site molecules (include/emdee_hip.h emdee_md_set_rigid3): atoms (n, 3) caller ids {apex, a, b}, geom (n, 2)
        {d_leg, d_base} with |apex - a| = |apex - b| = d_leg and |a - b| = d_base.  Every later step_ holds them rigid (SETTLE on
        the positions, RATTLE on the velocities).  Moves no atom; projects the velocities once.  Empty or None clears the table."""
        a = torch.as_tensor(atoms if atoms is not None else []).reshape(-1, 3).to(device=self.device, dtype=torch.int32).contiguous()
        g = torch.as_tensor(geom if geom is not None else [], dtype=torch.float64).reshape(-1, 2).to(device=self.device).contiguous()
        if a.shape[0] != g.shape[0]:
            raise ValueError("set_rigid3_: %d molecules but %d geometry rows" % (a.shape[0], g.shape[0]))
        _lib.call("emdee_md_set_rigid3", self._handle, C.c_void_p(a.data_ptr()) if a.numel() else None,
                  C.c_void_p(g.data_ptr()) if g.numel() else None, int(a.shape[0]))

    def set_hbonds_(self, atoms, dist):
        """Bonds to hydrogen at fixed lengths (include/emdee_hip.h emdee_md_set_hbonds): atoms (n, 4) caller ids {centre, s1, s2,
        s3} with -1 in the unused trailing slots, dist (n, 3) the centre-satellite distances (those of unused slots are ignored).
        Every later step_ holds them (M-SHAKE on the positions, RATTLE on the velocities).  Moves no atom; projects the velocities
        once.  Empty or None clears the table."""
        a = torch.as_tensor(atoms if atoms is not None else [])
        g = torch.as_tensor(dist if dist is not None else [], dtype=torch.float64)
        if a.numel() and (a.dim() != 2 or a.shape[1] != 4):
            raise ValueError("set_hbonds_: atoms must have shape (n, 4), got %s" % (tuple(a.shape),))
        if g.numel() and (g.dim() != 2 or g.shape[1] != 3):
            raise ValueError("set_hbonds_: dist must have shape (n, 3), got %s" % (tuple(g.shape),))
        a = a.reshape(-1, 4).to(device=self.device, dtype=torch.int32).contiguous()
        g = g.reshape(-1, 3).to(device=self.device).contiguous()
        if a.shape[0] != g.shape[0]:
            raise ValueError("set_hbonds_: %d clusters but %d rows of distances" % (a.shape[0], g.shape[0]))
        _lib.call("emdee_md_set_hbonds", self._handle, C.c_void_p(a.data_ptr()) if a.numel() else None,
                  C.c_void_p(g.data_ptr()) if g.numel() else None, int(a.shape[0]))

    def set_vsites_(self, atoms, weights):
        """Virtual interaction sites (include/emdee_hip.h emdee_md_set_vsites): atoms (n, 4) caller ids {site, a, b, c} with c = -1
        for a two-parent site, weights (n, 2) {w_b, w_c}; x_site = x_a + w_b (x_b - x_a) + w_c (x_c - x_a).  The sites are loaded
        with inv_mass = 0.  Zeroes the sites' velocities, places them, rebuilds the list and evaluates the forces; every later
        step_ and minimize_ keeps them on their parents and hands their forces to the parents.  Empty or None clears the table."""
        a = torch.as_tensor(atoms if atoms is not None else [])
        w = torch.as_tensor(weights if weights is not None else [], dtype=torch.float64)
        if a.numel() and (a.dim() != 2 or a.shape[1] != 4):
            raise ValueError("set_vsites_: atoms must have shape (n, 4), got %s" % (tuple(a.shape),))
        if w.numel() and (w.dim() != 2 or w.shape[1] != 2):
            raise ValueError("set_vsites_: weights must have shape (n, 2), got %s" % (tuple(w.shape),))
        a = a.reshape(-1, 4).to(device=self.device, dtype=torch.int32).contiguous()
        w = w.reshape(-1, 2).to(device=self.device).contiguous()
        if a.shape[0] != w.shape[0]:
            raise ValueError("set_vsites_: %d sites but %d rows of weights" % (a.shape[0], w.shape[0]))
        _lib.call("emdee_md_set_vsites", self._handle, C.c_void_p(a.data_ptr()) if a.numel() else None,
                  C.c_void_p(w.data_ptr()) if w.numel() else None, int(a.shape[0]))

    # -- position restraints (include/emdee_hip.h: emdee_md_set_restraints; undivided engines)
    _restraints = 0                                        # entries of the table in force

    def set_restraints_(self, atoms, k, ref=None, flat=None):
        """Position restraints (include/emdee_hip.h emdee_md_set_restraints): atoms (n,) caller ids; k the spring constants, a
        scalar, (n,) or (n, 3) per axis; ref (n, 3) in the coordinates state() returns (unwrapped; None: every named atom's current
        position); flat (n,) the flat-bottom radii r0 (None: all zero -- harmonic).  U = 1/2 sum k_a d_a^2, or 1/2 k max(0, rho -
        r0)^2 with rho over the axes with k_a > 0.  The references follow the box (scale_box_, the barostats).  Evaluates the forces
        again.  Empty or None atoms clears the table."""
        a = torch.as_tensor(atoms if atoms is not None else []).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        n = int(a.shape[0])
        kk = torch.as_tensor(k if k is not None else 0.0, dtype=torch.float64).to(device=self.device)
        if kk.dim() == 0:
            kk = kk.reshape(1, 1).expand(n, 3)
        elif kk.dim() == 1 and kk.shape[0] == n:
            kk = kk.reshape(n, 1).expand(n, 3)
        elif kk.dim() != 2 or tuple(kk.shape) != (n, 3):
            raise ValueError("set_restraints_: k is a scalar, (n,) or (n, 3) for n = %d atoms, got %s" % (n, tuple(kk.shape)))
        kk = kk.contiguous()
        r = f = None
        if ref is not None:
            r = torch.as_tensor(ref, dtype=torch.float64).to(device=self.device).contiguous()
            if tuple(r.shape) != (n, 3):
                raise ValueError("set_restraints_: ref must have shape (%d, 3), got %s" % (n, tuple(r.shape)))
        if flat is not None:
            f = torch.as_tensor(flat, dtype=torch.float64).to(device=self.device).contiguous()
            if tuple(f.shape) != (n,):
                raise ValueError("set_restraints_: flat must have shape (%d,), got %s" % (n, tuple(f.shape)))
        _lib.call("emdee_md_set_restraints", self._handle, C.c_void_p(a.data_ptr()) if n else None,
                  C.c_void_p(r.data_ptr()) if (r is not None and n) else None, C.c_void_p(kk.data_ptr()) if n else None,
                  C.c_void_p(f.data_ptr()) if (f is not None and n) else None, n)
        self._restraints = n

    def restraint_sums(self):
        """(8,) float64 numpy (blocking): [0] the restraint energy, [1:7] the sum of the restraint tensors (xx, yy, zz, xy, xz,
        yz), [7] the largest |x - ref| over the table.  Zeros without a table."""
        import numpy as np
        out = np.zeros(RESTRAINT_WORDS, dtype=np.float64)
        _lib.call("emdee_md_restraint_sums", self._handle, out.ctypes.data_as(C.c_void_p))
        return out

    def restraint_refs(self):
        """The references as they now stand (they follow the box): (n, 3) float64 tensor on the device, table order."""
        out = torch.zeros((self._restraints, 3), dtype=torch.float64, device=self.device)
        if self._restraints:
            _lib.call("emdee_md_get_restraint_refs", self._handle, C.c_void_p(out.data_ptr()))
        return out

    # -- centre-of-mass pulling between atom groups (include/emdee_hip.h: emdee_md_set_pull; undivided engines)
    _pull = None                                           # (n_coords, n_groups, log_capacity) of the table in force

    def set_pull_(self, group, coords, params=None, n_groups=None, log_every=0, log_capacity=0):
        """A bias between the centres of mass of atom groups (include/emdee_hip.h emdee_md_set_pull).  group: one integer per owned
        atom, -1 to leave the atom out (n_groups: how many groups, 1...8; None: the largest entry + 1).  coords: a list of dicts, one
        per coordinate, with a, b (groups), kind ("umbrella" or "constant-force"), geometry ("distance" or "direction"), k (the spring
        constant, or the force F of a constant force), r0, rate, and mask (distance: bit a keeps axis a, default 7) or n (direction:
        a vector, normalised by the library); or, with params, the raw tables: coords (n, 5) integers {a, b, kind, geometry, mask} and
        params (n, 6) floats {k or F, r0, rate, nx, ny, nz}.  log_every, log_capacity: the on-device log of (xi, f), one entry every
        log_every completed steps (capacity 0: none).  Evaluates the forces again.  Empty or None coords clears the table."""
        import numpy as np
        if params is None:
            rows_i, rows_d = [], []
            for c in (coords or []):
                kind, geom = c.get("kind", "umbrella"), c.get("geometry", "distance")
                n = [float(t) for t in c.get("n", (0.0, 0.0, 0.0))]
                rows_i.append([int(c["a"]), int(c["b"]), _PULL_KINDS.get(kind, kind), _PULL_GEOMETRIES.get(geom, geom), int(c.get("mask", 7))])
                rows_d.append([float(c.get("k", c.get("F", 0.0))), float(c.get("r0", 0.0)), float(c.get("rate", 0.0))] + n)
            ci, cd = np.array(rows_i, dtype=np.int32).reshape(-1, 5), np.array(rows_d, dtype=np.float64).reshape(-1, 6)
        else:
            ci = np.ascontiguousarray(np.asarray(coords, dtype=np.int32).reshape(-1, 5))
            cd = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, 6))
            if ci.shape[0] != cd.shape[0]:
                raise ValueError("set_pull_: %d rows of coords but %d rows of params" % (ci.shape[0], cd.shape[0]))
        nc = int(ci.shape[0])
        if nc == 0:
            _lib.call("emdee_md_set_pull", self._handle, None, 0, None, None, 0, 0, 0)
            self._pull = None
            return
        (g,), n_groups = self._per_atom_i32("set_pull_", n_groups, group=group)
        _lib.call("emdee_md_set_pull", self._handle, C.c_void_p(g.data_ptr()) if g is not None else None, n_groups,
                  ci.ctypes.data_as(C.c_void_p), cd.ctypes.data_as(C.c_void_p), nc, int(log_every), int(log_capacity))
        self._pull = (nc, n_groups, int(log_capacity))

    def pull(self):
        """What the last force pass wrote (blocking, one copy, no launch), as a dict of float64 numpy arrays: xi, xi0, f, U, work
        (n_coords,), D (n_coords, 3), centres (n_groups, 3) and masses (n_groups,)."""
        import numpy as np
        if self._pull is None:
            raise RuntimeError("pull: no pull table is set (set_pull_)")
        nc, ng, _ = self._pull
        c, g = np.zeros((nc, PULL_WORDS), dtype=np.float64), np.zeros((ng, 4), dtype=np.float64)
        _lib.call("emdee_md_pull_read", self._handle, c.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p))
        return dict(xi=c[:, 0].copy(), xi0=c[:, 1].copy(), f=c[:, 2].copy(), U=c[:, 3].copy(), work=c[:, 4].copy(), D=c[:, 5:8].copy(),
                    centres=g[:, :3].copy(), masses=g[:, 3].copy())

    def pull_log(self):
        """The on-device log so far (blocking), as a dict: xi and f, float64 numpy (count, n_coords), entry j taken at the pass that
        closed step (j + 1) log_every since the set; count; dropped, the samples that found the log full."""
        if self._pull is None:
            raise RuntimeError("pull_log: no pull table is set (set_pull_)")
        nc, _, cap = self._pull
        buf = torch.zeros((max(cap, 1), nc, 2), dtype=torch.float64, device=self.device)
        count, dropped = C.c_int64(), C.c_int64()
        _lib.call("emdee_md_pull_log_read", self._handle, C.c_void_p(buf.data_ptr()), C.byref(count), C.byref(dropped))
        h = buf[:count.value].cpu().numpy()
        return dict(xi=h[:, :, 0].copy(), f=h[:, :, 1].copy(), count=int(count.value), dropped=int(dropped.value))

    # -- soft-core alchemical decoupling (include/emdee_hip.h: emdee_md_set_alchemical; undivided engines)
    _alch = None                                           # (n_foreign, log_capacity) of the table in force

    def set_alchemical_(self, flag, lam=1.0, alpha=0.5, foreign=(), log_every=0, log_capacity=0):
        """Decouples the Lennard-Jones interaction between the flagged atoms (the solute) and all others along lam through a soft
        core (include/emdee_hip.h emdee_md_set_alchemical): U = lam 4 eps (D^-2 - D^-1) g with D = alpha (1 - lam) + (r / sigma)^6.
        flag: one integer per owned atom, 1 for the solute, 0 for the environment.  foreign: up to 16 more lambdas at which U_alch is
        evaluated for BAR / MBAR (by alchemical() and at log events).  log_every, log_capacity: the on-device log of (dU/dlam,
        U_alch, foreign energies), one entry every log_every completed steps (capacity 0: none).  Rebuilds the list and evaluates
        the forces again.  flag = None clears the table."""
        import numpy as np
        if flag is None:
            _lib.call("emdee_md_set_alchemical", self._handle, None, 1.0, 0.0, None, 0, 0, 0)
            self._alch = None
            self._alch_q = False
            return
        (f,), _ = self._per_atom_i32("set_alchemical_", 1, flag=flag)
        fl = np.ascontiguousarray(np.asarray(foreign, dtype=np.float64).reshape(-1))
        _lib.call("emdee_md_set_alchemical", self._handle, C.c_void_p(f.data_ptr()), float(lam), float(alpha),
                  fl.ctypes.data_as(C.c_void_p) if fl.size else None, int(fl.size), int(log_every), int(log_capacity))
        self._alch = (int(fl.size), int(log_capacity))
        self._alch_q = False                               # (a new table starts without the Coulomb stage)

    def set_lambda_(self, lam):
        """Moves lambda (a host scalar: no rebuild); the next step_ or query evaluates the forces anew.  For slow growth and lambda
        schedules."""
        _lib.call("emdee_md_set_lambda", self._handle, float(lam))

    set_alchemical, set_lambda = set_alchemical_, set_lambda_

    def alchemical(self):
        """The alchemical words of the current positions (blocking), as a dict: lam, U (U_alch), dUdl, virial (the cross pairs' scalar
        virial), pairs (the cross pairs inside the cutoff, an int) and foreign, float64 numpy (n_foreign,) of U_alch at the foreign
        lambdas."""
        import numpy as np
        if self._alch is None:
            raise RuntimeError("alchemical: no alchemical table is set (set_alchemical_)")
        w = np.zeros(ALCH_WORDS + self._alch[0], dtype=np.float64)
        _lib.call("emdee_md_alchemical_read", self._handle, w.ctypes.data_as(C.c_void_p))
        return dict(lam=float(w[0]), U=float(w[1]), dUdl=float(w[2]), virial=float(w[3]), pairs=int(round(w[4])), foreign=w[ALCH_WORDS:].copy())

    def alchemical_log(self):
        """The on-device log so far (blocking), as a dict: dUdl and U, float64 numpy (count,), foreign (count, n_foreign), entry j
        taken at the pass that closed step (j + 1) log_every since the set; count; dropped, the samples that found the log full."""
        if self._alch is None:
            raise RuntimeError("alchemical_log: no alchemical table is set (set_alchemical_)")
        nf, cap = self._alch
        buf = torch.zeros((max(cap, 1), 2 + nf), dtype=torch.float64, device=self.device)
        count, dropped = C.c_int64(), C.c_int64()
        _lib.call("emdee_md_alchemical_log_read", self._handle, C.c_void_p(buf.data_ptr()), C.byref(count), C.byref(dropped))
        h = buf[:count.value].cpu().numpy()
        return dict(dUdl=h[:, 0].copy(), U=h[:, 1].copy(), foreign=h[:, 2:].copy(), count=int(count.value), dropped=int(dropped.value))

    # -- the Coulomb stage of the alchemical table (include/emdee_hip.h: emdee_md_set_alchemical_coulomb; reaction-field engines)
    _alch_q = False

    def set_alchemical_coulomb_(self, lam_q, beta=0.0, foreign_q=()):
        """The Coulomb stage of the alchemical table in force, on the reaction field of set_coulomb_ (include/emdee_hip.h
        emdee_md_set_alchemical_coulomb): every cross pair's charge term becomes U_q = lam_q qq (1/rho + k_rf rho^2 - c_rf) with
        rho^2 = r^2 + beta (1 - lam_q); the solute's internal pairs keep their charges.  beta: a squared length in the caller's
        units.  foreign_q: as many lambda_q as the table has foreign lambdas; the k-th foreign state is (foreign[k], foreign_q[k]).
        Restarts the table's step count and both logs; no rebuild.  lam_q = None clears the stage."""
        import numpy as np
        if lam_q is None:
            _lib.call("emdee_md_set_alchemical_coulomb", self._handle, 0, 1.0, 0.0, None, 0)
            self._alch_q = False
            return
        fq = np.ascontiguousarray(np.asarray(foreign_q, dtype=np.float64).reshape(-1))
        _lib.call("emdee_md_set_alchemical_coulomb", self._handle, 1, float(lam_q), float(beta),
                  fq.ctypes.data_as(C.c_void_p) if fq.size else None, int(fq.size))
        self._alch_q = True

    def set_lambda_coulomb_(self, lam_q):
        """Moves lambda_q (a host scalar: no rebuild); the next step_ or query evaluates the forces anew."""
        _lib.call("emdee_md_set_lambda_coulomb", self._handle, float(lam_q))

    set_alchemical_coulomb, set_lambda_coulomb = set_alchemical_coulomb_, set_lambda_coulomb_

    def alchemical_coulomb(self):
        """The Coulomb stage's words of the current positions (blocking), as a dict: lam_q, U (U_q), dUdl (dU_q/dlam_q), virial (the
        cross pairs' scalar Coulomb virial) and foreign, float64 numpy (n_foreign,) of U_q at the foreign lambda_q."""
        import numpy as np
        if self._alch is None or not self._alch_q:
            raise RuntimeError("alchemical_coulomb: no Coulomb stage is set (set_alchemical_coulomb_)")
        w = np.zeros(ALCH_COULOMB_WORDS + self._alch[0], dtype=np.float64)
        _lib.call("emdee_md_alchemical_coulomb_read", self._handle, w.ctypes.data_as(C.c_void_p))
        return dict(lam_q=float(w[0]), U=float(w[1]), dUdl=float(w[2]), virial=float(w[3]), foreign=w[ALCH_COULOMB_WORDS:].copy())

    def alchemical_coulomb_log(self):
        """The Coulomb stage's on-device log so far (blocking), as a dict: dUdl and U, float64 numpy (count,), foreign (count,
        n_foreign); entry j is taken at the same pass as entry j of alchemical_log(); count; dropped."""
        if self._alch is None or not self._alch_q:
            raise RuntimeError("alchemical_coulomb_log: no Coulomb stage is set (set_alchemical_coulomb_)")
        nf, cap = self._alch
        buf = torch.zeros((max(cap, 1), 2 + nf), dtype=torch.float64, device=self.device)
        count, dropped = C.c_int64(), C.c_int64()
        _lib.call("emdee_md_alchemical_coulomb_log_read", self._handle, C.c_void_p(buf.data_ptr()), C.byref(count), C.byref(dropped))
        h = buf[:count.value].cpu().numpy()
        return dict(dUdl=h[:, 0].copy(), U=h[:, 1].copy(), foreign=h[:, 2:].copy(), count=int(count.value), dropped=int(dropped.value))

    def close(self):
        if self._handle is not None:
            _lib.call("emdee_md_destroy", self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pressure_tensor_dict(sums, volume):
    """twelve sums (W, K, each xx, yy, zz, xy, xz, yz) -> dict of 3 x 3 arrays virial, kinetic and pressure = (K + W) / V"""
    w, k = tensor_matrix(sums[:6]), tensor_matrix(sums[6:12])
    return dict(virial=w, kinetic=k, pressure=(k + w) / float(volume))
