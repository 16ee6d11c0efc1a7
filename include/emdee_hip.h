/*
 * emdee_hip.h -- C ABI of libemdee_hip.so: the MI355X (gfx950) implementation of
 * EmDee.jl's nonbonded pair-force hot path (cell-list neighbour build, switched
 * Lennard-Jones force / per-atom energy / per-atom virial, velocity-Verlet).
 *
 * This is the drop-in boundary.  EmDee's Julia operator layer (src/lennard_jones.jl,
 * src/nonbonded.jl, src/cells.jl of the reference) binds these symbols with `ccall`
 * in place of its CUDA.jl kernels; INTEGRATION.md shows that binding, and
 * emdee.jl_amd/ mirrors the same operator API in Python over ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types cross the boundary.
 *   - Every call returns int32 status: 0 = EMDEE_OK, negative = error; the message of
 *     the last error on the calling thread is emdee_last_error().  No exception crosses.
 *   - Handles are opaque, owned by the library, freed by the matching *_destroy.
 *   - "dev" pointers are device (HBM) pointers owned by the caller (hipMalloc,
 *     emdee_malloc or a torch tensor's data_ptr) on the context's device.
 *   - Work is enqueued on the context's HIP stream; emdee_sync() and the calls that
 *     return host values are the only blocking calls.  One host thread per context,
 *     as in the reference (single-threaded host, async launches, src/nonbonded.jl:115-119).
 *   - Streams.  A decomposed domain (emdee_dd_*) and the integrator it lends out (emdee_dd_engine)
 *     run on streams the library owns.  The calls that copy an engine's state into caller arrays --
 *     emdee_dd_get_state, emdee_md_get_state, emdee_md_nbr_list -- order themselves against the
 *     caller's context stream inside the library: the engine's stream waits for what the caller's
 *     stream had queued when the call was made (so a block the caller's allocator has just recycled is
 *     not written early), and the caller's stream waits for the copies (so work queued on it after the
 *     call sees them).  No device-wide synchronise, nothing for a binding to add.  Arrays handed IN
 *     (emdee_dd_set_atoms, emdee_md_create, ...) are read on the context's stream, in order.
 *   - Arrays follow the reference: positions/forces/velocities are 3xN column-major
 *     (xyz interleaved, src/nonbonded.jl:52-61), energies/virials length N.
 *   - precision = bytes per real of the caller's arrays: EMDEE_F32 (the reference's
 *     Float32) or EMDEE_F64 (north-star fp64).  Pair math runs in that type.
 *   - Pair semantics are the reference formula src/lennard_jones.jl:25-42.  The O(N)
 *     path drops pairs with r^2 >= rc^2 (EMDEE_CUTOFF); the all-pairs entry points can
 *     also reproduce the reference's literal behaviour, where the switch clamp gives
 *     g = 1 (full LJ) beyond rc (EMDEE_LITERAL).
 */
#ifndef EMDEE_HIP_H
#define EMDEE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMDEE_VERSION 100            /* 0.1.0, tracks the reference's Project.toml:4 */

/* status codes */
#define EMDEE_OK                 0
#define EMDEE_ERR_INVALID       -1   /* bad argument */
#define EMDEE_ERR_HIP           -2   /* HIP runtime error (message has hipGetErrorString) */
#define EMDEE_ERR_NO_DEVICE     -3   /* no usable gfx950 device */
#define EMDEE_ERR_ALLOC         -4
#define EMDEE_ERR_OVERFLOW      -5   /* neighbour capacity could not be grown */
#define EMDEE_ERR_STATE         -6   /* call out of order (e.g. step before set_state) */

/* output-selection bitmask -- src/nonbonded.jl:12-14 */
#define EMDEE_FORCES    1
#define EMDEE_ENERGIES  2
#define EMDEE_VIRIALS   4

/* precision = sizeof(real) */
#define EMDEE_F32 4
#define EMDEE_F64 8

/* pair semantics beyond the cutoff (all-pairs entry points only) */
#define EMDEE_LITERAL 0
#define EMDEE_CUTOFF  1

/* LennardJonesModel -- src/lennard_jones.jl:6-11: {rc^2, rs^2, 1/(rc^2 - rs^2)}.
 * Passed by value as doubles; the EMDEE_F32 path rounds each field to float first,
 * which is exactly the reference's Float32 struct. */
typedef struct emdee_lj_model { double rc2, rs2, inv_delta2; } emdee_lj_model;

/* LJAtom -- src/lennard_jones.jl:15-18, identical layout (2 x Float32, 8 bytes).
 * sigma_ij = half_sigma_i + half_sigma_j, 4 eps_ij = twice_sqrt_eps_i * twice_sqrt_eps_j
 * (Lorentz-Berthelot), src/lennard_jones.jl:29-30. */
typedef struct emdee_lj_atom { float half_sigma, twice_sqrt_eps; } emdee_lj_atom;

typedef struct emdee_ctx   emdee_ctx;     /* device + stream                      (replaces CUDA.jl context handling) */
typedef struct emdee_cells emdee_cells;   /* Cells                                (src/cells.jl:6-20) */
typedef struct emdee_nbr   emdee_nbr;     /* neighbour handle carried by `tiles`  (src/nonbonded.jl:18-26) */
typedef struct emdee_md    emdee_md;      /* velocity-Verlet state                (absent from the reference) */
typedef struct emdee_dd    emdee_dd;      /* spatial domain decomposition         (absent from the reference) */

/* ---------------------------------------------------------------- context */
const char *emdee_last_error(void);
int32_t emdee_version(void);
int32_t emdee_device_count(int32_t *count);
/* stream: a hipStream_t to enqueue on (e.g. torch's current stream), or NULL for the
 * device's default stream. */
int32_t emdee_ctx_create(int32_t device_id, void *stream, emdee_ctx **out);
int32_t emdee_ctx_destroy(emdee_ctx *ctx);
int32_t emdee_sync(emdee_ctx *ctx);
/* arch name ("gfx950..."), CU count and HBM bytes of the context's device */
int32_t emdee_device_info(emdee_ctx *ctx, char *arch, size_t arch_len, int32_t *cu_count, int64_t *hbm_bytes);

/* ---------------------------------------------------------------- memory
 * Replaces CuArray / CUDA.cu / CUDA.zeros / Array(dev) / unsafe_copyto!
 * (src/nonbonded.jl:25,123,151-153; test/runtests.jl:22-35). */
int32_t emdee_malloc(emdee_ctx *ctx, size_t nbytes, void **dev);
int32_t emdee_free(emdee_ctx *ctx, void *dev);
int32_t emdee_memcpy_h2d(emdee_ctx *ctx, void *dev, const void *host, size_t nbytes);
int32_t emdee_memcpy_d2h(emdee_ctx *ctx, void *host, const void *dev, size_t nbytes);   /* blocking */
int32_t emdee_memcpy_d2d(emdee_ctx *ctx, void *dst, const void *src, size_t nbytes);
int32_t emdee_memset(emdee_ctx *ctx, void *dev, int32_t byte, size_t nbytes);

/* ---------------------------------------------------------------- pair function
 * interaction(r2, model, atom_i, atom_j) -- src/lennard_jones.jl:25-42, evaluated by the
 * DEVICE pair function on n values of r2 (dev arrays of `precision` reals): E[k], W[k]. */
int32_t emdee_interaction(emdee_ctx *ctx, int32_t n, const void *r2_dev, emdee_lj_model model,
                          emdee_lj_atom atom_i, emdee_lj_atom atom_j, int32_t mode,
                          void *E_dev, void *W_dev, int32_t precision);

/* ---------------------------------------------------------------- Cells
 * Cells(r, L, cutoff; ndiv=2) -- src/cells.jl:176-194: M = floor(ndiv L / cutoff) cells per
 * dimension, 1-based cell id 1 + vx + M vy + M^2 vz, v = floor(M (s - floor s)), s = r / L.
 * emdee_cells_update = update_cells!(cells, r, L) (src/cells.jl:196-222); it re-bins all
 * atoms in O(N) (counting sort) instead of the reference's incremental linked-list edit. */
int32_t emdee_cells_create(emdee_ctx *ctx, int32_t N, double L, double cutoff, int32_t ndiv,
                           int32_t precision, emdee_cells **out);
int32_t emdee_cells_update(emdee_cells *cells, const void *positions_dev);
int32_t emdee_cells_destroy(emdee_cells *cells);
int32_t emdee_cells_M(const emdee_cells *cells, int32_t *M);
/* dev pointers valid until the next update/destroy: index[N] (1-based cell of each atom),
 * population[M^3], start[M^3+1] (0-based offsets into order), order[N] (atom ids by cell,
 * ascending within a cell -- the array form of the reference's head/next lists). */
int32_t emdee_cells_arrays(const emdee_cells *cells, const int32_t **index_dev,
                           const int32_t **population_dev, const int32_t **start_dev,
                           const int32_t **order_dev);

/* ---------------------------------------------------------------- neighbour handle
 * nonbonded_computation_tiles(N) (src/nonbonded.jl:18-26) returns what compute_nonbonded!
 * iterates over.  Here that object is a neighbour-list workspace for N atoms: cell binning,
 * cell-ordered copies and a full (owner-computes) list with a skin, rebuilt inside
 * emdee_compute_nonbonded when any atom has moved more than skin/2 since the last build. */
int32_t emdee_nbr_create(emdee_ctx *ctx, int32_t N, double skin, int32_t precision, emdee_nbr **out);
int32_t emdee_nbr_destroy(emdee_nbr *nbr);
/* builds = list builds so far; listed = entries in the current list; max_count = longest
 * row; capacity = row stride.  Blocking. */
int32_t emdee_nbr_stats(emdee_nbr *nbr, int64_t *builds, int64_t *listed, int32_t *max_count,
                        int32_t *capacity);
/* number of pairs with r^2 < rc^2 in the current list (each pair counted once). Blocking. */
int32_t emdee_nbr_count_pairs(emdee_nbr *nbr, int64_t *pairs_in_cutoff);

/* Verification accessor: the current list as CALLER ids.  counts_dev[i] = entries of atom i's row (skin entries
 * included), neighbors_dev[i * capacity + k] = its k-th neighbour, k < min(counts, capacity); capacity >= the
 * `capacity` of emdee_nbr_stats returns every row whole.  Owned atoms only; ghosts appear as neighbours.
 * (The list itself stores 16-bit tile-local slots; this decodes them through the brick tables.) */
int32_t emdee_nbr_list(emdee_nbr *nbr, int32_t *counts_dev, int32_t *neighbors_dev, int32_t capacity);
int32_t emdee_md_nbr_list(emdee_md *md, int32_t *counts_dev, int32_t *neighbors_dev, int32_t capacity);

/* Exclusions and 1-4 pairs (build-defined; SURVEY.md 8(f) item 2 "hooks": the reference parses lj14scale from its force-field
 * file, src/modelling.jl:197-200, and nothing consumes it -- its hot path sums every pair, src/nonbonded.jl:129-150).
 * pairs_dev: n_pairs pairs {i, j} of atom indices (caller order, 2 n_pairs int32, device); copied.  A pair named by
 * emdee_*_set_exclusions contributes nothing; a pair named by emdee_*_set_pairs14 contributes lj14scale times its pair terms
 * (forces, energy and virial halves).  Both are struck from the neighbour rows right after every list build -- the pair loop
 * carries no mask -- and the 1-4 pairs are evaluated by a kernel of their own behind every force pass (an integrator with
 * 1-4 pairs steps with the split kernels: force pass, 1-4 terms, kick + drift).  Each call replaces its table; n_pairs = 0
 * clears it.  All or nothing: each pair needs i != j and 0 <= i, j < N, else EMDEE_ERR_INVALID and both previous tables stay in
 * force.  Undivided boxes (emdee_nbr, emdee_md without ghosts); emdee_md: after emdee_md_set_state.  Two-species boxes with
 * exclusions keep the general-species kernels.  Decomposed runs: emdee_dd_set_exclusions / emdee_dd_set_pairs14 (tables over
 * global ids); an integrator lent by emdee_dd_engine refuses these calls with EMDEE_ERR_STATE.
 * A 1-4 partner is found through the neighbour rows (the list build records where it sits), in undivided and decomposed runs
 * alike.  That is the same as a look-up by index whenever the list is valid -- automatic rebuilds (rebuild_every = 0) and the
 * emdee_nbr calls: a pair beyond rc + skin at a build cannot come within rc before the next one.  With a fixed rebuild_every > 0
 * that lets atoms outrun the skin, a 1-4 pair is treated like any listed pair: the list's own contract. */
int32_t emdee_nbr_set_exclusions(emdee_nbr *nbr, const int32_t *pairs_dev, int32_t n_pairs);
int32_t emdee_nbr_set_pairs14(emdee_nbr *nbr, const int32_t *pairs_dev, int32_t n_pairs, double lj14scale);
int32_t emdee_md_set_exclusions(emdee_md *md, const int32_t *pairs_dev, int32_t n_pairs);
int32_t emdee_md_set_pairs14(emdee_md *md, const int32_t *pairs_dev, int32_t n_pairs, double lj14scale);

/* Bonded terms (the HarmonicBondForce, HarmonicAngleForce and PeriodicTorsionForce of an OpenMM force-field file, as the
 * reference's src/modelling.jl reads them).  kind, the ids of each term (atoms_dev, device, copied) and its fp64 parameters
 * (params_dev, device, copied):
 *   EMDEE_HARMONIC_BOND     i, j        {k, r0}            U = k/2 (r - r0)^2
 *   EMDEE_HARMONIC_ANGLE    i, j, k     {k, theta0}        U = k/2 (theta - theta0)^2, j the vertex, theta0 in radians
 *   EMDEE_PERIODIC_TORSION  i, j, k, l  {k, n, phase}      U = k (1 + cos(n phi - phase)), phi the IUPAC dihedral (trans = pi),
 *                                                          n an integer >= 1; a quadruple may appear once per (k, n, phase)
 * Vectors inside a term are chained minimum images along its bonds (r_j - r_i, then r_k - r_j, r_l - r_k): a term that crosses
 * the periodic boundary is unwrapped.  Owner computes: every atom of a term receives -grad U with respect to itself and 1/2,
 * 1/3 or 1/4 of the term's energy, of its virial W = sum_a x_a . F_a (x_a unwrapped; a bond gives -r dU/dr) and of its
 * symmetrised tensor sum_a x_a (x) F_a; the energies, virials, tensors and sums of emdee_md_* / emdee_dd_* include them.
 * Bonded terms do not change the pair set: exclusions and 1-4 pairs stay the caller's tables.
 * Singular geometries.  Where the direction of a term's force is undefined it gives ZERO FORCE on all its atoms and a FINITE
 * ENERGY, in both precisions, whatever k is: a bond of length 0 (U = k/2 r0^2), an angle with |a x b| = 0 -- straight or folded,
 * U = k/2 (theta - theta0)^2 with theta = pi or 0 -- and a torsion with |b1 x b2| = 0, |b2 x b3| = 0 or b2 = 0 (U finite: phi is
 * undefined).  A chain drawn along a lattice line is such a start, and emdee_md_minimize and emdee_*_step go through it: the
 * atoms stay on their line until something else moves them off it.  "Zero" is decided on the norm the formula divides by, as it
 * computes it: below 1e-37 (Float32) or 1e-300 (Float64) the force is zero, from there on the quotient is taken as it always was
 * (every term with its norms above the threshold keeps its bits).  Near a singular geometry the force is not clipped: its error
 * grows as u / sin(theta) (u the unit round-off; DESIGN.md has the measured constant), and a torsion's force on an end atom grows
 * as 1 / sin(theta) itself.  Two limits: a torsion's coefficient k n |b2| / |b1 x b2|^2 must stay inside the format (in Float32
 * and at k n = 1e6 that is sin(theta) above 1e-16 at unit bond lengths), and the zero force of a straight angle holds for arms
 * longer than 1e-4 (Float32; 1e-11 in Float64) of the length unit.
 *   - emdee_md_set_bonded: caller ids in [0, N), after emdee_md_set_state, undivided boxes.  emdee_dd_set_bonded: global ids
 *     in [0, 2^31), collective, before emdee_dd_load or between steps (after a load it rebuilds every domain).
 *   - Each call replaces the table of its kind; n_terms = 0 clears it.  All or nothing: EMDEE_ERR_INVALID, the previous tables
 *     in force, for an unknown kind, a NULL array with n_terms > 0, an atom named twice in a term, an id out of range, a
 *     non-finite parameter, r0 < 0, theta0 outside [0, pi], or n not an integer >= 1.  An integrator lent by emdee_dd_engine
 *     refuses emdee_md_set_bonded with EMDEE_ERR_STATE.
 *   - The partners are found through the neighbour rows: the filter that runs right after every build records where each one
 *     sits, so the terms are exact between builds whatever rebuild_every is.  A partner that is not in its owner's rows at a
 *     build (the term spans more than rc + skin) is an error: EMDEE_ERR_STATE naming the term, from the set call or at the
 *     latest from the next emdee_*_step / _energies / _pressure_tensor (no extra read-back inside a batch of steps), and the
 *     engine refuses to step until the tables or the state are replaced.
 *   - An engine with bonded terms steps in the split form (force pass, 1-4 and bonded terms, kick + drift) and keeps the
 *     general-species kernels. */
#define EMDEE_HARMONIC_BOND     1
#define EMDEE_HARMONIC_ANGLE    2
#define EMDEE_PERIODIC_TORSION  3
int32_t emdee_md_set_bonded(emdee_md *md, int32_t kind, const int32_t *atoms_dev, const double *params_dev, int32_t n_terms);

/* Reaction-field Coulomb forces between charged atoms (a cutoff method: the neighbour rows of the LJ model, no new
 * communication).  Each atom i carries a charge q_i; Coulomb's constant K is the caller's, in the caller's units (about
 * 138.935 kJ mol^-1 nm e^-2); eps_rf is the reaction-field dielectric, 1 <= eps_rf <= +inf; rc is the LJ model's cutoff:
 *   k_rf = (eps_rf - 1) / ((2 eps_rf + 1) rc^3)      (1 / (2 rc^3) at eps_rf = +inf, 0 at eps_rf = 1)
 *   c_rf = 1/rc + k_rf rc^2
 * For every listed pair with r^2 < rc^2 (the strict CUTOFF test of the LJ terms):
 *   U_ij = K q_i q_j (1/r + k_rf r^2 - c_rf)          so that U(rc) = 0
 *   W_ij = -r dU/dr = K q_i q_j (1/r - 2 k_rf r^2)
 *   F_i  = (W_ij / r^2) d,  d = r_i - r_j the minimum image (the LJ convention)
 * These terms are added to the LJ terms of the same pair in every output: forces, the per-atom energies and virials (half to
 * each atom), the per-atom tensors (W / r^2) d (x) d (half to each atom; tr W_i = w_i still holds), emdee_*_energies and
 * emdee_*_pressure_tensor.  An excluded pair contributes nothing; a 1-4 pair contributes coulomb14scale times its terms (same
 * formula, same cutoff), next to its lj14scale-scaled LJ terms.  There is NO self term and NO reaction-field correction for
 * excluded pairs.  Codes that add them (GROMACS' reaction field, for one) add K q_i q_j (k_rf r^2 - c_rf) for every excluded
 * pair within rc, which changes energies and forces, and a self term -K q_i^2 c_rf / 2 per atom, a constant that changes
 * energies only; energies from this library differ from theirs by those terms.  At eps_rf = +inf force and
 * energy both go to zero at rc; at a finite eps_rf the force jumps at rc by K q_i q_j 3 / ((2 eps_rf + 1) rc^2).
 *   - emdee_md_set_coulomb: charges in caller-id order, n = the owned atom count, after emdee_md_set_state; undivided engines
 *     only (an integrator lent by emdee_dd_engine, or one with ghosts, returns EMDEE_ERR_STATE).  The charges stay in force
 *     across a later set_state with the same atom count; after one with another count that set_state evaluates no forces,
 *     and the engine refuses with EMDEE_ERR_STATE to step, to evaluate forces and to hand out forces, energies, virials or
 *     tensors (emdee_md_get_state with any of them, _energies, _virial_tensor, _pressure_tensor) until the charges are set
 *     again or cleared; positions and velocities can still be read.
 *   - n = 0 clears the charges (the constants are then not looked at): the engine runs the uncharged kernels again.
 *   - The engine keeps two fp64 tables of n entries on the device: sqrt(K) q for its kernels, and the charges as given, for the
 *     charge word of emdee_md_set_spatial (q is not recovered exactly from sqrt(K) q): 16 bytes per atom, one more upload per call.
 *   - All or nothing: EMDEE_ERR_INVALID, the previous charges in force, for a NULL array with n > 0, the wrong n, a non-finite
 *     charge, K not finite or <= 0, eps_rf < 1 or NaN, a non-finite or negative coulomb14scale.
 *   - The 1-4 pairs themselves come from emdee_*_set_pairs14.
 *   - A charged engine steps in the split form (force pass, 1-4 and bonded terms, kick + drift) and keeps the general-species
 *     kernels, even where its LJ parameters are uniform.  Not on the operator path (emdee_compute_nonbonded, emdee_nbr_*). */
int32_t emdee_md_set_coulomb(emdee_md *md, const double *charges_dev, int32_t n, double coulomb_k, double eps_rf,
                             double coulomb14scale);

/* Ewald summation for a charged engine (emdee_md_set_coulomb first): alpha > 0 switches the engine's Coulomb terms from the
 * reaction field to the classical Ewald sum with splitting parameter alpha (an inverse length) and the integer wave vectors n,
 * |n_d| <= kmax[d], n != 0.  While it is on eps_rf is not looked at; coulomb_k and coulomb14scale stay those of
 * emdee_md_set_coulomb.  alpha == 0 switches back to the reaction field (kmax is then not looked at).  With qq = K q_i q_j,
 * V the current volume, Q = sum q_i and N the atom count:
 *   real space, every listed pair with r^2 < rc^2:
 *     U = qq erfc(alpha r) / r
 *     W = -r dU/dr = qq (erfc(alpha r) / r + (2 alpha / sqrt(pi)) exp(-alpha^2 r^2)),   F_i = (W / r^2) d
 *     halves to each atom in energies, virials and tensors, as the reaction-field terms.
 *   excluded pair (struck from the rows; minimum image, NO cutoff test):
 *     U = -qq erf(alpha r) / r
 *     W = -qq (erf(alpha r) / r - (2 alpha / sqrt(pi)) exp(-alpha^2 r^2))
 *   1-4 pair: its Coulomb part is coulomb14scale qq / r plus the excluded-pair correction above, with no cutoff test; its LJ
 *     part keeps lj14scale and the cutoff test.
 *   reciprocal space, k = 2 pi (n_x / L_x, n_y / L_y, n_z / L_z) of the current box, A(k) = (4 pi / V) exp(-k^2 / 4 alpha^2) / k^2,
 *   S(k) = sum_j q_j exp(i k.r_j):
 *     E_k  = (K / 2) sum_k A |S|^2
 *     F_i  = K q_i sum_k A k (sin(k.r_i) Re S - cos(k.r_i) Im S)
 *     e_i  = (K / 2) q_i sum_k A (cos(k.r_i) Re S + sin(k.r_i) Im S)
 *     W_i^ab = (K / 2) q_i sum_k A (cos(k.r_i) Re S + sin(k.r_i) Im S) (delta_ab - 2 k_a k_b (1 / k^2 + 1 / (4 alpha^2)))
 *     and the per-atom virial is its trace.  A direct O(N K) sum in fp64 whatever the engine's precision, no floating-point
 *     atomics: the same bits from run to run.
 *   self term: -K (alpha / sqrt(pi)) q_i^2 in e_i; no force, no virial.
 *   neutralising background: E_n = -pi K Q^2 / (2 V alpha^2); E_n / N in every e_i and in the xx, yy and zz components of every
 *     atom's tensor (3 E_n / N in its virial).
 * All of these are added to the LJ and bonded terms in every output of a charged engine: forces, per-atom energies, virials
 * and tensors, emdee_md_energies and emdee_md_pressure_tensor; the barostats couple to the Ewald pressure.  emdee_md_scale_box
 * keeps alpha and kmax and evaluates on the new box.  On return forces, energies and virials are current, as after
 * emdee_md_set_coulomb.
 *   - The setting survives a later emdee_md_set_coulomb with new charges and an emdee_md_set_state with the same atom count;
 *     clearing the charges (n = 0) switches it off.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous setting in force: alpha negative or not finite, a NULL kmax, a kmax[d]
 *     < 1 or > 64, alpha rc < 1 (nothing is split off).  EMDEE_ERR_STATE: before emdee_md_set_state, without charges, with
 *     ghosts, on a box that is not periodic in all three dimensions, on an integrator lent by emdee_dd_engine.
 *   - The row filter records the slot of every excluded and 1-4 partner at every build; a partner missing from its owner's rows
 *     (the pair spans more than rc + skin) is EMDEE_ERR_STATE naming the pair, under the rules of a bonded partner.
 *   - There is no emdee_dd_* counterpart (decomposed runs have the reaction field only) and nothing on the operator path.
 *   - The reciprocal-space pass runs behind every force pass; its device time is emdee_md_kernel_time index 8. */
int32_t emdee_md_set_ewald(emdee_md *md, double alpha, const int32_t kmax[3]);

/* Smooth particle-mesh Ewald (Essmann et al., J. Chem. Phys. 103, 8577, 1995) for a charged engine: alpha > 0 switches the
 * engine's reciprocal-space terms to a mesh of K_d = grid[d] points per axis and cardinal B-splines theta_p of order p = order.
 * alpha == 0 switches back to the reaction field (grid and order are then not looked at).  It excludes emdee_md_set_ewald:
 * whichever of the two was called last with alpha > 0 is in force, and alpha == 0 through either returns to the reaction field.
 * The real-space side is that of emdee_md_set_ewald, term for term: erfc pair terms, the correction of excluded and 1-4 pairs,
 * the coulomb14scale qq / r term, the self term, the neutralising background and the missing-partner error.  Only the
 * reciprocal sum over k is replaced.  With u_d = K_d (x_d - lo_d) / L_d the scaled coordinates, m a mesh point,
 *   Q(m) = sum_j q_j prod_d theta_p(u_jd - m_d) over periodic images          (the charge mesh),
 *   |b_d(m)|^2 = 1 / |sum_{k=0}^{p-2} theta_p(k + 1) exp(2 pi i m k / K_d)|^2   (Essmann eq. 4.4),  |b|^2 = |b_x|^2 |b_y|^2 |b_z|^2,
 *   k = 2 pi (n_x / L_x, n_y / L_y, n_z / L_z) with n_d the mesh index m_d folded to (-K_d / 2, K_d / 2], A(k) as above,
 *   F the discrete Fourier transform over the mesh, F^-1 its unnormalised inverse:
 *     E    = (K / 2) sum_{m != 0} A |b|^2 |F Q(m)|^2
 *     phi  = F^-1[A |b|^2 F Q]                                               (the convolved mesh)
 *     F_i  = -K q_i sum_m grad theta(u_i - m) phi(m)     (the analytic spline derivative: the exact gradient of E)
 *     e_i  = (K / 2) q_i sum_m theta(u_i - m) phi(m)
 *     W_i^ab = (K / 2) q_i sum_m theta(u_i - m) phi_ab(m),  phi_ab = F^-1[A |b|^2 (delta_ab - 2 k_a k_b (1 / k^2 + 1 / (4 alpha^2))) F Q]
 *     and the per-atom virial is its trace.  Summed over the atoms the tensor is Essmann's eq. 2.7, the exact volume derivative
 *     of E at a fixed mesh.  The mesh forces do not sum to zero exactly (the mesh breaks translation invariance).
 * Mesh and transforms are fp64 whatever the engine's precision.  The charge mesh is summed in 64-bit fixed point with integer
 * atomic adds, no floating-point atomics: the same bits from run to run.  The pass that writes every output costs one forward
 * and seven inverse transforms, the forces-only pass one and one; two complex meshes of K_x K_y K_z points are held.
 * emdee_md_scale_box and the barostats keep alpha, grid and order and evaluate on the new box.
 *   - The setting survives a later emdee_md_set_coulomb with new charges and an emdee_md_set_state with the same atom count;
 *     clearing the charges (n = 0) switches it off.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous setting in force: alpha negative or not finite, alpha rc < 1, a NULL
 *     grid, a grid[d] that is not a power of two in [8, 256], an order other than 4 or 6 (even orders have no zero of the spline
 *     modulus at the Nyquist index).  EMDEE_ERR_STATE: before emdee_md_set_state, without charges, with ghosts, on a box that
 *     is not periodic in all three dimensions, on an integrator lent by emdee_dd_engine.
 *   - Scope: undivided orthorhombic engines only; complex-to-complex transforms; no emdee_dd_* counterpart; nothing on the
 *     operator path.
 *   - The pass's device time is emdee_md_kernel_time index 8, as the direct sum's. */
int32_t emdee_md_set_pme(emdee_md *md, double alpha, const int32_t grid[3], int32_t order);

/* Rigid three-site molecules (SETTLE: Miyamoto & Kollman, J. Comput. Chem. 13, 952 (1992); build-defined like the integrator).
 * n_mol rigid three-site molecules.  atoms_dev: 3 n_mol caller ids {apex, a, b}; geom_dev: 2 n_mol doubles {d_leg, d_base}:
 * |apex - a| = |apex - b| = d_leg, |a - b| = d_base.  Device arrays, copied.  n_mol = 0 clears the table.
 * While a table is in force emdee_md_step takes every step in the closed form of a coupled engine -- each step opens and closes
 * its own half kick; no merged kicks, no run-ahead, no fused step -- with three stages around the unchanged kernels:
 *   (a) the constrained atoms' positions x0 are remembered (they satisfy the constraints);
 *   (b) v += (dt/2) f/m [; Langevin O step] ; x += dt v                                       (emdee_md_kick_drift's kernel)
 *   (c) x <- the rigid triangle nearest x in the SHAKE sense with respect to x0: x + sum_k lambda_k (x0_i - x0_j) / m_i over the
 *       three bonds, in closed form; v <- v + (x_constrained - x_unconstrained) / dt; the three atoms are tested against the
 *       skin/2 displacement threshold again and raise the same rebuild word;
 *   (d) the rebuild if due (rebuild_every, or the displacement word); f = F(x); v += (dt/2) f/m;
 *   (e) the components of the relative velocities along the three bonds are removed (RATTLE for a triangle: one 3 x 3 linear
 *       solve, no iteration).
 * step(40), 8 x step(5) and 40 x step(1) are the same sequence of launches and agree bit for bit; a run is bitwise reproducible
 * (one thread per molecule, no atomics on the state).  An engine without a table steps exactly as before.
 * Stages (c) and (e) work in fp64 on unwrapped differences whatever the engine's precision: minimum images of a - apex and
 * b - apex; a Float32 engine's cell-relative records get their cells' origins added in double before differencing; corrections
 * are added to each record in its own frame.  Masses are the engine's (inv_mass_dev of emdee_md_set_state, or 1).
 *   - Forces, energies, virials and tensors stay those of the force field: constraint forces are not added to any of them.  The
 *     pressure of a constrained engine therefore LACKS THE CONSTRAINT VIRIAL, and for that reason (and because scaling atom by
 *     atom would break the geometry) emdee_md_scale_box and emdee_md_set_barostat (other than OFF) return EMDEE_ERR_STATE on an
 *     engine with a table, and this call returns EMDEE_ERR_STATE while a barostat is on -- unless emdee_md_set_molecular_scaling
 *     (below) is on, which measures the pressure and scales by molecular centres of mass, where constraint forces drop out.
 *     The kinetic energy is that of the constrained velocities.
 *   - The call moves no atom.  It CHANGES VELOCITIES: stage (e) is applied once, so that the velocities it leaves are consistent
 *     with the constraints.  The neighbour list and the forces are kept.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous table in force: a NULL array with n_mol > 0, n_mol < 0, an id outside
 *     [0, n_owned), an atom named twice (within a molecule or across molecules), a distance that is not finite and > 0,
 *     d_base >= 2 d_leg (no triangle).  EMDEE_ERR_STATE naming a molecule (one device check, one read-back), the previous table
 *     in force: atoms a and b have different masses; the loaded positions miss a distance by more than 1e-3 relative (a wrong
 *     topology, not rounding).  EMDEE_ERR_STATE also before emdee_md_set_state, with ghosts, and on an integrator lent by
 *     emdee_dd_engine.
 *   - The table survives an emdee_md_set_state with the same atom count: it is checked against the new state (EMDEE_ERR_STATE
 *     from emdee_md_set_state if it does not fit) and the new velocities are projected.  After a state with another atom count,
 *     or one that did not fit, emdee_md_step returns EMDEE_ERR_STATE until the table is set again or cleared, as with charges.
 *   - A negative radicand in stage (c) means a molecule moved too far for a rigid solution: the molecule is left as it is and
 *     emdee_md_step, which reads one error word per call, returns EMDEE_ERR_STATE naming it; the engine then refuses to step
 *     until the table or the state is replaced.
 *   - Scope: emdee_md_step of undivided engines only.  The split calls (emdee_md_kick_drift, _forces, _kick, _fused_step) never
 *     constrain on their own; there is no emdee_dd_* counterpart.  Bonded terms that name a constrained pair stay legal: they
 *     contribute a constant.  The constraint virial is not provided; scaling by molecular centres is
 *     emdee_md_set_molecular_scaling.
 *   - With pressure coupling on (emdee_md_set_molecular_scaling), the step that completes an interval is followed, after its
 *     stage (e), by (f) the coupling event: the molecular pressure of that step's forces F(x) and stage-(e) velocities, then
 *     the molecular scale (a rebuild and a force pass on the new box; a fixed rebuild_every cadence restarts from it).
 *   - The device time of stages (a), (c) and (e) is emdee_md_kernel_time index 9. */
int32_t emdee_md_set_rigid3(emdee_md *md, const int32_t *atoms_dev, const double *geom_dev, int32_t n_mol);

/* Bonds to hydrogen held at fixed lengths (SHAKE in matrix form: Kraeutler, van Gunsteren & Huenenberger, J. Comput. Chem. 22,
 * 501 (2001); RATTLE: Andersen, J. Comput. Phys. 52, 24 (1983); build-defined like the integrator).
 * n_clusters star clusters: a centre and one, two or three satellites (X-H, XH2, XH3), every satellite at a fixed distance from
 * the centre; no constraint between satellites.  atoms_dev: 4 n_clusters caller ids {centre, s1, s2, s3}, -1 in the unused
 * trailing slots; dist_dev: 3 n_clusters doubles, |centre - s_k| (those of unused slots are ignored).  Device arrays, copied.
 * n_clusters = 0 clears the table.  Water stays with emdee_md_set_rigid3: the two tables may be in force together and name
 * disjoint atoms.
 * The contract is that of emdee_md_set_rigid3, point for point.  While a table is in force emdee_md_step takes the closed form
 * described there, and each of its stages runs for whichever tables exist:
 *   (a) the clusters' positions x0 are remembered;
 *   (c) x_c <- x_c + w_c sum_j lambda_j e_j, x_k <- x_k - w_k lambda_k e_k with e_k = x0_c - x0_k, w = 1/m, and the lambda that
 *       restore the n distances: Newton's method from lambda = 0 on the n coupled equations, each n x n system solved directly,
 *       to a residual | |r_k|^2 - d_k^2 | <= 4e-15 d_k^2 or 32 iterations (per thread, deterministic); v <- v + (x_constrained -
 *       x_unconstrained) / dt; the atoms are tested against the skin/2 threshold again and raise the same rebuild word;
 *   (e) the components of the relative velocities along the bonds are removed: one symmetric n x n solve, applied twice.
 * One thread per cluster, fp64 on unwrapped differences in both precisions, no atomics on the state: step(40), 8 x step(5) and
 * 40 x step(1) agree bit for bit, and an engine whose table was cleared steps exactly as one that never had one.
 *   - Device arrays are copied.  The call moves no atom and CHANGES VELOCITIES: stage (e) is applied once.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous table in force: a NULL array with n_clusters > 0, n_clusters < 0, an id
 *     outside [0, n_owned), an empty cluster (s1 < 0), a -1 followed by an id, an atom named twice (within a cluster or across
 *     clusters), an atom that the rigid table in force also names (emdee_md_set_rigid3 refuses the mirror case), a distance of
 *     a used slot that is not finite and > 0.  EMDEE_ERR_STATE naming a cluster, the previous table in force: the loaded
 *     positions miss a distance by more than 1e-3 relative.  EMDEE_ERR_STATE also before emdee_md_set_state, with ghosts, and
 *     on an integrator lent by emdee_dd_engine.
 *   - The table survives an emdee_md_set_state with the same atom count, checked against the new state and the new velocities
 *     projected; after a state with another count, or one that did not fit, emdee_md_step returns EMDEE_ERR_STATE until the
 *     table is set again or cleared.
 *   - A cluster for which stage (c) finds no solution (the iteration cap, a singular Jacobian, a number that is not finite) is
 *     left as it is; emdee_md_step, which reads one more error word per call, returns EMDEE_ERR_STATE naming it, and the engine
 *     refuses to step until the table or the state is replaced.
 *   - The split calls never constrain.  Forces, energies, virials and tensors stay those of the force field.  Masses are
 *     unrestricted.
 *   - Pressure: without a molecule table (emdee_md_set_molecules), whatever emdee_md_set_molecular_scaling says, an engine with
 *     an hbonds table refuses emdee_md_scale_box, emdee_md_set_barostat (other than OFF) and emdee_md_molecular_pressure_tensor
 *     with EMDEE_ERR_STATE, and this call returns EMDEE_ERR_STATE while a barostat is on: the molecular sums and the molecular
 *     scale of the rigid table are written for three-site molecules, and without the clusters' part the promise that constraint
 *     forces drop out of the molecular pressure would be false.  With a molecule table in force and
 *     emdee_md_set_molecular_scaling on, all four are accepted: the sums and the scale run over whole molecules, every cluster
 *     inside one (a cluster that the molecule table in force splits, or leaves at -1, is EMDEE_ERR_INVALID here).
 *   - The device time of stages (a), (c) and (e) is emdee_md_kernel_time index 11. */
int32_t emdee_md_set_hbonds(emdee_md *md, const int32_t *atoms_dev, const double *dist_dev, int32_t n_clusters);

/* Virtual interaction sites: massless particles that carry interactions (a charge, LJ parameters) and sit at a fixed linear
 * combination of two or three atoms with mass -- the fourth site of TIP4P/2005, TIP4P-Ew, TIP4P/Ice and OPC, GROMACS' site types 2
 * and 3 (build-defined like the integrator).
 * atoms_dev: 4 n_sites caller ids {site, a, b, c}, c = -1 for a two-parent site; weights_dev: 2 n_sites doubles {w_b, w_c} (w_c is
 * ignored when c = -1).  Device arrays, copied.  n_sites = 0 clears the table.
 *   Placement:  x_site = x_a + w_b mi(x_b - x_a) + w_c mi(x_c - x_a), mi the minimum image, in fp64 in both precisions (a Float32
 *               engine's cell-relative records get their origins added in double); the site's record moves to the image of the
 *               result nearest to where it was.  A bisector site at d_OM from the apex of a triangle (d_leg, d_base) has
 *               w_b = w_c = d_OM / (2 sqrt(d_leg^2 - d_base^2 / 4)).
 *   Spreading:  after a force pass, f_a += (1 - w_b - w_c) f_site, f_b += w_b f_site, f_c += w_c f_site, then f_site = 0.  One
 *               thread per distinct parent sums its shares in table order, in fp64: no floating-point atomics, runs stay bit
 *               for bit reproducible.  Several sites may share parents.
 * Out-of-plane sites (TIP5P's lone pairs, a cross product of the legs) are not covered: a follow-up.
 * Placement is linear, so sum_k x_k (x) (w_k f_site) = x_site (x) f_site on unwrapped coordinates: the box sums of energies,
 * virials and tensors are those of the force field and are not touched.  The PER-ATOM energies, virials and tensors keep the
 * site's half of its pair terms on the site; only the forces move to the parents.
 *   - Sites are massless: the caller loads them with inv_mass = 0, and kick, drift and Langevin noise then leave them alone; the
 *     kinetic energy and the kinetic tensor count them as exactly 0.  One device check, one read-back: EMDEE_ERR_STATE naming the
 *     site, the previous table in force, for a site with inv_mass != 0, a parent with inv_mass == 0, or a state loaded without
 *     masses.
 *   - On success the call zeroes the sites' velocities, places the sites, rebuilds the neighbour list and evaluates the forces
 *     (spread): on return positions, forces and list belong together.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous table in force: a NULL array with n_sites > 0, n_sites < 0, an id outside
 *     [0, n_owned), a or b negative, an atom named twice within an entry, an atom that is a site in two entries, a site that is a
 *     parent of another site, a site that the rigid or hbonds table in force names (emdee_md_set_rigid3 and emdee_md_set_hbonds
 *     refuse the mirror case: an atom that is a site; PARENTS may be in either table), a weight in use that is not finite.
 *     EMDEE_ERR_STATE also before emdee_md_set_state, with ghosts, and on an integrator lent by emdee_dd_engine.
 *   - The table survives an emdee_md_set_state with the same atom count: it is checked again (EMDEE_ERR_STATE from
 *     emdee_md_set_state if it does not fit), the sites are placed, their velocities zeroed and the list rebuilt.  After a state
 *     with another count, or one that did not fit, emdee_md_step and emdee_md_minimize return EMDEE_ERR_STATE until the table is
 *     set again or cleared.
 *   - While a table is in force emdee_md_step takes the closed form of emdee_md_set_rigid3 with two more stages: (c') after stage
 *     (c) of every constraint table the sites are placed (they are tested against the skin/2 threshold and raise the same rebuild
 *     word), (d') between the force pass and the closing kick the forces are spread.  emdee_md_minimize does the same; G of a
 *     site is 0.  Every force pass that writes the engine's force planes spreads once (emdee_md_set_state, emdee_md_forces,
 *     emdee_md_scale_box, emdee_md_get_state or emdee_md_energies evaluating all outputs); the tensor pass leaves the planes alone
 *     and does not.
 *   - emdee_md_scale_box, atom by atom or molecular, puts the sites back on their scaled parents before its rebuild: with
 *     emdee_md_set_molecular_scaling a site moves rigidly with its water, the molecular sums need nothing (the site is massless
 *     and carries no force after spreading), and pressure coupling works for four-site rigid water.
 *   - The split calls (emdee_md_kick_drift, _kick, _fused_step) never place sites, as they never constrain; there is no emdee_dd_*
 *     counterpart.
 *   - The device time of placement and spreading is emdee_md_kernel_time index 13. */
int32_t emdee_md_set_vsites(emdee_md *md, const int32_t *atoms_dev, const double *weights_dev, int32_t n_sites);

/* Energy minimisation on the device: FIRE (Bitzek, Koskinen, Gaehler, Moseler & Gumbsch, Phys. Rev. Lett. 97, 170201 (2006);
 * build-defined like the integrator), for free atoms, rigid molecules (emdee_md_set_rigid3) and hbonds clusters
 * (emdee_md_set_hbonds) alike: what prepares a box with close contacts for emdee_md_step.
 * FIRE integrates the equations of motion with the engine's masses and steers the velocities towards the force.  With F the
 * force-field force, w = 1/m, the paper's constants N_min = 5, f_inc = 1.1, f_dec = 0.5, alpha_0 = 0.1, f_alpha = 0.99 and the
 * scalars dt = dt_start, alpha = alpha_0, n_pos = 0, iteration 0 evaluates F (with the energies), G and the sums below at the
 * entry positions; every later iteration is
 *   1. the step cap: t = the largest value <= dt with t v_max + t^2 a_max / 2 <= max_step, v_max and a_max bounding |v_i| and
 *      |w_i F_i| over the atoms now, so that no atom's unconstrained drift exceeds max_step (overlapping starts are safe);
 *   2. one closed step of emdee_md_step with t -- stages (a) to (e) of emdee_md_set_rigid3 for whichever tables exist around kick +
 *      drift, the displacement-triggered re-sort, the force pass (forces and energies) and the kick;
 *   3. G, the force with the constraint components removed: F itself without a table; with tables w F is handed to stage (e) in
 *      place of the velocities, and G = (the result) / w;
 *   4. one fp64 reduction in a fixed order: P = sum G . v, sum v . v, sum G . G, the largest |G_i|, |v_i| and |w_i F_i|; one
 *      read-back carries them and the potential energy;
 *   5. the stop test: g_max = max |G_i| <= f_tol ends the call, converged;
 *   6. the update: P > 0: v <- (1 - alpha) v + alpha sqrt(sum v . v / sum G . G) G, stage (e) once more with tables, and if
 *      ++n_pos > N_min, dt <- min(f_inc dt, dt_max) and alpha <- f_alpha alpha; P <= 0: v <- 0, dt <- f_dec dt, alpha <- alpha_0,
 *      n_pos <- 0.
 * max_iter bounds the iterations after iteration 0 (max_iter = 0 evaluates and reports).  out may be NULL.
 *   - Undivided engines only: EMDEE_ERR_STATE on an integrator lent by emdee_dd_engine, on one with ghosts and before
 *     emdee_md_set_state; the refusals of emdee_md_step for a latched fault, a table or charges that do not fit the state apply.
 *   - EMDEE_ERR_INVALID before anything is written unless max_iter >= 0, f_tol >= 0, 0 < dt_start <= dt_max, max_step > 0, all finite.
 *   - Velocities are OVERWRITTEN: zeroed at entry, zero at return.  Thermostat and barostat settings are neither applied nor
 *     changed, the box is untouched.  Every call starts FIRE afresh: two identical calls from identical states agree bit for bit.
 *   - Positions, forces and energies at return belong together: the result's energy is that of the returned positions, and
 *     emdee_md_step follows without emdee_md_set_state.  The virials are not evaluated: emdee_md_energies and an emdee_md_get_state
 *     of energies or virials run their pass over all outputs first, as after emdee_md_step.
 *   - A constraint group without a solution ends the call as it ends emdee_md_step: EMDEE_ERR_STATE naming the group.
 *   - Charges, Ewald and PME, bonded tables, exclusions and 1-4 pairs are part of the force pass and work as in emdee_md_step.
 *   - One blocking read-back per iteration (beside the rebuild word's): the scalars live on the host.  The device time of what the
 *     call adds to the stages of its steps (G, the reduction, the mixing) is emdee_md_kernel_time index 12. */
typedef struct {
    int32_t iterations;     /* force evaluations after the first */
    int32_t converged;      /* 1: g_max <= f_tol */
    int32_t rebuilds;       /* neighbour rebuilds during the call */
    int32_t reserved;
    double  energy0, energy;/* potential energy before / after */
    double  g_max;          /* largest |G_i| at the returned positions */
    double  dt;             /* FIRE's time step at return */
} emdee_minimize_result;
int32_t emdee_md_minimize(emdee_md *md, int32_t max_iter, double f_tol, double dt_start, double dt_max, double max_step,
                          emdee_minimize_result *out);

/* compute_nonbonded!(forces, energies, virials, positions, L, tiles, model, atoms, Val(bitmask))
 * -- src/nonbonded.jl:109-120 -- O(N) neighbour-list path, EMDEE_CUTOFF semantics.
 * Outputs not selected by bitmask may be NULL and are left untouched; selected outputs are
 * overwritten (the reference zero-fills then accumulates, src/nonbonded.jl:112-114). */
int32_t emdee_compute_nonbonded(emdee_ctx *ctx, void *forces_dev, void *energies_dev, void *virials_dev,
                                const void *positions_dev, double L, emdee_nbr *nbr,
                                emdee_lj_model model, const emdee_lj_atom *atoms_dev,
                                int32_t bitmask, int32_t precision);
/* Per-atom virial tensors of the same pairs, O(N) list path: W_i^ab = 1/2 sum_j (-E'r / r^2) d^a d^b with d = r_i - r_j the
 * minimum image, so that its trace is the VIRIALS output w_i.  tensor_dev: 6 x N reals, caller order, the six components
 * of an atom adjacent in the order (xx, yy, zz, xy, xz, yz); overwritten.  1-4 pairs add their scaled terms, excluded pairs
 * none.  The handle's list is kept or rebuilt as by emdee_compute_nonbonded.  EMDEE_ERR_INVALID: NULL tensor_dev. */
int32_t emdee_compute_virial_tensor(emdee_ctx *ctx, void *tensor_dev, const void *positions_dev, double L,
                                    emdee_nbr *nbr, emdee_lj_model model, const emdee_lj_atom *atoms_dev,
                                    int32_t precision);

/* compute_tile! semantics (src/nonbonded.jl:44-107) for any N: all-pairs 64x64 tiles,
 * one wavefront per tile pair, lane rotation through DPP/bpermute instead of shfl_sync.
 * mode = EMDEE_LITERAL reproduces the reference operator exactly (Q1). */
int32_t emdee_compute_nonbonded_tiles(emdee_ctx *ctx, void *forces_dev, void *energies_dev, void *virials_dev,
                                      const void *positions_dev, double L, int32_t N,
                                      emdee_lj_model model, const emdee_lj_atom *atoms_dev,
                                      int32_t bitmask, int32_t mode, int32_t precision);

/* naively_compute_nonbonded!(forces, energies, virials, positions, L, model, atoms)
 * -- src/nonbonded.jl:122-155 -- the plain double loop, one device thread per atom i over
 * all j != i (no tiles, no list, no lane exchange); always all three outputs. */
int32_t emdee_compute_nonbonded_naive(emdee_ctx *ctx, void *forces_dev, void *energies_dev, void *virials_dev,
                                      const void *positions_dev, double L, int32_t N,
                                      emdee_lj_model model, const emdee_lj_atom *atoms_dev,
                                      int32_t mode, int32_t precision);

/* ---------------------------------------------------------------- velocity-Verlet
 * Build-defined:  v += (dt/2m) f ; x += dt v ; f = F(x) ; v += (dt/2m) f.
 * The state lives on the device in cell order between calls.  The box is orthorhombic
 * [lo, lo+len) per dimension; periodic[d] != 0 applies the minimum-image convention along d.
 * Atoms 0..n_owned-1 are integrated; atoms n_owned..n_owned+n_ghost-1 are ghosts (images
 * owned by another domain): they act on owned atoms but receive no force and
 * are moved only by emdee_md_unpack_ghosts.  The single-GPU reference-shaped case is
 * lo = 0, len = L, periodic = {1,1,1}, n_ghost = 0.  What an axis with periodic[d] == 0 means for atoms beyond its faces, for the
 * box scale and for the entries that need three periodic axes: "Open axes" at emdee_md_set_state. */
int32_t emdee_md_create(emdee_ctx *ctx, const double lo[3], const double len[3], const int32_t periodic[3],
                        emdee_lj_model model, double skin, int32_t precision, emdee_md **out);
int32_t emdee_md_destroy(emdee_md *md);
/* (Re)load the state, in caller order.  velocities_dev has 3 n_owned reals; inv_mass_dev
 * (n_owned reals) may be NULL for m = 1 (LJAtom has no mass, src/lennard_jones.jl:15-18).
 * Bins, sorts, builds the neighbour list and evaluates the forces.
 * Positions may lie outside the box: on a periodic axis the engine works on the image inside [lo, lo+len) and keeps, per atom
 * and axis, the number of box lengths it removed (10 bits: -512 .. 511), so that emdee_md_get_state answers in the caller's
 * image.  Positions up to 500 box lengths from the box are always accepted.  An atom whose count would leave the field is
 * refused: EMDEE_ERR_INVALID naming the atom, the axis and the count, and the engine then holds no state (as before the first
 * emdee_md_set_state) until a valid one is loaded.  Between 500 box lengths and that refusal the outcome is unspecified (the
 * count of a Float32 engine includes the step to the image next to the atom's cell).  Open axes keep no count.
 * The counts grow as atoms travel: when a rebuild inside emdee_md_step would push one out of the field, that atom's count
 * stays at the limit (no other atom's position is affected), the call whose read-back sees it returns EMDEE_ERR_STATE naming
 * the atom, and emdee_md_step and emdee_md_minimize refuse until the state is replaced.  That call ends inside a step (positions
 * drifted, velocities half kicked, the forces of that step not evaluated): positions of every other atom read afterwards are
 * right, velocities are not those of a completed step, and the force plane is the step before's (a read of energies or virials
 * evaluates all three afresh, as does the next emdee_md_step after a new state).
 *
 * Open axes (periodic[d] == 0; a slab has one, a droplet three).  The walls lo[d] and lo[d] + len[d] of an open axis are not walls:
 * they only place the cell grid.  No minimum image is taken along d anywhere -- pair terms, bonded terms, rigid molecules, bonds to
 * hydrogen, virtual sites, restraints and pull all use the plain difference -- so a molecule may be longer than len[d] / 2 along d.
 *   - An atom beyond a face, at the load or after steps, is binned into the outermost cell of that side, gets no image count, and
 *     comes back from emdee_md_get_state where it is (fp64: the bits it was given until it moves).
 *   - Results are guaranteed for atoms up to D beyond a face, with w the widest cell, w_d = len[d] / floor(len[d] / (cutoff + skin)):
 *     D = 12 w for a Float64 engine, D = 32 - 6 w length units for a Float32 engine ("Open axes", derives both).  Further
 *     out the outcome is unspecified, not refused: a Float64 neighbour list may then misjudge a pair within 1e-6 of cutoff + skin, a
 *     Float32 pair no longer sees the same separation from both of its atoms.  Many atoms far out also crowd the outermost cells.
 *   - emdee_md_scale_box and the barostats treat an open axis as any other: x_d <- lo_d + mu_d (x_d - lo_d), len_d <- mu_d len_d
 *     (without the 2 (cutoff + skin) test, which is the minimum image's), and the volume in every pressure is len_0 len_1 len_2,
 *     the open lengths included -- choose them as the volume the pressure is meant for, or give the axis a compressibility of 0:
 *     a factor mu_d of exactly 1 leaves len_d and every coordinate along d bit for bit.
 *   - Refused on a box with an open axis, each EMDEE_ERR_STATE with its own text: emdee_md_set_ewald, emdee_md_set_pme,
 *     emdee_md_set_rdf.  emdee_dd_create takes a fully periodic global box.  Everything else accepts open axes. */
int32_t emdee_md_set_state(emdee_md *md, int32_t n_owned, int32_t n_ghost, const void *positions_dev,
                           const void *velocities_dev, const emdee_lj_atom *atoms_dev,
                           const void *inv_mass_dev);
/* Copy the state back in caller order; any pointer may be NULL. positions: n_owned+n_ghost
 * atoms; velocities/forces/energies/virials: n_owned atoms.
 * Positions come back unwrapped, in the image the caller loaded plus what the atom has travelled since: exact to the engine's
 * rounding for atoms up to 500 box lengths from the box on a periodic axis (the limit of the image counts, see
 * emdee_md_set_state). */
int32_t emdee_md_get_state(emdee_md *md, void *positions_dev, void *velocities_dev, void *forces_dev,
                           void *energies_dev, void *virials_dev);
/* nsteps whole steps (n_ghost must be 0: a decomposed run drives the split calls below).
 * rebuild_every > 0: fixed cadence; 0: rebuild when max displacement > skin/2.
 * Every inner step is one kernel (force + kick + drift).  With the displacement trigger the steps are
 * queued a few at a time and read back once per batch; a step queued behind one that asked for a
 * rebuild checks a device word first and does nothing, so the states produced are exactly those of
 * stepping one at a time, and a given sequence of calls is bitwise reproducible from run to run
 * (deterministic cell order, owner-computes sums, no floating-point atomics). */
int32_t emdee_md_step(emdee_md *md, int32_t nsteps, double dt, int32_t rebuild_every);
/* split step for domain-decomposed runs:  kick_drift -> [halo exchange] -> forces -> kick */
/* v += kick (dt/m) f ; x += dt v (owned).  kick = 0.5: the opening half kick; kick = 1.0 also
 * carries the closing half kick of the previous step (same f), saving one pass over v and f. */
int32_t emdee_md_kick_drift(emdee_md *md, double dt, double kick);
/* f (and e, w) of owned atoms.  phase 0: all atoms; phase 1: only bricks whose LDS tile holds no
 * ghost cell (can run while the halo exchange is in flight); phase 2: the remaining bricks.
 * A charged engine (emdee_md_set_coulomb) has kernels for EMDEE_FORCES and for all three outputs only: a narrower request
 * (2 .. 6) evaluates all three, so the force plane is rewritten too, with the all-outputs kernel's rounding (an uncharged
 * engine leaves it alone: every plane the bitmask leaves out keeps its bits, on every kernel family -- where the all-outputs
 * kernel serves a narrower request, the 1024-thread brick variant and the two-species kernels, its other outputs go to spare
 * planes). */
int32_t emdee_md_forces(emdee_md *md, int32_t bitmask, int32_t phase);
int32_t emdee_md_kick(emdee_md *md, double dt);              /* v += (dt/2m) f */
/* One inner step as a single kernel: f = F(x), v += kick (dt/m) f, x += dt v, with the new positions
 * written to the second position buffer.  phase as in emdee_md_forces; the buffers are swapped after
 * phase 0 or phase 2, so a decomposed run calls phase 1 (interior bricks, while the halo exchange of
 * the CURRENT positions is in flight), unpacks the ghosts, then phase 2.  Sets *fused = 0 and does
 * nothing if the LDS-tiled kernels are not in use for this box (caller falls back to the split step). */
int32_t emdee_md_fused_step(emdee_md *md, double dt, double kick, int32_t phase, int32_t *fused);
/* 1 if some owned atom moved more than skin/2 since the last build. Blocking. */
int32_t emdee_md_needs_rebuild(emdee_md *md, int32_t *flag);
/* re-bin, re-sort and rebuild the neighbour list from the current positions */
int32_t emdee_md_rebuild(emdee_md *md);
/* halo: gather positions of the listed atoms (caller-order ids, dev int32[n]) into buf (3 n
 * reals), each plus the periodic-image shift shifts[3 codes[k] .. +2] (codes_dev: dev int32[n],
 * NULL = every atom uses shifts[0..2]; n_shifts <= 27 rows of 3 doubles on the HOST); and scatter
 * received positions into ghost slots first..first+n-1 (ghost-relative). */
int32_t emdee_md_pack_positions(emdee_md *md, const int32_t *ids_dev, const int32_t *codes_dev, int32_t n,
                                const double *shifts, int32_t n_shifts, void *buf_dev);
int32_t emdee_md_unpack_ghosts(emdee_md *md, const void *buf_dev, int32_t first, int32_t n);
/* totals over owned atoms: out[0] = potential energy (sum of per-atom halves), out[1] =
 * kinetic energy, out[2] = virial sum.  Evaluates energies/virials if needed. Blocking. */
int32_t emdee_md_energies(emdee_md *md, double out[3]);
/* per-atom virial tensors of the owned atoms (emdee_compute_virial_tensor's convention): tensor_dev 6 x n_owned reals, caller
 * order.  Evaluates them if they are not current (one extra pass over the list; the forces are left as they are, so a query
 * does not change the trajectory).  Ordered against the caller's stream.  EMDEE_ERR_STATE before emdee_md_set_state,
 * EMDEE_ERR_INVALID for a NULL tensor_dev. */
int32_t emdee_md_virial_tensor(emdee_md *md, void *tensor_dev);
/* box totals over owned atoms, fp64, deterministic: out[0..5] = sum_i W_i, out[6..11] = kinetic tensor K^ab = sum_i m_i v^a v^b
 * (the velocities emdee_md_energies takes: tr K = 2 x its kinetic energy), both (xx, yy, zz, xy, xz, yz).  The pressure
 * tensor is (K + W) / V.  Evaluates the tensors if needed.  Blocking. */
int32_t emdee_md_pressure_tensor(emdee_md *md, double out[12]);
/* Molecular pressure and centre-of-mass scaling: constant pressure for rigid molecules (build-defined).
 *
 * Molecules.  The molecules are those of the rigid table in force (emdee_md_set_rigid3); every other owned atom is a molecule
 * of one atom.  A rigid molecule with sites k = 0 (apex), 1, 2 is assembled exactly as the constraint stages assemble it: y_0 =
 * the apex record in double (plus its cell's origin for the cell-relative records of a Float32 engine), y_1 and y_2 = y_0 + the
 * minimum images of the legs from it.  For a caller: with x the unwrapped positions of emdee_md_get_state, y_0 = x_apex and
 * y_k = x_apex + (x_k - x_apex) - len rint((x_k - x_apex) / len) on the periodic axes.  Then
 *   M = sum_k m_k ;  Y = sum_k m_k y_k / M ;  V = sum_k m_k v_k / M ;  d_k = y_k - Y
 * (Y and V are formed from differences to the apex, not from an average of far numbers).
 *
 * Molecular sums, fp64, deterministic, order (xx, yy, zz, xy, xz, yz):
 *   W_mol^ab = W^ab - sum_mol sum_k 1/2 (d_k^a f_k^b + d_k^b f_k^a)
 *   K_mol^ab = K^ab - sum_mol (sum_k m_k v_k^a v_k^b - M V^a V^b)
 * W and K are the atomic sums of emdee_md_pressure_tensor; f_k are the engine's current force-field forces (the forces
 * emdee_md_get_state returns: Lennard-Jones, Coulomb, reciprocal space, 1-4 and bonded terms, no constraint forces).  sum d (x) f
 * is not symmetric -- molecules carry torques -- so its off-diagonals are symmetrised; the barostats use the diagonal.
 *   P_mol = (K_mol + W_mol) / V.
 * Constraint forces are internal to a molecule and sum to zero: they drop out of W_mol exactly, and tr W_mol is -dU/dln(mu) of
 * the molecular scale below, the volume derivative under the scaling actually applied.
 *
 * emdee_md_molecular_pressure_tensor: out[0..5] = W_mol, out[6..11] = K_mol.  Evaluates the tensor pass as
 * emdee_md_pressure_tensor does, and the forces if they are not current, as emdee_md_energies does.  Available whether or not
 * the switch below is on.  Without a rigid table it returns emdee_md_pressure_tensor's twelve numbers: the same kernels, nothing
 * added.  Blocking, one read-back (the atomic and the molecules' totals come back in one copy; the host subtracts).
 * EMDEE_ERR_STATE before emdee_md_set_state, and with a table set for another atom count or one the state did not fit (the
 * conditions emdee_md_step refuses on).
 *
 * Molecular scale by mu, velocity_scale: the box and every one-atom molecule scale exactly as emdee_md_scale_box scales them.
 * Every site of a rigid molecule moves by (mu_d - 1) (C_k,d - lo_d), where C_k = Y + (r_k - y_k) is the image of the centre of
 * mass that goes with that site's record r_k (r_k - y_k is a whole number of box lengths): the stored image counts stay valid,
 * the unwrapped coordinates of emdee_md_get_state transform consistently, and the molecule's minimum-image geometry is a pure
 * translation.  The shift is added to each record in its own frame in double and rounded once.  Velocities of the members:
 * v_k <- v_k + (velocity_scale - 1) V -- the centre-of-mass momentum scales, the rotation is untouched; velocity_scale = 1 leaves
 * the velocity planes bit for bit.  Then the re-bin, re-plan, rebuild and force pass of emdee_md_scale_box.  No re-projection
 * follows: distances and bond-relative velocities are unchanged up to rounding.
 *
 * emdee_md_set_molecular_scaling(on): 0 (the default) -- everything behaves as without this call, the three refusals of
 * emdee_md_set_rigid3's text included.  1 --
 *   - emdee_md_scale_box on an engine with a rigid table performs the molecular scale (EMDEE_ERR_STATE with a table set for
 *     another atom count or one the state did not fit; the all-or-nothing checks of mu and the 2 (rc + skin) limit are unchanged);
 *   - emdee_md_set_barostat is accepted with a table in force, and emdee_md_set_rigid3 while a barostat is on;
 *   - the coupling events of an engine with a table take P from the molecular sums, for all three couplings, always through
 *     the tensor path (one tensor pass per event): P_d = (K_mol^dd + W_mol^dd) / V, isotropic P = tr(K_mol + W_mol) / (3 V);
 *     mu and velocity_scale from the formulas of emdee_md_set_barostat, applied with the molecular scale.
 *   - with a molecule table in force (emdee_md_set_molecules, below) the three entries take their molecules from it, and an
 *     engine with an hbonds table is accepted by all of them.
 * On an engine without a table the switch changes nothing, bit for bit.  emdee_md_energies and emdee_md_pressure_tensor return
 * atomic values always.  EMDEE_ERR_INVALID for on outside {0, 1}; EMDEE_ERR_STATE on an integrator lent by emdee_dd_engine or
 * with ghosts, and for switching off while a barostat is on and a table is in force (the setting stays).
 * The device time of the molecular sums and the molecular scale is emdee_md_kernel_time index 10.
 * Scope: undivided orthorhombic boxes, the molecules of the rigid table or of the molecule table below; no emdee_dd_* counterpart.
 *
 * Whole molecules of any size.  The definitions above hold for ANY partition of the atoms into groups, as long as every
 * constraint lies inside one group: constraint forces are internal to a group and sum to zero, so they drop out of W_mol whatever
 * the group's size, and tr W_mol is -dU/dln(mu) of the scale that translates each group with its centre of mass.  The natural unit
 * is the whole molecule (solute, water, lipid, polymer chain): bonded geometry, constraint geometry and rotation then survive a box
 * scale to rounding.
 * emdee_md_set_molecules(molecule_dev, n): n = n_owned int32 ids in caller order on the device, each >= -1; equal ids >= 0 form one
 * molecule (ids need not be dense or ordered), -1 is a molecule of one.  The array is copied; the call blocks.  n = 0 with NULL
 * clears the table.  While a table is in force AND emdee_md_set_molecular_scaling is on, emdee_md_molecular_pressure_tensor,
 * emdee_md_scale_box and every barostat event take their molecules from this table instead of the rigid table: the inner sums of
 * W_mol and K_mol run over all atoms of each molecule; the scale moves every atom of a molecule by (mu - 1) (Y - lo) and adds
 * (velocity_scale - 1) V to its velocity.  An engine with an hbonds table then accepts emdee_md_scale_box, emdee_md_set_barostat
 * (Berendsen with all three couplings, C-rescale), emdee_md_molecular_pressure_tensor, and emdee_md_set_hbonds while a barostat is
 * on.  Without a table, or with the switch off, every entry behaves as before this call existed, texts and bits alike.
 *   - Centres of mass are formed in fp64 from the UNWRAPPED coordinates (the record plus the image counts kept per atom, as
 *     restraints and the pull take them), every difference relative to the molecule's first atom: a molecule may be larger than
 *     half a box, so THE CALLER LOADS EVERY MOLECULE WHOLE (emdee_md_set_pull has the same contract).  A record's shift uses the
 *     image of Y that goes with it, r' = r + (mu - 1) (Y - k L - lo) with k its image counts: the stored counts stay valid.
 *   - Three launches per use: the centres (one thread per molecule of up to 8 atoms, one wavefront per larger one), then the
 *     sums over the table's entries (the two-stage reduction of every box sum) or the shift (one thread per entry).  No atomics; the
 *     order of every sum depends on the table alone: the same bits in every run.  Molecules of one atom are left out of the table:
 *     they add exactly 0 and scale as free atoms do.  Timed under emdee_md_kernel_time index 10.
 *   - A virtual site may carry any id: it is massless and carries no force after spreading, so it adds nothing to the sums; after
 *     the scale the sites go back on their scaled parents.
 *   - All or nothing, as emdee_md_set_rigid3: the previous table stays in force on refusal.  EMDEE_ERR_INVALID: n neither 0 nor
 *     n_owned, NULL with n > 0, an id below -1, a rigid molecule or an hbonds cluster of the tables in force whose atoms do not
 *     all carry one id >= 0 (the constraint would not be internal to a molecule; emdee_md_set_rigid3 and emdee_md_set_hbonds refuse
 *     the same group the other way round).  EMDEE_ERR_STATE, from one device check and one read-back: a molecule whose total mass
 *     is 0; a molecule that is not loaded whole -- for a constraint group inside it the unwrapped distance of two sites is off
 *     the table's distance by more than 1e-3 (relative), the common mistake of wrapping a state atom by atom.  EMDEE_ERR_STATE
 *     before emdee_md_set_state, with ghosts, on an integrator lent by emdee_dd_engine; and for clearing the table, or switching
 *     emdee_md_set_molecular_scaling off, while a barostat is on and an hbonds table is in force.
 *   - The table survives an emdee_md_set_state with the same atom count and is checked against the new state; after a state with
 *     another count, or one that did not fit, emdee_md_step returns EMDEE_ERR_STATE until it is set again or cleared.
 *   - Restraint references, the pull, the minimiser, the thermostats and the count of degrees of freedom do not read the table.
 *     The Green-Kubo stress of a rigid-only engine takes whichever molecular sums are in force; an hbonds table keeps refusing
 *     both Green-Kubo masks.  The radial distribution functions keep their own molecule argument.
 * Scope: undivided orthorhombic boxes; no emdee_dd_* counterpart. */
int32_t emdee_md_molecular_pressure_tensor(emdee_md *md, double out[12]);
int32_t emdee_md_set_molecular_scaling(emdee_md *md, int32_t on);
int32_t emdee_md_set_molecules(emdee_md *md, const int32_t *molecule_dev, int32_t n);
int32_t emdee_md_nbr_stats(emdee_md *md, int64_t *builds, int64_t *listed, int32_t *max_count,
                           int32_t *capacity);
int32_t emdee_md_count_pairs(emdee_md *md, int64_t *pairs_in_cutoff);
/* Per-kernel device time from HIP events recorded on the context's stream while
 * profiling is on.  kernel: 0 = lj_force_nbr (plain force launches), 1 = verlet_kick_drift, 2 = rebuild
 * (bin + sort + nbr_build), 3 = verlet_kick, 4 = lj_force_nbr with the velocity-Verlet update fused in
 * (emdee_md_step's inner steps, emdee_md_fused_step); 8 = the reciprocal-space pass of an Ewald engine (emdee_md_set_ewald, emdee_md_set_pme),
 * which index 0 contains as well; 9 = the constraint stages of an engine with rigid molecules (emdee_md_set_rigid3);
 * 10 = its molecular sums and molecular scale (emdee_md_molecular_pressure_tensor, emdee_md_set_molecular_scaling), and those of a
 * molecule table (emdee_md_set_molecules);
 * 11 = the constraint stages of an engine with an hbonds table (emdee_md_set_hbonds); 12 = what emdee_md_minimize adds to the
 * stages of its steps (the constrained force, the reduction, the mixing); 13 = placement and force spreading of an engine with
 * virtual sites (emdee_md_set_vsites); 14 = the three launches of every event of a global thermostat (emdee_md_set_thermostat);
 * 15 = the four stages of every sample of the radial distribution functions (emdee_md_rdf_sample);
 * 16 = the three launches of every sample of the displacement and velocity correlations (emdee_md_msd_sample);
 * 17 = the launches every sample of the Green-Kubo observables adds to the tensor pass (emdee_md_gk_sample);
 * 18 = the launch the position restraints add to every force pass, and the scaling of their references (emdee_md_set_restraints);
 * 19 = the three launches the centre-of-mass pull adds to every force pass (emdee_md_set_pull);
 * 20 = the row pass of the alchemical table at every rebuild and its launches behind every force pass (emdee_md_set_alchemical).
 * Blocking. */
int32_t emdee_md_profile(emdee_md *md, int32_t enable);
int32_t emdee_md_kernel_time(emdee_md *md, int32_t kernel, double *total_ms, int64_t *launches);

/* Langevin thermostat (build-defined like the integrator: the reference has neither).
 * gamma > 0 switches it on for every later step of this integrator, gamma <= 0 off.  Each step becomes
 *   v += (dt/2) f/m ;  v = c1 v + c2 sqrt(T/m) xi ;  x += dt v ;  f = F(x) ;  v += (dt/2) f/m
 * with c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2) and xi three N(0,1) numbers that are a pure function of
 * (seed, step number, atom id): splitmix64-finalised counters + Box-Muller, so a run is reproducible whatever
 * the sort order or the decomposition.  Steps are numbered from first_step (pass the number of steps already
 * done when resuming).  The O step rides in the kick/drift pass (the fused step kernel or verlet_kick_drift);
 * the noise itself comes from one extra streaming kernel per step. */
int32_t emdee_md_set_langevin(emdee_md *md, double gamma, double temperature, uint64_t seed, uint64_t first_step);
/* Atom ids for the noise counters: device array in caller order, one int64 per owned atom (decomposed runs pass
 * global ids); NULL = the caller index.  Not copied: must stay valid, and is forgotten by emdee_md_set_state. */
int32_t emdee_md_set_langevin_ids(emdee_md *md, const int64_t *ids_dev);
/* The generator on its own, for tests: out_dev[3 i .. 3 i + 2] = xi(seed, step, ids_dev[i]). */
int32_t emdee_md_langevin_normals(emdee_md *md, uint64_t seed, uint64_t step, const int64_t *ids_dev, int32_t n,
                                  double *out_dev);

/* Pressure coupling (build-defined like the integrator and the thermostat: the reference has neither).  The box of an
 * undivided integrator is no longer fixed at create: emdee_md_scale_box rescales box, positions and velocities, and
 * emdee_md_set_barostat makes emdee_md_step do so every `every` steps from the pressure the engine measures itself.
 *
 * emdee_md_get_box: the current lo and len (len changes with every scale; lo never does).
 *
 * emdee_md_scale_box(mu, velocity_scale), the primitive (also for callers who drive the split calls):
 *   x_d   <- lo_d + mu_d (x_d - lo_d)        every owned atom, in fp64 arithmetic in both precisions (the unwrapped coordinate
 *                                            emdee_md_get_state returns scales the same way: image counts are kept)
 *   len_d <- mu_d len_d ;  lo stays
 *   v     <- velocity_scale v                (1.0 leaves the velocities bit for bit)
 * then the engine re-bins on the new box, re-plans, rebuilds the list and evaluates the forces at the new positions, as
 * emdee_md_rebuild followed by a force pass: on return forces, energies and virials belong to the new box.  Exclusion, 1-4,
 * bonded and charge tables stay in force (their slots are re-recorded by the rebuild).  The scaling is atomic, not by molecule
 * centres (for the molecules of a rigid table: emdee_md_set_molecular_scaling).  All or nothing:
 *   - EMDEE_ERR_INVALID, with box, state and list untouched and the engine still able to step, for a non-finite or
 *     non-positive mu_d or velocity_scale, and for a new periodic length below 2 (rc + skin);
 *   - EMDEE_ERR_STATE before emdee_md_set_state, with ghosts, and on an integrator lent by emdee_dd_engine.
 * emdee_md_step always returns with its last half kick closed, so a scale between two calls of it acts on full-step
 * velocities and on forces of the unscaled positions; a caller of the split calls closes its own (emdee_md_kick) first.
 *
 * emdee_md_set_barostat switches coupling on for every later emdee_md_step of this integrator (kind = EMDEE_BAROSTAT_OFF:
 * off; the other arguments are then not looked at).  Steps are numbered from first_step, as for the thermostat.  After the
 * step that brings the count s to a multiple of `every`, with Dt = every dt, V the volume and the instantaneous pressure
 * P^aa = (K^aa + W^aa) / V from the deterministic fp64 sums of emdee_md_pressure_tensor (isotropic: P = (2 KE + W) / (3 V)
 * from the sums of emdee_md_energies, which the event's own force pass evaluates -- the event's one read-back):
 *   Berendsen:   mu_d = 1 - (Dt / (3 tau_p)) beta_d (P_ref,d - P_d),  velocity_scale = 1
 *     isotropic:       one factor from P = (Pxx + Pyy + Pzz) / 3, p_ref[0], compressibility[0]
 *     semi-isotropic:  x and y share a factor from (Pxx + Pyy) / 2, p_ref[0], compressibility[0]; z its own from Pzz,
 *                      p_ref[2], compressibility[2]
 *     anisotropic:     three factors from Pxx, Pyy, Pzz and their own entries; the box stays orthorhombic
 *   C-rescale (stochastic cell rescaling, Bernetti & Bussi, J. Chem. Phys. 153, 114107 (2020); isotropic only):
 *     d_eps = -(beta / tau_p) (P_ref - P) Dt + sqrt(2 T beta Dt / (V tau_p)) xi
 *     mu = exp(d_eps / 3) on all three sides, velocity_scale = 1 / mu
 *     T = temperature in energy units (as emdee_md_set_langevin takes it); xi = component 0 of the thermostat's generator at
 *     (seed, s, id = -1), i.e. out_dev[0] of emdee_md_langevin_normals(md, seed, s, {-1}, 1, out_dev): a run is reproducible.
 * and then emdee_md_scale_box(mu, velocity_scale).  A coupling event always rebuilds; a fixed rebuild_every cadence restarts
 * from the event.  A refusal from the scale (a box shrunk below 2 (rc + skin), a non-finite mu from a NaN pressure) comes
 * back as EMDEE_ERR_STATE from emdee_md_step, the state being that of the completed step before the event.
 * With coupling on, emdee_md_step closes the half kick of every step (kick + drift, force pass, kick; no merged kicks and no
 * run-ahead): the states after s steps do not depend on how the steps were dealt to calls -- step(40), 8 x step(5) and
 * 40 x step(1) agree bit for bit -- no step is queued beyond an event, and the run stays bitwise reproducible.  The split
 * calls (emdee_md_kick_drift, _forces, _kick, _fused_step) never couple on their own.
 *   - All or nothing: EMDEE_ERR_INVALID, the previous setting in force, for an unknown kind or coupling, every < 1, tau_p
 *     not finite or <= 0, a non-finite p_ref, a negative or non-finite compressibility (all three entries are checked), a
 *     NULL array, C-rescale with another coupling than isotropic or with temperature <= 0.
 *   - EMDEE_ERR_STATE on an integrator lent by emdee_dd_engine and on one with ghosts.
 * Scope: undivided orthorhombic boxes.  There is no emdee_dd_set_barostat -- the domain geometry of emdee_dd is fixed at
 * create --, nothing on the operator path, no triclinic box, no long-range dispersion correction to the pressure. */
#define EMDEE_BAROSTAT_OFF        0
#define EMDEE_BAROSTAT_BERENDSEN  1
#define EMDEE_BAROSTAT_CRESCALE   2     /* stochastic cell rescaling, Bernetti & Bussi 2020 */
#define EMDEE_COUPLE_ISOTROPIC     0    /* one factor from P = (Pxx+Pyy+Pzz)/3 */
#define EMDEE_COUPLE_SEMIISOTROPIC 1    /* x and y share a factor from (Pxx+Pyy)/2, z its own from Pzz */
#define EMDEE_COUPLE_ANISOTROPIC   2    /* three factors from Pxx, Pyy, Pzz; the box stays orthorhombic */
int32_t emdee_md_get_box(emdee_md *md, double lo[3], double len[3]);
int32_t emdee_md_scale_box(emdee_md *md, const double mu[3], double velocity_scale);
int32_t emdee_md_set_barostat(emdee_md *md, int32_t kind, int32_t coupling, const double p_ref[3],
                              const double compressibility[3], double tau_p, int32_t every, double temperature,
                              uint64_t seed, uint64_t first_step);

/* Global thermostats (build-defined like the integrator: the reference has none).  Where the Langevin thermostat gives every
 * atom friction and noise of its own, these reduce the kinetic energy K = sum m v^2 / 2 of the owned atoms, update a few scalars
 * and multiply every velocity by one factor alpha, which leaves hydrodynamics alone and keeps the RATTLE conditions (linear and
 * homogeneous in v): they compose with every table of the engine.
 *
 * emdee_md_set_thermostat switches one on for every later emdee_md_step of this integrator (kind = EMDEE_THERMOSTAT_OFF: off,
 * the other arguments are then not looked at, and the engine behaves as if the call had never been made, bit for bit).
 *   temperature: kT in energy units, as emdee_md_set_langevin takes it; tau_t: the relaxation time; every >= 1: the steps between
 *   events; chain: the chain length M in 1...8 (kind NOSE_HOOVER only); seed, first_step: v-rescale's noise and the numbering of
 *   the steps, as for the barostat; n_dof > 0: the degrees of freedom, taken as given; n_dof == 0: the library's own count,
 *   evaluated at every emdee_md_step from the tables then in force,
 *     3 (n_owned - n_sites) - 3 n_rigid_molecules - (satellites of the hbonds table) - 3,
 *   which must be at least 3 (else emdee_md_step returns EMDEE_ERR_STATE).
 * With a thermostat on, emdee_md_step closes the half kick of every step, as with a barostat: the states after s steps do not
 * depend on how the steps were dealt to calls, bit for bit.  After the step that brings the count s to a multiple of `every`
 * (after the velocity stage of the constraints, before the barostat's event), with Delta = every dt:
 *   v-rescale (EMDEE_THERMOSTAT_VRESCALE; Bussi, Donadio & Parrinello, J. Chem. Phys. 126, 014101 (2007)):
 *     c = exp(-Delta / tau_t), Kbar = n_dof kT / 2, R1 ~ N(0,1), S ~ chi-squared with n_dof - 1 degrees of freedom,
 *     alpha^2 = c + (1 - c) (S + R1^2) Kbar / (n_dof K) + 2 R1 sqrt(c (1 - c) Kbar / (n_dof K)),  alpha = +sqrt(alpha^2)
 *     (alpha = 1 for K = 0);  E_th -= (alpha^2 - 1) K.
 *     {R1, S} are a pure function of (seed, s, n_dof): emdee_md_thermostat_draws returns them (the generator of the Langevin
 *     noise at ids -2, -3, ...; S = 2 Gamma((n_dof - 1) / 2) by Marsaglia & Tsang with at most 64 attempts).
 *   Nose-Hoover chain (EMDEE_THERMOSTAT_NOSE_HOOVER; Martyna, Tuckerman, Tobias & Klein, Mol. Phys. 87, 1117 (1996)):
 *     Q_1 = n_dof kT tau_t^2, Q_k = kT tau_t^2; the MTK factorisation without Suzuki-Yoshida weights, two passes of Delta / 2
 *     (DESIGN.md 4f has the lines); alpha is the product of the passes' factors exp(-(Delta / 2) v_1);
 *     E_th = sum Q_k v_k^2 / 2 + n_dof kT xi_1 + kT sum_{k > 1} xi_k.
 *   then v <- alpha v on every owned atom (fp64 product in both precisions).  U + K + E_th is the conserved quantity.
 * One application over Delta per event instead of Delta / 2 before and after the step: the sequence of states is the symmetric
 * integrator's, seen half a thermostat operation later.  An event is three launches on the engine's stream and no read-back;
 * their device time is emdee_md_kernel_time index 14.  emdee_md_minimize leaves the thermostat out and its state untouched.
 *
 * emdee_md_thermostat_state (blocking): out[0] = n_dof in use, [1] = K as the last event saw it, before its scaling, [2] = that
 * event's alpha, [3] = E_th, [4..11] = xi_k, [12..19] = v_xi_k (unused chain slots 0).  emdee_md_set_thermostat zeroes words
 * 1-19; emdee_md_set_thermostat_state writes words 3-19.  A restart is emdee_md_set_thermostat with first_step = the steps done,
 * then emdee_md_set_thermostat_state with the words read before.
 *   - All or nothing: EMDEE_ERR_INVALID, the previous setting in force, for an unknown kind, a temperature or tau_t that is not
 *     finite or <= 0, every < 1, n_dof < 0, chain outside 1...8 with kind NOSE_HOOVER, a NULL array.
 *   - EMDEE_ERR_STATE on an integrator lent by emdee_dd_engine and on one with ghosts; for a kind other than OFF while the
 *     Langevin thermostat is on (gamma > 0), and from emdee_md_set_langevin with gamma > 0 while a global thermostat is on.
 * Scope: undivided boxes; no emdee_dd_* counterpart. */
#define EMDEE_THERMOSTAT_OFF          0
#define EMDEE_THERMOSTAT_VRESCALE     1     /* stochastic velocity rescaling, Bussi, Donadio & Parrinello 2007 */
#define EMDEE_THERMOSTAT_NOSE_HOOVER  2     /* Nose-Hoover chain, Martyna, Tuckerman, Tobias & Klein 1996 */
#define EMDEE_THERMOSTAT_WORDS        20
int32_t emdee_md_set_thermostat(emdee_md *md, int32_t kind, double temperature, double tau_t, int32_t every, int64_t n_dof,
                                int32_t chain, uint64_t seed, uint64_t first_step);
int32_t emdee_md_thermostat_state(emdee_md *md, double out[EMDEE_THERMOSTAT_WORDS]);
int32_t emdee_md_set_thermostat_state(emdee_md *md, const double in[EMDEE_THERMOSTAT_WORDS]);
int32_t emdee_md_thermostat_draws(emdee_md *md, uint64_t seed, uint64_t step, int64_t n_dof, double out[2]);

/* Radial distribution functions (build-defined: the reference has no structural analysis).  The engine histograms the pair
 * distances of its current positions on the device, so that g(r) of a liquid -- g_OO, g_OH and g_HH of water -- costs no copy of
 * the positions to the host and no O(N^2) loop there.
 *
 * emdee_md_set_rdf(r_max, n_bins, n_groups, group_dev, molecule_dev) sets the table (blocking; n_bins = 0 clears it):
 *   n_groups in 1...8.  group_dev: n_owned int32 in caller order on the device, each in -1...n_groups-1; -1 leaves the atom out;
 *   NULL with n_groups == 1 puts every atom in group 0.  molecule_dev: NULL, or n_owned int32; a pair whose two entries are equal
 *   and >= 0 is intramolecular and is skipped; -1: the atom has no molecule.  Both arrays are copied, the group sizes are counted.
 *   One histogram per unordered pair of groups a <= b, in slot s(a, b) = a n_groups - a (a - 1) / 2 + (b - a); bin k of it is
 *   counts[s n_bins + k], a 64-bit integer on the device.  n_bins >= 1 and n_pairs n_bins <= 8192 (a workgroup keeps a private
 *   histogram in 32 KB of LDS); r_max finite, > 0 and at most half the shortest box side.  Setting a table zeroes the accumulators.
 *   - All or nothing: EMDEE_ERR_INVALID, the previous table in force, for arguments outside these limits; for a group or molecule
 *     value out of range the text names the first offending atom.
 *   - EMDEE_ERR_STATE, each with its own text: before emdee_md_set_state, on an integrator lent by emdee_dd_engine, on one with
 *     ghosts, on a box with an open axis.
 *
 * emdee_md_rdf_sample adds the current positions as one frame: work queued on the engine's stream, nothing read back.  Every
 * unordered pair {i, j} of grouped atoms that do not share a molecule is counted exactly once: its minimum-image distance r in
 * fp64 from the engine's records as doubles (a Float32 engine: the cell-relative record plus the origin of its cell), bin
 * (int)(r inv_dr) with inv_dr = n_bins / r_max formed once in double, dropped when the bin is n_bins or more.  The sums are
 * integers: the counts are exact and bitwise reproducible.  The host adds 1 to frames and 1 / V of the current box to
 * inv_volume_sum.  The sample bins the atoms on a grid of its own, made from the positions as they are: it does not read the
 * neighbour list and is exact whatever the list's age.  It does not touch the engine: no re-sort, no rebuild, no force pass; an
 * engine that samples and one that does not stay bit for bit equal.  Its device time is emdee_md_kernel_time index 15.
 *   - EMDEE_ERR_STATE, the accumulators untouched: no table is set; the table was set for another atom count; a barostat has
 *     shrunk the box so that r_max exceeds half the shortest side.
 * Sampling on a cadence inside emdee_md_step is not offered: emdee_md_step ends with a read-back anyway, so step(n) followed by
 * a sample costs nothing more.
 *
 * emdee_md_rdf_read (blocking; any pointer may be NULL): the n_pairs n_bins counts, the eight group sizes, frames and
 * inv_volume_sum.  emdee_md_rdf_reset zeroes the counts, frames and inv_volume_sum.  From them, with r_k = r_max k / n_bins,
 *   g_ab(k) = counts / (P_ab (4 pi / 3) (r_{k+1}^3 - r_k^3) inv_volume_sum),  P_ab = N_a N_b (a != b),  P_aa = N_a (N_a - 1) / 2,
 * and the running coordination number of b around a is the cumulative sum of the counts, times 2 for a == b, over N_a frames.
 * The pairs skipped as intramolecular are not taken out of P_ab, as is usual.
 * Scope: undivided boxes, periodic in all three dimensions; no emdee_dd_* counterpart. */
int32_t emdee_md_set_rdf(emdee_md *md, double r_max, int32_t n_bins, int32_t n_groups, const int32_t *group_dev,
                         const int32_t *molecule_dev);
int32_t emdee_md_rdf_sample(emdee_md *md);
int32_t emdee_md_rdf_read(emdee_md *md, int64_t *counts, int64_t group_sizes[8], int64_t *frames, double *inv_volume_sum);
int32_t emdee_md_rdf_reset(emdee_md *md);

/* Mean-squared displacement and velocity autocorrelation (build-defined: the reference has no analysis of the dynamics).  The
 * engine keeps a ring of snapshots of the grouped atoms -- unwrapped coordinates and velocities, as doubles -- in device memory and
 * correlates every sample with the origins still within reach, so that a diffusion coefficient (the Einstein slope of the MSD, the
 * Green-Kubo integral of the VACF) costs no copy of the state to the host and no bookkeeping of time origins there.
 *
 * emdee_md_set_msd(what, n_groups, group_dev, n_lags, origin_every) sets the table (blocking; n_lags = 0 clears it):
 *   what: a non-empty mask of EMDEE_MSD | EMDEE_VACF.  Without EMDEE_MSD no positions are stored and words 0-5 stay exactly 0;
 *   without EMDEE_VACF no velocities are stored and word 6 stays exactly 0.
 *   n_groups in 1...8.  group_dev: n_owned int32 in caller order on the device, each in -1...n_groups-1; -1 leaves the atom out;
 *   NULL with n_groups == 1 puts every atom in group 0.  The array is copied, the group sizes are counted; an empty group is legal.
 *   n_lags in 1...4096, origin_every >= 1; the ring holds n_origins = ceil(n_lags / origin_every) <= 64 snapshots and one more as
 *   scratch: (n_origins + 1) n_grouped 24 bytes (one of the two) or 48 bytes (both) of device memory.  Setting a table zeroes the sums.
 *   - All or nothing: EMDEE_ERR_INVALID, the previous table in force, for arguments outside these limits; for a group value out of
 *     range the text names the first offending atom.  A failed allocation (EMDEE_ERR_ALLOC) leaves the previous table in force too.
 *   - EMDEE_ERR_STATE, each with its own text: before emdee_md_set_state, on an integrator lent by emdee_dd_engine, on one with
 *     ghosts.  Open axes are fine: their image count is 0.
 *
 * emdee_md_msd_sample takes the current state as sample s = 0, 1, ... (counted from the last set or reset; what the interval
 * between two samples is, is the caller's: step(n); msd_sample()).  When s % origin_every == 0, sample s becomes an origin in ring
 * slot (s / origin_every) % n_origins.  Then, for every origin o taken at s_o <= s with lag l = s - s_o < n_lags (the one just
 * written included, l = 0) and every group g, with d_i = x_i(s) - x_i(s_o) on the unwrapped coordinates emdee_md_get_state returns,
 * seven words are added to sums[(l n_groups + g) 7 + w]:
 *   w = 0, 1, 2: sum_i d_ix^2, d_iy^2, d_iz^2;   w = 3, 4, 5: (sum_i d_ix)^2, (sum_i d_iy)^2, (sum_i d_iz)^2, the group's drift, squared
 *   per origin;   w = 6: sum_i v_i(s) . v_i(s_o).
 * With origins[l] the number of origins that have contributed to lag l: MSD(l) = (w0 + w1 + w2) / (origins N_g), the drift-free
 * MSD = (w0 + w1 + w2 - (w3 + w4 + w5) / N_g) / (origins N_g), VACF(l) = w6 / (origins N_g).  fp64 throughout in both precisions:
 * an fp64 engine's snapshot is bit for bit what emdee_md_get_state returns; a Float32 engine's is the record plus the origin of
 * its cell plus the box lengths removed, in double, unrounded.  Sums in a fixed order that depends on the table alone (chunks of
 * 1024 atoms of one group, never the device's CU count), no floating-point atomics: bitwise reproducible.  The work is queued on the
 * engine's stream, nothing is read back, and it writes only buffers of its own: an engine that samples and one that does not stay
 * bit for bit equal.  Its device time is emdee_md_kernel_time index 16.
 *   - EMDEE_ERR_STATE, nothing changed: no table is set; the table was set for another number of owned atoms; emdee_md_set_state
 *     has replaced the state since the last set or reset; the box lengths differ from those at the last set or reset
 *     (emdee_md_scale_box, a barostat): unwrapped coordinates across a rescaled box are not a displacement -- emdee_md_msd_reset
 *     starts again.
 * Sampling on a cadence inside emdee_md_step is not offered, as for the radial distribution functions.
 *
 * emdee_md_msd_read (blocking; any pointer may be NULL): the n_lags n_groups EMDEE_MSD_WORDS sums, origins[n_lags] and samples
 * (both kept on the host, functions of s alone) and the eight group sizes.  emdee_md_msd_reset zeroes the sums and origins,
 * restarts s at 0 and records the current box and state.
 * Scope: undivided boxes; no emdee_dd_* counterpart. */
#define EMDEE_MSD        1
#define EMDEE_VACF       2
#define EMDEE_MSD_WORDS  7
int32_t emdee_md_set_msd(emdee_md *md, int32_t what, int32_t n_groups, const int32_t *group_dev, int32_t n_lags,
                         int32_t origin_every);
int32_t emdee_md_msd_sample(emdee_md *md);
int32_t emdee_md_msd_read(emdee_md *md, double *sums, int64_t *origins, int64_t group_sizes[8], int64_t *samples);
int32_t emdee_md_msd_reset(emdee_md *md);

/* Green-Kubo observables: the autocorrelations of the stress and of the heat flux (build-defined: the reference has no analysis of
 * the dynamics).  The shear viscosity eta = V / (kT) int <P_ab(0) P_ab(t)> dt and the thermal conductivity
 * lambda = 1 / (V kT^2) int <J_a(0) J_a(t)> dt need 10^5 - 10^6 samples of the box stress and of the heat flux; the engine holds
 * everything both are made of -- the per-atom energies and virial tensors of the tensor pass, the full-step velocities, the
 * fixed-order box sums -- so a sample costs no read-back: nine fp64 words go to a ring on the device and a correlator adds their
 * products with the earlier samples to the lag sums.
 *
 * One sample = EMDEE_GK_WORDS = 9 words A_0 ... A_8, all energies (pressure x volume; no volume enters the sums):
 *   EMDEE_GK_STRESS, words 0-5: with S_ab = K_ab + W_ab from the twelve sums of emdee_md_pressure_tensor -- the same numbers from the
 *   same kernels, not read back -- A_0 = S_xy, A_1 = S_xz, A_2 = S_yz, A_3 = (S_xx - S_yy) / 2, A_4 = (S_yy - S_zz) / 2 (the five
 *   independent traceless components, for eta) and A_5 = (S_xx + S_yy + S_zz) / 3 = p V (for the bulk viscosity).  On an engine with
 *   a rigid table in force (emdee_md_set_rigid3) the twelve numbers of emdee_md_molecular_pressure_tensor take their place: the
 *   atomic tensor lacks the constraint virial, the molecular one is the valid stress.
 *   EMDEE_GK_HEAT, words 6-8: J = sum_i (k_i + e_i) v_i + sum_i W_i . v_i over the owned atoms, k_i = m_i v_i^2 / 2 (exactly 0 for
 *   inv_mass = 0), e_i and W_i the per-atom energy and symmetric virial tensor of the tensor pass (emdee_md_virial_tensor), v_i the
 *   velocities emdee_md_energies takes.  For pair forces this is the usual sum e_i v_i + 1/2 sum_{i != j} r_ij (f_ij . v_i).  The
 *   partial-enthalpy correction a mixture's thermal conductivity needs is not applied: J is the energy flux, which is the heat
 *   flux of a one-component fluid only.
 *   A mask bit that is off leaves its words exactly 0 and runs none of its kernels.
 *
 * emdee_md_set_gk(what, n_lags) sets the table (blocking; n_lags = 0 clears it): what is a non-empty mask of EMDEE_GK_STRESS |
 * EMDEE_GK_HEAT, n_lags in 1...65536.  The ring is n_lags x 9 doubles; setting a table zeroes the sums.
 *   - All or nothing, the previous table and its sums in force: EMDEE_ERR_INVALID for a mask outside 1...3 or n_lags outside
 *     0...65536; EMDEE_ERR_ALLOC for a failed allocation.
 *   - EMDEE_ERR_STATE, each with its own text: before emdee_md_set_state; on an integrator lent by emdee_dd_engine; on one with
 *     ghosts; with an hbonds table in force (emdee_md_set_hbonds), for any mask: neither stress holds the clusters' constraint virial.
 *   - EMDEE_ERR_STATE for EMDEE_GK_HEAT on an engine whose forces are not all pair terms of the neighbour rows -- exclusions, 1-4
 *     pairs, bonded terms, rigid molecules, virtual sites, Ewald summation or PME; the text names the setter of every one in the
 *     way.  Their per-atom
 *     tensors are not the half-pair split J is written for.  Lennard-Jones with or without reaction-field charges is accepted.
 *
 * emdee_md_gk_sample takes the current state as sample s = 0, 1, ... (counted from the last set or reset; what the interval between
 * two samples is, is the caller's: step(n); gk_sample()).  The forces (a rigid engine) and the tensor pass are evaluated first if
 * they are not current, as the pressure entries evaluate them.  A(s) goes to ring slot s % n_lags -- every sample is an origin --,
 * A_w(s) is added to totals[w], and for every lag l = 0 ... min(s, n_lags - 1) the product A_w(s) A_w(s - l) is added to
 * sums[l 9 + w].  The number of products behind lag l is max(0, samples - l).  Queued on the engine's stream, nothing read back; it
 * writes buffers of its own and the outputs of the tensor pass only: an engine that samples and one that does not stay bit for bit
 * equal.  Bitwise reproducible: the heat reduction has the shape of the box sums (a grid that depends on the atom count alone,
 * never on the device's CU count), one thread per lag owns its nine sums, no floating-point atomics.  The deferred fault word of
 * the bonded terms is checked in emdee_md_gk_read, not here.
 * Device time: emdee_md_kernel_time index 17 covers the launches a sample adds, not the tensor pass (index 0 counts that):
 * EMDEE_GK_STRESS alone 4 (the two of the box sums, the push, the correlator; 5 with a rigid table, whose molecule pass is index
 * 10's), EMDEE_GK_HEAT alone 4 (the heat partials, their finish, the push, the correlator), both 6.
 *   - EMDEE_ERR_STATE, nothing changed: no table is set; the conditions of emdee_md_set_gk no longer hold (a table attached
 *     since); the table was set for another number of owned atoms; and, until emdee_md_gk_reset: emdee_md_set_state has replaced
 *     the state since the last set or reset; the box lengths differ from those at the last set or reset (emdee_md_scale_box, a
 *     barostat): S and J are extensive and the Green-Kubo prefactor assumes one V.
 * Sampling on a cadence inside emdee_md_step is not offered, as for the radial distribution functions.
 *
 * emdee_md_gk_read (blocking; any pointer may be NULL): the n_lags x 9 sums, the nine totals, the most recent A (zeros before the
 * first sample) and samples.  emdee_md_gk_reset zeroes the sums, the totals and the ring, restarts s at 0 and records the current
 * box and state.
 * Scope: undivided engines; no emdee_dd_* counterpart.  No cross-correlations between words; the sums are not restartable. */
#define EMDEE_GK_STRESS  1
#define EMDEE_GK_HEAT    2
#define EMDEE_GK_WORDS   9
int32_t emdee_md_set_gk(emdee_md *md, int32_t what, int32_t n_lags);
int32_t emdee_md_gk_sample(emdee_md *md);
int32_t emdee_md_gk_read(emdee_md *md, double *sums, double totals[9], double last[9], int64_t *samples);
int32_t emdee_md_gk_reset(emdee_md *md);

/* Spatial profiles along an axis and around a centre (build-defined: the reference has no analysis).  What a slab, a droplet or a
 * box with vacuum in it is run for: the density profile across the interface, the normal and tangential pressure profiles and the
 * surface tension they integrate to, the temperature, flow and charge profiles, the radial profiles of a droplet.  The engine holds
 * every addend on the device -- positions and image counts, full-step velocities and inverse masses, the charges, the per-atom
 * energies and virial tensors of the tensor pass -- so a sample costs no copy of the state: ten fp64 words per (group, bin).
 *
 * emdee_md_set_spatial(geometry, what, n_bins, n_groups, group_dev, range, centre, centre_group) sets the table (blocking; n_bins = 0
 * clears it):
 *   geometry: EMDEE_SPATIAL_X, _Y, _Z: planar slabs normal to that axis, n = e_d.  On a periodic axis range must be NULL and the bins
 *   are fractions of the box, bin = floor((x_d - lo_d) n_bins / len_d) wrapped into 0...n_bins-1: they follow the box under a
 *   barostat.  On an open axis range = {r0, r1} is required, finite, r0 < r1, in absolute coordinates; an atom outside [r0, r1) adds 1
 *   to outside[group] and nothing else (atoms beyond the faces of an open axis are ordinary atoms here).
 *   EMDEE_SPATIAL_RADIAL: spherical shells, n = r / |r|, range = {0, r_max}, bin = (int)(r n_bins / r_max), r >= r_max is outside.
 *   r_max may be at most half the shortest PERIODIC side (a droplet box has none and no limit); distances are minimum-image on the
 *   periodic axes only.  The centre is centre[3] when centre_group = -1; otherwise the mass-weighted centre of the atoms of that
 *   group, formed on the device in fp64 at every sample from the unwrapped coordinates -- the group is loaded whole, as for
 *   emdee_md_set_pull -- with nothing read back; a centre group of total mass 0 is refused.  Its order is fixed so that a host
 *   can repeat it bit for bit from the coordinates emdee_md_get_state returns: per chunk of 1024 atoms of the group, ascending
 *   caller id, the products m x, m y, m z (each rounded on its own) and m go through a halving tree (s[i] += s[i + h], h = 512 ... 1,
 *   zeros beyond the count), the chunks' totals are added in chunk order, and R = (sum m x) / M.
 *   what: a non-empty mask.  sums[(g n_bins + k) EMDEE_SPATIAL_WORDS + w], all fp64:
 *     EMDEE_SPATIAL_DENSITY  w = 0: sum m;  1: sum q (0 on an engine without charges)
 *     EMDEE_SPATIAL_KINETIC  w = 2, 3, 4: sum m v_x, m v_y, m v_z;  5: sum m v^2;  6: sum m (v . n)^2
 *     EMDEE_SPATIAL_STRESS   w = 7: sum e_i;  8: sum tr W_i;  9: sum n . W_i . n
 *   m = 1 / (double)inv_mass, exactly 0 for inv_mass = 0 (a virtual site is binned where it sits, with mass 0); v the velocities
 *   emdee_md_energies takes; e_i and W_i the per-atom energies and tensors behind emdee_md_get_state and emdee_md_virial_tensor.  On
 *   the centre of the radial geometry n is undefined: words 6 and 9 take a third of words 5 and 8 there.  A bit that is off runs none
 *   of its loads and leaves its words exactly 0.  counts[g n_bins + k] (64-bit) is always kept.  With V_bin the bin's volume,
 *     P_N = (w6 + w9) / V_bin,   P_T = ((w5 - w6) + (w8 - w9)) / (2 V_bin).
 *   The per-atom split of the tensor pass is what is binned (the half-pair split, as the stress/atom profiles of other packages),
 *   not the Irving-Kirkwood contour.
 *   n_bins in 1...4096; n_groups and group_dev as emdee_md_set_msd takes them (1...8 groups, -1 leaves an atom out, NULL with one
 *   group takes every atom).  Setting a table zeroes the sums.
 *   - All or nothing, the previous table and its sums in force: EMDEE_ERR_INVALID for an argument outside these limits, a range on a
 *     periodic axis, no range on an open one, a number that is not finite, an r_max beyond half a periodic side, a centre_group outside
 *     -1...n_groups-1 or of mass 0; EMDEE_ERR_ALLOC for a failed allocation.
 *   - EMDEE_ERR_STATE, each with its own text: before emdee_md_set_state; on an integrator lent by emdee_dd_engine; on one with
 *     ghosts; EMDEE_SPATIAL_STRESS with a rigid or an hbonds table in force (emdee_md_set_rigid3, emdee_md_set_hbonds): the atomic
 *     tensors lack the constraint virial.  DENSITY and KINETIC are accepted there.  Bonded terms, exclusions, Ewald, PME, virtual
 *     sites, restraints, pull and alchemical tables all pass: the box sums of emdee_md_pressure_tensor are sums of these same planes.
 *
 * emdee_md_spatial_sample adds the current state to the sums: queued on the engine's stream, nothing read back.  With
 * EMDEE_SPATIAL_STRESS the tensor pass is evaluated first if it is not current, as emdee_md_gk_sample does; without it no pass of
 * the engine runs at all.  It writes buffers of its own and, with STRESS, the outputs of the tensor pass: an engine that samples and
 * one that does not stay bit for bit equal.  The host adds 1 to frames and, in the planar geometry, 1 / V_bin of the current box to
 * inv_bin_volume_sum (V_bin = the cross-section times len_d / n_bins, or times (r1 - r0) / n_bins; shell volumes do not depend on
 * the box: the radial geometry adds nothing).  A frame stands alone: neither a replaced state of the same size nor a rescaled box is
 * refused.  fp64 arithmetic from the planes as they are, in both precisions: an fp64 engine bins bit for bit the coordinates
 * emdee_md_get_state returns, a Float32 engine the record plus the origin of its cell plus the box lengths removed, in double,
 * unrounded.  The bin is one rule shared by host and device, every difference and product a rounding of its own.  Sums in a fixed
 * order that depends on the table alone (group-major, ascending caller id, chunks of 1024 atoms of one group; never the device's CU
 * count or the engine's cell order), no atomics: bitwise reproducible -- two engines given the same calls agree in every bit --
 * and a rebuild of the neighbour list between two samples of one state changes no bit of the counts and of the DENSITY and KINETIC
 * words.  The STRESS words read e_i and W_i, which the engine re-evaluates after a rebuild in the order of its new rows: those
 * inputs move in the last bit, and so may words 7-9.
 * Device time: emdee_md_kernel_time index 21 covers the sample's own launches, not the tensor pass (index 0 counts that): 3 for every
 * mask and every geometry (gather, accumulate, finish), 5 with a centre group (the chunks' partial sums and the centre of mass ahead
 * of them); none when no atom is grouped.
 *   - EMDEE_ERR_STATE, nothing changed: no table is set; the conditions of the set no longer hold (a rigid or hbonds table attached
 *     since); the table was set for another number of owned atoms; a barostat has put r_max beyond half a periodic side.
 * Sampling on a cadence inside emdee_md_step is not offered, as for the radial distribution functions.
 *
 * emdee_md_spatial_read (blocking; any pointer may be NULL): the n_groups n_bins counts, the n_groups n_bins EMDEE_SPATIAL_WORDS
 * sums, outside[8], the eight group sizes, frames and inv_bin_volume_sum; it checks the deferred fault word of the bonded terms.
 * emdee_md_spatial_reset zeroes the counts, the sums, outside, frames and inv_bin_volume_sum.
 * Scope: undivided engines; no emdee_dd_* counterpart.  No cylindrical shells, no off-diagonal stress profiles. */
#define EMDEE_SPATIAL_X        0
#define EMDEE_SPATIAL_Y        1
#define EMDEE_SPATIAL_Z        2
#define EMDEE_SPATIAL_RADIAL   3
#define EMDEE_SPATIAL_DENSITY  1
#define EMDEE_SPATIAL_KINETIC  2
#define EMDEE_SPATIAL_STRESS   4
#define EMDEE_SPATIAL_WORDS    10
int32_t emdee_md_set_spatial(emdee_md *md, int32_t geometry, int32_t what, int32_t n_bins, int32_t n_groups,
                             const int32_t *group_dev, const double range[2], const double centre[3], int32_t centre_group);
int32_t emdee_md_spatial_sample(emdee_md *md);
int32_t emdee_md_spatial_read(emdee_md *md, int64_t *counts, double *sums, int64_t outside[8], int64_t group_sizes[8],
                              int64_t *frames, double *inv_bin_volume_sum);
int32_t emdee_md_spatial_reset(emdee_md *md);

/* ---- position restraints: harmonic and flat-bottomed, scaled with the box (restraint.hpp)
 * An external field that ties the named atoms to reference points: the stage of an equilibration in which a solute is held near its
 * starting structure while the solvent relaxes, a slab pinned along one axis, a droplet kept off an open face.  With a table in force
 * the potential energy and the stress of the engine hold an EXTERNAL FIELD: emdee_md_energies, _pressure_tensor, _virial_tensor,
 * _get_state, the barostats and the Green-Kubo stress take the term with the rest, momentum is no longer conserved and the pressure
 * is that of the atoms in the field.
 * emdee_md_set_restraints (blocking, the device arrays are copied; n = 0 clears the table):
 *   atoms_dev  n caller ids.
 *   ref_dev    3 n doubles in the coordinates emdee_md_get_state returns: the caller's image, unwrapped; a reference may lie outside the
 *              box.  NULL: every named atom's current position (d = 0 exactly, in both precisions).
 *   k_dev      3 n doubles, the spring constants per axis, each finite and >= 0.
 *   flat_dev   n doubles, the flat-bottom radius r0 >= 0.  NULL: all zero.
 * The term of one atom: d = x_unwrapped - ref, formed in fp64 in both precisions from the record and the per-axis image count (a Float32
 * engine adds its cell origin in double); no minimum image, so an atom that walks through a box face or is re-sorted by a rebuild sees
 * a continuous force.  r0 = 0: U = 1/2 sum_a k_a d_a^2, f_a = -k_a d_a.  r0 > 0: the non-zero constants of the entry are one value k,
 * rho is the norm of d over the axes with k_a > 0 (the well is a sphere, a cylinder or a slab), U = 1/2 k max(0, rho - r0)^2, the force
 * points along the masked d and is exactly 0 inside the well.  The atom owns the whole term: its energy plane gets U, its virial plane
 * d . f, its tensor the symmetrised d (x) f in the component order of emdee_compute_virial_tensor, its force plane f, each only when the
 * pass's mask asks for it.  No atomics: bitwise reproducible.
 * The references follow the box: emdee_md_scale_box and every barostat event map ref <- lo + mu (ref - lo) per axis (GROMACS's
 * refcoord_scaling = all), so that with atom-by-atom scaling d -> mu d and tr W_restr = -dU_restr/dmu; with molecular scaling the
 * molecular virial holds the restraint force with the others.
 * With a table the engine steps in the split form, never the fused one: kick + drift, the force pass with the restraint launch behind
 * it, kick.  Every step closes its own half kick, as the steps of an engine with constraints, a barostat or a thermostat do, so the
 * state after s steps does not depend on how the s steps were dealt to calls: step(40), 8 x step(5) and 40 x step(1) agree bit for
 * bit.  emdee_md_minimize needs nothing new.  An engine without a table is bit for bit and launch for
 * launch what it was.  On success the forces are evaluated again: planes and table belong together on return.
 * Degrees of freedom: the library's own count (emdee_md_set_thermostat with n_dof = 0) still subtracts 3 for the centre of mass, which a
 * restrained system does not conserve; a caller who restrains atoms may pass n_dof explicitly.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous table in force: a NULL atoms_dev or k_dev with n > 0; n < 0; an id outside
 *     [0, n_owned); an atom named twice; a constant or radius that is not finite and >= 0; a reference that is not finite; r0 > 0 with
 *     unequal non-zero constants, or with no non-zero constant.  The text names the entry.
 *   - EMDEE_ERR_STATE, the previous table in force: a call before emdee_md_set_state; ghosts; an integrator lent by emdee_dd_engine; an
 *     entry that is a virtual site of the table in force (and emdee_md_set_vsites refuses a site that this table names); a state loaded
 *     without velocities.
 *   - The table survives an emdee_md_set_state with the same atom count, references kept.  After a state with another count
 *     emdee_md_step, emdee_md_minimize, emdee_md_scale_box and the reads refuse (EMDEE_ERR_STATE) until the table is set again or cleared.
 *   - The Green-Kubo heat flux (EMDEE_GK_HEAT) is refused with a restraint table, at set and at sample.
 * emdee_md_restraint_sums (blocking): out[0] = sum U, out[1..6] = the sum of the tensors (xx, yy, zz, xy, xz, yz), out[7] = the largest
 * |d| (all three axes) over the table; fp64 in a fixed order that depends on n alone.  All zero without a table.
 * emdee_md_get_restraint_refs: the references as they now stand (after an NPT stage, for a restart), 3 n doubles in table order to
 * ref_dev, queued on the context's stream; nothing is written without a table.
 * Device time: emdee_md_kernel_time index 18.
 * Scope: undivided engines; no emdee_dd_* counterpart.  No restraints on centres of mass, no distance or dihedral restraints, no
 * time-dependent references. */
#define EMDEE_RESTRAINT_WORDS 8
int32_t emdee_md_set_restraints(emdee_md *md, const int32_t *atoms_dev, const double *ref_dev, const double *k_dev,
                                const double *flat_dev, int32_t n);
int32_t emdee_md_restraint_sums(emdee_md *md, double out[EMDEE_RESTRAINT_WORDS]);
int32_t emdee_md_get_restraint_refs(emdee_md *md, double *ref_dev);

/* ---- centre-of-mass pulling between atom groups (pull.hpp)
 * A bias along a collective coordinate: a harmonic (umbrella) or constant force between the centres of mass of two groups of atoms --
 * umbrella sampling of a potential of mean force, steered MD, pulling a molecule through a slab, holding two solutes at a distance.
 * As with the restraints, the potential energy and the stress of the engine then hold the bias: emdee_md_energies, the pressure entries,
 * the molecular sums, the barostats, the Green-Kubo stress and emdee_md_minimize take the term with the rest.
 * emdee_md_set_pull (blocking; n_coords = 0 clears the table):
 *   group_dev     n_owned int32 on the device, -1 ... n_groups - 1 by caller id, as emdee_md_set_msd takes them; -1 leaves an atom out.
 *                 Every group in use is non-empty; the caller loads each group whole (no minimum image is taken anywhere).
 *   n_groups      1 ... 8.
 *   coords        HOST, n_coords x 5 int32: {a, b, kind, geometry, mask}.  a != b are groups; kind is EMDEE_PULL_UMBRELLA or
 *                 EMDEE_PULL_CONSTANT_FORCE; geometry EMDEE_PULL_DISTANCE or EMDEE_PULL_DIRECTION; mask (distance only) keeps axis a
 *                 where bit a is set, 1 ... 7.
 *   params        HOST, n_coords x 6 doubles: {k or F, r0, rate, nx, ny, nz}.  n (direction only) is normalised by the library.
 *   n_coords      1 ... 8.
 *   log_every, log_capacity   the on-device log (below); log_capacity = 0: none.
 * The coordinate.  M_g = sum m_i and R_g = sum m_i x_i / M_g over group g, with m_i = 1 / inv_mass (1 where the engine has no masses)
 * and x_i the UNWRAPPED coordinates emdee_md_get_state returns, formed in fp64 in both precisions from the record, the image count and,
 * for Float32, the cell origin: a group that diffuses through a box face or is re-sorted by a rebuild feels a continuous force.
 * D = R_b - R_a.  EMDEE_PULL_DISTANCE: xi = |m o D|, dxi/dD = m o D / xi.  EMDEE_PULL_DIRECTION: xi = n . D, signed, dxi/dD = n.
 * EMDEE_PULL_UMBRELLA: U = 1/2 k (xi - xi0)^2 with xi0 starting at r0; every completed step of length dt of emdee_md_step advances
 * xi0 by rate dt -- one fp64 addition per step on the host, so the sequence does not depend on how the steps are dealt to calls
 * (emdee_md_minimize leaves xi0 alone).  EMDEE_PULL_CONSTANT_FORCE: U = -F xi; rate must be 0.  With f = -dU/dxi the force on group b
 * is F_b = f dxi/dD, on group a -F_b.  At xi = 0 in the distance geometry the force is zero and U finite; no division happens.
 * An umbrella coordinate accumulates the work of its moving reference on the device by the RECTANGLE RULE: at the force pass that
 * closes a step, after xi0 has advanced, work += f rate dt with f at the new xi and xi0.
 * xi0 and r0 DO NOT SCALE WITH THE BOX: emdee_md_scale_box and the barostats leave them as they are.
 * Where the term goes.  Everything is mass-weighted, so a group accelerates as one body: atom i of group g gets the force m_i A_g with
 * A_g the sum over the coordinates that name g of (+-F_c) / M_g; its energy plane gets m_i / M_g 1/2 U_c per coordinate, its virial
 * and tensor planes m_i / M_g 1/2 sym(D_c (x) F_b,c), each only when the pass's mask asks for it.  The box sums then hold exactly U_c and
 * sym(D_c (x) F_b,c), and the per-atom values are translation invariant.  Three launches behind every force pass, no atomics, no order
 * of summation that depends on the device: bitwise reproducible.  An engine with a table steps in closed steps, as a restrained one
 * does; an engine without one is launch for launch and bit for bit what it was.  On success the forces are evaluated again.
 * emdee_md_pull_read (blocking, one copy, no launch): what the last force pass wrote.  coords_out: n_coords x EMDEE_PULL_WORDS doubles
 * {xi, xi0, f, U, work, Dx, Dy, Dz}; groups_out: n_groups x 4 doubles {X, Y, Z, M}.  Either may be NULL.
 * emdee_md_pull_log_read: the log takes entry j, {xi, f} per coordinate, at the pass that closes step (j + 1) log_every counted from the
 * set; when it is full, further samples are dropped and counted.  The entries so far go to log_dev (device, capacity x n_coords x 2
 * doubles, queued on the context's stream; may be NULL), their number to *count, the dropped samples to *dropped.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous table in force: n_groups or n_coords outside 1 ... 8; a group id outside
 *     -1 ... n_groups - 1; an empty group; a = b or a group outside the table; an unknown kind or geometry; a mask of 0 (or above 7) for
 *     a distance; a zero or non-finite direction; a parameter that is not finite; k < 0; rate != 0 with a constant force; a NULL array;
 *     a negative log_every or log_capacity, or a log without log_every >= 1.  The text names the entry and the value.
 *   - EMDEE_ERR_STATE, the previous table in force: a call before emdee_md_set_state; ghosts; an integrator lent by emdee_dd_engine; a
 *     grouped atom that is a virtual site of the table in force (it has no mass; emdee_md_set_vsites refuses the mirror case); a state
 *     loaded without velocities.  A force pass on the operator path refuses with a table.
 *   - The table survives an emdee_md_set_state with the same atom count.  After a state with another count emdee_md_step,
 *     emdee_md_minimize, emdee_md_scale_box and the reads refuse (EMDEE_ERR_STATE) until the table is set again or cleared.
 *   - The Green-Kubo heat flux (EMDEE_GK_HEAT) is refused with a pull table, at set and at sample.
 * Device time: emdee_md_kernel_time index 19.
 * Scope: undivided engines.  Follow-ups, not here: a fixed point in space as one end of a coordinate; angle and dihedral coordinates;
 * flat-bottomed biases; decomposed engines. */
#define EMDEE_PULL_WORDS           8
#define EMDEE_PULL_UMBRELLA        1
#define EMDEE_PULL_CONSTANT_FORCE  2
#define EMDEE_PULL_DISTANCE        1
#define EMDEE_PULL_DIRECTION       2
int32_t emdee_md_set_pull(emdee_md *md, const int32_t *group_dev, int32_t n_groups, const int32_t *coords, const double *params,
                          int32_t n_coords, int32_t log_every, int32_t log_capacity);
int32_t emdee_md_pull_read(emdee_md *md, double *coords_out, double *groups_out);
int32_t emdee_md_pull_log_read(emdee_md *md, double *log_dev, int64_t *count, int64_t *dropped);

/* ---- soft-core alchemical decoupling (alchemical.hpp)
 * The Lennard-Jones stage of a solvation free energy: the coupling of one group of atoms, the solute, to everything else is turned
 * off along lambda through a soft core.  (The Coulomb stage of a reaction-field engine is emdee_md_set_alchemical_coulomb, below.)
 * Every pair of one flagged and one unflagged atom inside the cutoff interacts by
 *     u = (r^2 / sigma_ij^2)^3,  D = alpha (1 - lambda) + u,  U(r; lambda) = lambda 4 eps_ij (D^-2 - D^-1) g(r)
 * -- Beutler et al. 1994 with lambda-power 1 and r-power 6 (GROMACS sc-power = 1, sc-r-power = 6); sigma_ij and 4 eps_ij from the
 * atoms' own records, g the model's switch, r^2 < rc^2 the test of every pair loop.  Flagged-flagged and unflagged-unflagged pairs
 * stay in the neighbour rows at full strength: DECOUPLING, NOT ANNIHILATION.  At lambda = 1 the term is the model's pair function, at
 * lambda = 0 exactly 0; at r = 0 with lambda < 1 and alpha > 0 it is finite and exerts no force; alpha = 0 is plain linear scaling,
 * which diverges at overlap.
 * emdee_md_set_alchemical (blocking; flag_dev = NULL clears the table):
 *   flag_dev      n_owned int32 on the device by caller id: 1 for a solute atom, 0 for the environment; at least one 1.
 *   lambda        in [0, 1]; emdee_md_set_lambda moves it later.
 *   alpha         the soft-core parameter, finite and >= 0 (0.5 is the usual choice).
 *   foreign       HOST, n_foreign doubles in [0, 1]: the lambdas U_alch is also evaluated at for BAR and MBAR; n_foreign 0 ... 16.
 *   log_every, log_capacity   the on-device log (below); log_capacity = 0: none.
 * How it runs.  Right after every list build the cross entries leave the rows of the owned atoms (after the exclusion filter: an
 * excluded cross pair stays excluded) and their slots go to a compact CSR of the build, memory O(struck entries).  Behind every force
 * pass one launch runs over the atoms that own struck entries -- a wavefront per solute atom, a thread per environment atom, half of a
 * pair's E and W to the owner, no atomics -- and adds to the force, energy, virial and tensor planes under the pass's mask, so that
 * emdee_md_minimize, emdee_md_energies, the pressure entries, the molecular sums, the barostats and the Green-Kubo stress see the
 * term with the rest.  The same pass leaves U_alch, dU/dlambda, the cross pairs' scalar virial and the number of cross pairs inside
 * rc on the device: fp64 sums in an order that depends on the state alone, bitwise reproducible.  An engine with a table steps in
 * closed steps, as a restrained or pulled one does; an engine without one is launch for launch and bit for bit what it was.  A
 * two-species box with a table runs on the general-species kernels.  Setting or clearing the table rebuilds the list and evaluates
 * the forces again.
 * emdee_md_set_lambda: lambda in [0, 1], a host scalar handed to the kernels as an argument -- no rebuild; the next step or query
 * evaluates the forces anew.  For slow growth and lambda schedules.
 * emdee_md_alchemical_read (blocking): words[0 .. EMDEE_ALCH_WORDS) = {lambda, U_alch, dU/dlambda, the cross virial, the cross pairs
 * inside rc} of the current positions, then the n_foreign energies U_alch(foreign[k]) at the same positions (one energies-only launch).
 * emdee_md_alchemical_log_read: the log takes entry j, {dU/dlambda, U_alch, the n_foreign foreign energies}, at the pass that closes
 * step (j + 1) log_every counted from the set; when it is full, further samples are dropped and counted.  The entries so far go to
 * log_dev (device, capacity x (2 + n_foreign) doubles, queued on the context's stream; may be NULL), their number to *count, the
 * dropped samples to *dropped.  The foreign energies are evaluated at log events and by the read only, never in a plain force pass.
 *   - All or nothing.  EMDEE_ERR_INVALID, the previous table in force: a flag that is neither 0 nor 1; no flagged atom; lambda or a
 *     foreign lambda outside [0, 1]; alpha negative or not finite; n_foreign outside 0 ... 16 or a NULL array with n_foreign > 0; a
 *     negative log_every or log_capacity, or a log without log_every >= 1.  The text names the entry and the value.
 *   - EMDEE_ERR_STATE, the previous table in force: a call before emdee_md_set_state; ghosts; an integrator lent by emdee_dd_engine.
 *     The reads and emdee_md_set_lambda refuse without a table.  A force pass on the operator path refuses with a table.
 *   - On a charged engine without the Coulomb stage (below) every flagged atom must carry charge 0: otherwise emdee_md_step and
 *     emdee_md_minimize refuse (EMDEE_ERR_STATE), naming the first such atom.  With zero charges the reaction field, Ewald and PME
 *     need nothing.
 *   - Flagged atoms may be atoms of rigid molecules, of hbonds clusters, or virtual sites: the flag says nothing about constraints.
 *   - The table survives an emdee_md_set_state with the same atom count.  After a state with another count emdee_md_step,
 *     emdee_md_minimize, emdee_md_scale_box and the reads refuse (EMDEE_ERR_STATE) until the table is set again or cleared.
 *   - The Green-Kubo heat flux (EMDEE_GK_HEAT) is refused with an alchemical table, at set and at sample.
 * Device time: emdee_md_kernel_time index 20 (the row pass at a rebuild and the launches behind a force pass).
 * Scope: undivided engines.  Follow-ups, not here: a Coulomb soft core under Ewald or PME (the solute's and the environment's structure
 * factors or charge meshes kept apart); more than one group, each with its own lambda; annihilation of the solute's internal pairs;
 * decomposed runs; a per-pair soft-core length.
 *
 * ---- the Coulomb stage (reaction-field engines)
 * emdee_md_set_alchemical_coulomb turns the charge term of the same cross pairs -- one flagged, one unflagged atom, the entries of the
 * table's CSR with r^2 < rc^2 -- into AMBER's soft-core Coulomb (Steinbrecher, Joung & Case 2011) on the reaction field of
 * emdee_md_set_coulomb.  With qq = K q_i q_j and the engine's k_rf and c_rf (k_rf = (eps_rf - 1) / ((2 eps_rf + 1) rc^3),
 * c_rf = 1 / rc + k_rf rc^2):
 *     rho2 = r^2 + beta (1 - lambda_q),  phi = 1 / rho + k_rf rho2 - c_rf,  wl = 1 / rho^3 - 2 k_rf
 *     U_q = lambda_q qq phi,  force = lambda_q qq wl d,  W_q = lambda_q qq wl r^2 = -r dU_q/dr,
 *     dU_q/dlambda_q = qq (phi + lambda_q (beta / 2) wl)
 * The solute's internal pairs keep their full charges: DECOUPLING, NOT ANNIHILATION (scaling the solute's charges with
 * emdee_md_set_coulomb would scale those too, and yields neither dU/dlambda nor foreign energies).  At lambda_q = 0 U_q, W_q and the force
 * are exactly 0 (dU_q/dlambda_q is not); at beta (1 - lambda_q) = 0 the term is lambda_q times the model's own reaction-field pair; at
 * r = 0 with beta (1 - lambda_q) > 0 everything is finite and the force is 0.  The cutoff is the strict test r^2 < rc^2 of every pair
 * loop: for beta (1 - lambda_q) > 0 U_q(rc) is not 0 (phi vanishes at rho = rc), a jump of the energy at the cutoff that GROMACS's
 * soft-core reaction field has as well.  1-4 and excluded cross pairs are struck before the alchemical pass and keep their treatment.
 *   enable        0 clears the stage (the other arguments are not looked at); a new emdee_md_set_alchemical, set or clear, clears it too.
 *   lambda_q      in [0, 1]; emdee_md_set_lambda_coulomb moves it later (a host scalar: no rebuild).
 *   beta          the soft-core length squared, in the caller's units of length^2, finite and >= 0.
 *   foreign_q     HOST, n_foreign doubles in [0, 1]; n_foreign must equal the table's: the k-th foreign state is the pair
 *                 (foreign[k], foreign_q[k]).  May be NULL with n_foreign = 0.
 * Opt-in: without the call an engine is launch for launch and bit for bit what it was, the refusal of a charged flagged atom included.
 * With it, and with charges, the launch behind every force pass takes its Coulomb instance: the charge term is formed beside the
 * Lennard-Jones one on the same entries, (wr2_lj + wr2_q) d goes to the force, U_q and W_q to the energy, virial and tensor planes; the
 * sums of U_q, dU_q/dlambda_q and W_q stay on the device, fixed order, no atomics, bitwise reproducible.  emdee_md_alchemical_read and
 * emdee_md_alchemical_log_read keep their layout and meaning: the Lennard-Jones words alone.
 * emdee_md_alchemical_coulomb_read (blocking): words[0 .. EMDEE_ALCH_COULOMB_WORDS) = {lambda_q, U_q, dU_q/dlambda_q, W_q (the cross
 * Coulomb virial)} of the current positions, then U_q at the n_foreign foreign_q (the energies-only launch).
 * emdee_md_alchemical_coulomb_log_read: a second on-device log of {dU_q/dlambda_q, U_q, the n_foreign foreign U_q} per entry, on the
 * table's own log_every and log_capacity; its entry j is taken at the same pass as entry j of the table's log, and count and dropped
 * are the same.  Setting the stage restarts the table's step count and both logs.
 *   - All or nothing; the previous stage stays in force; the text names the value.  EMDEE_ERR_INVALID: lambda_q or a foreign lambda_q
 *     outside [0, 1] or NaN; beta negative or not finite; n_foreign different from the table's, or a NULL array with n_foreign > 0.
 *   - EMDEE_ERR_STATE: no alchemical table; no charges (emdee_md_set_coulomb); ghosts; an integrator lent by emdee_dd_engine.  The
 *     reads and emdee_md_set_lambda_coulomb refuse without the stage.
 *   - Under emdee_md_set_ewald or emdee_md_set_pme a charged flagged atom is refused (EMDEE_ERR_STATE) with the stage on as with the
 *     stage off -- at the set and at the readiness check of emdee_md_step and emdee_md_minimize, whichever comes later; the text names
 *     the atom, this setter and the Ewald or PME setter.  With zero solute charges Ewald and PME keep working.
 *   - Clearing the charges (emdee_md_set_coulomb with n = 0) leaves the stage set but inert: U_q, dU_q/dlambda_q and W_q read 0. */
#define EMDEE_ALCH_WORDS           5
#define EMDEE_ALCH_MAX_FOREIGN     16
#define EMDEE_ALCH_COULOMB_WORDS   4    /* lambda_q, U_q, dU/dlambda_q, W_q (the cross Coulomb virial) */
int32_t emdee_md_set_alchemical(emdee_md *md, const int32_t *flag_dev, double lambda, double alpha, const double *foreign,
                                int32_t n_foreign, int32_t log_every, int32_t log_capacity);
int32_t emdee_md_set_lambda(emdee_md *md, double lambda);
int32_t emdee_md_alchemical_read(emdee_md *md, double *words);
int32_t emdee_md_alchemical_log_read(emdee_md *md, double *log_dev, int64_t *count, int64_t *dropped);
int32_t emdee_md_set_alchemical_coulomb(emdee_md *md, int32_t enable, double lambda_q, double beta, const double *foreign_q,
                                        int32_t n_foreign);
int32_t emdee_md_set_lambda_coulomb(emdee_md *md, double lambda_q);
int32_t emdee_md_alchemical_coulomb_read(emdee_md *md, double *words);
int32_t emdee_md_alchemical_coulomb_log_read(emdee_md *md, double *log_dev, int64_t *count, int64_t *dropped);

/* ---------------------------------------------------------------- domain decomposition (multi-GPU)
 * Build-defined (the reference is single-GPU; SURVEY.md 8(b) table rows emdee_dd_create / emdee_dd_step, 8(e)).
 * The periodic box [0, len_d) is cut into grid[0] x grid[1] x grid[2] bricks (at most 3 per dimension), domain
 * rank = cx + grid[0] (cy + grid[1] cz).  One emdee_dd drives the domains rank_first .. rank_first + n_local - 1:
 *   - one process per GPU: n_local = 1 and unique_id = the 128 bytes of emdee_dd_unique_id() as generated by ONE
 *     process and distributed by the caller (Julia Distributed / MPI / torch.distributed); the halo messages then
 *     travel over RCCL (ncclSend/ncclRecv over xGMI), resolved from librccl.so.1 at run time;
 *   - n_local = the whole grid, unique_id = NULL: every domain in this process on the context's device, messages
 *     as device-to-device copies (validation of a decomposition on a one-GPU box).
 * A step is, per domain, pack -> halo exchange on a communication stream || force + kick + drift of the interior
 * bricks -> unpack -> the boundary bricks; the steps of a call are queued a few at a time with device-side guard
 * words (the rebuild request rides on the halo messages), one host read-back per batch.  Rebuild = migration of
 * the atoms that left their brick + new ghost lists + re-sort + neighbour list.  Trajectories are those of the
 * undivided box to rounding. */
int32_t emdee_dd_unique_id(uint8_t out[128]);
/* Diagnostic: resolve librccl, build a ONE-rank communicator on the context's device and push n_bytes through
 * ncclSend/ncclRecv to itself (one group, a stream of its own) and 3 doubles through ncclAllReduce; fails unless the
 * bytes arrive unchanged.  Exercises the run-time binding (symbols, enum values, ncclUniqueId by value) on a one-GPU box. */
int32_t emdee_dd_rccl_selftest(emdee_ctx *ctx, int32_t n_bytes);
/* Host-only (no device needed): the geometry domain `rank` of the grid works with -- its neighbour directions in the
 * library's fixed order (x fastest; only cut dimensions move), the rank behind each direction and the periodic shift a
 * ghost sent that way carries, the distinct peer ranks (ascending), and the local box handed to the integrator (brick
 * plus a halo of width `halo` along cut dimensions, the whole period otherwise).  Arrays sized for 26 directions. */
int32_t emdee_dd_describe(const double len[3], const int32_t grid[3], double halo, int32_t rank, int32_t *ndirs,
                          int32_t dirs[78], int32_t dir_rank[26], double dir_shift[78], int32_t *npeers, int32_t peers[26],
                          double local_lo[3], double local_len[3], int32_t periodic[3]);
int32_t emdee_dd_create(emdee_ctx *ctx, const double len[3], const int32_t grid[3], int32_t rank_first, int32_t n_local,
                        const uint8_t *unique_id, emdee_lj_model model, double skin, int32_t precision, emdee_dd **out);
int32_t emdee_dd_destroy(emdee_dd *dd);
/* Atoms initially held by local domain `local` (any atoms of the box, anywhere: emdee_dd_load hands each to the brick
 * that contains it).  Device arrays in caller order: positions, velocities 3 x n reals; atoms n; gids n global ids
 * (they key the Langevin noise and identify atoms in emdee_dd_get_state).  Copied. */
int32_t emdee_dd_set_atoms(emdee_dd *dd, int32_t local, int32_t n, const void *positions_dev, const void *velocities_dev,
                           const emdee_lj_atom *atoms_dev, const int64_t *gids_dev);
/* Collective over all domains: migrate, select and exchange ghosts, bin/sort/list, forces. */
int32_t emdee_dd_load(emdee_dd *dd);
/* nsteps velocity-Verlet steps of the whole box (collective).  rebuild_every as in emdee_md_step. */
int32_t emdee_dd_step(emdee_dd *dd, int32_t nsteps, double dt, int32_t rebuild_every);
/* global {potential, kinetic, virial} sums (collective, blocking) */
int32_t emdee_dd_energies(emdee_dd *dd, double out[3]);
/* global emdee_md_pressure_tensor sums over all domains and ranks (collective like emdee_dd_energies, blocking);
 * EMDEE_ERR_STATE before emdee_dd_load */
int32_t emdee_dd_pressure_tensor(emdee_dd *dd, double out[12]);
/* atoms in the whole box / owned and ghost atoms of a local domain */
int32_t emdee_dd_counts(emdee_dd *dd, int32_t local, int64_t *n_global, int32_t *n_owned, int32_t *n_ghost);
/* owned atoms of a local domain: global ids and positions (wrapped into the global box at the last rebuild),
 * velocities, forces; n_owned entries each, any pointer may be NULL.  Blocking. */
int32_t emdee_dd_get_state(emdee_dd *dd, int32_t local, int64_t *gids_dev, void *positions_dev, void *velocities_dev,
                           void *forces_dev);
/* the integrator of a local domain, for the emdee_md_* queries (profile, kernel_time, nbr_stats, count_pairs);
 * borrowed: valid until emdee_dd_destroy, not to be stepped or destroyed by the caller */
int32_t emdee_dd_engine(emdee_dd *dd, int32_t local, emdee_md **out);
int32_t emdee_dd_set_langevin(emdee_dd *dd, double gamma, double temperature, uint64_t seed, uint64_t first_step);
/* out[0] = rebuilds, out[1] = batches of queued steps, out[2] = queued steps cancelled by a rebuild request,
 * out[3] = atoms that changed owner (this process) */
int32_t emdee_dd_stats(emdee_dd *dd, int64_t out[4]);
/* How the rebuilds of this process went: out[0] = rebuilds whose migrant and ghost rows travelled in capacity-padded
 * messages with no count exchange (one read-back), out[1] = of those, the ones redone with exact counts because a
 * capacity was exceeded on some rank, out[2] = migrant rows a message holds per peer, out[3] = ghost rows the messages
 * of local domain 0 hold in all (send side). */
int32_t emdee_dd_rebuild_stats(emdee_dd *dd, int64_t out[4]);
/* Where the host-side time of this process's decomposition goes, cumulative since emdee_dd_create (take differences
 * around a timed region): out[0] = wall-clock ms inside rebuilds (ownership path, exchanges, read-backs, the engines'
 * sort + list), out[1] = rebuilds (the load included), out[2] = wall-clock ms of blocking read-backs of device words,
 * out[3] = read-backs, out[4] = ghost share n_ghost / (n_owned + n_ghost) of local domain 0 as of now, out[5] = the read-backs
 * among out[3] that happened INSIDE rebuilds (a rebuild in the engines' own order has one, with the build's words; the read-back
 * of a batch's request words that asked for it is not among them), out[6] = rebuilds done in the engines' own order, out[7] =
 * engines loaded again for room (a local matter: the state outgrew the slots its last load left).
 * The device-side phases of a step are emdee_md_kernel_time of emdee_dd_engine: 5 = fused step launches over interior
 * bricks (or all bricks, in-order form), 6 = over boundary bricks, 7 = halo (pack -> exchange -> unpack), 2 = sort + list. */
int32_t emdee_dd_phase_times(emdee_dd *dd, double out[8]);
/* How a step meets its halo exchange.  1 (default): interior bricks while the messages travel on a communication stream,
 * boundary bricks on a stream of their own when they have arrived.  0: pack, exchange, unpack and ONE launch over all
 * bricks, in order on the compute stream -- no events, no split launch; cheaper when the messages are short next to the
 * cross-stream bookkeeping (small domains).  Same results either way; collective (all ranks must choose alike only for
 * speed, not for correctness).  Call between emdee_dd_step calls. */
int32_t emdee_dd_set_overlap(emdee_dd *dd, int32_t overlap);
/* Exclusions and 1-4 pairs of a decomposed run.  pairs_dev: n_pairs pairs {g, h} of GLOBAL ids (the gids of
 * emdee_dd_set_atoms), 2 n_pairs int64, device; copied.  Semantics as emdee_md_set_exclusions / emdee_md_set_pairs14: an
 * excluded pair contributes nothing, a 1-4 pair contributes lj14scale times its pair terms (forces, energy and virial halves),
 * CUTOFF semantics as the list kernels.  Each call replaces its own table; n_pairs = 0 clears it.
 *   - Collective: every process passes the whole table, all the same one; the domains of a process share one copy.
 *   - Before emdee_dd_load, or between emdee_dd_step calls: after a load the call rebuilds every domain (rows, 1-4 slots,
 *     forces), and on return the forces are current and follow the new tables.
 *   - All or nothing: each pair needs g != h and 0 <= g, h < 2^31, else EMDEE_ERR_INVALID and the previous tables stay in
 *     force.  A pair naming a gid no domain holds is legal and contributes nothing.
 * A domain with a 1-4 table steps in the split form (force pass behind the halo, 1-4 terms, kick + drift) under the same guard
 * words as the fused step; one with exclusions only keeps the fused, overlapped step.  Boxes with a table keep the
 * general-species kernels.  emdee_md_set_exclusions / _set_pairs14 on an integrator of emdee_dd_engine return EMDEE_ERR_STATE. */
int32_t emdee_dd_set_exclusions(emdee_dd *dd, const int64_t *pairs_dev, int64_t n_pairs);
int32_t emdee_dd_set_pairs14(emdee_dd *dd, const int64_t *pairs_dev, int64_t n_pairs, double lj14scale);
/* Bonded terms of a decomposed run over GLOBAL ids (int64, 2, 3 or 4 per term): see emdee_md_set_bonded.  Collective; the
 * domains of a process share one copy; a missing partner is reported on every rank (EMDEE_ERR_STATE), and every rank then
 * refuses emdee_dd_step until the tables or the state are replaced. */
int32_t emdee_dd_set_bonded(emdee_dd *dd, int32_t kind, const int64_t *atoms_dev, const double *params_dev, int64_t n_terms);
/* Charges of a decomposed run (see emdee_md_set_coulomb): a table indexed by GLOBAL id, n_ids entries.  Collective, before
 * emdee_dd_load or between steps (after a load it rebuilds every domain, as emdee_dd_set_bonded); the domains of a process share
 * one device copy; n_ids = 0 clears it.  A domain atom whose gid is >= n_ids is an error, never a zero charge: EMDEE_ERR_STATE
 * on every rank (from this call or from emdee_dd_load), and every rank then refuses emdee_dd_step until the charges are set
 * again. */
int32_t emdee_dd_set_coulomb(emdee_dd *dd, const double *charges_dev, int64_t n_ids, double coulomb_k, double eps_rf,
                             double coulomb14scale);

#ifdef __cplusplus
}
#endif
#endif /* EMDEE_HIP_H */
