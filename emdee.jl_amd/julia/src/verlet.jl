# verlet.jl -- velocity-Verlet on the device.  Build-defined: the reference has no integrator
# (SURVEY.md 8a row a16).  API in EmDee's style: a constructor and `!` mutators.
export VelocityVerlet, step!, energies, set_langevin!, set_langevin_ids!, virial_tensor!, pressure_tensor
export box, scale_box!, set_barostat!
export set_thermostat!, thermostat_state, set_thermostat_state!, thermostat_draws
export set_rdf!, rdf_sample!, rdf_reset!, rdf_read
export set_msd!, msd_sample!, msd_reset!, msd_read
export set_gk!, gk_sample!, gk_reset!, gk_read
export set_spatial!, spatial_sample!, spatial_reset!, spatial_read
export set_restraints!, restraint_sums, restraint_refs!
export set_pull!, pull_read, pull_log_read!
export set_alchemical!, set_lambda!, alchemical_read, alchemical_log_read!
export set_alchemical_coulomb!, set_lambda_coulomb!, alchemical_coulomb_read, alchemical_coulomb_log_read!

mutable struct VelocityVerlet{T}
    handle::Ptr{Cvoid}
    N::Int
end

# int32_t emdee_md_create(emdee_ctx*, const double lo[3], const double len[3], const int32_t periodic[3],
#                         emdee_lj_model model, double skin, int32_t precision, emdee_md **out);
# int32_t emdee_md_set_state(emdee_md*, int32_t n_owned, int32_t n_ghost, const void *positions,
#                            const void *velocities, const emdee_lj_atom *atoms, const void *inv_mass);
function VelocityVerlet(positions::HipArray{T,2}, velocities::HipArray{T,2}, L, model::LennardJonesModel,
                        atoms::HipArray{LJAtom,1}; skin=0.3) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    lo = Float64[0, 0, 0]; len = Float64[L, L, L]; per = Int32[1, 1, 1]
    check(ccall((:emdee_md_create, libemdee_hip), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, LennardJonesModel, Float64, Int32, Ref{Ptr{Cvoid}}),
                context().handle, lo, len, per, model, skin, precision_of(T), h))
    md = VelocityVerlet{T}(h[], size(positions, 2))
    # int32_t emdee_md_destroy(emdee_md *md);
    finalizer(m -> ccall((:emdee_md_destroy, libemdee_hip), Int32, (Ptr{Cvoid},), m.handle), md)
    check(ccall((:emdee_md_set_state, libemdee_hip), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                md.handle, md.N, 0, positions.ptr, velocities.ptr, atoms.ptr, C_NULL))
    return md
end

# int32_t emdee_md_step(emdee_md *md, int32_t nsteps, double dt, int32_t rebuild_every);
step!(md::VelocityVerlet, nsteps, dt; rebuild_every=0) =
    check(ccall((:emdee_md_step, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Float64, Int32), md.handle, nsteps, dt, rebuild_every))

# int32_t emdee_md_set_langevin(emdee_md *md, double gamma, double temperature, uint64_t seed, uint64_t first_step);
# gamma > 0: every later step does v = c1 v + c2 sqrt(T/m) xi(seed, step, atom) between its kick and its drift.
set_langevin!(md::VelocityVerlet, gamma, temperature; seed=0, first_step=0) =
    check(ccall((:emdee_md_set_langevin, libemdee_hip), Int32, (Ptr{Cvoid}, Float64, Float64, UInt64, UInt64),
                md.handle, gamma, temperature, seed, first_step))

# int32_t emdee_md_set_exclusions(emdee_md *md, const int32_t *pairs_dev, int32_t n_pairs);
# int32_t emdee_md_set_pairs14(emdee_md *md, const int32_t *pairs_dev, int32_t n_pairs, double lj14scale);
# pairs: 2 x n device matrix of 0-based atom indices (the hooks of src/modelling.jl:197-200: bonded neighbours contribute
# nothing, 1-4 pairs lj14scale times their pair terms); after the state is loaded; `nothing` clears the table.
set_exclusions!(md::VelocityVerlet, pairs::Union{Nothing,HipArray{Int32,2}}) =
    check(ccall((:emdee_md_set_exclusions, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), md.handle,
                pairs === nothing ? C_NULL : pairs.ptr, pairs === nothing ? 0 : size(pairs, 2)))
set_pairs14!(md::VelocityVerlet, pairs::Union{Nothing,HipArray{Int32,2}}, lj14scale) =
    check(ccall((:emdee_md_set_pairs14, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64), md.handle,
                pairs === nothing ? C_NULL : pairs.ptr, pairs === nothing ? 0 : size(pairs, 2), Float64(lj14scale)))

# int32_t emdee_md_set_bonded(emdee_md *md, int32_t kind, const int32_t *atoms_dev, const double *params_dev, int32_t n_terms);
# kind: HARMONIC_BOND (1), HARMONIC_ANGLE (2) or PERIODIC_TORSION (3); atoms: 2|3|4 x n device matrix of 0-based atom
# indices, params: 2|2|3 x n Float64 device matrix ({k, r0}, {k, theta0}, {k, n, phase}); after the state is loaded;
# `nothing` clears the kind's table.
const HARMONIC_BOND, HARMONIC_ANGLE, PERIODIC_TORSION = Int32(1), Int32(2), Int32(3)
set_bonded!(md::VelocityVerlet, kind, atoms::Union{Nothing,HipArray{Int32,2}}, params::Union{Nothing,HipArray{Float64,2}}) =
    check(ccall((:emdee_md_set_bonded, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Int32), md.handle,
                Int32(kind), atoms === nothing ? C_NULL : atoms.ptr, params === nothing ? C_NULL : params.ptr,
                atoms === nothing ? 0 : size(atoms, 2)))

# int32_t emdee_md_set_coulomb(emdee_md *md, const double *charges_dev, int32_t n, double coulomb_k, double eps_rf,
#                              double coulomb14scale);
# Reaction-field Coulomb forces: charges a device Float64 vector in caller order (n = the atom count), coulomb_k in the
# caller's units (138.935457644 kJ mol^-1 nm e^-2), eps_rf >= 1 (Inf: conducting boundary); `nothing` clears them.
set_coulomb!(md::VelocityVerlet, charges::Union{Nothing,HipArray{Float64,1}}, coulomb_k, eps_rf=Inf, coulomb14scale=1.0) =
    check(ccall((:emdee_md_set_coulomb, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Float64, Float64), md.handle,
                charges === nothing ? C_NULL : charges.ptr, charges === nothing ? 0 : length(charges), Float64(coulomb_k),
                Float64(eps_rf), Float64(coulomb14scale)))

# int32_t emdee_md_set_ewald(emdee_md *md, double alpha, const int32_t kmax[3]);
# Ewald summation for a charged engine: alpha > 0 (an inverse length) switches its Coulomb terms from the reaction field to the
# Ewald sum over the integer wave vectors |n_d| <= kmax[d]; alpha = 0 switches back (kmax may then be `nothing`).
set_ewald!(md::VelocityVerlet, alpha, kmax::Union{Nothing,Vector{Int32}}=nothing) =
    check(ccall((:emdee_md_set_ewald, libemdee_hip), Int32, (Ptr{Cvoid}, Float64, Ptr{Int32}), md.handle, Float64(alpha),
                kmax === nothing ? C_NULL : kmax))

# int32_t emdee_md_set_pme(emdee_md *md, double alpha, const int32_t grid[3], int32_t order);
# Smooth particle-mesh Ewald for a charged engine: alpha > 0 switches the reciprocal-space terms of the Ewald sum to a mesh of
# grid[d] points per axis (powers of two in [8, 256]) with B-splines of order 4 or 6; alpha = 0 switches back to the reaction
# field (grid may then be `nothing`).  Whichever of set_ewald! and set_pme! came last with alpha > 0 is in force.
set_pme!(md::VelocityVerlet, alpha, grid::Union{Nothing,Vector{Int32}}=nothing, order=4) =
    check(ccall((:emdee_md_set_pme, libemdee_hip), Int32, (Ptr{Cvoid}, Float64, Ptr{Int32}, Int32), md.handle, Float64(alpha),
                grid === nothing ? C_NULL : grid, Int32(order)))

# int32_t emdee_md_set_rigid3(emdee_md *md, const int32_t *atoms_dev, const double *geom_dev, int32_t n_mol);
# Rigid three-site molecules: atoms a device Int32 matrix (3, n) of caller ids {apex, a, b} (0-based, as the library counts),
# geom a device Float64 matrix (2, n) of {d_leg, d_base}; every later step! holds them rigid (SETTLE + RATTLE).  Moves no atom,
# projects the velocities once; `nothing` clears the table.
set_rigid3!(md::VelocityVerlet, atoms::Union{Nothing,HipArray{Int32,2}}, geom::Union{Nothing,HipArray{Float64,2}}=nothing) =
    check(ccall((:emdee_md_set_rigid3, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32), md.handle,
                atoms === nothing ? C_NULL : atoms.ptr, geom === nothing ? C_NULL : geom.ptr, atoms === nothing ? 0 : size(atoms, 2)))

# int32_t emdee_md_set_hbonds(emdee_md *md, const int32_t *atoms_dev, const double *dist_dev, int32_t n_clusters);
# Bonds to hydrogen at fixed lengths: atoms a device Int32 matrix (4, n) of caller ids {centre, s1, s2, s3} (0-based, -1 in the
# unused trailing slots), dist a device Float64 matrix (3, n) of the centre-satellite distances; every later step! holds them
# (M-SHAKE + RATTLE).  Moves no atom, projects the velocities once; `nothing` clears the table.
set_hbonds!(md::VelocityVerlet, atoms::Union{Nothing,HipArray{Int32,2}}, dist::Union{Nothing,HipArray{Float64,2}}=nothing) =
    check(ccall((:emdee_md_set_hbonds, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32), md.handle,
                atoms === nothing ? C_NULL : atoms.ptr, dist === nothing ? C_NULL : dist.ptr, atoms === nothing ? 0 : size(atoms, 2)))

# int32_t emdee_md_set_vsites(emdee_md *md, const int32_t *atoms_dev, const double *weights_dev, int32_t n_sites);
# Virtual interaction sites (the fourth site of TIP4P-family water and OPC): atoms a device Int32 matrix (4, n) of caller ids
# {site, a, b, c} (0-based, c = -1 for a two-parent site), weights a device Float64 matrix (2, n) of {w_b, w_c}; the sites are
# loaded with inv_mass = 0.  Zeroes the sites' velocities, places them, rebuilds the list and the forces; `nothing` clears the table.
set_vsites!(md::VelocityVerlet, atoms::Union{Nothing,HipArray{Int32,2}}, weights::Union{Nothing,HipArray{Float64,2}}=nothing) =
    check(ccall((:emdee_md_set_vsites, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32), md.handle,
                atoms === nothing ? C_NULL : atoms.ptr, weights === nothing ? C_NULL : weights.ptr, atoms === nothing ? 0 : size(atoms, 2)))

# int32_t emdee_md_set_restraints(emdee_md *md, const int32_t *atoms_dev, const double *ref_dev, const double *k_dev,
#                                 const double *flat_dev, int32_t n);
# Position restraints: atoms a device Int32 vector of n caller ids (0-based), k a device Float64 matrix (3, n) of the spring constants
# per axis, ref a device Float64 matrix (3, n) in the coordinates the state is read back in (unwrapped; `nothing`: every named atom's
# current position), flat a device Float64 vector of the flat-bottom radii (`nothing`: all zero).  U = 1/2 sum k_a d_a^2, or
# 1/2 k max(0, rho - r0)^2 with rho over the axes with k_a > 0.  The references follow the box (scale_box!, the barostats).  Evaluates
# the forces again; atoms = `nothing` clears the table.
set_restraints!(md::VelocityVerlet, atoms::Union{Nothing,HipArray{Int32,1}}, k::Union{Nothing,HipArray{Float64,2}}=nothing;
                ref::Union{Nothing,HipArray{Float64,2}}=nothing, flat::Union{Nothing,HipArray{Float64,1}}=nothing) =
    check(ccall((:emdee_md_set_restraints, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32), md.handle,
                atoms === nothing ? C_NULL : atoms.ptr, ref === nothing ? C_NULL : ref.ptr, k === nothing ? C_NULL : k.ptr,
                flat === nothing ? C_NULL : flat.ptr, atoms === nothing ? 0 : length(atoms)))

# int32_t emdee_md_restraint_sums(emdee_md *md, double out[EMDEE_RESTRAINT_WORDS]);
# (blocking) [1] the restraint energy, [2:7] the sum of the restraint tensors (xx, yy, zz, xy, xz, yz), [8] the largest |x - ref|
function restraint_sums(md::VelocityVerlet)
    out = zeros(Float64, 8)
    check(ccall((:emdee_md_restraint_sums, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, out))
    return out
end

# int32_t emdee_md_get_restraint_refs(emdee_md *md, double *ref_dev);
# The references as they now stand (they follow the box), into a device Float64 matrix (3, n), table order.
restraint_refs!(md::VelocityVerlet, out::HipArray{Float64,2}) =
    (check(ccall((:emdee_md_get_restraint_refs, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), md.handle, out.ptr)); out)

# int32_t emdee_md_set_pull(emdee_md *md, const int32_t *group_dev, int32_t n_groups, const int32_t *coords, const double *params,
#                           int32_t n_coords, int32_t log_every, int32_t log_capacity);
# Centre-of-mass pulling: group a device Int32 vector of n_owned entries in -1 ... n_groups - 1; coords a HOST Int32 matrix (5, n_coords)
# of {a, b, kind, geometry, mask} (groups 0-based; kind 1 umbrella, 2 constant force; geometry 1 distance, 2 direction; mask bits 1..7);
# params a HOST Float64 matrix (6, n_coords) of {k or F, r0, rate, nx, ny, nz}.  U = 1/2 k (xi - xi0)^2 with xi0 = r0 + rate t, or -F xi.
# xi0 and r0 do not scale with the box.  Evaluates the forces again; coords = `nothing` clears the table.
function set_pull!(md::VelocityVerlet, group::Union{Nothing,HipArray{Int32,1}}, n_groups::Integer,
                   coords::Union{Nothing,Matrix{Int32}}, params::Union{Nothing,Matrix{Float64}}; log_every::Integer=0, log_capacity::Integer=0)
    check(ccall((:emdee_md_set_pull, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Int32, Int32, Int32), md.handle,
                group === nothing ? C_NULL : group.ptr, n_groups, coords === nothing ? C_NULL : coords, params === nothing ? C_NULL : params,
                coords === nothing ? 0 : size(coords, 2), log_every, log_capacity))
end

# int32_t emdee_md_pull_read(emdee_md *md, double *coords_out, double *groups_out);
# (blocking, one copy) what the last force pass wrote: (8, n_coords) {xi, xi0, f, U, work, Dx, Dy, Dz} and (4, n_groups) {X, Y, Z, M}
function pull_read(md::VelocityVerlet, n_coords::Integer, n_groups::Integer)
    c, g = zeros(Float64, 8, n_coords), zeros(Float64, 4, n_groups)
    check(ccall((:emdee_md_pull_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), md.handle, c, g))
    return c, g
end

# int32_t emdee_md_pull_log_read(emdee_md *md, double *log_dev, int64_t *count, int64_t *dropped);
# The log so far into a device Float64 array (2, n_coords, capacity) of {xi, f}; returns (count, dropped).
function pull_log_read!(md::VelocityVerlet, out::HipArray{Float64,3})
    count, dropped = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:emdee_md_pull_log_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), md.handle, out.ptr, count, dropped))
    return count[], dropped[]
end

# int32_t emdee_md_set_alchemical(emdee_md *md, const int32_t *flag_dev, double lambda, double alpha, const double *foreign,
#                                 int32_t n_foreign, int32_t log_every, int32_t log_capacity);
# Soft-core alchemical decoupling: flag a device Int32 vector of n_owned entries (1 solute, 0 environment); the Lennard-Jones coupling
# between flagged and unflagged atoms becomes lambda 4 eps (D^-2 - D^-1) g with D = alpha (1 - lambda) + (r / sigma)^6.  foreign: HOST
# Float64 vector of up to 16 more lambdas for BAR / MBAR.  Rebuilds the list and evaluates the forces again; flag = `nothing` clears.
function set_alchemical!(md::VelocityVerlet, flag::Union{Nothing,HipArray{Int32,1}}; lambda::Real=1.0, alpha::Real=0.5,
                         foreign::Vector{Float64}=Float64[], log_every::Integer=0, log_capacity::Integer=0)
    check(ccall((:emdee_md_set_alchemical, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}, Int32, Int32, Int32), md.handle,
                flag === nothing ? C_NULL : flag.ptr, lambda, alpha, isempty(foreign) ? C_NULL : foreign, length(foreign), log_every, log_capacity))
end

# int32_t emdee_md_set_lambda(emdee_md *md, double lambda);
# (a host scalar: no rebuild; the next step or query evaluates the forces anew)
set_lambda!(md::VelocityVerlet, lambda::Real) =
    check(ccall((:emdee_md_set_lambda, libemdee_hip), Int32, (Ptr{Cvoid}, Float64), md.handle, lambda))

# int32_t emdee_md_alchemical_read(emdee_md *md, double *words);
# (blocking) {lambda, U_alch, dU/dlambda, the cross virial, the cross pairs inside rc}, then U_alch at the n_foreign foreign lambdas
function alchemical_read(md::VelocityVerlet, n_foreign::Integer)
    w = zeros(Float64, 5 + n_foreign)
    check(ccall((:emdee_md_alchemical_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, w))
    return w
end

# int32_t emdee_md_alchemical_log_read(emdee_md *md, double *log_dev, int64_t *count, int64_t *dropped);
# The log so far into a device Float64 array (2 + n_foreign, capacity) of {dU/dlambda, U_alch, foreign ...}; returns (count, dropped).
function alchemical_log_read!(md::VelocityVerlet, out::HipArray{Float64,2})
    count, dropped = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:emdee_md_alchemical_log_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), md.handle, out.ptr, count, dropped))
    return count[], dropped[]
end

# int32_t emdee_md_set_alchemical_coulomb(emdee_md *md, int32_t enable, double lambda_q, double beta, const double *foreign_q,
#                                         int32_t n_foreign);
# The Coulomb stage of the alchemical table in force, on the reaction field: every cross pair's charge term becomes
# lambda_q qq (1/rho + k_rf rho^2 - c_rf) with rho^2 = r^2 + beta (1 - lambda_q).  foreign_q: HOST Float64 vector, as long as the table's
# foreign lambdas.  No rebuild; restarts the table's step count and both logs.  lambda_q = `nothing` clears the stage.
function set_alchemical_coulomb!(md::VelocityVerlet, lambda_q::Union{Nothing,Real}; beta::Real=0.0, foreign_q::Vector{Float64}=Float64[])
    if lambda_q === nothing
        return check(ccall((:emdee_md_set_alchemical_coulomb, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Float64, Float64, Ptr{Float64}, Int32),
                           md.handle, 0, 1.0, 0.0, C_NULL, 0))
    end
    check(ccall((:emdee_md_set_alchemical_coulomb, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Float64, Float64, Ptr{Float64}, Int32), md.handle, 1,
                lambda_q, beta, isempty(foreign_q) ? C_NULL : foreign_q, length(foreign_q)))
end

# int32_t emdee_md_set_lambda_coulomb(emdee_md *md, double lambda_q);
# (a host scalar: no rebuild; the next step or query evaluates the forces anew)
set_lambda_coulomb!(md::VelocityVerlet, lambda_q::Real) =
    check(ccall((:emdee_md_set_lambda_coulomb, libemdee_hip), Int32, (Ptr{Cvoid}, Float64), md.handle, lambda_q))

# int32_t emdee_md_alchemical_coulomb_read(emdee_md *md, double *words);
# (blocking) {lambda_q, U_q, dU_q/dlambda_q, the cross Coulomb virial}, then U_q at the n_foreign foreign lambda_q
function alchemical_coulomb_read(md::VelocityVerlet, n_foreign::Integer)
    w = zeros(Float64, 4 + n_foreign)
    check(ccall((:emdee_md_alchemical_coulomb_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, w))
    return w
end

# int32_t emdee_md_alchemical_coulomb_log_read(emdee_md *md, double *log_dev, int64_t *count, int64_t *dropped);
# The second log so far into a device Float64 array (2 + n_foreign, capacity) of {dU_q/dlambda_q, U_q, foreign ...}; returns (count, dropped).
function alchemical_coulomb_log_read!(md::VelocityVerlet, out::HipArray{Float64,2})
    count, dropped = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:emdee_md_alchemical_coulomb_log_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), md.handle, out.ptr, count,
                dropped))
    return count[], dropped[]
end

# int32_t emdee_md_minimize(emdee_md *md, int32_t max_iter, double f_tol, double dt_start, double dt_max, double max_step,
#                           emdee_minimize_result *out);
# Energy minimisation by FIRE around the constrained step: at most max_iter iterations, until no atom's constrained force exceeds
# f_tol.  OVERWRITES the velocities with zeros.  Returns the emdee_minimize_result.
struct MinimizeResult
    iterations::Int32
    converged::Int32
    rebuilds::Int32
    reserved::Int32
    energy0::Float64
    energy::Float64
    g_max::Float64
    dt::Float64
end
function minimize!(md::VelocityVerlet, max_iter, f_tol; dt_start=0.001, dt_max=0.01, max_step=0.1)
    out = Ref(MinimizeResult(0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0))
    check(ccall((:emdee_md_minimize, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Float64, Float64, Float64, Float64, Ref{MinimizeResult}), md.handle,
                Int32(max_iter), Float64(f_tol), Float64(dt_start), Float64(dt_max), Float64(max_step), out))
    return out[]
end

# Pressure coupling (include/emdee_hip.h; undivided boxes).
# int32_t emdee_md_get_box(emdee_md *md, double lo[3], double len[3]);   -> (lo, len) of the engine's box
function box(md::VelocityVerlet)
    lo = zeros(Float64, 3); len = zeros(Float64, 3)
    check(ccall((:emdee_md_get_box, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), md.handle, lo, len))
    return (lo=lo, len=len)
end

# int32_t emdee_md_scale_box(emdee_md *md, const double mu[3], double velocity_scale);
# x <- lo + mu (x - lo) per axis, len <- mu len, v <- velocity_scale v; then re-bin, re-plan, rebuild and a force pass.
scale_box!(md::VelocityVerlet, mu, velocity_scale=1.0) =
    check(ccall((:emdee_md_scale_box, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}, Float64), md.handle,
                Float64[mu[1], mu[2], mu[3]], Float64(velocity_scale)))

# int32_t emdee_md_set_barostat(emdee_md *md, int32_t kind, int32_t coupling, const double p_ref[3], const double compressibility[3],
#                               double tau_p, int32_t every, double temperature, uint64_t seed, uint64_t first_step);
# kind: BAROSTAT_OFF, BAROSTAT_BERENDSEN or BAROSTAT_CRESCALE (isotropic only; needs temperature > 0); p_ref and compressibility:
# three entries (isotropic reads entry 1, semi-isotropic 1 for x and y and 3 for z); every: steps between coupling events.
const BAROSTAT_OFF, BAROSTAT_BERENDSEN, BAROSTAT_CRESCALE = Int32(0), Int32(1), Int32(2)
const COUPLE_ISOTROPIC, COUPLE_SEMIISOTROPIC, COUPLE_ANISOTROPIC = Int32(0), Int32(1), Int32(2)
set_barostat!(md::VelocityVerlet, kind, p_ref, compressibility, tau_p, every; coupling=COUPLE_ISOTROPIC, temperature=0.0, seed=0,
              first_step=0) =
    check(ccall((:emdee_md_set_barostat, libemdee_hip), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Float64, Int32, Float64, UInt64, UInt64), md.handle,
                Int32(kind), Int32(coupling), Float64[p_ref[1], p_ref[2], p_ref[3]],
                Float64[compressibility[1], compressibility[2], compressibility[3]], Float64(tau_p), Int32(every),
                Float64(temperature), UInt64(seed), UInt64(first_step)))

# Global thermostats (include/emdee_hip.h; undivided boxes).
# int32_t emdee_md_set_thermostat(emdee_md *md, int32_t kind, double temperature, double tau_t, int32_t every, int64_t n_dof,
#                                 int32_t chain, uint64_t seed, uint64_t first_step);
# kind: THERMOSTAT_OFF, THERMOSTAT_VRESCALE or THERMOSTAT_NOSE_HOOVER (chain: its length, 1...8); temperature: kT in energy units;
# every: steps between events; n_dof: the degrees of freedom, 0 for the library's own count from the tables in force.
const THERMOSTAT_OFF, THERMOSTAT_VRESCALE, THERMOSTAT_NOSE_HOOVER = Int32(0), Int32(1), Int32(2)
const THERMOSTAT_WORDS = 20
set_thermostat!(md::VelocityVerlet, kind, temperature=1.0, tau_t=1.0; every=1, n_dof=0, chain=3, seed=0, first_step=0) =
    check(ccall((:emdee_md_set_thermostat, libemdee_hip), Int32,
                (Ptr{Cvoid}, Int32, Float64, Float64, Int32, Int64, Int32, UInt64, UInt64), md.handle,
                Int32(kind), Float64(temperature), Float64(tau_t), Int32(every), Int64(n_dof), Int32(chain), UInt64(seed),
                UInt64(first_step)))

# int32_t emdee_md_thermostat_state(emdee_md *md, double out[EMDEE_THERMOSTAT_WORDS]);
# -> n_dof in use, K as the last event saw it, that event's alpha, E_th (U + K + E_th is conserved), xi (8), v_xi (8)
function thermostat_state(md::VelocityVerlet)
    w = zeros(Float64, THERMOSTAT_WORDS)
    check(ccall((:emdee_md_thermostat_state, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, w))
    return (n_dof=Int(w[1]), kinetic=w[2], alpha=w[3], energy=w[4], xi=w[5:12], v_xi=w[13:20])
end

# int32_t emdee_md_set_thermostat_state(emdee_md *md, const double in[EMDEE_THERMOSTAT_WORDS]);
# writes energy, xi and v_xi of a thermostat_state; a restart is set_thermostat!(...; first_step = steps done), then this
function set_thermostat_state!(md::VelocityVerlet, state)
    w = vcat(zeros(Float64, 3), Float64(state.energy), Float64.(state.xi), Float64.(state.v_xi))
    length(w) == THERMOSTAT_WORDS || throw(DimensionMismatch("xi and v_xi take 8 numbers each"))
    check(ccall((:emdee_md_set_thermostat_state, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, w))
end

# int32_t emdee_md_thermostat_draws(emdee_md *md, uint64_t seed, uint64_t step, int64_t n_dof, double out[2]);
# v-rescale's generator on its own: (R1, S) of the event that completes step `step`
function thermostat_draws(md::VelocityVerlet, seed, step, n_dof)
    out = zeros(Float64, 2)
    check(ccall((:emdee_md_thermostat_draws, libemdee_hip), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ptr{Float64}), md.handle,
                UInt64(seed), UInt64(step), Int64(n_dof), out))
    return (out[1], out[2])
end

# Radial distribution functions (include/emdee_hip.h; undivided boxes, periodic in all three dimensions).
# int32_t emdee_md_set_rdf(emdee_md *md, double r_max, int32_t n_bins, int32_t n_groups, const int32_t *group_dev,
#                          const int32_t *molecule_dev);
# groups, molecules: device Int32 vectors in caller order, or `nothing` (every atom in group 0 / no molecules); a group of -1
# leaves the atom out, pairs with equal molecule entries >= 0 are skipped.  n_bins = 0 clears the table.
const RDF_MAX_GROUPS = 8
function set_rdf!(md::VelocityVerlet, r_max, n_bins; n_groups=1, groups::Union{Nothing,HipArray{Int32,1}}=nothing,
                  molecules::Union{Nothing,HipArray{Int32,1}}=nothing)
    check(ccall((:emdee_md_set_rdf, libemdee_hip), Int32, (Ptr{Cvoid}, Float64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}), md.handle,
                Float64(r_max), Int32(n_bins), Int32(n_groups), groups === nothing ? C_NULL : groups.ptr,
                molecules === nothing ? C_NULL : molecules.ptr))
end

# int32_t emdee_md_rdf_sample(emdee_md *md);
# adds the current positions as one frame: queued on the stream, nothing read back, the run untouched
rdf_sample!(md::VelocityVerlet) = check(ccall((:emdee_md_rdf_sample, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_rdf_reset(emdee_md *md);
rdf_reset!(md::VelocityVerlet) = check(ccall((:emdee_md_rdf_reset, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_rdf_read(emdee_md *md, int64_t *counts, int64_t group_sizes[8], int64_t *frames, double *inv_volume_sum);
# blocking -> (counts (n_bins x n_pairs: column s = slot a n_groups - a (a - 1) / 2 + (b - a) of the pair a <= b), group sizes,
# frames, sum of 1 / V); g_ab = counts / (P_ab (4 pi / 3) (r_{k+1}^3 - r_k^3) inv_volume_sum), P_ab = N_a N_b or N_a (N_a - 1) / 2
function rdf_read(md::VelocityVerlet, n_bins, n_groups)
    n_pairs = n_groups * (n_groups + 1) ÷ 2
    counts = zeros(Int64, n_bins, n_pairs)
    sizes = zeros(Int64, RDF_MAX_GROUPS)
    frames = Ref{Int64}(0)
    inv_volume_sum = Ref{Float64}(0.0)
    check(ccall((:emdee_md_rdf_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}), md.handle,
                counts, sizes, frames, inv_volume_sum))
    return (counts=counts, group_sizes=sizes[1:n_groups], frames=frames[], inv_volume_sum=inv_volume_sum[])
end

# Mean-squared displacement and velocity autocorrelation (include/emdee_hip.h; undivided boxes).
# int32_t emdee_md_set_msd(emdee_md *md, int32_t what, int32_t n_groups, const int32_t *group_dev, int32_t n_lags,
#                          int32_t origin_every);
# what: EMDEE_MSD | EMDEE_VACF.  groups: a device Int32 vector in caller order, or `nothing` (every atom in group 0); a group of -1
# leaves the atom out.  n_lags in 1...4096, at most 64 origins within them; n_lags = 0 clears the table.
const EMDEE_MSD = 1
const EMDEE_VACF = 2
const EMDEE_MSD_WORDS = 7
function set_msd!(md::VelocityVerlet, n_lags; origin_every=1, n_groups=1, groups::Union{Nothing,HipArray{Int32,1}}=nothing,
                  what=EMDEE_MSD | EMDEE_VACF)
    check(ccall((:emdee_md_set_msd, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Int32, Int32), md.handle,
                Int32(what), Int32(n_groups), groups === nothing ? C_NULL : groups.ptr, Int32(n_lags), Int32(origin_every)))
end

# int32_t emdee_md_msd_sample(emdee_md *md);
# the current state as the next sample: queued on the stream, nothing read back, the run untouched
msd_sample!(md::VelocityVerlet) = check(ccall((:emdee_md_msd_sample, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_msd_reset(emdee_md *md);
msd_reset!(md::VelocityVerlet) = check(ccall((:emdee_md_msd_reset, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_msd_read(emdee_md *md, double *sums, int64_t *origins, int64_t group_sizes[8], int64_t *samples);
# blocking -> (sums (7 x n_groups x n_lags: word w of group g at lag l is sums[w + 1, g + 1, l + 1]), origins per lag, group sizes,
# samples); MSD(l) = (w0 + w1 + w2) / (origins N_g), drift-free: minus (w3 + w4 + w5) / N_g first; VACF(l) = w6 / (origins N_g)
function msd_read(md::VelocityVerlet, n_lags, n_groups)
    sums = zeros(Float64, EMDEE_MSD_WORDS, n_groups, n_lags)
    origins = zeros(Int64, n_lags)
    sizes = zeros(Int64, RDF_MAX_GROUPS)
    samples = Ref{Int64}(0)
    check(ccall((:emdee_md_msd_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), md.handle,
                sums, origins, sizes, samples))
    return (sums=sums, origins=origins, group_sizes=sizes[1:n_groups], samples=samples[])
end

# Green-Kubo observables: the autocorrelations of the stress and of the heat flux (include/emdee_hip.h; undivided engines).
# int32_t emdee_md_set_gk(emdee_md *md, int32_t what, int32_t n_lags);
# what: EMDEE_GK_STRESS | EMDEE_GK_HEAT.  n_lags in 1...65536; n_lags = 0 clears the table.
const EMDEE_GK_STRESS = 1
const EMDEE_GK_HEAT = 2
const EMDEE_GK_WORDS = 9
function set_gk!(md::VelocityVerlet, n_lags; what=EMDEE_GK_STRESS | EMDEE_GK_HEAT)
    check(ccall((:emdee_md_set_gk, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Int32), md.handle, Int32(what), Int32(n_lags)))
end

# int32_t emdee_md_gk_sample(emdee_md *md);
# the current state as the next sample: queued on the stream, nothing read back, the run untouched
gk_sample!(md::VelocityVerlet) = check(ccall((:emdee_md_gk_sample, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_gk_reset(emdee_md *md);
gk_reset!(md::VelocityVerlet) = check(ccall((:emdee_md_gk_reset, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_gk_read(emdee_md *md, double *sums, double totals[9], double last[9], int64_t *samples);
# blocking -> (sums (9 x n_lags: word w at lag l is sums[w + 1, l + 1], behind it max(0, samples - l) products), totals, last, samples);
# words 0-4: the traceless stress components, 5: p V, 6-8: the heat flux
function gk_read(md::VelocityVerlet, n_lags)
    sums = zeros(Float64, EMDEE_GK_WORDS, n_lags)
    totals = zeros(Float64, EMDEE_GK_WORDS)
    last = zeros(Float64, EMDEE_GK_WORDS)
    samples = Ref{Int64}(0)
    check(ccall((:emdee_md_gk_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), md.handle,
                sums, totals, last, samples))
    return (sums=sums, totals=totals, last=last, samples=samples[])
end

# Spatial profiles along an axis and around a centre (include/emdee_hip.h; undivided engines).
# int32_t emdee_md_set_spatial(emdee_md *md, int32_t geometry, int32_t what, int32_t n_bins, int32_t n_groups,
#                              const int32_t *group_dev, const double range[2], const double centre[3], int32_t centre_group);
# geometry: EMDEE_SPATIAL_X, _Y, _Z (range === nothing on a periodic axis, (r0, r1) on an open one) or EMDEE_SPATIAL_RADIAL
# (range = (0, r_max); centre, or centre_group >= 0: that group's centre of mass, formed on the device at every sample).  what: a
# mask of EMDEE_SPATIAL_DENSITY | _KINETIC | _STRESS.  groups as set_msd! takes them.  n_bins in 1...4096; n_bins = 0 clears the table.
const EMDEE_SPATIAL_X = 0
const EMDEE_SPATIAL_Y = 1
const EMDEE_SPATIAL_Z = 2
const EMDEE_SPATIAL_RADIAL = 3
const EMDEE_SPATIAL_DENSITY = 1
const EMDEE_SPATIAL_KINETIC = 2
const EMDEE_SPATIAL_STRESS = 4
const EMDEE_SPATIAL_WORDS = 10
function set_spatial!(md::VelocityVerlet, geometry, n_bins; what=EMDEE_SPATIAL_DENSITY | EMDEE_SPATIAL_KINETIC | EMDEE_SPATIAL_STRESS,
                      n_groups=1, groups::Union{Nothing,HipArray{Int32,1}}=nothing, range=nothing, centre=nothing, centre_group=-1)
    rng = range === nothing ? C_NULL : Float64[range[1], range[2]]
    ctr = centre === nothing ? C_NULL : Float64[centre[1], centre[2], centre[3]]
    check(ccall((:emdee_md_set_spatial, libemdee_hip), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32),
                md.handle, Int32(geometry), Int32(what), Int32(n_bins), Int32(n_groups), groups === nothing ? C_NULL : groups.ptr, rng, ctr,
                Int32(centre_group)))
end

# int32_t emdee_md_spatial_sample(emdee_md *md);
# the current state as one more frame: queued on the stream, nothing read back, the run untouched
spatial_sample!(md::VelocityVerlet) = check(ccall((:emdee_md_spatial_sample, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_spatial_reset(emdee_md *md);
spatial_reset!(md::VelocityVerlet) = check(ccall((:emdee_md_spatial_reset, libemdee_hip), Int32, (Ptr{Cvoid},), md.handle))

# int32_t emdee_md_spatial_read(emdee_md *md, int64_t *counts, double *sums, int64_t outside[8], int64_t group_sizes[8],
#                               int64_t *frames, double *inv_bin_volume_sum);
# blocking -> (counts (n_bins x n_groups), sums (10 x n_bins x n_groups: word w of bin k of group g is sums[w + 1, k + 1, g + 1]),
# outside, group sizes, frames, inv_bin_volume_sum); P_N = (w6 + w9) / V_bin, P_T = ((w5 - w6) + (w8 - w9)) / (2 V_bin)
function spatial_read(md::VelocityVerlet, n_bins, n_groups)
    counts = zeros(Int64, n_bins, n_groups)
    sums = zeros(Float64, EMDEE_SPATIAL_WORDS, n_bins, n_groups)
    outside = zeros(Int64, RDF_MAX_GROUPS)
    sizes = zeros(Int64, RDF_MAX_GROUPS)
    frames = Ref{Int64}(0)
    inv_bin_volume_sum = Ref{Float64}(0.0)
    check(ccall((:emdee_md_spatial_read, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                md.handle, counts, sums, outside, sizes, frames, inv_bin_volume_sum))
    return (counts=counts, sums=sums, outside=outside[1:n_groups], group_sizes=sizes[1:n_groups], frames=frames[],
            inv_bin_volume_sum=inv_bin_volume_sum[])
end

# int32_t emdee_md_set_langevin_ids(emdee_md *md, const int64_t *ids_dev);
# Atom ids keying the thermostat's noise (device Int64 vector in caller order); `nothing` = the caller index.
set_langevin_ids!(md::VelocityVerlet, ids::Union{Nothing,HipArray{Int64,1}}) =
    check(ccall((:emdee_md_set_langevin_ids, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), md.handle,
                ids === nothing ? C_NULL : ids.ptr))

# int32_t emdee_md_energies(emdee_md *md, double out[3]);   -> (potential, kinetic, virial sum)
function energies(md::VelocityVerlet)
    out = zeros(Float64, 3)
    check(ccall((:emdee_md_energies, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, out))
    return (potential=out[1], kinetic=out[2], virial=out[3])
end

# int32_t emdee_md_virial_tensor(emdee_md *md, void *tensor);   per-atom virial tensors, 6 x N, rows (xx, yy, zz, xy, xz, yz)
function virial_tensor!(tensor::HipArray{T,2}, md::VelocityVerlet{T}) where {T}
    size(tensor) == (6, md.N) || throw(DimensionMismatch("tensor must be 6 x $(md.N)"))
    check(ccall((:emdee_md_virial_tensor, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), md.handle, tensor.ptr))
    return tensor
end

# the twelve sums (xx, yy, zz, xy, xz, yz of W, then of K) -> symmetric 3x3 matrices
tensor3(s) = [s[1] s[4] s[5]; s[4] s[2] s[6]; s[5] s[6] s[3]]

# int32_t emdee_md_pressure_tensor(emdee_md *md, double out[12]);   -> (virial = sum W_i, kinetic = sum m v v, pressure = (K + W) / V)
function pressure_tensor(md::VelocityVerlet, volume)
    out = zeros(Float64, 12)
    check(ccall((:emdee_md_pressure_tensor, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, out))
    W, K = tensor3(out[1:6]), tensor3(out[7:12])
    return (virial=W, kinetic=K, pressure=(K + W) / volume)
end

# int32_t emdee_md_molecular_pressure_tensor(emdee_md *md, double out[12]);   -> pressure_tensor from the molecular sums W_mol, K_mol:
# the atomic sums minus what the atoms of the rigid molecules (set_rigid3!) carry about their centres of mass; without a table,
# pressure_tensor itself
function molecular_pressure_tensor(md::VelocityVerlet, volume)
    out = zeros(Float64, 12)
    check(ccall((:emdee_md_molecular_pressure_tensor, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Float64}), md.handle, out))
    W, K = tensor3(out[1:6]), tensor3(out[7:12])
    return (virial=W, kinetic=K, pressure=(K + W) / volume)
end

# int32_t emdee_md_set_molecular_scaling(emdee_md *md, int32_t on);
# on: an engine with rigid molecules accepts scale_box! and set_barostat! -- molecules are translated with their centres of mass,
# and the coupling takes the molecular pressure; changes nothing for an engine without a table.
set_molecular_scaling!(md::VelocityVerlet, on::Bool=true) =
    check(ccall((:emdee_md_set_molecular_scaling, libemdee_hip), Int32, (Ptr{Cvoid}, Int32), md.handle, Int32(on)))

# int32_t emdee_md_set_molecules(emdee_md *md, const int32_t *molecule_dev, int32_t n);
# The molecule table: a device Int32 vector of one id per atom in caller order, equal ids >= 0 form one molecule, -1 is a molecule
# of one.  With set_molecular_scaling! on, the molecular pressure, scale_box! and the barostats take whole molecules from it, and an
# engine with set_hbonds! in force can be pressure-coupled.  Load every molecule whole; `nothing` clears the table.
set_molecules!(md::VelocityVerlet, molecule::Union{Nothing,HipArray{Int32,1}}) =
    check(ccall((:emdee_md_set_molecules, libemdee_hip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), md.handle,
                molecule === nothing ? C_NULL : molecule.ptr, molecule === nothing ? 0 : length(molecule)))

# int32_t emdee_md_get_state(emdee_md*, void *positions, void *velocities, void *forces, void *energies, void *virials);
function state!(md::VelocityVerlet{T}, positions::HipArray{T,2}, velocities::HipArray{T,2}, forces::HipArray{T,2}) where {T}
    check(ccall((:emdee_md_get_state, libemdee_hip), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                md.handle, positions.ptr, velocities.ptr, forces.ptr, C_NULL, C_NULL))
    return nothing
end
