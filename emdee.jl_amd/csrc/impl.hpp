// impl.hpp -- the objects behind the C ABI handles, templated on the real type.
#pragma once

#include "allpairs.hpp"
#include "iface.hpp"
#include "nbsys.hpp"

namespace emdee {

// ------------------------------------------------------------------------------------ Cells
// Cells(r, L, cutoff; ndiv) / update_cells! -- src/cells.jl:176-222.  head/next linked lists become
// start/order arrays (counting sort); index and population keep the reference's meaning.
template <typename real>
struct CellsImpl : ICells {
    emdee_ctx *ctx;
    int N, Mdim;
    GridP<real> grid{};
    size_t ncell;
    DevBuf<int> index, population, start, fill, tmp, order;
    Scanner scanner;

    CellsImpl(emdee_ctx *c, int n, double L, double cutoff, int ndiv) : ctx(c), N(n) {
        EMDEE_REQUIRE(n >= 0 && L > 0 && cutoff > 0 && ndiv >= 1, EMDEE_ERR_INVALID, "Cells: need N >= 0, L > 0, cutoff > 0, ndiv >= 1");
        Mdim = std::max(1, (int)std::floor((double)ndiv * L / cutoff));   // src/cells.jl:36
        EMDEE_REQUIRE(Mdim <= 1290, EMDEE_ERR_INVALID, "Cells: M = %d cells per dimension overflows int32 ids", Mdim);
        for (int d = 0; d < 3; d++) {
            grid.lo[d] = 0; grid.len[d] = (real)L; grid.plen[d] = (real)L; grid.pinv[d] = (real)(1.0 / L);
            grid.per[d] = 1; grid.M[d] = Mdim;
        }
        grid.nd = ndiv;
        grid.one_based = 1;   // src/cells.jl:85,181
        ncell = (size_t)Mdim * Mdim * Mdim;
        index.ensure(n + 1); tmp.ensure(n + 1); order.ensure(n + 1);
        population.ensure(ncell + 2); start.ensure(ncell + 2); fill.ensure(ncell + 2);
    }

    void update(const void *positions) override {
        EMDEE_REQUIRE(positions || N == 0, EMDEE_ERR_INVALID, "Cells: positions is NULL");
        use_device(ctx);
        hipStream_t s = ctx->stream;
        EMDEE_HIP_CHECK(hipMemsetAsync(population.ptr, 0, (ncell + 1) * sizeof(int), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(fill.ptr, 0, ncell * sizeof(int), s));
        if (N > 0)
            hipLaunchKernelGGL((k_cell_assign<real, UserPos<real>>), dim3(blocks_for(N, 256)), dim3(256), 0, s, N,
                               UserPos<real>{(const real *)positions}, grid, index.ptr, population.ptr);
        EMDEE_HIP_CHECK(hipMemcpyAsync(start.ptr, population.ptr, (ncell + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
        scanner.run(start.ptr, ncell + 1, s);
        if (N > 0) {
            hipLaunchKernelGGL(k_cell_scatter, dim3(blocks_for(N, 256)), dim3(256), 0, s, N, index.ptr, 1, start.ptr,
                               fill.ptr, tmp.ptr);
            hipLaunchKernelGGL(k_cell_rankfix, dim3(blocks_for(N, 256)), dim3(256), 0, s, N, index.ptr, 1, start.ptr,
                               tmp.ptr, (const int *)nullptr, order.ptr);
        }
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    int M() const override { return Mdim; }
    void arrays(const int32_t **i, const int32_t **p, const int32_t **s, const int32_t **o) const override {
        if (i) *i = index.ptr;
        if (p) *p = population.ptr;
        if (s) *s = start.ptr;
        if (o) *o = order.ptr;
    }
};

// ------------------------------------------------------------------------------------ neighbour handle
template <typename real>
struct NbrImpl : INbr {
    NbSystem<real> sys;
    int N;
    double L_built = -1.0;

    NbrImpl(emdee_ctx *c, int n, double skin) : N(n) {
        EMDEE_REQUIRE(n >= 0 && skin >= 0, EMDEE_ERR_INVALID, "nbr: need N >= 0 and skin >= 0");
        sys.ctx = c;
        sys.skin = skin;
        // Float32 callers get the reference's Float32 pair geometry (EMDEE_F32_FAST=1: the MD loop's brick-relative tiles)
        sys.refmath = sizeof(real) == 4 && !std::getenv("EMDEE_F32_FAST");
    }

    void compute(void *forces, void *energies, void *virials, const void *positions, double L, const emdee_lj_model &model,
                 const emdee_lj_atom *atoms, int bitmask) override {
        EMDEE_REQUIRE(bitmask >= 0 && bitmask <= 7, EMDEE_ERR_INVALID, "bitmask must be a combination of FORCES|ENERGIES|VIRIALS");
        EMDEE_REQUIRE(!(bitmask & EMDEE_FORCES) || forces || N == 0, EMDEE_ERR_INVALID, "forces selected but NULL");
        EMDEE_REQUIRE(!(bitmask & EMDEE_ENERGIES) || energies || N == 0, EMDEE_ERR_INVALID, "energies selected but NULL");
        EMDEE_REQUIRE(!(bitmask & EMDEE_VIRIALS) || virials || N == 0, EMDEE_ERR_INVALID, "virials selected but NULL");
        Pass<real> out = Pass<real>::force(bitmask);
        if (bitmask & EMDEE_FORCES) out.f = (real *)forces;
        if (bitmask & EMDEE_ENERGIES) out.e = (real *)energies;
        if (bitmask & EMDEE_VIRIALS) out.w = (real *)virials;
        run(out, positions, L, model, atoms);
    }
    // emdee_compute_virial_tensor: the per-atom virial tensors (6 x N, caller order) of the same pairs compute() sums
    void compute_tensor(void *tensor, const void *positions, double L, const emdee_lj_model &model, const emdee_lj_atom *atoms) override {
        EMDEE_REQUIRE(tensor || N == 0, EMDEE_ERR_INVALID, "tensor is NULL");
        Pass<real> out = Pass<real>::force(TENSOR_PASS);
        out.vt = (real *)tensor;
        run(out, positions, L, model, atoms);
    }
    // one pass into the caller-order arrays of `out`: the tiled kernels write them themselves (owner lane, caller index from
    // perm), staging the tiles of the Float32 reference arithmetic from the caller's positions; the direct kernels write the
    // engine's arrays, which are then copied out
    void run(const Pass<real> &out, const void *positions, double L, const emdee_lj_model &model, const emdee_lj_atom *atoms) {
        use_device(sys.ctx);
        EMDEE_REQUIRE(L > 0, EMDEE_ERR_INVALID, "L must be positive");
        if (N == 0 || out.mask == 0) return;
        EMDEE_REQUIRE(positions && atoms, EMDEE_ERR_INVALID, "positions/atoms are NULL");
        prepare((const real *)positions, L, model, atoms);
        if (sys.brick_active) {
            Pass<real> p = out;
            p.pos = (const real *)positions;
            sys.compute_forces(p);
        } else {
            sys.compute_forces(out.mask);
            if (out.vt) sys.unsort_tensor(out.vt);
            else sys.unsort(nullptr, nullptr, out.f, out.e, out.w);
        }
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    // the list for these positions: kept if it still covers them, else re-sorted or rebuilt
    void prepare(const real *pos, double L, const emdee_lj_model &model, const emdee_lj_atom *atoms) {
        const double lo[3] = {0, 0, 0}, len[3] = {L, L, L};
        const int per[3] = {1, 1, 1};   // cubic periodic box, the reference's only geometry (Q9)
        sys.set_box(lo, len, per);
        sys.set_model(model, sys.skin);
        bool rebuild = !sys.has_list || sys.n_total != N;
        // list kept: one pass refreshes the records, tests the displacements and re-checks the species (the caller
        // may have edited atoms); one read-back
        bool resorted = false;
        if (!rebuild) {
            const bool was_uniform = sys.uniform_atoms;
            rebuild = sys.refresh_and_check(pos, atoms);
            // The list is outrun, but the pass above has just written the caller's positions (and LJAtom values) into the
            // cell-ordered records: an untyped box whose kernel class has not changed re-sorts from THOSE, as an MD rebuild does
            // -- nearly sorted input (one integer atomic per run of equal cells instead of one per atom), no second look at the
            // LJAtom array (k_atoms_differ, k_species_collect and their read-back).  Round 4: a reload 4.3 -> 3.7 ms at 10^7
            // atoms.  (Typed boxes are sorted by species, which an edited LJAtom array invalidates: they load afresh.)
            if (rebuild && sys.sorted && sys.nt == 1 && sys.uniform_atoms == was_uniform && !std::getenv("EMDEE_OPERATOR_RELOAD")) {
                sys.resort();
                resorted = true;
            }
        }
        if (rebuild && !resorted) sys.load_user(N, 0, pos, nullptr, atoms, nullptr);
    }
    void stats(int64_t *builds, int64_t *listed, int32_t *max_count, int32_t *capacity) override {
        use_device(sys.ctx);
        sys.list_stats(false, listed, max_count, nullptr);
        if (builds) *builds = sys.builds;
        if (capacity) *capacity = sys.stride;
    }
    void count_pairs(int64_t *pairs) override {
        use_device(sys.ctx);
        sys.list_stats(true, nullptr, nullptr, pairs);
    }
    void export_list(int32_t *counts, int32_t *neighbors, int32_t capacity) override {
        use_device(sys.ctx);
        sys.export_list(counts, neighbors, capacity);
    }
    void set_pairs(const int32_t *pairs, int32_t n_pairs, bool one_four, double lj14scale) override {
        use_device(sys.ctx);
        sys.set_pair_tables(N, pairs, n_pairs, one_four, lj14scale);
    }
};

// ------------------------------------------------------------------------------------ velocity-Verlet
template <typename real>
struct MdImpl : IMd {
    NbSystem<real> sys;
    int n_ghost = 0;
    int since_build = 0;
    int current_mask = 0;   // which of f/e/w match the current positions

    MdImpl(emdee_ctx *c, const double lo[3], const double len[3], const int32_t per[3], const emdee_lj_model &model,
           double skin) {
        sys.ctx = c;
        int p[3] = {per[0], per[1], per[2]};
        sys.set_box(lo, len, p);
        sys.set_model(model, skin);
        sys.with_vel = true;
        sys.image_limit = true;                              // (get_state returns the caller's image)
    }

    void set_state(int n_owned, int ng, const void *pos, const void *vel, const emdee_lj_atom *atoms,
                   const void *inv_mass) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(vel || n_owned == 0, EMDEE_ERR_INVALID, "velocities are NULL");
        n_ghost = ng;
        state_serial++;                                      // (before anything can throw: a state half replaced is another state too)
        sys.load_user(n_owned, ng, (const real *)pos, (const real *)vel, atoms, (const real *)inv_mass, tags_user);
        if (!lent) { sys.reset_bonded_error(); sys.reset_ewald_error(); }   // (a new state: the bonded terms and the struck pairs get another chance; a decomposition resets its own)
        since_build = 0;
        current_mask = 0;
        // (an attached table set for another atom count stays in force, unused, as charges do; for the same count it is checked
        // against the new state, the constraint tables first: their velocities are projected again; then the site table: the sites
        // are placed on their parents with zero velocity and the list is rebuilt for where they now are)
        for (int k = 0; k < TABLES; k++) unchecked[k] = unchecked[k] || (!lent && attached(k).present);   // (every table, before a check can refuse)
        for (int k = 0; k < TABLES; k++) {
            if (lent || !attached(k).present) continue;
            if (k < VSITES) sys.reset_error(sys.groups[k]);
            if (sys.stale(attached(k)) || ng != 0) continue;
            if (k < VSITES) {
                sys.check_state(sys.groups[k]);
                sys.velocities(sys.groups[k]);
            } else if (k == VSITES) {
                sys.check_vsites(sys.tables->vsites);
                sys.place_sites(true);
                sys.resort();
            } else if (k == MOLECULES) {
                sys.check_molecules(sys.tables->molecules);     // (after the constraint tables: their groups must be whole inside it)
            }                                                // (a restraint table asks nothing of the state but its atom count: the references are kept)
            unchecked[k] = false;
        }
        // (charges set for another atom count stay in force, unused: the engine refuses to step until they are set again or
        // cleared -- NbSystem::ensure_charges)
        if (!defer_forces && !sys.charges_stale() && !restraints_unfit() && !pull_unfit() && !alch_unfit()) {
            force_pass(EMDEE_FORCES);
            current_mask = EMDEE_FORCES;
        }
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    // a restraint table set for another atom count (or met by ghosts): it stays in force, unused, and the force pass waits for it to
    // be set again or cleared
    bool restraints_unfit() const { return !lent && sys.has_restraints() && (sys.stale(sys.tables->restraints) || n_ghost != 0); }
    // the same for the pull table (emdee_md_set_pull)
    bool pull_unfit() const { return !lent && sys.has_pull() && (sys.stale(sys.tables->pull) || n_ghost != 0); }
    // the same for the alchemical table (emdee_md_set_alchemical)
    bool alch_unfit() const { return !lent && sys.has_alch() && (sys.stale(sys.tables->alch) || n_ghost != 0); }
    // emdee_dd_step: the rebuild in the middle of a run is followed by a fused step, which evaluates the forces itself
    bool defer_forces = false;
    // The attached tables: one per constraint group (NbSystem::groups, same index), then the table of virtual sites
    // (emdee_md_set_vsites), then the table of position restraints (emdee_md_set_restraints), then the pull table (emdee_md_set_pull), then the molecule table (emdee_md_set_molecules), then the alchemical table (emdee_md_set_alchemical).  Only the state of a table is shared -- present, the atom count it was set for, stale, unchecked, the
    // texts; what is done with one stays per kind.
    enum { VSITES = NbSystem<real>::GROUPS, RESTRAINTS, PULL, MOLECULES, ALCHEMICAL, TABLES };
    const Topology::GroupTable &attached(int k) const {
        if (k == ALCHEMICAL) return sys.tables->alch;
        if (k == MOLECULES) return sys.tables->molecules;
        if (k == PULL) return sys.tables->pull;
        if (k == RESTRAINTS) return sys.tables->restraints;
        return k == VSITES ? sys.tables->vsites : sys.table(sys.groups[k]);
    }
    // what the texts of this file call the entries of table k, and the call that sets it
    struct GroupText { const char *one, *many, *setter; };
    static constexpr GroupText GROUP_TEXT[TABLES] = {{"a rigid molecule", "rigid molecules", "emdee_md_set_rigid3"},
                                                     {"an hbonds cluster", "hbonds clusters", "emdee_md_set_hbonds"},
                                                     {"a virtual site", "virtual sites", "emdee_md_set_vsites"},
                                                     {"a position restraint", "position restraints", "emdee_md_set_restraints"},
                                                     {"a pull group", "pull groups", "emdee_md_set_pull"},
                                                     {"a molecule", "molecules of the molecule table", "emdee_md_set_molecules"},
                                                     {"a flagged atom", "the flags of the alchemical table", "emdee_md_set_alchemical"}};
    // table k has not passed the check against the loaded state (another atom count, ghosts, or a refusal)
    bool unchecked[TABLES] = {false, false, false, false, false, false, false};
    // the conditions emdee_md_step refuses table k on
    void require_fitting(const char *what, int k) const {
        const Topology::GroupTable &t = attached(k);
        EMDEE_REQUIRE(!t.present || !(sys.stale(t) || unchecked[k]), EMDEE_ERR_STATE, "%s: %s set for %lld atoms, the state "
                      "holds %d (or does not fit them): set them again or clear them (%s)", what, GROUP_TEXT[k].many,
                      (long long)t.limit, sys.n_owned, GROUP_TEXT[k].setter);
    }
    // what emdee_md_step and emdee_md_minimize refuse alike: a fault reported before and not yet answered by new tables or a new
    // state, and a table that does not fit the state
    void require_ready(const char *what) const {
        const struct { const FaultWord &fault; const char *text; } reported[] = {
            {sys.bonded_fault, "a bonded term has lost a partner; replace the tables or the state"},
            {sys.ewald_fault, "an excluded or 1-4 pair of an Ewald engine spans more than rc + skin; replace the tables or the state"},
            {sys.image_fault, "an atom has travelled more than 511 box lengths from the box (reported before); replace the state"}};
        for (const auto &r : reported) EMDEE_REQUIRE(!r.fault.latched, EMDEE_ERR_STATE, "%s: %s", what, r.text);
        for (int k = 0; k < TABLES; k++) {
            if (k < VSITES)
                EMDEE_REQUIRE(!sys.groups[k].fault.latched, EMDEE_ERR_STATE, "%s: %s had no solution; replace the table or the state", what, GROUP_TEXT[k].one);
            require_fitting(what, k);
        }
        // (without the Coulomb stage a charged engine's solute carries no charge: its charges are scaled to zero first.  With the stage
        // (emdee_md_set_alchemical_coulomb) the reaction field's cross pairs carry the charge term; under Ewald or PME they do not)
        if (!lent && sys.has_alch() && sys.has_charges()) {
            const int64_t i = alch_first_charged(sys.tables->alch.atoms_h, sys.tables->q_h);
            if (!sys.has_alch_coulomb())
                EMDEE_REQUIRE(i < 0, EMDEE_ERR_STATE, "%s: atom %lld is flagged by the alchemical table (emdee_md_set_alchemical) and carries a charge: "
                              "the soft core covers the Lennard-Jones coupling only; set the solute's charges to zero (emdee_md_set_coulomb) first", what,
                              (long long)i);
            else require_no_recip_solute_charge(what, i);
        }
    }
    // the Coulomb stage covers the pair terms of the reaction field: a charged flagged atom under Ewald or PME is refused with the stage
    // on as it is with the stage off (i: alch_first_charged)
    void require_no_recip_solute_charge(const char *what, int64_t i) const {
        if (!sys.has_ewald()) return;
        const bool pme = sys.ewald.pme.on();
        EMDEE_REQUIRE(i < 0, EMDEE_ERR_STATE, "%s: atom %lld is flagged by the alchemical table and carries a charge: the Coulomb stage "
                      "(emdee_md_set_alchemical_coulomb) covers the reaction field only, not %s (%s); set the solute's charges to zero "
                      "(emdee_md_set_coulomb) or switch the reciprocal sum off first", what, (long long)i,
                      pme ? "particle-mesh Ewald" : "Ewald summation", pme ? "emdee_md_set_pme" : "emdee_md_set_ewald");
    }
    bool sites_in_use() const { return !lent && n_ghost == 0 && sys.vsites_fit() && !unchecked[VSITES]; }
    // A force pass into the engine's own arrays.  With a site table in force, a pass that writes the force planes is followed by the
    // spreading of the sites' forces to their parents (vsite.hpp), once; a pass that leaves the planes alone (energies and virials
    // only, the tensor pass, the interior half of a decomposed step) is not.
    void force_pass(const Pass<real> &p) {
        sys.compute_forces(p);
        if ((p.mask & EMDEE_FORCES) && p.phase != 1 && sites_in_use()) sys.spread_sites();
    }
    void force_pass(int bitmask) { force_pass(Pass<real>::force(bitmask)); }
    // an engine of a decomposition (emdee_dd_engine): its pair tables are the decomposition's, keyed by global id
    bool lent = false;
    // decomposed domains: the global ids of the atoms handed to set_state (caller order, owned atoms and ghosts); they travel
    // with the atoms from then on (NbSystem::tag) and order the atoms of a cell
    const long long *tags_user = nullptr;
    // an engine of an in-process decomposition runs on a stream of the library's own: the context its queries answer to
    // (common.hpp FenceOut; NULL: the engine's context is the caller's)
    const emdee_ctx *caller_ctx = nullptr;
    void get_state(void *pos, void *vel, void *frc, void *en, void *vir) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        // (charges set for another atom count: the state's forces were never evaluated -- refused, as a step is)
        EMDEE_REQUIRE(!((frc || en || vir) && sys.charges_stale()), EMDEE_ERR_STATE, "md: charges set for %lld atoms, the state "
                      "holds %d: set them again or clear them (emdee_md_set_coulomb) before reading forces, energies or virials",
                      (long long)sys.tables->q_n, sys.n_owned);
        if (frc || en || vir) require_fitting("md_get_state (forces, energies or virials)", RESTRAINTS);
        if (frc || en || vir) require_fitting("md_get_state (forces, energies or virials)", PULL);
        if (frc || en || vir) require_fitting("md_get_state (forces, energies or virials)", ALCHEMICAL);
        if ((en || vir) && (current_mask & 6) != 6) forces(7, 0);
        sys.ids_map();                                       // (scratch of the engine's own: before the fence)
        FenceOut fence(caller_ctx, sys.stream());
        sys.unsort((real *)pos, (real *)vel, (real *)frc, (real *)en, (real *)vir);
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void step(int nsteps, double dt, int rebuild_every) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        EMDEE_REQUIRE(n_ghost == 0, EMDEE_ERR_STATE, "md_step needs n_ghost == 0; decomposed runs drive kick_drift/forces/kick");
        EMDEE_REQUIRE(nsteps >= 0 && dt >= 0, EMDEE_ERR_INVALID, "md_step: negative nsteps or dt");
        require_ready("md_step");
        if (nsteps == 0) return;
        // (a restraint, pull or alchemical table: closed steps as well, so that the state after s steps does not depend on how they were dealt to calls)
        if (sys.has_rigid() || sys.has_hbonds() || sys.has_vsites() || sys.has_restraints() || sys.has_pull() || sys.has_alch() ||
            baro.kind != EMDEE_BAROSTAT_OFF ||
            thermo.kind != EMDEE_THERMOSTAT_OFF) {
            step_closed(nsteps, dt, rebuild_every);
            return;
        }
        if (!(current_mask & EMDEE_FORCES)) forces(EMDEE_FORCES, 0);
        // x_1 = x_0 + dt (v_0 + dt/2 f_0); then every inner step is ONE kernel (force + full kick + drift:
        // the closing half kick of step s rides on the opening half kick of step s+1); the last step ends
        // with a plain force pass and the closing half kick.
        sys.kick_drift(0.5 * dt, dt);
        current_mask = 0;                                    // (a call that a rebuild ends early leaves no current forces behind)
        int s = 1;
        if (rebuild_every == 0) {
            // displacement-triggered rebuilds: the inner steps are queued a few at a time (one read-back per
            // batch, NbSystem::fused_steps_run_ahead); same sequence of states as one step at a time
            bool stale = sys.read_rebuild_flag();
            while (s < nsteps) {
                if (stale) { sys.resort(); since_build = 0; }
                const int ran = sys.fused_steps_run_ahead(Pass<real>::step(dt, dt), nsteps - s, &stale);
                if (ran == 0) break;                          // direct kernels: one step at a time below
                s += ran; since_build += ran;
            }
            if (s == nsteps) {
                since_build++;
                if (stale) { sys.resort(); since_build = 0; }
                sys.compute_forces(EMDEE_FORCES);
                s++;
            }
        }
        for (; s <= nsteps; s++) {
            since_build++;
            bool rb = rebuild_every > 0 ? since_build >= rebuild_every : sys.read_rebuild_flag();
            if (rb) { sys.resort(); since_build = 0; }
            if (s == nsteps) {
                sys.compute_forces(EMDEE_FORCES);
            } else if (!sys.fused_step(Pass<real>::step(dt, dt))) {
                sys.compute_forces(EMDEE_FORCES);
                sys.kick_drift(dt, dt);
            }
        }
        sys.kick(0.5 * dt);
        current_mask = EMDEE_FORCES;
        EMDEE_HIP_CHECK(hipGetLastError());
        if (!lent) sys.check_bonded();                       // (one read-back per call, with bonded tables only)
    }
    // ---- pressure coupling (include/emdee_hip.h: emdee_md_scale_box, emdee_md_set_barostat)
    struct Barostat {
        int kind = EMDEE_BAROSTAT_OFF, coupling = EMDEE_COUPLE_ISOTROPIC, every = 1;
        double p_ref[3] = {0, 0, 0}, beta[3] = {0, 0, 0}, tau_p = 1.0, temperature = 0.0;
        unsigned long long seed = 0, step = 0;               // step: how many steps have been taken, counted from first_step
    } baro;
    DevBuf<long long> baro_id;                               // the id -1 of the coupling's random number (C-rescale)
    DevBuf<double> baro_xi;
    void get_box(double lo[3], double len[3]) override {
        for (int d = 0; d < 3; d++) { lo[d] = sys.lo[d]; len[d] = sys.len[d]; }
    }
    void require_undivided(const char *what) const {
        EMDEE_REQUIRE(!lent, EMDEE_ERR_STATE, "%s: this integrator is a domain's, lent by emdee_dd_engine (the geometry of a decomposition is fixed at create)", what);
        EMDEE_REQUIRE(n_ghost == 0 && !sys.has_ghosts, EMDEE_ERR_STATE, "%s: an integrator with ghosts (its box is a domain of a larger one)", what);
    }
    // emdee_md_set_molecular_scaling: an engine with a rigid table or a molecule table scales by molecular centres and couples to the
    // molecular pressure
    bool molecular = false;
    // The one predicate for "this engine may be pressure-coupled" (scaled, coupled, asked for its molecular pressure): it holds no
    // constraint table, or the switch is on and either a molecule table covers the groups (the setters see to that) or the engine is
    // rigid-only, whose molecules the Triangle kernels take from the rigid table.  on, table: the switch and whether a molecule table
    // is in force, as they are or as a call is about to leave them.
    bool couplable(bool on, bool table) const { return (!sys.has_rigid() && !sys.has_hbonds()) || (on && (table || !sys.has_hbonds())); }
    bool couplable() const { return couplable(molecular, sys.has_molecules()); }
    // the molecular entries take molecules from a table: the molecule table in force, else the rigid table
    bool by_molecules() const { return sys.molecule_table() != nullptr || sys.has_rigid(); }
    void set_molecular_scaling(int32_t on) override {
        EMDEE_REQUIRE(on == 0 || on == 1, EMDEE_ERR_INVALID, "set_molecular_scaling: on = %d is neither 0 nor 1", on);
        require_undivided("set_molecular_scaling");
        if (baro.kind != EMDEE_BAROSTAT_OFF && !couplable(on == 1, sys.has_molecules())) {
            EMDEE_REQUIRE(!sys.has_rigid(), EMDEE_ERR_STATE, "set_molecular_scaling: pressure coupling is on "
                          "and the engine holds rigid molecules: switch the coupling off (emdee_md_set_barostat) or clear the table (emdee_md_set_rigid3) first");
            EMDEE_REQUIRE(false, EMDEE_ERR_STATE, "set_molecular_scaling: pressure coupling is on and the engine holds an hbonds table: switch the "
                          "coupling off (emdee_md_set_barostat) or clear the table (emdee_md_set_hbonds) first");
        }
        molecular = on == 1;
        sys.molecules_on = molecular;
    }
    void scale_box(const double mu[3], double vscale) override {
        use_device(sys.ctx);
        require_undivided("scale_box");
        if (!couplable()) {
            EMDEE_REQUIRE(!sys.has_hbonds(), EMDEE_ERR_STATE, "scale_box: the engine holds an hbonds table (emdee_md_set_hbonds): scaling atom by atom would "
                          "break its bonds, and the molecular scale is written for three-site molecules; clear the table first");
            EMDEE_REQUIRE(false, EMDEE_ERR_STATE, "scale_box: the engine holds rigid molecules (emdee_md_set_rigid3): scaling atom by atom "
                          "would break their geometry, and its pressure lacks the constraint virial (emdee_md_set_molecular_scaling scales by molecular centres)");
        }
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "scale_box: no state loaded (call emdee_md_set_state first)");
        require_fitting("scale_box", sys.RIGID);
        require_fitting("scale_box", sys.HBONDS);
        require_fitting("scale_box", VSITES);
        require_fitting("scale_box", RESTRAINTS);
        require_fitting("scale_box", PULL);                  // (xi0 and r0 do not scale with the box)
        require_fitting("scale_box", ALCHEMICAL);
        if (molecular) require_fitting("scale_box", MOLECULES);
        sys.scale_box(mu, vscale, by_molecules());           // (validates before it writes; sites go back on their scaled parents)
        since_build = 0;
        current_mask = 0;
        if (!sys.charges_stale()) {
            force_pass(EMDEE_FORCES);
            current_mask = EMDEE_FORCES;
        }
        EMDEE_HIP_CHECK(hipGetLastError());
        sys.check_bonded();
    }
    void set_barostat(int32_t kind, int32_t coupling, const double *p_ref, const double *beta, double tau_p, int32_t every,
                      double temperature, uint64_t seed, uint64_t first_step) override {
        use_device(sys.ctx);
        require_undivided("set_barostat");
        if (kind != EMDEE_BAROSTAT_OFF && !couplable()) {
            EMDEE_REQUIRE(!sys.has_hbonds(), EMDEE_ERR_STATE, "set_barostat: the engine holds an hbonds table "
                          "(emdee_md_set_hbonds): its pressure lacks the clusters' constraint virial, and the molecular sums are written for "
                          "three-site molecules; clear the table first");
            EMDEE_REQUIRE(false, EMDEE_ERR_STATE, "set_barostat: the engine holds rigid molecules "
                          "(emdee_md_set_rigid3): its pressure lacks the constraint virial, and scaling atom by atom would break their geometry "
                          "(emdee_md_set_molecular_scaling couples to the molecular pressure)");
        }
        if (kind == EMDEE_BAROSTAT_OFF) { baro.kind = EMDEE_BAROSTAT_OFF; return; }
        EMDEE_REQUIRE(kind == EMDEE_BAROSTAT_BERENDSEN || kind == EMDEE_BAROSTAT_CRESCALE, EMDEE_ERR_INVALID, "set_barostat: unknown kind %d", kind);
        EMDEE_REQUIRE(coupling >= EMDEE_COUPLE_ISOTROPIC && coupling <= EMDEE_COUPLE_ANISOTROPIC, EMDEE_ERR_INVALID, "set_barostat: unknown coupling %d", coupling);
        EMDEE_REQUIRE(kind != EMDEE_BAROSTAT_CRESCALE || coupling == EMDEE_COUPLE_ISOTROPIC, EMDEE_ERR_INVALID,
                      "set_barostat: stochastic cell rescaling is isotropic only");
        EMDEE_REQUIRE(p_ref && beta, EMDEE_ERR_INVALID, "set_barostat: p_ref or compressibility is NULL");
        EMDEE_REQUIRE(every >= 1, EMDEE_ERR_INVALID, "set_barostat: every = %d must be >= 1", every);
        EMDEE_REQUIRE(std::isfinite(tau_p) && tau_p > 0.0, EMDEE_ERR_INVALID, "set_barostat: tau_p must be finite and > 0");
        for (int d = 0; d < 3; d++) {
            EMDEE_REQUIRE(std::isfinite(p_ref[d]), EMDEE_ERR_INVALID, "set_barostat: p_ref[%d] is not finite", d);
            EMDEE_REQUIRE(std::isfinite(beta[d]) && beta[d] >= 0.0, EMDEE_ERR_INVALID, "set_barostat: compressibility[%d] must be finite and >= 0", d);
        }
        EMDEE_REQUIRE(kind != EMDEE_BAROSTAT_CRESCALE || (std::isfinite(temperature) && temperature > 0.0), EMDEE_ERR_INVALID,
                      "set_barostat: stochastic cell rescaling needs a temperature > 0");
        if (kind == EMDEE_BAROSTAT_CRESCALE) {
            baro_xi.ensure(3);
            if (baro_id.ensure(1)) EMDEE_HIP_CHECK(hipMemsetAsync(baro_id.ptr, 0xff, sizeof(long long), sys.stream()));
        }
        // ---- commit
        baro.kind = kind; baro.coupling = coupling; baro.every = every; baro.tau_p = tau_p; baro.temperature = temperature;
        baro.seed = seed; baro.step = first_step;
        for (int d = 0; d < 3; d++) { baro.p_ref[d] = p_ref[d]; baro.beta[d] = beta[d]; }
    }
    // One closed step: the one place the sequence of stages lives, for emdee_md_step with a table or a barostat (step_closed) and
    // for emdee_md_minimize.  It closes its own half kick (kick + drift, force pass, kick): the state after s steps then does not
    // depend on how the s steps were dealt to calls -- step(40), 8 x step(5) and 40 x step(1) are the same sequence of launches,
    // bit for bit -- and no step is ever queued beyond an event on the box the event is about to change.  (The merged kicks and
    // the guarded run-ahead of the uncoupled loop would have to end at every call as well as at every event, and v + h + h is
    // not v + 2 h in floating point.)
    // Around the unchanged kernels, the three constraint stages of every table that exists (NbSystem::groups: SETTLE / RATTLE on
    // the molecules, then M-SHAKE / RATTLE on the clusters, whose atoms are disjoint): (a) the constrained atoms' positions are
    // remembered, (c) the distances are restored on the drifted records, (e) the bond components of the relative velocities are
    // removed.  Stage (c) re-tests its atoms against the rebuild threshold, so the displacement word is read after it; a re-sort
    // between (c) and (e) is harmless (the stages find atoms through inv_perm).
    // Virtual sites (emdee_md_set_vsites) add two stages: (c') the sites are put back on their parents after stage (c) of every table
    // (they raise the same displacement word), (d') their forces are spread to the parents between the force pass and the kick.
    // The order: (a) gather, (b) kick + drift, (c) positions, (c') place sites, [re-sort], (d) force pass, (d') spread, kick,
    // (e) velocities.  mask: the outputs of the force pass; rebuild_every: the cadence of the re-sort, 0 for the displacement
    // word.  Returns whether it re-sorted.
    bool closed_step(double dt, int mask, int rebuild_every) {
        sys.for_each_table([&](auto &g) { sys.gather(g); });
        sys.kick_drift(0.5 * dt, dt);
        current_mask = 0;                                    // (as in step(): until the force pass of this step)
        sys.for_each_table([&](auto &g) { sys.positions(g, dt); });
        if (sites_in_use()) sys.place_sites(false);          // (c'): after every constraint table's stage (c), before the word is read
        since_build++;
        const bool rb = rebuild_every > 0 ? since_build >= rebuild_every : sys.read_rebuild_flag();
        if (rb) { sys.resort(); since_build = 0; }
        force_pass(mask);                                    // ((d'): the sites' forces go to their parents before the closing kick)
        sys.kick(0.5 * dt);
        sys.for_each_table([&](auto &g) { sys.velocities(g); });
        current_mask = mask;
        return rb;
    }
    // what a call that ran closed steps ends with: the faults its kernels may have raised
    void check_closed_steps() {
        EMDEE_HIP_CHECK(hipGetLastError());
        sys.check_bonded();                                  // (one read-back per call, with bonded tables only)
        for (auto &g : sys.groups) sys.check(g);             // (one read-back per call and table)
    }
    // emdee_md_step with coupling on, with rigid molecules (emdee_md_set_rigid3), an hbonds table (emdee_md_set_hbonds), virtual
    // sites or position restraints (emdee_md_set_restraints): closed steps and, with pressure coupling on, after the step that completes an interval, (f) the event.  Without a
    // table the event's step evaluates the energies and virials with its forces when the coupling is isotropic: no pass is added
    // for the pressure.  With rigid molecules (emdee_md_set_molecular_scaling) the event takes the molecular pressure from that
    // step's forces F(x) and its stage-(e) velocities (one tensor pass), then the molecular scale, which rebuilds the list and
    // evaluates the forces on the new box; a fixed rebuild cadence restarts from the event.  A molecule table in force
    // (emdee_md_set_molecules) couples the same way, hbonds clusters included: its molecules take the place of the rigid table's.
    // A global thermostat (emdee_md_set_thermostat) sends the call here as well: after the step that completes one of its
    // intervals, (e') K, the scalar update and v <- alpha v, before (f).  It lives here and not in closed_step, so that
    // emdee_md_minimize runs without it.
    void step_closed(int nsteps, double dt, int rebuild_every) {
        const bool coupled = baro.kind != EMDEE_BAROSTAT_OFF, rigid = sys.has_rigid(), hbonds = sys.has_hbonds();
        EMDEE_REQUIRE(!coupled || !(rigid || hbonds) || molecular, EMDEE_ERR_STATE, "md_step: pressure coupling with rigid molecules needs emdee_md_set_molecular_scaling");
        EMDEE_REQUIRE(!coupled || couplable(), EMDEE_ERR_STATE, "md_step: pressure coupling with an hbonds table (emdee_md_set_hbonds)");
        const bool with_sums = !by_molecules() && baro.coupling == EMDEE_COUPLE_ISOTROPIC;
        const bool thermostatted = thermo.kind != EMDEE_THERMOSTAT_OFF;
        const long long n_dof = thermostatted ? degrees_of_freedom() : 0;
        EMDEE_REQUIRE(!thermostatted || n_dof >= 3, EMDEE_ERR_STATE, "md_step: the thermostat (emdee_md_set_thermostat) finds %lld degrees of "
                      "freedom in the state and its tables; it needs at least 3", n_dof);
        if (!(current_mask & EMDEE_FORCES)) forces(EMDEE_FORCES, 0);
        for (int s = 0; s < nsteps; s++) {
            const bool event = coupled && (baro.step + 1) % (unsigned long long)baro.every == 0;
            if (sys.has_pull()) sys.own_tables.pull.advance(dt);   // (xi0 <- xi0 + rate dt on the host; the step's force pass closes it: work, log)
            if (sys.has_alch()) sys.own_tables.alch.advance();     // (the step's force pass writes the log entry that is due)
            closed_step(dt, (event && with_sums) ? 7 : EMDEE_FORCES, rebuild_every);
            if (thermostatted && ++thermo.step % (unsigned long long)thermo.every == 0) thermostat_event(dt, n_dof);
            if (coupled) baro.step++;
            if (event) couple(dt);
        }
        check_closed_steps();
    }
    // ---- global thermostats (include/emdee_hip.h: emdee_md_set_thermostat; thermostat.hpp)
    struct Thermostat {
        int kind = EMDEE_THERMOSTAT_OFF, every = 1, chain = 3;
        double temperature = 0.0, tau_t = 1.0;
        long long n_dof = 0;                                 // 0: the library's own count
        unsigned long long seed = 0, step = 0;               // step: how many steps have been taken, counted from first_step
    } thermo;
    // the count a thermostat works with: the one given, or 3 (n_owned - n_sites) - 3 n_rigid - n_satellites - 3 from the tables in force
    long long degrees_of_freedom() const {
        if (thermo.n_dof > 0) return thermo.n_dof;
        const Topology &t = *sys.tables;
        long long n = 3LL * ((long long)sys.n_owned - (t.vsites.present ? t.vsites.n : 0)) - 3;
        if (t.rigid.present) n -= 3LL * t.rigid.n;
        if (t.hbonds.present)
            for (size_t k = 0; k < t.hbonds.atoms_h.size(); k++) n -= (k % 4 != 0 && t.hbonds.atoms_h[k] >= 0) ? 1 : 0;
        return n;
    }
    // stage (e') of an event step: after stage (e) of the closed step, before the barostat's event (f).  One application over
    // Delta = every dt; three launches on the engine's stream (NbSystem::thermostat_event), nothing read back.
    void thermostat_event(double dt, long long n_dof) {
        ThermostatParams p{};
        p.kind = thermo.kind; p.chain = thermo.chain; p.kT = thermo.temperature; p.tau = thermo.tau_t;
        p.Delta = (double)thermo.every * dt; p.n_dof = (double)n_dof; p.seed = thermo.seed; p.step = thermo.step;
        sys.thermostat_event(p);
    }
    void set_thermostat(int32_t kind, double temperature, double tau_t, int32_t every, int64_t n_dof, int32_t chain, uint64_t seed,
                        uint64_t first_step) override {
        use_device(sys.ctx);
        require_undivided("set_thermostat");
        EMDEE_REQUIRE(kind >= EMDEE_THERMOSTAT_OFF && kind <= EMDEE_THERMOSTAT_NOSE_HOOVER, EMDEE_ERR_INVALID, "set_thermostat: unknown kind %d", kind);
        if (kind == EMDEE_THERMOSTAT_OFF) { thermo.kind = EMDEE_THERMOSTAT_OFF; return; }
        EMDEE_REQUIRE(std::isfinite(temperature) && temperature > 0.0, EMDEE_ERR_INVALID, "set_thermostat: temperature must be finite and > 0");
        EMDEE_REQUIRE(std::isfinite(tau_t) && tau_t > 0.0, EMDEE_ERR_INVALID, "set_thermostat: tau_t must be finite and > 0");
        EMDEE_REQUIRE(every >= 1, EMDEE_ERR_INVALID, "set_thermostat: every = %d must be >= 1", every);
        EMDEE_REQUIRE(n_dof >= 0, EMDEE_ERR_INVALID, "set_thermostat: n_dof = %lld is negative (0: the library's own count)", (long long)n_dof);
        EMDEE_REQUIRE(kind != EMDEE_THERMOSTAT_NOSE_HOOVER || (chain >= 1 && chain <= TH_CHAIN_MAX), EMDEE_ERR_INVALID,
                      "set_thermostat: chain = %d is outside 1...%d", chain, TH_CHAIN_MAX);
        EMDEE_REQUIRE(!sys.lgv_on, EMDEE_ERR_STATE, "set_thermostat: the Langevin thermostat is on (emdee_md_set_langevin with gamma > 0): switch it off first");
        double *w = sys.thermostat_words();
        EMDEE_HIP_CHECK(hipMemsetAsync(w, 0, TH_WORDS * sizeof(double), sys.stream()));
        // ---- commit
        thermo.kind = kind; thermo.every = every; thermo.chain = kind == EMDEE_THERMOSTAT_NOSE_HOOVER ? chain : 0;
        thermo.temperature = temperature; thermo.tau_t = tau_t; thermo.n_dof = n_dof; thermo.seed = seed; thermo.step = first_step;
    }
    // blocking: the twenty words; word 0 is the count the next step would use while a thermostat is on and a state is loaded
    void thermostat_state(double *out) override {
        use_device(sys.ctx);
        sys.read_back_doubles(out, sys.thermostat_words(), TH_WORDS);
        if (thermo.kind != EMDEE_THERMOSTAT_OFF && (thermo.n_dof > 0 || sys.sorted)) out[TH_NDOF] = (double)degrees_of_freedom();
    }
    void set_thermostat_state(const double *in) override {
        use_device(sys.ctx);
        require_undivided("set_thermostat_state");
        for (int k = TH_ETH; k < TH_WORDS; k++)
            EMDEE_REQUIRE(std::isfinite(in[k]), EMDEE_ERR_INVALID, "set_thermostat_state: word %d is not finite", k);
        double *w = sys.thermostat_words();
        EMDEE_HIP_CHECK(hipMemcpyAsync(w + TH_ETH, in + TH_ETH, (TH_WORDS - TH_ETH) * sizeof(double), hipMemcpyHostToDevice, sys.stream()));
        EMDEE_HIP_CHECK(hipStreamSynchronize(sys.stream()));  // (the caller's array is its own again on return)
    }
    void thermostat_draws(uint64_t seed, uint64_t step, int64_t n_dof, double *out) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(n_dof >= 1, EMDEE_ERR_INVALID, "thermostat_draws: n_dof = %lld must be >= 1", (long long)n_dof);
        double *part = sys.red_partials();                   // (scratch of the box sums, which the stream orders)
        hipLaunchKernelGGL(k_thermostat_draws, dim3(1), dim3(64), 0, sys.stream(), (unsigned long long)seed, (unsigned long long)step,
                           (long long)n_dof, part);
        EMDEE_HIP_CHECK(hipGetLastError());
        sys.read_back_doubles(out, part, 2);
    }
    // ---- the observables (include/emdee_hip.h: emdee_md_set_rdf, emdee_md_set_msd, emdee_md_set_gk, emdee_md_set_spatial).  A table is one
    // record, host fields and device buffers together, and the refusals the three share are formed once (observables.hpp).  Every
    // setter is all or nothing and blocking: it builds a candidate record and queues its uploads, every refusal -- a failed
    // allocation included -- comes before the table in force changes, and install() swaps the candidate in whole.  Clearing puts
    // an empty record in.  A sample is queued on the stream, nothing read back; the engine's state, list and counters are not
    // touched, and a refusal changes nothing.  A read is blocking, and any of its pointers may be NULL.
    RdfRecord rdf;
    MsdRecord msd;
    GkRecord gk;
    uint64_t state_serial = 0;                               // counts emdee_md_set_state: a snapshot of one state is no origin for another
    ObsEngine obs_engine() const {
        return ObsEngine{lent, sys.has_ghosts, sys.sorted, sys.id_gaps, sys.n_owned, n_ghost, {sys.len[0], sys.len[1], sys.len[2]}, state_serial};
    }
    double shortest_side() const { return std::min(sys.len[0], std::min(sys.len[1], sys.len[2])); }
    // behind the candidate's uploads (the caller's arrays and this call's are their own again, the table in force is idle)
    template <class Record>
    void install(Record &in_force, Record &candidate) {
        EMDEE_HIP_CHECK(hipStreamSynchronize(sys.stream()));
        in_force = std::move(candidate);
        in_force.zero(sys.stream(), obs_engine());
        EMDEE_HIP_CHECK(hipStreamSynchronize(sys.stream()));
    }
    template <class Record>
    void reset(ObsKind kind, Record &t) {
        use_device(sys.ctx);
        obs_require_present(kind, "reset", t);
        t.zero(sys.stream(), obs_engine());
    }
    // a caller's array of one entry per owned atom, on the host
    std::vector<int32_t> fetched(const int32_t *dev) {
        std::vector<int32_t> host((size_t)sys.n_owned);
        if (!host.empty()) EMDEE_HIP_CHECK(hipMemcpyAsync(host.data(), dev, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, sys.stream()));
        EMDEE_HIP_CHECK(hipStreamSynchronize(sys.stream()));
        return host;
    }
    // ... a setter's group array, checked; empty where the caller gave none
    std::vector<int32_t> fetched_groups(ObsKind kind, const int32_t *dev, int n_groups) {
        EMDEE_REQUIRE(dev || n_groups == 1, EMDEE_ERR_INVALID, "%s: groups is NULL with n_groups = %d (NULL puts every atom in group 0)", OBS_TEXT[kind].set, n_groups);
        std::vector<int32_t> host = dev ? fetched(dev) : std::vector<int32_t>();
        obs_check_groups(kind, host.data(), (int)host.size(), n_groups);
        return host;
    }
    // ---- radial distribution functions (rdf.hpp)
    void set_rdf(double r_max, int32_t n_bins, int32_t n_groups, const int32_t *group_dev, const int32_t *molecule_dev) override {
        use_device(sys.ctx);
        if (n_bins == 0) { rdf = RdfRecord{}; return; }
        obs_require_whole_box("set_rdf", obs_engine());
        EMDEE_REQUIRE(sys.per[0] && sys.per[1] && sys.per[2], EMDEE_ERR_STATE, "set_rdf: the box has an open axis; the minimum image needs three periodic ones");
        EMDEE_REQUIRE(n_groups >= 1 && n_groups <= RDF_MAX_GROUPS, EMDEE_ERR_INVALID, "set_rdf: n_groups = %d is outside 1...%d", n_groups, RDF_MAX_GROUPS);
        EMDEE_REQUIRE(n_bins >= 1, EMDEE_ERR_INVALID, "set_rdf: n_bins = %d must be >= 1 (0 clears the table)", n_bins);
        EMDEE_REQUIRE((long long)rdf_n_pairs(n_groups) * n_bins <= RDF_MAX_COUNTERS, EMDEE_ERR_INVALID, "set_rdf: %d histograms of %d bins are %lld "
                      "counters, above the limit of %d (a workgroup's histogram in LDS)", rdf_n_pairs(n_groups), n_bins,
                      (long long)rdf_n_pairs(n_groups) * n_bins, RDF_MAX_COUNTERS);
        EMDEE_REQUIRE(std::isfinite(r_max) && r_max > 0.0, EMDEE_ERR_INVALID, "set_rdf: r_max must be finite and > 0");
        EMDEE_REQUIRE(r_max <= 0.5 * shortest_side(), EMDEE_ERR_INVALID, "set_rdf: r_max = %g exceeds half the shortest box side %g (minimum image)",
                      r_max, shortest_side());
        const int n = sys.n_owned;
        RdfRecord t;
        t.present = true; t.grouped = group_dev != nullptr; t.with_mol = molecule_dev != nullptr;
        t.n_atoms = n; t.n_bins = n_bins; t.n_groups = n_groups; t.r_max = r_max; t.inv_dr = (double)n_bins / r_max;
        t.sizes[0] = t.grouped ? 0 : n;
        for (int32_t g : fetched_groups(OBS_RDF, group_dev, n_groups))
            if (g >= 0) t.sizes[g]++;
        if (t.with_mol) {
            const std::vector<int32_t> host = fetched(molecule_dev);
            for (int i = 0; i < n; i++)
                EMDEE_REQUIRE(host[i] >= -1, EMDEE_ERR_INVALID, "set_rdf: the molecule %d of atom %d is below -1 (-1: none)", host[i], i);
        }
        t.group.ensure((size_t)n + 1); t.mol.ensure((size_t)n + 1);
        t.counts.ensure((size_t)t.n_counters());
        if (t.grouped && n > 0) EMDEE_HIP_CHECK(hipMemcpyAsync(t.group.ptr, group_dev, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, sys.stream()));
        if (t.with_mol && n > 0) EMDEE_HIP_CHECK(hipMemcpyAsync(t.mol.ptr, molecule_dev, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, sys.stream()));
        install(rdf, t);
    }
    void rdf_sample() override {
        use_device(sys.ctx);
        obs_require_present(OBS_RDF, "sample", rdf);
        obs_require_fit(OBS_RDF, rdf, obs_engine());
        EMDEE_REQUIRE(rdf.r_max <= 0.5 * shortest_side(), EMDEE_ERR_STATE, "rdf_sample: the box has shrunk: r_max = %g now exceeds half the shortest "
                      "side %g; set the table again with a smaller r_max", rdf.r_max, shortest_side());
        sys.rdf_sample(rdf_plan(sys.len, rdf.r_max, sys.n_owned), rdf);
        EMDEE_HIP_CHECK(hipGetLastError());
        rdf.samples++;
        rdf.inv_volume_sum += 1.0 / (sys.len[0] * sys.len[1] * sys.len[2]);
    }
    void rdf_read(int64_t *counts, int64_t *group_sizes, int64_t *frames, double *inv_volume_sum) override {
        use_device(sys.ctx);
        obs_require_present(OBS_RDF, "read", rdf);
        if (counts) {
            EMDEE_HIP_CHECK(hipMemcpyAsync(counts, rdf.counts.ptr, (size_t)rdf.n_counters() * sizeof(int64_t), hipMemcpyDeviceToHost, sys.stream()));
            EMDEE_HIP_CHECK(hipStreamSynchronize(sys.stream()));
        }
        if (group_sizes) for (int a = 0; a < RDF_MAX_GROUPS; a++) group_sizes[a] = rdf.sizes[a];
        if (frames) *frames = rdf.samples;
        if (inv_volume_sum) *inv_volume_sum = rdf.inv_volume_sum;
    }
    void rdf_reset() override { reset(OBS_RDF, rdf); }
    // ---- mean-squared displacement and velocity autocorrelation (msd.hpp)
    void set_msd(int32_t what, int32_t n_groups, const int32_t *group_dev, int32_t n_lags, int32_t origin_every) override {
        use_device(sys.ctx);
        if (n_lags == 0) { msd = MsdRecord{}; return; }
        obs_require_whole_box("set_msd", obs_engine());
        EMDEE_REQUIRE(what >= 1 && what <= (MSD_POSITIONS | MSD_VELOCITIES), EMDEE_ERR_INVALID, "set_msd: what = %d is not a non-empty mask of "
                      "EMDEE_MSD | EMDEE_VACF", what);
        EMDEE_REQUIRE(n_groups >= 1 && n_groups <= MSD_MAX_GROUPS, EMDEE_ERR_INVALID, "set_msd: n_groups = %d is outside 1...%d", n_groups, MSD_MAX_GROUPS);
        EMDEE_REQUIRE(n_lags >= 1 && n_lags <= MSD_MAX_LAGS, EMDEE_ERR_INVALID, "set_msd: n_lags = %d is outside 1...%d (0 clears the table)", n_lags, MSD_MAX_LAGS);
        EMDEE_REQUIRE(origin_every >= 1, EMDEE_ERR_INVALID, "set_msd: origin_every = %d must be >= 1", origin_every);
        EMDEE_REQUIRE(msd_n_origins(n_lags, origin_every) <= MSD_MAX_ORIGINS, EMDEE_ERR_INVALID, "set_msd: %d lags with an origin every %d samples "
                      "are %d origins in the ring, above the limit of %d", n_lags, origin_every, msd_n_origins(n_lags, origin_every), MSD_MAX_ORIGINS);
        const int n = sys.n_owned;
        const std::vector<int32_t> host = fetched_groups(OBS_MSD, group_dev, n_groups);
        const MsdLayout lay = msd_layout(group_dev ? host.data() : nullptr, n, n_groups);
        MsdRecord t;
        t.present = true; t.what = what; t.n_atoms = n; t.n_groups = n_groups; t.n_lags = n_lags; t.origin_every = origin_every;
        t.n_origins = msd_n_origins(n_lags, origin_every); t.n_grouped = lay.n_grouped; t.n_chunks = (int)lay.chunks.size();
        for (int g = 0; g < MSD_MAX_GROUPS; g++) t.sizes[g] = lay.sizes[g];
        t.pos_of.ensure((size_t)n + 1); t.chunk_of_group.ensure(MSD_MAX_GROUPS + 1); t.chunks.ensure(lay.chunks.size() + 1);
        t.ring.ensure((size_t)(t.n_origins + 1) * t.snapshot() + 1);
        t.partial.ensure((size_t)t.n_origins * lay.chunks.size() * MSD_WORDS + 1);
        t.sums.ensure(t.n_sums());
        if (n > 0) EMDEE_HIP_CHECK(hipMemcpyAsync(t.pos_of.ptr, lay.pos_of.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, sys.stream()));
        EMDEE_HIP_CHECK(hipMemcpyAsync(t.chunk_of_group.ptr, lay.chunk_of_group, sizeof(lay.chunk_of_group), hipMemcpyHostToDevice, sys.stream()));
        if (!lay.chunks.empty())
            EMDEE_HIP_CHECK(hipMemcpyAsync(t.chunks.ptr, lay.chunks.data(), lay.chunks.size() * sizeof(MsdChunk), hipMemcpyHostToDevice, sys.stream()));
        install(msd, t);
    }
    void msd_sample() override {
        use_device(sys.ctx);
        obs_require_present(OBS_MSD, "sample", msd);
        obs_require_fit(OBS_MSD, msd, obs_engine());
        MsdArgs a{};
        a.what = msd.what; a.n_grouped = msd.n_grouped; a.n_chunks = msd.n_chunks; a.n_groups = msd.n_groups; a.n_lags = msd.n_lags;
        a.origin_every = msd.origin_every; a.s = msd.samples; a.snapshot = msd.snapshot();
        const MsdSchedule q = msd_schedule(msd.samples, msd.n_lags, msd.origin_every);
        sys.msd_sample(a, q.is_origin ? q.slot : -1, msd);
        EMDEE_HIP_CHECK(hipGetLastError());
        for (const MsdLive &l : q.live) msd.origins[(size_t)l.lag]++;
        msd.samples++;
    }
    void msd_read(double *sums, int64_t *origins, int64_t *group_sizes, int64_t *samples) override {
        use_device(sys.ctx);
        obs_require_present(OBS_MSD, "read", msd);
        if (sums) sys.read_back_doubles(sums, msd.sums.ptr, (int)msd.n_sums());
        if (origins) for (int l = 0; l < msd.n_lags; l++) origins[l] = msd.origins[(size_t)l];
        if (group_sizes) for (int g = 0; g < MSD_MAX_GROUPS; g++) group_sizes[g] = msd.sizes[g];
        if (samples) *samples = msd.samples;
    }
    void msd_reset() override { reset(OBS_MSD, msd); }
    // ---- Green-Kubo observables: the stress and heat-flux autocorrelations (gk.hpp)
    // what the engine must be for a table with this mask, at set and again at every sample (a table may be attached later)
    void require_gk(const char *fn, int what) const {
        obs_require_whole_box(fn, obs_engine());
        EMDEE_REQUIRE(!sys.has_hbonds(), EMDEE_ERR_STATE, "%s: the engine holds an hbonds table (emdee_md_set_hbonds): neither the atomic nor the "
                      "molecular stress holds the clusters' constraint virial; clear the table first", fn);
        if (!(what & GK_HEAT)) return;
        // (the per-atom energies and tensors are the half-pair split of the neighbour rows' terms only)
        const bool pme = sys.has_ewald() && sys.ewald.pme.on();
        const struct { bool on; const char *text; } other[] = {
            {sys.has_excl(), "excluded pairs (emdee_md_set_exclusions)"},
            {sys.has_14(), "scaled 1-4 pairs (emdee_md_set_pairs14)"},
            {sys.has_bonded(), "bonded terms (emdee_md_set_bonded)"},
            {sys.has_rigid(), "rigid molecules (emdee_md_set_rigid3)"},
            {sys.has_vsites(), "virtual sites (emdee_md_set_vsites)"},
            {sys.has_restraints(), "position restraints (emdee_md_set_restraints)"},
            {sys.has_pull(), "a centre-of-mass pull (emdee_md_set_pull)"},
            {sys.has_alch(), "an alchemical table (emdee_md_set_alchemical)"},
            {pme, "particle-mesh Ewald (emdee_md_set_pme)"},
            {sys.has_ewald() && !pme, "Ewald summation (emdee_md_set_ewald)"}};
        std::string all;                                     // (every table in the way, so that one refusal says what to clear)
        for (const auto &o : other)
            if (o.on) all += (all.empty() ? "" : ", ") + std::string(o.text);
        EMDEE_REQUIRE(all.empty(), EMDEE_ERR_STATE, "%s: EMDEE_GK_HEAT on an engine with %s: the heat flux is written for forces that are all "
                      "pair terms of the neighbour rows, whose per-atom tensors are the half-pair split", fn, all.c_str());
    }
    void set_gk(int32_t what, int32_t n_lags) override {
        use_device(sys.ctx);
        if (n_lags == 0) { gk = GkRecord{}; return; }
        EMDEE_REQUIRE(what >= 1 && what <= (GK_STRESS | GK_HEAT), EMDEE_ERR_INVALID, "set_gk: what = %d is not a non-empty mask of "
                      "EMDEE_GK_STRESS | EMDEE_GK_HEAT", what);
        EMDEE_REQUIRE(n_lags >= 1 && n_lags <= GK_MAX_LAGS, EMDEE_ERR_INVALID, "set_gk: n_lags = %d is outside 1...%d (0 clears the table)", n_lags, GK_MAX_LAGS);
        require_gk("set_gk", what);
        GkRecord t;
        t.present = true; t.what = what; t.n_atoms = sys.n_owned; t.n_lags = n_lags;
        t.ring.ensure(t.ring_words());
        t.acc.ensure(t.acc_words());
        install(gk, t);
    }
    // one sample: the forces (a rigid engine) and the tensor pass if they are not current, as the pressure entries evaluate them, then
    // the sample's own launches
    void gk_sample() override {
        use_device(sys.ctx);
        obs_require_present(OBS_GK, "sample", gk);
        require_gk("gk_sample", gk.what);
        obs_require_fit(OBS_GK, gk, obs_engine());
        EMDEE_REQUIRE(!sys.charges_stale(), EMDEE_ERR_STATE, "gk_sample: charges set for %lld atoms, the state holds %d: set them again or clear "
                      "them (emdee_md_set_coulomb)", (long long)sys.tables->q_n, sys.n_owned);
        const bool molecular = sys.molecular_groups() > 0;
        if (sys.molecules_on) require_fitting("gk_sample", MOLECULES);
        if (by_molecules()) {
            require_fitting("gk_sample", sys.RIGID);
            if (!(current_mask & EMDEE_FORCES)) forces(EMDEE_FORCES, 0);
        }
        tensor_pass();
        sys.gk_sample(gk, molecular);
        EMDEE_HIP_CHECK(hipGetLastError());
        gk.samples++;
    }
    // the deferred fault word of the bonded terms is checked here, not in the sample
    void gk_read(double *sums, double *totals, double *last, int64_t *samples) override {
        use_device(sys.ctx);
        obs_require_present(OBS_GK, "read", gk);
        sys.check_bonded();
        const size_t n = gk.ring_words();
        if (sums) EMDEE_HIP_CHECK(hipMemcpyAsync(sums, gk.acc.ptr, n * sizeof(double), hipMemcpyDeviceToHost, sys.stream()));
        if (totals) EMDEE_HIP_CHECK(hipMemcpyAsync(totals, gk.acc.ptr + n, GK_WORDS * sizeof(double), hipMemcpyDeviceToHost, sys.stream()));
        if (last) EMDEE_HIP_CHECK(hipMemcpyAsync(last, gk.acc.ptr + n + GK_WORDS, GK_WORDS * sizeof(double), hipMemcpyDeviceToHost, sys.stream()));
        EMDEE_HIP_CHECK(hipStreamSynchronize(sys.stream()));
        if (samples) *samples = gk.samples;
    }
    void gk_reset() override { reset(OBS_GK, gk); }
    // ---- spatial profiles along an axis and around a centre (spatial.hpp)
    SpatialRecord spatial;
    // EMDEE_SPATIAL_STRESS bins the atomic tensors, which lack the constraint virial: at set and again at every sample
    void require_spatial(const char *fn, int what) const {
        obs_require_whole_box(fn, obs_engine());
        if (!(what & SPATIAL_STRESS)) return;
        EMDEE_REQUIRE(!sys.has_rigid(), EMDEE_ERR_STATE, "%s: EMDEE_SPATIAL_STRESS on an engine with rigid molecules (emdee_md_set_rigid3): the "
                      "per-atom tensors lack the constraint virial; clear the table first, or profile EMDEE_SPATIAL_DENSITY | EMDEE_SPATIAL_KINETIC", fn);
        EMDEE_REQUIRE(!sys.has_hbonds(), EMDEE_ERR_STATE, "%s: EMDEE_SPATIAL_STRESS on an engine with an hbonds table (emdee_md_set_hbonds): the "
                      "per-atom tensors lack the constraint virial; clear the table first, or profile EMDEE_SPATIAL_DENSITY | EMDEE_SPATIAL_KINETIC", fn);
    }
    // half the shortest periodic side: what a radial table's r_max may reach (a droplet box has no periodic side and no limit)
    double radial_limit() const {
        double h = INFINITY;
        for (int d = 0; d < 3; d++)
            if (sys.per[d]) h = std::min(h, 0.5 * sys.len[d]);
        return h;
    }
    void set_spatial(int32_t geometry, int32_t what, int32_t n_bins, int32_t n_groups, const int32_t *group_dev, const double *range,
                     const double *centre, int32_t centre_group) override {
        use_device(sys.ctx);
        if (n_bins == 0) { spatial = SpatialRecord{}; return; }
        EMDEE_REQUIRE(geometry >= SPATIAL_X && geometry <= SPATIAL_RADIAL, EMDEE_ERR_INVALID, "set_spatial: geometry = %d is none of EMDEE_SPATIAL_X, "
                      "_Y, _Z, _RADIAL (0...3)", geometry);
        EMDEE_REQUIRE(what >= 1 && what <= SPATIAL_ALL, EMDEE_ERR_INVALID, "set_spatial: what = %d is not a non-empty mask of "
                      "EMDEE_SPATIAL_DENSITY | EMDEE_SPATIAL_KINETIC | EMDEE_SPATIAL_STRESS", what);
        EMDEE_REQUIRE(n_bins >= 1 && n_bins <= SPATIAL_MAX_BINS, EMDEE_ERR_INVALID, "set_spatial: n_bins = %d is outside 1...%d (0 clears the table)",
                      n_bins, SPATIAL_MAX_BINS);
        EMDEE_REQUIRE(n_groups >= 1 && n_groups <= SPATIAL_MAX_GROUPS, EMDEE_ERR_INVALID, "set_spatial: n_groups = %d is outside 1...%d", n_groups,
                      SPATIAL_MAX_GROUPS);
        EMDEE_REQUIRE(centre_group >= -1 && centre_group < n_groups, EMDEE_ERR_INVALID, "set_spatial: centre_group = %d is outside -1...%d",
                      centre_group, n_groups - 1);
        require_spatial("set_spatial", what);
        SpatialRecord t;
        if (geometry == SPATIAL_RADIAL) {
            EMDEE_REQUIRE(range, EMDEE_ERR_INVALID, "set_spatial: the radial geometry needs range = {0, r_max}");
            EMDEE_REQUIRE(range[0] == 0.0 && std::isfinite(range[1]) && range[1] > 0.0, EMDEE_ERR_INVALID, "set_spatial: the radial range must be "
                          "{0, r_max} with r_max finite and > 0");
            EMDEE_REQUIRE(range[1] <= radial_limit(), EMDEE_ERR_INVALID, "set_spatial: r_max = %g exceeds half the shortest periodic side %g "
                          "(minimum image)", range[1], radial_limit());
            if (centre_group < 0) {
                EMDEE_REQUIRE(centre, EMDEE_ERR_INVALID, "set_spatial: the radial geometry needs a centre or a centre_group");
                EMDEE_REQUIRE(std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2]), EMDEE_ERR_INVALID,
                              "set_spatial: the centre is not finite");
                for (int d = 0; d < 3; d++) t.centre[d] = centre[d];
            }
            t.range[0] = 0.0; t.range[1] = range[1];
        } else if (sys.per[geometry]) {
            EMDEE_REQUIRE(!range, EMDEE_ERR_INVALID, "set_spatial: axis %d is periodic: its bins are fractions of the box, range must be NULL", geometry);
        } else {
            EMDEE_REQUIRE(range, EMDEE_ERR_INVALID, "set_spatial: axis %d is open: range = {r0, r1} is required", geometry);
            EMDEE_REQUIRE(std::isfinite(range[0]) && std::isfinite(range[1]) && range[0] < range[1], EMDEE_ERR_INVALID, "set_spatial: the range "
                          "must be finite with r0 < r1");
            t.range[0] = range[0]; t.range[1] = range[1];
        }
        const int n = sys.n_owned;
        const std::vector<int32_t> host = fetched_groups(OBS_SPATIAL, group_dev, n_groups);
        const MsdLayout lay = msd_layout(group_dev ? host.data() : nullptr, n, n_groups);
        std::vector<int> atoms((size_t)lay.n_grouped + 1, 0);
        for (int i = 0; i < n; i++)
            if (lay.pos_of[(size_t)i] >= 0) atoms[(size_t)lay.pos_of[(size_t)i]] = i;
        t.present = true; t.geometry = geometry; t.what = what; t.n_atoms = n; t.n_bins = n_bins; t.n_groups = n_groups;
        t.centre_group = geometry == SPATIAL_RADIAL ? centre_group : -1;
        t.n_grouped = lay.n_grouped; t.n_chunks = (int)lay.chunks.size();
        for (int g = 0; g < SPATIAL_MAX_GROUPS; g++) t.sizes[g] = lay.sizes[g];
        for (int g = 0; g <= SPATIAL_MAX_GROUPS; g++) t.chunk_of_group[g] = lay.chunk_of_group[g];
        const size_t nw = (size_t)spatial_n_words(what), slots = lay.chunks.size() * SPATIAL_CHUNK;
        t.pos_of.ensure((size_t)n + 1); t.atoms.ensure(atoms.size()); t.chunk_of_group_dev.ensure(SPATIAL_MAX_GROUPS + 1);
        t.chunks.ensure(lay.chunks.size() + 1); t.key.ensure((size_t)lay.n_grouped + 1); t.planes.ensure(nw * lay.n_grouped + 1);
        t.sbin.ensure(slots + 1); t.runn.ensure(slots + 1); t.runw.ensure(slots * nw + 1);
        t.sums.ensure(t.n_sums()); t.counts.ensure(t.n_cells() + SPATIAL_MAX_GROUPS);
        t.partial.ensure(4 * lay.chunks.size() + 4); t.centre_dev.ensure(4);
        if (n > 0) EMDEE_HIP_CHECK(hipMemcpyAsync(t.pos_of.ptr, lay.pos_of.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, sys.stream()));
        EMDEE_HIP_CHECK(hipMemcpyAsync(t.atoms.ptr, atoms.data(), atoms.size() * sizeof(int), hipMemcpyHostToDevice, sys.stream()));
        EMDEE_HIP_CHECK(hipMemcpyAsync(t.chunk_of_group_dev.ptr, lay.chunk_of_group, sizeof(lay.chunk_of_group), hipMemcpyHostToDevice, sys.stream()));
        if (!lay.chunks.empty())
            EMDEE_HIP_CHECK(hipMemcpyAsync(t.chunks.ptr, lay.chunks.data(), lay.chunks.size() * sizeof(MsdChunk), hipMemcpyHostToDevice, sys.stream()));
        if (t.centre_group >= 0) {                           // (the group's mass, once: the set is blocking anyway)
            double c[4] = {0.0, 0.0, 0.0, 0.0};
            if (sys.n_total > 0) {
                sys.spatial_centre(t);
                EMDEE_HIP_CHECK(hipGetLastError());
                sys.read_back_doubles(c, t.centre_dev.ptr, 4);
            }
            EMDEE_REQUIRE(c[3] > 0.0, EMDEE_ERR_INVALID, "set_spatial: the centre group %d has total mass 0: it has no centre of mass", centre_group);
        }
        install(spatial, t);
    }
    // the geometry of a sample from the box as it is now
    SpatialGeom spatial_geom() const {
        SpatialGeom g{};
        g.geometry = spatial.geometry; g.n_bins = spatial.n_bins;
        if (spatial.geometry == SPATIAL_RADIAL) {
            g.cx = spatial.centre[0]; g.cy = spatial.centre[1]; g.cz = spatial.centre[2];
            for (int d = 0; d < 3; d++) { g.len[d] = sys.per[d] ? sys.len[d] : 0.0; g.inv_len[d] = sys.per[d] ? 1.0 / sys.len[d] : 0.0; }
            g.r_max = spatial.range[1]; g.inv_dr = (double)spatial.n_bins / spatial.range[1];
        } else {
            const int d = spatial.geometry;
            g.periodic = sys.per[d] ? 1 : 0;
            g.lo = g.periodic ? sys.lo[d] : spatial.range[0];
            g.inv_width = (double)spatial.n_bins / (g.periodic ? sys.len[d] : spatial.range[1] - spatial.range[0]);
        }
        return g;
    }
    // one sample: with EMDEE_SPATIAL_STRESS the tensor pass first if it is not current, as gk_sample; without it no pass of the engine
    void spatial_sample() override {
        use_device(sys.ctx);
        obs_require_present(OBS_SPATIAL, "sample", spatial);
        require_spatial("spatial_sample", spatial.what);
        obs_require_fit(OBS_SPATIAL, spatial, obs_engine());
        const int d = spatial.geometry;
        if (d == SPATIAL_RADIAL)
            EMDEE_REQUIRE(spatial.range[1] <= radial_limit(), EMDEE_ERR_STATE, "spatial_sample: the box has shrunk: r_max = %g now exceeds half the "
                          "shortest periodic side %g; set the table again with a smaller r_max", spatial.range[1], radial_limit());
        else
            EMDEE_REQUIRE((sys.per[d] != 0) == (spatial.range[0] == spatial.range[1]), EMDEE_ERR_STATE, "spatial_sample: axis %d has been opened or "
                          "closed since the table was set: set it again (emdee_md_set_spatial)", d);
        if (spatial.what & (SPATIAL_DENSITY | SPATIAL_STRESS))
            EMDEE_REQUIRE(!sys.charges_stale(), EMDEE_ERR_STATE, "spatial_sample: charges set for %lld atoms, the state holds %d: set them again or "
                          "clear them (emdee_md_set_coulomb)", (long long)sys.tables->q_n, sys.n_owned);
        if (spatial.what & SPATIAL_STRESS) tensor_pass();
        sys.spatial_sample(spatial, spatial_geom());
        EMDEE_HIP_CHECK(hipGetLastError());
        spatial.samples++;
        if (d != SPATIAL_RADIAL) {
            const double area = sys.len[(d + 1) % 3] * sys.len[(d + 2) % 3];
            const double width = (sys.per[d] ? sys.len[d] : spatial.range[1] - spatial.range[0]) / (double)spatial.n_bins;
            spatial.inv_bin_volume_sum += 1.0 / (area * width);
        }
    }
    // the deferred fault word of the bonded terms is checked here, not in the sample
    void spatial_read(int64_t *counts, double *sums, int64_t *outside, int64_t *group_sizes, int64_t *frames, double *inv_bin_volume_sum) override {
        use_device(sys.ctx);
        obs_require_present(OBS_SPATIAL, "read", spatial);
        sys.check_bonded();
        const size_t nc = spatial.n_cells();
        if (counts) EMDEE_HIP_CHECK(hipMemcpyAsync(counts, spatial.counts.ptr, nc * sizeof(int64_t), hipMemcpyDeviceToHost, sys.stream()));
        if (outside) EMDEE_HIP_CHECK(hipMemcpyAsync(outside, spatial.counts.ptr + nc, SPATIAL_MAX_GROUPS * sizeof(int64_t), hipMemcpyDeviceToHost, sys.stream()));
        if (sums) EMDEE_HIP_CHECK(hipMemcpyAsync(sums, spatial.sums.ptr, spatial.n_sums() * sizeof(double), hipMemcpyDeviceToHost, sys.stream()));
        EMDEE_HIP_CHECK(hipStreamSynchronize(sys.stream()));
        if (group_sizes) for (int g = 0; g < SPATIAL_MAX_GROUPS; g++) group_sizes[g] = spatial.sizes[g];
        if (frames) *frames = spatial.samples;
        if (inv_bin_volume_sum) *inv_bin_volume_sum = spatial.inv_bin_volume_sum;
    }
    void spatial_reset() override { reset(OBS_SPATIAL, spatial); }
    // one coupling event: the pressure of the step just completed from the engine's own fp64 box sums (the event's one
    // read-back), the factors on the host, emdee_md_scale_box
    void couple(double dt) {
        const double Dt = (double)baro.every * dt, V = sys.len[0] * sys.len[1] * sys.len[2];
        double xi[3] = {0.0, 0.0, 0.0};
        if (baro.kind == EMDEE_BAROSTAT_CRESCALE) {          // xi(seed, s, id = -1), queued ahead of the sums: it comes back with them
            hipLaunchKernelGGL((k_langevin_normals_test<real>), dim3(1), dim3(64), 0, sys.stream(), 1, baro.seed, baro.step,
                               (const long long *)baro_id.ptr, baro_xi.ptr);
            EMDEE_HIP_CHECK(hipMemcpyAsync(xi, baro_xi.ptr, 3 * sizeof(double), hipMemcpyDeviceToHost, sys.stream()));
        }
        double P[3];
        if (by_molecules()) {                                // the molecular pressure, always through the tensor path
            tensor_pass();
            double t[TENSOR_SUMS];
            sys.molecular_tensor_sums(t);
            for (int d = 0; d < 3; d++) P[d] = (t[6 + d] + t[d]) / V;
            if (baro.coupling == EMDEE_COUPLE_ISOTROPIC) P[0] = P[1] = P[2] = (P[0] + P[1] + P[2]) / 3.0;
            if (baro.coupling == EMDEE_COUPLE_SEMIISOTROPIC) P[0] = P[1] = 0.5 * (P[0] + P[1]);
        } else if (baro.coupling == EMDEE_COUPLE_ISOTROPIC) {
            double e[3];
            sys.energy_sums(0.0, e);
            P[0] = P[1] = P[2] = (2.0 * e[1] + e[2]) / (3.0 * V);
        } else {
            tensor_pass();
            double t[TENSOR_SUMS];
            sys.tensor_sums(t);
            for (int d = 0; d < 3; d++) P[d] = (t[6 + d] + t[d]) / V;
            if (baro.coupling == EMDEE_COUPLE_SEMIISOTROPIC) P[0] = P[1] = 0.5 * (P[0] + P[1]);
        }
        // entries of p_ref and compressibility: 0 for the isotropic factor, 0 (x and y) and 2 (z) for the semi-isotropic ones
        const int src[3][3] = {{0, 0, 0}, {0, 0, 2}, {0, 1, 2}};
        double mu[3], vscale = 1.0;
        if (baro.kind == EMDEE_BAROSTAT_BERENDSEN) {
            for (int d = 0; d < 3; d++) {
                const int k = src[baro.coupling][d];
                mu[d] = 1.0 - (Dt / (3.0 * baro.tau_p)) * baro.beta[k] * (baro.p_ref[k] - P[d]);
            }
        } else {
            const double beta = baro.beta[0];
            const double de = -(beta / baro.tau_p) * (baro.p_ref[0] - P[0]) * Dt +
                              std::sqrt(2.0 * baro.temperature * beta * Dt / (V * baro.tau_p)) * xi[0];
            mu[0] = mu[1] = mu[2] = std::exp(de / 3.0);
            vscale = 1.0 / mu[0];
        }
        try {
            scale_box(mu, vscale);
        } catch (const Failure &f) {
            if (f.code != EMDEE_ERR_INVALID) throw;
            // (the message of the refusal stays; the state is the completed step's)
            std::string why = get_error();
            set_error("md_step: pressure coupling at step %llu refused (P = %g %g %g, mu = %g %g %g): %s", baro.step, P[0], P[1], P[2],
                      mu[0], mu[1], mu[2], why.c_str());
            throw Failure{EMDEE_ERR_STATE};
        }
    }
    // emdee_md_minimize (include/emdee_hip.h): FIRE around closed_step.  Iteration 0 is the evaluation at
    // the entry positions (force pass unless forces and energies are current, G, the reduction, the stop test); every later one is a
    // closed step with the capped time step, then G, the reduction, the stop test and the update of minimize.hpp.  The thermostat
    // is left out of the kick + drift for the length of the call and comes back as it was; the box never changes.
    void minimize(int max_iter, double f_tol, double dt_start, double dt_max, double max_step, emdee_minimize_result *out) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(max_iter >= 0, EMDEE_ERR_INVALID, "md_minimize: max_iter = %d is negative", max_iter);
        EMDEE_REQUIRE(std::isfinite(f_tol) && f_tol >= 0.0, EMDEE_ERR_INVALID, "md_minimize: f_tol must be finite and >= 0");
        EMDEE_REQUIRE(std::isfinite(dt_start) && std::isfinite(dt_max) && dt_start > 0.0 && dt_start <= dt_max, EMDEE_ERR_INVALID,
                      "md_minimize: need 0 < dt_start <= dt_max, both finite");
        EMDEE_REQUIRE(std::isfinite(max_step) && max_step > 0.0, EMDEE_ERR_INVALID, "md_minimize: max_step must be finite and > 0");
        require_undivided("md_minimize");
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md_minimize: no state loaded (call emdee_md_set_state first)");
        require_ready("md_minimize");
        sys.ensure_charges();                                // (charges set for another atom count: refused, as a step is)
        struct Unthermostatted {                             // (kick_drift applies the thermostat that is on, and counts its steps)
            NbSystem<real> &s;
            bool on;
            explicit Unthermostatted(NbSystem<real> &sys_) : s(sys_), on(sys_.lgv_on) { s.lgv_on = false; }
            ~Unthermostatted() { s.lgv_on = on; }
        } unthermostatted(sys);
        const int mask = EMDEE_FORCES | EMDEE_ENERGIES;
        emdee_minimize_result res{};
        FireState fire = fire_start(dt_start, dt_max);
        double r[FIRE_WORDS + 1];
        sys.zero_velocities();
        if ((current_mask & mask) != mask) { force_pass(mask); current_mask = mask; }
        const real *G = sys.constrained_force();
        sys.fire_sums(G, r);
        res.energy0 = r[FIRE_WORDS];
        double vmax = 0.0;                                   // the largest speed now: zero at entry and after a reset
        for (;;) {
            // (a sum that is not a number never counts as converged: the maxima alone would drop it)
            res.g_max = std::sqrt(r[3]);
            res.energy = r[FIRE_WORDS];
            if (res.g_max <= f_tol && std::isfinite(r[2])) { res.converged = 1; break; }
            if (res.iterations >= max_iter) break;
            const double t = fire_cap(fire.dt, vmax, std::sqrt(r[5]), max_step);
            if (closed_step(t, mask, 0)) res.rebuilds++;     // (the sites' forces are their parents': G of a site is 0)
            res.iterations++;
            G = sys.constrained_force();
            sys.fire_sums(G, r);
            if (std::sqrt(r[3]) <= f_tol && std::isfinite(r[2])) continue;   // (converged: no update; the test above ends the call)
            const double alpha = fire.alpha;
            if (fire_update(fire, r[0])) {
                // v <- (1 - alpha) v + alpha |v| G / |G|, tangent again through stage (e); no speed now exceeds the bound below
                const double c_g = alpha * std::sqrt(r[1] / r[2]);
                sys.fire_mix(G, 1.0 - alpha, c_g);
                sys.for_each_table([&](auto &g) { sys.velocities(g); });
                vmax = (1.0 - alpha) * std::sqrt(r[4]) + c_g * std::sqrt(r[3]);
            } else {
                sys.zero_velocities();
                vmax = 0.0;
            }
        }
        sys.zero_velocities();
        res.dt = fire.dt;
        check_closed_steps();
        if (out) *out = res;
    }
    void kick_drift(double dt, double kick) override {
        use_device(sys.ctx);
        sys.kick_drift(kick * dt, dt);
        since_build++;
        current_mask = 0;
    }
    void forces(int bitmask, int phase = 0) override {
        use_device(sys.ctx);
        force_pass(Pass<real>::force(bitmask, phase));
        current_mask = phase == 1 ? 0 : bitmask;
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void kick(double dt) override {
        use_device(sys.ctx);
        sys.kick(0.5 * dt);
    }
    bool fused_step(double dt, double kick, int phase) override {
        use_device(sys.ctx);
        const bool ok = sys.fused_step(Pass<real>::step(kick * dt, dt, phase));
        if (ok) { since_build += (phase != 1) ? 1 : 0; current_mask = 0; }
        EMDEE_HIP_CHECK(hipGetLastError());
        return ok;
    }
    bool needs_rebuild() override {
        use_device(sys.ctx);
        return sys.read_rebuild_flag();
    }
    void rebuild() override {
        use_device(sys.ctx);
        sys.resort();
        since_build = 0;
        current_mask = 0;
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void pack_positions(const int32_t *ids, const int32_t *codes, int n, const double *shifts, int n_shifts,
                        void *buf) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        if (n <= 0) return;
        ShiftTable<real> tab{};
        for (int k = 0; k < n_shifts; k++)
            for (int d = 0; d < 3; d++) tab.s[k][d] = (real)shifts[3 * k + d];
        hipLaunchKernelGGL((k_pack_positions<real>), dim3(blocks_for(n, 256)), dim3(256), 0, sys.stream(), n, ids, codes,
                           n_shifts, sys.inv_perm.ptr, sys.rec.ptr, tab, (real *)buf);
    }
    void unpack_ghosts(const void *buf, int first, int n) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        EMDEE_REQUIRE(first >= 0 && n >= 0 && first + n <= n_ghost, EMDEE_ERR_INVALID, "unpack_ghosts: range outside the ghosts");
        if (n == 0) return;
        hipLaunchKernelGGL((k_unpack_ghosts<real>), dim3(blocks_for(n, 256)), dim3(256), 0, sys.stream(), n,
                           sys.n_owned + first, sys.inv_perm.ptr, (const real *)buf, sys.rec.ptr);
        current_mask = 0;
    }
    void energies(double out[3]) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        if ((current_mask & 7) != 7) forces(7, 0);
        if (!lent) sys.check_bonded();                       // (a decomposition checks its domains together)
        sys.energy_sums(0.0, out);
    }
    // the tensor pass, unless the tensors are current: energies, virials and tensors; the forces stay as they are
    void tensor_pass() {
        if (current_mask & EMDEE_TENSOR) return;
        sys.compute_forces(TENSOR_PASS);
        current_mask |= TENSOR_PASS;
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void virial_tensor(void *out) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        EMDEE_REQUIRE(out || sys.n_owned == 0, EMDEE_ERR_INVALID, "tensor is NULL");
        tensor_pass();
        sys.ids_map();                                       // (scratch of the engine's own: before the fence)
        FenceOut fence(caller_ctx, sys.stream());
        sys.unsort_tensor((real *)out);
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void pressure_tensor(double out[12]) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        tensor_pass();
        if (!lent) sys.check_bonded();
        sys.tensor_sums(out);
    }
    // emdee_md_molecular_pressure_tensor: without a table, pressure_tensor's kernels and nothing added
    void molecular_pressure_tensor(double out[12]) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "md: no state loaded");
        EMDEE_REQUIRE(!sys.has_hbonds() || couplable(), EMDEE_ERR_STATE, "molecular_pressure_tensor: the engine holds an hbonds table (emdee_md_set_hbonds): the "
                      "molecular sums are written for three-site molecules and would keep the clusters' constraint forces; clear the table first");
        if (molecular) require_fitting("molecular_pressure_tensor", MOLECULES);   // (a stale table is refused, not passed over)
        if (!by_molecules()) { pressure_tensor(out); return; }
        EMDEE_REQUIRE(!lent && n_ghost == 0, EMDEE_ERR_STATE, "molecular_pressure_tensor: rigid molecules on an integrator with ghosts or a domain's");
        require_fitting("molecular_pressure_tensor", sys.RIGID);
        require_fitting("molecular_pressure_tensor", sys.HBONDS);
        if (!(current_mask & EMDEE_FORCES)) forces(EMDEE_FORCES, 0);
        tensor_pass();
        sys.check_bonded();
        sys.molecular_tensor_sums(out);
    }
    void stats(int64_t *builds, int64_t *listed, int32_t *max_count, int32_t *capacity) override {
        use_device(sys.ctx);
        sys.list_stats(false, listed, max_count, nullptr);
        if (builds) *builds = sys.builds;
        if (capacity) *capacity = sys.stride;
    }
    void count_pairs(int64_t *pairs) override {
        use_device(sys.ctx);
        sys.list_stats(true, nullptr, nullptr, pairs);
    }
    void export_list(int32_t *counts, int32_t *neighbors, int32_t capacity) override {
        use_device(sys.ctx);
        sys.ids_map();
        FenceOut fence(caller_ctx, sys.stream());
        sys.export_list(counts, neighbors, capacity);
    }
    void profile(bool enable) override {
        sys.profiling = enable;
        for (auto &t : sys.timers) t.reset();
    }
    void kernel_time(int kernel, double *total_ms, int64_t *launches) override {
        // ids 0..3: the TimerIds; 4: every fused step launch (interior + boundary halves of a decomposed step together, as
        // before they had timers of their own); 5: all but the boundary halves; 6: the boundary halves; 7: the halo of a
        // decomposed step (pack -> exchange -> unpack); 8: the reciprocal-space pass of an Ewald engine (part of 0's launches too);
        // 9: the constraint stages of an engine with rigid molecules; 10: its molecular sums and molecular scale, and those of a molecule table (emdee_md_set_molecules); 11: the constraint
        // stages of an engine with an hbonds table; 12: what emdee_md_minimize adds to the stages of its steps; 13: placement and
        // force spreading of an engine with virtual sites; 14: the three launches of every event of a global thermostat; 15: the four
        // stages of every sample of the radial distribution functions (emdee_md_rdf_sample); 16: the three launches of every sample
        // of the displacement and velocity correlations (emdee_md_msd_sample); 17: the launches every sample of the Green-Kubo
        // observables adds to the tensor pass (emdee_md_gk_sample); 18: the launch the position restraints add to every force pass, and
        // the scaling of their references (emdee_md_set_restraints); 19: the three launches the centre-of-mass pull adds to every force
        // pass (emdee_md_set_pull); 20: the row pass of the alchemical table at every rebuild and its launches behind every force pass
        // (emdee_md_set_alchemical); 21: the launches of every sample of the spatial profiles (emdee_md_spatial_sample)
        EMDEE_REQUIRE(kernel >= 0 && kernel <= 21, EMDEE_ERR_INVALID, "kernel id out of range");
        use_device(sys.ctx);
        const int ids[22][2] = {{T_FORCE, -1}, {T_KICK_DRIFT, -1}, {T_REBUILD, -1}, {T_KICK, -1}, {T_STEP, T_STEP_BOUNDARY}, {T_STEP, -1},
                                {T_STEP_BOUNDARY, -1}, {T_HALO, -1}, {T_EWALD, -1}, {T_SETTLE, -1}, {T_MOLECULAR, -1},
                                {T_HBONDS, -1}, {T_MINIMIZE, -1}, {T_VSITE, -1}, {T_THERMOSTAT, -1}, {T_RDF, -1}, {T_MSD, -1}, {T_GK, -1},
                                {T_RESTRAINTS, -1}, {T_PULL, -1}, {T_ALCHEMICAL, -1}, {T_SPATIAL, -1}};
        double ms = 0.0;
        int64_t n = 0;
        for (int q = 0; q < 2; q++) {
            if (ids[kernel][q] < 0) continue;
            sys.timers[ids[kernel][q]].collect();
            ms += sys.timers[ids[kernel][q]].total_ms;
            n += sys.timers[ids[kernel][q]].launches;
        }
        if (total_ms) *total_ms = ms;
        if (launches) *launches = n;
    }
    void set_langevin(double gamma, double temperature, uint64_t seed, uint64_t first_step) override {
        EMDEE_REQUIRE(!(gamma > 0.0) || thermo.kind == EMDEE_THERMOSTAT_OFF, EMDEE_ERR_STATE, "set_langevin: a global thermostat is on "
                      "(emdee_md_set_thermostat): switch it off first");
        sys.set_langevin(gamma, temperature, seed, first_step, sys.lgv_ids);
    }
    void set_langevin_ids(const int64_t *ids) override { sys.lgv_ids = reinterpret_cast<const long long *>(ids); }
    // The install path of the three table setters: refused on a domain's engine (`entry`: the decomposition's call for `what`)
    // and without a loaded, ghost-free state; then `set` replaces the table and resets what it must, and the list, the plan and
    // the forces follow the new tables on return (relist = false: a table the list and the forces do not depend on).
    template <class Set>
    void install(const char *what, const char *entry, Set &&set, bool relist = true) {
        use_device(sys.ctx);
        EMDEE_REQUIRE(!lent, EMDEE_ERR_STATE, "%s of a decomposed run: %s (this integrator is a domain's, lent by emdee_dd_engine)", what, entry);
        EMDEE_REQUIRE(sys.sorted && n_ghost == 0 && !sys.id_gaps, EMDEE_ERR_STATE, "%s: set them on a loaded integrator without ghosts (call emdee_md_set_state first)", what);
        set();
        if (!relist) { EMDEE_HIP_CHECK(hipGetLastError()); return; }
        sys.has_list = false; sys.plan = {};                 // (the rows in use follow the old tables; charged and uncharged engines take different kernels and LDS plans)
        sys.resort();                                        // the list, rows and slots for the new tables (a two-species box leaves the typed kernels)
        since_build = 0;
        force_pass(EMDEE_FORCES);
        current_mask = EMDEE_FORCES;
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void set_pairs(const int32_t *pairs, int32_t n_pairs, bool one_four, double lj14scale) override {
        install("exclusions / 1-4 pairs", "emdee_dd_set_exclusions / emdee_dd_set_pairs14", [&] {
            sys.set_pair_tables(sys.n_owned, pairs, n_pairs, one_four, lj14scale);
            sys.reset_ewald_error();
        });
        sys.check_ewald();                                   // (blocking read-back, Ewald engines with struck pairs only)
    }
    void set_bonded(int32_t kind, const int32_t *atoms, const double *params, int32_t n_terms) override {
        install("bonded terms", "emdee_dd_set_bonded", [&] {
            sys.own_tables.set_bonded(kind, atoms, params, n_terms, sys.n_owned, sys.stream());
            sys.reset_bonded_error();
        });
        sys.check_bonded();                                  // (blocking read-back; throws if a term spans more than the list radius)
    }
    void set_coulomb(const double *charges, int32_t n, double coulomb_k, double eps_rf, double coulomb14scale) override {
        install("charges", "emdee_dd_set_coulomb", [&] {
            sys.own_tables.set_charges(charges, n, coulomb_k, eps_rf, coulomb14scale, sys.n_owned, sys.stream());
            sys.reset_charge_error();
            if (n == 0) sys.ewald.clear();                   // (no charges, no Ewald sum: the next set_coulomb starts with the reaction field)
        });
    }
    // emdee_md_set_rigid3, emdee_md_set_hbonds: all or nothing -- the candidate table is checked on the host and then against the
    // loaded state before it replaces the one in force; no atom moves, the velocities are projected once (stage (e)).  The
    // neighbour list and the forces do not depend on the table: nothing is rebuilt.  set(check): the Topology setter of group k.
    template <class Set>
    void set_groups(int k, const char *what, Set &&set) {
        auto &g = sys.groups[k];
        install(what, "a decomposed run has none", [&] {
            set([&](const int *a, const double *d, const std::vector<int32_t> &h, int n) {
                sys.check_state(g, a, d, h, n);
                sys.check_groups_whole(a, d, n, g.sites);         // (a molecule table in force: the groups lie whole inside its molecules)
            });
            sys.reset_error(g);
            unchecked[k] = false;
            if (sys.table(g).present) sys.velocities(g);
        }, false);
    }
    void set_rigid3(const int32_t *atoms, const double *geom, int32_t n_mol) override {
        EMDEE_REQUIRE(baro.kind == EMDEE_BAROSTAT_OFF || molecular, EMDEE_ERR_STATE, "set_rigid3: pressure coupling is on (emdee_md_set_barostat): the pressure "
                      "of an engine with rigid molecules lacks the constraint virial; switch the coupling off first (or couple to the molecular "
                      "pressure: emdee_md_set_molecular_scaling)");
        set_groups(sys.RIGID, "rigid molecules", [&](auto &&check) { sys.own_tables.set_rigid3(atoms, geom, n_mol, sys.n_owned, sys.stream(), check); });
    }
    void set_hbonds(const int32_t *atoms, const double *dist, int32_t n_clusters) override {
        // (with a molecule table in force and the switch on, the engine stays couplable: the builder refuses a cluster the table splits)
        EMDEE_REQUIRE(baro.kind == EMDEE_BAROSTAT_OFF || n_clusters == 0 || (molecular && sys.has_molecules()), EMDEE_ERR_STATE, "set_hbonds: pressure coupling is on (emdee_md_set_barostat): the pressure of "
                      "an engine with an hbonds table lacks the clusters' constraint virial; switch the coupling off first");
        set_groups(sys.HBONDS, "hbonds clusters", [&](auto &&check) { sys.own_tables.set_hbonds(atoms, dist, n_clusters, sys.n_owned, sys.stream(), check); });
    }
    // emdee_md_set_molecules: all or nothing -- the candidate table is fetched, checked and built on the host (topo::molecule_table),
    // uploaded, and checked against the loaded state (NbSystem::check_molecules) before it replaces the one in force.  No atom moves;
    // neither the list nor the forces depend on the table.
    void set_molecules(const int32_t *molecule_dev, int32_t n) override {
        EMDEE_REQUIRE(n != 0 || baro.kind == EMDEE_BAROSTAT_OFF || couplable(molecular, false), EMDEE_ERR_STATE, "set_molecules: pressure coupling is on "
                      "(emdee_md_set_barostat) and the engine holds an hbonds table, which couples through the molecule table alone: switch the "
                      "coupling off or clear the hbonds table (emdee_md_set_hbonds) first");
        install("the molecule table (emdee_md_set_molecules)", "a decomposed run has none", [&] {
            EMDEE_REQUIRE(sys.with_vel, EMDEE_ERR_STATE, "set_molecules: the state was loaded without velocities");
            sys.own_tables.set_molecules(molecule_dev, n, sys.n_owned, sys.stream(), [&](const Topology::MoleculeTable &t) { sys.check_molecules(t); });
            unchecked[MOLECULES] = false;
        }, false);
    }
    // emdee_md_set_vsites: all or nothing -- the candidate table is checked on the host and then against the loaded masses before it
    // replaces the one in force.  The sites' velocities become 0, the sites are placed, and the list and the forces follow where they
    // now are (the relisting install path): on return positions, forces and list belong together.
    void set_vsites(const int32_t *atoms, const double *weights, int32_t n_sites) override {
        install("virtual sites", "a decomposed run has none", [&] {
            sys.own_tables.set_vsites(atoms, weights, n_sites, sys.n_owned, sys.stream(), [&](const Topology::VsiteTable &t) { sys.check_vsites(t); });
            unchecked[VSITES] = false;
            if (sys.vsites_fit()) sys.place_sites(true);
        });
    }
    // emdee_md_set_restraints: all or nothing -- the candidate table is fetched, checked on the host (topo::restraint_table) and uploaded
    // before anything in force changes, then installed whole.  The neighbour list does not depend on the table; the forces do, and are
    // evaluated again, so that planes and table belong together on return.
    void set_restraints(const int32_t *atoms, const double *ref, const double *k, const double *flat, int32_t n) override {
        install("position restraints", "a decomposed run has none", [&] {
            EMDEE_REQUIRE(sys.with_vel, EMDEE_ERR_STATE, "set_restraints: the state was loaded without velocities");
            sys.own_tables.set_restraints(atoms, ref, k, flat, n, sys.n_owned, sys.stream(),
                                          [&](const int *a, double *r, int m) { sys.capture_restraint_refs(a, r, m); });
            unchecked[RESTRAINTS] = false;
        }, false);
        if (sys.charges_stale()) { current_mask = 0; return; }
        force_pass(EMDEE_FORCES);
        current_mask = EMDEE_FORCES;
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void restraint_sums(double *out) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(out, EMDEE_ERR_INVALID, "restraint_sums: out is NULL");
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "restraint_sums: no state loaded (call emdee_md_set_state first)");
        require_fitting("restraint_sums", RESTRAINTS);
        sys.restraint_sums(out);
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    void get_restraint_refs(double *ref_dev) override {
        use_device(sys.ctx);
        const Topology::RestraintTable &t = sys.tables->restraints;
        if (!t.present || t.n == 0) return;
        EMDEE_REQUIRE(ref_dev, EMDEE_ERR_INVALID, "get_restraint_refs: ref is NULL");
        require_fitting("get_restraint_refs", RESTRAINTS);
        FenceOut fence(caller_ctx, sys.stream());
        EMDEE_HIP_CHECK(hipMemcpyAsync(ref_dev, t.ref.ptr, (size_t)3 * t.n * sizeof(double), hipMemcpyDeviceToDevice, sys.stream()));
    }
    // emdee_md_set_pull: all or nothing -- the group array is fetched, the table checked and built on the host (topo::pull_table) and
    // uploaded before anything in force changes, then installed whole.  The neighbour list does not depend on the table; the forces do,
    // and are evaluated again, so that planes, read-back words and table belong together on return.
    void set_pull(const int32_t *group, int32_t n_groups, const int32_t *coords, const double *params, int32_t n_coords, int32_t log_every,
                  int32_t log_capacity) override {
        install("the centre-of-mass pull (emdee_md_set_pull)", "a decomposed run has none", [&] {
            EMDEE_REQUIRE(sys.with_vel, EMDEE_ERR_STATE, "set_pull: the state was loaded without velocities");
            sys.own_tables.set_pull(group, n_groups, coords, params, n_coords, log_every, log_capacity, sys.n_owned, sys.stream());
            unchecked[PULL] = false;
        }, false);
        if (sys.charges_stale() || restraints_unfit() || alch_unfit()) { current_mask = 0; return; }
        force_pass(EMDEE_FORCES);
        current_mask = EMDEE_FORCES;
        EMDEE_HIP_CHECK(hipGetLastError());
    }
    // what the last force pass wrote: one copy, no launch
    void pull_read(double *coords_out, double *groups_out) override {
        use_device(sys.ctx);
        Topology::PullTable &t = sys.own_tables.pull;
        EMDEE_REQUIRE(!lent && t.present, EMDEE_ERR_STATE, "pull_read: no pull table is set (emdee_md_set_pull)");
        require_fitting("pull_read", PULL);
        double h[PULL_MAX_COORDS * PULL_WORDS + PULL_MAX_GROUPS * 4];
        sys.read_back_doubles(h, t.out.ptr, PULL_MAX_COORDS * PULL_WORDS + PULL_MAX_GROUPS * 4);
        if (coords_out) for (int q = 0; q < t.n * PULL_WORDS; q++) coords_out[q] = h[q];
        if (groups_out) for (int q = 0; q < t.n_groups * 4; q++) groups_out[q] = h[PULL_MAX_COORDS * PULL_WORDS + q];
    }
    void pull_log_read(double *log_dev, int64_t *count, int64_t *dropped) override {
        use_device(sys.ctx);
        Topology::PullTable &t = sys.own_tables.pull;
        EMDEE_REQUIRE(!lent && t.present, EMDEE_ERR_STATE, "pull_log_read: no pull table is set (emdee_md_set_pull)");
        if (count) *count = t.log_count;
        if (dropped) *dropped = t.log_dropped;
        if (!log_dev || t.log_count == 0) return;
        FenceOut fence(caller_ctx, sys.stream());
        EMDEE_HIP_CHECK(hipMemcpyAsync(log_dev, t.log.ptr, (size_t)2 * t.log_count * t.n * sizeof(double), hipMemcpyDeviceToDevice, sys.stream()));
    }
    // emdee_md_set_alchemical: all or nothing -- the flags are fetched and every check is made on the host (alchemical.hpp) before
    // anything in force changes, then the table is installed whole.  The rows depend on the table (the cross entries leave them, or
    // come back at a clear): the list is rebuilt and the forces are evaluated again, as after emdee_md_set_exclusions.
    void set_alchemical(const int32_t *flag, double lambda, double alpha, const double *foreign, int32_t n_foreign, int32_t log_every,
                        int32_t log_capacity) override {
        install("the alchemical table (emdee_md_set_alchemical)", "a decomposed run has none", [&] {
            EMDEE_REQUIRE(!sys.charges_stale() && !restraints_unfit() && !pull_unfit(), EMDEE_ERR_STATE, "set_alchemical: another table of the engine "
                          "(charges, restraints or pull) was set for another atom count: set it again or clear it first");
            sys.own_tables.set_alchemical(flag, lambda, alpha, foreign, n_foreign, log_every, log_capacity, sys.n_owned, sys.stream());
            unchecked[ALCHEMICAL] = false;
        });
    }
    // a host scalar, handed to the kernels as an argument: no rebuild; the next step or query evaluates the forces anew
    void set_lambda(double lambda) override {
        use_device(sys.ctx);
        Topology::AlchTable &t = sys.own_tables.alch;
        EMDEE_REQUIRE(!lent && t.present, EMDEE_ERR_STATE, "set_lambda: no alchemical table is set (emdee_md_set_alchemical)");
        alch_check_lambda("set_lambda", lambda);
        t.lambda = lambda;
        current_mask = 0;
    }
    // lambda, U_alch, dU/dlambda, the cross virial and the cross pairs inside rc of the current positions (a force pass if lambda or
    // the state changed since the last), then U_alch at the foreign lambdas (the energies-only launch); blocking, one copy
    void alchemical_read(double *words) override {
        use_device(sys.ctx);
        Topology::AlchTable &t = sys.own_tables.alch;
        EMDEE_REQUIRE(!lent && t.present, EMDEE_ERR_STATE, "alchemical_read: no alchemical table is set (emdee_md_set_alchemical)");
        EMDEE_REQUIRE(words, EMDEE_ERR_INVALID, "alchemical_read: words is NULL");
        require_fitting("alchemical_read", ALCHEMICAL);
        EMDEE_REQUIRE(n_ghost == 0, EMDEE_ERR_STATE, "alchemical_read: the state has ghosts");
        if (!(current_mask & EMDEE_FORCES)) forces(EMDEE_FORCES, 0);
        {
            typename NbSystem<real>::Timed timed(&sys, T_ALCHEMICAL);
            sys.queue_alch_foreign();
        }
        double h[ALCH_WORDS + ALCH_MAX_FOREIGN];
        sys.read_back_doubles(h, t.out.ptr, ALCH_WORDS + ALCH_MAX_FOREIGN);
        for (int q = 0; q < ALCH_WORDS + t.n_foreign; q++) words[q] = h[q];
    }
    void alchemical_log_read(double *log_dev, int64_t *count, int64_t *dropped) override {
        use_device(sys.ctx);
        Topology::AlchTable &t = sys.own_tables.alch;
        EMDEE_REQUIRE(!lent && t.present, EMDEE_ERR_STATE, "alchemical_log_read: no alchemical table is set (emdee_md_set_alchemical)");
        if (count) *count = t.log_count;
        if (dropped) *dropped = t.log_dropped;
        if (!log_dev || t.log_count == 0) return;
        FenceOut fence(caller_ctx, sys.stream());
        EMDEE_HIP_CHECK(hipMemcpyAsync(log_dev, t.log.ptr, (size_t)t.log_count * (2 + t.n_foreign) * sizeof(double), hipMemcpyDeviceToDevice,
                                       sys.stream()));
    }
    // emdee_md_set_alchemical_coulomb: the Coulomb stage of the table in force, all or nothing; the rows and the CSR do not depend on
    // it, so nothing is rebuilt: the next step or query evaluates the forces anew.  enable = 0 clears the stage.
    void set_alchemical_coulomb(int32_t enable, double lambda_q, double beta, const double *foreign_q, int32_t n_foreign) override {
        use_device(sys.ctx);
        EMDEE_REQUIRE(!lent, EMDEE_ERR_STATE, "set_alchemical_coulomb: a decomposed run has no alchemical table (this integrator is a domain's, "
                      "lent by emdee_dd_engine)");
        Topology::AlchTable &t = sys.own_tables.alch;
        if (enable) {
            EMDEE_REQUIRE(t.present, EMDEE_ERR_STATE, "set_alchemical_coulomb: no alchemical table is set (emdee_md_set_alchemical)");
            EMDEE_REQUIRE(sys.has_charges(), EMDEE_ERR_STATE, "set_alchemical_coulomb: the engine has no charges (call emdee_md_set_coulomb first)");
            EMDEE_REQUIRE(n_ghost == 0, EMDEE_ERR_STATE, "set_alchemical_coulomb: the state has %d ghosts; load a state without ghosts", n_ghost);
            alch_coulomb_check_params(lambda_q, beta, foreign_q, n_foreign, t.n_foreign);
            require_no_recip_solute_charge("set_alchemical_coulomb", alch_first_charged(t.atoms_h, sys.tables->q_h));
        }
        sys.own_tables.set_alchemical_coulomb(enable, lambda_q, beta, foreign_q, n_foreign, sys.stream());
        current_mask = 0;
    }
    void set_lambda_coulomb(double lambda_q) override {
        use_device(sys.ctx);
        Topology::AlchTable &t = sys.own_tables.alch;
        EMDEE_REQUIRE(!lent && t.present && t.coulomb, EMDEE_ERR_STATE, "set_lambda_coulomb: no Coulomb stage is set (emdee_md_set_alchemical_coulomb)");
        alch_check_lambda_q("set_lambda_coulomb", lambda_q);
        t.lambda_q = lambda_q;
        current_mask = 0;
    }
    // lambda_q, U_q, dU/dlambda_q and the cross Coulomb virial of the current positions (a force pass if a lambda or the state changed
    // since the last), then U_q at the foreign lambda_q (the energies-only launch); blocking, one copy
    void alchemical_coulomb_read(double *words) override {
        use_device(sys.ctx);
        Topology::AlchTable &t = sys.own_tables.alch;
        EMDEE_REQUIRE(!lent && t.present && t.coulomb, EMDEE_ERR_STATE, "alchemical_coulomb_read: no Coulomb stage is set (emdee_md_set_alchemical_coulomb)");
        EMDEE_REQUIRE(words, EMDEE_ERR_INVALID, "alchemical_coulomb_read: words is NULL");
        require_fitting("alchemical_coulomb_read", ALCHEMICAL);
        EMDEE_REQUIRE(n_ghost == 0, EMDEE_ERR_STATE, "alchemical_coulomb_read: the state has ghosts");
        if (!(current_mask & EMDEE_FORCES)) forces(EMDEE_FORCES, 0);
        {
            typename NbSystem<real>::Timed timed(&sys, T_ALCHEMICAL);
            sys.queue_alch_foreign();
        }
        double h[ALCH_COULOMB_WORDS + ALCH_MAX_FOREIGN];
        sys.read_back_doubles(h, t.out_q.ptr, ALCH_COULOMB_WORDS + ALCH_MAX_FOREIGN);
        for (int q = 0; q < ALCH_COULOMB_WORDS + t.n_foreign; q++) words[q] = h[q];
    }
    void alchemical_coulomb_log_read(double *log_dev, int64_t *count, int64_t *dropped) override {
        use_device(sys.ctx);
        Topology::AlchTable &t = sys.own_tables.alch;
        EMDEE_REQUIRE(!lent && t.present && t.coulomb, EMDEE_ERR_STATE, "alchemical_coulomb_log_read: no Coulomb stage is set (emdee_md_set_alchemical_coulomb)");
        if (count) *count = t.log_count;
        if (dropped) *dropped = t.log_dropped;
        if (!log_dev || t.log_count == 0) return;
        FenceOut fence(caller_ctx, sys.stream());
        EMDEE_HIP_CHECK(hipMemcpyAsync(log_dev, t.log_q.ptr, (size_t)t.log_count * (2 + t.n_foreign) * sizeof(double), hipMemcpyDeviceToDevice,
                                       sys.stream()));
    }
    // emdee_md_set_ewald, emdee_md_set_pme: all or nothing -- every refusal comes before the setting changes.  check(): the host
    // test of the setting; set(): EwaldRecip's setter (the mesh takes the place of the direct sum)
    template <class Check, class Set>
    void set_recip(const char *entry, const char *what, double alpha, Check &&check, Set &&set) {
        EMDEE_REQUIRE(alpha == 0.0 || (std::isfinite(alpha) && alpha > 0.0), EMDEE_ERR_INVALID, "%s: alpha must be finite and >= 0", entry);
        if (alpha > 0.0) check();
        require_undivided(entry);
        EMDEE_REQUIRE(sys.sorted, EMDEE_ERR_STATE, "%s: no state loaded (call emdee_md_set_state first)", entry);
        EMDEE_REQUIRE(sys.has_charges() && !sys.charges_stale(), EMDEE_ERR_STATE, "%s: the engine has no charges for its state (call emdee_md_set_coulomb first)", entry);
        EMDEE_REQUIRE(sys.per[0] && sys.per[1] && sys.per[2], EMDEE_ERR_STATE, "%s: the box must be periodic in all three dimensions", entry);
        install(what, "a decomposed run has none", [&] {
            if (alpha > 0.0) set(); else sys.ewald.clear();
            sys.reset_ewald_error();
        });
        sys.check_ewald();
    }
    void set_ewald(double alpha, const int32_t *kmax) override {
        set_recip("set_ewald", "Ewald summation", alpha, [&] { topo::check_ewald(alpha, kmax, std::sqrt(sys.model_d.rc2)); },
                  [&] { sys.ewald.set(alpha, kmax); });
    }
    void set_pme(double alpha, const int32_t *grid, int32_t order) override {
        set_recip("set_pme", "particle-mesh Ewald summation", alpha, [&] { topo::check_pme(alpha, grid, order, std::sqrt(sys.model_d.rc2)); },
                  [&] { sys.ewald.set_pme(alpha, grid, order); });
    }
    void langevin_normals(uint64_t seed, uint64_t step, const int64_t *ids, int n, double *out) override {
        use_device(sys.ctx);
        if (n <= 0) return;
        hipLaunchKernelGGL((k_langevin_normals_test<real>), dim3(blocks_for(n, 256)), dim3(256), 0, sys.stream(), n,
                           (unsigned long long)seed, (unsigned long long)step, reinterpret_cast<const long long *>(ids), out);
        EMDEE_HIP_CHECK(hipGetLastError());
    }
};

// ------------------------------------------------------------------------------------ factories
template <typename real>
ICells *Factory<real>::cells(emdee_ctx *ctx, int N, double L, double cutoff, int ndiv) {
    return new CellsImpl<real>(ctx, N, L, cutoff, ndiv);
}
template <typename real>
INbr *Factory<real>::nbr(emdee_ctx *ctx, int N, double skin) {
    return new NbrImpl<real>(ctx, N, skin);
}
template <typename real>
IMd *Factory<real>::md(emdee_ctx *ctx, const double lo[3], const double len[3], const int32_t per[3],
                       const emdee_lj_model &model, double skin) {
    return new MdImpl<real>(ctx, lo, len, per, model, skin);
}

template <typename real>
void Factory<real>::tiles(emdee_ctx *ctx, void *f, void *e, void *w, const void *pos, double L, int N,
                          const emdee_lj_model &model, const emdee_lj_atom *atoms, int bitmask, int mode) {
    use_device(ctx);
    EMDEE_REQUIRE(N >= 0 && L > 0, EMDEE_ERR_INVALID, "tiles: need N >= 0 and L > 0");
    EMDEE_REQUIRE(bitmask >= 0 && bitmask <= 7, EMDEE_ERR_INVALID, "bitmask must be a combination of FORCES|ENERGIES|VIRIALS");
    EMDEE_REQUIRE(mode == EMDEE_LITERAL || mode == EMDEE_CUTOFF, EMDEE_ERR_INVALID, "mode must be LITERAL or CUTOFF");
    if (N == 0 || bitmask == 0) return;
    EMDEE_REQUIRE(pos && atoms, EMDEE_ERR_INVALID, "positions/atoms are NULL");
    EMDEE_REQUIRE((!(bitmask & 1) || f) && (!(bitmask & 2) || e) && (!(bitmask & 4) || w), EMDEE_ERR_INVALID,
                  "a selected output is NULL");
    LJModel<real> m = make_model<real>(model);
    const int nt = (N + TILE - 1) / TILE;
    with_bool(mode == EMDEE_LITERAL, [&](auto literal) {
        hipLaunchKernelGGL((k_tiles<real, decltype(literal)::value ? EMDEE_LITERAL : EMDEE_CUTOFF>), dim3(nt), dim3(TILE_BLOCK), 0, ctx->stream, N,
                           (const real *)pos, (real)L, atoms, m, bitmask, (real *)f, (real *)e, (real *)w);
    });
    EMDEE_HIP_CHECK(hipGetLastError());
}

template <typename real>
void Factory<real>::naive(emdee_ctx *ctx, void *f, void *e, void *w, const void *pos, double L, int N,
                          const emdee_lj_model &model, const emdee_lj_atom *atoms, int mode) {
    use_device(ctx);
    EMDEE_REQUIRE(N >= 0 && L > 0, EMDEE_ERR_INVALID, "naive: need N >= 0 and L > 0");
    EMDEE_REQUIRE(mode == EMDEE_LITERAL || mode == EMDEE_CUTOFF, EMDEE_ERR_INVALID, "mode must be LITERAL or CUTOFF");
    if (N == 0) return;
    EMDEE_REQUIRE(pos && atoms && f && e && w, EMDEE_ERR_INVALID, "naive: NULL array");
    LJModel<real> m = make_model<real>(model);
    with_bool(mode == EMDEE_LITERAL, [&](auto literal) {
        hipLaunchKernelGGL((k_naive<real, decltype(literal)::value ? EMDEE_LITERAL : EMDEE_CUTOFF>), dim3(blocks_for(N, 64)), dim3(64), 0, ctx->stream,
                           N, (const real *)pos, (real)L, atoms, m, (real *)f, (real *)e, (real *)w);
    });
    EMDEE_HIP_CHECK(hipGetLastError());
}

template <typename real>
void Factory<real>::interaction(emdee_ctx *ctx, int n, const void *r2, const emdee_lj_model &model, emdee_lj_atom ai,
                                emdee_lj_atom aj, int mode, void *E, void *W) {
    use_device(ctx);
    EMDEE_REQUIRE(n >= 0, EMDEE_ERR_INVALID, "interaction: negative n");
    if (n == 0) return;
    EMDEE_REQUIRE(r2 && E && W, EMDEE_ERR_INVALID, "interaction: NULL array");
    hipLaunchKernelGGL((k_interaction<real>), dim3(blocks_for(n, 256)), dim3(256), 0, ctx->stream, n, (const real *)r2,
                       make_model<real>(model), ai, aj, mode, (real *)E, (real *)W);
    EMDEE_HIP_CHECK(hipGetLastError());
}

}  // namespace emdee
