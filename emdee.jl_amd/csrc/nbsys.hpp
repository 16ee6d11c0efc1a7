// nbsys.hpp -- host-side driver of the cell-ordered system: owns the HBM buffers and enqueues
// the kernels of kernels.hpp / brick.hpp on the context's stream.  Instantiated for float and double.
#pragma once
#include <cstdio>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "brick.hpp"
#include "ewald.hpp"
#include "kernels.hpp"
#include "minimize.hpp"
#include "molecule.hpp"
#include "observables.hpp"
#include "plan.hpp"
#include "pull.hpp"
#include "restraint.hpp"
#include "settle.hpp"
#include "shake.hpp"
#include "thermostat.hpp"
#include "topology_dev.hpp"
#include "typed.hpp"
#include "vsite.hpp"

namespace emdee {

// The laboratory of rounds 1-5 -- measured alternatives that lost and the ablation switches that measured them -- has been
// retired from the tree ("Product and laboratory", keeps the measurements).  A retired switch found in the
// environment is REFUSED with a message when an engine is created, not ignored (a run that believes it is measuring a
// variant must not silently measure the default).
static inline void refuse_experiment_switches() {
    static const char *const gone[] = {"EMDEE_DEBUG_RC2_SCALE", "EMDEE_TBUILD", "EMDEE_BUILD4", "EMDEE_BUILD_ALG", "EMDEE_BUILD_CHUNKED",
        "EMDEE_BUILD_STRIDED", "EMDEE_NO_BRICK_TABLES", "EMDEE_NO_PREMUL", "EMDEE_BUILD_NEARFAR", "EMDEE_NEAR_DELTA", "EMDEE_FAR_SKIP",
        "EMDEE_PLAN_MAXIMA", "EMDEE_PLAN_SYNC", "EMDEE_STRIDE", "EMDEE_BRICK_VARIANT"};
    for (const char *name : gone)
        EMDEE_REQUIRE(std::getenv(name) == nullptr, EMDEE_ERR_INVALID,
                      "%s is an experiment switch that has been retired with the laboratory (make EXPERIMENTS=1 no longer "
                      "exists): the variant it selected is not built; its measurement is recorded in DESIGN.md, "
                      "\"Product and laboratory\"", name);
}

// T_STEP: every fused step launch but the boundary-brick halves of a decomposed step, which go to T_STEP_BOUNDARY (emdee_md_kernel_time(4)
// reports the two together, 5 and 6 one each); T_HALO: pack -> exchange -> unpack of a decomposed step, on the stream they run on
// T_EWALD: the reciprocal-space pass of an Ewald engine (ewald.hpp), which runs inside T_FORCE's launches as well
// T_SETTLE: the three constraint stages of an engine with rigid molecules (settle.hpp)
// T_MOLECULAR: the molecular sums and the molecular scale of an engine with rigid molecules (settle.hpp) or a molecule table (molecule.hpp)
// T_HBONDS: the three constraint stages of an engine with an hbonds table (shake.hpp)
// T_MINIMIZE: what emdee_md_minimize adds to the stages of a closed step (minimize.hpp): the constrained force, the reduction, the mixing
// T_VSITE: placement and force spreading of an engine with virtual sites (vsite.hpp)
// T_THERMOSTAT: the three launches of a global thermostat's event (thermostat.hpp)
// T_RDF: the four stages of a sample of the radial distribution functions (rdf.hpp): count, scan, fill, pair loop
// T_MSD: the three launches of a sample of the displacement and velocity correlations (msd.hpp): gather, accumulate, finish
// T_GK: the launches a sample of the Green-Kubo observables adds to the tensor pass (gk.hpp): the box sums, the heat sums, push, correlate
// T_RESTRAINTS: the launch the position restraints add to every force pass, and the scaling of their references (restraint.hpp)
// T_PULL: the three launches the centre-of-mass pull adds to every force pass (pull.hpp): partial sums, finish, apply
// T_ALCHEMICAL: the row pass of the alchemical table at a rebuild and its launches behind a force pass (alchemical.hpp)
// T_SPATIAL: the three launches of a sample of the spatial profiles (spatial.hpp): gather, accumulate, finish; two more ahead of them
// with a centre group (the chunks' partial sums, the centre of mass)
enum TimerId { T_FORCE = 0, T_KICK_DRIFT = 1, T_REBUILD = 2, T_KICK = 3, T_STEP = 4, T_STEP_BOUNDARY = 5, T_HALO = 6, T_EWALD = 7, T_SETTLE = 8,
               T_MOLECULAR = 9, T_HBONDS = 10, T_MINIMIZE = 11, T_VSITE = 12, T_THERMOSTAT = 13, T_RDF = 14, T_MSD = 15, T_GK = 16, T_RESTRAINTS = 17,
               T_PULL = 18, T_ALCHEMICAL = 19, T_SPATIAL = 20, T_COUNT = 21 };
// The words of NbSystem::flags above the ones the build, the plan and the step kernels use (flags[0..15]).  Fault words (FaultWord,
// common.hpp), each the entry + 1 a kernel failed on: W_BONDED, a bonded term whose partner was missing from the rows (k_bonded);
// W_CHARGES, a key without a charge (k_fill_charges); W_EWALD, a struck pair whose partner was missing from the rows
// (k_ewald_struck); W_SETTLE / W_HBONDS, a molecule / a cluster that moved too far for a solution (k_constraint_positions).
// Words of the table checks (k_constraint_check), cleared and read by every check: W_RIGID_MASS, W_RIGID_DIST; W_HBONDS_DIST.
// W_VSITE_MASS, two words of the site table's check (k_vsite_check): a site with a mass, a site with a massless parent.
// W_MOLECULE_MASS, two words of the molecule table's check (molecule.hpp): a molecule of mass 0, a molecule not loaded whole.
// W_IMAGE, three words: an atom (id + 1) whose periodic image count left its 10-bit field, the axis and the count (kernels.hpp
// img_bound, raised by the two gathers); they ride the read-back every build makes.
enum FlagWord { W_BONDED = 16, W_CHARGES = 17, W_EWALD = 18, W_SETTLE = 20, W_RIGID_MASS = 21, W_RIGID_DIST = 22, W_HBONDS = 23,
                W_HBONDS_DIST = 24, W_IMAGE = 25, W_VSITE_MASS = 28, W_MOLECULE_MASS = 30 };
enum PathId { PATH_BRICK = 0, PATH_DIRECT = 1 };

// (the brick kernel variants, LDS_LIMIT and with_brick_variant: plan.hpp)
template <typename K>
static inline void allow_big_lds(K kernel, size_t bytes) {
    if (bytes > 48 * 1024)
        EMDEE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// What one force pass or one fused step is asked to do.  The defaults are a plain force pass over every brick into the engine's
// own arrays; a launch that is neither (build, tables, filter, export, stats) takes a default one.
template <typename real>
struct Pass {
    int mask = EMDEE_FORCES;
    int phase = 0;                        // 0: every brick; 1 / 2: the interior / the boundary bricks (the two halves of a decomposed step)
    double c = 0.0, dt = 0.0;             // a step: v += c f/m, x += dt v
    const int *guard = nullptr;           // a step (device words, see NbSystem::fused_step): does nothing but raise *trigger when *guard is set,
    int *trigger = nullptr;               // ... and raises *trigger when an atom has moved skin/2 since the last build (NULL: flags[1])
    // operator path, tiled kernels only: the outputs go straight to these caller-order arrays (vt: the tensor pass's 6 x N array)
    real *f = nullptr, *e = nullptr, *w = nullptr, *vt = nullptr;
    const real *pos = nullptr;            // ... and the caller's positions, which the tiles of the Float32 reference arithmetic are staged from
    // fused_step: copy the ghosts' current coordinates into the buffer that becomes current (callers that unpack fresh ghosts
    // before every force evaluation, as emdee_dd_step does, do not need it); the caller has already queued prepare_noise(dt) for
    // this step (it must precede work on another stream)
    bool carry_ghosts = true, noise_ready = false;
    // a force pass whose kernel instance writes more outputs than `mask` selects (NbSystem::runs_all_outputs): the engine's planes of
    // the outputs left out are not to be touched, the kernel writes those to the spare planes
    bool spare_unselected = false;

    bool to_caller() const { return f || e || w || vt; }
    static Pass force(int mask, int phase = 0) { Pass p; p.mask = mask; p.phase = phase; return p; }
    static Pass step(double c, double dt, int phase = 0) { Pass p; p.c = c; p.dt = dt; p.phase = phase; return p; }
};

template <typename real>
struct NbSystem {
    emdee_ctx *ctx = nullptr;
    double lo[3] = {0, 0, 0}, len[3] = {0, 0, 0};
    int per[3] = {1, 1, 1};
    double skin = 0.3, rlist = 0.0;
    emdee_lj_model model_d{};
    LJModel<real> model{};
    GridP<real> grid{};
    size_t ncell = 0;
    int n_total = 0, n_owned = 0;
    size_t pitch = 0;
    bool with_vel = false, with_mass = false;
    bool sorted = false, has_list = false;
    // the list's rows: entries per row, and whether they already include the typed rows' segment padding (both outlive a plan)
    int stride = 0;
    bool typed_stride = false;
    int64_t builds = 0;
    bool profiling = false;
    KernelTimer timers[T_COUNT];

    // path selection
    int path = PATH_BRICK;
    // which kernels the state runs on (plan.hpp): chosen by choose_plan at a load, kept from rebuild to rebuild while it holds
    // (build_list), dropped -- plan = {} -- by whatever changes the facts it was chosen for
    BrickPlan plan;
    const bool &brick_active = plan.active;   // (read-only: the brick kernels are in use, not the direct ones)
    struct PlanBlocks {                   // what this state has ruled out until the next load
        bool field16 = false;             // a 16-bit hit field overflowed under a plan that should have ruled it out: 32-bit fields
        bool typed = false;               // its rows outgrew the typed build
    } blocked;

    DevBuf<Rec<real>> rec, rec2;
    DevBuf<float> te, te2;
    DevBuf<real> vel, vel2, frc, en, vir, im, im2, xb, noise;
    DevBuf<int> perm, perm2, inv_perm, cell_of, cell_sorted, cell_sorted2, order, count, fill, nbr, cnt, flags, img, img2;
    DevBuf<int2> tmp2;                    // {id, sort key} in arrival order inside each cell (bin)
    // 64-bit ids that travel with the atoms through every sort (decomposed domains: the GLOBAL ids, owned atoms and ghosts).
    // With them the order inside a cell is by the low word of the tag, not by the local id: the cell order -- and with it the
    // order of every neighbour row and force sum -- no longer depends on how a domain numbers its atoms, i.e. on the history
    // of migrations or on the path a rebuild took (counted, count-free, in the engine's own order).
    DevBuf<long long> tag, tag2;
    bool use_tags = false;
    size_t cap_hint = 0;                  // reserve() sizes the per-atom arrays (and the plane pitch) for at least this many slots
    size_t capacity = 0;                  // ... what they hold
    bool has_ghosts = false;
    // ids: perm[p] < n_owned <=> owned.  After resort_edit the ids in use have gaps (id_space > n_total); callers that want
    // dense caller-order arrays get them through ids_map() (rank of every id in use: owned first, then ghosts)
    int id_space = 0;
    bool id_gaps = false;
    DevBuf<int> cmap;
    bool cmap_valid = false;
    // typed boxes (two species): sort digit = cell * nt + species; count[] then holds the per-(cell, species) starts and
    // cstart[] the per-cell ones every untyped consumer reads
    SpeciesTable species{1, {0, 0, 0, 0}};
    int nt = 1;
    // untyped boxes on the brick path: a cell's atoms ordered by quarter along x (kernels.hpp XSubBin), digit = cell * nsub + quarter
    int nsub = 1;
    bool subbins_enabled = std::getenv("EMDEE_NO_SUBBINS") == nullptr;
    // two-species boxes on the brick path (round 5): the typed build takes the same quarters, digit = (cell * 2 + species) * 4 + quarter
    // (EMDEE_TYPED_SUBBINS=0: the (cell, species) order of rounds 3-4, the A/B baseline)
    int tsub = 1;
    bool typed_subbins_enabled = std::getenv("EMDEE_TYPED_SUBBINS") == nullptr || std::atoi(std::getenv("EMDEE_TYPED_SUBBINS")) != 0;
    int digits() const { return nt > 1 ? nt * tsub : nsub; }
    DevBuf<int> bsub;
    bool typed_enabled = std::getenv("EMDEE_NO_TYPED") == nullptr;
    DevBuf<int> cstart;
    DevBuf<unsigned long long> species_tab;
    DevBuf<unsigned short> nbr16;
    DevBuf<int> btab;                     // per-brick tables of the current list (k_brick_tables)
    bool btab_valid = false;
    DevBuf<unsigned long long> stats;
    Scanner scanner;

    NbSystem() {
        refuse_experiment_switches();
        if (const char *e = std::getenv("EMDEE_PATH")) path = (std::string(e) == "direct") ? PATH_DIRECT : PATH_BRICK;
        if (const char *e = std::getenv("EMDEE_RUN_AHEAD")) run_ahead = std::max(1, std::min(RUN_AHEAD, std::atoi(e)));
    }

    hipStream_t stream() const { return ctx->stream; }
    AtomView<real> view() const { return AtomView<real>{rec.ptr, te.ptr, rel_grid(rel_now, cell_sorted.ptr)}; }

    // ---- cell-relative records (kernels.hpp RelGrid): fp32 integrators on the tiled path, undivided boxes ----
    // rel_now: what the records of the CURRENT sorted state are; decided anew at every sort (rel_wanted), the gather kernels
    // read one representation and write the other.  EMDEE_F32_ABS=1 keeps absolute fp32 records (the A/B baseline: rounds 1-4).
    bool rel_now = false;
    double rel_lo[3] = {0, 0, 0}, rel_cw[3] = {1, 1, 1};
    int rel_M[3] = {1, 1, 1};
    bool rel_wanted() const {
        return sizeof(real) == 4 && with_vel && !with_mass && !use_tags && !has_ghosts && path == PATH_BRICK &&
               std::getenv("EMDEE_F32_ABS") == nullptr;
    }
    RelGrid rel_grid(bool on, const int *cells) const {
        RelGrid r{};
        for (int d = 0; d < 3; d++) { r.lo[d] = rel_lo[d]; r.cw[d] = rel_cw[d]; r.M[d] = rel_M[d]; }
        r.on = on ? 1 : 0;
        r.cell = cells;
        return r;
    }
    // the grid the NEXT sorted state's records will be relative to (call after configure_grid)
    RelGrid rel_grid_next(bool on, const int *cells) const {
        RelGrid r{};
        for (int d = 0; d < 3; d++) { r.lo[d] = (double)grid.lo[d]; r.cw[d] = (double)grid.len[d] / (double)grid.M[d]; r.M[d] = grid.M[d]; }
        r.on = on ? 1 : 0;
        r.cell = cells;
        return r;
    }
    void rel_commit(bool on) {
        rel_now = on;
        for (int d = 0; d < 3; d++) { rel_lo[d] = (double)grid.lo[d]; rel_cw[d] = (double)grid.len[d] / (double)grid.M[d]; rel_M[d] = grid.M[d]; }
    }

    struct Timed {
        NbSystem *s;
        int id;
        size_t k = 0;
        Timed(NbSystem *sys, int which) : s(sys), id(which) {
            if (s->profiling) k = s->timers[id].begin(s->stream());
        }
        ~Timed() {
            if (s->profiling) s->timers[id].end(k, s->stream());
        }
    };
    // a launch, timed under `timer` when that is a TimerId and not -1
    template <class Launch>
    void timed_if(int timer, Launch &&launch) {
        if (timer < 0) { launch(); return; }
        Timed t(this, timer);
        launch();
    }

    // ---------------------------------------------------------------- box sums (reduce.hpp)
    // The scratch of every two-stage sum: the blocks' partials, sized for the widest term and shared by all (the stream orders their
    // users), and behind them the totals in fixed slots, so that totals which one launch or one copy reads together never alias.
    // The energy sums lie right behind FIRE's six words (fire_sums: one copy of seven), the molecules' tensor sums right behind the
    // atomic ones (molecular_tensor_sums: one copy of twenty-four; k_gk_push reads those and the heat sums in one launch).
    enum RedSlot { RED_FIRE = 0, RED_ENERGY = 6, RED_TENSOR = 9, RED_MOLECULE = 21, RED_HEAT = 33, RED_RESTRAINT = 36, RED_ALCH = 44,
                   RED_ALCH_FOREIGN = 48, RED_ALCH_COULOMB = 64, RED_ALCH_COULOMB_FOREIGN = 68, RED_TOTALS = 84 };
    DevBuf<double> red;
    double *red_partials() {
        red.ensure((size_t)RED_MAX_WORDS * RED_MAX_BLOCKS + RED_TOTALS);
        return red.ptr;
    }
    // The two stages of `term` over n > 0 elements, queued on the stream, nothing read back: the device address of the totals in
    // `slot`.  timer >= 0: each launch is timed under it.  The halves are for a caller that times them apart (the molecule pass) or
    // completes the sum in a kernel of its own (the thermostat): queue_partials returns the number of blocks, which stage 2 takes.
    template <class Term>
    int queue_partials(int n, const Term &term, int timer = -1) {
        const int nb = red_blocks(n);
        double *partial = red_partials();
        timed_if(timer, [&] { hipLaunchKernelGGL((k_reduce_partials<Term>), dim3(nb), dim3(RED_BLOCK), 0, stream(), n, term, partial); });
        return nb;
    }
    template <class Term>
    double *queue_final(int nb, int slot, int timer = -1) {
        const double *partial = red_partials();
        double *tot = red.ptr + (size_t)RED_MAX_WORDS * RED_MAX_BLOCKS + slot;
        timed_if(timer, [&] {
            hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(RED_BLOCK), 0, stream(), nb, Term::SUMS, Term::MAXES, partial, tot);
        });
        return tot;
    }
    template <class Term>
    double *queue(int n, const Term &term, int slot, int timer = -1) {
        return queue_final<Term>(queue_partials(n, term, timer), slot, timer);
    }

    // ---------------------------------------------------------------- geometry
    void set_box(const double lo_[3], const double len_[3], const int per_[3]) {
        bool same = true;
        for (int d = 0; d < 3; d++) same = same && lo[d] == lo_[d] && len[d] == len_[d] && per[d] == (per_[d] ? 1 : 0);
        if (!same) { sorted = has_list = false; plan = {}; }
        for (int d = 0; d < 3; d++) {
            lo[d] = lo_[d]; len[d] = len_[d]; per[d] = per_[d] ? 1 : 0;
            EMDEE_REQUIRE(len[d] > 0.0 && std::isfinite(len[d]), EMDEE_ERR_INVALID, "box length must be positive");
        }
    }

    void set_model(const emdee_lj_model &m, double skin_) {
        EMDEE_REQUIRE(m.rc2 > 0 && m.rs2 >= 0 && m.rs2 < m.rc2 && std::isfinite(m.inv_delta2), EMDEE_ERR_INVALID,
                      "LennardJonesModel needs 0 <= switch < cutoff (Q10: switch == cutoff gives 1/0)");
        EMDEE_REQUIRE(skin_ >= 0.0, EMDEE_ERR_INVALID, "skin must be >= 0");
        if (m.rc2 != model_d.rc2 || skin_ != skin) { has_list = sorted = false; plan = {}; }
        model_d = m;
        model = make_model<real>(m);
        skin = skin_;
        rlist = std::sqrt(m.rc2) + skin;
    }

    void configure_grid() {
        GridP<real> g{};
        size_t cells = 1;
        int M[3];
        for (int d = 0; d < 3; d++) {
            if (per[d])
                EMDEE_REQUIRE(rlist <= 0.5 * len[d], EMDEE_ERR_INVALID,
                              "cutoff + skin = %g exceeds half the periodic box length %g (minimum image)", rlist, len[d]);
            M[d] = std::max(1, (int)std::floor(len[d] / rlist));   // cell side >= rlist: 27-cell stencil
            M[d] = std::min(M[d], 1024);
        }
        // sparse boxes: never more cells than ~4 per atom (larger cells stay valid)
        while ((size_t)M[0] * M[1] * M[2] > 4 * (size_t)std::max(n_total, 16) + 64) {
            int big = 0;
            for (int d = 1; d < 3; d++)
                if (M[d] > M[big]) big = d;
            if (M[big] <= 1) break;
            M[big] = (M[big] + 1) / 2;
        }
        for (int d = 0; d < 3; d++) {
            g.lo[d] = (real)lo[d]; g.len[d] = (real)len[d];
            g.plen[d] = per[d] ? (real)len[d] : (real)0;
            g.pinv[d] = per[d] ? (real)(1.0 / len[d]) : (real)0;
            g.per[d] = per[d];
            g.M[d] = M[d];
            cells *= (size_t)M[d];
        }
        g.nd = 1;
        g.one_based = 0;
        grid = g;
        ncell = cells;
    }

    void reserve(int n, bool velocities, bool masses) {
        n_total = n;
        const size_t m = std::max((size_t)n, cap_hint);
        capacity = m;
        pitch = (m + 63) / 64 * 64 + 64;
        with_vel = velocities;
        with_mass = masses;
        rec.ensure(m + 1); rec2.ensure(m + 1);
        if (sizeof(real) == 4) { te.ensure(m + 1); te2.ensure(m + 1); }
        frc.ensure(3 * pitch); en.ensure(pitch); vir.ensure(pitch); xb.ensure(3 * pitch);
        if (velocities) { vel.ensure(3 * pitch); vel2.ensure(3 * pitch); }
        if (masses) { im.ensure(pitch); im2.ensure(pitch); }
        perm.ensure(m + 1); perm2.ensure(m + 1); inv_perm.ensure(m + 1); img.ensure(m + 1); img2.ensure(m + 1);
        cell_of.ensure(m + 1); cell_sorted.ensure(m + 1); cell_sorted2.ensure(m + 1); order.ensure(m + 1); cnt.ensure(m + 1);
        if (use_tags) { tag.ensure(m + 1); tag2.ensure(m + 1); }
        if (flags.ensure(32)) EMDEE_HIP_CHECK(hipMemsetAsync(flags.ptr, 0, 32 * sizeof(int), stream()));
        red_partials(); stats.ensure(4);
    }

    // ---------------------------------------------------------------- binning
    // n_items / tagkey / keep: see resort_edit (items struck out by keep[] take no part; the number that do is count[nbins])
    template <class Src, class Spc>
    void bin(Src src, const int *key, Spc spc, int n_items = -1, const long long *tagkey = nullptr, const unsigned char *keep = nullptr) {
        const int n = n_items >= 0 ? n_items : n_total;
        const int dm = digits();
        const size_t nbins = ncell * (size_t)dm;
        count.ensure(nbins + 2); fill.ensure(nbins + 2);
        Zeros zr;
        zr.add(count.ptr, nbins + 1).add(fill.ptr, nbins);
        if (dm > 1) {
            cstart.ensure(ncell + 2);
            if (n == 0) zr.add(cstart.ptr, ncell + 1);
        }
        zr.run(stream());
        if (n == 0) return;
        hipLaunchKernelGGL((k_cell_assign<real, Src, Spc>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, src, grid,
                           cell_of.ptr, count.ptr, spc, dm, keep);
        scanner.run(count.ptr, nbins + 1, stream());   // count[] becomes the start of every (cell, species / sub-bin) block
        tmp2.ensure(std::max((size_t)n, capacity) + 1);
        hipLaunchKernelGGL(k_cell_scatter_keyed, dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, cell_of.ptr, count.ptr,
                           fill.ptr, key, tmp2.ptr, tagkey);
        hipLaunchKernelGGL(k_cell_rankfix_keyed, dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, cell_of.ptr, count.ptr,
                           tmp2.ptr, order.ptr, keep ? count.ptr + nbins : nullptr, tagkey != nullptr ? 1 : 0);
        // (the first slot of every cell, cstart[], is written by the gather kernel that follows)
    }
    // K of the x sub-bins (plan.hpp plan_sub_k)
    int sub_k() const { return plan_sub_k((int)sizeof(real), len[0], grid.M[0], rlist); }
    // sub-bins only where the round-robin two-phase build can use them: the tiled path of an untyped box
    void choose_subbins() {
        nsub = (subbins_enabled && path == PATH_BRICK && nt == 1 && n_total > 0) ? 4 : 1;
        tsub = (subbins_enabled && typed_subbins_enabled && typed_enabled && path == PATH_BRICK && nt == 2 && n_total > 0) ? 4 : 1;
    }
    template <class Src, class Spc>
    void bin_species(Src src, const int *key, Spc spc, int n_items = -1, const long long *tagkey = nullptr, const unsigned char *keep = nullptr) {
        using Sub = XSubBin<real, Src>;
        if (tsub > 1) bin(src, key, SpeciesSub<Spc, Sub>{spc, Sub{src, grid.lo[0], grid.len[0], grid.M[0], grid.per[0], tsub}}, n_items, tagkey, keep);
        else bin(src, key, spc, n_items, tagkey, keep);
    }
    template <class Src>
    void bin_untyped(Src src, const int *key, int n_items = -1, const long long *tagkey = nullptr, const unsigned char *keep = nullptr) {
        if (nsub > 1) bin(src, key, XSubBin<real, Src>{src, grid.lo[0], grid.len[0], grid.M[0], grid.per[0], nsub}, n_items, tagkey, keep);
        else bin(src, key, NoSpecies{}, n_items, tagkey, keep);
    }
    const int *start() const { return digits() > 1 ? cstart.ptr : count.ptr; }   // first slot of every cell
    const int *tstart() const { return count.ptr; }                        // ... of every (cell, species) block (typed boxes)

    // caller-order arrays -> cell-ordered state (+ list)
    // (tags_user, optional: 64-bit ids in caller order, owned atoms and ghosts -- see `tag`)
    void load_user(int n_own, int n_ghost, const real *pos, const real *velocities, const emdee_lj_atom *atoms,
                   const real *inv_mass, const long long *tags_user = nullptr) {
        EMDEE_REQUIRE(n_own >= 0 && n_ghost >= 0, EMDEE_ERR_INVALID, "negative atom count");
        EMDEE_REQUIRE((int64_t)n_own + n_ghost < (int64_t)1 << 31, EMDEE_ERR_INVALID, "too many atoms");
        EMDEE_REQUIRE(n_own + n_ghost == 0 || (pos && atoms), EMDEE_ERR_INVALID, "positions/atoms are NULL");
        Timed t(this, T_REBUILD);
        n_owned = n_own;
        has_ghosts = n_ghost > 0;
        id_space = n_own + n_ghost; id_gaps = false; cmap_valid = false;
        lgv_ids = nullptr;                                   // caller-order array of the previous state
        use_tags = tags_user != nullptr;
        reserve(n_own + n_ghost, velocities != nullptr || with_vel, inv_mass != nullptr);
        if (image_limit) image_fault.reset(flags.ptr, stream());   // (a new state: its counts start from the caller's positions)
        detect_uniform_atoms(atoms);
        configure_grid();
        const int n = n_total;
        const bool rel_next = rel_wanted();
        choose_subbins();
        if (nt > 1) bin_species(UserPos<real>{pos}, nullptr, UserSpecies{species, atoms}, -1, use_tags ? tags_user : nullptr);
        else bin_untyped(UserPos<real>{pos}, nullptr, -1, use_tags ? tags_user : nullptr);
        if (n > 0)
            hipLaunchKernelGGL((k_gather_user<real>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, n_owned, pitch,
                               grid, order.ptr, cell_of.ptr, pos, atoms, velocities, inv_mass, rec.ptr, te.ptr, xb.ptr,
                               with_vel ? vel.ptr : nullptr, with_mass ? im.ptr : nullptr, perm.ptr, inv_perm.ptr,
                               cell_sorted.ptr, img.ptr, digits(), use_tags ? tags_user : nullptr, use_tags ? tag.ptr : nullptr,
                               (int)ncell, digits() > 1 ? cstart.ptr : nullptr, count.ptr, rel_grid_next(rel_next, nullptr),
                               image_word());
        rel_commit(rel_next);
        q_valid = false;
        // ghosts are never written by the step kernel: both position buffers carry their records (LJAtom fields)
        // from the start; their coordinates are refreshed by every halo unpack
        if (has_ghosts)
            hipLaunchKernelGGL((k_copy_ghost_records<real>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, n_owned,
                               perm.ptr, rec.ptr, rec2.ptr);
        sorted = true;
        build_list();
        if (image_limit && image_words[0] != 0) {            // (the state's positions could not be handed back: no state)
            sorted = false; has_list = false;
            image_fault.reset(flags.ptr, stream());
            EMDEE_REQUIRE(false, EMDEE_ERR_INVALID, "set_state: atom %d lies %d box lengths from the box along axis %d: the image count "
                          "kept per atom holds -512 .. 511 (positions up to 500 box lengths away are always accepted)",
                          image_words[0] - 1, image_words[2], image_words[1]);
        }
    }
    // An engine that hands positions back in the caller's image (emdee_md_get_state) keeps a count per atom and axis that must stay
    // in its field (kernels.hpp img_bound).  The gathers raise flags[W_IMAGE ..]; the words come back with every build's read-back
    // (image_words), a load refuses on them and a rebuild latches image_fault: the engine refuses to step until the state is replaced.
    bool image_limit = false;
    FaultWord image_fault{W_IMAGE};
    int32_t image_words[3] = {0, 0, 0};
    int *image_word() const { return image_limit ? flags.ptr + W_IMAGE : nullptr; }

    // re-bin / re-sort the current state (MD rebuild)
    void resort() {
        EMDEE_REQUIRE(sorted, EMDEE_ERR_STATE, "no state loaded");
        Timed t(this, T_REBUILD);
        const int n = n_total;
        configure_grid();
        choose_subbins();
        const long long *tk = use_tags ? tag.ptr : nullptr;
        const RelGrid rel_in = rel_grid(rel_now, cell_sorted.ptr);   // (the cells the current records are relative to: read before the grid may change)
        const bool rel_next = rel_wanted();
        if (nt > 1) bin_species(RecPos<real>{rec.ptr, rel_in}, perm.ptr, RecSpecies<real>{species, rec.ptr, te.ptr}, -1, tk);
        else bin_untyped(RecPos<real>{rec.ptr, rel_in}, perm.ptr, -1, tk);
        if (n > 0)
            hipLaunchKernelGGL((k_gather_sorted<real, false>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, pitch, grid,
                               order.ptr, cell_of.ptr, rec.ptr, te.ptr, with_vel ? vel.ptr : nullptr,
                               with_mass ? im.ptr : nullptr, perm.ptr, img.ptr, rec2.ptr, te2.ptr, xb.ptr,
                               with_vel ? vel2.ptr : nullptr, with_mass ? im2.ptr : nullptr, perm2.ptr, inv_perm.ptr,
                               cell_sorted2.ptr, img2.ptr, digits(), tk, use_tags ? tag2.ptr : nullptr, (const int *)nullptr,
                               (int *)nullptr, (int)ncell, digits() > 1 ? cstart.ptr : nullptr, count.ptr, rel_in,
                               rel_grid_next(rel_next, nullptr), image_word());
        swap_sorted_buffers();
        rel_commit(rel_next);
        build_list();
        if (image_limit && image_words[0] != 0 && !image_fault.latched) {
            image_fault.latched = true;
            EMDEE_REQUIRE(false, EMDEE_ERR_STATE, "rebuild: atom %d has travelled %d box lengths from the box along axis %d: the image "
                          "count kept per atom holds -512 .. 511; its unwrapped position is lost (every other atom's is intact): replace "
                          "the state", image_words[0] - 1, image_words[2], image_words[1]);
        }
    }
    // emdee_md_scale_box: can the box take the factors mu?  (checked before anything is written)
    void check_scaled_box(const double mu[3], double vscale) const {
        for (int d = 0; d < 3; d++)
            EMDEE_REQUIRE(std::isfinite(mu[d]) && mu[d] > 0.0, EMDEE_ERR_INVALID, "scale_box: mu[%d] = %g must be finite and > 0", d, mu[d]);
        EMDEE_REQUIRE(std::isfinite(vscale) && vscale > 0.0, EMDEE_ERR_INVALID, "scale_box: velocity_scale = %g must be finite and > 0", vscale);
        for (int d = 0; d < 3; d++) {
            const double nl = mu[d] * len[d];
            EMDEE_REQUIRE(std::isfinite(nl) && nl > 0.0, EMDEE_ERR_INVALID, "scale_box: the new box length %g along %d is not finite and > 0", nl, d);
            EMDEE_REQUIRE(!per[d] || nl >= 2.0 * rlist, EMDEE_ERR_INVALID, "scale_box: the new periodic box length %g along dimension %d is below "
                          "2 (cutoff + skin) = %g (minimum image)", nl, d, 2.0 * rlist);
        }
    }
    // ... then: the sorted state rescaled in place (k_cell_state_scale), the box mu_d len_d, and the re-sort -- new cells, a new
    // plan when the box changed (set_box), the list, the 1-4 and bonded slots, the charge plane at the next force pass.
    // No read-back of its own: mu and vscale are the caller's host values.
    // molecular (emdee_md_set_molecular_scaling, an engine with a rigid table or a molecule table): the atoms of the table move with
    // their molecules' centres of mass (molecule_table(): k_molecule_centres and k_molecule_shift over the molecule table, else
    // k_molecule_scale over the triangles) and k_cell_state_scale passes them over; every other atom scales as before.  Neither
    // kernel reads what the other writes.
    void scale_box(const double mu[3], double vscale, bool molecular = false) {
        EMDEE_REQUIRE(sorted && with_vel && !has_ghosts, EMDEE_ERR_STATE, "scale_box: needs a loaded state without ghosts");
        check_scaled_box(mu, vscale);
        if (n_total > 0) {
            ScaleBox s{};
            for (int d = 0; d < 3; d++) { s.lo[d] = lo[d]; s.mu[d] = mu[d]; }
            const int scale_vel = vscale != 1.0 ? 1 : 0;
            const Topology::MoleculeTable *mt = molecular ? molecule_table() : nullptr;
            if (mt && mt->n > 0) {
                queue_molecule_centres(*mt, T_MOLECULAR);
                Timed t(this, T_MOLECULAR);
                hipLaunchKernelGGL((k_molecule_shift<real>), dim3(blocks_for(mt->n_entries, 256)), dim3(256), 0, stream(), molecule_args(*mt), s,
                                   vscale, scale_vel);
            } else if (molecular && !mt && tables->rigid.n > 0) {
                Timed t(this, T_MOLECULAR);
                hipLaunchKernelGGL((k_molecule_scale<real>), dim3(blocks_for(tables->rigid.n, 256)), dim3(256), 0, stream(), settle_args(), s,
                                   vscale, scale_vel);
            }
            const unsigned char *member = !molecular ? nullptr : mt ? mt->member.ptr : tables->r_member.ptr;
            hipLaunchKernelGGL((k_cell_state_scale<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, pitch, rec.ptr,
                               vel.ptr, s, (real)vscale, scale_vel, rel_grid(rel_now, cell_sorted.ptr), member,
                               molecular ? (const int *)perm.ptr : (const int *)nullptr);
            if (has_restraints() && tables->restraints.n > 0) {   // (the references follow the box: ref <- lo + mu (ref - lo))
                Timed t(this, T_RESTRAINTS);
                hipLaunchKernelGGL(k_restraint_scale, dim3(blocks_for(tables->restraints.n, 256)), dim3(256), 0, stream(), tables->restraints.n,
                                   tables->restraints.ref.ptr, s);
            }
        }
        const double nl[3] = {mu[0] * len[0], mu[1] * len[1], mu[2] * len[2]};
        set_box(lo, nl, per);                                // (a changed box invalidates the sort, the list and the plan ...)
        sorted = true;                                       // ... but the records are this state's: the re-sort reads them
        if (vsites_fit()) place_sites(false);                // (sites back on their scaled parents, on the new box lengths, before the rebuild)
        resort();
    }
    void swap_sorted_buffers() {
        q_valid = false;                                     // (the charge plane is the previous order's)
        rec.swap(rec2); te.swap(te2); perm.swap(perm2); img.swap(img2); cell_sorted.swap(cell_sorted2);
        if (with_vel) vel.swap(vel2);
        if (with_mass) im.swap(im2);
        if (use_tags) tag.swap(tag2);
    }

    // ---------------------------------------------------------------- a decomposed domain's rebuild in its own order (dd.hpp)
    // The state is re-sorted from its OWN records -- no caller-order copy, no assembly of new caller arrays, no load:
    //  * keep[q] == 0 strikes slot q out (atoms that left for a neighbour, the old ghosts, the unused rows of padded messages);
    //  * the arrivals and the new ghosts have been written behind the old state, slots [n_total, n_items), by the caller --
    //    records (both LJAtom fields), velocity planes, tags;
    //  * the OLD slot q is an atom's id from now on: ids >= own_limit are ghosts (the ids in use have gaps: ids_map()).
    // How many atoms that leaves is a device word (*n_live_dev) until the build's read-back, which carries the caller's words
    // (`extra`: counts and overflow words of the messages) along: ONE blocking read-back for the whole rebuild.  The kernels in
    // between run over n_items.  The old state stays intact in the spare buffers until commit_edit(): when a message of the
    // rebuild turns out to have overflowed, rollback_edit() puts it back and the caller redoes the rebuild with counts.
    struct EditWords {
        const int *dev = nullptr;
        int n = 0;
        int32_t *host = nullptr;
    };
    bool in_edit = false, edit_abort = false;
    EditWords edit_extra{};
    int edit_n_plan = 0;
    struct EditSaved { int n_total, n_owned, id_space; bool id_gaps, has_ghosts, has_list; } edit_saved{};
    bool edit_fits(int n_items) const { return sorted && use_tags && with_vel && !with_mass && (size_t)n_items <= capacity; }
    bool edit_extra_read = false;
    bool resort_edit(int n_items, const unsigned char *keep, int own_limit, bool ghosts, int *n_live_dev, EditWords extra) {
        EMDEE_REQUIRE(edit_fits(n_items), EMDEE_ERR_STATE, "resort_edit: the state does not hold %d slots", n_items);
        Timed t(this, T_REBUILD);
        edit_saved = EditSaved{n_total, n_owned, id_space, id_gaps, has_ghosts, has_list};
        configure_grid();
        choose_subbins();
        EMDEE_REQUIRE(!rel_now, EMDEE_ERR_STATE, "resort_edit: cell-relative records (decomposed domains keep absolute ones)");
        if (nt > 1) bin_species(RecPos<real>{rec.ptr, RelGrid{}}, nullptr, RecSpecies<real>{species, rec.ptr, te.ptr}, n_items, tag.ptr, keep);
        else bin_untyped(RecPos<real>{rec.ptr, RelGrid{}}, nullptr, n_items, tag.ptr, keep);
        const size_t nbins = ncell * (size_t)digits();
        hipLaunchKernelGGL((k_gather_sorted<real, true>), dim3(blocks_for(n_items, 256)), dim3(256), 0, stream(), n_items, pitch, grid,
                           order.ptr, cell_of.ptr, rec.ptr, te.ptr, vel.ptr, (const real *)nullptr, perm.ptr, img.ptr, rec2.ptr, te2.ptr,
                           xb.ptr, vel2.ptr, (real *)nullptr, perm2.ptr, inv_perm.ptr, cell_sorted2.ptr, img2.ptr, digits(), tag.ptr,
                           tag2.ptr, count.ptr + nbins, n_live_dev, (int)ncell, digits() > 1 ? cstart.ptr : nullptr, count.ptr);
        swap_sorted_buffers();
        edit_n_plan = n_total;
        n_total = n_items;                                  // an upper bound until commit_edit()
        n_owned = own_limit;
        has_ghosts = ghosts;
        id_space = n_items; id_gaps = true; cmap_valid = false;
        in_edit = true; edit_abort = false; edit_extra = extra; edit_extra_read = false;
        struct Leave { bool &f; ~Leave() { f = false; } } leave{in_edit};
        // (an engine on the direct kernels, or without atoms so far: they count atoms on the host -- the re-sorted state is
        // complete, the caller reads the counts and loads the engine from it)
        if (path == PATH_BRICK && plan.active && edit_saved.n_total > 0) build_list();
        else edit_abort = true;
        if (edit_abort && !edit_extra_read && extra.n > 0) read_back_words(ctx, stream(), extra.dev, extra.n, extra.host);
        return !edit_abort;
    }
    void commit_edit(int n_live) {
        EMDEE_REQUIRE(n_live >= 0 && n_live <= n_total, EMDEE_ERR_STATE, "resort_edit: %d atoms in %d slots", n_live, n_total);
        n_total = n_live;
        // ghosts are never written by the step kernel: both position buffers carry their records from the start (only now:
        // until here the spare buffer held the state to roll back to)
        if (has_ghosts && n_total > 0)
            hipLaunchKernelGGL((k_copy_ghost_records<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned,
                               perm.ptr, rec.ptr, rec2.ptr);
    }
    void rollback_edit() {
        swap_sorted_buffers();
        n_total = edit_saved.n_total; n_owned = edit_saved.n_owned; id_space = edit_saved.id_space;
        id_gaps = edit_saved.id_gaps; has_ghosts = edit_saved.has_ghosts;
        cmap_valid = false;
        has_list = false; plan = {}; btab_valid = false;   // (inv_perm, xb, the cell tables and the list are the discarded sort's)
    }
    // rank of every id in use among the ids in use (NULL: the ids have no gaps)
    const int *ids_map() {
        if (!id_gaps) return nullptr;
        if (!cmap_valid) {
            cmap.ensure((size_t)id_space + 2);
            EMDEE_HIP_CHECK(hipMemsetAsync(cmap.ptr, 0, ((size_t)id_space + 1) * sizeof(int), stream()));
            if (n_total > 0) hipLaunchKernelGGL(k_mark_live, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, perm.ptr, cmap.ptr);
            scanner.run(cmap.ptr, (size_t)id_space + 1, stream());
            cmap_valid = true;
        }
        return cmap.ptr;
    }

    // ---------------------------------------------------------------- brick plumbing
    BrickArgs<real> brick_args(const Pass<real> &p = {}) {
        BrickArgs<real> a{};
        a.n = n_total; a.n_owned = n_owned; a.any_ghosts = has_ghosts ? 1 : 0;
        a.rec = rec.ptr; a.te = te.ptr; a.perm = perm.ptr; a.start = start();
        a.g = grid; a.bg = plan.grid; a.tile_cap = plan.tile_cap; a.own_cap = plan.own_cap;
        a.nbr = nbr16.ptr; a.stride = stride; a.cnt = cnt.ptr; a.flags = flags.ptr;
        a.rlist2 = (real)(rlist * rlist); a.margin = plan.build_margin; a.model = model; a.pitch = pitch;
        a.frc = frc.ptr; a.en = en.ptr; a.vir = vir.ptr; a.stats = stats.ptr;
        if (p.spare_unselected) {
            if (!(p.mask & EMDEE_FORCES)) a.frc = spare.ptr;
            if (!(p.mask & EMDEE_ENERGIES)) a.en = spare.ptr + 3 * pitch;
            if (!(p.mask & EMDEE_VIRIALS)) a.vir = spare.ptr + 4 * pitch;
        }
        a.phase = p.phase;
        a.vel = vel.ptr; a.vel_next = vel2.ptr; a.xb = xb.ptr; a.inv_mass = with_mass ? im.ptr : nullptr; a.rec_next = rec2.ptr;
        a.kick_c = (real)p.c; a.dt = (real)p.dt;
        a.uni_sigma2 = (real)uni_sigma2; a.uni_e4 = (real)uni_e4;
        a.uni = make_uni<real>(model, (real)uni_sigma, (real)uni_e4);
        a.idx_shift = plan.idx_shift;
        a.tstart = tstart(); a.tdig = nt > 1 ? tsub : 1;
        a.nsub = nsub; a.fstart = tstart(); a.bsub = nsub > 1 ? bsub.ptr : nullptr;
        a.sub_k = sub_k();
        for (int q = 0; q < 4; q++) { a.tsig2[q] = (real)0; a.te4[q] = (real)0; }
        if (nt == 2) {
            // sigma_ij^2 and 4 eps_ij of the four species pairs, with the operations the general-species pair loop uses
            for (int i = 0; i < 2; i++)
                for (int j = 0; j < 2; j++) {
                    float hi, ti, hj, tj;
                    species_atom(i, hi, ti); species_atom(j, hj, tj);
                    const real sg = (real)hi + (real)hj;
                    a.tsig2[i * 2 + j] = sg * sg;
                    a.te4[i * 2 + j] = (real)ti * (real)tj;
                }
        }
        a.rel = rel_now ? 1 : 0;
        for (int d = 0; d < 3; d++) { a.rcw[d] = rel_cw[d]; a.rlo[d] = rel_lo[d]; }
        a.refmath = ref_tiles(p) ? 1 : 0;
        a.user_pos = p.pos;
        a.thr2 = (real)(0.25 * skin * skin);
        a.trigger = p.trigger ? p.trigger : flags.ptr + 1;
        a.guard = p.guard;
        a.btab = btab_valid ? btab.ptr : nullptr;
        a.user_f = p.f; a.user_e = p.e; a.user_w = p.w;
        a.vt = vt.ptr; a.user_vt = p.vt;
        a.noise = lgv_on ? noise.ptr : nullptr; a.lgv_c1 = lgv_on ? (real)lgv_c1 : (real)1;
        a.chg = charge_args();
        return a;
    }

    void species_atom(int k, float &hs, float &te) const {
        const unsigned lo = (unsigned)(species.key[k] & 0xffffffffull), hi = (unsigned)(species.key[k] >> 32);
        memcpy(&hs, &lo, 4); memcpy(&te, &hi, 4);
    }
    // only force and step launches are phased: the stats launch takes a default Pass and covers every brick
    template <class V, class K>
    void launch_bricks(K kernel, size_t lds, const Pass<real> &p) {
        allow_big_lds(kernel, lds);
        const int blocks = (p.phase == 1 ? plan.grid.ib_per_xcd : p.phase == 2 ? plan.grid.bb_per_xcd : plan.grid.per_xcd) * NXCD;
        if (blocks == 0) return;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(V::THREADS), lds, stream(), brick_args(p));
    }
    // The tables of every brick, once per rebuild; the build and every force launch copy them in (brick.hpp k_brick_tables).
    // NT = 1 or TNT (species-major tables); sub = 4 when the sort orders a block's atoms by x quarter: the boundaries of every
    // brick's blocks go to bsub as well.  Returns the arguments the kernel ran with.
    // (the image depends on the brick shape only: a small workgroup writes it)
    template <class V, int NT>
    BrickArgs<real> launch_tables(int sub) {
        constexpr int TT = (NT > 1 || V::Shape::NTC > 128) ? 256 : 128;
        using BT = BrickTables<typename V::Shape, TT, NT>;
        static_assert(BT::row_ints() == BrickTables<typename V::Shape, V::THREADS, NT>::row_ints(), "table row layout");
        btab.ensure((size_t)plan.grid.nbricks * BT::row_ints());
        btab_valid = false;
        BrickArgs<real> ta = brick_args();
        ta.btab = btab.ptr;
        if (sub > 1) {
            bsub.ensure((size_t)plan.grid.nbricks * BT::NTT + 4);
            ta.nsub = sub; ta.bsub = bsub.ptr;
        }
        hipLaunchKernelGGL((k_brick_tables<real, typename V::Shape, TT, NT>), dim3(plan.grid.per_xcd * NXCD), dim3(TT), BT::bytes(0), stream(), ta);
        btab_valid = true;
        return ta;
    }
    template <class V, int NT>
    void launch_export(int *counts, int *out, int capacity, const int *map) {
        auto kernel = k_brick_export<real, typename V::Shape, V::THREADS, V::G, NT>;
        const size_t lds = BrickTables<typename V::Shape, V::THREADS, NT>::bytes(0);
        hipLaunchKernelGGL(kernel, dim3(plan.grid.per_xcd * NXCD), dim3(V::THREADS), lds, stream(), brick_args(), counts, out, capacity, map);
    }
    // typed boxes (typed.hpp): masks other than FORCES run the all-outputs kernel
    template <class V, int MODE, int BM>
    void launch_typed_kernel(const Pass<real> &p) {
        if constexpr (typed_variant<V>()) {
            constexpr int M = (MODE == BRICK_STATS) ? 0 : ((MODE == BRICK_STEP || BM == 1) ? 1 : BM == TENSOR_PASS ? TENSOR_PASS : 7);
            launch_bricks<V>(k_typed<real, typename V::Shape, V::THREADS, V::G, MODE, M>, plan.lds_force, p);
        }
    }

    // the Float32 reference arithmetic of an operator call: general-species tiles staged from the caller's positions
    bool ref_tiles(const Pass<real> &p) const { return sizeof(real) == 4 && refmath && p.pos != nullptr; }
    template <class V, int MODE, int BM>
    void launch_brick_kernel(const Pass<real> &p) {
        if (plan.typed) { launch_typed_kernel<V, MODE, BM>(p); return; }
        // charged engines: the general-species kernels with the reaction-field terms, whatever their LJ parameters
        if constexpr (MODE == BRICK_FORCE && (BM == 1 || BM == 7 || BM == TENSOR_PASS)) {
            if (has_charges()) {
                if constexpr (charged_variant<V>()) {
                    if (has_ewald()) {
                        // (variant 0 only, see choose_plan: the fp64 erfc does not fit the 128 registers of a 1024-thread workgroup)
                        if constexpr (std::is_same<V, BrickVariant<0>>::value) launch_brick_kernel_impl<V, MODE, BM | EMDEE_CHARGED | EMDEE_EWALD, false>(p);
                        else EMDEE_REQUIRE(false, EMDEE_ERR_STATE, "Ewald engine on brick variant %d", plan.variant);
                    } else launch_brick_kernel_impl<V, MODE, BM | EMDEE_CHARGED, false>(p);
                } else EMDEE_REQUIRE(false, EMDEE_ERR_STATE, "charged engine on brick variant %d", plan.variant);
                return;
            }
        }
        // single-species fast path for the kernels of the MD loop (default variant only)
        if constexpr (std::is_same<V, BrickVariant<0>>::value && (MODE == BRICK_STEP || (MODE == BRICK_FORCE && (BM == 1 || BM == 7 || BM == TENSOR_PASS)))) {
            // (the fp64 variant keeps coordinate planes only in LDS and needs the tile to fit their fixed pitch)
            if (uniform_atoms && plan.tile_cap <= SOA_SLOTS && plan.idx_shift == PLANE_SHIFT && !(MODE == BRICK_FORCE && ref_tiles(p))) {
                launch_brick_kernel_impl<V, MODE, BM, true>(p);
                return;
            }
        }
        launch_brick_kernel_impl<V, MODE, BM, false>(p);
    }

    template <class V, int MODE, int BM, bool UNI>
    void launch_brick_kernel_impl(const Pass<real> &p) {
        launch_bricks<V>(k_brick<real, typename V::Shape, V::THREADS, V::G, MODE, BM, UNI>,
                         (UNI && MODE != BRICK_STATS) ? brick_force_lds_bytes_soa<real, typename V::Shape, V::THREADS>(plan.own_cap) : plan.lds_force, p);
    }

    // the default variant has an instance for every mask; the tuning variants carry only the two masks the MD loop uses, and the
    // tensor pass
    // (a narrower request on those, and on the typed kernels, runs the all-outputs instance: runs_all_outputs)
    bool runs_all_outputs(int mask) const { return plan.active && mask >= 2 && mask <= 6 && (plan.typed || plan.variant != 0); }
    DevBuf<real> spare;                                      // three force planes, energies, virials: what such a pass is not asked for
    template <class V>
    void launch_brick_force(const Pass<real> &p) {
        using List = std::conditional_t<std::is_same<V, BrickVariant<0>>::value, AllMasks, LoopMasks>;
        with_mask(List{}, p.mask, [&](auto m) { launch_brick_kernel<V, BRICK_FORCE, decltype(m)::value>(p); });
    }

    // ---------------------------------------------------------------- the plan (plan.hpp)
    // what choose_plan and plan_kept decide from: the grid, the counts, the flags of the state and the switches of the environment
    PlanFacts plan_facts() const {
        PlanFacts f;
        f.real_bytes = (int)sizeof(real);
        for (int d = 0; d < 3; d++) { f.M[d] = grid.M[d]; f.per[d] = grid.per[d]; f.len[d] = len[d]; }
        f.rlist = rlist;
        f.n = n_total; f.n_plan = edit_n_plan; f.in_edit = in_edit;
        f.nt = nt; f.nsub = nsub;
        f.uniform = uniform_atoms; f.charged = has_charges(); f.ewald = has_ewald(); f.filters_rows = filters_rows() || has_alch();
        f.brick_path = path == PATH_BRICK;
        f.stride = stride; f.typed_stride = typed_stride;
        f.field16_blocked = blocked.field16; f.typed_blocked = blocked.typed;
        f.typed_all = std::getenv("EMDEE_TYPED_ALL") != nullptr;
        const char *tb = std::getenv("EMDEE_TYPED_BRICKS");
        f.typed_bricks7 = tb != nullptr && std::atoi(tb) == 7;
        f.debug = std::getenv("EMDEE_DEBUG_PLAN") != nullptr;
        return f;
    }
    // flags[6] = largest tile, flags[7] = most own atoms of a brick, flags[8] = most atoms in three consecutive cells of a tile row
    // (with_build_words: the build's own words flags[0..5) are cleared by the same launch -- the first attempt of build_list)
    template <class S>
    void launch_tile_max(const BrickGrid &bg, bool with_build_words = false) {
        if (with_build_words) Zeros().add(flags.ptr, 9).run(stream());
        else Zeros().add(flags.ptr + 6, 3).run(stream());
        hipLaunchKernelGGL((k_brick_tile_max<S>), dim3(blocks_for(bg.nbricks, 256)), dim3(256), 0, stream(), bg, grid.M[0], grid.M[1], grid.M[2],
                           grid.per[0], grid.per[1], grid.per[2], start(), flags.ptr + 6);
    }
    // The populations choose_plan asks for: one small kernel and one blocking read-back each (plans are rare).  The maxima of a
    // brick shape are measured once per choose_plan call -- the cell populations cannot change inside it.
    struct DeviceMeasure {
        NbSystem &s;
        bool have[2] = {false, false};
        std::array<int, 3> memo[2];
        template <class S>
        std::array<int, 3> maxima(S) {
            const int k = S::NOC == 8 ? 1 : 0;               // (the two brick shapes of plan.hpp)
            if (!have[k]) {
                s.template launch_tile_max<S>(brick_grid<S>(s.grid.M, s.grid.per));
                read_back_words(s.ctx, s.stream(), s.flags.ptr + 6, 3, s.ctx->host_flags + 6);
                memo[k] = {s.ctx->host_flags[6], s.ctx->host_flags[7], s.ctx->host_flags[8]};
                have[k] = true;
            }
            return memo[k];
        }
        template <class S>
        int typed_span(S) {
            const BrickGrid bg = brick_grid<S>(s.grid.M, s.grid.per);
            EMDEE_HIP_CHECK(hipMemsetAsync(s.flags.ptr + 8, 0, sizeof(int), s.stream()));
            hipLaunchKernelGGL((k_typed_span_max<S>), dim3(blocks_for(bg.nbricks, 256)), dim3(256), 0, s.stream(), bg, s.grid.M[0], s.grid.M[1],
                               s.grid.M[2], s.grid.per[0], s.grid.per[1], s.grid.per[2], s.tstart(), s.flags.ptr + 8, s.tsub);
            EMDEE_HIP_CHECK(hipMemcpyAsync(s.ctx->host_flags + 8, s.flags.ptr + 8, sizeof(int), hipMemcpyDeviceToHost, s.stream()));
            EMDEE_HIP_CHECK(hipStreamSynchronize(s.stream()));
            return s.ctx->host_flags[8];
        }
    };
    // full planning with blocking read-backs: the plan, the row stride it asks for, and its lines under EMDEE_DEBUG_PLAN
    void replan() {
        std::string text;
        plan = choose_plan(plan_facts(), DeviceMeasure{*this}, text);
        if (!text.empty()) std::fputs(text.c_str(), stderr);
        stride = plan.stride;
        typed_stride = plan.typed_stride;
        btab_valid = false;
    }

    // ---------------------------------------------------------------- neighbour list
    void build_list() {
        const int n = n_total;
        if (stride == 0) {
            double vol = len[0] * len[1] * len[2];
            double expect = n > 0 ? (4.0 / 3.0) * M_PI * rlist * rlist * rlist * (double)n / vol : 0.0;
            // first guess: 15 % above the mean row (a jittered lattice at rho* = 0.8, r_list = 2.8 has 73.6 +- 4, longest row 85; the
            // melt 91): rounded up to whole lane-major blocks below, 96 entries there.  A longer row grows the stride and
            // builds again.  (128 instead of 96 costs 2 % of the step: 33 % more bytes flushed per build, rows 256 B apart)
            stride = (int)((expect * 1.15 + 8.0) / 16.0 + 1.0) * 16;
            typed_stride = false;
        }
        btab_valid = false;
        // The plan of the previous build of this state (variant, capacities, build kernel) is kept when the cell grid is the
        // same (plan_kept): the maxima of the new populations come back with the build's overflow words -- ONE blocking
        // read-back per rebuild instead of two.
        // (taking the maxima from k_brick_tables instead, which has every brick's tables in LDS anyway, was measured and
        // lost: one workgroup per brick means one look at -- or atomic on -- three hot words per brick, 2.84 -> 2.95 ms per
        // rebuild even with a device-scope look before the atomic, 4.50 ms without; k_brick_tile_max reduces 64 bricks per
        // wavefront first)
        bool kept = plan_kept(plan, plan_facts());
        if (kept) with_brick_variant(plan.variant, [&](auto v) { launch_tile_max<typename decltype(v)::Shape>(plan.grid, true); });
        else replan();
        // (a state with a capacity hint -- decomposed domains -- sizes the list for it: no reallocation while atoms come and go)
        const size_t rows = std::max<size_t>((size_t)std::max(n, 1), cap_hint ? capacity : 0);
        for (int attempt = 0; attempt < 6; attempt++) {
            EMDEE_REQUIRE((double)n * stride < 1.7e10, EMDEE_ERR_OVERFLOW, "neighbour list would exceed 64 GiB");
            if (in_edit && !plan.active) { edit_abort = true; return; }   // (the direct kernels count atoms on the host: the caller reloads)
            if (!(kept && attempt == 0)) Zeros().add(flags.ptr, 5).run(stream());   // (a kept plan cleared them with the maxima)
            if (plan.active) {
                nbr16.ensure(rows * stride);
                with_brick_variant(plan.variant, [&](auto v) {
                    using V = decltype(v);
                    if constexpr (typed_variant<V>()) {
                        if (plan.typed) {   // two species: species-major tables and the two-segment build (typed.hpp)
                            const BrickArgs<real> ta = launch_tables<V, TNT>(tsub);
                            auto kernel = k_typed_build<real, typename V::Shape, V::THREADS, V::GB, V::G>;
                            allow_big_lds(kernel, plan.lds_build);
                            BrickArgs<real> ba = brick_args();
                            ba.nsub = ta.nsub; ba.bsub = ta.bsub;
                            hipLaunchKernelGGL(kernel, dim3(plan.grid.per_xcd * NXCD), dim3(V::THREADS), plan.lds_build, stream(), ba);
                            return;
                        }
                    }
                    if (!btab_valid) launch_tables<V, 1>(nsub);
                    auto kernel = k_brick_build<real, typename V::Shape, V::THREADS, V::GB, 1, V::G>;
                    if constexpr (V::GB == 8 || V::GB == 16) {
                        if (plan.build_alg == 3) kernel = k_brick_build<real, typename V::Shape, V::THREADS, V::GB, 3, V::G>;
                        if (plan.build_alg == 5) kernel = k_brick_build<real, typename V::Shape, V::THREADS, V::GB, 5, V::G>;
                        // round-robin candidates (brick.hpp): when the force kernels read plane values or 16-byte records with 4 lanes per atom
                        if constexpr (V::G == 4) {
                            const bool strided_ok = sizeof(real) == 4 || plan.idx_shift != 0;
                            if (plan.build_alg == 3 && strided_ok) kernel = k_brick_build<real, typename V::Shape, V::THREADS, V::GB, 13, V::G>;
                            if (plan.build_alg == 5 && strided_ok) kernel = k_brick_build<real, typename V::Shape, V::THREADS, V::GB, 15, V::G>;
                        }
                    }
                    allow_big_lds(kernel, plan.lds_build);
                    hipLaunchKernelGGL(kernel, dim3(plan.grid.per_xcd * NXCD), dim3(V::THREADS), plan.lds_build, stream(),
                                       brick_args());
                });
            } else {
                nbr.ensure(rows * stride);
                if (n > 0)
                    hipLaunchKernelGGL((k_nbr_build<real>), dim3(blocks_for((size_t)n * WAVE, NBR_BLOCK)), dim3(NBR_BLOCK),
                                       0, stream(), n, n_owned, view(), perm.ptr, cell_sorted.ptr, start(), grid,
                                       (real)(rlist * rlist), nbr.ptr, stride, cnt.ptr, flags.ptr);
            }
            // a build is rare (every ~7 steps): one blocking read-back -- the overflow words and, under a kept plan, the
            // population maxima it has to hold for
            if (in_edit && edit_extra.n > 0) {
                read_back_words(ctx, stream(), flags.ptr, 9, ctx->host_flags, edit_extra.dev, edit_extra.n, edit_extra.host);
                edit_extra_read = true;
            } else {
                // (an engine that keeps counts for its caller: the three words of image_fault ride along)
                read_back_words(ctx, stream(), flags.ptr, 9, ctx->host_flags, flags.ptr + W_IMAGE, image_limit ? 3 : 0, image_words);
            }
            if (kept && (!plan_holds(plan, ctx->host_flags + 6) || ctx->host_flags[2] != 0)) {
                // the populations outgrew the kept plan (the kernels skipped the bricks concerned): plan afresh and build again
                kept = false;
                replan();
                continue;
            }
            if (plan.active && ctx->host_flags[4] != 0) {
                // A lane's share of a tile row did not fit its 16-bit hit field.  The builds cannot overflow it (the plan's widest
                // 3-cell run is what picked the field): should they ever, the list is NOT taken -- this state goes on with 32-bit fields.
                EMDEE_REQUIRE(!blocked.field16, EMDEE_ERR_OVERFLOW, "neighbour build: a lane's share of a tile row (%d) overflows its hit field", ctx->host_flags[4]);
                blocked.field16 = true;
                kept = false;
                replan();
                continue;
            }
            EMDEE_REQUIRE(ctx->host_flags[2] == 0, EMDEE_ERR_OVERFLOW, "LDS tile overflow (%d records > %d)",
                          ctx->host_flags[2], plan.tile_cap);
            int needed = ctx->host_flags[0];
            if (needed <= stride) {
                builds++;
                has_list = true;
                apply_exclusions();
                apply_alchemical();
                return;
            }
            // grow and rebuild (after_build): rows longer than the typed build's LDS row buffers can take send this state on
            // with the general-species kernels, rows longer than theirs to the direct kernels
            bool block_typed = false;
            plan = after_build(plan, nsub, needed, block_typed);
            stride = plan.stride;
            if (block_typed) {
                blocked.typed = true;
                kept = false;
                replan();
                continue;
            }
            if (!plan.active) btab_valid = false;
        }
        EMDEE_REQUIRE(false, EMDEE_ERR_OVERFLOW, "neighbour capacity kept overflowing");
    }

    // ---------------------------------------------------------------- exclusions and 1-4 pairs (topology_dev.hpp Topology)
    // Every engine keys the rows of its tables the same way (kernels.hpp PairKeys): by tag when it carries tags (a decomposed
    // engine), else by caller id.  The row filter records where each 1-4 partner sits in the rows (slots14) and k_pairs14 sums
    // those slots after every force pass: no look-up by id during steps, and a pair beyond rc + skin at the build is beyond rc
    // while the list is valid.  Two-species boxes with tables keep the general-species kernels (a typed row is two
    // block-aligned segments: compacting one would move the other).
    Topology own_tables;                                     // an undivided engine's, over caller ids
    Topology *tables = &own_tables;                          // a decomposed engine's point at the decomposition's, over global ids
    DevBuf<int> slots14;                                     // per 1-4 entry of an owned atom's row: the partner's cell-order slot
    DevBuf<int> slotsb;                                      // per bonded partner of an owned atom: its cell-order slot
    bool has_excl() const { return tables->has_excl; }
    bool has_14() const { return tables->has_14; }
    bool has_bonded() const { return tables->has_bonded; }
    // terms added behind a whole force pass (add_post_terms): such a box steps in the split form (force pass, these terms,
    // kick + drift), not the fused one
    bool has_post() const { return has_14() || has_bonded() || has_charges() || has_restraints() || has_pull() || has_alch(); }
    // rows the filter visits right after every build: excluded pairs are struck, 1-4 and bonded partners' slots recorded
    bool filters_rows() const { return has_excl() || has_bonded(); }
    // a bonded term whose partner was missing from the rows (raised by k_bonded): the engine refuses to step until the tables or
    // the state are replaced
    FaultWord bonded_fault{W_BONDED};
    void reset_bonded_error() { bonded_fault.reset(flags.ptr, stream()); }
    // The shape of check_bonded, check_ewald and check(g).  Blocking, one read-back unless the fault is latched already:
    // EMDEE_ERR_STATE with message(entry) if the word has been raised since the last reset, with `reported_before` from then on.
    template <class Message>
    void throw_on_fault(FaultWord &fault, Message &&message, const char *reported_before) {
        if (const int32_t word = fault.poll(ctx, flags.ptr, stream())) {
            set_error("%s", message((int64_t)word - 1).c_str());
            throw Failure{EMDEE_ERR_STATE};
        }
        EMDEE_REQUIRE(!fault.latched, EMDEE_ERR_STATE, "%s", reported_before);
    }
    // The shape of check_state and check_vsites.  The n <= 2 words from flags[first] on are cleared, launch(words) queues the
    // kernel that raises them, one read-back: EMDEE_ERR_STATE with message(w, entry) for the first word w that names an entry.
    template <class Launch, class Message>
    void throw_on_check_words(int first, int n, Launch &&launch, Message &&message) {
        EMDEE_HIP_CHECK(hipMemsetAsync(flags.ptr + first, 0, n * sizeof(int), stream()));
        launch(flags.ptr + first);
        int32_t words[2] = {0, 0};
        read_back_words(ctx, stream(), flags.ptr + first, n, words);
        for (int w = 0; w < n; w++)
            if (words[w] != 0) {
                set_error("%s", message(w, (int64_t)words[w] - 1).c_str());
                throw Failure{EMDEE_ERR_STATE};
            }
    }
    // blocking: EMDEE_ERR_STATE naming the term if k_bonded has met a missing partner since the last reset
    void check_bonded() {
        check_ewald();                                       // (the other term that needs a partner in the rows)
        if (!has_bonded() || !flags.ptr) return;
        throw_on_fault(bonded_fault, [&](int64_t term) { return topo::lost_partner_message(tables->b_atoms, term); },
                       "a bonded term has lost a partner (reported before): replace the tables or the state");
    }
    // emdee_nbr_* / emdee_md_set_exclusions, _set_pairs14: replaces one of the engine's own tables (n = 0 clears it), all or nothing
    void set_pair_tables(int n_atoms, const int32_t *pairs_dev, int n_pairs, bool one_four, double scale) {
        own_tables.set(pairs_dev, n_pairs, one_four, scale, n_atoms, stream());
        has_list = false; plan = {};                         // (the rows in use were filtered with the old tables; typed rows are not filtered)
    }
    PairKeys pair_keys() const {
        return PairKeys{use_tags ? tag.ptr : nullptr, tables->rows, tables->p_start.ptr, tables->p_idx.ptr, has_14() ? slots14.ptr : nullptr,
                        (has_ewald() && has_excl()) ? slotsx.ptr : nullptr};
    }
    BondedKeys bonded_keys() const {
        return BondedKeys{tables->b_rows, tables->b_pstart.ptr, tables->b_pidx.ptr, has_bonded() ? slotsb.ptr : nullptr,
                          tables->b_tstart.ptr, tables->b_terms.ptr, tables->b_tid.ptr};
    }
    void check_tables(const char *what) const {
        if (tables != &own_tables) EMDEE_REQUIRE(use_tags, EMDEE_ERR_STATE, "%s over global ids: the state carries no tags", what);
        else EMDEE_REQUIRE(tables->limit == n_owned && !id_gaps, EMDEE_ERR_STATE, "%s set for %lld atoms, the state holds %d", what,
                           (long long)tables->limit, n_owned);
    }
    // right after a build: the rows without their excluded entries, and the 1-4 partners' slots
    void apply_exclusions() {
        if (!filters_rows() || n_total == 0) return;
        check_tables("exclusion / bonded tables");
        if (has_14()) slots14.ensure(tables->n14 + 1);
        if (has_bonded()) slotsb.ensure(tables->nb + 1);
        if (has_ewald() && has_excl()) slotsx.ensure(tables->nx + 1);
        if (brick_active) {
            EMDEE_REQUIRE(!plan.typed, EMDEE_ERR_STATE, "exclusions: typed rows are not filtered");
            with_brick_variant(plan.variant, [&](auto v) {
                using V = decltype(v);
                auto kernel = k_brick_filter<real, typename V::Shape, V::THREADS, V::G>;
                using BT = BrickTables<typename V::Shape, V::THREADS>;
                hipLaunchKernelGGL(kernel, dim3(plan.grid.per_xcd * NXCD), dim3(V::THREADS), BT::bytes(0), stream(), brick_args(),
                                   tables->x_start.ptr, tables->x_idx.ptr, pair_keys(), bonded_keys());
            });
        } else {
            hipLaunchKernelGGL(k_filter_rows, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, perm.ptr, nbr.ptr, stride,
                               cnt.ptr, tables->x_start.ptr, tables->x_idx.ptr, pair_keys(), bonded_keys());
        }
    }
    // ---------------------------------------------------------------- charges (Topology::set_charges)
    // A charged engine keeps sqrt(K) q of every slot in its own cell order (qp), owned atoms and ghosts, looked up by the key the
    // atom carries: filled before the first force pass after every sort or in-place edit (the messages of a decomposition carry
    // no charges), unchanged in between (ghost identities are fixed between rebuilds).
    DevBuf<real> qp;
    bool q_valid = false;
    FaultWord charge_fault{W_CHARGES};                       // a key without a charge: the engine refuses to step
    bool has_charges() const { return tables->has_charges; }
    // an undivided engine whose state no longer has the atom count the charges were set for
    bool charges_stale() const { return has_charges() && tables == &own_tables && (tables->q_n != n_owned || id_gaps); }
    Charges<real> charge_args() const {
        Charges<real> c{};
        if (!has_charges()) return c;
        const double rc = std::sqrt(model_d.rc2), rc3 = rc * rc * rc, eps = tables->eps_rf;
        const double k = std::isinf(eps) ? 0.5 / rc3 : (eps - 1.0) / ((2.0 * eps + 1.0) * rc3);
        c.q = qp.ptr;
        c.k = (real)k; c.k2 = (real)(2.0 * k); c.c = (real)(1.0 / rc + k * rc * rc);
        c.scale14 = (real)tables->scale14c;
        if (has_ewald()) { c.alpha = (real)ewald.alpha; c.a2spi = (real)(2.0 * ewald.alpha / std::sqrt(M_PI)); }
        return c;
    }
    void ensure_charges() {
        if (!has_charges()) return;
        EMDEE_REQUIRE(!charges_stale(), EMDEE_ERR_STATE, "charges set for %lld atoms, the state holds %d: set them again or clear them "
                      "(emdee_md_set_coulomb)", (long long)tables->q_n, n_owned);
        EMDEE_REQUIRE(!charge_fault.latched, EMDEE_ERR_STATE, "an atom has an id outside the charge table: set the charges again");
        if (q_valid || n_total == 0) return;
        if (tables != &own_tables) EMDEE_REQUIRE(use_tags, EMDEE_ERR_STATE, "charges over global ids: the state carries no tags");
        qp.ensure(std::max<size_t>((size_t)n_total, capacity) + 1);
        hipLaunchKernelGGL((k_fill_charges<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, perm.ptr,
                           use_tags ? tag.ptr : nullptr, tables->q_tab.ptr, (long long)tables->q_n, qp.ptr, flags.ptr + W_CHARGES);
        q_valid = true;
    }
    void reset_charge_error() {
        q_valid = false;
        charge_fault.reset(flags.ptr, stream());
    }
    // blocking: EMDEE_ERR_STATE if a fill has met a key outside the charge table since the last reset
    void check_charges() {
        if (!has_charges() || !flags.ptr) return;
        charge_fault.poll(ctx, flags.ptr, stream());
        EMDEE_REQUIRE(!charge_fault.latched, EMDEE_ERR_STATE, "an atom has an id outside the charge table (emdee_dd_set_coulomb: n_ids too "
                      "small); set the charges again");
    }

    // after a force pass: the scaled 1-4 terms on top (the _q twins of a charged engine take the charges as one more argument)
    void add_pairs14(const Pass<real> &p) {
        if (!has_14() || n_total == 0) return;
        check_tables("1-4 table");
        auto launch = [&](auto kernel, auto... extra) {
            hipLaunchKernelGGL(kernel, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, pitch, view(), perm.ptr,
                               pair_keys(), grid, model, (real)tables->scale14, p.mask, frc.ptr, en.ptr, vir.ptr, p.f, p.e, p.w, vt.ptr, p.vt,
                               extra...);
        };
        const bool tensor = p.mask & EMDEE_TENSOR;
        if (has_charges())
            with_bool(has_ewald(), [&](auto ew) {
                with_bool(tensor, [&](auto t) { launch(k_pairs14_q<real, decltype(t)::value, decltype(ew)::value>, charge_args()); });
            });
        else with_bool(tensor, [&](auto t) { launch(k_pairs14<real, decltype(t)::value>); });
    }

    // after a force pass: the bonded terms on top (k_bonded; not on the operator path, which has no bonded tables)
    void add_bonded(const Pass<real> &p) {
        if (!has_bonded() || n_total == 0) return;
        check_tables("bonded tables");
        with_bool(p.mask & EMDEE_TENSOR, [&](auto tensor) {
            hipLaunchKernelGGL((k_bonded<real, decltype(tensor)::value>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned,
                               pitch, view(), perm.ptr, pair_keys(), bonded_keys(), tables->template bonded_params<real>(), grid, p.mask, frc.ptr,
                               en.ptr, vir.ptr, vt.ptr, flags.ptr + W_BONDED);
        });
    }
    // ---------------------------------------------------------------- Ewald summation (emdee_md_set_ewald)
    // With ewald.alpha > 0 a charged engine's pair loops take the erfc-screened terms (the EMDEE_EWALD instances), the row filter
    // records the slot of every struck entry (slotsx), and behind every force pass k_ewald_struck corrects the struck pairs and
    // ewald.run adds the reciprocal-space terms, the self term and the background.  Undivided engines in a fully periodic box.
    EwaldRecip<real> ewald;
    DevBuf<int> slotsx;                                      // per entry of the struck CSR of an owned atom: the partner's cell-order slot
    bool has_ewald() const { return ewald.on() && has_charges(); }
    // a struck pair whose partner was missing from the rows (raised by k_ewald_struck): as bonded_fault
    FaultWord ewald_fault{W_EWALD};
    void reset_ewald_error() { ewald_fault.reset(flags.ptr, stream()); }
    // blocking: EMDEE_ERR_STATE naming the pair if k_ewald_struck has met a missing partner since the last reset
    void check_ewald() {
        if (!has_ewald() || !has_excl() || !flags.ptr) return;
        throw_on_fault(ewald_fault, [&](int64_t pair) { return topo::lost_pair_message(tables->excl, tables->p14, pair); },
                       "Ewald: an excluded or 1-4 pair spans more than rc + skin (reported before): replace the tables or the state");
    }
    void add_ewald(const Pass<real> &p) {
        if (!has_ewald() || n_total == 0) return;
        EMDEE_REQUIRE(!has_ghosts && n_total == n_owned && tables == &own_tables, EMDEE_ERR_STATE,
                      "Ewald summation on an engine with ghosts or a domain's engine: switch it off (emdee_md_set_ewald) or load a state without ghosts");
        EMDEE_REQUIRE(!p.to_caller(), EMDEE_ERR_STATE, "Ewald summation is not on the operator path");
        if (has_excl()) {
            check_tables("exclusion table");
            with_bool(p.mask & EMDEE_TENSOR, [&](auto tensor) {
                hipLaunchKernelGGL((k_ewald_struck<real, decltype(tensor)::value>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total,
                                   n_owned, pitch, view(), perm.ptr, pair_keys(), tables->x_start.ptr, grid, p.mask, frc.ptr, en.ptr, vir.ptr,
                                   vt.ptr, charge_args(), flags.ptr + W_EWALD);
            });
        }
        Timed t(this, T_EWALD);
        ewald.run(stream(), n_total, pitch, view(), lo, len, qp.ptr, tables->q_sum, tables->q_abs, p.mask, frc.ptr, en.ptr, vir.ptr, vt.ptr);
    }
    // ---------------------------------------------------------------- constraint groups (Topology::set_rigid3, set_hbonds)
    // The three stages MdImpl::closed_step puts around the unchanged kick + drift, force pass and kick, and the check of a table
    // against a loaded state: one thread per group, no atomics on the state, fp64 on unwrapped differences in both precisions.
    // Undivided engines only.  One ConstraintGroup per table says what differs -- the table, the policy's kernels (settle.hpp
    // Triangle: SETTLE / RATTLE on rigid three-site molecules; shake.hpp Star: M-SHAKE / RATTLE on bonds to hydrogen), the timer,
    // the words and the texts -- and the functions below serve both.  The atoms of the two tables are disjoint (topology.hpp), so
    // the order of the two kernels within a stage cannot matter.
    struct ConstraintGroup {
        Topology::GroupTable Topology::*table;
        int sites;                                           // x0 holds 3 * sites doubles per group
        int timer;
        FaultWord fault;                                     // a group that moved too far for a solution (raised by stage (c)): as bonded_fault
        int check_word, check_words;                         // the words of the table check
        std::string (*message)(const std::vector<int32_t> &, int64_t, const char *);
        const char *no_solution, *reported_before, *check_text[2];
        void (*k_gather)(ConstraintArgs<real>, double *);
        void (*k_positions)(ConstraintArgs<real>, const double *, double, const real *, real, int *, int *);
        void (*k_velocities)(ConstraintArgs<real>);
        void (*k_check)(ConstraintArgs<real>, int *);
        DevBuf<double> x0;                                   // stage (a): the sites of every group, table order
    };
    template <class G>
    static ConstraintGroup group_of(Topology::GroupTable Topology::*table, int timer, int fault, int check_word, int check_words,
                                    std::string (*message)(const std::vector<int32_t> &, int64_t, const char *), const char *no_solution,
                                    const char *reported_before, const char *check0, const char *check1) {
        return ConstraintGroup{table, G::SITES, timer, FaultWord{fault}, check_word, check_words, message, no_solution, reported_before,
                               {check0, check1}, k_constraint_gather<real, G>, k_constraint_positions<real, G>,
                               k_constraint_velocities<real, G>, k_constraint_check<real, G>, {}};
    }
    enum { RIGID = 0, HBONDS = 1, GROUPS = 2 };
    ConstraintGroup groups[GROUPS] = {
        group_of<Triangle>(&Topology::rigid, T_SETTLE, W_SETTLE, W_RIGID_MASS, 2, topo::rigid3_message,
                           "the step moved its atoms too far for a rigid solution (a negative radicand in SETTLE); the molecule was left as it "
                           "is: replace the table or the state",
                           "a rigid molecule had no solution (reported before): replace the table or the state",
                           "the two legs have different masses",
                           "the loaded positions miss a distance of the table by more than 1e-3 (relative): a wrong topology, not rounding"),
        group_of<Star>(&Topology::hbonds, T_HBONDS, W_HBONDS, W_HBONDS_DIST, 1, topo::hbonds_message,
                       "the step moved its atoms too far for the bonds to be restored (no solution of the SHAKE equations within the "
                       "iteration cap); the cluster was left as it is: replace the table or the state",
                       "an hbonds cluster had no solution (reported before): replace the table or the state",
                       "the loaded positions miss a distance of the table by more than 1e-3 (relative): a wrong topology, not rounding",
                       nullptr)};
    const Topology::GroupTable &table(const ConstraintGroup &g) const { return tables->*g.table; }
    bool has_rigid() const { return tables->rigid.present; }
    bool has_hbonds() const { return tables->hbonds.present; }
    template <class F>
    void for_each_table(F &&f) { for (auto &g : groups) if (table(g).present) f(g); }   // (every table that exists, in the order of groups[])
    // an engine whose state no longer has the atom count an attached table -- a constraint table or the site table -- was set for:
    // it refuses to step (as with charges)
    bool stale(const Topology::GroupTable &t) const { return t.present && (t.limit != n_owned || id_gaps); }
    void reset_error(ConstraintGroup &g) { g.fault.reset(flags.ptr, stream()); }
    // blocking, one read-back: EMDEE_ERR_STATE naming the group if stage (c) has met one without a solution since the last reset
    void check(ConstraintGroup &g) {
        if (!table(g).present || !flags.ptr) return;
        throw_on_fault(g.fault, [&](int64_t group) { return g.message(table(g).atoms_h, group, g.no_solution); }, g.reported_before);
    }
    ConstraintArgs<real> constraint_args(const int *atoms, const double *geom, int n) const {
        ConstraintArgs<real> a{};
        a.n = n; a.atoms = atoms; a.geom = geom; a.inv_perm = inv_perm.ptr; a.rec = rec.ptr; a.vel = vel.ptr;
        a.inv_mass = with_mass ? im.ptr : nullptr; a.pitch = pitch;
        a.rel = rel_grid(rel_now, cell_sorted.ptr);
        for (int d = 0; d < 3; d++) { a.box.len[d] = len[d]; a.box.per[d] = per[d]; }
        return a;
    }
    ConstraintArgs<real> constraint_args(const ConstraintGroup &g) const { return constraint_args(table(g).atoms.ptr, table(g).geom.ptr, table(g).n); }
    ConstraintArgs<real> settle_args() const { return constraint_args(groups[RIGID]); }   // (the molecular sums and the molecular scale)
    void gather(ConstraintGroup &g) {
        Timed t(this, g.timer);
        g.x0.ensure((size_t)3 * g.sites * table(g).n + 1);
        hipLaunchKernelGGL(g.k_gather, dim3(blocks_for(table(g).n, 256)), dim3(256), 0, stream(), constraint_args(g), g.x0.ptr);
    }
    void positions(ConstraintGroup &g, double dt) {
        Timed t(this, g.timer);
        const real thr = (real)(0.5 * skin);                 // (kick_drift's threshold)
        hipLaunchKernelGGL(g.k_positions, dim3(blocks_for(table(g).n, 256)), dim3(256), 0, stream(), constraint_args(g), (const double *)g.x0.ptr,
                           dt > 0.0 ? 1.0 / dt : 0.0, (const real *)xb.ptr, thr * thr, flags.ptr + 1, flags.ptr + g.fault.index);
    }
    void velocities(ConstraintGroup &g) {
        Timed t(this, g.timer);
        hipLaunchKernelGGL(g.k_velocities, dim3(blocks_for(table(g).n, 256)), dim3(256), 0, stream(), constraint_args(g));
    }
    // a table (in force, or a candidate not yet committed) against the loaded state: EMDEE_ERR_STATE naming the group that fails
    // the policy's test (settle.hpp Triangle::check, shake.hpp Star::check); one launch, one read-back
    void check_state(ConstraintGroup &g, const int *atoms, const double *geom, const std::vector<int32_t> &atoms_h, int n) {
        throw_on_check_words(g.check_word, g.check_words, [&](int *words) {
            hipLaunchKernelGGL(g.k_check, dim3(blocks_for(n, 256)), dim3(256), 0, stream(), constraint_args(atoms, geom, n), words);
        }, [&](int w, int64_t group) { return g.message(atoms_h, group, g.check_text[w]); });
    }
    void check_state(ConstraintGroup &g) { check_state(g, table(g).atoms.ptr, table(g).geom.ptr, table(g).atoms_h, table(g).n); }

    // ---------------------------------------------------------------- whole molecules (Topology::set_molecules; molecule.hpp)
    // The general path of the molecular sums and the molecular scale.  molecules_on: emdee_md_set_molecular_scaling's switch, as
    // MdImpl keeps it.  molecule_table() is the ONE place the molecular entries (scale_box, queue_molecular_tensor_sums,
    // molecular_tensor_sums) choose their path: the molecule table if one is in force, fits the state and the switch is on, else NULL
    // -- the Triangle kernels over the rigid table.  Undivided engines only.
    bool molecules_on = false;
    bool has_molecules() const { return tables->molecules.present; }
    const Topology::MoleculeTable *molecule_table() const {
        const Topology::MoleculeTable &t = tables->molecules;
        return (molecules_on && t.present && !stale(t) && !has_ghosts && tables == &own_tables) ? &t : nullptr;
    }
    // the molecules the path in force sums over and scales by (0: the molecular entries are the atomic ones)
    int molecular_groups() const {
        if (const Topology::MoleculeTable *mt = molecule_table()) return mt->n;
        return has_rigid() ? tables->rigid.n : 0;
    }
    MoleculeArgs<real> molecule_args(const Topology::MoleculeTable &t) const {
        MoleculeArgs<real> a{};
        a.n_mol = t.n; a.n_small = t.n_small; a.start = t.start.ptr; a.entry_mol = t.entry_mol.ptr; a.centres = t.centres.ptr;
        a.r = restraint_args(t.atoms.ptr, t.n_entries);
        a.rec = rec.ptr; a.vel = vel.ptr; a.inv_mass = with_mass ? im.ptr : nullptr;
        return a;
    }
    // kernel (1): the centres of every molecule of t, for the kernel the caller queues behind it
    void queue_molecule_centres(const Topology::MoleculeTable &t, int timer = -1) {
        const int small_blocks = blocks_for(t.n_small, 256), large_blocks = blocks_for(t.n - t.n_small, 256 / WAVE);
        timed_if(timer, [&] {
            hipLaunchKernelGGL((k_molecule_centres<real>), dim3(small_blocks + large_blocks), dim3(256), 0, stream(), molecule_args(t), small_blocks);
        });
    }
    // a molecule table (in force, or a candidate not yet committed) against the loaded state and the constraint tables in force:
    // EMDEE_ERR_STATE naming the molecule whose mass is 0 or that is not loaded whole; one read-back
    void check_molecules(const Topology::MoleculeTable &t) {
        if (t.n == 0) return;
        const char *const text[2] = {"its total mass is 0: the centre of mass of massless atoms is undefined (give every virtual site the id of its parents)",
                                     "it is not loaded whole: the unwrapped distance of two atoms of a constraint group inside it misses the table's "
                                     "distance by more than 1e-3 (relative), as after wrapping a state atom by atom; load every molecule in one piece "
                                     "(the image the caller loads is the one the centre of mass is formed from)"};
        throw_on_check_words(W_MOLECULE_MASS, 2, [&](int *words) {
            queue_molecule_centres(t);
            hipLaunchKernelGGL(k_molecule_check_mass, dim3(blocks_for(t.n, 256)), dim3(256), 0, stream(), t.n, (const double *)t.centres.ptr, words);
            const struct { const Topology::GroupTable &g; int sites; } held[2] = {{tables->rigid, 3}, {tables->hbonds, 4}};
            for (const auto &h : held)
                if (h.g.present && !stale(h.g) && h.g.n > 0)
                    hipLaunchKernelGGL((k_molecule_check_whole<real>), dim3(blocks_for(h.g.n, 256)), dim3(256), 0, stream(),
                                       restraint_args(t.atoms.ptr, t.n_entries), h.g.n, h.sites, (const int *)h.g.atoms.ptr,
                                       (const double *)h.g.geom.ptr, (const int *)t.mol_of.ptr, words);
        }, [&](int w, int64_t mol) { return topo::molecule_message(t.rows, mol, text[w]); });
    }
    // the same test for a candidate constraint table (emdee_md_set_rigid3, emdee_md_set_hbonds) against the molecule table in force
    void check_groups_whole(const int *atoms, const double *geom, int n, int sites) {
        const Topology::MoleculeTable &t = tables->molecules;
        if (!t.present || stale(t) || t.n == 0 || n == 0) return;
        throw_on_check_words(W_MOLECULE_MASS, 2, [&](int *words) {
            hipLaunchKernelGGL((k_molecule_check_whole<real>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), restraint_args(t.atoms.ptr, t.n_entries),
                               n, sites, atoms, geom, (const int *)t.mol_of.ptr, words);
        }, [&](int, int64_t mol) {
            return topo::molecule_message(t.rows, mol, "it is not loaded whole: the unwrapped distance of two atoms of a constraint group of this call "
                                                       "misses the table's distance by more than 1e-3 (relative); load every molecule in one piece");
        });
    }

    // ---------------------------------------------------------------- virtual interaction sites (Topology::set_vsites; vsite.hpp)
    // Placement after whatever moves parents (MdImpl::closed_step stage (c'), scale_box, the set call, a reload) and
    // spreading after every force pass that writes the engine's own force planes (MdImpl::force_pass): one thread per site or per
    // distinct parent, fp64 sums in table order, no atomics.  Undivided engines only.
    bool has_vsites() const { return tables->vsites.present; }
    // the table can be used on this state: it was set for this atom count and the state carries masses (a site's is 0)
    bool vsites_fit() const { return has_vsites() && !stale(tables->vsites) && with_mass && !has_ghosts && tables->vsites.n > 0; }
    VsiteArgs<real> vsite_args(const Topology::VsiteTable &t) const {
        VsiteArgs<real> a{};
        a.n = t.n; a.n_parents = t.n_parents; a.atoms = t.atoms.ptr; a.weights = t.geom.ptr;
        a.parent = t.parent.ptr; a.pstart = t.pstart.ptr; a.esite = t.esite.ptr; a.eweight = t.eweight.ptr;
        a.c = constraint_args(nullptr, nullptr, 0);
        return a;
    }
    // zero_vel: the sites' velocities become 0 as well (the set call, a reload)
    void place_sites(bool zero_vel) {
        const Topology::VsiteTable &t = tables->vsites;
        Timed tm(this, T_VSITE);
        const real thr = (real)(0.5 * skin);                 // (kick_drift's threshold)
        hipLaunchKernelGGL((k_vsite_place<real>), dim3(blocks_for(t.n, 256)), dim3(256), 0, stream(), vsite_args(t), (const real *)xb.ptr, thr * thr,
                           flags.ptr + 1, zero_vel ? 1 : 0);
    }
    // the sites' forces go to their parents and become 0: after a pass that has written the force planes, once
    void spread_sites() {
        const Topology::VsiteTable &t = tables->vsites;
        Timed tm(this, T_VSITE);
        hipLaunchKernelGGL((k_vsite_spread<real>), dim3(blocks_for(t.n_parents, 256)), dim3(256), 0, stream(), vsite_args(t), frc.ptr);
        hipLaunchKernelGGL((k_vsite_clear<real>), dim3(blocks_for(t.n, 256)), dim3(256), 0, stream(), vsite_args(t), frc.ptr);
    }
    // a site table (in force, or a candidate not yet committed) against the loaded state: EMDEE_ERR_STATE naming the site that has
    // a mass or a parent without one, or the first site when the state was loaded without masses; one launch, one read-back
    void check_vsites(const Topology::VsiteTable &t) {
        if (t.n == 0) return;
        if (!with_mass) {
            set_error("%s", topo::vsite_message(t.atoms_h, 0, "the state was loaded without masses (inv_mass NULL: every mass is 1), a site needs "
                                                               "inv_mass = 0: load the state with masses").c_str());
            throw Failure{EMDEE_ERR_STATE};
        }
        const char *const text[2] = {"the site has a mass (inv_mass != 0): a virtual site is loaded with inv_mass = 0",
                                     "a parent is massless (inv_mass == 0): a site is built on atoms with mass"};
        throw_on_check_words(W_VSITE_MASS, 2, [&](int *words) {
            hipLaunchKernelGGL((k_vsite_check<real>), dim3(blocks_for(t.n, 256)), dim3(256), 0, stream(), vsite_args(t), words);
        }, [&](int w, int64_t site) { return topo::vsite_message(t.atoms_h, site, text[w]); });
    }

    // ---------------------------------------------------------------- position restraints (Topology::set_restraints; restraint.hpp)
    // One launch behind a force pass, one thread per table entry; each atom owns its whole term.  Undivided engines only.
    bool has_restraints() const { return tables->restraints.present; }
    RestraintArgs<real> restraint_args(const int *atoms, int n) const {
        const Topology::RestraintTable &t = tables->restraints;
        RestraintArgs<real> a{};
        a.n = n; a.n_owned = n_owned; a.n_total = n_total;
        a.atoms = atoms; a.ref = t.ref.ptr; a.k = t.geom.ptr; a.flat = t.flat.ptr;
        a.inv_perm = inv_perm.ptr; a.img = img.ptr; a.rec = rec.ptr;
        a.rel = rel_grid(rel_now, cell_sorted.ptr);
        for (int d = 0; d < 3; d++) a.len[d] = (double)grid.len[d];
        a.pitch = pitch;
        return a;
    }
    RestraintArgs<real> restraint_args() const { return restraint_args(tables->restraints.atoms.ptr, tables->restraints.n); }
    // a table set for another atom count stays in force, unused, as charges do: whatever would evaluate it refuses
    void require_restraints_fit(const char *what) const {
        const Topology::RestraintTable &t = tables->restraints;
        EMDEE_REQUIRE(!stale(t) && !has_ghosts && tables == &own_tables, EMDEE_ERR_STATE, "%s: position restraints set for %lld atoms, the state "
                      "holds %d (or has ghosts): set them again or clear them (emdee_md_set_restraints)", what, (long long)t.limit, n_owned);
    }
    void add_restraints(const Pass<real> &p) {
        if (!has_restraints() || n_total == 0) return;
        require_restraints_fit("force pass");
        EMDEE_REQUIRE(!p.to_caller(), EMDEE_ERR_STATE, "position restraints are not on the operator path");
        if (tables->restraints.n == 0) return;
        Timed t(this, T_RESTRAINTS);
        with_bool(p.mask & EMDEE_TENSOR, [&](auto tensor) {
            hipLaunchKernelGGL((k_restraints<real, decltype(tensor)::value>), dim3(blocks_for(tables->restraints.n, 256)), dim3(256), 0, stream(),
                               restraint_args(), p.mask, frc.ptr, en.ptr, vir.ptr, vt.ptr);
        });
    }
    // a candidate table's references <- its atoms' current unwrapped coordinates (Topology::set_restraints, ref NULL)
    void capture_restraint_refs(const int *atoms, double *ref, int n) {
        hipLaunchKernelGGL((k_restraint_capture<real>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), restraint_args(atoms, n), ref);
    }
    // emdee_md_restraint_sums, blocking: out[0] = sum U, out[1..6] = the sum of the tensors, out[7] = the largest |d|; fp64 in a fixed
    // order that depends on the number of entries alone
    void restraint_sums(double out[RESTRAINT_WORDS]) {
        for (int q = 0; q < RESTRAINT_WORDS; q++) out[q] = 0.0;
        if (!has_restraints() || tables->restraints.n == 0) return;
        require_restraints_fit("restraint_sums");
        read_back_doubles(out, queue(tables->restraints.n, RestraintSums<real>{restraint_args()}, RED_RESTRAINT), RESTRAINT_WORDS);
    }

    // ---------------------------------------------------------------- the centre-of-mass pull (Topology::set_pull; pull.hpp)
    // Three launches behind a force pass: the chunks' partial sums, the one block that finishes the bookkeeping, one thread per grouped
    // atom.  The pass that follows PullTable::advance closes a step: the work words advance and the log takes its entry.  Undivided
    // engines only.
    bool has_pull() const { return tables->pull.present; }
    void require_pull_fit(const char *what) const {
        const Topology::PullTable &t = tables->pull;
        EMDEE_REQUIRE(!stale(t) && !has_ghosts && tables == &own_tables, EMDEE_ERR_STATE, "%s: the pull table was set for %lld atoms, the state "
                      "holds %d (or has ghosts): set it again or clear it (emdee_md_set_pull)", what, (long long)t.limit, n_owned);
    }
    void add_pull(const Pass<real> &p) {
        if (!has_pull() || n_total == 0) return;
        require_pull_fit("force pass");
        EMDEE_REQUIRE(!p.to_caller(), EMDEE_ERR_STATE, "the centre-of-mass pull (emdee_md_set_pull) is not on the operator path");
        Topology::PullTable &t = own_tables.pull;
        ComPullArgs a{};
        a.n_groups = t.n_groups; a.n_coords = t.n; a.closing = t.closing ? 1 : 0; a.log_slot = t.log_slot; a.dt = t.closing_dt;
        for (int g = 0; g <= PULL_MAX_GROUPS; g++) a.chunk_of_group[g] = t.chunk_of_group[g];
        for (int c = 0; c < PULL_MAX_COORDS; c++) { a.xi0[c] = t.xi0[c]; a.coord[c] = t.coord[c]; }
        t.closing = false; t.log_slot = -1;
        const RestraintArgs<real> ra = restraint_args(t.atoms.ptr, t.n_grouped);
        const real *w = with_mass ? im.ptr : nullptr;
        Timed timed(this, T_PULL);
        hipLaunchKernelGGL((k_pull_partials<real>), dim3(t.n_chunks), dim3(MSD_BLOCK), 0, stream(), ra, w, (const MsdChunk *)t.chunks.ptr, t.partial.ptr);
        hipLaunchKernelGGL(k_pull_finish, dim3(1), dim3(RED_BLOCK), 0, stream(), a, (const double *)t.partial.ptr, t.out.ptr, t.groups_out(),
                           t.group_words.ptr, t.log.ptr);
        with_bool(p.mask & EMDEE_TENSOR, [&](auto tensor) {
            hipLaunchKernelGGL((k_pull_apply<real, decltype(tensor)::value>), dim3(blocks_for(t.n_grouped, 256)), dim3(256), 0, stream(), ra, w,
                               (const int *)t.group_of.ptr, (const double *)t.group_words.ptr, p.mask, frc.ptr, en.ptr, vir.ptr, vt.ptr);
        });
    }

    // ---------------------------------------------------------------- soft-core alchemical decoupling (Topology::set_alchemical; alchemical.hpp)
    // Right after every build (and after the exclusion filter, so that an excluded cross pair stays excluded and is never recorded)
    // the row pass strikes the cross entries of every owned atom's row: count, one exclusive scan (the sort's Scanner), one read-back
    // of the three totals, fill.  Behind every force pass one launch over the owners the pass listed, then the two stages of the sums
    // and the launch that leaves the words of a read on the device.  The foreign energies are queued at log events and by the read
    // only.  Undivided engines only; launched only with a table in force.
    DevBuf<int> alch_scan, alch_xs;                          // the scan array of the row pass; the CSR of struck slots
    DevBuf<AlchOwner> alch_owners;
    DevBuf<double> alch_part, alch_part_f;                   // per owner ALCH_SUMS words; per solute owner ALCH_MAX_FOREIGN energies
    int alch_n_struck = 0, alch_n_sol = 0, alch_n_env = 0;   // of the list in use
    bool has_alch() const { return tables->alch.present; }
    void require_alch_fit(const char *what) const {
        const Topology::AlchTable &t = tables->alch;
        EMDEE_REQUIRE(!stale(t) && !has_ghosts && tables == &own_tables, EMDEE_ERR_STATE, "%s: the alchemical table was set for %lld atoms, the "
                      "state holds %d (or has ghosts): set it again or clear it (emdee_md_set_alchemical)", what, (long long)t.limit, n_owned);
    }
    void apply_alchemical() {
        alch_n_struck = alch_n_sol = alch_n_env = 0;
        if (!has_alch() || n_total == 0) return;
        if (stale(tables->alch) || has_ghosts || tables != &own_tables) return;   // (unfit: the force pass refuses; the rows stay whole)
        const Topology::AlchTable &t = own_tables.alch;
        Timed timed(this, T_ALCHEMICAL);
        const size_t n = (size_t)n_total;
        alch_scan.ensure(3 * n + 4);
        EMDEE_HIP_CHECK(hipMemsetAsync(alch_scan.ptr, 0, (3 * n + 4) * sizeof(int), stream()));
        auto rows = [&](auto fill) {
            constexpr bool FILL = decltype(fill)::value;
            if (brick_active) {
                EMDEE_REQUIRE(!plan.typed, EMDEE_ERR_STATE, "alchemical table: typed rows are not filtered");
                with_brick_variant(plan.variant, [&](auto v) {
                    using V = decltype(v);
                    auto kernel = k_brick_alch<real, typename V::Shape, V::THREADS, V::G, FILL>;
                    using BT = BrickTables<typename V::Shape, V::THREADS>;
                    hipLaunchKernelGGL(kernel, dim3(plan.grid.per_xcd * NXCD), dim3(V::THREADS), BT::bytes(0), stream(), brick_args(),
                                       (const int *)t.flag.ptr, alch_scan.ptr, alch_xs.ptr, alch_owners.ptr);
                });
            } else if constexpr (FILL) {
                hipLaunchKernelGGL(k_alch_strike_rows, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, perm.ptr, nbr.ptr,
                                   stride, cnt.ptr, (const int *)t.flag.ptr, (const int *)alch_scan.ptr, alch_xs.ptr, alch_owners.ptr);
            } else {
                hipLaunchKernelGGL(k_alch_count_rows, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, perm.ptr,
                                   (const int *)nbr.ptr, stride, (const int *)cnt.ptr, (const int *)t.flag.ptr, alch_scan.ptr);
            }
        };
        rows(std::false_type{});
        scanner.run(alch_scan.ptr, 3 * n + 1, stream());
        hipLaunchKernelGGL(k_alch_totals, dim3(1), dim3(64), 0, stream(), alch_scan.ptr, n_total);
        int32_t tot[3] = {0, 0, 0};
        read_back_words(ctx, stream(), alch_scan.ptr + 3 * n + 1, 3, tot);
        alch_n_struck = tot[0]; alch_n_sol = tot[1]; alch_n_env = tot[2];
        if (alch_n_struck == 0) return;
        alch_xs.ensure((size_t)alch_n_struck + 1);
        alch_owners.ensure((size_t)alch_n_sol + alch_n_env + 1);
        alch_part.ensure((size_t)ALCH_SUMS * ((size_t)alch_n_sol + alch_n_env) + 1);
        alch_part_f.ensure((size_t)ALCH_MAX_FOREIGN * alch_n_sol + 1);
        rows(std::true_type{});
    }
    // the two stages of one of the table's sums over n owners into `slot` (stage 1 under the family's own name)
    template <class Term>
    double *queue_alch_sums(int n, const Term &term, int slot) {
        const int nb = red_blocks(n);
        hipLaunchKernelGGL((k_alch_partials<Term>), dim3(nb), dim3(RED_BLOCK), 0, stream(), n, term, red_partials());
        return queue_final<Term>(nb, slot);
    }
    AlchArgs<real> alch_args() const {
        const Topology::AlchTable &t = own_tables.alch;
        AlchArgs<real> a{};
        a.n_sol = alch_n_sol; a.n_env = alch_n_env;
        a.owners = alch_owners.ptr; a.xs = alch_xs.ptr; a.pitch = pitch;
        a.lambda = (real)t.lambda; a.alpha = (real)t.alpha;
        a.sw = AlchModel<real>{model.idl2, model.x0, model.c60};
        a.rc2 = model.rc2;
        return a;
    }
    // The Coulomb stage (emdee_md_set_alchemical_coulomb) takes part in a pass when it is set and the engine has charges on the
    // reaction field; set on an engine whose charges were cleared it is inert (the instances without it run, its words read 0), and
    // under Ewald or PME the solute carries no charge (MdImpl::require_ready), so that every term would be 0.
    DevBuf<double> alch_part_q, alch_part_fq;                // per owner ALCH_COULOMB_SUMS words; per solute owner ALCH_MAX_FOREIGN U_q
    DevBuf<double> alch_part_x;                              // scratch for the Lennard-Jones partials of the words-only launch at lambda_q = 0
    bool has_alch_coulomb() const { return has_alch() && tables->alch.coulomb; }
    bool alch_coulomb_active() const { return has_alch_coulomb() && has_charges() && !has_ewald(); }
    AlchCoulomb<real> alch_coulomb_args() const {
        AlchCoulomb<real> c{};
        if (!alch_coulomb_active()) return c;
        const Topology::AlchTable &t = own_tables.alch;
        const Charges<real> ch = charge_args();
        c.q = ch.q;
        c.lambda_q = (real)t.lambda_q; c.beta = (real)t.beta;
        c.rf = AlchRf<real>{ch.k, ch.c};
        return c;
    }
    // U_alch at the table's foreign lambdas at the current positions, into out[ALCH_WORDS ...): the energies-only instance over the
    // solute owners and the sums, eight words at a time; with the Coulomb stage U_q at the foreign lambda_q into out_q[ALCH_COULOMB_WORDS ...)
    // from the same launch
    void queue_alch_foreign() {
        Topology::AlchTable &t = own_tables.alch;
        if (t.n_foreign == 0) return;
        double *dst = t.out.ptr + ALCH_WORDS;
        double *dst_q = t.coulomb ? t.out_q.ptr + ALCH_COULOMB_WORDS : nullptr;
        const bool coul = alch_coulomb_active();
        if (dst_q && (alch_n_sol == 0 || !coul)) EMDEE_HIP_CHECK(hipMemsetAsync(dst_q, 0, ALCH_MAX_FOREIGN * sizeof(double), stream()));
        if (alch_n_sol == 0) {
            EMDEE_HIP_CHECK(hipMemsetAsync(dst, 0, ALCH_MAX_FOREIGN * sizeof(double), stream()));
            return;
        }
        AlchForeign<real> f{};
        f.K = t.n_foreign;
        for (int k = 0; k < ALCH_MAX_FOREIGN; k++) { f.lambda[k] = (real)t.foreign[k]; f.lambda_q[k] = (real)t.foreign_q[k]; }
        if (coul) alch_part_fq.ensure((size_t)ALCH_MAX_FOREIGN * alch_n_sol + 1);
        with_bool(coul, [&](auto cq) {
            hipLaunchKernelGGL((k_alchemical_foreign<real, decltype(cq)::value>), dim3(alch_sol_blocks(alch_n_sol)), dim3(ALCH_BLOCK), 0, stream(),
                               alch_args(), alch_coulomb_args(), view(), grid, f, alch_part_f.ptr, alch_part_fq.ptr);
        });
        for (int first = 0; first < t.n_foreign; first += 8) {
            const double *tot = queue_alch_sums(alch_n_sol, AlchForeignSums{alch_part_f.ptr, first}, RED_ALCH_FOREIGN + first);
            EMDEE_HIP_CHECK(hipMemcpyAsync(dst + first, tot, 8 * sizeof(double), hipMemcpyDeviceToDevice, stream()));
        }
        if (!coul) return;
        for (int first = 0; first < t.n_foreign; first += 8) {
            const double *tot = queue_alch_sums(alch_n_sol, AlchCoulombForeignSums{alch_part_fq.ptr, first}, RED_ALCH_COULOMB_FOREIGN + first);
            EMDEE_HIP_CHECK(hipMemcpyAsync(dst_q + first, tot, 8 * sizeof(double), hipMemcpyDeviceToDevice, stream()));
        }
    }
    void add_alchemical(const Pass<real> &p) {
        if (!has_alch() || n_total == 0) return;
        require_alch_fit("force pass");
        EMDEE_REQUIRE(!p.to_caller(), EMDEE_ERR_STATE, "the alchemical table (emdee_md_set_alchemical) is not on the operator path");
        Topology::AlchTable &t = own_tables.alch;
        const int slot = t.log_slot;
        t.log_slot = -1;
        Timed timed(this, T_ALCHEMICAL);
        const int owners = alch_n_sol + alch_n_env;
        const bool coul = alch_coulomb_active() && owners > 0;
        if (owners == 0) {
            hipLaunchKernelGGL(k_alch_zero_words, dim3(1), dim3(64), 0, stream(), t.lambda, t.out.ptr, ALCH_WORDS);
        } else {
            const AlchArgs<real> a = alch_args();
            const dim3 blocks(alch_sol_blocks(a.n_sol) + alch_env_blocks(a.n_env));
            if (coul) alch_part_q.ensure((size_t)ALCH_COULOMB_SUMS * (size_t)owners + 1);
            // At lambda_q = 0 U_q, W_q and the force factor are exactly 0, and the planes come from the instance without the stage
            // itself: adding the zeros inside the Coulomb instance is not enough for equal bits, since the compiler contracts the
            // Float32 accumulation differently from instance to instance.  dU/dlambda_q is not 0 there: a second launch of the
            // Coulomb instance under an empty mask writes the stage's partials alone (its Lennard-Jones partials go to scratch).
            const bool split = coul && t.lambda_q == 0.0;
            with_bool(p.mask & EMDEE_TENSOR, [&](auto tensor) {
                with_bool(coul && !split, [&](auto cq) {
                    hipLaunchKernelGGL((k_alchemical<real, decltype(tensor)::value, decltype(cq)::value>), blocks, dim3(ALCH_BLOCK), 0, stream(), a,
                                       alch_coulomb_args(), view(), grid, p.mask, frc.ptr, en.ptr, vir.ptr, vt.ptr, alch_part.ptr, alch_part_q.ptr);
                });
            });
            if (split) {
                alch_part_x.ensure((size_t)ALCH_SUMS * (size_t)owners + 1);
                hipLaunchKernelGGL((k_alchemical<real, false, true>), blocks, dim3(ALCH_BLOCK), 0, stream(), a, alch_coulomb_args(), view(), grid, 0,
                                   frc.ptr, en.ptr, vir.ptr, vt.ptr, alch_part_x.ptr, alch_part_q.ptr);
            }
            const double *tot = queue_alch_sums(owners, AlchSums{alch_part.ptr}, RED_ALCH);
            hipLaunchKernelGGL(k_alch_finish, dim3(1), dim3(64), 0, stream(), t.lambda, tot, t.out.ptr);
        }
        if (t.coulomb) {                                     // the stage's words: the three sums, or 0 where it is inert
            if (coul) {
                const double *tot = queue_alch_sums(owners, AlchCoulombSums{alch_part_q.ptr}, RED_ALCH_COULOMB);
                hipLaunchKernelGGL(k_alch_coulomb_finish, dim3(1), dim3(64), 0, stream(), t.lambda_q, tot, t.out_q.ptr);
            } else {
                hipLaunchKernelGGL(k_alch_zero_words, dim3(1), dim3(64), 0, stream(), t.lambda_q, t.out_q.ptr, ALCH_COULOMB_WORDS);
            }
        }
        if (slot >= 0) {
            queue_alch_foreign();
            hipLaunchKernelGGL(k_alch_log, dim3(1), dim3(64), 0, stream(), (const double *)t.out.ptr, t.n_foreign,
                               t.log.ptr + (size_t)slot * (2 + t.n_foreign));
            if (t.coulomb)
                hipLaunchKernelGGL(k_alch_coulomb_log, dim3(1), dim3(64), 0, stream(), (const double *)t.out_q.ptr, t.n_foreign,
                                   t.log_q.ptr + (size_t)slot * (2 + t.n_foreign));
        }
    }

    void add_post_terms(const Pass<real> &p) {
        add_pairs14(p);
        add_bonded(p);
        add_ewald(p);
        add_restraints(p);
        add_pull(p);
        add_alchemical(p);
    }

    // ---------------------------------------------------------------- forces
    // (p.guard: the direct kernels of a queued step, guarded_split_step, look at this word first; the _q twins of a charged engine
    // take the charges as one more argument)
    template <int BM>
    void launch_direct_force(const Pass<real> &p) {
        const int n = n_total;
        const int nblocks = (n + FORCE_ATOMS - 1) / FORCE_ATOMS, per_xcd = (nblocks + NXCD - 1) / NXCD;
        auto launch = [&](auto kernel, auto... extra) {
            hipLaunchKernelGGL(kernel, dim3(per_xcd * NXCD), dim3(FORCE_BLOCK), 0, stream(), n, n_owned, per_xcd, view(), perm.ptr, nbr.ptr,
                               stride, cnt.ptr, grid, model, pitch, frc.ptr, en.ptr, vir.ptr, p.guard, vt.ptr, extra...);
        };
        if constexpr (BM == 1 || BM == 7 || BM == TENSOR_PASS) {
            if (has_ewald()) return launch(k_lj_force_nbr_q<real, BM | EMDEE_EWALD>, charge_args());
            if (has_charges()) return launch(k_lj_force_nbr_q<real, BM>, charge_args());
        }
        launch(k_lj_force_nbr<real, BM>);
    }

    bool uniform_atoms = false;            // every atom has the same LJAtom (checked when a state is loaded)
    double uni_sigma2 = 0.0, uni_e4 = 0.0, uni_sigma = 1.0;
    // neighbour entries = tile slot << plan.idx_shift; single-species boxes store byte offsets into the coordinate planes
    static constexpr int PLANE_SHIFT = sizeof(real) == 8 ? 3 : 2;

    // Are all LJAtom records identical?  (One small kernel + an 8-byte read-back per load.)
    // uniform_known: -1 = look at the atoms at every load; 0 / 1 = the caller vouches that the species set is mixed /
    // single (emdee_dd_*: agreed once over all domains; atoms only change owner afterwards) and the scan + read-back are skipped
    int uniform_known = -1;
    SpeciesTable species_known{1, {0, 0, 0, 0}};   // with uniform_known == 0: the box's two species, if it has exactly two
    emdee_lj_atom uni_first{0.f, 0.f};
    void detect_uniform_atoms(const emdee_lj_atom *atoms) {
        nt = 1;
        species.n = 1;
        blocked = {};
        if (uniform_known >= 0 && n_total > 0) {
            uniform_atoms = uniform_known == 1;
            // (decomposed runs: the two species every domain agreed on at the first load, emdee_dd_load)
            if (!uniform_atoms && species_known.n == 2 && typed_enabled) { species = species_known; nt = 2; }
            return;
        }
        uniform_atoms = false;
        if (n_total == 0 || std::getenv("EMDEE_NO_UNIFORM")) return;
        EMDEE_HIP_CHECK(hipMemsetAsync(flags.ptr + 5, 0, sizeof(int), stream()));
        hipLaunchKernelGGL(k_atoms_differ, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, atoms, flags.ptr + 5);
        // the distinct LJAtom values, if there are few (two: the box is sorted by species and takes the typed kernels)
        unsigned long long tab[MAX_SPECIES + 1];
        // (Float32 operator calls run the reference's arithmetic on the general-species kernels: those read untyped rows)
        const bool want_species = typed_enabled && !(sizeof(real) == 4 && refmath);
        if (want_species) {
            species_tab.ensure(MAX_SPECIES + 1);
            EMDEE_HIP_CHECK(hipMemsetAsync(species_tab.ptr, 0xff, MAX_SPECIES * sizeof(unsigned long long), stream()));
            EMDEE_HIP_CHECK(hipMemsetAsync(species_tab.ptr + MAX_SPECIES, 0, sizeof(unsigned long long), stream()));
            hipLaunchKernelGGL(k_species_collect, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, atoms, species_tab.ptr);
            EMDEE_HIP_CHECK(hipMemcpyAsync(tab, species_tab.ptr, sizeof(tab), hipMemcpyDeviceToHost, stream()));
        }
        emdee_lj_atom first;
        EMDEE_HIP_CHECK(hipMemcpyAsync(&first, atoms, sizeof(first), hipMemcpyDeviceToHost, stream()));
        EMDEE_HIP_CHECK(hipMemcpyAsync(ctx->host_flags + 5, flags.ptr + 5, sizeof(int), hipMemcpyDeviceToHost, stream()));
        EMDEE_HIP_CHECK(hipStreamSynchronize(stream()));
        if (want_species && tab[MAX_SPECIES] == 0) {
            int found = 0;
            for (int q = 0; q < MAX_SPECIES; q++) found += tab[q] != ~0ull ? 1 : 0;
            if (found == 2) {                                    // (the typed kernels are built for two species)
                std::sort(tab, tab + 2);                         // numbering by value, not by who arrived first
                species.n = 2;
                species.key[0] = tab[0]; species.key[1] = tab[1];
                nt = 2;
            }
        }
        uni_first = first;
        if (ctx->host_flags[5] == 0 && first.half_sigma > 0.f && std::isfinite(first.half_sigma)) {
            uniform_atoms = true;
            set_uniform_constants(first);
        }
    }
    // launch constants of the single-species kernels
    void set_uniform_constants(const emdee_lj_atom &first) {
        uni_first = first;
        // the same fp operations as the per-pair path: (hs + hs)^2 and te * te in the kernel's type
        const real sg = (real)first.half_sigma + (real)first.half_sigma;
        uni_sigma = (double)sg;
        uni_sigma2 = (double)(sg * sg);
        uni_e4 = (double)((real)first.twice_sqrt_eps * (real)first.twice_sqrt_eps);
    }

    // ---------------------------------------------------------------- Langevin thermostat (optional)
    // O step between the kick and the drift of every step: v = c1 v + c2 sqrt(T/m) xi(seed, step, id).
    bool lgv_on = false;
    double lgv_gamma = 0.0, lgv_T = 0.0, lgv_c1 = 1.0;
    unsigned long long lgv_seed = 0, lgv_step = 0;
    const long long *lgv_ids = nullptr;    // caller-order ids for the noise counters (NULL: the caller index)
    bool lgv_by_tag = false;               // ... or the tags that travel with the atoms (decomposed domains)
    void set_langevin(double gamma, double temperature, unsigned long long seed, unsigned long long first_step,
                      const long long *ids) {
        EMDEE_REQUIRE(std::isfinite(gamma) && std::isfinite(temperature) && temperature >= 0.0, EMDEE_ERR_INVALID,
                      "langevin: gamma and temperature must be finite, temperature >= 0");
        lgv_on = gamma > 0.0;
        lgv_gamma = gamma; lgv_T = temperature; lgv_seed = seed; lgv_step = first_step; lgv_ids = ids;
    }
    // noise of the step about to be integrated (cell order); the caller advances lgv_step once per step
    void prepare_noise(double dt) {
        if (!lgv_on || n_total == 0) return;
        noise.ensure(3 * pitch);
        lgv_c1 = std::exp(-lgv_gamma * dt);
        const double c2 = std::sqrt(1.0 - lgv_c1 * lgv_c1);
        hipLaunchKernelGGL((k_langevin_noise<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total,
                           n_owned, pitch, perm.ptr, lgv_ids, with_mass ? im.ptr : nullptr, lgv_seed, lgv_step, c2, lgv_T,
                           noise.ptr, (use_tags && lgv_by_tag) ? tag.ptr : nullptr);
    }

    // One inner velocity-Verlet step as a single kernel: f(x_k), v += c f/m, x_{k+1} = x_k + dt v written to
    // the other position buffer.  False if the brick kernels are not in use (caller runs the split kernels).
    // What the step obeys -- guard and trigger words, the halves of a decomposed step, ghosts, noise -- is in the Pass.
    bool fused_step(const Pass<real> &p) {
        EMDEE_REQUIRE(has_list && sorted && with_vel, EMDEE_ERR_STATE, "no state loaded");
        if (!brick_active || n_total == 0) return false;
        if (has_post()) return false;                          // (the scaled 1-4 and bonded terms are added behind a force pass: the split kernels)
        if (p.phase != 2 && !p.noise_ready) prepare_noise(p.dt);   // phases 1 and 2 are the two halves of one step
        {
            Timed t(this, p.phase == 2 ? T_STEP_BOUNDARY : T_STEP);
            with_brick_variant(plan.variant, [&](auto v) { launch_brick_kernel<decltype(v), BRICK_STEP, 1>(p); });
        }
        if (p.phase != 1 && lgv_on) lgv_step++;
        if (p.phase != 1) {
            if (p.carry_ghosts && has_ghosts)
                hipLaunchKernelGGL((k_copy_ghost_records<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(),
                                   n_total, n_owned, perm.ptr, rec.ptr, rec2.ptr);
            swap_step_buffers();
        }
        return true;
    }
    // positions and velocities ping-pong together
    void swap_step_buffers() { rec.swap(rec2); vel.swap(vel2); }

    // Up to RUN_AHEAD fused steps queued back to back, with ONE read-back for the whole batch instead of a
    // host round trip per step: launch i raises word i when an atom has moved skin/2, launch i + 1 looks at
    // word i first and turns itself into a no-op (passing the word on).  Returns how many steps really ran
    // (>= 1; 0 if the brick kernels are not in use); *stale says whether the last of them asked for a rebuild.
    static constexpr int RUN_AHEAD = 4;
    int run_ahead = RUN_AHEAD;            // EMDEE_RUN_AHEAD=1: one step per round trip (profiling: no no-op launches)
    int fused_steps_run_ahead(Pass<real> p, int want, bool *stale) {
        EMDEE_REQUIRE(has_list && sorted && with_vel, EMDEE_ERR_STATE, "no state loaded");
        *stale = false;
        if (!brick_active || n_total == 0 || has_ghosts || has_post()) return 0;
        const int B = std::max(1, std::min(want, run_ahead));
        int *words = flags.ptr + 9;                          // flags[9 .. 9 + RUN_AHEAD)
        EMDEE_HIP_CHECK(hipMemsetAsync(words, 0, B * sizeof(int), stream()));
        p.phase = 0;
        for (int i = 0; i < B; i++) {
            prepare_noise(p.dt);
            if (lgv_on) lgv_step++;
            Timed t(this, T_STEP);
            p.trigger = words + i;
            p.guard = i ? words + i - 1 : nullptr;
            with_brick_variant(plan.variant, [&](auto v) { launch_brick_kernel<decltype(v), BRICK_STEP, 1>(p); });
            swap_step_buffers();
        }
        read_back_words(ctx, stream(), words, B, ctx->host_flags + 9);
        int ran = B;
        for (int i = 0; i < B; i++)
            if (ctx->host_flags[9 + i]) { ran = i + 1; *stale = true; break; }
        if ((B - ran) & 1) swap_step_buffers();              // the skipped launches did not advance the ping-pong
        if (lgv_on) lgv_step -= (unsigned long long)(B - ran);
        if (profiling) timers[T_STEP].dropped += B - ran;
        return ran;
    }

    // per-atom virial tensors of the last tensor pass (TENSOR_PASS): six planes of pitch slots, allocated on first use
    DevBuf<real> vt;
    // fp32 operator path: pair geometry in the reference's own Float32 arithmetic (scaled positions, minimum image per
    // pair; brick.hpp BrickArgs::refmath) -- what keeps compute_nonbonded! within the reference's 1e-4 of its CPU loop
    bool refmath = false;

    void compute_forces(const Pass<real> &request) {
        Pass<real> p = request;
        EMDEE_REQUIRE(has_list, EMDEE_ERR_STATE, "no neighbour list");
        EMDEE_REQUIRE((p.mask >= 0 && p.mask <= 7) || p.mask == TENSOR_PASS, EMDEE_ERR_INVALID, "bitmask must be a combination of 1|2|4");
        EMDEE_REQUIRE(brick_active || !p.to_caller(), EMDEE_ERR_STATE, "only the tiled kernels write caller-order outputs");
        if (n_total == 0 || p.mask == 0) return;
        ensure_charges();
        // charged engines have instances for forces, all outputs and the tensor pass: a narrower request runs all outputs (and the
        // terms behind the force pass follow the kernel's outputs)
        if (has_charges() && p.mask != EMDEE_FORCES && p.mask != TENSOR_PASS) p.mask = 7;
        if (p.mask & EMDEE_TENSOR) vt.ensure(6 * pitch);
        if (!brick_active && p.phase == 1) return;   // the direct kernels have no brick phases: all work in phase 2
        // an all-outputs instance behind a narrower request into the engine's own arrays: the planes the request leaves out stay as
        // they are (include/emdee_hip.h, emdee_md_forces), and the terms behind the pass switch on the request
        if (runs_all_outputs(p.mask) && !p.to_caller()) {
            spare.ensure(5 * pitch);
            p.spare_unselected = true;
        }
        Timed t(this, T_FORCE);
        if (brick_active) {
            with_brick_variant(plan.variant, [&](auto v) { launch_brick_force<decltype(v)>(p); });
            if (p.phase != 1) add_post_terms(p);             // (once per force pass: behind its last half)
            return;
        }
        with_mask(AllMasks{}, p.mask, [&](auto m) { launch_direct_force<decltype(m)::value>(p); });
        add_post_terms(p);
    }
    void compute_forces(int bitmask) { compute_forces(Pass<real>::force(bitmask)); }

    // ---------------------------------------------------------------- integrator
    void kick_drift(double c, double dt, int *trigger = nullptr, const int *guard = nullptr) {
        EMDEE_REQUIRE(sorted && with_vel, EMDEE_ERR_STATE, "no velocities loaded");
        if (n_total == 0) return;
        prepare_noise(dt);
        Timed t(this, T_KICK_DRIFT);
        real thr = (real)(0.5 * skin);
        hipLaunchKernelGGL((k_kick_drift<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned,
                           pitch, perm.ptr, rec.ptr, vel.ptr, frc.ptr, with_mass ? im.ptr : nullptr, (real)c, (real)dt,
                           xb.ptr, thr * thr, trigger ? trigger : flags.ptr + 1, lgv_on ? noise.ptr : nullptr, (real)lgv_c1, guard);
        if (lgv_on) lgv_step++;
    }

    // One inner step of a domain whose tiles do not fit LDS (the direct kernels), obeying the same device words as
    // fused_step: nothing happens if *guard is set (and *trigger is raised, passing the request on), otherwise force pass,
    // full kick and drift in place, *trigger raised if an atom is now skin/2 away from its position at the last build.
    // Keeps a decomposed run's message sequence independent of which kernels a domain uses (emdee_dd_step).  Also the form of a
    // tiled domain with a 1-4 table (force pass, 1-4 terms, kick + drift): its force pass ignores the guard and leaves forces
    // at unmoved positions -- the rebuild the raised word brings evaluates them afresh.
    void guarded_split_step(const Pass<real> &p) {
        EMDEE_REQUIRE(has_list && sorted && with_vel, EMDEE_ERR_STATE, "no state loaded");
        EMDEE_REQUIRE(!brick_active || has_post(), EMDEE_ERR_STATE, "guarded_split_step is the direct kernels' form of fused_step");
        if (n_total == 0) return;
        Pass<real> f = Pass<real>::force(EMDEE_FORCES);
        f.guard = p.guard;
        compute_forces(f);
        kick_drift(p.c, p.dt, p.trigger, p.guard);
    }

    void kick(double c) {
        EMDEE_REQUIRE(sorted && with_vel, EMDEE_ERR_STATE, "no velocities loaded");
        if (n_total == 0) return;
        Timed t(this, T_KICK);
        hipLaunchKernelGGL((k_kick<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, pitch,
                           perm.ptr, vel.ptr, frc.ptr, with_mass ? im.ptr : nullptr, (real)c);
    }

    // blocking read of the rebuild trigger raised by kick_drift and the step kernels
    bool read_rebuild_flag() {
        read_back_words(ctx, stream(), flags.ptr + 1, 1, ctx->host_flags + 1);
        return ctx->host_flags[1] != 0;
    }

    // ---------------------------------------------------------------- energy minimisation (minimize.hpp; MdImpl::minimize drives these)
    DevBuf<real> gplane;                                     // a = w F, then the constrained force G (three planes, cell order)
    void zero_velocities() {
        if (n_total == 0) return;
        Timed t(this, T_MINIMIZE);
        EMDEE_HIP_CHECK(hipMemsetAsync(vel.ptr, 0, 3 * pitch * sizeof(real), stream()));
    }
    // G: the force-field forces of the last pass with the constraint components removed.  Without a table the force planes
    // themselves.  With tables a = w F goes through the velocity stage of every table that exists (ConstraintArgs::vel, the current
    // positions): what that stage does to a velocity is what a constraint force does to an acceleration.
    const real *constrained_force() {
        if (n_total == 0 || !(has_rigid() || has_hbonds())) return frc.ptr;
        Timed t(this, T_MINIMIZE);
        gplane.ensure(3 * pitch);
        const real *w = with_mass ? im.ptr : nullptr;
        hipLaunchKernelGGL((k_fire_weight<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, pitch, perm.ptr,
                           (const real *)frc.ptr, w, gplane.ptr, 0);
        for_each_table([&](ConstraintGroup &g) {
            ConstraintArgs<real> a = constraint_args(g);
            a.vel = gplane.ptr;
            hipLaunchKernelGGL(g.k_velocities, dim3(blocks_for(table(g).n, 256)), dim3(256), 0, stream(), a);
        });
        hipLaunchKernelGGL((k_fire_weight<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, pitch, perm.ptr,
                           (const real *)frc.ptr, w, gplane.ptr, 1);
        return gplane.ptr;
    }
    // out[0..5] = sum G . v, sum v . v, sum G . G, max |G_i|^2, max |v_i|^2, max |w_i F_i|^2, out[6] = the potential energy of the
    // last pass (energy_sums' term, so that it is the number emdee_md_energies gives), which RED_ENERGY keeps right behind
    // RED_FIRE's six words; one copy, blocking
    void fire_sums(const real *g, double out[FIRE_WORDS + 1]) {
        for (int q = 0; q <= FIRE_WORDS; q++) out[q] = 0.0;
        if (n_total == 0) return;
        static_assert(RED_ENERGY == RED_FIRE + FIRE_WORDS, "fire_sums copies the energy sums' first word with FIRE's six");
        const real *w = with_mass ? im.ptr : nullptr;
        double *tot;
        {
            Timed t(this, T_MINIMIZE);
            queue(n_total, EnergySums<real>{n_owned, pitch, perm.ptr, en.ptr, nullptr, nullptr, frc.ptr, w, (real)0}, RED_ENERGY);
            tot = queue(n_total, FireSums<real>{n_owned, pitch, perm.ptr, g, frc.ptr, vel.ptr, w}, RED_FIRE);
        }
        read_back_doubles(out, tot, FIRE_WORDS + 1);
    }
    void fire_mix(const real *g, double c_v, double c_g) {
        if (n_total == 0) return;
        Timed t(this, T_MINIMIZE);
        hipLaunchKernelGGL((k_fire_mix<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, pitch, perm.ptr,
                           vel.ptr, g, (real)c_v, (real)c_g);
    }

    // ---------------------------------------------------------------- global thermostats (thermostat.hpp; MdImpl::step_closed drives these)
    // th_words[0..19]: the state words of emdee_md_thermostat_state, on the device
    DevBuf<double> th_words;
    double *thermostat_words() {
        if (th_words.ensure(TH_WORDS)) EMDEE_HIP_CHECK(hipMemsetAsync(th_words.ptr, 0, TH_WORDS * sizeof(double), stream()));
        return th_words.ptr;
    }
    // stage (e') of an event: K, the scalar update, v <- alpha v; three launches on the stream, nothing read back
    void thermostat_event(const ThermostatParams &p) {
        if (n_total == 0) return;
        double *w = thermostat_words();
        const int nb = queue_partials(n_total, KineticSums<real>{n_owned, pitch, perm.ptr, vel.ptr, with_mass ? im.ptr : nullptr}, T_THERMOSTAT);
        {
            Timed t(this, T_THERMOSTAT);
            hipLaunchKernelGGL(k_thermostat_update, dim3(1), dim3(RED_BLOCK), 0, stream(), nb, (const double *)red_partials(), p, w);
        }
        {
            Timed t(this, T_THERMOSTAT);
            hipLaunchKernelGGL((k_scale_velocities<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, pitch,
                               perm.ptr, vel.ptr, (const double *)w);
        }
    }

    // ---------------------------------------------------------------- radial distribution functions (rdf.hpp; the table is MdImpl's RdfRecord, observables.hpp)
    // A sample reads the records, perm and the cells the Float32 records are relative to; it writes nothing of the engine's.
    // One frame into t.counts[0 .. n_counters): four timed stages on the stream, nothing read back.
    void rdf_sample(const RdfPlan &plan, RdfRecord &t) {
        if (n_total == 0) return;
        const int n = n_total, ncell = (int)rdf_plan_cells(plan), n_counters = t.n_counters();
        RdfGrid g{};
        for (int d = 0; d < 3; d++) {
            g.lo[d] = lo[d]; g.len[d] = len[d]; g.inv_len[d] = 1.0 / len[d];
            g.M[d] = plan.M[d]; g.wrap[d] = plan.wrap[d];
        }
        g.nd = plan.nd;
        t.cell_of.ensure((size_t)n + 1); t.atoms.ensure((size_t)n + 1);
        t.count.ensure((size_t)ncell + 2); t.fill.ensure((size_t)ncell + 2);
        const RelGrid rel = rel_grid(rel_now, cell_sorted.ptr);
        const int *grp = t.grouped ? t.group.ptr : nullptr, *mol = t.with_mol ? t.mol.ptr : nullptr;
        {
            Timed timed(this, T_RDF);
            EMDEE_HIP_CHECK(hipMemsetAsync(t.count.ptr, 0, ((size_t)ncell + 1) * sizeof(int), stream()));
            EMDEE_HIP_CHECK(hipMemsetAsync(t.fill.ptr, 0, (size_t)ncell * sizeof(int), stream()));
            hipLaunchKernelGGL((k_rdf_count<real>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, n_owned, (const Rec<real> *)rec.ptr, rel,
                               (const int *)perm.ptr, grp, g, t.cell_of.ptr, t.count.ptr);
        }
        {
            Timed timed(this, T_RDF);
            t.scanner.run(t.count.ptr, (size_t)ncell + 1, stream());   // count[] becomes the first slot of every cell
        }
        {
            Timed timed(this, T_RDF);
            hipLaunchKernelGGL((k_rdf_fill<real>), dim3(blocks_for(n, 256)), dim3(256), 0, stream(), n, (const Rec<real> *)rec.ptr, rel,
                               (const int *)perm.ptr, grp, mol, (const int *)t.cell_of.ptr, (const int *)t.count.ptr, t.fill.ptr,
                               t.atoms.ptr);
        }
        {
            Timed timed(this, T_RDF);
            const int blocks = std::max(1, std::min(ncell, 8 * std::max(ctx->cu_count, 32)));
            hipLaunchKernelGGL(k_rdf_pairs, dim3(blocks), dim3(RDF_BLOCK), (size_t)n_counters * sizeof(unsigned int), stream(), g, ncell,
                               (const int *)t.count.ptr, (const RdfAtom *)t.atoms.ptr, t.r_max * t.r_max * RDF_R2_MARGIN, t.inv_dr, t.n_bins,
                               t.n_groups, n_counters, t.counts.ptr);
        }
    }

    // ---------------------------------------------------------------- mean-squared displacement and velocity autocorrelation (msd.hpp; the table is MdImpl's MsdRecord, observables.hpp)
    // A sample reads the records, the image counts, perm, the velocities and the cells the Float32 records are relative to; it
    // writes nothing of the engine's.
    // sample a.s: the snapshot into ring slot `slot` (an origin) or into the scratch snapshot (slot < 0), then every live origin
    // against it; three timed launches on the stream, nothing read back
    void msd_sample(const MsdArgs &a, int slot, MsdRecord &t) {
        if (n_total == 0 || a.n_grouped == 0) return;
        double *cur = t.ring.ptr + (size_t)(slot >= 0 ? slot : t.n_origins) * a.snapshot;
        const int n_live = msd_live_count(a.s, a.n_lags, a.origin_every);
        {
            Timed timed(this, T_MSD);
            hipLaunchKernelGGL((k_msd_gather<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, grid,
                               (const int *)img.ptr, (const int *)perm.ptr, (const Rec<real> *)rec.ptr, rel_grid(rel_now, cell_sorted.ptr),
                               (const real *)vel.ptr, pitch, (const int *)t.pos_of.ptr, a.what, a.n_grouped, cur);
        }
        if (n_live == 0) return;
        {
            Timed timed(this, T_MSD);
            const bool pos = a.what & MSD_POSITIONS, vel_too = a.what & MSD_VELOCITIES;
            auto kernel = pos ? (vel_too ? k_msd_accumulate<true, true> : k_msd_accumulate<true, false>) : k_msd_accumulate<false, true>;
            hipLaunchKernelGGL(kernel, dim3(a.n_chunks), dim3(MSD_BLOCK), 0, stream(), a, (const MsdChunk *)t.chunks.ptr, (const double *)cur,
                               (const double *)t.ring.ptr, t.partial.ptr);
        }
        {
            Timed timed(this, T_MSD);
            hipLaunchKernelGGL(k_msd_finish, dim3(n_live, a.n_groups), dim3(RED_BLOCK), 0, stream(), a, (const int *)t.chunk_of_group.ptr,
                               (const double *)t.partial.ptr, t.sums.ptr);
        }
    }

    // ---------------------------------------------------------------- observables
    // blocking: n doubles of the device on the host, behind everything queued on the stream so far
    void read_back_doubles(double *dst, const double *src, int n) {
        EMDEE_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, stream()));
        EMDEE_HIP_CHECK(hipStreamSynchronize(stream()));
    }
    // out[0] = sum e, out[1] = kinetic energy (velocities advanced by a pending c f/m), out[2] = sum w
    void energy_sums(double pending_c, double out[3]) {
        out[0] = out[1] = out[2] = 0.0;
        if (n_total == 0) return;
        const EnergySums<real> term{n_owned, pitch, perm.ptr, en.ptr, vir.ptr, with_vel ? vel.ptr : nullptr, frc.ptr,
                                    with_mass ? im.ptr : nullptr, (real)pending_c};
        read_back_doubles(out, queue(n_total, term, RED_ENERGY), 3);
    }

    // out[0..5] = sum of the owned atoms' virial tensors (the last tensor pass), out[6..11] = kinetic tensor sum m v^a v^b;
    // (xx, yy, zz, xy, xz, yz), fp64, blocking
    // queues the atomic sums (RED_TENSOR, where the molecules' total has its slot next to them).  timer >= 0: each of the two
    // launches is timed under it (a sample of the Green-Kubo observables counts them as its own)
    double *queue_tensor_sums(int timer = -1) {
        const TensorSums<real> term{n_owned, pitch, perm.ptr, vt.ptr, with_vel ? vel.ptr : nullptr, with_mass ? im.ptr : nullptr};
        return queue(n_total, term, RED_TENSOR, timer);
    }
    void tensor_sums(double out[TENSOR_SUMS]) {
        for (int q = 0; q < TENSOR_SUMS; q++) out[q] = 0.0;
        if (n_total == 0) return;
        read_back_doubles(out, queue_tensor_sums(), TENSOR_SUMS);
    }
    // out[0..5] = W_mol, out[6..11] = K_mol (include/emdee_hip.h: emdee_md_molecular_pressure_tensor): the atomic sums above minus
    // what the atoms of the molecules carry about their centres of mass, with the current force planes -- MoleculeAtomSums over the
    // entries of the molecule table behind k_molecule_centres if one is in force (molecule_table()), else MoleculeSums over the rigid
    // table -- the molecule pass under T_MOLECULAR, its final under the caller's timer.  The two totals lie side by side.
    // The queueing half: both[0..11] the atomic sums, both[12..23] the molecules'; the difference both[q] - both[12 + q] is the
    // reader's (n_total > 0 and molecular_groups() > 0 are the caller's to check).
    double *queue_molecular_tensor_sums(int timer = -1) {
        static_assert(RED_MOLECULE == RED_TENSOR + TENSOR_SUMS, "the readers take both totals as one array of twenty-four");
        double *tot = queue_tensor_sums(timer);
        if (const Topology::MoleculeTable *mt = molecule_table()) {
            queue_molecule_centres(*mt, T_MOLECULAR);
            const int nb = red_blocks(mt->n_entries);
            double *partial = red_partials();
            timed_if(T_MOLECULAR, [&] {
                hipLaunchKernelGGL((k_molecule_partials<real>), dim3(nb), dim3(RED_BLOCK), 0, stream(), mt->n_entries,
                                   MoleculeAtomSums<real>{molecule_args(*mt), frc.ptr}, partial);
            });
            queue_final<MoleculeAtomSums<real>>(nb, RED_MOLECULE, timer);
        } else {
            const int nb = queue_partials(tables->rigid.n, MoleculeSums<real>{settle_args(), frc.ptr}, T_MOLECULAR);
            queue_final<MoleculeSums<real>>(nb, RED_MOLECULE, timer);
        }
        return tot;
    }
    // the read-back half: one copy of both totals, the subtraction on the host.  Blocking.
    void molecular_tensor_sums(double out[TENSOR_SUMS]) {
        for (int q = 0; q < TENSOR_SUMS; q++) out[q] = 0.0;
        if (n_total == 0) return;
        if (molecular_groups() == 0) { tensor_sums(out); return; }
        double both[2 * TENSOR_SUMS];
        read_back_doubles(both, queue_molecular_tensor_sums(), 2 * TENSOR_SUMS);
        for (int q = 0; q < TENSOR_SUMS; q++) out[q] = both[q] - both[TENSOR_SUMS + q];
    }

    // ---------------------------------------------------------------- Green-Kubo observables (gk.hpp; the table is MdImpl's GkRecord, observables.hpp)
    // A sample reads the outputs of the tensor pass, perm, the velocities and the masses; it writes the record's buffers and the
    // scratch of the box sums (red), nothing else of the engine's.
    // sample t.samples of the table: queued on the stream, nothing read back.  Behind a current tensor pass (and, with
    // `molecular`, current forces).  GK_STRESS: the box sums of the pressure entry (two launches, a third with `molecular`, whose
    // molecule pass is T_MOLECULAR's); GK_HEAT: the heat partials and their finish (two); then the push and the correlator (two).
    void gk_sample(GkRecord &t, bool molecular) {
        const double *box = nullptr, *heat = nullptr;
        if ((t.what & GK_STRESS) && n_total > 0) box = molecular ? queue_molecular_tensor_sums(T_GK) : queue_tensor_sums(T_GK);
        if ((t.what & GK_HEAT) && n_total > 0) {
            const HeatSums<real> term{n_owned, pitch, perm.ptr, en.ptr, vt.ptr, vel.ptr, with_mass ? im.ptr : nullptr};
            heat = queue(n_total, term, RED_HEAT, T_GK);
        }
        GkArgs a{};
        a.what = t.what; a.n_lags = t.n_lags; a.molecular = molecular ? 1 : 0; a.s = t.samples; a.ring = t.ring.ptr; a.acc = t.acc.ptr;
        {
            Timed timed(this, T_GK);
            hipLaunchKernelGGL(k_gk_push, dim3(1), dim3(WAVE), 0, stream(), a, box, heat);
        }
        {
            Timed timed(this, T_GK);
            hipLaunchKernelGGL(k_gk_correlate, dim3(blocks_for(gk_live_lags(t.samples, t.n_lags), GK_BLOCK)), dim3(GK_BLOCK), 0, stream(), a);
        }
    }

    // ---------------------------------------------------------------- spatial profiles (spatial.hpp; the table is MdImpl's SpatialRecord, observables.hpp)
    // A sample reads the records, the image counts, perm, the velocities, the masses, the charge table and (SPATIAL_STRESS) the outputs
    // of a current tensor pass; it writes the record's buffers, nothing of the engine's.
    // the centre of mass of the table's centre group into t.centre_dev (R, then M): two launches, timed under `timer` when >= 0
    void spatial_centre(SpatialRecord &t, int timer = -1) {
        const int c0 = t.chunk_of_group[t.centre_group], nc = t.chunk_of_group[t.centre_group + 1] - c0;
        const RestraintArgs<real> ra = restraint_args(t.atoms.ptr, t.n_grouped);
        if (nc > 0)
            timed_if(timer, [&] {
                hipLaunchKernelGGL((k_spatial_centre_partials<real>), dim3(nc), dim3(SPATIAL_BLOCK), 0, stream(), ra, with_mass ? (const real *)im.ptr : nullptr,
                                   (const MsdChunk *)t.chunks.ptr + c0, t.partial.ptr);
            });
        timed_if(timer, [&] {
            hipLaunchKernelGGL(k_spatial_centre, dim3(1), dim3(WAVE), 0, stream(), nc, (const double *)t.partial.ptr, t.centre_dev.ptr);
        });
    }
    // one sample with the geometry of the current box: queued on the stream, nothing read back
    void spatial_sample(SpatialRecord &t, const SpatialGeom &geom) {
        if (n_total == 0 || t.n_grouped == 0) return;
        const bool by_group = geom.geometry == SPATIAL_RADIAL && t.centre_group >= 0;
        if (by_group) spatial_centre(t, T_SPATIAL);
        SpatialSrc<real> a{};
        a.n = n_total; a.n_owned = n_owned; a.g = grid; a.img = img.ptr; a.perm = perm.ptr; a.rec = rec.ptr;
        a.rel = rel_grid(rel_now, cell_sorted.ptr);
        a.vel = with_vel ? vel.ptr : nullptr; a.inv_mass = with_mass ? im.ptr : nullptr; a.en = en.ptr; a.vt = vt.ptr; a.pitch = pitch;
        a.q_raw = has_charges() ? tables->q_raw.ptr : nullptr;
        a.q_n = tables->q_n;
        auto launch = [&](auto mask) {
            constexpr int MASK = decltype(mask)::value;
            {
                Timed timed(this, T_SPATIAL);
                hipLaunchKernelGGL((k_spatial_gather<real, MASK>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), a, geom,
                                   by_group ? (const double *)t.centre_dev.ptr : nullptr, (const int *)t.pos_of.ptr, t.n_grouped, t.key.ptr,
                                   t.planes.ptr);
            }
            {
                Timed timed(this, T_SPATIAL);
                hipLaunchKernelGGL((k_spatial_accumulate<MASK>), dim3(t.n_chunks), dim3(SPATIAL_BLOCK), 0, stream(), (const MsdChunk *)t.chunks.ptr,
                                   (const int *)t.key.ptr, (const double *)t.planes.ptr, (size_t)t.n_grouped, t.sbin.ptr, t.runn.ptr, t.runw.ptr);
            }
            {
                Timed timed(this, T_SPATIAL);
                hipLaunchKernelGGL((k_spatial_finish<MASK>), dim3(blocks_for((size_t)t.n_bins + 1, SPATIAL_BLOCK), t.n_groups), dim3(SPATIAL_BLOCK),
                                   0, stream(), t.n_bins, (const int *)t.chunk_of_group_dev.ptr, (const int *)t.sbin.ptr, (const int *)t.runn.ptr,
                                   (const double *)t.runw.ptr, t.sums.ptr, t.counts.ptr, t.counts.ptr + t.n_cells());
            }
        };
        switch (t.what) {
            case 1: launch(std::integral_constant<int, 1>{}); break;
            case 2: launch(std::integral_constant<int, 2>{}); break;
            case 3: launch(std::integral_constant<int, 3>{}); break;
            case 4: launch(std::integral_constant<int, 4>{}); break;
            case 5: launch(std::integral_constant<int, 5>{}); break;
            case 6: launch(std::integral_constant<int, 6>{}); break;
            default: launch(std::integral_constant<int, 7>{}); break;
        }
    }

    // caller-order copy of the last tensor pass's per-atom tensors (owned atoms, 6 x n_owned)
    void unsort_tensor(real *out) {
        if (n_total == 0) return;
        hipLaunchKernelGGL((k_unsort_tensor<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_owned, n_total, pitch,
                           perm.ptr, ids_map(), vt.ptr, out);
    }

    void list_stats(bool count_pairs, int64_t *listed, int32_t *max_count, int64_t *inside) {
        unsigned long long h[3] = {0, 0, 0};
        if (has_list && n_total > 0) {
            EMDEE_HIP_CHECK(hipMemsetAsync(stats.ptr, 0, 3 * sizeof(unsigned long long), stream()));
            if (brick_active) {
                with_brick_variant(plan.variant, [&](auto v) { launch_brick_kernel<decltype(v), BRICK_STATS, 0>(Pass<real>{}); });
            } else {
                hipLaunchKernelGGL((k_list_stats<real>), dim3(red_blocks(n_total)), dim3(RED_BLOCK), 0, stream(), n_total, view(), nbr.ptr,
                                   stride, cnt.ptr, grid, model.rc2, count_pairs ? 1 : 0, stats.ptr);
            }
            EMDEE_HIP_CHECK(hipMemcpyAsync(h, stats.ptr, sizeof(h), hipMemcpyDeviceToHost, stream()));
            EMDEE_HIP_CHECK(hipStreamSynchronize(stream()));
        }
        if (listed) *listed = (int64_t)h[0];
        if (max_count) *max_count = (int32_t)h[1];
        if (inside) *inside = (int64_t)(h[2] / 2);   // full list: every pair appears twice
    }

    // neighbour rows as caller ids (verification accessor): counts[n_owned], out[n_owned x capacity]
    void export_list(int *counts, int *out, int capacity) {
        EMDEE_REQUIRE(has_list, EMDEE_ERR_STATE, "no neighbour list");
        EMDEE_REQUIRE(counts && out && capacity > 0, EMDEE_ERR_INVALID, "export_list: bad arguments");
        if (n_total == 0) return;
        const int *map = ids_map();
        if (brick_active) {
            with_brick_variant(plan.variant, [&](auto v) {
                using V = decltype(v);
                if constexpr (typed_variant<V>()) {
                    if (plan.typed) return launch_export<V, TNT>(counts, out, capacity, map);
                }
                launch_export<V, 1>(counts, out, capacity, map);
            });
        } else {
            hipLaunchKernelGGL(k_export_rows, dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, n_owned, perm.ptr, nbr.ptr,
                               stride, cnt.ptr, counts, out, capacity, map);
        }
        EMDEE_HIP_CHECK(hipGetLastError());
    }

    // ---------------------------------------------------------------- caller-order copies
    // (dense caller order: owned atoms first, then the ghosts -- through ids_map() when the ids have gaps; atoms_out / tags_out
    // / raw: what a decomposition needs to go back to caller-order arrays, dd.hpp)
    void unsort(real *pos, real *velocities, real *forces, real *energies, real *virials, emdee_lj_atom *atoms_out = nullptr,
                long long *tags_out = nullptr, bool raw = false) {
        if (n_total == 0) return;
        EMDEE_REQUIRE(!velocities || with_vel, EMDEE_ERR_STATE, "no velocities loaded");
        EMDEE_REQUIRE(!tags_out || use_tags, EMDEE_ERR_STATE, "no tags loaded");
        const int *map = ids_map();
        hipLaunchKernelGGL((k_unsort<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_owned, n_total, pitch,
                           grid, img.ptr, perm.ptr, map, rec.ptr, te.ptr, with_vel ? vel.ptr : nullptr, frc.ptr, en.ptr, vir.ptr,
                           use_tags ? tag.ptr : nullptr, pos, velocities, forces, energies, virials, atoms_out, tags_out, raw ? 1 : 0,
                           rel_grid(rel_now, cell_sorted.ptr));
    }

    // operator path, list kept: refresh + displacement test + species test in one pass and one read-back.
    // Returns true if the list no longer covers the positions (the caller reloads).
    bool refresh_and_check(const real *pos, const emdee_lj_atom *atoms) {
        if (n_total == 0) return false;
        const real thr = (real)(0.5 * skin);
        EMDEE_HIP_CHECK(hipMemsetAsync(flags.ptr + 1, 0, sizeof(int), stream()));
        EMDEE_HIP_CHECK(hipMemsetAsync(flags.ptr + 5, 0, sizeof(int), stream()));
        hipLaunchKernelGGL((k_refresh_check<real>), dim3(blocks_for(n_total, 256)), dim3(256), 0, stream(), n_total, pitch,
                           grid, perm.ptr, pos, atoms, xb.ptr, rec.ptr, te.ptr, thr * thr, flags.ptr, nt > 1 ? 1 : 0);
        emdee_lj_atom first;
        read_back_words(ctx, stream(), flags.ptr, 16, ctx->host_flags);        // posted: 6 us of empty queue instead of two copies + a sync
        memcpy(&first.half_sigma, &ctx->host_flags[14], 4);
        memcpy(&first.twice_sqrt_eps, &ctx->host_flags[15], 4);
        uniform_atoms = false;
        uni_first = first;                                   // (what a decomposition votes on, and what the next load starts from)
        if (ctx->host_flags[5] == 0 && !std::getenv("EMDEE_NO_UNIFORM") && first.half_sigma > 0.f && std::isfinite(first.half_sigma)) {
            uniform_atoms = true;
            set_uniform_constants(first);
        }
        return ctx->host_flags[1] != 0;
    }
};

}  // namespace emdee
