// topology_dev.hpp -- the device side of the topology tables: what topology.hpp builds on the host, uploaded.
#pragma once

#include <cstddef>

#include "alchemical.hpp"
#include "common.hpp"
#include "topology.hpp"

namespace emdee {

static_assert(sizeof(topo::TermEntry) == sizeof(int4) && offsetof(topo::TermEntry, code) == offsetof(int4, x) &&
              offsetof(topo::TermEntry, loc) == offsetof(int4, y), "kernels.hpp BondedKeys reads the term entries as int4");

// Exclusions and scaled 1-4 pairs (kernels.hpp, "exclusions and 1-4 pairs"; the hooks of src/modelling.jl:197-200): pairs the
// caller names are struck from the rows right after every build, and the 1-4 pairs among them come back scaled by lj14scale
// after every force pass.  With them the bonded terms and the charges.  The topology does not change during a run: every table
// is built on the host once per call.  An undivided engine owns one over caller ids (NbSystem::own_tables); a decomposition owns
// one over global ids that all its engines point at (dd.hpp), which is simpler than carrying each atom's partners through
// migration: 4 (max id + 2) + 4 (directed pairs) bytes per pair table.
// Every setter is all or nothing: fetch the caller's arrays, validate and build on the host (topology.hpp), put the result
// into buffers of their own, synchronise, and only then swap and commit -- an invalid call throws and leaves the tables in
// force.  The caller makes sure nothing in flight reads the old tables.
struct Topology {
    // n elements at dev (device) -> host; blocking
    template <typename T>
    static std::vector<T> fetch(const T *dev, size_t n, hipStream_t s) {
        std::vector<T> h(n);
        if (n > 0) {
            EMDEE_HIP_CHECK(hipMemcpyAsync(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
            EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        }
        return h;
    }
    // h -> a buffer that holds it (D: the device's type for H, of the same size)
    template <typename D, typename H>
    static void put(DevBuf<D> &b, const std::vector<H> &h, hipStream_t s) {
        static_assert(sizeof(D) == sizeof(H), "put: element sizes differ");
        b.ensure(h.size() + 1);
        if (!h.empty()) EMDEE_HIP_CHECK(hipMemcpyAsync(b.ptr, h.data(), h.size() * sizeof(H), hipMemcpyHostToDevice, s));
    }

    // ---- exclusions and 1-4 pairs: two symmetric, sorted, duplicate-free CSRs (topo::PairCsrs)
    DevBuf<int> x_start, x_idx;                              // struck from the rows: the exclusions and the 1-4 pairs together
    DevBuf<int> p_start, p_idx;                              // the 1-4 pairs
    std::vector<int32_t> excl, p14;                          // the pairs as given: {i, j, i, j, ...}
    double scale14 = 1.0;
    int rows = 0;                                            // ids 0 .. rows - 1 have rows (max id + 1)
    int64_t limit = 0;                                       // ids of the last call lay in [0, limit): the atom count, or 2^31 (global ids)
    size_t n14 = 0;                                          // entries of the 1-4 CSR
    size_t nx = 0;                                           // entries of the struck CSR (slots of an Ewald engine's row filter)
    bool has_excl = false, has_14 = false;
    // Replaces one table by the n pairs at pairs_dev (device, {i, j, ...}): one_four, the 1-4 pairs scaled by `scale`, else the
    // exclusions; n = 0 clears it.
    template <typename T>
    void set(const T *pairs_dev, int64_t n, bool one_four, double scale, int64_t lim, hipStream_t s) {
        const char *what = one_four ? "set_pairs14" : "set_exclusions";
        EMDEE_REQUIRE(n >= 0 && (n == 0 || pairs_dev), EMDEE_ERR_INVALID, "%s: negative count or NULL array", what);
        EMDEE_REQUIRE(!one_four || std::isfinite(scale), EMDEE_ERR_INVALID, "%s: lj14scale must be finite", what);
        const std::vector<int32_t> h = topo::checked_pairs(what, fetch(pairs_dev, (size_t)2 * n, s), lim);
        const topo::PairCsrs t = topo::build_pairs(one_four ? excl : h, one_four ? h : p14);
        DevBuf<int> nxs, nxi, nps, npi;
        put(nxs, t.xs, s); put(nxi, t.xi, s); put(nps, t.ps, s); put(npi, t.pi, s);
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        // ---- commit
        x_start.swap(nxs); x_idx.swap(nxi); p_start.swap(nps); p_idx.swap(npi);
        if (one_four) { p14 = h; scale14 = scale; } else { excl = h; }
        rows = t.rows; limit = lim; n14 = t.n14; nx = t.xi.size();
        has_excl = t.has_excl; has_14 = t.has_14;
    }

    // ---- bonded terms (emdee_*_set_bonded): kernels.hpp BondedKeys, topo::BondedRows.  The terms as given are kept per kind
    // (b_atoms, b_prm) so that one kind can be replaced without the others.
    std::vector<int32_t> b_atoms[topo::KINDS];
    std::vector<double> b_prm[topo::KINDS];
    DevBuf<int> b_pstart, b_pidx, b_tstart, b_tid;
    DevBuf<int4> b_terms;
    DevBuf<double> b_prm_d;
    DevBuf<float> b_prm_f;
    int b_rows = 0;
    size_t nb = 0;                                           // entries of the partner CSR (slots of the row filter)
    bool has_bonded = false;
    template <typename real>
    const real *bonded_params() const {
        if constexpr (sizeof(real) == 8) return b_prm_d.ptr; else return b_prm_f.ptr;
    }
    // Replaces the table of one kind by the n terms at atoms_dev / params_dev (device; kind_atoms(kind) ids and
    // kind_params(kind) doubles per term); n = 0 clears it.
    template <typename T>
    void set_bonded(int kind, const T *atoms_dev, const double *params_dev, int64_t n, int64_t lim, hipStream_t s) {
        EMDEE_REQUIRE(kind >= 1 && kind <= 3, EMDEE_ERR_INVALID, "set_bonded: unknown kind %d (EMDEE_HARMONIC_BOND, "
                      "EMDEE_HARMONIC_ANGLE or EMDEE_PERIODIC_TORSION)", kind);
        EMDEE_REQUIRE(n >= 0 && (n == 0 || (atoms_dev && params_dev)), EMDEE_ERR_INVALID, "set_bonded: negative count or NULL array");
        const std::vector<T> raw = fetch(atoms_dev, (size_t)topo::kind_atoms(kind) * n, s);
        const std::vector<double> prm = fetch(params_dev, (size_t)topo::kind_params(kind) * n, s);
        const std::vector<int32_t> h = topo::checked_terms(kind, raw, prm, lim, b_atoms);
        const std::vector<int32_t> *at[topo::KINDS] = {};
        const std::vector<double> *pr[topo::KINDS] = {};
        for (int kd = 1; kd < topo::KINDS; kd++) { at[kd] = kd == kind ? &h : &b_atoms[kd]; pr[kd] = kd == kind ? &prm : &b_prm[kd]; }
        const topo::BondedRows t = topo::build_bonded(at, pr);
        DevBuf<int> nps, npi, nts, ntid;
        DevBuf<int4> nterms;
        DevBuf<double> npd;
        DevBuf<float> npf;
        put(nps, t.ps, s); put(npi, t.pi, s); put(nts, t.ts, s); put(ntid, t.tid, s);
        put(nterms, t.terms, s); put(npd, t.pd, s); put(npf, t.pf, s);
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        // ---- commit
        b_pstart.swap(nps); b_pidx.swap(npi); b_tstart.swap(nts); b_tid.swap(ntid); b_terms.swap(nterms);
        b_prm_d.swap(npd); b_prm_f.swap(npf);
        b_atoms[kind] = h; b_prm[kind] = prm;
        b_rows = t.rows; limit = lim; nb = t.nb;
        has_bonded = !t.terms.empty();
    }

    // ---- the constraint tables, undivided engines only: rigid three-site molecules (emdee_md_set_rigid3; settle.hpp), {apex, a, b}
    // caller ids and {d_leg, d_base} per molecule, and bonds to hydrogen (emdee_md_set_hbonds; shake.hpp), {centre, s1, s2, s3}
    // caller ids (-1: an unused trailing slot) and the three distances per cluster.  An atom is held by one table.
    struct GroupTable {
        DevBuf<int> atoms;
        DevBuf<double> geom;
        std::vector<int32_t> atoms_h;                        // the ids as given (the error texts name them; the other table's setter checks against them)
        int n = 0;                                           // groups
        int64_t limit = 0;                                   // the atom count the ids were checked against
        bool present = false;
    };
    GroupTable rigid, hbonds;
    DevBuf<unsigned char> r_member;                          // one byte per id below rigid.limit: named by the table (topo::rigid3_members)
    // Replaces table t by the n groups at atoms_dev / geom_dev (device; `sites` ids and `ngeom` doubles per group); n = 0 clears
    // it.  host(ids, geom): the host check of the fetched arrays, which it leaves as the kernels read them and may follow with
    // uploads of its own; it throws to refuse.  check(atoms, geom, ids, n): the engine's test of the uploaded candidate against
    // its state; it throws to refuse as well, and the table in force stays.  Returns whether a table was committed.
    template <class Host, class Check>
    bool set_groups(GroupTable &t, const char *name, const char *noun, int sites, int ngeom, const int32_t *atoms_dev, const double *geom_dev,
                    int64_t n, int64_t lim, hipStream_t s, Host &&host, Check &&check) {
        EMDEE_REQUIRE(n >= 0 && (n == 0 || (atoms_dev && geom_dev)), EMDEE_ERR_INVALID, "%s: negative count or NULL array", name);
        if (n == 0) {
            t.present = false; t.n = 0; t.atoms_h.clear();
            return false;
        }
        EMDEE_REQUIRE(n <= INT32_MAX / sites, EMDEE_ERR_INVALID, "%s: %lld %s (at most (2^31 - 1) / %d)", name, (long long)n, noun, sites);
        std::vector<int32_t> ids = fetch(atoms_dev, (size_t)sites * n, s);
        std::vector<double> geom = fetch(geom_dev, (size_t)ngeom * n, s);
        host(ids, geom);
        DevBuf<int> na;
        DevBuf<double> ng;
        put(na, ids, s); put(ng, geom, s);
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        check(na.ptr, ng.ptr, ids, (int)n);
        // ---- commit
        t.atoms.swap(na); t.geom.swap(ng);
        t.atoms_h = ids;
        t.n = (int)n; t.limit = lim;
        t.present = true;
        return true;
    }
    template <class Check>
    void set_rigid3(const int32_t *atoms_dev, const double *geom_dev, int64_t n, int64_t lim, hipStream_t s, Check &&check) {
        DevBuf<unsigned char> nm;
        std::vector<uint8_t> member;                         // (outlives the upload)
        const bool set = set_groups(rigid, "set_rigid3", "molecules", 3, 2, atoms_dev, geom_dev, n, lim, s, [&](std::vector<int32_t> &ids, std::vector<double> &geom) {
            ids = topo::checked_rigid3(ids, geom, lim, hbonds.present ? &hbonds.atoms_h : nullptr, vsites.present ? &vsites.atoms_h : nullptr);
            if (molecules.present && molecules.limit == lim)
                topo::refuse_split_groups("set_rigid3", "rigid molecule", "this call", 3, ids, molecules.ids_h);
            member = topo::rigid3_members(ids, lim);
            put(nm, member, s);
        }, check);
        if (set) r_member.swap(nm);
    }
    template <class Check>
    void set_hbonds(const int32_t *atoms_dev, const double *dist_dev, int64_t n, int64_t lim, hipStream_t s, Check &&check) {
        set_groups(hbonds, "set_hbonds", "clusters", 4, 3, atoms_dev, dist_dev, n, lim, s, [&](std::vector<int32_t> &ids, std::vector<double> &dist) {
            ids = topo::checked_hbonds(ids, dist, lim, rigid.present ? &rigid.atoms_h : nullptr, vsites.present ? &vsites.atoms_h : nullptr);
            if (molecules.present && molecules.limit == lim)
                topo::refuse_split_groups("set_hbonds", "hbonds cluster", "this call", 4, ids, molecules.ids_h);
            dist = topo::hbonds_distances(ids, dist);
        }, check);
    }

    // ---- whole molecules (emdee_md_set_molecules; molecule.hpp), undivided engines only: the CSR of topo::MoleculeRows (GroupTable:
    // atoms = the entries' caller ids, n = the molecules of two atoms and more), the molecule of every entry and of every caller id, the
    // membership bytes, and the centres the first kernel writes for the second.
    struct MoleculeTable : GroupTable {
        DevBuf<int> start, entry_mol, mol_of;
        DevBuf<unsigned char> member;
        DevBuf<double> centres;
        std::vector<int32_t> ids_h;                          // the ids as given, one per atom (the constraint setters check against them)
        topo::MoleculeRows rows;                             // the host copy (the error texts name molecules and atoms from it)
        int n_small = 0, n_entries = 0;
    };
    MoleculeTable molecules;
    // Replaces the table by the one the n ids at molecule_dev (device) describe; n = 0 with NULL clears it.  check(table): the
    // engine's test of the uploaded candidate against its state; it throws to refuse, and the table in force stays.
    template <class Check>
    void set_molecules(const int32_t *molecule_dev, int64_t n, int64_t lim, hipStream_t s, Check &&check) {
        EMDEE_REQUIRE(n >= 0 && (n == 0 || molecule_dev), EMDEE_ERR_INVALID, "set_molecules: negative count or NULL array with n > 0");
        if (n == 0) {
            molecules.present = false; molecules.n = 0; molecules.n_small = 0; molecules.n_entries = 0;
            molecules.atoms_h.clear(); molecules.ids_h.clear(); molecules.rows = topo::MoleculeRows{};
            return;
        }
        EMDEE_REQUIRE(n == lim, EMDEE_ERR_INVALID, "set_molecules: n = %lld is neither 0 nor the atom count %lld (one id per atom)", (long long)n,
                      (long long)lim);
        MoleculeTable t;
        t.ids_h = fetch(molecule_dev, (size_t)n, s);
        t.rows = topo::molecule_table(t.ids_h, lim, rigid.present && rigid.limit == lim ? &rigid.atoms_h : nullptr,
                                      hbonds.present && hbonds.limit == lim ? &hbonds.atoms_h : nullptr);
        put(t.start, t.rows.start, s); put(t.atoms, t.rows.atoms, s); put(t.entry_mol, t.rows.entry_mol, s);
        put(t.mol_of, t.rows.mol_of, s); put(t.member, t.rows.member, s);
        t.centres.ensure((size_t)MOL_CENTRE * t.rows.n_mol + 1);
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        t.atoms_h = t.rows.atoms;
        t.n = t.rows.n_mol; t.n_small = t.rows.n_small; t.n_entries = (int)t.rows.atoms.size(); t.limit = lim; t.present = true;
        check(t);
        // ---- commit
        molecules.start.swap(t.start); molecules.atoms.swap(t.atoms); molecules.entry_mol.swap(t.entry_mol); molecules.mol_of.swap(t.mol_of);
        molecules.member.swap(t.member); molecules.centres.swap(t.centres);
        molecules.atoms_h = t.atoms_h; molecules.ids_h = t.ids_h; molecules.rows = t.rows;
        molecules.n = t.n; molecules.n_small = t.n_small; molecules.n_entries = t.n_entries; molecules.limit = lim; molecules.present = true;
    }

    // ---- virtual interaction sites (emdee_md_set_vsites; vsite.hpp), undivided engines only: {site, a, b, c} caller ids (c = -1: a
    // two-parent site) and {w_b, w_c} per entry as `sites` (GroupTable: atoms, geom), and the parent list of topo::VsiteParents
    struct VsiteTable : GroupTable {
        DevBuf<int> parent, pstart, esite;
        DevBuf<double> eweight;
        int n_parents = 0;
    };
    VsiteTable vsites;
    // Replaces the table by the n entries at atoms_dev / weights_dev (device); n = 0 clears it.  check(table): the engine's test
    // of the uploaded candidate against its state; it throws to refuse, and the table in force stays.
    template <class Check>
    void set_vsites(const int32_t *atoms_dev, const double *weights_dev, int64_t n, int64_t lim, hipStream_t s, Check &&check) {
        EMDEE_REQUIRE(n >= 0 && (n == 0 || (atoms_dev && weights_dev)), EMDEE_ERR_INVALID, "set_vsites: negative count or NULL array");
        if (n == 0) {
            vsites.present = false; vsites.n = 0; vsites.n_parents = 0; vsites.atoms_h.clear();
            return;
        }
        EMDEE_REQUIRE(n <= INT32_MAX / 4, EMDEE_ERR_INVALID, "set_vsites: %lld sites (at most (2^31 - 1) / 4)", (long long)n);
        VsiteTable t;
        t.atoms_h = topo::checked_vsites(fetch(atoms_dev, (size_t)4 * n, s), fetch(weights_dev, (size_t)2 * n, s), lim,
                                         rigid.present ? &rigid.atoms_h : nullptr, hbonds.present ? &hbonds.atoms_h : nullptr,
                                         restraints.present ? &restraints.atoms_h : nullptr, pull.present ? &pull.atoms_h : nullptr);
        const std::vector<double> w = topo::vsite_weights(t.atoms_h, fetch(weights_dev, (size_t)2 * n, s));
        const topo::VsiteParents par = topo::build_vsite_parents(t.atoms_h, w);
        put(t.atoms, t.atoms_h, s); put(t.geom, w, s);
        put(t.parent, par.parent, s); put(t.pstart, par.start, s); put(t.esite, par.site, s); put(t.eweight, par.weight, s);
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        t.n = (int)n; t.n_parents = (int)par.parent.size(); t.limit = lim; t.present = true;
        check(t);
        // ---- commit
        vsites.atoms.swap(t.atoms); vsites.geom.swap(t.geom); vsites.parent.swap(t.parent); vsites.pstart.swap(t.pstart);
        vsites.esite.swap(t.esite); vsites.eweight.swap(t.eweight);
        vsites.atoms_h = t.atoms_h;
        vsites.n = t.n; vsites.n_parents = t.n_parents; vsites.limit = lim; vsites.present = true;
    }

    // ---- position restraints (emdee_md_set_restraints; restraint.hpp), undivided engines only: one caller id (GroupTable: atoms), three
    // spring constants (geom), three references and one flat-bottom radius per entry, in the caller's order.  The references follow the
    // box (NbSystem::scale_box), so they live on the device alone.
    struct RestraintTable : GroupTable {
        DevBuf<double> ref, flat;
    };
    RestraintTable restraints;
    // Replaces the table by the n entries at the device arrays (ref_dev NULL: capture(atoms, ref) fills the uploaded candidate's
    // references from the state, queued on s; flat_dev NULL: every radius 0); n = 0 clears it.  Every refusal comes before the table
    // in force changes.
    template <class Capture>
    void set_restraints(const int32_t *atoms_dev, const double *ref_dev, const double *k_dev, const double *flat_dev, int64_t n, int64_t lim,
                        hipStream_t s, Capture &&capture) {
        EMDEE_REQUIRE(n >= 0 && (n == 0 || (atoms_dev && k_dev)), EMDEE_ERR_INVALID, "set_restraints: negative count or NULL array (atoms and "
                      "spring constants are needed with n > 0)");
        if (n == 0) {
            restraints.present = false; restraints.n = 0; restraints.atoms_h.clear();
            return;
        }
        EMDEE_REQUIRE(n <= INT32_MAX / 3, EMDEE_ERR_INVALID, "set_restraints: %lld entries (at most (2^31 - 1) / 3)", (long long)n);
        const topo::RestraintRows rows = topo::restraint_table(fetch(atoms_dev, (size_t)n, s), ref_dev ? fetch(ref_dev, (size_t)3 * n, s) : std::vector<double>(),
                                                               fetch(k_dev, (size_t)3 * n, s), flat_dev ? fetch(flat_dev, (size_t)n, s) : std::vector<double>(),
                                                               lim, vsites.present ? &vsites.atoms_h : nullptr);
        RestraintTable t;
        put(t.atoms, rows.atoms, s); put(t.geom, rows.k, s); put(t.flat, rows.flat, s);
        t.ref.ensure((size_t)3 * n + 1);
        if (ref_dev) put(t.ref, rows.ref, s); else capture((const int *)t.atoms.ptr, t.ref.ptr, (int)n);
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        // ---- commit
        restraints.atoms.swap(t.atoms); restraints.geom.swap(t.geom); restraints.flat.swap(t.flat); restraints.ref.swap(t.ref);
        restraints.atoms_h = rows.atoms;
        restraints.n = (int)n; restraints.limit = lim; restraints.present = true;
    }

    // ---- the centre-of-mass pull (emdee_md_set_pull; pull.hpp), undivided engines only: the grouped caller ids in table order
    // (GroupTable: atoms; n: the coordinates), the group of every entry, the chunks, and the scratch and outputs of the three launches.
    // The host owns the coordinates, the moving references xi0, the count of completed steps and the log's bookkeeping.
    struct PullTable : GroupTable {
        DevBuf<int> group_of;
        DevBuf<MsdChunk> chunks;
        DevBuf<double> partial, out, group_words, log;       // out: n_coords x PULL_WORDS, then n_groups x 4 (one copy reads both)
        PullCoord coord[PULL_MAX_COORDS] = {};
        double xi0[PULL_MAX_COORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
        int chunk_of_group[PULL_MAX_GROUPS + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int n_groups = 0, n_grouped = 0, n_chunks = 0;
        int log_every = 0, log_capacity = 0;
        long long steps = 0, log_count = 0, log_dropped = 0; // completed steps since the set; entries written; samples dropped
        // what the next force pass closes (set by advance(), taken by NbSystem::add_pull)
        bool closing = false;
        double closing_dt = 0.0;
        int log_slot = -1;
        double *groups_out() { return out.ptr + (size_t)PULL_MAX_COORDS * PULL_WORDS; }
        // one more completed step of length dt: xi0 advances on the host, the next force pass closes the step
        void advance(double dt) {
            for (int c = 0; c < n; c++) xi0[c] = pull_advance(xi0[c], coord[c].rate, dt);
            steps++;
            closing = true; closing_dt = dt; log_slot = -1;
            if (log_capacity > 0 && log_every > 0 && steps % log_every == 0) {
                if (log_count < log_capacity) log_slot = (int)log_count++; else log_dropped++;
            }
        }
    };
    PullTable pull;
    // Replaces the table by the one the host arrays describe (group_dev: device, `lim` ids); n_coords = 0 clears it.  Every refusal
    // comes before the table in force changes.
    void set_pull(const int32_t *group_dev, int32_t n_groups, const int32_t *coords, const double *params, int32_t n_coords, int32_t log_every,
                  int32_t log_capacity, int64_t lim, hipStream_t s) {
        EMDEE_REQUIRE(n_coords >= 0, EMDEE_ERR_INVALID, "set_pull: n_coords = %d is outside 1...%d (0 clears the table)", n_coords, PULL_MAX_COORDS);
        if (n_coords == 0) {
            pull.present = false; pull.n = 0; pull.atoms_h.clear();
            return;
        }
        EMDEE_REQUIRE(n_coords <= PULL_MAX_COORDS, EMDEE_ERR_INVALID, "set_pull: n_coords = %d is outside 1...%d (0 clears the table)", n_coords, PULL_MAX_COORDS);
        EMDEE_REQUIRE(group_dev && coords && params, EMDEE_ERR_INVALID, "set_pull: NULL array (group, coords and params are needed with n_coords > 0)");
        EMDEE_REQUIRE(log_capacity >= 0 && log_every >= 0 && (log_capacity == 0 || log_every >= 1), EMDEE_ERR_INVALID, "set_pull: log_every = %d and "
                      "log_capacity = %d: a log (capacity > 0) needs log_every >= 1, and neither is negative", log_every, log_capacity);
        EMDEE_REQUIRE((int64_t)log_capacity * n_coords <= INT32_MAX / 2, EMDEE_ERR_INVALID, "set_pull: log_capacity = %d with %d coordinates is more "
                      "than 2^30 words", log_capacity, n_coords);
        const topo::PullRows rows = topo::pull_table(fetch(group_dev, (size_t)lim, s), n_groups,
                                                     std::vector<int32_t>(coords, coords + 5 * (size_t)n_coords),
                                                     std::vector<double>(params, params + 6 * (size_t)n_coords), n_coords,
                                                     vsites.present ? &vsites.atoms_h : nullptr);
        PullTable t;
        put(t.atoms, rows.ids, s); put(t.group_of, rows.group_of, s);
        t.chunks.ensure(rows.lay.chunks.size() + 1);
        EMDEE_HIP_CHECK(hipMemcpyAsync(t.chunks.ptr, rows.lay.chunks.data(), rows.lay.chunks.size() * sizeof(MsdChunk), hipMemcpyHostToDevice, s));
        t.partial.ensure(4 * rows.lay.chunks.size() + 1);
        t.out.ensure((size_t)PULL_MAX_COORDS * PULL_WORDS + (size_t)PULL_MAX_GROUPS * 4);
        t.group_words.ensure((size_t)PULL_MAX_GROUPS * PULL_GROUP_WORDS);
        t.log.ensure((size_t)2 * log_capacity * n_coords + 1);
        EMDEE_HIP_CHECK(hipMemsetAsync(t.out.ptr, 0, ((size_t)PULL_MAX_COORDS * PULL_WORDS + (size_t)PULL_MAX_GROUPS * 4) * sizeof(double), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(t.group_words.ptr, 0, (size_t)PULL_MAX_GROUPS * PULL_GROUP_WORDS * sizeof(double), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(t.log.ptr, 0, ((size_t)2 * log_capacity * n_coords + 1) * sizeof(double), s));
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        // ---- commit
        pull.atoms.swap(t.atoms); pull.group_of.swap(t.group_of); pull.chunks.swap(t.chunks); pull.partial.swap(t.partial);
        pull.out.swap(t.out); pull.group_words.swap(t.group_words); pull.log.swap(t.log);
        pull.atoms_h = rows.ids;
        for (int c = 0; c < PULL_MAX_COORDS; c++) { pull.coord[c] = rows.coord[c]; pull.xi0[c] = rows.r0[c]; }
        for (int g = 0; g <= PULL_MAX_GROUPS; g++) pull.chunk_of_group[g] = rows.lay.chunk_of_group[g];
        pull.n_groups = rows.n_groups; pull.n_grouped = rows.lay.n_grouped; pull.n_chunks = (int)rows.lay.chunks.size();
        pull.log_every = log_every; pull.log_capacity = log_capacity;
        pull.steps = 0; pull.log_count = 0; pull.log_dropped = 0;
        pull.closing = false; pull.closing_dt = 0.0; pull.log_slot = -1;
        pull.n = n_coords; pull.limit = lim; pull.present = true;
    }

    // ---- charges (emdee_*_set_coulomb): sqrt(K) q per atom key (caller id or global id, as the other tables), and the
    // reaction-field constants.  Every engine keeps a plane of them in its own cell order (NbSystem::qp).
    DevBuf<double> q_tab;
    DevBuf<double> q_raw;                                    // the charges as the caller gave them (the spatial profiles' sum q)
    int64_t q_n = 0;                                         // keys 0 .. q_n - 1 have a charge
    double coulomb_k = 0.0, eps_rf = INFINITY, scale14c = 1.0;
    double q_sum = 0.0;                                      // sum of sqrt(K) q in key order (the Ewald background term)
    double q_abs = 0.0;                                      // sum of sqrt(K) |q| (the fixed-point scale of the PME charge mesh)
    bool has_charges = false;
    // Replaces the charges by the n at charges_dev (device, fp64, one per key); n = 0 clears them.  want >= 0: the only
    // non-zero n accepted (an undivided engine's atom count).
    void set_charges(const double *charges_dev, int64_t n, double K, double eps, double s14, int64_t want, hipStream_t s) {
        EMDEE_REQUIRE(n >= 0 && (n == 0 || charges_dev), EMDEE_ERR_INVALID, "set_coulomb: negative count or NULL array");
        if (n == 0) {                                        // (clearing needs no constants)
            has_charges = false; q_n = 0; q_h.clear();
            return;
        }
        topo::check_coulomb(n, want, K, eps, s14);
        std::vector<double> h = fetch(charges_dev, (size_t)n, s);
        const std::vector<double> raw = h;                  // (its own copy: the upload is queued, h is scaled in place)
        DevBuf<double> nraw;
        put(nraw, raw, s);
        topo::scale_charges(h, K);
        double sum = 0.0, sum_abs = 0.0;
        for (double v : h) { sum += v; sum_abs += std::fabs(v); }
        DevBuf<double> nq;
        put(nq, h, s);
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        // ---- commit
        q_tab.swap(nq);
        q_raw.swap(nraw);
        q_n = n; coulomb_k = K; eps_rf = eps; scale14c = s14; q_sum = sum; q_abs = sum_abs;
        q_h.swap(h);
        has_charges = true;
    }
    std::vector<double> q_h;                                 // the host copy (the alchemical table's readiness check: a flagged atom carries charge 0)

    // ---- soft-core alchemical decoupling (emdee_md_set_alchemical; alchemical.hpp), undivided engines only: the flag of every caller
    // id on the device (GroupTable: atoms_h the flagged ids, n their count), the words of a read and the log.  The host owns lambda,
    // alpha, the foreign lambdas, the count of completed steps and the log's bookkeeping; the struck entries of a build are the
    // engine's (NbSystem::alch_*).
    struct AlchTable : GroupTable {
        DevBuf<int> flag;
        DevBuf<double> out, log;                             // out: ALCH_WORDS, then the foreign energies; log: capacity x (2 + n_foreign)
        double lambda = 1.0, alpha = 0.0, foreign[ALCH_MAX_FOREIGN] = {};
        int n_foreign = 0;
        int log_every = 0, log_capacity = 0;
        long long steps = 0, log_count = 0, log_dropped = 0; // completed steps since the set; entries written; samples dropped
        int log_slot = -1;                                   // the entry the next force pass writes (set by advance(), taken by NbSystem::add_alchemical)
        // the Coulomb stage (emdee_md_set_alchemical_coulomb): off until it is set; its own words and its own log, on the table's
        // cadence and capacity, entry j at the same pass as entry j of `log`
        bool coulomb = false;
        double lambda_q = 1.0, beta = 0.0, foreign_q[ALCH_MAX_FOREIGN] = {};
        DevBuf<double> out_q, log_q;                         // out_q: ALCH_COULOMB_WORDS, then the foreign U_q; log_q: capacity x (2 + n_foreign)
        void advance() {
            steps++;
            log_slot = -1;
            if (log_capacity > 0 && log_every > 0 && steps % log_every == 0) {
                if (log_count < log_capacity) log_slot = (int)log_count++; else log_dropped++;
            }
        }
    };
    AlchTable alch;
    // Replaces the table by the one the arrays describe (flag_dev: device, `lim` ints; foreign: host); flag_dev = NULL clears it.  Every
    // refusal comes before the table in force changes.
    void set_alchemical(const int32_t *flag_dev, double lambda, double alpha, const double *foreign, int32_t n_foreign, int32_t log_every,
                        int32_t log_capacity, int64_t lim, hipStream_t s) {
        if (!flag_dev) {
            alch.present = false; alch.n = 0; alch.atoms_h.clear();
            alch.coulomb = false;
            return;
        }
        alch_check_params(lambda, alpha, foreign, n_foreign, log_every, log_capacity);
        const std::vector<int32_t> raw = fetch(flag_dev, (size_t)lim, s);
        const std::vector<int32_t> ids = alch_check_flags(raw);
        AlchTable t;
        put(t.flag, raw, s);
        const size_t words = (size_t)ALCH_WORDS + ALCH_MAX_FOREIGN, log_words = (size_t)log_capacity * (2 + n_foreign) + 1;
        t.out.ensure(words);
        t.log.ensure(log_words);
        EMDEE_HIP_CHECK(hipMemsetAsync(t.out.ptr, 0, words * sizeof(double), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(t.log.ptr, 0, log_words * sizeof(double), s));
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        // ---- commit
        alch.flag.swap(t.flag); alch.out.swap(t.out); alch.log.swap(t.log);
        alch.atoms_h = ids;
        alch.lambda = lambda; alch.alpha = alpha; alch.n_foreign = n_foreign;
        for (int k = 0; k < ALCH_MAX_FOREIGN; k++) alch.foreign[k] = k < n_foreign ? foreign[k] : 0.0;
        alch.log_every = log_every; alch.log_capacity = log_capacity;
        alch.steps = 0; alch.log_count = 0; alch.log_dropped = 0; alch.log_slot = -1;
        alch.n = (int)ids.size(); alch.limit = lim; alch.present = true;
        alch.coulomb = false;                                // (a new table starts without the Coulomb stage)
    }
    // The Coulomb stage of the table in force (foreign_q: host); enable = 0 clears it, the other arguments unread.  Every refusal comes
    // before anything changes.  Setting it restarts the table's count of steps and both logs.
    void set_alchemical_coulomb(int32_t enable, double lambda_q, double beta, const double *foreign_q, int32_t n_foreign, hipStream_t s) {
        if (!enable) {
            alch.coulomb = false;
            return;
        }
        alch_coulomb_check_params(lambda_q, beta, foreign_q, n_foreign, alch.n_foreign);
        const size_t words = (size_t)ALCH_COULOMB_WORDS + ALCH_MAX_FOREIGN, log_words = (size_t)alch.log_capacity * (2 + alch.n_foreign) + 1;
        DevBuf<double> out_q, log_q;
        out_q.ensure(words);
        log_q.ensure(log_words);
        EMDEE_HIP_CHECK(hipMemsetAsync(out_q.ptr, 0, words * sizeof(double), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(log_q.ptr, 0, log_words * sizeof(double), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(alch.log.ptr, 0, log_words * sizeof(double), s));
        EMDEE_HIP_CHECK(hipStreamSynchronize(s));
        // ---- commit
        alch.out_q.swap(out_q); alch.log_q.swap(log_q);
        alch.lambda_q = lambda_q; alch.beta = beta;
        for (int k = 0; k < ALCH_MAX_FOREIGN; k++) alch.foreign_q[k] = k < n_foreign ? foreign_q[k] : 0.0;
        alch.steps = 0; alch.log_count = 0; alch.log_dropped = 0; alch.log_slot = -1;
        alch.coulomb = true;
    }
};

}  // namespace emdee
