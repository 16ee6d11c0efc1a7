// topology.hpp -- the host side of the topology tables: exclusions and 1-4 pairs, bonded terms, rigid molecules, hbonds clusters, whole
// molecules, virtual sites, position restraints, the centre-of-mass pull, charges.  Plain C++17 on
// std::vector, no HIP: every function here validates or builds and throws through EMDEE_REQUIRE before it returns anything, so
// a stand-alone host program can test it (tests/c/topology_host.cpp).  topology_dev.hpp holds the device buffers.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "error.hpp"
#include "molecule.hpp"
#include "pull.hpp"

namespace emdee {
namespace topo {

// pairs of the lists a and b ({i, j, i, j, ...}) -> rows 0 .. rows - 1: start[rows + 1], partners ascending, no duplicates
inline void csr(const std::vector<int32_t> &a, const std::vector<int32_t> &b, int rows, std::vector<int32_t> &st,
                std::vector<int32_t> &ix) {
    st.assign((size_t)rows + 1, 0);
    for (const std::vector<int32_t> *h : {&a, &b})
        for (size_t k = 0; k < h->size(); k++) st[(size_t)(*h)[k] + 1]++;
    for (int r = 0; r < rows; r++) st[(size_t)r + 1] += st[r];
    ix.assign(st[rows], 0);
    std::vector<int32_t> at(st.begin(), st.end() - 1);
    for (const std::vector<int32_t> *h : {&a, &b})
        for (size_t k = 0; k + 1 < h->size(); k += 2) {
            const int32_t g = (*h)[k], q = (*h)[k + 1];
            ix[at[g]++] = q;
            ix[at[q]++] = g;
        }
    size_t w = 0;
    for (int r = 0; r < rows; r++) {
        const size_t lo = st[r], hi = st[(size_t)r + 1];
        std::sort(ix.begin() + lo, ix.begin() + hi);
        st[r] = (int32_t)w;
        for (size_t k = lo; k < hi; k++)
            if (k == lo || ix[k] != ix[k - 1]) ix[w++] = ix[k];
    }
    st[rows] = (int32_t)w;
    ix.resize(w);
}

// ---- exclusions and 1-4 pairs
// the pairs as a caller gave them ({i, j, ...}, int32 or int64 ids): each two different ids in [0, lim), else refused
template <typename T>
std::vector<int32_t> checked_pairs(const char *what, const std::vector<T> &raw, int64_t lim) {
    for (size_t k = 0; k + 1 < raw.size(); k += 2) {
        const int64_t i = raw[k], j = raw[k + 1];
        EMDEE_REQUIRE(i != j && i >= 0 && j >= 0 && i < lim && j < lim, EMDEE_ERR_INVALID,
                      "%s: pair %lld = (%lld, %lld) is not a pair of two different ids in [0, %lld)", what, (long long)(k / 2),
                      (long long)i, (long long)j, (long long)lim);
    }
    return std::vector<int32_t>(raw.begin(), raw.end());
}
// Both tables are symmetric, sorted, duplicate-free CSRs over ids 0 .. rows - 1 (max id + 1).
struct PairCsrs {
    std::vector<int32_t> xs, xi;                             // struck from the rows: the exclusions and the 1-4 pairs together
    std::vector<int32_t> ps, pi;                             // the 1-4 pairs
    int rows = 0;
    size_t n14 = 0;                                          // entries of the 1-4 CSR
    bool has_excl = false, has_14 = false;
};
inline PairCsrs build_pairs(const std::vector<int32_t> &excl, const std::vector<int32_t> &p14) {
    PairCsrs t;
    for (const std::vector<int32_t> *h : {&excl, &p14})
        for (int32_t g : *h) t.rows = std::max(t.rows, g + 1);
    csr(excl, p14, t.rows, t.xs, t.xi);
    csr(p14, std::vector<int32_t>{}, t.rows, t.ps, t.pi);
    t.n14 = t.pi.size();
    t.has_excl = !t.xi.empty(); t.has_14 = !t.pi.empty();
    return t;
}

// ---- bonded terms: kinds 1 (bond), 2 (angle), 3 (torsion); arrays over kinds have KINDS entries, entry 0 unused
constexpr int KINDS = 4;
inline int kind_atoms(int kind) { return kind + 1; }
inline int kind_params(int kind) { return kind == 3 ? 3 : 2; }
inline const char *kind_name(int kind) {
    static const char *const names[KINDS] = {"", "bond", "angle", "torsion"};
    return names[kind];
}
// term number (over all kinds, in kind order) -> kind and index within it
inline void bonded_term_of(const std::vector<int32_t> (&atoms)[KINDS], int64_t id, int &kind, int64_t &index) {
    for (kind = 1; kind < KINDS - 1 && id >= (int64_t)(atoms[kind].size() / kind_atoms(kind)); kind++)
        id -= (int64_t)(atoms[kind].size() / kind_atoms(kind));
    index = id;
}
// The terms of one kind as a caller gave them (kind_atoms(kind) ids and kind_params(kind) doubles per term), to replace that
// kind of `atoms`: ids in [0, lim) and all different within a term, parameters finite and in range, fewer than 2^31 - 1 terms
// over all kinds; else refused.
template <typename T>
std::vector<int32_t> checked_terms(int kind, const std::vector<T> &raw, const std::vector<double> &prm, int64_t lim,
                                   const std::vector<int32_t> (&atoms)[KINDS]) {
    const int na = kind_atoms(kind), np = kind_params(kind);
    const int64_t n = (int64_t)(raw.size() / na);
    for (int64_t k = 0; k < n; k++) {
        for (int a = 0; a < na; a++) {
            const int64_t g = raw[(size_t)na * k + a];
            EMDEE_REQUIRE(g >= 0 && g < lim, EMDEE_ERR_INVALID, "set_bonded: %s %lld names id %lld, outside [0, %lld)", kind_name(kind),
                          (long long)k, (long long)g, (long long)lim);
            for (int b = 0; b < a; b++)
                EMDEE_REQUIRE(raw[(size_t)na * k + b] != raw[(size_t)na * k + a], EMDEE_ERR_INVALID,
                              "set_bonded: %s %lld names atom %lld twice", kind_name(kind), (long long)k, (long long)g);
        }
        const double *q = prm.data() + (size_t)np * k;
        for (int c = 0; c < np; c++)
            EMDEE_REQUIRE(std::isfinite(q[c]), EMDEE_ERR_INVALID, "set_bonded: %s %lld has a non-finite parameter", kind_name(kind), (long long)k);
        if (kind == 1) EMDEE_REQUIRE(q[1] >= 0.0, EMDEE_ERR_INVALID, "set_bonded: bond %lld has r0 < 0", (long long)k);
        if (kind == 2) EMDEE_REQUIRE(q[1] >= 0.0 && q[1] <= M_PI, EMDEE_ERR_INVALID, "set_bonded: angle %lld has theta0 outside [0, pi]", (long long)k);
        if (kind == 3) EMDEE_REQUIRE(q[1] >= 1.0 && q[1] == std::floor(q[1]), EMDEE_ERR_INVALID,
                                     "set_bonded: torsion %lld has a periodicity that is not an integer >= 1", (long long)k);
    }
    int64_t total = n;
    for (int kd = 1; kd < KINDS; kd++)
        if (kd != kind) total += (int64_t)(atoms[kd].size() / kind_atoms(kd));
    EMDEE_REQUIRE(total < INT32_MAX, EMDEE_ERR_INVALID, "set_bonded: %lld terms in all (at most 2^31 - 2)", (long long)total);
    return std::vector<int32_t>(raw.begin(), raw.end());
}
// One term entry of an atom's row (kernels.hpp BondedKeys; the device reads it as an int4): code = kind | role << 2 (role: the
// atom's position in the term), loc = the other atoms of the term, in term order, as positions in the atom's partner row.
struct TermEntry {
    int32_t code, loc[3];
};
// Rows 0 .. rows - 1 list each atom's bonded partners (ps / pi: ascending, unique) and its term entries (ts / terms, in (kind,
// term, role) order); per entry the term's number over all kinds (tid) and three parameters, zero padded (pd; pf the same in fp32).
struct BondedRows {
    std::vector<int32_t> ps, pi, ts, tid;
    std::vector<TermEntry> terms;
    std::vector<double> pd;
    std::vector<float> pf;
    int rows = 0;
    size_t nb = 0;                                           // entries of the partner CSR (slots of the row filter)
};
inline BondedRows build_bonded(const std::vector<int32_t> *const (&at)[KINDS], const std::vector<double> *const (&pr)[KINDS]) {
    BondedRows t;
    // partners: (owner, partner) over every role of every term -> CSR, ascending, unique
    for (int kd = 1; kd < KINDS; kd++)
        for (int32_t g : *at[kd]) t.rows = std::max(t.rows, g + 1);
    const int r = t.rows;
    std::vector<int32_t> half;                               // each partner pair once (csr() makes the rows symmetric)
    for (int kd = 1; kd < KINDS; kd++) {
        const int nk = kind_atoms(kd);
        for (size_t k = 0; k + nk <= at[kd]->size(); k += nk)
            for (int a = 0; a < nk; a++)
                for (int b = 0; b < nk; b++)
                    if ((*at[kd])[k + a] < (*at[kd])[k + b]) { half.push_back((*at[kd])[k + a]); half.push_back((*at[kd])[k + b]); }
    }
    csr(half, std::vector<int32_t>{}, r, t.ps, t.pi);
    t.nb = t.pi.size();
    // term entries, in (kind, term, role) order within each row
    t.ts.assign((size_t)r + 1, 0);
    for (int kd = 1; kd < KINDS; kd++)
        for (int32_t g : *at[kd]) t.ts[(size_t)g + 1]++;
    for (int q = 0; q < r; q++) t.ts[(size_t)q + 1] += t.ts[q];
    t.terms.resize(t.ts[r]);
    t.tid.resize(t.ts[r]);
    t.pd.assign((size_t)3 * t.ts[r], 0.0);
    t.pf.assign((size_t)3 * t.ts[r], 0.f);
    std::vector<int32_t> fill(t.ts.begin(), t.ts.end() - 1);
    int32_t number = 0;
    for (int kd = 1; kd < KINDS; kd++) {
        const int nk = kind_atoms(kd), npk = kind_params(kd);
        for (size_t k = 0; k + nk <= at[kd]->size(); k += nk, number++) {
            const int32_t *ids = at[kd]->data() + k;
            const double *q = pr[kd]->data() + (k / nk) * npk;
            for (int role = 0; role < nk; role++) {
                const int32_t g = ids[role];
                const int e = fill[g]++;
                int loc[3] = {0, 0, 0}, c = 0;
                for (int a = 0; a < nk; a++) {
                    if (a == role) continue;
                    const auto it = std::lower_bound(t.pi.begin() + t.ps[g], t.pi.begin() + t.ps[(size_t)g + 1], ids[a]);
                    loc[c++] = (int)(it - (t.pi.begin() + t.ps[g]));
                }
                t.terms[e] = TermEntry{kd | role << 2, {loc[0], loc[1], loc[2]}};
                t.tid[e] = number;
                for (int c2 = 0; c2 < npk; c2++) { t.pd[(size_t)3 * e + c2] = q[c2]; t.pf[(size_t)3 * e + c2] = (float)q[c2]; }
            }
        }
    }
    return t;
}
// the error text for term number `term` (as tid numbers them) whose owner did not find a partner in its rows
inline std::string lost_partner_message(const std::vector<int32_t> (&atoms)[KINDS], int64_t term) {
    int kind;
    int64_t index;
    bonded_term_of(atoms, term, kind, index);
    const int na = kind_atoms(kind);
    const int32_t *ids = atoms[kind].data() + (size_t)na * index;
    char text[1024];
    snprintf(text, sizeof(text), "bonded %s %lld (atoms %d %d%s%s%s%s): a partner is farther than rc + skin from its owner at a neighbour-list "
             "build, so the term cannot be evaluated; replace the tables or the state", kind_name(kind), (long long)index, ids[0], ids[1],
             na > 2 ? " " : "", na > 2 ? std::to_string(ids[2]).c_str() : "", na > 3 ? " " : "", na > 3 ? std::to_string(ids[3]).c_str() : "");
    return text;
}

// (defined with the site table below) no atom of a constraint table may be a site of the site table in force
inline void refuse_constrained_sites(const char *name, const char *noun, int sites_per_group, const std::vector<int32_t> &ids,
                                     const std::vector<int32_t> *vsites);

// ---- rigid three-site molecules (emdee_md_set_rigid3): {apex, a, b} ids and {d_leg, d_base} per molecule
// The table as a caller gave it: ids in [0, lim), no atom named twice within or across molecules, distances finite and > 0 with
// d_base < 2 d_leg (a triangle), and no atom that the hbonds table in force names (`hbonds`: its ids, -1 in unused slots; NULL:
// none in force), and no atom that is a site of the site table in force (`vsites`: its {site, a, b, c} ids; NULL: none); else refused.
template <typename T>
std::vector<int32_t> checked_rigid3(const std::vector<T> &raw, const std::vector<double> &geom, int64_t lim,
                                    const std::vector<int32_t> *hbonds = nullptr, const std::vector<int32_t> *vsites = nullptr) {
    const int64_t n = (int64_t)(raw.size() / 3);
    EMDEE_REQUIRE((int64_t)geom.size() == 2 * n, EMDEE_ERR_INVALID, "set_rigid3: %lld molecules but %lld distances", (long long)n, (long long)geom.size());
    EMDEE_REQUIRE(n <= INT32_MAX / 3, EMDEE_ERR_INVALID, "set_rigid3: %lld molecules (at most (2^31 - 1) / 3)", (long long)n);
    std::vector<std::pair<int64_t, int64_t>> named;           // (id, molecule)
    named.reserve((size_t)3 * n);
    for (int64_t k = 0; k < n; k++) {
        for (int a = 0; a < 3; a++) {
            const int64_t g = raw[(size_t)3 * k + a];
            EMDEE_REQUIRE(g >= 0 && g < lim, EMDEE_ERR_INVALID, "set_rigid3: molecule %lld names id %lld, outside [0, %lld)", (long long)k,
                          (long long)g, (long long)lim);
            named.emplace_back(g, k);
        }
        const double d_leg = geom[(size_t)2 * k], d_base = geom[(size_t)2 * k + 1];
        EMDEE_REQUIRE(std::isfinite(d_leg) && std::isfinite(d_base) && d_leg > 0.0 && d_base > 0.0, EMDEE_ERR_INVALID,
                      "set_rigid3: molecule %lld has a distance that is not finite and > 0", (long long)k);
        EMDEE_REQUIRE(d_base < 2.0 * d_leg, EMDEE_ERR_INVALID, "set_rigid3: molecule %lld has d_base = %g >= 2 d_leg = %g (no triangle)",
                      (long long)k, d_base, 2.0 * d_leg);
    }
    std::sort(named.begin(), named.end());
    for (size_t k = 1; k < named.size(); k++)
        EMDEE_REQUIRE(named[k].first != named[k - 1].first, EMDEE_ERR_INVALID, "set_rigid3: atom %lld is named twice (molecules %lld and %lld)",
                      (long long)named[k].first, (long long)named[k - 1].second, (long long)named[k].second);
    if (hbonds) {
        std::vector<int32_t> taken(*hbonds);
        std::sort(taken.begin(), taken.end());
        for (const auto &a : named)
            EMDEE_REQUIRE(!std::binary_search(taken.begin(), taken.end(), (int32_t)a.first), EMDEE_ERR_INVALID, "set_rigid3: atom %lld of molecule %lld "
                          "belongs to a cluster of the hbonds table in force (emdee_md_set_hbonds): an atom is held by one table",
                          (long long)a.first, (long long)a.second);
    }
    const std::vector<int32_t> out(raw.begin(), raw.end());
    refuse_constrained_sites("set_rigid3", "molecule", 3, out, vsites);
    return out;
}
// one byte per id in [0, lim): 1 for the atoms a (checked) table names, 0 for the others -- the one-atom molecules of the
// molecular scale (emdee_md_set_molecular_scaling), which the atom-by-atom scale kernel still moves
inline std::vector<uint8_t> rigid3_members(const std::vector<int32_t> &atoms, int64_t lim) {
    std::vector<uint8_t> member((size_t)std::max<int64_t>(lim, 0), 0);
    for (int32_t g : atoms)
        if (g >= 0 && g < lim) member[(size_t)g] = 1;
    return member;
}
// the error texts of the device checks (molecule: the number the kernels report, from 0)
inline std::string rigid3_message(const std::vector<int32_t> &atoms, int64_t molecule, const char *what) {
    char text[512];
    const bool in = molecule >= 0 && (size_t)(3 * molecule + 2) < atoms.size();
    snprintf(text, sizeof(text), "rigid molecule %lld (atoms %d %d %d): %s", (long long)molecule, in ? atoms[(size_t)3 * molecule] : -1,
             in ? atoms[(size_t)3 * molecule + 1] : -1, in ? atoms[(size_t)3 * molecule + 2] : -1, what);
    return text;
}

// ---- bonds to hydrogen (emdee_md_set_hbonds): star clusters {centre, s1, s2, s3} with -1 in the unused trailing slots, and the
// three centre-satellite distances per cluster
// The table as a caller gave it: ids in [0, lim), at least one satellite, no id after a -1, no atom named twice within or across
// clusters, none that the rigid table in force names (`rigid`: its ids; NULL: none in force), none that is a site of the site
// table in force (`vsites`: its {site, a, b, c} ids; NULL: none), the distance of every slot in use finite and > 0; else refused.
template <typename T>
std::vector<int32_t> checked_hbonds(const std::vector<T> &raw, const std::vector<double> &dist, int64_t lim,
                                    const std::vector<int32_t> *rigid = nullptr, const std::vector<int32_t> *vsites = nullptr) {
    const int64_t n = (int64_t)(raw.size() / 4);
    EMDEE_REQUIRE((int64_t)dist.size() == 3 * n, EMDEE_ERR_INVALID, "set_hbonds: %lld clusters but %lld distances", (long long)n, (long long)dist.size());
    EMDEE_REQUIRE(n <= INT32_MAX / 4, EMDEE_ERR_INVALID, "set_hbonds: %lld clusters (at most (2^31 - 1) / 4)", (long long)n);
    std::vector<std::pair<int64_t, int64_t>> named;           // (id, cluster)
    named.reserve((size_t)4 * n);
    std::vector<int32_t> out((size_t)4 * n, -1);
    for (int64_t k = 0; k < n; k++) {
        bool ended = false;
        for (int a = 0; a < 4; a++) {
            const int64_t g = raw[(size_t)4 * k + a];
            if (a >= 1 && g == -1) {
                EMDEE_REQUIRE(a >= 2, EMDEE_ERR_INVALID, "set_hbonds: cluster %lld is empty (its first satellite is -1)", (long long)k);
                ended = true;
                continue;
            }
            EMDEE_REQUIRE(g >= 0 && g < lim, EMDEE_ERR_INVALID, "set_hbonds: cluster %lld names id %lld, outside [0, %lld)", (long long)k,
                          (long long)g, (long long)lim);
            EMDEE_REQUIRE(!ended, EMDEE_ERR_INVALID, "set_hbonds: cluster %lld names id %lld after a -1 (unused slots are the trailing ones)",
                          (long long)k, (long long)g);
            const double d = dist[(size_t)3 * k + (a >= 1 ? a - 1 : 0)];
            EMDEE_REQUIRE(a == 0 || (std::isfinite(d) && d > 0.0), EMDEE_ERR_INVALID, "set_hbonds: cluster %lld has a distance that is not "
                          "finite and > 0 (satellite %d)", (long long)k, a);
            named.emplace_back(g, k);
            out[(size_t)4 * k + a] = (int32_t)g;
        }
    }
    std::sort(named.begin(), named.end());
    for (size_t k = 1; k < named.size(); k++)
        EMDEE_REQUIRE(named[k].first != named[k - 1].first, EMDEE_ERR_INVALID, "set_hbonds: atom %lld is named twice (clusters %lld and %lld)",
                      (long long)named[k].first, (long long)named[k - 1].second, (long long)named[k].second);
    if (rigid) {
        std::vector<int32_t> taken(*rigid);
        std::sort(taken.begin(), taken.end());
        for (const auto &a : named)
            EMDEE_REQUIRE(!std::binary_search(taken.begin(), taken.end(), (int32_t)a.first), EMDEE_ERR_INVALID, "set_hbonds: atom %lld of cluster %lld "
                          "belongs to a molecule of the rigid table in force (emdee_md_set_rigid3): an atom is held by one table",
                          (long long)a.first, (long long)a.second);
    }
    refuse_constrained_sites("set_hbonds", "cluster", 4, out, vsites);
    return out;
}
// the distances as the kernels read them: those of the unused slots are 0 (never read as a length)
inline std::vector<double> hbonds_distances(const std::vector<int32_t> &atoms, const std::vector<double> &dist) {
    std::vector<double> out(dist);
    for (size_t k = 0; k < out.size(); k++)
        if (atoms[4 * (k / 3) + 1 + k % 3] < 0) out[k] = 0.0;
    return out;
}
// the error texts of the device checks (cluster: the number the kernels report, from 0)
inline std::string hbonds_message(const std::vector<int32_t> &atoms, int64_t cluster, const char *what) {
    char text[512];
    const bool in = cluster >= 0 && (size_t)(4 * cluster + 3) < atoms.size();
    std::string ids;
    for (int a = 0; a < 4; a++) {
        const int32_t g = in ? atoms[(size_t)4 * cluster + a] : -1;
        if (a == 0 || g >= 0) ids += (a ? " " : "") + std::to_string(g);
    }
    snprintf(text, sizeof(text), "hbonds cluster %lld (atoms %s): %s", (long long)cluster, ids.c_str(), what);
    return text;
}

// ---- whole molecules (emdee_md_set_molecules; molecule.hpp): one id per atom, >= -1; equal ids >= 0 form one molecule, -1 is a
// molecule of one.  The table the kernels read holds the molecules of two atoms and more (a molecule of one adds exactly 0 to the
// molecular sums and scales as a free atom does): small ones (<= MOL_SMALL atoms) first, sorted by size and then by first atom, the
// large ones behind them by first atom; caller ids ascending within a molecule.  The order depends on the table alone.
struct MoleculeRows {
    int n_mol = 0, n_small = 0;
    std::vector<int32_t> start, atoms, entry_mol;            // the CSR in table order (start: n_mol + 1), the molecule of every entry
    std::vector<int32_t> mol_of;                             // per caller id: its molecule in table order, -1 for a molecule of one
    std::vector<int32_t> label;                              // per molecule in table order: the id the caller gave it
    std::vector<int32_t> compact;                            // per caller id: its molecule in order of first appearance (every atom has one)
    std::vector<uint8_t> member;                             // per caller id: 1 for the atoms of the table (k_cell_state_scale passes them over)
};
// the atoms of a molecule, for the error texts: at most eight ids, then their number
inline std::string molecule_atoms_text(const MoleculeRows &t, int64_t mol) {
    if (mol < 0 || mol >= t.n_mol) return "?";
    std::string ids;
    const int first = t.start[(size_t)mol], end = t.start[(size_t)mol + 1];
    for (int e = first; e < end && e < first + 8; e++) ids += (e > first ? " " : "") + std::to_string(t.atoms[(size_t)e]);
    if (end - first > 8) ids += " ... (" + std::to_string(end - first) + " atoms)";
    return ids;
}
// the error texts of the device checks (molecule: the number the kernels report, in table order)
inline std::string molecule_message(const MoleculeRows &t, int64_t mol, const char *what) {
    const bool in = mol >= 0 && mol < t.n_mol;
    return "molecule " + std::to_string(in ? t.label[(size_t)mol] : -1) + " of the molecule table (atoms " + molecule_atoms_text(t, mol) + "): " + what;
}
// Every constraint must lie inside one molecule: refused if a group of `ids` (`sites` per group, -1 in unused slots) has atoms that
// do not all carry one id >= 0 of `molecule` (one id per caller id).  name: the call that refuses; noun: "rigid molecule" or
// "hbonds cluster"; setter: the call that set the groups.
inline void refuse_split_groups(const char *name, const char *noun, const char *setter, int sites, const std::vector<int32_t> &ids,
                                const std::vector<int32_t> &molecule) {
    for (size_t g = 0; g < ids.size() / (size_t)sites; g++) {
        std::string text;
        int32_t first = -1, m0 = -1;
        for (int a = 0; a < sites; a++)
            if (ids[(size_t)sites * g + a] >= 0) text += (text.empty() ? "" : " ") + std::to_string(ids[(size_t)sites * g + a]);
        for (int a = 0; a < sites; a++) {
            const int32_t id = ids[(size_t)sites * g + a];
            if (id < 0 || (size_t)id >= molecule.size()) continue;
            const int32_t m = molecule[(size_t)id];
            EMDEE_REQUIRE(m >= 0, EMDEE_ERR_INVALID, "%s: %s %lld (atoms %s, %s) has atom %d in no molecule of the molecule table (id -1, "
                          "emdee_md_set_molecules): a constraint must lie inside one molecule", name, noun, (long long)g, text.c_str(), setter, id);
            if (first < 0) { first = id; m0 = m; }
            EMDEE_REQUIRE(m == m0, EMDEE_ERR_INVALID, "%s: %s %lld (atoms %s, %s) is split by the molecule table (emdee_md_set_molecules): atom "
                          "%d is in molecule %d, atom %d in molecule %d; a constraint must lie inside one molecule", name, noun, (long long)g,
                          text.c_str(), setter, first, m0, id, m);
        }
    }
}
// The table from the ids as a caller gave them (`rigid`, `hbonds`: the ids of the constraint tables in force; NULL: none): ids >= -1,
// no constraint group split or left at -1; else refused.
template <typename T>
MoleculeRows molecule_table(const std::vector<T> &raw, int64_t lim, const std::vector<int32_t> *rigid = nullptr,
                            const std::vector<int32_t> *hbonds = nullptr) {
    EMDEE_REQUIRE((int64_t)raw.size() == lim, EMDEE_ERR_INVALID, "set_molecules: %lld ids, the state holds %lld atoms (one id per atom; "
                  "n = 0 clears the table)", (long long)raw.size(), (long long)lim);
    const size_t n = raw.size();
    std::vector<int32_t> given(n);
    for (size_t i = 0; i < n; i++) {
        EMDEE_REQUIRE(raw[i] >= -1 && raw[i] <= INT32_MAX, EMDEE_ERR_INVALID, "set_molecules: the molecule %lld of atom %lld is below -1 "
                      "(-1: a molecule of one)", (long long)raw[i], (long long)i);
        given[i] = (int32_t)raw[i];
    }
    if (rigid) refuse_split_groups("set_molecules", "rigid molecule", "emdee_md_set_rigid3", 3, *rigid, given);
    if (hbonds) refuse_split_groups("set_molecules", "hbonds cluster", "emdee_md_set_hbonds", 4, *hbonds, given);
    // compaction in order of first appearance by caller id
    MoleculeRows t;
    t.compact.assign(n, -1); t.mol_of.assign(n, -1); t.member.assign(n, 0);
    std::vector<std::pair<int32_t, int32_t>> seen;            // (given id, atom), sorted: equal ids side by side, atoms ascending
    for (size_t i = 0; i < n; i++)
        if (given[i] >= 0) seen.emplace_back(given[i], (int32_t)i);
    std::sort(seen.begin(), seen.end());
    struct Mol { int32_t first, size, label; size_t at; };
    std::vector<Mol> mols;
    for (size_t k = 0; k < seen.size(); k++) {
        if (k == 0 || seen[k].first != seen[k - 1].first) mols.push_back(Mol{seen[k].second, 0, seen[k].first, k});
        mols.back().size++;
    }
    for (size_t i = 0; i < n; i++)
        if (given[i] < 0) mols.push_back(Mol{(int32_t)i, 1, -1, 0});
    std::sort(mols.begin(), mols.end(), [](const Mol &a, const Mol &b) { return a.first < b.first; });
    for (size_t c = 0; c < mols.size(); c++) {
        if (mols[c].label < 0) { t.compact[(size_t)mols[c].first] = (int32_t)c; continue; }
        for (int32_t k = 0; k < mols[c].size; k++) t.compact[(size_t)seen[mols[c].at + k].second] = (int32_t)c;
    }
    // the table order: molecules of one left out, size classes, the small class by size, then by first atom
    std::vector<Mol> order;
    for (const Mol &m : mols)
        if (m.size >= 2) order.push_back(m);
    std::sort(order.begin(), order.end(), [](const Mol &a, const Mol &b) {
        const int32_t ka = a.size <= MOL_SMALL ? a.size : MOL_SMALL + 1, kb = b.size <= MOL_SMALL ? b.size : MOL_SMALL + 1;
        return ka != kb ? ka < kb : a.first < b.first;
    });
    t.n_mol = (int)order.size();
    t.start.push_back(0);
    for (size_t m = 0; m < order.size(); m++) {
        if (order[m].size <= MOL_SMALL) t.n_small = (int)m + 1;
        t.label.push_back(order[m].label);
        for (int32_t k = 0; k < order[m].size; k++) {
            const int32_t id = seen[order[m].at + k].second;
            t.atoms.push_back(id); t.entry_mol.push_back((int32_t)m);
            t.mol_of[(size_t)id] = (int32_t)m; t.member[(size_t)id] = 1;
        }
        t.start.push_back((int32_t)t.atoms.size());
    }
    return t;
}

// ---- virtual interaction sites (emdee_md_set_vsites; vsite.hpp): {site, a, b, c} ids per entry, c = -1 for a two-parent site,
// and the weights {w_b, w_c} (w_c ignored where c = -1)
// The table as a caller gave it: ids in [0, lim) (c may be -1), no atom named twice within an entry, no atom that is a site in two
// entries, no site that is a parent of another site, no site that the rigid, the hbonds or the restraint table in force names (`rigid`,
// `hbonds`, `restrained`: their ids; NULL: none in force), no site in a group of the pull table in force (`pulled`: the grouped ids), the
// weights in use finite; else refused.  Parents may belong to any table.
template <typename T>
std::vector<int32_t> checked_vsites(const std::vector<T> &raw, const std::vector<double> &weights, int64_t lim,
                                    const std::vector<int32_t> *rigid = nullptr, const std::vector<int32_t> *hbonds = nullptr,
                                    const std::vector<int32_t> *restrained = nullptr, const std::vector<int32_t> *pulled = nullptr) {
    const int64_t n = (int64_t)(raw.size() / 4);
    EMDEE_REQUIRE((int64_t)weights.size() == 2 * n, EMDEE_ERR_INVALID, "set_vsites: %lld sites but %lld weights", (long long)n, (long long)weights.size());
    EMDEE_REQUIRE(n <= INT32_MAX / 4, EMDEE_ERR_INVALID, "set_vsites: %lld sites (at most (2^31 - 1) / 4)", (long long)n);
    std::vector<std::pair<int64_t, int64_t>> sites, parents;  // (id, entry)
    sites.reserve((size_t)n); parents.reserve((size_t)3 * n);
    for (int64_t k = 0; k < n; k++) {
        for (int a = 0; a < 4; a++) {
            const int64_t g = raw[(size_t)4 * k + a];
            if (a == 3 && g == -1) continue;
            EMDEE_REQUIRE(g >= 0 && g < lim, EMDEE_ERR_INVALID, "set_vsites: site %lld names id %lld, outside [0, %lld)%s", (long long)k,
                          (long long)g, (long long)lim, a == 3 ? " (c = -1 makes a two-parent site)" : "");
            for (int b = 0; b < a; b++)
                EMDEE_REQUIRE(raw[(size_t)4 * k + b] != raw[(size_t)4 * k + a], EMDEE_ERR_INVALID, "set_vsites: site %lld names atom %lld twice",
                              (long long)k, (long long)g);
            (a == 0 ? sites : parents).emplace_back(g, k);
        }
        const bool three = raw[(size_t)4 * k + 3] != -1;
        EMDEE_REQUIRE(std::isfinite(weights[(size_t)2 * k]) && (!three || std::isfinite(weights[(size_t)2 * k + 1])), EMDEE_ERR_INVALID,
                      "set_vsites: site %lld has a weight that is not finite", (long long)k);
    }
    std::sort(sites.begin(), sites.end());
    for (size_t k = 1; k < sites.size(); k++)
        EMDEE_REQUIRE(sites[k].first != sites[k - 1].first, EMDEE_ERR_INVALID, "set_vsites: atom %lld is the site of two entries (%lld and %lld)",
                      (long long)sites[k].first, (long long)sites[k - 1].second, (long long)sites[k].second);
    for (const auto &p : parents) {
        const auto it = std::lower_bound(sites.begin(), sites.end(), std::make_pair(p.first, (int64_t)-1));
        EMDEE_REQUIRE(it == sites.end() || it->first != p.first, EMDEE_ERR_INVALID, "set_vsites: atom %lld, the site of entry %lld, is a parent "
                      "of site %lld (a site is built on atoms with mass)", (long long)p.first, it == sites.end() ? -1LL : (long long)it->second,
                      (long long)p.second);
    }
    const std::vector<int32_t> *const held[2] = {rigid, hbonds};
    const char *const holder[2] = {"a molecule of the rigid table in force (emdee_md_set_rigid3)", "a cluster of the hbonds table in force (emdee_md_set_hbonds)"};
    if (restrained) {                                        // (the mirror of restraint_table's refusal)
        std::vector<int32_t> taken(*restrained);
        std::sort(taken.begin(), taken.end());
        for (const auto &s : sites)
            EMDEE_REQUIRE(!std::binary_search(taken.begin(), taken.end(), (int32_t)s.first), EMDEE_ERR_INVALID, "set_vsites: atom %lld, the site of "
                          "entry %lld, is named by the restraint table in force (emdee_md_set_restraints): a site is massless and follows its "
                          "parents, it cannot be restrained", (long long)s.first, (long long)s.second);
    }
    if (pulled) {                                            // (the mirror of pull_table's refusal)
        std::vector<int32_t> taken(*pulled);
        std::sort(taken.begin(), taken.end());
        for (const auto &s : sites)
            EMDEE_REQUIRE(!std::binary_search(taken.begin(), taken.end(), (int32_t)s.first), EMDEE_ERR_INVALID, "set_vsites: atom %lld, the site of "
                          "entry %lld, is in a group of the pull table in force (emdee_md_set_pull): a site is massless, a centre of mass "
                          "cannot hold it", (long long)s.first, (long long)s.second);
    }
    for (int t = 0; t < 2; t++) {
        if (!held[t]) continue;
        std::vector<int32_t> taken(*held[t]);
        std::sort(taken.begin(), taken.end());
        for (const auto &s : sites)
            EMDEE_REQUIRE(!std::binary_search(taken.begin(), taken.end(), (int32_t)s.first), EMDEE_ERR_INVALID, "set_vsites: atom %lld, the site of "
                          "entry %lld, belongs to %s: a site is massless and follows its parents, it cannot be constrained", (long long)s.first,
                          (long long)s.second, holder[t]);
    }
    return std::vector<int32_t>(raw.begin(), raw.end());
}
// the weights as the kernels read them: w_c of a two-parent site is 0 (never a number that is not finite)
inline std::vector<double> vsite_weights(const std::vector<int32_t> &atoms, const std::vector<double> &weights) {
    std::vector<double> out(weights);
    for (size_t k = 0; 4 * k + 3 < atoms.size(); k++)
        if (atoms[4 * k + 3] < 0) out[2 * k + 1] = 0.0;
    return out;
}
// the mirror refusal of the two constraint builders: no atom of a (checked) rigid or hbonds table may be a site of the site table
// in force (`vsites`: its {site, a, b, c} ids; NULL: none in force).  Parents may be constrained: that is the point of a site.
inline void refuse_constrained_sites(const char *name, const char *noun, int sites_per_group, const std::vector<int32_t> &ids,
                                     const std::vector<int32_t> *vsites) {
    if (!vsites) return;
    std::vector<int32_t> taken;
    for (size_t k = 0; k + 3 < vsites->size(); k += 4) taken.push_back((*vsites)[k]);
    std::sort(taken.begin(), taken.end());
    for (size_t k = 0; k < ids.size(); k++)
        EMDEE_REQUIRE(ids[k] < 0 || !std::binary_search(taken.begin(), taken.end(), ids[k]), EMDEE_ERR_INVALID, "%s: atom %d of %s %lld is a "
                      "virtual site of the table in force (emdee_md_set_vsites): a site is massless and follows its parents, it cannot be "
                      "constrained", name, ids[k], noun, (long long)(k / (size_t)sites_per_group));
}
// The parent list of a (checked) table with the weights of vsite_weights: the distinct parents in ascending id order, and per
// parent its (entry, weight) pairs in table order -- weight 1 - w_b - w_c for a, w_b for b, w_c for c.  One thread per parent sums
// its pairs in that order (vsite.hpp k_vsite_spread): no floating-point atomics, the same bits in every run.
struct VsiteParents {
    std::vector<int32_t> parent, start, site;
    std::vector<double> weight;
};
inline VsiteParents build_vsite_parents(const std::vector<int32_t> &atoms, const std::vector<double> &weights) {
    VsiteParents t;
    const size_t n = atoms.size() / 4;
    for (size_t k = 0; k < n; k++)
        for (int a = 1; a < 4; a++)
            if (atoms[4 * k + a] >= 0) t.parent.push_back(atoms[4 * k + a]);
    std::sort(t.parent.begin(), t.parent.end());
    t.parent.erase(std::unique(t.parent.begin(), t.parent.end()), t.parent.end());
    const auto row = [&](int32_t g) { return (size_t)(std::lower_bound(t.parent.begin(), t.parent.end(), g) - t.parent.begin()); };
    t.start.assign(t.parent.size() + 1, 0);
    for (size_t k = 0; k < n; k++)
        for (int a = 1; a < 4; a++)
            if (atoms[4 * k + a] >= 0) t.start[row(atoms[4 * k + a]) + 1]++;
    for (size_t q = 0; q < t.parent.size(); q++) t.start[q + 1] += t.start[q];
    t.site.assign((size_t)t.start[t.parent.size()], 0);
    t.weight.assign((size_t)t.start[t.parent.size()], 0.0);
    std::vector<int32_t> fill(t.start.begin(), t.start.end() - 1);
    for (size_t k = 0; k < n; k++) {
        const double w_b = weights[2 * k], w_c = weights[2 * k + 1];
        const double w[4] = {0.0, 1.0 - w_b - w_c, w_b, w_c};
        for (int a = 1; a < 4; a++) {
            if (atoms[4 * k + a] < 0) continue;
            const int32_t e = fill[row(atoms[4 * k + a])]++;
            t.site[(size_t)e] = (int32_t)k;
            t.weight[(size_t)e] = w[a];
        }
    }
    return t;
}
// the error texts of the device check (entry: the number the kernel reports, from 0)
inline std::string vsite_message(const std::vector<int32_t> &atoms, int64_t entry, const char *what) {
    char text[512];
    const bool in = entry >= 0 && (size_t)(4 * entry + 3) < atoms.size();
    snprintf(text, sizeof(text), "virtual site %lld (atoms %d %d %d %d): %s", (long long)entry, in ? atoms[(size_t)4 * entry] : -1,
             in ? atoms[(size_t)4 * entry + 1] : -1, in ? atoms[(size_t)4 * entry + 2] : -1, in ? atoms[(size_t)4 * entry + 3] : -1, what);
    return text;
}

// ---- position restraints (emdee_md_set_restraints; restraint.hpp): one caller id, three references, three spring constants and one
// flat-bottom radius per entry
// The table as the kernels read it, in the caller's order.
struct RestraintRows {
    std::vector<int32_t> atoms;
    std::vector<double> ref, k, flat;
};
// The table as a caller gave it: ids in [0, lim), no atom named twice, every constant and radius finite and >= 0, every reference
// finite, a flat-bottomed entry (r0 > 0) with at least one non-zero constant and all its non-zero constants equal, no entry that is a
// site of the site table in force (`vsites`: its {site, a, b, c} ids; NULL: none in force); else refused, the text naming the entry.
// ref empty: the engine fills the references from the atoms' positions; flat empty: every radius is 0.
template <typename T>
RestraintRows restraint_table(const std::vector<T> &ids, const std::vector<double> &ref, const std::vector<double> &k,
                              const std::vector<double> &flat, int64_t lim, const std::vector<int32_t> *vsites = nullptr) {
    const int64_t n = (int64_t)ids.size();
    EMDEE_REQUIRE((int64_t)k.size() == 3 * n, EMDEE_ERR_INVALID, "set_restraints: %lld entries but %lld spring constants (three per entry)",
                  (long long)n, (long long)k.size());
    EMDEE_REQUIRE(ref.empty() || (int64_t)ref.size() == 3 * n, EMDEE_ERR_INVALID, "set_restraints: %lld entries but %lld reference "
                  "coordinates (three per entry)", (long long)n, (long long)ref.size());
    EMDEE_REQUIRE(flat.empty() || (int64_t)flat.size() == n, EMDEE_ERR_INVALID, "set_restraints: %lld entries but %lld flat-bottom radii",
                  (long long)n, (long long)flat.size());
    EMDEE_REQUIRE(n <= INT32_MAX / 3, EMDEE_ERR_INVALID, "set_restraints: %lld entries (at most (2^31 - 1) / 3)", (long long)n);
    std::vector<std::pair<int64_t, int64_t>> named;          // (id, entry)
    named.reserve((size_t)n);
    for (int64_t e = 0; e < n; e++) {
        const int64_t g = ids[(size_t)e];
        EMDEE_REQUIRE(g >= 0 && g < lim, EMDEE_ERR_INVALID, "set_restraints: entry %lld names id %lld, outside [0, %lld)", (long long)e,
                      (long long)g, (long long)lim);
        named.emplace_back(g, e);
    }
    std::sort(named.begin(), named.end());
    for (size_t q = 1; q < named.size(); q++)
        EMDEE_REQUIRE(named[q].first != named[q - 1].first, EMDEE_ERR_INVALID, "set_restraints: atom %lld is named twice (entries %lld and "
                      "%lld)", (long long)named[q].first, (long long)named[q - 1].second, (long long)named[q].second);
    for (int64_t e = 0; e < n; e++) {
        const double *q = k.data() + 3 * (size_t)e;
        const double r0 = flat.empty() ? 0.0 : flat[(size_t)e];
        for (int a = 0; a < 3; a++)
            EMDEE_REQUIRE(std::isfinite(q[a]) && q[a] >= 0.0, EMDEE_ERR_INVALID, "set_restraints: entry %lld (atom %lld) has a spring constant "
                          "on axis %d that is not finite and >= 0", (long long)e, (long long)ids[(size_t)e], a);
        EMDEE_REQUIRE(std::isfinite(r0) && r0 >= 0.0, EMDEE_ERR_INVALID, "set_restraints: entry %lld (atom %lld) has a flat-bottom radius that "
                      "is not finite and >= 0", (long long)e, (long long)ids[(size_t)e]);
        if (!ref.empty())
            for (int a = 0; a < 3; a++)
                EMDEE_REQUIRE(std::isfinite(ref[3 * (size_t)e + a]), EMDEE_ERR_INVALID, "set_restraints: entry %lld (atom %lld) has a reference "
                              "on axis %d that is not finite", (long long)e, (long long)ids[(size_t)e], a);
        if (r0 > 0.0) {
            double kk = 0.0;
            for (int a = 0; a < 3; a++)
                if (q[a] > 0.0) {
                    EMDEE_REQUIRE(kk == 0.0 || q[a] == kk, EMDEE_ERR_INVALID, "set_restraints: entry %lld (atom %lld) is flat-bottomed (r0 = %g) "
                                  "with unequal non-zero spring constants %g and %g: the well is a sphere, a cylinder or a slab of one constant",
                                  (long long)e, (long long)ids[(size_t)e], r0, kk, q[a]);
                    kk = q[a];
                }
            EMDEE_REQUIRE(kk > 0.0, EMDEE_ERR_INVALID, "set_restraints: entry %lld (atom %lld) is flat-bottomed (r0 = %g) with no non-zero "
                          "spring constant", (long long)e, (long long)ids[(size_t)e], r0);
        }
    }
    if (vsites) {
        std::vector<int32_t> taken;
        for (size_t s = 0; s + 3 < vsites->size(); s += 4) taken.push_back((*vsites)[s]);
        std::sort(taken.begin(), taken.end());
        for (int64_t e = 0; e < n; e++)
            EMDEE_REQUIRE(!std::binary_search(taken.begin(), taken.end(), (int32_t)ids[(size_t)e]), EMDEE_ERR_STATE, "set_restraints: atom %lld "
                          "of entry %lld is a virtual site of the table in force (emdee_md_set_vsites): a site is massless and follows its "
                          "parents, it cannot be restrained", (long long)ids[(size_t)e], (long long)e);
    }
    RestraintRows t;
    t.atoms.assign(ids.begin(), ids.end());
    t.ref = ref;
    t.k = k;
    t.flat = flat.empty() ? std::vector<double>((size_t)n, 0.0) : flat;
    return t;
}

// ---- the centre-of-mass pull (emdee_md_set_pull; pull.hpp): a per-atom group array, and per coordinate five integers {a, b, kind,
// geometry, mask} and six doubles {k or F, r0, rate, nx, ny, nz}
// The table as the kernels read it: the grouped ids in the table order of group_layout.hpp with the group of every entry, the chunks,
// the coordinates (the direction vectors normalised) and the starting references.
struct PullRows {
    std::vector<int32_t> ids, group_of;
    MsdLayout lay;
    PullCoord coord[PULL_MAX_COORDS] = {};
    double r0[PULL_MAX_COORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int n_groups = 0, n_coords = 0;
};
// The table as a caller gave it: n_groups and n_coords in 1 ... 8, every group id in -1 ... n_groups - 1, every group non-empty, every
// coordinate between two different groups of the table, a known kind and geometry, a mask in 1 ... 7 for the distance geometry, a
// finite non-zero vector for the direction geometry, finite parameters, k >= 0 for an umbrella, rate = 0 for a constant force, no
// grouped atom that is a site of the site table in force (`vsites`: its {site, a, b, c} ids; NULL: none in force); else refused, the
// text naming the entry and the offending value.
template <typename T>
PullRows pull_table(const std::vector<T> &group, int64_t n_groups, const std::vector<int32_t> &coords, const std::vector<double> &params,
                    int64_t n_coords, const std::vector<int32_t> *vsites = nullptr) {
    EMDEE_REQUIRE(n_groups >= 1 && n_groups <= PULL_MAX_GROUPS, EMDEE_ERR_INVALID, "set_pull: n_groups = %lld is outside 1...%d", (long long)n_groups,
                  PULL_MAX_GROUPS);
    EMDEE_REQUIRE(n_coords >= 1 && n_coords <= PULL_MAX_COORDS, EMDEE_ERR_INVALID, "set_pull: n_coords = %lld is outside 1...%d (0 clears the table)",
                  (long long)n_coords, PULL_MAX_COORDS);
    EMDEE_REQUIRE((int64_t)coords.size() == 5 * n_coords && (int64_t)params.size() == 6 * n_coords, EMDEE_ERR_INVALID, "set_pull: %lld coordinates "
                  "but %lld integers (five per coordinate) and %lld parameters (six per coordinate)", (long long)n_coords, (long long)coords.size(),
                  (long long)params.size());
    EMDEE_REQUIRE((int64_t)group.size() <= INT32_MAX, EMDEE_ERR_INVALID, "set_pull: %lld atoms (at most 2^31 - 1)", (long long)group.size());
    const int n = (int)group.size();
    std::vector<int> g32((size_t)n);
    for (int i = 0; i < n; i++) {
        const int64_t g = group[(size_t)i];
        EMDEE_REQUIRE(g >= -1 && g < n_groups, EMDEE_ERR_INVALID, "set_pull: atom %d has group %lld, outside -1...%lld", i, (long long)g,
                      (long long)n_groups - 1);
        g32[(size_t)i] = (int)g;
    }
    PullRows t;
    t.n_groups = (int)n_groups; t.n_coords = (int)n_coords;
    t.lay = msd_layout(g32.data(), n, (int)n_groups);
    for (int g = 0; g < (int)n_groups; g++)
        EMDEE_REQUIRE(t.lay.sizes[g] > 0, EMDEE_ERR_INVALID, "set_pull: group %d is empty (every group in use holds at least one atom)", g);
    for (int c = 0; c < (int)n_coords; c++) {
        const int32_t *q = coords.data() + 5 * (size_t)c;
        const double *p = params.data() + 6 * (size_t)c;
        EMDEE_REQUIRE(q[0] >= 0 && q[0] < n_groups && q[1] >= 0 && q[1] < n_groups, EMDEE_ERR_INVALID, "set_pull: coordinate %d names groups %d and "
                      "%d, outside 0...%lld", c, q[0], q[1], (long long)n_groups - 1);
        EMDEE_REQUIRE(q[0] != q[1], EMDEE_ERR_INVALID, "set_pull: coordinate %d names group %d twice (a coordinate lies between two different groups)",
                      c, q[0]);
        EMDEE_REQUIRE(q[2] == PULL_UMBRELLA || q[2] == PULL_CONSTANT_FORCE, EMDEE_ERR_INVALID, "set_pull: coordinate %d has the unknown kind %d "
                      "(EMDEE_PULL_UMBRELLA or EMDEE_PULL_CONSTANT_FORCE)", c, q[2]);
        EMDEE_REQUIRE(q[3] == PULL_DISTANCE || q[3] == PULL_DIRECTION, EMDEE_ERR_INVALID, "set_pull: coordinate %d has the unknown geometry %d "
                      "(EMDEE_PULL_DISTANCE or EMDEE_PULL_DIRECTION)", c, q[3]);
        for (int w = 0; w < 3; w++)
            EMDEE_REQUIRE(std::isfinite(p[w]), EMDEE_ERR_INVALID, "set_pull: coordinate %d has the parameter %s = %g, which is not finite", c,
                          w == 0 ? "k (or F)" : w == 1 ? "r0" : "rate", p[w]);
        EMDEE_REQUIRE(q[2] != PULL_UMBRELLA || p[0] >= 0.0, EMDEE_ERR_INVALID, "set_pull: coordinate %d is an umbrella with k = %g < 0", c, p[0]);
        EMDEE_REQUIRE(q[2] != PULL_CONSTANT_FORCE || p[2] == 0.0, EMDEE_ERR_INVALID, "set_pull: coordinate %d is a constant force with rate = %g "
                      "(a constant force has no reference to move: rate must be 0)", c, p[2]);
        PullCoord &pc = t.coord[c];
        pc.a = q[0]; pc.b = q[1]; pc.kind = q[2]; pc.geometry = q[3]; pc.mask = 0;
        pc.k = p[0]; pc.rate = p[2];
        pc.n[0] = pc.n[1] = pc.n[2] = 0.0;
        if (q[3] == PULL_DISTANCE) {
            EMDEE_REQUIRE(q[4] >= 1 && q[4] <= 7, EMDEE_ERR_INVALID, "set_pull: coordinate %d has the axis mask %d, outside 1...7 (bit a keeps axis a; "
                          "a distance needs at least one)", c, q[4]);
            pc.mask = q[4];
        } else {
            const double norm = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5]);
            EMDEE_REQUIRE(std::isfinite(norm) && norm > 0.0, EMDEE_ERR_INVALID, "set_pull: coordinate %d has the direction (%g, %g, %g), which is "
                          "zero or not finite", c, p[3], p[4], p[5]);
            for (int a = 0; a < 3; a++) pc.n[a] = p[3 + a] / norm;
        }
        t.r0[c] = p[1];
    }
    t.ids.assign((size_t)t.lay.n_grouped, 0);
    t.group_of.assign((size_t)t.lay.n_grouped, 0);
    for (int i = 0; i < n; i++)
        if (t.lay.pos_of[(size_t)i] >= 0) {
            t.ids[(size_t)t.lay.pos_of[(size_t)i]] = i;
            t.group_of[(size_t)t.lay.pos_of[(size_t)i]] = g32[(size_t)i];
        }
    if (vsites) {
        for (size_t s = 0; s + 3 < vsites->size(); s += 4) {
            const int32_t site = (*vsites)[s];
            EMDEE_REQUIRE(site < 0 || site >= n || g32[(size_t)site] < 0, EMDEE_ERR_STATE, "set_pull: atom %d of group %d is a virtual site of the "
                          "table in force (emdee_md_set_vsites): a site is massless, a centre of mass cannot hold it", site,
                          (site >= 0 && site < n) ? g32[(size_t)site] : -1);
        }
    }
    return t;
}

// ---- charges and the reaction-field constants
// want >= 0: the only n accepted (an undivided engine's atom count)
inline void check_coulomb(int64_t n, int64_t want, double K, double eps, double s14) {
    EMDEE_REQUIRE(want < 0 || n == want, EMDEE_ERR_INVALID, "set_coulomb: %lld charges for %lld atoms", (long long)n, (long long)want);
    EMDEE_REQUIRE(n < ((int64_t)1 << 31), EMDEE_ERR_INVALID, "set_coulomb: %lld charges (at most 2^31 - 1)", (long long)n);
    EMDEE_REQUIRE(std::isfinite(K) && K > 0.0, EMDEE_ERR_INVALID, "set_coulomb: the Coulomb constant must be finite and > 0");
    EMDEE_REQUIRE(eps >= 1.0, EMDEE_ERR_INVALID, "set_coulomb: the reaction-field dielectric must be >= 1 (+inf allowed)");
    EMDEE_REQUIRE(std::isfinite(s14) && s14 >= 0.0, EMDEE_ERR_INVALID, "set_coulomb: coulomb14scale must be finite and >= 0");
}
// the charges as given -> sqrt(K) q, what the kernels multiply pairwise; a charge that is not finite is refused
inline void scale_charges(std::vector<double> &q, double K) {
    const double sk = std::sqrt(K);
    for (size_t k = 0; k < q.size(); k++) {
        EMDEE_REQUIRE(std::isfinite(q[k]), EMDEE_ERR_INVALID, "set_coulomb: charge %lld is not finite", (long long)k);
        q[k] *= sk;
    }
}


// ---- Ewald summation (emdee_md_set_ewald): the argument checks, the wave vectors and their coefficients for a box
// alpha > 0 (alpha == 0 switches back to the reaction field and is not checked here); rc: the LJ model's cutoff
inline void check_ewald(double alpha, const int32_t *kmax, double rc) {
    EMDEE_REQUIRE(std::isfinite(alpha) && alpha > 0.0, EMDEE_ERR_INVALID, "set_ewald: alpha must be finite and >= 0");
    EMDEE_REQUIRE(kmax != nullptr, EMDEE_ERR_INVALID, "set_ewald: kmax is NULL");
    for (int d = 0; d < 3; d++)
        EMDEE_REQUIRE(kmax[d] >= 1 && kmax[d] <= 64, EMDEE_ERR_INVALID, "set_ewald: kmax[%d] = %d outside [1, 64]", d, kmax[d]);
    EMDEE_REQUIRE(alpha * rc >= 1.0, EMDEE_ERR_INVALID, "set_ewald: alpha rc = %g < 1 splits nothing off (erfc(alpha rc) = %g at the cutoff)",
                  alpha * rc, std::erfc(alpha * rc));
}
// The integer wave vectors n of the half space -- n_x > 0, or n_x = 0 and n_y > 0, or n_x = n_y = 0 and n_z > 0 -- with
// |n_d| <= kmax[d], as {n_x, n_y, n_z, ...} in ascending (n_x, n_y, n_z) order: each stands for itself and for -n.
inline std::vector<int32_t> ewald_vectors(const int32_t kmax[3]) {
    std::vector<int32_t> n;
    for (int32_t x = 0; x <= kmax[0]; x++)
        for (int32_t y = (x == 0 ? 0 : -kmax[1]); y <= kmax[1]; y++)
            for (int32_t z = ((x == 0 && y == 0) ? 1 : -kmax[2]); z <= kmax[2]; z++) { n.push_back(x); n.push_back(y); n.push_back(z); }
    return n;
}
// One wave vector as the reciprocal-space kernels read it (ewald.hpp): k = 2 pi n / L per axis,
// a = A(k) = (4 pi / V) exp(-k^2 / 4 alpha^2) / k^2,  b = 2 (1 / k^2 + 1 / (4 alpha^2)) (the tensor's factor).
struct EwaldK {
    double a, b, kx, ky, kz;
    int32_t nx, ny, nz, pad;
};
inline std::vector<EwaldK> ewald_table(const std::vector<int32_t> &n, const double len[3], double alpha) {
    std::vector<EwaldK> t(n.size() / 3);
    const double V = len[0] * len[1] * len[2], q4 = 1.0 / (4.0 * alpha * alpha);
    for (size_t v = 0; v < t.size(); v++) {
        EwaldK &e = t[v];
        e.nx = n[3 * v]; e.ny = n[3 * v + 1]; e.nz = n[3 * v + 2]; e.pad = 0;
        e.kx = 2.0 * M_PI * e.nx / len[0]; e.ky = 2.0 * M_PI * e.ny / len[1]; e.kz = 2.0 * M_PI * e.nz / len[2];
        const double k2 = e.kx * e.kx + e.ky * e.ky + e.kz * e.kz;
        e.a = (4.0 * M_PI / V) * std::exp(-k2 * q4) / k2;
        e.b = 2.0 * (1.0 / k2 + q4);
    }
    return t;
}
// ---- smooth particle-mesh Ewald (emdee_md_set_pme; pme.hpp): the argument checks, the spline moduli, the index folding, the
// FFT twiddles and the fixed-point scale of the charge mesh
// alpha > 0 (alpha == 0 switches back to the reaction field and is not checked here); rc: the LJ model's cutoff
inline void check_pme(double alpha, const int32_t *grid, int32_t order, double rc) {
    EMDEE_REQUIRE(std::isfinite(alpha) && alpha > 0.0, EMDEE_ERR_INVALID, "set_pme: alpha must be finite and >= 0");
    EMDEE_REQUIRE(grid != nullptr, EMDEE_ERR_INVALID, "set_pme: grid is NULL");
    for (int d = 0; d < 3; d++)
        EMDEE_REQUIRE(grid[d] >= 8 && grid[d] <= 256 && (grid[d] & (grid[d] - 1)) == 0, EMDEE_ERR_INVALID,
                      "set_pme: grid[%d] = %d is not a power of two in [8, 256]", d, grid[d]);
    EMDEE_REQUIRE(order == 4 || order == 6, EMDEE_ERR_INVALID, "set_pme: order = %d is neither 4 nor 6", order);
    EMDEE_REQUIRE(alpha * rc >= 1.0, EMDEE_ERR_INVALID, "set_pme: alpha rc = %g < 1 splits nothing off (erfc(alpha rc) = %g at the cutoff)",
                  alpha * rc, std::erfc(alpha * rc));
}
// the cardinal B-spline of order p at t + j, j = 0 .. p - 1, for 0 <= t < 1: w[j] = M_p(t + j); with dw, dw[j] = M_p'(t + j).
// M_n(x) = (x M_{n-1}(x) + (n - x) M_{n-1}(x - 1)) / (n - 1), M_2(x) = 1 - |x - 1| on [0, 2]; M_n' (x) = M_{n-1}(x) - M_{n-1}(x - 1).
// (pme.hpp pme_axis / pme_raise is this recursion on the device, on named scalars)
inline void pme_bspline(double t, int p, double *w, double *dw) {
    w[0] = t; w[1] = 1.0 - t;
    for (int j = 2; j < p; j++) w[j] = 0.0;
    for (int n = 3; n <= p; n++) {
        if (n == p && dw != nullptr) {
            dw[0] = w[0];
            for (int j = 1; j < p; j++) dw[j] = w[j] - w[j - 1];
        }
        for (int j = n - 1; j >= 1; j--) w[j] = ((t + j) * w[j] + (n - t - j) * w[j - 1]) / (n - 1);
        w[0] = t * w[0] / (n - 1);
    }
}
// cos(pi x) and sin(pi x) of x = num / den, exact in the octant: the argument of the library call is at most pi / 4
inline void pme_sincospi(int64_t num, int64_t den, double *s, double *c) {
    num %= 2 * den;
    if (num < 0) num += 2 * den;                             // x in [0, 2)
    const bool neg = num >= den;                             // sin(pi (x + 1)) = -sin(pi x), and cos alike
    if (neg) num -= den;
    const bool mirror = 2 * num > den;                       // x in (1/2, 1): sin(pi (1 - x)) = sin(pi x), cos changes sign
    if (mirror) num = den - num;
    double sv, cv;
    if (4 * num <= den) { sv = std::sin(M_PI * (double)num / (double)den); cv = std::cos(M_PI * (double)num / (double)den); }
    else { sv = std::cos(M_PI * (double)(den - 2 * num) / (double)(2 * den)); cv = std::sin(M_PI * (double)(den - 2 * num) / (double)(2 * den)); }
    if (mirror) cv = -cv;
    *s = neg ? -sv : sv;
    *c = neg ? -cv : cv;
}
// |b(m)|^2, m = 0 .. K - 1, of Essmann et al. eq. 4.4: 1 / |sum_{k=0}^{p-2} M_p(k + 1) exp(2 pi i m k / K)|^2.  Even orders have
// no zero of the sum at m = K / 2.
inline std::vector<double> pme_moduli(int K, int p) {
    double w[8];
    pme_bspline(0.0, p, w, nullptr);                         // w[j] = M_p(j): M_p(k + 1) = w[k + 1]
    std::vector<double> b((size_t)K);
    for (int m = 0; m < K; m++) {
        double re = 0.0, im = 0.0;
        for (int k = 0; k <= p - 2; k++) {
            double s, c;
            pme_sincospi(2 * (int64_t)m * k, K, &s, &c);
            re += w[k + 1] * c; im += w[k + 1] * s;
        }
        b[(size_t)m] = 1.0 / (re * re + im * im);
    }
    return b;
}
// the mesh index m of an axis of K points as the integer of its wave vector, in (-K/2, K/2]
inline int pme_fold(int m, int K) { return m <= K / 2 ? m : m - K; }
// exp(-2 pi i j / K), j = 0 .. K/2 - 1, as {re, im, ...}: the twiddles of the forward transform (the inverse conjugates them)
inline std::vector<double> pme_twiddles(int K) {
    std::vector<double> t((size_t)K);
    for (int j = 0; j < K / 2; j++) {
        double s, c;
        pme_sincospi(2 * (int64_t)j, K, &s, &c);
        t[2 * (size_t)j] = c; t[2 * (size_t)j + 1] = -s;
    }
    return t;
}
// The charge mesh is summed in 64-bit fixed point: a contribution q w (|w| <= 1) becomes the integer nearest to q w 2^shift.
// With sum |q_i| < 2^e (frexp) and shift = 61 - e no mesh point exceeds 2^61 + N / 2 < 2^63 in magnitude, whatever the
// configuration; the quantum 2^-shift = 2^(e - 61) is at most 2^-60 sum |q_i|.
inline int pme_fixed_shift(double sum_abs_q) {
    EMDEE_REQUIRE(std::isfinite(sum_abs_q) && sum_abs_q >= 0.0, EMDEE_ERR_INVALID, "pme: the sum of |q| is not finite");
    if (sum_abs_q == 0.0) return 0;
    int e;
    (void)std::frexp(sum_abs_q, &e);
    return std::min(61 - e, 1000);
}

// the error text for entry `entry` of the struck CSR (xs / xi of build_pairs) whose owner did not find the partner in its rows
inline std::string lost_pair_message(const std::vector<int32_t> &excl, const std::vector<int32_t> &p14, int64_t entry) {
    const PairCsrs t = build_pairs(excl, p14);
    int owner = 0;
    while (owner + 1 < t.rows && t.xs[(size_t)owner + 1] <= entry) owner++;
    const int partner = (entry >= 0 && entry < (int64_t)t.xi.size()) ? t.xi[(size_t)entry] : -1;
    char text[512];
    snprintf(text, sizeof(text), "Ewald: the excluded or 1-4 pair (%d, %d) is farther apart than rc + skin at a neighbour-list build, so its "
             "correction cannot be evaluated; replace the tables or the state", owner, partner);
    return text;
}

}  // namespace topo
}  // namespace emdee
