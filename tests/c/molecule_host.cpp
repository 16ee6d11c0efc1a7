// molecule_host.cpp -- the host side of emdee_md_set_molecules, alone: the plain C++ of csrc/molecule.hpp (a centre of mass, one
// entry's share of the molecular sums and of the molecular scale) and the table builder of csrc/topology.hpp with its refusals and
// the mirror refusal of the constraint setters.  Reads one case from stdin and prints lines of numbers ("%.17g"), or "REFUSED <code>
// <message>" for a table the builder refuses.  tests/test_molecule_host.py compiles this with the host compiler under ASan and UBSan
// and compares with tests/helpers/molecule_ref.py.
//   words                                                      -> "<MOL_SMALL> <MOL_ACC> <MOL_CENTRE>"
//   table <n> {id} x n <lim> <nr> {apex a b} x nr <nh> {c s1 s2 s3} x nh
//                                                              -> "table <n_mol> <n_small>", then "start ...", "atoms ...", "entry_mol ...",
//                                                                 "mol_of ...", "label ...", "compact ...", "member ..."
//   mirror <rigid|hbonds> <n> {id} x n <ng> {group ids} x ng   -> "ok", or REFUSED: a candidate constraint table against the molecule ids
//   message <n> {id} x n <mol>                                 -> the text of a device check that names molecule <mol>
//   system <n> {id} x n {m rx ry rz kx ky kz vx vy vz fx fy fz} x n <len> x 3 <mu> x 3 <lo> x 3 <velocity_scale>
//                                                              -> "centres <n_mol>" and MOL_CENTRE words per molecule (table order), "sums" and
//                                                                 twelve words, "entries <n>" and "atom shift (3) dv (3)" per entry
//   triangle {y} x 9 {v} x 9 {f} x 9 <m_apex> <m_leg> <mu> x 3 <lo> x 3 <velocity_scale>
//                                                              -> settle.hpp's molecule_sums (12) and molecule_scale (shift 3, dv 3), then the
//                                                                 same eighteen words from the functions of molecule.hpp
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/molecule.hpp"
#include "../../emdee.jl_amd/csrc/settle.hpp"
#include "../../emdee.jl_amd/csrc/topology.hpp"

namespace emdee {
static char g_error[2048] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_error; }
}  // namespace emdee

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "molecule_host: input ends early\n"); exit(2); }
    return t;
}
static int64_t integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }

static std::vector<int64_t> ids_of(int64_t n) {
    std::vector<int64_t> v((size_t)(n > 0 ? n : 0));
    for (auto &g : v) g = integer();
    return v;
}
static std::vector<int32_t> ids32_of(int64_t n) {
    std::vector<int32_t> v((size_t)(n > 0 ? n : 0));
    for (auto &g : v) g = (int32_t)integer();
    return v;
}
static void line(const char *name, const std::vector<int32_t> &v) {
    printf("%s", name);
    for (int32_t g : v) printf(" %d", g);
    printf("\n");
}

static void table() {
    const std::vector<int64_t> raw = ids_of(integer());
    const int64_t lim = integer();
    const std::vector<int32_t> rigid = ids32_of(3 * integer()), hbonds = ids32_of(4 * integer());
    const topo::MoleculeRows t = topo::molecule_table(raw, lim, rigid.empty() ? nullptr : &rigid, hbonds.empty() ? nullptr : &hbonds);
    printf("table %d %d\n", t.n_mol, t.n_small);
    line("start", t.start); line("atoms", t.atoms); line("entry_mol", t.entry_mol); line("mol_of", t.mol_of); line("label", t.label);
    line("compact", t.compact);
    line("member", std::vector<int32_t>(t.member.begin(), t.member.end()));
}

// the centres of every molecule of t from unwrapped positions, as k_molecule_centres forms them: table order, first atom first
static std::vector<double> centres_of(const topo::MoleculeRows &t, const std::vector<double> &m, const std::vector<double> &x, const std::vector<double> &v) {
    std::vector<double> c((size_t)MOL_CENTRE * t.n_mol);
    for (int mol = 0; mol < t.n_mol; mol++) {
        const int first = t.start[(size_t)mol], end = t.start[(size_t)mol + 1];
        const size_t a1 = (size_t)t.atoms[(size_t)first];
        double acc[MOL_ACC] = {0, 0, 0, 0, 0, 0, 0};
        for (int e = first; e < end; e++) {
            const size_t a = (size_t)t.atoms[(size_t)e];
            molecule_centre_add(m[a], &x[3 * a], &v[3 * a], &x[3 * a1], &v[3 * a1], acc);
        }
        molecule_centre_finish(acc, &x[3 * a1], &v[3 * a1], &c[(size_t)MOL_CENTRE * mol]);
    }
    return c;
}

static void system_case() {
    const int64_t n = integer();
    const std::vector<int64_t> raw = ids_of(n);
    std::vector<double> m((size_t)n), r(3 * (size_t)n), k(3 * (size_t)n), v(3 * (size_t)n), f(3 * (size_t)n), x(3 * (size_t)n);
    for (size_t a = 0; a < (size_t)n; a++) {
        m[a] = number();
        for (int c = 0; c < 3; c++) r[3 * a + c] = number();
        for (int c = 0; c < 3; c++) k[3 * a + c] = number();
        for (int c = 0; c < 3; c++) v[3 * a + c] = number();
        for (int c = 0; c < 3; c++) f[3 * a + c] = number();
    }
    double len[3], mu[3], lo[3];
    for (auto &t : len) t = number();
    for (auto &t : mu) t = number();
    for (auto &t : lo) t = number();
    const double vscale = number();
    for (size_t a = 0; a < (size_t)n; a++)
        for (int c = 0; c < 3; c++) x[3 * a + c] = r[3 * a + c] + k[3 * a + c] * len[c];      // (restraint_unwrapped's sum)
    const topo::MoleculeRows t = topo::molecule_table(raw, n);
    const std::vector<double> cen = centres_of(t, m, x, v);
    printf("centres %d\n", t.n_mol);
    for (int mol = 0; mol < t.n_mol; mol++) {
        for (int w = 0; w < MOL_CENTRE; w++) printf("%.17g ", cen[(size_t)MOL_CENTRE * mol + w]);
        printf("\n");
    }
    double sums[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t e = 0; e < t.atoms.size(); e++) {
        const size_t a = (size_t)t.atoms[e];
        molecule_entry_sums(m[a], &x[3 * a], &v[3 * a], &f[3 * a], &cen[(size_t)MOL_CENTRE * t.entry_mol[e]], sums);
    }
    printf("sums\n");
    for (double s : sums) printf("%.17g ", s);
    printf("\nentries %zu\n", t.atoms.size());
    for (size_t e = 0; e < t.atoms.size(); e++) {
        const size_t a = (size_t)t.atoms[e];
        const double kl[3] = {k[3 * a] * len[0], k[3 * a + 1] * len[1], k[3 * a + 2] * len[2]};
        double shift[3], dv[3];
        molecule_entry_shift(&cen[(size_t)MOL_CENTRE * t.entry_mol[e]], kl, mu, lo, vscale, shift, dv);
        printf("%zu %.17g %.17g %.17g %.17g %.17g %.17g\n", a, shift[0], shift[1], shift[2], dv[0], dv[1], dv[2]);
    }
}

static void triangle() {
    double y[3][3], v[3][3], f[3][3], mu[3], lo[3];
    for (auto &s : y) for (auto &c : s) c = number();
    for (auto &s : v) for (auto &c : s) c = number();
    for (auto &s : f) for (auto &c : s) c = number();
    const double m_apex = number(), m_leg = number();
    for (auto &t : mu) t = number();
    for (auto &t : lo) t = number();
    const double vscale = number();
    double out[12], shift[3], dv[3];
    molecule_sums(y, v, f, m_apex, m_leg, out);
    molecule_scale(y, v, m_apex, m_leg, mu, lo, vscale, shift, dv);
    for (double s : out) printf("%.17g ", s);
    for (double s : shift) printf("%.17g ", s);
    for (double s : dv) printf("%.17g ", s);
    printf("\n");
    const double m[3] = {m_apex, m_leg, m_leg}, zero[3] = {0.0, 0.0, 0.0};
    double acc[MOL_ACC] = {0, 0, 0, 0, 0, 0, 0}, cen[MOL_CENTRE], sums[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < 3; s++) molecule_centre_add(m[s], y[s], v[s], y[0], v[0], acc);
    molecule_centre_finish(acc, y[0], v[0], cen);
    for (int s = 0; s < 3; s++) molecule_entry_sums(m[s], y[s], v[s], f[s], cen, sums);
    molecule_entry_shift(cen, zero, mu, lo, vscale, shift, dv);
    for (double s : sums) printf("%.17g ", s);
    for (double s : shift) printf("%.17g ", s);
    for (double s : dv) printf("%.17g ", s);
    printf("\n");
}

int main() {
    const std::string what = token();
    try {
        if (what == "words") {
            printf("%d %d %d\n", MOL_SMALL, MOL_ACC, MOL_CENTRE);
        } else if (what == "table") {
            table();
        } else if (what == "mirror") {
            const bool rigid = token() == "rigid";
            const std::vector<int32_t> mol = ids32_of(integer());
            const int sites = rigid ? 3 : 4;
            const std::vector<int32_t> groups = ids32_of(sites * integer());
            topo::refuse_split_groups(rigid ? "set_rigid3" : "set_hbonds", rigid ? "rigid molecule" : "hbonds cluster", "this call", sites, groups, mol);
            printf("ok\n");
        } else if (what == "message") {
            const std::vector<int64_t> raw = ids_of(integer());
            const topo::MoleculeRows t = topo::molecule_table(raw, (int64_t)raw.size());
            printf("%s\n", topo::molecule_message(t, integer(), "its total mass is 0").c_str());
        } else if (what == "system") {
            system_case();
        } else if (what == "triangle") {
            triangle();
        } else {
            fprintf(stderr, "molecule_host: unknown case %s\n", what.c_str());
            return 2;
        }
    } catch (const Failure &f) {
        printf("REFUSED %d %s\n", f.code, get_error());
    }
    return 0;
}
