// rdf_host.cpp -- the parts of the radial distribution functions with no HIP in them, alone: csrc/rdf.hpp (plain C++ there).  Reads
// one case from stdin and prints lines of numbers.  tests/test_rdf_host.py compiles this with the host compiler under ASan and
// UBSan and compares with tests/helpers/rdf_ref.py.
//   slots <n_groups>                                          -> one line per a: slot(a, b) for b = 0 .. n_groups - 1
//   bins <r_max> <n_bins> <n> then r2 x n                     -> "bin" per r2 (inv_dr = n_bins / r_max)
//   plan <lx> <ly> <lz> <r_max> <n_atoms>                     -> "Mx My Mz nd wrapx wrapy wrapz"
//   visits <lx> <ly> <lz> <r_max> <n_atoms>                   -> per home cell: the ids of the cells it visits, in the kernel's order
//   runs <M> <nd> <wrap>                                      -> per home coordinate of an x axis: "nseg xa0 xa1 xb0 xb1", then the
//                                                                cells rdf_axis_cell gives
//   pairs <lx> <ly> <lz> <r_max> <n_bins> <n_groups> <n> then per atom: x y z group mol
//                                                             -> n_pairs lines of n_bins counts: the pair loop the planner drives
//   normalise <n_groups> <n_bins> <r_max> <frames> <inv_volume_sum> then sizes x n_groups, counts x n_pairs n_bins
//                                                             -> n_pairs lines of g, then n_pairs lines of coordination ("%.17g")
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/rdf.hpp"

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "rdf_host: input ends early\n"); exit(2); }
    return t;
}
static long long integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }

static void slots() {
    const int n = (int)integer();
    for (int a = 0; a < n; a++) {
        for (int b = 0; b < n; b++) printf("%d ", rdf_pair_slot(a, b, n));
        printf("\n");
    }
}

static void bins() {
    const double r_max = number();
    const int n_bins = (int)integer();
    const long long n = integer();
    const double inv_dr = (double)n_bins / r_max;
    for (long long k = 0; k < n; k++) printf("%d\n", rdf_bin(number(), inv_dr, n_bins));
}

static RdfPlan read_plan(double len[3], double &r_max) {
    for (int d = 0; d < 3; d++) len[d] = number();
    r_max = number();
    const long long n_atoms = integer();
    return rdf_plan(len, r_max, n_atoms);
}

static void plan() {
    double len[3], r_max;
    const RdfPlan p = read_plan(len, r_max);
    printf("%d %d %d %d %d %d %d\n", p.M[0], p.M[1], p.M[2], p.nd, p.wrap[0], p.wrap[1], p.wrap[2]);
}

// the cells a home cell visits, as k_rdf_pairs walks them: z, then y by rdf_axis_cell, then the one or two runs of cells of the
// row along x that rdf_row_runs gives (the kernel turns each run into one range of the compact array)
static std::vector<int> visited(const RdfPlan &p, int c) {
    const int cx = c % p.M[0], cy = (c / p.M[0]) % p.M[1], cz = c / (p.M[0] * p.M[1]);
    int xa0, xa1, xb0, xb1;
    const int nseg = rdf_row_runs(p.M[0], p.nd, p.wrap[0], cx, xa0, xa1, xb0, xb1);
    std::vector<int> out;
    for (int kz = 0; kz < rdf_axis_count(p.M[2], p.nd, p.wrap[2]); kz++)
        for (int ky = 0; ky < rdf_axis_count(p.M[1], p.nd, p.wrap[1]); ky++) {
            const int row = (rdf_axis_cell(p.M[2], p.nd, p.wrap[2], cz, kz) * p.M[1] + rdf_axis_cell(p.M[1], p.nd, p.wrap[1], cy, ky)) * p.M[0];
            for (int q = 0; q < nseg; q++)
                for (int x2 = (q ? xb0 : xa0); x2 <= (q ? xb1 : xa1); x2++) out.push_back(row + x2);
        }
    return out;
}

// the runs of every home coordinate of an x axis of M cells, next to the cells rdf_axis_cell names
static void runs() {
    const int M = (int)integer(), nd = (int)integer(), wrap = (int)integer();
    for (int cx = 0; cx < M; cx++) {
        int xa0, xa1, xb0, xb1;
        const int nseg = rdf_row_runs(M, nd, wrap, cx, xa0, xa1, xb0, xb1);
        printf("%d %d %d %d %d", nseg, xa0, xa1, xb0, xb1);
        for (int k = 0; k < rdf_axis_count(M, nd, wrap); k++) printf(" %d", rdf_axis_cell(M, nd, wrap, cx, k));
        printf("\n");
    }
}

static void visits() {
    double len[3], r_max;
    const RdfPlan p = read_plan(len, r_max);
    for (int c = 0; c < (int)rdf_plan_cells(p); c++) {
        for (int v : visited(p, c)) printf("%d ", v);
        printf("\n");
    }
}

static void pairs() {
    double len[3];
    for (int d = 0; d < 3; d++) len[d] = number();
    const double r_max = number();
    const int n_bins = (int)integer(), n_groups = (int)integer(), n = (int)integer();
    std::vector<double> x((size_t)3 * n);
    std::vector<int> grp((size_t)n), mol((size_t)n), cell((size_t)n);
    const RdfPlan p = rdf_plan(len, r_max, n);
    for (int i = 0; i < n; i++) {
        for (int d = 0; d < 3; d++) x[3 * (size_t)i + d] = number();
        grp[i] = (int)integer();
        mol[i] = (int)integer();
        cell[i] = rdf_axis_cell_of(x[3 * (size_t)i], 0.0, len[0], p.M[0]) +
                  p.M[0] * (rdf_axis_cell_of(x[3 * (size_t)i + 1], 0.0, len[1], p.M[1]) + p.M[1] * rdf_axis_cell_of(x[3 * (size_t)i + 2], 0.0, len[2], p.M[2]));
    }
    // the compact array: grouped atoms in cell order
    std::vector<std::vector<int>> members((size_t)rdf_plan_cells(p));
    std::vector<int> slot((size_t)n, -1);
    int next = 0;
    for (int i = 0; i < n; i++)
        if (grp[i] >= 0) members[cell[i]].push_back(i);
    for (auto &m : members)
        for (int i : m) slot[i] = next++;
    const double inv_dr = (double)n_bins / r_max, r2_cut = r_max * r_max * RDF_R2_MARGIN;
    std::vector<long long> counts((size_t)rdf_n_pairs(n_groups) * n_bins, 0);
    for (int c = 0; c < (int)members.size(); c++)
        for (int c2 : visited(p, c))
            for (int i : members[c])
                for (int j : members[c2]) {
                    if (slot[j] <= slot[i]) continue;
                    if (mol[i] >= 0 && mol[i] == mol[j]) continue;
                    double r2 = 0.0;
                    for (int d = 0; d < 3; d++) {
                        double t = x[3 * (size_t)j + d] - x[3 * (size_t)i + d];
                        t -= len[d] * rint(t * (1.0 / len[d]));
                        r2 += t * t;
                    }
                    if (!(r2 <= r2_cut)) continue;
                    const int b = rdf_bin(r2, inv_dr, n_bins);
                    if (b >= 0) counts[(size_t)rdf_pair_slot(grp[i], grp[j], n_groups) * n_bins + b]++;
                }
    for (int s = 0; s < rdf_n_pairs(n_groups); s++) {
        for (int b = 0; b < n_bins; b++) printf("%lld ", counts[(size_t)s * n_bins + b]);
        printf("\n");
    }
}

static void normalise() {
    const int n_groups = (int)integer(), n_bins = (int)integer();
    const double r_max = number();
    const long long frames = integer();
    const double inv_volume_sum = number();
    long long sizes[RDF_MAX_GROUPS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n_groups < 1 || n_groups > RDF_MAX_GROUPS) { fprintf(stderr, "rdf_host: n_groups\n"); exit(2); }
    for (int a = 0; a < n_groups; a++) sizes[a] = integer();
    const size_t m = (size_t)rdf_n_pairs(n_groups) * n_bins;
    std::vector<long long> counts(m);
    for (auto &c : counts) c = integer();
    std::vector<double> g(m), cn(m);
    rdf_normalise(counts.data(), n_groups, n_bins, r_max, sizes, frames, inv_volume_sum, g.data(), cn.data());
    for (const auto *v : {&g, &cn})
        for (int s = 0; s < rdf_n_pairs(n_groups); s++) {
            for (int b = 0; b < n_bins; b++) printf("%.17g ", (*v)[(size_t)s * n_bins + b]);
            printf("\n");
        }
}

int main() {
    const std::string what = token();
    if (what == "slots") slots();
    else if (what == "bins") bins();
    else if (what == "plan") plan();
    else if (what == "visits") visits();
    else if (what == "runs") runs();
    else if (what == "pairs") pairs();
    else if (what == "normalise") normalise();
    else { fprintf(stderr, "rdf_host: unknown case %s\n", what.c_str()); return 2; }
    return 0;
}
