// spatial_host.cpp -- the parts of the spatial profiles with no HIP in them, alone: csrc/spatial.hpp (plain C++ there).
// Reads one case from stdin and prints lines of numbers.  tests/test_spatial_host.py compiles this with the host compiler under ASan
// and UBSan and compares with numpy and a brute-force enumeration of its own.
//   consts                                                    -> "SPATIAL_CHUNK SPATIAL_WORDS SPATIAL_MAX_BINS"
//   layout <n_groups> <n> <grouped: 0|1> then group x n       -> as msd_host's: "n_grouped n_chunks", the sizes (8), chunk_of_group
//                                                                (9), pos_of (n), then one line "first count group" per chunk
//   words <what>                                              -> the words behind the compact indices of that mask
//   planar <n> <lo> <inv_width> <n_bins> <periodic> then x x n -> the bins
//   radial <n> <centre x 3> <len x 3 (0: open)> <r_max> <n_bins> then xyz x n -> per atom "bin r d0 d1 d2" (r and d as "%a")
//   addends <what> <n> then per case m q v[3] e w[6] n[3] no_normal -> per case the ten words ("%.17g")
//   reduce <nw: 2|3|10> <n_groups> <n_bins> <n> <grouped> then group x n (if grouped), then per atom in caller order its bin and nw
//          words                                              -> the counts (n_groups x n_bins), the outside counts (n_groups), then
//                                                                per (group, bin) the nw sums ("%a": every bit)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/spatial.hpp"

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "spatial_host: input ends early\n"); exit(2); }
    return t;
}
static long long integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }

static MsdLayout read_layout(int n_groups, int n, int grouped, std::vector<int> &group) {
    group.assign((size_t)n, 0);
    if (grouped)
        for (int i = 0; i < n; i++) group[(size_t)i] = (int)integer();
    return msd_layout(grouped ? group.data() : nullptr, n, n_groups);
}

static void layout() {
    const int n_groups = (int)integer(), n = (int)integer(), grouped = (int)integer();
    std::vector<int> group;
    const MsdLayout t = read_layout(n_groups, n, grouped, group);
    printf("%d %zu\n", t.n_grouped, t.chunks.size());
    for (int g = 0; g < SPATIAL_MAX_GROUPS; g++) printf("%lld ", t.sizes[g]);
    printf("\n");
    for (int g = 0; g <= SPATIAL_MAX_GROUPS; g++) printf("%d ", t.chunk_of_group[g]);
    printf("\n");
    for (int i = 0; i < n; i++) printf("%d ", t.pos_of[(size_t)i]);
    printf("\n");
    for (const MsdChunk &c : t.chunks) printf("%d %d %d\n", c.first, c.count, c.group);
}

static void planar() {
    const long long n = integer();
    const double lo = number(), inv_width = number();
    const int n_bins = (int)integer(), periodic = (int)integer();
    for (long long i = 0; i < n; i++) printf("%d\n", spatial_bin_planar(number(), lo, inv_width, n_bins, periodic));
}

static void radial() {
    const long long n = integer();
    double c[3], len[3], inv_len[3];
    for (double &v : c) v = number();
    for (int a = 0; a < 3; a++) { len[a] = number(); inv_len[a] = len[a] != 0.0 ? 1.0 / len[a] : 0.0; }
    const double r_max = number();
    const int n_bins = (int)integer();
    const double inv_dr = (double)n_bins / r_max;
    for (long long i = 0; i < n; i++) {
        double d[3], r;
        for (int a = 0; a < 3; a++) d[a] = spatial_image(number(), c[a], len[a], inv_len[a]);
        const int bin = spatial_bin_radial(d, r_max, inv_dr, n_bins, r);
        printf("%d %a %a %a %a\n", bin, r, d[0], d[1], d[2]);
    }
}

static void addends() {
    const int what = (int)integer();
    const long long n = integer();
    for (long long k = 0; k < n; k++) {
        double v[3], w[6], nn[3], out[SPATIAL_WORDS];
        const double m = number(), q = number();
        for (double &t : v) t = number();
        const double e = number();
        for (double &t : w) t = number();
        for (double &t : nn) t = number();
        const bool no_normal = integer() != 0;
        spatial_addends(what, m, q, v, e, w, nn, no_normal, out);
        for (double t : out) printf("%.17g ", t);
        printf("\n");
    }
}

template <int NW>
static void reduce_case(int n_groups, int n_bins, int n, int grouped) {
    std::vector<int> group;
    const MsdLayout lay = read_layout(n_groups, n, grouped, group);
    const size_t ng = (size_t)lay.n_grouped;
    std::vector<int> bin(ng + 1, 0);
    std::vector<double> planes(ng * NW + 1, 0.0);
    for (int i = 0; i < n; i++) {
        const int b = (int)integer();
        double w[NW];
        for (double &t : w) t = number();
        const int e = lay.pos_of[(size_t)i];
        if (e < 0) continue;
        bin[(size_t)e] = b;
        for (int j = 0; j < NW; j++) planes[(size_t)j * ng + e] = w[j];
    }
    const size_t cells = (size_t)n_groups * n_bins;
    std::vector<double> sums(cells * NW, 0.0);
    std::vector<long long> counts(cells, 0), outside((size_t)n_groups, 0);
    spatial_reduce_host<NW>(lay, n_groups, n_bins, bin.data(), planes.data(), sums.data(), counts.data(), outside.data());
    for (size_t c = 0; c < cells; c++) printf("%lld ", counts[c]);
    printf("\n");
    for (int g = 0; g < n_groups; g++) printf("%lld ", outside[(size_t)g]);
    printf("\n");
    for (size_t c = 0; c < cells; c++) {
        for (int j = 0; j < NW; j++) printf("%a ", sums[c * NW + j]);
        printf("\n");
    }
}

int main() {
    const std::string what = token();
    if (what == "consts") printf("%d %d %d\n", SPATIAL_CHUNK, SPATIAL_WORDS, SPATIAL_MAX_BINS);
    else if (what == "layout") layout();
    else if (what == "words") {
        const int mask = (int)integer();
        for (int j = 0; j < spatial_n_words(mask); j++) printf("%d ", spatial_word_of(mask, j));
        printf("\n");
    } else if (what == "planar") planar();
    else if (what == "radial") radial();
    else if (what == "addends") addends();
    else if (what == "reduce") {
        const int nw = (int)integer(), n_groups = (int)integer(), n_bins = (int)integer(), n = (int)integer(), grouped = (int)integer();
        if (nw == 2) reduce_case<2>(n_groups, n_bins, n, grouped);
        else if (nw == 3) reduce_case<3>(n_groups, n_bins, n, grouped);
        else if (nw == 10) reduce_case<10>(n_groups, n_bins, n, grouped);
        else { fprintf(stderr, "spatial_host: nw = %d\n", nw); return 2; }
    } else { fprintf(stderr, "spatial_host: unknown case %s\n", what.c_str()); return 2; }
    return 0;
}
