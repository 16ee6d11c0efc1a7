// msd_host.cpp -- the parts of the displacement and velocity correlations with no HIP in them, alone: csrc/msd.hpp (plain C++ there).
// Reads one case from stdin and prints lines of numbers.  tests/test_msd_host.py compiles this with the host compiler under ASan and
// UBSan and compares with numpy and a brute-force enumeration of its own.
//   chunk                                                     -> "MSD_CHUNK MSD_WORDS"
//   layout <n_groups> <n> <grouped: 0|1> then group x n       -> "n_grouped n_chunks", the sizes (8), chunk_of_group (9), pos_of (n),
//                                                                then one line "first count group" per chunk
//   schedule <n_lags> <origin_every> <s_end>                  -> per s = 0 .. s_end: "is_origin slot n_live", then "slot lag" x n_live
//   term <n> then 12 doubles x n (current entry, origin entry)-> per case the seven addends ("%.17g")
//   finish <n> then 7 doubles x n                             -> per case the seven words ("%.17g")
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../emdee.jl_amd/csrc/msd.hpp"

using namespace emdee;

static std::string token() {
    std::string t;
    if (!(std::cin >> t)) { fprintf(stderr, "msd_host: input ends early\n"); exit(2); }
    return t;
}
static long long integer() { return strtoll(token().c_str(), nullptr, 10); }
static double number() { return strtod(token().c_str(), nullptr); }

static void layout() {
    const int n_groups = (int)integer(), n = (int)integer(), grouped = (int)integer();
    std::vector<int> group((size_t)n);
    if (grouped)
        for (int i = 0; i < n; i++) group[(size_t)i] = (int)integer();
    const MsdLayout t = msd_layout(grouped ? group.data() : nullptr, n, n_groups);
    printf("%d %zu\n", t.n_grouped, t.chunks.size());
    for (int g = 0; g < MSD_MAX_GROUPS; g++) printf("%lld ", t.sizes[g]);
    printf("\n");
    for (int g = 0; g <= MSD_MAX_GROUPS; g++) printf("%d ", t.chunk_of_group[g]);
    printf("\n");
    for (int i = 0; i < n; i++) printf("%d ", t.pos_of[(size_t)i]);
    printf("\n");
    for (const MsdChunk &c : t.chunks) printf("%d %d %d\n", c.first, c.count, c.group);
}

static void schedule() {
    const int n_lags = (int)integer(), every = (int)integer();
    const long long s_end = integer();
    for (long long s = 0; s <= s_end; s++) {
        const MsdSchedule q = msd_schedule(s, n_lags, every);
        printf("%d %d %zu", q.is_origin ? 1 : 0, q.slot, q.live.size());
        if ((int)q.live.size() != msd_live_count(s, n_lags, every)) { fprintf(stderr, "msd_host: live count\n"); exit(3); }
        for (const MsdLive &l : q.live) printf(" %d %d", l.slot, l.lag);
        printf("\n");
    }
}

static void term() {
    const long long n = integer();
    for (long long k = 0; k < n; k++) {
        double c[6], o[6], out[MSD_WORDS];
        for (double &v : c) v = number();
        for (double &v : o) v = number();
        msd_term(c, o, out);
        for (double v : out) printf("%.17g ", v);
        printf("\n");
    }
}

static void finish() {
    const long long n = integer();
    for (long long k = 0; k < n; k++) {
        double total[MSD_WORDS], out[MSD_WORDS];
        for (double &v : total) v = number();
        msd_finish(total, out);
        for (double v : out) printf("%.17g ", v);
        printf("\n");
    }
}

int main() {
    const std::string what = token();
    if (what == "chunk") printf("%d %d\n", MSD_CHUNK, MSD_WORDS);
    else if (what == "layout") layout();
    else if (what == "schedule") schedule();
    else if (what == "term") term();
    else if (what == "finish") finish();
    else { fprintf(stderr, "msd_host: unknown case %s\n", what.c_str()); return 2; }
    return 0;
}
