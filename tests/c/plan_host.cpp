// Stand-alone host program over emdee.jl_amd/csrc/plan.hpp (tests/test_plan_host.py builds it with g++ under ASan and UBSan):
// no GPU, no HIP header.  One command per line on stdin.
//   facts  := rb M0 M1 M2 per0 per1 per2 len0 len1 len2 rlist n n_plan nt nsub uniform charged ewald filters_rows brick_path
//             in_edit stride typed_stride field16_blocked typed_blocked typed_all typed_bricks7 debug
//   maxima := tile own span (bricks of 4 x 2 x 2 cells)  tile own span (2 x 2 x 2)  typed_span (4 x 2 x 2)  typed_span (2 x 2 x 2)
//   sizes rb variant tile_cap own_cap stride nsub -> the LDS bytes and constants of the variant, one line
//   plan facts maxima            -> "plan" + the fields of the plan, its lines prefixed with "| ", "."
//   kept facts maxima facts      -> plan_kept(choose_plan(first facts), second facts)
//   after facts maxima needed    -> the plan after after_build, and block_typed
//   sweep + four lines of lists (tiles, own divisors, spans, strides) -> one int32 record per combination, binary
#include <cstdint>
#include <iostream>
#include <sstream>
#include <vector>

#include "../../emdee.jl_amd/csrc/plan.hpp"

using namespace emdee;

struct Populations {
    int pop[2][3], span[2];
    int asked[2] = {0, 0};
    template <class S>
    std::array<int, 3> maxima(S) {
        const int k = S::NOC == 8 ? 1 : 0;
        asked[k]++;
        return {pop[k][0], pop[k][1], pop[k][2]};
    }
    template <class S>
    int typed_span(S) { return span[S::NOC == 8 ? 1 : 0]; }
};

static PlanFacts read_facts(std::istream &in) {
    PlanFacts f;
    in >> f.real_bytes >> f.M[0] >> f.M[1] >> f.M[2] >> f.per[0] >> f.per[1] >> f.per[2] >> f.len[0] >> f.len[1] >> f.len[2] >> f.rlist >> f.n >>
        f.n_plan >> f.nt >> f.nsub >> f.uniform >> f.charged >> f.ewald >> f.filters_rows >> f.brick_path >> f.in_edit >> f.stride >>
        f.typed_stride >> f.field16_blocked >> f.typed_blocked >> f.typed_all >> f.typed_bricks7 >> f.debug;
    return f;
}
static Populations read_populations(std::istream &in) {
    Populations m;
    for (int k = 0; k < 2; k++)
        for (int q = 0; q < 3; q++) in >> m.pop[k][q];
    in >> m.span[0] >> m.span[1];
    return m;
}
static void print_plan(const BrickPlan &p, const Populations &m) {
    const int k = p.variant == 9 ? 1 : 0;
    std::cout << "plan " << p.active << ' ' << p.typed << ' ' << p.reason << ' ' << p.variant << ' ' << p.tile_cap << ' ' << p.own_cap << ' '
              << p.row_block << ' ' << p.stride << ' ' << p.typed_stride << ' ' << p.build_alg << ' ' << p.span3_limit << ' ' << p.idx_shift << ' '
              << p.lds_force << ' ' << p.lds_build << ' ' << plan_holds(p, m.pop[k]) << ' ' << p.grid.nb[0] << ' ' << p.grid.nb[1] << ' '
              << p.grid.nb[2] << ' ' << p.n << ' ' << m.asked[0] << ' ' << m.asked[1] << ' ' << p.build_margin << '\n';
}

static void sizes(std::istream &in) {
    int rb, variant, tile_cap, own_cap, stride, nsub;
    in >> rb >> variant >> tile_cap >> own_cap >> stride >> nsub;
    with_brick_variant(variant, [&](auto v) {
        using V = decltype(v);
        using S = typename V::Shape;
        auto line = [&](auto r) {
            using real = decltype(r);
            std::cout << brick_force_lds_bytes<real, S, V::THREADS>(tile_cap, own_cap, false) << ' '
                      << brick_force_lds_bytes<real, S, V::THREADS>(tile_cap, own_cap, true) << ' '
                      << brick_force_lds_bytes_soa<real, S, V::THREADS>(own_cap) << ' '
                      << brick_build_lds_bytes<S, V::THREADS>(tile_cap, own_cap, stride, V::GB, nsub) << ' '
                      << typed_force_lds_bytes<real, S, V::THREADS>(own_cap) << ' '
                      << typed_build_lds_bytes<S, V::THREADS>(tile_cap, own_cap, stride, V::GB, V::G) << ' ' << typed_slots<S, V::THREADS>() << ' '
                      << brick_min_stride(V::G, V::THREADS) << ' ' << typed_min_stride<V>() << ' ' << EPL * V::G << ' ' << V::GB << ' '
                      << V::THREADS << '\n';
        };
        if (rb == 8) line(double{});
        else line(float{});
    });
}

// every combination of the flags with every entry of the four lists; the 2 x 2 x 2 bricks see two thirds of the tile (64 of 96
// cells), half the own atoms (8 of 16 cells) and the same span, a species half of the span
static void sweep(std::istream &in) {
    std::vector<int> lists[4];
    for (auto &l : lists) {
        std::string line;
        std::getline(in, line);
        std::istringstream ls(line);
        for (int t; ls >> t;) l.push_back(t);
    }
    std::vector<int32_t> out;
    std::string text;
    // mode 0: every flag; 1: an engine on the direct path; 2: a state without atoms (both precisions)
    for (int mode = 0; mode < 3; mode++)
    for (int bits = 0; bits < (mode == 0 ? 1 << 9 : 2); bits++)
        for (int nt = 1; nt <= (mode == 0 ? 3 : 1); nt++) {
            PlanFacts f;
            f.brick_path = mode != 1;
            f.real_bytes = (bits & 1) ? 8 : 4;
            f.uniform = bits & 2; f.charged = bits & 4; f.ewald = bits & 8; f.filters_rows = bits & 16;
            f.field16_blocked = bits & 32; f.typed_blocked = bits & 64; f.typed_all = bits & 128; f.typed_bricks7 = bits & 256;
            if (f.ewald && !f.charged) continue;                 // (an Ewald engine is a charged one)
            f.nt = nt; f.nsub = nt == 1 ? 4 : 1;
            for (int d = 0; d < 3; d++) { f.M[d] = 13; f.len[d] = 13 * 3.9; }
            f.rlist = 3.8; f.n = f.n_plan = mode == 2 ? 0 : 100000;
            for (int tile : lists[0])
                for (int div : lists[1])
                    for (int span : lists[2])
                        for (int stride : lists[3]) {
                            Populations m;
                            const int own = std::max(1, tile / div);
                            m.pop[0][0] = tile; m.pop[0][1] = own; m.pop[0][2] = span;
                            m.pop[1][0] = std::max(1, tile * 2 / 3); m.pop[1][1] = std::max(1, own / 2); m.pop[1][2] = span;
                            m.span[0] = m.span[1] = (span + 1) / 2;
                            f.stride = stride;
                            const BrickPlan p = choose_plan(f, m, text);
                            const int k = p.variant == 9 ? 1 : 0;
                            const int32_t rec[] = {f.real_bytes, nt, f.uniform, f.charged, f.ewald, f.filters_rows, f.field16_blocked, f.typed_blocked,
                                                   f.typed_all, f.typed_bricks7, tile, own, span, stride, m.pop[k][0], m.pop[k][1], m.span[k],
                                                   p.active, p.typed, p.reason, p.variant, p.tile_cap, p.own_cap, p.row_block, p.stride, p.build_alg,
                                                   p.span3_limit, p.idx_shift, (int32_t)p.lds_force, (int32_t)p.lds_build, plan_holds(p, m.pop[k]),
                                                   p.typed_stride};
                            out.insert(out.end(), std::begin(rec), std::end(rec));
                        }
        }
    std::cout.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * sizeof(int32_t)));
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "sizes") sizes(std::cin);
        else if (cmd == "plan" || cmd == "kept" || cmd == "after") {
            const PlanFacts f = read_facts(std::cin);
            Populations m = read_populations(std::cin);
            std::string text;
            BrickPlan p = choose_plan(f, m, text);
            if (cmd == "kept") {
                std::cout << "kept " << plan_kept(p, read_facts(std::cin)) << '\n';
                continue;
            }
            bool block_typed = false;
            if (cmd == "after") {
                int needed;
                std::cin >> needed;
                p = after_build(p, f.nsub, needed, block_typed);
            }
            print_plan(p, m);
            std::istringstream lines(text);
            for (std::string l; std::getline(lines, l);) std::cout << "| " << l << '\n';
            if (cmd == "after") std::cout << "block_typed " << block_typed << '\n';
            std::cout << ".\n";
        } else if (cmd == "sweep") {
            std::string rest;
            std::getline(std::cin, rest);
            sweep(std::cin);
        } else {
            std::cerr << "plan_host: unknown command " << cmd << '\n';
            return 2;
        }
    }
    return 0;
}
