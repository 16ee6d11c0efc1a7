// plan.hpp -- which kernels a state runs on, as a value: facts in, plan out.  Plain C++17 (no HIP header: tests/c/plan_host.cpp
// compiles it with g++), shared by the kernels (the shapes and LDS sizes below are theirs) and by NbSystem, which asks
// choose_plan once per load and keeps the BrickPlan it returns until the populations outgrow it.
//
// Contract with the kernels (tests/test_plan_host.py sweeps it): an active plan has tile_cap >= largest tile + 1 (the sentinel)
// and < 65536, own_cap >= most own atoms, both kernels within LDS_LIMIT, a stride of whole lane-major blocks that holds the
// prefetched blocks, idx_shift != 0 only where the tile fits the coordinate planes, and a build kernel whose hit fields hold
// the widest three-cell span.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>

#ifdef __HIPCC__
#define EMDEE_PLAN_HD __host__ __device__
#else
#define EMDEE_PLAN_HD
#endif

namespace emdee {

constexpr int WAVE = 64;
constexpr int NXCD = 8;
constexpr int EPL = 8;   // neighbour entries per lane per 16-byte load
constexpr int BUILD2_FIELD = 16;                      // bits per tile row in a lane's bit field (two-phase build, brick.hpp)
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int TNT = 2;   // species of a typed box

// bytes of one tile record (kernels.hpp Rec<real>; brick.hpp asserts the tie)
template <typename real>
constexpr size_t rec_bytes() { return sizeof(real) == 8 ? 32 : 16; }

// entries the force kernels read of every row without looking at its length: the NPF prefetched blocks of 8 G entries
// and the one after them (rows are sentinel-padded, so the row stride must hold them)
// (1024-thread workgroups with 4 lanes per atom are the long-row variant -- rc = 3.5 sigma: 184 entries -- and prefetch five
// 32-entry blocks: with two, every further block of a row is a dependent global load that four wavefronts per SIMD cannot hide)
constexpr int brick_prefetch_blocks(int G, int THREADS) { return (EPL * G) >= 128 ? 1 : ((G == 4 && THREADS >= 1024) ? 5 : 2); }
constexpr int brick_min_stride(int G, int THREADS) { return (brick_prefetch_blocks(G, THREADS) + 1) * EPL * G; }

template <int BX_, int BY_, int BZ_>
struct BrickShape {
    static constexpr int BX = BX_, BY = BY_, BZ = BZ_;
    static constexpr int TX = BX + 2, TY = BY + 2, TZ = BZ + 2;
    static constexpr int NTC = TX * TY * TZ;   // tile cells
    static constexpr int NOC = BX * BY * BZ;   // own cells
};

struct BrickGrid {
    int nb[3];         // bricks per dimension
    int nbricks;
    int per_xcd;       // ceil(nbricks / 8): XCD-contiguous remap of block ids
    // interior sub-box (bricks whose tile holds no ghost cell): phase-1 launches enumerate only these,
    // so that every XCD gets an equal share of them
    int ib_lo[3], ib_n[3];
    int ib_count, ib_per_xcd;
    // boundary bricks = the rest, enumerated densely as z-slabs, then y-slabs, then x-slabs (phase 2)
    int bb_z, bb_y, bb_count, bb_per_xcd;   // bb_z = #bricks in the z-slabs, bb_y = # in the y-slabs
};

// ---- sizes of the LDS tables shared by the build and force kernels (brick.hpp BrickTables carves them) ----
// NT = species the tables tell apart: 1 (brick.hpp, atoms of a cell in any order) or TNT (typed.hpp, species-major blocks)
template <class Shape, int THREADS, int NT = 1>
struct BrickTableSizes {
    static constexpr int NTC = Shape::NTC, NOC = Shape::NOC, NTT = NT * NTC, NOT = NT * NOC, NWAVES = THREADS / WAVE;
    static constexpr int own_words = NT == 1 ? 2 : 3;   // per own atom: oinfo (and the two segment lengths of a typed row)
    EMDEE_PLAN_HD static constexpr size_t fixed_ints() { return (NTT + 4) + NTT + NTC + (NOT + 4) + ((NWAVES + 1) & ~1); }
    EMDEE_PLAN_HD static size_t bytes(int own_cap) { return ((fixed_ints() + own_words * (size_t)own_cap) * 4 + 15) & ~(size_t)15; }
    // off | gbeg | shift | own are contiguous: that image (+ tile_n, n_own) is what k_brick_tables stores per brick
    EMDEE_PLAN_HD static constexpr int image_ints() { return (NTT + 4) + NTT + NTC + (NOT + 4); }
    EMDEE_PLAN_HD static constexpr int row_ints() { return (image_ints() + 2 + 3) & ~3; }
};

// Single-species fp64 force kernels keep only the three coordinate planes in LDS (24 B per record instead of the
// 32-byte HBM record): with a fixed plane pitch the three reads of a neighbour share one address register and differ
// in the instruction's immediate offset, and three workgroups fit a CU where the 32-byte tile allows two.
constexpr int SOA_SLOTS = 2048;                      // records a coordinate-plane tile can hold
// Plane pitch in records.  fp64: one record more than a power of two, so that the x and y reads of a neighbour cannot be
// merged into one ds_read2st64_b64 (8 LDS-array cycles per wavefront, MI355X_MICROARCH.md LDS table) and stay two
// ds_read_b64 (2 cycles each) off one address register with immediate offsets.
template <typename real>
constexpr int soa_pitch() { return SOA_SLOTS + (sizeof(real) == 8 ? 1 : 0); }
template <typename real, class Shape, int THREADS>
static inline size_t brick_force_lds_bytes_soa(int own_cap) {
    return (((size_t)3 * soa_pitch<real>() * sizeof(real) + 15) & ~(size_t)15) + BrickTableSizes<Shape, THREADS>::bytes(own_cap);
}

// bytes of dynamic LDS: force tile = HBM records (+ te plane for fp32) (+ charge plane: charged instances); build tile = float4
template <typename real>
EMDEE_PLAN_HD inline size_t brick_charge_lds_bytes(int tile_cap) { return ((size_t)tile_cap * sizeof(real) + 15) & ~(size_t)15; }
template <typename real, class Shape, int THREADS>
static inline size_t brick_force_lds_bytes(int tile_cap, int own_cap, bool charged = false) {
    size_t tile_bytes = (size_t)tile_cap * rec_bytes<real>();
    size_t te_bytes = sizeof(real) == 4 ? (((size_t)tile_cap * 4 + 15) & ~(size_t)15) : 0;
    return tile_bytes + te_bytes + (charged ? brick_charge_lds_bytes<real>(tile_cap) : 0) + BrickTableSizes<Shape, THREADS>::bytes(own_cap);
}
template <class Shape, int THREADS>
static inline size_t brick_build_lds_bytes(int tile_cap, int own_cap, int stride, int G, int nsub = 1) {
    // + one row buffer (stride uint16) per G-lane group
    // + the candidate rows of every own cell ({first slot, span} of its 9 tile rows, and one all-zero set for ghosts)
    // (one packed word per row; nsub > 1: one set of rows per own cell AND sub-bin)
    return (size_t)tile_cap * 16 + BrickTableSizes<Shape, THREADS>::bytes(own_cap) + (size_t)(THREADS / G) * stride * 2 +
           (((size_t)(Shape::NOC * nsub + 1) * 9 * 4 + 15) & ~(size_t)15);
}

// ---- two-species boxes (typed.hpp) ----
// planes of a typed tile: records per plane (compile time: the three reads of a neighbour share one address register).
// 512-thread workgroups keep the single-species pitch (three workgroups per CU); 1024-thread ones -- long cutoffs: the
// rc = 3.5 sigma tile holds ~4400 records -- take one workgroup per CU and 4608 records.
// (round 5: bricks of 2 x 2 x 2 cells -- 64 tile cells, 2916 records at rc = 3.5 sigma and rho* = 0.8 before the melt's fluctuations; 3104 slots are what half a
// CU's LDS holds in fp64 next to the tables -- in 512-thread workgroups, TWO per CU:
// with one 1024-thread workgroup per CU the vector units idled 30 % of the kernel -- nothing computes while a tile is staged
// or a workgroup is replaced, profiles/r05/valu_f64_mix_rc3.5.txt)
template <class Shape, int THREADS>
constexpr int typed_slots() { return THREADS >= 1024 ? 4608 : (Shape::NOC == 8 ? 3104 : SOA_SLOTS); }
template <typename real, class Shape, int THREADS>
constexpr int typed_pitch() { return typed_slots<Shape, THREADS>() + (sizeof(real) == 8 ? 1 : 0); }
// index blocks of a row (= of its species-0 segment) fetched one atom ahead: two of 32 entries where rows are short, four where
// the workgroup is a long-row one (rc = 3.5 sigma: ~92 neighbours per species; NOC = own cells of the brick shape)
constexpr int typed_prefetch_blocks(int G, int THREADS, int NOC = 16) { return (EPL * G) >= 128 ? 1 : ((G == 4 && (THREADS >= 1024 || NOC == 8)) ? 4 : 2); }
// entries the build's LDS row buffer holds per atom: ONE segment (the two species are emitted and flushed one after the other)
constexpr int typed_seg_cap(int stride, int GL) { return ((stride / 2) + EPL * GL - 1) / (EPL * GL) * (EPL * GL); }
template <typename real, class Shape, int THREADS>
static inline size_t typed_force_lds_bytes(int own_cap) {
    return (((size_t)3 * typed_pitch<real, Shape, THREADS>() * sizeof(real) + 15) & ~(size_t)15) + BrickTableSizes<Shape, THREADS, TNT>::bytes(own_cap) + 256;   // (+ the four pair-constant records)
}
template <class Shape, int THREADS>
static inline size_t typed_build_lds_bytes(int tile_cap, int own_cap, int stride, int G, int GL = 4) {
    return (size_t)tile_cap * 16 + BrickTableSizes<Shape, THREADS, TNT>::bytes(own_cap) + (size_t)(THREADS / G) * typed_seg_cap(stride, GL) * 2 +
           (((size_t)(Shape::NOC * 4 + 1) * 9 * TNT * 4 + 15) & ~(size_t)15);   // (row table: one packed word per (own cell, x quarter, species, row))
}

// ---- brick kernel variants (shape, workgroup size, lanes per atom); variant 0 is the default ----
template <int V>
struct BrickVariant;
// G = lanes per atom in the force kernels (and the row layout), GB = lanes per atom in the build kernel
template <> struct BrickVariant<0> { using Shape = BrickShape<4, 2, 2>; static constexpr int ID = 0, THREADS = 512, G = 4, GB = 8; };
// (7: the 1024-thread workgroup of variant 8 with FOUR lanes per atom: long rows, e.g. the rc = 3.5 sigma mixture -- 184 entries
// are 46 pair steps per lane -- amortise a round's fixed work over 16 atoms per wavefront instead of 8)
template <> struct BrickVariant<7> { using Shape = BrickShape<4, 2, 2>; static constexpr int ID = 7, THREADS = 1024, G = 4, GB = 8; };
template <> struct BrickVariant<8> { using Shape = BrickShape<4, 2, 2>; static constexpr int ID = 8, THREADS = 1024, G = 8, GB = G; };
// (9, round 5: two-species boxes with long rows on bricks of 2 x 2 x 2 cells -- a tile of 64 cells, ~2850 records at rc = 3.5 sigma,
// fits TWO 512-thread workgroups on a CU where variant 7's 96-cell tile leaves room for one of 1024: while one workgroup stages
// its tile or is being replaced, the other computes)
template <> struct BrickVariant<9> { using Shape = BrickShape<2, 2, 2>; static constexpr int ID = 9, THREADS = 512, G = 4, GB = 8; };

template <class F>
static inline void with_brick_variant(int v, F &&f) {
    switch (v) {
        case 7: f(BrickVariant<7>{}); break;
        case 8: f(BrickVariant<8>{}); break;
        case 9: f(BrickVariant<9>{}); break;
        default: f(BrickVariant<0>{}); break;
    }
}
// typed boxes (typed.hpp): variants 0 and 7 (4 lanes per atom, 512 / 1024 threads) and 9 carry the two-species kernels
template <class V>
constexpr bool typed_variant() {
    return std::is_same<V, BrickVariant<0>>::value || std::is_same<V, BrickVariant<7>>::value || std::is_same<V, BrickVariant<9>>::value;
}
template <class V>
constexpr int typed_min_stride() { return (typed_prefetch_blocks(V::G, V::THREADS, V::Shape::NOC) + 1) * EPL * V::G; }
// variants a general-species box reaches (0, and 8 for long rows) carry the charged force instances
template <class V>
constexpr bool charged_variant() { return std::is_same<V, BrickVariant<0>>::value || std::is_same<V, BrickVariant<8>>::value; }

// ---- the plan ----
enum PlanReason { PLAN_OK = 0, PLAN_NO_BRICK_PATH = 1, PLAN_NO_ATOMS = 2, PLAN_TILE_TOO_LARGE = 3, PLAN_BUILD_TOO_LARGE = 4 };

// everything a launch site reads; default-constructed = no plan (the direct kernels)
struct BrickPlan {
    bool active = false, typed = false;   // the brick kernels are in use; the two-species ones (typed.hpp)
    int reason = PLAN_OK;                 // of an inactive plan: the condition that failed
    int variant = 0;
    BrickGrid grid{};
    int tile_cap = 0, own_cap = 0, row_block = 1;
    int stride = 0;                       // entries per row the plan asks for: whole lane-major blocks
    bool typed_stride = false;            // ... which already include the typed rows' segment padding
    int build_alg = 1;                    // k_brick_build ALG (3 / 5 = two-phase, 16- / 32-bit hit fields; 1 when a tile row is too crowded for both)
    int span3_limit = 0;                  // most atoms in three consecutive cells of a tile row the chosen build kernel can take
    int idx_shift = 0;                    // neighbour entries = tile slot << idx_shift; single-species and typed boxes store byte offsets into the coordinate planes
    size_t lds_force = 0, lds_build = 0;  // dynamic LDS of the force kernels' record tile (typed: their planes) and of the build
    float build_margin = 0.f;
    int maxima[3] = {0, 0, 0};            // the populations it was made from: largest tile, most own atoms, widest three-cell span
    // what it was planned for (plan_kept)
    int M[3] = {0, 0, 0}, n = 0;
    bool uniform = false, charged = false;
    int nt = 1;
};

// everything the decision depends on, and nothing else
struct PlanFacts {
    int real_bytes = 8;
    int M[3] = {1, 1, 1}, per[3] = {1, 1, 1};
    double len[3] = {1, 1, 1}, rlist = 1;
    int n = 0, n_plan = 0;                // atoms (an upper bound inside an in-place edit), and before the edit
    int nt = 1, nsub = 1;
    bool uniform = false, charged = false, ewald = false, filters_rows = false, brick_path = true, in_edit = false;
    int stride = 0;                       // the list's current row stride
    bool typed_stride = false;
    bool field16_blocked = false, typed_blocked = false;   // "until the next load" blocks
    bool typed_all = false, typed_bricks7 = false, debug = false;   // EMDEE_TYPED_ALL, EMDEE_TYPED_BRICKS=7, EMDEE_DEBUG_PLAN
};

template <class S>
inline BrickGrid brick_grid(const int M[3], const int per[3]) {
    BrickGrid g{};
    g.nb[0] = (M[0] + S::BX - 1) / S::BX;
    g.nb[1] = (M[1] + S::BY - 1) / S::BY;
    g.nb[2] = (M[2] + S::BZ - 1) / S::BZ;
    g.nbricks = g.nb[0] * g.nb[1] * g.nb[2];
    g.per_xcd = (g.nbricks + NXCD - 1) / NXCD;
    // interior bricks: along an open dimension, those whose tile (brick +- 1 cell) stays clear of
    // the outermost cell layers, where the ghosts of a decomposed run live
    const int B[3] = {S::BX, S::BY, S::BZ};
    g.ib_count = 1;
    for (int d = 0; d < 3; d++) {
        int lo_b = 0, n_b = g.nb[d];
        if (!per[d]) {
            lo_b = 1;
            int hi_b = 1;
            while (hi_b < g.nb[d] && (hi_b + 1) * B[d] < M[d] - 1) hi_b++;
            n_b = std::max(0, hi_b - lo_b);
        }
        g.ib_lo[d] = lo_b; g.ib_n[d] = n_b;
        g.ib_count *= n_b;
    }
    g.ib_per_xcd = (g.ib_count + NXCD - 1) / NXCD;
    g.bb_z = (g.nb[2] - g.ib_n[2]) * g.nb[0] * g.nb[1];
    g.bb_y = g.ib_n[2] * (g.nb[1] - g.ib_n[1]) * g.nb[0];
    g.bb_count = g.nbricks - g.ib_count;
    g.bb_per_xcd = (g.bb_count + NXCD - 1) / NXCD;
    return g;
}

// K: how many quarters of a neighbour cell lie beyond r_list whatever the atom's position in its own quarter: the
// quarters < s + K of the left cell are at least (1 + (K - 1) / 4) cell widths away.  0 for a cell a little wider than
// r_list; -1 (one more quarter on either side) when the cell is r_list to within the margin that covers the rounding
// of M t in the box's own precision (t carries ~2 ulp of 1, M t as many ulp of M: 16 M eps is 8e-5 for the fp32 10^7-atom
// box, whose cells are 8.6e-4 wider than r_list)
inline int plan_sub_k(int real_bytes, double len_x, int Mx, double rlist) {
    const double cx = len_x / std::max(1, Mx);
    const double margin = 16.0 * Mx * (real_bytes == 4 ? 6.0e-8 : 1.2e-16) + 1e-9;
    return std::max(-1, (int)std::floor(4.0 * (1.0 - rlist * (1.0 + margin) / cx)));
}

// ---- the `emdee plan:` lines of EMDEE_DEBUG_PLAN (NbSystem prints them; six GPU test modules parse them) ----
template <typename... A>
inline std::string plan_format(const char *fmt, A... a) {
    char buf[512];
    std::snprintf(buf, sizeof(buf), fmt, a...);
    return buf;
}
inline std::string plan_text_bricks(const BrickPlan &p, const PlanFacts &f) {
    return plan_format("emdee plan: bricks %d x %d x %d, tile_cap %d (max %d), own_cap %d (max %d), max 3-cell span %d, x sub-bins %d K %d, variant %d\n",
                       p.grid.nb[0], p.grid.nb[1], p.grid.nb[2], p.tile_cap, p.maxima[0], p.own_cap, p.maxima[1], p.maxima[2], f.nsub,
                       plan_sub_k(f.real_bytes, f.len[0], f.M[0], f.rlist), p.variant);
}
inline std::string plan_text_typed(const BrickPlan &p, int span, int stride, size_t lds_force, size_t lds_build, bool ok) {
    return plan_format("emdee plan: two species, variant %d: tile_cap %d (max %d), own_cap %d, longest 3-cell span of one species %d, stride %d, LDS force %zu build %zu: typed kernels %s\n",
                       p.variant, p.tile_cap, p.maxima[0], p.own_cap, span, stride, lds_force, lds_build, ok ? "on" : "off");
}
inline std::string plan_text_no_build() { return "emdee plan: the build kernel's tile does not fit LDS: direct kernels\n"; }
inline std::string plan_text_charged(bool active, int variant, size_t lds_force) {
    return plan_format("emdee plan: charged engine, %s, variant %d, LDS force %zu\n", active ? "brick kernels" : "direct kernels", variant, lds_force);
}

// A plan is kept from one rebuild to the next (the populations barely change): capacities carry a few percent of
// headroom, and the maxima of the NEW populations are checked after the build, together with its overflow words.
inline int with_headroom(int v) { return (v + v / 32 + 8 + 15) / 16 * 16; }

// capacities, build kernel and LDS sizes of variant V for the population maxima {largest tile, most own atoms, widest
// three-cell span}; stride: the list's current one (0: none yet)
template <typename real, class V>
inline BrickPlan plan_sizes(const PlanFacts &f, int stride, const int maxima[3]) {
    using S = typename V::Shape;
    const int max_tile = maxima[0], max_own = maxima[1], max_span3 = maxima[2];
    BrickPlan p;
    p.variant = V::ID;
    p.grid = brick_grid<S>(f.M, f.per);
    p.row_block = EPL * V::G;
    for (int k = 0; k < 3; k++) p.maxima[k] = maxima[k];
    p.tile_cap = std::max(64, with_headroom(max_tile + 1));   // + 1: the sentinel record
    // (the single-species kernels keep coordinate planes of SOA_SLOTS records: do not let the headroom alone push a tile past them)
    if (max_tile + 1 <= SOA_SLOTS) p.tile_cap = std::min(p.tile_cap, SOA_SLOTS);
    p.own_cap = std::max(64, with_headroom(max_own));
    {   // ... nor cost a workgroup per CU in the build or force kernels: give headroom back 16 records at a time
        const int exact = std::max(64, (max_tile + 1 + 15) / 16 * 16), st = stride > 0 ? stride : 128;
        // (a CU holds three workgroups only up to ~50,000 B each, not 160 KB / 3: measured in round 2 by padding the launch)
        constexpr size_t USABLE = 150000;
        auto per_cu = [&](int tc) {
            const size_t b = brick_build_lds_bytes<S, V::THREADS>(tc, p.own_cap, st, V::GB, f.nsub),
                         fb = brick_force_lds_bytes<real, S, V::THREADS>(tc, p.own_cap, f.charged);
            return (int)(USABLE / std::max<size_t>(b, 1)) * 16 + (int)(USABLE / std::max<size_t>(fb, 1));
        };
        while (p.tile_cap > exact && per_cu(p.tile_cap) < per_cu(exact)) p.tile_cap -= 16;
    }
    const int span3 = max_span3 + max_span3 / 16 + 2;
    p.build_alg = (!f.field16_blocked && (V::GB == 8 || V::GB == 16) && span3 <= BUILD2_FIELD * V::GB) ? 3 : 1;
    // crowded tile rows (long cutoffs): the same build with one 32-bit hit field per row
    if (p.build_alg == 1 && (V::GB == 8 || V::GB == 16) && span3 <= 32 * V::GB) p.build_alg = 5;
    if (p.build_alg == 1) p.span3_limit = 1 << 30;               // the ballot build has no limit
    else p.span3_limit = (p.build_alg == 5 ? 32 : BUILD2_FIELD) * V::GB;   // what the chosen build can take
    p.lds_force = brick_force_lds_bytes<real, S, V::THREADS>(p.tile_cap, p.own_cap, f.charged);
    // fp32 pre-test of the build kernel (fp64 boxes): brick-relative coordinates are below
    // cmax, so each is off by <= cmax 2^-24 after rounding; with |d| <= r_list per component the
    // error of d^2 is below 4 sqrt(3) r_list cmax 2^-24 + 4 r_list^2 2^-23.  Band = 4 x that bound.
    if (sizeof(real) == 8) {
        double cmax = 0.0;
        const int B[3] = {S::BX, S::BY, S::BZ};
        for (int d = 0; d < 3; d++) cmax = std::max(cmax, (B[d] + 2) * f.len[d] / f.M[d]);
        const double bound = 4.0 * 1.7320508 * f.rlist * cmax * std::ldexp(1.0, -24) + 4.0 * f.rlist * f.rlist * std::ldexp(1.0, -23);
        p.build_margin = (float)(4.0 * bound);
    }
    return p;
}
// does the force kernels' record tile fit LDS and the 16-bit slots of the rows?
inline bool plan_tile_fits(const BrickPlan &p) { return p.lds_force <= LDS_LIMIT && p.tile_cap < 65536; }
// dynamic LDS of the build kernel the plan launches (the general-species build, or the two-segment one) at a row stride
inline size_t plan_build_lds(const BrickPlan &p, bool typed, int stride, int nsub) {
    size_t bytes = 0;
    with_brick_variant(p.variant, [&](auto v) {
        using V = decltype(v);
        bytes = typed ? typed_build_lds_bytes<typename V::Shape, V::THREADS>(p.tile_cap, p.own_cap, stride, V::GB, V::G)
                      : brick_build_lds_bytes<typename V::Shape, V::THREADS>(p.tile_cap, p.own_cap, stride, V::GB, nsub);
    });
    return bytes;
}

// do the maxima of the current populations fit the plan in use?
inline bool plan_holds(const BrickPlan &p, const int maxima[3]) {
    return maxima[0] + 1 <= p.tile_cap && maxima[1] <= p.own_cap && maxima[2] <= p.span3_limit;
}
// The plan of the previous build of a state is kept when the cell grid is the same and the atom count has moved by less than
// an eighth: the populations barely change between rebuilds, the capacities carry headroom, and the maxima of the new
// populations come back with the build's overflow words (plan_holds).
// (inside an in-place edit n is an upper bound: the plan is compared with the number of atoms before the edit)
inline bool plan_kept(const BrickPlan &p, const PlanFacts &f) {
    const int np = f.in_edit ? f.n_plan : f.n;
    return p.active && f.brick_path && f.n > 0 && p.M[0] == f.M[0] && p.M[1] == f.M[1] && p.M[2] == f.M[2] && p.n <= np + np / 8 &&
           np <= p.n + p.n / 8 && p.uniform == f.uniform && p.nt == f.nt && p.charged == f.charged;
}

template <typename real, class Measure>
inline BrickPlan choose_plan_as(const PlanFacts &f, Measure &&measure, std::string &text) {
    constexpr int PLANE_SHIFT = sizeof(real) == 8 ? 3 : 2;
    int stride = f.stride;
    bool typed_stride = f.typed_stride;
    // variant v sized for the populations of its brick shape
    auto sized = [&](int variant) {
        BrickPlan q;
        with_brick_variant(variant, [&](auto v) {
            using V = decltype(v);
            const std::array<int, 3> m = measure.maxima(typename V::Shape{});
            q = plan_sizes<real, V>(f, stride, m.data());
        });
        if (f.debug) text += plan_text_bricks(q, f);
        return q;
    };
    BrickPlan p;
    int reason = !f.brick_path ? PLAN_NO_BRICK_PATH : f.n <= 0 ? PLAN_NO_ATOMS : PLAN_OK;
    if (reason == PLAN_OK) {
        p = sized(0);
        if (!plan_tile_fits(p)) reason = PLAN_TILE_TOO_LARGE;
    }
    // A tile too large for two workgroups of the default variant per CU (long cutoffs, dense boxes: rc = 3.5
    // sigma needs 135 KB) would leave 2 waves per SIMD: take the same bricks with 1024-thread workgroups
    // (measured on the rc = 3.5 mixture: 116 -> 154 steps/s).
    // (Ewald engines stay on variant 0, one workgroup per CU if need be: under the 128-register budget of 1024 threads the
    // erfc of their pair loop would spill to scratch memory)
    if (reason == PLAN_OK && p.lds_force > LDS_LIMIT / 2 && !f.ewald) {
        p = sized(8);
        if (!plan_tile_fits(p)) p = sized(0);
    }
    if (reason == PLAN_OK) {
        stride = (stride + p.row_block - 1) / p.row_block * p.row_block;   // whole lane-major blocks
        with_brick_variant(p.variant, [&](auto v) { stride = std::max(stride, brick_min_stride(decltype(v)::G, decltype(v)::THREADS)); });
        // the build kernel's LDS (fp32 tile + tables + one row buffer per lane group) must fit as well: very dense or
        // very inhomogeneous boxes with a long cutoff fall back to the direct (global-gather) kernels
        if (plan_build_lds(p, false, stride, f.nsub) > LDS_LIMIT) {
            reason = PLAN_BUILD_TOO_LARGE;
            if (f.debug) text += plan_text_no_build();
        }
    }
    int idx_shift = (reason == PLAN_OK && p.variant == 0 && f.uniform && !f.charged && p.tile_cap <= SOA_SLOTS) ? PLANE_SHIFT : 0;
    // two species: the typed kernels (typed.hpp), if the tile fits their coordinate planes, no three cells of a tile row hold
    // more atoms of one species than the 16-bit hit fields of their build take, and both kernels fit LDS
    bool typed = false;
    if (reason == PLAN_OK && f.nt == 2 && !f.typed_blocked && !f.filters_rows && !f.charged) {
        // (where the general-species kernels take 1024 threads with 8 lanes per atom -- long cutoffs -- the typed ones take
        // 1024 threads with 4: rows are two block-aligned segments, and blocks of 32 entries pad them half as much as blocks of 64)
        // Measured (profiles/README.md, round 3): at rc = 3.5 sigma 190.7 -> 218.0 steps/s in fp64 and 233.8 -> 324.2 in fp32; at
        // rc = 2.5 (variant 0, rows of ~37 entries per species) the 18 short candidate rows cost the build more than the
        // pair loop gains, 453.9 -> 419.1: short-row boxes keep the general-species kernels (EMDEE_TYPED_ALL=1 overrides)
        // Long rows (the general kernels chose 1024-thread workgroups): first the small bricks of variant 9, two 512-thread
        // workgroups per CU -- if its tile and both kernels fit half a CU's LDS --, then variant 7 (EMDEE_TYPED_BRICKS=7: the
        // A/B baseline).  Short rows: variant 0, on request only.
        const int keep = p.variant;
        int cands[2] = {-1, -1};
        if (keep == 8) {
            cands[0] = f.typed_bricks7 ? 7 : 9;
            cands[1] = f.typed_bricks7 ? -1 : 7;
        } else if (keep == 0 && f.typed_all) {
            cands[0] = keep;
        }
        for (int ci = 0; ci < 2 && !typed; ci++) {
            const int cand = cands[ci];
            if (cand < 0) continue;
            p = sized(cand);                                     // (another brick shape: its own population maxima)
            with_brick_variant(cand, [&](auto v) {
                using V = decltype(v);
                if constexpr (typed_variant<V>()) {
                    using S = typename V::Shape;
                    // (the planes hold typed_slots records: do not let the headroom alone push a tile past them)
                    constexpr int slots = typed_slots<S, V::THREADS>();
                    if (p.maxima[0] + 1 <= slots) p.tile_cap = std::min(p.tile_cap, slots);
                    const int span = measure.typed_span(S{});
                    int st = stride;
                    if (!typed_stride) {
                        st = std::max(stride, typed_min_stride<V>()) + p.row_block;   // + the padding between the two segments
                        st = (st + p.row_block - 1) / p.row_block * p.row_block;
                    }
                    const size_t lds_f = typed_force_lds_bytes<real, S, V::THREADS>(p.own_cap),
                                 lds_b = typed_build_lds_bytes<S, V::THREADS>(p.tile_cap, p.own_cap, st, V::GB, V::G);
                    // (variant 9 exists to put two workgroups on a CU: it is taken only where both kernels leave room for that)
                    const size_t room = cand == 9 ? LDS_LIMIT / 2 - 128 : LDS_LIMIT;   // (- the kernels' static LDS)
                    const bool ok = p.tile_cap <= slots && span <= 16 * V::GB && lds_f <= room && lds_b <= room;
                    if (f.debug) text += plan_text_typed(p, span, st, lds_f, lds_b, ok);
                    if (ok) {
                        typed = true;
                        stride = st;
                        typed_stride = true;
                        idx_shift = PLANE_SHIFT;
                        p.lds_force = lds_f;
                    }
                }
            });
        }
        if (!typed && p.variant != keep) p = sized(keep);
    }
    if (!typed) typed_stride = false;
    if (f.charged && f.debug) text += plan_text_charged(reason == PLAN_OK, p.variant, p.lds_force);
    if (reason != PLAN_OK) p = BrickPlan{};
    p.active = reason == PLAN_OK;
    p.reason = reason;
    p.typed = typed;
    p.stride = stride;
    p.typed_stride = typed_stride;
    p.idx_shift = idx_shift;
    if (p.active) p.lds_build = plan_build_lds(p, typed, stride, f.nsub);
    p.uniform = f.uniform;
    p.charged = f.charged;
    p.nt = f.nt;
    p.n = f.in_edit ? f.n_plan : f.n;
    for (int d = 0; d < 3; d++) p.M[d] = f.M[d];
    return p;
}
// Variant, capacities, build kernel, stride rounding and index encoding for the facts of a state.  The populations come from
// `measure` alone: measure.maxima(shape) = {largest tile, most own atoms, widest three-cell span} of the bricks of that shape,
// measure.typed_span(shape) = the widest three-cell span of one species.  Writes nothing but its result and, under f.debug,
// the plan's lines appended to `text`.
template <class Measure>
inline BrickPlan choose_plan(const PlanFacts &f, Measure &&measure, std::string &text) {
    return f.real_bytes == 8 ? choose_plan_as<double>(f, measure, text) : choose_plan_as<float>(f, measure, text);
}

// After a build whose longest row (`needed`) did not fit the stride: the stride grows by an eighth, rounded to whole blocks
// under an active plan.  When the build kernel no longer fits LDS at that stride, a typed plan asks for the typed kernels to
// be blocked (the caller plans again, this state goes on with the general-species kernels) and any other plan gives way to
// the direct kernels.
inline BrickPlan after_build(BrickPlan p, int nsub, int needed, bool &block_typed) {
    block_typed = false;
    int stride = (needed + needed / 8 + 15) / 16 * 16;
    if (p.active) stride = (stride + p.row_block - 1) / p.row_block * p.row_block;
    if (p.active) p.lds_build = plan_build_lds(p, p.typed, stride, nsub);
    if (p.active && p.lds_build > LDS_LIMIT) {
        if (p.typed) block_typed = true;
        else {
            p = BrickPlan{};
            p.reason = PLAN_BUILD_TOO_LARGE;
        }
    }
    p.stride = stride;
    return p;
}

}  // namespace emdee
