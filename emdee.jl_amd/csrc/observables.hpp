// observables.hpp -- the tables of the on-device observables (emdee_md_set_rdf, emdee_md_set_msd, emdee_md_set_gk, emdee_md_set_spatial;
// rdf.hpp, msd.hpp, gk.hpp and spatial.hpp have the algorithms and the kernels): one record per observable, host fields and device buffers together, and the
// refusals they share, each formed once.  MdImpl (impl.hpp) builds a candidate record, checks it and swaps it in whole
// (MdImpl::install); NbSystem::rdf_sample / msd_sample / gk_sample / spatial_sample (nbsys.hpp) queue a sample on the record they are handed.  The
// part with no HIP in it -- the records' base, the texts and the gate -- is plain C++ at the top: a stand-alone host program
// drives it with the host compiler (tests/c/observables_host.cpp); the records below it own device memory.
#pragma once

#include "error.hpp"
#include "gk.hpp"
#include "msd.hpp"
#include "rdf.hpp"
#include "spatial.hpp"

namespace emdee {

enum ObsKind { OBS_RDF = 0, OBS_MSD = 1, OBS_GK = 2, OBS_SPATIAL = 3 };
// name: the prefix of the four entries' messages; since / replaced / rescaled: why a sample is refused after emdee_md_set_state or
// a rescaled box (nullptr: the observable pins neither -- a frame of the radial distribution functions stands alone)
struct ObsText { const char *name, *set, *setter, *reset, *since, *replaced, *rescaled; };
constexpr ObsText OBS_TEXT[4] = {
    {"rdf", "set_rdf", "emdee_md_set_rdf", "emdee_md_rdf_reset", nullptr, nullptr, nullptr},
    {"msd", "set_msd", "emdee_md_set_msd", "emdee_md_msd_reset", "the origins were taken", "a displacement between two states means nothing",
     "unwrapped coordinates across a rescaled box are not a displacement"},
    {"gk", "set_gk", "emdee_md_set_gk", "emdee_md_gk_reset", "the first sample", "a correlation between two states means nothing",
     "the stress and the heat flux are extensive and the Green-Kubo prefactor assumes one volume"},
    {"spatial", "set_spatial", "emdee_md_set_spatial", "emdee_md_spatial_reset", nullptr, nullptr, nullptr}};

// what the refusals ask of the engine (state_serial counts emdee_md_set_state)
struct ObsEngine {
    bool lent, has_ghosts, sorted, id_gaps;
    int n_owned, n_ghost;
    double len[3];
    uint64_t state_serial;
};
// what the three records share
struct ObsTable {
    bool present = false;
    int n_atoms = 0;
    int64_t samples = 0;                                     // s of the next sample (rdf: the frames)
    double len[3] = {0, 0, 0};                               // the box at the last set or reset
    uint64_t serial = 0;                                     // ... and the state serial
    void restart(const ObsEngine &e) {
        samples = 0; serial = e.state_serial;
        for (int d = 0; d < 3; d++) len[d] = e.len[d];
    }
};

// (a) a table is for an engine that sees the whole box, with a state loaded
inline void obs_require_whole_box(const char *fn, const ObsEngine &e) {
    EMDEE_REQUIRE(!e.lent, EMDEE_ERR_STATE, "%s: this integrator is a domain's, lent by emdee_dd_engine: it sees a part of the box only", fn);
    EMDEE_REQUIRE(e.n_ghost == 0 && !e.has_ghosts, EMDEE_ERR_STATE, "%s: an integrator with ghosts (its box is a domain of a larger one)", fn);
    EMDEE_REQUIRE(e.sorted && !e.id_gaps, EMDEE_ERR_STATE, "%s: no state loaded (call emdee_md_set_state first)", fn);
}
// (b) what sample, read and reset (`verb`) ask first
inline void obs_require_present(ObsKind kind, const char *verb, const ObsTable &t) {
    EMDEE_REQUIRE(t.present, EMDEE_ERR_STATE, "%s_%s: no table is set (call %s first)", OBS_TEXT[kind].name, verb, OBS_TEXT[kind].setter);
}
// (c) a sample: the table fits the state -- its atom count and, where the observable spans samples, the state and the box themselves
inline void obs_require_fit(ObsKind kind, const ObsTable &t, const ObsEngine &e) {
    const ObsText &x = OBS_TEXT[kind];
    EMDEE_REQUIRE(e.sorted && t.n_atoms == e.n_owned && e.n_ghost == 0 && !e.id_gaps, EMDEE_ERR_STATE, "%s_sample: the table was set for %d atoms, "
                  "the state holds %d: set it again (%s)", x.name, t.n_atoms, e.n_owned, x.setter);
    if (!x.since) return;
    EMDEE_REQUIRE(t.serial == e.state_serial, EMDEE_ERR_STATE, "%s_sample: the state has been replaced (emdee_md_set_state) since %s: %s; start "
                  "again with %s", x.name, x.since, x.replaced, x.reset);
    EMDEE_REQUIRE(t.len[0] == e.len[0] && t.len[1] == e.len[1] && t.len[2] == e.len[2], EMDEE_ERR_STATE, "%s_sample: the box has been rescaled "
                  "(emdee_md_scale_box or a barostat) since %s: %s; start again with %s", x.name, x.since, x.rescaled, x.reset);
}
// (d) a setter's group array, on the host: one entry per atom, -1 (left out) ... n_groups - 1
inline void obs_check_groups(ObsKind kind, const int32_t *group, int n, int n_groups) {
    for (int i = 0; i < n; i++)
        EMDEE_REQUIRE(group[i] >= -1 && group[i] < n_groups, EMDEE_ERR_INVALID, "%s: the group %d of atom %d is outside -1...%d", OBS_TEXT[kind].set,
                      group[i], i, n_groups - 1);
}

#if defined(__HIPCC__)
// Each record: zero() queues the clearing of the sums and starts the host's counters again (a set, a reset).  A record moves as a
// whole; the buffers of the one it replaces are freed with it (hipFree waits for the device: nothing in flight loses its memory).

// The table's copies of the caller's group and molecule arrays (caller order) and the u64 histogram; behind them the binning of
// one sample, sized by the sample that needs it.
struct RdfRecord : ObsTable {
    bool grouped = false, with_mol = false;
    int n_bins = 0, n_groups = 0;
    double r_max = 0.0, inv_dr = 0.0, inv_volume_sum = 0.0;
    int64_t sizes[RDF_MAX_GROUPS] = {0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf<int> group, mol, cell_of, count, fill;
    DevBuf<RdfAtom> atoms;
    DevBuf<unsigned long long> counts;
    Scanner scanner;
    int n_counters() const { return rdf_n_pairs(n_groups) * n_bins; }
    void zero(hipStream_t s, const ObsEngine &e) {
        EMDEE_HIP_CHECK(hipMemsetAsync(counts.ptr, 0, (size_t)n_counters() * sizeof(unsigned long long), s));
        inv_volume_sum = 0.0;
        restart(e);
    }
};
// The table order (pos_of, caller ids -> entries), its chunks, the ring of snapshots (n_origins + 1 of them, the last one the
// scratch snapshot), the chunk partials of one sample and the sums.
struct MsdRecord : ObsTable {
    int what = 0, n_groups = 0, n_lags = 0, origin_every = 1, n_origins = 0, n_grouped = 0, n_chunks = 0;
    int64_t sizes[MSD_MAX_GROUPS] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int64_t> origins;                            // per lag: the origins that have contributed
    DevBuf<int> pos_of, chunk_of_group;
    DevBuf<MsdChunk> chunks;
    DevBuf<double> ring, partial, sums;
    size_t snapshot() const { return (size_t)n_grouped * (((what & MSD_POSITIONS) ? 3 : 0) + ((what & MSD_VELOCITIES) ? 3 : 0)); }
    size_t n_sums() const { return (size_t)n_lags * n_groups * MSD_WORDS; }
    void zero(hipStream_t s, const ObsEngine &e) {
        EMDEE_HIP_CHECK(hipMemsetAsync(sums.ptr, 0, n_sums() * sizeof(double), s));
        origins.assign((size_t)n_lags, 0);
        restart(e);
    }
};
// The ring of samples (n_lags x 9), the lag sums with the totals and the last sample behind them (acc).
struct GkRecord : ObsTable {
    int what = 0, n_lags = 0;
    DevBuf<double> ring, acc;
    size_t ring_words() const { return (size_t)n_lags * GK_WORDS; }
    size_t acc_words() const { return ring_words() + 2 * GK_WORDS; }
    void zero(hipStream_t s, const ObsEngine &e) {
        EMDEE_HIP_CHECK(hipMemsetAsync(ring.ptr, 0, ring_words() * sizeof(double), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(acc.ptr, 0, acc_words() * sizeof(double), s));
        restart(e);
    }
};
// The table order (pos_of, and atoms: its inverse, one caller id per entry, for the centre group's centre of mass), its chunks, the
// planes of one sample (the bins, the masked addends), the chunks' runs (sorted bins, lengths, words), the sums and the counts
// (n_groups n_bins of them, then the eight `outside`).
struct SpatialRecord : ObsTable {
    int geometry = 0, what = 0, n_bins = 0, n_groups = 0, centre_group = -1, n_grouped = 0, n_chunks = 0;
    double range[2] = {0, 0}, centre[3] = {0, 0, 0}, inv_bin_volume_sum = 0.0;
    int64_t sizes[SPATIAL_MAX_GROUPS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int chunk_of_group[SPATIAL_MAX_GROUPS + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf<int> pos_of, atoms, chunk_of_group_dev, key, sbin, runn;
    DevBuf<MsdChunk> chunks;
    DevBuf<double> planes, runw, sums, partial, centre_dev;
    DevBuf<unsigned long long> counts;
    size_t n_cells() const { return (size_t)n_groups * n_bins; }
    size_t n_sums() const { return n_cells() * SPATIAL_WORDS; }
    void zero(hipStream_t s, const ObsEngine &e) {
        EMDEE_HIP_CHECK(hipMemsetAsync(sums.ptr, 0, n_sums() * sizeof(double), s));
        EMDEE_HIP_CHECK(hipMemsetAsync(counts.ptr, 0, (n_cells() + SPATIAL_MAX_GROUPS) * sizeof(unsigned long long), s));
        inv_bin_volume_sum = 0.0;
        restart(e);
    }
};
#endif

}  // namespace emdee
