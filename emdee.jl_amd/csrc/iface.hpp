// iface.hpp -- precision-erased interfaces between the C ABI (capi.hip) and the two template
// instantiations (impl_f32.hip, impl_f64.hip), so the translation units compile in parallel.
#pragma once

#include "common.hpp"

namespace emdee {

struct ICells {
    virtual ~ICells() {}
    virtual void update(const void *positions) = 0;
    virtual int M() const = 0;
    virtual void arrays(const int32_t **index, const int32_t **population, const int32_t **start,
                        const int32_t **order) const = 0;
};

struct INbr {
    virtual ~INbr() {}
    virtual void compute(void *forces, void *energies, void *virials, const void *positions, double L,
                         const emdee_lj_model &model, const emdee_lj_atom *atoms, int bitmask) = 0;
    virtual void stats(int64_t *builds, int64_t *listed, int32_t *max_count, int32_t *capacity) = 0;
    virtual void count_pairs(int64_t *pairs) = 0;
    virtual void export_list(int32_t *counts, int32_t *neighbors, int32_t capacity) = 0;
    virtual void set_pairs(const int32_t *pairs, int32_t n_pairs, bool one_four, double lj14scale) = 0;
    virtual void compute_tensor(void *tensor, const void *positions, double L, const emdee_lj_model &model, const emdee_lj_atom *atoms) = 0;
};

struct IMd {
    virtual ~IMd() {}
    virtual void set_state(int n_owned, int n_ghost, const void *pos, const void *vel, const emdee_lj_atom *atoms,
                           const void *inv_mass) = 0;
    virtual void get_state(void *pos, void *vel, void *frc, void *en, void *vir) = 0;
    virtual void step(int nsteps, double dt, int rebuild_every) = 0;
    virtual void minimize(int max_iter, double f_tol, double dt_start, double dt_max, double max_step, emdee_minimize_result *out) = 0;
    virtual void kick_drift(double dt, double kick) = 0;
    virtual void forces(int bitmask, int phase) = 0;
    virtual void kick(double dt) = 0;
    virtual bool fused_step(double dt, double kick, int phase) = 0;
    virtual bool needs_rebuild() = 0;
    virtual void rebuild() = 0;
    virtual void pack_positions(const int32_t *ids, const int32_t *codes, int n, const double *shifts, int n_shifts,
                                void *buf) = 0;
    virtual void unpack_ghosts(const void *buf, int first, int n) = 0;
    virtual void energies(double out[3]) = 0;
    virtual void virial_tensor(void *out) = 0;
    virtual void pressure_tensor(double out[12]) = 0;
    virtual void molecular_pressure_tensor(double out[12]) = 0;
    virtual void set_molecular_scaling(int32_t on) = 0;
    virtual void stats(int64_t *builds, int64_t *listed, int32_t *max_count, int32_t *capacity) = 0;
    virtual void count_pairs(int64_t *pairs) = 0;
    virtual void export_list(int32_t *counts, int32_t *neighbors, int32_t capacity) = 0;
    virtual void profile(bool enable) = 0;
    virtual void kernel_time(int kernel, double *total_ms, int64_t *launches) = 0;
    virtual void set_langevin(double gamma, double temperature, uint64_t seed, uint64_t first_step) = 0;
    virtual void set_langevin_ids(const int64_t *ids) = 0;
    virtual void langevin_normals(uint64_t seed, uint64_t step, const int64_t *ids, int n, double *out) = 0;
    virtual void set_pairs(const int32_t *pairs, int32_t n_pairs, bool one_four, double lj14scale) = 0;
    virtual void set_bonded(int32_t kind, const int32_t *atoms, const double *params, int32_t n_terms) = 0;
    virtual void set_coulomb(const double *charges, int32_t n, double coulomb_k, double eps_rf, double coulomb14scale) = 0;
    virtual void set_rigid3(const int32_t *atoms, const double *geom, int32_t n_mol) = 0;
    virtual void set_molecules(const int32_t *molecule, int32_t n) = 0;
    virtual void set_hbonds(const int32_t *atoms, const double *dist, int32_t n_clusters) = 0;
    virtual void set_vsites(const int32_t *atoms, const double *weights, int32_t n_sites) = 0;
    virtual void set_restraints(const int32_t *atoms, const double *ref, const double *k, const double *flat, int32_t n) = 0;
    virtual void restraint_sums(double *out) = 0;
    virtual void get_restraint_refs(double *ref_dev) = 0;
    virtual void set_pull(const int32_t *group, int32_t n_groups, const int32_t *coords, const double *params, int32_t n_coords,
                          int32_t log_every, int32_t log_capacity) = 0;
    virtual void pull_read(double *coords_out, double *groups_out) = 0;
    virtual void pull_log_read(double *log_dev, int64_t *count, int64_t *dropped) = 0;
    virtual void set_alchemical(const int32_t *flag, double lambda, double alpha, const double *foreign, int32_t n_foreign, int32_t log_every,
                                int32_t log_capacity) = 0;
    virtual void set_lambda(double lambda) = 0;
    virtual void alchemical_read(double *words) = 0;
    virtual void alchemical_log_read(double *log_dev, int64_t *count, int64_t *dropped) = 0;
    virtual void set_alchemical_coulomb(int32_t enable, double lambda_q, double beta, const double *foreign_q, int32_t n_foreign) = 0;
    virtual void set_lambda_coulomb(double lambda_q) = 0;
    virtual void alchemical_coulomb_read(double *words) = 0;
    virtual void alchemical_coulomb_log_read(double *log_dev, int64_t *count, int64_t *dropped) = 0;
    virtual void set_ewald(double alpha, const int32_t *kmax) = 0;
    virtual void set_pme(double alpha, const int32_t *grid, int32_t order) = 0;
    virtual void get_box(double lo[3], double len[3]) = 0;
    virtual void scale_box(const double mu[3], double velocity_scale) = 0;
    virtual void set_barostat(int32_t kind, int32_t coupling, const double *p_ref, const double *compressibility, double tau_p,
                              int32_t every, double temperature, uint64_t seed, uint64_t first_step) = 0;
    virtual void set_thermostat(int32_t kind, double temperature, double tau_t, int32_t every, int64_t n_dof, int32_t chain,
                                uint64_t seed, uint64_t first_step) = 0;
    virtual void thermostat_state(double *out) = 0;
    virtual void set_thermostat_state(const double *in) = 0;
    virtual void thermostat_draws(uint64_t seed, uint64_t step, int64_t n_dof, double *out) = 0;
    virtual void set_rdf(double r_max, int32_t n_bins, int32_t n_groups, const int32_t *group_dev, const int32_t *molecule_dev) = 0;
    virtual void rdf_sample() = 0;
    virtual void rdf_read(int64_t *counts, int64_t *group_sizes, int64_t *frames, double *inv_volume_sum) = 0;
    virtual void rdf_reset() = 0;
    virtual void set_msd(int32_t what, int32_t n_groups, const int32_t *group_dev, int32_t n_lags, int32_t origin_every) = 0;
    virtual void msd_sample() = 0;
    virtual void msd_read(double *sums, int64_t *origins, int64_t *group_sizes, int64_t *samples) = 0;
    virtual void msd_reset() = 0;
    virtual void set_gk(int32_t what, int32_t n_lags) = 0;
    virtual void gk_sample() = 0;
    virtual void gk_read(double *sums, double *totals, double *last, int64_t *samples) = 0;
    virtual void gk_reset() = 0;
    virtual void set_spatial(int32_t geometry, int32_t what, int32_t n_bins, int32_t n_groups, const int32_t *group_dev, const double *range,
                             const double *centre, int32_t centre_group) = 0;
    virtual void spatial_sample() = 0;
    virtual void spatial_read(int64_t *counts, double *sums, int64_t *outside, int64_t *group_sizes, int64_t *frames, double *inv_bin_volume_sum) = 0;
    virtual void spatial_reset() = 0;
};

// spatial domain decomposition (emdee_dd_*): the domains of the decomposition that live in this process
struct IDd {
    virtual ~IDd() {}
    virtual void set_atoms(int local, int n, const void *pos, const void *vel, const emdee_lj_atom *atoms, const int64_t *gids) = 0;
    virtual void load() = 0;
    virtual void step(int nsteps, double dt, int rebuild_every) = 0;
    virtual void energies(double out[3]) = 0;
    virtual void pressure_tensor(double out[12]) = 0;
    virtual int64_t n_atoms_global() = 0;
    virtual int n_owned(int local) = 0;
    virtual int n_ghost(int local) = 0;
    virtual IMd *engine(int local) = 0;
    virtual void get_state(int local, int64_t *gids, void *pos, void *vel, void *frc) = 0;
    virtual void set_langevin(double gamma, double temperature, uint64_t seed, uint64_t first_step) = 0;
    virtual void stats(int64_t out[4]) = 0;
    virtual void rebuild_stats(int64_t out[4]) = 0;
    virtual void phase_times(double out[8]) = 0;
    virtual void set_overlap(bool on) = 0;
    virtual void set_pair_table(const int64_t *pairs, int64_t n_pairs, bool one_four, double lj14scale) = 0;
    virtual void set_bonded(int32_t kind, const int64_t *atoms, const double *params, int64_t n_terms) = 0;
    virtual void set_coulomb(const double *charges, int64_t n_ids, double coulomb_k, double eps_rf, double coulomb14scale) = 0;
};

void dd_rccl_selftest(emdee_ctx *ctx, int n_bytes);
// host-only description of one domain's geometry (dd.hpp: DdGeom), for emdee_dd_describe
void dd_describe(const double len[3], const int32_t grid[3], double halo, int rank, int32_t *ndirs, int32_t *dirs,
                 int32_t *dir_rank, double *dir_shift, int32_t *npeers, int32_t *peers, double *local_lo, double *local_len,
                 int32_t *periodic);

template <typename real>
struct Factory {
    static IDd *dd(emdee_ctx *ctx, const double len[3], const int32_t grid[3], int rank_first, int n_local,
                   const void *unique_id, const emdee_lj_model &model, double skin);
    static ICells *cells(emdee_ctx *ctx, int N, double L, double cutoff, int ndiv);
    static INbr *nbr(emdee_ctx *ctx, int N, double skin);
    static IMd *md(emdee_ctx *ctx, const double lo[3], const double len[3], const int32_t per[3],
                   const emdee_lj_model &model, double skin);
    static void tiles(emdee_ctx *ctx, void *f, void *e, void *w, const void *pos, double L, int N,
                      const emdee_lj_model &model, const emdee_lj_atom *atoms, int bitmask, int mode);
    static void naive(emdee_ctx *ctx, void *f, void *e, void *w, const void *pos, double L, int N,
                      const emdee_lj_model &model, const emdee_lj_atom *atoms, int mode);
    static void interaction(emdee_ctx *ctx, int n, const void *r2, const emdee_lj_model &model, emdee_lj_atom ai,
                            emdee_lj_atom aj, int mode, void *E, void *W);
};

}  // namespace emdee
