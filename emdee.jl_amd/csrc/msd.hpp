// msd.hpp -- mean-squared displacement and velocity autocorrelation on the device (emdee_md_set_msd, emdee_md_msd_sample): a ring of
// snapshots of the grouped atoms' unwrapped coordinates and velocities in HBM, and per sample one streaming pass that correlates
// the current snapshot with every live origin.  The snapshots are kept in an order of their own, made once from the group array
// (group-major, ascending id inside a group): a rebuild of the neighbour list re-sorts the engine's records and leaves them alone.
// The parts with no HIP in them -- the table order and its chunks, the schedule of origins, an atom's seven addends, a group's seven
// words -- are plain C++ at the top, as the top of rdf.hpp is: a stand-alone host program tests them with the host compiler
// (tests/c/msd_host.cpp); the kernels below them need HIP.  DESIGN.md 4h has the algorithm; MdImpl::msd_sample (impl.hpp) queues a sample.
#pragma once

#include <vector>

#include "group_layout.hpp"

#if defined(__HIPCC__)
#define EMDEE_HD __host__ __device__ __forceinline__
#else
#define EMDEE_HD inline
#endif

namespace emdee {

constexpr int MSD_MAX_LAGS = 4096, MSD_MAX_ORIGINS = 64;
constexpr int MSD_WORDS = 7;
constexpr int MSD_POSITIONS = 1, MSD_VELOCITIES = 2;         // (EMDEE_MSD, EMDEE_VACF)

// ---- the schedule
// Samples are numbered s = 0, 1, ...  Sample s is an origin when s % origin_every == 0; origin number k = s / origin_every lives in
// ring slot k % n_origins, n_origins = ceil(n_lags / origin_every).  At sample s the live origins are those with lag
// s - k origin_every < n_lags: the newest is k = s / origin_every, there are never more than n_origins of them, and consecutive k
// have distinct slots -- an origin is overwritten only by the origin n_origins later, whose first lag is already n_lags or more.
EMDEE_HD int msd_n_origins(int n_lags, int origin_every) { return (n_lags + origin_every - 1) / origin_every; }
EMDEE_HD int msd_live_count(long long s, int n_lags, int origin_every) {
    const long long newest = s / origin_every;
    const long long lag0 = s - newest * origin_every;       // the newest origin's lag, < origin_every
    if (lag0 >= n_lags) return 0;
    const long long most = (n_lags - 1 - lag0) / origin_every + 1;
    return (int)(most < newest + 1 ? most : newest + 1);
}
// the j-th live origin, newest first (j < msd_live_count)
EMDEE_HD void msd_live(long long s, int n_lags, int origin_every, int j, int &slot, int &lag) {
    const long long k = s / origin_every - j;
    slot = (int)(k % msd_n_origins(n_lags, origin_every));
    lag = (int)(s - k * origin_every);
}
struct MsdLive {
    int slot, lag;
};
struct MsdSchedule {
    bool is_origin = false;
    int slot = -1;                                           // the ring slot sample s is written to when it is an origin
    std::vector<MsdLive> live;
};
inline MsdSchedule msd_schedule(long long s, int n_lags, int origin_every) {
    MsdSchedule q;
    q.is_origin = s % origin_every == 0;
    if (q.is_origin) q.slot = (int)((s / origin_every) % msd_n_origins(n_lags, origin_every));
    const int n = msd_live_count(s, n_lags, origin_every);
    for (int j = 0; j < n; j++) {
        MsdLive l;
        msd_live(s, n_lags, origin_every, j, l.slot, l.lag);
        q.live.push_back(l);
    }
    return q;
}

// ---- the sums
// an atom's seven addends from its current entry c and its entry o at the origin, both {x, y, z, vx, vy, vz}: the squares of the
// displacement, the displacement, v(s) . v(s_o)
EMDEE_HD void msd_term(const double c[6], const double o[6], double out[MSD_WORDS]) {
    const double dx = c[0] - o[0], dy = c[1] - o[1], dz = c[2] - o[2];
    out[0] = dx * dx; out[1] = dy * dy; out[2] = dz * dz;
    out[3] = dx; out[4] = dy; out[5] = dz;
    out[6] = c[3] * o[3] + c[4] * o[4] + c[5] * o[5];
}
// a group's seven words from the totals of its atoms' addends for one origin: the drift is squared here, per origin
EMDEE_HD void msd_finish(const double total[MSD_WORDS], double out[MSD_WORDS]) {
    out[0] = total[0]; out[1] = total[1]; out[2] = total[2];
    out[3] = total[3] * total[3]; out[4] = total[4] * total[4]; out[5] = total[5] * total[5];
    out[6] = total[6];
}

}  // namespace emdee

#if defined(__HIPCC__)

#include "kernels.hpp"

namespace emdee {

// A snapshot is 3 or 6 planes of n_grouped doubles in table order -- x, y, z when positions are kept, then vx, vy, vz when velocities
// are: consecutive threads read consecutive doubles of a plane.  The ring is n_origins + 1 snapshots, the last one the scratch
// snapshot of a sample that is no origin.
// what a sample needs of the table
struct MsdArgs {
    int what, n_grouped, n_chunks, n_groups, n_lags, origin_every;
    long long s;
    size_t snapshot;                                         // doubles per snapshot
};

// One thread per slot p of the engine's order: the unwrapped coordinates by k_unsort's expression -- an fp64 engine's entry is bit
// for bit what emdee_md_get_state returns; a Float32 engine's is the record (plus the origin of its cell) plus the box lengths in
// double, not rounded to fp32 -- and the velocities, as doubles, to entry pos_of[id] of snapshot dst.
template <typename real>
__global__ __launch_bounds__(256) void k_msd_gather(int n, int n_owned, GridP<real> g, const int *__restrict__ img,
                                                    const int *__restrict__ perm, const Rec<real> *__restrict__ rec, RelGrid rel,
                                                    const real *__restrict__ vel, size_t pitch, const int *__restrict__ pos_of,
                                                    int what, int n_grouped, double *__restrict__ dst) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int id = perm[p];
    if (id < 0 || id >= n_owned) return;
    const int e = pos_of[id];
    if (e < 0 || e >= n_grouped) return;
    double *out = dst + e;
    if (what & MSD_POSITIONS) {
        const Rec<real> r = rec[p];
        int kx, ky, kz;
        img_unpack(img[p], kx, ky, kz);
        double x, y, z;
        if (sizeof(real) == 4) {
            x = (double)r.x; y = (double)r.y; z = (double)r.z;
            if (rel.on) {
                double ox, oy, oz;
                rel.origin(rel.cell[p], ox, oy, oz);
                x += ox; y += oy; z += oz;
            }
            x += (double)kx * (double)g.len[0];
            y += (double)ky * (double)g.len[1];
            z += (double)kz * (double)g.len[2];
        } else {
            x = r.x + (real)kx * g.len[0];
            y = r.y + (real)ky * g.len[1];
            z = r.z + (real)kz * g.len[2];
        }
        out[0] = x; out[(size_t)n_grouped] = y; out[2 * (size_t)n_grouped] = z;
        out += 3 * (size_t)n_grouped;
    }
    if (what & MSD_VELOCITIES)
        for (int d = 0; d < 3; d++) out[d * (size_t)n_grouped] = (double)vel[d * pitch + p];
}

// One workgroup per chunk.  A thread keeps the current entries of its MSD_PER_THREAD atoms in registers (entries first + t,
// first + t + 256, ...: every load of a wavefront is 512 contiguous bytes) and walks the live origins, newest first: every origin
// entry is read once, the current snapshot once for all of them.  Per origin the seven sums of the chunk go to
// partial[j][chunk][0..6] in block_sum's order -- lanes by wave_sum_to_lane63, then the four waves one after the other -- through
// two alternating LDS rows, so one barrier per origin is enough: row j & 1 is written again two origins later, behind the barrier
// of origin j + 1, which the readers of origin j reach only when they are done.
template <bool POS, bool VEL>
__global__ __launch_bounds__(MSD_BLOCK) void k_msd_accumulate(MsdArgs a, const MsdChunk *__restrict__ chunks,
                                                              const double *__restrict__ cur, const double *__restrict__ ring,
                                                              double *__restrict__ partial) {
    __shared__ double sh[2][MSD_WORDS][MSD_BLOCK / WAVE];
    const MsdChunk ch = chunks[blockIdx.x];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const size_t ng = (size_t)a.n_grouped;
    constexpr int VOFF = POS ? 3 : 0;
    double c[MSD_PER_THREAD][6];
#pragma unroll
    for (int k = 0; k < MSD_PER_THREAD; k++) {
        const int e = t + k * MSD_BLOCK;
        const bool in = e < ch.count;
        const size_t at = (size_t)ch.first + (in ? e : 0);
#pragma unroll
        for (int w = 0; w < 3; w++) {
            c[k][w] = (POS && in) ? cur[w * ng + at] : 0.0;
            c[k][3 + w] = (VEL && in) ? cur[(VOFF + w) * ng + at] : 0.0;
        }
    }
    const int n_live = msd_live_count(a.s, a.n_lags, a.origin_every);
    for (int j = 0; j < n_live; j++) {
        int slot, lag;
        msd_live(a.s, a.n_lags, a.origin_every, j, slot, lag);
        const double *org = ring + (size_t)slot * a.snapshot;
        double sum[MSD_WORDS];
#pragma unroll
        for (int w = 0; w < MSD_WORDS; w++) sum[w] = 0.0;
#pragma unroll
        for (int k = 0; k < MSD_PER_THREAD; k++) {
            const int e = t + k * MSD_BLOCK;
            const bool in = e < ch.count;
            const size_t at = (size_t)ch.first + (in ? e : 0);
            double o[6];
#pragma unroll
            for (int w = 0; w < 3; w++) {
                o[w] = (POS && in) ? org[w * ng + at] : 0.0;
                o[3 + w] = (VEL && in) ? org[(VOFF + w) * ng + at] : 0.0;
            }
            double term[MSD_WORDS];
            msd_term(c[k], o, term);                         // (an entry beyond the chunk: zeros against zeros)
#pragma unroll
            for (int w = 0; w < MSD_WORDS; w++) sum[w] += term[w];
        }
#pragma unroll
        for (int w = 0; w < MSD_WORDS; w++) {
            if ((w < 6 && !POS) || (w == 6 && !VEL)) continue;
            const double v = wave_sum_to_lane63(sum[w]);
            if (lane == WAVE - 1) sh[j & 1][w][wv] = v;
        }
        __syncthreads();
        if (t < MSD_WORDS) {
            double tot = 0.0;
            if ((t < 6 && POS) || (t == 6 && VEL))
                for (int w = 0; w < MSD_BLOCK / WAVE; w++) tot += sh[j & 1][t][w];
            partial[((size_t)j * a.n_chunks + blockIdx.x) * MSD_WORDS + t] = tot;
        }
    }
}

// One workgroup per (live origin j, group g): the group's chunk partials summed in chunk order (final_word, reduce.hpp), msd_finish,
// and thread 0 adds the seven words to sums[lag][g][0..6].  No two workgroups of a sample share a (lag, group), and the samples
// follow one another on the stream: plain loads and stores, no atomics.
static __global__ __launch_bounds__(RED_BLOCK) void k_msd_finish(MsdArgs a, const int *__restrict__ chunk_of_group,
                                                                 const double *__restrict__ partial, double *__restrict__ sums) {
    __shared__ double sh[RED_BLOCK / WAVE];
    const int j = blockIdx.x, g = blockIdx.y;
    int slot, lag;
    msd_live(a.s, a.n_lags, a.origin_every, j, slot, lag);
    const int c0 = chunk_of_group[g], c1 = chunk_of_group[g + 1];
    double total[MSD_WORDS];
#pragma unroll
    for (int w = 0; w < MSD_WORDS; w++) total[w] = final_word(c1 - c0, partial + ((size_t)j * a.n_chunks + c0) * MSD_WORDS, MSD_WORDS, w, false, sh);
    if (threadIdx.x == 0) {
        double out[MSD_WORDS];
        msd_finish(total, out);
        double *dst = sums + ((size_t)lag * a.n_groups + g) * MSD_WORDS;
#pragma unroll
        for (int w = 0; w < MSD_WORDS; w++) dst[w] += out[w];
    }
}

}  // namespace emdee
#endif
