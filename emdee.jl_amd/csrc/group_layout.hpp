// group_layout.hpp -- the table order of a per-atom group array, shared by the displacement correlations (msd.hpp) and the centre-of-mass
// pull (pull.hpp): the grouped atoms group-major, ascending id inside a group, cut into chunks of one group each.  Made once from the
// group array on the host; a rebuild of the neighbour list re-sorts the engine's records and leaves it alone.  Plain C++, no HIP.
#pragma once

#include <vector>

namespace emdee {

constexpr int MSD_MAX_GROUPS = 8;
// the atoms of one workgroup of k_msd_accumulate: MSD_BLOCK threads x MSD_PER_THREAD atoms.  The chunks are made from the table
// alone, never from the device's CU count: the order of every sum is the same on every machine.
constexpr int MSD_BLOCK = 256, MSD_PER_THREAD = 4, MSD_CHUNK = MSD_BLOCK * MSD_PER_THREAD;

// ---- the table order
// entry e of a snapshot belongs to the atom id with pos_of[id] == e: the groups one after the other, ascending id inside a group,
// atoms of group -1 absent (pos_of = -1).  chunk_of_group[g] ... chunk_of_group[g + 1] - 1 are the chunks of group g, each at most
// MSD_CHUNK consecutive entries of that group alone.
struct MsdChunk {
    int first, count, group;
};
struct MsdLayout {
    std::vector<int> pos_of;
    std::vector<MsdChunk> chunks;
    long long sizes[MSD_MAX_GROUPS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int chunk_of_group[MSD_MAX_GROUPS + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int n_grouped = 0;
};
// group: n entries in -1 ... n_groups - 1 (checked by the caller), or NULL: every atom in group 0
inline MsdLayout msd_layout(const int *group, int n, int n_groups) {
    MsdLayout t;
    t.pos_of.assign((size_t)n, -1);
    for (int i = 0; i < n; i++) {
        const int g = group ? group[i] : 0;
        if (g >= 0) t.sizes[g]++;
    }
    int first[MSD_MAX_GROUPS + 1];
    first[0] = 0;
    for (int g = 0; g < n_groups; g++) first[g + 1] = first[g] + (int)t.sizes[g];
    t.n_grouped = first[n_groups];
    int fill[MSD_MAX_GROUPS];
    for (int g = 0; g < n_groups; g++) fill[g] = first[g];
    for (int i = 0; i < n; i++) {
        const int g = group ? group[i] : 0;
        if (g >= 0) t.pos_of[(size_t)i] = fill[g]++;
    }
    for (int g = 0; g < n_groups; g++) {
        t.chunk_of_group[g] = (int)t.chunks.size();
        for (int e = first[g]; e < first[g + 1]; e += MSD_CHUNK)
            t.chunks.push_back(MsdChunk{e, first[g + 1] - e < MSD_CHUNK ? first[g + 1] - e : MSD_CHUNK, g});
    }
    for (int g = n_groups; g <= MSD_MAX_GROUPS; g++) t.chunk_of_group[g] = (int)t.chunks.size();
    return t;
}

}  // namespace emdee
