"""numpy restatement of the radial distribution functions (include/emdee_hip.h: emdee_md_set_rdf): a brute force over all pairs in
fp64 with the library's conventions -- minimum image, bin (r * inv_dr).astype(int) with inv_dr = n_bins / r_max, a pair beyond the
last bin dropped, one histogram per unordered group pair in slot s(a, b) = a n_groups - a (a - 1) / 2 + (b - a), pairs of one
molecule skipped -- and the normalisation.  histogram() also counts, per bin edge k = 0 ... n_bins (edge n_bins is r_max), the pairs
within delta of the edge: the pairs whose bin a rounding of the positions could change."""
import numpy as np


# Two cases on which the x axis of the sample's grid does NOT wrap, so that the pair kernel takes a home cell's row along x as the
# run cx - nd ... cx + nd, and as two runs at the box faces -- what every cell of a large box does (tests/test_rdf_host.py pins
# the plans; tests/test_gpu_rdf.py compares the counts):
#   barostat_ref.fluid864 (L = 10.26) up to NOWRAP_FLUID_R_MAX: M = 6, 6, 6 with nd = 1, no axis wraps;
#   nowrap_box(): 864 atoms in 12.6 x 10.1 x 10.1 up to r_max = 5: M = 5, 4, 4 with nd = 2, x does not wrap, y and z do.
NOWRAP_FLUID_R_MAX = 1.5
NOWRAP_LENGTHS, NOWRAP_R_MAX, NOWRAP_N = (12.6, 10.1, 10.1), 5.0, 864


def nowrap_box():
    """positions (864, 3) drawn uniformly in the box NOWRAP_LENGTHS (lo = 0)"""
    return np.random.default_rng(5440).uniform(0.0, 1.0, (NOWRAP_N, 3)) * np.array(NOWRAP_LENGTHS)


def pair_slot(a, b, n_groups):
    a, b = min(a, b), max(a, b)
    return a * n_groups - a * (a - 1) // 2 + (b - a)


def n_pairs(n_groups):
    return n_groups * (n_groups + 1) // 2


def pairs(n_groups):
    return [(a, b) for a in range(n_groups) for b in range(a, n_groups)]


def histogram(pos, lengths, r_max, n_bins, groups=None, molecules=None, n_groups=None, delta=0.0, chunk=512):
    """counts (n_pairs, n_bins) int64 and edge_pairs (n_bins + 1,) int64 of the positions pos (n, 3) in the periodic box of sides
    `lengths`; groups / molecules: None or n integers (-1: not grouped / no molecule)"""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    L = np.asarray(lengths, dtype=np.float64).reshape(3)
    grp = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    mol = np.full(n, -1, dtype=np.int64) if molecules is None else np.asarray(molecules, dtype=np.int64)
    if n_groups is None:
        n_groups = max(int(grp.max()) + 1, 1) if n else 1
    inv_dr = n_bins / r_max
    edges = r_max * np.arange(n_bins + 1, dtype=np.float64) / n_bins
    counts = np.zeros((n_pairs(n_groups), n_bins), dtype=np.int64)
    edge_pairs = np.zeros(n_bins + 1, dtype=np.int64)
    idx = np.arange(n)
    for i0 in range(0, n, chunk):
        i = idx[i0:i0 + chunk]
        d = pos[None, :, :] - pos[i, None, :]
        d -= L * np.round(d / L)
        r = np.sqrt((d * d).sum(axis=2))
        keep = (idx[None, :] > i[:, None]) & (grp[i, None] >= 0) & (grp[None, :] >= 0)
        keep &= ~((mol[i, None] >= 0) & (mol[i, None] == mol[None, :]))
        ii, jj = np.nonzero(keep)
        rr = r[ii, jj]
        if delta > 0.0:
            near = rr < r_max + 2.0 * delta
            k = np.clip(np.rint(rr[near] * inv_dr).astype(np.int64), 0, n_bins)
            hit = np.abs(rr[near] - edges[k]) <= delta
            np.add.at(edge_pairs, k[hit], 1)
        b = (rr * inv_dr).astype(np.int64)
        ok = b < n_bins
        ga, gb = grp[i][ii[ok]], grp[jj[ok]]
        lo, hi = np.minimum(ga, gb), np.maximum(ga, gb)
        slot = lo * n_groups - lo * (lo - 1) // 2 + (hi - lo)
        np.add.at(counts, (slot, b[ok]), 1)
    return counts, edge_pairs


def normalise(counts, n_groups, r_max, sizes, frames, inv_volume_sum):
    """g and coordination, both (n_pairs, n_bins): g_ab = counts / (P_ab shell inv_volume_sum) with P_ab = N_a N_b (a != b) or
    N_a (N_a - 1) / 2; coordination = cumsum(counts) x (2 if a == b else 1) / (N_a frames)"""
    counts = np.asarray(counts, dtype=np.int64)
    n_bins = counts.shape[1]
    edges = r_max * np.arange(n_bins + 1, dtype=np.float64) / n_bins
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    g, coordination = np.zeros(counts.shape), np.zeros(counts.shape)
    for s, (a, b) in enumerate(pairs(n_groups)):
        P = 0.5 * sizes[a] * (sizes[a] - 1) if a == b else float(sizes[a]) * sizes[b]
        if P > 0 and inv_volume_sum > 0.0:
            g[s] = counts[s] / (P * shell * inv_volume_sum)
        if sizes[a] > 0 and frames > 0:
            coordination[s] = (2.0 if a == b else 1.0) * np.cumsum(counts[s]) / (float(sizes[a]) * frames)
    return g, coordination
