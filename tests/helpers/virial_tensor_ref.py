"""Host yardstick of the per-atom virial tensor (include/emdee_hip.h: emdee_compute_virial_tensor):

    W_i^ab = 1/2 sum_j (-E'r / r^2) d^a d^b,   d = r_i - r_j the minimum image,

in the order (xx, yy, zz, xy, xz, yz), so that the trace of W_i is the per-atom virial w_i.  Pairs come from the oracle's
neighbour list in cubic periodic boxes and from a numpy brute force otherwise; the pair function is a vectorised numpy
restatement of oracle.interaction in CUTOFF mode (the golden generator's formula, tests/golden/make_golden.py).  Excluded
pairs and 1-4 pairs are left out and the 1-4 pairs come back lj14scale times -- the rule _pair_terms of
tests/test_gpu_dd_pairs.py applies to f, e and w."""
import numpy as np

COMPONENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def pair_energy_virial(r2, rc, rs, hs_i, te_i, hs_j, te_j):
    """(E, W) of oracle.interaction(r2, model(rc, rs), (hs_i, te_i), (hs_j, te_j), mode=CUTOFF), vectorised, fp64.
    hs / te: LJAtom fields (half sigma, twice sqrt eps), float32 values."""
    r2 = np.asarray(r2, dtype=np.float64)
    rc2, rs2 = rc * rc, rs * rs
    idl2 = 1.0 / (rc2 - rs2)
    sigma = np.asarray(hs_i, np.float32).astype(np.float64) + np.asarray(hs_j, np.float32).astype(np.float64)
    e4 = np.asarray(te_i, np.float32).astype(np.float64) * np.asarray(te_j, np.float32).astype(np.float64)
    s2 = sigma * sigma / r2
    s6 = s2 * s2 * s2
    e4s6 = e4 * s6
    E = e4s6 * (s6 - 1.0)
    W = 6.0 * e4s6 * (2.0 * s6 - 1.0)
    x = (r2 - rs2) * idl2
    x = np.where((x > 0.0) & (x < 1.0), x, 0.0)
    g = 1.0 + x ** 3 * (15.0 * x - 6.0 * x * x - 10.0)
    mgr = 60.0 * x * x * (1.0 - 2.0 * x + x * x) * idl2 * r2
    inside = r2 < rc2
    return np.where(inside, E * g, 0.0), np.where(inside, W * g + E * mgr, 0.0)


def _minimum_image(d, lengths, periodic):
    for a in range(3):
        if periodic[a]:
            d[:, a] -= lengths[a] * np.rint(d[:, a] / lengths[a])
    return d


def pairs_in_range(pos, lengths, periodic, rc, oracle=None, rows=None, margin=0.1):
    """(i, j, d) of every pair i < j with |d| < rc + margin (d = minimum image of r_i - r_j on the periodic axes).
    rows: the sampled mode for boxes too large for the N^2 sum -- i runs over these atoms only and j over every other
    atom, so that each listed row is whole (O(len(rows) N))."""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    cubic = all(periodic) and lengths[0] == lengths[1] == lengths[2]
    rl = rc + margin
    if rows is not None:
        out = []
        for r in np.asarray(rows, dtype=np.int64):
            d = _minimum_image(pos[r] - pos, lengths, periodic)
            j = np.nonzero(np.einsum("ij,ij->i", d, d) < rl * rl)[0]
            j = j[j != r]
            out.append((np.full(j.shape[0], r), j, d[j]))
        return tuple(np.concatenate([o[k] for o in out]) for k in range(3))
    if cubic and oracle is not None and rl <= 0.5 * lengths[0]:
        off, nb = oracle.neighbor_list(pos, lengths[0], rl)
        i = np.repeat(np.arange(N), np.diff(off))
        j = nb.astype(np.int64)
        keep = i < j
        i, j = i[keep], j[keep]
    else:
        i, j = np.triu_indices(N, 1)
    d = _minimum_image(pos[i] - pos[j], lengths, periodic)
    keep = np.einsum("ij,ij->i", d, d) < rl * rl
    return i[keep], j[keep], d[keep]


def _pair_key(i, j, N):
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return lo.astype(np.int64) * N + hi


def per_atom_tensor(pos, lengths, periodic, rc, rs, hs, te, excl=None, p14=None, lj14scale=1.0, oracle=None):
    """(N, 6) per-atom virial tensors, and (N,) per-atom virials w, in fp64."""
    N = pos.shape[0]
    i, j, d = pairs_in_range(pos, lengths, periodic, rc, oracle)
    r2 = np.einsum("ij,ij->i", d, d)
    _, W = pair_energy_virial(r2, rc, rs, hs[i], te[i], hs[j], te[j])
    scale = np.ones(i.shape[0])
    key = _pair_key(i, j, N)
    named = []
    if excl is not None and len(excl):
        named.append(_pair_key(np.asarray(excl)[:, 0], np.asarray(excl)[:, 1], N))
    if p14 is not None and len(p14):
        k14 = _pair_key(np.asarray(p14)[:, 0], np.asarray(p14)[:, 1], N)
        named.append(k14)
        scale[np.isin(key, np.concatenate(named))] = 0.0
        scale[np.isin(key, k14)] = lj14scale
    elif named:
        scale[np.isin(key, np.concatenate(named))] = 0.0
    wr2 = 0.5 * scale * W / r2
    t = np.zeros((N, 6))
    for c, (a, b) in enumerate(COMPONENTS):
        h = wr2 * d[:, a] * d[:, b]
        t[:, c] = np.bincount(i, h, minlength=N) + np.bincount(j, h, minlength=N)
    w = np.bincount(i, 0.5 * scale * W, minlength=N) + np.bincount(j, 0.5 * scale * W, minlength=N)
    return t, w


def trace(t):
    return t[:, 0] + t[:, 1] + t[:, 2]


def matrix(six):
    xx, yy, zz, xy, xz, yz = six
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
