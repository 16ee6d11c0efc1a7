"""numpy reference of the spatial profiles (include/emdee_hip.h: emdee_md_set_spatial): the bin rules in the two-rounding form the
kernels use, the ten words per (group, bin), and what the tests' bounds need -- per word the sum of the absolute values of the
elementary products behind each bin, and the number of atoms within delta of every bin edge."""
import numpy as np

WORDS = 10
DENSITY, KINETIC, STRESS = 1, 2, 4
X, Y, Z, RADIAL = 0, 1, 2, 3


def planar(axis, n_bins, lo, length=None, range=None):
    """a planar geometry: periodic with the box's lo and length along the axis, or open with range = (r0, r1)"""
    if range is None:
        return dict(kind=int(axis), n_bins=int(n_bins), periodic=True, lo=float(lo), inv_width=float(n_bins) / float(length),
                    width=float(length) / n_bins)
    r0, r1 = float(range[0]), float(range[1])
    return dict(kind=int(axis), n_bins=int(n_bins), periodic=False, lo=r0, inv_width=float(n_bins) / (r1 - r0), width=(r1 - r0) / n_bins)


def radial(n_bins, r_max, centre, lengths, periodic):
    """shells around centre; lengths / periodic: the box, three each (the minimum image is taken on the periodic axes only)"""
    ln = np.array([float(l) if p else 0.0 for l, p in zip(lengths, periodic)])
    with np.errstate(divide="ignore"):
        inv = np.where(ln != 0.0, 1.0 / np.where(ln != 0.0, ln, 1.0), 0.0)
    return dict(kind=RADIAL, n_bins=int(n_bins), r_max=float(r_max), inv_dr=float(n_bins) / float(r_max), centre=np.array(centre, dtype=np.float64),
                len=ln, inv_len=inv, width=float(r_max) / n_bins)


def bins_planar(x, geom):
    """the bin of every coordinate, -1 outside an open range: the difference and the product are two roundings, then floor"""
    d = np.asarray(x, dtype=np.float64) - geom["lo"]
    s = d * geom["inv_width"]
    f = np.floor(s)
    if geom["periodic"]:
        return np.mod(f.astype(np.int64), geom["n_bins"]).astype(np.int64), s
    ok = (f >= 0.0) & (f < geom["n_bins"])
    return np.where(ok, f, -1.0).astype(np.int64), s


def image(pos, geom):
    d = np.asarray(pos, dtype=np.float64) - geom["centre"][None, :]
    q = d * geom["inv_len"][None, :]
    s = np.rint(q) * geom["len"][None, :]
    return d - s


def bins_radial(pos, geom):
    """(bin or -1, r, d, s = r inv_dr) of every position"""
    d = image(pos, geom)
    p = d * d
    r = np.sqrt((p[:, 0] + p[:, 1]) + p[:, 2])
    s = r * geom["inv_dr"]
    k = s.astype(np.int64)
    ok = (r < geom["r_max"]) & (k < geom["n_bins"])
    return np.where(ok, k, -1), r, d, s


def near_edges(s, geom, delta):
    """per edge 0 ... n_bins: the atoms whose s (in bin widths) lies within delta (a coordinate) of it; on a periodic axis edge n_bins
    is edge 0 and both entries hold the count.  The centre of the radial geometry is no edge."""
    n_bins = geom["n_bins"]
    tol = delta * (geom["inv_dr"] if geom["kind"] == RADIAL else geom["inv_width"])
    j = np.rint(s)
    close = np.abs(s - j) <= tol
    near = np.zeros(n_bins + 1, dtype=np.int64)
    j = j.astype(np.int64)
    if geom["kind"] != RADIAL and geom["periodic"]:
        np.add.at(near, np.mod(j[close], n_bins), 1)
        near[n_bins] = near[0]
    else:
        ok = close & (j >= (1 if geom["kind"] == RADIAL else 0)) & (j <= n_bins)
        np.add.at(near, j[ok], 1)
    return near


def profile(pos, vel, masses, charges, energies, tensors, groups, n_groups, geom, what=7, delta=0.0):
    """pos: unwrapped positions (N, 3); vel (N, 3) or None; masses (N,) (0: a massless atom); charges (N,) or None; energies (N,) and
    tensors (N, 6: xx, yy, zz, xy, xz, yz) or None; groups (N,) in -1 ... n_groups - 1 or None (every atom in group 0).
    -> dict: counts (n_groups, n_bins), words (n_groups, n_bins, 10), outside (n_groups,), absum (like words: the sum of the absolute
    elementary products behind each word), near (n_bins + 1: the grouped atoms within delta of each edge), bins (N,), grouped (N,)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    groups = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    m = np.asarray(masses, dtype=np.float64) * np.ones(n)
    q = np.zeros(n) if charges is None else np.asarray(charges, dtype=np.float64)
    v = np.zeros((n, 3)) if vel is None else np.asarray(vel, dtype=np.float64)
    e = np.zeros(n) if energies is None else np.asarray(energies, dtype=np.float64)
    w = np.zeros((n, 6)) if tensors is None else np.asarray(tensors, dtype=np.float64)
    n_bins = geom["n_bins"]
    no_normal = np.zeros(n, dtype=bool)
    if geom["kind"] == RADIAL:
        bins, r, d, s = bins_radial(pos, geom)
        no_normal = ~(r > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            nrm = np.where(no_normal[:, None], 0.0, d / np.where(no_normal, 1.0, r)[:, None])
    else:
        bins, s = bins_planar(pos[:, geom["kind"]], geom)
        nrm = np.zeros((n, 3))
        nrm[:, geom["kind"]] = 1.0
    words, absum = np.zeros((n, WORDS)), np.zeros((n, WORDS))
    if what & DENSITY:
        words[:, 0], absum[:, 0] = m, np.abs(m)
        words[:, 1], absum[:, 1] = q, np.abs(q)
    if what & KINETIC:
        words[:, 2:5] = m[:, None] * v
        absum[:, 2:5] = np.abs(words[:, 2:5])
        words[:, 5] = m * (v * v).sum(axis=1)
        absum[:, 5] = np.abs(words[:, 5])
        vn = (v * nrm).sum(axis=1)
        words[:, 6] = np.where(no_normal, words[:, 5] / 3.0, m * vn * vn)
        absum[:, 6] = np.where(no_normal, absum[:, 5] / 3.0, np.abs(m) * np.abs(v * nrm).sum(axis=1) ** 2)
    if what & STRESS:
        words[:, 7], absum[:, 7] = e, np.abs(e)
        words[:, 8], absum[:, 8] = w[:, 0:3].sum(axis=1), np.abs(w[:, 0:3]).sum(axis=1)
        full = np.stack([np.stack([w[:, 0], w[:, 3], w[:, 4]], axis=1), np.stack([w[:, 3], w[:, 1], w[:, 5]], axis=1),
                         np.stack([w[:, 4], w[:, 5], w[:, 2]], axis=1)], axis=1)
        terms = nrm[:, :, None] * full * nrm[:, None, :]
        words[:, 9] = np.where(no_normal, words[:, 8] / 3.0, terms.sum(axis=(1, 2)))
        absum[:, 9] = np.where(no_normal, absum[:, 8] / 3.0, np.abs(terms).sum(axis=(1, 2)))
    grouped = groups >= 0
    inside = grouped & (bins >= 0)
    counts = np.zeros((n_groups, n_bins), dtype=np.int64)
    np.add.at(counts, (groups[inside], bins[inside]), 1)
    outside = np.zeros(n_groups, dtype=np.int64)
    np.add.at(outside, groups[grouped & (bins < 0)], 1)
    tot, tot_abs = np.zeros((n_groups, n_bins, WORDS)), np.zeros((n_groups, n_bins, WORDS))
    np.add.at(tot, (groups[inside], bins[inside]), words[inside])
    np.add.at(tot_abs, (groups[inside], bins[inside]), absum[inside])
    return dict(counts=counts, words=tot, outside=outside, absum=tot_abs, near=near_edges(s[grouped], geom, delta), bins=bins,
                grouped=grouped)


def bound(counts, absum):
    """|dev - ref| <= 2 (n_k + 16) 2^-53 A_k: the summation order, and the few roundings in forming an addend"""
    return 2.0 * (np.asarray(counts, dtype=np.float64)[..., None] + 16.0) * 2.0 ** -53 * absum
