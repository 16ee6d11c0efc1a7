"""numpy reference of the displacement and velocity correlations (include/emdee_hip.h: emdee_md_set_msd) over the frames a test took
with md.state() at every sample: a plain double loop over the pairs of frames, written from the definition, not from the engine's
schedule.  Beside every word it returns A, the same sum over the absolute values of the addends, which the tolerances of
tests/test_gpu_msd.py are relative to, and what the Float32 bounds need."""
import numpy as np

WORDS = 7


def correlate(xs, vs, n_lags, origin_every, groups=None, n_groups=1, msd=True, vacf=True):
    """xs, vs: per sample the (N, 3) float64 unwrapped positions and the velocities.  Every pair of samples (s_o, s) with
    s_o % origin_every == 0 and 0 <= s - s_o < n_lags contributes to lag s - s_o.  Returns a dict:
      sums (n_lags, n_groups, 7); A (same shape): for w0-2 the sums themselves, for w3-5 sum over origins of (sum_i |d_i|)^2, for
      w6 sum |v_c v0_c|;  origins (n_lags,);  sizes (n_groups,);
      abs_d (n_lags, n_groups, 3): sum over origins and atoms of |d_i|;  abs_s1 (same): sum over origins of |sum_i d_i|."""
    n = len(xs[0])
    groups = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups)
    members = [np.nonzero(groups == g)[0] for g in range(n_groups)]
    out = {k: np.zeros((n_lags, n_groups, WORDS)) for k in ("sums", "A")}
    out["abs_d"], out["abs_s1"] = np.zeros((n_lags, n_groups, 3)), np.zeros((n_lags, n_groups, 3))
    out["origins"] = np.zeros(n_lags, dtype=np.int64)
    out["sizes"] = np.array([len(m) for m in members], dtype=np.int64)
    for s in range(len(xs)):
        for so in range(0, s + 1):
            lag = s - so
            if so % origin_every != 0 or lag >= n_lags:
                continue
            out["origins"][lag] += 1
            for g, idx in enumerate(members):
                if msd:
                    d = xs[s][idx] - xs[so][idx]
                    s1, a1 = d.sum(axis=0), np.abs(d).sum(axis=0)
                    out["sums"][lag, g, 0:3] += (d * d).sum(axis=0)
                    out["A"][lag, g, 0:3] += (d * d).sum(axis=0)
                    out["sums"][lag, g, 3:6] += s1 * s1
                    out["A"][lag, g, 3:6] += a1 * a1
                    out["abs_d"][lag, g] += a1
                    out["abs_s1"][lag, g] += np.abs(s1)
                if vacf:
                    vv = vs[s][idx] * vs[so][idx]
                    out["sums"][lag, g, 6] += vv.sum()
                    out["A"][lag, g, 6] += np.abs(vv).sum()
    return out


def bound64(ref):
    """what an fp64 engine may differ by, per word: its inputs are bitwise the reference's, only the order of summation and the
    contraction of a multiply-add differ.  Any order of n additions is within (n - 1) 2^-53 of the exact sum relative to the sum of
    the absolute addends A, to first order; n = N_g atoms, then the origins of the lag; a factor 8 for contraction and numpy's own
    rounding: 2^-50 (N_g + origins + 8) A.  Twice that for w3-5, the square of a sum."""
    n = ref["sizes"][None, :, None] + ref["origins"][:, None, None] + 8.0
    b = 2.0 ** -50 * n * ref["A"]
    b[..., 3:6] *= 2.0
    return b


def bound32(ref, x_max):
    """a Float32 engine: the device takes unrounded doubles where state() rounds to fp32, so a displacement differs by at most
    delta = 2 x 2^-24 x_max.  w0-2: + sum (2 |d_i| delta + delta^2); w3-5: + 2 |S1| N_g delta + N_g^2 delta^2 per origin; w6: the
    fp64 bound alone (fp32 velocities are exact in double)."""
    delta = 2.0 * 2.0 ** -24 * x_max
    b = bound64(ref)
    ng, no = ref["sizes"][None, :, None].astype(np.float64), ref["origins"][:, None, None].astype(np.float64)
    b[..., 0:3] += 2.0 * ref["abs_d"] * delta + no * ng * delta * delta
    b[..., 3:6] += 2.0 * ref["abs_s1"] * ng * delta + no * ng * ng * delta * delta
    return b


def drift_free(sums, origins, sizes):
    """(n_lags, n_groups): (w0 + w1 + w2 - (w3 + w4 + w5) / N_g) / (origins N_g); NaN where origins N_g == 0"""
    ng = np.asarray(sizes, dtype=np.float64)[None, :]
    count = np.asarray(origins, dtype=np.float64)[:, None] * ng
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count > 0, (sums[..., 0:3].sum(axis=2) - sums[..., 3:6].sum(axis=2) / ng) / count, np.nan)
