"""Host yardstick of pressure coupling (include/emdee_hip.h: emdee_md_scale_box, emdee_md_set_barostat).  Plain numpy fp64; it
never calls the library.  Built on tests/helpers/ortho_ref.py: the force field is a callable around ortho_ref.total, the
integrator is ortho_ref.verlet's velocity Verlet with a coupling event after every `every`-th step.

    P^aa  = (K^aa + W^aa) / V,  K^aa = sum_i m_i v_i^a v_i^a,  W^aa = sum_i W_i^aa        (emdee_md_pressure_tensor)
    isotropic       P = (Pxx + Pyy + Pzz) / 3 for all three axes, entry 0 of p_ref and compressibility
    semi-isotropic  (Pxx + Pyy) / 2 for x and y with entry 0, Pzz for z with entry 2
    anisotropic     Pxx, Pyy, Pzz with their own entries
    Berendsen       mu_d = 1 - (Dt / (3 tau_p)) beta_d (P_ref,d - P_d),  velocity scale 1,  Dt = every dt
    C-rescale       d_eps = -(beta / tau_p) (P_ref - P) Dt + sqrt(2 T beta Dt / (V tau_p)) xi,  mu = exp(d_eps / 3) on all three
                    axes, velocity scale 1 / mu (isotropic only)
    scale           x_d <- lo_d + mu_d (x_d - lo_d),  len_d <- mu_d len_d,  v <- velocity scale x v
"""
import numpy as np

BERENDSEN, CRESCALE = 1, 2
ISOTROPIC, SEMIISOTROPIC, ANISOTROPIC = 0, 1, 2
_ENTRY = {ISOTROPIC: (0, 0, 0), SEMIISOTROPIC: (0, 0, 2), ANISOTROPIC: (0, 1, 2)}


def coupled_pressure(P, coupling):
    """the pressure each axis couples to, from the diagonal (Pxx, Pyy, Pzz)"""
    P = np.asarray(P, dtype=np.float64)
    if coupling == ISOTROPIC:
        return np.full(3, P.sum() / 3.0)
    if coupling == SEMIISOTROPIC:
        return np.array([0.5 * (P[0] + P[1]), 0.5 * (P[0] + P[1]), P[2]])
    return P.copy()


def berendsen_mu(P, p_ref, beta, tau_p, Dt, coupling=ISOTROPIC):
    """mu[3] from the diagonal of the instantaneous pressure tensor"""
    Pc = coupled_pressure(P, coupling)
    k = list(_ENTRY[coupling])
    p_ref, beta = np.asarray(p_ref, dtype=np.float64)[k], np.asarray(beta, dtype=np.float64)[k]
    return 1.0 - (Dt / (3.0 * tau_p)) * beta * (p_ref - Pc)


def crescale_mu(P, p_ref, beta, tau_p, Dt, temperature, volume, xi):
    """(mu[3], velocity scale) of stochastic cell rescaling; P the diagonal, p_ref and beta scalars, xi one N(0, 1) number"""
    Pi = float(np.sum(P)) / 3.0
    de = -(beta / tau_p) * (p_ref - Pi) * Dt + np.sqrt(2.0 * temperature * beta * Dt / (volume * tau_p)) * xi
    mu = np.exp(de / 3.0)
    return np.full(3, mu), 1.0 / mu


def scale(pos, lo, lengths, mu):
    """(positions, lengths) after the scale: [lo, lo + len) goes onto [lo, lo + mu len)"""
    lo, mu = np.asarray(lo, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    return lo + mu * (np.asarray(pos, dtype=np.float64) - lo), mu * np.asarray(lengths, dtype=np.float64)


def pressure_diagonal(vel, tensors, lengths, inv_mass=None):
    """(Pxx, Pyy, Pzz) = (K + W) / V from the velocities and the per-atom virial tensors (N, 6) of ortho_ref.total"""
    m = 1.0 if inv_mass is None else 1.0 / np.asarray(inv_mass, dtype=np.float64)[:, None]
    K = (m * vel * vel).sum(axis=0)
    W = np.asarray(tensors)[:, :3].sum(axis=0)
    return (K + W) / float(np.prod(lengths))


def coupled_verlet(pos, vel, lo, lengths, total, nsteps, dt, kind, p_ref, beta, tau_p, every, coupling=ISOTROPIC,
                   temperature=None, xi=None, first_step=0, inv_mass=None):
    """Velocity Verlet with a coupling event after every step that brings the count (from first_step) to a multiple of
    `every`.  total(x, lengths) -> the dict of ortho_ref.total on that box.  xi(s): the event's N(0, 1) number (C-rescale).
    Returns (x, v, lengths, events), events = [(s, P diagonal, mu, velocity scale)]; positions are left unwrapped."""
    x, v = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    ln = np.array(lengths, dtype=np.float64)
    im = 1.0 if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)[:, None]
    out = total(x, ln)
    s, events = int(first_step), []
    for _ in range(nsteps):
        v += 0.5 * dt * im * out["f"]
        x += dt * v
        out = total(x, ln)
        v += 0.5 * dt * im * out["f"]
        s += 1
        if s % every:
            continue
        P = pressure_diagonal(v, out["t"], ln, inv_mass)
        if kind == BERENDSEN:
            mu, vs = berendsen_mu(P, p_ref, beta, tau_p, every * dt, coupling), 1.0
        else:
            assert coupling == ISOTROPIC
            mu, vs = crescale_mu(P, np.ravel(p_ref)[0], np.ravel(beta)[0], tau_p, every * dt, temperature, float(np.prod(ln)), xi(s))
        x, ln = scale(x, lo, ln, mu)
        v *= vs
        out = total(x, ln)
        events.append((s, P, mu, vs))
    return x, v, ln, events


# ---------------------------------------------------------------- the box the coupling tests share
RC, RS, SKIN, DT = 2.5, 2.0, 0.3, 0.004
_CACHE = {}


def lj_atoms(N):
    """N identical LJAtom records (sigma = eps = 1) in the library's layout"""
    a = np.zeros(N, dtype=np.dtype([("half_sigma", np.float32), ("twice_sqrt_eps", np.float32)]))
    a["half_sigma"], a["twice_sqrt_eps"] = 0.5, 2.0
    return a


def field(atoms, lo=(0.0, 0.0, 0.0), periodic=(1, 1, 1), rc=RC, rs=RS, **kw):
    """total(x, lengths) of coupled_verlet for a box of these atoms"""
    from . import ortho_ref as oref
    return lambda x, lengths: oref.total(x, np.asarray(lo, dtype=np.float64), np.asarray(lengths, dtype=np.float64), list(periodic),
                                         rc, rs, atoms, **kw)


def fluid864(syn, melt=30):
    """The 864-atom fluid of the bonded and orthorhombic tests (6^3 jittered fcc cells at rho* = 0.8, L = 10.26 sigma: three
    cells of rc + skin = 2.8 per side) after a short melt at T* = 1.4 on the host, so that no force vanishes by symmetry.
    Returns dict(pos (wrapped), vel, L, atoms); computed once per process."""
    if "fluid" not in _CACHE:
        from . import ortho_ref as oref
        pos, L = syn.fcc_positions(6)
        N = pos.shape[0]
        atoms = lj_atoms(N)
        vel = syn.velocities(N, temperature=1.4)
        f = field(atoms)
        x, v = oref.verlet(pos, vel, lambda q: f(q, [L] * 3)["f"], melt, DT)
        _CACHE["fluid"] = dict(pos=np.mod(x, L), vel=v, L=float(L), atoms=atoms)
    d = _CACHE["fluid"]
    return dict(pos=d["pos"].copy(), vel=d["vel"].copy(), L=d["L"], atoms=d["atoms"].copy())


def berendsen_case(syn, coupling, nsteps=40, every=5):
    """The Berendsen trajectory the GPU tests compare with, once per coupling: p_ref sits 20 (and 12, 28 on the other axes)
    above the starting pressure of about -0.3, compressibilities near 0.02 and tau_p = 1, so that every event shrinks the box by 1e-3 to
    1e-2 per side and the side stays above 3 x 2.8.  Returns dict(x, v, lengths, events, p_ref, beta, tau_p, every)."""
    key = ("berendsen", coupling, nsteps, every)
    if key not in _CACHE:
        S = fluid864(syn)
        tot = field(S["atoms"])
        P0 = pressure_diagonal(S["vel"], tot(S["pos"], [S["L"]] * 3)["t"], [S["L"]] * 3).mean()
        p_ref = np.round(P0) + np.array([20.0, 12.0, 28.0])
        beta, tau_p = np.array([0.02, 0.025, 0.015]), 1.0
        x, v, ln, ev = coupled_verlet(S["pos"], S["vel"], np.zeros(3), [S["L"]] * 3, tot, nsteps, DT, BERENDSEN, p_ref, beta, tau_p,
                                      every, coupling)
        _CACHE[key] = dict(x=x, v=v, lengths=ln, events=ev, p_ref=p_ref, beta=beta, tau_p=tau_p, every=every)
    return _CACHE[key]
