"""What the tabular tests share (TEST INFRASTRUCTURE): the numpy restatements of the file-4 and
law-9 bins, the oracle's tabular entries (oracle/c/file6.c) with their inputs, and the rigorous
enclosure of Legendre moments by bins.  Used by test_tabular_oracle.py (CPU) and
test_gpu_tabular.py (GPU)."""
import ctypes as C

import numpy as np
from numpy.polynomial import legendre as npleg

from conftest import OracleParams, dp, ip, oracle_params
from synth import kalbach_rows, law9_edata, mu_grid

# the scale-aware bar of the file-6 family against the Fortran (test_gpu_file6.py carries the same)
FILE6_TOL = 1e-10
# the bar of a restatement of bins, relative to the E_in's largest group P0
BIN_TOL = 1e-12

BINS5 = np.array([0.0, 1e-3, 0.1, 1.0, 5.0, 20.0])
BINS12 = np.concatenate([[0.0], np.logspace(-4, np.log10(20.0), 12)])
GROUPS = {5: BINS5, 12: BINS12}


def centres(n):
    return -1.0 + (2.0 * np.arange(n) + 1.0) / n


def edges(n):
    return -1.0 + 2.0 * np.arange(n + 1) / n


def p0_scale(p0):
    """per E_in: the largest group P0 (1 where the row is empty)"""
    s = np.abs(p0).max(axis=1)
    s[s == 0] = 1.0
    return s


def bin_err(got, ref, p0):
    """max |got - ref| over groups and bins, per E_in relative to its largest group P0; returns
    (worst, (E_in, group, bin) of the worst)"""
    e = np.abs(got - ref) / p0_scale(p0)[:, None, None]
    at = np.unravel_index(np.argmax(e), e.shape)
    return float(e[at]), tuple(int(x) for x in at)


# ---- file 4 ----------------------------------------------------------------------------------
def f4_lab(R, w):
    if R == 1.0:
        return np.sqrt(0.5 * (1.0 + w))
    return (1.0 + R * w) / np.sqrt(1.0 + R * R + 2.0 * R * w)


def f4_R(A, Q, E):
    return A * np.sqrt(1.0 + Q * (A + 1.0) / (A * E))


def file4_numpy(c, N, Q=0.0):
    """Independent restatement: the piecewise-linear f(w) of the trapezoid rule, cut at the grid
    points, at w = -R and at the CM cosines of every bin edge (roots of the kinematics' quadratic),
    each piece integrated exactly and given to the bin of its midpoint.  R = A sqrt(1 + Q (A + 1) /
    (A E)): A for elastic scattering, falling to 0 at the threshold of a level with Q < 0.  Returns
    the bins and, for the record, the plain trapezoid P0 in w of every (E_in, group)."""
    A, M = c["A"], c["f_tab"].shape[1]
    dmu = 2.0 / (M - 1)
    wg = -1.0 + np.arange(M) * dmu
    wg[-1] = 1.0
    eds = edges(N)
    out = np.zeros((len(c["ein"]), len(c["bins"]) - 1, N))
    p0 = np.zeros(out.shape[:2])
    for i, (E, r, fb) in enumerate(zip(c["ein"], c["row"], c["w"])):
        f = (1.0 - fb) * c["f_tab"][r] + fb * c["f_tab"][r + 1]
        R = f4_R(A, Q, E)
        for g in range(len(c["bins"]) - 1):
            wl = ((c["bins"][g] * (1 + A) ** 2 - E * (1 + R * R)) / (2 * R * E)).clip(-1, 1)
            wh = ((c["bins"][g + 1] * (1 + A) ** 2 - E * (1 + R * R)) / (2 * R * E)).clip(-1, 1)
            if wl == wh and abs(wl) == 1.0:
                continue
            grid = np.unique([wl, wh] + list(wg[(wg > wl) & (wg < wh)]))
            fg = np.interp(grid, wg, f)
            p0[i, g] = (0.5 * np.diff(grid) * (fg[1:] + fg[:-1])).sum()
            pts = list(grid)
            if R < 1.0 and wl < -R < wh:
                pts.append(-R)
            # s = sqrt(1 + R^2 + 2 R w) solves s^2 - 2 mu s + (1 - R^2) = 0
            for mu_e in eds:
                disc = mu_e * mu_e - 1.0 + R * R
                if disc < 0:
                    continue
                for s in (mu_e + np.sqrt(disc), mu_e - np.sqrt(disc)):
                    if s > 0:
                        we = (s * s - 1.0 - R * R) / (2.0 * R)
                        if wl < we < wh:
                            pts.append(we)
            pts = np.unique(pts)
            a, b = pts[:-1], pts[1:]
            fa, fbv = np.interp(a, wg, f), np.interp(b, wg, f)
            mass = 0.5 * (b - a) * (fa + fbv)
            k = np.clip(np.floor((f4_lab(R, 0.5 * (a + b)) + 1.0) * 0.5 * N).astype(int), 0, N - 1)
            np.add.at(out[i, g], k, mass)
    return out, p0


F4_LEVEL = dict(A=236.0058, Q=-0.0449)
F4_LEVEL_R = (0.05, 0.2, 0.5, 0.9, 0.999999, 1.000001, 1.5, 20.0)


def file4_level_case(M):
    """An inelastic level just above its threshold: E_in chosen so that R takes F4_LEVEL_R (both
    sides of R = 1, where the lab cosine of w < -R falls as w rises), and groups cut at E'(w) of
    w in {-1, -0.3, 0.4, 1} of every E_in plus 0 and 20 -- 33 groups, most of them narrower than a
    w panel at M <= 33.  Three table rows: two smooth ones and a sawtooth, on which a panel given
    to the wrong bin changes that bin visibly; every E_in blends two of them with w_hi = 0.3."""
    A, Q = F4_LEVEL["A"], F4_LEVEL["Q"]
    e_th = -Q * (A + 1.0) / A
    R = np.array(F4_LEVEL_R)
    ein = e_th / (1.0 - (R / A) ** 2)
    assert (np.diff(ein) > 0).all()
    Rf = f4_R(A, Q, ein)
    w = np.array([-1.0, -0.3, 0.4, 1.0])
    ep = ein[:, None] * (1.0 + Rf[:, None] ** 2 + 2.0 * Rf[:, None] * w[None, :]) / (1.0 + A) ** 2
    bins = np.unique(np.concatenate([[0.0, 20.0], ep.ravel()]))
    assert len(bins) == 34
    mu = mu_grid(M)
    saw = np.where(np.arange(M) % 2 == 0, 0.2, 1.0)
    f_tab = np.ascontiguousarray(np.stack([0.5 * (1.0 + 0.3 * mu + 0.2 * (1.5 * mu * mu - 0.5)),
                                           0.5 * (1.0 - 0.35 * mu + 0.1 * (1.5 * mu * mu - 0.5)),
                                           saw / (0.5 * np.diff(mu) * (saw[1:] + saw[:-1])).sum()]))
    row = (np.arange(len(ein)) % 2).astype(np.int32)
    return dict(A=A, Q=Q, R=Rf, f_tab=f_tab, ein=ein, row=row, w=np.full(len(ein), 0.3), bins=bins)


# ---- law 9 -----------------------------------------------------------------------------------
L9_ROWS = ((0.0, 0.0), (0.3, 0.1), (0.6, 0.3))       # the quadratic rows of the file6 golden


def law9_case(M):
    """The golden's law-9 case on a mu grid of M points: E_in = 0.4 lies below U = 0.5 (a zero row)
    and the upper groups lie above E_in - U for most of the others."""
    mu = mu_grid(M)
    f_tab = np.ascontiguousarray(np.stack([0.5 * (1 + a * mu + b * (1.5 * mu * mu - 0.5)) for a, b in L9_ROWS]))
    return dict(ein=np.array([0.4, 0.55, 0.8, 2.0, 7.5, 19.0]), row=np.array([0, 0, 0, 1, 1, 1], dtype=np.int32),
                w=np.array([0.1, 0.5, 0.9, 0.2, 0.6, 1.0]), f_tab=f_tab, edata=law9_edata(1e-3, 20.0),
                bins=np.concatenate([[0.0], np.logspace(-3, np.log10(20.0), 9)]))


def law9_numpy(f_tab, row, w, p0, N):
    """The blended row's exact bin integrals (np.interp, exact trapezoids between the union of the
    grid points and the bin edges), scaled by each group's P0: law 9's energy factor is common to
    both rows."""
    M = f_tab.shape[1]
    mu = mu_grid(M)
    x = np.unique(np.concatenate([mu, edges(N)]))
    out = np.zeros(p0.shape + (N,))
    for i, (r, ww) in enumerate(zip(row, w)):
        f = (1 - ww) * f_tab[r] + ww * f_tab[r + 1]
        fx = np.interp(x, mu, f)
        mass = 0.5 * np.diff(x) * (fx[1:] + fx[:-1])
        k = np.clip(np.floor((0.5 * (x[1:] + x[:-1]) + 1) * 0.5 * N).astype(int), 0, N - 1)
        frac = np.bincount(k, weights=mass, minlength=N)
        out[i] = p0[i][:, None] * (frac / frac.sum())[None, :]
    return out


# ---- file 6 ----------------------------------------------------------------------------------
def file6_case(M, intt, n_ein=5):
    """A Kalbach-Mann table on M cosines with duplicate end points, and n_ein incoming energies"""
    T = kalbach_rows(M, 4, 8, 18, 0.2, 20.0, seed=61 + intt, dup_last=True, intt=intt)
    rng = np.random.default_rng(3 + intt)
    ein = np.sort(rng.uniform(T["e_grid"][0], T["e_grid"][-1], n_ein))
    row = (np.searchsorted(T["e_grid"], ein, side="right") - 1).clip(0, 2).astype(np.int32)
    return T, ein, row


# ---- the oracle's entries --------------------------------------------------------------------
def bind_tab(oracle):
    PP, d, i = C.POINTER(OracleParams), C.c_double, C.c_int
    P, PI = C.POINTER(d), C.POINTER(i)
    oracle.oracle_file6_leg_batch.restype = i
    oracle.oracle_file6_leg_batch.argtypes = [PP, d, i, i, P, PI, i, P, PI, P, P, PI, P, i, P, P, i]
    oracle.oracle_file6_tab_batch.restype = i
    oracle.oracle_file6_tab_batch.argtypes = oracle.oracle_file6_leg_batch.argtypes + [i]
    oracle.oracle_law9_leg_batch.restype = i
    oracle.oracle_law9_leg_batch.argtypes = [PP, i, P, PI, P, i, P, P, i, P, P, i]
    oracle.oracle_law9_tab_batch.restype = i
    oracle.oracle_law9_tab_batch.argtypes = oracle.oracle_law9_leg_batch.argtypes + [i]
    return oracle


def oracle_file6(oracle, T, awr, frame_cm, ein, row, bins, n_tab=None, L=6, neg=10):
    """oracle_file6_tab_batch (n_tab bins) or, with n_tab None, oracle_file6_leg_batch (L orders)"""
    M = T["f"].shape[1]
    p = oracle_params(oracle, L, M)
    p.ne_per_grp = neg
    ein, bins = np.ascontiguousarray(ein, dtype=np.float64), np.ascontiguousarray(bins, dtype=np.float64)
    row = np.ascontiguousarray(row, dtype=np.int32)
    G = len(bins) - 1
    out = np.zeros((len(ein), G, L if n_tab is None else n_tab))
    args = (C.byref(p), awr, frame_cm, len(ein), dp(ein), ip(row), len(T["e_grid"]), dp(T["e_grid"]),
            ip(T["row_ptr"]), dp(T["eout"]), dp(T["pdf"]), ip(T["intt"]), dp(T["f"]), G, dp(bins), dp(out), 0)
    rc = oracle.oracle_file6_leg_batch(*args) if n_tab is None else oracle.oracle_file6_tab_batch(*args, n_tab)
    assert rc == 0
    return out


def oracle_law9(oracle, c, n_tab=None, L=6):
    M = c["f_tab"].shape[1]
    p = oracle_params(oracle, L, M)
    G = len(c["bins"]) - 1
    out = np.zeros((len(c["ein"]), G, L if n_tab is None else n_tab))
    arrs = [np.ascontiguousarray(c[k], dtype=np.float64) for k in ("ein", "w", "f_tab", "edata", "bins")]
    row = np.ascontiguousarray(c["row"], dtype=np.int32)
    args = (C.byref(p), len(arrs[0]), dp(arrs[0]), ip(row), dp(arrs[1]), arrs[2].shape[0], dp(arrs[2]),
            dp(arrs[3]), G, dp(arrs[4]), dp(out), 0)
    rc = oracle.oracle_law9_leg_batch(*args) if n_tab is None else oracle.oracle_law9_tab_batch(*args, n_tab)
    assert rc == 0
    return out


# ---- bins against moments --------------------------------------------------------------------
_EXTREMES = {}


def legendre_bin_extremes(N, lmax=5):
    """min and max of P_l (l = 0 .. lmax) on each of N equal bins, exactly: P_l at the two edges and
    at the roots of P_l' inside the bin.  Returns (pmin, pmax), each [lmax + 1][N]."""
    if (N, lmax) not in _EXTREMES:
        e = edges(N)
        pmin, pmax = np.zeros((lmax + 1, N)), np.zeros((lmax + 1, N))
        for l in range(lmax + 1):
            P = npleg.Legendre.basis(l)
            crit = np.real(P.deriv().roots()) if l >= 2 else np.zeros(0)
            for k in range(N):
                x = np.concatenate([e[k:k + 2], crit[(crit > e[k]) & (crit < e[k + 1])]])
                v = P(x)
                pmin[l, k], pmax[l, k] = v.min(), v.max()
        _EXTREMES[(N, lmax)] = (pmin, pmax)
    return _EXTREMES[(N, lmax)]


def enclosure_violation(tab, leg, lmax=5):
    """For T >= 0 the bins enclose every Legendre moment of the same density:
        sum_k T_k min_bin P_l  <=  a_l  <=  sum_k T_k max_bin P_l.
    Returns the largest violation over l = 1 .. lmax, relative to the E_in's largest |moment|
    (0 where every moment is enclosed)."""
    N = tab.shape[2]
    pmin, pmax = legendre_bin_extremes(N, lmax)
    lo = np.einsum("egk,lk->egl", tab, pmin)[:, :, 1:]
    hi = np.einsum("egk,lk->egl", tab, pmax)[:, :, 1:]
    a = leg[:, :, 1:lmax + 1]
    scale = np.abs(leg).reshape(leg.shape[0], -1).max(axis=1)
    scale[scale == 0] = 1.0
    viol = np.maximum(np.maximum(lo - a, a - hi), 0.0) / scale[:, None, None]
    return float(viol.max())
