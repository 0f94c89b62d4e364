"""TEST INFRASTRUCTURE: host restatements of ndpp_nbody_leg_batch (include/ndpp_hip.h: ACE law 66,
N-body phase space).

nbody_numpy      the definition, operation by operation in float64 and in its sum order, with the
                 library's own 32 nodes and weights (ndpp_nbody_rule): the same bits as the kernel.
nbody_converged  the same scheme -- outer variable t, breakpoints, inner variable sqrt(E') -- with a
                 96 x 96 rule: what the 32 x 32 rule is measured against.
nbody_cm_check   the same outer variable and breakpoints, but the inner integral over the CM cosine
                 at 64 x 64 and the lab cosine from the CM one: another route to the same numbers
                 (it converges algebraically, so it is a cross-check and nothing else).
All return out[n_ein][G][L]; nbody_numpy also the status words."""
from __future__ import annotations

import numpy as np

TWO_OVER_B = {3: 5.0929581789406507, 4: 13.125, 5: 23.282094532300118}     # 16/pi, 105/8, 512/(7 pi)
ST_RANGE = 2


def _setup(awr, Q, Ap, E):
    Emax = ((Ap - 1.0) / Ap) * ((awr / (awr + 1.0)) * E + Q)
    E0 = E / ((awr + 1.0) * (awr + 1.0))
    return Emax, E0


def _window_hit(Emax, rE0, lo, hi):
    rEm = np.sqrt(Emax)
    wd = rE0 - rEm
    wl = wd if wd > 0.0 else 0.0
    wh = rEm + rE0
    return bool(hi > wl * wl and lo < wh * wh)


def _points(Emax, rE0, rlo, rhi):
    """0, the kept breakpoints and 1: sorted, equal values once"""
    pts = {0.0, 1.0}
    for d in (rlo - rE0, rlo + rE0, rhi - rE0, rhi + rE0):
        Tb = d * d
        if Tb > 0.0 and Tb < Emax:
            sg = np.sqrt(Tb / Emax)
            pts.add(float(sg / (1.0 + np.sqrt(1.0 - sg * sg))))
    return sorted(pts)


def _outer(n, Emax, pa, pb, x, w):
    """the outer nodes of the piece [pa, pb]: T, and wt * W"""
    hm, cm = 0.5 * (pb - pa), 0.5 * (pb + pa)
    t = cm + hm * x
    wt = hm * w
    q = 1.0 + t * t
    s = (2.0 * t) / q
    c = (1.0 - t * t) / q
    s2 = s * s
    T = Emax * s2
    c2 = c * c
    c4 = c2 * c2
    cp = c2 if n == 3 else (c4 * c if n == 4 else c4 * c4)
    W = ((TWO_OVER_B[n] * s2) * cp) * (2.0 / q)
    return T, wt * W


def _legendre_terms(mu, L):
    """P_0 .. P_{L-1} at mu by the recurrence of the kernels (the quotients rounded once)"""
    P = [np.ones_like(mu), mu]
    for l in range(1, L - 1):
        P.append(((float(2 * l + 1) / float(l + 1)) * mu) * P[l] - (float(l) / float(l + 1)) * P[l - 1])
    return P[:L]


def nbody_numpy(awr, Q, n, Ap, ein, e_bins, L, rule=None):
    """(out, status) of ndpp_nbody_leg_batch, bit for bit.  rule: (x, w), default the library's."""
    if rule is None:
        from ndpp_amd import lib
        rule = lib.nbody_rule()
    x, w = (np.asarray(a, dtype=np.float64) for a in rule)
    N = len(x)
    ein, e_bins = np.asarray(ein, dtype=np.float64), np.asarray(e_bins, dtype=np.float64)
    G = len(e_bins) - 1
    out, status = np.zeros((len(ein), G, L)), np.zeros(len(ein), dtype=np.int32)
    with np.errstate(all="ignore"):
        for e, E in enumerate(ein):
            if not (E > 0.0) or not (E <= np.finfo(np.float64).max):
                status[e] = ST_RANGE
                continue
            Emax, E0 = _setup(awr, Q, Ap, E)
            if not (Emax > 0.0):
                continue
            rE0 = np.sqrt(E0)
            for g in range(G):
                lo, hi = e_bins[g], e_bins[g + 1]
                if not _window_hit(Emax, rE0, lo, hi):
                    continue
                rlo, rhi = np.sqrt(lo), np.sqrt(hi)
                pts = _points(Emax, rE0, rlo, rhi)
                total = np.zeros(L)
                for pa, pb in zip(pts[:-1], pts[1:]):
                    T, ww = _outer(n, Emax, pa, pb, x, w)          # [N] outer nodes
                    rT = np.sqrt(T)
                    ia = np.maximum(np.abs(rT - rE0), rlo)
                    ib = np.minimum(rT + rE0, rhi)
                    on = ib > ia
                    hm2, cm2 = 0.5 * (ib - ia), 0.5 * (ib + ia)
                    den = (2.0 * rT) * rE0
                    I = np.zeros((L, N))
                    for k in range(N):                              # the inner nodes, ascending
                        sp = cm2 + hm2 * x[k]
                        fk = (hm2 * w[k]) * (sp / den)
                        mu = ((sp - rT) * (sp + rT)) / ((2.0 * sp) * rE0) + rE0 / (2.0 * sp)
                        mu = np.where(mu < -1.0, -1.0, mu)
                        mu = np.where(mu > 1.0, 1.0, mu)
                        for l, P in enumerate(_legendre_terms(mu, max(L, 2))[:L]):
                            I[l] = I[l] + fk * P
                    I[:, ~on] = 0.0
                    v = ww * I                                       # [L][N]
                    piece = np.zeros(L)
                    for j in range(N):                              # the outer nodes, ascending
                        piece = piece + v[:, j]
                    total = total + piece
                out[e, g] = total
    return out, status


def _fine(awr, Q, n, Ap, ein, e_bins, L, order, inner):
    x, w = np.polynomial.legendre.leggauss(order)
    ein, e_bins = np.asarray(ein, dtype=np.float64), np.asarray(e_bins, dtype=np.float64)
    G = len(e_bins) - 1
    out = np.zeros((len(ein), G, L))
    with np.errstate(all="ignore"):
        for e, E in enumerate(ein):
            Emax, E0 = _setup(awr, Q, Ap, E)
            if not (E > 0.0) or not (Emax > 0.0):
                continue
            rE0 = np.sqrt(E0)
            for g in range(G):
                lo, hi = e_bins[g], e_bins[g + 1]
                if not _window_hit(Emax, rE0, lo, hi):
                    continue
                pts = _points(Emax, rE0, np.sqrt(lo), np.sqrt(hi))
                for pa, pb in zip(pts[:-1], pts[1:]):
                    T, ww = _outer(n, Emax, pa, pb, x, w)
                    out[e, g] += inner(T, ww, E0, lo, hi, x, w, L)
    return out


def _inner_sqrt(T, ww, E0, lo, hi, x, w, L):
    rT, rE0 = np.sqrt(T)[:, None], np.sqrt(E0)
    ia = np.maximum(np.abs(rT - rE0), np.sqrt(lo))
    ib = np.minimum(rT + rE0, np.sqrt(hi))
    on = (ib > ia)[:, 0]
    hm2, cm2 = 0.5 * (ib - ia), 0.5 * (ib + ia)
    sp = cm2 + hm2 * x[None, :]
    fk = (hm2 * w[None, :]) * (sp / ((2.0 * rT) * rE0))
    mu = np.clip(((sp - rT) * (sp + rT)) / ((2.0 * sp) * rE0) + rE0 / (2.0 * sp), -1.0, 1.0)
    I = np.array([(fk * P).sum(axis=1) for P in _legendre_terms(mu, max(L, 2))[:L]])
    I[:, ~on] = 0.0
    return (ww * I).sum(axis=1)


def _inner_cm(T, ww, E0, lo, hi, x, w, L):
    """over the CM cosine muc: E' = T + E0 + 2 muc sqrt(T E0) inside the group, density 1/2"""
    T = T[:, None]
    r = np.sqrt(T * E0)
    ia = np.maximum((lo - T - E0) / (2.0 * r), -1.0)
    ib = np.minimum((hi - T - E0) / (2.0 * r), 1.0)
    on = (ib > ia)[:, 0]
    hm2, cm2 = 0.5 * (ib - ia), 0.5 * (ib + ia)
    muc = cm2 + hm2 * x[None, :]
    Ep = T + E0 + 2.0 * muc * r
    mu = np.clip((np.sqrt(T) * muc + np.sqrt(E0)) / np.sqrt(Ep), -1.0, 1.0)
    fk = 0.5 * hm2 * w[None, :]
    I = np.array([(fk * P).sum(axis=1) for P in _legendre_terms(mu, max(L, 2))[:L]])
    I[:, ~on] = 0.0
    return (ww * I).sum(axis=1)


def nbody_converged(awr, Q, n, Ap, ein, e_bins, L, order=96):
    return _fine(awr, Q, n, Ap, ein, e_bins, L, order, _inner_sqrt)


def nbody_cm_check(awr, Q, n, Ap, ein, e_bins, L, order=64):
    return _fine(awr, Q, n, Ap, ein, e_bins, L, order, _inner_cm)


def threshold(awr, Q):
    """an incoming energy at which Emax is exactly <= 0 and one ulp above which it is positive: the
    largest E with (awr / (awr + 1)) * E + Q <= 0 in float64"""
    f = awr / (awr + 1.0)
    E = -Q / f
    while f * E + Q > 0.0:
        E = np.nextafter(E, 0.0)
    while f * np.nextafter(E, np.inf) + Q <= 0.0:
        E = np.nextafter(E, np.inf)
    return float(E)


def nbody_nuclide(with_mt16=True, p_valid=True):
    """A deuterium-like synthetic nuclide (the dict format of tests/synth.py): elastic scattering, one
    discrete level, and LAST an MT 16 reaction (Q = -2.2246, two neutrons) under law 66 with n = 3
    bodies and Ap = 2.9986, whose threshold is the grid point 3.4 MeV.  p_valid: MT 16 carries a
    validity table that falls from 1 to 0.8 (False: none, p_valid = 1)."""
    from synth import ace_adist
    awr, kT = 1.9968, 2.5301e-8
    energy = np.concatenate([np.geomspace(1e-11, 1.0, 16), [2.0, 3.0, 3.4, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 14.0,
                                                            16.0, 18.0, 20.0]])
    n_grid = len(energy)
    elastic = 3.0 + 0.4 / (1.0 + energy)
    thr51, thr16 = 16, 19                                   # 1-based: energy[15] = 1.0, energy[18] = 3.4
    s51 = 0.05 + 0.02 * np.arange(n_grid - thr51 + 1)
    s16 = 0.01 + 0.015 * np.arange(n_grid - thr16 + 1)
    Q51 = -0.5
    reactions = [
        dict(MT=2, Q=0.0, mult=1, thr=1, in_cm=1, sigma=None,
             adist=ace_adist([1e-11, 1e-3, 20.0], ["iso", "lin", "lin"], seed=16), edists=[]),
        dict(MT=51, Q=Q51, mult=1, thr=thr51, in_cm=1, sigma=s51,
             adist=ace_adist([energy[thr51 - 1], 20.0], ["lin", "hist"], seed=51),
             edists=[dict(law=3, data=np.array([(awr + 1.0) / awr * abs(Q51), (awr / (awr + 1.0)) ** 2]),
                          pv_x=None, pv_y=None)]),
    ]
    if with_mt16:
        pv = ([1e-5, 20.0], [1.0, 0.8]) if p_valid else (None, None)
        reactions.append(dict(MT=16, Q=-2.2246, mult=2, thr=thr16, in_cm=1, sigma=s16, adist=None,
                              edists=[dict(law=66, data=np.array([3.0, 2.9986]), pv_x=pv[0], pv_y=pv[1])]))
    return dict(awr=awr, kT=kT, freegas_cutoff=4.0 * kT, energy=energy, elastic=elastic, reactions=reactions,
                bins=np.array([0.0, 1e-3, 0.1, 1.0, 5.0, 20.0]), order=3, mu_bins=65)
