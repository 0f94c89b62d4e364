"""TEST INFRASTRUCTURE: host restatements of ndpp_nbody_tab_batch (include/ndpp_hip.h: ACE law 66 in
lab-cosine bins).

nbody_tab_numpy      the definition, operation by operation in float64 and in its sum order, with the
                     library's own 32 nodes and weights (ndpp_nbody_rule): the same bits as the kernel.
nbody_tab_converged  the same scheme with a 96-point rule: what the 32-point rule is measured against.
nbody_tab_cm_check   a route that shares nothing with the definition: the outer variable t and the
                     breakpoints of the Legendre scheme (nbody_ref._points, _outer), composite 8-point
                     panels, and at each CM energy T the mass of {s' : mu(s') <= m} in closed form; a
                     bin is the difference of two such sets.  The cosine cut puts kinks in T that the
                     panels do not know, so it converges algebraically: a cross-check against mass in
                     the wrong bin and nothing else.
All return out[n_ein][G][N]; nbody_tab_numpy also the status words."""
from __future__ import annotations

import numpy as np

from nbody_ref import ST_RANGE, TWO_OVER_B, _outer, _points, _setup, _window_hit

POWER = {3: 1.5, 4: 3.0, 5: 4.5}           # p = 3n/2 - 3


def tab_edges(N):
    """b_0 .. b_N of tab_kernels.hip's tab_edge: -1 + (2 k) / N, and 1 at k = N"""
    e = -1.0 + (2.0 * np.arange(N + 1, dtype=np.float64)) / float(N)
    e[N] = 1.0
    return e


def _order2(a, b):
    return np.where(a < b, a, b), np.where(a < b, b, a)


def _root(c, disc, sgn, sa, sb):
    """[G][N]: the root c + sgn sqrt(disc) where it lies strictly inside (sa, sb), else sb"""
    r = c + sgn * np.sqrt(disc)
    keep = (disc > 0.0)[None, :] & (r[None, :] > sa) & (r[None, :] < sb)
    return np.where(keep, r[None, :], sb)


def _piece(n, Emax, rE0, c0, c1, disc0, disc1, dm, pa, pb, x, w):
    ln = pb - pa
    piece = np.zeros_like(pa)
    for j in range(len(x)):                                  # the nodes, ascending
        u = 0.5 + 0.5 * x[j]
        h = (u * u) * (3.0 - 2.0 * u)
        sp = pa + ln * h
        wgt = ((0.5 * w[j]) * ln) * ((6.0 * u) * (1.0 - u))
        t0, t1 = sp - c0, sp - c1
        y0 = (disc0 - t0 * t0) / Emax
        y1 = (disc1 - t1 * t1) / Emax
        y0c = np.where(y0 > 0.0, y0, 0.0)
        y1c = np.where(y1 > 0.0, y1, 0.0)
        d = np.where(y0 > 0.0, (((2.0 * sp) * rE0) * dm) / Emax, y1c)
        q2 = (y1c * y1c + y1c * y0c) + y0c * y0c
        if n == 4:
            D = q2
        elif n == 3:
            D = q2 / (y1c * np.sqrt(y1c) + y0c * np.sqrt(y0c))
        else:
            a3, b3 = (y1c * y1c) * y1c, (y0c * y0c) * y0c
            D = (q2 * ((a3 * a3 + a3 * b3) + b3 * b3)) / ((a3 * y1c) * np.sqrt(y1c) + (b3 * y0c) * np.sqrt(y0c))
        f = np.where(y1c > 0.0, (sp * d) * D, 0.0)
        piece = piece + wgt * f
    return piece


def nbody_tab_numpy(awr, Q, n, Ap, ein, e_bins, N, rule=None):
    """(out, status) of ndpp_nbody_tab_batch, bit for bit.  rule: (x, w), default the library's."""
    if rule is None:
        from ndpp_amd import lib
        rule = lib.nbody_rule()
    x, w = (np.asarray(a, dtype=np.float64) for a in rule)
    ein, e_bins = np.asarray(ein, dtype=np.float64), np.asarray(e_bins, dtype=np.float64)
    G = len(e_bins) - 1
    out, status = np.zeros((len(ein), G, N)), np.zeros(len(ein), dtype=np.int32)
    edges = tab_edges(N)
    m0, m1 = edges[:-1], edges[1:]
    dm = m1 - m0
    lo, hi = e_bins[:-1], e_bins[1:]
    with np.errstate(all="ignore"):
        for e, E in enumerate(ein):
            if not (E > 0.0) or not (E <= np.finfo(np.float64).max):
                status[e] = ST_RANGE
                continue
            Emax, E0 = _setup(awr, Q, Ap, E)
            if not (Emax > 0.0):
                continue
            rE0, rEm = np.sqrt(E0), np.sqrt(Emax)
            wd = rE0 - rEm
            wl = wd if wd > 0.0 else 0.0
            wh = rEm + rE0
            hit = (hi > wl * wl) & (lo < wh * wh)
            rlo, rhi = np.sqrt(lo), np.sqrt(hi)
            sa = np.broadcast_to(np.where(rlo > wl, rlo, wl)[:, None], (G, N))
            sb = np.broadcast_to(np.where(rhi < wh, rhi, wh)[:, None], (G, N))
            c0, c1 = m0 * rE0, m1 * rE0
            disc0 = Emax - E0 * ((1.0 - m0) * (1.0 + m0))
            disc1 = Emax - E0 * ((1.0 - m1) * (1.0 + m1))
            b0, b1 = _root(c0, disc0, -1.0, sa, sb), _root(c0, disc0, 1.0, sa, sb)
            b2, b3 = _root(c1, disc1, -1.0, sa, sb), _root(c1, disc1, 1.0, sa, sb)
            b0, b1 = _order2(b0, b1)
            b2, b3 = _order2(b2, b3)
            b0, b2 = _order2(b0, b2)
            b1, b3 = _order2(b1, b3)
            b1, b2 = _order2(b1, b2)
            total, pa = np.zeros((G, N)), sa
            for pb in (b0, b1, b2, b3, sb):                      # the pieces, ascending
                on = pb > pa
                piece = _piece(n, Emax, rE0, c0[None, :], c1[None, :], disc0[None, :], disc1[None, :], dm[None, :],
                               pa, pb, x, w)
                total = np.where(on, total + piece, total)
                pa = np.where(on, pb, pa)
            val = (TWO_OVER_B[n] / (((4.0 * POWER[n]) * rEm) * rE0)) * total
            out[e] = np.where(hit[:, None], val, 0.0)
    return out, status


def nbody_tab_converged(awr, Q, n, Ap, ein, e_bins, N, order=96):
    return nbody_tab_numpy(awr, Q, n, Ap, ein, e_bins, N, rule=np.polynomial.legendre.leggauss(order))[0]


def nbody_tab_cm_check(awr, Q, n, Ap, ein, e_bins, N, panels=4000):
    x8, w8 = np.polynomial.legendre.leggauss(8)
    ein, e_bins = np.asarray(ein, dtype=np.float64), np.asarray(e_bins, dtype=np.float64)
    G = len(e_bins) - 1
    out = np.zeros((len(ein), G, N))
    m = tab_edges(N)[:, None]                                    # [N + 1][1]
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
                rlo, rhi = np.sqrt(lo), np.sqrt(hi)
                pts = _points(Emax, rE0, rlo, rhi)
                for pa, pb in zip(pts[:-1], pts[1:]):
                    k = max(8, int(np.ceil(panels * (pb - pa))))
                    cut = np.linspace(pa, pb, k + 1)
                    T, ww = _outer(n, Emax, cut[:-1, None], cut[1:, None], x8[None, :], w8[None, :])
                    T, ww = T.ravel()[None, :], ww.ravel()[None, :]          # [1][nodes]
                    rT = np.sqrt(T)
                    ia = np.maximum(np.abs(rT - rE0), rlo)
                    ib = np.minimum(rT + rE0, rhi)
                    rad = m * m * E0 - E0 + T                                # [N + 1][nodes]
                    r = np.sqrt(np.where(rad > 0.0, rad, 0.0))
                    a_ = np.maximum(m * rE0 - r, ia)
                    b_ = np.minimum(m * rE0 + r, ib)
                    F = np.where((rad > 0.0) & (b_ > a_) & (ib > ia), (b_ * b_ - a_ * a_) / (4.0 * rT * rE0), 0.0)
                    out[e, g] += (ww * (F[1:] - F[:-1])).sum(axis=1)
    return out
