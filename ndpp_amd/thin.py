"""Error-bounded thinning of incoming-energy grids (include/ndpp_hip.h:
ndpp_thin_segments, ndpp_thin_bounded).

The reference's thin_grid (ndpp_thin_grid, `thinning_tol`) tests a point against the last kept point
and its right neighbour only, under an element-wise relative metric: the points it has already
dropped are never checked against the pair that finally brackets them, so its tolerance bounds
nothing.  Here every candidate segment (a, a+d), d = 2..window, is measured against every point
strictly inside it under the scale-relative metric of ndpp_amd.gridcheck, and a point is dropped only
inside a segment whose worst error is at most tol:

  segment_errors_numpy(...)   host restatement of ndpp_thin_segments (same operations, same order:
                              same bits)
  chain(seg_err, tol)         the kept points: from each kept point to the farthest admissible partner
  thin_results(...)           the elastic and inelastic grids of every neutron table of a run
"""
from __future__ import annotations

import math

import numpy as np

from . import gridcheck, lib


def _scales(Y, L):
    with np.errstate(all="ignore"):
        return np.abs(Y[:, ::L]).max(axis=1)


def segment_errors_numpy(x, y, y2=None, tokeep=None, window: int = 32) -> np.ndarray:
    """ndpp_thin_segments on the host: seg_err[n][window-1].  math.log is the C library's log, the one
    the entry point calls; everything after it is IEEE + - * / in the kernel's order."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, G, L = y.shape
    W = int(window)
    secs = [y.reshape(n, G * L)] + ([] if y2 is None else [np.asarray(y2, dtype=np.float64).reshape(n, G * L)])
    scales = [_scales(Y, L) for Y in secs]
    lx = np.array([math.log(v) for v in x])
    keep = np.isin(x, np.asarray([] if tokeep is None else tokeep, dtype=np.float64))
    seg = np.full((n, W - 1), -1.0)
    for a in range(n):
        for d in range(2, min(W, n - 1 - a) + 1):
            b = a + d
            ks = np.arange(a + 1, b)
            if keep[ks].any():
                seg[a, d - 2] = np.inf
                continue
            f = (lx[ks] - lx[a]) / (lx[b] - lx[a])
            worst = 0.0
            for Y, s in zip(secs, scales):
                with np.errstate(all="ignore"):
                    dd = np.abs(Y[a] + (Y[b] - Y[a]) * f[:, None] - Y[ks])
                    bad = ~(dd < np.inf).all(axis=1)
                    dm = np.where(bad[:, None], 0.0, dd).max(axis=1)
                    scale = np.maximum(np.maximum(s[a], s[ks]), s[b])
                    e = np.where(scale == 0.0, 0.0, dm / np.where(scale == 0.0, 1.0, scale))
                e = np.where(bad, np.inf, e)
                worst = max(worst, float(e.max()))
            seg[a, d - 2] = worst
    return seg


def chain(seg_err, tol: float):
    """The kept points of a grid with segment errors seg_err[n][W-1] at tol: (indices, max_err).  A
    segment (a, a+d) is admissible when 0 <= seg_err[a][d-2] <= tol, (a, a+1) always; from each kept
    point the chain goes to the farthest admissible partner within the window, until n-1.  max_err is
    the largest seg_err along the chain."""
    seg = np.asarray(seg_err, dtype=np.float64)
    n, W = seg.shape[0], seg.shape[1] + 1
    if not (tol >= 0.0) or not math.isfinite(tol):
        raise ValueError(f"tol must be finite and not negative, got {tol!r}")
    kept, a, worst = [0], 0, 0.0
    while a < n - 1:
        nxt, e_nxt = a + 1, 0.0
        for d in range(min(W, n - 1 - a), 1, -1):
            e = seg[a, d - 2]
            if 0.0 <= e <= tol:
                nxt, e_nxt = a + d, float(e)
                break
        worst = max(worst, e_nxt)
        a = nxt
        kept.append(a)
    return np.array(kept, dtype=np.int32), worst


def must_keep(bins, data: dict) -> np.ndarray:
    """The energies thinning never removes from a neutron table's grids (next to the first and the last
    point): the group edges -- finish_scatt's tokeep -- and the table's breakpoints, the free-gas cutoff
    and the reaction thresholds (gridcheck.table_breakpoints)."""
    return np.concatenate([np.asarray(bins, dtype=np.float64), np.asarray(gridcheck.table_breakpoints(data), dtype=np.float64)])


def thin_results(p, bins, tables: list, results: list, nuscatter: bool, tol: float, window: int = 32, bounded=None):
    """Thin the elastic and the inelastic grid (nu-inelastic rides along, as in ndpp_thin_grid) of every
    neutron table.  tables: ndpp_amd.run.load_tables' list; results[k]: table k's rows (dict ein_el,
    el_mat, ein_inel, inel_mat, nuinel_mat), before print_tol.  Returns (new results, report): one
    record per table -- name, kind, sections = {elastic | inelastic: points_before, points_after,
    max_err}, breakpoints, note.  A thermal table's entry is returned as it came; thermal tables and chi
    grids are not thinned, and the record says so.  (p and nuscatter: the signature of
    gridcheck.refine; thinning integrates nothing.)"""
    if not (tol > 0.0) or not math.isfinite(tol):
        raise ValueError(f"tol must be a positive number, got {tol!r}")
    bounded = bounded or lib.thin_bounded
    out, report = [], []
    for t, r in zip(tables, results):
        rec = dict(name=t["listing"]["name"], kind=t["kind"], sections={})
        if t["kind"] != "neutron":
            rec["note"] = "thermal table: not thinned"
            out.append(r)
            report.append(rec)
            continue
        keep = must_keep(bins, t["data"])
        rec["breakpoints"] = gridcheck.table_breakpoints(t["data"])
        rec["note"] = "chi grid: not thinned"
        nr = dict(r)
        sections = [("elastic", "ein_el", ("el_mat",))]
        if r.get("ein_inel") is not None and len(r["ein_inel"]):
            sections.append(("inelastic", "ein_inel", ("inel_mat",) + (("nuinel_mat",) if r.get("nuinel_mat") is not None else ())))
        for name, xk, mats in sections:
            x = np.asarray(r[xk], dtype=np.float64)
            if len(x) < 2:
                rec["sections"][name] = dict(points_before=len(x), points_after=len(x), max_err=0.0)
                continue
            idx, worst = bounded(x, r[mats[0]], r[mats[1]] if len(mats) > 1 else None, keep, tol, window)
            nr[xk] = x[idx]
            for m in mats:
                nr[m] = np.ascontiguousarray(r[m][idx])
            rec["sections"][name] = dict(points_before=len(x), points_after=len(idx), max_err=float(worst))
            if len(mats) > 1:
                rec["sections"][name]["rides_along"] = "nu-inelastic"
        out.append(nr)
        report.append(rec)
    return out, report


def format_lines(report: list, tol: float) -> list:
    """One line per table of a thin_results() report."""
    lines = []
    for t in report:
        if not t["sections"]:
            lines.append(f"{t['name']:>12s} {t['note']}")
            continue
        body = ", ".join(f"{name} {s['points_before']} -> {s['points_after']} E_in (max err {s['max_err']:.3e})"
                         for name, s in t["sections"].items())
        lines.append(f"{t['name']:>12s} thinned to {tol:g}: {body}; {t['note']}")
    return lines
