"""What interpolating on an incoming-energy grid costs, and a grid refined until it costs less
than a tolerance.

A library is read by interpolating its rows between grid points, linearly in ln E (the rule
thin_grid assumes, thin.F90).  The grids come from the reference's heuristics; nothing in the
reference measures the interpolation error, because a fresh row costs it a CPU-second.  Here:

  midpoints(x)            geometric means of neighbouring grid points
  grid_error_numpy(...)   host restatement of ndpp_grid_error (same operations, same order: same bits)
  check(...)              every table's rows at the midpoints of its grids in ONE scatt_library_at
                          call (thermal tables: sab_batch), then lib.grid_error per section
  refine(...)             insert the midpoint row wherever the error exceeds tol, re-check only the
                          intervals an insertion created, until nothing is above tol

The metric is the absolute error of the interpolated row over the row's scale (the largest |P0| of
the three rows involved): a moment of 1e-12 next to P0 = 1 must not decide the grid.  The rows are
the integrated ones, before print_tol and thinning.  The last interval of every grid is left out:
its upper point is the copy add_one_more_point appends (scatt.F90:426, sab.F90:452).

Bisection cannot resolve a jump of the model.  There are two kinds: the free-gas cutoff, where
elastic scattering changes integrator, and a reaction threshold.  max_passes bounds the effort;
what is still above tol is listed as `unresolved`, and marked `at_breakpoint` when the interval
contains or touches one of the breakpoints the report names."""
from __future__ import annotations

import math

import numpy as np

from . import lib

SECTIONS = ("elastic", "inelastic", "nu-inelastic")


def midpoints(x) -> np.ndarray:
    """sqrt(x[i] * x[i+1]): the midpoints in ln E."""
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(x[:-1] * x[1:])


def grid_error_numpy(x, y, x_mid, y_mid):
    """ndpp_grid_error on the host (include/ndpp_hip.h): (err[n-1], arg[n-1]).  math.log is the
    C library's log, the one the entry point calls; everything after it is IEEE + - * / in the
    kernel's order."""
    x, x_mid = np.asarray(x, dtype=np.float64), np.asarray(x_mid, dtype=np.float64)
    y, y_mid = np.asarray(y, dtype=np.float64), np.asarray(y_mid, dtype=np.float64)
    n, G, L = y.shape
    Y, M = y.reshape(n, G * L), y_mid.reshape(n - 1, G * L)
    err, arg = np.zeros(n - 1), np.zeros(n - 1, dtype=np.int32)
    for i in range(n - 1):
        x0, x1, xm = float(x[i]), float(x[i + 1]), float(x_mid[i])
        if not (math.isfinite(x0) and math.isfinite(x1) and x0 > 0.0 and x1 > x0 and x0 < xm < x1):
            err[i], arg[i] = -1.0, -1
            continue
        f = math.log(xm / x0) / math.log(x1 / x0)
        with np.errstate(all="ignore"):
            d = np.abs(Y[i] + (Y[i + 1] - Y[i]) * f - M[i])
            bad = ~(d < np.inf)
        if bad.any():
            err[i], arg[i] = np.inf, int(np.argmax(bad))
            continue
        k = int(np.argmax(d))                       # the first of equal maxima
        scale = max(np.abs(Y[i, ::L]).max(), np.abs(Y[i + 1, ::L]).max(), np.abs(M[i, ::L]).max())
        err[i], arg[i] = (0.0 if scale == 0.0 else d[k] / scale), k
    return err, arg


def _pair_errors(error, x, mats, idx, xm, rows):
    """errors of the intervals idx of x against the rows at xm: {name: (err, arg)}.  The error
    function takes consecutive abscissae, so the chosen intervals are laid out as pairs
    (x[i], x[i+1]) one after the other; the intervals between two pairs get a NaN midpoint and
    come back skipped."""
    k = len(idx)
    px = np.empty(2 * k)
    px[0::2], px[1::2] = x[idx], x[idx + 1]
    pm = np.full(2 * k - 1, np.nan)
    pm[0::2] = xm
    out = {}
    for name, y in mats.items():
        py = np.empty((2 * k,) + y.shape[1:])
        py[0::2], py[1::2] = y[idx], y[idx + 1]
        pr = np.zeros((2 * k - 1,) + y.shape[1:])
        pr[0::2] = rows[name]
        e, a = error(px, py, pm, pr)
        out[name] = (e[0::2], a[0::2])
    return out


def _touches(lo, hi, breakpoints):
    return any(lo <= b <= hi for b in breakpoints)


def check_grids(grids: dict, evaluate, tol: float, error=None, breakpoints=None, exclude_last: bool = True) -> dict:
    """grids: {key: dict(x=ein[n], mats={section: y[n][G][L]})}.  evaluate({key: energies}) returns
    {key: {section: rows}}, called once.  Returns {key: {section: report}}: worst error, its interval,
    the (group, order) deciding it, intervals above tol, skipped, checked."""
    error = error or lib.grid_error
    breakpoints = breakpoints or {}
    count = {}
    for key, g in grids.items():
        n_int = len(g["x"]) - 1 - int(exclude_last)
        if n_int > 0:
            count[key] = n_int
    rows = evaluate({key: midpoints(grids[key]["x"])[:m] for key, m in count.items()}) if count else {}
    rep = {}
    for key, g in grids.items():
        rep[key] = {}
        x = np.asarray(g["x"], dtype=np.float64)
        L = next(iter(g["mats"].values())).shape[2]
        for name in g["mats"]:
            r = dict(intervals=0, above=0, skipped=0, worst=None, interval=None, group=None, order=None,
                     at_breakpoint=False, above_intervals=[])
            if key in count:
                m = count[key]                   # the first m intervals: consecutive, so no pair layout here
                e, a = error(x[:m + 1], g["mats"][name][:m + 1], midpoints(x)[:m], rows[key][name])
                r["intervals"], r["skipped"] = m, int((e < 0).sum())
                hot = np.flatnonzero(e > tol)
                r["above"] = int(len(hot))
                r["above_intervals"] = [[float(x[j]), float(x[j + 1])] for j in hot]
                if (e >= 0).any():
                    j = int(np.argmax(np.where(e >= 0, e, -1.0)))
                    r.update(worst=float(e[j]), interval=[float(x[j]), float(x[j + 1])],
                             group=int(a[j]) // L, order=int(a[j]) % L,
                             at_breakpoint=_touches(x[j], x[j + 1], breakpoints.get(key, ())))
            rep[key][name] = r
    return rep


def refine_grids(grids: dict, evaluate, tol: float, max_passes: int = 6, max_growth: float = 4.0, error=None,
                 breakpoints=None, exclude_last: bool = True):
    """The check loop on {key: dict(x, mats)} (see check_grids).  Every pass integrates the midpoints
    of the intervals still to be checked -- all of them in the first pass, afterwards only the ones an
    insertion created -- in one evaluate() call, and inserts the midpoint row where any section of the
    grid is above tol; no energy is ever integrated twice.  After max_passes passes of insertions the
    intervals created last are checked once more, without inserting.  A grid that would grow beyond
    max_growth times its original length stops there.  Returns (refined grids, {key: report}); a
    report lists what is still above tol as `unresolved` (never dropped silently)."""
    if not (tol > 0.0) or not math.isfinite(tol):
        raise ValueError(f"tol must be a positive number, got {tol!r}")
    if max_passes < 0 or not (max_growth >= 1.0):
        raise ValueError(f"max_passes={max_passes!r} (>= 0) and max_growth={max_growth!r} (>= 1) expected")
    error = error or lib.grid_error
    breakpoints = breakpoints or {}
    cur, todo, rep = {}, {}, {}
    for key, g in grids.items():
        x = np.array(g["x"], dtype=np.float64)
        cur[key] = dict(x=x, mats={s: np.array(y, dtype=np.float64) for s, y in g["mats"].items()})
        mask = np.zeros(max(len(x) - 1, 0), dtype=bool)
        mask[:max(len(x) - 1 - int(exclude_last), 0)] = True
        todo[key] = mask
        rep[key] = dict(points_before=len(x), points_after=len(x), added=0, passes=0, skipped=0, stopped="converged",
                        unresolved=[], breakpoints=[float(b) for b in breakpoints.get(key, ())])
    for p in range(max_passes + 1):
        req = {}
        for key, mask in todo.items():
            idx = np.flatnonzero(mask)
            if len(idx):
                req[key] = midpoints(cur[key]["x"])[idx]
        if not req:
            break
        rows = evaluate(req)
        for key, xm in req.items():
            g, r = cur[key], rep[key]
            x, idx = g["x"], np.flatnonzero(todo[key])
            L = next(iter(g["mats"].values())).shape[2]
            errs = _pair_errors(error, x, g["mats"], idx, xm, rows[key])
            worst = np.max([e for e, _ in errs.values()], axis=0)
            which = np.argmax([e for e, _ in errs.values()], axis=0)
            names = list(errs)
            r["skipped"] += int((worst < 0).sum())
            hot = np.flatnonzero(worst > tol)
            reason = None
            if p == max_passes:
                reason = "max_passes"
            elif len(x) + len(hot) > max_growth * r["points_before"]:
                reason = "max_growth"
            if reason or not len(hot):
                for j in hot:
                    a = int(errs[names[which[j]]][1][j])
                    lo, hi = float(x[idx[j]]), float(x[idx[j] + 1])
                    r["unresolved"].append(dict(section=names[which[j]], interval=[lo, hi], err=float(worst[j]),
                                                group=a // L, order=a % L, reason=reason,
                                                at_breakpoint=_touches(lo, hi, r["breakpoints"])))
                if len(hot):
                    r["stopped"] = reason
                todo[key] = np.zeros(len(x) - 1, dtype=bool)
                continue
            at = idx[hot] + 1                                  # positions in x the midpoints go in front of
            g["x"] = np.insert(x, at, xm[hot])
            for s in g["mats"]:
                g["mats"][s] = np.insert(g["mats"][s], at, rows[key][s][hot], axis=0)
            mask = np.zeros(len(g["x"]) - 1, dtype=bool)
            new_pos = at + np.arange(len(hot))                 # where the inserted points ended up
            mask[new_pos - 1] = True
            mask[new_pos] = True
            todo[key] = mask
            r["passes"] = p + 1
            r["added"] += int(len(hot))
            r["points_after"] = len(g["x"])
    return cur, rep


# ---- the tables of a run (ndpp_amd.run.load_tables) ---------------------------------------------------

def table_breakpoints(data: dict) -> list:
    """The energies where a neutron table's model jumps: the free-gas cutoff and the thresholds of
    its scattering reactions (is_valid_scatter, scattdata_header.F90:1502-1515)."""
    out = set()
    fc = float(data.get("freegas_cutoff", 0.0))
    if 0.0 < fc < math.inf:
        out.add(fc)
    for r in data["reactions"]:
        mt = int(r["MT"])
        if mt != 2 and 11 <= mt <= 91 and mt not in (18, 19, 20, 21, 38) and int(r["thr"]) > 1:
            out.add(float(data["energy"][int(r["thr"]) - 1]))
    return sorted(out)


def _neutron_grids(k, res):
    g = {(k, "el"): dict(x=res["ein_el"], mats={"elastic": res["el_mat"]})}
    if res.get("ein_inel") is not None and len(res["ein_inel"]):
        mats = {"inelastic": res["inel_mat"]}
        if res.get("nuinel_mat") is not None:
            mats["nu-inelastic"] = res["nuinel_mat"]
        g[(k, "inel")] = dict(x=res["ein_inel"], mats=mats)
    return g


def library_evaluator(p, bins, tables: list, nuscatter: bool, sentinels=None):
    """evaluate() for the keys (table index, "el" | "inel") of neutron tables and (index, "sab") of
    thermal ones: ONE scatt_library_at call for all neutron energies asked for, one sab_batch per
    thermal table (with a sentinel energy appended and dropped: the last row sab_batch returns is
    the copy of its neighbour, sab.F90:452; sentinels[key] is that energy, the grid's own top point)."""
    neut = [k for k, t in enumerate(tables) if t["kind"] == "neutron"]
    nucs = {k: lib.AceNuclide.from_desc(tables[k]["data"]) for k in neut}

    def evaluate(req: dict) -> dict:
        out = {}
        ks = [k for k in neut if (k, "el") in req or (k, "inel") in req]
        if ks:
            res = lib.scatt_library_at(p, [nucs[k] for k in ks], bins, [req.get((k, "el")) for k in ks],
                                       [req.get((k, "inel")) for k in ks], nuscatter)
            for k, r in zip(ks, res):
                if (k, "el") in req:
                    out[(k, "el")] = {"elastic": r["el_mat"]}
                if (k, "inel") in req:
                    out[(k, "inel")] = {"inelastic": r["inel_mat"]}
                    if r["nuinel_mat"] is not None:
                        out[(k, "inel")]["nu-inelastic"] = r["nuinel_mat"]
        for key, e in req.items():
            if key[1] == "sab":
                d = tables[key[0]]["data"]
                sentinel = float(sentinels[key])
                out[key] = {"elastic": lib.sab_batch(p, d, np.append(e, sentinel), bins)[:-1]}
        return out

    return evaluate


def _section_reports(tables, per_key):
    out = []
    for k, t in enumerate(tables):
        rec = dict(name=t["listing"]["name"], kind=t["kind"], sections={},
                   breakpoints=table_breakpoints(t["data"]) if t["kind"] == "neutron" else [])
        if t["kind"] == "thermal":
            rec["note"] = "thermal table: checked, not refined"
        for key in ((k, "el"), (k, "inel"), (k, "sab")):
            for name, r in per_key.get(key, {}).items():
                rec["sections"][name] = r
        out.append(rec)
    return out


def check(p, bins, tables: list, results: list, nuscatter: bool, tol: float = 1.0e-3, error=None) -> list:
    """Check the grids of a run.  tables: ndpp_amd.run.load_tables' list; results[k]: table k's rows
    as scatt_library / sab_batch returned them (dict ein_el, el_mat, ein_inel, inel_mat, nuinel_mat).
    Returns one record per table: name, kind, breakpoints, sections = {elastic | inelastic |
    nu-inelastic: worst error, its interval (E_lo, E_hi), group and order deciding it, intervals above
    tol (with their energies), skipped, checked}."""
    grids, bps, top = {}, {}, {}
    for k, (t, r) in enumerate(zip(tables, results)):
        if t["kind"] == "neutron":
            grids.update(_neutron_grids(k, r))
            bps[(k, "el")] = bps[(k, "inel")] = table_breakpoints(t["data"])
        else:
            grids[(k, "sab")] = dict(x=r["ein_el"], mats={"elastic": r["el_mat"]})
            top[(k, "sab")] = r["ein_el"][-1]
    per_key = check_grids(grids, library_evaluator(p, bins, tables, nuscatter, top), tol, error=error, breakpoints=bps)
    return _section_reports(tables, per_key)


def refine(p, bins, tables: list, results: list, nuscatter: bool, tol: float, max_passes: int = 6,
           max_growth: float = 4.0, error=None):
    """Refine the grids of the neutron tables of a run until no interval is above tol (refine_grids).
    Returns (new results, report): results[k] of a neutron table holds the refined grids and rows --
    every original energy and row is still there, untouched -- a thermal table's entry is returned as
    it came (thermal tables are checked, not refined); report[k]: per grid points before / after,
    passes, added, skipped, stopped, unresolved [dict(section, interval, err, group, order, reason,
    at_breakpoint)], breakpoints."""
    grids, bps = {}, {}
    for k, (t, r) in enumerate(zip(tables, results)):
        if t["kind"] == "neutron":
            grids.update(_neutron_grids(k, r))
            bps[(k, "el")] = bps[(k, "inel")] = table_breakpoints(t["data"])
    new, rep = refine_grids(grids, library_evaluator(p, bins, tables, nuscatter), tol, max_passes, max_growth,
                            error=error, breakpoints=bps)
    out, report = [], []
    for k, (t, r) in enumerate(zip(tables, results)):
        rec = dict(name=t["listing"]["name"], kind=t["kind"], grids={})
        if t["kind"] != "neutron":
            rec["note"] = "thermal table: checked, not refined"
            out.append(r)
            report.append(rec)
            continue
        nr = dict(r)
        nr["ein_el"], nr["el_mat"] = new[(k, "el")]["x"], new[(k, "el")]["mats"]["elastic"]
        rec["grids"]["elastic"] = rep[(k, "el")]
        if (k, "inel") in new:
            nr["ein_inel"], nr["inel_mat"] = new[(k, "inel")]["x"], new[(k, "inel")]["mats"]["inelastic"]
            if "nu-inelastic" in new[(k, "inel")]["mats"]:
                nr["nuinel_mat"] = new[(k, "inel")]["mats"]["nu-inelastic"]
            rec["grids"]["inelastic"] = rep[(k, "inel")]
        rec["breakpoints"] = table_breakpoints(t["data"])
        out.append(nr)
        report.append(rec)
    return out, report


def format_lines(check_report: list) -> list:
    """One line per table and section of a check() report."""
    lines = []
    for t in check_report:
        for name, r in t["sections"].items():
            if r["worst"] is None:
                lines.append(f"{t['name']:>12s} {name:13s} no interval to check")
                continue
            lines.append(f"{t['name']:>12s} {name:13s} worst {r['worst']:.3e} in [{r['interval'][0]:.6e}, "
                         f"{r['interval'][1]:.6e}] MeV (group {r['group']}, order {r['order']})"
                         f"{' at a breakpoint' if r['at_breakpoint'] else ''}; {r['above']} of {r['intervals']} "
                         f"intervals above tol, {r['skipped']} skipped"
                         f"{'; ' + t['note'] if t.get('note') else ''}")
    return lines
