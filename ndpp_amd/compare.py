"""How far two NDPP libraries are apart (include/ndpp_hip.h: ndpp_lib_compare).

--refine-grid adds incoming energies and --thin-grid removes them, so two libraries of the same
nuclides need not share a grid, and a field-by-field comparison says nothing.  What a consumer sees
is the row it interpolates, linearly in ln E, from each: the distance of two sections is the largest
difference between those two rows over the energies both cover, under the scale-relative metric of
ndpp_amd.gridcheck (the absolute difference over the largest |P0| of the rows involved).

Where the supremum lies.  Between two neighbouring points u_k < u_k+1 of the union of the two grids
both interpolants are linear in ln E, so the difference of every element is the absolute value of
a linear function: convex, largest at an end.  The scale is constant on [u_k, u_k+1) -- the four
rows are the same -- but it JUMPS at u_k+1, where a grid moves on to its next pair of rows (an exact
hit reads rows i and i + 1).  err is therefore continuous from the right at a union point and not
from the left, and its supremum over [u_k, u_k+1) is the larger of err(u_k) and the limit of err
from below u_k+1.  union_queries returns the union points and, for that limit, the largest double
below each of them: over these the maximum of err is the distance of the two sections, to the
rounding of one interpolation step, not a sample of it.

  compare_numpy(...)      host restatement of ndpp_lib_compare (same operations, same order: same bits)
  union_queries(xa, xb)   the sorted union of the grids clipped to the range both cover, each point
                          but the first preceded by the largest double below it
  compare_sections(a, b)  one pair of sections: worst error, where, worst[g][l], what lies outside
  compare_tables(ta, tb)  every section reader.py returns for a table: elastic, inelastic,
                          nu-inelastic, and chi (total, prompt, delayed-k: L = 1, scale max |chi|)
  compare_dirs(A, B)      two library directories, tables matched by name

A section that cannot be compared is reported with the reason, never left out: different group
structure, different scatt_type, a grid that is not strictly increasing (positive, finite), tabular
output (the tabular rows of the free-gas range do not settle), a section one
table lacks, no common energy range.

CLI: python -m ndpp_amd.compare DIR_A DIR_B [--tol T] [--json FILE]; one line per table and
section; exit 0 if every comparable section is within T (or no T was given), 1 if one is above T,
2 on an input error, 3 on a library or device error.
"""
from __future__ import annotations

import argparse
import json
import math
import struct
import sys
from pathlib import Path

import numpy as np

from . import lib, reader

EXIT_OK, EXIT_ABOVE, EXIT_INPUT, EXIT_LIBRARY = 0, 1, 2, 3
SCATT_SECTIONS = (("elastic", "elastic"), ("inelastic", "inelastic"), ("nu-inelastic", "nuinelastic"))
_BLOCK = 2048          # queries compare_numpy handles at a time


class InputError(ValueError):
    """a directory, ndpp_lib.xml or table file that cannot be read"""


def grid_ok(x) -> bool:
    """strictly increasing, positive and finite, at least two points: what ndpp_lib_compare takes"""
    x = np.asarray(x, dtype=np.float64)
    return bool(x.ndim == 1 and len(x) >= 2 and np.isfinite(x).all() and x[0] > 0.0 and (np.diff(x) > 0.0).all())


def _brackets(x, xq, ok):
    """per query the largest i with x[i] <= v and the weight of row i + 1 (math.log is the C library's
    log, the one the entry point calls)"""
    n = len(x)
    i = np.searchsorted(x, np.where(ok, xq, x[0]), side="right") - 1
    f = np.zeros(len(xq))
    for q in np.flatnonzero(ok):
        k, v = int(i[q]), float(xq[q])
        if v != x[k] and k != n - 1:
            f[q] = math.log(v / float(x[k])) / math.log(float(x[k + 1]) / float(x[k]))
    return i, f


def compare_numpy(xa, ya, xb, yb, xq):
    """ndpp_lib_compare on the host (include/ndpp_hip.h): (err[nq], arg[nq], worst[G][min(La, Lb)]).
    Everything after the logarithms is IEEE + - * / in the kernels' order."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    ya, yb = np.asarray(ya, dtype=np.float64), np.asarray(yb, dtype=np.float64)
    xq = np.asarray(xq, dtype=np.float64).ravel()
    if ya.ndim != 3 or yb.ndim != 3 or ya.shape[1] != yb.shape[1] or len(xa) != len(ya) or len(xb) != len(yb):
        raise ValueError(f"shapes do not match: xa {xa.shape}, ya {ya.shape}, xb {xb.shape}, yb {yb.shape}")
    if not (grid_ok(xa) and grid_ok(xb)):
        raise ValueError("both grids must be strictly increasing, positive and finite, with two points or more")
    (na, G, La), (nb, _, Lb) = ya.shape, yb.shape
    Lc = min(La, Lb)
    A, B = ya[:, :, :Lc].reshape(na, G * Lc), yb[:, :, :Lc].reshape(nb, G * Lc)
    with np.errstate(all="ignore"):
        ok = np.isfinite(xq) & (xq > 0.0) & (xq >= xa[0]) & (xq <= xa[-1]) & (xq >= xb[0]) & (xq <= xb[-1])
    ia, fa = _brackets(xa, xq, ok)
    ib, fb = _brackets(xb, xq, ok)
    ia1, ib1 = np.minimum(ia + 1, na - 1), np.minimum(ib + 1, nb - 1)
    err, arg = np.full(len(xq), -1.0), np.full(len(xq), -1, dtype=np.int32)
    worst = np.full(G * Lc, -1.0)
    live = np.flatnonzero(ok)
    for at in range(0, len(live), _BLOCK):
        q = live[at:at + _BLOCK]
        a0, a1, b0, b1 = A[ia[q]], A[ia1[q]], B[ib[q]], B[ib1[q]]
        with np.errstate(all="ignore"):
            d = np.abs((a0 + (a1 - a0) * fa[q, None]) - (b0 + (b1 - b0) * fb[q, None]))
            bad = ~(d < np.inf)
            scale = np.zeros(len(q))                   # fmax: a NaN never becomes the scale
            for rows in (a0, a1, b0, b1):
                scale = np.fmax(scale, np.fmax.reduce(np.abs(rows[:, ::Lc]), axis=1))
            zero = scale == 0.0
            v = np.where(bad, np.inf, np.where(zero[:, None], 0.0, d / np.where(zero, 1.0, scale)[:, None]))
        any_bad = bad.any(axis=1)
        k = np.where(any_bad, np.argmax(bad, axis=1), np.argmax(np.where(bad, -1.0, d), axis=1))   # the first of equal maxima
        err[q] = np.where(any_bad, np.inf, v[np.arange(len(q)), k])
        arg[q] = k
        worst = np.maximum(worst, v.max(axis=0))
    return err, arg, worst.reshape(G, Lc)


def union_points(xa, xb) -> np.ndarray:
    """The sorted union of two grids clipped to the range both cover.  Empty when the ranges do not meet."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    lo, hi = max(xa[0], xb[0]), min(xa[-1], xb[-1])
    u = np.union1d(xa, xb)
    return u[(u >= lo) & (u <= hi)]


def union_queries(xa, xb) -> np.ndarray:
    """Where the error of ndpp_lib_compare attains its supremum over the common range (module
    docstring): union_points, and in front of each but the first the largest double below it, which
    reads the rows of the interval that ends there.  Sorted, without duplicates."""
    u = union_points(xa, xb)
    return np.union1d(u, np.nextafter(u[1:], 0.0))


def _xy(sec):
    if isinstance(sec, reader.ScattSection):
        return sec.ein, sec.mat
    return sec


def _outside(x, lo, hi) -> dict:
    """the part of a grid outside [lo, hi]: its points there, and the energy ranges they span"""
    x = np.asarray(x, dtype=np.float64)
    return dict(points=int(((x < lo) | (x > hi)).sum()),
                below=[float(x[0]), float(lo)] if x[0] < lo else None,
                above=[float(hi), float(x[-1])] if x[-1] > hi else None)


def not_comparable(reason: str) -> dict:
    return dict(comparable=False, reason="not comparable: " + reason)


def compare_sections(a, b, compare=None) -> dict:
    """One pair of sections, each a reader.ScattSection or (x[n], y[n][G][L]).  Returns a dict:
    comparable, err (the worst error over union_queries), energy, group, moment (where it is),
    worst[g][l] (per compared element over all of them), queries, moments compared, and for each
    grid the part outside the common range (outside_a, outside_b: points, below, above).  A pair that
    cannot be compared: comparable False and the reason.  compare: lib.lib_compare (the device) unless
    given, e.g. compare_numpy."""
    compare = compare or lib.lib_compare
    (xa, ya), (xb, yb) = _xy(a), _xy(b)
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    ya, yb = np.asarray(ya, dtype=np.float64), np.asarray(yb, dtype=np.float64)
    if ya.ndim != 3 or yb.ndim != 3 or ya.shape[1] != yb.shape[1]:
        return not_comparable("different group structure")
    if not (grid_ok(xa) and grid_ok(xb)):
        return not_comparable("grid not increasing")
    xq = union_queries(xa, xb)
    if not len(xq):
        return not_comparable("no common energy range")
    err, arg, worst = compare(xa, ya, xb, yb, xq)
    Lc = min(ya.shape[2], yb.shape[2])
    k = int(np.argmax(err))                            # these queries are never skipped: every err >= 0
    return dict(comparable=True, err=float(err[k]), energy=float(xq[k]), group=int(arg[k]) // Lc,
                moment=int(arg[k]) % Lc, worst=np.asarray(worst), queries=int(len(xq)), moments=int(Lc),
                outside_a=_outside(xa, xq[0], xq[-1]), outside_b=_outside(xb, xq[0], xq[-1]))


def _chi_sections(t: reader.NdppTable) -> dict:
    """the chi sections of a table as (x, y[n][G][1])"""
    if not t.chi:
        return {}
    x = t.chi["e_grid"]
    out = {"chi-total": (x, t.chi["total"][:, :, None]), "chi-prompt": (x, t.chi["prompt"][:, :, None])}
    for k, d in enumerate(t.chi["delayed"]):
        out[f"chi-delayed-{k + 1}"] = (x, d[:, :, None])
    return out


def compare_tables(ta: reader.NdppTable, tb: reader.NdppTable, compare=None) -> dict:
    """Every section of two tables: {section name: compare_sections' dict}.  The scatter sections are
    not comparable when the scatt_type differs or is tabular; nothing is when the group structures
    differ; a section only one table holds is reported as such."""
    out = {}
    same_groups = np.array_equal(ta.e_bins, tb.e_bins)
    scatt_reason = None
    if ta.scatt_type != tb.scatt_type:
        scatt_reason = "different scatt_type"
    elif ta.scatt_type == reader.SCATT_TYPE_TABULAR:
        scatt_reason = "tabular output"
    pairs = [(name, getattr(ta, attr), getattr(tb, attr), scatt_reason) for name, attr in SCATT_SECTIONS]
    ca, cb = _chi_sections(ta), _chi_sections(tb)
    pairs += [(name, ca.get(name), cb.get(name), None) for name in list(ca) + [n for n in cb if n not in ca]]
    for name, a, b, reason in pairs:
        if a is None and b is None:
            continue
        if a is None or b is None:
            out[name] = not_comparable(f"section only in {'B' if a is None else 'A'}")
        elif not same_groups:
            out[name] = not_comparable("different group structure")
        elif reason:
            out[name] = not_comparable(reason)
        else:
            out[name] = compare_sections(a, b, compare)
    return out


def read_library(directory) -> dict:
    """{table name: (attributes, NdppTable)} of the library at `directory` (or its ndpp_lib.xml), in the
    order listed.  A table file is looked up at its `path` attribute, then next to the ndpp_lib.xml
    that names it.  Raises InputError."""
    d = Path(directory)
    xml = d / "ndpp_lib.xml" if d.is_dir() else d
    try:
        meta = reader.read_lib_xml(xml.read_bytes())
    except (OSError, ValueError, KeyError, IndexError) as e:
        raise InputError(f"cannot read {xml}: {e}") from None
    ftype = str(meta.get("filetype", "binary")).lower()
    if ftype not in ("binary", "ascii"):
        raise InputError(f"{xml}: filetype {ftype!r} is neither binary nor ascii")
    read = reader.read_binary if ftype == "binary" else reader.read_ascii
    out = {}
    for attrs in meta["tables"]:
        name, path = attrs.get("name"), attrs.get("path")
        if not name or not path:
            raise InputError(f"{xml}: an ndpp_table without name or path")
        if name in out:
            raise InputError(f"{xml}: table {name} is listed twice")
        p = Path(path)
        cands = [p if p.is_absolute() else xml.parent / p, xml.parent / p.name]
        f = next((c for c in cands if c.is_file()), None)
        if f is None:
            raise InputError(f"{xml}: the file of table {name} is neither at {cands[0]} nor at {cands[1]}")
        try:
            out[name] = (attrs, read(f.read_bytes()))
        except (OSError, ValueError, IndexError, struct.error) as e:
            raise InputError(f"{f}: not a{'n' if ftype == 'ascii' else ''} {ftype} NDPP table: {e}") from None
    return out


def compare_dirs(dir_a, dir_b, tol=None, compare=None) -> dict:
    """Two libraries, tables matched by name.  Returns dict(a, b, tol, tables = [dict(name, sections)]
    in A's order, only_in_a, only_in_b, err = the worst error of any comparable section (None if
    there is none), at = (table, section) holding it, above = [(table, section)] with err > tol,
    not_comparable = [(table, section)]).  Raises InputError on unreadable input, lib.NdppError from
    the device."""
    la, lb = read_library(dir_a), read_library(dir_b)
    rep = dict(a=str(dir_a), b=str(dir_b), tol=tol, tables=[], only_in_a=[n for n in la if n not in lb],
               only_in_b=[n for n in lb if n not in la], err=None, at=None, above=[], not_comparable=[])
    for name, (_, ta) in la.items():
        if name not in lb:
            continue
        secs = compare_tables(ta, lb[name][1], compare)
        rep["tables"].append(dict(name=name, sections=secs))
        for sname, s in secs.items():
            if not s["comparable"]:
                rep["not_comparable"].append((name, sname))
                continue
            if rep["err"] is None or s["err"] > rep["err"]:
                rep["err"], rep["at"] = s["err"], (name, sname)
            if tol is not None and s["err"] > tol:
                rep["above"].append((name, sname))
    return rep


def format_lines(rep: dict) -> list:
    """One line per table and section of a compare_dirs report, and per one-sided table."""
    lines = []
    for t in rep["tables"]:
        for sname, s in t["sections"].items():
            if not s["comparable"]:
                lines.append(f"{t['name']:>12s} {sname:14s} {s['reason']}")
                continue
            out = ", ".join(f"{k} has {o['points']} points outside the common range"
                            for k, o in (("A", s["outside_a"]), ("B", s["outside_b"])) if o["points"])
            flag = " ABOVE TOL" if rep["tol"] is not None and s["err"] > rep["tol"] else ""
            lines.append(f"{t['name']:>12s} {sname:14s} worst {s['err']:.3e} at {s['energy']:.6e} MeV (group {s['group']}, "
                         f"moment {s['moment']}); {s['queries']} queries, {s['moments']} moments per group"
                         f"{'; ' + out if out else ''}{flag}")
    for side, names in (("A", rep["only_in_a"]), ("B", rep["only_in_b"])):
        for n in names:
            lines.append(f"{n:>12s} only in {side}")
    return lines


def _num(x):
    """a float for JSON: inf as a string (json.dumps would write a bare Infinity)"""
    return x if x is None or math.isfinite(x) else str(x)


def as_json(rep: dict) -> dict:
    out = dict(rep, err=_num(rep["err"]), tables=[])
    for t in rep["tables"]:
        secs = {}
        for sname, s in t["sections"].items():
            secs[sname] = dict(s)
            if s["comparable"]:
                secs[sname].update(err=_num(s["err"]), worst=[[_num(float(v)) for v in row] for row in s["worst"]])
        out["tables"].append(dict(name=t["name"], sections=secs))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ndpp_amd.compare",
                                 description="The largest difference between the rows a consumer interpolates from two "
                                             "NDPP libraries, per table and section (exit 0: every comparable section "
                                             "within --tol, or no --tol; 1: a section above it; 2: input error; "
                                             "3: library or device error).")
    ap.add_argument("dir_a", help="directory holding library A's ndpp_lib.xml (or the xml file itself)")
    ap.add_argument("dir_b", help="the same for library B")
    ap.add_argument("--tol", metavar="T", default=None, help="exit 1 if a comparable section's worst error is above T")
    ap.add_argument("--json", default=None, help="write the full report to this file")
    a = ap.parse_args(argv)
    tol = None
    if a.tol is not None:
        try:
            tol = float(a.tol)
        except ValueError:
            tol = math.nan
        if not (tol >= 0.0) or not math.isfinite(tol):
            print(f"ndpp_amd.compare: input error: --tol {a.tol!r}: a finite number >= 0 is expected", file=sys.stderr)
            return EXIT_INPUT
    try:
        rep = compare_dirs(a.dir_a, a.dir_b, tol)
    except InputError as e:
        print(f"ndpp_amd.compare: input error: {e}", file=sys.stderr)
        return EXIT_INPUT
    except (lib.NdppError, RuntimeError, OSError) as e:
        print(f"ndpp_amd.compare: library error: {e}", file=sys.stderr)
        return EXIT_LIBRARY
    for line in format_lines(rep):
        print(line)
    n_sec = sum(len(t["sections"]) for t in rep["tables"])
    print(f"{len(rep['tables'])} tables in both, {len(rep['only_in_a'])} only in A, {len(rep['only_in_b'])} only in B; "
          f"{n_sec} sections, {len(rep['not_comparable'])} not comparable"
          + (f"; worst {rep['err']:.3e} in {rep['at'][0]} {rep['at'][1]}" if rep["err"] is not None else "")
          + (f"; {len(rep['above'])} above tol {tol:g}" if tol is not None else ""))
    if a.json:
        try:
            Path(a.json).write_text(json.dumps(as_json(rep), indent=1) + "\n")
        except OSError as e:
            print(f"ndpp_amd.compare: cannot write {a.json}: {e}", file=sys.stderr)
            return EXIT_LIBRARY
    return EXIT_ABOVE if rep["above"] else EXIT_OK


if __name__ == "__main__":
    sys.exit(main())
