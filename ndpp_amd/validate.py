"""Validation of NDPP libraries: outgoing-group condensation, Legendre expansion of the stored
moments, and the positivity check -- the library interface of the reference's user guide
(docs/source/usersguide/utilities.rst; src/utils/ndpp_data.py:272-396, driven over a library by
src/utils/validate_library.py), on the GPU (include/ndpp_hip.h: ndpp_expand_moments,
ndpp_scatt_positivity).

Rules (tests/test_validate.py and tests/test_gpu_validate.py pin them):

* Grid: mu_j = numpy.linspace(-1, 1, M).  M defaults to 21 for `positivity` (as
  validate_library.py) and to 201 for `expand` (as expand_scatt).
* f(mu_j) = sum_{l < n_moments} (l + 1/2) P_l(mu_j) a_l.  n_moments defaults to L =
  scatt_order + 1; a larger value is cut to L (the reference's min(order, scatt_order)).
* Band: for each E_in the rows g = gmin..gmax, the first and last groups with P0 > 0 -- the
  writer's rule, so for a file read back these are exactly the file's gmin / gmax.  Interior
  rows with P0 <= 0 are checked.  An E_in without any P0 > 0 is one zero row: it counts in
  `rows`, its value is 0.0 and it is never negative; its group is reported as -1 (the reference
  stores such an E_in as gmin = gmax = -1).
* Negative means !(f >= 0) at some grid point, so NaN moments are reported and never pass.
  min_value is the smallest non-NaN f (+inf if there is none).

The sampled check is a sample, not a proof: a dip of f between two grid points passes it (at M = 21
the spacing is 0.1, and f(mu) = (mu - 0.05)^2 - 1e-4 is +0.0024 at its smallest grid value).
`minimum` is the check that cannot miss: per row a certified enclosure lo <= min f <= hi with the
cosine attaining hi (ndpp_scatt_minimum), `--certified` on the command line.

Deviations from the reference utilities, on purpose:

* test_scatt_positivity reports (iE, g + gmin), which counts the band offset twice; the
  offending rows here are (iE, g), g the 0-based group.
* condense_outgoing_scatt sizes its result with an undefined name (Nein); `condense` here
  returns (NE, L) for the section it is given.
* validate_library.py calls test_scatt_positivity without its required `dtype`; the CLI here
  checks every scatter section of every table (elastic, inelastic, nu-inelastic).

CLI: python -m ndpp_amd.validate <dir with ndpp_lib.xml> [--mu-points 21] [--moments N]
[--json FILE]; exit 0 if every section is positive, 1 if any row is negative, 2 on an input
error (or when the check cannot run: no device).  With --certified [--rel-tol 1e-10] the Legendre
tables go through `minimum` (tabular ones keep tab_positivity): exit 1 if any row is negative or
non-finite; undecided and unsettled rows are counted and printed and do not fail the run.
--certified does not go together with --mu-points (exit 2).
--certified --repair-report adds to each section's line what `python -m ndpp_amd.run
--repair-positivity` would do to it (ndpp_amd.repair, defaults: rows by family, smallest t, largest
change); nothing is written and the exit status stays that of --certified.  Without --certified, or
with --moments (the repair acts on the stored rows, all moments), it is an input error (exit 2).
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import asdict, dataclass, field
from pathlib import Path

import numpy as np

from . import lib, reader

SECTIONS = ("elastic", "inelastic", "nuinelastic")
_RESULT_KEYS = {"elastic": "el_mat", "inelastic": "inel_mat", "nuinelastic": "nuinel_mat"}


@dataclass
class SectionReport:
    rows: int
    negative: int
    min_value: float
    min_ein: int
    min_group: int
    offending: list = field(default_factory=list)     # [(iE, g)] in (iE, g) order, 0-based
    offending_min: list = field(default_factory=list)  # the row's smallest non-NaN f (NaN if none)
    offending_mu: list = field(default_factory=list)   # index of that minimum on the mu grid

    @property
    def positive(self) -> bool:
        return self.negative == 0


@dataclass
class Report:
    """positivity() of a table or result: one SectionReport per scatter section present."""
    sections: dict
    mu_points: int
    n_moments: int

    @property
    def positive(self) -> bool:
        return all(s.positive for s in self.sections.values())

    @property
    def min_value(self) -> float:
        return min((s.min_value for s in self.sections.values()), default=math.inf)

    @property
    def offending(self) -> dict:
        return {k: s.offending for k, s in self.sections.items()}

    def as_dict(self) -> dict:
        return {"positive": self.positive, "min_value": _num(self.min_value), "mu_points": self.mu_points,
                "n_moments": self.n_moments,
                "sections": {k: _section_dict(s) for k, s in self.sections.items()}}


def _num(x: float):
    """a float for JSON: nan / inf as strings (json.dumps would write bare NaN / Infinity)"""
    return x if math.isfinite(x) else str(x)


def _section_dict(s: SectionReport) -> dict:
    d = asdict(s)
    d["positive"] = s.positive
    d["min_value"] = _num(s.min_value)
    d["offending_min"] = [_num(v) for v in s.offending_min]
    return d


def _matrix(section) -> np.ndarray:
    m = section.mat if isinstance(section, reader.ScattSection) else section
    m = np.asarray(m, dtype=np.float64)
    if m.ndim != 3:
        raise ValueError(f"a scatter section is (NE, G, L), got shape {m.shape}")
    return m


def condense(section, groups=None) -> np.ndarray:
    """Sum of the selected outgoing groups' moments per E_in, (NE, L) (condense_outgoing_scatt,
    ndpp_data.py:272-303).  section: reader.ScattSection or a dense (NE, G, L) array; groups:
    0-based, None for all.  The sum runs over ascending g from 0.0, vectorised over E_in -- the
    reference's order of operations, so the result equals its loop bit for bit.  Host numpy:
    O(NE G L), no kernel."""
    mat = _matrix(section)
    NE, G, L = mat.shape
    sel = range(G) if groups is None else sorted({int(g) for g in np.atleast_1d(groups)})
    for g in sel:
        if not 0 <= g < G:
            raise ValueError(f"group {g} outside 0..{G - 1}")
    out = np.zeros((NE, L))
    for g in sel:
        out = out + mat[:, g]
    return out


def expand(moments, mu_points: int = 201, n_moments=None):
    """f[iE][j] = sum_{l < n_moments} (l + 1/2) P_l(mu_j) moments[iE][l] on mu =
    linspace(-1, 1, mu_points), on the GPU (expand_scatt, ndpp_data.py:305-343).  moments:
    (NE, L), e.g. one group's moments or condense()'s.  Returns (f (NE, M), mu)."""
    mom = np.asarray(moments, dtype=np.float64)
    nm = None if n_moments is None else min(int(n_moments), mom.shape[1])
    return lib.expand_moments(mom, n_moments=nm, mu_points=int(mu_points))


def _sections_of(obj) -> dict:
    if isinstance(obj, reader.NdppTable):
        return {k: getattr(obj, k).mat for k in SECTIONS if getattr(obj, k) is not None}
    if isinstance(obj, dict):            # lib.scatt_nuclide / lib.finish_scatt result
        return {k: np.asarray(obj[v]) for k, v in _RESULT_KEYS.items()
                if obj.get(v) is not None and len(obj[v])}
    return {"section": _matrix(obj)}


def tab_positivity(obj, cap: int = 1000) -> Report:
    """The positivity check of a TABULAR table (scatt_type 1: N lab-cosine bins per group, no
    Legendre expansion): on the host, every entry that is < 0 or NaN counts as negative.  obj: a
    reader.NdppTable, a scatt_nuclide_tab / finish_scatt result dict or one (NE, G, N) section.
    Every (E_in, group) is a row; a row is offending when any of its bins is; offending_min is
    its smallest non-NaN bin (NaN if none) and offending_mu that bin's index.  `negative` counts
    entries.  The Report has the shape of positivity()'s, with n_moments = N and mu_points = 0."""
    secs = _sections_of(obj)
    out = {}
    N = 0
    for name, mat in secs.items():
        NE, G, N = mat.shape
        bad = ~(mat >= 0.0)
        fin = np.where(np.isnan(mat), np.inf, mat)
        mn = float(fin.min()) if mat.size else math.inf
        if mat.size and math.isfinite(mn):
            iE, g, _ = np.unravel_index(int(np.argmin(fin)), mat.shape)
        else:
            iE = g = -1
        rows_bad = np.argwhere(bad.any(axis=2))[:cap]
        omin = [float(fin[i, j].min()) if np.isfinite(fin[i, j]).any() else math.nan for i, j in rows_bad]
        omu = [int(np.argmax(bad[i, j])) for i, j in rows_bad]
        out[name] = SectionReport(int(NE * G), int(bad.sum()), mn, int(iE), int(g),
                                  [(int(i), int(j)) for i, j in rows_bad], omin, omu)
    return Report(out, 0, int(N))


def positivity(obj, mu_points: int = 21, n_moments=None) -> Report:
    """The positivity check (test_scatt_positivity, ndpp_data.py:345-396) on the GPU.
    obj: reader.NdppTable (elastic, inelastic and nu-inelastic), a result dict of
    lib.scatt_nuclide / lib.finish_scatt (band found from the dense matrix, as the writer finds
    it, so a result and its file read back give the same report), or one section
    (reader.ScattSection or a (NE, G, L) array, reported as "section").  Rules: module docstring.
    Returns a Report: .positive, .offending {section: [(iE, g)]}, .min_value, .sections."""
    secs = _sections_of(obj)
    L = max((m.shape[2] for m in secs.values()), default=0)
    nm = L if n_moments is None else min(int(n_moments), L)
    out = {}
    for name, mat in secs.items():
        s, rows, rmin, rmu = lib.scatt_positivity(mat, n_moments=min(nm, mat.shape[2]), mu_points=int(mu_points))
        out[name] = SectionReport(int(s.rows), int(s.negative), float(s.min_value), int(s.min_ein),
                                  int(s.min_group), [tuple(int(v) for v in r) for r in rows],
                                  [float(v) for v in rmin], [int(v) for v in rmu])
    return Report(out, int(mu_points), nm)


@dataclass
class MinimumSection:
    """minimum() of one section: ndpp_minimum's fields and the first `cap` negative or non-finite rows."""
    rows: int
    negative: int
    undecided: int
    nonfinite: int
    unsettled: int
    min_hi: float
    min_mu: float
    min_ein: int
    min_group: int
    offending: list = field(default_factory=list)      # [(iE, g)] in (iE, g) order, 0-based
    offending_hi: list = field(default_factory=list)    # the row's hi (NaN for a non-finite row)
    offending_mu: list = field(default_factory=list)    # the cosine attaining it

    @property
    def positive(self) -> bool:
        return self.negative == 0 and self.nonfinite == 0


@dataclass
class MinimumReport:
    """minimum() of a table or result: one MinimumSection per scatter section present."""
    sections: dict
    n_moments: int
    rel_tol: float

    @property
    def positive(self) -> bool:
        return all(s.positive for s in self.sections.values())

    @property
    def min_hi(self) -> float:
        return min((s.min_hi for s in self.sections.values()), default=math.inf)

    @property
    def offending(self) -> dict:
        return {k: s.offending for k, s in self.sections.items()}

    def as_dict(self) -> dict:
        secs = {}
        for k, s in self.sections.items():
            d = asdict(s)
            d["positive"] = s.positive
            d["min_hi"] = _num(s.min_hi)
            d["offending_hi"] = [_num(v) for v in s.offending_hi]
            secs[k] = d
        return {"certified": True, "positive": self.positive, "min_hi": _num(self.min_hi),
                "n_moments": self.n_moments, "rel_tol": self.rel_tol, "sections": secs}


def minimum(obj, n_moments=None, rel_tol: float = 1e-10, cap: int = 1000) -> MinimumReport:
    """The certified positivity check on the GPU (ndpp_scatt_minimum): for every row `positivity`
    examines, an enclosure lo <= min over [-1, 1] of f <= hi with the cosine attaining hi, so a row
    reported positive IS positive and a negative one comes with a witness.  obj: what `positivity`
    accepts.  Returns a MinimumReport; per section the counts (rows, negative, undecided: the minimum
    is within the tolerance of zero, nonfinite, unsettled: the evaluation cap was reached), the
    smallest hi with its cosine and row, and the first `cap` negative or non-finite rows with their
    hi and mu_at."""
    secs = _sections_of(obj)
    L = max((m.shape[2] for m in secs.values()), default=0)
    nm = L if n_moments is None else min(int(n_moments), L)
    out = {}
    for name, mat in secs.items():
        s, _, hi, mu_at, cls = lib.scatt_minimum(mat, n_moments=min(nm, mat.shape[2]), rel_tol=float(rel_tol))
        kind = cls & 3
        bad = np.argwhere((cls >= 0) & ((kind == lib.MIN_NEGATIVE) | (kind == lib.MIN_NONFINITE)))[:int(cap)]
        out[name] = MinimumSection(int(s.rows), int(s.negative), int(s.undecided), int(s.nonfinite),
                                   int(s.unsettled), float(s.min_hi), float(s.min_mu), int(s.min_ein),
                                   int(s.min_group), [(int(i), int(g)) for i, g in bad],
                                   [float(hi[i, g]) for i, g in bad], [float(mu_at[i, g]) for i, g in bad])
    return MinimumReport(out, nm, float(rel_tol))


def minimum_reference(row, n_moments=None):
    """Host reference of one row's minimum: (min over [-1, 1] of f, the cosine attaining it), from the
    real roots of f' inside (-1, 1) (numpy.polynomial.legendre: legder, legroots) and both ends,
    evaluated with legval; the first cosine in ascending order on a tie."""
    from numpy.polynomial import legendre as leg
    a = np.asarray(row, dtype=np.float64)
    nm = len(a) if n_moments is None else min(int(n_moments), len(a))
    c = (np.arange(nm) + 0.5) * a[:nm]
    cand = [-1.0, 1.0]
    d = np.trim_zeros(leg.legder(c), "b") if nm > 1 else np.zeros(0)
    if len(d) > 1:
        r = leg.legroots(d)
        r = r[np.abs(r.imag) <= 1e-9 * np.maximum(1.0, np.abs(r.real))].real if np.iscomplexobj(r) else r
        cand += [float(x) for x in r if -1.0 < x < 1.0]
    cand = np.array(sorted(cand))
    f = leg.legval(cand, c)
    k = int(np.argmin(f))
    return float(f[k]), float(cand[k])


def read_library(directory) -> list:
    """[(table attributes, NdppTable)] of every table ndpp_lib.xml lists, read with reader.py
    (BINARY or ASCII per <filetype>); paths are relative to the directory of ndpp_lib.xml."""
    d = Path(directory)
    xml = d / "ndpp_lib.xml" if d.is_dir() else d
    meta = reader.read_lib_xml(xml.read_bytes())
    ftype = meta.get("filetype", "binary").lower()
    if ftype not in ("binary", "ascii"):
        raise ValueError(f"{xml}: filetype {ftype!r} is neither binary nor ascii")
    read = reader.read_binary if ftype == "binary" else reader.read_ascii
    return [(t, read((xml.parent / t["path"]).read_bytes())) for t in meta["tables"]]


def _print_report(name: str, t: reader.NdppTable, rep: Report, out) -> None:
    status = "positive" if rep.positive else "NEGATIVE"
    if t.scatt_type == reader.SCATT_TYPE_TABULAR:
        print(f"{name}: {status}  (tabular, {t.groups} groups, {rep.n_moments} bins)", file=out)
        for sec, s in rep.sections.items():
            where = f" at E_in {s.min_ein + 1}, group {s.min_group + 1}" if s.min_group >= 0 else ""
            print(f"  {sec:12s} rows {s.rows:7d}  negative {s.negative:7d}  min {s.min_value: .6e}{where}", file=out)
            for (iE, g), v, k in list(zip(s.offending, s.offending_min, s.offending_mu))[:10]:
                print(f"      E_in {iE + 1:6d} ({_ein(t, sec, iE):.6e} MeV)  group {g + 1:4d}  "
                      f"min {v: .6e}, first in bin {k + 1}", file=out)
        return
    print(f"{name}: {status}  (P{t.scatt_order}, {t.groups} groups, {rep.n_moments} moments, "
          f"{rep.mu_points} mu points)", file=out)
    for sec, s in rep.sections.items():
        where = (f" at E_in {s.min_ein + 1}, group {s.min_group + 1}" if s.min_group >= 0 else
                 (f" at E_in {s.min_ein + 1} (all-zero)" if s.min_ein >= 0 else ""))
        print(f"  {sec:12s} rows {s.rows:7d}  negative {s.negative:7d}  min {s.min_value: .6e}{where}", file=out)
        for (iE, g), v, j in list(zip(s.offending, s.offending_min, s.offending_mu))[:10]:
            print(f"      E_in {iE + 1:6d} ({_ein(t, sec, iE):.6e} MeV)  group {g + 1:4d}  "
                  f"min {v: .6e} at mu = {np.linspace(-1, 1, rep.mu_points)[j]: .4f}", file=out)
        if s.negative > 10:
            print(f"      ... {s.negative - 10} more", file=out)


def _print_minimum(name: str, t: reader.NdppTable, rep: MinimumReport, out, repair_rep=None) -> None:
    status = "positive" if rep.positive else "NEGATIVE"
    print(f"{name}: {status}  (P{t.scatt_order}, {t.groups} groups, {rep.n_moments} moments, certified, "
          f"rel tol {rep.rel_tol:g})", file=out)
    for sec, s in rep.sections.items():
        where = (f" at mu = {s.min_mu: .6f}, E_in {s.min_ein + 1}, group {s.min_group + 1}" if s.min_group >= 0 else
                 (f" at E_in {s.min_ein + 1} (all-zero)" if s.min_ein >= 0 else ""))
        print(f"  {sec:12s} rows {s.rows:7d}  negative {s.negative:7d}  non-finite {s.nonfinite:7d}  "
              f"undecided {s.undecided:7d}  unsettled {s.unsettled:7d}  min {s.min_hi: .6e}{where}", file=out)
        for (iE, g), v, mu in list(zip(s.offending, s.offending_hi, s.offending_mu))[:10]:
            what = "non-finite moments" if math.isnan(v) else f"f = {v: .6e} at mu = {mu: .6f}"
            print(f"      E_in {iE + 1:6d} ({_ein(t, sec, iE):.6e} MeV)  group {g + 1:4d}  {what}", file=out)
        if s.negative + s.nonfinite > 10:
            print(f"      ... {s.negative + s.nonfinite - 10} more", file=out)
        if repair_rep is not None and sec in repair_rep.sections:
            r = repair_rep.sections[sec]
            what = (f", smallest t {r.min_t:.6f} at E_in {r.min_ein + 1}, group {r.min_group + 1}, largest change "
                    f"{r.max_change:.3e}" if r.repaired else "")
            print(f"      a repair ({repair_rep.mode}, {repair_rep.steps} steps) would change {r.repaired} rows: heat "
                  f"{r.heat}, uniform {r.uniform}; unrepairable {r.unrepairable}, non-finite {r.nonfinite}{what}",
                  file=out)


def _ein(t: reader.NdppTable, sec: str, iE: int) -> float:
    return float(getattr(t, sec).ein[iE])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ndpp_amd.validate",
                                 description="Check every scatter section of an NDPP library for negative "
                                             "Legendre expansions (exit 0: all positive, 1: negative rows, "
                                             "2: input error or no device).")
    ap.add_argument("library", help="directory holding ndpp_lib.xml (or the xml file itself)")
    ap.add_argument("--mu-points", type=int, default=None, help="points of linspace(-1, 1, M) (default 21)")
    ap.add_argument("--moments", type=int, default=None, help="moments to sum (default: all, scatt_order + 1)")
    ap.add_argument("--json", default=None, help="write the full report to this file")
    ap.add_argument("--certified", action="store_true",
                    help="enclose every row's true minimum instead of sampling a grid (not with --mu-points); "
                         "exit 1 if any row is negative or non-finite")
    ap.add_argument("--rel-tol", type=float, default=None,
                    help="with --certified: width of a settled enclosure relative to sum (l + 1/2)|a_l| "
                         "(default 1e-10)")
    ap.add_argument("--repair-report", action="store_true",
                    help="with --certified: add to each section what a repair of its negative rows would do "
                         "(python -m ndpp_amd.run --repair-positivity); writes nothing")
    a = ap.parse_args(argv)
    if a.repair_report and not a.certified:
        print("validate: --repair-report needs --certified", file=sys.stderr)
        return 2
    if a.repair_report and a.moments is not None:
        print("validate: --repair-report describes the repair of the stored rows, all moments: it does not go "
              "together with --moments", file=sys.stderr)
        return 2
    if a.certified and a.mu_points is not None:
        print("validate: --certified examines the whole interval; it does not go together with --mu-points",
              file=sys.stderr)
        return 2
    if a.rel_tol is not None and not a.certified:
        print("validate: --rel-tol needs --certified", file=sys.stderr)
        return 2
    if a.rel_tol is not None and not (a.rel_tol >= 0.0 and math.isfinite(a.rel_tol)):
        print("validate: --rel-tol must be a finite value >= 0", file=sys.stderr)
        return 2
    rel_tol = 1e-10 if a.rel_tol is None else a.rel_tol
    if a.mu_points is None:
        a.mu_points = 21
    if a.mu_points < 1 or (a.moments is not None and a.moments < 1):
        print("validate: --mu-points and --moments must be at least 1", file=sys.stderr)
        return 2
    try:
        tables = read_library(a.library)
    except (OSError, ValueError, KeyError, IndexError) as e:
        print(f"validate: cannot read the library at {a.library}: {e}", file=sys.stderr)
        return 2
    full, bad = {}, []
    for attrs, t in tables:
        name = attrs.get("name", t.name)
        repair_rep = None
        try:
            if t.scatt_type == reader.SCATT_TYPE_TABULAR:
                rep = tab_positivity(t)
            elif a.certified:
                rep = minimum(t, n_moments=a.moments, rel_tol=rel_tol)
                if a.repair_report:
                    from . import repair
                    _, repair_rep = repair.repair_sections(t, rel_tol=rel_tol)
            else:
                rep = positivity(t, mu_points=a.mu_points, n_moments=a.moments)
        except lib.NdppError as e:
            print(f"validate: {name}: {e}", file=sys.stderr)
            return 2
        if isinstance(rep, MinimumReport):
            _print_minimum(name, t, rep, sys.stdout, repair_rep)
        else:
            _print_report(name, t, rep, sys.stdout)
        full[name] = dict(rep.as_dict(), path=attrs.get("path"))
        if repair_rep is not None:
            full[name]["repair"] = repair_rep.as_dict()
        if not rep.positive:
            bad.append(name)
    print(f"{len(tables)} tables, {len(bad)} with negative" + (" or non-finite" if a.certified else "") + " rows"
          + (": " + ", ".join(bad) if bad else ""))
    if a.json:
        head = {"library": str(a.library), "positive": not bad}
        if a.certified:
            head.update(certified=True, rel_tol=rel_tol)
        Path(a.json).write_text(json.dumps(dict(head, tables=full), indent=1) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
