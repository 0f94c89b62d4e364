"""Repair of negative Legendre rows, certified positive (ndpp_scatt_repair).

`validate --certified` names the (E_in, group) rows whose truncated expansion goes negative; this
module acts on that verdict.  A repaired row is a_l * w_l(t) with one parameter t in [0, 1]:

  heat     w_l = t^(l(l+1)/2)         the heat kernel on the sphere: damps the high orders first
  uniform  w_0 = 1, w_l = t (l >= 1)  the blend towards the isotropic row with the same P0

P0 is untouched bit for bit (so the band, sum_g P0, print_tol and condensation are), P1 is kept to
exactly the fraction t, and t is the largest value of a fixed-length bisection whose filtered row the
certificate of `validate.minimum` classes POSITIVE.  The rules for the rows are in include/ndpp_hip.h.

`weights` restates the multiplication order of the device in numpy, so `mat * weights(t, L, how)` is
the repaired row bit for bit.  `repair_sections` runs the repair over every Legendre section that
`validate` examines; `repair_result` does so on a result dict of lib.finish_scatt and returns the dict
the writer takes.  The report holds, per section, the rows repaired by family, the rows that could not
be, the smallest t and where, and the largest change under the metric of DESIGN.md section 12:
max over the elements of a row of |repaired - stored| over max_g |P0| of the row's E_in."""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass

import numpy as np

from . import lib
from .validate import _RESULT_KEYS, _sections_of

MODES = {"best": lib.REPAIR_BEST, "heat": lib.REPAIR_HEAT, "uniform": lib.REPAIR_UNIFORM}
_FAMILIES = {"heat": lib.HOW_HEAT, "uniform": lib.HOW_UNIFORM, lib.HOW_HEAT: lib.HOW_HEAT,
             lib.HOW_UNIFORM: lib.HOW_UNIFORM}


def weights(t, L: int, mode) -> np.ndarray:
    """w_l(t), l < L, of one family ("heat" / "uniform", or the `how` values 1 / 2), by the products
    the device makes, in its order: heat p = t; w_1 = t; then p = p * t; w_l = w_{l-1} * p; uniform
    w_l = t; w_0 = 1.  t: a scalar or an array; the result has shape t.shape + (L,)."""
    try:
        fam = _FAMILIES[mode if isinstance(mode, str) else int(mode)]
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"weights: {mode!r} is neither heat (1) nor uniform (2)") from None
    if L < 1:
        raise ValueError(f"weights: L = {L} must be at least 1")
    t = np.asarray(t, dtype=np.float64)
    w = np.ones(t.shape + (int(L),))
    p = t.copy()
    for l in range(1, int(L)):
        if l == 1 or fam == lib.HOW_UNIFORM:
            w[..., l] = t
        else:
            p = p * t
            w[..., l] = w[..., l - 1] * p
    return w


@dataclass
class RepairSection:
    """repair of one section: ndpp_repair's fields and the largest change."""
    rows: int
    repaired: int
    heat: int
    uniform: int
    unrepairable: int
    nonfinite: int
    min_t: float
    min_ein: int
    min_group: int
    max_change: float          # max over E_in of max_e |out - mat| / max_g |P0|; 0 when nothing changed
    max_change_ein: int        # the row attaining it; -1, -1 when nothing changed
    max_change_group: int


@dataclass
class RepairReport:
    """repair_sections() of a table or result: one RepairSection per Legendre section present."""
    sections: dict
    mode: str
    steps: int
    rel_tol: float
    undecided: bool

    @property
    def repaired(self) -> int:
        return sum(s.repaired for s in self.sections.values())

    @property
    def max_change(self) -> float:
        return max((s.max_change for s in self.sections.values()), default=0.0)

    def as_dict(self) -> dict:
        return {"mode": self.mode, "steps": self.steps, "rel_tol": self.rel_tol, "undecided": self.undecided,
                "repaired": self.repaired, "max_change": self.max_change,
                "sections": {k: asdict(s) for k, s in self.sections.items()}}


def largest_change(mat, out):
    """(max over rows of max_e |out - mat| / max_g |P0| of the row's E_in, iE, g) -- the metric of
    DESIGN.md section 12 on the change a repair made; (0.0, -1, -1) when nothing changed.  Rows that
    hold a NaN or an infinity are copied unchanged and take no part."""
    mat, out = np.asarray(mat, dtype=np.float64), np.asarray(out, dtype=np.float64)
    if mat.size == 0:
        return 0.0, -1, -1
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(mat) & np.isfinite(out), np.abs(out - mat), 0.0).max(axis=2)
        scale = np.nanmax(np.abs(np.where(np.isfinite(mat[:, :, 0]), mat[:, :, 0], 0.0)), axis=1)
    rel = np.divide(d, scale[:, None], out=np.zeros_like(d), where=scale[:, None] > 0)
    k = int(np.argmax(rel))
    if rel.flat[k] == 0.0:
        return 0.0, -1, -1
    iE, g = np.unravel_index(k, rel.shape)
    return float(rel[iE, g]), int(iE), int(g)


def _mode_name(mode) -> str:
    if isinstance(mode, str):
        if mode.lower() not in MODES:
            raise ValueError(f"repair mode {mode!r} is none of best, heat, uniform")
        return mode.lower()
    for name, v in MODES.items():
        if v == int(mode):
            return name
    raise ValueError(f"repair mode {mode!r} is none of best (0), heat (1), uniform (2)")


def repair_sections(obj, mode="best", steps: int = 20, rel_tol: float = 1e-10, undecided: bool = False):
    """ndpp_scatt_repair over every Legendre section `validate.minimum` examines.  obj: a
    reader.NdppTable (elastic, inelastic, nu-inelastic; a thermal table's matrix is its elastic
    section), a result dict of lib.scatt_nuclide / lib.finish_scatt, or one (NE, G, L) section
    (reported as "section").  Returns ({section: dict(mat=repaired (NE, G, L), t=(NE, G), how=(NE, G))},
    RepairReport)."""
    name = _mode_name(mode)
    out, secs = {}, {}
    for sec, mat in _sections_of(obj).items():
        s, rep, t, how = lib.scatt_repair(mat, mode=MODES[name], steps=int(steps), undecided=bool(undecided),
                                          rel_tol=float(rel_tol))
        change, iE, g = largest_change(mat, rep)
        out[sec] = dict(mat=rep, t=t, how=how)
        secs[sec] = RepairSection(int(s.rows), int(s.repaired), int(s.heat), int(s.uniform), int(s.unrepairable),
                                  int(s.nonfinite), float(s.min_t), int(s.min_ein), int(s.min_group), change, iE, g)
    return out, RepairReport(secs, name, int(steps), float(rel_tol), bool(undecided))


def repair_result(result: dict, **kw):
    """repair_sections on a result dict of lib.finish_scatt: (the dict with its matrices repaired --
    grids and everything else shared with `result` -- and the RepairReport)."""
    secs, rep = repair_sections(result, **kw)
    new = dict(result)
    for sec, v in secs.items():
        new[_RESULT_KEYS[sec]] = v["mat"]
    return new, rep


def format_lines(name: str, report: RepairReport) -> list:
    """one line per section: what the repair did to table `name`"""
    lines = []
    for sec, s in report.sections.items():
        line = (f"{name:>12s} {sec:12s} repaired {s.repaired} of {s.rows} rows ({report.mode}: heat {s.heat}, "
                f"uniform {s.uniform}), unrepairable {s.unrepairable}, non-finite {s.nonfinite}")
        if s.repaired:
            line += (f", smallest t {s.min_t:.6f} at E_in {s.min_ein + 1}, group {s.min_group + 1}, largest change "
                     f"{s.max_change:.3e} at E_in {s.max_change_ein + 1}, group {s.max_change_group + 1}")
        lines.append(line)
    return lines


def check_options(steps, rel_tol) -> None:
    """the command lines' refusals; raises ValueError"""
    if not 1 <= int(steps) <= 52:
        raise ValueError(f"--repair-steps {steps}: must be between 1 and 52")
    if not (rel_tol >= 0.0 and math.isfinite(rel_tol)):
        raise ValueError(f"--repair-rel-tol {rel_tol}: must be a finite value >= 0")
