"""Sample an outgoing group and a scattering cosine from a library section, as a transport code does
(include/ndpp_hip.h: ndpp_scatt_sample).

At an incoming energy the section is read linearly in ln E (the rule of ndpp_lib_compare): the group
is drawn from the blended group masses, the cosine from the blended row of that group by inverting
its cumulative distribution -- exactly for cosine bins, by 53 bisection steps of the closed-form
integral of the Legendre expansion for moments.  The identity this gives is the consumer's: the
moments (or the bin histogram) of what is drawn are the moments (or bins) in the file.  It holds for
a row that is a distribution.  A Legendre row that is negative somewhere is sampled WITHOUT a flag
(the bisection ends where the CDF rises, never inside a dip; NEGDENSITY only catches a density that
does not evaluate): check with `python -m ndpp_amd.validate DIR --certified` and write the library
with `python -m ndpp_amd.run --repair-positivity` first.

  sample_numpy(scatt_type, x, y, ein, u_g, u_mu)  host restatement of ndpp_scatt_sample: the same
                          operations in the same order, the same bits (group, mu, status)
  sample_section(section, scatt_type, ein, u_g, u_mu, sample=None)  one reader.ScattSection (or
                          (x, y)) on the device (lib.scatt_sample) unless `sample` is given
  expectations(section, scatt_type, ein)  at one energy the exact probabilities of the blended row:
                          p[G] = w_g / W and shape[G][L] = a_l / a_0 (Legendre) or t_k / T (tabular),
                          NaN in the rows of groups that are never drawn
  check_energy(...)       draws against expectations, each difference in units of its standard error

CLI: python -m ndpp_amd.sample DIR --table NAME [--section elastic|inelastic|nuinelastic]
--energy E [E ...] [--events 200000] [--seed 1] [--json FILE]; per energy and group the sampled
fraction against w_g / W and the sampled mean of P_1 .. P_{L-1}(mu) (Legendre) or the bin histogram
(tabular) against the row, in standard errors; exit 0, 1 if an event was BADROW or NEGDENSITY, 2 on an
input error, 3 on a library or device error.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np

from . import lib, reader
from .compare import InputError, grid_ok, read_library, _brackets, _num, _xy
from .lib import SAMPLE_BADROW, SAMPLE_NEGDENSITY, SAMPLE_OK, SAMPLE_SKIPPED, SAMPLE_ZEROROW

EXIT_OK, EXIT_FLAGGED, EXIT_INPUT, EXIT_LIBRARY = 0, 1, 2, 3
SECTIONS = ("elastic", "inelastic", "nuinelastic")
STATUS_NAMES = {SAMPLE_OK: "ok", SAMPLE_SKIPPED: "skipped", SAMPLE_BADROW: "badrow", SAMPLE_ZEROROW: "zerorow",
                SAMPLE_NEGDENSITY: "negdensity"}
BISECTIONS = 53
_BLOCK = 1 << 16       # events sample_numpy handles at a time


def _masses(scatt_type, y):
    """s[n][G]: P0, or the sum of the bins in ascending k from 0.0"""
    if scatt_type == reader.SCATT_TYPE_LEGENDRE:
        return y[:, :, 0].copy()
    s = np.zeros(y.shape[:2])
    for k in range(y.shape[2]):
        s = s + y[:, :, k]
    return s


def _bad_mass(v):
    return ~(v >= 0.0) | ~(v < np.inf)


def _pick(w, u):
    """rows of masses w[B][K] and u[B]: (bad, total, index).  index: the smallest k whose running sum
    exceeds u * total, else the last k with w > 0 (-1: none); also the running sum below it and w there"""
    B, K = w.shape
    bad = np.zeros(B, dtype=bool)
    last = np.full(B, -1)
    tot = np.zeros(B)
    for k in range(K):
        bad |= _bad_mass(w[:, k])
        last = np.where(w[:, k] > 0.0, k, last)
        tot = tot + w[:, k]
    bad |= ~(tot < np.inf)
    target = u * tot
    c, pick = np.zeros(B), np.full(B, -1)
    below, at = np.zeros(B), np.zeros(B)
    for k in range(K):
        cn = c + w[:, k]
        take = (pick < 0) & ((cn > target) | (k == last))
        pick = np.where(take, k, pick)
        below = np.where(take, c, below)
        at = np.where(take, w[:, k], at)
        c = cn
    return bad, tot, target, pick, below, at


def _legendre_cdf(a, m):
    """F(m) of the header for rows a[B][L] at m[B], Bonnet upwards in the written order"""
    L = a.shape[1]
    F = (0.5 * a[:, 0]) * (m + 1.0)
    pm, p = np.ones_like(m), m
    for l in range(1, L):
        pn = ((float(2 * l + 1) / float(l + 1)) * m) * p - (float(l) / float(l + 1)) * pm
        F = F + (0.5 * a[:, l]) * (pn - pm)
        pm, p = p, pn
    return F


def _legendre_density(a, mu):
    """sum_l ((l + 1/2) a_l) P_l(mu) in ascending l from 0.0"""
    L = a.shape[1]
    d = np.zeros_like(mu)
    pm, p = np.ones_like(mu), mu
    for l in range(L):
        d = d + ((float(l) + 0.5) * a[:, l]) * pm
        pn = ((float(2 * l + 3) / float(l + 2)) * mu) * p - (float(l + 1) / float(l + 2)) * pm
        pm, p = p, pn
    return d


def sample_numpy(scatt_type, x, y, ein, u_g, u_mu):
    """ndpp_scatt_sample on the host (include/ndpp_hip.h): (group[n_ev] int32, mu[n_ev], status[n_ev]
    int32).  Everything after the logarithms is IEEE + - * / elementwise in the kernels' order."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ein, u_g, u_mu = (np.asarray(v, dtype=np.float64).ravel() for v in (ein, u_g, u_mu))
    if scatt_type not in (reader.SCATT_TYPE_LEGENDRE, reader.SCATT_TYPE_TABULAR):
        raise ValueError(f"scatt_type {scatt_type!r} is neither 0 (Legendre) nor 1 (tabular)")
    if y.ndim != 3 or x.shape != (y.shape[0],) or not (len(ein) == len(u_g) == len(u_mu)):
        raise ValueError(f"shapes do not match: x {x.shape}, y {y.shape}, events {len(ein)}, {len(u_g)}, {len(u_mu)}")
    n, G, L = y.shape
    Lmax = lib.NDPP_MAX_TAB_BINS if scatt_type == reader.SCATT_TYPE_TABULAR else lib.NDPP_MAX_ORDER
    if not 1 <= L <= Lmax or G < 1:
        raise ValueError(f"G = {G}, L = {L}: need G >= 1 and 1 <= L <= {Lmax}")
    if not grid_ok(x):
        raise ValueError("the grid must be strictly increasing, positive and finite, with two points or more")
    n_ev = len(ein)
    group, mu = np.full(n_ev, -1, dtype=np.int32), np.zeros(n_ev)
    status = np.full(n_ev, SAMPLE_SKIPPED, dtype=np.int32)
    with np.errstate(all="ignore"):
        ok = (np.isfinite(ein) & (ein > 0.0) & (ein >= x[0]) & (ein <= x[-1]) & (u_g >= 0.0) & (u_g < 1.0)
              & (u_mu >= 0.0) & (u_mu < 1.0))
        i_all, f_all = _brackets(x, ein, ok)
        s = _masses(scatt_type, y)
        live = np.flatnonzero(ok)
        for at in range(0, len(live), _BLOCK):
            q = live[at:at + _BLOCK]
            g, m, st = _sample_block(scatt_type, y, s, i_all[q], f_all[q], u_g[q], u_mu[q])
            group[q], mu[q], status[q] = g, m, st
    return group, mu, status


def _sample_block(scatt_type, y, s, i, f, ug, umu):
    n, G, L = y.shape
    B = len(i)
    i1 = np.minimum(i + 1, n - 1)
    s0, s1 = s[i], s[i1]
    bad, W, _, g, _, _ = _pick(s0 + (s1 - s0) * f[:, None], ug)
    status = np.where(bad, SAMPLE_BADROW, np.where(W == 0.0, SAMPLE_ZEROROW, SAMPLE_OK)).astype(np.int32)
    group, mu = np.full(B, -1, dtype=np.int32), np.zeros(B)
    q = np.flatnonzero(status == SAMPLE_OK)
    if not len(q):
        return group, mu, status
    gq, fq = g[q], f[q]
    r0, r1 = y[i[q], gq], y[i1[q], gq]
    a = r0 + (r1 - r0) * fq[:, None]
    if scatt_type == reader.SCATT_TYPE_TABULAR:
        bad, T, target, k, below, tk = _pick(a, umu[q])
        st = np.where(bad, SAMPLE_BADROW, np.where(T == 0.0, SAMPLE_ZEROROW, SAMPLE_OK))
        good = st == SAMPLE_OK
        h = 2.0 / float(L)
        kk = np.where(good, k, 0).astype(np.float64)
        left = -1.0 + h * kk
        right = np.where(k == L - 1, 1.0, -1.0 + h * (kk + 1.0))
        m = -1.0 + h * (kk + (target - below) / np.where(good, tk, 1.0))
        m = np.where(m < left, left, m)
        m = np.where(m > right, right, m)
        mu[q] = np.where(good, m, 0.0)
    else:
        good = (np.abs(a) < np.inf).all(axis=1)
        st = np.where(good, SAMPLE_OK, SAMPLE_BADROW)
        a = np.where(good[:, None], a, 0.0)
        target = umu[q] * a[:, 0]
        lo, hi = np.full(len(q), -1.0), np.ones(len(q))
        for _ in range(BISECTIONS):
            m = 0.5 * (lo + hi)
            below = _legendre_cdf(a, m) < target
            lo, hi = np.where(below, m, lo), np.where(below, hi, m)
        m = 0.5 * (lo + hi)
        st = np.where(good & ~(_legendre_density(a, m) >= 0.0), SAMPLE_NEGDENSITY, st)
        mu[q] = np.where(good, m, 0.0)
    keep = (st == SAMPLE_OK) | (st == SAMPLE_NEGDENSITY)
    group[q] = np.where(keep, gq, -1)
    status[q] = st
    return group, mu, status


def sample_section(section, scatt_type, ein, u_g, u_mu, sample=None):
    """(group, mu, status) of the events (ein, u_g, u_mu) drawn from `section`, a reader.ScattSection
    or (x[n], y[n][G][L]).  sample: lib.scatt_sample (the device) unless given, e.g. sample_numpy."""
    x, y = _xy(section)
    return (sample or lib.scatt_sample)(scatt_type, x, y, ein, u_g, u_mu)


def expectations(section, scatt_type, ein):
    """The exact probabilities of the row blended at the energy `ein`: (p[G], shape[G][L]) with
    p[g] = w_g / W, and shape[g] = a_l / a_0 (Legendre: the moments of the group's cosine distribution,
    shape[g][0] = 1) or t_k / T (tabular: the probability of every bin).  Groups that are never drawn
    (w_g = 0) hold NaN in shape.  Raises ValueError where ndpp_scatt_sample would skip the energy or
    finds a bad or an all-zero row."""
    x, y = _xy(section)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e = np.array([float(ein)])
    ok = np.isfinite(e) & (e > 0.0) & (e >= x[0]) & (e <= x[-1])
    if not (grid_ok(x) and ok[0]):
        raise ValueError(f"energy {float(ein)!r} is outside the grid, or the grid is not increasing")
    i, f = _brackets(x, e, ok)
    i, f = int(i[0]), float(f[0])
    i1 = min(i + 1, len(x) - 1)
    row = y[i] + (y[i1] - y[i]) * f
    w = row[:, 0] if scatt_type == reader.SCATT_TYPE_LEGENDRE else row.sum(axis=1)
    if _bad_mass(row if scatt_type == reader.SCATT_TYPE_TABULAR else w).any() or not np.isfinite(row).all():
        raise ValueError(f"the row at {float(ein)!r} holds a negative or non-finite entry")
    if not w.sum() > 0.0:
        raise ValueError(f"the row at {float(ein)!r} is zero")
    with np.errstate(all="ignore"):
        shape = np.where(w[:, None] > 0.0, row / w[:, None], np.nan)
    return w / w.sum(), shape


def _legendre_values(mu, L):
    """P_0 .. P_{L-1} at mu[n]: (L, n)"""
    P = np.ones((L, len(mu)))
    if L > 1:
        P[1] = mu
    for l in range(1, L - 1):
        P[l + 1] = ((2 * l + 1) * mu * P[l] - l * P[l - 1]) / (l + 1)
    return P


def check_energy(section, scatt_type, ein, group, mu, status):
    """The draws (group, mu, status) at the one energy `ein` against expectations: a dict with the
    events per status, and per group the expected and the sampled fraction, the sampled shape (means
    of P_l(mu), or bin fractions) next to the expected one, and their differences in standard errors
    (z_group, z_shape).  The standard error of a fraction p over n draws is sqrt(p (1 - p) / n); that
    of a mean of P_l is bounded by 1 / sqrt(n_g) because |P_l| <= 1, and this bound is the unit."""
    p, shape = expectations(section, scatt_type, ein)
    G, L = shape.shape
    drawn = (status == SAMPLE_OK) | (status == SAMPLE_NEGDENSITY)
    n = int(drawn.sum())
    out = dict(energy=float(ein), events=int(len(status)), drawn=n,
               status={name: int((status == code).sum()) for code, name in STATUS_NAMES.items()}, groups=[])
    for g in range(G):
        sel = drawn & (group == g)
        ng = int(sel.sum())
        frac = ng / n if n else math.nan
        se = math.sqrt(p[g] * (1.0 - p[g]) / n) if n else math.nan
        rec = dict(group=g, expected=float(p[g]), sampled=frac, n=ng,
                   z_group=(frac - p[g]) / se if se > 0.0 else (0.0 if frac == p[g] else math.inf))
        if ng:
            if scatt_type == reader.SCATT_TYPE_LEGENDRE:
                got = _legendre_values(mu[sel], L).mean(axis=1)
                se_l = np.full(L, 1.0 / math.sqrt(ng))
            else:
                k = np.minimum(((mu[sel] + 1.0) * (0.5 * L)).astype(np.int64), L - 1)
                got = np.bincount(k, minlength=L) / ng
                se_l = np.sqrt(shape[g] * (1.0 - shape[g]) / ng)
            with np.errstate(all="ignore"):
                z = np.where(se_l > 0.0, (got - shape[g]) / se_l, np.where(got == shape[g], 0.0, np.inf))
            rec.update(expected_shape=[float(v) for v in shape[g]], sampled_shape=[float(v) for v in got],
                       z_shape=[float(v) for v in z])
        out["groups"].append(rec)
    return out


def sample_table(table: reader.NdppTable, section: str, energies, events: int = 200000, seed: int = 1,
                 sample=None) -> dict:
    """Every energy of `energies` sampled with `events` events from table.<section>; u_g and u_mu come
    from numpy.random.default_rng(seed), drawn in that order per energy.  Returns dict(table, section,
    scatt_type, groups, entries, events, seed, energies=[check_energy's dict], flagged = the events that
    were BADROW or NEGDENSITY).  An energy the section does not cover, or whose row is bad or zero, is
    reported with its status counts and no groups."""
    sec = getattr(table, section)
    if sec is None:
        raise InputError(f"table {table.name} has no {section} section")
    rng = np.random.default_rng(seed)
    rep = dict(table=table.name, section=section, scatt_type=int(table.scatt_type), groups=int(sec.mat.shape[1]),
               entries=int(sec.mat.shape[2]), events=int(events), seed=int(seed), energies=[], flagged=0)
    for e in energies:
        u_g, u_mu = rng.random(events), rng.random(events)
        g, mu, st = sample_section(sec, table.scatt_type, np.full(events, float(e)), u_g, u_mu, sample)
        rep["flagged"] += int(((st == SAMPLE_BADROW) | (st == SAMPLE_NEGDENSITY)).sum())
        try:
            rep["energies"].append(check_energy(sec, table.scatt_type, e, g, mu, st))
        except ValueError as err:
            rep["energies"].append(dict(energy=float(e), events=int(events), drawn=0, reason=str(err), groups=[],
                                        status={name: int((st == code).sum()) for code, name in STATUS_NAMES.items()}))
    return rep


def format_lines(rep: dict) -> list:
    what = "mean P_l" if rep["scatt_type"] == reader.SCATT_TYPE_LEGENDRE else "bin fractions"
    lines = [f"{rep['table']} {rep['section']}: {rep['groups']} groups, {rep['entries']} "
             f"{'moments' if rep['scatt_type'] == reader.SCATT_TYPE_LEGENDRE else 'bins'}, {rep['events']} events per energy"]
    for e in rep["energies"]:
        counts = ", ".join(f"{k} {v}" for k, v in e["status"].items() if v)
        lines.append(f"E = {e['energy']:.6e} MeV: {counts}" + (f" ({e['reason']})" if "reason" in e else ""))
        for r in e["groups"]:
            line = f"  group {r['group']:3d}: fraction {r['sampled']:.6f} against {r['expected']:.6f} ({r['z_group']:+.2f} s.e.)"
            if "z_shape" in r:
                z = r["z_shape"][1:] if rep["scatt_type"] == reader.SCATT_TYPE_LEGENDRE else r["z_shape"]
                if z:
                    line += f"; {what} within {max(abs(v) for v in z):.2f} s.e."
            lines.append(line)
    return lines


def _json_safe(o):
    if isinstance(o, dict):
        return {k: _json_safe(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_json_safe(v) for v in o]
    return _num(o) if isinstance(o, float) else o


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ndpp_amd.sample",
                                 description="Draw outgoing groups and cosines from one section of an NDPP library on "
                                             "the GPU and hold them against the rows (exit 0; 1: an event met a bad row or "
                                             "a negative density; 2: input error; 3: library or device error).")
    ap.add_argument("dir", help="directory holding the library's ndpp_lib.xml (or the xml file itself)")
    ap.add_argument("--table", required=True, metavar="NAME", help="the table to sample, by its name in ndpp_lib.xml")
    ap.add_argument("--section", default="elastic", choices=SECTIONS)
    ap.add_argument("--energy", required=True, nargs="+", metavar="E", help="incoming energies, MeV")
    ap.add_argument("--events", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None, help="write the full report to this file")
    a = ap.parse_args(argv)
    try:
        energies = [float(e) for e in a.energy]
    except ValueError:
        energies = [math.nan]
    if not all(math.isfinite(e) and e > 0.0 for e in energies) or a.events < 1 or a.seed < 0:
        print("ndpp_amd.sample: input error: --energy takes positive finite numbers, --events at least 1, --seed at "
              "least 0", file=sys.stderr)
        return EXIT_INPUT
    try:
        tables = read_library(a.dir)
        if a.table not in tables:
            raise InputError(f"{a.dir}: no table {a.table} (it lists {', '.join(tables) or 'none'})")
        rep = sample_table(tables[a.table][1], a.section, energies, a.events, a.seed)
    except InputError as e:
        print(f"ndpp_amd.sample: input error: {e}", file=sys.stderr)
        return EXIT_INPUT
    except (lib.NdppError, RuntimeError, OSError) as e:
        print(f"ndpp_amd.sample: library error: {e}", file=sys.stderr)
        return EXIT_LIBRARY
    for line in format_lines(rep):
        print(line)
    if a.json:
        try:
            Path(a.json).write_text(json.dumps(_json_safe(rep), indent=1) + "\n")
        except OSError as e:
            print(f"ndpp_amd.sample: cannot write {a.json}: {e}", file=sys.stderr)
            return EXIT_LIBRARY
    return EXIT_FLAGGED if rep["flagged"] else EXIT_OK


if __name__ == "__main__":
    sys.exit(main())
