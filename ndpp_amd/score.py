"""Score collision events into group-to-group tallies, as the expected-value estimator of a transport
code does (include/ndpp_hip.h: ndpp_scatt_score).

At every event the section is read linearly in ln E (the rule of ndpp_lib_compare and of sampling) and
the whole [G][L] row, times the event's factor v, is added to the tally bin the caller names: v is the
weight (normalize 0) or the weight over the row's total mass W (normalize 1).  The order of the sum is
part of the definition: the scored events of a bin, in ascending event index, in chunks of
NDPP_SCORE_CHUNK = 256, each chunk summed sequentially from 0.0, the chunks' partials summed
sequentially from 0.0.  The identity this gives with sampling is the estimator's: the tally over the
count, with normalize 1, is the expectation of the analog tally 1(g) P_l(mu) (or 1(g, k) for cosine
bins) of ndpp_scatt_sample on the same events.  Nothing here knows a cross section or a spectrum.

  score_numpy(normalize, scatt_type, x, y, ein, weight, bin, n_bins)  host restatement of
                          ndpp_scatt_score: the same float64 operations in the same order, dense (no
                          band), the same bits (tally, wsum, count, status)
  contributions(...)      the scored events and what each adds, c[n_scored][G][L], for a check of the sum
  score_section(section, scatt_type, ein, weight, bin, n_bins, normalize=1, score=None)  one
                          reader.ScattSection (or (x, y)) on the device (lib.scatt_score) unless `score`
  analog_tally(...)       the sums of 1(g) P_l(mu) or 1(g, k) of drawn events per tally bin
  score_table(...)        the command line's work: per incoming bin the score against the analog tally

CLI: python -m ndpp_amd.score DIR --table NAME [--section elastic|inelastic|nuinelastic]
--edges E0 E1 [E2 ...] [--events 200000] [--seed 1] [--json FILE]; per incoming bin [E_k, E_k+1),
clipped to the section's grid, --events energies log-uniform with weight 1 are scored with normalize 1
and sampled with ndpp_scatt_sample; it prints the scored matrix's group sums and the largest deviation
of the analog tally from the score in standard errors; exit 0, 1 if an element is beyond 5 standard
errors or an event was BADROW, ZEROROW or NEGDENSITY, 2 on an input error, 3 on a library or device
error.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np

from . import lib, reader
from .compare import InputError, grid_ok, read_library, _brackets, _xy
from .lib import NDPP_SCORE_CHUNK, SCORE_BADROW, SCORE_OK, SCORE_SKIPPED, SCORE_ZEROROW
from .sample import (SAMPLE_BADROW, SAMPLE_NEGDENSITY, SAMPLE_OK, SAMPLE_ZEROROW, _bad_mass, _json_safe,
                     _legendre_values, _masses)

EXIT_OK, EXIT_FLAGGED, EXIT_INPUT, EXIT_LIBRARY = 0, 1, 2, 3
SECTIONS = ("elastic", "inelastic", "nuinelastic")
STATUS_NAMES = {SCORE_OK: "ok", SCORE_SKIPPED: "skipped", SCORE_BADROW: "badrow", SCORE_ZEROROW: "zerorow"}
Z_LIMIT = 5.0
_BLOCK = 1 << 16       # events the factor handles at a time
_ELEMENTS = 1 << 22    # elements of partial sums score_numpy holds at a time


def _arguments(normalize, scatt_type, x, y, ein, weight, bin, n_bins):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ein, weight = np.asarray(ein, dtype=np.float64).ravel(), np.asarray(weight, dtype=np.float64).ravel()
    bin = np.asarray(bin, dtype=np.int64).ravel()
    if normalize not in (0, 1):
        raise ValueError(f"normalize {normalize!r} is neither 0 nor 1")
    if normalize and scatt_type not in (reader.SCATT_TYPE_LEGENDRE, reader.SCATT_TYPE_TABULAR):
        raise ValueError(f"scatt_type {scatt_type!r} is neither 0 (Legendre) nor 1 (tabular)")
    if y.ndim != 3 or x.shape != (y.shape[0],) or not (len(ein) == len(weight) == len(bin)):
        raise ValueError(f"shapes do not match: x {x.shape}, y {y.shape}, events {len(ein)}, {len(weight)}, {len(bin)}")
    n, G, L = y.shape
    Lmax = lib.NDPP_MAX_ORDER if normalize and scatt_type == reader.SCATT_TYPE_LEGENDRE else lib.NDPP_MAX_TAB_BINS
    if not 1 <= L <= Lmax or G < 1 or n_bins < 1:
        raise ValueError(f"G = {G}, L = {L}, n_bins = {n_bins}: need G >= 1, 1 <= L <= {Lmax} and n_bins >= 1")
    if not grid_ok(x):
        raise ValueError("the grid must be strictly increasing, positive and finite, with two points or more")
    return x, y, ein, weight, bin


def _factors(normalize, scatt_type, x, y, ein, weight, bin, n_bins):
    """steps 1 and 2 of the header: (i, i1, f, v, status) per event"""
    n = len(x)
    ok = (np.isfinite(ein) & (ein > 0.0) & (ein >= x[0]) & (ein <= x[-1]) & np.isfinite(weight) & (bin >= 0)
          & (bin < n_bins))
    i, f = _brackets(x, ein, ok)
    i1 = np.minimum(i + 1, n - 1)
    status = np.where(ok, SCORE_OK, SCORE_SKIPPED).astype(np.int32)
    v = np.where(ok, weight, 0.0)
    if normalize:
        s = _masses(scatt_type, y)
        live = np.flatnonzero(ok)
        for at in range(0, len(live), _BLOCK):
            q = live[at:at + _BLOCK]
            s0, s1 = s[i[q]], s[i1[q]]
            w = s0 + (s1 - s0) * f[q][:, None]
            bad, W = np.zeros(len(q), dtype=bool), np.zeros(len(q))
            for g in range(w.shape[1]):
                bad |= _bad_mass(w[:, g])
                W = W + w[:, g]
            bad |= ~(W < np.inf)
            st = np.where(bad, SCORE_BADROW, np.where(W == 0.0, SCORE_ZEROROW, SCORE_OK))
            status[q] = st
            v[q] = np.where(st == SCORE_OK, weight[q] / np.where(st == SCORE_OK, W, 1.0), 0.0)
    return i, i1, f, v, status


def _chunks(status, bin, n_bins):
    """the scored events in the sorted order (by bin, each bin in ascending event index), count[n_bins],
    first[n_bins + 1] (the chunks of bin b are first[b] .. first[b + 1]), and per chunk its first place
    in the sorted order and its length"""
    scored = np.flatnonzero(status == SCORE_OK)
    order = scored[np.argsort(bin[scored], kind="stable")]
    count = np.bincount(bin[scored], minlength=n_bins).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(count)))
    nch = (count + NDPP_SCORE_CHUNK - 1) // NDPP_SCORE_CHUNK
    first = np.concatenate(([0], np.cumsum(nch)))
    cbin = np.repeat(np.arange(n_bins), nch)
    cstart = off[cbin] + (np.arange(first[-1]) - first[cbin]) * NDPP_SCORE_CHUNK
    clen = np.minimum(NDPP_SCORE_CHUNK, off[cbin + 1] - cstart)
    return order, count, first, cstart, clen


def _contribution(yf, i, i1, f, v):
    """step 3: v * (y[i] + (y[i1] - y[i]) * f) for events (rows of yf[n][G L])"""
    r0, r1 = yf[i], yf[i1]
    return v[:, None] * (r0 + (r1 - r0) * f[:, None])


def score_numpy(normalize, scatt_type, x, y, ein, weight, bin, n_bins):
    """ndpp_scatt_score on the host (include/ndpp_hip.h): (tally[n_bins][G][L], wsum[n_bins],
    count[n_bins] int64, status[n_ev] int32).  Everything after the logarithms is IEEE + - * / in the
    kernels' order: chunks of 256 summed sequentially, then the partials; vectorised over the elements
    and over the chunks, which changes no order.  Dense: every element of every event is added."""
    x, y, ein, weight, bin = _arguments(normalize, scatt_type, x, y, ein, weight, bin, n_bins)
    n, G, L = y.shape
    GL = G * L
    yf = y.reshape(n, GL)
    with np.errstate(all="ignore"):
        i, i1, f, v, status = _factors(normalize, scatt_type, x, y, ein, weight, bin, n_bins)
        order, count, first, cstart, clen = _chunks(status, bin, n_bins)
        n_chunks = len(cstart)
        partial = np.zeros((n_chunks, GL + 1))
        step = max(1, _ELEMENTS // (GL + 1))
        for c0 in range(0, n_chunks, step):
            cs, cl = cstart[c0:c0 + step], clen[c0:c0 + step]
            part = partial[c0:c0 + step]
            for k in range(NDPP_SCORE_CHUNK):
                m = np.flatnonzero(cl > k)
                if not len(m):
                    break
                ev = order[cs[m] + k]
                part[m, :GL] = part[m, :GL] + _contribution(yf, i[ev], i1[ev], f[ev], v[ev])
                part[m, GL] = part[m, GL] + v[ev]
        out = np.zeros((n_bins, GL + 1))
        nch = np.diff(first)
        for j in range(int(nch.max(initial=0))):
            b = np.flatnonzero(nch > j)
            out[b] = out[b] + partial[first[b] + j]
    return out[:, :GL].reshape(n_bins, G, L).copy(), out[:, GL].copy(), count, status


def contributions(normalize, scatt_type, x, y, ein, weight, bin, n_bins):
    """(events, c, v, status): the indices of the scored events in ascending order, what each adds to
    its bin, c[len(events)][G][L], its factor v[len(events)], and status[n_ev].  The terms of
    score_numpy's sums, for a check of the summation against a wider format."""
    x, y, ein, weight, bin = _arguments(normalize, scatt_type, x, y, ein, weight, bin, n_bins)
    n, G, L = y.shape
    with np.errstate(all="ignore"):
        i, i1, f, v, status = _factors(normalize, scatt_type, x, y, ein, weight, bin, n_bins)
        ev = np.flatnonzero(status == SCORE_OK)
        c = _contribution(y.reshape(n, G * L), i[ev], i1[ev], f[ev], v[ev])
    return ev, c.reshape(len(ev), G, L), v[ev], status


def score_section(section, scatt_type, ein, weight, bin, n_bins, normalize=1, score=None):
    """(tally, wsum, count, status) of the events (ein, weight, bin) scored into n_bins tallies from
    `section`, a reader.ScattSection or (x[n], y[n][G][L]).  score: lib.scatt_score (the device) unless
    given, e.g. score_numpy."""
    x, y = _xy(section)
    return (score or lib.scatt_score)(normalize, scatt_type, x, y, ein, weight, bin, n_bins)


def analog_tally(scatt_type, G, L, group, mu, status, bin, n_bins):
    """The analog estimator of drawn events (ndpp_scatt_sample's group, mu, status): per tally bin the
    sum of 1(g) P_l(mu) (Legendre) or 1(g, k) (cosine bins, k the bin mu falls in), [n_bins][G][L],
    and the number of events drawn (OK or NEGDENSITY), [n_bins]."""
    group, mu, status, bin = (np.asarray(a) for a in (group, mu, status, bin))
    drawn = ((status == SAMPLE_OK) | (status == SAMPLE_NEGDENSITY)) & (bin >= 0) & (bin < n_bins)
    g, m, b = group[drawn].astype(np.int64), mu[drawn], bin[drawn].astype(np.int64)
    out = np.zeros((n_bins, G, L))
    if scatt_type == reader.SCATT_TYPE_LEGENDRE:
        P = _legendre_values(m, L)
        for l in range(L):
            out[:, :, l] = np.bincount(b * G + g, weights=P[l], minlength=n_bins * G).reshape(n_bins, G)
    else:
        k = np.minimum(((m + 1.0) * (0.5 * L)).astype(np.int64), L - 1)
        out = np.bincount((b * G + g) * L + k, minlength=n_bins * G * L).reshape(n_bins, G, L).astype(np.float64)
    return out, np.bincount(b, minlength=n_bins)


def standard_errors(scatt_type, mean, n):
    """The unit of the comparison for the scored mean matrix mean[G][L] over n events.  Legendre:
    sqrt(p_g / n) for every moment of group g, p_g = mean[g][0] -- the analog term 1(g) P_l(mu) is bounded
    by the group's indicator, so its variance given the energy is at most p_g.  Bins: the binomial
    sqrt(p (1 - p) / n) of the element's own share."""
    with np.errstate(all="ignore"):
        if scatt_type == reader.SCATT_TYPE_LEGENDRE:
            return np.sqrt(np.maximum(mean[:, :1], 0.0) / n) * np.ones_like(mean)
        return np.sqrt(np.maximum(mean * (1.0 - mean), 0.0) / n)


def score_table(table: reader.NdppTable, section: str, edges, events: int = 200000, seed: int = 1, score=None,
                sample=None) -> dict:
    """Every incoming bin [edges[k], edges[k+1]), clipped to the grid of table.<section>, scored with
    `events` log-uniform energies of weight 1 (normalize 1, all bins in one call) and sampled on the
    same events; energies, u_g and u_mu come from numpy.random.default_rng(seed), drawn in that order per
    bin.  Returns dict(table, section, scatt_type, groups, entries, events, seed, edges, bins=[...],
    flagged, beyond); a bin the grid does not reach is reported without events."""
    sec = getattr(table, section)
    if sec is None:
        raise InputError(f"table {table.name} has no {section} section")
    x, y = _xy(sec)
    st_type, (_, G, L) = int(table.scatt_type), y.shape
    rng = np.random.default_rng(seed)
    rep = dict(table=table.name, section=section, scatt_type=st_type, groups=int(G), entries=int(L),
               events=int(events), seed=int(seed), edges=[float(e) for e in edges], bins=[], flagged=0, beyond=0)
    ein, ug, um, where = [], [], [], []
    spans = []
    for k in range(len(edges) - 1):
        lo, hi = max(float(edges[k]), float(x[0])), min(float(edges[k + 1]), float(x[-1]))
        spans.append((lo, hi))
        if not lo < hi:
            continue
        ein.append(np.clip(np.exp(rng.uniform(math.log(lo), math.log(hi), events)), lo, hi))
        ug.append(rng.random(events))
        um.append(rng.random(events))
        where.append(np.full(events, k, dtype=np.int32))
    n_bins = len(edges) - 1
    if ein:
        ein, ug, um, where = (np.concatenate(a) for a in (ein, ug, um, where))
        tally, wsum, count, status = score_section(sec, st_type, ein, np.ones(len(ein)), where, n_bins, 1, score)
        g, mu, sst = (sample or lib.scatt_sample)(st_type, x, y, ein, ug, um)
        analog, drawn = analog_tally(st_type, G, L, g, mu, sst, where, n_bins)
        rep["flagged"] = int(((status == SCORE_BADROW) | (status == SCORE_ZEROROW)).sum()
                             + ((sst == SAMPLE_NEGDENSITY) | (sst == SAMPLE_BADROW) | (sst == SAMPLE_ZEROROW)).sum())
    for k, (lo, hi) in enumerate(spans):
        rec = dict(bin=k, lo=lo, hi=hi, events=0, scored=0, drawn=0)
        if lo < hi:
            sel = where == k
            rec.update(events=int(sel.sum()), scored=int(count[k]), drawn=int(drawn[k]), wsum=float(wsum[k]),
                       status={name: int((status[sel] == code).sum()) for code, name in STATUS_NAMES.items()})
        else:
            rec["reason"] = "the section's grid does not reach this bin"
        if rec["scored"] and rec["drawn"]:
            mean = tally[k] / float(count[k])
            got = analog[k] / float(drawn[k])
            se = standard_errors(st_type, mean, float(count[k]))
            with np.errstate(all="ignore"):
                z = np.where(se > 0.0, np.abs(got - mean) / se, np.where(got == mean, 0.0, np.inf))
            z = np.where(np.isnan(z), np.inf, z)
            at = np.unravel_index(int(np.argmax(z)), z.shape)
            sums = mean[:, 0] if st_type == reader.SCATT_TYPE_LEGENDRE else mean.sum(axis=1)
            rec.update(group_sums=[float(s) for s in sums], total=float(sums.sum()), worst_z=float(z[at]),
                       worst_group=int(at[0]), worst_entry=int(at[1]), beyond=int((z > Z_LIMIT).sum()),
                       score=[[float(s) for s in row] for row in mean], analog=[[float(s) for s in row] for row in got])
            rep["beyond"] += rec["beyond"]
        rep["bins"].append(rec)
    return rep


def format_lines(rep: dict) -> list:
    what = "moments" if rep["scatt_type"] == reader.SCATT_TYPE_LEGENDRE else "bins"
    lines = [f"{rep['table']} {rep['section']}: {rep['groups']} groups, {rep['entries']} {what}, "
             f"{rep['events']} events per incoming bin"]
    for b in rep["bins"]:
        head = f"bin {b['bin']} [{b['lo']:.6e}, {b['hi']:.6e}) MeV: "
        if "reason" in b:
            lines.append(head + b["reason"])
            continue
        lines.append(head + ", ".join(f"{k} {v}" for k, v in b["status"].items() if v))
        if "group_sums" in b:
            lines.append("  group sums of the scored matrix: " + " ".join(f"{s:.6f}" for s in b["group_sums"])
                         + f" (total {b['total']:.15f})")
            lines.append(f"  analog tally within {b['worst_z']:.2f} s.e. of the score (group {b['worst_group']}, "
                         f"entry {b['worst_entry']}); {b['beyond']} elements beyond {Z_LIMIT:g}")
    return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ndpp_amd.score",
                                 description="Score collision events into group-to-group tallies from one section of an "
                                             "NDPP library on the GPU and hold the analog tally of the same events "
                                             "against them (exit 0; 1: an element beyond 5 standard errors, or an event "
                                             "met a bad or zero row or a negative density; 2: input error; 3: library "
                                             "or device error).")
    ap.add_argument("dir", help="directory holding the library's ndpp_lib.xml (or the xml file itself)")
    ap.add_argument("--table", required=True, metavar="NAME", help="the table to score, by its name in ndpp_lib.xml")
    ap.add_argument("--section", default="elastic", choices=SECTIONS)
    ap.add_argument("--edges", required=True, nargs="+", metavar="E", help="edges of the incoming bins, MeV, increasing")
    ap.add_argument("--events", type=int, default=200000, help="events per incoming bin")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None, help="write the full report to this file")
    a = ap.parse_args(argv)
    try:
        edges = [float(e) for e in a.edges]
    except ValueError:
        edges = [math.nan]
    if (len(edges) < 2 or not all(math.isfinite(e) and e > 0.0 for e in edges)
            or not all(p < q for p, q in zip(edges, edges[1:])) or a.events < 1 or a.seed < 0):
        print("ndpp_amd.score: input error: --edges takes two or more increasing positive finite numbers, --events at "
              "least 1, --seed at least 0", file=sys.stderr)
        return EXIT_INPUT
    try:
        tables = read_library(a.dir)
        if a.table not in tables:
            raise InputError(f"{a.dir}: no table {a.table} (it lists {', '.join(tables) or 'none'})")
        rep = score_table(tables[a.table][1], a.section, edges, a.events, a.seed)
    except InputError as e:
        print(f"ndpp_amd.score: input error: {e}", file=sys.stderr)
        return EXIT_INPUT
    except (lib.NdppError, RuntimeError, OSError) as e:
        print(f"ndpp_amd.score: library error: {e}", file=sys.stderr)
        return EXIT_LIBRARY
    for line in format_lines(rep):
        print(line)
    if a.json:
        try:
            Path(a.json).write_text(json.dumps(_json_safe(rep), indent=1) + "\n")
        except OSError as e:
            print(f"ndpp_amd.score: cannot write {a.json}: {e}", file=sys.stderr)
            return EXIT_LIBRARY
    return EXIT_FLAGGED if rep["flagged"] or rep["beyond"] else EXIT_OK


if __name__ == "__main__":
    sys.exit(main())
