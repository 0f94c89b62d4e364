"""Derive a library from a finished one: coarser outgoing groups, cosine bins from Legendre moments,
moments and their enclosure from bins (include/ndpp_hip.h: ndpp_derive_*).
Nothing is integrated again: every operation is a product of a stored row with a fixed table, or a sum
of neighbouring groups, on the GPU.

| request   | on a Legendre table                                         | on a tabular table               |
|-----------|-------------------------------------------------------------|----------------------------------|
| groups    | every edge bitwise one of the table's, same first and last  | same                             |
| bins N    | ndpp_derive_bins                                            | N divides the stored count: the bins are merged |
| moments L | the first L moments, L <= stored                            | ndpp_derive_moments              |

`groups` may be combined with one of the others and is applied first.  The chi rows (total, prompt,
delayed) follow `groups` as rows of one entry.

groups_numpy, bins_numpy and moments_numpy restate the entry points from the tables of
ndpp_derive_tables in float64, in the written order, vectorised over rows: they give the bits of the
device.  `table(..., kernels=NUMPY_KERNELS)` runs the whole tool on them (the CPU tests); without
`kernels` the device runs, and there is no other fallback.

Files are written by the writers of the driver (lib.nuclide_file, lib.lib_xml, run.write_library: all
or nothing), with the options of each table's own header.  A thermal table is written with is_sab = 0:
its header says nuscatter false and no chi, so its bytes are those of a neutron table, and the writer's
refusal of tabular thermal tables -- which guards the integrators, not a derived table -- does not apply.

CLI: python -m ndpp_amd.derive DIR_IN DIR_OUT [--groups E0 E1 ...] [--bins N] [--moments L] [--json FILE]
exit 0; 1: a derived row has a negative bin or is not finite (the library is still written, the rows
are counted per table and section; Legendre rows want `python -m ndpp_amd.run --repair-positivity`
first); 2: input error (edges not in the library, N not dividing, L too large, DIR_OUT equal to DIR_IN,
no request); 3: library or device error.  With --moments on a tabular library the report carries, per
section and per l, the widest enclosure (hi - lo) / S.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from dataclasses import replace
from pathlib import Path

import numpy as np

from . import compare, lib, reader
from .lib import DERIVE_NEGBIN, DERIVE_NONFINITE, DERIVE_ZERO

EXIT_OK, EXIT_FLAGGED, EXIT_INPUT, EXIT_LIBRARY = 0, 1, 2, 3
SECTIONS = ("elastic", "inelastic", "nuinelastic")
CHI_SECTIONS = ("total", "prompt", "delayed")


class InputError(ValueError):
    """a request the library at hand cannot honour, or an unreadable library: exit status 2"""


# ---- the restatements ---------------------------------------------------------------------------

def _rows(mat):
    mat = np.ascontiguousarray(mat, dtype=np.float64)
    if mat.ndim != 3:
        raise ValueError(f"mat must be (n, G, L), got {mat.shape}")
    return mat


def groups_numpy(mat, first) -> np.ndarray:
    """ndpp_derive_groups: the sum over first[c] <= g < first[c+1], ascending g from 0.0"""
    mat, first = _rows(mat), np.asarray(first, dtype=np.int64).ravel()
    n, G, L = mat.shape
    out = np.zeros((n, len(first) - 1, L))
    for c in range(len(first) - 1):
        s = np.zeros((n, L))
        for g in range(first[c], first[c + 1]):
            s = s + mat[:, g]
        out[:, c] = s
    return out


def bins_numpy(mat, N: int):
    """ndpp_derive_bins: (bins[n][G][N], status[n][G] int32)"""
    mat = _rows(mat)
    n, G, L = mat.shape
    W = lib.derive_tables(L, N)[0]
    t = np.zeros((n, G, N))
    with np.errstate(all="ignore"):
        for l in range(L):
            t = t + mat[:, :, l, None] * W[l]
        zero = mat[:, :, 0] == 0.0
        t[zero] = 0.0
        status = np.where(zero, DERIVE_ZERO, 0)
        status |= np.where(~np.isfinite(mat).all(axis=2) | ~np.isfinite(t).all(axis=2), DERIVE_NONFINITE, 0)
        status |= np.where((t < 0.0).any(axis=2), DERIVE_NEGBIN, 0)
    return t, status.astype(np.int32)


def moments_numpy(mat, L: int, bounds: bool = True):
    """ndpp_derive_moments: (moments, lo, hi, status)"""
    mat = _rows(mat)
    n, G, N = mat.shape
    _, V, pmin, pmax = lib.derive_tables(L, N)
    out = np.zeros((n, G, L))
    lo, hi = (np.zeros((n, G, L)), np.zeros((n, G, L))) if bounds else (None, None)
    with np.errstate(all="ignore"):
        for k in range(N):
            x = mat[:, :, k, None]
            out = out + x * V[:, k]
            if bounds:
                lo = lo + x * pmin[:, k]
                hi = hi + x * pmax[:, k]
        status = np.where(~np.isfinite(mat).all(axis=2) | ~np.isfinite(out).all(axis=2), DERIVE_NONFINITE, 0)
        status |= np.where((mat < 0.0).any(axis=2), DERIVE_NEGBIN, 0)
    return out, lo, hi, status.astype(np.int32)


NUMPY_KERNELS = dict(groups=groups_numpy, bins=bins_numpy, moments=moments_numpy)


class DeviceKernels(dict):
    """the entry points of the device, with the time their kernels took (ms) summed in .device_ms"""

    def __init__(self):
        super().__init__(groups=self._timed(lib.derive_groups), bins=self._timed(lib.derive_bins),
                         moments=self._timed(lib.derive_moments))
        self.device_ms = 0.0

    def _timed(self, call):
        def run(*args):
            out = call(*args)
            if args[0].shape[0]:
                self.device_ms += float(lib.load().ndpp_last_gpu_ms())
            return out
        return run


# ---- one table ----------------------------------------------------------------------------------

def group_segments(e_bins, groups) -> np.ndarray:
    """first[Gc + 1]: the positions of the edges `groups` among e_bins.  Every edge must be bitwise one of
    e_bins, ascending, with the same first and last edge.  Raises InputError."""
    e_bins = np.asarray(e_bins, dtype=np.float64)
    new = np.asarray(groups, dtype=np.float64).ravel()
    if len(new) < 2:
        raise InputError("a group structure needs at least two edges")
    if not np.all(np.diff(new) > 0.0):
        raise InputError("the group edges must be strictly increasing")
    first = []
    for e in new:
        at = np.nonzero(e_bins == e)[0]
        if len(at) != 1:
            raise InputError(f"the edge {float(e)!r} is not one of the library's {len(e_bins)} edges (the edges must "
                             "match in every bit)")
        first.append(int(at[0]))
    if first[0] != 0 or first[-1] != len(e_bins) - 1:
        raise InputError(f"the first and the last edge must be the library's, {float(e_bins[0])!r} and "
                         f"{float(e_bins[-1])!r}")
    return np.array(first, dtype=np.int32)


def _band(mat, tabular):
    """the writer's gmin, gmax (1-based, 0 for a row without any P0 > 0)"""
    p0 = mat[:, :, 0]
    if tabular:                          # the bins in ascending k from 0.0, as the writer sums them
        p0 = np.zeros(mat.shape[:2])
        for k in range(mat.shape[2]):
            p0 = p0 + mat[:, :, k]
    pos = p0 > 0.0
    G = mat.shape[1]
    anyp = pos.any(axis=1)
    gmin = np.where(anyp, pos.argmax(axis=1) + 1, 0).astype(np.int32)
    gmax = np.where(anyp, G - pos[:, ::-1].argmax(axis=1), 0).astype(np.int32)
    return gmin, gmax


def _plan(t: reader.NdppTable, groups, bins, moments):
    """what `table` does to t: (first or None, op, value) with op one of None, 'bins', 'merge', 'cut',
    'moments'.  Raises InputError."""
    if groups is None and bins is None and moments is None:
        raise InputError("nothing is asked for: give groups, bins or moments")
    if bins is not None and moments is not None:
        raise InputError("bins and moments do not go together: groups may be combined with one of them")
    first = None if groups is None else group_segments(t.e_bins, groups)
    tabular = t.scatt_type == reader.SCATT_TYPE_TABULAR
    stored = t.moments
    op, value = None, None
    if bins is not None:
        N = int(bins)
        if not 1 <= N <= lib.NDPP_MAX_TAB_BINS:
            raise InputError(f"bins = {N}: between 1 and {lib.NDPP_MAX_TAB_BINS} bins are possible")
        if tabular:
            if stored % N:
                raise InputError(f"{t.name}: {N} bins do not divide the {stored} stored bins")
            op, value = "merge", N
        else:
            op, value = "bins", N
    if moments is not None:
        L = int(moments)
        if not 1 <= L <= lib.NDPP_MAX_ORDER:
            raise InputError(f"moments = {L}: between 1 and {lib.NDPP_MAX_ORDER} moments are possible")
        if tabular:
            op, value = "moments", L
        else:
            if L > stored:
                raise InputError(f"{t.name}: {L} moments are asked for and {stored} are stored")
            op, value = "cut", L
    return first, op, value


def _section(mat, first, op, value, K, max_bytes, rep):
    """one scatter section through the plan, in slices of whole energies of at most max_bytes of output"""
    n, G, Lin = mat.shape
    Gout = G if first is None else len(first) - 1
    Lout = Lin if op is None else value
    out = np.zeros((n, Gout, Lout))
    per = max(1, int(max_bytes) // max(1, Gout * Lout * 8))
    flagged = dict(rows=int(n * Gout), negbin=0, nonfinite=0, zero=0)
    width = np.zeros(Lout) if op == "moments" else None
    for a in range(0, n, per):
        m = np.ascontiguousarray(mat[a:a + per])
        if first is not None:
            m = K["groups"](m, first)
        status = None
        if op == "bins":
            m, status = K["bins"](m, value)
        elif op == "merge":
            k, g, N = m.shape
            seg = np.arange(0, N + 1, N // value, dtype=np.int32)
            m = K["groups"](m.reshape(k * g, N, 1), seg).reshape(k, g, value)
        elif op == "cut":
            m = np.ascontiguousarray(m[:, :, :value])
        elif op == "moments":
            m, lo, hi, status = K["moments"](m, value)
            ok = ((status & (DERIVE_NEGBIN | DERIVE_NONFINITE)) == 0) & (m[:, :, 0] > 0.0)
            if ok.any():
                with np.errstate(all="ignore"):
                    w = ((hi - lo) / m[:, :, :1])[ok]
                width = np.maximum(width, w.max(axis=0))
        if status is not None:
            flagged["negbin"] += int(((status & DERIVE_NEGBIN) != 0).sum())
            flagged["nonfinite"] += int(((status & DERIVE_NONFINITE) != 0).sum())
            flagged["zero"] += int(((status & DERIVE_ZERO) != 0).sum())
        out[a:a + per] = m
    if width is not None:
        flagged["width"] = [compare._num(float(v)) for v in width]
    rep.append(flagged)
    return out


def table(t: reader.NdppTable, groups=None, bins=None, moments=None, kernels=None, max_bytes=1 << 30):
    """The table derived from t and a report: dict(name, sections = {section: dict(rows, negbin,
    nonfinite, zero[, width per l])}, flagged = rows with a negative bin or a value that is not finite).
    kernels: dict(groups=, bins=, moments=) of callables with the signatures of lib.derive_groups,
    lib.derive_bins and lib.derive_moments (NUMPY_KERNELS: the restatements); None: the device.
    Raises InputError for a request t cannot honour, lib.NdppError from the device."""
    first, op, value = _plan(t, groups, bins, moments)
    K = DeviceKernels() if kernels is None else kernels
    e_bins = t.e_bins if first is None else np.ascontiguousarray(t.e_bins[first])
    scatt_type, scatt_order = t.scatt_type, t.scatt_order
    if op == "bins":
        scatt_type, scatt_order = reader.SCATT_TYPE_TABULAR, value
    elif op == "merge":
        scatt_order = value
    elif op == "cut":
        scatt_order = value - 1
    elif op == "moments":
        scatt_type, scatt_order = reader.SCATT_TYPE_LEGENDRE, value - 1
    out = replace(t, e_bins=e_bins, scatt_type=scatt_type, scatt_order=scatt_order, elastic=None, inelastic=None,
                  nuinelastic=None, chi={})
    report = dict(name=t.name, sections={})
    tab_out = scatt_type == reader.SCATT_TYPE_TABULAR
    for name in SECTIONS:
        s = getattr(t, name)
        if s is None:
            continue
        rep = []
        mat = _section(s.mat, first, op, value, K, max_bytes, rep)
        gi = s.group_index if first is None else np.ascontiguousarray(s.group_index[first])
        setattr(out, name, reader.ScattSection(s.ein, gi, *_band(mat, tab_out), mat))
        report["sections"][name] = rep[0]
    if t.chi:
        out.chi = dict(t.chi)
        if first is not None:
            for name in CHI_SECTIONS:
                c = np.ascontiguousarray(t.chi[name], dtype=np.float64)
                rep = []
                r = _section(c.reshape(-1, c.shape[-1], 1), first, None, None, K, max_bytes, rep)
                out.chi[name] = r.reshape(c.shape[:-1] + (len(first) - 1,))
    report["flagged"] = sum(s["negbin"] + s["nonfinite"] for s in report["sections"].values())
    return out, report


# ---- a library ----------------------------------------------------------------------------------

def stored_name(data: bytes, lib_format: int) -> str:
    """the table name as its file holds it, padding included (the reader strips it): the ten characters
    the writers are handed"""
    if lib_format == lib.FMT_BINARY:
        return data[:reader.NAME_LEN].decode()
    return data.split(b"\n", 1)[0][:20].decode()[-reader.NAME_LEN:]


def table_file(t: reader.NdppTable, lib_format: int, name: str | None = None) -> bytes:
    """t's library file, by the driver's writer with the options of t's own header (is_sab = 0: see the
    module's text).  name: the name with its padding (stored_name), default t.name padded to ten."""
    name = f"{t.name:<{reader.NAME_LEN}s}" if name is None else name
    opts = lib.OutputOptions(lib_format=lib_format, scatt_type=t.scatt_type, scatt_order=t.scatt_order,
                             nuscatter=int(t.nuscatter), integrate_chi=int(t.chi_present), mu_bins=t.mu_bins,
                             print_tol=0.0, thin_tol=t.thin_tol)
    result = dict(ein_el=t.elastic.ein, el_mat=t.elastic.mat, ein_inel=None, inel_mat=None, nuinel_mat=None)
    if t.inelastic is not None:
        result.update(ein_inel=t.inelastic.ein, inel_mat=t.inelastic.mat)
        if t.nuinelastic is not None:
            result["nuinel_mat"] = t.nuinelastic.mat
    chi = None
    if t.chi_present and t.chi:
        chi = (t.chi["e_grid"], t.chi["total"], t.chi["prompt"], t.chi["delayed"])
    return lib.nuclide_file(opts, name, t.kT, result, t.e_bins, chi=chi, is_sab=0)


def library(dir_in, dir_out, groups=None, bins=None, moments=None, kernels=None, max_bytes=1 << 30) -> dict:
    """Derive every table of the library at dir_in and write the result to dir_out (all files or none).
    Returns dict(dir_in, dir_out, request, tables = [table reports], flagged, files, wall_s[, device_ms]).
    Raises InputError (nothing is written), lib.NdppError / RuntimeError / OSError."""
    t0 = time.perf_counter()
    din, dout = Path(dir_in), Path(dir_out)
    xml_in = din / "ndpp_lib.xml" if din.is_dir() or not din.exists() else din
    if dout.resolve() == xml_in.parent.resolve():
        raise InputError("DIR_OUT is DIR_IN: a derived library does not replace the one it came from")
    if groups is None and bins is None and moments is None:
        raise InputError("nothing is asked for: give --groups, --bins or --moments")
    try:
        tables = compare.read_library(din)
        meta = reader.read_lib_xml(xml_in.read_bytes())
    except compare.InputError as e:
        raise InputError(str(e)) from None
    if not tables:
        raise InputError(f"{xml_in} lists no table")
    for _, t in tables.values():                 # every refusal before any work
        _plan(t, groups, bins, moments)
    fmt = lib.FMT_BINARY if str(meta.get("filetype", "binary")).lower() == "binary" else lib.FMT_ASCII
    K = DeviceKernels() if kernels is None else kernels
    files, reports, rows, derived = [], [], [], None
    for attrs, t in tables.values():
        derived, rep = table(t, groups, bins, moments, K, max_bytes)
        reports.append(rep)
        name = Path(attrs["path"]).name
        p = Path(attrs["path"])                  # (where compare.read_library found the file)
        src = next(c for c in (p if p.is_absolute() else xml_in.parent / p, xml_in.parent / p.name) if c.is_file())
        files.append((name, table_file(derived, fmt, stored_name(src.read_bytes()[:128], fmt))))
        rows.append(dict(alias=attrs.get("alias", t.name), awr=attrs.get("awr", 0.0), name=attrs["name"], path=name,
                         kT=attrs.get("temperature", t.kT), zaid=attrs.get("zaid", 0),
                         metastable=attrs.get("metastable", "0") not in ("0", ""),
                         freegas_cutoff=attrs.get("freegas_cutoff", 0.0)))
    xml = lib.lib_xml(str(dout.resolve()) + "/", fmt, rows, derived.e_bins, derived.scatt_type, derived.scatt_order,
                      int(meta.get("mu_bins", derived.mu_bins)), bool(meta.get("nuscatter", False)),
                      bool(meta.get("chi_present", False)), float(meta.get("print_tol", 0.0)),
                      float(meta.get("thin_tol", 0.0)))
    from . import run
    dout.mkdir(parents=True, exist_ok=True)
    written = run.write_library(dout, files, xml)
    out = dict(dir_in=str(dir_in), dir_out=str(dir_out),
               request=dict(groups=None if groups is None else [float(e) for e in groups], bins=bins, moments=moments),
               tables=reports, flagged=sum(r["flagged"] for r in reports), files=[str(p) for p in written],
               wall_s=time.perf_counter() - t0)
    if isinstance(K, DeviceKernels):
        out["device_ms"] = K.device_ms
    return out


def format_lines(rep: dict) -> list:
    lines = []
    for t in rep["tables"]:
        for sec, s in t["sections"].items():
            line = (f"{t['name']:>12s} {sec:12s} rows {s['rows']:8d}  negative bin {s['negbin']:7d}  not finite "
                    f"{s['nonfinite']:7d}")
            if "width" in s:
                line += "  widest (hi - lo) / S per l: " + " ".join(f"{float(w):.2e}" for w in s["width"])
            lines.append(line)
    return lines


def main(argv=None, kernels=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ndpp_amd.derive",
                                 description="Derive a library from a finished one: coarser outgoing groups, cosine bins "
                                             "from Legendre moments, moments from bins (exit 0; 1: a derived row has a "
                                             "negative bin or is not finite; 2: input error; 3: library or device error).")
    ap.add_argument("dir_in", help="directory holding the library's ndpp_lib.xml")
    ap.add_argument("dir_out", help="directory the derived library is written to (not dir_in)")
    ap.add_argument("--groups", nargs="+", metavar="E", default=None,
                    help="the edges of the coarser group structure, each one of the library's in every bit")
    ap.add_argument("--bins", metavar="N", default=None, help="N equal cosine bins per group")
    ap.add_argument("--moments", metavar="L", default=None, help="L Legendre moments per group")
    ap.add_argument("--json", default=None, help="write the full report to this file")
    try:
        a = ap.parse_args(argv)
    except SystemExit as e:
        return EXIT_OK if e.code == 0 else EXIT_INPUT
    try:
        try:
            groups = None if a.groups is None else [float(v) for v in a.groups]
            nbins = None if a.bins is None else int(a.bins)
            nmom = None if a.moments is None else int(a.moments)
        except ValueError as e:
            raise InputError(f"not a number: {e}") from None
        rep = library(a.dir_in, a.dir_out, groups, nbins, nmom, kernels)
    except InputError as e:
        print(f"ndpp_amd.derive: input error: {e}", file=sys.stderr)
        return EXIT_INPUT
    except (lib.NdppError, RuntimeError, OSError) as e:
        print(f"ndpp_amd.derive: library error: {e}", file=sys.stderr)
        return EXIT_LIBRARY
    for line in format_lines(rep):
        print(line)
    print(f"{len(rep['tables'])} tables, {len(rep['files'])} files written to {rep['dir_out']} in {rep['wall_s']:.2f} s"
          + (f" ({rep['device_ms']:.2f} ms in kernels)" if "device_ms" in rep else ""))
    if a.json:
        try:
            Path(a.json).write_text(json.dumps(rep, indent=1) + "\n")
        except OSError as e:
            print(f"ndpp_amd.derive: cannot write {a.json}: {e}", file=sys.stderr)
            return EXIT_LIBRARY
    if rep["flagged"]:
        print(f"ndpp_amd.derive: {rep['flagged']} derived rows have a negative bin or are not finite; the library is "
              "written.  Negative bins come from Legendre rows that are negative somewhere: run the library through "
              "`python -m ndpp_amd.run --repair-positivity` first.", file=sys.stderr)
        return EXIT_FLAGGED
    return EXIT_OK


if __name__ == "__main__":
    sys.exit(main())
