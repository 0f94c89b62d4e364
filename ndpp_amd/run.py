"""Standalone driver: `python -m ndpp_amd.run <dir> [--json FILE]` reads <dir>/ndpp.xml, the
cross_sections.xml it names and the ACE tables listed there, and writes the NDPP library --
one `<name><library_name>` file per table (default library_name `.g<G>`) and ndpp_lib.xml --
into <dir>, under the names and in the formats the reference's `ndpp <dir>` writes.

Every step goes through the C ABI (include/ndpp_hip.h):
  neutron tables   all in ONE scatt_library (scatt_library_tab for scatt_type tabular) call;
  chi              chi_egrid_lib + chi_batch per fissionable table (integrate_chi);
  thermal tables   sab_egrid_lib (+ the extra top point) + sab_batch (sab_tab_batch with
                   --thermal-tabular);
  every table      finish_scatt (print_tol, thinning when thinning_tol > 0), nuclide_file;
  the run          lib_xml.
ndpp.xml is read with the reference's defaults (constants.F90) and refusals (ndpp.F90
init_ndpp); `threads` is accepted and ignored; output_format hdf5 and human are refused (the
library writes neither); tabular output of a thermal table is refused before anything is
computed unless --thermal-tabular asks for it (below).

Exit status: 0 library written, 2 input error (nothing written), 3 library or device error
(nothing written).  Files are written under temporary names and renamed once every table is
done, so a failed run leaves no partial library.
--json FILE: one record per table (kind, incoming energies, wall time, device time; `bins: N` for
a thermal table written in bins).

Thermal tables in bins (scatt_type tabular only; with scatt_type legendre the flag is an input
error):
  --thermal-tabular    the thermal tables go through sab_egrid_lib, the extra top point and
                       sab_tab_batch with N = scatt_order, and are written with is_sab = 2: every
                       discrete cosine's mass, whole, in the bin that holds it (include/ndpp_hip.h;
                       DESIGN.md section 17).  Opt-in because a histogram of point masses moves mass
                       from one bin to the next as E_in moves: such rows do not interpolate between
                       grid points the way the neutron tables' rows do.  Without the flag a tabular
                       run that lists a thermal table is refused, as before.

Grid quality (ndpp_amd.gridcheck; Legendre output only, scatt_type tabular with either flag is an
input error):
  --check-grid         once every table is computed, and before anything is written, integrate
                       every table at the midpoints of its incoming grids; the files written are
                       those of a run without the flag.  Prints, per table and section, the worst
                       error of interpolating between grid points; the report goes under "grid" in
                       --json.  The exit status does not depend on what the check finds (a device
                       error during the check is a library error like any other: exit 3, nothing
                       written).
  --refine-grid TOL    before print_tol / thinning / writing, insert midpoint rows into the grids
                       of the neutron tables until no interval's error is above TOL
                       (--max-passes N, default 6; --max-growth X, default 4); what stays above
                       TOL is reported as unresolved.  With --check-grid the refined grids are
                       what is checked.
  --check-tol X        the tolerance --check-grid counts intervals against (default: TOL of
                       --refine-grid, else 1e-3); an input error without --check-grid.
  --thin-grid TOL      before print_tol / thinning / writing, and after --refine-grid when both are
                       given, drop the points of the neutron tables' grids that interpolation between
                       the kept neighbours reproduces to TOL under the same metric (ndpp_amd.thin;
                       --thin-window W, default 32, the longest run of points one segment may skip,
                       2..64).  Group edges, the free-gas cutoff and the reaction thresholds are
                       kept.  Thermal tables and chi grids are not thinned.  With --check-grid the
                       thinned grids are what is checked.  `thinning_tol` of ndpp.xml -- the
                       reference's rule, the thin_tol of the file header -- is independent of it.

Positivity (ndpp_amd.repair; Legendre output only):
  --repair-positivity  the last step before a table's file is formed, after print_tol and thinning:
                       every row whose certified minimum (`validate --certified`) is negative is
                       replaced by a_l * w_l(t), the largest t of a bisection whose row is certified
                       positive.  The certified rows are exactly the rows
                       written; P0, the grids and gmin / gmax do not change; the file header is the
                       reference's and carries no mark.  One line per table and section is printed
                       and the report goes under "repair" in --json.  The figures of --check-grid,
                       --refine-grid and --thin-grid refer to the unrepaired rows: the report's
                       largest change is what the user adds to them.  scatt_type tabular is an input
                       error (bins are non-negative already).
  --repair-mode M      best (default: the family that keeps more), heat or uniform
  --repair-steps N     bisection steps, 1..52 (default 20): t is within 2^-N of a failing value
  --repair-rel-tol X   the certificate's tolerance, finite and >= 0 (default 1e-10)
  --repair-undecided   also repair rows whose minimum is within the tolerance of zero
                       Each of the four is an input error without --repair-positivity.

N-body phase space (ACE law 66):
  --nbody              integrate the reactions whose energy distribution is law 66 (deuterium's
                       (n,2n) is the best-known one) in closed form (lib.set_nbody; DESIGN.md section
                       20).  Without the flag they add nothing to the library, as in the reference.
                       The option is set for the run's library calls and put back afterwards; how many
                       reactions were integrated under law 66 goes under "nbody" in --json.  A tabular
                       run whose tables carry law 66 is an input error.
  --nbody-tabular      --nbody, and in a tabular run law 66 goes into the bins too (lib.set_nbody_tab:
                       ndpp_nbody_tab_batch, bins that cannot go negative) instead of being an input
                       error.  Both options are set for the run and put back afterwards; "nbody" in
                       --json gains "tabular": true."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
import xml.etree.ElementTree as ET
from pathlib import Path

import numpy as np

from . import ace, grid, gridcheck, lib, repair, thin

EXIT_OK, EXIT_INPUT, EXIT_LIBRARY = 0, 2, 3

# constants.F90 defaults of the reference
DEFAULTS = dict(scatt_type="legendre", scatt_order=5, nuscatter=False, integrate_chi=True, mu_bins=2001,
                output_format="binary", thinning_tol=0.0, print_tol=1.0e-8, freegas_cutoff=400.0,
                sab_threshold=1.0e-6, brent_mu_thresh=1.0e-6, adaptive_mu_tol=1.0e-7, adaptive_eout_tol=1.0e-8,
                adaptive_mu_its=15, adaptive_eout_its=15, sab_epts_per_bin=10, ne_per_grp=20, extend_pts=50,
                inel_extend_pts=30)
MAX_LEGENDRE_ORDER = 10
GLOBAL_FREEGAS_CUTOFF, INFINITE_FREEGAS_CUTOFF = -2.0, -1.0
_REALS = ("thinning_tol", "print_tol", "freegas_cutoff", "sab_threshold", "brent_mu_thresh", "adaptive_mu_tol",
          "adaptive_eout_tol")
_INTS = ("scatt_order", "mu_bins", "threads", "adaptive_mu_its", "adaptive_eout_its", "sab_epts_per_bin",
         "ne_per_grp", "extend_pts", "inel_extend_pts")


class InputError(ValueError):
    """An input the reference refuses (or this library cannot honour): exit status 2."""


def _warn(msg: str) -> None:
    print(f"ndpp_amd.run: warning: {msg}", file=sys.stderr)


def _text(root, tag):
    el = root.find(tag)
    return None if el is None or el.text is None else el.text.strip()


def _num(root, tag, kind):
    s = _text(root, tag)
    if s is None or s == "":
        return None
    try:
        v = kind(s.replace("D", "E").replace("d", "e")) if kind is float else int(s)
    except ValueError:
        raise InputError(f"ndpp.xml: <{tag}> {s!r} is not {'a number' if kind is float else 'an integer'}") from None
    if kind is float and not math.isfinite(v):
        raise InputError(f"ndpp.xml: <{tag}> must be finite")
    return v


def _parse_xml(path: Path, what: str):
    try:
        return ET.parse(path).getroot()
    except FileNotFoundError:
        raise InputError(f"{what} '{path}' does not exist!") from None
    except (ET.ParseError, OSError) as e:
        raise InputError(f"{what} '{path}': {e}") from None


def read_ndpp_xml(run_dir) -> dict:
    """The run settings of <run_dir>/ndpp.xml (see the module docstring)."""
    run_dir = Path(run_dir)
    root = _parse_xml(run_dir / "ndpp.xml", "Data Pre-Processing XML file")
    s = dict(DEFAULTS)
    for k in _REALS:
        v = _num(root, k, float)
        if v is not None:
            s[k] = v
    for k in _INTS:
        v = _num(root, k, int)
        if v is not None:
            s[k] = v
    xs = _text(root, "cross_sections") or os.environ.get("CROSS_SECTIONS", "").strip()
    if not xs:
        raise InputError("No cross_sections.xml file was specified in ndpp.xml or in the CROSS_SECTIONS "
                         "environment variable.")
    s["cross_sections"] = str(run_dir / xs) if not os.path.isabs(xs) else xs
    for k in ("integrate_chi", "nuscatter"):
        w = (_text(root, k) or "").lower()
        if w in ("true", "false"):
            s[k] = w == "true"
        elif w:
            _warn(f"Value for <{k}> provided, but does not match TRUE or FALSE. Using default of "
                  f"{str(DEFAULTS[k]).upper()}.")
    eb = _text(root, "energy_bins")
    if not eb:
        raise InputError("No energy group structure was specified in ndpp.xml.")
    try:
        bins = np.array([float(v.replace("D", "E").replace("d", "e")) for v in eb.split()], dtype=np.float64)
    except ValueError:
        raise InputError("Invalid energy group structure specified in ndpp.xml; not a list of numbers.") from None
    if len(bins) < 2 or not np.isfinite(bins).all():
        raise InputError("Invalid energy group structure specified in ndpp.xml; need at least two finite edges.")
    if (bins[:-1] < 0).any():
        raise InputError("Invalid energy group structure specified in ndpp.xml; Groups boundaries be positive.")
    if (bins[:-1] >= bins[1:]).any():
        raise InputError("Invalid energy group structure specified in ndpp.xml; Group boundaries must be in "
                         "increasing order.")
    if bins[0] != 0.0:
        raise InputError("Invalid Lower Energy Boundary: Bottom of Lowest Group  Must be Zero!")
    s["energy_bins"] = bins
    fmt = (_text(root, "output_format") or "binary").lower()
    if fmt in ("hdf5", "human"):
        raise InputError(f"<output_format> {fmt} is not supported: this library writes ascii, binary or none.")
    if fmt not in ("ascii", "binary", "none"):
        _warn("Value for <output_format> provided, but does not match ASCII, BINARY, HDF5, HUMAN, or NONE. "
              "Using default of BINARY.")
        fmt = "binary"
    s["output_format"] = fmt
    s["lib_format"] = {"ascii": lib.FMT_ASCII, "binary": lib.FMT_BINARY, "none": lib.FMT_NONE}[fmt]
    G = len(bins) - 1
    s["library_name"] = _text(root, "library_name") or f".g{G}"
    st = (_text(root, "scatt_type") or "legendre").lower()
    if st not in ("legendre", "tabular"):
        _warn(f"Value for <scatt_type> {st!r} does not match LEGENDRE or TABULAR. Using default of LEGENDRE.")
        st = "legendre"
    s["scatt_type"] = st
    n = s["scatt_order"]
    if n <= 0 or (st == "legendre" and n > MAX_LEGENDRE_ORDER):
        raise InputError("Invalid negative or zero scatt_order value specified in ndpp.xml." +
                         (f" (Legendre orders go up to {MAX_LEGENDRE_ORDER})" if n > 0 else ""))
    if st == "tabular" and n > lib.MAX_TAB_BINS:
        raise InputError(f"<scatt_order> {n}: tabular output holds at most {lib.MAX_TAB_BINS} bins.")
    fc = s["freegas_cutoff"]
    if fc == INFINITE_FREEGAS_CUTOFF:
        s["freegas_cutoff"] = math.inf
    elif fc < 0:
        raise InputError("Invalid negative value of <freegas_cutoff> specified in ndpp.xml. Specify -1 if no "
                         "cutoff is desired; all other values are invalid.")
    if s["thinning_tol"] < 0:
        _warn("Invalid thinning tolerance provided, setting to default of no thinning.")
        s["thinning_tol"] = 0.0
    s["thin_tol"] = 0.01 * s["thinning_tol"]                 # percent -> fraction
    if s["print_tol"] <= 0:
        _warn("Invalid printing tolerance provided, setting to default.")
        s["print_tol"] = DEFAULTS["print_tol"]
    if s["mu_bins"] <= 1:
        raise InputError("Invalid mu_bins value specified in ndpp.xml. Mu_bins must be two or greater.")
    for k in ("sab_threshold", "brent_mu_thresh", "adaptive_mu_tol", "adaptive_eout_tol", "sab_epts_per_bin",
              "ne_per_grp", "extend_pts", "inel_extend_pts", "adaptive_mu_its", "adaptive_eout_its"):
        if s[k] < 0:
            raise InputError(f"Invalid <{k}> value specified in ndpp.xml; value must be positive.")
    for k in ("adaptive_mu_its", "adaptive_eout_its"):
        if s[k] > 31:
            raise InputError(f"Invalid <{k}> value {s[k]} specified in ndpp.xml; the library takes 0..31.")
    return s


def read_cross_sections(path) -> dict:
    """cross_sections.xml: directory (default: the file's own), filetype, record_length, entries,
    and the ace_table listings with their attributes (freegas_cutoff in kT: -2 = the ndpp.xml
    value, -1 = no cutoff)."""
    path = Path(path)
    root = _parse_xml(path, "Cross sections XML file")
    directory = _text(root, "directory") or str(path.parent)
    ft = (_text(root, "filetype") or "ascii")
    if ft not in ("ascii", "binary"):
        raise InputError(f"Unknown filetype in cross_sections.xml: {ft}")
    try:
        recl, entries = int(_text(root, "record_length") or 0), int(_text(root, "entries") or 0)
    except ValueError:
        raise InputError("cross_sections.xml: <record_length> and <entries> must be integers") from None
    els = root.findall("ace_table")
    if not els:
        raise InputError("No ACE table listings present in cross_sections.xml file!")
    out = []
    for el in els:
        a = el.attrib
        name = a.get("name", "").strip()
        try:
            lst = dict(name=name, alias=a.get("alias", "").strip(), zaid=int(a.get("zaid", 0)),
                       metastable=int(a.get("metastable", 0)) != 0, awr=float(a.get("awr", 0.0)),
                       kT=float(a.get("temperature", 0.0)), location=int(a.get("location", 0)),
                       freegas_cutoff=float(a.get("freegas_cutoff", GLOBAL_FREEGAS_CUTOFF)))
        except ValueError as e:
            raise InputError(f"cross_sections.xml: ace_table {name!r}: {e}") from None
        fc = lst["freegas_cutoff"]
        if fc < 0 and fc not in (INFINITE_FREEGAS_CUTOFF, GLOBAL_FREEGAS_CUTOFF):
            raise InputError("Invalid value of freegas_cutoff element in cross_sections.xml file!")
        p = a.get("path", "").strip()
        lst["path"] = p if p.startswith("/") else os.path.join(directory, p)
        lst["type"] = "neutron" if name.endswith("c") else "thermal" if name.endswith("t") else "other"
        out.append(lst)
    return dict(directory=directory, filetype=ft, record_length=recl, entries=entries, listings=out)


def params_of(s: dict) -> lib.Params:
    order = s["scatt_order"] + 1 if s["scatt_type"] == "legendre" else 1     # tabular: unused, valid
    p = lib.Params.default(order, s["mu_bins"])
    for k in ("sab_threshold", "brent_mu_thresh", "adaptive_mu_tol", "adaptive_eout_tol", "adaptive_mu_its",
              "adaptive_eout_its", "ne_per_grp", "sab_epts_per_bin", "extend_pts", "inel_extend_pts"):
        setattr(p, k, s[k])
    return p


def options_of(s: dict) -> lib.OutputOptions:
    return lib.OutputOptions(lib_format=s["lib_format"], scatt_type=int(s["scatt_type"] == "tabular"),
                             scatt_order=s["scatt_order"], nuscatter=int(s["nuscatter"]),
                             integrate_chi=int(s["integrate_chi"]), mu_bins=s["mu_bins"], print_tol=s["print_tol"],
                             thin_tol=s["thin_tol"])


def load_tables(s: dict, xs: dict) -> list:
    """Read every listed table.  Returns [dict(listing, kind, data, file)] in listing order
    (tables that are neither neutron nor thermal are skipped, as the reference does)."""
    out = []
    for lst in xs["listings"]:
        if lst["type"] == "other":
            _warn(f"Invalid Entry in cross_sections listings: {lst['name']!r}. NDPP does not support dosimetry "
                  "Tables! Entry will be ignored.")
            continue
        try:
            t = ace.read_table(lst["path"], lst["location"], xs["filetype"], xs["record_length"], xs["entries"],
                               expect_name=lst["name"])
            data = ace.neutron(t) if lst["type"] == "neutron" else ace.thermal(t)
        except OSError as e:
            raise InputError(f"ACE library '{lst['path']}' ({lst['name']}): {e.strerror or e}") from None
        except ValueError as e:
            raise InputError(str(e)) from None
        base = t.name.strip() + s["library_name"].strip()
        if lst["type"] == "neutron":
            fc = lst["freegas_cutoff"]
            if fc == GLOBAL_FREEGAS_CUTOFF:
                fc = s["freegas_cutoff"]
            data["freegas_cutoff"] = math.inf if fc in (math.inf, INFINITE_FREEGAS_CUTOFF) else fc * data["kT"]
        else:
            i = base.find("/")                              # u/o2.10t -> u-o2.10t
            if i > 0:
                base = base[:i] + "-" + base[i + 1:]
        out.append(dict(listing=lst, kind=lst["type"], data=data, file=base))
    return out


def _device_ms() -> float:
    return float(sum(lib.profile_get().values()))


def compute(s: dict, tables: list, grid_opts: dict | None = None, repair_opts: dict | None = None) -> tuple:
    """Every table's file bytes, its timing record and the grid report: ([(file name, bytes)],
    [record], report).  The report is None without grid_opts (check, check_tol, refine_tol,
    max_passes, max_growth, thin_tol, thin_window).  With repair_opts (mode, steps, rel_tol,
    undecided) every table's finished rows are repaired before its file is formed and a fourth value
    is returned: [dict(name, kind, report)] per table."""
    p, o, bins = params_of(s), options_of(s), s["energy_bins"]
    tab = s["scatt_type"] == "tabular"
    th_tab = tab and bool(s.get("thermal_tabular"))         # --thermal-tabular: the thermal tables in bins too
    files, recs = [None] * len(tables), [None] * len(tables)
    go = grid_opts or {}
    raw, grid_rep = [None] * len(tables), None
    repair_rep = [None] * len(tables)

    def finish(k, result):
        fin, _ = lib.finish_scatt(o, result, bins)
        if repair_opts is not None:
            fin, rr = repair.repair_result(fin, **repair_opts)
            repair_rep[k] = dict(name=tables[k]["listing"]["name"], kind=tables[k]["kind"], report=rr)
        return fin
    neut = [k for k, t in enumerate(tables) if t["kind"] == "neutron"]
    if neut:
        lib.profile_reset()
        t0 = time.perf_counter()
        nucs = [tables[k]["data"] for k in neut]
        res = (lib.scatt_library_tab(p, s["scatt_order"], nucs, bins, s["nuscatter"]) if tab else
               lib.scatt_library(p, nucs, bins, s["nuscatter"]))
        wall, dev, last = time.perf_counter() - t0, _device_ms(), float(lib.load().ndpp_last_gpu_ms())
        call = "scatt_library_tab" if tab else "scatt_library"
        if go.get("refine_tol") is not None:
            t1 = time.perf_counter()
            res, rep = gridcheck.refine(p, bins, [tables[k] for k in neut], res, s["nuscatter"], go["refine_tol"],
                                        go["max_passes"], go["max_growth"])
            # one record per table of the run, in listing order: the thermal ones say that they are not refined
            by_table = dict(zip(neut, rep))
            rep = [by_table.get(k) or dict(name=t["listing"]["name"], kind=t["kind"], grids={},
                                           note="thermal table: checked, not refined")
                   for k, t in enumerate(tables)]
            grid_rep = dict(refine=dict(tol=go["refine_tol"], max_passes=go["max_passes"],
                                        max_growth=go["max_growth"], wall_s=time.perf_counter() - t1, tables=rep))
        if go.get("thin_tol") is not None:
            t1 = time.perf_counter()
            res, rep = thin.thin_results(p, bins, [tables[k] for k in neut], res, s["nuscatter"], go["thin_tol"],
                                         go["thin_window"])
            by_table = dict(zip(neut, rep))
            rep = [by_table.get(k) or dict(name=t["listing"]["name"], kind=t["kind"], sections={},
                                           note="thermal table: not thinned")
                   for k, t in enumerate(tables)]
            grid_rep = dict(grid_rep or {}, thin=dict(tol=go["thin_tol"], window=go["thin_window"],
                                                      wall_s=time.perf_counter() - t1, tables=rep))
        for k, r in zip(neut, res):
            raw[k] = r
            t = tables[k]
            chi, chi_rec = None, None
            if s["integrate_chi"] and t["data"]["fissionable"]:
                lib.profile_reset()
                c0 = time.perf_counter()
                case = ace.chi_case(t["data"])
                e_chi = lib.chi_egrid_lib(case)
                ct, cp, cd = lib.chi_batch(case, bins, e_chi)
                chi = (e_chi, ct, cp, cd)
                chi_rec = dict(energies=len(e_chi), wall_s=time.perf_counter() - c0, device_ms=_device_ms(),
                               last_gpu_ms=float(lib.load().ndpp_last_gpu_ms()))
            fin = finish(k, r)
            if s["lib_format"] != lib.FMT_NONE:
                files[k] = lib.nuclide_file(o, t["data"]["name"], t["data"]["kT"], fin, bins, chi=chi)
            recs[k] = dict(name=t["listing"]["name"], kind="neutron", file=t["file"],
                           energies=dict(elastic=len(r["ein_el"]),
                                         inelastic=0 if r["ein_inel"] is None else len(r["ein_inel"])),
                           batch=dict(call=call, tables=len(neut), wall_s=wall, device_ms=dev, last_gpu_ms=last),
                           chi=chi_rec)
    for k, t in enumerate(tables):
        if t["kind"] != "thermal":
            continue
        d = t["data"]
        lib.profile_reset()
        t0 = time.perf_counter()
        ein = grid.add_one_more_point(lib.sab_egrid_lib(p, d, bins))
        mat = lib.sab_tab_batch(p, s["scatt_order"], d, ein, bins) if th_tab else lib.sab_batch(p, d, ein, bins)
        wall, dev, last = time.perf_counter() - t0, _device_ms(), float(lib.load().ndpp_last_gpu_ms())
        raw[k] = dict(ein_el=ein, el_mat=mat, ein_inel=None, inel_mat=None, nuinel_mat=None)
        fin = finish(k, dict(ein_el=ein, el_mat=mat, ein_inel=None, inel_mat=None, nuinel_mat=None))
        if s["lib_format"] != lib.FMT_NONE:
            files[k] = lib.nuclide_file(o, d["name"], d["kT"], fin, bins, is_sab=2 if th_tab else True)
        recs[k] = dict(name=t["listing"]["name"], kind="thermal", file=t["file"],
                       energies=dict(elastic=len(ein), inelastic=0), wall_s=wall, device_ms=dev, last_gpu_ms=last)
        if th_tab:
            recs[k]["bins"] = s["scatt_order"]
    out = [(t["file"], f) for t, f in zip(tables, files)]
    if go.get("check"):
        t1 = time.perf_counter()
        rep = gridcheck.check(p, bins, tables, raw, s["nuscatter"], go["check_tol"])
        grid_rep = dict(grid_rep or {}, check=dict(tol=go["check_tol"], wall_s=time.perf_counter() - t1, tables=rep))
    if repair_opts is not None:
        return out, recs, grid_rep, repair_rep
    return out, recs, grid_rep


def nbody_reactions(tables: list, bins) -> dict:
    """Per neutron table that carries law 66: the number of reactions --nbody integrates under it (a
    scattering MT, is_valid_scatter, whose threshold energy is below the top group edge)."""
    out = {}
    for t in tables:
        if t["kind"] != "neutron":
            continue
        d, n, carries = t["data"], 0, False
        for r in d["reactions"]:
            if not any(int(ed["law"]) == 66 for ed in r["edists"]):
                continue
            carries = True
            mt = int(r["MT"])
            valid = mt == 2 or (11 <= mt <= 91 and mt not in ace.FISSION_MTS)
            if valid and max(float(d["energy"][int(r["thr"]) - 1]), float(bins[0])) < float(bins[-1]):
                n += 1
        if carries:
            out[t["listing"]["name"]] = n
    return out


def lib_xml_of(s: dict, run_dir, tables: list) -> bytes:
    rows = []
    for t in tables:
        lst, d = t["listing"], t["data"]
        thermal = t["kind"] == "thermal"
        rows.append(dict(alias=lst["name"] if thermal else lst["alias"], awr=lst["awr"], name=lst["name"],
                         path=t["file"], kT=lst["kT"], zaid=lst["zaid"], metastable=lst["metastable"],
                         freegas_cutoff=lst["freegas_cutoff"] if thermal else d["freegas_cutoff"]))
    return lib.lib_xml(str(Path(run_dir).resolve()) + "/", s["lib_format"], rows, s["energy_bins"],
                       int(s["scatt_type"] == "tabular"), s["scatt_order"], s["mu_bins"], s["nuscatter"],
                       s["integrate_chi"], s["print_tol"], s["thin_tol"])


def _refuse_thermal_tabular(s: dict, tables: list) -> None:
    """scatt_type tabular with a thermal table: the writer's refusal, before any device work."""
    if s["scatt_type"] != "tabular" or s["lib_format"] == lib.FMT_NONE:
        return
    th = [t for t in tables if t["kind"] == "thermal"]
    if not th:
        return
    probe = dict(ein_el=np.array([1e-11, 1.0]), el_mat=np.zeros((2, len(s["energy_bins"]) - 1, 1)), ein_inel=None,
                 inel_mat=None, nuinel_mat=None)
    try:
        lib.nuclide_file(options_of(s), th[0]["data"]["name"], th[0]["data"]["kT"], probe, s["energy_bins"],
                         is_sab=True)
    except lib.NdppError as e:
        raise InputError(f"{th[0]['listing']['name']}: {e}") from None


def write_library(run_dir, files: list, xml: bytes) -> list:
    """Write every file under a temporary name, then rename them all; on any failure remove
    what was written.  Returns the paths written."""
    run_dir = Path(run_dir)
    items = [(run_dir / name, data) for name, data in files if data is not None] + \
            ([(run_dir / "ndpp_lib.xml", xml)] if xml else [])
    tmp = []
    try:
        for path, data in items:
            t = path.with_name(f".{path.name}.{os.getpid()}.tmp")
            tmp.append(t)
            t.write_bytes(data)
        for (path, _), t in zip(items, tmp):
            os.replace(t, path)
    except BaseException:
        for t in tmp:
            t.unlink(missing_ok=True)
        raise
    return [p for p, _ in items]


def run(run_dir, json_path=None, out=sys.stdout, grid_opts: dict | None = None,
        repair_opts: dict | None = None, thermal_tabular: bool = False, nbody: bool = False,
        nbody_tabular: bool = False) -> int:
    """The whole driver; returns the exit status."""
    nbody = nbody or nbody_tabular                          # --nbody-tabular implies --nbody
    run_dir = Path(run_dir)
    t_start = time.perf_counter()
    try:
        s = read_ndpp_xml(run_dir)
        if thermal_tabular and s["scatt_type"] != "tabular":
            raise InputError("--thermal-tabular asks for the thermal tables of a tabular run in bins: give it with "
                             "<scatt_type> tabular")
        s["thermal_tabular"] = bool(thermal_tabular)
        if grid_opts is not None and s["scatt_type"] == "tabular":
            raise InputError("--check-grid, --refine-grid and --thin-grid cover Legendre output only: the tabular rows of the "
                             "free-gas range do not settle, so an error measured on them would be the "
                             "quadrature's, not the grid's.")
        if repair_opts is not None and s["scatt_type"] == "tabular":
            raise InputError("--repair-positivity covers Legendre output only: the bins of tabular output are "
                             "non-negative already.")
        xs = read_cross_sections(s["cross_sections"])
        tables = load_tables(s, xs)
        if not tables:
            raise InputError("no neutron or thermal tables to process")
        law66 = nbody_reactions(tables, s["energy_bins"]) if nbody else {}
        if law66 and s["scatt_type"] == "tabular" and not nbody_tabular:
            raise InputError(f"--nbody: {', '.join(law66)} carries ACE law 66, which has Legendre output only: give "
                             "it with <scatt_type> legendre, or give --nbody-tabular")
    except InputError as e:
        print(f"ndpp_amd.run: input error: {e}", file=sys.stderr)
        return EXIT_INPUT
    try:
        lib.load()
        try:
            if not s["thermal_tabular"]:
                _refuse_thermal_tabular(s, tables)
        except InputError as e:
            print(f"ndpp_amd.run: input error: {e}", file=sys.stderr)
            return EXIT_INPUT
        repair_rep = None
        nbody_before = lib.set_nbody(True) if nbody else False
        nbody_tab_before = lib.set_nbody_tab(True) if nbody_tabular else False
        try:
            if repair_opts is not None:
                files, recs, grid_rep, repair_rep = compute(s, tables, grid_opts, repair_opts)
            else:
                files, recs, grid_rep = compute(s, tables, grid_opts)
        finally:
            if nbody_tabular:
                lib.set_nbody_tab(nbody_tab_before)
            if nbody:
                lib.set_nbody(nbody_before)
        xml = lib_xml_of(s, run_dir, tables)
    except (lib.NdppError, RuntimeError, OSError) as e:
        print(f"ndpp_amd.run: library error: {e}", file=sys.stderr)
        return EXIT_LIBRARY
    try:
        written = write_library(run_dir, files, xml)
    except OSError as e:
        print(f"ndpp_amd.run: cannot write the library: {e}", file=sys.stderr)
        return EXIT_LIBRARY
    total = time.perf_counter() - t_start
    for r in recs:
        print(f"{r['name']:>12s} {r['kind']:8s} {r['energies']['elastic']:7d} + {r['energies']['inelastic']:6d} E_in"
              f"  -> {r['file']}", file=out)
    print(f"{len(tables)} tables, {len(written)} files written in {total:.2f} s", file=out)
    if grid_rep and "refine" in grid_rep:
        for t in grid_rep["refine"]["tables"]:
            for name, g in t["grids"].items():
                print(f"{t['name']:>12s} {name:13s} refined to {grid_rep['refine']['tol']:g}: {g['points_before']} -> "
                      f"{g['points_after']} E_in in {g['passes']} passes ({g['stopped']}), {len(g['unresolved'])} "
                      f"unresolved ({sum(u['at_breakpoint'] for u in g['unresolved'])} at a breakpoint)", file=out)
    if grid_rep and "thin" in grid_rep:
        for line in thin.format_lines(grid_rep["thin"]["tables"], grid_rep["thin"]["tol"]):
            print(line, file=out)
    if grid_rep and "check" in grid_rep:
        for line in gridcheck.format_lines(grid_rep["check"]["tables"]):
            print(line, file=out)
    if repair_rep is not None:
        for t in repair_rep:
            for line in repair.format_lines(t["name"], t["report"]):
                print(line, file=out)
    if json_path:
        rec = dict(run_dir=str(run_dir), wall_s=total, scatt_type=s["scatt_type"], tables=recs)
        if grid_opts is not None:
            rec["grid"] = grid_rep
        if nbody:
            rec["nbody"] = dict(reactions=sum(law66.values()), tables=law66)
            if nbody_tabular:
                rec["nbody"]["tabular"] = True
        if repair_rep is not None:
            rec["repair"] = dict(repair_opts, tables=[dict(name=t["name"], kind=t["kind"], **t["report"].as_dict())
                                                      for t in repair_rep])
        Path(json_path).write_text(json.dumps(rec, indent=1) + "\n")
    return EXIT_OK


def _grid_options(a):
    """The grid flags as compute()'s grid_opts (None: no flag given).  Raises InputError."""
    if a.check_tol is not None and not a.check_grid:
        raise InputError("--check-tol is the tolerance of --check-grid: give both")
    if a.thin_window is not None and a.thin_grid is None:
        raise InputError("--thin-window is the window of --thin-grid: give both")
    if not a.check_grid and a.refine_grid is None and a.thin_grid is None:
        return None

    def positive(flag, text):
        try:
            v = float(text)
        except ValueError:
            raise InputError(f"{flag} {text!r} is not a number") from None
        if not (v > 0.0) or not math.isfinite(v):
            raise InputError(f"{flag} {text!r}: a positive, finite number is expected")
        return v

    tol = None if a.refine_grid is None else positive("--refine-grid", a.refine_grid)
    ctol = positive("--check-tol", a.check_tol) if a.check_tol is not None else (tol if tol is not None else 1.0e-3)
    if a.max_passes < 0:
        raise InputError(f"--max-passes {a.max_passes}: must not be negative")
    if not (a.max_growth >= 1.0):
        raise InputError(f"--max-growth {a.max_growth}: must be at least 1")
    thin_tol = None if a.thin_grid is None else positive("--thin-grid", a.thin_grid)
    window = 32 if a.thin_window is None else a.thin_window
    if not 2 <= window <= 64:
        raise InputError(f"--thin-window {window}: must be between 2 and 64")
    return dict(check=bool(a.check_grid), check_tol=ctol, refine_tol=tol, max_passes=a.max_passes,
                max_growth=a.max_growth, thin_tol=thin_tol, thin_window=window)


def _repair_options(a):
    """The repair flags as compute()'s repair_opts (None: --repair-positivity not given).  Raises InputError."""
    given = [f for f, v in (("--repair-mode", a.repair_mode), ("--repair-steps", a.repair_steps),
                            ("--repair-rel-tol", a.repair_rel_tol), ("--repair-undecided", a.repair_undecided or None))
             if v is not None]
    if not a.repair_positivity:
        if given:
            raise InputError(f"{', '.join(given)}: a setting of --repair-positivity; give that flag too")
        return None
    steps = 20 if a.repair_steps is None else a.repair_steps
    rel_tol = 1e-10 if a.repair_rel_tol is None else a.repair_rel_tol
    try:
        repair.check_options(steps, rel_tol)
    except ValueError as e:
        raise InputError(str(e)) from None
    return dict(mode=a.repair_mode or "best", steps=steps, rel_tol=rel_tol, undecided=bool(a.repair_undecided))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ndpp_amd.run",
                                 description="Build an NDPP library from <dir>/ndpp.xml and the ACE tables its "
                                             "cross_sections.xml lists (exit 0: written, 2: input error, "
                                             "3: library or device error; nothing is written on failure).")
    ap.add_argument("run_dir", help="directory holding ndpp.xml; the library is written there")
    ap.add_argument("--json", default=None, help="write per-table timings to this file")
    ap.add_argument("--check-grid", action="store_true",
                    help="measure the interpolation error of every incoming-energy grid against midpoint integrals")
    ap.add_argument("--refine-grid", metavar="TOL", default=None,
                    help="insert midpoint rows into the neutron tables' grids until that error is below TOL")
    ap.add_argument("--max-passes", type=int, default=6, help="refinement passes at most (default 6)")
    ap.add_argument("--max-growth", type=float, default=4.0,
                    help="a grid stops refining before it exceeds this multiple of its length (default 4)")
    ap.add_argument("--check-tol", metavar="X", default=None,
                    help="tolerance --check-grid counts intervals against (default: TOL, else 1e-3)")
    ap.add_argument("--thin-grid", metavar="TOL", default=None,
                    help="drop the grid points of the neutron tables that interpolation between their kept "
                         "neighbours reproduces to TOL")
    ap.add_argument("--thin-window", metavar="W", type=int, default=None,
                    help="points one thinned segment may span, 2..64 (default 32)")
    ap.add_argument("--repair-positivity", action="store_true",
                    help="replace every row whose certified minimum is negative by a filtered row that is "
                         "certified positive (Legendre output only)")
    ap.add_argument("--repair-mode", choices=sorted(repair.MODES), default=None,
                    help="filter family: best (default), heat or uniform")
    ap.add_argument("--repair-steps", metavar="N", type=int, default=None, help="bisection steps, 1..52 (default 20)")
    ap.add_argument("--repair-rel-tol", metavar="X", type=float, default=None,
                    help="tolerance of the certificate, finite and >= 0 (default 1e-10)")
    ap.add_argument("--repair-undecided", action="store_true",
                    help="also repair rows whose minimum is within the tolerance of zero")
    ap.add_argument("--thermal-tabular", action="store_true",
                    help="with scatt_type tabular: write the thermal S(alpha,beta) tables in bins too, every "
                         "discrete cosine's mass whole in its bin (without it such a run is refused)")
    ap.add_argument("--nbody", action="store_true",
                    help="integrate the reactions under ACE law 66 (N-body phase space) in closed form; without it "
                         "they add nothing, as in the reference (Legendre output only)")
    ap.add_argument("--nbody-tabular", action="store_true",
                    help="--nbody, and with scatt_type tabular the law-66 reactions go into the bins too (without "
                         "it such a run is refused)")
    a = ap.parse_args(argv)
    try:
        grid_opts = _grid_options(a)
        repair_opts = _repair_options(a)
    except InputError as e:
        print(f"ndpp_amd.run: input error: {e}", file=sys.stderr)
        return EXIT_INPUT
    return run(a.run_dir, a.json, grid_opts=grid_opts, repair_opts=repair_opts, thermal_tabular=a.thermal_tabular,
               nbody=a.nbody, nbody_tabular=a.nbody_tabular)


if __name__ == "__main__":
    sys.exit(main())
