"""Measures the derive entry points (ndpp_derive_groups, ndpp_derive_bins, ndpp_derive_moments,
include/ndpp_hip.h) at library size: one JSON line per case, to stdout and to --out.

The section: n incoming energies (default 1e5) x G groups (70) x L moments (11), seeded, rows
a_l = a_0 exp(-l (l + 1) tau); the tabular sections are the bins derived from it.  Per case, after one
small warm call:
  call_s        host clock around the synchronising call: tables, uploads, the kernel, downloads
  kernel_ms     ndpp_last_gpu_ms: device events around the call's one kernel
  bytes         what the algorithm has to move, from the shapes: the rows in, the rows out (three
                arrays for the moments with bounds) and one status word per row
  hbm_share     bytes over kernel_ms as a share of 8 TB/s (the peak; about 6.3 TB/s is achievable)
Per-kernel times come from running this script under `rocprofv3 --kernel-trace --stats` (a run of its
own; the kernel names are derive_groups_kernel, derive_bins_kernel<L>, derive_moments_kernel<Bounds>).
With --library-ein K > 0 a synthetic Legendre library of one table with K energies is written and
derived with `--bins 32` through ndpp_amd.derive.library: wall_s of the whole run next to device_ms.
No GPU: it fails, it does not fall back.

    python tools/bench_derive.py [--rows-ein 100000] [--groups 70] [--moments 11] [--bins 32 128]
                                 [--library-ein 20000] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12


def section(n: int, G: int, L: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    l = np.arange(L)
    a0, tau = rng.uniform(0.1, 2.0, (n, G, 1)), rng.uniform(0.15, 1.0, (n, G, 1))
    return a0 * np.exp(-(l * (l + 1))[None, None, :] * tau)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-ein", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=70)
    ap.add_argument("--moments", type=int, default=11)
    ap.add_argument("--bins", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--library-ein", type=int, default=20_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    from ndpp_amd import derive, reader
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        print("bench_derive: no HIP device", file=sys.stderr)
        return 3
    n, G, L = a.rows_ein, a.groups, a.moments
    lines = []

    def timed(case, bytes_moved, call, *args):
        t0 = time.perf_counter()
        out = call(*args)
        call_s = time.perf_counter() - t0
        ms = float(lib.ndpp_last_gpu_ms())
        rec = dict(case=case, n=n, G=G, L=L, call_s=round(call_s, 4), kernel_ms=round(ms, 4), bytes=int(bytes_moved),
                   hbm_bound_ms=round(bytes_moved / HBM_PEAK * 1e3, 4),
                   hbm_share=round(bytes_moved / (ms * 1e-3) / HBM_PEAK, 4) if ms > 0 else None)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        return out

    small = section(8, G, L, 1)                                   # warm: code objects, the allocator
    ndpp_amd.derive_groups(small, [0, G])
    ndpp_amd.derive_moments(ndpp_amd.derive_bins(small, 8)[0], L)

    y = section(n, G, L, 11)
    first = np.linspace(0, G, min(G, 7) + 1).astype(np.int32)
    Gc = len(first) - 1
    timed(f"groups_{G}_to_{Gc}", 8 * n * L * (G + Gc), ndpp_amd.derive_groups, y, first)
    for N in a.bins:
        rows = n * G
        t, status = timed(f"bins_N{N}", rows * (8 * L + 8 * N + 4), ndpp_amd.derive_bins, y, N)
        flagged = int(((status & (ndpp_amd.DERIVE_NEGBIN | ndpp_amd.DERIVE_NONFINITE)) != 0).sum())
        lines[-1]["flagged_rows"] = flagged
        timed(f"moments_N{N}_bounds", rows * (8 * N + 24 * L + 4), ndpp_amd.derive_moments, t, L)
        timed(f"moments_N{N}", rows * (8 * N + 8 * L + 4), ndpp_amd.derive_moments, t, L, False)
        if N % 4 == 0:
            seg = np.arange(0, N + 1, 4, dtype=np.int32)
            timed(f"merge_N{N}_to_{N // 4}", rows * 8 * (N + N // 4), ndpp_amd.derive_groups, t.reshape(rows, N, 1), seg)
        del t
    if a.library_ein > 0:
        k = a.library_ein
        e_bins = np.concatenate([[0.0], np.geomspace(1e-9, 20.0, G)])
        ein = np.geomspace(1e-11, 20.0, k)
        tab = reader.NdppTable("1001.71c", 2.53e-8, e_bins, reader.SCATT_TYPE_LEGENDRE, L - 1, False, False, 2001, 0.0)
        mat = y[:k]
        tab.elastic = reader.ScattSection(ein, ndpp_amd.group_index(e_bins, ein), np.ones(k, np.int32),
                                          np.full(k, G, np.int32), mat)
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = Path(tmp) / "in", Path(tmp) / "out"
            src.mkdir()
            (src / "1001.71c.g").write_bytes(derive.table_file(tab, ndpp_amd.FMT_BINARY))
            (src / "ndpp_lib.xml").write_bytes(ndpp_amd.lib_xml(
                str(src) + "/", ndpp_amd.FMT_BINARY,
                [dict(alias="H-1", awr=0.999167, name="1001.71c", path="1001.71c.g", kT=2.53e-8, zaid=1001,
                      freegas_cutoff=0.0)], e_bins, 0, L - 1, 2001, False, False, 0.0, 0.0))
            rep = derive.library(src, dst, bins=32)
            rec = dict(case="library_bins_N32", n=k, G=G, L=L, wall_s=round(rep["wall_s"], 3),
                       device_ms=round(rep["device_ms"], 3), flagged_rows=rep["flagged"],
                       bytes_in=(src / "1001.71c.g").stat().st_size, bytes_out=(dst / "1001.71c.g").stat().st_size)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
