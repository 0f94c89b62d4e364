"""Measures scoring events into tallies (ndpp_scatt_score, include/ndpp_hip.h): one JSON line per case,
to stdout and to --out.

The section: n incoming energies (default 2000, log-spaced) x G groups x L entries.  Its rows are
banded as a library's are: at energy index r the groups that scatter are the `width` groups ending at
the group the energy falls in (G = 70: width 12; G = 2: both), Legendre rows a_l = a_0 exp(-l (l + 1)
tau), tabular rows uniform bins; every other element is exactly 0.0.  The events (default 1e6):
energies log-uniform over the grid, weights uniform in [0.5, 1.5], bins uniform over n_bins.

Shapes: (G, L) = (2, 6) and (70, 11) Legendre, (70, 32) tabular, each into 1, 70 and 10^4 bins, with
normalize 1.  Per case, warm (one untimed call first), --repeat timed calls ALTERNATING between the band
skip on and off (NDPP_SCORE_BAND=0), so that both see the same machine:
  call_s        host clock around the synchronising call, per run, and the best
  info          ndpp_scatt_score_info of the best run: bracket_ms, factor_ms (masses, bands, factors and
                the status download), group_ms (counting sort, chunk table), upload_ms, kernel_ms
                (device events around gather, chunk and fold kernels), download_ms, passes, chunks
  host_share    (bracket + group + upload) / call
  band_elements the elements inside the events' bands, summed over the events, counted from the
                section on the host with the rule of the header; dense_elements = events x G x L
  bytes_band    band_elements x 16 (two stored values per element)
  events_per_s  over call_s and over kernel_ms
  bytes_per_s   bytes_band over kernel_ms: the EFFECTIVE rate of the chunk kernel's row reads (the rows
                are a few MB and come from the caches, not from HBM; this is no share of the HBM peak);
                for the dense run dense_elements x 16 over its kernel_ms
Kernel times per kernel come from running this script under `rocprofv3 --kernel-trace --stats` with
--repeat 1 --modes band --cases <one case>.  No GPU: it fails, it does not fall back.

    python tools/bench_score.py [--rows-ein 2000] [--events 1000000] [--repeat 3] [--cases NAME ...]
                                [--modes band dense] [--check-events 20000] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [("leg_g2_l6", 0, 2, 6), ("leg_g70_l11", 0, 70, 11), ("tab_g70_n32", 1, 70, 32)]
BINS = [1, 70, 10000]


def section(scatt_type: int, n: int, G: int, L: int, seed: int):
    rng = np.random.default_rng(seed)
    x = np.geomspace(1e-11, 20.0, n)
    width = min(G, 12)
    top = np.minimum((np.arange(n) * G) // n, G - 1)             # the group the energy falls in
    if scatt_type == 1:
        rows = rng.random((n, G, L))
    else:
        l = np.arange(L)
        a0, tau = rng.uniform(0.1, 2.0, (n, G, 1)), rng.uniform(0.15, 1.0, (n, G, 1))
        rows = a0 * np.exp(-(l * (l + 1))[None, None, :] * tau)
    g = np.arange(G)[None, :]
    keep = (g <= top[:, None]) & (g > top[:, None] - width)
    return x, rows * keep[:, :, None]


def band_elements(x, y, ein) -> int:
    """sum over the events of L x (groups in the union of the two rows' bands), the header's rule"""
    n, G, L = y.shape
    nz = (y != 0.0).any(axis=2)
    lo = np.where(nz.any(axis=1), nz.argmax(axis=1), G)
    hi = np.where(nz.any(axis=1), G - 1 - nz[:, ::-1].argmax(axis=1), -1)
    i = np.clip(np.searchsorted(x, ein, side="right") - 1, 0, n - 1)
    i1 = np.minimum(i + 1, n - 1)
    width = np.maximum(np.maximum(hi[i], hi[i1]) - np.minimum(lo[i], lo[i1]) + 1, 0)
    return int(width.sum()) * L


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-ein", type=int, default=2000)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3, help="timed calls per case and band setting, alternating")
    ap.add_argument("--cases", nargs="*", default=None, help="e.g. leg_g70_l11_b70 (default: all nine)")
    ap.add_argument("--modes", nargs="+", default=["band", "dense"], choices=["band", "dense"],
                    help="band: the product; dense: NDPP_SCORE_BAND=0 (for a kernel trace take one)")
    ap.add_argument("--check-events", type=int, default=20000, help="events of the bit check against score_numpy")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    from ndpp_amd import score
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        print("bench_score: no HIP device", file=sys.stderr)
        return 3
    n, n_ev = a.rows_ein, a.events
    rng = np.random.default_rng(7)
    ein = np.clip(np.exp(rng.uniform(np.log(1e-11), np.log(20.0), n_ev)), 1e-11, 20.0)
    weight = rng.uniform(0.5, 1.5, n_ev)
    where = rng.random(n_ev)
    lines = []
    for name, scatt_type, G, L in SHAPES:
        x, y = section(scatt_type, n, G, L, 11 + scatt_type)
        ein = np.clip(ein, x[0], x[-1])
        in_band = band_elements(x, y, ein)
        for n_bins in BINS:
            case = f"{name}_b{n_bins}"
            if a.cases and case not in a.cases:
                continue
            bins = np.minimum((where * n_bins).astype(np.int32), n_bins - 1)
            runs = {"band": [], "dense": []}
            os.environ.pop("NDPP_SCORE_BAND", None)
            ndpp_amd.scatt_score(1, scatt_type, x, y, ein, weight, bins, n_bins)          # warm: this shape, untimed
            keep = {}
            for _ in range(a.repeat):
                for mode in a.modes:
                    if mode == "dense":
                        os.environ["NDPP_SCORE_BAND"] = "0"
                    else:
                        os.environ.pop("NDPP_SCORE_BAND", None)
                    t0 = time.perf_counter()
                    out = ndpp_amd.scatt_score(1, scatt_type, x, y, ein, weight, bins, n_bins)
                    runs[mode].append((time.perf_counter() - t0, ndpp_amd.scatt_score_info()))
                    keep[mode] = out
            os.environ.pop("NDPP_SCORE_BAND", None)
            rec = dict(case=case, scatt_type=scatt_type, n=n, G=G, L=L, events=n_ev, n_bins=n_bins,
                       band_elements=in_band, dense_elements=n_ev * G * L, bytes_band=in_band * 16,
                       scored=int(keep[a.modes[0]][2].sum()))
            if len(keep) == 2:
                rec["band_equals_dense"] = bool(all(p.tobytes() == q.tobytes() for p, q in zip(keep["band"], keep["dense"])))
            for mode, nbytes in (("band", in_band * 16), ("dense", n_ev * G * L * 16)):
                if mode not in runs or not runs[mode]:
                    continue
                best = min(runs[mode], key=lambda r: r[0])
                info = {k: round(v, 3) for k, v in best[1].items()}
                rec[mode] = dict(call_s=round(best[0], 4), call_s_all=[round(r[0], 4) for r in runs[mode]],
                                 kernel_ms_all=[round(r[1]["kernel_ms"], 3) for r in runs[mode]], info=info,
                                 host_share=round((info["bracket_ms"] + info["group_ms"] + info["upload_ms"]) * 1e-3
                                                  / best[0], 3),
                                 events_per_s_call=round(n_ev / best[0]),
                                 events_per_s_kernels=round(n_ev / (info["kernel_ms"] * 1e-3)),
                                 bytes_per_s=round(nbytes / (info["kernel_ms"] * 1e-3)))
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        m = min(a.check_events, n_ev)
        if m and not a.cases:
            t0 = time.perf_counter()
            want = score.score_numpy(1, scatt_type, x, y, ein[:m], weight[:m], (where[:m] * 70).astype(np.int32), 70)
            t = time.perf_counter() - t0
            got = ndpp_amd.scatt_score(1, scatt_type, x, y, ein[:m], weight[:m], (where[:m] * 70).astype(np.int32), 70)
            rec = dict(case=f"{name}_numpy", events=m, numpy_s=round(t, 3), events_per_s_numpy=round(m / t),
                       equal_to_device=bool(all(p.tobytes() == q.tobytes() for p, q in zip(got, want))))
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        del y
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
