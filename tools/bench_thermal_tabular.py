"""Measures the tabular output of a thermal table (ndpp_sab_tab_batch, include/ndpp_hip.h) next to
the Legendre path on the same grid: one JSON line per case, to stdout and to --out.

The table is the config-4b table of tests/test_sab.py: continuous mode, 116 incoming energies,
50 .. 300 outgoing energies each (seed 1002), NMU = 20, on the grid sab_egrid builds for it plus the
extra top point; --groups 2 or 70 as there.  With --discrete also the hh2o-like skewed table of that
file (116 x 64 x 16).  Per N: the device time of ndpp_sab_tab_batch (ndpp_last_gpu_ms: the events
around its kernels, the best of --repeat warm calls), the call time (host clock around the
synchronising call), the same two for ndpp_sab_batch at L = 11, the ratio of the device times, and
the worst bin against the numpy restatement tests/thermal_tab_ref.py relative to the E_in's largest
group P0, with the bar 4 n 2^-53 it is held to in the tests.  Kernel times for a profile come from
running this script under `rocprofv3 --kernel-trace --stats` with --repeat 1.  No GPU: it fails, it
does not fall back.

    python tools/bench_thermal_tabular.py [--bins 32 128] [--groups 70] [--discrete] [--repeat 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(lib, call, repeat):
    """best device time (ms) and best call time (ms) of `repeat` warm calls, and the last result"""
    call()
    dev, wall, res = np.inf, np.inf, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        res = call()
        wall = min(wall, time.perf_counter() - t0)
        dev = min(dev, float(lib.ndpp_last_gpu_ms()))
    return dev, wall * 1e3, res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--groups", type=int, default=70, choices=(2, 70))
    ap.add_argument("--discrete", action="store_true", help="also the skewed discrete table (116 x 64 x 16)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    import thermal_tab_ref as ref
    from synth import sab_table
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        raise SystemExit("bench_thermal_tabular: no HIP device")
    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    bins = np.array([0.0, 6.25e-7, 20.0]) if a.groups == 2 else \
        np.concatenate([[0.0], np.logspace(-11, np.log10(20.0), 70)])
    cases = [("continuous 116 x [50, 300] x 20", sab_table(2, seed=1002, NEi=116, NMU=20, NEo_range=(50, 300)))]
    if a.discrete:
        cases.append(("skewed 116 x 64 x 16", sab_table(1, seed=1001, NEi=116, NEo=64, NMU=16)))
    for label, t in cases:
        ein = ndpp_amd.add_one_more_point(ndpp_amd.sab_egrid(t, bins))
        flat = ndpp_amd.SabFlat.from_dict(t)
        p11 = ndpp_amd.Params.default(11, 2001)
        leg_dev, leg_wall, leg = timed(lib, lambda: ndpp_amd.sab_batch(p11, flat, ein, bins), a.repeat)
        emit(dict(case="legendre", table=label, groups=a.groups, n_ein=len(ein), L=11, device_ms=round(leg_dev, 4),
                  call_ms=round(leg_wall, 3)))
        n_in, _ = ref.masses_per_bin(t)
        for N in a.bins:
            dev, wall, got = timed(lib, lambda: ndpp_amd.sab_tab_batch(p11, N, flat, ein, bins, want_parts=True,
                                                                       want_status=True), a.repeat)
            mat, el, inel, status = got
            rmat, rel, rinel, rstatus = ref.sab_tab(t, ein, bins, N)
            worst = {}
            for name, g, r in (("scatt_mat", mat, rmat), ("inel", inel, rinel)):
                p0 = r.sum(axis=2)
                scale = np.abs(p0).max(axis=1)
                scale[scale == 0] = 1.0
                worst[name] = float((np.abs(g - r) / scale[:, None, None]).max())
            p0_err = float(np.abs(mat.sum(axis=2) - leg[:, :, 0]).max())
            emit(dict(case="tabular", table=label, groups=a.groups, n_ein=len(ein), N=N, device_ms=round(dev, 4),
                      call_ms=round(wall, 3), device_over_legendre=round(dev / leg_dev, 3),
                      worst_bin_vs_restatement=worst, bar=4 * n_in * 2.0 ** -53, masses_per_bin=n_in,
                      zero_pattern_equal=bool(np.array_equal(mat == 0, rmat == 0)),
                      status_equal=bool(np.array_equal(status, rstatus)), status_any=bool(status.any()),
                      max_abs_bin_sum_minus_p0=p0_err, negative_bins=int((mat < 0).sum())))
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
