"""Measures the certified positivity check (ndpp_scatt_minimum, include/ndpp_hip.h) against the sampled
one (ndpp_scatt_positivity at M = 21, 201, 2001) on the same matrix: one JSON line per case, to stdout
and to --out.

The matrix: seeded moments, n_ein x G rows at L = 11 (default 1e5 x 70), P0 in [0.5, 1.5], the higher
moments random and decaying.  Per case: call time (host clock around the synchronising call, warm;
includes the upload of the moments and, for the certified check, the copies back of lo, hi, mu_at and
cls: 28 bytes per row) and kernel time (ndpp_last_gpu_ms: the events around the call's kernels).  For
the certified check also the evaluations of f per row (mean, maximum, and the mean over waves of the
wave's maximum: what a wave of 64 rows in lockstep pays) and the class counts.  Kernel times for a
profile come from running this script under `rocprofv3 --kernel-trace --stats` with --repeat 1.
No GPU: it fails, it does not fall back.

    python tools/bench_minimum.py [--rows-ein 100000] [--groups 70] [--mu 21 201 2001] [--rel-tol 1e-10]
                                  [--out FILE]
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-ein", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=70)
    ap.add_argument("--mu", type=int, nargs="*", default=[21, 201, 2001])
    ap.add_argument("--rel-tol", type=float, default=1e-10)
    ap.add_argument("--repeat", type=int, default=3, help="timed calls per case (the best is reported)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        raise SystemExit("bench_minimum: no HIP device")
    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rng = np.random.default_rng(2026)
    NE, G, L = a.rows_ein, a.groups, 11
    mat = rng.standard_normal((NE, G, L)) * (0.2 / (np.arange(L) + 0.5))
    mat[:, :, 0] = rng.uniform(0.5, 1.5, (NE, G))

    def timed(call):
        best, kms, res = np.inf, np.inf, None
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            res = call()
            best = min(best, time.perf_counter() - t0)
            kms = min(kms, float(lib.ndpp_last_gpu_ms()))
        return best, kms, res

    for M in a.mu:
        ndpp_amd.scatt_positivity(mat[:1000], mu_points=M)                      # code load, caches
        call_s, kms, (s, *_) = timed(lambda: ndpp_amd.scatt_positivity(mat, mu_points=M, cap=1000))
        emit(dict(case="sampled", rows=int(s.rows), mu_points=M, n_moments=L, call_ms=round(call_s * 1e3, 3),
                  kernel_ms=round(kms, 3), negative=int(s.negative), min_value=s.min_value))

    ndpp_amd.scatt_minimum(mat[:1000], rel_tol=a.rel_tol)
    call_s, kms, (s, lo, hi, mu_at, cls) = timed(lambda: ndpp_amd.scatt_minimum(mat, rel_tol=a.rel_tol))
    ev = ndpp_amd.scatt_minimum(mat, rel_tol=a.rel_tol, want_evals=True)[5].ravel()
    # the kernel's rows-to-lanes map: blocks of whole incoming energies, 64 consecutive rows per wave
    epb = max(1, 512 // G)
    per_wave = []
    for e0 in range(0, min(NE, 20000), epb):
        blk = ev[e0 * G:(e0 + epb) * G]
        per_wave += [blk[k:k + 64].max() for k in range(0, len(blk), 64)]
    kind = np.bincount((cls[cls >= 0] & 3).ravel(), minlength=4)
    emit(dict(case="certified", rows=int(s.rows), rel_tol=a.rel_tol, n_moments=L, call_ms=round(call_s * 1e3, 3),
              kernel_ms=round(kms, 3), evals_mean=round(float(ev.mean()), 1), evals_max=int(ev.max()),
              evals_wave_max_mean=round(float(np.mean(per_wave)), 1),
              positive=int(kind[0]), undecided=int(kind[1]), negative=int(kind[2]), nonfinite=int(kind[3]),
              unsettled=int(s.unsettled), min_hi=s.min_hi, min_mu=s.min_mu,
              widest_rel=float(((hi - lo) / np.maximum((np.abs(mat) * (np.arange(L) + 0.5)).sum(axis=2), 1e-300)).max())))
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
