"""Measures library validation on the GPU (ndpp_scatt_positivity, include/ndpp_hip.h): one JSON line
per case, to stdout and to --out.

Cases:
  * random: seeded moments, n_ein x G rows at L = 11 (default 2e6 x 10 = 2e7 rows, 1.76 GB), one
    positivity call per M in --mu (default 21, 201, 2001);
  * library: the synthetic 423-nuclide library of tests/synth.synthetic_library, made once on the GPU
    (ndpp_scatt_library), every section of every nuclide validated (ndpp_amd.validate.positivity) at
    M = 21 and 2001.
Per case: call time (host clock around the synchronising call, warm; includes the upload of the
moments), kernel time (ndpp_last_gpu_ms: the three kernels of a call), flops 2 rows M n_mom and
bytes rows L 8 from the shapes, the bound that applies and its share of peak (FP64 vector 78.6 TF/s,
HBM 8 TB/s), and numpy on the host on a sample of rows as the baseline (per-row time scaled to the
case).  No GPU: it fails, it does not fall back.

    python tools/bench_validate.py [--rows-ein 2000000] [--groups 10] [--mu 21 201 2001]
                                   [--library-size 423] [--out FILE]
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
sys.path.insert(0, str(ROOT / "tests"))

PEAK_FP64 = 78.6e12      # FP64 vector, spec
PEAK_HBM = 8.0e12        # spec


def numpy_rate(mat2d, M, nm, rows=20000):
    """host seconds per row of the same check in numpy (matmul + row min), on a sample"""
    from scipy.special import eval_legendre
    mu = np.linspace(-1, 1, M)
    B = np.array([(l + 0.5) * eval_legendre(l, mu) for l in range(nm)])
    a = mat2d[:rows, :nm]
    t0 = time.perf_counter()
    for k in range(0, len(a), 5000):
        F = a[k:k + 5000] @ B
        (~(F >= 0).all(axis=1)).sum()
        F.min(axis=1)
    return (time.perf_counter() - t0) / len(a)


def case_line(name, rows, M, nm, L, call_s, kernel_ms, host_s_per_row, extra=None):
    flops = 2.0 * rows * M * nm
    byts = rows * L * 8.0
    t_fp, t_mem = flops / PEAK_FP64, byts / PEAK_HBM
    bound = "fp64" if t_fp >= t_mem else "hbm"
    k = kernel_ms * 1e-3
    d = dict(case=name, rows=int(rows), mu_points=M, n_moments=nm, L=L, flops=flops, bytes=byts,
             call_ms=round(call_s * 1e3, 3), kernel_ms=round(kernel_ms, 3),
             bound=bound, bound_ms=round(max(t_fp, t_mem) * 1e3, 4),
             share_of_peak=round(max(t_fp, t_mem) / k, 3) if k > 0 else None,
             fp64_tflops=round(flops / k / 1e12, 2) if k > 0 else None,
             hbm_tbs=round(byts / k / 1e12, 3) if k > 0 else None,
             numpy_s=round(host_s_per_row * rows, 3), numpy_threads=os.cpu_count(),
             speedup_vs_numpy_call=round(host_s_per_row * rows / call_s, 1))
    if extra:
        d.update(extra)
    return d


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-ein", type=int, default=2_000_000)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--mu", type=int, nargs="+", default=[21, 201, 2001])
    ap.add_argument("--repeat", type=int, default=3, help="timed calls per case (the best is reported)")
    ap.add_argument("--library-size", type=int, default=423, help="0: no library case")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    from ndpp_amd import validate
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        raise SystemExit("bench_validate: no HIP device")
    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    # ---- random moments ----
    rng = np.random.default_rng(2026)
    NE, G, L = a.rows_ein, a.groups, 11
    mat = rng.standard_normal((NE, G, L)) * (0.2 / (np.arange(L) + 0.5))
    mat[:, :, 0] = rng.uniform(0.5, 1.5, (NE, G))
    flat = mat.reshape(-1, L)
    for M in a.mu:
        ndpp_amd.scatt_positivity(mat[:1000], mu_points=M)                      # code load, caches
        best, kms, s = np.inf, np.inf, None
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            s, rows, _, _ = ndpp_amd.scatt_positivity(mat, mu_points=M, cap=1000)
            dt = time.perf_counter() - t0
            if dt < best:
                best = dt
            kms = min(kms, float(lib.ndpp_last_gpu_ms()))
        host = numpy_rate(flat, M, L, rows=20000 if M <= 201 else 4000)
        emit(case_line("random", s.rows, M, L, L, best, kms, host,
                       dict(negative=int(s.negative), min_value=s.min_value)))

    # ---- the synthetic library ----
    if a.library_size > 0:
        import synth
        t0 = time.perf_counter()
        libd = synth.synthetic_library(a.library_size, order=5)
        nucs, bins = libd["nuclides"], libd["nuclides"][0]["bins"]
        p = ndpp_amd.Params.default(6, 2001)
        res = ndpp_amd.scatt_library(p, nucs, bins, nuscatt=True)
        made_s = time.perf_counter() - t0
        sections = [m for r in res for m in (r["el_mat"], r["inel_mat"], r["nuinel_mat"]) if m is not None]
        rows_all = sum(m.shape[0] * m.shape[1] for m in sections)
        for M in (21, 2001):
            validate.positivity(res[0], mu_points=M)                            # warm
            best = np.inf
            for _ in range(a.repeat):
                t0, neg, checked = time.perf_counter(), 0, 0
                for r in res:
                    rep = validate.positivity(r, mu_points=M)
                    neg += sum(s.negative for s in rep.sections.values())
                    checked += sum(s.rows for s in rep.sections.values())
                best = min(best, time.perf_counter() - t0)
            # kernel time: the sum of every section call's ndpp_last_gpu_ms
            kms = 0.0
            for m in sections:
                ndpp_amd.scatt_positivity(m, mu_points=M, cap=0)
                kms += float(lib.ndpp_last_gpu_ms())
            host = numpy_rate(np.concatenate([m.reshape(-1, 6) for m in sections[:50]]), M, 6, rows=20000)
            emit(case_line("library", checked, M, 6, 6, best, kms, host,
                           dict(nuclides=len(res), sections=len(sections), dense_rows=int(rows_all),
                                negative=int(neg), library_made_s=round(made_s, 1),
                                note="flops/bytes from the checked (band) rows; calls are per section")))
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
