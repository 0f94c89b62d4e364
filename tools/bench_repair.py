"""Measures the repair of negative rows (ndpp_scatt_repair, include/ndpp_hip.h) against its model: one
JSON line per case, to stdout and to --out.

The matrix is that of tools/bench_minimum.py: seeded moments, n_ein x G rows at L = 11 (default
1e5 x 70), P0 in [0.5, 1.5], the higher moments random and decaying; 52.5 % of the rows are negative.
The model: every repaired row runs 2 * steps certified searches in mode best (steps in heat or uniform),
so the repair kernel should cost what ndpp_scatt_minimum's kernel costs per row (timed here, on the
same matrix) times the searches times the rows repaired, and a repaired row should make the mean
evaluations of f of an examined row times the searches.  Per mode: kernel time (ndpp_last_gpu_ms: the
events around the repair kernel alone), call time (host clock around the synchronising call, warm),
the ratio of both to the model, evaluations of f per repaired row (mean, maximum, and the mean over
waves of the wave's maximum: the kernel takes 64 consecutive listed rows per wave), the family counts
and the quantiles of t.  Kernel times for a profile come from running this script under
`rocprofv3 --kernel-trace --stats` with --repeat 1.

--library: the 32-nuclide miniature library (LIBRARY_SMALL of tests/golden/make_golden.py, P5) through
scatt_library, then ndpp_amd.repair.repair_sections on every table: the distribution of t and of the
family chosen, per section kind.  No GPU: it fails, it does not fall back.

    python tools/bench_repair.py [--rows-ein 100000] [--groups 70] [--steps 20] [--rel-tol 1e-10]
                                 [--modes best heat uniform] [--library] [--out FILE]
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

QUANTILES = (0.0, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0)


def t_summary(t, how) -> dict:
    """family counts and the quantiles of t over the repaired rows"""
    rep = (how == 1) | (how == 2)
    d = dict(repaired=int(rep.sum()), heat=int((how == 1).sum()), uniform=int((how == 2).sum()))
    if rep.any():
        d["t_quantiles"] = {f"{q:g}": round(float(v), 6) for q, v in zip(QUANTILES, np.quantile(t[rep], QUANTILES))}
        d["t_mean"] = round(float(t[rep].mean()), 6)
    return d


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-ein", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=70)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rel-tol", type=float, default=1e-10)
    ap.add_argument("--modes", nargs="*", default=["best", "heat", "uniform"])
    ap.add_argument("--repeat", type=int, default=2, help="timed calls per case (the best is reported)")
    ap.add_argument("--library", action="store_true", help="also the 32-nuclide miniature library at P5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    from ndpp_amd import repair
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        raise SystemExit("bench_repair: no HIP device")
    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if a.rows_ein > 0:
        rng = np.random.default_rng(2026)
        NE, G, L = a.rows_ein, a.groups, 11
        mat = rng.standard_normal((NE, G, L)) * (0.2 / (np.arange(L) + 0.5))
        mat[:, :, 0] = rng.uniform(0.5, 1.5, (NE, G))

        # the yardstick: the certified check on the same matrix
        ndpp_amd.scatt_minimum(mat[:1000], rel_tol=a.rel_tol)
        min_ms = np.inf
        for _ in range(a.repeat):
            s0, _, _, _, cls = ndpp_amd.scatt_minimum(mat, rel_tol=a.rel_tol)
            min_ms = min(min_ms, float(lib.ndpp_last_gpu_ms()))
        ev0 = ndpp_amd.scatt_minimum(mat, rel_tol=a.rel_tol, want_evals=True)[5]
        emit(dict(case="certified", rows=int(s0.rows), negative=int(s0.negative), kernel_ms=round(min_ms, 3),
                  evals_mean=round(float(ev0.mean()), 1), evals_mean_negative=round(float(ev0[(cls & 3) == 2].mean()), 1)))

        for mode in a.modes:
            searches = (2 if mode == "best" else 1) * a.steps
            ndpp_amd.scatt_repair(mat[:1000], mode=repair.MODES[mode], steps=a.steps, rel_tol=a.rel_tol)
            call_s, kms = np.inf, np.inf
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                s, _, t, how = ndpp_amd.scatt_repair(mat, mode=repair.MODES[mode], steps=a.steps, rel_tol=a.rel_tol)
                call_s = min(call_s, time.perf_counter() - t0)
                kms = min(kms, float(lib.ndpp_last_gpu_ms()))
            ev = ndpp_amd.scatt_repair(mat, mode=repair.MODES[mode], steps=a.steps, rel_tol=a.rel_tol, want_evals=True)[4]
            rep = (how == 1) | (how == 2)
            listed = ev[rep]                                  # (iE, g) order: the order of the kernel's list
            per_wave = [listed[k:k + 64].max() for k in range(0, min(len(listed), 1 << 20), 64)]
            model_ms = min_ms * searches * s.repaired / s0.rows
            model_evals = float(ev0.mean()) * searches
            emit(dict(case="repair", mode=mode, steps=a.steps, rel_tol=a.rel_tol, rows=int(s.rows),
                      unrepairable=int(s.unrepairable), nonfinite=int(s.nonfinite), kernel_ms=round(kms, 3),
                      call_ms=round(call_s * 1e3, 3), model_ms=round(model_ms, 3), kernel_over_model=round(kms / model_ms, 4),
                      evals_mean=round(float(listed.mean()), 1), evals_max=int(listed.max()),
                      evals_wave_max_mean=round(float(np.mean(per_wave)), 1), model_evals=round(model_evals, 1),
                      evals_over_model=round(float(listed.mean()) / model_evals, 4),
                      min_t=float(s.min_t), **t_summary(t, how)))
        del mat

    if a.library:
        sys.path.insert(0, str(ROOT / "tests"))
        sys.path.insert(0, str(ROOT / "tests" / "golden"))
        import synth
        from make_golden import LIBRARY_SMALL
        libd = synth.synthetic_library(**LIBRARY_SMALL)
        nucs, bins = libd["nuclides"], libd["nuclides"][0]["bins"]
        p = ndpp_amd.Params.default(nucs[0]["order"] + 1, nucs[0]["mu_bins"])
        p.extend_pts, p.inel_extend_pts = nucs[0]["extend_pts"], nucs[0]["inel_extend_pts"]
        res = ndpp_amd.scatt_library(p, nucs, bins, nuscatt=True)
        t0 = time.perf_counter()
        acc, change = {}, {}
        for r in res:
            secs, rr = repair.repair_sections(r, steps=a.steps, rel_tol=a.rel_tol)
            for name, v in secs.items():
                acc.setdefault(name, []).append((v["t"].ravel(), v["how"].ravel()))
                change[name] = max(change.get(name, 0.0), rr.sections[name].max_change)
        wall = time.perf_counter() - t0
        for name, parts in acc.items():
            t, how = np.concatenate([x for x, _ in parts]), np.concatenate([y for _, y in parts])
            emit(dict(case="library", section=name, tables=len(parts), order=nucs[0]["order"], steps=a.steps,
                      rows=int((how >= 0).sum()), unrepairable=int((how == 3).sum()), nonfinite=int((how == 4).sum()),
                      max_change=change[name], wall_s_all_sections=round(wall, 3), **t_summary(t, how)))
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
