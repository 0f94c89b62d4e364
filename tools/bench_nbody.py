"""Measures the law-66 integrator (ndpp_nbody_leg_batch, include/ndpp_hip.h): one JSON line per case,
to stdout and to --out.  A first measurement, with nothing to compare against.

Deuterium's (n,2n): awr 1.9968, Q -2.2246 MeV, n = 3 bodies, Ap 2.9986; incoming energies spread
evenly from just above the threshold to 20 MeV.  Two cases:
  library   3000 energies x 70 groups (log-spaced edges up to 20 MeV) x P7 (L = 8)
  small     100 energies x 2 groups ([0, 6.25e-7, 20]) x P7
Per case, warm (one untimed call of the same shape first), --repeat timed calls (default 3):
  kernel_ms   ndpp_last_gpu_ms: device events around the call's kernels
  call_s      host clock around the synchronising call: uploads, kernels, download
  items       (energy, group) pairs; live: those whose group meets the lab window, which integrate
  nodes       inner-rule evaluations of the live items: 32 x 32 per piece
  row_sum     the worst |sum over the groups of P0 - 1|: the edges cover the window
Then the tabular call (ndpp_nbody_tab_batch) next to the Legendre one, on the same 1000 energies x 70
groups: P5 (L = 6), N = 32 and N = 128 bins, one warm call each and then --repeat rounds that alternate
the three (leg, tab32, tab128, leg, ...), so that a drift of the clocks meets all three alike.  Per
call kernel_ms and call_s as above; row_sum is the worst |sum over groups and bins - 1|, min_bin the
smallest bin (never negative), sum_rule the worst |sum of the bins - P0 of the Legendre call|.
No GPU: it fails, it does not fall back.

    python tools/bench_nbody.py [--repeat 3] [--out FILE]
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

AWR, Q, N_BODIES, AP = 1.9968, -2.2246, 3, 2.9986


def work(ein, bins):
    """(live items, pieces of the live items) by the definition's window and breakpoint rules"""
    Emax = ((AP - 1.0) / AP) * ((AWR / (AWR + 1.0)) * ein + Q)
    rE0, rEm = np.sqrt(ein / ((AWR + 1.0) * (AWR + 1.0)))[:, None], np.sqrt(Emax)[:, None]
    lo, hi = bins[None, :-1], bins[None, 1:]
    wl = np.maximum(rE0 - rEm, 0.0)
    live = (hi > wl * wl) & (lo < (rEm + rE0) ** 2)
    pieces = np.ones(live.shape, dtype=np.int64)
    for edge, sign in ((lo, -1.0), (lo, 1.0), (hi, -1.0), (hi, 1.0)):
        Tb = (np.sqrt(edge) + sign * rE0) ** 2
        pieces += (Tb > 0.0) & (Tb < Emax[:, None])
    return int(live.sum()), int(pieces[live].sum())                  # (duplicates counted: an upper bound)


def tabular(ndpp_amd, lib, thr, repeat) -> list:
    """the tabular call at N = 32 and 128 next to the Legendre call at P5: alternating rounds"""
    n_ein, bins = 1000, np.concatenate([[0.0], np.geomspace(1e-11, 20.0, 70)])
    ein = np.linspace(thr * 1.001, 20.0, n_ein)
    p = ndpp_amd.Params.default(6, 65)
    calls = [("leg_P5", lambda: ndpp_amd.nbody_leg_batch(p, AWR, Q, N_BODIES, AP, ein, bins)),
             ("tab_N32", lambda: ndpp_amd.nbody_tab_batch(p, 32, AWR, Q, N_BODIES, AP, ein, bins)),
             ("tab_N128", lambda: ndpp_amd.nbody_tab_batch(p, 128, AWR, Q, N_BODIES, AP, ein, bins))]
    out, call_s, kernel_ms = {}, {k: [] for k, _ in calls}, {k: [] for k, _ in calls}
    for _, f in calls:
        f()                                                             # warm: this shape, untimed
    for _ in range(repeat):
        for name, f in calls:
            t0 = time.perf_counter()
            out[name], st = f()
            call_s[name].append(time.perf_counter() - t0)
            kernel_ms[name].append(float(lib.ndpp_last_gpu_ms()))
            assert not st.any()
    p0 = out["leg_P5"][:, :, 0]
    lines = []
    for name, _ in calls:
        o = out[name]
        rec = dict(case=name, n_ein=n_ein, G=len(bins) - 1, L=o.shape[2], elements=int(o.size),
                   kernel_ms=round(min(kernel_ms[name]), 3), kernel_ms_all=[round(v, 3) for v in kernel_ms[name]],
                   call_s=round(min(call_s[name]), 5), call_s_all=[round(v, 5) for v in call_s[name]])
        if name == "leg_P5":
            rec["row_sum"] = float(np.abs(p0.sum(axis=1) - 1.0).max())
        else:
            rec.update(row_sum=float(np.abs(o.sum(axis=(1, 2)) - 1.0).max()), min_bin=float(o.min()),
                       sum_rule=float(np.abs(o.sum(axis=2) - p0).max()))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        print("bench_nbody: no HIP device", file=sys.stderr)
        return 3
    thr = -Q * (AWR + 1.0) / AWR
    cases = [("library", 3000, np.concatenate([[0.0], np.geomspace(1e-11, 20.0, 70)])),
             ("small", 100, np.array([0.0, 6.25e-7, 20.0]))]
    lines = []
    for name, n_ein, bins in cases:
        ein = np.linspace(thr * 1.001, 20.0, n_ein)
        p = ndpp_amd.Params.default(8, 65)
        ndpp_amd.nbody_leg_batch(p, AWR, Q, N_BODIES, AP, ein, bins)           # warm: this shape, untimed
        call_s, kernel_ms = [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            out, st = ndpp_amd.nbody_leg_batch(p, AWR, Q, N_BODIES, AP, ein, bins)
            call_s.append(time.perf_counter() - t0)
            kernel_ms.append(float(lib.ndpp_last_gpu_ms()))
        live, pieces = work(ein, bins)
        rec = dict(case=name, n_ein=n_ein, G=len(bins) - 1, L=8, items=n_ein * (len(bins) - 1), live=live,
                   nodes=pieces * 32 * 32, kernel_ms=round(min(kernel_ms), 3),
                   kernel_ms_all=[round(v, 3) for v in kernel_ms], call_s=round(min(call_s), 5),
                   call_s_all=[round(v, 5) for v in call_s],
                   row_sum=float(np.abs(out[:, :, 0].sum(axis=1) - 1.0).max()), status_any=bool(st.any()))
        rec["nodes_per_s"] = round(rec["nodes"] / (rec["kernel_ms"] * 1e-3)) if rec["kernel_ms"] > 0 else None
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    lines += tabular(ndpp_amd, lib, thr, a.repeat)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
