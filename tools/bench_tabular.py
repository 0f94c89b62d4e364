"""Measures tabular scattering output next to the Legendre paths on the same inputs: one JSON line
per case, to stdout and to --out.

Cases:
  * headline: bench.py's workload (H-1 free gas, --nein log-spaced E_in to 400 kT, G = 2), the
    Legendre batch at P5 (ndpp_elastic_leg_batch) and the tabular batch at N = --bins
    (ndpp_elastic_tab_batch);
  * u238: the U-238-like nuclide of tests/synth.u238_case (bench.py's secondary workload) through
    ndpp_scatt_nuclide (P7) and ndpp_scatt_nuclide_tab (N = --bins).
Per call: host clock around the synchronising call (warm: one untimed call first), the device time
of the last batch (ndpp_last_gpu_ms; for a whole nuclide the per-family profile), and E_in per
second.  The tabular free-gas rows flagged NDPP_ST_TAB_UNSETTLED are counted.  No GPU: it fails.

    python tools/bench_tabular.py [--nein 100000] [--bins 32] [--skip-u238] [--out FILE]
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


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nein", type=int, default=100000)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--skip-u238", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import ndpp_amd as hip
    from bench import make_workload
    lib = hip.load()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    wl = make_workload(a.nein, 6)
    p = hip.Params.default(6, wl["M"])
    args = (wl["A"], wl["kT"], 1e300, 0.0, wl["ein"], wl["row_lo"], wl["w_hi"], wl["f_tab"], wl["bins"])
    warm = slice(0, 256)
    warm_args = args[:4] + tuple(x[warm] for x in args[4:7]) + args[7:]
    hip.elastic_leg_batch(p, *warm_args)
    hip.elastic_tab_batch(p, a.bins, *warm_args)
    (leg, _), t_leg = timed(lambda: hip.elastic_leg_batch(p, *args))
    ms_leg = float(lib.ndpp_last_gpu_ms())
    (tab, st), t_tab = timed(lambda: hip.elastic_tab_batch(p, a.bins, *args))
    ms_tab = float(lib.ndpp_last_gpu_ms())
    d = np.abs(tab.sum(axis=2) - leg[:, :, 0]).max()
    emit(dict(case="headline", n_ein=a.nein, groups=2, legendre_order=6, bins=a.bins,
              legendre_s=t_leg, legendre_gpu_ms=ms_leg, legendre_ein_per_s=a.nein / t_leg,
              tabular_s=t_tab, tabular_gpu_ms=ms_tab, tabular_ein_per_s=a.nein / t_tab,
              tabular_over_legendre=t_tab / t_leg, sum_rule_max_abs=float(d),
              unsettled_rows=int(((st & hip.lib.ST_TAB_UNSETTLED) != 0).sum())))

    if not a.skip_u238:
        from synth import u238_case
        c = u238_case()
        pu = hip.Params.default(c["order"] + 1, c["mu_bins"])
        pu.extend_pts, pu.inel_extend_pts = c["extend_pts"], c["inel_extend_pts"]
        hip.profile_reset()
        r_leg, t_leg = timed(lambda: hip.scatt_nuclide(pu, c, c["bins"], nuscatt=True))
        prof_leg = hip.profile_get()
        hip.profile_reset()
        r_tab, t_tab = timed(lambda: hip.scatt_nuclide_tab(pu, a.bins, c, c["bins"], nuscatt=True))
        prof_tab = hip.profile_get()
        n = len(r_leg["ein_el"]) + (len(r_leg["ein_inel"]) if r_leg["ein_inel"] is not None else 0)
        emit(dict(case="u238", n_ein=n, groups=len(c["bins"]) - 1, legendre_order=c["order"] + 1, bins=a.bins,
                  legendre_s=t_leg, legendre_ein_per_s=n / t_leg, legendre_profile_ms=prof_leg,
                  tabular_s=t_tab, tabular_ein_per_s=n / t_tab, tabular_profile_ms=prof_tab,
                  tabular_over_legendre=t_tab / t_leg))
    if a.out:
        Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
