"""Measures sampling from a section (ndpp_scatt_sample, include/ndpp_hip.h): one JSON line per case,
to stdout and to --out.

The section: n incoming energies (default 1e5, log-spaced) x G groups (70) x L entries (11), seeded;
Legendre rows a_l = a_0 exp(-l (l + 1) tau), tau in [0.15, 1] (the family of tests/test_sample.py,
without the positivity redraw: the time does not depend on it), tabular rows uniform bins.  The
events (default 1e7): energies log-uniform over the grid, sorted or not, u_g and u_mu uniform.

Per case (scatt_type x sorted / unsorted), warm (one untimed call of the same shape first):
  call_s        host clock around the synchronising call: brackets, uploads, kernels, downloads
  brackets_s    host clock around ndpp_sample_brackets alone on the same events: the host share
                (one upper_bound and two logarithms per event, one thread)
  kernel_ms     ndpp_last_gpu_ms: device events around the call's kernels (masses + events)
  bytes_*       what the algorithm has to move, from the shapes: the mass kernel reads the section
                once (every line of it, also for P0 at a pitch of L doubles) and writes n G doubles;
                the event kernel reads per event 16 (G + L) bytes of rows and 28 of inputs and writes
                16; uploads and downloads are the section plus 44 bytes per event
  hbm_bound_ms  bytes_kernels over 8 TB/s (the peak; about 6.3 TB/s is achievable), the least the
                kernels could take if every byte came from HBM once
  events_per_s  over call_s, and over kernel_ms
and once, for context, the restatement sample_numpy on --numpy-events of the unsorted events.
Kernel times per kernel come from running this script under `rocprofv3 --kernel-trace --stats` with
--repeat 1.  No GPU: it fails, it does not fall back.

    python tools/bench_sample.py [--rows-ein 100000] [--groups 70] [--entries 11] [--events 10000000]
                                 [--repeat 2] [--numpy-events 200000] [--out FILE]
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

HBM_PEAK = 8.0e12


def section(scatt_type: int, n: int, G: int, L: int, seed: int):
    rng = np.random.default_rng(seed)
    x = np.geomspace(1e-11, 20.0, n)
    if scatt_type == 1:
        return x, rng.random((n, G, L))
    l = np.arange(L)
    a0, tau = rng.uniform(0.0, 2.0, (n, G, 1)), rng.uniform(0.15, 1.0, (n, G, 1))
    return x, a0 * np.exp(-(l * (l + 1))[None, None, :] * tau)


def traffic(n: int, G: int, L: int, n_ev: int) -> dict:
    sec = n * G * L * 8
    mass = sec + n * G * 8
    ev = n_ev * (16 * (G + L) + 28 + 16)
    return dict(bytes_section=sec, bytes_mass_kernel=mass, bytes_event_kernel=ev, bytes_kernels=mass + ev,
                bytes_copies=sec + n_ev * 44)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-ein", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=70)
    ap.add_argument("--entries", type=int, default=11)
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=2, help="timed calls per case (the best is reported)")
    ap.add_argument("--numpy-events", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ndpp_amd
    from ndpp_amd import sample
    lib = ndpp_amd.load()
    if lib.ndpp_device_count() < 1:
        print("bench_sample: no HIP device", file=sys.stderr)
        return 3
    n, G, L, n_ev = a.rows_ein, a.groups, a.entries, a.events
    rng = np.random.default_rng(7)
    ein = np.exp(rng.uniform(np.log(1e-11), np.log(20.0), n_ev))
    u_g, u_mu = rng.random(n_ev), rng.random(n_ev)
    order = np.argsort(ein)
    lines = []
    for scatt_type in (0, 1):
        x, y = section(scatt_type, n, G, L, 11 + scatt_type)
        ein = np.clip(ein, x[0], x[-1])
        for name, ev in (("unsorted", (ein, u_g, u_mu)), ("sorted", (ein[order], u_g[order], u_mu[order]))):
            ndpp_amd.scatt_sample(scatt_type, x, y, *ev)                      # warm: this shape, untimed
            call_s, kernel_ms, brackets_s = [], [], []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                g, mu, st = ndpp_amd.scatt_sample(scatt_type, x, y, *ev)
                call_s.append(time.perf_counter() - t0)
                kernel_ms.append(float(lib.ndpp_last_gpu_ms()))
                t0 = time.perf_counter()
                ndpp_amd.sample_brackets(x, *ev)
                brackets_s.append(time.perf_counter() - t0)
            rec = dict(case=f"{'tabular' if scatt_type else 'legendre'}_{name}", scatt_type=scatt_type, n=n, G=G, L=L,
                       events=n_ev, call_s=round(min(call_s), 4), call_s_all=[round(v, 4) for v in call_s],
                       brackets_s=round(min(brackets_s), 4), kernel_ms=round(min(kernel_ms), 3),
                       kernel_ms_all=[round(v, 3) for v in kernel_ms], **traffic(n, G, L, n_ev))
            rec["host_share_of_call"] = round(rec["brackets_s"] / rec["call_s"], 3)
            rec["hbm_bound_ms"] = round(rec["bytes_kernels"] / HBM_PEAK * 1e3, 3)
            rec["kernel_over_hbm_bound"] = round(rec["kernel_ms"] / rec["hbm_bound_ms"], 2)
            rec["events_per_s_call"] = round(n_ev / rec["call_s"])
            rec["events_per_s_kernels"] = round(n_ev / (rec["kernel_ms"] * 1e-3))
            rec["status_counts"] = {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
            rec["mean_mu"] = float(mu.mean())
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        m = min(a.numpy_events, n_ev)
        t0 = time.perf_counter()
        want = sample.sample_numpy(scatt_type, x, y, ein[:m], u_g[:m], u_mu[:m])
        t = time.perf_counter() - t0
        got = ndpp_amd.scatt_sample(scatt_type, x, y, ein[:m], u_g[:m], u_mu[:m])
        rec = dict(case=f"{'tabular' if scatt_type else 'legendre'}_numpy", events=m, numpy_s=round(t, 3),
                   events_per_s_numpy=round(m / t), equal_to_device=bool(all(np.array_equal(p, q) for p, q in zip(got, want))))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        del y
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
