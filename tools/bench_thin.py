"""ndpp_thin_segments at G = 70, L = 11, n = 1e5, W = 32 on seeded smooth rows: three calls and one
ndpp_thin_bounded (run it under `rocprofv3 --kernel-trace --stats` for kernel times, alone for call
times); --numpy adds the host restatement on the first 1000 points.  profiles/thin_bounded/README.md."""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import ndpp_amd
n, G, L, W = 100_000, 70, 11, 32
rng = np.random.default_rng(1)
x = 1e-11 * np.exp(np.cumsum(rng.uniform(1e-5, 56.0 / n, n)))
u = np.log(x)[:, None]
y = (np.sin(0.3 * u + rng.uniform(0, 6, (1, G * L))) * rng.uniform(0.1, 1, (1, G * L))).reshape(n, G, L)
y[:, :, 0] = np.abs(y[:, :, 0]) + 0.1
y *= 1.0 + 1e-6 * rng.standard_normal((n, 1, 1))
ndpp_amd.load()
for i in range(3):
    t0 = time.perf_counter()
    seg = ndpp_amd.thin_segments(x, y, None, None, W)
    print(f"call {i}: wall {time.perf_counter() - t0:.3f} s, kernels (events) {ndpp_amd.load().ndpp_last_gpu_ms():.3f} ms, "
          f"finite {np.isfinite(seg).sum()}, -1: {(seg == -1).sum()}", flush=True)
t0 = time.perf_counter()
kept, me = ndpp_amd.thin_bounded(x, y, None, None, 1e-3, W)
print(f"thin_bounded: wall {time.perf_counter() - t0:.3f} s, kept {len(kept)} of {n}, max_err {me:.3e}", flush=True)
if "--numpy" in sys.argv:
    from ndpp_amd import thin
    m = 1000
    t0 = time.perf_counter()
    want = thin.segment_errors_numpy(x[:m], y[:m], None, None, W)
    dt = time.perf_counter() - t0
    got = ndpp_amd.thin_segments(x[:m], y[:m], None, None, W)
    print(f"numpy restatement n={m}: {dt:.2f} s host; bits equal to the device: {np.array_equal(got.view(np.int64), want.view(np.int64))}", flush=True)
