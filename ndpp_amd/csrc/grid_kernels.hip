// grid_kernels.hip -- what interpolating between two neighbours of an incoming-energy grid costs:
// the error of the interpolated row against a freshly integrated row at a point between them.
// Nothing in the reference does this (thin_grid, thin.F90, compares stored rows with each other);
// the interpolation rule is the one thin_grid assumes, linear in ln E (lne_weight, section_util.h):
//   f      = ln(x_mid / x_i) / ln(x_{i+1} / x_i)
//   d(g,l) = | y_i + (y_{i+1} - y_i) f - y_mid |
//   err_i  = the scale-relative metric of section_util.h over d, the scale from the three rows
//
// f is computed on the host, once per interval, and uploaded: the kernel is + - * / fabs and
// comparisons only, built without contraction, so a host restatement with the same operation
// order gives the same bits (ndpp_amd/gridcheck.py: grid_error_numpy).
//
// One wave64 per interval, the grid strides over intervals.  The three rows are G*L contiguous
// doubles each; the lanes stride over them (coalesced loads) and fold their maxima as WaveMax
// (section_util.h) says; lane 0 writes the two results.  No LDS, no atomics.
// Memory-bound: 3 * G * L * 8 bytes per interval.
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "section_util.h"

namespace ndpp {
namespace {

constexpr int kThreads = 256;          // 4 waves = 4 intervals per block and pass

__global__ void __launch_bounds__(kThreads)
grid_error_kernel(int n_int, int GL, int L, const double* __restrict__ y, const double* __restrict__ y_mid,
                  const double* __restrict__ f, double* __restrict__ err, int* __restrict__ arg) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long n_waves = ((long)gridDim.x * blockDim.x) >> 6;
  for (long i = wave; i < n_int; i += n_waves) {          // wave-uniform trip count
    const double fi = f[i];
    if (fi < 0.0) {                                       // skipped interval (marked by the host)
      if (lane == 0) { err[i] = -1.0; arg[i] = -1; }
      continue;
    }
    const double* a = y + (size_t)i * GL;
    const double* b = a + GL;
    const double* m = y_mid + (size_t)i * GL;
    WaveMax w;
    for (int e = lane; e < GL; e += 64) {
      const double ya = a[e], yb = b[e], ym = m[e];
      w.take(e, fabs(ya + (yb - ya) * fi - ym));
      if (e % L == 0) w.scale = fmax(w.scale, fmax(fabs(ya), fmax(fabs(yb), fabs(ym))));
    }
    w.fold();
    if (lane == 0) w.write(&err[i], &arg[i]);
  }
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_grid_error(int L, int G, int n, const double* x, const double* y, const double* x_mid,
                               const double* y_mid, double* err, int* arg) {
  if (L < 1 || G < 1 || n < 2) return fail(NDPP_EINVAL, "grid_error: L=%d G=%d n=%d (need L, G >= 1, n >= 2)", L, G, n);
  if (!x || !y || !x_mid || !y_mid || !err || !arg) return fail(NDPP_EINVAL, "grid_error: NULL argument");
  if (int rc = check_gl_index("grid_error", G, L)) return rc;
  const int GL = G * L, n_int = n - 1;
  if (int rc = require_device()) return rc;

  // f per interval; -1 marks the intervals that are skipped: abscissae that are not positive and
  // finite, x[i+1] <= x[i], or x_mid outside (x[i], x[i+1])
  std::vector<double> f((size_t)n_int);
  for (int i = 0; i < n_int; ++i) {
    const double x0 = x[i], x1 = x[i + 1], xm = x_mid[i];
    const bool ok = std::isfinite(x0) && std::isfinite(x1) && x0 > 0.0 && x1 > x0 && xm > x0 && xm < x1;
    f[i] = ok ? lne_weight(x0, x1, xm) : -1.0;
  }
  DevBuf<double> d_y, d_mid, d_f, d_err;
  DevBuf<int> d_arg;
  NDPP_TRY(d_y.upload(y, (size_t)n * GL));
  NDPP_TRY(d_mid.upload(y_mid, (size_t)n_int * GL));
  NDPP_TRY(d_f.upload(f.data(), f.size()));
  NDPP_TRY(d_err.alloc(n_int));
  NDPP_TRY(d_arg.alloc(n_int));
  {
    GpuSpan span(nullptr, -1);
    hipLaunchKernelGGL(grid_error_kernel, dim3(nblk((long)n_int * 64, kThreads)), dim3(kThreads), 0, 0, n_int, GL, L,
                       d_y.p, d_mid.p, d_f.p, d_err.p, d_arg.p);
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(hipMemcpy(err, d_err.p, sizeof(double) * n_int, hipMemcpyDeviceToHost));
  NDPP_TRY(hipMemcpy(arg, d_arg.p, sizeof(int) * n_int, hipMemcpyDeviceToHost));
  return NDPP_OK;
}
