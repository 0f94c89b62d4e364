// compare_kernels.hip -- how far two libraries are apart (include/ndpp_hip.h):
// the rows a consumer interpolates from section A and from section B at the same energy, under the
// scale-relative metric of section_util.h.  Nothing in the reference does this.  Both sections are
// read linearly in ln E (lne_weight, section_util.h):
//   A(x)   = ya[i] + (ya[i1] - ya[i]) fa      i the largest index with xa[i] <= x, i1 = min(i+1, na-1)
//   B(x)   = yb[j] + (yb[j1] - yb[j]) fb
//   d(g,l) = | A(x) - B(x) |                  g < G, l < Lc = min(La, Lb)
//   err    = the metric over d, the scale from the four rows
//   worst[g][l] = max over the queries of rel_err(d(g,l), scale)
//
// i, fa, j, fb are computed on the host, once per query, and uploaded: the kernels are + - * / fabs
// and comparisons only, built without contraction, so a host restatement with the same operation
// order gives the same bits (ndpp_amd/compare.py: compare_numpy).
//
// compare_error_kernel: one wave64 per query, the grid strides over queries.  The four rows are
// G*La or G*Lb contiguous doubles each; the lanes stride over the G*Lc compared elements (with
// La == Lb these are the whole rows, coalesced; otherwise runs of Lc doubles at pitch La or Lb)
// and fold their maxima as WaveMax (section_util.h) says; lane 0 writes err, arg and the scale.
// No LDS, no atomics.  Memory-bound: (2 La + 2 Lb) * G * 8 bytes per query.
//
// worst needs a maximum across queries per element.  The first kernel cannot keep it: a lane owns
// ceil(G*Lc / 64) elements, a number without a bound, and d / scale needs the scale the wave only
// has after its butterfly.  So a second kernel turns the layout round: a lane owns ONE element for
// its whole life (its offsets into the rows are computed once), a wave owns 64 consecutive elements
// and a contiguous chunk of the queries, and walks it with the scale the first kernel left.  Sorted
// queries that follow each other share their rows, so within a chunk the rows come from the cache;
// waves on different element tiles read disjoint parts of a row.  Every wave writes one partial
// maximum per element, a third kernel folds the chunks (coalesced over the elements).  The maxima
// are over exact values, so the chunking reaches no bit.  Storing d / scale per query and element
// from the first kernel instead would write as many bytes as the rows hold; floating-point atomics
// are not used anywhere.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "section_util.h"

namespace ndpp {
namespace {

constexpr int kThreads = 256;          // 4 waves = 4 queries (or 4 query chunks) per block and pass
constexpr int kWorstWaves = 4096;      // waves of the worst pass: 256 CUs x 16

__global__ void __launch_bounds__(kThreads)
compare_error_kernel(int nq, int G, int La, int Lb, int Lc, int na, int nb, const double* __restrict__ ya,
                     const double* __restrict__ yb, const int* __restrict__ ia, const double* __restrict__ fa,
                     const int* __restrict__ ib, const double* __restrict__ fb, double* __restrict__ err,
                     int* __restrict__ arg, double* __restrict__ scale_out) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long n_waves = ((long)gridDim.x * blockDim.x) >> 6;
  const int GLc = G * Lc;
  const size_t pa = (size_t)G * La, pb = (size_t)G * Lb;
  const int g0 = lane / Lc, l0 = lane - g0 * Lc;         // the lane's first element, and its step of 64
  const int dg = 64 / Lc, dl = 64 - dg * Lc;
  for (long q = wave; q < nq; q += n_waves) {            // wave-uniform trip count
    const int i = ia[q];
    if (i < 0) {                                         // skipped query (marked by the host)
      if (lane == 0) { err[q] = -1.0; arg[q] = -1; scale_out[q] = 0.0; }
      continue;
    }
    const int j = ib[q];
    const double fqa = fa[q], fqb = fb[q];
    const double* a0 = ya + (size_t)i * pa;
    const double* a1 = ya + (size_t)min(i + 1, na - 1) * pa;
    const double* b0 = yb + (size_t)j * pb;
    const double* b1 = yb + (size_t)min(j + 1, nb - 1) * pb;
    WaveMax w;
    int g = g0, l = l0;
    for (int e = lane; e < GLc; e += 64) {
      const int oa = g * La + l, ob = g * Lb + l;
      const double va0 = a0[oa], va1 = a1[oa], vb0 = b0[ob], vb1 = b1[ob];
      w.take(e, fabs((va0 + (va1 - va0) * fqa) - (vb0 + (vb1 - vb0) * fqb)));
      if (l == 0) w.scale = fmax(w.scale, fmax(fmax(fabs(va0), fabs(va1)), fmax(fabs(vb0), fabs(vb1))));
      g += dg;
      l += dl;
      if (l >= Lc) { l -= Lc; ++g; }
    }
    w.fold();
    if (lane == 0) {
      w.write(&err[q], &arg[q]);
      scale_out[q] = w.scale;
    }
  }
}

// part[c][e]: the maximum of d(e) / scale over the queries of chunk c (per queries each), -1 if it holds
// none that was not skipped.  blockIdx.x: the tile of 64 elements; blockIdx.y * 4 + wave: the chunk.
__global__ void __launch_bounds__(kThreads)
compare_worst_kernel(int nq, int per, int G, int La, int Lb, int Lc, int na, int nb,
                     const double* __restrict__ ya, const double* __restrict__ yb, const int* __restrict__ ia,
                     const double* __restrict__ fa, const int* __restrict__ ib, const double* __restrict__ fb,
                     const double* __restrict__ scale, double* __restrict__ part) {
  const int GLc = G * Lc;
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const long c = (long)blockIdx.y * (kThreads / 64) + (threadIdx.x >> 6);
  if (e >= GLc) return;
  const int g = e / Lc, l = e - g * Lc;
  const size_t pa = (size_t)G * La, pb = (size_t)G * Lb;
  const double* pya = ya + (g * La + l);
  const double* pyb = yb + (g * Lb + l);
  const long q0 = c * per, q1 = q0 + per < nq ? q0 + per : nq;
  double w = -1.0;
  for (long q = q0; q < q1; ++q) {
    const int i = ia[q];
    if (i < 0) continue;
    const int j = ib[q];
    const double va0 = pya[(size_t)i * pa], va1 = pya[(size_t)min(i + 1, na - 1) * pa];
    const double vb0 = pyb[(size_t)j * pb], vb1 = pyb[(size_t)min(j + 1, nb - 1) * pb];
    const double d = fabs((va0 + (va1 - va0) * fa[q]) - (vb0 + (vb1 - vb0) * fb[q]));
    const double v = rel_err(d, scale[q]);
    w = v > w ? v : w;
  }
  part[(size_t)c * GLc + e] = w;
}

__global__ void __launch_bounds__(kThreads)
compare_fold_kernel(int GLc, int n_chunks, const double* __restrict__ part, double* __restrict__ worst) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= GLc) return;
  double w = part[e];
  for (int c = 1; c < n_chunks; ++c) {
    const double v = part[(size_t)c * GLc + e];
    w = v > w ? v : w;
  }
  worst[e] = w;
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_lib_compare(int G, int La, int Lb, int na, const double* xa, const double* ya, int nb,
                                const double* xb, const double* yb, int nq, const double* xq, double* err,
                                int* arg, double* worst) {
  if (G < 1 || La < 1 || Lb < 1)
    return fail(NDPP_EINVAL, "lib_compare: G=%d La=%d Lb=%d (need G, La, Lb >= 1)", G, La, Lb);
  if (na < 2 || nb < 2) return fail(NDPP_EINVAL, "lib_compare: na=%d nb=%d (need na, nb >= 2)", na, nb);
  if (nq < 1) return fail(NDPP_EINVAL, "lib_compare: nq=%d (need nq >= 1)", nq);
  if (!xa || !ya || !xb || !yb || !xq || !err || !arg)
    return fail(NDPP_EINVAL, "lib_compare: NULL argument (only worst may be NULL)");
  const int Lmax = std::max(La, Lb), Lc = std::min(La, Lb);
  int rc = check_gl_index("lib_compare", G, Lmax);
  if (rc != NDPP_OK) return rc;
  if ((rc = check_energy_grid("lib_compare", "xa", na, xa))) return rc;
  if ((rc = check_energy_grid("lib_compare", "xb", nb, xb))) return rc;
  if ((rc = require_device("lib_compare"))) return rc;

  // rows and weights per query; row -1 marks the queries that are skipped: not positive and finite, or
  // outside the range of either grid
  std::vector<int> ia((size_t)nq), ib((size_t)nq);
  std::vector<double> fa((size_t)nq), fb((size_t)nq);
  for (int q = 0; q < nq; ++q) {
    const double v = xq[q];
    const bool ok = std::isfinite(v) && v > 0.0 && v >= xa[0] && v <= xa[na - 1] && v >= xb[0] && v <= xb[nb - 1];
    if (!ok) {
      ia[q] = ib[q] = -1;
      fa[q] = fb[q] = 0.0;
      continue;
    }
    bracket(na, xa, v, &ia[q], &fa[q]);
    bracket(nb, xb, v, &ib[q], &fb[q]);
  }
  const int GLc = G * Lc;
  const int tiles = (GLc + 63) / 64;
  // chunks of the worst pass: enough waves to fill the device, a multiple of the waves of a block
  const int per_block = kThreads / 64;
  int chunks = std::max(1, std::min(nq, kWorstWaves / tiles));
  const int per = (nq + chunks - 1) / chunks;
  chunks = ((nq + per - 1) / per + per_block - 1) / per_block * per_block;

  DevBuf<double> d_ya, d_yb, d_fa, d_fb, d_err, d_scale, d_part, d_worst;
  DevBuf<int> d_ia, d_ib, d_arg;
  NDPP_TRY(d_ya.upload(ya, (size_t)na * G * La));
  NDPP_TRY(d_yb.upload(yb, (size_t)nb * G * Lb));
  NDPP_TRY(d_ia.upload(ia.data(), ia.size()));
  NDPP_TRY(d_ib.upload(ib.data(), ib.size()));
  NDPP_TRY(d_fa.upload(fa.data(), fa.size()));
  NDPP_TRY(d_fb.upload(fb.data(), fb.size()));
  NDPP_TRY(d_err.alloc(nq));
  NDPP_TRY(d_arg.alloc(nq));
  NDPP_TRY(d_scale.alloc(nq));
  if (worst) {
    NDPP_TRY(d_part.alloc((size_t)chunks * GLc));
    NDPP_TRY(d_worst.alloc(GLc));
  }
  {
    GpuSpan span(nullptr, -1);
    hipLaunchKernelGGL(compare_error_kernel, dim3(nblk((long)nq * 64, kThreads)), dim3(kThreads), 0, 0, nq, G, La, Lb,
                       Lc, na, nb, d_ya.p, d_yb.p, d_ia.p, d_fa.p, d_ib.p, d_fb.p, d_err.p, d_arg.p, d_scale.p);
    NDPP_TRY(hipGetLastError());
    if (worst) {
      hipLaunchKernelGGL(compare_worst_kernel, dim3(tiles, chunks / per_block), dim3(kThreads), 0, 0, nq, per, G, La,
                         Lb, Lc, na, nb, d_ya.p, d_yb.p, d_ia.p, d_fa.p, d_ib.p, d_fb.p, d_scale.p, d_part.p);
      NDPP_TRY(hipGetLastError());
      hipLaunchKernelGGL(compare_fold_kernel, dim3(nblk(GLc, kThreads)), dim3(kThreads), 0, 0, GLc, chunks, d_part.p,
                         d_worst.p);
    }
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(d_err.download(err, nq));
  NDPP_TRY(d_arg.download(arg, nq));
  if (worst) NDPP_TRY(d_worst.download(worst, GLc));
  return NDPP_OK;
}
