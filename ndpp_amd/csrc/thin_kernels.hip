// thin_kernels.hip -- error-bounded thinning of an incoming-energy grid (include/ndpp_hip.h,
// DESIGN.md section 13).  For every anchor a and every partner b = a + d within the window, the
// error of every point k strictly between them against the interpolation between rows a and b,
// linear in ln E, under the scale-relative metric of section_util.h:
//   f          = (lx[k] - lx[a]) / (lx[b] - lx[a])
//   d(a,k,b)   = max_e | y[a][e] + (y[b][e] - y[a][e]) f - y[k][e] |
//   err(a,k,b) = rel_err(d, max(s[a], s[k], s[b]))
//   seg_err[a][d-2] = max_k err(a, k, a+d)
// lx and s come from the host; the device runs + - * / fabs and comparisons only, in that order,
// built without contraction, so a host restatement gives the same bits (ndpp_amd/thin.py).  The
// maxima are over exact values and return no argument: any lane layout gives the same bits.
//
// Layout.  The work item is (anchor, d, chunk of kChunk consecutive k): one thread, which reads
// y[a][e] and y[b][e] once per element for its kChunk points and keeps one running maximum per
// point in registers.  A block of kThreads items covers A consecutive anchors (as many as fill
// it); their rows a0 .. a0 + A - 1 + W are staged through the LDS one tile of kTile elements at a
// time (65 rows of 770 doubles do not fit), so a row read from memory serves every triple of the
// block it takes part in.  The row pitch is odd in doubles: lanes on different rows hit
// different banks.  A chunk past the end of its segment repeats the segment's last point, so the
// inner loop has no predicate and every LDS row it touches was loaded.  Each item writes one
// partial maximum; a second kernel folds the chunks of a segment and marks the segments that end
// beyond the grid.  No atomics, no scratch.
//
// Values that are not finite.  A NaN or an infinity in row a, k or b makes d(a,k,b) a NaN or an
// infinity at that element, whatever the other values are (f lies strictly inside (0, 1)), and finite
// rows can only overflow to +inf, which a running maximum keeps.  So the host flags the rows that
// hold such a value, once, and the inner loop carries no test: err is +inf when one of the three
// rows is flagged or the maximum is not finite.
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "section_util.h"

namespace ndpp {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                 // elements per LDS tile
constexpr int kPitch = kTile + 1;         // doubles per LDS row
constexpr int kChunk = 8;                 // points k per work item
constexpr int kMaxWindow = 64;
constexpr int kMaxAnchors = 32;           // anchors per block at most
constexpr int kMaxRows = kMaxWindow + 1;  // LDS rows: A + W never exceeds it (checked by the host)
constexpr unsigned char kKeep = 1, kNotFinite = 2;   // per-row flags

// items[r] = d | chunk << 8 for the r-th item of an anchor, ordered by d then chunk
__global__ void __launch_bounds__(kThreads)
thin_partial_kernel(int n, int GL, int W, int A, int C, const int* __restrict__ items,
                    const double* __restrict__ lx, const double* __restrict__ s, const double* __restrict__ s2,
                    const unsigned char* __restrict__ flags, const double* __restrict__ y,
                    const double* __restrict__ y2, double* __restrict__ part) {
  __shared__ double tile[kMaxRows * kPitch];
  const int a0 = blockIdx.x * A, rows = A + W;
  const int q = blockIdx.y * kThreads + threadIdx.x;
  int ai = 0, d = 2, c = 0, r = 0;
  bool live = q < A * C;
  if (live) {
    ai = q / C;
    r = q - ai * C;
    const int it = items[r];
    d = it & 0xff;
    c = it >> 8;
  }
  const int a = a0 + ai, b = a + d;
  live = live && b <= n - 1;
  // the rows of this item's points, relative to the block's first row; past the segment: its last point
  int off[kChunk];
  double f[kChunk];
#pragma unroll
  for (int j = 0; j < kChunk; ++j) {
    off[j] = ai + min(1 + c * kChunk + j, d - 1);
    f[j] = live ? (lx[a0 + off[j]] - lx[a]) / (lx[b] - lx[a]) : 0.0;
  }
  double res = 0.0;
  for (int sec = 0; sec < 2; ++sec) {
    const double* __restrict__ src = sec ? y2 : y;
    const double* __restrict__ sc = sec ? s2 : s;
    if (!src) break;                                     // block-uniform
    double dm[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) dm[j] = 0.0;
    for (int e0 = 0; e0 < GL; e0 += kTile) {
      const int te = min(kTile, GL - e0);
      for (int idx = threadIdx.x; idx < rows * kTile; idx += kThreads) {
        const int tr = idx / kTile, e = idx % kTile;
        const int row = a0 + tr;
        tile[tr * kPitch + e] = (row < n && e < te) ? src[(size_t)row * GL + e0 + e] : 0.0;
      }
      __syncthreads();
      if (live) {
        const double* pa = tile + ai * kPitch;
        const double* pb = pa + d * kPitch;
        for (int e = 0; e < te; ++e) {
          const double ya = pa[e];
          const double dy = pb[e] - ya;
#pragma unroll
          for (int j = 0; j < kChunk; ++j) {
            dm[j] = fmax(dm[j], fabs(ya + dy * f[j] - tile[off[j] * kPitch + e]));
          }
        }
      }
      __syncthreads();
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        const double sa = sc[a], sk = sc[a0 + off[j]], sb = sc[b];
        double scale = sa > sk ? sa : sk;
        scale = sb > scale ? sb : scale;
        const double e = rel_err(dm[j], scale);
        res = e > res ? e : res;
      }
    }
  }
  if (live) {
    unsigned char any = 0;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) any |= flags[a0 + off[j]];
    // a must-keep point strictly inside, or a row of the segment that holds a value that is not finite
    if ((any & (kKeep | kNotFinite)) || ((flags[a] | flags[b]) & kNotFinite)) res = INFINITY;
    part[(size_t)a * C + r] = res;
  }
}

// seg_err[a][d-2]: the maximum over the chunks of segment (a, a+d); first[d] is its first item
__global__ void __launch_bounds__(kThreads)
thin_fold_kernel(int n, int W, int C, const int* __restrict__ first, const double* __restrict__ part,
                 double* __restrict__ seg_err) {
  const long total = (long)n * (W - 1);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long a = i / (W - 1);
    const int d = (int)(i - a * (W - 1)) + 2;
    double v = -1.0;
    if (a + d <= n - 1) {
      const int chunks = (d - 1 + kChunk - 1) / kChunk;
      const double* p = part + (size_t)a * C + first[d];
      v = p[0];
      for (int c = 1; c < chunks; ++c) v = p[c] > v ? p[c] : v;
    }
    seg_err[i] = v;
  }
}

// the argument checks both entry points share; NDPP_OK or what fail() returned
int check_args(const char* who, int L, int G, int n, const double* x, const double* y, int n_keep,
               const double* tokeep, int window) {
  if (L < 1 || G < 1) return fail(NDPP_EINVAL, "%s: L=%d G=%d (need L, G >= 1)", who, L, G);
  if (n < 2) return fail(NDPP_EINVAL, "%s: n=%d (need n >= 2)", who, n);
  if (window < 2 || window > kMaxWindow)
    return fail(NDPP_EINVAL, "%s: window=%d (need 2..%d)", who, window, kMaxWindow);
  if (!x) return fail(NDPP_EINVAL, "%s: x is NULL", who);
  if (!y) return fail(NDPP_EINVAL, "%s: y is NULL", who);
  if (n_keep < 0) return fail(NDPP_EINVAL, "%s: n_keep=%d is negative", who, n_keep);
  if (n_keep > 0 && !tokeep) return fail(NDPP_EINVAL, "%s: tokeep is NULL with n_keep=%d", who, n_keep);
  if (int rc = check_gl_index(who, G, L)) return rc;
  // bytes of the largest arrays: the rows, and the partial maxima (at most 280 per anchor)
  if ((size_t)n > SIZE_MAX / sizeof(double) / ((size_t)G * L) || (size_t)n > SIZE_MAX / sizeof(double) / 512)
    return fail(NDPP_EINVAL, "%s: n=%d rows of G * L = %ld overflow the byte count", who, n, (long)G * L);
  return check_energy_grid(who, "x", n, x);
}

int segments(const char* who, int L, int G, int n, const double* x, const double* y, const double* y2,
             int n_keep, const double* tokeep, int W, double* seg_err) {
  const int GL = G * L;
  if (int rc = require_device(who)) return rc;

  std::vector<double> lx((size_t)n), s((size_t)n), s2(y2 ? (size_t)n : 0);
  std::vector<unsigned char> flags((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    lx[i] = std::log(x[i]);
    for (int t = 0; t < n_keep; ++t)
      if (tokeep[t] == x[i]) flags[i] |= kKeep;
    bool finite = true;
    for (int e = 0; e < GL; ++e)
      finite = finite && std::isfinite(y[(size_t)i * GL + e]) && (!y2 || std::isfinite(y2[(size_t)i * GL + e]));
    if (!finite) flags[i] |= kNotFinite;
    double m = 0.0, m2 = 0.0;
    for (int g = 0; g < G; ++g) {
      const double v = std::fabs(y[(size_t)i * GL + (size_t)g * L]);
      if (v > m) m = v;
      if (y2) {
        const double v2 = std::fabs(y2[(size_t)i * GL + (size_t)g * L]);
        if (v2 > m2) m2 = v2;
      }
    }
    s[i] = m;
    if (y2) s2[i] = m2;
  }
  // the items of one anchor and where each d starts
  std::vector<int> items, first((size_t)W + 1, 0);
  for (int d = 2; d <= W; ++d) {
    first[d] = (int)items.size();
    for (int c = 0; c * kChunk < d - 1; ++c) items.push_back(d | (c << 8));
  }
  const int C = (int)items.size();
  const int A = std::max(1, std::min(kMaxAnchors, kThreads / C));
  if (A + W > kMaxRows)
    return fail(NDPP_EINVAL, "%s: window=%d needs %d staged rows, %d at most", who, W, A + W, kMaxRows);
  const int n_anchor = n - 2;                           // anchors with a segment of d = 2 inside the grid

  DevBuf<double> d_lx, d_s, d_s2, d_y, d_y2, d_part, d_seg;
  DevBuf<unsigned char> d_flags;
  DevBuf<int> d_items, d_first;
  NDPP_TRY(d_lx.upload(lx.data(), lx.size()));
  NDPP_TRY(d_s.upload(s.data(), s.size()));
  if (y2) NDPP_TRY(d_s2.upload(s2.data(), s2.size()));
  NDPP_TRY(d_flags.upload(flags.data(), flags.size()));
  NDPP_TRY(d_items.upload(items.data(), items.size()));
  NDPP_TRY(d_first.upload(first.data(), first.size()));
  NDPP_TRY(d_y.upload(y, (size_t)n * GL));
  if (y2) NDPP_TRY(d_y2.upload(y2, (size_t)n * GL));
  NDPP_TRY(d_part.alloc((size_t)std::max(n_anchor, 1) * C));
  NDPP_TRY(d_seg.alloc((size_t)n * (W - 1)));
  {
    GpuSpan span(nullptr, -1);
    if (n_anchor > 0) {
      const dim3 grid((unsigned)((n_anchor + A - 1) / A), (unsigned)((A * C + kThreads - 1) / kThreads));
      hipLaunchKernelGGL(thin_partial_kernel, grid, dim3(kThreads), 0, 0, n, GL, W, A, C, d_items.p, d_lx.p, d_s.p,
                         y2 ? d_s2.p : nullptr, d_flags.p, d_y.p, y2 ? d_y2.p : nullptr, d_part.p);
      NDPP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(thin_fold_kernel, dim3(nblk((long)n * (W - 1), kThreads)), dim3(kThreads), 0, 0, n, W, C,
                       d_first.p, d_part.p, d_seg.p);
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(d_seg.download(seg_err, (size_t)n * (W - 1)));
  return NDPP_OK;
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_thin_segments(int L, int G, int n, const double* x, const double* y, const double* y2,
                                  int n_keep, const double* tokeep, int window, double* seg_err) {
  const int rc = check_args("thin_segments", L, G, n, x, y, n_keep, tokeep, window);
  if (rc != NDPP_OK) return rc;
  if (!seg_err) return fail(NDPP_EINVAL, "thin_segments: seg_err is NULL");
  return segments("thin_segments", L, G, n, x, y, y2, n_keep, tokeep, window, seg_err);
}

extern "C" int ndpp_thin_bounded(int L, int G, int n, const double* x, const double* y, const double* y2,
                                 int n_keep, const double* tokeep, double tol, int window, int* kept,
                                 int* n_kept, double* max_err) {
  int rc = check_args("thin_bounded", L, G, n, x, y, n_keep, tokeep, window);
  if (rc != NDPP_OK) return rc;
  if (!(std::isfinite(tol) && tol >= 0.0))
    return fail(NDPP_EINVAL, "thin_bounded: tol=%g (need a finite tol >= 0)", tol);
  if (!kept) return fail(NDPP_EINVAL, "thin_bounded: kept is NULL");
  if (!n_kept) return fail(NDPP_EINVAL, "thin_bounded: n_kept is NULL");
  if (!max_err) return fail(NDPP_EINVAL, "thin_bounded: max_err is NULL");
  const int W = window;
  std::vector<double> seg((size_t)n * (W - 1));
  rc = segments("thin_bounded", L, G, n, x, y, y2, n_keep, tokeep, W, seg.data());
  if (rc != NDPP_OK) return rc;
  // the chain: from a to the farthest admissible partner within the window (a + 1 always is)
  int a = 0, cnt = 0;
  double worst = 0.0;
  kept[cnt++] = 0;
  while (a < n - 1) {
    int next = a + 1;
    double e_next = 0.0;
    for (int d = std::min(W, n - 1 - a); d >= 2; --d) {
      const double e = seg[(size_t)a * (W - 1) + (d - 2)];
      if (e >= 0.0 && e <= tol) { next = a + d; e_next = e; break; }
    }
    if (e_next > worst) worst = e_next;
    a = next;
    kept[cnt++] = a;
  }
  *n_kept = cnt;
  *max_err = worst;
  return NDPP_OK;
}
