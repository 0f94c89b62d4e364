// minimum_kernels.hip -- certified positivity: for every (E_in, group) row of a matrix section an
// enclosure lo <= min over [-1, 1] of f <= hi of the truncated Legendre expansion
//   f(mu) = sum_{l < n_mom} c_l P_l(mu),   c_l = (l + 1/2) a_l,
// where hi = f(mu_at) is an attained value.  Replaces nothing: the reference (and
// ndpp_scatt_positivity, expand_kernels.hip) sample f on a grid.  Definition, classes and the rules
// for the rows are in ndpp_hip.h; why the bound holds is argued in DESIGN.md section 15.
//
// The search of one row (minimum_row) is in minimum_row.h, which repair_kernels.hip shares.  Here:
// one thread per row; a block holds whole incoming energies, so the band comes from LDS (block_shape
// and block_band, section_util.h).
//
// Built -DNDPP_FAST=0 -ffp-contract=off in every build: + - * / and comparisons in the order written,
// so two calls return the same bits.  Plain vector stores only, no atomics on floating point.
#include <cfloat>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "minimum_row.h"
#include "section_util.h"

namespace ndpp {
namespace {

template <int NM>
__global__ void __launch_bounds__(kMaxBlock)
minimum_kernel(int n_ein, int G, int L, int epb, const double* __restrict__ mat, double rel_tol,
               const double* __restrict__ basis /* [65][NM] */, double* __restrict__ out_lo,
               double* __restrict__ out_hi, double* __restrict__ out_mu, int* __restrict__ out_cls,
               int* __restrict__ out_evals /* or null */) {
  __shared__ int s_gmin[kMaxBlock], s_gmax[kMaxBlock];
  const int tid = threadIdx.x, B = blockDim.x;
  const long e0 = (long)blockIdx.x * epb;
  const int ne = (int)min((long)epb, (long)n_ein - e0);
  const int R = ne * G;

  block_band(mat, e0, ne, G, L, s_gmin, s_gmax);

  for (int r = tid; r < R; r += B) {
    const int e = r / G, g = r - e * G;
    const int gmin = s_gmin[e], gmax = s_gmax[e];
    const size_t at = (size_t)(e0 * G + r);
    double lo = 0.0, hi = 0.0, mu_at = 0.0;
    int cls = -1, evals = 0;
    if (gmin > gmax) {                       // no P0 > 0: one zero row at g = 0, lo = hi = 0, positive
      if (g == 0) cls = NDPP_MIN_POSITIVE;
    } else if (g >= gmin && g <= gmax) {
      minimum_row<NM>(mat + at * L, rel_tol, basis, &lo, &hi, &mu_at, &cls, &evals);
    }
    out_lo[at] = lo;
    out_hi[at] = hi;
    out_mu[at] = mu_at;
    out_cls[at] = cls;
    if (out_evals) out_evals[at] = evals;
  }
}

int minimum_impl(int n_ein, int G, int L, const double* mat, int n_moments, double rel_tol, double* lo,
                 double* hi, double* mu_at, int* cls, int* evals, ndpp_minimum* summary) {
  const char* who = "scatt_minimum";
  if (L < 1 || L > NDPP_MAX_ORDER) return fail(NDPP_EINVAL, "%s: L=%d outside 1..%d", who, L, NDPP_MAX_ORDER);
  if (n_moments < 1 || n_moments > L)
    return fail(NDPP_EINVAL, "%s: n_moments=%d outside 1..L=%d", who, n_moments, L);
  if (n_ein < 0 || G < 1) return fail(NDPP_EINVAL, "%s: n_ein=%d G=%d", who, n_ein, G);
  if (!(rel_tol >= 0.0) || !(rel_tol <= DBL_MAX))
    return fail(NDPP_EINVAL, "%s: rel_tol=%g is not a finite value >= 0", who, rel_tol);
  if (!mat || !lo || !hi || !mu_at || !cls || !summary)
    return fail(NDPP_EINVAL, "%s: NULL mat, lo, hi, mu_at, cls or summary", who);
  size_t mat_bytes = 0, row_bytes = 0;
  if (!bytes_of((size_t)n_ein, (size_t)G, (size_t)L * sizeof(double), &mat_bytes) ||
      !bytes_of((size_t)n_ein, (size_t)G, 3 * sizeof(double) + 2 * sizeof(int), &row_bytes))
    return fail(NDPP_EINVAL, "%s: sizes overflow (n_ein=%d G=%d L=%d)", who, n_ein, G, L);
  *summary = ndpp_minimum{0, 0, 0, 0, 0, INFINITY, 0.0, -1, -1};
  if (n_ein == 0) return NDPP_OK;
  int rc = require_device();
  if (rc) return rc;

  const std::vector<double> basis = node_basis(n_moments);
  const size_t rows = (size_t)n_ein * G;
  DevBuf<double> d_mat, d_basis, d_lo, d_hi, d_mu;
  DevBuf<int> d_cls, d_evals;
  NDPP_TRY(d_mat.upload(mat, rows * L));
  NDPP_TRY(d_basis.upload(basis.data(), basis.size()));
  NDPP_TRY(d_lo.alloc(rows));
  NDPP_TRY(d_hi.alloc(rows));
  NDPP_TRY(d_mu.alloc(rows));
  NDPP_TRY(d_cls.alloc(rows));
  if (evals) NDPP_TRY(d_evals.alloc(rows));
  {
    GpuSpan span(nullptr, -1);
    launch_minimum(n_ein, G, L, n_moments, d_mat.p, rel_tol, d_basis.p, d_lo.p, d_hi.p, d_mu.p, d_cls.p,
                   evals ? d_evals.p : nullptr);
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(d_lo.download(lo, rows));
  NDPP_TRY(d_hi.download(hi, rows));
  NDPP_TRY(d_mu.download(mu_at, rows));
  NDPP_TRY(d_cls.download(cls, rows));
  if (evals) NDPP_TRY(d_evals.download(evals, rows));

  // the summary, folded here from the dense arrays in (iE, g) order
  ndpp_minimum s{0, 0, 0, 0, 0, INFINITY, 0.0, -1, -1};
  for (int iE = 0; iE < n_ein; ++iE) {
    bool any_p0 = false;
    for (int g = 0; g < G && !any_p0; ++g) any_p0 = mat[((size_t)iE * G + g) * L] > 0.0;
    for (int g = 0; g < G; ++g) {
      const size_t at = (size_t)iE * G + g;
      if (cls[at] < 0) continue;
      ++s.rows;
      const int k = cls[at] & 3;
      s.negative += k == NDPP_MIN_NEGATIVE;
      s.undecided += k == NDPP_MIN_UNDECIDED;
      s.nonfinite += k == NDPP_MIN_NONFINITE;
      s.unsettled += (cls[at] & NDPP_MIN_UNSETTLED) != 0;
      if (k != NDPP_MIN_NONFINITE && hi[at] < s.min_hi) {
        s.min_hi = hi[at];
        s.min_mu = mu_at[at];
        s.min_ein = iE;
        s.min_group = any_p0 ? g : -1;
      }
    }
  }
  *summary = s;
  return NDPP_OK;
}

}  // namespace

void launch_minimum(int n_ein, int G, int L, int n_moments, const double* mat, double rel_tol, const double* basis,
                    double* lo, double* hi, double* mu_at, int* cls, int* evals) {
  int epb = 1, threads = 64;
  block_shape(G, &epb, &threads);
  const int nblk = (n_ein + epb - 1) / epb;
  dispatch_moments(n_moments, [&](auto nm) {
    hipLaunchKernelGGL(minimum_kernel<decltype(nm)::value>, dim3(nblk), dim3(threads), 0, 0, n_ein, G, L, epb, mat, rel_tol,
                       basis, lo, hi, mu_at, cls, evals);
  });
}

}  // namespace ndpp

extern "C" int ndpp_scatt_minimum(int n_ein, int G, int L, const double* mat, int n_moments, double rel_tol,
                                  double* lo, double* hi, double* mu_at, int* cls, ndpp_minimum* summary) {
  return ndpp::minimum_impl(n_ein, G, L, mat, n_moments, rel_tol, lo, hi, mu_at, cls, nullptr, summary);
}

extern "C" int ndpp_scatt_minimum_evals(int n_ein, int G, int L, const double* mat, int n_moments, double rel_tol,
                                        double* lo, double* hi, double* mu_at, int* cls, int* evals,
                                        ndpp_minimum* summary) {
  if (!evals) return ndpp::fail(NDPP_EINVAL, "scatt_minimum: NULL evals");
  return ndpp::minimum_impl(n_ein, G, L, mat, n_moments, rel_tol, lo, hi, mu_at, cls, evals, summary);
}
