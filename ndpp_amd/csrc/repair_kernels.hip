// repair_kernels.hip -- repair of negative Legendre rows, certified positive (ndpp_scatt_repair).
// Replaces nothing: the reference never repairs a row.  A row that ndpp_scatt_minimum classes
// NEGATIVE becomes a_l * w_l(t) with the largest t of a bisection for which minimum_row
// (minimum_row.h, the search ndpp_scatt_minimum runs) classes the filtered row POSITIVE.  Definition,
// families and the rules for the rows are in ndpp_hip.h; DESIGN.md section 16 argues why a passing t
// exists and what each family keeps.
//
// The host classifies on the device (launch_minimum, the matrix stays there), downloads the classes,
// lists the rows to repair in (iE, g) order and copies the matrix device-to-device into the output.
// repair_kernel then takes one thread per LISTED row in blocks of one wave: the moments a_l and the
// filtered row live in VGPRs, the 65-node basis is read by scalar loads as in minimum_kernel, and the
// search is one loop nest with minimum_row at ONE call site (every lane makes the same steps trips
// per family; inside a trip the lanes diverge as they do in minimum_kernel).  No LDS, no atomics;
// the repaired row, t and how leave by plain vector stores.
//
// Built -DNDPP_FAST=0 -ffp-contract=off in every build.  The weights are products only, in the
// order ndpp_hip.h writes down, so a host restatement (ndpp_amd/repair.py: weights) gives the same bits.
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

constexpr int kHowHeat = 1, kHowUniform = 2, kHowUnrepairable = 3, kHowNonfinite = 4;

// r_l = a_l * w_l(t): heat w_l = t^(l(l+1)/2) by p = p * t, w = w * p; uniform w_l = t; w_0 = 1
template <int NM>
__host__ __device__ inline void filtered_row(const double (&a)[NM], double t, int family, double (&r)[NM]) {
  r[0] = a[0];
  double p = t, w = t;
#pragma unroll
  for (int l = 1; l < NM; ++l) {
    if (l >= 2 && family == kHowHeat) { p = p * t; w = w * p; }
    r[l] = a[l] * w;
  }
}

template <int NM>
__global__ void __launch_bounds__(64)
repair_kernel(long n_list, const long* __restrict__ list /* row = iE * G + g */, const double* __restrict__ mat,
              int mode, int steps, double rel_tol, const double* __restrict__ basis /* [65][NM] */,
              double* __restrict__ out /* [.][NM], holds a copy of mat */, double* __restrict__ out_t /* [n_list] */,
              int* __restrict__ out_how /* [n_list] */, int* __restrict__ out_evals /* [n_list] or null */) {
  const long k = (long)blockIdx.x * 64 + threadIdx.x;
  if (k >= n_list) return;
  const size_t at = (size_t)list[k];
  double a[NM];
#pragma unroll
  for (int l = 0; l < NM; ++l) a[l] = mat[at * NM + l];

  const int first = mode == NDPP_REPAIR_UNIFORM ? kHowUniform : kHowHeat;
  const int last = mode == NDPP_REPAIR_HEAT ? kHowHeat : kHowUniform;
  const int trips = a[0] == 0.0 ? 0 : steps;       // P0 = 0: only the zero row can pass, t = 0
  double t_best = 0.0;
  int how = first, evals = 0;
  for (int family = first; family <= last; ++family) {
    double t_pass = 0.0, t_fail = 1.0;             // dyadic, t_fail - t_pass = 2^-trip: the midpoint is exact
    for (int s = 0; s < trips; ++s) {
      const double t = (t_pass + t_fail) * 0.5;
      double r[NM];
      filtered_row<NM>(a, t, family, r);
      double lo, hi, mu_at;
      int cls, ev;
      minimum_row<NM>(r, rel_tol, basis, &lo, &hi, &mu_at, &cls, &ev);
      evals += ev;
      if ((cls & 3) == NDPP_MIN_POSITIVE) t_pass = t;
      else t_fail = t;
    }
    if (family == first || t_pass >= t_best) { t_best = t_pass; how = family; }   // uniform on a tie
  }
  double r[NM];
  filtered_row<NM>(a, t_best, how, r);
#pragma unroll
  for (int l = 0; l < NM; ++l) out[at * NM + l] = r[l];
  out_t[k] = t_best;
  out_how[k] = how;
  if (out_evals) out_evals[k] = evals;
}

const ndpp_repair kNoRepair{0, 0, 0, 0, 0, 0, 1.0, -1, -1};

int repair_impl(int n_ein, int G, int L, const double* mat, int mode, int steps, int undecided, double rel_tol,
                double* out, double* t, int* how, int* evals, ndpp_repair* summary) {
  const char* who = "scatt_repair";
  if (L < 1 || L > NDPP_MAX_ORDER) return fail(NDPP_EINVAL, "%s: L=%d outside 1..%d", who, L, NDPP_MAX_ORDER);
  if (n_ein < 0 || G < 1) return fail(NDPP_EINVAL, "%s: n_ein=%d G=%d", who, n_ein, G);
  if (mode != NDPP_REPAIR_BEST && mode != NDPP_REPAIR_HEAT && mode != NDPP_REPAIR_UNIFORM)
    return fail(NDPP_EINVAL, "%s: mode=%d is none of NDPP_REPAIR_BEST, _HEAT, _UNIFORM", who, mode);
  if (steps < 1 || steps > 52) return fail(NDPP_EINVAL, "%s: steps=%d outside 1..52", who, steps);
  if (!(rel_tol >= 0.0) || !(rel_tol <= DBL_MAX))
    return fail(NDPP_EINVAL, "%s: rel_tol=%g is not a finite value >= 0", who, rel_tol);
  if (!mat || !out || !t || !how || !summary)
    return fail(NDPP_EINVAL, "%s: NULL mat, out, t, how or summary", who);
  size_t mat_bytes = 0, row_bytes = 0;
  if (!bytes_of((size_t)n_ein, (size_t)G, (size_t)L * sizeof(double), &mat_bytes) ||
      !bytes_of((size_t)n_ein, (size_t)G, 4 * sizeof(double) + 2 * sizeof(int) + 2 * sizeof(long), &row_bytes))
    return fail(NDPP_EINVAL, "%s: sizes overflow (n_ein=%d G=%d L=%d)", who, n_ein, G, L);
  *summary = kNoRepair;
  if (n_ein == 0) return NDPP_OK;
  int rc = require_device();
  if (rc) return rc;

  // the classes of the rows as they are (t = 1), on the device
  const std::vector<double> basis = node_basis(L);
  const size_t rows = (size_t)n_ein * G;
  DevBuf<double> d_mat, d_basis, d_lo, d_hi, d_mu, d_out;
  DevBuf<int> d_cls;
  NDPP_TRY(d_mat.upload(mat, rows * L));
  NDPP_TRY(d_basis.upload(basis.data(), basis.size()));
  NDPP_TRY(d_lo.alloc(rows));
  NDPP_TRY(d_hi.alloc(rows));
  NDPP_TRY(d_mu.alloc(rows));
  NDPP_TRY(d_cls.alloc(rows));
  NDPP_TRY(d_out.alloc(rows * L));
  {
    GpuSpan span(nullptr, -1);
    launch_minimum(n_ein, G, L, L, d_mat.p, rel_tol, d_basis.p, d_lo.p, d_hi.p, d_mu.p, d_cls.p, nullptr);
    NDPP_CLOSE_SPAN(span);
  }
  std::vector<int> cls(rows);
  NDPP_TRY(d_cls.download(cls.data(), rows));

  // who is repaired, in (iE, g) order; everything the kernel does not write is decided here
  ndpp_repair s = kNoRepair;
  std::vector<long> list;
  for (size_t at = 0; at < rows; ++at) {
    t[at] = -1.0;
    how[at] = -1;
    if (evals) evals[at] = 0;
    if (cls[at] < 0) continue;
    ++s.rows;
    t[at] = 1.0;
    how[at] = 0;
    const int k = cls[at] & 3;
    if (k == NDPP_MIN_NONFINITE) {
      how[at] = kHowNonfinite;
      ++s.nonfinite;
    } else if (k == NDPP_MIN_NEGATIVE || (k == NDPP_MIN_UNDECIDED && undecided)) {
      if (mat[at * L] < 0.0) {
        how[at] = kHowUnrepairable;
        ++s.unrepairable;
      } else {
        list.push_back((long)at);
      }
    }
  }
  const size_t n_list = list.size();
  if ((n_list + 63) / 64 > (size_t)INT_MAX)
    return fail(NDPP_EINVAL, "%s: %zu rows to repair do not fit one launch", who, n_list);

  NDPP_TRY(hipMemcpy(d_out.p, d_mat.p, rows * L * sizeof(double), hipMemcpyDeviceToDevice));
  std::vector<double> t_list(n_list);
  std::vector<int> how_list(n_list), evals_list(evals ? n_list : 0);
  if (n_list) {
    DevBuf<long> d_list;
    DevBuf<double> d_t;
    DevBuf<int> d_how, d_evals;
    NDPP_TRY(d_list.upload(list.data(), n_list));
    NDPP_TRY(d_t.alloc(n_list));
    NDPP_TRY(d_how.alloc(n_list));
    if (evals) NDPP_TRY(d_evals.alloc(n_list));
    {
      GpuSpan span(nullptr, -1);             // ndpp_last_gpu_ms: the repair kernel alone
      dispatch_moments(L, [&](auto nm) {
        hipLaunchKernelGGL(repair_kernel<decltype(nm)::value>, dim3((unsigned)((n_list + 63) / 64)), dim3(64), 0, 0,
                           (long)n_list, d_list.p, d_mat.p, mode, steps, rel_tol, d_basis.p, d_out.p, d_t.p, d_how.p,
                           evals ? d_evals.p : nullptr);
      });
      NDPP_CLOSE_SPAN(span);
    }
    NDPP_TRY(d_t.download(t_list.data(), n_list));
    NDPP_TRY(d_how.download(how_list.data(), n_list));
    if (evals) NDPP_TRY(d_evals.download(evals_list.data(), n_list));
  }
  NDPP_TRY(d_out.download(out, rows * L));

  for (size_t k = 0; k < n_list; ++k) {
    const size_t at = (size_t)list[k];
    t[at] = t_list[k];
    how[at] = how_list[k];
    if (evals) evals[at] = evals_list[k];
    ++s.repaired;
    s.heat += how_list[k] == kHowHeat;
    s.uniform += how_list[k] == kHowUniform;
    if (t_list[k] < s.min_t) {
      s.min_t = t_list[k];
      s.min_ein = (int)(at / G);
      s.min_group = (int)(at % G);
    }
  }
  *summary = s;
  return NDPP_OK;
}

}  // namespace
}  // namespace ndpp

extern "C" int ndpp_scatt_repair(int n_ein, int G, int L, const double* mat, int mode, int steps, int undecided,
                                 double rel_tol, double* out, double* t, int* how, ndpp_repair* summary) {
  return ndpp::repair_impl(n_ein, G, L, mat, mode, steps, undecided, rel_tol, out, t, how, nullptr, summary);
}

extern "C" int ndpp_scatt_repair_evals(int n_ein, int G, int L, const double* mat, int mode, int steps, int undecided,
                                       double rel_tol, double* out, double* t, int* how, int* evals,
                                       ndpp_repair* summary) {
  if (!evals) return ndpp::fail(NDPP_EINVAL, "scatt_repair: NULL evals");
  return ndpp::repair_impl(n_ein, G, L, mat, mode, steps, undecided, rel_tol, out, t, how, evals, summary);
}
