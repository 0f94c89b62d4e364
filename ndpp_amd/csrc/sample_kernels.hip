// sample_kernels.hip -- what a transport code does with a row (include/ndpp_hip.h: ndpp_scatt_sample,
// DESIGN.md section 18): at an incoming energy, read the section linearly in ln E, draw the outgoing
// group from the group masses and the cosine from the chosen group's row by inverting its cumulative
// distribution -- exactly for bins, by 53 fixed bisection steps of a closed-form CDF for Legendre
// moments.  Nothing in the reference does this.
//
// The row i and the weight f of row i + 1 come from the host (bracket, section_util.h: the rule of
// ndpp_lib_compare), once per event; the kernels are + - * / and comparisons only, built without
// contraction, in the order ndpp_hip.h writes out, so a host restatement with the same operation
// order gives the same bits (ndpp_amd/sample.py: sample_numpy).
//
// sample_mass_kernel: s[n][G], one thread per (row, group): P0 (Legendre) or the sequential sum of
// the bins (tabular).  Reads the section once; coalesced writes.
//
// sample_leg_kernel<L>, sample_tab_kernel: one thread per event, the grid strides over the events.
// A thread scans the two mass rows twice (2 G doubles, the second time from the cache): once for W
// and the bad-row test, once for the group.  Then it reads only the chosen group's 2 L doubles:
// about 16 (G + L) bytes per event, not 16 G L.  The Legendre kernel keeps a_l in registers behind a
// compile-time L (dispatch_moments); the tabular kernel keeps nothing per bin -- N goes up to 128 --
// and walks the chosen group's two rows twice instead (T, then the bin).  No LDS, no atomics, no
// scratch; every event writes its three outputs with ordinary stores.  Neighbouring lanes take
// different groups and leave the bisection's branches at different sides, which costs nothing: both
// sides are selects, and the trip counts (G, L, N, 53) are the same in every lane.
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "section_util.h"

namespace ndpp {
namespace {

constexpr int kThreads = 256;
constexpr int kBisections = 53;

__device__ inline double blend(double v0, double v1, double f) { return v0 + (v1 - v0) * f; }
// negative, NaN or infinite
__device__ inline bool bad_mass(double v) { return !(v >= 0.0) || !(v < INFINITY); }

__global__ void __launch_bounds__(kThreads)
sample_mass_kernel(long rows, int L, int tabular, const double* __restrict__ y, double* __restrict__ s) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    const double* p = y + (size_t)r * L;
    double m = p[0];
    if (tabular) {
      m = 0.0;
      for (int k = 0; k < L; ++k) m = m + p[k];
    }
    s[r] = m;
  }
}

// The outgoing group of one event from the mass rows s0, s1 (G doubles each) blended with f:
// NDPP_SAMPLE_OK and the group, or the status that ends the event.
__device__ inline int draw_group(int G, const double* __restrict__ s0, const double* __restrict__ s1, double f,
                                 double u, int* group) {
  double W = 0.0;
  int last = -1;
  bool bad = false;
  for (int g = 0; g < G; ++g) {
    const double w = blend(s0[g], s1[g], f);
    bad = bad || bad_mass(w);
    if (w > 0.0) last = g;
    W = W + w;
  }
  if (bad || !(W < INFINITY)) return NDPP_SAMPLE_BADROW;
  if (W == 0.0) return NDPP_SAMPLE_ZEROROW;
  const double target = u * W;
  double c = 0.0;
  int pick = -1;
  for (int g = 0; g < G; ++g) {
    c = c + blend(s0[g], s1[g], f);
    if (pick < 0 && c > target) pick = g;
  }
  *group = pick < 0 ? last : pick;
  return NDPP_SAMPLE_OK;
}

template <int L>
__global__ void __launch_bounds__(kThreads)
sample_leg_kernel(long n_ev, int G, int n, const double* __restrict__ y, const double* __restrict__ s,
                  const int* __restrict__ row, const double* __restrict__ wt, const double* __restrict__ u_g,
                  const double* __restrict__ u_mu, int* __restrict__ group, double* __restrict__ mu_out,
                  int* __restrict__ status) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_ev; e += stride) {
    const int i = row[e];
    int g = -1, st = NDPP_SAMPLE_SKIPPED;
    double mu = 0.0;
    if (i >= 0) {
      const int i1 = min(i + 1, n - 1);
      const double f = wt[e];
      st = draw_group(G, s + (size_t)i * G, s + (size_t)i1 * G, f, u_g[e], &g);
      if (st == NDPP_SAMPLE_OK) {
        const double* r0 = y + ((size_t)i * G + g) * L;
        const double* r1 = y + ((size_t)i1 * G + g) * L;
        double a[L];
        bool bad = false;
#pragma unroll
        for (int l = 0; l < L; ++l) {
          a[l] = blend(r0[l], r1[l], f);
          bad = bad || !(fabs(a[l]) < INFINITY);
        }
        if (bad) {
          st = NDPP_SAMPLE_BADROW;
          g = -1;
        } else {
          const double target = u_mu[e] * a[0];
          double lo = -1.0, hi = 1.0;
          for (int it = 0; it < kBisections; ++it) {
            const double m = 0.5 * (lo + hi);
            // F(m) = a_0/2 (m + 1) + sum_l a_l/2 (P_{l+1}(m) - P_{l-1}(m)), Bonnet upwards
            double F = (0.5 * a[0]) * (m + 1.0);
            double pm = 1.0, p = m;                    // P_{l-1}, P_l at l = 1
#pragma unroll
            for (int l = 1; l < L; ++l) {
              const double pn = (((double)(2 * l + 1) / (double)(l + 1)) * m) * p - ((double)l / (double)(l + 1)) * pm;
              F = F + (0.5 * a[l]) * (pn - pm);
              pm = p;
              p = pn;
            }
            if (F < target) lo = m; else hi = m;
          }
          mu = 0.5 * (lo + hi);
          // the density sum_l (l + 1/2) a_l P_l(mu), once
          double d = 0.0, pm = 1.0, p = mu;            // P_l, P_{l+1} at l = 0
#pragma unroll
          for (int l = 0; l < L; ++l) {
            d = d + (((double)l + 0.5) * a[l]) * pm;
            const double pn = (((double)(2 * l + 3) / (double)(l + 2)) * mu) * p - ((double)(l + 1) / (double)(l + 2)) * pm;
            pm = p;
            p = pn;
          }
          if (!(d >= 0.0)) st = NDPP_SAMPLE_NEGDENSITY;
        }
      } else {
        g = -1;
      }
    }
    group[e] = g;
    mu_out[e] = mu;
    status[e] = st;
  }
}

__global__ void __launch_bounds__(kThreads)
sample_tab_kernel(long n_ev, int G, int N, int n, const double* __restrict__ y, const double* __restrict__ s,
                  const int* __restrict__ row, const double* __restrict__ wt, const double* __restrict__ u_g,
                  const double* __restrict__ u_mu, int* __restrict__ group, double* __restrict__ mu_out,
                  int* __restrict__ status) {
  const long stride = (long)gridDim.x * blockDim.x;
  const double h = 2.0 / (double)N;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_ev; e += stride) {
    const int i = row[e];
    int g = -1, st = NDPP_SAMPLE_SKIPPED;
    double mu = 0.0;
    if (i >= 0) {
      const int i1 = min(i + 1, n - 1);
      const double f = wt[e];
      st = draw_group(G, s + (size_t)i * G, s + (size_t)i1 * G, f, u_g[e], &g);
      if (st == NDPP_SAMPLE_OK) {
        const double* r0 = y + ((size_t)i * G + g) * N;
        const double* r1 = y + ((size_t)i1 * G + g) * N;
        double T = 0.0;
        int last = -1;
        bool bad = false;
        for (int k = 0; k < N; ++k) {
          const double t = blend(r0[k], r1[k], f);
          bad = bad || bad_mass(t);
          if (t > 0.0) last = k;
          T = T + t;
        }
        if (bad || !(T < INFINITY)) {
          st = NDPP_SAMPLE_BADROW;
          g = -1;
        } else if (T == 0.0) {
          st = NDPP_SAMPLE_ZEROROW;
          g = -1;
        } else {
          const double target = u_mu[e] * T;
          double c = 0.0, below = 0.0, tk = 0.0;        // c_{k-1} and t_k of the chosen bin
          int pick = -1;
          for (int k = 0; k < N; ++k) {
            const double t = blend(r0[k], r1[k], f);
            const double cn = c + t;
            if (pick < 0 && (cn > target || k == last)) {   // (k == last: the fallback, nothing exceeds)
              pick = k;
              below = c;
              tk = t;
            }
            c = cn;
          }
          const double left = -1.0 + h * (double)pick, right = pick == N - 1 ? 1.0 : -1.0 + h * (double)(pick + 1);
          mu = -1.0 + h * ((double)pick + (target - below) / tk);
          mu = mu < left ? left : mu;
          mu = mu > right ? right : mu;
        }
      } else {
        g = -1;
      }
    }
    group[e] = g;
    mu_out[e] = mu;
    status[e] = st;
  }
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_sample_brackets(int n, const double* x, long n_ev, const double* ein, const double* u_g,
                                   const double* u_mu, int* row, double* weight) {
  if (n < 2) return fail(NDPP_EINVAL, "sample_brackets: n=%d (need n >= 2)", n);
  if (n_ev < 0) return fail(NDPP_EINVAL, "sample_brackets: n_ev=%ld (need n_ev >= 0)", n_ev);
  if (!x || !ein || !u_g || !u_mu || !row || !weight) return fail(NDPP_EINVAL, "sample_brackets: NULL argument");
  const int rc = check_energy_grid("sample_brackets", "x", n, x);
  if (rc != NDPP_OK) return rc;
  for (long e = 0; e < n_ev; ++e) {
    const double v = ein[e];
    const bool ok = std::isfinite(v) && v > 0.0 && v >= x[0] && v <= x[n - 1] && u_g[e] >= 0.0 && u_g[e] < 1.0 &&
                    u_mu[e] >= 0.0 && u_mu[e] < 1.0;
    if (!ok) {
      row[e] = -1;
      weight[e] = 0.0;
      continue;
    }
    bracket(n, x, v, &row[e], &weight[e]);
  }
  return NDPP_OK;
}

extern "C" int ndpp_scatt_sample(int scatt_type, int G, int L, int n, const double* x, const double* y, long n_ev,
                                 const double* ein, const double* u_g, const double* u_mu, int* group, double* mu,
                                 int* status) {
  if (scatt_type != NDPP_SCATT_LEGENDRE && scatt_type != NDPP_SCATT_TABULAR)
    return fail(NDPP_EINVAL, "scatt_sample: scatt_type=%d (need 0, Legendre, or 1, tabular)", scatt_type);
  const int Lmax = scatt_type == NDPP_SCATT_TABULAR ? NDPP_MAX_TAB_BINS : NDPP_MAX_ORDER;
  if (G < 1 || L < 1 || L > Lmax)
    return fail(NDPP_EINVAL, "scatt_sample: G=%d L=%d (need G >= 1 and 1 <= L <= %d)", G, L, Lmax);
  if (n < 2) return fail(NDPP_EINVAL, "scatt_sample: n=%d (need n >= 2)", n);
  if (n_ev < 0) return fail(NDPP_EINVAL, "scatt_sample: n_ev=%ld (need n_ev >= 0)", n_ev);
  if (!x || !y || !ein || !u_g || !u_mu || !group || !mu || !status)
    return fail(NDPP_EINVAL, "scatt_sample: NULL argument");
  int rc = check_gl_index("scatt_sample", G, L);
  if (rc != NDPP_OK) return rc;
  size_t y_bytes, s_bytes, ev_bytes;
  if (!bytes_of((size_t)n * G, L, sizeof(double), &y_bytes) || !bytes_of(n, G, sizeof(double), &s_bytes) ||
      !bytes_of((size_t)n_ev, 1, sizeof(double), &ev_bytes))
    return fail(NDPP_EINVAL, "scatt_sample: n=%d G=%d L=%d n_ev=%ld: the sizes overflow", n, G, L, n_ev);
  if ((rc = check_energy_grid("scatt_sample", "x", n, x))) return rc;
  if ((rc = require_device("scatt_sample"))) return rc;
  if (n_ev == 0) return NDPP_OK;

  // row and weight per event; row -1 marks the events that are skipped
  std::vector<int> row((size_t)n_ev);
  std::vector<double> wt((size_t)n_ev);
  if ((rc = ndpp_sample_brackets(n, x, n_ev, ein, u_g, u_mu, row.data(), wt.data()))) return rc;

  const long rows = (long)n * G;
  DevBuf<double> d_y, d_s, d_wt, d_ug, d_umu, d_mu;
  DevBuf<int> d_row, d_group, d_status;
  NDPP_TRY(d_y.upload(y, (size_t)rows * L));
  NDPP_TRY(d_s.alloc((size_t)rows));
  NDPP_TRY(d_row.upload(row.data(), row.size()));
  NDPP_TRY(d_wt.upload(wt.data(), wt.size()));
  NDPP_TRY(d_ug.upload(u_g, (size_t)n_ev));
  NDPP_TRY(d_umu.upload(u_mu, (size_t)n_ev));
  NDPP_TRY(d_group.alloc((size_t)n_ev));
  NDPP_TRY(d_mu.alloc((size_t)n_ev));
  NDPP_TRY(d_status.alloc((size_t)n_ev));
  {
    GpuSpan span(nullptr, -1);
    const bool tabular = scatt_type == NDPP_SCATT_TABULAR;
    hipLaunchKernelGGL(sample_mass_kernel, dim3(nblk(rows, kThreads)), dim3(kThreads), 0, 0, rows, L, (int)tabular,
                       d_y.p, d_s.p);
    NDPP_TRY(hipGetLastError());
    const dim3 grid(nblk(n_ev, kThreads));
    if (tabular) {
      hipLaunchKernelGGL(sample_tab_kernel, grid, dim3(kThreads), 0, 0, n_ev, G, L, n, d_y.p, d_s.p, d_row.p, d_wt.p,
                         d_ug.p, d_umu.p, d_group.p, d_mu.p, d_status.p);
    } else {
      dispatch_moments(L, [&](auto tag) {
        hipLaunchKernelGGL(sample_leg_kernel<decltype(tag)::value>, grid, dim3(kThreads), 0, 0, n_ev, G, n, d_y.p,
                           d_s.p, d_row.p, d_wt.p, d_ug.p, d_umu.p, d_group.p, d_mu.p, d_status.p);
      });
    }
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(d_group.download(group, (size_t)n_ev));
  NDPP_TRY(d_mu.download(mu, (size_t)n_ev));
  NDPP_TRY(d_status.download(status, (size_t)n_ev));
  return NDPP_OK;
}
