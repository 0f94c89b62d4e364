// nbody_kernels.hip -- ACE law 66, N-body phase space (include/ndpp_hip.h: ndpp_nbody_leg_batch,
// DESIGN.md section 20).  The reference leaves such a reaction uninitialised
// (scattdata_header.F90:105-109); nothing in it does this.  The density is closed-form at every
// incoming energy, so there is no table and no interpolation in E_in: per (E_in, group) a product
// Gauss-Legendre rule over the CM energy (in t, T = Emax sin^2(2 atan t)) and over sqrt(E'), cut at the
// values of t where a group edge enters or leaves the kinematic window.
//
// The kernels are + - * / sqrt and comparisons only, built without contraction in every build, in
// the order ndpp_hip.h writes out, so a host restatement with the same operation order gives the
// same bits (tests/nbody_ref.py: nbody_numpy).
//
// nbody_kernel<L>: kItems (E_in, group) items per block, 32 lanes each.  A lane is one outer node of
// the piece in hand: it runs the 32 inner nodes in ascending order with its L sums in registers (L is
// a compile-time constant, dispatch_moments), scales them and leaves them in LDS; lane l < L of the
// item then adds the 32 outer nodes of moment l in ascending order and the piece to its total: the
// sum order of the definition, whatever the hardware does with the lanes.  At most five pieces, each
// behind a block-wide barrier that every thread reaches (the loops over items and pieces have the
// same trip counts in every thread).  An item whose group misses the lab window, or whose energy is
// not integrated, idles and writes zeros.  No atomics, no scratch; 23 KB of LDS at L = 11.
//
// nbody_tab_kernel (ndpp_nbody_tab_batch): one thread per output element (E_in, group, bin);
// neighbouring lanes are neighbouring bins of one group, so the energy, the group edges and the ends of
// the s' range are the same in a wave.  In the lab variables (s' = sqrt(E'), mu) the density integrates
// over a cosine bin in closed form, so a bin is a one-dimensional rule in s': at most five pieces
// between the values of s' where a bin edge enters or leaves the kinematic window, 32 nodes each, run
// sequentially by the thread in the sum order of the definition.  The breakpoints live in named
// registers and are sorted by the same network as above.  No LDS, no barrier, no atomics, no scratch.
#include <cfloat>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "file6_device.h"
#include "kernels.h"
#include "nbody_rule.h"
#include "section_util.h"

namespace ndpp {
namespace {

constexpr int kOrder = NDPP_NBODY_ORDER;   // nodes of either rule = lanes of an item
constexpr int kItems = 8;
constexpr int kThreads = kItems * kOrder;
constexpr int kRow = kOrder + 1;           // LDS row of one moment, padded by one bank
constexpr int kMaxPieces = 5;              // four breakpoints at most

__constant__ double d_x[kOrder] = {NDPP_NBODY_X};
__constant__ double d_w[kOrder] = {NDPP_NBODY_W};
const double h_x[kOrder] = {NDPP_NBODY_X};
const double h_w[kOrder] = {NDPP_NBODY_W};
const double h_two_over_b[3] = {NDPP_NBODY_TWO_OVER_B};

int g_nbody = 0;       // ndpp_set_nbody: process-wide
int g_nbody_tab = 0;   // ndpp_set_nbody_tab: process-wide

struct NbodyArgs {
  double awr, Q, Ap, two_over_b;
  int n_bodies, n_ein, G;
  const double *ein, *e_bins;
  double* out;
};

// The breakpoint in t of the CM energy Tb = d^2 (d = sqrt(Eg) -+ sqrt(E0)) when 0 < Tb < Emax;
// 1.0, the end of the range, otherwise.
__device__ inline double breakpoint(double d, double Emax) {
  const double Tb = d * d;
  if (!(Tb > 0.0) || !(Tb < Emax)) return 1.0;
  const double sg = sqrt(Tb / Emax);
  return sg / (1.0 + sqrt(1.0 - sg * sg));
}

__device__ inline void order2(double& a, double& b) {
  const double lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// one outer node of one item: the L scaled inner sums v[l] = (wt W) I_l
template <int L>
__device__ inline void outer_node(const NbodyArgs& a, double Emax, double rE0, double rlo, double rhi, double pa,
                                  double pb, int j, double* v) {
  const double hm = 0.5 * (pb - pa), cm = 0.5 * (pb + pa);
  const double t = cm + hm * d_x[j];
  const double wt = hm * d_w[j];
  const double q = 1.0 + t * t;
  const double s = (2.0 * t) / q;
  const double c = (1.0 - t * t) / q;
  const double s2 = s * s;
  const double T = Emax * s2;
  const double c2 = c * c, c4 = c2 * c2;
  const double cp = a.n_bodies == 3 ? c2 : (a.n_bodies == 4 ? c4 * c : c4 * c4);   // c^(3n - 7)
  const double W = ((a.two_over_b * s2) * cp) * (2.0 / q);
  const double rT = sqrt(T);
  const double dlt = fabs(rT - rE0);
  const double ia = dlt > rlo ? dlt : rlo;
  const double sum = rT + rE0;
  const double ib = sum < rhi ? sum : rhi;
  double I[L];
#pragma unroll
  for (int l = 0; l < L; ++l) I[l] = 0.0;
  if (ib > ia) {
    const double hm2 = 0.5 * (ib - ia), cm2 = 0.5 * (ib + ia);
    const double den = (2.0 * rT) * rE0;
    for (int k = 0; k < kOrder; ++k) {
      const double sp = cm2 + hm2 * d_x[k];
      const double fk = (hm2 * d_w[k]) * (sp / den);
      double mu = ((sp - rT) * (sp + rT)) / ((2.0 * sp) * rE0) + rE0 / (2.0 * sp);
      mu = mu < -1.0 ? -1.0 : mu;
      mu = mu > 1.0 ? 1.0 : mu;
      double pm = 1.0, p = mu;                     // P_{l-1}, P_l at l = 1
      I[0] = I[0] + fk * pm;
#pragma unroll
      for (int l = 1; l < L; ++l) {
        I[l] = I[l] + fk * p;
        const double pn = (((double)(2 * l + 1) / (double)(l + 1)) * mu) * p - ((double)l / (double)(l + 1)) * pm;
        pm = p;
        p = pn;
      }
    }
  }
  const double ww = wt * W;
#pragma unroll
  for (int l = 0; l < L; ++l) v[l] = ww * I[l];
}

template <int L>
__global__ void __launch_bounds__(kThreads) nbody_kernel(NbodyArgs a) {
  __shared__ double fold[kItems][L][kRow];
  const int sub = threadIdx.x / kOrder, lane = threadIdx.x % kOrder;
  const long tot = (long)a.n_ein * a.G;
  for (long base = (long)blockIdx.x * kItems; base < tot; base += (long)gridDim.x * kItems) {
    const long item = base + sub;
    const bool in_range = item < tot;
    bool live = false;
    double Emax = 0.0, rE0 = 0.0, rlo = 0.0, rhi = 0.0;
    double b0 = 1.0, b1 = 1.0, b2 = 1.0, b3 = 1.0;   // the breakpoints, ascending; 1.0: none
    if (in_range) {
      const int e = (int)(item / a.G), g = (int)(item % a.G);
      const double E = a.ein[e], lo = a.e_bins[g], hi = a.e_bins[g + 1];
      if (E > 0.0 && E <= DBL_MAX) {
        Emax = ((a.Ap - 1.0) / a.Ap) * ((a.awr / (a.awr + 1.0)) * E + a.Q);
        const double E0 = E / ((a.awr + 1.0) * (a.awr + 1.0));
        if (Emax > 0.0) {
          rE0 = sqrt(E0);
          const double rEm = sqrt(Emax);
          const double wd = rE0 - rEm;                // (Emax >= E0: a neutron can be left at rest)
          const double wl = wd > 0.0 ? wd : 0.0;
          const double wh = rEm + rE0;
          live = hi > wl * wl && lo < wh * wh;       // the group meets the lab window
          if (live) {
            rlo = sqrt(lo);
            rhi = sqrt(hi);
            b0 = breakpoint(rlo - rE0, Emax); b1 = breakpoint(rlo + rE0, Emax);
            b2 = breakpoint(rhi - rE0, Emax); b3 = breakpoint(rhi + rE0, Emax);
            order2(b0, b1); order2(b2, b3); order2(b0, b2); order2(b1, b3); order2(b1, b2);
          }
        }
      }
    }
    double total = 0.0;                              // of moment `lane`, in lanes < L
    double pa = 0.0;
#pragma unroll 1
    for (int pc = 0; pc < kMaxPieces; ++pc) {          // (one copy of the node's code, not five)
      const double pb = pc == 0 ? b0 : (pc == 1 ? b1 : (pc == 2 ? b2 : (pc == 3 ? b3 : 1.0)));
      const bool on = live && pb > pa;                 // (equal ends: a duplicate breakpoint, no piece)
      if (on) {
        double v[L];
        outer_node<L>(a, Emax, rE0, rlo, rhi, pa, pb, lane, v);
#pragma unroll
        for (int l = 0; l < L; ++l) fold[sub][l][lane] = v[l];
      }
      __syncthreads();
      if (on && lane < L) {
        double s = 0.0;
        for (int j = 0; j < kOrder; ++j) s = s + fold[sub][lane][j];
        total = total + s;
      }
      __syncthreads();
      pa = pb;
    }
    if (in_range && lane < L) a.out[(size_t)item * L + lane] = total;
  }
}


// ---- tabular output ------------------------------------------------------------------------------
constexpr int kTabThreads = 256;

struct NbodyTabArgs {
  double awr, Q, Ap, two_over_b;
  int n_bodies, n_ein, G, N;
  const double *ein, *e_bins;
  double* out;
};

// tab_kernels.hip's bin edge, the same expression: the edges are the other tabular paths' in every bit
__device__ __forceinline__ double tab_edge(int k, int N) {
  return k >= N ? 1.0 : -1.0 + (2.0 * (double)k) / (double)N;
}

// The root c + sgn sqrt(disc) of y(m, s') = 0 (c = m rE0) when it lies strictly inside (a, b); b, the
// end of the range, otherwise.
__device__ inline double tab_root(double c, double disc, double sgn, double a, double b) {
  if (!(disc > 0.0)) return b;
  const double r = c + sgn * sqrt(disc);
  return (r > a && r < b) ? r : b;
}

// one piece [pa, pb] of one bin: the 32 nodes in ascending order, from 0.0
__device__ inline double tab_piece(int n_bodies, double Emax, double rE0, double c0, double c1, double disc0,
                                   double disc1, double dm, double pa, double pb) {
  const double len = pb - pa;
  double piece = 0.0;
  for (int j = 0; j < kOrder; ++j) {
    const double u = 0.5 + 0.5 * d_x[j];
    const double h = (u * u) * (3.0 - 2.0 * u);
    const double sp = pa + len * h;
    const double wgt = ((0.5 * d_w[j]) * len) * ((6.0 * u) * (1.0 - u));
    const double t0 = sp - c0, t1 = sp - c1;
    const double y0 = (disc0 - t0 * t0) / Emax;
    const double y1 = (disc1 - t1 * t1) / Emax;
    const double y0c = y0 > 0.0 ? y0 : 0.0;
    const double y1c = y1 > 0.0 ? y1 : 0.0;
    double f = 0.0;
    if (y1c > 0.0) {
      const double d = y0 > 0.0 ? (((2.0 * sp) * rE0) * dm) / Emax : y1c;
      const double q2 = (y1c * y1c + y1c * y0c) + y0c * y0c;
      double D;
      if (n_bodies == 4) {
        D = q2;
      } else if (n_bodies == 3) {
        D = q2 / (y1c * sqrt(y1c) + y0c * sqrt(y0c));
      } else {
        const double a3 = (y1c * y1c) * y1c, b3 = (y0c * y0c) * y0c;
        D = (q2 * ((a3 * a3 + a3 * b3) + b3 * b3)) / ((a3 * y1c) * sqrt(y1c) + (b3 * y0c) * sqrt(y0c));
      }
      f = (sp * d) * D;
    }
    piece = piece + wgt * f;
  }
  return piece;
}

__global__ void __launch_bounds__(kTabThreads) nbody_tab_kernel(NbodyTabArgs a) {
  const long tot = (long)a.n_ein * a.G * a.N;
  for (long idx = (long)blockIdx.x * kTabThreads + threadIdx.x; idx < tot; idx += (long)gridDim.x * kTabThreads) {
    const int k = (int)(idx % a.N);
    const long item = idx / a.N;
    const int e = (int)(item / a.G), g = (int)(item % a.G);
    const double E = a.ein[e], lo = a.e_bins[g], hi = a.e_bins[g + 1];
    double val = 0.0;
    if (E > 0.0 && E <= DBL_MAX) {
      const double Emax = ((a.Ap - 1.0) / a.Ap) * ((a.awr / (a.awr + 1.0)) * E + a.Q);
      const double E0 = E / ((a.awr + 1.0) * (a.awr + 1.0));
      if (Emax > 0.0) {
        const double rE0 = sqrt(E0), rEm = sqrt(Emax);
        const double wd = rE0 - rEm;
        const double wl = wd > 0.0 ? wd : 0.0;
        const double wh = rEm + rE0;
        if (hi > wl * wl && lo < wh * wh) {          // the group meets the lab window
          const double rlo = sqrt(lo), rhi = sqrt(hi);
          const double sa = rlo > wl ? rlo : wl, sb = rhi < wh ? rhi : wh;
          const double m0 = tab_edge(k, a.N), m1 = tab_edge(k + 1, a.N);
          const double dm = m1 - m0;
          const double c0 = m0 * rE0, c1 = m1 * rE0;
          const double disc0 = Emax - E0 * ((1.0 - m0) * (1.0 + m0));
          const double disc1 = Emax - E0 * ((1.0 - m1) * (1.0 + m1));
          double b0 = tab_root(c0, disc0, -1.0, sa, sb), b1 = tab_root(c0, disc0, 1.0, sa, sb);
          double b2 = tab_root(c1, disc1, -1.0, sa, sb), b3 = tab_root(c1, disc1, 1.0, sa, sb);
          order2(b0, b1); order2(b2, b3); order2(b0, b2); order2(b1, b3); order2(b1, b2);
          double total = 0.0, pa = sa;
#pragma unroll 1
          for (int pc = 0; pc < kMaxPieces; ++pc) {    // (one copy of the node's code, not five)
            const double pb = pc == 0 ? b0 : (pc == 1 ? b1 : (pc == 2 ? b2 : (pc == 3 ? b3 : sb)));
            if (pb > pa) {                             // (equal ends: a duplicate breakpoint, no piece)
              total = total + tab_piece(a.n_bodies, Emax, rE0, c0, c1, disc0, disc1, dm, pa, pb);
              pa = pb;
            }
          }
          const double pw = a.n_bodies == 3 ? 1.5 : (a.n_bodies == 4 ? 3.0 : 4.5);
          val = (a.two_over_b / (((4.0 * pw) * rEm) * rE0)) * total;
        }
      }
    }
    a.out[idx] = val;
  }
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_set_nbody(int enable) {
  return __atomic_exchange_n(&g_nbody, enable ? 1 : 0, __ATOMIC_SEQ_CST);
}

extern "C" int ndpp_get_nbody(void) { return __atomic_load_n(&g_nbody, __ATOMIC_SEQ_CST); }

extern "C" int ndpp_set_nbody_tab(int enable) {
  return __atomic_exchange_n(&g_nbody_tab, enable ? 1 : 0, __ATOMIC_SEQ_CST);
}

extern "C" int ndpp_get_nbody_tab(void) { return __atomic_load_n(&g_nbody_tab, __ATOMIC_SEQ_CST); }

extern "C" void ndpp_nbody_rule(double x[32], double w[32]) {
  for (int k = 0; k < kOrder; ++k) {
    x[k] = h_x[k];
    w[k] = h_w[k];
  }
}

extern "C" int ndpp_nbody_leg_batch(const ndpp_params* p, double awr, double Q, int n_bodies, double Ap, int n_ein,
                                    const double* ein, int G, const double* e_bins, double* out, int* status) {
  return nbody_batch_sink(p, awr, Q, n_bodies, Ap, n_ein, ein, G, e_bins, out, status, nullptr);
}

int ndpp::nbody_batch_sink(const ndpp_params* p, double awr, double Q, int n_bodies, double Ap, int n_ein,
                           const double* ein, int G, const double* e_bins, double* out, int* status,
                           DeviceSink* sink) {
  int rc;
  if ((rc = check_params(p, G, kCheckOrder))) return rc;
  if (n_bodies < 3 || n_bodies > 5) return fail(NDPP_EINVAL, "nbody_leg_batch: n_bodies=%d outside 3..5", n_bodies);
  if (!(Ap > 1.0) || !(Ap <= DBL_MAX)) return fail(NDPP_EINVAL, "nbody_leg_batch: Ap=%g (need a finite Ap > 1)", Ap);
  if (!(awr > 0.0) || !(awr <= DBL_MAX)) return fail(NDPP_EINVAL, "nbody_leg_batch: awr=%g (need a finite awr > 0)", awr);
  if (!std::isfinite(Q)) return fail(NDPP_EINVAL, "nbody_leg_batch: Q=%g is not finite", Q);
  if (n_ein < 0) return fail(NDPP_EINVAL, "nbody_leg_batch: n_ein=%d (need n_ein >= 0)", n_ein);
  if (n_ein == 0) return NDPP_OK;
  if (!ein || !e_bins || (!out && !sink)) return fail(NDPP_EINVAL, "nbody_leg_batch: NULL argument");
  const int L = p->order;
  size_t out_bytes;
  if ((rc = check_gl_index("nbody_leg_batch", G, L))) return rc;
  if (!bytes_of((size_t)n_ein * G, L, sizeof(double), &out_bytes))
    return fail(NDPP_EINVAL, "nbody_leg_batch: n_ein=%d G=%d L=%d: the sizes overflow", n_ein, G, L);
  if ((rc = require_device())) return rc;

  // classify_kernel's rule: an E_in that is not a positive finite number is not integrated (zero row,
  // NDPP_ST_RANGE)
  std::vector<int> st0(n_ein, 0);
  for (int i = 0; i < n_ein; ++i)
    if (!(ein[i] > 0.0) || !(ein[i] <= DBL_MAX)) st0[i] = NDPP_ST_RANGE;
  DevBuf<double> d_ein, d_bins, d_out;
  DevBuf<int> d_st;
  NDPP_TRY(d_ein.upload(ein, n_ein));
  NDPP_TRY(d_bins.upload(e_bins, G + 1));
  NDPP_TRY(d_out.alloc((size_t)n_ein * G * L));
  NDPP_TRY(d_st.upload(st0.data(), n_ein));
  NbodyArgs a;
  a.awr = awr; a.Q = Q; a.Ap = Ap; a.two_over_b = h_two_over_b[n_bodies - 3];
  a.n_bodies = n_bodies; a.n_ein = n_ein; a.G = G;
  a.ein = d_ein.p; a.e_bins = d_bins.p; a.out = d_out.p;
  GpuSpan span(nullptr, -1);
  const long tot = (long)n_ein * G;
  dispatch_moments(L, [&](auto tag) {
    hipLaunchKernelGGL(nbody_kernel<decltype(tag)::value>, dim3(nblk(tot, kItems)), dim3(kThreads), 0, 0, a);
  });
  return finish_batch(d_out.p, d_st.p, n_ein, (size_t)G * L, 0, out, status, sink, span);
}

extern "C" int ndpp_nbody_tab_batch(const ndpp_params* p, int n_tab, double awr, double Q, int n_bodies, double Ap,
                                    int n_ein, const double* ein, int G, const double* e_bins, double* out,
                                    int* status) {
  return nbody_tab_batch_sink(p, n_tab, awr, Q, n_bodies, Ap, n_ein, ein, G, e_bins, out, status, nullptr);
}

int ndpp::nbody_tab_batch_sink(const ndpp_params* p, int n_tab, double awr, double Q, int n_bodies, double Ap,
                               int n_ein, const double* ein, int G, const double* e_bins, double* out, int* status,
                               DeviceSink* sink) {
  int rc;
  if ((rc = check_params(p, G, kCheckTab, n_tab))) return rc;
  if (n_bodies < 3 || n_bodies > 5) return fail(NDPP_EINVAL, "nbody_tab_batch: n_bodies=%d outside 3..5", n_bodies);
  if (!(Ap > 1.0) || !(Ap <= DBL_MAX)) return fail(NDPP_EINVAL, "nbody_tab_batch: Ap=%g (need a finite Ap > 1)", Ap);
  if (!(awr > 0.0) || !(awr <= DBL_MAX)) return fail(NDPP_EINVAL, "nbody_tab_batch: awr=%g (need a finite awr > 0)", awr);
  if (!std::isfinite(Q)) return fail(NDPP_EINVAL, "nbody_tab_batch: Q=%g is not finite", Q);
  if (n_ein < 0) return fail(NDPP_EINVAL, "nbody_tab_batch: n_ein=%d (need n_ein >= 0)", n_ein);
  if (n_ein == 0) return NDPP_OK;
  if (!ein || !e_bins || (!out && !sink)) return fail(NDPP_EINVAL, "nbody_tab_batch: NULL argument");
  const int N = n_tab;
  size_t out_bytes;
  if ((rc = check_gl_index("nbody_tab_batch", G, N))) return rc;
  if (!bytes_of((size_t)n_ein * G, N, sizeof(double), &out_bytes))
    return fail(NDPP_EINVAL, "nbody_tab_batch: n_ein=%d G=%d N=%d: the sizes overflow", n_ein, G, N);
  if ((rc = require_device())) return rc;

  std::vector<int> st0(n_ein, 0);
  for (int i = 0; i < n_ein; ++i)
    if (!(ein[i] > 0.0) || !(ein[i] <= DBL_MAX)) st0[i] = NDPP_ST_RANGE;
  DevBuf<double> d_ein, d_bins, d_out;
  DevBuf<int> d_st;
  NDPP_TRY(d_ein.upload(ein, n_ein));
  NDPP_TRY(d_bins.upload(e_bins, G + 1));
  NDPP_TRY(d_out.alloc((size_t)n_ein * G * N));
  NDPP_TRY(d_st.upload(st0.data(), n_ein));
  NbodyTabArgs a;
  a.awr = awr; a.Q = Q; a.Ap = Ap; a.two_over_b = h_two_over_b[n_bodies - 3];
  a.n_bodies = n_bodies; a.n_ein = n_ein; a.G = G; a.N = N;
  a.ein = d_ein.p; a.e_bins = d_bins.p; a.out = d_out.p;
  GpuSpan span(nullptr, -1);
  const long tot = (long)n_ein * G * N;
  hipLaunchKernelGGL(nbody_tab_kernel, dim3(nblk(tot, kTabThreads)), dim3(kTabThreads), 0, 0, a);
  return finish_batch(d_out.p, d_st.p, n_ein, (size_t)G * N, 0, out, status, sink, span);
}
