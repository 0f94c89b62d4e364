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

int g_nbody = 0;   // ndpp_set_nbody: process-wide

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

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_set_nbody(int enable) {
  return __atomic_exchange_n(&g_nbody, enable ? 1 : 0, __ATOMIC_SEQ_CST);
}

extern "C" int ndpp_get_nbody(void) { return __atomic_load_n(&g_nbody, __ATOMIC_SEQ_CST); }

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
