// minimum_row.h -- the certified minimum of ONE row, shared by minimum_kernels.hip (one row per
// (E_in, group), ndpp_scatt_minimum) and repair_kernels.hip (the same search on a filtered row, many
// times per row, ndpp_scatt_repair).  For a row of NM stored moments an enclosure
//   lo <= min over [-1, 1] of f <= hi,   f(mu) = sum_{l < NM} c_l P_l(mu),   c_l = (l + 1/2) a_l,
// where hi = f(mu_at) is an attained value.  Definition and classes are in ndpp_hip.h; why the bound
// holds is argued in DESIGN.md section 15.
//
// The bound: on [a, a + h], f >= min(f(a), f(a + h)) - q(h), q(h) = M2 h^2 / 8, with
// M2 = sum_{l >= 2} |c_l| (l-1) l (l+1) (l+2) / 8 >= max |f''|.
//
// One thread per row, its c_l in VGPRs.  Per row:
//   1. f at the 65 nodes of 64 equal panels.  The nodes are the same for every lane, so the host-built
//      P_l(node) is read by scalar loads.  hi = the smallest node value.
//   2. the nodes once more (keeping 65 values would cost 130 VGPRs): a panel whose bound is within
//      the tolerance of hi is discarded, the others are marked in a 64-bit mask.
//   3. the marked panels are refined depth first WITHOUT a stack: the state is the interval (a, h), its
//      level, the path bits from the panel down, and f at both ends.  A discarded interval with an
//      even path steps to its right sibling, whose left end is the right end just left (f carried) and
//      whose right end is evaluated afresh; an odd one climbs.  A kept interval evaluates its midpoint
//      and descends to the left half.  Every trip of the loop makes exactly one evaluation of f at
//      ONE call site (lanes of a wave are in different states; two call sites would serialise), and
//      the loop is bounded by the evaluation counter, not by convergence.
// a, h and the midpoints are dyadic rationals of at most 51 bits: every interval end is exact.
//
// Both units are built -DNDPP_FAST=0 -ffp-contract=off in every build: + - * / and comparisons in the
// order written, so two calls return the same bits.
#pragma once
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "kernels.h"

namespace ndpp {

constexpr int kPanels = 64;                // first pass: 64 equal panels, 65 nodes
constexpr double kPanelWidth = 2.0 / kPanels;
constexpr int kMaxDepth = 45;              // levels below the panels: h >= 2^-50, ends stay exact
// Subdivision stops this far below the cap: what may still follow is one right-sibling evaluation per
// level on the way up (<= kMaxDepth) and two end evaluations for each panel not yet begun (<= 128).
constexpr int kEvalReserve = 256;
constexpr int kEvalStop = NDPP_MIN_MAX_EVALS - kEvalReserve;
static_assert(kMaxDepth + 2 * kPanels <= kEvalReserve, "the reserve covers the way out");

// P_l(x) by P_{l+1} = ((2l+1) x P_l - l P_{l-1}) / (l+1), f summed in ascending l
template <int NM>
__host__ __device__ inline double eval_f(const double (&c)[NM], double x) {
  double f = c[0];
  if (NM > 1) {
    double pm = 1.0, p = x;
    f = f + c[1 % NM] * x;
#pragma unroll
    for (int l = 1; l + 1 < NM; ++l) {
      const double pn = ((double)(2 * l + 1) * x * p - (double)l * pm) / (double)(l + 1);
      f = f + c[l + 1] * pn;
      pm = p;
      p = pn;
    }
  }
  return f;
}

// the same sum with P_l(node) from the host's table (the recurrence above, so the same bits)
template <int NM>
__host__ __device__ inline double eval_node(const double (&c)[NM], const double* __restrict__ b) {
  double f = c[0] * b[0];
#pragma unroll
  for (int l = 1; l < NM; ++l) f = f + c[l] * b[l];
  return f;
}

// one examined row: the enclosure, the class and the evaluations made (file header, steps 1-3)
template <int NM>
__host__ __device__ inline void minimum_row(const double* __restrict__ row, double rel_tol,
                                            const double* __restrict__ basis, double* p_lo, double* p_hi,
                                            double* p_mu, int* p_cls, int* p_evals) {
  double lo = 0.0, hi = 0.0, mu_at = 0.0;
  int cls = -1, evals = 0;
  double c[NM];
  double S = 0.0, M2 = 0.0;
  bool finite = true;
#pragma unroll
  for (int l = 0; l < NM; ++l) {
    const double a = row[l];
    finite = finite && (fabs(a) <= DBL_MAX);
    c[l] = ((double)l + 0.5) * a;
    S = S + fabs(c[l]);
    if (l >= 2) M2 = M2 + fabs(c[l]) * ((double)((l - 1) * l * (l + 1) * (l + 2)) / 8.0);
  }
  if (!finite || !(S <= DBL_MAX) || !(M2 <= DBL_MAX)) {     // (also a row whose S or M2 overflows)
    lo = hi = NAN;
    cls = NDPP_MIN_NONFINITE;
  } else {
    const double tolS = rel_tol * S, E = 256.0 * DBL_EPSILON * S;
    // 1. the nodes: hi and its cosine (the first node attaining it)
    hi = INFINITY;
    int jmin = 0;
    for (int j = 0; j <= kPanels; ++j) {
      const double f = eval_node<NM>(c, basis + (size_t)j * NM);
      if (f < hi) { hi = f; jmin = j; }
    }
    mu_at = -1.0 + (double)jmin * kPanelWidth;
    // 2. the panels: discard (the bound enters minb) or mark
    double minb = INFINITY;
    unsigned long long mask = 0;
    const double q0 = M2 * kPanelWidth * kPanelWidth * 0.125;
    double fl = eval_node<NM>(c, basis);
    for (int j = 0; j < kPanels; ++j) {
      const double fr = eval_node<NM>(c, basis + (size_t)(j + 1) * NM);
      const double m = fl < fr ? fl : fr;
      if ((m - hi) + tolS >= q0) {
        const double b = m - q0;
        if (b < minb) minb = b;
      } else {
        mask |= 1ull << j;
      }
      fl = fr;
    }
    evals = 2 * (kPanels + 1);
    // 3. the marked panels, depth first without a stack
    bool unsettled = false, done = (mask == 0), fresh = true, carry = false;
    bool running = false;                // an interval (a, h, fa, fb) is in hand
    double a = 0.0, h = kPanelWidth, fa = 0.0, fb = 0.0;
    int lev = 0;
    unsigned long long path = 0;
    while (!done && evals < NDPP_MIN_MAX_EVALS) {
      double x = 0.0;
      int what = 0;                      // the evaluation is: 0 a panel's left end, 1 a right end, 2 a midpoint
      if (running) {
        const double q = M2 * h * h * 0.125;
        const double m = fa < fb ? fa : fb;
        const bool ok = (m - hi) + tolS >= q;
        if (ok || lev == kMaxDepth || evals >= kEvalStop) {
          const double b = m - q;
          if (b < minb) minb = b;
          if (!ok) unsettled = true;
          while (lev > 0 && (path & 1ull)) { a = a - h; h = h * 2.0; path >>= 1; --lev; }
          if (lev == 0) {                // this panel is finished
            running = false;
            fresh = true;
            carry = true;                // fb is f at a + h, the panel's right end
            if (mask == 0) { done = true; break; }
          } else {                       // right sibling: its left end is the right end just left
            a = a + h;
            path |= 1ull;
            fa = fb;
            x = a + h;
            what = 1;
          }
        } else {
          x = a + 0.5 * h;
          what = 2;
        }
      }
      if (!running) {
        if (fresh) {                     // begin the next marked panel
          const int j = __builtin_ffsll((long long)mask) - 1;
          mask &= mask - 1ull;
          const double an = -1.0 + (double)j * kPanelWidth;
          const bool adjacent = carry && an == a + h;
          a = an;
          h = kPanelWidth;
          lev = 0;
          path = 0;
          fresh = false;
          if (adjacent) { fa = fb; x = a + h; what = 1; }
          else { x = a; what = 0; }
        } else {                         // left end known, now the right end
          x = a + h;
          what = 1;
        }
      }
      const double f = eval_f<NM>(c, x);
      ++evals;
      if (what == 0) {
        fa = f;
      } else if (what == 1) {
        fb = f;
        running = true;
      } else {
        if (f < hi) { hi = f; mu_at = x; }
        fb = f;
        h = h * 0.5;
        ++lev;
        path <<= 1;
      }
    }
    if (!done) {                         // cannot happen (kEvalReserve); |f| <= S holds regardless
      minb = -S;
      unsettled = true;
    }
    lo = (minb < hi ? minb : hi) - E;
    cls = lo >= 0.0 ? NDPP_MIN_POSITIVE : (hi < 0.0 ? NDPP_MIN_NEGATIVE : NDPP_MIN_UNDECIDED);
    if (unsettled) cls |= NDPP_MIN_UNSETTLED;
  }
  *p_lo = lo;
  *p_hi = hi;
  *p_mu = mu_at;
  *p_cls = cls;
  *p_evals = evals;
}

// P_l(node j), l < nm, by eval_f's recurrence
inline std::vector<double> node_basis(int nm) {
  std::vector<double> b((size_t)(kPanels + 1) * nm);
  for (int j = 0; j <= kPanels; ++j) {
    const double x = -1.0 + (double)j * kPanelWidth;
    double* p = &b[(size_t)j * nm];
    p[0] = 1.0;
    if (nm > 1) p[1] = x;
    for (int l = 1; l + 1 < nm; ++l)
      p[l + 1] = ((double)(2 * l + 1) * x * p[l] - (double)l * p[l - 1]) / (double)(l + 1);
  }
  return b;
}

// minimum_kernels.hip: ndpp_scatt_minimum's kernel on a matrix that is on the device already (null
// stream, nothing waited for).  basis: node_basis(n_moments) on the device; evals may be null.
void launch_minimum(int n_ein, int G, int L, int n_moments, const double* mat, double rel_tol, const double* basis,
                    double* lo, double* hi, double* mu_at, int* cls, int* evals);

}  // namespace ndpp
