// tab_kernels.hip -- tabular scattering output: the P0 integral of every path split into N equal
// bins of the lab cosine (include/ndpp_hip.h, "tabular scattering output").
//
//   file 4 (two-body CM)     f4_tab_kernel         thread per (E_in, group), both rows blended
//   file 6 CM                f6_cm_tab_kernel      thread per (E_in, group, lab E' point), then
//                            f6_cm_tab_finish      the E' trapezoid and the normalisation
//   file 6 lab               f6_lab_tab_kernel     thread per (E_in, group), then f6_lab_tab_norm
//   law 9                    law9_tab_kernel       thread per (E_in, row, group), then the blend
//   free gas                 fg_tab_kernel         thread per (E_in, group), then fg_tab_finish
//
// The piecewise-linear paths share one device helper, tab_spread: the exact integral of a linear
// panel over each bin it spans.  A thread owns its output row (N doubles in global memory) and
// carries the current bin's sum in a register (BinAcc), so a row is read and written once per bin
// change: no per-thread array indexed by bin, no scratch.  Every row is summed by one thread in a
// fixed order, so results repeat bit for bit.
//
// Built with -DNDPP_FAST=0 -ffp-contract=off like the Legendre integrators whose inputs and P0
// these kernels share (file4_device.h, file6_device.h, ndpp_math.h's strict arithmetic).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "file4_device.h"
#include "file6_device.h"
#include "kernels.h"
#include "ndpp_math.h"

#if NDPP_FAST
#error "tab_kernels.hip must be compiled with -DNDPP_FAST=0 -ffp-contract=off"
#endif

namespace ndpp {
namespace {

// ---- bins ------------------------------------------------------------------------------------
// b_k = -1 + 2k/N; (2k)/N is one correctly rounded quotient, so edge 2k of 2N bins is edge k of N
// bins bit for bit (the refinement property holds to the rounding of the integrals alone)
__device__ __forceinline__ double tab_edge(int k, int N) {
  return k >= N ? 1.0 : -1.0 + (2.0 * (double)k) / (double)N;
}
// the bin with b_k <= mu < b_{k+1}, clamped to 0 .. N-1
__device__ __forceinline__ int tab_bin(double mu, int N) {
  int k = (int)floor((mu + 1.0) * 0.5 * (double)N);
  k = k < 0 ? 0 : (k > N - 1 ? N - 1 : k);
  if (k > 0 && mu < tab_edge(k, N)) --k;
  else if (k < N - 1 && mu >= tab_edge(k + 1, N)) ++k;
  return k;
}

// the running sum of the current bin of a thread's row
struct BinAcc {
  double* row;
  int k;
  double v;
  __device__ explicit BinAcc(double* r) : row(r), k(-1), v(0.0) {}
  __device__ __forceinline__ void add(int kk, double x) {
    if (kk != k) {
      flush();
      k = kk;
    }
    v += x;
  }
  __device__ __forceinline__ void flush() {
    if (k >= 0) row[k] += v;
    k = -1;
    v = 0.0;
  }
};

struct LabIdentity {
  __device__ __forceinline__ double operator()(double mu) const { return mu; }
};

// The mass of the linear f on the panel [xa, xb] (fa at xa, fb at xb; xa < xb), times wgt, spread
// over the lab bins.  The panel's coordinate x maps to the lab cosine monotonically: mua, mub are
// the lab cosines of its ends and inv(mu) the x of a lab cosine on this branch (LabIdentity when x
// is the lab cosine).  Each bin receives the exact integral of the linear f over the x it covers.
template <class Inv>
__device__ __forceinline__ void tab_spread(double xa, double xb, double fa, double fb, double mua, double mub, Inv inv,
                           int N, double wgt, BinAcc& acc) {
  if (!(xb > xa)) return;
  const double s = (fb - fa) / (xb - xa);
  double u = xa, fu = fa;
  int k = tab_bin(mua, N);
  if (mub >= mua) {
    for (;;) {
      const double e = tab_edge(k + 1, N);
      if (k == N - 1 || e >= mub) break;
      double xe = inv(e);
      xe = xe < u ? u : (xe > xb ? xb : xe);
      const double fe = fa + s * (xe - xa);
      acc.add(k, wgt * (0.5 * (xe - u) * (fu + fe)));
      u = xe;
      fu = fe;
      ++k;
    }
  } else {
    for (;;) {
      const double e = tab_edge(k, N);
      if (k == 0 || e <= mub) break;
      double xe = inv(e);
      xe = xe < u ? u : (xe > xb ? xb : xe);
      const double fe = fa + s * (xe - xa);
      acc.add(k, wgt * (0.5 * (xe - u) * (fu + fe)));
      u = xe;
      fu = fe;
      --k;
    }
  }
  acc.add(k, wgt * (0.5 * (xb - u) * (fu + fb)));
}
__device__ __forceinline__ void tab_spread_lab(double xa, double xb, double fa, double fb, int N, double wgt,
                                               BinAcc& acc) {
  tab_spread(xa, xb, fa, fb, xa, xb, LabIdentity(), N, wgt, acc);
}

// ---- file 4 ----------------------------------------------------------------------------------
// The lab cosine of the CM cosine w of two-body kinematics, mu = (1 + R w) / sqrt(1 + R^2 + 2 R w)
// (tolab, scattdata_header.F90:1466-1496, for R >= 1 and for w >= -R; below -R the reference's
// tolab is a linear stand-in that ends under -1, which no bin could hold, so the exact kinematics
// are used there).  d mu / d w is proportional to R + w: monotone on either side of w = -R.
__device__ __forceinline__ double f4_lab(double R, double w) {
  if (R == 1.0) return sqrt(0.5 * (1.0 + w));
  return (1.0 + R * w) / sqrt(1.0 + R * R + 2.0 * R * w);
}
// w of the lab cosine mu: branch +1 (w >= -R, mu rising with w) or -1 (w < -R, R < 1)
struct F4Inv {
  double R, sgn;
  __device__ __forceinline__ double operator()(double mu) const {
    const double d = sqrt(fmax(mu * mu + (R * R - 1.0), 0.0));
    return (sgn * mu * d - (1.0 - mu) * (1.0 + mu)) / R;
  }
};
// one piece [xa, xb] of the trapezoid sum, split at w = -R where the lab cosine turns
__device__ __forceinline__ void f4_branch(double R, double xa, double xb, double fa, double fb, double sgn, int N,
                                          BinAcc& acc) {
  tab_spread(xa, xb, fa, fb, f4_lab(R, xa), f4_lab(R, xb), F4Inv{R, sgn}, N, 1.0, acc);
}
__device__ __forceinline__ void f4_piece(double R, double xa, double xb, double fa, double fb, int N, BinAcc& acc) {
  if (!(xb > xa)) return;
  if (R < 1.0 && xa < -R && xb > -R) {
    const double fm = fa + (fb - fa) * ((-R - xa) / (xb - xa));
    f4_branch(R, xa, -R, fa, fm, -1.0, N, acc);
    f4_branch(R, -R, xb, fm, fb, 1.0, N, acc);
    return;
  }
  f4_branch(R, xa, xb, fa, fb, (R < 1.0 && xb <= -R) ? -1.0 : 1.0, N, acc);
}

// integrate_file4_cm_leg's pieces (scattdata_header.F90:986-1076, file4_device.h) with the
// blended row (1 - fb) f_lo + fb f_hi, thread per (E_in of the list, group)
__global__ __launch_bounds__(64) void f4_tab_kernel(int n, const int* list, MuGrid grid, const double* ein,
                                                    const int* row_lo, const double* w_hi,
                                                    const double* f_tab, double awr, double Q, int G, int N,
                                                    const double* e_bins, double* out) {
  const long tot = (long)n * G;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < tot; t += (long)gridDim.x * blockDim.x) {
    const int j = (int)(t / G), g = (int)(t % G);
    const int i = list ? list[j] : j;
    double* row = out + ((size_t)i * G + g) * N;
    for (int k = 0; k < N; ++k) row[k] = 0.0;
    const double Ein = ein[i];
    const F4Kin kin = file4_kin(Ein, awr, Q);
    const F4Bounds bd = file4_bounds(kin, Ein, grid.dmu_fgk, e_bins[g], e_bins[g + 1]);
    if (bd.skip) continue;
    const double R = kin.R, wlo = bd.wlo, whi = bd.whi;
    const int ilo = bd.ilo, ihi = bd.ihi;
    const double* f0 = f_tab + (size_t)row_lo[i] * grid.M;
    const double* f1 = f0 + grid.M;
    const double fb = w_hi[i], fa = 1.0 - fb;
    auto fv = [&](int iw) { return fa * f0[iw] + fb * f1[iw]; };
    const double flo = fa * file4_f_at(grid, f0, wlo, ilo) + fb * file4_f_at(grid, f1, wlo, ilo);
    const double fhi = fa * file4_f_at(grid, f0, whi, ihi) + fb * file4_f_at(grid, f1, whi, ihi);
    BinAcc acc(row);
    if (ilo != ihi) {
      f4_piece(R, wlo, grid.at(ilo), flo, fv(ilo), N, acc);
      for (int iw = ilo + 1; iw <= ihi - 1; ++iw)
        f4_piece(R, grid.at(iw - 1), grid.at(iw), fv(iw - 1), fv(iw), N, acc);
      f4_piece(R, grid.at(ihi - 1), whi, fv(ihi - 1), fhi, N, acc);
    } else {
      f4_piece(R, wlo, whi, flo, fhi, N, acc);
    }
    acc.flush();
  }
}

// ---- file 6 ----------------------------------------------------------------------------------
// CM: the mu loop of integrate_file6_cm_leg (:1186-1244) for one (E_in, group, E' point), each panel
// of the lab-cosine grid mu_l_min .. 1 spread over the bins (f6_cm_point_kernel's walk, l = 0)
__global__ __launch_bounds__(64) void f6_cm_tab_kernel(F6Batch B) {
  const long n_live = (long)*B.cm_live;
  const int N = B.L;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n_live; q += (long)gridDim.x * blockDim.x) {
    const long t = (long)B.cm_list[q];
    const int iE = (int)(t % B.NEG) + 1;
    const int g = (int)((t / B.NEG) % B.G) + 1;
    const int e = (int)(t / ((long)B.NEG * B.G));
    const UbView v = B.view(e);
    CmItem it;
    if (!f6_cm_item(B, v, e, g, iE, it)) continue;
    BinAcc acc(B.fEl + (size_t)t * N);          // zeroed by f6_cm_list_kernel
    CmCols cc;
    const int M = B.M;
    double x0 = it.mu_l_min;
    double y0 = f6_cm_fval<false>(B.grid, v, cc, it.Eo, it.c, x0, it.dup_end);
    for (int imu = 2; imu <= M; ++imu) {
      const double x1 = it.mu_l_min + it.dmu * (double)(imu - 1);
      const double y1 = f6_cm_fval<false>(B.grid, v, cc, it.Eo, it.c, x1, it.dup_end);
      if (!(x1 - x0 < 1e-14)) tab_spread_lab(x0, x1, y0, y1, N, 1.0, acc);   // legendre.F90:44
      x0 = x1;
      y0 = y1;
    }
    acc.flush();
  }
}

// the E' trapezoid (:1246-1258) per bin and the normalisation by the sum over groups and bins
__global__ void f6_cm_tab_finish(F6Batch B) {
  const int N = B.L;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B.n_ein; e += gridDim.x * blockDim.x) {
    double* o = B.out + (size_t)e * B.G * N;
    for (int k = 0; k < B.G * N; ++k) o[k] = 0.0;
    const int g_lo = B.glohi[2 * e], g_hi = B.glohi[2 * e + 1];
    const double* Eb = B.ebnds + (size_t)e * (B.G + 2);
    double s = 0.0;
    for (int g = g_lo; g <= g_hi; ++g) {
      const double dEo = (Eb[g + 1] - Eb[g]) / (double)(B.NEG - 1);
      double* dg = o + (size_t)(g - 1) * N;
      for (int iE = 1; iE <= B.NEG; ++iE) {
        const double* fEl = B.fEl + (((size_t)e * B.G + (g - 1)) * B.NEG + (iE - 1)) * N;
        const double w = ((iE != 1) && (iE != B.NEG)) ? 2.0 : 1.0;
        for (int k = 0; k < N; ++k) dg[k] = dg[k] + w * fEl[k];
      }
      for (int k = 0; k < N; ++k) {
        dg[k] = dg[k] * dEo * 0.5;
        s = s + dg[k];
      }
    }
    if (s > 0.0) s = 1.0 / s;
    for (int g = g_lo; g <= g_hi; ++g)
      for (int k = 0; k < N; ++k) o[(size_t)(g - 1) * N + k] *= s;
  }
}

// lab: the M-1 panels of each group's fint (:1421-1425)
__global__ __launch_bounds__(64) void f6_lab_tab_kernel(F6Batch B) {
  const long tot = (long)B.n_ein * B.G;
  const int N = B.L;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < tot; t += (long)gridDim.x * blockDim.x) {
    const int g = (int)(t % B.G), e = (int)(t / B.G);
    double* row = B.out + (size_t)t * N;
    for (int k = 0; k < N; ++k) row[k] = 0.0;
    if (B.ebnds[(size_t)e * (B.G + 2) + g] == 0.0) continue;
    const double* fint = B.fEl + (size_t)t * B.M;
    BinAcc acc(row);
    double x0 = B.grid.at(0), y0 = fint[0];
    for (int imu = 1; imu <= B.M - 1; ++imu) {
      const double x1 = B.grid.at(imu), y1 = fint[imu];
      if (!(x1 - x0 < 1e-14)) tab_spread_lab(x0, x1, y0, y1, N, 1.0, acc);
      x0 = x1;
      y0 = y1;
    }
    acc.flush();
  }
}

// f_lo = ONE / sum(distro(1,:)) (:1447-1448) with each group's P0 the sum of its bins; the group
// sum compensated like flang's SUM (f6_lab_norm_kernel)
__global__ void f6_lab_tab_norm(F6Batch B) {
  const int N = B.L;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B.n_ein; e += gridDim.x * blockDim.x) {
    double* o = B.out + (size_t)e * B.G * N;
    KahanSum sum;
    for (int g = 0; g < B.G; ++g) {
      double p0 = 0.0;
      for (int k = 0; k < N; ++k) p0 += o[(size_t)g * N + k];
      sum.add(p0);
    }
    const double f_lo = 1.0 / sum.s;
    for (int k = 0; k < B.G * N; ++k) o[k] = o[k] * f_lo;
  }
}

// ---- law 9 -----------------------------------------------------------------------------------
// law9_scatter_lab_leg (:1274-1326), l = 0, per bin: thread per (E_in, row, group) into
// raw[n_ein][2][G][N]
__global__ __launch_bounds__(64) void law9_tab_kernel(int n_ein, const double* ein, const int* row_lo, MuGrid grid,
                                                      const double* f_tab, const double* edata, int G, int N,
                                                      const double* e_bins, double* raw) {
  const long tot = (long)n_ein * 2 * G;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < tot; t += (long)gridDim.x * blockDim.x) {
    const int g = (int)(t % G), r = (int)((t / G) % 2), e = (int)(t / (2L * G));
    double* row = raw + (size_t)t * N;
    for (int k = 0; k < N; ++k) row[k] = 0.0;
    const double Ein = ein[e];
    const double* fmu = f_tab + (size_t)(row_lo[e] + r) * grid.M;
    double pE;
    if (!law9_group(edata, tab1(edata, Ein), Ein, e_bins[g], e_bins[g + 1], pE)) continue;
    BinAcc acc(row);
    double x0 = grid.at(0), y0 = fmu[0];
    for (int imu = 1; imu <= grid.M - 1; ++imu) {
      const double x1 = grid.at(imu), y1 = fmu[imu];
      if (!(x1 - x0 < 1e-14)) tab_spread_lab(x0, x1, y0, y1, N, pE, acc);
      x0 = x1;
      y0 = y1;
    }
    acc.flush();
  }
}

// ---- free gas --------------------------------------------------------------------------------
// calc_fgk (freegas.F90:415-473) at l = 0 for the two bracketing rows at once: only f(mu) depends
// on the row
struct FgNode {
  double Ein, Eout, lterm, s2, AkT, beta;
};
__device__ __forceinline__ FgNode fg_node(double A, double kT, double Ein, double Eout) {
  FgNode q;
  q.Ein = Ein;
  q.Eout = Eout;
  const double r = (A + 1.0) / A;
  q.lterm = sqrt(Eout / Ein) / kT * (r * r);
  q.s2 = sqrt(Ein * Eout);
  q.AkT = A * kT;
  q.beta = (Eout - Ein) / kT;
  return q;
}
__device__ __forceinline__ void fg_k0(const FgNode& q, const MuGrid& grid, const double* f0, const double* f1,
                                      double mu, double& k0, double& k1) {
  int i;                                         // 1-based, as the reference
  if (mu <= -1.0) i = 1;
  else if (mu >= 1.0) i = grid.M - 1;
  else i = (int)((mu + 1.0) / grid.dmu_fgk) + 1;
  if (i > grid.M - 1) i = grid.M - 1;
  const double interp = (mu - grid.at(i - 1)) / (grid.at(i) - grid.at(i - 1));
  const double v0 = (1.0 - interp) * f0[i - 1] + interp * f0[i];
  const double v1 = (1.0 - interp) * f1[i - 1] + interp * f1[i];
  double alpha = (q.Ein + q.Eout - 2.0 * mu * q.s2) / q.AkT;
  if (alpha < 1.0E-6) alpha = 1.0E-6;
  const double t = alpha + q.beta;
  const double arg = -(t * t) / (4.0 * alpha);
  if (arg <= -708.0) {
    k0 = 0.0;
    k1 = 0.0;
    return;
  }
  const double c = q.lterm * exp(arg) / sqrt(kFourPi * alpha);
  k0 = v0 * c;
  k1 = v1 * c;
}

// Gauss-Legendre, 8 points on [-1, 1]
__constant__ double kGlX[4] = {0.18343464249564980494, 0.52553240991632898582, 0.79666647741362673959,
                               0.96028985649753623168};
__constant__ double kGlW[4] = {0.36268378337836198297, 0.31370664587788728734, 0.22238103445337447054,
                               0.10122853629037625915};
constexpr int kFgMuPieces = 16;   // equal pieces of [mu_lo, mu_hi] (further split at the bin edges)
constexpr int kFgMaxDoublings = 7; // E' panels per piece: 1, 2, ..., 128
constexpr double kFgRelTol = 1e-10;
// plus an absolute floor: the kernel integrates to ~1 over (E', mu), so 1e-13 is 1e-13 of a
// normalised row -- without it the tails, whose estimates are rounding noise around 0, never settle
constexpr double kFgAbsTol = 1e-13;

struct FgTab {
  int n, G, N;
  const int* list;
  const double* ein;
  const int* row_lo;
  const double* f_tab;
  const double* e_bins;
  double A, kT, sab_threshold, brent_thresh;
  MuGrid grid;
  double* ws;        // [n][G][3][2][N]: result, coarse, fine (rows lo, hi)
  int* status;       // [n_ein] of the call (indexed by E_in, not by list position)
};

// the mu integral at one E' (find_FG_mu's range, split at the bin edges), times wgt, into rows
// r0 / r1 (lo / hi).  The kernel goes like 1 / sqrt(alpha) and alpha, linear in mu, is smallest at
// mu = 1, where it vanishes as E' -> E_in: in t = sqrt(mu_hi - mu) (mu = mu_hi - t^2, dmu = 2t dt)
// that end is smooth.  Equal pieces in t, further split where t crosses a bin edge; t rising is
// mu falling, so the bins are walked downwards.
__device__ __forceinline__ void fg_tab_mu(const FgTab& P, const double* f0, const double* f1, double Ein, double Eout, double wgt,
                          double* r0, double* r1) {
  const FgNode q = fg_node(P.A, P.kT, Ein, Eout);
  const FgPair pr = make_pair(P.A, P.kT, Ein, Eout);
  double mlo, mhi;
  fg_find_mu(pr, P.A, Ein, Eout, P.sab_threshold, P.brent_thresh, mlo, mhi);
  if (!(mhi > mlo)) return;
  const int N = P.N;
  const double tmax = sqrt(mhi - mlo);
  const double h = tmax / (double)kFgMuPieces;
  BinAcc a0(r0), a1(r1);
  double u = 0.0;
  int k = tab_bin(mhi, N), j = 1;
  if (k > 0 && mhi == tab_edge(k, N)) --k;       // mu just below mu_hi
  while (j <= kFgMuPieces) {
    const double s_next = (j == kFgMuPieces) ? tmax : (double)j * h;
    const double e = tab_edge(k, N);
    const double e_next = (k > 0 && e > mlo) ? sqrt(mhi - e) : 2.0 * tmax + 1.0;
    const bool at_edge = e_next < s_next;
    const double v = at_edge ? e_next : s_next;
    if (v > u) {
      const double c = 0.5 * (u + v), r = 0.5 * (v - u);
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const double ta = c - r * kGlX[m], tb = c + r * kGlX[m];
        double ka0, ka1, kb0, kb1;
        fg_k0(q, P.grid, f0, f1, mhi - ta * ta, ka0, ka1);
        fg_k0(q, P.grid, f0, f1, mhi - tb * tb, kb0, kb1);
        s0 += kGlW[m] * (ta * ka0 + tb * kb0);
        s1 += kGlW[m] * (ta * ka1 + tb * kb1);
      }
      a0.add(k, 2.0 * wgt * r * s0);
      a1.add(k, 2.0 * wgt * r * s1);
    }
    u = v;
    if (at_edge) --k;
    else ++j;
  }
  a0.flush();
  a1.flush();
}

// composite Gauss-Legendre over [a, b] in E' with P panels into rows dst (2N, zeroed here)
__device__ __forceinline__ void fg_tab_eout(const FgTab& P, const double* f0, const double* f1, double Ein, double a, double b, int Pn,
                            double* dst) {
  const int N = P.N;
  for (int k = 0; k < 2 * N; ++k) dst[k] = 0.0;
  const double hp = (b - a) / (double)Pn;
  for (int ip = 0; ip < Pn; ++ip) {
    const double lo = a + (double)ip * hp, hi = (ip == Pn - 1) ? b : a + (double)(ip + 1) * hp;
    const double c = 0.5 * (lo + hi), r = 0.5 * (hi - lo);
    for (int m = 0; m < 4; ++m) {
      fg_tab_mu(P, f0, f1, Ein, c - r * kGlX[m], r * kGlW[m], dst, dst + N);
      fg_tab_mu(P, f0, f1, Ein, c + r * kGlX[m], r * kGlW[m], dst, dst + N);
    }
  }
}

// one E' piece: panels doubled until every bin of both rows has settled (the vector-valued error
// test), then added to the result rows.  Returns false when kFgMaxDoublings did not settle it (the
// finest estimate is kept; the caller flags the row NDPP_ST_TAB_UNSETTLED).
__device__ __forceinline__ bool fg_tab_piece(const FgTab& P, const double* f0, const double* f1, double Ein, double a, double b,
                             double* res, double* wa, double* wb) {
  if (!(b > a)) return true;
  bool settled = false;
  const int N = P.N;
  fg_tab_eout(P, f0, f1, Ein, a, b, 1, wa);
  for (int d = 1; d <= kFgMaxDoublings; ++d) {
    fg_tab_eout(P, f0, f1, Ein, a, b, 1 << d, wb);
    double err0 = 0.0, err1 = 0.0, tot0 = 0.0, tot1 = 0.0;
    for (int k = 0; k < N; ++k) {
      err0 = fmax(err0, fabs(wb[k] - wa[k]));
      err1 = fmax(err1, fabs(wb[N + k] - wa[N + k]));
      tot0 += fabs(wb[k]);
      tot1 += fabs(wb[N + k]);
    }
    double* t = wa;
    wa = wb;
    wb = t;
    if (err0 <= kFgRelTol * tot0 + kFgAbsTol && err1 <= kFgRelTol * tot1 + kFgAbsTol) {
      settled = true;
      break;
    }
  }
  for (int k = 0; k < 2 * N; ++k) res[k] += wa[k];
  return settled;
}

// integrate_freegas_leg's E' pieces (freegas.F90:40-131) for one (E_in, group)
__global__ __launch_bounds__(64) void fg_tab_kernel(FgTab P) {
  const long tot = (long)P.n * P.G;
  const int N = P.N;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < tot; t += (long)gridDim.x * blockDim.x) {
    const int j = (int)(t / P.G), g = (int)(t % P.G);
    const int i = P.list[j];
    double* res = P.ws + (size_t)t * 6 * N;
    double* wa = res + 2 * N;
    double* wb = res + 4 * N;
    for (int k = 0; k < 2 * N; ++k) res[k] = 0.0;
    const double Ein = P.ein[i], A = P.A, kT = P.kT;
    const double* f0 = P.f_tab + (size_t)P.row_lo[i] * P.grid.M;
    const double* f1 = f0 + P.grid.M;
    double alphaEin = (A - 1.0) / (A + 1.0);
    alphaEin = alphaEin * alphaEin * Ein;
    double Eout_lo, Eout_hi;
    fg_eout_bounds(A, kT, Ein, Eout_lo, Eout_hi);
    const double Eg = P.e_bins[g], Eg1 = P.e_bins[g + 1];
    bool ok = true;
    if ((Eg < Eout_hi) && (Eg1 > Eout_lo)) {
      double Elo = (Eout_lo > Eg) ? Eout_lo : Eg;
      const double Ehi = (Eout_hi < Eg1) ? Eout_hi : Eg1;
      const double Ebottom = (Eg == 0.0) ? 0.01 * Elo : Eg;
      ok &= fg_tab_piece(P, f0, f1, Ein, Ebottom, Elo, res, wa, wb);
      ok &= fg_tab_piece(P, f0, f1, Ein, Ehi, Eg1, res, wa, wb);
      if ((Elo < alphaEin) && (alphaEin < Ehi)) {
        ok &= fg_tab_piece(P, f0, f1, Ein, Elo, alphaEin, res, wa, wb);
        Elo = alphaEin;
      }
      if ((Elo < Ein) && (Ein < Ehi)) {
        ok &= fg_tab_piece(P, f0, f1, Ein, Elo, Ein, res, wa, wb);
        Elo = Ein;
      }
      ok &= fg_tab_piece(P, f0, f1, Ein, Elo, Ehi, res, wa, wb);
    } else {
      ok &= fg_tab_piece(P, f0, f1, Ein, Eg, Eg1, res, wa, wb);
    }
    if (!ok) atomicOr(P.status + i, NDPP_ST_TAB_UNSETTLED);
  }
}

// per E_in: each row normalised to sum_{g,k} = 1 (distro / p0_1g_norm, freegas.F90:143), then
// blended (1-f)*lo + f*hi
__global__ void fg_tab_finish(FgTab P, const double* w_hi, double* out) {
  const int N = P.N, G = P.G;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < P.n; j += gridDim.x * blockDim.x) {
    const int i = P.list[j];
    const double* ws = P.ws + (size_t)j * G * 6 * N;
    double s0 = 0.0, s1 = 0.0;
    for (int g = 0; g < G; ++g)
      for (int k = 0; k < N; ++k) {
        s0 += ws[(size_t)g * 6 * N + k];
        s1 += ws[(size_t)g * 6 * N + N + k];
      }
    const double f = w_hi[i];
    double* o = out + (size_t)i * G * N;
    for (int g = 0; g < G; ++g)
      for (int k = 0; k < N; ++k) {
        const double r = (1.0 - f) * (ws[(size_t)g * 6 * N + k] / s0);
        o[(size_t)g * N + k] = r + f * (ws[(size_t)g * 6 * N + N + k] / s1);
      }
  }
}

}  // namespace

void launch_law9_tab(int n_ein, const double* ein, const int* row_lo, int mu_bins, const double* f_tab,
                     const double* edata, int G, int N, const double* e_bins, double* raw) {
  hipLaunchKernelGGL(law9_tab_kernel, dim3(nblk((long)n_ein * 2 * G, 64)), dim3(64), 0, 0, n_ein, ein, row_lo,
                     make_mu_grid(mu_bins), f_tab, edata, G, N, e_bins, raw);
}

void launch_f6_tab(const F6Batch& B) {
  if (B.frame_cm) {
    const long tot = (long)B.n_ein * B.G * B.NEG;
    hipLaunchKernelGGL(f6_cm_list_kernel, dim3(nblk(tot, 256)), dim3(256), 0, 0, B);
    hipLaunchKernelGGL(f6_cm_tab_kernel, dim3(nblk(tot, 64)), dim3(64), 0, 0, B);
    hipLaunchKernelGGL(f6_cm_tab_finish, dim3(nblk(B.n_ein, 64)), dim3(64), 0, 0, B);
  } else {
    hipLaunchKernelGGL(f6_lab_tab_kernel, dim3(nblk((long)B.n_ein * B.G, 64)), dim3(64), 0, 0, B);
    hipLaunchKernelGGL(f6_lab_tab_norm, dim3(nblk(B.n_ein, 64)), dim3(64), 0, 0, B);
  }
}

int elastic_tab_batch_sink(const ndpp_params* p, double A, double kT, double freegas_cutoff, double Q, int n_ein,
                           const double* ein, const int* row_lo, const double* w_hi, int n_rows,
                           const double* f_tab, int G, const double* e_bins, int n_tab, double* out, int* status,
                           DeviceSink* sink) {
  int rc = check_params(p, G, kCheckTab, n_tab);
  if (rc) return rc;
  if (n_ein < 0 || n_rows < 2) return fail(NDPP_EINVAL, "n_ein=%d n_rows=%d", n_ein, n_rows);
  if (n_ein == 0) return NDPP_OK;
  if (!ein || !row_lo || !w_hi || !f_tab || !e_bins || (!out && !sink)) return fail(NDPP_EINVAL, "NULL argument");
  if ((rc = check_row_lo(n_ein, row_lo, n_rows)) || (rc = require_device())) return rc;
  const int N = n_tab, M = p->mu_bins;
  const size_t GN = (size_t)G * N;
  // classify_kernel's rule: an E_in that is not a positive finite number is not integrated (zero
  // row, NDPP_ST_RANGE); below the cutoff free gas, the rest file 4
  std::vector<int> fg, f4, st0(n_ein, 0);
  for (int i = 0; i < n_ein; ++i) {
    if (!(ein[i] > 0.0) || !(ein[i] <= DBL_MAX)) st0[i] = NDPP_ST_RANGE;
    else (ein[i] < freegas_cutoff ? fg : f4).push_back(i);
  }
  BatchInputs in;
  if ((rc = in.upload(n_ein, ein, w_hi, row_lo, (size_t)n_rows * M, f_tab, G, e_bins))) return rc;
  DevBuf<double> d_out, d_ws;
  DevBuf<int> d_st, d_fg, d_f4;
  NDPP_TRY(d_out.alloc((size_t)n_ein * GN));
  NDPP_TRY(hipMemsetAsync(d_out.p, 0, sizeof(double) * n_ein * GN, 0));
  NDPP_TRY(d_st.upload(st0.data(), n_ein));
  const MuGrid grid = make_mu_grid(M);
  GpuSpan span(nullptr, kProfFile4);
  if (!f4.empty()) {
    NDPP_TRY(d_f4.upload(f4.data(), f4.size()));
    const long tot = (long)f4.size() * G;
    hipLaunchKernelGGL(f4_tab_kernel, dim3(nblk(tot, 64)), dim3(64), 0, 0, (int)f4.size(), d_f4.p, grid, in.ein.p,
                       in.row_lo.p, in.w_hi.p, in.f_tab.p, A, Q, G, N, in.e_bins.p, d_out.p);
  }
  if (!fg.empty()) {
    NDPP_TRY(d_fg.upload(fg.data(), fg.size()));
    NDPP_TRY(d_ws.alloc(fg.size() * GN * 6));
    FgTab P;
    P.n = (int)fg.size(); P.G = G; P.N = N; P.list = d_fg.p; P.ein = in.ein.p; P.row_lo = in.row_lo.p;
    P.f_tab = in.f_tab.p; P.e_bins = in.e_bins.p; P.A = A; P.kT = kT; P.sab_threshold = p->sab_threshold;
    P.brent_thresh = p->brent_mu_thresh; P.grid = grid; P.ws = d_ws.p; P.status = d_st.p;
    hipLaunchKernelGGL(fg_tab_kernel, dim3(nblk((long)P.n * G, 64)), dim3(64), 0, 0, P);
    hipLaunchKernelGGL(fg_tab_finish, dim3(nblk(P.n, 64)), dim3(64), 0, 0, P, in.w_hi.p, d_out.p);
  }
  return finish_batch(d_out.p, d_st.p, n_ein, GN, 0, out, status, sink, span);
}

}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_elastic_tab_batch(const ndpp_params* p, int n_tab, double A, double kT, double freegas_cutoff,
                                      double Q, int n_ein, const double* ein, const int* row_lo, const double* w_hi,
                                      int n_rows, const double* f_tab, int G, const double* e_bins, double* out,
                                      int* status, ndpp_stats* stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  return elastic_tab_batch_sink(p, A, kT, freegas_cutoff, Q, n_ein, ein, row_lo, w_hi, n_rows, f_tab, G, e_bins,
                                n_tab, out, status, nullptr);
}

extern "C" int ndpp_file6_tab_batch(const ndpp_params* p, int n_tab, double awr, int frame_cm, int n_ein,
                                    const double* ein, const int* row_lo, int n_rows, const double* e_grid,
                                    const int* row_ptr, const double* eout, const double* pdf, const int* intt,
                                    const double* f, int G, const double* e_bins, double* out, int* status) {
  if (n_tab < 1 || n_tab > NDPP_MAX_TAB_BINS)
    return fail(NDPP_EINVAL, "n_tab=%d outside 1..%d", n_tab, NDPP_MAX_TAB_BINS);
  if (!p) return fail(NDPP_EINVAL, "params is NULL");
  return file6_batch_sink(p, awr, frame_cm, n_ein, ein, row_lo, n_rows, e_grid, row_ptr, eout, pdf, intt, f, G,
                          e_bins, n_tab, out, status, nullptr);
}

extern "C" int ndpp_law9_tab_batch(const ndpp_params* p, int n_tab, int n_ein, const double* ein, const int* row_lo,
                                   const double* w_hi, int n_rows, const double* f_tab, int n_edata,
                                   const double* edata, int G, const double* e_bins, double* out, int* status) {
  if (n_tab < 1) return check_params(p, G, kCheckTab, n_tab);     // (n_tab = 0 would ask the sink for moments)
  return law9_batch_sink(p, n_ein, ein, row_lo, w_hi, n_rows, f_tab, n_edata, edata, G, e_bins, n_tab, out, status,
                         nullptr);
}
