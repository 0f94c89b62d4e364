// file6_kernels.hip -- correlated energy-angle (ENDF file 6) scattering moments:
// unit-base interpolation between two tabulated incoming energies fused into the
// CM->lab (integrate_file6_cm_leg) and lab (integrate_file6_lab_leg) integrators,
// and the law-9 evaporation kernel.  Reference: scattdata_header.F90:1085-1450,
// :1521-1717.
//
// Always built with -DNDPP_FAST=0 -ffp-contract=off and written so that every
// output element is accumulated by ONE thread in the reference's order.  Everything but the
// panel integrals of (piecewise-linear f) x P_l follows the Fortran operation by operation;
// those come from Legendre identities (legendre_int.h) instead of the reference's per-order
// closed forms, so results agree with the Fortran to rounding (~1e-15 of a row's largest
// moment), not bit for bit.
// The reference materialises fEmu(M, |ub|) per incoming energy (1.6 MB at
// M=2001, |ub|~100, scattdata_header.F90:1651); here only the per-column
// interpolation coefficients are stored and the column values are recombined
// on the fly from the two tabulated rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "file6_device.h"
#include "kernels.h"
#include "ndpp_math.h"
#include "legendre_int.h"

#if NDPP_FAST
#error "file6_kernels.hip must be compiled with -DNDPP_FAST=0 -ffp-contract=off"
#endif

namespace ndpp {
namespace {

// (the shared stages -- unit base, CM bounds and item list, lab sums, status -- are in
// file6_device.h: the tabular kernels of tab_kernels.hip run them too)


template <int LMAX>
__global__ __launch_bounds__(64) void f6_cm_point_kernel(F6Batch B) {
  const long n_live = (long)*B.cm_live;
  for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < n_live;
       k += (long)gridDim.x * blockDim.x) {
    const long t = (long)B.cm_list[k];
    const int iE = (int)(t % B.NEG) + 1;
    const int g = (int)((t / B.NEG) % B.G) + 1;
    const int e = (int)(t / ((long)B.NEG * B.G));
    double* dst = B.fEl + (size_t)t * B.L;
    const UbView v = B.view(e);
    CmItem it;
    if (!f6_cm_item(B, v, e, g, iE, it)) continue;     // (never: the list holds live items)
    const int M = B.M;
    double acc[LMAX];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) acc[l] = 0.0;
    LinearLegendre<LMAX> walk;       // the M-1 panel integrals, :1240-1244
    CmCols cc;
    auto mu_at = [&](int imu) { return it.mu_l_min + it.dmu * (double)(imu - 1); };
    constexpr bool kRef = LMAX > 8;
    walk.start(mu_at(1), f6_cm_fval<kRef>(B.grid, v, cc, it.Eo, it.c, mu_at(1), it.dup_end));
    const double rh = 1.0 / it.dmu;     // (unused where dmu < 1e-14: those panels contribute nothing)
    int imu = 2;
    for (; imu + 1 <= M; imu += 2) {
      const double x1 = mu_at(imu), x2 = mu_at(imu + 1);
      const double f1 = f6_cm_fval<kRef>(B.grid, v, cc, it.Eo, it.c, x1, it.dup_end);
      const double f2 = f6_cm_fval<kRef>(B.grid, v, cc, it.Eo, it.c, x2, it.dup_end);
      walk.panel2_add(x1, f1, x2, f2, rh, acc);
    }
    if (imu <= M) {
      const double x1 = mu_at(imu);
      walk.panel_add(x1, f6_cm_fval<kRef>(B.grid, v, cc, it.Eo, it.c, x1, it.dup_end), acc);
    }
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
      if (l < B.L) dst[l] = acc[l];
  }
}

// The reaction sum of calc_inelastic_grid on the device (kernels.h launch_reaction_sum): thread
// per (row of the batch, entry); a reaction's incoming energies own distinct rows of the matrices.
__global__ void reaction_sum_kernel(int nb, size_t GL, const double* src, const int* where,
                                    const double* scale, const double* pv, const double* yield,
                                    double* dst, double* nudst) {
  const size_t tot = (size_t)nb * GL;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < tot; t += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(t / GL);
    const size_t j = t - (size_t)k * GL;
    const size_t o = (size_t)where[k] * GL + j;
    const double v = src[t] * scale[k] * pv[k];        // scattdata_header.F90:496
    dst[o] = dst[o] + v;                               // scatt.F90:753
    if (nudst) nudst[o] = nudst[o] + yield[k] * v;     // :762
  }
}

// Orders above P7 (L > 8): the panel integrals of orders 8, 9 and 10 are evaluated in the
// reference's own operation order (legendre_ref_forms.h) -- its closed forms carry 1e-10 ... 3e-10
// of cancellation noise of their own there, which nothing else reproduces; the lower orders come
// from Legendre identities (legendre_int.h).  NDPP_ST_ORDER_NOISE, which rounds 2-3 raised on such
// calls, is no longer set.
static inline int order_noise_bits(int) { return 0; }


// Stage C2: thread per incoming energy -- trapezoid over the lab energy points
// and the P0 normalisation (:1246-1264), in the reference's order.
__global__ void f6_cm_finish_kernel(F6Batch B) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B.n_ein; e += gridDim.x * blockDim.x) {
    double* o = B.out + (size_t)e * B.G * B.L;
    for (int k = 0; k < B.G * B.L; ++k) o[k] = 0.0;
    const int g_lo = B.glohi[2 * e], g_hi = B.glohi[2 * e + 1];
    const double* Eb = B.ebnds + (size_t)e * (B.G + 2);
    for (int g = g_lo; g <= g_hi; ++g) {
      const double dEo = (Eb[g + 1] - Eb[g]) / (double)(B.NEG - 1);
      double* dg = o + (size_t)(g - 1) * B.L;
      for (int iE = 1; iE <= B.NEG; ++iE) {
        const double* fEl = B.fEl + (((size_t)e * B.G + (g - 1)) * B.NEG + (iE - 1)) * B.L;
        if ((iE != 1) && (iE != B.NEG))
          for (int l = 0; l < B.L; ++l) dg[l] = dg[l] + 2.0 * fEl[l];
        else
          for (int l = 0; l < B.L; ++l) dg[l] = dg[l] + fEl[l];
      }
      for (int l = 0; l < B.L; ++l) dg[l] = dg[l] * dEo * 0.5;
    }
    double s = 0.0;
    for (int g = g_lo; g <= g_hi; ++g) s = s + o[(size_t)(g - 1) * B.L];
    if (s > 0.0) s = 1.0 / s;
    for (int g = g_lo; g <= g_hi; ++g)
      for (int l = 0; l < B.L; ++l) o[(size_t)(g - 1) * B.L + l] *= s;
  }
}


// Stage L2: thread per (incoming energy, group): the M-1 panel integrals (:1421-1425)
template <int LMAX>
__global__ __launch_bounds__(64) void f6_lab_panel_kernel(F6Batch B) {
  const long tot = (long)B.n_ein * B.G;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < tot;
       t += (long)gridDim.x * blockDim.x) {
    const int g = (int)(t % B.G), e = (int)(t / B.G);
    double* dg = B.out + (size_t)t * B.L;
    double acc[LMAX];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) acc[l] = 0.0;
    if (B.ebnds[(size_t)e * (B.G + 2) + g] != 0.0) {
      const double* fint = B.fEl + (size_t)t * B.M;
      LinearLegendre<LMAX> walk;
      walk.start(B.grid.at(0), fint[0]);
      for (int imu = 1; imu <= B.M - 1; ++imu) {
        walk.panel_add(B.grid.at(imu), fint[imu], acc);
      }
    }
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
      if (l < B.L) dg[l] = acc[l];
  }
}

// Stage L3: thread per incoming energy: f_lo = ONE / sum(distro(1,:)) (:1447-1448), the sum
// as flang's SUM intrinsic takes it.
__global__ void f6_lab_norm_kernel(F6Batch B) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B.n_ein; e += gridDim.x * blockDim.x) {
    double* o = B.out + (size_t)e * B.G * B.L;
    KahanSum sum;
    for (int g = 0; g < B.G; ++g) sum.add(o[(size_t)g * B.L]);
    const double f_lo = 1.0 / sum.s;
    for (int k = 0; k < B.G * B.L; ++k) o[k] = o[k] * f_lo;
  }
}

// ---- law 9 ---------------------------------------------------------------------
// thread per (incoming energy, row in {lo,hi}, group): law9_scatter_lab_leg (:1274-1326)
template <int LMAX>
__global__ __launch_bounds__(64) void law9_kernel(int n_ein, const double* ein, const int* row_lo, MuGrid grid,
                            const double* f_tab, const double* edata, int G, int L,
                            const double* e_bins, double* raw /*[n_ein][2][G][L]*/) {
  const long tot = (long)n_ein * 2 * G;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < tot;
       t += (long)gridDim.x * blockDim.x) {
    const int g = (int)(t % G), r = (int)((t / G) % 2), e = (int)(t / (2L * G));
    const double Ein = ein[e];
    const double* fmu = f_tab + (size_t)(row_lo[e] + r) * grid.M;
    double acc[LMAX], pan[LMAX];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) acc[l] = 0.0;
    double pE;
    if (law9_group(edata, tab1(edata, Ein), Ein, e_bins[g], e_bins[g + 1], pE)) {
      LinearLegendre<LMAX> walk;
      walk.start(grid.at(0), fmu[0]);
      for (int imu = 1; imu <= grid.M - 1; ++imu) {
        walk.panel(grid.at(imu), fmu[imu], pan);
#pragma unroll
        for (int l = 0; l < LMAX; ++l) acc[l] = acc[l] + pan[l] * pE;
      }
    }
    double* o = raw + (size_t)t * L;
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
      if (l < L) o[l] = acc[l];
  }
}

// result = (1-f)*lo + f*hi, scattdata_header.F90:628,:636
__global__ void law9_blend_kernel(int n_ein, const double* w_hi, const double* raw, int GL,
                                  double* out, int* status) {
  const long tot = (long)n_ein * GL;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < tot;
       t += (long)gridDim.x * blockDim.x) {
    const int e = (int)(t / GL), k = (int)(t % GL);
    const double f = w_hi[e];
    const double r = (1.0 - f) * raw[((size_t)2 * e) * GL + k];
    out[t] = r + f * raw[((size_t)2 * e + 1) * GL + k];
    if (k == 0 && status) status[e] = 0;
  }
}

template <int LMAX>
void launch_cm_point(const F6Batch& B) {
  const long tot = (long)B.n_ein * B.G * B.NEG;
  hipLaunchKernelGGL(f6_cm_list_kernel, dim3(nblk(tot, 256)), dim3(256), 0, 0, B);
  hipLaunchKernelGGL((f6_cm_point_kernel<LMAX>), dim3(nblk(tot, 64)), dim3(64), 0, 0, B);
}
template <int LMAX>
void launch_lab_panel(const F6Batch& B) {
  const long tot = (long)B.n_ein * B.G;
  hipLaunchKernelGGL((f6_lab_panel_kernel<LMAX>), dim3(nblk(tot, 64)), dim3(64), 0, 0, B);
}
template <int LMAX>
void launch_law9(int n_ein, const double* ein, const int* row_lo, const MuGrid& grid,
                 const double* f_tab, const double* edata, int G, int L, const double* e_bins,
                 double* raw) {
  const long tot = (long)n_ein * 2 * G;
  hipLaunchKernelGGL((law9_kernel<LMAX>), dim3(nblk(tot, 64)), dim3(64), 0, 0, n_ein, ein,
                     row_lo, grid, f_tab, edata, G, L, e_bins, raw);
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

void ndpp::launch_reaction_sum(int nb, size_t GL, const double* src, const int* where, const double* scale,
                               const double* pv, const double* yield, double* dst, double* nudst) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(reaction_sum_kernel, dim3(nblk((long)nb * (long)GL, 256)), dim3(256), 0, 0, nb, GL, src,
                     where, scale, pv, yield, dst, nudst);
}

extern "C" int ndpp_file6_leg_batch(const ndpp_params* p, double awr, int frame_cm, int n_ein,
                                    const double* ein, const int* row_lo, int n_rows,
                                    const double* e_grid, const int* row_ptr,
                                    const double* eout, const double* pdf, const int* intt,
                                    const double* f, int G, const double* e_bins, double* out,
                                    int* status) {
  return file6_batch_sink(p, awr, frame_cm, n_ein, ein, row_lo, n_rows, e_grid, row_ptr, eout, pdf, intt, f, G,
                          e_bins, 0, out, status, nullptr);
}

// n_tab = 0: the Legendre moments (L = p->order per group); n_tab > 0: the tabular bins
// (tab_kernels.hip), n_tab per group -- the stages before the panel integrals are shared.
int ndpp::file6_batch_sink(const ndpp_params* p, double awr, int frame_cm, int n_ein,
                           const double* ein, const int* row_lo, int n_rows,
                           const double* e_grid, const int* row_ptr,
                           const double* eout, const double* pdf, const int* intt,
                           const double* f, int G, const double* e_bins, int n_tab, double* out,
                           int* status, DeviceSink* sink, const double* f_dev) {
  if (n_tab < 0 || n_tab > NDPP_MAX_TAB_BINS) return fail(NDPP_EINVAL, "n_tab=%d outside 1..%d", n_tab, NDPP_MAX_TAB_BINS);
  if (!p || !ein || !row_lo || !e_grid || !row_ptr || !eout || !pdf || !intt || (!f && !f_dev) || !e_bins || (!out && !sink))
    if (n_ein != 0) return fail(NDPP_EINVAL, "NULL argument");
  if (n_ein < 0 || n_rows < 2) return fail(NDPP_EINVAL, "n_ein=%d n_rows=%d", n_ein, n_rows);
  if (n_ein == 0) return NDPP_OK;
  if (p && p->ne_per_grp < 2) return fail(NDPP_EINVAL, "ne_per_grp=%d < 2", p->ne_per_grp);
  int npmax = 0, ubcap = 0;
  for (int k = 0; k < n_rows; ++k) {
    const int np = row_ptr[k + 1] - row_ptr[k];
    if (np < 2) return fail(NDPP_EINVAL, "row %d has %d outgoing energies (need >= 2)", k, np);
    npmax = std::max(npmax, np);
    if (k + 1 < n_rows) ubcap = std::max(ubcap, np + row_ptr[k + 2] - row_ptr[k + 1]);
  }
  int rc;
  if ((rc = check_row_lo(n_ein, row_lo, n_rows)) || (rc = check_params(p, G, kCheckOrder)) || (rc = require_device()))
    return rc;

  const int L = n_tab > 0 ? n_tab : p->order, M = p->mu_bins, NEG = p->ne_per_grp;
  const size_t ntot = (size_t)row_ptr[n_rows];
  F6Batch B;
  B.n_ein = n_ein; B.G = G; B.L = L; B.M = M; B.NEG = NEG; B.frame_cm = frame_cm;
  B.ubcap = ubcap; B.npmax = npmax; B.awr = awr; B.grid = make_mu_grid(M);
  DevBuf<double> d_ein, d_eg, d_eout, d_pdf, d_f, d_bins, d_uba, d_ubb, d_ub, d_wf, d_Eo, d_pd,
      d_r1, d_r2, d_fEl, d_ebnds, d_out;
  DevBuf<int> d_row, d_rp, d_intt, d_nub, d_j1, d_j2, d_glohi, d_st;
  NDPP_TRY(d_ein.upload(ein, n_ein));
  NDPP_TRY(d_row.upload(row_lo, n_ein));
  NDPP_TRY(d_eg.upload(e_grid, n_rows));
  NDPP_TRY(d_rp.upload(row_ptr, n_rows + 1));
  NDPP_TRY(d_eout.upload(eout, ntot));
  NDPP_TRY(d_pdf.upload(pdf, ntot));
  NDPP_TRY(d_intt.upload(intt, n_rows));
  if (!f_dev) NDPP_TRY(d_f.upload(f, ntot * M));
  NDPP_TRY(d_bins.upload(e_bins, G + 1));
  NDPP_TRY(d_uba.alloc((size_t)n_ein * npmax));
  NDPP_TRY(d_ubb.alloc((size_t)n_ein * npmax));
  NDPP_TRY(d_ub.alloc((size_t)n_ein * ubcap));
  NDPP_TRY(d_nub.alloc(n_ein));
  NDPP_TRY(d_wf.alloc(n_ein));
  NDPP_TRY(d_Eo.alloc((size_t)n_ein * ubcap));
  NDPP_TRY(d_pd.alloc((size_t)n_ein * ubcap));
  NDPP_TRY(d_j1.alloc((size_t)n_ein * ubcap));
  NDPP_TRY(d_j2.alloc((size_t)n_ein * ubcap));
  NDPP_TRY(d_r1.alloc((size_t)n_ein * ubcap));
  NDPP_TRY(d_r2.alloc((size_t)n_ein * ubcap));
  const size_t nwork = frame_cm ? (size_t)n_ein * G * NEG * L : (size_t)n_ein * G * M;
  NDPP_TRY(d_fEl.alloc(nwork));
  NDPP_TRY(d_glohi.alloc((size_t)2 * n_ein));
  NDPP_TRY(d_ebnds.alloc((size_t)n_ein * (G + 2)));
  NDPP_TRY(d_out.alloc((size_t)n_ein * G * L));
  NDPP_TRY(d_st.alloc(n_ein));
  DevBuf<unsigned> d_list;                       // [items] + the count behind them
  const size_t n_items = frame_cm ? (size_t)n_ein * G * NEG : 0;
  if (n_items >= 0xffffffffull) return fail(NDPP_EINVAL, "file 6 CM batch of %zu items: split the call", n_items);
  NDPP_TRY(d_list.alloc(n_items + 1));
  NDPP_TRY(hipMemsetAsync(d_list.p + n_items, 0, sizeof(unsigned), 0));
  B.cm_list = d_list.p; B.cm_live = d_list.p + n_items;
  B.ein = d_ein.p; B.row_lo = d_row.p; B.e_grid = d_eg.p; B.row_ptr = d_rp.p;
  B.eout = d_eout.p; B.pdf = d_pdf.p; B.intt = d_intt.p; B.f = f_dev ? f_dev : d_f.p; B.e_bins = d_bins.p;
  B.ub_a = d_uba.p; B.ub_b = d_ubb.p; B.ub = d_ub.p; B.nub = d_nub.p; B.wf = d_wf.p;
  B.Eo = d_Eo.p; B.pd = d_pd.p; B.j1 = d_j1.p; B.j2 = d_j2.p; B.r1 = d_r1.p; B.r2 = d_r2.p;
  B.fEl = d_fEl.p; B.glohi = d_glohi.p; B.ebnds = d_ebnds.p; B.out = d_out.p; B.status = d_st.p;

  GpuSpan span(nullptr, frame_cm ? kProfFile6Cm : kProfFile6Lab);
  hipLaunchKernelGGL(f6_unitbase_kernel, dim3(nblk(n_ein, 64)), dim3(64), 0, 0, B);
  if (n_tab > 0) {
    if (frame_cm) hipLaunchKernelGGL(f6_cm_bounds_kernel, dim3(nblk(n_ein, 64)), dim3(64), 0, 0, B);
    else hipLaunchKernelGGL(f6_lab_int_kernel, dim3(nblk((long)n_ein * G * M, 256)), dim3(256), 0, 0, B);
    launch_f6_tab(B);
  } else if (frame_cm) {
    hipLaunchKernelGGL(f6_cm_bounds_kernel, dim3(nblk(n_ein, 64)), dim3(64), 0, 0, B);
    dispatch_lmax(L, [&](auto lmax) { launch_cm_point<decltype(lmax)::value>(B); });
    hipLaunchKernelGGL(f6_cm_finish_kernel, dim3(nblk(n_ein, 64)), dim3(64), 0, 0, B);
  } else {
    hipLaunchKernelGGL(f6_lab_int_kernel, dim3(nblk((long)n_ein * G * M, 256)), dim3(256), 0, 0, B);
    dispatch_lmax(L, [&](auto lmax) { launch_lab_panel<decltype(lmax)::value>(B); });
    hipLaunchKernelGGL(f6_lab_norm_kernel, dim3(nblk(n_ein, 64)), dim3(64), 0, 0, B);
  }
  return finish_batch(d_out.p, d_st.p, n_ein, (size_t)G * L, order_noise_bits(L), out, status, sink, span);
}

extern "C" int ndpp_law9_leg_batch(const ndpp_params* p, int n_ein, const double* ein,
                                   const int* row_lo, const double* w_hi, int n_rows,
                                   const double* f_tab, int n_edata, const double* edata, int G,
                                   const double* e_bins, double* out, int* status) {
  return law9_batch_sink(p, n_ein, ein, row_lo, w_hi, n_rows, f_tab, n_edata, edata, G, e_bins, 0, out, status,
                         nullptr);
}

// n_tab = 0: the Legendre moments; n_tab > 0: the tabular bins (law9_tab_kernel, tab_kernels.hip) --
// everything but the integrating kernel is shared.  The tabular call checks its parameters first and
// does not read the order; the Legendre call checks them last (n_ein = 0 is an empty call whatever
// they are): as the two entry points always did.
int ndpp::law9_batch_sink(const ndpp_params* p, int n_ein, const double* ein, const int* row_lo,
                          const double* w_hi, int n_rows, const double* f_tab, int n_edata,
                          const double* edata, int G, const double* e_bins, int n_tab, double* out,
                          int* status, DeviceSink* sink) {
  int rc;
  if (n_tab != 0 && (rc = check_params(p, G, kCheckTab, n_tab))) return rc;
  if (n_ein < 0 || n_rows < 2 || n_edata < 5) return fail(NDPP_EINVAL, "bad sizes");
  if (n_ein == 0) return NDPP_OK;
  if (!p || !ein || !row_lo || !w_hi || !f_tab || !edata || !e_bins || (!out && !sink))
    return fail(NDPP_EINVAL, "NULL argument");
  if ((rc = check_row_lo(n_ein, row_lo, n_rows)) || (rc = check_law9_edata(n_edata, edata))) return rc;
  if (n_tab == 0 && (rc = check_params(p, G, kCheckOrder))) return rc;
  if ((rc = require_device())) return rc;
  const int L = n_tab > 0 ? n_tab : p->order, M = p->mu_bins, GL = G * L;
  BatchInputs in;
  if ((rc = in.upload(n_ein, ein, w_hi, row_lo, (size_t)n_rows * M, f_tab, G, e_bins, n_edata, edata))) return rc;
  DevBuf<double> d_raw, d_out;
  DevBuf<int> d_st;
  NDPP_TRY(d_raw.alloc((size_t)n_ein * 2 * GL));
  NDPP_TRY(d_out.alloc((size_t)n_ein * GL));
  NDPP_TRY(d_st.alloc(n_ein));
  GpuSpan span(nullptr, kProfLaw9);
  if (n_tab > 0)
    launch_law9_tab(n_ein, in.ein.p, in.row_lo.p, M, in.f_tab.p, in.extra.p, G, L, in.e_bins.p, d_raw.p);
  else
    dispatch_lmax(L, [&](auto lmax) {
      launch_law9<decltype(lmax)::value>(n_ein, in.ein.p, in.row_lo.p, make_mu_grid(M), in.f_tab.p, in.extra.p, G,
                                         L, in.e_bins.p, d_raw.p);
    });
  hipLaunchKernelGGL(law9_blend_kernel, dim3(nblk((long)n_ein * GL, 256)), dim3(256), 0, 0, n_ein,
                     in.w_hi.p, d_raw.p, GL, d_out.p, d_st.p);
  return finish_batch(d_out.p, d_st.p, n_ein, (size_t)GL, n_tab > 0 ? 0 : order_noise_bits(L), out, status, sink,
                      span);
}
