// sab_kernels.hip -- thermal S(alpha,beta) scattering moments from ACE thermal
// tables: integrate_sab_el (sab.F90:21-109), integrate_sab_inel_disc (:142-245),
// integrate_sab_inel_cont (:253-408), combine_sab_grid (:415-454); i.e. the
// Legendre path of calc_scattsab (scatt.F90:543-596).
//
// Only calc_pn and + - * / are involved, every output element is accumulated by
// one thread in the reference's order, and the TU is always built with
// -DNDPP_FAST=0 -ffp-contract=off: results are bit-identical to the Fortran.
//
// A thermal table is a set of point masses (cosine, weight).  Each of the reference's three walks
// over them -- elastic, discrete inelastic, stage 1 of the continuous inelastic -- is written once,
// as a device function over a sink that says what a mass adds to the thread's element: MomentSink
// adds P_l(mu) w for the thread's order (ndpp_sab_batch), BinSink adds w, whole, where the cosine's
// bin is the thread's (ndpp_sab_tab_batch, include/ndpp_hip.h).  The Legendre and the tabular
// kernels are the two thread mappings onto the same walk: same masses, same order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "ndpp_math.h"

#if NDPP_FAST
#error "sab_kernels.hip must be compiled with -DNDPP_FAST=0 -ffp-contract=off"
#endif

namespace ndpp {
namespace {

constexpr int SAB_SECONDARY_EQUAL = 0, SAB_SECONDARY_SKEWED = 1, SAB_SECONDARY_CONT = 2;
constexpr int SAB_ELASTIC_DISCRETE = 3, SAB_ELASTIC_EXACT = 4;


struct SabDev {
  ndpp_sab_flat t;  // pointers are device pointers
  int NE, G, L;     // L entries per group: orders, or N lab-cosine bins
  const double* ein;
  const double* e_bins;
  const double* wgt;   // [NEo] discrete-mode weights (:167-186)
  double* distro;      // [NEi][G][L] continuous-mode table integrals (:281)
  int* row_lost;       // [NEi] tabular, continuous mode: the table row holds a cosine that is not finite
  double* el;          // [NE][G][L]
  double* inel;
  double* mat;
  int* status;
};

// ---- sinks: what one mass (cosine mu, weight w) adds to the thread's element -------------------
// slot is the element's place among a group's L; the thread with slot 0 raises the status bits.

// order l of the Legendre moments.  Every thread has an element and no cosine is ever lost.
struct MomentSink {
  int slot;
  __device__ bool owns() const { return true; }
  __device__ void add(double& acc, double mu, double w) { acc = acc + pn_rt(slot, mu) * w; }
  __device__ bool lost() const { return false; }
};

// The bin of a lab cosine: floor((mu + 1) * (0.5 * N)) clamped to 0 .. N-1, so that a cosine on an
// interior edge goes up, mu = 1 into the last bin and a cosine rounded past +-1 into the end bin;
// -1 for a cosine that is not finite (it goes into no bin).
__device__ inline int sab_bin(double mu, int N) {
  if (!(fabs(mu) <= DBL_MAX)) return -1;
  const double q = floor((mu + 1.0) * (0.5 * (double)N));
  return q < 0.0 ? 0 : (q > (double)(N - 1) ? N - 1 : (int)q);
}

// Bin slot of N: the mass goes, whole, to the thread whose bin holds its cosine.  All lanes walk the
// masses together -- the table reads are wave-uniform -- so every bin has one owner and one order of
// summation and nothing is shared between lanes.  Threads with slot >= N never write.
struct BinSink {
  int slot, N;
  bool lost_ = false;  // a cosine that is not finite
  __device__ bool owns() const { return slot < N; }
  __device__ void add(double& acc, double mu, double w) {
    const int kb = sab_bin(mu, N);
    lost_ = lost_ || kb < 0;
    if (kb == slot) acc = acc + w;
  }
  __device__ bool lost() const { return lost_; }
};

// ---- the walks --------------------------------------------------------------------------------
// integrate_sab_el for incoming energy i
template <class Sink>
__device__ __forceinline__ void sab_el_walk(const SabDev& D, int i, Sink sink) {
  const int slot = sink.slot;
  const bool own = sink.owns();
  const ndpp_sab_flat& t = D.t;
  double* row = D.el + (size_t)i * D.G * D.L;
  if (own) for (int g = 0; g < D.G; ++g) row[(size_t)g * D.L + slot] = 0.0;
  if (t.threshold_elastic == 0.0) return;
  const double Ein = D.ein[i];
  if (Ein < t.elastic_e_in[0]) return;
  else if (Ein >= t.threshold_elastic) return;
  const int isab = bsearch1(t.elastic_e_in, t.n_elastic_e_in, Ein);
  if (isab < 0) { if (slot == 0) atomicOr(&D.status[i], NDPP_ST_RANGE); return; }
  const double f = (Ein - t.elastic_e_in[isab - 1]) / (t.elastic_e_in[isab] - t.elastic_e_in[isab - 1]);
  if (Ein < D.e_bins[0]) return;
  else if (Ein > D.e_bins[D.G]) return;
  int g = bsearch1(D.e_bins, D.G + 1, Ein);
  if (g < 1) g = 1;  // NaN energy: stay inside the row
  double sig = 0.0;
  if (t.elastic_mode == SAB_ELASTIC_EXACT) sig = t.elastic_P[isab - 1] / Ein;
  else if (t.elastic_mode == SAB_ELASTIC_DISCRETE)
    sig = (1.0 - f) * t.elastic_P[isab - 1] + f * t.elastic_P[isab];
  double acc = 0.0;
  if (t.n_elastic_mu == 0) {
    sink.add(acc, 1.0 - t.elastic_e_in[isab - 1] / Ein, 1.0);  // coherent: one Bragg edge, :87
  } else if (t.elastic_mode == SAB_ELASTIC_DISCRETE) {
    const int NMU = t.n_elastic_mu;
    const double wgt = 1.0 / (double)NMU;
    for (int imu = 0; imu < NMU; ++imu) {
      const double mu = (1.0 - f) * t.elastic_mu[(size_t)(isab - 1) * NMU + imu] +
                        f * t.elastic_mu[(size_t)isab * NMU + imu];
      sink.add(acc, mu, wgt);
    }
  }
  if (own) row[(size_t)(g - 1) * D.L + slot] = sig * acc;
  if (sink.lost() && slot == 0) atomicOr(&D.status[i], NDPP_ST_NONFINITE);
}

// integrate_sab_inel_disc for incoming energy i; groups are visited in the order the discrete
// outgoing energies fall into them, exactly as :216-242.  A group's element stays in a register for
// as long as the outgoing energies keep falling into that group and goes back to the row when they
// move on (they may come back to it later).
template <class Sink>
__device__ __forceinline__ void sab_inel_disc_walk(const SabDev& D, int i, Sink sink) {
  const int slot = sink.slot;
  const bool own = sink.owns();
  const ndpp_sab_flat& t = D.t;
  const int NEo = t.n_inelastic_e_out, NMU = t.n_inelastic_mu, NEi = t.n_inelastic_e_in;
  double* row = D.inel + (size_t)i * D.G * D.L;
  if (own) for (int g = 0; g < D.G; ++g) row[(size_t)g * D.L + slot] = 0.0;
  const double Ein = D.ein[i];
  int isab;
  double f;
  if (Ein < t.inelastic_e_in[0]) { isab = 1; f = 0.0; }
  else if (Ein > t.threshold_inelastic) return;
  else if (Ein == t.threshold_inelastic) { isab = NEi - 1; f = 1.0; }
  else {
    isab = bsearch1(t.inelastic_e_in, NEi, Ein);
    if (isab < 0) { if (slot == 0) atomicOr(&D.status[i], NDPP_ST_RANGE); return; }
    f = (Ein - t.inelastic_e_in[isab - 1]) / (t.inelastic_e_in[isab] - t.inelastic_e_in[isab - 1]);
  }
  const double sig = (1.0 - f) * t.inelastic_sigma[isab - 1] + f * t.inelastic_sigma[isab];
  int held = 0;       // the group (1-based) whose element is in acc; 0: none yet
  double acc = 0.0;
  for (int io = 0; io < NEo; ++io) {
    const double Eout = (1.0 - f) * t.inelastic_e_out[(size_t)(isab - 1) * NEo + io] +
                        f * t.inelastic_e_out[(size_t)isab * NEo + io];
    if (Eout < D.e_bins[0]) continue;
    else if (Eout >= D.e_bins[D.G]) continue;
    int g = bsearch1(D.e_bins, D.G + 1, Eout);
    if (g < 1) g = 1;  // NaN energy: stay inside the row
    if (g != held) {
      if (own && held) row[(size_t)(held - 1) * D.L + slot] = acc;
      acc = own ? row[(size_t)(g - 1) * D.L + slot] : 0.0;
      held = g;
    }
    const double w = D.wgt[io];
    for (int imu = 0; imu < NMU; ++imu) {
      const double mu = (1.0 - f) * t.inelastic_mu[((size_t)(isab - 1) * NEo + io) * NMU + imu] +
                        f * t.inelastic_mu[((size_t)isab * NEo + io) * NMU + imu];
      sink.add(acc, mu, w);
    }
  }
  if (own) {
    if (held) row[(size_t)(held - 1) * D.L + slot] = acc;
    for (int g = 0; g < D.G; ++g) row[(size_t)g * D.L + slot] = sig * row[(size_t)g * D.L + slot];
  }
  if (sink.lost() && slot == 0) atomicOr(&D.status[i], NDPP_ST_NONFINITE);
}

// integrate_sab_inel_cont, stage 1 (:292-378), for table row k and group g into D.distro[at] (the
// kernel's loop index gives `at` without a multiplication).  D.row_lost[k] is set where one of the
// masses that count is not finite.
template <class Sink>
__device__ __forceinline__ void sab_cont_table_walk(const SabDev& D, int k, int g, size_t at, Sink sink) {
  const ndpp_sab_flat& t = D.t;
  const int NMU = t.n_inelastic_mu;
  const int o = t.cont_ptr[k], NEout = t.cont_ptr[k + 1] - o;
  const double *Eo = t.cont_e_out + o, *pd0 = t.cont_pdf + o;
  const double* mu_arr = t.cont_mu + (size_t)o * NMU;
  auto pdf = [&](int j1) -> double {  // 1-based, :299-303
    return (j1 == NEout) ? 0.0 : pd0[j1 - 1] * (Eo[j1] - Eo[j1 - 1]);
  };
  const double eg = D.e_bins[g], eg1 = D.e_bins[g + 1];
  double acc = 0.0;
  int iE_lo = 1, iE_hi = 0;
  bool live = true;
  // the group edge e inside the row: the masses of outgoing point j1 blended with its upper
  // neighbour, each of weight (the blend fraction) * pdf(j1); returns j1
  auto edge = [&](double e) -> int {
    int j1 = bsearch1(Eo, NEout, e);
    if (j1 < 1) j1 = 1;
    const double fr = (e - Eo[j1 - 1]) / (Eo[j1] - Eo[j1 - 1]);
    const double mult = fr * pdf(j1);
    for (int imu = 0; imu < NMU; ++imu) {
      const double mu = (1.0 - fr) * mu_arr[(size_t)(j1 - 1) * NMU + imu] + fr * mu_arr[(size_t)j1 * NMU + imu];
      sink.add(acc, mu, mult);
    }
    return j1;
  };
  if (eg < Eo[0]) iE_lo = 1;
  else if (eg >= Eo[NEout - 1]) live = false;
  else iE_lo = edge(eg) + 1;
  if (live) {
    if (eg1 < Eo[0]) live = false;
    else if (eg1 >= Eo[NEout - 1]) iE_hi = NEout - 1;
    else iE_hi = edge(eg1) - 1;
  }
  if (live) {
    for (int iE = iE_lo; iE <= iE_hi; ++iE) {
      const double w = pdf(iE);
      for (int imu = 0; imu < NMU; ++imu) sink.add(acc, mu_arr[(size_t)(iE - 1) * NMU + imu], w);
    }
    acc = acc / (double)NMU;
  }
  if (sink.owns()) D.distro[at] = live ? acc : 0.0;
  if (live && sink.lost() && sink.slot == 0) atomicOr(&D.row_lost[k], 1);
}

// ---- the Legendre kernels: thread per (E_in, order); stage 1: per (table E_in, group, order) ----
__global__ void sab_el_kernel(SabDev D) {
  const long tot = (long)D.NE * D.L;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < tot; q += (long)gridDim.x * blockDim.x)
    sab_el_walk(D, (int)(q / D.L), MomentSink{(int)(q % D.L)});
}

__global__ void sab_inel_disc_kernel(SabDev D) {
  const long tot = (long)D.NE * D.L;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < tot; q += (long)gridDim.x * blockDim.x)
    sab_inel_disc_walk(D, (int)(q / D.L), MomentSink{(int)(q % D.L)});
}

__global__ void sab_cont_table_kernel(SabDev D) {
  const long tot = (long)D.t.n_inelastic_e_in * D.G * D.L;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < tot; q += (long)gridDim.x * blockDim.x)
    sab_cont_table_walk(D, (int)(q / ((long)D.L * D.G)), (int)((q / D.L) % D.G), (size_t)q,
                        MomentSink{(int)(q % D.L)});
}

// ---- the tabular kernels: D.L holds N; block per E_in (stage 1: per (table E_in, group)), thread
// k owns bin k of every group ----
__global__ void sab_tab_el_kernel(SabDev D) {
  for (int i = blockIdx.x; i < D.NE; i += gridDim.x) sab_el_walk(D, i, BinSink{(int)threadIdx.x, D.L});
}

__global__ void sab_tab_inel_disc_kernel(SabDev D) {
  for (int i = blockIdx.x; i < D.NE; i += gridDim.x) sab_inel_disc_walk(D, i, BinSink{(int)threadIdx.x, D.L});
}

__global__ void sab_tab_cont_table_kernel(SabDev D) {
  const long tot = (long)D.t.n_inelastic_e_in * D.G;
  for (long q = blockIdx.x; q < tot; q += gridDim.x)
    sab_cont_table_walk(D, (int)(q / D.G), (int)(q % D.G), (size_t)q * D.L + threadIdx.x,
                        BinSink{(int)threadIdx.x, D.L});
}

// stage 2 (:383-407): thread per output element, moments and bins alike
__global__ void sab_cont_interp_kernel(SabDev D) {
  const ndpp_sab_flat& t = D.t;
  const int GL = D.G * D.L;
  const long tot = (long)D.NE * GL;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < tot; q += (long)gridDim.x * blockDim.x) {
    const int k = (int)(q % GL), i = (int)(q / GL);
    const double Ein = D.ein[i];
    double v = 0.0;
    if (Ein <= t.inelastic_e_in[0]) {
      v = D.distro[k] * t.inelastic_sigma[0];
    } else if (Ein >= t.threshold_inelastic) {
      v = 0.0;
    } else {
      const int isab = bsearch1(t.inelastic_e_in, t.n_inelastic_e_in, Ein);
      if (isab < 0) { if (k == 0) atomicOr(&D.status[i], NDPP_ST_RANGE); D.inel[q] = 0.0; continue; }
      const double f = (Ein - t.inelastic_e_in[isab - 1]) / (t.inelastic_e_in[isab] - t.inelastic_e_in[isab - 1]);
      const double sig = (1.0 - f) * t.inelastic_sigma[isab - 1] + f * t.inelastic_sigma[isab];
      v = ((1.0 - f) * D.distro[(size_t)(isab - 1) * GL + k] + f * D.distro[(size_t)isab * GL + k]) * sig;
    }
    D.inel[q] = v;
  }
}

// tabular: hands a table row's lost cosine to the incoming energies that read the row: thread per
// E_in, sab_cont_interp_kernel's brackets
__global__ void sab_tab_cont_status_kernel(SabDev D) {
  const ndpp_sab_flat& t = D.t;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D.NE; i += gridDim.x * blockDim.x) {
    const double Ein = D.ein[i];
    int lost = 0;
    if (Ein <= t.inelastic_e_in[0]) lost = D.row_lost[0];
    else if (Ein >= t.threshold_inelastic) lost = 0;
    else {
      const int isab = bsearch1(t.inelastic_e_in, t.n_inelastic_e_in, Ein);
      if (isab >= 1) lost = D.row_lost[isab - 1] | D.row_lost[isab];
    }
    if (lost) atomicOr(&D.status[i], NDPP_ST_NONFINITE);
  }
}

// combine_sab_grid (:415-454): thread per E_in; the last point copies its
// neighbour, so thread NE-1 computes row NE-2's values again.
__global__ void sab_combine_kernel(SabDev D) {
  const int GL = D.G * D.L;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D.NE; i += gridDim.x * blockDim.x) {
    const int src = (i == D.NE - 1 && D.NE >= 2) ? i - 1 : i;
    const double *e = D.el + (size_t)src * GL, *q = D.inel + (size_t)src * GL;
    double* m = D.mat + (size_t)i * GL;
    KahanSum sum;  // sum(scatt_mat(1,:,iE))
    for (int g = 0; g < D.G; ++g) sum.add(e[(size_t)g * D.L] + q[(size_t)g * D.L]);
    double s = sum.s;
    if (s > 0.0) {
      s = 1.0 / s;
      for (int k = 0; k < GL; ++k) m[k] = (e[k] + q[k]) * s;
    } else {
      for (int k = 0; k < GL; ++k) m[k] = 0.0;
    }
  }
}

// combine_sab_grid with a group's bin sum in the place of its P0: s is the compensated sum of
// el + inel over the row in storage order.  Block of 64 per E_in: the row is read 64 entries at a
// time and every lane sums them from shared memory in the same order.
__global__ void sab_tab_combine_kernel(SabDev D) {
  __shared__ double part[64];
  const int GL = D.G * D.L, k0 = threadIdx.x;
  for (int i = blockIdx.x; i < D.NE; i += gridDim.x) {
    const int src = (i == D.NE - 1 && D.NE >= 2) ? i - 1 : i;
    const double *e = D.el + (size_t)src * GL, *q = D.inel + (size_t)src * GL;
    double* m = D.mat + (size_t)i * GL;
    KahanSum sum;
    for (int base = 0; base < GL; base += 64) {
      __syncthreads();
      if (base + k0 < GL) part[k0] = e[base + k0] + q[base + k0];
      __syncthreads();
      const int n = min(64, GL - base);
      for (int j = 0; j < n; ++j) sum.add(part[j]);
    }
    double s = sum.s;
    if (s > 0.0) {
      s = 1.0 / s;
      for (int k = k0; k < GL; k += 64) m[k] = (e[k] + q[k]) * s;
    } else {
      for (int k = k0; k < GL; k += 64) m[k] = 0.0;
    }
  }
}

// apply_tol_scatt (scatt.F90:786-818): thread per incoming energy; both sum()s are
// compensated like flang's SUM intrinsic.
__global__ void apply_tol_kernel(int L, int G, int n, double* data, double tol) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double* d = data + (size_t)i * G * L;
    auto p0_sum = [&]() {
      KahanSum sum;
      for (int g = 0; g < G; ++g) sum.add(d[(size_t)g * L]);
      return sum.s;
    };
    const double orig = p0_sum();
    for (int g = 0; g < G; ++g)
      if ((d[(size_t)g * L] > 0.0) && (d[(size_t)g * L] < tol))
        for (int l = 0; l < L; ++l) d[(size_t)g * L + l] = 0.0;
    const double norm = (orig > 0.0) ? orig / p0_sum() : 0.0;
    for (int k = 0; k < G * L; ++k) d[k] = d[k] * norm;
  }
}

// ---- the host side ----------------------------------------------------------------------------
// the table's counts and mode
int check_sab_counts(const ndpp_sab_flat* t) {
  const int mode = t->secondary_mode;
  if (t->n_inelastic_e_in < 2 || t->n_inelastic_mu < 1)
    return fail(NDPP_EINVAL, "need >= 2 inelastic E_in and >= 1 cosine");
  if (mode != SAB_SECONDARY_EQUAL && mode != SAB_SECONDARY_SKEWED && mode != SAB_SECONDARY_CONT)
    return fail(NDPP_EINVAL, "secondary_mode=%d", mode);
  if (mode == SAB_SECONDARY_SKEWED && t->n_inelastic_e_out <= 4)  // reference: fatal_error, sab.F90:183
    return fail(NDPP_EINVAL, "skewed weighting needs more than 4 outgoing energies");
  return NDPP_OK;
}

// the continuous mode's rows and the elastic grid
int check_sab_arrays(const ndpp_sab_flat* t) {
  if (t->secondary_mode == SAB_SECONDARY_CONT) {
    if (!t->cont_ptr) return fail(NDPP_EINVAL, "continuous mode without cont_ptr");
    if (t->cont_ptr[0] != 0) return fail(NDPP_EINVAL, "cont_ptr[0] must be 0");
    for (int k = 0; k < t->n_inelastic_e_in; ++k)
      if (t->cont_ptr[k + 1] - t->cont_ptr[k] < 2)
        return fail(NDPP_EINVAL, "continuous row %d has < 2 outgoing energies", k);
  }
  if (t->threshold_elastic != 0.0 && t->n_elastic_e_in < 2)
    return fail(NDPP_EINVAL, "elastic data needs >= 2 E_in");
  return NDPP_OK;
}

// The table, the grid and the discrete-mode weights on the device, and the three results
// [n_ein][G][L] (L: orders, or bins when tab).  The table has passed both checks above.
struct SabStage {
  DevBuf<double> ei, sig, eo, mu, ce, cp, cm, ee, eP, emu, ein, bins, w, distro, el, inel, mat;
  DevBuf<int> cptr, st, row_lost;
  size_t nout = 0;

  int upload(const ndpp_sab_flat* t, int n_ein, const double* h_ein, int G, const double* e_bins, int L,
             bool tab, SabDev& D) {
    const int NEi = t->n_inelastic_e_in, NEo = t->n_inelastic_e_out, NMU = t->n_inelastic_mu;
    const int mode = t->secondary_mode;
    nout = (size_t)n_ein * G * L;
    // discrete-mode weights, sab.F90:167-186 (sum() as flang evaluates it)
    std::vector<double> wgt(std::max(NEo, 1), 0.0);
    if (mode == SAB_SECONDARY_EQUAL) {
      for (int k = 0; k < NEo; ++k) wgt[k] = 1.0 / ((double)NEo * (double)NMU);
    } else if (mode == SAB_SECONDARY_SKEWED) {
      wgt[0] = 0.1; wgt[1] = 0.4;
      for (int k = 2; k < NEo - 2; ++k) wgt[k] = 1.0;
      wgt[NEo - 2] = 0.4; wgt[NEo - 1] = 0.1;
      KahanSum sum;
      for (int k = 0; k < NEo; ++k) sum.add(wgt[k]);
      const double den = sum.s * (double)NMU;
      for (int k = 0; k < NEo; ++k) wgt[k] = wgt[k] / den;
    }
    D.t = *t;
    D.NE = n_ein; D.G = G; D.L = L;
    NDPP_TRY(ei.upload(t->inelastic_e_in, NEi));
    NDPP_TRY(sig.upload(t->inelastic_sigma, NEi));
    if (mode != SAB_SECONDARY_CONT) {
      NDPP_TRY(eo.upload(t->inelastic_e_out, (size_t)NEi * NEo));
      NDPP_TRY(mu.upload(t->inelastic_mu, (size_t)NEi * NEo * NMU));
    } else {
      const size_t tot = (size_t)t->cont_ptr[NEi];
      NDPP_TRY(cptr.upload(t->cont_ptr, NEi + 1));
      NDPP_TRY(ce.upload(t->cont_e_out, tot));
      NDPP_TRY(cp.upload(t->cont_pdf, tot));
      NDPP_TRY(cm.upload(t->cont_mu, tot * NMU));
    }
    if (t->threshold_elastic != 0.0) {
      NDPP_TRY(ee.upload(t->elastic_e_in, t->n_elastic_e_in));
      NDPP_TRY(eP.upload(t->elastic_P, t->n_elastic_e_in));
      if (t->n_elastic_mu > 0)
        NDPP_TRY(emu.upload(t->elastic_mu, (size_t)t->n_elastic_e_in * t->n_elastic_mu));
    }
    NDPP_TRY(ein.upload(h_ein, n_ein));
    NDPP_TRY(bins.upload(e_bins, G + 1));
    NDPP_TRY(w.upload(wgt.data(), wgt.size()));
    NDPP_TRY(distro.alloc((size_t)NEi * G * L));
    NDPP_TRY(el.alloc(nout));
    NDPP_TRY(inel.alloc(nout));
    NDPP_TRY(mat.alloc(nout));
    NDPP_TRY(st.alloc(n_ein));
    NDPP_TRY(hipMemset(st.p, 0, sizeof(int) * n_ein));
    if (tab) {
      NDPP_TRY(row_lost.alloc(NEi));
      NDPP_TRY(hipMemset(row_lost.p, 0, sizeof(int) * NEi));
    }
    D.t.inelastic_e_in = ei.p; D.t.inelastic_sigma = sig.p;
    D.t.inelastic_e_out = eo.p; D.t.inelastic_mu = mu.p;
    D.t.cont_ptr = cptr.p; D.t.cont_e_out = ce.p; D.t.cont_pdf = cp.p; D.t.cont_mu = cm.p;
    D.t.elastic_e_in = ee.p; D.t.elastic_P = eP.p; D.t.elastic_mu = emu.p;
    D.ein = ein.p; D.e_bins = bins.p; D.wgt = w.p; D.distro = distro.p; D.row_lost = row_lost.p;
    D.el = el.p; D.inel = inel.p; D.mat = mat.p; D.status = st.p;
    return NDPP_OK;
  }

  // after the kernels: wait for them and copy out what the caller asked for
  int download(double* h_el, double* h_inel, double* h_mat, int* h_status, int n_ein) {
    NDPP_TRY(hipGetLastError());
    NDPP_TRY(hipDeviceSynchronize());
    NDPP_TRY(mat.download(h_mat, nout));
    if (h_el) NDPP_TRY(el.download(h_el, nout));
    if (h_inel) NDPP_TRY(inel.download(h_inel, nout));
    if (h_status) NDPP_TRY(st.download(h_status, n_ein));
    return NDPP_OK;
  }
};

// tab false: the Legendre moments (p->order per group, n_tab is not read); tab true: n_tab
// lab-cosine bins per group (p->order is not read).  Every argument check comes before the device is
// asked for.
int sab_batch_any(const ndpp_params* p, const ndpp_sab_flat* t, bool tab, int n_tab, int n_ein, const double* ein,
                  int G, const double* e_bins, double* el, double* inel, double* scatt_mat, int* status) {
  if (!p || !t) return fail(NDPP_EINVAL, "NULL params/table");
  if (tab && (n_tab < 1 || n_tab > NDPP_MAX_TAB_BINS))
    return fail(NDPP_EINVAL, "n_tab=%d outside 1..%d", n_tab, NDPP_MAX_TAB_BINS);
  if (!tab && (p->order < 1 || p->order > NDPP_MAX_ORDER))
    return fail(NDPP_EINVAL, "order=%d outside 1..%d", p->order, NDPP_MAX_ORDER);
  if (G < 1 || n_ein < 0) return fail(NDPP_EINVAL, "G=%d n_ein=%d", G, n_ein);
  if (n_ein == 0) return NDPP_OK;
  if (!ein || !e_bins || !scatt_mat) return fail(NDPP_EINVAL, "NULL array argument");
  if (int rc = check_sab_counts(t)) return rc;
  if (int rc = check_sab_arrays(t)) return rc;
  if (int rc = require_device()) return rc;

  const int L = tab ? n_tab : p->order, NEi = t->n_inelastic_e_in;
  const bool cont = t->secondary_mode == SAB_SECONDARY_CONT;
  SabDev D;
  SabStage S;
  if (int rc = S.upload(t, n_ein, ein, G, e_bins, L, tab, D)) return rc;

  GpuSpan span(nullptr, kProfSab);
  if (tab) {
    static_assert(NDPP_MAX_TAB_BINS <= 128, "one thread per bin");
    const dim3 bins_block(L <= 64 ? 64 : 128);       // thread k owns bin k
    hipLaunchKernelGGL(sab_tab_el_kernel, dim3(nblk(n_ein, 1)), bins_block, 0, 0, D);
    if (cont) {
      hipLaunchKernelGGL(sab_tab_cont_table_kernel, dim3(nblk((long)NEi * G, 1)), bins_block, 0, 0, D);
      hipLaunchKernelGGL(sab_cont_interp_kernel, dim3(nblk((long)S.nout, 256)), dim3(256), 0, 0, D);
      hipLaunchKernelGGL(sab_tab_cont_status_kernel, dim3(nblk(n_ein, 128)), dim3(128), 0, 0, D);
    } else {
      hipLaunchKernelGGL(sab_tab_inel_disc_kernel, dim3(nblk(n_ein, 1)), bins_block, 0, 0, D);
    }
    hipLaunchKernelGGL(sab_tab_combine_kernel, dim3(nblk(n_ein, 1)), dim3(64), 0, 0, D);
  } else {
    hipLaunchKernelGGL(sab_el_kernel, dim3(nblk((long)n_ein * L, 128)), dim3(128), 0, 0, D);
    if (cont) {
      hipLaunchKernelGGL(sab_cont_table_kernel, dim3(nblk((long)NEi * G * L, 64)), dim3(64), 0, 0, D);
      hipLaunchKernelGGL(sab_cont_interp_kernel, dim3(nblk((long)S.nout, 256)), dim3(256), 0, 0, D);
    } else {
      hipLaunchKernelGGL(sab_inel_disc_kernel, dim3(nblk((long)n_ein * L, 128)), dim3(128), 0, 0, D);
    }
    hipLaunchKernelGGL(sab_combine_kernel, dim3(nblk(n_ein, 128)), dim3(128), 0, 0, D);
  }
  span.end();
  return S.download(el, inel, scatt_mat, tab ? status : nullptr, n_ein);
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_sab_batch(const ndpp_params* p, const ndpp_sab_flat* t, int n_ein,
                              const double* ein, int G, const double* e_bins, double* el,
                              double* inel, double* scatt_mat) {
  return sab_batch_any(p, t, false, 0, n_ein, ein, G, e_bins, el, inel, scatt_mat, nullptr);
}

extern "C" int ndpp_sab_tab_batch(const ndpp_params* p, const ndpp_sab_flat* t, int n_tab, int n_ein,
                                  const double* ein, int G, const double* e_bins, double* el,
                                  double* inel, double* scatt_mat, int* status) {
  return sab_batch_any(p, t, true, n_tab, n_ein, ein, G, e_bins, el, inel, scatt_mat, status);
}

extern "C" int ndpp_apply_tol_scatt(int L, int G, int n, double* data, double tol) {
  if (L < 1 || G < 1 || n < 0) return fail(NDPP_EINVAL, "L=%d G=%d n=%d", L, G, n);
  if (n == 0) return NDPP_OK;
  if (!data) return fail(NDPP_EINVAL, "NULL data");
  if (int rc = require_device()) return rc;
  DevBuf<double> d;
  const size_t tot = (size_t)n * G * L;
  NDPP_TRY(d.upload(data, tot));
  hipLaunchKernelGGL(apply_tol_kernel, dim3(nblk(n, 128)), dim3(128), 0, 0, L, G, n, d.p, tol);
  NDPP_TRY(hipGetLastError());
  NDPP_TRY(hipDeviceSynchronize());
  NDPP_TRY(hipMemcpy(data, d.p, sizeof(double) * tot, hipMemcpyDeviceToHost));
  return NDPP_OK;
}
