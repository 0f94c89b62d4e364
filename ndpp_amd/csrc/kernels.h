// kernels.h -- launchers shared between the translation units of libndpp_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/ndpp_hip.h"

namespace ndpp {

// records the message returned by ndpp_last_error() and returns `code`
int fail(int code, const char* fmt, ...);

// a HIP call of a function that returns an NDPP code: its failure is NDPP_EDEVICE, through fail()
#define NDPP_TRY(expr)                                                        \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess)                                                     \
      return fail(NDPP_EDEVICE, "%s failed: %s (%s:%d)", #expr,               \
                  hipGetErrorString(e_), __FILE__, __LINE__);                 \
  } while (0)

// ---- the host checks the batch entry points share (ndpp_hip.hip); each returns NDPP_OK or what
// fail() returned.  An entry point calls require_device LAST: a bad argument is reported before a
// missing device is.
// NDPP_EDEVICE when there is no device ("<who>: " in front of the message if given)
int require_device(const char* who = nullptr);
// every row_lo[i] has a row above it: 0 <= row_lo[i] <= n_rows - 2
int check_row_lo(int n_ein, const int* row_lo, int n_rows);
// the law-9 edist%data [NR, (NBT, INT) x NR, NE, E(NE), T(NE), U] fits its n_edata words
int check_law9_edata(int n_edata, const double* edata);
// params non-null, mu_bins >= 2 and G >= 1, and what `what` adds: the order (Legendre output), n_tab
// (tabular output, which does not read the order), the adaptive limits and tolerances (free gas)
enum ParamChecks { kCheckOrder = 1, kCheckTab = 2, kCheckFreegas = 4 };
int check_params(const ndpp_params* p, int G, int what, int n_tab = 0);

// is_valid_scatter, scattdata_header.F90:1502-1515
inline bool valid_scatter(int MT) {
  if (MT == 2 || (MT >= 11 && MT <= 91))
    return MT != 18 && MT != 19 && MT != 20 && MT != 21 && MT != 38;
  return false;
}

// f(std::integral_constant<int, LMAX>) with the smallest LMAX of 4, 6, 8, 11 that holds L orders:
// the kernels that keep their moments in registers are instantiated for these four
template <class F>
auto dispatch_lmax(int L, F&& f) {
  if (L <= 4) return f(std::integral_constant<int, 4>());
  if (L <= 6) return f(std::integral_constant<int, 6>());
  if (L <= 8) return f(std::integral_constant<int, 8>());
  return f(std::integral_constant<int, 11>());
}
// f(std::integral_constant<int, N>) with N = n_moments, 1 <= n_moments <= NDPP_MAX_ORDER (checked by
// the caller): the library analyses are instantiated for every number of moments they evaluate
template <class F>
void dispatch_moments(int n_moments, F&& f) {
  static_assert(NDPP_MAX_ORDER == 11, "one case per number of moments");
  switch (n_moments) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
    case 9: return f(std::integral_constant<int, 9>());
    case 10: return f(std::integral_constant<int, 10>());
    default: return f(std::integral_constant<int, 11>());
  }
}

// hipEvent bracket around the kernels of one batch call: the span between
// construction and end() is what ndpp_last_gpu_ms() reports (uploads, downloads
// and allocation are outside it).  The time is also added to the calling thread's
// per-family profile (ndpp_profile_get): which kernels a whole-nuclide call spent its
// device time in.
enum ProfileFamily { kProfFreegasMu = 0, kProfFreegasOther, kProfFile4, kProfFile6Cm, kProfFile6Lab,
                     kProfLaw9, kProfSab, kProfChi, kProfConvert, kNumProfileFamilies };
void profile_add(int family, double ms);
struct GpuSpan {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s;
  int family;
  explicit GpuSpan(hipStream_t stream = nullptr, int family = -1);
  void end();      // records the closing event; call before the final synchronise
  ~GpuSpan();      // after the device has synchronised: publishes the elapsed time
};

// file4_kernels.hip (always built with the reference's IEEE operation order:
// -DNDPP_FAST=0 -ffp-contract=off, the kernel is bit-identical to the Fortran).
// Thread per (E_in of `list` (or all if null), group): integrate_file4_cm_leg for
// rows_per_ein bracketing rows + blend, written to out[i][g][0..L).
// Mixed-nuclide batches pass nuc_of_ein / nuc_awr / nuc_Q (device arrays; awr and Q
// of incoming energy i are nuc_awr[nuc_of_ein[i]], nuc_Q[...]); otherwise null.
void launch_file4_any(int n, const int* list, int mu_bins, const double* ein,
                      const int* row_lo, const double* w_hi, const double* f_tab,
                      double awr, double Q, int G, int L, const double* e_bins,
                      int rows_per_ein, double* out, hipStream_t s,
                      const int* nuc_of_ein = nullptr, const double* nuc_awr = nullptr,
                      const double* nuc_Q = nullptr);

// One launcher per stage of the free-gas pipeline, in one arithmetic.  `batch` points to the
// caller's FgBatch (same layout in both arithmetic namespaces) and `bytes` is its size there; an
// entry returns NDPP_OK or what fail() returned.  The pipeline driver (ndpp_hip.hip) holds one
// table per arithmetic and a context calls through the table of its own.
struct FgStages {
  int (*setup)(const void* batch, size_t bytes, hipStream_t s);
  int (*prep)(const void* batch, size_t bytes, int level, hipStream_t s);
  int (*item)(const void* batch, size_t bytes, int level, hipStream_t s);
  int (*seg_zero)(const void* batch, size_t bytes, int level, hipStream_t s);
  int (*mu)(const void* batch, size_t bytes, int level, int num_cu, double* gstack, int* counter, hipStream_t s);
  int (*combine)(const void* batch, size_t bytes, int level, hipStream_t s);
  int (*node)(const void* batch, size_t bytes, int level, hipStream_t s);
  int (*reduce)(const void* batch, size_t bytes, int level, hipStream_t s);
  int (*assemble)(const void* batch, size_t bytes, hipStream_t s);
};
// fg_strict_stages.hip (always -DNDPP_FAST=0 -ffp-contract=off): the stages in the reference's
// arithmetic.
const FgStages& fg_strict_stages();

// Where a batch call leaves its moments when the caller goes on working on the device (the
// nuclide driver's reaction sum): consume() is handed the device array [n][G*L] instead of the
// call copying it to the host; it must only enqueue work on the null stream (the array is freed
// -- which waits for that work -- when the batch call returns).
struct DeviceSink {
  virtual ~DeviceSink() = default;
  virtual int consume(const double* out_d, int n, size_t GL) = 0;
};
// the batch entry points of the C ABI with a sink (null: host array `out`, as the ABI says)
int elastic_leg_batch_sink(const ndpp_params* p, double A, double kT, double freegas_cutoff, double Q,
                           int n_ein, const double* ein, const int* row_lo, const double* w_hi,
                           int n_rows, const double* f_tab, int G, const double* e_bins, double* out,
                           int* status, DeviceSink* sink);
// n_tab = 0: the Legendre moments of ndpp_file6_leg_batch; n_tab > 0: the tabular bins of
// ndpp_file6_tab_batch, n_tab per group.  (f_dev non-null: the table f[sum NP][M] is already on the
// device -- convert_distro_keep -- and `f` is not read)
int file6_batch_sink(const ndpp_params* p, double awr, int frame_cm, int n_ein, const double* ein,
                     const int* row_lo, int n_rows, const double* e_grid, const int* row_ptr,
                     const double* eout, const double* pdf, const int* intt, const double* f, int G,
                     const double* e_bins, int n_tab, double* out, int* status, DeviceSink* sink,
                     const double* f_dev = nullptr);
// n_tab = 0: the Legendre moments of ndpp_law9_leg_batch; n_tab > 0: the bins of ndpp_law9_tab_batch
int law9_batch_sink(const ndpp_params* p, int n_ein, const double* ein, const int* row_lo,
                    const double* w_hi, int n_rows, const double* f_tab, int n_edata,
                    const double* edata, int G, const double* e_bins, int n_tab, double* out, int* status,
                    DeviceSink* sink);
// nbody_kernels.hip: ndpp_nbody_leg_batch with a sink (Legendre moments only)
int nbody_batch_sink(const ndpp_params* p, double awr, double Q, int n_bodies, double Ap, int n_ein,
                     const double* ein, int G, const double* e_bins, double* out, int* status,
                     DeviceSink* sink);
// nbody_kernels.hip: ndpp_nbody_tab_batch with a sink (n_tab bins per group)
int nbody_tab_batch_sink(const ndpp_params* p, int n_tab, double awr, double Q, int n_bodies, double Ap, int n_ein,
                         const double* ein, int G, const double* e_bins, double* out, int* status,
                         DeviceSink* sink);
// tab_kernels.hip: law9_batch_sink's integrating kernel for n_tab = N > 0 (raw [n_ein][2][G][N], null
// stream), and the tabular counterpart of elastic_leg_batch_sink
void launch_law9_tab(int n_ein, const double* ein, const int* row_lo, int mu_bins, const double* f_tab,
                     const double* edata, int G, int N, const double* e_bins, double* raw);
int elastic_tab_batch_sink(const ndpp_params* p, double A, double kT, double freegas_cutoff, double Q,
                           int n_ein, const double* ein, const int* row_lo, const double* w_hi,
                           int n_rows, const double* f_tab, int G, const double* e_bins, int n_tab,
                           double* out, int* status, DeviceSink* sink);
// P0 of one group's row of L entries: the first moment, or (tab) the sum of the bins
inline double group_p0(const double* m, int L, bool tab) {
  if (!tab) return m[0];
  double s = 0.0;
  for (int k = 0; k < L; ++k) s += m[k];
  return s;
}
// ndpp_scatt_wire, with the gmin / gmax range found on group_p0(.., tab) (wire.hip)
long scatt_wire(const ndpp_scatt_result* r, int n_bins, const double* e_bins, bool tab, long cap,
                unsigned char* buf);
// ndpp_convert_distro that leaves the table where convert_kernel wrote it: *f_dev receives a
// device array [total_np][mu_bins] (dev_util.h's cached allocator; release with free_converted)
// for a consumer on the same device, and nothing of it crosses to the host
// (scattdata_header.F90:325-382 feeds integrate_distro: both ends are device kernels here).
int convert_distro_keep(int mu_bins, const ndpp_ace_reaction* r, int G, const double* e_bins, int NE,
                        int total_np, double* e_grid, int* row_ptr, double* eout, double* pdf,
                        double* cdf, int* intt, double** f_dev);
void free_converted(double* f_dev);
// dst[where[k]][j] += src[k][j] * scale[k] * pv[k]; nudst[where[k]][j] += yield[k] * that
// (scatt_interp_distro's scaling and calc_inelastic_grid's reaction sum, scattdata_header.F90:496,
// scatt.F90:753,:762, in their order of operations; all pointers device; null stream)
void launch_reaction_sum(int nb, size_t GL, const double* src, const int* where, const double* scale,
                         const double* pv, const double* yield, double* dst, double* nudst);

}  // namespace ndpp
