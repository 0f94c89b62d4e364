// derive_kernels.hip -- a finished library turned into another one (include/ndpp_hip.h:
// ndpp_derive_tables, ndpp_derive_groups, ndpp_derive_bins, ndpp_derive_moments):
// coarser outgoing groups, cosine bins from Legendre moments, moments and their enclosure from bins.
// Nothing in the reference does this.
//
// Every operation is a product of a row with a fixed [L x N] table, or a segmented sum, in the order
// the header writes out; the file is built without contraction in every build, so a host restatement
// from the same tables gives the same bits (ndpp_amd/derive.py).  The tables are host code.
//
// The kernels are memory-bound row kernels.  A block takes a tile of whole rows, reads it with
// consecutive threads into LDS (staging: the global loads are coalesced whatever the row length), and
// writes its outputs with consecutive threads along the innermost axis.  No atomics, no scratch; the
// tile loops and the pass loops have trip counts that depend on the block and the launch only, so
// every barrier and every shuffle is reached by all threads.
//
// derive_groups_kernel: tile = whole incoming energies of G * L doubles; one thread per output
//   (e, c, l), l fastest, sums its segment from LDS.  A row of more than kStageDoubles is read from
//   global memory directly (neighbouring threads still read neighbouring l).
// derive_bins_kernel<L>: W in LDS; a row is taken by T = min(64, N rounded up to a power of two)
//   neighbouring lanes, each with the row's L moments in registers and the bins k = lane, lane + T, ..;
//   the row's status is folded over the T lanes by shuffles.
// derive_moments_kernel<Bounds>: V (and pmin, pmax) transposed in LDS, [k][l], so that neighbouring l
//   are neighbouring banks; one thread per output (row, l), l fastest, walks the row's N bins in LDS.
//   The flags of a row's L threads meet in LDS (plain stores), and one thread per row writes the status.
#include <cfloat>
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
constexpr int kStageDoubles = 4096;     // 32 KB of staged rows at most
constexpr int kMaxGrid = 1 << 16;

__device__ inline bool finite_d(double v) { return fabs(v) < INFINITY; }

__global__ void __launch_bounds__(kThreads)
derive_groups_kernel(long n, int G, int L, int Gc, int epb, int staged, const double* __restrict__ mat,
                     const int* __restrict__ first, double* __restrict__ out) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, B = blockDim.x;
  const size_t GL = (size_t)G * L, GcL = (size_t)Gc * L;
  const long tiles = (n + epb - 1) / epb;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long e0 = tile * epb;
    const int ne = (int)min((long)epb, n - e0);
    const double* src = mat + (size_t)e0 * GL;
    if (staged) {
      __syncthreads();                               // the previous tile has been read
      const int words = ne * (int)GL;
      for (int i = tid; i < words; i += B) lds[i] = src[i];
      __syncthreads();
      src = lds;
    }
    const long outs = (long)ne * (long)GcL;
    for (long i = tid; i < outs; i += B) {
      const int e = (int)(i / (long)GcL);
      const int cl = (int)(i - (long)e * (long)GcL);
      const int c = cl / L, l = cl - c * L;
      const double* p = src + (size_t)e * GL + l;
      double s = 0.0;
      for (int g = first[c]; g < first[c + 1]; ++g) s = s + p[(size_t)g * L];
      out[(size_t)e0 * GcL + (size_t)i] = s;
    }
  }
}

template <int L>
__global__ void __launch_bounds__(kThreads)
derive_bins_kernel(long rows, int N, int T, int RT, const double* __restrict__ mat, const double* __restrict__ Wg,
                   double* __restrict__ out, int* __restrict__ status) {
  extern __shared__ double lds[];
  double* sW = lds;                  // [L][N]
  double* stage = lds + L * N;       // [RT][L]
  const int tid = threadIdx.x, B = blockDim.x;
  for (int i = tid; i < L * N; i += B) sW[i] = Wg[i];
  const int RB = B / T, sub = tid / T, lane = tid - sub * T;
  const long tiles = (rows + RT - 1) / RT;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long row0 = tile * RT;
    const int nr = (int)min((long)RT, rows - row0);
    __syncthreads();                                 // W is there; the previous tile has been read
    for (int i = tid; i < nr * L; i += B) stage[i] = mat[(size_t)row0 * L + i];
    __syncthreads();
    for (int rr = sub; rr < RT; rr += RB) {          // RT is a multiple of RB: the same trips in every lane
      const bool active = rr < nr;
      double a[L];
      int bits = 0;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        a[l] = active ? stage[rr * L + l] : 0.0;
        if (!finite_d(a[l])) bits |= NDPP_DERIVE_NONFINITE;
      }
      const bool zero = a[0] == 0.0;
      if (zero) bits |= NDPP_DERIVE_ZERO;
      for (int kb = 0; kb < N; kb += T) {
        const int k = kb + lane;
        if (k < N) {
          double t = 0.0;
#pragma unroll
          for (int l = 0; l < L; ++l) t = t + a[l] * sW[l * N + k];
          if (zero) t = 0.0;
          if (!finite_d(t)) bits |= NDPP_DERIVE_NONFINITE;
          if (t < 0.0) bits |= NDPP_DERIVE_NEGBIN;
          if (active) out[(size_t)(row0 + rr) * N + k] = t;
        }
      }
      for (int o = T >> 1; o > 0; o >>= 1) bits |= __shfl_xor(bits, o, T);
      if (active && lane == 0) status[row0 + rr] = bits;
    }
  }
}

template <bool Bounds>
__global__ void __launch_bounds__(kThreads)
derive_moments_kernel(long rows, int N, int L, int RT, const double* __restrict__ mat, const double* __restrict__ Vg,
                      const double* __restrict__ pming, const double* __restrict__ pmaxg, double* __restrict__ out,
                      double* __restrict__ lo, double* __restrict__ hi, int* __restrict__ status) {
  extern __shared__ double lds[];
  const int LN = L * N;
  double* sV = lds;                                  // [N][L], transposed
  double* sMin = sV + LN;                            // (Bounds only)
  double* sMax = sMin + (Bounds ? LN : 0);
  const int NP = N + 1;                              // the pitch of a staged row: the threads of a wave read
                                                     // the same k of up to 64 / L + 1 rows, which a pitch
                                                     // of N = 32 or 128 would put into one bank
  double* stage = sMax + (Bounds ? LN : 0);          // [RT][NP]
  int* flags = (int*)(stage + (size_t)RT * NP);      // [RT][L]
  const int tid = threadIdx.x, B = blockDim.x;
  for (int i = tid; i < LN; i += B) {
    const int l = i / N, k = i - l * N;
    sV[k * L + l] = Vg[i];
    if (Bounds) {
      sMin[k * L + l] = pming[i];
      sMax[k * L + l] = pmaxg[i];
    }
  }
  const long tiles = (rows + RT - 1) / RT;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long row0 = tile * RT;
    const int nr = (int)min((long)RT, rows - row0);
    __syncthreads();                                 // the tables are there; the previous tile is done
    for (int i = tid; i < nr * N; i += B) {
      const int r = i / N;
      stage[r * NP + (i - r * N)] = mat[(size_t)row0 * N + i];
    }
    __syncthreads();
    for (int i = tid; i < nr * L; i += B) {
      const int rr = i / L, l = i - rr * L;
      const double* x = stage + rr * NP;
      double s = 0.0, slo = 0.0, shi = 0.0;
      int bits = 0;
      for (int k = 0; k < N; ++k) {
        const double v = x[k];
        if (!finite_d(v)) bits |= NDPP_DERIVE_NONFINITE;
        if (v < 0.0) bits |= NDPP_DERIVE_NEGBIN;
        s = s + v * sV[k * L + l];
        if (Bounds) {
          slo = slo + v * sMin[k * L + l];
          shi = shi + v * sMax[k * L + l];
        }
      }
      if (!finite_d(s)) bits |= NDPP_DERIVE_NONFINITE;
      const size_t at = (size_t)row0 * L + i;
      out[at] = s;
      if (Bounds) {
        if (lo) lo[at] = slo;
        if (hi) hi[at] = shi;
      }
      flags[i] = bits;
    }
    __syncthreads();
    for (int rr = tid; rr < nr; rr += B) {
      int bits = 0;
      for (int l = 0; l < L; ++l) bits |= flags[rr * L + l];
      status[row0 + rr] = bits;
    }
  }
}

// ---- host: the tables ------------------------------------------------------------------------

// P_0 .. P_lmax at x, Bonnet upwards in the order of ndpp_scatt_sample
void legendre_upto(int lmax, double x, double* P) {
  P[0] = 1.0;
  if (lmax >= 1) P[1] = x;
  for (int l = 1; l < lmax; ++l)
    P[l + 1] = (((double)(2 * l + 1) / (double)(l + 1)) * x) * P[l] - ((double)l / (double)(l + 1)) * P[l - 1];
}

// x P_l(x) - P_{l-1}(x): (x^2 - 1) P_l'(x) / l, the sign of -P_l' inside (-1, 1)
double dleg_sign(int l, double x) {
  double P[NDPP_MAX_ORDER + 2];
  legendre_upto(l, x, P);
  return x * P[l] - P[l - 1];
}

// the l - 1 roots of P_l' in (-1, 1), ascending: one between each two neighbouring roots of P_l
// (Newton from the usual cosine guess), found by bisection down to neighbouring doubles
std::vector<double> dleg_roots(int l) {
  std::vector<double> z((size_t)l), r;
  double P[NDPP_MAX_ORDER + 2];
  for (int i = 0; i < l; ++i) {
    double x = -std::cos(M_PI * ((double)i + 0.75) / ((double)l + 0.5));
    for (int it = 0; it < 100; ++it) {
      legendre_upto(l, x, P);
      const double d = (double)l * (x * P[l] - P[l - 1]) / (x * x - 1.0);
      const double dx = P[l] / d;
      x -= dx;
      if (std::fabs(dx) < 1e-16) break;
    }
    z[(size_t)i] = x;
  }
  for (int i = 0; i + 1 < l; ++i) {
    double a = z[(size_t)i], b = z[(size_t)i + 1];
    const bool up = dleg_sign(l, a) < 0.0;           // the sign at a; it changes once before b
    for (int it = 0; it < 200; ++it) {
      const double m = 0.5 * (a + b);
      if (!(a < m && m < b)) break;
      if ((dleg_sign(l, m) < 0.0) == up) a = m; else b = m;
    }
    r.push_back(0.5 * (a + b));
  }
  return r;
}

int check_rows(const char* who, long n, int G, int Lin, int Lout) {
  if (n < 0) return fail(NDPP_EINVAL, "%s: n=%ld (need n >= 0)", who, n);
  if (G < 1) return fail(NDPP_EINVAL, "%s: G=%d (need G >= 1)", who, G);
  int rc = check_gl_index(who, G, std::max(Lin, Lout));
  if (rc != NDPP_OK) return rc;
  size_t a, b;
  if (!bytes_of((size_t)n, (size_t)G * Lin, sizeof(double), &a) ||
      !bytes_of((size_t)n, (size_t)G * Lout, sizeof(double), &b))
    return fail(NDPP_EINVAL, "%s: n=%ld G=%d: the sizes overflow", who, n, G);
  return NDPP_OK;
}

int grid_of(long tiles) { return (int)std::max<long>(1, std::min<long>(tiles, kMaxGrid)); }

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_derive_tables(int L, int N, double* W, double* V, double* pmin, double* pmax) {
  if (L < 1 || L > NDPP_MAX_ORDER || N < 1 || N > NDPP_MAX_TAB_BINS)
    return fail(NDPP_EINVAL, "derive_tables: L=%d N=%d (need 1 <= L <= %d and 1 <= N <= %d)", L, N, NDPP_MAX_ORDER,
                NDPP_MAX_TAB_BINS);
  if (!W || !V || !pmin || !pmax) return fail(NDPP_EINVAL, "derive_tables: NULL argument");
  // P_0 .. P_L at the N + 1 edges
  std::vector<double> P((size_t)(N + 1) * (L + 1));
  for (int k = 0; k <= N; ++k) {
    const double e = k == N ? 1.0 : -1.0 + (2.0 * (double)k) / (double)N;
    legendre_upto(L, e, &P[(size_t)k * (L + 1)]);
  }
  auto p = [&](int l, int k) { return P[(size_t)k * (L + 1) + l]; };
  auto edge = [&](int k) { return k == N ? 1.0 : -1.0 + (2.0 * (double)k) / (double)N; };
  const double margin = 8.0 * DBL_EPSILON;
  for (int l = 0; l < L; ++l) {
    const std::vector<double> roots = l >= 2 ? dleg_roots(l) : std::vector<double>();
    std::vector<double> at_root(roots.size());
    double Pr[NDPP_MAX_ORDER + 2];
    for (size_t i = 0; i < roots.size(); ++i) {
      legendre_upto(l, roots[i], Pr);
      at_root[i] = Pr[l];
    }
    for (int k = 0; k < N; ++k) {
      const size_t at = (size_t)l * N + k;
      if (l == 0) {
        W[at] = (edge(k + 1) - edge(k)) / 2.0;
        V[at] = 1.0;
      } else {
        W[at] = ((p(l + 1, k + 1) - p(l - 1, k + 1)) - (p(l + 1, k) - p(l - 1, k))) / 2.0;
        V[at] = ((double)N * W[at]) / (double)(2 * l + 1);
      }
      double mn = std::min(p(l, k), p(l, k + 1)), mx = std::max(p(l, k), p(l, k + 1));
      for (size_t i = 0; i < roots.size(); ++i)
        if (roots[i] > edge(k) && roots[i] < edge(k + 1)) {
          mn = std::min(mn, at_root[i]);
          mx = std::max(mx, at_root[i]);
        }
      pmin[at] = mn - margin;
      pmax[at] = mx + margin;
    }
  }
  return NDPP_OK;
}

extern "C" int ndpp_derive_groups(long n, int G, int L, const double* mat, int Gc, const int* first, double* out) {
  if (L < 1) return fail(NDPP_EINVAL, "derive_groups: L=%d (need L >= 1)", L);
  int rc = check_rows("derive_groups", n, G, L, L);
  if (rc != NDPP_OK) return rc;
  if (Gc < 1 || Gc > G) return fail(NDPP_EINVAL, "derive_groups: Gc=%d (need 1 <= Gc <= G = %d)", Gc, G);
  if (!first) return fail(NDPP_EINVAL, "derive_groups: NULL argument");
  if (first[0] != 0 || first[Gc] != G)
    return fail(NDPP_EINVAL, "derive_groups: first[0]=%d first[Gc]=%d (need 0 and G = %d)", first[0], first[Gc], G);
  for (int c = 0; c < Gc; ++c)
    if (!(first[c] < first[c + 1]))
      return fail(NDPP_EINVAL, "derive_groups: first[%d]=%d first[%d]=%d: first must be strictly increasing", c,
                  first[c], c + 1, first[c + 1]);
  if (n > 0 && (!mat || !out)) return fail(NDPP_EINVAL, "derive_groups: NULL argument");
  if ((rc = require_device("derive_groups"))) return rc;
  if (n == 0) return NDPP_OK;

  const size_t GL = (size_t)G * L, GcL = (size_t)Gc * L;
  DevBuf<double> d_mat, d_out;
  DevBuf<int> d_first;
  NDPP_TRY(d_mat.upload(mat, (size_t)n * GL));
  NDPP_TRY(d_first.upload(first, (size_t)Gc + 1));
  NDPP_TRY(d_out.alloc((size_t)n * GcL));
  {
    GpuSpan span(nullptr, -1);
    const int staged = GL <= (size_t)kStageDoubles;
    // whole energies per tile: as many as fit the stage, at most 4 outputs per thread
    int epb = 1;
    if (staged) epb = (int)std::max<size_t>(1, std::min<size_t>(kStageDoubles / GL, (4 * kThreads + GcL - 1) / GcL));
    const long tiles = (n + epb - 1) / epb;
    const size_t shmem = staged ? (size_t)epb * GL * sizeof(double) : 0;
    hipLaunchKernelGGL(derive_groups_kernel, dim3(grid_of(tiles)), dim3(kThreads), shmem, 0, n, G, L, Gc, epb, staged,
                       d_mat.p, d_first.p, d_out.p);
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(d_out.download(out, (size_t)n * GcL));
  return NDPP_OK;
}

extern "C" int ndpp_derive_bins(long n, int G, int L, const double* mat, int N, double* out, int* status) {
  if (L < 1 || L > NDPP_MAX_ORDER || N < 1 || N > NDPP_MAX_TAB_BINS)
    return fail(NDPP_EINVAL, "derive_bins: L=%d N=%d (need 1 <= L <= %d and 1 <= N <= %d)", L, N, NDPP_MAX_ORDER,
                NDPP_MAX_TAB_BINS);
  int rc = check_rows("derive_bins", n, G, L, N);
  if (rc != NDPP_OK) return rc;
  if (n > 0 && (!mat || !out || !status)) return fail(NDPP_EINVAL, "derive_bins: NULL argument");
  if ((rc = require_device("derive_bins"))) return rc;
  if (n == 0) return NDPP_OK;

  const size_t LN = (size_t)L * N;
  std::vector<double> W(LN), V(LN), pmin(LN), pmax(LN);
  if ((rc = ndpp_derive_tables(L, N, W.data(), V.data(), pmin.data(), pmax.data()))) return rc;
  const long rows = n * (long)G;
  DevBuf<double> d_mat, d_W, d_out;
  DevBuf<int> d_status;
  NDPP_TRY(d_mat.upload(mat, (size_t)rows * L));
  NDPP_TRY(d_W.upload(W.data(), LN));
  NDPP_TRY(d_out.alloc((size_t)rows * N));
  NDPP_TRY(d_status.alloc((size_t)rows));
  {
    GpuSpan span(nullptr, -1);
    int T = 1;
    while (T < N && T < 64) T <<= 1;                  // the lanes of a row
    const int RB = kThreads / T, RT = std::max(RB, 32);
    const long tiles = (rows + RT - 1) / RT;
    const size_t shmem = (LN + (size_t)RT * L) * sizeof(double);
    dispatch_moments(L, [&](auto tag) {
      hipLaunchKernelGGL(derive_bins_kernel<decltype(tag)::value>, dim3(grid_of(tiles)), dim3(kThreads), shmem, 0,
                         rows, N, T, RT, d_mat.p, d_W.p, d_out.p, d_status.p);
    });
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(d_out.download(out, (size_t)rows * N));
  NDPP_TRY(d_status.download(status, (size_t)rows));
  return NDPP_OK;
}

extern "C" int ndpp_derive_moments(long n, int G, int N, const double* mat, int L, double* out, double* lo,
                                   double* hi, int* status) {
  if (L < 1 || L > NDPP_MAX_ORDER || N < 1 || N > NDPP_MAX_TAB_BINS)
    return fail(NDPP_EINVAL, "derive_moments: L=%d N=%d (need 1 <= L <= %d and 1 <= N <= %d)", L, N, NDPP_MAX_ORDER,
                NDPP_MAX_TAB_BINS);
  int rc = check_rows("derive_moments", n, G, N, L);
  if (rc != NDPP_OK) return rc;
  if (n > 0 && (!mat || !out || !status)) return fail(NDPP_EINVAL, "derive_moments: NULL argument");
  if ((rc = require_device("derive_moments"))) return rc;
  if (n == 0) return NDPP_OK;

  const size_t LN = (size_t)L * N;
  std::vector<double> W(LN), V(LN), pmin(LN), pmax(LN);
  if ((rc = ndpp_derive_tables(L, N, W.data(), V.data(), pmin.data(), pmax.data()))) return rc;
  const long rows = n * (long)G;
  const bool bounds = lo || hi;
  DevBuf<double> d_mat, d_V, d_min, d_max, d_out, d_lo, d_hi;
  DevBuf<int> d_status;
  NDPP_TRY(d_mat.upload(mat, (size_t)rows * N));
  NDPP_TRY(d_V.upload(V.data(), LN));
  if (bounds) {
    NDPP_TRY(d_min.upload(pmin.data(), LN));
    NDPP_TRY(d_max.upload(pmax.data(), LN));
  }
  NDPP_TRY(d_out.alloc((size_t)rows * L));
  if (lo) NDPP_TRY(d_lo.alloc((size_t)rows * L));
  if (hi) NDPP_TRY(d_hi.alloc((size_t)rows * L));
  NDPP_TRY(d_status.alloc((size_t)rows));
  {
    GpuSpan span(nullptr, -1);
    const int RT = std::max(8, std::min(256, 2048 / N));    // 16 KB of staged bins at most
    const long tiles = (rows + RT - 1) / RT;
    const size_t shmem = ((bounds ? 3 : 1) * LN + (size_t)RT * (N + 1)) * sizeof(double) + (size_t)RT * L * sizeof(int);
    // a block loads up to 34 KB of tables for tiles of 16 KB: few blocks, many tiles each
    const int grid = std::min(grid_of(tiles), 4096);
    if (bounds)
      hipLaunchKernelGGL(derive_moments_kernel<true>, dim3(grid), dim3(kThreads), shmem, 0, rows, N, L, RT,
                         d_mat.p, d_V.p, d_min.p, d_max.p, d_out.p, d_lo.p, d_hi.p, d_status.p);
    else
      hipLaunchKernelGGL(derive_moments_kernel<false>, dim3(grid), dim3(kThreads), shmem, 0, rows, N, L, RT,
                         d_mat.p, d_V.p, (const double*)nullptr, (const double*)nullptr, d_out.p, (double*)nullptr,
                         (double*)nullptr, d_status.p);
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(d_out.download(out, (size_t)rows * L));
  if (lo) NDPP_TRY(d_lo.download(lo, (size_t)rows * L));
  if (hi) NDPP_TRY(d_hi.download(hi, (size_t)rows * L));
  NDPP_TRY(d_status.download(status, (size_t)rows));
  return NDPP_OK;
}
