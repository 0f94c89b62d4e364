// expand_kernels.hip -- library validation on the device: the truncated Legendre expansion
//   f(mu_j) = sum_{l < n_mom} (l + 1/2) P_l(mu_j) a_l
// of stored scattering moments, and the positivity check over whole matrix sections.
// Replaces the Python loops of the reference's src/utils/ndpp_data.py:305-343 (expand_scatt)
// and :345-396 (test_scatt_positivity); the rules (band, zero rows, NaN) are in ndpp_hip.h.
//
// Both kernels take the basis B[j][l] = (l + 1/2) P_l(mu_j), computed once per call on the
// host from the closed forms pn_rt (ndpp_math.h, the reference's calc_pn), and evaluate
//   f = B[j][0] a_0;  f = fma(B[j][l], a_l, f)  for l = 1 .. n_mom-1
// -- one fixed operation sequence, so expand and positivity agree bit for bit and every
// call repeats its bits.
//
// Positivity: one thread per (E_in, group) row, its n_mom moments in VGPRs; the lanes of a
// wave walk the mu grid in lockstep, so B[j][*] is wave-uniform and is read by scalar loads
// into SGPRs (the operand v_fma_f64 takes for free).  Per (row, mu): n_mom FMAs, one min, one
// add (the NaN witness).  A block holds whole incoming energies (block_shape, section_util.h), so
// the band is found in LDS from the P0 values the block reads anyway (block_band).  Offending rows
// are compacted in (iE, g) order per block (ballot + wave offsets), then a one-block kernel
// scans the per-block counts and folds the summary, and a gather copies the first `cap`
// offenders to the output.  Nothing of size rows x M touches memory.
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "ndpp_math.h"
#include "section_util.h"

namespace ndpp {
namespace {

constexpr int kFinalThreads = 1024;

struct PosPart {                      // per-block partial of the summary
  long rows, neg;
  double vmin;                        // smallest non-NaN row minimum (+inf if none)
  long key;                           // (iE, g) of it as iE * (G + 1) + g + 1 (g = -1: zero row)
};

struct PosSum {
  long rows, neg;
  double vmin;
  long key;
};

__device__ inline bool better(double v, long k, double bv, long bk) {
  return v < bv || (v == bv && k < bk);
}

// f(mu_j) of one row: the fixed operation sequence of the file header
template <int NM>
__device__ inline double expand_at(const double* __restrict__ b, const double (&a)[NM]) {
  double f = b[0] * a[0];
#pragma unroll
  for (int l = 1; l < NM; ++l) f = __builtin_fma(b[l], a[l], f);
  return f;
}

template <int NM>
__global__ void __launch_bounds__(kMaxBlock)
positivity_kernel(int n_ein, int G, int L, int epb, const double* __restrict__ mat, int n_mu,
                  const double* __restrict__ basis, PosPart* __restrict__ part, int* __restrict__ cand_row,
                  double* __restrict__ cand_min, int* __restrict__ cand_mu) {
  __shared__ int s_gmin[kMaxBlock], s_gmax[kMaxBlock];
  __shared__ int s_wc[kMaxBlock / 64];
  __shared__ long s_rows[kMaxBlock / 64], s_key[kMaxBlock / 64];
  __shared__ double s_vmin[kMaxBlock / 64];
  const int tid = threadIdx.x, B = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = (B + 63) >> 6;
  const long e0 = (long)blockIdx.x * epb;
  const int ne = (int)min((long)epb, (long)n_ein - e0);
  const int R = ne * G;
  const long slot0 = (long)blockIdx.x * epb * G;     // this block's region of the candidate arrays

  block_band(mat, e0, ne, G, L, s_gmin, s_gmax);

  long rows = 0, kmin = LONG_MAX;
  double vmin = INFINITY;
  int found = 0;                          // offenders of this block so far
  for (int r0 = 0; r0 < R; r0 += B) {     // same trip count for every thread of the block
    const int r = r0 + tid;
    bool neg = false;
    double rmin = 0.0;
    int rmu = 0, e = 0, g = 0;
    if (r < R) {
      e = r / G;
      g = r - e * G;
      const int gmin = s_gmin[e], gmax = s_gmax[e];
      const long iE = e0 + e;
      if (gmin > gmax) {                  // no P0 > 0: one zero row, min 0.0, never negative
        if (g == 0) {
          ++rows;
          if (better(0.0, iE * (G + 1), vmin, kmin)) { vmin = 0.0; kmin = iE * (G + 1); }
        }
      } else if (g >= gmin && g <= gmax) {
        ++rows;
        const double* row = mat + (size_t)(e0 * G + r) * L;
        double a[NM];
#pragma unroll
        for (int l = 0; l < NM; ++l) a[l] = row[l];
        double m = INFINITY, witness = 0.0;
#pragma unroll 2
        for (int j = 0; j < n_mu; ++j) {
          const double f = expand_at<NM>(basis + (size_t)j * NM, a);
          m = fmin(m, f);                 // NaN-ignoring
          witness += f;                   // NaN if any f is NaN (or +inf meets -inf: negative anyway)
        }
        neg = !(m >= 0.0) || witness != witness;
        if (m == m && m != INFINITY) {
          const long k = iE * (G + 1) + g + 1;
          if (better(m, k, vmin, kmin)) { vmin = m; kmin = k; }
        }
        if (neg) {                        // rare: find the first mu attaining the minimum
          rmin = NAN;
          for (int j = 0; j < n_mu; ++j) {
            const double f = expand_at<NM>(basis + (size_t)j * NM, a);
            if (f == m) { rmin = m; rmu = j; break; }
          }
        }
      }
    }
    // ordered compaction of this pass's offenders into the block's region
    const unsigned long long bal = __ballot(neg);
    if (lane == 0) s_wc[wave] = __popcll(bal);
    __syncthreads();
    int off = found, tot = 0;
    for (int w = 0; w < nw; ++w) {
      if (w < wave) off += s_wc[w];
      tot += s_wc[w];
    }
    if (neg) {
      const long at = slot0 + off + __popcll(bal & ((1ull << lane) - 1ull));
      cand_row[2 * at] = (int)(e0 + e);
      cand_row[2 * at + 1] = g;
      cand_min[at] = rmin;
      cand_mu[at] = rmu;
    }
    found += tot;
    __syncthreads();                      // s_wc is rewritten by the next pass
  }

  // block partials: rows (sum), (vmin, key) lexicographic minimum
  for (int o = 32; o > 0; o >>= 1) {
    rows += __shfl_xor(rows, o);
    const double v = __shfl_xor(vmin, o);
    const long k = __shfl_xor(kmin, o);
    if (better(v, k, vmin, kmin)) { vmin = v; kmin = k; }
  }
  if (lane == 0) { s_rows[wave] = rows; s_vmin[wave] = vmin; s_key[wave] = kmin; }
  __syncthreads();
  if (tid == 0) {
    PosPart p{0, found, INFINITY, LONG_MAX};
    for (int w = 0; w < nw; ++w) {
      p.rows += s_rows[w];
      if (better(s_vmin[w], s_key[w], p.vmin, p.key)) { p.vmin = s_vmin[w]; p.key = s_key[w]; }
    }
    part[blockIdx.x] = p;
  }
}

// one block: exclusive scan of the per-block offender counts (-> boff) and the summary
__global__ void __launch_bounds__(kFinalThreads)
positivity_final(int nblk, const PosPart* __restrict__ part, long* __restrict__ boff, PosSum* __restrict__ sum) {
  __shared__ long s_neg[kFinalThreads], s_rows[kFinalThreads], s_key[kFinalThreads];
  __shared__ double s_vmin[kFinalThreads];
  const int t = threadIdx.x;
  const int chunk = (nblk + kFinalThreads - 1) / kFinalThreads;
  const int b0 = min(nblk, t * chunk), b1 = min(nblk, b0 + chunk);
  long neg = 0, rows = 0, key = LONG_MAX;
  double vmin = INFINITY;
  for (int b = b0; b < b1; ++b) {
    const PosPart p = part[b];
    neg += p.neg;
    rows += p.rows;
    if (better(p.vmin, p.key, vmin, key)) { vmin = p.vmin; key = p.key; }
  }
  s_neg[t] = neg; s_rows[t] = rows; s_vmin[t] = vmin; s_key[t] = key;
  __syncthreads();
  if (t == 0) {
    PosSum s{0, 0, INFINITY, LONG_MAX};
    for (int k = 0; k < kFinalThreads; ++k) {
      const long n = s_neg[k];
      s_neg[k] = s.neg;                   // exclusive prefix
      s.neg += n;
      s.rows += s_rows[k];
      if (better(s_vmin[k], s_key[k], s.vmin, s.key)) { s.vmin = s_vmin[k]; s.key = s_key[k]; }
    }
    *sum = s;
  }
  __syncthreads();
  long at = s_neg[t];
  for (int b = b0; b < b1; ++b) {
    boff[b] = at;
    at += part[b].neg;
  }
}

// block b copies its offenders to positions boff[b] ... of the output, those below cap
__global__ void positivity_gather(long slot_stride, long cap, const PosPart* __restrict__ part,
                                  const long* __restrict__ boff, const int* __restrict__ cand_row,
                                  const double* __restrict__ cand_min, const int* __restrict__ cand_mu,
                                  int* __restrict__ out_row, double* __restrict__ out_min, int* __restrict__ out_mu) {
  const long n = part[blockIdx.x].neg, o = boff[blockIdx.x];
  const long src0 = (long)blockIdx.x * slot_stride;
  for (long i = threadIdx.x; i < n && o + i < cap; i += blockDim.x) {
    const long s = src0 + i, d = o + i;
    out_row[2 * d] = cand_row[2 * s];
    out_row[2 * d + 1] = cand_row[2 * s + 1];
    out_min[d] = cand_min[s];
    out_mu[d] = cand_mu[s];
  }
}

template <int NM>
__global__ void expand_kernel(long total, int n_mu, int L, const double* __restrict__ mom,
                              const double* __restrict__ basis, double* __restrict__ out) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long iE = t / n_mu;
    const int j = (int)(t - iE * n_mu);
    double a[NM];
#pragma unroll
    for (int l = 0; l < NM; ++l) a[l] = mom[iE * L + l];
    out[t] = expand_at<NM>(basis + (size_t)j * NM, a);
  }
}

// B[j][l] = (l + 1/2) P_l(mu_j), the basis of both kernels (nm <= NDPP_MAX_ORDER = 11, so l <= 10 and
// pn_rt's default branch is not reached)
std::vector<double> make_basis(int n_mu, const double* mu, int nm) {
  std::vector<double> b((size_t)n_mu * nm);
  for (int j = 0; j < n_mu; ++j)
    for (int l = 0; l < nm; ++l) b[(size_t)j * nm + l] = ((double)l + 0.5) * pn_rt(l, mu[j]);
  return b;
}

// the checks shared by both entry points (ndpp_hip.h)
int check_common(const char* who, int L, int n_moments, int n_mu, const double* mu) {
  if (L < 1 || L > NDPP_MAX_ORDER) return fail(NDPP_EINVAL, "%s: L=%d outside 1..%d", who, L, NDPP_MAX_ORDER);
  if (n_moments < 1 || n_moments > L) return fail(NDPP_EINVAL, "%s: n_moments=%d outside 1..L=%d", who, n_moments, L);
  if (n_mu < 1) return fail(NDPP_EINVAL, "%s: n_mu=%d, need at least one mu point", who, n_mu);
  if (!mu) return fail(NDPP_EINVAL, "%s: NULL mu", who);
  return NDPP_OK;
}

// the grid itself, read only once every size has been checked
int check_mu(const char* who, int n_mu, const double* mu) {
  for (int j = 0; j < n_mu; ++j)
    if (!std::isfinite(mu[j]) || mu[j] < -1.0 || mu[j] > 1.0)
      return fail(NDPP_EINVAL, "%s: mu[%d]=%g is not a finite value in [-1, 1]", who, j, mu[j]);
  return NDPP_OK;
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_scatt_positivity(int n_ein, int G, int L, const double* mat, int n_moments, int n_mu,
                                     const double* mu, long cap, int* neg_rows, double* neg_min, int* neg_mu,
                                     ndpp_positivity* summary) {
  int rc = check_common("scatt_positivity", L, n_moments, n_mu, mu);
  if (rc) return rc;
  if (n_ein < 0 || G < 1) return fail(NDPP_EINVAL, "scatt_positivity: n_ein=%d G=%d", n_ein, G);
  if (!mat || !summary) return fail(NDPP_EINVAL, "scatt_positivity: NULL mat or summary");
  if (cap < 0) return fail(NDPP_EINVAL, "scatt_positivity: cap=%ld < 0", cap);
  if (cap > 0 && !neg_rows) return fail(NDPP_EINVAL, "scatt_positivity: NULL neg_rows with cap=%ld", cap);
  size_t mat_bytes = 0, row_bytes = 0, cap_bytes = 0;
  if (!bytes_of((size_t)n_ein, (size_t)G, (size_t)L * sizeof(double), &mat_bytes) ||
      !bytes_of((size_t)n_ein, (size_t)G, 2 * sizeof(int) + sizeof(double) + sizeof(int), &row_bytes) ||
      !bytes_of((size_t)cap, 2, sizeof(int), &cap_bytes))
    return fail(NDPP_EINVAL, "scatt_positivity: sizes overflow (n_ein=%d G=%d L=%d cap=%ld)", n_ein, G, L, cap);
  if ((rc = check_mu("scatt_positivity", n_mu, mu))) return rc;
  *summary = ndpp_positivity{0, 0, INFINITY, -1, -1};
  if (n_ein == 0) return NDPP_OK;
  if ((rc = require_device())) return rc;

  const std::vector<double> basis = make_basis(n_mu, mu, n_moments);
  int epb = 1, threads = 64;
  block_shape(G, &epb, &threads);
  const int nblk = (n_ein + epb - 1) / epb;
  const long slot_stride = (long)epb * G;
  const long slots = (long)nblk * slot_stride;
  const long n_out_max = std::min<long>(cap, (long)n_ein * G);
  DevBuf<double> d_mat, d_basis, d_cmin, d_omin;
  DevBuf<int> d_crow, d_cmu, d_orow, d_omu;
  DevBuf<PosPart> d_part;
  DevBuf<long> d_boff;
  DevBuf<PosSum> d_sum;
  NDPP_TRY(d_mat.upload(mat, (size_t)n_ein * G * L));
  NDPP_TRY(d_basis.upload(basis.data(), basis.size()));
  NDPP_TRY(d_crow.alloc(2 * (size_t)slots));
  NDPP_TRY(d_cmin.alloc(slots));
  NDPP_TRY(d_cmu.alloc(slots));
  NDPP_TRY(d_part.alloc(nblk));
  NDPP_TRY(d_boff.alloc(nblk));
  NDPP_TRY(d_sum.alloc(1));
  NDPP_TRY(d_orow.alloc(2 * (size_t)n_out_max));
  NDPP_TRY(d_omin.alloc(n_out_max));
  NDPP_TRY(d_omu.alloc(n_out_max));
  {
    GpuSpan span(nullptr, -1);
    dispatch_moments(n_moments, [&](auto nm) {
      hipLaunchKernelGGL(positivity_kernel<decltype(nm)::value>, dim3(nblk), dim3(threads), 0, 0, n_ein, G, L, epb, d_mat.p, n_mu,
                         d_basis.p, d_part.p, d_crow.p, d_cmin.p, d_cmu.p);
    });
    hipLaunchKernelGGL(positivity_final, dim3(1), dim3(kFinalThreads), 0, 0, nblk, d_part.p, d_boff.p, d_sum.p);
    if (n_out_max > 0)
      hipLaunchKernelGGL(positivity_gather, dim3(nblk), dim3(256), 0, 0, slot_stride, n_out_max, d_part.p,
                         d_boff.p, d_crow.p, d_cmin.p, d_cmu.p, d_orow.p, d_omin.p, d_omu.p);
    NDPP_CLOSE_SPAN(span);
  }
  PosSum s;
  NDPP_TRY(hipMemcpy(&s, d_sum.p, sizeof(s), hipMemcpyDeviceToHost));
  const long n_out = std::min<long>(n_out_max, s.neg);
  if (n_out > 0) {
    NDPP_TRY(hipMemcpy(neg_rows, d_orow.p, 2 * sizeof(int) * n_out, hipMemcpyDeviceToHost));
    if (neg_min) NDPP_TRY(hipMemcpy(neg_min, d_omin.p, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    if (neg_mu) NDPP_TRY(hipMemcpy(neg_mu, d_omu.p, sizeof(int) * n_out, hipMemcpyDeviceToHost));
  }
  summary->rows = s.rows;
  summary->negative = s.neg;
  summary->min_value = s.vmin;
  if (s.key != LONG_MAX) {
    summary->min_ein = (int)(s.key / (G + 1));
    summary->min_group = (int)(s.key % (G + 1)) - 1;
  }
  return NDPP_OK;
}

extern "C" int ndpp_expand_moments(int n_ein, int L, const double* moments, int n_moments, int n_mu,
                                   const double* mu, double* out) {
  int rc = check_common("expand_moments", L, n_moments, n_mu, mu);
  if (rc) return rc;
  if (n_ein < 0) return fail(NDPP_EINVAL, "expand_moments: n_ein=%d", n_ein);
  if (!moments || !out) return fail(NDPP_EINVAL, "expand_moments: NULL moments or out");
  size_t mom_bytes = 0, out_bytes = 0;
  if (!bytes_of((size_t)n_ein, (size_t)L, sizeof(double), &mom_bytes) ||
      !bytes_of((size_t)n_ein, (size_t)n_mu, sizeof(double), &out_bytes))
    return fail(NDPP_EINVAL, "expand_moments: sizes overflow (n_ein=%d L=%d n_mu=%d)", n_ein, L, n_mu);
  if ((rc = check_mu("expand_moments", n_mu, mu))) return rc;
  if (n_ein == 0) return NDPP_OK;
  if ((rc = require_device())) return rc;

  const std::vector<double> basis = make_basis(n_mu, mu, n_moments);
  const long total = (long)n_ein * n_mu;
  DevBuf<double> d_mom, d_basis, d_out;
  NDPP_TRY(d_mom.upload(moments, (size_t)n_ein * L));
  NDPP_TRY(d_basis.upload(basis.data(), basis.size()));
  NDPP_TRY(d_out.alloc(total));
  {
    GpuSpan span(nullptr, -1);
    dispatch_moments(n_moments, [&](auto nm) {
      hipLaunchKernelGGL(expand_kernel<decltype(nm)::value>, dim3(nblk(total, 256)), dim3(256), 0, 0, total, n_mu, L, d_mom.p,
                         d_basis.p, d_out.p);
    });
    NDPP_CLOSE_SPAN(span);
  }
  NDPP_TRY(hipMemcpy(out, d_out.p, sizeof(double) * total, hipMemcpyDeviceToHost));
  return NDPP_OK;
}
