// section_util.h -- what the analyses of a finished library share: expand_kernels.hip (sampled
// positivity), minimum_kernels.hip (certified minimum), grid_kernels.hip (midpoint check),
// compare_kernels.hip (two libraries) and thin_kernels.hip (error-bounded thinning); sample_kernels.hip
// (sampling) takes its bracket and its grid checks from here.  The rules below
// are defined HERE, once; the files describe their own layout and point to this header.
//
// The band of an incoming energy: its groups from the first to the last with P0 > 0.  Only these rows
// are examined; an energy without any P0 > 0 counts as one zero row at g = 0 (ndpp_hip.h).
//
// The block shape of the kernels that take one thread per (E_in, group) row: a block holds whole
// incoming energies (so that it finds their bands by itself) on at most kMaxBlock threads.
//
// The scale-relative metric of a row (or of the rows interpolated at one energy) against another:
//   d(e)  = | difference at element e |
//   scale = max_g |P0| over the rows that take part
//   err   = max_e d(e) / scale     0 when the scale is 0, +inf when a d(e) is NaN or infinite
//   arg   = the lowest e attaining the maximum; the first e that is not finite when err = +inf
// The absolute error over the row's scale, not an element-wise relative error: the moments of a
// row pass through zero.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "kernels.h"

namespace ndpp {

// ---- host ------------------------------------------------------------------------------------

// a * b * c bytes without overflow (and below 2^62, so that every signed index fits)
inline bool bytes_of(size_t a, size_t b, size_t c, size_t* out) {
  size_t ab;
  return !__builtin_mul_overflow(a, b, &ab) && !__builtin_mul_overflow(ab, c, out) && *out < ((size_t)1 << 62);
}

constexpr int kMaxBlock = 512;        // a block of rows: at most 8 waves

// incoming energies per block and the block size: whole energies per block, as few idle lanes as
// possible (G = 7: 64 energies on 448 threads; G = 70: 7 on 512 -> 490 rows)
inline void block_shape(int G, int* epb, int* threads) {
  int best_e = 1, best_b = kMaxBlock;
  double best_waste = 2.0;
  const int emax = std::max(1, kMaxBlock / G);
  for (int e = 1; e <= emax; ++e) {
    const long R = (long)e * G;
    const long passes = (R + kMaxBlock - 1) / kMaxBlock;
    const long b = ((R + passes - 1) / passes + 63) / 64 * 64;
    const double waste = (double)(passes * b - R) / (double)(passes * b);
    if (waste <= best_waste) { best_waste = waste; best_e = e; best_b = (int)b; }
  }
  *epb = best_e;
  *threads = best_b;
}

// an incoming-energy grid x[n] called `name` in the messages of entry point `who`
inline int check_energy_grid(const char* who, const char* name, int n, const double* x) {
  for (int i = 0; i < n; ++i)
    if (!(std::isfinite(x[i]) && x[i] > 0.0 && (i == 0 || x[i] > x[i - 1])))
      return fail(NDPP_EINVAL, "%s: %s[%d] = %.17g: %s must be strictly increasing, positive and finite", who,
                  name, i, x[i], name);
  return NDPP_OK;
}

// an element of a row of G * L doubles (and twice that) is indexed by an int
inline int check_gl_index(const char* who, int G, int L) {
  if ((long)G * L > INT_MAX / 2) return fail(NDPP_EINVAL, "%s: G * L = %ld does not fit an index", who, (long)G * L);
  return NDPP_OK;
}

// the weight of row x1 at xm in [x0, x1], linear in ln E (the rule thin_grid assumes, thin.hip)
inline double lne_weight(double x0, double x1, double xm) { return std::log(xm / x0) / std::log(x1 / x0); }

// the rows a consumer reads at v inside [x[0], x[n-1]] (ndpp_lib_compare, ndpp_scatt_sample): the
// largest i with x[i] <= v, and the weight of row i + 1
inline void bracket(int n, const double* x, double v, int* i_out, double* f_out) {
  const int i = (int)(std::upper_bound(x, x + n, v) - x) - 1;
  *i_out = i;
  *f_out = (v == x[i] || i == n - 1) ? 0.0 : lne_weight(x[i], x[i + 1], v);
}

// closes the span of an entry point's kernels and waits for them; a failure returns from the
// entry point through NDPP_TRY, which names the call that failed
#define NDPP_CLOSE_SPAN(span)           \
  do {                                  \
    (span).end();                       \
    NDPP_TRY(hipGetLastError());        \
    NDPP_TRY(hipDeviceSynchronize());   \
  } while (0)

// ---- device ----------------------------------------------------------------------------------

// The bands of the block's ne incoming energies e0 .. e0 + ne - 1 of mat[.][G][L], left in
// s_gmin[e], s_gmax[e] (gmin > gmax: no P0 > 0), found from the P0 values the block reads anyway.
// Called by every thread of the block; the arrays are readable when it returns.
__device__ inline void block_band(const double* __restrict__ mat, long e0, int ne, int G, int L, int* s_gmin,
                                  int* s_gmax) {
  const int tid = threadIdx.x, B = blockDim.x, R = ne * G;
  for (int e = tid; e < ne; e += B) { s_gmin[e] = G; s_gmax[e] = -1; }
  __syncthreads();
  for (int r = tid; r < R; r += B) {
    const int e = r / G, g = r - e * G;
    if (mat[(size_t)(e0 * G + r) * L] > 0.0) { atomicMin(&s_gmin[e], g); atomicMax(&s_gmax[e], g); }
  }
  __syncthreads();
}

// d / scale of the metric for one value
__device__ inline double rel_err(double d, double scale) {
  return !(d < INFINITY) ? INFINITY : (scale == 0.0 ? 0.0 : d / scale);
}

// The metric over the elements a wave64 strides across: every lane take()s its elements in
// ascending order and raises `scale` on the P0 elements, fold() leaves the wave's result in every
// lane ("larger value, then lower index"), and lane 0 write()s it.  No LDS, no atomics.
struct WaveMax {
  double dmax = -1.0, scale = 0.0;
  int imax = INT_MAX, ibad = INT_MAX;
  __device__ void take(int e, double d) {
    if (!(d < INFINITY)) { if (e < ibad) ibad = e; }    // NaN or infinite
    else if (d > dmax) { dmax = d; imax = e; }
  }
  __device__ void fold() {
    for (int o = 32; o > 0; o >>= 1) {
      const double v = __shfl_xor(dmax, o);
      const int k = __shfl_xor(imax, o);
      if (v > dmax || (v == dmax && k < imax)) { dmax = v; imax = k; }
      ibad = min(ibad, __shfl_xor(ibad, o));
      scale = fmax(scale, __shfl_xor(scale, o));
    }
  }
  __device__ void write(double* err, int* arg) const {
    if (ibad != INT_MAX) { *err = INFINITY; *arg = ibad; }
    else { *err = scale == 0.0 ? 0.0 : dmax / scale; *arg = imax; }
  }
};

}  // namespace ndpp
