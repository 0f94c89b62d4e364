// score_kernels.hip -- the expected-value consumer of a section (include/ndpp_hip.h: ndpp_scatt_score,
// DESIGN.md section 19): at every collision the whole [G][L] row, read linearly in ln E, is added,
// times the event's factor, to the tally bin the caller names.  Nothing in the reference does this.
//
// The sum order is part of the definition (the bits depend on it), so there are no atomics: the
// scored events of a bin, in ascending event index, are cut into chunks of NDPP_SCORE_CHUNK, a chunk
// is summed sequentially into a partial, and a bin's partials are summed sequentially into the tally.
// The kernels are + - * / and comparisons only, built without contraction, in the order ndpp_hip.h
// writes out, so a host restatement gives the same bits (ndpp_amd/score.py: score_numpy).
//
// Host: bracket and classify the events (bracket, section_util.h; on up to 16 host threads from
// 65536 events on, every event for itself), group the scored ones by bin with a stable counting
// sort, build the chunk table.  With normalize = 1 the statuses BADROW and ZEROROW come from the
// device (score_factor_kernel) before the grouping, because an event that is not scored takes no
// place in a chunk.  So there are two uploads, not one: the section and the events in event order
// (row, f, weight) first, then the sorted order and the chunk table; and the record of a scored
// event (row, f, v, band) is not built on the host but by score_gather_kernel from those arrays,
// which keeps one path for both values of normalize -- v exists only on the device when it is
// weight / W.
//
// score_rows_kernel     one thread per (stored row, group): the group's mass (sample_mass_kernel's
//                       rule) and whether any of its L elements is not exactly 0.0
// score_band_kernel     one thread per stored row: the first and the last group with such an element.
//                       NOT the P0 > 0 band of section_util.h: a group with P0 == 0 and P1 != 0 counts
// score_factor_kernel   normalize = 1, one thread per event: W as in step 2 of ndpp_scatt_sample
//                       (over the groups of the two rows' bands: the others add +-0.0), the status,
//                       v = weight / W
// score_gather_kernel   one thread per scored event in sorted order: its record (row, f, v and the
//                       union of its two rows' bands; every group when v is not finite)
// score_chunk_kernel    a lane owns one element e of one chunk and runs over the chunk's events in
//                       order: no cross-lane reduction, no LDS, no atomics.  Element G L is the
//                       chunk's sum of v.  A "unit" is (chunk, tile of W elements), W lanes wide; a
//                       block holds 256 / W units, tiles fastest, so that the waves of a block read
//                       the same records.  W = 64 when G L + 1 > 32: the record is then one address
//                       per wave, y[i][e] and y[i1][e] are coalesced, and a wave visits only the
//                       events whose band reaches its tile (a ballot over 64 records at a time).
//                       Smaller rows take the power of two that holds them, several chunks per
//                       wave (G = 2, L = 6: 16 lanes).
// score_fold_kernel     one thread per (bin, element), over the bin's chunks of this pass in
//                       ascending order, continuing tally = tally + partial across passes
//
// The partials are taken in passes over ascending chunk ranges under NDPP_SCORE_PARTIAL_MB (default
// 256).  The rows of a section are a few MB and stay in the L2 / the Infinity Cache across chunks.
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"
#include "section_util.h"

namespace ndpp {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = NDPP_SCORE_CHUNK;

struct ScoreRec {
  double f, v;
  int row, lo, hi, pad;
};

__device__ inline double blend(double v0, double v1, double f) { return v0 + (v1 - v0) * f; }
// negative, NaN or infinite
__device__ inline bool bad_mass(double v) { return !(v >= 0.0) || !(v < INFINITY); }

__global__ void __launch_bounds__(kThreads)
score_rows_kernel(long rows, int L, int tabular, const double* __restrict__ y, double* __restrict__ s,
                  int* __restrict__ nz) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    const double* p = y + (size_t)r * L;
    double m = p[0];
    if (tabular) {
      m = 0.0;
      for (int k = 0; k < L; ++k) m = m + p[k];
    }
    int any = 0;
    for (int k = 0; k < L; ++k) any |= (p[k] != 0.0);      // a NaN is not zero, -0.0 is
    s[r] = m;
    nz[r] = any;
  }
}

__global__ void __launch_bounds__(kThreads)
score_band_kernel(int n, int G, const int* __restrict__ nz, int* __restrict__ blo, int* __restrict__ bhi) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    int lo = G, hi = -1;                                   // lo > hi: the row is all zero
    for (int g = 0; g < G; ++g)
      if (nz[(size_t)r * G + g]) {
        lo = min(lo, g);
        hi = g;
      }
    blo[r] = lo;
    bhi[r] = hi;
  }
}

__global__ void __launch_bounds__(kThreads)
score_factor_kernel(long n_ev, int G, int n, int use_band, const double* __restrict__ s, const int* __restrict__ row,
                    const double* __restrict__ wt, const double* __restrict__ weight, const int* __restrict__ blo,
                    const int* __restrict__ bhi, double* __restrict__ v, int* __restrict__ status) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_ev; e += stride) {
    const int i = row[e];
    int st = NDPP_SCORE_SKIPPED;
    double val = 0.0;
    if (i >= 0) {
      const int i1 = min(i + 1, n - 1);
      const double f = wt[e];
      const double* s0 = s + (size_t)i * G;
      const double* s1 = s + (size_t)i1 * G;
      // outside the two rows' bands both masses are +-0.0, w_g is, and W (from +0.0) keeps its bits
      const int g0 = use_band ? min(blo[i], blo[i1]) : 0, g1 = use_band ? max(bhi[i], bhi[i1]) : G - 1;
      double W = 0.0;
      bool bad = false;
      for (int g = g0; g <= g1; ++g) {
        const double w = blend(s0[g], s1[g], f);
        bad = bad || bad_mass(w);
        W = W + w;
      }
      if (bad || !(W < INFINITY)) st = NDPP_SCORE_BADROW;
      else if (W == 0.0) st = NDPP_SCORE_ZEROROW;
      else {
        st = NDPP_SCORE_OK;
        val = weight[e] / W;
      }
    }
    v[e] = val;
    status[e] = st;
  }
}

__global__ void __launch_bounds__(kThreads)
score_gather_kernel(long n_sc, int G, int n, int use_band, const long* __restrict__ perm, const int* __restrict__ row,
                    const double* __restrict__ wt, const double* __restrict__ v, const int* __restrict__ blo,
                    const int* __restrict__ bhi, ScoreRec* __restrict__ rec) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n_sc; k += stride) {
    const long e = perm[k];
    const int i = row[e], i1 = min(i + 1, n - 1);
    ScoreRec r;
    r.f = wt[e];
    r.v = v[e];
    r.row = i;
    r.lo = min(blo[i], blo[i1]);
    r.hi = max(bhi[i], bhi[i1]);
    if (!use_band || !(fabs(r.v) < INFINITY)) {      // inf * 0 is a NaN: nothing is skipped
      r.lo = 0;
      r.hi = G - 1;
    }
    r.pad = 0;
    rec[k] = r;
  }
}

// partial[(c - c0) * (GL + 1) + e] for the chunks c0 <= c < c0 + nc; cstart[c] .. cstart[c + 1] are the
// chunk's records.  W lanes per unit, a power of two <= 64; tiles = ceil((GL + 1) / W).
// W = 64: the wave first asks, 64 records at a time (one per lane), which events' bands reach its
// tile at all, and then walks only those, in ascending order -- the order of the sum does not change,
// an event outside the tile's groups would have added nothing in any lane.
__global__ void __launch_bounds__(kThreads)
score_chunk_kernel(long c0, long nc, int G, int L, int n, int W, int tiles, const double* __restrict__ y,
                   const ScoreRec* __restrict__ rec, const long* __restrict__ cstart, double* __restrict__ partial) {
  const int GL = G * L;
  long u = (long)blockIdx.x * (kThreads / W) + threadIdx.x / W;
  if (W == 64) u = ((long)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
                   (unsigned)__builtin_amdgcn_readfirstlane((int)u);      // one unit per wave: scalar record reads
  const long cl = u / tiles;
  if (cl >= nc) return;                                  // (the whole wave when W = 64)
  const int tile = (int)(u - cl * tiles);
  const int e = tile * W + (threadIdx.x & (W - 1));
  const bool live = e <= GL;
  const int g = e / L;                                   // (G for the sum of v: never inside a band)
  const long k0 = cstart[c0 + cl], k1 = cstart[c0 + cl + 1];
  double acc = 0.0;
  if (W == 64) {
    const int lane = threadIdx.x & 63;
    const int e_last = min(tile * 64 + 63, GL);
    const bool all = e_last == GL;                       // the tile that holds the sum of v takes every event
    const int g_lo = (tile * 64) / L, g_hi = min(e_last, GL - 1) / L;
    for (long kb = k0; kb < k1; kb += 64) {
      bool hit = false;
      if (kb + lane < k1) hit = all || (g_lo <= rec[kb + lane].hi && g_hi >= rec[kb + lane].lo);
      unsigned long long m = __ballot(hit);
      while (m) {
        const ScoreRec r = rec[kb + __builtin_ctzll(m)];
        m &= m - 1;
        if (e == GL) {
          acc = acc + r.v;
        } else if (live && g >= r.lo && g <= r.hi) {
          const int i1 = min(r.row + 1, n - 1);
          const double y0 = y[(size_t)r.row * GL + e], y1 = y[(size_t)i1 * GL + e];
          acc = acc + r.v * blend(y0, y1, r.f);
        }
      }
    }
  } else if (e == GL) {
    for (long k = k0; k < k1; ++k) acc = acc + rec[k].v;
  } else if (live) {
    for (long k = k0; k < k1; ++k) {
      const ScoreRec r = rec[k];
      if (g >= r.lo && g <= r.hi) {
        const int i1 = min(r.row + 1, n - 1);
        const double y0 = y[(size_t)r.row * GL + e], y1 = y[(size_t)i1 * GL + e];
        acc = acc + r.v * blend(y0, y1, r.f);
      }
    }
  }
  if (live) partial[(size_t)cl * (GL + 1) + e] = acc;
}

// tally[b][e] = tally[b][e] + the partials of bin b among the chunks c0 <= c < c1, ascending (element
// GL: wsum[b]); bins b0 <= b < b0 + nb, first[b] .. first[b + 1] the chunks of bin b
__global__ void __launch_bounds__(kThreads)
score_fold_kernel(long b0, long nb, int GL, long c0, long c1, const long* __restrict__ first,
                  const double* __restrict__ partial, double* __restrict__ tally, double* __restrict__ wsum) {
  const int GLp = GL + 1;
  const long total = nb * GLp, stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const long b = b0 + t / GLp;
    const int e = (int)(t % GLp);
    const long lo = first[b] > c0 ? first[b] : c0, hi = first[b + 1] < c1 ? first[b + 1] : c1;
    double* dst = e < GL ? tally + (size_t)b * GL + e : wsum + b;
    double acc = *dst;
    long c = lo;
    for (; c + 8 <= hi; c += 8) {                       // eight loads in flight, the additions in order
      double p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] = partial[(size_t)(c - c0 + j) * GLp + e];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = acc + p[j];
    }
    for (; c < hi; ++c) acc = acc + partial[(size_t)(c - c0) * GLp + e];
    *dst = acc;
  }
}

// what ndpp_scatt_score_info reports of the calling thread's last call
thread_local double g_info[NDPP_SCORE_INFO_LEN] = {0};

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// body(e0, e1) over [0, n) on a few host threads when there are enough events (nuclide.hip's
// parallel_rows for events: every event owns its outputs, so the result does not depend on the
// split).  A thread that cannot be started (the process is at its limit) costs nothing but time:
// its range runs on the calling thread, and every thread that did start is joined.
template <class F>
void parallel_events(long n, F body) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::min<unsigned>(nt ? nt : 1, 16);
  if (n < (1L << 16) || nt < 2) { body(0L, n); return; }
  std::vector<std::thread> th;
  th.reserve(nt);                                       // (before any thread runs: emplace_back below cannot allocate)
  const long per = (n + nt - 1) / nt;
  for (unsigned t = 1; t < nt; ++t) {
    const long e0 = std::min(n, (long)t * per), e1 = std::min(n, e0 + per);
    if (e0 >= e1) continue;
    try {
      th.emplace_back([=] { body(e0, e1); });
    } catch (const std::system_error&) {
      body(e0, e1);
    }
  }
  body(0L, std::min(n, per));
  for (auto& x : th) x.join();
}

long env_long(const char* name, long dflt, long lo, long hi) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const long x = std::strtol(v, &end, 10);
  if (end == v || *end) return dflt;
  return std::min(hi, std::max(lo, x));
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" int ndpp_scatt_score_info(double* out, int n) {
  if (!out || n < 0) return fail(NDPP_EINVAL, "scatt_score_info: NULL argument or n=%d", n);
  for (int k = 0; k < n; ++k) out[k] = k < NDPP_SCORE_INFO_LEN ? g_info[k] : 0.0;
  return NDPP_OK;
}

extern "C" int ndpp_scatt_score(int normalize, int scatt_type, int G, int L, int n, const double* x, const double* y,
                                long n_ev, const double* ein, const double* weight, const int* bin, int n_bins,
                                double* tally, double* wsum, long* count, int* status) {
  if (normalize != 0 && normalize != 1) return fail(NDPP_EINVAL, "scatt_score: normalize=%d (need 0 or 1)", normalize);
  if (normalize && scatt_type != NDPP_SCATT_LEGENDRE && scatt_type != NDPP_SCATT_TABULAR)
    return fail(NDPP_EINVAL, "scatt_score: scatt_type=%d (normalize = 1 needs 0, Legendre, or 1, tabular)", scatt_type);
  const int Lmax = (normalize && scatt_type == NDPP_SCATT_LEGENDRE) ? NDPP_MAX_ORDER : NDPP_MAX_TAB_BINS;
  if (G < 1 || L < 1 || L > Lmax)
    return fail(NDPP_EINVAL, "scatt_score: G=%d L=%d (need G >= 1 and 1 <= L <= %d)", G, L, Lmax);
  if (n < 2) return fail(NDPP_EINVAL, "scatt_score: n=%d (need n >= 2)", n);
  if (n_ev < 0) return fail(NDPP_EINVAL, "scatt_score: n_ev=%ld (need n_ev >= 0)", n_ev);
  if (n_bins < 1) return fail(NDPP_EINVAL, "scatt_score: n_bins=%d (need n_bins >= 1)", n_bins);
  if (!x || !y || !ein || !weight || !bin || !tally || !wsum || !count || !status)
    return fail(NDPP_EINVAL, "scatt_score: NULL argument");
  int rc = check_gl_index("scatt_score", G, L);
  if (rc != NDPP_OK) return rc;
  const int GL = G * L, GLp = GL + 1;
  size_t y_bytes, t_bytes, ev_bytes;
  if (!bytes_of((size_t)n * G, L, sizeof(double), &y_bytes) || !bytes_of(n_bins, GLp, sizeof(double), &t_bytes) ||
      !bytes_of((size_t)n_ev + n_bins + 1, 1, sizeof(ScoreRec), &ev_bytes))
    return fail(NDPP_EINVAL, "scatt_score: n=%d G=%d L=%d n_ev=%ld n_bins=%d: the sizes overflow", n, G, L, n_ev,
                n_bins);
  if ((rc = check_energy_grid("scatt_score", "x", n, x))) return rc;
  if ((rc = require_device("scatt_score"))) return rc;

  for (double& v : g_info) v = 0.0;
  std::fill(tally, tally + (size_t)n_bins * GL, 0.0);
  std::fill(wsum, wsum + n_bins, 0.0);
  std::fill(count, count + n_bins, 0L);
  if (n_ev == 0) return NDPP_OK;
  const long budget_mb = env_long("NDPP_SCORE_PARTIAL_MB", 256, 1, 1 << 16);      // read once per call
  const int use_band = env_long("NDPP_SCORE_BAND", 1, 0, 1) != 0;                // 0: measurements only

  // 1. row and weight of row i + 1 per event; row -1 marks the events that are skipped
  auto t0 = std::chrono::steady_clock::now();
  std::vector<int> row((size_t)n_ev);
  std::vector<double> wt((size_t)n_ev);
  parallel_events(n_ev, [&](long e0, long e1) {
    for (long e = e0; e < e1; ++e) {
      const double v = ein[e];
      const bool ok = std::isfinite(v) && v > 0.0 && v >= x[0] && v <= x[n - 1] && std::isfinite(weight[e]) &&
                      bin[e] >= 0 && bin[e] < n_bins;
      if (!ok) {
        row[e] = -1;
        wt[e] = 0.0;
        status[e] = NDPP_SCORE_SKIPPED;
        continue;
      }
      status[e] = NDPP_SCORE_OK;
      bracket(n, x, v, &row[e], &wt[e]);
    }
  });
  g_info[NDPP_SCORE_INFO_BRACKET_MS] = ms_since(t0);

  // the section, its masses and bands; with normalize = 1 the factors and the statuses they decide
  t0 = std::chrono::steady_clock::now();
  const long rows = (long)n * G;
  DevBuf<double> d_y, d_s, d_wt, d_weight, d_v;
  DevBuf<int> d_nz, d_blo, d_bhi, d_row, d_status;
  NDPP_TRY(d_y.upload(y, (size_t)rows * L));
  NDPP_TRY(d_row.upload(row.data(), row.size()));
  NDPP_TRY(d_wt.upload(wt.data(), wt.size()));
  NDPP_TRY(d_weight.upload(weight, (size_t)n_ev));
  NDPP_TRY(d_s.alloc((size_t)rows));
  NDPP_TRY(d_nz.alloc((size_t)rows));
  NDPP_TRY(d_blo.alloc((size_t)n));
  NDPP_TRY(d_bhi.alloc((size_t)n));
  g_info[NDPP_SCORE_INFO_UPLOAD_MS] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(score_rows_kernel, dim3(nblk(rows, kThreads)), dim3(kThreads), 0, 0, rows, L,
                     (int)(normalize && scatt_type == NDPP_SCATT_TABULAR), d_y.p, d_s.p, d_nz.p);
  NDPP_TRY(hipGetLastError());
  hipLaunchKernelGGL(score_band_kernel, dim3(nblk(n, kThreads)), dim3(kThreads), 0, 0, n, G, d_nz.p, d_blo.p, d_bhi.p);
  NDPP_TRY(hipGetLastError());
  if (normalize) {
    NDPP_TRY(d_v.alloc((size_t)n_ev));
    NDPP_TRY(d_status.alloc((size_t)n_ev));
    hipLaunchKernelGGL(score_factor_kernel, dim3(nblk(n_ev, kThreads)), dim3(kThreads), 0, 0, n_ev, G, n, use_band,
                       d_s.p, d_row.p, d_wt.p, d_weight.p, d_blo.p, d_bhi.p, d_v.p, d_status.p);
    NDPP_TRY(hipGetLastError());
    NDPP_TRY(hipDeviceSynchronize());
    NDPP_TRY(d_status.download(status, (size_t)n_ev));
  }
  g_info[NDPP_SCORE_INFO_FACTOR_MS] = ms_since(t0);

  // 2. the scored events by bin, each bin in ascending event index (a stable counting sort), and
  // the chunk table: first[b] .. first[b + 1] the chunks of bin b, cstart[c] .. cstart[c + 1] chunk c's
  // places in the sorted order
  t0 = std::chrono::steady_clock::now();
  std::vector<long> off((size_t)n_bins + 1, 0), first((size_t)n_bins + 1, 0);
  for (long e = 0; e < n_ev; ++e)
    if (status[e] == NDPP_SCORE_OK) ++off[(size_t)bin[e] + 1];
  for (int b = 0; b < n_bins; ++b) {
    count[b] = off[(size_t)b + 1];
    first[(size_t)b + 1] = first[b] + (off[(size_t)b + 1] + kChunk - 1) / kChunk;
    off[(size_t)b + 1] += off[b];
  }
  const long n_sc = off[n_bins], n_chunks = first[n_bins];
  std::vector<long> perm((size_t)n_sc), cstart((size_t)n_chunks + 1, 0);
  {
    std::vector<long> at(off.begin(), off.end() - 1);
    for (long e = 0; e < n_ev; ++e)
      if (status[e] == NDPP_SCORE_OK) perm[(size_t)at[bin[e]]++] = e;
  }
  for (int b = 0; b < n_bins; ++b)
    for (long c = first[b]; c < first[(size_t)b + 1]; ++c) cstart[c] = off[b] + (c - first[b]) * kChunk;
  cstart[n_chunks] = n_sc;
  // (chunk c ends where chunk c + 1 starts: the bins are contiguous in the sorted order)
  g_info[NDPP_SCORE_INFO_GROUP_MS] = ms_since(t0);
  g_info[NDPP_SCORE_INFO_SCORED] = (double)n_sc;
  g_info[NDPP_SCORE_INFO_CHUNKS] = (double)n_chunks;
  if (n_sc == 0) {                       // nothing to sum; the row and band kernels are still queued on these buffers
    NDPP_TRY(hipDeviceSynchronize());
    return NDPP_OK;
  }

  // the shape of the chunk kernel and the chunks of a pass
  int W = 64;
  if (GLp <= 32) {
    W = 1;
    while (W < GLp) W *= 2;
  }
  const int tiles = (GLp + W - 1) / W, upb = kThreads / W;
  long per_pass = std::max<long>(1, (budget_mb << 20) / ((long)GLp * (long)sizeof(double)));
  per_pass = std::min(per_pass, (long)(INT_MAX / 2) * upb / tiles);       // the grid fits an int
  per_pass = std::max<long>(1, std::min(per_pass, n_chunks));

  t0 = std::chrono::steady_clock::now();
  DevBuf<long> d_perm, d_cstart, d_first;
  DevBuf<ScoreRec> d_rec;
  DevBuf<double> d_partial, d_tally, d_wsum;
  NDPP_TRY(d_perm.upload(perm.data(), perm.size()));
  NDPP_TRY(d_cstart.upload(cstart.data(), cstart.size()));
  NDPP_TRY(d_first.upload(first.data(), first.size()));
  NDPP_TRY(d_rec.alloc((size_t)n_sc));
  NDPP_TRY(d_partial.alloc((size_t)per_pass * GLp));
  NDPP_TRY(d_tally.alloc((size_t)n_bins * GL));
  NDPP_TRY(d_wsum.alloc((size_t)n_bins));
  NDPP_TRY(hipMemset(d_tally.p, 0, (size_t)n_bins * GL * sizeof(double)));
  NDPP_TRY(hipMemset(d_wsum.p, 0, (size_t)n_bins * sizeof(double)));
  g_info[NDPP_SCORE_INFO_UPLOAD_MS] += ms_since(t0);
  int passes = 0;
  {
    GpuSpan span(nullptr, -1);
    hipLaunchKernelGGL(score_gather_kernel, dim3(nblk(n_sc, kThreads)), dim3(kThreads), 0, 0, n_sc, G, n, use_band,
                       d_perm.p, d_row.p, d_wt.p, normalize ? d_v.p : d_weight.p, d_blo.p, d_bhi.p, d_rec.p);
    NDPP_TRY(hipGetLastError());
    long b0 = 0;
    for (long c0 = 0; c0 < n_chunks; c0 += per_pass, ++passes) {
      const long nc = std::min(per_pass, n_chunks - c0), c1 = c0 + nc;
      const long units = nc * tiles;
      hipLaunchKernelGGL(score_chunk_kernel, dim3((unsigned)((units + upb - 1) / upb)), dim3(kThreads), 0, 0, c0, nc, G,
                         L, n, W, tiles, d_y.p, d_rec.p, d_cstart.p, d_partial.p);
      NDPP_TRY(hipGetLastError());
      // the bins with a chunk in [c0, c1): from the first that ends after c0 to the last that starts before c1
      while (b0 < n_bins && first[(size_t)b0 + 1] <= c0) ++b0;
      long b1 = b0;
      while (b1 < n_bins && first[b1] < c1) ++b1;
      hipLaunchKernelGGL(score_fold_kernel, dim3(nblk((b1 - b0) * GLp, kThreads)), dim3(kThreads), 0, 0, b0, b1 - b0,
                         GL, c0, c1, d_first.p, d_partial.p, d_tally.p, d_wsum.p);
      NDPP_TRY(hipGetLastError());
    }
    NDPP_CLOSE_SPAN(span);
  }
  g_info[NDPP_SCORE_INFO_PASSES] = (double)passes;
  t0 = std::chrono::steady_clock::now();
  NDPP_TRY(d_tally.download(tally, (size_t)n_bins * GL));
  NDPP_TRY(d_wsum.download(wsum, (size_t)n_bins));
  g_info[NDPP_SCORE_INFO_DOWNLOAD_MS] = ms_since(t0);
  g_info[NDPP_SCORE_INFO_KERNEL_MS] = (double)ndpp_last_gpu_ms();
  return NDPP_OK;
}
