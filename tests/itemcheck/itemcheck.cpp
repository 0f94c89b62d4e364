// tests/itemcheck/itemcheck.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The set-up of the free-gas inner walk (ndpp_amd/csrc/fg_pipeline.h) against a restatement of the
// set-up it replaced, on the CPU:
//   1. split_segment / split_own_from, the closed forms for "the rank-th depth-4 node counted from the
//      peak's outwards" and "the depth from which accepted leaves are the item's own", against the two
//      loops that used to find them, for all 16 x 16 (jp, rank); for every jp the 16 ranks are a
//      permutation of the 16 nodes.
//   2. fg_item_build + mu_init / mu_init_split, which go through the item record, against
//      old_mu_init / old_mu_init_split below, which gather from the task order, the node, the job and
//      the task records as the walk itself used to: every field of the lane state, to the bit, for
//      every task of level 0 of two jobs (reversed task order), among them nodes with mask 0, level-0
//      aliases, and tasks with one row taken by the Gauss stage.  The same for the forms of mu_init /
//      mu_init_split that build the one record where they stand (tests/hostsim calls those).
// Built in either arithmetic (-DNDPP_FAST=1 / 0).  Prints a summary and exits 0, or a complaint and 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ndpp_amd/csrc/fg_pipeline.h"

using namespace ndpp;

// ---- the restatement: the loops of the previous mu_init_split ------------------------------------
static void old_segment(int jp, int rank, int& seg, int& own_from) {
  int lo = jp - 1, hi = jp, cur = hi;
  for (int k = 0; k <= rank; ++k) {
    if (((k & 1) == 0 && hi < kSplit) || lo < 0) cur = hi++;
    else cur = lo--;
  }
  int tz = 0;
  while (tz < kSplitLog2 && !(((unsigned)cur >> tz) & 1u)) ++tz;
  seg = cur;
  own_from = kSplitLog2 - tz;
}

// ---- the restatement: the previous mu_init and mu_init_split -------------------------------------
template <int R, int LMAX>
static void old_mu_init(const FgBatch& B, int level, int base, int t, MuLane<R, LMAX>& s) {
  int n, slot;
  fg_task_decode(B, level, base, t, n, slot);
  s.node = n;
  s.slot = slot;
  s.mask = (unsigned)B.node_info[4 * n + 0] & MuLane<R, LMAX>::kChanMask;
  s.pending = 0; s.depth = 0; s.visits = 0; s.ovisits = 0;
  for (int ch = 0; ch < R * LMAX; ++ch) s.acc[ch] = 0.0;
  s.path_left = 0; s.own_from = 0; s.path_bits = 0; s.own_pending = false; s.slot_path = 0;
  s.task = t;
  s.chans = s.mask;
  if (s.mask == 0) return;
  const int rec = B.rec_index(level, base, n, slot);
  if (B.t_gl) {
    const unsigned rows = B.t_gl[rec];
    for (int r = 0; r < R; ++r)
      if (rows >> r & 1u) s.mask &= ~(((1u << kRowBits) - 1u) << (r * kRowBits));
    s.chans = s.mask;
    if (s.mask == 0) return;
  }
  const int job = B.node_job(n);
  const double Ein = B.job_ein[job];
  const double Eout = fg_slot_point(B.node_a[n], B.node_b[n], slot);
  s.q = make_pair(B.A_of(job), B.kT_of(job), Ein, Eout);
  s.f.off = 8u * (unsigned)B.M * (unsigned)B.job_row[(size_t)job * R];
  s.a = B.t_mulo[rec];
  s.b = B.t_muhi[rec];
  double Xa[R];
  for (int r = 0; r < R; ++r) {
    Xa[r] = B.tX(0, r, rec);
    s.Xb[r] = B.tX(1, r, rec);
    s.Xc[r] = B.tX(2, r, rec);
  }
  const double h = s.b - s.a;
  s.wp = h / 6.0;
  double Pa[LMAX];
  pn_all<LMAX>(s.a, Pa, make_pn_consts());
  for (int r = 0; r < R; ++r)
    for (int l = 0; l < LMAX; ++l) s.fa[r * LMAX + l] = Xa[r] * Pa[l];
}

template <int R, int LMAX>
static void old_mu_init_split(const FgBatch& B, int level, int base, int t, MuLane<R, LMAX>& s) {
  const int nt = B.n_mu_tasks(level);
  const int i = t % nt, rank = t / nt;
  old_mu_init<R, LMAX>(B, level, base, i, s);
  int jp = 0;
  if (s.mask != 0) {
#if NDPP_FAST
    const double pa = s.q.p, qa = s.q.q;
#else
    const double pa = s.q.EpE / s.q.AkT, qa = 2.0 * s.q.s2 / s.q.AkT;
#endif
    const double x = ((pa - fabs(s.q.beta)) / qa - s.a) / (s.b - s.a) * (double)kSplit;
    jp = (x > 0.0) ? (x < (double)(kSplit - 1) ? (int)x : kSplit - 1) : 0;
  }
  int seg, own;
  old_segment(jp, rank, seg, own);
  s.path_left = kSplitLog2;
  s.path_bits = (unsigned)seg;
  s.slot_path = 0;
  s.own_from = own;
  s.own_pending = (own != 0);
}

static bool same(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }

// every field of the lane state the walk goes on to read (`full`: those past the mask-0 early return too)
template <int R, int LMAX>
static const char* lane_diff(const MuLane<R, LMAX>& x, const MuLane<R, LMAX>& y) {
  if (x.mask != y.mask) return "mask";
  if (x.chans != y.chans) return "chans";
  if (x.node != y.node) return "node";
  if (x.slot != y.slot) return "slot";
  if (x.task != y.task) return "task";
  if (x.pending != y.pending || x.depth != y.depth || x.visits != y.visits || x.ovisits != y.ovisits) return "counters";
  if (!same(x.acc, y.acc, sizeof x.acc)) return "acc";
  if (x.path_left != y.path_left) return "path_left";
  if (x.path_bits != y.path_bits) return "path_bits";
  if (x.own_from != y.own_from || x.own_pending != y.own_pending) return "own_from";
  if (x.slot_path != y.slot_path) return "slot_path";
  if (x.mask == 0) return nullptr;
  // (of the pair, what this arithmetic's walk reads: item_pair_store)
#if NDPP_FAST
  if (!same(&x.q.C1, &y.q.C1, 8) || !same(&x.q.p, &y.q.p, 8) || !same(&x.q.q, &y.q.q, 8) || !same(&x.q.beta, &y.q.beta, 8)) return "q";
#else
  if (!same(&x.q, &y.q, sizeof x.q)) return "q";
#endif
  if (x.f.off != y.f.off) return "f.off";
  if (!same(&x.a, &y.a, 8) || !same(&x.b, &y.b, 8) || !same(&x.wp, &y.wp, 8)) return "a, b, wp";
  if (!same(x.Xb, y.Xb, sizeof x.Xb) || !same(x.Xc, y.Xc, sizeof x.Xc)) return "Xb, Xc";
  if (!same(x.fa, y.fa, sizeof x.fa)) return "fa";
  return nullptr;
}

int main() {
  // ---- 1. the segment order -------------------------------------------------------------------------
  for (int jp = 0; jp < kSplit; ++jp) {
    unsigned seen = 0;
    for (int rank = 0; rank < kSplit; ++rank) {
      int seg, own;
      old_segment(jp, rank, seg, own);
      const int got = split_segment(jp, rank);
      if (got != seg || got < 0 || got >= kSplit) { printf("FAIL: segment(jp %d, rank %d) = %d, the loop gives %d\n", jp, rank, got, seg); return 1; }
      if (split_own_from(got) != own) { printf("FAIL: own_from(segment %d) = %d, the loop gives %d\n", got, split_own_from(got), own); return 1; }
      seen |= 1u << got;
    }
    if (seen != (1u << kSplit) - 1u) { printf("FAIL: the ranks of jp %d are no permutation (%#x)\n", jp, seen); return 1; }
  }

  // ---- 2. the item records -------------------------------------------------------------------------
  constexpr int R = 2, LMAX = 6, M = 2001, G = 2;
  std::vector<double> f_tab((size_t)3 * M);
  for (int k = 0; k < M; ++k) {
    const double mu = -1.0 + 2.0 * k / (M - 1);
    f_tab[k] = 0.5; f_tab[M + k] = 0.5 * (1.0 + 0.1 * mu); f_tab[2 * M + k] = 0.5 * (1.0 + 0.3 * mu);
  }
  // (the second energy lies above the lower group: that group's [.., E_in] segment is dead there)
  const double ein[2] = {2.53e-8, 5e-6}, bins[G + 1] = {0.0, 6.25e-7, 20.0};
  const int row[2 * R] = {0, 1, 1, 2};
  FgBatch B{};
  B.n_jobs = 2; B.R = R; B.G = G; B.L = LMAX; B.M = M;
  B.A = 0.999167; B.kT = 2.5301e-8;
  B.job_ein = ein; B.job_row = row; B.f_tab = f_tab.data(); B.e_bins = bins;
  B.sab_threshold = 1e300; B.brent_thresh = 1e-6;    // (only the limits depend on these, and both set-ups read the same)
  B.mu_tol = 1e-7; B.eout_tol = 1e-7; B.mu_its = 15; B.eout_its = 15;
  B.grid = make_mu_grid(M);
  const int nn = B.n_trees();
  B.ncap = nn;
  std::vector<double> na(nn), nb(nn), nS((size_t)B.nch() * nn);
  std::vector<int> info((size_t)4 * nn), alias((size_t)5 * nn, -1), order(nn), cnt(kMaxLevels + 2, 0);
  B.node_a = na.data(); B.node_b = nb.data(); B.node_S = nS.data(); B.node_info = info.data();
  B.tcap = 5 * nn;
  B.icap = B.tcap;
  std::vector<double> t1(B.tcap), t2(B.tcap), t3((size_t)3 * R * B.tcap), itd((size_t)kItemDoubles * B.icap, -7.0);
  std::vector<int> iti((size_t)kItemInts * B.icap, -7);
  std::vector<unsigned char> tgl(B.tcap, 0);
  B.t_mulo = t1.data(); B.t_muhi = t2.data(); B.t_X = t3.data(); B.t_gl = tgl.data(); B.t_alias = alias.data();
  B.it_d = itd.data(); B.it_i = iti.data();
  cnt[0] = nn;
  B.lvl_cnt = cnt.data();
  for (int j = 0; j < B.n_jobs; ++j)
    for (int g = 0; g < G; ++g) fg_setup_group(B, j, g);
  const int nt = B.n_tasks(0);
  for (int t = 0; t < nt; ++t) fg_prep_task(B, 0, 0, t);
  // the Gauss-rule byte as the Gauss stage leaves it: the rows it has done.  Aliases keep theirs (all rows);
  // of the others every seventh live task gets row 0 taken and every eleventh row 1.
  int n_alias = 0, n_row = 0, n_dead = 0, live_k = 0;
  for (int t = 0; t < nt; ++t) {
    if (info[4 * (t / 5)] == 0) { n_dead += 1; continue; }
    if (tgl[t] & kGaussAlias) { n_alias += 1; continue; }
    tgl[t] = 0;
    live_k += 1;
    if (live_k % 7 == 0) { tgl[t] = 1; n_row += 1; }
    else if (live_k % 11 == 0) { tgl[t] = 2; n_row += 1; }
  }
  if (!n_alias || !n_row || !n_dead) { printf("FAIL: the case lost its coverage (%d aliases, %d Gauss-taken rows, %d dead tasks)\n", n_alias, n_row, n_dead); return 1; }
  for (int k = 0; k < nn; ++k) order[k] = nn - 1 - k;
  long checked = 0;
  for (int pass = 0; pass < 2; ++pass) {       // node order, then a task order
    B.order = pass ? order.data() : nullptr;
    for (int i = 0; i < nt; ++i) fg_item_build<R>(B, 0, 0, i, i);
    for (int i = 0; i < nt; ++i) {
      MuLane<R, LMAX> s_new, s_old;
      memset(&s_new, 0, sizeof s_new); memset(&s_old, 0, sizeof s_old);
      mu_init<R, LMAX>(B, i, s_new);
      old_mu_init<R, LMAX>(B, 0, 0, i, s_old);
      if (const char* d = lane_diff(s_new, s_old)) { printf("FAIL: pass %d task %d: %s differs\n", pass, i, d); return 1; }
      // (the forms that build the one record where they stand, as the host simulator calls them)
      memset(&s_new, 0, sizeof s_new);
      mu_init<R, LMAX>(B, 0, 0, i, s_new);
      if (const char* d = lane_diff(s_new, s_old)) { printf("FAIL: pass %d task %d, stand-alone: %s differs\n", pass, i, d); return 1; }
      for (int rank = 0; rank < kSplit; ++rank) {
        memset(&s_new, 0, sizeof s_new); memset(&s_old, 0, sizeof s_old);
        mu_init_split<R, LMAX>(B, i, rank, s_new);
        old_mu_init_split<R, LMAX>(B, 0, 0, rank * nt + i, s_old);
        if (const char* d = lane_diff(s_new, s_old)) { printf("FAIL: pass %d task %d item %d: %s differs\n", pass, i, rank, d); return 1; }
        memset(&s_new, 0, sizeof s_new);
        mu_init_split<R, LMAX>(B, 0, 0, rank * nt + i, s_new);
        if (const char* d = lane_diff(s_new, s_old)) { printf("FAIL: pass %d task %d item %d, stand-alone: %s differs\n", pass, i, rank, d); return 1; }
        checked += 1;
      }
    }
  }
  printf("segments ok; items %ld aliases %d gauss_rows %d dead %d\n", checked, n_alias, n_row, n_dead);
  return 0;
}
