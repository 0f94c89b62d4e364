// nuclide.hip -- host-only orchestration of one nuclide: calc_scatt (scatt.F90:33-157)
// behind the C ABI, for hosts that are not the reference's Fortran.  scatt_nuclide_impl is the
// sequence of its steps:
//
//   read_hooks              the NDPP_HIP_* hooks of this file and ndpp_get_nbody, once per call
//   convert_reactions       ScattData%init + convert_distro -> ndpp_scattdata_shape / ndpp_convert_distro
//   cutoff_and_threshold    scatt.F90:103-123
//   make_grids              create_Ein_grid -> ndpp_create_ein_grid (or the caller's lists); the result
//   run_grid, per grid      calc_elastic_grid (:603-675) / calc_inelastic_grid (:682-778):
//     select_energies, select_yields   the bookkeeping of one reaction
//     integrate_reaction               integrate_distro's dispatch over the batch calls (+ law 66, opt-in)
//     ElasticAssign / HostSum / DeviceSum   take() a reaction's moments, finish() the grid
//     copy_top_rows
// "Bookkeeping" is scatt_interp_distro (scattdata_header.F90:391-499): threshold and
// top-of-grid tests, the cross-section interpolation, the row search with the
// duplicate-row skip, p_valid, and after the batch call the sigma * p_valid scaling,
// the reaction sum and the nu-scatter yield (scatt.F90:745-762) in the reference's
// order of operations.  ElasticDefer (append_reaction, run_elastic_defer) collects angular-only
// reactions for one ndpp_elastic_leg_multi call: a library's elastic grids, a host-summed grid's
// levels.  fortran/ndpp_hip_mod.f90 holds the same logic for the Fortran host; both are checked
// against the reference's calc_scatt.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <memory>
#include <vector>

#include "../../include/ndpp_hip.h"
#include "dev_util.h"
#include "kernels.h"

namespace ndpp {
namespace {

// The NDPP_HIP_* hooks of the whole-nuclide driver, each with its default and meaning (INTEGRATION.md
// section 6); read once per scatt_nuclide_impl call, here and nowhere else.
struct Hooks {
  bool device_tables = true;              // NDPP_HIP_NO_DEVICE_TABLES=1 (test): every table through the host
  bool level_batch = true;                // NDPP_HIP_NO_LEVEL_BATCH=1 (test): one batch call per level
  size_t dev_sum_min = (size_t)1 << 20;   // NDPP_HIP_DEV_SUM_MIN=n (test): see run_grid
  bool host_timing = false;               // NDPP_HIP_HOST_TIMING=1: HostClock's line on stderr
};
Hooks read_hooks() {
  const auto is_one = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
  Hooks h;
  h.device_tables = !is_one("NDPP_HIP_NO_DEVICE_TABLES");
  h.level_batch = !is_one("NDPP_HIP_NO_LEVEL_BATCH");
  if (const char* e = getenv("NDPP_HIP_DEV_SUM_MIN")) h.dev_sum_min = (size_t)atoll(e);
  h.host_timing = is_one("NDPP_HIP_HOST_TIMING");
  return h;
}

// Hooks::host_timing: where the host side of one nuclide spends its time (stderr)
struct HostClock {
  using clk = std::chrono::steady_clock;
  bool print;
  clk::time_point t0 = clk::now();
  double acc[6] = {0, 0, 0, 0, 0, 0};   // convert, grids + matrices, bookkeeping, batch calls, reaction sum, top rows
  explicit HostClock(bool on) : print(on) {}
  void lap(int k) {
    const clk::time_point t = clk::now();
    acc[k] += std::chrono::duration<double, std::milli>(t - t0).count();
    t0 = t;
  }
  ~HostClock() {
    if (print)
      fprintf(stderr, "ndpp_scatt_nuclide host ms: convert %.1f  grids+matrices %.1f  bookkeeping %.1f  "
                      "batch calls %.1f  reaction sum / download %.1f  top rows %.1f\n",
              acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]);
  }
};

// The (L, G) blocks a batch call returns for one reaction: page-locked when the driver grants
// it (the device-to-host copy of a many-group reaction -- 54 MB at G = 70 -- then runs at the
// link's rate instead of through the runtime's bounce buffers), ordinary memory otherwise.
// Not zero-filled: every batch call writes all of what it is given.
struct ResultStage {
  double* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  double* get(size_t n) {
    if (n <= cap) return p;
    release();
    if (n * sizeof(double) >= ((size_t)1 << 20) &&
        hipHostMalloc((void**)&p, n * sizeof(double), hipHostMallocDefault) == hipSuccess) {
      pinned = true;
    } else {
      (void)hipGetLastError();
      p = static_cast<double*>(malloc(n * sizeof(double)));
      pinned = false;
    }
    cap = p ? n : 0;
    return p;
  }
  void release() {
    if (p) { if (pinned) (void)hipHostFree(p); else free(p); }
    p = nullptr;
    cap = 0;
  }
  ~ResultStage() { release(); }
};

// calc_inelastic_grid's reaction sum kept on the device: the matrices of the inelastic grid live
// in HBM while the reactions are integrated, every batch call hands its moments over on the
// device (kernels.h DeviceSink) and one kernel scales and adds them; one copy to the host at the
// end.  (At G = 70 a U-238-like nuclide has 44 reactions x 54 MB: the host-side sum and the
// copies were 0.7 s of its 12 s.)
struct ReactionSum : DeviceSink {
  DevBuf<double> mat, numat;
  DevBuf<char> args;            // one upload per reaction: scale[cap], pv[cap], yield[cap], where[cap]
  std::vector<char> args_h;
  int cap = 0, nb = 0;
  size_t GL = 0, rows = 0;
  bool with_nu = false;
  const double* scale_d() const { return reinterpret_cast<const double*>(args.p); }
  const double* pv_d() const { return scale_d() + cap; }
  const double* yield_d() const { return scale_d() + 2 * (size_t)cap; }
  const int* where_d() const { return reinterpret_cast<const int*>(scale_d() + 3 * (size_t)cap); }
  int init(size_t n_rows, size_t gl, bool nu, int max_nb) {
    rows = n_rows; GL = gl; with_nu = nu; cap = max_nb;
    args_h.resize((size_t)cap * (3 * sizeof(double) + sizeof(int)));
    if (mat.alloc(rows * GL) != hipSuccess || (nu && numat.alloc(rows * GL) != hipSuccess) ||
        args.alloc(args_h.size()) != hipSuccess)
      return fail(NDPP_ENOMEM, "out of device memory for the inelastic matrices");
    if (hipMemset(mat.p, 0, rows * GL * sizeof(double)) != hipSuccess ||
        (nu && hipMemset(numat.p, 0, rows * GL * sizeof(double)) != hipSuccess))
      return fail(NDPP_EDEVICE, "hipMemset failed");
    return NDPP_OK;
  }
  // the rows, cross sections, p_valid and yields of the next batch call
  int stage(int n, const int* w, const double* s, const double* v, const double* y) {
    nb = n;
    double* d = reinterpret_cast<double*>(args_h.data());
    std::copy(s, s + n, d);
    std::copy(v, v + n, d + cap);
    std::copy(y, y + n, d + 2 * (size_t)cap);
    std::copy(w, w + n, reinterpret_cast<int*>(d + 3 * (size_t)cap));
    if (hipMemcpy(args.p, args_h.data(), args_h.size(), hipMemcpyHostToDevice) != hipSuccess)
      return fail(NDPP_EDEVICE, "upload of a reaction's scaling failed");
    return NDPP_OK;
  }
  int consume(const double* out_d, int n, size_t gl) override {
    if (n != nb || gl != GL) return fail(NDPP_EINVAL, "reaction sum: batch of %d x %zu, staged %d x %zu", n, gl, nb, GL);
    launch_reaction_sum(n, GL, out_d, where_d(), scale_d(), pv_d(), yield_d(), mat.p, with_nu ? numat.p : nullptr);
    return hipGetLastError() == hipSuccess ? NDPP_OK : fail(NDPP_EDEVICE, "reaction sum kernel failed to launch");
  }
  int download(double* m, double* nm) {
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(m, mat.p, rows * GL * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        (with_nu && nm && hipMemcpy(nm, numat.p, rows * GL * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
      return fail(NDPP_EDEVICE, "download of the inelastic matrices failed");
    return NDPP_OK;
  }
};

// body(k0, k1) over [0, n) on a few host threads when the range carries enough work (the
// reaction sum of a many-group structure moves ~250 MB per reaction; the items are independent:
// every incoming energy of a reaction owns its row of the matrices)
template <class F>
void parallel_rows(int n, size_t work_per_row, F body) {
  const size_t work = (size_t)n * work_per_row;
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::min<unsigned>(nt ? nt : 1, 16);
  if (work < ((size_t)1 << 21) || nt < 2 || n < 2 * (int)nt) { body(0, n); return; }
  std::vector<std::thread> th;
  const int per = (n + (int)nt - 1) / (int)nt;
  for (unsigned t = 1; t < nt; ++t) {
    const int k0 = std::min(n, (int)t * per), k1 = std::min(n, k0 + per);
    if (k0 < k1) th.emplace_back([=] { body(k0, k1); });
  }
  body(0, std::min(n, per));
  for (auto& x : th) x.join();
}

// interpolate_tab1_object, interpolation.F90:132-206; rc != 0 where it aborts
int tab1(int n_regions, const int* nbt, const int* intc, int n_pairs, const double* x,
         const double* y, double xv, double* out) {
  if (n_pairs < 1 || !x || !y) return fail(NDPP_EINVAL, "empty TAB1 function");
  if (xv < x[0]) { *out = y[0]; return NDPP_OK; }
  if (xv > x[n_pairs - 1]) { *out = y[n_pairs - 1]; return NDPP_OK; }
  if (n_pairs == 1) { *out = y[0]; return NDPP_OK; }
  const int i = bsearch1_clamped(x, n_pairs, xv);
  int interp = 2;
  if (n_regions == 1) interp = intc[0];
  else if (n_regions > 1)
    for (int j = 0; j < n_regions; ++j)
      if (i < nbt[j]) { interp = intc[j]; break; }
  if (interp == 1) { *out = y[i - 1]; return NDPP_OK; }
  const double x0 = x[i - 1], x1 = x[i], y0 = y[i - 1], y1 = y[i];
  double r;
  switch (interp) {
    case 2: r = (xv - x0) / (x1 - x0); *out = (1 - r) * y0 + r * y1; break;
    case 3: r = (std::log(xv) - std::log(x0)) / (std::log(x1) - std::log(x0));
            *out = (1 - r) * y0 + r * y1; break;
    case 4: r = (xv - x0) / (x1 - x0);
            *out = std::exp((1 - r) * std::log(y0) + r * std::log(y1)); break;
    case 5: r = (std::log(xv) - std::log(x0)) / (std::log(x1) - std::log(x0));
            *out = std::exp((1 - r) * std::log(y0) + r * std::log(y1)); break;
    default: return fail(NDPP_EINVAL, "Unsupported interpolation scheme: %d", interp);
  }
  return NDPP_OK;
}

// one ScattData after init + convert_distro
struct SD {
  bool is_init = false;
  int law = 0;
  bool has_adist = false, has_edist = false;   // associated(this%adist / this%edist)
  const ndpp_ace_rxn* rxn = nullptr;
  const ndpp_ace_edist* edist = nullptr;
  bool in_cm = false;
  int NE = 0;
  std::vector<double> e_grid, eout, pdf, cdf, f;
  std::vector<int> row_ptr, intt;
  // a table only the file-6 integrators read stays on the device, where convert_kernel wrote it and
  // they read it (f is then empty): a continuum's M x sum NP doubles -- 10 to 200 MB for a U-238-class
  // nuclide -- cross to the host and back otherwise
  std::shared_ptr<double> f_dev;
};

// Elastic batches of several nuclides, collected instead of run, so that a library is
// integrated by ONE ndpp_elastic_leg_multi call (small per-nuclide batches leave the GPU
// mostly idle).
struct ElasticDefer {
  std::vector<double> A, kT, cut, Q;        // per collected batch ("nuclide" of the multi call)
  std::vector<double> ein, w, f_tab;
  std::vector<int> nuc, row;
  std::vector<double*> dst;                 // where each incoming energy's (L,G) block goes
  struct Top { double* mat; const double* Ein; int n; };
  std::vector<Top> tops;                    // elastic matrices whose top point is copied last
  int n_rows = 0;
};

// Where the two incoming grids of a nuclide come from: create_Ein_grid (no GivenGrids), or the
// caller's own lists (ndpp_scatt_library_at).  Everything after the grids is the same code.
struct GivenGrids {
  int n_el, n_inel;
  const double *ein_el, *ein_inel;
};

// the parts of a Reaction that ScattData%init may rewrite (:160-223)
struct RxnState {
  bool has_angle_dist;
  bool in_cm;
  bool fabricated = false;
  double fab_energy[2];
};

// what the steps of one scatt_nuclide_impl call share
struct Call {
  const ndpp_params* p;
  const ndpp_ace_nuclide* nuc;
  int n_bins;
  const double* e_bins;
  int n_tab, G, L, M;     // n_tab = 0: L = p->order Legendre moments; n_tab > 0: L = n_tab bins
  bool nbody;             // ndpp_set_nbody, read once per call: law 66 is integrated
  bool nbody_tab;         // ndpp_set_nbody_tab, read with it: law 66 also in a tabular call (acts only with nbody)
  size_t GL;
  double Etop;
  Hooks hooks;
  HostClock hc;
  Call(const ndpp_params* p_, const ndpp_ace_nuclide* nuc_, int n_bins_, const double* e_bins_, int n_tab_)
      : p(p_), nuc(nuc_), n_bins(n_bins_), e_bins(e_bins_), n_tab(n_tab_), G(n_bins_ - 1),
        L(n_tab_ > 0 ? n_tab_ : p_->order), M(p_->mu_bins), GL((size_t)G * L), Etop(e_bins_[G]),
        nbody(ndpp_get_nbody() != 0), nbody_tab(ndpp_get_nbody_tab() != 0), hooks(read_hooks()),
        hc(hooks.host_timing) {}
};

// ---- init + convert_distro for every reaction and nested distribution (:59-106)

// the Reaction as the next ScattData%init sees it: rx, with what an earlier init rewrote on it
ndpp_ace_reaction reaction_view(const ndpp_ace_nuclide* nuc, const ndpp_ace_rxn& rx, const ndpp_ace_edist* ed,
                                const RxnState& st) {
  const static int kIso[2] = {1, 1}, kZero[2] = {0, 0};
  const static double kZeroD[2] = {0.0, 0.0};
  ndpp_ace_reaction a;
  memset(&a, 0, sizeof(a));
  a.MT = rx.MT;
  a.law = ed ? ed->law : 0;
  a.threshold_energy = nuc->energy[rx.threshold - 1];
  if (st.has_angle_dist) {
    a.has_angle_dist = 1;
    if (st.fabricated) {   // the isotropic adist an earlier init wrote into rxn%adist
      a.n_adist = 2; a.adist_energy = st.fab_energy; a.adist_type = kIso;
      a.adist_location = kZero; a.n_adist_data = 2; a.adist_data = kZeroD;
    } else {
      a.n_adist = rx.n_adist; a.adist_energy = rx.adist_energy; a.adist_type = rx.adist_type;
      a.adist_location = rx.adist_location; a.n_adist_data = rx.n_adist_data;
      a.adist_data = rx.adist_data;
    }
  }
  if (ed) { a.n_edata = ed->n_data; a.edata = ed->data; }
  return a;
}

// what init leaves behind (:135-223): on the ScattData, and on the reaction for the inits after it
void after_init(const Call& c, const ndpp_ace_edist* ed, double threshold_energy, SD* sd, RxnState* st) {
  const bool had_adist = st->has_angle_dist;
  if (had_adist) {
    sd->has_adist = true;
    sd->has_edist = ed && ed->law != 3;
  } else if (ed) {
    if (ed->law == 4 || ed->law == 3 || ed->law == 9) {
      sd->has_adist = true;
      sd->has_edist = (ed->law == 9 || ed->law == 4);
    } else {
      sd->has_edist = true;
    }
  } else {
    sd->has_adist = true;
    st->in_cm = true;   // :218
  }
  if (!had_adist && sd->has_adist) {      // rxn%adist now holds the isotropic table
    st->has_angle_dist = true;
    st->fabricated = true;
    st->fab_energy[1] = c.Etop;
    st->fab_energy[0] = (threshold_energy > c.e_bins[0]) ? threshold_energy : c.e_bins[0];
  }
  sd->edist = sd->has_edist ? ed : nullptr;
}

// integrate_distro's dispatch (:533-656): 1 angular only, 2 file 6 in the CM, 3 law 9, 4 file 6 in the lab;
// 5, not the reference's: law 66 in closed form (init_nbody)
int distro_kind(const SD& sd) {
  if (sd.law == 66) return 5;
  if (sd.has_adist && !sd.has_edist) return 1;
  if (sd.in_cm) return 2;
  if (sd.has_adist && sd.law == 9) return 3;
  return 4;
}

// convert_distro: the table on the host, or kept on the device for the file-6 integrators
int convert_table(const Call& c, const ndpp_ace_reaction& a, int NE, int tot, SD* sd) {
  sd->NE = NE;
  sd->e_grid.resize(NE); sd->row_ptr.resize(NE + 1); sd->intt.resize(NE);
  sd->eout.resize(tot); sd->pdf.resize(tot); sd->cdf.resize(tot);
  // angular-only tables (kind 1) go into host-side batches, law 9 reads column 1 of every row on
  // the host; the rest is file 6 (in_cm, not yet known here, only chooses between kinds 2 and 4)
  const bool file6_only = !(sd->has_adist && !sd->has_edist) && !(sd->has_adist && sd->law == 9);
  if (file6_only && c.hooks.device_tables) {
    double* fd = nullptr;
    const int rc = convert_distro_keep(c.M, &a, c.G, c.e_bins, NE, tot, sd->e_grid.data(), sd->row_ptr.data(),
                                       sd->eout.data(), sd->pdf.data(), sd->cdf.data(), sd->intt.data(), &fd);
    sd->f_dev = std::shared_ptr<double>(fd, [](double* q) { free_converted(q); });
    return rc;
  }
  sd->f.resize((size_t)tot * c.M);
  return ndpp_convert_distro(c.M, &a, c.G, c.e_bins, NE, tot, sd->e_grid.data(), sd->row_ptr.data(),
                             sd->eout.data(), sd->pdf.data(), sd->cdf.data(), sd->intt.data(), sd->f.data());
}

// Law 66 with the option on: the ScattData the reference leaves uninitialised (:105-109), initialised
// here.  There is no table: the grid is the two ends of the reaction's range, which the grid builder and
// the row search read, and the reaction's angular distribution is left as it is.  Nothing above the top
// group edge: not initialised.
void init_nbody(const Call& c, const ndpp_ace_edist* ed, double threshold_energy, SD* sd) {
  const double e_lo = (threshold_energy > c.e_bins[0]) ? threshold_energy : c.e_bins[0];
  if (e_lo >= c.Etop) return;
  sd->is_init = true;
  sd->law = 66;
  sd->has_edist = true;
  sd->edist = ed;
  sd->NE = 2;
  sd->e_grid = {e_lo, c.Etop};
}

// every reaction's SD list; RxnState lives here, one per reaction
int convert_reactions(const Call& c, std::vector<SD>* sds) {
  const ndpp_ace_nuclide* nuc = c.nuc;
  for (int ir = 0; ir < nuc->n_reaction; ++ir) {
    const ndpp_ace_rxn& rx = nuc->reactions[ir];
    if (rx.threshold < 1 || rx.threshold > nuc->n_grid)
      return fail(NDPP_EINVAL, "reaction %d: threshold index %d outside the grid", ir, rx.threshold);
    RxnState st;
    st.has_angle_dist = rx.has_angle_dist != 0;
    st.in_cm = rx.scatter_in_cm != 0;
    const size_t first = sds->size();
    for (int k = 0; k < std::max(rx.n_edist, 1); ++k) {
      const ndpp_ace_edist* ed = (rx.n_edist > 0) ? &rx.edist[k] : nullptr;
      const ndpp_ace_reaction a = reaction_view(nuc, rx, ed, st);
      int is_init = 0, law = 0, NE = 0, tot = 0;
      int rc = ndpp_scattdata_shape(&a, &is_init, &law, &NE, &tot);
      if (rc) return rc;
      SD sd;
      sd.rxn = &rx;
      sd.is_init = is_init != 0;
      if (c.nbody && ed && ed->law == 66 && valid_scatter(rx.MT)) {
        if (c.n_tab > 0 && !c.nbody_tab)
          return fail(NDPP_EINVAL, "MT %d: law 66 (N-body phase space) has Legendre output only", rx.MT);
        if (ed->n_data < 2 || !ed->data)
          return fail(NDPP_EINVAL, "MT %d: law 66 needs its 2 data words (the number of bodies and Ap)", rx.MT);
        init_nbody(c, ed, a.threshold_energy, &sd);
      } else if (sd.is_init) {
        sd.law = law;
        after_init(c, ed, a.threshold_energy, &sd, &st);
        rc = convert_table(c, a, NE, tot, &sd);
        if (rc) return rc;
      }
      sds->push_back(std::move(sd));
    }
    // scatter_in_cm as the integrators will see it (the flag lives on the reaction)
    for (size_t k = first; k < sds->size(); ++k) (*sds)[k].in_cm = st.in_cm;
  }
  return NDPP_OK;
}

// ---- free-gas cutoff and inelastic threshold (:103-123)
int cutoff_and_threshold(const Call& c, const std::vector<SD>& sds, double* cutoff, double* inel_thresh) {
  *cutoff = 0.0;
  *inel_thresh = c.Etop;
  bool any = false;
  for (const SD& sd : sds) {
    if (!sd.is_init) continue;
    any = true;
    if (sd.rxn->MT == 2) *cutoff = c.nuc->freegas_cutoff;
    else if (c.nuc->energy[sd.rxn->threshold - 1] < *inel_thresh)
      *inel_thresh = c.nuc->energy[sd.rxn->threshold - 1];
  }
  return any ? NDPP_OK : fail(NDPP_EINVAL, "no scattering reaction in this nuclide");
}

// ---- incoming grids (:134-135), or the caller's, and the matrices.  What a failure leaves allocated
// is freed by the caller's one exit.
int make_grids(Call& c, const std::vector<SD>& sds, double cutoff, double inel_thresh, const GivenGrids* given,
               int nuscatt, ndpp_scatt_result* out) {
  const ndpp_ace_nuclide* nuc = c.nuc;
  std::vector<ndpp_sd_grid> gs(sds.size());
  for (size_t k = 0; k < sds.size(); ++k) {
    gs[k].is_init = sds[k].is_init;
    gs[k].MT = sds[k].rxn->MT;
    gs[k].Q_value = sds[k].rxn->Q_value;
    gs[k].n = sds[k].NE;
    gs[k].e_grid = sds[k].e_grid.data();
  }
  int n_el = 0, n_in = 0;
  if (given) {
    n_el = given->n_el;
    n_in = given->n_inel;
  } else {
    const int rc = ndpp_create_ein_grid(c.p, (int)gs.size(), gs.data(), c.n_bins, c.e_bins, nuc->n_grid, nuc->energy,
                                        nuc->awr, nuc->kT, cutoff, inel_thresh, 0, nullptr, &n_el, 0, nullptr, &n_in);
    if (rc) return rc;
  }
  out->L = c.L; out->G = c.G; out->n_el = n_el; out->n_inel = n_in;
  c.hc.lap(0);
  // (an empty given list still gets its one-element arrays: a NULL here means out of memory)
  out->ein_el = (double*)calloc(std::max<size_t>((size_t)n_el, 1), sizeof(double));
  out->el_mat = (double*)calloc(std::max<size_t>((size_t)n_el * c.GL, 1), sizeof(double));
  if (n_in) {
    out->ein_inel = (double*)calloc((size_t)n_in, sizeof(double));
    // (overwritten as a whole by the download of the device-side reaction sum)
    out->inel_mat = (double*)malloc(std::max<size_t>((size_t)n_in * c.GL, 1) * sizeof(double));
    if (nuscatt) out->nuinel_mat = (double*)malloc(std::max<size_t>((size_t)n_in * c.GL, 1) * sizeof(double));
  }
  if (!out->ein_el || !out->el_mat || (n_in && (!out->ein_inel || !out->inel_mat)) ||
      (n_in && nuscatt && !out->nuinel_mat))
    return fail(NDPP_ENOMEM, "out of host memory for the result matrices");
  if (given) {
    std::copy(given->ein_el, given->ein_el + n_el, out->ein_el);
    if (n_in) std::copy(given->ein_inel, given->ein_inel + n_in, out->ein_inel);
  } else {
    const int rc = ndpp_create_ein_grid(c.p, (int)gs.size(), gs.data(), c.n_bins, c.e_bins, nuc->n_grid, nuc->energy,
                                        nuc->awr, nuc->kT, cutoff, inel_thresh, n_el, out->ein_el, &n_el,
                                        std::max(n_in, 0), out->ein_inel, &n_in);
    if (rc) return rc;
  }
  c.hc.lap(1);
  return NDPP_OK;
}

// ---- one reaction on one grid: the incoming energies it contributes to (where: their rows of the
// matrices), and per energy what the batch call (ein, row_lo, w_hi) and the sum (scale = sigma, pv =
// p_valid, yield) need.  Sized for the grid once, refilled per reaction.
struct Selection {
  std::vector<int> where, row_lo;
  std::vector<double> ein, w_hi, scale, pv, yield;
  int nb = 0;
  explicit Selection(int n) : where(n), row_lo(n), ein(n), w_hi(n), scale(n), pv(n), yield(n) {}
};

// scatt_interp_distro's bookkeeping; no device work
int select_energies(const Call& c, const SD& sd, bool elastic, int NEin, const double* Ein, Selection* s) {
  const ndpp_ace_nuclide* nuc = c.nuc;
  const ndpp_ace_rxn& rx = *sd.rxn;
  const double* sig = elastic ? nuc->elastic : rx.sigma;
  const int nsig = elastic ? nuc->n_grid : rx.n_sigma;
  if (!sig || nsig < 1) return fail(NDPP_EINVAL, "MT %d has no cross section", rx.MT);
  if (sd.NE < 2) return fail(NDPP_EINVAL, "MT %d: fewer than 2 tabulated energies", rx.MT);
  int nb = 0;
  for (int iE = 0; iE < NEin; ++iE) {
    const double E = Ein[iE];
    // (E > Etop: the top point, copied by copy_top_rows)
    if ((E <= nuc->energy[rx.threshold - 1] && rx.threshold > 1) || E > c.Etop) continue;  // :423-431
    double sigS;
    int iEg;
    if (E >= nuc->energy[nuc->n_grid - 1]) {                             // :432-442
      sigS = sig[nsig - 1];
      iEg = sd.NE - 1;
    } else {
      int ni = (E <= nuc->energy[0]) ? 1 : bsearch1_clamped(nuc->energy, nuc->n_grid, E);
      if (nuc->energy[ni - 1] == nuc->energy[ni]) ni = ni + 1;
      const double fr = (E - nuc->energy[ni - 1]) / (nuc->energy[ni] - nuc->energy[ni - 1]);
      ni = ni - rx.threshold + 1;
      if (ni < 1 || ni + 1 > nsig) return fail(NDPP_EINVAL, "MT %d: cross section shorter than the grid", rx.MT);
      sigS = (1.0 - fr) * sig[ni - 1] + fr * sig[ni];
      if (sigS <= 0.0) continue;                                         // :466-468
      iEg = (E < sd.e_grid[0]) ? 1 : ((E > sd.e_grid[sd.NE - 1]) ? -1 : bsearch1_clamped(sd.e_grid.data(), sd.NE, E));
      if (iEg < 0) return fail(NDPP_EINVAL, "MT %d: E_in %g above its tabulated energies", rx.MT, E);
      if (iEg + 1 <= sd.NE - 1 && sd.e_grid[iEg - 1] >= sd.e_grid[iEg]) iEg = iEg + 1;   // :480-482
    }
    double pval = 1.0;
    if (sd.has_edist && sd.edist) {
      const int rc = tab1(sd.edist->pv_n_regions, sd.edist->pv_nbt, sd.edist->pv_int, sd.edist->pv_n_pairs,
                          sd.edist->pv_x, sd.edist->pv_y, E, &pval);
      if (rc) return rc;
    }
    s->where[nb] = iE;
    s->ein[nb] = E;
    s->row_lo[nb] = iEg - 1;
    s->w_hi[nb] = (E - sd.e_grid[iEg - 1]) / (sd.e_grid[iEg] - sd.e_grid[iEg - 1]);   // :542
    s->scale[nb] = sigS;
    s->pv[nb] = pval;
    ++nb;
  }
  s->nb = nb;
  return NDPP_OK;
}

// the nu-scatter yields of the selected energies (scatt.F90:745-762); the table only where it is summed
int select_yields(const ndpp_ace_rxn& rx, bool with_nu, Selection* s) {
  for (int k = 0; k < s->nb; ++k) {
    s->yield[k] = (double)rx.multiplicity;
    if (with_nu && rx.has_mult_E) {
      const int rc = tab1(rx.mE_n_regions, rx.mE_nbt, rx.mE_int, rx.mE_n_pairs, rx.mE_x, rx.mE_y, s->ein[k],
                          &s->yield[k]);
      if (rc) return rc;
    }
  }
  return NDPP_OK;
}

// ---- integrate_distro for the selected energies of one reaction: the batch call of its kind, Legendre
// or tabular, into the host array res [nb][GL] or (res null) the sink.  cutoff: the free-gas cutoff of
// the elastic grid, 0 on the inelastic one.
int integrate_reaction(const Call& c, const SD& sd, int kind, double cutoff, const Selection& s, double* res,
                       DeviceSink* sink) {
  const ndpp_ace_nuclide* nuc = c.nuc;
  std::vector<int> status(s.nb);
  if (kind == 5 && c.n_tab > 0)
    return nbody_tab_batch_sink(c.p, c.n_tab, nuc->awr, sd.rxn->Q_value, (int)sd.edist->data[0], sd.edist->data[1],
                                s.nb, s.ein.data(), c.G, c.e_bins, res, status.data(), sink);
  if (kind == 5)
    return nbody_batch_sink(c.p, nuc->awr, sd.rxn->Q_value, (int)sd.edist->data[0], sd.edist->data[1], s.nb,
                            s.ein.data(), c.G, c.e_bins, res, status.data(), sink);
  if (kind == 1 && c.n_tab > 0)
    return elastic_tab_batch_sink(c.p, nuc->awr, nuc->kT, cutoff, sd.rxn->Q_value, s.nb, s.ein.data(),
                                  s.row_lo.data(), s.w_hi.data(), sd.NE, sd.f.data(), c.G, c.e_bins, c.n_tab, res,
                                  status.data(), sink);
  if (kind == 1)
    return elastic_leg_batch_sink(c.p, nuc->awr, nuc->kT, cutoff, sd.rxn->Q_value, s.nb, s.ein.data(),
                                  s.row_lo.data(), s.w_hi.data(), sd.NE, sd.f.data(), c.G, c.e_bins, res,
                                  status.data(), sink);
  if (kind == 3) {
    std::vector<double> ftab((size_t)sd.NE * c.M);   // column 1 of every row
    for (int k = 0; k < sd.NE; ++k)
      std::copy(sd.f.begin() + (size_t)sd.row_ptr[k] * c.M, sd.f.begin() + (size_t)(sd.row_ptr[k] + 1) * c.M,
                ftab.begin() + (size_t)k * c.M);
    return law9_batch_sink(c.p, s.nb, s.ein.data(), s.row_lo.data(), s.w_hi.data(), sd.NE, ftab.data(),
                           sd.edist->n_data, sd.edist->data, c.G, c.e_bins, c.n_tab, res, status.data(), sink);
  }
  return file6_batch_sink(c.p, nuc->awr, kind == 2 ? 1 : 0, s.nb, s.ein.data(), s.row_lo.data(), sd.NE,
                          sd.e_grid.data(), sd.row_ptr.data(), sd.eout.data(), sd.pdf.data(), sd.intt.data(),
                          sd.f.data(), c.G, c.e_bins, c.n_tab, res, status.data(), sink, sd.f_dev.get());
}

// ---- ElasticDefer: collect, run, and the top point

// One angular-only reaction with its selected energies as the next "nuclide" of the multi call.  mat: the
// matrix its (L,G) blocks go to (null: the caller keeps track).  Returns its first row in the call.
size_t append_reaction(ElasticDefer* d, const ndpp_ace_nuclide* nuc, double cutoff, const SD& sd,
                       const Selection& s, double* mat, size_t GL) {
  const size_t first = d->ein.size();
  const int k = (int)d->A.size();
  d->A.push_back(nuc->awr); d->kT.push_back(nuc->kT); d->cut.push_back(cutoff); d->Q.push_back(sd.rxn->Q_value);
  for (int j = 0; j < s.nb; ++j) {
    d->ein.push_back(s.ein[j]); d->w.push_back(s.w_hi[j]);
    d->nuc.push_back(k); d->row.push_back(d->n_rows + s.row_lo[j]);
    if (mat) d->dst.push_back(mat + (size_t)s.where[j] * GL);
  }
  d->f_tab.insert(d->f_tab.end(), sd.f.begin(), sd.f.end());
  d->n_rows += sd.NE;
  return first;
}

// what was collected through ONE ndpp_elastic_leg_multi call: rows [d.ein.size()][G * p->order]
int run_elastic_defer(const ndpp_params* p, const ElasticDefer& d, int G, const double* e_bins,
                      std::vector<double>* rows) {
  const int n = (int)d.ein.size();
  if (n == 0) return NDPP_OK;
  rows->resize((size_t)n * G * p->order);
  std::vector<int> status(n);
  return ndpp_elastic_leg_multi(p, (int)d.A.size(), d.A.data(), d.kT.data(), d.cut.data(), d.Q.data(), n,
                                d.ein.data(), d.nuc.data(), d.row.data(), d.w.data(), d.n_rows, d.f_tab.data(), G,
                                e_bins, rows->data(), status.data(), nullptr);
}

// an incoming energy above the top group edge takes the row before it (scatt.F90:664-670, :766-774)
void copy_top_rows(int NEin, const double* Ein, double Etop, size_t GL, double* mat, double* numat) {
  for (int iE = 1; iE < NEin; ++iE)
    if (Ein[iE] > Etop) {
      std::copy(mat + (size_t)(iE - 1) * GL, mat + (size_t)iE * GL, mat + (size_t)iE * GL);
      if (numat) std::copy(numat + (size_t)(iE - 1) * GL, numat + (size_t)iE * GL, numat + (size_t)iE * GL);
    }
}

// ---- The three ways a reaction's moments reach the matrices of a grid: take() one reaction with its
// selected energies, finish() after the last.

// The elastic grid: assigned row by row, not scaled (:494-497, scatt.F90:660).  In a library call the
// angular-only reaction is collected into the mixed batch instead, which fills its rows.
struct ElasticAssign {
  double* mat;
  ElasticDefer* defer;
  ResultStage stage;
  int take(Call& c, const SD& sd, int kind, const Selection& s) {
    if (kind == 1 && defer) {
      append_reaction(defer, c.nuc, c.nuc->freegas_cutoff, sd, s, mat, c.GL);
      return NDPP_OK;
    }
    double* res = stage.get((size_t)s.nb * c.GL);
    if (!res) return fail(NDPP_ENOMEM, "out of host memory for a reaction's moments");
    const int rc = integrate_reaction(c, sd, kind, c.nuc->freegas_cutoff, s, res, nullptr);
    c.hc.lap(3);
    if (rc) return rc;
    parallel_rows(s.nb, c.GL * 2 * sizeof(double), [&](int k0, int k1) {
      for (int k = k0; k < k1; ++k)
        std::copy(res + (size_t)k * c.GL, res + (size_t)(k + 1) * c.GL, mat + (size_t)s.where[k] * c.GL);
    });
    c.hc.lap(4);
    return NDPP_OK;
  }
  int finish(Call&) { return NDPP_OK; }
};

// A small inelastic grid, summed on the host.  The level reactions -- angular distribution only,
// dozens per nuclide, a few hundred incoming energies each -- are collected and integrated by
// ONE ndpp_elastic_leg_multi call (a "nuclide" of that call = one level: its Q and its rows)
// instead of one batch call each; every reaction's moments are kept until all are there and
// then summed in the reaction order of take(): same bits as one call per level
// (Hooks::level_batch off; the tabular output has no multi call).
struct HostSum {
  struct Pending {
    int nb = 0;
    long off = -1;                          // >= 0: first row of this reaction in the level batch
    std::vector<int> where;
    std::vector<double> scale, pv, yld, res;
  };
  double *mat, *numat;
  bool level_batch;
  std::vector<Pending> pend;
  ElasticDefer lvl;
  HostSum(const Call& c, int NEin, double* m, double* nm)
      : mat(m), numat(nm), level_batch(c.n_tab == 0 && c.hooks.level_batch) {
    std::fill(mat, mat + (size_t)NEin * c.GL, 0.0);
    if (numat) std::fill(numat, numat + (size_t)NEin * c.GL, 0.0);
  }
  int take(Call& c, const SD& sd, int kind, const Selection& s) {
    pend.emplace_back();
    Pending& pd = pend.back();
    pd.nb = s.nb;
    pd.where.assign(s.where.begin(), s.where.begin() + s.nb);
    pd.scale.assign(s.scale.begin(), s.scale.begin() + s.nb);
    pd.pv.assign(s.pv.begin(), s.pv.begin() + s.nb);
    pd.yld.assign(s.yield.begin(), s.yield.begin() + s.nb);
    if (level_batch && kind == 1) {
      pd.off = (long)append_reaction(&lvl, c.nuc, 0.0, sd, s, nullptr, c.GL);
      c.hc.lap(2);
      return NDPP_OK;
    }
    pd.res.resize((size_t)s.nb * c.GL);
    const int rc = integrate_reaction(c, sd, kind, 0.0, s, pd.res.data(), nullptr);
    c.hc.lap(3);
    return rc;
  }
  int finish(Call& c) {
    std::vector<double> lvl_res;
    const int rc = run_elastic_defer(c.p, lvl, c.G, c.e_bins, &lvl_res);
    if (!lvl.ein.empty()) c.hc.lap(3);
    if (rc) return rc;
    for (const Pending& pd : pend)             // the reaction sum, in the order of take()
      for (int k = 0; k < pd.nb; ++k) {
        double* dst = mat + (size_t)pd.where[k] * c.GL;
        double* nudst = numat ? numat + (size_t)pd.where[k] * c.GL : nullptr;
        const double* src = pd.off >= 0 ? lvl_res.data() + (size_t)(pd.off + k) * c.GL : pd.res.data() + (size_t)k * c.GL;
        for (size_t j = 0; j < c.GL; ++j) {
          const double t = src[j] * pd.scale[k] * pd.pv[k];     // :496
          dst[j] = dst[j] + t;                                  // scatt.F90:753
          if (nudst) nudst[j] = nudst[j] + pd.yld[k] * t;       // :762
        }
      }
    c.hc.lap(4);
    return NDPP_OK;
  }
};

// A large inelastic grid, summed on the device through ReactionSum: one staged upload per reaction, the
// batch call hands its moments to the sink, one download at the end.
struct DeviceSum {
  double *mat, *numat;
  ReactionSum rsum;
  int init(const Call& c, int NEin) { return rsum.init((size_t)NEin, c.GL, numat != nullptr, NEin); }
  int take(Call& c, const SD& sd, int kind, const Selection& s) {
    int rc = rsum.stage(s.nb, s.where.data(), s.scale.data(), s.pv.data(), s.yield.data());
    if (rc) return rc;
    rc = integrate_reaction(c, sd, kind, 0.0, s, nullptr, &rsum);
    c.hc.lap(3);
    return rc;
  }
  int finish(Call& c) {
    const int rc = rsum.download(mat, numat);
    if (rc) return rc;
    c.hc.lap(4);
    return NDPP_OK;
  }
};

// the reactions of one grid, in their order, through one of the three
template <class Acc>
int run_reactions(Call& c, const std::vector<SD>& sds, bool elastic, int NEin, const double* Ein, bool with_nu,
                  Acc& acc) {
  Selection s(NEin);
  for (const SD& sd : sds) {
    if (!sd.is_init || (sd.rxn->MT == 2) != elastic) continue;
    int rc = select_energies(c, sd, elastic, NEin, Ein, &s);
    if (rc) return rc;
    c.hc.lap(2);
    if (s.nb == 0) continue;
    if (!elastic) rc = select_yields(*sd.rxn, with_nu, &s);
    if (rc == NDPP_OK) rc = acc.take(c, sd, distro_kind(sd), s);
    if (rc) return rc;
  }
  return acc.finish(c);
}

// ---- calc_elastic_grid / calc_inelastic_grid.  The reaction sum of a large inelastic grid stays on
// the device; a small one (the shipped two-group structure: a few hundred KB) is summed on the host,
// which costs less than the allocations of the device matrices (0.4 s over the 423 nuclides of the
// library workload).  Hooks::dev_sum_min moves the border.
int run_grid(Call& c, const std::vector<SD>& sds, bool elastic, ndpp_scatt_result* out, ElasticDefer* defer) {
  const int NEin = elastic ? out->n_el : out->n_inel;
  const double* Ein = elastic ? out->ein_el : out->ein_inel;
  double* mat = elastic ? out->el_mat : out->inel_mat;
  double* numat = elastic ? nullptr : out->nuinel_mat;
  if (NEin == 0) return NDPP_OK;
  int rc;
  if (elastic) {
    ElasticAssign acc{mat, defer};
    rc = run_reactions(c, sds, true, NEin, Ein, false, acc);
  } else if ((size_t)NEin * c.GL >= c.hooks.dev_sum_min) {
    DeviceSum acc{mat, numat};
    rc = acc.init(c, NEin);
    if (rc == NDPP_OK) rc = run_reactions(c, sds, false, NEin, Ein, numat != nullptr, acc);
  } else {
    HostSum acc(c, NEin, mat, numat);
    rc = run_reactions(c, sds, false, NEin, Ein, numat != nullptr, acc);
  }
  if (rc) return rc;
  if (elastic && defer) {                                  // filled and copied by the caller
    defer->tops.push_back({mat, Ein, NEin});
    return NDPP_OK;
  }
  copy_top_rows(NEin, Ein, c.Etop, c.GL, mat, numat);
  c.hc.lap(5);
  return NDPP_OK;
}

}  // namespace
}  // namespace ndpp

using namespace ndpp;

extern "C" void ndpp_free_scatt_result(ndpp_scatt_result* r) {
  if (!r) return;
  free(r->ein_el); free(r->ein_inel); free(r->el_mat); free(r->inel_mat); free(r->nuinel_mat);
  memset(r, 0, sizeof(*r));
}

// n_tab = 0: Legendre moments (L = p->order); n_tab > 0: calc_scatt with scatt_type = tabular,
// n_tab lab-cosine bins per group (the tabular batch calls; no deferred or level batches).
// defer: a library's mixed elastic batch; given: the caller's grids instead of create_Ein_grid's.
static int scatt_nuclide_impl(const ndpp_params* p, const ndpp_ace_nuclide* nuc, int n_bins,
                              const double* e_bins, int nuscatt, ndpp_scatt_result* out,
                              ElasticDefer* defer, int n_tab = 0, const GivenGrids* given = nullptr) {
  if (!p || !nuc || !e_bins || !out) return fail(NDPP_EINVAL, "NULL argument");
  memset(out, 0, sizeof(*out));
  if (n_tab < 0 || n_tab > NDPP_MAX_TAB_BINS)
    return fail(NDPP_EINVAL, "n_tab=%d outside 1..%d", n_tab, NDPP_MAX_TAB_BINS);
  if (n_tab > 0 && defer)
    return fail(NDPP_EINVAL, "tabular output has no deferred (mixed-nuclide) elastic batch");
  if (n_bins < 2) return fail(NDPP_EINVAL, "need at least one group");
  if (nuc->n_grid < 2 || !nuc->energy || !nuc->elastic)
    return fail(NDPP_EINVAL, "nuclide energy grid / elastic cross section missing");
  if (nuc->n_reaction < 1 || !nuc->reactions) return fail(NDPP_EINVAL, "nuclide has no reactions");
  Call c(p, nuc, n_bins, e_bins, n_tab);
  std::vector<SD> sds;
  double cutoff, inel_thresh;
  int rc = convert_reactions(c, &sds);
  if (rc == NDPP_OK) rc = cutoff_and_threshold(c, sds, &cutoff, &inel_thresh);
  if (rc == NDPP_OK) rc = make_grids(c, sds, cutoff, inel_thresh, given, nuscatt, out);
  if (rc == NDPP_OK) rc = run_grid(c, sds, true, out, defer);
  if (rc == NDPP_OK) rc = run_grid(c, sds, false, out, nullptr);
  if (rc != NDPP_OK) ndpp_free_scatt_result(out);   // the one exit of every failure after the arguments
  return rc;
}

extern "C" int ndpp_scatt_nuclide(const ndpp_params* p, const ndpp_ace_nuclide* nuc, int n_bins,
                                  const double* e_bins, int nuscatt, ndpp_scatt_result* out) {
  return scatt_nuclide_impl(p, nuc, n_bins, e_bins, nuscatt, out, nullptr);
}

// the deferred elastic grids of a library as ONE mixed batch, each row to its matrix; then the top points
static int flush_library(const ndpp_params* p, int n_bins, const double* e_bins, ElasticDefer* d) {
  int rc = NDPP_OK;
  if (!d->ein.empty()) {
    const int G = n_bins - 1;
    const size_t GL = (size_t)G * p->order;
    std::vector<double> res;
    rc = run_elastic_defer(p, *d, G, e_bins, &res);
    if (rc == NDPP_OK) {
      for (size_t i = 0; i < d->dst.size(); ++i)
        std::copy(res.begin() + i * GL, res.begin() + (i + 1) * GL, d->dst[i]);
      for (const ElasticDefer::Top& t : d->tops) copy_top_rows(t.n, t.Ein, e_bins[G], GL, t.mat, nullptr);
    }
    *d = ElasticDefer();
  }
  return rc;
}

// calc_scatt for a list of nuclides, their elastic grids in ONE mixed batch -- or several, when the
// tables collected so far approach what one batch call addresses (32-bit byte offsets into f_tab:
// run_batch_d).  grids: null (every nuclide builds its own, ndpp_scatt_library) or one GivenGrids per
// nuclide (ndpp_scatt_library_at).
static int scatt_library_impl(const ndpp_params* p, int n_nuclides, const ndpp_ace_nuclide* nuclides,
                              int n_bins, const double* e_bins, int nuscatt, const GivenGrids* grids,
                              ndpp_scatt_result* out) {
  if (n_nuclides < 0 || (n_nuclides > 0 && (!nuclides || !out)))
    return fail(NDPP_EINVAL, "n_nuclides=%d or NULL array", n_nuclides);
  for (int k = 0; k < n_nuclides; ++k) memset(&out[k], 0, sizeof(out[k]));
  ElasticDefer d;
  int rc = NDPP_OK;
  constexpr size_t kFlushBytes = (size_t)3 << 30;
  for (int k = 0; k < n_nuclides && rc == NDPP_OK; ++k) {
    rc = scatt_nuclide_impl(p, &nuclides[k], n_bins, e_bins, nuscatt, &out[k], &d, 0, grids ? &grids[k] : nullptr);
    if (rc == NDPP_OK && d.f_tab.size() * sizeof(double) > kFlushBytes) rc = flush_library(p, n_bins, e_bins, &d);
  }
  if (rc == NDPP_OK) rc = flush_library(p, n_bins, e_bins, &d);
  if (rc != NDPP_OK)
    for (int k = 0; k < n_nuclides; ++k) ndpp_free_scatt_result(&out[k]);
  return rc;
}

extern "C" int ndpp_scatt_library(const ndpp_params* p, int n_nuclides,
                                  const ndpp_ace_nuclide* nuclides, int n_bins,
                                  const double* e_bins, int nuscatt, ndpp_scatt_result* out) {
  return scatt_library_impl(p, n_nuclides, nuclides, n_bins, e_bins, nuscatt, nullptr, out);
}

// a caller's list of incoming energies: positive, finite, never decreasing (the grids
// create_Ein_grid builds keep the duplicates of the tables they merge, so equal neighbours pass)
static int check_given_list(const char* what, int k, int n, const double* e, double Etop) {
  if (n < 0) return fail(NDPP_EINVAL, "scatt_library_at: nuclide %d: %s list of %d energies", k, what, n);
  if (n > 0 && !e) return fail(NDPP_EINVAL, "scatt_library_at: nuclide %d: NULL %s list", k, what);
  // an energy above the top group edge takes the row before it: there must be one
  if (n > 0 && e[0] > Etop)
    return fail(NDPP_EINVAL, "scatt_library_at: nuclide %d: the first %s energy %g is above the top group edge %g", k, what, e[0], Etop);
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(e[i]) || !(e[i] > 0.0))
      return fail(NDPP_EINVAL, "scatt_library_at: nuclide %d: %s energy %d = %g is not positive and finite", k, what, i, e[i]);
    if (i > 0 && e[i] < e[i - 1])
      return fail(NDPP_EINVAL, "scatt_library_at: nuclide %d: %s energies decrease at %d", k, what, i);
  }
  return NDPP_OK;
}

extern "C" int ndpp_scatt_library_at(const ndpp_params* p, int n_nuclides, const ndpp_ace_nuclide* nuclides,
                                     int n_bins, const double* e_bins, int nuscatt, const int* n_el,
                                     const double* const* ein_el, const int* n_inel,
                                     const double* const* ein_inel, ndpp_scatt_result* out) {
  if (n_nuclides > 0 && out)
    for (int k = 0; k < n_nuclides; ++k) memset(&out[k], 0, sizeof(out[k]));
  if (!p || !e_bins) return fail(NDPP_EINVAL, "scatt_library_at: NULL argument");
  if (n_nuclides < 0 || (n_nuclides > 0 && (!nuclides || !out || !n_el || !ein_el || !n_inel || !ein_inel)))
    return fail(NDPP_EINVAL, "scatt_library_at: n_nuclides=%d or NULL array", n_nuclides);
  if (n_bins < 2) return fail(NDPP_EINVAL, "need at least one group");
  std::vector<GivenGrids> grids((size_t)std::max(n_nuclides, 0));
  for (int k = 0; k < n_nuclides; ++k) {
    int rc = check_given_list("elastic", k, n_el[k], ein_el[k], e_bins[n_bins - 1]);
    if (rc == NDPP_OK) rc = check_given_list("inelastic", k, n_inel[k], ein_inel[k], e_bins[n_bins - 1]);
    if (rc) return rc;
    grids[k] = GivenGrids{n_el[k], n_inel[k], ein_el[k], ein_inel[k]};
  }
  return scatt_library_impl(p, n_nuclides, nuclides, n_bins, e_bins, nuscatt, grids.data(), out);
}

extern "C" int ndpp_scatt_nuclide_tab(const ndpp_params* p, int n_tab, const ndpp_ace_nuclide* nuc, int n_bins,
                                      const double* e_bins, int nuscatt, ndpp_scatt_result* out) {
  if (out) memset(out, 0, sizeof(*out));
  if (n_tab < 1 || n_tab > NDPP_MAX_TAB_BINS)
    return fail(NDPP_EINVAL, "n_tab=%d outside 1..%d", n_tab, NDPP_MAX_TAB_BINS);
  return scatt_nuclide_impl(p, nuc, n_bins, e_bins, nuscatt, out, nullptr, n_tab);
}

// one nuclide after the other: the tabular elastic grids are not batched across nuclides, so the
// results are those of ndpp_scatt_nuclide_tab by construction
extern "C" int ndpp_scatt_library_tab(const ndpp_params* p, int n_tab, int n_nuclides,
                                      const ndpp_ace_nuclide* nuclides, int n_bins, const double* e_bins,
                                      int nuscatt, ndpp_scatt_result* out) {
  if (n_nuclides < 0 || (n_nuclides > 0 && (!nuclides || !out)))
    return fail(NDPP_EINVAL, "n_nuclides=%d or NULL array", n_nuclides);
  for (int k = 0; k < n_nuclides; ++k) memset(&out[k], 0, sizeof(out[k]));
  int rc = NDPP_OK;
  for (int k = 0; k < n_nuclides && rc == NDPP_OK; ++k)
    rc = ndpp_scatt_nuclide_tab(p, n_tab, &nuclides[k], n_bins, e_bins, nuscatt, &out[k]);
  if (rc != NDPP_OK)
    for (int k = 0; k < n_nuclides; ++k) ndpp_free_scatt_result(&out[k]);
  return rc;
}
