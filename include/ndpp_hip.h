/*
 * ndpp_hip.h -- C ABI of libndpp_hip.so, the MI355X (gfx950) implementation of
 * NDPP's scattering-moment integration hot path.
 *
 * The reference (ndpp/ndpp, Fortran) has no FFI; its seams are module
 * procedures.  Each entry point below names the reference procedure it
 * replaces (file:line under the reference's src/).  Conventions:
 *   - all reals are IEEE double, all integers 32-bit;
 *   - arrays are 0-based but keep the Fortran (column-major) element order, so
 *     a Fortran caller can pass c_loc(array) unchanged:  distro(order,groups)
 *     is double[G][L] with the Legendre index fastest;
 *   - pointers are HOST pointers unless the function name ends in _d;
 *   - the caller allocates outputs; outputs are fully written;
 *   - return 0 on success, a negative errno-style code otherwise; the library
 *     never calls exit()/stop (the reference's fatal_error -> stop,
 *     error.F90:79-154, becomes a return code + per-point status word);
 *   - the caller selects the device (hipSetDevice) before calling; calls are
 *     re-entrant per device; there is NO CPU fallback: without a usable HIP
 *     device every compute entry point returns NDPP_EDEVICE.
 * INTEGRATION.md shows the ISO_C_BINDING interface block for each function.
 */
#ifndef NDPP_HIP_H
#define NDPP_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDPP_OK         0
#define NDPP_EDEVICE   (-5)    /* HIP runtime error / no device              */
#define NDPP_ENOMEM    (-12)   /* workspace allocation failed                */
#define NDPP_EINVAL    (-22)   /* bad argument                               */
#define NDPP_EOVERFLOW (-75)   /* adaptive tree outgrew the workspace        */

/* per-E_in status bits */
#define NDPP_ST_OK        0
#define NDPP_ST_NONFINITE 1    /* NaN/Inf in the result row                  */
#define NDPP_ST_RANGE     2    /* E_in / row index outside the tables        */
#define NDPP_ST_ORDER_NOISE 4  /* retired (never set since 0.4).  Rounds 2-3 raised it on file-6 /
                                  law-9 batches with order > 8: their moments of orders 8-10 agreed
                                  with the reference's only to its own rounding noise (1e-10 ...
                                  3e-10, legendre.F90:46-140).  Those moments are now evaluated in the
                                  reference's operation order and hold the 1e-10 bar up to P10. */

#define NDPP_ST_TAB_UNSETTLED 8 /* tabular free gas: an E' piece of the row did not settle to the
                                  error test within 128 panels (the finest estimate is kept) */

/* per-event status of ndpp_scatt_sample (a value, not a bit set) */
#define NDPP_SAMPLE_OK         0
#define NDPP_SAMPLE_SKIPPED    1  /* E_in outside the grid or not positive and finite, or a u outside [0, 1) */
#define NDPP_SAMPLE_BADROW     2  /* a negative or non-finite group mass, bin or moment in the blended row */
#define NDPP_SAMPLE_ZEROROW    3  /* nothing scatters at this energy: every group mass is zero          */
#define NDPP_SAMPLE_NEGDENSITY 4  /* Legendre: the density is negative at the cosine drawn (still returned) */
/* per-event status of ndpp_scatt_score (a value, not a bit set) */
#define NDPP_SCORE_OK          0
#define NDPP_SCORE_SKIPPED     1  /* E_in outside the grid or not positive and finite, a weight that is not finite, a bin outside [0, n_bins) */
#define NDPP_SCORE_BADROW      2  /* normalize = 1: a negative or non-finite group mass in the blended row */
#define NDPP_SCORE_ZEROROW     3  /* normalize = 1: every group mass is zero                             */
/* the scored events of a tally bin are summed in chunks of this many (part of the definition) */
#define NDPP_SCORE_CHUNK       256
/* ndpp_scatt_score_info: what the calling thread's last ndpp_scatt_score did.  MEASUREMENT ONLY, NOT
 * STABLE: these indices, their number and the entry point itself serve tools/bench_score.py and the
 * tests, and may change or go without notice; a consumer of the tallies has no use for them.       */
#define NDPP_SCORE_INFO_BRACKET_MS  0  /* host: bracket and classify                                  */
#define NDPP_SCORE_INFO_FACTOR_MS   1  /* device, waited for: masses, bands, and with normalize = 1 the factors and the status download */
#define NDPP_SCORE_INFO_GROUP_MS    2  /* host: counting sort by bin and the chunk table              */
#define NDPP_SCORE_INFO_UPLOAD_MS   3  /* allocations and host-to-device copies                       */
#define NDPP_SCORE_INFO_KERNEL_MS   4  /* device events around gather, chunk and fold kernels         */
#define NDPP_SCORE_INFO_DOWNLOAD_MS 5
#define NDPP_SCORE_INFO_PASSES      6  /* passes over the partial buffer                              */
#define NDPP_SCORE_INFO_SCORED      7  /* scored events                                               */
#define NDPP_SCORE_INFO_CHUNKS      8  /* chunks                                                      */
#define NDPP_SCORE_INFO_LEN         9

#define NDPP_MAX_ORDER 11      /* L = scatt_order+1 <= 11 (ndpp.F90:290-301) */

/* <scatt_type> (constants.F90, ndpp.F90:280-287): what a scattering row holds */
#define NDPP_SCATT_LEGENDRE 0  /* L Legendre moments per (E_in, group)                 */
#define NDPP_SCATT_TABULAR  1  /* N bins of the lab cosine per (E_in, group)            */
#define NDPP_MAX_TAB_BINS 128  /* 1 <= N <= 128                                        */

/* Module `global`'s hidden numerics (global.F90:32-59, defaults
 * constants.F90:70-100, set from ndpp.xml at ndpp.F90:355-423) plus the two
 * sizes every kernel needs.  Read-only during a call.  Every batch call refuses
 * with NDPP_EINVAL: adaptive_mu_its or adaptive_eout_its outside 0..31 (the
 * level counters and stacks are sized for 32 levels), and a tolerance (sab_threshold,
 * brent_mu_thresh, adaptive_mu_tol, adaptive_eout_tol) that is negative, NaN or
 * infinite (the reference reads only values >= 0). */
typedef struct ndpp_params {
  int    order;              /* L = scatt_order + 1 Legendre moments          */
  int    mu_bins;            /* M, points of the uniform mu grid (2001)       */
  double sab_threshold;      /* SAB_THRESHOLD        1e-6                     */
  double brent_mu_thresh;    /* BRENT_MU_THRESH      1e-6                     */
  double adaptive_mu_tol;    /* ADAPTIVE_MU_TOL      1e-7                     */
  double adaptive_eout_tol;  /* ADAPTIVE_EOUT_TOL    1e-8                     */
  int    adaptive_mu_its;    /* ADAPTIVE_MU_ITS      15                       */
  int    adaptive_eout_its;  /* ADAPTIVE_EOUT_ITS    15                       */
  int    ne_per_grp;         /* NE_PER_GRP           20                       */
  int    sab_epts_per_bin;   /* SAB_EPTS_PER_BIN     10  (grid builders)      */
  int    extend_pts;         /* EXTEND_PTS           50  (grid builders)      */
  int    inel_extend_pts;    /* INEL_EXTEND_PTS      30  (grid builders)      */
} ndpp_params;

/* Device-side work counters of the last batch call (optional out-param). */
typedef struct ndpp_stats {
  unsigned long long k_evals;      /* free-gas kernel evaluations (exp count) */
  unsigned long long mu_visits;    /* joint mu-tree node visits               */
  unsigned long long mu_integrals; /* inner (mu) adaptive integrals           */
  unsigned long long eout_nodes;   /* outer (E_out) adaptive tree nodes       */
  double             mu_kernel_ms; /* sum of hipEvent spans of fg_mu_kernel   */
  int                mu_kernel_launches;
  double             total_ms;     /* hipEvent time of the whole batch        */
  unsigned long long wave_iters;   /* fg_mu_kernel loop trips, summed over waves */
  unsigned long long lane_iters;   /* ... of which lanes doing a node (<= 64x)   */
  unsigned long long order_visits; /* sum over node visits of active orders      */
  double             mu_level_ms[32]; /* fg_mu_kernel time per outer-tree level  */
  double             mu_busy_ms;   /* time with at least one inner-integration launch
                                      (fg_mu_kernel, fg_gauss_kernel) in flight (the
                                      pipeline contexts of a batch overlap theirs)       */
  int                contexts;     /* pipeline contexts that ran side by side (1 or 2)    */
  unsigned long long gauss_integrals; /* inner integrals (every row of the job) done by the
                                      certified Gauss rule instead of the walk           */
  double             gauss_ms;     /* sum of hipEvent spans of fg_gauss_kernel            */
} ndpp_stats;

void        ndpp_default_params(ndpp_params *p);
const char *ndpp_version(void);
/* message of the last failing call on this thread ("" if none) */
const char *ndpp_last_error(void);
/* Device time (ms, hipEvent bracket) of the kernels of this thread's last batch
 * call; host<->device staging is outside the bracket.  Measurement aid.        */
float ndpp_last_gpu_ms(void);
/* Device time (ms) the calling thread's batch calls have spent per kernel family since the last
 * reset -- what a whole-nuclide call (ndpp_scatt_nuclide) is made of.  Families, in order:
 * free-gas inner walk (fg_mu_kernel), free-gas other stages, file4-CM (+ classification),
 * file6-CM, file6-lab, law 9, S(alpha,beta), chi, ACE -> tabular conversion.  ndpp_profile_get
 * fills min(n, #families) entries and returns the number of families.  Measurement aid.     */
#define NDPP_PROFILE_FAMILIES 9
void        ndpp_profile_reset(void);
int         ndpp_profile_get(double *ms, int n);
/* number of visible HIP devices (0 if none); never fails */
int         ndpp_device_count(void);
/* Which free-gas moments this build integrates in the reference's own arithmetic (about 1.5x the
 * cost of the product arithmetic; replaces nothing in the reference -- it is the reference's
 * freegas.F90:415-553 operation for operation): every incoming energy whose bracketing table
 * rows are not linear in mu (ndpp_freegas_rough_rows: rough[row] = 1; host-side mirror of what
 * the batch calls decide on the device), and, on linear rows, the energies below
 * ndpp_freegas_strict_below (MeV; 0 = never, +inf = always).  For cost models that balance work
 * across GPUs (ndpp_amd/dist.py) and for tests.                                              */
double      ndpp_freegas_strict_below(int groups, double A, double kT);
int         ndpp_freegas_rough_rows(int mu_bins, int n_rows, const double *f_tab, int *rough);
/* Select / query the calling thread's device, for hosts that do not link HIP themselves (a
 * Fortran host with one MPI rank or OpenMP thread per GPU; the reference's ranks each take a
 * block of nuclides, ndpp.F90:934-950).  Every entry point works on the calling thread's
 * current device; the cached workspace and the lock that serialises batch calls are per
 * device, so threads that selected different devices run concurrently.                  */
int         ndpp_set_device(int device);
int         ndpp_get_device(void);      /* ordinal >= 0, or a negative error code */
/* free the cached workspace of the current device */
int         ndpp_release_workspace(void);
/* Allocate the cached device workspace ahead of time: bytes = 0 reserves what the largest
 * batch may take (min(60 % of free HBM, 128 GB)).  Without it the first large batch pays
 * for the allocation (up to seconds for ~100 GB).                                      */
int         ndpp_reserve_workspace(size_t bytes);
/* Device buffers for hosts that call the *_d entry points without linking HIP themselves
 * (e.g. a Fortran host that keeps its tables resident across calls).  ndpp_dev_alloc
 * returns NULL on failure (message in ndpp_last_error); copies are synchronous.          */
void       *ndpp_dev_alloc(size_t bytes);
int         ndpp_dev_free(void *p);
int         ndpp_dev_upload(void *dst_d, const void *src, size_t bytes);
int         ndpp_dev_download(void *dst, const void *src_d, size_t bytes);
int         ndpp_dev_synchronize(void);   /* hipDeviceSynchronize on the current device */

/* ---- B-fine: replaces `subroutine integrate_freegas_leg(Ein, A, kT, fEmu,
 * mu, E_bins, order, distro)` freegas.F90:18-146.  fEmu[M] is f(mu) on the
 * uniform grid mu[M] (scattdata_header.F90:251-257); mu may be NULL, otherwise
 * it must equal that grid bit for bit (NDPP_EINVAL if not -- the reference's
 * calc_fgk indexing, freegas.F90:437-448, is only meaningful on it).
 * distro[G][L] is fully written (normalised so that sum_g P0 = 1).          */
int ndpp_integrate_freegas_leg(const ndpp_params *p, double Ein, double A,
                               double kT, const double *fEmu, const double *mu,
                               const double *E_bins, int n_bins, double *distro);

/* ---- B-fine: replaces `subroutine integrate_file4_cm_leg(fw, Ein, awr, Q,
 * E_bins, w, order, distro)` scattdata_header.F90:956-1078.  Unlike the
 * Fortran (whose callers pre-zero distro, :545-546,:569) distro[G][L] is fully
 * written: groups the routine does not reach are 0.                          */
int ndpp_integrate_file4_cm_leg(const ndpp_params *p, const double *fw,
                                double Ein, double awr, double Q,
                                const double *E_bins, int n_bins,
                                const double *w, double *distro);

/* ---- B-batch: the adist-only branch of `integrate_distro`
 * (scattdata_header.F90:533-591) evaluated for n_ein incoming energies of ONE
 * ScattData (one reaction): for every E_in both bracketing rows of the
 * tabulated angular distribution are integrated at that same E_in and blended
 *     out = lo*(1-f) + hi*f                     (:566,:589)
 * with integrate_freegas_leg where ein < freegas_cutoff (MT=2 only: pass
 * freegas_cutoff = 0 for other reactions) and integrate_file4_cm_leg (with Q)
 * elsewhere (:548-564).
 *   f_tab  [n_rows][M]  this%distro(iE)%data(:,1) rows, contiguous
 *                       (n_rows * M * 8 bytes < 4 GiB per call: NDPP_EINVAL otherwise)
 *   row_lo [n_ein]      0-based lower bracketing row (upper = row_lo+1)
 *   w_hi   [n_ein]      f of :542
 *   out    [n_ein][G][L]
 *   status [n_ein]      NDPP_ST_* bits, may be NULL
 * This is the loop body of calc_elastic_grid (scatt.F90:633-672) minus the
 * sigma/threshold bookkeeping of scatt_interp_distro, which stays host-side. */
int ndpp_elastic_leg_batch(const ndpp_params *p, double A, double kT,
                           double freegas_cutoff, double Q, int n_ein,
                           const double *ein, const int *row_lo,
                           const double *w_hi, int n_rows, const double *f_tab,
                           int G, const double *e_bins, double *out,
                           int *status, ndpp_stats *stats);

/* Same, with ein/row_lo/w_hi/f_tab/e_bins/out/status already resident in
 * device memory (HBM) of the current device; work is enqueued on `stream`
 * (a hipStream_t, NULL = default stream) and the call returns after the batch
 * has completed on the device (it synchronises the stream).                 */
int ndpp_elastic_leg_batch_d(const ndpp_params *p, double A, double kT,
                             double freegas_cutoff, double Q, int n_ein,
                             const double *ein_d, const int *row_lo_d,
                             const double *w_hi_d, int n_rows,
                             const double *f_tab_d, int G,
                             const double *e_bins_d, double *out_d,
                             int *status_d, void *stream, ndpp_stats *stats);

/* Mixed-nuclide form of the two calls above: ONE call for the elastic grids of a whole
 * library shard.  Incoming energy i belongs to nuclide nuc_of_ein[i] (0-based), whose
 * awr, kT, free-gas cutoff and Q are A[k], kT[k], freegas_cutoff[k], Q[k]; row_lo[i]
 * indexes the concatenated table f_tab[n_rows][mu_bins] of all nuclides.  The group
 * structure is common.  Results are bit-identical to per-nuclide calls; the point is
 * occupancy: a nuclide has only 10^2-10^3 free-gas points and every level of the
 * breadth-first pipeline lasts as long as its slowest inner integral, so small batches
 * leave most of the GPU idle (measured: 423 nuclides, 2.1e5 points, 273 s as 423
 * calls vs one call).  _d: all arrays are device pointers.      */
int ndpp_elastic_leg_multi(const ndpp_params *p, int n_nuc, const double *A, const double *kT,
                           const double *freegas_cutoff, const double *Q, int n_ein,
                           const double *ein, const int *nuc_of_ein, const int *row_lo,
                           const double *w_hi, int n_rows, const double *f_tab, int G,
                           const double *e_bins, double *out, int *status, ndpp_stats *stats);
int ndpp_elastic_leg_multi_d(const ndpp_params *p, int n_nuc, const double *A_d,
                             const double *kT_d, const double *cutoff_d, const double *Q_d,
                             int n_ein, const double *ein_d, const int *nuc_of_ein_d,
                             const int *row_lo_d, const double *w_hi_d, int n_rows,
                             const double *f_tab_d, int G, const double *e_bins_d,
                             double *out_d, int *status_d, void *stream, ndpp_stats *stats);

/* ---- B-batch: the edist branches of `integrate_distro`
 * (scattdata_header.F90:593-656) for n_ein incoming energies of ONE ScattData
 * whose secondary distribution is a correlated energy-angle table (ACE laws
 * 4 / 44 / 61 after convert_distro):  unit-base interpolation between the two
 * bracketing incoming energies (`unitbase` :1521, `cast_to_unitbase` :1554,
 * `interp_unitbase` :1616 -- fused, the fEmu(M,|ub|) table is never
 * materialised) followed by
 *   frame_cm = 1: `integrate_file6_cm_leg`  (:1085-1266, uses awr, ne_per_grp)
 *   frame_cm = 0: `integrate_file6_lab_leg` (:1334-1450).
 * The ScattData is passed flattened (CSR over incoming energies):
 *   e_grid  [n_rows]           this%E_grid
 *   row_ptr [n_rows+1]         offsets of each row's outgoing-energy block
 *   eout,pdf[row_ptr[n_rows]]  this%Eouts(k)%data, this%pdfs(k)%data
 *   intt    [n_rows]           this%INTT (1 histogram, 2 lin-lin, 3..5 log forms)
 *   f       [row_ptr[n_rows]][M]  this%distro(k)%data(:, j): one f(mu) column per
 *                              (row, outgoing energy), contiguous in mu
 *   row_lo  [n_ein]            0-based iE of scatt_interp_distro (:471-482)
 *   out     [n_ein][G][L]      fully written; NOT multiplied by sigma*p_valid
 * Every row needs >= 2 outgoing energies.  Bit-identical to the Fortran.      */
int ndpp_file6_leg_batch(const ndpp_params *p, double awr, int frame_cm, int n_ein,
                         const double *ein, const int *row_lo, int n_rows,
                         const double *e_grid, const int *row_ptr,
                         const double *eout, const double *pdf, const int *intt,
                         const double *f, int G, const double *e_bins, double *out,
                         int *status);

/* ---- B-batch: the law-9 branch of `integrate_distro` (:605-638): for every
 * E_in `law9_scatter_lab_leg` (:1274-1326) on both bracketing rows of the
 * tabulated angular distribution f_tab[n_rows][M], blended (1-f)*lo + f*hi.
 * edata[n_edata] is edist%data: the TAB1 of the nuclear temperature T(E)
 * followed by the restriction energy U.                                       */
int ndpp_law9_leg_batch(const ndpp_params *p, int n_ein, const double *ein,
                        const int *row_lo, const double *w_hi, int n_rows,
                        const double *f_tab, int n_edata, const double *edata,
                        int G, const double *e_bins, double *out, int *status);

/* ---- tabular scattering output (scatt_type = NDPP_SCATT_TABULAR) ----------------------
 * The reference's user guide defines <scatt_type>tabular</scatt_type> with <scatt_order> N as
 * the number of bins in mu; the reference parses it and writes it into the header but never
 * computes it (integrate_distro's SCATT_TYPE_TABULAR branch is empty).  Definition here:
 *   - N equal bins of the LAB cosine, edges b_k = -1 + 2k/N (k = 0..N, b_N = 1 exactly),
 *     1 <= n_tab <= NDPP_MAX_TAB_BINS, anything else NDPP_EINVAL.  (The reference's unused
 *     mu_out array, scatt.F90:129-134, holds N points; the guide's N bins are followed.)
 *   - T[iE][g][k] is the P0 integral of the same path over only the part of its domain whose
 *     lab cosine lies in bin k: same inputs, same blending of the bracketing rows, same
 *     normalisation, so sum_k T[iE][g][k] = P0[iE][g] (to rounding; free gas: to its
 *     quadrature tolerance) and T >= 0 wherever the tables are non-negative.
 *   - out[n_ein][G][N], bin index fastest: the layout of [G][L]; ndpp_scatt_result.L holds N.
 * Per path:
 *   file 4 (two-body CM): the exact integral of the piecewise-linear f(w) over the part of
 *     [wlo, whi] that the exact two-body kinematics map into bin k (R < 1: split at w = -R,
 *     where the lab cosine turns; the reference's tolab replaces the part w < -R, of width
 *     1 - R, by a linear stand-in below -1 that no bin could hold);
 *   file 6 CM / lab, law 9: every panel of the Legendre integrators' lab-cosine grids
 *     contributes its exact integral clipped to each bin (panels narrower than 1e-14 nothing,
 *     as there); the E' points, weights and normalisation are those of the Legendre path;
 *   free gas: the P0 double integral of calc_fgk over E' in the group and mu in
 *     [mu_lo, mu_hi] of find_FG_mu, split at the bin edges: Gauss-Legendre panels in mu,
 *     composite Gauss-Legendre in E' refined until every bin of both rows has settled to
 *     1e-10 of the row's integral over that E' piece plus 1e-13 (the kernel integrates to ~1), normalised to sum_{g,k} T = 1.
 * Each entry takes the argument list of its Legendre twin plus n_tab after p.             */
int ndpp_elastic_tab_batch(const ndpp_params *p, int n_tab, double A, double kT,
                           double freegas_cutoff, double Q, int n_ein,
                           const double *ein, const int *row_lo,
                           const double *w_hi, int n_rows, const double *f_tab,
                           int G, const double *e_bins, double *out,
                           int *status, ndpp_stats *stats);
int ndpp_file6_tab_batch(const ndpp_params *p, int n_tab, double awr, int frame_cm, int n_ein,
                         const double *ein, const int *row_lo, int n_rows,
                         const double *e_grid, const int *row_ptr,
                         const double *eout, const double *pdf, const int *intt,
                         const double *f, int G, const double *e_bins, double *out,
                         int *status);
int ndpp_law9_tab_batch(const ndpp_params *p, int n_tab, int n_ein, const double *ein,
                        const int *row_lo, const double *w_hi, int n_rows,
                        const double *f_tab, int n_edata, const double *edata,
                        int G, const double *e_bins, double *out, int *status);

/* ---- thermal S(alpha,beta) tables ------------------------------------------
 * Flattened `type(SAlphaBeta)` (ace_header.F90:201-235).  Arrays keep the
 * Fortran element order (first index fastest), so a Fortran host passes
 * c_loc(sab%inelastic_mu) etc. unchanged; the continuous secondary mode's
 * per-E_in jagged `inelastic_data(:)` is concatenated (CSR via cont_ptr).     */
typedef struct ndpp_sab_flat {
  double threshold_inelastic, threshold_elastic;   /* 0 elastic: no elastic data */
  int n_inelastic_e_in, n_inelastic_e_out, n_inelastic_mu;
  int secondary_mode;             /* 0 equal, 1 skewed, 2 continuous (constants.F90:144-147) */
  const double *inelastic_e_in;   /* [NEi]                                       */
  const double *inelastic_sigma;  /* [NEi]                                       */
  const double *inelastic_e_out;  /* (NEo, NEi)       modes 0,1                  */
  const double *inelastic_mu;     /* (NMU, NEo, NEi)  modes 0,1                  */
  const int    *cont_ptr;         /* [NEi+1]          mode 2                     */
  const double *cont_e_out;       /* [cont_ptr[NEi]]  inelastic_data(k)%e_out    */
  const double *cont_pdf;         /*                  inelastic_data(k)%e_out_pdf */
  const double *cont_mu;          /* (NMU, sum)       inelastic_data(k)%mu       */
  int elastic_mode;               /* 3 discrete, 4 exact (constants.F90:150-152) */
  int n_elastic_e_in, n_elastic_mu;
  const double *elastic_e_in;     /* [NEe]                                       */
  const double *elastic_P;        /* [NEe]                                       */
  const double *elastic_mu;       /* (NMUe, NEe)                                 */
} ndpp_sab_flat;

/* Replaces the Legendre path of `calc_scattsab` (scatt.F90:543-596):
 * `integrate_sab_el` (sab.F90:21) + `integrate_sab_inel` (:117; discrete :142 or
 * continuous :253) + `combine_sab_grid` (:415) on the incoming grid ein[n_ein]
 * (built by sab_egrid + add_one_more_point on the host).
 *   scatt_mat [n_ein][G][L]   normalised so that sum_g P0 = 1; last point = its
 *                             neighbour (sab.F90:452)
 *   el, inel  [n_ein][G][L]   optional (NULL): the un-normalised sigma-weighted
 *                             parts (sab_int_el / sab_int_inel)
 * Bit-identical to the Fortran.                                               */
int ndpp_sab_batch(const ndpp_params *p, const ndpp_sab_flat *t, int n_ein,
                   const double *ein, int G, const double *e_bins, double *el,
                   double *inel, double *scatt_mat);

/* Tabular output of a thermal table (scatt_type = NDPP_SCATT_TABULAR), opt-in: the writer and the
 * driver take it only where asked to (ndpp_nuclide_file is_sab = 2, `run --thermal-tabular`).
 * A thermal table holds discrete cosines with weights: the density behind ndpp_sab_batch's
 * a_l = sum_i w_i P_l(mu_i) is sum_i w_i delta(mu - mu_i), and its tabular form is exact -- every
 * mass w_i goes, whole, into the bin that holds mu_i.  No quadrature, nothing has to settle.
 *   Bins    n_tab = N equal bins of the lab cosine, 1 <= N <= NDPP_MAX_TAB_BINS (else
 *           NDPP_EINVAL), edges -1 + 2k/N as for the other tabular paths.
 *   Bin of a cosine   the value of ONE floating-point expression,
 *             k = (int)floor((mu + 1.0) * (0.5 * N)), clamped to 0 .. N-1:
 *           a cosine on an interior edge goes to the upper bin, mu = 1 to bin N-1, a cosine
 *           slightly outside [-1, 1] to the end bin.  A cosine that is not finite goes into no bin
 *           and sets NDPP_ST_NONFINITE in the status word of every E_in that read it.  The cosines
 *           are computed exactly as the Legendre kernels compute them (the (1-f) mu_a + f mu_b
 *           blends; the single Bragg-edge cosine 1 - E_bragg/E_in of the reference's coherent
 *           branch, quirk included), in the same translation unit and arithmetic: bins and moments
 *           describe the same set of masses.
 *   Value   T[iE][g][k] is what the Legendre kernel accumulates for order 0 of (iE, g), restricted
 *           to the masses whose cosine lies in bin k: the masses in the same order (io ascending,
 *           imu ascending; continuous mode: lower edge term, upper edge term, interior points,
 *           then / NMU), the same equal or skewed weights, sigma factors, E_in interpolation of the
 *           continuous mode's per-table-row results, and NDPP_ST_RANGE cases.
 *   Normalisation   combine_sab_grid with a group's bin sum in the place of its P0: s is the Kahan
 *           sum of el + inel over (g, then k) in storage order; rows are scaled by 1/s when s > 0,
 *           else zero; the last point copies its neighbour.
 * At N = 1 the three outputs are ndpp_sab_batch's at order 1 (L = 1), bit for bit.  A bin has one
 * fixed order of summation: two calls give the same bits.
 * A histogram of point masses moves mass from one bin to the next as E_in moves, so these rows do
 * not interpolate between grid points the way the piecewise-linear paths' rows do: hence opt-in.
 *   el, inel, scatt_mat [n_ein][G][n_tab], bin index fastest; el and inel optional (NULL)
 *   status [n_ein]      NDPP_ST_* bits, may be NULL
 * The checks are ndpp_sab_batch's, with n_tab in the place of p->order (which is not read), and
 * all come before the device is asked for.                                                   */
int ndpp_sab_tab_batch(const ndpp_params *p, const ndpp_sab_flat *t, int n_tab,
                       int n_ein, const double *ein, int G, const double *e_bins,
                       double *el, double *inel, double *scatt_mat, int *status);

/* ---- fission spectrum chi ---------------------------------------------------
 * One secondary energy distribution: a fission reaction's `edist` (one entry per
 * nested distribution, in `edist%next` chain order -- calc_chi, chi.F90:49-87) or
 * a delayed precursor group's (`nuc%nu_d_edist(j)`, :90-93).                    */
typedef struct ndpp_chi_spectrum {
  int law, n_data;              /* ACE law: 4/61 tabular, 7 Maxwell, 9 evaporation,
                                   11 Watt; other laws yield zeros like the reference */
  const double *data;           /* edist%data                                       */
  int threshold, n_sigma;       /* prompt only: rxn%threshold and the reaction's     */
  const double *sigma;          /*   sigma (nuc%fission for MT 18, chi.F90:72-76)    */
  int has_next;                 /* associated(edist%next)                            */
  int pv_n_regions, pv_n_pairs; /* edist%p_valid (Tab1, endf_header.F90:9-20)        */
  const int *pv_nbt, *pv_int;
  const double *pv_x, *pv_y;
} ndpp_chi_spectrum;

typedef struct ndpp_chi_nuclide {
  int n_grid;
  const double *energy, *fission;        /* nuc%energy, nuc%fission [n_grid]          */
  int nu_t_type, n_nu_t;                 /* 1 polynomial, 2 tabular (constants.F90:187) */
  const double *nu_t_data;
  int nu_d_type, n_nu_d;                 /* 0 none, 2 tabular                          */
  const double *nu_d_data;
  int n_precursor, n_prec_data;
  const double *nu_d_precursor_data;     /* per group: lambda, TAB1 of the yield       */
} ndpp_chi_nuclide;

/* Replaces the incoming-energy loop of `calc_chi` (chi.F90:124-159):
 * ChiData%beta / %prob / %integrate (chidata_header.F90:139-493) for every
 * spectrum, their combination (including the overwrite at chi.F90:135) and the
 * three normalisations.  e_grid[n_ein] is the union grid of the spectra
 * (chi.F90:97-113; ndpp_amd.grid.chi_egrid on the host).
 *   chi_t, chi_p [n_ein][G]            == chi_total/chi_prompt(groups, NE)
 *   chi_d        [n_delay][n_ein][G]   == chi_delay(groups, NE, n_precursor)       */
int ndpp_chi_batch(const ndpp_chi_nuclide *nuc, int n_prompt,
                   const ndpp_chi_spectrum *prompt, int n_delay,
                   const ndpp_chi_spectrum *delay, int G, const double *e_bins,
                   int n_ein, const double *e_grid, double *chi_t, double *chi_p,
                   double *chi_d);

/* ---- ACE -> tabular conversion ------------------------------
 * One reaction and the (nested) energy distribution in hand, as ScattData%init
 * receives them (scattdata_header.F90:78): pointers into the Nuclide's own arrays. */
typedef struct ndpp_ace_reaction {
  int MT;                        /* rxn%MT                                            */
  int law;                       /* edist%law; 0: no energy distribution passed       */
  int has_angle_dist;            /* rxn%has_angle_dist                                */
  int n_adist;                   /* rxn%adist%n_energy                                */
  const double *adist_energy;    /* rxn%adist%energy  [n_adist]                       */
  const int    *adist_type;      /* rxn%adist%type    [n_adist] (constants.F90:138-141) */
  const int    *adist_location;  /* rxn%adist%location[n_adist]                       */
  int n_adist_data;
  const double *adist_data;      /* rxn%adist%data                                    */
  int n_edata;
  const double *edata;           /* edist%data (law 4 / 44 / 61 / 9 blocks)           */
  double threshold_energy;       /* nuc%energy(rxn%threshold)                         */
} ndpp_ace_reaction;

/* Replaces the shape decisions of `ScattData%init` (scattdata_header.F90:78-271):
 * is_init = 0 for a non-scattering MT or an unsupported law (the reference leaves
 * the object uninitialised, :101,:105-109); sd_law = this%law; NE incoming
 * energies; total_np = sum over them of the number of outgoing energies.  Host only. */
int ndpp_scattdata_shape(const ndpp_ace_reaction *r, int *is_init, int *sd_law, int *NE,
                         int *total_np);

/* Replaces `ScattData%init` + `scatt_convert_distro` (scattdata_header.F90:78,:325;
 * convert_file4 :669, convert_file6 :769): evaluates every ACE angular
 * distribution of the reaction on the uniform mu grid.  Outputs are the tables
 * ndpp_elastic_leg_batch / ndpp_file6_leg_batch / ndpp_law9_leg_batch take:
 *   e_grid [NE], row_ptr [NE+1], eout/pdf/cdf [total_np] (zeros where the reference
 *   has none), intt [NE], f [total_np][mu_bins] (== distro(iE)%data(mu_bins, NP)).
 * Reference behaviour kept on purpose: a law-4 table receives the angular
 * distribution in its first two outgoing-energy columns only (:364-366, sic);
 * unknown angular types / file-4 interpolation codes give zero columns.  Where the
 * reference aborts or reads out of bounds this returns NDPP_EINVAL.              */
int ndpp_convert_distro(int mu_bins, const ndpp_ace_reaction *r, int G, const double *e_bins,
                        int NE, int total_np, double *e_grid, int *row_ptr, double *eout,
                        double *pdf, double *cdf, int *intt, double *f);

/* ---- incoming-energy grids of one nuclide, host only --------
 * What the grid builders read of a ScattData: is_init, rxn%MT, rxn%Q_value and its
 * incoming-energy grid (after ndpp_convert_distro / ScattData%init).             */
typedef struct ndpp_sd_grid {
  int is_init;
  int MT;
  double Q_value;
  int n;
  const double *e_grid;
} ndpp_sd_grid;

/* Replaces `merge(a, b, result)` array_merge.F90:13-107 (a zero becomes MIN_EIN
 * 1e-14 unless it meets an equal value).  *n_out is always set; out is written
 * when cap suffices.                                                             */
int ndpp_merge_grids(int na, const double *a, int nb, const double *b, int cap, double *out,
                     int *n_out);

/* Replaces `create_Ein_grid` scatt.F90:166-243 (combine_Eins :252, add_elastic_Eins
 * :313, add_one_more_point :426, add_inelastic_Eins :456): the elastic grid and,
 * if any non-elastic ScattData is initialised, the inelastic grid (else
 * *n_inel = 0).  cutoff = the elastic ScattData's freegas_cutoff (MeV; 0 when the
 * free-gas treatment is off), thresh = the lowest non-elastic threshold energy
 * (calc_scatt, scatt.F90:103-123).  Uses p->extend_pts / p->inel_extend_pts.
 * Two-call protocol: counts are always returned, arrays are written when their
 * capacity suffices.                                                             */
int ndpp_create_ein_grid(const ndpp_params *p, int n_sd, const ndpp_sd_grid *sds, int n_bins,
                         const double *e_bins, int n_nuc, const double *nuc_grid, double awr,
                         double kT, double cutoff, double thresh, int cap_el, double *ein_el,
                         int *n_el, int cap_inel, double *ein_inel, int *n_inel);

/* ---- whole nuclide (SURVEY 8a row H1, 8b "B-batch convenience") ----------------
 * The parts of the ACE data model calc_scatt reads (ace_header.F90:14-164), as
 * pointers into the host's own arrays.                                           */
typedef struct ndpp_ace_edist {     /* one DistEnergy of the rxn%edist -> %next chain */
  int law, n_data;
  const double *data;               /* edist%data                                     */
  int pv_n_regions, pv_n_pairs;     /* edist%p_valid (Tab1)                           */
  const int *pv_nbt, *pv_int;
  const double *pv_x, *pv_y;
} ndpp_ace_edist;

typedef struct ndpp_ace_rxn {
  int MT;
  double Q_value;
  int multiplicity;                 /* rxn%multiplicity                               */
  int threshold;                    /* rxn%threshold: 1-based index into nuc%energy   */
  int scatter_in_cm;
  int n_sigma;
  const double *sigma;              /* rxn%sigma (from the threshold index on)        */
  int has_mult_E;                   /* rxn%multiplicity_with_E; then multiplicity_E:  */
  int mE_n_regions, mE_n_pairs;
  const int *mE_nbt, *mE_int;
  const double *mE_x, *mE_y;
  int has_angle_dist, n_adist;      /* rxn%adist, as in ndpp_ace_reaction             */
  const double *adist_energy;
  const int *adist_type, *adist_location;
  int n_adist_data;
  const double *adist_data;
  int n_edist;                      /* length of the edist chain (0: none)            */
  const ndpp_ace_edist *edist;
} ndpp_ace_rxn;

typedef struct ndpp_ace_nuclide {
  double awr, kT, freegas_cutoff;   /* nuc%awr, %kT, %freegas_cutoff (MeV)            */
  int n_grid;
  const double *energy, *elastic;   /* nuc%energy, nuc%elastic [n_grid]               */
  int n_reaction;
  const ndpp_ace_rxn *reactions;
} ndpp_ace_nuclide;

typedef struct ndpp_scatt_result {  /* allocated by the library                       */
  int n_el, n_inel, L, G;
  double *ein_el, *ein_inel;        /* Ein_el(n_el), Ein_inel(n_inel)                 */
  double *el_mat, *inel_mat;        /* (L, G, n_el), (L, G, n_inel) Fortran order     */
  double *nuinel_mat;               /* NULL unless nuscatt                            */
} ndpp_scatt_result;

/* Replaces `calc_scatt(nuc, energy_bins, scatt_type=Legendre, order, mu_bins, nuscatt,
 * Ein_el, Ein_inel, el_mat, inel_mat, nuinel_mat)` scatt.F90:33-157 (order and mu_bins
 * come in p): ScattData%init + convert_distro for every reaction and nested
 * distribution, create_Ein_grid, calc_elastic_grid, calc_inelastic_grid.  The result
 * arrays are owned by the library until ndpp_free_scatt_result.                    */
int  ndpp_scatt_nuclide(const ndpp_params *p, const ndpp_ace_nuclide *nuc, int n_bins,
                        const double *e_bins, int nuscatt, ndpp_scatt_result *out);
void ndpp_free_scatt_result(ndpp_scatt_result *r);

/* calc_scatt for n_nuclides nuclides (one group structure): identical results to
 * n_nuclides ndpp_scatt_nuclide calls, but the elastic grids of all nuclides -- where
 * > 99 % of the time goes -- are integrated by ONE ndpp_elastic_leg_multi call.
 * out[n_nuclides]; on error every result is freed.                                  */
int  ndpp_scatt_library(const ndpp_params *p, int n_nuclides, const ndpp_ace_nuclide *nuclides,
                        int n_bins, const double *e_bins, int nuscatt, ndpp_scatt_result *out);

/* ndpp_scatt_library at the caller's incoming energies: create_Ein_grid (scatt.F90:166-243) is
 * replaced by the lists n_el[k] / ein_el[k] and n_inel[k] / ein_inel[k] of nuclide k; everything
 * else -- init / convert_distro, the free-gas / file-4 routing per energy, the one mixed elastic
 * batch, the reaction sum, nu-scatter, result ownership -- is the code of the call above.  Replaces
 * nothing in the reference, which integrates on its own grids only; it is what lets a host ask
 * what a row BETWEEN two grid points is (ndpp_grid_error).  Each list holds positive, finite
 * energies that never decrease (equal neighbours pass: the built grids keep the duplicates of
 * the tables they merge); an empty list (n = 0, pointer unread) gives an empty section.  An
 * energy above the top group edge gets the copy of the row before it, as in the built grids;
 * a list that STARTS above the top edge has no such row and is NDPP_EINVAL.
 * Given the grids ndpp_scatt_library built -- or any subset of them -- the rows are the same
 * bits.  Legendre moments only.  NDPP_EINVAL is decided before the device is touched.         */
int  ndpp_scatt_library_at(const ndpp_params *p, int n_nuclides, const ndpp_ace_nuclide *nuclides,
                           int n_bins, const double *e_bins, int nuscatt,
                           const int *n_el, const double *const *ein_el,
                           const int *n_inel, const double *const *ein_inel,
                           ndpp_scatt_result *out);

/* calc_scatt(..., scatt_type = tabular, ...): the two calls above with N = n_tab lab-cosine
 * bins per (E_in, group) instead of Legendre moments (see ndpp_elastic_tab_batch); same
 * incoming grids, same sigma * p_valid weighting and reaction sum, nu-scatter included.
 * el_mat / inel_mat / nuinel_mat are (N, G, NE); r->L = N.  p->order must be valid but is unused.
 * ndpp_scatt_library_tab equals n_nuclides ndpp_scatt_nuclide_tab calls bit for bit.     */
int  ndpp_scatt_nuclide_tab(const ndpp_params *p, int n_tab, const ndpp_ace_nuclide *nuc,
                            int n_bins, const double *e_bins, int nuscatt, ndpp_scatt_result *out);
int  ndpp_scatt_library_tab(const ndpp_params *p, int n_tab, int n_nuclides,
                            const ndpp_ace_nuclide *nuclides, int n_bins, const double *e_bins,
                            int nuscatt, ndpp_scatt_result *out);

/* ---- wire format, host only ---------------------------------------
 * The byte stream the reference's BINARY writers produce (stream access: raw
 * little-endian int32 / float64).  Each function returns the number of bytes of the
 * section (or -1) and writes it when cap suffices, so a host can size, then fill.   */
/* group indices of the energy-bin edges in an incoming grid, ndpp.F90:648-679 (1-based) */
int  ndpp_group_index(int n_bins, const double *e_bins, int n_ein, const double *ein, int *index);
/* print_scatt_bin scatt.F90:1139-1258: NE, Ein, group indices, then per E_in gmin, gmax and
 * the moments of groups gmin..gmax (range found on P0 > 0); elastic, inelastic, nu-inelastic */
long ndpp_scatt_wire(const ndpp_scatt_result *r, int n_bins, const double *e_bins, long cap,
                     unsigned char *buf);
/* print_chi_bin chi.F90:319-353; arrays as ndpp_chi_batch returns them */
long ndpp_chi_wire(int G, int n_ein, int n_prec, const double *e_grid, const double *chi_t,
                   const double *chi_p, const double *chi_d, long cap, unsigned char *buf);
/* file header ndpp.F90:1314-1329 */
long ndpp_header_wire(const char *name, int name_len, double kT, int G, const double *e_bins,
                      int scatt_type, int scatt_order, int nuscatter, int chi_present,
                      int mu_bins, double thin_tol, long cap, unsigned char *buf);

/* ---- formatted outputs, host only ----------------------------------
 * The ASCII library format and ndpp_lib.xml, character for character as the reference's
 * formatted writes produce them (lines end with '\n'); same size-then-fill convention.   */
enum { NDPP_FMT_ASCII = 1, NDPP_FMT_BINARY = 2, NDPP_FMT_HDF5 = 3, NDPP_FMT_NONE = 4,
       NDPP_FMT_HUMAN = 5 };            /* constants.F90:56-58,193-194 */
/* to_str(real(8)) string.F90:408-455 (6 significant digits); out16 holds <= 15 chars + NUL;
 * returns the length */
int  ndpp_real_to_str(double x, char *out16);
/* print_ascii_array output.F90:221-253: four 1PE20.12 fields per line, lines trimmed */
long ndpp_ascii_array(int n, const double *a, long cap, char *buf);
/* print_scatt_ascii scatt.F90:881-997, print_chi_ascii chi.F90:203-244, ASCII header
 * ndpp.F90:1283-1304: the text counterparts of ndpp_scatt_wire / _chi_wire / _header_wire */
long ndpp_scatt_ascii(const ndpp_scatt_result *r, int n_bins, const double *e_bins, long cap,
                      char *buf);
long ndpp_chi_ascii(int G, int n_ein, int n_prec, const double *e_grid, const double *chi_t,
                    const double *chi_p, const double *chi_d, long cap, char *buf);
long ndpp_header_ascii(const char *name, int name_len, double kT, int G, const double *e_bins,
                       int scatt_type, int scatt_order, int nuscatter, int chi_present,
                       int mu_bins, double thin_tol, long cap, char *buf);
/* ndpp_lib.xml: print_ndpp_lib_xml_header / _nuclide / _closer ndpp.F90:958-1110
 * (directory = the reference's path_input; strings are trimmed like trim()) */
long ndpp_lib_xml_header(const char *directory, int lib_format, int n_listings, int nuscatter,
                         int chi_present, int scatt_type, int scatt_order, double print_tol,
                         double thin_tol, int mu_bins, int n_bins, const double *e_bins,
                         long cap, char *buf);
long ndpp_lib_xml_nuclide(const char *alias, double awr, const char *name, const char *path,
                          double kT, int zaid, int metastable, double freegas_cutoff,
                          int lib_format, long cap, char *buf);
long ndpp_lib_xml_closer(int lib_format, long cap, char *buf);

/* ---- one table from matrices to file: ndpp.F90:594-717 / :755-813 -------------------- */
typedef struct ndpp_output_options {   /* the run-level settings of nuclearDataPreProc */
  int lib_format;                      /* NDPP_FMT_ASCII or NDPP_FMT_BINARY             */
  int scatt_type, scatt_order;         /* as written to the header (order, not order+1) */
  int nuscatter, integrate_chi, mu_bins;
  double print_tol, thin_tol;
} ndpp_output_options;
/* apply_tol_scatt on every matrix, then (thin_tol > 0) thin_grid on the elastic grid and on
 * the inelastic grid with nu-inelastic riding along (ndpp.F90:611-646); in place, r->n_el /
 * r->n_inel shrink.  thin_report (NULL or 4 doubles): compression and max error, elastic
 * then inelastic.                                                                         */
int  ndpp_finish_scatt(const ndpp_output_options *o, ndpp_scatt_result *r, int n_bins,
                       const double *e_bins, double *thin_report);
/* The table's library file: header (init_library ndpp.F90:1246), scatter section
 * (print_scatt, group indices ndpp.F90:648-679), chi section when integrate_chi and
 * n_chi > 0 (print_chi); is_sab: 0 a neutron table; 1 a thermal table (nuscatter flag written
 * as 0, no chi), refused with scatt_type tabular; 2 a thermal table whose matrix may be tabular
 * (ndpp_sab_tab_batch): the header is the one is_sab = 1 writes, with scatt_type and scatt_order
 * as the options give them.                                                               */
long ndpp_nuclide_file(const ndpp_output_options *o, const char *name, int name_len, double kT,
                       int is_sab, const ndpp_scatt_result *r, int n_bins, const double *e_bins,
                       int n_chi, int n_prec, const double *e_chi, const double *chi_t,
                       const double *chi_p, const double *chi_d, long cap, unsigned char *buf);

/* ---- thinning: replaces `thin_grid(xout, yout, tokeep, tol, compression, maxerr[, yout2
 * [, yout3]])` thin.F90:17-501, host only, in place: x[n] and the matrices y[n][G][L]
 * (y2 of the same shape and the 1-D y3[n] optional, NULL when absent) keep their first
 * *n_out entries.  tokeep[n_keep]: abscissae never removed (the group edges).              */
int ndpp_thin_grid(int n, double *x, int L, int G, double *y, double *y2, double *y3, int n_keep,
                   const double *tokeep, double tol, int *n_out, double *compression,
                   double *maxerr);

/* Replaces `sab_egrid(sab, energy_bins, Ein)` sab.F90:460-568 (host only; the caller then
 * appends the extra top point, scatt.F90:426) and the union grid of calc_chi, chi.F90:97-113.
 * Counts are always returned, arrays written when cap suffices.                             */
int ndpp_sab_egrid(const ndpp_params *p, const ndpp_sab_flat *t, int n_bins, const double *e_bins,
                   int cap, double *ein, int *n_out);
int ndpp_chi_egrid(int n_prompt, const ndpp_chi_spectrum *prompt, int n_delay,
                   const ndpp_chi_spectrum *delay, int cap, double *e_grid, int *n_out);

/* ---- epilogue: replaces `apply_tol_scatt(data, tol)` scatt.F90:786-818, in place
 * on data[n][G][L]: groups whose P0 lies in (0, tol) are zeroed and every row is
 * renormalised to its original sum_g P0.  Bit-identical to the Fortran.        */
int ndpp_apply_tol_scatt(int L, int G, int n, double *data, double tol);

/* ---- library validation: the truncated Legendre expansion of stored moments
 *   f(mu_j) = sum_{l < n_moments} (l + 1/2) P_l(mu_j) a_l
 * on a caller's mu grid (Python passes numpy.linspace(-1, 1, M), the reference's grid).
 * P_l are the closed forms of calc_pn (legendre.F90:349-432); every f(mu_j) is computed by
 * one fixed operation sequence, so results repeat bit for bit and the two entry points agree.
 * mat / moments keep the Legendre index fastest, row stride L; n_moments <= L truncates
 * the sum (the reference's `order` argument).  Arguments are checked before the device is
 * touched (NDPP_EINVAL: L outside 1..NDPP_MAX_ORDER, n_moments outside 1..L, n_mu < 1, a mu
 * that is not finite or outside [-1, 1], a NULL pointer, cap < 0, sizes whose bytes
 * overflow); without a device NDPP_EDEVICE. n_ein = 0 is an empty, successful call.       */
typedef struct ndpp_positivity {
  long   rows;              /* (E_in, group) rows examined                                  */
  long   negative;          /* rows with some mu_j where !(f >= 0)  (NaN counts as negative) */
  double min_value;         /* smallest non-NaN f seen; 0.0 for an all-zero E_in; +inf if none */
  int    min_ein, min_group;/* 0-based, first row in (iE, g) order attaining min_value
                               (min_group -1: an all-zero E_in; both -1 if no row)           */
} ndpp_positivity;
/* Replaces test_scatt_positivity, src/utils/ndpp_data.py:345-396, for one matrix section
 * mat[n_ein][G][L].  Rows: for each E_in the groups gmin..gmax, the first and last with
 * P0 > 0 (the writer's rule, scatt.F90:1181-1198, so a read-back file's own gmin/gmax);
 * interior rows with P0 <= 0 are checked.  An E_in without P0 > 0 is one zero row: counted,
 * value 0.0, never negative.  A row is negative when !(f >= 0) at some mu_j.  The offending
 * rows come out in (iE, g) order: the first `cap` of them in neg_rows[k] = {iE, g} (0-based;
 * the reference reports g + gmin, a double-counted offset), with the row's smallest non-NaN f
 * (NaN if every f is NaN) in neg_min[k] and its first mu index in neg_mu[k] (both optional).
 * summary->negative may exceed cap.                                                       */
int ndpp_scatt_positivity(int n_ein, int G, int L, const double *mat, int n_moments,
                          int n_mu, const double *mu, long cap, int *neg_rows /* [cap][2] */,
                          double *neg_min /* [cap] or NULL */, int *neg_mu /* [cap] or NULL */,
                          ndpp_positivity *summary);
/* Replaces expand_scatt, src/utils/ndpp_data.py:305-343: out[n_ein][n_mu] = f of the rows
 * moments[n_ein][L] (one group's, or condensed, moments per E_in).                        */
int ndpp_expand_moments(int n_ein, int L, const double *moments, int n_moments,
                        int n_mu, const double *mu, double *out /* [n_ein][n_mu] */);

/* ---- certified positivity.  Replaces nothing: test_scatt_positivity and
 * ndpp_scatt_positivity sample f on a grid, and a dip between two grid points passes.  Here every
 * examined row gets an enclosure  lo <= min over [-1, 1] of f <= hi  of
 *   f(mu) = sum_{l < n_moments} c_l P_l(mu),   c_l = (l + 1/2) a_l,
 * with hi = f(mu_at) an attained value.  With
 *   S  = sum |c_l|                                     (|f| <= S on [-1, 1])
 *   M2 = sum_{l >= 2} |c_l| (l-1) l (l+1) (l+2) / 8    (|f''| <= M2: |P_l''| is largest at the ends)
 *   E  = 256 * DBL_EPSILON * S                          (the evaluation allowance)
 * the enclosure rests on  f >= min(f(a), f(a+h)) - M2 h^2 / 8  on [a, a+h]  (f minus its chord is
 * f''(xi) (mu-a)(mu-a-h) / 2).
 * Rows: exactly those ndpp_scatt_positivity examines -- per E_in the groups gmin..gmax, the first and
 * last with P0 > 0, interior rows with P0 <= 0 included.  An E_in without P0 > 0 is one row, held at
 * group 0 of the arrays: lo = hi = mu_at = 0, class positive, named as group -1 in the summary.  An
 * entry outside the band gets cls = -1, lo = hi = mu_at = 0.
 * Search: f at the 65 nodes of 64 equal panels gives the first hi.  An interval is DISCARDED when
 *   (min(f(a), f(a+h)) - hi) + rel_tol S >= M2 h^2 / 8
 * (its bound is within rel_tol S of hi; arranged so that a tiny M2 h^2 / 8 is not absorbed by the
 * subtraction); otherwise its midpoint is evaluated, hi and mu_at follow a smaller value, and both
 * halves are examined, at most 45 levels below the panels, where an interval is discarded with
 * whatever bound it has.  lo = min(smallest discarded bound, hi) - E: a lower bound of the exact
 * polynomial of the stored doubles.  A row is SETTLED when every interval was discarded by the rule;
 * then hi - lo <= rel_tol S + E (to the rounding of that expression).  A row makes at most
 * NDPP_MIN_MAX_EVALS evaluations of f, the nodes (read twice) and re-evaluated interval ends counted;
 * a row that runs into the cap or into the depth limit returns the valid, wider enclosure it has,
 * with NDPP_MIN_UNSETTLED set.  No loop on the device depends on convergence alone.
 * cls: -1 not examined; else the class in the low two bits -- NDPP_MIN_POSITIVE lo >= 0;
 * NDPP_MIN_NEGATIVE hi < 0 (mu_at is a witness); NDPP_MIN_UNDECIDED lo < 0 <= hi (the minimum is
 * within the tolerance of zero); NDPP_MIN_NONFINITE a NaN or an infinity among the row's n_moments
 * moments (or an S or M2 that overflows): lo = hi = NaN, mu_at = 0, never passes -- plus the bit
 * NDPP_MIN_UNSETTLED.  rel_tol = 0 is legal: rows with M2 = 0 (constant or linear f) settle at once,
 * the rest come back unsettled.
 * Arithmetic: P_0 = 1, P_1 = mu, P_{l+1} = (((2l+1) mu) P_l - l P_{l-1}) / (l+1); f = c_0, then
 * f = f + c_l P_l in ascending l; only + - * / and comparisons, without contraction, in every build:
 * two calls on the same input return the same bits.  The summary is folded on the host from the
 * dense arrays in (iE, g) order.
 * NDPP_EINVAL, decided before the device is touched: L outside 1..NDPP_MAX_ORDER, n_moments outside
 * 1..L, G < 1, n_ein < 0, rel_tol negative, NaN or infinite, a NULL pointer, sizes whose bytes
 * overflow.  n_ein = 0 is an empty, successful call.  Without a device NDPP_EDEVICE.              */
#define NDPP_MIN_MAX_EVALS 16384
#define NDPP_MIN_POSITIVE  0
#define NDPP_MIN_UNDECIDED 1
#define NDPP_MIN_NEGATIVE  2
#define NDPP_MIN_NONFINITE 3
#define NDPP_MIN_UNSETTLED 4
typedef struct ndpp_minimum {
  long   rows, negative, undecided, nonfinite, unsettled;
  double min_hi, min_mu;      /* smallest hi over examined finite rows, and its cosine; +inf / 0 if none */
  int    min_ein, min_group;  /* first row in (iE, g) order attaining it; all-zero E_in: group -1; none: -1, -1 */
} ndpp_minimum;
int ndpp_scatt_minimum(int n_ein, int G, int L, const double *mat /* [n_ein][G][L] */, int n_moments,
                       double rel_tol, double *lo, double *hi, double *mu_at, int *cls /* each [n_ein][G] */,
                       ndpp_minimum *summary);
/* the same call, which also returns the evaluations of f each row made (0 where none was needed):
 * for measurements (tools/bench_minimum.py) and for the test of the cap.  NULL evals: NDPP_EINVAL. */
int ndpp_scatt_minimum_evals(int n_ein, int G, int L, const double *mat, int n_moments, double rel_tol,
                             double *lo, double *hi, double *mu_at, int *cls, int *evals /* [n_ein][G] */,
                             ndpp_minimum *summary);

/* ---- repair of negative rows, certified positive.  Replaces nothing: the
 * reference never repairs a row.  A row has stored moments a_0 .. a_{L-1} and
 * f(mu) = sum (l + 1/2) a_l P_l(mu).  The repaired row is a_l * w_l(t) with one parameter t in [0, 1],
 * in one of two families:
 *   heat     w_l = t^(l(l+1)/2): the heat kernel on the sphere, e^(-tau l(l+1)) with t = e^(-2 tau), a
 *            non-negative smoothing kernel; it damps what truncation produced (high orders) far more
 *            than P1;
 *   uniform  w_0 = 1, w_l = t for l >= 1: the blend towards the isotropic row with the same P0.
 * In both w_0 = 1 (P0 is untouched bit for bit, hence the band gmin..gmax, sum_g P0, print_tol and
 * condensation), P1 is kept to exactly the fraction t, t = 1 is the identity and t = 0 gives
 * f = a_0 / 2, positive when a_0 > 0: a passing t always exists.
 * Weights, by multiplications only and in this order (host and device give the same bits; no exp or
 * pow on the device): heat  p = t; w_1 = t; for l = 2 .. L-1: p = p * t; w_l = w_{l-1} * p;  uniform
 * w_l = t;  repaired moment a_l * w_l (a_0 itself for l = 0).
 * Search: bisection on t with exactly `steps` trips (1..52).  Invariant: t_pass (initially 0) passes
 * and t_fail (initially 1) fails; each trip tests the exact dyadic midpoint and moves one end; the
 * result is t_pass.  A value t PASSES when ndpp_scatt_minimum's search of one row, at rel_tol and
 * n_moments = L, classes the row a_l * w_l(t) NDPP_MIN_POSITIVE (NDPP_MIN_UNSETTLED may be set: lo >= 0
 * is valid either way); NDPP_MIN_UNDECIDED counts as failing.  Positivity is not assumed monotone in t:
 * the invariant alone makes the result certified, and t + 2^-steps is a value that was seen to fail.
 * No loop depends on convergence: at most steps trips, each bounded by NDPP_MIN_MAX_EVALS.
 * mode: NDPP_REPAIR_HEAT, NDPP_REPAIR_UNIFORM, or NDPP_REPAIR_BEST: both searches, the one with the
 * larger t is kept, uniform on a tie (when t_uniform >= t_heat the uniform row keeps at least as much
 * of every moment as the heat row; otherwise heat keeps more of P1).
 * Rows: those ndpp_scatt_minimum examines at n_moments = L -- per E_in the groups gmin..gmax, the first
 * and last with P0 > 0, interior rows included.  A row whose class at t = 1 is NEGATIVE is repaired;
 * an UNDECIDED one only when undecided != 0.  Of these, a row with a_0 == 0 becomes the zero row
 * (t = 0, no search) and a row with a_0 < 0 is UNREPAIRABLE: copied unchanged and counted.  A
 * non-finite row is copied unchanged and counted.  Everything else, entries outside the band
 * included, is copied bit for bit.
 * how: -1 not examined, 0 untouched, 1 heat, 2 uniform, 3 unrepairable, 4 non-finite.  t: the
 * parameter of a repaired row, 1.0 where untouched (how 0, 3, 4), -1.0 where not examined.
 * The classes are found on the device with the matrix kept there; the rows to repair are listed on
 * the host in (iE, g) order, and the summary is folded there in that order.  ndpp_last_gpu_ms()
 * after the call is the time of the repair kernel (of the classification when no row was listed).
 * NDPP_EINVAL, decided before the device is touched: L outside 1..NDPP_MAX_ORDER, G < 1, n_ein < 0,
 * an unknown mode, steps outside 1..52, rel_tol negative, NaN or infinite, a NULL pointer, sizes
 * whose bytes overflow.  n_ein = 0 is an empty, successful call.  Without a device NDPP_EDEVICE.    */
#define NDPP_REPAIR_BEST    0
#define NDPP_REPAIR_HEAT    1
#define NDPP_REPAIR_UNIFORM 2
typedef struct ndpp_repair {
  long   rows, repaired, heat, uniform, unrepairable, nonfinite;  /* rows: examined; repaired = heat + uniform */
  double min_t;               /* smallest t over the repaired rows; 1.0 if none */
  int    min_ein, min_group;  /* first row in (iE, g) order attaining it; none: -1, -1 */
} ndpp_repair;
int ndpp_scatt_repair(int n_ein, int G, int L, const double *mat /* [n_ein][G][L] */, int mode, int steps,
                      int undecided, double rel_tol, double *out /* [n_ein][G][L] */,
                      double *t /* [n_ein][G] */, int *how /* [n_ein][G] */, ndpp_repair *summary);
/* the same call, which also returns the evaluations of f each repaired row made in its searches (0
 * elsewhere): for measurements (tools/bench_repair.py).  NULL evals: NDPP_EINVAL.                 */
int ndpp_scatt_repair_evals(int n_ein, int G, int L, const double *mat, int mode, int steps, int undecided,
                            double rel_tol, double *out, double *t, int *how, int *evals /* [n_ein][G] */,
                            ndpp_repair *summary);

/* ---- interpolation error of an incoming-energy grid.  Replaces nothing: the reference never
 * measures it (thin_grid compares stored rows with each other, never with a fresh one).
 * x[n] with rows y[n][G][L]; x_mid[n-1] with rows y_mid[n-1][G][L] integrated there.  For
 * interval i, with f = ln(x_mid[i] / x[i]) / ln(x[i+1] / x[i]) (thin_grid's rule, thin.F90):
 *   err[i] = max over (g,l) of | y[i] + (y[i+1] - y[i]) f - y_mid[i] | / scale_i,
 *   scale_i = max over g of |P0| (l = 0) in the rows y[i], y[i+1], y_mid[i];
 * err[i] = 0 when scale_i is 0.  arg[i] = g * L + l of the maximum, the lowest on a tie.
 * An interval with x[i+1] <= x[i], with x_mid[i] outside (x[i], x[i+1]), or with an abscissa
 * that is not positive and finite is skipped: err = -1, arg = -1.  A NaN or an infinity in the
 * three rows (or produced by them) gives err = +inf and arg = the first such element.
 * f comes from the host's log, the rest is + - * / and comparisons in that order without
 * contraction, on the device: a host restatement reproduces err and arg bit for bit.
 * NDPP_EINVAL: L < 1, G < 1, n < 2, a NULL pointer -- decided before the device is touched.   */
int ndpp_grid_error(int L, int G, int n, const double *x, const double *y /* [n][G][L] */,
                    const double *x_mid /* [n-1] */, const double *y_mid /* [n-1][G][L] */,
                    double *err /* [n-1] */, int *arg /* [n-1] */);

/* ---- error-bounded thinning of an incoming-energy grid.  Replaces nothing:
 * thin_grid (above) tests a point against the last kept point and its right neighbour only, under
 * an element-wise relative metric, so its tolerance bounds nothing.  Here every candidate segment is
 * measured.  x[n] strictly increasing, positive and finite; rows y[n][G][L] and, on the same grid,
 * y2[n][G][L] or NULL (inelastic with nu-inelastic riding along).  With
 *   lx[i] = log(x[i])                    (the host's log, once per point)
 *   s[i]  = max over g of |y[i][g][0]|   (s2 alike for y2)
 * and, for a < k < b,
 *   f          = (lx[k] - lx[a]) / (lx[b] - lx[a])
 *   d(a,k,b)   = max over elements e of | y[a][e] + (y[b][e] - y[a][e]) * f - y[k][e] |
 *   err(a,k,b) = d / max(s[a], s[k], s[b])    (0 when that scale is 0; +inf when an element
 *                involved, or the value they produce, is a NaN or an infinity; with y2 the larger
 *                of the two sections' values, each over its own scale)
 * the result is, for d = 2..window,
 *   seg_err[a][d-2] = max over a < k < a+d of err(a, k, a+d)
 *                     -1 when a + d > n - 1; +inf when some k strictly inside is a must-keep point
 *                     (x[k] equal to one of tokeep[n_keep]).
 * Only + - * / fabs and comparisons run on the device, in the order written, without contraction: a
 * host restatement reproduces seg_err bit for bit (ndpp_amd/thin.py: segment_errors_numpy).
 * NDPP_EINVAL, decided before the device is touched: L or G < 1, n < 2, window outside 2..64, a NULL
 * pointer (tokeep may be NULL when n_keep is 0), n_keep < 0, x not strictly increasing, positive and
 * finite, sizes whose bytes overflow.  Without a device NDPP_EDEVICE.                              */
int ndpp_thin_segments(int L, int G, int n, const double *x, const double *y /* [n][G][L] */,
                       const double *y2 /* [n][G][L] or NULL */, int n_keep, const double *tokeep,
                       int window, double *seg_err /* [n][window-1] */);
/* ndpp_thin_segments plus the chain over it.  A segment (a, a+d) is admissible when
 * 0 <= seg_err[a][d-2] <= tol; (a, a+1) always is.  reach[a] is the largest admissible a+d within
 * the window; the kept points are 0 -> reach[0] -> reach[reach[0]] -> ... -> n-1.  kept[0..*n_kept)
 * receives their indices in increasing order (no data moves: the caller gathers rows by them) and
 * *max_err the largest seg_err along the chain: every dropped point is within it, and so within tol,
 * of the interpolation between its two kept neighbours.  Also NDPP_EINVAL: tol not finite or < 0.
 * n = 2: both points kept, *max_err = 0.                                                          */
int ndpp_thin_bounded(int L, int G, int n, const double *x, const double *y, const double *y2,
                      int n_keep, const double *tokeep, double tol, int window,
                      int *kept /* [n] */, int *n_kept, double *max_err);

/* ---- distance between two sections on different incoming-energy grids.
 * Replaces nothing: the reference never compares two libraries.  Section A: xa[na] with rows
 * ya[na][G][La]; section B: xb[nb] with rows yb[nb][G][Lb]; the same G outgoing groups, and the
 * first Lc = min(La, Lb) entries of every group are compared (a P5 library against a P10 one).  Both
 * grids strictly increasing, positive and finite.  A consumer reads a section linearly in ln E
 * (thin_grid's rule): for a query x = xq[q] inside both grids' ranges, with i the largest index with
 * xa[i] <= x and i1 = min(i + 1, na - 1),
 *   fa   = ln(x / xa[i]) / ln(xa[i+1] / xa[i])      (0 when x == xa[i]; the host's log)
 *   A(x) = ya[i] + (ya[i1] - ya[i]) * fa
 * and B(x) alike with j, j1 and fb.  Then, for e = (g, l), g < G, l < Lc,
 *   d_e    = | A(x)_e - B(x)_e |
 *   scale  = max over g of |P0| (l = 0) in the rows ya[i], ya[i1], yb[j], yb[j1]
 *   err[q] = max over e of d_e / scale               (0 when scale is 0)
 *   arg[q] = g * Lc + l of the maximum, the lowest on a tie.
 * A NaN or an infinity in an element involved, or in what it produces, gives err[q] = +inf and
 * arg[q] = the lowest such e.  A query that is not positive and finite, or outside the range of
 * either grid, is skipped: err = -1, arg = -1.  worst[g][l] (optional) = the maximum of d_e / scale
 * over the queries that were not skipped: +inf if any of them gave a NaN or an infinity for that
 * element, -1 if every query was skipped.
 * Between two neighbouring points u, u' of the union of xa and xb both interpolants are linear in
 * ln x and the scale is constant on [u, u'), so the supremum of err there is err(u) or the limit of
 * err from below u' (the scale jumps at u', where a grid moves on to its next rows): queried at the
 * union points and at the largest double below each (ndpp_amd/compare.py: union_queries), max err
 * is the distance of the two sections, not a sample of it.
 * i, fa, j, fb come from the host; + - * / fabs and comparisons run on the device in the order
 * written, without contraction: a host restatement reproduces err, arg and worst bit for bit
 * (ndpp_amd/compare.py: compare_numpy).
 * NDPP_EINVAL, decided before the device is touched: G, La or Lb < 1, na or nb < 2, nq < 1, a NULL
 * pointer (worst may be NULL), a grid that is not strictly increasing, positive and finite, a
 * G * max(La, Lb) that does not fit an index.  Without a device NDPP_EDEVICE.                      */
int ndpp_lib_compare(int G, int La, int Lb,
                     int na, const double *xa, const double *ya /* [na][G][La] */,
                     int nb, const double *xb, const double *yb /* [nb][G][Lb] */,
                     int nq, const double *xq,
                     double *err /* [nq] */, int *arg /* [nq] */,
                     double *worst /* [G][min(La,Lb)], may be NULL */);

/* ---- sample an outgoing group and a scattering cosine from a section.
 * Replaces nothing: the reference writes libraries and never reads a row the way a transport code
 * does.  The section: x[n] strictly increasing, positive and finite, with the dense rows y[n][G][L] as
 * ndpp_amd/reader.py's ScattSection.mat holds them; scatt_type NDPP_SCATT_LEGENDRE: L Legendre
 * moments per group, 1 <= L <= NDPP_MAX_ORDER; NDPP_SCATT_TABULAR: L = N equal cosine bins per group,
 * 1 <= N <= NDPP_MAX_TAB_BINS.  Event e has the incoming energy ein[e] and two uniform numbers
 * u_g[e], u_mu[e] in [0, 1).  Every sum below starts from 0.0 and runs sequentially in ascending
 * index; "blend(v0, v1) = v0 + (v1 - v0) * f".
 * 1. Bracket (ndpp_lib_compare's rule and host code): i the largest index with x[i] <= ein,
 *    i1 = min(i + 1, n - 1), f = ln(ein / x[i]) / ln(x[i1] / x[i]) with the host's log, f = 0 when
 *    ein == x[i] (and at the last point).  An ein that is not positive and finite or lies outside
 *    [x[0], x[n-1]], or a u_g or u_mu outside [0, 1) (a NaN included): status NDPP_SAMPLE_SKIPPED,
 *    group -1, mu 0.
 * 2. Group.  The mass of group g in the stored row r: s_r[g] = y[r][g][0] (Legendre), the sum over k
 *    of y[r][g][k] (tabular).  w_g = blend(s_i[g], s_i1[g]), W = sum over g of w_g.  A w_g that is
 *    negative or not finite, or a W that is not finite: NDPP_SAMPLE_BADROW, group -1, mu 0.
 *    W == 0: NDPP_SAMPLE_ZEROROW, group -1, mu 0.  Otherwise group is the smallest g whose running
 *    sum w_0 + ... + w_g exceeds u_g * W; if rounding leaves none, the last g with w_g > 0.  A group
 *    with w_g = 0 is never drawn.
 * 3. Cosine, tabular.  t_k = blend(y[i][g][k], y[i1][g][k]); a negative or non-finite t_k, or a sum
 *    T of the t_k that is not finite: BADROW, group -1, mu 0; T == 0 (underflow only): ZEROROW alike.
 *    target = u_mu * T; k is the smallest bin whose running sum c_k = t_0 + ... + t_k exceeds target,
 *    else the last k with t_k > 0: a bin with t_k = 0 is never drawn.  With h = 2.0 / N,
 *      mu = -1.0 + h * (k + (target - c_{k-1}) / t_k)            (c_{-1} = 0)
 *    clamped to the bin [-1.0 + h * k, -1.0 + h * (k + 1)], whose right end is 1.0 for k = N - 1.
 * 4. Cosine, Legendre.  a_l = blend(y[i][g][l], y[i1][g][l]), l < L; an a_l that is not finite:
 *    BADROW, group -1, mu 0 (a_0 = w_g > 0 here).  The row's density is sum_l (l + 1/2) a_l P_l(mu),
 *    its integral from -1
 *      F(mu) = (0.5 * a_0) * (mu + 1.0) + sum over l = 1 .. L-1 of (0.5 * a_l) * (P_{l+1}(mu) - P_{l-1}(mu))
 *    with F(1) = a_0, accumulated in ascending l, P by Bonnet's recurrence upwards in the order
 *      P_0 = 1.0, P_1 = mu, P_{l+1} = (A_l * mu) * P_l - B_l * P_{l-1},
 *      A_l = (double)(2 l + 1) / (double)(l + 1), B_l = (double)l / (double)(l + 1).
 *    target = u_mu * a_0; lo = -1.0, hi = 1.0; 53 times: m = 0.5 * (lo + hi); if F(m) < target then
 *    lo = m, else hi = m; mu = 0.5 * (lo + hi).  No moment problem is solved and nothing is assumed of
 *    the row: on a positive row F is increasing and mu is the inverse of the CDF to the last bit of
 *    the interval.  The density d = sum in ascending l (from 0.0) of ((l + 0.5) * a_l) * P_l(mu) is
 *    evaluated once at the end: !(d >= 0) gives NDPP_SAMPLE_NEGDENSITY, with the group and the cosine
 *    still returned -- such a row is not a distribution, and wants --repair-positivity
 *    (ndpp_scatt_repair) before it is sampled.  The status is no positivity check: the bisection keeps
 *    F(lo) < target <= F(hi) and so ends where F crosses the target upwards, where d is not negative;
 *    a row with a dip inside (-1, 1) is sampled without a flag, and only a d that does not evaluate
 *    (inf - inf) is caught.  ndpp_scatt_minimum decides whether a row is positive.
 * 5. Otherwise status NDPP_SAMPLE_OK.
 * i and f come from the host; + - * / and comparisons run on the device in the order written,
 * without contraction: a host restatement reproduces group, mu and status bit for bit
 * (ndpp_amd/sample.py: sample_numpy).
 * NDPP_EINVAL, decided before the device is touched: a scatt_type other than 0 or 1, G < 1, L outside
 * its range, n < 2, n_ev < 0, a NULL pointer, a grid that is not strictly increasing, positive and
 * finite, sizes whose bytes overflow.  Without a device NDPP_EDEVICE; with one, n_ev == 0 is an empty
 * success.                                                                                          */
/* step 1 alone, the host half of ndpp_scatt_sample (which calls it): row[e] = i and weight[e] = f, or
 * row[e] = -1 and weight[e] = 0 for an event that is skipped.  Needs no device.  For measurements
 * (tools/bench_sample.py) and for a host that wants the brackets of its events.  NDPP_EINVAL: n < 2,
 * n_ev < 0, a NULL pointer, a bad grid.                                                            */
int ndpp_sample_brackets(int n, const double *x, long n_ev, const double *ein, const double *u_g,
                         const double *u_mu, int *row /* [n_ev] */, double *weight /* [n_ev] */);
int ndpp_scatt_sample(int scatt_type, int G, int L,
                      int n, const double *x, const double *y /* [n][G][L] */,
                      long n_ev, const double *ein, const double *u_g, const double *u_mu,
                      int *group /* [n_ev] */, double *mu /* [n_ev] */, int *status /* [n_ev] */);

/* ---- score collision events into group-to-group tallies: the expected-value
 * consumer.  Replaces nothing in the reference.  At every event the whole row [G][L] of the section at
 * the event's energy, times the event's factor, is added to the tally bin the caller names.  The
 * entry point is elementwise over a row: it serves L Legendre moments and L = N cosine bins alike,
 * knows nothing of cross sections or spectra and claims no multigroup constants.  The section is that
 * of ndpp_scatt_sample: x[n] strictly increasing, positive and finite, y[n][G][L] dense.  Event e has
 * the incoming energy ein[e], the weight weight[e] and the tally bin bin[e].
 * scatt_type is read only with normalize = 1, where a group's mass needs its rule: NDPP_SCATT_LEGENDRE
 * (1 <= L <= NDPP_MAX_ORDER) or NDPP_SCATT_TABULAR (1 <= L <= NDPP_MAX_TAB_BINS).  With normalize = 0
 * it is ignored and 1 <= L <= NDPP_MAX_TAB_BINS.
 * 1. Bracket, on the host, as step 1 of ndpp_scatt_sample: i the largest index with x[i] <= ein,
 *    i1 = min(i + 1, n - 1), f = ln(ein / x[i]) / ln(x[i1] / x[i]) with the host's log, f = 0 when
 *    ein == x[i] (and at the last point).  NDPP_SCORE_SKIPPED: an ein that is not positive and finite
 *    or lies outside [x[0], x[n-1]], a weight that is not finite, a bin outside [0, n_bins).  A weight
 *    of zero or below zero is scored.
 * 2. Factor.  normalize = 0: v = weight.  normalize = 1: v = weight / W with W and the w_g of step 2 of
 *    ndpp_scatt_sample, the same operations in the same order: s_r[g] = y[r][g][0] (Legendre) or the
 *    sum over k from 0.0 of y[r][g][k] (tabular), w_g = s_i[g] + (s_i1[g] - s_i[g]) * f, W the sum over
 *    g from 0.0.  A w_g that is negative or not finite, or a W that is not finite:
 *    NDPP_SCORE_BADROW; W == 0: NDPP_SCORE_ZEROROW.  Such events contribute nothing and are not
 *    counted.  Every other event is scored, NDPP_SCORE_OK.
 * 3. Contribution.  c[e] = v * (y[i][e] + (y[i1][e] - y[i][e]) * f) for every element e < G * L, in
 *    the order written, without contraction.  Stored values that are not finite are not tested: they
 *    go into the tally by IEEE rules.
 * 4. Sum order.  The scored events of a tally bin, in ascending event index, are cut into chunks of
 *    NDPP_SCORE_CHUNK events.  A chunk's partial is the sequential sum of its contributions from 0.0
 *    in ascending event order; tally[b][e] is the sequential sum of the partials of bin b from 0.0 in
 *    ascending chunk order; wsum[b] is the sum of the bin's v in the same chunked order; count[b] is
 *    the number of scored events.  A bin without scored events is all 0.0.  No atomics: the same
 *    events give the same bits on every run, and a host restatement reproduces them
 *    (ndpp_amd/score.py: score_numpy).
 * An element whose two stored values are both exactly 0.0 contributes +-0.0 whatever the finite
 * factor, and adding that to a sum that started at +0.0 changes no bit.  The device therefore reads,
 * per event, only the groups from the first to the last with ANY element that is not exactly 0.0 in
 * either stored row (a NaN counts as not zero), and every group when v is not finite.  This is not
 * the P0 > 0 band of the norms.  The partial sums are held in a device buffer of
 * NDPP_SCORE_PARTIAL_MB megabytes (environment, read once per call, default 256) and taken in passes
 * over ascending chunk ranges; the result does not depend on it.  NDPP_SCORE_BAND=0 (environment)
 * makes the device read every group of every event, for measurements of what the skip saves; it
 * changes no bit either, is a measurement hook only and not a stable part of the interface.
 * NDPP_EINVAL, decided before the device is touched: normalize not 0 or 1, with normalize = 1 a
 * scatt_type other than 0 or 1, G < 1, L outside its range, n < 2, n_ev < 0, n_bins < 1, a NULL
 * pointer, a grid that is not strictly increasing, positive and finite, a G * L that does not fit
 * an index, sizes whose bytes overflow.  Without a device NDPP_EDEVICE; with one, n_ev == 0 is an
 * empty success with zeroed outputs.                                                               */
int ndpp_scatt_score(int normalize, int scatt_type, int G, int L,
                     int n, const double *x, const double *y /* [n][G][L] */,
                     long n_ev, const double *ein, const double *weight, const int *bin, int n_bins,
                     double *tally /* [n_bins][G][L] */, double *wsum /* [n_bins] */,
                     long *count /* [n_bins] */, int *status /* [n_ev] */);
/* out[k], k < n: the NDPP_SCORE_INFO_* figures of the calling thread's last ndpp_scatt_score that
 * reached the device (0 beyond NDPP_SCORE_INFO_LEN).  Measurement only (tools/bench_score.py, the
 * test of the passes), not a stable part of the ABI: see the constants above.                       */
int ndpp_scatt_score_info(double *out, int n);

/* ---- ACE law 66: N-body phase space, in closed form -----------------------
 * The reference leaves a reaction whose energy distribution is law 66 uninitialised
 * (scattdata_header.F90:105-109): it adds nothing to a library.  ndpp_nbody_leg_batch integrates it.
 * There is no table and nothing is interpolated in E_in: the density is closed-form at every
 * incoming energy.
 *   out[e][g][l], l < L = p->order: the moment of order l of group [lo, hi] = e_bins[g], e_bins[g+1]
 *     at E = ein[e], fully written, not scaled by a cross section or p_valid (as ndpp_file6_leg_batch)
 *   status[e]: NDPP_ST_RANGE and a zero row for an E that is not positive and finite (as the other
 *     batch calls); NDPP_ST_NONFINITE as everywhere.  May be NULL.
 * With A = awr, Q the reaction's Q value, n = n_bodies in 3..5 and Ap > 1 (the two LDAT words):
 *   Emax = ((Ap - 1) / Ap) * ((A / (A + 1)) * E + Q),   E0 = E / ((A + 1) * (A + 1)).
 * Emax <= 0: the row is zero.  In the centre of mass the neutron energy T has the density
 * x^(1/2) (1 - x)^(3n/2 - 4) / B(3/2, 3n/2 - 3), x = T / Emax, the direction is isotropic, and the lab
 * energy is E' = T + E0 + 2 muc sqrt(T E0).  A group that misses the lab window -- hi <= wl * wl or
 * lo >= wh * wh, wl = max(sqrt(E0) - sqrt(Emax), 0), wh = sqrt(Emax) + sqrt(E0) -- is zero without
 * integrating.  Otherwise, in IEEE double, one operation per written operator, no contraction, x[k]
 * and w[k] (k = 0..31, ascending) the 32-point Gauss-Legendre rule of ndpp_nbody_rule:
 *   rE0 = sqrt(E0), rlo = sqrt(lo), rhi = sqrt(hi)
 *   breakpoints: for d in (rlo - rE0, rlo + rE0, rhi - rE0, rhi + rE0): Tb = d * d; kept when
 *     0 < Tb < Emax, as sg / (1 + sqrt(1 - sg * sg)), sg = sqrt(Tb / Emax).  The kept values, 0 and 1,
 *     sorted, equal values once: consecutive values pa < pb are the pieces, ascending.
 *   outer node j of a piece:
 *     hm = 0.5 * (pb - pa), cm = 0.5 * (pb + pa), t = cm + hm * x[j], wt = hm * w[j]
 *     q = 1 + t * t, s = (2 * t) / q, c = (1 - t * t) / q, s2 = s * s, T = Emax * s2
 *     c2 = c * c, c4 = c2 * c2, cp = c2 (n = 3), c4 * c (n = 4), c4 * c4 (n = 5)
 *     W = ((K * s2) * cp) * (2 / q), K = 2 / B: 16/pi, 105/8, 512/(7 pi) rounded once
 *     (T = Emax sin^2(theta), theta = 2 atan t: both end-point singularities are gone)
 *     rT = sqrt(T), ia = max(|rT - rE0|, rlo), ib = min(rT + rE0, rhi); I_l = 0.0, and unless ib > ia
 *     they stay so; else with hm2 = 0.5 * (ib - ia), cm2 = 0.5 * (ib + ia), den = (2 * rT) * rE0:
 *   inner node k, in s' = sqrt(E'):
 *     sp = cm2 + hm2 * x[k], fk = (hm2 * w[k]) * (sp / den)
 *     mu = ((sp - rT) * (sp + rT)) / ((2 * sp) * rE0) + rE0 / (2 * sp), clamped to [-1, 1]
 *     P_0 = 1, P_1 = mu, P_(l+1) = (((2l + 1) / (l + 1)) * mu) * P_l - (l / (l + 1)) * P_(l-1),
 *     the quotients rounded once (the recurrence of ndpp_scatt_sample)
 *     I_l = I_l + fk * P_l, k ascending
 *   v_l[j] = (wt * W) * I_l;  piece_l = v_l[0] + ... + v_l[31], from 0.0, j ascending;
 *   out[e][g][l] = the pieces, from 0.0, ascending.
 * The cut at the breakpoints is what makes the rule converge: the inner limits have kinks in T where
 * a group edge enters or leaves the kinematic window.  tests/nbody_ref.py restates the operations
 * (nbody_numpy gives the same bits) and measures the rule against finer ones; the figures are in
 * profiles/nbody/README.md.
 * NDPP_EINVAL, decided before the device is touched: p NULL, its order or mu_bins out of range, G < 1,
 * n_bodies outside 3..5, Ap not a finite number above 1, awr not finite and positive, Q not finite,
 * n_ein < 0; for n_ein > 0 a NULL array, a G * L that does not fit an index.  n_ein == 0 is an empty
 * success.  Without a device NDPP_EDEVICE.                                                          */
int ndpp_nbody_leg_batch(const ndpp_params *p, double awr, double Q, int n_bodies, double Ap,
                         int n_ein, const double *ein, int G, const double *e_bins,
                         double *out /* [n_ein][G][L] */, int *status /* [n_ein] */);
/* the nodes and weights the call uses (host only; for restatements) */
void ndpp_nbody_rule(double x[32], double w[32]);
/* Opt-in, process-wide, default 0; returns the previous value.  The whole-nuclide calls read it once
 * per nuclide.  With 1, a law-66 energy distribution of a scattering reaction (is_valid_scatter) is a
 * ScattData of its own: no angular distribution is fabricated for it, its grid is
 * {max(threshold energy, e_bins[0]), top edge} (none when that is not below the top edge), and its
 * rows come from ndpp_nbody_leg_batch, scaled and summed like any other reaction's.  A tabular call
 * that meets such a reaction returns NDPP_EINVAL ("law 66 has Legendre output only") unless
 * ndpp_set_nbody_tab is on as well (below).  With 0 nothing changes anywhere.  ndpp_scattdata_shape
 * and ndpp_convert_distro do not read it.                                                           */
int ndpp_set_nbody(int enable);
int ndpp_get_nbody(void);

/* ---- ACE law 66 in cosine bins ("Tabular output") ---------------------------
 * The tabular counterpart of ndpp_nbody_leg_batch: the P0 of a group split into n_tab = N equal bins of
 * the lab cosine, 1 <= N <= NDPP_MAX_TAB_BINS, with the edges of the other tabular calls
 * (b_k = -1 + (2 * k) / N, b_N = 1).
 *   out[e][g][k]: bin k of group [lo, hi] at E = ein[e], fully written, not scaled; never negative
 *   status[e]: as ndpp_nbody_leg_batch.  May be NULL.
 * The symbols are those of ndpp_nbody_leg_batch: A, Q, n, Ap, Emax, E0, rE0 = sqrt(E0), rEm =
 * sqrt(Emax), wl, wh, K = 2 / B, x[j], w[j]; p = 3n/2 - 3 (1.5, 3, 4.5).  In the lab variables
 * (s' = sqrt(E'), mu) the CM energy is T(m, s') = (s' * s' + E0) - 2 m s' rE0, the density is
 * proportional to s' * s' * y^(p-1) with y(m, s') = 1 - T / Emax where that is positive, and its
 * integral over the cosine from m0 to m1 at fixed s' is
 *   C * s' * (max(y(m1, s'), 0)^p - max(y(m0, s'), 0)^p),   C = K / (4 p rEm rE0):
 * a bin is a one-dimensional integral over s' and nothing else.  The difference of the two powers is
 * never formed: it is the product d * D below, each factor without cancellation, so a bin cannot come
 * out negative and a heavy target (E0 << Emax) loses no digits.
 * A row with an E that is not positive and finite (NDPP_ST_RANGE), or with Emax <= 0, is zero; so is
 * a group with hi <= wl * wl or lo >= wh * wh (the test of ndpp_nbody_leg_batch), without integrating.
 * Otherwise, in IEEE double, one operation per written operator, no contraction:
 *   rlo = sqrt(lo), rhi = sqrt(hi), a = max(rlo, wl), b = min(rhi, wh)   (x > y ? x : y, x < y ? x : y)
 *   m0 = b_k, m1 = b_(k+1), dm = m1 - m0
 *   for m in (m0, m1): c = m * rE0, disc = Emax - E0 * ((1 - m) * (1 + m)): Emax y(m, s') is
 *     disc - (s' - c)^2, and y is evaluated in this form (c0, disc0 and c1, disc1 below).  Just above
 *     the threshold Emax << E0, and 1 - T / Emax as written would lose log10(E0 / Emax) digits.
 *   breakpoints: for m in (m0, m1), when disc > 0: the two roots c - sqrt(disc), c + sqrt(disc) of
 *     y(m, s') = 0, each kept when a < root < b.  a, b and the kept roots, sorted, equal values once:
 *     consecutive values pa < pb are the pieces, at most five, ascending.  (b <= a: no piece.)
 *   node j of a piece, len = pb - pa:
 *     u = 0.5 + 0.5 * x[j], h = (u * u) * (3 - 2 * u), sp = pa + len * h
 *     wgt = ((0.5 * w[j]) * len) * ((6 * u) * (1 - u))
 *     (s' = pa + len h(u): at a root the integrand starts like (s' - root)^p, p = 3/2 for n = 3; in u
 *     it is smooth at both ends of the piece)
 *     t0 = sp - c0, t1 = sp - c1
 *     y0 = (disc0 - t0 * t0) / Emax,  y1 = (disc1 - t1 * t1) / Emax
 *     y0c = y0 > 0 ? y0 : 0,  y1c = y1 > 0 ? y1 : 0
 *     f = 0.0 unless y1c > 0; then
 *       d = (((2 * sp) * rE0) * dm) / Emax where y0 > 0 (this is y1 - y0 without the subtraction),
 *           y1c otherwise
 *       q2 = (y1c * y1c + y1c * y0c) + y0c * y0c
 *       D = (y1c^p - y0c^p) / (y1c - y0c), as
 *         n = 4: q2
 *         n = 3: q2 / (y1c * sqrt(y1c) + y0c * sqrt(y0c))
 *         n = 5: a3 = (y1c * y1c) * y1c, b3 = (y0c * y0c) * y0c,
 *                (q2 * ((a3 * a3 + a3 * b3) + b3 * b3)) / ((a3 * y1c) * sqrt(y1c) + (b3 * y0c) * sqrt(y0c))
 *       f = (sp * d) * D
 *     piece = piece + wgt * f, from 0.0, j ascending
 *   total = the pieces, from 0.0, ascending;  out[e][g][k] = (K / (((4 * p) * rEm) * rE0)) * total.
 * tests/nbody_tab_ref.py restates the operations (nbody_tab_numpy gives the same bits) and measures
 * the rule against a 96-point one, against the Legendre call's P0 and against an independent route
 * through the CM variables; the figures, and the known limit E0 << Emax for n = 3 (a very heavy target:
 * 7.5e-10 at A = 1e6 and N = 1), are in profiles/nbody_tab/README.md.
 * NDPP_EINVAL, decided before the device is touched: n_tab outside 1..NDPP_MAX_TAB_BINS, and the
 * argument checks of ndpp_nbody_leg_batch except the order, which tabular output does not read.
 * n_ein == 0 is an empty success.  Without a device NDPP_EDEVICE.                                    */
int ndpp_nbody_tab_batch(const ndpp_params *p, int n_tab, double awr, double Q, int n_bodies,
                         double Ap, int n_ein, const double *ein, int G, const double *e_bins,
                         double *out /* [n_ein][G][n_tab] */, int *status /* [n_ein] */);
/* Opt-in, process-wide, default 0; returns the previous value.  Read once per nuclide, next to
 * ndpp_get_nbody, and acts only when that is 1 as well: a tabular whole-nuclide call then initialises
 * a law-66 reaction as a Legendre call does and takes its rows from ndpp_nbody_tab_batch.  With 0 the
 * tabular call refuses as before.                                                                    */
int ndpp_set_nbody_tab(int enable);
int ndpp_get_nbody_tab(void);

/* ---- derive a library from a finished one: coarser outgoing groups, cosine
 * bins from Legendre moments, moments and their enclosure from bins.  Replaces nothing in the
 * reference.  The arguments are host arrays; rows are independent, so a caller may cut a section into
 * slices of whole energies without changing a bit.  Every sum below starts from 0.0 and runs
 * sequentially in ascending index, one IEEE operation per written operator, without contraction in
 * every build: a host restatement from the tables of ndpp_derive_tables reproduces every output and
 * every status bit for bit (ndpp_amd/derive.py: groups_numpy, bins_numpy, moments_numpy).
 *
 * Status bits of a row (ndpp_derive_bins, ndpp_derive_moments):                                      */
#define NDPP_DERIVE_NONFINITE 1 /* an input of the row, or an entry of out, is not finite            */
#define NDPP_DERIVE_NEGBIN 2    /* bins: an output bin is below zero; moments: an input bin is       */
#define NDPP_DERIVE_ZERO 4      /* bins: a_0 == 0, the row is written as zeros                       */
/* The tables, host code, no device needed; each is [L][N], 1 <= L <= NDPP_MAX_ORDER,
 * 1 <= N <= NDPP_MAX_TAB_BINS, anything else (or a NULL pointer) NDPP_EINVAL.
 *   e_k = -1.0 + (2.0 * k) / N for k < N, e_N = 1.0: the edges of the N equal cosine bins
 *   P_l(e_k): Bonnet's recurrence upwards in the order of ndpp_scatt_sample,
 *     P_0 = 1.0, P_1 = x, P_{l+1} = (A_l * x) * P_l - B_l * P_{l-1}, A_l and B_l rounded once
 *   D_l(x) = P_{l+1}(x) - P_{l-1}(x)
 *   W[0][k] = (e_{k+1} - e_k) / 2
 *   W[l][k] = (D_l(e_{k+1}) - D_l(e_k)) / 2, l >= 1: the integral of (l + 1/2) P_l over bin k, a
 *     difference of the CDF terms ndpp_scatt_sample inverts
 *   V[0][k] = 1.0;  V[l][k] = (N * W[l][k]) / (2 l + 1), l >= 1: the mean of P_l over bin k
 *   pmin[l][k], pmax[l][k]: the smallest and the largest of P_l at the two edges of bin k and at the
 *     roots of P_l' strictly inside it, moved outward by 8 * DBL_EPSILON (8 ulp of 1) so that the
 *     evaluation error of P_l cannot make a bound too tight.  The roots are found on the host by
 *     bisection between neighbouring roots of P_l, down to neighbouring doubles.                     */
int ndpp_derive_tables(int L, int N, double *W /* [L][N] */, double *V, double *pmin, double *pmax);
/* Segmented sum over the middle axis.  first[Gc + 1] strictly increasing, first[0] = 0, first[Gc] = G:
 *   out[e][c][l] = mat[e][first[c]][l] + ... + mat[e][first[c+1] - 1][l]
 * Serves outgoing groups (any L >= 1: moments or bins alike), chi rows (L = 1) and, on the view
 * [n * G][N][1] of a tabular section, the merging of N bins into Gc = N' bins, N' a divisor of N.
 * NDPP_EINVAL, decided before the device is touched: n < 0, G < 1, L < 1, Gc outside 1..G, first NULL
 * or not as above, for n > 0 a NULL array, a G * L that does not fit an index, sizes whose bytes
 * overflow.  Without a device NDPP_EDEVICE; with one, n == 0 is an empty success.                    */
int ndpp_derive_groups(long n, int G, int L, const double *mat /* [n][G][L] */, int Gc,
                       const int *first /* [Gc+1] */, double *out /* [n][Gc][L] */);
/* Bins from moments.  With r = (e, g) a row of L moments a_l = mat[r][l]:
 *   t_k = sum over l of a_l * W[l][k]          (multiply, then add)
 *   a_0 == 0: NDPP_DERIVE_ZERO and t_k = 0.0 for every k, whatever the other moments hold (the
 *     writers drop such a row; a NaN or infinite a_l of it still sets NDPP_DERIVE_NONFINITE)
 *   out[r][k] = t_k;  NDPP_DERIVE_NONFINITE: an a_l or a t_k is not finite;  NDPP_DERIVE_NEGBIN: a
 *   t_k < 0 -- the row's density is negative somewhere and wants --repair-positivity
 *   (ndpp_scatt_repair) first; the bins are written as they come out.
 * sum_k t_k equals a_0 to rounding.  NDPP_EINVAL before the device is touched: n < 0, G < 1, L outside
 * 1..NDPP_MAX_ORDER, N outside 1..NDPP_MAX_TAB_BINS, for n > 0 a NULL array, an index or a size that
 * does not fit.  Without a device NDPP_EDEVICE; with one, n == 0 is an empty success.                */
int ndpp_derive_bins(long n, int G, int L, const double *mat /* [n][G][L] */, int N,
                     double *out /* [n][G][N] */, int *status /* [n][G] */);
/* Moments from bins.  With r = (e, g) a row of N bin integrals t_k = mat[r][k]:
 *   out[r][l] = sum over k of t_k * V[l][k]: the moments of the histogram t_k / (e_{k+1} - e_k);
 *     out[r][0] is the row's mass S exactly as ndpp_scatt_sample sums it
 *   lo[r][l]  = sum over k of t_k * pmin[l][k],  hi[r][l] = sum over k of t_k * pmax[l][k]
 *   NDPP_DERIVE_NEGBIN: a t_k < 0;  NDPP_DERIVE_NONFINITE: a t_k or an out[r][l] is not finite
 * lo and hi may be NULL (either or both).  For a row without NDPP_DERIVE_NEGBIN and ANY non-negative
 * density with these bin integrals, its moment a_l satisfies
 *   lo[r][l] - 1e-13 * S <= a_l <= hi[r][l] + 1e-13 * S
 * (the 1e-13 covers the rounding of the sums), and lo <= out <= hi holds as computed.  The histogram's
 * own moments are one member of that family, not the moments of the density the bins came from
 * (DESIGN.md section 21 has the distances).  For a row with NDPP_DERIVE_NEGBIN lo and hi mean
 * nothing: they are written, and enclose nothing.
 * NDPP_EINVAL and NDPP_EDEVICE as ndpp_derive_bins (out and status may not be NULL).                 */
int ndpp_derive_moments(long n, int G, int N, const double *mat /* [n][G][N] */, int L,
                        double *out /* [n][G][L] */, double *lo, double *hi /* [n][G][L], may be NULL */,
                        int *status /* [n][G] */);

#ifdef __cplusplus
}
#endif
#endif /* NDPP_HIP_H */
