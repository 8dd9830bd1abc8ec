/* gwi_engine.h -- C ABI of the MI355X-native hierarchical population-likelihood engine.
 *
 * GWInferno (the reference) has no FFI layer: its hot path is a set of Python calling
 * conventions.  This header is the C-ABI seam a binding would target; every
 * entry point names the reference interface it stands in for (paths relative to the reference
 * root).  The library behind it is gwinferno_amd/_lib/libgwi_engine.so (hand-written HIP for
 * gfx950); there is NO CPU fallback -- without a usable GPU gwi_create() fails with
 * GWI_ERR_NO_DEVICE.
 *
 * Data model
 *   A *catalog* is two sample sets that share one column schema:
 *     PE set         n_ev x n_pe samples, event-major (pedict[param] : (N_ev, N_pe),
 *                    gwinferno/pipeline/utils.py:82-84)
 *     injection set  n_inj samples        (injdict[param] : (N_inj,), pipeline/utils.py:86)
 *   Columns are float64 and hold per-sample quantities that do not depend on the
 *   hyper-parameters (log m1, log q, log(1+z), spline coordinates, ...).  One column, `kappa`,
 *   holds log(dVc/dz) - log(prior) with -inf for samples any static truncation excludes
 *   (models/bsplines/single.py:54-55, distributions.py:119,143,162, parametric.py:141-145,
 *   tests/inference_test.py:172).
 *   A *model* is a product of terms (gwi_term); each term reads <= 2 columns and a few entries of
 *   the flat hyper-parameter vector theta.  Grid normalisers (interpolation.py:280-291,
 *   parametric.py:123-124, spline_perturbation.py:323-336) are described by gwi_norm.
 *
 * Threading: one handle = one device + one HIP stream; gwi_eval* are not re-entrant per handle;
 * distinct handles are independent.  Ownership: the caller owns every host buffer passed in or
 * out; the engine copies inputs during gwi_create and owns all device memory.  Errors: integer
 * status, never C++ exceptions; non-finite likelihood values are VALUES (reference semantics,
 * jnp.nan_to_num at pipeline/analysis.py:280-315), not errors.
 */
#ifndef GWI_ENGINE_H
#define GWI_ENGINE_H

#ifndef __HIPCC_RTC__ /* hipRTC defines the fixed-width integer types itself and has no system headers */
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define GWI_ABI_VERSION 3 /* 2: GWI_TERM_PLPEAK takes ONE column (log x); 3: GWI_MAX_NORMS 8 -> 12, GWI_MAX_COLS 16 -> 32 (gwi_spec grows) */
#define GWI_MAX_TERMS 12
#define GWI_MAX_THETA 256
#define GWI_MAX_NORMS 12 /* one grid normaliser per term at most */
#define GWI_MAX_COLS 32  /* twelve terms x two columns + kappa fit */

typedef int32_t gwi_status;
enum {
  GWI_OK = 0,
  GWI_ERR_INVALID = -1,     /* malformed spec / argument */
  GWI_ERR_NO_DEVICE = -2,   /* no usable gfx950 device: the engine never falls back to the CPU */
  GWI_ERR_HIP = -3,         /* a HIP runtime call failed; see gwi_last_error() */
  GWI_ERR_UNSUPPORTED = -4, /* gradient of marginalize_selection via gwi_combine; host placement unknown */
  GWI_ERR_TIMEOUT = -5
};

/* Term kinds.  `cols[]` index the catalog's column table, `theta[]` index the flat
 * hyper-parameter vector, `p[]` are fixed constants. */
enum {
  /* x^alpha on the fixed interval [lo,hi]           distributions.py:100-119 (scalar bounds)
   * cols[0]=log x; theta[0]=alpha; p[0]=lo, p[1]=hi */
  GWI_TERM_POWERLAW = 1,
  /* (1-lam) PL(x;alpha,lo,hi) + lam TN(x;mpp,sigpp,lo,hi)   parametric.py:49-53 (delta=None)
   * cols[0]=log x (the kernels form x = exp(log x) for the Gaussian component themselves: one exponential per sample instead
   * of a second 8-byte column -- config 2 then streams its algorithmic 32 B per sample, not 40); theta = alpha, mpp, sigpp, lam;
   * p[0]=lo, p[1]=hi */
  GWI_TERM_PLPEAK = 2,
  /* q^beta on [mmin/m1, 1]: powerlaw_pdf(q, beta, mmin/m1, 1)   parametric.py:28,40; separable.py:364
   * cols[0]=log q, cols[1]=log m1; theta[0]=beta; p[0]=log(mmin).
   * m1 == mmin (an empty q interval, a NaN weight in the reference) is the CALLER's to exclude through kappa, on the quotient
   * mmin / m1; a live sample whose log m1 equals log(mmin) is an m1 an ulp above mmin and is evaluated at r = 1 - 2^-53.
   * With GWI_RATIO_LOGM_FROM_SPLINE in flags, cols[1] is the coordinate column of a spline term in log m1 of the same model
   * (BSplinePrimaryPowerlawRatio, separable.py:295-365: the LogXLogYBSpline of m1) and p[1], p[2], p[3] = that spline's lo,
   * (n_basis - 3) / (hi - lo), (hi - lo) / (n_basis - 3): the engine keeps that column as the knot coordinate u and this term
   * forms log m1 = lo + u dx itself -- one column per sample less (config 3: 64 B per sample, the algorithmic figure, not 72).
   * The caller guarantees that every sample alive for this term lies inside that spline's domain (the spline's own mask). */
  GWI_TERM_POWERLAW_RATIO = 3,
  /* Beta(a; alpha, beta) on [0, 1]                  distributions.py:146-162, parametric.py:63-81
   * cols[0]=log a, cols[1]=log(1-a); theta = alpha, beta */
  GWI_TERM_BETA = 4,
  /* (1-xi)/2 + xi TN(ct; 1, sigma, -1, 1)           parametric.py:84-86
   * cols[0]=cos tilt; theta = xi, sigma */
  GWI_TERM_TILT_MIXTURE = 5,
  /* dVc/dz (1+z)^(lamb-1) / Z(lamb)                 parametric.py:112-145
   * cols[0]=log(1+z) (log dVc/dz lives in kappa); theta[0]=lamb; norm = grid normaliser id */
  GWI_TERM_POWERLAW_REDSHIFT = 6,
  /* exp(sum_k c_k B_k(x)) [/ Z(c)] on uniform cubic B-splines   interpolation.py:360-449,
   * models/bsplines/single.py:77-109, spline_perturbation.py:352
   * cols[0]=spline coordinate (x or log x); coef_off/n_basis; p[0]=lo, p[1]=hi of the coordinate;
   * flags: GWI_SPLINE_OUTSIDE_ZERO_EXPONENT; norm = grid normaliser id or -1 */
  GWI_TERM_EXP_SPLINE = 7,
  /* truncated normal TN(x; mu, sigma, lo, hi)       distributions.py:122-143 (log=False)
   * cols[0]=x; theta = mu, sigma; p[0]=lo, p[1]=hi */
  GWI_TERM_TRUNCNORM = 8,
  /* sum_k c_k B_k(x) [/ Z(c)]: linear-Y B-spline density (BSpline basis)   interpolation.py:293-317,
   * models/bsplines/single.py:199-318 (chi_eff, chi_p)
   * cols[0]=spline coordinate; coef_off/n_basis; p[0]=lo, p[1]=hi; norm = grid normaliser (linear) or -1.
   * Non-positive values of the spline count as zero density. */
  GWI_TERM_LINEAR_SPLINE = 9,
  /* (1-xi)/4 + xi TN(ct1;1,sigma,-1,1) TN(ct2;1,sigma,-1,1)   parametric.py:97-102 (default_spin_tilt)
   * cols = cos tilt 1, cos tilt 2; theta = xi, sigma */
  GWI_TERM_TILT_JOINT = 10,
  /* low-mass taper as the reference evaluates it: 1 / (1 + exp(d/(x-xmin) + d/(x-xmin-d))) for EVERY x
   * (distributions.py:16-21: the second `where` condition holds for all x), e.g. smooth(delta, q m1, mmin)
   * of plpeak_primary_ratio_pdf (parametric.py:39-46).  cols[0] = x - xmin; theta[0] = d (delta) */
  GWI_TERM_SMOOTH = 11,
  /* (1-lam) PL(x) smooth(delta, x, lo) + lam TN(x): plpeak_primary_pdf with delta (parametric.py:49-53).
   * cols[0]=x, cols[1]=log x; theta = alpha, mpp, sigpp, lam; coef_off = theta index of delta; p[0]=lo, p[1]=hi */
  GWI_TERM_PLPEAK_SMOOTH = 12,
  /* x^alpha on [lo,hi] with the BOUNDS hyper-parameters too: Powerlaw.log_prob with sampled minimum / maximum
   * (numpyro_distributions.py:101-136; examples/config_files/config.yml:8-25).  cols[0]=log x, cols[1]=x; theta = alpha, lo, hi.
   * x < lo | x > hi is excluded (a sample exactly on a bound is inside); the gradient w.r.t. lo / hi is 0 (the normaliser cancels in log_l and the
   * truncation itself is piecewise constant), as reverse-mode differentiation of the reference gives. */
  GWI_TERM_POWERLAW_BOUNDS = 13,
  /* exp(interp(x, grid, lpdfs)) / Z, lpdfs_g = sum_k c_k B_k(us_g): BSplineDistribution.log_prob
   * (numpyro_distributions.py:266-293).  cols[0] = fractional grid index of the sample (j + f, clamped to the grid as
   * np.interp holds the end values); coef_off/n_basis; p[0]=lo, p[1]=hi of the spline coordinate; norm = the grid
   * normaliser whose `us` table (spline coordinate per grid point) and trapezoid weights define grid and Z (required);
   * flags: GWI_SPLINE_OUTSIDE_ZERO_EXPONENT as for EXP_SPLINE (otherwise a grid point outside [lo,hi] has lpdf -inf) */
  GWI_TERM_EXP_SPLINE_LERP = 14,
  /* EXP_SPLINE / LINEAR_SPLINE with a NARROW coordinate column: meaning, p[], flags, normaliser and gradient are those of kinds 7
   * and 9; the engine keeps cols[0] as the raw spline coordinate x in float32 (4 bytes per sample in HBM instead of 8) and the
   * scan forms the knot coordinate u = (x - p[0]) (n_basis - 3) / (p[1] - p[0]) itself, with the arithmetic (and clamp) of the
   * one-off conversion the wide kinds get -- the same u to the bit.  Every value of the column, posterior samples and injections,
   * must survive a float32 round trip (gwi_create / gwi_create_ingest fail with GWI_ERR_INVALID otherwise, naming the term and
   * the number of offending values); non-finite entries (excluded samples: kappa = -inf) are parked at the float32 value
   * nearest the domain's midpoint.  No other term may read the column (no other kind, no kind 7 / 9, no
   * GWI_RATIO_LOGM_FROM_SPLINE reference); several narrow terms may.  The term order of a model is canonical with these kinds
   * ranked as their wide twins (15 as 7, 16 as 9). */
  GWI_TERM_EXP_SPLINE_F32 = 15,
  GWI_TERM_LINEAR_SPLINE_F32 = 16
};

/* POWERLAW flag: bare x^alpha with no normaliser and no truncation (the (m2/m1)^beta pairing factor,
 * models/bsplines/separable.py:609-613, :703). */
#define GWI_POWERLAW_UNNORMALISED 2
#define GWI_RATIO_LOGM_FROM_SPLINE 8 /* GWI_TERM_POWERLAW_RATIO: see there */
/* gwi_norm.spline_flags bit: the integrand is the linear spline itself, Z = sum_g tw_g sum_k c_k B_k
 * (BSpline.norm, interpolation.py:280-291), not exp(...) of it. */
#define GWI_NORM_LINEAR_SPLINE 4

/* EXP_SPLINE flag: outside [lo,hi] the basis is 0 (BSpline/LogXBSpline.bases,
 * interpolation.py:175) so the factor is exp(0)=1, instead of the sample being excluded
 * (LogY bases, :407,:449 -- those are folded into kappa by the caller). */
#define GWI_SPLINE_OUTSIDE_ZERO_EXPONENT 1

typedef struct {
  int32_t kind;
  int32_t cols[2];
  int32_t theta[4];
  int32_t n_basis;  /* EXP_SPLINE */
  int32_t coef_off; /* EXP_SPLINE: theta offset of c_0 */
  int32_t flags;
  int32_t norm;     /* index into gwi_spec.norms of the normaliser dividing this term, or -1 */
  int32_t reserved;
  double p[4];
} gwi_term;

/* Grid normaliser  Z = sum_g tw[g] * exp( lb[g] + (theta[expo_theta]+expo_add) * l1[g]
 *                                        + sum_k theta[coef_off+k] B_k(us[g]) )
 * tw = trapezoid weights of the reference's grid (0 where the reference's integrand is masked). */
typedef struct {
  int32_t n_pts;
  int32_t expo_theta; /* -1: no power-law factor */
  int32_t n_basis;    /* 0: no spline factor */
  int32_t coef_off;
  int32_t spline_flags;
  int32_t reserved;
  double expo_add;
  double lo, hi;      /* spline coordinate domain */
  const double* tw;
  const double* lb;   /* may be NULL (zeros) */
  const double* l1;   /* may be NULL iff expo_theta < 0 */
  const double* us;   /* may be NULL iff n_basis == 0 */
} gwi_norm;

typedef struct {
  int32_t abi_version; /* GWI_ABI_VERSION */
  int32_t n_cols;
  int32_t kappa_col;
  int32_t n_theta;
  int32_t n_terms;
  int32_t n_norms;
  int32_t vt_norm;     /* normaliser reported as `surveyed_hypervolume` (analysis.py:267), or -1 */
  int32_t reserved;
  gwi_term terms[GWI_MAX_TERMS];
  gwi_norm norms[GWI_MAX_NORMS];
} gwi_spec;

/* Likelihood options == keyword arguments of hierarchical_likelihood (analysis.py:139-163). */
typedef struct {
  double n_obs;        /* Nobs (global number of events) */
  double total_inj;    /* total_inj */
  int32_t marginalize_selection;
  int32_t min_neff_cut;
  int32_t max_variance_cut;
  int32_t reserved;
} gwi_options;

/* Scalar results of one evaluation; names follow the numpyro sites of analysis.py:260-319. */
typedef struct {
  double log_likelihood;      /* numpyro.factor("log_likelihood") :319 (after every cut) */
  double log_l;               /* site "log_l" :284-291 */
  double sum_logBFs;          /* :282 */
  double selection_factor;    /* :278-281 */
  double log_det_eff;         /* log mu before marginalisation / cuts :259 */
  double log_nEff_inj;        /* :260 */
  double variance_log_detection_efficiency; /* :265 */
  double variance_log_likelihood;           /* :305-308 */
  double min_log_nEff;        /* min_i log n_eff_i (:295) */
  double surveyed_hypervolume_norm; /* Z of spec.vt_norm (raw; the site divides by 1e9, x Tobs) */
  double log_norm_const;      /* sum of sample-independent log-normalisers folded out of the scan */
  double reserved[5];
} gwi_summary;

typedef struct gwi_engine* gwi_handle;

/* device argument of gwi_create: the current HIP device, or a host-only handle that owns no device
 * memory and supports only gwi_prepare_combine / gwi_combine / gwi_partial_len (used by ranks that
 * merely assemble gathered records, and by the CPU test-suite). */
#define GWI_DEVICE_CURRENT (-1)
#define GWI_DEVICE_HOST_ONLY (-2)

/* Build an engine for one catalog + model.  Stands in for the reference's model construction
 * (Base1DBSplineModel.__init__, single.py:35-58; PowerlawRedshiftModel.__init__,
 * parametric.py:113-121): copies the columns to HBM once.  `pe_cols[c]` has n_ev*n_pe entries
 * (event-major), `inj_cols[c]` n_inj.  device < 0 selects the current HIP device. */
gwi_status gwi_create(const gwi_spec* spec, const double* const* pe_cols, int64_t n_ev, int64_t n_pe,
                      const double* const* inj_cols, int64_t n_inj, int32_t device, gwi_handle* out);

/* ---- setup on the device ---------------------------------------------------------
 * The reference prepares its per-sample, hyper-parameter-independent quantities eagerly on the host when the model
 * objects are constructed: validity masks (models/bsplines/single.py:54-55, distributions.py:119,143,162,
 * parametric.py:141-145), logarithms of the mass / ratio / redshift columns (interpolation.py:357,447), dVc/dz per
 * sample by linear interpolation into the comoving-distance table (cosmology.py:95-120, parametric.py:116) and the
 * division by the sampling prior (examples/simple_bspline_example.py:58-71).  gwi_create_ingest() takes the RAW catalog
 * columns (the arrays of pedict / injdict, float64 or float32) and a small register program per sample set that
 * describes those operations; one HIP kernel evaluates the program for every sample and writes the engine's columns
 * (kappa included) straight into HBM.  The program is straight-line code over `n_regs` fp64 registers (booleans are
 * 0.0 / 1.0), the same for every sample:
 *
 *   LOAD  dst <- sources[a][i]           CONST dst <- k
 *   LOG LOG1P NEG ABS NOT SQRT ISFINITE  dst <- f(r[a])
 *   ADD SUB MUL DIV LT GT LE GE AND OR   dst <- r[a] (op) r[b]         (IEEE fp64, never fused)
 *   WHERE dst <- r[a] != 0 ? r[b] : r[c]
 *   INTERP dst <- linear interpolation of r[a] in (tables[b], tables[c]), end values held outside (numpy.interp /
 *                 jnp.interp as used at cosmology.py:111-120); NaN in, NaN out
 *   GRIDINDEX dst <- j + f, the piece j and weight f numpy.interp would use on tables[b]
 *   STORE  column dst <- r[a]
 *
 * Every step except LOG / LOG1P reproduces the host (NumPy) evaluation of the same program to the bit. */
enum {
  GWI_ING_LOAD = 0, GWI_ING_CONST = 1,
  GWI_ING_LOG = 2, GWI_ING_LOG1P = 3, GWI_ING_NEG = 4, GWI_ING_ABS = 5, GWI_ING_NOT = 6, GWI_ING_SQRT = 7, GWI_ING_ISFINITE = 8,
  GWI_ING_ADD = 10, GWI_ING_SUB = 11, GWI_ING_MUL = 12, GWI_ING_DIV = 13, GWI_ING_LT = 14, GWI_ING_GT = 15, GWI_ING_LE = 16,
  GWI_ING_GE = 17, GWI_ING_AND = 18, GWI_ING_OR = 19,
  GWI_ING_WHERE = 20, GWI_ING_INTERP = 21, GWI_ING_GRIDINDEX = 22, GWI_ING_STORE = 23
};
#define GWI_INGEST_MAX_REGS 64
#define GWI_INGEST_MAX_SOURCES 32
#define GWI_INGEST_MAX_TABLES 16
enum { GWI_DTYPE_F64 = 0, GWI_DTYPE_F32 = 1 };

typedef struct gwi_ingest_op {
  int32_t op, dst, a, b, c, reserved;
  double k;
} gwi_ingest_op;

typedef struct gwi_ingest_program {
  int32_t n_ops, n_regs, n_sources, n_tables;
  const gwi_ingest_op* ops;
  const void* const* sources;      /* host arrays, one value per sample of the set, in sample order */
  const int32_t* source_dtype;     /* GWI_DTYPE_F64 | GWI_DTYPE_F32 per source */
  const double* const* tables;     /* host arrays */
  const int64_t* table_len;
} gwi_ingest_program;

/* gwi_create() with the columns computed on the device: `pe` / `inj` must STORE every column 0 .. spec->n_cols-1 of
 * their sample set.  Raw sources are uploaded once (float32 ones as float32) and released after the kernel ran. */
gwi_status gwi_create_ingest(const gwi_spec* spec, const gwi_ingest_program* pe, int64_t n_ev, int64_t n_pe,
                             const gwi_ingest_program* inj, int64_t n_inj, int32_t device, gwi_handle* out);

/* The ingest kernel on its own: run `prog` over n samples on `device` and copy the n_cols columns it stores back to
 * the host (cols[c] has n entries).  What the parity test of the setup path compares with the host evaluation. */
gwi_status gwi_ingest_columns(const gwi_ingest_program* prog, int64_t n, int32_t n_cols, double* const* cols, int32_t device);

/* Copy column `col` of an engine's resident catalog back to the host (`pe_side` != 0: n_ev * n_pe entries, else n_inj).
 * Resident means what the kernels read: a column that only GWI_TERM_EXP_SPLINE / GWI_TERM_LINEAR_SPLINE terms with one set of
 * knots read holds the KNOT coordinate (x - p[0]) * (n_basis - 3) / (p[1] - p[0]) of the spline coordinate x the caller handed
 * over (clamped into [0, n_basis - 3) for exponentiated splines without GWI_SPLINE_OUTSIDE_ZERO_EXPONENT), computed once at
 * gwi_create / gwi_create_ingest; every other column is returned as it was handed over or ingested.  A narrow column
 * (GWI_TERM_EXP_SPLINE_F32 / GWI_TERM_LINEAR_SPLINE_F32) holds the raw coordinate in float32: it is returned widened to float64
 * (non-finite entries as parked). */
gwi_status gwi_read_column(gwi_handle h, int32_t pe_side, int32_t col, double* out);

/* Bytes of catalog columns the scan kernels stream, per sample set: the sum over the resident columns (kappa, every term's
 * columns and their private knot-coordinate copies) of 8 bytes (4 for a narrow column) x n_ev * n_pe (pe_bytes) or x n_inj
 * (inj_bytes).  Either output may be NULL. */
gwi_status gwi_resident_bytes(gwi_handle h, int64_t* pe_bytes, int64_t* inj_bytes);

/* One value-and-gradient evaluation == one execution of the user's NumPyro model body ending in
 * hierarchical_likelihood(...) (analysis.py:139-319) under jit(value_and_grad)
 * (tests/inference_test.py:320-326).  theta has spec.n_theta entries.  Nullable outputs:
 * grad[n_theta] = d log_likelihood / d theta; log_bfs / log_neffs / variances [n_ev] = sites
 * "logBFs", "log_nEffs", "variance_log_BFs"; norms[n_norms] = normaliser values Z.
 * A non-finite theta yields the reference's NaN branch: log_likelihood = nan_to_num(-inf), zero gradient
 * (analysis.py:287-289).  With opt->marginalize_selection and a gradient requested, a second launch set
 * with squared weights supplies sum_j w_j^2 dl_j/dtheta (analysis.py:270-271). */
gwi_status gwi_eval(gwi_handle h, const double* theta, const gwi_options* opt, gwi_summary* summary,
                    double* grad, double* log_bfs, double* log_neffs, double* variances, double* norms);

/* The same in two halves, for several handles in flight on one GPU (independent chains whose trajectory
 * lengths differ cannot be batched in lock step, but their evaluations can overlap): gwi_eval_begin() does the
 * host prelude and issues the launches of handle h, gwi_eval_end() waits for and assembles that evaluation.
 * gwi_eval == begin + end.  One evaluation per handle may be pending; every handle has its own stream,
 * buffers and copy of the catalog. */
gwi_status gwi_eval_begin(gwi_handle h, const double* theta, const gwi_options* opt, int32_t want_grad);
gwi_status gwi_eval_end(gwi_handle h, gwi_summary* summary, double* grad, double* log_bfs, double* log_neffs,
                        double* variances, double* norms);

/* k_batch hyper-parameter points in ONE set of launches (blockIdx.y = point): what vectorised
 * multi-chain NUTS evaluates per step.  thetas[k_batch][n_theta] row-major; outputs are arrays of
 * k_batch entries (summaries[k], grads[k][n_theta], log_bfs[k][n_ev], ..., norms[k][n_norms]; any may
 * be NULL).  The catalog is streamed from HBM once per workgroup tile and re-read from L2/Infinity
 * Cache for the other points; launch, combine and host latencies are paid once per batch.
 * k_batch <= GWI_MAX_BATCH (environment, default 16, at most 64). */
gwi_status gwi_eval_batch(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, gwi_summary* summaries,
                          double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms);

/* The same in two halves, like gwi_eval_begin / gwi_eval_end: begin does the host prelude and issues the launches of the K points
 * (after, on a spline model's first batch, the blocking measurement of its two batched kernels; and after the blocking
 * squared-weight pass when opt->marginalize_selection and want_grad), end waits for and assembles them.  A blocking batch leaves
 * the GPU to its combine / final launches and the host for a third of its time: two or three sets in flight -- one handle each,
 * ONE host thread -- fill it (config 2, K = 16: 243 k -> 315-360 k evaluations per second).  want_events: the per-event sites
 * will be asked for at gwi_eval_batch_end.  One evaluation or batch per handle may be pending. */
gwi_status gwi_eval_batch_begin(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, int32_t want_grad, int32_t want_events);
gwi_status gwi_eval_batch_end(gwi_handle h, gwi_summary* summaries, double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms);

/* Which kernel a batched launch of k_batch points would use: "taps" (one grid row per point, 4-tap gradient into LDS rows;
 * the default) or "mfma" (GWI_BATCH_MFMA=1 at gwi_create, models with spline terms whose term sequence and basis counts
 * have a matrix-core instantiation, k_batch >= 9: the spline-coefficient gradient as a v_mfma_f64_16x16x4 GEMM over 16
 * points per wavefront, gwinferno_amd/csrc/gwi_mfma.h).  Both are kept because both are measured: see DESIGN.md.
 * Models without spline terms: "rows-per-point" (one grid row per point, scan_kernel BATCH: the default since round 6) or
 * "pbatch" (GWI_PBATCH=1 or a row size GWI_PBATCH_PTS: scan_pbatch_kernel, every sample loaded once for the points a workgroup
 * draws; which of the two is faster depends on the box, within 10 %: profiles/round6/EXPERIMENTS.md section 5). */
const char* gwi_batch_path(gwi_handle h, int32_t k_batch);
/* Spline models that have both batched kernels: which one runs follows a STATIC rule by default (matrix cores from 9 points per
 * launch on, up to 8 gradient tiles; otherwise the 4-tap kernel) -- the two kernels sum in different orders, so the same model on
 * the same catalog must not get one or the other from a race of wall times.  The environment can name a path (GWI_BATCH_MFMA,
 * GWI_BATCH_ROWS) or, with GWI_BATCH_AUTOTUNE=1, ask for a measurement on the engine's FIRST batched launch of >= 9 points (three
 * evaluation sets of each on the caller's own points, host theta -> host results; the faster stays; per handle; last-bit results
 * then depend on which kernel won).  gwi_batch_path answers with the static rule, or with the measured choice after that launch;
 * this returns whether a measurement has been made and the best microseconds per evaluation set of either kernel. */
gwi_status gwi_batch_calibration(gwi_handle h, int32_t* measured, double* mfma_us, double* taps_us);
/* A spline model whose kinds and basis counts have no ahead-of-time matrix-core instantiation gets one compiled at run time
 * (gwinferno_amd/csrc/gwi_jit.h) on its first batched launch of >= 9 points (at gwi_create with GWI_BATCH_MFMA=1): this says what
 * happened -- "compiled jit-mfma:6,207,107 ..." or why not (more than eight 16-basis gradient tiles, a term without a matrix-core
 * form, register spills, hipRTC missing); "" before the attempt and for models that have an ahead-of-time instantiation. */
const char* gwi_batch_kernel_note(gwi_handle h);

/* Per-sample log-weights log(p(theta|Lambda)/prior) (-inf for excluded samples), the arrays the
 * reference passes to hierarchical_likelihood as pe_weights / inj_weights (tests/inference_test.py:
 * 174-175).  Diagnostic / parity entry point; not used on the sampling path. */
gwi_status gwi_log_weights(gwi_handle h, const double* theta, double* pe_logw, double* inj_logw);

/* Weighted index draws on the device: what the reference's posterior-predictive branch does per hyper-parameter point
 * (pipeline/analysis.py:321-355: per event one posterior sample drawn with probability proportional to its population weight,
 * and found injections from the injection weights) and what reweighted single-event posteriors and predicted-detection samples
 * are made of -- without the per-sample weights ever leaving HBM (gwinferno_amd/csrc/gwi_draw.h).
 *
 * A segment is one event's n_pe posterior samples, or the injection set.  For a segment with log-weights lw_j (those of
 * gwi_log_weights), a 0/1 mask a_j and a uniform u in [0, 1):  M = max of lw_j over samples with a_j = 1 and lw_j finite;
 * w_j = a_j ? exp(lw_j - M) : 0 (0 for a non-finite lw_j);  C_j = w_0 + ... + w_j;  the draw is the smallest j with
 * C_j > u C_last and w_j > 0 (the last sample with positive weight when rounding runs past the end), -1 for a segment without
 * any positive weight.  The uniforms are the caller's: there is no random number generator on the device.  The order of summation
 * is fixed, so the indices are a pure function of the arguments (same on every call and on every handle of one model).
 *
 * gwi_set_draw_mask(): the masks (the mass cuts of analysis.py:326-338, which depend on the catalog only) -- pe_mask has
 * n_ev * n_pe bytes (uint8, event-major), inj_mask n_inj; copied to HBM once; NULL = all ones (the state of a new handle).
 * gwi_draw_indices(): for each of the k points thetas[k][n_theta], n_draw_pe draws per event (u_pe[k][n_ev][n_draw_pe] ->
 * idx_pe of the same shape: indices within the event) and n_draw_inj draws from the injection set (u_inj[k][n_draw_inj] ->
 * idx_inj).  Either count may be 0 (its pointers are then ignored).  k is not bound by the batch limit: the points are evaluated
 * one after another inside the library and the indices come back in one copy -- the only device-to-host traffic.
 * GWI_ERR_INVALID for bad counts / null pointers and for host-only handles; GWI_ERR_UNSUPPORTED on a handle that holds a shard
 * (after gwi_comm_init / gwi_shm_comm_init): injection draws need the global set. */
gwi_status gwi_set_draw_mask(gwi_handle h, const unsigned char* pe_mask, const unsigned char* inj_mask);
gwi_status gwi_draw_indices(gwi_handle h, const double* thetas, int32_t k, const double* u_pe, int32_t n_draw_pe, const double* u_inj, int32_t n_draw_inj,
                            int32_t* idx_pe, int32_t* idx_inj);

/* Resampled injection sets on the device: the reference's resample_injections (preprocess/selection.py:143-156), which thins a
 * found-injection set to the set a fiducial population theta would have produced -- N = floor((sum w)^2 / sum w^2) injections drawn
 * with replacement in proportion to w = p(.|theta) / prior -- for many draws from one segment, with the generator on the device
 * (gwinferno_amd/csrc/gwi_resample.h; the NumPy statement is gwinferno_amd/draws.py: resample_indices_reference).
 *
 * The injection set is one segment of gwi_draw_indices: the same lw_j, the same mask (the injection mask of gwi_set_draw_mask
 * applies), M, w_j = exp(lw_j - M) and the same tile masses and tile prefix; C_j is the inclusive prefix inside a tile of 1 024 samples
 * on top of the preceding tile's prefix, every sum of a fixed shape (the same bits on every call and on every handle of one model).
 * Draw d has stream index first_index + d and takes one Philox4x32-10 block with key = seed (low word, high word) and counter
 * (index low, index high, 0, 0x52534D50); u = words 0,1, a uniform being ((hi >> 5) 2^26 + (lo >> 6)) 2^-53.  The target is u C_last;
 * a binary search finds a tile whose prefix exceeds it and whose predecessor's does not, a tile without mass is passed over for the
 * next one with mass, a target past the end takes the last tile with mass; inside the tile the same search runs on the in-tile prefix
 * against the rest of the target and yields the first sample with w_j > 0 from there on, else the tile's last sample with weight.
 * idx[d] is that sample and logw_sel[d] = lw_idx (gwi_log_weights' value, sample-independent constant included: bit for bit).
 *
 * n_request < 0 makes the reference's N draws, N = floor(n_eff); otherwise exactly n_request draws are made.  *n_draws is the number
 * made.  idx and logw_sel hold n_request entries, or n_inj when n_request < 0 (N <= n_inj always); they may be NULL for n_request = 0.
 * sums[4] = { log sum w, log sum w^2, n_eff = (sum w)^2 / sum w^2, the number of injections with w_j > 0 }, the logarithms absolute
 * (M and the sample-independent constant included), whatever n_request.  A draw depends on (catalog, mask, theta, seed,
 * first_index + d) only -- not on the cut into launches of 2^20 draws, nor on how a request is split over calls.  Without any live
 * sample: GWI_OK, *n_draws = 0, sums = { -inf, -inf, 0, 0 }, nothing written to idx / logw_sel.
 * GWI_ERR_INVALID for null pointers, a host-only handle or first_index < 0; GWI_ERR_UNSUPPORTED on a handle that holds a shard, as
 * gwi_draw_indices.
 *
 * gwi_resample_times(): DIAGNOSTIC ONLY, for tools/resample_injections_time.py: of the calling thread's last call, the wall time of
 * the (blocking) log-weight pass and the device times (HIP events) of the tile / merge / prefix / stats launches together and of the
 * select launches together, and the number of select launches. */
gwi_status gwi_resample_injections(gwi_handle h, const double* theta, uint64_t seed, int64_t first_index, int64_t n_request, int64_t* n_draws, double* sums /* [4] */,
                                   int32_t* idx, double* logw_sel);
void gwi_resample_times(double* logw_ms, double* prefix_ms, double* select_ms, int32_t* launches);

/* Weighted histograms on the device: the population-informed posterior of every event, marginalised over hyper-parameter points,
 * and its counterpart for the selection, the predicted detected distribution from the injection set -- the deterministic
 * counterpart of the observed-versus-predicted check of the reference's posterior-predictive branch (pipeline/analysis.py:321-355),
 * which gwi_draw_indices estimates with one index per point (gwinferno_amd/csrc/gwi_hist.h; the NumPy statement is
 * gwinferno_amd/draws.py: weighted_histograms_reference).
 *
 * Segments, lw_j, the masks, M and w_j = exp(lw_j - M) are gwi_draw_indices' (the masks of gwi_set_draw_mask apply).  With
 * S = the sum of w_j over the whole segment, a point adds  h[c][b] = (the sum of w_j over the samples whose code in column c is b) / S
 * onto the running sums:  H[segment][c][b] += h[c][b], the points in the order of the call.  A sample coded 0xFFFF is in no bin but
 * counts in S, so a column's bins sum to at most 1 and the deficit is the weight share outside.  A segment whose S is 0 or not
 * finite adds nothing; dead[segment] is incremented instead (segment n_ev is the injection set).  Every sum has a fixed shape --
 * sample order within a tile of 1 024 samples and a bin, then tile order, then point order -- and there are no atomics: the bits of H
 * are a pure function of the arguments.
 *
 * gwi_set_histogram_bins(): 1 <= n_cols <= 8 binned quantities with 1 <= n_bins <= 256 bins each; pe_bins[n_cols][n_ev][n_pe] and
 * inj_bins[n_cols][n_inj] are the samples' bin codes (uint16; they do not depend on theta), copied to HBM once; either may be NULL
 * (that set is then left out), not both.  A code >= n_bins other than 0xFFFF is refused.  The workspace is allocated here.  A new
 * call replaces the bins.
 * gwi_weighted_histograms(): hist_pe[n_ev][n_cols][n_bins] (ignored without pe_bins), hist_inj[n_cols][n_bins] (ignored without
 * inj_bins) and dead[n_ev + 1] are IN/OUT: the caller's values are uploaded, the k points thetas[k][n_theta] are added in order, and
 * the sums are copied back -- (n_ev + 1) n_cols n_bins doubles per call, whatever k.  A request split over calls (2 + 1, 1 + 1 + 1)
 * therefore returns the bits of one call.  k is not bound by the batch limit.
 * GWI_ERR_INVALID (with a gwi_last_error message) for limits, codes, null pointers, a host-only handle and a call before the bins
 * are set; GWI_ERR_UNSUPPORTED on a handle that holds a shard, as gwi_draw_indices.
 *
 * gwi_histogram_times(): DIAGNOSTIC ONLY, for tools/weighted_histograms_time.py: of the calling thread's last call, summed over its
 * points, the wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge / histogram
 * tile launches together and of the histogram merge launches, and the number of kernel launches after the log-weight passes.  It
 * covers gwi_weighted_histograms_weighted() likewise.
 *
 * gwi_weighted_histograms_weighted(): the same sums with a linear weight per (point, segment), v[k][n_ev + 1] in [0, 1] (segment n_ev is
 * the injection set), uploaded once per call: H[segment][c][b] += v h[c][b] -- the quotient h is formed as without weights and then
 * multiplied by v in a product of its own, so v = 1 gives the bits of gwi_weighted_histograms() -- and vsum[segment] += v for a live
 * segment; the weighted mean over the points is H / vsum.  A point whose v is 0 adds nothing and does not touch dead[segment].  vsum
 * [n_ev + 1] is IN/OUT like the histograms and dead; k >= 1 as there.  Leave-one-out posteriors (v proportional to the reciprocal
 * of the event's own factor of the likelihood) and a change of hyper-prior (one v per point, the same for every segment) are both
 * stated this way.  GWI_ERR_INVALID also for a null v or vsum, an entry of v that is NaN, negative or above 1, and k < 0. */
gwi_status gwi_set_histogram_bins(gwi_handle h, int32_t n_cols, int32_t n_bins, const uint16_t* pe_bins /* [n_cols][n_ev][n_pe] or NULL */,
                                  const uint16_t* inj_bins /* [n_cols][n_inj] or NULL */);
gwi_status gwi_weighted_histograms(gwi_handle h, const double* thetas, int32_t k, double* hist_pe /* in/out [n_ev][n_cols][n_bins] */,
                                   double* hist_inj /* in/out [n_cols][n_bins] */, int32_t* dead /* in/out [n_ev + 1] */);
gwi_status gwi_weighted_histograms_weighted(gwi_handle h, const double* thetas, int32_t k, const double* v /* [k][n_ev + 1] */,
                                            double* hist_pe /* in/out [n_ev][n_cols][n_bins] */, double* hist_inj /* in/out [n_cols][n_bins] */,
                                            int32_t* dead /* in/out [n_ev + 1] */, double* vsum /* in/out [n_ev + 1] */);
void gwi_histogram_times(double* logw_ms, double* tile_ms, double* merge_ms, int32_t* launches);

/* Catalog predictive checks on the device: per hyper-parameter point the cumulative distributions that observed-versus-predicted
 * figures with credible bands and the extreme-event (outlier) test are made of (gwinferno_amd/csrc/gwi_cdf.h; the NumPy statement is
 * gwinferno_amd/draws.py: point_cdfs_reference; the contract is DESIGN 8g).  A band is a percentile over the points and the CDF of the
 * catalog's largest value a product over the events, P(max_e x_e <= g | theta_k) = prod_e F_ke(g): neither can be rebuilt from the
 * sums over points gwi_weighted_histograms returns, so these go back per point.
 *
 * The bins are those of gwi_set_histogram_bins, made as CUMULATIVE codes from a grid g_0 < ... < g_{G-1}, 1 <= G = n_bins <= 256
 * (draws.py: cdf_codes): a sample's code in a column is the number of grid points < x (np.searchsorted(grid, x, side="left")), so code
 * j < G means g_{j-1} < x <= g_j; code G, or a NaN value, becomes 0xFFFF: the sample counts in S and in no bin.  The sum of
 * h[c][0 ... j] is then exactly the weight share with x <= g_j, without a bin-width error, and 1 - the last entry the share above the
 * grid.  The library does not look at the grid: it sums whatever codes were set.
 *
 * For one point, with h[seg][c][b] the quotient gwi_weighted_histograms forms (tile order, then / S): F[seg][c][b] = the running sum
 * of h[seg][c][0 ... b], strictly left to right (the bits of np.cumsum).  A segment is live at the point where S > 0 and finite;
 * n_live counts the live events.  out[k][4][n_cols][n_bins] holds per point
 *   slot 0  cdf_det         F of the injection segment (n_ev); NaN if that segment is dead or there are no injection bins
 *   slot 1  cdf_obs         (sum of F over the live events, in event order) / n_live, one division at the end; NaN if n_live = 0 or
 *                           there are no PE bins
 *   slot 2  log_all_below   the sum of log F over the live events, in event order: the log CDF of the catalog's maximum; log 0 = -inf
 *                           stays
 *   slot 3  log_all_above   the sum of log1p(-min(F, 1)) over the live events, in event order: the CDF of the catalog's minimum is
 *                           1 - exp(.)
 * (slots 2 and 3 are NaN without PE bins and 0, the empty sum, with n_live = 0), and live[k][2] = (n_live, injection segment live ? 1
 * : 0; n_live is 0 without PE bins).  Nothing is in/out.  k >= 1 is not bound by the batch limit: the points are staged on the device 64
 * at a time and copied back per chunk, 4 n_cols n_bins doubles per point.  The masks of gwi_set_draw_mask apply.  No point weights go to
 * the device: a weight on the k axis (leave-one-out, a change of hyper-prior) is applied by the host to the K C G numbers.  Every sum has
 * a fixed shape and there are no atomics: the bits are a pure function of the arguments, whatever the split of the points over calls.
 * Not done: sharded handles; the events' own per-point CDFs travelling back (K n_ev C G numbers); more than 256 grid points.
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer, k < 1, a host-only handle and a call before the bins are set;
 * GWI_ERR_UNSUPPORTED on a handle that holds a shard, as gwi_weighted_histograms.
 *
 * gwi_point_cdf_times(): DIAGNOSTIC ONLY, for tools/point_cdfs_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge / histogram tile launches
 * together and of the two CDF launches, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_point_cdfs(gwi_handle h, const double* thetas, int32_t k, double* out /* [k][4][n_cols][n_bins] */, int32_t* live /* [k][2] */);
void gwi_point_cdf_times(double* logw_ms, double* tile_ms, double* reduce_ms, int32_t* launches);

/* Per-event calibration on the device: per hyper-parameter point and event a rigorous bracket of the probability integral transform
 * (PIT) of the event under the predicted detected distribution, PIT_kec = sum_i (w_ki / S_ke) F_det,k(x_i) -- what a P-P plot and its
 * leave-one-out form (LOO-PIT) are made of (gwinferno_amd/csrc/gwi_pit.h; the NumPy statement is gwinferno_amd/draws.py:
 * point_pits_reference with the loop pit_bracket; the contract is DESIGN 8h).  The PIT is a product of two per-point objects, the
 * event's weights and the injection set's CDF: no sum over points that another entry keeps can give it, and leave-one-out needs
 * another weight on the k axis for every event, so the brackets go back per (point, event).
 *
 * The bins are those of gwi_set_histogram_bins for BOTH sets, made as the cumulative codes of gwi_point_cdfs against one grid
 * g_0 < ... < g_{G-1} per column, 1 <= G = n_bins <= 256.  For one point, event e and column c: q[j] is the event's normalised bin (the
 * bits of what gwi_weighted_histograms returns for that single point), F_e = the running sum of q (the bits of np.cumsum), D[j] the
 * injection segment's CDF (the bits of gwi_point_cdfs slot 0) and o = max(0, 1 - F_e[G-1]) the event's share above the grid.  A sample
 * with code j lies in (g_{j-1}, g_j], so its F_det lies in [D[j-1], D[j]] with D[-1] := 0; a sample outside has F_det in [D[G-1], 1]:
 *   pit_lo = q[1] D[0] + q[2] D[1] + ... + q[G-1] D[G-2] + o D[G-1]
 *   pit_hi = q[0] D[0] + q[1] D[1] + ... + q[G-1] D[G-1] + o
 * bracket the un-gridded PIT; the error is the grid's alone (hi - lo <= max_j (D[j] - D[j-1]) when nothing lies outside).  Either is
 * summed from 0.0 strictly left to right, the outside term last, every product and every sum rounded on its own (no fused
 * multiply-add): the bits of a plain Python loop over the same q and D.
 *
 * pit[k][n_ev][n_cols][2] holds (lo, hi), NaN for an event or an injection segment without weight at the point; cdf_det[k][n_cols][n_bins]
 * (optional) holds D, NaN for a dead injection segment; dead[k][n_ev + 1] holds 1 for every segment without weight at the point, the
 * injection segment last.  Nothing is in/out.  k >= 1 is not bound by the batch limit: the points are staged on the device 64 at a time
 * and copied back per chunk.  The masks of gwi_set_draw_mask apply.  No point weights go to the device: a weight on the k axis is
 * applied by the host.  Every sum has a fixed shape and there are no atomics: the bits are a pure function of (theta_k, bins, masks),
 * whatever the split of the points over calls, and the call changes no state another entry reads.
 * Not done: sharded handles; the events' own per-point CDFs travelling back; more than 256 grid points (the exact un-gridded PIT is
 * gwi_point_pits_exact's, below).
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null thetas, pit or dead, k < 1, a host-only handle, a call before the bins are
 * set and a call while either set has no bins; GWI_ERR_UNSUPPORTED on a handle that holds a shard, as gwi_point_cdfs.
 *
 * gwi_point_pit_times(): DIAGNOSTIC ONLY, for tools/point_pits_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge / histogram tile launches
 * together and of the CDF and PIT launches, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_point_pits(gwi_handle h, const double* thetas, int32_t k, double* pit /* [k][n_ev][n_cols][2]: lo, hi */,
                          double* cdf_det /* [k][n_cols][n_bins] or NULL */, int32_t* dead /* [k][n_ev + 1] */);
void gwi_point_pit_times(double* logw_ms, double* tile_ms, double* pit_ms, int32_t* launches);

/* Exact per-event calibration on the device: per hyper-parameter point and event the UN-GRIDDED probability integral transform of the
 * event under the predicted detected distribution -- the weighted rank of every PE sample among the injections (gwinferno_amd/csrc/
 * gwi_rank.h; the NumPy statement is gwinferno_amd/draws.py: rank_codes, point_pits_exact_reference; the contract is DESIGN 8i).  With
 * Pareto-smoothed leave-one-out weights on the k axis (draws.py: pareto_smooth, applied by the host) it is what ArviZ calls loo_pit.
 *
 * gwi_set_rank_columns(): what does not depend on theta, made by the host once.  Per column c, 1 <= n_cols <= 8: order_inj[c] is a
 * permutation of the injections along which the column's values do not decrease (the library does not sort), rank_lt_pe[c][e][i] the
 * number of injections whose value lies below that of PE sample i of event e and rank_le_pe[c][e][i] the number at or below it: int32
 * in [0, n_inj], rank_lt <= rank_le, equal unless the sample ties with an injection.  The arrays are checked in O(n) (every order a
 * permutation, every rank in range, rank_lt <= rank_le), copied to HBM, and the entry's own workspace is allocated: the prefix table
 * P[n_cols][n_inj + 1], the tiles' partial sums and staging rows for 64 points.  The workspaces of gwi_set_histogram_bins and
 * gwi_set_quantile_columns are neither used nor resized.
 *
 * gwi_point_pits_exact(): for one point, u_j = exp(lw_j - M) are the injections' weights and w_i those of an event (0 for a masked or
 * non-finite sample; the masks of gwi_set_draw_mask apply), S_e the event's total, P[c][r] the sum of u over the first r injections
 * along order_inj[c] and T_c = P[c][n_inj]:
 *   pit_lt = sum_i w_i P[c][rank_lt_i] / S_e / T_c        pit_le = sum_i w_i P[c][rank_le_i] / S_e / T_c
 * pit_le is the PIT under F_det(x) = share of detected weight with x_inj <= x, pit_lt uses <; the two differ only through ties between
 * the two sets, and their midpoint is the expectation of the randomised PIT.  pit[k][n_ev][n_cols][2] holds (lt, le), NaN for an event
 * whose S is 0 or not finite and everywhere when the injection segment's is; dead[k][n_ev + 1] holds 1 for every segment without weight
 * at the point, the injection segment last.  k >= 1 is not bound by the batch limit: the points are staged on the device 64 at a time
 * and copied back per chunk.  Every sum has a fixed shape (rank order inside a tile of 1 024, then tile order) and there are no atomics:
 * the bits are a pure function of (theta_k, ranks, masks), whatever the split of the points over calls, and the call changes no state
 * another entry reads.  Not done: sharded handles; more than 8 columns; leave-one-out for the injection segment.
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer, k < 1, n_cols outside 1 ... 8, an order that is no permutation, a
 * rank outside [0, n_inj], rank_lt > rank_le, a host-only handle and a call before the rank columns are set; GWI_ERR_UNSUPPORTED on a
 * handle that holds a shard.
 *
 * gwi_point_rank_times(): DIAGNOSTIC ONLY, for tools/point_ranks_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge / three prefix launches
 * together and of the two PIT launches, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_set_rank_columns(gwi_handle h, int32_t n_cols, const int32_t* order_inj /* [n_cols][n_inj] */, const int32_t* rank_lt_pe /* [n_cols][n_ev][n_pe] */,
                                const int32_t* rank_le_pe /* [n_cols][n_ev][n_pe] */);
gwi_status gwi_point_pits_exact(gwi_handle h, const double* thetas, int32_t k, double* pit /* [k][n_ev][n_cols][2]: lt, le */, int32_t* dead /* [k][n_ev + 1] */);
void gwi_point_rank_times(double* logw_ms, double* prefix_ms, double* pit_ms, int32_t* launches);

/* Per-point moments on the device: per hyper-parameter point and segment the weighted means and the full weighted covariance of the
 * columns of gwi_set_kde_columns -- what a correlation between two quantities, taken point by point, is made of (gwinferno_amd/csrc/
 * gwi_moment.h; the NumPy statement is gwinferno_amd/draws.py: point_moments_reference; the contract is DESIGN 8j).
 *
 * gwi_point_moments(): the columns (C of them, 1 <= C <= 8) are read where gwi_set_kde_columns left them; nothing is copied and there is
 * no setter of this entry's own.  Segments, lw_i, the masks of gwi_set_draw_mask, M, w_i = exp(lw_i - M) and the segment total S are
 * gwi_draw_indices'.  For point k and segment s (the injection segment last), with P = C (C + 1) / 2:
 *   m_c  = sum_i w_i x_ci / S                                   out[k][s][c]
 *   V_cd = sum_i w_i (x_ci - m_c)(x_di - m_d) / S,  c <= d      out[k][s][C + t], t counting the upper triangle row by row
 * in two passes over the samples, the second centred on the means of the first.  A segment whose S is 0 or not finite gives NaN and
 * dead[k][s] = 1; the segments of a set that was given no columns give NaN (dead still tells whether they had weight); a segment with one
 * live sample gives that sample and a covariance of exactly 0.  k >= 1 is not bound by the batch limit: the points are staged on the
 * device 64 at a time and copied back per chunk.  Every sum has a fixed shape (sample order inside a tile of 1 024, then tile order)
 * and there are no atomics: the bits are a pure function of (theta_k, columns, masks), whatever the split of the points over calls, and
 * the call changes no state another entry reads.  Not done: sharded handles; more than 8 columns (rank correlation: gwi_point_rank_correlations; conditional means: gwi_point_conditionals).
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer, k < 1, a host-only handle and a call before columns are set;
 * GWI_ERR_UNSUPPORTED on a handle that holds a shard.
 *
 * gwi_point_moment_times(): DIAGNOSTIC ONLY, for tools/point_moments_time.py: of the calling thread's last call, summed over its points,
 * the wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge / two mean launches
 * together and of the two covariance launches, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_point_moments(gwi_handle h, const double* thetas, int32_t k, double* out /* [k][n_ev + 1][C + C(C+1)/2] */, int32_t* dead /* [k][n_ev + 1] */);
void gwi_point_moment_times(double* logw_ms, double* mean_ms, double* cov_ms, int32_t* launches);

/* Per-point conditional moments on the device: per hyper-parameter point and segment, for every bin of a conditioning quantity x, the
 * bin's share of the weight and the weighted mean and variance of another quantity y among the bin's samples -- E[y | x] and Var[y | x]
 * as functions of x, what a drift of a mean or a growth of a width with another quantity is stated in, and what a covariance (linear only)
 * does not see (gwinferno_amd/csrc/gwi_cond.h; the NumPy statement is gwinferno_amd/draws.py: point_conditionals_reference; the contract
 * is DESIGN 8k).
 *
 * gwi_point_conditionals(): pairs[r] = (cx, cy): cx a bin column of gwi_set_histogram_bins (n_bins is that setter's), cy a value column
 * of gwi_set_kde_columns; both are read where they lie, nothing is copied and there is no setter of this entry's own.  1 <= n_pairs <= 8
 * and n_pairs n_bins <= 512.  A sample set is covered when it has both bins and columns.  Segments, lw_i, the masks of gwi_set_draw_mask,
 * M, w_i = exp(lw_i - M) and the segment total S are gwi_draw_indices'.  For point k, segment s (the injection segment last), pair r and
 * bin b, with W_b the sum of w_i over the samples coded b:
 *   a_b = W_b / S                                  out[k][s][r][0][b]   (a sample coded 0xFFFF counts in S and in no bin)
 *   m_b = sum_{i in b} w_i y_i / W_b               out[k][s][r][1][b]
 *   v_b = sum_{i in b} w_i (y_i - m_b)^2 / W_b     out[k][s][r][2][b]
 * in two passes over the samples, the second centred on the m_b of the first.  Slot 0 has the bits gwi_weighted_histograms adds for this
 * one point onto a zeroed histogram of column cx.  A bin with W_b = 0 gives a_b = +0.0 and NaN for m_b and v_b: no error, no flag.  A
 * segment whose S is 0 or not finite gives NaN in all three slots and dead[k][s] = 1; the segments of a set that is not covered give NaN
 * (dead still tells whether they had weight).  k >= 1 is not bound by the batch limit: the points are staged on the device 64 at a time
 * and copied back per chunk.  Every sum has a fixed shape (sample order inside a tile of 1 024 and a bin, then tile order) and there are
 * no atomics: the bits are a pure function of (theta_k, codes, columns, masks, pairs), whatever the split of the points over calls, and
 * the call changes no state another entry reads.  Not done: sharded handles; more than 8 pairs or 512 (pair, bin)
 * items; two conditioning quantities at once.
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer, k < 1, n_pairs outside 1 ... 8, an index outside the bin columns
 * or the value columns, n_pairs n_bins > 512, a call before bins are set or before columns are set, no sample set covered by both, and a
 * host-only handle; GWI_ERR_UNSUPPORTED on a handle that holds a shard.
 *
 * gwi_point_conditional_times(): DIAGNOSTIC ONLY, for tools/post_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge / two mean launches together
 * and of the two variance launches, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_point_conditionals(gwi_handle h, const double* thetas, int32_t k, int32_t n_pairs, const int32_t* pairs /* [n_pairs][2] */,
                                  double* out /* [k][n_ev + 1][n_pairs][3][n_bins] */, int32_t* dead /* [k][n_ev + 1] */);
void gwi_point_conditional_times(double* logw_ms, double* mean_ms, double* var_ms, int32_t* launches);

/* Per-point rank (Spearman) correlations on the device: per hyper-parameter point and for each of two rank sets the weighted second
 * moments of the members' weighted mid-ranks -- a correlation that no monotone map of either quantity changes and no heavy tail
 * dominates (gwinferno_amd/csrc/gwi_rankcorr.h; the NumPy statement is gwinferno_amd/draws.py: rankcorr_codes,
 * point_rank_correlations_reference; the contract is DESIGN 8l).
 *
 * The sets: obs, all PE samples pooled (N = n_ev n_pe members, member i = sample i % n_pe of event i / n_pe), u_i = w_i / S_e with w, M,
 * S, the live rule and the masks of gwi_draw_indices and u_i = 0 for a sample of a dead event: the equal-weight mixture of the live
 * events' population-informed posteriors; det, the injections, u_j = exp(lw_j - M).
 *
 * gwi_set_rankcorr_columns(): what does not depend on theta, made by the host once.  Per set and column c, 1 <= n_cols <= 8: order[c]
 * is a permutation of the set's members along which the column's values do not decrease (a stable argsort); lt[c][i] and le[c][i] are
 * the numbers of members of the SAME set with a value below / at or below member i's, in [0, n] with lt <= position of i along the
 * order < le.  The arrays are checked (O(n)) and copied to HBM, and the entry's workspace is allocated here; no other setter's workspace
 * is touched, and a second call replaces the columns.
 *
 * gwi_point_rank_correlations(): with P[c][r] the sum of u over the first r members along order[c] and T_c = P[c][n],
 *   d_ci = ((P[c][lt_i] + P[c][le_i]) - T_c) / (2 T_c),   r_ci = 0.5 + d_ci
 * is the centred and the plain weighted mid-rank of member i in column c: ties share a rank, a column whose members all tie has d = 0
 * and r = 0.5 exactly.  For point k and set s (0 obs, 1 det), with I = 1 + C + C (C + 1) / 2 items:
 *   U    = sum_i u_i                          out[k][s][0]
 *   m_c  = sum_i u_i r_ci / U                 out[k][s][1 + c]         (0.5 in exact arithmetic: a self-check)
 *   R_cd = sum_i u_i d_ci d_di / U,  c <= d   out[k][s][1 + C + t], t counting the upper triangle row by row
 * Spearman's rho is R_cd / sqrt(R_cc R_dd) and is formed by the caller.  dead[k][0 ... n_ev] flags the segments whose S is 0 or not
 * finite, the injection set last (as gwi_point_moments), dead[k][n_ev + 1] the observed set, which is dead when no event is live; a dead
 * set gives NaN in every slot but U.  k >= 1 is not bound by the batch limit: the points are staged on the device 64 at a time and copied
 * back per chunk.  Every sum has a fixed shape and there are no atomics: the bits are a pure function of (theta_k, codes, masks),
 * whatever the split of the points over calls, and the call changes no state another entry reads.  Not done: sharded handles; per-event
 * rank correlations (each event's own order); Kendall's tau; more than 8 columns.
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer, k < 1, n_cols outside 1 ... 8, codes that fail a check, a call
 * before columns are set and a host-only handle; GWI_ERR_UNSUPPORTED on a handle that holds a shard, checked first.
 *
 * gwi_point_rankcorr_times(): DIAGNOSTIC ONLY, for tools/post_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge / tile-sum / offset / prefix
 * launches together and of the covariance and merge launches, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_set_rankcorr_columns(gwi_handle h, int32_t n_cols, const int32_t* order_obs /* [n_cols][n_ev n_pe] */, const int32_t* lt_obs, const int32_t* le_obs,
                                    const int32_t* order_det /* [n_cols][n_inj] */, const int32_t* lt_det, const int32_t* le_det);
gwi_status gwi_point_rank_correlations(gwi_handle h, const double* thetas, int32_t k, double* out /* [k][2][1 + C + C(C+1)/2] */, int32_t* dead /* [k][n_ev + 2] */);
void gwi_point_rankcorr_times(double* logw_ms, double* prefix_ms, double* cov_ms, int32_t* launches);

/* Per-point tails of the inner importance sums on the device: per hyper-parameter point and segment the m largest live log-weights,
 * what defines the cut-off below them and the sum of everything outside the tail -- all a Pareto fit of the largest weights (Vehtari
 * et al., Pareto smoothed importance sampling) needs, without the weights leaving HBM (gwinferno_amd/csrc/gwi_tail.h; the NumPy
 * statement is gwinferno_amd/draws.py: point_tails_reference; the fit is the host's, draws.pareto_tail_fit; the contract is DESIGN 8m).
 *
 * Segments (an event's n_pe samples; the injection set, last), the masks, M and S are gwi_draw_indices' and gwi_weighted_histograms'.
 * A sample is live when it is unmasked and l_j = lw_j + log_const is finite; l_j has the bits gwi_log_weights returns for the sample.
 *
 * gwi_set_tail_sizes(): the tail sizes of the events' segments and of the injection set, 1 <= m <= 4096, m_pe < n_pe, m_inj < n_inj.
 * Nothing is uploaded; a second call replaces the sizes.
 *
 * gwi_point_tails(): per point k and segment s with tail size m (the events' tails first, [n_ev][m_pe], then the injection set's):
 *   tail[m]    the m largest live l_j in ascending order, as the bits of the inputs; values compare as numbers, -0.0 and +0.0 tie and
 *              which of them appears is unspecified; with fewer than m live samples the live values sit at the top end, -inf in front
 *   v* = tail[0], the m-th largest
 *   counts[k][s] = (n_live, n_gt, n_eq, dead): the live samples, those > v*, those == v*, and 1 for a segment whose S is 0 or not finite
 *   stats[k][s]  = (M, S, body, below_max): below_max the largest live l_j < v* (-inf: none), body = sum over l_j < v* of exp(l_j - M)
 * The cut-off of the fit, the (m + 1)-th largest, is v* when n_gt + n_eq > m and below_max otherwise, and the sum of exp(l_j - M) over
 * everything outside the tail is body + (n_gt + n_eq - m) exp(v* - M): no subtraction.  A dead segment has an all -inf tail, zero counts,
 * below_max = -inf and NaN body.  The selection is an exact radix selection on order-preserving 64-bit keys followed by a sort of the
 * tail: tail, counts and below_max are the same bits on every call, handle and split of the points over calls; body is a sum of a fixed
 * shape (four consecutive samples per lane, butterfly, wave order, tile order) and so are its bits.  No floating-point atomics.  k >= 1
 * is not bound by the batch limit: the points are staged on the device 64 at a time and copied back per chunk; n_ev m_pe + m_inj +
 * 4 (n_ev + 1) doubles and 4 (n_ev + 1) ints come back per point.  The call changes no state another entry reads.  Not done: the fit on
 * the device; sharded handles; tails longer than 4096; smoothed weights fed back into the likelihood.
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer, k < 1, a tail size out of range or not below the segment's
 * length, a call before the sizes are set and a host-only handle; GWI_ERR_UNSUPPORTED on a handle that holds a shard, checked first.
 *
 * gwi_point_tail_times(): DIAGNOSTIC ONLY, for tools/post_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge launches with the twelve
 * selection launches and of the two collection launches, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_set_tail_sizes(gwi_handle h, int32_t m_pe, int32_t m_inj);
gwi_status gwi_point_tails(gwi_handle h, const double* thetas, int32_t k, double* tail /* [k][n_ev * m_pe + m_inj] */,
                           double* stats /* [k][n_ev + 1][4]: max, S, body, below_max */, int32_t* counts /* [k][n_ev + 1][4]: n_live, n_gt, n_eq, dead */);
void gwi_point_tail_times(double* logw_ms, double* select_ms, double* collect_ms, int32_t* launches); /* diagnostic only */

/* Bootstrap replicates of the inner importance sums on the device: per hyper-parameter point and segment the sums of B Poisson-bootstrap
 * replicates of the segment's samples, with the SAME resampling at every point (common random numbers), so that the sampling noise of
 * a difference log L(theta_a) - log L(theta_b) and the bias of the logarithm follow on the host while the weights never leave HBM
 * (gwinferno_amd/csrc/gwi_boot.h; the NumPy statement is gwinferno_amd/draws.py: bootstrap_counts, point_bootstrap_reference; the
 * replicates of the likelihood are the host's, draws.bootstrap_likelihood; the contract is DESIGN 8n).
 *
 * Segments (an event's n_pe samples; the injection set, last), the masks, M and S are gwi_draw_indices' and gwi_weighted_histograms'.
 * w_i = exp(lw_i - M), 0 for a sample that is masked or whose log-weight is not finite.  Sample i of a segment has the global index
 * e n_pe + j (PE sample j of event e) or n_ev n_pe + j (injection j).  In replicate b it is taken c_ib times, c_ib ~ Poisson(1): word
 * b % 4 of the Philox4x32-10 block with the key (seed low, seed high) and the counter (index low, index high, b / 4, 0x424F4F54), and
 * c_ib = the number of entries of the table floor(2^32 F(j)), j = 0 ... 12 (F the Poisson(1) CDF), that are <= the word.  Integer
 * comparisons only: a count is the same bits on host and device and depends on (seed, index, b) alone, never on the point.
 *
 * gwi_set_bootstrap(): the seed, the number of replicates of a call, 1 <= n_replicates <= 1024, and the first one,
 * first_replicate >= 0, first_replicate + n_replicates <= 2^20.  Nothing is uploaded; a second call replaces the setting.
 *
 * gwi_point_bootstrap(): per point k, segment s and replicate b = first_replicate + r
 *   sums[k][s][r]   A_b = sum_i c_ib w_i over the segment
 *   stats[k][s]     (M, S), the bits gwi_point_tails returns
 *   dead[k][s]      1 for a segment whose S is 0 or not finite: its sums are NaN
 *   counts[s][r]    C_b = sum_i c_ib over the segment's unmasked samples, whether or not their weight is finite: exact, the same at
 *                   every point, returned once per call
 * A_b is a sum of ONE shape -- sample order within a slice of 128 consecutive samples of a tile, the tile's 8 slices in order, the
 * segment's tiles in order -- that involves neither n_replicates nor first_replicate: the bits of A_b are the same on every call,
 * handle and split of the points or of the replicates over calls.  No atomics.  k >= 1 is not bound by the batch limit: the points are
 * staged on the device 64 at a time and copied back per chunk; (n_ev + 1)(B + 2) doubles and n_ev + 1 ints come back per point.  The
 * call changes no state another entry reads.  Not done: sharded handles; replicates of the gradient; the Bayesian (exponential-weight)
 * bootstrap; replicates of the marginalised-selection term and of the cuts; more than 1024 replicates per call; feeding anything back
 * into the likelihood.
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer, k < 1, a setting out of range, a call before the setting and a
 * host-only handle; GWI_ERR_UNSUPPORTED on a handle that holds a shard, checked first.
 *
 * gwi_point_bootstrap_times(): DIAGNOSTIC ONLY, for tools/post_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge launches with the tile
 * launch and of the merge launch, and the number of kernel launches after the log-weight passes. */
gwi_status gwi_set_bootstrap(gwi_handle h, uint64_t seed, int32_t n_replicates, int32_t first_replicate);
gwi_status gwi_point_bootstrap(gwi_handle h, const double* thetas, int32_t k, double* sums /* [k][n_ev + 1][B] */, double* stats /* [k][n_ev + 1][2]: M, S */,
                               int32_t* dead /* [k][n_ev + 1] */, int64_t* counts /* [n_ev + 1][B] */);
void gwi_point_bootstrap_times(double* logw_ms, double* tile_ms, double* merge_ms, int32_t* launches); /* diagnostic only */

/* Per-point joint (two-dimensional) histograms on the device: per hyper-parameter point, segment and pair (cx, cy) of the bin columns of
 * gwi_set_histogram_bins the B x B table of weight shares -- what Pearson's rho (gwi_point_moments), the conditional moments
 * (gwi_point_conditionals) and Spearman's rho (gwi_point_rank_correlations) each compress to a number or two per pair, and the only
 * object that shows a dependence that is neither linear nor monotone (gwinferno_amd/csrc/gwi_hist2d.h; the NumPy statement is
 * gwinferno_amd/draws.py: point_histograms2d_reference; the contract is DESIGN 8o).
 *
 * gwi_point_histograms2d(): pairs[r] = (cx, cy), both bin columns of gwi_set_histogram_bins, read where they lie: nothing is uploaded
 * and there is no setter of this entry's own.  1 <= n_pairs <= 8; the bins must have been set with n_bins = B <= 64 (this entry alone
 * refuses more; the other entries keep their 256).  Segments, lw_i, the masks of gwi_set_draw_mask, M, w_i = exp(lw_i - M) and the
 * segment total S are gwi_draw_indices'.  For point k, segment s (the injection segment last), pair r and cell (bx, by)
 *   q_s[r][bx][by] = (sum of w_i over the samples coded bx in column cx and by in column cy) / S
 * (a sample coded 0xFFFF in either column counts in S and in no cell).  Per point come back
 *   obs[k][r][bx][by]    (sum of q_e over the live events e, in event order) / n_live_events   NaN without a live event or PE bins
 *   pred[k][r][bx][by]   q of the injection segment                                           NaN when it is dead or has no bins
 *   live[k]              (n_live_events, 1 if the injection segment is live else 0)
 * and, onto the caller's running sums (in/out, as gwi_weighted_histograms'; each may be NULL: not kept),
 *   hist_pe[e][r] += v q_e   hist_inj[r] += v q_inj   n_dead[s] += 1 for a dead segment   vsum[s] += v for a live one (with v only)
 * with v[k][s] in [0, 1] the point's linear weight of the segment, or v = NULL for 1 everywhere.  The quotient is formed as without
 * weights and then multiplied in a product of its own: v = 1 gives the bits of v = NULL; v = 0 touches nothing of the segment's sums,
 * n_dead included.  obs, pred and live do not depend on v.  A segment whose S is 0 or not finite is dead: it adds nothing and is left
 * out of obs.  Every sum has a fixed shape (sample order inside a tile of 1 024 and a cell, then tile order, then event order for obs,
 * then point order for the running sums) and there are no atomics: the bits are a pure function of (theta_k, codes, masks, pairs, v),
 * whatever the split of the points over calls or the other pairs of the call; a pair (c, c) has gwi_weighted_histograms' bits for
 * column c on its diagonal and exact zeros off it.  k >= 1 is not bound by the batch limit: the points are staged on the device 64 at a
 * time; 2 n_pairs B B doubles and two ints come back per point.  The call changes no state another entry reads.  Not done: sharded
 * handles; more than 64 bins per axis or 8 pairs; different bin counts per axis; three-way tables; per-event tables per point.
 * GWI_ERR_INVALID (with a gwi_last_error message) for a null pointer among thetas, pairs, obs, pred and live, k < 1, n_pairs outside
 * 1 ... 8, a column index outside the bin columns, bins set with more than 64 bins, a v outside [0, 1] or NaN, a call before bins are
 * set, and a host-only handle; GWI_ERR_UNSUPPORTED on a handle that holds a shard.
 *
 * gwi_point_hist2d_times(): DIAGNOSTIC ONLY, for tools/post_time.py: of the calling thread's last call, summed over its points, the
 * wall time of the (blocking) log-weight passes, the device times (HIP events) of the draw tile / draw merge launches with the first
 * pair's tile launch and of everything after it (the first pair's merge and mix launches, then the other pairs' three launches), and
 * the number of kernel launches after the log-weight passes (2 + 3 n_pairs per point). */
gwi_status gwi_point_histograms2d(gwi_handle h, const double* thetas, int32_t k, int32_t n_pairs, const int32_t* pairs /* [n_pairs][2] */,
                                  const double* v /* [k][n_ev + 1] or NULL */, double* hist_pe /* in/out [n_ev][n_pairs][B][B] or NULL */,
                                  double* hist_inj /* in/out [n_pairs][B][B] or NULL */, double* obs /* [k][n_pairs][B][B] */, double* pred /* like obs */,
                                  int32_t* live /* [k][2]: live events, injection set live */, int32_t* n_dead /* in/out [n_ev + 1] or NULL */,
                                  double* vsum /* in/out [n_ev + 1] or NULL */);
void gwi_point_hist2d_times(double* logw_ms, double* tile_ms, double* merge_ms, int32_t* launches); /* diagnostic only */

/* Credible intervals of the population-informed event posteriors on the device: the marginal posterior weight of every sample, and
 * weighted quantiles and moments of any quantity under it (gwinferno_amd/csrc/gwi_quant.h; the NumPy statement is
 * gwinferno_amd/draws.py: marginal_weights_reference, weighted_quantiles_reference).
 *
 * Segments, lw_i, the masks, M, w_i = exp(lw_i - M) and the segment total S are gwi_draw_indices' and gwi_weighted_histograms'.
 * Marginal weights: W_i += w_i / S, one point after another in the order of the call -- one running double per sample in HBM,
 * n_ev n_pe + n_inj of them.  A segment whose S is 0 or not finite adds nothing; dead[segment] is incremented instead (segment n_ev
 * is the injection set).  n_points counts the points added.  W, dead and n_points are state of the handle: zero at creation and
 * after gwi_marginal_weights_reset(), released with the handle; they do not depend on any quantile column (one accumulation serves
 * any number of column sets) and changing the draw mask does NOT reset them: a mask applies to the points added while it is set.
 *
 * Quantile columns: 1 <= n_cols <= 8 quantities.  Quantity c supplies its values x_pe[c][n_ev][n_pe] and / or x_inj[c][n_inj] and
 * per segment a sort order, an int32 permutation of the segment's sample indices along which the values do not decrease
 * (order_pe[c][n_ev][n_pe], order_inj[c][n_inj]).  The library does not sort: ties are in the caller's order.  Either set may be
 * NULL (it is then left out), not both.  Values and orders are checked on the host and copied to HBM once; a new call replaces them.
 *
 * Quantile of level p in [0, 1], rule "inverted CDF": with C_r the inclusive prefix of W along the order and C_last the last prefix,
 * the sample at the smallest rank r with C_r >= p C_last and W > 0 at that rank; the last rank with weight when rounding runs past
 * the end; -1 when the segment has no weight.  p = 0 is the smallest value with weight, p = 1 the largest.  The entry returns the
 * sample's index within its segment.  Moments, per (segment, column), summed along the order: m1 = sum W_i x_i, m2 = sum W_i x_i^2;
 * mass[segment] = C_last (of column 0's order), so that mean = m1 / mass and variance = m2 / mass - mean^2.
 *
 * Every sum has a fixed shape -- rank order inside a tile of 1 024 ranks, then tile order, then, for W, point order on one stream --
 * and there are no atomics: the bits of W, of the indices and of the moments are a pure function of the arguments and of the order
 * of the points.  A request split over calls (2 + 1, 1 + 1 + 1) gives the bits of one call; two handles of one model give the same.
 *
 * gwi_marginal_weights_add(): adds the k >= 0 points thetas[k][n_theta]; k is not bound by the batch limit.
 * gwi_marginal_weights_add_weighted(): the same with a linear weight per (point, segment), v[k][n_ev + 1] in [0, 1] (segment n_ev is
 * the injection set), uploaded once per call: W_i += v (w_i / S) -- the quotient is formed as without weights and then multiplied by v
 * in a product of its own, so v = 1 gives the bits of gwi_marginal_weights_add().  Two more running doubles per segment are state of
 * the handle beside dead: vsum[segment] += v and vsum2[segment] += v v at every point at which the segment is live, in point order
 * (gwi_marginal_weights_add() counts v = 1: after unweighted points alone vsum == n_points - dead exactly).  A point whose v is 0 adds
 * nothing to W, vsum or vsum2, is counted in n_points and does not touch dead.  Weighted and unweighted calls may be mixed;
 * gwi_marginal_weights_reset() zeroes vsum and vsum2 too.  Quantiles and densities normalise by the segment's sum of W and need no
 * weights of their own.  (vsum)^2 / vsum2 is the effective number of points of the segment.
 * gwi_marginal_point_weights(): copies vsum[n_ev + 1] and vsum2[n_ev + 1] back.
 * gwi_marginal_weights_read(): copies W (pe_w[n_ev][n_pe] and inj_w[n_inj]; either may be NULL), dead[n_ev + 1] and n_points back:
 * 8 bytes per sample, whatever the number of points.
 * gwi_weighted_quantiles(): 1 <= n_levels <= 32 levels; idx_pe[n_ev][n_cols][n_levels] and moments_pe[n_ev][n_cols][2] (ignored
 * without PE columns), idx_inj[n_cols][n_levels] and moments_inj[n_cols][2] (ignored without injection columns), mass[n_ev + 1]
 * (0 for a set that is left out).  With nothing accumulated every index is -1 and mass is 0.
 * GWI_ERR_INVALID (with a gwi_last_error message) for null pointers, k < 0, n_cols outside 1 ... 8, n_levels outside 1 ... 32, a level
 * that is NaN or outside [0, 1], an order that is no permutation of its segment, values that are not finite or decrease along the
 * order, a quantile call before the columns are set, a null v, an entry of v that is NaN, negative or above 1, and a host-only
 * handle; GWI_ERR_UNSUPPORTED on a handle that holds a shard, as gwi_draw_indices.
 *
 * gwi_quantile_times(): DIAGNOSTIC ONLY, for tools/weighted_quantiles_time.py: of the calling thread's last gwi_marginal_weights_add(_weighted),
 * summed over its points, the wall time of the (blocking) log-weight passes and the device time (HIP events) of the draw tile / draw
 * merge / marginal add launches; the device time of the calling thread's last gwi_weighted_quantiles (its three launches); and the
 * number of kernel launches of the last of the two calls. */
gwi_status gwi_marginal_weights_reset(gwi_handle h);
gwi_status gwi_marginal_weights_add(gwi_handle h, const double* thetas, int32_t k);
gwi_status gwi_marginal_weights_add_weighted(gwi_handle h, const double* thetas, int32_t k, const double* v /* [k][n_ev + 1] */);
gwi_status gwi_marginal_point_weights(gwi_handle h, double* vsum /* [n_ev + 1] */, double* vsum2 /* [n_ev + 1] */);
gwi_status gwi_marginal_weights_read(gwi_handle h, double* pe_w /* [n_ev][n_pe] or NULL */, double* inj_w /* [n_inj] or NULL */, int32_t* dead /* [n_ev + 1] */,
                                     int64_t* n_points);
gwi_status gwi_set_quantile_columns(gwi_handle h, int32_t n_cols, const double* x_pe /* [n_cols][n_ev][n_pe] or NULL */, const int32_t* order_pe /* like x_pe */,
                                    const double* x_inj /* [n_cols][n_inj] or NULL */, const int32_t* order_inj /* like x_inj */);
gwi_status gwi_weighted_quantiles(gwi_handle h, const double* levels, int32_t n_levels, int32_t* idx_pe /* [n_ev][n_cols][n_levels] */,
                                  int32_t* idx_inj /* [n_cols][n_levels] */, double* moments_pe /* [n_ev][n_cols][2] */, double* moments_inj /* [n_cols][2] */,
                                  double* mass /* [n_ev + 1] */);
void gwi_quantile_times(double* logw_ms, double* add_ms, double* query_ms, int32_t* launches);

/* Smooth densities of the population-informed event posteriors on the device: a weighted Gaussian kernel density estimate of the
 * marginal weights W that gwi_marginal_weights_add accumulated, per segment (an event's n_pe samples, or the injection set: segment
 * n_ev), per quantity in one dimension and per pair of quantities in two, on the caller's grid points (gwinferno_amd/csrc/gwi_kde.h;
 * the NumPy statement is gwinferno_amd/draws.py: weighted_kde_reference, weighted_kde2d_reference; the contract is DESIGN 8e).  One
 * accumulation serves quantiles, 1-D and 2-D densities and any number of column sets.
 *
 * Bandwidth: scipy.stats.gaussian_kde(weights=...)'s.  With p_i = W_i / sum W over the segment: s2 = sum p_i^2, n_eff = 1 / s2, the
 * mean sum p_i x_i, and the covariance sum p_i (x_i - mean)(y_i - mean_y) / (1 - s2), centred on the mean of a first pass.  The
 * factor is f = n_eff^(-1/(d+4)) (rule 0, Scott) or (n_eff (d+2)/4)^(-1/(d+4)) (rule 1, Silverman), times scale > 0.
 * 1-D: h^2 = var f^2, rho(g) = sum_i p_i exp(-(g - x_i)^2 / 2h^2) / sqrt(2 pi h^2).  A column may have reflecting bounds lo, hi
 * (bounds[c] = {lo, hi}; NaN: none; bounds NULL: none at all): the images 2 lo - x_i and 2 hi - x_i are added for grid points inside
 * [lo, hi], points outside get 0, and the bandwidth is that of the unreflected data.
 * 2-D: H = f^2 Cov (the full 2 x 2 matrix), rho(gx, gy) = sum_i p_i exp(-d^T H^-1 d / 2) / (2 pi sqrt|H|) on the tensor grid
 * gridx[pair] x gridy[pair]; no reflection.
 * Grid points must be finite; they need not be uniform or sorted.  1 <= n_cols <= 8, 1 <= n_grid <= 1024, 1 <= n_pairs <= 4,
 * 1 <= n_gx, n_gy <= 128.
 *
 * A segment without weight gives NaN, neff = 0 and no flag (so does every segment when nothing is accumulated).  A segment with fewer
 * than two samples of positive weight, or whose variance (|H|) is not > 0 and finite, gives NaN and degenerate = 1.  bw holds h
 * (cov: Hxx, Hxy, Hyy), NaN where there is no curve.  A set without columns is left out: its outputs are not written (bw NaN, neff 0).
 *
 * The value at a grid point is a pure function of the point, the segment's W and values and the rule: every sum has a fixed shape
 * (sample order inside a tile of 1 024 samples, then tile order) and there are no atomics.  A grid split over calls gives the bits
 * of one call, point by point; so do two calls, two handles of one model, and the same W however it was accumulated.
 *
 * gwi_set_kde_columns(): the values (finite: checked on the host) are copied to HBM once; a new call replaces them.  Either set may be
 * NULL (it is then left out), not both.  No sort order is needed.
 * GWI_ERR_INVALID (with a gwi_last_error message) for null pointers, counts outside the limits, a value or grid point that is not
 * finite, a bound that is infinite or lo >= hi, scale not > 0, an unknown rule, a pair index outside the columns, a call before the
 * columns are set and a host-only handle; GWI_ERR_UNSUPPORTED on a handle that holds a shard, as gwi_weighted_quantiles.
 *
 * gwi_kde_times(): DIAGNOSTIC ONLY, for tools/weighted_kde_time.py: of the calling thread's last density query the device time (HIP
 * events) of the four statistics launches and of the evaluation and sum launches, the wall time of the copies to the host, and the
 * number of kernel launches. */
gwi_status gwi_set_kde_columns(gwi_handle h, int32_t n_cols, const double* x_pe /* [n_cols][n_ev][n_pe] or NULL */, const double* x_inj /* [n_cols][n_inj] or NULL */,
                               const double* bounds /* [n_cols][2], NaN = none; or NULL */);
gwi_status gwi_weighted_kde(gwi_handle h, const double* grid /* [n_cols][n_grid] */, int32_t n_grid, int32_t rule, double scale, double* rho_pe /* [n_ev][n_cols][n_grid] */,
                            double* rho_inj /* [n_cols][n_grid] */, double* bw /* [n_ev + 1][n_cols]: h */, double* neff /* [n_ev + 1] */,
                            int32_t* degenerate /* [n_ev + 1][n_cols] */);
gwi_status gwi_weighted_kde2d(gwi_handle h, const int32_t* pairs /* [n_pairs][2] column indices */, int32_t n_pairs, const double* gridx /* [n_pairs][n_gx] */, int32_t n_gx,
                              const double* gridy /* [n_pairs][n_gy] */, int32_t n_gy, int32_t rule, double scale, double* rho_pe /* [n_ev][n_pairs][n_gx][n_gy] */,
                              double* rho_inj /* [n_pairs][n_gx][n_gy] */, double* cov /* [n_ev + 1][n_pairs][3]: H */, double* neff /* [n_ev + 1] */,
                              int32_t* degenerate /* [n_ev + 1][n_pairs] */);
void gwi_kde_times(double* stats_ms, double* eval_ms, double* copy_ms, int32_t* launches);

/* Effective-spin catalogs (gwinferno_amd/csrc/gwi_spinprior.h; the NumPy statement is gwinferno_amd/spin_priors.py).  Stand-alone
 * entries like gwi_ingest_columns: no handle, host pointers in and out, their own stream and buffers on `device` (negative: the
 * calling thread's current device).  The calling thread's current device is the same after the call as before it.
 *
 * gwi_effective_spins(): per sample, from the component spins (q, a_1, a_2, cos tilt_1, cos tilt_2) --
 *   chi_eff = (a1 ct1 + q a2 ct2) / (1 + q)  and  chi_p = max(a1 sin t1, (3 + 4q) / (4 + 3q) q a2 sin t2)   (preprocess/conversions.py:8-62);
 *   p_chi_eff_iso     = p(chi_eff | q) for uniform, isotropic spins with magnitudes below a_max (Callister, arXiv:2104.09508;
 *                       preprocess/priors.py:79-196): the closed form at chi_eff = 0, the five open cases, 0 for |chi_eff| >= a_max, and
 *                       for a value exactly on a case boundary the mean of the form at |chi_eff| +- 1e-6;
 *   p_chi_eff_aligned = the same for aligned spins (priors.py:38-76);   p_chi_p_iso = p(chi_p | q) (priors.py:199-244);
 * each evaluated at the sample's own chi_eff / chi_p.  Any output may be NULL.  A sample with a NaN, q <= 0 or |cos tilt| > 1 yields
 * NaN in every output.  n = 0 is GWI_OK and writes nothing.
 *
 * gwi_chi_p_conditional_prior(): p(chi_p | chi_eff, q) by the estimator of priors.py:288-333 with a counter-based generator and
 * bounded rejection.  Slot d of sample s (catalog index first_index + s) tries attempts t = 0, 1, ... < max_attempts; attempt t draws
 * a1 = a_max u0, a2 = a_max u1, cos t2 = 2 u2 - 1 from Philox4x32-10 with key = seed (low word, high word) and counters
 * (index low, index high, d, 2t) -> (u0: words 0,1; u1: words 2,3) and (.., 2t + 1) -> (u2: words 0,1), a uniform being
 * ((hi >> 5) 2^26 + (lo >> 6)) 2^-53; it is kept when |cos t1| <= 1 for cos t1 = (chi_eff (1 + q) - q a2 cos t2) / a1.  The slot's
 * draw is the chi_p of its first kept attempt with weight (1 + q) / a1; a slot without one carries no weight.  accepted[s] counts the
 * filled slots; with none, p[s] = NaN.  The density is scipy.stats.gaussian_kde's weighted Gaussian KDE of the draws (Scott's factor
 * n_eff^(-1/5), n_eff = 1 / sum w^2 of the normalised weights, variance with the 1 / (1 - sum w^2) correction) on the 50 points from
 * 0.05 to 0.95 max_chi_p, zeros added at 0 and max_chi_p, normalised by the trapezoid rule, interpolated linearly at chi_p.  The
 * values depend on (seed, first_index + s) only -- not on how a catalog is cut into calls -- and on nothing that varies between runs.
 * n is cut into launches sized by the worst case, every slot using all max_attempts attempts (n_draws (50 + 8 max_attempts) units
 * per sample against a budget of 4.6e10), so a larger max_attempts means smaller launches, not longer ones.
 * GWI_ERR_INVALID for n_draws < 2, max_attempts < 1 or > 65536, first_index < 0 or a null pointer with n > 0.
 *
 * gwi_spin_prior_times(): DIAGNOSTIC ONLY, for tools/effective_spins_time.py -- not part of the catalog interface, and nothing in the
 * package depends on it.  Device time of the calling thread's last call of either entry (HIP events around the launches): the total,
 * the longest single launch and the number of launches. */
gwi_status gwi_effective_spins(int64_t n, const double* q, const double* a1, const double* a2, const double* ct1, const double* ct2, double a_max, double* chi_eff,
                               double* chi_p, double* p_chi_eff_iso, double* p_chi_eff_aligned, double* p_chi_p_iso, int32_t device);
gwi_status gwi_chi_p_conditional_prior(int64_t n, const double* chi_p, const double* chi_eff, const double* q, double a_max, int32_t n_draws, int32_t max_attempts,
                                       uint64_t seed, int64_t first_index, double* p, int32_t* accepted, int32_t device);
void gwi_spin_prior_times(double* total_ms, double* max_launch_ms, int32_t* launches);

/* Population draws (gwinferno_amd/csrc/gwi_popdraw.h; the NumPy statement is gwinferno_amd/population_draws.py): fair draws from
 * tabulated 1-D densities.  Stand-alone like gwi_effective_spins: no handle, host pointers in and out, its own stream and buffers on
 * `device` (negative: the calling thread's current device), which is the thread's current device again after the call.
 *
 * Table t is the unnormalised density pdf[t][0..n_grid) on the uniform grid lo[t] ... hi[t], read as piecewise linear: cell c has mass
 * m_c = (p_c + p_{c+1}) dx / 2, dx = (hi - lo) / (n_grid - 1), and C_c is the inclusive prefix of the masses (a block scan of fixed
 * shape: the same bits on every call).  Draw j of table t takes one Philox4x32-10 block with key = seed (low word, high word) and counter
 * (index low, index high, t, 0x504F5044), index = first_index + j; u = words 0,1 and v = words 2,3, a uniform being
 * ((hi >> 5) 2^26 + (lo >> 6)) 2^-53.  Without `lower` the target is u C_last; a binary search finds a cell whose prefix exceeds it and
 * whose predecessor's does not, a cell without mass is passed over for the next one with mass, a target past the end takes the last
 * cell with mass, and with r the target's excess over the preceding prefix, s = (p_{c+1} - p_c) / dx:
 *   x = x_c + 2 r / (p_c + sqrt(p_c^2 + 2 s r)),  clamped into the cell.
 * With lower[t][j] the draw comes from the density restricted to x >= lower and renormalised: C(lower) = the prefix up to lower's cell
 * plus that cell's partial trapezoid, the target is C(lower) + u (C_last - C(lower)), mass[t][j] = 1 - C(lower) / C_last is the
 * probability the restriction keeps and accept[t][j] = (v < mass) as one byte -- thinning the draws of another factor by `accept` samples
 * a product under the constraint exactly, with no rejection loop.  lower <= lo is no bound (mass 1, accept 1); when no mass lies at or
 * above lower: x = min(max(lower, lo), hi), mass 0, accept 0; a NaN bound: x = mass = NaN, accept 0.  mass and accept may be NULL, and
 * are 1 without `lower`.  x, mass, accept and lower are [n_tables][n_draws].  The call is cut into launches of at most 2^20 draws per
 * table; a draw depends on (tables, seed, t, first_index + j) only, not on the cut or on how a request is split over calls.
 *
 * Checked on the host before anything is uploaded, each GWI_ERR_INVALID with a message (gwi_table_draws_error(), of the calling
 * thread's last call) naming the first offending table: n_grid < 2 (or > 4096: a table is staged in LDS), hi <= lo, a negative or
 * non-finite density entry, a table whose total mass is 0.  Without a gfx950 device: GWI_ERR_NO_DEVICE -- there is no CPU fallback.
 *
 * gwi_table_draws_times(): DIAGNOSTIC ONLY, for tools/population_draws_time.py: device time (HIP events) of the calling thread's last
 * call -- the prefix kernel, the draw launches together, and their number. */
gwi_status gwi_table_draws(int32_t device, int32_t n_tables, int32_t n_grid, const double* lo, const double* hi, const double* pdf /* [n_tables][n_grid] */,
                           int64_t n_draws, uint64_t seed, uint64_t first_index, const double* lower /* [n_tables][n_draws] or NULL */,
                           double* x /* [n_tables][n_draws] */, double* mass /* or NULL */, unsigned char* accept /* or NULL */);
const char* gwi_table_draws_error(void);
void gwi_table_draws_times(double* cdf_ms, double* draw_ms, int32_t* launches);

/* Mock catalogs (gwinferno_amd/csrc/gwi_mock.h; the NumPy statement is gwinferno_amd/mock_catalog.py; the model is DESIGN.md's section
 * "Mock catalogs"): noisy data and detection of true sources, and the posterior samples of detected events.  Stand-alone like
 * gwi_table_draws: no handle, host pointers in and out, own stream and buffers on `device` (negative: the calling thread's current
 * device), which is the thread's current device again after the call.
 *
 * A source has n_coords <= 8 coordinates; coordinate c has a transform T_c (is_log[c] != 0: log, else identity), a noise scale sigma[c]
 * in T-space and a support [lo[c], hi[c]] in natural units.
 *
 * gwi_mock_observe: data[c][j] = T_c(x_true[c][j]) + sigma[c] n with n standard normal.  From the data, m1_d, q_d, z_d = T^-1 of the
 * coordinates i_m1, i_q, i_z; Mc = m1_d (1 + z_d) q_d^(3/5) / (1 + q_d)^(1/5); snr = rho_ref (Mc / mc_ref)^(5/6) dl_ref / DL(z_d) with
 * detection = {rho_ref, mc_ref, dl_ref, rho_th} and DL by linear interpolation (numpy.interp's form) in (table_z, table_dl);
 * found[j] = (m1_d > 0 and q_d > 0 and z_d > 0 and snr >= rho_th) as one byte.  snr = 0 where a detector-frame quantity is not positive
 * or z_d lies past the table's end; NaN true parameters give NaN data, NaN snr and found = 0.
 *
 * gwi_mock_posteriors: x[c][e][s], sample s of event e, from the normal centred on data[c][e] with scale sigma[c] truncated to
 * [T_c(lo), T_c(hi)] -- the posterior under a prior flat in T_c(x) -- by inverse CDF from one uniform, mapped back with T^-1 and clamped
 * into [lo, hi]; prior[e][s] = prod_c |T_c'(x_c)| / (T_c(hi_c) - T_c(lo_c)), i.e. 1 / (x ln(hi / lo)) per log coordinate.  Data that
 * are not finite give NaN samples and a NaN prior.
 *
 * Generator: Philox4x32-10 with key = seed (low word, high word); a coordinate takes one uniform ((hi >> 5) 2^26 + (lo >> 6)) 2^-53, so
 * block b serves coordinates 2 b (words 0, 1) and 2 b + 1 (words 2, 3).  Counter (index low, index high, 0, 0x4D4F4B00 + b) with
 * index = first_index + j for the data; (index low, index high, s, 0x4D4F4B10 + b) with index = first_event + e for the samples.  Word 3
 * is disjoint from the other entries' (0x504F5044, 0x52534D50, 2 * attempt (+ 1) < 2^17).  The normal is -sqrt2 erfcinv(2 u) for
 * u <= 1/2 (u = 0 read as 2^-54), else +sqrt2 erfcinv(2 (1 - u)).  The truncated normal with standardised bounds a, b: a > 0 is mirrored
 * (a, b, u) -> (-b, -a, 1 - u); b <= 0: y = -sqrt2 erfcinv(2 (Phi(a) + u (Phi(b) - Phi(a)))); else Z = 1 - Phi(a) - Q(b) and
 * y = -sqrt2 erfcinv(2 (Phi(a) + u Z)) while that argument is <= 1, else y = +sqrt2 erfcinv(2 (Q(b) + (1 - u) Z)); Phi and Q come from
 * erfc of a non-negative argument and erfcinv never sees an argument above 1.  A value is a pure function of (inputs, seed, stream
 * index, sample index, coordinate): requests are cut into launches of at most 2^20 lanes, and neither the cut nor a split of a request
 * over calls (first_index / first_event) changes a value.
 *
 * Checked on the host before anything is uploaded, each GWI_ERR_INVALID with a message (gwi_mock_error(), of the calling thread's last
 * call): n_coords outside 1 ... 8, sigma <= 0 or not finite, hi <= lo, a log coordinate with lo <= 0, a role index out of range (or two
 * equal), detection parameters that are not positive and finite, a DL table that is not ascending or does not cover
 * [0, T^-1(T(hi_z) + 9 sigma_z)], null pointers.  Without a gfx950 device: GWI_ERR_NO_DEVICE -- there is no CPU fallback.
 *
 * gwi_mock_times(): DIAGNOSTIC ONLY, for tools/mock_catalog_time.py: device time (HIP events) of the calling thread's last call -- the
 * observe launches, the posterior launches, and their number. */
gwi_status gwi_mock_observe(int32_t device, int32_t n_coords, const int32_t* is_log, const double* sigma, const double* lo, const double* hi, int32_t i_m1, int32_t i_q,
                            int32_t i_z, const double* detection /* [4] */, int32_t n_table, const double* table_z, const double* table_dl, int64_t n,
                            const double* x_true /* [n_coords][n] */, uint64_t seed, uint64_t first_index, double* data /* [n_coords][n] */, double* snr /* [n] */,
                            unsigned char* found /* [n] */);
gwi_status gwi_mock_posteriors(int32_t device, int32_t n_coords, const int32_t* is_log, const double* sigma, const double* lo, const double* hi, int64_t n_ev, int64_t n_pe,
                               const double* data /* [n_coords][n_ev] */, uint64_t seed, uint64_t first_event, double* x /* [n_coords][n_ev][n_pe] */,
                               double* prior /* [n_ev][n_pe] */);
const char* gwi_mock_error(void);
void gwi_mock_times(double* observe_ms, double* posterior_ms, int32_t* launches);

/* Multi-GPU (one process per GPU): each rank's engine holds a contiguous block of events and a
 * slice of the injections.  gwi_eval_partial() runs the scan and leaves this rank's partial
 * record (gwi_partial_len() doubles) in `record`; the caller exchanges records (RCCL all-gather
 * over xGMI) and every rank calls gwi_combine() on the gathered buffer. */
int64_t gwi_partial_len(gwi_handle h);
gwi_status gwi_eval_partial(gwi_handle h, const double* theta, double* record_host, double* log_bfs,
                            double* log_neffs, double* variances);
/* Host-only: recompute the sample-independent constants of `theta` that gwi_combine folds in
 * (gwi_eval_partial does this implicitly). */
gwi_status gwi_prepare_combine(gwi_handle h, const double* theta);
gwi_status gwi_combine(gwi_handle h, const double* records, int32_t n_ranks, const gwi_options* opt,
                       gwi_summary* summary, double* grad, double* norms);

/* In-engine collective (one process per GPU, RCCL over xGMI).  gwi_comm_unique_id() fills 128 bytes
 * on ONE rank (ncclGetUniqueId); the caller distributes them (any out-of-band channel) and every rank
 * calls gwi_comm_init().  `rccl_path` names the librccl to dlopen (NULL: "librccl.so.1").  Afterwards
 * gwi_eval_sharded() == gwi_eval_partial + ncclAllGather of the records on the engine's own stream +
 * gwi_combine, with no host round trip between the scan and the exchange; log_bfs / log_neffs /
 * variances are this rank's events. */
gwi_status gwi_comm_unique_id(const char* rccl_path, void* id128);
gwi_status gwi_comm_init(gwi_handle h, const char* rccl_path, const void* id128, int32_t rank, int32_t world);
gwi_status gwi_eval_sharded(gwi_handle h, const double* theta, const gwi_options* opt, gwi_summary* summary,
                            double* grad, double* log_bfs, double* log_neffs, double* variances, double* norms);

/* Single-node exchange without a collective launch: the ranks of ONE node publish their partial records into a POSIX
 * shared-memory segment (`name`, created by whichever rank gets there first; unlink it with gwi_shm_comm_unlink once every
 * rank has attached) and poll each other's sequence stamps -- the records are ~1 KiB and already end up in host memory, so
 * the exchange costs a few cache-line transfers between host cores instead of a collective's launch + small-message latency.
 * After gwi_shm_comm_init(), gwi_eval_sharded() evaluates this rank's shard through the engine's regular (AQL) fast path
 * and exchanges through the segment; it takes precedence over a communicator set up with gwi_comm_init().  Works on
 * host-only handles too (gwi_shm_exchange with caller-made records: the CPU test-suite).  Every rank must issue the same
 * sequence of exchanges.  Same partitioning contract as above (pipeline/analysis.py:78-86, :126-134). */
gwi_status gwi_shm_comm_init(gwi_handle h, const char* name, int32_t rank, int32_t world);
gwi_status gwi_shm_comm_unlink(const char* name);
/* publish `record` (gwi_partial_len() doubles) as this rank's, wait for every rank's, copy them to gathered[world][len] */
gwi_status gwi_shm_exchange(gwi_handle h, const double* record, double* gathered);

/* Sharded BATCHES: K hyper-parameter points per exchange (one process per GPU, or ranks sharing one GPU).  The counterpart of
 * gwi_eval_batch / _begin / _end -- same arguments, same semantics, k_batch <= max_batch -- valid after gwi_shm_comm_init or
 * gwi_comm_init: every rank scans its shard for all K points, ONE exchange carries K records per rank (the shared-memory
 * segment; or one ncclAllGather of K records on the engine's stream, copied to host memory point-major by one workgroup per
 * point), and every rank assembles the same K results from the ranks' records of each point in rank order, with gwi_combine's
 * arithmetic.  summaries[k], grads[k][n_theta] and norms[k][n_norms] are the global results, identical on every rank;
 * log_bfs / log_neffs / variances [k][n_ev] are this rank's events with the global constant applied.  A two-pass repeat is
 * made by the rank that asks for it before it publishes (shared memory) or by every rank together (RCCL); with
 * marginalize_selection and a gradient, a first exchange carries the K squared-weight records.  Over shared memory a rank whose
 * half of a batch fails (any error of _begin or _end before its exchange) publishes that, and a rank whose K differs is reported
 * as GWI_ERR_INVALID: every rank then returns, without waiting out the exchange's time-out, with an error that names the rank
 * (over RCCL a failed rank leaves the others in the collective).  Every rank must issue the same sequence of batches. */
gwi_status gwi_eval_batch_sharded(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, gwi_summary* summaries,
                                  double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms);
gwi_status gwi_eval_batch_sharded_begin(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, int32_t want_grad, int32_t want_events);
gwi_status gwi_eval_batch_sharded_end(gwi_handle h, gwi_summary* summaries, double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms);
/* ... for callers that exchange the records themselves: gwi_eval_batch_partial is the batched gwi_eval_partial (records[k][len],
 * per-event sites [k][n_ev] without the global constant); gwi_combine_batch assembles records[n_ranks][k][len] for the points
 * thetas[k][n_theta] (it computes their host constants itself; host-only handles too) -- for k = 1 exactly what gwi_combine gives.
 * gwi_shm_exchange_batch publishes records[k][len] (k <= 64) and returns every rank's in gathered[world][k][len]; records NULL
 * publishes a failure of this rank instead (the others return with an error naming it; this call returns GWI_OK once every
 * rank has published). */
gwi_status gwi_eval_batch_partial(gwi_handle h, const double* thetas, int32_t k, double* records, double* log_bfs, double* log_neffs, double* variances);
gwi_status gwi_combine_batch(gwi_handle h, const double* thetas, int32_t k, const double* records, int32_t n_ranks, const gwi_options* opt,
                             gwi_summary* summaries, double* grads, double* norms);
gwi_status gwi_shm_exchange_batch(gwi_handle h, const double* records, int32_t k, double* gathered);

/* Diagnostic: the launch geometry gwi_create chose -- out = {PE tile size, injection tile size, tiles per event, injection
 * tiles, scan workgroups per hyper-parameter point, injection groups of the combine launch} (samples / counts). */
gwi_status gwi_launch_geometry(gwi_handle h, int32_t out[6]);

/* Diagnostic: the tail of the MOST RECENT evaluation launched on this handle -- out = {1 where the combine launch published
 * per-group rows that the host summed (host-final mode), 0 where the final launch summed them on the device; workgroups of the
 * final launch (GWI_FINAL_GROUPS; not launched in host-final mode); workgroup size of the combine launch; 1 where that
 * evaluation published the per-event sites}.  Before any evaluation: what a single evaluation would take.  Changes nothing. */
gwi_status gwi_tail_path(gwi_handle h, int32_t out[4]);

/* Timing of the most recent gwi_eval*: milliseconds between the start/stop HIP events attached to each
 * launch on the engine's stream ([0]=scan kernel, [1]=per-event combine, [2]=final reduce; 0 when the
 * host does the final sum). */
gwi_status gwi_last_kernel_ms(gwi_handle h, float ms[3]);
/* Per-launch kernel timing (off by default: it adds host overhead).  1: kernel begin/end of every launch of an
 * evaluation -- dispatch timestamps of the engine's AQL queue where that is active, HIP events attached to the launches
 * otherwise; 2: the same, forced through the HIP stream (A/B against the AQL path); 0: off. */
gwi_status gwi_set_timing(gwi_handle h, int32_t enabled);

/* Diagnostic: run `n_iter` sequential gwi_eval calls from C (no binding overhead) and return the
 * mean seconds per evaluation; separates host-language overhead from launch + device time. */
gwi_status gwi_selftime(gwi_handle h, const double* theta, const gwi_options* opt, int32_t n_iter, double* seconds_per_eval);

/* n sequential, blocking evaluations (value + gradient) at the given points thetas[n][n_theta] -- the inner loop of
 * a sampler (examples/utils.py:63-85 runs it inside one XLA program) with no host-language binding between two
 * evaluations; uses gwi_eval_sharded when gwi_comm_init has been called on the handle.  log_likelihoods[n];
 * grads[n][n_theta] nullable.  kernel_ms[n][3] (nullable): launch durations [scan, combine, final] of every
 * `timing_every`-th evaluation (event timing switched on for those only), -1 for the others. */
gwi_status gwi_eval_sequence(gwi_handle h, const double* thetas, int32_t n, const gwi_options* opt, double* log_likelihoods, double* grads, int32_t timing_every,
                             float* kernel_ms);

/* The same loop, recording the wall-clock seconds of every evaluation (host theta in -> host results out) into
 * seconds[n]: the latency distribution (median, p5/p95) of SURVEY.md section 8(d). */
gwi_status gwi_eval_latencies(gwi_handle h, const double* thetas, int32_t n, const gwi_options* opt, double* seconds);

/* Models with spline terms: the scan weighs a tile's samples against a reference exponent known before the tile's first
 * sample -- the tile's exact maximum at the previous evaluation of the handle (of the same point of a batch), applied as an
 * exact power of two so that results do not depend on it to the bit.  When the tile's true maximum turns out more than
 * 2^430 (2^215 in a squared-weight pass) away from it -- the first evaluation of a handle whose log-weights lie that far
 * from 0, or a jump in theta that moves a tile's weights by ~300 e-folds -- the evaluation is repeated once; the failed
 * attempt has left the exact maxima behind, so the repeat cannot miss.  This counts the repeated evaluations (a sampler
 * moves theta by a leapfrog step between two evaluations: 0 in any ordinary run, whatever the prior width). */
int64_t gwi_two_pass_repeats(gwi_handle h);

/* Host tuning: restrict the CALLING thread to the CPUs next to the engine's GPU (the local_cpulist of its PCI function,
 * intersected with the thread's current affinity).  Every evaluation is a few PCIe round trips driven by that thread.
 * GWI_ERR_UNSUPPORTED (and no change) when sysfs does not say. */
gwi_status gwi_pin_thread_to_engine(gwi_handle h);
/* the same by device index (GWI_DEVICE_CURRENT = the current HIP device), e.g. BEFORE engines are created, so that their
 * pinned host buffers are first touched on that side too */
gwi_status gwi_pin_thread_to_device(int32_t device);

/* Measured HBM bandwidth of the device, the number SURVEY.md section 8(d) asks to report next to the vendor figure the
 * roofline is normalised against: a read-only sweep (sum of one array: what the scan kernel's traffic looks like) and a
 * STREAM triad a = b + s c, each over arrays of n_doubles (>= 64 Mi doubles recommended: beyond the 256 MB Infinity Cache),
 * best of `iters` launches timed with HIP events.  GB/s = bytes moved / time (triad: 24 B per element).  No reference
 * counterpart (a measurement aid). */
gwi_status gwi_hbm_bandwidth(int32_t device, int64_t n_doubles, int32_t iters, double* read_gbs, double* triad_gbs);

/* The device maths primitives of the scan kernels, called on their own: one launch applies primitive `op` to n lanes of
 * caller-supplied arguments (gwinferno_amd/csrc/gwi_probe.h holds the table: what a[] and b[] carry and what comes back per op).
 * No reference counterpart (a testing aid: tests/test_gpu_math_probe.py holds every primitive to a 50-digit reference).
 *   a     per lane: 1 double (8 for GWI_PROBE_WAVE_SUM8: the eight values of the lane)
 *   b     per lane: 1 double -- the shift of fast_exp_shift, the weight of cubic_taps_weighted, the spline coefficient of
 *         GWI_PROBE_SPLINE_VALUE (lanes 4g .. 4g + 3 evaluate the cubic of b[4g .. 4g + 3], each at its own t = a[i]) --, or 3 for
 *         GWI_PROBE_LOCATE_TERM / _X / GWI_PROBE_LOCATE: lo, inv_dx, n_basis as doubles; read only by these ops, never NULL
 *   out   4 doubles per lane: the four taps; otherwise the result in slot 0 and zeros.  The wave reductions store what each of
 *         the 64 lanes of a wave received (lanes past n enter with the reduction's identity)
 *   iout  1 int per lane: k of the locate family, binades_of; otherwise 0
 * GWI_ERR_INVALID for a NULL pointer, n < 0 or an unknown op, with nothing written; n == 0 is a successful no-op. */
enum {
  GWI_PROBE_EXP = 1,
  GWI_PROBE_EXP_SHIFT = 2,
  GWI_PROBE_EXPM1 = 3,
  GWI_PROBE_RCP = 4,
  GWI_PROBE_CUBIC_TAPS = 5,
  GWI_PROBE_CUBIC_TAPS_WEIGHTED = 6,
  GWI_PROBE_SPLINE_VALUE = 7, /* spline_poly into LDS, then spline_value */
  GWI_PROBE_LOCATE_KNOT = 8,
  GWI_PROBE_LOCATE_TERM = 9,
  GWI_PROBE_LOCATE_X = 10,
  GWI_PROBE_LOCATE = 11,
  GWI_PROBE_WAVE_SUM = 12,
  GWI_PROBE_WAVE_MAX = 13,
  GWI_PROBE_WAVE_MAX_COARSE = 14,
  GWI_PROBE_WAVE_SUM8 = 15,
  GWI_PROBE_BINADES_OF = 16
};
gwi_status gwi_math_probe(int32_t device, int32_t op, int64_t n, const double* a, const double* b, double* out, int32_t* iout);

/* How plain evaluations are dispatched: "aql: active" (AQL packets into a user-mode queue of the engine's own,
 * gwinferno_amd/csrc/gwi_aql.h: 0.4 us of host time per launch instead of 3.5) or the reason the HIP stream is used. */
const char* gwi_dispatch_info(gwi_handle h);

/* Name of the scan kernel this engine runs: the compiled term chain ("plq+plz+spline5", ...; gwi_kernel_variant_name) or
 * "generic (run-time term loop)" -- any product of <= GWI_MAX_TERMS terms has a kernel (the reference's model function
 * multiplies whatever densities the user picks: tests/inference_test.py:256-260, examples/simple_bspline_example.py:58-71);
 * products outside the ahead-of-time set get a chain compiled at gwi_create ("jit:...", below); the generic kernel (2-2.7 x the
 * scan time) runs only where that is impossible. */
const char* gwi_scan_kernel_name(gwi_handle h);

/* ---- scan chains compiled at run time (gwinferno_amd/csrc/gwi_jit.h) ---------------------------------------------------
 * The reference's user model multiplies whatever densities the user picks (tests/inference_test.py:256-260,
 * models/bsplines/separable.py:295-778).  A product of terms whose kind sequence has no ahead-of-time scan kernel gets one
 * at gwi_create: the scan template instantiated for exactly that sequence by hipRTC (gfx950, the flags of the library's
 * own build, from the headers embedded in the library), kept as a code object under $GWI_JIT_CACHE (default
 * ~/.cache/gwinferno_amd).  Without hipRTC (or with GWI_JIT=0) such models run the generic kernel.  The cache is trusted only as
 * far as it is the caller's: a directory that is a link, belongs to another user or is writable by group / others is skipped
 * (next candidate, else compile in this process only, said once on stderr); a cache file is a regular 0600 file of this user
 * carrying a digest of (kinds, samples per lane, kernel names, code object) and is compiled over, never loaded, when it does not
 * match (tests/test_jit_cache_cpu.py).
 *
 * gwi_jit_compile(): compile (or find in the cache) the chain of `kinds` (GWI_TERM_* numbers, ascending -- kinds 15 / 16 ranked as
 * 7 / 9) with
 * `samples_per_lane` (1 | 2) samples per lane -- needs no GPU (samples_per_lane = 0: the batched matrix-core kernel of a spline
 * model instead, `kinds` then being kind + 100 x 16-basis gradient tiles of each term, as gwi_batch_kernel_note names it).  path_out (nullable, path_cap bytes) receives the cache file
 * ("" when no cache directory is both writable and trusted), or the reason on failure; compile_seconds = hipRTC time spent by THIS call chain
 * (0 when the code object came from the cache), from_cache = 1 then.  GWI_ERR_UNSUPPORTED: hipRTC missing / compilation failed.
 * gwi_jit_info(): whether this engine's scan kernel was compiled at run time, what that cost this process and whether the
 * disk cache supplied it; note = why the generic kernel runs where it does ("" otherwise).  All outputs nullable. */
gwi_status gwi_jit_compile(const int32_t* kinds, int32_t n_kinds, int32_t samples_per_lane, char* path_out, int64_t path_cap, double* compile_seconds,
                           int32_t* from_cache);
gwi_status gwi_jit_info(gwi_handle h, int32_t* compiled_at_run_time, double* compile_seconds, int32_t* from_cache, const char** note);

const char* gwi_last_error(gwi_handle h);
void gwi_destroy(gwi_handle h);

/* Library-level queries usable without a GPU. */
int32_t gwi_abi_version(void);
int32_t gwi_kernel_variants(void);         /* number of compiled term sequences */
const char* gwi_kernel_variant_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* GWI_ENGINE_H */
