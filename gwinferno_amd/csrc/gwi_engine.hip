// gwi_engine.hip -- host side + C ABI of the population-likelihood engine (see include/gwi_engine.h).
// gfx950 only; no CPU fallback: every entry point that computes needs a live HIP device.
#include "gwi_device.h"
#include "gwi_mfma.h"
#include "gwi_aql.h"
#include "gwi_ingest.h"
#include "gwi_draw.h"
#include "gwi_spinprior.h"
#include "gwi_mock.h"
#include "gwi_popdraw.h"
#include "gwi_resample.h"
#include "gwi_hist.h"
#include "gwi_cdf.h"
#include "gwi_pit.h"
#include "gwi_rank.h"
#include "gwi_moment.h"
#include "gwi_quant.h"
#include "gwi_kde.h"
#include "gwi_jit.h"
#include "gwi_sampler_queue.h"
#include "gwi_plan.h"
#include "gwi_probe.h"

#include <hip/hip_ext.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cerrno>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

using namespace gwi;

// gwi_plan.h plans launches without the device headers: its copies of their constants are the same numbers
static_assert(gwi_plan::kBlock == kBlock && gwi_plan::kGeomTilesBits == kGeomTilesBits && gwi_plan::kRegularRepShift == kRegularRepShift && gwi_plan::kPolyStride == kPolyStride,
              "gwi_plan.h restates constants of gwi_device.h");

// The two headers a scan chain is compiled from, embedded as text: what hipRTC gets when a model's term sequence has no
// ahead-of-time instantiation (gwi_jit.h).  (.incbin searches the -I directories of the build; host pass only.)
#ifndef __HIP_DEVICE_COMPILE__
__asm__(
    ".pushsection .rodata\n"
    ".global gwi_embedded_device_h\n"
    "gwi_embedded_device_h:\n"
    ".incbin \"gwi_device.h\"\n"
    ".byte 0\n"
    ".global gwi_embedded_engine_h\n"
    "gwi_embedded_engine_h:\n"
    ".incbin \"gwi_engine.h\"\n"
    ".byte 0\n"
    ".global gwi_embedded_mfma_h\n"
    "gwi_embedded_mfma_h:\n"
    ".incbin \"gwi_mfma.h\"\n"
    ".byte 0\n"
    ".popsection\n");
#endif
extern "C" const char gwi_embedded_device_h[];
extern "C" const char gwi_embedded_engine_h[];
extern "C" const char gwi_embedded_mfma_h[];

namespace {

// ------------------------------------------------------------------------------------------------
// compiled term sequences: each entry below is one explicit instantiation of scan_kernel.
// ------------------------------------------------------------------------------------------------
// the scan takes its tile geometry and first column pointers as fourteen scalar dwords ahead of the argument block (ScanHead,
// gwi_device.h): the command processor preloads those into scalar registers
using ScanFn = void (*)(const double*, const double*, const double*, const double*, const double*, unsigned, unsigned, unsigned, unsigned, const KArgs);
using MfmaFn = void (*)(const KArgs);
// the scan's kernel-argument segment as the host stages it
struct ScanBlock {
  ScanHead head;
  KArgs k;
};
static_assert(offsetof(ScanBlock, k) == sizeof(ScanHead) && sizeof(ScanHead) % alignof(KArgs) == 0, "the struct follows the scalars without padding, as in the kernel's argument list");

// Kernel roles of a term sequence (jit::Role): scan (single evaluation), logw (per-sample log-weights), batch (one grid row
// per point), safe (spline models: two-pass / replay instantiation, single and batched launches), pbatch (parametric models:
// batched launches that load every sample once, scan_pbatch_kernel).
struct Variant {
  const char* name;
  int n;
  int kinds[GWI_MAX_TERMS];
  int samples_per_lane;
  ScanFn fn[jit::kRoles];  // nullptr where the role has no instantiation -- and for every role of a chain compiled at run time:
  jit::Chain* jit;         // ... whose kernels come out of this chain's code object (gwi_jit.h)
  bool has(int role) const { return jit ? !jit->lowered[role].empty() : fn[role] != nullptr; }
};

// the SAFE instantiation exists for spline term sequences only, the pbatch one for the others
template <int U, int... Ks>
constexpr ScanFn safe_scan() {
  if constexpr (Chain<U, Ks...>::kSpline)
    return &scan_kernel<false, false, true, U, Ks...>;
  else
    return nullptr;
}
template <int U, int... Ks>
constexpr ScanFn pbatch_scan() {
  if constexpr (Chain<U, Ks...>::kSpline)
    return nullptr;
  else
    return &scan_pbatch_kernel<pbatch_u(U), Ks...>;
}

#define K_PL GWI_TERM_POWERLAW
#define K_PP GWI_TERM_PLPEAK
#define K_PQ GWI_TERM_POWERLAW_RATIO
#define K_BE GWI_TERM_BETA
#define K_TI GWI_TERM_TILT_MIXTURE
#define K_PZ GWI_TERM_POWERLAW_REDSHIFT
#define K_SP GWI_TERM_EXP_SPLINE
#define K_TN GWI_TERM_TRUNCNORM
#define K_LS GWI_TERM_LINEAR_SPLINE
#define K_TJ GWI_TERM_TILT_JOINT
#define K_SM GWI_TERM_SMOOTH
#define K_PS GWI_TERM_PLPEAK_SMOOTH
#define K_PB GWI_TERM_POWERLAW_BOUNDS
#define K_SL GWI_TERM_EXP_SPLINE_LERP
#define K_SPN GWI_TERM_EXP_SPLINE_F32

// U = samples per lane per trip (2 for the register-light parametric models, 1 or 2 for spline models)
#define GWI_VARIANT_U(NAME, U, ...) \
  { NAME, (int)(sizeof((int[]){__VA_ARGS__}) / sizeof(int)), {__VA_ARGS__}, U, {&scan_kernel<false, false, false, U, __VA_ARGS__>, \
    &scan_kernel<true, false, false, U, __VA_ARGS__>, &scan_kernel<false, true, false, U, __VA_ARGS__>,                           \
    safe_scan<U, __VA_ARGS__>(), pbatch_scan<U, __VA_ARGS__>()}, nullptr }
#define GWI_VARIANT(NAME, ...) GWI_VARIANT_U(NAME, 2, __VA_ARGS__)

// Term sequences are canonical: the host sorts a model's terms by kind id (stable).
const Variant kVariants[] = {
#ifdef GWI_AB_FEW_VARIANTS  // quick experiment builds (tools/build_ablations.sh): the chains of the BASELINE configurations only
    GWI_VARIANT("plpeak+plq+plz", K_PP, K_PQ, K_PZ),
    GWI_VARIANT("plpeak+plq+beta2+tilt2+plz", K_PP, K_PQ, K_BE, K_BE, K_TI, K_TI, K_PZ),
    GWI_VARIANT("plq+plz+spline5", K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT_U("plq+plz+spline5/u1", 1, K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT_U("plz+spline7", 1, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP),
#else
    // tests/inference_test.py:162-197 -- powerlaw_primary_ratio_pdf x PowerlawRedshiftModel
    GWI_VARIANT("pl+plq+plz", K_PL, K_PQ, K_PZ),
    // BASELINE config 2 -- PL+Peak m1 x PL q [x PL z]
    GWI_VARIANT("plpeak+plq", K_PP, K_PQ),
    GWI_VARIANT("plpeak+plq+plz", K_PP, K_PQ, K_PZ),
    GWI_VARIANT_U("plpeak+plq+plz/u1", 1, K_PP, K_PQ, K_PZ),  // 128 VGPRs -> 4 waves/SIMD
    // BASELINE config 1 -- + independent Beta magnitudes + independent tilt mixtures
    GWI_VARIANT("plpeak+plq+beta2+tilt2+plz", K_PP, K_PQ, K_BE, K_BE, K_TI, K_TI, K_PZ),
    // tests/inference_test.py:244-285 -- PL z x {BSpline m1, BSpline q, spline(log z)}
    GWI_VARIANT("plz+spline3", K_PZ, K_SP, K_SP, K_SP),
    GWI_VARIANT_U("plz+spline3/u1", 1, K_PZ, K_SP, K_SP, K_SP),
    // BASELINE config 3/4 -- PL q x PL z x {BSpline m1, IID spin magnitudes [, IID tilts]}
    GWI_VARIANT("plq+plz+spline3", K_PQ, K_PZ, K_SP, K_SP, K_SP),
    GWI_VARIANT("plq+plz+spline5", K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT_U("plq+plz+spline5/u1", 1, K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP),
    // BASELINE config 5 -- PL z x {BSpline m1, q, a1, a2, ct1, ct2, spline(log z)}
    // (one sample per lane: 160 VGPRs -> 3 waves/SIMD; measured 83 vs 93 us per scan on config 5)
    GWI_VARIANT_U("plz+spline7", 1, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT_U("plz+spline7/u2", 2, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP),
    // the same two with float32 spline coordinates (narrow columns, GWI_TERM_EXP_SPLINE_F32): config 3/4's spin magnitudes and
    // tilts, config 5's mass ratio, magnitudes and tilts (and the one-sample-per-lane sibling config 3's small catalogs take)
    GWI_VARIANT("plq+plz+spline+splinef4", K_PQ, K_PZ, K_SP, K_SPN, K_SPN, K_SPN, K_SPN),
    GWI_VARIANT_U("plq+plz+spline+splinef4/u1", 1, K_PQ, K_PZ, K_SP, K_SPN, K_SPN, K_SPN, K_SPN),
    GWI_VARIANT_U("plz+spline+splinef5+spline", 1, K_PZ, K_SP, K_SPN, K_SPN, K_SPN, K_SPN, K_SPN, K_SP),
    // PLPeakPrimaryBSplineRatio (separable.py:368-443) x PL z
    GWI_VARIANT("plpeak+plz+spline", K_PP, K_PZ, K_SP),
    // plpeak_primary_ratio_pdf (parametric.py:39-46) x B-spline spin magnitudes and tilts (IID or independent:
    // separable.py:17-292) x PL z -- parametric masses with non-parametric spins
    GWI_VARIANT("plpeak+plq+plz+spline4", K_PP, K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT("plpeak+plq+plz+spline2", K_PP, K_PQ, K_PZ, K_SP, K_SP),                      // ... magnitudes only (or tilts only)
    GWI_VARIANT("plpeak+plq+plz+spline5", K_PP, K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP),    // ... and the redshift spline
    // other products of the separable B-spline models (separable.py) the reference's factories allow (pipeline/utils.py:104-155):
    // B-spline masses with spin magnitudes / tilts and a power-law or spline redshift model
    GWI_VARIANT("plz+spline4", K_PZ, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT("plz+spline5", K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT_U("plz+spline6", 1, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT("plq+plz+spline2", K_PQ, K_PZ, K_SP, K_SP),
    GWI_VARIANT("plq+plz+spline4", K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP),
    GWI_VARIANT_U("plq+plz+spline6", 1, K_PQ, K_PZ, K_SP, K_SP, K_SP, K_SP, K_SP, K_SP),
    // mass-only B-spline models: BSplinePrimaryBSplineRatio / BSplinePrimaryPowerlawRatio x PL z
    GWI_VARIANT("plz+spline2", K_PZ, K_SP, K_SP),
    GWI_VARIANT("plq+plz+spline", K_PQ, K_PZ, K_SP),
    // BSplinePrimaryBSplineRatio x BSplineEffectiveSpinDims (chi_eff, chi_p: separable.py:706-778) x PL z
    GWI_VARIANT_U("plz+spline2+lspline2", 1, K_PZ, K_SP, K_SP, K_LS, K_LS),
    // BSplineIID/IndependentComponentMasses (separable.py:533-703): (m2/m1)^beta x p(m1) p(m2) x PL z
    GWI_VARIANT("pl+plz+spline2", K_PL, K_PZ, K_SP, K_SP),
    // PL+Peak x PL q x default_spin_tilt (parametric.py:97-102) x PL z
    GWI_VARIANT("plpeak+plq+plz+tiltjoint", K_PP, K_PQ, K_PZ, K_TJ),
    // BSplineRedshift (single.py:398-492) in place of the power-law redshift factor: with the parametric
    // mass pair, and with BSplinePrimaryBSplineRatio
    GWI_VARIANT("pl+plq+spline", K_PL, K_PQ, K_SP),
    GWI_VARIANT("spline3", K_SP, K_SP, K_SP),
    // BSplinePrimaryBSplineRatio alone: the (m1, q) mesh of the posterior-predictive curves (postprocess/calculations.py:20-60)
    GWI_VARIANT("spline2", K_SP, K_SP),
    // log-normal m1 peak x BSplineRatio (postprocess/calculations.py:94-130)
    GWI_VARIANT("spline+truncnorm", K_SP, K_TN),
    // merger rate of redshift, (1 + z)^lamb exp(spline(log z)) (postprocess/calculations.py:261-276)
    GWI_VARIANT("pl+spline", K_PL, K_SP),
    // plpeak_primary_ratio_pdf with the low-mass taper `delta` (parametric.py:39-53) [x PL z]
    GWI_VARIANT("plq+plz+smooth+plpeaksmooth", K_PQ, K_PZ, K_SM, K_PS),
    GWI_VARIANT("plq+smooth+plpeaksmooth", K_PQ, K_SM, K_PS),
    GWI_VARIANT("plz+plpeaksmooth", K_PZ, K_PS),
    // PLPeakPrimaryBSplineRatio (separable.py:368-443) x BSplineSymmetricChiEffective (single.py:233-284) x PL z
    GWI_VARIANT("plpeak+plz+spline+lspline", K_PP, K_PZ, K_SP, K_LS),
    // construct_hierarchical_model (analysis.py:359-424) on the reference's own distributions
    // (numpyro_distributions.py): Powerlaw m1 and q with sampled bounds x PowerlawRedshift
    // (examples/config_files/config.yml), and BSplineDistribution m1, q x PowerlawRedshift
    GWI_VARIANT("plz+plb2", K_PZ, K_PB, K_PB),
    GWI_VARIANT("plz+lerp2", K_PZ, K_SL, K_SL),
    GWI_VARIANT("plb", K_PB),
    GWI_VARIANT("lerp", K_SL),
    // single-term sequences (term-level parity tests)
    GWI_VARIANT("lspline", K_LS),
    GWI_VARIANT("tiltjoint", K_TJ),
    GWI_VARIANT("pl", K_PL),
    GWI_VARIANT("plpeak", K_PP),
    GWI_VARIANT("plq", K_PQ),
    GWI_VARIANT("beta", K_BE),
    GWI_VARIANT("tilt", K_TI),
    GWI_VARIANT("plz", K_PZ),
    GWI_VARIANT("spline", K_SP),
    GWI_VARIANT("truncnorm", K_TN),
    GWI_VARIANT("smooth", K_SM),
    GWI_VARIANT("plpeaksmooth", K_PS),
#endif
};
constexpr int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));

// The fallback for every other product of terms: the generic chain (gwi_device.h, kGenericChain), whose term kinds are read
// from the argument block at run time.  One kernel plays every role (single / batched / two-pass / replay: the SAFE
// instantiation takes those as run-time options) plus the log-weight variant.
const Variant kGenericVariant = {"generic (run-time term loop)", 0, {0}, 1, {&scan_kernel<false, false, true, 1, kGenericChain>, &scan_kernel<true, false, false, 1, kGenericChain>,
                                 &scan_kernel<false, false, true, 1, kGenericChain>, &scan_kernel<false, false, true, 1, kGenericChain>, nullptr}, nullptr};

// ---- batched launches of spline models on the matrix cores (gwi_mfma.h): term sequences with the number of 16-basis
// gradient tiles of every spline term fixed at compile time.  A model qualifies when its kinds match and every spline
// term has n_basis <= 16 * tiles; the first qualifying entry is used (entries with fewer tiles first).
struct MfmaVariant {
  const char* name;
  int n;
  int kinds[GWI_MAX_TERMS];
  int tiles[GWI_MAX_TERMS];
  MfmaFn fn;        // gradient tiles on the matrix cores (scan_mfma_kernel)
  MfmaFn rows_fn;   // gradient rows in LDS (scan_rows_kernel)
  int row_doubles;  // doubles a staged sample occupies (gwi_mfma.h: MChain::kRowDoubles)
};
#define T1(K) (100 + (K))
#define T2(K) (200 + (K))
#define T4(K) (400 + (K))
#define GWI_MFMA(NAME, U, ...) \
  { NAME, (int)(sizeof((int[]){__VA_ARGS__}) / sizeof(int)), {__VA_ARGS__}, {0}, &scan_mfma_kernel<U, __VA_ARGS__>, &scan_rows_kernel<U, __VA_ARGS__>, MChain<false, __VA_ARGS__>::kRowDoubles }
MfmaVariant kMfmaVariants[] = {
    // tests/inference_test.py:244-285 model and the mass-only models
    GWI_MFMA("plz+spline3 (16,16,16)", 1, K_PZ, T1(K_SP), T1(K_SP), T1(K_SP)),
    GWI_MFMA("plz+spline2 (32,16)", 1, K_PZ, T2(K_SP), T1(K_SP)),
    // BASELINE config 3/4: PL q x PL z x {m1 (30), IID spin magnitudes (16, 16), IID tilts (16, 16)}
    GWI_MFMA("plq+plz+spline5 (32,16,16,16,16)", 1, K_PQ, K_PZ, T2(K_SP), T1(K_SP), T1(K_SP), T1(K_SP), T1(K_SP)),
    GWI_MFMA("plq+plz+spline3 (32,16,16)", 1, K_PQ, K_PZ, T2(K_SP), T1(K_SP), T1(K_SP)),
    // BASELINE config 5: PL z x {m1 (30), q (14), a1, a2, ct1, ct2 (12 each), z (12)}
    GWI_MFMA("plz+spline7 (32,16,16,16,16,16,16)", 1, K_PZ, T2(K_SP), T1(K_SP), T1(K_SP), T1(K_SP), T1(K_SP), T1(K_SP), T1(K_SP)),
    // ... both with float32 spline coordinates (narrow columns): the batched path of a narrow model is its wide twin's
    GWI_MFMA("plq+plz+spline+splinef4 (32,16,16,16,16)", 1, K_PQ, K_PZ, T2(K_SP), T1(K_SPN), T1(K_SPN), T1(K_SPN), T1(K_SPN)),
    GWI_MFMA("plz+spline+splinef5+spline (32,16,16,16,16,16,16)", 1, K_PZ, T2(K_SP), T1(K_SPN), T1(K_SPN), T1(K_SPN), T1(K_SPN), T1(K_SPN), T1(K_SP)),
    // the reference's default spline counts (pipeline/utils.py:29-33): m1 50, q 30, spins 16, z 20
    GWI_MFMA("plz+spline7 (64,32,16,16,16,16,32)", 1, K_PZ, T4(K_SP), T2(K_SP), T1(K_SP), T1(K_SP), T1(K_SP), T1(K_SP), T2(K_SP)),
    // linear (chi_eff / chi_p) splines
    GWI_MFMA("plz+spline2+lspline2 (16,16,16,16)", 1, K_PZ, T1(K_SP), T1(K_SP), T1(K_LS), T1(K_LS)),
    // parametric masses with B-spline spins
    GWI_MFMA("plpeak+plq+plz+spline4 (16,16,16,16)", 1, K_PP, K_PQ, K_PZ, T1(K_SP), T1(K_SP), T1(K_SP), T1(K_SP)),
};
constexpr int kNumMfmaVariants = (int)(sizeof(kMfmaVariants) / sizeof(kMfmaVariants[0]));
struct MfmaTableInit {
  MfmaTableInit() {
    for (auto& v : kMfmaVariants)
      for (int t = 0; t < v.n; ++t) {
        v.tiles[t] = v.kinds[t] / 100;
        v.kinds[t] %= 100;
      }
  }
} g_mfma_table_init;

const MfmaVariant* find_mfma_variant(const gwi_spec& s) {
  for (int v = 0; v < kNumMfmaVariants; ++v) {
    const MfmaVariant& m = kMfmaVariants[v];
    if (m.n != s.n_terms) continue;
    bool ok = true;
    for (int t = 0; t < s.n_terms && ok; ++t) {
      ok = m.kinds[t] == s.terms[t].kind;
      if (ok && m.tiles[t] > 0) ok = s.terms[t].n_basis <= 16 * m.tiles[t];
    }
    if (ok) return &m;
  }
  return nullptr;
}

// First entry whose kind sequence matches; GWI_SAMPLES_PER_LANE=1|2 prefers that unroll where compiled.
const Variant* find_variant(const gwi_spec& s) {
  int prefer = 0;
  if (const char* env = std::getenv("GWI_SAMPLES_PER_LANE")) prefer = std::atoi(env);
  const Variant* first = nullptr;
  for (int v = 0; v < kNumVariants; ++v) {
    if (kVariants[v].n != s.n_terms) continue;
    bool same = true;
    for (int t = 0; t < s.n_terms; ++t) same = same && kVariants[v].kinds[t] == s.terms[t].kind;
    if (!same) continue;
    if (!first) first = &kVariants[v];
    if (prefer && kVariants[v].samples_per_lane == prefer) return &kVariants[v];
  }
  return first;
}

// record published by final_kernel (doubles):
//   [0] completion stamp  [1] sum_i logsumexp_i  [2] sum_i variance_i  [3] min_i nan_to_num(log n_eff_i)
//   [4] inj M  [5] inj S1  [6] inj S2  [7] n_ev (local)  [8..) norms, grad_pe[n_theta], grad_inj[n_theta]
constexpr int kRecNormOff = 8;

// ------------------------------------------------------------------------------------------------
// hyper-parameter-only scalars ("prelude"), computed on the host in double precision
// ------------------------------------------------------------------------------------------------
// log of the power-law normaliser (1+a)/(hi^(1+a) - lo^(1+a)) and its alpha-derivative
// (distributions.py:112-116), evaluated in the log domain so large |alpha| cannot overflow.
//
// alpha = -1 is a REMOVABLE singularity, and the closed forms below cancel next to it: log1p(-rho) loses log A to
// eps / |t| and 1/a1 - (..)/(1 - rho) loses d log A to eps h / t^2 (t = a1 h, h = log(hi/lo) / 2) -- 1e-5 of d log A at
// |1 + alpha| = 1e-6, all of it at 1e-8.  For |t| < 1 the same two numbers are therefore written around the midpoint
// c = (log hi + log lo) / 2, where nothing cancels:
//   log A   = -a1 c - log(2 h) - log(sinh t / t)
//   dlogA/da = -c - h L(t),   L(t) = coth t - 1/t = t/3 - t^3/45 + 2 t^5/945 - ...   (the Langevin function)
// L by its series below |t| = 0.1 (the next term, t^15 / 4.5e7, is < 1e-22 there) and directly above (coth t - 1/t is then
// good to 10 eps).  The exact point keeps its own branch (the reference's, and the same numbers as ever), and |t| >= 1 -- every
// draw of the benchmark priors -- the log-domain forms.
double langevin(double t) {
  if (std::fabs(t) < 0.1) {
    const double u = t * t;
    return t * (1.0 / 3.0 + u * (-1.0 / 45.0 + u * (2.0 / 945.0 + u * (-1.0 / 4725.0 + u * (2.0 / 93555.0 + u * (-1382.0 / 638512875.0 + u * (4.0 / 18243225.0)))))));
  }
  return 1.0 / std::tanh(t) - 1.0 / t;
}
//
// The WIDTH log(hi / lo) = 2 h is taken as log1p((hi - lo) / lo), not as log hi - log lo: the difference of two separately rounded
// logarithms carries an absolute error of an ulp of log hi, which for sampled bounds (GWI_TERM_POWERLAW_BOUNDS) that lie
// close together is a large relative error of h -- 1.3e-10 in log(2 h) at hi / lo - 1 = 1e-6.  hi - lo is exact for hi < 2 lo.
void powerlaw_lognorm(double alpha, double lo, double hi, double* logA, double* dlogA) {
  const double a1 = 1.0 + alpha, llo = std::log(lo), lhi = std::log(hi), lw = std::log1p((hi - lo) / lo);
  if (a1 == 0.0) {
    *logA = -std::log(lw);
    *dlogA = -0.5 * (lhi + llo);
    return;
  }
  const double c = 0.5 * (lhi + llo), h = 0.5 * lw, t = a1 * h;
  if (std::fabs(t) < 1.0) {
    *logA = -a1 * c - std::log(2.0 * h) - std::log(std::sinh(t) / t);
    *dlogA = -c - h * langevin(t);
    return;
  }
  if (a1 > 0) {
    const double rho = std::exp(-a1 * lw);  // (lo/hi)^a1
    *logA = std::log(a1) - (a1 * lhi + std::log1p(-rho));
    *dlogA = 1.0 / a1 - (lhi - rho * llo) / (1.0 - rho);
  } else {
    const double rho = std::exp(a1 * lw);  // (hi/lo)^a1
    *logA = std::log(-a1) - (a1 * llo + std::log1p(-rho));
    *dlogA = 1.0 / a1 - (llo - rho * lhi) / (1.0 - rho);
  }
}

// log of the truncated-normal normaliser 1/(sig sqrt(2pi) (Phi(b)-Phi(a))) and its derivatives
// (distributions.py:136-142)
void truncnorm_lognorm(double mu, double sg, double lo, double hi, double* logC, double* dmu, double* dsg) {
  const double r2 = std::sqrt(2.0);
  const double a = (lo - mu) / sg, b = (hi - mu) / sg;
  const double dphi = 0.5 * (1.0 + std::erf(b / r2)) - 0.5 * (1.0 + std::erf(a / r2));
  const double inv_s2pi = 1.0 / std::sqrt(2.0 * M_PI);
  const double pa = std::exp(-0.5 * a * a) * inv_s2pi, pb = std::exp(-0.5 * b * b) * inv_s2pi;
  *logC = -std::log(sg) - 0.5 * std::log(2.0 * M_PI) - std::log(dphi);
  *dmu = (pb - pa) / (sg * dphi);
  *dsg = -1.0 / sg + (b * pb - a * pa) / (sg * dphi);
}

}  // namespace

// ---- RCCL, bound at run time (no link-time dependency; the same librccl the host framework uses) ----
namespace {
struct NcclId {  // ncclUniqueId (rccl.h:43), passed by value
  char b[128];
};
struct NcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
NcclApi g_nccl;
constexpr int kNcclDouble = 8;  // ncclFloat64 (rccl.h:467)

bool load_nccl(const char* path, std::string* err) {
  if (g_nccl.lib) return true;
  const char* p = (path && *path) ? path : "librccl.so.1";
  void* lib = dlopen(p, RTLD_NOW | RTLD_GLOBAL);
  if (!lib) {
    *err = std::string("dlopen(") + p + ") failed: " + dlerror();
    return false;
  }
  g_nccl.GetUniqueId = reinterpret_cast<decltype(g_nccl.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
  g_nccl.CommInitRank = reinterpret_cast<decltype(g_nccl.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
  g_nccl.AllGather = reinterpret_cast<decltype(g_nccl.AllGather)>(dlsym(lib, "ncclAllGather"));
  g_nccl.CommDestroy = reinterpret_cast<decltype(g_nccl.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
  g_nccl.GetErrorString = reinterpret_cast<decltype(g_nccl.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
  if (!g_nccl.GetUniqueId || !g_nccl.CommInitRank || !g_nccl.AllGather || !g_nccl.CommDestroy) {
    *err = std::string("librccl at ") + p + " lacks the expected symbols";
    return false;
  }
  g_nccl.lib = lib;
  return true;
}

// An owned device array that only grows: reserve(n) keeps the allocation while it holds n elements and otherwise frees it and
// allocates anew (always at least one element); reset() frees it.  It is freed on the device that is current at the time, so the
// owner selects the array's device first.
template <class T>
struct DeviceBuffer {
  T* ptr = nullptr;
  size_t cap = 0;
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr, o.cap = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {  // (the previous allocation goes away with `o`)
    std::swap(ptr, o.ptr);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DeviceBuffer() { reset(); }
  hipError_t reserve(size_t n) {
    n = n ? n : 1;
    if (n <= cap) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc(&ptr, sizeof(T) * n);
    if (e != hipSuccess) ptr = nullptr;
    cap = ptr ? n : 0;
    return e;
  }
  void reset() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
  // src[n] copied from the host into an allocation that holds it
  hipError_t upload(const T* src, size_t n) {
    const hipError_t e = reserve(n);
    return e != hipSuccess || !n ? e : hipMemcpy(ptr, src, sizeof(T) * n, hipMemcpyHostToDevice);
  }
  operator T*() const { return ptr; }
};

// Device memory of the post-processing entries of one engine.  destroy_impl assigns an empty set over it where the engine's other
// device memory is freed; gwi_set_histogram_bins does the same with `hist`.
struct PostprocessBuffers {
  DeviceBuffer<double> d_logw_pe, d_logw_inj;  // the log-weight role of the scan chain (fill_log_weights)
  DeviceBuffer<double> d_point_w;              // the points' weights [k][n_ev + 1] of one weighted call (grown on demand, kept)
  // index draws (gwi_draw.h): the caller's masks, the tiles' (max, sum, mass, prefix) + the segments' maxima, and the uniforms /
  // indices of one gwi_draw_indices call (grown on demand, kept)
  DeviceBuffer<unsigned char> d_draw_mask_pe, d_draw_mask_inj;
  DeviceBuffer<double> d_draw_tiles, d_draw_u;
  DeviceBuffer<int> d_draw_idx;
  // injection resampling (gwi_resample.h): the injection tiles' (max, sum, mass, prefix, sum w^2) + M + the stats record, the tiles'
  // live counts, the in-tile prefix of every injection, and the indices / log-weights of one select launch (grown on demand, kept)
  DeviceBuffer<double> d_rs_tiles, d_rs_prefix, d_rs_lw;
  DeviceBuffer<int> d_rs_live, d_rs_idx;
  // weighted histograms (gwi_hist.h): the bin codes of gwi_set_histogram_bins, the tiles' partial histograms, the running sums
  // [n_ev + 1][n_cols][n_bins], the dead counts [n_ev + 1] and the sums of the points' weights [n_ev + 1] of one
  // gwi_weighted_histograms(_weighted) call (allocated with the bins, kept)
  struct Histogram {
    DeviceBuffer<unsigned short> d_bins_pe, d_bins_inj;
    DeviceBuffer<double> d_partial, d_sums, d_vsum;
    DeviceBuffer<int> d_dead;
    // ... and of gwi_point_cdfs (gwi_cdf.h): one point's F [n_ev + 1][n_cols][n_bins] and segment flags [n_ev + 1], the staged rows
    // [64][4][n_cols][n_bins] and live counts [64][2] (allocated on that entry's first call after the bins were set, released with them)
    DeviceBuffer<double> d_cdf, d_cdf_stage;
    DeviceBuffer<int> d_cdf_dead, d_cdf_live;
    // ... and of gwi_point_pits (gwi_pit.h), which shares d_cdf and d_cdf_dead: the staged brackets [64][n_ev][n_cols][2], detected CDFs
    // [64][n_cols][n_bins] and flags [64][n_ev + 1] (allocated on that entry's first call after the bins were set, released with them)
    DeviceBuffer<double> d_pit_stage, d_pit_det;
    DeviceBuffer<int> d_pit_dead;
    int cols = 0, bins = 0;
  } hist;
  // marginal weights and their quantiles (gwi_quant.h).  The state of the handle: one running double per sample [n_ev n_pe | n_inj],
  // the dead counts [n_ev + 1], the sums of the points' weights and of their squares [2][n_ev + 1] (allocated and zeroed on the
  // first use of any of the entries) and the number of points added
  struct Marginal {
    DeviceBuffer<double> d_w, d_vsum;
    DeviceBuffer<int> d_dead;
    long long n_points = 0;
  } marg;
  // ... the columns of gwi_set_quantile_columns (values and orders of either set), the tiles' sums [n_tiles][n_cols][3] and their
  // prefix [n_tiles][n_cols] (allocated with the columns, kept), and the levels / indices / (moments, mass) of one query
  struct Quantile {
    DeviceBuffer<double> d_x_pe, d_x_inj, d_partial, d_prefix, d_levels, d_out;
    DeviceBuffer<int> d_order_pe, d_order_inj, d_idx;
    int cols = 0;
  } quant;
  // weighted kernel density estimates of the marginal weights (gwi_kde.h): the columns and bounds of gwi_set_kde_columns and the tiles'
  // and segments' moments (allocated with the columns, kept); the pairs, grids, bandwidth records, partials and densities of one query
  // (grown on demand, kept)
  struct Kde {
    DeviceBuffer<double> d_x_pe, d_x_inj, d_bounds, d_part1, d_seg1, d_part2, d_band, d_bw, d_neff, d_grid, d_partial, d_rho;
    DeviceBuffer<int> d_pairs, d_degenerate;
    int cols = 0;
  } kde;
};
// ... and of the exact per-event PITs (gwi_rank.h): the injections' orders and the PE samples' ranks of gwi_set_rank_columns, and the
// entry's own workspace -- the injection tiles' sums and offsets [2][n_cols][n_inj_tiles], the prefix table P [n_cols][n_inj + 1], the
// event tiles' partial sums [n_ev tiles_per_event][n_cols][2] and the staged rows [64][n_ev][n_cols][2] and flags [64][n_ev + 1]
// (allocated with the columns, kept).  A record of its own at the END of the engine: PostprocessBuffers sits in the middle of it, and
// growing it moved every field the evaluation path reads after it, which the single-evaluation benchmark saw (1.2 % at config 2).
struct RankBuffers {
  DeviceBuffer<int> d_order_inj, d_rank_lt, d_rank_le, d_dead;
  DeviceBuffer<double> d_tiles, d_prefix, d_partial, d_stage;
  int cols = 0;
};
// ... and of the per-point moments (gwi_moment.h), which read the columns of gwi_set_kde_columns where they lie: the tiles' sums
// [n_tiles][n_cols + P] and the staged rows [64][n_ev + 1][n_cols + P] and flags [64][n_ev + 1] (grown on demand, kept).  At the end of
// the engine for RankBuffers' reason.
struct MomentBuffers {
  DeviceBuffer<double> d_partial, d_stage;
  DeviceBuffer<int> d_dead;
};
// ... and of the per-point conditional moments (gwi_cond.h), which read the codes of gwi_set_histogram_bins and the columns of
// gwi_set_kde_columns where they lie: the tiles' sums [n_tiles][n_pairs][3][n_bins], the bins' weights [n_ev + 1][n_pairs][n_bins] and the
// staged rows [64][n_ev + 1][n_pairs][3][n_bins] and flags [64][n_ev + 1] (grown on demand, kept).  At the end of the engine for
// RankBuffers' reason, and there as a pointer: the record is made on the entry's first call and released by release_moment_and_conditional_buffers(),
// which like the entry and its kernels is defined behind everything the evaluation path runs.  A member by value grew destroy_impl
// and the engine's destructor, every function behind them moved by 16 bytes, and the single-evaluation benchmark read 1.5 % lower
// (measured: profiles/point_conditionals/RESULTS.md, "The buffers' place").  The engine's destructor does not know the record: the
// one path that deletes a device handle without release_moment_and_conditional_buffers() is destroy_impl's poisoned one, which
// leaks device memory on purpose (a kernel may still run), as it does with `post`.
struct ConditionalBuffers {
  DeviceBuffer<double> d_partial, d_bin_w, d_stage;
  DeviceBuffer<int> d_dead;
};
// ... and of the per-point rank correlations (gwi_rankcorr.h): per rank set (the pooled PE samples, the injections) the orders and the
// members' ranks of gwi_set_rankcorr_columns, and the entry's own workspace -- the order tiles' sums and offsets [2][n_cols][order
// tiles of both sets], the prefix tables P [n_cols][n + 1] of either set, the sample tiles' sums [n_tiles][items] and the staged rows
// [64][2][items] and flags [64][n_ev + 2] (allocated with the columns, kept).  A pointer for ConditionalBuffers' reason, released with it.
struct RankcorrBuffers {
  DeviceBuffer<int> d_codes, d_dead;  // order, lt, le of the observed set, then of the detected set
  DeviceBuffer<double> d_tiles, d_prefix, d_partial, d_stage;
  int cols = 0;
};
// ... and of the per-point tails (gwi_tail.h): the tail sizes of gwi_set_tail_sizes, and the entry's own workspace -- the segments'
// prefixes [n_ev + 1] and the tiles' largest keys below [n_tiles] (d_keys), the tiles' histograms, then candidates [n_tiles][2048], the
// segments' ranks [n_ev + 1][2] and the tiles' counts [n_tiles][4] (d_ints), the tiles' body sums [n_tiles] and the staged rows
// [64][n_ev m_pe + m_inj] and [64][n_ev + 1][4] of either kind (grown on demand, kept).  A pointer for ConditionalBuffers' reason,
// released with it.
struct TailBuffers {
  DeviceBuffer<unsigned long long> d_keys;
  DeviceBuffer<int> d_hist, d_ints, d_counts;
  DeviceBuffer<double> d_body, d_tail, d_stats;
  int m_pe = 0, m_inj = 0;
};
// ... and of the bootstrap replicates (gwi_boot.h): the setting of gwi_set_bootstrap, and the entry's own workspace -- the tiles' partial
// sums and counts [n_tiles][B], the staged rows [64][n_ev + 1][B], [64][n_ev + 1][2] and [64][n_ev + 1] and the call's counts
// [n_ev + 1][B] (grown on demand, kept).  A pointer for ConditionalBuffers' reason, released with it.
struct BootBuffers {
  DeviceBuffer<double> d_tile_sum, d_sums, d_stats;
  DeviceBuffer<int> d_tile_count, d_dead;
  DeviceBuffer<long long> d_counts;
  unsigned long long seed = 0;
  int n_rep = 0, first_rep = 0;
};
// ... and of the per-point joint histograms (gwi_hist2d.h), which read the codes of gwi_set_histogram_bins where they lie: ONE pair's
// partials [n_tiles][B B] and shares [n_ev + 1][B B], the point's segment flags [n_ev + 1], the running sums [n_ev + 1][n_pairs][B B]
// with the dead counts and weight sums [n_ev + 1] of one call, and the staged rows [64][n_pairs][B B] of either kind and [64][2]
// (reserved on the entry's first call, grown on demand, kept).  A pointer for ConditionalBuffers' reason, released with it.
struct Hist2dBuffers {
  DeviceBuffer<double> d_partial, d_share, d_sums, d_vsum, d_obs, d_pred;
  DeviceBuffer<int> d_seg_dead, d_dead, d_live;
};
}  // namespace

struct gwi_engine {
  gwi_spec spec;
  const Variant* variant = nullptr;
  Variant* jit_variant = nullptr;     // owned: the variant record of a chain compiled at gwi_create (variant points at it)
  hipFunction_t jit_fn[jit::kRoles] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // ... its kernels in the chain's module on this device
  std::string jit_note;               // why the generic kernel runs although a chain could have been compiled (gwi_jit_info)
  long long aql_rerings = 0;          // times a wait on the AQL queue rang the doorbell a second time (aql_wait_slow)
  bool pbatch = false;                // parametric model: batched launches load every sample once (scan_pbatch_kernel)
  int pbatch_pts = 0;                 // ... GWI_PBATCH_PTS: points per grid row in rows mode (0: chosen per launch from the batch size and the grid)
  bool pbatch_balanced = true;        // ... (tile, point) units dealt out evenly to one round of resident workgroups (GWI_PBATCH_BALANCED=0: rows mode)
  int pbatch_wgs_per_cu = 4;          // ... resident workgroups of scan_pbatch_kernel per CU (occupancy query at gwi_create)
  int scan_role = jit::kScan;         // role of the scan launch being issued
  const MfmaVariant* mfma = nullptr;  // batched launches with 16 points per wavefront (gwi_mfma.h), when the model qualifies
  bool batch_rows = false;            // ... with the gradient in LDS rows (scan_rows_kernel) instead of MFMA tiles
  int rows_rep = 4;
  int mfma_min_batch = 9;             // ... from this many points per launch (a wave carries 16)
  // which of the two batched kernels a spline model runs follows a STATIC rule (matrix cores from 9 points on when the model has
  // <= 8 gradient tiles): the two kernels sum in different orders, so the choice must not depend on a race of wall times -- same
  // model + same catalog shape = same kernel = same bits, on every handle and every box.  GWI_BATCH_AUTOTUNE=1 opts into the
  // measurement (calibrate_batch_path: three launches of each on the caller's own points on the first batched launch, the faster
  // one stays; per handle, costs 8 extra evaluation sets once, and results then depend on which kernel won).
  // a spline model without an ahead-of-time matrix-core instantiation gets one compiled (gwi_jit.h) on its first batched launch
  // of >= 9 points, or at gwi_create when GWI_BATCH_MFMA=1 asks for that path
  MfmaVariant* jit_mfma = nullptr;    // owned record of that instantiation (mfma points at it once it is loaded)
  hipFunction_t jit_mfma_fn = nullptr;
  bool mfma_jit_pending = false;      // worth trying, not tried yet
  std::string mfma_jit_note;
  bool autotune_wanted = false;       // GWI_BATCH_AUTOTUNE=1
  bool batch_autotune = false;        // a choice is still to be made (only ever true when autotune_wanted)
  bool batch_measured = false;        // ... and has been
  double batch_us[2] = {0.0, 0.0};    // best wall time of one batched evaluation set: [matrix-core kernel, 4-tap kernel]
  size_t mfma_lds_bytes = 0;
  bool batch_used_mfma = false;       // path of the most recent batched launch
  bool batch_events = true;           // gwi_eval_batch: the caller wants the per-event sites
  int combine_threads = kBlock;       // workgroup size of the combine launch
  int device = 0;
  int n_cus = 256;
  hipStream_t stream = nullptr;
  long long n_ev = 0, n_pe = 0, n_inj = 0;
  // device memory
  std::vector<double*> d_cols_pe, d_cols_inj;
  NormD* d_norms = nullptr;
  std::vector<double*> d_norm_arrays;
  double *d_partials = nullptr, *d_ev_out = nullptr, *d_ev_grad = nullptr, *d_inj_out = nullptr, *d_inj_grad = nullptr;
  std::vector<double> sq_records;  // records of the squared-weight pass (marginalize_selection gradient)
  PostprocessBuffers post;  // what the post-processing entries keep on the device (none of it allocated before its first use)
  // pinned, device-visible host memory
  double *h_record = nullptr, *h_record_dev = nullptr;
  // device-final mode: the final launch's G workgroups publish one partial record each here; the host merges them into h_record
  double *h_fin = nullptr, *h_fin_dev = nullptr;
  int final_groups = 1;
  double *h_ev = nullptr, *h_ev_dev = nullptr;
  // host-final mode: per-group result rows + normaliser values in pinned host memory
  bool host_final = false;
  // launch geometry (gwi_plan.h): [0] the single evaluation's, [1] that of batched launches (K >= 4, device-final) where it
  // differs ([1].distinct): two trips per workgroup instead of one
  gwi_plan::Geometry geo[2] = {{256, 256, 1, 1, 0, 1, 1}, {}};
  int geo_now = 0;  // which of the two the pipeline being issued runs on (set_geometry)
  const gwi_plan::Geometry& cur() const { return geo[geo_now]; }
  int rec_stride = 0;
  double *h_rows = nullptr, *h_rows_dev = nullptr;
  double *h_norm = nullptr, *h_norm_dev = nullptr;                    // pinned: Z_j
  unsigned long long *h_norm_stamp = nullptr, *h_norm_stamp_dev = nullptr;  // pinned: per-normaliser stamps
  size_t scan_lds_bytes = 0;
  int gacc_rep = 1;
  bool deterministic = false;   // GWI_DETERMINISTIC=1: replay mode of the shared gradient rows (scan_kernel)
  unsigned long long* d_seq = nullptr;                              // device words: [0] sequence number of the evaluation in flight, [1] redo request
  int* d_tile_nref = nullptr;   // spline models: every tile's reference exponent = its exact maximum at the previous evaluation (KArgs::tile_nref)
  unsigned long long *h_redo = nullptr, *h_redo_dev = nullptr;      // pinned: a scan workgroup asks for the two-pass repeat
  long redo_count = 0;          // evaluations repeated in two-pass mode so far
  unsigned long long seq = 0;
  // results of the last prelude (one per hyper-parameter point of the last launch)
  std::vector<double> host_consts = std::vector<double>(1, 0.0);
  // batched evaluation: up to max_batch hyper-parameter points per launch (blockIdx.y)
  int max_batch = 16;
  ThetaBlock *d_tblocks = nullptr, *h_tblocks = nullptr, *h_tblocks_dev = nullptr;
  bool stage_kernel = true;  // GWI_STAGE_KERNEL=0: upload theta blocks with hipMemcpyAsync instead
  // timing
  bool timing = false;
  bool spin_wait = true;
  bool host_only = false;
  // in-engine RCCL communicator (optional)
  void* nccl_comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  double *d_send = nullptr, *d_recv = nullptr;  // [max_batch][len] / [world][max_batch][len]
  double *h_gather = nullptr, *h_gather_dev = nullptr;  // pinned: [max_batch][world][len] (publish_batch_kernel), then one word:
  unsigned long long *h_gather_redo = nullptr, *h_gather_redo_dev = nullptr;  // ... a gathered record asked for the repeat (= seq)
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // start/stop pairs: scan, combine, final
  float last_ms[3] = {0, 0, 0};
  bool timed_final = false;
  bool last_host_rows = false;   // how the most recent run_pipeline publishes (what its waiter must poll)
  bool last_publish_events = true;  // ... and whether its tail published the per-event sites (gwi_tail_path)
  int last_final_groups = 0;        // ... and the workgroups of its final launch (0: none yet)
  bool pending = false;          // gwi_eval_begin issued, gwi_eval_end not yet called
  bool pending_sq = false;
  bool pending_batch = false;          // ... the pending evaluation is a batch (gwi_eval_batch_begin)
  bool pending_sharded = false;        // ... a sharded batch (gwi_eval_batch_sharded_begin)
  int pending_k = 0;
  std::vector<double> pending_thetas;
  gwi_options pending_opt{};
  std::string err;
  // the engine's own AQL queue (gwi_aql.h): plain single-point evaluations are dispatched through it
  aql::Queue aq;
  aql::Kernel aq_scan, aq_scan_safe, aq_scan_batch, aq_scan_pbatch, aq_combine, aq_final;
  bool aq_have_pbatch = false;
  bool aql_batch = false;          // batched launches (4-tap kernel) can go through the AQL queue too
  char* aq_tail_batch[2] = {nullptr, nullptr};  // persistent TailArgs of batched launches: [publish_events]
  bool scan_is_batch = false;
  int aql_tail_variant = 0;        // 0: single evaluation, 1 / 2: batched without / with the per-event sites
  bool scan_is_safe = false;  // the scan launch being issued is the SAFE instantiation
  bool generic = false;       // no compiled chain for this model: the generic scan kernel (kGenericVariant)
  bool small_geometry = false;  // small catalog of a spline model: the one-sample-per-lane sibling on many small workgroups (gwi_create)
  bool combine_acquire = false;  // the combine packet carries an acquire fence after all (A/B only)
  bool aql_tail_only = true;  // scan launches rewrite only the per-evaluation tail of their argument block (GWI_AQL_TAIL=0: the whole block)
  unsigned tail_parity = 0; // which of the two persistent scan-argument slots the next launch rewrites (aql::dispatch_tail)
  bool aql_active = false;  // queue, argument ring and the three kernels are ready
  char* aq_tail_args = nullptr;  // persistent kernel-argument slot holding this engine's (constant) TailArgs
  bool aql_now = false;     // the pipeline being issued / awaited went through the AQL queue
  bool force_hip_stream = false;  // gwi_set_timing(h, 2): time with HIP events on the HIP stream (A/B against the AQL path)
  std::string aql_note;     // why not, when not
  bool poisoned = false;    // an evaluation timed out or the queue failed with work possibly in flight: no further evaluations
  // single-node record exchange through a POSIX shared-memory segment (gwi_shm_comm_init)
  char* shm_base = nullptr;
  size_t shm_bytes = 0, shm_slot_bytes = 0;
  int shm_rank = 0, shm_world = 0;
  unsigned long long shm_seq = 0;
  std::vector<double> shm_gather;
  ScanBlock sblock;          // what a scan launch takes: preloaded head + argument block
  KArgs& kargs = sblock.k;
  long long inj_off = 0;     // element offset of the injections inside every column allocation (inj_offset)
  std::vector<char> col_f32;  // per entry of d_cols_pe: a narrow (float32) allocation
  RankBuffers rank;           // gwi_set_rank_columns / gwi_point_pits_exact (freed with `post`)
  MomentBuffers moment;       // gwi_point_moments (freed with `post`)
  ConditionalBuffers* cond = nullptr;  // gwi_point_conditionals (release_moment_and_conditional_buffers, with `post`)
  RankcorrBuffers* rankcorr = nullptr;  // gwi_set_rankcorr_columns / gwi_point_rank_correlations (released with `cond`)
  TailBuffers* tail = nullptr;          // gwi_set_tail_sizes / gwi_point_tails (released with `cond`)
  BootBuffers* boot = nullptr;          // gwi_set_bootstrap / gwi_point_bootstrap (released with `cond`)
  Hist2dBuffers* hist2d = nullptr;      // gwi_point_histograms2d (released with `cond`)
};

namespace {

// narrow spline kinds: the coordinate column is float32 in HBM (include/gwi_engine.h: GWI_TERM_EXP_SPLINE_F32)
inline bool is_narrow_kind(int k) { return k == GWI_TERM_EXP_SPLINE_F32 || k == GWI_TERM_LINEAR_SPLINE_F32; }
int term_cols(int kind);

#define GWI_HIP(call)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_);                                   \
      return GWI_ERR_HIP;                                                                           \
    }                                                                                               \
  } while (0)

gwi_status fail(gwi_handle h, gwi_status s, const std::string& msg) {
  if (h) h->err = msg;
  return s;
}

int record_len(const gwi_engine* h) { return kRecNormOff + h->spec.n_norms + 2 * h->spec.n_theta; }

gwi_status validate_spec(gwi_handle h, const gwi_spec* s) {
  if (s->abi_version != GWI_ABI_VERSION) return fail(h, GWI_ERR_INVALID, "abi_version mismatch");
  if (s->n_cols < 1 || s->n_cols > GWI_MAX_COLS) return fail(h, GWI_ERR_INVALID, "n_cols out of range");
  if (s->n_terms < 1 || s->n_terms > GWI_MAX_TERMS) return fail(h, GWI_ERR_INVALID, "n_terms out of range");
  if (s->n_theta < 1 || s->n_theta > GWI_MAX_THETA) return fail(h, GWI_ERR_INVALID, "n_theta out of range");
  if (s->n_norms < 0 || s->n_norms > GWI_MAX_NORMS) return fail(h, GWI_ERR_INVALID, "n_norms out of range");
  if (s->kappa_col < 0 || s->kappa_col >= s->n_cols) return fail(h, GWI_ERR_INVALID, "kappa_col out of range");
  if (s->vt_norm >= s->n_norms) return fail(h, GWI_ERR_INVALID, "vt_norm out of range");
  auto theta_ok = [&](int i) { return i >= 0 && i < s->n_theta; };
  auto col_ok = [&](int i) { return i >= 0 && i < s->n_cols; };
  for (int t = 0; t < s->n_terms; ++t) {
    const gwi_term& tm = s->terms[t];
    int n_cols = 1, n_th = 1;
    switch (tm.kind) {
      case GWI_TERM_POWERLAW: break;
      case GWI_TERM_PLPEAK: n_th = 4; break;  // one column: log x
      case GWI_TERM_POWERLAW_RATIO: n_cols = 2; break;
      case GWI_TERM_BETA: n_cols = 2; n_th = 2; break;
      case GWI_TERM_TILT_MIXTURE: n_th = 2; break;
      case GWI_TERM_POWERLAW_REDSHIFT: break;
      case GWI_TERM_TRUNCNORM: n_th = 2; break;
      case GWI_TERM_TILT_JOINT: n_cols = 2; n_th = 2; break;
      case GWI_TERM_SMOOTH: break;
      case GWI_TERM_PLPEAK_SMOOTH:
        n_cols = 2;
        n_th = 4;
        if (!theta_ok(tm.coef_off)) return fail(h, GWI_ERR_INVALID, "PLPEAK_SMOOTH: coef_off must be the theta index of delta");
        break;
      case GWI_TERM_POWERLAW_BOUNDS: n_cols = 2; n_th = 3; break;
      case GWI_TERM_EXP_SPLINE_LERP:
        if (tm.norm < 0 || tm.norm >= s->n_norms || !s->norms[tm.norm].us || s->norms[tm.norm].n_pts < 2)
          return fail(h, GWI_ERR_INVALID, "EXP_SPLINE_LERP: norm must name the grid normaliser carrying the grid's spline coordinates (us)");
        [[fallthrough]];
      case GWI_TERM_LINEAR_SPLINE:
      case GWI_TERM_EXP_SPLINE:
      case GWI_TERM_LINEAR_SPLINE_F32:
      case GWI_TERM_EXP_SPLINE_F32:
        n_th = 0;
        if (tm.n_basis < 4 || !theta_ok(tm.coef_off) || !theta_ok(tm.coef_off + tm.n_basis - 1)) return fail(h, GWI_ERR_INVALID, "spline coefficient range invalid");
        if (!(tm.p[1] > tm.p[0])) return fail(h, GWI_ERR_INVALID, "spline domain invalid");
        break;
      default: return fail(h, GWI_ERR_INVALID, "unknown term kind");
    }
    for (int c = 0; c < n_cols; ++c)
      if (!col_ok(tm.cols[c])) return fail(h, GWI_ERR_INVALID, "term column index out of range");
    for (int k = 0; k < n_th; ++k)
      if (!theta_ok(tm.theta[k])) return fail(h, GWI_ERR_INVALID, "term theta index out of range");
    if (tm.norm >= s->n_norms) return fail(h, GWI_ERR_INVALID, "term norm index out of range");
  }
  // a narrow column (float32 in HBM) is read by narrow spline terms only: kappa, any other kind, a wide spline term and a
  // GWI_RATIO_LOGM_FROM_SPLINE reference would all read it as float64
  for (int t = 0; t < s->n_terms; ++t) {
    if (!is_narrow_kind(s->terms[t].kind)) continue;
    const int c = s->terms[t].cols[0];
    if (c == s->kappa_col) return fail(h, GWI_ERR_INVALID, "term " + std::to_string(t) + " (narrow spline): its column is kappa");
    for (int t2 = 0; t2 < s->n_terms; ++t2) {
      const gwi_term& o = s->terms[t2];
      const int n_read = o.kind == GWI_TERM_POWERLAW_RATIO ? 2 : term_cols(o.kind);
      for (int j = 0; j < n_read && j < 2; ++j)
        if (o.cols[j] == c && !(is_narrow_kind(o.kind) && j == 0))
          return fail(h, GWI_ERR_INVALID, "term " + std::to_string(t) + " (narrow spline, kind " + std::to_string(s->terms[t].kind) + "): its column " + std::to_string(c) +
                                              " is also read by term " + std::to_string(t2) + " (kind " + std::to_string(o.kind) + "); a narrow column may be read by narrow spline terms only");
    }
  }
  for (int j = 0; j < s->n_norms; ++j) {
    const gwi_norm& nm = s->norms[j];
    if (nm.n_pts < 2 || !nm.tw) return fail(h, GWI_ERR_INVALID, "normaliser grid invalid");
    if (nm.expo_theta >= 0 && (!theta_ok(nm.expo_theta) || !nm.l1)) return fail(h, GWI_ERR_INVALID, "normaliser exponent invalid");
    if (nm.n_basis > 0 && (nm.n_basis < 4 || !nm.us || !theta_ok(nm.coef_off) || !theta_ok(nm.coef_off + nm.n_basis - 1) || !(nm.hi > nm.lo)))
      return fail(h, GWI_ERR_INVALID, "normaliser spline invalid");
  }
  return GWI_OK;
}

// theta -> derived scalars of every term + the sample-independent log-normaliser total
void prelude(gwi_engine* h, const double* theta, double* theta_out, double (*derived_out)[kMaxDerived], double* host_const) {
  double c = 0.0;
  for (int t = 0; t < h->spec.n_terms; ++t) {
    const gwi_term& tm = h->spec.terms[t];
    double* d = derived_out[t];
    for (int i = 0; i < kMaxDerived; ++i) d[i] = 0.0;
    switch (tm.kind) {
      case GWI_TERM_POWERLAW: {
        if (tm.flags & GWI_POWERLAW_UNNORMALISED) break;  // bare x^alpha pairing factor
        double la, dla;
        powerlaw_lognorm(theta[tm.theta[0]], tm.p[0], tm.p[1], &la, &dla);
        c += la;
        break;
      }
      case GWI_TERM_POWERLAW_BOUNDS: {
        const double lo = theta[tm.theta[1]], hi = theta[tm.theta[2]];
        double la, dla;
        powerlaw_lognorm(theta[tm.theta[0]], lo, hi, &la, &dla);
        // at alpha == -1 exactly the reference's Powerlaw.log_prob subtracts log(max/min), not log(log(max/min))
        // (numpyro_distributions.py:130); reproduced, since the per-event sites show it (it cancels in log_l)
        if (theta[tm.theta[0]] == -1.0) la = -std::log(hi / lo);
        c += la;
        break;
      }
      case GWI_TERM_TILT_JOINT: {
        double dmu;
        truncnorm_lognorm(1.0, theta[tm.theta[1]], -1.0, 1.0, &d[0], &dmu, &d[1]);
        const double sg = theta[tm.theta[1]];
        d[2] = 1.0 / (sg * sg);
        d[3] = d[2] / sg;
        break;
      }
      case GWI_TERM_PLPEAK_SMOOTH:
      case GWI_TERM_PLPEAK: {
        powerlaw_lognorm(theta[tm.theta[0]], tm.p[0], tm.p[1], &d[0], &d[1]);
        truncnorm_lognorm(theta[tm.theta[1]], theta[tm.theta[2]], tm.p[0], tm.p[1], &d[2], &d[3], &d[4]);
        const double sg = theta[tm.theta[2]];
        d[5] = 1.0 / (sg * sg);
        d[6] = d[5] / sg;
        break;
      }
      case GWI_TERM_POWERLAW_RATIO: {
        const double b1 = 1.0 + theta[tm.theta[0]];
        d[0] = b1 != 0.0 ? 1.0 / b1 : 0.0;
        d[1] = 0x1p53 * d[0];  // 1 / (1 - r^b1) at r = 1 - 2^-53: a sample whose log m1 rounded onto log mmin (gwi_device.h)
        break;
      }
      case GWI_TERM_BETA: {
        const double a = theta[tm.theta[0]], b = theta[tm.theta[1]];
        c -= std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b);  // betaln (distributions.py:161)
        break;
      }
      case GWI_TERM_TILT_MIXTURE: {
        double dmu;
        truncnorm_lognorm(1.0, theta[tm.theta[1]], -1.0, 1.0, &d[0], &dmu, &d[1]);
        const double sg = theta[tm.theta[1]];
        d[2] = 1.0 / (sg * sg);
        d[3] = d[2] / sg;
        break;
      }
      case GWI_TERM_TRUNCNORM: {
        double lc, dmu, dsg;
        truncnorm_lognorm(theta[tm.theta[0]], theta[tm.theta[1]], tm.p[0], tm.p[1], &lc, &dmu, &dsg);
        c += lc;
        const double sg = theta[tm.theta[1]];
        d[0] = 1.0 / (sg * sg);
        d[1] = d[0] / sg;
        break;
      }
      default: break;
    }
  }
  // A non-finite hyper-parameter makes every weight NaN in the reference, i.e. log_l = nan_to_num(-inf)
  // and a zero gradient (analysis.py:287-289).  The device exp clamps its argument (NaN -> 0), so the
  // case is decided here: a NaN constant routes assemble() down exactly that branch.
  bool theta_finite = true;
  for (int p = 0; p < h->spec.n_theta; ++p) theta_finite = theta_finite && std::isfinite(theta[p]);
  *host_const = theta_finite ? c : NAN;
  std::memcpy(theta_out, theta, sizeof(double) * h->spec.n_theta);
}

// Timing mode attaches a start/stop event pair to the launch itself (hipExtLaunchKernelGGL): the pair
// brackets the kernel's own begin/end as the dispatch reports it -- the quantity rocprofv3's kernel
// trace shows -- instead of stream positions around it, which add 1-3 us of launch gap per bracket.
template <typename F, typename A>
void launch_timed(gwi_handle h, int slot, F fn, dim3 grid, dim3 block, size_t lds, const A& args, size_t used_bytes = sizeof(A)) {
  if (h->aql_now) {  // slot 0 / 1 / 2 = scan / combine / final of the plain evaluation path
    const aql::Kernel& k = slot == 0 ? (h->scan_role == jit::kSafe ? h->aq_scan_safe : (h->scan_role == jit::kPbatch ? h->aq_scan_pbatch : (h->scan_role == jit::kBatch ? h->aq_scan_batch : h->aq_scan)))
                                     : (slot == 1 ? h->aq_combine : h->aq_final);
    const hsa_signal_t done = h->timing ? h->aq.done[slot] : hsa_signal_t{0};
    if (slot > 0 && h->aq_tail_args) {  // constant arguments, staged once at gwi_create
      char* staged = h->aql_tail_variant == 0 ? h->aq_tail_args : h->aq_tail_batch[h->aql_tail_variant - 1];
      // the combine launch reads the scan's records with cache-bypassing loads: no acquire fence (GWI_AQL_COMBINE_ACQUIRE=1: with)
      (void)aql::dispatch_staged(h->aq, k, staged, grid.x, grid.y, block.x, (uint32_t)lds, done, /*acquire=*/slot != 1 || h->combine_acquire);
      return;
    }
    if constexpr (std::is_same<A, ScanBlock>::value) {
      constexpr size_t kOff = offsetof(ScanBlock, k);  // the argument block sits behind the preloaded scalars
      if (!h->aql_tail_only) {  // GWI_AQL_TAIL=0: the whole block into a ring slot per launch (A/B only)
        (void)aql::dispatch(h->aq, k, &args, kOff + used_bytes, grid.x, grid.y, block.x, (uint32_t)lds, done);
        return;
      }
      // the scan's block: fixed head in place, only the per-evaluation tail through the BAR (aql::dispatch_tail)
      const size_t off_theta = kOff + offsetof(KArgs, theta);
      const size_t ranges[3][2] = {{kOff + offsetof(KArgs, norm_seq), offsetof(KArgs, derived) - offsetof(KArgs, norm_seq)},
                                   {kOff + offsetof(KArgs, derived), sizeof(double) * kMaxDerived * (size_t)h->spec.n_terms},
                                   {off_theta, kOff + used_bytes > off_theta ? kOff + used_bytes - off_theta : 0}};
      (void)aql::dispatch_tail(h->aq, k, h->tail_parity++, &args, kOff + offsetof(KArgs, norm_seq), kOff + used_bytes, ranges, 3, grid.x, grid.y, block.x, (uint32_t)lds, done);
      return;  // on a queue error nothing was submitted; the waiters surface it
    } else {
      if (aql::dispatch(h->aq, k, &args, used_bytes, grid.x, grid.y, block.x, (uint32_t)lds, done)) return;
      // the queue reported an error: nothing was submitted; the waiters surface it
      return;
    }
  }
  if constexpr (std::is_same<A, ScanBlock>::value) {
    const ScanHead& hd = args.head;
    if (h->variant->jit) {
      // a chain compiled at gwi_create: its kernel lives in a module, and the staged block IS the kernel-argument segment
      // (preloaded scalars + argument block: static_assert on ScanBlock above)
      size_t bytes = sizeof(ScanBlock);
      void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<ScanBlock*>(&args), HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
      hipFunction_t f = h->jit_fn[h->scan_role];
      if (h->timing)
        (void)hipExtModuleLaunchKernel(f, grid.x * block.x, grid.y, 1, block.x, 1, 1, lds, h->stream, nullptr, extra, h->ev[2 * slot], h->ev[2 * slot + 1], 0);
      else
        (void)hipModuleLaunchKernel(f, grid.x, grid.y, 1, block.x, 1, 1, (unsigned)lds, h->stream, nullptr, extra);
      return;
    }
    if (h->timing)
      hipExtLaunchKernelGGL(fn, grid, block, (unsigned)lds, h->stream, h->ev[2 * slot], h->ev[2 * slot + 1], 0, hd.col[0], hd.col[1], hd.col[2], hd.col[3], hd.col[4], hd.geom, hd.chunks, hd.n_pe, hd.n_inj, args.k);
    else
      hipLaunchKernelGGL(fn, grid, block, lds, h->stream, hd.col[0], hd.col[1], hd.col[2], hd.col[3], hd.col[4], hd.geom, hd.chunks, hd.n_pe, hd.n_inj, args.k);
  } else {
    if (h->timing)
      hipExtLaunchKernelGGL(fn, grid, block, (unsigned)lds, h->stream, h->ev[2 * slot], h->ev[2 * slot + 1], 0, args);
    else
      hipLaunchKernelGGL(fn, grid, block, lds, h->stream, args);
  }
}

// scan_pbatch_kernel takes single-trip tiles: it applies when the geometry of the launch being issued has them
bool pbatch_applies(const gwi_engine* h) {
  if (!h->pbatch) return false;
  const long long gran = (long long)pbatch_u(h->variant->samples_per_lane) * kBlock;
  return h->kargs.chunk_pe <= gran && h->kargs.chunk_inj <= gran;
}
// Points per grid row of a pbatch launch of K points.  One row (every sample loaded once for all K points) is the least work,
// but a tile x K points is a long workgroup: the rows are split until the launch has about eight workgroups per CU to balance
// (config 2, K = 16: 788 tiles on 256 CUs -- one row leaves a quarter of the chip idle behind the CUs that drew four tiles).
int pbatch_points(const gwi_engine* h, int K, const gwi_plan::Geometry& g) {
  int pts = h->pbatch_pts;
  if (pts <= 0) {
    const long long blocks = g.n_scan_blocks;
    int rows = 1;
    while (rows < K && blocks * rows < 8LL * h->n_cus) rows *= 2;
    pts = (K + rows - 1) / rows;
  }
  return std::max(1, std::min(pts, kPbatchMaxPts));
}

constexpr int kPbatchBalancedFrom = 8;  // points per launch from which the balanced mode is used
// Balanced mode: how many workgroups a pbatch launch of K points gets.  One round of resident workgroups, or the next smaller
// count with which every workgroup draws the same number of (tile, point) units: ceil(N / ceil(N / capacity)).
int pbatch_workgroups(const gwi_engine* h, int K) {
  const long long n_units = (long long)h->cur().n_scan_blocks * K, capacity = (long long)h->n_cus * h->pbatch_wgs_per_cu;
  const long long per_wg = (n_units + capacity - 1) / capacity;
  return (int)((n_units + per_wg - 1) / per_wg);
}

gwi_status launch_scan(gwi_handle h, bool logw, int K = 1, bool batch = false) {
  if (logw) h->aql_now = false;  // the log-weight variant is another kernel and always goes through the HIP stream
  // the first n_norms workgroups integrate the normaliser grids (a log-weight launch has none and runs on the single evaluation's geometry: fill_log_weights)
  const int grid = h->cur().n_scan_blocks + (logw ? 0 : h->spec.n_norms);
  // two-pass repeats and the replay mode run the SAFE instantiation (spline models; it takes single and batched launches)
  // ... and so does any replica count other than the 16 the regular kernels are built for (GWI_GACC_REP)
  const bool safe = !logw && h->variant->has(jit::kSafe) && (h->generic || h->kargs.two_pass || h->kargs.deterministic || h->gacc_rep != (1 << kRegularRepShift));
  // parametric models: a batched launch on single-trip tiles loads every sample once for all its points (scan_pbatch_kernel)
  // ... where a grid row holds more than one point: with one point per row (small catalogs: the rows are split until the launch
  // fills the chip) it has nothing to share and the one-row-per-point kernel is the same thing without the staging
  // (balanced mode from eight points on: below that the shared loads no longer pay for the staging -- config 2, K = 4: 18.5 us
  // against 17.4 with one grid row per point, K = 2: 12.8 against 11.3; profiles/round6/balanced_ab.txt)
  const bool balanced = h->pbatch_balanced && K >= kPbatchBalancedFrom;
  const bool pb = batch && !safe && !logw && pbatch_applies(h) && (balanced || pbatch_points(h, K, h->cur()) > 1);
  h->scan_role = logw ? jit::kLogw : (safe ? jit::kSafe : (pb ? jit::kPbatch : (batch ? jit::kBatch : jit::kScan)));
  ScanFn fn = h->variant->fn[h->scan_role];
  h->scan_is_safe = safe;
  h->kargs.k_batch = batch ? K : 1;
  if (pb) {
    const size_t used = offsetof(KArgs, theta);  // the points' hyper-parameters travel in their ThetaBlocks
    if (balanced) {
      const int n_wg = pbatch_workgroups(h, K);
      h->kargs.pbatch_pts = -n_wg;
      launch_timed(h, 0, fn, dim3(h->spec.n_norms * K + n_wg, 1), dim3(kBlock), 0, h->sblock, used);
      GWI_HIP(hipGetLastError());
      return GWI_OK;
    }
    const int pts = pbatch_points(h, K, h->cur());
    h->kargs.pbatch_pts = pts;
    launch_timed(h, 0, fn, dim3(grid - h->spec.n_norms + h->spec.n_norms * K, (K + pts - 1) / pts), dim3(kBlock), 0, h->sblock, used);
    GWI_HIP(hipGetLastError());
    return GWI_OK;
  }
  if (batch && !safe && !logw) {
    h->batch_used_mfma = h->mfma && K >= h->mfma_min_batch;
    if (h->batch_used_mfma && h->mfma == h->jit_mfma && h->jit_mfma_fn) {  // ... the instantiation compiled at run time: a module launch, the argument block as the buffer
      size_t bytes = sizeof(KArgs);
      void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &h->kargs, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
      const unsigned gy_m = (unsigned)((K + kPts - 1) / kPts);
      h->aql_now = false;
      if (h->timing)
        (void)hipExtModuleLaunchKernel(h->jit_mfma_fn, (unsigned)grid * kBlock, gy_m, 1, kBlock, 1, 1, h->mfma_lds_bytes, h->stream, nullptr, extra, h->ev[0], h->ev[1], 0);
      else
        (void)hipModuleLaunchKernel(h->jit_mfma_fn, (unsigned)grid, gy_m, 1, kBlock, 1, 1, (unsigned)h->mfma_lds_bytes, h->stream, nullptr, extra);
      GWI_HIP(hipGetLastError());
      return GWI_OK;
    }
    if (h->batch_used_mfma) {  // 16 points per wavefront: the grid's second dimension counts groups of 16
      launch_timed(h, 0, h->batch_rows ? h->mfma->rows_fn : h->mfma->fn, dim3(grid, (K + kPts - 1) / kPts), dim3(kBlock), h->mfma_lds_bytes, h->kargs, offsetof(KArgs, theta));
      GWI_HIP(hipGetLastError());
      return GWI_OK;
    }
  }
  // theta is the LAST member of the argument block: only the hyper-parameters in use travel through the BAR
  const size_t used = offsetof(KArgs, theta) + sizeof(double) * (size_t)h->spec.n_theta;
  launch_timed(h, 0, fn, dim3(grid, batch ? K : 1), dim3(kBlock), h->scan_lds_bytes, h->sblock, used);
  GWI_HIP(hipGetLastError());
  return GWI_OK;
}

// (the single evaluation is 16 to 28 us end to end: the helpers on its way fold into their entries, as the code they replace did)
#define GWI_HOT inline __attribute__((always_inline))
GWI_HOT gwi_status collect_local(gwi_handle h, int K);
void release_moment_and_conditional_buffers(gwi_handle h);

// launches scan -> combine -> final; `record_dev` is where final_kernel publishes (pinned host record
// or, for the sharded path, the device send buffer); `wait` polls the pinned completion stamp.
// (Folding the two tail stages into the scan launch -- the workgroup that completes a group combines
// it -- was measured and lost: every workgroup then has to drain agent-scope write-through stores and
// wait for an atomic round trip across the XCDs' separate L2s, ~5 us of a resident slot each, more than
// the two launch boundaries cost.  See DESIGN.md.)
#ifdef GWI_HOST_PHASES
// diagnostic build only: accumulated host time per phase of run_pipeline [prelude, scan launch, combine
// launch, norm launch, wait] in seconds, and the call count
double g_phase[5] = {0, 0, 0, 0, 0};
long g_phase_calls = 0;
#define GWI_PHASE(i)                                                                       \
  do {                                                                                     \
    const auto now_ = std::chrono::steady_clock::now();                                    \
    g_phase[i] += std::chrono::duration<double>(now_ - phase_t_).count();                  \
    phase_t_ = now_;                                                                       \
  } while (0)
#else
#define GWI_PHASE(i) \
  do {               \
  } while (0)
#endif

// Arguments of the combine / final launches.  Nothing in them changes from one evaluation to the next (the completion
// stamp travels through a device word the scan writes): on the AQL path they sit in two persistent kernel-argument slots.
TailArgs tail_args(const gwi_engine* h, double* record_dev, int which_geo = 0) {
  const gwi_plan::Geometry& g = h->geo[which_geo];
  TailArgs ta;
  std::memset(&ta, 0, sizeof(ta));
  ta.partials = h->d_partials;
  ta.ev_out = h->d_ev_out;
  ta.ev_grad = h->d_ev_grad;
  ta.inj_out = h->d_inj_out;
  ta.inj_grad = h->d_inj_grad;
  ta.ev_host = h->h_ev_dev;
  ta.host_rows = h->host_final && !record_dev ? h->h_rows_dev : nullptr;
  ta.record = record_dev ? record_dev : h->h_fin_dev;
  ta.final_groups = record_dev ? 1 : h->final_groups;  // the sharded path's single record feeds the all-gather
  ta.seq_ptr = h->d_seq;
  ta.redo_ptr = h->d_seq + 1;
  ta.n_ev = (int)h->n_ev;
  ta.tiles_per_event = g.tiles_per_event;
  ta.n_inj_tiles = g.n_inj_tiles;
  ta.n_inj_groups = g.n_inj_groups;
  ta.tiles_per_inj_group = g.tiles_per_inj_group;
  ta.n_theta = h->spec.n_theta;
  ta.rec_stride = h->rec_stride;
  ta.n_scan_blocks = g.n_scan_blocks;
  ta.n_norms = h->spec.n_norms;
  ta.record_len = record_len(h);
  ta.n_pe = (double)h->n_pe;
  ta.publish_events = 1;
  ta.combine_threads = h->combine_threads;
  ta.row_lines = (3 + h->spec.n_theta + 6) / 7;
  return ta;
}

// which launch geometry the scan's argument block describes: the batched one (geo[1]) or the single evaluation's
void set_geometry(gwi_engine* h, bool batched) {
  h->geo_now = batched ? 1 : 0;
  const gwi_plan::Geometry& g = h->cur();
  h->kargs.tiles_per_event = g.tiles_per_event;
  h->kargs.chunk_pe = g.chunk_pe;
  h->kargs.n_inj_tiles = g.n_inj_tiles;
  h->kargs.chunk_inj = g.chunk_inj;
  ScanHead& hd = h->sblock.head;
  hd.geom = (unsigned)h->kargs.n_ev | ((unsigned)h->kargs.tiles_per_event << kGeomEventBits) | ((unsigned)h->kargs.n_norms << (kGeomEventBits + kGeomTilesBits));
  hd.chunks = pack_chunk(h->kargs.chunk_pe) | (pack_chunk(h->kargs.chunk_inj) << 16);
}

// columns a term kind reads (= the doubles of its Term<K>::In): the order of the scan's preloaded column slots
int term_cols(int kind) {
  switch (kind) {
#define GWI_X(K) \
  case K: return (int)(sizeof(typename Term<K>::In) / sizeof(double));
    GWI_FOR_EACH_KIND(GWI_X)
#undef GWI_X
    default: return 0;
  }
}

gwi_status run_pipeline_once(gwi_handle h, const double* theta, double* record_dev, bool wait, int K, bool batch, bool square) {
#ifdef GWI_HOST_PHASES
  auto phase_t_ = std::chrono::steady_clock::now();
  ++g_phase_calls;
#endif
  const int n_theta = h->spec.n_theta;
  h->kargs.square = square ? 1 : 0;
  // tile references: row 0 belongs to single evaluations, rows 1..max_batch to the points of a batch on the single
  // evaluation's tiling, rows 1 + max_batch.. to the points of a batch on the batched launches' own tiling (geo[1]: other tile
  // boundaries, so another tile's maximum).  Row k of a block keeps meaning "point k of the batch": a vectorised caller
  // should keep chain k in slot k from one call to the next (a reference left by another chain is still only a range
  // question -- a miss costs one repeat, never a wrong bit).
  h->kargs.nref_row0 = batch ? ((K >= 4 && h->geo[1].distinct) ? 1 + h->max_batch : 1) : 0;
  // plain evaluations go through the engine's AQL queue; whatever must be ordered with other work on the HIP stream
  // (batched theta uploads, the sharded path's exchange behind record_dev) stays on the stream, and so does everything
  // after gwi_set_timing(h, 2)
  // batched launches of the 4-tap kernel follow once their theta blocks can be written through the BAR (K >= 4: the
  // device-final form whose tail arguments are staged)
  const bool batch_on_aql = batch && K >= 4 && h->aql_batch && !h->kargs.two_pass && !h->kargs.deterministic && !(h->mfma && K >= h->mfma_min_batch);
  h->aql_now = h->aql_active && !h->aq.failed() && !h->force_hip_stream && record_dev == nullptr && ((!batch && K == 1) || batch_on_aql);
  h->scan_is_batch = batch;
  h->aql_tail_variant = batch_on_aql ? (h->batch_events ? 2 : 1) : 0;
  if (h->aql_now && h->timing && !aql::timed_prepare(h->aq)) h->aql_now = false;  // no dispatch timestamps: time this one with HIP events
  if ((int)h->host_consts.size() < K) h->host_consts.resize(K);
  if (!batch) {
    prelude(h, theta, h->kargs.theta, h->kargs.derived, &h->host_consts[0]);
    h->kargs.tblocks = nullptr;
  } else {
    for (int k = 0; k < K; ++k) prelude(h, theta + (size_t)k * n_theta, h->h_tblocks[k].theta, h->h_tblocks[k].derived, &h->host_consts[k]);
    if (h->aql_now) {
      // theta blocks straight into device memory through the BAR (only the parts in use: a few hundred bytes per point),
      // one hand-off for all of them; the scan packet that reads them is published afterwards
      ThetaBlock* dev = reinterpret_cast<ThetaBlock*>(aql::extra_area(h->aq));
      const size_t th_bytes = sizeof(double) * (size_t)n_theta, der_bytes = sizeof(double) * kMaxDerived * (size_t)h->spec.n_terms;
      for (int k = 0; k < K; ++k) {
        std::memcpy(dev[k].theta, h->h_tblocks[k].theta, th_bytes);
        std::memcpy(dev[k].derived, h->h_tblocks[k].derived, der_bytes);
      }
      // no hand-off of their own: the scan's argument block is written next and handed over with ONE sfence + read-back
      // (aql::dispatch_tail / stage_args), which retires these posted writes as well -- a read cannot pass any posted write
      // ahead of it, whatever its address (a second read-back here cost every batch 1.4 us)
      h->kargs.tblocks = dev;
    } else if (h->stage_kernel && K >= 10) {  // below ~20 KiB the runtime's small-copy path is quicker than a launch
      hipLaunchKernelGGL(stage_theta_kernel, dim3(K), dim3(kBlock), 0, h->stream, (const ThetaBlock*)h->h_tblocks_dev, h->d_tblocks);
      GWI_HIP(hipGetLastError());
    } else {
      GWI_HIP(hipMemcpyAsync(h->d_tblocks, h->h_tblocks, sizeof(ThetaBlock) * K, hipMemcpyHostToDevice, h->stream));
    }
    if (!h->aql_now) h->kargs.tblocks = h->d_tblocks;
  }
  const unsigned gy = batch ? (unsigned)K : 1u;
  // batched device-final launches run on their own geometry where gwi_create found one (two trips per workgroup)
  set_geometry(h, batch && K >= 4 && h->geo[1].distinct);
  TailArgs ta = tail_args(h, record_dev, h->geo_now);
  if (batch && K >= 4) {
    // Many points per launch: sum over groups on the DEVICE whatever the problem size.  Host-final mode publishes one row
    // per (group, point) -- K x (N_ev + injection groups) rows of two small posted PCIe writes each, which is what a
    // 16-point batch of config 2 spent a quarter of its time on (1216 rows) -- against one record per point here; the
    // per-event sites travel (three more small writes per event and point) only when the caller asked for them.
    ta.host_rows = nullptr;
    ta.publish_events = h->batch_events ? 1 : 0;
  }
  h->last_host_rows = ta.host_rows != nullptr;
  h->last_publish_events = ta.publish_events != 0;
  h->last_final_groups = ta.final_groups;
  h->kargs.norm_seq = h->seq + 1;  // the normaliser workgroups of this launch stamp their results with it
  GWI_PHASE(0);
  gwi_status st = launch_scan(h, false, K, batch);
  if (st != GWI_OK) return st;
  GWI_PHASE(1);
  launch_timed(h, 1, combine_kernel, dim3((unsigned)(h->n_ev + ta.n_inj_groups), gy), dim3((unsigned)ta.combine_threads), 0, ta);
  GWI_HIP(hipGetLastError());
  ++h->seq;
  h->timed_final = false;
  GWI_PHASE(2);
  if (ta.host_rows) {
    GWI_PHASE(3);
    const gwi_status sw = wait ? collect_local(h, K) : GWI_OK;
    GWI_PHASE(4);
    return sw;
  }
  launch_timed(h, 2, final_kernel, dim3((unsigned)ta.final_groups, gy), dim3(kFinalThreads), 0, ta);
  GWI_HIP(hipGetLastError());
  h->timed_final = true;
  return wait ? collect_local(h, K) : GWI_OK;
}

// A scan workgroup whose reference exponent turned out too far from its tile's true maximum (models with spline terms:
// scan_kernel, shared mode) has stored this evaluation's sequence number in the pinned redo word.
bool redo_requested(const gwi_engine* h) { return *reinterpret_cast<volatile unsigned long long*>(h->h_redo) == h->seq; }

// The repeat ladder of every evaluating path: when asked() says that the collected evaluation wants a repeat, count it and
// run_again().  The failed attempt has left every tile's exact maximum in tile_nref, so the repeat is the same (fast) kernel with
// exact references and cannot miss; should it ever ask again (it never has) the two-pass instantiation, where the variant has
// one, finds the maxima in a sweep of its own.
template <typename Run, typename Asked>
gwi_status repeat_while_asked(gwi_handle h, Run run_again, Asked asked) {
  if (!asked()) return GWI_OK;
  ++h->redo_count;
  gwi_status st = run_again();
  if (st == GWI_OK && asked() && h->variant->has(jit::kSafe)) {
    h->kargs.two_pass = 1;
    st = run_again();
    h->kargs.two_pass = 0;
  }
  return st;
}

// ... of this rank's own launches: scan -> combine [-> final] once more, waited for.  run_pipeline does this itself with `wait`;
// callers that pass wait = false come here once their results are in (collect_local).
gwi_status repeat_after_redo(gwi_handle h, const double* theta, double* record_dev, int K, bool batch, bool square) {
  return repeat_while_asked(h, [&] { return run_pipeline_once(h, theta, record_dev, true, K, batch, square); }, [&] { return redo_requested(h); });
}
// The matrix-core batched kernel for a spline model that has no ahead-of-time instantiation of it: scan_mfma_kernel
// instantiated for this model's kinds and tile counts by hipRTC (gwi_jit.h), loaded as a module.  Returns whether h->mfma is set.
bool try_jit_mfma(gwi_handle h) {
  h->mfma_jit_pending = false;
  const gwi_spec& s = h->spec;
  int kts[GWI_MAX_TERMS], tiles_total = 0, row_doubles = 0;
  bool any_spline = false;
  for (int t = 0; t < s.n_terms; ++t) {
    const int kind = s.terms[t].kind;
    if (kind == GWI_TERM_EXP_SPLINE_LERP) {
      h->mfma_jit_note = "the interpolated-grid spline term has no matrix-core form";
      return false;
    }
    const bool spline = kind == GWI_TERM_EXP_SPLINE || kind == GWI_TERM_LINEAR_SPLINE || is_narrow_kind(kind);
    const int tiles = spline ? (s.terms[t].n_basis + 15) / 16 : 0;
    any_spline = any_spline || spline;
    kts[t] = kind + 100 * tiles;
    tiles_total += tiles;
    row_doubles += spline ? kSplineStage : term_cols(kind);
  }
  if (!any_spline || tiles_total > 8) {  // more than eight gradient tiles: the 4-tap kernel wins by arithmetic (DESIGN section 0 of round 4, row 4)
    h->mfma_jit_note = any_spline ? "more than eight 16-basis gradient tiles" : "no spline term";
    return false;
  }
  std::string why;
  jit::Chain* c = jit::get_chain(kts, s.n_terms, 0, gwi_embedded_device_h, gwi_embedded_engine_h, why, gwi_embedded_mfma_h);
  hipModule_t mod = c ? jit::module_on(c, h->device, why) : nullptr;
  if (c && !mod && c->from_cache) {
    jit::discard_chain(c);
    c = jit::get_chain(kts, s.n_terms, 0, gwi_embedded_device_h, gwi_embedded_engine_h, why, gwi_embedded_mfma_h);
    mod = c ? jit::module_on(c, h->device, why) : nullptr;
  }
  hipFunction_t fn = nullptr;
  if (mod && hipModuleGetFunction(&fn, mod, c->lowered[jit::kScan].c_str()) != hipSuccess) {
    why = "jit: hipModuleGetFunction(" + c->lowered[jit::kScan] + ") failed";
    (void)hipGetLastError();
    fn = nullptr;
  }
  int scratch = 0;
  if (fn && hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn) == hipSuccess && scratch > 0) {
    why = "the instantiation spills registers to scratch (" + std::to_string(scratch) + " B per lane)";
    fn = nullptr;
  }
  if (!fn) {
    h->mfma_jit_note = why;
    return false;
  }
  MfmaVariant* v = new MfmaVariant();
  std::memset(v, 0, sizeof(*v));
  v->name = c->name.c_str();
  v->n = s.n_terms;
  for (int t = 0; t < s.n_terms; ++t) {
    v->kinds[t] = kts[t] % 100;
    v->tiles[t] = kts[t] / 100;
  }
  v->row_doubles = row_doubles;
  h->jit_mfma = v;
  h->jit_mfma_fn = fn;
  h->mfma = v;
  h->batch_rows = false;
  h->mfma_lds_bytes = sizeof(double) * mfma_lds_doubles(s.n_theta, s.n_terms, row_doubles, 0);
  h->mfma_jit_note = "compiled " + c->name + (c->from_cache ? " (disk cache)" : "");
  return true;
}

// First batched launch of a spline model that has both batched kernels: three timed evaluation sets of each (after one untimed
// set each) on the caller's points, host theta -> host results as a sampler pays them; the faster kernel stays.
gwi_status run_pipeline(gwi_handle h, const double* theta, double* record_dev, bool wait, int K, bool batch, bool square);
gwi_status calibrate_batch_path(gwi_handle h, const double* theta, int K) {
  h->batch_autotune = false;
  const MfmaVariant* const both[2] = {h->mfma, nullptr};
  double best[2] = {1e30, 1e30};
  gwi_status st = GWI_OK;
  for (int rep = 0; rep < 4 && st == GWI_OK; ++rep)
    for (int which = 0; which < 2 && st == GWI_OK; ++which) {
      h->mfma = both[which];
      const auto t0 = std::chrono::steady_clock::now();
      st = run_pipeline(h, theta, nullptr, true, K, true, false);
      const double us = 1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (rep > 0 && us < best[which]) best[which] = us;
    }
  h->batch_us[0] = best[0];
  h->batch_us[1] = best[1];
  h->batch_measured = st == GWI_OK;
  h->mfma = (st != GWI_OK || best[0] <= best[1]) ? both[0] : nullptr;
  return st;
}

// Before a batched launch of K points: a matrix-core kernel still to be compiled is compiled on the first launch that would use it,
// and (GWI_BATCH_AUTOTUNE=1 only) measured against the 4-tap kernel.  Blocking.
gwi_status ensure_batch_kernel(gwi_handle h, const double* thetas, int K) {
  if (K < h->mfma_min_batch) return GWI_OK;
  if (h->mfma_jit_pending) h->batch_autotune = try_jit_mfma(h) && h->autotune_wanted;
  return h->batch_autotune && h->mfma ? calibrate_batch_path(h, thetas, K) : GWI_OK;
}

gwi_status run_pipeline(gwi_handle h, const double* theta, double* record_dev = nullptr, bool wait = true, int K = 1, bool batch = false, bool square = false) {
  gwi_status st = batch && wait && !record_dev ? ensure_batch_kernel(h, theta, K) : GWI_OK;
  if (st == GWI_OK) st = run_pipeline_once(h, theta, record_dev, wait, K, batch, square);
  if (st == GWI_OK && wait) st = repeat_after_redo(h, theta, record_dev, K, batch, square);
  return st;
}

// The AQL path has no HIP stream behind it: when the quick poll gives up, keep polling (with the queue's error flag in
// view) for up to 10 s, then report.  `ready` re-evaluates the completion condition.
template <typename Ready>
gwi_status aql_wait_slow(gwi_handle h, Ready ready, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  bool rung_again = false;
  for (unsigned long long spin = 1;; ++spin) {
    if (ready()) {
      // (said once per process: with several processes time-slicing one GPU an evaluation can simply take longer than 50 ms)
      static std::atomic<bool> said{false};
      if (rung_again && !std::getenv("GWI_QUIET") && !said.exchange(true))
        std::fprintf(stderr, "gwi: waited more than 50 ms for %s and rang the queue's doorbell again as a precaution; they arrived (a busy or shared GPU does this too)\n", what);
      return GWI_OK;
    }
    // packets of this evaluation may still be in flight: the handle takes no further evaluations, and gwi_destroy
    // waits for the queue to drain (or leaks the buffers) instead of freeing memory a kernel may still write
    if (h->aq.failed()) {
      h->poisoned = true;
      return fail(h, GWI_ERR_HIP, h->aq.why());
    }
    __builtin_ia32_pause();
    if ((spin & 0xffff) == 0) {
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      hsa_queue_t* hq = h->aq.sq ? h->aq.sq->q : nullptr;
      if (waited > 0.05 && !rung_again && hq) {
        // 50 ms without a result is ~1000 evaluations' worth: if the command processor has not taken the packets (read index
        // behind the write index), ring the doorbell once more with the last index written -- a doorbell that did not register
        // would otherwise cost the whole evaluation; ringing twice with the same index is harmless
        aql::Api& api = aql::api();
        const uint64_t w = api.add_write_index(hq, 0), r = api.load_read_index(hq);
        if (r < w) api.signal_store(hq->doorbell_signal, (hsa_signal_value_t)(w - 1));
        rung_again = true;
        h->aql_rerings++;
      }
      if (waited > 10.0) {
        h->poisoned = true;
        std::string state;
        if (hq) {
          aql::Api& api = aql::api();
          state = " (queue write index " + std::to_string((unsigned long long)api.add_write_index(hq, 0)) + ", read index " + std::to_string((unsigned long long)api.load_read_index(hq)) +
                  ", evaluation " + std::to_string((unsigned long long)h->seq) + ", doorbell rung again: " + (rung_again ? "yes" : "no") + "; normaliser stamps";
          for (int j = 0; j < h->spec.n_norms && j < 16; ++j) state += " " + std::to_string((unsigned long long)h->h_norm_stamp[j]) + ":" + std::to_string(h->h_norm[j]);
          state += "; redo word " + std::to_string((unsigned long long)*reinterpret_cast<volatile unsigned long long*>(h->h_redo)) + "; kernel " + (h->variant ? h->variant->name : "?") +
                   ", role " + std::to_string(h->scan_role) + ", blocks " + std::to_string(h->geo[0].n_scan_blocks) + ")";
        }
        return fail(h, GWI_ERR_TIMEOUT, std::string(what) + " did not arrive from the AQL queue within 10 s" + state);
      }
    }
  }
}

// The skeleton of every wait for results in pinned host memory.  ready() says whether they have all arrived (it may keep a cursor:
// what has arrived stays).  A bounded quick poll (~2 ms) instead of paying a stream synchronise; then the slow wait of the AQL
// path, or the blocking call on the stream path (which also surfaces any error) and one more look; then the acquire fence ahead
// of the caller's reads.  `gated`: the quick poll only without timing and with spin_wait.  `grace`: results that are posted
// writes behind the stream's completion get that many more polls to land after the synchronise.
template <typename Ready>
gwi_status wait_until(gwi_handle h, bool gated, long grace, Ready ready, const char* what, const char* mismatch) {
  bool done = false;
  if (!gated || (!h->timing && h->spin_wait))
    for (long spin = 0; spin < 400000 && !(done = ready()); ++spin) __builtin_ia32_pause();
  if (!done && h->aql_now) {
    const gwi_status sw = aql_wait_slow(h, ready, what);
    if (sw != GWI_OK) return sw;
  } else if (!done) {
    GWI_HIP(hipStreamSynchronize(h->stream));
    for (long spin = 0; spin < grace && !ready(); ++spin) __builtin_ia32_pause();
    if (!ready()) return fail(h, GWI_ERR_HIP, mismatch);
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return GWI_OK;
}

// with gwi_set_timing: the kernel times of the evaluation just waited for, from the AQL queue's dispatch timestamps or the HIP events
gwi_status collect_kernel_times(gwi_handle h) {
  if (!h->timing) return GWI_OK;
  const int n_launches = h->timed_final ? 3 : 2;
  h->last_ms[2] = 0.0f;  // host-final mode has no third launch
  if (h->aql_now) return aql::timed_collect(h->aq, n_launches, h->last_ms) ? GWI_OK : fail(h, GWI_ERR_HIP, "dispatch timestamps of the AQL queue are not available");
  GWI_HIP(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n_launches; ++i) GWI_HIP(hipEventElapsedTime(&h->last_ms[i], h->ev[2 * i], h->ev[2 * i + 1]));
  return GWI_OK;
}

// the normaliser launch publishes Z_j + a stamp per normaliser; copy them into rank 0's record slots (point k's at
// record + k * stride; stride 0: one record per point)
gwi_status wait_for_norms(gwi_handle h, double* record, int K = 1, size_t stride = 0) {
  const int n = h->spec.n_norms;
  if (n == 0) return GWI_OK;
  const int total = n * K;
  const gwi_status sw = wait_until(h, /*gated=*/false, /*grace=*/0, [&] {
    for (int j = 0; j < total; ++j)
      if (*reinterpret_cast<volatile unsigned long long*>(h->h_norm_stamp + j) != h->seq) return false;
    return true;
  }, "normaliser stamps", "normaliser stamp mismatch after stream synchronise");
  if (sw != GWI_OK) return sw;
  const size_t step = stride ? stride : (size_t)record_len(h);
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < n; ++j) record[(size_t)k * step + kRecNormOff + j] = h->h_norm[k * n + j];
  return GWI_OK;
}

// n partial records (one after the other, `len` doubles each) merged into one: sums, the minimum, the injection triples brought
// to their common exponent M, gradients in record order (g_pe, g_inj: n_theta sums each, overwritten).  Workgroups of one launch
// and ranks of one exchange are merged by this one loop, so a record means the same whoever summed it.  `marked`: the records
// are a launch's workgroups', whose event count (slot 7) carries the repeat mark as -(count + 1); a rank's is read as it stands.
struct MergedRecord {
  double sum_lse = 0.0, sum_var = 0.0, min_lneff = INFINITY, n_ev = 0.0, M = -INFINITY, S1 = 0.0, S2 = 0.0;
  bool redo = false;
};
GWI_HOT MergedRecord merge_records(const gwi_engine* h, const double* records, int n, bool marked, double* g_pe, double* g_inj) {
  const int n_theta = h->spec.n_theta, n_norms = h->spec.n_norms;
  const size_t len = (size_t)record_len(h);
  MergedRecord m;
  for (int i = 0; i < n; ++i) {
    const double* r = records + (size_t)i * len;
    const bool mark = marked && r[7] < 0.0;
    m.sum_lse += r[1];
    m.sum_var += r[2];
    m.min_lneff = std::fmin(m.min_lneff, r[3]);
    m.M = std::fmax(m.M, r[4]);
    m.redo = m.redo || mark;
    m.n_ev += mark ? -r[7] - 1.0 : r[7];
  }
  for (int p = 0; p < n_theta; ++p) g_pe[p] = g_inj[p] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double* r = records + (size_t)i * len;
    const double f = (r[4] == -INFINITY) ? 0.0 : std::exp(r[4] - m.M);
    m.S1 += f * r[5];
    m.S2 += f * f * r[6];
    const double* gp = r + kRecNormOff + n_norms;
    const double* gi = gp + n_theta;
    for (int p = 0; p < n_theta; ++p) {
      g_pe[p] += gp[p];
      g_inj[p] += f * gi[p];
    }
  }
  return m;
}

// Device-final mode: the G partial records of point k (h_fin) -> one record (h_record)
void merge_final_records(gwi_handle h, int K) {
  const int G = h->final_groups;
  const size_t len = (size_t)record_len(h);
  for (int k = 0; k < K; ++k) {
    double* out = h->h_record + (size_t)k * len;
    double* gpe = out + kRecNormOff + h->spec.n_norms;
    const MergedRecord m = merge_records(h, h->h_fin + (size_t)k * G * len, G, /*marked=*/true, gpe, gpe + h->spec.n_theta);
    out[1] = m.sum_lse;
    out[2] = m.sum_var;
    out[3] = m.min_lneff;
    out[4] = m.M;
    out[5] = m.S1;
    out[6] = m.S2;
    out[7] = m.redo ? -(m.n_ev + 1.0) : m.n_ev;
  }
}

// Completion: final_kernel (or the kernel that publishes gathered records) stores the sequence stamp into pinned host memory LAST
// (system-scope release after __threadfence_system), so the host can poll it.  Stamp k sits at host_buf + k * stride (stride 0:
// one record per stamp).
gwi_status wait_for_stamp(gwi_handle h, double* host_buf, int K = 1, size_t stride = 0) {
  const size_t len = stride ? stride : (size_t)record_len(h);
  int k = 0;  // the stamps before it have been seen
  const gwi_status sw = wait_until(h, /*gated=*/true, /*grace=*/0, [&] {
    while (k < K && *reinterpret_cast<volatile unsigned long long*>(host_buf + (size_t)k * len) == h->seq) ++k;
    return k == K;
  }, "the completion stamp", "completion stamp mismatch after stream synchronise");
  return sw == GWI_OK ? collect_kernel_times(h) : sw;
}

// Assemble the sites of analysis.py:259-319 from gathered per-rank records.
// `records_sq` (same layout, from a pass run with KArgs::square): its injection slots hold the sums
// weighted by w^2, which the gradient of the marginalised selection term needs; nullptr otherwise.
void assemble(const gwi_engine* h, const double* records, int n_ranks, const gwi_options* opt, gwi_summary* out, double* grad, double* norms,
              double host_const, const double* records_sq = nullptr) {
  const int n_theta = h->spec.n_theta, n_norms = h->spec.n_norms;
  const int len = record_len(h);
  const double NEG_BIG = -1.7976931348623157e308;  // jnp.nan_to_num(-inf)
  std::vector<double> g_pe(n_theta), g_inj(n_theta);
  const MergedRecord merged = merge_records(h, records, n_ranks, /*marked=*/false, g_pe.data(), g_inj.data());
  const double sum_lse = merged.sum_lse, sum_var = merged.sum_var, min_lneff = merged.min_lneff, n_ev_total = merged.n_ev, M = merged.M, S1 = merged.S1, S2 = merged.S2;
  const double* nrm = records + kRecNormOff;  // every rank integrates the same grids
  double log_const = host_const;
  for (int t = 0; t < h->spec.n_terms; ++t)
    if (h->spec.terms[t].norm >= 0) log_const -= std::log(nrm[h->spec.terms[t].norm]);
  if (norms)
    for (int j = 0; j < n_norms; ++j) norms[j] = nrm[j];

  const double n_obs = opt->n_obs, n_tot = opt->total_inj, n_pe = (double)h->n_pe;
  gwi_summary s;
  std::memset(&s, 0, sizeof(s));
  s.log_norm_const = log_const;
  s.sum_logBFs = sum_lse + n_ev_total * (log_const - std::log(n_pe));
  // detection_efficiency (analysis.py:124-136), scale-free forms of var and n_eff
  const double log_mu = std::log(S1) + M - std::log(n_tot) + log_const;
  const double log_neff_inj = 2.0 * std::log(S1) - std::log(S2 - S1 * S1 / n_tot);
  const double var_mu = 1.0 / std::exp(log_neff_inj) - 1.0 / n_tot;
  s.log_det_eff = log_mu;
  s.log_nEff_inj = log_neff_inj;
  s.variance_log_detection_efficiency = var_mu;
  s.min_log_nEff = min_lneff;
  s.surveyed_hypervolume_norm = h->spec.vt_norm >= 0 ? nrm[h->spec.vt_norm] : NAN;
  double lde = log_mu;
  if (opt->marginalize_selection) lde = lde - (3.0 + n_obs) / (2.0 * std::exp(log_neff_inj));  // :271
  bool cut = false;
  if (opt->min_neff_cut && !(log_neff_inj >= std::log(4.0 * n_obs))) lde = INFINITY;  // :273-277
  s.selection_factor = std::isinf(lde) ? NEG_BIG : -n_obs * lde;                       // :278-281
  if (std::isinf(lde)) cut = true;
  double log_l = s.selection_factor + s.sum_logBFs;
  if (std::isnan(log_l)) {
    log_l = NEG_BIG;  // :287-288
    cut = true;
  } else if (std::isinf(log_l)) {
    log_l = log_l > 0 ? 1.7976931348623157e308 : NEG_BIG;  // nan_to_num :289
    cut = true;
  }
  s.log_l = log_l;
  if (opt->min_neff_cut) {
    const double min_neff = std::exp(min_lneff);  // :295
    if (min_neff <= n_obs) {                      // :296-303
      log_l = NEG_BIG;
      cut = true;
    }
  }
  s.variance_log_likelihood = n_obs * n_obs * var_mu + sum_var;  // :305-308
  if (opt->max_variance_cut && !(s.variance_log_likelihood <= 1.0)) {  // :309-317
    log_l = NEG_BIG;
    cut = true;
  }
  s.log_likelihood = log_l;
  if (out) *out = s;
  if (grad) {
    // d log_l / d theta = sum_i sum_j s_ij dl_ij - N_obs sum_j s_j dl_j  (SURVEY.md appendix A);
    // a cut replaces log_l by a constant, whose gradient is zero.
    for (int p = 0; p < n_theta; ++p) grad[p] = cut ? 0.0 : g_pe[p] - n_obs * (S1 > 0 ? g_inj[p] / S1 : 0.0);
    if (opt->marginalize_selection && records_sq && !cut && S1 > 0) {
      // lde = log mu - c / n_eff, c = (3 + N_obs)/2 (analysis.py:271);  log n_eff = 2 log S1 - log V,
      // V = S2 - S1^2/N_tot;  dS1 = G (sum w dl), dS2 = 2 H (H = sum w^2 dl, from the squared pass)
      double M2 = -INFINITY;
      for (int r = 0; r < n_ranks; ++r) M2 = std::fmax(M2, records_sq[(size_t)r * len + 4]);
      std::vector<double> H(n_theta, 0.0);
      for (int r = 0; r < n_ranks; ++r) {
        const double* rec = records_sq + (size_t)r * len;
        const double f2 = (rec[4] == -INFINITY) ? 0.0 : std::exp(rec[4] - M2);
        const double* gi = rec + kRecNormOff + n_norms + n_theta;
        for (int p = 0; p < n_theta; ++p) H[p] += f2 * gi[p];
      }
      // S1, S2 and g_inj are in units of e^M (e^2M for S2), H in units of e^M2: each pass reports the exponent its own records
      // were brought to, and nothing makes M2 equal 2 M (the two passes normalise their tile records independently)
      const double h_scale = (M2 == -INFINITY || M == -INFINITY) ? 0.0 : std::exp(M2 - 2.0 * M);
      const double V = S2 - S1 * S1 / n_tot;
      const double c_over_neff = (3.0 + n_obs) / (2.0 * std::exp(log_neff_inj));
      for (int p = 0; p < n_theta; ++p) {
        const double dlog_neff = 2.0 * g_inj[p] / S1 - (2.0 * h_scale * H[p] - 2.0 * S1 * g_inj[p] / n_tot) / V;
        grad[p] -= n_obs * c_over_neff * dlog_neff;
      }
    }
  }
}

// Host-final mode: poll every group's stamp, then do what final_kernel does (fixed summation order)
// into h_record so that assemble() is shared with the device-final and sharded paths.
gwi_status wait_for_rows(gwi_handle h, int K) {
  const int n_groups = (int)h->n_ev + h->geo[0].n_inj_groups;
  const int n_theta = h->spec.n_theta, n_lines = (3 + n_theta + 6) / 7, stride = 8 * n_lines;
  const size_t total_lines = (size_t)n_groups * K * n_lines;
  // every 64-byte line carries the evaluation's sequence number in its eighth slot
  size_t seen = 0;  // the lines before it carry it
  // (the lines are posted writes behind the stream's completion: after a synchronise the last ones get a moment to land)
  gwi_status sw = wait_until(h, /*gated=*/true, /*grace=*/4000000, [&] {
    while (seen < total_lines && *reinterpret_cast<volatile unsigned long long*>(h->h_rows + seen * 8 + 7) == h->seq) ++seen;
    return seen == total_lines;
  }, "group result rows", "group row stamp mismatch after stream synchronise");
  if (sw == GWI_OK) sw = collect_kernel_times(h);
  if (sw != GWI_OK) return sw;
  const int n_ev = (int)h->n_ev, n_norms = h->spec.n_norms, len = record_len(h);
  for (int k = 0; k < K; ++k) {
    double* r = h->h_record + (size_t)k * len;
    const double* rows = h->h_rows + (size_t)k * n_groups * stride;
    // a group's row unpacked from its 64-byte lines (seven values + the sequence number each) into row[0 .. 3 + n_theta):
    // the sums below then run over contiguous values (index arithmetic per value -- i / 7, i % 7 -- cost config 3, 79 rows
    // of 56 values, 1.4 us per evaluation)
    double row[3 + GWI_MAX_THETA + 7];
    auto unpack = [&](int g) {
      const double* src = rows + (size_t)g * stride;
      for (int l = 0; l < n_lines; ++l) std::memcpy(row + 7 * l, src + 8 * l, 7 * sizeof(double));
    };
    double* ev = h->h_ev + (size_t)k * 3 * n_ev;
    double sum = 0.0, var = 0.0, mn = INFINITY;
    double* gpe = r + kRecNormOff + n_norms;
    double* ginj = gpe + n_theta;
    for (int p = 0; p < n_theta; ++p) gpe[p] = ginj[p] = 0.0;
    for (int e = 0; e < n_ev; ++e) {
      unpack(e);
      const double lse = row[0], lneff = row[1], v = row[2];
      sum += lse;
      var += v;
      double le = lneff;  // jnp.min(jnp.nan_to_num(logn_effs)) (analysis.py:295)
      if (le != le) le = 0.0;
      le = std::fmin(std::fmax(le, -1.7976931348623157e308), 1.7976931348623157e308);
      mn = std::fmin(mn, le);
      ev[e] = lse;
      ev[n_ev + e] = lneff;
      ev[2 * n_ev + e] = v;
      for (int p = 0; p < n_theta; ++p) gpe[p] += row[3 + p];
    }
    double M = -INFINITY;
    for (int j = 0; j < h->geo[0].n_inj_groups; ++j) M = std::fmax(M, rows[(size_t)(n_ev + j) * stride]);
    double S1 = 0.0, S2 = 0.0;
    for (int j = 0; j < h->geo[0].n_inj_groups; ++j) {
      unpack(n_ev + j);
      const double mj = row[0];
      const double f = (mj == -INFINITY) ? 0.0 : std::exp(mj - M);
      S1 += f * row[1];
      S2 += f * f * row[2];
      for (int p = 0; p < n_theta; ++p) ginj[p] += f * row[3 + p];
    }
    r[1] = sum;
    r[2] = var;
    r[3] = mn;
    r[4] = M;
    r[5] = S1;
    r[6] = S2;
    r[7] = (double)n_ev;
  }
  return wait_for_norms(h, h->h_record, K);
}

// The only place that turns this rank's launched evaluation of K points into h_record, h_ev and the normalisers: from the result
// rows where the launch published rows, else from the final launch's records.
GWI_HOT gwi_status collect_local(gwi_handle h, int K) {
  if (h->last_host_rows) return wait_for_rows(h, K);
  const gwi_status st = wait_for_stamp(h, h->h_fin, K * h->final_groups);
  if (st != GWI_OK) return st;
  merge_final_records(h, K);
  return wait_for_norms(h, h->h_record, K);
}

// ... and its counterpart behind the in-engine RCCL exchange: the ranks' records of K points in h_gather, [K][world][len]
gwi_status wait_for_gathered(gwi_handle h, int K) {
  const size_t stride = (size_t)record_len(h) * (size_t)h->comm_world;
  const gwi_status st = wait_for_stamp(h, h->h_gather, K, stride);
  if (st != GWI_OK) return st;
  return wait_for_norms(h, h->h_gather, K, stride);  // every rank integrates the same grids: rank 0's slots of each point are what assemble() reads
}

void destroy_impl(gwi_engine* h) {
  if (!h) return;
  struct VariantGuard {  // the variant record of a run-time compiled chain goes with the handle (the chain itself is process-wide)
    Variant* v;
    ~VariantGuard() { delete v; }
  } guard{h->jit_variant};
  h->jit_variant = nullptr;
  struct MfmaGuard {
    MfmaVariant* v;
    ~MfmaGuard() { delete v; }
  } mguard{h->jit_mfma};
  h->jit_mfma = nullptr;
  if (h->host_only) {
    if (h->shm_base) munmap(h->shm_base, h->shm_bytes);
    delete h;
    return;
  }
  (void)hipSetDevice(h->device);
  if (h->shm_base) munmap(h->shm_base, h->shm_bytes);
  if (h->poisoned && !aql::drain(h->aq, 2.0)) {
    // a kernel of the timed-out evaluation may still be running: leak the device buffers rather than free them under it
    aql::abandon_queue(h->aq);
    (void)new PostprocessBuffers(std::move(h->post));  // (out of the handle's reach and never destroyed)
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return;
  }
  if (h->poisoned) (void)hipDeviceSynchronize();
  aql::close_queue(h->aq);
  for (double* p : h->d_cols_pe) (void)hipFree(p);  // each holds both sample sets (alloc_pair); d_cols_inj are interior pointers
  for (double* p : h->d_norm_arrays) (void)hipFree(p);
  (void)hipFree(h->d_norms);
  (void)hipFree(h->d_partials);
  (void)hipFree(h->d_ev_out);
  (void)hipFree(h->d_ev_grad);
  (void)hipFree(h->d_inj_out);
  (void)hipFree(h->d_inj_grad);
  h->post = PostprocessBuffers();
  h->rank = RankBuffers();
  release_moment_and_conditional_buffers(h);
  if (h->nccl_comm && g_nccl.CommDestroy) (void)g_nccl.CommDestroy(h->nccl_comm);
  (void)hipFree(h->d_send);
  (void)hipFree(h->d_recv);
  if (h->h_gather) (void)hipHostFree(h->h_gather);
  if (h->h_record) (void)hipHostFree(h->h_record);
  if (h->h_fin) (void)hipHostFree(h->h_fin);
  if (h->h_ev) (void)hipHostFree(h->h_ev);
  if (h->h_rows) (void)hipHostFree(h->h_rows);
  if (h->h_norm) (void)hipHostFree(h->h_norm);
  if (h->h_norm_stamp) (void)hipHostFree(h->h_norm_stamp);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  (void)hipFree(h->d_tblocks);
  (void)hipFree(h->d_seq);
  (void)hipFree(h->d_tile_nref);
  if (h->h_redo) (void)hipHostFree(h->h_redo);
  if (h->h_tblocks) (void)hipHostFree(h->h_tblocks);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

gwi_status upload(gwi_handle h, const double* src, size_t n, double** dst, std::vector<double*>* keep) {
  double* d = nullptr;
  GWI_HIP(hipMalloc(&d, sizeof(double) * (n ? n : 1)));
  keep->push_back(d);
  if (n) GWI_HIP(hipMemcpy(d, src, sizeof(double) * n, hipMemcpyHostToDevice));
  *dst = d;
  return GWI_OK;
}

// One allocation per column for BOTH sample sets: the posterior samples first, the injections inj_offset() elements behind
// (a 256-byte boundary).  The scan addresses either set through the same pointer (ScanHead, gwi_device.h).  d_cols_pe owns
// the allocations; d_cols_inj holds the interior pointers.
gwi_status alloc_pair(gwi_handle h, double** dpe, double** dinj) {
  double* d = nullptr;
  const size_t n = (size_t)h->inj_off + (size_t)(h->n_inj ? h->n_inj : 1);
  GWI_HIP(hipMalloc(&d, sizeof(double) * n));
  h->d_cols_pe.push_back(d);
  h->d_cols_inj.push_back(d + h->inj_off);
  h->col_f32.push_back(0);
  *dpe = d;
  *dinj = d + h->inj_off;
  return GWI_OK;
}
// The same for a NARROW column in slot c of d_cols_pe (an allocation of float32: the injections inj_offset() FLOAT elements
// behind, as the scan's narrow loads count them, gwi_device.h: gload_f32); the slot's previous allocation is handed back in
// `old`, for the caller to release once nothing reads it.
gwi_status alloc_pair_f32(gwi_handle h, int c, float** dpe, double** old) {
  float* d = nullptr;
  const size_t n = (size_t)h->inj_off + (size_t)(h->n_inj ? h->n_inj : 1);
  GWI_HIP(hipMalloc(&d, sizeof(float) * n));
  *old = h->d_cols_pe[c];
  h->d_cols_pe[c] = reinterpret_cast<double*>(d);
  h->d_cols_inj[c] = reinterpret_cast<double*>(d + h->inj_off);
  h->col_f32[c] = 1;
  *dpe = d;
  return GWI_OK;
}

// Every evaluating entry point: the handle must not hold an uncollected gwi_eval_begin (its kernel arguments, sequence
// stamp and dispatch path would be overwritten under the evaluation in flight) and must not be poisoned by a time-out.
gwi_status busy_guard(gwi_handle h, const char* who) {
  if (h->poisoned) return fail(h, GWI_ERR_INVALID, std::string(who) + ": an earlier evaluation of this handle timed out or its queue failed; destroy the handle");
  if (h->pending) return fail(h, GWI_ERR_INVALID, std::string(who) + ": an evaluation begun with gwi_eval_begin has not been collected (gwi_eval_end)");
  return GWI_OK;
}

// What the evaluating entries refuse, in their common order: null arguments (with them the handle without a scan kernel, and a
// count below 1; no message), a sharded entry without its exchange, a count above max_batch, the options, a host-only handle,
// a busy or poisoned one.
gwi_status check_options(gwi_handle h, const gwi_options* opt) {
  if (opt->max_variance_cut && (opt->marginalize_selection || opt->min_neff_cut))
    return fail(h, GWI_ERR_INVALID, "max_variance_cut requires marginalize_selection and min_neff_cut to be off (analysis.py:237-243)");
  return GWI_OK;
}
gwi_status check_exchange(gwi_handle h) {
  return h->nccl_comm || h->shm_base ? GWI_OK : fail(h, GWI_ERR_INVALID, "neither gwi_shm_comm_init nor gwi_comm_init has been called");
}
constexpr int kMaxBatchCap = 64;  // what gwi_create clamps max_batch to: the points an entry may hold results of on its stack (finish_points)
gwi_status check_batch_size(gwi_handle h, int k, const char* name) {
  return k <= h->max_batch ? GWI_OK : fail(h, GWI_ERR_INVALID, std::string(name) + " exceeds the engine's max_batch (GWI_MAX_BATCH, default 16)");
}
// ... its last part; leaves the calling thread on the handle's device
gwi_status eval_preflight(gwi_handle h, const char* who) {
  if (h->host_only) return fail(h, GWI_ERR_NO_DEVICE, "host-only handle: no device to evaluate on");
  const gwi_status st = busy_guard(h, who);
  if (st != GWI_OK) return st;
  GWI_HIP(hipSetDevice(h->device));
  return GWI_OK;
}

// point k's result from records[k][n_ranks][len] (the ranks' records of point k in rank order, as gwi_combine reads them)
GWI_HOT void assemble_points(gwi_handle h, const double* records, const double* records_sq, int n_ranks, int K, const gwi_options* opt, const double* consts,
                     gwi_summary* summaries, double* grads, double* norms) {
  const size_t blk = (size_t)n_ranks * record_len(h);
  const int n_theta = h->spec.n_theta, n_norms = h->spec.n_norms;
  for (int k = 0; k < K; ++k) {
    gwi_summary s;
    assemble(h, records + k * blk, n_ranks, opt, &s, grads ? grads + (size_t)k * n_theta : nullptr, norms ? norms + (size_t)k * n_norms : nullptr, consts[k],
             records_sq ? records_sq + k * blk : nullptr);
    if (summaries) summaries[k] = s;
  }
}

// this rank's per-event sites of K collected points (h_ev) into the caller's arrays: with the global constant of point k's assembled
// summary, logBF_i = logsumexp_i - log N_pe (analysis.py:80); without summaries as they are (the caller adds it after gwi_combine)
GWI_HOT void local_sites(gwi_handle h, int K, const gwi_summary* summaries, double* log_bfs, double* log_neffs, double* variances) {
  const size_t n = (size_t)h->n_ev;
  for (int k = 0; k < K; ++k) {
    const double* ev = h->h_ev + (size_t)k * 3 * n;
    if (log_bfs && summaries) {
      const double shift = summaries[k].log_norm_const - std::log((double)h->n_pe);
      for (size_t i = 0; i < n; ++i) log_bfs[k * n + i] = ev[i] + shift;
    } else if (log_bfs) {
      std::memcpy(log_bfs + k * n, ev, sizeof(double) * n);
    }
    if (log_neffs) std::memcpy(log_neffs + k * n, ev + n, sizeof(double) * n);
    if (variances) std::memcpy(variances + k * n, ev + 2 * n, sizeof(double) * n);
  }
}

// The end of every entry that assembles on this handle: K points (at most max_batch <= kMaxBatchCap) from the ranks' records of the last
// exchange, or this rank's own with n_ranks = 1, under the constants of the last prelude; then this rank's sites.
GWI_HOT void finish_points(gwi_handle h, const double* records, const double* records_sq, int n_ranks, int K, const gwi_options* opt, gwi_summary* summaries, double* grads,
                   double* log_bfs, double* log_neffs, double* variances, double* norms) {
  gwi_summary s[kMaxBatchCap];
  assemble_points(h, records, records_sq, n_ranks, K, opt, h->host_consts.data(), s, grads, norms);
  if (summaries) std::memcpy(summaries, s, sizeof(gwi_summary) * K);
  local_sites(h, K, s, log_bfs, log_neffs, variances);
}

// ---- the scaffold of the post-processing entries ----------------------------------------------------------------------------------

// What the handle-bound entries refuse, in their common order: a host-only handle ("no device to <no_device_to>"), the entry's own
// arguments (bad_args() names what is wrong with them, or returns an empty string), a handle that holds a shard ("<global_set_for>
// the global set"), a handle that is busy or poisoned.
template <class ArgCheck>
gwi_status post_preflight(gwi_handle h, const char* who, const char* no_device_to, const char* global_set_for, ArgCheck&& bad_args) {
  const std::string entry = std::string(who) + ": ";
  if (h->host_only) return fail(h, GWI_ERR_INVALID, entry + "host-only handle: no device to " + no_device_to);
  const std::string why = bad_args();
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, entry + why);
  if (h->comm_world > 1 || h->shm_world > 1) return fail(h, GWI_ERR_UNSUPPORTED, entry + "this handle holds one shard of the catalog; " + global_set_for + " the global set");
  return busy_guard(h, who);
}

// puts the calling thread back on the device it was on when the scope ends.  Declared before an entry's buffers: they are freed on
// `device`, then the thread goes back
struct DeviceScope {
  int previous = -1;
  ~DeviceScope() {
    if (previous >= 0) (void)hipSetDevice(previous);
  }
  gwi_status select(int32_t device) {  // (device < 0: the current one)
    int n_dev = 0, current = -1;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return GWI_ERR_NO_DEVICE;
    if (device >= n_dev) return GWI_ERR_NO_DEVICE;
    if (device < 0) return GWI_OK;
    if (hipGetDevice(&current) != hipSuccess) return GWI_ERR_HIP;
    if (current == device) return GWI_OK;
    if (hipSetDevice(device) != hipSuccess) return GWI_ERR_HIP;
    previous = current;
    return GWI_OK;
  }
};

// a failed call of an entry without a handle: "<entry>: <call>: <hip error string>" on stderr and GWI_ERR_HIP (`sc` is the
// entry's LaunchScratch)
#define GWI_SCRATCH_HIP(call)                                  \
  do {                                                         \
    if (sc.failed((call), #call)) return GWI_ERR_HIP;          \
  } while (0)

// device buffers, a stream and events that go away with the scope
struct LaunchScratch {
  const char* where;  // the entry, for the line a failed call prints
  std::vector<void*> bufs;
  hipStream_t stream = nullptr;
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  explicit LaunchScratch(const char* entry) : where(entry) {}
  LaunchScratch(const LaunchScratch&) = delete;
  ~LaunchScratch() {
    for (void* b : bufs) (void)hipFree(b);
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
    if (stream) (void)hipStreamDestroy(stream);
  }
  template <class T>
  T* alloc(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) return nullptr;
    bufs.push_back(p);
    return (T*)p;
  }
  hipError_t events(int n) {  // (an entry that launches on its engine's stream opens these only)
    hipError_t err = hipSuccess;
    for (int i = 0; i < n && err == hipSuccess; ++i) err = hipEventCreate(&e[i]);
    return err;
  }
  bool open() { return hipStreamCreate(&stream) == hipSuccess && events(2) == hipSuccess; }
  bool failed(hipError_t err, const char* call) const {
    if (err != hipSuccess) std::fprintf(stderr, "%s: %s: %s\n", where, call, hipGetErrorString(err));
    return err != hipSuccess;
  }
  // launch() between the two events on the scope's stream
  template <class Launch>
  gwi_status enqueue_timed(Launch&& launch) {
    LaunchScratch& sc = *this;
    GWI_SCRATCH_HIP(hipEventRecord(e[0], stream));
    launch();
    GWI_SCRATCH_HIP(hipGetLastError());
    GWI_SCRATCH_HIP(hipEventRecord(e[1], stream));
    return GWI_OK;
  }
  // ... waited for: *ms is the time between the events
  template <class Launch>
  gwi_status timed(Launch&& launch, float* ms) {
    LaunchScratch& sc = *this;
    const gwi_status st = enqueue_timed(launch);
    if (st != GWI_OK) return st;
    GWI_SCRATCH_HIP(hipEventSynchronize(e[1]));
    GWI_SCRATCH_HIP(hipEventElapsedTime(ms, e[0], e[1]));
    return GWI_OK;
  }
  // ... with what after() enqueues behind it (the copies of its results), and the whole stream waited for
  template <class Launch, class After>
  gwi_status timed(Launch&& launch, After&& after, float* ms) {
    LaunchScratch& sc = *this;
    gwi_status st = enqueue_timed(launch);
    if (st == GWI_OK) st = after();
    if (st != GWI_OK) return st;
    GWI_SCRATCH_HIP(hipStreamSynchronize(stream));
    GWI_SCRATCH_HIP(hipEventElapsedTime(ms, e[0], e[1]));
    return GWI_OK;
  }
};

// up to three times of a feature's last call on the calling thread, and its launches; every feature has an instance of its own
struct StageTimes {
  double ms[3] = {0.0, 0.0, 0.0};
  int launches = 0;
  void report(double* ms0, double* ms1, double* ms2, int32_t* n) const {
    if (ms0) *ms0 = ms[0];
    if (ms1) *ms1 = ms[1];
    if (ms2) *ms2 = ms[2];
    if (n) *n = launches;
  }
};

// why a feature's last call on the calling thread was refused
struct ErrorSlot {
  std::string text;
  gwi_status refuse(const std::string& why) {
    text = why;
    return GWI_ERR_INVALID;
  }
};

// A grid of rows x items cut into launches: at most items_cap items of a row per launch (rounded up to whole workgroups they are
// its lanes), and as many rows as 65535 (grid.y) and lane_budget lanes allow, at least one
struct LaunchCut {
  long long items_max, rows_max;
};
LaunchCut launch_cut(long long n_rows, long long n_items, long long items_cap, long long lane_budget, int block) {
  const long long items_max = std::min<long long>(n_items, items_cap);
  const long long lanes_per_row = (items_max + block - 1) / block * block;
  return {items_max, std::max<long long>(1, std::min<long long>(std::min<long long>(n_rows, 65535), lane_budget / lanes_per_row))};
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int32_t gwi_abi_version(void) { return GWI_ABI_VERSION; }
int32_t gwi_kernel_variants(void) { return kNumVariants; }
const char* gwi_kernel_variant_name(int32_t i) { return (i >= 0 && i < kNumVariants) ? kVariants[i].name : nullptr; }
const char* gwi_scan_kernel_name(gwi_handle h) { return (h && h->variant) ? h->variant->name : "none"; }

const char* gwi_last_error(gwi_handle h) {
  static const char* none = "";
  static const char* null_handle = "null handle (gwi_create failed before an engine existed: no HIP device?)";
  if (!h) return null_handle;
  return h->err.empty() ? none : h->err.c_str();
}

void gwi_destroy(gwi_handle h) { destroy_impl(h); }

// The engine's AQL queue (gwi_aql.h).  Never fatal: on any failure the note says why and the HIP stream is used.
static void setup_aql(gwi_engine* h, const hipDeviceProp_t& prop) {
  h->aql_active = false;
  if (const char* env = std::getenv("GWI_AQL"))
    if (std::atoi(env) == 0) {
      h->aql_note = "disabled by GWI_AQL=0";
      return;
    }
  std::string code = "gwi_kernels.hsaco";
  if (const char* env = std::getenv("GWI_AQL_CODE")) {
    code = env;
  } else {
    Dl_info info;
    if (dladdr(reinterpret_cast<const void*>(&gwi_abi_version), &info) && info.dli_fname) {
      const std::string so = info.dli_fname;
      const size_t cut = so.find_last_of('/');
      code = (cut == std::string::npos ? std::string(".") : so.substr(0, cut)) + "/gwi_kernels.hsaco";
    }
  }
  aql::Device* dev = aql::open_device((uint32_t)prop.pciDomainID, (uint32_t)prop.pciBusID, (uint32_t)prop.pciDeviceID, 0u, code);
  if (!dev->ok) {
    h->aql_note = dev->why;
    return;
  }
  // the scan kernels of a chain compiled at gwi_create come out of its own code object, loaded into a second executable
  hsa_executable_t jit_exe{};
  jit::Chain* jc = h->variant->jit;
  if (jc) {
    std::lock_guard<std::mutex> lock(jc->mu);
    bool have = false;
    for (auto& kv : jc->hsa_executables)
      if (kv.first == dev) jit_exe.handle = kv.second, have = true;
    if (!have) {
      if (!aql::load_code(dev, jc->code.data(), jc->code.size(), jit_exe, h->aql_note)) return;
      jc->hsa_executables.emplace_back(dev, jit_exe.handle);
    }
  }
  auto find_scan = [&](int role, aql::Kernel& out) {
    if (!h->variant->has(role)) return false;
    if (jc) return aql::find_kernel(dev, jc->lowered[role].c_str(), out, h->aql_note, &jit_exe);
    return aql::find_kernel(dev, hipKernelNameRefByPtr(reinterpret_cast<const void*>(h->variant->fn[role]), h->stream), out, h->aql_note);
  };
  if (!find_scan(jit::kScan, h->aq_scan)) return;
  if (!aql::find_kernel(dev, hipKernelNameRefByPtr(reinterpret_cast<const void*>(&combine_kernel), h->stream), h->aq_combine, h->aql_note)) return;
  if (!aql::find_kernel(dev, hipKernelNameRefByPtr(reinterpret_cast<const void*>(&final_kernel), h->stream), h->aq_final, h->aql_note)) return;
  if (h->variant->has(jit::kSafe) && !find_scan(jit::kSafe, h->aq_scan_safe)) return;
  if (h->aq_scan.kernarg_bytes != sizeof(ScanBlock) || h->aq_combine.kernarg_bytes != sizeof(TailArgs) || h->aq_final.kernarg_bytes != sizeof(TailArgs)) {
    h->aql_note = "kernel argument sizes of the code object differ from this build (stale gwi_kernels.hsaco?)";
    return;
  }
  bool have_batch_kernel = find_scan(jit::kBatch, h->aq_scan_batch);
  // the batched launches of a parametric model are pbatch launches wherever their tiles are single trips: both kernels or neither
  h->aq_have_pbatch = h->variant->has(jit::kPbatch) && find_scan(jit::kPbatch, h->aq_scan_pbatch);
  if (h->pbatch && !h->aq_have_pbatch) have_batch_kernel = false;
  if (!aql::open_queue(dev, h->aq, h->aql_note)) return;
  if (have_batch_kernel && sizeof(ThetaBlock) * (size_t)h->max_batch <= aql::kExtraBytes) {
    for (int ev = 0; ev < 2; ++ev) {
      TailArgs tb = tail_args(h, nullptr, h->geo[1].distinct ? 1 : 0);
      tb.host_rows = nullptr;
      tb.publish_events = ev;
      h->aq_tail_batch[ev] = aql::stage_args(h->aq, aql::kSlots - 2 - ev, &tb, sizeof(tb));
    }
    h->aql_batch = h->aq_tail_batch[0] && h->aq_tail_batch[1];
    if (const char* env = std::getenv("GWI_AQL_BATCH")) h->aql_batch = h->aql_batch && std::atoi(env) != 0;
  }
  {
    const TailArgs ta = tail_args(h, nullptr);  // the AQL path never publishes to a device record (that is the RCCL exchange, on the HIP stream)
    h->aq_tail_args = aql::stage_args(h->aq, aql::kSlots - 1, &ta, sizeof(ta));
    if (!h->aq_tail_args) {
      h->aql_note = "staging the tail kernels' arguments failed";
      return;
    }
  }
  if (const char* env = std::getenv("GWI_AQL_TAIL")) h->aql_tail_only = std::atoi(env) != 0;
  if (const char* env = std::getenv("GWI_AQL_COMBINE_ACQUIRE")) h->combine_acquire = std::atoi(env) != 0;
  h->aql_active = true;
  h->aql_note = "active";
}

// ---- gwi_create / gwi_create_ingest: the columns either come from the host ready-made (pe_cols / inj_cols) or are computed
// on the device from raw sources by the two setup programs (gwi_ingest.h).  create_impl runs the phases below in order; on
// failure the handle stays with the caller (gwi_last_error, gwi_destroy), whatever the phases allocated so far in it.

// what the phases hand to one another
struct Creation {
  const gwi_spec* spec;
  const double* const* pe_cols;
  const double* const* inj_cols;
  const gwi_ingest_program *ing_pe, *ing_inj;
  long long n_ev, n_pe, n_inj;
  gwi_plan::Knobs knobs;
  std::vector<int> narrow_term;                                       // per column: the first narrow spline term reading it (validate_spec: only such terms do)
  std::vector<const double*> tab_pe, tab_inj;                         // per column: its array in HBM
  std::vector<const double*> over_pe, over_inj, over_pe1, over_inj1;  // per term: the knot coordinates that stand in for its cols[0] / cols[1]
  bool has_spline = false;                                            // the scan keeps gradient rows in LDS
  int max_scan_blocks = 0, max_inj_groups = 0;                        // over the launch geometries in use
};

// The scan kernel of this product of terms: an ahead-of-time chain (kVariants), else a chain compiled now for exactly
// this sequence (gwi_jit.h: hipRTC, cached on disk), else -- hipRTC missing, GWI_JIT=0 -- the generic kernel
static void choose_scan_kernel(gwi_engine* h, const Creation& cr) {
  const gwi_spec* spec = cr.spec;
  const gwi_plan::Knobs& knobs = cr.knobs;
  const bool force_generic = knobs.force_generic.on(), force_jit = knobs.force_jit.on();
  h->variant = (force_generic || force_jit) ? nullptr : find_variant(*spec);
  const bool jit_allowed = !force_generic && !knobs.jit.off();
  if (!h->variant && jit_allowed) {
    int kinds[GWI_MAX_TERMS], n_spline = 0;
    for (int t = 0; t < spec->n_terms; ++t) {
      kinds[t] = spec->terms[t].kind;
      n_spline += jit::is_spline_kind(kinds[t]) ? 1 : 0;
    }
    // samples per lane: 2, or 1 from six spline terms on (the register budget of the config-5 chain) and for small catalogs
    // of spline models (gwi_plan.h, small_catalog: one round of small workgroups)
    int U = n_spline >= 6 ? 1 : 2;
    bool small = false;
    if (U == 2 && n_spline > 0 && !gwi_plan::explicit_geometry(knobs) && gwi_plan::small_catalog(cr.n_ev, cr.n_pe, cr.n_inj, h->n_cus)) U = 1, small = true;
    if (knobs.samples_per_lane.v == 1 || knobs.samples_per_lane.v == 2) U = knobs.samples_per_lane.v, small = false;
    std::string why;
    jit::Chain* jc = jit::get_chain(kinds, spec->n_terms, U, gwi_embedded_device_h, gwi_embedded_engine_h, why);
    hipModule_t mod = jc ? jit::module_on(jc, h->device, why) : nullptr;
    if (jc && !mod && jc->from_cache) {  // a cache file the runtime does not accept: drop it and compile once more
      jit::discard_chain(jc);
      jc = jit::get_chain(kinds, spec->n_terms, U, gwi_embedded_device_h, gwi_embedded_engine_h, why);
      mod = jc ? jit::module_on(jc, h->device, why) : nullptr;
    }
    bool ok = mod != nullptr;
    for (int role = 0; role < jit::kRoles && ok; ++role) {
      if (jc->lowered[role].empty()) continue;
      const hipError_t e = hipModuleGetFunction(&h->jit_fn[role], mod, jc->lowered[role].c_str());
      if (e != hipSuccess) {
        why = "jit: hipModuleGetFunction(" + jc->lowered[role] + "): " + hipGetErrorString(e);
        ok = false;
      }
    }
    if (ok) {
      Variant* v = new Variant();
      std::memset(v, 0, sizeof(*v));
      v->name = jc->name.c_str();
      v->n = jc->n;
      for (int t = 0; t < jc->n; ++t) v->kinds[t] = jc->kinds[t];
      v->samples_per_lane = jc->samples_per_lane;
      v->jit = jc;
      h->jit_variant = v;
      h->variant = v;
      h->small_geometry = small;
    } else {
      h->jit_note = why;
    }
  } else if (!h->variant) {
    h->jit_note = force_generic ? "GWI_FORCE_GENERIC" : "switched off (GWI_JIT=0)";
  }
  if (!h->variant) {
    // no compiled chain for this product of terms: the generic scan kernel evaluates it (term kinds read at run time)
    h->variant = &kGenericVariant;
    h->generic = true;
    static std::atomic<bool> warned{false};
    if (!force_generic && !warned.exchange(true) && !knobs.quiet.set) {
      std::string cmd;
      for (int t = 0; t < spec->n_terms; ++t) cmd += (t ? " " : "") + std::to_string(spec->terms[t].kind);
      std::fprintf(stderr,
                   "gwi: term-kind sequence [%s] has no ahead-of-time scan kernel and none could be compiled now (%s): using the generic one (run-time term loop, "
                   "2-2.7 x the scan time).  `python -m gwinferno_amd.precompile %s` on a machine with libhiprtc fills a cache directory this one can be pointed at (GWI_JIT_CACHE).\n",
                   cmd.c_str(), h->jit_note.c_str(), cmd.c_str());
    }
  }
  // small catalogs of spline models: the one-sample-per-lane sibling of an ahead-of-time chain (gwi_plan.h, small_catalog)
  if (!h->variant->jit && h->variant->samples_per_lane == 2 && h->variant->has(jit::kSafe) && !h->generic && !knobs.samples_per_lane.set && !gwi_plan::explicit_geometry(knobs) &&
      gwi_plan::small_catalog(cr.n_ev, cr.n_pe, cr.n_inj, h->n_cus)) {
    for (int v = 0; v < kNumVariants; ++v) {
      const Variant& s = kVariants[v];
      if (s.samples_per_lane != 1 || s.n != h->variant->n) continue;
      bool same = true;
      for (int t = 0; t < s.n; ++t) same = same && s.kinds[t] == h->variant->kinds[t];
      if (same) {
        h->variant = &s;
        h->small_geometry = true;
      }
    }
  }
}

// columns -> HBM (struct-of-arrays: one contiguous fp64 array per column and sample set)
static gwi_status upload_columns(gwi_engine* h, Creation& cr) {
  const gwi_spec* spec = cr.spec;
  gwi_status st;
  cr.narrow_term.assign(spec->n_cols, -1);
  for (int t = spec->n_terms - 1; t >= 0; --t)
    if (is_narrow_kind(spec->terms[t].kind)) cr.narrow_term[spec->terms[t].cols[0]] = t;
  cr.tab_pe.assign(spec->n_cols, nullptr);
  cr.tab_inj.assign(spec->n_cols, nullptr);
  if (cr.ing_pe) {
    // setup on the device: raw catalog columns up, one kernel per sample set writes the engine's columns (gwi_ingest.h)
    for (int c = 0; c < spec->n_cols; ++c) {
      double *dpe = nullptr, *dinj = nullptr;
      if ((st = alloc_pair(h, &dpe, &dinj)) != GWI_OK) return st;
      cr.tab_pe[c] = dpe;
      cr.tab_inj[c] = dinj;
    }
    if ((st = ingest_run(h->err, cr.ing_pe, h->n_ev * h->n_pe, spec->n_cols, h->d_cols_pe.data(), h->stream)) != GWI_OK) return st;
    if ((st = ingest_run(h->err, cr.ing_inj, h->n_inj, spec->n_cols, h->d_cols_inj.data(), h->stream)) != GWI_OK) return st;
  } else {
    for (int c = 0; c < spec->n_cols; ++c) {
      double *dpe = nullptr, *dinj = nullptr;
      if ((st = alloc_pair(h, &dpe, &dinj)) != GWI_OK) return st;
      if (cr.narrow_term[c] < 0) {
        if (h->n_ev * h->n_pe) GWI_HIP(hipMemcpy(dpe, cr.pe_cols[c], sizeof(double) * (size_t)(h->n_ev * h->n_pe), hipMemcpyHostToDevice));
        if (h->n_inj) GWI_HIP(hipMemcpy(dinj, cr.inj_cols[c], sizeof(double) * (size_t)h->n_inj, hipMemcpyHostToDevice));
      }
      cr.tab_pe[c] = dpe;
      cr.tab_inj[c] = dinj;
    }
  }
  return GWI_OK;
}

// ---- narrow columns (GWI_TERM_EXP_SPLINE_F32 / _LINEAR_SPLINE_F32): float32 in HBM, after checking that every value survives
// the round trip -- on the host for columns handed over, on the device (narrow_column_kernel) for ingested ones
static gwi_status narrow_columns(gwi_engine* h, Creation& cr) {
  const gwi_spec* spec = cr.spec;
  gwi_status st;
  for (int c = 0; c < spec->n_cols; ++c) {
    const int t = cr.narrow_term[c];
    if (t < 0) continue;
    const gwi_term& tm = spec->terms[t];
    const float park = (float)(0.5 * (tm.p[0] + tm.p[1]));  // the parking place of non-finite entries: the domain's middle
    float* d = nullptr;
    double* old = nullptr;
    if ((st = alloc_pair_f32(h, c, &d, &old)) != GWI_OK) return st;
    unsigned long long bad = 0;
    if (cr.ing_pe) {
      unsigned long long* d_bad = nullptr;
      hipError_t e = hipMalloc(&d_bad, sizeof(unsigned long long));
      if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), h->stream);
      if (e == hipSuccess) e = narrow_column_run(old, d, d_bad, h->n_ev * h->n_pe, park, h->stream);
      if (e == hipSuccess) e = narrow_column_run(old + h->inj_off, d + h->inj_off, d_bad, h->n_inj, park, h->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      (void)hipFree(d_bad);
      (void)hipFree(old);
      GWI_HIP(e);
    } else {
      (void)hipFree(old);
      std::vector<float> buf((size_t)std::max<long long>(h->n_ev * h->n_pe, h->n_inj));
      auto narrow = [&](const double* x, long long n) {
        for (long long i = 0; i < n; ++i) {
          const double v = x[i];
          float f = (float)v;
          if (!std::isfinite(v))
            f = park;
          else if ((double)f != v)
            ++bad;
          buf[(size_t)i] = f;
        }
      };
      narrow(cr.pe_cols[c], h->n_ev * h->n_pe);
      if (h->n_ev * h->n_pe) GWI_HIP(hipMemcpy(d, buf.data(), sizeof(float) * (size_t)(h->n_ev * h->n_pe), hipMemcpyHostToDevice));
      narrow(cr.inj_cols[c], h->n_inj);
      if (h->n_inj) GWI_HIP(hipMemcpy(d + h->inj_off, buf.data(), sizeof(float) * (size_t)h->n_inj, hipMemcpyHostToDevice));
    }
    if (bad)
      return fail(h, GWI_ERR_INVALID, "term " + std::to_string(t) + " (narrow spline, kind " + std::to_string(tm.kind) + "): " + std::to_string(bad) + " value" +
                                          (bad == 1 ? "" : "s") + " of column " + std::to_string(c) + " do not survive a float32 round trip");
    cr.tab_pe[c] = reinterpret_cast<const double*>(d);
    cr.tab_inj[c] = reinterpret_cast<const double*>(d + h->inj_off);
  }
  return GWI_OK;
}

// ---- spline terms read the KNOT coordinate of their column (gwi_device.h: spline_locate_knot): convert x -> u once, here.
// A column that several spline terms read with different knots, or that another kind of term (or kappa) reads too, is
// copied for each distinct use; otherwise it is converted in place.
static gwi_status knot_coordinates(gwi_engine* h, Creation& cr) {
  const gwi_spec* spec = cr.spec;
  gwi_status st;
  cr.over_pe.assign(spec->n_terms, nullptr);
  cr.over_inj.assign(spec->n_terms, nullptr);
  struct Use {
    double lo, inv_dx, top;
    const double *pe, *inj;
  };
  std::vector<std::vector<Use>> uses(spec->n_cols);
  std::vector<char> plain(spec->n_cols, 0);  // read as it is by some term or as kappa
  auto is_knot_term = [](const gwi_term& tm) { return tm.kind == GWI_TERM_EXP_SPLINE || tm.kind == GWI_TERM_LINEAR_SPLINE; };
  // the conversion a knot term asks for: its first knot, 1/dx of the uniform knots (interpolation.py:100-101) and, where the
  // exponent is clamped at the domain's end, the last coordinate below that end (else -1)
  auto use_of = [](const gwi_term& tm) {
    const int n_int = tm.n_basis - 3;
    const bool clamp = tm.kind == GWI_TERM_EXP_SPLINE && !(tm.flags & GWI_SPLINE_OUTSIDE_ZERO_EXPONENT);
    return Use{tm.p[0], (double)n_int / (tm.p[1] - tm.p[0]), clamp ? std::nextafter((double)n_int, 0.0) : -1.0, nullptr, nullptr};
  };
  auto same_use = [](const Use& a, const Use& b) { return a.lo == b.lo && a.inv_dx == b.inv_dx && a.top == b.top; };
  plain[spec->kappa_col] = 1;
  // a mass-ratio power law that takes log m1 from the m1 spline's column (GWI_RATIO_LOGM_FROM_SPLINE) reads the knot
  // coordinate too: it follows whatever conversion the spline term of the same knots asked for
  auto follows_knots = [](const gwi_term& tm, int j) { return tm.kind == GWI_TERM_POWERLAW_RATIO && (tm.flags & GWI_RATIO_LOGM_FROM_SPLINE) && j == 1; };
  for (int t = 0; t < spec->n_terms; ++t) {
    const gwi_term& tm = spec->terms[t];
    for (int j = 0; j < 2; ++j) {
      const int c = tm.cols[j];
      if (c < 0 || c >= spec->n_cols) continue;
      if (!(is_knot_term(tm) && j == 0) && !follows_knots(tm, j)) plain[c] = 1;
    }
  }
  for (int t = 0; t < spec->n_terms; ++t) {
    const gwi_term& tm = spec->terms[t];
    if (!is_knot_term(tm)) continue;
    const int c = tm.cols[0];
    Use u = use_of(tm);
    const Use* hit = nullptr;
    for (const Use& have : uses[c])
      if (same_use(have, u)) hit = &have;
    if (!hit) {
      // in place when every knot term of this column wants the same conversion and nobody reads the column as it is;
      // else every distinct use gets a copy and the column itself stays what the caller handed over
      bool all_agree = !plain[c];
      for (int t2 = 0; t2 < spec->n_terms && all_agree; ++t2) {
        const gwi_term& o = spec->terms[t2];
        if (!is_knot_term(o) || o.cols[0] != c) continue;
        all_agree = same_use(use_of(o), u);
      }
      double *dpe = h->d_cols_pe[c], *dinj = h->d_cols_inj[c];
      if (!all_agree) {  // a private copy for this use
        if ((st = alloc_pair(h, &dpe, &dinj)) != GWI_OK) return st;
      }
      GWI_HIP(spline_knot_run(cr.tab_pe[c], dpe, h->n_ev * h->n_pe, u.lo, u.inv_dx, u.top, h->stream));
      GWI_HIP(spline_knot_run(cr.tab_inj[c], dinj, h->n_inj, u.lo, u.inv_dx, u.top, h->stream));
      u.pe = dpe;
      u.inj = dinj;
      uses[c].push_back(u);
      hit = &uses[c].back();
    }
    cr.over_pe[t] = hit->pe;
    cr.over_inj[t] = hit->inj;
  }
  cr.over_pe1.assign(spec->n_terms, nullptr);
  cr.over_inj1.assign(spec->n_terms, nullptr);
  for (int t = 0; t < spec->n_terms; ++t) {
    const gwi_term& tm = spec->terms[t];
    if (!follows_knots(tm, 1)) continue;
    const int c = tm.cols[1];
    const Use* hit = nullptr;
    if (c >= 0 && c < spec->n_cols)
      for (const Use& u : uses[c])
        if (u.lo == tm.p[1] && u.inv_dx == tm.p[2]) hit = &u;
    if (!hit) return fail(h, GWI_ERR_INVALID, "GWI_RATIO_LOGM_FROM_SPLINE: cols[1] is not the coordinate column of a spline term with the knots given in p[1], p[2]");
    cr.over_pe1[t] = hit->pe;
    cr.over_inj1[t] = hit->inj;
  }
  GWI_HIP(hipStreamSynchronize(h->stream));
  return GWI_OK;
}

// normaliser grids
static gwi_status upload_norms(gwi_engine* h, const Creation& cr) {
  const gwi_spec* spec = cr.spec;
  gwi_status st;
  std::vector<NormD> nd(spec->n_norms ? spec->n_norms : 1);
  for (int j = 0; j < spec->n_norms; ++j) {
    const gwi_norm& nm = spec->norms[j];
    NormD& d = nd[j];
    std::memset(&d, 0, sizeof(d));
    d.n_pts = nm.n_pts;
    d.expo_theta = nm.expo_theta;
    d.n_basis = nm.n_basis;
    d.coef_off = nm.coef_off;
    d.flags = nm.spline_flags;
    d.expo_add = nm.expo_add;
    d.lo = nm.lo;
    d.hi = nm.hi;
    double* p;
    if ((st = upload(h, nm.tw, nm.n_pts, &p, &h->d_norm_arrays)) != GWI_OK) return st;
    d.tw = p;
    if (nm.lb) {
      if ((st = upload(h, nm.lb, nm.n_pts, &p, &h->d_norm_arrays)) != GWI_OK) return st;
      d.lb = p;
    }
    if (nm.expo_theta >= 0) {
      if ((st = upload(h, nm.l1, nm.n_pts, &p, &h->d_norm_arrays)) != GWI_OK) return st;
      d.l1 = p;
    }
    if (nm.n_basis > 0) {
      if ((st = upload(h, nm.us, nm.n_pts, &p, &h->d_norm_arrays)) != GWI_OK) return st;
      d.us = p;
    }
    // the spec's host pointers are not retained
    h->spec.norms[j].tw = h->spec.norms[j].lb = h->spec.norms[j].l1 = h->spec.norms[j].us = nullptr;
  }
  GWI_HIP(hipMalloc(&h->d_norms, sizeof(NormD) * nd.size()));
  GWI_HIP(hipMemcpy(h->d_norms, nd.data(), sizeof(NormD) * nd.size(), hipMemcpyHostToDevice));
  return GWI_OK;
}

// Dynamic LDS of the scan kernel: the workgroup's spline-gradient rows and the power-basis table behind them (gwi_plan.h,
// gacc_replicas, which also says why 16 replicas)
static void size_gradient_rows(gwi_engine* h, Creation& cr) {
  const gwi_spec* spec = cr.spec;
  for (int t = 0; t < spec->n_terms; ++t) cr.has_spline = cr.has_spline || jit::is_spline_kind(spec->terms[t].kind);
  cr.has_spline = cr.has_spline || h->generic;  // the generic chain keeps every gradient sum in the LDS rows
  if (cr.knobs.deterministic.set) h->deterministic = cr.knobs.deterministic.v != 0;
  if (!cr.has_spline) return;
  size_t static_lds = 14 * 1024;  // s_theta + s_out + s_part + s_wrec (what the kernel reports replaces this guess)
  if (h->variant->jit) {
    int v = 0;
    if (hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, h->jit_fn[jit::kScan]) == hipSuccess && v > 0) static_lds = (size_t)v;
  } else {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(h->variant->fn[jit::kScan])) == hipSuccess && fa.sharedSizeBytes > 0) static_lds = fa.sharedSizeBytes;
  }
  const gwi_plan::GaccRows rows = gwi_plan::gacc_replicas(spec->n_theta, static_lds, h->deterministic, cr.knobs);
  h->gacc_rep = rows.rep;
  h->scan_lds_bytes = rows.scan_lds;
  if (rows.scan_lds > 48 * 1024 && !h->variant->jit) {  // beyond the default dynamic-LDS limit of a HIP launch (the AQL packets carry any size; so do module launches)
    for (int role = 0; role < jit::kRoles; ++role)
      if (h->variant->fn[role]) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(h->variant->fn[role]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows.scan_lds);
  }
}

// The kernel of batched launches of a spline model.
// Batched launches of >= 9 points take the 16-points-per-wavefront kernel (gwi_mfma.h) where the model has an
// instantiation: at K = 16 it measures 15 % ahead of the 4-tap kernel on the BASELINE catalogs (config 5: 34.9 vs 41.0 us
// per evaluation, config 3: 8.7 vs 10.5) and its gradient is bit-reproducible.  GWI_BATCH_MFMA=0 keeps the 4-tap kernel,
// =2 uses the matrix-core kernel for every batch size; GWI_BATCH_ROWS=1 selects the LDS-row variant of the same kernel.
static void choose_batch_kernel(gwi_engine* h, const Creation& cr) {
  if (!cr.has_spline) return;
  const gwi_spec* spec = cr.spec;
  const gwi_plan::Knobs& knobs = cr.knobs;
  const bool named = knobs.batch_mfma.set || knobs.batch_rows.set;  // the environment names a path
  h->mfma = find_mfma_variant(*spec);
  if (h->mfma && !named) {
    // more than 8 gradient tiles: the 4-tap kernel is faster (the reference's default spline counts, 11 tiles / 165
    // hyper-parameters, on the config-3 catalog: 11.7 us per evaluation against 14.4 on the matrix cores and 14.5 with LDS rows)
    int tiles = 0;
    for (int t = 0; t < h->mfma->n; ++t) tiles += h->mfma->tiles[t];
    if (tiles > 8) h->mfma = nullptr;
  }
  if (knobs.batch_mfma.off()) h->mfma = nullptr;
  if (knobs.batch_mfma.v >= 2) h->mfma_min_batch = 1;
  if (knobs.batch_rows.v >= 1) {
    h->mfma = find_mfma_variant(*spec);
    h->batch_rows = h->mfma != nullptr;
  }
  if (knobs.batch_rows.v >= 2) h->mfma_min_batch = 1;
  // no path named by the environment: the static rule above stands (config 3 is a tie between the kernels that flipped from box
  // to box when it was measured by default, config 5 prefers the matrix cores by 15 %); GWI_BATCH_AUTOTUNE=1 measures instead
  if (knobs.batch_autotune.set) h->autotune_wanted = knobs.batch_autotune.v != 0;
  h->batch_autotune = h->autotune_wanted && h->mfma && !named && !h->deterministic;
  // a spline model without an ahead-of-time matrix-core instantiation: compiled on its first batched launch of >= 9 points and used
  // from then on (GWI_BATCH_MFMA=1: compiled now; GWI_JIT=0 or GWI_BATCH_MFMA=0: not at all; GWI_BATCH_AUTOTUNE=1: measured against
  // the 4-tap kernel there)
  const bool jit_ok = !h->generic && !h->deterministic && !find_mfma_variant(*spec) && !knobs.batch_rows.set && !knobs.jit.off();
  if (jit_ok && knobs.batch_mfma.v >= 1) {
    if (try_jit_mfma(h) && knobs.batch_mfma.v >= 2) h->mfma_min_batch = 1;
  } else if (jit_ok && !knobs.batch_mfma.set) {
    h->mfma_jit_pending = true;
  }
  if (!h->mfma) return;
  if (h->batch_rows) {
    // sample-slot replicas of the gradient rows: as many (4, 2, 1) as leave two workgroups per CU their LDS
    h->rows_rep = 4;
    while (h->rows_rep > 1 && sizeof(double) * mfma_lds_doubles(spec->n_theta, spec->n_terms, h->mfma->row_doubles, h->rows_rep) + 4608 > 80 * 1024) h->rows_rep >>= 1;
    if (knobs.rows_rep.set) h->rows_rep = std::max(1, std::min(4, knobs.rows_rep.v));
  }
  h->mfma_lds_bytes = sizeof(double) * mfma_lds_doubles(spec->n_theta, spec->n_terms, h->mfma->row_doubles, h->batch_rows ? h->rows_rep : 0);
  if (h->mfma_lds_bytes > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(h->batch_rows ? h->mfma->rows_fn : h->mfma->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->mfma_lds_bytes);
}

// The launch geometries (gwi_plan.h: plan_geometry states the rules and their knobs) and, for a parametric model, whether
// batched launches load every sample once.
// Parametric models have two batched kernels: one grid row per point (scan_kernel BATCH: the catalog streams K times through
// L2 / the Infinity Cache) and scan_pbatch_kernel (every sample loaded once for the points a workgroup draws; single-trip
// tiles: the single evaluation's where those are single trips already, else a batch geometry of one trip per workgroup).
// Which one is faster turned out to depend on the BOX: round 5's boxes ran pbatch 3-8 % ahead (42.3 against 43.7 us at config 2,
// K = 16), every box of round 6 ran it 5-14 % behind at every catalog size from 1 to 8 x config 2 (49.4 against 54.8 us; 287
// against 327 us at 8 x; blocking 242-251 k against 215-227 k evals/s: profiles/round6/EXPERIMENTS.md section 5) although it issues
// 30 % fewer instructions and moves a seventh of the bytes -- the denser fp64 kernel is the one whose time varies from box to
// box.  The choice must be static (the two sum in different orders): the row-per-point kernel is the default since round 6,
// GWI_PBATCH=1 (or a row size, GWI_PBATCH_PTS) selects the one-load-per-sample kernel.
static gwi_status plan_launch(gwi_engine* h, Creation& cr) {
  const gwi_plan::Knobs& knobs = cr.knobs;
  // resident workgroups per CU of one of this chain's kernels
  auto occupancy = [&](int role, size_t lds, int* occ) {
    return h->variant->jit ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(occ, h->jit_fn[role], kBlock, lds)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, h->variant->fn[role], kBlock, lds);
  };
  int scan_occupancy = 0;  // 0: not known (and not asked where GWI_SAMPLES_PER_BLOCK names the workgroup size)
  if (knobs.samples_per_block.v <= 0 && occupancy(jit::kScan, h->scan_lds_bytes, &scan_occupancy) != hipSuccess) scan_occupancy = 0;
  h->pbatch = false;
  if (knobs.pbatch_pts.set) h->pbatch_pts = std::max(0, knobs.pbatch_pts.v);
  h->pbatch = knobs.pbatch.set ? knobs.pbatch.v != 0 : h->pbatch_pts > 0;
  h->pbatch = h->pbatch && h->variant->has(jit::kPbatch) && !h->generic;
  h->pbatch_balanced = h->pbatch_pts == 0;  // (naming a row size asks for the rows mode)
  if (knobs.pbatch_balanced.set) h->pbatch_balanced = knobs.pbatch_balanced.v != 0;
  if (h->pbatch) {
    int occ = 0;
    const hipError_t oe = occupancy(jit::kPbatch, 0, &occ);
    if (oe != hipSuccess) (void)hipGetLastError();
    h->pbatch_wgs_per_cu = (oe == hipSuccess && occ > 0) ? std::min(occ, 8) : 4;
    if (knobs.pbatch_wgs_per_cu.set) h->pbatch_wgs_per_cu = std::max(1, std::min(16, knobs.pbatch_wgs_per_cu.v));
  }
  const long long pbatch_spb = h->pbatch ? (long long)pbatch_u(h->variant->samples_per_lane) * kBlock : 0;
  const gwi_plan::LaunchPlan plan = gwi_plan::plan_geometry(h->n_ev, h->n_pe, h->n_inj, h->n_cus, h->variant->samples_per_lane, scan_occupancy, h->small_geometry, pbatch_spb, knobs);
  h->geo[0] = plan.geo[0];
  h->geo[1] = plan.geo[1];
  h->rec_stride = kRecHeader + cr.spec->n_theta;
  if (!gwi_plan::fits_tail(h->geo[0]))
    return fail(h, GWI_ERR_INVALID, "launch geometry: more than 64 tile records per group (internal error: the tile sizes above should have prevented this)");
  cr.max_scan_blocks = std::max(h->geo[0].n_scan_blocks, h->geo[1].distinct ? h->geo[1].n_scan_blocks : 0);
  cr.max_inj_groups = std::max(h->geo[0].n_inj_groups, h->geo[1].distinct ? h->geo[1].n_inj_groups : 0);
  return GWI_OK;
}

// device and pinned host memory of the evaluations; every buffer holds either launch geometry
static gwi_status allocate_buffers(gwi_engine* h, const Creation& cr) {
  const gwi_spec* spec = cr.spec;
  const gwi_plan::Knobs& knobs = cr.knobs;
  const size_t KB = (size_t)h->max_batch;  // every per-evaluation buffer holds max_batch hyper-parameter points
  GWI_HIP(hipMalloc(&h->d_partials, sizeof(double) * KB * (size_t)(cr.max_scan_blocks ? cr.max_scan_blocks : 1) * h->rec_stride));
  GWI_HIP(hipMalloc(&h->d_ev_out, sizeof(double) * KB * 4 * (size_t)(h->n_ev ? h->n_ev : 1)));
  GWI_HIP(hipMalloc(&h->d_ev_grad, sizeof(double) * KB * (size_t)(h->n_ev ? h->n_ev : 1) * spec->n_theta));
  GWI_HIP(hipMalloc(&h->d_inj_out, sizeof(double) * KB * 4 * (size_t)cr.max_inj_groups));
  GWI_HIP(hipMalloc(&h->d_inj_grad, sizeof(double) * KB * (size_t)cr.max_inj_groups * spec->n_theta));
  GWI_HIP(hipMalloc(&h->d_tblocks, sizeof(ThetaBlock) * KB));
  GWI_HIP(hipHostMalloc((void**)&h->h_tblocks, sizeof(ThetaBlock) * KB, hipHostMallocMapped));
  GWI_HIP(hipHostGetDevicePointer((void**)&h->h_tblocks_dev, h->h_tblocks, 0));
  if (knobs.stage_kernel.set) h->stage_kernel = knobs.stage_kernel.v != 0;
  GWI_HIP(hipHostMalloc((void**)&h->h_record, sizeof(double) * KB * record_len(h), hipHostMallocMapped));
  GWI_HIP(hipHostGetDevicePointer((void**)&h->h_record_dev, h->h_record, 0));
  GWI_HIP(hipHostMalloc((void**)&h->h_ev, sizeof(double) * KB * 3 * (size_t)(h->n_ev ? h->n_ev : 1), hipHostMallocMapped));
  GWI_HIP(hipHostGetDevicePointer((void**)&h->h_ev_dev, h->h_ev, 0));
  std::memset(h->h_record, 0, sizeof(double) * KB * record_len(h));
  // the final launch: one workgroup per ~48 events (at most 8), each publishing a partial record (config 5, 200 events:
  // 1 / 4 / 8 / 16 workgroups = 7.6 / 5.8 / 5.9 / 6.7 us -- more records are more small PCIe writes)
  h->final_groups = (int)std::max<long long>(1, std::min<long long>(8, h->n_ev / 48));
  if (knobs.final_groups.set) h->final_groups = std::max(1, std::min(64, knobs.final_groups.v));
  GWI_HIP(hipHostMalloc((void**)&h->h_fin, sizeof(double) * KB * h->final_groups * record_len(h), hipHostMallocMapped));
  GWI_HIP(hipHostGetDevicePointer((void**)&h->h_fin_dev, h->h_fin, 0));
  std::memset(h->h_fin, 0, sizeof(double) * KB * h->final_groups * record_len(h));
  {  // tile references of spline models (scan_kernel, shared mode): none yet
    const size_t n = (size_t)(1 + 2 * h->max_batch) * (size_t)(cr.max_scan_blocks ? cr.max_scan_blocks : 1);  // rows: see nref_row0
    std::vector<int> none(n, kNoRef);
    GWI_HIP(hipMalloc(&h->d_tile_nref, sizeof(int) * n));
    GWI_HIP(hipMemcpy(h->d_tile_nref, none.data(), sizeof(int) * n, hipMemcpyHostToDevice));
  }
  GWI_HIP(hipMalloc(&h->d_seq, 2 * sizeof(unsigned long long)));
  GWI_HIP(hipMemset(h->d_seq, 0, 2 * sizeof(unsigned long long)));
  GWI_HIP(hipHostMalloc((void**)&h->h_redo, sizeof(unsigned long long), hipHostMallocMapped));
  GWI_HIP(hipHostGetDevicePointer((void**)&h->h_redo_dev, h->h_redo, 0));
  *h->h_redo = 0;
  // host-final mode for small problems: the per-group rows fit a few KiB, so the host sums them and
  // the third launch (final_kernel: ~1.5 us boundary + ~6-9 us of latency chain) disappears
  {
    const size_t n_groups = (size_t)h->n_ev + h->geo[0].n_inj_groups;
    const size_t row_bytes = 64 * n_groups * (size_t)((3 + spec->n_theta + 6) / 7);  // self-validating 64-byte lines: 7 values + the sequence number
    // measured per evaluation: config 3 (48 KB of rows) gains 2 us from host-final, the reference's default spline counts on 69 events
    // (165 hyper-parameters: 114 KB) 0.85 us (27.35 against 28.21 us; profiles/round6/hostfinal_def50k.txt), config 5 (195 KB) loses 5-8
    size_t host_final_limit = 120 * 1024;
    if (knobs.host_final_bytes.set) host_final_limit = (size_t)knobs.host_final_bytes.v;
    h->host_final = row_bytes <= host_final_limit;
    if (knobs.host_final.set) h->host_final = h->host_final && knobs.host_final.v != 0;
    GWI_HIP(hipHostMalloc((void**)&h->h_rows, KB * row_bytes, hipHostMallocMapped));
    GWI_HIP(hipHostGetDevicePointer((void**)&h->h_rows_dev, h->h_rows, 0));
    std::memset(h->h_rows, 0, KB * row_bytes);
    const size_t nn = KB * (size_t)(spec->n_norms ? spec->n_norms : 1);
    GWI_HIP(hipHostMalloc((void**)&h->h_norm, sizeof(double) * nn, hipHostMallocMapped));
    GWI_HIP(hipHostGetDevicePointer((void**)&h->h_norm_dev, h->h_norm, 0));
    GWI_HIP(hipHostMalloc((void**)&h->h_norm_stamp, sizeof(unsigned long long) * nn, hipHostMallocMapped));
    GWI_HIP(hipHostGetDevicePointer((void**)&h->h_norm_stamp_dev, h->h_norm_stamp, 0));
    std::memset(h->h_norm_stamp, 0, sizeof(unsigned long long) * nn);
  }
  return GWI_OK;
}

// the constant part of the kernel-argument block
static gwi_status fill_kernel_arguments(gwi_engine* h, const Creation& cr) {
  const gwi_spec* spec = cr.spec;
  const gwi_plan::Geometry &g = h->geo[0], &b = h->geo[1];
  KArgs& k = h->kargs;
  std::memset(&k, 0, sizeof(k));
  for (int t = 0; t < spec->n_terms; ++t)
    for (int j = 0; j < 2; ++j) {
      const int c = spec->terms[t].cols[j] >= 0 && spec->terms[t].cols[j] < spec->n_cols ? spec->terms[t].cols[j] : spec->terms[t].cols[0];
      k.pe_tcols[t][j] = (j == 0 && cr.over_pe[t]) ? cr.over_pe[t] : (j == 1 && cr.over_pe1[t]) ? cr.over_pe1[t] : cr.tab_pe[c];
      k.inj_tcols[t][j] = (j == 0 && cr.over_inj[t]) ? cr.over_inj[t] : (j == 1 && cr.over_inj1[t]) ? cr.over_inj1[t] : cr.tab_inj[c];
    }
  k.kappa_pe = cr.tab_pe[spec->kappa_col];
  k.kappa_inj = cr.tab_inj[spec->kappa_col];
  k.norms = h->d_norms;
  k.norm_out_host = h->h_norm_dev;
  k.norm_stamps_host = h->h_norm_stamp_dev;
  k.partials = h->d_partials;
  k.n_pe = h->n_pe;
  k.n_inj = h->n_inj;
  k.n_ev = (int)h->n_ev;
  k.tiles_per_event = g.tiles_per_event;
  k.chunk_pe = g.chunk_pe;
  k.n_inj_tiles = g.n_inj_tiles;
  k.chunk_inj = g.chunk_inj;
  k.n_norms = spec->n_norms;
  k.n_terms = spec->n_terms;
  k.n_theta = spec->n_theta;
  k.kappa_col = spec->kappa_col;
  k.rec_stride = h->rec_stride;
#ifdef GWI_STAMPS
  GWI_HIP(hipMalloc(&k.stamps, sizeof(unsigned long long) * (size_t)(g.n_scan_blocks + spec->n_norms + 1) * kWaves * 8));
  GWI_HIP(hipMemset(k.stamps, 0, sizeof(unsigned long long) * (size_t)(g.n_scan_blocks + spec->n_norms + 1) * kWaves * 8));
#endif
  k.gacc_rep = h->gacc_rep;
  k.gacc_shift = __builtin_ctz((unsigned)h->gacc_rep);
  k.seq_dev = h->d_seq;
  k.tile_nref = h->d_tile_nref;
  k.nref_stride = cr.max_scan_blocks ? cr.max_scan_blocks : 1;
  k.rows_rep = h->rows_rep;
  k.redo_host = h->h_redo_dev;
  k.redo_dev = h->d_seq + 1;
  k.two_pass = 0;
  k.deterministic = h->deterministic ? 1 : 0;
  {  // the scan's preloaded arguments (ScanHead): kappa, then the terms' columns in term order; geometry by set_geometry
    ScanHead& hd = h->sblock.head;
    std::memset(&hd, 0, sizeof(hd));
    int slot = 0;
    bool joint = true;
    auto put = [&](const double* pe, const double* inj, bool f32) {
      // (a narrow column counts its offset in float elements)
      joint = joint && (f32 ? reinterpret_cast<const void*>(reinterpret_cast<const float*>(pe) + h->inj_off) == reinterpret_cast<const void*>(inj) : inj == pe + h->inj_off);
      if (slot < kHeadCols) hd.col[slot] = pe;
      ++slot;
    };
    put(k.kappa_pe, k.kappa_inj, false);
    for (int t = 0; t < spec->n_terms; ++t)
      for (int j = 0; j < term_cols(spec->terms[t].kind) && j < 2; ++j) put(k.pe_tcols[t][j], k.inj_tcols[t][j], j == 0 && is_narrow_kind(spec->terms[t].kind));
    for (; slot < kHeadCols; ++slot) hd.col[slot] = k.kappa_pe;  // unused slots: any valid address
    if (!joint) return fail(h, GWI_ERR_INVALID, "internal error: a column's injection part does not sit inj_offset() behind its posterior-sample part");
    if (h->n_ev >= (1LL << kGeomEventBits) || h->n_pe >= (1LL << 32) || h->n_inj >= (1LL << 32) || spec->n_norms >= 16 || g.tiles_per_event >= (1 << kGeomTilesBits) ||
        !chunk_packs(g.chunk_pe) || !chunk_packs(g.chunk_inj) || (b.distinct && (!chunk_packs(b.chunk_pe) || !chunk_packs(b.chunk_inj))))
      return fail(h, GWI_ERR_INVALID, "catalog shape outside the scan's packed geometry (events < 2^20, samples per event and injections < 2^32, tiles < 8.4 M samples)");
    hd.n_pe = (unsigned)h->n_pe;
    hd.n_inj = (unsigned)h->n_inj;
  }
  for (int t = 0; t < spec->n_terms; ++t) {
    const gwi_term& tm = spec->terms[t];
    TermD& d = k.terms[t];
    d.kind = tm.kind;
    d.n_basis = tm.n_basis;
    d.th0 = tm.theta[0];
    d.th1 = tm.theta[1];
    d.th2 = tm.theta[2];
    d.th3 = tm.theta[3];
    d.flags = tm.flags;
    d.p0 = tm.p[0];
    d.p1 = tm.p[1];
    d.p2 = tm.p[2];
    d.p3 = tm.p[3];
    d.th4 = tm.kind == GWI_TERM_PLPEAK_SMOOTH ? tm.coef_off : 0;
    if (tm.kind == GWI_TERM_EXP_SPLINE_LERP) d.th1 = tm.norm;  // the grid's spline coordinates live in that normaliser's `us`
    if (jit::is_spline_kind(tm.kind)) {  // (the narrow kinds form their knot coordinate from p0 and this p2: gwi_device.h, knot_of_x)
      d.th0 = tm.coef_off;
      d.p2 = (double)(tm.n_basis - 3) / (tm.p[1] - tm.p[0]);  // 1/dx of the uniform knots (interpolation.py:100-101)
      d.p3 = (double)(tm.n_basis - 3);                          // the closed domain in knot coordinates: [0, p3]
    }
  }
  h->combine_threads = spec->n_theta + 4 <= 64 ? 64 : kBlock;
  if (cr.knobs.combine_threads.set) h->combine_threads = cr.knobs.combine_threads.v == 64 ? 64 : kBlock;
  return GWI_OK;
}

static gwi_status create_impl(const gwi_spec* spec, const double* const* pe_cols, int64_t n_ev, int64_t n_pe, const double* const* inj_cols, int64_t n_inj,
                              int32_t device, gwi_handle* out, const gwi_ingest_program* ing_pe, const gwi_ingest_program* ing_inj) {
  if (!out) return GWI_ERR_INVALID;
  *out = nullptr;
  const bool ingest = ing_pe != nullptr;
  if (!spec || n_ev < 0 || n_pe < 1 || n_inj < 0) return GWI_ERR_INVALID;
  if (ingest ? !ing_inj : (!pe_cols || !inj_cols)) return GWI_ERR_INVALID;
  int n_dev = 0;
  if (device != GWI_DEVICE_HOST_ONLY && (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1)) return GWI_ERR_NO_DEVICE;
  gwi_engine* h = new (std::nothrow) gwi_engine();
  if (!h) return GWI_ERR_INVALID;
  *out = h;  // returned even on failure so gwi_last_error() can explain; caller must gwi_destroy()
  gwi_status st = validate_spec(h, spec);
  if (st != GWI_OK) return st;
  h->spec = *spec;
  if (device == GWI_DEVICE_HOST_ONLY) {
    h->host_only = true;
    h->n_ev = n_ev;
    h->n_pe = n_pe;
    h->n_inj = n_inj;
    for (int j = 0; j < spec->n_norms; ++j) h->spec.norms[j].tw = h->spec.norms[j].lb = h->spec.norms[j].l1 = h->spec.norms[j].us = nullptr;
    std::memset(&h->kargs, 0, sizeof(h->kargs));
    return GWI_OK;
  }
  if (device < 0) {
    GWI_HIP(hipGetDevice(&h->device));
  } else {
    if (device >= n_dev) return fail(h, GWI_ERR_NO_DEVICE, "device index out of range");
    h->device = device;
  }
  GWI_HIP(hipSetDevice(h->device));
  hipDeviceProp_t prop;
  GWI_HIP(hipGetDeviceProperties(&prop, h->device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(h, GWI_ERR_NO_DEVICE, std::string("engine is built for gfx950 only; device reports ") + prop.gcnArchName);
  h->n_cus = prop.multiProcessorCount;
  Creation cr{spec, pe_cols, inj_cols, ing_pe, ing_inj, n_ev, n_pe, n_inj, gwi_plan::Knobs::from_env()};
  const gwi_plan::Knobs& knobs = cr.knobs;
  choose_scan_kernel(h, cr);
  GWI_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  if (knobs.spin_wait.set) h->spin_wait = knobs.spin_wait.v != 0;
  for (auto& e : h->ev) GWI_HIP(hipEventCreate(&e));
  if (knobs.max_batch.set) h->max_batch = knobs.max_batch.v;
  h->max_batch = std::max(1, std::min(kMaxBatchCap, h->max_batch));
  h->n_ev = n_ev;
  h->n_pe = n_pe;
  h->n_inj = n_inj;
  h->inj_off = inj_offset(n_ev, n_pe);
  if ((st = upload_columns(h, cr)) != GWI_OK) return st;
  if ((st = narrow_columns(h, cr)) != GWI_OK) return st;
  if ((st = knot_coordinates(h, cr)) != GWI_OK) return st;
  if ((st = upload_norms(h, cr)) != GWI_OK) return st;
  size_gradient_rows(h, cr);
  choose_batch_kernel(h, cr);
  if ((st = plan_launch(h, cr)) != GWI_OK) return st;
  if ((st = allocate_buffers(h, cr)) != GWI_OK) return st;
  if ((st = fill_kernel_arguments(h, cr)) != GWI_OK) return st;
  setup_aql(h, prop);
  return GWI_OK;
}

gwi_status gwi_create(const gwi_spec* spec, const double* const* pe_cols, int64_t n_ev, int64_t n_pe, const double* const* inj_cols, int64_t n_inj,
                      int32_t device, gwi_handle* out) {
  return create_impl(spec, pe_cols, n_ev, n_pe, inj_cols, n_inj, device, out, nullptr, nullptr);
}

gwi_status gwi_create_ingest(const gwi_spec* spec, const gwi_ingest_program* pe, int64_t n_ev, int64_t n_pe, const gwi_ingest_program* inj, int64_t n_inj,
                             int32_t device, gwi_handle* out) {
  if (!pe || !inj) return GWI_ERR_INVALID;
  if (device == GWI_DEVICE_HOST_ONLY) return GWI_ERR_INVALID;  // a host-only handle owns no columns: use gwi_create
  return create_impl(spec, nullptr, n_ev, n_pe, nullptr, n_inj, device, out, pe, inj);
}

gwi_status gwi_ingest_columns(const gwi_ingest_program* prog, int64_t n, int32_t n_cols, double* const* cols, int32_t device) {
  if (!prog || !cols || n < 0 || n_cols < 1 || n_cols > GWI_MAX_COLS) return GWI_ERR_INVALID;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return GWI_ERR_NO_DEVICE;
  if (device >= n_dev) return GWI_ERR_NO_DEVICE;
  if (device >= 0 && hipSetDevice(device) != hipSuccess) return GWI_ERR_HIP;
  std::string err;
  LaunchScratch sc("gwi_ingest_columns");
  std::vector<double*> d(n_cols, nullptr);
  for (int c = 0; c < n_cols; ++c)
    if (!(d[c] = sc.alloc<double>((size_t)n))) return GWI_ERR_HIP;
  gwi_status st = ingest_run(err, prog, n, n_cols, d.data(), nullptr);
  for (int c = 0; c < n_cols && st == GWI_OK; ++c)
    if (n && hipMemcpy(cols[c], d[c], sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) st = GWI_ERR_HIP;
  if (st != GWI_OK && !err.empty()) std::fprintf(stderr, "gwi_ingest_columns: %s\n", err.c_str());
  return st;
}

gwi_status gwi_read_column(gwi_handle h, int32_t pe_side, int32_t col, double* out) {
  if (!h || !out || h->host_only) return GWI_ERR_INVALID;
  const std::vector<double*>& cols = pe_side ? h->d_cols_pe : h->d_cols_inj;
  if (col < 0 || col >= (int)cols.size()) return fail(h, GWI_ERR_INVALID, "gwi_read_column: column out of range");
  const size_t n = pe_side ? (size_t)(h->n_ev * h->n_pe) : (size_t)h->n_inj;
  GWI_HIP(hipSetDevice(h->device));
  if (n && h->col_f32[col]) {  // a narrow column: float32 values, widened
    std::vector<float> buf(n);
    GWI_HIP(hipMemcpy(buf.data(), cols[col], sizeof(float) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = (double)buf[i];
  } else if (n) {
    GWI_HIP(hipMemcpy(out, cols[col], sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  return GWI_OK;
}

gwi_status gwi_resident_bytes(gwi_handle h, int64_t* pe_bytes, int64_t* inj_bytes) {
  if (!h || h->host_only) return GWI_ERR_INVALID;
  // every distinct column allocation a scan reads: kappa and each term's columns (a knot-coordinate copy is a column of its own)
  std::vector<const double*> seen;
  int64_t width = 0;  // bytes per sample
  auto add = [&](const double* p) {
    if (!p || std::find(seen.begin(), seen.end(), p) != seen.end()) return;
    seen.push_back(p);
    bool f32 = false;
    for (size_t i = 0; i < h->d_cols_pe.size(); ++i)
      if (h->d_cols_pe[i] == p) f32 = h->col_f32[i] != 0;
    width += f32 ? 4 : 8;
  };
  add(h->kargs.kappa_pe);
  for (int t = 0; t < h->spec.n_terms; ++t)
    for (int j = 0; j < term_cols(h->spec.terms[t].kind) && j < 2; ++j) add(h->kargs.pe_tcols[t][j]);
  if (pe_bytes) *pe_bytes = width * (int64_t)(h->n_ev * h->n_pe);
  if (inj_bytes) *inj_bytes = width * (int64_t)h->n_inj;
  return GWI_OK;
}

// Pin the calling thread to the CPUs next to a GPU (sysfs local_cpulist of its PCI function), within what the thread is
// allowed already.  An evaluation is a handful of PCIe round trips (arguments out through the BAR, results and stamps
// polled in pinned memory): from the far socket each costs more (config 2: 18.8 vs 17.5 us per evaluation).
static gwi_status pin_thread_to_device(int device, std::string& why) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) {
    why = "hipDeviceGetPCIBusId failed";
    return GWI_ERR_NO_DEVICE;
  }
  for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
  const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
  FILE* f = std::fopen(path.c_str(), "r");
  char line[4096] = {0};
  const bool got = f && std::fgets(line, sizeof(line), f) != nullptr;
  if (f) std::fclose(f);
  if (!got) {
    why = path + " is not readable";
    return GWI_ERR_UNSUPPORTED;
  }
  cpu_set_t allowed, want;
  CPU_ZERO(&want);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) {
    why = "sched_getaffinity failed";
    return GWI_ERR_UNSUPPORTED;
  }
  int n_set = 0;
  for (char* tok = std::strtok(line, ",\n"); tok; tok = std::strtok(nullptr, ",\n")) {  // "0-63,128-191"
    int a = 0, b = 0;
    const int fields = std::sscanf(tok, "%d-%d", &a, &b);
    if (fields < 1) continue;
    if (fields == 1) b = a;
    for (int c = a; c <= b && c < CPU_SETSIZE; ++c)
      if (CPU_ISSET(c, &allowed)) {
        CPU_SET(c, &want);
        ++n_set;
      }
  }
  if (n_set == 0 || sched_setaffinity(0, sizeof(want), &want) != 0) {
    why = "none of the GPU's local CPUs is available to this thread";
    return GWI_ERR_UNSUPPORTED;
  }
  return GWI_OK;
}

gwi_status gwi_pin_thread_to_device(int32_t device) {
  std::string why;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return GWI_ERR_NO_DEVICE;
  if (device < 0) (void)hipGetDevice(&device);
  return pin_thread_to_device(device, why);
}

gwi_status gwi_pin_thread_to_engine(gwi_handle h) {
  if (!h || h->host_only) return GWI_ERR_INVALID;
  std::string why;
  const gwi_status st = pin_thread_to_device(h->device, why);
  if (st != GWI_OK) h->err = why;
  return st;
}

gwi_status gwi_hbm_bandwidth(int32_t device, int64_t n_doubles, int32_t iters, double* read_gbs, double* triad_gbs) {
  if (n_doubles < 1024 || iters < 1 || !read_gbs || !triad_gbs) return GWI_ERR_INVALID;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return GWI_ERR_NO_DEVICE;
  if (device == GWI_DEVICE_CURRENT && hipGetDevice(&device) != hipSuccess) return GWI_ERR_HIP;
  if (device < 0 || device >= n_dev || hipSetDevice(device) != hipSuccess) return GWI_ERR_INVALID;
  const long long n2 = n_doubles / 2;
  LaunchScratch sc("gwi_hbm_bandwidth");
  double2 *a = sc.alloc<double2>((size_t)n2), *b = sc.alloc<double2>((size_t)n2), *c = sc.alloc<double2>((size_t)n2);
  double* out = sc.alloc<double>(64);
  if (!a || !b || !c || !out || !sc.open()) return GWI_ERR_HIP;
  hipStream_t st = sc.stream;
  hipEvent_t e0 = sc.e[0], e1 = sc.e[1];
  if (hipMemsetAsync(a, 0, sizeof(double2) * n2, st) != hipSuccess || hipMemsetAsync(b, 0, sizeof(double2) * n2, st) != hipSuccess ||
      hipMemsetAsync(c, 0, sizeof(double2) * n2, st) != hipSuccess || hipMemsetAsync(out, 0, 64 * sizeof(double), st) != hipSuccess)
    return GWI_ERR_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return GWI_ERR_HIP;
  const unsigned grid = (unsigned)prop.multiProcessorCount * 32u;
  float best_r = 1e30f, best_t = 1e30f;
  bool ok = true;
  for (int it = 0; it < iters + 2 && ok; ++it) {  // two untimed warm-up rounds
    float ms = 0.0f;
    ok = ok && hipEventRecord(e0, st) == hipSuccess;
    hipLaunchKernelGGL(bw_read_kernel, dim3(grid), dim3(kBlock), 0, st, (const double2*)b, n2, out, (int)grid);
    ok = ok && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (it >= 2 && ms < best_r) best_r = ms;
    ok = ok && hipEventRecord(e0, st) == hipSuccess;
    hipLaunchKernelGGL(bw_triad_kernel, dim3(grid), dim3(kBlock), 0, st, a, (const double2*)b, (const double2*)c, 3.0, n2, (int)grid);
    ok = ok && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (it >= 2 && ms < best_t) best_t = ms;
  }
  if (!ok || hipGetLastError() != hipSuccess) return GWI_ERR_HIP;
  *read_gbs = 16.0 * (double)n2 / ((double)best_r * 1e-3) / 1e9;
  *triad_gbs = 48.0 * (double)n2 / ((double)best_t * 1e-3) / 1e9;
  return GWI_OK;
}

gwi_status gwi_math_probe(int32_t device, int32_t op, int64_t n, const double* a, const double* b, double* out, int32_t* iout) {
  namespace P = gwi::probe;
  if (!a || !b || !out || !iout || n < 0 || op < GWI_PROBE_EXP || op > GWI_PROBE_BINADES_OF) return GWI_ERR_INVALID;
  if (n > ((int64_t)1 << 24)) return GWI_ERR_INVALID;  // a testing aid: 16 Mi lanes at the most
  DeviceScope scope;
  const gwi_status st = scope.select(device);
  if (st != GWI_OK) return st;
  if (n == 0) return GWI_OK;
  LaunchScratch sc("gwi_math_probe");
  if (!sc.open()) return GWI_ERR_HIP;
  const size_t na = (size_t)n * (size_t)P::a_stride(op), nb = (size_t)n * (size_t)P::b_stride(op);
  double *d_a = sc.alloc<double>(na), *d_b = sc.alloc<double>(nb), *d_out = sc.alloc<double>((size_t)n * P::kOutDoubles);
  int* d_iout = sc.alloc<int>((size_t)n);
  if (!d_a || !d_b || !d_out || !d_iout) return GWI_ERR_HIP;
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_a, a, sizeof(double) * na, hipMemcpyHostToDevice, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_b, b, sizeof(double) * nb, hipMemcpyHostToDevice, sc.stream));
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(P::math_probe_kernel, dim3(blocks), dim3(kBlock), 0, sc.stream, (int)op, (long long)n, (const double*)d_a, (const double*)d_b, d_out, d_iout);
  GWI_SCRATCH_HIP(hipGetLastError());
  GWI_SCRATCH_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)n * P::kOutDoubles, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(iout, d_iout, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipStreamSynchronize(sc.stream));
  return GWI_OK;
}

const char* gwi_dispatch_info(gwi_handle h) {
  if (!h) return "no engine";
  return h->aql_active ? (h->aq.failed() ? h->aq.why().c_str() : "aql: active") : h->aql_note.c_str();
}

gwi_status gwi_launch_geometry(gwi_handle h, int32_t out[6]) {
  if (!h || !out || h->host_only) return GWI_ERR_INVALID;
  const gwi_plan::Geometry& g = h->geo[0];
  out[0] = g.chunk_pe;
  out[1] = g.chunk_inj;
  out[2] = g.tiles_per_event;
  out[3] = g.n_inj_tiles;
  out[4] = g.n_scan_blocks;
  out[5] = g.n_inj_groups;
  return GWI_OK;
}

gwi_status gwi_tail_path(gwi_handle h, int32_t out[4]) {
  if (!h || !out || h->host_only) return GWI_ERR_INVALID;
  out[0] = (h->seq == 0 ? h->host_final : h->last_host_rows) ? 1 : 0;
  out[1] = h->last_final_groups ? h->last_final_groups : h->final_groups;
  out[2] = h->combine_threads;
  out[3] = h->last_publish_events ? 1 : 0;
  return GWI_OK;
}

gwi_status gwi_set_timing(gwi_handle h, int32_t enabled) {
  if (!h) return GWI_ERR_INVALID;
  h->timing = enabled != 0;
  h->force_hip_stream = enabled == 2;
  return GWI_OK;
}

gwi_status gwi_last_kernel_ms(gwi_handle h, float ms[3]) {
  if (!h || !ms) return GWI_ERR_INVALID;
  for (int i = 0; i < 3; ++i) ms[i] = h->last_ms[i];
  return GWI_OK;
}

int64_t gwi_partial_len(gwi_handle h) { return h ? record_len(h) : 0; }
int64_t gwi_two_pass_repeats(gwi_handle h) { return h ? h->redo_count : 0; }
const char* gwi_batch_path(gwi_handle h, int32_t k_batch) {
  if (!h || h->host_only) return "none";
  const bool safe = h->variant && h->variant->has(jit::kSafe) && h->kargs.deterministic;
  if (h->variant && h->variant->has(jit::kPbatch) && !h->generic) {  // parametric model: one load per sample where the tiles of a launch of k_batch points are single trips
    const long long gran = (long long)pbatch_u(h->variant->samples_per_lane) * kBlock;
    const gwi_plan::Geometry& g = h->geo[k_batch >= 4 && h->geo[1].distinct ? 1 : 0];
    if (h->pbatch && g.chunk_pe <= gran && g.chunk_inj <= gran && ((h->pbatch_balanced && k_batch >= kPbatchBalancedFrom) || pbatch_points(h, k_batch, g) > 1))
      return "pbatch";
    return "rows-per-point";
  }
  return (h->mfma && !safe && k_batch >= h->mfma_min_batch) ? (h->batch_rows ? "rows" : "mfma") : "taps";
}

const char* gwi_batch_kernel_note(gwi_handle h) { return h ? h->mfma_jit_note.c_str() : ""; }

gwi_status gwi_batch_calibration(gwi_handle h, int32_t* measured, double* mfma_us, double* taps_us) {
  if (!h) return GWI_ERR_INVALID;
  if (measured) *measured = h->batch_measured ? 1 : 0;
  if (mfma_us) *mfma_us = h->batch_us[0];
  if (taps_us) *taps_us = h->batch_us[1];
  return GWI_OK;
}

gwi_status gwi_jit_compile(const int32_t* kinds, int32_t n_kinds, int32_t samples_per_lane, char* path_out, int64_t path_cap, double* compile_seconds, int32_t* from_cache) {
  if (!kinds || n_kinds < 1 || n_kinds > GWI_MAX_TERMS) return GWI_ERR_INVALID;
  int ks[GWI_MAX_TERMS];
  for (int t = 0; t < n_kinds; ++t) ks[t] = kinds[t];
  std::string why;
  jit::Chain* c = jit::get_chain(ks, n_kinds, samples_per_lane, gwi_embedded_device_h, gwi_embedded_engine_h, why, samples_per_lane == 0 ? gwi_embedded_mfma_h : nullptr);
  if (!c) {
    std::fprintf(stderr, "gwi_jit_compile: %s\n", why.c_str());
    if (path_out && path_cap > 0) std::snprintf(path_out, (size_t)path_cap, "%s", why.c_str());
    return why.find("kinds") != std::string::npos ? GWI_ERR_INVALID : GWI_ERR_UNSUPPORTED;
  }
  if (path_out && path_cap > 0) std::snprintf(path_out, (size_t)path_cap, "%s", c->path.c_str());
  if (compile_seconds) *compile_seconds = c->compile_seconds;
  if (from_cache) *from_cache = c->from_cache ? 1 : 0;
  return GWI_OK;
}

gwi_status gwi_jit_info(gwi_handle h, int32_t* compiled_at_run_time, double* compile_seconds, int32_t* from_cache, const char** note) {
  if (!h) return GWI_ERR_INVALID;
  const jit::Chain* c = h->variant ? h->variant->jit : nullptr;
  if (compiled_at_run_time) *compiled_at_run_time = c ? 1 : 0;
  if (compile_seconds) *compile_seconds = c ? c->compile_seconds : 0.0;
  if (from_cache) *from_cache = (c && c->from_cache) ? 1 : 0;
  if (note) *note = h->jit_note.c_str();
  return GWI_OK;
}

gwi_status gwi_prepare_combine(gwi_handle h, const double* theta) {
  if (!h || !theta) return GWI_ERR_INVALID;
  prelude(h, theta, h->kargs.theta, h->kargs.derived, &h->host_consts[0]);
  return GWI_OK;
}

gwi_status gwi_eval_partial(gwi_handle h, const double* theta, double* record_host, double* log_bfs, double* log_neffs, double* variances) {
  if (!h || !theta || !h->variant) return GWI_ERR_INVALID;
  gwi_status st = eval_preflight(h, "gwi_eval_partial");
  if (st == GWI_OK) st = run_pipeline(h, theta);
  if (st != GWI_OK) return st;
  if (record_host) std::memcpy(record_host, h->h_record, sizeof(double) * record_len(h));
  local_sites(h, 1, nullptr, log_bfs, log_neffs, variances);
  return GWI_OK;
}

gwi_status gwi_combine(gwi_handle h, const double* records, int32_t n_ranks, const gwi_options* opt, gwi_summary* summary, double* grad, double* norms) {
  if (!h || !records || n_ranks < 1 || !opt) return GWI_ERR_INVALID;
  const gwi_status st = check_options(h, opt);
  if (st != GWI_OK) return st;
  if (opt->marginalize_selection && grad)
    return fail(h, GWI_ERR_UNSUPPORTED, "gradient with marginalize_selection=True needs the squared-weight records, which the caller-exchanged path (gwi_eval_partial / gwi_combine) does not carry: use gwi_eval or gwi_eval_sharded");
  assemble(h, records, n_ranks, opt, summary, grad, norms, h->host_consts[0]);
  return GWI_OK;
}

gwi_status gwi_eval_begin(gwi_handle h, const double* theta, const gwi_options* opt, int32_t want_grad) {
  if (!h || !theta || !opt || !h->variant) return GWI_ERR_INVALID;
  gwi_status st = check_options(h, opt);
  if (st != GWI_OK) return st;
  // (in this entry's own words; a host-only handle never holds an evaluation, so the common order of the refusals stands)
  if (h->pending) return fail(h, GWI_ERR_INVALID, "gwi_eval_begin: the previous evaluation of this handle has not been collected (gwi_eval_end)");
  st = eval_preflight(h, "gwi_eval_begin");
  if (st != GWI_OK) return st;
  h->pending_opt = *opt;
  h->pending_sq = opt->marginalize_selection && want_grad;
  if (h->pending_sq) {  // squared-weight pass first: the regular pass then leaves its per-event arrays in place
    st = run_pipeline(h, theta, nullptr, true, 1, false, /*square=*/true);
    if (st != GWI_OK) return st;
    h->sq_records.assign(h->h_record, h->h_record + record_len(h));
  }
  st = run_pipeline(h, theta, nullptr, /*wait=*/false);
  if (st != GWI_OK) return st;
  h->pending = true;
  return GWI_OK;
}

// gwi_eval_end (one point, batch = false) and gwi_eval_batch_end (the K points of the batch begun)
static GWI_HOT gwi_status eval_end_impl(gwi_handle h, int K, bool batch, gwi_summary* summaries, double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms) {
  h->pending = false;
  h->pending_batch = false;
  GWI_HIP(hipSetDevice(h->device));
  gwi_status st = collect_local(h, K);
  if (st != GWI_OK) return st;
  if (redo_requested(h)) {  // repeat, blocking (the squared-weight pass, if any, went through run_pipeline already)
    // a batch kept its points for this; a single evaluation's are in the argument block, which the repeat's prelude rewrites
    std::vector<double> th;
    if (!batch) th.assign(h->kargs.theta, h->kargs.theta + h->spec.n_theta);
    st = repeat_after_redo(h, batch ? h->pending_thetas.data() : th.data(), nullptr, K, batch, false);
    if (st != GWI_OK) return st;
  }
  finish_points(h, h->h_record, (h->pending_sq && grads) ? h->sq_records.data() : nullptr, 1, K, &h->pending_opt, summaries, grads, log_bfs, log_neffs, variances, norms);
  return GWI_OK;
}

gwi_status gwi_eval_end(gwi_handle h, gwi_summary* summary, double* grad, double* log_bfs, double* log_neffs, double* variances, double* norms) {
  if (!h) return GWI_ERR_INVALID;
  if (!h->pending || h->pending_batch) return fail(h, GWI_ERR_INVALID, "gwi_eval_end without gwi_eval_begin");
  return eval_end_impl(h, 1, false, summary, grad, log_bfs, log_neffs, variances, norms);
}

gwi_status gwi_eval(gwi_handle h, const double* theta, const gwi_options* opt, gwi_summary* summary, double* grad, double* log_bfs, double* log_neffs,
                    double* variances, double* norms) {
  const gwi_status st = gwi_eval_begin(h, theta, opt, grad != nullptr);
  if (st != GWI_OK) return st;
  return gwi_eval_end(h, summary, grad, log_bfs, log_neffs, variances, norms);
}

gwi_status gwi_eval_batch_begin(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, int32_t want_grad, int32_t want_events) {
  if (!h || !thetas || !opt || !h->variant || k_batch < 1) return GWI_ERR_INVALID;
  gwi_status st = check_batch_size(h, k_batch, "k_batch");
  if (st == GWI_OK) st = check_options(h, opt);
  if (st == GWI_OK) st = eval_preflight(h, "gwi_eval_batch_begin");
  if (st != GWI_OK) return st;
  const size_t len = (size_t)record_len(h);
  h->pending_opt = *opt;
  h->pending_sq = opt->marginalize_selection && want_grad;
  h->pending_k = k_batch;
  h->pending_thetas.assign(thetas, thetas + (size_t)k_batch * h->spec.n_theta);  // a repeat (reference exponent outrun) needs the points again
  h->batch_events = want_events != 0;
  st = ensure_batch_kernel(h, thetas, k_batch);  // (here, blocking: the launch below is not waited for)
  if (st != GWI_OK) return st;
  if (h->pending_sq) {  // squared-weight pass first, blocking: the regular pass then leaves its per-event arrays in place
    st = run_pipeline(h, thetas, nullptr, true, k_batch, true, /*square=*/true);
    if (st != GWI_OK) return st;
    h->sq_records.assign(h->h_record, h->h_record + len * k_batch);
  }
  st = run_pipeline(h, thetas, nullptr, /*wait=*/false, k_batch, true);
  if (st != GWI_OK) return st;
  h->pending = true;
  h->pending_batch = true;
  return GWI_OK;
}

gwi_status gwi_eval_batch_end(gwi_handle h, gwi_summary* summaries, double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms) {
  if (!h) return GWI_ERR_INVALID;
  if (!h->pending || !h->pending_batch || h->pending_sharded) return fail(h, GWI_ERR_INVALID, "gwi_eval_batch_end without gwi_eval_batch_begin");
  return eval_end_impl(h, h->pending_k, true, summaries, grads, log_bfs, log_neffs, variances, norms);
}

gwi_status gwi_eval_batch(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, gwi_summary* summaries, double* grads,
                          double* log_bfs, double* log_neffs, double* variances, double* norms) {
  const gwi_status st = gwi_eval_batch_begin(h, thetas, k_batch, opt, grads != nullptr, (log_bfs || log_neffs || variances) ? 1 : 0);
  if (st != GWI_OK) return st;
  return gwi_eval_batch_end(h, summaries, grads, log_bfs, log_neffs, variances, norms);
}

gwi_status gwi_comm_unique_id(const char* rccl_path, void* id128) {
  if (!id128) return GWI_ERR_INVALID;
  std::string err;
  if (!load_nccl(rccl_path, &err)) return GWI_ERR_HIP;
  return g_nccl.GetUniqueId(id128) == 0 ? GWI_OK : GWI_ERR_HIP;
}

gwi_status gwi_comm_init(gwi_handle h, const char* rccl_path, const void* id128, int32_t rank, int32_t world) {
  if (!h || !id128 || world < 1 || rank < 0 || rank >= world) return GWI_ERR_INVALID;
  if (h->host_only) return fail(h, GWI_ERR_NO_DEVICE, "host-only handle: no device to communicate from");
  if (!load_nccl(rccl_path, &h->err)) return GWI_ERR_HIP;
  GWI_HIP(hipSetDevice(h->device));
  NcclId id;
  std::memcpy(id.b, id128, 128);
  void* comm = nullptr;
  const int rc = g_nccl.CommInitRank(&comm, world, id, rank);
  if (rc != 0) return fail(h, GWI_ERR_HIP, std::string("ncclCommInitRank: ") + (g_nccl.GetErrorString ? g_nccl.GetErrorString(rc) : "error"));
  h->nccl_comm = comm;
  h->comm_rank = rank;
  h->comm_world = world;
  const size_t len = (size_t)record_len(h);
  // room for a batch of max_batch points (gwi_eval_batch_sharded): K records per rank in ONE all-gather
  const size_t KB = (size_t)h->max_batch, gather_doubles = len * world * KB;
  GWI_HIP(hipMalloc(&h->d_send, sizeof(double) * len * KB));
  GWI_HIP(hipMalloc(&h->d_recv, sizeof(double) * gather_doubles));
  GWI_HIP(hipHostMalloc((void**)&h->h_gather, sizeof(double) * (gather_doubles + 1), hipHostMallocMapped));
  GWI_HIP(hipHostGetDevicePointer((void**)&h->h_gather_dev, h->h_gather, 0));
  std::memset(h->h_gather, 0, sizeof(double) * (gather_doubles + 1));
  h->h_gather_redo = reinterpret_cast<unsigned long long*>(h->h_gather + gather_doubles);
  h->h_gather_redo_dev = reinterpret_cast<unsigned long long*>(h->h_gather_dev + gather_doubles);
  return GWI_OK;
}


// ---- single-node record exchange through POSIX shared memory ------------------------------------------------------
// Segment: [2 parities][world ranks] slots of { u64 stamp; i32 K; i32 status; double records[K][len] }, each padded to a
// multiple of 128 B.  A slot has room for kShmMaxRecords records -- the hard cap on GWI_MAX_BATCH -- whatever the rank's own
// max_batch, so every rank computes the same segment size.  Exchange s (s = 1, 2, ...): write K, the status and the records
// into slot [s & 1][rank], release-store the stamp s, then acquire-poll the stamps of all ranks.  Two parities suffice: a rank
// can only reach exchange s + 2 after every rank has published s + 1, i.e. after every rank has finished READING exchange s.
// A rank whose local half failed still publishes its stamp, with its (non-zero) status and no records; a rank that finds a
// failed status, or a K other than its own, returns -- once every rank has published the exchange -- with an error that names
// that rank.
constexpr int kShmMaxRecords = 64;
struct ShmHeader {
  unsigned long long stamp;
  int32_t k, status;
};
static_assert(sizeof(ShmHeader) == 16, "records follow the header 16-byte aligned");

static size_t shm_slot_size(size_t len) { return ((sizeof(ShmHeader) + sizeof(double) * len * kShmMaxRecords + 127) / 128) * 128; }

// publish this rank's K records (status != 0: its failure, no records), wait for every rank's, copy them to gathered[world][K][len].
// Every rank, a failing one included, waits until every rank has published the exchange (none can then still be reading its slot
// when it reaches the exchange after next); a failing rank returns GWI_OK: the failure it reports is its own.
static gwi_status shm_exchange_k(gwi_handle h, const double* records, int K, int32_t status, double* gathered) {
  const size_t len = (size_t)record_len(h);
  const unsigned long long s = ++h->shm_seq;
  char* const bank = h->shm_base + (size_t)(s & 1) * h->shm_slot_bytes * (size_t)h->shm_world;
  char* mine = bank + (size_t)h->shm_rank * h->shm_slot_bytes;
  ShmHeader* head = reinterpret_cast<ShmHeader*>(mine);
  head->k = K;
  head->status = status;
  if (status == 0) std::memcpy(mine + sizeof(ShmHeader), records, sizeof(double) * len * (size_t)K);
  __atomic_store_n(&head->stamp, s, __ATOMIC_RELEASE);
  // every rank waits for EVERY rank's stamp, whatever it finds on the way: only then can no rank still be reading this bank when
  // another reaches exchange s + 2 and rewrites it.  The first failure or mismatch found is reported after the loop.
  const auto t0 = std::chrono::steady_clock::now();
  gwi_status bad = GWI_OK;
  std::string why;
  for (int r = 0; r < h->shm_world; ++r) {
    const char* theirs = bank + (size_t)r * h->shm_slot_bytes;
    const ShmHeader* th = reinterpret_cast<const ShmHeader*>(theirs);
    for (unsigned long long spin = 1; __atomic_load_n(&th->stamp, __ATOMIC_ACQUIRE) != s; ++spin) {
      __builtin_ia32_pause();
      if ((spin & 0xfffff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 60.0)
        return fail(h, GWI_ERR_TIMEOUT, "shared-memory exchange: rank " + std::to_string(r) + " did not publish exchange " + std::to_string(s) + " within 60 s");
    }
    if (status != 0 || bad != GWI_OK) continue;
    if (th->status != 0) {
      bad = th->status;
      why = "shared-memory exchange " + std::to_string(s) + ": rank " + std::to_string(r) + " failed its local evaluation (status " + std::to_string(th->status) + ")";
    } else if (th->k != K) {
      bad = GWI_ERR_INVALID;
      why = "shared-memory exchange " + std::to_string(s) + ": rank " + std::to_string(r) + " published " + std::to_string(th->k) + " records, rank " +
            std::to_string(h->shm_rank) + " " + std::to_string(K) + " (every rank must issue the same batches)";
    } else {
      std::memcpy(gathered + (size_t)r * K * len, theirs + sizeof(ShmHeader), sizeof(double) * len * (size_t)K);
    }
  }
  return bad == GWI_OK ? GWI_OK : fail(h, bad, why);
}

gwi_status gwi_shm_comm_unlink(const char* name) {
  if (!name || !*name) return GWI_ERR_INVALID;
  return shm_unlink(name) == 0 ? GWI_OK : GWI_ERR_INVALID;
}

gwi_status gwi_shm_comm_init(gwi_handle h, const char* name, int32_t rank, int32_t world) {
  if (!h || !name || !*name || world < 1 || rank < 0 || rank >= world) return GWI_ERR_INVALID;
  if (h->shm_base) return fail(h, GWI_ERR_INVALID, "gwi_shm_comm_init: already attached");
  const size_t len = (size_t)record_len(h);
  const size_t slot = shm_slot_size(len);
  const size_t bytes = slot * 2 * (size_t)world;
  const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);
  if (fd < 0) return fail(h, GWI_ERR_INVALID, std::string("shm_open(") + name + "): " + std::strerror(errno));
  struct stat sb;
  // every rank computes the same length (the slots do not depend on max_batch) and sizes the zero-filled segment to it; whoever
  // comes later finds it sized already.  A segment of another length belongs to ranks that disagree about the model or the world
  // size: refused, not resized under a rank that may have mapped it.
  if (fstat(fd, &sb) != 0 || (sb.st_size == 0 && ftruncate(fd, (off_t)bytes) != 0)) {
    const std::string why = std::strerror(errno);
    close(fd);
    return fail(h, GWI_ERR_INVALID, std::string("sizing shared-memory segment ") + name + ": " + why);
  }
  if (fstat(fd, &sb) != 0 || (size_t)sb.st_size != bytes) {
    close(fd);
    return fail(h, GWI_ERR_INVALID, std::string("shared-memory segment ") + name + " has " + std::to_string((long long)sb.st_size) + " bytes, rank " +
                                        std::to_string(rank) + " expects " + std::to_string(bytes) + " (same model and world size on every rank?)");
  }
  void* base = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (base == MAP_FAILED) return fail(h, GWI_ERR_INVALID, std::string("mmap of shared-memory segment ") + name + ": " + std::strerror(errno));
  h->shm_base = static_cast<char*>(base);
  h->shm_bytes = bytes;
  h->shm_slot_bytes = slot;
  h->shm_rank = rank;
  h->shm_world = world;
  h->shm_seq = 0;
  h->shm_gather.assign(len * (size_t)world, 0.0);
  h->comm_rank = rank;
  h->comm_world = world;
  return GWI_OK;
}

gwi_status gwi_shm_exchange(gwi_handle h, const double* record, double* gathered) {
  if (!h || !record || !gathered) return GWI_ERR_INVALID;
  if (!h->shm_base) return fail(h, GWI_ERR_INVALID, "gwi_shm_comm_init has not been called");
  return shm_exchange_k(h, record, 1, 0, gathered);
}

gwi_status gwi_shm_exchange_batch(gwi_handle h, const double* records, int32_t k, double* gathered) {
  if (!h || k < 1 || (records && !gathered)) return GWI_ERR_INVALID;
  if (k > kShmMaxRecords) return fail(h, GWI_ERR_INVALID, "gwi_shm_exchange_batch: k exceeds 64 records");
  if (!h->shm_base) return fail(h, GWI_ERR_INVALID, "gwi_shm_comm_init has not been called");
  return shm_exchange_k(h, records, k, records ? 0 : GWI_ERR_HIP, gathered);
}

gwi_status gwi_eval_sharded(gwi_handle h, const double* theta, const gwi_options* opt, gwi_summary* summary, double* grad, double* log_bfs,
                            double* log_neffs, double* variances, double* norms) {
  if (!h || !theta || !opt || !h->variant) return GWI_ERR_INVALID;
  gwi_status st = check_exchange(h);
  if (st == GWI_OK) st = check_options(h, opt);
  if (st == GWI_OK) st = eval_preflight(h, "gwi_eval_sharded");
  if (st != GWI_OK) return st;
  const size_t len = (size_t)record_len(h);
  const double* const gathered = h->shm_base ? h->shm_gather.data() : h->h_gather;
  auto run = [&](bool square) -> gwi_status {
    if (h->shm_base) {
      // this rank's shard through the regular fast path (AQL dispatch, host-final where it applies): its record ends up
      // in host memory anyway, so the exchange is a publish + poll between host cores of the node -- no collective launch
      gwi_status st_ = run_pipeline(h, theta, nullptr, /*wait=*/true, 1, false, square);
      if (st_ != GWI_OK) return st_;
      return gwi_shm_exchange(h, h->h_record, h->shm_gather.data());
    }
    // scan -> combine -> final (record stays on the device) -> all-gather -> publish, all on one stream
    gwi_status st_ = run_pipeline(h, theta, h->d_send, /*wait=*/false, 1, false, square);
    if (st_ != GWI_OK) return st_;
    const int rc = g_nccl.AllGather(h->d_send, h->d_recv, len, kNcclDouble, h->nccl_comm, h->stream);
    if (rc != 0) return fail(h, GWI_ERR_HIP, std::string("ncclAllGather: ") + (g_nccl.GetErrorString ? g_nccl.GetErrorString(rc) : "error"));
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(kBlock), 0, h->stream, h->d_recv, h->h_gather_dev, (int)(len * h->comm_world), h->seq);
    GWI_HIP(hipGetLastError());
    return wait_for_gathered(h, 1);
  };
  // in-engine RCCL path: a rank whose scan asked for the two-pass repeat marked its record (negative event count), so
  // every rank sees the request in the gathered records and all repeat the exchange together (the ranks whose tiles were fine
  // find their references exact as well).  Over shared memory run_pipeline has repeated locally, before publishing.
  auto marked = [&] {
    bool redo = false;
    for (int r = 0; r < h->comm_world; ++r) redo = redo || h->h_gather[(size_t)r * len + 7] < 0.0;
    return redo;
  };
  auto run_checked = [&](bool square) -> gwi_status {
    const gwi_status st_ = run(square);
    if (st_ != GWI_OK || h->shm_base) return st_;
    return repeat_while_asked(h, [&] { return run(square); }, marked);
  };
  const bool need_sq = opt->marginalize_selection && grad;
  if (need_sq) {  // a second exchange carries the squared-weight numerators
    st = run_checked(true);
    if (st != GWI_OK) return st;
    h->sq_records.assign(gathered, gathered + len * h->comm_world);
  }
  st = run_checked(false);
  if (st != GWI_OK) return st;
  finish_points(h, gathered, need_sq ? h->sq_records.data() : nullptr, h->comm_world, 1, opt, summary, grad, log_bfs, log_neffs, variances, norms);
  return GWI_OK;
}

// ---- K points per exchange: the sharded counterpart of gwi_eval_batch -----------------------------------------------
// the sample-independent constants of K points (what gwi_prepare_combine computes for one)
static void host_constants(gwi_handle h, const double* thetas, int K, double* consts) {
  std::vector<double> th(h->spec.n_theta);
  std::vector<double> der((size_t)kMaxDerived * (h->spec.n_terms > 0 ? h->spec.n_terms : 1));
  for (int k = 0; k < K; ++k)
    prelude(h, thetas + (size_t)k * h->spec.n_theta, th.data(), reinterpret_cast<double (*)[kMaxDerived]>(der.data()), &consts[k]);
}

// [n_ranks][K][len] -> [K][n_ranks][len]
static void points_major(const double* in, int n_ranks, int K, size_t len, std::vector<double>& out) {
  out.resize((size_t)n_ranks * K * len);
  for (int r = 0; r < n_ranks; ++r)
    for (int k = 0; k < K; ++k) std::memcpy(out.data() + ((size_t)k * n_ranks + r) * len, in + ((size_t)r * K + k) * len, sizeof(double) * len);
}

gwi_status gwi_eval_batch_partial(gwi_handle h, const double* thetas, int32_t k, double* records, double* log_bfs, double* log_neffs, double* variances) {
  if (!h || !thetas || !h->variant || k < 1) return GWI_ERR_INVALID;
  gwi_status st = check_batch_size(h, k, "k");
  if (st == GWI_OK) st = eval_preflight(h, "gwi_eval_batch_partial");
  if (st != GWI_OK) return st;
  h->batch_events = log_bfs || log_neffs || variances;
  st = run_pipeline(h, thetas, nullptr, /*wait=*/true, k, /*batch=*/true);
  if (st != GWI_OK) return st;
  if (records) std::memcpy(records, h->h_record, sizeof(double) * record_len(h) * (size_t)k);
  local_sites(h, k, nullptr, log_bfs, log_neffs, variances);
  return GWI_OK;
}

gwi_status gwi_combine_batch(gwi_handle h, const double* thetas, int32_t k, const double* records, int32_t n_ranks, const gwi_options* opt, gwi_summary* summaries,
                             double* grads, double* norms) {
  if (!h || !thetas || !records || k < 1 || n_ranks < 1 || !opt) return GWI_ERR_INVALID;
  const gwi_status st = check_options(h, opt);
  if (st != GWI_OK) return st;
  if (opt->marginalize_selection && grads)
    return fail(h, GWI_ERR_UNSUPPORTED, "gradient with marginalize_selection=True needs the squared-weight records, which the caller-exchanged path (gwi_eval_batch_partial / gwi_combine_batch) does not carry: use gwi_eval_batch_sharded");
  std::vector<double> consts(k), by_point;
  host_constants(h, thetas, k, consts.data());
  points_major(records, n_ranks, k, (size_t)record_len(h), by_point);
  assemble_points(h, by_point.data(), nullptr, n_ranks, k, opt, consts.data(), summaries, grads, norms);
  return GWI_OK;
}

// In-engine RCCL: scan -> combine -> final ([K][len] into the device send buffer) -> ONE all-gather of K * len doubles ->
// publish_batch_kernel ([K][world][len] in pinned host memory, a stamp per point, the repeat marks folded into one word)
static gwi_status rccl_batch_issue(gwi_handle h, const double* thetas, int K, bool square) {
  const size_t len = (size_t)record_len(h);
  gwi_status st = run_pipeline(h, thetas, h->d_send, /*wait=*/false, K, /*batch=*/true, square);
  if (st != GWI_OK) return st;
  const int rc = g_nccl.AllGather(h->d_send, h->d_recv, len * (size_t)K, kNcclDouble, h->nccl_comm, h->stream);
  if (rc != 0) return fail(h, GWI_ERR_HIP, std::string("ncclAllGather: ") + (g_nccl.GetErrorString ? g_nccl.GetErrorString(rc) : "error"));
  hipLaunchKernelGGL(publish_batch_kernel, dim3((unsigned)K), dim3(kBlock), 0, h->stream, h->d_recv, h->h_gather_dev, h->h_gather_redo_dev, h->comm_world, K, (int)len, h->seq);
  GWI_HIP(hipGetLastError());
  return GWI_OK;
}
// after a collected batch: a rank whose scan asked for the two-pass repeat marked its record, every rank sees the mark in the
// gathered records and all repeat the whole batch together (the single-point path's protocol)
static gwi_status rccl_batch_repeat(gwi_handle h, const double* thetas, int K, bool square) {
  return repeat_while_asked(
      h,
      [&] {
        const gwi_status st = rccl_batch_issue(h, thetas, K, square);
        return st == GWI_OK ? wait_for_gathered(h, K) : st;
      },
      [&] { return *reinterpret_cast<volatile unsigned long long*>(h->h_gather_redo) == h->seq; });
}

// Shared memory: this rank's K records through the regular batched path (repeated locally, before publishing, when a scan asks
// for it); a local failure is published too, so that the other ranks return at once.  Leaves [K][world][len] in sq / h->shm_gather.
static gwi_status shm_batch_exchange(gwi_handle h, int K, gwi_status local, std::vector<double>& by_point) {
  if (local != GWI_OK) {
    const std::string why = h->err;
    (void)shm_exchange_k(h, nullptr, K, local, nullptr);
    h->err = why;
    return local;
  }
  const size_t len = (size_t)record_len(h);
  std::vector<double>& gathered = h->shm_gather;
  gathered.resize(len * (size_t)h->shm_world * K);
  const gwi_status st = shm_exchange_k(h, h->h_record, K, 0, gathered.data());
  if (st != GWI_OK) return st;
  points_major(gathered.data(), h->shm_world, K, len, by_point);
  return GWI_OK;
}

// Over shared memory, a rank whose half of a batch fails before it has taken part in that batch's exchange publishes the failure
// (the other ranks then return at once instead of after the exchange's time-out); `seq0` = the handle's exchange count when the
// entry point was called.  Failures of the exchange itself, and the local failures shm_batch_exchange publishes, have advanced it.
static gwi_status publish_unexchanged_failure(gwi_handle h, gwi_status st, unsigned long long seq0, int K) {
  if (st == GWI_OK || !h->shm_base || h->shm_seq != seq0) return st;
  const std::string why = h->err;
  (void)shm_exchange_k(h, nullptr, K < 1 ? 1 : (K > kShmMaxRecords ? kShmMaxRecords : K), st, nullptr);
  h->err = why;
  return st;
}

static gwi_status sharded_begin_impl(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, int32_t want_grad, int32_t want_events) {
  if (!thetas || !opt || !h->variant || k_batch < 1) return GWI_ERR_INVALID;
  gwi_status st = check_exchange(h);
  if (st == GWI_OK) st = check_batch_size(h, k_batch, "k_batch");
  if (st == GWI_OK) st = check_options(h, opt);
  if (st == GWI_OK) st = eval_preflight(h, "gwi_eval_batch_sharded_begin");
  if (st != GWI_OK) return st;
  h->pending_opt = *opt;
  h->pending_sq = opt->marginalize_selection && want_grad;
  h->pending_k = k_batch;
  h->pending_thetas.assign(thetas, thetas + (size_t)k_batch * h->spec.n_theta);
  h->batch_events = want_events != 0;
  st = ensure_batch_kernel(h, thetas, k_batch);  // the same batched kernel as gwi_eval_batch would run
  if (st != GWI_OK) return st;
  if (h->pending_sq) {  // a first exchange, blocking, carries the K squared-weight records
    if (h->shm_base) {
      st = shm_batch_exchange(h, k_batch, run_pipeline(h, thetas, nullptr, true, k_batch, true, /*square=*/true), h->sq_records);
    } else {
      st = rccl_batch_issue(h, thetas, k_batch, true);
      if (st == GWI_OK) st = wait_for_gathered(h, k_batch);
      if (st == GWI_OK) st = rccl_batch_repeat(h, thetas, k_batch, true);
      if (st == GWI_OK) h->sq_records.assign(h->h_gather, h->h_gather + (size_t)record_len(h) * h->comm_world * k_batch);
    }
    if (st != GWI_OK) return st;
  }
  if (h->shm_base) {
    st = run_pipeline(h, thetas, nullptr, /*wait=*/false, k_batch, true);
    if (st != GWI_OK) {
      std::vector<double> none;
      return shm_batch_exchange(h, k_batch, st, none);  // publishes the failure: the other ranks return at once
    }
  } else {
    st = rccl_batch_issue(h, thetas, k_batch, false);
    if (st != GWI_OK) return st;
  }
  h->pending = true;
  h->pending_batch = true;
  h->pending_sharded = true;
  return GWI_OK;
}

static gwi_status sharded_end_impl(gwi_handle h, gwi_summary* summaries, double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms) {
  h->pending = false;
  h->pending_batch = false;
  h->pending_sharded = false;
  GWI_HIP(hipSetDevice(h->device));
  const int K = h->pending_k;
  const double* thetas = h->pending_thetas.data();
  const bool need_sq = h->pending_sq && grads;
  gwi_status st;
  std::vector<double> by_point;
  const double* recs;
  int n_ranks;
  if (h->shm_base) {
    st = collect_local(h, K);
    if (st == GWI_OK) st = repeat_after_redo(h, thetas, nullptr, K, true, false);  // before publishing
    st = shm_batch_exchange(h, K, st, by_point);
    if (st != GWI_OK) return st;
    recs = by_point.data();
    n_ranks = h->shm_world;
  } else {
    st = wait_for_gathered(h, K);
    if (st == GWI_OK) st = rccl_batch_repeat(h, thetas, K, false);
    if (st != GWI_OK) return st;
    recs = h->h_gather;
    n_ranks = h->comm_world;
  }
  finish_points(h, recs, need_sq ? h->sq_records.data() : nullptr, n_ranks, K, &h->pending_opt, summaries, grads, log_bfs, log_neffs, variances, norms);
  return GWI_OK;
}

gwi_status gwi_eval_batch_sharded_begin(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, int32_t want_grad, int32_t want_events) {
  if (!h) return GWI_ERR_INVALID;
  // (a handle with a batch in flight owes that batch's exchange to gwi_eval_batch_sharded_end: the call is refused in the common
  // order, by its arguments or as busy, and nothing is published for the misuse)
  const bool in_flight = h->pending;
  const unsigned long long seq0 = h->shm_seq;
  const gwi_status st = sharded_begin_impl(h, thetas, k_batch, opt, want_grad, want_events);
  return in_flight ? st : publish_unexchanged_failure(h, st, seq0, k_batch);
}

gwi_status gwi_eval_batch_sharded_end(gwi_handle h, gwi_summary* summaries, double* grads, double* log_bfs, double* log_neffs, double* variances, double* norms) {
  if (!h) return GWI_ERR_INVALID;
  if (!h->pending || !h->pending_sharded) return fail(h, GWI_ERR_INVALID, "gwi_eval_batch_sharded_end without gwi_eval_batch_sharded_begin");
  const unsigned long long seq0 = h->shm_seq;
  return publish_unexchanged_failure(h, sharded_end_impl(h, summaries, grads, log_bfs, log_neffs, variances, norms), seq0, h->pending_k);
}

gwi_status gwi_eval_batch_sharded(gwi_handle h, const double* thetas, int32_t k_batch, const gwi_options* opt, gwi_summary* summaries, double* grads,
                                  double* log_bfs, double* log_neffs, double* variances, double* norms) {
  const gwi_status st = gwi_eval_batch_sharded_begin(h, thetas, k_batch, opt, grads != nullptr, (log_bfs || log_neffs || variances) ? 1 : 0);
  if (st != GWI_OK) return st;
  return gwi_eval_batch_sharded_end(h, summaries, grads, log_bfs, log_neffs, variances, norms);
}

gwi_status gwi_nuts_engine_queue_sharded(const gwi_handle* handles, int32_t n_groups, int32_t slots_per_group, int32_t n_chains, int32_t n_theta, const gwi_options* lopt,
                                         const gwi_param_prior* priors, const gwi_smoothing_penalty* penalties, int32_t n_penalties, const double* u0,
                                         const gwi_nuts_options* opt, double* samples, double* log_prob, int32_t* tree_depth, gwi_nuts_result* results) {
  if (!handles || n_groups < 1) return GWI_ERR_INVALID;
  for (int g = 0; g < n_groups; ++g)
    if (!handles[g] || (!handles[g]->nccl_comm && !handles[g]->shm_base)) return handles[g] ? fail(handles[g], GWI_ERR_INVALID, "gwi_nuts_engine_queue_sharded: a handle without an exchange (gwi_shm_comm_init / gwi_comm_init)") : GWI_ERR_INVALID;
  return gwi_detail::nuts_engine_queue_with(&gwi_eval_batch_sharded_begin, &gwi_eval_batch_sharded_end, handles, n_groups, slots_per_group, n_chains, n_theta, lopt, priors,
                                            penalties, n_penalties, u0, opt, samples, log_prob, tree_depth, results);
}

gwi_status gwi_selftime(gwi_handle h, const double* theta, const gwi_options* opt, int32_t n_iter, double* seconds_per_eval) {
  if (!h || !theta || !opt || n_iter < 1 || !seconds_per_eval) return GWI_ERR_INVALID;
  std::vector<double> grad(h->spec.n_theta);
  gwi_summary s;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < n_iter; ++i) {
    gwi_status st = gwi_eval(h, theta, opt, &s, grad.data(), nullptr, nullptr, nullptr, nullptr);
    if (st != GWI_OK) return st;
  }
  *seconds_per_eval = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n_iter;
  return GWI_OK;
}

// A given trajectory of hyper-parameter points, one blocking evaluation after the other (what a sampler's
// leapfrog loop does between two of its own few flops), without a host-language binding in the loop.
gwi_status gwi_eval_sequence(gwi_handle h, const double* thetas, int32_t n, const gwi_options* opt, double* log_likelihoods, double* grads, int32_t timing_every,
                             float* kernel_ms) {
  if (!h || !thetas || !opt || n < 1 || !log_likelihoods) return GWI_ERR_INVALID;
  const int nt = h->spec.n_theta;
  std::vector<double> scratch(grads ? 0 : nt);
  const bool was_timing = h->timing;
  gwi_summary s;
  for (int i = 0; i < n; ++i) {
    const bool timed = kernel_ms && timing_every > 0 && (i % timing_every == 0);
    h->timing = timed;
    double* g = grads ? grads + (size_t)i * nt : scratch.data();
    const double* th = thetas + (size_t)i * nt;
    const gwi_status st = (h->nccl_comm || h->shm_base) ? gwi_eval_sharded(h, th, opt, &s, g, nullptr, nullptr, nullptr, nullptr) : gwi_eval(h, th, opt, &s, g, nullptr, nullptr, nullptr, nullptr);
    if (st != GWI_OK) {
      h->timing = was_timing;
      return st;
    }
    log_likelihoods[i] = s.log_likelihood;
    if (kernel_ms)
      for (int k = 0; k < 3; ++k) kernel_ms[(size_t)i * 3 + k] = timed ? h->last_ms[k] : -1.0f;
  }
  h->timing = was_timing;
  return GWI_OK;
}

gwi_status gwi_eval_latencies(gwi_handle h, const double* thetas, int32_t n, const gwi_options* opt, double* seconds) {
  if (!h || !thetas || !opt || n < 1 || !seconds) return GWI_ERR_INVALID;
  const int nt = h->spec.n_theta;
  std::vector<double> g(nt);
  gwi_summary s;
  const bool sharded = h->nccl_comm || h->shm_base;
  for (int i = 0; i < n; ++i) {
    const double* th = thetas + (size_t)i * nt;
    const auto t0 = std::chrono::steady_clock::now();
    const gwi_status st = sharded ? gwi_eval_sharded(h, th, opt, &s, g.data(), nullptr, nullptr, nullptr, nullptr) : gwi_eval(h, th, opt, &s, g.data(), nullptr, nullptr, nullptr, nullptr);
    seconds[i] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st != GWI_OK) return st;
  }
  return GWI_OK;
}

#ifdef GWI_HOST_PHASES
extern "C" void gwi_debug_host_phases(double* out6) {
  for (int i = 0; i < 5; ++i) out6[i] = g_phase[i];
  out6[5] = (double)g_phase_calls;
  for (int i = 0; i < 5; ++i) g_phase[i] = 0;
  g_phase_calls = 0;
}
#endif

#ifdef GWI_STAMPS
// diagnostic build only (not part of the ABI): fetch the per-wave phase stamps of the last scan launch
gwi_status gwi_debug_stamps(gwi_handle h, unsigned long long* out, int64_t n_words) {
  if (!h || !out) return GWI_ERR_INVALID;
  const int64_t have = (int64_t)h->geo[0].n_scan_blocks * kWaves * 8;
  GWI_HIP(hipMemcpy(out, h->kargs.stamps, sizeof(unsigned long long) * (size_t)(n_words < have ? n_words : have), hipMemcpyDeviceToHost));
  return GWI_OK;
}
#endif

// The log-weight role of the engine's scan chain at theta: leaves log(p(theta|Lambda)/prior) of every sample in d_logw_pe /
// d_logw_inj, without the sample-independent constant, which is returned in *log_const.  Blocking.
static gwi_status fill_log_weights(gwi_handle h, const double* theta, double* log_const) {
  GWI_HIP(h->post.d_logw_pe.reserve((size_t)(h->n_ev * h->n_pe)));
  GWI_HIP(h->post.d_logw_inj.reserve((size_t)h->n_inj));
  // normaliser values come from a regular evaluation
  gwi_status st = run_pipeline(h, theta);
  if (st != GWI_OK) return st;
  double c = h->host_consts[0];
  const double* nrm = h->h_record + kRecNormOff;
  for (int t = 0; t < h->spec.n_terms; ++t)
    if (h->spec.terms[t].norm >= 0) c -= std::log(nrm[h->spec.terms[t].norm]);
  *log_const = c;
  h->kargs.logw_pe = h->post.d_logw_pe;
  h->kargs.logw_inj = h->post.d_logw_inj;
  set_geometry(h, false);
  st = launch_scan(h, true);
  if (st != GWI_OK) return st;
  GWI_HIP(hipStreamSynchronize(h->stream));
  return GWI_OK;
}

gwi_status gwi_log_weights(gwi_handle h, const double* theta, double* pe_logw, double* inj_logw) {
  if (!h || !theta || !h->variant) return GWI_ERR_INVALID;
  gwi_status st = eval_preflight(h, "gwi_log_weights");
  if (st != GWI_OK) return st;
  const size_t n_pe_tot = (size_t)(h->n_ev * h->n_pe), n_inj = (size_t)h->n_inj;
  double log_const = 0.0;
  st = fill_log_weights(h, theta, &log_const);
  if (st != GWI_OK) return st;
  if (pe_logw) {
    GWI_HIP(hipMemcpy(pe_logw, h->post.d_logw_pe, sizeof(double) * n_pe_tot, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_pe_tot; ++i) pe_logw[i] += log_const;
  }
  if (inj_logw) {
    GWI_HIP(hipMemcpy(inj_logw, h->post.d_logw_inj, sizeof(double) * n_inj, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_inj; ++i) inj_logw[i] += log_const;
  }
  return GWI_OK;
}

// one mask of a set: uploaded over the previous one, or dropped (all ones) for NULL
static gwi_status set_one_draw_mask(gwi_handle h, const unsigned char* src, size_t n, DeviceBuffer<unsigned char>* dst) {
  if (!src) {
    dst->reset();
    return GWI_OK;
  }
  GWI_HIP(dst->upload(src, n));
  return GWI_OK;
}

// (no scan kernel is needed and a shard may keep a mask: the refusals of post_preflight do not fit)
gwi_status gwi_set_draw_mask(gwi_handle h, const unsigned char* pe_mask, const unsigned char* inj_mask) {
  if (!h) return GWI_ERR_INVALID;
  if (h->host_only) return fail(h, GWI_ERR_INVALID, "gwi_set_draw_mask: host-only handle: no device to keep a mask on");
  gwi_status st = busy_guard(h, "gwi_set_draw_mask");
  if (st != GWI_OK) return st;
  GWI_HIP(hipSetDevice(h->device));
  st = set_one_draw_mask(h, pe_mask, (size_t)(h->n_ev * h->n_pe), &h->post.d_draw_mask_pe);
  if (st != GWI_OK) return st;
  return set_one_draw_mask(h, inj_mask, (size_t)h->n_inj, &h->post.d_draw_mask_inj);
}

// The tile workspace of gwi_draw.h's first two kernels over the whole catalog, and the one place that knows its size and layout:
// [max | sum | mass | prefix][n_tiles] (the PE tiles event-major, then the injection tiles), then the segments' maxima [n_ev + 1].
// Refuses a catalog one launch cannot index ("<who>: more <what> (or samples per segment) ..."), selects the engine's device,
// reserves the workspace and leaves *a zeroed but for the geometry, the masks and the carved pointers.
static gwi_status draw_workspace(gwi_handle h, const char* who, const char* what, gwi::draw::DrawArgs* a, long long* n_tiles_out) {
  namespace D = gwi::draw;
  const long long tiles_per_event = D::tiles_of(h->n_pe), n_inj_tiles = D::tiles_of(h->n_inj), n_tiles = h->n_ev * tiles_per_event + n_inj_tiles;
  if (n_tiles > 0x7fffffffLL || h->n_pe > 0x7fffffffLL || h->n_inj > 0x7fffffffLL)
    return fail(h, GWI_ERR_INVALID, std::string(who) + ": more " + what + " (or samples per segment) than one launch can index");
  GWI_HIP(hipSetDevice(h->device));
  GWI_HIP(h->post.d_draw_tiles.reserve((size_t)(4 * n_tiles + h->n_ev + 1)));
  std::memset(a, 0, sizeof(*a));
  a->mask_pe = h->post.d_draw_mask_pe;
  a->mask_inj = h->post.d_draw_mask_inj;
  a->tile_max = h->post.d_draw_tiles;
  a->tile_sum = a->tile_max + n_tiles;
  a->tile_mass = a->tile_sum + n_tiles;
  a->tile_prefix = a->tile_mass + n_tiles;
  a->seg_max = a->tile_prefix + n_tiles;
  a->n_pe = h->n_pe;
  a->n_inj = h->n_inj;
  a->n_ev = (int)h->n_ev;
  a->tiles_per_event = (int)tiles_per_event;
  a->n_inj_tiles = (int)n_inj_tiles;
  *n_tiles_out = n_tiles;
  return GWI_OK;
}

// ... and that of gwi_resample_injections, which runs the same two kernels over the injection set as the only segment (no events,
// its tiles from 0) and keeps more per tile: [max | sum | mass | prefix | sum w^2][n_tiles], M, the stats record; beside it the
// tiles' live counts and every injection's prefix within its tile.  n_inj is at least 1 and fits an int32 index.
static gwi_status resample_workspace(gwi_handle h, gwi::draw::DrawArgs* da, gwi::resample::Args* a) {
  namespace R = gwi::resample;
  const long long n_inj = h->n_inj, n_tiles = gwi::draw::tiles_of(n_inj);
  GWI_HIP(hipSetDevice(h->device));
  GWI_HIP(h->post.d_rs_tiles.reserve((size_t)(5 * n_tiles + 1 + R::kStats)));
  GWI_HIP(h->post.d_rs_live.reserve((size_t)n_tiles));
  GWI_HIP(h->post.d_rs_prefix.reserve((size_t)n_inj));
  std::memset(da, 0, sizeof(*da));
  da->mask_inj = h->post.d_draw_mask_inj;
  da->tile_max = h->post.d_rs_tiles;
  da->tile_sum = da->tile_max + n_tiles;
  da->tile_mass = da->tile_sum + n_tiles;
  da->tile_prefix = da->tile_mass + n_tiles;
  da->seg_max = da->tile_prefix + 2 * n_tiles;
  da->n_inj = n_inj;
  da->n_inj_tiles = (int)n_tiles;
  da->tiles_per_event = 1;  // (no event has a tile: a divisor only)
  std::memset(a, 0, sizeof(*a));
  a->mask = da->mask_inj;
  a->seg_max = da->seg_max;
  a->tile_mass = da->tile_mass;
  a->tile_prefix = da->tile_prefix;
  a->sample_prefix = h->post.d_rs_prefix;
  a->tile_sq = da->tile_prefix + n_tiles;
  a->tile_live = h->post.d_rs_live;
  a->stats = da->seg_max + 1;
  a->n = n_inj;
  a->n_tiles = (int)n_tiles;
  return GWI_OK;
}

}  // extern "C"

namespace {
// The tiles and segments of draw_workspace's layout that a query covers.  PE tiles and segments come first, the injection set's
// last: a set without columns (or bins) is left out of the query's launches.
struct QueryCover {
  int first_tile, first_seg;
  long long tiles, segs;
  QueryCover(bool with_pe, bool with_inj, long long n_ev, const gwi::draw::DrawArgs& d) {
    const long long n_pe_tiles = n_ev * d.tiles_per_event;
    first_tile = with_pe ? 0 : (int)n_pe_tiles;
    first_seg = with_pe ? 0 : (int)n_ev;
    tiles = (with_pe ? n_pe_tiles : 0) + (with_inj ? d.n_inj_tiles : 0);
    segs = (with_pe ? n_ev : 0) + (with_inj ? 1 : 0);
  }
};

// what the arguments of the queries on the marginal weights (gwi_quant.h, gwi_kde.h) share: the weights, the geometry, the cover
template <class Args>
void fill_query_args(gwi_handle h, const gwi::draw::DrawArgs& geometry, const QueryCover& cover, Args* a) {
  a->w_pe = h->post.marg.d_w;
  a->w_inj = h->post.marg.d_w + (size_t)(h->n_ev * h->n_pe);
  a->n_pe = h->n_pe;
  a->n_inj = h->n_inj;
  a->n_ev = (int)h->n_ev;
  a->tiles_per_event = geometry.tiles_per_event;
  a->n_inj_tiles = geometry.n_inj_tiles;
  a->first_tile = cover.first_tile;
  a->first_seg = cover.first_seg;
}

// The per-point pass of the post-processing entries.  One point after another, in the order of the call, since each needs its own
// normalisers and its own pass over the catalog: the log-weights at the point (blocking), the two draw launches over the whole
// catalog (*d and n_tiles as draw_workspace left them; the entry's launches see what they filled in), the entry's own launches
// stage1(p) and stage2(p), one wait for the stream, then after(p), which returns a status.  With `times` (reset by the entry) the
// host clock of the log-weights is added to ms[0], the HIP-event time of the draw launches and stage1 to ms[1], that of stage2, of
// n_stages = 2, to ms[2], and launches_per_point to the launches.  Without, no event is created.  A failure returns at once.
template <class Stage1, class Stage2, class After>
gwi_status per_point_pass(gwi_handle h, const char* who, const double* thetas, int k, gwi::draw::DrawArgs* d, long long n_tiles, StageTimes* times, int n_stages,
                                 int launches_per_point, Stage1&& stage1, Stage2&& stage2, After&& after) {
  namespace D = gwi::draw;
  LaunchScratch ev(who);
  if (times) GWI_HIP(ev.events(n_stages + 1));
  const int nt = h->spec.n_theta;
  for (int p = 0; p < k; ++p) {
    const auto t0 = std::chrono::steady_clock::now();
    gwi_status st = fill_log_weights(h, thetas + (size_t)p * nt, &d->log_const);
    if (st != GWI_OK) return st;
    if (times) times->ms[0] += 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    d->logw_pe = h->post.d_logw_pe;
    d->logw_inj = h->post.d_logw_inj;
    if (times) GWI_HIP(hipEventRecord(ev.e[0], h->stream));
    if (n_tiles) hipLaunchKernelGGL(D::draw_tile_kernel, dim3((unsigned)n_tiles), dim3(D::kDrawBlock), 0, h->stream, *d);
    hipLaunchKernelGGL(D::draw_merge_kernel, dim3((unsigned)(h->n_ev + 1)), dim3(D::kDrawBlock), 0, h->stream, *d);
    stage1(p);
    if (times && n_stages == 2) GWI_HIP(hipEventRecord(ev.e[1], h->stream));
    stage2(p);
    GWI_HIP(hipGetLastError());
    if (times) GWI_HIP(hipEventRecord(ev.e[n_stages], h->stream));
    // the next point's evaluation may go through the engine's own queue: this point's launches are over before it starts
    GWI_HIP(hipStreamSynchronize(h->stream));
    st = after(p);
    if (st != GWI_OK) return st;
    for (int s = 0; times && s < n_stages; ++s) {
      float ms = 0.f;
      GWI_HIP(hipEventElapsedTime(&ms, ev.e[s], ev.e[s + 1]));
      times->ms[1 + s] += ms;
    }
    if (times) times->launches += launches_per_point;
  }
  return GWI_OK;
}
const auto no_stage = [](int) {};
const auto no_step = [](int) { return GWI_OK; };

// The rows an entry hands back per point go through a stage on the device: kStagePoints points' rows of every array, copied to the
// caller when the stage is full or the call ends.  An entry registers (caller's array, stage, elements per point) in the order of
// the copies, points its launches of point p at slot(i, p) of array i and passes after(p) to per_point_pass.  Built per call from the
// entry's own buffers: it owns nothing.  An array the caller left out (null) or whose rows are empty is not copied.
constexpr int kStagePoints = 64;
struct StagedRows {
  struct Array {
    char *to, *stage;
    size_t bytes;  // per point
  };
  gwi_handle h;
  int k, n = 0;  // points of the call, arrays
  Array arrays[3];
  StagedRows(gwi_handle h, int k) : h(h), k(k) {}
  template <class T>
  void add(T* to, T* stage, size_t per_point) {
    arrays[n++] = Array{(char*)to, (char*)stage, sizeof(T) * per_point};
  }
  template <class T>
  T* slot(int i, int p) const {
    return (T*)(arrays[i].stage + (size_t)(p % kStagePoints) * arrays[i].bytes);
  }
  gwi_status after(int p) const {
    const int last = p % kStagePoints;
    if (last + 1 != kStagePoints && p + 1 != k) return GWI_OK;
    for (int i = 0; i < n; ++i) {
      const Array& a = arrays[i];
      if (a.to && a.bytes) GWI_HIP(hipMemcpy(a.to + (size_t)(p - last) * a.bytes, a.stage, (size_t)(last + 1) * a.bytes, hipMemcpyDeviceToHost));
    }
    return GWI_OK;
  }
};

// What the per-point entries refuse of their arguments, in their common order, or an empty string: an engine without a scan kernel,
// `unset` (what the entry works on is not set; empty when it is), no points, an output that is null.
struct NamedOutput {
  const char* name;
  const void* ptr;
};
std::string bad_point_args(gwi_handle h, const char* unset, const double* thetas, int k, std::initializer_list<NamedOutput> outputs) {
  if (!h->variant) return "the engine has no scan kernel";
  if (*unset) return unset;
  if (!thetas || k < 1) return "thetas is null or k < 1";
  for (const NamedOutput& o : outputs)
    if (!o.ptr) return std::string(o.name) + " is null";
  return "";
}
}  // namespace

extern "C" {

gwi_status gwi_draw_indices(gwi_handle h, const double* thetas, int32_t k, const double* u_pe, int32_t n_draw_pe, const double* u_inj, int32_t n_draw_inj,
                            int32_t* idx_pe, int32_t* idx_inj) {
  if (!h) return GWI_ERR_INVALID;
  gwi_status st = post_preflight(h, "gwi_draw_indices", "draw on", "injection draws need", [&]() -> std::string {
    if (!h->variant) return "the engine has no scan kernel";
    if (!thetas || k < 1) return "thetas is null or k < 1";
    if (n_draw_pe < 0 || n_draw_inj < 0) return "a negative number of draws";
    if (n_draw_pe > 0 && (!u_pe || !idx_pe)) return "n_draw_pe > 0 needs u_pe and idx_pe";
    if (n_draw_inj > 0 && (!u_inj || !idx_inj)) return "n_draw_inj > 0 needs u_inj and idx_inj";
    return "";
  });
  if (st != GWI_OK) return st;
  if (n_draw_pe == 0 && n_draw_inj == 0) return GWI_OK;
  namespace D = gwi::draw;
  const long long batches_pe = (n_draw_pe + D::kDrawBatch - 1) / D::kDrawBatch, batches_inj = (n_draw_inj + D::kDrawBatch - 1) / D::kDrawBatch;
  const long long select_blocks = h->n_ev * batches_pe + batches_inj;
  const size_t per_point = (size_t)h->n_ev * (size_t)n_draw_pe + (size_t)n_draw_inj, total = per_point * (size_t)k;
  if (select_blocks > 0x7fffffffLL || total > (size_t)1 << 40)
    return fail(h, GWI_ERR_INVALID, "gwi_draw_indices: more draws (or samples per segment) than one launch can index");
  D::DrawArgs a;
  long long n_tiles = 0;
  st = draw_workspace(h, "gwi_draw_indices", "draws", &a, &n_tiles);
  if (st != GWI_OK) return st;
  GWI_HIP(h->post.d_draw_u.reserve(total));
  GWI_HIP(h->post.d_draw_idx.reserve(total));
  double* const d_u = h->post.d_draw_u;
  int* const d_idx = h->post.d_draw_idx;
  // uniforms: [k][n_ev][n_draw_pe], then [k][n_draw_inj]; the indices likewise
  const size_t pe_all = (size_t)k * (size_t)h->n_ev * (size_t)n_draw_pe, pe_point = (size_t)h->n_ev * (size_t)n_draw_pe;
  if (pe_all) GWI_HIP(hipMemcpy(d_u, u_pe, sizeof(double) * pe_all, hipMemcpyHostToDevice));
  if (n_draw_inj) GWI_HIP(hipMemcpy(d_u + pe_all, u_inj, sizeof(double) * (size_t)k * (size_t)n_draw_inj, hipMemcpyHostToDevice));
  a.n_draw_pe = n_draw_pe;
  a.n_draw_inj = n_draw_inj;
  a.batches_pe = (int)batches_pe;
  const auto select = [&](int p) {  // (the first two launches do not look at the uniforms or the indices)
    a.u_pe = d_u + (size_t)p * pe_point;
    a.u_inj = d_u + pe_all + (size_t)p * (size_t)n_draw_inj;
    a.idx_pe = d_idx + (size_t)p * pe_point;
    a.idx_inj = d_idx + pe_all + (size_t)p * (size_t)n_draw_inj;
    hipLaunchKernelGGL(D::draw_select_kernel, dim3((unsigned)select_blocks), dim3(D::kDrawBlock), 0, h->stream, a);
  };
  st = per_point_pass(h, "gwi_draw_indices", thetas, k, &a, n_tiles, nullptr, 1, 3, select, no_stage, no_step);
  if (st != GWI_OK) return st;
  if (pe_all) GWI_HIP(hipMemcpy(idx_pe, d_idx, sizeof(int) * pe_all, hipMemcpyDeviceToHost));
  if (n_draw_inj) GWI_HIP(hipMemcpy(idx_inj, d_idx + pe_all, sizeof(int) * (size_t)k * (size_t)n_draw_inj, hipMemcpyDeviceToHost));
  return GWI_OK;
}

// ---- injection resampling (gwi_resample.h) --------------------------------------------------------------------------------
enum { kResampleLogw, kResamplePrefix, kResampleSelect };
static thread_local StageTimes g_resample_times;

constexpr long long kResampleDrawsPerLaunch = 1ll << 20;
constexpr long long kResampleBlocksPerLaunch = 2048;  // the rest of a launch's draws by grid stride

gwi_status gwi_resample_injections(gwi_handle h, const double* theta, uint64_t seed, int64_t first_index, int64_t n_request, int64_t* n_draws, double* sums, int32_t* idx,
                                   double* logw_sel) {
  if (!h) return GWI_ERR_INVALID;
  g_resample_times = StageTimes();
  gwi_status st = post_preflight(h, "gwi_resample_injections", "draw on", "injection draws need", [&]() -> std::string {
    if (!h->variant) return "the engine has no scan kernel";
    if (!theta || !n_draws || !sums) return "theta, n_draws or sums is null";
    if (n_request != 0 && (!idx || !logw_sel)) return "draws are asked for: idx and logw_sel are needed";
    if (first_index < 0) return "first_index < 0";
    return "";
  });
  if (st != GWI_OK) return st;
  namespace D = gwi::draw;
  namespace R = gwi::resample;
  const long long n_inj = h->n_inj, n_tiles = D::tiles_of(n_inj);
  if (n_inj > 0x7fffffffLL) return fail(h, GWI_ERR_INVALID, "gwi_resample_injections: more injections than an int32 index can address");
  *n_draws = 0;
  sums[0] = sums[1] = -__builtin_inf();
  sums[2] = sums[3] = 0.0;
  if (n_inj == 0) return GWI_OK;
  D::DrawArgs da;
  R::Args a;
  st = resample_workspace(h, &da, &a);
  if (st != GWI_OK) return st;
  LaunchScratch ev("gwi_resample_injections");
  GWI_HIP(ev.events(2));
  const auto t0 = std::chrono::steady_clock::now();
  st = fill_log_weights(h, theta, &da.log_const);  // (blocking)
  if (st != GWI_OK) return st;
  g_resample_times.ms[kResampleLogw] = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  da.logw_inj = a.lw = h->post.d_logw_inj;
  a.log_const = da.log_const;
  a.seed = (unsigned long long)seed;
  float ms = 0.f;
  GWI_HIP(hipEventRecord(ev.e[0], h->stream));
  hipLaunchKernelGGL(D::draw_tile_kernel, dim3((unsigned)n_tiles), dim3(D::kDrawBlock), 0, h->stream, da);
  hipLaunchKernelGGL(D::draw_merge_kernel, dim3(1), dim3(D::kDrawBlock), 0, h->stream, da);
  hipLaunchKernelGGL(R::resample_prefix_kernel, dim3((unsigned)n_tiles), dim3(R::kBlock), 0, h->stream, a);
  hipLaunchKernelGGL(R::resample_stats_kernel, dim3(1), dim3(R::kBlock), 0, h->stream, a);
  GWI_HIP(hipGetLastError());
  GWI_HIP(hipEventRecord(ev.e[1], h->stream));
  double stats[R::kStats];
  GWI_HIP(hipMemcpyAsync(stats, a.stats, sizeof(stats), hipMemcpyDeviceToHost, h->stream));
  GWI_HIP(hipStreamSynchronize(h->stream));
  GWI_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  g_resample_times.ms[kResamplePrefix] = ms;
  const double q = stats[R::kStatQ], c_last = stats[R::kStatCLast], big = stats[R::kStatMax];
  if (!(c_last > 0.0) || !(q > 0.0) || stats[R::kStatLastTile] < 0.0) return GWI_OK;  // no live sample: nothing to draw
  sums[0] = big + std::log(c_last);
  sums[1] = 2.0 * big + std::log(q);
  sums[2] = c_last * c_last / q;
  sums[3] = stats[R::kStatLive];
  const long long n = n_request < 0 ? std::min<long long>((long long)std::floor(sums[2]), n_inj) : (long long)n_request;  // (n_eff <= the live samples <= n_inj)
  const size_t chunk = (size_t)std::min<long long>(n, kResampleDrawsPerLaunch);
  GWI_HIP(h->post.d_rs_idx.reserve(chunk));
  GWI_HIP(h->post.d_rs_lw.reserve(chunk));
  a.idx = h->post.d_rs_idx;
  a.lw_sel = h->post.d_rs_lw;
  // launches of at most 2^20 draws: a draw depends on (seed, first_index + d) only, so the cut changes nothing
  for (long long d0 = 0; d0 < n; d0 += kResampleDrawsPerLaunch) {
    const long long dc = std::min<long long>(kResampleDrawsPerLaunch, n - d0);
    const long long blocks = std::min<long long>((dc + R::kBlock - 1) / R::kBlock, kResampleBlocksPerLaunch);
    a.first_index = (unsigned long long)first_index + (unsigned long long)d0;
    a.n_draws = dc;
    a.n_lanes = (int)(blocks * R::kBlock);
    GWI_HIP(hipEventRecord(ev.e[0], h->stream));
    hipLaunchKernelGGL(R::resample_select_kernel, dim3((unsigned)blocks), dim3(R::kBlock), 0, h->stream, a);
    GWI_HIP(hipGetLastError());
    GWI_HIP(hipEventRecord(ev.e[1], h->stream));
    GWI_HIP(hipMemcpyAsync(idx + d0, a.idx, sizeof(int) * (size_t)dc, hipMemcpyDeviceToHost, h->stream));
    GWI_HIP(hipMemcpyAsync(logw_sel + d0, a.lw_sel, sizeof(double) * (size_t)dc, hipMemcpyDeviceToHost, h->stream));
    GWI_HIP(hipStreamSynchronize(h->stream));  // the launch's buffers are free again
    GWI_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    g_resample_times.ms[kResampleSelect] += ms;
    ++g_resample_times.launches;
  }
  *n_draws = n;
  return GWI_OK;
}

void gwi_resample_times(double* logw_ms, double* prefix_ms, double* select_ms, int32_t* launches) { g_resample_times.report(logw_ms, prefix_ms, select_ms, launches); }

// ---- the points' weights of the weighted post-processing entries ------------------------------------------------------------------
// what is wrong with v[k][n_segs], or an empty string: every entry a number in [0, 1]
static std::string bad_point_weights(const double* v, int32_t k, long long n_segs) {
  if (!v) return "v is null";
  for (long long i = 0; i < (long long)k * n_segs; ++i)
    if (!(v[i] >= 0.0 && v[i] <= 1.0))
      return "v: point " + std::to_string(i / n_segs) + ", segment " + std::to_string(i % n_segs) + " is " + std::to_string(v[i]) + ": not in [0, 1]";
  return "";
}

// v[k][n_ev + 1] copied to the engine's device once per call
static gwi_status upload_point_weights(gwi_handle h, const double* v, int32_t k, const double** d_v) {
  const size_t n = (size_t)k * (size_t)(h->n_ev + 1);
  *d_v = nullptr;
  if (!n) return GWI_OK;
  GWI_HIP(h->post.d_point_w.upload(v, n));
  *d_v = h->post.d_point_w;
  return GWI_OK;
}

// ---- weighted histograms (gwi_hist.h) ---------------------------------------------------------------------------------------
static thread_local StageTimes g_histogram_times;

gwi_status gwi_set_histogram_bins(gwi_handle h, int32_t n_cols, int32_t n_bins, const uint16_t* pe_bins, const uint16_t* inj_bins) {
  if (!h) return GWI_ERR_INVALID;
  namespace H = gwi::hist;
  gwi_status st = post_preflight(h, "gwi_set_histogram_bins", "keep the bins on", "the injection histogram needs", [&]() -> std::string {
    if (n_cols < 1 || n_cols > H::kMaxCols) return "n_cols = " + std::to_string(n_cols) + " is not in 1 ... " + std::to_string(H::kMaxCols);
    if (n_bins < 1 || n_bins > H::kMaxBins) return "n_bins = " + std::to_string(n_bins) + " is not in 1 ... " + std::to_string(H::kMaxBins);
    if (!pe_bins && !inj_bins) return "pe_bins and inj_bins are both null";
    return "";
  });
  if (st != GWI_OK) return st;
  const size_t n_pe_codes = pe_bins ? (size_t)n_cols * (size_t)(h->n_ev * h->n_pe) : 0, n_inj_codes = inj_bins ? (size_t)n_cols * (size_t)h->n_inj : 0;
  for (int set = 0; set < 2; ++set) {
    const uint16_t* codes = set ? inj_bins : pe_bins;
    const size_t n = set ? n_inj_codes : n_pe_codes;
    for (size_t i = 0; i < n; ++i)
      if (codes[i] >= n_bins && codes[i] != H::kOutside)
        return fail(h, GWI_ERR_INVALID, std::string("gwi_set_histogram_bins: ") + (set ? "inj_bins" : "pe_bins") + " entry " + std::to_string(i) + " is " + std::to_string(codes[i]) +
                                            ": neither a bin below n_bins = " + std::to_string(n_bins) + " nor 0xFFFF (outside every bin)");
  }
  gwi::draw::DrawArgs geometry;
  long long n_tiles = 0;
  st = draw_workspace(h, "gwi_set_histogram_bins", "tiles", &geometry, &n_tiles);
  if (st != GWI_OK) return st;
  // the previous bins go away first: should an allocation fail, gwi_weighted_histograms refuses until they are set again
  PostprocessBuffers::Histogram& hist = h->post.hist;
  hist = PostprocessBuffers::Histogram();
  const size_t per_seg = (size_t)n_cols * (size_t)n_bins;
  if (n_pe_codes) GWI_HIP(hist.d_bins_pe.upload(pe_bins, n_pe_codes));  // (an empty set is one without bins)
  if (n_inj_codes) GWI_HIP(hist.d_bins_inj.upload(inj_bins, n_inj_codes));
  GWI_HIP(hist.d_partial.reserve((size_t)n_tiles * per_seg));
  GWI_HIP(hist.d_sums.reserve((size_t)(h->n_ev + 1) * per_seg));
  GWI_HIP(hist.d_dead.reserve((size_t)(h->n_ev + 1)));
  GWI_HIP(hist.d_vsum.reserve((size_t)(h->n_ev + 1)));
  hist.cols = n_cols;
  hist.bins = n_bins;
  return GWI_OK;
}

// What the arguments of the histogram and the CDF launches share (a->d is draw_workspace's): the bins, the tiles' partial histograms
// and the cover of the sets that have bins, which is returned.
static QueryCover fill_hist_args(gwi_handle h, gwi::hist::Args* a) {
  const PostprocessBuffers::Histogram& hist = h->post.hist;
  const QueryCover cover(hist.d_bins_pe.ptr != nullptr, hist.d_bins_inj.ptr != nullptr, h->n_ev, a->d);
  a->bins_pe = hist.d_bins_pe;
  a->bins_inj = hist.d_bins_inj;
  a->partial = hist.d_partial;
  a->n_cols = hist.cols;
  a->n_bins = hist.bins;
  a->first_tile = cover.first_tile;
  a->first_seg = cover.first_seg;
  return cover;
}

// gwi_weighted_histograms (weighted = false: v and vsum are not looked at) and gwi_weighted_histograms_weighted
static gwi_status weighted_histograms(gwi_handle h, const char* who, bool weighted, const double* thetas, int32_t k, const double* v, double* hist_pe, double* hist_inj,
                                      int32_t* dead, double* vsum) {
  g_histogram_times = StageTimes();
  const PostprocessBuffers::Histogram& hist = h->post.hist;
  const bool with_pe = hist.d_bins_pe.ptr != nullptr, with_inj = hist.d_bins_inj.ptr != nullptr;
  gwi_status st = post_preflight(h, who, "sum on", "the injection histogram needs", [&]() -> std::string {
    if (!h->variant) return "the engine has no scan kernel";
    if (!hist.cols) return "no bins are set (gwi_set_histogram_bins)";
    if (weighted && k < 0) return "k < 0";
    if (!thetas || k < 1) return "thetas is null or k < 1";
    if (with_pe && !hist_pe) return "pe_bins are set: hist_pe is needed";
    if (with_inj && !hist_inj) return "inj_bins are set: hist_inj is needed";
    if (!dead) return "dead is null";
    if (weighted && !vsum) return "vsum is null";
    return weighted ? bad_point_weights(v, k, h->n_ev + 1) : std::string();
  });
  if (st != GWI_OK) return st;
  namespace D = gwi::draw;
  namespace H = gwi::hist;
  H::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);  // (as gwi_set_histogram_bins found it)
  if (st != GWI_OK) return st;
  const double* d_v = nullptr;
  if (weighted) {
    st = upload_point_weights(h, v, k, &d_v);
    if (st != GWI_OK) return st;
    GWI_HIP(hipMemcpy(hist.d_vsum, vsum, sizeof(double) * (size_t)(h->n_ev + 1), hipMemcpyHostToDevice));
  }
  const size_t per_seg = (size_t)hist.cols * (size_t)hist.bins, n_pe_out = (size_t)h->n_ev * per_seg;
  // the caller's running sums: the points of this call are added onto them, so a request may be split over calls
  if (with_pe && n_pe_out) GWI_HIP(hipMemcpy(hist.d_sums, hist_pe, sizeof(double) * n_pe_out, hipMemcpyHostToDevice));
  if (with_inj) GWI_HIP(hipMemcpy(hist.d_sums + n_pe_out, hist_inj, sizeof(double) * per_seg, hipMemcpyHostToDevice));
  GWI_HIP(hipMemcpy(hist.d_dead, dead, sizeof(int) * (size_t)(h->n_ev + 1), hipMemcpyHostToDevice));
  const QueryCover cover = fill_hist_args(h, &a);
  a.hist = hist.d_sums;
  a.n_dead = hist.d_dead;
  a.vsum = hist.d_vsum;
  const auto tile = [&](int) {
    if (cover.tiles) hipLaunchKernelGGL(H::hist_tile_kernel, dim3((unsigned)cover.tiles), dim3(H::kBlock), 0, h->stream, a);
  };
  const auto merge = [&](int p) {
    if (!cover.segs) return;
    if (weighted) {
      a.v = d_v + (size_t)p * (size_t)(h->n_ev + 1);
      hipLaunchKernelGGL(H::hist_merge_kernel<true>, dim3((unsigned)cover.segs, (unsigned)a.n_cols), dim3(H::kBlock), 0, h->stream, a);
    } else {
      hipLaunchKernelGGL(H::hist_merge_kernel<false>, dim3((unsigned)cover.segs, (unsigned)a.n_cols), dim3(H::kBlock), 0, h->stream, a);
    }
  };
  st = per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_histogram_times, 2, 4, tile, merge, no_step);
  if (st != GWI_OK) return st;
  if (with_pe && n_pe_out) GWI_HIP(hipMemcpy(hist_pe, hist.d_sums, sizeof(double) * n_pe_out, hipMemcpyDeviceToHost));
  if (with_inj) GWI_HIP(hipMemcpy(hist_inj, hist.d_sums + n_pe_out, sizeof(double) * per_seg, hipMemcpyDeviceToHost));
  GWI_HIP(hipMemcpy(dead, hist.d_dead, sizeof(int) * (size_t)(h->n_ev + 1), hipMemcpyDeviceToHost));
  if (weighted) GWI_HIP(hipMemcpy(vsum, hist.d_vsum, sizeof(double) * (size_t)(h->n_ev + 1), hipMemcpyDeviceToHost));
  return GWI_OK;
}

gwi_status gwi_weighted_histograms(gwi_handle h, const double* thetas, int32_t k, double* hist_pe, double* hist_inj, int32_t* dead) {
  if (!h) return GWI_ERR_INVALID;
  return weighted_histograms(h, "gwi_weighted_histograms", false, thetas, k, nullptr, hist_pe, hist_inj, dead, nullptr);
}

gwi_status gwi_weighted_histograms_weighted(gwi_handle h, const double* thetas, int32_t k, const double* v, double* hist_pe, double* hist_inj, int32_t* dead, double* vsum) {
  if (!h) return GWI_ERR_INVALID;
  // a handle that holds a shard can have no bins (gwi_set_histogram_bins refuses it): it is told that it holds a shard, not that no bins are set
  if (!h->host_only && (h->comm_world > 1 || h->shm_world > 1))
    return fail(h, GWI_ERR_UNSUPPORTED, "gwi_weighted_histograms_weighted: this handle holds one shard of the catalog; the injection histogram needs the global set");
  return weighted_histograms(h, "gwi_weighted_histograms_weighted", true, thetas, k, v, hist_pe, hist_inj, dead, vsum);
}

void gwi_histogram_times(double* logw_ms, double* tile_ms, double* merge_ms, int32_t* launches) { g_histogram_times.report(logw_ms, tile_ms, merge_ms, launches); }

// ---- per-point CDFs and the catalog's extremes (gwi_cdf.h) ------------------------------------------------------------------
static thread_local StageTimes g_point_cdf_times;

gwi_status gwi_point_cdfs(gwi_handle h, const double* thetas, int32_t k, double* out, int32_t* live) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_cdfs";
  g_point_cdf_times = StageTimes();
  PostprocessBuffers::Histogram& hist = h->post.hist;
  const bool with_pe = hist.d_bins_pe.ptr != nullptr, with_inj = hist.d_bins_inj.ptr != nullptr;
  gwi_status st = post_preflight(h, who, "sum on", "the injection CDF needs",
                                 [&] { return bad_point_args(h, hist.cols ? "" : "no bins are set (gwi_set_histogram_bins)", thetas, k, {{"out", out}, {"live", live}}); });
  if (st != GWI_OK) return st;
  namespace D = gwi::draw;
  namespace H = gwi::hist;
  namespace F = gwi::cdf;
  F::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.h.d, &n_tiles);  // (as gwi_set_histogram_bins found it)
  if (st != GWI_OK) return st;
  // the workspace of this entry alone, allocated on its first call after the bins were set and released with them
  const size_t per_seg = (size_t)hist.cols * (size_t)hist.bins, per_point = (size_t)F::kSlots * per_seg;
  GWI_HIP(hist.d_cdf.reserve((size_t)(h->n_ev + 1) * per_seg));
  GWI_HIP(hist.d_cdf_dead.reserve((size_t)(h->n_ev + 1)));
  GWI_HIP(hist.d_cdf_stage.reserve((size_t)kStagePoints * per_point));
  GWI_HIP(hist.d_cdf_live.reserve((size_t)kStagePoints * 2));
  StagedRows rows(h, k);  // 4 n_cols n_bins doubles and two ints per point
  rows.add(out, hist.d_cdf_stage.ptr, per_point);
  rows.add(live, hist.d_cdf_live.ptr, 2);
  const QueryCover cover = fill_hist_args(h, &a.h);
  a.cdf = hist.d_cdf;
  a.seg_dead = hist.d_cdf_dead;
  a.with_pe = with_pe ? 1 : 0;
  a.with_inj = with_inj ? 1 : 0;
  const auto tile = [&](int) {
    if (cover.tiles) hipLaunchKernelGGL(H::hist_tile_kernel, dim3((unsigned)cover.tiles), dim3(H::kBlock), 0, h->stream, a.h);
  };
  const auto reduce = [&](int p) {  // into the point's slot of the stage
    a.out = rows.slot<double>(0, p);
    a.live = rows.slot<int>(1, p);
    if (cover.segs) hipLaunchKernelGGL(F::cdf_segment_kernel, dim3((unsigned)cover.segs, (unsigned)a.h.n_cols), dim3(F::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(F::cdf_catalog_kernel, dim3((unsigned)a.h.n_cols), dim3(F::kBlock), 0, h->stream, a);
  };
  return per_point_pass(h, who, thetas, k, &a.h.d, n_tiles, &g_point_cdf_times, 2, 5, tile, reduce, [&](int p) { return rows.after(p); });
}

void gwi_point_cdf_times(double* logw_ms, double* tile_ms, double* reduce_ms, int32_t* launches) { g_point_cdf_times.report(logw_ms, tile_ms, reduce_ms, launches); }

// ---- per-event calibration: per-point PIT brackets (gwi_pit.h) ---------------------------------------------------------------
static thread_local StageTimes g_point_pit_times;

gwi_status gwi_point_pits(gwi_handle h, const double* thetas, int32_t k, double* pit, double* cdf_det, int32_t* dead) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_pits";
  g_point_pit_times = StageTimes();
  PostprocessBuffers::Histogram& hist = h->post.hist;
  const bool with_pe = hist.d_bins_pe.ptr != nullptr, with_inj = hist.d_bins_inj.ptr != nullptr;
  const char* unset = !hist.cols  ? "no bins are set (gwi_set_histogram_bins)"
                      : !with_pe  ? "no PE bins are set: an event's PIT needs the bins of both sets (gwi_set_histogram_bins)"
                      : !with_inj ? "no injection bins are set: an event's PIT needs the bins of both sets (gwi_set_histogram_bins)"
                                  : "";
  gwi_status st = post_preflight(h, who, "sum on", "the injection CDF needs", [&] { return bad_point_args(h, unset, thetas, k, {{"pit", pit}, {"dead", dead}}); });
  if (st != GWI_OK) return st;
  namespace H = gwi::hist;
  namespace F = gwi::cdf;
  namespace P = gwi::pit;
  P::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.f.h.d, &n_tiles);  // (as gwi_set_histogram_bins found it)
  if (st != GWI_OK) return st;
  const size_t n_segs = (size_t)(h->n_ev + 1), per_seg = (size_t)hist.cols * (size_t)hist.bins, per_point = (size_t)h->n_ev * (size_t)hist.cols * 2;
  GWI_HIP(hist.d_cdf.reserve(n_segs * per_seg));
  GWI_HIP(hist.d_cdf_dead.reserve(n_segs));
  GWI_HIP(hist.d_pit_stage.reserve((size_t)kStagePoints * per_point));
  GWI_HIP(hist.d_pit_det.reserve((size_t)kStagePoints * per_seg));
  GWI_HIP(hist.d_pit_dead.reserve((size_t)kStagePoints * n_segs));
  StagedRows rows(h, k);  // 2 n_ev n_cols (+ n_cols n_bins where the caller takes cdf_det) doubles and n_ev + 1 ints per point
  rows.add(pit, hist.d_pit_stage.ptr, per_point);
  rows.add(cdf_det, hist.d_pit_det.ptr, per_seg);
  rows.add(dead, hist.d_pit_dead.ptr, n_segs);
  const QueryCover cover = fill_hist_args(h, &a.f.h);  // (both sets have bins: every tile and every segment)
  a.f.cdf = hist.d_cdf;
  a.f.seg_dead = hist.d_cdf_dead;
  a.f.with_pe = a.f.with_inj = 1;
  const auto tile = [&](int) {
    if (cover.tiles) hipLaunchKernelGGL(H::hist_tile_kernel, dim3((unsigned)cover.tiles), dim3(H::kBlock), 0, h->stream, a.f.h);
  };
  const auto walk = [&](int p) {  // into the point's slot of the stage
    a.pit = rows.slot<double>(0, p);
    a.cdf_det = rows.slot<double>(1, p);
    a.dead = rows.slot<int>(2, p);
    hipLaunchKernelGGL(F::cdf_segment_kernel, dim3((unsigned)cover.segs, (unsigned)a.f.h.n_cols), dim3(F::kBlock), 0, h->stream, a.f);
    hipLaunchKernelGGL(P::pit_kernel, dim3((unsigned)cover.segs, (unsigned)a.f.h.n_cols), dim3(P::kBlock), 0, h->stream, a);
  };
  return per_point_pass(h, who, thetas, k, &a.f.h.d, n_tiles, &g_point_pit_times, 2, 5, tile, walk, [&](int p) { return rows.after(p); });
}

void gwi_point_pit_times(double* logw_ms, double* tile_ms, double* pit_ms, int32_t* launches) { g_point_pit_times.report(logw_ms, tile_ms, pit_ms, launches); }

// ---- exact per-event calibration: weighted ranks among the injections (gwi_rank.h) ---------------------------------------------------
static thread_local StageTimes g_point_rank_times;

// what is wrong with the rank columns, or an empty string: every order a permutation of the injections, every rank in [0, n_inj],
// rank_lt <= rank_le
static std::string bad_rank_columns(int n_cols, long long n_pe_all, long long n_inj, const int32_t* order_inj, const int32_t* rank_lt, const int32_t* rank_le) {
  std::vector<unsigned char> seen((size_t)n_inj);
  for (int c = 0; c < n_cols; ++c) {
    std::fill(seen.begin(), seen.end(), 0);
    const int32_t* order = order_inj + (size_t)c * (size_t)n_inj;
    for (long long r = 0; r < n_inj; ++r) {
      const long long j = order[r];
      if (j < 0 || j >= n_inj || seen[(size_t)j])
        return "order_inj column " + std::to_string(c) + ": rank " + std::to_string(r) + " holds " + std::to_string(j) + ": not a permutation of the " + std::to_string(n_inj) + " injections";
      seen[(size_t)j] = 1;
    }
    const int32_t* lt = rank_lt + (size_t)c * (size_t)n_pe_all;
    const int32_t* le = rank_le + (size_t)c * (size_t)n_pe_all;
    for (long long i = 0; i < n_pe_all; ++i) {
      const std::string where = " column " + std::to_string(c) + ", sample " + std::to_string(i) + ": ";
      if (lt[i] < 0 || lt[i] > n_inj) return "rank_lt_pe" + where + std::to_string(lt[i]) + " is not in 0 ... n_inj = " + std::to_string(n_inj);
      if (le[i] < 0 || le[i] > n_inj) return "rank_le_pe" + where + std::to_string(le[i]) + " is not in 0 ... n_inj = " + std::to_string(n_inj);
      if (lt[i] > le[i]) return "rank_lt_pe" + where + std::to_string(lt[i]) + " exceeds rank_le_pe = " + std::to_string(le[i]);
    }
  }
  return "";
}

gwi_status gwi_set_rank_columns(gwi_handle h, int32_t n_cols, const int32_t* order_inj, const int32_t* rank_lt_pe, const int32_t* rank_le_pe) {
  if (!h) return GWI_ERR_INVALID;
  namespace R = gwi::rank;
  const char* who = "gwi_set_rank_columns";
  gwi_status st = post_preflight(h, who, "keep the columns on", "the injection ranks need", [&]() -> std::string {
    if (n_cols < 1 || n_cols > R::kMaxCols) return "n_cols = " + std::to_string(n_cols) + " is not in 1 ... " + std::to_string(R::kMaxCols);
    if (!order_inj || !rank_lt_pe || !rank_le_pe) return "order_inj, rank_lt_pe or rank_le_pe is null";
    if (h->n_pe > 0x7fffffffLL || h->n_inj >= 0x7fffffffLL) return "more samples per segment than an int32 rank can count";
    return bad_rank_columns(n_cols, h->n_ev * h->n_pe, h->n_inj, order_inj, rank_lt_pe, rank_le_pe);
  });
  if (st != GWI_OK) return st;
  gwi::draw::DrawArgs geometry;
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &geometry, &n_tiles);
  if (st != GWI_OK) return st;
  // the previous columns go away first: should an allocation fail, gwi_point_pits_exact refuses until they are set again
  RankBuffers& rank = h->rank;
  rank = RankBuffers();
  const size_t n_pe_all = (size_t)(h->n_ev * h->n_pe), n_inj = (size_t)h->n_inj, cols = (size_t)n_cols;
  const size_t n_prefix = cols * (n_inj + 1);
  GWI_HIP(rank.d_order_inj.upload(order_inj, cols * n_inj));
  GWI_HIP(rank.d_rank_lt.upload(rank_lt_pe, cols * n_pe_all));
  GWI_HIP(rank.d_rank_le.upload(rank_le_pe, cols * n_pe_all));
  GWI_HIP(rank.d_tiles.reserve(2 * cols * (size_t)geometry.n_inj_tiles));
  GWI_HIP(rank.d_prefix.reserve(n_prefix));
  GWI_HIP(rank.d_partial.reserve((size_t)(h->n_ev * geometry.tiles_per_event) * cols * 2));
  GWI_HIP(rank.d_stage.reserve((size_t)kStagePoints * (size_t)h->n_ev * cols * 2));
  GWI_HIP(rank.d_dead.reserve((size_t)kStagePoints * (size_t)(h->n_ev + 1)));
  GWI_HIP(hipMemset(rank.d_prefix, 0, sizeof(double) * n_prefix));  // (an empty injection set launches nothing that would store P[c][0])
  rank.cols = n_cols;
  return GWI_OK;
}

gwi_status gwi_point_pits_exact(gwi_handle h, const double* thetas, int32_t k, double* pit, int32_t* dead) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_pits_exact";
  g_point_rank_times = StageTimes();
  RankBuffers& rank = h->rank;
  gwi_status st = post_preflight(h, who, "sum on", "the injection ranks need",
                                 [&] { return bad_point_args(h, rank.cols ? "" : "no rank columns are set (gwi_set_rank_columns)", thetas, k, {{"pit", pit}, {"dead", dead}}); });
  if (st != GWI_OK) return st;
  namespace R = gwi::rank;
  R::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);  // (as gwi_set_rank_columns found it)
  if (st != GWI_OK) return st;
  const size_t n_segs = (size_t)(h->n_ev + 1), per_point = (size_t)h->n_ev * (size_t)rank.cols * 2;
  const unsigned cols = (unsigned)rank.cols, inj_tiles = (unsigned)a.d.n_inj_tiles, pe_tiles = (unsigned)(h->n_ev * a.d.tiles_per_event);
  a.order_inj = rank.d_order_inj;
  a.rank_lt = rank.d_rank_lt;
  a.rank_le = rank.d_rank_le;
  a.tile_sum = rank.d_tiles;
  a.tile_off = rank.d_tiles + (size_t)rank.cols * (size_t)a.d.n_inj_tiles;
  a.prefix = rank.d_prefix;
  a.partial = rank.d_partial;
  a.n_cols = rank.cols;
  StagedRows rows(h, k);  // 2 n_ev n_cols doubles and n_ev + 1 ints per point
  rows.add(pit, rank.d_stage.ptr, per_point);
  rows.add(dead, rank.d_dead.ptr, n_segs);
  const auto prefix = [&](int) {
    if (!inj_tiles) return;
    hipLaunchKernelGGL(R::rank_tile_kernel, dim3(inj_tiles, cols), dim3(R::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(R::rank_merge_kernel, dim3(cols), dim3(R::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(R::rank_prefix_kernel, dim3(inj_tiles, cols), dim3(R::kBlock), 0, h->stream, a);
  };
  const auto sum = [&](int p) {  // into the point's slot of the stage
    a.pit = rows.slot<double>(0, p);
    a.dead = rows.slot<int>(1, p);
    if (pe_tiles) hipLaunchKernelGGL(R::pit_rank_kernel, dim3(pe_tiles, cols), dim3(R::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(R::pit_rank_merge_kernel, dim3((unsigned)n_segs, cols), dim3(R::kBlock), 0, h->stream, a);
  };
  return per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_point_rank_times, 2, 7, prefix, sum, [&](int p) { return rows.after(p); });
}

void gwi_point_rank_times(double* logw_ms, double* prefix_ms, double* pit_ms, int32_t* launches) { g_point_rank_times.report(logw_ms, prefix_ms, pit_ms, launches); }

// ---- per-point moments: means and full covariance of the KDE columns (gwi_moment.h) -------------------------------------------------
static thread_local StageTimes g_point_moment_times;

gwi_status gwi_point_moments(gwi_handle h, const double* thetas, int32_t k, double* out, int32_t* dead) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_moments";
  g_point_moment_times = StageTimes();
  PostprocessBuffers::Kde& kde = h->post.kde;
  gwi_status st = post_preflight(h, who, "sum on", "the injection moments need", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_weighted_kde: a shard cannot be given columns, and says that it is one)
  const std::string why = bad_point_args(h, kde.cols ? "" : "no columns are set (gwi_set_kde_columns)", thetas, k, {{"out", out}, {"dead", dead}});
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  namespace M = gwi::moment;
  M::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);  // (as gwi_set_kde_columns found it)
  if (st != GWI_OK) return st;
  const bool with_pe = kde.d_x_pe.ptr != nullptr, with_inj = kde.d_x_inj.ptr != nullptr;
  const size_t n_segs = (size_t)(h->n_ev + 1), cols = (size_t)kde.cols, pairs = (size_t)M::pairs_of(kde.cols), per_point = n_segs * (cols + pairs);
  MomentBuffers& mom = h->moment;
  GWI_HIP(mom.d_partial.reserve((size_t)n_tiles * (cols + pairs)));
  GWI_HIP(mom.d_stage.reserve((size_t)kStagePoints * per_point));
  GWI_HIP(mom.d_dead.reserve((size_t)kStagePoints * n_segs));
  StagedRows rows(h, k);  // (n_ev + 1)(n_cols + P) doubles and n_ev + 1 ints per point
  rows.add(out, mom.d_stage.ptr, per_point);
  rows.add(dead, mom.d_dead.ptr, n_segs);
  // a set without columns is left out of the tile launches; its segments come back NaN
  const QueryCover cover(with_pe, with_inj, h->n_ev, a.d);
  a.x_pe = kde.d_x_pe;
  a.x_inj = kde.d_x_inj;
  a.part1 = mom.d_partial;
  a.part2 = mom.d_partial + (size_t)n_tiles * cols;
  a.n_cols = kde.cols;
  a.first_tile = cover.first_tile;
  a.first_seg = cover.first_seg;
  a.n_seg_covered = (int)cover.segs;
  const auto means = [&](int p) {  // into the point's slot of the stage
    a.out = rows.slot<double>(0, p);
    a.dead = rows.slot<int>(1, p);
    if (cover.tiles) hipLaunchKernelGGL(M::moment_sum_kernel, dim3((unsigned)cover.tiles), dim3(M::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(M::moment_mean_kernel, dim3((unsigned)n_segs), dim3(64), 0, h->stream, a);
  };
  const auto covariances = [&](int) {
    if (cover.tiles) M::launch_cov((unsigned)cover.tiles, h->stream, a);
    hipLaunchKernelGGL(M::moment_merge_kernel, dim3((unsigned)n_segs), dim3(64), 0, h->stream, a);
  };
  return per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_point_moment_times, 2, 6, means, covariances, [&](int p) { return rows.after(p); });
}

void gwi_point_moment_times(double* logw_ms, double* mean_ms, double* cov_ms, int32_t* launches) { g_point_moment_times.report(logw_ms, mean_ms, cov_ms, launches); }

// ---- per-point conditional moments: a bin's share, and the mean and variance of y given the bin of x (gwi_cond.h) ---------------------
// (the kernels' header is included here and not at the top: their host stubs then lie behind the evaluation path -- ConditionalBuffers)
}  // extern "C"
#include "gwi_cond.h"
namespace {
__attribute__((noinline)) void release_moment_and_conditional_buffers(gwi_handle h) {
  h->moment = MomentBuffers();
  delete h->cond;
  h->cond = nullptr;
  delete h->rankcorr;
  h->rankcorr = nullptr;
  delete h->tail;
  h->tail = nullptr;
  delete h->boot;
  h->boot = nullptr;
  delete h->hist2d;
  h->hist2d = nullptr;
}
}  // namespace
extern "C" {
static thread_local StageTimes g_point_conditional_times;

gwi_status gwi_point_conditionals(gwi_handle h, const double* thetas, int32_t k, int32_t n_pairs, const int32_t* pairs, double* out, int32_t* dead) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_conditionals";
  g_point_conditional_times = StageTimes();
  namespace Q = gwi::cond;
  const PostprocessBuffers::Histogram& hist = h->post.hist;
  const PostprocessBuffers::Kde& kde = h->post.kde;
  gwi_status st = post_preflight(h, who, "sum on", "the injection moments need", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments: a shard cannot be given bins or columns, and says that it is one)
  const bool with_pe = hist.d_bins_pe.ptr != nullptr && kde.d_x_pe.ptr != nullptr, with_inj = hist.d_bins_inj.ptr != nullptr && kde.d_x_inj.ptr != nullptr;
  const char* unset = !hist.cols ? "no bins are set (gwi_set_histogram_bins)" : !kde.cols ? "no columns are set (gwi_set_kde_columns)" : "";
  std::string why = bad_point_args(h, unset, thetas, k, {{"pairs", pairs}, {"out", out}, {"dead", dead}});
  if (why.empty() && (n_pairs < 1 || n_pairs > Q::kMaxPairs)) why = "n_pairs = " + std::to_string(n_pairs) + " is not in 1 ... " + std::to_string(Q::kMaxPairs);
  for (int r = 0; why.empty() && r < n_pairs; ++r) {
    const int cx = pairs[2 * r], cy = pairs[2 * r + 1];
    if (cx < 0 || cx >= hist.cols)
      why = "pair " + std::to_string(r) + ": bin column " + std::to_string(cx) + " is not in 0 ... " + std::to_string(hist.cols - 1) + " (gwi_set_histogram_bins)";
    else if (cy < 0 || cy >= kde.cols)
      why = "pair " + std::to_string(r) + ": value column " + std::to_string(cy) + " is not in 0 ... " + std::to_string(kde.cols - 1) + " (gwi_set_kde_columns)";
  }
  if (why.empty() && n_pairs * hist.bins > Q::kMaxItems) why = "n_pairs n_bins = " + std::to_string(n_pairs * hist.bins) + " exceeds " + std::to_string(Q::kMaxItems);
  if (why.empty() && !with_pe && !with_inj) why = "no sample set has both bins and columns: the bins are set for one set, the columns for the other";
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  Q::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);  // (as the two setters found it)
  if (st != GWI_OK) return st;
  const size_t n_segs = (size_t)(h->n_ev + 1), items = (size_t)n_pairs * (size_t)hist.bins, per_point = n_segs * Q::kSlots * items;
  if (!h->cond) h->cond = new (std::nothrow) ConditionalBuffers();
  if (!h->cond) return fail(h, GWI_ERR_INVALID, std::string(who) + ": out of host memory");
  ConditionalBuffers& cb = *h->cond;
  GWI_HIP(cb.d_partial.reserve((size_t)n_tiles * Q::kSlots * items));
  GWI_HIP(cb.d_bin_w.reserve(n_segs * items));
  GWI_HIP(cb.d_stage.reserve((size_t)kStagePoints * per_point));
  GWI_HIP(cb.d_dead.reserve((size_t)kStagePoints * n_segs));
  StagedRows rows(h, k);  // 3 (n_ev + 1) n_pairs n_bins doubles and n_ev + 1 ints per point
  rows.add(out, cb.d_stage.ptr, per_point);
  rows.add(dead, cb.d_dead.ptr, n_segs);
  // a set without bins or without columns is left out of the tile launches; its segments come back NaN
  const QueryCover cover(with_pe, with_inj, h->n_ev, a.d);
  a.bins_pe = hist.d_bins_pe;
  a.bins_inj = hist.d_bins_inj;
  a.x_pe = kde.d_x_pe;
  a.x_inj = kde.d_x_inj;
  a.part1 = cb.d_partial;
  a.part2 = cb.d_partial + (size_t)n_tiles * 2 * items;
  a.bin_w = cb.d_bin_w;
  a.n_pairs = n_pairs;
  a.n_bins = hist.bins;
  for (int r = 0; r < n_pairs; ++r) {  // the pairs' distinct columns, in the order of their first use
    const int cx = pairs[2 * r], cy = pairs[2 * r + 1];
    int ix = 0, iy = 0;
    while (ix < a.n_x && a.x_col[ix] != cx) ++ix;
    while (iy < a.n_y && a.y_col[iy] != cy) ++iy;
    if (ix == a.n_x) a.x_col[a.n_x++] = cx;
    if (iy == a.n_y) a.y_col[a.n_y++] = cy;
    a.pair_x[r] = ix;
    a.pair_y[r] = iy;
  }
  a.first_tile = cover.first_tile;
  a.first_seg = cover.first_seg;
  a.n_seg_covered = (int)cover.segs;
  const dim3 merge_grid((unsigned)n_segs, (unsigned)n_pairs);
  const auto means = [&](int p) {  // into the point's slot of the stage
    a.out = rows.slot<double>(0, p);
    a.dead = rows.slot<int>(1, p);
    if (cover.tiles) Q::launch_tiles<false>((unsigned)cover.tiles, h->stream, a);
    hipLaunchKernelGGL(Q::cond_mean_kernel, merge_grid, dim3(Q::kBlock), 0, h->stream, a);
  };
  const auto variances = [&](int) {
    if (cover.tiles) Q::launch_tiles<true>((unsigned)cover.tiles, h->stream, a);
    hipLaunchKernelGGL(Q::cond_var_kernel, merge_grid, dim3(Q::kBlock), 0, h->stream, a);
  };
  return per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_point_conditional_times, 2, 6, means, variances, [&](int p) { return rows.after(p); });
}

void gwi_point_conditional_times(double* logw_ms, double* mean_ms, double* var_ms, int32_t* launches) { g_point_conditional_times.report(logw_ms, mean_ms, var_ms, launches); }

// ---- per-point rank correlations: weighted mid-ranks within the pooled PE samples and within the injections (gwi_rankcorr.h) ----------
// (the header is included here for gwi_cond.h's reason)
}  // extern "C"
#include "gwi_rankcorr.h"
namespace {
// what is wrong with one rank set's codes, or an empty string: every order a permutation of the set's n members, every rank in [0, n],
// lt <= position of the member along the order < le
std::string bad_rankcorr_codes(const char* set, int n_cols, long long n, const int32_t* order, const int32_t* lt, const int32_t* le) {
  std::vector<int32_t> pos((size_t)n);
  for (int c = 0; c < n_cols; ++c) {
    std::fill(pos.begin(), pos.end(), -1);
    const int32_t* o = order + (size_t)c * (size_t)n;
    for (long long r = 0; r < n; ++r) {
      const long long i = o[r];
      if (i < 0 || i >= n || pos[(size_t)i] >= 0)
        return std::string("order_") + set + " column " + std::to_string(c) + ": position " + std::to_string(r) + " holds " + std::to_string(i) + ": not a permutation of the set's " +
               std::to_string(n) + " members";
      pos[(size_t)i] = (int32_t)r;
    }
    const int32_t* below = lt + (size_t)c * (size_t)n;
    const int32_t* upto = le + (size_t)c * (size_t)n;
    for (long long i = 0; i < n; ++i) {
      const std::string where = std::string("_") + set + " column " + std::to_string(c) + ", member " + std::to_string(i) + ": ";
      if (below[i] < 0 || below[i] > n) return "lt" + where + std::to_string(below[i]) + " is not in 0 ... n = " + std::to_string(n);
      if (upto[i] < 0 || upto[i] > n) return "le" + where + std::to_string(upto[i]) + " is not in 0 ... n = " + std::to_string(n);
      if (below[i] > upto[i]) return "lt" + where + std::to_string(below[i]) + " exceeds le = " + std::to_string(upto[i]);
      if (below[i] > pos[(size_t)i] || pos[(size_t)i] >= upto[i])
        return "lt" + where + "the member's position " + std::to_string(pos[(size_t)i]) + " along the order is not in lt = " + std::to_string(below[i]) + " ... le - 1 = " + std::to_string(upto[i] - 1);
    }
  }
  return "";
}
}  // namespace
extern "C" {
static thread_local StageTimes g_point_rankcorr_times;

gwi_status gwi_set_rankcorr_columns(gwi_handle h, int32_t n_cols, const int32_t* order_obs, const int32_t* lt_obs, const int32_t* le_obs, const int32_t* order_det,
                                    const int32_t* lt_det, const int32_t* le_det) {
  if (!h) return GWI_ERR_INVALID;
  namespace R = gwi::rankcorr;
  const char* who = "gwi_set_rankcorr_columns";
  gwi_status st = post_preflight(h, who, "keep the columns on", "the rank sets need", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments: a shard says that it is one)
  const long long n_obs = h->n_ev * h->n_pe, n_det = h->n_inj;
  std::string why;
  if (n_cols < 1 || n_cols > R::kMaxCols) why = "n_cols = " + std::to_string(n_cols) + " is not in 1 ... " + std::to_string(R::kMaxCols);
  else if (!order_obs || !lt_obs || !le_obs || !order_det || !lt_det || !le_det) why = "order_obs, lt_obs, le_obs, order_det, lt_det or le_det is null";
  else if (n_obs >= 0x7fffffffLL || n_det >= 0x7fffffffLL) why = "more members of a set than an int32 rank can count";
  else why = bad_rankcorr_codes("obs", n_cols, n_obs, order_obs, lt_obs, le_obs);
  if (why.empty()) why = bad_rankcorr_codes("det", n_cols, n_det, order_det, lt_det, le_det);
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  gwi::draw::DrawArgs geometry;
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &geometry, &n_tiles);
  if (st != GWI_OK) return st;
  // the previous columns go away first: should an allocation fail, gwi_point_rank_correlations refuses until they are set again
  delete h->rankcorr;
  h->rankcorr = new (std::nothrow) RankcorrBuffers();
  if (!h->rankcorr) return fail(h, GWI_ERR_INVALID, std::string(who) + ": out of host memory");
  RankcorrBuffers& rc = *h->rankcorr;
  const size_t cols = (size_t)n_cols, obs = cols * (size_t)n_obs, det = cols * (size_t)n_det, items = (size_t)R::items_of(n_cols);
  const size_t order_tiles = (size_t)(gwi::draw::tiles_of(n_obs) + gwi::draw::tiles_of(n_det)), n_prefix = cols * (size_t)(n_obs + 1 + n_det + 1);
  GWI_HIP(rc.d_codes.reserve(3 * (obs + det)));
  const int32_t* src[6] = {order_obs, lt_obs, le_obs, order_det, lt_det, le_det};
  for (int i = 0; i < 6; ++i) {
    const size_t count = i < 3 ? obs : det, at = i < 3 ? (size_t)i * obs : 3 * obs + (size_t)(i - 3) * det;
    if (count) GWI_HIP(hipMemcpy(rc.d_codes.ptr + at, src[i], sizeof(int32_t) * count, hipMemcpyHostToDevice));
  }
  GWI_HIP(rc.d_tiles.reserve(2 * cols * order_tiles + 1));
  GWI_HIP(rc.d_prefix.reserve(n_prefix));
  GWI_HIP(rc.d_partial.reserve((size_t)n_tiles * items + 1));
  GWI_HIP(rc.d_stage.reserve((size_t)kStagePoints * R::kSets * items));
  GWI_HIP(rc.d_dead.reserve((size_t)kStagePoints * (size_t)(h->n_ev + 2)));
  GWI_HIP(hipMemset(rc.d_prefix, 0, sizeof(double) * n_prefix));  // (an empty set launches nothing that would store P[c][0])
  rc.cols = n_cols;
  return GWI_OK;
}

gwi_status gwi_point_rank_correlations(gwi_handle h, const double* thetas, int32_t k, double* out, int32_t* dead) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_rank_correlations";
  g_point_rankcorr_times = StageTimes();
  gwi_status st = post_preflight(h, who, "sum on", "the rank sets need", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments)
  const bool set = h->rankcorr && h->rankcorr->cols;
  const std::string why = bad_point_args(h, set ? "" : "no rank-correlation columns are set (gwi_set_rankcorr_columns)", thetas, k, {{"out", out}, {"dead", dead}});
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  namespace R = gwi::rankcorr;
  RankcorrBuffers& rc = *h->rankcorr;
  R::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);  // (as gwi_set_rankcorr_columns found it)
  if (st != GWI_OK) return st;
  const size_t cols = (size_t)rc.cols, items = (size_t)R::items_of(rc.cols), n_obs = (size_t)(h->n_ev * h->n_pe), n_det = (size_t)h->n_inj;
  const size_t obs = cols * n_obs, det = cols * n_det;
  a.n[R::kObs] = (long long)n_obs;
  a.n[R::kDet] = (long long)n_det;
  a.order_tiles[R::kObs] = (int)gwi::draw::tiles_of((long long)n_obs);
  a.order_tiles[R::kDet] = (int)gwi::draw::tiles_of((long long)n_det);
  const unsigned order_tiles = (unsigned)(a.order_tiles[R::kObs] + a.order_tiles[R::kDet]);
  a.order[R::kObs] = rc.d_codes;
  a.lt[R::kObs] = rc.d_codes + obs;
  a.le[R::kObs] = rc.d_codes + 2 * obs;
  a.order[R::kDet] = rc.d_codes + 3 * obs;
  a.lt[R::kDet] = rc.d_codes + 3 * obs + det;
  a.le[R::kDet] = rc.d_codes + 3 * obs + 2 * det;
  a.prefix[R::kObs] = rc.d_prefix;
  a.prefix[R::kDet] = rc.d_prefix + cols * (n_obs + 1);
  a.tile_sum = rc.d_tiles;
  a.tile_off = rc.d_tiles + cols * order_tiles;
  a.partial = rc.d_partial;
  a.n_cols = rc.cols;
  StagedRows rows(h, k);  // 2 (1 + C + C (C + 1) / 2) doubles and n_ev + 2 ints per point
  rows.add(out, rc.d_stage.ptr, (size_t)R::kSets * items);
  rows.add(dead, rc.d_dead.ptr, (size_t)(h->n_ev + 2));
  const auto prefix = [&](int) {
    if (!order_tiles) return;
    hipLaunchKernelGGL(R::rankcorr_tile_kernel, dim3(order_tiles, (unsigned)cols), dim3(R::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(R::rankcorr_offset_kernel, dim3((unsigned)cols, R::kSets), dim3(64), 0, h->stream, a);
    hipLaunchKernelGGL(R::rankcorr_prefix_kernel, dim3(order_tiles, (unsigned)cols), dim3(R::kBlock), 0, h->stream, a);
  };
  const auto covariances = [&](int p) {  // into the point's slot of the stage
    a.out = rows.slot<double>(0, p);
    a.dead = rows.slot<int>(1, p);
    if (n_tiles) R::launch_cov((unsigned)n_tiles, h->stream, a);
    hipLaunchKernelGGL(R::rankcorr_merge_kernel, dim3(R::kSets), dim3(64), 0, h->stream, a);
  };
  return per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_point_rankcorr_times, 2, 7, prefix, covariances, [&](int p) { return rows.after(p); });
}

void gwi_point_rankcorr_times(double* logw_ms, double* prefix_ms, double* cov_ms, int32_t* launches) { g_point_rankcorr_times.report(logw_ms, prefix_ms, cov_ms, launches); }

// ---- per-point tails: the m largest live log-weights of every segment, the cut-off below them and the rest's sum (gwi_tail.h) ----------
// (the header is included here for gwi_cond.h's reason)
}  // extern "C"
#include "gwi_tail.h"
extern "C" {
static thread_local StageTimes g_point_tail_times;

gwi_status gwi_set_tail_sizes(gwi_handle h, int32_t m_pe, int32_t m_inj) {
  if (!h) return GWI_ERR_INVALID;
  namespace T = gwi::tail;
  const char* who = "gwi_set_tail_sizes";
  gwi_status st = post_preflight(h, who, "keep a tail on", "the injection tail needs", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments: a shard says that it is one)
  std::string why;
  const auto bad = [&](const char* name, int m, long long n, const char* n_name) -> std::string {
    if (m < 1 || m > T::kMaxTail) return std::string(name) + " = " + std::to_string(m) + " is not in 1 ... " + std::to_string(T::kMaxTail);
    if (m >= n) return std::string(name) + " = " + std::to_string(m) + " is not below " + n_name + " = " + std::to_string(n);
    return "";
  };
  why = bad("m_pe", m_pe, h->n_pe, "n_pe");
  if (why.empty()) why = bad("m_inj", m_inj, h->n_inj, "n_inj");
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  if (!h->tail) h->tail = new (std::nothrow) TailBuffers();
  if (!h->tail) return fail(h, GWI_ERR_INVALID, std::string(who) + ": out of host memory");
  h->tail->m_pe = m_pe;
  h->tail->m_inj = m_inj;
  return GWI_OK;
}

gwi_status gwi_point_tails(gwi_handle h, const double* thetas, int32_t k, double* tail, double* stats, int32_t* counts) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_tails";
  g_point_tail_times = StageTimes();
  gwi_status st = post_preflight(h, who, "select on", "the injection tail needs", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments)
  const bool set = h->tail && h->tail->m_pe > 0;
  const std::string why = bad_point_args(h, set ? "" : "no tail sizes are set (gwi_set_tail_sizes)", thetas, k, {{"tail", tail}, {"stats", stats}, {"counts", counts}});
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  namespace T = gwi::tail;
  TailBuffers& tb = *h->tail;
  T::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);
  if (st != GWI_OK) return st;
  const size_t n_segs = (size_t)(h->n_ev + 1), tiles = (size_t)n_tiles, row = (size_t)h->n_ev * (size_t)tb.m_pe + (size_t)tb.m_inj;
  GWI_HIP(tb.d_keys.reserve(n_segs + tiles));
  GWI_HIP(tb.d_hist.reserve(tiles * T::kHistStride + 1));
  GWI_HIP(tb.d_ints.reserve(2 * n_segs + tiles * T::kTileInts));
  GWI_HIP(tb.d_body.reserve(tiles + 1));
  GWI_HIP(tb.d_tail.reserve((size_t)kStagePoints * row));
  GWI_HIP(tb.d_stats.reserve((size_t)kStagePoints * n_segs * T::kStats));
  GWI_HIP(tb.d_counts.reserve((size_t)kStagePoints * n_segs * T::kCounts));
  a.prefix = tb.d_keys;
  a.tile_below = tb.d_keys.ptr + n_segs;
  a.hist = tb.d_hist;
  a.rank = tb.d_ints;
  a.tile_counts = tb.d_ints.ptr + 2 * n_segs;
  a.tile_body = tb.d_body;
  a.m_pe = tb.m_pe;
  a.m_inj = tb.m_inj;
  StagedRows rows(h, k);  // n_ev m_pe + m_inj + 4 (n_ev + 1) doubles and 4 (n_ev + 1) ints per point
  rows.add(tail, tb.d_tail.ptr, row);
  rows.add(stats, tb.d_stats.ptr, n_segs * T::kStats);
  rows.add(counts, tb.d_counts.ptr, n_segs * T::kCounts);
  const auto selection = [&](int) {  // the same launches whatever the data are
    for (a.pass = 0; a.pass < T::kPasses; ++a.pass) {
      if (n_tiles) hipLaunchKernelGGL(T::tail_hist_kernel, dim3((unsigned)n_tiles), dim3(T::kBlock), 0, h->stream, a);
      hipLaunchKernelGGL(T::tail_pick_kernel, dim3((unsigned)n_segs), dim3(T::kBlock), 0, h->stream, a);
    }
  };
  const auto collection = [&](int p) {  // into the point's slot of the stage
    a.tail = rows.slot<double>(0, p);
    a.stats = rows.slot<double>(1, p);
    a.counts = rows.slot<int>(2, p);
    if (n_tiles) hipLaunchKernelGGL(T::tail_collect_kernel, dim3((unsigned)n_tiles), dim3(T::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(T::tail_merge_kernel, dim3((unsigned)n_segs), dim3(T::kBlock), 0, h->stream, a);
  };
  return per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_point_tail_times, 2, 2 + 2 * T::kPasses + 2, selection, collection, [&](int p) { return rows.after(p); });
}

void gwi_point_tail_times(double* logw_ms, double* select_ms, double* collect_ms, int32_t* launches) { g_point_tail_times.report(logw_ms, select_ms, collect_ms, launches); }

// ---- bootstrap replicates of the inner importance sums: the same Poisson resampling of every segment at every point (gwi_boot.h) ------
// (the header is included here for gwi_cond.h's reason)
}  // extern "C"
#include "gwi_boot.h"
extern "C" {
static thread_local StageTimes g_point_bootstrap_times;

gwi_status gwi_set_bootstrap(gwi_handle h, uint64_t seed, int32_t n_replicates, int32_t first_replicate) {
  if (!h) return GWI_ERR_INVALID;
  namespace B = gwi::boot;
  const char* who = "gwi_set_bootstrap";
  gwi_status st = post_preflight(h, who, "resample on", "the injection replicates need", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments: a shard says that it is one)
  if (n_replicates < 1 || n_replicates > B::kMaxReplicates)
    return fail(h, GWI_ERR_INVALID, std::string(who) + ": n_replicates = " + std::to_string(n_replicates) + " is not in 1 ... " + std::to_string(B::kMaxReplicates));
  if (first_replicate < 0 || (long long)first_replicate + n_replicates > B::kMaxReplicate)
    return fail(h, GWI_ERR_INVALID, std::string(who) + ": first_replicate = " + std::to_string(first_replicate) + " is negative or first_replicate + n_replicates exceeds " +
                                        std::to_string(B::kMaxReplicate));
  if (!h->boot) h->boot = new (std::nothrow) BootBuffers();
  if (!h->boot) return fail(h, GWI_ERR_INVALID, std::string(who) + ": out of host memory");
  h->boot->seed = seed;
  h->boot->n_rep = n_replicates;
  h->boot->first_rep = first_replicate;
  return GWI_OK;
}

gwi_status gwi_point_bootstrap(gwi_handle h, const double* thetas, int32_t k, double* sums, double* stats, int32_t* dead, int64_t* counts) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_bootstrap";
  g_point_bootstrap_times = StageTimes();
  gwi_status st = post_preflight(h, who, "resample on", "the injection replicates need", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments)
  const bool set = h->boot && h->boot->n_rep > 0;
  const std::string why = bad_point_args(h, set ? "" : "no replicates are set (gwi_set_bootstrap)", thetas, k, {{"sums", sums}, {"stats", stats}, {"dead", dead}, {"counts", counts}});
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  namespace B = gwi::boot;
  BootBuffers& bb = *h->boot;
  B::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);
  if (st != GWI_OK) return st;
  const size_t n_segs = (size_t)(h->n_ev + 1), tiles = (size_t)n_tiles, n_rep = (size_t)bb.n_rep;
  GWI_HIP(bb.d_tile_sum.reserve(tiles * n_rep + 1));
  GWI_HIP(bb.d_tile_count.reserve(tiles * n_rep + 1));
  GWI_HIP(bb.d_sums.reserve((size_t)kStagePoints * n_segs * n_rep));
  GWI_HIP(bb.d_stats.reserve((size_t)kStagePoints * n_segs * B::kStats));
  GWI_HIP(bb.d_dead.reserve((size_t)kStagePoints * n_segs));
  GWI_HIP(bb.d_counts.reserve(n_segs * n_rep));
  a.tile_sum = bb.d_tile_sum;
  a.tile_count = bb.d_tile_count;
  a.counts = bb.d_counts;
  a.seed = bb.seed;
  a.n_rep = bb.n_rep;
  a.first_rep = bb.first_rep;
  StagedRows rows(h, k);  // (n_ev + 1)(B + 2) doubles and n_ev + 1 ints per point
  rows.add(sums, bb.d_sums.ptr, n_segs * n_rep);
  rows.add(stats, bb.d_stats.ptr, n_segs * B::kStats);
  rows.add(dead, bb.d_dead.ptr, n_segs);
  const auto tile = [&](int p) {
    a.want_counts = p == 0;  // the counts do not depend on the point
    if (n_tiles) hipLaunchKernelGGL(B::boot_tile_kernel, dim3((unsigned)n_tiles), dim3(B::kBlock), 0, h->stream, a);
  };
  const auto merge = [&](int p) {  // into the point's slot of the stage
    a.sums = rows.slot<double>(0, p);
    a.stats = rows.slot<double>(1, p);
    a.dead = rows.slot<int>(2, p);
    hipLaunchKernelGGL(B::boot_merge_kernel, dim3((unsigned)n_segs), dim3(B::kBlock), 0, h->stream, a);
  };
  st = per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_point_bootstrap_times, 2, 4, tile, merge, [&](int p) { return rows.after(p); });
  if (st != GWI_OK) return st;
  GWI_HIP(hipMemcpy(counts, bb.d_counts.ptr, n_segs * n_rep * sizeof(long long), hipMemcpyDeviceToHost));
  return GWI_OK;
}

void gwi_point_bootstrap_times(double* logw_ms, double* tile_ms, double* merge_ms, int32_t* launches) { g_point_bootstrap_times.report(logw_ms, tile_ms, merge_ms, launches); }

// ---- per-point joint histograms of two bin columns: every segment's table, the catalog's mixture, the predicted table (gwi_hist2d.h) --
// (the header is included here for gwi_cond.h's reason)
}  // extern "C"
#include "gwi_hist2d.h"
extern "C" {
static thread_local StageTimes g_point_hist2d_times;

gwi_status gwi_point_histograms2d(gwi_handle h, const double* thetas, int32_t k, int32_t n_pairs, const int32_t* pairs, const double* v, double* hist_pe, double* hist_inj,
                                  double* obs, double* pred, int32_t* live, int32_t* n_dead, double* vsum) {
  if (!h) return GWI_ERR_INVALID;
  const char* who = "gwi_point_histograms2d";
  g_point_hist2d_times = StageTimes();
  namespace J = gwi::hist2d;
  const PostprocessBuffers::Histogram& hist = h->post.hist;
  gwi_status st = post_preflight(h, who, "sum on", "the injection table needs", [&] { return std::string(h->variant ? "" : "the engine has no scan kernel"); });
  if (st != GWI_OK) return st;
  // (after the shard refusal, as gwi_point_moments: a shard cannot be given bins, and says that it is one)
  const bool with_pe = hist.d_bins_pe.ptr != nullptr, with_inj = hist.d_bins_inj.ptr != nullptr;
  std::string why = bad_point_args(h, hist.cols ? "" : "no bins are set (gwi_set_histogram_bins)", thetas, k, {{"pairs", pairs}, {"obs", obs}, {"pred", pred}, {"live", live}});
  if (why.empty() && (n_pairs < 1 || n_pairs > J::kMaxPairs)) why = "n_pairs = " + std::to_string(n_pairs) + " is not in 1 ... " + std::to_string(J::kMaxPairs);
  for (int r = 0; why.empty() && r < n_pairs; ++r)
    for (int side = 0; why.empty() && side < 2; ++side)
      if (pairs[2 * r + side] < 0 || pairs[2 * r + side] >= hist.cols)
        why = "pair " + std::to_string(r) + ": bin column " + std::to_string(pairs[2 * r + side]) + " is not in 0 ... " + std::to_string(hist.cols - 1) + " (gwi_set_histogram_bins)";
  if (why.empty() && hist.bins > J::kMaxBins)
    why = "the bins were set with n_bins = " + std::to_string(hist.bins) + ": a joint table takes at most " + std::to_string(J::kMaxBins) + " bins per axis";
  if (why.empty() && v) why = bad_point_weights(v, k, h->n_ev + 1);
  if (!why.empty()) return fail(h, GWI_ERR_INVALID, std::string(who) + ": " + why);
  J::Args a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);  // (as gwi_set_histogram_bins found it)
  if (st != GWI_OK) return st;
  const size_t n_segs = (size_t)(h->n_ev + 1), n_cells = (size_t)hist.bins * (size_t)hist.bins, per_point = (size_t)n_pairs * n_cells;
  const size_t per_seg = per_point, n_pe_out = (size_t)h->n_ev * per_seg;
  if (!h->hist2d) h->hist2d = new (std::nothrow) Hist2dBuffers();
  if (!h->hist2d) return fail(h, GWI_ERR_INVALID, std::string(who) + ": out of host memory");
  Hist2dBuffers& jb = *h->hist2d;
  GWI_HIP(jb.d_partial.reserve((size_t)n_tiles * n_cells));
  GWI_HIP(jb.d_share.reserve(n_segs * n_cells));
  GWI_HIP(jb.d_seg_dead.reserve(n_segs));
  GWI_HIP(jb.d_obs.reserve((size_t)kStagePoints * per_point));
  GWI_HIP(jb.d_pred.reserve((size_t)kStagePoints * per_point));
  GWI_HIP(jb.d_live.reserve((size_t)kStagePoints * 2));
  // the caller's running sums: the points of this call are added onto them, so a request may be split over calls
  const bool sum_pe = with_pe && hist_pe && n_pe_out, sum_inj = with_inj && hist_inj;
  if (sum_pe || sum_inj) {
    GWI_HIP(jb.d_sums.reserve(n_segs * per_seg));
    if (sum_pe) GWI_HIP(hipMemcpy(jb.d_sums, hist_pe, sizeof(double) * n_pe_out, hipMemcpyHostToDevice));
    else if (n_pe_out) GWI_HIP(hipMemsetAsync(jb.d_sums, 0, sizeof(double) * n_pe_out, h->stream));
    if (sum_inj) GWI_HIP(hipMemcpy(jb.d_sums + n_pe_out, hist_inj, sizeof(double) * per_seg, hipMemcpyHostToDevice));
    else GWI_HIP(hipMemsetAsync(jb.d_sums + n_pe_out, 0, sizeof(double) * per_seg, h->stream));
    a.hist = jb.d_sums;
  }
  if (n_dead) {
    GWI_HIP(jb.d_dead.reserve(n_segs));
    GWI_HIP(hipMemcpy(jb.d_dead, n_dead, sizeof(int) * n_segs, hipMemcpyHostToDevice));
    a.n_dead = jb.d_dead;
  }
  const double* d_v = nullptr;
  if (v) {
    st = upload_point_weights(h, v, k, &d_v);
    if (st != GWI_OK) return st;
    if (vsum) {
      GWI_HIP(jb.d_vsum.reserve(n_segs));
      GWI_HIP(hipMemcpy(jb.d_vsum, vsum, sizeof(double) * n_segs, hipMemcpyHostToDevice));
      a.vsum = jb.d_vsum;
    }
  }
  StagedRows rows(h, k);  // 2 n_pairs B B doubles and two ints per point
  rows.add(obs, jb.d_obs.ptr, per_point);
  rows.add(pred, jb.d_pred.ptr, per_point);
  rows.add(live, jb.d_live.ptr, 2);
  // a set without bins is left out of the tile and merge launches; its side of the point's rows comes back NaN
  const QueryCover cover(with_pe, with_inj, h->n_ev, a.d);
  a.bins_pe = hist.d_bins_pe;
  a.bins_inj = hist.d_bins_inj;
  a.partial = jb.d_partial;
  a.share = jb.d_share;
  a.seg_dead = jb.d_seg_dead;
  a.n_bins = hist.bins;
  a.n_pairs = n_pairs;
  a.first_tile = cover.first_tile;
  a.first_seg = cover.first_seg;
  a.with_pe = with_pe ? 1 : 0;
  a.with_inj = with_inj ? 1 : 0;
  const unsigned cell_blocks = (unsigned)((n_cells + J::kBlock - 1) / J::kBlock);
  const auto pair_tiles = [&](int r) {
    a.pair = r;
    a.cx = pairs[2 * r];
    a.cy = pairs[2 * r + 1];
    if (cover.tiles) hipLaunchKernelGGL(J::hist2d_tile_kernel, dim3((unsigned)cover.tiles), dim3(J::kBlock), sizeof(double) * n_cells, h->stream, a);
  };
  const auto pair_rest = [&]() {
    if (cover.segs) hipLaunchKernelGGL(J::hist2d_merge_kernel, dim3((unsigned)cover.segs, cell_blocks), dim3(J::kBlock), 0, h->stream, a);
    hipLaunchKernelGGL(J::hist2d_mix_kernel, dim3(cell_blocks), dim3(J::kBlock), 0, h->stream, a);
  };
  // the timed split is that of the first pair: tile | merge + mix; the launches of the pairs that follow (one pair's partials are
  // the whole workspace, so they run after the first pair's merge) are counted in the second stage
  const auto tile = [&](int p) {  // into the point's slot of the stage
    a.obs = rows.slot<double>(0, p);
    a.pred = rows.slot<double>(1, p);
    a.live = rows.slot<int>(2, p);
    a.v = d_v ? d_v + (size_t)p * n_segs : nullptr;
    pair_tiles(0);
  };
  const auto rest = [&](int) {
    pair_rest();
    for (int r = 1; r < n_pairs; ++r) {
      pair_tiles(r);
      pair_rest();
    }
  };
  st = per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_point_hist2d_times, 2, 2 + 3 * n_pairs, tile, rest, [&](int p) { return rows.after(p); });
  if (st != GWI_OK) return st;
  if (sum_pe) GWI_HIP(hipMemcpy(hist_pe, jb.d_sums, sizeof(double) * n_pe_out, hipMemcpyDeviceToHost));
  if (sum_inj) GWI_HIP(hipMemcpy(hist_inj, jb.d_sums + n_pe_out, sizeof(double) * per_seg, hipMemcpyDeviceToHost));
  if (n_dead) GWI_HIP(hipMemcpy(n_dead, jb.d_dead, sizeof(int) * n_segs, hipMemcpyDeviceToHost));
  if (a.vsum) GWI_HIP(hipMemcpy(vsum, jb.d_vsum, sizeof(double) * n_segs, hipMemcpyDeviceToHost));
  return GWI_OK;
}

void gwi_point_hist2d_times(double* logw_ms, double* tile_ms, double* merge_ms, int32_t* launches) { g_point_hist2d_times.report(logw_ms, tile_ms, merge_ms, launches); }

// ---- marginal weights and their quantiles (gwi_quant.h) ---------------------------------------------------------------------
enum { kQuantLogw, kQuantAdd, kQuantQuery };
static thread_local StageTimes g_quantile_times;

// the handle's marginal weights and dead counts on the engine's device (selected by the caller): allocated and zeroed on first use
static gwi_status marginal_state(gwi_handle h) {
  PostprocessBuffers::Marginal& m = h->post.marg;
  if (m.d_w.ptr && m.d_dead.ptr && m.d_vsum.ptr) return GWI_OK;
  const size_t n_w = (size_t)(h->n_ev * h->n_pe) + (size_t)h->n_inj, n_dead = (size_t)(h->n_ev + 1);
  m = PostprocessBuffers::Marginal();
  GWI_HIP(m.d_w.reserve(n_w));
  GWI_HIP(m.d_dead.reserve(n_dead));
  GWI_HIP(m.d_vsum.reserve(2 * n_dead));
  GWI_HIP(hipMemsetAsync(m.d_w, 0, sizeof(double) * (n_w ? n_w : 1), h->stream));
  GWI_HIP(hipMemsetAsync(m.d_dead, 0, sizeof(int) * n_dead, h->stream));
  GWI_HIP(hipMemsetAsync(m.d_vsum, 0, sizeof(double) * 2 * n_dead, h->stream));
  GWI_HIP(hipStreamSynchronize(h->stream));
  return GWI_OK;
}

gwi_status gwi_marginal_weights_reset(gwi_handle h) {
  if (!h) return GWI_ERR_INVALID;
  gwi_status st = post_preflight(h, "gwi_marginal_weights_reset", "keep the weights on", "the injection weights need", []() -> std::string { return ""; });
  if (st != GWI_OK) return st;
  GWI_HIP(hipSetDevice(h->device));
  h->post.marg = PostprocessBuffers::Marginal();  // (zeroed anew on the next use)
  return marginal_state(h);
}

// gwi_marginal_weights_add (weighted = false: v is not looked at) and gwi_marginal_weights_add_weighted
static gwi_status marginal_weights_add(gwi_handle h, const char* who, bool weighted, const double* thetas, int32_t k, const double* v) {
  g_quantile_times = StageTimes();
  gwi_status st = post_preflight(h, who, "sum on", "the injection weights need", [&]() -> std::string {
    if (!h->variant) return "the engine has no scan kernel";
    if (!thetas || k < 0) return "thetas is null or k < 0";
    return weighted ? bad_point_weights(v, k, h->n_ev + 1) : std::string();
  });
  if (st != GWI_OK) return st;
  namespace D = gwi::draw;
  namespace Q = gwi::quant;
  Q::MargArgs a;
  std::memset(&a, 0, sizeof(a));
  long long n_tiles = 0;
  st = draw_workspace(h, who, "tiles", &a.d, &n_tiles);
  if (st != GWI_OK) return st;
  st = marginal_state(h);
  if (st != GWI_OK) return st;
  const double* d_v = nullptr;
  if (weighted) {
    st = upload_point_weights(h, v, k, &d_v);
    if (st != GWI_OK) return st;
  }
  PostprocessBuffers::Marginal& m = h->post.marg;
  a.w_pe = m.d_w;
  a.w_inj = m.d_w + (size_t)(h->n_ev * h->n_pe);
  a.dead = m.d_dead;
  a.vsum = m.d_vsum;
  a.vsum2 = m.d_vsum + (size_t)(h->n_ev + 1);
  const auto add = [&](int p) {
    if (!n_tiles) return;
    if (weighted) {
      a.v = d_v + (size_t)p * (size_t)(h->n_ev + 1);
      hipLaunchKernelGGL(Q::marg_add_kernel<true>, dim3((unsigned)n_tiles), dim3(Q::kBlock), 0, h->stream, a);
    } else {
      hipLaunchKernelGGL(Q::marg_add_kernel<false>, dim3((unsigned)n_tiles), dim3(Q::kBlock), 0, h->stream, a);
    }
  };
  const auto count = [&](int) {  // (completed points only)
    ++m.n_points;
    return GWI_OK;
  };
  return per_point_pass(h, who, thetas, k, &a.d, n_tiles, &g_quantile_times, 1, 3, add, no_stage, count);
}

gwi_status gwi_marginal_weights_add(gwi_handle h, const double* thetas, int32_t k) {
  if (!h) return GWI_ERR_INVALID;
  return marginal_weights_add(h, "gwi_marginal_weights_add", false, thetas, k, nullptr);
}

gwi_status gwi_marginal_weights_add_weighted(gwi_handle h, const double* thetas, int32_t k, const double* v) {
  if (!h) return GWI_ERR_INVALID;
  return marginal_weights_add(h, "gwi_marginal_weights_add_weighted", true, thetas, k, v);
}

gwi_status gwi_marginal_point_weights(gwi_handle h, double* vsum, double* vsum2) {
  if (!h) return GWI_ERR_INVALID;
  gwi_status st = post_preflight(h, "gwi_marginal_point_weights", "keep the weights on", "the injection weights need", [&]() -> std::string {
    if (!vsum || !vsum2) return "vsum or vsum2 is null";
    return "";
  });
  if (st != GWI_OK) return st;
  GWI_HIP(hipSetDevice(h->device));
  st = marginal_state(h);
  if (st != GWI_OK) return st;
  const PostprocessBuffers::Marginal& m = h->post.marg;
  const size_t n = (size_t)(h->n_ev + 1);
  GWI_HIP(hipMemcpy(vsum, m.d_vsum, sizeof(double) * n, hipMemcpyDeviceToHost));
  GWI_HIP(hipMemcpy(vsum2, m.d_vsum + n, sizeof(double) * n, hipMemcpyDeviceToHost));
  return GWI_OK;
}

gwi_status gwi_marginal_weights_read(gwi_handle h, double* pe_w, double* inj_w, int32_t* dead, int64_t* n_points) {
  if (!h) return GWI_ERR_INVALID;
  gwi_status st = post_preflight(h, "gwi_marginal_weights_read", "keep the weights on", "the injection weights need", [&]() -> std::string {
    if (!dead || !n_points) return "dead or n_points is null";
    return "";
  });
  if (st != GWI_OK) return st;
  GWI_HIP(hipSetDevice(h->device));
  st = marginal_state(h);
  if (st != GWI_OK) return st;
  const PostprocessBuffers::Marginal& m = h->post.marg;
  const size_t n_pe_tot = (size_t)(h->n_ev * h->n_pe), n_inj = (size_t)h->n_inj;
  if (pe_w && n_pe_tot) GWI_HIP(hipMemcpy(pe_w, m.d_w, sizeof(double) * n_pe_tot, hipMemcpyDeviceToHost));
  if (inj_w && n_inj) GWI_HIP(hipMemcpy(inj_w, m.d_w + n_pe_tot, sizeof(double) * n_inj, hipMemcpyDeviceToHost));
  GWI_HIP(hipMemcpy(dead, m.d_dead, sizeof(int) * (size_t)(h->n_ev + 1), hipMemcpyDeviceToHost));
  *n_points = m.n_points;
  return GWI_OK;
}

// what is wrong with one set's columns (x and order [n_cols][n_segs][n]), or an empty string: every order a permutation of its
// segment, every value finite, no value smaller than the one before it along the order
static std::string bad_quantile_columns(const char* set, bool with_events, int n_cols, long long n_segs, long long n, const double* x, const int32_t* order) {
  std::vector<unsigned char> seen((size_t)n);
  for (int c = 0; c < n_cols; ++c)
    for (long long s = 0; s < n_segs; ++s) {
      const size_t at = ((size_t)c * (size_t)n_segs + (size_t)s) * (size_t)n;
      const std::string where = std::string(set) + " column " + std::to_string(c) + (with_events ? ", event " + std::to_string(s) : std::string());
      std::fill(seen.begin(), seen.end(), 0);
      double before = -__builtin_inf();
      for (long long r = 0; r < n; ++r) {
        const long long j = order[at + (size_t)r];
        if (j < 0 || j >= n || seen[(size_t)j]) return "order_" + where + ": rank " + std::to_string(r) + " holds " + std::to_string(j) + ": not a permutation of the segment's " + std::to_string(n) + " samples";
        seen[(size_t)j] = 1;
        const double v = x[at + (size_t)j];
        if (!(std::fabs(v) < __builtin_inf())) return "x_" + where + ": sample " + std::to_string(j) + " is not finite";
        if (v < before) return "x_" + where + ": the values decrease along the order at rank " + std::to_string(r);
        before = v;
      }
    }
  return "";
}

gwi_status gwi_set_quantile_columns(gwi_handle h, int32_t n_cols, const double* x_pe, const int32_t* order_pe, const double* x_inj, const int32_t* order_inj) {
  if (!h) return GWI_ERR_INVALID;
  namespace Q = gwi::quant;
  gwi_status st = post_preflight(h, "gwi_set_quantile_columns", "keep the columns on", "the injection quantiles need", [&]() -> std::string {
    if (n_cols < 1 || n_cols > Q::kMaxCols) return "n_cols = " + std::to_string(n_cols) + " is not in 1 ... " + std::to_string(Q::kMaxCols);
    if (!x_pe && !x_inj) return "x_pe and x_inj are both null";
    if ((x_pe != nullptr) != (order_pe != nullptr)) return "x_pe and order_pe are given together";
    if ((x_inj != nullptr) != (order_inj != nullptr)) return "x_inj and order_inj are given together";
    if (h->n_pe > 0x7fffffffLL || h->n_inj > 0x7fffffffLL) return "more samples per segment than an int32 index can address";
    if (x_pe) {
      const std::string why = bad_quantile_columns("pe", true, n_cols, h->n_ev, h->n_pe, x_pe, order_pe);
      if (!why.empty()) return why;
    }
    if (x_inj) return bad_quantile_columns("inj", false, n_cols, 1, h->n_inj, x_inj, order_inj);
    return "";
  });
  if (st != GWI_OK) return st;
  gwi::draw::DrawArgs geometry;
  long long n_tiles = 0;
  st = draw_workspace(h, "gwi_set_quantile_columns", "tiles", &geometry, &n_tiles);
  if (st != GWI_OK) return st;
  // the previous columns go away first: should an allocation fail, gwi_weighted_quantiles refuses until they are set again
  PostprocessBuffers::Quantile& quant = h->post.quant;
  quant = PostprocessBuffers::Quantile();
  const size_t n_pe_vals = x_pe ? (size_t)n_cols * (size_t)(h->n_ev * h->n_pe) : 0, n_inj_vals = x_inj ? (size_t)n_cols * (size_t)h->n_inj : 0;
  if (x_pe) {  // (a set that is given has columns, even where it is empty)
    GWI_HIP(quant.d_x_pe.upload(x_pe, n_pe_vals));
    GWI_HIP(quant.d_order_pe.upload(order_pe, n_pe_vals));
  }
  if (x_inj) {
    GWI_HIP(quant.d_x_inj.upload(x_inj, n_inj_vals));
    GWI_HIP(quant.d_order_inj.upload(order_inj, n_inj_vals));
  }
  GWI_HIP(quant.d_partial.reserve((size_t)n_tiles * (size_t)n_cols * Q::kSums));
  GWI_HIP(quant.d_prefix.reserve((size_t)n_tiles * (size_t)n_cols));
  quant.cols = n_cols;
  return GWI_OK;
}

gwi_status gwi_weighted_quantiles(gwi_handle h, const double* levels, int32_t n_levels, int32_t* idx_pe, int32_t* idx_inj, double* moments_pe, double* moments_inj, double* mass) {
  if (!h) return GWI_ERR_INVALID;
  namespace Q = gwi::quant;
  PostprocessBuffers::Quantile& quant = h->post.quant;
  const bool with_pe = quant.d_x_pe.ptr != nullptr, with_inj = quant.d_x_inj.ptr != nullptr;
  gwi_status st = post_preflight(h, "gwi_weighted_quantiles", "select on", "the injection quantiles need", [&]() -> std::string {
    if (!quant.cols) return "no columns are set (gwi_set_quantile_columns)";
    if (n_levels < 1 || n_levels > Q::kMaxLevels) return "n_levels = " + std::to_string(n_levels) + " is not in 1 ... " + std::to_string(Q::kMaxLevels);
    if (!levels) return "levels is null";
    for (int q = 0; q < n_levels; ++q)
      if (!(levels[q] >= 0.0 && levels[q] <= 1.0)) return "level " + std::to_string(q) + " is " + std::to_string(levels[q]) + ": not in [0, 1]";
    if (with_pe && (!idx_pe || !moments_pe)) return "PE columns are set: idx_pe and moments_pe are needed";
    if (with_inj && (!idx_inj || !moments_inj)) return "injection columns are set: idx_inj and moments_inj are needed";
    if (!mass) return "mass is null";
    return "";
  });
  if (st != GWI_OK) return st;
  gwi::draw::DrawArgs geometry;
  long long n_tiles = 0;
  st = draw_workspace(h, "gwi_weighted_quantiles", "tiles", &geometry, &n_tiles);  // (as gwi_set_quantile_columns found it)
  if (st != GWI_OK) return st;
  st = marginal_state(h);
  if (st != GWI_OK) return st;
  const size_t n_segs = (size_t)(h->n_ev + 1), per_seg_idx = (size_t)quant.cols * (size_t)n_levels, per_seg_mom = (size_t)quant.cols * 2;
  GWI_HIP(quant.d_idx.reserve(n_segs * per_seg_idx));
  GWI_HIP(quant.d_out.reserve(n_segs * per_seg_mom + n_segs));
  GWI_HIP(quant.d_levels.upload(levels, (size_t)n_levels));
  GWI_HIP(hipMemsetAsync(quant.d_out, 0, sizeof(double) * (n_segs * per_seg_mom + n_segs), h->stream));  // (the mass of a set that is left out)
  Q::Args a;
  std::memset(&a, 0, sizeof(a));
  // a set without columns is left out of the launches
  const QueryCover cover(with_pe, with_inj, h->n_ev, geometry);
  fill_query_args(h, geometry, cover, &a);
  a.x_pe = quant.d_x_pe;
  a.x_inj = quant.d_x_inj;
  a.order_pe = quant.d_order_pe;
  a.order_inj = quant.d_order_inj;
  a.partial = quant.d_partial;
  a.prefix = quant.d_prefix;
  a.levels = quant.d_levels;
  a.idx = quant.d_idx;
  a.moments = quant.d_out;
  a.mass = quant.d_out + n_segs * per_seg_mom;
  a.n_cols = quant.cols;
  a.n_levels = n_levels;
  const long long q_tiles = cover.tiles, q_segs = cover.segs;
  LaunchScratch ev("gwi_weighted_quantiles");
  GWI_HIP(ev.events(2));
  GWI_HIP(hipEventRecord(ev.e[0], h->stream));
  if (q_tiles) hipLaunchKernelGGL(Q::quant_tile_kernel, dim3((unsigned)q_tiles, (unsigned)a.n_cols), dim3(Q::kBlock), 0, h->stream, a);
  if (q_segs) hipLaunchKernelGGL(Q::quant_merge_kernel, dim3((unsigned)q_segs, (unsigned)a.n_cols), dim3(Q::kBlock), 0, h->stream, a);
  if (q_segs) hipLaunchKernelGGL(Q::quant_select_kernel, dim3((unsigned)q_segs, (unsigned)a.n_cols), dim3(Q::kBlock), 0, h->stream, a);
  GWI_HIP(hipGetLastError());
  GWI_HIP(hipEventRecord(ev.e[1], h->stream));
  GWI_HIP(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  GWI_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  g_quantile_times.ms[kQuantQuery] = ms;
  g_quantile_times.launches = 3;
  const size_t n_ev = (size_t)h->n_ev;
  if (with_pe && n_ev) {
    GWI_HIP(hipMemcpy(idx_pe, quant.d_idx, sizeof(int) * n_ev * per_seg_idx, hipMemcpyDeviceToHost));
    GWI_HIP(hipMemcpy(moments_pe, quant.d_out, sizeof(double) * n_ev * per_seg_mom, hipMemcpyDeviceToHost));
  }
  if (with_inj) {
    GWI_HIP(hipMemcpy(idx_inj, quant.d_idx + n_ev * per_seg_idx, sizeof(int) * per_seg_idx, hipMemcpyDeviceToHost));
    GWI_HIP(hipMemcpy(moments_inj, quant.d_out + n_ev * per_seg_mom, sizeof(double) * per_seg_mom, hipMemcpyDeviceToHost));
  }
  GWI_HIP(hipMemcpy(mass, a.mass, sizeof(double) * n_segs, hipMemcpyDeviceToHost));
  return GWI_OK;
}

void gwi_quantile_times(double* logw_ms, double* add_ms, double* query_ms, int32_t* launches) { g_quantile_times.report(logw_ms, add_ms, query_ms, launches); }

// ---- weighted kernel density estimates of the marginal weights (gwi_kde.h) --------------------------------------------------------
enum { kKdeStats, kKdeEval, kKdeCopy };
static thread_local StageTimes g_kde_times;

// the index of the first value of x[n] that is not finite, or -1
static long long first_not_finite(const double* x, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(std::fabs(x[i]) < __builtin_inf())) return (long long)i;
  return -1;
}

gwi_status gwi_set_kde_columns(gwi_handle h, int32_t n_cols, const double* x_pe, const double* x_inj, const double* bounds) {
  if (!h) return GWI_ERR_INVALID;
  namespace K = gwi::kde;
  gwi_status st = post_preflight(h, "gwi_set_kde_columns", "keep the columns on", "the injection densities need", [&]() -> std::string {
    if (n_cols < 1 || n_cols > K::kMaxCols) return "n_cols = " + std::to_string(n_cols) + " is not in 1 ... " + std::to_string(K::kMaxCols);
    if (!x_pe && !x_inj) return "x_pe and x_inj are both null";
    if (x_pe) {
      const long long at = first_not_finite(x_pe, (size_t)n_cols * (size_t)(h->n_ev * h->n_pe));
      if (at >= 0) return "x_pe: value " + std::to_string(at) + " is not finite";
    }
    if (x_inj) {
      const long long at = first_not_finite(x_inj, (size_t)n_cols * (size_t)h->n_inj);
      if (at >= 0) return "x_inj: value " + std::to_string(at) + " is not finite";
    }
    for (int c = 0; bounds && c < n_cols; ++c) {
      const double lo = bounds[2 * c], hi = bounds[2 * c + 1];
      if (std::isinf(lo) || std::isinf(hi)) return "bounds of column " + std::to_string(c) + ": a bound is finite or NaN (none)";
      if (lo == lo && hi == hi && !(lo < hi)) return "bounds of column " + std::to_string(c) + ": lo is not below hi";
    }
    return "";
  });
  if (st != GWI_OK) return st;
  gwi::draw::DrawArgs geometry;
  long long n_tiles = 0;
  st = draw_workspace(h, "gwi_set_kde_columns", "tiles", &geometry, &n_tiles);
  if (st != GWI_OK) return st;
  // the previous columns go away first: should an allocation fail, the density entries refuse until they are set again
  PostprocessBuffers::Kde& kde = h->post.kde;
  kde = PostprocessBuffers::Kde();
  const size_t n_pe_vals = x_pe ? (size_t)n_cols * (size_t)(h->n_ev * h->n_pe) : 0, n_inj_vals = x_inj ? (size_t)n_cols * (size_t)h->n_inj : 0;
  if (x_pe) GWI_HIP(kde.d_x_pe.upload(x_pe, n_pe_vals));  // (a set that is given has columns, even where it is empty)
  if (x_inj) GWI_HIP(kde.d_x_inj.upload(x_inj, n_inj_vals));
  double host_bounds[2 * K::kMaxCols];
  for (int i = 0; i < 2 * n_cols; ++i) host_bounds[i] = bounds ? bounds[i] : __builtin_nan("");
  GWI_HIP(kde.d_bounds.reserve(2 * K::kMaxCols));
  GWI_HIP(hipMemcpy(kde.d_bounds, host_bounds, sizeof(double) * 2 * (size_t)n_cols, hipMemcpyHostToDevice));
  const size_t n_segs = (size_t)(h->n_ev + 1);
  GWI_HIP(kde.d_part1.reserve((size_t)n_tiles * (size_t)(K::kHead + n_cols)));
  GWI_HIP(kde.d_seg1.reserve(n_segs * (size_t)(K::kHead + n_cols)));
  GWI_HIP(kde.d_part2.reserve((size_t)n_tiles * (size_t)(n_cols + K::kMaxPairs)));
  kde.cols = n_cols;
  return GWI_OK;
}

// one query of either dimension (d = 1: pairs is null and n_items the columns; d = 2: n_items pairs).  The arguments have passed
// the entry's own checks.
static gwi_status kde_query(gwi_handle h, const char* who, int d, const int32_t* pairs, int n_items, const double* gridx, int n_gx, const double* gridy, int n_gy, int rule,
                            double scale, double* rho_pe, double* rho_inj, double* bw, double* neff, int32_t* degenerate) {
  namespace K = gwi::kde;
  PostprocessBuffers::Kde& kde = h->post.kde;
  const bool with_pe = kde.d_x_pe.ptr != nullptr, with_inj = kde.d_x_inj.ptr != nullptr;
  gwi::draw::DrawArgs geometry;
  long long n_tiles = 0;
  gwi_status st = draw_workspace(h, who, "tiles", &geometry, &n_tiles);  // (as gwi_set_kde_columns found it)
  if (st != GWI_OK) return st;
  st = marginal_state(h);
  if (st != GWI_OK) return st;
  if (h->n_ev + 1 > 65535) return fail(h, GWI_ERR_INVALID, std::string(who) + ": more segments than one launch can index");
  g_kde_times = StageTimes();
  const size_t n_segs = (size_t)(h->n_ev + 1), n_ev = (size_t)h->n_ev, per_bw = d == 1 ? 1 : 3;
  const long long n_points = d == 1 ? n_gx : (long long)n_gx * n_gy, n_blocks = (n_points + K::kBlock - 1) / K::kBlock;
  // a set without columns is left out of the launches
  const QueryCover cover(with_pe, with_inj, h->n_ev, geometry);
  const long long q_tiles = cover.tiles, q_segs = cover.segs;
  // the grid blocks of one evaluation pass: as many as keep the partials within kPartialCap doubles, at least one
  const long long per_block = std::max<long long>(1, q_tiles) * n_items * K::kBlock;
  const long long pass_blocks = std::max<long long>(1, std::min<long long>(n_blocks, K::kPartialCap / per_block));
  const size_t n_gridx = (size_t)n_items * (size_t)n_gx, n_gridy = d == 2 ? (size_t)n_items * (size_t)n_gy : 0;
  GWI_HIP(kde.d_grid.reserve(n_gridx + n_gridy));
  GWI_HIP(kde.d_pairs.reserve(2 * K::kMaxPairs));
  GWI_HIP(kde.d_band.reserve(n_segs * (size_t)n_items * K::kBand));
  GWI_HIP(kde.d_bw.reserve(n_segs * (size_t)n_items * 3));
  GWI_HIP(kde.d_neff.reserve(n_segs));
  GWI_HIP(kde.d_degenerate.reserve(n_segs * (size_t)n_items));
  GWI_HIP(kde.d_partial.reserve((size_t)(per_block * pass_blocks)));
  GWI_HIP(kde.d_rho.reserve(n_segs * (size_t)n_items * (size_t)n_points));
  GWI_HIP(hipMemcpy(kde.d_grid, gridx, sizeof(double) * n_gridx, hipMemcpyHostToDevice));
  if (d == 2) {
    GWI_HIP(hipMemcpy(kde.d_grid + n_gridx, gridy, sizeof(double) * n_gridy, hipMemcpyHostToDevice));
    GWI_HIP(hipMemcpy(kde.d_pairs, pairs, sizeof(int32_t) * 2 * (size_t)n_items, hipMemcpyHostToDevice));
  }
  K::Args a;
  std::memset(&a, 0, sizeof(a));
  fill_query_args(h, geometry, cover, &a);
  a.x_pe = kde.d_x_pe;
  a.x_inj = kde.d_x_inj;
  a.bounds = kde.d_bounds;
  a.pairs = kde.d_pairs;
  a.part1 = kde.d_part1;
  a.seg1 = kde.d_seg1;
  a.part2 = kde.d_part2;
  a.band = kde.d_band;
  a.bw = kde.d_bw;
  a.neff = kde.d_neff;
  a.degenerate = kde.d_degenerate;
  a.gridx = kde.d_grid;
  a.gridy = kde.d_grid + n_gridx;
  a.partial = kde.d_partial;
  a.rho = kde.d_rho;
  a.scale = scale;
  a.n_cols = kde.cols;
  a.n_pairs = d == 2 ? n_items : 0;
  a.n_items = n_items;
  a.rule = rule;
  a.n_gx = n_gx;
  a.n_gy = d == 2 ? n_gy : 1;
  a.n_points = (int)n_points;
  LaunchScratch ev(who);
  GWI_HIP(ev.events(3));
  GWI_HIP(hipEventRecord(ev.e[0], h->stream));
  int launches = (q_tiles ? 2 : 0) + (q_segs ? 1 : 0);
  if (q_tiles) hipLaunchKernelGGL(K::kde_moment_kernel<1>, dim3((unsigned)q_tiles), dim3(K::kBlock), 0, h->stream, a);
  if (q_segs) hipLaunchKernelGGL(K::kde_mean_kernel, dim3((unsigned)q_segs), dim3(64), 0, h->stream, a);
  if (q_tiles) hipLaunchKernelGGL(K::kde_moment_kernel<2>, dim3((unsigned)q_tiles), dim3(K::kBlock), 0, h->stream, a);
  if (q_segs) {
    if (d == 1) hipLaunchKernelGGL(K::kde_band_kernel<1>, dim3((unsigned)q_segs), dim3(64), 0, h->stream, a);
    else hipLaunchKernelGGL(K::kde_band_kernel<2>, dim3((unsigned)q_segs), dim3(64), 0, h->stream, a);
    ++launches;
  }
  GWI_HIP(hipGetLastError());
  GWI_HIP(hipEventRecord(ev.e[1], h->stream));
  for (long long b0 = 0; b0 < n_blocks && q_segs; b0 += pass_blocks) {
    const long long nb = std::min<long long>(pass_blocks, n_blocks - b0);
    a.first_block = (int)b0;
    a.pass_points = (int)(nb * K::kBlock);
    if (q_tiles) {
      if (d == 1) hipLaunchKernelGGL(K::kde_eval_kernel<1>, dim3((unsigned)q_tiles, (unsigned)n_items, (unsigned)nb), dim3(K::kBlock), 0, h->stream, a);
      else hipLaunchKernelGGL(K::kde_eval_kernel<2>, dim3((unsigned)q_tiles, (unsigned)n_items, (unsigned)nb), dim3(K::kBlock), 0, h->stream, a);
      ++launches;
    }
    hipLaunchKernelGGL(K::kde_sum_kernel, dim3((unsigned)nb, (unsigned)n_items, (unsigned)q_segs), dim3(K::kBlock), 0, h->stream, a);
    ++launches;
  }
  GWI_HIP(hipGetLastError());
  GWI_HIP(hipEventRecord(ev.e[2], h->stream));
  GWI_HIP(hipStreamSynchronize(h->stream));
  float stats_ms = 0.f, eval_ms = 0.f;
  GWI_HIP(hipEventElapsedTime(&stats_ms, ev.e[0], ev.e[1]));
  GWI_HIP(hipEventElapsedTime(&eval_ms, ev.e[1], ev.e[2]));
  g_kde_times.ms[kKdeStats] = stats_ms;
  g_kde_times.ms[kKdeEval] = eval_ms;
  g_kde_times.launches = launches;
  // a segment that is left out: no curve, no bandwidth, nothing flagged
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < n_segs * (size_t)n_items * per_bw; ++i) bw[i] = __builtin_nan("");
  for (size_t i = 0; i < n_segs; ++i) neff[i] = 0.0;
  for (size_t i = 0; i < n_segs * (size_t)n_items; ++i) degenerate[i] = 0;
  const size_t s0 = (size_t)a.first_seg, ns = (size_t)q_segs, per_rho = (size_t)n_items * (size_t)n_points;
  if (ns) {
    GWI_HIP(hipMemcpy(bw + s0 * n_items * per_bw, kde.d_bw + s0 * n_items * per_bw, sizeof(double) * ns * n_items * per_bw, hipMemcpyDeviceToHost));
    GWI_HIP(hipMemcpy(neff + s0, kde.d_neff + s0, sizeof(double) * ns, hipMemcpyDeviceToHost));
    GWI_HIP(hipMemcpy(degenerate + s0 * n_items, kde.d_degenerate + s0 * n_items, sizeof(int32_t) * ns * n_items, hipMemcpyDeviceToHost));
  }
  if (with_pe && n_ev) GWI_HIP(hipMemcpy(rho_pe, kde.d_rho, sizeof(double) * n_ev * per_rho, hipMemcpyDeviceToHost));
  if (with_inj) GWI_HIP(hipMemcpy(rho_inj, kde.d_rho + n_ev * per_rho, sizeof(double) * per_rho, hipMemcpyDeviceToHost));
  g_kde_times.ms[kKdeCopy] = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return GWI_OK;
}

// what is wrong with the arguments the two density entries share, or an empty string.  That no columns are set is said after the
// other refusals: a handle that holds a shard cannot set any and is told so
static std::string bad_kde_request(const PostprocessBuffers::Kde& kde, int32_t rule, double scale, const double* rho_pe, const double* rho_inj, const double* bw, const double* neff,
                                   const int32_t* degenerate) {
  if (rule != gwi::kde::kScott && rule != gwi::kde::kSilverman) return "rule = " + std::to_string(rule) + " is neither 0 (Scott) nor 1 (Silverman)";
  if (!(scale > 0.0 && scale < __builtin_inf())) return "scale = " + std::to_string(scale) + " is not a positive finite number";
  if (kde.d_x_pe.ptr && !rho_pe) return "PE columns are set: rho_pe is needed";
  if (kde.d_x_inj.ptr && !rho_inj) return "injection columns are set: rho_inj is needed";
  if (!bw || !neff || !degenerate) return "the bandwidth, neff or degenerate output is null";
  return "";
}

gwi_status gwi_weighted_kde(gwi_handle h, const double* grid, int32_t n_grid, int32_t rule, double scale, double* rho_pe, double* rho_inj, double* bw, double* neff,
                            int32_t* degenerate) {
  if (!h) return GWI_ERR_INVALID;
  namespace K = gwi::kde;
  const PostprocessBuffers::Kde& kde = h->post.kde;
  gwi_status st = post_preflight(h, "gwi_weighted_kde", "evaluate on", "the injection densities need", [&]() -> std::string {
    if (n_grid < 1 || n_grid > K::kMaxGrid) return "n_grid = " + std::to_string(n_grid) + " is not in 1 ... " + std::to_string(K::kMaxGrid);
    const std::string why = bad_kde_request(kde, rule, scale, rho_pe, rho_inj, bw, neff, degenerate);
    if (!why.empty()) return why;
    if (!grid) return "grid is null";
    const long long at = first_not_finite(grid, (size_t)std::max(kde.cols, 1) * (size_t)n_grid);
    if (at >= 0) return "grid: point " + std::to_string(at) + " is not finite";
    return "";
  });
  if (st != GWI_OK) return st;
  if (!kde.cols) return fail(h, GWI_ERR_INVALID, "gwi_weighted_kde: no columns are set (gwi_set_kde_columns)");
  return kde_query(h, "gwi_weighted_kde", 1, nullptr, kde.cols, grid, n_grid, nullptr, 1, rule, scale, rho_pe, rho_inj, bw, neff, degenerate);
}

gwi_status gwi_weighted_kde2d(gwi_handle h, const int32_t* pairs, int32_t n_pairs, const double* gridx, int32_t n_gx, const double* gridy, int32_t n_gy, int32_t rule,
                              double scale, double* rho_pe, double* rho_inj, double* cov, double* neff, int32_t* degenerate) {
  if (!h) return GWI_ERR_INVALID;
  namespace K = gwi::kde;
  const PostprocessBuffers::Kde& kde = h->post.kde;
  gwi_status st = post_preflight(h, "gwi_weighted_kde2d", "evaluate on", "the injection densities need", [&]() -> std::string {
    if (n_pairs < 1 || n_pairs > K::kMaxPairs) return "n_pairs = " + std::to_string(n_pairs) + " is not in 1 ... " + std::to_string(K::kMaxPairs);
    if (n_gx < 1 || n_gx > K::kMaxGrid2 || n_gy < 1 || n_gy > K::kMaxGrid2)
      return "n_gx = " + std::to_string(n_gx) + ", n_gy = " + std::to_string(n_gy) + ": not in 1 ... " + std::to_string(K::kMaxGrid2);
    const std::string why = bad_kde_request(kde, rule, scale, rho_pe, rho_inj, cov, neff, degenerate);
    if (!why.empty()) return why;
    if (!pairs || !gridx || !gridy) return "pairs, gridx or gridy is null";
    for (int i = 0; i < 2 * n_pairs; ++i)
      if (kde.cols && (pairs[i] < 0 || pairs[i] >= kde.cols)) return "pair " + std::to_string(i / 2) + " names column " + std::to_string(pairs[i]) + ": not in 0 ... " + std::to_string(kde.cols - 1);
    long long at = first_not_finite(gridx, (size_t)n_pairs * (size_t)n_gx);
    if (at >= 0) return "gridx: point " + std::to_string(at) + " is not finite";
    at = first_not_finite(gridy, (size_t)n_pairs * (size_t)n_gy);
    if (at >= 0) return "gridy: point " + std::to_string(at) + " is not finite";
    return "";
  });
  if (st != GWI_OK) return st;
  if (!kde.cols) return fail(h, GWI_ERR_INVALID, "gwi_weighted_kde2d: no columns are set (gwi_set_kde_columns)");
  return kde_query(h, "gwi_weighted_kde2d", 2, pairs, n_pairs, gridx, n_gx, gridy, n_gy, rule, scale, rho_pe, rho_inj, cov, neff, degenerate);
}

void gwi_kde_times(double* stats_ms, double* eval_ms, double* copy_ms, int32_t* launches) { g_kde_times.report(stats_ms, eval_ms, copy_ms, launches); }

}  // extern "C"

// ---- effective-spin catalogs (gwi_spinprior.h): stand-alone entries, no handle ----------------------------------------------
namespace {
enum { kSpinTotal, kSpinMaxLaunch };
thread_local StageTimes g_spin_times;
}  // namespace

extern "C" {

gwi_status gwi_effective_spins(int64_t n, const double* q, const double* a1, const double* a2, const double* ct1, const double* ct2, double a_max, double* chi_eff,
                               double* chi_p, double* p_chi_eff_iso, double* p_chi_eff_aligned, double* p_chi_p_iso, int32_t device) {
  namespace S = gwi::spinprior;
  if (n < 0 || !(a_max > 0.0) || !(a_max < __builtin_inf())) return GWI_ERR_INVALID;
  if (n > 0 && (!q || !a1 || !a2 || !ct1 || !ct2)) return GWI_ERR_INVALID;
  DeviceScope scope;
  gwi_status st = scope.select(device);
  if (st != GWI_OK) return st;
  g_spin_times = StageTimes();
  if (n == 0) return GWI_OK;
  LaunchScratch sc("gwi_effective_spins");
  if (!sc.open()) return GWI_ERR_HIP;
  const size_t bytes = sizeof(double) * (size_t)n;
  const double* in[5] = {q, a1, a2, ct1, ct2};
  double* out[5] = {chi_eff, chi_p, p_chi_eff_iso, p_chi_eff_aligned, p_chi_p_iso};
  double *d_in[5], *d_out[5];
  for (int c = 0; c < 5; ++c) {
    d_in[c] = sc.alloc<double>((size_t)n);
    d_out[c] = out[c] ? sc.alloc<double>((size_t)n) : nullptr;
    if (!d_in[c] || (out[c] && !d_out[c])) return GWI_ERR_HIP;
    GWI_SCRATCH_HIP(hipMemcpyAsync(d_in[c], in[c], bytes, hipMemcpyHostToDevice, sc.stream));
  }
  const long long blocks = std::min<long long>((n + S::kBlock - 1) / S::kBlock, 2048);
  S::SpinArgs a{d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], d_out[0], d_out[1], d_out[2], d_out[3], d_out[4], a_max, (long long)n, blocks * S::kBlock};
  float ms = 0.f;
  st = sc.timed([&] { hipLaunchKernelGGL(S::effective_spins_kernel, dim3((unsigned)blocks), dim3(S::kBlock), 0, sc.stream, a); },
                [&] {
                  for (int c = 0; c < 5; ++c)
                    if (out[c]) GWI_SCRATCH_HIP(hipMemcpyAsync(out[c], d_out[c], bytes, hipMemcpyDeviceToHost, sc.stream));
                  return GWI_OK;
                },
                &ms);
  if (st != GWI_OK) return st;
  g_spin_times.ms[kSpinTotal] = g_spin_times.ms[kSpinMaxLaunch] = ms;
  g_spin_times.launches = 1;
  return GWI_OK;
}

gwi_status gwi_chi_p_conditional_prior(int64_t n, const double* chi_p, const double* chi_eff, const double* q, double a_max, int32_t n_draws, int32_t max_attempts,
                                       uint64_t seed, int64_t first_index, double* p, int32_t* accepted, int32_t device) {
  namespace S = gwi::spinprior;
  if (n < 0 || n_draws < 2 || max_attempts < 1 || max_attempts > (1 << 16) || first_index < 0 || !(a_max > 0.0) || !(a_max < __builtin_inf())) return GWI_ERR_INVALID;
  if (n > 0 && (!chi_p || !chi_eff || !q || !p || !accepted)) return GWI_ERR_INVALID;
  DeviceScope scope;
  gwi_status st = scope.select(device);
  if (st != GWI_OK) return st;
  g_spin_times = StageTimes();
  if (n == 0) return GWI_OK;
  LaunchScratch sc("gwi_chi_p_conditional_prior");
  if (!sc.open()) return GWI_ERR_HIP;
  const size_t bytes = sizeof(double) * (size_t)n;
  const double* in[3] = {chi_p, chi_eff, q};
  double* d_in[3];
  for (int c = 0; c < 3; ++c) {
    d_in[c] = sc.alloc<double>((size_t)n);
    if (!d_in[c]) return GWI_ERR_HIP;
    GWI_SCRATCH_HIP(hipMemcpyAsync(d_in[c], in[c], bytes, hipMemcpyHostToDevice, sc.stream));
  }
  double* d_p = sc.alloc<double>((size_t)n);
  int* d_acc = sc.alloc<int>((size_t)n);
  if (!d_p || !d_acc) return GWI_ERR_HIP;
  // one workgroup per sample.  A launch is sized by its WORST case, every slot using all its attempts: a slot then costs 50
  // exponentials and, over the two passes, 2 max_attempts pairs of Philox blocks, a pair being about 4 exponentials' worth of
  // instructions -- 50 + 8 max_attempts units.  The budget is 8192 samples of 10^4 draws at the default 64 attempts (4.6e10 units);
  // a typical slot needs two or three attempts (some 70 units), so a typical launch is about an eighth of the worst one, and a larger
  // max_attempts shrinks the launch in proportion, down to one sample
  const double slot_units = 50.0 + 8.0 * (double)max_attempts;
  const long long per_launch = std::max<long long>(1, std::min<long long>(1 << 20, (long long)(4.6e10 / (slot_units * (double)n_draws))));
  for (long long base = 0; base < n; base += per_launch) {
    const long long m = std::min<long long>(per_launch, n - base);
    S::CondArgs a{d_in[0] + base, d_in[1] + base, d_in[2] + base, d_p + base, d_acc + base, a_max, (unsigned long long)seed, (long long)first_index + base, n_draws, max_attempts};
    float ms = 0.f;
    st = sc.timed([&] { hipLaunchKernelGGL(S::chi_p_conditional_kernel, dim3((unsigned)m), dim3(S::kBlock), 0, sc.stream, a); }, &ms);
    if (st != GWI_OK) return st;
    g_spin_times.ms[kSpinTotal] += ms;
    g_spin_times.ms[kSpinMaxLaunch] = std::max<double>(g_spin_times.ms[kSpinMaxLaunch], ms);
    ++g_spin_times.launches;
  }
  GWI_SCRATCH_HIP(hipMemcpyAsync(p, d_p, bytes, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(accepted, d_acc, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipStreamSynchronize(sc.stream));
  return GWI_OK;
}

void gwi_spin_prior_times(double* total_ms, double* max_launch_ms, int32_t* launches) { g_spin_times.report(total_ms, max_launch_ms, nullptr, launches); }

}  // extern "C"

// ---- population draws (gwi_popdraw.h): a stand-alone entry, no handle -------------------------------------------------------
namespace {

enum { kPopdrawCdf, kPopdrawDraw };
thread_local StageTimes g_popdraw_times;
thread_local ErrorSlot g_popdraw_error;

constexpr long long kPopdrawDrawsPerLaunch = 1ll << 20;    // per table
constexpr long long kPopdrawThreadsPerLaunch = 1ll << 26;  // over the tables of a launch

}  // namespace

extern "C" {

gwi_status gwi_table_draws(int32_t device, int32_t n_tables, int32_t n_grid, const double* lo, const double* hi, const double* pdf, int64_t n_draws, uint64_t seed,
                           uint64_t first_index, const double* lower, double* x, double* mass, unsigned char* accept) {
  namespace P = gwi::popdraw;
  ErrorSlot& err = g_popdraw_error;
  err.text.clear();
  g_popdraw_times = StageTimes();
  // ---- the argument checks: on the host, before anything is uploaded
  if (n_tables < 0 || n_draws < 0) return err.refuse("negative n_tables or n_draws");
  if (n_grid < 2) return err.refuse("table 0: n_grid = " + std::to_string(n_grid) + " < 2 (a table has at least one cell)");
  if (n_grid > P::kMaxGrid) return err.refuse("table 0: n_grid = " + std::to_string(n_grid) + " > " + std::to_string(P::kMaxGrid) + " (a table is staged in LDS)");
  if (n_tables > 0 && (!lo || !hi || !pdf)) return err.refuse("null lo, hi or pdf");
  if (n_tables > 0 && n_draws > 0 && !x) return err.refuse("null x");
  for (int32_t t = 0; t < n_tables; ++t) {
    const double width = hi[t] - lo[t];
    if (!(hi[t] > lo[t]) || !(width < __builtin_inf())) return err.refuse("table " + std::to_string(t) + ": hi <= lo (or a bound that is not finite)");
    const double* p = pdf + (size_t)t * (size_t)n_grid;
    for (int32_t i = 0; i < n_grid; ++i)
      if (!(p[i] >= 0.0) || !(p[i] < __builtin_inf())) return err.refuse("table " + std::to_string(t) + ": density entry " + std::to_string(i) + " is negative or not finite");
    const double dx = width / (double)(n_grid - 1);
    bool live = false;
    for (int32_t i = 0; i + 1 < n_grid && !live; ++i) live = 0.5 * (p[i] + p[i + 1]) * dx > 0.0;  // the kernel's cell mass
    if (!live) return err.refuse("table " + std::to_string(t) + ": the total mass is 0");
  }
  DeviceScope scope;
  gwi_status st = scope.select(device);
  if (st != GWI_OK) return st;
  if (n_tables == 0 || n_draws == 0) return GWI_OK;
  LaunchScratch sc("gwi_table_draws");
  if (!sc.open()) return GWI_ERR_HIP;
  const size_t n_cell = (size_t)n_grid - 1;
  double* d_pdf = sc.alloc<double>((size_t)n_tables * (size_t)n_grid);
  double* d_lo = sc.alloc<double>((size_t)n_tables);
  double* d_hi = sc.alloc<double>((size_t)n_tables);
  double* d_prefix = sc.alloc<double>((size_t)n_tables * n_cell);
  int* d_last = sc.alloc<int>((size_t)n_tables);
  if (!d_pdf || !d_lo || !d_hi || !d_prefix || !d_last) return GWI_ERR_HIP;
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_pdf, pdf, sizeof(double) * (size_t)n_tables * (size_t)n_grid, hipMemcpyHostToDevice, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_lo, lo, sizeof(double) * (size_t)n_tables, hipMemcpyHostToDevice, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_hi, hi, sizeof(double) * (size_t)n_tables, hipMemcpyHostToDevice, sc.stream));
  float ms = 0.f;
  {
    P::CdfArgs a{d_pdf, d_lo, d_hi, d_prefix, d_last, n_grid};
    st = sc.timed([&] { hipLaunchKernelGGL(P::table_cdf_kernel, dim3((unsigned)n_tables), dim3(P::kBlock), 0, sc.stream, a); }, &ms);
    if (st != GWI_OK) return st;
    g_popdraw_times.ms[kPopdrawCdf] = ms;
  }
  // the draws, cut into launches of at most 2^20 draws per table and 2^26 lanes: a draw depends on (seed, table, first_index + j)
  // only, so the cut changes nothing
  const LaunchCut cut = launch_cut(n_tables, n_draws, kPopdrawDrawsPerLaunch, kPopdrawThreadsPerLaunch, P::kBlock);
  const long long dc_max = cut.items_max, tc_max = cut.rows_max;
  const size_t chunk = (size_t)dc_max * (size_t)tc_max;
  double* d_lower = lower ? sc.alloc<double>(chunk) : nullptr;
  double* d_x = sc.alloc<double>(chunk);
  double* d_mass = mass ? sc.alloc<double>(chunk) : nullptr;
  unsigned char* d_acc = accept ? sc.alloc<unsigned char>(chunk) : nullptr;
  if (!d_x || (lower && !d_lower) || (mass && !d_mass) || (accept && !d_acc)) return GWI_ERR_HIP;
  const size_t lds_bytes = sizeof(double) * (2 * n_cell + 1);
  const size_t host_pitch = sizeof(double) * (size_t)n_draws, dev_pitch = sizeof(double) * (size_t)dc_max;
  for (long long t0 = 0; t0 < n_tables; t0 += tc_max) {
    const long long tc = std::min<long long>(tc_max, n_tables - t0);
    for (long long j0 = 0; j0 < n_draws; j0 += dc_max) {
      const long long dc = std::min<long long>(dc_max, n_draws - j0);
      const size_t host_at = (size_t)t0 * (size_t)n_draws + (size_t)j0;
      if (lower)
        GWI_SCRATCH_HIP(hipMemcpy2DAsync(d_lower, dev_pitch, lower + host_at, host_pitch, sizeof(double) * (size_t)dc, (size_t)tc, hipMemcpyHostToDevice, sc.stream));
      P::DrawArgs a{d_pdf, d_lo, d_hi, d_prefix, d_last, d_lower, d_x, d_mass, d_acc, (unsigned long long)seed, (unsigned long long)first_index + (unsigned long long)j0,
                    dc,    dc_max, n_grid, (int)t0};
      st = sc.timed([&] { hipLaunchKernelGGL(P::table_draw_kernel, dim3((unsigned)((dc + P::kBlock - 1) / P::kBlock), (unsigned)tc), dim3(P::kBlock), lds_bytes, sc.stream, a); },
                    [&] {  // (once the stream has been waited for, the launch's buffers are free again)
                      GWI_SCRATCH_HIP(hipMemcpy2DAsync(x + host_at, host_pitch, d_x, dev_pitch, sizeof(double) * (size_t)dc, (size_t)tc, hipMemcpyDeviceToHost, sc.stream));
                      if (mass) GWI_SCRATCH_HIP(hipMemcpy2DAsync(mass + host_at, host_pitch, d_mass, dev_pitch, sizeof(double) * (size_t)dc, (size_t)tc, hipMemcpyDeviceToHost, sc.stream));
                      if (accept) GWI_SCRATCH_HIP(hipMemcpy2DAsync(accept + host_at, (size_t)n_draws, d_acc, (size_t)dc_max, (size_t)dc, (size_t)tc, hipMemcpyDeviceToHost, sc.stream));
                      return GWI_OK;
                    },
                    &ms);
      if (st != GWI_OK) return st;
      g_popdraw_times.ms[kPopdrawDraw] += ms;
      ++g_popdraw_times.launches;
    }
  }
  return GWI_OK;
}

const char* gwi_table_draws_error(void) { return g_popdraw_error.text.c_str(); }

void gwi_table_draws_times(double* cdf_ms, double* draw_ms, int32_t* launches) { g_popdraw_times.report(cdf_ms, draw_ms, nullptr, launches); }

}  // extern "C"

// ---- mock catalogs (gwi_mock.h): stand-alone entries, no handle -------------------------------------------------------------
namespace {

enum { kMockObserve, kMockPosterior };
thread_local StageTimes g_mock_times;
thread_local ErrorSlot g_mock_error;

constexpr long long kMockLanesPerLaunch = 1ll << 20;

// the observation model, checked and put into the kernels' form; *why is set when it is refused
bool mock_model(int32_t n_coords, const int32_t* is_log, const double* sigma, const double* lo, const double* hi, gwi::mock::Model* m, std::string* why) {
  if (n_coords < 1 || n_coords > gwi::mock::kMaxCoords) {
    *why = "n_coords = " + std::to_string(n_coords) + " outside 1 ... " + std::to_string(gwi::mock::kMaxCoords);
    return false;
  }
  if (!is_log || !sigma || !lo || !hi) {
    *why = "null is_log, sigma, lo or hi";
    return false;
  }
  *m = gwi::mock::Model();
  m->n_coords = n_coords;
  m->i_m1 = m->i_q = m->i_z = -1;
  for (int32_t c = 0; c < n_coords; ++c) {
    const std::string who = "coordinate " + std::to_string(c) + ": ";
    if (!(sigma[c] > 0.0) || !(sigma[c] < __builtin_inf())) {
      *why = who + "sigma <= 0 or not finite";
      return false;
    }
    if (!(hi[c] > lo[c]) || !(hi[c] - lo[c] < __builtin_inf())) {
      *why = who + "hi <= lo (or a bound that is not finite)";
      return false;
    }
    if (is_log[c] && !(lo[c] > 0.0)) {
      *why = who + "a log coordinate needs lo > 0";
      return false;
    }
    m->is_log[c] = is_log[c] ? 1 : 0;
    m->sigma[c] = sigma[c];
    m->lo[c] = lo[c];
    m->hi[c] = hi[c];
    m->t_lo[c] = is_log[c] ? std::log(lo[c]) : lo[c];
    m->t_hi[c] = is_log[c] ? std::log(hi[c]) : hi[c];
    m->width[c] = is_log[c] ? std::log(hi[c] / lo[c]) : hi[c] - lo[c];
  }
  return true;
}
}  // namespace

extern "C" {

gwi_status gwi_mock_observe(int32_t device, int32_t n_coords, const int32_t* is_log, const double* sigma, const double* lo, const double* hi, int32_t i_m1, int32_t i_q,
                            int32_t i_z, const double* detection, int32_t n_table, const double* table_z, const double* table_dl, int64_t n, const double* x_true,
                            uint64_t seed, uint64_t first_index, double* data, double* snr, unsigned char* found) {
  namespace K = gwi::mock;
  ErrorSlot& err = g_mock_error;
  err.text.clear();
  g_mock_times = StageTimes();
  // ---- the argument checks: on the host, before anything is uploaded
  K::Model m;
  std::string why;
  if (!mock_model(n_coords, is_log, sigma, lo, hi, &m, &why)) return err.refuse(why);
  if (n < 0) return err.refuse("negative n");
  const int32_t roles[3] = {i_m1, i_q, i_z};
  for (int r = 0; r < 3; ++r)
    if (roles[r] < 0 || roles[r] >= n_coords) return err.refuse(std::string("role index ") + (r == 0 ? "m1" : r == 1 ? "q" : "z") + " = " + std::to_string(roles[r]) + " out of range");
  if (i_m1 == i_q || i_m1 == i_z || i_q == i_z) return err.refuse("the role indices m1, q, z must differ");
  if (!detection) return err.refuse("null detection parameters");
  for (int k = 0; k < 4; ++k)
    if (!(detection[k] > 0.0) || !(detection[k] < __builtin_inf())) return err.refuse("detection parameter " + std::to_string(k) + " (rho_ref, mc_ref, dl_ref, rho_th) is not positive and finite");
  if (!table_z || !table_dl) return err.refuse("null DL table");
  if (n_table < 2) return err.refuse("the DL table has fewer than two points");
  for (int32_t i = 0; i < n_table; ++i) {
    if (i > 0 && !(table_z[i] > table_z[i - 1])) return err.refuse("the DL table's redshifts are not ascending at entry " + std::to_string(i));
    if (!(table_dl[i] >= 0.0) || !(table_dl[i] < __builtin_inf()) || (i > 0 && !(table_dl[i] > 0.0)))
      return err.refuse("DL table entry " + std::to_string(i) + " is not positive and finite");
  }
  {
    // the largest redshift the data can show: 9 sigma above the support's end (a 53-bit uniform gives |n| < 8.3)
    const double t_top = m.t_hi[i_z] + 9.0 * m.sigma[i_z];
    const double z_top = m.is_log[i_z] ? std::exp(t_top) : t_top;
    if (!(table_z[0] <= 0.0) || !(table_z[n_table - 1] >= z_top))
      return err.refuse("the DL table covers [" + std::to_string(table_z[0]) + ", " + std::to_string(table_z[n_table - 1]) + "], not [0, hi_z + 9 sigma_z = " + std::to_string(z_top) + "]");
  }
  if (n > 0 && (!x_true || !data || !snr || !found)) return err.refuse("null x_true, data, snr or found");
  m.i_m1 = i_m1;
  m.i_q = i_q;
  m.i_z = i_z;
  m.rho_ref = detection[0];
  m.mc_ref = detection[1];
  m.dl_ref = detection[2];
  m.rho_th = detection[3];
  DeviceScope scope;
  gwi_status st = scope.select(device);
  if (st != GWI_OK) return st;
  if (n == 0) return GWI_OK;
  LaunchScratch sc("gwi_mock_observe");
  if (!sc.open()) return GWI_ERR_HIP;
  const size_t cn = (size_t)n_coords * (size_t)n;
  double* d_x = sc.alloc<double>(cn);
  double* d_d = sc.alloc<double>(cn);
  double* d_snr = sc.alloc<double>((size_t)n);
  unsigned char* d_found = sc.alloc<unsigned char>((size_t)n);
  double* d_tz = sc.alloc<double>((size_t)n_table);
  double* d_tv = sc.alloc<double>((size_t)n_table);
  if (!d_x || !d_d || !d_snr || !d_found || !d_tz || !d_tv) return GWI_ERR_HIP;
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_x, x_true, sizeof(double) * cn, hipMemcpyHostToDevice, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_tz, table_z, sizeof(double) * (size_t)n_table, hipMemcpyHostToDevice, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_tv, table_dl, sizeof(double) * (size_t)n_table, hipMemcpyHostToDevice, sc.stream));
  // launches of at most 2^20 lanes: a value depends on (inputs, seed, first_index + j, coordinate) only, so the cut changes nothing
  for (long long j0 = 0; j0 < n; j0 += kMockLanesPerLaunch) {
    const long long nj = std::min<long long>(kMockLanesPerLaunch, n - j0);
    K::ObserveArgs a{m, d_x, d_tz, d_tv, d_d, d_snr, d_found, (unsigned long long)seed, (unsigned long long)first_index + (unsigned long long)j0, nj, (long long)n, j0, n_table};
    float ms = 0.f;
    st = sc.timed([&] { hipLaunchKernelGGL(K::mock_observe_kernel, dim3((unsigned)((nj + K::kBlock - 1) / K::kBlock)), dim3(K::kBlock), 0, sc.stream, a); }, &ms);
    if (st != GWI_OK) return st;
    g_mock_times.ms[kMockObserve] += ms;
    ++g_mock_times.launches;
  }
  GWI_SCRATCH_HIP(hipMemcpyAsync(data, d_d, sizeof(double) * cn, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(snr, d_snr, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(found, d_found, (size_t)n, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipStreamSynchronize(sc.stream));
  return GWI_OK;
}

gwi_status gwi_mock_posteriors(int32_t device, int32_t n_coords, const int32_t* is_log, const double* sigma, const double* lo, const double* hi, int64_t n_ev, int64_t n_pe,
                               const double* data, uint64_t seed, uint64_t first_event, double* x, double* prior) {
  namespace K = gwi::mock;
  ErrorSlot& err = g_mock_error;
  err.text.clear();
  g_mock_times = StageTimes();
  K::Model m;
  std::string why;
  if (!mock_model(n_coords, is_log, sigma, lo, hi, &m, &why)) return err.refuse(why);
  if (n_ev < 0 || n_pe < 0) return err.refuse("negative n_ev or n_pe");
  if (n_pe > 0xffffffffLL) return err.refuse("n_pe does not fit the 32-bit sample word of the counter");
  if (n_ev > 0 && !data) return err.refuse("null data");
  if (n_ev > 0 && n_pe > 0 && (!x || !prior)) return err.refuse("null x or prior");
  DeviceScope scope;
  gwi_status st = scope.select(device);
  if (st != GWI_OK) return st;
  if (n_ev == 0 || n_pe == 0) return GWI_OK;
  LaunchScratch sc("gwi_mock_posteriors");
  if (!sc.open()) return GWI_ERR_HIP;
  const size_t plane = (size_t)n_ev * (size_t)n_pe;
  double* d_d = sc.alloc<double>((size_t)n_coords * (size_t)n_ev);
  double* d_x = sc.alloc<double>((size_t)n_coords * plane);
  double* d_prior = sc.alloc<double>(plane);
  if (!d_d || !d_x || !d_prior) return GWI_ERR_HIP;
  GWI_SCRATCH_HIP(hipMemcpyAsync(d_d, data, sizeof(double) * (size_t)n_coords * (size_t)n_ev, hipMemcpyHostToDevice, sc.stream));
  // launches of at most 2^20 lanes (and 65535 events): a sample depends on (data, seed, first_event + e, s, coordinate) only
  const LaunchCut cut = launch_cut(n_ev, n_pe, kMockLanesPerLaunch, kMockLanesPerLaunch, K::kBlock);
  const long long sc_max = cut.items_max, ec_max = cut.rows_max;
  for (long long e0 = 0; e0 < n_ev; e0 += ec_max) {
    const long long ec = std::min<long long>(ec_max, n_ev - e0);
    for (long long s0 = 0; s0 < n_pe; s0 += sc_max) {
      const long long ns = std::min<long long>(sc_max, n_pe - s0);
      K::PosteriorArgs a{m, d_d, d_x, d_prior, (unsigned long long)seed, (unsigned long long)first_event, (long long)n_ev, (long long)n_pe, e0, s0, ns};
      float ms = 0.f;
      st = sc.timed([&] { hipLaunchKernelGGL(K::mock_posterior_kernel, dim3((unsigned)((ns + K::kBlock - 1) / K::kBlock), (unsigned)ec), dim3(K::kBlock), 0, sc.stream, a); }, &ms);
      if (st != GWI_OK) return st;
      g_mock_times.ms[kMockPosterior] += ms;
      ++g_mock_times.launches;
    }
  }
  GWI_SCRATCH_HIP(hipMemcpyAsync(x, d_x, sizeof(double) * (size_t)n_coords * plane, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipMemcpyAsync(prior, d_prior, sizeof(double) * plane, hipMemcpyDeviceToHost, sc.stream));
  GWI_SCRATCH_HIP(hipStreamSynchronize(sc.stream));
  return GWI_OK;
}

const char* gwi_mock_error(void) { return g_mock_error.text.c_str(); }

void gwi_mock_times(double* observe_ms, double* posterior_ms, int32_t* launches) { g_mock_times.report(observe_ms, posterior_ms, nullptr, launches); }

}  // extern "C"
