// TEST INFRASTRUCTURE (CPU): a queue of chains whose batched evaluation fails part-way (tests/test_sampler_queue_failure_cpu.py,
// under AddressSanitizer + UndefinedBehaviorSanitizer).  gwi_nuts_engine_queue runs 7 chains over one group of 3 slots; the
// stand-in for gwi_eval_batch_begin fails on its second call, while four chains are still queued and have never run.  The
// sampler must unwind the chains it started, leave the others alone, and return GWI_ERR_HIP.  Stand-ins for exactly the four
// engine symbols gwi_sampler.cpp references; the target is a standard Gaussian.
#include <cstdio>
#include <cstring>
#include <vector>

#include "gwi_sampler.h"

namespace {
int g_begins = 0;
std::vector<double> g_thetas;
int g_k = 0;
constexpr int kDim = 2;
}  // namespace

extern "C" gwi_status gwi_eval_sequence(gwi_handle, const double* thetas, int32_t n, const gwi_options*, double* log_likelihoods, double* grads, int32_t, float*) {
  for (int s = 0; s < n; ++s) {
    double q = 0.0;
    for (int i = 0; i < kDim; ++i) {
      const double x = thetas[(size_t)s * kDim + i];
      q += x * x;
      if (grads) grads[(size_t)s * kDim + i] = -x;
    }
    log_likelihoods[s] = -0.5 * q;
  }
  return GWI_OK;
}

extern "C" gwi_status gwi_pin_thread_to_engine(gwi_handle) { return GWI_ERR_UNSUPPORTED; }

extern "C" gwi_status gwi_eval_batch_begin(gwi_handle, const double* thetas, int32_t k, const gwi_options*, int32_t, int32_t) {
  if (++g_begins == 2) return GWI_ERR_HIP;  // e.g. a peer rank's failure reported through the exchange
  g_thetas.assign(thetas, thetas + (size_t)k * kDim);
  g_k = k;
  return GWI_OK;
}

extern "C" gwi_status gwi_eval_batch_end(gwi_handle h, gwi_summary* summaries, double* grads, double*, double*, double*, double*) {
  std::vector<double> ll(g_k);
  const gwi_status st = gwi_eval_sequence(h, g_thetas.data(), g_k, nullptr, ll.data(), grads, 0, nullptr);
  for (int j = 0; j < g_k; ++j) {
    std::memset(&summaries[j], 0, sizeof(gwi_summary));
    summaries[j].log_likelihood = ll[j];
  }
  return st;
}

int main() {
  const int n_chains = 7, slots = 3;
  int dummy = 0;
  const gwi_handle handles[1] = {reinterpret_cast<gwi_handle>(&dummy)};
  gwi_options lopt;
  std::memset(&lopt, 0, sizeof(lopt));
  gwi_param_prior priors[kDim];
  for (auto& p : priors) {
    std::memset(&p, 0, sizeof(p));
    p.kind = GWI_BIJECT_IDENTITY;
    p.sigma = 0.0;  // flat
  }
  std::vector<double> u0((size_t)n_chains * kDim);
  for (size_t i = 0; i < u0.size(); ++i) u0[i] = 0.1 * (double)(i % 5) - 0.2;
  gwi_nuts_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.n_warmup = 20;
  opt.n_samples = 20;
  opt.max_tree_depth = 4;
  opt.target_accept = 0.8;
  opt.seed = 3;
  std::vector<double> samples((size_t)n_chains * opt.n_samples * kDim);
  const gwi_status st = gwi_nuts_engine_queue(handles, 1, slots, n_chains, kDim, &lopt, priors, nullptr, 0, u0.data(), &opt, samples.data(), nullptr, nullptr, nullptr);
  std::printf("status %d after %d batch begins\n", (int)st, g_begins);
  if (st != GWI_ERR_HIP || g_begins != 2) return 1;
  std::printf("OK\n");
  return 0;
}
