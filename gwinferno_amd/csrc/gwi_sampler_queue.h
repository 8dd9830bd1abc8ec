// gwi_sampler_queue.h -- internal seam between gwi_sampler.cpp and gwi_engine.hip (not part of the C ABI).
// gwi_sampler.cpp calls the engine through a fixed set of entry points only (its sanitizer build links it against stand-ins
// for exactly those, tests/native/); the queue of chains on batched evaluations therefore takes the two halves of a batch as
// pointers: gwi_nuts_engine_queue passes gwi_eval_batch_begin / _end, gwi_nuts_engine_queue_sharded (gwi_engine.hip) the
// sharded pair.
#ifndef GWI_SAMPLER_QUEUE_H
#define GWI_SAMPLER_QUEUE_H

#include "gwi_sampler.h"

namespace gwi_detail {
using BatchBeginFn = gwi_status (*)(gwi_handle, const double*, int32_t, const gwi_options*, int32_t, int32_t);
using BatchEndFn = gwi_status (*)(gwi_handle, gwi_summary*, double*, double*, double*, double*, double*);
gwi_status nuts_engine_queue_with(BatchBeginFn begin_fn, BatchEndFn end_fn, const gwi_handle* handles, int32_t n_groups, int32_t slots_per_group, int32_t n_chains,
                                  int32_t n_theta, const gwi_options* lopt, const gwi_param_prior* priors, const gwi_smoothing_penalty* pens, int32_t n_pens,
                                  const double* u0, const gwi_nuts_options* opt, double* samples, double* logp, int32_t* tree_depth, gwi_nuts_result* results);
}  // namespace gwi_detail

#endif  // GWI_SAMPLER_QUEUE_H
