// Pieces of the optimiser step shared by adam_step_kernel (optim.hip) and adam_pack_kernel (adam_pack.hip).  (mlp_dw.hip
// only produces the norm partials these read.)
#pragma once

#include "rlg_device.hpp"
#include "rlg_hip.h"

namespace rlg {

// The kernels' argument: the fields of rlg_adam_desc (include/rlg_hip.h documents each of them) and the guard record.
struct AdamArgs {
  float* params;
  float* grads;
  float* exp_avg;
  float* exp_avg_sq;
  long long n;
  const double* norm_partials;
  int norm_blocks;
  float grad_scale;
  float max_norm;
  double* lr_slots;
  const long long* step_counter;
  double beta1, beta2, eps, weight_decay;
  int schedule_kind;
  const float* kl;
  float kl_scale;
  double kl_threshold, min_lr, max_lr, lr_multiplier;
  float* stats_out;
  const unsigned* skip_flag;
  unsigned* guard;         // range-guard record (csrc/range_guard.hip: [0] tag, 0 = clear, [1] index) or nullptr.  With a
                           // record the launch is skipped as under skip_flag when the record is set or the total gradient
                           // norm is not finite, and block 0 then records (RLG_GUARD_TAG_ADAM, step) in a clear record
#ifdef RLG_ADAM_TRACE
  unsigned long long* trace_rows;   // diagnostic builds only (tools/exp/build_trace_libs.sh): see adam_trace.hpp
  int trace_cap, trace_flags;
#endif
};

// torch.optim.Adam (single-tensor path) scalar prologue, evaluated in double like Python
struct AdamScalars {
  float step_size, bc2_sqrt, w1, b2, w2, eps, wd;
};
__device__ __forceinline__ AdamScalars adam_scalars(const AdamArgs& a, long long step, double lr) {
  AdamScalars k;
  const double bc1 = 1.0 - pow(a.beta1, static_cast<double>(step));
  const double bc2 = 1.0 - pow(a.beta2, static_cast<double>(step));
  k.step_size = static_cast<float>(lr / bc1);
  k.bc2_sqrt = static_cast<float>(sqrt(bc2));
  k.w1 = static_cast<float>(1.0 - a.beta1);
  k.b2 = static_cast<float>(a.beta2);
  k.w2 = static_cast<float>(1.0 - a.beta2);
  k.eps = static_cast<float>(a.eps);
  k.wd = static_cast<float>(a.weight_decay);
  return k;
}
// one parameter: g = (grad * grad_scale) * clip is written back (like clip_grad_norm_), then the Adam update
__device__ __forceinline__ void adam_update(const AdamArgs& a, const AdamScalars& k, long long i, float clip) {
  float g = (a.grads[i] * a.grad_scale) * clip;
  a.grads[i] = g;
  float p = a.params[i];
  if (k.wd != 0.0f) g = g + k.wd * p;                          // grad.add(param, alpha=wd)
  float m = a.exp_avg[i];
  m = m + k.w1 * (g - m);                                      // exp_avg.lerp_(grad, 1-beta1)
  float v = a.exp_avg_sq[i];
  v = v * k.b2 + (k.w2 * g) * g;                               // mul_(beta2).addcmul_(g, g, 1-beta2)
  const float denom = sqrt_rn(v) / k.bc2_sqrt + k.eps;
  p = p - k.step_size * (m / denom);                           // addcdiv_(exp_avg, denom, -step_size)
  a.exp_avg[i] = m;
  a.exp_avg_sq[i] = v;
  a.params[i] = p;
}
// clip_coef = max_norm / (total_norm + 1e-6); clamp(max=1.0)       torch clip_grad_norm_
// torch.clamp propagates NaN while fminf returns its non-NaN operand: a NaN norm (one NaN gradient) is passed on, so that
// every gradient, moment and parameter becomes NaN as in the reference, and stats_out[1] is NaN.  An infinite norm gives
// 0 on both sides (only the infinite gradients turn into NaN).
__device__ __forceinline__ float adam_clip_coef(float max_norm, float total_norm) {
  const float coef = fminf(max_norm / (total_norm + 1e-6f), 1.0f);
  return total_norm != total_norm ? total_norm : coef;
}
// Guarded launches (AdamArgs::guard).  Every workgroup computes the same norm, so all of them take the same decision; the
// record is read in front of the norm and written by block 0 only when the norm trips - a workgroup that already sees
// block 0's word skips, as it would have on the norm.  An infinite norm trips as well: without a record its clip
// coefficient is 0 and only the infinite gradients turn into NaN; a guarded run drops the whole step instead.
__device__ __forceinline__ bool adam_guard_trips(const AdamArgs& a, float total_norm) {
  return a.guard != nullptr && !(fabsf(total_norm) <= 3.4028234663852886e38f);
}
__device__ __forceinline__ void adam_guard_record(const AdamArgs& a, long long step) {
  if (a.guard[0] == 0u) {
    a.guard[1] = static_cast<unsigned>(step);
    __threadfence();
    a.guard[0] = static_cast<unsigned>(RLG_GUARD_TAG_ADAM);
  }
}
// AdaptiveScheduler.update in python-float arithmetic (schedulers.py:27-33) + the statistics row; one thread
__device__ __forceinline__ void adam_finish(const AdamArgs& a, int cur, double lr, bool skip, float total_norm, float clip) {
  double next = lr;
  if (a.schedule_kind == 1 && !skip) {
    const double kl = static_cast<double>(*a.kl * a.kl_scale);
    if (kl > 2.0 * a.kl_threshold) next = fmax(lr / a.lr_multiplier, a.min_lr);
    if (kl < 0.5 * a.kl_threshold) next = fmin(lr * a.lr_multiplier, a.max_lr);
  }
  a.lr_slots[cur ^ 1] = next;
  if (a.stats_out) {
    a.stats_out[0] = total_norm;
    a.stats_out[1] = clip;
    a.stats_out[2] = static_cast<float>(lr);
    a.stats_out[3] = static_cast<float>(next);
  }
}

}  // namespace rlg

#include "adam_trace.hpp"

namespace rlg {

// Host: what every rlg_adam_* entry does with its descriptor - reject what no launch may see, then fill the kernels'
// argument (guard_or_null: AdamArgs::guard).  0 or hipErrorInvalidValue.
inline int adam_args_from_desc(const rlg_adam_desc* d, unsigned* guard_or_null, AdamArgs& a) {
  if (d == nullptr || d->n <= 0 || !d->step_counter) return static_cast<int>(hipErrorInvalidValue);
  if (d->schedule_kind == 1 && !d->kl_or_null) return static_cast<int>(hipErrorInvalidValue);
  // (one thread per group of 4 parameters, 16-byte loads: torch allocations are aligned)
  if ((reinterpret_cast<uintptr_t>(d->params) | reinterpret_cast<uintptr_t>(d->grads) |
       reinterpret_cast<uintptr_t>(d->exp_avg) | reinterpret_cast<uintptr_t>(d->exp_avg_sq)) % 16 != 0)
    return static_cast<int>(hipErrorInvalidValue);
  a.params = d->params;
  a.grads = d->grads;
  a.exp_avg = d->exp_avg;
  a.exp_avg_sq = d->exp_avg_sq;
  a.n = d->n;
  a.norm_partials = d->norm_partials_or_null;
  a.norm_blocks = d->norm_blocks;
  a.grad_scale = d->grad_scale;
  a.max_norm = d->max_norm;
  a.lr_slots = d->lr_slots;
  a.step_counter = d->step_counter;
  a.beta1 = d->beta1;
  a.beta2 = d->beta2;
  a.eps = d->eps;
  a.weight_decay = d->weight_decay;
  a.schedule_kind = d->schedule_kind;
  a.kl = d->kl_or_null;
  a.kl_scale = d->kl_scale;
  a.kl_threshold = d->kl_threshold;
  a.min_lr = d->min_lr;
  a.max_lr = d->max_lr;
  a.lr_multiplier = d->lr_multiplier;
  a.stats_out = d->stats_out_or_null;
  a.skip_flag = d->skip_flag_or_null;
  a.guard = guard_or_null;
  RLG_ADAM_TRACE_FILL(a);
  return 0;
}
// the guarded entries' own condition: a record, and the norm partials it watches (without them it would watch nothing)
inline bool adam_guard_args_ok(const rlg_adam_desc* d, const unsigned* guard_record) {
  return guard_record != nullptr && d != nullptr && d->norm_partials_or_null != nullptr && d->norm_blocks > 0;
}

}  // namespace rlg
