// Continuous policies with a state-dependent sigma head (`fixed_sigma: False`) and every sigma form of the reference
// (`apply_sigma_parametrization`, rl_games/algos_torch/models.py:272-301): the clipped-PPO loss with its complete
// analytic backward, and the rollout's policy head, gfx950.
//
// The fixed-sigma kernels (ppo_loss_tile.hpp, experience.hip) carry log sigma as a parameter vector [A] and know
// sigma = exp(log sigma) only; here sigma is a function of each row's raw head output, so that
//   * sigma, log sigma and d sigma / d raw come from ONE device function, sigma_of(), shared by both kernels;
//   * the loss kernel emits d loss / d raw sigma per element next to d mu and d value - INCLUDING the entropy term
//     (d entropy / d raw = (d sigma / d raw) / sigma differs per element; the fixed-sigma kernels leave that term, a
//     constant per column, to the finalise launch) - and the finalise launch runs with actions_num = 0, as for the
//     discrete loss: there is no parameter vector whose gradient it would have to fold.
//
// Work split (both kernels): a QUAD of lanes per row, lane q owning the columns a = q, q + 4, ...; the four lanes read
// 16 consecutive bytes of each of the row's arrays, a wave 16 consecutive rows.  Up to 4 * kK columns stay in registers
// from the loads to the stores (kK = 2 for A <= 8, 8 for A <= 32); wider rows stream: the second pass re-reads mu, raw
// sigma and the actions, which are then in L2.  A row's sums over its A columns are formed by quad-permute DPP moves:
// every lane of the quad receives the terms of columns 4 k + 0 .. 4 k + 3 in turn and adds them in that order, so each
// of the four lanes holds the row's sums, added LEFT TO RIGHT in fp32 (the numeric contract of include/rlg_hip.h) - no
// LDS, no barrier, no cross-lane tree whose grouping would depend on A.  The row-level maths (ppo_loss_row of
// ppo_loss_tile.hpp: surrogate, critic, the weights) runs redundantly in the four lanes, which also load the row's six
// scalars four times (one 16-byte-wide request per quad: the same cache line) - a choice: every lane needs the row's g
// and w for its own columns' gradients, and computing them in place costs ~40 VALU ops against a second round of DPP
// broadcasts behind a dependent branch; the kernel waits on memory either way.  Loss kernel: one workgroup of
// 1,024 threads per 256 rows; its seven block sums go in fp64 through LDS in a fixed order (block_sum), no atomics, into
// the [blocks][kLossScalars] partials that rlg_ppo_loss_finalize folds.

#include "ppo_loss_tile.hpp"

namespace rlg {

constexpr int kSigmaExp = 0, kSigmaSoftplus = 1, kSigmaLinear = 2;     // rlg_sigma_kind of the header
constexpr int kSigmaLossRows = 256;                                     // rows per workgroup of the loss kernel
constexpr int kSigmaLossThreads = 4 * kSigmaLossRows;
constexpr int kSigmaHeadRows = 64;                                      // ... of the rollout head: one wave per 16 rows
constexpr int kSigmaHeadThreads = 4 * kSigmaHeadRows;

struct SigmaForm {
  int kind, has_bounds;
  float lo, hi, min_sigma;
};

struct Sigma {
  float sigma, logstd, dsigma;     // sigma, log sigma as the reference's neglogp uses it, d sigma / d raw
};

// torch.nn.functional.softplus (beta 1, threshold 20) and its derivative as softplus_backward forms it: z / (z + 1), z = e^x.
__device__ __forceinline__ float softplus_f(float x, float& d) {
  if (x > 20.0f) {
    d = 1.0f;
    return x;
  }
  const float e = expf(x);
  d = e / (e + 1.0f);
  return log1pf(e);
}

// ActorCriticNetwork.sigma_and_logstd (policy.py; models.py:272-301), statement for statement, one rounding per op.
__device__ __forceinline__ Sigma sigma_of(float raw, const SigmaForm& f) {
  Sigma s;
  if (f.kind == kSigmaSoftplus) {
    s.sigma = softplus_f(raw, s.dsigma) + f.min_sigma;
    s.logstd = logf(s.sigma);
  } else if (f.kind == kSigmaLinear) {                      // sigma ~ raw above a smooth floor
    const float floor = fmaxf(f.min_sigma, 1e-3f);
    s.sigma = floor + softplus_f(raw - floor, s.dsigma);
    s.logstd = logf(s.sigma);
  } else {
    float l = raw, inside = 1.0f;
    if (f.has_bounds) {                                     // torch.clamp: the gradient passes AT the bounds
      l = clamp_nan(raw, f.lo, f.hi);
      inside = (raw >= f.lo && raw <= f.hi) ? 1.0f : 0.0f;
    }
    const float e = expf(l);
    s.sigma = e;
    s.logstd = l;
    s.dsigma = e * inside;
    if (f.min_sigma > 0.0f) {
      s.sigma = e + f.min_sigma;
      s.logstd = logf(s.sigma);
    }
  }
  return s;
}

// Lane J of every quad, to all four of its lanes.
template <int J>
__device__ __forceinline__ float quad_bcast(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), J | (J << 2) | (J << 4) | (J << 6), 0xf, 0xf, true));
}

// sum += the quad's four terms of columns a0 .. a0 + 3 that exist, in that order.  Every lane of the wave must be here.
__device__ __forceinline__ void quad_add(float& sum, float term, int a0, int A) {
  const float t0 = quad_bcast<0>(term), t1 = quad_bcast<1>(term), t2 = quad_bcast<2>(term), t3 = quad_bcast<3>(term);
  sum += t0;
  if (a0 + 1 < A) sum += t1;
  if (a0 + 2 < A) sum += t2;
  if (a0 + 3 < A) sum += t3;
}

// `base` is the fixed-sigma kernels' argument, embedded so that ppo_loss_row (ppo_loss_tile.hpp) runs on it unchanged.
// Live here: mu, values, actions, old_neglogp, advantages, old_values, returns, old_mu, old_sigma, mask, mask_sum, d_mu,
// d_values, mb, A, e_clip, critic_coef, bounds_coef, clip_value, smooth, bound_kind, write_back - and partials, which
// holds [blocks][kLossScalars] rows here (no column sums behind the scalars: ChainNet sums the head biases itself).
// Dead: logstd (nullptr) and the four int strides ld_mu / ld_val / ld_dmu / ld_dval - the strides of this kernel are
// the 64-bit ones below, as in the descriptor.
struct SigmaLossArgs {
  LossArgs base;
  SigmaForm form;
  const float* raw_sigma;        // [rows, A], row stride ld_raw
  float* d_raw_sigma;            // [rows, A], row stride ld_draw
  float* new_neglogp;            // [rows] or nullptr
  long long ld_mu, ld_raw, ld_val, ld_dmu, ld_draw, ld_dval;
  float entropy_coef;
};

struct SigmaLossElem {
  float mu, raw, x, omu, osg;
};

__device__ __forceinline__ SigmaLossElem sigma_loss_load(const SigmaLossArgs& p, long long i, int a, bool ok, bool old) {
  SigmaLossElem e{0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  if (ok) {
    e.mu = p.base.mu[i * p.ld_mu + a];
    e.raw = p.raw_sigma[i * p.ld_raw + a];
    e.x = p.base.actions[i * p.base.A + a];
    if (old) {
      e.omu = p.base.old_mu[i * p.base.A + a];
      e.osg = p.base.old_sigma[i * p.base.A + a];
    }
  }
  return e;
}

struct SigmaRowSums {
  float z2 = 0.0f, kl = 0.0f, b = 0.0f, ls = 0.0f, ent = 0.0f;
};

// The terms of one element of the row's five sums, added into the quad's running sums (columns a0 .. a0 + 3).
__device__ __forceinline__ void sigma_loss_terms(const SigmaLossArgs& p, const SigmaLossElem& e, bool ok, int a0,
                                                 SigmaRowSums& s) {
  float t_z2 = 0.0f, t_kl = 0.0f, t_b = 0.0f, t_ls = 0.0f, t_ent = 0.0f;
  if (ok) {
    const Sigma sg = sigma_of(e.raw, p.form);
    const float z = (e.x - e.mu) / sg.sigma;                                  // models.py:362
    t_z2 = z * z;
    t_ls = sg.logstd;
    t_ent = 1.4189385332046727f + logf(sg.sigma);                            // Normal.entropy()
    // policy_kl(p0 = new, p1 = old)                                          torch_ext.py:28-31
    const float c1 = logf(e.osg / sg.sigma + 1e-5f);
    const float dm = e.omu - e.mu;
    const float c2 = (sg.sigma * sg.sigma + dm * dm) / (2.0f * (e.osg * e.osg + 1e-5f));
    t_kl = (c1 + c2) + (-0.5f);
    if (p.base.bound_kind == 1) {                                             // a2c_continuous.py:248-253
      const float hi_t = clamp_min_nan(e.mu - 1.1f, 0.0f);
      const float lo_t = clamp_max_nan(e.mu + 1.1f, 0.0f);
      t_b = lo_t * lo_t + hi_t * hi_t;
    } else if (p.base.bound_kind == 2) {                                      // :241-246
      t_b = e.mu * e.mu;
    }
  }
  const int A = p.base.A;
  quad_add(s.z2, t_z2, a0, A);
  quad_add(s.kl, t_kl, a0, A);
  quad_add(s.b, t_b, a0, A);
  quad_add(s.ls, t_ls, a0, A);
  quad_add(s.ent, t_ent, a0, A);
}

// d loss / d mu and d loss / d raw sigma of one element, and the write-back of the step's policy (datasets.py:33-43).
//   d nlp / d mu = -z / sigma;  d nlp / d raw = (1 - z^2) s'/sigma;  d entropy / d raw = s'/sigma   (s' = d sigma / d raw)
__device__ __forceinline__ void sigma_loss_grads(const SigmaLossArgs& p, const SigmaLossElem& e, long long i, int a,
                                                 const LossRow& R) {
  const Sigma sg = sigma_of(e.raw, p.form);
  const float z = (e.x - e.mu) / sg.sigma;
  float db = 0.0f;
  if (p.base.bound_kind == 1) {
    db = 2.0f * fminf(e.mu + 1.1f, 0.0f) + 2.0f * fmaxf(e.mu - 1.1f, 0.0f);
  } else if (p.base.bound_kind == 2) {
    db = 2.0f * e.mu;
  }
  p.base.d_mu[i * p.ld_dmu + a] = R.g * (-(z / sg.sigma)) + (R.w * p.base.bounds_coef) * db;
  p.d_raw_sigma[i * p.ld_draw + a] = (R.g * (1.0f - z * z) - p.entropy_coef * R.w) * (sg.dsigma / sg.sigma);
  if (p.base.write_back) {
    p.base.old_mu[i * p.base.A + a] = e.mu;
    p.base.old_sigma[i * p.base.A + a] = sg.sigma;
  }
}

// kK > 0: A <= 4 * kK, the row's elements held in registers.  kK == 0: any A, streamed twice.
template <int kK>
__global__ __launch_bounds__(kSigmaLossThreads) void ppo_loss_sigma_kernel(SigmaLossArgs p) {
  __shared__ double red[kLossScalars * (kSigmaLossThreads / kWave)];
  const int A = p.base.A;
  const int tid = threadIdx.x;
  const int r = tid >> 2, q = tid & 3;
  const long long row0 = static_cast<long long>(blockIdx.x) * kSigmaLossRows;
  const bool row_ok = row0 + r < p.base.mb;
  const long long i = row_ok ? row0 + r : 0;
  const int rounds = (A + 3) >> 2;

  float r_adv = 0.0f, r_onlp = 0.0f, r_v = 0.0f, r_vo = 0.0f, r_ret = 0.0f, r_mask = 1.0f;
  if (row_ok) {
    r_adv = p.base.advantages[i];
    r_onlp = p.base.old_neglogp[i];
    r_v = p.base.values[i * p.ld_val];
    r_vo = p.base.old_values[i];
    r_ret = p.base.returns[i];
    if (p.base.mask) r_mask = p.base.mask[i];
  }
  float denom_count = static_cast<float>(p.base.mb);
  if (p.base.mask) denom_count = fmaxf(*p.base.mask_sum, 1.0f);              // torch_ext.py:165

  // ---- pass 1: every load of the row up front (kK > 0), the five sums over the columns
  SigmaLossElem held[kK > 0 ? kK : 1];
  SigmaRowSums s;
  if constexpr (kK > 0) {
#pragma unroll
    for (int k = 0; k < kK; ++k) held[k] = sigma_loss_load(p, i, q + 4 * k, row_ok && q + 4 * k < A, true);
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      if (4 * k < A) sigma_loss_terms(p, held[k], row_ok && q + 4 * k < A, 4 * k, s);     // (uniform in the workgroup)
    }
  } else {
    for (int k = 0; k < rounds; ++k) {
      const bool ok = row_ok && q + 4 * k < A;
      sigma_loss_terms(p, sigma_loss_load(p, i, q + 4 * k, ok, true), ok, 4 * k, s);
    }
  }

  // ---- the row: the same bits in the four lanes of its quad; lane 0 owns its outputs
  const float lo = 1.0f - p.base.e_clip, hi = 1.0f + p.base.e_clip;
  double acc[kLossScalars] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double none[kLossScalars];
  const bool owner = row_ok && q == 0;
  const LossRow R = ppo_loss_row(p.base, A, s.z2, s.kl, s.b, s.ls, s.ent, r_adv, r_onlp, r_v, r_vo, r_ret, r_mask, lo, hi,
                                 denom_count, owner ? acc : none);
  if (owner) {
    p.base.d_values[i * p.ld_dval] = R.dv;
    // (the expression of ppo_loss_row, models.py:361-364)
    if (p.new_neglogp) p.new_neglogp[i] = (0.5f * s.z2 + static_cast<float>(0.9189385332046727 * A)) + s.ls;
  }

  // ---- pass 2: the gradients of the lane's elements, the step's mu / sigma over the old ones
  if constexpr (kK > 0) {
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      if (row_ok && q + 4 * k < A) sigma_loss_grads(p, held[k], i, q + 4 * k, R);
    }
  } else {
    for (int k = 0; k < rounds; ++k) {
      const bool ok = row_ok && q + 4 * k < A;
      if (ok) sigma_loss_grads(p, sigma_loss_load(p, i, q + 4 * k, ok, false), i, q + 4 * k, R);
    }
  }

  block_sum<kLossScalars, kSigmaLossThreads>(acc, red);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < kLossScalars; ++k) p.base.partials[static_cast<long long>(blockIdx.x) * kLossScalars + k] = acc[k];
  }
}

// ---------------------------------------------------------------------------------
// Rollout policy head (is_train = False branch of ModelA2CContinuousLogStd.forward, models.py:348-364, denorm_value
// :58-60) for a per-row sigma, fused with the buffer writes of its outputs - rollout_policy_head_kernel (experience.hip)
// with sigma = sigma_of(raw) per element in place of exp(logstd[a]):
//   action = mu + sigma * noise;  neglogp = 0.5 sum z^2 + 0.5 log(2 pi) A + sum log sigma,  z = (action - mu) / sigma
// The argument is the public descriptor under the name the kernel's symbol carries.
// ---------------------------------------------------------------------------------
struct PolicyHeadSigmaArgs : rlg_policy_head_sigma_desc {};

__global__ __launch_bounds__(kSigmaHeadThreads) void rollout_policy_head_sigma_kernel(PolicyHeadSigmaArgs p) {
  const int A = p.A;
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  const long long env = static_cast<long long>(blockIdx.x) * kSigmaHeadRows + r;
  const bool row_ok = env < p.N;
  const long long e = row_ok ? env : 0;
  const SigmaForm form{p.sigma_kind, p.has_bounds, p.sigma_lo, p.sigma_hi, p.min_sigma};
  const long long slot = e * p.H + p.step;
  float s_z2 = 0.0f, s_ls = 0.0f;
  for (int k = 0; 4 * k < A; ++k) {
    const int a = q + 4 * k;
    float t_z2 = 0.0f, t_ls = 0.0f;
    if (row_ok && a < A) {
      const float mu = p.heads[e * p.ld + 1 + a];
      const Sigma sg = sigma_of(p.raw_sigma[e * p.ld_raw_sigma + a], form);
      const float act = mu + sg.sigma * p.noise[e * A + a];
      const float z = (act - mu) / sg.sigma;
      t_z2 = z * z;
      t_ls = sg.logstd;
      const long long o = slot * A + a;
      p.actions_out[e * A + a] = act;
      if (p.env_actions_out) {
        // d = (high - low) / 2, m = (high + low) / 2, clamp(act, -1, 1) * d + m - each op rounded like the
        // reference's separate torch kernels
        const float lo = p.act_low[a], hi = p.act_high[a];
        const float d = (hi - lo) / 2.0f, m = (hi + lo) / 2.0f;
        p.env_actions_out[e * A + a] = clamp_nan(act, -1.0f, 1.0f) * d + m;
      }
      p.buf_actions[o] = act;
      p.buf_mus[o] = mu;
      p.buf_sigmas[o] = sg.sigma;
    }
    quad_add(s_z2, t_z2, 4 * k, A);
    quad_add(s_ls, t_ls, 4 * k, A);
  }
  if (row_ok && q == 0) {
    p.buf_neglogp[slot] = (0.5f * s_z2 + static_cast<float>(0.9189385332046727 * A)) + s_ls;
    float v = p.value[(e / p.value_repeat) * p.ld_value];
    if (p.v_mean) {
      const float m = static_cast<float>(p.v_mean[0]);
      const float d = sqrt_rn(static_cast<float>(p.v_var[0]) + p.eps);
      v = d * clamp_nan(v, -5.0f, 5.0f) + m;
    }
    p.values_out[e] = v;
    p.buf_values[slot] = v;
  }
}

static bool sigma_form_ok(int kind, int has_bounds, float lo, float hi, float min_sigma) {
  if (kind != kSigmaExp && kind != kSigmaSoftplus && kind != kSigmaLinear) return false;
  if (has_bounds && !(lo <= hi)) return false;
  return min_sigma >= 0.0f;
}

}  // namespace rlg

RLG_ABI_SIZE(rlg_ppo_loss_sigma_desc, 248);
RLG_ABI_SIZE(rlg_policy_head_sigma_desc, 208);

extern "C" {

int rlg_ppo_loss_sigma_num_blocks(int rows) { return (rows + rlg::kSigmaLossRows - 1) / rlg::kSigmaLossRows; }

int rlg_ppo_loss_sigma(const rlg_ppo_loss_sigma_desc* desc, void* stream) {
  using namespace rlg;
  if (desc == nullptr) return static_cast<int>(hipErrorInvalidValue);
  const rlg_ppo_loss_sigma_desc& d = *desc;
  if (!d.mu || !d.raw_sigma || !d.values || !d.actions || !d.old_neglogp || !d.advantages || !d.old_values || !d.returns ||
      !d.old_mu || !d.old_sigma || !d.d_mu || !d.d_raw_sigma || !d.d_values || !d.partials)
    return static_cast<int>(hipErrorInvalidValue);
  if (d.rows <= 0 || d.actions_num <= 0 || (d.mask_or_null && !d.mask_sum_or_null))
    return static_cast<int>(hipErrorInvalidValue);
  // the widths rlg_ppo_loss_fused takes: its tile of this many rows fits the LDS
  const int tile_rows = d.rows <= kLossSmallBatch ? kLossRowsSmall : kLossRows;
  if (ppo_loss_lds_bytes(tile_rows, d.actions_num) > 160 * 1024) return static_cast<int>(hipErrorInvalidValue);
  const int A = d.actions_num;
  if (d.ld_mu < A || d.ld_raw_sigma < A || d.ld_d_mu < A || d.ld_d_raw_sigma < A || d.ld_values < 1 || d.ld_d_values < 1)
    return static_cast<int>(hipErrorInvalidValue);
  if (!sigma_form_ok(d.sigma_kind, d.has_bounds, d.sigma_lo, d.sigma_hi, d.min_sigma) || d.use_smooth_clamp < 0 ||
      d.use_smooth_clamp > kSurrogateNone || d.bound_kind < 0 || d.bound_kind > 2)
    return static_cast<int>(hipErrorInvalidValue);
  SigmaLossArgs p{};
  LossArgs& b = p.base;
  b.mu = d.mu;
  b.values = d.values;
  b.actions = d.actions;
  b.old_neglogp = d.old_neglogp;
  b.advantages = d.advantages;
  b.old_values = d.old_values;
  b.returns = d.returns;
  b.old_mu = d.old_mu;
  b.old_sigma = d.old_sigma;
  b.mask = d.mask_or_null;
  b.mask_sum = d.mask_sum_or_null;
  b.d_mu = d.d_mu;
  b.d_values = d.d_values;
  b.partials = d.partials;
  b.mb = d.rows;
  b.A = A;
  b.e_clip = d.e_clip;
  b.critic_coef = d.critic_coef;
  b.bounds_coef = d.bounds_coef;
  b.clip_value = d.clip_value;
  b.smooth = d.use_smooth_clamp;
  b.bound_kind = d.bound_kind;
  b.write_back = d.write_back;
  p.form = SigmaForm{d.sigma_kind, d.has_bounds, d.sigma_lo, d.sigma_hi, d.min_sigma};
  p.raw_sigma = d.raw_sigma;
  p.d_raw_sigma = d.d_raw_sigma;
  p.new_neglogp = d.new_neglogp_or_null;
  p.ld_mu = d.ld_mu;
  p.ld_raw = d.ld_raw_sigma;
  p.ld_val = d.ld_values;
  p.ld_dmu = d.ld_d_mu;
  p.ld_draw = d.ld_d_raw_sigma;
  p.ld_dval = d.ld_d_values;
  p.entropy_coef = d.entropy_coef;
  const dim3 grid(rlg_ppo_loss_sigma_num_blocks(d.rows)), block(kSigmaLossThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A <= 8) {
    hipLaunchKernelGGL(ppo_loss_sigma_kernel<2>, grid, block, 0, s, p);
  } else if (A <= 32) {
    hipLaunchKernelGGL(ppo_loss_sigma_kernel<8>, grid, block, 0, s, p);
  } else {
    hipLaunchKernelGGL(ppo_loss_sigma_kernel<0>, grid, block, 0, s, p);
  }
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_rollout_policy_head_sigma(const rlg_policy_head_sigma_desc* desc, void* stream) {
  if (!desc) return static_cast<int>(hipErrorInvalidValue);
  if (desc->N <= 0) return 0;
  rlg::PolicyHeadSigmaArgs p{*desc};
  if (!p.heads || !p.raw_sigma || !p.noise || !p.actions_out || !p.values_out || !p.buf_actions || !p.buf_mus ||
      !p.buf_sigmas || !p.buf_neglogp || !p.buf_values)
    return static_cast<int>(hipErrorInvalidValue);
  if (p.step < 0 || p.step >= p.H || p.A <= 0 || p.ld < 1 + p.A || p.ld_raw_sigma < p.A || (p.v_mean && !p.v_var))
    return static_cast<int>(hipErrorInvalidValue);
  if (p.env_actions_out && (!p.act_low || !p.act_high)) return static_cast<int>(hipErrorInvalidValue);
  if (!rlg::sigma_form_ok(p.sigma_kind, p.has_bounds, p.sigma_lo, p.sigma_hi, p.min_sigma))
    return static_cast<int>(hipErrorInvalidValue);
  if (!p.value) {                      // column 0 of the heads
    p.value = p.heads;
    p.ld_value = p.ld;
    p.value_repeat = 1;
  } else if (p.ld_value < 1 || p.value_repeat < 1) {
    return static_cast<int>(hipErrorInvalidValue);
  }
  hipLaunchKernelGGL(rlg::rollout_policy_head_sigma_kernel, dim3((p.N + rlg::kSigmaHeadRows - 1) / rlg::kSigmaHeadRows),
                     dim3(rlg::kSigmaHeadThreads), 0, static_cast<hipStream_t>(stream), p);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
