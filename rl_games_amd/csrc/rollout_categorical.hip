// Categorical policy head of a rollout step for gfx950 (MI355X): the is_train = False branch of the discrete models
// (rl_games/algos_torch/models.py:95-125 ModelA2C, :157-206 ModelA2CMultiDiscrete, CategoricalMasked of
// common/extensions/distributions.py:24-47) + denorm_value (models.py:58-60), fused with the update_data writes of the
// step's actions / neglogpacs / values (a2c_common.py:1008-1009).  Per row and branch b of sizes[b] columns:
//   x     = mask ? logit : -1e8                                   (CategoricalMasked; no mask: the logits)
//   norm  = x - (log(sum exp(x - m)) + m),  m = max x (0 if inf)  (Categorical.__init__: logits - logsumexp)
//   p     = exp(norm - max norm) / sum exp(norm - max norm)       (Categorical.probs = softmax(norm))
//   a     = argmax p / q,  q ~ Exp(1) from the caller, lowest index on ties  (multinomial's one-sample path)
//   neglogp = sum over branches, left to right, of -norm[a]
// Every op is one fp32 op rounded on its own (-ffp-contract=off, expf / logf, no fast-math intrinsics), and the two
// exp sums are added in the order of torch's kernels for branches of < 128 actions: norm and p are torch's bits
// there (wider branches: the logsumexp sum in another order, last-bit differences).
//
// Two forms.  Tile form (every row's columns fit the LDS tile): a 64-row workgroup stages its logits (mask applied),
// its noise and its value column in LDS with coalesced loads, then one thread per (row, branch) runs the branch from
// LDS, and one thread per row sums the branches' neglogp.  Wave form (wider rows): one wave per row walks the
// branches in order, each with 64-lane reductions.  The kernel is launch- and latency-bound either way.

#include "categorical_rows.hpp"
#include "rlg_hip.h"

namespace rlg {

// The rows (categorical_rows.hpp) and what the rollout adds to them: the value column and the step's buffer slots.
struct CategoricalHeadArgs : CategoricalRows {
  const float* value;       // [ceil(N / value_repeat), ld_value], column 0: row r reads row r / value_repeat
  const double* v_mean;     // value RunningMeanStd (fp64) or nullptr when normalize_value is off
  const double* v_var;
  long long* actions_out;   // [N, B] contiguous
  float* values_out;        // [N]
  long long* buf_actions;   // env-major [N][H][B]
  float* buf_neglogp;       // [N][H]
  float* buf_values;        // [N][H]
  long long ld_value;
  float eps;
  int H, step;
  int value_repeat;         // rows per value row (a central value network's num_agents; 1: one value per row)
};

__device__ __forceinline__ float denorm_value(const CategoricalHeadArgs& p, float v) {
  if (p.v_mean) {
    const float m = static_cast<float>(p.v_mean[0]);
    const float d = sqrt_rn(static_cast<float>(p.v_var[0]) + p.eps);
    v = d * clamp_nan(v, -5.0f, 5.0f) + m;
  }
  return v;
}

// lds: [kCatTileRows][ld] masked logits | [kCatTileRows][ld] noise | [kCatTileRows][B] neglogp parts |
// [kCatTileRows][P + 1] sum scratch; ld = S | 1 (an odd row stride spreads a column's rows over the banks), P =
// next_pow2 of the widest branch.
__global__ __launch_bounds__(kCatTileRows) void rollout_categorical_tile_kernel(CategoricalHeadArgs p) {
  extern __shared__ float cat_lds[];
  const int env0 = blockIdx.x * kCatTileRows;
  const int rows = min(kCatTileRows, p.N - env0);
  const int B = p.B, ld = p.S | 1;
  float* const sx = cat_lds;
  float* const sq = cat_lds + kCatTileRows * ld;
  float* const snlp = cat_lds + 2 * kCatTileRows * ld;
  float* const scratch = snlp + kCatTileRows * B + threadIdx.x * (p.pow2 + 1);
  const int t = threadIdx.x;
  const float v = t < rows ? p.value[static_cast<long long>((env0 + t) / p.value_repeat) * p.ld_value] : 0.0f;
  stage_categorical_tile(p, env0, rows, ld, sx, sq);
  __syncthreads();
  for (int i = t; i < rows * B; i += kCatTileRows) {
    const int r = i / B;
    const int b = i - r * B;
    const int o = r * ld + p.off[b];
    float nlp;
    const long long a = categorical_branch(sx + o, sq + o, p.size[b], scratch, &nlp);
    snlp[i] = nlp;
    const long long env = env0 + r;
    p.actions_out[env * B + b] = a;
    p.buf_actions[(env * p.H + p.step) * B + b] = a;
  }
  __syncthreads();
  if (t < rows) {
    float nlp = 0.0f;
    for (int b = 0; b < B; ++b) nlp += snlp[t * B + b];
    const long long env = env0 + t;
    const long long slot = env * p.H + p.step;
    const float vd = denorm_value(p, v);
    p.buf_neglogp[slot] = nlp;
    p.values_out[env] = vd;
    p.buf_values[slot] = vd;
  }
}

// One wave per row, the branches in order; each branch's columns lane-strided, reduced across the 64 lanes.
__global__ __launch_bounds__(kCatWaveBlock) void rollout_categorical_wave_kernel(CategoricalHeadArgs p) {
  const long long env = static_cast<long long>(blockIdx.x) * (kCatWaveBlock / kWave) + wave_id();
  if (env >= p.N) return;
  const int lane = lane_id();
  float nlp = 0.0f;
  for (int b = 0; b < p.B; ++b) {
    float best_norm;
    const int a = categorical_branch_wave(p, env, b, lane, &best_norm);
    nlp += -best_norm;
    if (lane == 0) {
      p.actions_out[env * p.B + b] = a;
      p.buf_actions[(env * p.H + p.step) * p.B + b] = a;
    }
  }
  if (lane == 0) {
    const long long slot = env * p.H + p.step;
    const float vd = denorm_value(p, p.value[(env / p.value_repeat) * p.ld_value]);
    p.buf_neglogp[slot] = nlp;
    p.values_out[env] = vd;
    p.buf_values[slot] = vd;
  }
}

// Host: the kernels' argument from the public descriptor - the rows with their branch table (categorical_rows_setup), then
// what the rollout adds; the hipError_t of a bad description.
static int categorical_head_args(CategoricalHeadArgs& p, const rlg_categorical_head_desc& d) {
  const int bad = categorical_rows_setup(p, d.logits, d.ld_logits, d.branch_sizes, d.num_branches, d.exp_noise,
                                         d.masks_or_null, d.ld_masks, d.num_envs);
  if (bad) return bad;
  p.value = d.value;
  p.v_mean = d.v_mean_or_null;
  p.v_var = d.v_var_or_null;
  p.actions_out = reinterpret_cast<long long*>(d.actions_out);
  p.values_out = d.values_out;
  p.buf_actions = reinterpret_cast<long long*>(d.buf_actions);
  p.buf_neglogp = d.buf_neglogp;
  p.buf_values = d.buf_values;
  p.ld_value = d.ld_value;
  p.eps = d.eps;
  p.H = d.horizon;
  p.step = d.step;
  p.value_repeat = d.value_repeat;
  return 0;
}

}  // namespace rlg

extern "C" {

int rlg_rollout_categorical_head(const rlg_categorical_head_desc* desc, void* stream) {
  using namespace rlg;
  if (!desc) return static_cast<int>(hipErrorInvalidValue);
  const rlg_categorical_head_desc& d = *desc;
  const int num_envs = d.num_envs;
  if (num_envs <= 0) return 0;
  if (d.num_branches > kMaxBranches) return static_cast<int>(hipErrorNotSupported);
  if (!d.logits || !d.exp_noise || !d.value || !d.actions_out || !d.values_out || !d.buf_actions || !d.buf_neglogp ||
      !d.buf_values || d.step < 0 || d.step >= d.horizon || (d.v_mean_or_null && !d.v_var_or_null) ||
      d.value_repeat < 1 || d.ld_value < 1)
    return static_cast<int>(hipErrorInvalidValue);
  CategoricalHeadArgs p;
  const int bad = categorical_head_args(p, d);
  if (bad) return bad;
  const int ld = p.S | 1;
  if (ld <= kCatTileMaxStride) {
    const size_t lds = static_cast<size_t>(kCatTileRows) * (2 * ld + p.B + p.pow2 + 1) * sizeof(float);
    hipLaunchKernelGGL(rollout_categorical_tile_kernel, dim3((num_envs + kCatTileRows - 1) / kCatTileRows),
                       dim3(kCatTileRows), lds, static_cast<hipStream_t>(stream), p);
  } else {
    constexpr int rows_per_block = kCatWaveBlock / kWave;
    hipLaunchKernelGGL(rollout_categorical_wave_kernel, dim3((num_envs + rows_per_block - 1) / rows_per_block),
                       dim3(kCatWaveBlock), 0, static_cast<hipStream_t>(stream), p);
  }
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
