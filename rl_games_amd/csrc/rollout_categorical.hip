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

#include "rlg_device.hpp"

namespace rlg {

constexpr int kMaxBranches = 16;
constexpr int kCatTileRows = 64;        // rows (and threads: one wave) per workgroup of the tile form
constexpr int kCatTileMaxStride = 64;   // the tile form's LDS row stride limit (floats): 2 tiles of 64 x 64 = 32 KiB
constexpr int kCatWaveBlock = 256;      // wave form: 4 rows per workgroup

struct CategoricalHeadArgs {
  const float* logits;      // [N, ld_logits], columns 0 .. S-1
  const float* value;       // [ceil(N / value_repeat), ld_value], column 0: row r reads row r / value_repeat
  const float* noise;       // branch-major blocks: block b = [N, size[b]] contiguous at N * off[b]
  const uint8_t* masks;     // [N, ld_masks] bool, or nullptr
  const double* v_mean;     // value RunningMeanStd (fp64) or nullptr when normalize_value is off
  const double* v_var;
  long long* actions_out;   // [N, B] contiguous
  float* values_out;        // [N]
  long long* buf_actions;   // env-major [N][H][B]
  float* buf_neglogp;       // [N][H]
  float* buf_values;        // [N][H]
  long long ld_logits, ld_value, ld_masks;
  float eps;
  int N, H, step, B, S;
  int value_repeat;         // rows per value row (a central value network's num_agents; 1: one value per row)
  int pow2;                 // next power of two >= the widest branch
  int size[kMaxBranches];
  int off[kMaxBranches];    // first column of each branch
};

__device__ __forceinline__ float denorm_value(const CategoricalHeadArgs& p, float v) {
  if (p.v_mean) {
    const float m = static_cast<float>(p.v_mean[0]);
    const float d = sqrt_rn(static_cast<float>(p.v_var[0]) + p.eps);
    v = d * clamp_nan(v, -5.0f, 5.0f) + m;
  }
  return v;
}

__device__ __forceinline__ float masked_logit(const CategoricalHeadArgs& p, long long row, int col) {
  const float l = p.logits[row * p.ld_logits + col];
  return (p.masks && !p.masks[row * p.ld_masks + col]) ? -1e8f : l;
}

__device__ __forceinline__ int last_pow2(int n) { return 1 << (31 - __builtin_clz(n)); }
__device__ __forceinline__ int next_pow2(int n) { return n == 1 ? 1 : 1 << (32 - __builtin_clz(n - 1)); }

// One branch of one row from LDS: x = the branch's masked logits, q its noise, a = a per-thread scratch of
// next_pow2(n) floats.  Returns the action, *nlp = -norm[a].  The two exp sums are added in the order of torch's
// kernels for rows of < 128 columns, so that norm and p are torch's bits: logsumexp's sum (the reduction kernel on a
// contiguous last dim: lane t of last_pow2(n) lanes holds x[t] + x[t + lanes], then a pairwise tree over adjacent
// lanes) and softmax's sum (the persistent warp softmax: one column per lane of next_pow2(n), a butterfly over
// halves).
__device__ __forceinline__ int categorical_branch(const float* x, const float* q, int n, float* a, float* nlp) {
  float mx = x[0];
  for (int j = 1; j < n; ++j) mx = x[j] > mx ? x[j] : mx;
  const float m = isinf(mx) ? 0.0f : mx;
  const int bw = last_pow2(n);
  for (int t = 0; t < bw; ++t) a[t] = expf(x[t] - m) + (t + bw < n ? expf(x[t + bw] - m) : 0.0f);
  for (int w = 1; w < bw; w <<= 1)
    for (int t = 0; t + w < bw; t += 2 * w) a[t] += a[t + w];
  const float lse = logf(a[0]) + m;
  const float m2 = mx - lse;                     // = max_j (x_j - lse): rounding is monotone
  const int ws = next_pow2(n);
  for (int j = 0; j < ws; ++j) a[j] = j < n ? expf((x[j] - lse) - m2) : 0.0f;
  for (int off = ws >> 1; off > 0; off >>= 1)
    for (int j = 0; j < off; ++j) a[j] += a[j + off];
  const float s2 = a[0];
  int act = 0;
  float best = (expf((x[0] - lse) - m2) / s2) / q[0];
  for (int j = 1; j < n; ++j) {
    const float r = (expf((x[j] - lse) - m2) / s2) / q[j];
    if (r > best) {
      best = r;
      act = j;
    }
  }
  *nlp = -(x[act] - lse);
  return act;
}

// lds: [kCatTileRows][ld] masked logits | [kCatTileRows][ld] noise | [kCatTileRows][B] neglogp parts |
// [kCatTileRows][P + 1] sum scratch; ld = S | 1 (an odd row stride spreads a column's rows over the banks), P =
// next_pow2 of the widest branch.
__global__ __launch_bounds__(kCatTileRows) void rollout_categorical_tile_kernel(CategoricalHeadArgs p) {
  extern __shared__ float cat_lds[];
  const int env0 = blockIdx.x * kCatTileRows;
  const int rows = min(kCatTileRows, p.N - env0);
  const int S = p.S, B = p.B, ld = S | 1;
  float* const sx = cat_lds;
  float* const sq = cat_lds + kCatTileRows * ld;
  float* const snlp = cat_lds + 2 * kCatTileRows * ld;
  float* const scratch = snlp + kCatTileRows * B + threadIdx.x * (p.pow2 + 1);
  const int t = threadIdx.x;
  const float v = t < rows ? p.value[static_cast<long long>((env0 + t) / p.value_repeat) * p.ld_value] : 0.0f;
  for (int i = t; i < rows * S; i += kCatTileRows) {
    const int r = i / S;
    const int c = i - r * S;
    sx[r * ld + c] = masked_logit(p, env0 + r, c);
  }
  for (int b = 0; b < B; ++b) {
    const int n = p.size[b];
    const float* gq = p.noise + static_cast<long long>(p.N) * p.off[b] + static_cast<long long>(env0) * n;
    for (int i = t; i < rows * n; i += kCatTileRows) {
      const int r = i / n;
      sq[r * ld + p.off[b] + (i - r * n)] = gq[i];
    }
  }
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

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float y = __shfl_xor(x, o, kWave);
    x = y > x ? y : x;
  }
  return x;
}

// One wave per row, the branches in order; each branch's columns lane-strided, reduced across the 64 lanes.
__global__ __launch_bounds__(kCatWaveBlock) void rollout_categorical_wave_kernel(CategoricalHeadArgs p) {
  const long long env = static_cast<long long>(blockIdx.x) * (kCatWaveBlock / kWave) + wave_id();
  if (env >= p.N) return;
  const int lane = lane_id();
  float nlp = 0.0f;
  for (int b = 0; b < p.B; ++b) {
    const int n = p.size[b], c0 = p.off[b];
    const float* q = p.noise + static_cast<long long>(p.N) * c0 + env * n;
    float mx = -INFINITY;
    for (int j = lane; j < n; j += kWave) {
      const float x = masked_logit(p, env, c0 + j);
      mx = x > mx ? x : mx;
    }
    mx = wave_max(mx);
    const float m = isinf(mx) ? 0.0f : mx;
    // the sums in torch's order below 128 columns (see categorical_branch): lane t < last_pow2(n) holds
    // x[t] + x[t + lanes], pairwise tree over adjacent lanes ...
    const int bw = min(last_pow2(n), kWave);
    float s = 0.0f;
    if (lane < bw) {
      s = expf(masked_logit(p, env, c0 + lane) - m);
      for (int j = lane + bw; j < n; j += bw) s += expf(masked_logit(p, env, c0 + j) - m);
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) s += __shfl_down(s, o, kWave);
    const float lse = logf(__shfl(s, 0, kWave)) + m;
    const float m2 = mx - lse;
    // ... softmax: lane l < next_pow2(n) holds its columns l, l + 64, ... in turn, butterfly over halves
    const int ws = min(next_pow2(n), kWave);
    float s2 = 0.0f;
    if (lane < ws)
      for (int j = lane; j < n; j += ws) s2 += expf((masked_logit(p, env, c0 + j) - lse) - m2);
    s2 = wave_sum(s2);
    // (ratio, column) of the lane's best column, lowest column on ties; then the same order across lanes
    float best = -INFINITY, best_norm = 0.0f;
    int a = n;
    for (int j = lane; j < n; j += kWave) {
      const float norm = masked_logit(p, env, c0 + j) - lse;
      const float r = (expf(norm - m2) / s2) / q[j];
      if (a == n || r > best) {
        best = r;
        a = j;
        best_norm = norm;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float rb = __shfl_xor(best, o, kWave);
      const int ab = __shfl_xor(a, o, kWave);
      const float nb = __shfl_xor(best_norm, o, kWave);
      if (ab < n && (a == n || rb > best || (rb == best && ab < a))) {
        best = rb;
        a = ab;
        best_norm = nb;
      }
    }
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

}  // namespace rlg

extern "C" {

int rlg_rollout_categorical_head_cv(const float* logits, int ld_logits, const float* value, int ld_value,
                                    int value_repeat, const int* branch_sizes, int num_branches,
                                    const float* exp_noise, const uint8_t* masks_or_null, int ld_masks,
                                    const double* v_mean_or_null, const double* v_var_or_null, float eps,
                                    int64_t* actions_out, float* values_out, int64_t* buf_actions, float* buf_neglogp,
                                    float* buf_values, int num_envs, int horizon, int step, void* stream) {
  using namespace rlg;
  if (num_envs <= 0) return 0;
  if (num_branches > kMaxBranches) return static_cast<int>(hipErrorNotSupported);
  if (num_branches < 1 || !branch_sizes || step < 0 || step >= horizon || (v_mean_or_null && !v_var_or_null) ||
      value_repeat < 1)
    return static_cast<int>(hipErrorInvalidValue);
  CategoricalHeadArgs p;
  p.value_repeat = value_repeat;
  p.B = num_branches;
  p.S = 0;
  for (int b = 0; b < num_branches; ++b) {
    if (branch_sizes[b] < 1) return static_cast<int>(hipErrorInvalidValue);
    p.size[b] = branch_sizes[b];
    p.off[b] = p.S;
    p.S += branch_sizes[b];
  }
  if (ld_logits < p.S || ld_value < 1 || (masks_or_null && ld_masks < p.S)) return static_cast<int>(hipErrorInvalidValue);
  p.logits = logits;
  p.value = value;
  p.noise = exp_noise;
  p.masks = masks_or_null;
  p.v_mean = v_mean_or_null;
  p.v_var = v_var_or_null;
  p.actions_out = reinterpret_cast<long long*>(actions_out);
  p.values_out = values_out;
  p.buf_actions = reinterpret_cast<long long*>(buf_actions);
  p.buf_neglogp = buf_neglogp;
  p.buf_values = buf_values;
  p.ld_logits = ld_logits;
  p.ld_value = ld_value;
  p.ld_masks = ld_masks;
  p.eps = eps;
  p.N = num_envs;
  p.H = horizon;
  p.step = step;
  int widest = 1;
  for (int b = 0; b < num_branches; ++b) widest = branch_sizes[b] > widest ? branch_sizes[b] : widest;
  p.pow2 = 1;
  while (p.pow2 < widest) p.pow2 <<= 1;
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

int rlg_rollout_categorical_head(const float* logits, int ld_logits, const float* value, int ld_value,
                                 const int* branch_sizes, int num_branches, const float* exp_noise,
                                 const uint8_t* masks_or_null, int ld_masks, const double* v_mean_or_null,
                                 const double* v_var_or_null, float eps, int64_t* actions_out, float* values_out,
                                 int64_t* buf_actions, float* buf_neglogp, float* buf_values, int num_envs,
                                 int horizon, int step, void* stream) {
  return rlg_rollout_categorical_head_cv(logits, ld_logits, value, ld_value, 1, branch_sizes, num_branches, exp_noise,
                                         masks_or_null, ld_masks, v_mean_or_null, v_var_or_null, eps, actions_out,
                                         values_out, buf_actions, buf_neglogp, buf_values, num_envs, horizon, step,
                                         stream);
}

}  // extern "C"
