// What a player runs behind the policy's heads, for gfx950 (MI355X): the action of a step without neglogp, values or
// buffer writes (rl_games/algos_torch/players.py:60-83 get_action, :117-160 get_masked_action / get_action), and the
// episode accounting of BasePlayer.run (rl_games/common/player.py:242-330) without a host read per step.
//   rlg_play_policy_head       a = mu (deterministic) or mu + exp(logstd) * noise; with bounds
//                              clamp(a, -1, 1) * ((hi - lo) / 2) + ((hi + lo) / 2) - the statements of
//                              rlg_rollout_policy_head's actions_out / env_actions_out, so the same bits
//   rlg_play_categorical_head  per branch the arg-max of the masked logits (torch.argmax's rule) or, with Exp(1) draws,
//                              the sample of rlg_rollout_categorical_head (the row functions of categorical_rows.hpp)
//   rlg_play_post_step         cur_r += reward, cur_n += 1; where done, (cur_r, cur_n, 1) into the block's fp64 sums of
//                              the step's slot, then both zeroed
//   rlg_play_fold              the slots' sums into (reward sum, length sum, games), slot by slot while games <
//                              games_limit: the host loop's "add the step, break once games >= games_num"
// Launch-only, no atomics, every sum in a fixed order: two runs give the same bits.

#include "categorical_rows.hpp"

namespace rlg {

constexpr int kPlayBlock = 256;

struct PlayHeadArgs {
  const float* mu;         // heads + mu_col: [rows, ld]
  const float* logstd;     // [A]
  const float* noise;      // [rows, A] standard normal, or nullptr: deterministic
  const float* act_low;    // [A], or nullptr: no clamp + rescale
  const float* act_high;
  float* actions_out;      // [rows, A] contiguous
  long long ld, total;     // total = rows * A
  int A;
};

// One thread per (row, action), consecutive threads on consecutive output (and noise) addresses.  The means are read
// as runs of A floats at the heads' row stride: every run is contiguous and the runs of a wave lie ld - A floats apart,
// so a wave's 64 loads touch the cache lines of its rows once - no phase walks a row per thread, which is what the
// rollout head stages its tiles in LDS for.
__global__ __launch_bounds__(kPlayBlock) void play_policy_head_kernel(PlayHeadArgs p) {
  const long long idx = static_cast<long long>(blockIdx.x) * kPlayBlock + threadIdx.x;
  if (idx >= p.total) return;
  const long long row = idx / p.A;
  const int a = static_cast<int>(idx - row * p.A);
  float act = p.mu[row * p.ld + a];
  if (p.noise) {
    const float sg = expf(p.logstd[a]);
    act = act + sg * p.noise[idx];
  }
  if (p.act_low) {
    const float lo = p.act_low[a], hi = p.act_high[a];
    const float d = (hi - lo) / 2.0f, m = (hi + lo) / 2.0f;
    act = clamp_nan(act, -1.0f, 1.0f) * d + m;
  }
  p.actions_out[idx] = act;
}

struct PlayCategoricalArgs : CategoricalRows {
  long long* actions_out;   // [N, B] contiguous
};

// Tile form.  lds: [kCatTileRows][ld] masked logits, and with draws | [kCatTileRows][ld] noise | [kCatTileRows][P + 1]
// sum scratch (ld = S | 1, P = next_pow2 of the widest branch).  One thread per (row, branch).
__global__ __launch_bounds__(kCatTileRows) void play_categorical_tile_kernel(PlayCategoricalArgs p) {
  extern __shared__ float play_lds[];
  const int env0 = blockIdx.x * kCatTileRows;
  const int rows = min(kCatTileRows, p.N - env0);
  const int B = p.B, ld = p.S | 1;
  float* const sx = play_lds;
  float* const sq = p.noise ? play_lds + kCatTileRows * ld : nullptr;
  float* const scratch = play_lds + 2 * kCatTileRows * ld + threadIdx.x * (p.pow2 + 1);
  stage_categorical_tile(p, env0, rows, ld, sx, sq);
  __syncthreads();
  for (int i = threadIdx.x; i < rows * B; i += kCatTileRows) {
    const int r = i / B;
    const int b = i - r * B;
    const int o = r * ld + p.off[b];
    float nlp;
    const int a = sq ? categorical_branch(sx + o, sq + o, p.size[b], scratch, &nlp) : argmax_branch(sx + o, p.size[b]);
    p.actions_out[static_cast<long long>(env0 + r) * B + b] = a;
  }
}

// Wave form (rows wider than the tile): one wave per row, the branches in order.
__global__ __launch_bounds__(kCatWaveBlock) void play_categorical_wave_kernel(PlayCategoricalArgs p) {
  const long long env = static_cast<long long>(blockIdx.x) * (kCatWaveBlock / kWave) + wave_id();
  if (env >= p.N) return;
  const int lane = lane_id();
  for (int b = 0; b < p.B; ++b) {
    float norm;
    const int a = p.noise ? categorical_branch_wave(p, env, b, lane, &norm) : argmax_branch_wave(p, env, b, lane);
    if (lane == 0) p.actions_out[env * p.B + b] = a;
  }
}

// One thread per row; the block's sums of the finished rows in the order of block_sum (wave tree, waves in order).
__global__ __launch_bounds__(kPlayBlock) void play_post_step_kernel(const float* __restrict__ rewards, long long ld,
                                                                    const uint8_t* __restrict__ dones,
                                                                    float* __restrict__ cur_r, float* __restrict__ cur_n,
                                                                    double* __restrict__ partials, int rows) {
  __shared__ double scratch[3 * (kPlayBlock / kWave)];
  const int i = blockIdx.x * kPlayBlock + threadIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  if (i < rows) {
    const float r = cur_r[i] + rewards[i * ld];
    const float n = cur_n[i] + 1.0f;
    const bool done = dones[i] != 0;
    if (done) {
      acc[0] = r;
      acc[1] = n;
      acc[2] = 1.0;
    }
    cur_r[i] = done ? 0.0f : r;
    cur_n[i] = done ? 0.0f : n;
  }
  block_sum<3, kPlayBlock>(acc, scratch);
  if (threadIdx.x == 0) {
    double* out = partials + static_cast<long long>(blockIdx.x) * 3;
    out[0] = acc[0];
    out[1] = acc[1];
    out[2] = acc[2];
  }
}

// One workgroup.  Per slot, in order: thread t adds the slot's blocks t, t + 256, ... in ascending order, block_sum
// joins the threads, thread 0 adds the slot to the totals - so the totals do not depend on how the slots are spread over
// calls.  A slot is folded only while games < games_limit at its start.
__global__ __launch_bounds__(kPlayBlock) void play_fold_kernel(const double* __restrict__ partials, int slots, int blocks,
                                                               long long games_limit, double* __restrict__ totals) {
  __shared__ double scratch[3 * (kPlayBlock / kWave)];
  __shared__ long long games_now;
  long long* const games = reinterpret_cast<long long*>(totals + 2);
  if (threadIdx.x == 0) games_now = *games;
  __syncthreads();
  for (int s = 0; s < slots; ++s) {
    if (games_now >= games_limit) return;        // (the same value in every thread)
    double acc[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < blocks; b += kPlayBlock) {
      const double* p = partials + (static_cast<long long>(s) * blocks + b) * 3;
      acc[0] += p[0];
      acc[1] += p[1];
      acc[2] += p[2];
    }
    __syncthreads();                             // everyone has read games_now; scratch is free again
    block_sum<3, kPlayBlock>(acc, scratch);
    if (threadIdx.x == 0) {
      totals[0] += acc[0];
      totals[1] += acc[1];
      games_now += static_cast<long long>(acc[2]);
      *games = games_now;
    }
    __syncthreads();
  }
}

}  // namespace rlg

extern "C" {

int rlg_play_policy_head(const float* heads, int ld_heads, int mu_col, const float* logstd, const float* noise_or_null,
                         const float* act_low_or_null, const float* act_high_or_null, float* actions_out, int rows,
                         int actions_num, void* stream) {
  using namespace rlg;
  if (!heads || !actions_out || (noise_or_null && !logstd) || rows < 0 || actions_num <= 0 || ld_heads < 1 ||
      mu_col < 0 || static_cast<long long>(mu_col) + actions_num > ld_heads || (!act_low_or_null != !act_high_or_null))
    return static_cast<int>(hipErrorInvalidValue);
  if (rows == 0) return 0;
  PlayHeadArgs p;
  p.mu = heads + mu_col;
  p.logstd = logstd;
  p.noise = noise_or_null;
  p.act_low = act_low_or_null;
  p.act_high = act_high_or_null;
  p.actions_out = actions_out;
  p.ld = ld_heads;
  p.total = static_cast<long long>(rows) * actions_num;
  p.A = actions_num;
  const long long grid = (p.total + kPlayBlock - 1) / kPlayBlock;
  if (grid > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(play_policy_head_kernel, dim3(static_cast<unsigned>(grid)), dim3(kPlayBlock), 0,
                     static_cast<hipStream_t>(stream), p);
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_play_categorical_head(const float* logits, int ld_logits, const int* branch_sizes, int num_branches,
                              const float* exp_noise_or_null, const uint8_t* masks_or_null, int ld_masks,
                              int64_t* actions_out, int rows, void* stream) {
  using namespace rlg;
  if (num_branches > kMaxBranches) return static_cast<int>(hipErrorNotSupported);
  if (!logits || !actions_out || rows < 0 || ld_logits < 1 || (masks_or_null && ld_masks < 1))
    return static_cast<int>(hipErrorInvalidValue);
  PlayCategoricalArgs p;
  const int bad = categorical_rows_setup(p, logits, ld_logits, branch_sizes, num_branches, exp_noise_or_null,
                                         masks_or_null, ld_masks, rows);
  if (bad) return bad;
  if (rows == 0) return 0;
  p.actions_out = reinterpret_cast<long long*>(actions_out);
  const int ld = p.S | 1;
  if (ld <= kCatTileMaxStride) {
    const size_t floats = exp_noise_or_null ? static_cast<size_t>(2 * ld + p.pow2 + 1) : static_cast<size_t>(ld);
    hipLaunchKernelGGL(play_categorical_tile_kernel, dim3((rows + kCatTileRows - 1) / kCatTileRows), dim3(kCatTileRows),
                       kCatTileRows * floats * sizeof(float), static_cast<hipStream_t>(stream), p);
  } else {
    constexpr int rows_per_block = kCatWaveBlock / kWave;
    hipLaunchKernelGGL(play_categorical_wave_kernel, dim3((rows + rows_per_block - 1) / rows_per_block),
                       dim3(kCatWaveBlock), 0, static_cast<hipStream_t>(stream), p);
  }
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_play_post_step_num_blocks(int rows) { return rows <= 0 ? 1 : (rows + rlg::kPlayBlock - 1) / rlg::kPlayBlock; }

int rlg_play_post_step(const float* rewards, int ld_rewards, const uint8_t* dones, float* cur_rewards,
                       float* cur_lengths, double* partials_slot, int rows, void* stream) {
  using namespace rlg;
  if (!rewards || !dones || !cur_rewards || !cur_lengths || !partials_slot || rows < 0 || ld_rewards < 1)
    return static_cast<int>(hipErrorInvalidValue);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(play_post_step_kernel, dim3(rlg_play_post_step_num_blocks(rows)), dim3(kPlayBlock), 0,
                     static_cast<hipStream_t>(stream), rewards, static_cast<long long>(ld_rewards), dones, cur_rewards,
                     cur_lengths, partials_slot, rows);
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_play_fold(const double* partials, int slots, int blocks, long long games_limit, double* totals, void* stream) {
  using namespace rlg;
  if (!partials || !totals || slots < 0 || blocks < 1) return static_cast<int>(hipErrorInvalidValue);
  if (slots == 0) return 0;
  hipLaunchKernelGGL(play_fold_kernel, dim3(1), dim3(kPlayBlock), 0, static_cast<hipStream_t>(stream), partials, slots,
                     blocks, games_limit, totals);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
