/*
 * rlg_hip.h - C ABI of librlg_hip.so: the MI355X (gfx950) PPO hot path behind the
 * rl_games A2CAgent / torch_runner.Runner API.
 *
 * The reference (Denys88/rl_games v2.0.0) is 100 % Python on PyTorch and has no FFI of
 * its own; every entry point below therefore replaces a *Python* function or method of
 * the reference, cited as `file:line` relative to the reference checkout.  The binding a
 * reference maintainer would add is a ctypes stub; the in-tree host
 * code (the .py files of rl_games_amd/) is that binding.
 *
 * Conventions (all entry points):
 *   - plain device pointers + explicit sizes/strides, scalars by value, no torch types;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - launch only: never allocates, never synchronises, safe inside hipGraph capture;
 *   - returns 0 (hipSuccess) or the hipError_t of the failed launch / hipErrorInvalidValue
 *     for an unsupported shape; the Python binding raises RuntimeError on non-zero;
 *   - fp32 arithmetic is evaluated op by op (library built with -ffp-contract=off) in the
 *     order of the reference's eager PyTorch ops, so integer/mask/index results are
 *     bit-exact and fp32 results agree to rounding of reductions.
 *   - strides are in ELEMENTS, not bytes.
 */
#ifndef RLG_HIP_H_
#define RLG_HIP_H_

#include <stdint.h>

/* sizeof of a descriptor struct is part of the ABI (the ctypes classes of _lib.py mirror the layouts) */
#ifdef __cplusplus
#define RLG_ABI_SIZE(type, bytes) static_assert(sizeof(type) == (bytes), #type ": layout is part of the C ABI")
extern "C" {
#else
#define RLG_ABI_SIZE(type, bytes) _Static_assert(sizeof(type) == (bytes), #type ": layout is part of the C ABI")
#endif

/* ------------------------------------------------------------------------------------
 * GAE backward scan
 *   replaces rl_games/triton_kernels/gae_kernel.py: _gae_kernel :17-60, _pytorch_gae
 *   :63-80, _triton_gae :83-119, compute_gae :125-147; called from
 *   rl_games/common/a2c_common.py: A2CBase.discount_values :729-734.
 * ---------------------------------------------------------------------------------- */

/* General layout: rewards/values/advs [H, N, V] fp32 with arbitrary element strides,
 * dones [H, N] and last_dones [N] either fp32 (dones_are_float=1, what the reference
 * passes after `.float()`, a2c_common.py:1055-1056) or uint8/bool (dones_are_float=0).
 * strides17 (host array of 17 int64): r_t,r_e,r_v, v_t,v_e,v_v, d_t,d_e, lv_e,lv_v,
 * ld_e, a_t,a_e,a_v, q_t,q_e,q_v.  returns_or_null, when non-NULL, additionally
 * receives advs + values (a2c_common.py:1060) with strides q_*. */
int rlg_gae_strided(const float* rewards, const float* values, const void* dones,
                    const float* last_values, const void* last_dones, float* advs,
                    float* returns_or_null, int horizon, int num_envs, int value_size,
                    const long long* strides17, int dones_are_float, float gamma,
                    float gamma_tau, void* stream);

/* Env-major fast path = the ExperienceBuffer's native storage (flat index env*H + t,
 * the order swap_and_flatten01 produces: a2c_common.py:33-40): rewards/values [N, H] fp32
 * contiguous, dones [N, H] uint8 contiguous, value_size 1, 16-byte aligned bases,
 * horizon % 4 == 0 and 4 <= horizon <= 64 (rlg_gae_envmajor_supported). */
int rlg_gae_envmajor_supported(int horizon);

/* Number of wave tiles (= rows of the [*, 6] fp64 moment_partials array). */
int rlg_gae_envmajor_num_partials(int num_envs);

/* One pass: returns = A + v (a2c_common.py:1060), advantages = returns - v
 * (a2c_common.py:1598, both individually rounded) and, if moment_partials != NULL, per
 * tile fp64 {sum adv, sum adv^2, sum v, sum v^2, sum ret, sum ret^2} for the advantage
 * normaliser (a2c_common.py:1634) and value RunningMeanStd (a2c_common.py:1616-1620). */
int rlg_gae_envmajor_fused(const float* rewards, const float* values, const uint8_t* dones,
                           const float* last_values, const uint8_t* last_dones, float* returns,
                           float* advantages, double* moment_partials, int num_envs, int horizon,
                           float gamma, float gamma_tau, void* stream);

/* Profiling hooks used by bench.py (not part of the reference surface): hipEvent handles as
 * void*, and the fused GAE launch with start/stop events attached to that dispatch on the same
 * stream (hipExtLaunchKernelGGL) - elapsed time = the kernel's own duration, as rocprofv3 reports it. */
int rlg_event_create(void** event_out);
int rlg_event_destroy(void* event);
int rlg_event_elapsed_us(void* start, void* stop, float* us_out);   /* synchronises on `stop` */
int rlg_gae_envmajor_fused_timed(const float* rewards, const float* values, const uint8_t* dones,
                                 const float* last_values, const uint8_t* last_dones, float* returns,
                                 float* advantages, double* moment_partials, int num_envs,
                                 int horizon, float gamma, float gamma_tau, void* stream,
                                 void* ev_start, void* ev_stop);

/* Raw A_t only (the compute_gae return value) on the env-major layout. */
int rlg_gae_envmajor_raw(const float* rewards, const float* values, const uint8_t* dones,
                         const float* last_values, const uint8_t* last_dones, float* gae_out,
                         int num_envs, int horizon, float gamma, float gamma_tau, void* stream);

/* ------------------------------------------------------------------------------------
 * Rollout buffer (ExperienceBuffer) writes and per-step glue
 *   replaces rl_games/common/experience.py: ExperienceBuffer.update_data :433-456 and the
 *   per-step part of rl_games/common/a2c_common.py: A2CBase.play_steps :994-1051.
 *   Storage is env-major: field[env][t][row], flat index env*H + t (swap_and_flatten01
 *   order, a2c_common.py:33-40), so get_transformed_list (experience.py:508-522) is a view.
 * ---------------------------------------------------------------------------------- */

/* One launch for all `update_data(name, step, val)` calls of a step (a2c_common.py:1000-1011):
 * srcs[k] is [num_envs][row_bytes[k]] contiguous, dsts[k] the env-major field storage.
 * count <= 12.  srcs/dsts/row_bytes are HOST arrays of device pointers / sizes. */
int rlg_rollout_store_step(int count, const void* const* srcs, void* const* dsts,
                           const int* row_bytes, int num_envs, int horizon, int step,
                           void* stream);

/* Non-temporal stores for buffer rows of >= 128 bytes (observations); returns the previous setting,
 * enable < 0 only queries.  Default on. */
int rlg_rollout_store_streaming(int enable);

int rlg_rollout_post_step_num_blocks(int num_envs);

/* After vec_env.step: DefaultRewardsShaper (rl_games/common/tr_helpers.py:33-42; clamp_rewards bit 0 =
 * clamp to [rmin, rmax], bit 1 = log_val: log of the shaped reward behind the clamp), time-out bootstrap (a2c_common.py:1021-1023), update_data('rewards') (:1025),
 * current_rewards/current_shaped_rewards/current_lengths accumulate + zero-on-done
 * (:1027-1051).  Finished-episode sums go to ep_partials[step][block][2V+2] (fp64) and are
 * folded into the meters by rlg_episode_meters_update.  N counts rows (envs x agents); with num_agents > 1 only the
 * first agent row of an env feeds the meters (all_done_indices[::num_agents], :1040-1044).
 * Required: rewards, dones, values, rewards_buf, cur_rewards, cur_shaped, cur_lengths, ep_partials.  May be NULL:
 * time_outs (time_outs_kind and bootstrap are then read as 0), live_rows.  num_agents < 1 is read as 1.
 * A NULL descriptor: hipErrorInvalidValue.  N <= 0 returns 0 without a launch.  Then, before the runtime is asked for
 * anything, hipErrorInvalidValue for a NULL required pointer, V outside [1, 8], step outside [0, H).  Like every
 * descriptor of this header it is read before the entry returns. */
typedef struct rlg_post_step_desc {
  const float* rewards;        /* [N, V] raw env rewards of this step */
  const uint8_t* dones;        /* [N] done flags produced by this step */
  const void* time_outs;       /* [N] or NULL (infos['time_outs']) */
  int time_outs_kind;          /* 0 none, 1 uint8 / bool, 2 fp32 */
  const float* values;         /* [N, V] critic values of this step (res_dict['values']) */
  const float* live_rows;      /* [N] or NULL: 1 - prev_dones (next_step autoreset mask, :1002-1006) */
  float* rewards_buf;          /* env-major [N][H][V] */
  float* cur_rewards;          /* [N, V] */
  float* cur_shaped;           /* [N, V] */
  float* cur_lengths;          /* [N] */
  double* ep_partials;         /* [H][rlg_rollout_post_step_num_blocks(N)][2V+2]: sum rew[V], sum shaped[V], sum len, count */
  float shift, scale, rmin, rmax;
  int clamp_rewards;
  int bootstrap;               /* value_bootstrap and 'time_outs' in infos */
  float gamma;
  int N, H, V, step;           /* rows, horizon, value_size <= 8, the buffer slot written */
  int num_agents;              /* meters take one row per env: rows with row % num_agents == 0 */
} rlg_post_step_desc;
RLG_ABI_SIZE(rlg_post_step_desc, 136);

int rlg_rollout_post_step(const rlg_post_step_desc* desc, void* stream);

/* Replays AverageMeter.update (rl_games/algos_torch/torch_ext.py:333-342) for the three
 * episode meters (game_rewards, game_shaped_rewards, game_lengths; a2c_common.py:1042-1044)
 * over steps 0..horizon-1.  current_sizes is int[3], finished_total an int64 counter. */
int rlg_episode_meters_update(const double* ep_partials, int horizon, int num_blocks,
                              int value_size, int max_size, float* mean_rewards,
                              float* mean_shaped, float* mean_lengths, int* current_sizes,
                              long long* finished_total, void* stream);

/* Rollout policy head (rl_games/algos_torch/models.py:348-364, denorm_value :58-60) fused with
 * the update_data writes of its outputs (a2c_common.py:1008-1009).  heads [N, ld]: column 0 the
 * critic value, columns 1..A the action means; noise [N, A] ~ N(0,1).  Writes actions/mus/
 * sigmas/neglogpacs/values of step `step` into the env-major buffer fields and the contiguous
 * actions [N, A] / de-normalised values [N] the env step and the post-step kernel consume.
 * Value-source contract: value == NULL is column 0 of the heads - the entry reads (value, ld_value, value_repeat) as
 * (heads, ld, 1) and looks at neither ld_value nor value_repeat.  With value given - the rollout of an agent with a
 * central value network (a2c_common.py:593-600, central_value.py:208-228), whose critic's value replaces the actor's -
 * row r (env-major, r = env * value_repeat + agent) reads value[(r / value_repeat) * ld_value], de-normalised with the
 * statistics passed here (the critic's value_mean_std), and the heads' column 0 is not read: value.repeat(1, A)
 * .view(N * A, -1) of central_value.py:223-225 with value_repeat = A; ld_value < 1 or value_repeat < 1:
 * hipErrorInvalidValue.  Numeric contract: the outputs with value = the heads' own column 0, ld_value = ld,
 * value_repeat = 1 are those of value == NULL, bit for bit.
 * Required: heads, logstd, noise, the two outputs and the five buffer fields.  May be NULL: value; v_mean and v_var
 * together (no de-normalisation); env_actions_out (then act_low / act_high are not read).
 * A NULL descriptor: hipErrorInvalidValue.  N <= 0 returns 0 without a launch.  Then, before the runtime is asked for
 * anything, hipErrorInvalidValue for a NULL required pointer, v_mean without v_var, env_actions_out without act_low /
 * act_high, A <= 0, step outside [0, H). */
typedef struct rlg_policy_head_desc {
  const float* heads;      /* [N, ld] */
  int ld;
  const float* value;      /* NULL, or [ceil(N / value_repeat), ld_value], column 0 */
  long long ld_value;
  int value_repeat;
  const float* logstd;     /* [A] */
  const float* noise;      /* [N, A] standard normal */
  const double* v_mean;    /* value RunningMeanStd (fp64), or NULL when normalize_value is off */
  const double* v_var;
  float eps;
  float* actions_out;      /* [N, A] contiguous (goes to the env) */
  float* values_out;       /* [N] de-normalised values (the time-out bootstrap needs them) */
  float* buf_actions;      /* env-major [N][H][A] */
  float* buf_mus;
  float* buf_sigmas;
  float* buf_neglogp;      /* [N][H] */
  float* buf_values;       /* [N][H] */
  /* optional [N, A]: rescale_actions(low, high, clamp(actions, -1, 1)) - what preprocess_actions hands to the env when
   * clip_actions is set (a2c_common.py:725-733); act_low / act_high [A] */
  float* env_actions_out;
  const float* act_low;
  const float* act_high;
  int N, H, A, step;       /* rows, horizon, actions_num, the buffer slot written */
} rlg_policy_head_desc;
RLG_ABI_SIZE(rlg_policy_head_desc, 176);

int rlg_rollout_policy_head(const rlg_policy_head_desc* desc, void* stream);

/* Categorical rollout head (discrete_a2c / multi_discrete_a2c eval branch: rl_games/algos_torch/models.py:95-125,
 * :157-206, CategoricalMasked common/extensions/distributions.py:24-47, denorm_value :58-60) fused with the
 * update_data writes of its outputs (a2c_common.py:1008-1009).  logits [N, sum(sizes)] and value (column 0) with
 * any row strides (the chain's heads: one tensor [value | logits] for a shared trunk); branch_sizes a HOST array of
 * num_branches <= 16 sizes (more: hipErrorNotSupported); masks bool [N, sum(sizes)] or NULL.  Writes actions_out
 * [N, B] (int64, what env_step receives), de-normalised values_out [N], and slot `step` of the env-major buffer
 * fields actions [N][H][B], neglogpacs [N][H], values [N][H].
 *
 * Numeric contract: per row and branch, in fp32, one rounding per op, the op sequence of DiscreteA2CModel.forward:
 * masked logits set to exactly -1e8 (an all-masked row stays uniform); norm = l - (log(sum exp(l - m)) + m) with
 * m = max l (0 when infinite); p = exp(norm - max norm) / sum; a = argmax p / q (lowest index on ties); neglogp =
 * sum over the branches, left to right, of -norm[a].  The two exp sums are added in the order of torch's logsumexp
 * and softmax kernels for branches of < 128 actions, so norm and p are torch's bits on the same logits (wider branches:
 * last-bit differences).  Values: sqrt(var + eps) * clamp(v, -5, 5) + mean, as rlg_rollout_policy_head.
 * RNG contract: exp_noise holds the Exp(1) draws q in branch-major blocks, block b = [N, sizes[b]] contiguous at
 * N * (sizes[0] + ... + sizes[b-1]).  Drawing block b with exponential_ on the default generator, in branch order,
 * is exactly what Categorical(logits).sample() draws (multinomial's one-sample path: argmax(probs / Exp(1))), so
 * the actions are the torch path's, except where its top two p/q lie within a few ulps of each other.
 * Value-source contract: row r reads value[(r / value_repeat) * ld_value]; value_repeat = 1 is one value per row,
 * value_repeat = num_agents a central value network's one state row per env.  ld_value < 1 or value_repeat < 1:
 * hipErrorInvalidValue.
 * Required: logits, branch_sizes, exp_noise, value, the two outputs and the three buffer fields.  May be NULL:
 * masks_or_null (ld_masks is then not read); v_mean_or_null and v_var_or_null together.
 * A NULL descriptor: hipErrorInvalidValue.  num_envs <= 0 returns 0 without a launch.  Then, before the runtime is asked
 * for anything, more than 16 branches hipErrorNotSupported, and hipErrorInvalidValue for a NULL required pointer, v_mean
 * without v_var, no branch, a branch size < 1, ld_logits (with masks: ld_masks) below sum(sizes), step outside
 * [0, horizon). */
typedef struct rlg_categorical_head_desc {
  const float* logits;
  int ld_logits;
  const int* branch_sizes;     /* host array [num_branches] */
  int num_branches;
  const float* exp_noise;
  const uint8_t* masks_or_null;
  int ld_masks;
  const float* value;          /* [ceil(num_envs / value_repeat), ld_value], column 0 */
  int ld_value;
  int value_repeat;
  const double* v_mean_or_null;   /* value RunningMeanStd (fp64), or NULL when normalize_value is off */
  const double* v_var_or_null;
  float eps;
  int64_t* actions_out;
  float* values_out;
  int64_t* buf_actions;
  float* buf_neglogp;
  float* buf_values;
  int num_envs, horizon, step;
} rlg_categorical_head_desc;
RLG_ABI_SIZE(rlg_categorical_head_desc, 152);

int rlg_rollout_categorical_head(const rlg_categorical_head_desc* desc, void* stream);

/* play_steps_rnn zero-on-done: s[:, done_envs, :] = 0 (a2c_common.py:1150-1153).
 * states [layers][num_envs][units] contiguous. */
int rlg_rnn_zero_done_states(float* states, const uint8_t* dones, int layers, int num_envs,
                             int units, void* stream);

/* ------------------------------------------------------------------------------------
 * Players (csrc/play.hip): what runs behind the policy's heads when a checkpoint is played
 *   rl_games/algos_torch/players.py:60-83, :117-160 (get_action / get_masked_action);
 *   rl_games/common/player.py:242-330 (run: the episode accounting).
 * Common contract: launch-only (no allocation, no synchronise, capturable), no atomics, every clamp propagates NaN,
 * rows == 0 returns 0 without a launch.  Before the runtime is asked for anything: a NULL required pointer, rows < 0,
 * actions_num <= 0, a leading dimension < 1 (or smaller than the columns read), act_low without act_high (or the other
 * way round), a branch size <= 0: hipErrorInvalidValue; more than 16 branches: hipErrorNotSupported.
 * ---------------------------------------------------------------------------------- */

/* The action of a Gaussian policy.  heads [rows, ld_heads], the means in columns mu_col .. mu_col + actions_num - 1;
 * noise [rows, actions_num] contiguous or NULL; actions_out [rows, actions_num] contiguous.
 *   noise == NULL:  a = mu (logstd is not read and may be NULL);   else  a = mu + expf(logstd) * noise
 *   bounds given:   out = clamp(a, -1, 1) * ((hi - lo) / 2) + ((hi + lo) / 2), each op rounded on its own;  else out = a
 * Numeric contract: on the same heads, logstd and noise the output equals env_actions_out (bounds) / actions_out (none)
 * of rlg_rollout_policy_head bit for bit. */
int rlg_play_policy_head(const float* heads, int ld_heads, int mu_col, const float* logstd, const float* noise_or_null,
                         const float* act_low_or_null, const float* act_high_or_null, float* actions_out, int rows,
                         int actions_num, void* stream);

/* The action of a (multi-)categorical policy, actions_out int64 [rows, num_branches] contiguous.  Masked logits are set
 * to exactly -1e8.  exp_noise == NULL: per branch the arg-max by torch.argmax's rule on the CPU - lowest index on ties,
 * the first NaN wins, an all-masked branch gives 0.  Else the sample of rlg_rollout_categorical_head: the same op
 * sequence on the same branch-major Exp(1) draws, actions_out bit-identical to that entry's. */
int rlg_play_categorical_head(const float* logits, int ld_logits, const int* branch_sizes, int num_branches,
                              const float* exp_noise_or_null, const uint8_t* masks_or_null, int ld_masks,
                              int64_t* actions_out, int rows, void* stream);

/* Episode accounting of one step.  cur_rewards[i] += rewards[i * ld_rewards] (fp32), cur_lengths[i] += 1; where
 * dones[i], (cur_rewards[i], cur_lengths[i], 1) go into the workgroup's fp64 sums - fixed order - and both are zeroed.
 * partials_slot: fp64 [rlg_play_post_step_num_blocks(rows)][3], written whole (zeros where nothing finished). */
int rlg_play_post_step_num_blocks(int rows);
int rlg_play_post_step(const float* rewards, int ld_rewards, const uint8_t* dones, float* cur_rewards,
                       float* cur_lengths, double* partials_slot, int rows, void* stream);

/* One workgroup folds partials fp64 [slots][blocks][3] into totals (24 bytes: fp64 reward sum, fp64 length sum, int64
 * games): the slots in order, a slot's blocks in a fixed order, a slot only while games < games_limit at its start -
 * the host loop's "add the step, then break once games >= games_num".  The totals are the same bits however the slots
 * are spread over calls.  slots == 0 returns 0; slots < 0 or blocks < 1: hipErrorInvalidValue. */
int rlg_play_fold(const double* partials, int slots, int blocks, long long games_limit, double* totals, void* stream);

/* ------------------------------------------------------------------------------------
 * RunningMeanStd / advantage normalisation
 *   replaces rl_games/algos_torch/running_mean_std.py: RunningMeanStd.forward :69-114,
 *   _update_mean_var_count_from_moments :55-67; rl_games/algos_torch/torch_ext.py:
 *   get_mean_var_with_masks :182-191; ContinuousA2CBase.prepare_dataset value/advantage part
 *   (rl_games/common/a2c_common.py:1598-1634); GeneralizedMovingStats 'mean_std'
 *   (rl_games/algos_torch/moving_mean_std.py:52-61,:102-134,:136-150).
 * ---------------------------------------------------------------------------------- */

int rlg_column_moments_num_blocks(long long rows, int cols);

/* Per-block fp64 partial sums of a row-major fp32 [rows, cols] matrix:
 * partials[block][2*cols+1] = {sum x*m [cols], sum x*x*m [cols], sum m}; m = row mask or 1. */
int rlg_column_moments(const float* x, const float* row_mask_or_null, long long rows, int cols,
                       double* partials, int num_blocks, void* stream);

/* The same moments for num_segments consecutive bands of rows_per_segment rows in two launches -
 * the minibatches of one epoch, which every mini-epoch revisits unchanged (rl_games/common/
 * datasets.py:57-75: fixed slices): table[seg][2*cols+1] = {sum[cols], sumsq[cols], rows}.
 * partials: scratch of num_segments * num_blocks * (2*cols+1) doubles.  rlg_mlp_chain_forward folds
 * a table row into the running state in its prologue. */
int rlg_column_moments_segments(const float* x, long long rows_per_segment, int cols, int num_segments,
                                double* partials, int num_blocks, double* table, void* stream);

/* Chan merge of the batch moments into the fp64/int64 running state (running_mean_std.py:
 * 55-67).  mode 0: population variance, count += rows (:74-75,:83); mode 1: masked moments
 * of get_mean_var_with_masks, count += rows (:72,:83); mode 2: moments of the selected rows
 * only, count += #selected (values[valid], a2c_common.py:1609-1611).  `ticket` is a zero-initialised
 * device word owned by the caller (self-resetting arrival counter of the per-column blocks). */
int rlg_rms_update(const double* partials, int num_blocks, int cols, long long total_rows,
                   int mode, double* running_mean, double* running_var, long long* count,
                   unsigned int* ticket, void* stream);

/* y = clamp((x-mean)/sqrt(var+eps),-5,5) (mode 0, :112-113); denorm (mode 1, :106-107);
 * norm_only (mode 2, :110).  mean/var are the fp64 buffers, cast to fp32 like `.float()`. */
int rlg_rms_apply(const float* x, float* y, long long rows, int cols, const double* running_mean,
                  const double* running_var, float eps, int mode, void* stream);

/* Cross-rank synchronisation of ALL running normalisers of an agent, once per epoch (multi-GPU).
 *   replaces rl_games/common/a2c_common.py: _running_stats_totals :43-47, seed_stats_sync_snapshot
 *   :50-58, merge_rank_stats :61-93, broadcast_rank_stats :124-141; called from
 *   A2CBase.sync_running_stats :782-808 and _seed_stats_sync_snapshots :766-780.
 * The reference runs ~12 fp64 torch ops and THREE collectives per normaliser; here normaliser s
 * (state: means[s] / vars[s] fp64 [dims[s]], counts[s] int64 scalar) is the segment
 *   [count | first moments [dims[s]] | second moments [dims[s]]]
 * of one flat fp64 buffer (segments back to back, rlg_stats_sync_flat_size doubles), so an epoch's
 * exchange is pack -> ONE collective over the flat buffer -> apply.  num_segments <= 8.  Same fp64
 * operations in the same order as the reference (bit-identical statistics for identical reduced
 * sums); counts travel as doubles (exact below 2^53).  has_snapshot[s] == 0: the segment's whole
 * history is rank-local (no merge yet, :72-74) - its base is zero.
 * pack  mode 0: out = totals(state) - snapshot (this epoch's deltas);  mode 1: snapshot = totals(state)
 *       (after loading a checkpoint; out unused);  mode 2: out = raw state [count, mean, var] (broadcast mode).
 * apply mode 0: totals = snapshot + reduced;  mean = s1/n, var = max(s2/n - mean^2, 1e-8);  snapshot = totals;
 *       mode 2: state = reduced (rank 0's raw state after a broadcast). */
long long rlg_stats_sync_flat_size(int num_segments, const int* dims);
int rlg_stats_sync_pack(int num_segments, double* const* means, double* const* vars, long long* const* counts,
                        const int* dims, const int* has_snapshot, double* snapshot, double* out, int mode,
                        void* stream);
int rlg_stats_sync_apply(int num_segments, double* const* means, double* const* vars, long long* const* counts,
                         const int* dims, const int* has_snapshot, double* snapshot, const double* reduced, int mode,
                         void* stream);

int rlg_prepare_stats_bytes(void);

/* value_size==1 prepare_dataset statistics from the GAE kernel's partial moments: updates the
 * value RunningMeanStd with `values` then `returns` (a2c_common.py:1616-1619), computes the
 * advantage mean / unbiased std + 1e-8 (:1634) or the EMA statistics (moving_mean_std.py).
 * flags: 1 normalize_value, 2 normalize_advantage, 4 freeze_critic, 8 normalize_rms_advantage. */
/* Same 6 sums as the GAE kernel's partials (7 with a mask: + sum mask, every term weighted
 * by the mask) for batches that did not come out of rlg_gae_envmajor_fused. */
int rlg_triple_moments_num_blocks(long long batch);
int rlg_triple_moments(const float* advantages, const float* values, const float* returns,
                       const float* mask_or_null, long long batch, double* partials, int num_blocks,
                       void* stream);

/* stride 6: unmasked partials; stride 7: masked (valid-row statistics, a2c_common.py:1605-1615,
 * torch_ext.py:172-191). */
int rlg_prepare_finalize(const double* gae_partials, int num_tiles, int stride, long long batch,
                         int flags,
                         double* value_running_mean, double* value_running_var,
                         long long* value_count, float eps, float* ema_mean, float* ema_sqrs,
                         int* ema_step, float ema_decay, float ema_factor, float ema_max,
                         float ema_eps, void* stats_out, void* stream);

/* values/returns normalised with their respective statistics, advantages normalised
 * (a2c_common.py:1618-1619,:1634).  Outputs may alias the inputs. */
int rlg_prepare_apply(const float* values, const float* returns, const float* advantages,
                      float* values_out, float* returns_out, float* advantages_out, long long batch,
                      int flags, const void* stats, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused clipped-PPO loss forward + backward + KL
 *   replaces rl_games/algos_torch/models.py: ModelA2CContinuousLogStd epilogue :333-347,
 *   neglogp :361-364; rl_games/algos_torch/a2c_continuous.py: calc_losses :97-134,
 *   bound_loss/reg_loss :241-257, the KL block of calc_gradients :215-221;
 *   rl_games/common/common_losses.py: actor_loss :64-82, smoothed_actor_loss :39-61,
 *   default_critic_loss :16-29; rl_games/algos_torch/torch_ext.py: apply_masks :157-170,
 *   policy_kl :27-36; rl_games/common/datasets.py: PPODataset.update_mu_sigma :33-43.
 * ---------------------------------------------------------------------------------- */

int rlg_ppo_loss_num_blocks(int minibatch);
int rlg_ppo_loss_partials_per_block(int actions);

/* mu [mb,A], logstd [A] (fixed sigma, 'exp'), values [mb]; dataset slices actions [mb,A],
 * old_neglogp/advantages/old_values/returns [mb], old_mu/old_sigma [mb,A] (overwritten with
 * the new mu/sigma when write_back).  Emits d_mu [mb,A], d_values [mb] (already scaled by
 * 1/mb or mask/sum(mask)) and fp64 partials [blocks][rlg_ppo_loss_partials_per_block(A)].
 * mu/values/d_mu/d_values take row strides ld_* (elements) so they can be column views of a fused
 * [mb, 1+A] head buffer.  bound_kind 0 none / 1 'bound' / 2 'regularisation'.
 * use_smooth_clamp selects the actor loss of rl_games/common/common_losses.py:39-82: 0 = actor_loss (clipped PPO),
 * 1 = smoothed_actor_loss (`use_smooth_clamp: True`), 2 = `ppo: False` (a_loss = neglogp * advantage, either function's
 * else branch; round 6) - here and in every entry point / descriptor that carries the flag.
 * The arguments travel as a descriptor, which the chain's backward launches take as well (rlg_mlp_chain_backward, _step,
 * _backward_lean, _backward_bx).  Like every descriptor of this header it is read before the entry returns and may be
 * freed or reused then (rlg_mlp_dw_launch does the same with its own); NULL: hipErrorInvalidValue. */
typedef struct rlg_ppo_loss_desc {
  const float* mu;            /* [rows, A] view, row stride ld_mu */
  const float* logstd;        /* [A] */
  const float* values;        /* [rows] view, stride ld_values */
  const float* actions;       /* [rows, A] */
  const float* old_neglogp;   /* [rows] */
  const float* advantages;
  const float* old_values;
  const float* returns;
  float* old_mu;              /* [rows, A] read, then overwritten when write_back */
  float* old_sigma;
  const float* mask_or_null;
  const float* mask_sum_or_null;
  float* d_mu;                /* [rows, A] view, row stride ld_d_mu */
  float* d_values;            /* [rows] view, stride ld_d_values */
  double* partials;
  int minibatch, actions_num;
  int ld_mu, ld_values, ld_d_mu, ld_d_values;
  float e_clip, critic_coef, bounds_coef;
  int clip_value, use_smooth_clamp, bound_kind, write_back;
} rlg_ppo_loss_desc;
RLG_ABI_SIZE(rlg_ppo_loss_desc, 176);

int rlg_ppo_loss_fused(const rlg_ppo_loss_desc* desc, void* stream);

/* Value-only loss of the central value network - replaces CentralValueTrain.calc_loss
 * (rl_games/algos_torch/central_value.py:262-276: common_losses.critic_loss + apply_masks).
 * partials [ceil(mb/256)][7] feed rlg_ppo_loss_finalize (actions_num 0, critic_coef 2 -> total =
 * mean c_loss); d_values [mb] = d mean(c) / d value. */
int rlg_value_loss(const float* values, const float* old_values, const float* returns,
                   const float* mask_or_null, const float* mask_sum_or_null, float* d_values, double* partials,
                   int minibatch, float e_clip, int clip_value, void* stream);

/* Discrete (Categorical) variant - replaces rl_games/algos_torch/a2c_discrete.py:
 * DiscreteA2CAgent.calc_gradients :121-209 with the model epilogues ModelA2C (models.py:95-111) and
 * ModelA2CMultiDiscrete (:153-179) incl. CategoricalMasked (common/extensions/distributions.py:24-47):
 * logits [mb, n] (row stride ld), n = sum(branch_sizes); actions int64 [mb, num_branches];
 * action_masks bool [mb, n] or NULL.  Emits d_logits [mb, n] (actor + entropy terms, scaled) and
 * d_values [mb]; partials [blocks][7] feed rlg_ppo_loss_finalize with actions_num = 0
 * (kl = 0.5 (old_nlp - nlp)^2, :192-198).
 * The heads may live inside wider rows (the fused chain's [value | logits] head matrix and its gradient): values /
 * d_values take an element stride, d_logits a row stride; separate contiguous tensors are ld_values = ld_d_values = 1,
 * ld_d_logits = n.  Each row's neglogp (the sum over the branches, as the loss used it) is also stored into
 * new_neglogp_or_null [mb] - the per-minibatch diagnostics read it (rlg_ppo_diag).  NULL: no store.
 * Required: every pointer not named _or_null; mask_or_null needs mask_sum_or_null.  Before the runtime is asked for
 * anything, hipErrorInvalidValue for a NULL descriptor or required pointer, minibatch <= 0, num_branches outside
 * [1, 16], a branch size < 1, ld_values or ld_d_values < 1, ld_logits or ld_d_logits below n, a mask without its sum. */
int rlg_ppo_loss_discrete_num_blocks(int minibatch);
typedef struct rlg_discrete_loss_desc {
  const float* logits;
  long long ld_logits;
  const float* values;
  long long ld_values;
  const long long* actions;
  const unsigned char* action_masks_or_null;
  const int* branch_sizes;     /* host array [num_branches] */
  int num_branches;
  const float* old_neglogp;
  const float* advantages;
  const float* old_values;
  const float* returns;
  const float* mask_or_null;
  const float* mask_sum_or_null;
  float* d_logits;
  long long ld_d_logits;
  float* d_values;
  long long ld_d_values;
  double* partials;
  int minibatch;
  float e_clip, critic_coef, entropy_coef;
  int clip_value, use_smooth_clamp;
  float* new_neglogp_or_null;
} rlg_discrete_loss_desc;
RLG_ABI_SIZE(rlg_discrete_loss_desc, 184);

int rlg_ppo_loss_discrete_nlp(const rlg_discrete_loss_desc* desc, void* stream);

/* PPO diagnostics (`use_diagnostics`; rl_games/common/diagnostics.py, torch_ext.py:182-227), csrc/ppo_diag.hip.  A row of
 * the diagnostics table is rlg_ppo_diag_stats() = 10 fp64: {rows, W = sum m, C = sum m*clipped, mean_ret, M2_ret,
 * mean_val, M2_val, mean_d, M2_d, elements}.  Both launches write (do not accumulate) their columns, fold their
 * workgroups' partials in a fixed order (no float atomics: bit-reproducible), take one zero-initialised uint ticket per
 * output row and leave it at zero; no host synchronisation: capturable.
 *
 * rlg_ppo_diag - one minibatch, columns 0..2; m = mask[i] (1 without a mask).  Row i is clipped when
 * (old_neglogp[i] - new_nlp) in fp32 is < log_lo or > log_hi, log_lo / log_hi = fp32(log(1 -/+ e_clip)).
 * new_nlp: new_neglogp_or_null[i], or - NULL - recomputed with the continuous loss tile's arithmetic from mu [mb, A]
 * (row stride ld_mu), logstd [A] and actions [mb, A]: z = (x - mu) / expf(logstd),
 * nlp = (0.5 fp32(sum_f64 z^2) + fp32(0.9189385332046727 A)) + fp32(sum_f64 logstd); 1 <= A <= 32.
 * neglogp_out_or_null [mb] receives the new_nlp of every row.  partials: rlg_ppo_diag_num_blocks(mb) x 3 doubles.
 *
 * rlg_ppo_diag_moments - `slices` consecutive minibatch slices of rows x cols values / returns (row-major) and
 * rows masks each, columns 3..9 of the row out + s * ld_out of slice s: the m(row)-weighted centred moments
 * (mean, M2 = sum m (x - mean)^2, fp64 Welford + Chan merges) of returns, values and d = returns - values (fp32) over
 * the slice's rows x cols elements, and the element count.  partials: slices x rlg_ppo_diag_moments_num_blocks(rows,
 * cols) x 9 doubles; tickets: slices uints. */
int rlg_ppo_diag_stats(void);
int rlg_ppo_diag_num_blocks(int minibatch);
int rlg_ppo_diag(const float* mu, long long ld_mu, const float* logstd, const float* actions, long long ld_actions,
                 const float* new_neglogp_or_null, const float* old_neglogp, const float* mask_or_null, int minibatch,
                 int actions_num, float log_lo, float log_hi, double* partials, unsigned int* ticket, double* out,
                 float* neglogp_out_or_null, void* stream);
int rlg_ppo_diag_moments_num_blocks(int rows, int cols);
int rlg_ppo_diag_moments(const float* values, const float* returns, const float* mask_or_null, int slices, int rows,
                         int cols, double* partials, unsigned int* tickets, double* out, long long ld_out,
                         void* stream);

/* scalars8 = {a_loss, c_loss, entropy, b_loss, kl, loss, sum(mask), 0}; d_logstd [A];
 * kl_slot_or_null receives the KL as well (e.g. the tail slot of the flat gradient arena);
 * d_mu_bias_or_null [A] / d_value_bias_or_null [1] receive sum_rows d_mu / d_values, i.e. the
 * bias gradients of the mu and value heads (what nn.Linear's backward computes with sum(0)).
 * rlg_mlp_dw_launch takes the same descriptor and folds the loss partials in its finalise launch (a few extra
 * workgroups next to the weight-gradient ones) instead of a launch of its own - the head-bias / logstd gradients, the
 * loss scalars and the KL are then ready when the weight gradients are.  NULL here: hipErrorInvalidValue. */
typedef struct rlg_loss_finalize_desc {
  const double* partials;
  int num_blocks, actions_num, minibatch, masked;
  float critic_coef, entropy_coef, bounds_coef;
  float* scalars8;
  float* d_logstd;
  float* kl_slot_or_null;
  float* d_mu_bias_or_null;
  float* d_value_bias_or_null;
} rlg_loss_finalize_desc;
RLG_ABI_SIZE(rlg_loss_finalize_desc, 80);

int rlg_ppo_loss_finalize(const rlg_loss_finalize_desc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Gradient truncation + Adam + adaptive learning rate on a flat arena
 *   replaces rl_games/common/a2c_common.py: trancate_gradients_and_step :493-514, update_lr
 *   :564-576, the per-minibatch schedule :1557-1563; rl_games/common/schedulers.py:
 *   AdaptiveScheduler.update :27-33; optimiser built at a2c_continuous.py:44-48.
 * ---------------------------------------------------------------------------------- */

int rlg_grad_norm_num_blocks(long long n);
/* Also increments *step_counter_or_null (the device-resident Adam step count) by one. */
int rlg_grad_sumsq(const float* grads, long long n, float grad_scale, double* partials,
                   int num_blocks, long long* step_counter_or_null, void* stream);

/* One optimiser step over n contiguous parameters: the arguments of the four rlg_adam_* entries.  No per-call host
 * scalars - step and learning rate are device words - so a (norm, Adam) launch pair replays from a captured HIP graph.
 * The entries read the descriptor before they return; it may be freed or reused then.  hipErrorInvalidValue: a NULL
 * descriptor, n <= 0, no step_counter, schedule_kind 1 without kl_or_null, an arena that is not 16-byte aligned. */
typedef struct rlg_adam_desc {
  float* params;
  float* grads;                 /* overwritten with the scaled / clipped gradient (like clip_grad_norm_) */
  float* exp_avg;
  float* exp_avg_sq;            /* the four arenas: [n] fp32, 16-byte aligned */
  long long n;
  const double* norm_partials_or_null;  /* [norm_blocks] sums of (grad * grad_scale)^2 (rlg_grad_sumsq, rlg_mlp_dw_launch):
                                         * grads are also scaled by the clip coefficient min(1, max_norm / (norm + 1e-6));
                                         * NULL: no truncation */
  int norm_blocks;
  float grad_scale;             /* 1 / world_size (multi-GPU average), 1 otherwise */
  float max_norm;               /* grad_norm */
  double* lr_slots;             /* [2] fp64; slot (step - 1) & 1 is the lr of this step, the other receives the next lr */
  const long long* step_counter;  /* device word: the 1-based Adam step of THIS update (advanced by rlg_grad_sumsq) */
  double beta1, beta2, eps, weight_decay;
  int schedule_kind;            /* 0 keep the lr, 1 KL-adaptive on *kl_or_null * kl_scale (the KL of THIS minibatch) */
  const float* kl_or_null;      /* device scalar */
  float kl_scale;               /* 1 / world_size when *kl_or_null holds a cross-rank SUM */
  double kl_threshold, min_lr, max_lr, lr_multiplier;
  float* stats_out_or_null;     /* [4] = {total_norm, clip_coef, lr_used, lr_next} */
  const unsigned* skip_flag_or_null;  /* device word (rlg_ipc_comm_error_word); non-zero = the gradients are invalid (a
                                       * failed in-graph all-reduce): parameters and moments stay untouched, the lr is
                                       * carried over unchanged */
} rlg_adam_desc;
RLG_ABI_SIZE(rlg_adam_desc, 184);

int rlg_adam_step(const rlg_adam_desc* desc, void* stream);

/* rlg_adam_step that also leaves the fused chain's weight planes (both directions, the layout and buffer of
 * rlg_mlp_chain_pack_planes direction 2) for the NEW weights: the thread that updates a 4 x 4 block of a weight
 * matrix writes its rows as forward fragments and its columns as backward fragments (csrc/mlp_chain_bx.hip,
 * adam_pack_kernel) - one launch instead of rlg_adam_step + rlg_mlp_chain_pack_planes per optimiser step, and no pack
 * launch in front of the rollout forwards.  Same Adam arithmetic, same plane bytes.  hipErrorInvalidValue (use the
 * two launches) unless the four arenas are 16-byte aligned (as for rlg_adam_step) and every weights[l] lies inside
 * [params, params + n) at a multiple of 4 floats with in_features[l] % 4 == 0; `planes` must have been packed in full
 * once (the zero padding of the fragments). */
int rlg_adam_step_pack(const rlg_adam_desc* desc, int num_layers, const float* const* weights, const int* in_features,
                       const int* out_features, void* planes, void* stream);

/* ------------------------------------------------------------------------------------
 * Range guard of the split-fp16 products (csrc/range_guard.hip)
 *   The split-fp16 launches hold |weight| < 1023 and |hidden activation| < 4094 (csrc/bx_form.hpp); past that a plane
 *   is Inf and what is computed from it is Inf / NaN.  The guard record is 4 device words (16-byte aligned, zeroed by
 *   the caller = clear): record[0] = tag of what tripped (0: nothing), record[1] = where; record[2..3] belong to the
 *   scan.  A set record is sticky: no launch below changes it.
 *   rlg_range_scan: ONE launch over up to 8 fp32 arrays (arrays[k], counts[k] elements, tags[k] != 0).  On a non-finite
 *   value: record[0] = the tag of the first array in argument order that holds one, record[1] = the smallest offending
 *   flat index in that array - whatever the scheduling.  Clean arrays: 16-byte loads and no store, no atomic.  A launch
 *   that finds the record set leaves it bit for bit.  Capturable; a captured launch must not be replayed over a record
 *   that an earlier replay of itself set (it would take that record for its own and keep the better of the two hits).
 *   hipErrorInvalidValue before the runtime is asked for anything: NULL or misaligned record, num_arrays outside
 *   [0, 8], a negative count or one above 2^32 - 1, a tag of 0, a NULL array with a non-zero count.
 *   rlg_adam_step_guarded / rlg_adam_pack_guarded: rlg_adam_step / rlg_adam_step_pack with such a record (not NULL) and
 *   with norm_partials (not NULL, norm_blocks > 0: the guard watches the norm; max_norm = +Inf never clips).
 *   The launch is skipped exactly as under skip_flag - parameters, moments, planes untouched, the learning rate carried
 *   over, the step counter as skip_flag leaves it - when the record is set or the total gradient norm (with
 *   norm_partials) is not finite; in the second case a clear record becomes (RLG_GUARD_TAG_ADAM, low 32 bits of the
 *   optimiser step).  An infinite norm trips too, where the unguarded launch clips with coefficient 0.  The unguarded
 *   entries are unchanged: a NaN norm reaches every parameter, as torch.clamp would have it.
 * ---------------------------------------------------------------------------------- */
#define RLG_GUARD_TAG_ADAM 0x4144414d   /* 'ADAM' */
int rlg_range_scan(int num_arrays, const float* const* arrays, const long long* counts, const int* tags,
                   unsigned* record, void* stream);
int rlg_adam_step_guarded(const rlg_adam_desc* desc, unsigned* guard_record, void* stream);
int rlg_adam_pack_guarded(const rlg_adam_desc* desc, unsigned* guard_record, int num_layers, const float* const* weights,
                          const int* in_features, const int* out_features, void* planes, void* stream);

/* ------------------------------------------------------------------------------------
 * Manual MLP backward helpers
 *   replace, per hidden layer of A2CBuilder's MLP (rl_games/algos_torch/network_builder.py:
 *   118-147, forward :498), aten's activation backward + the bias-gradient sum(0) of
 *   nn.Linear's backward that loss.backward() (a2c_continuous.py:211) runs.
 * ---------------------------------------------------------------------------------- */

int rlg_act_bwd_num_blocks(long long rows, int cols);

/* d_pre = d_out * act'(pre_act) (may alias d_out), partials[block][cols] = column sums of d_pre.
 * act_kind 0 identity, 1 elu(alpha 1), 2 relu, 3 tanh; 17 / 18 / 19: the same derivatives evaluated
 * from the layer OUTPUT act(z) passed as `pre_act` (in-place activations; aten's elu_backward with
 * is_result = true: h > 0 ? 1 : h + 1).  cols % 4 == 0, ld = row stride. */
int rlg_act_bwd_colsum(const float* d_out, const float* pre_act, float* d_pre, long long rows,
                       int cols, long long ld, int act_kind, double* partials, int num_blocks,
                       void* stream);

/* out[c] (+)= sum_b partials[b][c]: the bias gradient. */
int rlg_colsum_finalize(const double* partials, int num_blocks, int cols, float* out, int accumulate,
                        void* stream);

/* ------------------------------------------------------------------------------------
 * fp32-MFMA MLP layer kernels (fused epilogues)
 *   replace torch.addmm + activation of every nn.Linear/activation pair built by
 *   A2CBuilder._build_sequential_mlp (rl_games/algos_torch/network_builder.py:118-147, forward
 *   :498) and the mu/value heads (:295-311).
 * ---------------------------------------------------------------------------------- */

/* ---- MLP forward / input-gradient GEMMs on f32 MFMA with fused epilogues -------------------
 * H = act(X W^T + b) (+ Z) replaces nn.Linear + activation of A2CBuilder._build_sequential_mlp and
 * the heads (rl_games/algos_torch/network_builder.py:118-147, :295-311, forward :498-512);
 * dZ_prev = (dZ W) * act'(Z_prev) replaces their autograd (grad_output.mm(weight) + elu_backward).
 * in_features (forward) / out_features (backward) must be a multiple of 4 (rlg_mlp_rowgemm_supported). */
int rlg_mlp_rowgemm_supported(int reduction_dim, long long leading_dim);
int rlg_mlp_linear_act_forward(const float* x, long long ldx, const float* w, const float* bias_or_null,
                               float* pre_act_or_null, float* out, long long ldo, int rows, int out_features,
                               int in_features, int act_kind, void* stream);
int rlg_mlp_linear_act_backward(const float* dz, long long lddz, const float* w, const float* z_prev_or_null,
                                float* dz_prev, long long ldo, int rows, int out_features, int in_features,
                                int act_kind, void* stream);

/* ---- MLP weight gradients on the matrix cores -----------------------------------------------
 * G_l [No, Mi] = dZ_l^T X_l for every nn.Linear of the policy MLP in ONE launch (+ one finalise
 * launch): replaces autograd's `grad_output.t().mm(input)` of A2CBuilder's layers
 * (rl_games/algos_torch/network_builder.py:118-147, heads :295-311; torch.nn.Linear backward).
 * fp32 in, fp32 out, fp32 accumulation.  Products: split-bf16 (each fp32 product as six exact bf16 plane
 * products on v_mfma_f32_16x16x32_bf16, truncation <= 3 * 2^-24 |x||y| - as accurate against fp64 as
 * exact products) by default; RLG_DW_BF16=0 in the environment selects exact f32 products
 * (v_mfma_f32_16x16x4_f32, 1.4x slower).
 * rlg_mlp_dw_plan fills plan4 = {bo, tiles_o, tiles_i, ksplit} for one layer and returns the
 * workspace size in floats (-1: shape unsupported, use the library GEMM); target_blocks <= 0: the
 * default workgroup count. */
long long rlg_mlp_dw_plan(int rows, int out_features, int in_features, int target_blocks, int* plan4);
/* One weight-gradient launch: rlg_mlp_dw_launch / rlg_mlp_dw_launch_form.  Arrays are indexed by job (= layer); the
 * descriptor is read before the entry returns.  hipErrorInvalidValue: a NULL descriptor, num_layers outside [1, 8], rows
 * <= 0, num_colsums outside [0, 8], a bad plan / misaligned workspace or gradient, a bad maxima field (below). */
typedef struct rlg_mlp_dw_desc {
  int num_layers;
  int rows;
  const float* const* dz;          /* [rows, out_features[l]] contiguous */
  const float* const* x;           /* [rows, in_features[l]] contiguous */
  float* const* partial;           /* split-K workspace of rlg_mlp_dw_plan's size, 16-byte aligned */
  float* const* grad;              /* [out_features[l], in_features[l]], 16-byte aligned */
  const int* out_features;
  const int* in_features;
  const int* plans4;               /* [4 * num_layers] from rlg_mlp_dw_plan */
  /* bias gradients `grad_output.sum(0)` finished in the same finalise launch from the per-block fp64 column sums of
   * rlg_act_bwd_colsum / the chain's backward (partials [blocks][cols]); num_colsums may be 0 */
  int num_colsums;
  const double* const* colsum_partials;
  const int* colsum_blocks;
  const int* colsum_cols;
  float* const* colsum_out;
  const rlg_loss_finalize_desc* loss_finalize_or_null;  /* rlg_ppo_loss_finalize's work rides in the finalise launch */
  /* optional by-product: norm_partials[b] = sum (g * grad_scale)^2 over the gradient elements finalise block b wrote
   * (*finalize_blocks_out blocks, host int) - the input of rlg_adam_step's clipping when THIS launch produces every
   * gradient of the arena and nothing touches them before Adam (single GPU); it then also advances step_counter like
   * rlg_grad_sumsq does. */
  double* norm_partials_or_null;
  float grad_scale;
  long long* step_counter_or_null;
  int* finalize_blocks_out_or_null;
  /* Split-fp16 form.  The launch sums over the batch rows, so it scales an operand by ONE power of two per K-slice of
   * rows: dz of job k by what the largest entry over a wave's rows asks for, maxima[dz_slot[k] * maxima_stride + e] = the
   * largest |dZ| of rows [e * maxima_rows_per_entry, ...) as the chain's backward launch left them (rlg_chain_bwd), x of
   * job k by x_scale[k], the fixed power of two the forward splits the same tensor with (16 for hidden activations,
   * 4096 for normalised observations).  NULL maxima: the other fields are not read, the launch runs the bf16 form.  With
   * maxima: maxima_stride <= 0, maxima_rows_per_entry other than 16 / 64, a dz_slot outside [0, 7] or an x_scale that is
   * not > 0 is hipErrorInvalidValue; a stride below ceil(rows / maxima_rows_per_entry) counts as no maxima. */
  const float* maxima_or_null;
  int maxima_stride;
  int maxima_rows_per_entry;
  const int* dz_slot;
  const float* x_scale;
} rlg_mlp_dw_desc;
RLG_ABI_SIZE(rlg_mlp_dw_desc, 176);

/* The product form is the library's choice: three fp16 plane products with maxima, else six bf16 plane products
 * (RLG_DW_BF16 / RLG_DW_F16 in the environment are the defaults of that choice). */
int rlg_mlp_dw_launch(const rlg_mlp_dw_desc* desc, void* stream);

/* rlg_mlp_dw_launch with the product form of THIS launch instead of the process-wide environment switches: form 0 =
 * exact f32 products (no range limit), 1 = six bf16 plane products, 2 = three fp16 plane products (needs the
 * descriptor's maxima, else hipErrorInvalidValue; |x| * x_scale must stay below 65,504), -1 = the library's choice, i.e.
 * rlg_mlp_dw_launch.  Plans of rlg_mlp_dw_plan serve every form. */
int rlg_mlp_dw_launch_form(int form, const rlg_mlp_dw_desc* desc, void* stream);

/* ---- the MLP as one vertically fused chain on f32 MFMA (csrc/mlp_chain.hip) ------------------
 * forward : heads = head(act(... act(norm(x) W_0^T + b_0) ...)) for a row tile, every layer in ONE
 *           launch with the activations resident in LDS; replaces A2CBuilder.Network.forward
 *           (rl_games/algos_torch/network_builder.py:447-512: actor_mlp + value/mu heads, arranged
 *           as one [1+A, K] last layer) and norm_obs in front of it (rl_games/algos_torch/models.py:
 *           54-56; RunningMeanStd eval formula rl_games/algos_torch/running_mean_std.py:112-113).
 *           act_out[l] (row stride act_ld[l]) receives layer l's output: required for the last
 *           layer (the heads), optional (training: what backward needs) for the hidden ones;
 *           xn_out (optional) receives the normalised observations [rows, in_0].
 * backward: dZ_{l-1} = (dZ_l W_l) * act'_{l-1}(H_{l-1}) down the chain from d_out = d loss / d heads
 *           (autograd's grad_output.mm(weight) + activation backward + bias sum(0) per nn.Linear);
 *           dz_out[l] (l < last) receives dZ_l, bias_partials[l] (optional) [num_blocks, out_l]
 *           fp64 per-workgroup column sums of dZ_l (finished by rlg_mlp_dw_launch's colsum items).
 * acts: 0 identity, 1 elu, 2 relu, 3 tanh (backward evaluates act' from the layer OUTPUT).
 * groups: 16-row groups per workgroup, 1 / 2 / 4 (0 = chosen from rows and direction:
 * rlg_mlp_chain_groups; rlg_mlp_chain_num_blocks takes the resolved value).  direction of rlg_mlp_chain_groups and
 * rlg_mlp_chain_bx_supported names the launch kind: 0 = inference forward, 1 = backward, 2 = training forward (activations
 * kept) - the 64-row split-product kernels take training launches from 8,192 rows, inference forwards from 16,384.
 * rlg_mlp_chain_lds_bytes: LDS of one workgroup (direction 0 forward, 1 backward), -1 if the
 * network does not fit the 160 KiB LDS with that many groups. */
int rlg_mlp_chain_prepare(void);   /* once per process, outside stream capture: raises the kernels' LDS limit */
int rlg_mlp_chain_groups(long long rows, int requested, int direction);
int rlg_mlp_chain_num_blocks(long long rows, int groups);
int rlg_mlp_chain_lds_bytes(int num_layers, const int* in_features, const int* out_features, int groups,
                            int direction);
/* tools only: the following forward launches record shader-clock stamps per phase into
 * buffer [blocks][4 waves][32] (int64); NULL switches it off. */
int rlg_mlp_chain_debug_stamps(long long* buffer);
/* plane products per fp32 product of the split-product chain kernels: 3 (two fp16 planes per operand) */
int rlg_mlp_chain_split_products(void);

/* The six launching entries (rlg_mlp_chain_forward / _backward / _step and their _lean forms) take their arguments as
 * descriptors: the network, the forward half, the backward half, the launch.  Like every descriptor of this header they
 * are read before the entry returns; a NULL one is hipErrorInvalidValue, answered first. */
typedef struct rlg_chain_net {
  int num_layers;
  const float* const* weights;      /* [out, in] fp32 per layer; the lean entries read fragments instead: may be NULL there */
  const float* const* biases;       /* NULL: no biases (the backward entries do not read it) */
  const int* in_features;
  const int* out_features;
  const int* acts;                  /* 0 identity, 1 elu, 2 relu, 3 tanh */
} rlg_chain_net;
RLG_ABI_SIZE(rlg_chain_net, 48);

typedef struct rlg_chain_fwd {
  float* const* act_out;            /* layer l's output: required for the last layer (the heads), optional for the hidden */
  const long long* act_ld;          /*   ones (training: what backward needs; the step entries need all); row strides */
  const float* x;                   /* observations [rows, in_0], row stride ldx */
  long long ldx;
  const double* rms_mean_or_null;   /* RunningMeanStd state: normalise x on the way in; NULL: x as it is */
  const double* rms_var;
  float rms_eps;
  float* xn_out_or_null;            /* receives the normalised observations [rows, in_0] */
  /* training-mode RunningMeanStd.forward (rl_games/algos_torch/running_mean_std.py:69-84, called from models.py:54-56):
   * fold this minibatch's column moments rms_batch = {sum[in], sumsq[in], rows} (rlg_column_moments_segments) into the
   * state BEFORE normalising; the new state goes to the *_out buffers, which must differ from the inputs (every
   * workgroup folds from the old state).  NULL rms_batch: normalise with the state as it is. */
  const double* rms_batch_or_null;
  const long long* rms_count;
  double* rms_mean_out;
  double* rms_var_out;
  long long* rms_count_out;
  const void* weight_form_or_null;  /* rlg_mlp_chain_forward: forward planes (the 64-row split kernel runs when it applies);
                                     * the lean entries: forward fragments, required */
  void* pack_backward_planes_or_null;  /* rlg_mlp_chain_forward only: split the weights for the backward launch that
                                        * follows, in extra workgroups at the end of the grid */
} rlg_chain_fwd;
RLG_ABI_SIZE(rlg_chain_fwd, 120);

typedef struct rlg_chain_bwd {
  const float* const* act_in;       /* H_l of the hidden layers (the forward's act_out) and their row strides; the step */
  const long long* act_ld;          /*   entries do not read the two: H is their forward half's act_out */
  float* d_out;                     /* d loss / d heads [rows, out_last], row stride ld_dout; read, and with a loss */
  long long ld_dout;                /*   descriptor written first by the launch's own loss tile */
  float* const* dz_out;             /* dZ_l of the hidden layers and their row strides */
  const long long* dz_ld;
  double* const* bias_partials_or_null;  /* [num_blocks, out_l] fp64 per-workgroup column sums of dZ_l (finished by
                                          * rlg_mlp_dw_launch's colsum items) */
  /* With a descriptor of rlg_ppo_loss_fused the launch evaluates the loss of its own row tile in front of its prologue -
   * no separate loss launch - i.e. it first writes d mu / d values (which must be views of d_out), the mu/sigma
   * write-back and one row of partials per workgroup (rlg_mlp_chain_num_blocks(rows, resolved backward groups) rows of
   * rlg_ppo_loss_partials_per_block doubles).  minibatch must equal rows.  The step entries require it. */
  const rlg_ppo_loss_desc* ppo_loss_or_null;
  const void* weight_form_or_null;  /* rlg_mlp_chain_backward: backward planes (the 64-row split kernel runs when it applies
                                     * and H / dZ are 16-byte aligned); the lean entries: backward fragments, required */
  /* Gradient maxima for the weight-gradient launch (rlg_mlp_dw_desc): a split-fp16 launch leaves per workgroup the
   * largest magnitude of dZ of layer l (the last layer: of the d heads it read) in maxima[l * maxima_stride + workgroup],
   * plain stores.  The 64-row split kernel of rlg_mlp_chain_backward: one entry per 64 rows, maxima it cannot use (another
   * kernel runs, stride < ceil(rows / 64)) are ignored.  The lean entries: one entry per 16 rows, stride < ceil(rows / 16)
   * is hipErrorInvalidValue.  rlg_mlp_chain_step leaves none. */
  float* maxima_or_null;
  int maxima_stride;
  int* maxima_rows_out_or_null;     /* host int: the rows one entry covers, 64 or 16; 0 = this launch leaves no maxima */
} rlg_chain_bwd;
RLG_ABI_SIZE(rlg_chain_bwd, 96);

typedef struct rlg_chain_launch {
  long long rows;                   /* <= 0: nothing to do, 0 */
  int groups;                       /* rlg_mlp_chain_forward / _backward: 16-row groups per workgroup, 1 / 2 / 4, 0 = chosen
                                     * from rows and direction (rlg_mlp_chain_groups); the other entries run 16-row workgroups */
  void* ev_start_or_null;           /* HIP events (rlg_event_create) on THIS dispatch; not for launches inside a graph */
  void* ev_stop_or_null;            /*   capture.  bench.py's roofline_fwd / roofline_bwd */
} rlg_chain_launch;
RLG_ABI_SIZE(rlg_chain_launch, 32);

int rlg_mlp_chain_forward(const rlg_chain_net* net, const rlg_chain_fwd* fwd, const rlg_chain_launch* launch, void* stream);
int rlg_mlp_chain_backward(const rlg_chain_net* net, const rlg_chain_bwd* bwd, const rlg_chain_launch* launch, void* stream);

/* Forward + PPO loss + backward of one minibatch as ONE launch (round 4; csrc/mlp_chain.hip,
 * mlp_chain_step_pipe_kernel): rlg_mlp_chain_forward in its training form (every act_out given) and
 * rlg_mlp_chain_backward with a loss descriptor whose mu / values are the forward's heads and whose d_mu / d_values are
 * `d_out`.  For minibatches below 16,384 rows (a data-parallel rank's 4,096 - 8,192): the loss tile's inputs are
 * requested before the forward and arrive during it, and the launch boundary between the two halves is gone
 * (a2c_continuous.py:136-234: model forward, calc_losses, loss.backward() up to the weight-gradient GEMMs).  Same device
 * code as the two launches, same results.  Returns hipErrorNotSupported (801) when the shape is outside the kernel's
 * envelope - the caller then issues rlg_mlp_chain_forward and rlg_mlp_chain_backward. */
int rlg_mlp_chain_step(const rlg_chain_net* net, const rlg_chain_fwd* fwd, const rlg_chain_bwd* bwd,
                       const rlg_chain_launch* launch, void* stream);

/* The 16-row launches of a data-parallel rank's minibatches (< 16,384 rows; rollouts of that size) in their LEAN form
 * (round 4; csrc/mlp_chain_lean.hip, mlp_chain_fwd_lean_kernel / mlp_chain_bwd_lean_kernel): the weights as FRAGMENTS (round 6: two fp16 planes of 64 w per group of 32 k values where rounds 4 - 5 had two fp32 chunks - the same bytes; csrc/split_f16.hpp) in
 * the order each of the 8 waves of a workgroup consumes them - one linear stream per wave across blocks and layers, zero
 * padding instead of out-of-range selects; the backward's fragments are the transposed matrices (one 16-byte load per lane and chunk where the row-major matrix
 * needs four strided dword loads).  Same maths as rlg_mlp_chain_forward / rlg_mlp_chain_backward in their 16-row form
 * (network_builder.py:447-512 and autograd's backward of it); round 6: three fp16 plane products per fp32 product - results
 * within the split kernels' tolerance of the pipelined exact-product kernels.
 *   rlg_mlp_chain_frags_bytes: size of one direction's fragment buffer (0 forward, 1 backward), < 0: shape
 *     outside the format.
 *   rlg_mlp_chain_pack_frags / _both: weights -> fragments, one launch (the bias pointers are not read); to be repeated behind every change of
 *     the weights (an agent issues it behind its optimiser step).
 *   rlg_mlp_chain_forward_lean / rlg_mlp_chain_backward_lean: the launches; the descriptors of their namesakes, the
 *     weights read from weight_form.  hipErrorNotSupported (801): shape outside the kernels' envelope (LDS, unaligned H / dZ
 *     rows) - the caller then uses rlg_mlp_chain_forward / rlg_mlp_chain_backward. */
long long rlg_mlp_chain_frags_bytes(int num_layers, const int* in_features, const int* out_features, int direction);
int rlg_mlp_chain_pack_frags(int num_layers, const float* const* weights, const float* const* biases_or_null,
                             const int* in_features, const int* out_features, int direction, void* frags, void* stream);
int rlg_mlp_chain_pack_frags_both(int num_layers, const float* const* weights, const float* const* biases,
                                  const int* in_features, const int* out_features, void* frags_fwd, void* frags_bwd_or_null,
                                  void* stream);
int rlg_mlp_chain_forward_lean(const rlg_chain_net* net, const rlg_chain_fwd* fwd, const rlg_chain_launch* launch, void* stream);
/* forward + PPO loss + backward in ONE lean launch (rlg_mlp_chain_step on the fragments; minibatches of at most
 * 16 rows x CUs; 801 otherwise) */
int rlg_mlp_chain_step_lean(const rlg_chain_net* net, const rlg_chain_fwd* fwd, const rlg_chain_bwd* bwd,
                            const rlg_chain_launch* launch, void* stream);
int rlg_mlp_chain_backward_lean(const rlg_chain_net* net, const rlg_chain_bwd* bwd, const rlg_chain_launch* launch, void* stream);

/* Split-product form of the chain (csrc/mlp_chain_bx.hip): every fp32 product as three exact fp16 plane products on
 * v_mfma_f32_16x16x32_f16 (round 6, csrc/split_f16.hpp: results within 3 * 2^-22 |x||w| per product of the exact-product
 * kernels in the worst case, ~2^-24 rms).  The weights
 * are split ONCE per optimizer step into plane fragments; the launch that is given them (weight_form_or_null of
 * rlg_mlp_chain_backward, direction 1) uses the split kernel when rlg_mlp_chain_bx_supported says so and the
 * activation arrays are 16-byte aligned, else the exact-product kernel.  Same autograd nodes as above
 * (rl_games/algos_torch/network_builder.py:447-512).
 * pack_backward_planes_or_null of rlg_chain_fwd: the forward launch of a training step splits the weights
 * for the backward launch that follows it (same weights) in extra workgroups at the end of its grid - no launch of its own.
 *   rlg_mlp_chain_planes_bytes : size of the fragment buffer for one direction (0 forward products, 1 backward) or,
 *                                direction 2, of ONE buffer with both (the backward fragments at
 *                                rlg_mlp_chain_planes_offset(..., 1))
 *   rlg_mlp_chain_pack_planes  : weights [out, in] fp32 -> fragments (one launch, all layers; direction 2: both
 *                                directions into the combined buffer - networks of up to 4 layers) */
long long rlg_mlp_chain_planes_bytes(int num_layers, const int* in_features, const int* out_features, int direction);
long long rlg_mlp_chain_planes_offset(int num_layers, const int* in_features, const int* out_features, int direction);
int rlg_mlp_chain_pack_planes(int num_layers, const float* const* weights, const int* in_features,
                              const int* out_features, int direction, void* planes, void* stream);
int rlg_mlp_chain_bx_supported(int num_layers, const int* in_features, const int* out_features, long long rows,
                               int groups, int direction);

/* ---- recurrent policy (BASELINE config #5) -------------------------------------------------
 * Sequence-persistent LSTM layer: replaces the per-timestep torch.nn.LSTM calls + done-state
 * resets of rl_games/common/layers/recurrent.py:26-58 (LSTMWithDones) as used by A2CBuilder
 * (rl_games/algos_torch/network_builder.py:447-512, rnn after the MLP) and autograd's BPTT.
 * gates [S*T, 4H] (row = seq*T + t) holds x_t W_ih^T + b_ih + b_hh on entry and the activated
 * gates (i, f, g, o) on exit; the state entering step t is zeroed where dones[seq*T+t] != 0.
 * rlg_lstm_supported(hidden): 1 for 16, 32, 64 and 128, else 0.  The recurrent weights are fetched once per launch and
 * stay on the CU for all T steps: W_hh [4H, H] in LDS as fp32 up to 64 units (64 KB; csrc/lstm.hip), at 128 units
 * (256 KB, more than a CU's 160 KB of LDS) in the registers of a 1,024-thread workgroup as operand fragments of
 * v_mfma_f32_16x16x4_f32 (csrc/lstm_wide.hip; w_hh must then be 16-byte aligned).  256 units and more (>= 1 MB) fit
 * neither a CU's 512 KB register file nor registers + LDS together, and other widths have no instantiation: the entry
 * points return hipErrorInvalidValue for them. */
int rlg_lstm_supported(int hidden);

/* The four sequence entries (LSTM / GRU, forward / backward) take an array of one or two problem descriptors and the
 * shape the problems share: num_seqs, seq_len, hidden.  The descriptors hold one problem's pointers and are read before
 * the entry returns; a field named *_or_null below (in the comments) may be NULL, every other one is required.
 * num_problems 1: one launch of the single kernel on ceil(S / tile) workgroups.
 * num_problems 2: a paired launch of two problems A = problems[0] and B = problems[1] of ONE shape (cell, hidden,
 * num_seqs, seq_len) that do not depend on each other - the actor's and the critic's recurrence of a `separate: True`
 * network, each with its own RNN (network_builder.py:272-277, :372-421).  The grid has ceil(S / tile) x 2 workgroups:
 * row 0 runs problem A, row 1 problem B, each workgroup the code of the single kernel, the tile chosen from ONE problem's
 * num_seqs exactly as for one problem.  Every output is therefore bit-identical to what the two single launches write
 * (csrc/rnn_seq.hpp, "paired launches").  An optional output may be given for one problem and NULL for the other.
 * hipErrorInvalidValue, before the runtime is asked for anything and with nothing launched, in this order: a NULL
 * problems or a num_problems other than 1 or 2 (answered first); num_seqs <= 0, seq_len <= 0 or a width other than
 * 16 / 32 / 64 / 128; a NULL required pointer in any problem; with two problems an output buffer of A - gates, out,
 * c_all / hn_all, hprev, hT, cT; d_gates; d_gx, d_gh - that is also the same-named buffer of B; at 128 units a w_hh of
 * any problem that is not 16-byte aligned (not rlg_lstm_seq_backward, whose kernel loads w_hh one float at a time). */
typedef struct rlg_lstm_fwd {
  float* gates;                     /* [S*T, 4H]: gate inputs on entry, activated gates on exit */
  const float* w_hh;                /* [4H, H] */
  const float* h0;                  /* [S, H] */
  const float* c0;                  /* [S, H] */
  const unsigned char* dones;       /* _or_null: [S*T]; NULL: no resets */
  float* out;                       /* [S*T, H]: h_t */
  float* c_all;                     /* _or_null: [S*T, H]: c_t, for the backward */
  float* hprev;                     /* _or_null: [S*T, H]: the state entering each step after the reset (dW_hh) */
  float* hT;                        /* _or_null: [S, H]: h after the last step */
  float* cT;                        /* _or_null: [S, H]: c after the last step */
} rlg_lstm_fwd;
RLG_ABI_SIZE(rlg_lstm_fwd, 80);
int rlg_lstm_seq_forward(const rlg_lstm_fwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                         void* stream);

/* d_gates [S*T, 4H] = d loss / d gate pre-activations given d_out = d loss / d h_t. */
typedef struct rlg_lstm_bwd {
  const float* gates;               /* the forward's activated gates, c_all and c0 */
  const float* c_all;
  const float* c0;
  const unsigned char* dones;       /* _or_null */
  const float* w_hh;
  const float* d_out;               /* [S*T, H] */
  float* d_gates;
} rlg_lstm_bwd;
RLG_ABI_SIZE(rlg_lstm_bwd, 56);
int rlg_lstm_seq_backward(const rlg_lstm_bwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                          void* stream);

/* Sequence-persistent GRU layer: the same position in the network and the same contract (rows seq*T + t, done rule,
 * one launch for all T steps, weights fetched once per launch) for `rnn: {name: gru, layers: 1}`
 * (rl_games/common/layers/recurrent.py GRUWithDones, network_builder.py:250-276).  The cell is torch.nn.GRU's, gate
 * order (r, z, n):
 *   r = sigmoid(gx_r + W_hr h + b_hr)   z = sigmoid(gx_z + W_hz h + b_hz)
 *   hn = W_hn h + b_hn                  n = tanh(gx_n + r * hn)              h' = (1 - z) * n + z * h
 * gates [S*T, 3H] holds gx = x_t W_ih^T + b_ih on entry and the activated (r, z, n) on exit.  b_hn sits inside the
 * product with r and cannot be folded into the input side, so b_hh [3H] is an argument of its own.
 * For training the forward keeps hn_all [S*T, H] (hn, before the gating by r) and hprev [S*T, H] (the state entering
 * each step after the reset); for inference hT [S, H].
 * rlg_gru_supported(hidden): 1 for 16, 32, 64 and 128, else 0.  W_hh [3H, H] in LDS as fp32 up to 64 units (48 KB;
 * csrc/gru.hip); at 128 units (192 KB, more than a CU's 160 KB of LDS) in the registers of a 1,024-thread workgroup as
 * operand fragments of v_mfma_f32_16x16x4_f32 (csrc/gru_wide.hip; w_hh must then be 16-byte aligned).  Other widths:
 * hipErrorInvalidValue. */
int rlg_gru_supported(int hidden);
typedef struct rlg_gru_fwd {
  float* gates;                     /* [S*T, 3H]: gx on entry, activated (r, z, n) on exit */
  const float* w_hh;                /* [3H, H] */
  const float* b_hh;                /* [3H] */
  const float* h0;                  /* [S, H] */
  const unsigned char* dones;       /* _or_null */
  float* out;                       /* [S*T, H]: h_t */
  float* hn_all;                    /* _or_null */
  float* hprev;                     /* _or_null */
  float* hT;                        /* _or_null: [S, H]: h after the last step */
} rlg_gru_fwd;
RLG_ABI_SIZE(rlg_gru_fwd, 72);
int rlg_gru_seq_forward(const rlg_gru_fwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                        void* stream);

/* Given d_out = d loss / d h_t:  d_gx [S*T, 3H] = (dr_pre, dz_pre, dn_pre), the gradient of the input side (dW_ih,
 * db_ih, the trunk's dX), and d_gh [S*T, 3H] = (dr_pre, dz_pre, dn_pre * r), the gradient of the hidden side
 * (dW_hh = d_gh^T hprev, db_hh). */
typedef struct rlg_gru_bwd {
  const float* gates;               /* the forward's activated gates, hn_all and hprev */
  const float* hn_all;
  const float* hprev;
  const unsigned char* dones;       /* _or_null */
  const float* w_hh;
  const float* d_out;               /* [S*T, H] */
  float* d_gx;
  float* d_gh;
} rlg_gru_bwd;
RLG_ABI_SIZE(rlg_gru_bwd, 64);
int rlg_gru_seq_backward(const rlg_gru_bwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                         void* stream);

/* Layer normalisation behind the recurrent layer (csrc/rnn_layer_norm.hip): `rnn: {layer_norm: True}`,
 * nn.LayerNorm(rnn_units) over the RNN output [rows, hidden] (network_builder.py:447-500), hidden 16 / 32 / 64 / 128.
 *   forward:  y = (x - mean) * rstd * gamma + beta, biased variance from the centred values, rstd = 1 / sqrt(var + eps);
 *             stats_or_null [rows, 2] fp32 receives (mean, rstd) per row for the backward (NULL: inference).
 *   backward: g = d_y * gamma, xh = (x - mean) * rstd:  d_x = rstd * (g - mean_H(g) - xh * mean_H(g * xh));
 *             d_gamma_partials / d_beta_partials [num_blocks][hidden] fp64: per-workgroup column sums of d_y * xh and
 *             d_y, the layout rlg_act_bwd_colsum writes - finished by rlg_colsum_finalize or rlg_mlp_dw_launch's colsums.
 *             num_blocks: rlg_rnn_layer_norm_num_blocks(rows, hidden) (0 for an unsupported width or rows <= 0).
 * x, y, d_y, d_x contiguous and 16-byte aligned.  A row's result depends on the row alone (fixed summation order).
 * Unsupported widths, rows <= 0, NULL or misaligned pointers: hipErrorInvalidValue, nothing is launched. */
int rlg_rnn_layer_norm_num_blocks(long long rows, int hidden);
int rlg_rnn_layer_norm_forward(const float* x, const float* gamma, const float* beta, float eps, float* y,
                               float* stats_or_null, long long rows, int hidden, void* stream);
int rlg_rnn_layer_norm_backward(const float* d_y, const float* x, const float* stats, const float* gamma, float* d_x,
                                double* d_gamma_partials, double* d_beta_partials, int num_blocks, long long rows,
                                int hidden, void* stream);

/* Value head + clipped value loss + its backward behind the recurrent layer of a central value critic
 * (csrc/rnn_value_tail.hip): one value column over the RNN (or layer-normed) features feat [rows, hidden], hidden
 * 16 / 32 / 64 / 128, as in the reference's recurrent SMAC critics (central_value.py:262-335).
 *   values[r] = b + sum_k feat[r,k] w[k], products and sum in fp64, rounded to fp32 once; w [hidden], b [1].
 *   rlg_rnn_value_head: the values alone (a rollout step, get_value) - the same bits as the training form.
 *   rlg_rnn_value_tail: also the row loss and gradient of rlg_value_loss (the same device function) -> d_values [rows],
 *     d_feat[r,k] = d_values[r] w[k], and per workgroup in fp64: loss_partials [num_blocks][7] in rlg_value_loss's
 *     slots (for rlg_ppo_loss_finalize with actions_num 0), d_w_partials [num_blocks][hidden] = sum_r d_values[r]
 *     feat[r,k] and d_b_partials [num_blocks][1] = sum_r d_values[r], the layout rlg_act_bwd_colsum writes - finished by
 *     rlg_colsum_finalize or rlg_mlp_dw_launch's colsums.  num_blocks: rlg_rnn_value_tail_num_blocks(rows, hidden)
 *     (0 for an unsupported width or rows <= 0).
 * feat, d_feat contiguous and 16-byte aligned.  A row's result depends on the row alone (fixed summation order).
 * Unsupported widths, rows <= 0, a mask without its sum, NULL or misaligned pointers: hipErrorInvalidValue, nothing is
 * launched. */
int rlg_rnn_value_tail_num_blocks(long long rows, int hidden);
int rlg_rnn_value_head(const float* feat, const float* w, const float* b, float* values, long long rows, int hidden,
                       void* stream);
int rlg_rnn_value_tail(const float* feat, const float* w, const float* b, const float* old_values,
                       const float* returns, const float* mask_or_null, const float* mask_sum_or_null, float* values,
                       float* d_values, float* d_feat, double* loss_partials, double* d_w_partials,
                       double* d_b_partials, int num_blocks, long long rows, int hidden, float e_clip, int clip_value,
                       void* stream);

/* ---- products too narrow for the MFMA kernels (csrc/mlp_narrow.hip; BASELINE config #5: obs 3, act 1) ----------
 * rlg_narrow_dx: dX [rows, in] = dZ [rows, out] W [out, in] for out <= 8 - autograd's grad_output.mm(weight) of the fused
 *   (value | mu) head (rl_games/algos_torch/network_builder.py:295-311, :506-512).
 * rlg_narrow_dw: grad [out, in] = dZ^T X for in <= 8, out <= 256 - grad_output.t().mm(input) of actor_mlp's first
 *   nn.Linear over a few observations (network_builder.py:118-147); partials: rlg_narrow_dw_blocks(rows) * out * in
 *   doubles of scratch (fp64 partial sums per workgroup, combined in a fixed order). */
int rlg_narrow_dx(const float* dz, long long lddz, const float* w, float* dx, long long lddx, long long rows,
                  int out_features, int in_features, void* stream);
int rlg_narrow_dw_blocks(long long rows);
int rlg_narrow_dw(const float* dz, long long lddz, const float* x, long long ldx, float* grad, double* partials,
                  long long rows, int out_features, int in_features, void* stream);

/* ------------------------------------------------------------------------------------
 * In-graph gradient all-reduce over peer-mapped device memory (csrc/ipc_allreduce.hip)
 *   replaces dist.all_reduce(SUM) of the flattened gradients in A2CBase.trancate_gradients_and_step
 *   (rl_games/common/a2c_common.py:493-509) and of the minibatch KL (:1559-1560, carried in a tail
 *   slot of the same arena).  One process per GPU: rlg_ipc_comm_create allocates the rank's staging
 *   memory and returns its hipIpcMemHandle_t (rlg_ipc_handle_bytes() bytes); the host exchanges the
 *   handles (any channel), rlg_ipc_comm_connect maps the peers; rlg_ipc_allreduce_sum is then ONE
 *   kernel launch (no host sync, capturable in a HIP graph) that leaves the identical rank-ordered
 *   sum in `data` on every rank.  The wait for the peers is bounded by wall time (default 600 s,
 *   RLG_IPC_TIMEOUT_S / rlg_ipc_comm_set_timeout; <= 0 = unbounded).  A launch that gives up, and every
 *   launch after it, is fail-safe: zeros instead of a sum of stale data in `data`, the sticky error word
 *   (rlg_ipc_comm_error_word) set - rlg_adam_step takes that word as its skip flag, so no parameter is
 *   touched by invalid gradients - and rlg_ipc_comm_status reports the launch ordinal.
 *   rlg_ipc_comm_create fails (the caller then uses RCCL) when the runtime has no fine-grained device
 *   memory: the protocol needs mid-kernel visibility across devices.
 *   Variant 1 (rlg_ipc_comm_set_variant / RLG_IPC_TWO_PHASE): reduce-scatter + all-gather - 2/P of the
 *   bytes per xGMI link, two synchronisations; same bits as the one-shot variant.
 * ---------------------------------------------------------------------------------- */
int rlg_ipc_handle_bytes(void);
int rlg_ipc_comm_create(int rank, int world, long long max_floats, void** comm_out, void* handle_out);
int rlg_ipc_comm_connect(void* comm, const void* all_handles /* world x handle bytes, rank-major */);
int rlg_ipc_comm_fine_grained(void* comm);
int rlg_ipc_comm_set_timeout(void* comm, double seconds);
int rlg_ipc_comm_set_variant(void* comm, int two_phase);
/* the settings in effect, environment defaults (RLG_IPC_TWO_PHASE, RLG_IPC_TIMEOUT_S) included; timeout 0 = unbounded.
 * Every rank must run the same variant: the host compares these across ranks before the first launch. */
int rlg_ipc_comm_get_config(void* comm, int* two_phase_out, double* timeout_s_out);
int rlg_ipc_comm_error_word(void* comm, unsigned** word_out);
int rlg_ipc_allreduce_sum(void* comm, float* data, long long n, void* stream);
/* The same launch with a by-product: norm_partials[rlg_ipc_allreduce_norm_blocks()] = per-workgroup sums of
 * (reduced x * grad_scale)^2 over the first norm_n elements (the gradients; the arena's tail slots are not),
 * and *step_counter += 1 - what rlg_grad_sumsq would compute in a launch of its own after the collective
 * (clip_grad_norm_ of the averaged gradients, a2c_common.py:498-512). */
int rlg_ipc_allreduce_norm_blocks(void);
int rlg_ipc_allreduce_sum_norm(void* comm, float* data, long long n, double* norm_partials, long long norm_n,
                               float grad_scale, long long* step_counter_or_null, void* stream);
int rlg_ipc_comm_status(void* comm, unsigned* launches_out, unsigned* timed_out_launch_out);
int rlg_ipc_comm_destroy(void* comm);

/* ---- RCCL behind the C ABI (csrc/rccl_wrap.hip) ---------------------------------------------------
 * "plus an RCCL wrapper taking ncclComm_t".  The gradient all-reduce of
 * A2CBase.trancate_gradients_and_step (rl_games/common/a2c_common.py:493-509) as a launch on the caller's stream
 * - capturable into the mini-epoch HIP graph, unlike a collective issued through torch.distributed - for nodes on
 * which the hipIpc kernel (rlg_ipc_*) is not available.  `comm` is an ncclComm_t; the unique id (rlg_rccl_unique_id_bytes()
 * bytes, from rank 0's rlg_rccl_get_unique_id) travels through whatever channel the ranks share.  librccl is resolved
 * with dlopen at first use: rlg_rccl_available() == 0 and hipErrorNotSupported from the others when there is none.
 * Every rank receives the same bits; in place. */
int rlg_rccl_available(void);
int rlg_rccl_unique_id_bytes(void);
int rlg_rccl_get_unique_id(void* id_out);
int rlg_rccl_comm_create(const void* unique_id, int rank, int world, void** comm_out /* ncclComm_t */);
int rlg_rccl_allreduce_sum(void* comm /* ncclComm_t */, float* data, long long n, void* stream);
int rlg_rccl_allreduce_sum_f64(void* comm /* ncclComm_t */, double* data, long long n, void* stream);
int rlg_rccl_comm_destroy(void* comm /* ncclComm_t */);

#ifdef __cplusplus
}
#endif

#endif /* RLG_HIP_H_ */
