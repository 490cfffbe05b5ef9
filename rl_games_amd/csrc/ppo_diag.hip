// PPO diagnostics (`use_diagnostics`, rl_games/common/diagnostics.py): the clip fraction of the step's probability
// ratio and the moments behind the explained variance of the value targets, reduced on the device into fp64 rows of a
// table that the host reads once per epoch.  Two launches:
//
// ppo_diag_clip_kernel - one per minibatch, inside the update (and its captured graphs), in front of the optimiser step.
// Per row i (weight m_i = mask[i], or 1 without a mask):
//   new_nlp   given (discrete loss output, torch forms), or recomputed from the written-back mu, the pre-step logstd and
//             the actions with the loss tile's arithmetic (ppo_loss_tile.hpp, ppo_loss_row):
//               z = (x - mu) / expf(logstd) ;  nlp = (0.5 * fp32(sum_f64 z^2) + fp32(0.9189385332046727 A)) + fp32(sum_f64 logstd)
//   logratio  = old_nlp - new_nlp (fp32); clipped when logratio < log_lo or logratio > log_hi     (torch_ext.py:217-227)
// and writes columns 0..2 of the minibatch's row: rows, sum m, sum m*clipped.
//
// ppo_diag_moments_kernel - once per mini-epoch, outside the update: the old values and returns do not change while
// the dataset is trained on, so one launch covers every minibatch slice of the dataset (blockIdx.y = slice) and writes
// columns 3..9 of each slice's row: (mean, M2 = sum m (x - mean)^2) of returns, values and d = returns - values (fp32)
// over the slice's rows x value columns with element weights m(row), and the element count.  Centred moments: a
// weighted Welford pass per thread, Chan merges in a fixed tree.
//
// Both: every workgroup writes its partial row, the last to arrive (ticket, reset by the same launch so that a replayed
// graph finds it at 0) folds them in index order and writes the output - written, not accumulated: replays are
// idempotent, and no float atomics: the rows are bit-reproducible.
#include "rlg_device.hpp"
#include "../../include/rlg_hip.h"

namespace rlg {

constexpr int kDiagThreads = 256;
constexpr int kDiagMaxBlocks = 256;   // <= kDiagThreads: the last workgroup loads one partial per thread
constexpr int kDiagStats = 10;
enum DiagStat { kRows = 0, kWeight, kClipped, kMeanRet, kM2Ret, kMeanVal, kM2Val, kMeanDiff, kM2Diff, kElements };
constexpr int kClipStats = 3;          // columns kRows .. kClipped
constexpr int kMomentStats = 9;        // element count, element weight, (unused), then the three (mean, M2) pairs

struct DiagClipArgs {
  const float* mu;           // [mb, A], row stride ld_mu (recompute form) ...
  long long ld_mu;
  const float* logstd;       // [A]
  const float* actions;      // [mb, A], row stride ld_actions
  long long ld_actions;
  const float* new_neglogp;  // ... or [mb] (given form; mu / logstd / actions unused)
  const float* old_neglogp;  // [mb]
  const float* mask;         // [mb] or nullptr
  float* nlp_out;            // [mb] or nullptr: the new neglogp each row used
  double* partials;          // [gridDim.x][kClipStats]
  unsigned int* ticket;
  double* out;               // [kDiagStats]: columns 0..2 written
  int mb, A;
  float log_lo, log_hi;
};

__global__ __launch_bounds__(kDiagThreads) void ppo_diag_clip_kernel(DiagClipArgs p) {
  __shared__ float s_sigma[32], s_logstd[32];
  __shared__ double scratch[kClipStats * (kDiagThreads / kWave)];
  __shared__ bool last;
  const bool recompute = p.new_neglogp == nullptr;
  if (recompute && threadIdx.x < p.A) {
    const float ls = p.logstd[threadIdx.x];
    s_logstd[threadIdx.x] = ls;
    s_sigma[threadIdx.x] = expf(ls);                                       // models.py:296, the loss tile's bits
  }
  __syncthreads();
  double v[kClipStats] = {0.0, 0.0, 0.0};
  const long long stride = static_cast<long long>(gridDim.x) * kDiagThreads;
  for (long long i = static_cast<long long>(blockIdx.x) * kDiagThreads + threadIdx.x; i < p.mb; i += stride) {
    float nlp;
    if (recompute) {
      double z2 = 0.0, ls_sum = 0.0;
      const float* mu = p.mu + i * p.ld_mu;
      const float* x = p.actions + i * p.ld_actions;
      for (int a = 0; a < p.A; ++a) {
        const float z = (x[a] - mu[a]) / s_sigma[a];
        z2 += static_cast<double>(z * z);
        ls_sum += static_cast<double>(s_logstd[a]);
      }
      nlp = (0.5f * static_cast<float>(z2) + static_cast<float>(0.9189385332046727 * p.A)) + static_cast<float>(ls_sum);
    } else {
      nlp = p.new_neglogp[i];
    }
    if (p.nlp_out) p.nlp_out[i] = nlp;
    const float logratio = p.old_neglogp[i] - nlp;
    const bool clipped = (logratio < p.log_lo) || (logratio > p.log_hi);
    const double m = p.mask ? static_cast<double>(p.mask[i]) : 1.0;
    v[0] += 1.0;
    v[1] += m;
    v[2] += clipped ? m : 0.0;
  }
  block_sum<kClipStats, kDiagThreads>(v, scratch);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kClipStats; ++k) p.partials[blockIdx.x * kClipStats + k] = v[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    last = atomicAdd(p.ticket, 1u) == gridDim.x - 1u;
  }
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
  for (int k = 0; k < kClipStats; ++k)
    v[k] = threadIdx.x < gridDim.x ? __builtin_nontemporal_load(p.partials + threadIdx.x * kClipStats + k) : 0.0;
  block_sum<kClipStats, kDiagThreads>(v, scratch);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kClipStats; ++k) p.out[k] = v[k];
    *p.ticket = 0u;
  }
}

struct DiagMomentArgs {
  const float* values;       // [slices * rows, cols]
  const float* returns;      // [slices * rows, cols]
  const float* mask;         // [slices * rows] or nullptr
  double* partials;          // [slices][gridDim.x][kMomentStats]
  unsigned int* tickets;     // [slices]
  double* out;               // slice s: out + s * ld_out, columns kMeanRet .. kElements written
  long long ld_out;
  int rows, cols;
};

struct MomentAcc {
  double v[kMomentStats];    // element count, weight, (unused), mean_r, M2_r, mean_v, M2_v, mean_d, M2_d
};

// weighted Welford step of one (mean, M2) pair; w_new = total weight including this element (> 0)
__device__ __forceinline__ void welford(double& mean, double& m2, double x, double m, double w_new) {
  const double delta = x - mean;
  mean += delta * (m / w_new);
  m2 += m * delta * (x - mean);
}

// a <- a (+) b: counts add, (mean, M2) pairs merge by weight (Chan et al.)
__device__ __forceinline__ void moment_merge(MomentAcc& a, const MomentAcc& b) {
  const double wa = a.v[1], wb = b.v[1], w = wa + wb;
  a.v[0] += b.v[0];
  if (w > 0.0) {
    const double fb = wb / w, cross = wa * wb / w;
#pragma unroll
    for (int k = 3; k < kMomentStats; k += 2) {
      const double delta = b.v[k] - a.v[k];
      a.v[k] = a.v[k] + delta * fb;
      a.v[k + 1] = (a.v[k + 1] + b.v[k + 1]) + delta * delta * cross;
    }
  }
  a.v[1] = w;
}

// fixed-order tree over the block's threads (stride halving); result in thread 0
__device__ __forceinline__ void moment_block_fold(MomentAcc& s, double* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kMomentStats; ++k) lds[k * kDiagThreads + tid] = s.v[k];
  __syncthreads();
  for (int half = kDiagThreads / 2; half > 0; half >>= 1) {
    if (tid < half) {
      MomentAcc o;
#pragma unroll
      for (int k = 0; k < kMomentStats; ++k) o.v[k] = lds[k * kDiagThreads + tid + half];
      moment_merge(s, o);
#pragma unroll
      for (int k = 0; k < kMomentStats; ++k) lds[k * kDiagThreads + tid] = s.v[k];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kDiagThreads) void ppo_diag_moments_kernel(DiagMomentArgs p) {
  __shared__ double lds[kMomentStats * kDiagThreads];
  __shared__ bool last;
  const int slice = blockIdx.y;
  const long long n = static_cast<long long>(p.rows) * p.cols;
  const float* vals = p.values + slice * n;
  const float* rets = p.returns + slice * n;
  const float* mask = p.mask ? p.mask + static_cast<long long>(slice) * p.rows : nullptr;
  MomentAcc s;
#pragma unroll
  for (int k = 0; k < kMomentStats; ++k) s.v[k] = 0.0;
  const long long stride = static_cast<long long>(gridDim.x) * kDiagThreads;
  for (long long e = static_cast<long long>(blockIdx.x) * kDiagThreads + threadIdx.x; e < n; e += stride) {
    const float r = rets[e], v = vals[e];
    const float d = r - v;
    const double m = mask ? static_cast<double>(mask[e / p.cols]) : 1.0;
    s.v[0] += 1.0;
    if (m != 0.0) {
      const double w = s.v[1] + m;
      s.v[1] = w;
      welford(s.v[3], s.v[4], r, m, w);
      welford(s.v[5], s.v[6], v, m, w);
      welford(s.v[7], s.v[8], d, m, w);
    }
  }
  moment_block_fold(s, lds);
  double* part = p.partials + static_cast<long long>(slice) * gridDim.x * kMomentStats;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kMomentStats; ++k) part[blockIdx.x * kMomentStats + k] = s.v[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    last = atomicAdd(p.tickets + slice, 1u) == gridDim.x - 1u;
  }
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
  for (int k = 0; k < kMomentStats; ++k)
    s.v[k] = threadIdx.x < gridDim.x ? __builtin_nontemporal_load(part + threadIdx.x * kMomentStats + k) : 0.0;
  moment_block_fold(s, lds);
  if (threadIdx.x == 0) {
    double* o = p.out + slice * p.ld_out;
#pragma unroll
    for (int k = 3; k < kMomentStats; ++k) o[k] = s.v[k];        // kMeanRet .. kM2Diff
    o[kElements] = s.v[0];
    p.tickets[slice] = 0u;
  }
}

}  // namespace rlg

extern "C" {

int rlg_ppo_diag_stats(void) { return rlg::kDiagStats; }

static int diag_blocks(long long n) {
  const long long b = (n + rlg::kDiagThreads - 1) / rlg::kDiagThreads;
  return static_cast<int>(b < 1 ? 1 : (b > rlg::kDiagMaxBlocks ? rlg::kDiagMaxBlocks : b));
}

int rlg_ppo_diag_num_blocks(int minibatch) { return diag_blocks(minibatch); }

int rlg_ppo_diag(const float* mu, long long ld_mu, const float* logstd, const float* actions, long long ld_actions,
                 const float* new_neglogp_or_null, const float* old_neglogp, const float* mask_or_null, int minibatch,
                 int actions_num, float log_lo, float log_hi, double* partials, unsigned int* ticket, double* out,
                 float* neglogp_out_or_null, void* stream) {
  using namespace rlg;
  if (minibatch <= 0 || !old_neglogp || !partials || !ticket || !out) return static_cast<int>(hipErrorInvalidValue);
  if (!new_neglogp_or_null) {
    if (!mu || !logstd || !actions || actions_num <= 0 || actions_num > 32 || ld_mu < actions_num ||
        ld_actions < actions_num)
      return static_cast<int>(hipErrorInvalidValue);
  }
  DiagClipArgs p;
  p.mu = mu;
  p.ld_mu = ld_mu;
  p.logstd = logstd;
  p.actions = actions;
  p.ld_actions = ld_actions;
  p.new_neglogp = new_neglogp_or_null;
  p.old_neglogp = old_neglogp;
  p.mask = mask_or_null;
  p.nlp_out = neglogp_out_or_null;
  p.partials = partials;
  p.ticket = ticket;
  p.out = out;
  p.mb = minibatch;
  p.A = new_neglogp_or_null ? 0 : actions_num;
  p.log_lo = log_lo;
  p.log_hi = log_hi;
  hipLaunchKernelGGL(ppo_diag_clip_kernel, dim3(diag_blocks(minibatch)), dim3(kDiagThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_ppo_diag_moments_num_blocks(int rows, int cols) {
  return diag_blocks(static_cast<long long>(rows) * cols);
}

int rlg_ppo_diag_moments(const float* values, const float* returns, const float* mask_or_null, int slices, int rows,
                         int cols, double* partials, unsigned int* tickets, double* out, long long ld_out,
                         void* stream) {
  using namespace rlg;
  if (slices <= 0 || slices > 65535 || rows <= 0 || cols <= 0 || !values || !returns || !partials || !tickets || !out ||
      ld_out < kDiagStats)
    return static_cast<int>(hipErrorInvalidValue);
  DiagMomentArgs p;
  p.values = values;
  p.returns = returns;
  p.mask = mask_or_null;
  p.partials = partials;
  p.tickets = tickets;
  p.out = out;
  p.ld_out = ld_out;
  p.rows = rows;
  p.cols = cols;
  hipLaunchKernelGGL(ppo_diag_moments_kernel, dim3(diag_blocks(static_cast<long long>(rows) * cols), slices),
                     dim3(kDiagThreads), 0, static_cast<hipStream_t>(stream), p);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
