// Row functions of the categorical heads (csrc/rollout_categorical.hip: the rollout's sampling head; csrc/play.hip: the
// players' head): the description of a [N, sum(sizes)] logits view with its masks and Exp(1) draws, the masked logit, one
// branch of one row in both forms (from an LDS tile, one thread per branch; across a wave, one wave per row), sampled or
// arg-max.  Per row and branch b of sizes[b] columns:
//   x     = mask ? logit : -1e8                                   (CategoricalMasked; no mask: the logits)
//   norm  = x - (log(sum exp(x - m)) + m),  m = max x (0 if inf)  (Categorical.__init__: logits - logsumexp)
//   p     = exp(norm - max norm) / sum exp(norm - max norm)       (Categorical.probs = softmax(norm))
//   a     = argmax p / q,  q ~ Exp(1) from the caller, lowest index on ties  (multinomial's one-sample path)
// Every op is one fp32 op rounded on its own (-ffp-contract=off, expf / logf, no fast-math intrinsics), and the two
// exp sums are added in the order of torch's kernels for branches of < 128 actions: norm and p are torch's bits
// there (wider branches: the logsumexp sum in another order, last-bit differences).
#pragma once

#include "rlg_device.hpp"

namespace rlg {

constexpr int kMaxBranches = 16;
constexpr int kCatTileRows = 64;        // rows (and threads: one wave) per workgroup of the tile form
constexpr int kCatTileMaxStride = 64;   // the tile form's LDS row stride limit (floats): 2 tiles of 64 x 64 = 32 KiB
constexpr int kCatWaveBlock = 256;      // wave form: 4 rows per workgroup

struct CategoricalRows {
  const float* logits;      // [N, ld_logits], columns 0 .. S-1
  const float* noise;       // branch-major blocks: block b = [N, size[b]] contiguous at N * off[b]
  const uint8_t* masks;     // [N, ld_masks] bool, or nullptr
  long long ld_logits, ld_masks;
  int N, B, S;
  int pow2;                 // next power of two >= the widest branch
  int size[kMaxBranches];
  int off[kMaxBranches];    // first column of each branch
};

__device__ __forceinline__ float masked_logit(const CategoricalRows& p, long long row, int col) {
  const float l = p.logits[row * p.ld_logits + col];
  return (p.masks && !p.masks[row * p.ld_masks + col]) ? -1e8f : l;
}

__device__ __forceinline__ int last_pow2(int n) { return 1 << (31 - __builtin_clz(n)); }
__device__ __forceinline__ int next_pow2(int n) { return n == 1 ? 1 : 1 << (32 - __builtin_clz(n - 1)); }

// The tile form's staging: the masked logits of rows env0 .. env0 + rows - 1 into sx and (sq given) their draws into
// sq, both [kCatTileRows][ld], with consecutive threads on consecutive addresses.  The caller synchronises.
__device__ __forceinline__ void stage_categorical_tile(const CategoricalRows& p, int env0, int rows, int ld, float* sx,
                                                       float* sq) {
  const int t = threadIdx.x, S = p.S;
  for (int i = t; i < rows * S; i += kCatTileRows) {
    const int r = i / S;
    const int c = i - r * S;
    sx[r * ld + c] = masked_logit(p, env0 + r, c);
  }
  if (!sq) return;
  for (int b = 0; b < p.B; ++b) {
    const int n = p.size[b];
    const float* gq = p.noise + static_cast<long long>(p.N) * p.off[b] + static_cast<long long>(env0) * n;
    for (int i = t; i < rows * n; i += kCatTileRows) {
      const int r = i / n;
      sq[r * ld + p.off[b] + (i - r * n)] = gq[i];
    }
  }
}

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

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float y = __shfl_xor(x, o, kWave);
    x = y > x ? y : x;
  }
  return x;
}

// One branch of one row across a wave: the branch's columns lane-strided, reduced across the 64 lanes.  Returns the
// action in every lane, *norm_out = norm[a].
__device__ __forceinline__ int categorical_branch_wave(const CategoricalRows& p, long long env, int b, int lane,
                                                       float* norm_out) {
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
  *norm_out = best_norm;
  return a;
}

// torch.argmax's order on (value, column) pairs: does (vb, b) come in front of (va, a)?  The first NaN wins, then the
// largest value, the lowest column on ties.
__device__ __forceinline__ bool argmax_before(float vb, int b, float va, int a) {
  const bool nan_a = va != va, nan_b = vb != vb;
  if (nan_a || nan_b) return nan_b && (!nan_a || b < a);
  return vb > va || (vb == va && b < a);
}

// Arg-max of one branch of one row from LDS (x = the branch's masked logits).
__device__ __forceinline__ int argmax_branch(const float* x, int n) {
  int act = 0;
  float best = x[0];
  for (int j = 1; j < n; ++j) {
    if (argmax_before(x[j], j, best, act)) {
      best = x[j];
      act = j;
    }
  }
  return act;
}

// Arg-max of one branch of one row across a wave; the action in every lane.
__device__ __forceinline__ int argmax_branch_wave(const CategoricalRows& p, long long env, int b, int lane) {
  const int n = p.size[b], c0 = p.off[b];
  float best = 0.0f;
  int a = n;                                     // n: this lane has no column yet
  for (int j = lane; j < n; j += kWave) {
    const float x = masked_logit(p, env, c0 + j);
    if (a == n || argmax_before(x, j, best, a)) {
      best = x;
      a = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float vb = __shfl_xor(best, o, kWave);
    const int ab = __shfl_xor(a, o, kWave);
    if (ab < n && (a == n || argmax_before(vb, ab, best, a))) {
      best = vb;
      a = ab;
    }
  }
  return a;
}

// Host: fills the branch table of `p` (B, S, size, off, pow2) and the views; the hipError_t of a bad description.
inline int categorical_rows_setup(CategoricalRows& p, const float* logits, long long ld_logits, const int* branch_sizes,
                                  int num_branches, const float* noise, const uint8_t* masks, long long ld_masks,
                                  int rows) {
  if (num_branches > kMaxBranches) return static_cast<int>(hipErrorNotSupported);
  if (num_branches < 1 || !branch_sizes) return static_cast<int>(hipErrorInvalidValue);
  p.B = num_branches;
  p.S = 0;
  int widest = 1;
  for (int b = 0; b < num_branches; ++b) {
    if (branch_sizes[b] < 1) return static_cast<int>(hipErrorInvalidValue);
    p.size[b] = branch_sizes[b];
    p.off[b] = p.S;
    p.S += branch_sizes[b];
    widest = branch_sizes[b] > widest ? branch_sizes[b] : widest;
  }
  for (int b = num_branches; b < kMaxBranches; ++b) p.size[b] = p.off[b] = 0;
  if (ld_logits < p.S || (masks && ld_masks < p.S)) return static_cast<int>(hipErrorInvalidValue);
  p.pow2 = 1;
  while (p.pow2 < widest) p.pow2 <<= 1;
  p.logits = logits;
  p.noise = noise;
  p.masks = masks;
  p.ld_logits = ld_logits;
  p.ld_masks = ld_masks;
  p.N = rows;
  return 0;
}

}  // namespace rlg
