// Layer normalisation behind the recurrent layer of a policy network, gfx950.
//
// `rnn: {layer_norm: True}` (rl_games/algos_torch/network_builder.py:447-500): nn.LayerNorm(rnn_units) over the RNN
// output [rows, H], H one of the widths the sequence-persistent kernels run (16 / 32 / 64 / 128, csrc/rnn_seq.hpp).
//   forward   y = (x - mean) * rstd * gamma + beta,  mean over the row, biased variance, rstd = 1 / sqrt(var + eps);
//             the mean first, then the centred sum of squares (no E[x^2] - mean^2); (mean, rstd) kept per row for
//             training as [rows, 2] fp32
//   backward  g = d_y * gamma, xh = (x - mean) * rstd:  d_x = rstd * (g - mean_H(g) - xh * mean_H(g * xh)),
//             d gamma = sum_rows d_y * xh,  d beta = sum_rows d_y  as per-workgroup fp64 column partials in the
//             [blocks][H] layout of act_bwd_colsum_kernel (csrc/mlp_fused.hip) - finished by rlg_colsum_finalize or by
//             the finalise of the weight-gradient launch like every other bias gradient.
//
// A row lives in the lanes of one wave: 16 lanes at H <= 64 (1 / 2 / 4 consecutive elements per lane), 32 lanes at
// H = 128 (4 per lane) - a wave covers 4 (2) consecutive rows per pass and reads one contiguous span.  Row sums are an
// xor butterfly over the row's lanes in fp64: the order is fixed, every lane of the row ends with the same bits, and a
// row's result depends on nothing but the row.  No atomics; LDS only to add the four waves' column partials.
// Memory-bound: forward 8 B, backward 16 B per element.

#include "rlg_device.hpp"

namespace rlg {

constexpr int kLnBlock = 256;
constexpr int kLnWaves = kLnBlock / kWave;

template <int H>
struct LnShape {
  static constexpr int kLanes = H == 128 ? 32 : 16;   // lanes of a row
  static constexpr int kPer = H / kLanes;             // consecutive elements per lane
  static constexpr int kRows = kWave / kLanes;        // rows of a wave's pass
};

template <int LANES>
__device__ __forceinline__ double ln_row_sum(double v) {
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// PER consecutive floats of a row (PER 4: one 16-byte access; rows are 16-byte aligned and H % 4 == 0); zeros when !ok
template <int PER>
__device__ __forceinline__ void ln_load(const float* p, bool ok, float (&v)[PER]) {
  if (PER == 4) {
    f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = t[k];
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = ok ? p[k] : 0.0f;
  }
}

template <int PER>
__device__ __forceinline__ void ln_store(float* p, const float (&v)[PER]) {
  if (PER == 4) {
    f32x4 t;
#pragma unroll
    for (int k = 0; k < PER; ++k) t[k] = v[k];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) p[k] = v[k];
  }
}

template <int H>
__global__ __launch_bounds__(kLnBlock) void rnn_layer_norm_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    float* __restrict__ y, float* __restrict__ stats_or_null, long long rows) {
  using S = LnShape<H>;
  constexpr int PER = S::kPer;
  const int lane = lane_id();
  const int sub = lane / S::kLanes;
  const int col = (lane % S::kLanes) * PER;
  float gm[PER], bt[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    gm[k] = gamma[col + k];
    bt[k] = beta[col + k];
  }
  const long long wave = static_cast<long long>(blockIdx.x) * kLnWaves + wave_id();
  const long long nwaves = static_cast<long long>(gridDim.x) * kLnWaves;
  const long long groups = (rows + S::kRows - 1) / S::kRows;
  for (long long g = wave; g < groups; g += nwaves) {          // (wave-uniform: every lane takes part in the sums)
    const long long row = g * S::kRows + sub;
    const bool ok = row < rows;
    float v[PER];
    ln_load<PER>(x + (ok ? row * H + col : 0), ok, v);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) s += static_cast<double>(v[k]);
    const float mean = static_cast<float>(ln_row_sum<S::kLanes>(s) / H);
    float d[PER];
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      d[k] = v[k] - mean;
      q += static_cast<double>(d[k]) * static_cast<double>(d[k]);
    }
    const double var = ln_row_sum<S::kLanes>(q) / H;
    const float rstd = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
    if (!ok) continue;
    float o[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) o[k] = d[k] * rstd * gm[k] + bt[k];
    ln_store<PER>(y + row * H + col, o);
    if (stats_or_null != nullptr && col == 0) {
      stats_or_null[row * 2] = mean;
      stats_or_null[row * 2 + 1] = rstd;
    }
  }
}

// partials layout: d_gamma_partials / d_beta_partials [gridDim.x][H] fp64.
template <int H>
__global__ __launch_bounds__(kLnBlock) void rnn_layer_norm_bwd_kernel(
    const float* __restrict__ d_y, const float* __restrict__ x, const float* __restrict__ stats,
    const float* __restrict__ gamma, float* __restrict__ d_x, double* __restrict__ d_gamma_partials,
    double* __restrict__ d_beta_partials, long long rows) {
  using S = LnShape<H>;
  constexpr int PER = S::kPer;
  __shared__ double part[kLnWaves][2][H];
  const int lane = lane_id();
  const int sub = lane / S::kLanes;
  const int col = (lane % S::kLanes) * PER;
  float gm[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) gm[k] = gamma[col + k];
  double acc_g[PER], acc_b[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) acc_g[k] = acc_b[k] = 0.0;
  const long long wave = static_cast<long long>(blockIdx.x) * kLnWaves + wave_id();
  const long long nwaves = static_cast<long long>(gridDim.x) * kLnWaves;
  const long long groups = (rows + S::kRows - 1) / S::kRows;
  for (long long g = wave; g < groups; g += nwaves) {
    const long long row = g * S::kRows + sub;
    const bool ok = row < rows;
    const long long off = ok ? row * H + col : 0;
    float dy[PER], v[PER];
    ln_load<PER>(d_y + off, ok, dy);
    ln_load<PER>(x + off, ok, v);
    const float mean = ok ? stats[row * 2] : 0.0f;
    const float rstd = ok ? stats[row * 2 + 1] : 0.0f;
    float gk[PER], xh[PER];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      gk[k] = dy[k] * gm[k];
      xh[k] = (v[k] - mean) * rstd;
      s1 += static_cast<double>(gk[k]);
      s2 += static_cast<double>(gk[k]) * static_cast<double>(xh[k]);
      acc_g[k] += static_cast<double>(dy[k]) * static_cast<double>(xh[k]);      // (a row past the end adds zeros)
      acc_b[k] += static_cast<double>(dy[k]);
    }
    const float m1 = static_cast<float>(ln_row_sum<S::kLanes>(s1) / H);
    const float m2 = static_cast<float>(ln_row_sum<S::kLanes>(s2) / H);
    if (!ok) continue;
    float o[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) o[k] = rstd * (gk[k] - m1 - xh[k] * m2);
    ln_store<PER>(d_x + row * H + col, o);
  }
  // column partials: the wave's row slots (same columns, lanes LANES apart), then the waves in index order
#pragma unroll
  for (int k = 0; k < PER; ++k) {
#pragma unroll
    for (int o = S::kLanes; o < kWave; o <<= 1) {
      acc_g[k] += __shfl_xor(acc_g[k], o, kWave);
      acc_b[k] += __shfl_xor(acc_b[k], o, kWave);
    }
  }
  if (sub == 0) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      part[wave_id()][0][col + k] = acc_g[k];
      part[wave_id()][1][col + k] = acc_b[k];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * H; j += kLnBlock) {
    const int which = j / H, c = j - which * H;
    double t = part[0][which][c];
#pragma unroll
    for (int w = 1; w < kLnWaves; ++w) t += part[w][which][c];
    (which == 0 ? d_gamma_partials : d_beta_partials)[static_cast<long long>(blockIdx.x) * H + c] = t;
  }
}

static bool ln_width_ok(int hidden) { return hidden == 16 || hidden == 32 || hidden == 64 || hidden == 128; }

static bool ln_aligned(const void* p, uintptr_t a) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % a == 0; }

constexpr int kLnMaxBlocks = 1024;

}  // namespace rlg

extern "C" {

int rlg_rnn_layer_norm_num_blocks(long long rows, int hidden) {
  using namespace rlg;
  if (rows <= 0 || !ln_width_ok(hidden)) return 0;
  const int rows_per_pass = kLnWaves * (hidden == 128 ? 2 : 4);
  long long need = (rows + rows_per_pass * 4LL - 1) / (rows_per_pass * 4LL);      // >= 4 passes per workgroup
  if (need < 1) need = 1;
  if (need > 256) need = 256;      // one workgroup per CU; few partial rows for the finalise pass
  return static_cast<int>(need);
}

int rlg_rnn_layer_norm_forward(const float* x, const float* gamma, const float* beta, float eps, float* y,
                               float* stats_or_null, long long rows, int hidden, void* stream) {
  using namespace rlg;
  if (rows <= 0 || !ln_width_ok(hidden) || !(eps >= 0.0f)) return static_cast<int>(hipErrorInvalidValue);
  if (!ln_aligned(x, 16) || !ln_aligned(y, 16) || !ln_aligned(gamma, 4) || !ln_aligned(beta, 4) ||
      (stats_or_null != nullptr && !ln_aligned(stats_or_null, 4)))
    return static_cast<int>(hipErrorInvalidValue);
  const int rows_per_pass = kLnWaves * (hidden == 128 ? 2 : 4);
  long long blocks = (rows + rows_per_pass - 1) / rows_per_pass;
  if (blocks > kLnMaxBlocks) blocks = kLnMaxBlocks;
  const dim3 grid(static_cast<unsigned>(blocks)), block(kLnBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define RLG_LN_FWD(HH)                                                                                     \
  hipLaunchKernelGGL((rnn_layer_norm_fwd_kernel<HH>), grid, block, 0, st, x, gamma, beta, eps, y, stats_or_null, rows)
  switch (hidden) {
    case 16: RLG_LN_FWD(16); break;
    case 32: RLG_LN_FWD(32); break;
    case 64: RLG_LN_FWD(64); break;
    default: RLG_LN_FWD(128); break;
  }
#undef RLG_LN_FWD
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_rnn_layer_norm_backward(const float* d_y, const float* x, const float* stats, const float* gamma, float* d_x,
                                double* d_gamma_partials, double* d_beta_partials, int num_blocks, long long rows,
                                int hidden, void* stream) {
  using namespace rlg;
  if (rows <= 0 || !ln_width_ok(hidden) || num_blocks < 1 || num_blocks > kLnMaxBlocks)
    return static_cast<int>(hipErrorInvalidValue);
  if (!ln_aligned(d_y, 16) || !ln_aligned(x, 16) || !ln_aligned(d_x, 16) || !ln_aligned(stats, 4) ||
      !ln_aligned(gamma, 4) || !ln_aligned(d_gamma_partials, 8) || !ln_aligned(d_beta_partials, 8))
    return static_cast<int>(hipErrorInvalidValue);
  const dim3 grid(static_cast<unsigned>(num_blocks)), block(kLnBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define RLG_LN_BWD(HH)                                                                                          \
  hipLaunchKernelGGL((rnn_layer_norm_bwd_kernel<HH>), grid, block, 0, st, d_y, x, stats, gamma, d_x, d_gamma_partials, \
                     d_beta_partials, rows)
  switch (hidden) {
    case 16: RLG_LN_BWD(16); break;
    case 32: RLG_LN_BWD(32); break;
    case 64: RLG_LN_BWD(64); break;
    default: RLG_LN_BWD(128); break;
  }
#undef RLG_LN_BWD
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
