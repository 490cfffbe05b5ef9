// Value head + clipped value loss + its backward behind the recurrent layer of a central value critic, gfx950.
//
// `central_value_config.network` of the reference's recurrent SMAC critics ends in one value column over the RNN
// (or layer-normed) features feat [rows, H], H one of the widths the sequence-persistent kernels run (16 / 32 / 64 /
// 128, csrc/rnn_seq.hpp).  One launch replaces a 1-column product padded to an MFMA tile, rlg_value_loss, the head's dX,
// a torch.sum for the bias gradient and a 1 x H weight-gradient job:
//   value     values[r] = b + sum_k feat[r,k] w[k]: products and sum in fp64 (a product of two fp32 values is exact
//             there), rounded to fp32 once
//   loss      value_loss_row (value_loss_row.hpp - the row formula of rlg_value_loss) -> d_values[r], and per workgroup
//             the fp64 partials {0, sum c m, 0, 0, 0, sum m, 0} that rlg_ppo_loss_finalize folds
//   backward  d_feat[r,k] = d_values[r] w[k] (one fp32 product);  d w = sum_r d_values[r] feat[r,k] and
//             d b = sum_r d_values[r] as per-workgroup fp64 column partials in the [blocks][cols] layout of
//             act_bwd_colsum_kernel (csrc/mlp_fused.hip) - finished by rlg_colsum_finalize or by the finalise of the
//             weight-gradient launch like every other bias gradient.
// rnn_value_head_kernel is the inference form: the values alone, the same bits.
//
// The shape of csrc/rnn_layer_norm.hip: a row lives in the lanes of one wave, 16 lanes at H <= 64 (1 / 2 / 4
// consecutive elements per lane), 32 lanes at H = 128 (4 per lane); row sums are an xor butterfly over the row's lanes
// in fp64, so the order is fixed, every lane of the row ends with the same bits, and a row's result depends on nothing
// but the row.  No atomics; LDS only to add the four waves' partials.  Memory-bound: 8 B per feature element.

#include "value_loss_row.hpp"

namespace rlg {

constexpr int kVtBlock = 256;
constexpr int kVtWaves = kVtBlock / kWave;
constexpr int kVtMaxBlocks = 1024;
constexpr int kVtLossSlots = 7;      // kLossScalars of ppo_loss_tile.hpp: what rlg_ppo_loss_finalize reads per block

template <int H>
struct VtShape {
  static constexpr int kLanes = H == 128 ? 32 : 16;   // lanes of a row
  static constexpr int kPer = H / kLanes;             // consecutive elements per lane
  static constexpr int kRows = kWave / kLanes;        // rows of a wave's pass
};

// PER consecutive floats of a row (PER 4: one 16-byte access; rows are 16-byte aligned and H % 4 == 0); zeros when !ok
template <int PER>
__device__ __forceinline__ void vt_load(const float* p, bool ok, float (&v)[PER]) {
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
__device__ __forceinline__ void vt_store(float* p, const float (&v)[PER]) {
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

// The row's value from this lane's PER features: every lane of the row returns the same bits.
template <int LANES, int PER>
__device__ __forceinline__ float vt_row_value(const float (&f)[PER], const float (&w)[PER], float bias) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < PER; ++k) s += static_cast<double>(f[k]) * static_cast<double>(w[k]);
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
  return static_cast<float>(static_cast<double>(bias) + s);
}

template <int H>
__global__ __launch_bounds__(kVtBlock) void rnn_value_head_kernel(
    const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ b,
    float* __restrict__ values, long long rows) {
  using S = VtShape<H>;
  constexpr int PER = S::kPer;
  const int lane = lane_id();
  const int sub = lane / S::kLanes;
  const int col = (lane % S::kLanes) * PER;
  float wk[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) wk[k] = w[col + k];
  const float bias = b[0];
  const long long wave = static_cast<long long>(blockIdx.x) * kVtWaves + wave_id();
  const long long nwaves = static_cast<long long>(gridDim.x) * kVtWaves;
  const long long groups = (rows + S::kRows - 1) / S::kRows;
  for (long long g = wave; g < groups; g += nwaves) {          // (wave-uniform: every lane takes part in the sums)
    const long long row = g * S::kRows + sub;
    const bool ok = row < rows;
    float f[PER];
    vt_load<PER>(feat + (ok ? row * H + col : 0), ok, f);
    const float v = vt_row_value<S::kLanes, PER>(f, wk, bias);
    if (ok && col == 0) values[row] = v;
  }
}

// partials layout: loss_partials [gridDim.x][7], d_w_partials [gridDim.x][H], d_b_partials [gridDim.x][1], all fp64.
template <int H>
__global__ __launch_bounds__(kVtBlock) void rnn_value_tail_kernel(
    const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ old_values, const float* __restrict__ returns, const float* __restrict__ mask,
    const float* __restrict__ mask_sum, float* __restrict__ values, float* __restrict__ d_values,
    float* __restrict__ d_feat, double* __restrict__ loss_partials, double* __restrict__ d_w_partials,
    double* __restrict__ d_b_partials, long long rows, float e_clip, int clip_value) {
  using S = VtShape<H>;
  constexpr int PER = S::kPer;
  __shared__ double part_w[kVtWaves][H];
  __shared__ double part_s[kVtWaves][3];
  const int lane = lane_id();
  const int sub = lane / S::kLanes;
  const int col = (lane % S::kLanes) * PER;
  float wk[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) wk[k] = w[col + k];
  const float bias = b[0];
  const float denom = mask ? fmaxf(*mask_sum, 1.0f) : static_cast<float>(rows);
  double acc_w[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) acc_w[k] = 0.0;
  double acc_c = 0.0, acc_m = 0.0, acc_b = 0.0;        // the row's first lane alone adds to these
  const long long wave = static_cast<long long>(blockIdx.x) * kVtWaves + wave_id();
  const long long nwaves = static_cast<long long>(gridDim.x) * kVtWaves;
  const long long groups = (rows + S::kRows - 1) / S::kRows;
  for (long long g = wave; g < groups; g += nwaves) {
    const long long row = g * S::kRows + sub;
    const bool ok = row < rows;
    float f[PER];
    vt_load<PER>(feat + (ok ? row * H + col : 0), ok, f);
    const float v = vt_row_value<S::kLanes, PER>(f, wk, bias);
    if (!ok) continue;                                  // (after the butterfly)
    const float m = mask ? mask[row] : 1.0f;
    const ValueLossRow r = value_loss_row(v, old_values[row], returns[row], m, denom, e_clip, clip_value);
    float o[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      o[k] = r.d_value * wk[k];
      acc_w[k] += static_cast<double>(r.d_value) * static_cast<double>(f[k]);
    }
    vt_store<PER>(d_feat + row * H + col, o);
    if (col == 0) {
      values[row] = v;
      d_values[row] = r.d_value;
      acc_c += static_cast<double>(r.c_loss) * m;
      acc_m += m;
      acc_b += static_cast<double>(r.d_value);
    }
  }
  // column partials: the wave's row slots (same columns, lanes LANES apart), then the waves in index order
#pragma unroll
  for (int k = 0; k < PER; ++k) {
#pragma unroll
    for (int o = S::kLanes; o < kWave; o <<= 1) acc_w[k] += __shfl_xor(acc_w[k], o, kWave);
  }
  acc_c = wave_sum(acc_c);
  acc_m = wave_sum(acc_m);
  acc_b = wave_sum(acc_b);
  if (sub == 0) {
#pragma unroll
    for (int k = 0; k < PER; ++k) part_w[wave_id()][col + k] = acc_w[k];
  }
  if (lane == 0) {
    part_s[wave_id()][0] = acc_c;
    part_s[wave_id()][1] = acc_m;
    part_s[wave_id()][2] = acc_b;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < H; j += kVtBlock) {
    double t = part_w[0][j];
#pragma unroll
    for (int wv = 1; wv < kVtWaves; ++wv) t += part_w[wv][j];
    d_w_partials[static_cast<long long>(blockIdx.x) * H + j] = t;
  }
  if (threadIdx.x == kVtBlock - 1) {                    // (a thread the column loop above leaves idle)
    double t[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      t[q] = part_s[0][q];
#pragma unroll
      for (int wv = 1; wv < kVtWaves; ++wv) t[q] += part_s[wv][q];
    }
    double* out = loss_partials + static_cast<long long>(blockIdx.x) * kVtLossSlots;
    out[0] = 0.0;
    out[1] = t[0];
    out[2] = 0.0;
    out[3] = 0.0;
    out[4] = 0.0;
    out[5] = t[1];
    out[6] = 0.0;
    d_b_partials[blockIdx.x] = t[2];
  }
}

static bool vt_width_ok(int hidden) { return hidden == 16 || hidden == 32 || hidden == 64 || hidden == 128; }

static bool vt_aligned(const void* p, uintptr_t a) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace rlg

extern "C" {

int rlg_rnn_value_tail_num_blocks(long long rows, int hidden) {
  using namespace rlg;
  if (rows <= 0 || !vt_width_ok(hidden)) return 0;
  const int rows_per_pass = kVtWaves * (hidden == 128 ? 2 : 4);
  long long need = (rows + rows_per_pass * 4LL - 1) / (rows_per_pass * 4LL);      // >= 4 passes per workgroup
  if (need < 1) need = 1;
  if (need > 256) need = 256;      // one workgroup per CU; few partial rows for the finalise pass
  return static_cast<int>(need);
}

int rlg_rnn_value_head(const float* feat, const float* w, const float* b, float* values, long long rows, int hidden,
                       void* stream) {
  using namespace rlg;
  if (rows <= 0 || !vt_width_ok(hidden)) return static_cast<int>(hipErrorInvalidValue);
  if (!vt_aligned(feat, 16) || !vt_aligned(w, 4) || !vt_aligned(b, 4) || !vt_aligned(values, 4))
    return static_cast<int>(hipErrorInvalidValue);
  const int rows_per_pass = kVtWaves * (hidden == 128 ? 2 : 4);
  long long blocks = (rows + rows_per_pass - 1) / rows_per_pass;
  if (blocks > kVtMaxBlocks) blocks = kVtMaxBlocks;
  const dim3 grid(static_cast<unsigned>(blocks)), block(kVtBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define RLG_VT_HEAD(HH) hipLaunchKernelGGL((rnn_value_head_kernel<HH>), grid, block, 0, st, feat, w, b, values, rows)
  switch (hidden) {
    case 16: RLG_VT_HEAD(16); break;
    case 32: RLG_VT_HEAD(32); break;
    case 64: RLG_VT_HEAD(64); break;
    default: RLG_VT_HEAD(128); break;
  }
#undef RLG_VT_HEAD
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_rnn_value_tail(const float* feat, const float* w, const float* b, const float* old_values,
                       const float* returns, const float* mask_or_null, const float* mask_sum_or_null, float* values,
                       float* d_values, float* d_feat, double* loss_partials, double* d_w_partials,
                       double* d_b_partials, int num_blocks, long long rows, int hidden, float e_clip, int clip_value,
                       void* stream) {
  using namespace rlg;
  if (rows <= 0 || !vt_width_ok(hidden) || num_blocks < 1 || num_blocks > kVtMaxBlocks)
    return static_cast<int>(hipErrorInvalidValue);
  if (mask_or_null && !mask_sum_or_null) return static_cast<int>(hipErrorInvalidValue);
  if (!vt_aligned(feat, 16) || !vt_aligned(d_feat, 16) || !vt_aligned(w, 4) || !vt_aligned(b, 4) ||
      !vt_aligned(old_values, 4) || !vt_aligned(returns, 4) || !vt_aligned(values, 4) || !vt_aligned(d_values, 4) ||
      !vt_aligned(loss_partials, 8) || !vt_aligned(d_w_partials, 8) || !vt_aligned(d_b_partials, 8) ||
      (mask_or_null != nullptr && (!vt_aligned(mask_or_null, 4) || !vt_aligned(mask_sum_or_null, 4))))
    return static_cast<int>(hipErrorInvalidValue);
  const dim3 grid(static_cast<unsigned>(num_blocks)), block(kVtBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define RLG_VT_TAIL(HH)                                                                                              \
  hipLaunchKernelGGL((rnn_value_tail_kernel<HH>), grid, block, 0, st, feat, w, b, old_values, returns, mask_or_null, \
                     mask_sum_or_null, values, d_values, d_feat, loss_partials, d_w_partials, d_b_partials, rows,    \
                     e_clip, clip_value)
  switch (hidden) {
    case 16: RLG_VT_TAIL(16); break;
    case 32: RLG_VT_TAIL(32); break;
    case 64: RLG_VT_TAIL(64); break;
    default: RLG_VT_TAIL(128); break;
  }
#undef RLG_VT_TAIL
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
