// Sequence-persistent GRU layer for recurrent PPO policies (`rnn: {name: gru, layers: 1}` behind the MLP), gfx950.
//
// The GRU counterpart of csrc/lstm.hip, for the same position in A2CBuilder's network
// (rl_games/algos_torch/network_builder.py:250-276 with rl_games/common/layers/recurrent.py `GRUWithDones`): it
// replaces the per-timestep torch.nn.GRU calls, the done-state resets between them and autograd's BPTT.
//
// The cell is torch.nn.GRU's, gate order (r, z, n):
//   r = sigmoid(gx_r + W_hr h + b_hr)     z = sigmoid(gx_z + W_hz h + b_hz)
//   hn = W_hn h + b_hn                    n = tanh(gx_n + r * hn)                h' = (1 - z) * n + z * h
// gx = x W_ih^T + b_ih for every timestep is ONE product before the launch (rows ordered seq*T + t).  b_hn is
// multiplied by r and cannot be folded into gx the way lstm.hip folds b_hh: the kernel takes b_hh [3H] and adds it.
//
// One launch runs ALL timesteps of a tile of sequences, as in lstm.hip (the product scheme, shared with it, the cell
// formulas, shared with gru_wide.hip, and the launch and dispatch helpers are in rnn_seq.hpp):
//   * W_hh [3H, H] (48 KB for H = 64) lives in LDS for the whole kernel;
//   * thread (j, group) owns hidden unit j of R sequences; the hidden state goes through a double-buffered LDS tile
//     (one barrier per timestep);
//   * the kernel overwrites gx with the activated gates (r, z, n); for training it also keeps hn (before the gating
//     by r - what c_all is to the LSTM) and the state entering each step.
// Backward walks the same tile in reverse and emits TWO arrays: d_gx = (dr, dz, dn), the gradient of the input side
// (dW_ih = d_gx^T X, db_ih, the trunk's dX), and d_gh = (dr, dz, dn * r), the gradient of the hidden side
// (dW_hh = d_gh^T Hprev, db_hh); the weight gradients are whole-sequence products outside the kernel.
//   dn = dh (1 - z)(1 - n^2)   dz = dh (h_prev - n) z (1 - z)   dr = dn hn r (1 - r)
//   dh_prev = dh z + W_hh^T d_gh, zeroed where step t is done.
//
// The matvec per step is H*3H MACs per sequence: latency-bound by the timestep chain, VALU FMAs out of LDS.
// 128 units: csrc/gru_wide.hip.

#include "rnn_seq.hpp"

namespace rlg {

// Bodies as functions: the single and the paired kernel run the same code (rnn_seq.hpp, "paired launches").
template <int H, int SB>
__device__ __forceinline__ void gru_seq_fwd_body(
    float* __restrict__ gates,           // [S*T, 3H]  in: x-part + b_ih, out: activated gates (r, z, n)
    const float* __restrict__ w_hh,      // [3H, H]
    const float* __restrict__ b_hh,      // [3H]
    const float* __restrict__ h0,        // [S, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    float* __restrict__ out,             // [S*T, H]  h_t
    float* __restrict__ hn_all,          // [S*T, H]  W_hn h + b_hn    (nullptr: not kept)
    float* __restrict__ hprev,           // [S*T, H]  state entering step t, after the reset (nullptr)
    float* __restrict__ hT,              // [S, H] final h (nullptr)
    int S, int T) {
  constexpr int G = 3 * H;
  constexpr int kGroups = kSeqThreads / H;             // sequence groups per block
  constexpr int R = SB / kGroups;                      // sequences per thread
  static_assert(kSeqThreads % H == 0 && SB % kGroups == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wT = smem;                                     // [H][3H]: wT[k][r] = w_hh[r][k]
  float* hbuf = smem + H * G;                           // [2][SB][H]
  const int tid = threadIdx.x;
  const int j = tid % H;
  const int grp = tid / H;
  narrow_stage_w_transposed<3, H>(wT, w_hh);
  const float bias[3] = {b_hh[0 * H + j], b_hh[1 * H + j], b_hh[2 * H + j]};
  int seq[R];
  bool live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    tile_slot(blockIdx.x * SB + grp * R + r, S, seq[r], live[r]);
    hbuf[(grp * R + r) * H + j] = h0[static_cast<long long>(seq[r]) * H + j];
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const float* hcur = hbuf + (t & 1) * SB * H;
    float* hnext = hbuf + ((t + 1) & 1) * SB * H;
    float acc[3][R];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
      for (int r = 0; r < R; ++r) acc[g][r] = 0.0f;
    }
#pragma unroll 4
    for (int k = 0; k < H; ++k) {
      const float w0 = wT[k * G + 0 * H + j];
      const float w1 = wT[k * G + 1 * H + j];
      const float w2 = wT[k * G + 2 * H + j];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float hv = hcur[(grp * R + r) * H + k];   // wave-uniform address: LDS broadcast
        acc[0][r] = __builtin_fmaf(w0, hv, acc[0][r]);
        acc[1][r] = __builtin_fmaf(w1, hv, acc[1][r]);
        acc[2][r] = __builtin_fmaf(w2, hv, acc[2][r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = static_cast<long long>(seq[r]) * T + t;
      const float keep = step_keep(dones, row);
      float* grow = gates + row * G;
      const float hp = hcur[(grp * R + r) * H + j] * keep;
      // a slot past S aliases sequence S - 1, whose gates its owner overwrites in this very step: it loads none of
      // them (its state only ever reaches its own column of the LDS tile and is never stored)
      const float x[3] = {live[r] ? grow[0 * H + j] : 0.0f, live[r] ? grow[1 * H + j] : 0.0f,
                          live[r] ? grow[2 * H + j] : 0.0f};
      const float a[3] = {acc[0][r], acc[1][r], acc[2][r]};
      float g[3], hn;
      const float hnew = gru_fwd_point(x, a, bias, keep, hp, g, hn);
      hnext[(grp * R + r) * H + j] = hnew;
      if (live[r]) {
        grow[0 * H + j] = g[0];
        grow[1 * H + j] = g[1];
        grow[2 * H + j] = g[2];
        out[row * H + j] = hnew;
        if (hn_all) hn_all[row * H + j] = hn;
        if (hprev) hprev[row * H + j] = hp;
      }
    }
    __syncthreads();
  }
  if (hT) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (live[r]) hT[static_cast<long long>(seq[r]) * H + j] = hbuf[(T & 1) * SB * H + (grp * R + r) * H + j];
    }
  }
}

template <int H, int SB>
__device__ __forceinline__ void gru_seq_bwd_body(
    const float* __restrict__ gates,     // [S*T, 3H] activated gates of the forward pass
    const float* __restrict__ hn_all,    // [S*T, H]
    const float* __restrict__ hprev,     // [S*T, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    const float* __restrict__ w_hh,      // [3H, H]
    const float* __restrict__ d_out,     // [S*T, H]  d loss / d h_t (from the layers above)
    float* __restrict__ d_gx,            // [S*T, 3H] d loss / d (x W_ih^T + b_ih)
    float* __restrict__ d_gh,            // [S*T, 3H] d loss / d (h W_hh^T + b_hh)
    int S, int T) {
  constexpr int G = 3 * H;
  constexpr int kGroups = kSeqThreads / H;
  constexpr int R = SB / kGroups;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* w = smem;                                      // [3H][H] as stored
  float* dgb = smem + G * H;                            // [SB][3H]
  const int tid = threadIdx.x;
  const int j = tid % H;
  const int grp = tid / H;
  if (T > 1) {                                          // (T = 1: no state before step 0 to send a gradient to)
    narrow_stage_w<3, H>(w, w_hh);
  }
  int seq[R];
  bool live[R];
  float dh_next[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    tile_slot(blockIdx.x * SB + grp * R + r, S, seq[r], live[r]);
    dh_next[r] = 0.0f;
  }
  __syncthreads();

  for (int t = T - 1; t >= 0; --t) {
    float keep[R], dhz[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = static_cast<long long>(seq[r]) * T + t;
      keep[r] = step_keep(dones, row);
      const float* grow = gates + row * G;
      const float g[3] = {grow[0 * H + j], grow[1 * H + j], grow[2 * H + j]};
      const float hn = hn_all[row * H + j];
      const float hp = hprev[row * H + j];
      const float dh = d_out[row * H + j] + dh_next[r];
      float dgx[3], dnr;
      dhz[r] = gru_bwd_point(g, hn, hp, dh, dgx, dnr);
      float* db = dgb + (grp * R + r) * G;
      db[0 * H + j] = dgx[0];
      db[1 * H + j] = dgx[1];
      db[2 * H + j] = dnr;
      if (live[r]) {
        float* xrow = d_gx + row * G;
        float* hrow = d_gh + row * G;
        xrow[0 * H + j] = dgx[0];
        xrow[1 * H + j] = dgx[1];
        xrow[2 * H + j] = dgx[2];
        hrow[0 * H + j] = dgx[0];
        hrow[1 * H + j] = dgx[1];
        hrow[2 * H + j] = dnr;
      }
    }
    if (t == 0) break;                                  // nothing consumes d h_{-1}
    __syncthreads();
    float acc[R];
    narrow_bwd_product<3, H, R>(acc, w, dgb, j, grp);
#pragma unroll
    for (int r = 0; r < R; ++r) dh_next[r] = (dhz[r] + acc[r]) * keep[r];
    __syncthreads();
  }
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void gru_seq_fwd_kernel(
    float* __restrict__ gates, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
    const float* __restrict__ h0, const uint8_t* __restrict__ dones, float* __restrict__ out,
    float* __restrict__ hn_all, float* __restrict__ hprev, float* __restrict__ hT, int S, int T) {
  gru_seq_fwd_body<H, SB>(gates, w_hh, b_hh, h0, dones, out, hn_all, hprev, hT, S, T);
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void gru_seq_fwd_pair_kernel(GruFwdArgs a, GruFwdArgs b, int S, int T) {
  const GruFwdArgs& p = pair_problem(a, b);
  gru_seq_fwd_body<H, SB>(p.gates, p.w_hh, p.b_hh, p.h0, p.dones, p.out, p.hn_all, p.hprev, p.hT, S, T);
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void gru_seq_bwd_kernel(
    const float* __restrict__ gates, const float* __restrict__ hn_all, const float* __restrict__ hprev,
    const uint8_t* __restrict__ dones, const float* __restrict__ w_hh, const float* __restrict__ d_out,
    float* __restrict__ d_gx, float* __restrict__ d_gh, int S, int T) {
  gru_seq_bwd_body<H, SB>(gates, hn_all, hprev, dones, w_hh, d_out, d_gx, d_gh, S, T);
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void gru_seq_bwd_pair_kernel(GruBwdArgs a, GruBwdArgs b, int S, int T) {
  const GruBwdArgs& p = pair_problem(a, b);
  gru_seq_bwd_body<H, SB>(p.gates, p.hn_all, p.hprev, p.dones, p.w_hh, p.d_out, p.d_gx, p.d_gh, S, T);
}

// 128 units: W_hh (192 KB) does not fit LDS; csrc/gru_wide.hip keeps it in registers as MFMA fragments.
int launch_gru_fwd_wide(const GruFwdArgs* problems, int count, int S, int T, hipStream_t st);
int launch_gru_bwd_wide(const GruBwdArgs* problems, int count, int S, int T, hipStream_t st);

// kernel families for rnn_seq.hpp's launch_seq
struct GruFwd {
  using Args = GruFwdArgs;
  template <int H, int SB>
  static constexpr auto kernel = gru_seq_fwd_kernel<H, SB>;
  template <int H, int SB>
  static constexpr auto pair_kernel = gru_seq_fwd_pair_kernel<H, SB>;
  static constexpr size_t lds_floats(int H, int SB) { return static_cast<size_t>(3) * H * H + 2 * SB * H; }
  static constexpr auto wide = launch_gru_fwd_wide;
};

struct GruBwd {
  using Args = GruBwdArgs;
  template <int H, int SB>
  static constexpr auto kernel = gru_seq_bwd_kernel<H, SB>;
  template <int H, int SB>
  static constexpr auto pair_kernel = gru_seq_bwd_pair_kernel<H, SB>;
  static constexpr size_t lds_floats(int H, int SB) { return static_cast<size_t>(3) * H * H + SB * 3 * H; }
  static constexpr auto wide = launch_gru_bwd_wide;
};

// kernel order of the code object: rnn_seq.hpp
static_assert(single_kernels_first<GruFwd>() && single_kernels_first<GruBwd>());

}  // namespace rlg

extern "C" {

int rlg_gru_supported(int hidden) { return rlg::seq_hidden_supported(hidden) ? 1 : 0; }

int rlg_gru_seq_forward(const rlg_gru_fwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                        void* stream) {
  return rlg::launch_seq<rlg::GruFwd>(problems, num_problems, hidden, num_seqs, seq_len, stream);
}

int rlg_gru_seq_backward(const rlg_gru_bwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                         void* stream) {
  return rlg::launch_seq<rlg::GruBwd>(problems, num_problems, hidden, num_seqs, seq_len, stream);
}

}  // extern "C"
