// Sequence-persistent LSTM layer for the recurrent PPO policy (BASELINE config #5), gfx950.
//
// Replaces, for the `rnn: {name: lstm, layers: 1}` policies of A2CBuilder
// (rl_games/algos_torch/network_builder.py:447-512 with rl_games/common/layers/recurrent.py:26-58
// `LSTMWithDones`), the per-timestep torch.nn.LSTM (MIOpen) calls, the done-state resets between
// them and - in backward - autograd's BPTT through that Python loop.
//
// One launch runs ALL timesteps of a tile of sequences:
//   * the recurrent weights W_hh [4H, H] (64 KB for H = 64) live in LDS for the whole kernel;
//   * thread (j, group) owns hidden unit j of R sequences: their cell state c stays in registers,
//     the hidden state goes through a double-buffered LDS tile (one barrier per timestep);
//   * the input projection  x_t W_ih^T + b_ih + b_hh  for every timestep is ONE library GEMM
//     before the kernel (rows ordered seq*T + t, the dataset's order); the kernel overwrites it
//     with the activated gates (i, f, g, o - torch.nn.LSTM's gate order), which backward reuses;
//   * done handling: the zeroing of the state entering a done step is recurrent.py:45-55's semantics; the mirror is
//     policy.RnnWithDones.
// Backward walks the same tile in reverse, emitting d(gates pre-activation) [B, 4H]; the weight
// gradients are then plain GEMMs over all timesteps at once (dW_ih = dG^T X, dW_hh = dG^T Hprev).
//
// The matvec per step is H*4H MACs per sequence (16 K at H = 64): far below MFMA tile sizes per
// block and latency-bound by the timestep chain, so it runs on VALU FMAs out of LDS.
//
// The product scheme (shared with gru.hip), the cell formulas (shared with lstm_wide.hip) and the launch and dispatch
// helpers are in rnn_seq.hpp.

#include "rnn_seq.hpp"

namespace rlg {

// The kernels' bodies are functions, so that the single kernel and the paired one (rnn_seq.hpp, "paired launches")
// run the same code: a body reads its tile from blockIdx.x and nothing else of the grid.
template <int H, int SB>
__device__ __forceinline__ void lstm_seq_fwd_body(
    float* __restrict__ gates,           // [S*T, 4H]  in: x-part + biases, out: activated gates
    const float* __restrict__ w_hh,      // [4H, H]
    const float* __restrict__ h0,        // [S, H]
    const float* __restrict__ c0,        // [S, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    float* __restrict__ out,             // [S*T, H]  h_t
    float* __restrict__ c_all,           // [S*T, H]  c_t             (nullptr: not kept)
    float* __restrict__ hprev,           // [S*T, H]  state entering step t, after the reset (nullptr)
    float* __restrict__ hT,              // [S, H] final h (nullptr)
    float* __restrict__ cT,              // [S, H] final c (nullptr)
    int S, int T) {
  constexpr int G = 4 * H;
  constexpr int kGroups = kSeqThreads / H;              // sequence groups per block
  constexpr int R = SB / kGroups;                       // sequences per thread
  static_assert(kSeqThreads % H == 0 && SB % kGroups == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wT = smem;                                     // [H][4H]: wT[k][r] = w_hh[r][k]
  float* hbuf = smem + H * G;                           // [2][SB][H]
  const int tid = threadIdx.x;
  const int j = tid % H;
  const int grp = tid / H;
  narrow_stage_w_transposed<4, H>(wT, w_hh);
  int seq[R];
  bool live[R];
  float c[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    tile_slot(blockIdx.x * SB + grp * R + r, S, seq[r], live[r]);
    c[r] = c0[static_cast<long long>(seq[r]) * H + j];
    hbuf[(grp * R + r) * H + j] = h0[static_cast<long long>(seq[r]) * H + j];
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const float* hcur = hbuf + (t & 1) * SB * H;
    float* hnext = hbuf + ((t + 1) & 1) * SB * H;
    float acc[4][R];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int r = 0; r < R; ++r) acc[g][r] = 0.0f;
    }
#pragma unroll 4
    for (int k = 0; k < H; ++k) {
      const float w0 = wT[k * G + 0 * H + j];
      const float w1 = wT[k * G + 1 * H + j];
      const float w2 = wT[k * G + 2 * H + j];
      const float w3 = wT[k * G + 3 * H + j];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float hv = hcur[(grp * R + r) * H + k];   // wave-uniform address: LDS broadcast
        acc[0][r] = __builtin_fmaf(w0, hv, acc[0][r]);
        acc[1][r] = __builtin_fmaf(w1, hv, acc[1][r]);
        acc[2][r] = __builtin_fmaf(w2, hv, acc[2][r]);
        acc[3][r] = __builtin_fmaf(w3, hv, acc[3][r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = static_cast<long long>(seq[r]) * T + t;
      const float keep = step_keep(dones, row);
      float* grow = gates + row * G;
      const float a[4] = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
      float g[4];
      const float hn = lstm_fwd_point(grow + j, H, a, keep, c[r], g);
      const float hp = hcur[(grp * R + r) * H + j] * keep;
      hnext[(grp * R + r) * H + j] = hn;
      if (live[r]) {
        grow[0 * H + j] = g[0];
        grow[1 * H + j] = g[1];
        grow[2 * H + j] = g[2];
        grow[3 * H + j] = g[3];
        out[row * H + j] = hn;
        if (c_all) c_all[row * H + j] = c[r];
        if (hprev) hprev[row * H + j] = hp;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!live[r]) continue;
    if (hT) hT[static_cast<long long>(seq[r]) * H + j] = hbuf[(T & 1) * SB * H + (grp * R + r) * H + j];
    if (cT) cT[static_cast<long long>(seq[r]) * H + j] = c[r];
  }
}

template <int H, int SB>
__device__ __forceinline__ void lstm_seq_bwd_body(
    const float* __restrict__ gates,     // [S*T, 4H] activated gates of the forward pass
    const float* __restrict__ c_all,     // [S*T, H]
    const float* __restrict__ c0,        // [S, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    const float* __restrict__ w_hh,      // [4H, H]
    const float* __restrict__ d_out,     // [S*T, H]  d loss / d h_t (from the layers above)
    float* __restrict__ d_gates,         // [S*T, 4H] d loss / d gate pre-activations
    int S, int T) {
  constexpr int G = 4 * H;
  constexpr int kGroups = kSeqThreads / H;
  constexpr int R = SB / kGroups;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* w = smem;                                      // [4H][H] as stored
  float* dgb = smem + G * H;                            // [SB][4H]
  const int tid = threadIdx.x;
  const int j = tid % H;
  const int grp = tid / H;
  narrow_stage_w<4, H>(w, w_hh);
  int seq[R];
  bool live[R];
  float dh_next[R], dc_next[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    tile_slot(blockIdx.x * SB + grp * R + r, S, seq[r], live[r]);
    dh_next[r] = 0.0f;
    dc_next[r] = 0.0f;
  }
  __syncthreads();

  for (int t = T - 1; t >= 0; --t) {
    float keep[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = static_cast<long long>(seq[r]) * T + t;
      keep[r] = step_keep(dones, row);
      const float* grow = gates + row * G;
      const float g[4] = {grow[0 * H + j], grow[1 * H + j], grow[2 * H + j], grow[3 * H + j]};
      const float ct = c_all[row * H + j];
      const float c_in = (t > 0 ? c_all[(row - 1) * H + j] : c0[static_cast<long long>(seq[r]) * H + j]) * keep[r];
      const float dh = d_out[row * H + j] + dh_next[r];
      float dg[4];
      lstm_bwd_point(g, ct, c_in, dh, keep[r], dc_next[r], dg);
      float* db = dgb + (grp * R + r) * G;
      db[0 * H + j] = dg[0];
      db[1 * H + j] = dg[1];
      db[2 * H + j] = dg[2];
      db[3 * H + j] = dg[3];
      if (live[r]) {
        float* drow = d_gates + row * G;
        drow[0 * H + j] = dg[0];
        drow[1 * H + j] = dg[1];
        drow[2 * H + j] = dg[2];
        drow[3 * H + j] = dg[3];
      }
    }
    __syncthreads();
    float acc[R];
    narrow_bwd_product<4, H, R>(acc, w, dgb, j, grp);
#pragma unroll
    for (int r = 0; r < R; ++r) dh_next[r] = acc[r] * keep[r];
    __syncthreads();
  }
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void lstm_seq_fwd_kernel(
    float* __restrict__ gates, const float* __restrict__ w_hh, const float* __restrict__ h0,
    const float* __restrict__ c0, const uint8_t* __restrict__ dones, float* __restrict__ out,
    float* __restrict__ c_all, float* __restrict__ hprev, float* __restrict__ hT, float* __restrict__ cT, int S,
    int T) {
  lstm_seq_fwd_body<H, SB>(gates, w_hh, h0, c0, dones, out, c_all, hprev, hT, cT, S, T);
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void lstm_seq_fwd_pair_kernel(LstmFwdArgs a, LstmFwdArgs b, int S, int T) {
  const LstmFwdArgs& p = pair_problem(a, b);
  lstm_seq_fwd_body<H, SB>(p.gates, p.w_hh, p.h0, p.c0, p.dones, p.out, p.c_all, p.hprev, p.hT, p.cT, S, T);
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void lstm_seq_bwd_kernel(
    const float* __restrict__ gates, const float* __restrict__ c_all, const float* __restrict__ c0,
    const uint8_t* __restrict__ dones, const float* __restrict__ w_hh, const float* __restrict__ d_out,
    float* __restrict__ d_gates, int S, int T) {
  lstm_seq_bwd_body<H, SB>(gates, c_all, c0, dones, w_hh, d_out, d_gates, S, T);
}

template <int H, int SB>
__global__ __launch_bounds__(kSeqThreads) void lstm_seq_bwd_pair_kernel(LstmBwdArgs a, LstmBwdArgs b, int S, int T) {
  const LstmBwdArgs& p = pair_problem(a, b);
  lstm_seq_bwd_body<H, SB>(p.gates, p.c_all, p.c0, p.dones, p.w_hh, p.d_out, p.d_gates, S, T);
}

// 128 units: W_hh (256 KB) does not fit LDS; csrc/lstm_wide.hip keeps it in registers as MFMA fragments.
int launch_lstm_fwd_wide(const LstmFwdArgs* problems, int count, int S, int T, hipStream_t st);
int launch_lstm_bwd_wide(const LstmBwdArgs* problems, int count, int S, int T, hipStream_t st);

// kernel families for rnn_seq.hpp's launch_seq
struct LstmFwd {
  using Args = LstmFwdArgs;
  template <int H, int SB>
  static constexpr auto kernel = lstm_seq_fwd_kernel<H, SB>;
  template <int H, int SB>
  static constexpr auto pair_kernel = lstm_seq_fwd_pair_kernel<H, SB>;
  static constexpr size_t lds_floats(int H, int SB) { return static_cast<size_t>(4) * H * H + 2 * SB * H; }
  static constexpr auto wide = launch_lstm_fwd_wide;
};

struct LstmBwd {
  using Args = LstmBwdArgs;
  template <int H, int SB>
  static constexpr auto kernel = lstm_seq_bwd_kernel<H, SB>;
  template <int H, int SB>
  static constexpr auto pair_kernel = lstm_seq_bwd_pair_kernel<H, SB>;
  static constexpr size_t lds_floats(int H, int SB) { return static_cast<size_t>(4) * H * H + SB * 4 * H; }
  static constexpr auto wide = launch_lstm_bwd_wide;
};

// kernel order of the code object: rnn_seq.hpp
static_assert(single_kernels_first<LstmFwd>() && single_kernels_first<LstmBwd>());

}  // namespace rlg

extern "C" {

int rlg_lstm_supported(int hidden) { return rlg::seq_hidden_supported(hidden) ? 1 : 0; }

int rlg_lstm_seq_forward(const rlg_lstm_fwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                         void* stream) {
  return rlg::launch_seq<rlg::LstmFwd>(problems, num_problems, hidden, num_seqs, seq_len, stream);
}

int rlg_lstm_seq_backward(const rlg_lstm_bwd* problems, int num_problems, int num_seqs, int seq_len, int hidden,
                          void* stream) {
  return rlg::launch_seq<rlg::LstmBwd>(problems, num_problems, hidden, num_seqs, seq_len, stream);
}

}  // extern "C"
