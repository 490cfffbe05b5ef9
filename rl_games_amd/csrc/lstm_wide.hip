// Sequence-persistent LSTM layer at 128 hidden units, gfx950: the contract of csrc/lstm.hip (same arguments, same
// meaning of gates / c_all / hprev / hT / cT / d_gates, one launch for all T steps) for the width whose recurrent
// weights no longer fit LDS.
//
// W_hh [512, 128] is 256 KB as fp32: more than a CU's 160 KB of LDS, half of its 512 KB register file.  A workgroup of
// 1,024 threads (16 waves, 128 registers per lane) therefore keeps it in REGISTERS, as operand fragments of
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation): 64 registers per lane, fetched once per launch.
// The product scheme - fragment layout, k order, LDS tiles, why the tile is always 16 sequences - is rnn_seq.hpp's
// wide scheme with NG = 4: every row of the forward's A blocks is a gate row, and the backward runs KQ = 64 k-steps.
//
// Forward: a lane's D fragment holds the four gate pre-activations (i, f, g, o) of one unit of ONE sequence: the cell
// update runs in registers, c never leaves them.  A column of the product depends on its own sequence only, so a
// sequence's rows are bit-identical whatever shares its tile; columns past S repeat sequence S - 1 and store nothing.
//
// Backward: the cell-level arithmetic is lstm.hip's; its d(gates) tile goes to global memory and to LDS [16][516]
// (32 KB).  The product for the state entering step 0 is not needed and not computed.
// Weight gradients stay whole-sequence products outside the kernel.
//
// Arithmetic: the cell formulas are the ones lstm.hip uses (rnn_seq.hpp).  The sum over k runs in a different order
// from lstm.hip's (4 interleaved partial chains), fp32 throughout.

#include "rnn_seq.hpp"

namespace rlg {

constexpr int kWideG = 4 * kWideH;
constexpr int kWideGP = kWideG + kWidePad;      // padded row of the [SB][4H] LDS tile

// Bodies as functions: the single and the paired kernel run the same code (rnn_seq.hpp, "paired launches").
__device__ __forceinline__ void lstm_seq_fwd_wide_body(
    float* __restrict__ gates,           // [S*T, 4H]  in: x-part + biases, out: activated gates
    const float* __restrict__ w_hh,      // [4H, H], 16-byte aligned
    const float* __restrict__ h0,        // [S, H]
    const float* __restrict__ c0,        // [S, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    float* __restrict__ out,             // [S*T, H]  h_t
    float* __restrict__ c_all,           // [S*T, H]  c_t             (nullptr: not kept)
    float* __restrict__ hprev,           // [S*T, H]  state entering step t, after the reset (nullptr)
    float* __restrict__ hT,              // [S, H] final h (nullptr)
    float* __restrict__ cT,              // [S, H] final c (nullptr)
    int S, int T) {
  constexpr int H = kWideH, G = kWideG;
  __shared__ __attribute__((aligned(16))) float hbuf[2][kWideSB][kWideHP];
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;               // column: sequence of the tile
  const int q = lane >> 4;               // k quarter as an operand lane, unit of the block as a result lane

  float wreg[2][32];
  wide_fwd_load_a<4>(wreg, w_hh, wave, n, q);

  bool live;
  long long seq;
  tile_slot(blockIdx.x * kWideSB + n, S, seq, live);
  int j[2];
  float c[2];
#pragma unroll
  for (int bb = 0; bb < 2; ++bb) {
    j[bb] = 4 * (2 * wave + bb) + q;
    c[bb] = c0[seq * H + j[bb]];
    hbuf[0][n][j[bb]] = h0[seq * H + j[bb]];
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const float(*hcur)[kWideHP] = hbuf[t & 1];
    float(*hnext)[kWideHP] = hbuf[(t + 1) & 1];
    const long long row = seq * T + t;
    const float keep = step_keep(dones, row);
    float* grow = gates + row * G;
    float gin[2][4];                     // issued ahead of the products: independent of h
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) gin[bb][g] = grow[g * H + j[bb]];
    }
    f32x4 acc[2];
    wide_fwd_product(acc, wreg, reinterpret_cast<const f32x4*>(&hcur[n][32 * q]));
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      const int u = j[bb];
      const float a[4] = {acc[bb][0], acc[bb][1], acc[bb][2], acc[bb][3]};
      float g[4];
      const float hn = lstm_fwd_point(gin[bb], 1, a, keep, c[bb], g);
      const float hp = hcur[n][u] * keep;
      hnext[n][u] = hn;
      if (live) {
        grow[0 * H + u] = g[0];
        grow[1 * H + u] = g[1];
        grow[2 * H + u] = g[2];
        grow[3 * H + u] = g[3];
        out[row * H + u] = hn;
        if (c_all) c_all[row * H + u] = c[bb];
        if (hprev) hprev[row * H + u] = hp;
      }
    }
    __syncthreads();
  }
  if (live) {
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      if (hT) hT[seq * H + j[bb]] = hbuf[T & 1][n][j[bb]];
      if (cT) cT[seq * H + j[bb]] = c[bb];
    }
  }
}

__device__ __forceinline__ void lstm_seq_bwd_wide_body(
    const float* __restrict__ gates,     // [S*T, 4H] activated gates of the forward pass
    const float* __restrict__ c_all,     // [S*T, H]
    const float* __restrict__ c0,        // [S, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    const float* __restrict__ w_hh,      // [4H, H]
    const float* __restrict__ d_out,     // [S*T, H]  d loss / d h_t (from the layers above)
    float* __restrict__ d_gates,         // [S*T, 4H] d loss / d gate pre-activations
    int S, int T) {
  constexpr int H = kWideH, G = kWideG;
  __shared__ __attribute__((aligned(16))) float dgb[kWideSB][kWideGP];
  __shared__ __attribute__((aligned(16))) float dhp[2][kWideSB][kWideHP];
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;
  const int q = lane >> 4;
  const int mb = wave & 7;               // hidden units 16 mb .. 16 mb + 15
  const int kh = wave >> 3;              // gate rows 256 kh .. 256 kh + 255; k = 256 kh + 64 q + s

  float wreg[64];
  wide_bwd_load_a<64>(wreg, w_hh, T, mb, kh, n, q);

  // cell-level work: unit j of sequences 2 sg, 2 sg + 1
  const int j = tid & (H - 1);
  const int sg = tid >> 7;
  long long seq[2];
  bool live[2];
  float dh_next[2], dc_next[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    tile_slot(blockIdx.x * kWideSB + 2 * sg + r, S, seq[r], live[r]);
    dh_next[r] = 0.0f;
    dc_next[r] = 0.0f;
  }

  for (int t = T - 1; t >= 0; --t) {
    float keep[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long long row = seq[r] * T + t;
      keep[r] = step_keep(dones, row);
      const float* grow = gates + row * G;
      const float g[4] = {grow[0 * H + j], grow[1 * H + j], grow[2 * H + j], grow[3 * H + j]};
      const float ct = c_all[row * H + j];
      const float c_in = (t > 0 ? c_all[(row - 1) * H + j] : c0[seq[r] * H + j]) * keep[r];
      const float dh = d_out[row * H + j] + dh_next[r];
      float dg[4];
      lstm_bwd_point(g, ct, c_in, dh, keep[r], dc_next[r], dg);
      float* db = dgb[2 * sg + r];
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
    if (t == 0) break;                   // nothing consumes d h_{-1}
    __syncthreads();
    // result lane (n, q): units 16 mb + 4 q .. + 3 of sequence n
    wide_bwd_product<64>(&dhp[kh][n][16 * mb + 4 * q], wreg,
                         reinterpret_cast<const f32x4*>(&dgb[n][256 * kh + 64 * q]));
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) dh_next[r] = (dhp[0][2 * sg + r][j] + dhp[1][2 * sg + r][j]) * keep[r];
  }
}

__global__ __launch_bounds__(kWideThreads) void lstm_seq_fwd_wide_kernel(
    float* __restrict__ gates, const float* __restrict__ w_hh, const float* __restrict__ h0,
    const float* __restrict__ c0, const uint8_t* __restrict__ dones, float* __restrict__ out,
    float* __restrict__ c_all, float* __restrict__ hprev, float* __restrict__ hT, float* __restrict__ cT, int S,
    int T) {
  lstm_seq_fwd_wide_body(gates, w_hh, h0, c0, dones, out, c_all, hprev, hT, cT, S, T);
}

__global__ __launch_bounds__(kWideThreads) void lstm_seq_fwd_wide_pair_kernel(LstmFwdArgs a, LstmFwdArgs b, int S,
                                                                              int T) {
  const LstmFwdArgs& p = pair_problem(a, b);
  lstm_seq_fwd_wide_body(p.gates, p.w_hh, p.h0, p.c0, p.dones, p.out, p.c_all, p.hprev, p.hT, p.cT, S, T);
}

__global__ __launch_bounds__(kWideThreads) void lstm_seq_bwd_wide_kernel(
    const float* __restrict__ gates, const float* __restrict__ c_all, const float* __restrict__ c0,
    const uint8_t* __restrict__ dones, const float* __restrict__ w_hh, const float* __restrict__ d_out,
    float* __restrict__ d_gates, int S, int T) {
  lstm_seq_bwd_wide_body(gates, c_all, c0, dones, w_hh, d_out, d_gates, S, T);
}

__global__ __launch_bounds__(kWideThreads) void lstm_seq_bwd_wide_pair_kernel(LstmBwdArgs a, LstmBwdArgs b, int S,
                                                                              int T) {
  const LstmBwdArgs& p = pair_problem(a, b);
  lstm_seq_bwd_wide_body(p.gates, p.c_all, p.c0, p.dones, p.w_hh, p.d_out, p.d_gates, S, T);
}

int launch_lstm_fwd_wide(const LstmFwdArgs* problems, int count, int S, int T, hipStream_t st) {
  if (!wide_aligned(problems, count)) return static_cast<int>(hipErrorInvalidValue);
  return launch_problems<lstm_seq_fwd_wide_kernel, lstm_seq_fwd_wide_pair_kernel>(problems, count, S, T, kWideSB,
                                                                                  kWideThreads, 0, st);
}

// (no alignment rule: rnn_seq.hpp's list of asymmetries)
int launch_lstm_bwd_wide(const LstmBwdArgs* problems, int count, int S, int T, hipStream_t st) {
  return launch_problems<lstm_seq_bwd_wide_kernel, lstm_seq_bwd_wide_pair_kernel>(problems, count, S, T, kWideSB,
                                                                                  kWideThreads, 0, st);
}

}  // namespace rlg
