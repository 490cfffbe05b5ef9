// Sequence-persistent GRU layer at 128 hidden units, gfx950: the contract of csrc/gru.hip (same arguments, same
// meaning of gates / hn_all / hprev / hT / d_gx / d_gh, one launch for all T steps) for the width whose recurrent
// weights no longer fit LDS.
//
// W_hh [384, 128] is 192 KB as fp32: more than a CU's 160 KB of LDS.  As in csrc/lstm_wide.hip a workgroup of 1,024
// threads (16 waves, 128 registers per lane) keeps it in REGISTERS, as operand fragments of v_mfma_f32_16x16x4_f32
// (exact fp32 products, fp32 accumulation), fetched once per launch: rnn_seq.hpp's wide scheme with NG = 3.
//
// Forward: the fourth row of every unit in the A blocks is ZERO, so a lane's D fragment is (W_hr h, W_hz h, W_hn h, 0)
// of one unit of ONE sequence: the gate arithmetic and the state update run in registers.  A quarter of the MFMA work
// multiplies zeros; a step is bound by the latency of its dependent chain, not by MFMA throughput, and a dense
// 24-block packing would split a unit's three rows over lanes (an LDS round trip per step).
// A column of the product depends on its own sequence only, so a sequence's rows are bit-identical whatever shares
// its tile; columns past S take sequence S - 1's state and dones, load no gate inputs (their owner overwrites them in
// the same step) and store nothing.
//
// Backward: dh_prev = dh z + W_hh^T . d_gh, KQ = 48 k-steps per wave, no padding.  The cell-level arithmetic is
// gru.hip's; d_gx and d_gh go to global memory, d_gh also to LDS [16][388] (24 KB).  The product for the state
// entering step 0 is not needed and not computed.
// Weight gradients stay whole-sequence products outside the kernel.
//
// Arithmetic: the cell formulas are the ones gru.hip uses (rnn_seq.hpp).

#include "rnn_seq.hpp"

namespace rlg {

constexpr int kGruWideG = 3 * kWideH;
constexpr int kGruWideGP = kGruWideG + kWidePad;   // padded row of the [SB][3H] LDS tile

// Bodies as functions: the single and the paired kernel run the same code (rnn_seq.hpp, "paired launches").
__device__ __forceinline__ void gru_seq_fwd_wide_body(
    float* __restrict__ gates,           // [S*T, 3H]  in: x-part + b_ih, out: activated gates (r, z, n)
    const float* __restrict__ w_hh,      // [3H, H], 16-byte aligned
    const float* __restrict__ b_hh,      // [3H]
    const float* __restrict__ h0,        // [S, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    float* __restrict__ out,             // [S*T, H]  h_t
    float* __restrict__ hn_all,          // [S*T, H]  W_hn h + b_hn    (nullptr: not kept)
    float* __restrict__ hprev,           // [S*T, H]  state entering step t, after the reset (nullptr)
    float* __restrict__ hT,              // [S, H] final h (nullptr)
    int S, int T) {
  constexpr int H = kWideH, G = kGruWideG;
  __shared__ __attribute__((aligned(16))) float hbuf[2][kWideSB][kWideHP];
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;               // column: sequence of the tile
  const int q = lane >> 4;               // k quarter as an operand lane, unit of the block as a result lane

  float wreg[2][32];
  wide_fwd_load_a<3>(wreg, w_hh, wave, n, q);

  bool live;
  long long seq;
  tile_slot(blockIdx.x * kWideSB + n, S, seq, live);
  int j[2];
  float bias[2][3];
#pragma unroll
  for (int bb = 0; bb < 2; ++bb) {
    j[bb] = 4 * (2 * wave + bb) + q;
#pragma unroll
    for (int g = 0; g < 3; ++g) bias[bb][g] = b_hh[g * H + j[bb]];
    hbuf[0][n][j[bb]] = h0[seq * H + j[bb]];
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const float(*hcur)[kWideHP] = hbuf[t & 1];
    float(*hnext)[kWideHP] = hbuf[(t + 1) & 1];
    const long long row = seq * T + t;
    const float keep = step_keep(dones, row);
    float* grow = gates + row * G;
    float gin[2][3];                     // issued ahead of the products: independent of h
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
      for (int g = 0; g < 3; ++g) gin[bb][g] = live ? grow[g * H + j[bb]] : 0.0f;   // (S - 1's owner overwrites these)
    }
    f32x4 acc[2];
    wide_fwd_product(acc, wreg, reinterpret_cast<const f32x4*>(&hcur[n][32 * q]));
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      const int u = j[bb];
      const float hp = hcur[n][u] * keep;
      const float a[3] = {acc[bb][0], acc[bb][1], acc[bb][2]};
      float g[3], hn;
      const float hnew = gru_fwd_point(gin[bb], a, bias[bb], keep, hp, g, hn);
      hnext[n][u] = hnew;
      if (live) {
        grow[0 * H + u] = g[0];
        grow[1 * H + u] = g[1];
        grow[2 * H + u] = g[2];
        out[row * H + u] = hnew;
        if (hn_all) hn_all[row * H + u] = hn;
        if (hprev) hprev[row * H + u] = hp;
      }
    }
    __syncthreads();
  }
  if (live && hT) {
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) hT[seq * H + j[bb]] = hbuf[T & 1][n][j[bb]];
  }
}

__device__ __forceinline__ void gru_seq_bwd_wide_body(
    const float* __restrict__ gates,     // [S*T, 3H] activated gates of the forward pass
    const float* __restrict__ hn_all,    // [S*T, H]
    const float* __restrict__ hprev,     // [S*T, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    const float* __restrict__ w_hh,      // [3H, H]
    const float* __restrict__ d_out,     // [S*T, H]  d loss / d h_t (from the layers above)
    float* __restrict__ d_gx,            // [S*T, 3H] d loss / d (x W_ih^T + b_ih)
    float* __restrict__ d_gh,            // [S*T, 3H] d loss / d (h W_hh^T + b_hh)
    int S, int T) {
  constexpr int H = kWideH, G = kGruWideG;
  constexpr int KH = G / 2;              // gate rows per wave half: 192
  constexpr int KQ = KH / 4;             // k-steps per wave: 48
  __shared__ __attribute__((aligned(16))) float dgb[kWideSB][kGruWideGP];
  __shared__ __attribute__((aligned(16))) float dhp[2][kWideSB][kWideHP];
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;
  const int q = lane >> 4;
  const int mb = wave & 7;               // hidden units 16 mb .. 16 mb + 15
  const int kh = wave >> 3;              // gate rows 192 kh .. 192 kh + 191; k = 192 kh + 48 q + s

  float wreg[KQ];
  wide_bwd_load_a<KQ>(wreg, w_hh, T, mb, kh, n, q);

  // cell-level work: unit j of sequences 2 sg, 2 sg + 1
  const int j = tid & (H - 1);
  const int sg = tid >> 7;
  long long seq[2];
  bool live[2];
  float dh_next[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    tile_slot(blockIdx.x * kWideSB + 2 * sg + r, S, seq[r], live[r]);
    dh_next[r] = 0.0f;
  }

  for (int t = T - 1; t >= 0; --t) {
    float keep[2], dhz[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long long row = seq[r] * T + t;
      keep[r] = step_keep(dones, row);
      const float* grow = gates + row * G;
      const float g[3] = {grow[0 * H + j], grow[1 * H + j], grow[2 * H + j]};
      const float hn = hn_all[row * H + j];
      const float hp = hprev[row * H + j];
      const float dh = d_out[row * H + j] + dh_next[r];
      float dgx[3], dnr;
      dhz[r] = gru_bwd_point(g, hn, hp, dh, dgx, dnr);
      float* db = dgb[2 * sg + r];
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
    if (t == 0) break;                   // nothing consumes d h_{-1}
    __syncthreads();
    // result lane (n, q): units 16 mb + 4 q .. + 3 of sequence n
    wide_bwd_product<KQ>(&dhp[kh][n][16 * mb + 4 * q], wreg,
                         reinterpret_cast<const f32x4*>(&dgb[n][KH * kh + KQ * q]));
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r)
      dh_next[r] = (dhz[r] + (dhp[0][2 * sg + r][j] + dhp[1][2 * sg + r][j])) * keep[r];
  }
}

__global__ __launch_bounds__(kWideThreads) void gru_seq_fwd_wide_kernel(
    float* __restrict__ gates, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
    const float* __restrict__ h0, const uint8_t* __restrict__ dones, float* __restrict__ out,
    float* __restrict__ hn_all, float* __restrict__ hprev, float* __restrict__ hT, int S, int T) {
  gru_seq_fwd_wide_body(gates, w_hh, b_hh, h0, dones, out, hn_all, hprev, hT, S, T);
}

__global__ __launch_bounds__(kWideThreads) void gru_seq_fwd_wide_pair_kernel(GruFwdArgs a, GruFwdArgs b, int S,
                                                                             int T) {
  const GruFwdArgs& p = pair_problem(a, b);
  gru_seq_fwd_wide_body(p.gates, p.w_hh, p.b_hh, p.h0, p.dones, p.out, p.hn_all, p.hprev, p.hT, S, T);
}

__global__ __launch_bounds__(kWideThreads) void gru_seq_bwd_wide_kernel(
    const float* __restrict__ gates, const float* __restrict__ hn_all, const float* __restrict__ hprev,
    const uint8_t* __restrict__ dones, const float* __restrict__ w_hh, const float* __restrict__ d_out,
    float* __restrict__ d_gx, float* __restrict__ d_gh, int S, int T) {
  gru_seq_bwd_wide_body(gates, hn_all, hprev, dones, w_hh, d_out, d_gx, d_gh, S, T);
}

__global__ __launch_bounds__(kWideThreads) void gru_seq_bwd_wide_pair_kernel(GruBwdArgs a, GruBwdArgs b, int S,
                                                                             int T) {
  const GruBwdArgs& p = pair_problem(a, b);
  gru_seq_bwd_wide_body(p.gates, p.hn_all, p.hprev, p.dones, p.w_hh, p.d_out, p.d_gx, p.d_gh, S, T);
}

int launch_gru_fwd_wide(const GruFwdArgs* problems, int count, int S, int T, hipStream_t st) {
  if (!wide_aligned(problems, count)) return static_cast<int>(hipErrorInvalidValue);
  return launch_problems<gru_seq_fwd_wide_kernel, gru_seq_fwd_wide_pair_kernel>(problems, count, S, T, kWideSB,
                                                                                kWideThreads, 0, st);
}

int launch_gru_bwd_wide(const GruBwdArgs* problems, int count, int S, int T, hipStream_t st) {
  if (!wide_aligned(problems, count)) return static_cast<int>(hipErrorInvalidValue);
  return launch_problems<gru_seq_bwd_wide_kernel, gru_seq_bwd_wide_pair_kernel>(problems, count, S, T, kWideSB,
                                                                                kWideThreads, 0, st);
}

}  // namespace rlg
