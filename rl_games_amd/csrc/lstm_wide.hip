// Sequence-persistent LSTM layer at 128 hidden units, gfx950: the contract of csrc/lstm.hip (same arguments, same
// meaning of gates / c_all / hprev / hT / cT / d_gates, rows ordered seq*T + t, dones[seq*T+t] zeroes the state
// ENTERING step t, one launch for all T steps) for the width whose recurrent weights no longer fit LDS.
//
// W_hh [512, 128] is 256 KB as fp32: more than a CU's 160 KB of LDS, half of its 512 KB register file.  A workgroup of
// 1,024 threads (16 waves, 128 registers per lane) therefore keeps it in REGISTERS, as operand fragments of
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation): 64 registers per lane, fetched once per launch.
//
// Forward, per timestep:  pre[4H x SB] = W_hh[4H x H] . h[H x SB]  for a tile of SB = 16 sequences.
//   * The 512 gate rows are 32 blocks of 16; wave w owns blocks 2w and 2w + 1 (2 blocks x 32 k-steps = 64 A registers,
//     64 MFMAs per step, two independent accumulator chains).
//   * Block b holds hidden units 4b .. 4b + 3, A-fragment row 4u + g = W_hh row g*H + 4b + u.  A lane's D fragment is
//     rows 4q .. 4q + 3 (q = lane / 16) of column lane % 16, i.e. the four gate pre-activations (i, f, g, o) of unit
//     4b + q of ONE sequence: the cell update runs in registers as in lstm.hip, c never leaves them.
//   * k order inside a block is free as long as A and B agree: lane quad q supplies k = 32q + s at MFMA step s, so a
//     lane's B values of a step are 32 consecutive floats of its sequence's h row (8 ds_read_b128) and its A values
//     32 consecutive floats of a W_hh row (8 global 16-byte loads, once).
//   * h goes through a double-buffered LDS tile [2][16][132] (rows padded by 4 floats: conflict-free 16-byte reads),
//     one barrier per step.
// A column of the product depends on its own sequence only, so a sequence's rows are bit-identical whatever shares
// its tile; columns past S repeat sequence S - 1 and store nothing.
//
// Backward, per timestep:  dh_prev[H x SB] = W_hh^T[H x 4H] . dgates[4H x SB]  - the same weights, transposed.
//   * wave w owns the 16 hidden units 16 (w % 8) .. + 15 and the half w / 8 of the 512 gate rows (1 block x 64 k-steps
//     = 64 A registers, 64 MFMAs per step, two accumulator chains over alternate k-steps);
//   * the cell-level arithmetic is thread (unit j = tid % 128, sequences 2 (tid / 128), + 1) exactly as in lstm.hip -
//     global accesses contiguous over j -; its d(gates) tile goes to global memory and to LDS [16][516] (32 KB);
//   * the two half-K partial sums come back through LDS [2][16][132] and are added in a fixed order: deterministic,
//     no atomics.  The product for the state entering step 0 is not needed and not computed.
// Weight gradients stay whole-sequence products outside the kernel.
//
// The tile is 16 sequences for every (S, T): 16 is the MFMA's N, so a smaller tile would not shorten a step (the
// unused columns cost the same cycles), and a 32-sequence tile needs a second set of B registers and accumulators
// that the 128-register budget of a 16-wave workgroup does not have.
//
// Arithmetic: -ffp-contract=off; sigmoid_f / tanhf as in lstm.hip; the only fused multiply-adds are the MFMA's.
// The sum over k runs in a different order from lstm.hip's (4 interleaved partial chains), fp32 throughout.

#include "rlg_device.hpp"

namespace rlg {

constexpr int kWideH = 128;
constexpr int kWideG = 4 * kWideH;
constexpr int kWideSB = 16;                 // sequences per workgroup = N of the MFMA
constexpr int kWideThreads = 1024;          // 16 waves: 4 per SIMD, 128 registers each
constexpr int kWideHP = kWideH + 4;         // padded row of an [SB][H] LDS tile
constexpr int kWideGP = kWideG + 4;         // padded row of the [SB][4H] LDS tile

__device__ __forceinline__ float wide_sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(kWideThreads) void lstm_seq_fwd_wide_kernel(
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

  // A fragments: row i = lane % 16 of blocks 2 wave, 2 wave + 1; k = 32 q + s
  float wreg[2][32];
#pragma unroll
  for (int bb = 0; bb < 2; ++bb) {
    const int b = 2 * wave + bb;
    const int wrow = (n & 3) * H + 4 * b + (n >> 2);
    const f32x4* src = reinterpret_cast<const f32x4*>(w_hh + wrow * H + 32 * q);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const f32x4 x = src[v];
      wreg[bb][4 * v + 0] = x[0];
      wreg[bb][4 * v + 1] = x[1];
      wreg[bb][4 * v + 2] = x[2];
      wreg[bb][4 * v + 3] = x[3];
    }
  }

  const int s_raw = blockIdx.x * kWideSB + n;
  const bool live = s_raw < S;
  const long long seq = live ? s_raw : S - 1;
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
    const float keep = (dones && dones[row]) ? 0.0f : 1.0f;
    float* grow = gates + row * G;
    float gin[2][4];                     // issued ahead of the products: independent of h
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) gin[bb][g] = grow[g * H + j[bb]];
    }
    f32x4 acc[2];
    acc[0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    acc[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4* hb = reinterpret_cast<const f32x4*>(&hcur[n][32 * q]);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const f32x4 hv = hb[v];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[0][4 * v + e], hv[e], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[1][4 * v + e], hv[e], acc[1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      const int u = j[bb];
      const float gi = wide_sigmoid_f(gin[bb][0] + keep * acc[bb][0]);
      const float gf = wide_sigmoid_f(gin[bb][1] + keep * acc[bb][1]);
      const float gg = tanhf(gin[bb][2] + keep * acc[bb][2]);
      const float go = wide_sigmoid_f(gin[bb][3] + keep * acc[bb][3]);
      const float cn = gf * (c[bb] * keep) + gi * gg;
      const float hn = go * tanhf(cn);
      const float hp = hcur[n][u] * keep;
      c[bb] = cn;
      hnext[n][u] = hn;
      if (live) {
        grow[0 * H + u] = gi;
        grow[1 * H + u] = gf;
        grow[2 * H + u] = gg;
        grow[3 * H + u] = go;
        out[row * H + u] = hn;
        if (c_all) c_all[row * H + u] = cn;
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

__global__ __launch_bounds__(kWideThreads) void lstm_seq_bwd_wide_kernel(
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

  // A fragments of W_hh^T: A[i = unit][k = gate row]
  float wreg[64];
#pragma unroll
  for (int s = 0; s < 64; ++s) wreg[s] = 0.0f;
  if (T > 1) {
    const float* src = w_hh + (256 * kh + 64 * q) * H + 16 * mb + n;
#pragma unroll
    for (int s = 0; s < 64; ++s) wreg[s] = src[s * H];
  }

  // cell-level work: unit j of sequences 2 sg, 2 sg + 1
  const int j = tid & (H - 1);
  const int sg = tid >> 7;
  long long seq[2];
  bool live[2];
  float dh_next[2], dc_next[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int s = blockIdx.x * kWideSB + 2 * sg + r;
    live[r] = s < S;
    seq[r] = live[r] ? s : S - 1;
    dh_next[r] = 0.0f;
    dc_next[r] = 0.0f;
  }

  for (int t = T - 1; t >= 0; --t) {
    float keep[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long long row = seq[r] * T + t;
      keep[r] = (dones && dones[row]) ? 0.0f : 1.0f;
      const float* grow = gates + row * G;
      const float gi = grow[0 * H + j], gf = grow[1 * H + j], gg = grow[2 * H + j], go = grow[3 * H + j];
      const float ct = c_all[row * H + j];
      const float c_in = (t > 0 ? c_all[(row - 1) * H + j] : c0[seq[r] * H + j]) * keep[r];
      const float dh = d_out[row * H + j] + dh_next[r];
      const float tc = tanhf(ct);
      const float d_o = dh * tc;
      const float dc = dc_next[r] + (dh * go) * (1.0f - tc * tc);
      const float dgi = (dc * gg) * (gi * (1.0f - gi));
      const float dgf = (dc * c_in) * (gf * (1.0f - gf));
      const float dgg = (dc * gi) * (1.0f - gg * gg);
      const float dgo = d_o * (go * (1.0f - go));
      dc_next[r] = (dc * gf) * keep[r];
      float* db = dgb[2 * sg + r];
      db[0 * H + j] = dgi;
      db[1 * H + j] = dgf;
      db[2 * H + j] = dgg;
      db[3 * H + j] = dgo;
      if (live[r]) {
        float* drow = d_gates + row * G;
        drow[0 * H + j] = dgi;
        drow[1 * H + j] = dgf;
        drow[2 * H + j] = dgg;
        drow[3 * H + j] = dgo;
      }
    }
    if (t == 0) break;                   // nothing consumes d h_{-1}
    __syncthreads();
    f32x4 acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4* bsrc = reinterpret_cast<const f32x4*>(&dgb[n][256 * kh + 64 * q]);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const f32x4 bv = bsrc[v];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 0], bv[0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 1], bv[1], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 2], bv[2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 3], bv[3], acc1, 0, 0, 0);
    }
    // result lane (n, q): units 16 mb + 4 q .. + 3 of sequence n
    *reinterpret_cast<f32x4*>(&dhp[kh][n][16 * mb + 4 * q]) = acc0 + acc1;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) dh_next[r] = (dhp[0][2 * sg + r][j] + dhp[1][2 * sg + r][j]) * keep[r];
  }
}

int launch_lstm_fwd_wide(float* gates, const float* w_hh, const float* h0, const float* c0, const uint8_t* dones,
                         float* out, float* c_all, float* hprev, float* hT, float* cT, int S, int T,
                         hipStream_t st) {
  if ((reinterpret_cast<uintptr_t>(w_hh) & 15u) != 0) return static_cast<int>(hipErrorInvalidValue);
  const int grid = (S + kWideSB - 1) / kWideSB;
  hipLaunchKernelGGL(lstm_seq_fwd_wide_kernel, dim3(grid), dim3(kWideThreads), 0, st, gates, w_hh, h0, c0, dones,
                     out, c_all, hprev, hT, cT, S, T);
  RLG_RETURN_LAUNCH_STATUS();
}

int launch_lstm_bwd_wide(const float* gates, const float* c_all, const float* c0, const uint8_t* dones,
                         const float* w_hh, const float* d_out, float* d_gates, int S, int T, hipStream_t st) {
  const int grid = (S + kWideSB - 1) / kWideSB;
  hipLaunchKernelGGL(lstm_seq_bwd_wide_kernel, dim3(grid), dim3(kWideThreads), 0, st, gates, c_all, c0, dones, w_hh,
                     d_out, d_gates, S, T);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // namespace rlg
