// Sequence-persistent GRU layer at 128 hidden units, gfx950: the contract of csrc/gru.hip (same arguments, same
// meaning of gates / hn_all / hprev / hT / d_gx / d_gh, rows ordered seq*T + t, dones[seq*T+t] zeroes the state
// ENTERING step t, one launch for all T steps) for the width whose recurrent weights no longer fit LDS.
//
// W_hh [384, 128] is 192 KB as fp32: more than a CU's 160 KB of LDS.  As in csrc/lstm_wide.hip a workgroup of 1,024
// threads (16 waves, 128 registers per lane) keeps it in REGISTERS, as operand fragments of v_mfma_f32_16x16x4_f32
// (exact fp32 products, fp32 accumulation), fetched once per launch.
//
// Forward, per timestep:  gh[3H x SB] = W_hh[3H x H] . h[H x SB]  for a tile of SB = 16 sequences.
//   * lstm_wide.hip's row layout with the fourth row of a unit left ZERO: 32 blocks of 16 rows, wave w owns blocks
//     2w and 2w + 1 (2 blocks x 32 k-steps = 64 A registers, 64 MFMAs per step, two independent accumulator chains).
//     Block b holds hidden units 4b .. 4b + 3, A-fragment row 4u + g = W_hh row g*H + 4b + u for g < 3 (r, z, n).
//     A lane's D fragment is rows 4q .. 4q + 3 (q = lane / 16) of column lane % 16, i.e. (W_hr h, W_hz h, W_hn h, 0)
//     of unit 4b + q of ONE sequence: the gate arithmetic and the state update run in registers.  A quarter of the
//     MFMA work multiplies zeros; a step is bound by the latency of its dependent chain, not by MFMA throughput, and
//     a dense 24-block packing would split a unit's three rows over lanes (an LDS round trip per step).
//   * k order, the double-buffered LDS tile of h [2][16][132] and the one barrier per step are lstm_wide.hip's.
// A column of the product depends on its own sequence only, so a sequence's rows are bit-identical whatever shares
// its tile; columns past S take sequence S - 1's state and dones, load no gate inputs (their owner overwrites them in
// the same step) and store nothing.
//
// Backward, per timestep:  dh_prev[H x SB] = dh z + W_hh^T[H x 3H] . d_gh[3H x SB].
//   * wave w owns the 16 hidden units 16 (w % 8) .. + 15 and the half w / 8 of the 384 gate rows: 1 block x 48 k-steps
//     = 48 A registers, no padding, two accumulator chains over alternate k-steps;
//   * the cell-level arithmetic is thread (unit j = tid % 128, sequences 2 (tid / 128), + 1) as in gru.hip - global
//     accesses contiguous over j -; d_gx and d_gh go to global memory, d_gh also to LDS [16][388] (24 KB);
//   * the two half-K partial sums come back through LDS [2][16][132] and are added in a fixed order: deterministic,
//     no atomics.  The product for the state entering step 0 is not needed and not computed.
// Weight gradients stay whole-sequence products outside the kernel.
//
// The tile is 16 sequences for every (S, T), for lstm_wide.hip's reasons: 16 is the MFMA's N, and a 32-sequence tile
// needs a second set of B registers and accumulators that the 128-register budget does not have.
//
// Arithmetic: -ffp-contract=off; the sigmoid / tanhf forms of gru.hip; the only fused multiply-adds are the MFMA's.

#include "rlg_device.hpp"

namespace rlg {

constexpr int kGruWideH = 128;
constexpr int kGruWideG = 3 * kGruWideH;
constexpr int kGruWideSB = 16;                  // sequences per workgroup = N of the MFMA
constexpr int kGruWideThreads = 1024;           // 16 waves: 4 per SIMD, 128 registers each
constexpr int kGruWideHP = kGruWideH + 4;       // padded row of an [SB][H] LDS tile
constexpr int kGruWideGP = kGruWideG + 4;       // padded row of the [SB][3H] LDS tile

__device__ __forceinline__ float gru_wide_sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(kGruWideThreads) void gru_seq_fwd_wide_kernel(
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
  constexpr int H = kGruWideH, G = kGruWideG;
  __shared__ __attribute__((aligned(16))) float hbuf[2][kGruWideSB][kGruWideHP];
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;               // column: sequence of the tile
  const int q = lane >> 4;               // k quarter as an operand lane, unit of the block as a result lane

  // A fragments: row i = lane % 16 = 4u + g of blocks 2 wave, 2 wave + 1; k = 32 q + s; rows with g = 3 are zero
  float wreg[2][32];
  const int ag = n & 3;
#pragma unroll
  for (int bb = 0; bb < 2; ++bb) {
    const int b = 2 * wave + bb;
    const int wrow = (ag < 3 ? ag : 0) * H + 4 * b + (n >> 2);
    const f32x4* src = reinterpret_cast<const f32x4*>(w_hh + wrow * H + 32 * q);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const f32x4 x = src[v];
      wreg[bb][4 * v + 0] = ag < 3 ? x[0] : 0.0f;
      wreg[bb][4 * v + 1] = ag < 3 ? x[1] : 0.0f;
      wreg[bb][4 * v + 2] = ag < 3 ? x[2] : 0.0f;
      wreg[bb][4 * v + 3] = ag < 3 ? x[3] : 0.0f;
    }
  }

  const int s_raw = blockIdx.x * kGruWideSB + n;
  const bool live = s_raw < S;
  const long long seq = live ? s_raw : S - 1;
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
    const float(*hcur)[kGruWideHP] = hbuf[t & 1];
    float(*hnext)[kGruWideHP] = hbuf[(t + 1) & 1];
    const long long row = seq * T + t;
    const float keep = (dones && dones[row]) ? 0.0f : 1.0f;
    float* grow = gates + row * G;
    float gin[2][3];                     // issued ahead of the products: independent of h
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
      for (int g = 0; g < 3; ++g) gin[bb][g] = live ? grow[g * H + j[bb]] : 0.0f;   // (S - 1's owner overwrites these)
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
      const float hp = hcur[n][u] * keep;
      const float gr = gru_wide_sigmoid_f(gin[bb][0] + (keep * acc[bb][0] + bias[bb][0]));
      const float gz = gru_wide_sigmoid_f(gin[bb][1] + (keep * acc[bb][1] + bias[bb][1]));
      const float hn = keep * acc[bb][2] + bias[bb][2];
      const float gn = tanhf(gin[bb][2] + gr * hn);
      const float hnew = (1.0f - gz) * gn + gz * hp;
      hnext[n][u] = hnew;
      if (live) {
        grow[0 * H + u] = gr;
        grow[1 * H + u] = gz;
        grow[2 * H + u] = gn;
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

__global__ __launch_bounds__(kGruWideThreads) void gru_seq_bwd_wide_kernel(
    const float* __restrict__ gates,     // [S*T, 3H] activated gates of the forward pass
    const float* __restrict__ hn_all,    // [S*T, H]
    const float* __restrict__ hprev,     // [S*T, H]
    const uint8_t* __restrict__ dones,   // [S*T] or nullptr
    const float* __restrict__ w_hh,      // [3H, H]
    const float* __restrict__ d_out,     // [S*T, H]  d loss / d h_t (from the layers above)
    float* __restrict__ d_gx,            // [S*T, 3H] d loss / d (x W_ih^T + b_ih)
    float* __restrict__ d_gh,            // [S*T, 3H] d loss / d (h W_hh^T + b_hh)
    int S, int T) {
  constexpr int H = kGruWideH, G = kGruWideG;
  constexpr int KH = G / 2;              // gate rows per wave half: 192
  constexpr int KQ = KH / 4;             // k-steps per wave: 48
  __shared__ __attribute__((aligned(16))) float dgb[kGruWideSB][kGruWideGP];
  __shared__ __attribute__((aligned(16))) float dhp[2][kGruWideSB][kGruWideHP];
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;
  const int q = lane >> 4;
  const int mb = wave & 7;               // hidden units 16 mb .. 16 mb + 15
  const int kh = wave >> 3;              // gate rows 192 kh .. 192 kh + 191; k = 192 kh + 48 q + s

  // A fragments of W_hh^T: A[i = unit][k = gate row]
  float wreg[KQ];
#pragma unroll
  for (int s = 0; s < KQ; ++s) wreg[s] = 0.0f;
  if (T > 1) {
    const float* src = w_hh + (KH * kh + KQ * q) * H + 16 * mb + n;
#pragma unroll
    for (int s = 0; s < KQ; ++s) wreg[s] = src[s * H];
  }

  // cell-level work: unit j of sequences 2 sg, 2 sg + 1
  const int j = tid & (H - 1);
  const int sg = tid >> 7;
  long long seq[2];
  bool live[2];
  float dh_next[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int s = blockIdx.x * kGruWideSB + 2 * sg + r;
    live[r] = s < S;
    seq[r] = live[r] ? s : S - 1;
    dh_next[r] = 0.0f;
  }

  for (int t = T - 1; t >= 0; --t) {
    float keep[2], dhz[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long long row = seq[r] * T + t;
      keep[r] = (dones && dones[row]) ? 0.0f : 1.0f;
      const float* grow = gates + row * G;
      const float gr = grow[0 * H + j], gz = grow[1 * H + j], gn = grow[2 * H + j];
      const float hn = hn_all[row * H + j];
      const float hp = hprev[row * H + j];
      const float dh = d_out[row * H + j] + dh_next[r];
      const float dn = (dh * (1.0f - gz)) * (1.0f - gn * gn);
      const float dz = (dh * (hp - gn)) * (gz * (1.0f - gz));
      const float dr = (dn * hn) * (gr * (1.0f - gr));
      const float dnr = dn * gr;
      dhz[r] = dh * gz;
      float* db = dgb[2 * sg + r];
      db[0 * H + j] = dr;
      db[1 * H + j] = dz;
      db[2 * H + j] = dnr;
      if (live[r]) {
        float* xrow = d_gx + row * G;
        float* hrow = d_gh + row * G;
        xrow[0 * H + j] = dr;
        xrow[1 * H + j] = dz;
        xrow[2 * H + j] = dn;
        hrow[0 * H + j] = dr;
        hrow[1 * H + j] = dz;
        hrow[2 * H + j] = dnr;
      }
    }
    if (t == 0) break;                   // nothing consumes d h_{-1}
    __syncthreads();
    f32x4 acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4* bsrc = reinterpret_cast<const f32x4*>(&dgb[n][KH * kh + KQ * q]);
#pragma unroll
    for (int v = 0; v < KQ / 4; ++v) {
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
    for (int r = 0; r < 2; ++r)
      dh_next[r] = (dhz[r] + (dhp[0][2 * sg + r][j] + dhp[1][2 * sg + r][j])) * keep[r];
  }
}

int launch_gru_fwd_wide(float* gates, const float* w_hh, const float* b_hh, const float* h0, const uint8_t* dones,
                        float* out, float* hn_all, float* hprev, float* hT, int S, int T, hipStream_t st) {
  if ((reinterpret_cast<uintptr_t>(w_hh) & 15u) != 0) return static_cast<int>(hipErrorInvalidValue);
  const int grid = (S + kGruWideSB - 1) / kGruWideSB;
  hipLaunchKernelGGL(gru_seq_fwd_wide_kernel, dim3(grid), dim3(kGruWideThreads), 0, st, gates, w_hh, b_hh, h0, dones,
                     out, hn_all, hprev, hT, S, T);
  RLG_RETURN_LAUNCH_STATUS();
}

int launch_gru_bwd_wide(const float* gates, const float* hn_all, const float* hprev, const uint8_t* dones,
                        const float* w_hh, const float* d_out, float* d_gx, float* d_gh, int S, int T,
                        hipStream_t st) {
  if ((reinterpret_cast<uintptr_t>(w_hh) & 15u) != 0) return static_cast<int>(hipErrorInvalidValue);
  const int grid = (S + kGruWideSB - 1) / kGruWideSB;
  hipLaunchKernelGGL(gru_seq_bwd_wide_kernel, dim3(grid), dim3(kGruWideThreads), 0, st, gates, hn_all, hprev, dones,
                     w_hh, d_out, d_gx, d_gh, S, T);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // namespace rlg
