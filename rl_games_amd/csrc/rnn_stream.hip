// Sequence-persistent LSTM / GRU layer at 256 hidden units, gfx950: rnn_seq.hpp's third product scheme, "streamed".
//
// W_hh [NG*256, 256] is 1 MB (LSTM) / 768 KB (GRU) as fp32: it fits neither a CU's registers nor its LDS, and a split of
// a sequence's gate rows over CUs would need a grid-wide hand-over per timestep.  Sequences are independent, though: a
// workgroup of 1,024 threads keeps a tile of 16 sequences for all T steps, as the narrow and wide schemes do, and
// STREAMS the weights from L2 every timestep.  They arrive as operand fragments of v_mfma_f32_16x16x4_f32 (exact fp32
// products, fp32 accumulation) packed once per weight version in the order each wave consumes them
// (rnn_stream_pack_kernel): a fragment is 64 lanes x 16 bytes = 1 KB, a wave's fragments are contiguous, and a wave walks
// its stream with bounds-checked buffer loads whose only moving part is a constant scalar offset, kStreamFwdDepth / kStreamBwdDepth
// fragments ahead.  The stream is the same every timestep, so the ring simply wraps: the next step's first fragments are in
// flight under this step's cell update.  No grid barrier, no atomics, no traffic between workgroups; the kernels read
// the packed form only.
//
// Forward, per timestep: pre[1024 x 16] = A[1024 x 256] . h[256 x 16].  The rows of A are 64 blocks of 16, wave w owns
// blocks 4w .. 4w + 3 (64 fragments, 256 MFMAs, four independent accumulator chains).  lstm_wide's row order: block b
// holds hidden units 4b .. 4b + 3, A row 4u + g = W_hh row g*256 + 4b + u for g < NG and zero for g >= NG (the GRU's
// fourth row: a quarter of its products multiply zeros, and a unit's gates stay in one lane).  A lane's D fragment is
// the NG pre-activations of unit 16w + 4bb + q of ONE sequence n = lane % 16 (q = lane / 16): the cell update runs in
// registers, c never leaves them.  Lane quad q supplies k = 64q + 4v + e at MFMA (v, e): its B values are consecutive
// floats of its sequence's h row (one ds_read_b128 feeds 16 MFMAs).  h: double-buffered LDS tile [2][16][260].
// The step's gate tile [16][NG*256 + 4] lives in LDS: thread i moves the 16-byte slots i, i + 1024, ... between LDS
// and global memory, row-contiguous in both directions - the activated gates of step t out and, into the same slot, the
// gate inputs of step t + 1 (loaded a step ahead) in.  h_t, c_t / hn and the state entering the step leave as whole
// 1 KB rows too, one per wave (c_t / hn through the tile `aux`).  Two barriers per step: behind the cell update and
// behind the tile exchange; the next step's products run between them.
//
// Backward, per timestep: dh_prev[256 x 16] = W_hh^T[256 x NG*256] . dgates[NG*256 x 16].  Wave w owns the 32 hidden
// units 32 (w % 8) .. + 31 (two blocks) and the half w / 8 of the gate rows: 2 x NG*8 fragments, two accumulator
// chains; lane quad q supplies k = half*G/2 + q*G/8 + 4v + e.  The cell-level arithmetic is thread (unit j = tid % 256,
// sequences 4 (tid / 256) .. + 3): global accesses contiguous over j, its inputs loaded a step ahead, under the
// products.  Its gate gradients go to global memory and to the LDS tile [16][NG*256 + 4] (64 KB for the LSTM); the two
// half-K partial sums come back through LDS [2][16][260] and are added in a fixed order.  The product for the state
// entering step 0 is not needed and not computed.
//
// Tile rule: 16 sequences per workgroup for every (S, T).  16 is the MFMA's N; a 32-sequence tile (a second set of B
// fragments and accumulators, half the L2 bytes per MFMA) is not built: at 256 workgroups, one per CU, a T = 16 forward
// takes 1.16 x (GRU 1.13 x) what it takes at 64, so L2 nearly sustains 1 MB per CU and step (profiles/rnn_stream.txt).
//
// Arithmetic: the cell formulas are rnn_seq.hpp's, unchanged; -ffp-contract=off; a sequence's rows depend on nothing
// but that sequence, slots past S alias sequence S - 1 and store nothing, training and inference forms compute the
// same bits.

#include "rnn_seq.hpp"

namespace rlg {

constexpr int kStreamH = 256;
constexpr int kStreamSB = 16;                     // sequences per workgroup = N of the MFMA
constexpr int kStreamThreads = 1024;              // 16 waves: 4 per SIMD, 128 registers each
constexpr int kStreamWaves = kStreamThreads / kWave;
constexpr int kStreamHP = kStreamH + 4;           // padded row of an [SB][H] LDS tile
constexpr int kStreamFwdDepth = 8;                // fragments in flight per wave: forward
constexpr int kStreamBwdDepth = 2;                // backward (its cell-level inputs of the next step share the registers)
constexpr int kStreamFragFloats = kWave * 4;      // one fragment: 64 lanes x 4 floats = 1 KB
constexpr int kStreamFwdFrags = 64;               // per wave and step: 16 k-chunks x 4 blocks
constexpr int stream_bwd_frags(int ng) { return ng * 16; }          // NG*256/32 k-chunks x 2 blocks
constexpr long long stream_fwd_floats() { return 1LL * kStreamWaves * kStreamFwdFrags * kStreamFragFloats; }
constexpr long long stream_bwd_floats(int ng) { return 1LL * kStreamWaves * stream_bwd_frags(ng) * kStreamFragFloats; }

struct StreamLstm {
  static constexpr int NG = 4;
  using Fwd = LstmFwdArgs;
  using Bwd = LstmBwdArgs;
};
struct StreamGru {
  static constexpr int NG = 3;
  using Fwd = GruFwdArgs;
  using Bwd = GruBwdArgs;
};

using stream_rsrc_t = __amdgpu_buffer_rsrc_t;

// A wave's fragment stream behind a resource whose bound is the stream's end (a load past it returns zero)
__device__ __forceinline__ stream_rsrc_t stream_rsrc(const float* packed, int wave, int frags) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(packed + wave * frags * kStreamFragFloats), 0,
                                           frags * kStreamFragFloats * 4, 0x00020000);
}

__device__ __forceinline__ f32x4 stream_frag(stream_rsrc_t r, unsigned lane_bytes, int frag) {
  // (fragment = 4 KB groups in the scalar offset, 1 KB steps in the instruction's immediate: 16 scalar constants, not 64)
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
      r, lane_bytes + (frag & 3) * kStreamFragFloats * 4, (frag >> 2) * 4 * kStreamFragFloats * 4, 0));
}

template <int D>
__device__ __forceinline__ void stream_fill(f32x4 (&ring)[D], stream_rsrc_t r, unsigned lane_bytes) {
#pragma unroll
  for (int f = 0; f < D; ++f) ring[f] = stream_frag(r, lane_bytes, f);
}

// acc[m] (+)= the wave's NB blocks over NV k-chunks; fragment f = NB v + m sits in ring[f % depth] and is replaced by
// fragment f + depth (mod NF: the next step's).  bsrc: the lane's 4 NV consecutive B floats.
// 10 wait states between v_mfma_f32_16x16x4_f32 and the first VALU read of its result are not interlocked on gfx950 and
// hipcc counts short across branches (tools/audit_mfma.py): the accumulators pass through the s_nop statement.
template <int NB, int NV, int D>
__device__ __forceinline__ void stream_product(f32x4 (&acc)[NB], f32x4 (&ring)[D], stream_rsrc_t r,
                                               unsigned lane_bytes, const float* bsrc) {
  constexpr int NF = NB * NV;
  static_assert(NF % D == 0, "the ring must be in the same state at the start of every step");
#pragma unroll
  for (int m = 0; m < NB; ++m) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bsrc + 4 * v);
#pragma unroll
    for (int m = 0; m < NB; ++m) {
      const int f = NB * v + m;
      const f32x4 av = ring[f % D];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc[m], 0, 0, 0);
      ring[f % D] = stream_frag(r, lane_bytes, (f + D) % NF);
    }
  }
  if constexpr (NB == 2) asm volatile("s_nop 7\n\ts_nop 1" : "+v"(acc[0]), "+v"(acc[1]));
  else asm volatile("s_nop 7\n\ts_nop 1" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
}

// ------------------------------------------------------------------------------------------- pack

// [forward stream | backward stream] from W_hh [NG*256, 256]; one thread per lane of a fragment.
// forward, wave w, fragment 4v + bb, lane (i = lane % 16, q = lane / 16): W_hh[(i % 4)*256 + 16w + 4bb + i / 4][64q + 4v + e]
// (zero for the gate slot i % 4 >= NG); backward, wave (mb = w % 8, kh = w / 8), fragment 2v + m:
// W_hh[kh*G/2 + q*G/8 + 4v + e][32mb + 16m + i].
template <int NG>
__global__ __launch_bounds__(256) void rnn_stream_pack_kernel(const float* __restrict__ w_hh, float* __restrict__ packed) {
  constexpr int H = kStreamH, G = NG * H, NFB = stream_bwd_frags(NG);
  constexpr int fwd_slots = kStreamWaves * kStreamFwdFrags * kWave, bwd_slots = kStreamWaves * NFB * kWave;
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= fwd_slots + bwd_slots) return;
  f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
  if (slot < fwd_slots) {
    const int lane = slot & 63, frag = (slot >> 6) & 63, w = slot >> 12;
    const int i = lane & 15, q = lane >> 4, v = frag >> 2, bb = frag & 3, g = i & 3;
    if (g < NG) x = *reinterpret_cast<const f32x4*>(w_hh + (g * H + 16 * w + 4 * bb + (i >> 2)) * H + 64 * q + 4 * v);
  } else {
    const int s = slot - fwd_slots;
    const int lane = s & 63, frag = (s >> 6) % NFB, w = (s >> 6) / NFB;
    const int i = lane & 15, q = lane >> 4, v = frag >> 1, m = frag & 1, mb = w & 7, kh = w >> 3;
    const float* src = w_hh + (kh * (G / 2) + q * (G / 8) + 4 * v) * H + 32 * mb + 16 * m + i;
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = src[e * H];
  }
  *reinterpret_cast<f32x4*>(packed + 4LL * slot) = x;
}

// ------------------------------------------------------------------------------------------- forward

template <class Cell>
__global__ __launch_bounds__(kStreamThreads) void rnn_stream_fwd_kernel(typename Cell::Fwd a,
                                                                        const float* __restrict__ packed, int S, int T) {
  constexpr int NG = Cell::NG, H = kStreamH, HP = kStreamHP, G = NG * H, GP = G + 4, G4 = G / 4;
  constexpr bool kLstm = NG == 4;
  extern __shared__ __attribute__((aligned(16))) float stream_lds[];
  float(*hbuf)[kStreamSB][HP] = reinterpret_cast<float(*)[kStreamSB][HP]>(stream_lds);                 // [2]
  float(*gt)[GP] = reinterpret_cast<float(*)[GP]>(stream_lds + 2 * kStreamSB * HP);                     // [16]
  float(*aux)[HP] = reinterpret_cast<float(*)[HP]>(stream_lds + 2 * kStreamSB * HP + kStreamSB * GP);   // [16]
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;               // column: sequence of the tile
  const int q = lane >> 4;               // k quarter as an operand lane, unit of the block as a result lane
  const int tile0 = blockIdx.x * kStreamSB;
  float* kept = nullptr;                 // c_all / hn_all
  if constexpr (kLstm) kept = a.c_all;
  else kept = a.hn_all;

  const stream_rsrc_t wr = stream_rsrc(packed, wave, kStreamFwdFrags);
  const unsigned lane_bytes = lane * 16;
  f32x4 ring[kStreamFwdDepth];
  stream_fill(ring, wr, lane_bytes);

  // the cell update's sequence (column n), the tile exchange's NG gate slots and the wave's h row
  long long cseq, hseq, gseq[NG];
  bool clive, hlive, glive[NG];
  int gn[NG], gc[NG];
  tile_slot(tile0 + n, S, cseq, clive);
  tile_slot(tile0 + wave, S, hseq, hlive);
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int idx = tid + kStreamThreads * i;
    gn[i] = idx / G4;
    gc[i] = 4 * (idx - gn[i] * G4);
    tile_slot(tile0 + gn[i], S, gseq[i], glive[i]);
    *reinterpret_cast<f32x4*>(&gt[gn[i]][gc[i]]) = *reinterpret_cast<const f32x4*>(a.gates + gseq[i] * T * G + gc[i]);
  }
  const int hc = 4 * lane;
  *reinterpret_cast<f32x4*>(&hbuf[0][wave][hc]) = *reinterpret_cast<const f32x4*>(a.h0 + hseq * H + hc);
  float c[4], bias[4][3];
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    const int u = 16 * wave + 4 * bb + q;
    if constexpr (kLstm) {
      c[bb] = a.c0[cseq * H + u];
    } else {
#pragma unroll
      for (int g = 0; g < 3; ++g) bias[bb][g] = a.b_hh[g * H + u];
    }
  }
  __syncthreads();
  f32x4 acc[4];
  stream_product<4, 16>(acc, ring, wr, lane_bytes, &hbuf[0][n][64 * q]);

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const bool more = t + 1 < T;
    f32x4 gnext[NG];                     // the gate inputs of step t + 1: a step ahead, independent of h
    if (more) {
#pragma unroll
      for (int i = 0; i < NG; ++i)
        gnext[i] = *reinterpret_cast<const f32x4*>(a.gates + (gseq[i] * T + t + 1) * G + gc[i]);
    }
    const float keep = step_keep(a.dones, cseq * T + t);
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const int u = 16 * wave + 4 * bb + q;
      if constexpr (kLstm) {
        const float pre[4] = {acc[bb][0], acc[bb][1], acc[bb][2], acc[bb][3]};
        float g[4];
        const float hn = lstm_fwd_point(&gt[n][u], H, pre, keep, c[bb], g);
#pragma unroll
        for (int k = 0; k < 4; ++k) gt[n][k * H + u] = g[k];
        hbuf[nxt][n][u] = hn;
        aux[n][u] = c[bb];
      } else {
        const float x[3] = {gt[n][u], gt[n][H + u], gt[n][2 * H + u]};
        const float pre[3] = {acc[bb][0], acc[bb][1], acc[bb][2]};
        const float hp = hbuf[cur][n][u] * keep;
        float g[3], hn;
        const float hnew = gru_fwd_point(x, pre, bias[bb], keep, hp, g, hn);
#pragma unroll
        for (int k = 0; k < 3; ++k) gt[n][k * H + u] = g[k];
        hbuf[nxt][n][u] = hnew;
        aux[n][u] = hn;
      }
    }
    __syncthreads();
    // tile exchange: the activated gates of step t out, the gate inputs of step t + 1 into the same slots
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      f32x4* slot = reinterpret_cast<f32x4*>(&gt[gn[i]][gc[i]]);
      if (glive[i]) *reinterpret_cast<f32x4*>(a.gates + (gseq[i] * T + t) * G + gc[i]) = *slot;
      if (more) *slot = gnext[i];
    }
    if (hlive) {
      const long long row = hseq * T + t;
      *reinterpret_cast<f32x4*>(a.out + row * H + hc) = *reinterpret_cast<const f32x4*>(&hbuf[nxt][wave][hc]);
      if (kept) *reinterpret_cast<f32x4*>(kept + row * H + hc) = *reinterpret_cast<const f32x4*>(&aux[wave][hc]);
      if (a.hprev) {
        const float hkeep = step_keep(a.dones, row);
        const f32x4 hv = *reinterpret_cast<const f32x4*>(&hbuf[cur][wave][hc]);
        *reinterpret_cast<f32x4*>(a.hprev + row * H + hc) = f32x4{hv[0] * hkeep, hv[1] * hkeep, hv[2] * hkeep, hv[3] * hkeep};
      }
    }
    if (more) stream_product<4, 16>(acc, ring, wr, lane_bytes, &hbuf[nxt][n][64 * q]);
    __syncthreads();
  }
  if (hlive) {
    if (a.hT) *reinterpret_cast<f32x4*>(a.hT + hseq * H + hc) = *reinterpret_cast<const f32x4*>(&hbuf[T & 1][wave][hc]);
    if constexpr (kLstm) {
      if (a.cT) *reinterpret_cast<f32x4*>(a.cT + hseq * H + hc) = *reinterpret_cast<const f32x4*>(&aux[wave][hc]);
    }
  }
}

// ------------------------------------------------------------------------------------------- backward

template <class Cell>
__global__ __launch_bounds__(kStreamThreads) void rnn_stream_bwd_kernel(typename Cell::Bwd a,
                                                                        const float* __restrict__ packed, int S, int T) {
  constexpr int NG = Cell::NG, H = kStreamH, HP = kStreamHP, G = NG * H, GP = G + 4;
  constexpr int KH = G / 2, KQ = G / 8, NV = KQ / 4, NF = stream_bwd_frags(NG);
  constexpr bool kLstm = NG == 4;
  static_assert(NF == 2 * NV, "two blocks per k-chunk");
  extern __shared__ __attribute__((aligned(16))) float stream_lds[];
  float(*dgb)[GP] = reinterpret_cast<float(*)[GP]>(stream_lds);                                        // [16]
  float(*dhp)[kStreamSB][HP] = reinterpret_cast<float(*)[kStreamSB][HP]>(stream_lds + kStreamSB * GP);  // [2]
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int n = lane & 15;
  const int q = lane >> 4;
  const int mb = wave & 7;               // hidden units 32 mb .. 32 mb + 31
  const int kh = wave >> 3;              // gate rows KH kh .. KH kh + KH - 1; k = KH kh + KQ q + 4v + e

  const stream_rsrc_t wr = stream_rsrc(packed, wave, NF);
  const unsigned lane_bytes = lane * 16;
  f32x4 ring[kStreamBwdDepth];
  if (T > 1) stream_fill(ring, wr, lane_bytes);
  else {
#pragma unroll
    for (int f = 0; f < kStreamBwdDepth; ++f) ring[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  // cell-level work: unit j of sequences 4 sg .. 4 sg + 3
  const int j = tid & (H - 1);
  const int sg = tid >> 8;
  // (slot r's sequence and liveness are recomputed where they are used: four 64-bit indices less to keep)
  const int slot0 = blockIdx.x * kStreamSB + 4 * sg;
  float dh_next[4], dc_next[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dh_next[r] = 0.0f;
    dc_next[r] = 0.0f;
  }
  // one step's inputs, loaded a step ahead: gates, LSTM (c_t, c entering the step) / GRU (hn, h entering), d_out, keep
  float in_g[4][NG], in_a[4], in_b[4], in_d[4], in_keep[4];
  auto load_step = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      long long sq;
      bool alive;
      tile_slot(slot0 + r, S, sq, alive);
      const long long row = sq * T + t;
      in_keep[r] = step_keep(a.dones, row);
#pragma unroll
      for (int g = 0; g < NG; ++g) in_g[r][g] = a.gates[row * G + g * H + j];
      if constexpr (kLstm) {
        in_a[r] = a.c_all[row * H + j];
        in_b[r] = (t > 0 ? a.c_all[(row - 1) * H + j] : a.c0[sq * H + j]) * in_keep[r];
      } else {
        in_a[r] = a.hn_all[row * H + j];
        in_b[r] = a.hprev[row * H + j];
      }
      in_d[r] = a.d_out[row * H + j];
    }
  };
  load_step(T - 1);

  for (int t = T - 1; t >= 0; --t) {
    float keep[4], dhz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      long long sq;
      bool alive;
      tile_slot(slot0 + r, S, sq, alive);
      const long long row = sq * T + t;
      keep[r] = in_keep[r];
      const float dh = in_d[r] + dh_next[r];
      float* db = dgb[4 * sg + r];
      if constexpr (kLstm) {
        const float g[4] = {in_g[r][0], in_g[r][1], in_g[r][2], in_g[r][3]};
        float dg[4];
        lstm_bwd_point(g, in_a[r], in_b[r], dh, keep[r], dc_next[r], dg);
        dhz[r] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) db[k * H + j] = dg[k];
        if (alive) {
#pragma unroll
          for (int k = 0; k < 4; ++k) a.d_gates[row * G + k * H + j] = dg[k];
        }
      } else {
        const float g[3] = {in_g[r][0], in_g[r][1], in_g[r][2]};
        float dgx[3], dnr;
        dhz[r] = gru_bwd_point(g, in_a[r], in_b[r], dh, dgx, dnr);
        db[0 * H + j] = dgx[0];
        db[1 * H + j] = dgx[1];
        db[2 * H + j] = dnr;
        if (alive) {
          float* xrow = a.d_gx + row * G;
          float* hrow = a.d_gh + row * G;
          xrow[0 * H + j] = dgx[0];
          xrow[1 * H + j] = dgx[1];
          xrow[2 * H + j] = dgx[2];
          hrow[0 * H + j] = dgx[0];
          hrow[1 * H + j] = dgx[1];
          hrow[2 * H + j] = dnr;
        }
      }
    }
    if (t == 0) break;                   // nothing consumes d h_{-1}
    load_step(t - 1);                    // under the products
    __syncthreads();
    f32x4 acc[2];
    stream_product<2, NV>(acc, ring, wr, lane_bytes, &dgb[n][KH * kh + KQ * q]);
    // result lane (n, q): units 32 mb + 16 m + 4 q .. + 3 of sequence n
    *reinterpret_cast<f32x4*>(&dhp[kh][n][32 * mb + 4 * q]) = acc[0];
    *reinterpret_cast<f32x4*>(&dhp[kh][n][32 * mb + 16 + 4 * q]) = acc[1];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float wsum = dhp[0][4 * sg + r][j] + dhp[1][4 * sg + r][j];
      if constexpr (kLstm) dh_next[r] = wsum * keep[r];
      else dh_next[r] = (dhz[r] + wsum) * keep[r];
    }
  }
}

// ------------------------------------------------------------------------------------------- host

template <int NG>
constexpr size_t stream_fwd_lds() {
  return sizeof(float) * (2 * kStreamSB * kStreamHP + kStreamSB * (NG * kStreamH + 4) + kStreamSB * kStreamHP);
}
template <int NG>
constexpr size_t stream_bwd_lds() {
  return sizeof(float) * (kStreamSB * (NG * kStreamH + 4) + 2 * kStreamSB * kStreamHP);
}
static_assert(stream_fwd_lds<4>() <= 160 * 1024 && stream_bwd_lds<4>() <= 160 * 1024, "a CU has 160 KB of LDS");

static bool stream_aligned(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15u) == 0;
}

static int stream_gates(int cell, int hidden) {
  if (hidden != kStreamH) return 0;
  return cell == 0 ? 4 : cell == 1 ? 3 : 0;
}

// One problem; the descriptor's checks are launch_seq's (rnn_seq.hpp), then the 16-byte rule of every array the kernel
// moves 16 bytes at a time.
template <class Cell, class D>
static int stream_forward(const D* problem, const float* packed, int S, int T, hipStream_t st) {
  typename Cell::Fwd p = {};
  static_cast<D&>(p) = *problem;
  if (!p.complete()) return static_cast<int>(hipErrorInvalidValue);
  const float* kept;
  if constexpr (Cell::NG == 4) kept = p.c_all;
  else kept = p.hn_all;
  const float* c_final = nullptr;
  if constexpr (Cell::NG == 4) c_final = p.cT;
  if (!stream_aligned({packed, p.gates, p.h0, p.out, kept, p.hprev, p.hT, c_final}))
    return static_cast<int>(hipErrorInvalidValue);
  return launch_tile<rnn_stream_fwd_kernel<Cell>>(S, kStreamSB, kStreamThreads, stream_fwd_lds<Cell::NG>(), st, p,
                                                   packed, S, T);
}

template <class Cell, class D>
static int stream_backward(const D* problem, const float* packed, int S, int T, hipStream_t st) {
  typename Cell::Bwd p = {};
  static_cast<D&>(p) = *problem;
  if (!p.complete() || !stream_aligned({packed})) return static_cast<int>(hipErrorInvalidValue);
  return launch_tile<rnn_stream_bwd_kernel<Cell>>(S, kStreamSB, kStreamThreads, stream_bwd_lds<Cell::NG>(), st, p,
                                                   packed + stream_fwd_floats(), S, T);
}

}  // namespace rlg

extern "C" {

int rlg_rnn_stream_supported(int cell, int hidden) { return rlg::stream_gates(cell, hidden) != 0 ? 1 : 0; }

long long rlg_rnn_stream_pack_bytes(int cell, int hidden) {
  const int ng = rlg::stream_gates(cell, hidden);
  return ng == 0 ? -1 : 4 * (rlg::stream_fwd_floats() + rlg::stream_bwd_floats(ng));
}

int rlg_rnn_stream_pack(int cell, int hidden, const float* w_hh, void* packed, void* stream) {
  const int ng = rlg::stream_gates(cell, hidden);
  if (ng == 0 || w_hh == nullptr || packed == nullptr || !rlg::stream_aligned({w_hh, packed}))
    return static_cast<int>(hipErrorInvalidValue);
  const int slots = static_cast<int>((rlg::stream_fwd_floats() + rlg::stream_bwd_floats(ng)) / 4);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  float* dst = static_cast<float*>(packed);
  if (ng == 4) hipLaunchKernelGGL(rlg::rnn_stream_pack_kernel<4>, dim3((slots + 255) / 256), dim3(256), 0, st, w_hh, dst);
  else hipLaunchKernelGGL(rlg::rnn_stream_pack_kernel<3>, dim3((slots + 255) / 256), dim3(256), 0, st, w_hh, dst);
  RLG_RETURN_LAUNCH_STATUS();
}

int rlg_rnn_stream_forward(int cell, const void* problem, const void* packed, int num_seqs, int seq_len, int hidden,
                           void* stream) {
  const int ng = rlg::stream_gates(cell, hidden);
  if (problem == nullptr || packed == nullptr || num_seqs <= 0 || seq_len <= 0 || ng == 0)
    return static_cast<int>(hipErrorInvalidValue);
  const float* pk = static_cast<const float*>(packed);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (ng == 4)
    return rlg::stream_forward<rlg::StreamLstm>(static_cast<const rlg_lstm_fwd*>(problem), pk, num_seqs, seq_len, st);
  return rlg::stream_forward<rlg::StreamGru>(static_cast<const rlg_gru_fwd*>(problem), pk, num_seqs, seq_len, st);
}

int rlg_rnn_stream_backward(int cell, const void* problem, const void* packed, int num_seqs, int seq_len, int hidden,
                            void* stream) {
  const int ng = rlg::stream_gates(cell, hidden);
  if (problem == nullptr || packed == nullptr || num_seqs <= 0 || seq_len <= 0 || ng == 0)
    return static_cast<int>(hipErrorInvalidValue);
  const float* pk = static_cast<const float*>(packed);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (ng == 4)
    return rlg::stream_backward<rlg::StreamLstm>(static_cast<const rlg_lstm_bwd*>(problem), pk, num_seqs, seq_len, st);
  return rlg::stream_backward<rlg::StreamGru>(static_cast<const rlg_gru_bwd*>(problem), pk, num_seqs, seq_len, st);
}

}  // extern "C"
