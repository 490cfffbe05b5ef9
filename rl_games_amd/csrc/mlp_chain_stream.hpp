// The exact-product scheme that csrc/mlp_chain_ln.hip and csrc/mlp_chain_twin.hip share: activations resident in LDS as
// [k-chunk][G row groups][64 lanes][4] floats in whole zero-padded k-batches, weights streamed from L2 through
// bounds-checked buffer loads one k-batch ahead, every product TRANSPOSED on v_mfma_f32_16x16x4_f32 (i = output feature,
// j = row, k = input feature; operand mapping as in csrc/mlp_chain.hip:1-31).  A workgroup has 4 waves; the 16-feature
// output blocks of a layer are dealt to them (block ob to wave ob & 3), and a wave computes its block for all G row groups
// from ONE fetch of the weight fragment.
#pragma once

#include "mlp_chain_shared.hpp"

namespace rlg {

// 4 consecutive elements [elem, elem + 4) of a vector behind a resource whose bound is the vector's end (zero past it)
__device__ __forceinline__ f32x4 sw_ld4(rsrc_t r, int elem, bool ok, bool fast) {
  if (fast) return buf_load4(r, ok ? static_cast<unsigned>(elem) * 4u : kOob);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = buf_load1(r, ok ? static_cast<unsigned>(elem + e) * 4u : kOob);
  return v;
}

// This lane's A operands of k-chunk c of block ob: A[16 ob + (lane & 15)][16 c + 4 (lane >> 4) + s], s = 0 .. 3; zero outside
// the I x K matrix.  kT = false: A[i][k] = W[i][k] (forward; vec: one 16-byte load, K % 4 == 0); kT = true: A[i][k] = W[k][i]
// (backward: four dword loads, each 64 contiguous bytes per 16 lanes).  ld: row stride of W in floats.
template <bool kT>
__device__ __forceinline__ f32x4 sw_frag(rsrc_t wr, int I, int K, int ld, bool vec, int ob, int c, int lane) {
  const int i = ob * 16 + (lane & 15), k0 = c * 16 + 4 * (lane >> 4);
  if (!kT && vec) return buf_load4(wr, (i < I && k0 < K) ? static_cast<unsigned>(i * ld + k0) * 4u : kOob);
  f32x4 v;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int off = kT ? (k0 + s) * ld + i : i * ld + k0 + s;
    v[s] = buf_load1(wr, (i < I && k0 + s < K) ? static_cast<unsigned>(off) * 4u : kOob);
  }
  return v;
}

// The product of one layer for this wave: blocks ob = wave, wave + 4, ... of the I output features, each for all G row
// groups of the tile `tin` (K features in whole k-batches of 4 chunks, zero behind the K-th), the fragments of a batch
// requested one batch ahead.
// pre(ob): loads the epilogue needs, issued with the block's first batch; epi(ob, acc): the block's G accumulators.
template <int G, bool kT, class Pre, class Epi>
__device__ __forceinline__ void sw_product(rsrc_t wr, int I, int K, int ld, bool vec, const float* tin, int wave, int lane,
                                           Pre pre, Epi epi) {
  const int NOB = (I + 15) >> 4, NBAT = (((K + 15) >> 4) + 3) >> 2;
  const int T = ((NOB - wave + 3) >> 2) * NBAT;          // batches of this wave
  if (T <= 0) return;
  f32x4 fa[4], fb[4], acc[G];
  int fj = 0, fbat = 0;                                  // the next batch to request: block wave + 4 fj, batch fbat
  auto fetch = [&](f32x4 (&d)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = sw_frag<kT>(wr, I, K, ld, vec, wave + 4 * fj, 4 * fbat + u, lane);
    if (++fbat == NBAT) {
      fbat = 0;
      ++fj;
    }
    RLG_PIN();
  };
  int cj = 0, cb = 0;                                    // the batch whose MFMAs issue next
  auto compute = [&](const f32x4 (&av)[4]) {
    const int ob = wave + 4 * cj;
    if (cb == 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      pre(ob);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = 4 * cb + u;        // (past the layer's last chunk: zero weight fragments, zero chunks of the tile)
      f32x4 bv[G];
#pragma unroll
      for (int g = 0; g < G; ++g) bv[g] = *reinterpret_cast<const f32x4*>(tin + ((c * G + g) * 64 + lane) * 4);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][s], bv[g][s], acc[g], 0, 0, 0);
      }
    }
    // 10 wait states between v_mfma_f32_16x16x4_f32 and the first VALU read of its result: not interlocked on gfx950, and
    // hipcc counts short across branches (csrc/mlp_chain.hip, tools/audit_mfma.py).  In front of the branch, so that every
    // path out of a batch has them: 10 cycles per 16 G MFMAs.
    // (every accumulator passes through the statement: it stays behind the batch's last MFMA)
    if constexpr (G == 1) asm volatile("s_nop 7\n\ts_nop 1" : "+a"(acc[0]));
    else if constexpr (G == 2) asm volatile("s_nop 7\n\ts_nop 1" : "+a"(acc[0]), "+a"(acc[1]));
    else asm volatile("s_nop 7\n\ts_nop 1" : "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3]));
    if (++cb == NBAT) {
      cb = 0;
      ++cj;
      epi(ob, acc);
    }
    RLG_PIN();
  };
  fetch(fa);
#pragma unroll 1
  for (int t = 0; t < T; t += 2) {
    if (t + 1 < T) fetch(fb);
    compute(fa);
    if (t + 1 < T) {
      if (t + 2 < T) fetch(fa);
      compute(fb);
    }
  }
}

// rows x features tile of a [rows, ld] array -> LDS in the operand layout, zero outside; norm: the observation normaliser
// (mean32 at sc[f], denominator at sc[wp + f]) on the way, the result to xn as well
template <int G>
__device__ __forceinline__ void sw_load_tile(const float* src, long long ld, int width, long long row0, long long n_rows,
                                             float* tile, int wave, int lane, const float* sc, int wp, float* xn) {
  const int KC = (((width + 15) >> 4) + 3) & ~3, q4 = 4 * (lane >> 4);       // whole k-batches: zero chunks behind the width
  const bool sv = vec4_ok(src, ld), xnv = xn != nullptr && vec4_ok(xn, width);
  for (int it = wave; it < KC * G; it += 4) {
    const int c = it / G, g = it - c * G, f = c * 16 + q4;
    const long long row = row0 + 16 * g + (lane & 15);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row < n_rows && f < width) {
      v = load_row4(src, ld, row, f, width, sv);
      if (sc != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (f + e < width) v[e] = clamp_nan((v[e] - sc[f + e]) / sc[wp + f + e], -5.0f, 5.0f);
        }
      }
      if (xn != nullptr) store_row4(xn, width, row, f, width, v, xnv);
    }
    *reinterpret_cast<f32x4*>(tile + ((c * G + g) * 64 + lane) * 4) = v;
  }
}

}  // namespace rlg
