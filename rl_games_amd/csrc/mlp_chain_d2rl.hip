// Dense-to-dense (D2RL) trunks - `mlp.d2rl: True`, rl_games/algos_torch/d2rl.py: every layer behind the first reads the
// previous layer's output concatenated with the network input - as ONE vertically fused chain per direction on f32 MFMA
// (gfx950).  One workgroup owns one row tile for the whole launch.
//
//   forward :  x -> [RunningMeanStd: fold the minibatch's moments (training), normalise] -> tile Xn in LDS, once, for good
//              H_0 = act(W_0 Xn + b_0),   H_l = act(W_l [H_{l-1} | Xn] + b_l),   heads = W_head H_last + b_head
//   backward:  dZ_last = d heads,  dZ_{l-1} = (dZ_l W_l[:, :u_{l-1}]) * act'(H_{l-1});  no dX of the observations
//
// Product form: EXACT fp32 products on v_mfma_f32_16x16x4_f32, the scheme of csrc/mlp_chain_stream.hpp (operand tiles in
// LDS as [k-chunk][G][64 lanes][4] floats in whole zero-padded k-batches, weights streamed from L2 through bounds-checked
// buffer loads one k-batch ahead, a wave computes a 16-feature output block for all G row groups from one fetch of the
// weight fragment).  A row's result depends on nothing but the row.  No atomics.
//
// What is this file's own:
//   * No concatenation.  LDS = [tile Xn | region A | region B].  Tile Xn is written by the prologue and read by EVERY
//     hidden layer; hidden tile t lives in region A (t even) or B (t odd).  A layer's K loop is two segments: the batches
//     of the previous hidden tile against columns [0, u_{l-1}) of W_l, then the batches of tile Xn against columns
//     [u_{l-1}, u_{l-1} + in0).  Each segment is padded to whole k-batches on its own, so the fragment stream of a block
//     is one sequence of batches with a (tile, weight column) origin per batch - the double-buffered fetch / MFMA
//     pipeline runs across the seam without a bubble.  Layer 0 is the second segment alone, the head the first alone.
//   * Weight rows of stride u + in0.  With in0 off a multiple of 4 a row of W_l does not start on 16 bytes: the
//     fragments of such a layer are fetched as dwords (4 x 64 contiguous bytes per 16 lanes), the others as one 16-byte
//     load per lane.  Nothing is repacked on the host.
//   * Training leaves the weight gradients' operands as they are needed: act_out[l] of a layer that feeds a D2RL layer
//     is the row [H_l | Xn] at its own row stride - H_l from the layer's epilogue, Xn from the prologue, which has the
//     normalised tile in registers anyway.  dW_l = dZ_l^T [H_{l-1} | Xn] is then an ordinary product (csrc/mlp_dw*.hip).
//   * The backward reads the LEFT column block of every W_l only (kT fragments at row stride u + in0); H_{l-1} comes
//     from the concat buffer at that buffer's stride.  Epilogue as csrc/mlp_chain_twin.hip: dZ to the other LDS region
//     and to global memory from the accumulators, fp64 column sums per workgroup, plain stores.  One barrier per layer.
//
// Work split: 256 threads = 4 waves; a tile of 16 G rows, G = 1 / 2 / 4.  LDS, [256, 128, 64] over 60 observations:
// forward (4 + 16 + 8) G KiB = 28 / 56 / 112 KiB, backward 2 x 16 G KiB.  G grows with the rows (2 from 8,192, 4 from 16,384)
// while two workgroups fit a CU's 160 KiB; a network that fits with one group only runs at G = 1.
// Envelope (rlg_mlp_chain_d2rl_supported): 2 - 4 hidden layers, one activation kind (elu / relu / tanh), hidden widths
// multiples of 4 up to 512, an identity head, any observation width that fits, no layer norm.

#include "mlp_chain_stream.hpp"

namespace rlg {

constexpr int kD2MaxLayers = 5;            // up to 4 hidden layers and the head
constexpr int kD2MaxWidth = 512;
constexpr int kD2LdsMax = 160 * 1024;

struct D2Layer {
  const float* w;            // [out, in] row-major; in = u_{l-1} + in0 for the hidden layers behind the first
  const float* bias;         // forward
  float* h;                  // forward: the layer's output ([H_l | Xn] rows in front of a D2RL layer) or nullptr; backward: read
  float* dz;                 // backward: dZ_l, out
  double* bias_partials;     // backward: [gridDim.x, out] or nullptr
  long long ldh, lddz;
  int in, out;
};

struct D2Args {
  D2Layer layer[kD2MaxLayers];
  int num_layers;
  int tile_off[kD2MaxLayers];  // forward: float offset in LDS of hidden tile t
  const float* x;              // raw observations [rows, ldx]
  long long ldx;
  const double* rms_mean;      // RunningMeanStd state or nullptr
  const double* rms_var;
  float rms_eps;
  const double* rms_batch;     // training: fold {sum[in], sumsq[in], rows} into the state first (chain_norm_stats)
  const long long* rms_count;
  double* rms_mean_out;
  double* rms_var_out;
  long long* rms_count_out;
  float* xn;                   // normalised observations out [rows, in0] or nullptr
  const float* d_out;          // backward: d loss / d heads [rows, ld_dout]
  long long ld_dout;
  long long rows;
  int act;                     // the hidden layers' activation
  int in0;
  int scratch_off;             // forward: mean32 / denominator of the normaliser, in region A
  int r2_off;                  // backward: the second operand region (the first starts at 0)
};

// blocks [NOB, NOB rounded up to a k-batch) of an operand tile: zero
template <int G>
__device__ __forceinline__ void d2_zero_pad(float* tile, int width, int wave, int lane) {
  const int NOB = (width + 15) >> 4;
  for (int ob = NOB + wave; ob < ((NOB + 3) & ~3); ob += 4) {
#pragma unroll
    for (int g = 0; g < G; ++g) *reinterpret_cast<f32x4*>(tile + ((ob * G + g) * 64 + lane) * 4) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
}

// The observations of the tile: read once, normalised (mean32 at sc[f], denominator at sc[wp + f]; sc null: as they are),
// into LDS in the operand layout (zero outside), to xn and behind the activations of every concat row [H_l | Xn].
template <int G>
__device__ __forceinline__ void d2_load_obs(const D2Args& a, float* tile, long long row0, long long n_rows, int wave, int lane,
                                            const float* sc, int wp) {
  const int width = a.in0, ncat = a.num_layers - 2;
  const int KC = (((width + 15) >> 4) + 3) & ~3, q4 = 4 * (lane >> 4);
  const bool sv = vec4_ok(a.x, a.ldx), xnv = a.xn != nullptr && vec4_ok(a.xn, width);
  for (int it = wave; it < KC * G; it += 4) {
    const int c = it / G, g = it - c * G, f = c * 16 + q4;
    const long long row = row0 + 16 * g + (lane & 15);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row < n_rows && f < width) {
      v = load_row4(a.x, a.ldx, row, f, width, sv);
      if (sc != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (f + e < width) v[e] = clamp_nan((v[e] - sc[f + e]) / sc[wp + f + e], -5.0f, 5.0f);
        }
      }
      if (a.xn != nullptr) store_row4(a.xn, width, row, f, width, v, xnv);
      for (int L = 0; L < ncat; ++L) {
        if (a.layer[L].h != nullptr) {
          float* dst = a.layer[L].h + a.layer[L].out;
          store_row4(dst, a.layer[L].ldh, row, f, width, v, vec4_ok(dst, a.layer[L].ldh));
        }
      }
    }
    *reinterpret_cast<f32x4*>(tile + ((c * G + g) * 64 + lane) * 4) = v;
  }
}

// The product of one D2RL layer for this wave: blocks ob = wave, wave + 4, ... of the I output features, each for all G row
// groups, over TWO operand segments - tile t1 (K1 features) against columns [0, K1) of W, then tile t2 (K2 features) against
// columns [K1, K1 + K2); either may be empty.  A batch is 4 k-chunks of ONE segment; the fragments of a batch are requested
// one batch ahead, across the seam and across blocks.  ld: row stride of W in floats; vec: 16-byte fragment loads (every row
// of W starts on 16 bytes and K1, K2 are whole 4-float groups), else dwords.
// pre(ob): loads the epilogue needs, issued with the block's first batch; epi(ob, acc): the block's G accumulators.
template <int G, class Pre, class Epi>
__device__ __forceinline__ void d2_product(rsrc_t wr, int I, int ld, bool vec, const float* t1, int K1, const float* t2, int K2,
                                           int wave, int lane, Pre pre, Epi epi) {
  const int NOB = (I + 15) >> 4;
  const int NB1 = (((K1 + 15) >> 4) + 3) >> 2, NBAT = NB1 + ((((K2 + 15) >> 4) + 3) >> 2);
  const int T = ((NOB - wave + 3) >> 2) * NBAT;          // batches of this wave
  if (T <= 0) return;
  const int i16 = lane & 15, q4 = 4 * (lane >> 4);
  f32x4 fa[4], fb[4], acc[G];
  int fj = 0, fbat = 0;                                  // the next batch to request: block wave + 4 fj, batch fbat
  auto fetch = [&](f32x4 (&d)[4]) {
    const bool second = fbat >= NB1;
    const int K = second ? K2 : K1, col0 = second ? K1 : 0, cb0 = 4 * (second ? fbat - NB1 : fbat);
    const int i = (wave + 4 * fj) * 16 + i16;
    const int base = i * ld + col0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k0 = (cb0 + u) * 16 + q4;
      if (vec) {
        d[u] = buf_load4(wr, (i < I && k0 < K) ? static_cast<unsigned>(base + k0) * 4u : kOob);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) d[u][s] = buf_load1(wr, (i < I && k0 + s < K) ? static_cast<unsigned>(base + k0 + s) * 4u : kOob);
      }
    }
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
    const bool second = cb >= NB1;
    const float* tin = second ? t2 : t1;
    const int c0 = 4 * (second ? cb - NB1 : cb);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u;            // (past the segment's last chunk: zero weight fragments, zero chunks of the tile)
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
    // hipcc counts short across branches (csrc/mlp_chain_stream.hpp, tools/audit_mfma.py).  In front of the branch, so that
    // every path out of a batch has them.  (every accumulator passes through the statement)
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

template <int G>
__global__ __launch_bounds__(256) void mlp_chain_d2rl_fwd_kernel(D2Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int r16 = lane & 15, q4 = 4 * (lane >> 4);
  const long long row0 = static_cast<long long>(blockIdx.x) * (16 * G);
  const long long n_rows = pin_s(a.rows);
  const int act = pin_s(a.act), n = pin_s(a.num_layers), in0 = pin_s(a.in0);
  const float* xt = lds;                 // tile Xn: resident to the end of the kernel
  {
    const int in0p = (in0 + 3) & ~3;
    float* sc = a.rms_mean != nullptr ? lds + a.scratch_off : nullptr;
    if (sc != nullptr) {
      chain_norm_stats<4>(a, sc, in0, in0p);
      __syncthreads();
    }
    d2_load_obs<G>(a, lds, row0, n_rows, wave, lane, sc, in0p);
    __syncthreads();                     // (the scratch lies where hidden tile 0 goes: read for the last time above)
  }
  const float* tin = lds;                // the previous hidden tile (layer 0: none, K1 = 0)
  for (int L = 0; L < n; ++L) {
    const D2Layer& ly = a.layer[L];
    const bool last = L == n - 1;
    const int I = pin_s(ly.out), ld = pin_s(ly.in), lact = last ? static_cast<int>(kChIdentity) : act;
    const int K2 = last ? 0 : in0, K1 = ld - K2;
    const float* l_w = pin_s(ly.w);
    const float* l_bias = pin_s(ly.bias);
    float* g_dst = pin_s(ly.h);
    const long long g_ld = pin_s(ly.ldh);
    const bool g_vec = g_dst != nullptr && vec4_ok(g_dst, g_ld);
    float* tout = lds + pin_s(a.tile_off[L]);
    const rsrc_t wr = make_rsrc(l_w, static_cast<unsigned>(I) * static_cast<unsigned>(ld) * 4u);
    const rsrc_t br = make_rsrc(l_bias, l_bias != nullptr ? static_cast<unsigned>(I) * 4u : 0u);
    const bool w_vec = aligned16(l_w) && (ld & 3) == 0;
    const bool b_fast = aligned16(l_bias) && (I & 3) == 0;
    f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
    d2_product<G>(
        wr, I, ld, w_vec, tin, K1, xt, K2, wave, lane, [&](int ob) { bv = sw_ld4(br, ob * 16 + q4, ob * 16 + q4 < I, b_fast); },
        [&](int ob, f32x4(&acc)[G]) {
          const int f = ob * 16 + q4;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            f32x4 v = chain_act4<kChAny>(acc[g] + bv, lact);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = f + e < I ? v[e] : 0.0f;
            if (!last) *reinterpret_cast<f32x4*>(tout + ((ob * G + g) * 64 + lane) * 4) = v;
            const long long row = row0 + 16 * g + r16;
            if (g_dst != nullptr && row < n_rows && f < I) store_row4(g_dst, g_ld, row, f, I, v, g_vec);
          }
        });
    if (!last) d2_zero_pad<G>(tout, I, wave, lane);
    // one barrier per layer: the tile just written is the next operand, the one just read is written again two layers on
    __syncthreads();
    tin = tout;
  }
}

template <int G>
__global__ __launch_bounds__(256) void mlp_chain_d2rl_bwd_kernel(D2Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int r16 = lane & 15, q4 = 4 * (lane >> 4);
  const long long row0 = static_cast<long long>(blockIdx.x) * (16 * G);
  const long long n_rows = pin_s(a.rows);
  const int act = pin_s(a.act), n = pin_s(a.num_layers);
  float* cur = lds;                      // dZ_l, the product's operand
  float* nxt = lds + a.r2_off;           // dZ_{l-1}, written by the product's epilogue
  sw_load_tile<G>(a.d_out, a.ld_dout, a.layer[n - 1].out, row0, n_rows, cur, wave, lane, nullptr, 0, nullptr);
  __syncthreads();
  for (int L = n - 1; L >= 1; --L) {
    // dH_{L-1} = dZ_L W_L[:, :H]: the left column block at the matrix's own row stride, the Xn block is never read
    const int H = pin_s(a.layer[L - 1].out), K = pin_s(a.layer[L].out), ld = pin_s(a.layer[L].in);
    const float* l_w = pin_s(a.layer[L].w);
    const float* l_h = pin_s(a.layer[L - 1].h);
    const long long h_ld = pin_s(a.layer[L - 1].ldh);
    float* l_dz = pin_s(a.layer[L - 1].dz);
    const long long dz_ld = pin_s(a.layer[L - 1].lddz);
    const bool h_vec = vec4_ok(l_h, h_ld), dz_vec = vec4_ok(l_dz, dz_ld);
    double* bpart = pin_s(a.layer[L - 1].bias_partials);
    const long long prow = static_cast<long long>(blockIdx.x) * H;
    const rsrc_t wr = make_rsrc(l_w, static_cast<unsigned>(K) * static_cast<unsigned>(ld) * 4u);
    f32x4 hv[G];
    sw_product<G, true>(
        wr, H, K, ld, false, cur, wave, lane,
        [&](int ob) {                    // H_{L-1} of the block: on its way during the block's MFMAs
          const int f = ob * 16 + q4;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const long long row = row0 + 16 * g + r16;
            hv[g] = (row < n_rows && f < H) ? load_row4(l_h, h_ld, row, f, H, h_vec) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          }
        },
        [&](int ob, f32x4(&acc)[G]) {
          const int f = ob * 16 + q4;
          double sb[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const long long row = row0 + 16 * g + r16;
            const bool ok = row < n_rows && f < H;           // rows behind the minibatch, features behind H: zero
            f32x4 dz = chain_act_grad4(acc[g], hv[g], act);
#pragma unroll
            for (int e = 0; e < 4; ++e) dz[e] = ok ? dz[e] : 0.0f;
            *reinterpret_cast<f32x4*>(nxt + ((ob * G + g) * 64 + lane) * 4) = dz;
            if (ok) store_row4(l_dz, dz_ld, row, f, H, dz, dz_vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) sb[e] += static_cast<double>(row16_sum(dz[e]));
          }
          if (bpart != nullptr && r16 == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (f + e < H) as_global(bpart)[prow + f + e] = sb[e];
            }
          }
        });
    d2_zero_pad<G>(nxt, H, wave, lane);
    __syncthreads();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static long long d2_nb(int w) { return static_cast<long long>(((w + 15) / 16 + 3) & ~3); }      // blocks of a tile: whole k-batches

// 0, hipErrorInvalidValue for a malformed network - one that is no D2RL shape: in[l] == out[l-1] + in[0] for every hidden
// layer behind the first, in[last] == out[last-1] - hipErrorNotSupported for one outside the envelope; *act: the hidden kind
static int d2_check(const rlg_chain_net* net, int* act) {
  if (net == nullptr || net->num_layers < 1 || net->num_layers > kChainMaxLayers || net->in_features == nullptr ||
      net->out_features == nullptr || net->acts == nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  const int n = net->num_layers;
  int kind = 0;
  bool outside = n < 3 || n > kD2MaxLayers;              // 2 - 4 hidden layers and the head
  for (int L = 0; L < n; ++L) {
    if (net->in_features[L] <= 0 || net->out_features[L] <= 0 || net->acts[L] < kChIdentity || net->acts[L] > kChTanh)
      return static_cast<int>(hipErrorInvalidValue);
    if (L > 0) {
      const long long want = static_cast<long long>(net->out_features[L - 1]) + (L + 1 < n ? net->in_features[0] : 0);
      if (net->in_features[L] != want) return static_cast<int>(hipErrorInvalidValue);
    }
    if (L + 1 < n) {
      const int w = net->out_features[L], k = net->acts[L];
      if ((w & 3) != 0 || w > kD2MaxWidth || k == kChIdentity || (kind != 0 && k != kind)) outside = true;
      kind = kind != 0 ? kind : k;
    } else if (net->acts[L] != kChIdentity || net->out_features[L] > kD2MaxWidth) {
      outside = true;
    }
  }
  if ((static_cast<long long>(net->in_features[0]) + kD2MaxWidth) * kD2MaxWidth * 4 >= static_cast<long long>(kOob)) outside = true;
  if (outside) return static_cast<int>(hipErrorNotSupported);
  *act = kind;
  return 0;
}

// LDS bytes at G groups, -1: does not fit.  Forward (direction 0 / 2): tile Xn, region A (the even hidden tiles; the
// normaliser's scratch in front of them), region B (the odd ones).  Backward: two regions, each as large as the widest tile
// (d heads included).
static int d2_lds_plan(const rlg_chain_net* net, int G, int direction, D2Args* args) {
  const long long blk = 256LL * G;
  const int n = net->num_layers;
  long long floats;
  if (direction == 1) {
    long long r = 0;
    for (int L = 0; L < n; ++L) r = d2_nb(net->out_features[L]) > r ? d2_nb(net->out_features[L]) : r;
    floats = 2 * r * blk;
    if (args) args->r2_off = static_cast<int>(r * blk);
  } else {
    const int in0 = net->in_features[0];
    const long long nbx = d2_nb(in0), scratch = 2LL * ((in0 + 3) & ~3);
    long long region[2] = {0, 0};
    for (int L = 0; L + 1 < n; ++L) region[L & 1] = d2_nb(net->out_features[L]) > region[L & 1] ? d2_nb(net->out_features[L]) : region[L & 1];
    const long long pp = (region[0] + region[1]) * blk;
    floats = nbx * blk + (pp > scratch ? pp : scratch);
    if (args && floats * 4 <= kD2LdsMax) {
      for (int L = 0; L + 1 < n; ++L) args->tile_off[L] = static_cast<int>((nbx + ((L & 1) ? region[0] : 0)) * blk);
      args->scratch_off = static_cast<int>(nbx * blk);
    }
  }
  return floats * 4 <= kD2LdsMax ? static_cast<int>(floats * 4) : -1;
}

// The 16-row groups of a launch, chosen as csrc/mlp_chain_twin.hip chooses them: 2 from 8,192 rows, 4 from 16,384, while two
// workgroups fit a CU's LDS; G = 1 whenever it fits at all.  0: no G fits.
static int d2_pick_groups(const rlg_chain_net* net, long long rows, int direction) {
  for (int G = rows >= 16384 ? 4 : (rows >= 8192 ? 2 : 1); G >= 1; G >>= 1) {
    const int bytes = d2_lds_plan(net, G, direction, nullptr);
    if (bytes >= 0 && (G == 1 || bytes <= kD2LdsMax / 2)) return G;
  }
  return 0;
}

// raises the kernels' dynamic-LDS limit, once per process; 0 or the hipError_t of the attribute call (kept)
static int d2_prepare() {
  static const int status = [] {
    const void* kernels[] = {reinterpret_cast<const void*>(mlp_chain_d2rl_fwd_kernel<1>), reinterpret_cast<const void*>(mlp_chain_d2rl_fwd_kernel<2>),
                             reinterpret_cast<const void*>(mlp_chain_d2rl_fwd_kernel<4>), reinterpret_cast<const void*>(mlp_chain_d2rl_bwd_kernel<1>),
                             reinterpret_cast<const void*>(mlp_chain_d2rl_bwd_kernel<2>), reinterpret_cast<const void*>(mlp_chain_d2rl_bwd_kernel<4>)};
    for (const void* k : kernels) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kD2LdsMax);
      if (e != hipSuccess) {
        (void)hipGetLastError();                       // (the launch entries return it; it must not surface in another launch)
        return static_cast<int>(e);
      }
    }
    return 0;
  }();
  return status;
}

// shape, weights and the hidden activation into args; non-zero: a hipError_t
static int d2_fill_net(D2Args& args, const rlg_chain_net* net) {
  args = D2Args{};
  if (const int e = d2_check(net, &args.act)) return e;
  if (net->weights == nullptr) return static_cast<int>(hipErrorInvalidValue);
  args.num_layers = net->num_layers;
  args.in0 = net->in_features[0];
  for (int L = 0; L < net->num_layers; ++L) {
    D2Layer& ly = args.layer[L];
    ly.w = net->weights[L];
    ly.in = net->in_features[L];
    ly.out = net->out_features[L];
    if (ly.w == nullptr || reinterpret_cast<uintptr_t>(ly.w) % 4 != 0) return static_cast<int>(hipErrorInvalidValue);
  }
  return 0;
}

// the groups of a launch and its LDS plan; < 0: minus a hipError_t
static int d2_resolve_groups(const rlg_chain_net* net, const rlg_chain_launch& launch, int direction, D2Args& args, int* lds_bytes) {
  int G = launch.groups;
  if (G == 0) {
    G = d2_pick_groups(net, launch.rows, direction);
    if (G == 0) return -static_cast<int>(hipErrorNotSupported);
  } else if (G != 1 && G != 2 && G != 4) {
    return -static_cast<int>(hipErrorInvalidValue);
  }
  *lds_bytes = d2_lds_plan(net, G, direction, &args);
  if (*lds_bytes < 0) return -static_cast<int>(launch.groups == 0 ? hipErrorNotSupported : hipErrorInvalidValue);
  return G;
}

template <int Dir>
static int d2_launch(int G, int grid, int lds_bytes, const ChainQueue& q, const D2Args& args) {
  if constexpr (Dir == 0) {
    if (G == 4) return chain_launch_kernel(mlp_chain_d2rl_fwd_kernel<4>, grid, 256, lds_bytes, q, args);
    if (G == 2) return chain_launch_kernel(mlp_chain_d2rl_fwd_kernel<2>, grid, 256, lds_bytes, q, args);
    return chain_launch_kernel(mlp_chain_d2rl_fwd_kernel<1>, grid, 256, lds_bytes, q, args);
  } else {
    if (G == 4) return chain_launch_kernel(mlp_chain_d2rl_bwd_kernel<4>, grid, 256, lds_bytes, q, args);
    if (G == 2) return chain_launch_kernel(mlp_chain_d2rl_bwd_kernel<2>, grid, 256, lds_bytes, q, args);
    return chain_launch_kernel(mlp_chain_d2rl_bwd_kernel<1>, grid, 256, lds_bytes, q, args);
  }
}

}  // namespace rlg

// ---------------------------------------------------------------------------------
// C ABI (declared in include/rlg_hip.h)
// ---------------------------------------------------------------------------------
extern "C" {

int rlg_mlp_chain_d2rl_supported(const rlg_chain_net* net, const rlg_chain_ln* ln_or_null, long long rows, int direction) {
  using namespace rlg;
  int act = 0;
  if (direction < 0 || direction > 2 || d2_check(net, &act) != 0) return 0;
  if (ln_or_null != nullptr && ln_or_null->gamma != nullptr) {
    for (int L = 0; L < net->num_layers; ++L) {
      if (ln_or_null->gamma[L] != nullptr) return 0;   // a D2RL trunk with normalisation layers: no station for them here
    }
  }
  // the answer is host arithmetic; a failure of the attribute call is not "outside the envelope": the launch entries report it
  const int G = d2_pick_groups(net, rows, direction);
  if (G > 0) (void)d2_prepare();
  return G;
}

int rlg_mlp_chain_d2rl_forward(const rlg_chain_net* net, const rlg_chain_fwd* fwd, const rlg_chain_launch* launch, void* stream) {
  using namespace rlg;
  if (net == nullptr || fwd == nullptr || launch == nullptr || launch->rows <= 0) return static_cast<int>(hipErrorInvalidValue);
  D2Args args;
  if (const int e = d2_fill_net(args, net)) return e;
  if (fwd->weight_form_or_null != nullptr || fwd->pack_backward_planes_or_null != nullptr) return static_cast<int>(hipErrorNotSupported);
  const int n = net->num_layers;
  const long long rows = launch->rows;
  if (fwd->act_out == nullptr || fwd->act_ld == nullptr || fwd->act_out[n - 1] == nullptr || fwd->x == nullptr ||
      reinterpret_cast<uintptr_t>(fwd->x) % 4 != 0 || fwd->ldx < args.in0)
    return static_cast<int>(hipErrorInvalidValue);
  bool training = false;
  for (int L = 0; L < n; ++L) {
    D2Layer& ly = args.layer[L];
    ly.bias = net->biases ? net->biases[L] : nullptr;
    ly.h = fwd->act_out[L];
    ly.ldh = fwd->act_ld[L];
    // the output of a layer that feeds a D2RL layer is the row [H_l | Xn]
    const long long width = ly.out + (L + 2 < n ? args.in0 : 0);
    if (reinterpret_cast<uintptr_t>(ly.bias) % 4 != 0 || reinterpret_cast<uintptr_t>(ly.h) % 4 != 0 || (ly.h != nullptr && ly.ldh < width))
      return static_cast<int>(hipErrorInvalidValue);
    training = training || (L + 1 < n && ly.h != nullptr);
  }
  args.x = fwd->x;
  args.ldx = fwd->ldx;
  args.rms_mean = fwd->rms_mean_or_null;
  args.rms_var = args.rms_mean ? fwd->rms_var : nullptr;
  if (args.rms_mean != nullptr && args.rms_var == nullptr) return static_cast<int>(hipErrorInvalidValue);
  args.rms_eps = fwd->rms_eps;
  args.rms_batch = args.rms_mean ? fwd->rms_batch_or_null : nullptr;
  if (args.rms_batch != nullptr) {
    const rlg_chain_fwd& f = *fwd;
    if (!f.rms_count || !f.rms_mean_out || !f.rms_var_out || !f.rms_count_out || f.rms_mean_out == args.rms_mean ||
        f.rms_var_out == f.rms_var || f.rms_count_out == f.rms_count)
      return static_cast<int>(hipErrorInvalidValue);      // the fold publishes into a second buffer set
    args.rms_count = f.rms_count;
    args.rms_mean_out = f.rms_mean_out;
    args.rms_var_out = f.rms_var_out;
    args.rms_count_out = f.rms_count_out;
  }
  args.xn = fwd->xn_out_or_null;
  if (reinterpret_cast<uintptr_t>(args.xn) % 4 != 0) return static_cast<int>(hipErrorInvalidValue);
  args.rows = rows;
  int lds_bytes = 0;
  const int G = d2_resolve_groups(net, *launch, training ? 2 : 0, args, &lds_bytes);
  if (G < 0) return -G;
  if (const int e = d2_prepare()) return e;
  const int grid = static_cast<int>((rows + 16 * G - 1) / (16 * G));
  return d2_launch<0>(G, grid, lds_bytes, chain_queue(*launch, stream), args);
}

int rlg_mlp_chain_d2rl_backward(const rlg_chain_net* net, const rlg_chain_bwd* bwd, const rlg_chain_launch* launch, void* stream) {
  using namespace rlg;
  if (net == nullptr || bwd == nullptr || launch == nullptr || launch->rows <= 0) return static_cast<int>(hipErrorInvalidValue);
  if (bwd->maxima_rows_out_or_null) *bwd->maxima_rows_out_or_null = 0;
  D2Args args;
  if (const int e = d2_fill_net(args, net)) return e;
  if (bwd->ppo_loss_or_null != nullptr || bwd->weight_form_or_null != nullptr || bwd->maxima_or_null != nullptr)
    return static_cast<int>(hipErrorNotSupported);
  const int n = net->num_layers;
  const long long rows = launch->rows;
  const rlg_chain_bwd& b = *bwd;
  if (b.d_out == nullptr || b.act_in == nullptr || b.act_ld == nullptr || b.dz_out == nullptr || b.dz_ld == nullptr ||
      reinterpret_cast<uintptr_t>(b.d_out) % 4 != 0 || b.ld_dout < net->out_features[n - 1])
    return static_cast<int>(hipErrorInvalidValue);
  args.d_out = b.d_out;
  args.ld_dout = b.ld_dout;
  for (int L = 0; L + 1 < n; ++L) {
    D2Layer& ly = args.layer[L];
    ly.h = const_cast<float*>(b.act_in[L]);
    ly.ldh = b.act_ld[L];
    ly.dz = b.dz_out[L];
    ly.lddz = b.dz_ld[L];
    ly.bias_partials = b.bias_partials_or_null ? b.bias_partials_or_null[L] : nullptr;
    if (ly.h == nullptr || ly.dz == nullptr || reinterpret_cast<uintptr_t>(ly.h) % 4 != 0 || reinterpret_cast<uintptr_t>(ly.dz) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(ly.bias_partials) % 8 != 0 || ly.ldh < ly.out || ly.lddz < ly.out)
      return static_cast<int>(hipErrorInvalidValue);
  }
  args.rows = rows;
  int lds_bytes = 0;
  const int G = d2_resolve_groups(net, *launch, 1, args, &lds_bytes);
  if (G < 0) return -G;
  if (const int e = d2_prepare()) return e;
  const int grid = static_cast<int>((rows + 16 * G - 1) / (16 * G));
  return d2_launch<1>(G, grid, lds_bytes, chain_queue(*launch, stream), args);
}

}  // extern "C"
