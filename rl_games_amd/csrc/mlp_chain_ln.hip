// MLP trunks whose layers end in a row normalisation, as a vertically fused chain on f32 MFMA (gfx950):
//
//   forward :  x -> [RunningMeanStd normalise, state as it is] -> (Linear_l -> act -> optional LayerNorm_l) x L -> Linear head
//   backward:  d heads -> (dY_l = dZ_{l+1} W_{l+1} -> LayerNorm backward -> dZ_l = dA_l * act'(A_l)) x L, with the per-workgroup
//              fp64 column partials of dZ_l (bias), dY_l * xhat_l (d gamma) and dY_l (d beta)
//
// the trunk `network.normalization: layer_norm` builds (rl_games/algos_torch/network_builder.py:105-130: Linear, activation,
// LayerNorm(width) per layer; with norm_only_first_layer behind the first layer alone).  Operand mapping of the products as
// in csrc/mlp_chain.hip:1-31: every product TRANSPOSED on v_mfma_f32_16x16x4_f32 (i = output feature, j = row, k = input
// feature), so a layer's result comes out as "lane = (row, 4 consecutive features)" and is the next product's B operand
// after one 16-byte LDS write per lane.  The kernels and their pipeline are this file's own (the first two points live in
// csrc/mlp_chain_stream.hpp, which csrc/mlp_chain_twin.hip shares):
//   * a workgroup of 4 waves owns 16 G rows (G = 1 / 2 / 4).  LDS tile of a layer with nb 16-feature blocks: [nb][G][64 lanes][4]
//     floats.  The 16-feature output blocks of a layer are dealt to the waves (block ob to wave ob & 3); a wave computes its
//     block for all G row groups from ONE fetch of the weight fragment.
//   * the weights stream from L2 through bounds-checked buffer loads (rows / columns outside the matrix: zero) in k-batches
//     of 4 chunks (64 input features, 16 G MFMAs); the fragments of batch t + 1 - which may belong to the wave's next block -
//     are requested before the MFMAs of batch t issue.  A batch is branch-free: an operand tile holds whole batches, and a
//     chunk past the layer's last one multiplies zero fragments with the tile's zero chunks.  The K and feature padding of
//     every tile is exactly zero in LDS.
//   * the row normalisation is a station behind the layer barrier, on the LDS tile: wave g owns row group g; the 4 lanes of a
//     row (lane = row + 16 q) walk the row's blocks and combine their fp64 sums with an xor butterfly (16, 32) - the order is
//     fixed, every lane of a row ends with the same bits, a row's result depends on nothing but the row.  Formulas and their
//     order as in csrc/rnn_layer_norm.hip:5-16 (mean first, then the centred sum of squares; biased variance;
//     rstd = 1 / sqrt(var + eps); backward through xhat = (A - mean) rstd from the kept A, never through y / gamma).
//   * backward: the product leaves dY_l in one LDS region; the row station reads it with A_l (global), the row statistics and
//     gamma and writes dZ_l over the consumed dZ_{l+1} tile, the next product's operand; a column pass in which a wave again
//     owns whole blocks for all G row groups then sums the three partial rows: 16 rows by rotations on the DPP path, the row
//     groups in index order in fp64, one plain vector store per column - no atomics, bit-reproducible.
// Exact fp32 products only: there is no split-fp16 form of these kernels and therefore no operand range limit.

#include "mlp_chain_stream.hpp"

RLG_ABI_SIZE(rlg_chain_ln, 64);

namespace rlg {

struct LnLayer {
  const float* w;            // [out, in] row-major
  const float* bias;         // forward
  const float* gamma;        // nullptr: no normalisation behind this layer
  const float* beta;
  float* h;                  // forward: act_out (y behind a normalisation, else the activation) or nullptr; backward: the same, read
  float* pre;                // normed layers: A, the activation in front of the normalisation (forward: out or nullptr; backward: in)
  float* stats;              // normed layers: (mean, rstd) [rows, 2]
  float* dz;                 // backward: dZ of this layer, out
  double* bias_partials;     // backward: [gridDim.x, out] or nullptr
  double* gamma_partials;
  double* beta_partials;
  long long ldh, ldpre, lddz;
  int in, out, act;
  float eps;
};

struct LnArgs {
  LnLayer layer[kChainMaxLayers];
  int num_layers;
  const float* x;            // forward: raw observations [rows, ldx]; backward: d heads [rows, ldx]
  long long ldx;
  const double* rms_mean;    // forward: RunningMeanStd state or nullptr
  const double* rms_var;
  float rms_eps;
  float* xn;                 // forward: normalised observations out or nullptr
  long long rows;
  int tile_off[kChainMaxLayers + 1];   // forward: float offset in LDS of tile t, the input of layer t
  int scratch_off;                     // forward: mean32 / denominator of the observation normaliser
  int r2_off;                          // backward: the dY region (the dZ region starts at 0)
};

// sum over the 4 lanes of a row (lane = row + 16 q), fp64, all four end with the same bits
__device__ __forceinline__ double ln_quad_sum(double v) {
  v += __shfl_xor(v, 16, kWave);
  v += __shfl_xor(v, 32, kWave);
  return v;
}

template <int G>
__global__ __launch_bounds__(256) void mlp_chain_ln_fwd_kernel(LnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int r16 = lane & 15, q4 = 4 * (lane >> 4);
  const long long row0 = static_cast<long long>(blockIdx.x) * (16 * G);
  const long long n_rows = pin_s(a.rows);
  const int num_layers = pin_s(a.num_layers);
  {
    // mean32 / denominator exactly like rms_apply_kernel mode 0 (running_mean_std.py:112-113), the state as it is
    const int in0 = a.layer[0].in, in0p = (in0 + 3) & ~3;
    float* sc = a.rms_mean != nullptr ? lds + a.scratch_off : nullptr;
    if (sc != nullptr) {
      for (int f = threadIdx.x; f < in0; f += 256) {
        sc[f] = static_cast<float>(a.rms_mean[f]);
        sc[in0p + f] = sqrt_rn(static_cast<float>(a.rms_var[f]) + a.rms_eps);
      }
      __syncthreads();
    }
    sw_load_tile<G>(a.x, a.ldx, in0, row0, n_rows, lds + a.tile_off[0], wave, lane, sc, in0p, a.xn);
    __syncthreads();
  }
  for (int L = 0; L < num_layers; ++L) {
    const bool last = L == num_layers - 1;
    const int K = pin_s(a.layer[L].in), I = pin_s(a.layer[L].out), act = pin_s(a.layer[L].act);
    const float* l_w = pin_s(a.layer[L].w);
    const float* l_bias = pin_s(a.layer[L].bias);
    const float* l_gamma = pin_s(a.layer[L].gamma);
    const bool has_ln = l_gamma != nullptr;
    // the product's epilogue writes A_l: to pre_out in front of a normalisation, else it is the layer's act_out
    float* g_dst = has_ln ? pin_s(a.layer[L].pre) : pin_s(a.layer[L].h);
    const long long g_ld = has_ln ? pin_s(a.layer[L].ldpre) : pin_s(a.layer[L].ldh);
    const bool g_vec = g_dst != nullptr && vec4_ok(g_dst, g_ld);
    const float* tin = lds + pin_s(a.tile_off[L]);
    float* tout = lds + pin_s(a.tile_off[L + 1]);
    const rsrc_t wr = make_rsrc(l_w, static_cast<unsigned>(I) * static_cast<unsigned>(K) * 4u);
    const rsrc_t br = make_rsrc(l_bias, l_bias != nullptr ? static_cast<unsigned>(I) * 4u : 0u);
    const bool w_vec = aligned16(l_w) && (K & 3) == 0;
    const bool b_fast = aligned16(l_bias) && (I & 3) == 0;
    f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
    sw_product<G, false>(
        wr, I, K, K, w_vec, tin, wave, lane, [&](int ob) { bv = sw_ld4(br, ob * 16 + q4, ob * 16 + q4 < I, b_fast); },
        [&](int ob, f32x4(&acc)[G]) {
          const int f = ob * 16 + q4;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            f32x4 v = chain_act4<kChAny>(acc[g] + bv, act);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = f + e < I ? v[e] : 0.0f;
            if (!last) *reinterpret_cast<f32x4*>(tout + ((ob * G + g) * 64 + lane) * 4) = v;
            const long long row = row0 + 16 * g + r16;
            if (g_dst != nullptr && row < n_rows && f < I) store_row4(g_dst, g_ld, row, f, I, v, g_vec);
          }
        });
    if (last) break;
    for (int ob = ((I + 15) >> 4) + wave; ob < ((((I + 15) >> 4) + 3) & ~3); ob += 4) {      // up to a whole k-batch: zero blocks
#pragma unroll
      for (int g = 0; g < G; ++g) *reinterpret_cast<f32x4*>(tout + ((ob * G + g) * 64 + lane) * 4) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    __syncthreads();
    if (!has_ln) continue;
    // ---- the normalisation station: row group g on wave g, in place
    const int H = I, NOB = (H + 15) >> 4;
    const float* l_beta = pin_s(a.layer[L].beta);
    const float eps = a.layer[L].eps;
    float* y_dst = pin_s(a.layer[L].h);
    const long long y_ld = pin_s(a.layer[L].ldh);
    const bool y_vec = y_dst != nullptr && vec4_ok(y_dst, y_ld);
    float* l_stats = pin_s(a.layer[L].stats);
    const rsrc_t gr = make_rsrc(l_gamma, static_cast<unsigned>(H) * 4u), ber = make_rsrc(l_beta, static_cast<unsigned>(H) * 4u);
    const bool p_fast = aligned16(l_gamma) && aligned16(l_beta) && (H & 3) == 0;
    for (int g = wave; g < G; g += 4) {
      float* tg = tout + (g * 64 + lane) * 4;           // block ob of this lane's row: + ob * G * 256
      double s = 0.0;
      for (int ob = 0; ob < NOB; ++ob) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(tg + ob * G * 256);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += ob * 16 + q4 + e < H ? static_cast<double>(v[e]) : 0.0;
      }
      const float mean = static_cast<float>(ln_quad_sum(s) / H);
      double qs = 0.0;
      for (int ob = 0; ob < NOB; ++ob) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(tg + ob * G * 256);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[e] - mean;
          qs += ob * 16 + q4 + e < H ? static_cast<double>(d) * static_cast<double>(d) : 0.0;
        }
      }
      const double var = ln_quad_sum(qs) / H;
      const float rstd = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
      const long long row = row0 + 16 * g + r16;
      for (int ob = 0; ob < NOB; ++ob) {
        const int f = ob * 16 + q4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(tg + ob * G * 256);
        const f32x4 gm = sw_ld4(gr, f, f < H, p_fast), bt = sw_ld4(ber, f, f < H, p_fast);
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = f + e < H ? (v[e] - mean) * rstd * gm[e] + bt[e] : 0.0f;
        *reinterpret_cast<f32x4*>(tg + ob * G * 256) = y;
        if (y_dst != nullptr && row < n_rows && f < H) store_row4(y_dst, y_ld, row, f, H, y, y_vec);
      }
      if (l_stats != nullptr && q4 == 0 && row < n_rows) {
        as_global(l_stats)[row * 2] = mean;
        as_global(l_stats)[row * 2 + 1] = rstd;
      }
    }
    __syncthreads();
  }
}

template <int G>
__global__ __launch_bounds__(256) void mlp_chain_ln_bwd_kernel(LnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int r16 = lane & 15, q4 = 4 * (lane >> 4);
  const long long row0 = static_cast<long long>(blockIdx.x) * (16 * G);
  const long long n_rows = pin_s(a.rows);
  const int num_layers = pin_s(a.num_layers);
  float* tz = lds;                       // dZ_{l+1}, the product's operand; the row station puts dZ_l there
  float* ty = lds + a.r2_off;            // dY_l, the product's result
  sw_load_tile<G>(a.x, a.ldx, a.layer[num_layers - 1].out, row0, n_rows, tz, wave, lane, nullptr, 0, nullptr);
  __syncthreads();
  for (int L = num_layers - 1; L >= 1; --L) {
    const int p = L - 1;
    const int H = pin_s(a.layer[L].in), K = pin_s(a.layer[L].out), NOB = (H + 15) >> 4;
    const float* l_w = pin_s(a.layer[L].w);
    const rsrc_t wr = make_rsrc(l_w, static_cast<unsigned>(H) * static_cast<unsigned>(K) * 4u);
    sw_product<G, true>(
        wr, H, K, H, false, tz, wave, lane, [](int) {},
        [&](int ob, f32x4(&acc)[G]) {
#pragma unroll
          for (int g = 0; g < G; ++g) *reinterpret_cast<f32x4*>(ty + ((ob * G + g) * 64 + lane) * 4) = acc[g];
        });
    __syncthreads();
    const int act = pin_s(a.layer[p].act);
    const float* l_gamma = pin_s(a.layer[p].gamma);
    const bool has_ln = l_gamma != nullptr;
    const float* l_a = has_ln ? pin_s(a.layer[p].pre) : pin_s(a.layer[p].h);        // A_p: the layer's activation
    const long long a_ld = has_ln ? pin_s(a.layer[p].ldpre) : pin_s(a.layer[p].ldh);
    const float* l_stats = pin_s(a.layer[p].stats);
    float* l_dz = pin_s(a.layer[p].dz);
    const long long dz_ld = pin_s(a.layer[p].lddz);
    const rsrc_t gr = make_rsrc(l_gamma, has_ln ? static_cast<unsigned>(H) * 4u : 0u);
    const bool p_fast = aligned16(l_gamma);
    // ---- row station: dY -> dA (through the normalisation) -> dZ = dA * act'(A); rows behind the minibatch: zero
    for (int g = wave; g < G; g += 4) {
      const long long row = row0 + 16 * g + r16;
      const bool ok = row < n_rows;
      const float* yg = ty + (g * 64 + lane) * 4;
      float* zg = tz + (g * 64 + lane) * 4;
      float mean = 0.0f, rstd = 0.0f, m1 = 0.0f, m2 = 0.0f;
      if (has_ln) {
        if (ok) {
          mean = as_global(l_stats)[row * 2];
          rstd = as_global(l_stats)[row * 2 + 1];
        }
        double s1 = 0.0, s2 = 0.0;
        for (int ob = 0; ob < NOB; ++ob) {
          const int f = ob * 16 + q4;
          if (f < H) {
            const f32x4 dy = *reinterpret_cast<const f32x4*>(yg + ob * G * 256);
            const f32x4 av = ok ? load_row4(l_a, a_ld, row, f, H, true) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const f32x4 gm = sw_ld4(gr, f, true, p_fast);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float gk = dy[e] * gm[e], xh = (av[e] - mean) * rstd;
              s1 += static_cast<double>(gk);
              s2 += static_cast<double>(gk) * static_cast<double>(xh);
            }
          }
        }
        m1 = static_cast<float>(ln_quad_sum(s1) / H);
        m2 = static_cast<float>(ln_quad_sum(s2) / H);
      }
      for (int ob = 0; ob < ((NOB + 3) & ~3); ++ob) {          // (the next product's operand: whole k-batches, zero behind H)
        const int f = ob * 16 + q4;
        f32x4 dz = {0.0f, 0.0f, 0.0f, 0.0f};
        if (f < H && ok) {
          f32x4 d = *reinterpret_cast<const f32x4*>(yg + ob * G * 256);
          const f32x4 av = load_row4(l_a, a_ld, row, f, H, true);
          if (has_ln) {
            const f32x4 gm = sw_ld4(gr, f, true, p_fast);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float gk = d[e] * gm[e], xh = (av[e] - mean) * rstd;
              d[e] = rstd * (gk - m1 - xh * m2);
            }
          }
          dz = chain_act_grad4(d, av, act);
          store_row4(l_dz, dz_ld, row, f, H, dz, true);
        }
        *reinterpret_cast<f32x4*>(zg + ob * G * 256) = dz;
      }
    }
    __syncthreads();
    // ---- column pass: a wave owns whole blocks again; 16 rows by DPP rotations, the row groups in index order in fp64
    double* bpart = pin_s(a.layer[p].bias_partials);
    double* gpart = pin_s(a.layer[p].gamma_partials);
    double* bepart = pin_s(a.layer[p].beta_partials);
    const long long prow = static_cast<long long>(blockIdx.x) * H;
    for (int ob = wave; ob < NOB; ob += 4) {
      const int f = ob * 16 + q4;
      double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0}, se[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const long long row = row0 + 16 * g + r16;
        const bool ok = row < n_rows && f < H;
        const f32x4 dz = *reinterpret_cast<const f32x4*>(tz + ((ob * G + g) * 64 + lane) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) sb[e] += static_cast<double>(row16_sum(dz[e]));
        if (has_ln) {
          const f32x4 dy = *reinterpret_cast<const f32x4*>(ty + ((ob * G + g) * 64 + lane) * 4);
          f32x4 av = {0.0f, 0.0f, 0.0f, 0.0f};
          float mean = 0.0f, rstd = 0.0f;
          if (ok) {
            av = load_row4(l_a, a_ld, row, f, H, true);
            mean = as_global(l_stats)[row * 2];
            rstd = as_global(l_stats)[row * 2 + 1];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float dye = ok ? dy[e] : 0.0f;
            sg[e] += static_cast<double>(row16_sum(dye * ((av[e] - mean) * rstd)));
            se[e] += static_cast<double>(row16_sum(dye));
          }
        }
      }
      if (r16 == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (f + e < H) {
            if (bpart != nullptr) as_global(bpart)[prow + f + e] = sb[e];
            if (has_ln && gpart != nullptr) as_global(gpart)[prow + f + e] = sg[e];
            if (has_ln && bepart != nullptr) as_global(bepart)[prow + f + e] = se[e];
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
constexpr int kLnLdsMax = 160 * 1024;

// Rows decide how many 16-row groups a workgroup would like (as for the other chain kernels: 16-row workgroups keep every
// CU busy below 8,192 rows); the LDS decides how many it gets.
static int ln_groups_wanted(long long rows) { return rows >= 16384 ? 4 : (rows >= 8192 ? 2 : 1); }

// LDS bytes at G groups, -1: does not fit.  Forward (direction 0 / 2): even tiles grow from the bottom, odd ones end at the
// top, so the need is the input tile plus the output tile of the widest adjacent pair (the head's output is not staged);
// the normaliser's scratch sits behind the first tile.  Backward: the dZ region takes every tile, the dY region the hidden.
static int ln_lds_plan(int num_layers, const int* in_features, const int* out_features, int G, int direction, LnArgs* args) {
  const long long blk = 256LL * G;
  auto nb = [](int w) { return static_cast<long long>(((w + 15) / 16 + 3) & ~3); };      // tiles hold whole k-batches of 4 blocks
  long long floats;
  if (direction == 1) {
    long long r1 = 0, r2 = 0;
    for (int L = 0; L < num_layers; ++L) {
      r1 = nb(out_features[L]) > r1 ? nb(out_features[L]) : r1;
      if (L + 1 < num_layers) r2 = nb(out_features[L]) > r2 ? nb(out_features[L]) : r2;
    }
    floats = (r1 + r2) * blk;
    if (floats * 4 > kLnLdsMax) return -1;
    if (args) args->r2_off = static_cast<int>(r1 * blk);
  } else {
    long long pair = nb(in_features[0]);
    for (int t = 0; t + 1 < num_layers; ++t) {
      const long long s = nb(in_features[t]) + nb(out_features[t]);
      pair = s > pair ? s : pair;
    }
    const long long scratch = 2LL * ((in_features[0] + 3) & ~3);
    const long long with_scratch = nb(in_features[0]) * blk + scratch;
    floats = pair * blk > with_scratch ? pair * blk : with_scratch;
    if (floats * 4 > kLnLdsMax) return -1;
    if (args) {
      for (int t = 0; t < num_layers; ++t)
        args->tile_off[t] = (t & 1) ? static_cast<int>((pair - nb(in_features[t])) * blk) : 0;
      args->tile_off[num_layers] = 0;                    // (the head's output: not staged)
      args->scratch_off = static_cast<int>(floats - scratch);
    }
  }
  return static_cast<int>(floats * 4);
}

static bool ln_shape_ok(int num_layers, const int* in_features, const int* out_features) {
  if (num_layers < 1 || num_layers > kChainMaxLayers || in_features == nullptr || out_features == nullptr) return false;
  for (int L = 0; L < num_layers; ++L) {
    if (in_features[L] <= 0 || out_features[L] <= 0 || (L > 0 && in_features[L] != out_features[L - 1])) return false;
    if (L + 1 < num_layers && (out_features[L] & 3) != 0) return false;           // hidden widths: whole 4-float groups
    if (static_cast<long long>(in_features[L]) * out_features[L] * 4 >= static_cast<long long>(kOob)) return false;
  }
  return true;
}

static int ln_pick_groups(int num_layers, const int* in_features, const int* out_features, long long rows, int direction) {
  if (!ln_shape_ok(num_layers, in_features, out_features) || direction < 0 || direction > 2) return 0;
  if (direction == 1 && num_layers < 2) return 0;
  for (int G = ln_groups_wanted(rows); G >= 1; G >>= 1) {
    if (ln_lds_plan(num_layers, in_features, out_features, G, direction, nullptr) >= 0) return G;
  }
  return 0;
}

// Raises the kernels' dynamic-LDS limit, once per process (a function-local static: initialised by one thread); the answer -
// 0 or the hipError_t of the attribute call - is kept, so every launch entry reports a failure as what it is.  Not a stream
// operation; rlg_mlp_chain_ln_groups makes the call too, so that a caller can have it made outside a stream capture.
static int ln_prepare() {
  static const int status = [] {
    const void* kernels[] = {reinterpret_cast<const void*>(mlp_chain_ln_fwd_kernel<1>), reinterpret_cast<const void*>(mlp_chain_ln_fwd_kernel<2>),
                             reinterpret_cast<const void*>(mlp_chain_ln_fwd_kernel<4>), reinterpret_cast<const void*>(mlp_chain_ln_bwd_kernel<1>),
                             reinterpret_cast<const void*>(mlp_chain_ln_bwd_kernel<2>), reinterpret_cast<const void*>(mlp_chain_ln_bwd_kernel<4>)};
    for (const void* k : kernels) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLnLdsMax);
      if (e != hipSuccess) {
        (void)hipGetLastError();                       // (the launch entries return it; it must not surface in another launch)
        return static_cast<int>(e);
      }
    }
    return 0;
  }();
  return status;
}

static bool ln_vec4_host(const void* p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (ld & 3) == 0; }

// the network half of LnArgs; non-zero: a hipError_t
static int ln_fill_net(LnArgs& args, const rlg_chain_net& net, const rlg_chain_ln& ln) {
  if (!ln_shape_ok(net.num_layers, net.in_features, net.out_features)) {
    // a malformed network is an error, one outside the envelope (a hidden width of 18) is declined
    if (net.num_layers < 1 || net.num_layers > kChainMaxLayers || net.in_features == nullptr || net.out_features == nullptr)
      return static_cast<int>(hipErrorInvalidValue);
    return static_cast<int>(hipErrorNotSupported);
  }
  if (net.weights == nullptr || net.acts == nullptr) return static_cast<int>(hipErrorInvalidValue);
  args = LnArgs{};
  args.num_layers = net.num_layers;
  for (int L = 0; L < net.num_layers; ++L) {
    LnLayer& ly = args.layer[L];
    ly.w = net.weights[L];
    ly.in = net.in_features[L];
    ly.out = net.out_features[L];
    ly.act = net.acts[L];
    if (ly.w == nullptr || reinterpret_cast<uintptr_t>(ly.w) % 4 != 0 || ly.act < kChIdentity || ly.act > kChTanh)
      return static_cast<int>(hipErrorInvalidValue);
    ly.gamma = ln.gamma ? ln.gamma[L] : nullptr;
    if (ly.gamma != nullptr) {
      if (L + 1 == net.num_layers || ln.beta == nullptr || ln.beta[L] == nullptr || ln.eps == nullptr || !(ln.eps[L] >= 0.0f) ||
          reinterpret_cast<uintptr_t>(ly.gamma) % 4 != 0 || reinterpret_cast<uintptr_t>(ln.beta[L]) % 4 != 0)
        return static_cast<int>(hipErrorInvalidValue);
      ly.beta = ln.beta[L];
      ly.eps = ln.eps[L];
    }
  }
  return 0;
}

static int ln_resolve_groups(const rlg_chain_net& net, const rlg_chain_launch& launch, int direction, LnArgs& args, int* lds_bytes) {
  int G = launch.groups;
  if (G == 0) {
    G = ln_pick_groups(net.num_layers, net.in_features, net.out_features, launch.rows, direction);
    if (G == 0) return -static_cast<int>(hipErrorNotSupported);
  } else if (G != 1 && G != 2 && G != 4) {
    return -static_cast<int>(hipErrorInvalidValue);
  }
  *lds_bytes = ln_lds_plan(net.num_layers, net.in_features, net.out_features, G, direction, &args);
  if (*lds_bytes < 0) return -static_cast<int>(launch.groups == 0 ? hipErrorNotSupported : hipErrorInvalidValue);
  return G;
}

}  // namespace rlg

// ---------------------------------------------------------------------------------
// C ABI (declared in include/rlg_hip.h)
// ---------------------------------------------------------------------------------
extern "C" {

int rlg_mlp_chain_ln_groups(int num_layers, const int* in_features, const int* out_features, long long rows, int direction) {
  // the answer is host arithmetic; a failure of the attribute call is not "outside the envelope": the launch entries report it
  const int G = rlg::ln_pick_groups(num_layers, in_features, out_features, rows, direction);
  if (G > 0) (void)rlg::ln_prepare();
  return G;
}

int rlg_mlp_chain_ln_forward(const rlg_chain_net* net, const rlg_chain_fwd* fwd, const rlg_chain_ln* ln,
                             const rlg_chain_launch* launch, void* stream) {
  using namespace rlg;
  if (net == nullptr || fwd == nullptr || ln == nullptr || launch == nullptr) return static_cast<int>(hipErrorInvalidValue);
  if (fwd->rms_batch_or_null != nullptr || fwd->weight_form_or_null != nullptr || fwd->pack_backward_planes_or_null != nullptr)
    return static_cast<int>(hipErrorNotSupported);
  const long long rows = launch->rows;
  if (rows <= 0) return 0;
  LnArgs args;
  if (const int e = ln_fill_net(args, *net, *ln)) return e;
  const int n = net->num_layers;
  if (fwd->act_out == nullptr || fwd->act_ld == nullptr || fwd->act_out[n - 1] == nullptr || fwd->x == nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  for (int L = 0; L < n; ++L) {
    LnLayer& ly = args.layer[L];
    ly.bias = net->biases ? net->biases[L] : nullptr;
    if (reinterpret_cast<uintptr_t>(ly.bias) % 4 != 0) return static_cast<int>(hipErrorInvalidValue);
    ly.h = fwd->act_out[L];
    ly.ldh = fwd->act_ld[L];
    if (ly.gamma != nullptr) {
      ly.pre = ln->pre_out ? ln->pre_out[L] : nullptr;
      ly.ldpre = (ly.pre != nullptr && ln->pre_ld) ? ln->pre_ld[L] : 0;
      ly.stats = ln->stats ? ln->stats[L] : nullptr;
      if ((ly.pre != nullptr && ly.ldpre < ly.out) || reinterpret_cast<uintptr_t>(ly.stats) % 4 != 0)
        return static_cast<int>(hipErrorInvalidValue);
    }
    if (ly.h != nullptr && ly.ldh < ly.out) return static_cast<int>(hipErrorInvalidValue);
  }
  args.x = fwd->x;
  args.ldx = fwd->ldx;
  args.rms_mean = fwd->rms_mean_or_null;
  args.rms_var = args.rms_mean ? fwd->rms_var : nullptr;
  if (args.rms_mean != nullptr && args.rms_var == nullptr) return static_cast<int>(hipErrorInvalidValue);
  args.rms_eps = fwd->rms_eps;
  args.xn = fwd->xn_out_or_null;
  args.rows = rows;
  bool training = false;
  for (int L = 0; L + 1 < n; ++L) training = training || args.layer[L].h != nullptr;
  int lds_bytes = 0;
  const int G = ln_resolve_groups(*net, *launch, training ? 2 : 0, args, &lds_bytes);
  if (G < 0) return -G;
  if (const int e = ln_prepare()) return e;
  const int grid = static_cast<int>((rows + 16 * G - 1) / (16 * G));
  const ChainQueue q = chain_queue(*launch, stream);
  if (G == 4) return chain_launch_kernel(mlp_chain_ln_fwd_kernel<4>, grid, 256, lds_bytes, q, args);
  if (G == 2) return chain_launch_kernel(mlp_chain_ln_fwd_kernel<2>, grid, 256, lds_bytes, q, args);
  return chain_launch_kernel(mlp_chain_ln_fwd_kernel<1>, grid, 256, lds_bytes, q, args);
}

int rlg_mlp_chain_ln_backward(const rlg_chain_net* net, const rlg_chain_bwd* bwd, const rlg_chain_ln* ln,
                              const rlg_chain_launch* launch, void* stream) {
  using namespace rlg;
  if (net == nullptr || bwd == nullptr || ln == nullptr || launch == nullptr) return static_cast<int>(hipErrorInvalidValue);
  if (bwd->maxima_rows_out_or_null) *bwd->maxima_rows_out_or_null = 0;
  if (bwd->ppo_loss_or_null != nullptr || bwd->weight_form_or_null != nullptr || bwd->maxima_or_null != nullptr)
    return static_cast<int>(hipErrorNotSupported);
  const long long rows = launch->rows;
  if (rows <= 0) return 0;
  LnArgs args;
  if (const int e = ln_fill_net(args, *net, *ln)) return e;
  const int n = net->num_layers;
  if (n < 2 || bwd->d_out == nullptr || bwd->act_in == nullptr || bwd->act_ld == nullptr || bwd->dz_out == nullptr ||
      bwd->dz_ld == nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  for (int L = 0; L + 1 < n; ++L) {
    LnLayer& ly = args.layer[L];
    ly.h = const_cast<float*>(bwd->act_in[L]);
    ly.ldh = bwd->act_ld[L];
    ly.dz = bwd->dz_out[L];
    ly.lddz = bwd->dz_ld[L];
    ly.bias_partials = bwd->bias_partials_or_null ? bwd->bias_partials_or_null[L] : nullptr;
    if (ly.dz == nullptr) return static_cast<int>(hipErrorInvalidValue);
    const float* act_in = ly.h;
    long long act_ld = ly.ldh;
    if (ly.gamma != nullptr) {
      if (ln->pre_out == nullptr || ln->pre_ld == nullptr || ln->stats == nullptr || ln->pre_out[L] == nullptr || ln->stats[L] == nullptr)
        return static_cast<int>(hipErrorInvalidValue);
      ly.pre = ln->pre_out[L];
      ly.ldpre = ln->pre_ld[L];
      ly.stats = ln->stats[L];
      ly.gamma_partials = ln->gamma_partials_or_null ? ln->gamma_partials_or_null[L] : nullptr;
      ly.beta_partials = ln->beta_partials_or_null ? ln->beta_partials_or_null[L] : nullptr;
      act_in = ly.pre;
      act_ld = ly.ldpre;
    }
    if (act_in == nullptr) return static_cast<int>(hipErrorInvalidValue);
    // the stations read A and write dZ in 16-byte row accesses
    if (!(ln_vec4_host(act_in, act_ld) && ln_vec4_host(ly.dz, ly.lddz) && act_ld >= ly.out && ly.lddz >= ly.out))
      return static_cast<int>(hipErrorNotSupported);
  }
  args.x = bwd->d_out;
  args.ldx = bwd->ld_dout;
  args.rows = rows;
  int lds_bytes = 0;
  const int G = ln_resolve_groups(*net, *launch, 1, args, &lds_bytes);
  if (G < 0) return -G;
  if (const int e = ln_prepare()) return e;
  const int grid = static_cast<int>((rows + 16 * G - 1) / (16 * G));
  const ChainQueue q = chain_queue(*launch, stream);
  if (G == 4) return chain_launch_kernel(mlp_chain_ln_bwd_kernel<4>, grid, 256, lds_bytes, q, args);
  if (G == 2) return chain_launch_kernel(mlp_chain_ln_bwd_kernel<2>, grid, 256, lds_bytes, q, args);
  return chain_launch_kernel(mlp_chain_ln_bwd_kernel<1>, grid, 256, lds_bytes, q, args);
}

}  // extern "C"
