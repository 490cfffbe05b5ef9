// Separate actor / critic MLPs of a continuous policy (`network.separate: True`, no RNN; rl_games/algos_torch/
// network_builder.py:224-311: actor_mlp -> mu, critic_mlp -> value) as ONE vertically fused chain per direction on f32 MFMA
// (gfx950): one workgroup owns one row tile and runs BOTH trunks on it.
//
//   forward :  x -> [RunningMeanStd: fold the minibatch's moments (training), normalise] -> tile X in LDS, once
//              actor :  X -> (Linear -> act) x La -> mu      critic:  X -> (Linear -> act) x Lc -> value
//   backward:  d mu -> (dZ_l = (dZ_{l+1} W_{l+1}) * act'(H_l)) x La,  d value -> the same x Lc;  no dX of the observations
//
// Product form built: EXACT fp32 products on v_mfma_f32_16x16x4_f32, the only form of these kernels - no fp16 planes, no
// operand range limit, nothing for the range guard to watch (`chain_products: exact` is what they always run).  The scheme
// is csrc/mlp_chain_stream.hpp's: activations in LDS as [k-chunk][G][64 lanes][4] floats in whole zero-padded k-batches,
// weights streamed from L2 through bounds-checked buffer loads one k-batch ahead, a wave computes a 16-feature output block
// for all G row groups from one fetch of the weight fragment.  A row is a B-operand column: its result depends on nothing
// but the row.  No atomics.
//
// What is this file's own:
//   * Observations once.  The raw tile is read, normalised (and, with rms_batch, the statistics folded first, workgroup 0
//     publishing the new state - chain_norm_stats, the prologue of csrc/mlp_chain.hip) ONCE; tile X stays in LDS for the
//     whole launch and is the B operand of both trunks' first layers.  Two launches of a single-trunk chain read and
//     normalise every row twice.
//   * Trunks back to back.  LDS = [tile X | ping-pong region]: hidden tile t of a trunk sits at the bottom of the region
//     when t is even and ends at its top when t is odd, so the region is as large as the widest adjacent pair of EITHER
//     trunk; the critic reuses the actor's region behind one barrier.  The heads are stored straight from the accumulators
//     through their own pointer and row stride: the caller points them at one joint row [value | mu].
//   * Backward without stations.  The activation backward, the dZ store and the bias column sums are the product's
//     epilogue: H_l of the block is requested with the block's first k-batch, dZ_l goes to the other LDS region (the next
//     product's operand) and to global memory from the accumulators, the 16 rows of a group are summed by rotations on
//     the DPP path and the groups in index order in fp64 - one plain store per column and workgroup.  One barrier per
//     layer where csrc/mlp_chain_ln.hip needs three.
//
// Work split: 256 threads = 4 waves, one per SIMD, up to 512 VGPRs each; a tile of 16 G rows, G = 1 / 2 / 4.
//   * LDS per workgroup, [256, 128, 64] twice over 17 observations (the MuJoCo shape): forward (4 + 16 + 8) G KiB = 28 / 56 /
//     112 KiB, backward 2 x 16 G KiB = 32 / 64 / 128 KiB.  A tile of more rows re-reads the weights from L2 less often (the
//     ~360 KB of both trunks per 16 G rows); a workgroup's barriers and epilogues are covered only by ANOTHER workgroup on
//     the CU.  So G grows with the rows (2 from 8,192, 4 from 16,384: below that, 16-row tiles are what fills 256 CUs) but
//     only while two workgroups fit the 160 KiB of a CU (80 KiB each); a width that fits with one group only runs at G = 1.
//     512-wide layers: forward X + 32 KiB (one) or X + 64 KiB (two adjacent) at G = 1, backward 64 KiB.
//   * Registers: two weight batches in flight (32), G accumulators, G B operands, G H fragments (backward): far below the
//     budget at every G - see profiles/chain_twin.txt for the compiled figures (no scratch, no spills).
//   * A layer narrower than 64 features leaves waves without a block, for as long as that layer takes - a time that
//     shrinks with the layer.  Blocks are not split further: the idle waves of a narrow trunk do not shape the kernel.
// Envelope (rlg_mlp_chain_twin_supported): 1 - 4 hidden layers per trunk, one activation kind (elu / relu / tanh) for both,
// hidden widths multiples of 4 up to 512, any observation width, identity heads, one value column, no layer norm.

#include "mlp_chain_stream.hpp"

namespace rlg {

constexpr int kTwinMaxLayers = 5;          // per trunk: up to 4 hidden layers and the head
constexpr int kTwinMaxWidth = 512;
constexpr int kTwinLdsMax = 160 * 1024;

struct TwLayer {
  const float* w;            // [out, in] row-major
  const float* bias;         // forward
  float* h;                  // forward: the layer's output or nullptr (the head: required); backward: H_l, read
  float* dz;                 // backward: dZ_l, out
  double* bias_partials;     // backward: [gridDim.x, out] or nullptr
  long long ldh, lddz;
  int in, out;
};

struct TwTrunk {
  TwLayer layer[kTwinMaxLayers];
  const float* d_out;        // backward: d loss / d head [rows, ld_dout]
  long long ld_dout;
  int num_layers;
  int tile_off[kTwinMaxLayers];      // forward: float offset in LDS of hidden tile t, the output of layer t
};

struct TwArgs {
  TwTrunk trunk[2];          // actor, critic
  const float* x;            // raw observations [rows, ldx]
  long long ldx;
  const double* rms_mean;    // RunningMeanStd state or nullptr
  const double* rms_var;
  float rms_eps;
  const double* rms_batch;   // training: fold {sum[in], sumsq[in], rows} into the state first (chain_norm_stats)
  const long long* rms_count;
  double* rms_mean_out;
  double* rms_var_out;
  long long* rms_count_out;
  float* xn;                 // normalised observations out or nullptr
  long long rows;
  int act;                   // the hidden layers' activation
  int scratch_off;           // forward: mean32 / denominator of the normaliser, in the ping-pong region
  int r2_off;                // backward: the second operand region (the first starts at 0)
};

// blocks [NOB, NOB rounded up to a k-batch) of an operand tile: zero
template <int G>
__device__ __forceinline__ void tw_zero_pad(float* tile, int width, int wave, int lane) {
  const int NOB = (width + 15) >> 4;
  for (int ob = NOB + wave; ob < ((NOB + 3) & ~3); ob += 4) {
#pragma unroll
    for (int g = 0; g < G; ++g) *reinterpret_cast<f32x4*>(tile + ((ob * G + g) * 64 + lane) * 4) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
}

template <int G>
__global__ __launch_bounds__(256) void mlp_chain_twin_fwd_kernel(TwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int r16 = lane & 15, q4 = 4 * (lane >> 4);
  const long long row0 = static_cast<long long>(blockIdx.x) * (16 * G);
  const long long n_rows = pin_s(a.rows);
  const int act = pin_s(a.act);
  {
    const int in0 = a.trunk[0].layer[0].in, in0p = (in0 + 3) & ~3;
    float* sc = a.rms_mean != nullptr ? lds + a.scratch_off : nullptr;
    if (sc != nullptr) {
      chain_norm_stats<4>(a, sc, in0, in0p);
      __syncthreads();
    }
    sw_load_tile<G>(a.x, a.ldx, in0, row0, n_rows, lds, wave, lane, sc, in0p, a.xn);
    __syncthreads();                   // (the scratch lies where the first hidden tile goes: read for the last time above)
  }
  for (int tr = 0; tr < 2; ++tr) {
    const int n = pin_s(a.trunk[tr].num_layers);
    const float* tin = lds;            // tile X
    for (int L = 0; L < n; ++L) {
      const TwLayer& ly = a.trunk[tr].layer[L];
      const bool last = L == n - 1;
      const int K = pin_s(ly.in), I = pin_s(ly.out), lact = last ? static_cast<int>(kChIdentity) : act;
      const float* l_w = pin_s(ly.w);
      const float* l_bias = pin_s(ly.bias);
      float* g_dst = pin_s(ly.h);
      const long long g_ld = pin_s(ly.ldh);
      const bool g_vec = g_dst != nullptr && vec4_ok(g_dst, g_ld);
      float* tout = lds + pin_s(a.trunk[tr].tile_off[L]);
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
              f32x4 v = chain_act4<kChAny>(acc[g] + bv, lact);
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = f + e < I ? v[e] : 0.0f;
              if (!last) *reinterpret_cast<f32x4*>(tout + ((ob * G + g) * 64 + lane) * 4) = v;
              const long long row = row0 + 16 * g + r16;
              if (g_dst != nullptr && row < n_rows && f < I) store_row4(g_dst, g_ld, row, f, I, v, g_vec);
            }
          });
      if (!last) tw_zero_pad<G>(tout, I, wave, lane);
      // one barrier per layer: the tile just written is the next operand, the one just read is written again two layers
      // on - or, behind a trunk's head, by the other trunk's first layer
      __syncthreads();
      tin = tout;
    }
  }
}

template <int G>
__global__ __launch_bounds__(256) void mlp_chain_twin_bwd_kernel(TwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int r16 = lane & 15, q4 = 4 * (lane >> 4);
  const long long row0 = static_cast<long long>(blockIdx.x) * (16 * G);
  const long long n_rows = pin_s(a.rows);
  const int act = pin_s(a.act);
  for (int tr = 0; tr < 2; ++tr) {
    const TwTrunk& T = a.trunk[tr];
    const int n = pin_s(T.num_layers);
    float* cur = lds;                    // dZ_{l+1}, the product's operand
    float* nxt = lds + a.r2_off;         // dZ_l, written by the product's epilogue
    sw_load_tile<G>(T.d_out, T.ld_dout, T.layer[n - 1].out, row0, n_rows, cur, wave, lane, nullptr, 0, nullptr);
    __syncthreads();
    for (int L = n - 1; L >= 1; --L) {
      const int H = pin_s(T.layer[L].in), K = pin_s(T.layer[L].out);
      const float* l_w = pin_s(T.layer[L].w);
      const float* l_h = pin_s(T.layer[L - 1].h);
      const long long h_ld = pin_s(T.layer[L - 1].ldh);
      float* l_dz = pin_s(T.layer[L - 1].dz);
      const long long dz_ld = pin_s(T.layer[L - 1].lddz);
      double* bpart = pin_s(T.layer[L - 1].bias_partials);
      const long long prow = static_cast<long long>(blockIdx.x) * H;
      const rsrc_t wr = make_rsrc(l_w, static_cast<unsigned>(H) * static_cast<unsigned>(K) * 4u);
      f32x4 hv[G];
      sw_product<G, true>(
          wr, H, K, H, false, cur, wave, lane,
          [&](int ob) {                  // H_l of the block: on its way during the block's MFMAs
            const int f = ob * 16 + q4;
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const long long row = row0 + 16 * g + r16;
              hv[g] = (row < n_rows && f < H) ? load_row4(l_h, h_ld, row, f, H, true) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
          },
          [&](int ob, f32x4(&acc)[G]) {
            const int f = ob * 16 + q4;
            double sb[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const long long row = row0 + 16 * g + r16;
              const bool ok = row < n_rows && f < H;         // rows behind the minibatch, features behind H: zero
              f32x4 dz = chain_act_grad4(acc[g], hv[g], act);
#pragma unroll
              for (int e = 0; e < 4; ++e) dz[e] = ok ? dz[e] : 0.0f;
              *reinterpret_cast<f32x4*>(nxt + ((ob * G + g) * 64 + lane) * 4) = dz;
              if (ok) store_row4(l_dz, dz_ld, row, f, H, dz, true);
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
      tw_zero_pad<G>(nxt, H, wave, lane);
      __syncthreads();
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static long long tw_nb(int w) { return static_cast<long long>(((w + 15) / 16 + 3) & ~3); }      // blocks of a tile: whole k-batches

// 0, hipErrorInvalidValue for a malformed network, hipErrorNotSupported for one outside the envelope; *act: the hidden kind
static int tw_check(const rlg_chain_net* const nets[2], int* act) {
  int kind = 0;
  bool outside = false;
  for (int t = 0; t < 2; ++t) {
    const rlg_chain_net* net = nets[t];
    if (net == nullptr || net->num_layers < 1 || net->num_layers > kChainMaxLayers || net->in_features == nullptr ||
        net->out_features == nullptr || net->acts == nullptr)
      return static_cast<int>(hipErrorInvalidValue);
    const int n = net->num_layers;
    for (int L = 0; L < n; ++L) {
      if (net->in_features[L] <= 0 || net->out_features[L] <= 0 || (L > 0 && net->in_features[L] != net->out_features[L - 1]) ||
          net->acts[L] < kChIdentity || net->acts[L] > kChTanh)
        return static_cast<int>(hipErrorInvalidValue);
      if (L + 1 < n) {
        const int w = net->out_features[L], k = net->acts[L];
        if ((w & 3) != 0 || w > kTwinMaxWidth || k == kChIdentity || (kind != 0 && k != kind)) outside = true;
        kind = kind != 0 ? kind : k;
      } else if (net->acts[L] != kChIdentity || net->out_features[L] > kTwinMaxWidth) {
        outside = true;
      }
    }
    if (n < 2 || n > kTwinMaxLayers) outside = true;
  }
  if (nets[0]->in_features[0] != nets[1]->in_features[0]) return static_cast<int>(hipErrorInvalidValue);
  if (nets[1]->out_features[nets[1]->num_layers - 1] != 1) outside = true;                  // one value column
  if (static_cast<long long>(nets[0]->in_features[0]) * kTwinMaxWidth * 4 >= static_cast<long long>(kOob)) outside = true;
  if (outside) return static_cast<int>(hipErrorNotSupported);
  *act = kind;
  return 0;
}

// LDS bytes at G groups, -1: does not fit.  Forward (direction 0 / 2): tile X, then the ping-pong region - the widest
// adjacent pair of hidden tiles of either trunk, or the normaliser's scratch if that is larger.  Backward: two regions,
// each as large as the widest tile (d heads included) of either trunk.
static int tw_lds_plan(const rlg_chain_net* const nets[2], int G, int direction, TwArgs* args) {
  const long long blk = 256LL * G;
  long long floats;
  if (direction == 1) {
    long long r = 0;
    for (int t = 0; t < 2; ++t) {
      for (int L = 0; L < nets[t]->num_layers; ++L) r = tw_nb(nets[t]->out_features[L]) > r ? tw_nb(nets[t]->out_features[L]) : r;
    }
    floats = 2 * r * blk;
    if (args) args->r2_off = static_cast<int>(r * blk);
  } else {
    const int in0 = nets[0]->in_features[0];
    const long long nbx = tw_nb(in0), scratch = 2LL * ((in0 + 3) & ~3);
    long long pair = 0;
    for (int t = 0; t < 2; ++t) {
      for (int L = 0; L + 1 < nets[t]->num_layers; ++L) {
        long long s = tw_nb(nets[t]->out_features[L]);
        if (L + 2 < nets[t]->num_layers) s += tw_nb(nets[t]->out_features[L + 1]);
        pair = s > pair ? s : pair;
      }
    }
    floats = nbx * blk + (pair * blk > scratch ? pair * blk : scratch);
    if (args && floats * 4 <= kTwinLdsMax) {
      for (int t = 0; t < 2; ++t) {
        for (int L = 0; L + 1 < nets[t]->num_layers; ++L)
          args->trunk[t].tile_off[L] = static_cast<int>((nbx + ((L & 1) ? pair - tw_nb(nets[t]->out_features[L]) : 0)) * blk);
      }
      args->scratch_off = static_cast<int>(nbx * blk);
    }
  }
  return floats * 4 <= kTwinLdsMax ? static_cast<int>(floats * 4) : -1;
}

// The 16-row groups of a launch (file header, "Work split"): 2 from 8,192 rows, 4 from 16,384, while two workgroups fit a
// CU's LDS; G = 1 whenever it fits at all.  0: no G fits.
static int tw_pick_groups(const rlg_chain_net* const nets[2], long long rows, int direction) {
  for (int G = rows >= 16384 ? 4 : (rows >= 8192 ? 2 : 1); G >= 1; G >>= 1) {
    const int bytes = tw_lds_plan(nets, G, direction, nullptr);
    if (bytes >= 0 && (G == 1 || bytes <= kTwinLdsMax / 2)) return G;
  }
  return 0;
}

// raises the kernels' dynamic-LDS limit, once per process; 0 or the hipError_t of the attribute call (kept)
static int tw_prepare() {
  static const int status = [] {
    const void* kernels[] = {reinterpret_cast<const void*>(mlp_chain_twin_fwd_kernel<1>), reinterpret_cast<const void*>(mlp_chain_twin_fwd_kernel<2>),
                             reinterpret_cast<const void*>(mlp_chain_twin_fwd_kernel<4>), reinterpret_cast<const void*>(mlp_chain_twin_bwd_kernel<1>),
                             reinterpret_cast<const void*>(mlp_chain_twin_bwd_kernel<2>), reinterpret_cast<const void*>(mlp_chain_twin_bwd_kernel<4>)};
    for (const void* k : kernels) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kTwinLdsMax);
      if (e != hipSuccess) {
        (void)hipGetLastError();                       // (the launch entries return it; it must not surface in another launch)
        return static_cast<int>(e);
      }
    }
    return 0;
  }();
  return status;
}

static bool tw_has_norm(const rlg_chain_net* net, const rlg_chain_ln* ln) {
  if (ln == nullptr || ln->gamma == nullptr) return false;
  for (int L = 0; L < net->num_layers; ++L) {
    if (ln->gamma[L] != nullptr) return true;
  }
  return false;
}

static bool tw_vec4_host(const void* p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (ld & 3) == 0; }

// shape, weights and the hidden activation of both trunks into args; non-zero: a hipError_t
static int tw_fill_nets(TwArgs& args, const rlg_chain_net* const nets[2]) {
  args = TwArgs{};
  if (const int e = tw_check(nets, &args.act)) return e;
  for (int t = 0; t < 2; ++t) {
    if (nets[t]->weights == nullptr) return static_cast<int>(hipErrorInvalidValue);
    args.trunk[t].num_layers = nets[t]->num_layers;
    for (int L = 0; L < nets[t]->num_layers; ++L) {
      TwLayer& ly = args.trunk[t].layer[L];
      ly.w = nets[t]->weights[L];
      ly.in = nets[t]->in_features[L];
      ly.out = nets[t]->out_features[L];
      if (ly.w == nullptr || reinterpret_cast<uintptr_t>(ly.w) % 4 != 0) return static_cast<int>(hipErrorInvalidValue);
    }
  }
  return 0;
}

// the groups of a launch and its LDS plan; < 0: minus a hipError_t
static int tw_resolve_groups(const rlg_chain_net* const nets[2], const rlg_chain_launch& launch, int direction, TwArgs& args,
                             int* lds_bytes) {
  int G = launch.groups;
  if (G == 0) {
    G = tw_pick_groups(nets, launch.rows, direction);
    if (G == 0) return -static_cast<int>(hipErrorNotSupported);
  } else if (G != 1 && G != 2 && G != 4) {
    return -static_cast<int>(hipErrorInvalidValue);
  }
  *lds_bytes = tw_lds_plan(nets, G, direction, &args);
  if (*lds_bytes < 0) return -static_cast<int>(launch.groups == 0 ? hipErrorNotSupported : hipErrorInvalidValue);
  return G;
}

}  // namespace rlg

// ---------------------------------------------------------------------------------
// C ABI (declared in include/rlg_hip.h)
// ---------------------------------------------------------------------------------
extern "C" {

int rlg_mlp_chain_twin_supported(const rlg_chain_net* actor, const rlg_chain_net* critic, const rlg_chain_ln* actor_ln_or_null,
                                 const rlg_chain_ln* critic_ln_or_null, long long rows, int direction) {
  using namespace rlg;
  const rlg_chain_net* const nets[2] = {actor, critic};
  int act = 0;
  if (direction < 0 || direction > 2 || tw_check(nets, &act) != 0) return 0;
  if (tw_has_norm(actor, actor_ln_or_null) || tw_has_norm(critic, critic_ln_or_null)) return 0;
  // the answer is host arithmetic; a failure of the attribute call is not "outside the envelope": the launch entries report it
  const int G = tw_pick_groups(nets, rows, direction);
  if (G > 0) (void)tw_prepare();
  return G;
}

int rlg_mlp_chain_twin_forward(const rlg_chain_net* actor, const rlg_chain_net* critic, const rlg_chain_fwd* actor_fwd,
                               const rlg_chain_fwd* critic_fwd, const rlg_chain_launch* launch, void* stream) {
  using namespace rlg;
  if (actor == nullptr || critic == nullptr || actor_fwd == nullptr || critic_fwd == nullptr || launch == nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  const rlg_chain_net* const nets[2] = {actor, critic};
  const rlg_chain_fwd* const fwds[2] = {actor_fwd, critic_fwd};
  for (const rlg_chain_fwd* f : fwds) {
    if (f->weight_form_or_null != nullptr || f->pack_backward_planes_or_null != nullptr) return static_cast<int>(hipErrorNotSupported);
  }
  const long long rows = launch->rows;
  if (rows <= 0) return 0;
  TwArgs args;
  if (const int e = tw_fill_nets(args, nets)) return e;
  // the observations and the normaliser are the actor half's; the critic half may repeat the observations, nothing else
  if (actor_fwd->x == nullptr || (critic_fwd->x != nullptr && (critic_fwd->x != actor_fwd->x || critic_fwd->ldx != actor_fwd->ldx)) ||
      critic_fwd->rms_batch_or_null != nullptr || critic_fwd->xn_out_or_null != nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  bool training = false;
  for (int t = 0; t < 2; ++t) {
    const int n = nets[t]->num_layers;
    if (fwds[t]->act_out == nullptr || fwds[t]->act_ld == nullptr || fwds[t]->act_out[n - 1] == nullptr)
      return static_cast<int>(hipErrorInvalidValue);
    for (int L = 0; L < n; ++L) {
      TwLayer& ly = args.trunk[t].layer[L];
      ly.bias = nets[t]->biases ? nets[t]->biases[L] : nullptr;
      ly.h = fwds[t]->act_out[L];
      ly.ldh = fwds[t]->act_ld[L];
      if (reinterpret_cast<uintptr_t>(ly.bias) % 4 != 0 || reinterpret_cast<uintptr_t>(ly.h) % 4 != 0 ||
          (ly.h != nullptr && ly.ldh < ly.out))
        return static_cast<int>(hipErrorInvalidValue);
      training = training || (L + 1 < n && ly.h != nullptr);
    }
  }
  args.x = actor_fwd->x;
  args.ldx = actor_fwd->ldx;
  if (args.ldx < args.trunk[0].layer[0].in) return static_cast<int>(hipErrorInvalidValue);
  args.rms_mean = actor_fwd->rms_mean_or_null;
  args.rms_var = args.rms_mean ? actor_fwd->rms_var : nullptr;
  if (args.rms_mean != nullptr && args.rms_var == nullptr) return static_cast<int>(hipErrorInvalidValue);
  args.rms_eps = actor_fwd->rms_eps;
  args.rms_batch = args.rms_mean ? actor_fwd->rms_batch_or_null : nullptr;
  if (args.rms_batch != nullptr) {
    const rlg_chain_fwd& f = *actor_fwd;
    if (!f.rms_count || !f.rms_mean_out || !f.rms_var_out || !f.rms_count_out || f.rms_mean_out == args.rms_mean ||
        f.rms_var_out == f.rms_var || f.rms_count_out == f.rms_count)
      return static_cast<int>(hipErrorInvalidValue);      // the fold publishes into a second buffer set
    args.rms_count = f.rms_count;
    args.rms_mean_out = f.rms_mean_out;
    args.rms_var_out = f.rms_var_out;
    args.rms_count_out = f.rms_count_out;
  }
  args.xn = actor_fwd->xn_out_or_null;
  args.rows = rows;
  int lds_bytes = 0;
  const int G = tw_resolve_groups(nets, *launch, training ? 2 : 0, args, &lds_bytes);
  if (G < 0) return -G;
  if (const int e = tw_prepare()) return e;
  const int grid = static_cast<int>((rows + 16 * G - 1) / (16 * G));
  const ChainQueue q = chain_queue(*launch, stream);
  if (G == 4) return chain_launch_kernel(mlp_chain_twin_fwd_kernel<4>, grid, 256, lds_bytes, q, args);
  if (G == 2) return chain_launch_kernel(mlp_chain_twin_fwd_kernel<2>, grid, 256, lds_bytes, q, args);
  return chain_launch_kernel(mlp_chain_twin_fwd_kernel<1>, grid, 256, lds_bytes, q, args);
}

int rlg_mlp_chain_twin_backward(const rlg_chain_net* actor, const rlg_chain_net* critic, const rlg_chain_bwd* actor_bwd,
                                const rlg_chain_bwd* critic_bwd, const rlg_chain_launch* launch, void* stream) {
  using namespace rlg;
  if (actor == nullptr || critic == nullptr || actor_bwd == nullptr || critic_bwd == nullptr || launch == nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  const rlg_chain_net* const nets[2] = {actor, critic};
  const rlg_chain_bwd* const bwds[2] = {actor_bwd, critic_bwd};
  for (const rlg_chain_bwd* b : bwds) {
    if (b->maxima_rows_out_or_null) *b->maxima_rows_out_or_null = 0;
  }
  for (const rlg_chain_bwd* b : bwds) {
    if (b->ppo_loss_or_null != nullptr || b->weight_form_or_null != nullptr || b->maxima_or_null != nullptr)
      return static_cast<int>(hipErrorNotSupported);
  }
  const long long rows = launch->rows;
  if (rows <= 0) return 0;
  TwArgs args;
  if (const int e = tw_fill_nets(args, nets)) return e;
  for (int t = 0; t < 2; ++t) {
    const rlg_chain_bwd& b = *bwds[t];
    const int n = nets[t]->num_layers;
    if (b.d_out == nullptr || b.act_in == nullptr || b.act_ld == nullptr || b.dz_out == nullptr || b.dz_ld == nullptr ||
        reinterpret_cast<uintptr_t>(b.d_out) % 4 != 0 || b.ld_dout < nets[t]->out_features[n - 1])
      return static_cast<int>(hipErrorInvalidValue);
    args.trunk[t].d_out = b.d_out;
    args.trunk[t].ld_dout = b.ld_dout;
    for (int L = 0; L + 1 < n; ++L) {
      TwLayer& ly = args.trunk[t].layer[L];
      ly.h = const_cast<float*>(b.act_in[L]);
      ly.ldh = b.act_ld[L];
      ly.dz = b.dz_out[L];
      ly.lddz = b.dz_ld[L];
      ly.bias_partials = b.bias_partials_or_null ? b.bias_partials_or_null[L] : nullptr;
      if (ly.h == nullptr || ly.dz == nullptr || reinterpret_cast<uintptr_t>(ly.bias_partials) % 8 != 0)
        return static_cast<int>(hipErrorInvalidValue);
      // the epilogues read H and write dZ in 16-byte row accesses
      if (!(tw_vec4_host(ly.h, ly.ldh) && tw_vec4_host(ly.dz, ly.lddz) && ly.ldh >= ly.out && ly.lddz >= ly.out))
        return static_cast<int>(hipErrorNotSupported);
    }
  }
  args.rows = rows;
  int lds_bytes = 0;
  const int G = tw_resolve_groups(nets, *launch, 1, args, &lds_bytes);
  if (G < 0) return -G;
  if (const int e = tw_prepare()) return e;
  const int grid = static_cast<int>((rows + 16 * G - 1) / (16 * G));
  const ChainQueue q = chain_queue(*launch, stream);
  if (G == 4) return chain_launch_kernel(mlp_chain_twin_bwd_kernel<4>, grid, 256, lds_bytes, q, args);
  if (G == 2) return chain_launch_kernel(mlp_chain_twin_bwd_kernel<2>, grid, 256, lds_bytes, q, args);
  return chain_launch_kernel(mlp_chain_twin_bwd_kernel<1>, grid, 256, lds_bytes, q, args);
}

}  // extern "C"
