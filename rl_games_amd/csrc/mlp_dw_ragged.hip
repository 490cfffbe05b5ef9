// Weight gradient of a layer whose widths are NOT multiples of 4, on the matrix cores (gfx950):
//
//   G [No, Mi] = dZ [rows, No]^T  X [rows, Mi]        No 1 .. 1024, Mi 1 .. 512, rows >= 1, fp32, dense row-major operands
//
// autograd's `grad_weight = grad_output.t().mm(input)` of a first nn.Linear over 9, 11, 17, 27, 98, 105 ... observations
// (rl_games/algos_torch/network_builder.py:118-147), which csrc/mlp_dw.hip declines: its lanes load 4 / 8 / 16-byte vectors
// of row-major X straight into MFMA source registers, and a row of 98 floats neither starts at a 16-byte boundary nor ends a
// tile inside the row.  Same matrix instruction and operand mapping here (v_mfma_f32_16x16x4_f32, i = output feature, j =
// input feature, k = minibatch row: exact fp32 products, fp32 sums), with a data path through LDS in between:
//   * split-K over workgroups by SLICES of kRgRows = 16 rows.  The rows of a dense matrix start every slice at a 16-byte
//     boundary whatever the width, so the slice is one contiguous run of floats that 128-bit buffer loads walk from its first
//     byte.  The descriptor is made per slice: its record count ends the run with the slice - in the last one, with `rows`.
//     A workgroup (4 waves) walks `spw` consecutive slices, so the partial tiles number rows / (16 spw) however long the
//     minibatch is; the grid's second dimension tiles outputs wider than 128 x 128.
//   * a tile's operands are the columns [c0, c0 + cw) of each matrix.  A thread owns (row, quad) pairs of the slice that do
//     not change from slice to slice: quad j of row r is the aligned 16 bytes at float (r W + c0 & ~3) + 4 j, and (cw + 3) / 4
//     + 1 quads cover the row's columns wherever they start.  Each of the 4 floats goes to LDS at [r][column - c0] when its
//     column is in the tile - a SELECTION: floats of the neighbouring row, rows behind `rows` (never requested: the caller's
//     buffer may go on there, with anything in it) and the columns behind cw (zeroed once, never written) cannot reach a sum.
//     The one quad that straddles the end of the matrix is fetched float by float.
//   * LDS: two buffers of [16][PA] dZ and [16][PB] X floats; the quads of slice s + 1 are requested before the MFMAs of slice
//     s issue and stored behind them, one barrier per slice.  Pitch = the tile's width in whole 16-column blocks, raised to
//     16 mod 64: the four rows that an operand read touches (lane l reads [r + (l >> 4)][c + (l & 15)]) fall into four
//     different quarters of the 64 banks - no conflicts.
//   * the 4 waves share the tile's 16 x 16 blocks as WO x WI (4 x 1 from 4 block rows, 2 x 2 from 2, else 1 x 4); wave
//     (wo, wi) owns blocks (a WO + wo, b WI + wi), a < BO <= 2, b < BI <= 8: at most 64 accumulator registers, held for the
//     whole slice loop.  Blocks behind the tile multiply the zero columns (branch-free k-steps).
//   * every workgroup stores its fp32 tile once; a second kernel sums the partials of an element in index order in fp64.
//     No atomics: the same inputs give the same bits.

#include "mlp_chain_common.hpp"

RLG_ABI_SIZE(rlg_dw_ragged, 56);

namespace rlg {

constexpr int kRgRows = 16;          // rows of a slice (a multiple of 4: every slice starts at a 16-byte boundary)
constexpr int kRgQuads = 3;          // (row, quad) pairs of a thread per matrix: 16 rows x 33 quads / 256 threads
constexpr int kRgMaxPitch = 144;     // 128 columns raised to 16 mod 64
constexpr int kRgTileBlocks = 8;     // a tile: at most 8 x 8 blocks of 16 x 16
constexpr int kRgMinSlices = 4;      // slices a workgroup walks: at least 64 rows per partial tile,
constexpr int kRgMaxSlices = 16;     //   256 rows from where every CU has a workgroup (profiles/dw_ragged.txt)
constexpr int kRgCus = 256;
constexpr int kRgTargetBlocks = 512; // workgroups of a launch at most, two per CU

struct RgPlan {
  int tiles_o, tiles_i;     // output tiles per dimension
  int tbo, tbi;             // 16-column blocks of a tile per dimension (the last tile may hold fewer)
  int WO, WI, BO, BI;       // waves and blocks per wave, per dimension
  int PA, PB;               // LDS row pitches in floats
  int nslices, spw, groups; // slices, slices per workgroup, workgroups per tile = partial tiles per element
};

struct RgArgs {
  const float* dz;
  const float* x;
  float* ws;
  long long rows;
  int No, Mi;
  RgPlan p;
};

static int rg_pitch(int cols) { return ((cols + 47) / 64) * 64 + 16; }

static bool rg_plan(long long rows, int No, int Mi, RgPlan& p) {
  if (rows < 1 || rows > (1LL << 30) || No < 1 || No > 1024 || Mi < 1 || Mi > 512) return false;
  const int nbo = (No + 15) / 16, nbi = (Mi + 15) / 16;
  p.tiles_o = (nbo + kRgTileBlocks - 1) / kRgTileBlocks;
  p.tiles_i = (nbi + kRgTileBlocks - 1) / kRgTileBlocks;
  p.tbo = (nbo + p.tiles_o - 1) / p.tiles_o;
  p.tbi = (nbi + p.tiles_i - 1) / p.tiles_i;
  p.WO = p.tbo >= 4 ? 4 : (p.tbo >= 2 ? 2 : 1);
  p.WI = 4 / p.WO;
  p.BO = (p.tbo + p.WO - 1) / p.WO;
  const int bi = (p.tbi + p.WI - 1) / p.WI;
  p.BI = bi > 4 ? 8 : (bi > 2 ? 4 : bi);
  p.PA = rg_pitch(p.WO * p.BO * 16);
  p.PB = rg_pitch(p.WI * p.BI * 16);
  p.nslices = static_cast<int>((rows + kRgRows - 1) / kRgRows);
  const int tiles = p.tiles_o * p.tiles_i;
  // slices per workgroup: what gives every CU a workgroup, within [kRgMinSlices, kRgMaxSlices] - a short minibatch is a
  // latency chain per workgroup (one slice of look-ahead), a long one pays for every partial tile it writes and re-reads
  // - and never more than kRgTargetBlocks workgroups
  const long long par = static_cast<long long>(p.nslices) * tiles / kRgCus;
  p.spw = par < kRgMinSlices ? kRgMinSlices : (par > kRgMaxSlices ? kRgMaxSlices : static_cast<int>(par));
  const int cap = kRgTargetBlocks / tiles > 0 ? kRgTargetBlocks / tiles : 1;
  if (p.spw < (p.nslices + cap - 1) / cap) p.spw = (p.nslices + cap - 1) / cap;
  p.groups = (p.nslices + p.spw - 1) / p.spw;
  return p.BO <= 2 && p.BI <= 8 && p.PA <= kRgMaxPitch && p.PB <= kRgMaxPitch;
}

// A thread's (row, quad) pairs of one operand: the same in every slice
struct RgStage {
  int foff[kRgQuads];       // float offset of the quad from the slice's first float, or -1: no pair
  int col0[kRgQuads];       // tile column of the quad's first float: -3 .. cw + 3
  int dst[kRgQuads];        // LDS float index of that column in the operand's [16][pitch] array
};

__device__ __forceinline__ void rg_stage_init(RgStage& s, int W, int c0, int cw, int pitch) {
  const int Q = ((cw + 3) >> 2) + 1;
#pragma unroll
  for (int u = 0; u < kRgQuads; ++u) {
    const int p = threadIdx.x + 256 * u;
    const int row = p / Q, j = p - row * Q;
    const int start = row * W + c0;
    const int f0 = (start & ~3) + 4 * j;
    s.foff[u] = row < kRgRows ? f0 : -1;
    s.col0[u] = f0 - start;
    s.dst[u] = row * pitch + (f0 - start);
  }
}

// the quads of a slice of n floats behind r (record count: 4 n bytes); nothing behind the n-th float is requested
__device__ __forceinline__ void rg_fetch(const RgStage& s, rsrc_t r, int n, f32x4 (&v)[kRgQuads]) {
#pragma unroll
  for (int u = 0; u < kRgQuads; ++u) {
    int f = s.foff[u];
    asm volatile("" : "+v"(f));      // compared anew in every slice: hoisted out of the slice loop, the lane masks of all
                                     // these selections would spill scalar registers
    if (f >= 0 && f + 4 <= n) {
      v[u] = buf_load4(r, static_cast<unsigned>(f) * 4u);
    } else if (f >= 0 && f < n) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[u][e] = f + e < n ? buf_load1(r, static_cast<unsigned>(f + e) * 4u) : 0.0f;
    } else {
      v[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
  }
}

__device__ __forceinline__ void rg_put(const RgStage& s, const f32x4 (&v)[kRgQuads], float* dst, int cw) {
#pragma unroll
  for (int u = 0; u < kRgQuads; ++u) {
    int c0 = s.col0[u];
    asm volatile("" : "+v"(c0));     // (as in rg_fetch)
    if (s.foff[u] >= 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + e;
        if (c >= 0 && c < cw) dst[s.dst[u] + e] = v[u][e];
      }
    }
  }
}

template <int BO, int BI>
__global__ __launch_bounds__(256) void mlp_dw_ragged_kernel(RgArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kRgRows * 2 * kRgMaxPitch];      // 36,864 bytes
  const RgPlan& p = a.p;
  const int lane = lane_id(), wave = wave_id_uniform();
  const int to = static_cast<int>(blockIdx.y) / p.tiles_i, ti = static_cast<int>(blockIdx.y) - to * p.tiles_i;
  const int o0 = to * p.tbo * 16, i0 = ti * p.tbi * 16;
  const int cwa = min(p.tbo * 16, a.No - o0), cwb = min(p.tbi * 16, a.Mi - i0);
  const int buf_floats = kRgRows * (p.PA + p.PB), b_off = kRgRows * p.PA;

  RgStage sa, sb;
  rg_stage_init(sa, a.No, o0, cwa, p.PA);
  rg_stage_init(sb, a.Mi, i0, cwb, p.PB);

  const int s_begin = static_cast<int>(blockIdx.x) * p.spw;
  const int s_end = min(s_begin + p.spw, p.nslices);
  f32x4 va[kRgQuads], vb[kRgQuads];
  auto fetch = [&](int s) {
    const long long row0 = static_cast<long long>(s) * kRgRows;
    const long long left = a.rows - row0;
    const int nr = left < kRgRows ? static_cast<int>(left) : kRgRows;
    rg_fetch(sa, make_rsrc(a.dz + row0 * a.No, static_cast<unsigned>(nr * a.No) * 4u), nr * a.No, va);
    rg_fetch(sb, make_rsrc(a.x + row0 * a.Mi, static_cast<unsigned>(nr * a.Mi) * 4u), nr * a.Mi, vb);
  };
  auto put = [&](int b) {
    rg_put(sa, va, lds + b * buf_floats, cwa);
    rg_put(sb, vb, lds + b * buf_floats + b_off, cwb);
  };

  fetch(s_begin);
  // the columns behind the tile, in both buffers: zero from here on (no slice writes them)
  for (int t = threadIdx.x; t < 2 * buf_floats; t += 256) lds[t] = 0.0f;
  __syncthreads();
  put(0);
  __syncthreads();

  f32x4 acc[BO][BI];
#pragma unroll
  for (int f = 0; f < BO; ++f) {
#pragma unroll
    for (int g = 0; g < BI; ++g) acc[f][g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int wo = wave % p.WO, wi = wave / p.WO;
  const int a_lane = (lane >> 4) * p.PA + wo * 16 + (lane & 15);
  const int b_lane = (lane >> 4) * p.PB + wi * 16 + (lane & 15);
  const int a_blk = p.WO * 16, b_blk = p.WI * 16;

#pragma unroll 1
  for (int s = s_begin; s < s_end; ++s) {
    const int cur = (s - s_begin) & 1;
    const bool more = s + 1 < s_end;
    if (more) fetch(s + 1);
    RLG_PIN();
    const float* pa = lds + cur * buf_floats + a_lane;
    const float* pb = lds + cur * buf_floats + b_off + b_lane;
#pragma unroll
    for (int ks = 0; ks < kRgRows / 4; ++ks) {
      float av[BO], bv[BI];
#pragma unroll
      for (int f = 0; f < BO; ++f) av[f] = pa[ks * 4 * p.PA + f * a_blk];
#pragma unroll
      for (int g = 0; g < BI; ++g) bv[g] = pb[ks * 4 * p.PB + g * b_blk];
#pragma unroll
      for (int f = 0; f < BO; ++f) {
#pragma unroll
        for (int g = 0; g < BI; ++g) acc[f][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[f], bv[g], acc[f][g], 0, 0, 0);
      }
    }
    RLG_PIN();
    if (more) put(cur ^ 1);
    __syncthreads();
  }
  // 10 wait states between v_mfma_f32_16x16x4_f32 and the first VALU / store read of its result: not interlocked on gfx950,
  // and hipcc counts short across branches (csrc/mlp_chain.hip, tools/audit_mfma.py)
  RLG_PIN();
  asm volatile("s_nop 7\n\ts_nop 1");
  RLG_PIN();

  // acc[f][g][e] = G[o0 + 16 (f WO + wo) + 4 (lane >> 4) + e][i0 + 16 (g WI + wi) + (lane & 15)]
  float* out = a.ws + static_cast<long long>(blockIdx.x) * a.No * a.Mi;
#pragma unroll
  for (int f = 0; f < BO; ++f) {
#pragma unroll
    for (int g = 0; g < BI; ++g) {
      const int ic = 16 * (g * p.WI + wi) + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int oc = 16 * (f * p.WO + wo) + 4 * (lane >> 4) + e;
        if (oc < cwa && ic < cwb) out[static_cast<long long>(o0 + oc) * a.Mi + i0 + ic] = acc[f][g][e];
      }
    }
  }
}

// G[e] = the partials of element e, in workgroup order, in fp64
__global__ __launch_bounds__(256) void mlp_dw_ragged_finalize_kernel(const float* __restrict__ ws, int groups, int n,
                                                                     float* __restrict__ grad) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double t = 0.0;
  for (int g = 0; g < groups; ++g) t += static_cast<double>(ws[static_cast<long long>(g) * n + e]);
  grad[e] = static_cast<float>(t);
}

template <int BO>
static bool rg_launch(const RgArgs& a, dim3 grid, hipStream_t st) {
  switch (a.p.BI) {
    case 1: hipLaunchKernelGGL((mlp_dw_ragged_kernel<BO, 1>), grid, dim3(256), 0, st, a); return true;
    case 2: hipLaunchKernelGGL((mlp_dw_ragged_kernel<BO, 2>), grid, dim3(256), 0, st, a); return true;
    case 4: hipLaunchKernelGGL((mlp_dw_ragged_kernel<BO, 4>), grid, dim3(256), 0, st, a); return true;
    case 8: hipLaunchKernelGGL((mlp_dw_ragged_kernel<BO, 8>), grid, dim3(256), 0, st, a); return true;
  }
  return false;
}

}  // namespace rlg

extern "C" {

long long rlg_mlp_dw_ragged_workspace(long long rows, int out_features, int in_features) {
  rlg::RgPlan p;
  if (!rlg::rg_plan(rows, out_features, in_features, p)) return 0;
  return static_cast<long long>(p.groups) * out_features * in_features;
}

int rlg_mlp_dw_ragged(const rlg_dw_ragged* d, void* stream) {
  if (d == nullptr || d->dz == nullptr || d->x == nullptr || d->grad == nullptr || d->workspace == nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  rlg::RgArgs a;
  if (!rlg::rg_plan(d->rows, d->out_features, d->in_features, a.p)) return static_cast<int>(hipErrorNotSupported);
  if (((reinterpret_cast<uintptr_t>(d->dz) | reinterpret_cast<uintptr_t>(d->x) | reinterpret_cast<uintptr_t>(d->grad)
        | reinterpret_cast<uintptr_t>(d->workspace)) & 15u) != 0)
    return static_cast<int>(hipErrorNotSupported);
  const int n = d->out_features * d->in_features;
  if (d->workspace_floats < static_cast<long long>(a.p.groups) * n) return static_cast<int>(hipErrorInvalidValue);
  a.dz = d->dz;
  a.x = d->x;
  a.ws = d->workspace;
  a.rows = d->rows;
  a.No = d->out_features;
  a.Mi = d->in_features;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(a.p.groups, a.p.tiles_o * a.p.tiles_i);
  if (!(a.p.BO == 1 ? rlg::rg_launch<1>(a, grid, st) : rlg::rg_launch<2>(a, grid, st)))
    return static_cast<int>(hipErrorNotSupported);
  hipLaunchKernelGGL(rlg::mlp_dw_ragged_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a.ws, a.p.groups, n,
                     d->grad);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
