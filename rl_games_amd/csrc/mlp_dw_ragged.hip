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
// Minibatches below some 20,000 rows have a kernel of their own further down (mlp_dw_ragged_short_kernel): one launch.

#include "mlp_chain_common.hpp"

#include <algorithm>

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

// ---- short minibatches (1 .. 20,479 rows): one launch ----------------------------------------------------------------
// The kernel above gives a workgroup one 16-row slice of look-ahead and sums the partial tiles in a second launch: below
// some 20,000 rows that is a chain of exposed load latencies in front of a launch gap (profiles/dw_ragged.txt).  Same
// product, same selection of floats into LDS, same wave-to-block mapping and pitches here, but:
//   * a workgroup owns a RUN of consecutive rows of one output tile, in bursts of `rb` rows (a multiple of 4: every burst
//     starts at a 16-byte boundary).  EVERY 128-bit buffer load of a burst, for both operands, is issued before the first
//     is waited for (up to kRsQuads quads per thread and operand, their (row, quad) pairs computed on the fly: no staging
//     registers survive a burst); the floats are then selected into ONE LDS buffer of [rb][PA] + [rb][PB] floats, and the
//     burst is walked in k-steps of 4 rows.  A run of up to rb rows is one burst: one exposed latency per workgroup.  A
//     longer run (rs_plan says when) issues all loads of burst b + 1 before the MFMAs of burst b and selects them behind.
//   * tiles for first layers: all of Mi up to 128 columns, and 32, 64 or 128 output features, chosen by rs_plan.
//   * the sum in the same launch: a workgroup stores its fp32 partial tile, fences once (thread 0, behind a barrier), and
//     draws a ticket from its tile's counter word with one agent-scope atomic add.  Whoever draws the tile's last ticket fences again, sums the tile's
//     partials in index order in fp64 (mlp_dw_ragged_finalize_kernel's order and type), writes grad and stores 0 into the
//     counter: the next call, or a graph replay, finds it zero.  The order of arrival decides WHO sums, never in what
//     order: the same inputs give the same bits.  Nobody waits for anybody: no spin, no grid barrier.  A tile with one
//     workgroup writes grad directly and touches no counter.
// Static LDS of 64 KB at most: no function attribute, nothing to prepare outside a stream capture.

constexpr int kRsQuads = 8;              // (row, quad) pairs of a thread per operand and burst: 64 load registers in flight
constexpr int kRsLdsFloats = 16380;      // the burst's LDS; with the ticket word 65,524 bytes
constexpr int kRsMaxBursts = 8;          // bursts of a run at most
constexpr int kRsSumElems = 4;           // the sum of a tile's partials: elements of a thread and partials of each
constexpr int kRsSumGroups = 16;         //   that are loaded before the first is added
constexpr int kRsCounters = 128;         // counter words in front of the partial tiles: 32 x 4 tiles at most (fixed, so
                                         // that callers may share one zero-filled workspace between shapes)

struct RsPlan {
  int tiles_o, tiles_i, tbo, tbi, WO, WI, BO, BI, PA, PB;      // as RgPlan
  int rb, bursts, run;      // rows of a burst, bursts of a run, rows of a run = rb * bursts
  int groups;               // workgroups per tile = partial tiles per element
};

struct RsArgs {
  const float* dz;
  const float* x;
  float* grad;
  float* parts;             // [groups][No, Mi] partial tiles (groups > 1)
  unsigned* tickets;        // [tiles] counter words, zero between calls
  long long rows;
  int No, Mi;
  RsPlan p;
};

// The plan's rule.  Input tiles as above (all of Mi up to 128 columns).  Output tiles of 32, then 64, then 128 features:
// the narrowest first, because a tile's partials are summed by ONE workgroup (groups x tile elements, serial behind the
// last arrival), so more tiles of fewer partials each make the shortest tail; a wider tile is taken only when the
// narrower one's runs would be longer than kRsMaxBursts bursts.  Rows of a run, a multiple of 4:
//   * what leaves every CU a workgroup: rows * tiles / 256, rounded down;
//   * but at least No Mi / (No + Mi), so that the partial tiles written and read again (groups No Mi floats each way)
//     are no more than the operands (rows (No + Mi) floats) - short minibatches then run on fewer than 256 workgroups;
//   * at most kRsMaxBursts bursts of the rows that fit the LDS buffer and kRsQuads quads per thread, and `rows`.
// The run is then split evenly into the fewest bursts.
static bool rs_plan(long long rows, int No, int Mi, RsPlan& p) {
  if (rows < 1 || rows > (1LL << 30) || No < 1 || No > 1024 || Mi < 1 || Mi > 512) return false;
  const int nbo = (No + 15) / 16, nbi = (Mi + 15) / 16;
  p.tiles_i = (nbi + kRgTileBlocks - 1) / kRgTileBlocks;
  p.tbi = (nbi + p.tiles_i - 1) / p.tiles_i;
  const long long rows4 = (rows + 3) & ~3LL;
  const long long least = ((static_cast<long long>(No) * Mi + No + Mi - 1) / (No + Mi) + 3) & ~3LL;
  for (int tb = 2; tb <= kRgTileBlocks; tb *= 2) {
    p.tiles_o = (nbo + tb - 1) / tb;
    p.tbo = (nbo + p.tiles_o - 1) / p.tiles_o;
    p.WO = p.tbo >= 4 ? 4 : (p.tbo >= 2 ? 2 : 1);
    p.WI = 4 / p.WO;
    p.BO = (p.tbo + p.WO - 1) / p.WO;
    const int bi = (p.tbi + p.WI - 1) / p.WI;
    p.BI = bi > 4 ? 8 : (bi > 2 ? 4 : bi);
    p.PA = rg_pitch(p.WO * p.BO * 16);
    p.PB = rg_pitch(p.WI * p.BI * 16);
    const int qa = (std::min(p.tbo * 16, No) + 3) / 4 + 1, qb = (std::min(p.tbi * 16, Mi) + 3) / 4 + 1;
    const int rbmax = std::min(kRsLdsFloats / (p.PA + p.PB), kRsQuads * 256 / std::max(qa, qb)) & ~3;
    const long long cap = static_cast<long long>(kRsMaxBursts) * rbmax;
    long long run = std::min(std::max((rows * p.tiles_o * p.tiles_i / kRgCus) & ~3LL, least), rows4);
    const bool fits = run <= cap;
    if (!fits) run = cap;
    p.bursts = static_cast<int>((run + rbmax - 1) / rbmax);
    p.rb = static_cast<int>(((run + p.bursts - 1) / p.bursts + 3) & ~3LL);
    p.run = p.rb * p.bursts;
    p.groups = static_cast<int>((rows + p.run - 1) / p.run);
    if (fits) break;
  }
  return p.BO <= 2 && p.BI <= 8 && p.PA <= kRgMaxPitch && p.PB <= kRgMaxPitch;
}

// (row, quad) pair u of a thread: pair index threadIdx.x + 256 u over Q quads per row, stepped without a division
struct RsPair {
  int row, j, dq, dr, Q;
  __device__ __forceinline__ RsPair(int Q_) : dq(256 / Q_), dr(256 % Q_), Q(Q_) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));      // derived anew in every burst: hoisted out of the burst loop, the lane masks of all
                                     // the selections would spill scalar registers (as in rg_fetch)
    row = t / Q_;
    j = t - row * Q_;
  }
  __device__ __forceinline__ void next() {
    row += dq;
    j += dr;
    if (j >= Q) {
      j -= Q;
      ++row;
    }
  }
};

// A thread's floats of one operand and burst: its quads, and (threads 0 .. 2) one float of the last, incomplete quad
struct RsBurst {
  f32x4 v[kRsQuads];
  float tail;
};

// every quad of a burst of nr rows of a [.., W] matrix behind r (record count: 4 n bytes, n = nr W) that touches the
// tile's columns [c0, c0 + cw): quad j of row `row` is the aligned 16 bytes at float (row W + c0 & ~3) + 4 j.  Branch-free,
// so that every load is in flight before the first wait: a quad that is not wholly in front of the n-th float (rows
// behind the burst, pairs behind the last) is asked for far outside the record count and comes back as zeros.  The one
// quad that straddles the n-th float is never requested as a quad: its n & 3 floats are fetched one each by threads 0 .. 2
__device__ __forceinline__ void rs_fetch(rsrc_t r, int n, int W, int c0, int cw, int rb, RsBurst& s) {
  RsPair pr(((cw + 3) >> 2) + 1);
#pragma unroll
  for (int u = 0; u < kRsQuads; ++u, pr.next()) {
    const int f = ((pr.row * W + c0) & ~3) + 4 * pr.j;
    s.v[u] = buf_load4(r, pr.row < rb && f + 4 <= n ? static_cast<unsigned>(f) * 4u : kOob);
  }
  const int ft = (n & ~3) + static_cast<int>(threadIdx.x);
  s.tail = buf_load1(r, ft < n ? static_cast<unsigned>(ft) * 4u : kOob);
}

// the selection: each float of a quad to dst[row][column - c0] when its column is in the tile.  Rows behind the burst's
// last get the zeros rs_fetch left: a shorter last burst overwrites what the burst before it put there.  The floats of
// the straddling quad are written by the threads that hold them, and by nobody else
__device__ __forceinline__ void rs_put(const RsBurst& s, float* dst, int n, int W, int c0, int cw, int rb, int pitch) {
  RsPair pr(((cw + 3) >> 2) + 1);
  const int fs = n & ~3;
#pragma unroll
  for (int u = 0; u < kRsQuads; ++u, pr.next()) {
    const int start = pr.row * W + c0;
    const int f = (start & ~3) + 4 * pr.j;
    const int col0 = f - start;      // -3 .. cw + 3
    if (pr.row < rb) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = col0 + e;
        if (c >= 0 && c < cw && !(f == fs && f + e < n)) dst[pr.row * pitch + c] = s.v[u][e];
      }
    }
  }
  const int ft = fs + static_cast<int>(threadIdx.x);
  if (ft < n) {
    const int row = ft / W, c = ft - row * W - c0;
    if (c >= 0 && c < cw) dst[row * pitch + c] = s.tail;
  }
}

template <int BO, int BI>
__global__ __launch_bounds__(256) void mlp_dw_ragged_short_kernel(RsArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kRsLdsFloats];
  __shared__ unsigned ticket;
  const RsPlan& p = a.p;
  const int lane = lane_id(), wave = wave_id_uniform();
  const int tile = static_cast<int>(blockIdx.y);
  const int to = tile / p.tiles_i, ti = tile - to * p.tiles_i;
  const int o0 = to * p.tbo * 16, i0 = ti * p.tbi * 16;
  const int cwa = min(p.tbo * 16, a.No - o0), cwb = min(p.tbi * 16, a.Mi - i0);
  float* lds_b = lds + p.rb * p.PA;

  const long long row0 = static_cast<long long>(blockIdx.x) * p.run;
  const long long left = a.rows - row0;                    // >= 1: groups = ceil(rows / run)
  const int nrun = left < p.run ? static_cast<int>(left) : p.run;
  const int nb = (nrun + p.rb - 1) / p.rb;
  RsBurst sa, sb;
  auto fetch = [&](int b) {
    const long long r0 = row0 + static_cast<long long>(b) * p.rb;
    const int nr = min(p.rb, nrun - b * p.rb);
    rs_fetch(make_rsrc(a.dz + r0 * a.No, static_cast<unsigned>(nr * a.No) * 4u), nr * a.No, a.No, o0, cwa, p.rb, sa);
    rs_fetch(make_rsrc(a.x + r0 * a.Mi, static_cast<unsigned>(nr * a.Mi) * 4u), nr * a.Mi, a.Mi, i0, cwb, p.rb, sb);
  };

  fetch(0);
  // the columns behind the tile: zero from here on (no burst writes them)
  for (int t = threadIdx.x; t < p.rb * (p.PA + p.PB); t += 256) lds[t] = 0.0f;
  __syncthreads();

  f32x4 acc[BO][BI];
#pragma unroll
  for (int f = 0; f < BO; ++f) {
#pragma unroll
    for (int g = 0; g < BI; ++g) acc[f][g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int wo = wave % p.WO, wi = wave / p.WO;
  const float* pa = lds + (lane >> 4) * p.PA + wo * 16 + (lane & 15);
  const float* pb = lds_b + (lane >> 4) * p.PB + wi * 16 + (lane & 15);
  const int a_blk = p.WO * 16, b_blk = p.WI * 16;

#pragma unroll 1
  for (int b = 0; b < nb; ++b) {
    const int nr = min(p.rb, nrun - b * p.rb);
    rs_put(sa, lds, nr * a.No, a.No, o0, cwa, p.rb, p.PA);
    rs_put(sb, lds_b, nr * a.Mi, a.Mi, i0, cwb, p.rb, p.PB);
    __syncthreads();
    if (b + 1 < nb) fetch(b + 1);
    RLG_PIN();
    const int ksteps = (nr + 3) >> 2;      // (the rows up to the 4th are zeros)
    for (int ks = 0; ks < ksteps; ++ks) {
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
    __syncthreads();
  }
  // (as above: 10 wait states between the last MFMA and the first read of its result)
  RLG_PIN();
  asm volatile("s_nop 7\n\ts_nop 1");
  RLG_PIN();

  const int n = a.No * a.Mi;
  float* out = p.groups == 1 ? a.grad : a.parts + static_cast<long long>(blockIdx.x) * n;
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
  if (p.groups == 1) return;

  // The barrier orders every wave's stores (workgroup scope) in front of thread 0's fence, which releases them at agent
  // scope - cumulative, so ONE wave of the workgroup pays for it.  On this part an agent-scope release writes the XCD's
  // L2 back: fenced by every wave, as this kernel first did, the fences were 20 - 28 us of a 34 - 58 us launch
  // (profiles/dw_ragged_short.txt)
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    ticket = __hip_atomic_fetch_add(a.tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (ticket != static_cast<unsigned>(p.groups - 1)) return;
  __threadfence();                     // the last ticket: every other workgroup's partial tile is behind its fence
  // kRsSumElems elements of a thread x kRsSumGroups partials each in flight at once (the loads of a thread are otherwise
  // a chain of round trips to memory), added in index order.  One buffer resource per chunk of partials, the partial's
  // index in the VECTOR offset (the range check does not cover a scalar offset): a partial behind the last is behind the
  // record count, is not fetched and reads as +0.0, which changes no sum
  const int ne = cwa * cwb;
#pragma unroll 1
  for (int t0 = threadIdx.x; t0 < ne; t0 += 256 * kRsSumElems) {
    unsigned eoff[kRsSumElems];
    double s[kRsSumElems];
#pragma unroll
    for (int q = 0; q < kRsSumElems; ++q) {
      const int t = t0 + 256 * q < ne ? t0 + 256 * q : t0;      // (behind the tile: t0's element again, not stored)
      const int oc = t / cwb, ic = t - oc * cwb;
      eoff[q] = static_cast<unsigned>((o0 + oc) * a.Mi + i0 + ic) * 4u;
      s[q] = 0.0;
    }
#pragma unroll 1
    for (int g0 = 0; g0 < p.groups; g0 += kRsSumGroups) {
      const int ng = min(kRsSumGroups, p.groups - g0);
      const rsrc_t r = make_rsrc(a.parts + static_cast<long long>(g0) * n, static_cast<unsigned>(ng * n) * 4u);
      float v[kRsSumElems][kRsSumGroups];
#pragma unroll
      for (int k = 0; k < kRsSumGroups; ++k) {
#pragma unroll
        for (int q = 0; q < kRsSumElems; ++q)
          v[q][k] = buf_load1(r, eoff[q] + static_cast<unsigned>(k * n) * 4u);
      }
#pragma unroll
      for (int k = 0; k < kRsSumGroups; ++k) {
#pragma unroll
        for (int q = 0; q < kRsSumElems; ++q) s[q] += static_cast<double>(v[q][k]);
      }
    }
#pragma unroll
    for (int q = 0; q < kRsSumElems; ++q) {
      if (t0 + 256 * q < ne) a.grad[eoff[q] >> 2] = static_cast<float>(s[q]);
    }
  }
  if (threadIdx.x == 0) a.tickets[tile] = 0u;
}

template <int BO>
static bool rs_launch(const RsArgs& a, dim3 grid, hipStream_t st) {
  switch (a.p.BI) {
    case 1: hipLaunchKernelGGL((mlp_dw_ragged_short_kernel<BO, 1>), grid, dim3(256), 0, st, a); return true;
    case 2: hipLaunchKernelGGL((mlp_dw_ragged_short_kernel<BO, 2>), grid, dim3(256), 0, st, a); return true;
    case 4: hipLaunchKernelGGL((mlp_dw_ragged_short_kernel<BO, 4>), grid, dim3(256), 0, st, a); return true;
    case 8: hipLaunchKernelGGL((mlp_dw_ragged_short_kernel<BO, 8>), grid, dim3(256), 0, st, a); return true;
  }
  return false;
}

static long long rs_workspace(const RsPlan& p, int n) {
  return kRsCounters + (p.groups > 1 ? static_cast<long long>(p.groups) * n : 0);
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

long long rlg_mlp_dw_ragged_short_workspace(long long rows, int out_features, int in_features) {
  rlg::RsPlan p;
  if (!rlg::rs_plan(rows, out_features, in_features, p)) return 0;
  return rlg::rs_workspace(p, out_features * in_features);
}

int rlg_mlp_dw_ragged_short(const rlg_dw_ragged* d, void* stream) {
  if (d == nullptr || d->dz == nullptr || d->x == nullptr || d->grad == nullptr || d->workspace == nullptr)
    return static_cast<int>(hipErrorInvalidValue);
  rlg::RsArgs a;
  if (!rlg::rs_plan(d->rows, d->out_features, d->in_features, a.p)) return static_cast<int>(hipErrorNotSupported);
  if (((reinterpret_cast<uintptr_t>(d->dz) | reinterpret_cast<uintptr_t>(d->x) | reinterpret_cast<uintptr_t>(d->grad)
        | reinterpret_cast<uintptr_t>(d->workspace)) & 15u) != 0)
    return static_cast<int>(hipErrorNotSupported);
  if (d->workspace_floats < rlg::rs_workspace(a.p, d->out_features * d->in_features))
    return static_cast<int>(hipErrorInvalidValue);
  a.dz = d->dz;
  a.x = d->x;
  a.grad = d->grad;
  a.tickets = reinterpret_cast<unsigned*>(d->workspace);
  a.parts = d->workspace + rlg::kRsCounters;
  a.rows = d->rows;
  a.No = d->out_features;
  a.Mi = d->in_features;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(a.p.groups, a.p.tiles_o * a.p.tiles_i);
  if (!(a.p.BO == 1 ? rlg::rs_launch<1>(a, grid, st) : rlg::rs_launch<2>(a, grid, st)))
    return static_cast<int>(hipErrorNotSupported);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
