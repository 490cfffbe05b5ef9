// Shared pieces of the sequence-persistent recurrent kernels (csrc/lstm.hip, lstm_wide.hip, gru.hip, gru_wide.hip).
//
// The eight kernels are two things multiplied out:
//   * a SCHEME for the per-timestep products  W_hh . h  (forward) and  W_hh^T . dgates  (backward), which knows the
//     cell only by its number of gates NG (LSTM 4, GRU 3):
//       narrow (16 / 32 / 64 units): W_hh in LDS, VALU FMAs, 256 threads, a tile of 16, 8 or 4 sequences; thread
//         (j = tid % H, grp = tid / H) owns hidden unit j of the R sequences grp*R .. grp*R + R - 1 of the tile;
//       wide (128 units): W_hh in registers as v_mfma_f32_16x16x4_f32 fragments, 1,024 threads, a tile of 16;
//   * a CELL: what a hidden unit does with its pre-activations, forward and backward, which does not know the scheme.
// Each scheme and each cell formula is written once, here; the .hip files hold the kernels (argument lists, LDS
// layout, the time loop, loads and stores) and what is specific to their cell or width.
//
// Common to all: rows ordered seq*T + t; where dones[seq*T + t] is set the state ENTERING step t is zeroed (`keep`);
// a slot of the last tile past S aliases sequence S - 1, computes along and stores nothing.
//
// Arithmetic: the library is compiled with -ffp-contract=off and the tests compare bits, so the operations and the
// parenthesisation of the cell formulas are part of the contract.  The only fused multiply-adds are the spelled-out
// __builtin_fmaf of the narrow products and the MFMAs.
//
// Known asymmetries between the kernels.  They change generated code or memory traffic, so they are kept as they were
// written; whoever touches one decides about it on purpose:
//   * the GRU forwards load no gate inputs for slots past S (the owner of S - 1 overwrites them in the same step); the
//     LSTM forwards load them;
//   * the GRU backwards and the wide LSTM backward skip the W_hh load when T = 1 and `break` at t = 0 (nothing consumes
//     d h_{-1}); the narrow LSTM backward does neither;
//   * launch_lstm_bwd_wide does not check that w_hh is 16-byte aligned (its loads are scalar); the other three wide
//     launchers do, although only the two forwards load 16 bytes at a time.
//
// Paired launches.  Separate actor / critic trunks run two recurrences of one shape (cell, H, S, T) that do not depend
// on each other, each bound by its chain of T dependent steps and, at ceil(S / tile) workgroups, far from filling the
// chip.  Every kernel therefore has a paired form: the grid gets a second row, blockIdx.y (uniform over the workgroup,
// so the choice is scalar: selects between kernel-argument words, no lane ever branches on it) picks problem A or B,
// and the workgroup runs the body of the single kernel on it.  The tile is chosen from ONE problem's S exactly as
// for a single launch, so a paired launch computes, bit for bit, what the two single launches compute; it inherits
// the asymmetries above.  The problems' argument sets travel by value as the *Args structs below.
#pragma once

#include <type_traits>

#include "rlg_device.hpp"
#include "rlg_hip.h"

namespace rlg {

// ------------------------------------------------------------------------------------------- device, both schemes

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// Slot s of the grid's sequence axis: `seq` is the sequence it reads, `live` whether it may store.
template <typename Index>
__device__ __forceinline__ void tile_slot(int s, int S, Index& seq, bool& live) {
  live = s < S;
  seq = live ? s : S - 1;
}

// 0 where step `row` starts a new episode (the state entering it is zeroed), else 1
__device__ __forceinline__ float step_keep(const uint8_t* dones, long long row) {
  return (dones && dones[row]) ? 0.0f : 1.0f;
}

// One problem's arguments: the fields of the public descriptor (include/rlg_hip.h states them, in the order of the
// single kernels' argument lists), under the name the paired kernels' symbols carry.  complete(): no required pointer
// is NULL; shares_output(): a buffer this problem writes is the one the other writes under the same name;
// positional(fn): fn(the fields as the single kernel takes them).
static inline bool same_buffer(const void* p, const void* q) { return p != nullptr && p == q; }

struct LstmFwdArgs : rlg_lstm_fwd {
  template <typename Fn>
  int positional(Fn fn) const { return fn(gates, w_hh, h0, c0, dones, out, c_all, hprev, hT, cT); }
  bool complete() const { return gates && w_hh && h0 && c0 && out; }
  bool shares_output(const LstmFwdArgs& o) const {
    return same_buffer(gates, o.gates) || same_buffer(out, o.out) || same_buffer(c_all, o.c_all) ||
           same_buffer(hprev, o.hprev) || same_buffer(hT, o.hT) || same_buffer(cT, o.cT);
  }
};

struct LstmBwdArgs : rlg_lstm_bwd {
  template <typename Fn>
  int positional(Fn fn) const { return fn(gates, c_all, c0, dones, w_hh, d_out, d_gates); }
  bool complete() const { return gates && c_all && c0 && w_hh && d_out && d_gates; }
  bool shares_output(const LstmBwdArgs& o) const { return same_buffer(d_gates, o.d_gates); }
};

struct GruFwdArgs : rlg_gru_fwd {
  template <typename Fn>
  int positional(Fn fn) const { return fn(gates, w_hh, b_hh, h0, dones, out, hn_all, hprev, hT); }
  bool complete() const { return gates && w_hh && b_hh && h0 && out; }
  bool shares_output(const GruFwdArgs& o) const {
    return same_buffer(gates, o.gates) || same_buffer(out, o.out) || same_buffer(hn_all, o.hn_all) ||
           same_buffer(hprev, o.hprev) || same_buffer(hT, o.hT);
  }
};

struct GruBwdArgs : rlg_gru_bwd {
  template <typename Fn>
  int positional(Fn fn) const { return fn(gates, hn_all, hprev, dones, w_hh, d_out, d_gx, d_gh); }
  bool complete() const { return gates && hn_all && hprev && w_hh && d_out && d_gx && d_gh; }
  bool shares_output(const GruBwdArgs& o) const { return same_buffer(d_gx, o.d_gx) || same_buffer(d_gh, o.d_gh); }
};

// The problem of this workgroup in a paired launch (grid row 0: a, row 1: b)
template <typename A>
__device__ __forceinline__ const A& pair_problem(const A& a, const A& b) {
  return blockIdx.y != 0 ? b : a;
}

// ------------------------------------------------------------------------------------------- device, narrow scheme

constexpr int kSeqThreads = 256;
constexpr int kSeqMaxPerBlock = 16;

// wT [H][NG*H]: wT[k][r] = w_hh[r][k], for the forward (LDS write contiguous, global read strided: L2)
template <int NG, int H>
__device__ __forceinline__ void narrow_stage_w_transposed(float* wT, const float* w_hh) {
  constexpr int G = NG * H;
  for (int idx = threadIdx.x; idx < G * H; idx += kSeqThreads) {
    const int k = idx / G, r = idx - k * G;
    wT[idx] = w_hh[r * H + k];
  }
}

// w [NG*H][H] as stored, for the backward
template <int NG, int H>
__device__ __forceinline__ void narrow_stage_w(float* w, const float* w_hh) {
  for (int idx = threadIdx.x; idx < NG * H * H; idx += kSeqThreads) w[idx] = w_hh[idx];
}

// The forward product  acc[g][r] = sum_k w_hh[g*H + j][k] * h[grp*R + r][k]  is NOT in here: lstm.hip and gru.hip each
// keep their copy (a k loop under `#pragma unroll 4` around R x NG FMAs).  Written as a function of NG - the whole
// loop or one k step of it, gate rows in a loop or spelled out - the same IR reaches the optimiser with its blocks in
// another order and comes out with other register counts wherever a thread owns two or more sequences (LSTM 72 -> 58
// at H = 32 / SB = 16, GRU 62 -> 66 with occupancy 8 -> 7 there).  The backward product below does not do that.

// acc[r] = sum_row dgb[grp*R + r][row] * w_hh[row][j];  dgb is the tile's [SB][NG*H] gate gradients
template <int NG, int H, int R>
__device__ __forceinline__ void narrow_bwd_product(float (&acc)[R], const float* w, const float* dgb, int j, int grp) {
  constexpr int G = NG * H;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0f;
#pragma unroll 4
  for (int row = 0; row < G; ++row) {
    const float wv = w[row * H + j];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(dgb[(grp * R + r) * G + row], wv, acc[r]);
  }
}

// ------------------------------------------------------------------------------------------- device, wide scheme
//
// Forward, per timestep: pre[4H x SB] = A[4H x H] . h[H x SB].  The 512 rows of A are 32 blocks of 16; wave w owns
// blocks 2w and 2w + 1 (2 blocks x 32 k-steps = 64 A registers, 64 MFMAs per step, two independent accumulator
// chains).  Block b holds hidden units 4b .. 4b + 3, A row 4u + g = W_hh row g*H + 4b + u for g < NG and zero for
// g >= NG.  A lane's D fragment is rows 4q .. 4q + 3 (q = lane / 16) of column n = lane % 16: the NG pre-activations
// of unit 4b + q of ONE sequence, so the cell update runs in registers.  k order inside a block is free as long as A
// and B agree: lane quad q supplies k = 32q + s at MFMA step s, so a lane's B values of a step are 32 consecutive
// floats of its sequence's h row (8 ds_read_b128) and its A values 32 consecutive floats of a W_hh row (8 global
// 16-byte loads, once per launch).  h goes through a double-buffered LDS tile [2][16][132] (rows padded by 4 floats:
// conflict-free 16-byte reads), one barrier per step.
//
// Backward, per timestep: dh_prev[H x SB] = W_hh^T[H x NG*H] . dgates[NG*H x SB].  Wave w owns the 16 hidden units
// 16 (w % 8) .. + 15 and the half w / 8 of the gate rows: 1 block x KQ k-steps (KQ = NG*H / 8: 64 for the LSTM, 48
// for the GRU) = KQ A registers, two accumulator chains over alternate k-steps.  The cell-level arithmetic is thread
// (unit j = tid % 128, sequences 2 (tid / 128), + 1), global accesses contiguous over j; its gate gradients go to LDS
// [16][NG*H + 4], and the two half-K partial sums come back through LDS [2][16][132] to be added in a fixed order:
// deterministic, no atomics.
//
// The tile is 16 sequences for every (S, T): 16 is the MFMA's N, so a smaller tile would not shorten a step, and a
// 32-sequence tile needs a second set of B registers and accumulators that the 128-register budget of a 16-wave
// workgroup does not have.

constexpr int kWideH = 128;
constexpr int kWideSB = 16;                 // sequences per workgroup = N of the MFMA
constexpr int kWideThreads = 1024;          // 16 waves: 4 per SIMD, 128 registers each
constexpr int kWidePad = 4;                 // floats added to a row of an LDS tile
constexpr int kWideHP = kWideH + kWidePad;  // padded row of an [SB][H] LDS tile

// forward A fragments: row i = n = 4u + g of blocks 2 wave, 2 wave + 1; k = 32 q + s
template <int NG>
__device__ __forceinline__ void wide_fwd_load_a(float (&wreg)[2][32], const float* w_hh, int wave, int n,
                                                int q) {
  constexpr int H = kWideH;
  const int ag = n & 3;
#pragma unroll
  for (int bb = 0; bb < 2; ++bb) {
    const int b = 2 * wave + bb;
    const int wrow = (ag < NG ? ag : 0) * H + 4 * b + (n >> 2);
    const f32x4* src = reinterpret_cast<const f32x4*>(w_hh + wrow * H + 32 * q);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const f32x4 x = src[v];
      wreg[bb][4 * v + 0] = ag < NG ? x[0] : 0.0f;
      wreg[bb][4 * v + 1] = ag < NG ? x[1] : 0.0f;
      wreg[bb][4 * v + 2] = ag < NG ? x[2] : 0.0f;
      wreg[bb][4 * v + 3] = ag < NG ? x[3] : 0.0f;
    }
  }
}

// acc[bb] = A(block 2 wave + bb) . h;  hb: the lane's 32 floats of its sequence's h row
__device__ __forceinline__ void wide_fwd_product(f32x4 (&acc)[2], const float (&wreg)[2][32], const f32x4* hb) {
  acc[0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  acc[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const f32x4 hv = hb[v];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[0][4 * v + e], hv[e], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[1][4 * v + e], hv[e], acc[1], 0, 0, 0);
    }
  }
}

// backward A fragments of W_hh^T: A[i = unit 16 mb + n][k = gate row 4 KQ kh + KQ q + s]; left zero when T = 1
template <int KQ>
__device__ __forceinline__ void wide_bwd_load_a(float (&wreg)[KQ], const float* w_hh, int T, int mb,
                                                int kh, int n, int q) {
#pragma unroll
  for (int s = 0; s < KQ; ++s) wreg[s] = 0.0f;
  if (T > 1) {
    const float* src = w_hh + (4 * KQ * kh + KQ * q) * kWideH + 16 * mb + n;
#pragma unroll
    for (int s = 0; s < KQ; ++s) wreg[s] = src[s * kWideH];
  }
}

// dhp4 (units 16 mb + 4 q .. + 3 of sequence n, half kh) = the wave's half of W_hh^T . dgates;
// bsrc: the lane's KQ floats of its sequence's gate-gradient row
template <int KQ>
__device__ __forceinline__ void wide_bwd_product(float* dhp4, const float (&wreg)[KQ], const f32x4* bsrc) {
  f32x4 acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int v = 0; v < KQ / 4; ++v) {
    const f32x4 bv = bsrc[v];
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 0], bv[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 1], bv[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 2], bv[2], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[4 * v + 3], bv[3], acc1, 0, 0, 0);
  }
  *reinterpret_cast<f32x4*>(dhp4) = acc0 + acc1;
}

// ------------------------------------------------------------------------------------------- cell formulas

// LSTM, gate order (i, f, g, o) as torch.nn.LSTM.  x[g * xs]: gate inputs (x W_ih^T + b_ih + b_hh), read here, one
// in front of each activation; a: W_hh . h; c: the cell state, entering and leaving.  -> g: activated gates; returns h.
__device__ __forceinline__ float lstm_fwd_point(const float* x, int xs, const float (&a)[4], float keep, float& c,
                                                float (&g)[4]) {
  g[0] = sigmoid_f(x[0 * xs] + keep * a[0]);
  g[1] = sigmoid_f(x[1 * xs] + keep * a[1]);
  g[2] = tanhf(x[2 * xs] + keep * a[2]);
  g[3] = sigmoid_f(x[3 * xs] + keep * a[3]);
  c = g[1] * (c * keep) + g[0] * g[2];
  return g[3] * tanhf(c);
}

// g: activated gates, ct: c_t, c_in: c entering step t (after the reset), dh: d loss / d h_t in total,
// dc_next: d loss / d c_t from step t + 1, replaced by the one for step t - 1.  -> dg: d gate pre-activations.
__device__ __forceinline__ void lstm_bwd_point(const float (&g)[4], float ct, float c_in, float dh, float keep,
                                               float& dc_next, float (&dg)[4]) {
  const float gi = g[0], gf = g[1], gg = g[2], go = g[3];
  const float tc = tanhf(ct);
  const float d_o = dh * tc;
  const float dc = dc_next + (dh * go) * (1.0f - tc * tc);
  dg[0] = (dc * gg) * (gi * (1.0f - gi));
  dg[1] = (dc * c_in) * (gf * (1.0f - gf));
  dg[2] = (dc * gi) * (1.0f - gg * gg);
  dg[3] = d_o * (go * (1.0f - go));
  dc_next = (dc * gf) * keep;
}

// GRU, gate order (r, z, n) as torch.nn.GRU.  x: gate inputs (x W_ih^T + b_ih), a: W_hh . h, b: b_hh of the unit,
// hp: the state entering the step (after the reset).  -> g: activated gates, hn = W_hn h + b_hn; returns h.
__device__ __forceinline__ float gru_fwd_point(const float (&x)[3], const float (&a)[3], const float (&b)[3],
                                               float keep, float hp, float (&g)[3], float& hn) {
  g[0] = sigmoid_f(x[0] + (keep * a[0] + b[0]));
  g[1] = sigmoid_f(x[1] + (keep * a[1] + b[1]));
  hn = keep * a[2] + b[2];
  g[2] = tanhf(x[2] + g[0] * hn);
  return (1.0f - g[1]) * g[2] + g[1] * hp;
}

// -> dgx = (dr, dz, dn), the input side's gradient; the hidden side's is (dr, dz, dnr = dn * r).
// Returns dh * z, the part of d h_{t-1} that does not go through W_hh.
__device__ __forceinline__ float gru_bwd_point(const float (&g)[3], float hn, float hp, float dh, float (&dgx)[3],
                                               float& dnr) {
  const float gr = g[0], gz = g[1], gn = g[2];
  const float dn = (dh * (1.0f - gz)) * (1.0f - gn * gn);
  dgx[1] = (dh * (hp - gn)) * (gz * (1.0f - gz));
  dgx[0] = (dn * hn) * (gr * (1.0f - gr));
  dgx[2] = dn;
  dnr = dn * gr;
  return dh * gz;
}

// ------------------------------------------------------------------------------------------- host

// Launches Kernel(args...) on ceil(S / sb) workgroups per problem (Problems = 2: a paired kernel, the grid's second
// row); `shm` bytes of dynamic LDS are allowed once per instantiation.
template <auto Kernel, int Problems = 1, typename... Args>
static int launch_tile(int S, int sb, int threads, size_t shm, hipStream_t st, Args... args) {
  static bool attr_set = false;
  if (shm != 0 && !attr_set) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(shm));
    if (e != hipSuccess) return static_cast<int>(e);
    attr_set = true;
  }
  hipLaunchKernelGGL(Kernel, dim3((S + sb - 1) / sb, Problems), dim3(threads), shm, st, args...);
  RLG_RETURN_LAUNCH_STATUS();
}

// Sequences per block of the narrow scheme: 16 (at H = 64 four per thread: every W_hh value read from LDS feeds 4
// FMAs) when that still gives >= 256 blocks, otherwise fewer, so that a 1,024-sequence minibatch uses the whole chip
// instead of 64 CUs.
static int seq_per_block(int S, int H) {
  const int min_sb = kSeqThreads / H;                  // one sequence per thread group at least
  int sb = kSeqMaxPerBlock;
  while (sb > min_sb && (S + sb - 1) / sb < 256) sb >>= 1;
  return sb;
}

// One or two problems on one kernel pair: the single kernel takes problem 0's fields as positional arguments, the
// paired kernel both problems by value; grid and LDS are those of ONE problem either way.
template <auto Kernel, auto PairKernel, typename A>
static int launch_problems(const A* p, int count, int S, int T, int sb, int threads, size_t shm, hipStream_t st) {
  if (count == 2) return launch_tile<PairKernel, 2>(S, sb, threads, shm, st, p[0], p[1], S, T);
  return p[0].positional([&](auto... field) { return launch_tile<Kernel>(S, sb, threads, shm, st, field..., S, T); });
}

// The wide forms' 16-byte rule for w_hh, on each problem
template <typename A>
static bool wide_aligned(const A* p, int count) {
  uintptr_t bits = 0;
  for (int i = 0; i < count; ++i) bits |= reinterpret_cast<uintptr_t>(p[i].w_hh);
  return (bits & 15u) == 0;
}

// A kernel family F (one cell, one direction) gives: F::Args, its problems' type; F::kernel<H, SB> and
// F::pair_kernel<H, SB>, the narrow kernels; F::lds_floats(H, SB), their dynamic LDS; F::wide(problems, count, S, T,
// stream), the 128-unit launcher.
template <typename F, int H, int SB>
static int launch_narrow_sb(const typename F::Args* p, int count, int S, int T, hipStream_t st) {
  if constexpr (SB < kSeqThreads / H) {
    return static_cast<int>(hipErrorInvalidValue);
  } else {
    return launch_problems<F::template kernel<H, SB>, F::template pair_kernel<H, SB>>(
        p, count, S, T, SB, kSeqThreads, F::lds_floats(H, SB) * sizeof(float), st);
  }
}

template <typename F, int H>
static int launch_narrow(const typename F::Args* p, int count, int S, int T, hipStream_t st) {
  switch (seq_per_block(S, H)) {                        // S of ONE problem, also for a pair
    case 16: return launch_narrow_sb<F, H, 16>(p, count, S, T, st);
    case 8: return launch_narrow_sb<F, H, 8>(p, count, S, T, st);
    default: return launch_narrow_sb<F, H, 4>(p, count, S, T, st);
  }
}

// A file's kernels stand in its code object in the order of their first use.  lstm.hip and gru.hip assert this for
// their forward and backward family in front of their entry points: that names F's single kernels, in the order
// launch_narrow reaches them, ahead of every paired kernel - the order the files have always had - so that a change on
// the host side leaves a file's disassembly comparable hash for hash (profiles/rnn_seq_descriptors.txt).
template <typename F>
constexpr bool single_kernels_first() {
  return F::template kernel<16, 16> && F::template kernel<32, 16> && F::template kernel<32, 8> &&
         F::template kernel<64, 16> && F::template kernel<64, 8> && F::template kernel<64, 4>;
}

static bool seq_hidden_supported(int hidden) { return hidden == 16 || hidden == 32 || hidden == 64 || hidden == 128; }

// The four entry points: `count` (1 or 2) problems of one shape.  Everything is checked here, on the host, before the
// runtime is asked for anything; the wide launchers' alignment rule comes last.
template <typename F, typename D>
static int launch_seq(const D* problems, int count, int hidden, int S, int T, void* stream) {
  using A = typename F::Args;
  static_assert(std::is_base_of_v<D, A> && sizeof(A) == sizeof(D), "F::Args is the public descriptor and nothing else");
  constexpr int invalid = static_cast<int>(hipErrorInvalidValue);
  if (problems == nullptr || (count != 1 && count != 2)) return invalid;
  if (S <= 0 || T <= 0 || !seq_hidden_supported(hidden)) return invalid;
  A p[2] = {};
  for (int i = 0; i < count; ++i) {
    static_cast<D&>(p[i]) = problems[i];
    if (!p[i].complete()) return invalid;
  }
  if (count == 2 && p[0].shares_output(p[1])) return invalid;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  switch (hidden) {
    case 16: return launch_narrow<F, 16>(p, count, S, T, st);
    case 32: return launch_narrow<F, 32>(p, count, S, T, st);
    case 64: return launch_narrow<F, 64>(p, count, S, T, st);
    default: return F::wide(p, count, S, T, st);        // 128
  }
}

}  // namespace rlg
