// Range guard of the split-fp16 products: one launch that looks through up to 8 fp32 arrays for
// non-finite values and, only when it finds one, leaves (tag of the first array in argument order with a hit, smallest
// offending flat index of that array) in a device-resident guard record.
//
// The split-fp16 kernels (csrc/bx_form.hpp) hold |weight| < 1023 and |hidden activation| < 4094; beyond that a plane is
// Inf and everything computed from it is Inf / NaN - never a finite wrong value.  So "did a product overflow" can be
// answered behind the launches, from what they left: the rollout's values, neglogps, mus and returns here, the
// gradient norm in the guarded optimiser launches (optim.hip, adam_pack.hip), which take the same record.
//
// The record is 4 words: [0] tag (0 = clear), [1] index, [2..3] one 64-bit key that the scan's hit path competes on.
// Clean data costs 16-byte loads, one ballot per wave and nothing else: no store, no atomic.  On a hit the wave's best
// candidate competes with compare-and-swap (device scope) on the key, and whoever raised the key publishes words 0..1
// from it, so the record does not depend on which workgroup ran first.  The key carries the launch's nonce: a record that
// was set before this launch - by an earlier scan, by an optimiser launch - holds another nonce (or none) and is left
// exactly as it is.  (The nonce is a kernel argument: a captured launch replays with the nonce of its capture, and takes
// a record that an earlier replay of itself left for one of its own.  Read and clear the record between replays.)
#include "rlg_device.hpp"

#include <atomic>

namespace rlg {

constexpr int kScanMaxArrays = 8;
constexpr int kScanBlock = 256;

struct ScanArgs {
  const float* p[kScanMaxArrays];
  long long n[kScanMaxArrays];
  unsigned tag[kScanMaxArrays];
  int num;
  unsigned nonce;              // 1 .. 2^24 - 1
  unsigned* record;
};

typedef unsigned long long u64;

// larger = better: this launch's nonce, then the earlier array, then the smaller index
__device__ __forceinline__ u64 scan_key(unsigned nonce, int array, unsigned index) {
  return (static_cast<u64>(nonce) << 40) | (static_cast<u64>(kScanMaxArrays - 1 - array) << 32) |
         static_cast<u64>(0xffffffffu - index);
}
__device__ __forceinline__ bool non_finite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u; }

#define RLG_SCAN_ORDER __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT

// one lane of a wave that found something; `mine` is the wave's best candidate
__device__ void scan_publish(const ScanArgs& a, u64 mine) {
  u64* key = reinterpret_cast<u64*>(a.record + 2);
  u64* words01 = reinterpret_cast<u64*>(a.record);
  // set before this launch?  (word 0 first: a writer of THIS launch stores it behind its swap of the key, so whoever sees
  // such a word 0 also sees this launch's nonce in the key)
  const unsigned w0 = __hip_atomic_load(a.record, RLG_SCAN_ORDER);
  u64 cur = __hip_atomic_load(key, RLG_SCAN_ORDER);
  if (w0 != 0u && (cur >> 40) != a.nonce) return;
  for (;;) {
    if ((cur >> 40) == a.nonce && cur >= mine) return;          // a better candidate holds the key: its owner publishes
    if (__hip_atomic_compare_exchange_strong(key, &cur, mine, __ATOMIC_SEQ_CST, RLG_SCAN_ORDER)) break;
  }
  // publish the key's candidate until the key is the one just published: the key only rises, every lane that raised it
  // stores afterwards, and the last store in memory order is followed by a look at the key that finds it unchanged
  u64 k = mine;
  for (;;) {
    const int array = kScanMaxArrays - 1 - static_cast<int>((k >> 32) & 7u);
    const unsigned index = 0xffffffffu - static_cast<unsigned>(k);
    __hip_atomic_store(words01, (static_cast<u64>(index) << 32) | a.tag[array], RLG_SCAN_ORDER);
    const u64 now = __hip_atomic_load(key, RLG_SCAN_ORDER);
    if (now == k) return;
    k = now;
  }
}

__global__ __launch_bounds__(kScanBlock) void range_scan_kernel(ScanArgs a) {
  const long long tid = static_cast<long long>(blockIdx.x) * kScanBlock + threadIdx.x;
  const long long stride = static_cast<long long>(gridDim.x) * kScanBlock;
  u64 best = 0;
  for (int k = 0; k < a.num && best == 0; ++k) {
    const float* p = a.p[k];
    const long long n = a.n[k];
    // [0, head) scalars up to the first 16-byte boundary, then nvec groups of 4, then the tail: < 8 scalars per array
    long long head = (4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3;
    head = head < n ? head : n;
    const long long nvec = (n - head) >> 2;
    const long long tail_begin = head + (nvec << 2);
    const long long edge = head + (n - tail_begin);
    if (tid < edge) {
      const long long i = tid < head ? tid : tail_begin + (tid - head);
      if (non_finite_bits(__float_as_uint(p[i]))) best = scan_key(a.nonce, k, static_cast<unsigned>(i));
    }
    const u32x4* v = reinterpret_cast<const u32x4*>(p + head);
    // first hit of group g (0: none)
    auto group_hit = [&](const u32x4 q, long long g) {
      u64 hit = 0;
#pragma unroll
      for (int e = 3; e >= 0; --e)
        if (non_finite_bits(q[e])) hit = scan_key(a.nonce, k, static_cast<unsigned>(head + (g << 2) + e));
      return hit;
    };
    // grid-strided, four 16-byte loads in flight per lane; the lane's later groups lie behind its first hit
    u64 hit = 0;
    long long g = tid;
    for (; hit == 0 && g + 3 * stride < nvec; g += 4 * stride) {
      const u32x4 q0 = v[g], q1 = v[g + stride], q2 = v[g + 2 * stride], q3 = v[g + 3 * stride];
      const u64 h0 = group_hit(q0, g), h1 = group_hit(q1, g + stride);
      const u64 h2 = group_hit(q2, g + 2 * stride), h3 = group_hit(q3, g + 3 * stride);
      hit = h0 ? h0 : (h1 ? h1 : (h2 ? h2 : h3));
    }
    for (; hit == 0 && g < nvec; g += stride) hit = group_hit(v[g], g);
    best = hit > best ? hit : best;
  }
  if (__ballot(best != 0) == 0ull) return;                       // the clean path ends here
  // the wave's best candidate, then one lane competes for the record
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(best, o, kWave);
    best = other > best ? other : best;
  }
  if (lane_id() == 0) scan_publish(a, best);
}

static std::atomic<unsigned> g_scan_nonce{0};

}  // namespace rlg

extern "C" {

int rlg_range_scan(int num_arrays, const float* const* arrays, const long long* counts, const int* tags,
                   unsigned* record, void* stream) {
  using namespace rlg;
  if (record == nullptr || num_arrays < 0 || num_arrays > kScanMaxArrays) return static_cast<int>(hipErrorInvalidValue);
  if (num_arrays > 0 && (arrays == nullptr || counts == nullptr || tags == nullptr)) return static_cast<int>(hipErrorInvalidValue);
  if (reinterpret_cast<uintptr_t>(record) % 16 != 0) return static_cast<int>(hipErrorInvalidValue);
  ScanArgs a = {};
  long long work = 0;
  for (int k = 0; k < num_arrays; ++k) {
    // (the index word has 32 bits; a tag of 0 would read as "clear"; fp32 arrays are 4-byte aligned)
    if (counts[k] < 0 || counts[k] > 0xffffffffll || tags[k] == 0) return static_cast<int>(hipErrorInvalidValue);
    if (counts[k] > 0 && (arrays[k] == nullptr || reinterpret_cast<uintptr_t>(arrays[k]) % 4 != 0))
      return static_cast<int>(hipErrorInvalidValue);
    if (counts[k] == 0) continue;
    a.p[a.num] = arrays[k];
    a.n[a.num] = counts[k];
    a.tag[a.num] = static_cast<unsigned>(tags[k]);
    ++a.num;
    work = counts[k] > work ? counts[k] : work;
  }
  if (a.num == 0) return 0;
  unsigned nonce;
  do {
    nonce = g_scan_nonce.fetch_add(1u, std::memory_order_relaxed) + 1u;
    nonce &= 0xffffffu;
  } while (nonce == 0u);
  a.nonce = nonce;
  a.record = record;
  // 4 groups of 4 elements per lane and round of the largest array, at most 1,024 workgroups (4 per CU)
  long long grid = (work / 16 + kScanBlock - 1) / kScanBlock;
  grid = grid < 1 ? 1 : (grid > 1024 ? 1024 : grid);
  hipLaunchKernelGGL(range_scan_kernel, dim3(static_cast<int>(grid)), dim3(kScanBlock), 0,
                     static_cast<hipStream_t>(stream), a);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
