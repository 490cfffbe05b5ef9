// What mlp_chain.hip (unit-structured and pipelined exact-product kernels, the C entry points of the chain) and
// mlp_chain_lean.hip (the lean 16-row kernels and theirs) share: the host-side helpers behind the entry points.  Round 5:
// the two kernel generations that survive live in files of their own.  The launchers of the split-product kernels
// (mlp_chain_bx.hip, mlp_chain_bx_fwd.hip) take the launch helper and chain_elu_only from here.
#pragma once

#include "mlp_chain_common.hpp"

namespace rlg {

// ---- host side (defined in mlp_chain.hip) ------------------------------------------------------------------------------
// ChainArgs from the network descriptor: layer table, activation kinds; non-zero: a shape / pointer the kernels do not take
int chain_fill(ChainArgs& args, const rlg_chain_net& net);
// the same for the kernels that read their weights from fragments: no weight pointers (layer[L].w = nullptr), no checks of them
int chain_fill_shape(ChainArgs& args, const rlg_chain_net& net);
// The forward half of a filled ChainArgs: bias / activation output / its row stride per layer, observations, normaliser
// state, rows.  hipErrorInvalidValue for a fold of the normaliser state (rms_batch) that would not publish into a second
// buffer set.  Which act_out entries may be null, dbg, the LDS fields and no_ksplit are the caller's.
int chain_fill_forward(ChainArgs& args, const rlg_chain_net& net, const rlg_chain_fwd& fwd, long long rows);
// The backward half: H (act_in / act_ld: the step entries pass their forward's act_out) / dZ / bias partials of the hidden
// layers, d heads, no normaliser, no gradient maxima, rows.  Checks nothing: the entries that need 16-byte rows ask
// chain_rows16_status, which answers for missing arrays layer by layer as well.
void chain_fill_backward(ChainArgs& args, const float* const* act_in, const long long* act_ld, const rlg_chain_bwd& bwd,
                         long long rows);
// The pipelined 16-row and the lean backward kernels read H and write dZ of every hidden layer in 16-byte row accesses
// (aligned arrays, row strides and widths of whole 4-float groups, strides below 2^20).  0, or the answer of the first hidden
// layer they do not take: hipErrorInvalidValue for a missing H / dZ, hipErrorNotSupported for rows of another kind.
int chain_rows16_status(const ChainArgs& args);
// LossArgs from the C descriptor of a minibatch of `rows` rows; hipErrorInvalidValue for one the loss tile does not take
int chain_loss_args(LossArgs& loss, const rlg_ppo_loss_desc& d, long long rows);
// forward: the ELU-or-identity network (every BASELINE configuration) runs its own kernel instance
bool chain_elu_only(const ChainArgs& args);
// tools only (rlg_mlp_chain_debug_stamps): phase stamps of the next launches, or nullptr
long long* chain_debug_stamps();

// ChainQueue of a launch descriptor and the entry's stream
static inline ChainQueue chain_queue(const rlg_chain_launch& launch, void* stream) {
  return {static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(launch.ev_start_or_null),
          static_cast<hipEvent_t>(launch.ev_stop_or_null)};
}

// One chain launch with the timing events on its dispatch when there are any - the plain launch otherwise: the one that
// stream capture takes.  Returns the launch status.
template <class... P, class... A>
static int chain_launch_kernel(void (*kern)(P...), int grid, int block, int lds_bytes, const ChainQueue& q, const A&... a) {
  if (q.ev0 != nullptr)
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), static_cast<size_t>(lds_bytes), q.st, q.ev0, q.ev1, 0, a...);
  else
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), static_cast<size_t>(lds_bytes), q.st, a...);
  RLG_RETURN_LAUNCH_STATUS();
}

}  // namespace rlg
