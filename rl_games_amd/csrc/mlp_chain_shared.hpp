// What mlp_chain.hip (unit-structured and pipelined exact-product kernels, the C entry points of the chain) and
// mlp_chain_lean.hip (the lean 16-row kernels and theirs) share: the host-side helpers behind the entry points.  Round 5:
// the two kernel generations that survive live in files of their own.  The launchers of the split-product kernels
// (mlp_chain_bx.hip, mlp_chain_bx_fwd.hip) take the launch helper and chain_elu_only from here.
#pragma once

#include "mlp_chain_common.hpp"

namespace rlg {

// ---- host side (defined in mlp_chain.hip) ------------------------------------------------------------------------------
// ChainArgs from the C arrays: layer table, activation kinds; non-zero: a shape / pointer the kernels do not take
int chain_fill(ChainArgs& args, int num_layers, const float* const* weights, const int* in_features, const int* out_features,
               const int* acts);
// the same for the kernels that read their weights from fragments: no weight pointers (layer[L].w = nullptr), no checks of them
int chain_fill_shape(ChainArgs& args, int num_layers, const int* in_features, const int* out_features, const int* acts);
// The forward half of a filled ChainArgs: bias / activation output / its row stride per layer, observations, normaliser
// state, rows.  hipErrorInvalidValue for a fold of the normaliser state (rms_batch) that would not publish into a second
// buffer set.  Which act_out entries may be null, dbg, the LDS fields and no_ksplit are the caller's.
int chain_fill_forward(ChainArgs& args, const float* const* biases_or_null, float* const* act_out, const long long* act_ld,
                       const float* x, long long ldx, const double* rms_mean, const double* rms_var, float rms_eps,
                       float* xn_out, const double* rms_batch, const long long* rms_count, double* rms_mean_out,
                       double* rms_var_out, long long* rms_count_out, long long rows);
// The backward half: H / dZ / bias partials of the hidden layers, d heads, no normaliser, rows.  Checks nothing: the entries
// that need 16-byte rows ask chain_rows16_status, which answers for missing arrays layer by layer as well.
void chain_fill_backward(ChainArgs& args, const float* const* act_in, const long long* act_ld, const float* d_out,
                         long long ld_dout, float* const* dz_out, const long long* dz_ld, double* const* bias_partials_or_null,
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
// rlg_mlp_chain_time_next: the HIP events the NEXT chain launch carries on its dispatch (taken = cleared)
void chain_take_events(hipEvent_t* ev_start, hipEvent_t* ev_stop);
// rlg_mlp_chain_gradient_maxima: where the NEXT backward launch leaves its gradient maxima (taken = cleared)
void chain_take_gradient_maxima(float** entries, int* stride);

// One chain launch with the timing events ev0 / ev1 on its dispatch when there are any - the plain launch otherwise: the
// one that stream capture takes.  Returns the launch status.  (In this form for the split-product launchers:
// rlg_mlp_chain_forward / _backward take the events for them, and the backward puts them back when it does not launch.)
template <class... P, class... A>
static int chain_launch_timed(void (*kern)(P...), int grid, int block, int lds_bytes, hipStream_t st, hipEvent_t ev0,
                              hipEvent_t ev1, const A&... a) {
  if (ev0 != nullptr)
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), static_cast<size_t>(lds_bytes), st, ev0, ev1, 0, a...);
  else
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), static_cast<size_t>(lds_bytes), st, a...);
  RLG_RETURN_LAUNCH_STATUS();
}
// The same for a launcher that no caller has taken the one-shot events for (chain_take_events): takes them, launches.
template <class... P, class... A>
static int chain_launch_kernel(void (*kern)(P...), int grid, int block, int lds_bytes, hipStream_t st, const A&... a) {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  chain_take_events(&ev0, &ev1);
  return chain_launch_timed(kern, grid, block, lds_bytes, st, ev0, ev1, a...);
}

}  // namespace rlg
