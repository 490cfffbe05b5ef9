"""ctypes binding of librlg_hip.so (the C ABI declared in include/rlg_hip.h).

The product path has no CPU or eager-PyTorch fallback: if the HIP library is missing,
fails to load, or a launch fails, the caller gets a RuntimeError.  `torch` is imported
first on purpose - the library must bind to the HIP runtime PyTorch already loaded, so
that raw `data_ptr()` addresses and `torch.cuda.current_stream()` handles are valid.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the dlopen below)

_HERE = os.path.dirname(os.path.abspath(__file__))
# RLG_HIP_LIB: another build of the same ABI (A/B measurements of kernel variants, tools only)
LIB_PATH = os.environ.get('RLG_HIP_LIB') or os.path.join(_HERE, 'librlg_hip.so')

_c_void_p = ctypes.c_void_p
_c_int = ctypes.c_int
_c_float = ctypes.c_float
_c_double = ctypes.c_double
_c_ll = ctypes.c_longlong
_P = _c_void_p  # every device pointer crosses the boundary as an address

# name -> argtypes.  Order/meaning: include/rlg_hip.h.  All functions return int.
_PROTOTYPES = {
    'rlg_gae_strided': [_P, _P, _P, _P, _P, _P, _P, _c_int, _c_int, _c_int,
                        ctypes.POINTER(_c_ll), _c_int, _c_float, _c_float, _P],
    'rlg_gae_envmajor_supported': [_c_int],
    'rlg_gae_envmajor_num_partials': [_c_int],
    'rlg_gae_envmajor_fused': [_P, _P, _P, _P, _P, _P, _P, _P, _c_int, _c_int, _c_float,
                               _c_float, _P],
    'rlg_gae_envmajor_raw': [_P, _P, _P, _P, _P, _P, _c_int, _c_int, _c_float, _c_float, _P],
    'rlg_event_create': [ctypes.POINTER(_P)],
    'rlg_event_destroy': [_P],
    'rlg_event_elapsed_us': [_P, _P, ctypes.POINTER(_c_float)],
    'rlg_gae_envmajor_fused_timed': [_P, _P, _P, _P, _P, _P, _P, _P, _c_int, _c_int, _c_float,
                                     _c_float, _P, _P, _P],
    # experience.hip
    'rlg_rollout_store_step': [_c_int, ctypes.POINTER(_P), ctypes.POINTER(_P),
                               ctypes.POINTER(_c_int), _c_int, _c_int, _c_int, _P],
    'rlg_rollout_store_streaming': [_c_int],
    'rlg_rollout_post_step_num_blocks': [_c_int],
    'rlg_rollout_post_step': [_P, _P],               # (PostStepDesc, stream)
    'rlg_episode_meters_update': [_P, _c_int, _c_int, _c_int, _c_int, _P, _P, _P, _P, _P, _P],
    'rlg_rnn_zero_done_states': [_P, _P, _c_int, _c_int, _c_int, _P],
    'rlg_rollout_policy_head': [_P, _P],             # (PolicyHeadDesc, stream)
    # rollout_categorical.hip
    'rlg_rollout_categorical_head': [_P, _P],        # (CategoricalHeadDesc, stream)
    # play.hip
    'rlg_play_policy_head': [_P, _c_int, _c_int, _P, _P, _P, _P, _P, _c_int, _c_int, _P],
    'rlg_play_categorical_head': [_P, _c_int, ctypes.POINTER(_c_int), _c_int, _P, _P, _c_int, _P, _c_int, _P],
    'rlg_play_post_step_num_blocks': [_c_int],
    'rlg_play_post_step': [_P, _c_int, _P, _P, _P, _P, _c_int, _P],
    'rlg_play_fold': [_P, _c_int, _c_int, _c_ll, _P, _P],
    # running_stats.hip
    'rlg_column_moments_num_blocks': [_c_ll, _c_int],
    'rlg_column_moments': [_P, _P, _c_ll, _c_int, _P, _c_int, _P],
    'rlg_column_moments_segments': [_P, _c_ll, _c_int, _c_int, _P, _c_int, _P, _P],
    'rlg_rms_update': [_P, _c_int, _c_int, _c_ll, _c_int, _P, _P, _P, _P, _P],
    'rlg_rms_apply': [_P, _P, _c_ll, _c_int, _P, _P, _c_float, _c_int, _P],
    'rlg_stats_sync_flat_size': [_c_int, _P],
    'rlg_stats_sync_pack': [_c_int, _P, _P, _P, _P, _P, _P, _P, _c_int, _P],
    'rlg_stats_sync_apply': [_c_int, _P, _P, _P, _P, _P, _P, _P, _c_int, _P],
    'rlg_prepare_stats_bytes': [],
    'rlg_triple_moments_num_blocks': [_c_ll],
    'rlg_triple_moments': [_P, _P, _P, _P, _c_ll, _P, _c_int, _P],
    'rlg_prepare_finalize': [_P, _c_int, _c_int, _c_ll, _c_int, _P, _P, _P, _c_float, _P, _P, _P,
                             _c_float, _c_float, _c_float, _c_float, _P, _P],
    'rlg_prepare_apply': [_P, _P, _P, _P, _P, _P, _c_ll, _c_int, _P, _P],
    # ppo_loss.hip
    'rlg_ppo_loss_num_blocks': [_c_int],
    'rlg_ppo_loss_partials_per_block': [_c_int],
    'rlg_ppo_loss_fused': [_P, _P],                  # (PpoLossDesc, stream)
    'rlg_mlp_rowgemm_supported': [_c_int, _c_ll],
    'rlg_mlp_linear_act_forward': [_P, _c_ll, _P, _P, _P, _P, _c_ll, _c_int, _c_int, _c_int, _c_int, _P],
    'rlg_mlp_linear_act_backward': [_P, _c_ll, _P, _P, _P, _c_ll, _c_int, _c_int, _c_int, _c_int, _P],
    'rlg_mlp_dw_plan': [_c_int, _c_int, _c_int, _c_int, _P],
    'rlg_mlp_dw_launch': [_P, _P],                   # (MlpDwDesc, stream)
    'rlg_mlp_dw_launch_form': [_c_int, _P, _P],      # (form, MlpDwDesc, stream)
    'rlg_narrow_dx': [_P, _c_ll, _P, _P, _c_ll, _c_ll, _c_int, _c_int, _P],
    'rlg_narrow_dw_blocks': [_c_ll],
    'rlg_narrow_dw': [_P, _c_ll, _P, _c_ll, _P, _P, _c_ll, _c_int, _c_int, _P],
    # mlp_chain.hip
    'rlg_mlp_chain_prepare': [],
    'rlg_mlp_chain_groups': [_c_ll, _c_int, _c_int],
    'rlg_mlp_chain_num_blocks': [_c_ll, _c_int],
    'rlg_mlp_chain_lds_bytes': [_c_int, _P, _P, _c_int, _c_int],
    'rlg_mlp_chain_debug_stamps': [_P],
    'rlg_mlp_chain_split_products': [],
    'rlg_mlp_chain_forward': [_P, _P, _P, _P],       # (ChainNet, ChainFwd, ChainLaunch, stream)
    'rlg_mlp_chain_step': [_P, _P, _P, _P, _P],      # (ChainNet, ChainFwd, ChainBwd, ChainLaunch, stream)
    'rlg_mlp_chain_backward': [_P, _P, _P, _P],      # (ChainNet, ChainBwd, ChainLaunch, stream)
    # lean 16-row forward (csrc/mlp_chain_lean.hip, mlp_chain_fwd_lean_kernel)
    'rlg_mlp_chain_frags_bytes': [_c_int, _P, _P, _c_int],
    'rlg_mlp_chain_pack_frags': [_c_int, _P, _P, _P, _P, _c_int, _P, _P],
    'rlg_mlp_chain_pack_frags_both': [_c_int, _P, _P, _P, _P, _P, _P, _P],
    'rlg_mlp_chain_step_lean': [_P, _P, _P, _P, _P],      # as rlg_mlp_chain_step
    'rlg_mlp_chain_backward_lean': [_P, _P, _P, _P],      # as rlg_mlp_chain_backward
    'rlg_mlp_chain_forward_lean': [_P, _P, _P, _P],       # as rlg_mlp_chain_forward
    # mlp_chain_bx.hip
    'rlg_mlp_chain_planes_bytes': [_c_int, _P, _P, _c_int],
    'rlg_mlp_chain_planes_offset': [_c_int, _P, _P, _c_int],
    'rlg_mlp_chain_pack_planes': [_c_int, _P, _P, _P, _c_int, _P, _P],
    'rlg_mlp_chain_bx_supported': [_c_int, _P, _P, _c_ll, _c_int, _c_int],
    'rlg_lstm_supported': [_c_int],
    # sequence entries: (LstmFwd / LstmBwd / GruFwd / GruBwd array, num_problems, num_seqs, seq_len, hidden, stream)
    'rlg_lstm_seq_forward': [_P, _c_int, _c_int, _c_int, _c_int, _P],
    'rlg_lstm_seq_backward': [_P, _c_int, _c_int, _c_int, _c_int, _P],
    'rlg_gru_supported': [_c_int],
    'rlg_gru_seq_forward': [_P, _c_int, _c_int, _c_int, _c_int, _P],
    'rlg_gru_seq_backward': [_P, _c_int, _c_int, _c_int, _c_int, _P],
    # rnn_layer_norm.hip
    'rlg_rnn_layer_norm_num_blocks': [_c_ll, _c_int],
    'rlg_rnn_layer_norm_forward': [_P, _P, _P, _c_float, _P, _P, _c_ll, _c_int, _P],
    'rlg_rnn_layer_norm_backward': [_P, _P, _P, _P, _P, _P, _P, _c_int, _c_ll, _c_int, _P],
    # rnn_value_tail.hip
    'rlg_rnn_value_tail_num_blocks': [_c_ll, _c_int],
    'rlg_rnn_value_head': [_P, _P, _P, _P, _c_ll, _c_int, _P],
    'rlg_rnn_value_tail': [_P] * 13 + [_c_int, _c_ll, _c_int, _c_float, _c_int, _P],
    'rlg_value_loss': [_P, _P, _P, _P, _P, _P, _P, _c_int, _c_float, _c_int, _P],
    'rlg_ppo_loss_discrete_num_blocks': [_c_int],
    'rlg_ppo_loss_discrete_nlp': [_P, _P],           # (DiscreteLossDesc, stream)
    # ppo_diag.hip
    'rlg_ppo_diag_stats': [],
    'rlg_ppo_diag_num_blocks': [_c_int],
    'rlg_ppo_diag': [_P, _c_ll, _P, _P, _c_ll, _P, _P, _P, _c_int, _c_int, _c_float, _c_float, _P, _P, _P, _P, _P],
    'rlg_ppo_diag_moments_num_blocks': [_c_int, _c_int],
    'rlg_ppo_diag_moments': [_P, _P, _P, _c_int, _c_int, _c_int, _P, _P, _P, _c_ll, _P],
    'rlg_ppo_loss_finalize': [_P, _P],               # (LossFinalizeDesc, stream)
    # mlp_fused.hip
    'rlg_act_bwd_num_blocks': [_c_ll, _c_int],
    'rlg_act_bwd_colsum': [_P, _P, _P, _c_ll, _c_int, _c_ll, _c_int, _P, _c_int, _P],
    'rlg_colsum_finalize': [_P, _c_int, _c_int, _P, _c_int, _P],
    # ipc_allreduce.hip
    'rlg_ipc_handle_bytes': [],
    'rlg_ipc_comm_create': [_c_int, _c_int, _c_ll, ctypes.POINTER(_P), _P],
    'rlg_ipc_comm_connect': [_P, ctypes.c_char_p],
    'rlg_ipc_comm_fine_grained': [_P],
    'rlg_ipc_comm_set_timeout': [_P, _c_double],
    'rlg_ipc_comm_set_variant': [_P, _c_int],
    'rlg_ipc_comm_get_config': [_P, ctypes.POINTER(_c_int), ctypes.POINTER(_c_double)],
    'rlg_ipc_comm_error_word': [_P, ctypes.POINTER(_P)],
    'rlg_ipc_allreduce_sum': [_P, _P, _c_ll, _P],
    'rlg_ipc_allreduce_norm_blocks': [],
    'rlg_ipc_allreduce_sum_norm': [_P, _P, _c_ll, _P, _c_ll, _c_float, _P, _P],
    'rlg_ipc_comm_status': [_P, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)],
    'rlg_ipc_comm_destroy': [_P],
    # optim.hip
    'rlg_grad_norm_num_blocks': [_c_ll],
    'rlg_grad_sumsq': [_P, _c_ll, _c_float, _P, _c_int, _P, _P],
    'rlg_adam_step': [_P, _P],                       # (AdamDesc, stream)
    'rlg_rccl_available': [],
    'rlg_rccl_unique_id_bytes': [],
    'rlg_rccl_get_unique_id': [ctypes.c_char_p],
    'rlg_rccl_comm_create': [ctypes.c_char_p, _c_int, _c_int, ctypes.POINTER(_P)],
    'rlg_rccl_allreduce_sum': [_P, _P, _c_ll, _P],
    'rlg_rccl_allreduce_sum_f64': [_P, _P, _c_ll, _P],
    'rlg_rccl_comm_destroy': [_P],
    'rlg_adam_step_pack': [_P, _c_int, _P, _P, _P, _P, _P],
    # range_guard.hip and the guarded optimiser entries (optim.hip, adam_pack.hip)
    'rlg_range_scan': [_c_int, _P, _P, _P, _P, _P],
    'rlg_adam_step_guarded': [_P, _P, _P],           # (AdamDesc, guard record, stream)
    'rlg_adam_pack_guarded': [_P, _P, _c_int, _P, _P, _P, _P, _P],
}

_lib = None


class HipLibraryError(RuntimeError):
    pass


def exported_prototypes():
    return dict(_PROTOTYPES)


_RETURNS_LONG_LONG = {'rlg_mlp_dw_plan', 'rlg_stats_sync_flat_size', 'rlg_mlp_chain_planes_bytes', 'rlg_mlp_chain_planes_offset',
                      'rlg_mlp_chain_frags_bytes'}


def load():
    """dlopen librlg_hip.so once and attach argtypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f'{LIB_PATH} is not built. Run `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `make -C rl_games_amd/csrc`. rl_games_amd has no CPU fallback.')
    try:
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - depends on the box
        raise HipLibraryError(f'cannot load {LIB_PATH}: {e}') from e
    for name, argtypes in _PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f'{LIB_PATH} does not export {name}; rebuild it') from e
        fn.argtypes = argtypes
        fn.restype = _c_ll if name in _RETURNS_LONG_LONG else _c_int
    _lib = lib
    return lib


class PpoLossDesc(ctypes.Structure):
    """rlg_ppo_loss_desc (include/rlg_hip.h): the arguments of rlg_ppo_loss_fused and of a fused backward launch."""
    _fields_ = ([(n, ctypes.c_void_p) for n in (
        'mu', 'logstd', 'values', 'actions', 'old_neglogp', 'advantages', 'old_values', 'returns', 'old_mu',
        'old_sigma', 'mask_or_null', 'mask_sum_or_null', 'd_mu', 'd_values', 'partials')]
        + [(n, ctypes.c_int) for n in ('minibatch', 'actions_num', 'ld_mu', 'ld_values', 'ld_d_mu', 'ld_d_values')]
        + [(n, ctypes.c_float) for n in ('e_clip', 'critic_coef', 'bounds_coef')]
        + [(n, ctypes.c_int) for n in ('clip_value', 'use_smooth_clamp', 'bound_kind', 'write_back')])


class LossFinalizeDesc(ctypes.Structure):
    """rlg_loss_finalize_desc (include/rlg_hip.h): the arguments of rlg_ppo_loss_finalize, for launches
    that fold the loss partials alongside their own work (rlg_mlp_dw_launch)."""
    _fields_ = [('partials', ctypes.c_void_p), ('num_blocks', ctypes.c_int), ('actions_num', ctypes.c_int),
                ('minibatch', ctypes.c_int), ('masked', ctypes.c_int), ('critic_coef', ctypes.c_float),
                ('entropy_coef', ctypes.c_float), ('bounds_coef', ctypes.c_float), ('scalars8', ctypes.c_void_p),
                ('d_logstd', ctypes.c_void_p), ('kl_slot_or_null', ctypes.c_void_p),
                ('d_mu_bias_or_null', ctypes.c_void_p), ('d_value_bias_or_null', ctypes.c_void_p)]


# Every pointer field of the descriptors below is a plain address (ctypes.addressof for host arrays and descriptors):
# whoever fills one keeps what it points at alive until the entry has returned.
class DiscreteLossDesc(ctypes.Structure):
    """rlg_discrete_loss_desc (include/rlg_hip.h): the arguments of rlg_ppo_loss_discrete_nlp."""
    _fields_ = ([('logits', _P), ('ld_logits', _c_ll), ('values', _P), ('ld_values', _c_ll), ('actions', _P),
                 ('action_masks_or_null', _P), ('branch_sizes', _P), ('num_branches', _c_int)]
                + [(n, _P) for n in ('old_neglogp', 'advantages', 'old_values', 'returns', 'mask_or_null',
                                     'mask_sum_or_null')]
                + [('d_logits', _P), ('ld_d_logits', _c_ll), ('d_values', _P), ('ld_d_values', _c_ll), ('partials', _P),
                   ('minibatch', _c_int), ('e_clip', _c_float), ('critic_coef', _c_float), ('entropy_coef', _c_float),
                   ('clip_value', _c_int), ('use_smooth_clamp', _c_int), ('new_neglogp_or_null', _P)])


class PostStepDesc(ctypes.Structure):
    """rlg_post_step_desc (include/rlg_hip.h): the arguments of rlg_rollout_post_step."""
    _fields_ = ([('rewards', _P), ('dones', _P), ('time_outs', _P), ('time_outs_kind', _c_int)]
                + [(n, _P) for n in ('values', 'live_rows', 'rewards_buf', 'cur_rewards', 'cur_shaped', 'cur_lengths',
                                     'ep_partials')]
                + [(n, _c_float) for n in ('shift', 'scale', 'rmin', 'rmax')]
                + [('clamp_rewards', _c_int), ('bootstrap', _c_int), ('gamma', _c_float)]
                + [(n, _c_int) for n in ('N', 'H', 'V', 'step', 'num_agents')])


class PolicyHeadDesc(ctypes.Structure):
    """rlg_policy_head_desc (include/rlg_hip.h): the arguments of rlg_rollout_policy_head."""
    _fields_ = ([('heads', _P), ('ld', _c_int), ('value', _P), ('ld_value', _c_ll), ('value_repeat', _c_int),
                 ('logstd', _P), ('noise', _P), ('v_mean', _P), ('v_var', _P), ('eps', _c_float)]
                + [(n, _P) for n in ('actions_out', 'values_out', 'buf_actions', 'buf_mus', 'buf_sigmas', 'buf_neglogp',
                                     'buf_values', 'env_actions_out', 'act_low', 'act_high')]
                + [(n, _c_int) for n in ('N', 'H', 'A', 'step')])


class CategoricalHeadDesc(ctypes.Structure):
    """rlg_categorical_head_desc (include/rlg_hip.h): the arguments of rlg_rollout_categorical_head."""
    _fields_ = ([('logits', _P), ('ld_logits', _c_int), ('branch_sizes', _P), ('num_branches', _c_int),
                 ('exp_noise', _P), ('masks_or_null', _P), ('ld_masks', _c_int), ('value', _P), ('ld_value', _c_int),
                 ('value_repeat', _c_int), ('v_mean_or_null', _P), ('v_var_or_null', _P), ('eps', _c_float)]
                + [(n, _P) for n in ('actions_out', 'values_out', 'buf_actions', 'buf_neglogp', 'buf_values')]
                + [(n, _c_int) for n in ('num_envs', 'horizon', 'step')])


class AdamDesc(ctypes.Structure):
    """rlg_adam_desc (include/rlg_hip.h): the optimiser step of the four rlg_adam_* entries."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('params', 'grads', 'exp_avg', 'exp_avg_sq')]
                + [('n', _c_ll), ('norm_partials_or_null', ctypes.c_void_p), ('norm_blocks', _c_int),
                   ('grad_scale', _c_float), ('max_norm', _c_float), ('lr_slots', ctypes.c_void_p),
                   ('step_counter', ctypes.c_void_p)]
                + [(n, _c_double) for n in ('beta1', 'beta2', 'eps', 'weight_decay')]
                + [('schedule_kind', _c_int), ('kl_or_null', ctypes.c_void_p), ('kl_scale', _c_float)]
                + [(n, _c_double) for n in ('kl_threshold', 'min_lr', 'max_lr', 'lr_multiplier')]
                + [('stats_out_or_null', ctypes.c_void_p), ('skip_flag_or_null', ctypes.c_void_p)])


class ChainNet(ctypes.Structure):
    """rlg_chain_net (include/rlg_hip.h): the network of the six launching chain entries, stated once per chain."""
    _fields_ = [('num_layers', _c_int)] + [(n, _P) for n in ('weights', 'biases', 'in_features', 'out_features', 'acts')]


class ChainFwd(ctypes.Structure):
    """rlg_chain_fwd: the forward half of a chain launch."""
    _fields_ = ([('act_out', _P), ('act_ld', _P), ('x', _P), ('ldx', _c_ll), ('rms_mean_or_null', _P), ('rms_var', _P),
                 ('rms_eps', _c_float), ('xn_out_or_null', _P)]
                + [(n, _P) for n in ('rms_batch_or_null', 'rms_count', 'rms_mean_out', 'rms_var_out', 'rms_count_out',
                                     'weight_form_or_null', 'pack_backward_planes_or_null')])


class ChainBwd(ctypes.Structure):
    """rlg_chain_bwd: the backward half of a chain launch."""
    _fields_ = [('act_in', _P), ('act_ld', _P), ('d_out', _P), ('ld_dout', _c_ll), ('dz_out', _P), ('dz_ld', _P),
                ('bias_partials_or_null', _P), ('ppo_loss_or_null', _P), ('weight_form_or_null', _P),
                ('maxima_or_null', _P), ('maxima_stride', _c_int), ('maxima_rows_out_or_null', _P)]


class ChainLaunch(ctypes.Structure):
    """rlg_chain_launch: rows, groups and the HIP events on this dispatch."""
    _fields_ = [('rows', _c_ll), ('groups', _c_int), ('ev_start_or_null', _P), ('ev_stop_or_null', _P)]


class MlpDwDesc(ctypes.Structure):
    """rlg_mlp_dw_desc: one weight-gradient launch (rlg_mlp_dw_launch / rlg_mlp_dw_launch_form)."""
    _fields_ = ([('num_layers', _c_int), ('rows', _c_int)]
                + [(n, _P) for n in ('dz', 'x', 'partial', 'grad', 'out_features', 'in_features', 'plans4')]
                + [('num_colsums', _c_int)]
                + [(n, _P) for n in ('colsum_partials', 'colsum_blocks', 'colsum_cols', 'colsum_out',
                                     'loss_finalize_or_null', 'norm_partials_or_null')]
                + [('grad_scale', _c_float), ('step_counter_or_null', _P), ('finalize_blocks_out_or_null', _P),
                   ('maxima_or_null', _P), ('maxima_stride', _c_int), ('maxima_rows_per_entry', _c_int),
                   ('dz_slot', _P), ('x_scale', _P)])


class LstmFwd(ctypes.Structure):
    """rlg_lstm_fwd: one problem of rlg_lstm_seq_forward."""
    _fields_ = [(n, _P) for n in ('gates', 'w_hh', 'h0', 'c0', 'dones', 'out', 'c_all', 'hprev', 'hT', 'cT')]


class LstmBwd(ctypes.Structure):
    """rlg_lstm_bwd: one problem of rlg_lstm_seq_backward."""
    _fields_ = [(n, _P) for n in ('gates', 'c_all', 'c0', 'dones', 'w_hh', 'd_out', 'd_gates')]


class GruFwd(ctypes.Structure):
    """rlg_gru_fwd: one problem of rlg_gru_seq_forward."""
    _fields_ = [(n, _P) for n in ('gates', 'w_hh', 'b_hh', 'h0', 'dones', 'out', 'hn_all', 'hprev', 'hT')]


class GruBwd(ctypes.Structure):
    """rlg_gru_bwd: one problem of rlg_gru_seq_backward."""
    _fields_ = [(n, _P) for n in ('gates', 'hn_all', 'hprev', 'dones', 'w_hh', 'd_out', 'd_gx', 'd_gh')]


def check(err, what):
    if err != 0:
        raise HipLibraryError(f'{what} failed with hipError_t {err}')


def ptr(t):
    """Device address of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_handle(device=None):
    """hipStream_t of torch's current stream, as an integer address."""
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(t, what):
    if not t.is_cuda:
        raise HipLibraryError(
            f'{what}: tensor lives on {t.device}; the rl_games_amd hot path only runs on an '
            f'MI355X (HIP) device and has no CPU fallback')
