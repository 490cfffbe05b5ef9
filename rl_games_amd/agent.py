"""A2CAgent: the rl_games continuous-PPO agent with the per-epoch hot path on MI355X kernels.

Drop-in for `rl_games.algos_torch.a2c_continuous.A2CAgent` (rl_games/algos_torch/
a2c_continuous.py:12-257) and its bases `ContinuousA2CBase` / `A2CBase`
(rl_games/common/a2c_common.py:168-1202, :1482-1782) behind the same plugin seam:

    runner.algo_factory.register_builder('a2c_continuous', lambda **kw: A2CAgent(**kw))
    agent = A2CAgent(base_name='run', params=params);  agent.train()

Same constructor (`base_name`, `params` dict with the reference's config keys), same public
methods and attributes: init_tensors, env_reset, play_steps, play_steps_rnn,
prepare_dataset, dataset[i], train_actor_critic, calc_gradients, train_epoch, train,
get_action_values, get_values, update_lr, save/restore, get/set_weights, get/set_param,
experience_buffer.tensor_dict, game_rewards/game_lengths, value_mean_std, ...

What runs where (per epoch):
  rollout   : model forward on rocBLAS/hipBLASLt via torch; every buffer write of a step is ONE
              launch (csrc/experience.hip); reward shaping, time-out bootstrap, episode
              accumulators and meters are one launch per step + one per rollout, with no host
              sync (the reference syncs twice per step: a2c_common.py:1039, algo_observer.py:42)
  GAE       : one launch -> returns, advantages, fp64 moments (csrc/gae.hip)
  dataset   : 2 launches (statistics, normalise); swap_and_flatten01 is a view
  minibatch : obs normaliser 3 launches, fused loss fwd+bwd+KL 2 launches, clip+Adam+adaptive-lr
              2 launches, one all-reduce; learning rate and KL stay on the device.
"""
import os
import time
from datetime import datetime

import numpy as np
import torch
from torch import nn

from . import distributed as rdist
from . import ops, range_guard
from .actor_paths import AutogradPath, Plan
from .diagnostics import DefaultDiagnostics, PpoDiagnostics
from .flat_optim import FlatAdam
from .gae import compute_gae, gae_returns_advantages
from .hip_graphs import GraphCaptureError, GraphCapturer, StepGraphs, UpdateGraphs
from .lr_control import AdaptiveScheduler, IdentityScheduler, LinearScheduler
from .minibatch import PPODataset
from .normalizers import GeneralizedMovingStats
from .policy import PolicyBuilder
from .rollout_buffer import ExperienceBuffer
from .weight_forms import ChainFormSet


def swap_and_flatten01(arr):
    """[H, N, ...] -> [N*H, ...], flat index env*H + t (a2c_common.py:33-40).  On the env-major
    buffer views this is a zero-copy reshape."""
    if arr is None:
        return arr
    s = arr.size()
    return arr.transpose(0, 1).reshape(s[0] * s[1], *s[2:])


def rescale_actions(low, high, action):
    d = (high - low) / 2.0
    m = (high + low) / 2.0
    return action * d + m


class NullObserver:
    """AlgoObserver interface (rl_games/common/algo_observer.py:6-26) with no-op hooks."""

    def before_init(self, base_name, config, experiment_name):
        pass

    def after_init(self, algo):
        pass

    def process_infos(self, infos, done_indices):
        pass

    def after_steps(self):
        pass

    def after_clear_stats(self):
        pass

    def after_print_stats(self, frame, epoch_num, total_time):
        pass


class NullWriter:
    def add_scalar(self, *args, **kwargs):
        pass

    def flush(self):
        pass


def _make_writer(summaries_dir):
    try:
        from tensorboardX import SummaryWriter  # optional, like the reference (a2c_common.py:21)
        return SummaryWriter(summaries_dir)
    except Exception:
        return NullWriter()


class DeviceAverageMeter:
    """AverageMeter (rl_games/algos_torch/torch_ext.py:326-352) whose running mean and size
    live on the device and are updated by rlg_episode_meters_update; host reads are lazy."""

    def __init__(self, in_shape, max_size, device, sizes, slot):
        self.max_size = max_size
        self.mean = torch.zeros(in_shape, dtype=torch.float32, device=device)
        self._sizes = sizes
        self._slot = slot

    @property
    def current_size(self):
        return int(self._sizes[self._slot].item())

    def __len__(self):
        return self.current_size

    def clear(self):
        self._sizes[self._slot] = 0
        self.mean.fill_(0)

    def get_mean(self):
        return self.mean.squeeze(0).cpu().numpy()

    def update(self, values):
        size = values.size()[0]
        if size == 0:
            return
        new_mean = torch.mean(values.float(), dim=0)
        size = int(np.clip(size, 0, self.max_size))
        old_size = min(self.max_size - size, self.current_size)
        size_sum = old_size + size
        self._sizes[self._slot] = size_sum
        self.mean = (self.mean * old_size + new_mean * size) / size_sum


class A2CAgent:
    def __init__(self, base_name, params):
        self.config = config = params['config']
        self.params = params
        self.name = base_name
        full_name = config.get('full_experiment_name', None)
        self.experiment_name = full_name or (config['name'] + datetime.now().strftime('_%d-%H-%M-%S'))
        features = config.get('features') or {}
        self.algo_observer = features.get('observer') or NullObserver()
        self.algo_observer.before_init(base_name, config, self.experiment_name)
        self.network = config['network'] = PolicyBuilder(params)          # load_networks :516-525
        self.central_value_config = config.get('central_value_config', None)

        # ---- ranks / device (a2c_common.py:193-220) ----
        self.multi_gpu = config.get('multi_gpu', False)
        self.multi_gpu_sync_stats = config.get('multi_gpu_sync_stats', True)
        self.multi_gpu_sync_stats_mode = rdist.resolve_stats_sync_mode(
            config.get('multi_gpu_sync_stats_mode', 'pooled'))
        # once per epoch: do all ranks hold the same parameter / Adam-moment bits?  'raise' (default) | 'rebroadcast'
        # (rank 0's optimiser state wins, a warning is printed) | False
        self.multi_gpu_param_check = config.get('multi_gpu_param_check', 'raise')
        if self.multi_gpu_param_check not in ('raise', 'rebroadcast', False, None):
            raise ValueError("multi_gpu_param_check must be 'raise', 'rebroadcast' or False")
        # range guard of the split-fp16 products (range_guard.py): split_range 'warn' | 'raise' | 'exact', chain_products
        # 'auto' | 'exact'.  `chain_products` is also the mode the agent is on NOW ('exact' after a trip under 'exact').
        self.split_range, self.chain_products = range_guard.policy_from_config(config)
        self.local_rank = self.global_rank = 0
        self.world_size = 1
        if self.multi_gpu:
            self.local_rank, self.global_rank, self.world_size = rdist.env_ranks()
            dev_index = rdist.local_device_index(self.local_rank)
            config['device'] = 'cuda:' + str(dev_index)
            torch.cuda.set_device(dev_index)
            rdist.init_process_group(True)
            if self.global_rank != 0:
                config['print_stats'] = False
        self.ppo_device = config.get('device', 'cuda:0')
        if config.get('gemm_tuning', True):
            from . import gemm_tuning
            gemm_tuning.enable(allow_tuning=bool(config.get('gemm_tuning_online', False)))
        if not str(self.ppo_device).startswith('cuda'):
            raise RuntimeError(f"rl_games_amd.A2CAgent runs on an MI355X HIP device only, got device "
                               f"'{self.ppo_device}' (there is no CPU fallback)")

        # ---- environment (a2c_common.py:228-241) ----
        self.env_config = config.get('env_config', {})
        self.num_actors = config['num_actors']
        self.env_name = config.get('env_name', 'synthetic')
        self.env_info = config.get('env_info')
        self.vec_env = config.get('vec_env', None)
        if self.env_info is None:
            if self.vec_env is None:
                from .synthetic_env import SyntheticTensorEnv
                self.vec_env = SyntheticTensorEnv(self.num_actors, device=self.ppo_device, **self.env_config)
            self.env_info = self.vec_env.get_env_info()
        self.value_size = self.env_info.get('value_size', 1)
        self.observation_space = self.env_info['observation_space']
        self.num_agents = self.env_info.get('agents', 1)
        self.weight_decay = config.get('weight_decay', 0.0)
        self.has_central_value = self.central_value_config is not None
        if self.has_central_value:                                   # a2c_common.py:254-266
            self.state_space = self.env_info.get('state_space', None)
            if self.state_space is None:
                self.state_space = self.observation_space
                self.env_info['state_space'] = self.state_space
            if type(self.state_space).__name__ == 'Dict':
                raise NotImplementedError('dict state spaces are not implemented on the MI355X hot path')
            self.state_shape = self.state_space.shape
        self.use_action_masks = bool(config.get('use_action_masks', False))
        if self.use_action_masks and not self._supports_action_masks():
            raise NotImplementedError('action masks are not implemented for continuous actions')
        self.is_train = config.get('is_train', True)

        self.save_freq = config.get('save_frequency', 0)
        self.save_best_after = config.get('save_best_after', 100)
        self.print_stats = config.get('print_stats', True)
        self.epochs_between_resets = config.get('epochs_between_resets', 0)
        self.rnn_states = None
        self.ppo = config.get('ppo', True)      # False: a_loss = neglogp * advantage (common_losses.py:59, 80) - surrogate kind 2
        self.max_epochs = config.get('max_epochs', -1)
        self.max_frames = max(config.get('max_frames', -1), config.get('max_steps', -1))
        self.stop_fn = config.get('stop_fn', None)
        if self.stop_fn is not None and not callable(self.stop_fn):
            raise ValueError(f"'stop_fn' must be callable, got {type(self.stop_fn).__name__}")

        # ---- lr schedule (a2c_common.py:286-332) ----
        lr_schedule = config.get('lr_schedule')
        self.is_adaptive_lr = lr_schedule == 'adaptive'
        self.linear_lr = lr_schedule == 'linear'
        self.schedule_type = config.get('schedule_type', 'per_minibatch')
        if self.schedule_type == 'legacy':
            self.schedule_type = 'per_minibatch'
        if self.is_adaptive_lr:
            self.kl_threshold = config['kl_threshold']
            self.scheduler = AdaptiveScheduler(self.kl_threshold, min_lr=config.get('min_lr', 1e-6),
                                               max_lr=config.get('max_lr', 1e-2),
                                               lr_multiplier=config.get('lr_multiplier', 1.5))
        elif self.linear_lr:
            if self.max_epochs == -1 and self.max_frames == -1:
                self.scheduler = IdentityScheduler()
            else:
                use_epochs = self.max_epochs != -1
                self.scheduler = LinearScheduler(
                    float(config['learning_rate']), min_lr=config.get('min_lr', 1e-6),
                    max_steps=self.max_epochs if use_epochs else self.max_frames, use_epochs=use_epochs,
                    apply_to_entropy=config.get('schedule_entropy', False),
                    start_entropy_coef=config.get('entropy_coef'))
        else:
            self.scheduler = IdentityScheduler()

        self.e_clip = config['e_clip']
        self.clip_value = config['clip_value']
        self.rewards_shaper = config.get('reward_shaper', {})
        self.autoreset_mode = (self.env_info or {}).get('autoreset_mode', 'same_step')
        self.mask_autoreset_rows = self.autoreset_mode == 'next_step'
        self._autoreset_prev_dones = None
        if self.mask_autoreset_rows and self.num_agents > 1:
            raise ValueError('PPO next_step autoreset masking does not support multi-agent envs; '
                             'wrap the env with a same_step autoreset adapter instead')
        self.horizon_length = config['horizon_length']
        self.seq_length = config.get('seq_length', 4)
        self.bptt_len = config.get('bptt_length', self.seq_length)
        self.zero_rnn_on_done = config.get('zero_rnn_on_done', True)
        self.normalize_advantage = config['normalize_advantage']
        self.normalize_rms_advantage = config.get('normalize_rms_advantage', False)
        # a2c_common.py:222-227: the PPO health curves, collected on rank 0 only
        self.use_diagnostics = config.get('use_diagnostics', False)
        self.diagnostics = PpoDiagnostics() if self.use_diagnostics and self.global_rank == 0 else DefaultDiagnostics()
        self._diag_slot = None
        self.normalize_input = config['normalize_input']
        self.normalize_value = config.get('normalize_value', False)
        self.truncate_grads = config.get('truncate_grads', False)
        if type(self.observation_space).__name__ == 'Dict':
            raise NotImplementedError('dict observations are not implemented on the MI355X hot path')
        self.obs_shape = self.observation_space.shape
        self.critic_coef = config['critic_coef']
        self.grad_norm = config['grad_norm']
        self.gamma = config['gamma']
        self.tau = config['tau']
        self.games_to_track = config.get('games_to_track', 100)

        self.batch_size = self.horizon_length * self.num_actors * self.num_agents
        self.batch_size_envs = self.horizon_length * self.num_actors
        if 'minibatch_size' not in config and 'minibatch_size_per_env' not in config:
            raise ValueError("Configuration must include either 'minibatch_size' or 'minibatch_size_per_env'. "
                             'Neither was found in the provided config.')
        self.minibatch_size_per_env = config.get('minibatch_size_per_env', 0)
        self.minibatch_size = config.get('minibatch_size', self.num_actors * self.minibatch_size_per_env)
        if self.minibatch_size <= 0:
            raise ValueError(f"'minibatch_size' must be greater than 0. Calculated value: {self.minibatch_size}.")
        self.games_num = self.minibatch_size // self.seq_length
        self.num_minibatches = self.batch_size // self.minibatch_size
        if self.batch_size % self.minibatch_size != 0:
            raise ValueError(f"'batch_size' ({self.batch_size}) must be divisible by 'minibatch_size' "
                             f'({self.minibatch_size}).')
        self.mini_epochs_num = config['mini_epochs']
        self.mixed_precision = False
        if config.get('mixed_precision', False):
            print('rl_games_amd: mixed_precision requested - this path computes in fp32 (parity); ignoring')
        self.last_lr = float(config['learning_rate'])
        self.frame = 0
        self.update_time = 0
        self.mean_rewards = self.last_mean_rewards = -float('inf')
        self.play_time = 0
        self.epoch_num = 0
        self.curr_frames = 0
        self.train_dir = config.get('train_dir', 'runs')
        self.experiment_dir = os.path.join(self.train_dir, self.experiment_name)
        self.nn_dir = os.path.join(self.experiment_dir, 'nn')
        self.summaries_dir = os.path.join(self.experiment_dir, 'summaries')
        self._dirs_made = False
        self.entropy_coef = config['entropy_coef']
        self.writer = None
        self.value_bootstrap = config.get('value_bootstrap', True)
        self.use_smooth_clamp = config.get('use_smooth_clamp', False)
        # which actor loss the kernels evaluate (ops.SURROGATE_*): clipped PPO / smooth clamp / none (ppo: False)
        self.surrogate = 2 if not self.ppo else (1 if self.use_smooth_clamp else 0)
        self.is_tensor_obses = False
        self.aux_loss_dict = {}

        self._init_action_space(config)
        dev = self.ppo_device

        # ---- A2CAgent.__init__ (a2c_continuous.py:18-76) ----
        build_config = {
            'actions_num': self.actions_num, 'input_shape': self.obs_shape,
            'num_seqs': self.num_actors * self.num_agents, 'value_size': self.value_size,
            'normalize_value': self.normalize_value, 'normalize_input': self.normalize_input,
        }
        self.model = self.network.build(build_config)
        self.model.to(dev)
        self.states = None
        self.is_rnn = self.model.is_rnn()
        self.bound_loss_type = config.get('bound_loss_type', 'bound')
        # which engine runs the network (actor_paths.py): planned in front of the optimiser, whose arena
        # takes the path's layout, built behind it
        plan = Plan(self, config)
        self.optimizer = FlatAdam(self.model.parameters(), self.last_lr, eps=1e-08,
                                  weight_decay=self.weight_decay, layout=plan.layout)
        self._path = plan.build(self)
        # where a step or a minibatch goes whose observations the path does not take (takes())
        self._autograd = self._path if type(self._path) is AutogradPath else AutogradPath(self)
        self.dataset = PPODataset(self.batch_size, self.minibatch_size, self.is_discrete, self.is_rnn,
                                  dev, self.seq_length)
        self.central_value_net = None
        if self.has_central_value:                                   # a2c_continuous.py:44-66
            from .central_value import CentralValueTrain
            cv_cfg = self.central_value_config
            cv_builder = PolicyBuilder({'model': cv_cfg.get('model', {'name': 'central_value'}),
                                        'network': cv_cfg['network']})
            self.central_value_net = CentralValueTrain(
                state_shape=self.state_shape, value_size=self.value_size, ppo_device=dev,
                num_agents=self.num_agents, horizon_length=self.horizon_length, num_actors=self.num_actors,
                num_actions=self.actions_num, seq_length=self.seq_length, normalize_value=self.normalize_value,
                network=cv_builder, config=cv_cfg, writter=self.writer, max_epochs=self.max_epochs,
                multi_gpu=self.multi_gpu, zero_rnn_on_done=self.zero_rnn_on_done)
            if not self.is_rnn:
                # the reference advances a recurrent critic with the rollout only in play_steps_rnn (a2c_common.py:1085-1086)
                self.central_value_net.decline_rnn_engine('the actor is not recurrent')
        # (the reference's defaults: True for the continuous agent, a2c_continuous.py:70; False for the discrete one,
        #  a2c_discrete.py:72 - its actor trains no value loss next to a central value network unless asked to)
        self.use_experimental_cv = config.get('use_experimental_cv', not self.is_discrete)
        if self.normalize_value:
            self.value_mean_std = (self.central_value_net.model.value_mean_std if self.has_central_value
                                   else self.model.value_mean_std)
        if self.normalize_advantage and self.normalize_rms_advantage:
            momentum = config.get('adv_rms_momentum', 0.5)
            self.advantage_mean_std = GeneralizedMovingStats((1,), decay=momentum).to(dev)
        self.has_value_loss = self.use_experimental_cv or not self.has_central_value
        self._fused_rollout = self._fused_rollout_eligible()      # (with the critic in place)
        self._form_chains = forms = ChainFormSet(self._graph_chains())
        self._lean_chain, self._adam_pack_chain = forms.lean_chain, forms.adam_pack_chain

        # device-side episode meters (game_rewards / game_shaped_rewards / game_lengths)
        self._meter_sizes = torch.zeros(3, dtype=torch.int32, device=dev)
        self._finished_total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.game_rewards = DeviceAverageMeter(self.value_size, self.games_to_track, dev, self._meter_sizes, 0)
        self.game_shaped_rewards = DeviceAverageMeter(self.value_size, self.games_to_track, dev,
                                                      self._meter_sizes, 1)
        self.game_lengths = DeviceAverageMeter(1, self.games_to_track, dev, self._meter_sizes, 2)
        self.obs = None

        # per-minibatch scratch
        mb = self.minibatch_size
        self._alloc_loss_scratch(mb, dev)
        self._mb_scalars = torch.zeros(max(1, self.mini_epochs_num * self.num_minibatches), 8,
                                       dtype=torch.float32, device=dev)
        self._mb_index = 0
        self._prep_stats = ops.prepare_stats_buffer(dev)
        self._host_lr = self.last_lr
        self.train_result = None
        self.kernel_timers = None
        # HIP graphs (hip_graphs.py): the update graphs and the rollout's step graphs, captured into one pool; the
        # first epoch always runs eagerly (allocations, GEMM selection).
        self._hip_graphs = bool(config.get('hip_graphs', True))
        self._capturer = GraphCapturer(forms, self.optimizer)
        self._update_graphs = UpdateGraphs()
        self._rollout_graphs, self._rollout_graph_key = StepGraphs(self._capturer), None
        self.last_allreduce = None    # 'ipc' | 'rccl' once a multi-GPU step has run (bench.py reports it)
        self._graph_failed = False
        self._fold_ready = False      # this epoch's minibatch observation moments are precomputed
        self._norm_ready = None       # (partials, count) when the finalise / all-reduce launch produced the gradient norm
        self._roll_env_actions = None
        self._ar_norm_partials = None
        self._fold_index = None
        self._ipc_comm = None
        self._rnn_state_store = None
        self._eager_epochs = 0
        self._graph_rows = torch.zeros(max(1, self.num_minibatches), 8, dtype=torch.float32, device=dev)
        if isinstance(self.diagnostics, PpoDiagnostics):
            # the device table every minibatch launch writes its row of (captured graphs included): allocated here
            self.diagnostics.allocate(self.mini_epochs_num, max(1, self.num_minibatches), self.minibatch_size, dev,
                                     value_size=self.value_size)
        self._obs_norm_mb = (torch.empty((mb,) + tuple(self.obs_shape), dtype=torch.float32, device=dev)
                             if self.normalize_input else None)
        self._arm_range_guard()
        self.algo_observer.after_init(self)

    def _init_action_space(self, config):
        """ContinuousA2CBase.__init__ (a2c_common.py:1484-1498)."""
        self.is_discrete = False
        action_space = self.env_info['action_space']
        if type(action_space).__name__ != 'Box':
            raise ValueError(f'A2CAgent (a2c_continuous) needs a Box action space, got '
                             f'{type(action_space).__name__}; use DiscreteA2CAgent for a2c_discrete')
        self.actions_num = action_space.shape[0]
        self.bounds_loss_coef = config.get('bounds_loss_coef', None)
        self.clip_actions = config.get('clip_actions', True)
        dev = self.ppo_device
        self.actions_low = torch.from_numpy(np.asarray(action_space.low).copy()).float().to(dev)
        self.actions_high = torch.from_numpy(np.asarray(action_space.high).copy()).float().to(dev)

    # the engines of the chosen path under the names tests, tools and bench.py read (None where the path is another one)
    _engine = property(lambda self: self._path.engine)
    _rnn_pair = property(lambda self: self._path.pair)
    _chains = property(lambda self: self._path.chains)
    _rnn_engine = property(lambda self: self._path.recurrent)
    _fin_norm_ok = property(lambda self: self._path.norm_ok)

    def _alloc_loss_scratch(self, mb, dev):
        A = self.actions_num
        self._d_policy = torch.empty(mb, A, dtype=torch.float32, device=dev)
        self._d_val = torch.empty(mb, dtype=torch.float32, device=dev)
        self._loss_blocks = ops.ppo_loss_blocks(mb)
        # (a fused backward launch leaves one row per 16 / 32 / 64-row workgroup)
        self._loss_partials = torch.empty(max(self._loss_blocks, (mb + 15) // 16),
                                          ops.ppo_loss_partials_per_block(A), dtype=torch.float64, device=dev)

    def _rollout_fields(self):
        return ['actions', 'neglogpacs', 'values', 'mus', 'sigmas']

    def _supports_action_masks(self):
        return False

    # ================================================================== small helpers
    @property
    def device(self):
        return self.ppo_device

    def _ensure_dirs(self):
        if not self._dirs_made:
            for d in (self.train_dir, self.experiment_dir, self.nn_dir, self.summaries_dir):
                os.makedirs(d, exist_ok=True)
            if self.global_rank == 0:
                self.writer = _make_writer(self.summaries_dir)
            self._dirs_made = True

    def _shaper_params(self):
        s = self.rewards_shaper
        get = (lambda k, d: s.get(k, d)) if isinstance(s, dict) else (lambda k, d: getattr(s, k, d))
        return (float(get('shift_value', 0)), float(get('scale_value', 1)),
                float(get('min_val', -np.inf)), float(get('max_val', np.inf)), bool(get('log_val', False)))

    def _uses_observer_infos(self):
        fn = getattr(type(self.algo_observer), 'process_infos', None)
        return fn is not None and fn is not NullObserver.process_infos and \
            getattr(fn, '__qualname__', '').split('.')[0] != 'AlgoObserver'

    def update_epoch(self):
        self.epoch_num += 1
        return self.epoch_num

    def set_eval(self):
        self.model.eval()
        if self.normalize_rms_advantage:
            self.advantage_mean_std.eval()
        if self.epochs_between_resets > 0 and self.epoch_num % self.epochs_between_resets == 0:
            self.reset_envs()
            rows = self.num_agents * self.num_actors
            self.init_current_rewards(rows, (rows, self.value_size))

    def set_train(self):
        self.model.train()
        if self.normalize_rms_advantage:
            self.advantage_mean_std.train()

    def update_lr(self, lr):
        """a2c_common.py:564-576.  The per-minibatch adaptive schedule never calls this (the lr
        moves on the device); host-driven schedules and user code do."""
        self.last_lr = lr
        self._host_lr = lr
        self.optimizer.set_lr(lr)

    def _sync_lr_to_host(self):
        self.last_lr = self.optimizer.current_lr()
        return self.last_lr

    # ================================================================== model queries
    def _preproc_obs(self, obs_batch):
        if obs_batch.dtype == torch.uint8:
            obs_batch = obs_batch.float() / 255.0
        return obs_batch

    def _eval_batch(self, obs, **more):
        """The input of the model's eval forward on the current RNN states."""
        return dict(is_train=False, prev_actions=None, obs=self._preproc_obs(obs['obs']), rnn_states=self.rnn_states, **more)

    def get_action_values(self, obs):
        self.model.eval()
        with torch.no_grad():
            res_dict = self.model(self._eval_batch(obs))
            if self.has_central_value:                               # a2c_common.py:593-600
                res_dict['values'] = self.get_central_value({'is_train': False, 'states': obs['states']})
        return res_dict

    def get_central_value(self, obs_dict):
        return self.central_value_net.get_value(obs_dict)

    def train_central_value(self):
        return self.central_value_net.train_net()

    def get_values(self, obs):
        with torch.no_grad():
            if self.has_central_value:                               # a2c_common.py:605-614
                self.central_value_net.eval()
                return self.get_central_value({'is_train': False, 'states': obs['states'], 'actions': None,
                                               'is_done': self.dones})
            self.model.eval()
            return self.model(self._eval_batch(obs))['values']

    def get_masked_action_values(self, obs, action_masks):
        raise NotImplementedError('Masked action values are not implemented for continuous actions')

    # ================================================================== env plumbing
    def cast_obs(self, obs):
        if isinstance(obs, torch.Tensor):
            self.is_tensor_obses = True
            if obs.device != torch.device(self.ppo_device):
                obs = obs.to(self.ppo_device)
        elif isinstance(obs, np.ndarray):
            assert obs.dtype != np.int8
            if obs.dtype == np.uint8:
                obs = torch.from_numpy(obs).to(self.ppo_device)
            else:
                obs = torch.from_numpy(obs).float().to(self.ppo_device)
        return obs

    def obs_to_tensors(self, obs):
        if isinstance(obs, dict):
            upd = {k: self.cast_obs(v) for k, v in obs.items()}
            return upd if 'obs' in obs else {'obs': upd}
        return {'obs': self.cast_obs(obs)}

    def preprocess_actions(self, actions):
        if self.clip_actions:
            clamped = torch.clamp(actions, -1.0, 1.0)
            rescaled = rescale_actions(self.actions_low, self.actions_high, clamped)
        else:
            rescaled = actions
        if not self.is_tensor_obses:
            rescaled = rescaled.cpu().numpy()
        return rescaled

    def env_step(self, actions, preprocessed=None):
        """`preprocessed`: device tensor already clamped/rescaled by the fused rollout step."""
        if preprocessed is None:
            actions = self.preprocess_actions(actions)
        else:
            actions = preprocessed if self.is_tensor_obses else preprocessed.cpu().numpy()
        obs, rewards, dones, infos = self.vec_env.step(actions)
        dev = self.ppo_device
        if not isinstance(rewards, torch.Tensor):
            rewards = torch.from_numpy(np.asarray(rewards)).to(dev, dtype=torch.float32)
            dones = torch.from_numpy(np.asarray(dones)).to(dev)
        else:
            rewards, dones = rewards.to(dev), dones.to(dev)
        if self.value_size == 1 and rewards.dim() == 1:
            rewards = rewards.unsqueeze(1)
        return self.obs_to_tensors(obs), rewards, dones, infos

    def env_reset(self):
        obs = self.vec_env.reset()
        obs = self.obs_to_tensors(obs)
        self._autoreset_prev_dones = None
        return obs

    def reset_envs(self):
        if self.is_rnn:
            self.rnn_states = [s.to(self.ppo_device) for s in self.model.get_default_rnn_state()]
        self.obs = self.env_reset()

    # ================================================================== buffers
    def init_tensors(self):
        rows = self.num_agents * self.num_actors
        algo_info = {'num_actors': self.num_actors, 'horizon_length': self.horizon_length,
                     'has_central_value': self.has_central_value, 'use_action_masks': self.use_action_masks}
        self.experience_buffer = ExperienceBuffer(self.env_info, algo_info, self.ppo_device)
        self.init_current_rewards(rows, (rows, self.value_size))
        dev = self.ppo_device
        self._post_blocks = ops.post_step_num_blocks(rows)
        self._ep_partials = torch.zeros(self.horizon_length, self._post_blocks, 2 * self.value_size + 2,
                                        dtype=torch.float64, device=dev)
        B = self.batch_size
        self._returns = torch.empty(rows, self.horizon_length, dtype=torch.float32, device=dev)
        self._advantages = torch.empty(rows, self.horizon_length, dtype=torch.float32, device=dev)
        self._norm_values = torch.empty(B, 1, dtype=torch.float32, device=dev)
        self._norm_returns = torch.empty(B, 1, dtype=torch.float32, device=dev)
        self._norm_advantages = torch.empty(B, dtype=torch.float32, device=dev)
        from .gae import num_moment_partials
        self._gae_partials = torch.empty(num_moment_partials(rows), 6, dtype=torch.float64, device=dev)
        self.update_list = self._rollout_fields()
        self.tensor_list = self.update_list + ['obses', 'states', 'dones']
        if self._fast_rollout_ok():
            self._alloc_rollout_scratch(rows, dev)
            if self.has_central_value:
                self.central_value_net.reserve_rollout()
        if self.is_rnn:
            self.rnn_states = [s.to(dev) for s in self.model.get_default_rnn_state()]
            num_seqs = self.horizon_length // self.seq_length
            if (self.horizon_length * rows // self.num_minibatches) % self.seq_length != 0:
                raise ValueError(f'Horizon length ({self.horizon_length}) times total agents ({rows}) divided by '
                                 f'num minibatches ({self.num_minibatches}) must be divisible by sequence '
                                 f'length ({self.seq_length})')
            self.mb_rnn_states = [torch.zeros((num_seqs, s.size()[0], rows, s.size()[2]),
                                              dtype=torch.float32, device=dev) for s in self.rnn_states]

    def _alloc_rollout_scratch(self, rows, dev):
        self._roll_obs_norm = torch.empty((rows,) + tuple(self.obs_shape), dtype=torch.float32, device=dev)
        self._roll_noise = torch.empty(rows, self.actions_num, dtype=torch.float32, device=dev)
        self._roll_actions = torch.empty(rows, self.actions_num, dtype=torch.float32, device=dev)
        self._roll_values = torch.empty(rows, dtype=torch.float32, device=dev)

    def init_current_rewards(self, batch_size, current_rewards_shape):
        dev = self.ppo_device
        self.current_rewards = torch.zeros(current_rewards_shape, dtype=torch.float32, device=dev)
        self.current_shaped_rewards = torch.zeros(current_rewards_shape, dtype=torch.float32, device=dev)
        self.current_lengths = torch.zeros(batch_size, dtype=torch.float32, device=dev)
        self.dones = torch.ones((batch_size,), dtype=torch.uint8, device=dev)

    def discount_values(self, fdones, last_extrinsic_values, mb_fdones, mb_extrinsic_values, mb_rewards):
        """a2c_common.py:729-734 (function seam kept for subclasses)."""
        return compute_gae(mb_rewards, mb_extrinsic_values, mb_fdones, last_extrinsic_values, fdones,
                           self.gamma, self.tau)

    def clear_stats(self, clean_rewards=True):
        self.game_rewards.clear()
        self.game_shaped_rewards.clear()
        self.game_lengths.clear()
        if clean_rewards:
            self.mean_rewards = self.last_mean_rewards = -float('inf')
        self.algo_observer.after_clear_stats()

    # ================================================================== rollout
    def _as_u8(self, dones):
        if dones.dtype == torch.uint8:
            return dones
        if dones.dtype == torch.bool:
            return dones.view(torch.uint8)
        return (dones != 0).to(torch.uint8)

    def _rollout_step_tail(self, n, res_dict, rewards, infos, mb_valid):
        """Everything after vec_env.step for step n (a2c_common.py:1021-1051)."""
        buf = self.experience_buffer
        time_outs = None
        if self.value_bootstrap and isinstance(infos, dict) and 'time_outs' in infos:
            time_outs = self.cast_obs(infos['time_outs'])
            if time_outs.dtype not in (torch.uint8, torch.bool, torch.float32):
                time_outs = time_outs.float()
        values = res_dict['values']
        if not values.is_contiguous():
            values = values.contiguous()
        if not rewards.is_contiguous():
            rewards = rewards.contiguous()
        live = None if mb_valid is None else mb_valid[n]
        ops.rollout_post_step(rewards.float() if rewards.dtype != torch.float32 else rewards, self.dones,
                              time_outs, values, live, buf.storage['rewards'], self.current_rewards,
                              self.current_shaped_rewards, self.current_lengths, self._ep_partials,
                              self._shaper, time_outs is not None, self.gamma, self.horizon_length, n,
                              num_agents=self.num_agents)
        if self._observer_needs_infos:
            done_indices = self.dones.nonzero(as_tuple=False)[::self.num_agents]
            self.algo_observer.process_infos(infos, done_indices)

    def _finish_rollout(self, batch_dict, mb_valid, step_time):
        buf = self.experience_buffer
        H = self.horizon_length
        rows = self.num_agents * self.num_actors
        ops.episode_meters_update(self._ep_partials, H, self._post_blocks, self.value_size,
                                  self.games_to_track, self.game_rewards.mean, self.game_shaped_rewards.mean,
                                  self.game_lengths.mean, self._meter_sizes, self._finished_total)
        if self._fast_rollout_ok():
            last_values = self._fast_values(self.obs)
        else:
            last_values = self.get_values(self.obs)
        if self.value_size == 1 and ops._lib.load().rlg_gae_envmajor_supported(H):
            lv = last_values.reshape(-1).contiguous()
            timers = self.kernel_timers
            ev = None
            if timers is not None:      # bench.py: HIP events on the launch stream around the kernel
                from .gae import HipEventPair
                ev = HipEventPair()
                timers.setdefault('gae_envmajor_fused', []).append(ev)
            gae_returns_advantages(buf.storage['rewards'].view(rows, H), buf.storage['values'].view(rows, H),
                                   buf.storage['dones'], lv, self.dones, self.gamma, self.tau,
                                   out_returns=self._returns, out_advantages=self._advantages,
                                   moment_partials=self._gae_partials, events=ev)
            batch_dict['returns'] = self._returns.view(rows * H, 1)
            batch_dict['_fused'] = {'advantages': self._advantages.view(rows * H), 'partials': self._gae_partials}
        else:
            mb_advs = self.discount_values(self.dones, last_values, buf.tensor_dict['dones'],
                                           buf.tensor_dict['values'], buf.tensor_dict['rewards'])
            batch_dict['returns'] = swap_and_flatten01(mb_advs + buf.tensor_dict['values'])
        batch_dict['played_frames'] = self.batch_size
        batch_dict['step_time'] = step_time
        if mb_valid is not None:
            batch_dict['rnn_masks'] = swap_and_flatten01(mb_valid)
        return batch_dict

    def _fast_policy_step(self, n):
        """Rollout forward of step n on the engine (see _policy_step_kernels).  From the second epoch
        on the launches of a step are replayed as one HIP graph per step index; its inputs must live at
        fixed addresses: the buffer slot of the step (plain float observations) or static copies of the
        env-owned tensors (recurrent policies, integer observations)."""
        states = self.obs['states'] if self.has_central_value else None
        if not self._rollout_graphs_usable():
            return self._policy_step_kernels(n, self.obs['obs'], self.dones, self.rnn_states, states=states)
        key = (id(self.experience_buffer), tuple(self.obs['obs'].shape), self.obs['obs'].dtype)
        if states is not None:
            key += (tuple(states.shape), states.dtype)
        buf = self.experience_buffer
        obs = self.obs['obs']
        # Plain float observations without recurrent state: the step's observations / done flags (and a central value
        # network's states) go from the env's tensors straight into the buffer (the one launch that had to happen
        # anyway) and the captured forwards read them from that buffer slot - no staging copies in front of the graph.
        direct = (not self.is_rnn and obs.dtype == torch.float32 and obs.dim() == 2 and obs.is_contiguous()
                  and torch.is_tensor(buf.storage['obses']) and self.config.get('rollout_obs_from_buffer', True)
                  and (states is None or (states.dtype == torch.float32 and states.dim() == 2
                                          and states.is_contiguous() and torch.is_tensor(buf.storage['states']))))
        if self._rollout_graph_key != key:
            self._rollout_graphs.clear()
            self._rollout_graph_key = key
        if direct:
            fields = {'obses': obs, 'dones': self.dones}
            if states is not None:
                fields['states'] = states
            buf.store_step(n, fields)
            args = (n, buf.storage['obses'][:, n, :], None, None, False,
                    None if states is None else buf.storage['states'][:, n, :])
            inputs, body = None, lambda: self._policy_step_kernels(*args)
        else:                                                    # (by the names _policy_step_kernels takes them under)
            inputs = {'obs_raw': obs, 'dones': self.dones, 'rnn_states': self.rnn_states if self.is_rnn else None,
                      'states': states,
                      'cv_rnn_states': self.central_value_net.rnn_states if self._critic_steps_rnn() else None}
            body = lambda **static: self._policy_step_kernels(n, **static)
        return self._rollout_graphs.step(direct, body, inputs, index=n)     # (one set of statics for all steps)

    def _rollout_graphs_usable(self):
        return (self._hip_graphs and self.config.get('rollout_graphs', True) and self._eager_epochs >= 1
                and not self._graph_failed and isinstance(self.obs['obs'], torch.Tensor))

    def _policy_step_kernels(self, n, obs_raw, dones, rnn_states, store=True, states=None, cv_rnn_states=None):
        """obs normalise -> the path's inference forward -> (central value: the critic's forward on `states`) -> the
        draws and the fused policy-head kernel that also writes actions / neglogpacs / values (/ mus / sigmas) of the step
        into the buffer (_sample_step) -> obs + dones (+ states) into the buffer.  Same maths and the same generator use
        as get_(masked_)action_values + update_data + preprocess_actions; no autograd, nothing that depends on the host,
        so the step can be captured.  cv_rnn_states: the states a recurrent critic's step reads (None: the critic's own
        `rnn_states`); the ones it leaves go into the result."""
        cv = self.central_value_net
        obs = self._preproc_obs(obs_raw)
        heads = self._path.infer(obs, rnn_states, logits_only=self.has_central_value)
        value = cv.infer(states, cv_rnn_states) if self.has_central_value else None
        env_actions = self._sample_step(n, heads, value)
        # the buffer keeps the observation as the env delivered it (a2c_common.py:1000), not the
        # /255-preprocessed copy
        if store:
            self._store_step_inputs(n, obs_raw, dones, states)
        res = {'actions': self._roll_actions, 'values': self._roll_values.view(obs.shape[0], 1)}
        if env_actions is not None:
            res['env_actions'] = env_actions
        if self.is_rnn:
            res['rnn_states'] = self._path.last_states
        if self._critic_steps_rnn():
            res['cv_rnn_states'] = cv.last_states
        return res

    def _sample_step(self, n, heads, value):
        """Gaussian noise, then one launch: sample, score, write the step into the buffer - and clamp + rescale for the env
        in the same launch (3 element-wise launches less per step).  Returns the actions the env takes."""
        torch.randn(self._roll_noise.shape, device=self._roll_noise.device, out=self._roll_noise)
        vs, eps = self._rollout_value_stats()
        env_actions = None
        if self.clip_actions:
            if self._roll_env_actions is None or self._roll_env_actions.shape != self._roll_actions.shape:
                self._roll_env_actions = torch.empty_like(self._roll_actions)
            env_actions = (self._roll_env_actions, self.actions_low, self.actions_high)
        ops.rollout_policy_head(heads, self.model.a2c_network.sigma.data, self._roll_noise, vs, eps,
                                self._roll_actions, self._roll_values, self.experience_buffer.storage, self.horizon_length,
                                n, env_actions=env_actions, value=value,
                                value_repeat=self.num_agents if value is not None else 1)
        return self._roll_env_actions if self.clip_actions else self._roll_actions

    def _store_step_inputs(self, n, obs_raw, dones, states):
        """update_data('obses' / 'dones' (/ 'states'), n) of a fused step (a2c_common.py:1000-1011): one launch per row
        count (a multi-agent env's states have one row per env)."""
        fields = {'obses': obs_raw if obs_raw.is_contiguous() else obs_raw.contiguous(), 'dones': dones}
        if states is not None:
            fields['states'] = states
        self.experience_buffer.store_step(n, fields)

    def _critic_chain(self):
        """The central value network's chain_net.ChainNet, or None (a name the tests read, like `_engine`)."""
        return self.central_value_net._engine if self.has_central_value else None

    def _critic_steps_rnn(self):
        """A recurrent critic on its engine: the fused step carries its states."""
        return self.has_central_value and self.central_value_net.rnn_on_engine

    def _rollout_value_stats(self):
        """(mean, var) and epsilon of the value de-normaliser of the rollout: the critic's with a central value network
        (its values replace the actor's, a2c_common.py:593-600), else the actor model's; (None, 1e-5) when off."""
        if not self.normalize_value:
            return None, 1e-5
        vm = self.central_value_net.model.value_mean_std if self.has_central_value else self.model.value_mean_std
        return (vm.running_mean, vm.running_var), vm.epsilon

    def _denorm_values(self, v):
        """Raw values [rows, 1] -> de-normalised with the rollout's statistics (_rollout_value_stats)."""
        vs, eps = self._rollout_value_stats()
        if vs is None:
            return v
        return ops.rms_apply(v.contiguous(), vs[0], vs[1], eps, 1)

    def _fast_values(self, obs):
        """get_values on the path's engine: de-normalised critic values [N] of `obs`.  With a central value network
        (a2c_common.py:605-614) the critic's forward only - the actor does not run and nothing is drawn from the
        generator - every agent of an env given the env's value (central_value.py:223-225); a recurrent critic's
        states advance with it, as CentralValueTrain.get_value leaves them (central_value.py:222)."""
        if self.has_central_value:
            cv = self.central_value_net
            v = self._denorm_values(cv.infer(obs['states']))
            if self._critic_steps_rnn():
                cv.rnn_states = list(cv.last_states)
            return v.expand(-1, self.num_agents).reshape(-1)
        if not self._path.takes(obs['obs']):
            return self.get_values(obs)
        v = self._path.values(self._preproc_obs(obs['obs']), self.rnn_states)
        self._draw_value_noise(v.shape[0])
        return self._denorm_values(v).view(-1)

    def _draw_value_noise(self, rows):
        """What get_values' eval forward draws from the generator next to the values: nothing for a Gaussian policy."""

    def _obs_rms(self):
        if not self.normalize_input:
            return None
        m = self.model.running_mean_std
        return (m.running_mean, m.running_var)

    def _obs_eps(self):
        return self.model.running_mean_std.epsilon if self.normalize_input else 1e-5

    def _fused_rollout_eligible(self):
        """The rollout on the fused forwards: one value column, no central value network or one the fused step can run
        (behind a recurrent actor, whose play_steps_rnn is where the reference advances a recurrent critic), `fused_rollout`
        on, and the path's own conditions (rollout_ok)."""
        cv_ok = not self.has_central_value or self.central_value_net.rollout_ok(self.state_space, self.is_rnn)
        return self.value_size == 1 and cv_ok and self.config.get('fused_rollout', True) and self._path.rollout_ok

    def _fast_rollout_ok(self):
        """Does the rollout run fused (decided when the agent was built)."""
        return self._fused_rollout

    def _torch_action_values(self):
        """get_(masked_)action_values of the current observations (a2c_common.py:995-997)."""
        if self.use_action_masks:
            return self.get_masked_action_values(self.obs, self.vec_env.get_action_masks())
        return self.get_action_values(self.obs)

    def _store_torch_step(self, n, res_dict):
        """update_data of a step on the torch path (a2c_common.py:1000-1011): observations, done flags, the model's
        outputs (and a central value network's states) into the buffer, one launch."""
        fields = {'obses': self.obs['obs'], 'dones': self.dones}
        for k in self.update_list:
            fields[k] = res_dict[k]
        if self.has_central_value:
            fields['states'] = self.obs['states']
        self.experience_buffer.store_step(n, fields)

    def _mark_autoreset_rows(self, mb_valid, n):
        """next_step autoreset: mb_valid[n] = 0 for the rows whose previous step ended an episode (this step's
        observation is the reset filler).  Returns those done flags."""
        prev = self._autoreset_prev_dones
        if prev is None:
            prev = torch.zeros_like(self.dones)
        mb_valid[n] = 1.0 - prev.float()
        return prev

    def play_steps(self):
        """a2c_common.py:985-1069."""
        return self._play_steps(recurrent=False)

    def play_steps_rnn(self):
        """a2c_common.py:1071-1202."""
        return self._play_steps(recurrent=True)

    def _play_steps(self, recurrent):
        """The rollout loop of both entry points.  What play_steps_rnn adds is marked `recurrent`: the state every sequence
        starts from, the new states behind the forward, their zeroing where an episode ended, and behind the loop the
        done flags of filler rows and the kept states for the dataset."""
        buf = self.experience_buffer
        self._shaper = self._shaper_params()
        self._observer_needs_infos = self._uses_observer_infos()
        step_time = 0.0
        mb_valid = None
        fast = self._fast_rollout_ok()
        if fast:
            self._form_chains.before_replay(rollout=True)
        if self.mask_autoreset_rows:
            mb_valid = torch.ones((self.horizon_length, self.num_actors * self.num_agents),
                                  dtype=torch.float32, device=self.ppo_device)
        for n in range(self.horizon_length):
            if recurrent:
                if n % self.seq_length == 0:
                    for s, mb_s in zip(self.rnn_states, self.mb_rnn_states):
                        mb_s[n // self.seq_length, :, :, :] = s
                if self.has_central_value:
                    self.central_value_net.pre_step_rnn(n)       # a2c_common.py:1085-1086
            res_dict = self._fast_policy_step(n) if fast else self._torch_action_values()
            if recurrent:
                self.rnn_states = [s.contiguous() for s in res_dict['rnn_states']]
                if res_dict.get('cv_rnn_states') is not None:    # (a fused step: get_value's update, central_value.py:222)
                    self.central_value_net.rnn_states = [s.contiguous() for s in res_dict['cv_rnn_states']]
            elif not fast:
                self._store_torch_step(n, res_dict)
            if mb_valid is not None:
                prev = self._mark_autoreset_rows(mb_valid, n)
                if recurrent:                                    # (the critic absorbed the same filler row: :1112-1115)
                    self._zero_rnn_states(prev)
            if recurrent and not fast:                           # (a recurrent step is stored behind its state upkeep)
                self._store_torch_step(n, res_dict)
            t0 = time.perf_counter()
            self.obs, rewards, dones, infos = self.env_step(res_dict['actions'], res_dict.get('env_actions'))
            self.dones = self._as_u8(dones)
            if self.mask_autoreset_rows:
                self._autoreset_prev_dones = self.dones.clone()
            step_time += time.perf_counter() - t0
            if recurrent:                                        # a2c_common.py:1151-1152
                self._zero_rnn_states(self.dones)
            self._rollout_step_tail(n, res_dict, rewards, infos, mb_valid)
        batch_dict = buf.get_transformed_list(swap_and_flatten01, self.tensor_list)
        batch_dict = self._finish_rollout(batch_dict, mb_valid, step_time)
        self._scan_rollout(batch_dict)
        if not recurrent:
            return batch_dict
        if mb_valid is not None and self.zero_rnn_on_done:
            rnn_dones = buf.tensor_dict['dones'].clone()
            garbage = (mb_valid == 0.0)
            rnn_dones[1:] = torch.maximum(rnn_dones[1:], garbage[:-1].to(rnn_dones.dtype))
            batch_dict['dones'] = swap_and_flatten01(rnn_dones)
        states = []
        for k, mb_s in enumerate(self.mb_rnn_states):
            t_size = mb_s.size()[0] * mb_s.size()[2]
            h_size = mb_s.size()[3]
            flat = mb_s.permute(1, 2, 0, 3).reshape(-1, t_size, h_size)
            if self._rnn_state_store is None or len(self._rnn_state_store) <= k:
                self._rnn_state_store = (self._rnn_state_store or []) + [torch.empty_like(flat)]
            self._rnn_state_store[k].copy_(flat)      # same storage every epoch (HIP-graph replays)
            states.append(self._rnn_state_store[k])
        batch_dict['rnn_states'] = states
        return batch_dict

    def _zero_rnn_states(self, ended):
        """`zero_rnn_on_done`: the actor's states - and a recurrent critic's - start from zero where `ended` is set."""
        if self.zero_rnn_on_done:
            for s in self.rnn_states:
                ops.rnn_zero_done_states(s, ended)
        if self.has_central_value:
            self.central_value_net.zero_states_where(ended)

    # ================================================================== dataset
    def prepare_dataset(self, batch_dict):
        """a2c_common.py:1586-1660."""
        returns = batch_dict['returns']
        values = batch_dict['values']
        rnn_masks = batch_dict.get('rnn_masks', None)
        B = returns.shape[0]
        if self.value_size != 1:
            return self._prepare_dataset_general(batch_dict)
        fused = batch_dict.get('_fused')
        values_flat = values.reshape(-1)
        returns_flat = returns.reshape(-1)
        if not values_flat.is_contiguous():
            values_flat = values_flat.contiguous()
        if not returns_flat.is_contiguous():
            returns_flat = returns_flat.contiguous()
        mask = None
        if rnn_masks is not None:
            mask = rnn_masks.reshape(-1).float().contiguous()
        if fused is not None and mask is None:
            advantages, partials = fused['advantages'], fused['partials']
        else:
            advantages = returns_flat - values_flat                                     # :1598
            partials = ops.triple_moments(advantages, values_flat, returns_flat, mask)
        flags = 0
        value_stats = None
        if self.normalize_value:
            flags |= ops.PREP_NORM_VALUE
            if self.config.get('freeze_critic', False):
                flags |= ops.PREP_FREEZE_CRITIC
            m = self.value_mean_std
            value_stats = (m.running_mean, m.running_var, m.count)
        ema = None
        if self.normalize_advantage:
            if self.normalize_rms_advantage:
                flags |= ops.PREP_EMA_ADV
                ema = self.advantage_mean_std.kernel_state()
            else:
                flags |= ops.PREP_NORM_ADV
        eps = self.value_mean_std.epsilon if self.normalize_value else 1e-5
        if B > self._norm_values.shape[0]:
            raise ValueError('batch larger than the allocated dataset buffers')
        nv, nr, na = self._norm_values[:B], self._norm_returns[:B], self._norm_advantages[:B]
        if flags:
            ops.prepare_finalize(partials, B, flags, value_stats, eps, ema, self._prep_stats)
        else:
            self._prep_stats.zero_()
        ops.prepare_apply(values_flat, returns_flat, advantages, flags, self._prep_stats,
                          out=(nv.view(-1), nr.view(-1), na))
        if self.normalize_value:
            self.value_mean_std.eval()
        self._update_datasets(batch_dict, nv, nr, na, rnn_masks)

    def _update_datasets(self, batch_dict, values, returns, advantages, rnn_masks):
        """The actor's dataset and (a2c_common.py:1651-1660) the central value network's, of the prepared tensors."""
        dataset_dict = {
            'old_values': values, 'old_logp_actions': batch_dict['neglogpacs'], 'advantages': advantages,
            'returns': returns, 'actions': batch_dict['actions'], 'obs': batch_dict['obses'],
            'dones': batch_dict['dones'], 'rnn_states': batch_dict.get('rnn_states', None),
            'rnn_masks': rnn_masks,
        }
        if not self.is_discrete:
            dataset_dict['mu'], dataset_dict['sigma'] = batch_dict['mus'], batch_dict['sigmas']
        if self.use_action_masks:                                    # a2c_common.py:1346-1347
            dataset_dict['action_masks'] = batch_dict['action_masks']
        self.dataset.update_values_dict(dataset_dict)
        if self.has_central_value:
            self.central_value_net.update_dataset({
                'old_values': values, 'advantages': advantages, 'returns': returns, 'actions': batch_dict['actions'],
                'obs': batch_dict['states'], 'dones': batch_dict['dones'], 'rnn_masks': rnn_masks,
            })

    def _prepare_dataset_general(self, batch_dict):
        """prepare_dataset for value_size > 1 (returns / values [B, V]): the reference's operation sequence
        (a2c_common.py:1598-1634) with the normaliser modules and torch ops - the fused prepare kernels carry one value
        column.  advantages = returns - values BEFORE the value normalisation, summed over V behind it (:1622)."""
        from . import torch_fallback as tf
        returns, values = batch_dict['returns'], batch_dict['values']
        rnn_masks = batch_dict.get('rnn_masks', None)
        advantages = returns - values                                                   # :1598
        if self.normalize_value:
            vms = self.value_mean_std
            if self.config.get('freeze_critic', False):                                 # :1601-1604
                vms.eval()
                values, returns = vms(values), vms(returns)
            elif rnn_masks is not None:                                                 # :1605-1615
                valid = rnn_masks.reshape(-1).bool()
                vms.train()
                vms(values[valid])
                vms(returns[valid])
                vms.eval()
                values, returns = vms(values), vms(returns)
            else:                                                                       # :1616-1620
                vms.train()
                values = vms(values)
                returns = vms(returns)
                vms.eval()
        advantages = torch.sum(advantages, dim=1)                                       # :1622
        if self.normalize_advantage:
            if self.normalize_rms_advantage:
                advantages = self.advantage_mean_std(advantages, mask=rnn_masks)
            else:
                advantages = tf.normalize_advantages(advantages, rnn_masks)
        self._update_datasets(batch_dict, values, returns, advantages, rnn_masks)

    # ================================================================== update
    def train_actor_critic(self, input_dict):
        self.set_train()
        self.calc_gradients(input_dict)
        return self.train_result

    def calc_gradients(self, input_dict):
        """a2c_continuous.py:136-234, a2c_discrete.py:121-209 - forward, fused loss + analytic backward + KL, optimiser."""
        row = self._mb_scalars[self._mb_index % self._mb_scalars.shape[0]]
        self._mb_index += 1
        self._forward_loss_backward(input_dict, row)
        self.trancate_gradients_and_step()
        # (a central value network without `use_experimental_cv`: no actor value loss, a2c_discrete.py:164-167)
        c_loss = row[1] if self.has_value_loss else torch.zeros((), device=row.device)
        self.train_result = (row[0], c_loss, row[2], row[4], self._host_lr, 1.0)
        if not self.is_discrete:        # dataset.update_mu_sigma happened inside the loss kernel (write_back)
            self.train_result += (input_dict['mu'], input_dict['sigma'], row[3])

    def _forward_loss_backward(self, input_dict, row):
        """Everything of calc_gradients up to (and including) the gradients in the arena: the update of the chosen path,
        or the autograd path's where the path does not take the minibatch's observations."""
        path = self._path if self._path.takes(input_dict['obs']) else self._autograd
        path.update(input_dict, row)

    def _torch_batch(self, input_dict, obs):
        """The training input of the torch model's forward (a2c_continuous.py:141-153, a2c_discrete.py:131-144)."""
        batch = {'is_train': True, 'prev_actions': input_dict['actions'], 'obs': obs}
        if self.is_rnn:
            batch['rnn_states'] = input_dict['rnn_states']
            batch['seq_length'] = self.seq_length
            if self.zero_rnn_on_done:
                batch['dones'] = input_dict['dones']
        return batch

    def _loss_scalars(self):
        """(coef_c, coef_b, bound kind) of the loss.  Central value without `use_experimental_cv`: the actor's own value
        head is not trained (c_loss = zeros, a2c_continuous.py:112-115) - a zero coefficient removes it from loss and grads."""
        coef_b = self.bounds_loss_coef if self.bounds_loss_coef is not None else 0.0
        kind = 0 if self.bounds_loss_coef is None else ops.BOUND_KINDS.get(self.bound_loss_type, 0)
        return self.critic_coef if self.has_value_loss else 0.0, coef_b, kind

    def _ppo_loss_setup(self, input_dict, mu, logstd, values, d_mu, d_values):
        """The loss of one minibatch, set up once for every path: (args, fin) - `args` the arguments of ops.ppo_loss_fused
        / ppo_loss_desc, fin(blocks, row, *bias_grads) those of ops.ppo_loss_finalize / loss_finalize_desc."""
        mask, mask_sum = ops.sequence_mask(input_dict.get('rnn_masks', None))
        coef_c, coef_b, kind = self._loss_scalars()
        (mb, A), sigma_grad = mu.shape, self.model.a2c_network.sigma.grad
        args = (mu.detach(), logstd.detach(), values, input_dict['actions'], input_dict['old_logp_actions'],
                input_dict['advantages'], input_dict['old_values'].reshape(-1), input_dict['returns'].reshape(-1),
                input_dict['mu'], input_dict['sigma'], d_mu, d_values, self._loss_partials, self.e_clip, coef_c, coef_b,
                self.clip_value, self.surrogate, kind, True, mask, mask_sum)

        def fin(blocks, row, *bias_grads):
            return (self._loss_partials, blocks, A, mb, mask is not None, coef_c, self.entropy_coef, coef_b, row,
                    sigma_grad, self.optimizer.kl_slot) + bias_grads
        return args, fin

    @torch.no_grad()
    def _loss_launches(self, input_dict, row, policy, values, d_mu, d_values):
        """The fused loss launch (d mu / d value, per-block partials, mu / sigma written back into the dataset) and its
        finalise launch (the scalars in `row`, log sigma's gradient, the KL)."""
        args, fin = self._ppo_loss_setup(input_dict, *policy, values, d_mu, d_values)
        ops.ppo_loss_fused(*args)
        ops.ppo_loss_finalize(*fin(ops.ppo_loss_blocks(d_mu.shape[0]), row))

    def _diag_update(self, input_dict, policy):
        """Behind the backward: the step's mu is in the dataset (write_back), log sigma still the pre-step one."""
        self._diag_minibatch(input_dict, mu=input_dict['mu'], logstd=policy[1].detach(), actions=input_dict['actions'])

    def _diag_minibatch(self, input_dict, **new_policy):
        """The diagnostics launch of this minibatch (a2c_continuous.py:223-230, a2c_discrete.py:200-207): writes the
        minibatch's row of the device table; nothing when `use_diagnostics` is off or on ranks other than 0.
        new_policy: new_neglogp [mb], or mu / logstd / actions (the neglogp recomputed in the launch)."""
        if not isinstance(self.diagnostics, PpoDiagnostics):
            return
        slot = self._diag_slot if self._diag_slot is not None else (self._mb_index - 1) % len(self.dataset)
        masks = input_dict.get('rnn_masks', None)
        batch = dict(values=input_dict['old_values'], returns=input_dict['returns'],
                     old_neglogp=input_dict['old_logp_actions'], masks=masks, **new_policy)
        with torch.no_grad():
            self.diagnostics.mini_batch(self, batch, self.e_clip, slot)

    def _native_comm(self):
        """The in-graph gradient collective, created on first use: the hipIpc all-reduce kernel
        (csrc/ipc_allreduce.hip; `native_allreduce: True`, the default), RCCL through the C ABI as a stream launch
        (csrc/rccl_wrap.hip; `native_allreduce: 'rccl'`, or as the fallback of the former with `rccl_in_graph_fallback:
        True`), or None: `native_allreduce: False` / nothing of the above could be set up - the collective then runs
        through torch.distributed between two graph replays per step."""
        if self._ipc_comm is False:
            return None
        if self._ipc_comm is None:
            self._ipc_comm = False
            want = self.config.get('native_allreduce', True)
            if self.multi_gpu and want:
                n = self.optimizer.flat_grads.numel()
                if want != 'rccl':
                    try:
                        from .ipc_allreduce import IpcAllReduce
                        self._ipc_comm = IpcAllReduce(n, self.ppo_device,
                                                      timeout_s=self.config.get('native_allreduce_timeout_s'),
                                                      two_phase=self.config.get('native_allreduce_two_phase'))
                    except Exception as e:
                        print(f'rl_games_amd: native all-reduce unavailable ({type(e).__name__}: {e}); using RCCL')
                        self._ipc_comm = False
                if not self._ipc_comm and (want == 'rccl' or self.config.get('rccl_in_graph_fallback', False)):
                    try:
                        from .rccl_allreduce import RcclAllReduce
                        self._ipc_comm = RcclAllReduce(n, self.ppo_device)
                    except Exception as e:
                        print(f'rl_games_amd: in-graph RCCL unavailable ({type(e).__name__}: {e}); using torch.distributed')
                        self._ipc_comm = False
        return self._ipc_comm or None

    def _all_reduce_grads(self):
        """Gradients + KL slot, one collective (a2c_common.py:493-509, :1559-1560)."""
        comm = self._native_comm()
        if comm is not None:
            # a plain kernel launch: capturable.  The reduced gradients pass through its registers, so it
            # also leaves the sums of squares clip_grad_norm_ needs (no grad_sumsq launch behind it).
            comm.all_reduce_sum(self.optimizer.flat_grads, norm=self._all_reduce_norm_plan(comm))
        else:
            rdist.all_reduce_sum(self.optimizer.flat_grads)
        self.last_allreduce = getattr(comm, 'kind', 'ipc') if comm is not None else 'rccl'

    def _all_reduce_norm_plan(self, comm):
        """The `norm` argument of the native all-reduce launch; also tells the optimiser launch (eager or about
        to be captured) that the gradient norm partials will be there.  Launches nothing."""
        if comm is None or not getattr(comm, 'supports_norm', True) or not self.config.get('norm_in_allreduce', True):
            return None
        opt = self.optimizer
        if self._ar_norm_partials is None:
            self._ar_norm_partials = torch.zeros(comm.norm_blocks(), dtype=torch.float64, device=self.ppo_device)
        self._norm_ready = (self._ar_norm_partials, comm.norm_blocks())
        return (self._ar_norm_partials, opt.numel, 1.0 / self.world_size, opt.step_counter)

    def trancate_gradients_and_step(self):
        """a2c_common.py:493-514 (+ the per-minibatch lr control of :1557-1563)."""
        if self.multi_gpu:
            self._all_reduce_grads()
        self._optimizer_kernels()

    def _step_arguments(self):
        scale = 1.0 / self.world_size if self.multi_gpu else 1.0
        schedule = None
        if self.is_adaptive_lr and self.schedule_type == 'per_minibatch':
            schedule = self.scheduler.device_rule()
        return dict(grad_scale=scale, max_norm=self.grad_norm if self.truncate_grads else None,
                    schedule=schedule, kl_scale=scale)

    def _optimizer_kernels(self):
        opt = self.optimizer
        # behind the in-graph all-reduce the step takes the collective's error word: a step whose gradients
        # are invalid (a peer never arrived) changes nothing
        skip = self._ipc_comm.error_word if (self.multi_gpu and self._ipc_comm) else None
        # the Adam launch writes the planes of adam_pack_chain, one pack launch behind it the lean 16-row kernels' fragments
        # - inside the captured graphs too: no launch of this agent ever packs on demand
        opt.step(norm_ready=self._norm_ready, skip_flag=skip, pack=self._adam_pack_chain(), **self._step_arguments())
        self._norm_ready = None
        self._form_chains.after_step(opt)

    def _graph_chains(self):
        """The fused chains that this agent's captured graphs read, in the order their forms are brought up to date: the
        actor path's, then the critic's (_ChainForms)."""
        actor = self._path.chain_forms()
        critic = self.central_value_net.chain_forms() if self.has_central_value else []
        # (the discrete recurrent engine's chain has always come behind the critic's; the order is the order of the pack
        #  launches in front of a replayed rollout, so it stays)
        return critic + actor if self._path.kind == 'recurrent' else actor + critic

    # ------------------------------------------------------------------ HIP graphs
    def _with_fold(self, mb_index, fn, *args):
        """Run fn with the minibatch index visible to _forward_loss_backward (the in-kernel statistics
        fold needs it); a no-op wrapper when the epoch has no precomputed minibatch moments."""
        self._fold_index = mb_index if self._fold_ready else None
        self._diag_slot = mb_index
        try:
            return fn(*args)
        finally:
            self._fold_index = self._diag_slot = None

    def _prepare_obs_fold(self):
        """Once per epoch, after prepare_dataset: column moments of every minibatch's observations in
        two launches (instead of a moments + a merge launch in each of the epoch's optimiser steps)."""
        self._fold_ready = False
        if (self._path.fused_chain is None or not self.normalize_input or self.is_rnn
                or not self.config.get('fold_obs_stats', True)):
            return
        obs = self.dataset.values_dict.get('obs')
        if not torch.is_tensor(obs) or obs.dim() != 2 or not obs.is_contiguous() or obs.dtype != torch.float32:
            return
        if obs.shape[0] != len(self.dataset) * self.minibatch_size:
            return
        self.model.running_mean_std.precompute_minibatch_moments(obs, self.minibatch_size)
        self._fold_ready = True

    def _graph_signature(self):
        """Everything a captured minibatch graph bakes in: dataset storage addresses and the
        scalar hyper-parameters passed by value to the kernels."""
        vd = self.dataset.values_dict
        ptrs = tuple(vd[k].data_ptr() for k in ('obs', 'actions', 'old_logp_actions', 'advantages',
                                               'old_values', 'returns', 'mu', 'sigma', 'dones'))
        if self.is_rnn:
            ptrs += tuple(s.data_ptr() for s in vd['rnn_states'])
        s = self.scheduler
        sched = (getattr(s, 'kl_threshold', None), getattr(s, 'min_lr', None), getattr(s, 'max_lr', None),
                 getattr(s, 'lr_multiplier', None))
        return (ptrs, self.e_clip, self.critic_coef, self.entropy_coef, self.bounds_loss_coef,
                self.bound_loss_type, self.clip_value, self.surrogate, self.grad_norm,
                self.truncate_grads, self.schedule_type, self.is_adaptive_lr, sched, self.world_size,
                self._fold_ready and self.model.running_mean_std._mb_table.data_ptr(),
                self.chain_products, self._guard is not None)

    def _graphs_usable(self):
        return (self._hip_graphs and self._path.graphs and self._eager_epochs >= 1
                and self.dataset.values_dict.get('rnn_masks') is None and not self._graph_failed)

    def _graph_minibatch(self, i):
        """Replay (capturing on first use) the forward/loss/backward graph of minibatch i, run the
        gradient all-reduce eagerly, then replay the (norm, Adam, lr) graph."""
        graphs, capture = self._update_graphs, self._capturer.capture
        graphs.refresh(self._graph_signature())
        g = graphs.minibatch.get(i)
        if g is None:
            item = self.dataset[i]
            g = graphs.minibatch[i] = capture(lambda: self._with_fold(i, self._forward_loss_backward, item,
                                                                      self._graph_rows[i]))
            graphs.norm_state = self._norm_ready      # what the captured launches will have produced
        self._form_chains.before_replay()
        if graphs.optimizer is None:
            # Captured BEFORE anything of this minibatch runs (a failed capture then leaves minibatch i untouched
            # for the eager path), knowing which launch in front of it produces the gradient norm - the
            # weight-gradient finalise on one GPU, the native all-reduce on several - so that the graph carries no
            # grad_sumsq of its own.
            self._norm_ready = graphs.norm_state
            if self.multi_gpu:
                self._all_reduce_norm_plan(self._native_comm())
            graphs.optimizer = capture(self._optimizer_kernels)
        g.replay()
        if self.multi_gpu:
            self._all_reduce_grads()
        self._norm_ready = None
        graphs.optimizer.replay()
        self.optimizer.step_done()
        self._form_chains.after_step(self.optimizer, packed=True)

    def _graph_mini_epoch(self, nmb):
        """Single-GPU runs with nothing to do on the host between minibatches (device-side or
        per-epoch lr schedule): ALL minibatches of a mini-epoch - forward, loss, backward, clip, Adam,
        lr update, nmb times - are one HIP graph, replayed once per mini-epoch."""
        graphs = self._update_graphs
        graphs.refresh(self._graph_signature())
        if graphs.epoch is None:
            def body():
                for i in range(nmb):
                    self._with_fold(i, self._forward_loss_backward, self.dataset[i], self._graph_rows[i])
                    if self.multi_gpu:
                        self._all_reduce_grads()          # native in-graph collective only (see train_epoch)
                    self._optimizer_kernels()
                if self._fold_ready:
                    self.model.running_mean_std.fold_sync(nmb)
            graphs.epoch = self._capturer.capture(body)
        self._form_chains.before_replay()
        graphs.epoch.replay()
        self.optimizer.step_count += nmb
        self.optimizer.weights_version += nmb
        self._form_chains.after_step(self.optimizer, packed=True)

    def _host_schedule(self, kl_value):
        lr, self.entropy_coef = self.scheduler.update(self._host_lr, self.entropy_coef, self.epoch_num,
                                                      self.frame, kl_value)
        if lr != self._host_lr:
            self.update_lr(lr)

    def train_epoch(self):
        """a2c_common.py:1517-1584."""
        self.vec_env.set_train_info(self.frame, self)
        self.set_eval()
        play_time_start = time.perf_counter()
        with torch.no_grad():
            batch_dict = self.play_steps_rnn() if self.is_rnn else self.play_steps()
        play_time_end = time.perf_counter()
        update_time_start = time.perf_counter()
        self.set_train()
        self.curr_frames = batch_dict.pop('played_frames')
        if self._guard is not None and self._range_verdict('rollout'):
            # policy 'exact': the rollout came off overflowed planes - no prepare_dataset (value_mean_std), no update
            now = time.perf_counter()
            nan = [torch.full((), float('nan'), device=self.ppo_device)]
            return (batch_dict['step_time'], play_time_end - play_time_start, now - update_time_start,
                    now - play_time_start, nan, list(nan), [], list(nan), list(nan), self._host_lr, 1.0)
        self.prepare_dataset(batch_dict)
        self.algo_observer.after_steps()
        self._prepare_obs_fold()

        a_losses, c_losses, b_losses, entropies, kls = [], [], [], [], []
        if self.has_central_value:                                   # a2c_common.py:1536-1537
            self.train_central_value()
            self.set_train()
        self._mb_index = 0
        device_schedule = self.is_adaptive_lr and self.schedule_type == 'per_minibatch'
        last_lr, lr_mul = self.last_lr, 1.0
        use_graphs = self._graphs_usable() and (device_schedule or self.schedule_type != 'per_minibatch'
                                                or not self.is_adaptive_lr)
        nmb = len(self.dataset)
        for mini_ep in range(self.mini_epochs_num):
            first = self._mb_index
            done = 0                     # minibatches of this mini-epoch already stepped
            fold_synced = False
            if use_graphs:
                try:
                    self.set_train()
                    host_between = self.schedule_type == 'per_minibatch' and not device_schedule
                    in_graph_comm = (not self.multi_gpu) or self._native_comm() is not None
                    if in_graph_comm and not host_between and self.config.get('mini_epoch_graph', True):
                        self._graph_mini_epoch(nmb)      # (the statistics hand-back is part of the graph)
                        done = nmb
                        fold_synced = True
                    else:
                        for i in range(nmb):
                            self._graph_minibatch(i)
                            done = i + 1
                            if host_between:
                                self._host_schedule(None)
                except GraphCaptureError as e:
                    # A capture executes nothing and the host mirrors were rolled back, so the
                    # remaining minibatches of this mini-epoch (and all later ones) run eagerly.
                    print(f'rl_games_amd: HIP graph capture failed ({e.__cause__!r}); continuing eagerly')
                    self._graph_failed = True
                    self._update_graphs.clear()
                    self._rollout_graphs.clear()      # (never used again: _rollout_graphs_usable)
                    use_graphs = False
                self._mb_scalars[first:first + done].copy_(self._graph_rows[:done])
                self._mb_index += done
                for i in range(done):
                    row = self._mb_scalars[first + i]
                    a_losses.append(row[0])
                    c_losses.append(row[1])
                    entropies.append(row[2])
                    if self.bounds_loss_coef is not None:
                        b_losses.append(row[3])
            if done < nmb:
                if self.is_discrete and done == 0:    # a2c_common.py:1263 (no-op unless `permute`)
                    self.dataset.apply_permutation()
                for i in range(done, nmb):
                    res = self._with_fold(i, self.train_actor_critic, self.dataset[i])
                    a_loss, c_loss, entropy, kl, last_lr, lr_mul = res[:6]
                    b_loss = res[8] if len(res) > 8 else None
                    a_losses.append(a_loss)
                    c_losses.append(c_loss)
                    entropies.append(entropy)
                    if self.bounds_loss_coef is not None:
                        b_losses.append(b_loss)
                    if self.schedule_type == 'per_minibatch' and not device_schedule:
                        self._host_schedule(None if not self.is_adaptive_lr else float(kl.item()))
            if self._fold_ready and not fold_synced:
                self.model.running_mean_std.fold_sync(nmb)
            av_kls = self._mb_scalars[first:self._mb_index, 4].mean()
            if self.multi_gpu:
                rdist.all_reduce_sum(av_kls)
                av_kls /= self.world_size
            if self.schedule_type == 'standard':
                self._host_schedule(float(av_kls.item()))
            kls.append(av_kls)
            self.diagnostics.mini_epoch(self, mini_ep)                 # a2c_common.py:1574
            if self.normalize_input:
                self.model.running_mean_std.eval()
        if self.schedule_type == 'standard_epoch':
            self._host_schedule(float(torch.stack(kls).mean().item()))
        self._fold_ready = False
        self.sync_running_stats()
        # (policy 'exact': every step from the tripped one on was skipped on the device; the next epoch runs on exact
        #  products, eagerly - it is the warm-up epoch of the new launches, so this epoch does not count as one)
        switched = self._guard is not None and self._range_verdict('update')
        self._check_ranks_in_sync()
        if self._ipc_comm:
            # one host read per epoch; the verdict is collective, so that every rank raises in the same epoch
            # instead of one rank leaving the others to hang in their next collective
            _, timed_out = self._ipc_comm.status()
            flag = torch.tensor([float(timed_out != 0)], device=self.ppo_device)
            import torch.distributed as dist
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            if flag.item() != 0:
                raise RuntimeError(f'in-graph all-reduce: a launch gave up waiting for a peer rank (this rank: '
                                   f'launch {timed_out or "none"}); the optimiser steps behind it were skipped on the '
                                   f'rank that gave up - parameters may differ between ranks, aborting on all ranks. '
                                   f'Raise native_allreduce_timeout_s / RLG_IPC_TIMEOUT_S for legitimately long rank '
                                   f'skews, or set native_allreduce: False to use RCCL.')
        self._eager_epochs += 0 if (use_graphs or switched) else 1
        if self._guard is None:
            self._check_split_range()
        if device_schedule:
            # one host read per epoch: [lr the last minibatch was stepped with, lr for the next one]
            used, nxt = self.optimizer.last_and_next_lr()
            last_lr = used                  # what the reference returns (train_result[4])
            self.last_lr = self._host_lr = nxt
        else:
            last_lr = self._host_lr
        update_time_end = time.perf_counter()
        play_time = play_time_end - play_time_start
        update_time = update_time_end - update_time_start
        total_time = update_time_end - play_time_start
        return (batch_dict['step_time'], play_time, update_time, total_time, a_losses, c_losses, b_losses,
                entropies, kls, last_lr, lr_mul)

    def _check_split_range(self):
        """Split-fp16 chain launches (csrc/bx_form.hpp) scale weights and hidden activations by FIXED powers of two: a
        hidden activation of 4,094 or a weight of 1,023 and more becomes Inf in its plane and NaN in everything computed
        from it - never a finite wrong value, but the reason deserves a sentence (a warning, once: the reference would train on
        with NaNs as well).  One host read per epoch."""
        if self._path.fused_chain is None or self._mb_index == 0:
            return
        n = min(self._mb_index, self._mb_scalars.shape[0])
        if not getattr(self, '_split_range_warned', False) and \
                not bool(torch.isfinite(self._mb_scalars[:n, :5]).all().item()):
            self._split_range_warned = True
            import warnings
            warnings.warn(
                'rl_games_amd: non-finite losses in this epoch.  If the inputs are finite: the split-fp16 chain kernels hold '
                '|hidden activation| < 4094 and |weight| < 1023 (fixed operand scales, csrc/bx_form.hpp); a network '
                "beyond that runs on exact fp32 products with chain_products: 'exact'; split_range: 'raise' / 'exact' "
                'keeps such an epoch away from parameters and normalisers.', RuntimeWarning)

    # ------------------------------------------------------------------ range guard (range_guard.py)
    def _range_engines(self):
        """Every engine of this agent that finishes weight gradients (chain_net.WeightGrads)."""
        return list(self._path.engines) + (self.central_value_net.engines() if self.has_central_value else [])

    def _set_chain_products(self, mode):
        """Every chain of the agent (and of its central value network) on `mode`, the weight-gradient launches on the
        matching form.  Captured graphs hold the other mode's launches: they go (the mode is part of the update graphs'
        signature too), and the next epoch runs eagerly like the first."""
        self._form_chains.set_products(mode)
        for e in self._range_engines():
            e.weight_grads.form = 'exact' if mode == 'exact' else None
        if mode != self.chain_products:
            self._update_graphs.clear()
            self._rollout_graphs.clear()
            self._eager_epochs = 0
        self.chain_products = mode
        if self.central_value_net is not None:
            self.central_value_net.chain_products = mode

    def _arm_range_guard(self):
        """At the end of construction: the configured product mode on every chain, and - split_range 'raise' / 'exact' -
        the guard record into this agent's optimiser and its critic's."""
        self._guard = None
        self._range_noticed = False
        if self.central_value_net is not None and self.central_value_net.chain_products == 'exact':
            self.chain_products = 'exact'                 # (one mode for the agent and its critic)
        self._set_chain_products(self.chain_products)
        if self.split_range == 'warn' and (self.central_value_net is None or self.central_value_net.split_range == 'warn'):
            return
        if self.split_range == 'warn':
            self.split_range = self.central_value_net.split_range
        self._guard = ops.guard_record(self.ppo_device)
        self.optimizer.guard = self._guard
        if self.central_value_net is not None:
            self.central_value_net.share_range_guard(self._guard)

    def _scan_rollout(self, batch_dict):
        """Armed: ONE launch, behind _finish_rollout, over everything prepare_dataset and the update take from the policy
        launches - values (a central value critic's, where there is one: they replace the actor's in the buffer),
        neglogps, for a continuous policy mus (a discrete policy's logits are not kept; its neglogps come from them), and
        the returns: the bootstrap values of the observation behind the last step are one more launch on the same planes,
        kept in no buffer, and reach value_mean_std through the returns alone.  No host read."""
        if self._guard is None:
            return
        st = self.experience_buffer.storage
        arrays = [(st['values'], range_guard.TAG_CRITIC_VALUES if self.has_central_value else range_guard.TAG_VALUES),
                  (st['neglogpacs'], range_guard.TAG_NEGLOGPS)]
        if not self.is_discrete:
            arrays.append((st['mus'], range_guard.TAG_POLICY))
        returns = batch_dict['returns']
        arrays.append((returns if returns.is_contiguous() else returns.contiguous(), range_guard.TAG_RETURNS))
        ops.range_scan(arrays, self._guard)

    def _range_verdict(self, phase):
        """One host read of the guard record; under multi_gpu the verdict is collective (MAX), so every rank takes the
        same branch in the same epoch.  Clean: False.  Tripped: SplitRangeError under policy 'raise', or when the
        products are exact already (then the inputs are not finite); under policy 'exact' one notice, every chain on
        exact products, the record cleared, True - the caller drops what is left of the epoch."""
        what = range_guard.verdict(self._guard, phase, self.split_range, self.chain_products, self.multi_gpu,
                                   self.ppo_device, ops.read_guard)
        if what is None:
            return False
        if not self._range_noticed:
            self._range_noticed = True
            print(f'rl_games_amd: {what}.  split_range: exact - the rest of this epoch is dropped, training continues on '
                  f'exact fp32 products (the actions of this rollout have already gone to the environment).', flush=True)
        self._set_chain_products('exact')
        self._guard.zero_()
        return True

    # ================================================================== multi-GPU stats
    def _stats_sync_modules(self):
        mods = []
        if self.normalize_input and hasattr(self.model, 'running_mean_std'):
            mods.append(self.model.running_mean_std)
        if self.normalize_value and getattr(self.model, 'value_mean_std', None) is not None:
            mods.append(self.model.value_mean_std)
        if self.has_central_value:                                   # a2c_common.py:759-765
            cv_model = self.central_value_net.model
            if getattr(cv_model, 'running_mean_std', None) is not None:
                mods.append(cv_model.running_mean_std)
            if getattr(cv_model, 'value_mean_std', None) is not None:
                mods.append(cv_model.value_mean_std)
        return mods

    def _stats_sync(self):
        """One StatsSync over every normaliser of the agent (actor + central value): an epoch's exchange is
        two launches and ONE collective (csrc/running_stats.hip, distributed.StatsSync)."""
        mods = self._stats_sync_modules()
        if not mods:
            return None
        sync = getattr(self, '_stats_sync_obj', None)
        if sync is None or not sync.covers(mods):
            sync = self._stats_sync_obj = rdist.StatsSync(mods)
        return sync

    def _seed_stats_sync_snapshots(self):
        """a2c_common.py:766-780: restored statistics are shared history, not fresh per-rank data."""
        if not self.multi_gpu or not self.multi_gpu_sync_stats or self.multi_gpu_sync_stats_mode == 'broadcast':
            return
        sync = self._stats_sync()
        if sync is not None:
            sync.seed()

    def _check_ranks_in_sync(self):
        """Guard against silent rank drift (round 5: two ranks ended epochs with `exp_avg_sq` one update apart in 16
        elements, profiles/r5_two_rank_sync.txt - found by bench.py's probe only): an exact checksum of parameters and
        Adam moments, one tiny all-reduce per epoch."""
        if not self.multi_gpu or not self.multi_gpu_param_check:
            return
        o = self.optimizer
        if rdist.ranks_in_sync([o.flat_params, o.exp_avg, o.exp_avg_sq]):
            return
        if self.multi_gpu_param_check == 'rebroadcast':
            print(f'rl_games_amd: rank {self.global_rank}: parameters / Adam moments differ between the ranks after epoch '
                  f'{self.epoch_num}; taking rank 0\'s', flush=True)
            import torch.distributed as dist
            for t in (o.flat_params, o.exp_avg, o.exp_avg_sq):
                dist.broadcast(t, 0)
            o.weights_changed()
            return
        raise RuntimeError(f'rank {self.global_rank}: parameters / Adam moments are no longer bit-identical across the ranks '
                           f'(epoch {self.epoch_num}); multi_gpu_param_check: \'rebroadcast\' re-aligns them instead of raising')

    def sync_running_stats(self):
        """a2c_common.py:782-808."""
        if not self.multi_gpu or not self.multi_gpu_sync_stats:
            return
        sync = self._stats_sync()
        if sync is None:
            return
        if self.multi_gpu_sync_stats_mode == 'broadcast':
            sync.adopt_rank0(rdist.broadcast_from_rank0)
        else:
            sync.merge(rdist.all_reduce_sum)

    # ================================================================== weights / checkpoints
    def get_stats_weights(self, model_stats=False):
        state = {}
        if self.normalize_rms_advantage:
            state['advantage_mean_std'] = self.advantage_mean_std.state_dict()
        if self.has_central_value:
            state['central_val_stats'] = self.central_value_net.get_stats_weights(model_stats)
        if model_stats:
            if self.normalize_input:
                state['running_mean_std'] = self.model.running_mean_std.state_dict()
            if self.normalize_value:
                state['reward_mean_std'] = self.model.value_mean_std.state_dict()
        return state

    def set_stats_weights(self, weights):
        if self.normalize_rms_advantage and 'advantage_mean_std' in weights:
            self.advantage_mean_std.load_state_dict(weights['advantage_mean_std'])
        if self.normalize_input and 'running_mean_std' in weights:
            self.model.running_mean_std.load_state_dict(weights['running_mean_std'])
        if self.normalize_value and 'reward_mean_std' in weights:
            self.model.value_mean_std.load_state_dict(weights['reward_mean_std'])

    def _plain_model(self):
        """The policy module itself.  The reference Runner re-assigns `agent.model = torch.compile(agent.model)` unless the
        config says `torch_compile: False` (torch_runner.py:283-307); nothing of this agent calls the wrapper's forward,
        and checkpoints are written / read in the plain key format whichever object `self.model` is."""
        return getattr(self.model, '_orig_mod', self.model)

    def get_weights(self):
        state = self.get_stats_weights()
        state['model'] = self._plain_model().state_dict()
        return state

    def set_weights(self, weights):
        model_state = {k.replace('_orig_mod.', ''): v for k, v in weights['model'].items()}
        self._plain_model().load_state_dict(model_state)      # copy_ into the arena views: params stay flat
        self.optimizer.weights_changed()
        self.set_stats_weights(weights)
        self._seed_stats_sync_snapshots()

    def get_full_state_weights(self):
        state = self.get_weights()
        state['epoch'] = self.epoch_num
        state['frame'] = self.frame
        state['optimizer'] = self.optimizer.state_dict()
        if self.has_central_value:
            state['assymetric_vf_nets'] = self.central_value_net.state_dict()
            state['assymetric_vf_optimizer'] = self.central_value_net.optimizer.state_dict()
        state['last_mean_rewards'] = self.last_mean_rewards
        if self.vec_env is not None:
            state['env_state'] = self.vec_env.get_env_state()
        manifest = self.config.get('capability_manifest')
        if manifest is not None:
            state['capability_manifest'] = manifest
        return state

    def set_full_state_weights(self, weights, set_epoch=True):
        self.set_weights(weights)
        if set_epoch:
            self.epoch_num = weights['epoch']
            self.frame = weights['frame']
        if self.has_central_value:
            self.set_central_value_function_weights(weights)
            if 'assymetric_vf_optimizer' in weights:
                self.central_value_net.optimizer.load_state_dict(weights['assymetric_vf_optimizer'])
        self.optimizer.load_state_dict(weights['optimizer'])
        self._host_lr = self.last_lr = self.optimizer.param_groups[0]['lr']
        self.last_mean_rewards = weights.get('last_mean_rewards', -float('inf'))
        if self.vec_env is not None:
            self.vec_env.set_env_state(weights.get('env_state', None))
        if 'capability_manifest' in weights and self.config.get('capability_manifest') is None:
            self.config['capability_manifest'] = weights['capability_manifest']
        self._seed_stats_sync_snapshots()

    def save(self, fn):
        state = self.get_full_state_weights()
        path = fn if fn.endswith('.pth') else fn + '.pth'
        torch.save(state, path)                              # torch_ext.save_checkpoint :73-92
        return path

    def restore(self, fn, set_epoch=True):
        checkpoint = torch.load(fn, map_location=self.ppo_device, weights_only=False)
        self.set_full_state_weights(checkpoint, set_epoch=set_epoch)

    def set_central_value_function_weights(self, weights):
        state = {k.replace('_orig_mod.', ''): v for k, v in weights['assymetric_vf_nets'].items()}
        self.central_value_net.load_state_dict(state)
        self._seed_stats_sync_snapshots()

    def restore_central_value_function(self, fn):
        checkpoint = torch.load(fn, map_location=self.ppo_device, weights_only=False)
        self.set_central_value_function_weights(checkpoint)

    def get_param(self, param_name):
        if param_name in ('grad_norm', 'critic_coef', 'bounds_loss_coef', 'entropy_coef', 'kl_threshold',
                          'gamma', 'tau', 'mini_epochs_num', 'e_clip'):
            return getattr(self, param_name)
        if param_name == 'learning_rate':
            return self._sync_lr_to_host()
        raise NotImplementedError(f"Can't get param {param_name}")

    def set_param(self, param_name, param_value):
        if param_name in ('grad_norm', 'critic_coef', 'bounds_loss_coef', 'entropy_coef', 'gamma', 'tau',
                          'mini_epochs_num', 'e_clip'):
            setattr(self, param_name, param_value)
        elif param_name == 'learning_rate':
            if self.is_adaptive_lr:
                raise NotImplementedError("Can't directly mutate LR on this schedule")
            self.update_lr(param_value)
        elif param_name == 'kl_threshold':
            if not self.is_adaptive_lr:
                raise NotImplementedError("Can't directly mutate kl threshold")
            self.kl_threshold = param_value
            self.scheduler.kl_threshold = param_value
        else:
            raise NotImplementedError(f'No param found for {param_value}')

    def broadcast_parameters(self):
        """Rank 0's parameters and normaliser state to every rank (a2c_common.py:1670-1680, C2) -
        one broadcast of the flat arena instead of a pickled state_dict."""
        if not self.multi_gpu:
            return
        import torch.distributed as dist
        dist.broadcast(self.optimizer.flat_params, 0)
        self.optimizer.weights_changed()
        if self.has_central_value:
            dist.broadcast(self.central_value_net.optimizer.flat_params, 0)
            # (c10d collectives write in place WITHOUT bumping the tensor's version counter: the chain's planes /
            #  fragments of the pre-broadcast weights have to be invalidated by hand, like the actor's above)
            self.central_value_net.optimizer.weights_changed()
        sync = self._stats_sync()
        if sync is not None:
            sync.adopt_rank0(rdist.broadcast_from_rank0)
        self._seed_stats_sync_snapshots()

    # ================================================================== training loop
    def train(self):
        """a2c_common.py:1662-1782.  Returns (last_mean_rewards, epoch_num)."""
        self._ensure_dirs()
        self.init_tensors()
        total_time = 0
        self.obs = self.env_reset()
        self.curr_frames = self.batch_size_envs
        self.broadcast_parameters()
        while True:
            epoch_num = self.update_epoch()
            res = self.train_epoch()
            if len(res) == 10:                     # discrete agents report no bound losses
                res = res[:6] + ([],) + res[6:]
            (step_time, play_time, update_time, sum_time, a_losses, c_losses, b_losses, entropies, kls,
             last_lr, lr_mul) = res
            total_time += sum_time
            curr_frames = self.curr_frames * self.world_size if self.multi_gpu else self.curr_frames
            self.frame += curr_frames
            frame = self.frame // self.num_agents
            self.dataset.update_values_dict(None)
            should_exit = False
            if self.global_rank == 0:
                self.diagnostics.epoch(self, current_epoch=epoch_num)         # a2c_common.py:1695
                if self.print_stats:
                    fps_step = curr_frames / max(step_time, 1e-9)
                    fps_inf = curr_frames / (self.num_agents * play_time)
                    fps_total = curr_frames / (self.num_agents * sum_time)
                    print(f'fps step: {fps_step:.0f} fps step and policy inference: {fps_inf:.0f} '
                          f'fps total: {fps_total:.0f} epoch: {epoch_num:.0f}/{self.max_epochs:.0f} '
                          f'frames: {frame:.0f}/{self.max_frames:.0f}')
                w = self.writer
                self.diagnostics.send_info(w)                                 # write_stats, a2c_common.py:529
                w.add_scalar('performance/step_inference_rl_update_fps', curr_frames / sum_time, frame)
                w.add_scalar('performance/step_inference_fps', curr_frames / play_time, frame)
                w.add_scalar('performance/rl_update_time', update_time, frame)
                w.add_scalar('performance/step_inference_time', play_time, frame)
                if not isinstance(w, NullWriter):
                    w.add_scalar('losses/a_loss', torch.stack(a_losses).mean().item(), frame)
                    w.add_scalar('losses/c_loss', torch.stack(c_losses).mean().item(), frame)
                    w.add_scalar('losses/entropy', torch.stack(entropies).mean().item(), frame)
                    w.add_scalar('info/kl', torch.stack(kls).mean().item(), frame)
                    if len(b_losses) > 0:
                        w.add_scalar('losses/bounds_loss', torch.stack(b_losses).mean().item(), frame)
                w.add_scalar('info/last_lr', last_lr * lr_mul, frame)
                w.add_scalar('info/e_clip', self.e_clip * lr_mul, frame)
                w.add_scalar('info/epochs', epoch_num, frame)
                self.algo_observer.after_print_stats(frame, epoch_num, total_time)
                mean_rewards = -np.inf
                if self.game_rewards.current_size > 0:
                    mean_rewards = self.game_rewards.get_mean()
                    mean_lengths = self.game_lengths.get_mean()
                    mean_rewards = np.atleast_1d(mean_rewards)
                    self.mean_rewards = mean_rewards[0]
                    w.add_scalar('rewards/step', mean_rewards[0], frame)
                    w.add_scalar('rewards/iter', mean_rewards[0], epoch_num)
                    w.add_scalar('episode_lengths/step', float(np.atleast_1d(mean_lengths)[0]), frame)
                    checkpoint_name = self.config['name'] + '_ep_' + str(epoch_num) + '_rew_' + str(mean_rewards[0])
                    if self.save_freq > 0 and epoch_num % self.save_freq == 0:
                        self.save(os.path.join(self.nn_dir, 'last_' + checkpoint_name))
                    if mean_rewards[0] > self.last_mean_rewards and epoch_num >= self.save_best_after:
                        self.last_mean_rewards = mean_rewards[0]
                        self.save(os.path.join(self.nn_dir, self.config['name']))
                        if 'score_to_win' in self.config and self.last_mean_rewards > self.config['score_to_win']:
                            self.save(os.path.join(self.nn_dir, checkpoint_name))
                            should_exit = True
                if epoch_num >= self.max_epochs and self.max_epochs != -1:
                    self.save(os.path.join(self.nn_dir, 'last_' + self.config['name'] + '_ep_' + str(epoch_num)))
                    should_exit = True
                if self.frame >= self.max_frames and self.max_frames != -1:
                    self.save(os.path.join(self.nn_dir, 'last_' + self.config['name'] + '_frame_' + str(self.frame)))
                    should_exit = True
                if not should_exit and self.stop_fn is not None and self.stop_fn(self):
                    self.save(os.path.join(self.nn_dir, 'last_' + self.config['name'] + '_custom_stop_ep_'
                                           + str(epoch_num)))
                    should_exit = True
            if self.multi_gpu:
                import torch.distributed as dist
                flag = torch.tensor(float(should_exit), device=self.ppo_device)
                dist.broadcast(flag, 0)                                                   # C8
                should_exit = bool(flag.item())
            if should_exit:
                return self.last_mean_rewards, epoch_num
