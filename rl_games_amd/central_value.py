"""Central (asymmetric) value function on MI355X - host mirror of `CentralValueTrain`
(rl_games/algos_torch/central_value.py:14-383): a value-only network over the privileged `states`,
trained on its own minibatches before the actor's, whose predictions replace the actor's values in
the rollout (a2c_common.py:593-615) and therefore in GAE.

Same kernels as the actor path: the state normaliser and value de-normaliser are `RunningMeanStd`
(csrc/running_stats.hip), the clipped value loss + its gradient + masked mean is one fused kernel
(`rlg_value_loss`) reduced by `rlg_ppo_loss_finalize`, clipping + Adam run on a flat parameter arena
(`FlatAdam`, csrc/optim.hip) with one in-place all-reduce per step in multi-GPU runs.  The network itself runs on the
actor paths' engines where it has their form - feed-forward critics on chain_net.ChainNet (`_engine`), recurrent ones on
chain_net.RecurrentChainNet with the value tail of csrc/rnn_value_tail.hip (`_rnn_engine`) - and keeps the torch module
between the loss and optimiser kernels otherwise (the conditions: DESIGN.md 4.1a).

Multi-agent envs (round 6, central_value.py:153-158,223-234): one state row per env, its value repeated for the env's agents
in the rollout, the critic trained on agent 0's values and returns.  Recurrent critics (round 6,
central_value.py:96-107,163-205): the network's RNN advances with the rollout (`pre_step_rnn` keeps the state every sequence
starts from, `post_step_rnn` / `zero_states_where` zero it where an episode ended) and trains on sequence minibatches.
"""
import torch
from torch import nn

from . import distributed as rdist
from . import ops, range_guard
from .actor_paths import fp32_space, train_forward
from .chain_net import ChainNet, RecurrentChainNet, arena_layout, rnn_cell_declined
from .flat_optim import FlatAdam
from .lr_control import IdentityScheduler, LinearScheduler
from .minibatch import PPODataset
from .normalizers import launch_stats
from .weight_forms import _ChainForms


def _value_chain(net, arena, max_rows):
    """Trunk + value head of a central value network on the fused chain kernels (chain_net.ChainNet): what autograd does
    for `CentralValueTrain.calc_gradients` (rl_games/algos_torch/central_value.py:278-335) between the loss kernel and
    the optimiser.  Raises NotImplementedError for networks outside the kernels' envelope (the caller keeps autograd)."""
    if not isinstance(net.value_act, nn.Identity) or net.value.out_features != 1:
        raise NotImplementedError('one linear value column only')
    if not getattr(net, 'plain_trunk', True) or net.is_rnn():
        raise NotImplementedError('plain Linear + activation trunks only')
    return ChainNet(net.actor_mlp, [net.value], arena, max_rows)


def _recurrent_critic_declined(net, config, value_size):
    """Why a recurrent critic stays off chain_net.RecurrentChainNet (None: it is eligible) - the conditions of
    actor_paths.RecurrentPath.declined for a value-only network."""
    if not config.get('fused_mlp', True):
        return 'fused_mlp is off'
    if not config.get('manual_lstm', True):
        return 'manual_lstm is off'
    if value_size != 1 or not isinstance(net.value_act, nn.Identity) or net.value.out_features != 1:
        return 'one linear value column only'
    if not getattr(net, 'plain_trunk_rnn_ln', False):
        return 'plain Linear + activation trunks only'
    return rnn_cell_declined(net.rnn_name, net.rnn_layers, net.rnn_units)


class CentralValueTrain(nn.Module):
    def __init__(self, state_shape, value_size, ppo_device, num_agents, horizon_length, num_actors,
                 num_actions, seq_length, normalize_value, network, config, writter, max_epochs, multi_gpu,
                 zero_rnn_on_done):
        super().__init__()
        self.ppo_device = ppo_device
        self.num_agents, self.horizon_length, self.num_actors = num_agents, horizon_length, num_actors
        self.seq_length, self.normalize_value, self.num_actions = seq_length, normalize_value, num_actions
        self.state_shape, self.value_size, self.max_epochs = state_shape, value_size, max_epochs
        self.multi_gpu, self.config = multi_gpu, config
        self.normalize_input = config['normalize_input']
        self.zero_rnn_on_done = zero_rnn_on_done
        # range guard of the split-fp16 products (range_guard.py).  Inside an agent the agent's keys and its record
        # take over (share_range_guard); a critic trained on its own arms a record of its own and gives the verdict
        # at the end of train_net.
        self.split_range, self.chain_products = range_guard.policy_from_config(config)
        self._guard, self._guard_shared, self._range_noticed = None, False, False
        self.model = network.build({
            'value_size': value_size, 'input_shape': state_shape, 'actions_num': num_actions,
            'num_agents': num_agents, 'num_seqs': num_actors, 'normalize_input': self.normalize_input,
            'normalize_value': self.normalize_value,
        }).to(ppo_device)
        self.is_rnn = self.model.is_rnn()
        self.rnn_states = None
        self.lr = float(config['learning_rate'])
        self.linear_lr = config.get('lr_schedule') == 'linear'
        if self.linear_lr:
            self.scheduler = LinearScheduler(self.lr, max_steps=self.max_epochs, apply_to_entropy=False,
                                             start_entropy_coef=0)
        else:
            self.scheduler = IdentityScheduler()
        self.mini_epoch = config['mini_epochs']
        if 'minibatch_size' not in config and 'minibatch_size_per_env' not in config:
            raise ValueError("Configuration must include either 'minibatch_size' or 'minibatch_size_per_env'. "
                             'Neither was found in the provided config.')
        self.minibatch_size_per_env = config.get('minibatch_size_per_env', 0)
        self.minibatch_size = config.get('minibatch_size', self.num_actors * self.minibatch_size_per_env)
        self.num_minibatches = self.horizon_length * self.num_actors // self.minibatch_size
        self.clip_value = config['clip_value']
        self.writter = writter
        self.weight_decay = config.get('weight_decay', 0.0)
        net = self.model.a2c_network
        layout = None
        rnn_declined = _recurrent_critic_declined(net, config, value_size) if self.is_rnn else None
        if self.is_rnn and rnn_declined is None:
            # what RecurrentChainNet asks of the arena: the head behind the matrices, the trunk's biases directly behind
            # the last matrix (chain_net.arena_layout)
            rest = [p for p in self.model.parameters() if all(p is not q for q in net.parameters())]
            first = [m.bias for m in net.actor_mlp if isinstance(m, nn.Linear)]
            layout = arena_layout(list(net.parameters()), [[net.value]], first_vectors=first) + rest
        self.optimizer = FlatAdam(self.model.parameters(), self.lr, eps=1e-08, weight_decay=self.weight_decay,
                                  layout=layout)
        self._engine = None            # feed-forward critics: chain_net.ChainNet
        self._rnn_engine = None        # recurrent critics: chain_net.RecurrentChainNet with the value tail
        if self.is_rnn:
            try:
                if rnn_declined is not None:
                    raise NotImplementedError(rnn_declined)
                self._rnn_engine = RecurrentChainNet(net.actor_mlp, net.rnn.rnn, net.layer_norm if net.rnn_ln else None,
                                                     [net.value], self.optimizer, self.minibatch_size,
                                                     infer_rows=self.num_actors, value_tail=True)
            except NotImplementedError as e:
                print(f'rl_games_amd: recurrent central value network outside the sequence-persistent RNN kernels ({e}); '
                      f'using autograd')
        elif config.get('fused_mlp', True) and value_size == 1:
            try:
                self._engine = _value_chain(net, self.optimizer, self.minibatch_size)
            except NotImplementedError as e:
                print(f'rl_games_amd: central value network outside the fused chain kernels ({e}); using autograd')
        self.set_chain_products(self.chain_products)
        if self.split_range != 'warn':
            self._guard = ops.guard_record(ppo_device)
            self.optimizer.guard = self._guard
        self.frame = 0
        self.epoch_num = 0
        self.grad_norm = config.get('grad_norm', 1)
        self.truncate_grads = config.get('truncate_grads', False)
        self.e_clip = config.get('e_clip', 0.2)
        self.batch_size = self.horizon_length * self.num_actors
        self.local_rank = self.global_rank = 0
        self.world_size = 1
        if self.multi_gpu:
            self.local_rank, self.global_rank, self.world_size = rdist.env_ranks()
        if self.is_rnn:                                            # central_value.py:96-107
            self.rnn_states = [s.to(ppo_device) for s in self.model.get_default_rnn_state()]
            num_seqs = self.horizon_length // self.seq_length
            assert (self.horizon_length * self.num_actors // self.num_minibatches) % self.seq_length == 0
            self.mb_rnn_states = [torch.zeros((num_seqs, s.size()[0], self.num_actors, s.size()[2]), dtype=torch.float32,
                                              device=ppo_device) for s in self.rnn_states]
        self.dataset = PPODataset(self.batch_size, self.minibatch_size, True, self.is_rnn, ppo_device, self.seq_length)
        mb = self.minibatch_size
        self._d_val = torch.empty(mb, dtype=torch.float32, device=ppo_device)
        self._partials = torch.empty((mb + 255) // 256, 7, dtype=torch.float64, device=ppo_device)
        self._rows = torch.zeros(max(1, self.mini_epoch * self.num_minibatches), 8, dtype=torch.float32,
                                 device=ppo_device)
        self._no_logstd = torch.zeros(1, dtype=torch.float32, device=ppo_device)
        self._row_index = 0

    def set_chain_products(self, mode):
        """'auto' / 'exact' for the critic's chain and its weight-gradient launch (ops.MlpChain.products)."""
        for eng in self.engines():
            eng.chain.products = mode
            eng.weight_grads.form = 'exact' if mode == 'exact' else None
        self.chain_products = mode

    # ------------------------------------------------------------------ what the agent asks of its critic
    rnn_on_engine = property(lambda self: self._rnn_engine is not None)
    last_states = property(lambda self: self._rnn_engine.last_states)       # behind infer() of a recurrent critic

    def engines(self):
        """The critic's engines that finish weight gradients (chain_net.WeightGrads): one at most."""
        return [e for e in (self._engine, self._rnn_engine) if e is not None]

    def chain_forms(self):
        """The chains an agent's step graphs read: the rollout's inference forward of `num_actors` rows."""
        return [_ChainForms(e.chain, ((self.num_actors, 0),), self.optimizer.flat_params) for e in self.engines()]

    def rollout_ok(self, state_space, recurrent_actor):
        """Can the agent's fused rollout step run this critic: on the chain kernels (feed-forward, one value column,
        `fused_mlp` not off in its config) or - behind a recurrent actor, whose play_steps_rnn is where the reference
        advances a recurrent critic (a2c_common.py:1085-1086) - on its recurrent engine, over fp32 states.  Any other
        critic keeps the torch rollout."""
        on_kernels = self._engine is not None or (self.rnn_on_engine and recurrent_actor)
        return on_kernels and fp32_space(state_space)

    def reserve_rollout(self):
        """The rollout heads [num_actors, 1]: allocated now, not inside the first step's capture."""
        if self._engine is not None:
            self._engine.reserve_infer(self.num_actors)

    def infer(self, states, rnn_states=None):
        """get_value's forward on the engine (central_value.py:208-222, ModelCentralValue.forward models.py:452-458): the
        states normalised in eval mode inside the launch; raw values [num_actors, 1] (any row stride of `states`).  A
        recurrent critic: its engine's T = 1 forward from `rnn_states` (None: the critic's own, which arrive zeroed
        where an episode ended), the next states left in `last_states`."""
        if states.stride(-1) != 1:
            states = states.contiguous()
        rms, eps = launch_stats(self.model.running_mean_std if self.normalize_input else None)
        if self.rnn_on_engine:
            return self._rnn_engine.forward(states, rms, eps, self.rnn_states if rnn_states is None else rnn_states,
                                            None, 1, keep=False)
        return self._engine.infer(states, rms, eps)

    def share_range_guard(self, record):
        """The agent's guard record: the critic's optimiser steps are guarded by it and the agent gives the verdict."""
        self._guard, self._guard_shared = record, True
        self.optimizer.guard = record

    def _range_verdict(self):
        """A critic with a record of its own: one host read behind its epoch (A2CAgent._range_verdict, phase 'update')."""
        what = range_guard.verdict(self._guard, 'central value update', self.split_range, self.chain_products,
                                   self.multi_gpu, self.ppo_device, ops.read_guard)
        if what is None:
            return
        if not self._range_noticed:
            self._range_noticed = True
            print(f'rl_games_amd: {what}.  split_range: exact - the optimiser steps from the tripped one on were skipped, '
                  f'training continues on exact fp32 products.', flush=True)
        self.set_chain_products('exact')
        self._guard.zero_()

    def decline_rnn_engine(self, reason):
        """Take a recurrent critic off its engine (the agent: conditions that only it knows); it trains with autograd."""
        if self._rnn_engine is not None:
            print(f'rl_games_amd: recurrent central value network outside the sequence-persistent RNN kernels ({reason}); '
                  f'using autograd')
            self._rnn_engine = None

    # ------------------------------------------------------------------ reference API
    def update_lr(self, lr):
        self.optimizer.set_lr(float(lr))           # identical on every rank by construction

    def get_stats_weights(self, model_stats=False):
        state = {}
        if model_stats:
            if self.normalize_input:
                state['running_mean_std'] = self.model.running_mean_std.state_dict()
            if self.normalize_value:
                state['reward_mean_std'] = self.model.value_mean_std.state_dict()
        return state

    def set_stats_weights(self, weights):
        pass

    def update_dataset(self, batch_dict):
        if self.num_agents > 1:                                    # central_value.py:153-158
            res = self.update_multiagent_tensors(batch_dict['old_values'], batch_dict['returns'], batch_dict['actions'],
                                                 batch_dict['dones'])
            batch_dict['old_values'], batch_dict['returns'], batch_dict['actions'], batch_dict['dones'] = res
        if self.is_rnn:                                            # central_value.py:163-170
            states = []
            for mb_s in self.mb_rnn_states:
                t_size = mb_s.size()[0] * mb_s.size()[2]
                states.append(mb_s.permute(1, 2, 0, 3).reshape(-1, t_size, mb_s.size()[3]))
            batch_dict['rnn_states'] = states
        self.dataset.update_values_dict(batch_dict)

    def _preproc_obs(self, obs_batch):
        if obs_batch.dtype == torch.uint8:
            obs_batch = obs_batch.float() / 255.0
        return obs_batch

    def pre_step_rnn(self, n):
        """central_value.py:189-194: the state each sequence of the rollout starts from."""
        if self.is_rnn and n % self.seq_length == 0:
            for s, mb_s in zip(self.rnn_states, self.mb_rnn_states):
                mb_s[n // self.seq_length, :, :, :] = s

    def post_step_rnn(self, all_done_indices, zero_rnn_on_done=True):
        """central_value.py:196-203 (indices of finished rows)."""
        if not self.is_rnn or not self.zero_rnn_on_done:
            return
        idx = all_done_indices[::self.num_agents] // self.num_agents
        for s in self.rnn_states:
            s[:, idx, :] = 0

    def zero_states_where(self, done_mask):
        """post_step_rnn for a device-side mask [num_actors * num_agents] instead of an index list (nothing waits for the
        host).  Multi-agent: post_step_rnn looks at every num_agents-th finished row, whichever agents those are; this
        form asks for agent 0 of an env - the same thing wherever the agents of an env finish together."""
        if self.is_rnn and self.zero_rnn_on_done:
            if self.num_agents > 1:
                done_mask = done_mask[::self.num_agents].contiguous()
            for s in self.rnn_states:
                ops.rnn_zero_done_states(s, done_mask)

    def update_multiagent_tensors(self, value_preds, returns, actions, dones):
        """central_value.py:225-234: the critic trains on one row per env and step - agent 0's values and returns in
        env-major order (the order of the flattened states); `dones` are cut, not re-ordered, exactly as there."""
        batch_size = self.batch_size
        ma_batch_size = self.num_actors * self.num_agents * self.horizon_length
        shape = (self.num_actors, self.num_agents, self.horizon_length, self.value_size)
        value_preds = value_preds.reshape(shape).transpose(0, 1).contiguous().view(ma_batch_size, self.value_size)[:batch_size]
        returns = returns.reshape(shape).transpose(0, 1).contiguous().view(ma_batch_size, self.value_size)[:batch_size]
        dones = dones.contiguous().view(ma_batch_size, self.value_size)[:batch_size]
        return value_preds, returns, actions, dones

    def forward(self, input_dict):
        return self.model(input_dict)

    def get_value(self, input_dict):
        self.eval()
        obs_batch = self._preproc_obs(input_dict['states'])
        with torch.no_grad():
            res = self.forward({'obs': obs_batch, 'actions': input_dict.get('actions', None),
                                'rnn_states': self.rnn_states, 'is_train': False})
        if self.is_rnn:                                            # central_value.py:222
            self.rnn_states = [s.contiguous() for s in res['rnn_states']]
        value = res['values']
        if self.num_agents > 1:                                    # every agent of an env gets the env's value (:223-225)
            value = value.repeat(1, self.num_agents)
            value = value.view(value.size()[0] * self.num_agents, -1)
        return value

    def train_critic(self, input_dict):
        self.train()
        return self.calc_gradients(input_dict)

    def train_net(self):
        """central_value.py:236-260.  Returns the mean loss as a 0-dim device tensor (one host read
        per epoch instead of the reference's `.item()` per minibatch)."""
        self.train()
        self._row_index = 0
        count = 0
        for _ in range(self.mini_epoch):
            if self.config.get('freeze_critic', False):
                break
            for i in range(len(self.dataset)):
                self.train_critic(self.dataset[i])
                count += 1
            if self.normalize_input:
                self.model.running_mean_std.eval()
        total = self._rows[:count, 5].sum() if count else torch.zeros((), device=self.ppo_device)
        avg_loss = total / (self.mini_epoch * self.num_minibatches)
        self.epoch_num += 1
        self.lr, _ = self.scheduler.update(self.lr, 0, self.epoch_num, self.frame, 0)
        self.update_lr(self.lr)
        self.frame += self.batch_size
        if self._guard is not None and not self._guard_shared:
            self._range_verdict()
        if self.writter is not None:
            self.writter.add_scalar('losses/cval_loss', avg_loss.item(), self.frame)
            self.writter.add_scalar('info/cval_lr', self.lr, self.frame)
        return avg_loss

    def calc_gradients(self, batch):
        """central_value.py:278-335: forward, fused value loss + gradient, backward, (all-reduce,)
        clip, Adam.  Returns the minibatch loss (0-dim device tensor)."""
        opt = self.optimizer
        obs_batch = self._preproc_obs(batch['obs'])
        rnn_masks = batch.get('rnn_masks')
        opt.zero_grad()
        eng = self._engine
        reng = self._rnn_engine if obs_batch.dtype == torch.float32 else None
        mask, mask_sum = ops.sequence_mask(rnn_masks)
        row = self._rows[self._row_index % self._rows.shape[0]]
        self._row_index += 1
        if reng is not None:
            # the same normaliser update, then trunk + gate-input product, the sequence kernel, (layer norm,) and the
            # value tail: head, loss, d values, the gradient of the recurrent features and the head's gradient partials
            mb = obs_batch.shape[0]
            train_forward(reng, self.model.running_mean_std if self.normalize_input else None, obs_batch,
                          batch['rnn_states'], batch['dones'], self.seq_length,
                          value_loss=(batch['old_values'].reshape(-1).contiguous(), batch['returns'].reshape(-1).contiguous(),
                                      mask, mask_sum, self.e_clip, self.clip_value))
            ops.ppo_loss_finalize(reng.loss_partials, reng.loss_blocks, 0, mb, mask is not None, 2.0, 0.0, 0.0,
                                  row, self._no_logstd)
            reng.backward()
            return self._all_reduce_and_step(row)
        if eng is not None:
            # models.py:54-56 (norm_obs: training mode updates the statistics first), then the whole network in one launch
            rms, eps = launch_stats(self.model.running_mean_std if self.normalize_input else None, obs_batch)
            values = eng.forward(obs_batch, rms, eps)                       # [mb, 1]
        else:
            rnn = None
            if self.is_rnn:                                                 # central_value.py:300-307
                rnn = {'rnn_states': batch['rnn_states'], 'seq_length': self.seq_length, 'dones': batch['dones']}
            values = self.model.forward_values(obs_batch, rnn)              # [mb, V], autograd graph
        mb = values.shape[0]
        if values.shape[1] != 1:
            # value_size > 1: the loss kernel carries one value column - calc_loss as torch ops (common_losses.py:16-29,
            # torch_ext.apply_masks: masked, the sum over every column of the valid rows over the number of valid rows)
            old, ret = batch['old_values'].reshape(values.shape), batch['returns'].reshape(values.shape)
            if self.clip_value:
                clipped = old + (values - old).clamp(-self.e_clip, self.e_clip)
                c = torch.max((values - ret) ** 2, (clipped - ret) ** 2)
            else:
                c = (ret - values) ** 2
            loss = c.mean() if mask is None else (c * mask.view(-1, 1)).sum() / mask_sum.clamp(min=1.0)[0]
            loss.backward()
            row.zero_()
            row[1] = row[5] = loss.detach()
            return self._all_reduce_and_step(row)
        d_val = self._d_val[:mb] if eng is None else eng.d_heads[:mb].view(-1)
        with torch.no_grad():
            ops.value_loss(values.detach().reshape(-1), batch['old_values'].reshape(-1).contiguous(),
                           batch['returns'].reshape(-1).contiguous(), d_val, self._partials, self.e_clip,
                           self.clip_value, mask, mask_sum)
            ops.ppo_loss_finalize(self._partials, (mb + 255) // 256, 0, mb, mask is not None, 2.0, 0.0, 0.0,
                                  row, self._no_logstd)
        if eng is not None:
            eng.backward()
        else:
            torch.autograd.backward([values], [d_val.view(mb, 1)])
        return self._all_reduce_and_step(row)

    def _all_reduce_and_step(self, row):
        opt = self.optimizer
        if self.multi_gpu:
            rdist.all_reduce_sum(opt.flat_grads)
        scale = 1.0 / self.world_size if self.multi_gpu else 1.0
        opt.step(grad_scale=scale, max_norm=self.grad_norm if self.truncate_grads else None)
        return row[5]
