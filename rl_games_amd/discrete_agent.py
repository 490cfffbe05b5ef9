"""Discrete-action PPO agent on MI355X - host mirror of `DiscreteA2CAgent`
(rl_games/algos_torch/a2c_discrete.py:13-209 over `DiscreteA2CBase`,
rl_games/common/a2c_common.py:1204-1359), BASELINE.json config #1 (CartPole-shaped).

Shares the rollout / GAE / dataset-preparation / optimiser path with `A2CAgent`; what differs:
  * `Discrete` or `Tuple`-of-`Discrete` (multi-discrete) action spaces, int64 actions, update_list
    without mus/sigmas, optional action masks from `vec_env.get_action_masks()` with
    CategoricalMasked semantics (a2c_common.py:995-997,1224-1229; a2c_discrete.py:92-114);
  * the minibatch loss is the categorical one, a single fused HIP kernel
    (csrc/ppo_loss.hip `ppo_loss_discrete_kernel`) that emits d loss/d logits and d loss/d value;
  * the network around it runs on the fused chain kernels of the continuous hot path (chain_net.ChainNet: observation
    normaliser + trunk + heads as one forward launch, one backward launch, MFMA weight gradients) - one chain over
    [value | logits] behind a shared trunk, one chain per trunk with `separate: True` (ppo_cartpole.yaml:17) - where the
    network has that form (plain Linear + ELU / ReLU / tanh trunks, widths that are multiples of 4, value_size 1);
    anything else, or `fused_mlp: False`, keeps autograd around the loss kernel (`torch.autograd.backward` on the heads);
  * recurrent networks of the reference's SMAC shape (one shared trunk, one LSTM / GRU layer of 16 / 32 / 64 / 128 units
    behind it, optionally a layer norm behind the RNN) run update and rollout on chain_net.RecurrentChainNet
    (`_rnn_engine`; `manual_lstm: False` keeps them on torch modules);
  * the rollout runs on the same chains (`fused_rollout`, _policy_step_kernels): each chain's inference forward, the
    Exp(1) draws of Categorical.sample(), and one launch of the categorical head (csrc/rollout_categorical.hip) that
    samples, scores and writes the step into the buffer - replayed as one HIP graph per step index like the continuous
    agent's rollout;
  * the lr schedule is stepped once per mini-epoch on the mean KL (a2c_common.py:1271-1278),
    whatever `schedule_type` says, and `train_epoch` returns the 10-tuple without bound losses.
"""
import torch

from torch import nn

from . import ops
from .agent import A2CAgent
from .chain_net import ChainNet, RecurrentChainNet, arena_layout, rnn_cell_declined
from .normalizers import launch_stats
from .weight_forms import _ChainForms


class DiscreteA2CAgent(A2CAgent):
    def _init_action_space(self, config):
        """DiscreteA2CBase.__init__ (a2c_common.py:1206-1222)."""
        action_space = self.env_info['action_space']
        kind = type(action_space).__name__
        rows = self.num_agents * self.num_actors
        if kind == 'Discrete':
            self.actions_shape = (self.horizon_length, rows)
            self.actions_num = int(action_space.n)
            self.branch_sizes = [self.actions_num]
            self.is_multi_discrete = False
        elif kind == 'Tuple':
            self.actions_shape = (self.horizon_length, rows, len(action_space))
            self.actions_num = [int(a.n) for a in action_space]
            self.branch_sizes = list(self.actions_num)
            self.is_multi_discrete = True
        else:
            raise ValueError(f'Unsupported action space type for DiscreteA2CBase: {type(action_space)}')
        self.is_discrete = True
        self.bounds_loss_coef = None
        self.clip_actions = False
        # the reference's discrete train_epoch has no per-minibatch scheduling: it always updates
        # the lr once per mini-epoch with the mean KL - the base class's 'standard' schedule
        self.schedule_type = 'standard'

    def _supports_action_masks(self):
        return True

    def _chain_heads(self):
        """Head groups of the network, one per chain: [[value, logits...]] behind a shared trunk, [[logits...], [value]]
        for separate actor / critic trunks."""
        net = self.model.a2c_network
        logits = list(net.logits) if net.is_multi_discrete else [net.logits]
        return [logits, [net.value]] if net.is_separate_critic() else [[net.value] + logits]

    def _recurrent_engine_declined(self, config):
        """Why a recurrent network stays off chain_net.RecurrentChainNet (None: it is eligible): one shared trunk of
        Linear + activation pairs, one LSTM / GRU layer of a supported width plainly behind it (a layer norm behind the
        RNN is fine), and `manual_lstm` - recurrent policies through this library's kernels - not switched off."""
        net = self.model.a2c_network
        if not config.get('manual_lstm', True):
            return 'manual_lstm is off'
        if not getattr(net, 'plain_trunk_rnn_ln', False) or net.is_separate_critic():
            return 'plain Linear + activation trunks only'
        return rnn_cell_declined(net.rnn_name, net.rnn_layers, net.rnn_units)

    def _arena_layout(self, config):
        if not config.get('fused_mlp', True):
            return None
        net = self.model.a2c_network
        rest = [p for p in self.model.parameters() if all(p is not q for q in net.parameters())]
        first = ()
        if net.is_rnn() and self._recurrent_engine_declined(config) is None:
            first = [m.bias for m in net.actor_mlp if isinstance(m, nn.Linear)]      # (RecurrentChainNet's trunk)
        return arena_layout(list(net.parameters()), self._chain_heads(), first_vectors=first) + rest

    def _init_chains(self, config):
        """Feed-forward networks: `_chains`, one ChainNet per trunk.  Recurrent ones: `_rnn_engine`, a RecurrentChainNet
        over the shared trunk ([value | logits] heads); `_chains` stays None for them."""
        self._chains = None
        self._rnn_engine = None
        net = self.model.a2c_network
        if not config.get('fused_mlp', True):
            return
        try:
            if self.value_size != 1 or not isinstance(net.value_act, nn.Identity):
                raise NotImplementedError('one linear value column only')
            rows = self.minibatch_size
            groups = self._chain_heads()
            roll = self.num_actors * self.num_agents
            if net.is_rnn():
                why = self._recurrent_engine_declined(config)
                if why is not None:
                    raise NotImplementedError(why)
                self._rnn_engine = RecurrentChainNet(net.actor_mlp, net.rnn.rnn, net.layer_norm if net.rnn_ln else None,
                                                     groups[0], self.optimizer, rows, infer_rows=roll)
                return
            if not getattr(net, 'plain_trunk', True):
                raise NotImplementedError('plain Linear + activation trunks only')
            trunks = [net.actor_mlp, net.critic_mlp] if net.is_separate_critic() else [net.actor_mlp]
            self._chains = [ChainNet(t, g, self.optimizer, rows, infer_rows=roll) for t, g in zip(trunks, groups)]
        except NotImplementedError as e:
            print(f'rl_games_amd: discrete network outside the fused chain kernels ({e}); using autograd')
            self._chains = self._rnn_engine = None

    def _graph_chains(self):
        """... and the recurrent engine's trunk chain: a replayed step graph reads its fragments / planes."""
        forms = super()._graph_chains()
        if self._rnn_engine is not None:
            roll = self.num_actors * self.num_agents
            forms.append(_ChainForms(self._rnn_engine.chain, ((roll, 0),), self.optimizer.flat_params))
        return forms

    # ------------------------------------------------------------------ fused rollout
    def _fused_rollout_network_ok(self):
        """A feed-forward network on the chains or a recurrent one on its engine, of at most
        ops.CATEGORICAL_MAX_BRANCHES action branches."""
        on_kernels = self._rnn_engine is not None if self.is_rnn else self._chains is not None
        return on_kernels and len(self.branch_sizes) <= ops.CATEGORICAL_MAX_BRANCHES

    def init_tensors(self):
        super().init_tensors()
        if self._fast_rollout_ok():
            rows, dev = self.num_actors * self.num_agents, self.ppo_device
            # Exp(1) draws, branch b as a contiguous [rows, n_b] block (the tensor Categorical.sample() draws into)
            self._roll_noise = torch.empty(rows * sum(self.branch_sizes), dtype=torch.float32, device=dev)
            self._roll_actions = torch.empty((rows, len(self.branch_sizes)) if self.is_multi_discrete else (rows,),
                                             dtype=torch.int64, device=dev)
            self._roll_values = torch.empty(rows, dtype=torch.float32, device=dev)

    @staticmethod
    def _fp32_after_preproc(obs):
        return obs.dtype in (torch.float32, torch.uint8)         # (_preproc_obs: uint8 / 255 -> fp32)

    def _fast_policy_step(self, n):
        """The step's action masks go into the buffer slot first (the head kernel reads them there); observations that
        are not fp32 after preprocessing take the torch path for this step, as the update does."""
        masks = None
        if self.use_action_masks:                                # a2c_common.py:995-997
            masks = torch.as_tensor(self.vec_env.get_action_masks(), dtype=torch.bool, device=self.ppo_device)
        if not self._fp32_after_preproc(self.obs['obs']):
            res = (self.get_action_values(self.obs) if masks is None
                   else self.get_masked_action_values(self.obs, masks))
            self._store_torch_step(n, res)
            return res
        if masks is not None:
            self.experience_buffer.store_step(n, {'action_masks': masks.contiguous()})
        return super()._fast_policy_step(n)

    def _chain_heads_of(self, obs, logits_only=False, rnn_states=None):
        """(logits [N, sum(sizes)], value [N, 1]) of fp32 observations (any row stride): each chain's inference
        forward, the observation normaliser in eval mode inside the launch.  logits_only (a central value network
        supplies the values): the separate critic trunk does not run, value is None.  Recurrent policies: the engine's
        T = 1 forward on `rnn_states` - the states arrive zeroed where an episode ended (play_steps_rnn), as for the
        model's eval forward, which takes no done flags (a2c_common.py:590) - leaving the next ones in its last_states."""
        if obs.stride(-1) != 1:
            obs = obs.contiguous()
        if self._rnn_engine is not None:                         # [value | logits]
            heads = self._rnn_engine.forward(obs, self._obs_rms(), self._obs_eps(), rnn_states, None, 1, keep=False)
            return heads[:, 1:], heads[:, :1]
        chains = self._chains[:1] if logits_only else self._chains
        heads = [c.infer(obs, self._obs_rms(), self._obs_eps()) for c in chains]
        if len(self._chains) == 1:                               # [value | logits]
            return heads[0][:, 1:], heads[0][:, :1]
        return heads[0], (None if logits_only else heads[1])

    def _draw_exp_noise(self, rows):
        """The Exp(1) draws of Categorical.sample() (multinomial's one-sample path): one exponential_ per branch, in
        branch order, on a contiguous [rows, n_b] block."""
        at = 0
        for size in self.branch_sizes:
            self._roll_noise[at:at + rows * size].view(rows, size).exponential_()
            at += rows * size

    def _policy_step_kernels(self, n, obs_raw, dones, rnn_states, store=True, states=None, cv_rnn_states=None):
        """Chain forward(s) -> (central value: the critic's chain forward on `states`) -> Exp(1) draws -> categorical
        head (actions / neglogpacs / values into the buffer) -> obs + dones (+ states) into the buffer.  Same maths and
        the same generator use as get_(masked_)action_values + update_data; no host read, so the step can be captured."""
        buf = self.experience_buffer
        cv = self.has_central_value
        logits, value = self._chain_heads_of(self._preproc_obs(obs_raw), logits_only=cv, rnn_states=rnn_states)
        if cv:
            value = self._critic_infer(states, cv_rnn_states)
        rows = logits.shape[0]
        self._draw_exp_noise(rows)
        vs, eps = self._rollout_value_stats()
        masks = buf.storage['action_masks'][:, n] if self.use_action_masks else None
        ops.rollout_categorical_head(logits, value, self.branch_sizes, self._roll_noise, masks, vs, eps,
                                     self._roll_actions, self._roll_values, buf.storage, self.horizon_length, n,
                                     value_repeat=self.num_agents if cv else 1)
        if store:
            self._store_step_inputs(n, obs_raw, dones, states)
        res = {'actions': self._roll_actions, 'values': self._roll_values.view(rows, 1)}
        if self._rnn_engine is not None:
            res['rnn_states'] = self._rnn_engine.last_states
        if self._critic_rnn_engine() is not None:
            res['cv_rnn_states'] = self._critic_rnn_engine().last_states
        return res

    def _fast_values(self, obs):
        """get_values on the chains: the critic column, de-normalised."""
        if self.has_central_value:
            return self._central_fast_values(obs['states'])     # (the critic only: no actor forward, no draws)
        x = obs['obs']
        if not self._fp32_after_preproc(x):
            return self.get_values(obs)
        x = self._preproc_obs(x)
        if x.stride(-1) != 1:
            x = x.contiguous()
        if self._rnn_engine is not None:
            # the same forward as a rollout step; the states it leaves are dropped
            v = self._chain_heads_of(x, rnn_states=self.rnn_states)[1].contiguous()
        else:
            # the critic is column 0 of the last chain's heads ([value | logits], or the critic trunk's [value])
            v = self._chains[-1].infer(x, self._obs_rms(), self._obs_eps())[:, :1].contiguous()
        # get_values runs the model's whole eval forward, which samples actions: the same draws keep the generator where
        # the torch path leaves it
        self._draw_exp_noise(x.shape[0])
        return self._denorm_values(v).view(-1)

    def _alloc_loss_scratch(self, mb, dev):
        self._d_logits = torch.empty(mb, sum(self.branch_sizes), dtype=torch.float32, device=dev)
        self._d_val = torch.empty(mb, dtype=torch.float32, device=dev)
        self._loss_blocks = ops.ppo_loss_discrete_blocks(mb)
        self._loss_partials = torch.empty(self._loss_blocks, ops.ppo_loss_partials_per_block(0),
                                          dtype=torch.float64, device=dev)
        self._no_logstd = torch.zeros(1, dtype=torch.float32, device=dev)
        # each row's neglogp out of the loss launch, for the diagnostics (only allocated when they are on)
        self._diag_nlp = (torch.empty(mb, dtype=torch.float32, device=dev) if self.use_diagnostics and self.global_rank == 0
                          else None)

    def _rollout_fields(self):
        fields = ['actions', 'neglogpacs', 'values']               # a2c_common.py:1224-1229
        return fields + ['action_masks'] if self.use_action_masks else fields

    def get_masked_action_values(self, obs, action_masks):
        """a2c_discrete.py:92-114.  action_masks: bool [rows, sum(head sizes)] (numpy or tensor)."""
        processed_obs = self._preproc_obs(obs['obs'])
        action_masks = torch.as_tensor(action_masks, dtype=torch.bool, device=self.ppo_device)
        self.model.eval()
        with torch.no_grad():
            res_dict = self.model({'is_train': False, 'prev_actions': None, 'obs': processed_obs,
                                   'action_masks': action_masks, 'rnn_states': self.rnn_states})
            if self.has_central_value:
                res_dict['values'] = self.get_central_value({'is_train': False, 'states': obs['states']})
        res_dict['action_masks'] = action_masks
        return res_dict

    def preprocess_actions(self, actions):
        """a2c_common.py:736-739 - discrete actions go to the env as they are."""
        if not self.is_tensor_obses:
            actions = actions.cpu().numpy()
        return actions

    def calc_gradients(self, input_dict):
        """a2c_discrete.py:121-209."""
        row = self._mb_scalars[self._mb_index % self._mb_scalars.shape[0]]
        self._mb_index += 1
        self._forward_loss_backward(input_dict, row)
        self.trancate_gradients_and_step()
        # (a central value network without `use_experimental_cv`: no actor value loss, a2c_discrete.py:164-167)
        c_loss = row[1] if self.has_value_loss else torch.zeros((), device=row.device)
        self.train_result = (row[0], c_loss, row[2], row[4], self._host_lr, 1.0)

    def _forward_loss_backward(self, input_dict, row):
        opt = self.optimizer
        obs_batch = self._preproc_obs(input_dict['obs'])
        rnn_masks = input_dict.get('rnn_masks', None)
        opt.zero_grad()
        chains = self._chains if obs_batch.dtype == torch.float32 else None
        rnn_eng = self._rnn_engine if obs_batch.dtype == torch.float32 else None
        if rnn_eng is not None:
            # the same normaliser update, then trunk + gate-input product, the sequence kernel, (layer norm,) heads
            rms, eps = launch_stats(self.model.running_mean_std if self.normalize_input else None, obs_batch)
            mb = obs_batch.shape[0]
            heads = rnn_eng.forward(obs_batch, rms, eps, input_dict['rnn_states'],
                                    input_dict['dones'] if self.zero_rnn_on_done else None, self.seq_length, keep=True)
            logits, values = heads[:, 1:], heads[:, 0]           # [value | logits]
            d_logits, d_val = rnn_eng.d_heads[:mb, 1:], rnn_eng.d_heads[:mb, 0]
        elif chains is not None:
            # models.py:54-56 (norm_obs: training mode updates the statistics first), then each trunk + its heads as
            # one launch that normalises on the way in
            rms, eps = launch_stats(self.model.running_mean_std if self.normalize_input else None, obs_batch)
            outs = [c.forward(obs_batch, rms, eps) for c in chains]
            mb = obs_batch.shape[0]
            if len(chains) == 1:                                   # [value | logits]
                logits, values = outs[0][:, 1:], outs[0][:, 0]
                d_logits, d_val = chains[0].d_heads[:mb, 1:], chains[0].d_heads[:mb, 0]
            else:
                logits, values = outs[0], outs[1][:, 0]
                d_logits, d_val = chains[0].d_heads[:mb], chains[1].d_heads[:mb, 0]
        else:
            batch = {'is_train': True, 'obs': obs_batch}
            if self.is_rnn:                                        # a2c_discrete.py:138-144
                batch.update(rnn_states=input_dict['rnn_states'], seq_length=self.seq_length)
                if self.zero_rnn_on_done:
                    batch['dones'] = input_dict['dones']
            logits, values = self.model.forward_heads(batch)
            mb = logits.shape[0]
            d_logits, d_val = self._d_logits[:mb], self._d_val[:mb]
        mask, mask_sum = ops.sequence_mask(rnn_masks)
        with torch.no_grad():
            lg = logits.detach()
            ops.ppo_loss_discrete(lg if lg.stride(1) == 1 else lg.contiguous(), values.detach().reshape(-1),
                                  input_dict['actions'], input_dict['old_logp_actions'],
                                  input_dict['advantages'], input_dict['old_values'].reshape(-1),
                                  input_dict['returns'].reshape(-1), d_logits, d_val, self._loss_partials,
                                  self.e_clip, self.critic_coef if self.has_value_loss else 0.0,
                                  self.entropy_coef, self.clip_value, self.surrogate, mask, mask_sum,
                                  branch_sizes=self.branch_sizes, action_masks=input_dict.get('action_masks'),
                                  new_neglogp=None if self._diag_nlp is None else self._diag_nlp[:mb])
            ops.ppo_loss_finalize(self._loss_partials, ops.ppo_loss_discrete_blocks(mb), 0, mb,
                                  mask is not None, self.critic_coef if self.has_value_loss else 0.0,
                                  self.entropy_coef, 0.0, row,
                                  self._no_logstd, opt.kl_slot)
        if rnn_eng is not None:
            rnn_eng.backward()
        elif chains is not None:
            for c in chains:
                c.backward()
        else:
            torch.autograd.backward([logits, values], [d_logits, d_val.view(mb, 1)])
        if self._diag_nlp is not None:
            self._diag_minibatch(input_dict, new_neglogp=self._diag_nlp[:mb])

    def train_epoch(self):
        """a2c_common.py:1232-1289: (step_time, play_time, update_time, total_time, a_losses,
        c_losses, entropies, kls, last_lr, lr_mul)."""
        res = super().train_epoch()
        return res[:6] + res[7:]
