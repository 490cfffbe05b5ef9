"""Discrete-action PPO agent on MI355X - host mirror of `DiscreteA2CAgent`
(rl_games/algos_torch/a2c_discrete.py:13-209 over `DiscreteA2CBase`,
rl_games/common/a2c_common.py:1204-1359), BASELINE.json config #1 (CartPole-shaped).

Shares the rollout / GAE / dataset-preparation / optimiser path with `A2CAgent`; what differs:
  * `Discrete` or `Tuple`-of-`Discrete` (multi-discrete) action spaces, int64 actions, update_list
    without mus/sigmas, optional action masks from `vec_env.get_action_masks()` with
    CategoricalMasked semantics (a2c_common.py:995-997,1224-1229; a2c_discrete.py:92-114);
  * the minibatch loss is the categorical one, a single fused HIP kernel
    (csrc/ppo_loss.hip `ppo_loss_discrete_kernel`) that emits d loss/d logits and d loss/d value;
  * the network around it runs on the fused chain kernels of the continuous hot path - feed-forward ones on one or two
    chain_net.ChainNet (`_chains`), recurrent ones on chain_net.RecurrentChainNet (`_rnn_engine`) - or keeps autograd
    around the loss kernel: actor_paths.py chooses, DESIGN.md 4.1a has each path's conditions;
  * the rollout runs on the same engines (`fused_rollout`, _policy_step_kernels): the path's inference forward, the
    Exp(1) draws of Categorical.sample(), and one launch of the categorical head (csrc/rollout_categorical.hip) that
    samples, scores and writes the step into the buffer - replayed as one HIP graph per step index like the continuous
    agent's rollout;
  * the lr schedule is stepped once per mini-epoch on the mean KL (a2c_common.py:1271-1278),
    whatever `schedule_type` says, and `train_epoch` returns the 10-tuple without bound losses.
"""
import torch

from . import ops
from .agent import A2CAgent


def draw_exp_noise(noise, rows, branch_sizes):
    """The Exp(1) draws of Categorical.sample() (multinomial's one-sample path) into the flat `noise`: one exponential_
    per branch, in branch order, on its contiguous [rows, n_b] block.  Every categorical head of the package draws here -
    agents and players consume the generator alike."""
    at = 0
    for size in branch_sizes:
        noise[at:at + rows * size].view(rows, size).exponential_()
        at += rows * size


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

    def _alloc_rollout_scratch(self, rows, dev):
        # Exp(1) draws, branch b as a contiguous [rows, n_b] block (the tensor Categorical.sample() draws into)
        self._roll_noise = torch.empty(rows * sum(self.branch_sizes), dtype=torch.float32, device=dev)
        self._roll_actions = torch.empty((rows, len(self.branch_sizes)) if self.is_multi_discrete else (rows,),
                                         dtype=torch.int64, device=dev)
        self._roll_values = torch.empty(rows, dtype=torch.float32, device=dev)

    def _fast_policy_step(self, n):
        """The step's action masks go into the buffer slot first (the head kernel reads them there); observations that
        are not fp32 after preprocessing take the torch path for this step, as the update does."""
        masks = None
        if self.use_action_masks:                                # a2c_common.py:995-997
            masks = torch.as_tensor(self.vec_env.get_action_masks(), dtype=torch.bool, device=self.ppo_device)
        if not self._path.takes(self.obs['obs']):
            res = (self.get_action_values(self.obs) if masks is None
                   else self.get_masked_action_values(self.obs, masks))
            self._store_torch_step(n, res)
            return res
        if masks is not None:
            self.experience_buffer.store_step(n, {'action_masks': masks.contiguous()})
        return super()._fast_policy_step(n)

    def _draw_exp_noise(self, rows):
        draw_exp_noise(self._roll_noise, rows, self.branch_sizes)

    _draw_value_noise = _draw_exp_noise     # (get_values runs the model's whole eval forward, which samples actions)

    def _sample_step(self, n, heads, value):
        """Exp(1) draws -> categorical head (actions / neglogpacs / values into the buffer).  heads: the path's (logits,
        value); `value` - a central value network's - replaces the latter."""
        logits, own_value = heads
        cv = value is not None
        self._draw_exp_noise(logits.shape[0])
        vs, eps = self._rollout_value_stats()
        buf = self.experience_buffer
        masks = buf.storage['action_masks'][:, n] if self.use_action_masks else None
        ops.rollout_categorical_head(logits, value if cv else own_value, self.branch_sizes, self._roll_noise, masks, vs,
                                     eps, self._roll_actions, self._roll_values, buf.storage, self.horizon_length, n,
                                     value_repeat=self.num_agents if cv else 1)

    def _alloc_loss_scratch(self, mb, dev):
        self._d_policy = torch.empty(mb, sum(self.branch_sizes), dtype=torch.float32, device=dev)
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
        action_masks = torch.as_tensor(action_masks, dtype=torch.bool, device=self.ppo_device)
        self.model.eval()
        with torch.no_grad():
            res_dict = self.model(self._eval_batch(obs, action_masks=action_masks))
            if self.has_central_value:
                res_dict['values'] = self.get_central_value({'is_train': False, 'states': obs['states']})
        res_dict['action_masks'] = action_masks
        return res_dict

    def preprocess_actions(self, actions):
        """a2c_common.py:736-739 - discrete actions go to the env as they are."""
        if not self.is_tensor_obses:
            actions = actions.cpu().numpy()
        return actions

    @torch.no_grad()
    def _loss_launches(self, input_dict, row, logits, values, d_logits, d_values):
        """The categorical loss launch (d logits / d value, per-block partials) and its finalise launch."""
        mb = logits.shape[0]
        mask, mask_sum = ops.sequence_mask(input_dict.get('rnn_masks', None))
        coef_c = self._loss_scalars()[0]
        lg = logits.detach()
        ops.ppo_loss_discrete(lg if lg.stride(1) == 1 else lg.contiguous(), values, input_dict['actions'],
                              input_dict['old_logp_actions'], input_dict['advantages'],
                              input_dict['old_values'].reshape(-1), input_dict['returns'].reshape(-1), d_logits, d_values,
                              self._loss_partials, self.e_clip, coef_c, self.entropy_coef, self.clip_value, self.surrogate,
                              mask, mask_sum, branch_sizes=self.branch_sizes, action_masks=input_dict.get('action_masks'),
                              new_neglogp=None if self._diag_nlp is None else self._diag_nlp[:mb])
        ops.ppo_loss_finalize(self._loss_partials, ops.ppo_loss_discrete_blocks(mb), 0, mb, mask is not None, coef_c,
                              self.entropy_coef, 0.0, row, self._no_logstd, self.optimizer.kl_slot)

    def _diag_update(self, input_dict, logits):
        if self._diag_nlp is not None:
            self._diag_minibatch(input_dict, new_neglogp=self._diag_nlp[:logits.shape[0]])

    def train_epoch(self):
        """a2c_common.py:1232-1289: (step_time, play_time, update_time, total_time, a_losses,
        c_losses, entropies, kls, last_lr, lr_mul)."""
        res = super().train_epoch()
        return res[:6] + res[7:]
