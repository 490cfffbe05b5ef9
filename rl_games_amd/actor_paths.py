"""Which engine runs an agent's network: one object per way of running the actor, chosen once when the agent is built
- engine, pair, chains, recurrent, autograd or general; the table with each path's conditions: DESIGN.md 4.1a.
The choice has two phases, because the arena layout must exist before FlatAdam and the engine after it: a Plan holds the
path's class, the layout and the reason a faster path was declined; Plan.build makes the path once the optimiser exists.
A path answers what the agents need to know about their network: the engines that finish weight gradients, the chains
captured graphs read, whether it takes an observation tensor, whether the rollout can run fused, the rollout's inference
forward and where the next RNN states are, and the update's forward / loss / backward of one minibatch.
"""
import numpy as np
import torch
from torch import nn

from . import ops
from .chain_net import ChainNet, RecurrentChainNet, RecurrentChainPair, arena_layout, rnn_cell_declined
from .mlp_engine import ManualMLP
from .normalizers import launch_stats
from .weight_forms import _ChainForms


def train_forward(engine, normaliser, obs, rnn_states, dones, seq_length, **kw):
    """The normaliser's statistics first (models.py:54-56: a module in training mode folds the batch in), then the
    training forward of a RecurrentChainNet / RecurrentChainPair, which normalises on the way in."""
    rms, eps = launch_stats(normaliser, obs)
    return engine.forward(obs, rms, eps, rnn_states, dones, seq_length, keep=True, **kw)


def fp32_space(space):
    dtype = getattr(space, 'dtype', None)
    return dtype is not None and np.dtype(dtype) == np.float32


def _unit_stride(obs):
    return obs if obs.stride(-1) == 1 else obs.contiguous()


def _value_and_rest(heads):
    """[value | logits] or [value | mu] head rows -> (the rest [rows, n], value [rows, 1])."""
    return heads[:, 1:], heads[:, :1]


def chain_heads(net):
    """Head groups of a discrete network, one per chain: [[value, logits...]] behind a shared trunk, [[logits...],
    [value]] for separate actor / critic trunks."""
    logits = list(net.logits) if net.is_multi_discrete else [net.logits]
    return [logits, [net.value]] if net.is_separate_critic() else [[net.value] + logits]


class AutogradPath:
    """Torch modules between the fused loss kernels, and the base of every other path: update() is the one statement of
    zero_grad -> train_forward -> the agent's loss launches -> backward."""
    kind = 'autograd'
    engine = pair = chains = recurrent = None      # what A2CAgent._engine / _rnn_pair / _chains / _rnn_engine show
    fused_chain = None                             # the one chain that runs a whole feed-forward actor (engine path)
    graphs = grads_overwritten = False             # the update may be captured / writes every gradient slot itself
    engines = ()                                   # the engines that finish weight gradients (chain_net.WeightGrads)
    rollout_ok = False                             # the rollout can run fused (for the agent's observation space)
    last_states = None                             # the next RNN states behind infer()
    norm_ok = None                                 # the finalise launch leaves the gradient norm (EnginePath)

    def __init__(self, agent):
        self.agent = agent

    def chain_forms(self):
        """The fused chains the agent's captured graphs read (_ChainForms), in the order their forms are brought up to
        date.  Updates that stay eager: the rollout's inference forward on each engine's chain alone."""
        a = self.agent
        return [_ChainForms(e.chain, ((a.num_actors * a.num_agents, 0),), a.optimizer.flat_params) for e in self.engines]

    def takes(self, obs):
        """Does this path run on the observation tensor as the env / the dataset delivers it (else: the autograd path)."""
        return True

    def _stats_module(self):
        return self.agent.model.running_mean_std if self.agent.normalize_input else None

    def update(self, inp, row):
        a = self.agent
        obs = a._preproc_obs(inp['obs'])
        a.optimizer.zero_grad()
        policy, values, d_policy, d_values = self.train_forward(obs, inp)
        a._loss_launches(inp, row, policy, values, d_policy, d_values)
        self.backward()
        a._norm_ready = None
        a._diag_update(inp, policy)

    def train_forward(self, obs, inp):
        """-> (policy, values [mb], d_policy, d_values [mb]): what the agent's loss launches read and write - policy is
        (mu, log sigma) or the logits."""
        a = self.agent
        out = a.model.forward_heads(a._torch_batch(inp, obs))
        head, values = (out[0], out[1]) if a.is_discrete else (out[0], out[2])
        mb = head.shape[0]
        self._outputs = (head, values, a._d_policy[:mb], a._d_val[:mb])
        return (head if a.is_discrete else out[:2]), values.detach().reshape(-1), a._d_policy[:mb], a._d_val[:mb]

    def backward(self):
        head, values, d_head, d_values = self._outputs
        torch.autograd.backward([head, values], [d_head, d_values.view(-1, 1)])


class GeneralPath(AutogradPath):
    """value_size > 1 (the fused loss kernels carry one value column), a state-dependent sigma head (fixed_sigma False:
    the kernels carry log sigma as a parameter vector) or a sigma that is not exp of an unbounded log sigma (logstd_bounds,
    min_sigma, softplus / linear forms): forward with autograd, the losses as torch ops (torch_fallback.py:
    a2c_continuous.py:97-134, :173-221), loss.backward() into the arena views."""
    kind = 'general'

    def update(self, inp, row):
        """Leaves the same things behind as the fused paths: the five scalars in `row`, the KL in the arena's tail slot
        (the device-side lr rule and the multi-GPU average read it there), mu / sigma written back into the dataset."""
        from . import torch_fallback as tf
        a = self.agent
        opt, net = a.optimizer, a.model.a2c_network
        batch = a._torch_batch(inp, a._preproc_obs(inp['obs']))
        rnn_masks = inp.get('rnn_masks', None)
        mask = None if rnn_masks is None else rnn_masks.reshape(-1).float()
        coef_c, coef_b, kind = a._loss_scalars()
        opt.zero_grad()
        mu, logstd, values, _ = a.model.forward_heads(batch)
        mb = mu.shape[0]
        loss, scalars, sigma = tf.ppo_loss(
            mu, logstd, values.reshape(mb, -1), inp['actions'], inp['old_logp_actions'], inp['advantages'],
            inp['old_values'].reshape(mb, -1), inp['returns'].reshape(mb, -1), e_clip=a.e_clip, critic_coef=coef_c,
            entropy_coef=a.entropy_coef, bounds_coef=coef_b, bound_kind=kind, clip_value=a.clip_value, smooth=a.surrogate,
            mask=mask, sigma_fn=None if net.plain_sigma else net.sigma_and_logstd)
        loss.backward()
        with torch.no_grad():
            sig = sigma.detach().expand_as(mu)
            kl = tf.policy_kl(mu.detach(), sig, inp['mu'], inp['sigma'], mask)
            row[0], row[1], row[2], row[3], row[4] = (scalars['a_loss'], scalars['c_loss'], scalars['entropy'],
                                                      scalars['b_loss'], kl)
            opt.kl_slot.copy_(kl.reshape(1))
            inp['mu'].copy_(mu.detach())                                                # datasets.py:33-43
            inp['sigma'].copy_(sig)
            a._diag_minibatch(inp, new_neglogp=scalars['neglogp'])
        a._norm_ready = None


class EnginePath(AutogradPath):
    """The continuous agent's shared trunk on mlp_engine.ManualMLP: update and rollout without autograd.  The only path
    whose update is captured into HIP graphs, and (no parameter outside the network) whose launches overwrite every
    gradient slot, so that the per-step zero fill of the arena is skipped."""
    kind, graphs, rollout_ok = 'engine', True, True
    fused_chain = property(lambda self: self.engine.chain)
    last_states = property(lambda self: self.engine.last_states)

    def __init__(self, agent):
        super().__init__(agent)
        cfg, model = agent.config, agent.model
        self.engine = ManualMLP(model.a2c_network, agent.optimizer,
                                max(agent.minibatch_size, agent.num_actors * agent.num_agents),
                                mfma_dw=bool(cfg.get('mfma_dw', True)), inplace_act=bool(cfg.get('inplace_act', True)),
                                fused_chain=bool(cfg.get('fused_mlp', True)))
        self.engines = [self.engine]
        self.grads_overwritten = len(list(model.parameters())) == len(list(model.a2c_network.parameters()))
        self.norm_ok = self.norm_partials = None      # decided on first use (norm_in_finalize)

    def chain_forms(self):
        """The update's training forward (2) and backward (1), the rollout's inference forward (0)."""
        a, eng = self.agent, self.engine
        launches = ((a.minibatch_size, 2), (a.minibatch_size, 1), (a.num_actors * a.num_agents, 0))
        arena = a.optimizer.flat_params
        forms = []
        if eng.chain is not None:
            forms.append(_ChainForms(eng.chain, launches, arena, True, bool(a.config.get('adam_writes_planes', True))))
        if eng.chain_rnn is not None:
            forms.append(_ChainForms(eng.chain_rnn, launches, arena, True, False))
        return forms

    def _rnn_arguments(self, rnn_states, dones, seq_length):
        if not self.agent.is_rnn:
            return {}
        return dict(rnn_states=rnn_states, dones=dones, seq_length=seq_length)

    def infer(self, obs, rnn_states, logits_only=False):
        """Heads [rows, 1 + A] ([value | mu]) of preprocessed observations (any row stride on the fused chain: a buffer
        slot [:, n, :]), the normaliser in eval mode.  No autograd, no host read."""
        a, eng = self.agent, self.engine
        if not obs.is_contiguous() and (eng.chain is None or obs.stride(-1) != 1):
            obs = obs.contiguous()
        if eng.chain is not None:
            # normaliser + every layer + heads in one launch; nothing but the heads is written
            return eng.forward_obs(obs, a._obs_rms(), a._obs_eps(), keep=False)
        rnn = self._rnn_arguments(rnn_states, None, 1)
        if a.is_rnn and eng.chain_rnn is not None and obs.dtype == torch.float32:
            # recurrent policy: normaliser + trunk + gate-input product in one launch, then the LSTM step + heads
            return eng.forward(obs, keep=False, raw_rms=a._obs_rms() or (), eps=a._obs_eps(), **rnn)
        if a.normalize_input:
            m = a.model.running_mean_std
            obs = ops.rms_apply(obs, m.running_mean, m.running_var, m.epsilon, 0, out=a._roll_obs_norm)
        return eng.forward(obs, keep=False, **rnn)

    def values(self, obs, rnn_states):
        return self.infer(obs.contiguous(), rnn_states)[:, 0].contiguous().view(-1, 1)

    def norm_in_finalize(self):
        """The weight-gradient finalise launch may leave the gradient-norm partials (and advance the Adam
        step counter) when it writes EVERY gradient of the arena and nothing touches them before Adam."""
        if self.norm_ok is None:
            a, eng = self.agent, self.engine
            self.norm_ok = (not a.multi_gpu and eng.chain is not None and not a.is_rnn
                             and a.config.get('norm_in_finalize', True)
                             and eng.gradient_elements() == a.optimizer.numel)
            if self.norm_ok:
                # one entry per finalise workgroup: ~ one per 64 weights + the bias / loss blocks (MlpDwPlan.
                # finalize_blocks); a plan that still needs more falls back to grad_sumsq (chain_net.WeightGrads.finish)
                entries = max(1 << 15, eng.gradient_elements() // 64 + 8192)
                self.norm_partials = torch.zeros(entries, dtype=torch.float64, device=a.ppo_device)
        return self.norm_ok

    @torch.no_grad()
    def update(self, inp, row):
        """No host-side scalars change between calls for a given minibatch slice, so this body is what gets captured
        into a HIP graph per minibatch index."""
        a, eng = self.agent, self.engine
        opt, cfg, net = a.optimizer, a.config, a.model.a2c_network
        obs = a._preproc_obs(inp['obs'])
        if not self.grads_overwritten:
            opt.zero_grad()
        rnn = self._rnn_arguments(inp.get('rnn_states'), inp['dones'] if a.zero_rnn_on_done else None, a.seq_length)
        stats = self._stats_module()
        if eng.chain is not None:
            if not obs.is_contiguous():
                obs = obs.contiguous()
            rms, fold = a._obs_rms(), None
            if stats is not None and stats.training:
                if a._fold_index is not None:
                    # statistics first (models.py:54-56), in the launch's prologue, from the
                    # epoch's precomputed minibatch moments
                    rms, fold = stats.fold_buffers(a._fold_index)
                else:
                    stats.update(obs)
            # forward + loss + backward as ONE launch where the chain has that form (minibatches < 16,384 rows,
            # the loss evaluated by the backward launch): the forward is handed to eng.backward() below
            defer = (cfg.get('fused_step16', True) and cfg.get('fold_loss_finalize', True)
                     and cfg.get('loss_in_backward', True) and not eng.chain.split_products(obs.shape[0], 2))
            heads = eng.forward_obs(obs, rms, a._obs_eps(), rms_fold=fold, defer=defer)
        elif a.is_rnn and eng.chain_rnn is not None and obs.dtype == torch.float32:
            # recurrent policy on the fused trunk: the statistics update stays its own (two) launches, the
            # normalisation happens inside the trunk launch
            if not obs.is_contiguous():
                obs = obs.contiguous()
            rms, eps = launch_stats(stats, obs)
            heads = eng.forward(obs, raw_rms=rms or (), eps=eps, **rnn)
        else:
            if stats is not None:                                   # updates the obs statistics
                obs = stats(obs, out=a._obs_norm_mb[:obs.shape[0]])
            heads = eng.forward(obs, **rnn)
        mu, mb = eng.mu_view(heads), heads.shape[0]
        d_heads = eng.d_heads[:mb]
        args, fin = a._ppo_loss_setup(inp, mu, net.sigma, eng.values_view(heads).reshape(mb, -1)[:, 0],
                                      eng.mu_view(d_heads), eng.values_view(d_heads)[:, 0])
        fold = cfg.get('fold_loss_finalize', True)
        if fold and eng.chain is not None and cfg.get('loss_in_backward', True):
            # On the fused chain the backward launch evaluates the loss of its own row tiles first (no loss
            # launch; one partial row per backward workgroup).
            blocks, ppo = eng.chain.num_blocks(mb, 1), ops.ppo_loss_desc(*args)
        else:
            blocks, ppo = ops.ppo_loss_blocks(mb), None
            ops.ppo_loss_fused(*args)
        fin = fin(blocks, row, eng.net.mu.bias.grad, eng.net.value.bias.grad)
        if fold:
            # the loss partials are folded by the weight-gradient finalise launch (one launch less),
            # and - single GPU, every gradient of the arena written by that launch - the sums of
            # squares for clip_grad_norm_ with them (another one)
            norm = (self.norm_partials, 1.0, opt.step_counter) if self.norm_in_finalize() else None
            nb = eng.backward(d_heads, loss_finalize=ops.loss_finalize_desc(*fin), norm=norm, ppo_loss=ppo)
            a._norm_ready = (self.norm_partials, nb) if nb else None
        else:
            ops.ppo_loss_finalize(*fin)
            eng.backward(d_heads)
        # the step's mu is in the dataset now (write_back) and logstd is still the pre-step one (Adam comes behind)
        a._diag_update(inp, (mu, net.sigma))


class PairPath(AutogradPath):
    """Separate actor / critic trunks with an RNN each on chain_net.RecurrentChainPair - update and rollout; the loss
    launch writes d mu / d value into the two engines' d_heads.  Updates stay eager: the step graphs alone read its chains."""
    kind = 'pair'
    last_states = property(lambda self: self.pair.last_states)
    rollout_ok = property(lambda self: fp32_space(self.agent.observation_space))

    @staticmethod
    def declined(agent, config, general):
        """Why a network stays off the pair (None: it is eligible)."""
        net = agent.model.a2c_network
        if not getattr(net, 'plain_separate_rnn', False):
            return 'not a continuous policy of separate plain trunks with an RNN each'
        if not config.get('manual_lstm', True):
            return 'manual_lstm is off'
        if not config.get('fused_mlp', True):
            return 'fused_mlp is off'
        if general:
            return 'a log sigma vector and one value column only'
        if not all(isinstance(a, nn.Identity) for a in (net.mu_act, net.value_act, net.sigma_act)):
            return 'identity head activations only'
        return rnn_cell_declined(net.rnn_name, net.rnn_layers, net.rnn_units)

    @staticmethod
    def layout(net):
        """The matrices first, each trunk's bias vectors directly behind them (where RecurrentChainNet's chains want
        them), the head biases last."""
        first = [m.bias for trunk in (net.actor_mlp, net.critic_mlp) for m in trunk if isinstance(m, nn.Linear)]
        return arena_layout(list(net.parameters()), [[net.mu], [net.value]], first_vectors=first)

    def __init__(self, agent):
        super().__init__(agent)
        net = agent.model.a2c_network
        ln = (net.a_layer_norm, net.c_layer_norm) if net.rnn_ln else (None, None)
        self.pair = RecurrentChainPair(
            net.actor_mlp, net.a_rnn.rnn, ln[0], net.mu, net.critic_mlp, net.c_rnn.rnn, ln[1], net.value,
            agent.optimizer, agent.minibatch_size, infer_rows=agent.num_actors * agent.num_agents)
        self.engines = [self.pair.actor, self.pair.critic]

    def takes(self, obs):
        return obs.dtype == torch.float32          # (the pair's chains read the observations raw)

    def infer(self, obs, rnn_states, logits_only=False):
        """The pair's T = 1 forward on `rnn_states` (the actor's, then the critic's), whose [value | mu] rows are the
        pair's joint heads and whose next states stay in its `last_states`."""
        a = self.agent
        self.pair.forward(_unit_stride(obs), a._obs_rms(), a._obs_eps(), rnn_states, None, 1, keep=False)
        return self.pair.joint_heads[:obs.shape[0]]

    values = EnginePath.values

    def train_forward(self, obs, inp):
        a, pair = self.agent, self.pair
        if not obs.is_contiguous():
            obs = obs.contiguous()
        mu, values = train_forward(pair, self._stats_module(), obs, inp['rnn_states'],
                                   inp['dones'] if a.zero_rnn_on_done else None, a.seq_length)
        mb = mu.shape[0]
        return (mu, a.model.a2c_network.sigma), values[:, 0], pair.actor.d_heads[:mb], pair.critic.d_heads[:mb, 0]

    def backward(self):
        self.pair.backward()


class ChainsPath(AutogradPath):
    """A feed-forward discrete network on the fused chain kernels: one ChainNet over [value | logits] behind a shared
    trunk, one per trunk with `separate: True` ([logits], [value])."""
    kind = 'chains'
    rollout_ok = property(lambda self: len(self.agent.branch_sizes) <= ops.CATEGORICAL_MAX_BRANCHES)

    def __init__(self, agent):
        super().__init__(agent)
        net = agent.model.a2c_network
        trunks = [net.actor_mlp, net.critic_mlp] if net.is_separate_critic() else [net.actor_mlp]
        self.chains = [ChainNet(t, g, agent.optimizer, agent.minibatch_size, infer_rows=agent.num_actors * agent.num_agents)
                       for t, g in zip(trunks, chain_heads(net))]
        self.engines = self.chains

    def takes(self, obs):
        return obs.dtype in (torch.float32, torch.uint8)         # (_preproc_obs: uint8 / 255 -> fp32)

    def infer(self, obs, rnn_states=None, logits_only=False):
        """(logits [N, sum(sizes)], value [N, 1]) of fp32 observations (any row stride): each chain's inference forward,
        the observation normaliser in eval mode inside the launch.  logits_only (a central value network supplies the
        values): the separate critic trunk does not run, value is None."""
        a, obs = self.agent, _unit_stride(obs)
        chains = self.chains[:1] if logits_only else self.chains
        heads = [c.infer(obs, a._obs_rms(), a._obs_eps()) for c in chains]
        if len(self.chains) == 1:
            return _value_and_rest(heads[0])
        return heads[0], (None if logits_only else heads[1])

    def values(self, obs, rnn_states):
        """The critic alone: column 0 of the last chain's heads ([value | logits], or the critic trunk's [value])."""
        a = self.agent
        return self.chains[-1].infer(_unit_stride(obs), a._obs_rms(), a._obs_eps())[:, :1].contiguous()

    def train_forward(self, obs, inp):
        """Each trunk + its heads as one launch that normalises on the way in."""
        chains, mb = self.chains, obs.shape[0]
        rms, eps = launch_stats(self._stats_module(), obs)
        outs = [c.forward(obs, rms, eps) for c in chains]
        if len(chains) == 1:
            (logits, values), (d_logits, d_values) = _value_and_rest(outs[0]), _value_and_rest(chains[0].d_heads[:mb])
        else:
            logits, values, d_logits, d_values = outs[0], outs[1], chains[0].d_heads[:mb], chains[1].d_heads[:mb]
        return logits, values[:, 0], d_logits, d_values[:, 0]

    def backward(self):
        for c in self.chains:
            c.backward()


class RecurrentPath(ChainsPath):
    """A recurrent discrete network of the reference's SMAC shape on chain_net.RecurrentChainNet over [value | logits]:
    trunk + gate-input product, the sequence kernel, (layer norm,) heads."""
    kind, chains = 'recurrent', None
    last_states = property(lambda self: self.recurrent.last_states)

    @staticmethod
    def declined(net, config):
        """Why a recurrent network stays off the engine (None: it is eligible)."""
        if not config.get('manual_lstm', True):
            return 'manual_lstm is off'
        if not getattr(net, 'plain_trunk_rnn_ln', False) or net.is_separate_critic():
            return 'plain Linear + activation trunks only'
        return rnn_cell_declined(net.rnn_name, net.rnn_layers, net.rnn_units)

    def __init__(self, agent):
        AutogradPath.__init__(self, agent)
        net = agent.model.a2c_network
        self.recurrent = RecurrentChainNet(net.actor_mlp, net.rnn.rnn, net.layer_norm if net.rnn_ln else None,
                                           chain_heads(net)[0], agent.optimizer, agent.minibatch_size,
                                           infer_rows=agent.num_actors * agent.num_agents)
        self.engines = [self.recurrent]

    def infer(self, obs, rnn_states=None, logits_only=False):
        """The engine's T = 1 forward on `rnn_states` - the states arrive zeroed where an episode ended, as for the
        model's eval forward, which takes no done flags (a2c_common.py:590) - leaving the next ones in last_states."""
        a = self.agent
        return _value_and_rest(self.recurrent.forward(_unit_stride(obs), a._obs_rms(), a._obs_eps(), rnn_states, None, 1,
                                                      keep=False))

    def values(self, obs, rnn_states):
        """The same forward as a rollout step; the states it leaves are dropped."""
        return self.infer(obs, rnn_states)[1].contiguous()

    def train_forward(self, obs, inp):
        a, eng = self.agent, self.recurrent
        heads = train_forward(eng, self._stats_module(), obs, inp['rnn_states'],
                              inp['dones'] if a.zero_rnn_on_done else None, a.seq_length)
        (logits, values), (d_logits, d_values) = _value_and_rest(heads), _value_and_rest(eng.d_heads[:obs.shape[0]])
        return logits, values[:, 0], d_logits, d_values[:, 0]

    def backward(self):
        self.recurrent.backward()


class Plan:
    """Phase one, in front of FlatAdam: the path an agent's network can take (`cls`; None: none of the engines was asked
    for), the arena layout that path needs (None: parameters() order), and why it was declined (`why`) - every
    eligibility question is asked here, once.  build() is phase two."""

    def __init__(self, agent, config):
        net = agent.model.a2c_network
        rest = [p for p in agent.model.parameters() if all(p is not q for q in net.parameters())]
        self.cls = self.why = self.notice = self.layout = None
        self.fallback = AutogradPath
        if agent.is_discrete:
            # (the arena is reordered for the chains even where they then decline the network: the order in which the
            #  gradient-norm partials are summed, and so the bits of every such run, hang on it - left as it is)
            if not config.get('fused_mlp', True):
                return
            self.notice = 'discrete network outside the fused chain kernels ({}); using autograd'
            rnn_why = RecurrentPath.declined(net, config) if net.is_rnn() else None
            first = ()
            if net.is_rnn() and rnn_why is None:
                first = [m.bias for m in net.actor_mlp if isinstance(m, nn.Linear)]      # (RecurrentChainNet's trunk)
            self.layout = arena_layout(list(net.parameters()), chain_heads(net), first_vectors=first) + rest
            self.cls = RecurrentPath if net.is_rnn() else ChainsPath
            if agent.value_size != 1 or not isinstance(net.value_act, nn.Identity):
                self.why = 'one linear value column only'
            elif net.is_rnn():
                self.why = rnn_why
            elif not getattr(net, 'plain_trunk', True):
                self.why = 'plain Linear + activation trunks only'
            return
        general = (agent.value_size != 1 or not getattr(net, 'fixed_sigma', True) or not getattr(net, 'plain_sigma', True))
        if general:
            self.fallback = GeneralPath
        if (config.get('manual_mlp', True) and not general and getattr(net, 'plain_trunk', True)
                and not net.is_separate_critic() and (not agent.is_rnn or config.get('manual_lstm', True))):
            self.cls, self.notice = EnginePath, 'manual MLP engine unavailable ({}); using autograd'
            self.layout = ManualMLP.layout(net) + rest
        elif net.is_rnn() and net.is_separate_critic():
            self.cls = PairPath
            self.notice = 'separate recurrent trunks outside the paired RNN engine ({}); using autograd'
            self.why = PairPath.declined(agent, config, general)
            if self.why is None:
                self.layout = PairPath.layout(net) + rest

    def build(self, agent):
        """Behind the optimiser: the planned path, or - declined, or its engine refuses the network - the notice and
        the autograd (general) path."""
        if self.cls is not None and self.why is None:
            try:
                return self.cls(agent)
            except NotImplementedError as e:
                self.why = str(e)
        if self.notice is not None:
            print('rl_games_amd: ' + self.notice.format(self.why))
        return self.fallback(agent)
