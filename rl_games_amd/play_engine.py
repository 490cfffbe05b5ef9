"""The players' fused path (`player.fused: True`): a trained policy's step on the inference forwards the agents roll
out through, the action from one launch of csrc/play.hip behind the heads, the whole step replayed as a HIP graph from
its second call on, and the episode accounting of run() on the device (one host read every `fused_poll_steps` steps).
Which engine runs the network, and whether one does, is actor_paths.Plan's answer - the player is shown to it as the
agent it asks (_PlayAgent): the same eligibility checks, arena layouts and infer sequences as the agents' rollout.
"""
import torch

from . import ops
from .actor_paths import EnginePath, Plan
from .agent import A2CAgent
from .discrete_agent import draw_exp_noise
from .flat_optim import FlatArena
from .hip_graphs import GraphCaptureError, GraphCapturer, StepGraphs
from .weight_forms import ChainFormSet

TRAIN_ROWS = 16        # rows the engines' training buffers are sized for where a constructor takes them apart (infer_rows)
NOTICE = 'rl_games_amd: player outside the fused play path ({}); using torch modules'


class _PlayAgent:
    """What actor_paths.Plan and its paths ask an agent, answered for a player of `rows` rows: no optimiser (a FlatArena
    in its place), no minibatches (TRAIN_ROWS), one agent per row."""
    num_agents, minibatch_size, _roll_obs_norm = 1, TRAIN_ROWS, None
    _obs_rms, _obs_eps = A2CAgent._obs_rms, A2CAgent._obs_eps

    def __init__(self, player, rows):
        self.model, self.config, self.optimizer = player.model, player.config, None
        self.is_discrete = hasattr(player, 'is_multi_discrete')
        self.value_size, self.is_rnn, self.normalize_input = player.value_size, player.is_rnn, player.normalize_input
        self.observation_space, self.num_actors = player.observation_space, rows
        if self.is_discrete:
            self.branch_sizes = list(player.actions_num) if player.is_multi_discrete else [player.actions_num]


class FusedPlay:
    """One player's engine, step graphs and episode totals.  declined: why the network plays on its torch modules
    (None: it runs here)."""

    def __init__(self, player, rows):
        self.player, self.path, self.rows = player, None, 0
        self._graphs_ok = bool(player.config.get('hip_graphs', True))
        self._agent = agent = _PlayAgent(player, rows)
        self._plan = plan = Plan(agent, player.config)
        self.declined = plan.why
        if plan.cls is None:
            general = not agent.is_discrete and plan.fallback is not None and plan.fallback.kind == 'general'
            self.declined = ('a log sigma vector and one value column only' if general else
                             'no engine takes this network')
        if self.declined is None:
            params = list(player.model.parameters())
            agent.optimizer = self.arena = FlatArena(params, plan.layout)
            self._build(rows)
        if self.declined is not None:
            print(NOTICE.format(self.declined))

    def _build(self, rows):
        """The planned path for `rows` rows (again when a call brings more): engines, scratch, no graphs yet."""
        agent, player = self._agent, self.player
        agent.num_actors = rows
        try:
            path = self._plan.cls(agent)
        except NotImplementedError as e:
            self.declined = str(e)
            return
        if isinstance(path, EnginePath) and path.engine.chain is None and path.engine.chain_rnn is None:
            self.declined = 'the fused chain does not take this network'
        elif not path.rollout_ok:
            self.declined = 'more than 16 branches' if agent.is_discrete else 'fp32 observation spaces only'
        if self.declined is not None:
            return
        self.path, self.rows = path, rows
        self._forms = ChainFormSet(path.chain_forms())
        self._graphs, self._seen = StepGraphs(GraphCapturer(self._forms)), set()
        self.replayed = False                       # the last step was a graph replay
        dev = player.device
        if agent.is_discrete:
            sizes = agent.branch_sizes
            self._noise = torch.empty(rows * sum(sizes), dtype=torch.float32, device=dev)
            self._actions = torch.empty((rows, len(sizes)) if player.is_multi_discrete else (rows,), dtype=torch.int64,
                                        device=dev)
        else:
            self._noise = torch.empty(rows, player.actions_num, dtype=torch.float32, device=dev)
            self._actions = torch.empty(rows, player.actions_num, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ one step
    def takes(self, obs):
        return self.declined is None and obs.dim() == 2 and self.path.takes(obs)

    def _kernels(self, obs, states, masks, deterministic):
        """Inference forward (the normaliser in eval mode inside the launch), the draws, one head launch.
        -> (actions, next states)."""
        player, rows = self.player, obs.shape[0]
        heads = self.path.infer(obs, states, logits_only=True)
        actions = self._actions[:rows]
        if self._agent.is_discrete:
            noise = None
            if not deterministic:
                noise = self._noise
                draw_exp_noise(noise, rows, self._agent.branch_sizes)
            ops.play_categorical_head(heads[0], self._agent.branch_sizes, noise, masks, actions)
        else:
            noise = None
            if not deterministic:
                noise = self._noise[:rows]
                torch.randn(noise.shape, device=noise.device, out=noise)
            bounds = (player.actions_low, player.actions_high) if player.clip_actions else None
            ops.play_policy_head(heads[:, 1:], player.model.a2c_network.sigma.data, noise, actions, bounds)
        return actions, (self.path.last_states if self._agent.is_rnn else None)

    @torch.no_grad()
    def step(self, obs, masks, deterministic):
        """obs fp32 [rows, ...] as _to_device leaves it, masks bool [rows, sum(sizes)] or None.  Sets the player's
        states; returns the actions (this object's buffer: valid until the next step).  The first call at a (rows, dtype,
        deterministic, masks) key runs eagerly, the second captures the step, every later one replays it."""
        player, rows = self.player, obs.shape[0]
        if rows > self.rows:
            self._build(rows)
        if not obs.is_contiguous():
            obs = obs.contiguous()
        key = (rows, obs.dtype, bool(deterministic), masks is not None)
        self._forms.before_replay(rollout=True)
        if not (self._graphs_ok and key in self._seen):
            self._seen.add(key)
            self.replayed = False
            actions, states = self._kernels(obs, player.states, masks, deterministic)
        else:
            try:
                body = lambda **static: self._kernels(**static, deterministic=deterministic)
                actions, states = self._graphs.step(key, body, {'obs': obs, 'states': player.states, 'masks': masks})
            except GraphCaptureError as e:
                print(f'rl_games_amd: HIP graph capture of the play step failed ({e.__cause__!r}); continuing eagerly')
                self._graphs_ok = False
                return self.step(obs, masks, deterministic)
            self.replayed = True
        if states is not None:
            player.states = list(states)
        return actions

    # ------------------------------------------------------------------ run(): episode accounting on the device
    def start_run(self, rows, poll_steps):
        dev = self.player.device
        self._poll = max(1, int(poll_steps))
        self._cur_r = torch.zeros(rows, dtype=torch.float32, device=dev)
        self._cur_n = torch.zeros(rows, dtype=torch.float32, device=dev)
        self._partials = torch.zeros(self._poll, ops.play_post_step_blocks(rows), 3, dtype=torch.float64, device=dev)
        self._totals, self._games = ops.play_totals(dev)
        self._step = 0

    def post_step(self, rewards, dones):
        """One launch: the step's rewards / done flags into the running episodes and slot step % K; where an episode
        ended the RNN states are zeroed (one launch per state).  Every K steps: one fold launch.  -> K steps are full."""
        dones = dones.reshape(-1)
        if dones.dtype not in (torch.bool, torch.uint8):
            dones = dones != 0
        if rewards.dtype != torch.float32:
            rewards = rewards.float()
        ops.play_post_step(rewards.reshape(self._cur_r.shape[0], -1), dones, self._cur_r, self._cur_n,
                           self._partials[self._step % self._poll])
        flags = dones.view(torch.uint8) if dones.dtype == torch.bool else dones
        for s in self.player.states or ():
            ops.rnn_zero_done_states(s, flags)
        self._step += 1
        return self._step % self._poll == 0

    def fold(self, games_limit):
        """The slots written since the last fold into the totals."""
        slots = self._step % self._poll or self._poll
        ops.play_fold(self._partials, slots, games_limit, self._totals)

    def read_totals(self):
        """The one host read: (reward sum, length sum, games)."""
        host = self._totals.cpu()
        return float(host[0]), float(host[1]), int(host.view(torch.int64)[2])
