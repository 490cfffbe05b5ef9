"""The fused rollout of agents with a central value network: the head kernels' value source
(ops.rollout_policy_head / rollout_categorical_head with `value=` / `value_repeat=`, the value fields of the two heads'
descriptors, csrc/experience.hip and csrc/rollout_categorical.hip) against the heads' own column and a torch restatement, and the
agents' rollout with `fused_rollout` on against off (a2c_common.py:593-617 get_action_values / get_values with a central
value: the critic's de-normalised value, repeated for the agents of an env), with the step graphs on against off, after
new critic weights between epochs, and the eligibility rule."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, STEP = 4, 2


def _value_stats(on):
    if not on:
        return None
    from rl_games_amd.normalizers import RunningMeanStd
    vm = RunningMeanStd((1,)).to(DEV)
    vm.running_mean.fill_(0.75)
    vm.running_var.fill_(2.5)
    vm.eval()
    return vm


def _denorm(v, vstats):
    return v if vstats is None else vstats(v, denorm=True)


# ----------------------------------------------------------------------------- continuous head

def _cont_storage(N, A):
    return {'actions': torch.full((N, H, A), -7.0, device=DEV), 'mus': torch.full((N, H, A), -7.0, device=DEV),
            'sigmas': torch.full((N, H, A), -7.0, device=DEV), 'neglogpacs': torch.full((N, H), 1234.5, device=DEV),
            'values': torch.full((N, H, 1), -99.0, device=DEV)}


def _run_cont(heads, logstd, noise, vstats, value=None, repeat=1, clip=None):
    from rl_games_amd import ops
    N, A = noise.shape
    st = _cont_storage(N, A)
    acts, vals = torch.empty(N, A, device=DEV), torch.empty(N, device=DEV)
    vs = None if vstats is None else (vstats.running_mean, vstats.running_var)
    env = None if clip is None else (torch.empty(N, A, device=DEV), clip[0], clip[1])
    ops.rollout_policy_head(heads, logstd, noise, vs, 1e-5 if vstats is None else vstats.epsilon, acts, vals, st, H,
                            STEP, env_actions=env, value=value, value_repeat=repeat)
    return acts, vals, st, (None if env is None else env[0])


@pytest.mark.parametrize('N', [300, 4099, 65536])
@pytest.mark.parametrize('A', [1, 12, 21, 64])
def test_policy_head_value_source(N, A):
    """The new entry against the existing one on the same heads and noise: actions / mus / sigmas / neglogp bit for bit;
    values = denorm(value).repeat_interleave(repeat); with value = heads[:, :1] and repeat 1 the values are the existing
    entry's bits too.  A <= 21: the LDS tile form; A = 64: the block's tiles (64 * (1 + 2A) floats) pass 32 KiB, so the
    one-thread-per-env form runs.  Value columns with a row stride > 1 (ld_value 5)."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(N + 7 * A)
    assert (64 * (1 + 2 * A) * 4 > 32 * 1024) == (A == 64)
    heads = torch.randn(N, 1 + A, generator=gen, device=DEV) * 3
    logstd = torch.randn(A, generator=gen, device=DEV) * 0.3
    clip = (-torch.rand(A, generator=gen, device=DEV) - 0.5, torch.rand(A, generator=gen, device=DEV) + 0.5)
    for repeat in (1, 3):
        rows = N - N % repeat
        h, noise = heads[:rows], torch.randn(rows, A, generator=gen, device=DEV)
        cv = torch.randn(rows // repeat, 5, generator=gen, device=DEV)[:, 2:3] * 4          # ld_value 5
        for norm in (False, True):
            vstats = _value_stats(norm)
            ref_a, ref_v, ref_st, ref_env = _run_cont(h, logstd, noise, vstats, clip=clip)
            a, v, st, env = _run_cont(h, logstd, noise, vstats, value=cv, repeat=repeat, clip=clip)
            assert torch.equal(a, ref_a) and torch.equal(env, ref_env)
            for k in ('actions', 'mus', 'sigmas', 'neglogpacs'):
                assert torch.equal(st[k], ref_st[k]), k
            want = _denorm(cv, vstats).reshape(-1).repeat_interleave(repeat)
            assert torch.allclose(v, want, rtol=1e-6, atol=1e-6)
            assert torch.equal(st['values'][:, STEP, 0], v)
            others = [t for t in range(H) if t != STEP]
            assert (st['values'][:, others] == -99.0).all()
            if repeat == 1:                                     # the new entry with the heads' own value column
                a1, v1, st1, env1 = _run_cont(h, logstd, noise, vstats, value=h[:, :1], repeat=1, clip=clip)
                assert torch.equal(a1, ref_a) and torch.equal(v1, ref_v)
                for k in st1:
                    assert torch.equal(st1[k], ref_st[k]), k
                # value=None travels as a NULL field, for which the entry puts the heads' column 0 itself: every output
                # and buffer field of that run against the run that names the column
                a0, v0, st0, env0 = _run_cont(h, logstd, noise, vstats, value=None, clip=clip)
                assert torch.equal(a0, a1) and torch.equal(v0, v1) and torch.equal(env0, env1)
                for k in st1:
                    assert torch.equal(st0[k], st1[k]), k


def test_head_entries_reject_value_repeat_below_one():
    from rl_games_amd import _lib
    lib = _lib.load()
    N, A = 8, 2
    heads, noise = torch.zeros(N, 1 + A, device=DEV), torch.ones(N, A, device=DEV)
    logstd, st = torch.zeros(A, device=DEV), _cont_storage(N, A)
    acts, vals = torch.empty(N, A, device=DEV), torch.empty(N, device=DEV)
    sizes = (ctypes.c_int * 1)(A)
    cat_acts = torch.empty(N, dtype=torch.int64, device=DEV)
    cat_buf = torch.empty(N, H, dtype=torch.int64, device=DEV)
    for repeat in (0, -2):
        head = _lib.PolicyHeadDesc(
            heads=heads.data_ptr(), ld=1 + A, value=heads.data_ptr(), ld_value=1 + A, value_repeat=repeat,
            logstd=logstd.data_ptr(), noise=noise.data_ptr(), eps=1e-5, actions_out=acts.data_ptr(),
            values_out=vals.data_ptr(), buf_actions=st['actions'].data_ptr(), buf_mus=st['mus'].data_ptr(),
            buf_sigmas=st['sigmas'].data_ptr(), buf_neglogp=st['neglogpacs'].data_ptr(),
            buf_values=st['values'].data_ptr(), N=N, H=H, A=A, step=STEP)
        err = lib.rlg_rollout_policy_head(ctypes.addressof(head), None)
        assert err == 1, err                                    # hipErrorInvalidValue
        cat = _lib.CategoricalHeadDesc(
            logits=heads[:, 1:].data_ptr(), ld_logits=1 + A, branch_sizes=ctypes.addressof(sizes), num_branches=1,
            exp_noise=noise.data_ptr(), value=heads.data_ptr(), ld_value=1 + A, value_repeat=repeat, eps=1e-5,
            actions_out=cat_acts.data_ptr(), values_out=vals.data_ptr(), buf_actions=cat_buf.data_ptr(),
            buf_neglogp=st['neglogpacs'].data_ptr(), buf_values=st['values'].data_ptr(), num_envs=N, horizon=H,
            step=STEP)
        err = lib.rlg_rollout_categorical_head(ctypes.addressof(cat), None)
        assert err == 1, err
    head.value_repeat = cat.value_repeat = 1                    # the same descriptors are launched once the field is valid
    assert lib.rlg_rollout_policy_head(ctypes.addressof(head), None) == 0
    assert lib.rlg_rollout_categorical_head(ctypes.addressof(cat), None) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- categorical head

def _run_cat(logits, value, sizes, noise, masks, vstats, repeat):
    from rl_games_amd import ops
    N, B = logits.shape[0], len(sizes)
    st = {'actions': torch.full((N, H, B), -7, dtype=torch.int64, device=DEV),
          'neglogpacs': torch.full((N, H), 1234.5, device=DEV), 'values': torch.full((N, H, 1), -99.0, device=DEV)}
    acts = torch.empty(N, B, dtype=torch.int64, device=DEV)
    vals = torch.empty(N, device=DEV)
    vs = None if vstats is None else (vstats.running_mean, vstats.running_var)
    ops.rollout_categorical_head(logits, value, sizes, noise, masks, vs, 1e-5 if vstats is None else vstats.epsilon,
                                 acts, vals, st, H, STEP, value_repeat=repeat)
    return acts, vals, st


@pytest.mark.parametrize('N', [300, 4098, 65535])
@pytest.mark.parametrize('sizes', [[6], [3, 5, 2], [3, 70]])
def test_categorical_head_value_source(N, sizes):
    """Actions and neglogp bit for bit against the existing entry on the same logits, masks and draws; values =
    denorm(value).repeat_interleave(3).  [3, 70]: the one-wave-per-row form, else the 64-row LDS tile form."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(N + len(sizes))
    S = sum(sizes)
    t = (torch.rand(N, 1 + S + 3, generator=gen, device=DEV) * 2 - 1) * 30
    logits, own_value = t[:, 1:1 + S], t[:, :1]
    noise = torch.empty(N * S, device=DEV).exponential_(generator=gen)
    masks = torch.rand(N, S, generator=gen, device=DEV) > 0.3
    cv = torch.randn(N // 3, 4, generator=gen, device=DEV)[:, 1:2] * 4
    for m in (None, masks):
        for norm in (False, True):
            vstats = _value_stats(norm)
            ref_a, _, ref_st = _run_cat(logits, own_value, sizes, noise, m, vstats, 1)
            a, v, st = _run_cat(logits, cv, sizes, noise, m, vstats, 3)
            assert torch.equal(a, ref_a) and torch.equal(st['actions'], ref_st['actions'])
            assert torch.equal(st['neglogpacs'], ref_st['neglogpacs'])
            want = _denorm(cv, vstats).reshape(-1).repeat_interleave(3)
            assert torch.allclose(v, want, rtol=1e-6, atol=1e-6)
            assert torch.equal(st['values'][:, STEP, 0], v)


# ----------------------------------------------------------------------------- the agents

def _cv_config(units=(32, 16), norm_in=True, **over):
    cfg = {'minibatch_size': 128, 'mini_epochs': 2, 'learning_rate': 5e-4, 'clip_value': True,
           'normalize_input': norm_in, 'truncate_grads': True, 'grad_norm': 1.0,
           'network': {'name': 'actor_critic', 'central_value': True,
                       'mlp': {'units': list(units), 'activation': 'elu', 'initializer': {'name': 'default'}}}}
    cfg.update(over)
    return cfg


def _cont_params(num_actors=64, horizon=8, agents=1, cv_norm_in=True, norm_value=True, clip_actions=True, lstm=False,
                 cv_over=None, **over):
    from rl_games_amd import configs
    params = configs.tiny(num_actors=num_actors, horizon=horizon, obs_dim=12, act_dim=3, seq_length=4,
                          normalize_value=norm_value, clip_actions=clip_actions, **over)
    if lstm:
        params['network']['rnn'] = {'name': 'lstm', 'units': 16, 'layers': 1}
    params['config']['central_value_config'] = _cv_config(norm_in=cv_norm_in, minibatch_size=num_actors * horizon // 2,
                                                          **(cv_over or {}))
    params['config']['env_config'].update(state_dim=9, agents=agents, p_done=0.1)
    return params


def _disc_params(layout, agents=1, num_actors=64, horizon=8, **over):
    from rl_games_amd import configs
    params = configs.cartpole_discrete(num_actors=num_actors, device=DEV, normalize_input=True, normalize_value=True,
                                       horizon_length=horizon, minibatch_size=num_actors * agents * horizon // 2,
                                       **over)
    net = params['network']
    net['separate'] = layout == 'separate'
    params['config']['env_config'].update(obs_dim=8, discrete_actions=4, autoreset_mode='same_step', state_dim=13,
                                          agents=agents)
    if layout == 'multi_discrete_masked':                # SMAC-like: several agents per env, action masks
        net['space'] = {'multi_discrete': None}
        params['model']['name'] = 'multi_discrete_a2c'
        params['config']['use_action_masks'] = True
        params['config']['env_config'].update(discrete_actions=[3, 5, 2], obs_dim=12, action_masks=True)
    params['config']['central_value_config'] = _cv_config(minibatch_size=num_actors * horizon // 2)
    return params


_FIELDS = ('obses', 'dones', 'states', 'actions', 'mus', 'sigmas', 'neglogpacs', 'values', 'action_masks')


def _agent(params, seed=4):
    from rl_games_amd.agent import A2CAgent
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    torch.manual_seed(seed)
    cls = DiscreteA2CAgent if params['algo']['name'] == 'a2c_discrete' else A2CAgent
    agent = cls('cvroll', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    batches = []
    play = agent.play_steps_rnn if agent.is_rnn else agent.play_steps

    def recording_play_steps():
        batch = play()
        rec = {k: batch[k].clone() for k in _FIELDS if k in batch}
        rec['returns'] = batch['returns'].clone()
        rec['rng'] = torch.cuda.get_rng_state()
        batches.append(rec)
        return batch
    if agent.is_rnn:
        agent.play_steps_rnn = recording_play_steps
    else:
        agent.play_steps = recording_play_steps
    return agent, batches


def _run_epochs(agent, n):
    for _ in range(n):
        agent.update_epoch()
        agent.train_epoch()


def _compare_fused_torch(out, exact, close, tol=1e-5):
    for a, b in zip(out[True], out[False]):
        assert a.keys() == b.keys()
        assert torch.equal(a['rng'], b['rng']), 'generator state differs after play_steps'
        for k in exact:
            if k in a:
                assert torch.equal(a[k], b[k]), k
        for k in close:
            if k in a:
                assert torch.allclose(a[k], b[k], rtol=tol, atol=tol), (k, (a[k] - b[k]).abs().max().item())


@pytest.mark.parametrize('cv_norm_in,norm_value,agents,clip_actions', [
    (True, True, 1, True), (False, True, 1, True), (True, False, 1, False), (True, True, 3, True),
    (False, False, 3, False)])
def test_continuous_fused_rollout_matches_torch_rollout(cv_norm_in, norm_value, agents, clip_actions):
    """Two epochs (the second replays the step graphs) with `fused_rollout` on and off at the same seed, value_bootstrap
    with the env's time-outs: obses / dones / states bit for bit, actions / mus / sigmas / neglogpacs / values (the
    critic's) and returns to 1e-5, the generator in the same state after every play_steps (one normal_ of [rows, A] per
    step on both paths, nothing for the bootstrap)."""
    out = {}
    for fused in (True, False):
        agent, batches = _agent(_cont_params(agents=agents, cv_norm_in=cv_norm_in, norm_value=norm_value,
                                             clip_actions=clip_actions, fused_rollout=fused))
        assert agent.has_central_value and agent.value_bootstrap and agent.num_agents == agents
        assert agent._fast_rollout_ok() == fused
        _run_epochs(agent, 2)
        if fused:
            assert len(agent._rollout_graphs) > 0
        out[fused] = batches
    _compare_fused_torch(out, ('obses', 'dones', 'states'),
                         ('actions', 'mus', 'sigmas', 'neglogpacs', 'values', 'returns'))
    if agents > 1:
        v = out[True][-1]['values'].reshape(64, agents, 8)
        assert torch.equal(v[:, 0], v[:, 1]) and torch.equal(v[:, 0], v[:, 2])


@pytest.mark.parametrize('layout,agents', [('shared', 1), ('separate', 1), ('multi_discrete_masked', 3),
                                           ('separate', 3)])
def test_discrete_fused_rollout_matches_torch_rollout(layout, agents):
    """The discrete agent with a central value network, `fused_rollout` on against off over two epochs: identical
    actions (and observations, dones, states, masks), values to 1e-5, the generator in the same state (the bootstrap
    runs the critic only: no Exp(1) draws)."""
    out = {}
    for fused in (True, False):
        agent, batches = _agent(_disc_params(layout, agents=agents, fused_rollout=fused))
        assert agent._fast_rollout_ok() == fused
        _run_epochs(agent, 2)
        if fused:
            assert len(agent._rollout_graphs) > 0
        out[fused] = batches
    _compare_fused_torch(out, ('obses', 'dones', 'states', 'actions', 'action_masks'), ('neglogpacs', 'values'))


def test_lstm_actor_with_feed_forward_critic():
    """play_steps_rnn on the LSTM engine with the critic on its chain: fused against torch, same tolerances."""
    out = {}
    for fused in (True, False):
        agent, batches = _agent(_cont_params(lstm=True, fused_rollout=fused))
        assert agent.is_rnn and agent._engine is not None and not agent.central_value_net.is_rnn
        assert agent._fast_rollout_ok() == fused
        _run_epochs(agent, 2)
        out[fused] = batches
    _compare_fused_torch(out, ('obses', 'dones', 'states'),
                         ('actions', 'mus', 'sigmas', 'neglogpacs', 'values', 'returns'))


@pytest.mark.parametrize('num_actors', [64, 16384])
@pytest.mark.parametrize('kind', ['continuous', 'discrete'])
def test_rollout_graphs_replay_the_eager_rollout(kind, num_actors):
    """Three epochs with the step graphs on and off: every rollout tensor bit-identical.  16,384 envs: the actor's and the
    critic's inference forwards both run on split planes."""
    horizon = 4 if num_actors > 1024 else 8
    out = {}
    for graphs in (True, False):
        params = (_cont_params(num_actors=num_actors, horizon=horizon, agents=1, rollout_graphs=graphs)
                  if kind == 'continuous' else
                  _disc_params('separate', num_actors=num_actors, horizon=horizon, rollout_graphs=graphs))
        agent, batches = _agent(params)
        if num_actors >= 16384:
            assert agent._critic_chain().chain.split_products(num_actors, 0)
            actor = agent._engine.chain if kind == 'continuous' else agent._chains[0].chain
            assert actor.split_products(num_actors, 0)
        _run_epochs(agent, 3)
        assert (len(agent._rollout_graphs) > 0) == graphs
        out[graphs] = batches
    for a, b in zip(out[True], out[False]):
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('how', ['restore', 'set_central_value_function_weights', 'set_full_state_weights'])
@pytest.mark.parametrize('num_actors', [64, 16384])
def test_replayed_rollout_sees_new_critic_weights(how, num_actors, tmp_path):
    """New critic weights between epochs: the next rollout, replayed from graphs captured for the old weights, equals a
    fresh agent's eager rollout from the same weights, observations and seed."""
    horizon = 4 if num_actors > 1024 else 8
    params = _cont_params(num_actors=num_actors, horizon=horizon)
    donor, _ = _agent(params, seed=11)
    _run_epochs(donor, 1)
    path = donor.save(str(tmp_path / 'donor'))
    state = donor.get_full_state_weights()
    trained, got = _agent(params, seed=4)
    _run_epochs(trained, 2)
    assert len(trained._rollout_graphs) > 0
    fresh, ref = _agent(params, seed=5)
    for agent in (trained, fresh):
        if how == 'restore':
            agent.restore(path)
        elif how == 'set_full_state_weights':
            agent.set_full_state_weights(copy.deepcopy(state))
        else:
            agent.set_weights(donor.get_weights())                     # (the actor too, so that both rollouts agree)
            agent.set_central_value_function_weights({'assymetric_vf_nets': donor.central_value_net.state_dict()})
        agent.vec_env.seed(321)
        agent.obs = agent.env_reset()
        agent.dones = torch.ones_like(agent.dones)
        agent.set_eval()
        torch.manual_seed(99)
        with torch.no_grad():
            agent.play_steps()
    assert len(fresh._rollout_graphs) == 0 and fresh._fast_rollout_ok()
    for k in got[-1]:
        assert torch.equal(got[-1][k], ref[-1][k]), k


def test_eligibility():
    """Recurrent critics, `fused_mlp: False` in the critic's config and `fused_rollout: False` keep the torch rollout."""
    from rl_games_amd.agent import A2CAgent
    from rl_games_amd.discrete_agent import DiscreteA2CAgent

    def ok(params):
        cls = DiscreteA2CAgent if params['algo']['name'] == 'a2c_discrete' else A2CAgent
        return cls('cvok', copy.deepcopy(params))._fast_rollout_ok()
    assert ok(_cont_params()) and ok(_disc_params('separate'))
    rnn_critic = _cont_params()
    rnn_critic['config']['central_value_config']['network']['rnn'] = {'name': 'gru', 'units': 12, 'layers': 1}
    assert not ok(rnn_critic)
    assert not ok(_cont_params(cv_over={'fused_mlp': False}))
    assert not ok(_cont_params(fused_rollout=False))
    assert not ok(_disc_params('separate', fused_rollout=False))
    disc = _disc_params('shared')
    disc['config']['central_value_config']['fused_mlp'] = False
    assert not ok(disc)
