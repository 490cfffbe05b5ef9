"""GPU: continuous policies with separate actor / critic trunks, each with its own RNN (`separate: True`,
network_builder.py:272-277, :372-421) on chain_net.RecurrentChainPair - two RecurrentChainNet whose sequence kernels run
as one paired launch - in the update (hand-written BPTT against torch autograd and against recordings of the real
reference agent) and in the fused, captured rollout.  `_rnn_pair` is the agent's engine for them; `_engine` stays None."""
import copy
import gzip
import io
import os

import pytest
import torch

from rl_games_amd.synthetic_env import SyntheticTensorEnv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _agent(params, seed=0):
    from rl_games_amd.agent import A2CAgent
    torch.manual_seed(seed)
    return A2CAgent('test', copy.deepcopy(params))


def _params(cell='lstm', units=64, layer_norm=False, num_actors=24, horizon=8, **over):
    """The lunar shape (separate [64] relu trunks, one recurrent layer each) at a test's size: sequences of 4,
    p_done 0.2 with next_step autoreset (filler rows, rnn_masks, resets inside the sequences)."""
    from rl_games_amd import configs
    params = configs.lunar_separate_rnn(num_actors=num_actors, units=units, cell=cell, layer_norm=layer_norm,
                                        horizon_length=horizon, **over)
    params['config']['env_config'].update(p_done=0.2, autoreset_mode='next_step')
    return params


# ---- one epoch of the real reference agent -------------------------------------------------------------------------

def _replay(agent, cap):
    """The recorded rollout through this agent's dataset preparation and every minibatch step, as
    tests/test_agent_gpu.py::test_lstm_update_matches_reference_epoch replays it: per-step scalars, per-mini-epoch KLs."""
    agent.model.load_state_dict(cap['state_after_rollout'])
    batch = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [s.to(DEV) for s in v]) for k, v in cap['batch'].items()}
    agent.set_train()
    agent.prepare_dataset(batch)
    rows = []
    for mini_ep in range(agent.mini_epochs_num):
        for i in range(len(agent.dataset)):
            a, c, e, kl, lr, lr_mul, mu, sigma, b = agent.train_actor_critic(agent.dataset[i])
            rows.append(torch.stack([a, c, e, kl, b]).clone())
    rows = torch.stack(rows).cpu()
    kls = rows[:, 3].reshape(agent.mini_epochs_num, len(agent.dataset)).mean(1)
    return rows, kls


def _assert_epoch(agent, cap, rows, kls):
    """The quantities and tolerances of test_lstm_update_matches_reference_epoch."""
    for col, key in ((0, 'a_losses'), (1, 'c_losses'), (2, 'entropies')):
        print(key, 'max |diff|', (rows[:, col] - cap[key]).abs().max().item())
        assert torch.allclose(rows[:, col], cap[key], rtol=1e-5, atol=2e-6), key
    print('kl max |diff|', (kls - cap['mini_epoch_kls']).abs().max().item())
    assert torch.allclose(kls, cap['mini_epoch_kls'], rtol=1e-4, atol=2e-7), (kls, cap['mini_epoch_kls'])
    assert agent.optimizer.last_and_next_lr()[1] == cap['lrs'][-1]
    final = agent.model.state_dict()
    for k, v in cap['final_state'].items():
        tol = dict(rtol=1e-3, atol=5e-6) if v.is_floating_point() else dict(rtol=0, atol=0)
        assert torch.allclose(final[k].cpu().to(v.dtype), v, **tol), (k, (final[k].cpu().to(v.dtype) - v).abs().max())


def _recorded_agent(cap, **over):
    from rl_games_amd.agent import A2CAgent
    params = copy.deepcopy(cap['params'])
    params['config'].update(device=DEV, **over)
    env_kw = {k: v for k, v in cap['env'].items() if k != 'num_envs'}
    env = SyntheticTensorEnv(cap['env']['num_envs'], device=DEV, **env_kw)
    params['config']['vec_env'] = env
    params['config']['env_info'] = env.get_env_info()
    agent = A2CAgent('test', params)
    agent.init_tensors()
    return agent


def test_pair_matches_the_recorded_reference_epoch(golden):
    """tests/golden/epoch_separate_rnn.pt['separate_lstm'] (continuous, LSTM 16 per trunk, recorded from the real
    reference agent) with the default config: the pair runs it."""
    cap = golden('epoch_separate_rnn.pt')['separate_lstm']
    agent = _recorded_agent(cap)
    assert agent.is_rnn and agent._rnn_pair is not None and agent._engine is None
    assert agent._rnn_pair.paired and agent._rnn_pair.lstm
    assert len(agent.model.get_default_rnn_state()) == len(cap['batch']['rnn_states']) == 4
    rows, kls = _replay(agent, cap)
    _assert_epoch(agent, cap, rows, kls)


def test_twelve_units_decline_the_pair_and_still_match_the_recording(golden, capsys):
    """['separate_gru_layer_norm'] has 12 units, a width without kernels: the notice, then the torch path."""
    cap = golden('epoch_separate_rnn.pt')['separate_gru_layer_norm']
    agent = _recorded_agent(cap)
    assert 'outside the paired RNN engine' in capsys.readouterr().out
    assert agent.is_rnn and agent._rnn_pair is None and agent._engine is None and not agent._fast_rollout_ok()
    rows, kls = _replay(agent, cap)
    _assert_epoch(agent, cap, rows, kls)


# ---- the engine against autograd, the fused rollout against the torch step -----------------------------------------

def _grads(agent, batch, snapshot):
    b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'}
    agent.model.load_state_dict(snapshot)
    agent.set_train()
    agent.prepare_dataset(b)
    agent.train_actor_critic(agent.dataset[1])
    g = {n: p.grad.detach().clone() for n, p in agent.model.named_parameters()}
    res = agent.train_result
    g['_scalars'] = torch.stack([res[0], res[1], res[2], res[3], res[8]])
    return g


@pytest.mark.parametrize('cell,units,layer_norm', [('lstm', 64, False), ('gru', 128, True)])
def test_pair_matches_autograd_gradients_and_the_torch_rollout(cell, units, layer_norm):
    """24 envs x horizon 8 in sequences of 4 (24 sequences a minibatch: one and a half of the wide kernels' tiles),
    p_done 0.2 with filler rows; the engine is twinned with a `manual_lstm: False` agent holding the same weights.
    (i) The fused rollout (T = 1 launches) leaves the values, neglogpacs, mus and next states the torch model gives step
    by step for the stored actions.  (ii) One minibatch: autograd's scalars and gradients, layer-norm weight and bias
    included, at the tolerances of test_recurrent_engine_matches_autograd_gradients_and_rollout; the paired launch and two
    single launches give the same gradients bit for bit."""
    base = _params(cell, units, layer_norm, minibatch_size=96, learning_rate=0.0, grad_norm=1e9, lr_schedule=None)
    a1 = _agent(base)
    p2 = copy.deepcopy(base)
    p2['config']['manual_lstm'] = False
    a2 = _agent(p2)
    assert a1._rnn_pair is not None and a1._engine is None and a2._rnn_pair is None and a2._engine is None
    net = a1.model.a2c_network
    assert (net.rnn_name, net.rnn_units, net.rnn_ln, net.separate) == (cell, units, layer_norm, True)
    assert a1._fast_rollout_ok() and not a2._fast_rollout_ok()
    a2.model.load_state_dict(a1.model.state_dict())
    a1.init_tensors()
    a1.obs = a1.env_reset()
    a1.set_eval()
    with torch.no_grad():
        batch = a1.play_steps_rnn()
    assert batch['rnn_masks'].min() == 0                  # there are filler rows
    a2.init_tensors()
    a2.set_eval()
    Hz, N, T = a1.horizon_length, a1.num_actors, a1.seq_length
    per = 2 if cell == 'lstm' else 1
    assert len(batch['rnn_states']) == 2 * per
    obs = batch['obses'].reshape(N, Hz, -1)
    acts = batch['actions'].reshape(N, Hz, -1)
    mus, values = batch['mus'].reshape(N, Hz, -1), batch['values'].reshape(N, Hz, 1)
    nlp = batch['neglogpacs'].reshape(N, Hz)
    dones = a1.experience_buffer.tensor_dict['dones']     # [Hz, N]: the flags entering each step
    kept = [s.reshape(N, Hz // T, units) for s in batch['rnn_states']]      # the states entering each sequence
    with torch.no_grad():
        st = [s[:, ::Hz // T].contiguous() for s in batch['rnn_states']]      # states at t = 0
        assert st[0].shape == (1, N, units)
        for t in range(Hz):
            if t > 0:
                # play_steps_rnn zeroes the states of the episodes that ended in step t - 1 (flags of step t) and those a
                # filler row left in step t - 1 (flags of step t - 1; the flags the first rollout starts with mark none)
                keep = 1.0 - dones[t].float()
                if t > 1:
                    keep = keep * (1.0 - dones[t - 1].float())
                st = [s * keep.reshape(1, -1, 1) for s in st]
            if t % T == 0:
                # the four / two states the fused steps left, as play_steps_rnn kept them for the update
                for k, s in enumerate(st):
                    assert torch.allclose(kept[k][:, t // T], s[0], rtol=1e-4, atol=2e-6), (t, k)
            res = a2.model({'is_train': True, 'obs': obs[:, t], 'rnn_states': st, 'prev_actions': acts[:, t]})
            st = res['rnn_states']
            assert len(st) == 2 * per
            assert torch.allclose(res['mus'], mus[:, t], rtol=1e-4, atol=2e-6), t
            assert torch.allclose(a2.model.denorm_value(res['values']), values[:, t], rtol=1e-4, atol=2e-5), t
            assert torch.allclose(res['prev_neglogp'], nlp[:, t], rtol=1e-4, atol=2e-6), t
        # ... and the states behind the last step: the live ones
        keep = ((1.0 - a1.dones.float()) * (1.0 - dones[Hz - 1].float())).reshape(1, -1, 1)
        for k, s in enumerate(st):
            assert torch.allclose(a1.rnn_states[k], s * keep, rtol=1e-4, atol=2e-6), k
    snapshot = {k: v.detach().clone() for k, v in a1.model.state_dict().items()}
    g1 = _grads(a1, batch, snapshot)
    g2 = _grads(a2, batch, snapshot)
    assert a1._rnn_pair.paired
    a1._rnn_pair.paired = False                           # two single launches
    g3 = _grads(a1, batch, snapshot)
    a1._rnn_pair.paired = True
    assert a1._rnn_pair.actor.last_dw_path == 'mfma' and a1._rnn_pair.critic.last_dw_path == 'mfma'
    for n in g1:
        assert torch.equal(g1[n], g3[n]), f'{n}: the paired launch and two single launches differ'
    print('scalars', g1['_scalars'].tolist(), g2['_scalars'].tolist())
    assert torch.allclose(g1.pop('_scalars'), g2.pop('_scalars'), rtol=1e-5, atol=1e-7)
    assert any('layer_norm' in n for n in g2) == layer_norm
    assert any(n.startswith('a2c_network.c_rnn') for n in g2) and any(n.startswith('a2c_network.a_rnn') for n in g2)
    for n in g2:
        scale = g2[n].abs().max().item() + 1e-12
        print(n, 'max |diff|', (g1[n] - g2[n]).abs().max().item(), 'scale', scale)
        assert torch.allclose(g1[n], g2[n], rtol=1e-4, atol=5e-6 * scale), (n, (g1[n] - g2[n]).abs().max().item(), scale)


# ---- step graphs ---------------------------------------------------------------------------------------------------

_FIELDS = ('obses', 'dones', 'states', 'actions', 'mus', 'sigmas', 'neglogpacs', 'values', 'returns')


def _recording_agent(params, seed=4):
    """The agent with its rollouts recorded: every rollout tensor, the generator state, the live and the kept states."""
    agent = _agent(params, seed)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    batches = []
    play = agent.play_steps_rnn

    def recording_play_steps():
        batch = play()
        rec = {k: batch[k].clone() for k in _FIELDS if k in batch}
        rec['rng'] = torch.cuda.get_rng_state()
        for k, s in enumerate(agent.rnn_states):
            rec[f'rnn_states{k}'] = s.clone()
        for k, s in enumerate(batch['rnn_states']):
            rec[f'mb_rnn_states{k}'] = s.clone()
        if agent.has_central_value:
            for k, s in enumerate(agent.central_value_net.rnn_states):
                rec[f'cv_rnn_states{k}'] = s.clone()
        batches.append(rec)
        return batch
    agent.play_steps_rnn = recording_play_steps
    return agent, batches


def _run_epochs(agent, n):
    out = []
    for _ in range(n):
        agent.update_epoch()
        out.append(agent.train_epoch())
    return out


def _with_recurrent_critic(params):
    """configs.smac_rnn_cv_discrete's critic shape - a ReLU trunk [512, 256], one LSTM layer of 128 units, one value
    column over the env's privileged state - behind the continuous separate actor."""
    from rl_games_amd import configs
    cv = configs.smac_rnn_cv_discrete(num_actors=8, agents=1)['config']['central_value_config']
    cv['minibatch_size'] = params['config']['minibatch_size']
    params['config']['central_value_config'] = cv
    params['config']['env_config'].update(state_dim=21, agents=1)
    params['config']['normalize_value'] = True
    return params


@pytest.mark.parametrize('central_value', [False, True], ids=['own_critic', 'recurrent_central_value'])
def test_step_graphs_replay_the_eager_rollout(central_value):
    """Three training epochs with the step graphs on and off, 8 envs: every rollout tensor, the generator and the four
    live and kept states bit-identical.  Once with a recurrent central value critic behind the pair."""
    out = {}
    for graphs in (True, False):
        params = _params('lstm', 64, True, num_actors=8, horizon=8, minibatch_size=32, rollout_graphs=graphs)
        if central_value:
            params = _with_recurrent_critic(params)
        agent, batches = _recording_agent(params)
        assert agent._rnn_pair is not None and agent._engine is None and agent._fast_rollout_ok()
        assert agent.has_central_value == central_value
        if central_value:
            assert agent.central_value_net._rnn_engine is not None
        res = _run_epochs(agent, 3)
        assert len(agent._rollout_graphs) == (agent.horizon_length if graphs else 0)
        assert all(torch.isfinite(torch.stack(list(x))).all() for r in res for x in r[4:6])
        assert len(agent.rnn_states) == 4 and all(s.abs().max() > 0 for s in agent.rnn_states)
        out[graphs] = batches
    assert len(out[True]) == 3
    for a, b in zip(out[True], out[False]):
        assert a.keys() == b.keys() and ('cv_rnn_states0' in a) == central_value
        for k in a:
            assert torch.equal(a[k], b[k]), k
    # the optimiser moved the weights between the epochs, and the replayed steps saw them
    assert not torch.equal(out[True][1]['mus'], out[True][2]['mus'])


def test_replayed_rollout_sees_new_weights():
    """New weights between epochs: the next rollout, replayed from graphs captured for the old weights, equals a fresh
    agent's eager rollout from the same weights, observations, states and seed."""
    params = _params('gru', 128, False, num_actors=8, horizon=8, minibatch_size=32)
    donor, _ = _recording_agent(params, seed=11)
    _run_epochs(donor, 1)
    trained, got = _recording_agent(params, seed=4)
    _run_epochs(trained, 2)
    assert len(trained._rollout_graphs) == trained.horizon_length
    fresh, ref = _recording_agent(params, seed=5)
    for agent in (trained, fresh):
        agent.set_weights(donor.get_weights())
        agent.vec_env.seed(321)
        agent.obs = agent.env_reset()
        agent.dones = torch.ones_like(agent.dones)
        agent._autoreset_prev_dones = None
        agent.rnn_states = [torch.zeros_like(s) for s in agent.rnn_states]
        agent.set_eval()
        torch.manual_seed(99)
        with torch.no_grad():
            agent.play_steps_rnn()
    assert len(fresh._rollout_graphs) == 0 and fresh._fast_rollout_ok()
    for k in got[-1]:
        assert torch.equal(got[-1][k], ref[-1][k]), k
    assert not torch.equal(got[-1]['mus'], got[-2]['mus'])


# ---- shapes the pair declines --------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', ['concat_input', 'before_mlp', 'two_layers', 'units_256', 'state_sigma',
                                     'manual_lstm_off', 'fused_mlp_off'])
def test_shapes_outside_the_pair_keep_the_torch_path(variant, capsys):
    params = _params('gru', 256 if variant == 'units_256' else 32, num_actors=8, horizon=8, minibatch_size=32)
    if variant in ('concat_input', 'before_mlp'):
        params['network']['rnn'][variant] = True
    elif variant == 'two_layers':
        params['network']['rnn']['layers'] = 2
    elif variant == 'state_sigma':
        params['network']['space']['continuous']['fixed_sigma'] = False
    elif variant == 'manual_lstm_off':
        params['config']['manual_lstm'] = False
    elif variant == 'fused_mlp_off':
        params['config']['fused_mlp'] = False
    agent = _agent(params, seed=7)
    assert 'outside the paired RNN engine' in capsys.readouterr().out
    assert agent.is_rnn and agent._rnn_pair is None and agent._engine is None and not agent._fast_rollout_ok()
    agent.init_tensors()
    agent.obs = agent.env_reset()
    before = {k: v.clone() for k, v in agent.model.state_dict().items()}
    res = _run_epochs(agent, 1)[0]
    assert not agent._rollout_graphs
    assert all(torch.isfinite(torch.stack(list(x))).all() for x in res[4:6])
    assert any(not torch.equal(v, before[k]) for k, v in agent.model.state_dict().items() if 'rnn' in k)


# ---- new recordings: the lunar shape and a wide GRU with layer norm ------------------------------------------------

def _engine_golden():
    from conftest import GOLDEN_DIR
    path = os.path.join(GOLDEN_DIR, 'separate_rnn_engine.pt.gz')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_separate_rnn_engine_golden',
                                                  os.path.join(GOLDEN_DIR, 'make_separate_rnn_engine_golden.py'))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)                          # (expand(): the compact forms of the big matrices)
    with gzip.open(path, 'rb') as f:
        raw = torch.load(io.BytesIO(f.read()), map_location='cpu', weights_only=False)
    return {name: maker.expand(cap) for name, cap in raw.items()}


@pytest.mark.parametrize('variant', ['lstm64', 'gru128_ln'])
def test_pair_matches_the_reference_epoch_at_kernel_widths(variant):
    """tests/golden/separate_rnn_engine.pt.gz (make_separate_rnn_engine_golden.py): one train_epoch of the real
    reference A2CAgent at the lunar shape - `lstm64` - and with GRU 128 + layer norm - `gru128_ln` -, 16 envs x horizon
    16 in sequences of 4 with next-step autoreset, 8 optimiser steps; the quantities and tolerances of
    test_pair_matches_the_recorded_reference_epoch."""
    cap = _engine_golden()[variant]
    agent = _recorded_agent(cap)
    net = agent.model.a2c_network
    assert agent._rnn_pair is not None and agent._engine is None and agent._rnn_pair.paired
    assert (net.rnn_name, net.rnn_units, net.rnn_ln) == (('lstm', 64, False) if variant == 'lstm64' else ('gru', 128, True))
    assert (agent.num_actors, agent.horizon_length, agent.seq_length, agent.minibatch_size) == (16, 16, 4, 128)
    assert cap['batch']['rnn_masks'].min() == 0
    rows, kls = _replay(agent, cap)
    assert rows.shape[0] == 8
    _assert_epoch(agent, cap, rows, kls)
