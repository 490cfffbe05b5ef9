"""GPU: recurrent discrete policies on chain_net.RecurrentChainNet - the trunk + gate-input product as one fused chain
launch, the sequence-persistent LSTM / GRU kernels, the layer norm behind the RNN (csrc/rnn_layer_norm.hip), [value |
logits] heads - in the update (hand-written BPTT against torch autograd) and in the fused, captured rollout; one epoch of
the real reference agent at SMAC widths (tests/golden/discrete_rnn_wide.pt.gz, written by
tests/golden/make_discrete_rnn_wide_golden.py)."""
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
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    torch.manual_seed(seed)
    return DiscreteA2CAgent('test', copy.deepcopy(params))


def _allowed(actions, masks, sizes):
    """Every sub-action of actions [rows(, branches)] is allowed by masks [rows, sum(sizes)]."""
    acts = actions.reshape(actions.shape[0], len(sizes))
    at = 0
    for b, n in enumerate(sizes):
        if not masks.gather(1, (acts[:, b] + at).view(-1, 1)).all():
            return False
        at += n
    return True


@pytest.mark.parametrize('cell,units,layer_norm,actions', [('lstm', 64, False, 5), ('lstm', 128, True, [3, 4]),
                                                          ('gru', 128, False, [3, 4]), ('gru', 32, True, 5)])
def test_recurrent_engine_matches_autograd_gradients_and_rollout(cell, units, layer_norm, actions):
    """test_gru_engine_matches_autograd_gradients_and_rollout for the discrete agent: 24 envs x horizon 8 in sequences of
    4 (24 sequences a minibatch: one and a half of the kernels' 16-sequence tiles), next_step autoreset with p_done 0.2
    (filler rows, rnn_masks, resets inside the sequences).  (i) the engine's rollout (T = 1 launches) leaves the values
    and neglogpacs the torch model gives step by step for the stored actions; (ii) for one minibatch the hand-written
    BPTT produces autograd's scalars and gradients, layer-norm weight and bias included."""
    from rl_games_amd import configs
    multi = isinstance(actions, list)
    sizes = actions if multi else [actions]
    base = configs.smac_rnn_discrete(num_actors=24, cell=cell, units=units, layer_norm=layer_norm, actions=actions,
                                     horizon_length=8, seq_length=4, minibatch_size=96, learning_rate=0.0, grad_norm=1e9,
                                     use_action_masks=multi)
    base['config']['env_config'].update(p_done=0.2, autoreset_mode='next_step', action_masks=multi)
    a1 = _agent(base)
    p2 = copy.deepcopy(base)
    p2['config']['manual_lstm'] = False
    a2 = _agent(p2)
    assert a1._rnn_engine is not None and a2._rnn_engine is None and a1._chains is None and a2._chains is None
    net = a1.model.a2c_network
    assert (net.rnn_name, net.rnn_units, net.rnn_ln) == (cell, units, layer_norm)
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
    obs = batch['obses'].reshape(N, Hz, -1)
    acts = batch['actions'].reshape(N, Hz, -1)
    masks = batch['action_masks'].reshape(N, Hz, -1) if multi else None
    values, nlp = batch['values'].reshape(N, Hz, 1), batch['neglogpacs'].reshape(N, Hz)
    dones = a1.experience_buffer.tensor_dict['dones']     # [Hz, N]: the flags entering each step
    if multi:
        assert _allowed(batch['actions'], batch['action_masks'], sizes)
    with torch.no_grad():
        assert len(batch['rnn_states']) == (2 if cell == 'lstm' else 1)
        st = [s[:, ::Hz // T].contiguous() for s in batch['rnn_states']]      # states at t = 0 (first sequence of each env)
        assert st[0].shape == (1, N, units)
        for t in range(Hz):
            if t > 0:
                # play_steps_rnn zeroes the states of the episodes that ended in step t - 1 (flags of step t) and those a
                # filler row left in step t - 1 (flags of step t - 1; the flags the first rollout starts with - all set -
                # mark no filler rows)
                keep = 1.0 - dones[t].float()
                if t > 1:
                    keep = keep * (1.0 - dones[t - 1].float())
                keep = keep.reshape(1, -1, 1)
                st = [s * keep for s in st]
            inp = {'is_train': True, 'obs': obs[:, t], 'rnn_states': st, 'prev_actions': acts[:, t]}
            if multi:
                inp['action_masks'] = masks[:, t]
            res = a2.model(inp)
            st = res['rnn_states']
            assert torch.allclose(a2.model.denorm_value(res['values']), values[:, t], rtol=1e-4, atol=2e-5), t
            assert torch.allclose(res['prev_neglogp'], nlp[:, t], rtol=1e-4, atol=2e-6), t
    snapshot = {k: v.detach().clone() for k, v in a1.model.state_dict().items()}
    grads = []
    for ag in (a1, a2):
        b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'}
        ag.model.load_state_dict(snapshot)
        ag.set_train()
        ag.prepare_dataset(b)
        ag.train_actor_critic(ag.dataset[1])
        grads.append({n: p.grad.detach().clone() for n, p in ag.model.named_parameters()})
        grads[-1]['_scalars'] = torch.stack(list(ag.train_result[:4]))
    g1, g2 = grads
    if units >= 64:
        assert a1._rnn_engine.last_dw_path == 'mfma'
    print('scalars', g1['_scalars'].tolist(), g2['_scalars'].tolist())
    assert torch.allclose(g1.pop('_scalars'), g2.pop('_scalars'), rtol=1e-5, atol=1e-7)
    assert any('layer_norm' in n for n in g2) == layer_norm
    for n in g2:
        scale = g2[n].abs().max().item() + 1e-12
        print(n, 'max |diff|', (g1[n] - g2[n]).abs().max().item(), 'scale', scale)
        assert torch.allclose(g1[n], g2[n], rtol=1e-4, atol=5e-6 * scale), (n, (g1[n] - g2[n]).abs().max().item(), scale)


def _epochs(params, n):
    agent = _agent(params, seed=7)
    agent.init_tensors()
    agent.obs = agent.env_reset()
    before = {k: v.clone() for k, v in agent.model.state_dict().items()}
    losses = []
    for _ in range(n):
        agent.epoch_num += 1
        res = agent.train_epoch()
        losses.append([torch.stack(list(x)).cpu() for x in res[4:8]])      # a, c, entropy per minibatch; KL per mini-epoch
    return agent, before, losses


@pytest.mark.parametrize('cell,layer_norm', [('lstm', True), ('gru', False)])
def test_recurrent_discrete_epochs_run_fused_and_captured(cell, layer_norm):
    """Three epochs of configs.smac_rnn_discrete at 128 units: the rollout runs fused, its steps are replayed as HIP
    graphs from the second epoch on, losses and states stay finite, the RNN, layer-norm and logits weights move.  The
    same seed without rollout graphs gives the first epoch's losses bit for bit."""
    from rl_games_amd import configs
    params = configs.smac_rnn_discrete(num_actors=32, cell=cell, units=128, layer_norm=layer_norm)
    agent, before, losses = _epochs(params, 3)
    assert agent._rnn_engine is not None and agent._chains is None and agent._fast_rollout_ok()
    assert len(agent._rollout_graphs) == agent.horizon_length
    assert all(torch.isfinite(x).all() for l in losses for x in l)
    assert all(torch.isfinite(s).all() and s.abs().max() > 0 for s in agent.rnn_states)
    vd = agent.dataset.values_dict
    assert _allowed(vd['actions'], vd['action_masks'], agent.branch_sizes)
    moved = [k for k, v in agent.model.state_dict().items() if not torch.equal(v, before[k])]
    wanted = ['rnn.rnn.weight_hh', 'rnn.rnn.weight_ih', 'logits', 'actor_mlp'] + (['layer_norm.weight', 'layer_norm.bias'] if layer_norm else [])
    for part in wanted:
        assert any(part in k for k in moved), part
    p2 = copy.deepcopy(params)
    p2['config']['rollout_graphs'] = False
    agent2, _, losses2 = _epochs(p2, 1)
    assert agent2._fast_rollout_ok() and not agent2._rollout_graphs
    assert all(torch.equal(x, y) for x, y in zip(losses[0], losses2[0]))


@pytest.mark.parametrize('variant', ['separate', 'before_mlp', 'two_layers', 'units_256', 'manual_lstm_off', 'fused_mlp_off'])
def test_networks_outside_the_recurrent_engine_keep_the_torch_path(variant):
    from rl_games_amd import configs
    params = configs.smac_rnn_discrete(num_actors=8, cell='gru', units=256 if variant == 'units_256' else 32,
                                       horizon_length=8, minibatch_size=32)
    if variant == 'separate':
        params['network']['separate'] = True
    elif variant == 'before_mlp':
        params['network']['rnn']['before_mlp'] = True
    elif variant == 'two_layers':
        params['network']['rnn']['layers'] = 2
    elif variant == 'manual_lstm_off':
        params['config']['manual_lstm'] = False
    elif variant == 'fused_mlp_off':
        params['config']['fused_mlp'] = False
    agent, before, losses = _epochs(params, 1)
    assert agent.is_rnn and agent._rnn_engine is None and agent._chains is None and not agent._fast_rollout_ok()
    assert all(torch.isfinite(x).all() for x in losses[0])
    assert any(not torch.equal(v, before[k]) for k, v in agent.model.state_dict().items() if 'rnn' in k)


# ---- one epoch of the real reference agent at SMAC widths ----------------------------------------------------------

def _golden():
    from conftest import GOLDEN_DIR
    with gzip.open(os.path.join(GOLDEN_DIR, 'discrete_rnn_wide.pt.gz'), 'rb') as f:
        return torch.load(io.BytesIO(f.read()), map_location='cpu', weights_only=False)


@pytest.mark.parametrize('variant', ['gru128_multi_masked', 'lstm64_ln_masked'])
def test_recurrent_engine_matches_reference_epoch(variant):
    """The reference agent's rollout batch (16 envs x horizon 16, sequences of 8, minibatch 64, 2 mini-epochs = 8
    optimiser steps) through this agent's dataset preparation and every minibatch step on the engine, as
    tests/test_discrete_gpu.py::test_discrete_update_matches_reference_epoch replays it.  Scalars: the criterion of
    tests/test_gru_gpu.py::_check_against_truth (plain bounds rtol 1e-5 + 2e-6, KL 1e-4; an entry outside them at most
    1.5 x as far from the recorded fp64 trajectory as the recorded fp32 reference; never beyond 1e-3 of the scale); the
    learning rates exactly; the final parameters at rtol 1e-4 / atol 2e-6."""
    from test_gru_gpu import _check_against_truth
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    cap = _golden()[variant]
    params = copy.deepcopy(cap['params'])
    params['config'].update(device=DEV)
    env = SyntheticTensorEnv(cap['num_envs'], device=DEV, **params['config']['env_config'])
    params['config']['vec_env'] = env
    params['config']['env_info'] = env.get_env_info()
    agent = DiscreteA2CAgent('test', params)
    agent.init_tensors()
    assert agent._rnn_engine is not None and agent._chains is None
    assert (agent.num_actors, agent.horizon_length, agent.seq_length, agent.minibatch_size) == (16, 16, 8, 64)
    agent.model.load_state_dict(cap['state_after_rollout'])
    batch = {k: ([s.to(DEV) for s in v] if isinstance(v, (list, tuple)) else v.to(DEV)) for k, v in cap['batch'].items()}
    agent.set_train()
    agent.epoch_num = 1
    agent.prepare_dataset(batch)
    rows, lrs, kls = [], [], []
    for mini_ep in range(agent.mini_epochs_num):
        first = len(rows)
        for i in range(len(agent.dataset)):
            a, c, e, kl, lr, lr_mul = agent.train_actor_critic(agent.dataset[i])
            rows.append(torch.stack([a, c, e, kl]).clone())
        av_kl = torch.stack([r[3] for r in rows[first:]]).mean()
        kls.append(av_kl)
        agent._host_schedule(float(av_kl.item()))          # what train_epoch does per mini-epoch
        lrs.append(agent._host_lr)
        if agent.normalize_input:
            agent.model.running_mean_std.eval()
    rows = torch.stack(rows).cpu()
    assert rows.shape[0] == 8
    needed = {}
    for col, (key, name) in enumerate((('a_loss', 'a_losses'), ('c_loss', 'c_losses'), ('entropy', 'entropies'))):
        needed[key] = _check_against_truth(rows[:, col], cap[name].reshape(-1), cap['truth_' + name].reshape(-1), key)
    needed['kl'] = _check_against_truth(torch.stack(kls).cpu(), cap['mini_epoch_kls'].reshape(-1),
                                        cap['truth_mini_epoch_kls'].reshape(-1), 'kl')
    print('entries that needed the fp64 yardstick:', needed)
    assert lrs == cap['lrs']
    final = agent.model.state_dict()
    for k, v in cap['final_state'].items():
        tol = dict(rtol=1e-4, atol=2e-6) if v.is_floating_point() else dict(rtol=0, atol=0)
        assert torch.allclose(final[k].cpu().to(v.dtype), v, **tol), (k, (final[k].cpu().to(v.dtype) - v).abs().max().item())
