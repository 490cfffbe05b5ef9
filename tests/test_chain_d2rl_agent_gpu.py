"""GPU: `mlp.d2rl: True` trunks of the discrete agent and of a feed-forward central value critic on csrc/mlp_chain_d2rl.hip
with `d2rl_kernels: True`: the 'chains' actor path (update and fused rollout), and - against the same agent without the key,
same seed - one train_epoch at learning rate 0: the rollout's actions equal, the observation statistics bit for bit, every
gradient to 1e-5 of its scale (the bar of tests/test_discrete_gpu.py::test_discrete_chain_gradients_equal_autograd)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NOTICE = 'outside the fused chain kernels'


def _agent(key, separate=False, critic=False, normalization=None):
    from rl_games_amd import configs
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    params = configs.discrete_d2rl(num_actors=64, separate=separate, d2rl_kernels=key, device=DEV, horizon_length=8,
                                   minibatch_size=256, learning_rate=0.0, grad_norm=1e9)
    params['network']['normalization'] = normalization
    if critic:
        params['config']['env_config'].update(state_dim=13)
        params['config']['central_value_config'] = {
            'minibatch_size': 256, 'mini_epochs': 1, 'learning_rate': 0.0, 'clip_value': True, 'normalize_input': True,
            'truncate_grads': True, 'grad_norm': 1e9, 'd2rl_kernels': key,
            'network': {'name': 'actor_critic', 'central_value': True,
                        'mlp': {'units': [64, 36], 'activation': 'elu', 'd2rl': True, 'initializer': {'name': 'default'}}}}
    torch.manual_seed(3)
    agent = DiscreteA2CAgent('chain_d2rl', copy.deepcopy(params))
    agent.init_tensors()
    agent.obs = agent.env_reset()
    return agent


def _epoch(agent, model):
    torch.manual_seed(5)
    agent.train_epoch()
    rms = model.running_mean_std
    return (agent.experience_buffer.tensor_dict['actions'].clone(), [t.clone() for t in (rms.running_mean, rms.running_var, rms.count)],
            {n: p.grad.detach().clone() for n, p in model.named_parameters()})


def _same(on, off):
    assert torch.equal(on[0], off[0])                                        # the rollout's actions
    assert all(torch.equal(a, b) for a, b in zip(on[1], off[1]))             # observation statistics, bit for bit
    assert any(g.abs().max().item() > 0 for g in off[2].values())
    for n, want in off[2].items():
        diff, scale = (on[2][n] - want).abs().max().item(), want.abs().max().item()
        print(n, 'max |diff|', diff, 'scale', scale)
        assert diff <= 1e-5 * scale + 1e-9, (n, diff, scale)


@pytest.mark.parametrize('separate', [False, True])
def test_d2rl_trunk_runs_on_the_chain_kernels_with_the_key(separate, capsys):
    from rl_games_amd import ops
    a1 = _agent(True, separate)
    assert NOTICE not in capsys.readouterr().out
    assert a1._path.kind == 'chains' and len(a1._chains) == (2 if separate else 1)
    assert all(c.d2rl and isinstance(c.chain, ops.MlpChainD2rl) for c in a1._chains) and a1._fast_rollout_ok()
    a2 = _agent(False, separate)
    assert a2._path.kind == 'autograd' and a2._chains is None and NOTICE in capsys.readouterr().out
    a2.model.load_state_dict(a1.model.state_dict())
    _same(_epoch(a1, a1.model), _epoch(a2, a2.model))


def test_layer_norm_d2rl_is_declined_with_its_reason(capsys):
    a = _agent(True, normalization='layer_norm')
    out = capsys.readouterr().out
    assert a._path.kind == 'autograd' and NOTICE in out and 'D2RL trunks without layer_norm / batch_norm only' in out


def test_d2rl_central_value_critic_runs_on_the_chain_kernels_with_the_key(capsys):
    from rl_games_amd import ops
    a1 = _agent(True, critic=True)
    assert NOTICE not in capsys.readouterr().out
    cv1 = a1.central_value_net
    assert cv1._engine is not None and isinstance(cv1._engine.chain, ops.MlpChainD2rl) and a1._fast_rollout_ok()
    a2 = _agent(False, critic=True)
    cv2 = a2.central_value_net
    assert cv2._engine is None and a2._path.kind == 'autograd'
    a2.model.load_state_dict(a1.model.state_dict())
    cv2.load_state_dict(cv1.state_dict())
    _same(_epoch(a1, cv1.model), _epoch(a2, cv2.model))
