"""GPU: continuous policies with separate actor / critic MLPs and no RNN (configs.mujoco_separate_mlp) on the twin-trunk
chain (actor_paths.TwinPath over chain_net.TwinChainNet, csrc/mlp_chain_twin.hip): the 'twin' path and a graph-replayed
fused rollout instead of silent autograd, and - at learning rate 0, against a second agent from the same seed on
`fused_mlp: False` (torch modules + autograd) - the rollout's mu and values, one minibatch's losses and KL and every
gradient, with the tolerance of tests/test_chain_ln_agent_gpu.py: each tensor to 1e-5 of its largest magnitude, the
scalars to rtol 1e-5."""
import copy

import pytest
import torch

from test_chain_ln_agent_gpu import _close, _close_grads, _rollout

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NOTICE = 'outside the twin chain kernel'


def _agent(num_actors=24, units=(64, 36), critic_units=(32, 16, 8), **over):
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    params = configs.mujoco_separate_mlp(num_actors=num_actors, units=units, critic_units=critic_units, device=DEV,
                                         horizon_length=8, minibatch_size=num_actors * 4, **over)
    torch.manual_seed(3)
    agent = A2CAgent('chain_twin', copy.deepcopy(params))
    agent.init_tensors()
    return agent


def test_separate_mlp_policy_runs_on_the_twin_chain_and_agrees_with_autograd(capsys):
    a1 = _agent(learning_rate=0.0, grad_norm=1e9)
    a2 = _agent(learning_rate=0.0, grad_norm=1e9, fused_mlp=False)
    assert 'using autograd' not in capsys.readouterr().out
    assert a1._path.kind == 'twin' and a1._fast_rollout_ok() and a2._path.kind == 'autograd'
    assert all(torch.equal(p, q) for p, q in zip(a1.model.state_dict().values(), a2.model.state_dict().values()))
    batch = _rollout(a1)
    a2.set_eval()
    with torch.no_grad():
        res = a2.model({'is_train': True, 'obs': batch['obses'], 'prev_actions': batch['actions']})
    _close('values', batch['values'], a2.model.denorm_value(res['values']))
    _close('mus', batch['mus'], res['mus'])
    snapshot = {k: v.detach().clone() for k, v in a1.model.state_dict().items()}
    grads = []
    for ag in (a1, a2):
        ag.model.load_state_dict(snapshot)
        ag.set_train()
        ag.prepare_dataset({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'})
        out = ag.train_actor_critic(ag.dataset[1])
        grads.append({n: p.grad.detach().clone() for n, p in ag.model.named_parameters()})
        grads[-1]['_scalars'] = torch.stack(list(out[:4]))                    # a_loss, c_loss, entropy, kl
    g1, g2 = grads
    assert a1._path.twin.last_dw_path == 'mfma'
    assert torch.allclose(g1.pop('_scalars'), g2.pop('_scalars'), rtol=1e-5, atol=1e-7)
    assert sum('critic_mlp' in n for n in g2) == 6 and sum('actor_mlp' in n for n in g2) == 4
    _close_grads(g1, g2)


@pytest.mark.parametrize('num_actors', [8, 64])
def test_separate_mlp_policy_trains_and_replays_its_rollout(num_actors):
    agent = _agent(num_actors)
    agent.obs = agent.env_reset()
    before = {k: v.clone() for k, v in agent.model.state_dict().items()}
    for _ in range(2):                                       # (the second epoch's rollout is captured and replayed)
        agent.update_epoch()
        res = agent.train_epoch()
    assert len(agent._rollout_graphs) == agent.horizon_length
    assert all(torch.isfinite(torch.stack(list(x))).all() for x in res[4:6])
    after = agent.model.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    for part in ('actor_mlp', 'critic_mlp', 'a2c_network.mu', 'a2c_network.value'):
        assert any(part in k and not torch.equal(v, before[k]) for k, v in after.items()), part


def test_a_hidden_width_of_18_prints_the_notice_and_trains_on_autograd(capsys):
    agent = _agent(units=(18,), critic_units=None)
    assert NOTICE in capsys.readouterr().out and agent._path.kind == 'autograd'
    agent.obs = agent.env_reset()
    agent.update_epoch()
    res = agent.train_epoch()
    assert not agent._rollout_graphs and all(torch.isfinite(torch.stack(list(x))).all() for x in res[4:6])
