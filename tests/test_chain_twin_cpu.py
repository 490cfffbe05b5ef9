"""CPU: actor_paths.Plan's branch for continuous policies with separate actor / critic MLPs - which networks it sends to
TwinPath and which keep the route they had - with the engine replaced by a recorder.  No kernel runs."""
import types

import pytest
import torch

from rl_games_amd import actor_paths, configs
from rl_games_amd.policy import ActorCriticNetwork, ContinuousA2CLogStdModel


def _agent(value_size=1, **net_over):
    net_params = configs.mujoco_separate_mlp(units=(32, 16), critic_units=(16,))['network']
    for k, v in net_over.items():
        if isinstance(v, dict) and isinstance(net_params.get(k), dict):
            net_params[k].update(v)
        else:
            net_params[k] = v
    net = ActorCriticNetwork(net_params, 3, (9,), value_size=value_size)
    model = ContinuousA2CLogStdModel(net, (9,), False, True, value_size)
    return types.SimpleNamespace(model=model, is_discrete=False, value_size=value_size, is_rnn=net.is_rnn(), optimizer='arena',
                                 minibatch_size=64, num_actors=8, num_agents=1)


def test_plan_sends_plain_separate_trunks_to_the_twin_path_with_its_arena_order(monkeypatch):
    built = []
    monkeypatch.setattr(actor_paths, 'TwinChainNet', lambda *a, **kw: built.append((a, kw)) or types.SimpleNamespace())
    agent = _agent()
    net = agent.model.a2c_network
    plan = actor_paths.Plan(agent, {})
    assert plan.cls is actor_paths.TwinPath and plan.why is None
    n_mat = sum(p.dim() == 2 for p in net.parameters())
    assert [p.dim() for p in plan.layout[:n_mat]] == [2] * n_mat                       # the matrices first ...
    assert plan.layout[n_mat - 2] is net.mu.weight and plan.layout[n_mat - 1] is net.value.weight
    biases = [m.bias for t in (net.actor_mlp, net.critic_mlp) for m in t if isinstance(m, torch.nn.Linear)]
    assert all(a is b for a, b in zip(plan.layout[n_mat:], biases))                    # ... the trunks' biases behind them
    assert plan.layout[-2] is net.mu.bias and plan.layout[-1] is net.value.bias        # ... the head biases last
    path = plan.build(agent)
    assert path.kind == 'twin' and path.engines == [path.twin] and path.twin.head_bias_done
    (args, kw), = built
    assert args[:6] == (net.actor_mlp, net.mu, net.critic_mlp, net.value, 'arena', 64) and kw == {'infer_rows': 8}


@pytest.mark.parametrize('name,config,net_over,value_size', [
    ('rnn', {}, {'rnn': {'name': 'lstm', 'units': 16, 'layers': 1}}, 1),
    ('general: two value columns', {}, {}, 2),
    ('general: a sigma head', {}, {'space': {'continuous': dict(configs._network([8])['space']['continuous'], fixed_sigma=False)}}, 1),
    ('fused_mlp off', {'fused_mlp': False}, {}, 1),
    ('manual_mlp off', {'manual_mlp': False}, {}, 1),
    ('layer norm', {}, {'normalization': 'layer_norm'}, 1),
    ('shared trunk', {}, {'separate': False}, 1)])
def test_plan_keeps_every_other_network_on_its_route(name, config, net_over, value_size):
    if name == 'rnn':
        net_over = dict(net_over, mlp={'critic_units': None})
    plan = actor_paths.Plan(_agent(value_size, **net_over), config)
    assert plan.cls is not actor_paths.TwinPath
    if name in ('fused_mlp off', 'layer norm') or name.startswith('general'):
        assert plan.cls is None and plan.notice is None and plan.layout is None          # autograd (general), silently, as ever


def test_plan_declines_in_front_of_the_optimiser_and_an_engine_may_still_refuse(monkeypatch, capsys):
    plan = actor_paths.Plan(_agent(mlp={'units': [18], 'critic_units': None}), {})
    assert plan.cls is actor_paths.TwinPath and 'multiples of 4' in plan.why and plan.layout is None
    assert plan.build(types.SimpleNamespace()).kind == 'autograd'
    assert 'separate MLP trunks outside the twin chain kernel (hidden widths must be multiples of 4); using autograd' in capsys.readouterr().out

    def refuse(*a, **kw):
        raise NotImplementedError('no LDS')
    monkeypatch.setattr(actor_paths, 'TwinChainNet', refuse)
    agent = _agent()
    assert actor_paths.Plan(agent, {}).build(agent).kind == 'autograd'
    assert 'twin chain kernel (no LDS); using autograd' in capsys.readouterr().out
