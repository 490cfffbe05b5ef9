"""CPU: actor_paths.Plan's opt-in branch for continuous policies with a sigma head (`sigma_head_kernels: True`) - which
networks it sends to SigmaPath, which it declines with a notice and the arena order they always had - with the engine
replaced by a recorder, and ops.sigma_form.  No kernel runs."""
import types

import numpy as np
import pytest

from rl_games_amd import actor_paths, configs, ops
from rl_games_amd.policy import ActorCriticNetwork, ContinuousA2CLogStdModel

ON = {'sigma_head_kernels': True}


def _agent(value_size=1, space=(), obs_dtype=np.float32, **extra):
    net_over = {k: extra.pop(k) for k in list(extra) if k != 'trains'}
    net_params = configs.pendulum_sigma_head(units=(32, 16), sigma_parametrization='softplus', min_sigma=0.05)['network']
    net_params['space']['continuous'].update(space)
    net_params.update(net_over)
    net = ActorCriticNetwork(net_params, 3, (9,), value_size=value_size)
    model = ContinuousA2CLogStdModel(net, (9,), False, True, value_size)
    return types.SimpleNamespace(model=model, is_discrete=False, value_size=value_size, is_rnn=net.is_rnn(), optimizer='arena',
                                 minibatch_size=64, num_actors=8, num_agents=1, ppo_device='cpu',
                                 observation_space=types.SimpleNamespace(dtype=obs_dtype), **extra)


def test_plan_without_the_key_is_what_it_was():
    plan = actor_paths.Plan(_agent(), {})
    assert plan.cls is None and plan.notice is None and plan.layout is None and plan.fallback is actor_paths.GeneralPath


def test_plan_sends_an_eligible_sigma_head_to_the_sigma_path(monkeypatch):
    built = []
    monkeypatch.setattr(actor_paths, 'ChainNet', lambda *a, **kw: built.append((a, kw)) or types.SimpleNamespace())
    agent = _agent()
    net = agent.model.a2c_network
    plan = actor_paths.Plan(agent, ON)
    assert plan.cls is actor_paths.SigmaPath and plan.why is None
    n_mat = sum(p.dim() == 2 for p in net.parameters())
    assert all(a is b for a, b in zip(plan.layout[n_mat - 3:n_mat], (net.value.weight, net.mu.weight, net.sigma.weight)))
    assert all(a is b for a, b in zip(plan.layout[-3:], (net.value.bias, net.mu.bias, net.sigma.bias)))
    path = plan.build(agent)
    assert path.kind == 'sigma' and path.row_sigma and path.engines == [path.chain]
    assert path.form == dict(sigma_kind=1, has_bounds=0, sigma_lo=0.0, sigma_hi=0.0, min_sigma=pytest.approx(0.05))
    (args, kw), = built
    assert args[0] is net.actor_mlp and args[1] == [net.value, net.mu, net.sigma] and kw == {'infer_rows': 8}


@pytest.mark.parametrize('why,value_size,net_over', [
    ('a shared trunk only', 1, {'separate': True}),
    ('feed-forward networks only', 1, {'rnn': {'name': 'lstm', 'units': 16, 'layers': 1}}),
    ('one value column only', 2, {}),
    ('plain Linear + activation trunks only', 1, {'normalization': 'layer_norm'}),
    ('identity head activations only', 1, {'space': {'mu_activation': 'tanh'}}),
    ('fp32 observation spaces only', 1, {'obs_dtype': np.uint8})])
def test_plan_declines_with_a_notice_and_the_arena_order_as_it_was(why, value_size, net_over, capsys):
    plan = actor_paths.Plan(_agent(value_size, **net_over), ON)
    assert plan.cls is actor_paths.SigmaPath and plan.why == why and plan.layout is None
    assert plan.build(types.SimpleNamespace()).kind == 'general'
    assert f'rl_games_amd: sigma head outside the sigma-head kernels ({why}); using autograd' in capsys.readouterr().out


def test_a_player_is_not_offered_the_sigma_path_and_declines_as_before(capsys):
    from rl_games_amd.play_engine import FusedPlay, _PlayAgent
    assert _PlayAgent.trains is False
    plan = actor_paths.Plan(_agent(trains=False), ON)
    assert plan.cls is None and plan.layout is None and plan.fallback is actor_paths.GeneralPath
    model = _agent().model
    player = types.SimpleNamespace(model=model, config=ON, value_size=1, is_rnn=False, normalize_input=True, observation_space=None)
    assert FusedPlay(player, 8).declined == 'a log sigma vector and one value column only'
    assert 'a log sigma vector and one value column only' in capsys.readouterr().out


@pytest.mark.parametrize('net,want', [
    (dict(sigma_parametrization='exp'), (0, 0, 0.0, 0.0, 0.0)),
    (dict(sigma_parametrization='exp', logstd_bounds=(-1.0, 0.5), min_sigma=0.25), (0, 1, -1.0, 0.5, 0.25)),
    (dict(sigma_parametrization='softplus', logstd_bounds=(-1.0, 0.5), min_sigma=0.5), (1, 0, 0.0, 0.0, 0.5)),
    (dict(sigma_parametrization='linear', min_sigma=0.125), (2, 0, 0.0, 0.0, 0.125)),
    (dict(sigma_parametrization='scalar'), (2, 0, 0.0, 0.0, 0.0))])
def test_sigma_form_of_each_parametrisation(net, want):
    form = ops.sigma_form(types.SimpleNamespace(**net))
    assert tuple(form[k] for k in ('sigma_kind', 'has_bounds', 'sigma_lo', 'sigma_hi', 'min_sigma')) == want
    assert ops.sigma_form(net) == form
