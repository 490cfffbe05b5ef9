"""GPU: a continuous policy with a sigma head and `sigma_head_kernels: True` runs on actor_paths.SigmaPath (one ChainNet over
[value | mu | raw sigma], csrc/ppo_loss_sigma.hip) - and, at learning rate 0, agrees with a second agent with the same
weights and the key off (GeneralPath: torch modules, torch_fallback.ppo_loss under autograd): a fused rollout against the
model's own forward, then one minibatch's five loss scalars and every gradient by parameter name (the arena layouts
differ), each tensor to 1e-5 of its largest magnitude (tests/test_chain_ln_agent_gpu.py's figure and helpers)."""
import copy

import pytest
import torch

from test_chain_ln_agent_gpu import _close, _close_grads, _rollout

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _agent(form, key):
    from rl_games_amd import configs
    from rl_games_amd.agent import A2CAgent
    params = configs.pendulum_sigma_head(num_actors=16, units=(32, 16), obs_dim=12, act_dim=3, horizon_length=8,
                                         minibatch_size=128, mini_epochs=1, device=DEV, learning_rate=0.0, grad_norm=1e9,
                                         sigma_head_kernels=key, **form)
    torch.manual_seed(3)
    agent = A2CAgent('sigma_head', copy.deepcopy(params))
    agent.init_tensors()
    return agent


@pytest.mark.parametrize('form', [dict(sigma_parametrization='exp', logstd_bounds=(-1.0, 0.5)),
                                  dict(sigma_parametrization='softplus', min_sigma=0.05)], ids=['exp_bounds', 'softplus_floor'])
def test_sigma_head_policy_runs_on_the_sigma_path_and_agrees_with_autograd(form, capsys):
    a1, a2 = _agent(form, True), _agent(form, False)
    assert 'using autograd' not in capsys.readouterr().out
    assert a1._path.kind == 'sigma' and a1._fast_rollout_ok() and a1._autograd.kind == a2._path.kind == 'general'
    with torch.no_grad():
        a1.model.a2c_network.sigma.weight.normal_(0.0, 0.3)               # a sigma that depends on the row
    a2.model.load_state_dict(a1.model.state_dict())
    batch = _rollout(a1)
    a2.set_eval()
    with torch.no_grad():
        res = a2.model({'is_train': True, 'obs': batch['obses'], 'prev_actions': batch['actions']})
    _close('values', batch['values'], a2.model.denorm_value(res['values']))
    _close('mus', batch['mus'], res['mus'])
    _close('sigmas', batch['sigmas'], res['sigmas'])
    _close('neglogpacs', batch['neglogpacs'], res['prev_neglogp'])
    last = lambda k: a1.experience_buffer.storage[k].view(16, 8, 3)[:, -1]     # the last step: env-major [N][H][A]
    _close('actions', last('actions'), last('mus') + last('sigmas') * a1._roll_noise)
    snapshot = {k: v.detach().clone() for k, v in a1.model.state_dict().items()}
    grads = []
    for ag in (a1, a2):
        ag.model.load_state_dict(snapshot)
        ag.set_train()
        ag.prepare_dataset({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'})
        out = ag.train_actor_critic(ag.dataset[0])
        grads.append({n: p.grad.detach().clone() for n, p in ag.model.named_parameters()})
        grads[-1]['_scalars'] = torch.stack([out[0], out[1], out[2], out[3], out[8]])     # a, c, entropy, kl, b
    g1, g2 = grads
    assert torch.allclose(g1.pop('_scalars'), g2.pop('_scalars'), rtol=1e-5, atol=1e-7)
    assert any('sigma.weight' in n for n in g2) and all(g2[n].abs().max() > 0 for n in g2)
    _close_grads(g1, g2)
