"""GPU: `network.normalization: layer_norm` trunks of the discrete agent and of a feed-forward central value critic on
the fused chain kernels of csrc/mlp_chain_ln.hip (chain_net.ChainNet over ops.MlpChainLn): the 'chains' actor path and the
fused rollout instead of the "outside the fused chain kernels" notice, and - at learning rate 0, against a second agent
with the same weights on `fused_mlp: False` (torch modules + autograd) - the rollout's values and neglogpacs, one
minibatch's losses and every gradient, the layer norms' weight and bias included: each tensor to 1e-5 of its largest
magnitude (_close), the loss scalars to rtol 1e-5."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NOTICE = 'outside the fused chain kernels'


def _params(separate, multi, critic=False, **over):
    from rl_games_amd import configs
    params = configs.cartpole_discrete(num_actors=24, device=DEV, normalize_input=True, normalize_value=True,
                                       horizon_length=8, minibatch_size=96, learning_rate=0.0, grad_norm=1e9, **over)
    net = params['network']
    net.update(separate=separate, normalization='layer_norm')
    net['mlp'].update(units=[64, 36], activation='relu')
    env = params['config']['env_config']
    env.update(obs_dim=33, discrete_actions=6, autoreset_mode='same_step')
    if multi:                                   # SMAC-like: multi-discrete heads with action masks
        net['space'] = {'multi_discrete': None}
        params['model']['name'] = 'multi_discrete_a2c'
        params['config']['use_action_masks'] = True
        env.update(discrete_actions=[3, 5, 2], action_masks=True)
    if critic:
        env.update(state_dim=13)
        params['config']['central_value_config'] = {
            'minibatch_size': 96, 'mini_epochs': 1, 'learning_rate': 0.0, 'clip_value': True, 'normalize_input': True,
            'truncate_grads': True, 'grad_norm': 1e9,
            'network': {'name': 'actor_critic', 'central_value': True, 'normalization': 'layer_norm',
                        'mlp': {'units': [64, 36], 'activation': 'relu', 'initializer': {'name': 'default'}}}}
    return params


def _agent(params):
    from rl_games_amd.discrete_agent import DiscreteA2CAgent
    torch.manual_seed(3)
    agent = DiscreteA2CAgent('chain_ln', copy.deepcopy(params))
    agent.init_tensors()
    return agent


def _rollout(agent):
    agent.obs = agent.env_reset()
    agent.set_eval()
    with torch.no_grad():
        return agent.play_steps()


def _close(name, have, want):
    """The second term of tests/test_chain_ln_gpu.py's rule, with the torch agent in fp32 as the reference: the largest
    difference is at most 1e-5 of the tensor's largest magnitude."""
    diff, scale = (have - want).abs().max().item(), want.abs().max().item()
    print(name, 'max |diff|', diff, 'scale', scale)
    assert diff <= 1e-5 * scale, (name, diff, scale)


def _close_grads(g1, g2):
    for n in g2:
        _close(n, g1[n], g2[n])


@pytest.mark.parametrize('separate,multi', [(False, True), (True, False)])
def test_layer_norm_trunk_runs_on_the_chain_kernels(separate, multi, capsys):
    from rl_games_amd import ops
    a1 = _agent(_params(separate, multi))
    assert NOTICE not in capsys.readouterr().out
    assert a1._path.kind == 'chains' and len(a1._chains) == (2 if separate else 1)
    assert all(c.normed and isinstance(c.chain, ops.MlpChainLn) for c in a1._chains)
    assert a1._fast_rollout_ok()
    a2 = _agent(_params(separate, multi, fused_mlp=False))
    assert a2._chains is None
    a2.model.load_state_dict(a1.model.state_dict())
    batch = _rollout(a1)
    a2.set_eval()
    with torch.no_grad():
        inp = {'is_train': True, 'obs': batch['obses'], 'prev_actions': batch['actions']}
        if multi:
            inp['action_masks'] = batch['action_masks']
        res = a2.model(inp)
    _close('values', batch['values'], a2.model.denorm_value(res['values']))
    _close('neglogpacs', batch['neglogpacs'], res['prev_neglogp'])
    snapshot = {k: v.detach().clone() for k, v in a1.model.state_dict().items()}
    grads = []
    for ag in (a1, a2):
        ag.model.load_state_dict(snapshot)
        ag.set_train()
        ag.prepare_dataset({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'})
        out = ag.train_actor_critic(ag.dataset[1])
        grads.append({n: p.grad.detach().clone() for n, p in ag.model.named_parameters()})
        grads[-1]['_scalars'] = torch.stack(list(out[:4]))
    g1, g2 = grads
    assert all(c.last_dw_path == 'mfma' for c in a1._chains)
    assert torch.allclose(g1.pop('_scalars'), g2.pop('_scalars'), rtol=1e-5, atol=1e-7)
    assert sum('actor_mlp' in n and g2[n].dim() == 1 and g2[n].numel() in (64, 36) for n in g2) == 6      # 2 biases + 2 norms x 2
    _close_grads(g1, g2)


def test_layer_norm_trunk_plays_on_the_fused_play_path(tmp_path):
    """tests/test_player_fused_gpu.py's comparison for this network: the fused player (`player.fused: True`) is on the
    'chains' path over ops.MlpChainLn and picks the torch player's deterministic masked actions wherever the torch
    path's top two normalised logits lie more than 1e-5 apart."""
    from test_player_fused_gpu import ENVS, _act, _inputs, _player, _top_two_gap
    from rl_games_amd import ops
    params = _params(False, True)
    path = _agent(params).save(str(tmp_path / 'ckpt'))
    torch_player, fused_player = _player(params, path, False), _player(params, path, True)
    assert torch_player._fused is None and fused_player._fused.path.kind == 'chains'
    assert isinstance(fused_player._fused.path.chains[0].chain, ops.MlpChainLn)
    steps, sizes = _inputs(params, 31)
    for k, (obs, masks, _) in enumerate(steps[:3]):
        got = _act(fused_player, obs, masks, True)
        res = torch_player._forward(obs, action_masks=masks)
        want = torch_player._pick(res, True)
        clear = _top_two_gap(res['logits'], masks, sizes) > 1e-5
        assert clear.sum() >= 0.98 * ENVS and torch.equal(got[clear], want[clear]), k


def test_layer_norm_central_value_critic_runs_on_the_chain_kernels(capsys):
    a1 = _agent(_params(False, False, critic=True))
    assert NOTICE not in capsys.readouterr().out
    cv1 = a1.central_value_net
    assert cv1._engine is not None and cv1._engine.normed and a1._fast_rollout_ok()
    p2 = _params(False, False, critic=True)
    p2['config']['central_value_config']['fused_mlp'] = False
    a2 = _agent(p2)
    cv2 = a2.central_value_net
    assert cv2._engine is None and NOTICE not in capsys.readouterr().out
    a2.model.load_state_dict(a1.model.state_dict())
    cv2.load_state_dict(cv1.state_dict())
    batch = _rollout(a1)                           # the fused rollout step takes the critic's value from its chain
    _close('values', batch['values'], cv2.get_value({'states': batch['states']}))
    out = []
    for ag in (a1, a2):
        ag.set_train()
        ag.prepare_dataset({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items() if k != '_fused'})
        cv = ag.central_value_net
        loss = cv.train_critic(cv.dataset[0]).clone()
        out.append((loss, {n: p.grad.detach().clone() for n, p in cv.model.named_parameters()}))
    assert torch.allclose(out[0][0], out[1][0], rtol=1e-5, atol=1e-7)
    assert any('actor_mlp.2.weight' in n for n in out[1][1])                # the first layer norm
    _close_grads(out[0][1], out[1][1])
